"""The Predictor sampler and the code-0 repetition penalty on the device (include/q3tts.h, "Predictor sampler and repetition penalty"): ids
against the CPU restatement tests/_pred_sample.py, `==`. tests/test_pred_sample_cpu.py pins the restatement to the oracle and asserts that
a greedy Predictor (or no penalty) cannot pass the sampled cases below."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import _pred_sample as S

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
INVALID, STATE = -1, -5   # Q3TTS_ERR_INVALID, Q3TTS_ERR_STATE


def _engine(cfg):
    from q3tts import native
    return native.NativeEngine(cfg)


@pytest.fixture(scope="module")
def tiny(oracle):
    cfg = S.tiny_cfg(with_vocoder=1)
    eng = _engine(cfg)
    om = oracle.OracleModel(cfg.model, seed=0, n_ctx=S.N_CTX, n_threads=8)
    yield cfg, eng, om, S.mats_from_model(om, False, False), S.prompt(om)
    eng.close()
    om.close()


@pytest.fixture(autouse=True)
def _defaults_after(request):
    yield
    if "tiny" in request.fixturenames:
        eng = request.getfixturevalue("tiny")[1]
        eng.k_pred_variant(0)
        eng.set_predictor_sampler(0.0, 0, 1.0)
        eng.set_repetition_penalty(1.0)


# ---- 1. the three sampler configurations, greedy and sampled Talker -------------------------------------------------------------------
@pytest.mark.parametrize("talker", sorted(S.TALKERS))
@pytest.mark.parametrize("name", sorted(S.PRED_CONFIGS))
def test_ids_equal_the_restatement(tiny, name, talker):
    cfg, eng, om, pred, pe = tiny
    ps = S.PRED_CONFIGS[name]
    ref, _ = S.generate(om, pred, pe, pred_sampler=ps, **S.request(talker))
    eng.set_predictor_sampler(*ps)
    assert eng.predictor_sampler() == pytest.approx(ps)
    got = eng.generate(embd=pe, **S.request(talker))
    assert got.status == 0 and ref.shape[0] == S.FRAMES and np.array_equal(got.codes, ref)
    if name == "top1":   # top_k = 1 is greedy
        eng.set_predictor_sampler(0.0, 0, 1.0)
        assert np.array_equal(eng.generate(embd=pe, **S.request(talker)).codes, ref)


# ---- 2. one engine through both frame-step forms --------------------------------------------------------------------------------------
def _sequence(eng, om, pred, pe):
    """defaults | the sampling form at temperature 0 (sample_row's greedy branch on stored logits) | (0.9, 50, 1.0) | off again"""
    kw = S.request("sampled")
    a = eng.generate(embd=pe, **kw).codes
    eng.k_pred_variant(1)
    b = eng.generate(embd=pe, **kw).codes
    eng.k_pred_variant(0)
    eng.set_predictor_sampler(*S.PRED_CONFIGS["select"])
    c = eng.generate(embd=pe, **kw).codes
    eng.set_predictor_sampler(0.0, 0, 1.0)
    d = eng.generate(embd=pe, **kw).codes
    ref_greedy, _ = om.generate(pe, **kw)
    ref, _ = S.generate(om, pred, pe, pred_sampler=S.PRED_CONFIGS["select"], **kw)
    assert np.array_equal(a, ref_greedy) and np.array_equal(b, a) and np.array_equal(d, a)   # the ARGMAX path and the greedy branch agree
    assert np.array_equal(c, ref) and not np.array_equal(c, a)


def test_switching_between_the_two_graph_sets(tiny):
    cfg, eng, om, pred, pe = tiny
    _sequence(eng, om, pred, pe)


_CHILD = """
import sys
sys.path.insert(0, %r)
import _oracle as O, _pred_sample as S
import test_pred_sample_gpu as T
cfg = S.tiny_cfg()
eng = T._engine(cfg)
om = O.OracleModel(cfg.model, seed=0, n_ctx=S.N_CTX, n_threads=8)
T._sequence(eng, om, S.mats_from_model(om, False, False), S.prompt(om))
eng.close()
print("eager ok")
"""


def test_switching_without_graphs():
    env = dict(os.environ, Q3TTS_NO_GRAPH="1")
    out = subprocess.run([sys.executable, "-c", _CHILD % HERE], env=env, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "eager ok" in out.stdout, out.stdout + out.stderr


# ---- 3. continuous batching: the draw index is positional ----------------------------------------------------------------------------
def test_continuous_batching_equals_one_at_a_time(tiny):
    cfg, eng, om, pred, pe = tiny
    ps = S.PRED_CONFIGS["select"]
    eng.set_predictor_sampler(*ps)
    reqs = S.batch_requests(om)   # 7 requests on 4 slots
    batch = eng.generate_batch(reqs)
    for i, r in enumerate(reqs):
        one = eng.generate(**r)
        assert batch[i].status == 0 and one.codes.shape[0] == r["min_frames"] and np.array_equal(batch[i].codes, one.codes), i
    ref, _ = S.generate(om, pred, reqs[1]["embd"], pred_sampler=ps, **{k: v for k, v in reqs[1].items() if k != "embd"})
    assert np.array_equal(batch[1].codes, ref)


# ---- 4. a 2048-wide head: NP = 2048 and 16 candidates per thread in the select path ---------------------------------------------------
def test_wide_codebook(oracle):
    cfg = S.tiny_cfg(wide=True)
    eng = _engine(cfg)
    om = oracle.OracleModel(cfg.model, seed=0, n_ctx=S.N_CTX, n_threads=8)
    try:
        pred, pe = S.mats_from_model(om, False, False), S.prompt(om)
        for name in ("select", "sort_top_p"):
            ps = S.PRED_CONFIGS[name]
            ref, _ = S.generate(om, pred, pe, pred_sampler=ps, **S.request("sampled", 4))
            eng.set_predictor_sampler(*ps)
            assert np.array_equal(eng.generate(embd=pe, **S.request("sampled", 4)).codes, ref), name
    finally:
        eng.close()
        om.close()


def test_widest_codebook(oracle):
    """codebook_size = Q3_SAMP_MAX = 4096, the widest head the sampler takes: k_pred_next<true> holds more than 64 KiB of LDS here
    (50 KiB static + the 16 KiB row), the size its kernel attribute is asked for."""
    cfg = S.tiny_cfg(max_batch=2)
    cfg.model.codebook_size = cfg.model.codecq_rows = 4096
    eng = _engine(cfg)
    om = oracle.OracleModel(cfg.model, seed=0, n_ctx=S.N_CTX, n_threads=8)
    try:
        pred, pe = S.mats_from_model(om, False, False), S.prompt(om)
        ps = S.PRED_CONFIGS["select"]
        tr = []
        ref, _ = S.generate(om, pred, pe, pred_sampler=ps, trace=tr, **S.request("sampled", 4))
        diff, n = S.differing(tr)
        assert 4 * diff >= n   # (the input condition: a greedy Predictor cannot pass)
        eng.set_predictor_sampler(*ps)
        assert np.array_equal(eng.generate(embd=pe, **S.request("sampled", 4)).codes, ref)
    finally:
        eng.close()
        om.close()


def test_refused_above_the_samplers_widest_row():
    """codebook_size > Q3_SAMP_MAX: a temperature > 0 is Q3TTS_ERR_INVALID and leaves the state as it was; temperature 0 is still accepted."""
    cfg = S.tiny_cfg(max_batch=1)
    cfg.model.codebook_size = cfg.model.codecq_rows = 8192
    eng = _engine(cfg)
    try:
        assert eng.lib.q3tts_set_predictor_sampler(eng.h, 0.9, 50, 1.0) == INVALID
        assert eng.lib.q3tts_k_pred_variant(eng.h, 1) == INVALID
        assert eng.predictor_sampler() == pytest.approx((0.0, 0, 1.0))
        assert eng.lib.q3tts_set_predictor_sampler(eng.h, 0.0, 50, 0.9) == 0
        assert eng.predictor_sampler() == pytest.approx((0.0, 50, 0.9))
        assert eng.lib.q3tts_set_repetition_penalty(eng.h, 1.1) == 0   # the penalty works on sample_limit, not on codebook_size
    finally:
        eng.close()


# ---- 5. the W8A8 Predictor ------------------------------------------------------------------------------------------------------------
def test_q8_predictor(oracle):
    cfg = S.tiny_cfg(pred_q8=2)
    eng = _engine(cfg)
    om = oracle.OracleModel(cfg.model, seed=0, n_ctx=S.N_CTX, n_threads=8)
    try:
        pred8, pe = S.mats_from_model(om, False, True), S.prompt(om)
        ps = S.PRED_CONFIGS["select"]
        ref, _ = S.generate(om, pred8, pe, pred_sampler=ps, **S.request("sampled", 4))
        eng.set_predictor_sampler(*ps)
        assert np.array_equal(eng.generate(embd=pe, **S.request("sampled", 4)).codes, ref)
        eng.set_predictor_sampler(0.0, 0, 1.0)
        eng.k_pred_variant(1)   # stored logits + the greedy branch against the ARGMAX epilogue of k_bgemm8
        b = eng.generate(embd=pe, **S.request("sampled", 4)).codes
        eng.k_pred_variant(0)
        assert np.array_equal(b, eng.generate(embd=pe, **S.request("sampled", 4)).codes)
    finally:
        eng.close()
        om.close()


# ---- 6. repetition penalty -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", sorted(S.PENALTY_CASES))
def test_penalty_equals_the_restatement(tiny, case):
    cfg, eng, om, pred, _ = tiny
    ids, talker = S.PENALTY_CASES[case]
    pe = S.prompt(om, ids)
    kw = dict(talker, max_steps=S.FRAMES, min_frames=S.FRAMES)
    base = eng.generate(embd=pe, **kw).codes
    ref, _ = S.generate(om, pred, pe, penalty=S.PENALTY, **kw)
    eng.set_repetition_penalty(S.PENALTY)
    assert eng.repetition_penalty() == pytest.approx(S.PENALTY)
    got = eng.generate(embd=pe, **kw).codes
    assert np.array_equal(got, ref) and not np.array_equal(got, base)
    assert np.array_equal(eng.generate(embd=pe, **kw).codes, ref)   # the seen set is cleared at admission
    eng.set_repetition_penalty(1.0)
    assert np.array_equal(eng.generate(embd=pe, **kw).codes, base)


def test_penalty_behind_a_voice_prefix(oracle, tiny):
    cfg, eng, om, pred, _ = tiny
    ids, talker = S.PENALTY_CASES["greedy"]
    kw = dict(talker, max_steps=S.FRAMES, min_frames=S.FRAMES)
    eng.set_repetition_penalty(S.PENALTY)
    eng.set_predictor_sampler(*S.PRED_CONFIGS["select"])
    whole, k1 = oracle.make_prompt_desc(ids, spk_emb=S.spk(cfg.model.d_embed))
    voice, k2 = oracle.make_prompt_desc(None, spk_emb=S.spk(cfg.model.d_embed), part="voice")
    text, k3 = oracle.make_prompt_desc(ids, part="text")
    want = eng.generate(desc=whole, **kw).codes
    ref, _ = S.generate(om, pred, S.prompt(om, ids), penalty=S.PENALTY, pred_sampler=S.PRED_CONFIGS["select"], **kw)
    assert np.array_equal(want, ref)
    with eng.create_prefix(desc=voice) as x:
        got = eng.generate(desc=text, prefix=x, **kw).codes
    assert np.array_equal(got, want)


# ---- 7. sessions, streams, errors -------------------------------------------------------------------------------------------------------
def test_session_and_state_errors(tiny):
    from q3tts import _abi, native
    cfg, eng, om, pred, pe = tiny
    lib = eng.lib
    ps = S.PRED_CONFIGS["select"]
    eng.set_predictor_sampler(*ps)
    eng.set_repetition_penalty(S.PENALTY)
    reqs = [dict(r, want_pcm=1) for r in S.batch_requests(om)[:5]]
    want = eng.generate_batch(reqs)
    chunks, finals = {}, {}
    with native.NativeSession(eng) as sess:
        ids = [sess.submit(**r) for r in reqs]
        # the setters are refused while the session owns the engine
        assert lib.q3tts_set_predictor_sampler(eng.h, 0.5, 10, 0.9) == STATE
        assert lib.q3tts_set_repetition_penalty(eng.h, 1.1) == STATE
        assert lib.q3tts_k_pred_variant(eng.h, 1) == STATE
        for rid, kind, pcm, is_final, res in sess.events(timeout_ms=60000):
            if kind == _abi.EV_CHUNK:
                chunks.setdefault(rid, []).append(pcm)
            else:
                finals[rid] = (kind, res)
    for i, rid in enumerate(ids):
        assert finals[rid][0] == _abi.EV_DONE and np.array_equal(finals[rid][1].codes, want[i].codes), i
        assert np.array_equal(np.concatenate(chunks[rid]), want[i].pcm), i
    assert eng.predictor_sampler() == pytest.approx(ps) and eng.repetition_penalty() == pytest.approx(S.PENALTY)
    # a stream holds the state too
    r, keep = native.NativeEngine.make_request(embd=pe, want_pcm=1, **S.request("sampled"))
    st = C.c_void_p()
    assert lib.q3tts_stream_begin(eng.h, C.byref(r), C.byref(st)) == 0
    assert lib.q3tts_set_predictor_sampler(eng.h, 0.5, 10, 0.9) == STATE
    assert lib.q3tts_set_repetition_penalty(eng.h, 1.1) == STATE
    assert lib.q3tts_stream_end(st, None) == 0
    assert eng.predictor_sampler() == pytest.approx(ps) and eng.repetition_penalty() == pytest.approx(S.PENALTY)
    # ... and a stream opened after the setters generates under them: the ids and PCM of generate()
    one = eng.generate(embd=pe, want_pcm=1, **S.request("sampled"))
    pcm = [c for c, fin in native.stream_chunks(eng, embd=pe, want_pcm=1, **S.request("sampled"))]
    assert np.array_equal(eng.last_stream_result.codes, one.codes) and np.array_equal(np.concatenate(pcm), one.pcm)
    # invalid arguments leave the state as it was
    for bad in ((-0.5, 50, 1.0), (float("nan"), 50, 1.0), (float("inf"), 50, 1.0), (0.9, 50, float("nan"))):
        assert lib.q3tts_set_predictor_sampler(eng.h, *bad) == INVALID, bad
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        assert lib.q3tts_set_repetition_penalty(eng.h, bad) == INVALID, bad
    assert eng.predictor_sampler() == pytest.approx(ps) and eng.repetition_penalty() == pytest.approx(S.PENALTY)
    ref, _ = S.generate(om, pred, pe, pred_sampler=ps, penalty=S.PENALTY, **S.request("sampled"))
    assert np.array_equal(eng.generate(embd=pe, **S.request("sampled")).codes, ref)


# ---- 8. the reference-style API -----------------------------------------------------------------------------------------------------------
def test_api_mirror():
    from q3tts import api
    eng = api.TtsEngine.new(config=S.tiny_cfg(max_batch=1))
    try:
        d = eng.get_predictor_sampler_config()
        assert (d.temperature, d.top_k, d.top_p) == (0.0, 0, 1.0) and eng.get_repetition_penalty() == 1.0   # defaults: greedy, no penalty
        eng.set_predictor_sampler_config(api.SamplerConfig(temperature=0.9, top_k=50, top_p=1.0, seed=123))
        eng.set_repetition_penalty(1.05)
        g = eng.get_predictor_sampler_config()
        assert (g.temperature, g.top_k, g.top_p, g.seed) == (pytest.approx(0.9), 50, 1.0, None)
        assert eng.get_repetition_penalty() == pytest.approx(1.05)
    finally:
        eng.close()


# ---- 9. the real Predictor shape (5 layers, d 1024, 2048-wide heads) behind the tiny Talker ------------------------------------------------
# (the whole full shape — 28 Talker layers on the CPU as well — is asserted once by tools/pred_sample_bench.py)
def test_real_predictor_shape(oracle):
    cfg = S.tiny_cfg(max_batch=2)
    m = cfg.model
    m.p_n_layer, m.p_d_model, m.p_n_head, m.p_n_kv_head, m.p_head_dim, m.p_d_ffn = 5, 1024, 16, 8, 128, 3072
    m.codebook_size, m.codecq_rows = 2048, 2048
    eng = _engine(cfg)
    om = oracle.OracleModel(cfg.model, seed=0, n_ctx=S.N_CTX, n_threads=8)
    try:
        pred, pe = S.mats_from_model(om, False, False), S.prompt(om, np.arange(300, 310))
        ps = S.PRED_CONFIGS["select"]
        tr = []
        ref, _ = S.generate(om, pred, pe, pred_sampler=ps, trace=tr, **S.request("sampled", 4))
        diff, n = S.differing(tr)
        assert 4 * diff >= n   # (the input condition, here because the CPU file does not pay for this shape twice)
        eng.set_predictor_sampler(*ps)
        assert np.array_equal(eng.generate(embd=pe, **S.request("sampled", 4)).codes, ref)
    finally:
        eng.close()
        om.close()

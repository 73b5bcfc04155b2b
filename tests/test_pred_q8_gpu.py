"""q3tts_engine_config.predictor_q8_0 = 2 on the device: the Predictor in ggml's Q8_0 x Q8_0 arithmetic (W8A8), bit for bit against the CPU
statement tests/_pred_q8.py (pinned to the oracle by tests/test_pred_q8_cpu.py)."""
import ctypes as C
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import _pred_q8 as P

pytestmark = pytest.mark.gpu
N_CTX = 256


def _spk(d):
    return ((np.arange(d) % 13 - 6) * 0.03125).astype(np.float32)


def _cfg(talker=0, pred=2, max_batch=4, with_vocoder=0, n_ctx=N_CTX):
    from q3tts import _abi
    cfg = _abi.tiny_config(max_batch=max_batch, n_ctx=n_ctx, with_vocoder=with_vocoder)
    cfg.talker_q8_0, cfg.predictor_q8_0 = talker, pred
    return cfg


def _oracle_model(oracle, cfg, n_ctx=N_CTX):
    om = oracle.OracleModel(cfg.model, seed=0, n_ctx=n_ctx, n_threads=8)
    if cfg.talker_q8_0 == 2:
        om.set_talker_q8a8()
    elif cfg.talker_q8_0 == 1:
        om.set_talker_q8()
    return om


def _prompt(oracle, om, ids):
    desc, keep = oracle.make_prompt_desc(np.asarray(ids), spk_emb=_spk(om.cfg.d_embed))
    return om.build_prompt(desc)


# ---- 1. the argmax epilogue of k_bgemm8 ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,K,N,with_ssp", [(1, 512, 32, True), (2, 1024, 64, True), (17, 512, 2048, True), (64, 1024, 2048, True),
                                            (128, 1024, 2048, True), (128, 512, 32, True), (17, 1024, 64, False), (64, 512, 64, True)])
def test_argmax_hook_is_argmax_of_the_oracle_gemm(oracle, B, K, N, with_ssp):
    from q3tts import native
    rng = np.random.default_rng(B * 7 + K + N)
    w = (rng.standard_normal((N, K)) * 0.02).astype(np.float32)
    # exact ties: a weight row duplicated into a LOWER and a HIGHER column; every other activation row leans towards it, so that the pair
    # holds those rows' maximum
    lo, hi = (5, N - 3) if N > 32 else (5, 20)
    w[hi] = w[lo]
    q, d16 = oracle.quantize_q8_0(w)
    v = rng.standard_normal((B, K)).astype(np.float32)
    v[::2] += 2.0 * np.sign(w[lo])[None, :]
    v = (v * np.exp2(rng.integers(-3, 4, size=(B, 1)))).astype(np.float32)
    aq, ad = oracle.quantize_q8_0_act(v)
    ssp = (rng.random((B, K // 16)) * 16.0 + 0.5).astype(np.float32) if with_ssp else None
    y = oracle.bgemm_q8a8(aq, ad, q, d16, ssp, K, 1e-6, 0)["y"]
    assert np.array_equal(y[:, lo].view(np.uint32), y[:, hi].view(np.uint32))
    want = np.argmax(y, axis=1)
    assert np.all(want[::2] == lo) and not np.any(want == hi)   # the tied rows: the lower column is the answer
    got = native.k_bgemm_q8a8_argmax(aq, ad, q, d16, ssp, K, 1e-6)
    assert np.array_equal(got, want)


# ---- 2. engine ids on the tiny shape -------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=[0, 2], ids=["talker_bf16", "talker_q8a8"])
def tiny(oracle, request):
    from q3tts import native
    cfg = _cfg(talker=request.param)
    eng = native.NativeEngine(cfg)
    om = _oracle_model(oracle, cfg)
    yield cfg, eng, om, P.mats_from_model(om, False, True)
    eng.close()
    om.close()


def test_engine_ids_equal_the_cpu_statement(oracle, tiny):
    cfg, eng, om, pred = tiny
    pe = _prompt(oracle, om, np.arange(100, 120))
    for kw in (dict(temperature=0.0, max_steps=8, min_frames=8), dict(temperature=0.7, top_k=40, top_p=0.9, seed=11, max_steps=8, min_frames=8)):
        ref, _ = P.generate(om, pred, pe, **kw)
        got = eng.generate(embd=pe, **kw)
        assert ref.shape[0] == 8 and got.status == 0 and np.array_equal(got.codes, ref), kw
    # the quantisation is really in the path: a bf16 Predictor gives other ids
    ref16, _ = om.generate(pe, temperature=0.0, max_steps=8, min_frames=8)
    assert not np.array_equal(ref16, P.generate(om, pred, pe, temperature=0.0, max_steps=8, min_frames=8)[0])


def test_continuous_batching_equals_one_at_a_time(oracle, tiny):
    cfg, eng, om, pred = tiny
    rng = np.random.default_rng(5)
    reqs = []
    for i in range(5):   # 5 requests on 4 slots: one slot is refilled
        pe = _prompt(oracle, om, rng.integers(0, 151643, size=int(rng.integers(3, 30))))
        t = [3, 9, 5, 12, 7][i]
        reqs.append(dict(embd=pe, temperature=0.7, top_k=40, top_p=0.9, seed=40 + i, max_steps=16, min_frames=t, force_eos_at=t))
    batch = eng.generate_batch(reqs)
    for i, r in enumerate(reqs):
        one = eng.generate(**r)
        assert batch[i].status == 0 and one.codes.shape[0] == r["min_frames"] and np.array_equal(batch[i].codes, one.codes), i
    ref, _ = P.generate(om, pred, reqs[1]["embd"], **{k: v for k, v in reqs[1].items() if k != "embd"})
    assert np.array_equal(batch[1].codes, ref)


def test_default_mode_is_what_it_was(oracle):
    from q3tts import native
    cfg = _cfg(talker=0, pred=0, max_batch=2)
    eng = native.NativeEngine(cfg)
    om = _oracle_model(oracle, cfg)
    try:
        pe = _prompt(oracle, om, np.arange(100, 120))
        ref, _ = om.generate(pe, temperature=0.0, max_steps=8, min_frames=8)
        assert np.array_equal(eng.generate(embd=pe, temperature=0.0, max_steps=8, min_frames=8).codes, ref)
    finally:
        eng.close()
        om.close()


# ---- 3. 64 slots ---------------------------------------------------------------------------------------------------------------------
def test_64_slots_equal_two_slots_and_the_cpu_statement(oracle):
    from q3tts import native
    cfg64, cfg2 = _cfg(talker=2, max_batch=64), _cfg(talker=2, max_batch=2)
    om = _oracle_model(oracle, cfg64)
    pred = P.mats_from_model(om, False, True)
    rng = np.random.default_rng(64)
    reqs = []
    for i in range(64):
        pe = _prompt(oracle, om, rng.integers(0, 151643, size=int(rng.integers(3, 24))))
        t = int(rng.integers(2, 9))
        reqs.append(dict(embd=pe, temperature=0.7, top_k=40, top_p=0.9, seed=6400 + i, max_steps=12, min_frames=t, force_eos_at=t))
    outs = {}
    for name, cfg in (("64", cfg64), ("2", cfg2)):
        eng = native.NativeEngine(cfg)
        try:
            outs[name] = eng.generate_batch(reqs)
        finally:
            eng.close()
    for i in range(64):
        assert outs["64"][i].status == 0 and outs["64"][i].codes.shape[0] == reqs[i]["min_frames"]
        assert np.array_equal(outs["64"][i].codes, outs["2"][i].codes), i
    for i in (0, 31, 63):
        ref, _ = P.generate(om, pred, reqs[i]["embd"], **{k: v for k, v in reqs[i].items() if k != "embd"})
        assert np.array_equal(outs["64"][i].codes, ref), i
    om.close()


# ---- 4. the real Predictor shape behind the tiny Talker ------------------------------------------------------------------------------
def test_real_predictor_shape(oracle):
    from q3tts import native
    cfg = _cfg(talker=0, max_batch=2)
    m = cfg.model
    m.p_n_layer, m.p_d_model, m.p_n_head, m.p_n_kv_head, m.p_head_dim, m.p_d_ffn = 5, 1024, 16, 8, 128, 3072
    m.codebook_size, m.codecq_rows = 2048, 2048
    cfg.vocoder.codebook_size = 2048
    eng = native.NativeEngine(cfg)
    om = _oracle_model(oracle, cfg)
    try:
        pred = P.mats_from_model(om, False, True)
        pe = _prompt(oracle, om, np.arange(300, 310))
        kws = (dict(temperature=0.0, max_steps=3, min_frames=3), dict(temperature=0.7, top_k=40, top_p=0.9, seed=5, max_steps=3, min_frames=3))
        with ThreadPoolExecutor(2) as ex:   # the two CPU references side by side (the oracle's calls release the interpreter lock)
            refs = list(ex.map(lambda kw: P.generate(om, pred, pe, **kw)[0], kws))
        for kw, ref in zip(kws, refs):
            assert ref.shape[0] == 3 and np.array_equal(eng.generate(embd=pe, **kw).codes, ref), kw
    finally:
        eng.close()
        om.close()


# ---- 5. from files -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ptype", ["q8_0", "f32"])
def test_predictor_from_model_files(oracle, tmp_path, ptype):
    import _gguf as G
    from q3tts import native
    cfg = _cfg(talker=0, max_batch=2, n_ctx=128)
    oracle.write_model_dir(str(tmp_path), cfg.model, 0, matrix_type=G.BF16, predictor_type=G.Q8_0 if ptype == "q8_0" else G.F32)
    cfg.weights_path = str(tmp_path).encode()
    eng = native.NativeEngine(cfg)
    om = _oracle_model(oracle, cfg, n_ctx=128)
    try:
        tens = oracle.synth_transformer_tensors(cfg.model, 0, False)
        blocks = None
        if ptype == "q8_0":   # the file's own blocks (tests/_gguf.py's writer), which must reach the device as stored
            blocks = {k: P.split_q8_0(G.encode(v, G.Q8_0), v.shape[0], v.shape[1]) for k, v in tens.items() if v.ndim == 2}
        pred = P.mats_from_tensors(cfg.model, tens, blocks)
        if ptype == "f32":    # the device's quantiser is q3o_quantize_q8_0: the synthetic model quantised by the oracle is the same Predictor
            auto = P.mats_from_model(om, False, True)
            assert all(np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) for a, b in zip(auto.qkv + [auto.head], pred.qkv + [pred.head]))
        pe = _prompt(oracle, om, np.arange(900, 912))
        for kw in (dict(temperature=0.0, max_steps=5, min_frames=5), dict(temperature=0.7, top_k=40, top_p=0.9, seed=11, max_steps=5, min_frames=5)):
            ref, _ = P.generate(om, pred, pe, **kw)
            assert ref.shape[0] == 5 and np.array_equal(eng.generate(embd=pe, **kw).codes, ref), kw
    finally:
        eng.close()
        om.close()


# ---- 6. contracts that keep holding --------------------------------------------------------------------------------------------------
def test_session_chunks_equal_generate_batch(oracle):
    from q3tts import _abi, native
    cfg = _cfg(talker=2, max_batch=2, with_vocoder=1)
    eng = native.NativeEngine(cfg)
    om = _oracle_model(oracle, cfg)
    try:
        reqs = [dict(embd=_prompt(oracle, om, np.arange(50 + 9 * i, 60 + 11 * i)), temperature=0.7, top_k=40, top_p=0.9, seed=9 + i, max_steps=10,
                     min_frames=t, force_eos_at=t, want_pcm=1) for i, t in enumerate((6, 9, 5))]
        want = eng.generate_batch(reqs)
        with native.NativeSession(eng) as sess:
            ids = [sess.submit(**r) for r in reqs]
            parts = {}
            for rid, kind, pcm, fin, res in sess.events(120000):
                g = parts.setdefault(rid, dict(chunks=[], res=None))
                if kind == _abi.EV_CHUNK:
                    g["chunks"].append(pcm)
                else:
                    assert kind == _abi.EV_DONE, kind
                    g["res"] = res
        for i, rid in enumerate(ids):
            assert np.array_equal(parts[rid]["res"].codes, want[i].codes), i
            assert np.array_equal(np.concatenate(parts[rid]["chunks"]).view(np.uint32), want[i].pcm.view(np.uint32)), i
    finally:
        eng.close()
        om.close()


def test_voice_prefix_gives_the_whole_prompts_codes(oracle):
    from q3tts import native
    cfg = _cfg(talker=2, max_batch=2)
    eng = native.NativeEngine(cfg)
    try:
        voice = dict(spk_emb=_spk(cfg.model.d_embed))
        dv, kv = oracle.make_prompt_desc(None, part="voice", **voice)
        with eng.create_prefix(desc=dv) as x:
            for i, text in enumerate((np.arange(200, 215), np.arange(400, 407))):
                dw, kw_ = oracle.make_prompt_desc(text, **voice)
                dt, kt = oracle.make_prompt_desc(text, part="text")
                s = dict(temperature=0.7, top_k=40, top_p=0.9, seed=20 + i, max_steps=8, min_frames=8)
                whole, got = eng.generate(desc=dw, **s), eng.generate(desc=dt, prefix=x, **s)
                assert whole.codes.shape[0] == 8 and np.array_equal(got.codes, whole.codes), i
    finally:
        eng.close()


# ---- 7. refusals ---------------------------------------------------------------------------------------------------------------------
def test_refusals():
    from q3tts import _abi
    lib = _abi.load_library()
    unsupported = -6   # Q3TTS_ERR_UNSUPPORTED (include/q3tts.h)
    cfg = _cfg(pred=1, max_batch=1)
    h = C.c_void_p()
    assert lib.q3tts_engine_create(C.byref(cfg), C.byref(h)) == unsupported and not h
    assert b"predictor_q8_0" in lib.q3tts_last_error(None)
    cfg = _cfg(pred=2, max_batch=1)
    cfg.model.p_d_ffn = 768
    rc = lib.q3tts_engine_create(C.byref(cfg), C.byref(h))
    assert rc != 0 and rc != unsupported and not h   # Q3TTS_ERR_INVALID
    assert b"p_d_ffn" in lib.q3tts_last_error(None)

"""The Predictor sampler and the code-0 repetition penalty on the CPU: the restatement tests/_pred_sample.py pinned to the oracle, the C
ABI's new symbols, and the condition on the inputs of tests/test_pred_sample_gpu.py — a build that kept the Predictor greedy, or applied
no penalty, must not be able to pass them."""
import ctypes as C

import numpy as np
import pytest

import _pred_sample as S


@pytest.fixture(scope="module")
def tiny(oracle):
    cfg = S.tiny_cfg()
    om = oracle.OracleModel(cfg.model, seed=0, n_ctx=S.N_CTX, n_threads=8)
    yield om, S.mats_from_model(om, False, False), S.prompt(om)
    om.close()


@pytest.mark.parametrize("talker", sorted(S.TALKERS))
def test_restatement_with_the_controls_off_is_the_oracle(tiny, talker):
    om, pred, pe = tiny
    ref, ref_eos = om.generate(pe, **S.request(talker))
    got, eos = S.generate(om, pred, pe, **S.request(talker))   # defaults: Predictor temperature 0, penalty 1.0
    assert ref.shape[0] == S.FRAMES and eos == ref_eos and np.array_equal(got, ref)
    got, _ = S.generate(om, pred, pe, pred_sampler=(0.0, 50, 0.8), penalty=1.0, **S.request(talker))   # temperature 0: top_k / top_p are not looked at
    assert np.array_equal(got, ref)


def test_new_symbols_and_null_engine():
    from q3tts import _abi
    lib = _abi.load_library()
    t, k, p = C.c_float(), C.c_int32(), C.c_float()
    invalid = -1   # Q3TTS_ERR_INVALID
    assert lib.q3tts_set_predictor_sampler(None, 0.9, 50, 1.0) == invalid
    assert lib.q3tts_get_predictor_sampler(None, C.byref(t), C.byref(k), C.byref(p)) == invalid
    assert lib.q3tts_set_repetition_penalty(None, 1.05) == invalid
    assert lib.q3tts_get_repetition_penalty(None, C.byref(p)) == invalid
    assert lib.q3tts_k_pred_variant(None, 1) == invalid
    assert C.sizeof(_abi.Request) == 80   # the controls are engine state: the request did not grow
    assert _abi.EngineConfig._fields_[-1][0] == "predictor_q8_0"


@pytest.mark.parametrize("talker", sorted(S.TALKERS))
@pytest.mark.parametrize("name", ["select", "sort_top_p"])
def test_gpu_inputs_a_greedy_predictor_would_fail(tiny, talker, name):
    om, pred, pe = tiny
    base, _ = S.generate(om, pred, pe, **S.request(talker))
    tr = []
    got, _ = S.generate(om, pred, pe, pred_sampler=S.PRED_CONFIGS[name], trace=tr, **S.request(talker))
    diff, n = S.differing(tr)
    assert n == S.FRAMES * (om.cfg.n_codebooks - 1) and 4 * diff >= n, (diff, n)
    assert not np.array_equal(got, base)


@pytest.mark.parametrize("talker", sorted(S.TALKERS))
def test_top_k_1_is_greedy(tiny, talker):
    om, pred, pe = tiny
    base, _ = S.generate(om, pred, pe, **S.request(talker))
    got, _ = S.generate(om, pred, pe, pred_sampler=S.PRED_CONFIGS["top1"], **S.request(talker))
    assert np.array_equal(got, base)


@pytest.mark.parametrize("case", sorted(S.PENALTY_CASES))
def test_gpu_penalty_inputs_change_a_code0(tiny, case):
    om, pred, _ = tiny
    ids, talker = S.PENALTY_CASES[case]
    pe = S.prompt(om, ids)
    kw = dict(talker, max_steps=S.FRAMES, min_frames=S.FRAMES)
    base, _ = S.generate(om, pred, pe, **kw)
    pen, _ = S.generate(om, pred, pe, penalty=S.PENALTY, **kw)
    assert len(set(base[:, 0].tolist())) < S.FRAMES          # the unpenalised run repeats a code 0 ...
    assert np.any(pen[:, 0] != base[:, 0])                   # ... and the penalty moves at least one
    one, _ = S.generate(om, pred, pe, penalty=1.0, **kw)
    assert np.array_equal(one, base)


def test_gpu_batch_wide_and_q8_inputs_a_greedy_predictor_would_fail(oracle, tiny):
    om, pred, pe = tiny
    ps = S.PRED_CONFIGS["select"]
    r = S.batch_requests(om)[1]   # the batching test compares this request with the restatement
    tr = []
    S.generate(om, pred, r["embd"], pred_sampler=ps, trace=tr, **{k: v for k, v in r.items() if k != "embd"})
    diff, n = S.differing(tr)
    assert 4 * diff >= n, (diff, n)
    pred8 = S.mats_from_model(om, False, True)   # predictor_q8_0 = 2
    tr = []
    S.generate(om, pred8, pe, pred_sampler=ps, trace=tr, **S.request("sampled", 4))
    diff, n = S.differing(tr)
    assert 4 * diff >= n, (diff, n)
    cfgw = S.tiny_cfg(wide=True)
    omw = oracle.OracleModel(cfgw.model, seed=0, n_ctx=S.N_CTX, n_threads=8)
    try:
        tr = []
        S.generate(omw, S.mats_from_model(omw, False, False), S.prompt(omw), pred_sampler=ps, trace=tr, **S.request("sampled", 4))
        diff, n = S.differing(tr)
        assert 4 * diff >= n, (diff, n)
    finally:
        omw.close()

"""sample_row on the device (k_sample_rows behind the q3tts_k_sample hook; k_sample_input and k_pred_next<true> through an engine) over the
calls of tests/_sampler_ref.py: `==` against q3o_sample, and membership in the float64 admissible set, which does not involve the oracle.
tests/test_sampler_cpu.py shows on the CPU what the second comparison is worth."""
import time

import numpy as np
import pytest

import _pred_sample as S
import _sampler_ref as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def native():
    from q3tts import native
    return native


@pytest.fixture(scope="module")
def calls():
    return list(R.cases(0))


@pytest.fixture(scope="module")
def device(native, calls):
    """The device's ids of every call, computed once."""
    t0 = time.time()
    out = [native.k_sample(lg, limit, T, k, p, r) for (fam, limit, T, k, p, lg, r) in calls]
    print("%d hook calls, %d rows: %.2f s" % (len(out), sum(o.size for o in out), time.time() - t0))
    return out


def _oracle_ids(oracle, lg, limit, T, k, p, r):
    L = oracle.lib()
    return np.array([L.q3o_sample(oracle.ptr(lg[i], oracle.f32p), limit, T, k, p, float(r[i])) for i in range(lg.shape[0])], dtype=np.int32)


def test_sample_rows_equal_the_oracle_on_every_case(oracle, calls, device):
    for (fam, limit, T, k, p, lg, r), got in zip(calls, device):
        assert got.shape == (R.ROWS,) and np.all((got >= 0) & (got < limit)), (fam, limit, T, k, p, got)
        ref = _oracle_ids(oracle, lg, limit, T, k, p, r)
        assert np.array_equal(got, ref), (fam, limit, T, k, p, got, ref)


def test_sample_rows_lie_in_the_float64_admissible_set(calls, device):
    out = []
    for (fam, limit, T, k, p, lg, r), got in zip(calls, device):
        for i in range(R.ROWS):
            A = R.admissible(lg[i], limit, T, k, p, r[i])
            if int(got[i]) not in A:
                out.append((fam, limit, T, k, p, i, float(r[i]), int(got[i]), sorted(A)[:4]))
    assert not out, (len(out), out[:5])


def test_select_overflow_falls_back_to_the_sort(oracle, native):
    rng = np.random.default_rng(21)
    for limit in (2049, 2160, 4096):
        lg = R.family_rows("overflow", rng, limit, 64)
        r = ((np.arange(64) + rng.random(64)) / 64.0).astype(np.float32)   # 64 distinct draws, one per 64th
        for top_k in (255, 256, 257):   # 257 takes the sort directly
            if limit != 2049 and top_k != 257:
                assert all(R.select_list_length(row, limit, top_k) > 2048 for row in lg)
            for top_p in (1.0, 0.9):
                got = native.k_sample(lg, limit, 1.0, top_k, top_p, r)
                assert np.array_equal(got, _oracle_ids(oracle, lg, limit, 1.0, top_k, top_p, r)), (limit, top_k, top_p)
                if top_p == 1.0:
                    assert np.unique(got).size > 8, (limit, top_k, got)   # not collapsed to one key


def test_greedy_is_the_first_maximum(calls, device):
    n = 0
    for (fam, limit, T, k, p, lg, r), got in zip(calls, device):
        if T <= 0.0:
            n += 1
            assert [int(g) for g in got] == [R.greedy(row, limit) for row in lg], (fam, limit)
    assert n == len(R.FAMILIES) * len(R.LIMITS) + 1
    fam, limit, T, k, p, lg, r = calls[-1]
    assert fam == "nan" and np.isnan(lg[0, :limit]).all() and device[-1][0] == 0   # the all-NaN row


def test_hook_refuses_rows_wider_than_the_sampler(native):
    from q3tts import _abi
    lg = np.zeros((2, 4200), dtype=np.float32)
    for limit, rows in ((0, lg), (4097, lg), (65, lg[:, :64])):
        with pytest.raises(_abi.Q3Error, match="bad shape"):
            native.k_sample(rows, limit, 0.7, 40, 0.9, np.zeros(2, dtype=np.float32))


# ---- the fused entry points, at the boundaries an engine reaches by configuration --------------------------------------------------------
FRAMES = 8


def _request(temperature, top_k, top_p):
    return dict(temperature=temperature, top_k=top_k, top_p=top_p, seed=11, max_steps=FRAMES, min_frames=FRAMES)


@pytest.fixture(scope="module")
def tiny(oracle):
    from q3tts import native
    cfg = S.tiny_cfg()
    eng = native.NativeEngine(cfg)
    om = oracle.OracleModel(cfg.model, seed=0, n_ctx=S.N_CTX, n_threads=8)
    yield eng, om, S.mats_from_model(om, False, False), S.prompt(om)
    eng.close()
    om.close()


@pytest.mark.parametrize("top_p", [1e-6, 0.999999])
@pytest.mark.parametrize("top_k", [255, 256, 257])
def test_frame_step_sampler_at_the_select_sort_boundary(tiny, top_k, top_p):
    """k_sample_input: the Talker's sampler on sample_limit = 2160 logits with top_k on both sides of the select path's 256 and top_p at
    both ends; min_frames masks the EOS logit with -inf on every frame."""
    eng, om, pred, pe = tiny
    kw = _request(0.7, top_k, top_p)
    ref, _ = S.generate(om, pred, pe, **kw)
    got = eng.generate(embd=pe, **kw)
    assert got.status == 0 and ref.shape[0] == FRAMES and np.array_equal(got.codes, ref)


def test_predictor_sampler_on_the_wide_codebook(oracle):
    """k_pred_next<true>: the Predictor sampler (0.9, 256, 1.0) on 2048-wide heads (the select path's largest top_k, 8 candidates per
    thread), behind a Talker at temperature 1e-3 (every exp but the first is 0)."""
    from q3tts import native
    cfg = S.tiny_cfg(wide=True)
    eng = native.NativeEngine(cfg)
    om = oracle.OracleModel(cfg.model, seed=0, n_ctx=S.N_CTX, n_threads=8)
    try:
        pred, pe = S.mats_from_model(om, False, False), S.prompt(om)
        ps = (0.9, 256, 1.0)
        kw = _request(1e-3, 256, 0.999999)
        tr = []
        ref, _ = S.generate(om, pred, pe, pred_sampler=ps, trace=tr, **kw)
        diff, n = S.differing(tr)
        assert 4 * diff >= n   # (the input condition: a greedy Predictor cannot pass)
        eng.set_predictor_sampler(*ps)
        got = eng.generate(embd=pe, **kw)
        assert got.status == 0 and ref.shape[0] == FRAMES and np.array_equal(got.codes, ref)
    finally:
        eng.close()
        om.close()

"""The device side of tests/test_q8_scales_cpu.py: k_bgemm8 (W8A8) and k_bgemm<Q8> (W8A16) at the magnitudes where an f16 activation scale
would be subnormal, zero or infinite, and with weight blocks whose FILE scale is a subnormal f16, 0x0001 or 0x7BFF — first bit for bit
against the oracle (the hardware's conversions and denormal mode against the oracle's integer code), then against float64."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _q8_scales as S  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def native():
    from q3tts import native
    return native


E_GPU = [-24, -21, -20, -19, -12, -10, -9, -8, 0, 8, 20, 21, 22, 24]   # both sides of each f16 boundary of d = amax / 127 for rows of ~1.5 x 2^e


def _edge_weight_scales(d16, epi):
    """File scales no quantiser produces: subnormal f16, the smallest subnormal, the largest finite f16, zero with non-zero quants.
    SwiGLU: the two maximal ones go to up rows (a gate of 1e9 would test expf's overflow, not the GEMM)."""
    d16 = d16.copy()
    big = d16.shape[0] // 2 if epi == 2 else 0
    d16[0, 0] = 0x0001; d16[1, 1] = 0x03ff; d16[2, 0] = 0x0200; d16[big + 4, 2] = 0x7bff; d16[5, 0] = 0x0000; d16[6, 1] = 0x8001; d16[big + 7, 3] = 0xfbff
    return d16


@pytest.mark.parametrize("B,K,N,epi", [(64, 2048, 4096, 0), (64, 2048, 2048, 1), (64, 2048, 12288, 2), (64, 6144, 2048, 1), (64, 2048, 3072, 0),
                                       (1, 2048, 4096, 0), (1, 2048, 2048, 1), (1, 2048, 12288, 2), (1, 6144, 2048, 1), (1, 2048, 3072, 0),
                                       (37, 1024, 256, 2), (130, 512, 512, 1)])
def test_bgemm_q8a8_bit_equal_over_activation_and_weight_scale_range(oracle, native, B, K, N, epi):
    """The Talker's five GEMMs at 64 rows and 1 row, a ragged row tile, > 64 rows. Row r of the operand sits at its own magnitude 2^e
    (E_GPU, cycled), so one launch holds blocks whose scale an f16 would flush, round to a subnormal, keep, or overflow; one block is
    zero, one has a zero scale over non-zero quants; weight scales include subnormal, 0x0001, 0x7BFF and their negatives."""
    rng = np.random.default_rng(B + K + N + epi)
    es = np.array([E_GPU[r % len(E_GPU)] for r in range(B)])
    a = (rng.standard_normal((B, K)) * 1.5).astype(np.float32) * np.float32(2.0) ** es[:, None]
    a[B // 2, 64:96] = 0.0
    aq, ad = oracle.quantize_q8_0_act(a)
    ad[0, 3] = 0.0   # zero scale, non-zero quants upstream
    w = (0.02 * rng.standard_normal((N, K))).astype(np.float32)
    q, d16 = oracle.quantize_q8_0(w)
    d16 = _edge_weight_scales(d16, epi)
    ssp = ((np.abs(rng.standard_normal((B, K // 16))) * 4.0 + 0.5) * 4.0 ** es[:, None]).astype(np.float32) if epi in (0, 2) else None   # s_r ~ 2^-e
    nw_next = (1.0 + 0.05 * rng.standard_normal(N)).astype(np.float32) if epi == 1 else None
    y0 = ((2.0 * rng.standard_normal((B, N))).astype(np.float32) * np.float32(2.0) ** es[:, None]) if epi == 1 else None
    ref = oracle.bgemm_q8a8(aq, ad, q, d16, ssp, K, 1e-6, epi, nw_next, y0)
    got = native.k_bgemm_q8a8(aq, ad, q, d16, ssp, K, 1e-6, epi, nw_next, y0)
    if epi in (0, 1):
        assert np.all(np.isfinite(ref["y"])) and np.array_equal(S.bits(got["y"]), S.bits(ref["y"]))
    if epi == 1:
        assert np.array_equal(S.bits(got["ssp_out"]), S.bits(ref["ssp_out"]))
    if epi in (1, 2):
        assert np.array_equal(S.bits(got["yd"]), S.bits(ref["yd"])) and np.array_equal(got["yq"], ref["yq"])
        assert np.count_nonzero(got["yq"]) > got["yq"].size // 2 and np.all(np.isfinite(got["yd"]))


@pytest.mark.parametrize("B,K,N,epi", [(64, 2048, 4096, 0), (64, 2048, 2048, 1), (64, 2048, 12288, 2), (64, 6144, 2048, 1), (1, 2048, 3072, 0), (37, 1024, 256, 2),
                                       (130, 512, 512, 1)])
def test_bgemm_q8_bit_equal_with_edge_weight_scales(oracle, native, B, K, N, epi):
    """Mode 1 (W8A16): bf16 rows at per-row magnitudes 2^e against Q8_0 blocks whose file scales include subnormal f16, 0x0001, 0x7BFF."""
    rng = np.random.default_rng(3 * B + K + N + epi)
    es = np.array([E_GPU[r % len(E_GPU)] for r in range(B)])
    x = (rng.standard_normal((B, K)) * 1.5).astype(np.float32) * np.float32(2.0) ** es[:, None]
    xb = S.bf16_bits(x)
    w = (0.02 * rng.standard_normal((N, K))).astype(np.float32)
    q, d16 = oracle.quantize_q8_0(w)
    d16 = _edge_weight_scales(d16, epi)
    ssp = ((np.abs(rng.standard_normal((B, K // 16))) * 4.0 + 0.5) * 4.0 ** es[:, None]).astype(np.float32) if epi in (0, 2) else None   # s_r ~ 2^-e
    nw_next = (1.0 + 0.05 * rng.standard_normal(N)).astype(np.float32) if epi == 1 else None
    y0 = ((2.0 * rng.standard_normal((B, N))).astype(np.float32) * np.float32(2.0) ** es[:, None]) if epi == 1 else None
    ref = oracle.bgemm_q8(xb, q, d16, ssp, K, 1e-6, epi, nw_next, y0)
    got = native.k_bgemm_q8(xb, q, d16, ssp, K, 1e-6, epi, nw_next, y0)
    if epi in (0, 1):
        assert np.all(np.isfinite(ref["y"])) and np.array_equal(S.bits(got["y"]), S.bits(ref["y"]))
    if epi == 1:
        assert np.array_equal(got["yb"], ref["yb"]) and np.array_equal(S.bits(got["ssp_out"]), S.bits(ref["ssp_out"]))
    if epi == 2:
        assert np.array_equal(got["yb"], ref["yb"])


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_device_gemm_invariance_and_float64_accuracy(oracle, native, mode):
    """The CPU file's two properties on the device output: y(2^e x) == y(x) bit for bit at eps = 0 over e = -24 .. +24 (each e also equal to
    the oracle), and for W8A8 the float64 error within the measured margin of ggml's order over the range where that is flat."""
    gemm = dict(bf16=native.k_bgemm, q8=native.k_bgemm_q8, q8a8=native.k_bgemm_q8a8)
    c = S.case(19, *S.SHAPES[0])
    y0 = S.layer0(c, 0, 0.0, mode, gemm)
    assert np.array_equal(S.bits(y0), S.bits(S.layer0(c, 0, 0.0, mode)))
    bad = [e for e in S.E_SWEEP if not np.array_equal(S.bits(S.layer0(c, e, 0.0, mode, gemm)), S.bits(y0))]
    assert not bad, f"mode {mode}: device y(2^e x) != y(x) at e = {bad}"
    if mode == 2:
        mean, std = oracle.Q8_SCALE_RATIO["gemm"]
        acc = []
        for e in S.E_FLAT[::3]:
            dev, ref = S.layer0_errors(c, e, 1e-6, gemm)
            print(f"e = {e:+3d}: device {dev:.4e}  ggml's order {ref:.4e}")
            if not dev / ref <= mean + oracle.Q8_SCALE_SIGMAS * std:
                acc.append((e, round(dev / ref, 4)))
        assert not acc, acc


def test_device_producer_epilogues_over_magnitudes(oracle, native):
    """The residual and SwiGLU producers of k_bgemm8 at the CPU file's magnitudes: bit-equal to the oracle at every step of the sweeps."""
    c = S.resid_case(200, 8, 1024, 256)
    for e in S.E_SWEEP[::2]:
        ref, got = S.resid(c, e), S.resid(c, e, native.k_bgemm_q8a8)
        assert all(np.array_equal(S.bits(got[k]), S.bits(ref[k])) for k in ("y", "yd", "ssp_out")) and np.array_equal(got["yq"], ref["yq"]), e
    for small in (True, False):
        c = S.swiglu_case(300, 8, 1024, 256, small)
        for ew in S.EW_SWEEP[::3] + [S.EW_SWEEP[-1]]:
            ref, got = S.swiglu(c, ew), S.swiglu(c, ew, native.k_bgemm_q8a8)
            assert np.array_equal(S.bits(got["yd"]), S.bits(ref["yd"])) and np.array_equal(got["yq"], ref["yq"]), (small, ew)


@pytest.mark.parametrize("B,K,N,epi", [(64, 2048, 12288, 2), (64, 6144, 2048, 1)])
@pytest.mark.parametrize("e", [-24, 24])
def test_full_shape_legs_at_the_extreme_magnitudes(oracle, native, B, K, N, epi, e):
    """The benchmarked shape's SwiGLU and down-projection launches with every row at 2^-24 / 2^+24."""
    rng = np.random.default_rng(K + e)
    a = (rng.standard_normal((B, K)) * 1.5).astype(np.float32) * np.float32(2.0 ** e)
    aq, ad = oracle.quantize_q8_0_act(a)
    q, d16 = oracle.quantize_q8_0((0.02 * rng.standard_normal((N, K))).astype(np.float32))
    ssp = np.full((B, K // 16), 16.0 * 2.25 * 4.0 ** e, dtype=np.float32) if epi == 2 else None   # the rows' own sum of squares: s_r ~ 2^-e / 1.5
    nw_next = (1.0 + 0.05 * rng.standard_normal(N)).astype(np.float32) if epi == 1 else None
    y0 = ((2.0 * rng.standard_normal((B, N))).astype(np.float32) * np.float32(2.0 ** e)) if epi == 1 else None
    ref = oracle.bgemm_q8a8(aq, ad, q, d16, ssp, K, 0.0, epi, nw_next, y0)
    got = native.k_bgemm_q8a8(aq, ad, q, d16, ssp, K, 0.0, epi, nw_next, y0)
    assert np.array_equal(S.bits(got["yd"]), S.bits(ref["yd"])) and np.array_equal(got["yq"], ref["yq"]) and np.count_nonzero(got["yq"]) > got["yq"].size // 2
    if epi == 1:
        assert np.array_equal(S.bits(got["y"]), S.bits(ref["y"])) and np.array_equal(S.bits(got["ssp_out"]), S.bits(ref["ssp_out"]))


def _attend_policy(decode, prefill):
    from q3tts import _abi
    assert _abi.load_library().q3tts_k_attend_policy(decode, prefill) == 0


def test_engine_prefill_over_prompt_magnitudes(oracle):
    """The producers without a kernel hook — the prompt rows' k_norm_inputs_q8, the attention output o / l — through an engine with
    talker_q8_0 = 2 (tiny shape): prompt rows x 2^e, hidden and logits bit-equal to the oracle at every e under each attention policy."""
    from q3tts import _abi, native
    cfg = _abi.tiny_config(max_batch=2, n_ctx=128, with_vocoder=0)
    cfg.talker_q8_0 = 2
    eng = native.NativeEngine(cfg)
    om = oracle.OracleModel(cfg.model, seed=0, n_ctx=128, n_threads=min(16, os.cpu_count() or 4))
    om.set_talker_q8a8()
    try:
        pe0 = S.talker_prompt(om, cfg, 400)
        for e in S.E_TALKER:
            pe = pe0 * np.float32(2.0 ** e)
            h_ref, l_ref = om.talker_prefill(pe)
            assert np.all(np.isfinite(l_ref)) and np.any(l_ref != 0)
            try:
                for pol in ((0, 0), (1, 1), (0, 2)):
                    _attend_policy(*pol)
                    h, l = eng.talker_prefill(pe)
                    assert np.array_equal(S.bits(l), S.bits(l_ref)) and np.array_equal(S.bits(h), S.bits(h_ref)), (e, pol)
            finally:
                _attend_policy(0, 0)
    finally:
        eng.close()
        om.close()

"""The Q8_0 Talker's arithmetic away from O(1) magnitudes, on the oracle alone (the device is held to the oracle bit for bit by
tests/test_q8_scales_gpu.py). W8A8 (talker_q8_0 = 2) quantises every activation where it is produced, from the UN-normalised v = x * nw, so
the block scale d = amax / 127 carries the magnitude of the residual stream. Kept as f16 it is subnormal below amax = 127 * 2^-14, zero
below 127 * 2^-25 and infinite above 127 * 65504. Run against the oracle as it was with f16 activation scales, this file fails for mode 2
only: the GEMM invariance at every e <= -8 and e >= +14 (the x300 channels overflow first), the accuracy test from e = +13 up (inf, NaN from
+21), the residual producer at e <= -8 and e >= +20, the SwiGLU producer at every step of the small base and from 2^+21 of the large one,
the whole Talker at e = -20 (logits all zero); modes 0 and 1 pass either way. The scale is therefore d rounded to f16's
11-bit significand but kept in f32 (q3o_round_sig11): same bits wherever the f16 scale was normal, no exponent limit. DESIGN.md §4.1d."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _oracle as O  # noqa: E402
import _q8_scales as S  # noqa: E402


def test_activation_scale_is_f16_precision_without_f16_range():
    """q3o_round_sig11 == the f16 conversion wherever that is a normal number (so no existing expectation moves), a 11-bit significand at
    every other exponent, exact under 2^e, 0 -> 0; the quantiser's quants do not depend on the magnitude at all."""
    rng = np.random.default_rng(1)
    d = np.abs(rng.standard_normal(4000)).astype(np.float32) * np.float32(2.0) ** rng.integers(-13, 15, size=4000)
    d = np.concatenate([d, np.float32([2.0 ** -14, 65504.0, 65519.0 * 0.5, 1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11, 2.0 - 2.0 ** -12])])
    d = d[(d >= 2.0 ** -14) & (d < 65520.0)]
    r = np.array([O.lib().q3o_round_sig11(float(v)) for v in d], dtype=np.float32)
    assert np.array_equal(r, d.astype(np.float16).astype(np.float32))
    for e in (-100, -40, -20, 30, 100):
        re = np.array([O.lib().q3o_round_sig11(float(np.float32(v) * np.float32(2.0 ** e))) for v in d[:500]], dtype=np.float32)
        assert np.array_equal(re.astype(np.float64), r[:500].astype(np.float64) * 2.0 ** e)
        assert not np.any(S.bits(re) & 0x1fff)
    assert O.lib().q3o_round_sig11(0.0) == 0.0
    x = (rng.standard_normal((4, 256)) * 1.5).astype(np.float32); x[1, 32:64] = 0.0
    q0, d0 = O.quantize_q8_0_act(x)
    q16, d16 = O.quantize_q8_0(x)
    assert np.array_equal(q0, q16) and np.array_equal(d0, d16.view(np.float16).astype(np.float32))   # O(1): the f16 scale, bit for bit
    assert d0[1, 1] == 0.0 and not q0[1, 32:64].any()                                                # a zero block: d = 0, q = 0
    for e in S.E_SWEEP:
        qe, de = O.quantize_q8_0_act(x * np.float32(2.0 ** e))
        assert np.array_equal(qe, q0) and np.array_equal(de.astype(np.float64), d0.astype(np.float64) * 2.0 ** e), e


@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("shape", S.SHAPES)
def test_gemm_output_is_bit_invariant_under_power_of_two_row_scaling(shape, mode):
    """eps = 0, rows x 2^e: squares, tile sums, ss / d, 1 / sqrtf of an even power, x * nw, the operand rounding (bf16 or int8 + scale),
    every block product and the row scale all move by exact powers of two, so y(2^e x) == y(x) BIT FOR BIT — in the bf16 path, with Q8_0
    weights, and in W8A8. No tolerance. e = -24 .. +24: both sides of every boundary an f16 activation scale would have."""
    c = S.case(11 + shape[0], *shape)
    y0 = S.layer0(c, 0, 0.0, mode)
    assert np.all(np.isfinite(y0)) and np.count_nonzero(y0) > y0.size // 2
    bad = [e for e in S.E_SWEEP if not np.array_equal(S.bits(S.layer0(c, e, 0.0, mode)), S.bits(y0))]
    assert not bad, f"mode {mode}: y(2^e x) != y(x) at e = {bad}"


@pytest.mark.parametrize("seed", [100, 101, 102])
def test_gemm_accuracy_against_float64_with_ggml_order_as_yardstick(seed):
    """RMSNorm -> Linear at eps = 1e-6 against float64 on the de-quantised weights (the activation side alone). e_ref = the same product
    with the row quantised in ggml's order (the normalised row, f16 d, the rule of tests/_gguf.py); the range is where e_ref is flat (within
    2 % of e = 0: asserted). This design's error may exceed e_ref at the same e by the ratio measured at e = 0 plus the sampling noise of the
    two int8 roundings (tests/_oracle.py Q8_SCALE_RATIO)."""
    c = S.case(seed, *S.SHAPES[0])
    mean, std = O.Q8_SCALE_RATIO["gemm"]
    ref0 = S.layer0_errors(c, 0, 1e-6)[1]
    rows = []
    for e in S.E_FLAT:
        dev, ref = S.layer0_errors(c, e, 1e-6)
        rows.append((e, dev, ref))
        print(f"e = {e:+3d}: this design {dev:.4e}  ggml's order {ref:.4e}  ratio {dev / ref:.4f}")
    assert all(abs(ref / ref0 - 1.0) <= 0.02 for _, _, ref in rows), "ggml's order is not flat over E_FLAT"
    bad = [(e, round(dev / ref, 4)) for e, dev, ref in rows if not dev / ref <= mean + O.Q8_SCALE_SIGMAS * std]
    assert not bad, f"error / e_ref above {mean + O.Q8_SCALE_SIGMAS * std:.4f} at (e, ratio) = {bad}"


def test_residual_epilogue_over_magnitudes():
    """q3o_bgemm_q8a8 epilogue 1 with the whole sum y0 + RAW at 2^e (y0 scaled, RAW through the activation scales: both exact): the produced
    quants are bit-identical, y, the block scales and the de-quantised yd * yq scale exactly, ssp_out by 4^e; and the produced operand is as
    close to float64 v = (y0 + RAW) * nw as ggml's quantiser is on the same row at O(1)."""
    c = S.resid_case(200, 8, 1024, 256)
    o0 = S.resid(c, 0)
    mean, std = O.Q8_SCALE_RATIO["resid"]
    assert np.count_nonzero(o0["yq"]) > o0["yq"].size // 2
    bad, acc = [], []
    for e in S.E_SWEEP:
        o = S.resid(c, e)
        k = 2.0 ** e
        same = (np.array_equal(o["yq"], o0["yq"]) and np.array_equal(o["yd"].astype(np.float64), o0["yd"].astype(np.float64) * k)
                and np.array_equal(o["y"].astype(np.float64), o0["y"].astype(np.float64) * k)
                and np.array_equal(o["ssp_out"].astype(np.float64), o0["ssp_out"].astype(np.float64) * k * k))
        if not same:
            bad.append(e)
        dev, ref = S.producer_errors(o["yq"], o["yd"], S.resid_f64(c, e))
        print(f"e = {e:+3d}: produced operand {dev:.4e}  ggml's quantiser {ref:.4e}")
        if not dev / ref <= mean + O.Q8_SCALE_SIGMAS * std:
            acc.append((e, round(dev / ref, 4)))
    assert not bad, f"residual producer not scale-invariant at e = {bad}"
    assert not acc, f"residual producer error / ggml's above {mean + O.Q8_SCALE_SIGMAS * std:.4f} at (e, ratio) = {acc}"


@pytest.mark.parametrize("small", [True, False])
def test_swiglu_epilogue_over_magnitudes(small):
    """Epilogue 2: h = silu(g) * u is linear in u, and u moves exactly with the up half's weight scales (kept normal f16: x 2^-1 .. 2^+24).
    small: the row scale is 2^-8, so whole rows of h lie below 127 * 2^-17 at the low end (asserted) — where an f16 block scale has lost
    its precision — and the other base reaches the largest magnitude the range allows. Quants bit-identical, scales exact, float64 accuracy."""
    c = S.swiglu_case(300, 8, 1024, 256, small)
    o0 = S.swiglu(c, 0)
    mean, std = O.Q8_SCALE_RATIO["swiglu"]
    assert np.count_nonzero(o0["yq"]) > o0["yq"].size // 2
    if small:
        assert np.abs(S.swiglu_f64(c, S.EW_SWEEP[0])).max() < 127 * 2.0 ** -17
    bad, acc = [], []
    for ew in S.EW_SWEEP:
        o = S.swiglu(c, ew)
        if not (np.array_equal(o["yq"], o0["yq"]) and np.array_equal(o["yd"].astype(np.float64), o0["yd"].astype(np.float64) * 2.0 ** ew)):
            bad.append(ew)
        dev, ref = S.producer_errors(o["yq"], o["yd"], S.swiglu_f64(c, ew))
        if not dev / ref <= mean + O.Q8_SCALE_SIGMAS * std:
            acc.append((ew, round(dev / ref, 4)))
    assert not bad, f"SwiGLU producer not scale-invariant at up-weight exponent {bad}"
    assert not acc, f"SwiGLU producer error / ggml's above {mean + O.Q8_SCALE_SIGMAS * std:.4f} at (ew, ratio) = {acc}"


def test_whole_talker_over_prompt_magnitudes():
    """The tiny model's prefill with the prompt rows x 2^e in all three modes: everything finite, no all-zero logit row, and the quantised
    modes' distance from the bf16 mode at the same e bounded as stated at tests/_oracle.py Q8_SCALE_RATIO."""
    m1, s1 = O.Q8_SCALE_RATIO["talker_1"]; m2, s2 = O.Q8_SCALE_RATIO["talker_2"]
    rel = O.Q8_SCALE_SIGMAS * float(np.hypot(s1 / m1, s2 / m2))
    bad = []
    for e in S.E_TALKER:
        h0, l0 = S.talker_logits(400, e, 0)
        fig = {}
        for mode in (1, 2):
            h, l = S.talker_logits(400, e, mode)
            assert np.all(np.isfinite(h)) and np.all(np.isfinite(l)) and np.any(l != 0), (e, mode)
            fig[mode] = S.rel_rms(l, l0)
        print(f"e = {e:+3d}: logits against bf16: mode 1 {fig[1]:.5f}  mode 2 {fig[2]:.5f}")
        if not (fig[1] <= O.Q8_TALKER_MARGIN * m1 and fig[2] <= O.Q8_TALKER_MARGIN * m2 and fig[2] <= fig[1] * np.sqrt(2.0) * (1.0 + rel)):
            bad.append((e, round(fig[1], 5), round(fig[2], 5)))
    assert not bad, f"(e, mode 1, mode 2) = {bad}"

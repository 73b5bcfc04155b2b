"""The stage-by-stage float64 check of the vocoder's convolution half (tests/_voc_ref.py, used on the device by
tests/test_vocoder_stages_gpu.py) can fail: proven here on the CPU.

The bf16-input oracle's own stage data, put into the device's tap format, passes every stage (its sequential f32 sums sit inside the bounds;
this also checks the numpy references against oracle/q3_oracle_vocoder.c). Then one stage output at a time is replaced by what a plausible
kernel bug would have written. Each must exceed its stage bound by >= 10x in at least one element; each is also pushed through the rest of
the oracle to the PCM, and the whole-signal RMS criterion of the PCM tests (<= 2e-3 at these shapes) is printed beside it."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _oracle  # noqa: E402
import _voc_ref as VR  # noqa: E402

PCM_RMS_TOL = 2e-3   # tests/test_parity_gpu.py: the small shapes' whole-signal bound


def _vc(shape):
    from q3tts import _abi
    vc = _abi.tiny_config(max_batch=1, n_ctx=128, with_vocoder=1).vocoder
    if shape == "narrow":
        vc.decoder_dim, vc.n_dec_blocks = 768, 3
        for i, r in enumerate((8, 5, 3)):
            vc.dec_rates[i] = r
    return vc


@pytest.fixture(scope="module", params=["tiny", "narrow"])
def voc(request):
    L = VR.bind(_oracle.lib())
    vc = _vc(request.param)
    v = L.q3o_vocoder_create(C.byref(vc), 0, 4)
    W = VR.Weights(L, v, vc)
    codes = np.random.default_rng(9).integers(0, vc.codebook_size, size=(3, 16)).astype(np.int32)
    yield request.param, W, codes, VR.oracle_taps(W, codes, fused=False)
    L.q3o_vocoder_destroy(v)


def test_oracle_stage_data_passes_every_stage(voc):
    shape, W, codes, taps = voc
    R = _oracle.VOC_STAGE_R[shape]
    for fused in (False, True):
        t = {k: a for k, a in taps.items() if not (fused and k.endswith(".z"))}
        res = VR.check_call(W, t, R)
        print(f"\n{shape}, {'fused' if fused else 'un-fused'} tap set: worst error / bound per stage")
        for stage, ratio, where in res:
            print(f"  {stage:44s} {ratio:6.3f}")
        assert all(r <= 1.0 for _, r, _ in res), [(s, r) for s, r, _ in res if not r <= 1.0]
    hc = VR.history_carry(None, taps)
    assert hc and all(ok for _, ok in hc)
    # ... and the carry check sees one wrong history row
    bad = dict(taps)
    a, H = taps["b0.r2.c1_in"]
    a = a.copy(); a[H - 1, 3] = 0x3F80
    bad["b0.r2.c1_in"] = (a, H)
    assert not all(ok for _, ok in VR.history_carry(None, bad))


# ---- deliberately wrong stage outputs --------------------------------------------------------------------------------------------------------
def _f(taps, name):
    a, H = taps[name]
    return VR.operand(a), H


def m_dilated_tap_row_late(W, t):
    """one tap of a dilated convolution reads one row late, only in the first 6 * dil rows of the call (a chunk-edge history error)"""
    b, u = 1, 2
    dil, C_ = VR.DIL[u], W.blocks[b][2]
    w, bias = W.conv(VR.VC_BLK + 4 * b + 1 + u, VR.VW_W, VR.VW_B, 7, C_, C_, C_, 0.5)
    x, H = _f(t, f"b{b}.r{u}.c1_in")
    acc, _ = VR.conv64(x, H, w, dil)
    T, tap, edge = acc.shape[0], 2, 6 * dil
    sh = (6 - tap) * dil
    acc[:edge] += (x[H - sh + 1:H - sh + 1 + edge] - x[H - sh:H - sh + edge]) @ w[tap].T
    ea2, ib2 = W.snake(VR.VC_BLK + 4 * b + 1 + u, VR.VW_ALPHA2, VR.VW_BETA2, C_)
    c1 = (acc + bias).astype(np.float32)
    return f"b{b}.r{u}.z", VR.bf16_bits(VR.snake64(c1.astype(np.float64), ea2, ib2).astype(np.float32)), 303 + 20 * b + 4 * u, c1, f"b{b}.r{u}.c1 + snake2 -> z"


def _ct(W, t, b, swap_phase=None, flat_bias=False, zero_ch=None):
    r, cin, cout = W.blocks[b]
    w, bias = W.conv(VR.VC_BLK + 4 * b, VR.VW_W, VR.VW_B, 2, cin, r * cout, cout, 1.0)
    w = w.copy()
    if swap_phase is not None:
        p = slice(swap_phase * cout, (swap_phase + 1) * cout)
        w[0, p], w[1, p] = w[1, p].copy(), w[0, p].copy()
    x, H = _f(t, f"b{b}.ct_in")
    acc, _ = VR.conv64(x, H, w, 1)
    bb = np.tile(bias, r)
    if flat_bias:
        bb = bias[np.minimum(np.arange(r * cout), cout - 1)]
    o = (acc + bb).reshape(-1, cout).astype(np.float32)
    if zero_ch is not None:
        o[:, zero_ch] = 0.0
    return f"b{b}.o_ct", o, 301 + 20 * b, o, f"b{b}.ct"


def m_ct_phase_other_tap(W, t):
    """one output phase of a transposed convolution uses the other tap's weights"""
    return _ct(W, t, 0, swap_phase=3)


def m_ct_bias_not_repeating(W, t):
    """the ConvTranspose bias does not repeat every cout (columns past cout read the last entry)"""
    return _ct(W, t, 1, flat_bias=True)


def m_zero_channel(W, t):
    """one output channel of the last block's transposed convolution is zero (the 96-wide block on the narrow shape)"""
    return _ct(W, t, len(W.blocks) - 1, zero_ch=17)


def m_snake_param_neighbour(W, t):
    """one channel's SnakeBeta alpha / 1/beta is taken from the neighbouring unit"""
    b, C_ = 2, W.blocks[2][2]
    ea, ib = (a.copy() for a in W.snake(VR.VC_BLK + 4 * b + 2, VR.VW_ALPHA, VR.VW_BETA, C_))
    ea2, ib2 = W.snake(VR.VC_BLK + 4 * b + 3, VR.VW_ALPHA, VR.VW_BETA, C_)
    ea[5], ib[5] = ea2[5], ib2[5]
    o = t[f"b{b}.r0.o"][0].astype(np.float64)
    y = VR.snake64(o, ea, ib).astype(np.float32)
    return f"b{b}.r1.c1_in", np.concatenate([t[f"b{b}.r1.c1_in"][0][:t[f"b{b}.r1.c1_in"][1]], VR.bf16_bits(y)]), 302 + 20 * b + 4, y, f"b{b}.r0 snake -> b{b}.r1.c1_in"


def m_snake_before_bias(W, t):
    """SnakeBeta applied before instead of after the bias (decoder input convolution)"""
    ch = W.blocks[0][1]
    w, bias = W.conv(VR.VC_DEC_IN, VR.VW_W, VR.VW_B, 7, W.d, ch, ch, 1.0)
    x, H = _f(t, "dec_in.in")
    acc, _ = VR.conv64(x, H, w, 1)
    ea, ib = W.snake(VR.VC_BLK, VR.VW_ALPHA, VR.VW_BETA, ch)
    y = (VR.snake64(acc, ea, ib) + bias).astype(np.float32)
    return "b0.ct_in", np.concatenate([t["b0.ct_in"][0][:1], VR.bf16_bits(y)]), 300, y, "dec_in + snake"


def m_residual_tile_twice(W, t):
    """the residual of one 16-row tile is added twice"""
    b = len(W.blocks) - 1
    o = t[f"b{b}.r0.o"][0].copy()
    o[32:48] += o[32:48] - t[f"b{b}.o_ct"][0][32:48]
    return f"b{b}.r0.o", o, 305 + 20 * b, o, f"b{b}.r0.o"


def _dw_ln(W, t, u, unbiased=False, reverse=False):
    d, comp = W.d, VR.VC_UP + u
    dw_w, dw_b = W.vec(comp, VR.VW_DW_W, 7 * d, 0.0, 0.3).reshape(7, d), W.vec(comp, VR.VW_DW_B, d, 0.0, 0.02)
    ln_w, ln_b = W.vec(comp, VR.VW_LN_W, d, 1.0, 0.05), W.vec(comp, VR.VW_LN_B, d, 0.0, 0.02)
    if reverse:
        dw_w = dw_w[::-1]
    raw, H = t[f"up{u}.raw"]
    x, T = raw.astype(np.float64), raw.shape[0] - H
    dw = np.tile(dw_b, (T, 1))
    for tap in range(7):
        dw += x[H - 6 + tap:H - 6 + tap + T] * dw_w[tap]
    z = dw - dw.mean(axis=1, keepdims=True)
    var = (z * z).sum(axis=1, keepdims=True) / (d - 1 if unbiased else d)
    y = (z / np.sqrt(var + 1e-6) * ln_w + ln_b).astype(np.float32)
    return f"up{u}.ln", y, 102 + 10 * u, y, f"up{u}.dw_ln"


def m_layernorm_unbiased_variance(W, t):
    """LayerNorm of k_voc_dw_ln with the unbiased variance (d - 1) instead of the biased one"""
    return _dw_ln(W, t, 1, unbiased=True)


def m_depthwise_reversed(W, t):
    """the depthwise kernel reversed in time"""
    return _dw_ln(W, t, 0, reverse=True)


MUTATIONS = [m_dilated_tap_row_late, m_ct_phase_other_tap, m_ct_bias_not_repeating, m_snake_param_neighbour, m_snake_before_bias,
             m_residual_tile_twice, m_zero_channel, m_layernorm_unbiased_variance, m_depthwise_reversed]


@pytest.mark.parametrize("mut", MUTATIONS, ids=lambda f: f.__name__[2:])
def test_stage_check_sees(voc, mut):
    shape, W, codes, taps = voc
    R = _oracle.VOC_STAGE_R[voc[0]]
    name, wrong, inj_stage, inj, stage = mut(W, taps)
    assert wrong.shape == taps[name][0].shape and wrong.dtype == taps[name][0].dtype, (name, wrong.shape, taps[name][0].shape)
    bad = dict(taps)
    bad[name] = (wrong, taps[name][1])
    ratio = {s: r for s, r, _ in VR.check_call(W, bad, R)}[stage]
    n = codes.shape[0]
    spf = taps["pcm"][0].shape[0] // n
    clean = np.clip(VR.oracle_stage(W, codes, 4, (n * spf, 1)), -1, 1)
    dirty = np.clip(VR.oracle_stage(W, codes, 4, (n * spf, 1), inject=(inj_stage, inj)), -1, 1)
    rms = float(np.sqrt(np.mean((dirty.astype(np.float64) - clean) ** 2)))
    print(f"\n{voc[0]}: {mut.__doc__}: stage '{stage}' at {ratio:.3g} x its bound; through the oracle to the PCM: RMS {rms:.2e} -> the whole-signal "
          f"criterion (<= {PCM_RMS_TOL:.0e}) {'would have let it through' if rms <= PCM_RMS_TOL else 'would have caught it'}")
    assert rms > 0.0, "the injected stage did not reach the PCM"
    assert ratio >= 10.0, (stage, ratio)

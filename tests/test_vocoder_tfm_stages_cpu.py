"""The stage-by-stage float64 check of the vocoder's front half (tests/_voc_tfm_ref.py, used on the device by
tests/test_vocoder_tfm_stages_gpu.py) can fail: proven here on the CPU.

The bf16-input oracle's own stage data, cut into calls of 4 frames in the device's tap format, passes every stage (this also checks the
numpy references against oracle/q3_oracle_vocoder.c). Then one tap of a call past the window and once round the ring is replaced by what a
plausible kernel bug would have written; each must be reported at its own stage with a ratio above 1."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _oracle  # noqa: E402
import _voc_ref as VR  # noqa: E402
import _voc_tfm_ref as TR  # noqa: E402

N, POS0, NF = 28, 24, 4   # the call under test: past the window and the ring's length at both shapes, so pos % RW has wrapped


@pytest.fixture(scope="module", params=["tiny", "hd128"])
def tfm(request):
    from q3tts import _abi
    L = TR.bind(_oracle.lib())
    vc = TR.shape_vocoder(_abi.tiny_config(max_batch=1, n_ctx=128, with_vocoder=1).vocoder, request.param)
    v = L.q3o_vocoder_create(C.byref(vc), 0, 4)
    W = VR.Weights(L, v, vc)
    codes = np.random.default_rng(9).integers(0, vc.codebook_size, size=(N, 16)).astype(np.int32)
    codes[POS0 + 1, 3], codes[POS0 + 1, 7], codes[POS0 + 2, 0], codes[2, 5] = -3, vc.codebook_size + 5, vc.codebook_size, -1
    S = TR.oracle_stages(W, codes)
    yield request.param, W, codes, S
    L.q3o_vocoder_destroy(v)


def test_oracle_stage_data_passes_every_stage(tfm):
    shape, W, codes, S = tfm
    R, D = _oracle.VOC_STAGE_R[shape], TR.Dims(W.vc)
    assert POS0 - D.W + 1 >= D.RW
    worst, prev = {}, None
    for pos0 in range(0, N, 4):
        taps = TR.oracle_call_taps(W, S, pos0, 4)
        for stage, ratio, where in TR.check_tfm_call(W, taps, R, pos0, codes[pos0:pos0 + 4]):
            worst[stage] = max(worst.get(stage, 0.0), ratio)
        if prev is not None:
            rc = TR.ring_carry(W, prev, taps, pos0)
            assert len(rc) == 2 * D.nl and all(ok for _, ok in rc)
        prev = taps
    print(f"\n{shape}: worst error / bound per stage over the calls of {N} frames")
    for stage, ratio in worst.items():
        print(f"  {stage:44s} {ratio:6.3f}")
    assert all(r <= 1.0 for r in worst.values()), {s: r for s, r in worst.items() if not r <= 1.0}
    # a 1-frame and a 3-frame call pass too, and the carry check sees one changed row of an earlier position
    for pos0, nf in ((8, 1), (9, 3)):
        res = TR.check_tfm_call(W, TR.oracle_call_taps(W, S, pos0, nf), R, pos0, codes[pos0:pos0 + nf])
        assert all(r <= 1.0 for _, r, _ in res), [(s, r) for s, r, _ in res if not r <= 1.0]
    bad = dict(prev)
    a = prev["l1.vring"][0].copy()
    a[(POS0 - 1) % D.RW, 3] += 1.0
    bad["l1.vring"] = (a, 0)
    assert [k for k, ok in TR.ring_carry(W, TR.oracle_call_taps(W, S, POS0 - 4, 4), bad, POS0) if not ok] == ["l1.vring"]


# ---- deliberately wrong taps: each returns (tap name, wrong array, the stage that must report it) ------------------------------------------
def _q64(W, t, l):
    D = TR.Dims(W.vc)
    return TR.rope64(D, t[f"l{l}.qkv"][0][:, :D.HH], POS0 + np.arange(NF))[0]


def _att(W, S, t, l, **kw):
    D = TR.Dims(W.vc)
    att = TR.attend64(D, _q64(W, t, l), t[f"l{l}.kring"][0], t[f"l{l}.vring"][0], POS0, **kw)[0]
    return f"l{l}.att", VR.bf16_bits(att.astype(np.float32)), f"l{l}.attn"


def m_window_one_short(W, S, t):
    """the window is W - 1 at a position past the window"""
    return _att(W, S, t, 1, window=W.vc.sliding_window - 1)


def m_window_one_long(W, S, t):
    """the window is W + 1 at a position past the window"""
    return _att(W, S, t, 0, window=W.vc.sliding_window + 1)


def m_stale_oldest_ring_row(W, S, t):
    """the oldest ring row of the window is stale: it holds the row RW positions older"""
    D = TR.Dims(W.vc)
    return _att(W, S, t, 1, oldest=lambda j0: (S["l1.kr"][j0 - D.RW].astype(np.float64), S["l1.v"][j0 - D.RW].astype(np.float64)))


def _kring(W, t, l, pos, **kw):
    D = TR.Dims(W.vc)
    ring = t[f"l{l}.kring"][0].copy()
    ring[(POS0 + np.arange(NF)) % D.RW] = TR.rope64(D, t[f"l{l}.qkv"][0][:, D.HH:2 * D.HH], pos, **kw)[0].astype(np.float32)
    return f"l{l}.kring", ring, f"l{l}.rope k"


def m_rope_first_position_for_all(W, S, t):
    """every token of a 4-frame call is rotated with the call's first position"""
    return _kring(W, t, 0, np.full(NF, POS0))


def m_rope_interleaved_pairs(W, S, t):
    """rotary pairs are taken interleaved instead of half-split"""
    return _kring(W, t, 1, POS0 + np.arange(NF), interleaved=True)


def m_head_scale_of_other_head_dim(W, S, t):
    """one head uses the 1 / sqrt(hd) of another hd"""
    return _att(W, S, t, 0, scale_hd={1: 2 * W.vc.head_dim})


def m_softmax_sum_misses_last_key(W, S, t):
    """the softmax denominator misses the last key"""
    return _att(W, S, t, 1, drop_last_in_sum=True)


def m_layer_scales_swapped(W, S, t):
    """ls_attn and ls_mlp are swapped"""
    P = TR.layer(W, 0)
    acc = TR.gemm64(VR.operand(t["l0.att"][0]), P["o"])[0]
    return "l0.x_att", (t["x0"][0].astype(np.float64) + P["ls_mlp"] * acc).astype(np.float32), "l0.o"


def m_gate_up_swapped(W, S, t):
    """gate and up are swapped in SwiGLU"""
    P, x = TR.layer(W, 1), VR.operand(t["l1.xn2"][0])
    g = TR.swiglu64(TR.gemm64(x, P["up"])[0], TR.gemm64(x, P["gate"])[0])
    return "l1.g", VR.bf16_bits(g.astype(np.float32)), "l1.gu"


def m_rmsnorm_divides_by_d_minus_1(W, S, t):
    """RMSNorm divides by d - 1"""
    D = TR.Dims(W.vc)
    y = TR.rms64(t["x0"][0], TR.layer(W, 0)["in_norm"], D.eps, div=D.d - 1)[0]
    return "l0.xn", VR.bf16_bits(y.astype(np.float32)), "l0.in_norm"


def m_preconv_history_one_row_late(W, S, t):
    """the pre-conv reads its history rows one row late"""
    D = TR.Dims(W.vc)
    emb, H = t["emb"]
    x = VR.operand(emb)
    x[:H] = x[1:H + 1]
    w, b = W.conv(TR.VC_PRE, TR.VW_W, TR.VW_B, D.K, D.cd, D.d, D.d, 1.0)
    return "x0", (VR.conv64(x, H, w, 1)[0] + b).astype(np.float32), "pre"


def _emb(W, t, codes, **kw):
    emb, H = t["emb"]
    emb = emb.copy()
    emb[H:] = TR.embed_f32(W, codes[POS0:POS0 + NF], **kw)
    return "emb", emb, "emb"


def m_codebook_left_out(W, S, t, codes):
    """one codebook is left out of the embedding sum"""
    return _emb(W, t, codes, skip=11)


def m_out_of_range_code_wraps(W, S, t, codes):
    """an out-of-range code wraps instead of clamping"""
    return _emb(W, t, codes, wrap=True)


MUTATIONS = [m_window_one_short, m_window_one_long, m_stale_oldest_ring_row, m_rope_first_position_for_all, m_rope_interleaved_pairs,
             m_head_scale_of_other_head_dim, m_softmax_sum_misses_last_key, m_layer_scales_swapped, m_gate_up_swapped,
             m_rmsnorm_divides_by_d_minus_1, m_preconv_history_one_row_late, m_codebook_left_out, m_out_of_range_code_wraps]


@pytest.mark.parametrize("mut", MUTATIONS, ids=lambda f: f.__name__[2:])
def test_tfm_stage_check_sees(tfm, mut):
    shape, W, codes, S = tfm
    R = _oracle.VOC_STAGE_R[shape]
    taps = TR.oracle_call_taps(W, S, POS0, NF)
    name, wrong, stage = mut(W, S, taps, codes) if mut.__code__.co_argcount == 4 else mut(W, S, taps)
    assert wrong.shape == taps[name][0].shape and wrong.dtype == taps[name][0].dtype, (name, wrong.shape, wrong.dtype)
    assert not np.array_equal(wrong, taps[name][0])
    bad = dict(taps)
    bad[name] = (wrong, taps[name][1])
    clean = {s: r for s, r, _ in TR.check_tfm_call(W, taps, R, POS0, codes[POS0:POS0 + NF])}
    ratio = {s: r for s, r, _ in TR.check_tfm_call(W, bad, R, POS0, codes[POS0:POS0 + NF])}
    print(f"\n{shape}: {mut.__doc__}: stage '{stage}' at {ratio[stage]:.3g} x its bound (the oracle's own tap: {clean[stage]:.3g})")
    assert clean[stage] <= 1.0 and ratio[stage] > 1.0, (stage, clean[stage], ratio[stage])

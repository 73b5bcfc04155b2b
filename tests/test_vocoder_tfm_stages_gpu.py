"""The vocoder's front half on the device, stage by stage against float64 (tests/_voc_tfm_ref.py): embedding sum, pre-conv, and per transformer
layer the norms, the four projections, RoPE, the K / V ring and the sliding-window attention.

Every stage's input is the device's own tapped operand (q3tts_k_vocoder_taps: the production launches, copies taken in between), so nothing
compounds and LayerScale damps nothing; every output element is judged on its own against 4x the error of the CPU restatement
(tests/_oracle.py VOC_STAGE_R) plus the element-wise terms written in _voc_tfm_ref. Shapes (_voc_tfm_ref.SHAPES): tiny (k_vgemm_small,
k_voc_attn_lds), hd128 and hd64t (A-tiled bf16 into k_bgemm; k_voc_attn with two full score trips / the LDS kernel), hd96 (a partial second
trip), hd48 (LDS row stride 49), w1 (one key, a ring of 5 rows), w508 (the largest window: 508 keys, no LDS kernel, the ring wraps at 512),
full (all 8 layers, in two groups). Drives: one shot of 1 and 4 frames, 1-frame and 3-frame calls tapped on the first, the second and two
calls past W + 4 positions, one call with out-of-range codes; w508 and full add a drive of 4-frame calls tapped at the window and ring edges
(_drives). The ring rows a call did not write equal the previous call's bit for bit, and Q3TTS_VOC_ATTN_OLD=1 gives the same taps bit for
bit on the calls where it selects another kernel (_lds_default). q3tts_engine_create accepts head_dim 96 and 48 as they are."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _voc_ref as VR  # noqa: E402
import _voc_tfm_ref as TR  # noqa: E402
import test_vocoder_stages_gpu as SG  # noqa: E402  (its _shape("full"), _env, _same, _report)
from _oracle import VOC_STAGE_R  # noqa: E402

pytestmark = pytest.mark.gpu

CASES = [(s, None) for s in TR.SHAPES] + [("full", (0, 1, 2, 3)), ("full", (4, 5, 6, 7))]
LDS_SHAPES = ("tiny", "hd64t", "hd48", "w1", "full")   # the shapes that are here to run k_voc_attn_lds, at every call size


def _lds_default(vc, nf):
    """voc_launch_attn's rule for a call of nf frames: k_voc_attn_lds unless Q3TTS_VOC_ATTN_OLD=1 (then k_voc_attn, as for every other shape)."""
    return vc.head_dim <= 64 and vc.head_dim % 4 == 0 and (vc.sliding_window + nf - 1) * (2 * vc.head_dim + 1) * 4 <= 48 * 1024


def _cfg(shape):
    from q3tts import _abi
    if shape == "full":
        return SG._shape("full")
    cfg = _abi.tiny_config(max_batch=2, n_ctx=2048 if shape == "w508" else 128, with_vocoder=1)
    TR.shape_vocoder(cfg.vocoder, shape)
    if shape == "w508":
        cfg.max_steps_cap = 1040   # (< n_ctx): the drive goes to position 567
    return cfg


def _calls(n, chunk):
    """[(first frame, frames)] of the drive's calls: chunks of chunk_frames, calls of at most 4 frames inside a chunk."""
    out, chunk = [], chunk if chunk > 0 else n
    for f in range(0, n, chunk):
        end = min(f + chunk, n)
        while f < end:
            out.append((f, min(4, end - f)))
            f += out[-1][1]
    return out


def _drives(shape, Wn):
    """[(frames, chunk_frames, tapped calls, out-of-range codes)]"""
    c3 = (Wn + 4) // 3 + 2   # the 3-frame call whose first position is past W + 4
    d = [(1, 0, (0,), False), (4, 0, (0,), False), (4, 0, (0,), True),
         (Wn + 8, 1, (0, 1, Wn + 5, Wn + 6), False), (3 * (c3 + 1), 3, (0, 1, c3 - 1, c3), False)]
    if shape == "w508":
        # position 0; nk = 505 .. 508 (positions 504 .. 507); 508 .. 511; the first call past 512, where pos % RW wraps; a later one
        d.append((568, 4, (0, 126, 127, 128, 140), False))
    if shape == "full":
        # 4 + 3 frame calls: position 0; 18 .. 20 inside the window; 70 .. 73 across 71 / 72 (the first key leaves the window);
        # 74 .. 76 across the ring's end (RW = 76); 77 .. 80 past it
        d.append((84, 7, (0, 5, 20, 21, 22), False))
    return d


@pytest.mark.parametrize("shape,layers", CASES, ids=[s if g is None else f"{s}-l{g[0]}..{g[-1]}" for s, g in CASES])
def test_vocoder_tfm_stages_vs_float64(oracle, shape, layers):
    from q3tts import native
    cfg = _cfg(shape)
    vc = cfg.vocoder
    L = TR.bind(oracle.lib())
    v = L.q3o_vocoder_create(C.byref(vc), 0, 4)
    eng = native.NativeEngine(cfg)
    try:
        W, R, D = VR.Weights(L, v, vc), VOC_STAGE_R[shape], TR.Dims(vc)
        rng = np.random.default_rng(78)
        codes = rng.integers(0, vc.codebook_size, size=(max(n for n, _, _, _ in _drives(shape, D.W)), 16)).astype(np.int32)
        oor = codes.copy()
        oor[0, 2], oor[1, 0], oor[1, 15], oor[3, 7], oor[2, 9] = -1, vc.codebook_size, -2 ** 31, 2 ** 31 - 1, vc.codebook_size + 7
        worst, carries, same_old = {}, 0, 0
        for n, chunk, tapped, with_oor in _drives(shape, D.W):
            cd = (oor if with_oor else codes)[:n]
            calls, prev, prev_call = _calls(n, chunk), None, None
            for call in tapped:
                pos0, nf = calls[call]
                taps = eng.vocoder_taps(cd, chunk_frames=chunk, tap_call=call)
                res = TR.check_tfm_call(W, taps, R, pos0, cd[pos0:pos0 + nf], layers)
                SG._report(worst, res)
                bad = [(s, r, w) for s, r, w in res if not r <= 1.0]
                assert not bad, (shape, n, chunk, call, pos0, bad)
                if prev_call == call - 1:   # every ring row this call did not write: the previous call's, bit for bit
                    rc = TR.ring_carry(W, prev, taps, pos0)
                    assert len(rc) == 2 * D.nl and all(ok for _, ok in rc), (shape, n, chunk, call, [k for k, ok in rc if not ok])
                    carries += len(rc)
                prev, prev_call = taps, call
                assert _lds_default(vc, nf) == (shape in LDS_SHAPES), (shape, nf)   # the shape runs the attention kernel it is here for
                if _lds_default(vc, nf):
                    with SG._env({"Q3TTS_VOC_ATTN_OLD": "1"}):
                        other = eng.vocoder_taps(cd, chunk_frames=chunk, tap_call=call)
                    assert SG._same(taps, other), (shape, n, chunk, call, "Q3TTS_VOC_ATTN_OLD=1")
                    same_old += 1
        print(f"\n{shape}{'' if layers is None else ' layers ' + str(layers)}: worst error / bound per stage over all drives; {carries} ring carries "
              f"bit for bit; {same_old} calls with Q3TTS_VOC_ATTN_OLD=1 bit for bit")
        for stage in worst:
            print(f"  {stage:44s} {worst[stage][0]:7.3f} at {worst[stage][1]}")
    finally:
        eng.close()
        L.q3o_vocoder_destroy(v)

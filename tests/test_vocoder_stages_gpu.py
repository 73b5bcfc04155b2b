"""The vocoder's convolution half on the device, stage by stage against float64 (tests/_voc_ref.py).

Every stage's input is the device's own operand buffer (q3tts_k_vocoder_taps: the production launches, copies taken in between), so nothing
compounds from stage to stage and every output element is judged on its own against 4x the error of the instruction model's chain
(tests/_oracle.py VOC_STAGE_R, measured on the CPU). Shapes: the tiny vocoder, the narrow-block shape (fused residual units, the 96-wide
tile), the full shape. Drives: one shot of 1 and 4 frames, a 9-frame one shot (split 4 + 4 + 1), chunked 1 / 3 / 4 with taps on the first,
the second and a later call; random codes and one repeated frame. Launch switches: taps bit for bit equal to the default's (except the PCM
of Q3TTS_VOC_OUT_OLD=1, a kernel with another documented summation order, which is judged against float64 itself). Histories: carried
from call to call bit for bit."""
import contextlib
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _voc_ref as VR  # noqa: E402
from _oracle import VOC_STAGE_R  # noqa: E402

pytestmark = pytest.mark.gpu

# (n_frames, chunk_frames, tapped calls): history empty, partly filled (block 0's 54-row history of dilation 9 needs two 1-frame calls), full
DRIVES = [(1, 0, (0,)), (4, 0, (0,)), (9, 0, (2,)), (6, 1, (0, 1, 2, 4)), (10, 3, (0, 1, 3)), (12, 4, (0, 1, 2))]
SWITCHES = [{"Q3TTS_VOC_NOFUSE": "1"}, {"Q3TTS_VOC_NORING": "1"}, {"Q3TTS_VOC_NOTAP": "1"}, {"Q3TTS_VOC_TAP_MIN": "1"}, {"Q3TTS_VOC_POLITE": "1"},
            {"Q3TTS_VOC_OUT_OLD": "1"}, {"Q3TTS_VOC_POLITE": "1", "Q3TTS_VOC_TAP_MIN": "1"}]


@contextlib.contextmanager
def _env(kv):
    old = {k: os.environ.get(k) for k in kv}
    os.environ.update(kv)
    try:
        yield
    finally:
        for k, val in old.items():
            if val is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = val


def _shape(name):
    from q3tts import _abi
    if name == "full":
        cfg = _abi.full_config_py()
        cfg.max_batch, cfg.n_ctx, cfg.max_steps_cap = 1, 256, 160
        cfg.model.t_n_layer, cfg.model.p_n_layer = 1, 1   # the decoder is not under test here
        return cfg
    cfg = _abi.tiny_config(max_batch=2, n_ctx=128, with_vocoder=1)
    if name == "narrow":   # tests/test_parity_gpu.py::test_vocoder_narrow_block_kernels
        vc = cfg.vocoder
        vc.decoder_dim, vc.n_dec_blocks = 768, 3
        for i, r in enumerate((8, 5, 3)):
            vc.dec_rates[i] = r
    return cfg


def _same(a, b):
    return set(a) == set(b) and all(a[k][1] == b[k][1] and a[k][0].dtype == b[k][0].dtype and np.array_equal(a[k][0].view(np.uint8), b[k][0].view(np.uint8)) for k in a)


def _report(worst, stage_results):
    for stage, ratio, where in stage_results:
        if ratio >= worst.get(stage, (-1.0,))[0]:
            worst[stage] = (ratio, where)


@pytest.mark.parametrize("shape", ["tiny", "narrow", "full"])
def test_vocoder_stages_vs_float64(oracle, shape):
    from q3tts import native
    cfg = _shape(shape)
    vc = cfg.vocoder
    L = VR.bind(oracle.lib())
    v = L.q3o_vocoder_create(C.byref(vc), 0, 4)
    eng = native.NativeEngine(cfg)
    try:
        W, R = VR.Weights(L, v, vc), VOC_STAGE_R[shape]
        rng = np.random.default_rng(77)
        codes = rng.integers(0, vc.codebook_size, size=(12, 16)).astype(np.int32)
        flat = np.repeat(codes[:1], 12, axis=0)   # one frame repeated: a constant latent, a wrong phase or tap shows as structure
        worst, worst_nf, worst_old, carries = {}, {}, {}, 0
        for n, chunk, calls in DRIVES:
            prev, prev_call = None, None
            for call in calls:
                taps = eng.vocoder_taps(codes[:n], chunk_frames=chunk, tap_call=call)
                res = VR.check_call(W, taps, R)
                _report(worst, res)
                bad = [(s, r, w) for s, r, w in res if not r <= 1.0]
                assert not bad, (shape, n, chunk, call, bad)
                # histories: zeros after the reset, otherwise the last H rows of the same buffer one call earlier, bit for bit
                if call == 0 or prev_call == call - 1:
                    hc = VR.history_carry(None if call == 0 else prev, taps)
                    assert hc and all(ok for _, ok in hc), (shape, n, chunk, call, [k for k, ok in hc if not ok])
                    carries += len(hc)
                prev, prev_call = taps, call
                if (n, chunk, call) in ((4, 0, 0), (10, 3, 1), (6, 1, 2)):
                    # every launch switch that selects another kernel for the same stage: the same taps, bit for bit
                    for sw in SWITCHES:
                        with _env(sw):
                            other = eng.vocoder_taps(codes[:n], chunk_frames=chunk, tap_call=call)
                        if "Q3TTS_VOC_NOFUSE" in sw or "Q3TTS_VOC_OUT_OLD" in sw:
                            # the un-fused units are judged on their own z as well. k_voc_out sums in another order than k_voc_out8 by
                            # design (its header comment), so its PCM is judged against float64 like the default's, not against the default
                            res = VR.check_call(W, other, R)
                            _report(worst_nf if "Q3TTS_VOC_NOFUSE" in sw else worst_old, res)
                            bad = [(s, r, w) for s, r, w in res if not r <= 1.0]
                            assert not bad, (shape, n, chunk, call, sw, bad)
                            other = {k: a for k, a in other.items() if k in taps and not (k == "pcm" and "Q3TTS_VOC_OUT_OLD" in sw)}
                        assert len(other) >= len(taps) - 1
                        assert _same({k: a for k, a in taps.items() if k in other}, other), (shape, n, chunk, call, sw)
        for n, chunk, call in ((8, 4, 1), (3, 1, 2)):
            res = VR.check_call(W, eng.vocoder_taps(flat[:n], chunk_frames=chunk, tap_call=call), R)
            _report(worst, res)
            bad = [(s, r, w) for s, r, w in res if not r <= 1.0]
            assert not bad, (shape, "repeated frame", n, chunk, call, bad)
        print(f"\n{shape}: worst error / bound per stage over all drives (default launches | Q3TTS_VOC_NOFUSE=1); {carries} history carries bit for bit")
        for stage in worst:
            nf = worst_nf.get(stage)
            print(f"  {stage:44s} {worst[stage][0]:7.3f} at {worst[stage][1]}" + (f" | {nf[0]:7.3f}" if nf else ""))
        print(f"  {'out conv + clamp (Q3TTS_VOC_OUT_OLD=1)':44s} {worst_old['out conv + clamp'][0]:7.3f}")
        for stage in worst_nf:
            if stage not in worst:
                print(f"  {stage:44s}       - | {worst_nf[stage][0]:7.3f} at {worst_nf[stage][1]}")
        # the transposed convolutions' f32 output before any transcendental against the instruction model's chain itself
        taps = eng.vocoder_taps(codes[:4], chunk_frames=0, tap_call=0)
        for bi, (r, cin, cout) in enumerate(W.blocks):
            w, b = W.conv(VR.VC_BLK + 4 * bi, VR.VW_W, VR.VW_B, 2, cin, r * cout, cout, 1.0)
            x, H = taps[f"b{bi}.ct_in"]
            chain = VR.mfma_chain(W, x, H, w, 1, max_rows=8)
            want = (chain + np.tile(b, r).astype(np.float32)[None, :]).astype(np.float32).reshape(-1, cout)
            got = taps[f"b{bi}.o_ct"][0][:want.shape[0]]
            same = int(np.count_nonzero(got.view(np.uint32) == want.view(np.uint32)))
            print(f"  b{bi}.ct == chain of q3o_mfma_bf16_dot32 + bias (f32): {same} of {want.size} elements bit for bit")
            assert same == want.size, (shape, bi, same, want.size)
    finally:
        eng.close()
        L.q3o_vocoder_destroy(v)

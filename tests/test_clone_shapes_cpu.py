"""The clone-encoder oracle against the model family's own modules at the shapes of tests/_clone_shapes.py.

tests/test_clone_family_cpu.py's two comparisons (floats to 2e-5 of the larger of 1 and the largest reference magnitude, codec ids equal in at
least 0.99 of the entries), on the clips tests/test_clone_shapes_gpu.py compares device and oracle on: if those two ever disagree at a shape,
this file says which of them restates the model wrongly. The family code is the installed transformers package (tests/_clone_family.py).

The 0.99 on the ids is a cap on near-ties, not a measurement: a residual VQ turns one flipped id into a different residual for every later
codebook of the frame. So for every clip the family module in float32 must meet the same 0.99 against ITSELF in float64, with no oracle
involved; the clips' seeds (clip(n, n), as the GPU tests use them) were chosen so that it does, and that is asserted first.

Measured here (largest over the table): oracle against family f32 1.5e-6 at every shape but rope_edge, 1.5e-5 at rope_edge, where the family
evaluates its rotary angles in f32 (position 16 383 x 2^-24 is 1e-3 rad) and the oracle and the engine tabulate them in double; the family's
own f32-against-f64 error is 1.2e-6. Every id agreed in all three pairings. All figures are inside the 2e-5 the tiny config is held to, so no
shape needed a bound of its own.

Not expressible by the family's modules, skipped by name below: codebook sizes that are no power of two (MimiModel refuses them), one
codebook (MimiConfig wants more quantizers than semantic ones), ae_down_stride 3 (MimiModel's frame-rate convolution has stride 2 written in),
and speaker clips no longer than the widest reflect padding (torch's reflect mode refuses them; the oracle and the engine clamp).
"""
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import _clone_shapes as S

TOL = 2e-5

AUDIO_INEXPRESSIBLE = {
    "down3": "MimiModel's frame-rate convolution has stride 2 written in",
    "vq1x16x1": "MimiConfig requires num_quantizers > num_semantic_quantizers = 1",
    "vq63x16x2": "MimiModel refuses a codebook size that is no power of two",
    "vq1000x48x3": "MimiModel refuses a codebook size that is no power of two",
    "vq1025x16x64": "MimiModel refuses a codebook size that is no power of two",
    "vq2049x32x3": "MimiModel refuses a codebook size that is no power of two",
    "vq3000x48x3": "MimiModel refuses a codebook size that is no power of two",
    "vq5000x272x2": "MimiModel refuses a codebook size that is no power of two",
}


@functools.lru_cache(maxsize=2)
def _mimi(name):
    import _clone_family as F
    m = F.mimi(S.audio_config(name), max_rows=S.ROPE_MAX_T)
    return m, F.to_float64(m)


@functools.lru_cache(maxsize=2)
def _ecapa(name):
    import _clone_family as F
    return F.ecapa(S.speaker_config(name))


def test_the_skip_list_is_exactly_what_the_family_cannot_express():
    for name in S.AUDIO:
        c = S.audio_config(name)
        cs = c.ae_codebook_size
        inexpressible = c.ae_down_stride != 2 or c.ae_n_codebooks < 2 or (cs & (cs - 1)) != 0
        assert inexpressible == (name in AUDIO_INEXPRESSIBLE), name


_AUDIO_CLIPS = sorted({(name, n) for name, _, n in S.audio_cases()}, key=lambda c: (list(S.AUDIO).index(c[0]), c[1]))


@pytest.mark.parametrize("name,n", _AUDIO_CLIPS, ids=["%s-n%d" % c for c in _AUDIO_CLIPS])
def test_audio_oracle_equals_family_mimi_encoder_at_shapes(oracle, name, n):
    if name in AUDIO_INEXPRESSIBLE:
        pytest.skip(AUDIO_INEXPRESSIBLE[name])
    import _clone_family as F
    m, m64 = _mimi(name)
    a = S.clip(n, n)
    lat, codes = F.mimi_run(m, a)
    lat64, codes64 = F.mimi_run(m64, a)
    assert (codes == codes64).mean() >= 0.99, "the family's own f32 ids leave its f64 ids on this clip: choose another seed"
    codes_ref, lat_ref = S.audio_ref(name, n)
    scale = max(1.0, np.abs(lat_ref).max())
    print("%s n %d: oracle vs family f32 %.2e, family f32 vs f64 %.2e (x %.1f); ids %.4f" % (
        name, n, np.abs(lat - lat_ref).max() / scale, np.abs(lat - lat64).max() / scale, scale, (codes == codes_ref).mean()))
    assert lat.shape == lat_ref.shape and np.abs(lat - lat_ref).max() <= TOL * scale
    assert (codes == codes_ref).mean() >= 0.99


_SPEAKER_CLIPS = sorted({(name, T) for name, _, T in S.speaker_cases()}, key=lambda c: (list(S.SPEAKER).index(c[0]), c[1]))


@pytest.mark.parametrize("name,T", _SPEAKER_CLIPS, ids=["%s-T%d" % c for c in _SPEAKER_CLIPS])
def test_speaker_oracle_equals_family_ecapa_at_shapes(oracle, name, T):
    import _clone_family as F
    pad = F.speaker_reflect_pad(S.speaker_config(name))
    if T <= pad:
        pytest.skip("torch's reflect padding needs more than %d frames at this shape" % pad)
    out = F.ecapa_run(_ecapa(name), S.mel(T))
    ref = S.speaker_ref(name, T)
    print("%s T %d: oracle vs family f32 %.2e" % (name, T, np.abs(out - ref).max() / max(1.0, np.abs(ref).max())))
    assert np.abs(out - ref).max() <= TOL * max(1.0, np.abs(ref).max())

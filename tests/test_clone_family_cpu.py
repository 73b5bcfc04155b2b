"""The clone-encoder oracle (oracle/q3_oracle_clone.c) against the model family's own code.

The reference's encoder graphs are ONNX files outside its repository, so nothing of the reference pins their arithmetic
(PARITY UNPINNED). What can be pinned is that the oracle restates the family structure correctly: this container's
transformers package holds that structure as plain PyTorch — ECAPA_TimeDelayNet (qwen2_5_omni) for the speaker encoder
and MimiModel's encoder / encoder_transformer / downsample / quantizer for the audio encoder. The tests load the oracle's
seeded synthetic weights into those modules (tests/_clone_family.py) and compare outputs: floats to 2e-5 (torch's conv / matmul summation order vs
the canonical order; measured 3e-6), codec ids equal. CPU only.
"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")


def test_speaker_oracle_equals_family_ecapa(oracle):
    O = oracle
    from q3tts import _abi
    import _clone_family as F
    c = _abi.tiny_clone_config()
    m = F.ecapa(c)
    rng = np.random.default_rng(0)
    for T in (7, 60):
        mel = (rng.standard_normal((T, 128)) * 2 - 4).astype(np.float32)
        ref = O.speaker_encode(c, 0, mel)
        out = F.ecapa_run(m, mel)
        assert np.abs(out - ref).max() <= 2e-5 * max(1.0, np.abs(ref).max()), T


def test_audio_oracle_equals_family_mimi_encoder(oracle):
    O = oracle
    from q3tts import _abi
    import _clone_family as F
    c = _abi.tiny_clone_config()
    m = F.mimi(c)
    rng = np.random.default_rng(0)
    for n in (5000, 24000):
        a = (rng.standard_normal(n) * 0.2).astype(np.float32)
        codes_ref, lat_ref = O.audio_encode(c, 0, a)
        lat, codes = F.mimi_run(m, a)
        assert lat.shape == lat_ref.shape and np.abs(lat - lat_ref).max() <= 2e-5 * max(1.0, np.abs(lat_ref).max()), n
        # ids can differ only at a near-tie between two codewords; with these sizes none occurs
        assert (codes == codes_ref).mean() >= 0.99, n


def test_clone_oracle_edge_cases(oracle):
    """frame arithmetic (ceil through every stride), empty / one-sample clips, one mel frame, determinism, causality"""
    import ctypes as C
    from q3tts import _abi
    c = _abi.tiny_clone_config()
    L = oracle.lib()
    for n, want in [(0, 0), (1, 1), (960, 1), (961, 1), (1920, 1), (1921, 2), (72000, 38)]:
        assert L.q3o_audio_frames(C.byref(c), n) == want, n
    codes, lat = oracle.audio_encode(c, 0, np.zeros(0, dtype=np.float32))
    assert codes.shape == (0, 16)
    rng = np.random.default_rng(1)
    a = (rng.standard_normal(9000) * 0.2).astype(np.float32)
    c1, l1 = oracle.audio_encode(c, 0, a)
    c2, l2 = oracle.audio_encode(c, 0, a)
    assert c1.shape == (5, 16) and np.array_equal(c1, c2) and np.array_equal(l1, l2)
    assert not np.array_equal(c1, oracle.audio_encode(c, 1, a)[0])  # another weight seed, another codec
    cp, _ = oracle.audio_encode(c, 0, a[:1920 * 3])
    assert np.array_equal(cp[:2], c1[:2])  # causal: a prefix of the clip gives a prefix of the codes
    e1 = oracle.speaker_encode(c, 0, np.full((1, 128), -3.0, dtype=np.float32))
    assert e1.shape == (512,) and np.isfinite(e1).all()

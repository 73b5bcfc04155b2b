"""An engine whose clone encoders come from qwen3_tts_speaker_encoder.gguf and qwen3_tts_codec_encoder.gguf computes what the
same weights give from the seeded generator and what the CPU oracle gives, bit for bit — codes and floats. The pairs are written by
tests/_clone_file.py from the oracle's synthetic encoders; the tiny shape and a second one (tests/_clone_file.py shape_b). Every clip is
short: 1 sample, a ragged 1921, 7000.
"""
import os
import struct

import numpy as np
import pytest

import _clone_file as CF
import _clone_shapes as CS

pytestmark = pytest.mark.gpu

MEL_T = (1, 5, 46)
CLIPS = (1, 1921, 7000)
SHAPES = {"tiny": CF.shape_tiny, "b": CF.shape_b}


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


_REF = {}


def _ref(oracle, shape, seed):
    """{("mel", T): embedding, ("clip", n): (codes, rows)} of the oracle at (shape, seed); computed once, shared, read-only"""
    if (shape, seed) not in _REF:
        c, r = SHAPES[shape](), {}
        for T in MEL_T:
            r[("mel", T)] = oracle.speaker_encode(c, seed, CS.mel(T))
            r[("mel", T)].setflags(write=False)
        for n in CLIPS:
            codes, lat = oracle.audio_encode(c, seed, CS.clip(n, n))
            codes.setflags(write=False); lat.setflags(write=False)
            r[("clip", n)] = (codes, lat)
        _REF[(shape, seed)] = r
    return _REF[(shape, seed)]


def _outputs(eng):
    out = {}
    for T in MEL_T:
        out[("mel", T)] = eng.speaker_from_mel(CS.mel(T))
    for n in CLIPS:
        a = CS.clip(n, n)
        out[("clip", n)] = (eng.audio_encode(a), eng.audio_latent(a))
    return out


def _assert_same(got, want):
    for T in MEL_T:
        assert np.array_equal(_bits(got[("mel", T)]), _bits(want[("mel", T)])), T
    for n in CLIPS:
        assert got[("clip", n)][0].shape == want[("clip", n)][0].shape and got[("clip", n)][0].shape[0] >= 1
        assert np.array_equal(got[("clip", n)][0], want[("clip", n)][0].astype(np.int64)), n
        assert np.array_equal(_bits(got[("clip", n)][1]), _bits(want[("clip", n)][1])), n


@pytest.fixture(scope="module")
def engine(oracle):
    """one seed-0 engine without weight files for the whole module"""
    from q3tts import _abi, native
    eng = native.NativeEngine(_abi.tiny_config(max_batch=2, n_ctx=256, with_vocoder=1))
    yield eng
    eng.close()


@pytest.mark.parametrize("container", ["bf16", "f32_perturbed"])
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_a_seed_0_pair_gives_the_bits_of_clone_init_and_of_the_oracle(oracle, engine, tmp_path, shape, container):
    """clone_load of a pair written from seed 0 on the seed-0 engine: speaker_from_mel, audio_encode and audio_latent == clone_init's on the
    same engine == the oracle's; clone_source says 2, and 1 again after clone_init. BF16 container with the files in the parent directory;
    F32 container off the bf16 values (only nearest-even rounding brings them back) in the directory itself."""
    c = SHAPES[shape]()
    wdir = tmp_path / "gguf"
    os.makedirs(wdir)
    where = tmp_path if container == "bf16" else wdir
    CF.write(where, where, c, 0, container)
    engine.clone_load(wdir)
    assert engine.clone_source == 2
    loaded = type(c).from_buffer_copy(engine.clone_cfg)
    loaded.ae_layer_scale = c.ae_layer_scale   # (a generator parameter: no file states it)
    assert bytes(loaded) == bytes(c)
    from_file = _outputs(engine)
    engine.clone_init(c)
    assert engine.clone_source == 1
    from_seed = _outputs(engine)
    _assert_same(from_file, _ref(oracle, shape, 0))
    _assert_same(from_seed, _ref(oracle, shape, 0))


@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_other_weights_are_the_files_not_the_seeds(oracle, engine, tmp_path, shape):
    """A pair written from seed 5 on the seed-0 engine: everything == the oracle at seed 5, and not seed 0's. (A loader that fell back to
    the generator would compute seed 0's.)"""
    c = SHAPES[shape]()
    CF.write(tmp_path, tmp_path, c, 5)
    engine.clone_load(tmp_path)
    assert engine.clone_source == 2
    got = _outputs(engine)
    _assert_same(got, _ref(oracle, shape, 5))
    r0 = _ref(oracle, shape, 0)
    assert not np.array_equal(got[("mel", 46)], r0[("mel", 46)])
    assert not np.array_equal(got[("clip", 7000)][1], r0[("clip", 7000)][1])
    assert not np.array_equal(got[("clip", 7000)][0], r0[("clip", 7000)][0].astype(np.int64))


def test_a_wrong_pair_is_refused_on_the_host_and_the_loaded_encoders_stay(oracle, engine, tmp_path):
    """q3tts_clone_load with a k_proj of the wrong shape, then with one file missing, then with no directory on an engine that has no
    weights_path: each is refused with its status and message, and the encoders loaded before still give their bits."""
    from q3tts import _abi
    c = CF.shape_tiny()
    good, bad = tmp_path / "good", tmp_path / "bad"
    CF.write(good, good, c, 5)
    engine.clone_load(good)
    name = "encoder_transformer.layers.1.self_attn.k_proj.weight"
    CF.write(bad, bad, c, 0, edit_codec=lambda t: t.__setitem__(name, np.zeros((128, 64), dtype=np.float32)))
    rc = engine.lib.q3tts_clone_load(engine.h, os.fsencode(str(bad)))
    msg = engine.lib.q3tts_last_error(engine.h).decode()
    assert rc == -1 and CF.CODEC_FILE in msg and f"'{name}'" in msg and "[128][64]" in msg and "[128][128]" in msg
    os.remove(bad / CF.SPK_FILE)
    with pytest.raises(_abi.Q3Error, match=CF.SPK_FILE + " not found"):
        engine.clone_load(bad)
    assert engine.lib.q3tts_clone_load(engine.h, os.fsencode(str(bad))) == -4
    assert engine.lib.q3tts_clone_load(engine.h, None) == -5 and b"weights_path" in engine.lib.q3tts_last_error(engine.h)
    assert engine.clone_source == 2
    got = {("clip", 1921): (engine.audio_encode(CS.clip(1921, 1921)), engine.audio_latent(CS.clip(1921, 1921))), ("mel", 5): engine.speaker_from_mel(CS.mel(5))}
    want = _ref(oracle, "tiny", 5)
    assert np.array_equal(got[("clip", 1921)][0], want[("clip", 1921)][0].astype(np.int64))
    assert np.array_equal(_bits(got[("clip", 1921)][1]), _bits(want[("clip", 1921)][1]))
    assert np.array_equal(_bits(got[("mel", 5)]), _bits(want[("mel", 5)]))


def test_a_session_clones_with_the_loaded_files(oracle, engine, tmp_path):
    """NativeSession.clone_voice on the engine loaded from the seed-5 pair: the seed-5 oracle's codes and embedding; q3tts_clone_load is
    refused while the session is open."""
    from q3tts import _abi, native
    c = CF.shape_tiny()
    CF.write(tmp_path, tmp_path, c, 5)
    engine.clone_load(tmp_path)
    a = CS.clip(9000, 4)
    with native.NativeSession(engine) as sess:
        codes, emb = sess.clone_voice(a)
        with pytest.raises(_abi.Q3Error):
            engine.clone_load(tmp_path)
    codes_ref, _ = oracle.audio_encode(c, 5, a)
    assert codes.shape == (5, 16) and np.array_equal(codes, codes_ref.astype(np.int64))
    assert np.array_equal(_bits(emb), _bits(oracle.speaker_encode(c, 5, engine.mel(a))))
    assert engine.clone_source == 2


def _write_wav_f32(path, samples):
    body = samples.astype("<f4").tobytes()
    hdr = b"RIFF" + struct.pack("<I", 36 + len(body)) + b"WAVE" + b"fmt " + struct.pack("<IHHIIHH", 16, 3, 1, 24000, 24000 * 4, 4, 32)
    with open(path, "wb") as f:
        f.write(hdr + b"data" + struct.pack("<I", len(body)) + body)


def test_a_model_directory_with_the_pair(oracle, tmp_path, monkeypatch):
    """TtsEngine.new on a model directory (oracle.write_model_dir) that holds the pair: the encoders are loaded from it
    (clone_is_synthetic False) and create_voice_file returns the oracle's codes and embedding bits at the pair's seed. With one file of the
    pair it raises naming the other; with a pair whose n_codebooks is not the model's it raises with both numbers; with neither nothing is
    loaded and load_clone_encoders gives the synthetic ones as before."""
    from q3tts import _abi, api
    monkeypatch.chdir(tmp_path)
    cfg = _abi.tiny_config(max_batch=1, n_ctx=128, with_vocoder=0)
    cfg.model.text_vocab = 1024   # (a small text table: no text is spoken here)
    c = _abi.tiny_clone_config(cfg.model.d_embed)
    root = tmp_path / "models"
    oracle.write_model_dir(str(root / "gguf"), cfg.model, 0, matrix_type=30, assets="gguf", with_text=True)
    a = CS.clip(9000, 4)
    _write_wav_f32(tmp_path / "ref.wav", a)
    # neither file: nothing changes
    te = api.TtsEngine.new(str(root), "none", config=cfg)
    try:
        assert te.clone_is_synthetic is False and te._native.clone_source == 0
        with pytest.raises(_abi.Q3Error, match="AudioEncoder not loaded"):
            te.create_voice_file(tmp_path / "ref.wav", [1])
        te.load_clone_encoders(c)
        assert te.clone_is_synthetic is True
    finally:
        te.close()
    # the pair, seed 5 (the model's is 0): the speaker file beside the quant directories, the codec file inside one
    CF.write(root, root / "gguf", c, 5)
    te = api.TtsEngine.new(str(root), "none", config=cfg)
    try:
        assert te.clone_is_synthetic is False and te._native.clone_source == 2
        v = te.create_voice_file(tmp_path / "ref.wav", [9, 8, 7])
        codes_ref, _ = oracle.audio_encode(c, 5, a)
        emb_ref = oracle.speaker_encode(c, 5, te._native.mel(a))
    finally:
        te.close()
    assert v.audio_codes == codes_ref.reshape(-1).tolist() and len(v.audio_codes) == 5 * 16
    assert np.array_equal(_bits(np.asarray(v.speaker_embedding, dtype=np.float32)), _bits(emb_ref))
    # one file only
    os.remove(root / CF.SPK_FILE)
    with pytest.raises(_abi.Q3Error, match=CF.SPK_FILE):
        api.TtsEngine.new(str(root), "none", config=cfg)
    os.remove(root / "gguf" / CF.CODEC_FILE)
    CF.write(root, None, c, 5)
    with pytest.raises(_abi.Q3Error, match=CF.CODEC_FILE):
        api.TtsEngine.new(str(root), "none", config=cfg)
    # a pair with 8 codebooks where the model has 16
    c8 = _abi.tiny_clone_config(cfg.model.d_embed)
    c8.ae_n_codebooks = 8
    CF.write(root, root, c8, 5)
    with pytest.raises(_abi.Q3Error, match=r"n_codebooks = 8, the model has 16"):
        api.TtsEngine.new(str(root), "none", config=cfg)

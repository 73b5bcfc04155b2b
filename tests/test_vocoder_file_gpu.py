"""An engine whose vocoder weights come from qwen3_tts_vocoder.gguf computes what the same weights give from the seeded
generator, bit for bit. The files are written by tests/_voc_file.py from the oracle's synthetic vocoder, so every comparison has an engine
or the CPU oracle on the other side. The vocoder is driven through q3tts_k_vocoder on given codes: 9 frames in chunks of 4, so that the
convolution histories and the attention ring carry across calls. Two tiny shapes (tests/_voc_file.py).
"""
import ctypes as C
import os

import numpy as np
import pytest

import _voc_file as VF

pytestmark = pytest.mark.gpu

S, S2 = 5, 6
PCM_RMS_TOL = 2e-3   # the suite's small-shape PCM bound (tests/test_parity_gpu.py)
SHAPES = {"tiny": VF.shape_tiny, "b": VF.shape_b}
MODEL_FILES = ("qwen3_tts_talker.gguf", "qwen3_tts_predictor.gguf", "qwen3_assets.gguf")


@pytest.fixture(scope="module")
def model_files(tmp_path_factory):
    """One quant directory with the synthetic Talker / Predictor / assets (seed 0, tiny shape, a small text table): the model directories
    below link to its files."""
    import _model_dir as MD
    d = tmp_path_factory.mktemp("voc_file_models")
    MD.write_dir(str(d / "gguf"), MD.shape_tiny(text_vocab=1024), seed=0)
    return d / "gguf"


def _model_dir(tmp_path, model_files, name):
    d = tmp_path / name
    os.makedirs(d / "gguf")
    for f in MODEL_FILES:
        os.symlink(model_files / f, d / "gguf" / f)
    return d


def _config(model_dir, vc, seed, max_batch=1):
    """The tiny engine configuration opened on model_dir (q3tts_config_from_model_dir: the vocoder block comes from the file if there is one)."""
    from q3tts import _abi, native
    base = _abi.tiny_config(max_batch=max_batch, n_ctx=256, with_vocoder=1)
    base.vocoder = vc
    base.synth_seed = seed
    return native.config_from_model_dir(str(model_dir), None, base=base)


def _synthetic_engine(vc, seed):
    from q3tts import _abi, native
    cfg = _abi.tiny_config(max_batch=1, n_ctx=256, with_vocoder=1)
    cfg.vocoder = vc
    cfg.synth_seed = seed
    return native.NativeEngine(cfg)


def _codes(vc):
    return np.random.default_rng(9).integers(0, vc.codebook_size, size=(9, 16)).astype(np.int32)


@pytest.fixture(scope="module")
def synthetic_pcm():
    """{(shape, seed): PCM of the synthetic engine on _codes, 9 frames in chunks of 4} — computed once per (shape, seed)."""
    memo = {}

    def get(shape, seed):
        if (shape, seed) not in memo:
            vc = SHAPES[shape]()
            eng = _synthetic_engine(vc, seed)
            try:
                assert eng.vocoder_source == 1
                pcm = eng.vocoder(_codes(vc), chunk_frames=4)
            finally:
                eng.close()
            assert pcm.shape == (9 * VF.samples_per_frame(vc),)
            pcm.setflags(write=False)
            memo[(shape, seed)] = pcm
        return memo[(shape, seed)]
    return get


@pytest.mark.parametrize("container,where", [("bf16", "parent"), ("f32_perturbed", "quant")])
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_same_seed_file_gives_the_synthetic_engines_bits(oracle, tmp_path, model_files, synthetic_pcm, shape, container, where):
    """synth_seed = S and a file written from seed S: PCM == the synthetic engine's, bit for bit. BF16 container in the model directory;
    F32 container off the bf16 values (only nearest-even rounding brings them back) in the quant directory. Every SnakeBeta pair on the
    device is the generator's, or the PCM would differ."""
    from q3tts import native
    vc = SHAPES[shape]()
    d = _model_dir(tmp_path, model_files, "m")
    VF.write((d if where == "parent" else d / "gguf") / VF.FILE, oracle, vc, S, container)
    other = VF.shape_b() if shape == "tiny" else VF.shape_tiny()   # the base's block is another shape: the file's must replace it
    cfg = _config(d, other, S)
    assert bytes(cfg.vocoder) == bytes(vc)
    eng = native.NativeEngine(cfg)
    try:
        assert eng.vocoder_source == 2
        pcm = eng.vocoder(_codes(vc), chunk_frames=4)
        assert np.array_equal(pcm.view(np.uint32), synthetic_pcm(shape, S).view(np.uint32))
        assert np.array_equal(eng.vocoder(_codes(vc)).view(np.uint32), pcm.view(np.uint32))   # one call == chunks of 4
    finally:
        eng.close()


@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_other_weights_are_the_files_not_the_seeds(oracle, tmp_path, model_files, synthetic_pcm, shape):
    """A file written from seed S2 in an engine with synth_seed = S: the PCM is the seed-S2 synthetic engine's bit for bit, differs from
    the seed-S engine's, and is within the small-shape bound of the CPU oracle at seed S2. (Without the loader the engine computes the
    seed-S PCM: this is the test that fails.)"""
    from q3tts import native
    vc = SHAPES[shape]()
    d = _model_dir(tmp_path, model_files, "m")
    VF.write(d / VF.FILE, oracle, vc, S2)
    eng = native.NativeEngine(_config(d, vc, S))
    try:
        assert eng.vocoder_source == 2
        pcm = eng.vocoder(_codes(vc), chunk_frames=4)
    finally:
        eng.close()
    assert np.array_equal(pcm.view(np.uint32), synthetic_pcm(shape, S2).view(np.uint32))
    assert not np.array_equal(pcm, synthetic_pcm(shape, S))
    L = oracle.lib()
    v = L.q3o_vocoder_create(C.byref(vc), S2, 4)
    try:
        codes = _codes(vc)
        ref = np.zeros(pcm.size + 64, dtype=np.float32)
        n = L.q3o_vocoder_decode(v, oracle.ptr(codes, oracle.i32p), codes.shape[0], 1, oracle.ptr(ref, oracle.f32p), ref.size)
    finally:
        L.q3o_vocoder_destroy(v)
    assert n == pcm.size
    rms = float(np.sqrt(np.mean((pcm - ref[:n]) ** 2)))
    print(f"file weights (seed {S2}) vs the oracle, shape {shape}: PCM RMS error {rms:.2e} (signal RMS {float(np.sqrt(np.mean(ref[:n] ** 2))):.2f})")
    assert rms <= PCM_RMS_TOL, rms


def test_whole_request_with_a_vocoder_file(oracle, tmp_path, model_files, monkeypatch):
    """TtsEngine.new on a model directory with a vocoder file (shape b, seed 0 = the default synth_seed): one generate_batch request gives
    codes == and PCM == an engine on the same model files without the vocoder file whose synth_seed and vocoder block match."""
    from q3tts import _abi, api, native
    monkeypatch.chdir(tmp_path)
    vc = VF.shape_b()
    d = _model_dir(tmp_path, model_files, "with_file")
    VF.write(d / "gguf" / VF.FILE, oracle, vc, 0)
    base = _abi.tiny_config(max_batch=2, n_ctx=256, with_vocoder=1)   # (another vocoder block than the file's)
    cfg = native.config_from_model_dir(str(d), None, base=base)
    eng = api.TtsEngine.new(str(d), "none", config=cfg)
    spk = ((np.arange(cfg.model.d_embed) % 13 - 6) * 0.03125).astype(np.float32)
    desc, keep = oracle.make_prompt_desc(np.arange(300, 317), spk_emb=spk)
    req = dict(desc=desc, temperature=0.7, top_k=40, top_p=0.9, seed=12, max_steps=9, min_frames=9, want_pcm=1)
    try:
        assert eng.vocoder_is_synthetic is False and eng._native.vocoder_source == 2 and bytes(eng.cfg.vocoder) == bytes(vc)
        got = eng._native.generate_batch([req])[0]
    finally:
        eng.close()
    plain = _model_dir(tmp_path, model_files, "without_file")
    cfg2 = _config(plain, vc, 0, max_batch=2)
    assert bytes(cfg2.vocoder) == bytes(vc)
    eng2 = api.TtsEngine.new(str(plain), "none", config=cfg2)
    try:
        assert eng2.vocoder_is_synthetic is True
        want = eng2._native.generate_batch([req])[0]
    finally:
        eng2.close()
    assert got.status == 0 and want.status == 0 and got.codes.shape[0] == 9
    assert np.array_equal(got.codes, want.codes)
    assert got.pcm is not None and got.pcm.shape == (9 * VF.samples_per_frame(vc),)
    assert np.array_equal(got.pcm.view(np.uint32), want.pcm.view(np.uint32))


def test_a_wrong_shape_is_refused_on_the_host_and_the_next_create_succeeds(oracle, tmp_path, model_files):
    """q3tts_engine_create with a file whose pwconv2 has the wrong shape: the error names the tensor and both shapes, no engine exists,
    and a valid create right after it works. The refusal is the host check's (it comes
    before the first device allocation), not a fault."""
    from q3tts import _abi, native
    vc = VF.shape_tiny()
    d = _model_dir(tmp_path, model_files, "bad")
    VF.write(d / VF.FILE, oracle, vc, S, edit_tensors=lambda t: t.__setitem__("upsample.1.1.pwconv2.weight", np.zeros((64, 192), dtype=np.float32)))
    base = _abi.tiny_config(max_batch=1, n_ctx=256, with_vocoder=1)
    base.synth_seed = S
    cfg = _abi.copy_config(base)
    cfg.weights_path = os.fsencode(str(d / "gguf"))   # (config_from_model_dir would refuse the file already: go straight to the engine)
    lib = _abi.load_library()
    h = C.c_void_p()
    rc = lib.q3tts_engine_create(C.byref(cfg), C.byref(h))
    msg = lib.q3tts_last_error(None).decode()
    assert rc == -1 and not h.value
    assert VF.FILE in msg and "'upsample.1.1.pwconv2.weight'" in msg and "[64][192]" in msg and "[64][256]" in msg
    with pytest.raises(_abi.Q3Error, match="pwconv2"):
        native.NativeEngine(cfg)
    VF.write(d / VF.FILE, oracle, vc, S)
    eng = native.NativeEngine(cfg)
    try:
        assert eng.vocoder_source == 2
        assert eng.vocoder(_codes(vc), chunk_frames=4).shape == (9 * VF.samples_per_frame(vc),)
    finally:
        eng.close()

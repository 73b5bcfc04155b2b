"""The clone encoders' weights files on the host: every relayout and rounding of the loader against the oracle's arrays, the
shape read back from the pair, where the two files are found, every refusal and cross-check, and the converter. CPU only:
q3tts_k_clone_file_tensor returns what q3tts_clone_load would upload, and q3tts_k_clone_load_check is the host half of q3tts_clone_load (its
refusals come before the device is touched). The pairs are written by tests/_clone_file.py from the oracle's synthetic encoders, at the GPU
parity tests' tiny shape and a second one put together from tests/_clone_shapes.py.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import _clone_file as CF
import _gguf as G

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = {"tiny": CF.shape_tiny, "b": CF.shape_b}
SEED = 5
SP, CP = CF.SPK_ARCH + ".", CF.CODEC_ARCH + "."
ERR_INVALID, ERR_IO = -1, -4
ARRAY_FIELDS = ("se_channels", "se_kernels", "se_dilations", "ae_ratios")


def _fields(c):
    from q3tts import _abi
    return {n: (list(getattr(c, n)) if n in ARRAY_FIELDS else getattr(c, n)) for n, _ in _abi.CloneConfig._fields_}


def _base():
    """a complete config none of whose file-stated fields is a test shape's, with a layer scale of its own"""
    from q3tts import _abi
    b = _abi.full_clone_config_py()
    b.ae_layer_scale = 0.125
    return b


def _want(c, base):
    w = _fields(c)
    w["ae_layer_scale"] = base.ae_layer_scale   # a generator parameter: no file states it
    return w


def _config_call(wdir, base):
    """q3tts_clone_config_from_dir -> (status, message, config)"""
    import ctypes as C
    from q3tts import _abi
    lib = _abi.load_library()
    cc = _abi.CloneConfig.from_buffer_copy(base)
    err = C.create_string_buffer(2048)
    rc = lib.q3tts_clone_config_from_dir(os.fsencode(str(wdir)), C.byref(cc), err, len(err))
    return rc, err.value.decode("utf-8", "replace"), cc


# ---- 1. the arrays ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("container", ["bf16", "f32_perturbed"])
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_every_file_array_equals_the_oracles(oracle, tmp_path, shape, container):
    """For every generator id (comp, which): the array the loader would upload == the oracle's array, bit for bit (device layout: rows
    W[n][tap * cin + ci] with zeros up to round512(k * cin), q / k / v fused in that order; after rounding). The F32 container holds the
    matrices' values moved by (1 -/+ 2^-12): only round-to-nearest-even brings every one of them back (truncation lands one bf16 step low
    wherever the factor is below 1). The speaker file lies in the model directory, the codec file in the quant directory."""
    from q3tts import native
    c = SHAPES[shape]()
    wdir = tmp_path / "gguf"
    spk_path, codec_path = CF.write(tmp_path, wdir, c, SEED, container)
    ents = CF.entries(c)
    names = [n for e in ents for n in e.names]
    assert len({(e.comp, e.which) for e in ents}) == len(ents) and len(set(names)) == len(names)
    assert max(len(n.encode()) for n in names) <= 63   # GGUF's usable tensor-name length
    if container == "f32_perturbed":   # the container really holds other values than the bf16 ones, in F32
        rd = G.read(spk_path)
        e = next(e for e in ents if e.names == ["mfa.conv.weight"])
        ref = CF.tensors(c, SEED)[CF.SPK]["mfa.conv.weight"]
        assert rd["mfa.conv.weight"][1] == G.F32 and not np.array_equal(rd["mfa.conv.weight"][0], ref)
        assert np.array_equal(G.bf16_bits_to_f32(G.f32_to_bf16_bits(rd["mfa.conv.weight"][0])), ref)
        trunc = (rd["mfa.conv.weight"][0].view(np.uint32) & np.uint32(0xFFFF0000)).view(np.float32)
        assert not np.array_equal(trunc, ref)
        assert e.is_matrix
    n_mat = 0
    for e in ents:
        got = native.k_clone_file_tensor(wdir, c, e.comp, e.which)
        ref = CF.device_array(c, SEED, e).reshape(-1)
        assert got.shape == ref.shape and np.array_equal(got.view(np.uint32), ref.view(np.uint32)), e.names
        if e.is_matrix:
            n_mat += 1
            kc = (e.k or 1) * e.cin
            assert got.size == e.n * CF.round512(kc) and not got.reshape(e.n, -1)[:, kc:].any()
            assert np.array_equal(G.bf16_bits_to_f32(G.f32_to_bf16_bits(got)), got)   # bf16-representable
    assert n_mat == 1 + 3 * (3 + c.se_res2net_scale) + 4 + 1 + 3 * c.ae_n_ratios + 1 + 4 * c.ae_n_layer + 3
    with pytest.raises(Exception, match=r"no tensor of id \(61, 0\)"):
        native.k_clone_file_tensor(wdir, c, 61, 0)
    with pytest.raises(Exception, match=r"no tensor of id \(%d, 0\)" % (64 + c.ae_n_layer)):
        native.k_clone_file_tensor(wdir, c, 64 + c.ae_n_layer, 0)


# ---- 2. the shape from the pair, and where the pair is found ---------------------------------------------------------------------------
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_config_from_dir_reproduces_the_shape_wherever_the_files_lie(oracle, tmp_path, shape):
    from q3tts import native
    c, base = SHAPES[shape](), _base()
    wdir = tmp_path / "m" / "gguf"
    os.makedirs(wdir)
    # none: Q3TTS_ERR_IO, both named, the caller's config untouched
    snap = bytes(base)
    rc, msg, cc = _config_call(wdir, base)
    assert rc == ERR_IO and CF.SPK_FILE in msg and CF.CODEC_FILE in msg and bytes(cc) == snap
    # both in the quant directory
    CF.write(wdir, wdir, c, SEED)
    assert _fields(native.clone_config_from_dir(wdir, base)) == _want(c, base)
    assert bytes(base) == snap                                  # the caller's block is not written
    assert _fields(native.clone_config_from_dir(str(wdir) + "/", base)) == _want(c, base)   # a trailing slash names the same directory
    # both in the parent (the model directory): one unquantised pair serves every quant directory
    for f in (CF.SPK_FILE, CF.CODEC_FILE):
        os.rename(wdir / f, tmp_path / "m" / f)
    assert _fields(native.clone_config_from_dir(wdir, base)) == _want(c, base)
    os.makedirs(tmp_path / "m" / "gguf_q8_0")
    assert _fields(native.clone_config_from_dir(tmp_path / "m" / "gguf_q8_0", base)) == _want(c, base)
    # a file in the quant directory wins over the parent's: the other shape's codec file there disagrees with nothing in the speaker file
    other = SHAPES["b" if shape == "tiny" else "tiny"]()
    CF.write(None, wdir, other, SEED)
    got = _fields(native.clone_config_from_dir(wdir, base))
    assert got["ae_hidden"] == other.ae_hidden and got["ae_n_codebooks"] == other.ae_n_codebooks and got["se_dim"] == c.se_dim
    os.remove(wdir / CF.CODEC_FILE)
    # exactly one absent: Q3TTS_ERR_IO, the message names the missing one (first) and says the other was there
    os.remove(tmp_path / "m" / CF.CODEC_FILE)
    rc, msg, cc = _config_call(wdir, base)
    assert rc == ERR_IO and msg.startswith(CF.CODEC_FILE + " not found") and bytes(cc) == snap
    CF.write(None, wdir, c, SEED)
    os.remove(tmp_path / "m" / CF.SPK_FILE)
    rc, msg, cc = _config_call(wdir, base)
    assert rc == ERR_IO and msg.startswith(CF.SPK_FILE + " not found") and bytes(cc) == snap
    assert native.clone_files_found(wdir) == (None, str(wdir / CF.CODEC_FILE))
    assert native.k_clone_load_check(wdir)[0] == ERR_IO


# ---- 3. the refusals of q3tts_clone_load's host half, and the cross-checks of q3tts_clone_config_from_dir ------------------------------
def _poke(name, idx, value=np.nan):
    def edit(t):
        a = t[name].copy(); a.reshape(-1)[idx] = value; t[name] = a
    return edit


def _reshaped(name, shape):
    return lambda t: t.__setitem__(name, np.zeros(shape, dtype=np.float32))


def _more_layers(t):   # one more layer than the metadata counts
    for k in [k for k in t if k.startswith("encoder_transformer.layers.0.")]:
        t[k.replace("layers.0.", "layers.7.")] = t[k]


# case -> (shape, write kwargs, file named in the message, needles, refused by q3tts_clone_config_from_dir too)
REFUSALS = {
    "missing tensor, speaker": ("tiny", dict(edit_spk={"blocks.2.se_block.conv2.bias": CF.DROP}), CF.SPK_FILE, ["tensor 'blocks.2.se_block.conv2.bias' is missing"], True),
    "missing tensor, codec": ("b", dict(edit_codec={"encoder_transformer.layers.1.mlp.fc2.weight": CF.DROP}), CF.CODEC_FILE,
                              ["tensor 'encoder_transformer.layers.1.mlp.fc2.weight' is missing"], True),
    "missing last convolution": ("b", dict(edit_codec={"encoder.layers.8.conv.bias": CF.DROP}), CF.CODEC_FILE, ["tensor 'encoder.layers.8.conv.bias' is missing"], True),
    "conv shape": ("tiny", dict(edit_spk=_reshaped("mfa.conv.weight", (192, 192, 3))), CF.SPK_FILE, ["tensor 'mfa.conv.weight'", "[192][192][3]", "[192][192][1]"], True),
    "conv as a matrix": ("tiny", dict(edit_spk=_reshaped("fc.weight", (512, 384))), CF.SPK_FILE, ["tensor 'fc.weight'", "[512][384]", "[512][384][1]"], True),
    "bias shape": ("b", dict(edit_codec=_reshaped("encoder.layers.3.conv.bias", (65,))), CF.CODEC_FILE, ["'encoder.layers.3.conv.bias'", "[65]", "[64]"], True),
    "k_proj shape": ("b", dict(edit_codec=_reshaped("encoder_transformer.layers.2.self_attn.k_proj.weight", (128, 128))), CF.CODEC_FILE,
                     ["'encoder_transformer.layers.2.self_attn.k_proj.weight'", "[128][128]", "[96][128]"], True),
    "o_proj shape": ("b", dict(edit_codec=_reshaped("encoder_transformer.layers.0.self_attn.o_proj.weight", (96, 128))), CF.CODEC_FILE,
                     ["'encoder_transformer.layers.0.self_attn.o_proj.weight'", "[96][128]", "[128][96]"], True),
    "fc1 shape": ("tiny", dict(edit_codec=_reshaped("encoder_transformer.layers.1.mlp.fc1.weight", (128, 256))), CF.CODEC_FILE,
                  ["'encoder_transformer.layers.1.mlp.fc1.weight'", "[128][256]", "[256][128]"], True),
    "stride conv kernel is 2 x ratio": ("tiny", dict(edit_codec_meta={CP + "ratios": [4, 5, 6, 7]}), CF.CODEC_FILE,
                                        ["'encoder.layers.12.conv.weight'", "[512][256][16]", "[512][256][14]"], True),
    "frame-rate conv kernel is 2 x stride": ("tiny", dict(edit_codec_meta={CP + "down_stride": 3}), CF.CODEC_FILE,
                                             ["'downsample.conv.weight'", "[128][128][4]", "[128][128][6]"], True),
    "codebook shape": ("b", dict(edit_codec_meta={CP + "codebook_size": 1024}), CF.CODEC_FILE, ["'quantizer.codebook.0.weight'", "[1000][48]", "[1024][48]"], True),
    "layer count": ("tiny", dict(edit_codec_meta={CP + "block_count": 3}), CF.CODEC_FILE, ["'q3tts-codec-encoder.block_count' implies 3", "has 2"], True),
    "layer count, more in the file": ("tiny", dict(edit_codec=_more_layers), CF.CODEC_FILE, ["'q3tts-codec-encoder.block_count' implies 2", "has 3"], True),
    "stage count": ("tiny", dict(edit_codec_meta={CP + "ratios": [4, 5, 6]}), CF.CODEC_FILE, ["'q3tts-codec-encoder.ratios' implies 3", "has 4"], True),
    "codebook count": ("tiny", dict(edit_codec={"quantizer.codebook.15.weight": CF.DROP}), CF.CODEC_FILE,
                       ["'q3tts-codec-encoder.n_codebooks' implies 16", "'quantizer.codebook.N.weight...'", "has 15"], True),
    "Res2Net branch count": ("tiny", dict(edit_spk_meta={SP + "res2net_scale": 2}), CF.SPK_FILE,
                             ["'q3tts-speaker-encoder.res2net_scale' implies 1", "'blocks.1.res2net_block.blocks.N.conv.weight...'", "has 3"], True),
    "key missing, speaker": ("tiny", dict(edit_spk_meta={SP + "embedding_length": CF.DROP}), CF.SPK_FILE, ["'q3tts-speaker-encoder.embedding_length' is missing"], True),
    "key missing, codec": ("tiny", dict(edit_codec_meta={CP + "vq_dim": CF.DROP}), CF.CODEC_FILE, ["'q3tts-codec-encoder.vq_dim' is missing"], True),
    "integer key holds a float": ("tiny", dict(edit_spk_meta={SP + "res2net_scale": 4.0}), CF.SPK_FILE, ["'q3tts-speaker-encoder.res2net_scale' is not an integer"], True),
    "float key holds an integer": ("tiny", dict(edit_codec_meta={CP + "rope.freq_base": 10000}), CF.CODEC_FILE, ["'q3tts-codec-encoder.rope.freq_base' is not a float"], True),
    "array key holds a scalar": ("tiny", dict(edit_spk_meta={SP + "channels": 64}), CF.SPK_FILE, ["'q3tts-speaker-encoder.channels' is not an integer array"], True),
    "array of 4": ("tiny", dict(edit_spk_meta={SP + "dilations": [1, 2, 3, 4]}), CF.SPK_FILE, ["'q3tts-speaker-encoder.dilations' has 4 entries"], True),
    "architecture": ("tiny", dict(edit_codec_meta={"general.architecture": CF.SPK_ARCH}), CF.CODEC_FILE, ["'general.architecture' = 'q3tts-speaker-encoder'"], True),
    "tensor type": ("tiny", dict(raw_types={"asp.tdnn.conv.weight": 2}), CF.SPK_FILE, ["'asp.tdnn.conv.weight'", "unsupported ggml type 2"], True),
    "NaN in a bias": ("tiny", dict(edit_spk=_poke("asp.conv.bias", 7)), CF.SPK_FILE, ["'asp.conv.bias'", "not finite", "element 7"], False),
    "infinity in a matrix": ("b", dict(container="f32", edit_codec=_poke("encoder_transformer.layers.1.self_attn.v_proj.weight", 1234, np.inf)), CF.CODEC_FILE,
                             ["'encoder_transformer.layers.1.self_attn.v_proj.weight'", "not finite", "1234"], False),
    "infinity in a codebook": ("b", dict(edit_codec=_poke("quantizer.codebook.2.weight", 5, -np.inf)), CF.CODEC_FILE, ["'quantizer.codebook.2.weight'", "not finite"], False),
    "NaN in a LayerScale": ("tiny", dict(edit_codec=_poke("encoder_transformer.layers.0.mlp_layer_scale.scale", 0)), CF.CODEC_FILE,
                            ["'encoder_transformer.layers.0.mlp_layer_scale.scale'", "not finite"], False),
    # consistent files whose shape the encoders' own config rules refuse: the message is validate()'s
    "config refused: window": ("tiny", dict(edit_codec_meta={CP + "attention.sliding_window": 9000}), None, ["clone config:", "ae_window must be 1..8192"], False),
}


@pytest.mark.parametrize("case", sorted(REFUSALS))
def test_a_wrong_pair_is_refused_on_the_host(oracle, tmp_path, case):
    """Each refusal is Q3TTS_ERR_INVALID and names the file and the tensor or key (a shape: both shapes). What the metadata or the tensor
    list gets wrong is refused by q3tts_clone_config_from_dir as well, with the same words, and leaves the caller's config untouched."""
    from q3tts import native
    shape, kw, fname, needles, by_config = REFUSALS[case]
    c = SHAPES[shape]()
    CF.write(tmp_path / "gguf", tmp_path, c, SEED, **kw)
    rc, msg = native.k_clone_load_check(tmp_path / "gguf")
    assert rc == ERR_INVALID, (rc, msg)
    for n in needles + ([fname] if fname else []):
        assert n in msg, (n, msg)
    base = _base()
    snap = bytes(base)
    rc2, msg2, cc = _config_call(tmp_path / "gguf", base)
    if by_config:
        assert rc2 == ERR_INVALID and msg2 == msg and bytes(cc) == snap
    else:
        assert rc2 == 0 and bytes(cc) != snap


def test_a_good_pair_passes_the_host_check(oracle, tmp_path):
    from q3tts import native
    for shape in sorted(SHAPES):
        CF.write(tmp_path / shape, tmp_path / shape, SHAPES[shape](), SEED)
        assert native.k_clone_load_check(tmp_path / shape) == (0, "")


def test_a_file_that_ends_early_is_refused(oracle, tmp_path):
    """q3tts_clone_load's host half: Q3TTS_ERR_INVALID; q3tts_clone_config_from_dir: Q3TTS_ERR_IO (an unreadable file), like the vocoder's."""
    from q3tts import native
    c = CF.shape_b()
    spk_path, codec_path = CF.write(tmp_path, tmp_path, c, SEED)
    for path in (codec_path, spk_path):
        raw = open(path, "rb").read()
        for cut in (len(raw) - 64, len(raw) // 2, 200, 10):   # inside the last tensor, inside the data, inside the metadata, inside the header
            with open(path, "wb") as f:
                f.write(raw[:cut])
            rc, msg = native.k_clone_load_check(tmp_path)
            assert rc == ERR_INVALID and os.path.basename(path) in msg, (cut, msg)
            rc2, msg2, _ = _config_call(tmp_path, _base())
            assert rc2 == ERR_IO and msg2 == msg
        with open(path, "wb") as f:
            f.write(raw[:len(raw) - 64])
        assert "lies outside the file" in native.k_clone_load_check(tmp_path)[1]
        with open(path, "wb") as f:
            f.write(raw)
    assert native.k_clone_load_check(tmp_path) == (0, "")


def test_unknown_tensors_are_ignored(oracle, tmp_path):
    from q3tts import native
    c = CF.shape_tiny()
    extra = lambda t: t.update({"quantizer.semantic_residual_vector_quantizer.output_proj.weight": np.ones((128, 32, 1), dtype=np.float32),
                                "decoder.layers.0.conv.weight": np.full((4, 4, 3), np.nan, dtype=np.float32),
                                "quantizer.acoustic_residual_vector_quantizer.layers.20.codebook.embed_sum": np.ones((64, 32), dtype=np.float32)})
    CF.write(tmp_path, tmp_path, c, SEED, edit_codec=extra, edit_spk=lambda t: t.update({"blocks.0.norm.weight": np.ones(64, dtype=np.float32)}))
    assert native.k_clone_load_check(tmp_path) == (0, "")
    assert _fields(native.clone_config_from_dir(tmp_path, _base())) == _want(c, _base())


# ---- 4. the converter ------------------------------------------------------------------------------------------------------------------------
def _family_config(c):
    """CONFIG.json in the family configs' keys, for the modules tests/_clone_family.py builds"""
    import _clone_family as FAM
    m = FAM.mimi(c)
    cfg = {k: v for k, v in m.config.to_dict().items() if isinstance(v, (int, float, str, bool, list)) or v is None}
    cfg.update(mel_dim=128, enc_channels=list(c.se_channels), enc_kernel_sizes=list(c.se_kernels), enc_dilations=list(c.se_dilations),
               enc_attention_channels=c.se_attn_channels, enc_res2net_scale=c.se_res2net_scale, enc_se_channels=c.se_se_channels, enc_dim=c.se_dim)
    return cfg, m


@pytest.fixture(scope="module")
def family_checkpoints(tmp_path_factory):
    """The family's own modules with the oracle's seed-0 weights, torch.save'd: their state_dict keys are what the converter copies by name."""
    torch = pytest.importorskip("torch")
    pytest.importorskip("transformers")
    import _clone_family as FAM
    c = CF.shape_tiny()
    d = tmp_path_factory.mktemp("clone_ckpt")
    cfg, mimi = _family_config(c)
    torch.save({"spk." + k: v for k, v in FAM.ecapa(c).state_dict().items()}, d / "speaker.pt")   # under a prefix, as inside a larger model
    torch.save(mimi.state_dict(), d / "codec.pt")
    with open(d / "config.json", "w") as f:
        json.dump(cfg, f)
    return c, d, cfg


def _tool():
    sys.path.insert(0, os.path.join(REPO, "tools"))
    try:
        import clone_to_gguf
    finally:
        sys.path.pop(0)
    return clone_to_gguf


def test_converter_copies_the_familys_keys_and_the_loader_gives_the_oracles_arrays(oracle, family_checkpoints, tmp_path):
    """tools/clone_to_gguf.py on the state dicts of transformers' ECAPA_TimeDelayNet and MimiModel (this pins the key names against the
    installed package): every device array == the oracle's, the metadata reads back as the config, both dtypes."""
    from q3tts import native
    c, d, _ = family_checkpoints
    for dtype in ("f32", "bf16"):
        out = tmp_path / dtype
        r = subprocess.run([sys.executable, os.path.join(REPO, "tools", "clone_to_gguf.py"), str(d / "speaker.pt"), str(d / "codec.pt"), str(out),
                            "--config", str(d / "config.json"), "--dtype", dtype, "--speaker-prefix", "spk."], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        assert CF.SPK_FILE in r.stdout and CF.CODEC_FILE in r.stdout
        assert _fields(native.clone_config_from_dir(out, _base())) == _want(c, _base())
        assert native.k_clone_load_check(out) == (0, "")
        for e in CF.entries(c):
            got = native.k_clone_file_tensor(out, c, e.comp, e.which)
            ref = CF.device_array(c, 0, e).reshape(-1)
            assert np.array_equal(got.view(np.uint32), ref.view(np.uint32)), e.names
        rd = G.read(str(out / CF.CODEC_FILE))
        want_ty = G.BF16 if dtype == "bf16" else G.F32
        assert rd["downsample.conv.weight"][1] == want_ty and rd["encoder_transformer.layers.0.mlp.fc1.weight"][1] == want_ty
        assert rd["quantizer.codebook.3.weight"][1] == G.F32 and rd["encoder.layers.0.conv.bias"][1] == G.F32
        assert not any(k.startswith("decoder") or "output_proj" in k or "embed_sum" in k for k in rd)
        assert set(rd) == {n for e in CF.entries(c) if e.file == CF.CODEC for n in e.names}


def test_converter_keeps_the_first_n_codebooks(oracle, family_checkpoints, tmp_path):
    from q3tts import native
    c, d, _ = family_checkpoints
    _tool().convert(str(d / "speaker.pt"), str(d / "codec.pt"), str(tmp_path), str(d / "config.json"), speaker_prefix="spk.", n_codebooks=5)
    got = native.clone_config_from_dir(tmp_path, _base())
    assert got.ae_n_codebooks == 5
    for q in (0, 4):   # the semantic quantiser first, then the acoustic ones in order
        e = next(e for e in CF.entries(c) if e.comp == 110 + q)
        assert np.array_equal(native.k_clone_file_tensor(tmp_path, got, 110 + q, 0), CF.device_array(c, 0, e).reshape(-1))


def test_converter_lists_every_missing_key_and_every_inexpressible_value(oracle, family_checkpoints, tmp_path):
    torch = pytest.importorskip("torch")
    c, d, cfg = family_checkpoints
    tool = _tool()
    gone_spk = ["spk.blocks.2.res2net_block.blocks.1.conv.bias", "spk.fc.weight"]
    gone_codec = ["encoder.layers.14.conv.weight", "encoder_transformer.layers.1.self_attn_layer_scale.scale", "downsample.conv.weight",
                  "quantizer.acoustic_residual_vector_quantizer.layers.3.codebook.cluster_usage", "quantizer.semantic_residual_vector_quantizer.layers.0.codebook.embed_sum"]
    sd = torch.load(d / "speaker.pt", weights_only=True)
    torch.save({k: v for k, v in sd.items() if k not in gone_spk}, tmp_path / "speaker.pt")
    sd = torch.load(d / "codec.pt", weights_only=True)
    torch.save({k: v for k, v in sd.items() if k not in gone_codec}, tmp_path / "codec.pt")
    bad = dict(cfg, num_residual_layers=2, use_conv_shortcut=True, use_causal_conv=False, num_semantic_quantizers=2, num_key_value_heads=2, hidden_act="gelu")
    with open(tmp_path / "config.json", "w") as f:
        json.dump(bad, f)
    with pytest.raises(SystemExit) as ei:
        tool.convert(str(tmp_path / "speaker.pt"), str(tmp_path / "codec.pt"), str(tmp_path / "out"), str(tmp_path / "config.json"), speaker_prefix="spk.")
    msg = str(ei.value)
    for k in [k[len("spk."):] for k in gone_spk] + gone_codec:
        assert k in msg, (k, msg)
    assert "lack 7 required key(s)" in msg
    for k in ("num_residual_layers", "use_conv_shortcut", "use_causal_conv", "num_semantic_quantizers", "num_key_value_heads", "hidden_act"):
        assert f"config: {k} = " in msg, (k, msg)
    assert not os.path.exists(tmp_path / "out" / CF.SPK_FILE) and not os.path.exists(tmp_path / "out" / CF.CODEC_FILE)


def test_converter_builds_the_codebooks_as_the_float64_quotient(oracle, family_checkpoints, tmp_path):
    """cluster_usage that is not all ones (some entries below the class's eps, so the clamp acts): table = embed_sum / clamp(cluster_usage,
    eps)[:, None] evaluated in float64 and rounded once to f32 — not the f32 quotient wherever the two differ."""
    torch = pytest.importorskip("torch")
    from q3tts import native
    c, d, _ = family_checkpoints
    tool = _tool()
    eps = tool.mimi_eps()
    from transformers.models.mimi.modeling_mimi import MimiEuclideanCodebook
    import inspect
    assert eps == inspect.signature(MimiEuclideanCodebook.__init__).parameters["epsilon"].default
    sd = torch.load(d / "codec.pt", weights_only=True)
    rng = np.random.default_rng(2)
    usage = {}
    for q in range(c.ae_n_codebooks):
        key = ("quantizer.semantic_residual_vector_quantizer.layers.0." if q == 0 else f"quantizer.acoustic_residual_vector_quantizer.layers.{q - 1}.") + "codebook.cluster_usage"
        u = rng.uniform(0.3, 7.0, size=c.ae_codebook_size).astype(np.float32)
        u[::9] = np.float32(eps) / 4
        usage[q] = u
        sd[key] = torch.from_numpy(u.copy())
    torch.save(sd, tmp_path / "codec.pt")
    tool.convert(str(d / "speaker.pt"), str(tmp_path / "codec.pt"), str(tmp_path), str(d / "config.json"), speaker_prefix="spk.")
    differs = 0
    for q in range(c.ae_n_codebooks):
        e = next(e for e in CF.entries(c) if e.comp == 110 + q)
        es = CF.device_array(c, 0, e)
        want = (es.astype(np.float64) / np.maximum(usage[q].astype(np.float64), eps)[:, None]).astype(np.float32)
        got = native.k_clone_file_tensor(tmp_path, c, 110 + q, 0).reshape(want.shape)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), q
        differs += int((want != es / np.maximum(usage[q], np.float32(eps))[:, None]).sum())
    assert differs > 0


def test_converter_says_plainly_that_a_safetensors_file_needs_the_package(family_checkpoints, tmp_path, monkeypatch):
    c, d, _ = family_checkpoints
    monkeypatch.setitem(sys.modules, "safetensors.torch", None)   # importing it now raises ImportError
    monkeypatch.setitem(sys.modules, "safetensors", None)
    with pytest.raises(SystemExit, match=r"speaker\.safetensors: reading a \.safetensors file needs the safetensors package"):
        _tool().convert(str(tmp_path / "speaker.safetensors"), str(d / "codec.pt"), str(tmp_path / "out"), str(d / "config.json"))


# ---- 5. the lookup rule's one home -----------------------------------------------------------------------------------------------------------
def test_clone_files_find_returns_what_the_loader_would_open(oracle, tmp_path):
    """q3tts_clone_files_find: the count and the two paths (quant directory first, then its parent, each file on its own; "" when absent), a
    trailing slash, and a buffer that is too small refused with the size needed."""
    import ctypes as C
    from q3tts import _abi, native
    lib = _abi.load_library()
    wdir = tmp_path / "m" / "gguf"
    os.makedirs(wdir)

    def find(d, cap=4096):
        a, b = C.create_string_buffer(cap), C.create_string_buffer(cap)
        return lib.q3tts_clone_files_find(os.fsencode(str(d)), a, b, cap), os.fsdecode(a.value), os.fsdecode(b.value)

    assert find(wdir) == (0, "", "") and native.clone_files_found(wdir) == (None, None)
    c = CF.shape_tiny()
    CF.write(tmp_path / "m", wdir, c, SEED)
    want = (2, str(tmp_path / "m" / CF.SPK_FILE), str(wdir / CF.CODEC_FILE))
    assert find(wdir) == want and find(str(wdir) + "/") == want
    assert native.clone_files_found(wdir) == want[1:]
    CF.write(wdir, None, c, SEED)   # the quant directory's own speaker file wins over the parent's
    assert find(wdir) == (2, str(wdir / CF.SPK_FILE), str(wdir / CF.CODEC_FILE))
    os.remove(wdir / CF.CODEC_FILE)
    assert find(wdir) == (1, str(wdir / CF.SPK_FILE), "")
    assert find(tmp_path / "m" / "gguf_q8_0") == (1, str(tmp_path / "m" / CF.SPK_FILE), "")   # a quant directory that does not exist: its parent's file
    rc, a, b = find(wdir, cap=8)
    assert rc == ERR_INVALID and (a, b) == ("", "") and "bytes are needed" in lib.q3tts_last_error(None).decode()

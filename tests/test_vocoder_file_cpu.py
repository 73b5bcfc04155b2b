"""The vocoder's weights file qwen3_tts_vocoder.gguf on the host: every relayout and rounding of the loader against the
oracle's arrays, the shape read back from the file, where a model directory's file is found, every refusal, and the converter. CPU only:
q3tts_k_voc_file_tensor returns what q3tts_engine_create would upload, and the engine's refusals happen before it looks for a device.
The files are written by tests/_voc_file.py from the oracle's synthetic vocoder, at the GPU parity tests' tiny shape and a second one.
"""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import _gguf as G
import _model_dir as MD
import _voc_file as VF

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = {"tiny": VF.shape_tiny, "b": VF.shape_b}
SEED = 5
P = VF.ARCH + "."


def _fields(vc):
    from q3tts import _abi
    return {n: (list(getattr(vc, n)) if n in ("upsample_ratios", "dec_rates") else getattr(vc, n)) for n, _ in _abi.VocoderConfig._fields_}


# ---- 1. the arrays ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("container", ["bf16", "f32_perturbed"])
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_every_file_array_equals_the_oracles(oracle, tmp_path, shape, container):
    """For every generator id (comp, which): the array the loader would upload == the oracle's array, bit for bit (device layout, after
    rounding). The F32 container holds the matrices' values moved by (1 -/+ 2^-12): only round-to-nearest-even brings every one of them
    back (truncation lands one bf16 step low wherever the factor is below 1). SnakeBeta pairs: within 1 f32 ulp of float(exp(double))
    recomputed here in numpy (libm against numpy); their bit-equality with the generator's is the GPU test's."""
    from q3tts import native
    vc = SHAPES[shape]()
    path = VF.write(tmp_path / VF.FILE, oracle, vc, SEED, container)
    want = VF.oracle_arrays(oracle, vc, SEED)
    ents = VF.entries(vc)
    assert len({(e.comp, e.which) for e in ents}) == len(ents) == len({e.name for e in ents})
    assert max(len(e.name) for e in ents) <= 56
    if container == "f32_perturbed":   # the container really holds other values than the bf16 ones, in F32
        rd = G.read(path)
        e = next(e for e in ents if e.name == "decoder.0.conv.weight")
        assert rd[e.name][1] == G.F32 and not np.array_equal(e.to_device(rd[e.name][0]), want[(e.comp, e.which)])
        assert np.array_equal(G.bf16_bits_to_f32(G.f32_to_bf16_bits(rd[e.name][0])), e.to_torch(want[(e.comp, e.which)]))
        trunc = (rd[e.name][0].view(np.uint32) & np.uint32(0xFFFF0000)).view(np.float32)
        assert not np.array_equal(trunc, e.to_torch(want[(e.comp, e.which)]))
    n_snake = 0
    for e in ents:
        got = native.k_voc_file_tensor(path, vc, e.comp, e.which)
        ref = want[(e.comp, e.which)]
        if e.kind in ("snake_a", "snake_b"):
            ev = VF.snake_eval(e.kind, ref)
            assert got.shape == ev.shape and np.all(np.abs(got.view(np.int32).astype(np.int64) - ev.view(np.int32).astype(np.int64)) <= 1), e.name
            n_snake += 1
        else:
            assert got.shape == ref.shape and np.array_equal(got.view(np.uint32), ref.view(np.uint32)), e.name
    assert n_snake == 2 * (1 + 7 * vc.n_dec_blocks)
    with pytest.raises(Exception, match=r"no tensor of id \(61, 0\)"):
        native.k_voc_file_tensor(path, vc, 61, 0)


# ---- 2. the shape from the file ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_config_from_file_reproduces_the_shape(oracle, tmp_path, shape):
    from q3tts import _abi, native
    vc = SHAPES[shape]()
    path = VF.write(tmp_path / VF.FILE, oracle, vc, SEED)
    base = _abi.default_config().vocoder   # the full shape: every field the file states has to change
    base.layer_scale_init = 0.125
    got = native.vocoder_config_from_file(path, base)
    want = _fields(vc)
    want["layer_scale_init"] = 0.125       # a generator parameter: no file states it
    assert _fields(got) == want
    assert base.latent_dim == 1024         # the caller's block is not written


def _dir_with_models(tmp_path, name="gguf"):
    m = MD.shape_b(text_vocab=1024)
    MD.write_dir(str(tmp_path / name), m)
    return m


def test_model_dir_finds_the_file_in_the_quant_directory_then_in_its_parent_else_leaves_the_block_alone(oracle, tmp_path):
    from q3tts import native
    m = _dir_with_models(tmp_path)
    base = MD.base_config()
    base.with_vocoder = 1
    before = bytes(base.vocoder)
    # none: the whole block stays
    cfg = native.config_from_model_dir(str(tmp_path), None, base=base)
    assert bytes(cfg.vocoder) == before and MD.file_fields(cfg.model) == MD.file_fields(m)
    # in the parent (the model directory): shape b
    VF.write(tmp_path / VF.FILE, oracle, VF.shape_b(), SEED)
    cfg = native.config_from_model_dir(str(tmp_path), None, base=base)
    want = _fields(VF.shape_b()); want["layer_scale_init"] = base.vocoder.layer_scale_init
    assert _fields(cfg.vocoder) == want and MD.file_fields(cfg.model) == MD.file_fields(m) and cfg.max_batch == 7
    # in the quant directory too: that one wins (the tiny shape)
    VF.write(tmp_path / "gguf" / VF.FILE, oracle, VF.shape_tiny(), SEED)
    cfg = native.config_from_model_dir(str(tmp_path), None, base=base)
    want = _fields(VF.shape_tiny()); want["layer_scale_init"] = base.vocoder.layer_scale_init
    assert _fields(cfg.vocoder) == want
    # with_vocoder = 0: the file is ignored
    base.with_vocoder = 0
    assert bytes(native.config_from_model_dir(str(tmp_path), None, base=base).vocoder) == before
    # a wrong file fails the call and leaves the config alone
    base.with_vocoder = 1
    VF.write(tmp_path / "gguf" / VF.FILE, oracle, VF.shape_tiny(), SEED, edit_meta={P + "latent_dim": VF.DROP})
    snap = bytes(base)
    rc, msg, _ = MD.call(tmp_path, None, base)
    assert rc == -1 and VF.FILE in msg and "'q3tts-vocoder.latent_dim' is missing" in msg and bytes(base) == snap


# ---- 3. the loader's refusals: q3tts_engine_create, on the host before it looks for a device -------------------------------------------------
def _create(wdir, vc):
    """q3tts_engine_create on a directory that holds only the vocoder file -> (status, message). A file that passed would go on to the
    device (or to 'no HIP device'), so every case here must be refused by the file check."""
    from q3tts import _abi
    lib = _abi.load_library()
    cfg = _abi.tiny_config(max_batch=1, n_ctx=128, with_vocoder=1)
    cfg.vocoder = vc
    cfg.weights_path = os.fsencode(str(wdir))
    h = C.c_void_p()
    rc = lib.q3tts_engine_create(C.byref(cfg), C.byref(h))
    assert rc != 0 and not h.value
    return rc, lib.q3tts_last_error(None).decode("utf-8", "replace")


def _nan_in(name, idx, value=np.nan):
    def edit(t):
        a = t[name].copy(); a.reshape(-1)[idx] = value; t[name] = a
    return edit


def _reshaped(name, shape):
    return lambda t: t.__setitem__(name, np.zeros(shape, dtype=np.float32))


REFUSALS = {
    # (shape, write kwargs, vocoder-config edit, what the message must hold)
    "missing tensor": ("b", dict(edit_tensors={"decoder.3.alpha": VF.DROP}), None, ["tensor 'decoder.3.alpha' is missing"]),
    "missing codebook": ("tiny", dict(edit_tensors={"codebook.15.weight": VF.DROP}), None, ["tensor 'codebook.15.weight' is missing"]),
    "shape": ("tiny", dict(edit_tensors=_reshaped("upsample.1.1.pwconv2.weight", (64, 192))), None,
              ["tensor 'upsample.1.1.pwconv2.weight'", "[64][192]", "[64][256]"]),
    "shape of a vector": ("b", dict(edit_tensors=_reshaped("decoder.2.block.3.act2.beta", (65,))), None, ["'decoder.2.block.3.act2.beta'", "[65]", "[64]"]),
    "metadata integer": ("tiny", dict(), lambda vc: setattr(vc, "sliding_window", 9), ["'q3tts-vocoder.attention.sliding_window' = 8", "configuration has 9"]),
    "metadata float": ("tiny", dict(), lambda vc: setattr(vc, "rope_theta", 5000.0), ["'q3tts-vocoder.rope.freq_base' = 10000", "5000"]),
    "metadata array": ("b", dict(), lambda vc: vc.dec_rates.__setitem__(1, 3), ["'q3tts-vocoder.decoder_rates' = [5, 4]", "[5, 3]"]),
    "metadata key missing": ("tiny", dict(edit_meta={P + "sample_rate": VF.DROP}), None, ["'q3tts-vocoder.sample_rate' is missing"]),
    "architecture": ("tiny", dict(edit_meta={"general.architecture": "qwen3"}), None, ["'general.architecture' = 'qwen3'"]),
    "tensor type": ("tiny", dict(raw_types={"pre_transformer.layers.1.mlp.up_proj.weight": 2}), None,
                    ["'pre_transformer.layers.1.mlp.up_proj.weight'", "unsupported ggml type 2"]),
    "NaN in a bias": ("tiny", dict(edit_tensors=_nan_in("decoder.6.conv.bias", 0)), None, ["'decoder.6.conv.bias'", "not finite"]),
    "infinity in a matrix": ("b", dict(container="f32", edit_tensors=_nan_in("upsample.0.0.conv.weight", 1234, np.inf)), None,
                             ["'upsample.0.0.conv.weight'", "not finite", "1234"]),
    "infinity in a log": ("tiny", dict(edit_tensors=_nan_in("decoder.2.block.0.alpha", 3, -np.inf)), None, ["'decoder.2.block.0.alpha'", "not finite"]),
}


@pytest.mark.parametrize("case", sorted(REFUSALS))
def test_engine_create_refuses_a_wrong_file_before_the_device(oracle, tmp_path, case):
    shape, kw, cfg_edit, needles = REFUSALS[case]
    vc = SHAPES[shape]()
    VF.write(tmp_path / VF.FILE, oracle, vc, SEED, **kw)
    if cfg_edit:
        cfg_edit(vc)
    rc, msg = _create(tmp_path, vc)
    assert rc == -1 and VF.FILE in msg, msg
    for n in needles:
        assert n in msg, (n, msg)


def test_engine_create_refuses_a_file_that_ends_early(oracle, tmp_path):
    vc = VF.shape_b()
    path = VF.write(tmp_path / VF.FILE, oracle, vc, SEED)
    raw = open(path, "rb").read()
    for cut in (len(raw) - 64, len(raw) // 2, 200, 10):   # inside the last tensor, inside the data, inside the metadata, inside the header
        with open(path, "wb") as f:
            f.write(raw[:cut])
        rc, msg = _create(tmp_path, vc)
        assert rc == -1 and VF.FILE in msg, (cut, msg)
    with open(path, "wb") as f:   # the last tensor is the output convolution's bias
        f.write(raw[:len(raw) - 64])
    assert "lies outside the file" in _create(tmp_path, vc)[1]


def test_the_file_in_the_parent_directory_is_checked_too_and_no_vocoder_means_no_check(oracle, tmp_path):
    from q3tts import _abi
    vc = VF.shape_tiny()
    os.makedirs(tmp_path / "gguf")
    VF.write(tmp_path / VF.FILE, oracle, vc, SEED, edit_tensors={"pre_conv.conv.bias": VF.DROP})
    rc, msg = _create(tmp_path / "gguf", vc)
    assert rc == -1 and "tensor 'pre_conv.conv.bias' is missing" in msg
    assert "pre_conv.conv.bias" in _create(str(tmp_path / "gguf") + "/", vc)[1]   # a trailing slash names the same directory
    # with_vocoder = 0: the wrong file is ignored, the create gets as far as opening the (absent) Talker file or the device
    lib = _abi.load_library()
    cfg = _abi.tiny_config(max_batch=1, n_ctx=128, with_vocoder=0)
    cfg.weights_path = os.fsencode(str(tmp_path / "gguf"))
    h = C.c_void_p()
    rc = lib.q3tts_engine_create(C.byref(cfg), C.byref(h))
    assert rc != 0 and not h.value and VF.FILE not in lib.q3tts_last_error(None).decode()


# ---- 4. the cross-checks of q3tts_vocoder_config_from_file ------------------------------------------------------------------------------------
def _shift_layers(t):   # one more layer than the metadata counts
    for k in [k for k in t if k.startswith("pre_transformer.layers.0.")]:
        t[k.replace("layers.0.", "layers.7.")] = t[k]


CROSS = {
    "layer count": ("tiny", dict(edit_meta={P + "block_count": 3}), ["'q3tts-vocoder.block_count' implies 3", "has 2"]),
    "an uncounted layer": ("tiny", dict(edit_tensors=_shift_layers), ["'q3tts-vocoder.block_count' implies 2", "has 3"]),
    "codebook count": ("tiny", dict(edit_meta={P + "n_codebooks": 15}), ["'q3tts-vocoder.n_codebooks' implies 15", "has 16"]),
    "up-sampling stage count": ("b", dict(edit_meta={P + "upsample_ratios": [3, 2]}), ["'q3tts-vocoder.upsample_ratios' implies 2", "has 1"]),
    "decoder block count": ("b", dict(edit_meta={P + "decoder_rates": [5, 4, 3]}), ["'q3tts-vocoder.decoder_rates' implies 3", "has 2"]),
    "table shape": ("tiny", dict(edit_meta={P + "codebook_size": 128}), ["tensor 'codebook.0.weight'", "[64][32]", "[128][32]"]),
    "table width": ("tiny", dict(edit_tensors=_reshaped("codebook.9.weight", (64, 16))), ["tensor 'codebook.9.weight'", "[64][16]", "[64][32]"]),
    "q_proj": ("tiny", dict(edit_meta={P + "attention.head_count": 4}), ["'pre_transformer.layers.0.self_attn.q_proj.weight'", "[64][64]", "[128][64]"]),
    "gate_proj": ("b", dict(edit_meta={P + "feed_forward_length": 96}), ["'pre_transformer.layers.0.mlp.gate_proj.weight'", "[128][64]", "[96][64]"]),
    "up-sampling ConvTranspose against its ratio": ("b", dict(edit_meta={P + "upsample_ratios": [2]}), ["'upsample.0.0.conv.weight'", "[64][64][3]", "[64][64][2]"]),
    "decoder ConvTranspose against its rate": ("b", dict(edit_meta={P + "decoder_rates": [5, 3]}), ["'decoder.2.block.1.conv.weight'", "[128][64][8]", "[128][64][6]"]),
    "channel halving": ("b", dict(edit_tensors=_reshaped("decoder.2.block.1.conv.weight", (128, 32, 8))), ["'decoder.2.block.1.conv.weight'", "[128][32][8]", "[128][64][8]"]),
    "decoder_dim": ("b", dict(edit_meta={P + "decoder_dim": 128}), ["'decoder.0.conv.weight'", "[256][64][7]", "[128][64][7]"]),
    "a key of another type": ("tiny", dict(edit_meta={P + "latent_dim": 64.0}), ["'q3tts-vocoder.latent_dim' is not an integer"]),
    "too many rates": ("tiny", dict(edit_meta={P + "decoder_rates": [2] * 9}), ["'q3tts-vocoder.decoder_rates' has 9 entries"]),
}


@pytest.mark.parametrize("case", sorted(CROSS))
def test_config_from_file_cross_checks(oracle, tmp_path, case):
    from q3tts import _abi
    shape, kw, needles = CROSS[case]
    path = VF.write(tmp_path / VF.FILE, oracle, SHAPES[shape](), SEED, **kw)
    lib = _abi.load_library()
    vc = _abi.default_config().vocoder
    before = bytes(vc)
    err = C.create_string_buffer(1024)
    rc = lib.q3tts_vocoder_config_from_file(os.fsencode(path), C.byref(vc), err, len(err))
    msg = err.value.decode()
    assert rc == -1 and VF.FILE in msg and bytes(vc) == before, msg
    for n in needles:
        assert n in msg, (n, msg)


def test_config_from_file_io_errors_and_a_short_message_buffer(oracle, tmp_path):
    from q3tts import _abi
    lib = _abi.load_library()
    vc = _abi.default_config().vocoder
    err = C.create_string_buffer(b"\x55" * 16)
    assert lib.q3tts_vocoder_config_from_file(os.fsencode(str(tmp_path / "absent.gguf")), C.byref(vc), err, 8) == -4
    assert err.raw[7] == 0 and err.raw[8] == 0x55 and err.value == b"cannot "
    assert lib.q3tts_vocoder_config_from_file(None, C.byref(vc), None, 0) == -1


# ---- 5. the converter ----------------------------------------------------------------------------------------------------------------------
def _tool():
    sys.path.insert(0, os.path.join(REPO, "tools"))
    import vocoder_to_gguf
    return vocoder_to_gguf


def _family_checkpoint(vc, seed):
    """A randomly initialised Qwen3OmniMoeCode2Wav of the shape vc plus random codebook.* / pre_conv.* -> (state dict, CONFIG.json dict)."""
    torch = pytest.importorskip("torch")
    pytest.importorskip("transformers")
    from transformers.models.qwen3_omni_moe.modeling_qwen3_omni_moe import Qwen3OmniMoeCode2Wav
    from test_vocoder_family_cpu import _family_config
    torch.manual_seed(seed)
    fc = _family_config(vc)
    sd = {k: v.detach().clone().float().contiguous() for k, v in Qwen3OmniMoeCode2Wav(fc).state_dict().items()}
    for k in sd:   # (norm weights are ones, biases zeros at initialisation: make every value its own)
        sd[k] = sd[k] + 0.01 * torch.randn_like(sd[k])
    for q in range(vc.n_codebooks):
        sd[f"codebook.{q}.weight"] = torch.randn(vc.codebook_size, vc.codebook_dim)
    sd["pre_conv.conv.weight"] = torch.randn(vc.latent_dim, vc.codebook_dim, vc.pre_conv_kernel)
    sd["pre_conv.conv.bias"] = torch.randn(vc.latent_dim)
    cj = {"codebook_size": vc.codebook_size, "hidden_size": vc.latent_dim, "num_hidden_layers": vc.n_layer, "num_attention_heads": vc.n_head,
          "intermediate_size": vc.d_ffn, "sliding_window": vc.sliding_window, "rms_norm_eps": float(vc.rms_eps),
          "rope_parameters": {"rope_type": "default", "rope_theta": float(vc.rope_theta)}, "num_quantizers": vc.n_codebooks,
          "upsampling_ratios": [vc.upsample_ratios[i] for i in range(vc.n_upsample)], "upsample_rates": [vc.dec_rates[i] for i in range(vc.n_dec_blocks)],
          "decoder_dim": vc.decoder_dim, "head_dim": vc.head_dim}
    return sd, cj


def test_converter_copies_a_family_checkpoint_by_name(tmp_path):
    """safetensors -> GGUF -> read back: the table's names, PyTorch shapes and F32 values bit-equal, nothing else in the file (the
    family's code_embedding.weight stays out), the metadata == the config, and the library reads the shape back. Through the command line."""
    from safetensors.torch import save_file
    from q3tts import native
    vc = VF.shape_b()
    sd, cj = _family_checkpoint(vc, 3)
    assert "code_embedding.weight" in sd
    save_file({"decoder." + k: v for k, v in sd.items()}, str(tmp_path / "ck.safetensors"))
    (tmp_path / "config.json").write_text(json.dumps(cj))
    out = tmp_path / VF.FILE
    r = subprocess.run([sys.executable, os.path.join(REPO, "tools", "vocoder_to_gguf.py"), str(tmp_path / "ck.safetensors"), str(out),
                        "--config", str(tmp_path / "config.json"), "--prefix", "decoder."], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    rd = G.read(str(out))
    names = [e.name for e in VF.entries(vc)]
    assert sorted(rd) == sorted(names)
    for k in names:
        a, ty = rd[k]
        assert ty == G.F32 and a.shape == tuple(sd[k].shape) and np.array_equal(a.view(np.uint32), sd[k].numpy().view(np.uint32)), k
    got = native.vocoder_config_from_file(str(out), VF.shape_tiny())
    assert _fields(got) == _fields(vc)
    # --dtype bf16: matrices BF16 (nearest even), vectors and the depth-wise taps F32; the device arrays are those of the F32 file
    tool = _tool()
    torch = pytest.importorskip("torch")
    torch.save(sd, str(tmp_path / "ck.pt"))
    out16 = tmp_path / "bf16.gguf"
    tool.main([str(tmp_path / "ck.pt"), str(out16), "--config", str(tmp_path / "config.json"), "--dtype", "bf16"])
    rd16 = G.read(str(out16))
    assert rd16["decoder.1.block.1.conv.weight"][1] == G.BF16 and rd16["codebook.3.weight"][1] == G.BF16
    assert rd16["upsample.0.1.dwconv.conv.weight"][1] == G.F32 and rd16["pre_transformer.norm.weight"][1] == G.F32
    for e in VF.entries(vc):
        assert np.array_equal(native.k_voc_file_tensor(str(out16), vc, e.comp, e.which).view(np.uint32),
                              native.k_voc_file_tensor(str(out), vc, e.comp, e.which).view(np.uint32)), e.name


def test_converter_lists_every_missing_key(tmp_path):
    from safetensors.torch import save_file
    vc = VF.shape_b()
    sd, cj = _family_checkpoint(vc, 4)
    gone = ["decoder.2.block.3.act2.beta", "upsample.0.1.gamma"]
    save_file({k: v for k, v in sd.items() if k not in gone}, str(tmp_path / "ck.safetensors"))
    (tmp_path / "config.json").write_text(json.dumps(cj))
    r = subprocess.run([sys.executable, os.path.join(REPO, "tools", "vocoder_to_gguf.py"), str(tmp_path / "ck.safetensors"), str(tmp_path / "o.gguf"),
                        "--config", str(tmp_path / "config.json")], capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and all(k in r.stderr for k in gone) and "2 required key(s)" in r.stderr, r.stderr[-2000:]
    assert not os.path.exists(tmp_path / "o.gguf")


def test_converter_rvq_mimi_tables_sum_to_the_quantisers_decode(tmp_path):
    """--rvq mimi: 1 semantic + 15 acoustic residual quantisers as transformers' MimiSplitResidualVectorQuantizer holds them (random
    embed_sum, cluster_usage with entries under eps, random 1x1 output projections). The sum of the 16 looked-up table rows against the
    module's own decode run in float64. Bound 2e-6 of the largest |decode| element: a table entry is a float64 value rounded once to f32
    (relative 6e-8) and 16 of them are added here in float64, so the error is at most 16 x 6e-8 x max|table| — under 1e-6 of the largest
    element even if every rounding lined up; measured 2.4e-8."""
    torch = pytest.importorskip("torch")
    pytest.importorskip("transformers")
    from safetensors.torch import save_file
    from transformers.models.mimi.configuration_mimi import MimiConfig
    from transformers.models.mimi.modeling_mimi import MimiSplitResidualVectorQuantizer
    vc = VF.shape_b()
    mc = MimiConfig(codebook_size=vc.codebook_size, codebook_dim=24, vector_quantization_hidden_dimension=24, hidden_size=vc.codebook_dim,
                    num_quantizers=vc.n_codebooks, num_semantic_quantizers=1)
    torch.manual_seed(11)
    rvq = MimiSplitResidualVectorQuantizer(mc)
    with torch.no_grad():
        for half in (rvq.semantic_residual_vector_quantizer, rvq.acoustic_residual_vector_quantizer):
            half.output_proj.weight.copy_(torch.randn_like(half.output_proj.weight))
            for layer in half.layers:
                layer.codebook.embed_sum.copy_(torch.randn_like(layer.codebook.embed_sum) * 7)
                layer.codebook.cluster_usage.copy_(torch.rand_like(layer.codebook.cluster_usage) * 20)
                layer.codebook.cluster_usage[::9] = 1e-7   # under eps: the clamp decides
    sd, cj = _family_checkpoint(vc, 5)
    for q in range(vc.n_codebooks):
        del sd[f"codebook.{q}.weight"]
    sd.update({"quantizer." + k: v.detach().clone().float().contiguous() for k, v in rvq.state_dict().items()})
    save_file(sd, str(tmp_path / "ck.safetensors"))
    (tmp_path / "config.json").write_text(json.dumps(cj))
    out = tmp_path / VF.FILE
    _tool().main([str(tmp_path / "ck.safetensors"), str(out), "--config", str(tmp_path / "config.json"), "--rvq", "mimi"])
    rd = G.read(str(out))
    tabs = [rd[f"codebook.{q}.weight"][0] for q in range(vc.n_codebooks)]
    assert all(t.shape == (vc.codebook_size, vc.codebook_dim) for t in tabs)
    codes = torch.from_numpy(np.random.default_rng(6).integers(0, vc.codebook_size, size=(2, vc.n_codebooks, 40)))
    with torch.no_grad():
        ref = rvq.double().decode(codes).numpy()          # [B][hidden][T]
    got = np.zeros_like(ref)
    for q in range(vc.n_codebooks):
        got += tabs[q].astype(np.float64)[codes[:, q].numpy()].transpose(0, 2, 1)
    err = float(np.abs(got - ref).max() / np.abs(ref).max())
    print(f"--rvq mimi: sum of table rows vs the quantiser's float64 decode: {err:.1e} of the largest element")
    assert err <= 2e-6, err
    # a quantiser short of one layer's cluster_usage: named
    del sd["quantizer.acoustic_residual_vector_quantizer.layers.4.codebook.cluster_usage"]
    save_file(sd, str(tmp_path / "ck2.safetensors"))
    with pytest.raises(SystemExit, match="acoustic_residual_vector_quantizer.layers.4.codebook.cluster_usage"):
        _tool().main([str(tmp_path / "ck2.safetensors"), str(tmp_path / "o2.gguf"), "--config", str(tmp_path / "config.json"), "--rvq", "mimi"])

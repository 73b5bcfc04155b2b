#!/usr/bin/env python3
"""PyTorch speaker-encoder and codec-encoder checkpoints -> qwen3_tts_speaker_encoder.gguf + qwen3_tts_codec_encoder.gguf (the engine's
clone encoder weights files).

    clone_to_gguf.py SPEAKER_CKPT CODEC_CKPT OUT_DIR --config CONFIG.json [--dtype f32|bf16] [--speaker-prefix P] [--codec-prefix P]
                     [--n-codebooks N]

Each checkpoint is a .safetensors file (read with the safetensors package; refused plainly where it cannot be imported) or a torch.save'd
state dict. The files' tensor names ARE the state_dict keys of the model family's modules (transformers' ECAPA_TimeDelayNet; MimiModel's encoder, encoder_transformer,
downsample and the quantiser's two input_proj), in PyTorch layout: this tool copies them by name (after stripping the prefix) and never
relayouts — the engine's loader owns every relayout. Everything else in a checkpoint (decoder.*, output_proj, ...) is left out.

quantizer.codebook.{q}.weight [codebook_size][codebook_dim] is built here, because the family holds embed_sum and cluster_usage, not the
table: embed_sum / clamp(cluster_usage, eps)[:, None] in float64 with MimiEuclideanCodebook's own eps, stored as f32. The semantic quantiser
comes first, then the first N - 1 acoustic ones (N = --n-codebooks, default the config's num_quantizers).

CONFIG.json states the shape with the family configs' keys, either flat or under "speaker_encoder" / "codec_encoder": mel_dim, enc_channels,
enc_kernel_sizes, enc_dilations, enc_attention_channels, enc_res2net_scale, enc_se_channels, enc_dim; MimiConfig's num_filters, kernel_size,
residual_kernel_size, last_kernel_size, upsampling_ratios (the encoder runs them reversed), hidden_size, num_hidden_layers,
num_attention_heads, head_dim (default hidden_size / num_attention_heads), intermediate_size, sliding_window, rope_theta, norm_eps,
codebook_dim, codebook_size, num_quantizers. The frame-rate convolution's stride is the family's 2.

Refused, with the list of ALL reasons: missing keys, and config values the engine's structure cannot express (num_residual_layers != 1,
use_conv_shortcut, non-causal convolutions, num_semantic_quantizers != 1, num_key_value_heads != num_attention_heads, an activation other
than gelu_pytorch_tanh, compress != 2, a padding mode other than constant, codebook_dim != vector_quantization_hidden_dimension, a
frame-rate convolution whose kernel is not 4).

--dtype bf16 stores what the engine holds in bf16 anyway (convolution and projection matrices) as BF16, rounded to nearest even — the same
device bits as an f32 file at half the size; biases, LayerNorm, LayerScale and codebooks stay F32. Default f32.

The containers are written by the repository's GGUF writer (tests/_gguf.py).
"""
import argparse
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tests"))
import _gguf as G  # noqa: E402

SPK_ARCH, CODEC_ARCH = "q3tts-speaker-encoder", "q3tts-codec-encoder"
SPK_FILE, CODEC_FILE = "qwen3_tts_speaker_encoder.gguf", "qwen3_tts_codec_encoder.gguf"
DOWN_STRIDE = 2   # MimiModel.downsample: stride 2, kernel 2 * int(encodec_frame_rate / frame_rate)


def mimi_eps():
    """MimiEuclideanCodebook's own epsilon (the class default of the installed transformers; 1e-5 where it cannot be imported)."""
    try:
        import inspect
        from transformers.models.mimi.modeling_mimi import MimiEuclideanCodebook
        return float(inspect.signature(MimiEuclideanCodebook.__init__).parameters["epsilon"].default)
    except Exception:
        return 1e-5


def load_checkpoint(path):
    """-> {key: f32 ndarray}"""
    import torch
    if path.endswith(".safetensors"):
        try:
            from safetensors.torch import load_file
        except ImportError:
            raise SystemExit(f"{path}: reading a .safetensors file needs the safetensors package, which cannot be imported here; "
                             "install it, or give a torch.save'd state dict instead")
        sd = load_file(path)
    else:
        sd = torch.load(path, map_location="cpu", weights_only=True)
        if isinstance(sd, dict) and "state_dict" in sd and not any(hasattr(v, "shape") for v in sd.values()):
            sd = sd["state_dict"]
    return {k: v.detach().to(torch.float32).cpu().numpy() for k, v in sd.items() if hasattr(v, "detach")}


def strip(tensors, prefix):
    return {k[len(prefix):]: v for k, v in tensors.items() if k.startswith(prefix)} if prefix else dict(tensors)


def speaker_shape(cfg, problems):
    s = {}
    for key, name in (("mel_dim", "mel_dim"), ("enc_attention_channels", "attention_channels"), ("enc_res2net_scale", "res2net_scale"),
                      ("enc_se_channels", "se_channels"), ("enc_dim", "embedding_length")):
        if key not in cfg:
            problems.append(f"config: '{key}' is missing")
        else:
            s[name] = int(cfg[key])
    for key, name in (("enc_channels", "channels"), ("enc_kernel_sizes", "kernel_sizes"), ("enc_dilations", "dilations")):
        if key not in cfg:
            problems.append(f"config: '{key}' is missing")
        elif len(cfg[key]) != 5:
            problems.append(f"config: '{key}' has {len(cfg[key])} entries, the structure has 5 (TDNN, three SE-Res2Net blocks, aggregation)")
        else:
            s[name] = [int(v) for v in cfg[key]]
    return s


def codec_shape(cfg, n_codebooks, problems):
    s = {}
    for key, name in (("num_filters", "filters"), ("kernel_size", "kernel_size"), ("residual_kernel_size", "residual_kernel_size"),
                      ("last_kernel_size", "last_kernel_size"), ("hidden_size", "embedding_length"), ("num_hidden_layers", "block_count"),
                      ("num_attention_heads", "attention.head_count"), ("intermediate_size", "feed_forward_length"),
                      ("sliding_window", "attention.sliding_window"), ("codebook_dim", "vq_dim"), ("codebook_size", "codebook_size")):
        if key not in cfg:
            problems.append(f"config: '{key}' is missing")
        else:
            s[name] = int(cfg[key])
    if "upsampling_ratios" not in cfg:
        problems.append("config: 'upsampling_ratios' is missing")
    else:
        s["ratios"] = [int(r) for r in cfg["upsampling_ratios"]][::-1]
    if "attention.head_count" in s and "embedding_length" in s:
        s["attention.key_length"] = int(cfg.get("head_dim") or s["embedding_length"] // s["attention.head_count"])
    rope = cfg.get("rope_theta")
    if rope is None:
        rope = (cfg.get("rope_parameters") or {}).get("rope_theta", 10000.0)
    s["rope.freq_base"] = float(rope)
    if "norm_eps" not in cfg:
        problems.append("config: 'norm_eps' is missing")
    else:
        s["attention.layer_norm_epsilon"] = float(cfg["norm_eps"])
    s["down_stride"] = DOWN_STRIDE
    nq = cfg.get("num_quantizers")
    if n_codebooks is None and nq is None:
        problems.append("config: 'num_quantizers' is missing (or give --n-codebooks)")
    else:
        s["n_codebooks"] = int(n_codebooks if n_codebooks is not None else nq)
        if nq is not None and s["n_codebooks"] > int(nq):
            problems.append(f"--n-codebooks {s['n_codebooks']} exceeds the config's num_quantizers = {nq}")
        if s["n_codebooks"] < 1:
            problems.append(f"n_codebooks = {s['n_codebooks']}: at least the semantic quantiser is needed")
    # what the engine's structure cannot express
    heads = cfg.get("num_attention_heads")
    for key, ok, why in (
            ("num_residual_layers", lambda v: int(v) == 1, "the structure has one residual unit per stage"),
            ("use_conv_shortcut", lambda v: not v, "the residual units have an identity shortcut"),
            ("use_causal_conv", lambda v: bool(v), "every convolution is causal"),
            ("num_semantic_quantizers", lambda v: int(v) == 1, "the split quantiser has one semantic codebook"),
            ("num_key_value_heads", lambda v: heads is None or int(v) == int(heads), "the attention has one K/V head per query head (num_attention_heads = %s)" % heads),
            ("hidden_act", lambda v: v == "gelu_pytorch_tanh", "the MLP's activation is gelu_pytorch_tanh"),
            ("compress", lambda v: int(v) == 2, "a residual unit halves its channels"),
            ("pad_mode", lambda v: v == "constant", "the convolutions pad with zeros"),
            ("vector_quantization_hidden_dimension", lambda v: "codebook_dim" not in cfg or int(v) == int(cfg["codebook_dim"]),
             "the input projections map straight to codebook_dim = %s" % cfg.get("codebook_dim"))):
        if key in cfg and not ok(cfg[key]):
            problems.append(f"config: {key} = {cfg[key]!r} cannot be expressed: {why}")
    return s


def speaker_keys(s):
    bases = ["blocks.0.conv"]
    for i in (1, 2, 3):
        p = f"blocks.{i}."
        bases += [p + "tdnn1.conv"] + [p + f"res2net_block.blocks.{b}.conv" for b in range(s["res2net_scale"] - 1)]
        bases += [p + "tdnn2.conv", p + "se_block.conv1", p + "se_block.conv2"]
    bases += ["mfa.conv", "asp.tdnn.conv", "asp.conv", "fc"]
    return [b + x for b in bases for x in (".weight", ".bias")]


def codec_keys(s):
    """the copied tensors of the codec file (the codebooks are built, not copied)"""
    bases, li = ["encoder.layers.0.conv"], 1
    for _ in s["ratios"]:
        bases += [f"encoder.layers.{li}.block.1.conv", f"encoder.layers.{li}.block.3.conv", f"encoder.layers.{li + 2}.conv"]
        li += 3
    bases.append(f"encoder.layers.{li + 1}.conv")
    keys = [b + x for b in bases for x in (".weight", ".bias")]
    for l in range(s["block_count"]):
        p = f"encoder_transformer.layers.{l}."
        keys += [p + n for n in ("input_layernorm.weight", "input_layernorm.bias", "post_attention_layernorm.weight", "post_attention_layernorm.bias",
                                 "self_attn.q_proj.weight", "self_attn.k_proj.weight", "self_attn.v_proj.weight", "self_attn.o_proj.weight",
                                 "self_attn_layer_scale.scale", "mlp_layer_scale.scale", "mlp.fc1.weight", "mlp.fc2.weight")]
    keys += ["downsample.conv.weight", "quantizer.semantic_residual_vector_quantizer.input_proj.weight",
             "quantizer.acoustic_residual_vector_quantizer.input_proj.weight"]
    return keys


def codebooks(tensors, n_codebooks, eps):
    """quantizer.codebook.{q}.weight from the family's buffers: ({name: f32 table}, [missing keys])."""
    out, missing = {}, []
    for q in range(n_codebooks):
        root = ("quantizer.semantic_residual_vector_quantizer.layers.0." if q == 0 else f"quantizer.acoustic_residual_vector_quantizer.layers.{q - 1}.") + "codebook."
        es, cu = tensors.get(root + "embed_sum"), tensors.get(root + "cluster_usage")
        missing += [k for k, v in ((root + "embed_sum", es), (root + "cluster_usage", cu)) if v is None]
        if es is not None and cu is not None:
            out[f"quantizer.codebook.{q}.weight"] = (es.astype(np.float64) / np.maximum(cu.astype(np.float64), eps)[:, None]).astype(np.float32)
    return out, missing


def is_bf16_tensor(name, arr):
    """What the engine holds in bf16: convolution and projection matrices; not the codebooks, not the vectors."""
    return name.endswith(".weight") and arr.ndim >= 2 and not name.startswith("quantizer.codebook.")


def convert(speaker_ckpt, codec_ckpt, out_dir, config, dtype="f32", speaker_prefix="", codec_prefix="", n_codebooks=None):
    with open(config) as f:
        cfg = json.load(f)
    spk_t, codec_t = strip(load_checkpoint(speaker_ckpt), speaker_prefix), strip(load_checkpoint(codec_ckpt), codec_prefix)
    problems = []
    ss = speaker_shape(cfg.get("speaker_encoder", cfg), problems)
    cs = codec_shape(cfg.get("codec_encoder", cfg), n_codebooks, problems)
    if problems and not ({"res2net_scale"} <= set(ss) and {"ratios", "block_count", "n_codebooks"} <= set(cs)):
        raise SystemExit("cannot convert, %d problem(s):\n  %s" % (len(problems), "\n  ".join(problems)))
    sk, ck = speaker_keys(ss), codec_keys(cs)
    books, missing_books = codebooks(codec_t, cs["n_codebooks"], mimi_eps())
    codec_t.update(books)
    ck += [f"quantizer.codebook.{q}.weight" for q in range(cs["n_codebooks"])]
    missing = [f"speaker checkpoint: {k}" for k in sk if k not in spk_t]
    missing += [f"codec checkpoint: {k}" for k in ck if k not in codec_t and not k.startswith("quantizer.codebook.")]
    missing += [f"codec checkpoint: {k}" for k in missing_books]
    if missing:
        problems.append("the checkpoints lack %d required key(s):\n    %s" % (len(missing), "\n    ".join(missing)))
    dw = codec_t.get("downsample.conv.weight")
    if dw is not None and (dw.ndim != 3 or dw.shape[2] != 2 * DOWN_STRIDE):
        problems.append(f"downsample.conv.weight has shape {list(dw.shape)}: the frame-rate convolution's kernel must be {2 * DOWN_STRIDE} (stride {DOWN_STRIDE})")
    if problems:
        raise SystemExit("cannot convert, %d problem(s):\n  %s" % (len(problems), "\n  ".join(problems)))
    os.makedirs(out_dir, exist_ok=True)
    metas = []
    for arch, fname, shape, keys, tens in ((SPK_ARCH, SPK_FILE, ss, sk, spk_t), (CODEC_ARCH, CODEC_FILE, cs, ck, codec_t)):
        meta = {"general.architecture": arch}
        meta.update({arch + "." + k: v for k, v in shape.items()})
        G.write(os.path.join(out_dir, fname), [(k, tens[k], G.BF16 if dtype == "bf16" and is_bf16_tensor(k, tens[k]) else G.F32) for k in keys], meta=meta)
        metas.append(meta)
    return sk, ck, metas


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("speaker_ckpt")
    ap.add_argument("codec_ckpt")
    ap.add_argument("out_dir")
    ap.add_argument("--config", required=True)
    ap.add_argument("--dtype", choices=("f32", "bf16"), default="f32")
    ap.add_argument("--speaker-prefix", default="", help="key prefix to strip from the speaker checkpoint (keys without it are dropped)")
    ap.add_argument("--codec-prefix", default="", help="key prefix to strip from the codec checkpoint (keys without it are dropped)")
    ap.add_argument("--n-codebooks", type=int, default=None, help="codebooks to keep: the semantic one and the first N - 1 acoustic ones (default: num_quantizers)")
    a = ap.parse_args(argv)
    sk, ck, _ = convert(a.speaker_ckpt, a.codec_ckpt, a.out_dir, a.config, a.dtype, a.speaker_prefix, a.codec_prefix, a.n_codebooks)
    for fname, keys in ((SPK_FILE, sk), (CODEC_FILE, ck)):
        p = os.path.join(a.out_dir, fname)
        print(f"{p}: {len(keys)} tensors, {os.path.getsize(p)} bytes")


if __name__ == "__main__":
    main()

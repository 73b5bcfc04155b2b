#!/usr/bin/env python3
"""PyTorch vocoder checkpoint -> qwen3_tts_vocoder.gguf (the engine's vocoder weights file).

    vocoder_to_gguf.py CHECKPOINT OUT.gguf --config CONFIG.json [--dtype f32|bf16] [--prefix decoder.] [--rvq mimi [--rvq-prefix quantizer.]]

CHECKPOINT is a .safetensors file or a torch.save'd state dict. The file's tensor names ARE the state_dict keys of the model family's
module (transformers' Qwen3OmniMoeCode2Wav) plus codebook.{q}.weight and pre_conv.conv.{weight,bias}, in PyTorch layout: this tool
copies them by name (after stripping --prefix) and never relayouts — the engine's loader owns every relayout. A checkpoint that lacks a
required key is refused with the list of ALL missing keys.

CONFIG.json states the shape: the family config's keys (codebook_size, hidden_size, num_hidden_layers, num_attention_heads,
intermediate_size, sliding_window, rms_norm_eps, rope_theta or rope_parameters.rope_theta, num_quantizers, upsampling_ratios,
upsample_rates, decoder_dim) and optionally head_dim (default hidden_size / num_attention_heads), lookahead_frames (0), sample_rate
(24000). codebook_dim and pre_conv_kernel are read off pre_conv.conv.weight [hidden_size][codebook_dim][kernel].

--dtype bf16 stores what the engine holds in bf16 anyway (matrices, convolutions, codebook tables) as BF16, rounded to nearest even —
the same device bits as an f32 file at half the size; vectors stay F32. Default f32.

--rvq mimi builds codebook.{q}.weight from a split residual vector quantiser held the way transformers' Mimi holds it (keys under
--rvq-prefix): {semantic,acoustic}_residual_vector_quantizer.layers.{i}.codebook.{embed_sum,cluster_usage} and each half's 1x1
output_proj.weight. table_q = (embed_sum / clamp(cluster_usage, eps)) @ W_proj^T in float64, stored as f32 — already projected, so the
sum of the n_codebooks looked-up rows is the quantiser's decode. Semantic quantisers come first. eps is MimiEuclideanCodebook's.

The container is written by the repository's GGUF writer (tests/_gguf.py).
"""
import argparse
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tests"))
import _gguf as G  # noqa: E402

ARCH = "q3tts-vocoder"
MIMI_EPS = 1e-5   # transformers.models.mimi.modeling_mimi.MimiEuclideanCodebook(epsilon=1e-5)


def load_checkpoint(path):
    """-> {key: f32 ndarray}"""
    import torch
    if path.endswith(".safetensors"):
        from safetensors.torch import load_file
        sd = load_file(path)
    else:
        sd = torch.load(path, map_location="cpu", weights_only=True)
        if isinstance(sd, dict) and "state_dict" in sd and not any(hasattr(v, "shape") for v in sd.values()):
            sd = sd["state_dict"]
    return {k: v.detach().to(torch.float32).cpu().numpy() for k, v in sd.items() if hasattr(v, "detach")}


def shape_from_config(cfg, tensors):
    """The metadata's numbers (plain dict) from CONFIG.json and pre_conv.conv.weight."""
    rope = cfg.get("rope_theta")
    if rope is None:
        rope = (cfg.get("rope_parameters") or {}).get("rope_theta", 10000.0)
    s = {
        "n_codebooks": int(cfg["num_quantizers"]), "codebook_size": int(cfg["codebook_size"]), "latent_dim": int(cfg["hidden_size"]),
        "block_count": int(cfg["num_hidden_layers"]), "attention.head_count": int(cfg["num_attention_heads"]),
        "attention.key_length": int(cfg.get("head_dim") or cfg["hidden_size"] // cfg["num_attention_heads"]),
        "feed_forward_length": int(cfg["intermediate_size"]), "attention.sliding_window": int(cfg["sliding_window"]),
        "rope.freq_base": float(rope), "attention.layer_norm_rms_epsilon": float(cfg["rms_norm_eps"]),
        "upsample_ratios": [int(r) for r in cfg["upsampling_ratios"]], "decoder_dim": int(cfg["decoder_dim"]),
        "decoder_rates": [int(r) for r in cfg["upsample_rates"]],
        "lookahead_frames": int(cfg.get("lookahead_frames", 0)), "sample_rate": int(cfg.get("sample_rate", 24000)),
    }
    pre = tensors.get("pre_conv.conv.weight")
    s["codebook_dim"] = int(cfg["codebook_dim"]) if "codebook_dim" in cfg else (int(pre.shape[1]) if pre is not None and pre.ndim == 3 else 0)
    s["pre_conv_kernel"] = int(cfg["pre_conv_kernel"]) if "pre_conv_kernel" in cfg else (int(pre.shape[2]) if pre is not None and pre.ndim == 3 else 0)
    return s


def required_keys(s):
    """Every tensor name of the file for the shape s, in the loader's order."""
    keys = [f"codebook.{q}.weight" for q in range(s["n_codebooks"])] + ["pre_conv.conv.weight", "pre_conv.conv.bias"]
    for l in range(s["block_count"]):
        p = f"pre_transformer.layers.{l}."
        keys += [p + n for n in ("input_layernorm.weight", "post_attention_layernorm.weight", "self_attn_layer_scale.scale", "mlp_layer_scale.scale",
                                 "self_attn.q_proj.weight", "self_attn.k_proj.weight", "self_attn.v_proj.weight", "self_attn.o_proj.weight",
                                 "mlp.gate_proj.weight", "mlp.up_proj.weight", "mlp.down_proj.weight")]
    keys.append("pre_transformer.norm.weight")
    for u in range(len(s["upsample_ratios"])):
        p = f"upsample.{u}."
        keys += [p + n for n in ("0.conv.weight", "0.conv.bias", "1.dwconv.conv.weight", "1.dwconv.conv.bias", "1.norm.weight", "1.norm.bias",
                                 "1.pwconv1.weight", "1.pwconv1.bias", "1.pwconv2.weight", "1.pwconv2.bias", "1.gamma")]
    keys += ["decoder.0.conv.weight", "decoder.0.conv.bias"]
    nb = len(s["decoder_rates"])
    for b in range(nb):
        p = f"decoder.{1 + b}.block."
        keys += [p + n for n in ("0.alpha", "0.beta", "1.conv.weight", "1.conv.bias")]
        for u in range(3):
            keys += [p + f"{2 + u}." + n for n in ("act1.alpha", "act1.beta", "conv1.conv.weight", "conv1.conv.bias",
                                                   "act2.alpha", "act2.beta", "conv2.conv.weight", "conv2.conv.bias")]
    keys += [f"decoder.{1 + nb}.alpha", f"decoder.{1 + nb}.beta", f"decoder.{2 + nb}.conv.weight", f"decoder.{2 + nb}.conv.bias"]
    return keys


def mimi_tables(tensors, prefix, n_codebooks):
    """codebook.{q}.weight from a Mimi-style split RVQ: ({name: f32 table}, [missing keys])."""
    out, missing, q = {}, [], 0
    for half in ("semantic", "acoustic"):
        root = f"{prefix}{half}_residual_vector_quantizer."
        n = 0
        while f"{root}layers.{n}.codebook.embed_sum" in tensors or f"{root}layers.{n}.codebook.cluster_usage" in tensors:
            n += 1
        proj = tensors.get(root + "output_proj.weight")   # Conv1d [hidden][vq_dim][1]; absent when the two dimensions are equal
        W = None if proj is None else proj.reshape(proj.shape[0], proj.shape[1]).astype(np.float64)
        for i in range(n):
            es, cu = tensors.get(f"{root}layers.{i}.codebook.embed_sum"), tensors.get(f"{root}layers.{i}.codebook.cluster_usage")
            missing += [k for k, v in ((f"{root}layers.{i}.codebook.embed_sum", es), (f"{root}layers.{i}.codebook.cluster_usage", cu)) if v is None]
            if es is not None and cu is not None:
                embed = es.astype(np.float64) / np.maximum(cu.astype(np.float64), MIMI_EPS)[:, None]
                out[f"codebook.{q}.weight"] = (embed if W is None else embed @ W.T).astype(np.float32)
            q += 1
    if q != n_codebooks:
        missing.append(f"{prefix}*_residual_vector_quantizer.layers.*: {q} quantisers found, the config's num_quantizers is {n_codebooks}")
    return out, missing


def is_bf16_tensor(name, arr):
    """What the engine holds in bf16 (or as bf16-representable f32): matrices, convolutions and the codebook tables; not the depth-wise taps."""
    return name.endswith(".weight") and arr.ndim >= 2 and "dwconv" not in name


def convert(checkpoint, out, config, dtype="f32", prefix="", rvq=None, rvq_prefix="quantizer."):
    every = load_checkpoint(checkpoint)
    tensors = {k[len(prefix):]: v for k, v in every.items() if k.startswith(prefix)} if prefix else dict(every)
    with open(config) as f:
        cfg = json.load(f)
    missing = []
    if rvq == "mimi":
        tabs, missing = mimi_tables(every, rvq_prefix, int(cfg["num_quantizers"]))
        tensors.update(tabs)
    elif rvq is not None:
        raise SystemExit(f"--rvq {rvq}: only 'mimi' is known")
    s = shape_from_config(cfg, tensors)
    keys = required_keys(s)
    missing += [k for k in keys if k not in tensors]
    if missing:
        raise SystemExit("the checkpoint lacks %d required key(s):\n  %s" % (len(missing), "\n  ".join(missing)))
    meta = {"general.architecture": ARCH}
    meta.update({ARCH + "." + k: v for k, v in s.items()})
    G.write(out, [(k, tensors[k], G.BF16 if dtype == "bf16" and is_bf16_tensor(k, tensors[k]) else G.F32) for k in keys], meta=meta)
    return keys, meta


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("checkpoint")
    ap.add_argument("out")
    ap.add_argument("--config", required=True)
    ap.add_argument("--dtype", choices=("f32", "bf16"), default="f32")
    ap.add_argument("--prefix", default="", help="key prefix to strip (keys without it are dropped), e.g. decoder.")
    ap.add_argument("--rvq", default=None, help="'mimi': build codebook.{q}.weight from a Mimi-style split residual quantiser")
    ap.add_argument("--rvq-prefix", default="quantizer.", help="where the quantiser's keys start in the checkpoint (--prefix does not apply to them)")
    a = ap.parse_args(argv)
    keys, _ = convert(a.checkpoint, a.out, a.config, a.dtype, a.prefix, a.rvq, a.rvq_prefix)
    print(f"{a.out}: {len(keys)} tensors, {os.path.getsize(a.out)} bytes")


if __name__ == "__main__":
    main()

"""The clone encoders' weights files (qwen3_tts_speaker_encoder.gguf, qwen3_tts_codec_encoder.gguf) written from the oracle's
synthetic encoders — test infrastructure.

`entries(c)` is the table of DESIGN.md §29 once more, independent of csrc/q3_gguf.cpp: for every tensor id (comp, which) of
oracle/q3_oracle_clone.c (the ids tests/_clone_family.py loads the family's modules with) its generator call, the file it belongs to and the
file's tensor name(s). `device_array` is the oracle's array of an id as the device holds it, `tensors` the same values in the PyTorch layouts
the files hold, `write` puts them into two GGUF containers with tests/_gguf.py.
"""
import os

import numpy as np

import _gguf as G
import _oracle as O

SPK_ARCH, CODEC_ARCH = "q3tts-speaker-encoder", "q3tts-codec-encoder"
SPK_FILE, CODEC_FILE = "qwen3_tts_speaker_encoder.gguf", "qwen3_tts_codec_encoder.gguf"
SPK, CODEC = 0, 1


def tid(comp, w):
    return (5 << 16) | (comp << 8) | w


def round512(k):
    return (k + 511) // 512 * 512


def shape_tiny():
    from q3tts import _abi
    return _abi.tiny_clone_config()


def shape_b():
    """A second shape put together from tests/_clone_shapes.py: the speaker shape "s2" (Res2Net scale 2, other kernels and dilations, an
    aggregation convolution with k = 3, se_dim 16) and an audio encoder with two stages, three layers, one head of 96 (n_head * head_dim !=
    ae_hidden), a stride-3 frame-rate convolution and three codebooks of 1000 x 48 — so that index arithmetic in names (encoder.layers.{3 i +
    1}, the last convolution's index, res2net_block.blocks.{p - 1}, layers.{l}) and the q / k / v row blocks cannot hide behind the tiny one."""
    import _clone_shapes as CS
    kw = dict(CS.SPEAKER["s2"])
    for name in ("heads1x96", "down3", "vq1000x48x3"):
        kw.update(CS.AUDIO[name][0])
    kw.update(ae_n_ratios=2, ae_ratios=[4, 5], ae_n_layer=3)
    return CS.make(**kw)


class Entry:
    """One generator id. kind 'conv' (Conv1d [n][cin][k]; a Linear is k = None, [n][cin]; 'qkv' three Linear [n / 3][cin]) | 'vec' (gen = base,
    std) | 'book' ([n][cin] f32 table). names: the file's tensors, in the order their rows stack on the device."""

    def __init__(self, file, comp, which, kind, names, n, cin=0, k=None, gen=None):
        self.file, self.comp, self.which, self.kind, self.names, self.n, self.cin, self.k, self.gen = file, comp, which, kind, names, n, cin, k, gen

    @property
    def is_matrix(self):
        return self.kind in ("conv", "qkv")


def entries(c):
    out = []

    def conv(file, comp, ww, base, n, cin, k, bias=True):
        out.append(Entry(file, comp, ww, "conv", [base + ".weight"], n, cin, k))
        if bias:
            out.append(Entry(file, comp, ww + 1, "vec", [base + ".bias"], n, gen=(0.0, 0.02)))

    C, C4, S = c.se_channels[0], c.se_channels[4], c.se_res2net_scale
    conv(SPK, 0, 0, "blocks.0.conv", C, c.mel_dim, c.se_kernels[0])
    for i in (1, 2, 3):
        p = f"blocks.{i}."
        conv(SPK, i, 0, p + "tdnn1.conv", C, C, 1)
        for br in range(1, S):
            conv(SPK, i, 16 + 2 * br, p + f"res2net_block.blocks.{br - 1}.conv", C // S, C // S, c.se_kernels[i])
        conv(SPK, i, 2, p + "tdnn2.conv", C, C, 1)
        conv(SPK, i, 4, p + "se_block.conv1", c.se_se_channels, C, 1)
        conv(SPK, i, 6, p + "se_block.conv2", C, c.se_se_channels, 1)
    conv(SPK, 8, 0, "mfa.conv", C4, 3 * C, c.se_kernels[4])
    conv(SPK, 9, 0, "asp.tdnn.conv", c.se_attn_channels, 3 * C4, 1)
    conv(SPK, 10, 0, "asp.conv", C4, c.se_attn_channels, 1)
    conv(SPK, 11, 0, "fc", c.se_dim, 2 * C4, 1)

    Ca = c.ae_filters
    conv(CODEC, 32, 0, "encoder.layers.0.conv", Ca, 1, c.ae_kernel)
    li = 1
    for i in range(c.ae_n_ratios):
        comp, r = 33 + 4 * i, c.ae_ratios[i]
        conv(CODEC, comp, 0, f"encoder.layers.{li}.block.1.conv", Ca // 2, Ca, c.ae_res_kernel)
        conv(CODEC, comp + 1, 0, f"encoder.layers.{li}.block.3.conv", Ca, Ca // 2, 1)
        conv(CODEC, comp + 2, 0, f"encoder.layers.{li + 2}.conv", 2 * Ca, Ca, 2 * r)
        li += 3
        Ca *= 2
    H, dq, F = c.ae_hidden, c.ae_n_head * c.ae_head_dim, c.ae_d_ffn
    conv(CODEC, 60, 0, f"encoder.layers.{li + 1}.conv", H, Ca, c.ae_last_kernel)
    ls = np.float32(c.ae_layer_scale)
    lsg = (float(ls), float(np.float32(0.1) * ls))
    for l in range(c.ae_n_layer):
        comp, p = 64 + l, f"encoder_transformer.layers.{l}."
        for w, name, gen in ((0, "input_layernorm.weight", (1.0, 0.05)), (1, "input_layernorm.bias", (0.0, 0.02)),
                             (5, "post_attention_layernorm.weight", (1.0, 0.05)), (6, "post_attention_layernorm.bias", (0.0, 0.02)),
                             (4, "self_attn_layer_scale.scale", lsg), (9, "mlp_layer_scale.scale", lsg)):
            out.append(Entry(CODEC, comp, w, "vec", [p + name], H, gen=gen))
        out.append(Entry(CODEC, comp, 2, "qkv", [p + f"self_attn.{x}_proj.weight" for x in "qkv"], 3 * dq, H))
        out.append(Entry(CODEC, comp, 3, "conv", [p + "self_attn.o_proj.weight"], H, dq))
        out.append(Entry(CODEC, comp, 7, "conv", [p + "mlp.fc1.weight"], F, H))
        out.append(Entry(CODEC, comp, 8, "conv", [p + "mlp.fc2.weight"], H, F))
    conv(CODEC, 100, 0, "downsample.conv", H, H, 2 * c.ae_down_stride, bias=False)
    conv(CODEC, 101, 0, "quantizer.semantic_residual_vector_quantizer.input_proj", c.ae_vq_dim, H, 1, bias=False)
    conv(CODEC, 102, 0, "quantizer.acoustic_residual_vector_quantizer.input_proj", c.ae_vq_dim, H, 1, bias=False)
    for q in range(c.ae_n_codebooks):
        out.append(Entry(CODEC, 110 + q, 0, "book", [f"quantizer.codebook.{q}.weight"], c.ae_codebook_size, c.ae_vq_dim))
    return out


_CACHE = {}


def device_array(c, seed, e):
    """The oracle generator's array of entry e as the device holds it: matrices [n][round512(k * cin)] bf16-representable with the K padding
    zeroed (the files hold no padding; the generator fills it, and no kernel reads it: the im2col rows are zero there), vectors and codebooks
    as generated. Computed once per (shape, seed, id); read-only."""
    key = (bytes(c), int(seed), e.comp, e.which)
    if key not in _CACHE:
        if e.kind == "vec":
            a = O.synth_tensor(seed, tid(e.comp, e.which), (e.n,), e.gen[0], e.gen[1], False)
        elif e.kind == "book":
            a = O.synth_tensor(seed, tid(e.comp, e.which), (e.n, e.cin), 0.0, float(np.float32(1.0) / np.sqrt(np.float32(e.cin))), False)
        else:
            kc = (e.k or 1) * e.cin
            a = O.synth_tensor(seed, tid(e.comp, e.which), (e.n, round512(kc)), 0.0, float(np.float32(1.0) / np.sqrt(np.float32(kc))), True)
            a[:, kc:] = 0.0
        a.setflags(write=False)
        _CACHE[key] = a
    return _CACHE[key]


def tensors(c, seed):
    """({name: array}, {name: array}) — the speaker and the codec file's tensors in PyTorch layout, of the synthetic encoders (c, seed)."""
    files = ({}, {})
    for e in entries(c):
        a = device_array(c, seed, e)
        if e.kind in ("vec", "book"):
            files[e.file][e.names[0]] = a.copy()
        elif e.kind == "qkv":
            for j, name in enumerate(e.names):
                files[e.file][name] = np.ascontiguousarray(a[j * (e.n // 3):(j + 1) * (e.n // 3), :e.cin])
        elif e.k is None:
            files[e.file][e.names[0]] = np.ascontiguousarray(a[:, :e.cin])
        else:
            files[e.file][e.names[0]] = np.ascontiguousarray(a[:, :e.k * e.cin].reshape(e.n, e.k, e.cin).transpose(0, 2, 1))
    return files


def matrix_names(c):
    return {n for e in entries(c) if e.is_matrix for n in e.names}


def meta(c):
    s, a = SPK_ARCH + ".", CODEC_ARCH + "."
    spk = {"general.architecture": SPK_ARCH, s + "mel_dim": c.mel_dim, s + "channels": list(c.se_channels), s + "kernel_sizes": list(c.se_kernels),
           s + "dilations": list(c.se_dilations), s + "attention_channels": c.se_attn_channels, s + "res2net_scale": c.se_res2net_scale,
           s + "se_channels": c.se_se_channels, s + "embedding_length": c.se_dim}
    codec = {"general.architecture": CODEC_ARCH, a + "filters": c.ae_filters, a + "kernel_size": c.ae_kernel,
             a + "residual_kernel_size": c.ae_res_kernel, a + "last_kernel_size": c.ae_last_kernel,
             a + "ratios": [int(c.ae_ratios[i]) for i in range(c.ae_n_ratios)], a + "embedding_length": c.ae_hidden, a + "block_count": c.ae_n_layer,
             a + "attention.head_count": c.ae_n_head, a + "attention.key_length": c.ae_head_dim, a + "feed_forward_length": c.ae_d_ffn,
             a + "attention.sliding_window": c.ae_window, a + "rope.freq_base": float(c.ae_rope_theta),
             a + "attention.layer_norm_epsilon": float(c.ae_ln_eps), a + "down_stride": c.ae_down_stride, a + "vq_dim": c.ae_vq_dim,
             a + "n_codebooks": c.ae_n_codebooks, a + "codebook_size": c.ae_codebook_size}
    return spk, codec


def perturb(a):
    """v (1 -/+ 2^-12), the sign alternating: exact in f32 for a bf16-representable v, nearer to v than to any other bf16 value — so
    round-to-nearest-even gives v back and truncation gives v's lower neighbour at every element scaled down."""
    s = np.where(np.arange(a.size).reshape(a.shape) % 2 == 0, np.float32(1 - 2.0 ** -12), np.float32(1 + 2.0 ** -12)).astype(np.float32)
    return (a * s).astype(np.float32)


DROP = object()


def _edit(dct, edit):
    if callable(edit):
        edit(dct)
    elif edit:
        for k, v in edit.items():
            if v is DROP:
                dct.pop(k, None)
            else:
                dct[k] = v


def write(spk_dir, codec_dir, c, seed, container="bf16", edit_spk=None, edit_codec=None, edit_spk_meta=None, edit_codec_meta=None, raw_types=None):
    """The synthetic encoders (c, seed) as a pair of weights files; a directory of None leaves that file out. container: "bf16" (matrices
    BF16, the rest F32), "f32" (all F32) or "f32_perturbed" (all F32, the matrices' values moved off their bf16 values by `perturb`).
    edit_*: dict name -> replacement (DROP removes the entry) or a callable changing the dict in place. Returns the two paths."""
    tens, mt = tensors(c, seed), meta(c)
    mats = matrix_names(c)
    paths = []
    for i, (d, fname, et, em) in enumerate(((spk_dir, SPK_FILE, edit_spk, edit_spk_meta), (codec_dir, CODEC_FILE, edit_codec, edit_codec_meta))):
        if d is None:
            paths.append(None)
            continue
        t = dict(tens[i])
        if container == "f32_perturbed":
            t = {k: (perturb(v) if k in mats else v) for k, v in t.items()}
        m = dict(mt[i])
        _edit(t, et)
        _edit(m, em)
        os.makedirs(str(d), exist_ok=True)
        path = os.path.join(str(d), fname)
        G.write(path, [(k, v, G.BF16 if (container == "bf16" and k in mats) else G.F32) for k, v in t.items()], meta=m, raw_types=raw_types)
        paths.append(path)
    return tuple(paths)

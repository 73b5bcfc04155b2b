"""The vocoder's weights file (qwen3_tts_vocoder.gguf) written from the oracle's synthetic vocoder — test infrastructure.

`entries(vc)` is the table of DESIGN.md §27 once more, independent of csrc/q3_gguf.cpp: for every tensor id (comp, which) of
oracle/q3_oracle_vocoder.c its generator call (the values tests/test_vocoder_family_cpu.py::_load_family uses), the file's tensor name and
the map from the oracle's array (device layout) to the PyTorch layout the file holds. `tensors(vc, seed)` applies it through
q3o_vocoder_mat / q3o_vocoder_vec; `write` puts the dict into a GGUF container with tests/_gguf.py.
"""
import ctypes as C

import numpy as np

import _gguf as G

ARCH = "q3tts-vocoder"
FILE = "qwen3_tts_vocoder.gguf"
VC_CODEBOOK, VC_PRE, VC_TFM, VC_FINAL_NORM, VC_UP, VC_DEC_IN, VC_BLK, VC_OUT = 0, 32, 40, 60, 64, 72, 80, 120
(VW_W, VW_B, VW_IN_NORM, VW_Q, VW_K, VW_V, VW_O, VW_LS_ATTN, VW_POST_NORM, VW_GATE, VW_UP, VW_DOWN, VW_LS_MLP, VW_DW_W, VW_DW_B, VW_LN_W, VW_LN_B,
 VW_PW1, VW_PW1_B, VW_PW2, VW_PW2_B, VW_GAMMA, VW_ALPHA, VW_BETA, VW_W2, VW_B2, VW_ALPHA2, VW_BETA2) = range(28)


def shape_tiny():
    """The vocoder block of the GPU parity tests' tiny shape."""
    from q3tts import _abi
    return _abi.VocoderConfig.from_buffer_copy(_abi.tiny_config().vocoder)


def shape_b():
    """A second tiny shape: other layer, up-sampling-stage and decoder-block counts and other rates, so that index arithmetic in names
    (decoder.{1+b}, decoder.{2+nb}, upsample.{u}) cannot hide behind the first one."""
    vc = shape_tiny()
    vc.n_layer = 3
    vc.n_upsample = 1
    vc.upsample_ratios[:] = [3, 0, 0, 0]
    vc.decoder_dim, vc.n_dec_blocks = 256, 2
    vc.dec_rates[:] = [5, 4, 0, 0, 0, 0, 0, 0]
    return vc


def samples_per_frame(vc):
    return int(np.prod([vc.upsample_ratios[i] for i in range(vc.n_upsample)] + [vc.dec_rates[i] for i in range(vc.n_dec_blocks)]))


class Entry:
    """One generator id: kind 'mat' (gen = rows, cols, fan_in, gain; bf16-representable) | 'vec' (gen = n, base, std) | 'snake_a' |
    'snake_b' (a 'vec' of logs whose device array is the evaluated value); name = the file's tensor; to_torch: oracle array -> PyTorch
    layout; to_device: the inverse, on the file's (raw) values."""

    def __init__(self, comp, which, kind, gen, name, to_torch, to_device):
        self.comp, self.which, self.kind, self.gen, self.name, self.to_torch, self.to_device = comp, which, kind, gen, name, to_torch, to_device


def entries(vc):
    d, H, F, dd = vc.latent_dim, vc.n_head * vc.head_dim, vc.d_ffn, vc.decoder_dim
    out = []
    flat = lambda a: a.reshape(-1)

    def vec(comp, which, name, n, base, std, kind="vec"):
        out.append(Entry(comp, which, kind, (n, base, std), name, lambda a: a.reshape(n), flat))

    def mat(comp, which, name, rows, cols, fan_in, gain=1.0):
        out.append(Entry(comp, which, "mat", (rows, cols, fan_in, gain), name, lambda a: a.reshape(rows, cols), flat))

    def conv(comp, which, name, ntap, cin, nout, gain=1.0):  # oracle [tap][n][ci] <-> Conv1d [n][ci][tap]
        out.append(Entry(comp, which, "mat", (ntap * nout, cin, ntap * cin, gain), name,
                         lambda a: a.reshape(ntap, nout, cin).transpose(1, 2, 0), lambda w: flat(w.transpose(2, 0, 1))))

    for q in range(vc.n_codebooks):
        mat(VC_CODEBOOK + q, VW_W, f"codebook.{q}.weight", vc.codebook_size, vc.codebook_dim, 16)
    conv(VC_PRE, VW_W, "pre_conv.conv.weight", vc.pre_conv_kernel, vc.codebook_dim, d)
    vec(VC_PRE, VW_B, "pre_conv.conv.bias", d, 0.0, 0.02)
    lsi = float(vc.layer_scale_init)
    for l in range(vc.n_layer):
        c, p = VC_TFM + l, f"pre_transformer.layers.{l}."
        vec(c, VW_IN_NORM, p + "input_layernorm.weight", d, 1.0, 0.05)
        vec(c, VW_POST_NORM, p + "post_attention_layernorm.weight", d, 1.0, 0.05)
        vec(c, VW_LS_ATTN, p + "self_attn_layer_scale.scale", d, lsi, 0.1 * lsi)
        vec(c, VW_LS_MLP, p + "mlp_layer_scale.scale", d, lsi, 0.1 * lsi)
        for w, nm in ((VW_Q, "q"), (VW_K, "k"), (VW_V, "v")):
            mat(c, w, p + f"self_attn.{nm}_proj.weight", H, d, d)
        mat(c, VW_O, p + "self_attn.o_proj.weight", d, H, H)
        mat(c, VW_GATE, p + "mlp.gate_proj.weight", F, d, d)
        mat(c, VW_UP, p + "mlp.up_proj.weight", F, d, d)
        mat(c, VW_DOWN, p + "mlp.down_proj.weight", d, F, F)
    vec(VC_FINAL_NORM, VW_W, "pre_transformer.norm.weight", d, 1.0, 0.05)
    for u in range(vc.n_upsample):
        c, r, p = VC_UP + u, vc.upsample_ratios[u], f"upsample.{u}."
        # oracle [j][o][i] <-> ConvTranspose1d [in][out][k]
        out.append(Entry(c, VW_W, "mat", (r * d, d, d, 1.0), p + "0.conv.weight",
                         lambda a, r=r: a.reshape(r, d, d).transpose(2, 1, 0), lambda w: flat(w.transpose(2, 1, 0))))
        vec(c, VW_B, p + "0.conv.bias", d, 0.0, 0.02)
        out.append(Entry(c, VW_DW_W, "vec", (7 * d, 0.0, 0.3), p + "1.dwconv.conv.weight",
                         lambda a: a.reshape(7, d).T[:, None, :], lambda w: flat(w[:, 0, :].T)))
        vec(c, VW_DW_B, p + "1.dwconv.conv.bias", d, 0.0, 0.02)
        vec(c, VW_LN_W, p + "1.norm.weight", d, 1.0, 0.05)
        vec(c, VW_LN_B, p + "1.norm.bias", d, 0.0, 0.02)
        mat(c, VW_PW1, p + "1.pwconv1.weight", 4 * d, d, d)
        vec(c, VW_PW1_B, p + "1.pwconv1.bias", 4 * d, 0.0, 0.02)
        mat(c, VW_PW2, p + "1.pwconv2.weight", d, 4 * d, 4 * d)
        vec(c, VW_PW2_B, p + "1.pwconv2.bias", d, 0.0, 0.02)
        vec(c, VW_GAMMA, p + "1.gamma", d, 0.1, 0.01)
    conv(VC_DEC_IN, VW_W, "decoder.0.conv.weight", 7, d, dd)
    vec(VC_DEC_IN, VW_B, "decoder.0.conv.bias", dd, 0.0, 0.02)
    ch = dd
    for b in range(vc.n_dec_blocks):
        c, r, co, p = VC_BLK + 4 * b, vc.dec_rates[b], ch // 2, f"decoder.{1 + b}.block."
        vec(c, VW_ALPHA, p + "0.alpha", ch, 0.0, 0.1, "snake_a")
        vec(c, VW_BETA, p + "0.beta", ch, 0.0, 0.1, "snake_b")

        def ct_torch(a, r=r, co=co, ch=ch):   # oracle [tap][j][o][i]; tap 1 = the current latent step = kernel taps 0 .. r-1
            W = a.reshape(2, r, co, ch)
            w = np.zeros((ch, co, 2 * r), dtype=np.float32)
            w[:, :, :r] = W[1].transpose(2, 1, 0)
            w[:, :, r:] = W[0].transpose(2, 1, 0)
            return w

        def ct_device(w, r=r):
            return flat(np.stack([w[:, :, r:].transpose(2, 1, 0), w[:, :, :r].transpose(2, 1, 0)]))
        out.append(Entry(c, VW_W, "mat", (2 * r * co, ch, 2 * ch, 1.0), p + "1.conv.weight", ct_torch, ct_device))
        vec(c, VW_B, p + "1.conv.bias", co, 0.0, 0.02)
        for u in range(3):
            rc, q = c + 1 + u, p + f"{2 + u}."
            vec(rc, VW_ALPHA, q + "act1.alpha", co, 0.0, 0.1, "snake_a")
            vec(rc, VW_BETA, q + "act1.beta", co, 0.0, 0.1, "snake_b")
            conv(rc, VW_W, q + "conv1.conv.weight", 7, co, co, 0.5)
            vec(rc, VW_B, q + "conv1.conv.bias", co, 0.0, 0.02)
            vec(rc, VW_ALPHA2, q + "act2.alpha", co, 0.0, 0.1, "snake_a")
            vec(rc, VW_BETA2, q + "act2.beta", co, 0.0, 0.1, "snake_b")
            conv(rc, VW_W2, q + "conv2.conv.weight", 1, co, co, 0.5)
            vec(rc, VW_B2, q + "conv2.conv.bias", co, 0.0, 0.02)
        ch = co
    nb = vc.n_dec_blocks
    vec(VC_OUT, VW_ALPHA, f"decoder.{1 + nb}.alpha", ch, 0.0, 0.1, "snake_a")
    vec(VC_OUT, VW_BETA, f"decoder.{1 + nb}.beta", ch, 0.0, 0.1, "snake_b")
    conv(VC_OUT, VW_W, f"decoder.{2 + nb}.conv.weight", 7, ch, 1, 0.1)
    vec(VC_OUT, VW_B, f"decoder.{2 + nb}.conv.bias", 1, 0.0, 0.02)
    return out


def _lib(O):
    L = O.lib()
    L.q3o_vocoder_mat.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int64, C.c_int64, C.c_int32, C.c_float, C.c_void_p]
    L.q3o_vocoder_mat.restype = None
    L.q3o_vocoder_vec.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int64, C.c_float, C.c_float, C.c_void_p]
    L.q3o_vocoder_vec.restype = None
    return L


_CACHE = {}


def oracle_arrays(O, vc, seed):
    """{(comp, which): the oracle generator's flat f32 array} — for a SnakeBeta id the raw logs. Computed once per (shape, seed)."""
    key = (bytes(vc), int(seed))
    if key not in _CACHE:
        L = _lib(O)
        v = L.q3o_vocoder_create(C.byref(vc), seed, 1)
        try:
            got = {}
            for e in entries(vc):
                if e.kind == "mat":
                    rows, cols, fan_in, gain = e.gen
                    a = np.zeros(rows * cols, dtype=np.float32)
                    L.q3o_vocoder_mat(v, e.comp, e.which, rows, cols, fan_in, gain, a.ctypes.data)
                else:
                    n, base, std = e.gen
                    a = np.zeros(n, dtype=np.float32)
                    L.q3o_vocoder_vec(v, e.comp, e.which, n, base, std, a.ctypes.data)
                a.setflags(write=False)
                got[(e.comp, e.which)] = a
        finally:
            L.q3o_vocoder_destroy(v)
        _CACHE[key] = got
    return _CACHE[key]


def snake_eval(kind, logs):
    """What both sides evaluate in double on the host: exp(alpha), 1 / (exp(beta) + 1e-9), rounded to f32."""
    x = np.exp(logs.astype(np.float64))
    return (x if kind == "snake_a" else 1.0 / (x + 1e-9)).astype(np.float32)


def tensors(O, vc, seed):
    """The PyTorch-layout tensor dict (name -> f32 array; insertion order = creation order) of the synthetic vocoder (vc, seed)."""
    arr = oracle_arrays(O, vc, seed)
    return {e.name: np.ascontiguousarray(e.to_torch(arr[(e.comp, e.which)]), dtype=np.float32) for e in entries(vc)}


def meta(vc):
    p = ARCH + "."
    return {
        "general.architecture": ARCH,
        p + "n_codebooks": vc.n_codebooks, p + "codebook_size": vc.codebook_size, p + "codebook_dim": vc.codebook_dim,
        p + "latent_dim": vc.latent_dim, p + "pre_conv_kernel": vc.pre_conv_kernel,
        p + "block_count": vc.n_layer, p + "attention.head_count": vc.n_head, p + "attention.key_length": vc.head_dim,
        p + "feed_forward_length": vc.d_ffn, p + "attention.sliding_window": vc.sliding_window,
        p + "rope.freq_base": float(vc.rope_theta), p + "attention.layer_norm_rms_epsilon": float(vc.rms_eps),
        p + "upsample_ratios": [int(vc.upsample_ratios[i]) for i in range(vc.n_upsample)],
        p + "decoder_dim": vc.decoder_dim, p + "decoder_rates": [int(vc.dec_rates[i]) for i in range(vc.n_dec_blocks)],
        p + "lookahead_frames": vc.lookahead_frames, p + "sample_rate": vc.sample_rate,
    }


def perturb(a):
    """v (1 -/+ 2^-12), the sign alternating: exact in f32 for a bf16-representable v, nearer to v than to any other bf16 value — so
    round-to-nearest-even gives v back and truncation gives v's lower neighbour at every element scaled down."""
    s = np.where(np.arange(a.size).reshape(a.shape) % 2 == 0, np.float32(1 - 2.0 ** -12), np.float32(1 + 2.0 ** -12)).astype(np.float32)
    return (a * s).astype(np.float32)


DROP = object()


def write(path, O, vc, seed, container="bf16", edit_tensors=None, edit_meta=None, raw_types=None):
    """The synthetic vocoder (vc, seed) as a weights file. container: "bf16" (matrices BF16, the rest F32), "f32" (all F32) or
    "f32_perturbed" (all F32, the matrices' values moved off their bf16 values by `perturb`). edit_tensors / edit_meta: dict name ->
    replacement (DROP removes the entry) or a callable changing the dict in place."""
    tens, mt = tensors(O, vc, seed), meta(vc)
    is_mat = {e.name: e.kind == "mat" for e in entries(vc)}
    if container == "f32_perturbed":
        tens = {k: (perturb(v) if is_mat[k] else v) for k, v in tens.items()}
    for dct, edit in ((tens, edit_tensors), (mt, edit_meta)):
        if callable(edit):
            edit(dct)
        elif edit:
            for k, v in edit.items():
                if v is DROP:
                    dct.pop(k, None)
                else:
                    dct[k] = v
    G.write(str(path), [(k, v, G.BF16 if (container == "bf16" and is_mat.get(k, False)) else G.F32) for k, v in tens.items()], meta=mt, raw_types=raw_types)
    return str(path)

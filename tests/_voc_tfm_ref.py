"""Stage-isolated float64 references of the vocoder's front half: embedding sum, pre-conv, and per transformer layer the two norms, the four
projections, RoPE, the K / V ring and the sliding-window attention (tests/test_vocoder_tfm_stages_{cpu,gpu}.py). The sister of
tests/_voc_ref.py, whose tap format, weights, judge() and bounds machinery it uses.

A call is {name: (array[hist + T][C], hist)} as NativeEngine.vocoder_taps returns it (include/q3tts.h lists the names), together with the
position of its first frame and the codes of its frames. Every stage takes the device's own tapped operand, computes the stage in float64
from the oracle's weight generators and judges every element of the output tap on its own:

    embedding sum     bit for bit: the clamped codebook rows added in codebook order with f32 adds
    pre-conv, qkv     4 R sqrt(sum (x_i w_i)^2) + the f32 bias add (as tests/_voc_ref.py)
    o, down           |ls| 4 R sqrt(sum (x_i w_i)^2) + 2^-24 (|ls acc| + |x| + |x + ls acc|): the product and the sum, one rounding each
    gate / up         SiLU(gate) up with gate and up known to 4 R sqrt(..) each (|SiLU'| <= 1.1), three roundings and the exponential
    RMSNorm           4 R |x| rinv |w|
    RoPE (K rows)     2^-24 (2 |a cos| + 2 |b sin| + |result|): the rounded table entry and the rounded product, twice; the rounded sum
    V rows            bit for bit the v columns of the qkv tap
    attention         float64 softmax over positions max(0, pos - W + 1) .. pos of the tapped ring rows, q rotated in float64 from the qkv tap:
                      4 R A (1 + D) + 2 EXP_REL A, A_i = sum_j p_j |v_ji|, D = max_j scale sum_i |q_i k_ji| (the size of a score's terms)
    bf16 outputs      + half a bf16 step (judge_bf16)

The rotated q has no tap: the attention kernels keep it in LDS only. It is judged through the attention output alone, which is bf16, so a q
RoPE error below half a bf16 step (2^-9 relative) of that output passes; only the K rows' RoPE, which reads the same cos / sin table, is
judged at 2^-24.

R per stage kind: tests/_oracle.py VOC_STAGE_R, measured by restatement_R() on the CPU (tools/voc_stage_bounds.py)."""
import ctypes as C

import numpy as np

import _voc_ref as VR
from _voc_ref import EPS32, bf16_bits, conv64, judge, judge_bf16, operand

VC_CODEBOOK, VC_PRE, VC_TFM, VC_FINAL_NORM = 0, 32, 40, 60
VW_W, VW_B, VW_IN_NORM, VW_Q, VW_K, VW_V, VW_O, VW_LS_ATTN, VW_POST_NORM, VW_GATE, VW_UP, VW_DOWN, VW_LS_MLP = range(13)
FCAP = 4   # frames per call (VOC_FCAP): the ring holds sliding_window + FCAP rows
# The device's exponentials: expf in the attention kernels (1 ulp = 2^-23 in HIP's table), q3_expf in k_bgemm's SwiGLU (2.2e-7 relative,
# DESIGN.md 4.5), against libm's in float64. 2^-21 = 4.8e-7 is twice the larger of the two classes, stated before any device run.
EXP_REL = 2.0 ** -21
R_KINDS = ("pre", "rmsnorm", "qkv", "o", "gu", "down", "attn")
TINY = 1e-300   # keeps 0 / 0 out of a ratio where operand and allowance are both exactly zero


# The shapes of tests/test_vocoder_tfm_stages_gpu.py and tools/voc_stage_bounds.py: the vocoder fields changed on the tiny config ("full" is
# the shipped shape). hd128 / hd64t: every K a multiple of 256, the projections on k_bgemm from A-tiled bf16; hd128 and hd96: k_voc_attn only
# (two full 64-wide trips of its score loop; one and a half); hd48: k_voc_attn_lds with a row stride of 49 floats; w1: one key, a ring of 5
# rows; w508: the largest window the ring allows (score rows of 512 almost full, the LDS kernel not eligible).
SHAPES = {
    "tiny": {},
    "hd128": dict(latent_dim=256, n_head=2, head_dim=128, d_ffn=512, sliding_window=10),
    "hd64t": dict(latent_dim=256, n_head=4, head_dim=64, d_ffn=256, sliding_window=10),
    "hd96": dict(n_head=1, head_dim=96),
    "hd48": dict(n_head=2, head_dim=48),
    "w1": dict(sliding_window=1),
    "w508": dict(sliding_window=508),
}


def shape_vocoder(vc, name):
    for k, val in SHAPES[name].items():
        setattr(vc, k, val)
    return vc


def bind(L):
    L = VR.bind(L)
    L.q3o_vocoder_stages.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]
    L.q3o_vocoder_stages.restype = C.c_int32
    return L


class Dims:
    def __init__(self, vc):
        self.d, self.H, self.hd, self.F, self.W = vc.latent_dim, vc.n_head, vc.head_dim, vc.d_ffn, vc.sliding_window
        self.HH, self.RW, self.half = self.H * self.hd, self.W + FCAP, self.hd // 2
        self.cd, self.ncb, self.cbs, self.K, self.nl = vc.codebook_dim, vc.n_codebooks, vc.codebook_size, vc.pre_conv_kernel, vc.n_layer
        self.theta, self.eps, self.ls = float(vc.rope_theta), float(vc.rms_eps), np.float32(vc.layer_scale_init)


def layer(W, l):
    """The float64 tensors of transformer layer l from the oracle's generators (the calls of q3o_vocoder_create)."""
    k = ("tfm", l)
    if k not in W._m:
        D, comp = Dims(W.vc), VC_TFM + l
        ls_std = float(np.float32(0.1) * D.ls)   # the f32 product both sides form
        q, kk, v = (W.mat(comp, w, D.HH, D.d, D.d, 1.0) for w in (VW_Q, VW_K, VW_V))
        W._m[k] = dict(in_norm=W.vec(comp, VW_IN_NORM, D.d, 1.0, 0.05), post_norm=W.vec(comp, VW_POST_NORM, D.d, 1.0, 0.05),
                       ls_attn=W.vec(comp, VW_LS_ATTN, D.d, float(D.ls), ls_std), ls_mlp=W.vec(comp, VW_LS_MLP, D.d, float(D.ls), ls_std),
                       qkv=np.concatenate([q, kk, v]), o=W.mat(comp, VW_O, D.d, D.HH, D.HH, 1.0), gate=W.mat(comp, VW_GATE, D.F, D.d, D.d, 1.0),
                       up=W.mat(comp, VW_UP, D.F, D.d, D.d, 1.0), down=W.mat(comp, VW_DOWN, D.d, D.F, D.F, 1.0))
    return W._m[k]


def codebooks(W):
    D = Dims(W.vc)
    return [W.mat(VC_CODEBOOK + q, VW_W, D.cbs, D.cd, 16, 1.0).astype(np.float32) for q in range(D.ncb)]


def embed_f32(W, codes, skip=None, wrap=False):
    """k_voc_embed: the clamped codes' rows added in codebook order, f32. skip / wrap: the wrong kernels of the CPU test."""
    D, cb = Dims(W.vc), codebooks(W)
    out = np.zeros((codes.shape[0], D.cd), dtype=np.float32)
    for q in range(D.ncb):
        if q == skip:
            continue
        c = np.mod(codes[:, q], D.cbs) if wrap else np.clip(codes[:, q], 0, D.cbs - 1)
        out = (out + cb[q][c]).astype(np.float32)
    return out


def gemm64(x, w):
    acc, nrm = conv64(x, 0, w[None], 1)
    return acc, nrm


def rms64(x, w, eps, div=None):
    x = x.astype(np.float64)
    rinv = 1.0 / np.sqrt((x * x).sum(axis=1, keepdims=True) / (div or x.shape[1]) + eps)
    return x * rinv * w, np.abs(x) * rinv * np.abs(w)


def rope_tab(D, pos):
    """float64 cos / sin [len(pos)][half] of the angle pos * theta^(-2 i / hd)."""
    inv = np.power(D.theta, -2.0 * np.arange(D.half) / D.hd)
    ang = np.asarray(pos, dtype=np.float64)[:, None] * inv[None, :]
    return np.cos(ang), np.sin(ang)


def rope64(D, x, pos, interleaved=False):
    """x [T][HH] rotated half-split at positions pos -> (rotated, allowance), float64."""
    T = x.shape[0]
    cs, sn = rope_tab(D, pos)
    x = x.astype(np.float64).reshape(T, D.H, D.hd)
    a, b = (x[..., 0::2], x[..., 1::2]) if interleaved else (x[..., :D.half], x[..., D.half:])
    cs, sn = cs[:, None, :], sn[:, None, :]
    lo, hi = a * cs - b * sn, b * cs + a * sn
    alo = EPS32 * (2 * np.abs(a * cs) + 2 * np.abs(b * sn) + np.abs(lo))
    ahi = EPS32 * (2 * np.abs(b * cs) + 2 * np.abs(a * sn) + np.abs(hi))
    if interleaved:
        out, al = np.empty_like(x), np.empty_like(x)
        out[..., 0::2], out[..., 1::2], al[..., 0::2], al[..., 1::2] = lo, hi, alo, ahi
    else:
        out, al = np.concatenate([lo, hi], axis=-1), np.concatenate([alo, ahi], axis=-1)
    return out.reshape(T, D.HH), al.reshape(T, D.HH) + TINY


def attend64(D, q, kring, vring, pos0, window=None, oldest=None, scale_hd=None, drop_last_in_sum=False):
    """float64 sliding-window attention of the call's tokens from rotated q [T][HH] and the ring rows [RW][HH] -> (att, A, Dmax) [T][HH].
    window / oldest (position -> k row, v row in place of the window's oldest) / scale_hd {head: hd} / drop_last_in_sum: the wrong kernels of the CPU test."""
    T, Wn = q.shape[0], window or D.W
    att, A, Dm = (np.zeros((T, D.H, D.hd)) for _ in range(3))
    q = q.reshape(T, D.H, D.hd)
    for t in range(T):
        pos = pos0 + t
        j = np.arange(max(0, pos - Wn + 1), pos + 1)
        rows = j % D.RW
        k, v = kring[rows].astype(np.float64), vring[rows].astype(np.float64)
        if oldest is not None:
            k[0], v[0] = oldest(int(j[0]))
        k, v = k.reshape(-1, D.H, D.hd), v.reshape(-1, D.H, D.hd)
        for h in range(D.H):
            sc = 1.0 / np.sqrt(float((scale_hd or {}).get(h, D.hd)))
            s = sc * (k[:, h] @ q[t, h])
            p = np.exp(s - s.max())
            p /= p[:-1].sum() if drop_last_in_sum else p.sum()
            att[t, h] = p @ v[:, h]
            A[t, h] = p @ np.abs(v[:, h])
            Dm[t, h] = (sc * (np.abs(k[:, h]) @ np.abs(q[t, h]))).max()
    return att.reshape(T, D.HH), A.reshape(T, D.HH), Dm.reshape(T, D.HH)


def swiglu64(g, u):
    return g / (1.0 + np.exp(-g)) * u


def _out(res, stage, tap, ref, pre):
    """bf16 taps carry half a bf16 step on top of pre; f32 taps (the oracle's own, the final norm of the narrow shapes) do not."""
    if tap.dtype == np.uint16:
        judge_bf16(res, stage, tap, ref, pre)
    else:
        judge(res, stage, tap, ref, pre + TINY)


def _bits(res, stage, a, b):
    same = a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))
    res.append((stage, 0.0 if same else np.inf, ()))


def check_tfm_call(W, taps, R, pos0, codes, layers=None):
    """All front-half stages of one vocoder call whose first frame is at position pos0 and whose frames' codes are `codes` [T][n_codebooks]
    (as given to the device: out-of-range values included). R: {stage kind: measured normalised error of the restatement}; bound = 4 R.
    layers: the transformer layers to judge (default all; the embedding, the pre-conv and the final norm go with the first / last).
    Returns [(stage, worst error / bound, where)]."""
    res, D = [], Dims(W.vc)
    t = {k: v[0] for k, v in taps.items()}
    layers = range(D.nl) if layers is None else layers
    if 0 in layers:
        emb, H = taps["emb"]
        T = emb.shape[0] - H
        assert H == D.K - 1 and T == codes.shape[0], (H, T, codes.shape)
        _bits(res, "emb", emb[H:], embed_f32(W, codes))
        w, b = W.conv(VC_PRE, VW_W, VW_B, D.K, D.cd, D.d, D.d, 1.0)
        acc, nrm = conv64(operand(emb), H, w, 1)
        v = acc + b
        judge(res, "pre", t["x0"], v, 4 * R["pre"] * nrm + EPS32 * (np.abs(acc) + np.abs(b) + np.abs(v)))
    for l in layers:
        P, n = layer(W, l), f"l{l}"
        x = (t["x0"] if l == 0 else t[f"l{l - 1}.x_out"]).astype(np.float64)
        T = x.shape[0]
        pos = pos0 + np.arange(T)
        ref, sc = rms64(x, P["in_norm"], D.eps)
        _out(res, f"{n}.in_norm", t[f"{n}.xn"], ref, 4 * R["rmsnorm"] * sc)
        acc, nrm = gemm64(operand(t[f"{n}.xn"]), P["qkv"])
        qkv = t[f"{n}.qkv"]
        judge(res, f"{n}.qkv", qkv, acc, 4 * R["qkv"] * nrm + TINY)
        # the ring after the attention launch: this call's rows are the rotated k / the plain v of the qkv tap
        kring, vring = t[f"{n}.kring"], t[f"{n}.vring"]
        assert kring.shape == vring.shape == (D.RW, D.HH), (kring.shape, D.RW, D.HH)
        _bits(res, f"{n}.vring rows of the call == qkv v", vring[pos % D.RW], qkv[:, 2 * D.HH:])
        kref, kal = rope64(D, qkv[:, D.HH:2 * D.HH], pos)
        judge(res, f"{n}.rope k", kring[pos % D.RW], kref, kal)
        # attention over the tapped ring, q rotated here in float64 (the restatement behind R["attn"] rotates its q in f32 as the device does)
        q64 = rope64(D, qkv[:, :D.HH], pos)[0]
        att, A, Dm = attend64(D, q64, kring, vring, pos0)
        _out(res, f"{n}.attn", t[f"{n}.att"], att, 4 * R["attn"] * A * (1.0 + Dm) + 2 * EXP_REL * A)
        acc, nrm = gemm64(operand(t[f"{n}.att"]), P["o"])
        ls = P["ls_attn"]
        ref = x + ls * acc
        judge(res, f"{n}.o", t[f"{n}.x_att"], ref, np.abs(ls) * 4 * R["o"] * nrm + EPS32 * (np.abs(ls * acc) + np.abs(x) + np.abs(ref)) + TINY)
        x = t[f"{n}.x_att"].astype(np.float64)
        ref, sc = rms64(x, P["post_norm"], D.eps)
        _out(res, f"{n}.post_norm", t[f"{n}.xn2"], ref, 4 * R["rmsnorm"] * sc)
        xg = operand(t[f"{n}.xn2"])
        ga, gn = gemm64(xg, P["gate"])
        ua, un = gemm64(xg, P["up"])
        ref = swiglu64(ga, ua)
        silu = np.abs(swiglu64(ga, 1.0))
        dg, du = 4 * R["gu"] * gn, 4 * R["gu"] * un
        _out(res, f"{n}.gu", t[f"{n}.g"], ref, 1.1 * dg * (np.abs(ua) + du) + silu * du + (3 * EPS32 + EXP_REL) * np.abs(ref))
        acc, nrm = gemm64(operand(t[f"{n}.g"]), P["down"])
        ls = P["ls_mlp"]
        ref = x + ls * acc
        judge(res, f"{n}.down", t[f"{n}.x_out"], ref, np.abs(ls) * 4 * R["down"] * nrm + EPS32 * (np.abs(ls * acc) + np.abs(x) + np.abs(ref)) + TINY)
    if D.nl - 1 in layers:
        x = t[f"l{D.nl - 1}.x_out"].astype(np.float64)
        ref, sc = rms64(x, W.vec(VC_FINAL_NORM, VW_W, D.d, 1.0, 0.05), D.eps)
        _out(res, "final_norm", t["final.xn"], ref, 4 * R["rmsnorm"] * sc)
        if "up0.in" in taps:   # the buffer the first up-sampling GEMM reads is the one the final norm wrote
            a, b = t["final.xn"], t["up0.in"]
            res.append(("final.xn is up0.in", 0.0 if a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8)) else np.inf, ()))
    return res


def ring_carry(W, prev, nxt, pos0):
    """[(tap, ok)]: every ring row that the call at pos0 did not write equals the same row one call earlier, bit for bit (prev: the taps of the
    call before). On the device prev and nxt come from two runs of the same drive, and rows no call of the drive has written yet are whatever
    the buffer held. They are equal in both runs only because (1) q3_voc_reset leaves the rings' contents alone and (2) q3tts_k_vocoder_taps
    ends the drive at the tapped call, so no later call of the first run has written them. If reset starts clearing the rings, or the drive
    runs on past the tapped call, this check fails on those rows without any kernel being wrong."""
    D, out = Dims(W.vc), []
    for name, (a, _) in nxt.items():
        if not (name.endswith(".kring") or name.endswith(".vring")):
            continue
        T = nxt["x0"][0].shape[0]
        keep = np.ones(D.RW, dtype=bool)
        keep[(pos0 + np.arange(T)) % D.RW] = False
        out.append((name, bool(np.array_equal(a[keep].view(np.uint32), prev[name][0][keep].view(np.uint32)))))
    return out


# ---- the oracle's own stage data in tap format -------------------------------------------------------------------------------------------------
_LAYER_STAGES = ("xn", "q", "k", "v", "qr", "kr", "att", "x_att", "xn2", "g", "x_out")


def oracle_stages(W, codes):
    """{name: array} of one whole-utterance decode of the bf16-input oracle's front half (one decode: q3o_vocoder_stages)."""
    D, n = Dims(W.vc), codes.shape[0]
    want = {"emb": (5, D.cd), "x0": (1, D.d), "final.xn": (2, D.d)}
    width = {"xn": D.d, "x_att": D.d, "xn2": D.d, "x_out": D.d, "g": D.F}
    for l in range(D.nl):
        for k, s in enumerate(_LAYER_STAGES):
            want[f"l{l}.{s}"] = (500 + 20 * l + k, width.get(s, D.HH))
    out = {name: np.zeros((n, c), dtype=np.float32) for name, (_, c) in want.items()}
    names = list(want)
    ids = np.array([want[k][0] for k in names], dtype=np.int32)
    ptrs = (C.c_void_p * len(names))(*[out[k].ctypes.data for k in names])
    codes = np.ascontiguousarray(codes, dtype=np.int32)
    bind(W.L).q3o_vocoder_stages(W.v, codes.ctypes.data, n, len(names), ids.ctypes.data, ptrs)
    return out


def oracle_call_taps(W, S, pos0, nf, f32=False):
    """The call of nf frames at pos0 cut out of oracle_stages() as the device would have tapped it (bf16 buffers as bits unless f32; the ring as
    the calls up to this one left it, unwritten rows zero)."""
    D, taps = Dims(W.vc), {}
    rows = slice(pos0, pos0 + nf)
    H = D.K - 1
    emb = np.zeros((H + nf, D.cd), dtype=np.float32)
    lo = max(0, pos0 - H)
    emb[H - (pos0 - lo):] = S["emb"][lo:pos0 + nf]
    taps["emb"], taps["x0"] = (emb, H), (S["x0"][rows].copy(), 0)
    bf = (lambda a: a.copy()) if f32 else bf16_bits
    for l in range(D.nl):
        g = lambda s: S[f"l{l}.{s}"]   # noqa: E731
        taps[f"l{l}.xn"] = (bf(g("xn")[rows]), 0)
        taps[f"l{l}.qkv"] = (np.concatenate([g("q")[rows], g("k")[rows], g("v")[rows]], axis=1), 0)
        for ring, src in (("kring", "kr"), ("vring", "v")):
            a = np.zeros((D.RW, D.HH), dtype=np.float32)
            p = np.arange(max(0, pos0 + nf - D.RW), pos0 + nf)
            a[p % D.RW] = g(src)[p]
            taps[f"l{l}.{ring}"] = (a, 0)
        for name, s in (("att", "att"), ("xn2", "xn2"), ("g", "g")):
            taps[f"l{l}.{name}"] = (bf(g(s)[rows]), 0)
        taps[f"l{l}.x_att"], taps[f"l{l}.x_out"] = (g("x_att")[rows].copy(), 0), (g("x_out")[rows].copy(), 0)
    taps["final.xn"] = (S["final.xn"][rows].copy(), 0)
    return taps


def restatement_R(W, codes):
    """{stage kind: worst normalised error of the CPU restatement} on the bf16-input oracle's own activations of `codes`, call by call of 4
    frames: the chain of q3o_mfma_bf16_dot32 for the GEMM stages (the pre-conv's taps ascending, 32-wide K steps inside), the oracle's
    sequential f32 code for RMSNorm and the attention."""
    D, S, R = Dims(W.vc), oracle_stages(W, codes), {}

    def upd(kind, val):
        R[kind] = max(R.get(kind, 0.0), val)
    unit = {k: 0.25 for k in R_KINDS}   # 4 R = 1: ratio = error / scale
    for pos0 in range(0, codes.shape[0], FCAP):
        nf = min(FCAP, codes.shape[0] - pos0)
        taps = oracle_call_taps(W, S, pos0, nf, f32=True)
        for stage, ratio, _ in check_tfm_call(W, taps, unit, pos0, codes[pos0:pos0 + nf]):
            if stage.endswith("_norm"):
                upd("rmsnorm", ratio)
            elif stage.endswith(".attn"):
                upd("attn", ratio)
        emb, H = taps["emb"]
        upd("pre", VR.chain_R(W, bf16_bits(emb), H, W.conv(VC_PRE, VW_W, VW_B, D.K, D.cd, D.d, D.d, 1.0)[0], 1))
        for l in range(D.nl):
            P = layer(W, l)
            xn, xn2 = bf16_bits(taps[f"l{l}.xn"][0]), bf16_bits(taps[f"l{l}.xn2"][0])
            upd("qkv", VR.chain_R(W, xn, 0, P["qkv"][None], 1))
            upd("o", VR.chain_R(W, bf16_bits(taps[f"l{l}.att"][0]), 0, P["o"][None], 1))
            upd("gu", max(VR.chain_R(W, xn2, 0, P["gate"][None], 1), VR.chain_R(W, xn2, 0, P["up"][None], 1)))
            upd("down", VR.chain_R(W, bf16_bits(taps[f"l{l}.g"][0]), 0, P["down"][None], 1))
    return R

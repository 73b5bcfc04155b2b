"""Stage-isolated float64 references of the vocoder's convolution half (tests/test_vocoder_stages_{cpu,gpu}.py).

A "call" is a dict of taps {name: (array[hist + T][C], hist)} in the format of NativeEngine.vocoder_taps (include/q3tts.h lists the names):
f32 taps are float32, bf16 taps are uint16 bits. Every stage takes its INPUT tap as it is (the operand the MFMA consumed, history rows
included), computes the stage in numpy float64 from the oracle's weight generators, and judges every element of the OUTPUT tap on its own:

    |device - float64|  <=  4 R sqrt(sum_i (x_i w_i)^2)            the GEMM's accumulation; R = the measured error of the instruction model's
                                                                    own chain on that scale (tests/_oracle.py VOC_STAGE_R), 4x for regrouping
                          + n_ops 2^-24 (|operands| + |result|)     f32 element-wise epilogue arithmetic (bias, layer scale, residual): one
                                                                    rounding of half an ulp per operation, from the number format
                          + transcendental term                     device sinf / erff against libm, stated per function below
                          + half a bf16 step                        where the output buffer is bf16

check_call() returns [(stage, worst error / bound, where)]; a stage passes when its ratio is <= 1."""
import ctypes as C

import numpy as np

VC_UP, VC_DEC_IN, VC_BLK, VC_OUT = 64, 72, 80, 120
VW_W, VW_B, VW_DW_W, VW_DW_B, VW_LN_W, VW_LN_B, VW_PW1, VW_PW1_B, VW_PW2, VW_PW2_B, VW_GAMMA = 0, 1, 13, 14, 15, 16, 17, 18, 19, 20, 21
VW_ALPHA, VW_BETA, VW_W2, VW_B2, VW_ALPHA2, VW_BETA2 = 22, 23, 24, 25, 26, 27
DIL = (1, 3, 9)
EPS32 = 2.0 ** -24   # half an ulp of f32, relative

# Device sin is the fast intrinsic (__sinf: the argument times 1 / 2 pi in f32, then the hardware sine of a turn fraction). Its absolute error
# class is that of CUDA's __sinf, documented as 2^-21.41 on [-pi, pi] and growing with |x| through the f32 argument scaling; we allow
# 2^-18 + 2^-21 |x| (8x that class and two argument roundings), stated before any device run. SnakeBeta squares the sine (|d sin^2| <= 2 |d sin|).
SIN_ABS, SIN_ARG = 2.0 ** -18, 2.0 ** -21
# erff against libm: the last place of erf, amplified by (1 + erf) for negative x — tests/test_parity_gpu.py::test_bgemm_vocoder_epilogue_extras
# states it as 2^-20 |x| absolute, and so do we.
ERF_ABS = 2.0 ** -20


def bind(L):
    vp, i32 = C.c_void_p, C.c_int32
    L.q3o_vocoder_mat.argtypes = [vp, i32, i32, C.c_int64, C.c_int64, i32, C.c_float, vp]
    L.q3o_vocoder_mat.restype = None
    L.q3o_vocoder_vec.argtypes = [vp, i32, i32, C.c_int64, C.c_float, C.c_float, vp]
    L.q3o_vocoder_vec.restype = None
    L.q3o_vocoder_stage.argtypes = [vp, vp, i32, i32, vp]
    L.q3o_vocoder_stage.restype = i32
    L.q3o_vocoder_stage_inject.argtypes = [vp, vp, i32, i32, vp, i32, vp]
    L.q3o_vocoder_stage_inject.restype = i32
    L.q3o_vconv_mfma.argtypes = [vp, i32, i32, vp, i32, i32, i32, i32, vp, i32]
    L.q3o_vconv_mfma.restype = None
    return L


def bf16_bits(a):
    u = np.ascontiguousarray(a, dtype=np.float32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def bf16_val(bits):
    return (np.asarray(bits, dtype=np.uint16).astype(np.uint32) << 16).view(np.float32).astype(np.float64)


def operand(a):
    """A GEMM operand as the MFMA sees it, in float64: bf16 bits as they are, f32 rows rounded to bf16 (what the kernel does at load)."""
    return bf16_val(a) if a.dtype == np.uint16 else bf16_val(bf16_bits(a))


def half_bf16_step(x):
    """Half a bf16 step in the binade of |x| (float64 array)."""
    ax = np.maximum(np.abs(x), 2.0 ** -126)
    return 2.0 ** (np.floor(np.log2(ax)) - 8)


class Weights:
    """The synthetic vocoder's convolution-half tensors from the oracle's generators, as float64 (bf16-representable matrices, f32 vectors)."""

    def __init__(self, L, v, vc):
        self.L, self.v, self.vc, self._m = bind(L), v, vc, {}
        self.d = vc.latent_dim
        self.ups = [vc.upsample_ratios[i] for i in range(vc.n_upsample)]
        self.blocks, ch = [], vc.decoder_dim
        for b in range(vc.n_dec_blocks):
            self.blocks.append((vc.dec_rates[b], ch, ch // 2))
            ch //= 2
        self.out_c = ch

    def mat(self, comp, which, rows, cols, fan_in, gain):
        k = ("m", comp, which)
        if k not in self._m:
            out = np.zeros((rows, cols), dtype=np.float32)
            self.L.q3o_vocoder_mat(self.v, comp, which, rows, cols, fan_in, gain, out.ctypes.data)
            self._m[k] = out.astype(np.float64)
        return self._m[k]

    def vec(self, comp, which, n, base, std):
        k = ("v", comp, which)
        if k not in self._m:
            out = np.zeros(n, dtype=np.float32)
            self.L.q3o_vocoder_vec(self.v, comp, which, n, base, std, out.ctypes.data)
            self._m[k] = out.astype(np.float64)
        return self._m[k]

    def snake(self, comp, wa, wb, n):
        """(exp(alpha), 1 / (exp(beta) + 1e-9)): exp() in double, the parameters rounded to f32 as both sides store them."""
        a, b = self.vec(comp, wa, n, 0.0, 0.1), self.vec(comp, wb, n, 0.0, 0.1)
        return np.exp(a).astype(np.float32).astype(np.float64), (1.0 / (np.exp(b) + 1e-9)).astype(np.float32).astype(np.float64)

    def conv(self, comp, ww, wb, ntap, cin, nout, bias_n, gain):
        w = self.mat(comp, ww, ntap * nout, cin, ntap * cin, gain).reshape(ntap, nout, cin)
        return w, self.vec(comp, wb, bias_n, 0.0, 0.02)

    def next_snake(self, b, u):
        """SnakeBeta parameters of the consumer of unit u's sum in block b: the next unit, the next block's transposed convolution, the output."""
        C_ = self.blocks[b][2]
        if u < 2:
            return self.snake(VC_BLK + 4 * b + 2 + u, VW_ALPHA, VW_BETA, C_), f"b{b}.r{u + 1}.c1_in"
        if b + 1 < len(self.blocks):
            return self.snake(VC_BLK + 4 * (b + 1), VW_ALPHA, VW_BETA, C_), f"b{b + 1}.ct_in"
        return self.snake(VC_OUT, VW_ALPHA, VW_BETA, C_), "out.in"


def conv64(x, hist, w, dil):
    """Causal multi-tap convolution in float64: x [hist + T][cin] (hist >= (ntap-1)*dil), w [ntap][nout][cin] -> (acc [T][nout], norm [T][nout])
    with norm = sqrt(sum_i (x_i w_i)^2), the scale the accumulation error is measured on."""
    ntap, T = w.shape[0], x.shape[0] - hist
    acc = np.zeros((T, w.shape[1])); sq = np.zeros_like(acc)
    for tap in range(ntap):
        sh = (ntap - 1 - tap) * dil
        xs = x[hist - sh:hist - sh + T]
        acc += xs @ w[tap].T
        sq += (xs * xs) @ (w[tap] * w[tap]).T
    return acc, np.sqrt(sq)


def snake64(v, ea, ib):
    s = np.sin(v * ea)
    return v + ib * s * s


def snake_slack(v, dv, ea, ib):
    """Bound on |device SnakeBeta - float64 SnakeBeta| for an input known to within dv: the slope, the sine (SIN_*), three f32 roundings."""
    arg = np.abs(v * ea)
    dsin = SIN_ABS + SIN_ARG * arg + 2 * EPS32 * arg
    out = np.abs(snake64(v, ea, ib))
    return (1.0 + ib * ea) * dv + 2.0 * ib * dsin + 3 * EPS32 * (np.abs(v) + out)


def judge(res, stage, dev, ref, allowed):
    """Every element on its own: worst |dev - ref| / allowed."""
    dev = np.asarray(dev, dtype=np.float64)
    assert dev.shape == ref.shape == allowed.shape, (stage, dev.shape, ref.shape, allowed.shape)
    assert np.all(np.isfinite(dev)), stage
    ratio = np.abs(dev - ref) / allowed
    i = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
    res.append((stage, float(ratio[i]), tuple(int(k) for k in i)))


def judge_bf16(res, stage, dev_bits, ref, pre):
    """A bf16 output tap: half a bf16 step (of the larger of the two values) on top of the error allowed before the rounding."""
    dev = bf16_val(dev_bits)
    judge(res, stage, dev, ref, half_bf16_step(np.maximum(np.abs(ref), np.abs(dev))) + pre)


def check_call(W, taps, R):
    """All stages of one vocoder call. R: {stage kind: measured normalised error of the restatement} (tests/_oracle.py); bound = 4 R."""
    res, d = [], W.d
    t = {k: v[0] for k, v in taps.items()}
    h = {k: v[1] for k, v in taps.items()}
    for u, r in enumerate(W.ups):
        comp = VC_UP + u
        # ConvTranspose k = r, stride r: X W^T + bias[n % d], [T][r d] == [T r][d]
        w, b = W.conv(comp, VW_W, VW_B, 1, d, r * d, d, 1.0)
        x = operand(t[f"up{u}.in"])
        acc, nrm = conv64(x, 0, w, 1)
        bias = np.tile(b, r)[None, :]
        raw, H = t[f"up{u}.raw"], h[f"up{u}.raw"]
        T = raw.shape[0] - H
        judge(res, f"up{u}.ct", raw[H:], (acc + bias).reshape(T, d), (4 * R["up_ct"] * nrm + EPS32 * (np.abs(acc) + np.abs(bias) + np.abs(acc + bias))).reshape(T, d))
        # causal depthwise k = 7 over [history + T], bias, LayerNorm (biased variance, eps 1e-6)
        dw_w, dw_b = W.vec(comp, VW_DW_W, 7 * d, 0.0, 0.3).reshape(7, d), W.vec(comp, VW_DW_B, d, 0.0, 0.02)
        ln_w, ln_b = W.vec(comp, VW_LN_W, d, 1.0, 0.05), W.vec(comp, VW_LN_B, d, 0.0, 0.02)
        x = raw.astype(np.float64)
        dw, mag = np.tile(dw_b, (T, 1)), np.tile(np.abs(dw_b), (T, 1))
        for tap in range(7):
            xs = x[H - 6 + tap:H - 6 + tap + T]
            dw += xs * dw_w[tap]; mag += np.abs(xs * dw_w[tap])
        mean = dw.mean(axis=1, keepdims=True)
        rinv = 1.0 / np.sqrt(((dw - mean) ** 2).mean(axis=1, keepdims=True) + 1e-6)
        ln = (dw - mean) * rinv * ln_w + ln_b
        scale = mag.max(axis=1, keepdims=True) * rinv * np.abs(ln_w) + np.abs(ln) + np.abs(ln_b)
        if t[f"up{u}.ln"].dtype == np.uint16:
            judge_bf16(res, f"up{u}.dw_ln", t[f"up{u}.ln"], ln, 4 * R["dw_ln"] * scale)
        else:
            judge(res, f"up{u}.dw_ln", t[f"up{u}.ln"], ln, 4 * R["dw_ln"] * scale)
        # pointwise 1: GELU(X W1^T + b1)
        w, b = W.conv(comp, VW_PW1, VW_PW1_B, 1, d, 4 * d, 4 * d, 1.0)
        acc, nrm = conv64(operand(t[f"up{u}.ln"]), 0, w, 1)
        v = acc + b
        from math import sqrt
        erf = _erf(v / sqrt(2.0))
        g = 0.5 * v * (1.0 + erf)
        dv = 4 * R["pw1"] * nrm + EPS32 * (np.abs(acc) + np.abs(b) + np.abs(v))
        pre = 1.13 * dv + ERF_ABS * np.abs(v) + 4 * EPS32 * (np.abs(v) + np.abs(g))   # |GELU'| <= 1.13
        if t[f"up{u}.gelu"].dtype == np.uint16:
            judge_bf16(res, f"up{u}.pw1", t[f"up{u}.gelu"], g, pre)
        else:
            judge(res, f"up{u}.pw1", t[f"up{u}.gelu"], g, pre)
        # pointwise 2: raw + gamma (G W2^T + b2), in place behind the untouched history rows
        w, b = W.conv(comp, VW_PW2, VW_PW2_B, 1, 4 * d, d, d, 1.0)
        gamma = W.vec(comp, VW_GAMMA, d, 0.1, 0.01)
        acc, nrm = conv64(operand(t[f"up{u}.gelu"]), 0, w, 1)
        out = t[f"up{u}.out"]
        ref = x[H:] + gamma * (acc + b)
        allowed = np.abs(gamma) * (4 * R["pw2"] * nrm + EPS32 * (np.abs(acc) + np.abs(b) + 2 * np.abs(acc + b))) + EPS32 * (np.abs(x[H:]) + np.abs(ref))
        judge(res, f"up{u}.pw2", out[H:], ref, allowed)
        res.append((f"up{u}.history rows untouched by the residual", 0.0 if np.array_equal(out[:H].view(np.uint32), raw[:H].view(np.uint32)) else np.inf, ()))
        nxt = t[f"up{u + 1}.in"] if u + 1 < len(W.ups) else t["dec_in.in"][h["dec_in.in"]:]
        if nxt.dtype == np.uint16:   # the bf16 copy the next GEMM reads: RNE of the f32 result, bit for bit
            res.append((f"up{u}.out -> bf16 operand of the next stage", 0.0 if np.array_equal(nxt, bf16_bits(out[H:])) else np.inf, ()))
        else:
            res.append((f"up{u}.out -> f32 operand of the next stage", 0.0 if np.array_equal(nxt.view(np.uint32), out[H:].view(np.uint32)) else np.inf, ()))
    # decoder input convolution: causal k = 7, then block 0's SnakeBeta into its transposed convolution's buffer
    ch = W.blocks[0][1]
    w, b = W.conv(VC_DEC_IN, VW_W, VW_B, 7, d, ch, ch, 1.0)
    acc, nrm = conv64(operand(t["dec_in.in"]), h["dec_in.in"], w, 1)
    ea, ib = W.snake(VC_BLK, VW_ALPHA, VW_BETA, ch)
    v = acc + b
    dv = 4 * R["dec_in"] * nrm + EPS32 * (np.abs(acc) + np.abs(b) + np.abs(v))
    judge_bf16(res, "dec_in + snake", t["b0.ct_in"][h["b0.ct_in"]:], snake64(v, ea, ib), snake_slack(v, dv, ea, ib))
    for bi, (r, cin, cout) in enumerate(W.blocks):
        comp = VC_BLK + 4 * bi
        # transposed convolution k = 2 r, stride r, right-trimmed: two taps of [r cout] outputs, bias repeating every cout
        w, b = W.conv(comp, VW_W, VW_B, 2, cin, r * cout, cout, 1.0)
        acc, nrm = conv64(operand(t[f"b{bi}.ct_in"]), h[f"b{bi}.ct_in"], w, 1)
        bias = np.tile(b, r)[None, :]
        o_dev = t[f"b{bi}.o_ct"]
        T = o_dev.shape[0]
        judge(res, f"b{bi}.ct", o_dev, (acc + bias).reshape(T, cout), (4 * R["blk_ct"] * nrm + EPS32 * (np.abs(acc) + np.abs(bias) + np.abs(acc + bias))).reshape(T, cout))
        ea, ib = W.snake(comp + 1, VW_ALPHA, VW_BETA, cout)
        o = o_dev.astype(np.float64)
        judge_bf16(res, f"b{bi}.ct snake -> r0.c1_in", t[f"b{bi}.r0.c1_in"][h[f"b{bi}.r0.c1_in"]:], snake64(o, ea, ib), snake_slack(o, 0.0, ea, ib))
        for u in range(3):
            rc, dil, name = comp + 1 + u, DIL[u], f"b{bi}.r{u}"
            w1, b1 = W.conv(rc, VW_W, VW_B, 7, cout, cout, cout, 0.5)
            w2, b2 = W.conv(rc, VW_W2, VW_B2, 1, cout, cout, cout, 0.5)
            ea2, ib2 = W.snake(rc, VW_ALPHA2, VW_BETA2, cout)
            acc, nrm = conv64(operand(t[f"{name}.c1_in"]), h[f"{name}.c1_in"], w1, dil)
            v = acc + b1
            dv = 4 * R["res_c1"] * nrm + EPS32 * (np.abs(acc) + np.abs(b1) + np.abs(v))
            z64, dz = snake64(v, ea2, ib2), snake_slack(v, dv, ea2, ib2)
            flip = 0.0
            if f"{name}.z" in t:   # un-fused: SnakeBeta 2's bf16 output is a buffer of its own, and the second GEMM is judged on it
                judge_bf16(res, f"{name}.c1 + snake2 -> z", t[f"{name}.z"], z64, dz)
                z = bf16_val(t[f"{name}.z"])
            else:
                # fused: z stays in LDS. The reference rounds its own z to bf16; where the float64 value lies within dz of a rounding
                # boundary the device may legitimately have rounded to the other neighbour, one whole bf16 step away: that step, times |W2|,
                # is allowed for exactly those elements (computed, not assumed: far from a boundary nothing is added).
                zb = bf16_val(bf16_bits(z64.astype(np.float32)))
                step = 2 * half_bf16_step(z64)
                near = np.abs(np.abs(z64 - zb) - 0.5 * step) <= dz + np.abs(z64) * 2.0 ** -23
                flip = (near * step) @ np.abs(w2[0]).T
                z = zb
            acc2 = z @ w2[0].T
            nrm2 = np.sqrt((z * z) @ (w2[0] * w2[0]).T)
            c2 = acc2 + b2
            o_new = o + c2
            do = 4 * R["res_c2"] * nrm2 + flip + EPS32 * (np.abs(acc2) + np.abs(b2) + np.abs(c2) + np.abs(o) + np.abs(o_new))
            (ea, ib), cons = W.next_snake(bi, u)
            if u < 2:
                o_dev = t[f"{name}.o"]
                judge(res, f"{name}.o", o_dev, o_new, do)
                o = o_dev.astype(np.float64)
                judge_bf16(res, f"{name} snake -> {cons}", t[cons][h[cons]:], snake64(o, ea, ib), snake_slack(o, 0.0, ea, ib))
            else:   # the last unit's sum is never stored: it is judged through the consumer's SnakeBeta
                judge_bf16(res, f"{name}.o + snake -> {cons}", t[cons][h[cons]:], snake64(o_new, ea, ib), snake_slack(o_new, do, ea, ib))
    # output convolution: causal k = 7, C -> 1, clamp
    w, b = W.conv(VC_OUT, VW_W, VW_B, 7, W.out_c, 1, 1, 0.1)
    acc, nrm = conv64(operand(t["out.in"]), h["out.in"], w, 1)
    v = acc + b
    judge(res, "out conv + clamp", t["pcm"], np.clip(v, -1.0, 1.0), 4 * R["out"] * nrm + EPS32 * (np.abs(acc) + np.abs(b) + np.abs(v)))
    return res


def _erf(x):
    from scipy.special import erf
    return erf(x)


def history_carry(prev, nxt):
    """[(buffer, ok)]: the history rows at the start of a call equal the last H rows of the same buffer at the end of the call before, bit
    for bit (prev None: the first call after a reset, zeros). up<u>.raw is the buffer whose history the device keeps for the ConvNeXt stage."""
    out = []
    for name, (a, H) in nxt.items():
        if H == 0 or name.endswith(".out") and name.startswith("up"):
            continue
        want = np.zeros_like(a[:H]) if prev is None else prev[name][0][-H:]
        out.append((name, bool(np.array_equal(a[:H].view(np.uint16 if a.dtype == np.uint16 else np.uint32), want.view(np.uint16 if a.dtype == np.uint16 else np.uint32)))))
    return out


# ---- the oracle's own stage data in tap format (CPU tests; the GPU test never needs a whole oracle decode) ------------------------------------
def oracle_stage(W, codes, stage, shape, inject=None):
    out = np.zeros(shape, dtype=np.float32)
    codes = np.ascontiguousarray(codes, dtype=np.int32)
    if inject is None:
        W.L.q3o_vocoder_stage(W.v, codes.ctypes.data, codes.shape[0], stage, out.ctypes.data)
    else:
        inj = np.ascontiguousarray(inject[1], dtype=np.float32)
        W.L.q3o_vocoder_stage_inject(W.v, codes.ctypes.data, codes.shape[0], stage, out.ctypes.data, inject[0], inj.ctypes.data)
    return out


def stage_ids(W):
    """{tap name: (oracle stage id, rows per frame, channels, hist rows, bf16 on the device)} of one whole-utterance decode."""
    ids, rows, d = {}, 1, W.d
    for u, r in enumerate(W.ups):
        ids[f"up{u}.in"] = (100 + 10 * u, rows, d, 0, False)
        rows *= r
        ids[f"up{u}.raw"] = (101 + 10 * u, rows, d, 6, False)
        ids[f"up{u}.ln"] = (102 + 10 * u, rows, d, 0, False)
        ids[f"up{u}.gelu"] = (103 + 10 * u, rows, 4 * d, 0, False)
        ids[f"up{u}.out"] = (104 + 10 * u, rows, d, 6, False)
    ids["dec_in.in"] = (104 + 10 * (len(W.ups) - 1), rows, d, 6, True)
    for b, (r, cin, cout) in enumerate(W.blocks):
        ids[f"b{b}.ct_in"] = (300 + 20 * b, rows, cin, 1, True)
        rows *= r
        ids[f"b{b}.o_ct"] = (301 + 20 * b, rows, cout, 0, False)
        for u in range(3):
            ids[f"b{b}.r{u}.c1_in"] = (302 + 20 * b + 4 * u, rows, cout, 6 * DIL[u], True)
            ids[f"b{b}.r{u}.z"] = (304 + 20 * b + 4 * u, rows, cout, 0, True)
            if u < 2:
                ids[f"b{b}.r{u}.o"] = (305 + 20 * b + 4 * u, rows, cout, 0, False)
    ids["out.in"] = (400, rows, W.out_c, 6, True)
    ids["pcm"] = (4, rows, 1, 0, False)
    return ids


def oracle_taps(W, codes, fused=False, inject=None):
    """One whole-utterance decode of the bf16-input oracle as the taps of a single call on an empty history (zero history rows)."""
    taps, n = {}, codes.shape[0]
    for name, (sid, rpf, ch, H, is_bf) in stage_ids(W).items():
        if fused and name.endswith(".z"):
            continue
        a = oracle_stage(W, codes, sid, (n * rpf, ch), inject)
        if name == "pcm":
            a = np.clip(a, -1.0, 1.0)
        a = np.concatenate([np.zeros((H, ch), np.float32), a])
        taps[name] = (bf16_bits(a) if is_bf else a, H)
    return taps


# ---- the instruction model's own chain (bounds table of tests/_oracle.py; bit-equality checks) ----------------------------------------------
def mfma_chain(W, x_bits, hist, w, dil, max_rows=None, threads=8):
    """q3o_vconv_mfma over the first max_rows rows: the chain of q3o_mfma_bf16_dot32 in the device kernels' K-step order (vstep), f32."""
    ntap, nout, cin = w.shape
    assert hist == (ntap - 1) * dil and x_bits.dtype == np.uint16
    T = x_bits.shape[0] - hist
    T = min(T, max_rows) if max_rows else T
    x = np.ascontiguousarray(x_bits[:hist + T])
    wb = bf16_bits(w.astype(np.float32))
    out = np.zeros((T, nout), dtype=np.float32)
    chunked = 1 if (ntap == 7 and cin % 64 == 0 and cin >= 256) else 0
    W.L.q3o_vconv_mfma(x.ctypes.data, T, cin, wb.ctypes.data, ntap, dil, nout, chunked, out.ctypes.data, threads)
    return out


def chain_R(W, x_bits, hist, w, dil, max_rows=96):
    """Worst |chain - float64| / sqrt(sum (x_i w_i)^2) over the first max_rows rows."""
    got = mfma_chain(W, x_bits, hist, w, dil, max_rows)
    acc, nrm = conv64(bf16_val(x_bits[:hist + got.shape[0]]), hist, w, dil)
    return float((np.abs(got - acc) / np.maximum(nrm, 1e-300)).max())


def restatement_R(W, codes):
    """{stage kind: worst normalised error of the CPU restatement} on the bf16-input oracle's own activations of `codes`: the MFMA chain for
    the GEMM stages, the oracle's sequential f32 code for the element-wise stages (k_voc_dw_ln, the output convolution)."""
    taps = oracle_taps(W, codes)
    t = {k: (v[0] if v[0].dtype == np.uint16 else bf16_bits(v[0])) for k, v in taps.items()}
    h = {k: v[1] for k, v in taps.items()}
    d, R = W.d, {}

    def upd(kind, val):
        R[kind] = max(R.get(kind, 0.0), val)
    for u, r in enumerate(W.ups):
        comp = VC_UP + u
        upd("up_ct", chain_R(W, t[f"up{u}.in"], 0, W.conv(comp, VW_W, VW_B, 1, d, r * d, d, 1.0)[0], 1))
        upd("pw1", chain_R(W, t[f"up{u}.ln"], 0, W.conv(comp, VW_PW1, VW_PW1_B, 1, d, 4 * d, 4 * d, 1.0)[0], 1))
        upd("pw2", chain_R(W, t[f"up{u}.gelu"], 0, W.conv(comp, VW_PW2, VW_PW2_B, 1, 4 * d, d, d, 1.0)[0], 1))
    ch = W.blocks[0][1]
    upd("dec_in", chain_R(W, t["dec_in.in"], 6, W.conv(VC_DEC_IN, VW_W, VW_B, 7, d, ch, ch, 1.0)[0], 1))
    for b, (r, cin, cout) in enumerate(W.blocks):
        comp = VC_BLK + 4 * b
        upd("blk_ct", chain_R(W, t[f"b{b}.ct_in"], 1, W.conv(comp, VW_W, VW_B, 2, cin, r * cout, cout, 1.0)[0], 1))
        for u in range(3):
            upd("res_c1", chain_R(W, t[f"b{b}.r{u}.c1_in"], 6 * DIL[u], W.conv(comp + 1 + u, VW_W, VW_B, 7, cout, cout, cout, 0.5)[0], DIL[u]))
            upd("res_c2", chain_R(W, t[f"b{b}.r{u}.z"], 0, W.conv(comp + 1 + u, VW_W2, VW_B2, 1, cout, cout, cout, 0.5)[0], 1))
    unit = {k: 0.25 for k in ("up_ct", "dw_ln", "pw1", "pw2", "dec_in", "blk_ct", "res_c1", "res_c2", "out")}   # 4 R = 1: ratio = error / scale
    for stage, ratio, _ in check_call(W, taps, unit):
        if stage.endswith(".dw_ln"):
            upd("dw_ln", ratio)
        elif stage.startswith("out conv"):
            upd("out", ratio)
    return R

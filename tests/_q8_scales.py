"""Shared by tests/test_q8_scales_cpu.py and tests/test_q8_scales_gpu.py: the Q8_0 Talker's GEMM chain at magnitudes away from O(1).

The quantised Talker (q3tts_engine_config.talker_q8_0 = 1 / 2) is otherwise only compared with its own oracle; here both meet a plain
float64 reference and an exact invariance (scaling the rows by 2^e), over the magnitudes where an f16 activation scale is subnormal, zero
or infinite. `python tests/_q8_scales.py` re-measures the ratios committed in tests/_oracle.py (Q8_SCALE_RATIO), CPU only.
"""
import numpy as np

import _gguf as G
import _oracle as O

E_SWEEP = list(range(-24, 25))        # every power of two: both sides of normal/subnormal (e ~ -9), subnormal/zero (~ -20), max/inf (~ +21) of an f16 scale
E_FLAT = list(range(-14, 25))         # where ggml's own order is flat at eps = 1e-6 (checked by the accuracy test: within 2 % of e = 0; below, eps moves it by 1.5 - 2 %)
E_TALKER = [-20, -12, 0, 12, 20]
SHAPES = [(8, 2048, 256), (37, 1024, 96)]   # (rows, K, N): the issue's shape and a ragged one
EW_SWEEP = list(range(-1, 25))        # exponent added to the up half's weight scales (they stay normal f16: d_w ~ 2^-13 .. 2^-10 before)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def bf16_bits(x):
    return G.f32_to_bf16_bits(np.ascontiguousarray(x, dtype=np.float32))


def rel_rms(got, want):
    got = np.asarray(got, dtype=np.float64); want = np.asarray(want, dtype=np.float64)
    return float(np.sqrt(np.mean((got - want) ** 2) / np.mean(want ** 2)))


def scale_f16_bits(d16, e):
    """f16 bit patterns times 2^e, asserting that every non-zero scale was and stays a NORMAL f16 (exact)."""
    f = d16.view(np.float16).astype(np.float32)
    g = (f * np.float32(2.0 ** e)).astype(np.float16)
    nz = f != 0
    assert np.all(np.abs(f[nz]) >= 2.0 ** -14) and np.all(np.abs(g[nz].astype(np.float32)) >= 2.0 ** -14) and np.all(np.isfinite(g))
    assert np.array_equal(g.astype(np.float64), f.astype(np.float64) * 2.0 ** e)
    return np.ascontiguousarray(g).view(np.uint16)


def case(seed, B, K, N):
    """Unit-normal rows x 1.5 with the special channels of the parity tests, a norm weight, a matrix as Q8_0 blocks (+ its bf16 form)."""
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((B, K)) * 1.5).astype(np.float32)
    x[:, :7] *= 300.0; x[:, 100:140] *= 1e-3
    nw = (1.0 + 0.05 * rng.standard_normal(K)).astype(np.float32)
    w = (0.02 * rng.standard_normal((N, K))).astype(np.float32)
    w = G.bf16_bits_to_f32(G.f32_to_bf16_bits(w))
    w[3 % N, 64:96] = 0.0
    q, d16 = O.quantize_q8_0(w)
    return dict(x=x, nw=nw, w=w, wb=bf16_bits(w), q=q, d16=d16)


def dequant_w(q, d16):
    N, K = q.shape
    return (q.astype(np.float64).reshape(N, K // 32, 32) * d16.view(np.float16).astype(np.float64)[:, :, None]).reshape(N, K)


def dequant_a(aq, ad):
    B, K = aq.shape
    return (aq.astype(np.float64).reshape(B, K // 32, 32) * np.asarray(ad, dtype=np.float64)[:, :, None]).reshape(B, K)


def layer0(c, e, eps, mode, gemm=None):
    """RMSNorm -> Linear as the Talker's first GEMM runs it: the producer's operand from x * 2^e, the consumer's row scale from ssp.
    mode 0 bf16, 1 W8A16, 2 W8A8. gemm: dict of the three GEMM callables (default: the oracle's; the GPU tests pass the kernel hooks)."""
    gemm = gemm or dict(bf16=O.bgemm, q8=O.bgemm_q8, q8a8=O.bgemm_q8a8)
    x = (c["x"] * np.float32(2.0 ** e)).astype(np.float32)
    K = x.shape[1]
    xb, ssp = O.norm_inputs(x, c["nw"])
    if mode == 0:
        return gemm["bf16"](xb, c["wb"], ssp, K, eps, 0)["y"]
    if mode == 1:
        return gemm["q8"](xb, c["q"], c["d16"], ssp, K, eps, 0)["y"]
    aq, ad = O.quantize_q8_0_act(x * c["nw"])
    return gemm["q8a8"](aq, ad, c["q"], c["d16"], ssp, K, eps, 0)["y"]


def ggml_quant_rows(v):
    """Rows quantised ggml's way with the rule of tests/_gguf.py (d = amax / 127 as f16, q = roundf(v / d)), de-quantised to float64."""
    v = np.ascontiguousarray(v, dtype=np.float32)
    raw = G.quantize_q8_0(v)
    return G.dequantize_q8_0(raw, v.size).astype(np.float64).reshape(v.shape)


def layer0_f64(c, e, eps):
    """(float64 RMSNorm -> Linear on the de-quantised weights, the same product with the row quantised in ggml's order: the NORMALISED row)."""
    x = c["x"].astype(np.float64) * 2.0 ** e
    wd = dequant_w(c["q"], c["d16"])
    s = 1.0 / np.sqrt((x ** 2).mean(axis=1, keepdims=True) + eps)
    want = (x * s * c["nw"].astype(np.float64)) @ wd.T
    xn = (x * s * c["nw"].astype(np.float64)).astype(np.float32)    # what ggml's RMSNorm hands to the mul_mat
    return want, ggml_quant_rows(xn) @ wd.T


def layer0_errors(c, e, eps, gemm=None):
    want, ref = layer0_f64(c, e, eps)
    return rel_rms(layer0(c, e, eps, 2, gemm), want), rel_rms(ref, want)


# ---- the quantising epilogues -------------------------------------------------------------------------------------------------------
def resid_case(seed, B, K, N):
    rng = np.random.default_rng(seed)
    a = (rng.standard_normal((B, K)) * 1.5).astype(np.float32)
    aq, ad = O.quantize_q8_0_act(a)
    w = (0.02 * rng.standard_normal((N, K))).astype(np.float32)
    q, d16 = O.quantize_q8_0(w)
    y0 = (2.0 * rng.standard_normal((B, N))).astype(np.float32)
    nw = (1.0 + 0.05 * rng.standard_normal(N)).astype(np.float32)
    return dict(aq=aq, ad=ad, q=q, d16=d16, y0=y0, nw=nw)


def resid(c, e, gemm=None):
    """The residual epilogue with the whole sum at 2^e: y0 and (through the activation scales, exactly) RAW."""
    f = (gemm or O.bgemm_q8a8)
    s = np.float32(2.0 ** e)
    return f(c["aq"], c["ad"] * s, c["q"], c["d16"], None, c["aq"].shape[1], 0.0, 1, c["nw"], c["y0"] * s)


def resid_f64(c, e):
    """float64: v = (y0 + RAW) * nw at 2^e from the de-quantised operands."""
    raw = dequant_a(c["aq"], c["ad"]) @ dequant_w(c["q"], c["d16"]).T
    return (c["y0"].astype(np.float64) + raw) * c["nw"].astype(np.float64) * 2.0 ** e


def swiglu_case(seed, B, K, F, small):
    """small: the row scale is 2^-8 (ssp tiles of 16 * 2^16, eps = 0), so h = silu(s g) (s u) sits near 2^-17 before the up half moves."""
    rng = np.random.default_rng(seed)
    a = (rng.standard_normal((B, K)) * 1.5).astype(np.float32)
    aq, ad = O.quantize_q8_0_act(a)
    w = (0.02 * rng.standard_normal((2 * F, K))).astype(np.float32)
    q, d16 = O.quantize_q8_0(w)
    ssp = np.full((B, K // 16), 16.0 * (2.0 ** 16 if small else 1.0), dtype=np.float32)
    return dict(aq=aq, ad=ad, q=q, d16=d16, ssp=ssp, F=F)


def swiglu(c, ew, gemm=None):
    f = (gemm or O.bgemm_q8a8)
    d16 = c["d16"].copy()
    d16[c["F"]:] = scale_f16_bits(c["d16"][c["F"]:], ew)
    return f(c["aq"], c["ad"], c["q"], d16, c["ssp"], c["aq"].shape[1], 0.0, 2)


def swiglu_f64(c, ew):
    F = c["F"]
    raw = dequant_a(c["aq"], c["ad"]) @ dequant_w(c["q"], c["d16"]).T
    s = 1.0 / np.sqrt(c["ssp"].astype(np.float64).sum(axis=1, keepdims=True) / c["aq"].shape[1])
    g = s * raw[:, :F]; u = s * raw[:, F:] * 2.0 ** ew
    return g / (1.0 + np.exp(-g)) * u


def producer_errors(yq, yd, v):
    """(error of the produced blocks against float64 v, error of ggml's quantiser applied to v brought to O(1) by an exact power of two)."""
    got = dequant_a(yq, yd)
    k = 2.0 ** -np.round(np.log2(np.sqrt(np.mean(v ** 2))))
    return rel_rms(got, v), rel_rms(ggml_quant_rows((v * k).astype(np.float32)), v * k)


# ---- a whole Talker ------------------------------------------------------------------------------------------------------------------
def talker_logits(prompt_seed, e, mode):
    """Prefill logits / hidden of the tiny synthetic model in mode 0 bf16 / 1 W8A16 / 2 W8A8 with the prompt rows scaled by 2^e."""
    from q3tts import _abi
    cfg = _abi.tiny_config(max_batch=2, n_ctx=128, with_vocoder=0)
    om = O.OracleModel(cfg.model, seed=0, n_ctx=128, n_threads=4)
    try:
        if mode == 2:
            om.set_talker_q8a8()
        elif mode == 1:
            om.set_talker_q8()
        pe = talker_prompt(om, cfg, prompt_seed) * np.float32(2.0 ** e)
        return om.talker_prefill(pe)
    finally:
        om.close()


def talker_prompt(om, cfg, prompt_seed):
    rng = np.random.default_rng(prompt_seed)
    spk = ((np.arange(cfg.model.d_embed) % 13 - 6) * 0.03125).astype(np.float32)
    desc, keep = O.make_prompt_desc(rng.integers(0, 151643, size=14), spk_emb=spk)
    return om.build_prompt(desc)


def measure():
    """Prints the table committed as tests/_oracle.py Q8_SCALE_RATIO."""
    out = {}
    r = [np.divide(*layer0_errors(case(100 + s, *SHAPES[0]), 0, 1e-6)) for s in range(8)]
    out["gemm"] = (float(np.mean(r)), float(np.std(r, ddof=1)))
    r = []
    for s in range(8):
        c = resid_case(200 + s, 8, 1024, 256); o = resid(c, 0)
        r.append(np.divide(*producer_errors(o["yq"], o["yd"], resid_f64(c, 0))))
    out["resid"] = (float(np.mean(r)), float(np.std(r, ddof=1)))
    r = []
    for s in range(8):
        c = swiglu_case(300 + s, 8, 1024, 256, False); o = swiglu(c, 0)
        r.append(np.divide(*producer_errors(o["yq"], o["yd"], swiglu_f64(c, 0))))
    out["swiglu"] = (float(np.mean(r)), float(np.std(r, ddof=1)))
    for mode in (1, 2):
        r = [rel_rms(talker_logits(400 + s, 0, mode)[1], talker_logits(400 + s, 0, 0)[1]) for s in range(5)]
        out["talker_%d" % mode] = (float(np.mean(r)), float(np.std(r, ddof=1)))
    print("Q8_SCALE_RATIO = {")
    for k, (m, s) in out.items():
        print('    "%s": (%.6g, %.3g),' % (k, m, s))
    print("}")


if __name__ == "__main__":
    measure()

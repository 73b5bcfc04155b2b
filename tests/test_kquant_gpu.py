"""K-quant weights kept quantised on the device (csrc/q3_bgemmk.hip): the GEMM that decodes Q4_K / Q5_K / Q6_K super-blocks
in registers against the bf16 GEMM on the numpy-decoded weights (tests/_gguf.py), bit for bit, and against float64."""
import numpy as np
import pytest

import _gguf as G
from q3tts import native

pytestmark = pytest.mark.gpu

BS = {G.Q4_K: 144, G.Q5_K: 176, G.Q6_K: 210}
MIX = (G.Q5_K, G.Q6_K, G.Q4_K)


def _raw(rng, ty, rows, K):
    """rows x K/256 super-blocks whose every bit field is random; the f16 d / dmin finite, exponents within 2^-8 .. 2^-2, either sign."""
    b = rng.integers(0, 256, size=(rows * (K // 256), BS[ty]), dtype=np.uint8)
    n = b.shape[0]
    f16 = lambda: (np.ldexp(rng.uniform(1.0, 2.0, n), rng.integers(-8, -1, n)) * rng.choice([-1.0, 1.0], n)).astype(np.float16).view(np.uint8).reshape(n, 2)
    if ty == G.Q6_K:
        b[:, 208:210] = f16()
    else:
        b[:, 0:2] = f16(); b[:, 2:4] = f16()
    return b.reshape(-1)


def _weights(rng, segs, K, rep=1):
    """raw bytes of the segments in order, and bf16(dequantize(raw)) as bits [N][K]; rep: a segment is rows / rep random rows, repeated
    (the numpy decoder walks the blocks one by one)"""
    raws, wbs = [], []
    for rows, ty in segs:
        r = _raw(rng, ty, rows // rep, K)
        raws.append(np.tile(r, rep))
        wbs.append(np.tile(G.f32_to_bf16_bits(G.decode(r.tobytes(), ty, rows // rep * K)).reshape(rows // rep, K), (rep, 1)))
    return np.concatenate(raws), np.concatenate(wbs)


def _rows(rng, B, K):
    xb = G.f32_to_bf16_bits(rng.standard_normal((B, K)).astype(np.float32))
    ssp = rng.uniform(0.5, 2.0, size=(B, K // 16)).astype(np.float32)
    return xb, ssp


def _equal(got, ref, epi, with_nw):
    if epi in (0, 1):
        assert np.array_equal(got["y"].view(np.uint32), ref["y"].view(np.uint32))
    if epi == 2 or (epi == 1 and with_nw):
        assert np.array_equal(got["yb"], ref["yb"])
    if epi == 1 and with_nw:
        assert np.array_equal(got["ssp_out"].view(np.uint32), ref["ssp_out"].view(np.uint32))
    if epi == 3:
        assert np.array_equal(got["keys"], ref["keys"])


def _run_both(rng, K, B, segs, epi, rep=1):
    N = sum(r for r, _ in segs)
    raw, wb = _weights(rng, segs, K, rep)
    xb, ssp = _rows(rng, B, K)
    nw = rng.uniform(0.5, 1.5, N).astype(np.float32) if epi == 1 else None
    y0 = rng.standard_normal((B, N)).astype(np.float32) if epi == 1 else None
    sp = None if epi == 1 else ssp   # the engine's RESID launches carry no row scale
    got = native.k_bgemm_kq(xb, raw, segs, sp, K, 1e-6, epi, nw_next=nw, y0=y0)
    ref = native.k_bgemm(xb, wb, sp, K, 1e-6, epi, nw_next=nw, y0=y0)
    _equal(got, ref, epi, nw is not None)


# K: a K slice of a quarter / half / one / three super-blocks (four waves share a d; the ring refills at three). B: one row, a partial
# second row tile, four tiles. One tile row of one type, or one of each type in one matrix. RESID writes its A-tiled norm inputs in
# 32-column blocks, so its cases have two tile rows per type (N = 32, and 96 for the mix); SWIGLU interleaves 8 + 8 columns (N = 64).
def _segs(ty, epi):
    per = 32 if epi == 1 else 16
    if ty == "mix":
        return [(per, t) for t in MIX]
    return [(64 if epi == 2 else per, ty)]


CASES = [
    (512, 1, G.Q4_K, 0), (512, 17, G.Q5_K, 1), (512, 64, G.Q6_K, 3),
    (1024, 64, G.Q4_K, 1), (1024, 1, G.Q5_K, 3), (1024, 17, G.Q6_K, 0),
    (2048, 17, G.Q4_K, 3), (2048, 64, G.Q5_K, 0), (2048, 1, G.Q6_K, 1),
    (6144, 1, G.Q4_K, 0), (6144, 17, G.Q5_K, 1), (6144, 64, G.Q6_K, 0),
    (512, 17, "mix", 0), (1024, 64, "mix", 1), (2048, 1, "mix", 3), (6144, 17, "mix", 0),
    (512, 64, G.Q5_K, 2), (1024, 17, G.Q6_K, 2), (2048, 1, G.Q4_K, 2), (6144, 64, G.Q5_K, 2),
]


@pytest.mark.parametrize("K,B,ty,epi", CASES)
def test_kq_gemm_equals_bf16_gemm_on_decoded_weights(K, B, ty, epi):
    _run_both(np.random.default_rng(K + 7 * B + epi), K, B, _segs(ty, epi), epi)


@pytest.mark.parametrize("K,N,ty,epi", [(2048, 12288, G.Q5_K, 2), (6144, 2048, G.Q6_K, 1)])
def test_kq_gemm_full_shape(K, N, ty, epi):
    """the two launches that carry most of the Talker's bytes: gate/up (SWIGLU) and down (RESID), 64 rows"""
    _run_both(np.random.default_rng(N), K, 64, [(N, ty)], epi, rep=16)


@pytest.mark.parametrize("K", [512, 2048])
@pytest.mark.parametrize("ty", [G.Q4_K, G.Q5_K, G.Q6_K])
def test_kq_gemm_against_float64(K, ty):
    """STORE against s_r * sum_k a_k w_k in float64 over the same bf16 operands, independent of the bf16 kernel. Bound, with S = sum |a_k w_k|,
    from the MFMA's documented arithmetic (profiles/r01/bf16_mfma_arithmetic.md): a step consumes 8 products against
    q = 2^(E - 24), E the largest operand-exponent sum of the step, so q <= 2^-24 max |a_k w_k| of the step; the 8 products and the accumulator
    are truncated to multiples of q (< 9 q, summed over all steps < 9 * 2^-24 S); every step rounds its sum (<= 2^-24 S each, K/8 steps over
    the 8 slices; the cut to 32 leading bits is 2^-31 relative); 7 slice additions and the product with s_r round once each (<= 2^-24 S);
    s_r itself is f32 arithmetic over K/16 positive partials (at most K/32 + 3 half-ulps relative after the square root). Together
    |y - s_r RAW| <= (K/8 + K/32 + 21) * 2^-24 * s_r * S — tighter than K * 2^-23 * s_r * S, which holds for any order of truncating f32
    additions of exact products."""
    rng = np.random.default_rng(K + ty)
    B, N = 17, 16
    raw, wb = _weights(rng, [(N, ty)], K)
    xb, ssp = _rows(rng, B, K)
    got = native.k_bgemm_kq(xb, raw, [(N, ty)], ssp, K, 1e-6, 0)["y"].astype(np.float64)
    a = G.bf16_bits_to_f32(xb).astype(np.float64); w = G.bf16_bits_to_f32(wb).astype(np.float64)
    s = 1.0 / np.sqrt(ssp.astype(np.float64).sum(axis=1) / K + 1e-6)
    ref = s[:, None] * (a @ w.T)
    bound = (K / 8 + K / 32 + 21) * 2.0 ** -24 * s[:, None] * (np.abs(a) @ np.abs(w).T)
    err = np.abs(got - ref)
    print("max err / bound:", float((err / bound).max()))
    assert (err <= bound).all()


def _recipe(name, up=G.Q5_K):
    """llama.cpp's Q5_K_M choice per matrix: attn_v and output.weight Q6_K, ffn_down Q6_K in block 0, everything else Q5_K"""
    if "attn_v" in name or name == "output.weight" or name == "blk.0.ffn_down.weight":
        return G.Q6_K
    return up if "ffn_up" in name else G.Q5_K


def _write_dir(oracle, path, m, up):
    """the synthetic model as a quant directory typed per tensor; -> {ggml type: tiled bytes}, bf16 bytes, bytes saved against bf16"""
    oracle.write_model_dir(str(path), m, 0, matrix_type=G.F32)
    held, bf16, saved = {G.Q4_K: 0, G.Q5_K: 0, G.Q6_K: 0}, 0, 0
    for talker, fname in ((True, "qwen3_tts_talker.gguf"), (False, "qwen3_tts_predictor.gguf")):
        tens = oracle.synth_transformer_tensors(m, 0, talker)
        G.write(str(path / fname), [(k, v, _recipe(k, up) if v.ndim == 2 else G.F32) for k, v in tens.items()],
                meta={"general.architecture": "qwen3", "general.alignment": 32})
        for k, v in tens.items():
            if v.ndim != 2:
                continue
            N, K = v.shape
            if up != G.Q5_K and ("ffn_up" in k or "ffn_gate" in k):   # gate and up differ in type: their matrix stays bf16
                bf16 += 2 * N * K
                continue
            b = native.k_kq_bytes(_recipe(k, up), N, K)
            held[_recipe(k, up)] += b; saved += 2 * N * K - b
    return held, bf16, saved


def test_engine_kquant_resident(oracle, tmp_path):
    """An engine that keeps the K-quant tensors of a Q5_K_M-typed directory quantised against the default engine on the same files: prompt
    rows, greedy and sampled ids ==; the matrices reported under their own types; device bytes smaller by exactly the matrices' saving; a
    gate / up pair of two types falls back to bf16; the option is refused together with talker_q8_0."""
    from q3tts import _abi
    cfg = _abi.tiny_config(max_batch=2, n_ctx=128, with_vocoder=0)
    held, bf16, saved = _write_dir(oracle, tmp_path / "q5km", cfg.model, G.Q5_K)
    held2, bf16_2, saved2 = _write_dir(oracle, tmp_path / "mixed_ffn", cfg.model, G.Q6_K)

    def engine(d, **kw):
        c = _abi.tiny_config(max_batch=2, n_ctx=128, with_vocoder=0)
        c.weights_path = str(tmp_path / d).encode()
        for k, v in kw.pop("cfg", {}).items():
            setattr(c, k, v)
        return native.NativeEngine(c, **kw)

    engs = [engine("q5km", kquant_resident=True), engine("q5km"), engine("mixed_ffn", kquant_resident=True), engine("mixed_ffn")]
    try:
        res, plain, res2, plain2 = engs
        desc, keep = oracle.make_prompt_desc(np.arange(900, 912), spk_emb=((np.arange(cfg.model.d_embed) % 13 - 6) * 0.03125).astype(np.float32))
        assert np.array_equal(res.build_prompt(desc).view(np.uint32), plain.build_prompt(desc).view(np.uint32))
        for kw in (dict(temperature=0.0, max_steps=6), dict(temperature=0.7, top_k=40, top_p=0.9, seed=11, max_steps=6)):
            a, b = res.generate(desc=desc, **kw), plain.generate(desc=desc, **kw)
            assert a.codes.shape[0] > 0 and np.array_equal(a.codes, b.codes)
            a, b = res2.generate(desc=desc, **kw), plain2.generate(desc=desc, **kw)
            assert a.codes.shape[0] > 0 and np.array_equal(a.codes, b.codes)
        assert res.weight_formats == {"bf16": 0, "q4_k": 0, "q5_k": held[G.Q5_K], "q6_k": held[G.Q6_K]}
        assert res2.weight_formats == {"bf16": bf16_2, "q4_k": 0, "q5_k": held2[G.Q5_K], "q6_k": held2[G.Q6_K]}
        assert plain.weight_formats["q5_k"] == 0 and plain.weight_formats["q6_k"] == 0 and plain.weight_formats["bf16"] == held[G.Q5_K] + held[G.Q6_K] + saved
        assert res.device_bytes() == plain.device_bytes() - saved and res2.device_bytes() == plain2.device_bytes() - saved2
    finally:
        for e in engs:
            e.close()
    with pytest.raises(_abi.Q3Error, match="kquant_resident.*talker_q8_0"):
        engine("q5km", kquant_resident=True, cfg=dict(talker_q8_0=1))

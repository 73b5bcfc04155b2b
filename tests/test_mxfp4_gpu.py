"""The Talker's GEMM on MXFP4 weights (q3tts_engine_options.talker_mxfp4; csrc/q3_bgemm4.hip)."""
import numpy as np
import pytest

import _gguf as G
import _mxfp4 as M
from q3tts import _abi, native

pytestmark = pytest.mark.gpu
U = 2.0 ** -24


@pytest.mark.parametrize("case", ["block_scales", "row_col_values"])
@pytest.mark.parametrize("B,K,N", [(16, 128, 16), (33, 1152, 48)])
def test_operand_map_on_an_exact_grid(case, B, K, N):
    """Weights +-{0.5, 1, 2} * 2^s, rows of small integers (exact in E4M3): every partial sum is exact in f32, so the output equals the integer
    product whatever the hardware's order; a swapped lane, nibble or scale does not. block_scales: every 32-block of every column has its own
    scale; row_col_values: every row and column of a tile carries a value of its own."""
    rng, mag = np.random.default_rng(B + K), np.array([1, 2, 4], dtype=np.uint8)   # mag: the E2M1 codes of 0.5, 1, 2
    codes = mag[rng.integers(0, 3, size=(N, K))] | (rng.integers(0, 2, size=(N, K)).astype(np.uint8) << 3)
    x = rng.integers(-7, 8, size=(B, K)).astype(np.float32)
    if case == "block_scales":      # (products are multiples of 2^-4 and sums stay below 2^18: exact in f32 in any order)
        e = (125 + (np.arange(N)[:, None] * 5 + np.arange(K // 32)[None, :] * 3) % 6).astype(np.uint8)
        x *= np.repeat(np.exp2((np.arange(B)[:, None] + np.arange(K // 32)[None, :]) % 3 - 1), 32, axis=1).astype(np.float32)
    else:
        e = np.broadcast_to((125 + np.arange(N) % 6).astype(np.uint8)[:, None], (N, K // 32))
        codes = np.broadcast_to(mag[np.arange(N) % 3][:, None], (N, K)) | ((np.arange(N)[:, None] + np.arange(K)[None, :]) % 2 << 3).astype(np.uint8)
        x = np.broadcast_to((np.arange(B) % 14 + 1)[:, None], (B, K)).astype(np.float32) * np.where(np.arange(K) % 3 == 0, -1.0, 1.0).astype(np.float32)
    blocks = M.pack_mxfp4(codes, e)
    got = native.k_bgemm_mxfp4(G.f32_to_bf16_bits(x), blocks, None, K, 1e-6, 0, rows_out=True)
    assert np.array_equal(got["blocks"], blocks)
    assert np.array_equal(M.dequant_fp8_rows(got["a8"], got["ae"]), x.astype(np.float64)), "the rows are exact in MXFP8"
    assert np.array_equal(got["y"].astype(np.float64), x.astype(np.float64) @ M.dequant_mxfp4(blocks).T)


def test_quantisers_bit_for_bit():
    """Random data plus a zero block, a block whose amax is a power of two, rounding midpoints of both grids and values that saturate."""
    rng = np.random.default_rng(3)
    B, K, N = 17, 256, 32
    w = (rng.standard_normal((N, K)) * 0.02).astype(np.float32)
    w[0, :32] = 0.0; w[1, 32:64] = np.where(np.arange(32) == 5, 0.25, w[1, 32:64] * 0.1); w[2, :32] = np.linspace(-0.05, 0.05, 32)
    w[3, :16] = np.array([0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5, 7, -0.25, -0.75, -1.25, -1.75, -2.5, -3.5, -5, -7]) * 2.0 ** -7  # midpoints of the E2M1 grid
    x = rng.standard_normal((B, K)).astype(np.float32)
    w[3, 16], x[0, :32] = 6 * 2.0 ** -7, 0.0
    x[1, :32] = np.where(np.arange(32) == 0, 256.0, np.array([17, 19, 21, 23, 25, 27, 29, 31] * 4))   # amax 2^8: E = 127; odd integers 17 .. 31 are midpoints of the step-2 binade
    x[2, :32] = np.where(np.arange(32) == 0, 256.0, np.arange(32) * 0.0 + 0.001953125 * 1.5)          # a subnormal midpoint (1.5 * 2^-9)
    x[3, :32] = 3.0; x[3, :4] = [448.0, 464.0, 480.0, -510.0]                                            # 448 kept, 464 -> 448 (tie to even), 480 and -510 saturate
    xb = G.f32_to_bf16_bits(x)
    got = native.k_bgemm_mxfp4(xb, w, None, K, 1e-6, 0, rows_out=True)
    assert np.array_equal(got["blocks"], M.quantize_row_mxfp4(w))
    q, E = M.mx_fp8_rows(xb)
    assert np.array_equal(got["ae"], E) and np.array_equal(got["a8"], q)


def _reference(xb, w, ssp=None, d_norm=1, eps=1e-6):
    """float64 RAW of the dequantised operands and the bound gamma_K * sum |a w| per output, both scaled by the row scale."""
    a = M.dequant_fp8_rows(*M.mx_fp8_rows(xb)); wd = M.dequant_mxfp4(M.quantize_row_mxfp4(w))
    K = a.shape[1]
    raw, S = a @ wd.T, np.abs(a) @ np.abs(wd).T
    bound = K * U / (1 - K * U) * S
    if ssp is not None:      # s_r = 1 / sqrtf(sum / d_norm + eps): a handful of f32 roundings on the scale, one on the product
        sc = (1.0 / np.sqrt(ssp.astype(np.float64).sum(axis=1) / d_norm + eps))[:, None]
        raw, bound = raw * sc, bound * sc + 8 * U * np.abs(raw * sc)
    return raw, bound


@pytest.mark.parametrize("B,K,N", [(1, 128, 16), (15, 256, 48), (16, 1024, 16), (17, 1152, 48), (33, 512, 1024), (65, 512, 512), (65, 1024, 512), (200, 512, 2048)])
def test_gemm_against_float64(B, K, N):
    """The four block GEMMs' epilogues against the float64 product of the dequantised operands: |err| <= gamma_K * sum |a w| (gamma_K = K u /
    (1 - K u), u = 2^-24), times the row scale where there is one, plus the epilogue's own roundings: the residual add (u |y|), SwiGLU in f32
    (16 u) and its bf16 output (2^-8: half a unit of an 8-bit significand)."""
    rng = np.random.default_rng(B * 7 + K + N)
    w = (rng.standard_normal((N, K)) * 0.01).astype(np.float32)      # (gate values stay inside q3_expf's domain, |g| < 87: checked below)
    xb = G.f32_to_bf16_bits(rng.standard_normal((B, K)) * np.exp2(rng.integers(-3, 4, size=(B, 1))))
    ssp = rng.uniform(0.5, 2.0, size=(B, K // 16)).astype(np.float32)
    y0 = rng.standard_normal((B, N)).astype(np.float32)
    nw = rng.uniform(0.5, 1.5, size=N).astype(np.float32)
    # QKV: STORE with row scales
    raw, bound = _reference(xb, w, ssp, K, 1e-6)
    got = native.k_bgemm_mxfp4(xb, w, ssp, K, 1e-6, 0)
    assert (np.abs(got["y"] - raw) <= bound).all(), ("store", np.max(np.abs(got["y"] - raw) / np.maximum(bound, 1e-300)))
    # O / down: RESID, with and without the next norm's inputs (computed from the kernel's own y: their roundings alone)
    raw, bound = _reference(xb, w)
    for nwn in (nw, None) if N % 32 == 0 else (None,):
        r = native.k_bgemm_mxfp4(xb, w, None, K, 1e-6, 1, nw_next=nwn, y0=y0)
        assert (np.abs(r["y"] - (y0 + raw)) <= bound + U * np.abs(y0 + raw) * 1.0001).all(), "resid"
        if nwn is not None:
            assert np.array_equal(r["yb"], G.f32_to_bf16_bits(r["y"] * nwn[None, :]))
            sq = (r["y"].astype(np.float64) ** 2).reshape(B, N // 16, 16).sum(axis=2)
            assert (np.abs(r["ssp_out"] - sq) <= 17 * U * sq).all()
    # gate / up: SWIGLU with row scales (w: the N/2 gate rows, then the N/2 up rows)
    if N % 64 == 0:
        raw, bound = _reference(xb, w, ssp, K, 1e-6)
        g, u, eg, eu = raw[:, :N // 2], raw[:, N // 2:], bound[:, :N // 2], bound[:, N // 2:]
        assert np.abs(g).max() < 80.0
        silu = g / (1 + np.exp(-g))
        tol = 1.1 * eg * (np.abs(u) + eu) + np.abs(silu) * eu + (16 * U + 2.0 ** -8) * np.abs(silu * u) + 1e-37
        r = native.k_bgemm_mxfp4(xb, w, ssp, K, 1e-6, 2)
        out = (r["yb"].astype(np.uint32) << 16).view(np.float32)
        assert (np.abs(out - silu * u) <= tol).all(), ("swiglu", float(np.max(np.abs(out - silu * u) / tol)))


def test_a_row_has_the_same_bits_at_every_row_count_and_instance():
    lib = _abi.load_library()
    rng, K, N = np.random.default_rng(11), 1152, 48
    w = (rng.standard_normal((N, K)) * 0.05).astype(np.float32)
    xb = G.f32_to_bf16_bits(rng.standard_normal((65, K)))
    want = native.k_bgemm_mxfp4(xb, w, None, K, 1e-6, 0)["y"]
    try:
        for rt, nt, B in [(0, 0, 1), (0, 0, 17), (1, 1, 65), (2, 3, 33), (3, 1, 65), (4, 3, 65), (4, 1, 64)]:
            lib.q3tts_k_bgemm_force(rt, nt)
            assert np.array_equal(native.k_bgemm_mxfp4(xb[:B], w, None, K, 1e-6, 0)["y"].view(np.uint32), want[:B].view(np.uint32)), (rt, nt, B)
    finally:
        lib.q3tts_k_bgemm_force(0, 0)


def _engine(max_batch=1, path=None, q8=0, **kw):
    cfg = _abi.tiny_config(max_batch=max_batch, n_ctx=256)
    cfg.weights_path, cfg.talker_q8_0 = path, q8
    return native.NativeEngine(cfg, **kw)


@pytest.mark.parametrize("other", ["three_slots", "session"])
def test_engine_ids_do_not_depend_on_slots_or_sessions(other):
    rng = np.random.default_rng(5)
    one, three = _engine(1, talker_mxfp4=True), _engine(3, talker_mxfp4=True)
    reqs = [dict(embd=(rng.standard_normal((20 + 3 * i, one.cfg.model.d_embed)) * 0.05).astype(np.float32), temperature=0.7, top_k=40, top_p=0.9,
                 seed=7 + i, max_steps=12, min_frames=8, force_eos_at=8 + i, want_pcm=1) for i in range(4)]
    try:
        want = one.generate_batch(reqs)
        assert all(w.status == 0 and w.codes.shape[0] == r["force_eos_at"] for w, r in zip(want, reqs))
        if other == "three_slots":
            got = [(g.codes, g.pcm) for g in three.generate_batch(reqs)]
        else:
            s = native.NativeSession(three)
            try:
                ids = [s.submit(**r) for r in reqs]
                ev = list(s.events(timeout_ms=60000))
            finally:
                s.close()
            got = [([e[4] for e in ev if e[0] == rid and e[1] != _abi.EV_CHUNK][0].codes,
                    np.concatenate([e[2] for e in ev if e[0] == rid and e[1] == _abi.EV_CHUNK])) for rid in ids]
        for (codes, pcm), w in zip(got, want):
            assert np.array_equal(codes, w.codes) and np.array_equal(pcm.view(np.uint32), w.pcm.view(np.uint32))
    finally:
        one.close(); three.close()


def test_engine_formats_bytes_refusals_and_the_default():
    plain, off, on = _engine(), _engine(kquant_resident=True), _engine(talker_mxfp4=True)   # off: the options struct with talker_mxfp4 = 0 (synthetic weights have no K-quants)
    m = plain.cfg.model
    nq, nqkv = m.t_n_head * m.t_head_dim, (m.t_n_head + 2 * m.t_n_kv_head) * m.t_head_dim
    n = m.t_n_layer * (nqkv * m.t_d_model + m.t_d_model * nq + 3 * m.t_d_model * m.t_d_ffn)     # every block matrix has K % 128 == 0 here
    req = [dict(embd=(np.random.default_rng(9).standard_normal((24, m.d_embed)) * 0.05).astype(np.float32), max_steps=10, min_frames=6, force_eos_at=6)]
    try:
        assert on.weight_formats["mxfp4"] == n // 32 * 17 and "mxfp4" not in plain.weight_formats
        assert plain.weight_formats["bf16"] - on.weight_formats["bf16"] == 2 * n and plain.device_bytes() - on.device_bytes() == 2 * n - n // 32 * 17
        assert np.array_equal(off.generate_batch(req)[0].codes, plain.generate_batch(req)[0].codes)
    finally:
        for e in (plain, off, on):
            e.close()
    for kw, what in ((dict(q8=2), "talker_q8_0 = 2"), (dict(kquant_resident=True), "kquant_resident = 1")):
        with pytest.raises(_abi.Q3Error, match="talker_mxfp4 = 1.*" + what):
            _engine(talker_mxfp4=True, **kw)


def test_a_type_39_file_loads_its_blocks_as_stored(oracle, tmp_path, monkeypatch):
    """Block matrices as GGUF type 39 against f32 tensors of the blocks' values, which re-quantise to exactly those blocks (checked): equal ids."""
    enc = G.encode
    monkeypatch.setattr(G, "encode", lambda a, ty: M.quantize_row_mxfp4(a).tobytes() if ty == 39 else enc(a, ty))
    m = _abi.tiny_config().model
    tens = oracle.synth_transformer_tensors(m, 0, True)
    blk = {k: M.quantize_row_mxfp4(v) for k, v in tens.items() if v.ndim == 2 and k.startswith("blk.")}
    vals = {k: M.dequant_mxfp4(b).astype(np.float32) for k, b in blk.items()}
    assert all(np.array_equal(M.quantize_row_mxfp4(vals[k]), blk[k]) for k in blk)
    engs = []
    for d, ty in (("mx", 39), ("f32", G.F32)):
        oracle.write_model_dir(str(tmp_path / d), m, 0, matrix_type=G.F32)
        G.write(str(tmp_path / d / "qwen3_tts_talker.gguf"), [(k, vals.get(k, v), ty if k in blk else G.F32) for k, v in tens.items()],
                meta={"general.architecture": "qwen3", "general.alignment": 32})
        engs.append(_engine(path=str(tmp_path / d).encode(), talker_mxfp4=True))
    try:
        desc, _ = oracle.make_prompt_desc(np.arange(900, 912), spk_emb=((np.arange(m.d_embed) % 13 - 6) * 0.03125).astype(np.float32))
        a, b = (e.generate(desc=desc, temperature=0.7, top_k=40, top_p=0.9, seed=11, max_steps=6) for e in engs)
        assert a.codes.shape[0] > 0 and np.array_equal(a.codes, b.codes) and engs[0].weight_formats == engs[1].weight_formats
    finally:
        for e in engs:
            e.close()

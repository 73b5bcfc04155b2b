"""The Talker's GEMM on MXFP8 weights, FP8 x FP8 (q3tts_engine_options.talker_mxfp8; k_bgemm_mx8 in csrc/q3_bgemm4.hip).
The reference quantiser of both operands is tests/_mxfp4.py::mx_fp8_rows on bf16 bits. (No accepted engine config has a block matrix whose K
is not a multiple of 512, so "such a matrix stays bf16" cannot be reached through an engine; the shapes below are what exists.)"""
import ctypes as C

import numpy as np
import pytest

import _gguf as G
import _mxfp4 as M
from q3tts import _abi, native

pytestmark = pytest.mark.gpu
U = 2.0 ** -24


def _wq(w):
    return M.mx_fp8_rows(G.f32_to_bf16_bits(w))


@pytest.mark.parametrize("case", ["block_scales", "row_col_values"])
@pytest.mark.parametrize("B,K,N", [(16, 128, 16), (33, 1152, 48)])
def test_operand_map_on_an_exact_grid(case, B, K, N):
    """Weights +-{1, 1.25, 1.5, 1.75} * {1, 2} * 2^s (four-bit significands, a block's largest below 1.875 * 2^n: exact in E4M3 under the
    block's own scale), rows of small integers: products are multiples of 2^(s0 - 3) and sums stay below 2^(s0 + 19), so every partial sum is
    exact in f32 and the output equals the float64 product whatever the hardware's order; a swapped lane, half, byte or scale does not.
    block_scales: every 32-block of a 128-step has its own scale on both sides; row_col_values: every row and column of a tile its own value."""
    rng, man = np.random.default_rng(B + K), np.array([1, 1.25, 1.5, 1.75])
    n, k, b = np.arange(N)[:, None], np.arange(K)[None, :], np.arange(B)[:, None]
    if case == "block_scales":
        w = man[rng.integers(0, 4, size=(N, K))] * rng.integers(1, 3, size=(N, K)) * rng.choice([-1.0, 1.0], size=(N, K)) * np.exp2((n * 5 + k // 32 * 3) % 4 - 10)
        x = rng.integers(-7, 8, size=(B, K)) * np.exp2((b + k // 32) % 3 - 1)
    else:
        w = man[n % 4] * (1 + n % 2) * np.where((n + k) % 2, -1.0, 1.0) * np.exp2(n % 4 - 10)
        x = (b % 14 + 1) * np.where(k % 3 == 0, -1.0, 1.0)
    w, x = w.astype(np.float32), x.astype(np.float32)
    got = native.k_bgemm_mxfp8(G.f32_to_bf16_bits(x), w, None, K, 1e-6, 0, rows_out=True)
    assert np.array_equal(M.dequant_fp8_rows(got["q"], got["e"]), w.astype(np.float64)), "the weights are exact in MXFP8"
    assert np.array_equal(M.dequant_fp8_rows(got["a8"], got["ae"]), x.astype(np.float64)), "the rows are exact in MXFP8"
    assert np.array_equal(got["y"].astype(np.float64), x.astype(np.float64) @ w.astype(np.float64).T)


@pytest.mark.parametrize("epi", [0, 2])
def test_quantisers_bit_for_bit(epi):
    """Random data plus a zero block, a block whose amax is a power of two, E4M3 midpoints (normal and subnormal) and values at and past 448
    scale units, on both operands; epi 2 also runs the gate / up interleave of the load kernel."""
    rng = np.random.default_rng(3)
    B, K, N = 17, 256, 64
    sp = np.zeros((4, 32))
    sp[1] = np.where(np.arange(32) == 5, 256.0, rng.standard_normal(32) * 20)       # amax 2^8 exactly
    sp[2] = np.where(np.arange(32) == 0, 256.0, np.array([17, 19, 21, 23, 25, 27, 29, 31] * 4))   # odd integers 17 .. 31: midpoints of the step-2 binade
    sp[2, 16:] = 0.001953125 * 1.5                                                                 # a subnormal midpoint (1.5 * 2^-9)
    sp[3] = 3.0; sp[3, :4] = [448.0, 464.0, 480.0, -510.0]                                          # 448 kept, 464 -> 448 (tie to even), 480 and -510 saturate
    w = (rng.standard_normal((N, K)) * 0.02).astype(np.float32)
    x = rng.standard_normal((B, K)).astype(np.float32)
    for i in range(4):   # (weights in units of 2^-12, in a gate and an up row; rows in units of 1)
        w[i, 32 * i:32 * i + 32] = w[40 + i, 64:96] = sp[i] * 2.0 ** -12
        x[i, :32] = sp[i]
    xb = G.f32_to_bf16_bits(x)
    got = native.k_bgemm_mxfp8(xb, w, None, K, 1e-6, epi, rows_out=True)
    q, e = _wq(w)
    assert np.array_equal(got["e"], e) and np.array_equal(got["q"], q)
    q, e = M.mx_fp8_rows(xb)
    assert np.array_equal(got["ae"], e) and np.array_equal(got["a8"], q)


def _reference(xb, w, ssp=None, d_norm=1, eps=1e-6):
    """float64 RAW of the dequantised operands and the bound gamma_K * sum |a w| per output, both scaled by the row scale."""
    a, wd = M.dequant_fp8_rows(*M.mx_fp8_rows(xb)), M.dequant_fp8_rows(*_wq(w))
    K = a.shape[1]
    raw, bound = a @ wd.T, K * U / (1 - K * U) * (np.abs(a) @ np.abs(wd).T)
    if ssp is not None:      # s_r = 1 / sqrtf(sum / d_norm + eps): a handful of f32 roundings on the scale, one on the product
        sc = (1.0 / np.sqrt(ssp.astype(np.float64).sum(axis=1) / d_norm + eps))[:, None]
        raw, bound = raw * sc, bound * sc + 8 * U * np.abs(raw * sc)
    return raw, bound


@pytest.mark.parametrize("B,K,N", [(1, 128, 16), (15, 256, 48), (17, 1152, 48), (33, 512, 1024), (65, 1024, 512)])
def test_gemm_against_float64(B, K, N):
    """The four block GEMMs' epilogues against the float64 product of the dequantised operands: |err| <= gamma_K * sum |a w| (gamma_K = K u /
    (1 - K u), u = 2^-24), times the row scale where there is one, plus the epilogue's own roundings: the residual add (u |y|), SwiGLU in f32
    (16 u) and its bf16 output (2^-8: half a unit of an 8-bit significand)."""
    rng = np.random.default_rng(B * 7 + K + N)
    w = (rng.standard_normal((N, K)) * 0.01).astype(np.float32)      # (gate values stay inside q3_expf's domain: checked below)
    xb = G.f32_to_bf16_bits(rng.standard_normal((B, K)) * np.exp2(rng.integers(-3, 4, size=(B, 1))))
    ssp = rng.uniform(0.5, 2.0, size=(B, K // 16)).astype(np.float32)
    y0 = rng.standard_normal((B, N)).astype(np.float32)
    nw = rng.uniform(0.5, 1.5, size=N).astype(np.float32)
    raw, bound = _reference(xb, w, ssp, K, 1e-6)     # QKV: STORE with row scales
    got = native.k_bgemm_mxfp8(xb, w, ssp, K, 1e-6, 0)
    assert (np.abs(got["y"] - raw) <= bound).all(), ("store", np.max(np.abs(got["y"] - raw) / np.maximum(bound, 1e-300)))
    if N % 64 == 0:                                  # gate / up: SWIGLU with row scales (w: the N/2 gate rows, then the N/2 up rows)
        g, u, eg, eu = raw[:, :N // 2], raw[:, N // 2:], bound[:, :N // 2], bound[:, N // 2:]
        assert np.abs(g).max() < 80.0
        silu = g / (1 + np.exp(-g))
        tol = 1.1 * eg * (np.abs(u) + eu) + np.abs(silu) * eu + (16 * U + 2.0 ** -8) * np.abs(silu * u) + 1e-37
        out = (native.k_bgemm_mxfp8(xb, w, ssp, K, 1e-6, 2)["yb"].astype(np.uint32) << 16).view(np.float32)
        assert (np.abs(out - silu * u) <= tol).all(), ("swiglu", float(np.max(np.abs(out - silu * u) / tol)))
    raw, bound = _reference(xb, w)                   # O / down: RESID, with and without the next norm's inputs (from the kernel's own y)
    for nwn in (nw, None) if N % 32 == 0 else (None,):
        r = native.k_bgemm_mxfp8(xb, w, None, K, 1e-6, 1, nw_next=nwn, y0=y0)
        assert (np.abs(r["y"] - (y0 + raw)) <= bound + U * np.abs(y0 + raw) * 1.0001).all(), "resid"
        if nwn is not None:
            assert np.array_equal(r["yb"], G.f32_to_bf16_bits(r["y"] * nwn[None, :]))
            sq = (r["y"].astype(np.float64) ** 2).reshape(B, N // 16, 16).sum(axis=2)
            assert (np.abs(r["ssp_out"] - sq) <= 17 * U * sq).all()


def test_a_row_has_the_same_bits_at_every_row_count_and_instance():
    lib = _abi.load_library()
    rng, K, N = np.random.default_rng(11), 1152, 48
    w = (rng.standard_normal((N, K)) * 0.05).astype(np.float32)
    xb = G.f32_to_bf16_bits(rng.standard_normal((65, K)))
    want = native.k_bgemm_mxfp8(xb, w, None, K, 1e-6, 0)["y"]
    try:
        for rt, nt, B in [(0, 0, 1), (0, 0, 17), (1, 1, 65), (2, 3, 33), (3, 1, 65), (4, 3, 65), (4, 1, 64)]:
            lib.q3tts_k_bgemm_force(rt, nt)
            assert np.array_equal(native.k_bgemm_mxfp8(xb[:B], w, None, K, 1e-6, 0)["y"].view(np.uint32), want[:B].view(np.uint32)), (rt, nt, B)
    finally:
        lib.q3tts_k_bgemm_force(0, 0)


def _engine(max_batch=1, q8=0, **kw):
    cfg = _abi.tiny_config(max_batch=max_batch, n_ctx=256)
    cfg.talker_q8_0 = q8
    return native.NativeEngine(cfg, **kw)


def _requests(d_embed):
    rng = np.random.default_rng(5)
    return [dict(embd=(rng.standard_normal((20 + 3 * i, d_embed)) * 0.05).astype(np.float32), temperature=0.7, top_k=40, top_p=0.9,
                 seed=7 + i, max_steps=12, min_frames=8, force_eos_at=8 + i, want_pcm=1) for i in range(4)]


@pytest.mark.parametrize("other", ["three_slots", "session"])
def test_engine_ids_do_not_depend_on_slots_or_sessions(other):
    one, three = _engine(1, talker_mxfp8=True), _engine(3, talker_mxfp8=True)
    reqs = _requests(one.cfg.model.d_embed)
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


def _with_options(struct_size, mx8):
    """An engine from a raw options struct: the current layout, or the caller's that ends behind talker_mxfp4."""
    lib, cfg, h = _abi.load_library(), _abi.tiny_config(max_batch=1, n_ctx=256), C.c_void_p()
    opts = _abi.EngineOptions(struct_size, 0, 0, 0, 0, 0, mx8)
    assert lib.q3tts_engine_create_opts(C.byref(cfg), C.byref(opts), C.byref(h)) == 0, lib.q3tts_last_error(None).decode()
    eng = native.NativeEngine.__new__(native.NativeEngine)
    eng.lib, eng.cfg, eng.h, eng._prefixes = lib, cfg, h, set()
    return eng


def test_engine_formats_bytes_refusals_and_the_default():
    plain, on, mx4 = _engine(), _engine(talker_mxfp8=True), _engine(talker_mxfp4=True)
    off, short = _with_options(C.sizeof(_abi.EngineOptions), 0), _with_options(_abi.EngineOptions.talker_mxfp8.offset, 1)   # (short: the field is not read)
    m = plain.cfg.model
    nq, nqkv = m.t_n_head * m.t_head_dim, (m.t_n_head + 2 * m.t_n_kv_head) * m.t_head_dim
    n = m.t_n_layer * (nqkv * m.t_d_model + m.t_d_model * nq + 3 * m.t_d_model * m.t_d_ffn)     # every block matrix has K % 128 == 0 here
    req = _requests(m.d_embed)[:1]
    try:
        assert on.weight_formats["mxfp8"] == n // 32 * 33 and "mxfp4" not in on.weight_formats
        assert "mxfp8" not in plain.weight_formats and "mxfp8" not in mx4.weight_formats
        assert plain.weight_formats["bf16"] - on.weight_formats["bf16"] == 2 * n and plain.device_bytes() - on.device_bytes() == 2 * n - n // 32 * 33
        ids = {k: e.generate_batch(req)[0].codes for k, e in dict(plain=plain, on=on, mx4=mx4, off=off, short=short).items()}
        assert np.array_equal(ids["off"], ids["plain"]) and np.array_equal(ids["short"], ids["plain"])
        assert not np.array_equal(ids["on"], ids["plain"]) and not np.array_equal(ids["on"], ids["mx4"])
    finally:
        for e in (plain, on, mx4, off, short):
            e.close()
    for kw, what in ((dict(talker_mxfp4=True), "talker_mxfp4 = 1"), (dict(q8=2), "talker_q8_0 = 2"), (dict(kquant_resident=True), "kquant_resident = 1")):
        with pytest.raises(_abi.Q3Error, match="talker_mxfp8 = 1.*" + what):
            _engine(talker_mxfp8=True, **kw)

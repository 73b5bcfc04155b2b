"""Long utterances on the device against the CPU oracle: the vocoder far past its sliding window, decode attention up to n_ctx.

The rest of the suite stops at 12 vocoder frames and ~620 decode keys; the product runs 25-250 frames per utterance (bench.py) and a
default n_ctx of 4096 (8192 at most). Here:
  * the full-shape vocoder over 160 frames (window 72, ring of 76 rows, RoPE table of max_steps_cap + 4 rows): the transformer's rows
    frame by frame, the PCM over the whole signal and per 4-frame chunk, and every launch variant bit for bit;
  * 64 slots x 72 requests of 25-160 frames with the vocoder on: every utterance's PCM equals the one-slot vocoder on its codes;
  * decode attention (the fused kernels k_attend_gqa2, k_attend<2, true>, k_attend<4, true>) at 4096 and 8192 keys: bit for bit
    against the oracle and within a stated bound of a float64 reference, on inputs that stress the softmax;
  * a tiny engine with n_ctx = 8192 and prompts of ~1000 and ~4000 rows: greedy ids equal the oracle's under both decode kernels.
"""
import ctypes as C
import os
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

PCM_RMS_TOL_FULL = 3.5e-3   # tests/test_parity_gpu.py: the full-shape PCM bound (bf16 operands vs both oracles)
# Per frame, RMS(device - oracle) / RMS(oracle) of the transformer's output row after the final norm (bf16-input oracle stage 2): the
# bounds and their measured values are in tests/_oracle.py (the CPU test shows a window off by one moves the oracle's rows by >= 10x).
from _oracle import VOC_LATENT_TOL, VOC_LATENT_TOL_EARLY  # noqa: E402
ATT_F64_TOL = 2e-5          # decode attention vs float64, relative to max |V| of the (slot, KV head); measured: see the print


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _bf16_bits(a):
    u = np.ascontiguousarray(a, dtype=np.float32).view(np.uint32).astype(np.uint64)
    u = u + 0x7FFF + ((u >> 16) & 1)
    return (u >> 16).astype(np.uint16)


def _bf16(a):
    return (_bf16_bits(a).astype(np.uint32) << 16).view(np.float32)


def _voc_lib(O):
    L = O.lib()
    L.q3o_vocoder_vec.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int64, C.c_float, C.c_float, C.c_void_p]
    L.q3o_vocoder_vec.restype = None
    L.q3o_vocoder_stage.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p]
    L.q3o_vocoder_stage.restype = C.c_int32
    return L


def _oracle_pcm(O, v, codes, spf=1920):
    L = O.lib()
    L.q3o_vocoder_reset(v)
    codes = np.ascontiguousarray(codes, dtype=np.int32)
    pcm = np.zeros(codes.shape[0] * spf + 64, dtype=np.float32)
    n = L.q3o_vocoder_decode(v, O.ptr(codes, O.i32p), codes.shape[0], 1, O.ptr(pcm, O.f32p), pcm.size)
    return pcm[:n].copy()


def _rms(a, b):
    return float(np.sqrt(np.mean((np.asarray(a, np.float64) - b) ** 2)))


def _chunk_rms(a, b, spf=1920, k=4):
    n = a.size // (spf * k)
    return np.array([_rms(a[i * spf * k:(i + 1) * spf * k], b[i * spf * k:(i + 1) * spf * k]) for i in range(n)])


def _full_voc_engine(max_batch):
    from q3tts import _abi, native
    cfg = _abi.full_config_py()
    cfg.max_batch, cfg.n_ctx, cfg.max_steps_cap = max_batch, 256, 160
    m = cfg.model
    m.t_n_layer, m.p_n_layer = 1, 1   # the decoder is not under test here (as in test_full_shape_vocoder_pcm_vs_oracle)
    return cfg, native.NativeEngine(cfg)


def _check_pcm_vs_oracles(pcm, ref, ref32, what):
    """A4's PCM checks: whole-signal RMS against both oracles, every 4-frame chunk's RMS, and no drift past the window."""
    e, e32 = _rms(pcm, ref), _rms(pcm, ref32)
    ch = _chunk_rms(pcm, ref)
    before, after = ch[:18].max(), ch[19:].max()   # chunks of frames < 72 | chunks of frames >= 76
    print(f"{what}: PCM RMS vs bf16-input oracle {e:.2e}, vs f32 oracle {e32:.2e}; per 4-frame chunk: worst {ch.max():.2e}, "
          f"worst before frame 72 {before:.2e}, worst from frame 76 {after:.2e} (tolerance {PCM_RMS_TOL_FULL:.1e}, drift bound 1.5x)")
    assert e <= PCM_RMS_TOL_FULL and e32 <= PCM_RMS_TOL_FULL, (e, e32)
    assert ch.max() <= PCM_RMS_TOL_FULL, (int(ch.argmax()), ch.max())
    assert after <= 1.5 * before, (before, after)


def _latent_err(O, v, vc, codes, dev_x):
    """Per-frame relative error of the device's transformer rows (final RMSNorm applied here in float64) against the oracle's stage 2."""
    L = _voc_lib(O)
    ref = np.zeros((codes.shape[0], vc.latent_dim), dtype=np.float32)
    L.q3o_vocoder_stage(v, np.ascontiguousarray(codes, dtype=np.int32).ctypes.data, codes.shape[0], 2, ref.ctypes.data)
    w = np.zeros(vc.latent_dim, dtype=np.float32)
    L.q3o_vocoder_vec(v, 60, 0, vc.latent_dim, 1.0, 0.05, w.ctypes.data)   # final norm weights (VC_FINAL_NORM, VW_W)
    x = dev_x.astype(np.float64)
    y = x / np.sqrt(np.mean(x * x, axis=1, keepdims=True) + vc.rms_eps) * w.astype(np.float64)
    return np.sqrt(np.mean((y - ref) ** 2, axis=1) / np.mean(ref.astype(np.float64) ** 2, axis=1)), np.abs(y - ref).max(axis=1) / np.abs(ref).max(axis=1)


@pytest.fixture(scope="module")
def full_voc(oracle):
    cfg, eng = _full_voc_engine(1)
    L = oracle.lib()
    v = L.q3o_vocoder_create(C.byref(cfg.vocoder), 0, min(16, os.cpu_count() or 4))
    yield cfg, eng, v
    eng.close()
    L.q3o_vocoder_destroy(v)


def test_full_shape_vocoder_160_frames_latents_and_pcm(oracle, full_voc):
    """One slot, 160 random frames (max_steps_cap = 160: the last RoPE rows; the 76-row ring wraps twice; the call graph is captured on
    the 2nd call and replayed while the window fills and wraps). Latents frame by frame within VOC_LATENT_TOL(_EARLY) of the
    bf16-input oracle's stage 2; PCM within PCM_RMS_TOL_FULL of both oracles over the whole signal AND per 4-frame chunk, with no drift past the
    window. Then chunk_frames 0/1/3/4 and every launch variant give the same bits over all 160 frames."""
    cfg, eng, v = full_voc
    vc = cfg.vocoder
    n = cfg.max_steps_cap
    codes = np.random.default_rng(160).integers(0, vc.codebook_size, size=(n, 16)).astype(np.int32)
    t0 = time.time()
    lat = eng.vocoder_latent(codes, chunk_frames=4)
    err, emax = _latent_err(oracle, v, vc, codes, lat)
    print(f"full-shape vocoder latents, {n} frames: worst per-frame relative RMS error {err.max():.2e} (frame {int(err.argmax())}); "
          f"frames < 71: {err[:71].max():.2e} (tolerance {VOC_LATENT_TOL_EARLY:.1e}), frames >= 71: {err[71:].max():.2e} "
          f"(tolerance {VOC_LATENT_TOL:.1e}), frames >= 76: {err[76:].max():.2e}; worst max-abs / max |row| {emax.max():.2e}")
    assert err[:71].max() <= VOC_LATENT_TOL_EARLY, (int(err.argmax()), float(err.max()))
    assert err[71:].max() <= VOC_LATENT_TOL, (71 + int(err[71:].argmax()), float(err[71:].max()))
    assert np.array_equal(_bits(eng.vocoder_latent(codes, chunk_frames=0)), _bits(lat))
    one = eng.vocoder(codes)
    assert one.shape == (n * 1920,)
    ref = _oracle_pcm(oracle, v, codes)
    oracle.lib().q3o_vocoder_set_arith(v, 1)
    try:
        ref32 = _oracle_pcm(oracle, v, codes)
    finally:
        oracle.lib().q3o_vocoder_set_arith(v, 0)
    _check_pcm_vs_oracles(one, ref, ref32, f"full-shape vocoder, {n} frames")
    for ch in (1, 3, 4):
        assert np.array_equal(eng.vocoder(codes, chunk_frames=ch), one), ch
    for env in (("Q3TTS_VOC_ATTN_OLD",), ("Q3TTS_VOC_NORING",), ("Q3TTS_VOC_TAP_MIN",), ("Q3TTS_VOC_POLITE",), ("Q3TTS_VOC_POLITE", "Q3TTS_VOC_TAP_MIN")):
        for k in env:
            os.environ[k] = "1"
        try:
            assert np.array_equal(eng.vocoder(codes), one), env
            assert np.array_equal(eng.vocoder(codes, chunk_frames=3), one), env
            if env == ("Q3TTS_VOC_ATTN_OLD",):
                assert np.array_equal(_bits(eng.vocoder_latent(codes, chunk_frames=1)), _bits(lat))
        finally:
            for k in env:
                os.environ.pop(k, None)
    print(f"  ... oracle + variants {time.time() - t0:.0f} s")


def test_full_shape_64_slots_long_utterances_equal_the_one_slot_vocoder(oracle):
    """64 slots, 72 sampled requests with want_pcm, lengths forced over 25-160 frames: the first 64 run 76-160 frames (one of exactly 160,
    several with n % 4 == 0 and several not), so the 8 waiting requests (25-40 frames) take slots freed by utterances that ran past the
    76-row ring. Every utterance's PCM equals q3tts_k_vocoder on its returned codes BIT FOR BIT: slot count, chunking, launch mode and a
    slot's previous utterance never move a bit. The oracle replays three with A4's PCM checks: the longest (160), one on a re-used slot and
    one with n % 4 == 0 (the shorter two without the per-chunk drift bound, which needs frames past 76)."""
    import json
    cfg, eng = _full_voc_engine(64)
    threads = min(16, os.cpu_count() or 4)
    L = oracle.lib()
    v = L.q3o_vocoder_create(C.byref(cfg.vocoder), 0, threads)
    try:
        with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "speakers", "vivian.json")) as f:
            spk = np.asarray(json.load(f)["spk_emb"], dtype=np.float32)
        rng = np.random.default_rng(7272)
        lens = [int(x) for x in np.linspace(76, 160, 64).round()]
        lens[63] = 160
        lens += [25, 28, 31, 32, 36, 37, 40, 39]
        assert len(lens) == 72 and sum(1 for x in lens if x % 4 == 0) >= 8 and max(lens) == 160 and min(lens) == 25
        reqs, keep_all = [], []
        for i, n in enumerate(lens):
            desc, keep = oracle.make_prompt_desc(rng.integers(0, 151643, size=int(rng.integers(2, 9))), spk_emb=spk)
            keep_all.append(keep)
            reqs.append(dict(desc=desc, want_pcm=1, temperature=0.7, top_k=40, top_p=0.9, seed=500 + i, max_steps=n, min_frames=n, force_eos_at=n))
        outs = eng.generate_batch(reqs)
        assert all(o.status == 0 for o in outs) and [o.n_frames for o in outs] == lens
        for i, o in enumerate(outs):
            assert o.pcm.shape == (lens[i] * 1920,), i
            assert np.array_equal(eng.vocoder(o.codes), o.pcm), (i, lens[i])
        t0 = time.time()
        for i in (63, 64, 65):   # 160 frames; the first re-used slot (25 frames); n % 4 == 0 on a re-used slot (28 frames)
            codes = np.clip(outs[i].codes, 0, cfg.vocoder.codebook_size - 1).astype(np.int32)
            ref = _oracle_pcm(oracle, v, codes)
            L.q3o_vocoder_set_arith(v, 1)
            try:
                ref32 = _oracle_pcm(oracle, v, codes)
            finally:
                L.q3o_vocoder_set_arith(v, 0)
            if lens[i] > 80:
                _check_pcm_vs_oracles(outs[i].pcm, ref, ref32, f"64 slots, request {i} ({lens[i]} frames)")
            else:
                e, e32, ch = _rms(outs[i].pcm, ref), _rms(outs[i].pcm, ref32), _chunk_rms(outs[i].pcm, ref)
                print(f"64 slots, request {i} ({lens[i]} frames, re-used slot): PCM RMS {e:.2e} / {e32:.2e}, worst chunk {ch.max():.2e}")
                assert e <= PCM_RMS_TOL_FULL and e32 <= PCM_RMS_TOL_FULL and ch.max() <= PCM_RMS_TOL_FULL, (i, e, e32, ch.max())
        print(f"64 slots, 72 requests of 25..160 frames: every PCM equals the one-slot vocoder; oracle {time.time() - t0:.0f} s on {threads} threads")
    finally:
        eng.close()
        L.q3o_vocoder_destroy(v)


# ---- decode attention to n_ctx ------------------------------------------------------------------------------------------------
HD = 128
SECTIONS = np.array([24, 20, 20, 0], dtype=np.int32)
THETA, EPS = 1e6, 1e-6


def _rope_tables(n, hd=HD, theta=THETA, sections=SECTIONS):
    """The device's / oracle's table: angle in double, cos / sin rounded to f32."""
    half = hd // 2
    s3 = int(sections[:3].sum())
    i = np.arange(half)
    inv = np.power(float(theta), -2.0 * i / hd)
    ang = np.arange(n)[:, None].astype(np.float64) * inv[None, :]
    ang[:, i >= s3] = 0.0
    return np.cos(ang).astype(np.float32), np.sin(ang).astype(np.float32)


def _f64_decode(qkv_s, Hq, Hkv, qn, kn, cs, sn):
    """float64 reference of the decode row (the last of qkv_s): q / k RMSNorm and M-RoPE in float64 from the f32 tables, K / V rounded to
    bf16 as the cache stores them. Returns out [Hq * HD] and max |V| per KV head."""
    n = qkv_s.shape[0]
    half = HD // 2
    x = qkv_s.astype(np.float64).reshape(n, Hq + 2 * Hkv, HD)

    def norm_rope(h, w, pos):
        y = h / np.sqrt(np.mean(h * h, axis=-1, keepdims=True) + EPS) * w.astype(np.float64)
        c, s = cs[pos].astype(np.float64), sn[pos].astype(np.float64)
        a, b = y[..., :half], y[..., half:]
        return np.concatenate([a * c - b * s, b * c + a * s], axis=-1)
    pos = np.arange(n)
    k = norm_rope(x[:, Hq:Hq + Hkv], kn, pos[:, None])                        # [n][Hkv][HD]
    k = _bf16(k.astype(np.float32)).astype(np.float64)
    v = _bf16(x[:, Hq + Hkv:].astype(np.float32)).astype(np.float64)         # exact: the rows are f32
    q = norm_rope(x[n - 1, :Hq], qn, n - 1)                                    # [Hq][HD]
    R = Hq // Hkv
    out = np.zeros((Hq, HD))
    for h in range(Hq):
        g = h // R
        sc = k[:, g] @ q[h] / np.sqrt(HD)
        p = np.exp(sc - sc.max())
        out[h] = (p @ v[:, g]) / p.sum()
    return out.reshape(-1), np.abs(v).max(axis=(0, 2))


def _decode_case(rng, lens, Hq, Hkv, kind, cs):
    """qkv rows of every slot back to back, and the norm weights, for one input kind."""
    ld = (Hq + 2 * Hkv) * HD
    half = HD // 2
    qn = (1.0 + rng.standard_normal(HD) * 0.05).astype(np.float32)
    kn = (1.0 + rng.standard_normal(HD) * 0.05).astype(np.float32)
    if kind == "wide":            # scores ~ N(0, 16^2): a span of > 100 over the long slots, most exp() underflow
        qn, kn = qn * 4.0, kn * 4.0
    if kind in ("first", "newest"):
        qn = kn = np.full(HD, 2.0, dtype=np.float32)   # uniform weights: the norm commutes with the rotation below
    if kind == "uniform":         # k = 0: every score is 0, a uniform softmax over all keys
        kn = np.zeros(HD, dtype=np.float32)
    rows = []
    for n in lens:
        x = rng.standard_normal((n, ld)).astype(np.float32)
        qv = x[n - 1, :Hq * HD].reshape(Hkv, Hq // Hkv, HD)
        qv[:] = qv[:, :1]          # every query head of a group the same: the dominant key dominates all of them
        if kind == "newest":      # key at t = n - 1 (served from LDS by the fused kernels) = the query: score 2^2 * 128 / sqrt(128) ~ 45
            for g in range(Hkv):
                x[n - 1, (Hq + g) * HD:(Hq + g + 1) * HD] = qv[g, 0]
        if kind == "first" and n > 1:   # key at t = 0 (rotation 0) = the query rotated to position n - 1: the same score ~ 45
            c, s = cs[0][n - 1].astype(np.float64), cs[1][n - 1].astype(np.float64)
            for g in range(Hkv):
                a, b = qv[g, 0, :half].astype(np.float64), qv[g, 0, half:].astype(np.float64)
                x[0, (Hq + g) * HD:(Hq + g + 1) * HD] = np.concatenate([a * c - b * s, b * c + a * s]).astype(np.float32)
        if kind == "outliers":    # value rows at block edges
            for t, sgn in ((63, 1), (64, -1), (255, 1), (256, -1)):
                if t < n:
                    x[t, (Hq + Hkv) * HD:] = sgn * 300.0
        rows.append(x)
    return np.concatenate(rows), qn, kn


@pytest.mark.parametrize("n_ctx", [4096, 8192])
@pytest.mark.parametrize("Hq,Hkv,policy", [(4, 2, 0), (4, 2, 1), (4, 1, 0)])
def test_decode_attention_to_n_ctx(oracle, n_ctx, Hq, Hkv, policy):
    """One fused decode launch (q3tts_k_attention_decode) with slots of 1, 2, 63, 64, 65, 255, 256, 257, 1000, n_ctx - 1 and n_ctx keys:
    R = 2 runs k_attend_gqa2 (policy 0) or k_attend<2, true> (policy 1), R = 4 runs k_attend<4, true>; at these n_ctx the score buffer
    of k_attend<4, true> (and at 8192 that of both R = 2 kernels) is above 64 KiB of LDS. Per input kind (standard normals; scores spread
    over > 100; a dominant key at t = 0; a dominant newest key; a uniform softmax; +-300 value rows at 63/64 and 255/256): the f32 output
    equals the oracle bit for bit (q3o_attention_last), the bf16 operand equals bf16(f32 output), and the output is within ATT_F64_TOL of a
    float64 reference, relative to max |V|."""
    from q3tts import native
    L = oracle.lib()
    lens = [1, 2, 63, 64, 65, 255, 256, 257, 1000, n_ctx - 1, n_ctx]
    cs = _rope_tables(n_ctx)
    worst = {}
    for ki, kind in enumerate(("normal", "wide", "first", "newest", "uniform", "outliers")):
        rng = np.random.default_rng(1000 * n_ctx + 10 * Hq + Hkv + ki)
        qkv, qn, kn = _decode_case(rng, lens, Hq, Hkv, kind, cs)
        out, ob = native.k_attention_decode(qkv, lens, n_ctx, Hq, Hkv, HD, qn, kn, EPS, THETA, SECTIONS, policy=policy)
        assert np.array_equal(ob, _bf16_bits(out)), kind
        r0, w = 0, 0.0
        for s, n in enumerate(lens):
            q_s = np.ascontiguousarray(qkv[r0:r0 + n])
            ref = np.zeros(Hq * HD, dtype=np.float32)
            L.q3o_attention_last(oracle.ptr(q_s, oracle.f32p), n, Hq, Hkv, HD, oracle.ptr(qn, oracle.f32p), oracle.ptr(kn, oracle.f32p),
                                 EPS, THETA, oracle.ptr(SECTIONS, oracle.i32p), oracle.ptr(ref, oracle.f32p))
            assert np.array_equal(_bits(out[s]), _bits(ref)), (kind, n)
            f64, vmax = _f64_decode(q_s, Hq, Hkv, qn, kn, *cs)
            e = np.abs(out[s].astype(np.float64) - f64).reshape(Hkv, -1).max(axis=1) / vmax
            w = max(w, float(e.max()))
            if kind in ("first", "newest") and n > 1:   # the dominant key carries the output: its value row, not the mean of the others
                t = 0 if kind == "first" else n - 1
                vt = _bf16(q_s[t, (Hq + Hkv) * HD:]).reshape(Hkv, HD).astype(np.float64)
                vt = np.repeat(vt, Hq // Hkv, axis=0).reshape(-1)
                assert np.abs(f64 - vt).max() <= 1e-3 * np.abs(vt).max(), (kind, n)
            r0 += n
        worst[kind] = w
    print(f"decode attention, n_ctx {n_ctx}, R = {Hq // Hkv}, policy {policy}: oracle bits equal; worst error vs float64 / max|V|: "
          + ", ".join(f"{k} {v:.1e}" for k, v in worst.items()) + f" (tolerance {ATT_F64_TOL:.0e})")
    assert max(worst.values()) <= ATT_F64_TOL, worst


def test_engine_n_ctx_8192_long_prompts_greedy_ids(oracle):
    """A tiny engine with n_ctx = 8192: prompts of ~1000 and ~4000 rows admitted together (one group fills up to n_ctx rows, so both go
    through one prefill), 3 greedy frames: ids equal the oracle's under decode policy 0 (k_attend_gqa2) and 1 (k_attend<2, true)."""
    from q3tts import _abi, native
    cfg = _abi.tiny_config(max_batch=2, n_ctx=8192, with_vocoder=0)
    eng = native.NativeEngine(cfg)
    om = oracle.OracleModel(cfg.model, seed=0, n_ctx=8192, n_threads=min(16, os.cpu_count() or 4))
    lib = _abi.load_library()
    try:
        reqs, refs = [], []
        for n_text in (1000, 4000):
            desc, keep = oracle.make_prompt_desc(np.random.default_rng(n_text).integers(0, 151643, size=n_text),
                                                 spk_emb=((np.arange(cfg.model.d_embed) % 13 - 6) * 0.03125).astype(np.float32))
            pe = om.build_prompt(desc)
            assert pe.shape[0] >= n_text
            refs.append(om.generate(pe, temperature=0.0, max_steps=3, min_frames=3)[0])
            reqs.append(dict(embd=pe, temperature=0.0, max_steps=3, min_frames=3))
        try:
            for decode in (0, 1):
                assert lib.q3tts_k_attend_policy(decode, 0) == 0
                for o, r in zip(eng.generate_batch(reqs), refs):
                    assert o.status == 0 and np.array_equal(o.codes, r), decode
        finally:
            lib.q3tts_k_attend_policy(0, 0)
        print(f"n_ctx 8192: prompts of {reqs[0]['embd'].shape[0]} and {reqs[1]['embd'].shape[0]} rows, 3 greedy frames equal the oracle under both decode kernels")
    finally:
        eng.close()
        om.close()

"""The Predictor's layer-0 QKV table and the gathering form of k_attend_small, on the GPU.

With a bf16 Predictor and greedy heads, block 0 of passes q = 1 .. n_codebooks - 2 reads its raw q / k / v from a table row chosen by the
code of the pass before instead of launching k_pred_next(q) and the QKV GEMM. Every comparison here is `==` on raw bits: the table is
built with the decode path's own kernels and the gathering form runs the plain form's statements from the row pointer on, so there is
no tolerance to state.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HD, HQ, HKV, NCTX = 128, 4, 2, 64          # the Predictor's attention at the tiny shape of the parity tests (k_attend_small<2>)
LD, NQ = (HQ + 2 * HKV) * HD, HQ * HD
EPS, THETA = 1e-6, 1000000.0
NCB = 16


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _key(v, n):
    """q3_argmax_key(v, n) for a finite non-zero v; n may be any u32 (an index no codebook has gives an out-of-range code)."""
    u = int(np.float32(v).view(np.uint32))
    u = (~u & 0xFFFFFFFF) if u & 0x80000000 else (u | 0x80000000)
    return (u << 32) | (0xFFFFFFFF - (n & 0xFFFFFFFF))


def _code_of(keys_row):
    """k_pred_next<false>'s reduction: the largest key; q3_argmax_idx (key 0, which every NaN logit gives, is code 0)."""
    k = int(max(int(x) for x in keys_row))
    if k == 0:
        return 0
    c = 0xFFFFFFFF - (k & 0xFFFFFFFF)
    return c - (1 << 32) if c >= (1 << 31) else c


def _keys_for(rng, codes, n_parts, specials=()):
    """Per-tile maxima that make row b pick codes[b]: the winner sits in its own tile, every other tile holds a smaller logit.
    specials: {row: "tie" | "nan"} — a tie between two tiles at the same logit (the smaller index must win), or a row of key 0."""
    B = len(codes)
    keys = np.zeros((B, n_parts), dtype=np.uint64)
    for b, c in enumerate(codes):
        for t in range(n_parts):
            keys[b, t] = _key(float(rng.uniform(-2.0, 0.5)), 16 * t + int(rng.integers(0, 16)))
        kind = dict(specials).get(b)
        if kind == "nan":
            keys[b, :] = 0
        elif kind == "tie":   # codes[b] (in a tile before the last) and an index of a later tile, both at the winning logit
            t0 = c // 16
            t1 = int(rng.integers(t0 + 1, n_parts))
            keys[b, t0] = _key(1.5, c)
            keys[b, t1] = _key(1.5, 16 * t1 + 5)
        else:
            keys[b, (c // 16) % n_parts if 0 <= c < 16 * n_parts else int(rng.integers(0, n_parts))] = _key(1.5, c)
    return keys


def _state(native, rng, q, keys, rows_q, d, dp, active, cap=8):
    B = keys.shape[0]
    codec = rng.standard_normal((rows_q, d)).astype(np.float32)
    pproj = rng.standard_normal((rows_q, dp)).astype(np.float32)
    bias = rng.standard_normal(dp).astype(np.float32)
    fb = rng.standard_normal((B, d)).astype(np.float32)
    px = rng.standard_normal((B, dp)).astype(np.float32)
    codes = rng.integers(-5, 5, size=(B, cap, NCB)).astype(np.int32)
    n_frames = rng.integers(0, cap, size=B).astype(np.int32)
    mk = lambda: native.PredStepState(q, NCB, keys, active, n_frames, codec, pproj, bias, fb, px, codes)
    return mk, dict(codec=codec, pproj=pproj, bias=bias, fb=fb, px=px, codes=codes, n_frames=n_frames)


# ---------------------------------------------------------------------------------------------------------------
# 1. table rows = the bits k_pred_next + the QKV GEMM leave
# ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tiny_table(oracle):
    from q3tts import _abi, native
    cfg = _abi.tiny_config(max_batch=2, n_ctx=128, with_vocoder=0)
    eng = native.NativeEngine(cfg)
    m = cfg.model
    assets = oracle.synth_asset_tensors(m, 0, with_text=False)
    G, W = oracle._G_PRED, oracle._W
    st = lambda w, shape, base, std, rb: oracle.synth_tensor(0, oracle._tid(G, 0, W[w]), shape, base, std, rb)
    nq, nkv, dp = m.p_n_head * m.p_head_dim, m.p_n_kv_head * m.p_head_dim, m.p_d_model
    wqkv = np.concatenate([st("q", (nq, dp), 0.0, 0.02, True), st("k", (nkv, dp), 0.0, 0.02, True), st("v", (nkv, dp), 0.0, 0.02, True)])
    wb = (_bits(wqkv) >> 16).astype(np.uint16)   # (synthetic matrices are bf16-exact)
    assert np.array_equal((wb.astype(np.uint32) << 16).view(np.float32), wqkv)
    yield dict(eng=eng, cfg=cfg, assets=assets, wb=wb, nw=st("attn_norm", (dp,), 1.0, 0.05, False))
    eng.close()


@pytest.mark.parametrize("q", [1, NCB - 2])
def test_table_rows_are_the_decode_paths_bits(tiny_table, q):
    """q in {1, n_codebooks - 2}, codes {0, 1, rows - 1, -1, rows} (the last two: the fallback row). k_pred_next<false>(q) on keys that
    select the code writes the row's norm inputs; the QKV GEMM hook on them (STORE, the row scale from ssp) gives what the frame step
    left in sc.qkv. The table row must hold the same bits."""
    from q3tts import native
    t = tiny_table
    m = t["cfg"].model
    rows, d, dp = m.codecq_rows, m.d_embed, m.p_d_model
    codec = t["assets"]["codec_embd.%d" % q]
    pproj, _, _ = native.k_project(codec, t["assets"]["proj.weight"], t["assets"]["proj.bias"])   # pproj[q], by the kernel that builds it
    codes = [0, 1, rows - 1, -1, rows]
    rng = np.random.default_rng(q)
    keys = _keys_for(rng, codes, m.codebook_size // 16)
    assert [_code_of(k) for k in keys] == codes
    B = len(codes)
    stt = native.PredStepState(q, NCB, keys, np.ones(B, np.int32), np.zeros(B, np.int32), codec, pproj, t["assets"]["proj.bias"],
                               np.zeros((B, d), np.float32), np.zeros((B, dp), np.float32), np.zeros((B, 4, NCB), np.int32))
    xb, ssp = native.k_pred_next(stt, t["nw"])
    for b, c in enumerate(codes):   # the row k_pred_next put into px: the table row of the code, or the projection's bias
        want = pproj[c] if 0 <= c < rows else t["assets"]["proj.bias"]
        assert np.array_equal(_bits(stt.px[b]), _bits(want)), c
    y = native.k_bgemm(xb, t["wb"], ssp, dp, m.rms_eps, 0)["y"]
    for b, c in enumerate(codes):
        row = t["eng"].pred_table_row(q, c)
        assert np.array_equal(_bits(row), _bits(y[b])), (q, c)
    assert np.array_equal(_bits(t["eng"].pred_table_row(q, -1)), _bits(t["eng"].pred_table_row(q, rows)))
    assert not np.array_equal(_bits(t["eng"].pred_table_row(q, 0)), _bits(t["eng"].pred_table_row(q, 1)))


# ---------------------------------------------------------------------------------------------------------------
# 2. gathering attention = plain attention on the same rows; 3. its bookkeeping = k_pred_next's
# ---------------------------------------------------------------------------------------------------------------
def _gather_case(native, B, n_parts, pos, seed, out_form):
    """One gathering launch against the plain k_attend_small<2> fed the table rows of the same codes, and against k_pred_next<false> on the
    same keys and state. Rows: ordinary codes, a tie between two tiles, a row of NaN-loses keys, codes -1 and rows_q (the fallback
    row), and (B > 1) one inactive slot."""
    rng = np.random.default_rng(seed)
    rows_q, d, dp, q = 16 * n_parts, 512, 512, pos - 1     # pass q runs at position q + 1
    length = pos + 1
    codes = [int(c) for c in rng.integers(0, rows_q, size=B)]
    specials = {}
    if B >= 16:
        codes[1] = int(rng.integers(0, rows_q - 16)); specials[1] = "tie"
        specials[2] = "nan"
        codes[3], codes[4], codes[5] = -1, rows_q, rows_q - 1
        codes[6] = 0
    else:
        codes[0] = int(rng.integers(0, rows_q - 16)); specials[0] = "tie"
    keys = _keys_for(rng, codes, n_parts, specials)
    got_codes = [_code_of(k) for k in keys]
    for b in range(B):
        if specials.get(b) == "nan":
            assert got_codes[b] == 0      # q3_argmax_idx(0): what k_pred_next makes of a row whose logits are all NaN
        else:
            assert got_codes[b] == codes[b], (b, got_codes[b], codes[b])   # (a tie: the smaller index)
    active = np.ones(B, np.int32)
    if B > 1:
        active[B - 1] = 0
    table = (rng.standard_normal((rows_q + 1, LD)) * 0.7).astype(np.float32)
    qn = (1.0 + 0.1 * rng.standard_normal(HD)).astype(np.float32); kn = (1.0 + 0.1 * rng.standard_normal(HD)).astype(np.float32)
    runs = (rng.standard_normal((B, length, LD)) * 0.7).astype(np.float32)
    plain = runs.copy()
    for b in range(B):
        c = got_codes[b]
        plain[b, length - 1] = table[c if 0 <= c < rows_q else rows_q]
    gath = runs.copy()
    gath[:, length - 1] = np.float32(np.nan)     # never read: the gathering form is given only the keys
    ref = native.k_attention_decode_ex(plain.reshape(-1, LD), [length] * B, NCTX, HQ, HKV, HD, qn, kn, EPS, THETA, None, row_indexed=True, out_form=out_form)
    mk, init = _state(native, rng, q, keys, rows_q, d, dp, active)
    sg = mk()
    got = native.k_attention_gather(sg, table, gath.reshape(-1, LD), length, NCTX, HQ, HKV, HD, qn, kn, EPS, THETA, None, out_form=out_form)
    assert np.array_equal(got["out"].view(np.uint8), ref["out"].view(np.uint8))
    assert np.array_equal(got["k_cache"], ref["k_cache"]) and np.array_equal(got["v_cache"], ref["v_cache"])
    if out_form == 0:
        assert np.isfinite(got["out"]).all()
    sn = mk()
    native.k_pred_next(sn, (1.0 + 0.1 * rng.standard_normal(dp)).astype(np.float32))
    assert np.array_equal(sg.codes, sn.codes) and np.array_equal(_bits(sg.fb), _bits(sn.fb)) and np.array_equal(_bits(sg.px), _bits(sn.px))
    for b in range(B):   # and what that is, stated once more
        f = init["n_frames"][b]
        if not active[b]:
            assert np.array_equal(sg.codes[b], init["codes"][b]) and np.array_equal(_bits(sg.fb[b]), _bits(init["fb"][b]))
            assert np.array_equal(_bits(sg.px[b]), _bits(init["px"][b]))
            continue
        c = got_codes[b]
        ok = 0 <= c < rows_q
        want = init["codes"][b].copy(); want[f, q] = c
        assert np.array_equal(sg.codes[b], want), b
        assert np.array_equal(_bits(sg.fb[b]), _bits(init["fb"][b] + (init["codec"][c] if ok else np.float32(0.0)))), b
        assert np.array_equal(_bits(sg.px[b]), _bits(init["pproj"][c] if ok else init["bias"])), b


# B in {1, 16, 64}; positions 2 (the first gathered pass) and n_codebooks - 1 (the last). Key parts: 4 (the tiny codebook), 128 (the
# 1.7B shape's 2048 codes: both parts of a lane) and 130 (past 128: the loop)
@pytest.mark.parametrize("B,n_parts", [(1, 4), (16, 128), (64, 130)])
@pytest.mark.parametrize("pos", [2, NCB - 1])
def test_gathering_attention_equals_plain_attention(B, n_parts, pos):
    from q3tts import native
    _gather_case(native, B, n_parts, pos, seed=1000 * B + pos, out_form=1)   # the O projection's A-tiled bf16 operand: the frame step's form


def test_gathering_attention_f32_rows_and_bookkeeping():
    """One pass-q launch at B = 16 with f32 output rows: outputs, appended K / V, codes, fb and P.x against the plain kernel and
    k_pred_next<false>(q) on the same keys and state."""
    from q3tts import native
    _gather_case(native, 16, 4, 7, seed=77, out_form=0)


def test_gathering_launch_is_refused_for_other_kernels():
    """The gathering form exists for k_attend_small<2> only: a cache longer than 64 positions (k_attend_gqa2's launch) is refused loudly."""
    from q3tts import _abi, native
    rng = np.random.default_rng(5)
    keys = _keys_for(rng, [3], 4)
    mk, _ = _state(native, rng, 1, keys, 64, 512, 512, np.ones(1, np.int32))
    table = np.zeros((65, LD), np.float32)
    with pytest.raises(_abi.Q3Error, match="refused"):
        native.k_attention_gather(mk(), table, np.zeros((3, LD), np.float32), 3, 128, HQ, HKV, HD, np.ones(HD, np.float32), np.ones(HD, np.float32),
                                  EPS, THETA, None)


# ---------------------------------------------------------------------------------------------------------------
# 4. / 5. engine ids: the table frame against the frame with every launch, every row bucket, and the oracle
# ---------------------------------------------------------------------------------------------------------------
def _requests(oracle, om, cfg, n, seed):
    rng = np.random.default_rng(seed)
    reqs = []
    for i in range(n):
        n_text = int(rng.integers(3, 20))
        target = 8 + (i * 32) // max(n - 1, 1) if n > 1 else 12      # forced lengths spread over 8 .. 40 frames: every row bucket on the way down
        spk = ((np.arange(cfg.model.d_embed) % 13 - 6) * 0.03125).astype(np.float32)
        desc, keep = oracle.make_prompt_desc(rng.integers(0, 151643, size=n_text), spk_emb=spk)
        # greedy Predictor (the default), sampled Talker: the benchmark's 0.7 / 40 / 0.9
        kw = dict(temperature=0.7, top_k=40, top_p=0.9, seed=2000 + i, max_steps=48, min_frames=target, force_eos_at=target)
        reqs.append(dict(embd=om.build_prompt(desc), **kw))
    return reqs


def _engine(monkeypatch, cfg, **env):
    from q3tts import native
    for k in ("Q3TTS_PRED_TABLE", "Q3TTS_PRED_TABLE_MAX_MB"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    eng = native.NativeEngine(cfg)     # (both switches are read here, once)
    for k in env:
        monkeypatch.delenv(k, raising=False)
    return eng


def _has_table(eng):
    from q3tts import _abi
    try:
        eng.pred_table_row(1, 0)
        return True
    except _abi.Q3Error as e:
        assert "no layer-0 QKV table" in str(e)
        return False


@pytest.fixture(scope="module")
def batch64(oracle):
    """64 slots at the tiny shape: the requests, the oracle's replay of three of them, and the ids of the engine created under
    Q3TTS_PRED_TABLE=0 (the frame step with k_pred_next(q) and block 0's QKV GEMM in every pass)."""
    from q3tts import _abi
    mp = pytest.MonkeyPatch()
    cfg = _abi.tiny_config(max_batch=64, n_ctx=256, with_vocoder=0)
    om = oracle.OracleModel(cfg.model, seed=0, n_ctx=256, n_threads=4)
    try:
        reqs = _requests(oracle, om, cfg, 64, seed=640)
        refs = {i: om.generate(reqs[i]["embd"], **{k: v for k, v in reqs[i].items() if k != "embd"})[0] for i in (0, 31, 63)}
        eng = _engine(mp, cfg, Q3TTS_PRED_TABLE="0")
        try:
            assert not _has_table(eng)
            old = [o.codes for o in eng.generate_batch(reqs)]
            tm = eng.timings()
        finally:
            eng.close()
        assert [c.shape[0] for c in old] == [r["min_frames"] for r in reqs] and tm.mean_rows < 60.0   # it did drain through the buckets
        yield dict(cfg=cfg, reqs=reqs, refs=refs, old=old, old_bytes=tm.algo_bytes_per_step, old_live=tm.mean_live_slots)
    finally:
        om.close()
        mp.undo()


def test_engine_ids_with_table_equal_the_old_frame_and_the_oracle(batch64, monkeypatch):
    eng = _engine(monkeypatch, batch64["cfg"])
    try:
        assert _has_table(eng)
        outs = eng.generate_batch(batch64["reqs"])
        tm = eng.timings()
    finally:
        eng.close()
    for i, (o, c) in enumerate(zip(outs, batch64["old"])):
        assert o.status == 0 and np.array_equal(o.codes, c), i
    for i, r in batch64["refs"].items():
        assert np.array_equal(outs[i].codes, r), i
    # the byte accounting: n_codebooks - 2 streams of wqkv[0] out, one table row per live row and pass in
    m = batch64["cfg"].model
    nqkv = (m.p_n_head + 2 * m.p_n_kv_head) * m.p_head_dim
    assert abs(tm.mean_live_slots - batch64["old_live"]) < 1e-3
    want = batch64["old_bytes"] - (NCB - 2) * nqkv * m.p_d_model * 2 + int((NCB - 2) * tm.mean_live_slots * nqkv * 4)
    assert abs(tm.algo_bytes_per_step - want) <= 64, (tm.algo_bytes_per_step, want)


def test_engine_ids_at_batch_one(oracle, monkeypatch):
    from q3tts import _abi
    cfg = _abi.tiny_config(max_batch=1, n_ctx=256, with_vocoder=0)
    om = oracle.OracleModel(cfg.model, seed=0, n_ctx=256, n_threads=4)
    try:
        reqs = _requests(oracle, om, cfg, 3, seed=11)
        refs = [om.generate(r["embd"], **{k: v for k, v in r.items() if k != "embd"})[0] for r in reqs]
    finally:
        om.close()
    got = {}
    for name, env in (("table", {}), ("old", {"Q3TTS_PRED_TABLE": "0"})):
        eng = _engine(monkeypatch, cfg, **env)
        try:
            assert _has_table(eng) == (name == "table")
            got[name] = [eng.generate(**r).codes for r in reqs]
        finally:
            eng.close()
    for a, b, r in zip(got["table"], got["old"], refs):
        assert np.array_equal(a, b) and np.array_equal(a, r)


def test_table_above_the_size_limit_falls_back_silently(batch64, monkeypatch):
    """Q3TTS_PRED_TABLE_MAX_MB=0: the engine is created without a table, the row hook says so, the ids are the table engine's."""
    eng = _engine(monkeypatch, batch64["cfg"], Q3TTS_PRED_TABLE_MAX_MB="0")
    try:
        assert not _has_table(eng)
        outs = eng.generate_batch(batch64["reqs"])
    finally:
        eng.close()
    for i, (o, c) in enumerate(zip(outs, batch64["old"])):
        assert o.status == 0 and np.array_equal(o.codes, c), i


def test_sampling_predictor_keeps_its_launches(oracle, monkeypatch):
    """An engine WITH a table whose Predictor runs the sampling form of the frame step (forced, temperature 0: the greedy branch of the
    sampler) keeps k_pred_next and every QKV GEMM — and must give the ids of the table frame."""
    from q3tts import _abi
    cfg = _abi.tiny_config(max_batch=4, n_ctx=256, with_vocoder=0)
    om = oracle.OracleModel(cfg.model, seed=0, n_ctx=256, n_threads=4)
    try:
        reqs = _requests(oracle, om, cfg, 4, seed=3)
    finally:
        om.close()
    eng = _engine(monkeypatch, cfg)
    try:
        assert _has_table(eng)
        a = [o.codes for o in eng.generate_batch(reqs)]
        eng.k_pred_variant(1)
        b = [o.codes for o in eng.generate_batch(reqs)]
        eng.k_pred_variant(0)
        c = [o.codes for o in eng.generate_batch(reqs)]
    finally:
        eng.close()
    for x, y, z in zip(a, b, c):
        assert np.array_equal(x, y) and np.array_equal(x, z)


# ---------------------------------------------------------------------------------------------------------------
# 6. the 1.7B shape: the 470 MB build, short
# ---------------------------------------------------------------------------------------------------------------
def test_full_shape_table_ids_equal_the_oracle(oracle, monkeypatch):
    """4 utterances x 4 frames at the 1.7B shape with the table on (14 x 2049 x 4096 f32): ids equal the oracle's."""
    import os
    from q3tts import _abi
    cfg = _abi.full_config_py()
    cfg.max_batch, cfg.n_ctx, cfg.max_steps_cap, cfg.with_vocoder = 4, 128, 16, 0
    threads = min(16, os.cpu_count() or 4)
    om = oracle.OracleModel(cfg.model, seed=0, n_ctx=128, n_threads=threads)
    eng = _engine(monkeypatch, cfg)
    try:
        assert _has_table(eng)
        rng = np.random.default_rng(17)
        spk = ((np.arange(cfg.model.d_embed) % 13 - 6) * 0.03125).astype(np.float32)
        reqs, refs = [], []
        for i in range(4):
            desc, keep = oracle.make_prompt_desc(rng.integers(0, 151643, size=2 + i), spk_emb=spk)
            pe = om.build_prompt(desc)
            kw = dict(temperature=0.7, top_k=40, top_p=0.9, seed=1700 + i, max_steps=8, min_frames=4, force_eos_at=4)
            refs.append(om.generate(pe, **kw)[0])
            reqs.append(dict(embd=pe, **kw))
        outs = eng.generate_batch(reqs)
        for o, r in zip(outs, refs):
            assert o.status == 0 and r.shape == (4, 16) and np.array_equal(o.codes, r)
    finally:
        eng.close()
        om.close()

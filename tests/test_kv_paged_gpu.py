"""The paged Talker K/V cache (csrc/q3_attend_paged.hip, q3tts_engine_options.kv_pages) against the contiguous cache: paging
changes addresses, never arithmetic, so every comparison is `==` on bits. Unowned pool pages are filled with bf16 NaN: any read of one
that reaches a result shows. The f32 decode outputs are also held to the two-stage float64 bound of tests/_attend_ref.py."""
import ctypes as C

import numpy as np
import pytest

import _attend_ref as A
from _oracle import ATT_STAGE2_TOL

pytestmark = pytest.mark.gpu
NAN = 0x7FC0


def _table(lens_or_tot, n_ctx, perm, n_pages):
    """Rows of `perm` (a fixed scramble of page numbers), entries past each slot's last block zeroed: the zero page."""
    t = np.array(perm, dtype=np.int32).reshape(len(lens_or_tot), n_ctx // 64)
    for s, n in enumerate(lens_or_tot):
        t[s, (n + 63) // 64:] = 0
    assert t.max() <= n_pages and len(set(t[t > 0])) == (t > 0).sum()
    return t


def _inputs(rows, Hq, Hkv, seed):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((rows, (Hq + 2 * Hkv) * A.HD)).astype(np.float32)
    return x, (1.0 + rng.standard_normal(A.HD) * 0.05).astype(np.float32), (1.0 + rng.standard_normal(A.HD) * 0.05).astype(np.float32)


def _same(a, b, what):
    for k in ("out", "k_cache", "v_cache"):
        assert np.array_equal(a[k], b[k]), what + (k,)


# interleaves the two slots' pages, partly descending; pages 6, 13, 15, 16 (and whatever a short slot leaves) are spare
DECODE_PERM = [11, 2, 9, 4, 7, 14, 12, 1, 10, 3, 8, 5]


@pytest.mark.parametrize("length", [1, 63, 64, 65, 128, 257, 321])
@pytest.mark.parametrize("policy", [0, 1])
@pytest.mark.parametrize("Hkv,R", [(1, 1), (2, 2), (1, 4)])
def test_decode_kernels(Hkv, R, policy, length):
    from q3tts import native
    n_ctx, Hq = 384, Hkv * R
    lens = [length, (3 * length) // 4 + 1]
    x, qn, kn = _inputs(sum(lens), Hq, Hkv, [31, Hkv, R, length])
    tbl = _table(lens, n_ctx, DECODE_PERM, 16)
    args = (n_ctx, Hq, Hkv, A.HD, qn, kn, A.EPS, A.THETA, A.SECTIONS)
    for form in (0, 1):
        if R == 1:   # no fused kernel for one query head per KV head: the step is k_qk_prep + k_attend<1, false>, a run of one row
            runs = [(n - 1, 1) for n in lens]
            call = lambda **kw: native.k_attention_runs(x, runs, *args, policy=1, out_form=form, **kw)
        else:
            call = lambda **kw: native.k_attention_decode_ex(x, lens, *args, policy=policy, out_form=form, **kw)
        want, got = call(), call(paged=(16, tbl, NAN))
        _same(got, want, (Hkv, R, policy, length, form))
        r0 = got if form == 0 else r0
    assert native.k_attend_pick_paged(1 if R > 1 else 0, R, n_ctx, n_kv_head=Hkv) in ({1: (15,), 2: (18, 20), 4: (19,)}[R])
    # the f32 outputs against float64 attention over the cache as stored, from float64-prepared queries (stage 2 of _attend_ref)
    cs, sn = A.rope_tables(n_ctx)
    row0 = 0
    for s, n in enumerate(lens):
        h = x[row0 + n - 1].reshape(Hq + 2 * Hkv, A.HD)[:Hq].astype(np.float64)
        y = h / np.sqrt(np.mean(h * h, axis=-1, keepdims=True) + A.EPS) * qn.astype(np.float64)
        a, b, c, si = y[:, :64], y[:, 64:], cs[n - 1].astype(np.float64), sn[n - 1].astype(np.float64)
        q = np.concatenate([a * c - b * si, b * c + a * si], axis=-1).astype(np.float32)[None]
        kb, vb = r0["k_cache"][s].transpose(1, 0, 2)[:n], r0["v_cache"][s].transpose(1, 0, 2)[:n]
        err = A.stage2_error(r0["out"][s:s + 1], q, kb, vb, n - 1, Hq, Hkv)
        assert err <= ATT_STAGE2_TOL, (Hkv, R, policy, length, s, err)
        row0 += n


RUNS_A = [(0, 1), (0, 64), (0, 65), (60, 10), (64, 64), (0, 128)]   # k_attend_prefill's shapes (n <= 128, pos0 + n <= 256)
RUNS_B = [(0, 200)]                                                  # ... and one it does not take


@pytest.mark.parametrize("policy", [1, 2])
@pytest.mark.parametrize("runs", [RUNS_A, RUNS_B], ids=["short", "long"])
def test_prefill_and_append(runs, policy):
    from q3tts import native
    n_ctx, Hq, Hkv = 256, 4, 2
    tot = [p + n for p, n in runs]
    x, qn, kn = _inputs(sum(tot), Hq, Hkv, [32, len(runs)])
    n_pages = 4 * len(runs) + 3
    perm = [1 + (7 * i + 3) % (4 * len(runs)) for i in range(4 * len(runs))] if len(runs) > 1 else [4, 1, 6, 2]
    tbl = _table(tot, n_ctx, perm, n_pages)
    seg = dict(n_seg=len(runs), seg_max_n=max(n for _, n in runs), seg_max_t=max(tot))
    lib = native._abi.load_library()
    assert lib.q3tts_k_attend_policy(0, policy) == 0
    try:
        assert native.k_attend_pick_paged(0, 2, n_ctx, n_kv_head=Hkv, **seg) == (21 if (policy == 2 and runs is RUNS_A) else 16)
    finally:
        lib.q3tts_k_attend_policy(0, 0)
    for form in (0, 1):
        kw = dict(policy=policy, out_form=form)
        want = native.k_attention_runs(x, runs, n_ctx, Hq, Hkv, A.HD, qn, kn, A.EPS, A.THETA, A.SECTIONS, **kw)
        got = native.k_attention_runs(x, runs, n_ctx, Hq, Hkv, A.HD, qn, kn, A.EPS, A.THETA, A.SECTIONS, paged=(n_pages, tbl, NAN), **kw)
        _same(got, want, (len(runs), policy, form))


def test_prefix_copy_and_save():
    from q3tts import native
    L, Hkv, P, n_ctx = 2, 2, 70, 256
    rng = np.random.default_rng(33)
    ks, vs = (rng.integers(1, 0x7F00, size=(L, Hkv, 128 * A.HD)).astype(np.uint16) for _ in range(2))   # (nonzero past P too: the save zeroes it)
    want = native.k_kv_prefix_roundtrip(ks, vs, P, n_ctx)
    got = native.k_kv_prefix_roundtrip(ks, vs, P, n_ctx, paged=(9, [7, 3, 0, 0], NAN))
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    kz = ks.reshape(L, Hkv, 2, 16, 64, 8).copy()      # [block][chunk][key][8]
    kz[:, :, 1, :, P - 64:] = 0
    vz = vs.reshape(L, Hkv, 128, A.HD).copy()
    vz[:, :, P:] = 0
    assert np.array_equal(got[0], kz.reshape(ks.shape)) and np.array_equal(got[1], vz.reshape(vs.shape))


# ---- engines ------------------------------------------------------------------------------------------------------------------------
def _cfg(max_batch):
    from q3tts import _abi
    return _abi.tiny_config(max_batch=max_batch, n_ctx=256, with_vocoder=1)


def _requests(oracle, cfg, n_texts, steps, keep):
    spk = ((np.arange(cfg.model.d_embed) % 13 - 6) * 0.03125).astype(np.float32)
    reqs = []
    for i, (nt, ms) in enumerate(zip(n_texts, steps)):
        d, k = oracle.make_prompt_desc(np.random.default_rng([34, i]).integers(0, 151643, size=nt), spk_emb=spk)
        keep += [d, k]
        reqs.append(dict(desc=d, temperature=0.8, top_k=20, top_p=0.95, seed=100 + i, max_steps=ms, min_frames=ms, want_pcm=1))
    return reqs, spk


def _eq(a, b, what):
    assert a.status == 0 and b.status == 0, what
    assert np.array_equal(a.codes, b.codes), what
    assert np.array_equal(a.pcm.view(np.uint32), b.pcm.view(np.uint32)), what


def _session_one(native, _abi, eng, req):
    with native.NativeSession(eng) as sess:
        rid = sess.submit(**req)
        chunks, res = [], None
        for r, kind, pcm, fin, rs in sess.events(60000):
            assert r == rid
            if kind == _abi.EV_CHUNK:
                chunks.append(pcm)
            else:
                assert kind == _abi.EV_DONE, kind
                res = rs
    return res.codes, np.concatenate(chunks)


def test_engine_matches_contiguous(oracle):
    """Prompts of 56 .. 121 rows with max_steps that carry them over positions 64 and 128; five requests on two slots recycle pages."""
    from q3tts import _abi, native
    keep = []
    out = []
    for pages in (0, 12):
        cfg = _cfg(2)
        eng = native.NativeEngine(cfg, kv_pages=pages)
        try:
            if pages:
                eng.kv_pages_shuffle(7)
                assert eng.kv_pages == (12, 12, 0)
            reqs, spk = _requests(oracle, cfg, [45, 110, 50, 20, 100], [20, 16, 24, 12, 30], keep)
            res = eng.generate_batch(reqs)
            dv, kv = oracle.make_prompt_desc(None, part="voice", spk_emb=spk)
            dt, kt = oracle.make_prompt_desc(np.arange(200, 245), part="text")
            keep += [dv, kv, dt, kt]
            with eng.create_prefix(desc=dv) as x:
                behind = eng.generate_batch([dict(desc=dt, prefix=x, temperature=0.8, seed=5, max_steps=20, min_frames=20, want_pcm=1)])[0]
            sess = _session_one(native, _abi, eng, dict(reqs[1]))
            if pages:
                total, free, peak = eng.kv_pages
                assert free == total == 12 and 3 <= peak <= 12
            out.append((res, behind, sess))
        finally:
            eng.close()
    (res0, behind0, sess0), (res1, behind1, sess1) = out
    for i, (a, b) in enumerate(zip(res0, res1)):
        _eq(a, b, i)
    _eq(behind0, behind1, "prefix")
    assert np.array_equal(sess0[0], sess1[0]) and np.array_equal(sess0[1].view(np.uint32), sess1[1].view(np.uint32))
    assert np.array_equal(sess1[0], res1[1].codes)


def test_gating(oracle):
    """Four slots, eight requests of three pages each (111 prompt rows + 24 steps = 135 positions), a pool of seven: two run at a time."""
    from q3tts import _abi, native
    keep = []
    got = []
    for pages in (0, 7):
        cfg = _cfg(4)
        eng = native.NativeEngine(cfg, kv_pages=pages)
        try:
            reqs, spk = _requests(oracle, cfg, [100] * 8, [24] * 8, keep)
            # a ninth that cannot fit: kv_pages >= n_ctx / 64 holds for every engine, so what exceeds the pool exceeds n_ctx first
            over = dict(reqs[0], max_steps=64, min_frames=0, desc=oracle.make_prompt_desc(np.arange(190), spk_emb=spk)[0])
            res = eng.generate_batch(reqs + [over])
            assert res[8].status == -1   # Q3TTS_ERR_INVALID
            got.append(res[:8])
            if pages:
                total, free, peak = eng.kv_pages
                assert (total, free) == (7, 7) and 3 <= peak <= 7
        finally:
            eng.close()
    for i, (a, b) in enumerate(zip(*got)):
        _eq(a, b, i)


def test_refusals_and_memory(monkeypatch):
    from q3tts import _abi, native
    cfg = _cfg(2)
    cfg.kv_q8_0 = 1
    with pytest.raises(_abi.Q3Error, match=r"kv_pages.*kv_q8_0"):
        native.NativeEngine(cfg, kv_pages=8)
    with pytest.raises(_abi.Q3Error, match=r"kv_pages = 3.*n_ctx = 256"):
        native.NativeEngine(_cfg(2), kv_pages=3)
    eng = native.NativeEngine(_cfg(2), kv_pages=8)
    try:
        with pytest.raises(_abi.Q3Error, match=r"\(-6\).*paged"):
            native.NativeSession(eng, swap_mb=1)
    finally:
        eng.close()

    class OldOptions(C.Structure):
        _fields_ = [("struct_size", C.c_uint32), ("kquant_resident", C.c_int32)]
    lib, h, out = _abi.load_library(), C.c_void_p(), (C.c_int64 * 4)()
    cfg = _cfg(2)
    old = OldOptions(8, 0)
    assert lib.q3tts_engine_create_opts(C.byref(cfg), C.cast(C.pointer(old), C.POINTER(_abi.EngineOptions)), C.byref(h)) == 0
    assert lib.q3tts_get_kv_pages(h, out) == 0 and list(out) == [0, 0, 0, 0]
    lib.q3tts_engine_destroy(h)

    # 256 slots of n_ctx = 4096 over a pool far below 256 * 64 pages: the pool's bytes are the formula's, page for page
    monkeypatch.setenv("Q3TTS_NO_GRAPH", "1")   # (no frame-step captures: this is about memory)
    size = {}
    for pages in (64, 96):
        big = _abi.tiny_config(max_batch=256, n_ctx=4096, with_vocoder=0)
        eng = native.NativeEngine(big, kv_pages=pages)
        try:
            size[pages] = (eng.device_bytes(), eng.kv_pages_stats())
        finally:
            eng.close()
    m = big.model
    page = 2 * m.t_n_layer * m.t_n_kv_head * 64 * m.t_head_dim * 2
    assert size[64][1] == (64, 64, 0, page) and size[96][0] - size[64][0] == 32 * page
    assert size[64][0] < 256 * 64 * page   # the whole engine is smaller than the contiguous cache alone would be

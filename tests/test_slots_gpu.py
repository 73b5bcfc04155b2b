"""Engines of 65..256 slots on the device. The contract: a request's ids and PCM do not depend on the slot count — every
kernel sums in one batch-independent order — so the 64-slot engine, itself pinned to the oracle, is the reference
for the larger ones, with `==` on ids and on PCM bits; a few requests are replayed by the CPU oracle as tests/test_parity_gpu.py does.
The single launches whose shapes only more than 64 rows reach (GEMMs of 65..256 rows with every epilogue, attention over 65..256 slots)
are checked against the oracle on their own."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import _attend_ref as A
import _slots as SL

pytestmark = pytest.mark.gpu

PCM_RMS_TOL = 2e-3        # tests/test_parity_gpu.py: the small vocoder shapes
PCM_RMS_TOL_FULL = 3.5e-3  # ... and the full shape


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _rand(rng, shape, scale=1.0):
    return (rng.standard_normal(shape) * scale).astype(np.float32)


def _same(got, want, what):
    assert got.status == 0 and want.status == 0, (what, got.status, want.status)
    assert got.codes.shape == want.codes.shape and np.array_equal(got.codes, want.codes), what
    assert got.hit_eos == want.hit_eos, what
    assert (got.pcm is None) == (want.pcm is None), what
    if want.pcm is not None:
        assert got.pcm.shape == want.pcm.shape and np.array_equal(_bits(got.pcm), _bits(want.pcm)), what


def _oracle_pcm(oracle, v, codes, spf=1920):
    oracle.lib().q3o_vocoder_reset(v)
    pcm = np.zeros(codes.shape[0] * spf + 64, dtype=np.float32)
    n = oracle.lib().q3o_vocoder_decode(v, oracle.ptr(np.ascontiguousarray(codes, dtype=np.int32), oracle.i32p), codes.shape[0], 1,
                                        oracle.ptr(pcm, oracle.f32p), pcm.size)
    return pcm[:n].copy()


@pytest.fixture(scope="module")
def engines():
    e = SL.Engines()
    yield e
    e.close()


@pytest.fixture(scope="module")
def om(oracle, engines):
    m = oracle.OracleModel(engines.cfg(64).model, seed=0, n_ctx=SL.N_CTX, n_threads=8)
    yield m
    m.close()


@pytest.fixture(scope="module")
def mixed(oracle, engines, om):
    """The 260 requests and their results on the 64-slot engine (today's path): computed once, shared, never changed."""
    reqs = SL.mixed_requests(SL.base_rows(oracle, om))
    want = engines.get(64).generate_batch(reqs)
    return reqs, want


# ---- 1. the range ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nb", [65, 128, 256])
def test_engines_of_more_than_64_slots_are_created(engines, nb):
    eng = engines.get(nb)
    assert eng.row_buckets()[-1] == nb and eng.device_bytes() > 0


def test_257_slots_are_refused():
    from q3tts import _abi
    lib = _abi.load_library()
    cfg = _abi.tiny_config(max_batch=257, n_ctx=256, with_vocoder=0)
    h = C.c_void_p()
    assert lib.q3tts_engine_create(C.byref(cfg), C.byref(h)) == -1 and not h.value   # Q3TTS_ERR_INVALID
    assert b"max_batch" in lib.q3tts_last_error(None)


def test_a_footprint_above_the_cards_memory_is_refused_before_any_allocation():
    """256 slots of a 56-layer Talker at n_ctx 8192: the KV cache alone is 2 x 56 x 8 x 128 x 8192 x 2 B = 1.9 GB per slot, 481 GB for 256 —
    more than any card holds, so arithmetic decides and nothing is allocated. The message carries the bytes needed and the bytes free."""
    import re
    from q3tts import _abi
    lib = _abi.load_library()
    cfg = _abi.full_config_py()
    cfg.model.t_n_layer = 56
    cfg.max_batch, cfg.n_ctx, cfg.max_steps_cap = 256, 8192, 32
    kv = 256 * 2 * 56 * 8 * 128 * 8192 * 2
    assert kv > 400 << 30   # (the MI355X has 288 GB)

    def refused():
        h = C.c_void_p()
        assert lib.q3tts_engine_create(C.byref(cfg), C.byref(h)) == -3 and not h.value   # Q3TTS_ERR_OOM
        msg = lib.q3tts_last_error(None).decode()
        nums = [int(x) for x in re.findall(r"\d{9,}", msg)]
        assert len(nums) == 2, msg
        return nums + [msg]
    need, free, msg = refused()
    assert kv <= need < 2 * kv and 0 < free < need, msg
    need2, free2, _ = refused()
    assert need2 == need and abs(free2 - free) < (64 << 20)   # the refused call left nothing allocated


def test_the_footprint_is_a_lower_bound_of_what_the_engine_allocates(engines):
    """q3tts_k_engine_footprint (what create compares with the free memory) against q3tts_k_device_bytes of the created engine: never above
    it — it must not refuse a config that fits — on the tiny shape at 64, 128 and 256 slots and on the full shape, bf16 and Q8_0; and on
    the full shape at least half of it: what is left out — the text table (1.2 GB), the codec and projection tables (< 1 GB), the
    Predictor's QKV table (0.5 GB, bf16 only) and the vocoder's weights and work buffers (< 1 GB) — is below 3.7 GB, what is counted is
    above 6 GB even with Q8_0 weights."""
    from q3tts import _abi, native
    for nb in (64, 128, 256):
        fp, real = native.engine_footprint(engines.cfg(nb)), engines.get(nb).device_bytes()
        print(f"tiny, {nb} slots: footprint {fp} <= allocated {real}")
        assert 0 < fp <= real, nb
    for q8 in (0, 2):
        cfg = _abi.full_config_py()
        cfg.max_batch, cfg.n_ctx, cfg.max_steps_cap, cfg.talker_q8_0, cfg.predictor_q8_0 = 128, 256, 16, q8, q8
        eng = native.NativeEngine(cfg)
        try:
            fp, real = native.engine_footprint(cfg), eng.device_bytes()
        finally:
            eng.close()
        print(f"full shape, 128 slots, q8 {q8}: footprint {fp} <= allocated {real} ({fp / real:.2f})")
        assert 0.5 * real <= fp <= real, q8


# ---- 2. ids and PCM do not depend on the slot count ----------------------------------------------------------------------------------
def test_the_64_slot_reference_equals_the_oracle(oracle, engines, om, mixed):
    """Six of the 260 requests replayed by the oracle: the first, the one that lands in the highest slot of the 256-slot engine (255),
    the one that finishes as the batch's last live row (LONGEST), two that wait for a re-used slot on every engine (256, 258) and one
    from the middle. ids ==, PCM within the small-shape bound."""
    reqs, want = mixed
    cfg = engines.cfg(64)
    v = oracle.lib().q3o_vocoder_create(C.byref(cfg.vocoder), 0, 4)
    try:
        worst = 0.0
        for i in (0, SL.LONGEST, 129, 255, 256, 258):
            ref, _ = om.generate(reqs[i]["embd"], **SL.oracle_kw(reqs[i]))
            assert ref.shape[0] == reqs[i]["force_eos_at"] and np.array_equal(want[i].codes, ref), i
            if reqs[i]["want_pcm"]:
                ref_pcm = _oracle_pcm(oracle, v, np.clip(ref, 0, cfg.vocoder.codebook_size - 1).astype(np.int32))
                assert want[i].pcm.shape == ref_pcm.shape, i
                worst = max(worst, float(np.sqrt(np.mean((want[i].pcm - ref_pcm) ** 2))))
        print(f"64-slot reference: ids of 6 replayed requests equal; worst PCM RMS {worst:.2e} (bound {PCM_RMS_TOL:.0e})")
        assert sum(reqs[i]["want_pcm"] for i in (0, SL.LONGEST, 129, 255, 256, 258)) >= 4 and worst <= PCM_RMS_TOL
        assert reqs[SL.LONGEST]["force_eos_at"] == max(r["force_eos_at"] for r in reqs)
        assert sum(r["force_eos_at"] == reqs[SL.LONGEST]["force_eos_at"] for r in reqs) == 1
    finally:
        oracle.lib().q3o_vocoder_destroy(v)


@pytest.mark.parametrize("nb", [65, 128, 200, 256])
def test_ids_and_pcm_do_not_depend_on_the_slot_count(engines, mixed, nb):
    """The same 260 requests on an engine of nb slots: codes == and PCM == bit for bit with the 64-slot engine's. Requests are admitted as
    slots free up, so the batch drains through every bucket from nb down to 1 (200: 200 -> 192 -> 160 ...; its vocoder calls run
    64 + 64 + 64 + 8 slots); the counter shows that more than one bucket above 64 ran (one for 65: the only one it has)."""
    reqs, want = mixed
    eng = engines.get(nb)
    before = eng.bucket_steps()
    got = eng.generate_batch(reqs)
    steps = {b: n - before[b] for b, n in eng.bucket_steps().items()}
    for i, (g, w) in enumerate(zip(got, want)):
        _same(g, w, (nb, i))
    above = [b for b, n in steps.items() if b > 64 and n > 0]
    print(f"{nb} slots: frame steps per bucket {steps}")
    assert steps[nb] > 0 and len(above) >= (1 if nb == 65 else 2), steps
    assert any(n > 0 for b, n in steps.items() if b <= 64), steps    # ... and on through the buckets of 64 and fewer rows
    tm = eng.timings()
    assert tm.mean_rows - tm.mean_live_slots < 32.0   # multiples of 32 above 64: at most 31 padding rows


# ---- 3. one GEMM launch at decode row counts ------------------------------------------------------------------------------------------
ROWS = [65, 96, 127, 128, 129, 255, 256]
# the tiny shape's GEMMs: QKV (STORE), O / down (RESID), gate/up (SWIGLU), the Predictor's head (ARGMAX)
TINY_GEMMS = {0: (512, 1024), 1: (1024, 512), 2: (512, 2048), 3: (512, 64)}


def _policies(lib, fn):
    out = []
    try:
        for pol in (-1, 0):
            assert lib.q3tts_k_bgemm_policy(pol) == 0
            out.append(fn())
    finally:
        assert lib.q3tts_k_bgemm_policy(0) == 0
    return out


@pytest.mark.parametrize("epi", [0, 1, 2, 3], ids=["store", "resid", "swiglu", "argmax"])
@pytest.mark.parametrize("B", ROWS)
def test_bgemm_at_decode_row_counts(oracle, B, epi):
    from q3tts import _abi, native
    K, N = TINY_GEMMS[epi]
    rng = np.random.default_rng(1000 * epi + B)
    x = _rand(rng, (B, K), 1.5); x[:, :7] *= 300.0; x[:, 100:140] *= 1e-3
    xb, wb = A.bf16_bits(x), A.bf16_bits(_rand(rng, (N, K), 0.02))
    scaled = epi != 1
    ssp = (np.abs(_rand(rng, (B, K // 16), 4.0)) + 0.5).astype(np.float32) if scaled else None
    nw_next = (1.0 + _rand(rng, (N,), 0.05)).astype(np.float32) if epi == 1 else None
    y0 = _rand(rng, (B, N), 2.0) if epi == 1 else None
    ref = oracle.bgemm(xb, wb, ssp, K, 1e-6, epi, nw_next, y0)
    for got in _policies(_abi.load_library(), lambda: native.k_bgemm(xb, wb, ssp, K, 1e-6, epi, nw_next, y0)):
        if epi in (0, 1):
            assert np.array_equal(_bits(got["y"]), _bits(ref["y"]))
        if epi == 1:
            assert np.array_equal(got["yb"], ref["yb"]) and np.array_equal(_bits(got["ssp_out"]), _bits(ref["ssp_out"]))
        if epi == 2:
            assert np.array_equal(got["yb"], ref["yb"]) and np.count_nonzero(got["yb"] & 0x7fff) > got["yb"].size // 2
        if epi == 3:
            assert np.array_equal(got["keys"], ref["keys"])


@pytest.mark.parametrize("epi", [0, 1, 2, 3], ids=["store", "resid", "swiglu", "argmax"])
@pytest.mark.parametrize("B", ROWS)
def test_bgemm_q8a8_at_decode_row_counts(oracle, B, epi):
    from q3tts import _abi, native
    K, N = TINY_GEMMS[epi]
    rng = np.random.default_rng(5000 + 1000 * epi + B)
    a = _rand(rng, (B, K), 1.5); a[:, :7] *= 300.0; a[:, 100:140] *= 1e-3; a[B // 2, 64:96] = 0.0
    w = _rand(rng, (N, K), 0.02); w[3, 64:96] = 0.0; w[5 % N, :32] *= 40.0
    aq, ad = oracle.quantize_q8_0_act(a)   # f32 block scales, as the W8A8 producers store them
    q, d16 = oracle.quantize_q8_0(w)
    ssp = (np.abs(_rand(rng, (B, K // 16), 4.0)) + 0.5).astype(np.float32) if epi != 1 else None
    nw_next = (1.0 + _rand(rng, (N,), 0.05)).astype(np.float32) if epi == 1 else None
    y0 = _rand(rng, (B, N), 2.0) if epi == 1 else None
    lib = _abi.load_library()
    if epi == 3:   # the hook reduces the per-tile keys as k_pred_next does: ids == argmax of the oracle's logits, the lower column of a tie
        logits = oracle.bgemm_q8a8(aq, ad, q, d16, ssp, K, 1e-6, 0)["y"]
        for got in _policies(lib, lambda: native.k_bgemm_q8a8_argmax(aq, ad, q, d16, ssp, K, 1e-6)):
            assert np.array_equal(got, np.argmax(logits, axis=1))
        return
    ref = oracle.bgemm_q8a8(aq, ad, q, d16, ssp, K, 1e-6, epi, nw_next, y0)
    for got in _policies(lib, lambda: native.k_bgemm_q8a8(aq, ad, q, d16, ssp, K, 1e-6, epi, nw_next, y0)):
        if epi in (0, 1):
            assert np.array_equal(_bits(got["y"]), _bits(ref["y"]))
        if epi == 1:
            assert np.array_equal(_bits(got["ssp_out"]), _bits(ref["ssp_out"]))
        if epi in (1, 2):
            assert np.array_equal(got["yd"], ref["yd"]) and np.array_equal(got["yq"], ref["yq"])
            assert np.count_nonzero(got["yq"]) > got["yq"].size // 2


def test_the_picker_is_unchanged_up_to_64_rows():
    """q3tts_k_bgemm_pick for 1, 16, 48 and 64 rows of every decoder GEMM shape bench.py probes and of the two heads, bf16 and Q8_0 weights,
    and of the vocoder's transformer and upsampling shapes, against the table recorded from the commit before engines took more than 64 slots (tests/golden/bgemm_pick_le64.json)."""
    from q3tts import _abi
    lib = _abi.load_library()
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "bgemm_pick_le64.json")) as f:
        cases = json.load(f)["cases"]
    assert len(cases) == 100 and {c["B"] for c in cases} == {1, 16, 48, 64} and any(c["name"].startswith("vocoder") for c in cases)
    for c in cases:
        o5 = (C.c_int32 * 5)()
        assert lib.q3tts_k_bgemm_pick(c["B"], c["K"], c["N"], c["epilogue"], c["w_once"], c["q8"], o5) == 0
        assert list(o5) == c["pick"], c


# ---- 4. attention over more than 64 slots ---------------------------------------------------------------------------------------------
def _att_specs():
    v = lambda n_ctx, kernel, decode=None: dict(n_ctx=n_ctx, kernel=kernel, decode=decode, prefill=None)   # noqa: E731
    specs = []
    for n in (65, 130, 256):
        lens128 = [1 + (37 * i) % 128 for i in range(n)]   # 37 is a unit mod 128: every length 1 .. 128 (n >= 128), unequal neighbours
        lens64 = [1 + (29 * i) % 64 for i in range(n)]
        specs += [
            dict(name="slots%d_talker" % n, hook="decode", heads=(4, 2), seqs=[(t - 1, 1) for t in lens128], outliers=lambda i, p, k: (0, p // 2, p),
                 variants=[v(128, "k_attend_gqa2", 0), v(128, "k_attend<2, true>", 1)]),
            dict(name="slots%d_small" % n, hook="decode", heads=(4, 2), seqs=[(t - 1, 1) for t in lens64], outliers=lambda i, p, k: (15, 16, p),
                 variants=[v(64, "k_attend_small<2>")]),
            dict(name="slots%d_rowidx" % n, hook="decode", heads=(4, 2), seqs=[(16, 1)] * n, outliers=lambda i, p, k: (15, 16, p), row_indexed=True,
                 variants=[v(64, "k_attend_small<2>")]),
            dict(name="slots%d_pair" % n, hook="pair", heads=(4, 2), seqs=[(0, 2)] * n, outliers=lambda i, p, k: (i % 2,), variants=[v(64, "k_attend_pair")]),
        ]
    return specs


ATT_SPECS = {s["name"]: s for s in _att_specs()}


@pytest.mark.parametrize("name", sorted(ATT_SPECS))
def test_attention_over_more_than_64_slots(oracle, name):
    """tests/test_attend_gpu.py's six assertions (oracle bits, the bf16 and Q8_0 forms, the cache, the two-stage float64 reference, the
    kernel q3tts_k_attend_pick names) at 65, 130 and 256 slots: the Talker's decode kernels on slots of unequal lengths 1 .. n_ctx, the
    Predictor's k_attend_small<2> with both addressings and k_attend_pair. Two input kinds (the oracle walks every slot's whole sequence)."""
    from q3tts import native
    from test_attend_gpu import _check_case
    spec = ATT_SPECS[name]
    if "talker" in name and len(spec["seqs"]) >= 128:
        assert {p + 1 for p, _ in spec["seqs"]} == set(range(1, 129))
    worst = {}
    for kind in ("normal", "outliers"):
        _check_case(oracle, native, spec, kind, worst)
    print(name, {k: "%.1e" % e for k, e in worst.items()})


# ---- 5. more prefixed requests in one admission than the prefix descriptor holds ------------------------------------------------------
def test_prefixes_past_the_descriptor(oracle):
    """100 text-only requests behind one prefix and 30 whole-prompt requests, admitted together on 128 slots with n_ctx 2048: the text
    parts are 4 .. 8 rows, so all 130 prompts share ONE prefill group (about 1 200 of its 2 048 rows) and the 65th prefixed request finds
    the 64-entry descriptor full — q3tts_k_prefix_stats shows one group of 100 prefixed requests and two k_kv_prefix launches per
    admission. Codes and PCM == the same requests with whole prompts, under three attention policies."""
    from q3tts import _abi, native
    cfg = _abi.tiny_config(max_batch=128, n_ctx=2048, with_vocoder=1)
    eng = native.NativeEngine(cfg)
    d = cfg.model.d_embed
    voice = dict(spk_emb=SL.spk(d), lang_id=2055)
    rng = np.random.default_rng(100)
    keep, whole, mixed_reqs = [], [], []
    dv, kv = oracle.make_prompt_desc(None, part="voice", **voice)
    lib = _abi.load_library()
    try:
        with eng.create_prefix(desc=dv) as x:
            rows = 0
            for i in range(130):
                t = rng.integers(0, 151643, size=int(rng.integers(1, 6)))
                f = 2 + i % 7
                kw = dict(temperature=0.7, top_k=40, top_p=0.9, seed=900 + i, max_steps=12, min_frames=f, force_eos_at=f, want_pcm=1 if i % 4 == 0 else 0)
                dw, k1 = oracle.make_prompt_desc(t, **voice)
                dt, k2 = oracle.make_prompt_desc(t, part="text")
                keep += [dw, k1, dt, k2]
                whole.append(dict(desc=dw, **kw))
                mixed_reqs.append(dict(desc=dt, prefix=x, **kw) if i < 100 else dict(desc=dw, **kw))
                rows += len(t) + 3 + (0 if i < 100 else x.n_rows)
            assert rows <= cfg.n_ctx   # one prefill group holds them all
            want = eng.generate_batch(whole)
            assert eng.prefix_stats() == (0, 0)
            for k, pol in enumerate(((0, 0), (0, 2), (1, 1))):
                assert lib.q3tts_k_attend_policy(*pol) == 0
                got = eng.generate_batch(mixed_reqs)
                # the full descriptor (64 entries) was launched on its own, the other 36 with the group's layers
                assert eng.prefix_stats() == (2 * (k + 1), 100), (pol, eng.prefix_stats())
                for i, (g, w) in enumerate(zip(got, want)):
                    _same(g, w, (pol, i))
        assert all(w.codes.shape[0] == 2 + i % 7 for i, w in enumerate(want))
    finally:
        lib.q3tts_k_attend_policy(0, 0)
        eng.close()


# ---- 6. a session on 128 slots --------------------------------------------------------------------------------------------------------
def _session_case(oracle, eng, d, fmt, rate):
    """140 requests at once on 128 slots (12 wait): 128 whole-text ones and 12 with streamed text that arrives in pieces while the others
    run; one request is cancelled at its first chunk. Returns nothing; asserts every request's joined chunks == its generate_batch PCM."""
    from q3tts import _abi, native
    rng = np.random.default_rng(140)
    keep, reqs, texts = [], [], {}
    for i in range(140):
        ids = rng.integers(0, 151643, size=int(rng.integers(6, 14))).astype(np.uint32)
        f = 17 + (i * 5) % 7   # 17 .. 23 frames: all 128 slots still run in the fifth chunk, however far the worker is ahead of the consumer (4 staging buffers)
        kw = dict(temperature=0.7, top_k=40, top_p=0.9, seed=1400 + i, max_steps=24, min_frames=f, force_eos_at=f)
        desc, k = oracle.make_prompt_desc(ids, spk_emb=SL.spk(d))
        keep += [desc, k]
        if i % 11 == 5 and len(texts) < 12:
            texts[i] = ids
            reqs.append(dict(desc=desc, text_stream=True, **kw))
        else:
            reqs.append(dict(desc=desc, **kw))
    assert len(texts) == 12
    victim = 7
    reqs[victim] = dict(reqs[victim], max_steps=40, min_frames=40, force_eos_at=40)
    want = eng.generate_batch([dict(r, want_pcm=1) for r in reqs])
    got, cancelled = {}, False
    steps0 = eng.bucket_steps()
    with native.NativeSession(eng, fmt) as sess:
        ids_of, fed = {}, {}
        for i, r in enumerate(reqs):
            if i in texts:   # the first two ids now, open: the rest follows in two pieces
                d1, k1 = oracle.make_prompt_desc(texts[i][:2], spk_emb=SL.spk(d))
                keep += [d1, k1]
                rid = sess.submit(**dict(r, desc=d1, text_open=True))
                fed[rid] = [texts[i][2:5], texts[i][5:]]
            else:
                rid = sess.submit(**r)
            ids_of[rid] = i
        vid = [rid for rid, i in ids_of.items() if i == victim][0]
        n_events, fed_at = 0, [None, None]   # fed_at: the bucket-step counts (since the session began) at the two appends
        while sess._open:
            ev = sess.next(120000)
            assert ev is not None, "the session went quiet"
            rid, kind, pcm, fin, res = ev
            n_events += 1
            if n_events in (3, 40):   # text arrives while more than 64 others run: first the middle piece of every streamed request, later the rest
                fed_at[0 if n_events == 3 else 1] = {b: n - steps0[b] for b, n in eng.bucket_steps().items()}
                for r2, pieces in fed.items():
                    if pieces:
                        p = pieces.pop(0)
                        sess.append_text(r2, p, close=not pieces)
            g = got.setdefault(rid, dict(chunks=[], final=None))
            if rid == vid and cancelled:
                assert kind == _abi.EV_CANCELLED, "an event of the cancelled request other than CANCELLED"
            if kind == _abi.EV_CHUNK:
                g["chunks"].append((pcm, fin))
                if rid == vid and not cancelled:
                    sess.cancel(vid); cancelled = True
            else:
                g["final"] = (kind, res)
    assert cancelled and got[vid]["final"][0] == _abi.EV_CANCELLED and len(got[vid]["chunks"]) == 1
    steps = {b: n - steps0[b] for b, n in eng.bucket_steps().items()}
    # both text pieces were appended while more than 64 slots ran: frame steps on buckets above 64 before AND after the second append
    assert fed_at[0] is not None and fed_at[1] is not None, fed_at
    assert sum(n for b, n in fed_at[0].items() if b > 64) > 0, fed_at
    assert sum(n for b, n in steps.items() if b > 64) > sum(n for b, n in fed_at[1].items() if b > 64) > 0, (steps, fed_at)
    for rid, i in ids_of.items():
        if i == victim:
            continue
        g, w = got[rid], want[i]
        kind, res = g["final"]
        assert kind == _abi.EV_DONE and res.status == 0 and np.array_equal(res.codes, w.codes), i
        assert g["chunks"] and g["chunks"][-1][1] and not any(f for _, f in g["chunks"][:-1]), i
        pcm = np.concatenate([c for c, _ in g["chunks"]])
        if fmt == _abi.PCM_I16:
            ref = np.trunc(np.clip(w.pcm * np.float32(32767), -32768, 32767)).astype(np.int16)
            assert pcm.dtype == np.int16 and np.array_equal(pcm, ref), i
        else:
            assert pcm.dtype == np.float32 and np.array_equal(_bits(pcm), _bits(w.pcm)), i
        assert res.n_samples == pcm.size and res.sample_rate == (rate or 24000), i


@pytest.mark.parametrize("fmt,rate", [("f32", 0), ("i16", 0), ("f32", 8000)])
def test_session_on_128_slots(oracle, engines, fmt, rate):
    from q3tts import _abi
    eng = engines.get(128)
    if rate:
        eng.set_output_rate(rate)
    try:
        _session_case(oracle, eng, engines.cfg(128).model.d_embed, _abi.PCM_I16 if fmt == "i16" else _abi.PCM_F32, rate)
    finally:
        if rate:
            eng.set_output_rate(0)


# ---- 7. the Predictor sampler with the repetition penalty, and W8A8 ------------------------------------------------------------------
def _pred_requests(oracle, om, n=130):
    rng = np.random.default_rng(130)
    reqs = []
    for i in range(n):
        desc, keep = oracle.make_prompt_desc(rng.integers(0, 151643, size=int(rng.integers(3, 24))), spk_emb=SL.spk(om.cfg.d_embed))
        t = 2 + i % 7
        reqs.append(dict(embd=om.build_prompt(desc), temperature=0.7, top_k=40, top_p=0.9, seed=1300 + i, max_steps=12, min_frames=t, force_eos_at=t))
    return reqs


def test_predictor_sampler_and_penalty_on_128_slots(oracle, om):
    """The sampling frame step (stored logits, k_pred_next<true>) with the repetition penalty at 1.05 on 128 slots: codes == a 64-slot
    engine's for 130 requests, four replayed by tests/_pred_sample.py."""
    import _pred_sample as S
    from q3tts import native
    ps, pen = S.PRED_CONFIGS["select"], 1.05
    reqs = _pred_requests(oracle, om)
    pred = S.mats_from_model(om, False, False)
    outs = {}
    for nb in (128, 64):
        eng = native.NativeEngine(S.tiny_cfg(max_batch=nb))
        try:
            eng.set_predictor_sampler(*ps)
            eng.set_repetition_penalty(pen)
            outs[nb] = eng.generate_batch(reqs)
        finally:
            eng.close()
    for i, (g, w) in enumerate(zip(outs[128], outs[64])):
        _same(g, w, i)
    for i in (0, 64, 127, 129):
        ref, _ = S.generate(om, pred, reqs[i]["embd"], pred_sampler=ps, penalty=pen, **SL.oracle_kw(reqs[i]))
        assert np.array_equal(outs[128][i].codes, ref), i


def test_w8a8_on_128_slots(oracle):
    """talker_q8_0 = 2 and predictor_q8_0 = 2 (k_bgemm8 at 65..256 rows in every GEMM of the step) on 128 slots: codes == a 64-slot engine's
    for 130 requests, four replayed by tests/_pred_q8.py over the oracle's W8A8 Talker."""
    import _pred_q8 as P
    from q3tts import _abi, native
    cfg = {nb: _abi.tiny_config(max_batch=nb, n_ctx=SL.N_CTX, with_vocoder=0) for nb in (128, 64)}
    for c in cfg.values():
        c.talker_q8_0 = c.predictor_q8_0 = 2
    om8 = oracle.OracleModel(cfg[64].model, seed=0, n_ctx=SL.N_CTX, n_threads=8)
    try:
        om8.set_talker_q8a8()
        reqs = _pred_requests(oracle, om8)
        outs = {}
        for nb in (128, 64):
            eng = native.NativeEngine(cfg[nb])
            try:
                outs[nb] = eng.generate_batch(reqs)
            finally:
                eng.close()
        for i, (g, w) in enumerate(zip(outs[128], outs[64])):
            _same(g, w, i)
        pred = P.mats_from_model(om8, False, True)
        for i in (0, 64, 127, 129):
            ref, _ = P.generate(om8, pred, reqs[i]["embd"], **SL.oracle_kw(reqs[i]))
            assert np.array_equal(outs[128][i].codes, ref), i
    finally:
        om8.close()


# ---- 8. the full shape, once ----------------------------------------------------------------------------------------------------------
def test_full_shape_128_slots(oracle):
    """The 1.7B shape with 128 slots at n_ctx 256: 130 sampled requests of <= 8 frames with PCM — codes and PCM == the same list on a 64-slot
    engine; two are replayed by the oracle (ids ==, PCM within the full-shape bound), as tests/test_parity_gpu.py's full-shape test does."""
    from q3tts import _abi, native
    threads = min(16, os.cpu_count() or 4)
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "speakers", "vivian.json")) as f:
        spk = np.asarray(json.load(f)["spk_emb"], dtype=np.float32)
    rng = np.random.default_rng(128128)
    reqs, metas, keep = [], [], []
    for i in range(130):
        desc, k = oracle.make_prompt_desc(rng.integers(0, 151643, size=int(rng.integers(2, 9))), spk_emb=spk)
        keep.append((desc, k))
        t = 1 + i % 8 if i not in (0, 129) else 3
        kw = dict(temperature=0.7, top_k=40, top_p=0.9, seed=5000 + i, max_steps=12, min_frames=t, force_eos_at=t)
        reqs.append(dict(desc=desc, want_pcm=1, **kw)); metas.append((desc, kw, t))
    outs = {}
    for nb in (128, 64):
        cfg = _abi.full_config_py()
        cfg.max_batch, cfg.n_ctx, cfg.max_steps_cap = nb, 256, 16
        eng = native.NativeEngine(cfg)
        try:
            outs[nb] = eng.generate_batch(reqs)
            if nb == 128:
                steps = eng.bucket_steps()
                assert steps[128] > 0 and steps[96] > 0, steps
        finally:
            eng.close()
    for i, (g, w) in enumerate(zip(outs[128], outs[64])):
        _same(g, w, i)
        assert g.codes.shape[0] == metas[i][2] and g.pcm.size == metas[i][2] * 1920, i
    cfg = _abi.full_config_py()
    om = oracle.OracleModel(cfg.model, seed=0, n_ctx=256, n_threads=threads)
    v = oracle.lib().q3o_vocoder_create(C.byref(cfg.vocoder), 0, threads)
    try:
        worst = 0.0
        for i in (0, 129):   # the first slot, and a request that waits for a re-used slot
            desc, kw, t = metas[i]
            ref, _ = om.generate(om.build_prompt(desc), **kw)
            assert ref.shape == (t, 16) and np.array_equal(outs[128][i].codes, ref), i
            ref_pcm = _oracle_pcm(oracle, v, np.clip(ref, 0, cfg.vocoder.codebook_size - 1).astype(np.int32))
            assert outs[128][i].pcm.shape == ref_pcm.shape, i
            worst = max(worst, float(np.sqrt(np.mean((outs[128][i].pcm - ref_pcm) ** 2))))
        print(f"full shape, 128 slots: ids of 2 replayed requests equal; worst PCM RMS {worst:.2e} (bound {PCM_RMS_TOL_FULL:.1e})")
        assert worst <= PCM_RMS_TOL_FULL
    finally:
        om.close()
        oracle.lib().q3o_vocoder_destroy(v)


# ---- 9. a node whose engines take more than 64 slots ----------------------------------------------------------------------------------
def test_node_with_more_than_64_slots(engines, mixed):
    """q3tts_node_* with max_batch = 128 on one device: the engine of the node takes the config's slot count, and 140 of the mixed
    requests give the codes and PCM of the 64-slot engine."""
    from q3tts import native
    reqs, want = mixed
    node = native.NativeNode(engines.cfg(128), [0])
    try:
        got = node.generate_batch(reqs[:140])
    finally:
        node.close()
    for i, (g, w) in enumerate(zip(got, want[:140])):
        _same(g, w, i)

"""Sessions (include/q3tts.h, "sessions"): continuous batching with per-request streaming through the C ABI.

Every request's chunks, joined, must equal what q3tts_generate_batch returns for it bit for bit; chunk sizes must equal the streaming
ABI's (q3tts_stream_poll, the reference vocoder thread's calls: src/tts/engine.rs:507-541); the codes must equal the batch's (and the
oracle's for a few). Also the PCM gather kernel hook against numpy.
"""
import ctypes as C
import json
import os
import threading

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _spk(d):
    return ((np.arange(d) % 13 - 6) * 0.03125).astype(np.float32)


def _i16(pcm):
    return np.trunc(np.clip(pcm * np.float32(32767), -32768, 32767)).astype(np.int16)


def _collect(sess, timeout_ms=120000):
    """Reads events until every submitted id has its final: {id: dict(chunks=[(pcm, is_final)], final=(kind, result), order=[kinds])}."""
    from q3tts import _abi
    got = {}
    for rid, kind, pcm, fin, res in sess.events(timeout_ms):
        g = got.setdefault(rid, dict(chunks=[], final=None, order=[]))
        assert g["final"] is None, "an event after the final one"
        g["order"].append(kind)
        if kind == _abi.EV_CHUNK:
            g["chunks"].append((pcm, fin))
        else:
            assert fin
            g["final"] = (kind, res)
    assert not sess._open, "events timed out"
    return got


def _check_done(g, want, sizes=None):
    from q3tts import _abi
    kind, res = g["final"]
    assert kind == _abi.EV_DONE and res.status == 0 and res.pcm is None
    assert g["chunks"] and g["chunks"][-1][1] and not any(f for _, f in g["chunks"][:-1])
    pcm = np.concatenate([c for c, _ in g["chunks"]])
    assert np.array_equal(res.codes, want.codes)
    assert pcm.dtype == want.pcm.dtype and np.array_equal(pcm.view(np.uint32), want.pcm.view(np.uint32))
    assert res.n_samples == pcm.size
    if sizes is not None:
        assert [c.size for c, _ in g["chunks"] if c.size] == sizes
    return pcm


@pytest.fixture(scope="module")
def tiny4(oracle):
    from q3tts import _abi, native
    cfg = _abi.tiny_config(max_batch=4, n_ctx=256, with_vocoder=1)
    eng = native.NativeEngine(cfg)
    om = oracle.OracleModel(cfg.model, seed=0, n_ctx=256, n_threads=4)
    desc, keep = oracle.make_prompt_desc(np.arange(100, 112), spk_emb=_spk(cfg.model.d_embed))
    pe = om.build_prompt(desc)
    yield cfg, eng, om, pe
    eng.close()
    om.close()


def _mixed(pe, n=11):
    return [dict(embd=pe, temperature=0.7, top_k=40, top_p=0.9, seed=100 + i, max_steps=20, min_frames=3 + (i * 7) % 15,
                 force_eos_at=3 + (i * 7) % 15) for i in range(n)]


def test_session_equals_generate_batch_and_streaming(tiny4):
    """11 sampled requests of mixed lengths (force_eos_at 3..17) at once over 4 slots: joined chunks == generate_batch PCM bit for bit, codes
    == batch codes (== the oracle's for three), chunk sizes == the streaming ABI's."""
    from q3tts import native
    cfg, eng, om, pe = tiny4
    reqs = _mixed(pe)
    assert sorted({r["force_eos_at"] for r in reqs})[0] == 3 and max(r["force_eos_at"] for r in reqs) == 17
    want = eng.generate_batch([dict(r, want_pcm=1) for r in reqs])
    sizes = [[c.size for c, _ in native.stream_chunks(eng, **dict(r, want_pcm=1))] for r in reqs]
    for i in (0, 4, 10):
        ref, _ = om.generate(pe, **{k: v for k, v in reqs[i].items() if k != "embd"})
        assert np.array_equal(want[i].codes, ref), i
    with native.NativeSession(eng) as sess:
        ids = [sess.submit(**r) for r in reqs]
        got = _collect(sess)
    for i, rid in enumerate(ids):
        _check_done(got[rid], want[i], sizes[i])
        assert got[rid]["final"][1].n_frames == reqs[i]["force_eos_at"]


def test_session_late_arrivals_from_another_thread(tiny4):
    from q3tts import _abi, native
    cfg, eng, om, pe = tiny4
    reqs = _mixed(pe, 8)
    want = eng.generate_batch([dict(r, want_pcm=1) for r in reqs])
    sizes = [[c.size for c, _ in native.stream_chunks(eng, **dict(r, want_pcm=1))] for r in reqs]
    got = {}
    with native.NativeSession(eng) as sess:
        ids = [sess.submit(**r) for r in reqs[:3]]
        seen = set()
        while len(seen) < 3:   # every early request has produced a chunk
            rid, kind, pcm, fin, res = sess.next(60000)
            g = got.setdefault(rid, dict(chunks=[], final=None, order=[]))
            g["order"].append(kind)
            if kind == _abi.EV_CHUNK:
                g["chunks"].append((pcm, fin)); seen.add(rid)
            else:
                g["final"] = (kind, res); seen.add(rid)
        late = []
        th = threading.Thread(target=lambda: late.extend(sess.submit(**r) for r in reqs[3:]))
        th.start(); th.join()
        ids += late
        for rid, v in _collect(sess).items():
            g = got.setdefault(rid, dict(chunks=[], final=None, order=[]))
            assert g["final"] is None
            g["chunks"] += v["chunks"]; g["final"] = v["final"]; g["order"] += v["order"]
    for i, rid in enumerate(ids):
        _check_done(got[rid], want[i], sizes[i])


def test_session_vocoder_lookahead(oracle):
    """V4 (lookahead_frames = 2) on the six lengths of test_vocoder_lookahead_on_the_device: chunk sizes == the q3o_chunk_plan parts of the
    reference thread; with vocoder_flush_tail = 1 every frame is audio and the last chunk is final; joined == generate_batch of the same engine."""
    from q3tts import _abi, native
    LA = 2
    om = None
    engs = []
    try:
        for flush in (0, 1):
            cfg = _abi.tiny_config(max_batch=2, n_ctx=256, with_vocoder=1)
            cfg.vocoder.lookahead_frames = LA
            cfg.vocoder_flush_tail = flush
            eng = native.NativeEngine(cfg); engs.append(eng)
            if om is None:
                om = oracle.OracleModel(cfg.model, seed=0, n_ctx=256, n_threads=4)
                desc, keep = oracle.make_prompt_desc(np.arange(60, 70), spk_emb=_spk(cfg.model.d_embed))
                pe = om.build_prompt(desc)
            lens = (8, 6, 3, 4, 12, 13)
            reqs = [dict(embd=pe, temperature=0.7, top_k=40, top_p=0.9, seed=40 + n, max_steps=16, min_frames=n, force_eos_at=n) for n in lens]
            want = eng.generate_batch([dict(r, want_pcm=1) for r in reqs])
            L = oracle.lib()
            with native.NativeSession(eng) as sess:
                ids = [sess.submit(**r) for r in reqs]
                got = _collect(sess)
            for n, rid, w in zip(lens, ids, want):
                g = got[rid]
                if flush:
                    pcm = _check_done(g, w)
                    assert pcm.size == n * 1920 and g["chunks"][-1][1], n
                else:   # the reference thread's calls (q3o_chunk_plan); the streaming ABI gives the same sizes (test_parity_gpu)
                    cf, cl = np.zeros(n + 2, dtype=np.int32), np.zeros(n + 2, dtype=np.int32)
                    k = L.q3o_chunk_plan(n, oracle.ptr(cf, oracle.i32p), oracle.ptr(cl, oracle.i32p), cf.size)
                    sizes = [c.size for c, _ in native.stream_chunks(eng, **dict(reqs[lens.index(n)], want_pcm=1))]
                    assert len(sizes) <= k
                    pcm = _check_done(g, w, sizes)
                    assert pcm.size == (n - LA if n % 4 == 0 else n) * 1920, n
    finally:
        for e in engs:
            e.close()
        if om is not None:
            om.close()


def test_session_cancel(tiny4):
    """Cancel one request after its first chunk: no further chunk, exactly one CANCELLED; the others equal a generate_batch run without it,
    and a later request that reuses its slot is bit-identical too."""
    from q3tts import _abi, native
    cfg, eng, om, pe = tiny4
    reqs = _mixed(pe, 6)
    victim = 1
    reqs[victim] = dict(reqs[victim], max_steps=40, min_frames=40, force_eos_at=40)
    others = [r for i, r in enumerate(reqs) if i != victim]
    extra = dict(embd=pe, temperature=0.7, top_k=40, top_p=0.9, seed=777, max_steps=20, min_frames=9, force_eos_at=9)
    want = eng.generate_batch([dict(r, want_pcm=1) for r in others + [extra]])
    with native.NativeSession(eng) as sess:
        ids = [sess.submit(**r) for r in reqs]
        vid = ids[victim]
        got, cancelled = {}, False
        while sess._open:
            ev = sess.next(60000)
            assert ev is not None
            rid, kind, pcm, fin, res = ev
            g = got.setdefault(rid, dict(chunks=[], final=None, order=[]))
            g["order"].append(kind)
            if rid == vid and cancelled:
                assert kind == _abi.EV_CANCELLED, "an event of the cancelled request other than CANCELLED"
            if kind == _abi.EV_CHUNK:
                g["chunks"].append((pcm, fin))
                if rid == vid and not cancelled:
                    sess.cancel(vid); cancelled = True
                    eid = sess.submit(**extra)   # takes a slot once one frees up (possibly the victim's)
            else:
                g["final"] = (kind, res)
        with pytest.raises(_abi.Q3Error):
            sess.cancel(vid)                   # its final event was delivered
        with pytest.raises(_abi.Q3Error):
            sess.cancel(123456789)             # unknown
    assert got[vid]["order"].count(_abi.EV_CANCELLED) == 1 and got[vid]["order"][-1] == _abi.EV_CANCELLED
    assert len(got[vid]["chunks"]) == 1
    for w, rid in zip(want, [i for k, i in enumerate(ids) if k != victim] + [eid]):
        _check_done(got[rid], w)


def test_session_i16(tiny4):
    from q3tts import _abi, native
    cfg, eng, om, pe = tiny4
    reqs = _mixed(pe, 5)
    want = eng.generate_batch([dict(r, want_pcm=1) for r in reqs])
    with native.NativeSession(eng, _abi.PCM_I16) as sess:
        ids = [sess.submit(**r) for r in reqs]
        got = _collect(sess)
    for rid, w in zip(ids, want):
        pcm = np.concatenate([c for c, _ in got[rid]["chunks"]])
        assert pcm.dtype == np.int16 and np.array_equal(pcm, _i16(w.pcm))
        assert np.array_equal(got[rid]["final"][1].codes, w.codes)


def test_session_errors_and_engine_ownership(tiny4):
    from q3tts import _abi, native
    cfg, eng, om, pe = tiny4
    reqs = _mixed(pe, 4)
    before = eng.generate_batch([dict(r, want_pcm=1) for r in reqs])
    long_prompt = np.concatenate([pe] * (240 // pe.shape[0] + 1))[:240]
    bad = dict(embd=long_prompt, temperature=0.7, top_k=40, top_p=0.9, seed=5, max_steps=40, force_eos_at=4)   # prompt + max_steps > n_ctx
    sess = native.NativeSession(eng)
    try:
        ids = [sess.submit(**r) for r in reqs[:2]]
        bid = sess.submit(**bad)
        ids += [sess.submit(**r) for r in reqs[2:]]
        lib = eng.lib
        r, keep = eng.make_request(embd=pe, max_steps=4, want_pcm=1)
        res = (_abi.Result * 1)()
        assert lib.q3tts_generate_batch(eng.h, C.byref(r), 1, res) == -5
        assert b"session" in lib.q3tts_last_error(eng.h)
        h = C.c_void_p()
        assert lib.q3tts_stream_begin(eng.h, C.byref(r), C.byref(h)) == -5
        assert lib.q3tts_session_create(eng.h, 0, C.byref(h)) == -5
        assert lib.q3tts_k_probe(eng.h, 0) == -5
        got = _collect(sess)
        kind, res_bad = got[bid]["final"]
        assert kind == _abi.EV_FAILED and res_bad.status == -1 and not got[bid]["chunks"]
        for rid, w in zip(ids, before):
            _check_done(got[rid], w)
        # close with requests in flight
        for r in reqs:
            sess.submit(**r)
        ev = sess.next(60000)
        assert ev is not None
    finally:
        sess.close()
    with pytest.raises(_abi.Q3Error, match="closed"):
        sess.submit(**reqs[0])
    after = eng.generate_batch([dict(r, want_pcm=1) for r in reqs])
    for a, b in zip(before, after):
        assert np.array_equal(a.codes, b.codes) and np.array_equal(a.pcm.view(np.uint32), b.pcm.view(np.uint32))


def test_one_session_per_engine(tiny4):
    from q3tts import _abi, native
    cfg, eng, om, pe = tiny4
    sess = native.NativeSession(eng)
    lib, h = eng.lib, sess.h
    # a second handle on the same engine is refused while the first is open; after close, the engine takes a new one
    h2 = C.c_void_p()
    assert lib.q3tts_session_create(eng.h, 0, C.byref(h2)) == -5
    sess.close()
    sess2 = native.NativeSession(eng)
    rid = sess2.submit(embd=pe, temperature=0.0, max_steps=4)
    got = _collect(sess2)
    assert got[rid]["final"][0] == _abi.EV_DONE
    sess2.close()
    assert h is not None


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_k_pcm_pack_against_numpy(seed):
    from q3tts import native
    rng = np.random.default_rng(seed)
    rows, stride = 7, 4099   # odd stride: rows start at every 16-byte phase
    src = (rng.standard_normal((rows, stride)) * 0.7).astype(np.float32)
    src[0, :8] = [1.5, -1.5, 0.99999, -0.99999, 1.0, -1.0, 0.0, -0.0]
    ents, off = [], 0
    for j in range(int(rng.integers(1, 65))):
        row = int(rng.integers(0, rows))
        first = int(rng.integers(0, stride))
        count = 0 if j % 9 == 3 else int(rng.integers(0, min(stride - first, 3000) + 1))
        ents.append((row, first, count, off)); off += count + int(rng.integers(0, 3))
    ents.append((0, 0, 8, off)); off += 8
    for fmt in (0, 1):
        out = native.k_pcm_pack(src, ents, off, fmt)
        ref = np.zeros(off, dtype=np.float32)
        for row, first, count, d in ents:
            ref[d:d + count] = src[row, first:first + count]
        if fmt:
            assert out.dtype == np.int16 and np.array_equal(out, _i16(ref))
        else:
            assert np.array_equal(out.view(np.uint32), ref.view(np.uint32))


def test_session_full_shape_64_slots(oracle):
    """The benchmarked shape and batch: 80 sampled requests over 64 slots with the vocoder on; every one equals generate_batch bit for bit
    (chunks joined) and gets its first CHUNK before its DONE."""
    from q3tts import _abi, native
    cfg = _abi.full_config_py()
    cfg.max_batch, cfg.n_ctx, cfg.max_steps_cap = 64, 128, 32
    eng = native.NativeEngine(cfg)
    try:
        with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "speakers", "vivian.json")) as f:
            spk = np.asarray(json.load(f)["spk_emb"], dtype=np.float32)
        rng = np.random.default_rng(8080)
        reqs, keep_all = [], []
        for i in range(80):
            desc, keep = oracle.make_prompt_desc(rng.integers(0, 151643, size=int(rng.integers(2, 9))), spk_emb=spk)
            keep_all.append((desc, keep))
            target = 3 + (i * 5) % 14
            reqs.append(dict(desc=desc, temperature=0.7, top_k=40, top_p=0.9, seed=2000 + i, max_steps=20, min_frames=target, force_eos_at=target))
        want = eng.generate_batch([dict(r, want_pcm=1) for r in reqs])
        with native.NativeSession(eng) as sess:
            ids = [sess.submit(**r) for r in reqs]
            got = _collect(sess, 300000)
        for i, rid in enumerate(ids):
            g = got[rid]
            assert g["order"][0] == _abi.EV_CHUNK and g["order"][-1] == _abi.EV_DONE, i
            _check_done(g, want[i])
    finally:
        eng.close()

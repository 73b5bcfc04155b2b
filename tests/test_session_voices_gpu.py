"""Voices in a session (include/q3tts.h, "voices in a session"): prefix jobs, keep-voice requests, release and clone calls
while the batch runs.

The yardstick throughout is existing code: q3tts_prefix_create outside a session for the store's bytes, the whole-prompt path through
q3tts_generate_batch for every request's codes, hit_eos and PCM, and the out-of-session encoders for the clone call. Where a test needs
"every slot busy" it does not race the worker: two requests of 20 frames need five chunk boundaries, the session has four staging
buffers, so until the test reads events the fifth boundary waits with both slots occupied and whatever is submitted stays queued.
"""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N_CTX = 512


def _spk(d):
    return ((np.arange(d) % 13 - 6) * 0.03125).astype(np.float32)


def _bits_equal(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def _voices(cfg):
    """name -> voice fields of make_prompt_desc: a clone voice with instruct and ref_text, a spk_id voice with no language, a spk_emb voice."""
    rng = np.random.default_rng(77)
    m = cfg.model
    return {
        "clone": dict(spk_emb=_spk(m.d_embed), lang_id=2055, instruct_ids=rng.integers(0, 151643, size=5),
                      ref_codes=rng.integers(0, m.codecq_rows, size=(21, 16)), ref_text_ids=rng.integers(0, 151643, size=9)),
        "spk_id": dict(spk_id=3000, lang_id=None),
        "spk_emb": dict(spk_emb=_spk(m.d_embed) * 0.5),
    }


def _texts(n, lo=4, hi=24, seed=5):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 151643, size=int(rng.integers(lo, hi))) for _ in range(n)]


def _sampled(i, max_steps=20):
    target = 3 + (i * 5) % 13
    return dict(temperature=0.7, top_k=40, top_p=0.9, seed=300 + i, max_steps=max_steps, min_frames=target if i % 2 else 0,
                force_eos_at=target if i % 3 else -1)


def _long(i):
    """20 frames: five chunk boundaries"""
    return dict(temperature=0.7, top_k=40, top_p=0.9, seed=900 + i, max_steps=20, min_frames=20)


def _engine(max_batch=2, kv8=0, mode=0):
    from q3tts import _abi, native
    cfg = _abi.tiny_config(max_batch=max_batch, n_ctx=N_CTX, with_vocoder=1)
    cfg.kv_q8_0, cfg.talker_q8_0 = kv8, mode
    return cfg, native.NativeEngine(cfg)


def _read_store(x):
    """(K bytes, V bytes) of a ready prefix, padding included"""
    n = C.c_int64(0)
    assert x.lib.q3tts_k_prefix_read(x.h, None, None, 0, C.byref(n)) == 0 and n.value > 0
    k, v = np.empty(n.value, dtype=np.uint8), np.empty(n.value, dtype=np.uint8)
    assert x.lib.q3tts_k_prefix_read(x.h, k.ctypes.data_as(C.c_void_p), v.ctypes.data_as(C.c_void_p), n.value, C.byref(n)) == 0
    return k, v


class _Log:
    """Every event of a session in arrival order, and per id its chunks, its final event and its PREFIX event."""

    def __init__(self):
        self.order, self.ids = [], {}

    def add(self, ev):
        from q3tts import _abi
        rid, kind, pcm, fin, res = ev
        g = self.ids.setdefault(rid, dict(chunks=[], final=None, prefix=None))
        assert g["final"] is None, "an event after the final one"
        self.order.append((rid, kind))
        if kind == _abi.EV_CHUNK:
            g["chunks"].append(pcm)
        elif kind == _abi.EV_PREFIX:
            assert g["prefix"] is None, "two PREFIX events for one id"
            g["prefix"] = (res.status, fin)
            if fin:
                g["final"] = (kind, res)
        else:
            assert fin
            g["final"] = (kind, res)

    def drain(self, sess, timeout_ms=120000):
        for ev in sess.events(timeout_ms):
            self.add(ev)
        assert not sess._open, "events timed out"
        return self

    def until(self, sess, pred, timeout_ms=60000):
        while not pred(self):
            ev = sess.next(timeout_ms)
            assert ev is not None, "events timed out"
            self.add(ev)
        return self

    def first(self, rid, kind=None):
        return next(i for i, (r, k) in enumerate(self.order) if r == rid and (kind is None or k == kind))

    def check_done(self, rid, want, what):
        from q3tts import _abi
        g = self.ids[rid]
        kind, res = g["final"]
        assert kind == _abi.EV_DONE and res.status == 0, (what, kind, res.status)
        assert np.array_equal(res.codes, want.codes) and res.hit_eos == want.hit_eos, what
        assert _bits_equal(np.concatenate(g["chunks"]), want.pcm), what


# ---- 1. the store's bytes ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kv8,mode", [(0, 0), (1, 0), (0, 2)])
def test_store_bytes_equal_prefix_create(oracle, kv8, mode):
    """For P in {1, 63, 64, 65, 130} rows of one whole prompt: the store of q3tts_prefix_create, of an in-session prefix job and of an
    in-session keep-voice submit of the whole prompt with voice_rows = P are equal as bytes, K and V, padding included. At 63 and 65 the
    last key block of the slot holds the request's own keys behind P; 130 crosses two blocks. The jobs come after the requests, so they
    land in slots whose caches are not clean."""
    from q3tts import _abi, native
    cfg, eng = _engine(max_batch=4, kv8=kv8, mode=mode)
    try:
        desc, keep = oracle.make_prompt_desc(np.arange(1000, 1150), **_voices(cfg)["clone"])
        w = eng.build_prompt(desc)
        assert w.shape[0] > 131
        Ps = [1, 63, 64, 65, 130]
        a = [eng.create_prefix(embd=w[:P]) for P in Ps]
        want = [_read_store(x) for x in a]
        with native.NativeSession(eng) as sess:
            c = [sess.submit(embd=w, keep_voice=True, voice_rows=P, temperature=0.0, max_steps=4) for P in Ps]
            b = [sess.create_prefix(embd=w[:P]) for P in Ps]
            log = _Log().drain(sess)
        for (rid, x) in b:
            assert log.ids[rid]["prefix"] == (0, True) and log.ids[rid]["chunks"] == []
        for (rid, x) in c:
            assert log.ids[rid]["prefix"] == (0, False) and log.ids[rid]["final"][0] == _abi.EV_DONE
        for i, P in enumerate(Ps):
            for what, (rid, x) in (("job", b[i]), ("keep-voice", c[i])):
                assert x.state == 1 and x.n_rows == P, (what, P)
                k, v = _read_store(x)
                assert k.size == want[i][0].size and np.array_equal(k, want[i][0]), (what, P, "K")
                assert np.array_equal(v, want[i][1]), (what, P, "V")
                x.close()
        assert any(np.any(k) for k, v in want) and any(np.any(v) for k, v in want)
        for x in a:
            x.close()
    finally:
        eng.close()


@pytest.fixture(scope="module")
def tiny2(oracle):
    cfg, eng = _engine(max_batch=2)
    yield cfg, eng
    eng.close()


# ---- 2. results --------------------------------------------------------------------------------------------------------------------------
def test_results_equal_whole_prompts(oracle, tiny2):
    """Two plain requests stream on 2 slots; a keep-voice request in the clone voice and three requests naming its still-pending prefix
    arrive while they do, later a prefix job for a second voice with two requests behind it. Every request equals the same request as a
    whole prompt through generate_batch; the plain requests' chunks equal a run without any voice work; PREFIX precedes every chunk of a
    request that names the prefix; the desc form's rows equal the out-of-session prefix's."""
    from q3tts import _abi, native
    cfg, eng = tiny2
    vs = _voices(cfg)
    keep = []

    def descs(voice, t):
        dw, kw = oracle.make_prompt_desc(t, **voice)
        dt, kt = oracle.make_prompt_desc(t, part="text")
        keep.extend([dw, kw, dt, kt])
        return dw, dt

    texts = _texts(8, seed=41)
    plain = [dict(desc=descs(vs["spk_emb"], texts[i])[0], **_long(i)) for i in range(2)]
    cl = [descs(vs["clone"], texts[2 + i]) for i in range(4)]
    sp = [descs(vs["spk_id"], texts[6 + i]) for i in range(2)]
    whole = plain + [dict(desc=dw, **_sampled(i)) for i, (dw, dt) in enumerate(cl)] + [dict(desc=dw, **_sampled(7 + i)) for i, (dw, dt) in enumerate(sp)]
    want = eng.generate_batch([dict(r, want_pcm=1) for r in whole])
    rows = {}
    for name in ("clone", "spk_id"):
        dv, kv = oracle.make_prompt_desc(None, part="voice", **vs[name])
        keep.extend([dv, kv])
        with eng.create_prefix(desc=dv) as x:
            rows[name] = x.n_rows
    dv2, kv2 = oracle.make_prompt_desc(None, part="voice", **vs["spk_id"])
    with native.NativeSession(eng) as sess:   # the run without voice work
        pid = [sess.submit(**r) for r in plain]
        base = _Log().drain(sess)
    with native.NativeSession(eng) as sess:
        ids = [sess.submit(**r) for r in plain]
        log = _Log().until(sess, lambda L: any(k == _abi.EV_CHUNK for _, k in L.order))
        kid, x = sess.submit(desc=cl[0][0], keep_voice=True, **_sampled(0))
        assert x.state in (0, 1) and (x.state == 1 or x.n_rows == 0)
        ids.append(kid)
        ids += [sess.submit(desc=cl[i][1], prefix=x, **_sampled(i)) for i in (1, 2, 3)]
        log.until(sess, lambda L: L.ids.get(kid, {}).get("prefix") is not None)
        jid, x2 = sess.create_prefix(desc=dv2)
        ids += [sess.submit(desc=sp[i][1], prefix=x2, **_sampled(7 + i)) for i in range(2)]
        log.drain(sess)
        assert x.state == 1 and x.n_rows == rows["clone"] and x2.state == 1 and x2.n_rows == rows["spk_id"]
        x.close(); x2.close()
    assert log.ids[kid]["prefix"] == (0, False) and log.ids[jid]["prefix"] == (0, True)
    for i, rid in enumerate(ids):
        log.check_done(rid, want[i], i)
    for i in range(2):
        assert len(log.ids[ids[i]]["chunks"]) == len(base.ids[pid[i]]["chunks"])
        for g, b in zip(log.ids[ids[i]]["chunks"], base.ids[pid[i]]["chunks"]):
            assert _bits_equal(g, b), i
    for follower in ids[3:6]:
        assert log.first(kid, _abi.EV_PREFIX) < log.first(follower, _abi.EV_CHUNK)
    for follower in ids[6:8]:
        assert log.first(jid, _abi.EV_PREFIX) < log.first(follower, _abi.EV_CHUNK)


# ---- 3. jobs under pressure ----------------------------------------------------------------------------------------------------------------
def test_job_waits_its_turn(oracle, tiny2):
    """Both slots busy and two requests queued: a prefix job behind them is admitted after them (its PREFIX follows the first chunk of the
    request two places ahead of it: two slots admit at most two entries per boundary), the request behind it after the job; all complete."""
    from q3tts import _abi, native
    cfg, eng = tiny2
    v = _voices(cfg)["spk_emb"]
    keep = []
    texts = _texts(5, seed=58)
    dws = []
    for t in texts:
        dw, kw = oracle.make_prompt_desc(t, **v)
        keep.extend([dw, kw])
        dws.append(dw)
    dt, kt = oracle.make_prompt_desc(texts[4], part="text")
    dv, kv = oracle.make_prompt_desc(None, part="voice", **v)
    reqs = [dict(desc=dws[i], **_long(i)) for i in range(2)] + [dict(desc=dws[i], **_sampled(i)) for i in (2, 3, 4)]
    want = eng.generate_batch([dict(r, want_pcm=1) for r in reqs])
    with native.NativeSession(eng) as sess:
        ids = [sess.submit(**r) for r in reqs[:4]]   # two run (and wait for the reader at their fifth boundary), two queue
        jid, x = sess.create_prefix(desc=dv)
        ids.append(sess.submit(desc=dt, prefix=x, **_sampled(4)))
        assert x.state == 0
        log = _Log().drain(sess)
        x.close()
    assert log.ids[jid]["prefix"] == (0, True)
    for i, rid in enumerate(ids):
        log.check_done(rid, want[i], i)
    assert log.first(ids[2], _abi.EV_CHUNK) < log.first(jid, _abi.EV_PREFIX) < log.first(ids[4], _abi.EV_CHUNK)
    assert log.first(ids[0]) < log.first(ids[2]) and log.first(ids[1]) < log.first(ids[3])


# ---- 4. clone in a session ---------------------------------------------------------------------------------------------------------------
def _clip(n, rate, seed):
    rng = np.random.default_rng(seed)
    t = np.arange(n, dtype=np.float64) / rate
    ph = 2 * np.pi * np.cumsum(120.0 + 30.0 * np.sin(2 * np.pi * 1.3 * t)) / rate
    x = sum(np.sin(k * ph) / k for k in range(1, 6)) * 0.2 + rng.standard_normal(n) * 0.02
    return np.clip(x, -1, 1).astype(np.float32)


def test_clone_in_a_session(oracle):
    """clone_voice on a 0.5 s clip while two requests stream: codes and speaker embedding equal audio_encode / speaker_encode taken
    before the session opened, at 16 kHz the out-of-session resample followed by the encoders; the streams' PCM is unchanged."""
    from q3tts import _abi, native
    cfg, eng = _engine(max_batch=2)
    try:
        lib = eng.lib
        a24, a16 = _clip(12000, 24000, 4), _clip(8000, 16000, 5)
        d, kd = oracle.make_prompt_desc(_texts(1, seed=3)[0], **_voices(cfg)["spk_emb"])
        reqs = [dict(desc=d, **_long(i)) for i in range(2)]
        with native.NativeSession(eng) as sess:   # before q3tts_clone_init: the usual refusal
            with pytest.raises(_abi.Q3Error, match=r"\(-5\).*not loaded"):
                sess.clone_voice(a24)
        eng.clone_init(_abi.tiny_clone_config(cfg.model.d_embed))
        want = eng.generate_batch([dict(r, want_pcm=1) for r in reqs])
        c24, s24 = eng.audio_encode(a24), eng.speaker_encode(a24)
        r16 = eng.resample(a16, 16000, 24000)
        c16, s16 = eng.audio_encode(r16), eng.speaker_encode(r16)
        assert c24.shape[0] > 0 and c16.shape[0] > 0 and np.abs(s24).max() > 0
        with native.NativeSession(eng) as sess:
            ids = [sess.submit(**r) for r in reqs]
            log = _Log().until(sess, lambda L: any(k == _abi.EV_CHUNK for _, k in L.order))
            g24 = sess.clone_voice(a24)
            g16 = sess.clone_voice(a16, rate=16000)
            n = C.c_int32(0)   # either output may be NULL
            spk = np.zeros_like(s24)
            assert lib.q3tts_session_clone(sess.h, a24.ctypes.data_as(C.POINTER(C.c_float)), a24.size, 24000, None, 0, C.byref(n),
                                           spk.ctypes.data_as(C.POINTER(C.c_float))) == 0
            assert lib.q3tts_clone_audio_encode(eng.h, None, 0, None, 0, C.byref(n)) == -5
            log.drain(sess)
        assert np.array_equal(g24[0], c24) and _bits_equal(g24[1], s24) and _bits_equal(spk, s24)
        assert np.array_equal(g16[0], c16) and _bits_equal(g16[1], s16)
        for i, rid in enumerate(ids):
            log.check_done(rid, want[i], i)
    finally:
        eng.close()


# ---- 5. lifetime and errors --------------------------------------------------------------------------------------------------------------
def test_lifetime_and_errors(oracle, tiny2):
    from q3tts import _abi, native
    cfg, eng = tiny2
    lib = eng.lib
    vs = _voices(cfg)
    v = vs["clone"]
    keep = []
    texts = _texts(4, seed=23)
    pairs = []
    for t in texts:
        dw, kw = oracle.make_prompt_desc(t, **v)
        dt, kt = oracle.make_prompt_desc(t, part="text")
        keep.extend([dw, kw, dt, kt])
        pairs.append((dw, dt))
    dv, kv = oracle.make_prompt_desc(None, part="voice", **v)
    busy = [dict(desc=pairs[i][0], **_long(i)) for i in range(2)]
    whole = busy + [dict(desc=pairs[2][0], **_sampled(2)), dict(desc=pairs[3][0], **_sampled(3))]
    want = eng.generate_batch([dict(r, want_pcm=1) for r in whole])
    with eng.create_prefix(desc=dv) as x0:
        P, store = x0.n_rows, _read_store(x0)[0].size
    b0 = eng.device_bytes()

    # release while a queued request names the prefix; submit after release; refused combinations; the old calls stay refused
    with native.NativeSession(eng) as sess:
        jid, x = sess.create_prefix(desc=dv)
        log = _Log().until(sess, lambda L: jid in L.ids)
        assert log.ids[jid]["prefix"] == (0, True) and x.state == 1 and x.n_rows == P
        b1 = eng.device_bytes()
        assert b1 - b0 == 2 * store
        ids = [sess.submit(**r) for r in busy]
        f = sess.submit(desc=pairs[2][1], prefix=x, **_sampled(2))          # queued: both slots stay busy until events are read
        xh = x.h
        sess.release_prefix(x)
        r, k = native.NativeEngine.make_request(desc=pairs[3][1], **_sampled(3))
        r.prefix = xh
        rid = C.c_uint64(0)
        assert lib.q3tts_session_submit(sess.h, C.byref(r), C.byref(rid)) == -1
        assert b"released" in lib.q3tts_session_last_error(sess.h)
        assert lib.q3tts_session_prefix_release(sess.h, xh) == -1
        log.drain(sess)
        for i, q in enumerate(ids + [f]):
            log.check_done(q, want[i], i)
        h = C.c_void_p()
        assert lib.q3tts_prefix_create(eng.h, C.byref(dv), None, 0, C.byref(h)) == -5 and not h.value
    assert eng.device_bytes() == b0   # the store went when its last queued request had been admitted

    with eng.create_prefix(desc=dv) as xo:
        with native.NativeSession(eng) as sess:
            assert lib.q3tts_prefix_destroy(xo.h) == -5
            with pytest.raises(_abi.Q3Error, match=r"\(-1\)"):              # keep-voice together with req->prefix
                sess.submit(desc=pairs[2][1], prefix=xo, keep_voice=True, **_sampled(2))
            with pytest.raises(_abi.Q3Error, match=r"\(-1\)"):              # prompt_embd without its voice rows
                sess.submit(embd=np.zeros((8, cfg.model.d_embed), np.float32), keep_voice=True, **_sampled(2))

    # a job of n_tok >= n_ctx: PREFIX with INVALID, the request naming it FAILED; an oversized keep-voice request fails both its events
    with native.NativeSession(eng) as sess:
        jid, xb = sess.create_prefix(embd=np.zeros((N_CTX, cfg.model.d_embed), np.float32))
        fb = sess.submit(desc=pairs[2][1], prefix=xb, **_sampled(2))
        long_t = np.arange(N_CTX - P - 3 - 10, dtype=np.uint32) % 151643
        dl, kl = oracle.make_prompt_desc(long_t, **v)
        keep.extend([dl, kl])
        kid, xk = sess.submit(desc=dl, keep_voice=True, **_sampled(3))
        ok = sess.submit(**whole[3])
        log = _Log().drain(sess)
        assert log.ids[jid]["prefix"] == (-1, True) and xb.state == -1 and xb.n_rows == 0
        assert log.ids[fb]["final"][0] == _abi.EV_FAILED and log.ids[fb]["final"][1].status == -1 and not log.ids[fb]["chunks"]
        assert log.ids[kid]["prefix"] == (-1, False) and log.ids[kid]["final"][0] == _abi.EV_FAILED and xk.state == -1
        assert log.first(kid, _abi.EV_PREFIX) < log.first(kid, _abi.EV_FAILED)
        log.check_done(ok, want[3], "beside the failures")
        sess.release_prefix(xb)
        sess.release_prefix(xk)

    # a keep-voice request cancelled before admission: a failed handle that still releases
    with native.NativeSession(eng) as sess:
        ids = [sess.submit(**r) for r in busy]
        kid, xk = sess.submit(desc=pairs[2][0], keep_voice=True, **_sampled(2))
        sess.cancel(kid)
        assert xk.state == -5
        log = _Log().drain(sess)
        assert log.ids[kid]["prefix"] == (-5, False) and log.ids[kid]["final"][0] == _abi.EV_CANCELLED
        for i, q in enumerate(ids):
            log.check_done(q, want[i], i)
        sess.release_prefix(xk)

    # close with a pending job: the handle reads failed and q3tts_prefix_destroy takes it; a ready prefix outlives the session
    sess = native.NativeSession(eng)
    j0, xr = sess.create_prefix(desc=dv)
    log = _Log().until(sess, lambda L: j0 in L.ids)
    ids = [sess.submit(**r) for r in busy]
    j1, xp = sess.create_prefix(desc=dv)
    assert xp.state == 0
    sess.close()
    assert xp.state == -5 and xp.n_rows == 0 and xr.state == 1 and xr.n_rows == P
    xp.close()
    got = eng.generate_batch([dict(desc=pairs[2][1], prefix=xr, want_pcm=1, **_sampled(2))])[0]
    assert got.status == 0 and np.array_equal(got.codes, want[2].codes) and _bits_equal(got.pcm, want[2].pcm)
    xr.close()


# ---- 6. the reference-style API ----------------------------------------------------------------------------------------------------------
def test_api_prefix_auto():
    """stream_batch_with_voice(texts, [voice] * 5, prefix="auto") yields the same chunks, bit for bit, as the call without it."""
    from q3tts import _abi, api
    cfg = _abi.tiny_config(max_batch=4, n_ctx=256, with_vocoder=1)
    eng = api.TtsEngine(cfg)
    try:
        eng.set_max_steps(12)
        eng.set_sampler_config(api.SamplerConfig(temperature=0.7, top_k=40, top_p=0.9, seed=11))
        rng = np.random.default_rng(31)
        voice = api.VoiceFile.new([int(i) for i in rng.integers(0, 151643, size=6)], [int(c) for c in rng.integers(0, 64, size=12 * 16)],
                                  _spk(cfg.model.d_embed).tolist())
        ins = [5, 6, 7]
        texts = [list(t) for t in _texts(5, seed=31)]
        seeds = [40 + i for i in range(5)]

        def run(**kw):
            parts = {}
            for i, pcm, fin in eng.stream_batch_with_voice(texts, [voice] * 5, [ins] * 5, seeds, **kw):
                parts.setdefault(i, []).append(pcm)
            return parts

        want, got = run(), run(prefix="auto")
        assert sorted(got) == sorted(want) == list(range(5))
        for i in range(5):
            assert len(got[i]) == len(want[i]), i
            for g, w in zip(got[i], want[i]):
                assert _bits_equal(g, w), i
        with pytest.raises(ValueError):
            list(eng.stream_batch_with_voice(texts[:1], [voice], [ins], prefix="automatic"))
    finally:
        eng.close()

"""Streamed text input on the device (include/q3tts.h, "streaming text input"): codes and hit_eos against the CPU restatement
tests/_text_stream.py with `==`, PCM bit for bit between the engine's own paths. tests/test_text_stream_cpu.py pins the restatement to the
oracle and asserts that the whole-text layout (or tts_pad on every feedback row) cannot pass the cases below. Tiny shape: 4 slots,
n_ctx 256, at most 16 frames per request."""
import ctypes as C
import threading

import numpy as np
import pytest

import _text_stream as TS

pytestmark = pytest.mark.gpu
INVALID = -1   # Q3TTS_ERR_INVALID
WAIT_MS, QUIET_MS = 60000, 200   # an event that must come | a pause in which none may


def _engine(cfg):
    from q3tts import native
    return native.NativeEngine(cfg)


class Env:
    """One engine (with vocoder) and oracle per module; CPU references are computed once per (text, talker, Predictor sampler)."""

    def __init__(self, oracle, talker_q8=0):
        self.cfg = TS.tiny_cfg(with_vocoder=1, talker_q8=talker_q8)
        self.eng = _engine(self.cfg)
        self.om = oracle.OracleModel(self.cfg.model, seed=0, n_ctx=TS.N_CTX, n_threads=8)
        if talker_q8 == 2:
            self.om.set_talker_q8a8()
        self.pred = TS.mats_from_model(self.om, False, False)
        self.d = self.cfg.model.d_embed
        self._refs, self._one = {}, {}

    def close(self):
        self.eng.close()
        self.om.close()

    def ref(self, ids, kw, pred_sampler=(0.0, 0, 1.0)):
        key = (tuple(int(i) for i in ids), tuple(sorted(kw.items())), pred_sampler)
        if key not in self._refs:
            rows, T = TS.prompt(self.om, ids)
            self._refs[key] = TS.generate(self.om, self.pred, rows, T, pred_sampler=pred_sampler, **kw)
        return self._refs[key]

    def stream_kw(self, ids, **kw):
        desc, keep = TS.stream_desc(ids, self.d)
        return dict(desc=desc, text_stream=True, **kw), keep

    def one_shot(self, name, talker):
        """Case 1's engine result with PCM (checked against the reference by test_one_shot), shared by the session tests."""
        key = (name, talker)
        if key not in self._one:
            kw, keep = self.stream_kw(TS.TEXTS[name], want_pcm=1, **TS.request(talker))
            self._one[key] = self.eng.generate(**kw)
        return self._one[key]


@pytest.fixture(scope="module")
def env(oracle):
    e = Env(oracle)
    yield e
    e.close()


def _i16(pcm):
    return np.trunc(np.clip(pcm * np.float32(32767), -32768, 32767)).astype(np.int16)


def _joined(chunks, dtype):
    return np.concatenate([c for c in chunks]) if chunks else np.zeros(0, dtype=dtype)


def _same_pcm(got, want_f32, i16):
    want = _i16(want_f32) if i16 else want_f32
    return got.dtype == want.dtype and got.size == want.size and np.array_equal(got.view(np.uint8), want.view(np.uint8))


# ---- 1. one-shot: closed text through q3tts_generate ----------------------------------------------------------------------------------
@pytest.mark.parametrize("talker", sorted(TS.TALKERS))
@pytest.mark.parametrize("name", sorted(TS.TEXTS))
def test_one_shot(env, name, talker):
    ids = TS.TEXTS[name]
    ref, ref_eos = env.ref(ids, TS.request(talker))
    got = env.one_shot(name, talker)
    assert got.status == 0 and ref.shape[0] == TS.FRAMES
    assert np.array_equal(got.codes, ref) and got.hit_eos == ref_eos
    assert got.pcm is not None and got.pcm.size > 0


# ---- 2. the other consumers of the last pass: a W8A8 Talker, the sampling instantiation -------------------------------------------------
def test_w8a8_talker(oracle):
    e = Env(oracle, talker_q8=2)
    try:
        ids, kw = TS.TEXTS["n6"], TS.request("sampled")
        ref, ref_eos = e.ref(ids, kw)
        skw, keep = e.stream_kw(ids, **kw)
        got = e.eng.generate(**skw)
        assert got.status == 0 and np.array_equal(got.codes, ref) and got.hit_eos == ref_eos
    finally:
        e.close()


def test_sampling_predictor(env):
    ids, kw = TS.TEXTS["n6"], TS.request("sampled")
    ref, ref_eos = env.ref(ids, kw, TS.PRED_SAMPLER)
    plain, _ = env.ref(ids, kw)
    skw, keep = env.stream_kw(ids, **kw)
    env.eng.set_predictor_sampler(*TS.PRED_SAMPLER)
    try:
        got = env.eng.generate(**skw)
    finally:
        env.eng.set_predictor_sampler(0.0, 0, 1.0)
    assert got.status == 0 and np.array_equal(got.codes, ref) and got.hit_eos == ref_eos and not np.array_equal(ref, plain)
    assert np.array_equal(env.eng.generate(**skw).codes, plain)   # and back on the argmax form's own text sets


# ---- 3. streamed and whole-text requests in one batch, slots refilled -----------------------------------------------------------------
def test_mixed_batch(env, oracle):
    reqs = TS.batch_requests()
    kws, keep, refs = [], [], []
    for r in reqs:
        if r["stream"]:
            kw, k = env.stream_kw(r["ids"], **r["kw"])
            refs.append(env.ref(r["ids"], r["kw"]))
        else:
            desc, k = TS.stream_desc(r["ids"], env.d)   # the same desc, text_stream = 0: the whole text in the prompt
            kw = dict(desc=desc, **r["kw"])
            refs.append(env.om.generate(TS.whole_prompt(env.om, r["ids"]), **r["kw"]))
        kws.append(kw); keep.append(k)
    assert len(reqs) == 7 and env.cfg.max_batch == 4 and any(r["stream"] for r in reqs) and not all(r["stream"] for r in reqs)
    outs = env.eng.generate_batch(kws)
    for i, (o, (ref, ref_eos)) in enumerate(zip(outs, refs)):
        assert o.status == 0 and np.array_equal(o.codes, ref) and o.hit_eos == ref_eos, i
    whole_only = [kw for kw, r in zip(kws, reqs) if not r["stream"]]   # afterwards the default frame step serves as before
    for o, (ref, _) in zip(env.eng.generate_batch(whole_only), [f for f, r in zip(refs, reqs) if not r["stream"]]):
        assert np.array_equal(o.codes, ref)


# ---- sessions --------------------------------------------------------------------------------------------------------------------------
def _next(sess, timeout_ms=WAIT_MS):
    ev = sess.next(timeout_ms)
    assert ev is not None, "no event"
    return ev


def _drain(sess, rid, chunks):
    """Events of rid up to its final one; chunks of rid are appended. Returns (kind, result) of the final event."""
    from q3tts import _abi
    while True:
        r, kind, pcm, fin, res = _next(sess)
        assert r == rid
        if kind == _abi.EV_CHUNK:
            chunks.append(pcm)
        else:
            return kind, res


# ---- 4. text fed piece by piece equals the whole text at submission --------------------------------------------------------------------
@pytest.mark.parametrize("i16", [False, True], ids=["f32", "i16"])
def test_incremental_feed_equals_whole_text(env, i16):
    from q3tts import _abi, native
    ids = TS.TEXTS["n6"]
    want = env.one_shot("n6", "sampled")
    spf = want.pcm.size // TS.FRAMES
    kw, keep = env.stream_kw(ids[:1], **TS.request("sampled"))
    with native.NativeSession(env.eng, _abi.PCM_I16 if i16 else _abi.PCM_F32) as sess:
        rid = sess.submit(text_open=True, **kw)
        assert sess.next(QUIET_MS) is None                      # one id, open: nothing can run
        sess.append_text(rid, ids[1:5])
        r, kind, pcm, fin, res = _next(sess)                    # len(T) = 4: frames 0..3 and no further
        assert (r, kind, fin) == (rid, _abi.EV_CHUNK, False) and pcm.size == 4 * spf
        assert sess.next(QUIET_MS) is None
        chunks = [pcm]
        sess.append_text(rid, ids[5:], close=True)
        kind, res = _drain(sess, rid, chunks)
    assert kind == _abi.EV_DONE and res.status == 0
    assert np.array_equal(res.codes, want.codes) and res.hit_eos == want.hit_eos
    assert _same_pcm(_joined(chunks, want.pcm.dtype), want.pcm, i16)


# ---- 5. parked while the batch around it changes ---------------------------------------------------------------------------------------
def test_parked_under_a_full_bucket(env):
    from q3tts import _abi, native
    ids = TS.TEXTS["n40"]
    want = env.one_shot("n40", "sampled")
    frames = [4, 8, 12, 8]   # three neighbours, then a fourth into the first freed slot
    nb = []
    for i, t in enumerate(frames):
        desc, k = TS.stream_desc(np.arange(700 + 10 * i, 705 + 12 * i), env.d)
        nb.append((dict(desc=desc, temperature=0.7, top_k=40, top_p=0.9, seed=500 + i, max_steps=16, min_frames=t, force_eos_at=t), k))
    nb_want = env.eng.generate_batch([dict(kw, want_pcm=1) for kw, _ in nb])
    kw, keep = env.stream_kw(ids[:5], **TS.request("sampled"))
    chunks, got = [], {}
    with native.NativeSession(env.eng) as sess:
        rid = sess.submit(text_open=True, **kw)                 # len(T) = 4: one chunk, then parked
        r, kind, pcm, fin, res = _next(sess)
        assert (r, kind, fin) == (rid, _abi.EV_CHUNK, False)
        chunks.append(pcm)
        assert sess.next(QUIET_MS) is None
        nids = [sess.submit(**k) for k, _ in nb[:3]]            # a full bucket of 4 slots, one of them parked
        nids.append(sess.submit(**nb[3][0]))                    # waits for a slot: the row plan changes when it gets one
        open_ids = set(nids)
        while open_ids:
            r, kind, pcm, fin, res = _next(sess)
            assert r in open_ids, "the parked request produced an event"
            g = got.setdefault(r, dict(chunks=[], res=None))
            if kind == _abi.EV_CHUNK:
                g["chunks"].append(pcm)
            else:
                assert kind == _abi.EV_DONE
                g["res"] = res; open_ids.discard(r)
        assert sess.next(QUIET_MS) is None                      # still parked
        sess.append_text(rid, ids[5:], close=True)
        kind, res = _drain(sess, rid, chunks)
    assert kind == _abi.EV_DONE and np.array_equal(res.codes, want.codes) and res.hit_eos == want.hit_eos
    assert _same_pcm(_joined(chunks, np.float32), want.pcm, False)
    for i, nid in enumerate(nids):
        assert np.array_equal(got[nid]["res"].codes, nb_want[i].codes) and got[nid]["res"].codes.shape[0] == frames[i], i
        assert _same_pcm(_joined(got[nid]["chunks"], np.float32), nb_want[i].pcm, False), i


# ---- 6. a parked request can be cancelled, and closed over -----------------------------------------------------------------------------
def test_cancel_and_close_while_parked(env):
    from q3tts import _abi, native
    ids = TS.TEXTS["n40"]
    kw, keep = env.stream_kw(ids[:5], **TS.request("greedy"))
    sess = native.NativeSession(env.eng)
    try:
        rid = sess.submit(text_open=True, **kw)
        r, kind, pcm, fin, res = _next(sess)
        assert (r, kind) == (rid, _abi.EV_CHUNK)
        assert sess.next(QUIET_MS) is None                      # parked
        sess.cancel(rid)
        r, kind, pcm, fin, res = _next(sess)
        assert (r, kind) == (rid, _abi.EV_CANCELLED)
        assert sess.next(QUIET_MS) is None                      # and no further chunk
        with pytest.raises(_abi.Q3Error):
            sess.append_text(rid, ids[5:9])
        rid2 = sess.submit(text_open=True, **kw)                # parked again, and left open
        r, kind, pcm, fin, res = _next(sess)
        assert (r, kind) == (rid2, _abi.EV_CHUNK)
        assert sess.next(QUIET_MS) is None
    finally:
        th = threading.Thread(target=sess.close, daemon=True)   # the close must not wait for text that never comes
        th.start()
        th.join(30)
    assert not th.is_alive(), "q3tts_session_close hangs on a parked request"
    ref = env.one_shot("n40", "greedy")                          # the engine serves q3tts_generate as before
    skw, keep2 = env.stream_kw(ids, **TS.request("greedy"))
    assert np.array_equal(env.eng.generate(**skw).codes, ref.codes)
    desc, k = TS.stream_desc(ids, env.d)
    whole, _ = env.om.generate(TS.whole_prompt(env.om, ids), **TS.request("greedy"))
    assert np.array_equal(env.eng.generate(desc=desc, **TS.request("greedy")).codes, whole)


# ---- 7. behind a voice prefix ----------------------------------------------------------------------------------------------------------
def test_prefix_plus_streamed_text(env):
    from q3tts import native
    ids = TS.TEXTS["n6"]
    want = env.one_shot("n6", "sampled")
    vdesc, vk = native.make_prompt_desc(None, spk_emb=TS.S.spk(env.d), part="voice")
    tdesc, tk = native.make_prompt_desc(ids, part="text")
    with env.eng.create_prefix(desc=vdesc) as px:
        got = env.eng.generate(desc=tdesc, prefix=px, text_stream=True, want_pcm=1, **TS.request("sampled"))
    assert got.status == 0 and np.array_equal(got.codes, want.codes) and _same_pcm(got.pcm, want.pcm, False)


# ---- 8. refusals -----------------------------------------------------------------------------------------------------------------------
def test_refusals(env):
    from q3tts import _abi, native
    eng, ids = env.eng, TS.TEXTS["n6"]
    kw, keep = env.stream_kw(ids, **TS.request("greedy"))
    pe = TS.whole_prompt(env.om, ids)

    def refused(fn, *words):
        with pytest.raises(_abi.Q3Error) as ex:
            fn()
        msg = str(ex.value)
        assert f"({INVALID})" in msg and all(w in msg for w in words), msg

    def status(**k):   # q3tts_generate returns the request's status with the engine's message
        r, kp = eng.make_request(**k)
        res = _abi.Result()
        rc = eng.lib.q3tts_generate(eng.h, C.byref(r), C.byref(res))
        eng.lib.q3tts_result_free(C.byref(res))
        return rc, eng.lib.q3tts_last_error(eng.h).decode()
    rc, msg = status(embd=pe, text_stream=True, max_steps=4)
    assert rc == INVALID and "prompt_embd" in msg
    desc0, k0 = TS.stream_desc(np.zeros(0, dtype=np.uint32), env.d)
    rc, msg = status(desc=desc0, text_stream=True, max_steps=4)
    assert rc == INVALID and "n_text" in msg
    rc, msg = status(text_open=True, **kw)
    assert rc == INVALID and "text_open" in msg
    refused(lambda: eng.generate_batch([dict(kw, text_open=True)]), "text_open")
    refused(lambda: list(native.stream_chunks(eng, **dict(kw, text_open=True, want_pcm=1))), "text_open")
    with native.NativeSession(eng) as sess:
        refused(lambda: sess.submit(embd=pe, text_stream=True), "prompt_embd")
        refused(lambda: sess.submit(desc=desc0, text_stream=True), "n_text")
        refused(lambda: sess.append_text(12345, ids), "unknown id")
        whole = sess.submit(desc=kw["desc"], **TS.request("greedy"))
        refused(lambda: sess.append_text(whole, ids), "without text_stream")
        closed = sess.submit(**kw)
        refused(lambda: sess.append_text(closed, ids), "closed")
        rc = sess.lib.q3tts_session_append_text(sess.h, closed, None, 3, 0)
        assert rc == INVALID and b"ids missing" in sess.lib.q3tts_session_last_error(sess.h)
        for _ in sess.events(WAIT_MS):
            pass
        refused(lambda: sess.append_text(closed, ids), "unknown id")   # finished
    node = native.NativeNode(TS.tiny_cfg(max_batch=1), [0])
    try:
        refused(lambda: node.generate_batch([kw]), "text_stream")
    finally:
        node.close()


# ---- the streaming ABI and the reference-style API ---------------------------------------------------------------------------------------
def test_stream_abi_takes_closed_streamed_text(env):
    from q3tts import native
    want = env.one_shot("n6", "sampled")
    kw, keep = env.stream_kw(TS.TEXTS["n6"], want_pcm=1, **TS.request("sampled"))
    chunks = [c for c, _ in native.stream_chunks(env.eng, **kw)]
    assert _same_pcm(_joined(chunks, np.float32), want.pcm, False)


def test_api_stream_text_with_voice():
    """TtsEngine.stream_text_with_voice: pieces (id lists) fed from its helper thread give the audio of the same ids submitted closed."""
    from q3tts import _abi, api
    cfg = TS.tiny_cfg(with_vocoder=1)
    eng = api.TtsEngine(cfg)
    try:
        eng.set_max_steps(12)
        eng.set_sampler_config(api.SamplerConfig(temperature=0.7, top_k=40, top_p=0.9, seed=21))
        voice = api.VoiceFile.new("", [], TS.S.spk(cfg.model.d_embed).tolist())
        ids = [int(i) for i in TS.TEXTS["n40"][:14]]
        pieces = [ids[:1], [], ids[1:4], ids[4:5], ids[5:11], ids[11:]]
        desc, keep = eng._desc(ids, voice, None)
        want = eng._native.generate(desc=desc, temperature=0.7, top_k=40, top_p=0.9, seed=21, max_steps=12, want_pcm=1, text_stream=True)
        got = list(eng.stream_text_with_voice(iter(pieces), voice))
        assert got and got[-1][1] and not any(f for _, f in got[:-1])
        assert want.status == 0 and _same_pcm(_joined([c for c, _ in got], np.float32), want.pcm, False)
        with eng.voice_prefix(voice) as x:
            again = list(eng.stream_text_with_voice(iter(pieces), voice, prefix=x))
        assert _same_pcm(_joined([c for c, _ in again], np.float32), want.pcm, False)
        with pytest.raises(ValueError):
            list(eng.stream_text_with_voice(iter([[], []]), voice))
    finally:
        eng.close()

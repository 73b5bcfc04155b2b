"""Paced requests and swapping on the device (include/q3tts.h, "paced requests and swapping"). The contract: for any
schedule of grants, text arrivals, swap-outs and swap-ins a request's events are those of the same request submitted plainly — the same
chunk sizes in the same order, the chunks joined equal to q3tts_generate_batch's PCM bit for bit, the same codes, n_frames and hit_eos.
Each reference is the engine's own generate_batch (and, for chunk sizes, the same requests through a plain session). Tests 2-7 assert
swap counters > 0, so none passes with swapping silently off. Tiny shape: 2 slots, n_ctx 256, max_steps_cap 64, vocoder window 8."""
import ctypes as C
import threading
from collections import defaultdict

import numpy as np
import pytest

import _text_stream as TS

pytestmark = pytest.mark.gpu
INVALID, STATE = -1, -5   # Q3TTS_ERR_INVALID, Q3TTS_ERR_STATE
WAIT_MS, QUIET_MS = 60000, 200   # an event that must come | a pause in which none may
ARENA = 32 << 20


def _cfg(**over):
    cfg = TS.tiny_cfg(max_batch=2, with_vocoder=1)
    for k, v in over.items():
        if k.startswith("voc_"):
            setattr(cfg.vocoder, k[4:], v)
        else:
            setattr(cfg, k, v)
    return cfg


def _engine(cfg):
    from q3tts import native
    return native.NativeEngine(cfg)


@pytest.fixture(scope="module")
def eng():
    e = _engine(_cfg())
    yield e
    e.close()


def _req(eng, i, frames, n_text=6):
    """Whole-text request i of exactly `frames` frames (forced as the session tests force them), sampled."""
    desc, keep = TS.stream_desc(np.arange(400 + 31 * i, 400 + 31 * i + n_text), eng.cfg.model.d_embed)
    return dict(desc=desc, temperature=0.7, top_k=40, top_p=0.9, seed=900 + i, max_steps=min(64, frames + 8), min_frames=frames,
                force_eos_at=frames), keep


def _i16(pcm):
    return np.trunc(np.clip(pcm * np.float32(32767), -32768, 32767)).astype(np.int16)


def _same_pcm(got, want):
    return got.dtype == want.dtype and got.size == want.size and np.array_equal(got.view(np.uint8), want.view(np.uint8))


class Col:
    """Collects a session's events per id."""

    def __init__(self, sess):
        self.sess, self.chunks, self.fin = sess, defaultdict(list), {}

    def take(self, timeout_ms=WAIT_MS):
        from q3tts import _abi
        ev = self.sess.next(timeout_ms)
        if ev is None:
            return None
        rid, kind, pcm, fin, res = ev
        if kind == _abi.EV_CHUNK:
            self.chunks[rid].append(pcm)
        elif kind != _abi.EV_PREFIX:
            assert rid not in self.fin, "a second final event"
            self.fin[rid] = (kind, res)
        return ev

    def until(self, done):
        while not done():
            assert self.take() is not None, "no event"

    def quiet(self):
        """Everything that can run has run: events until a pause of QUIET_MS."""
        while self.take(QUIET_MS) is not None:
            pass

    def n(self, rid):
        return len(self.chunks[rid])

    def joined(self, rid, dtype):
        c = self.chunks[rid]
        return np.concatenate(c) if c else np.zeros(0, dtype=dtype)


def _references(eng, kws, i16=False):
    """Per request: generate_batch's result, and the chunk sizes of the same request through a plain session."""
    from q3tts import _abi, native
    want = eng.generate_batch([dict(kw, want_pcm=1) for kw in kws])
    sizes = []
    with native.NativeSession(eng, _abi.PCM_I16 if i16 else _abi.PCM_F32) as sess:
        col = Col(sess)
        for kw in kws:   # one at a time: a request's chunks do not depend on its neighbours
            rid = sess.submit(**kw)
            col.until(lambda: rid in col.fin)
            sizes.append([c.size for c in col.chunks[rid]])
    return want, sizes


def _check(col, rid, want, sizes, i16=False):
    from q3tts import _abi
    kind, res = col.fin[rid]
    assert kind == _abi.EV_DONE and res.status == 0 and want.status == 0
    assert res.codes.shape == want.codes.shape and np.array_equal(res.codes, want.codes) and res.hit_eos == want.hit_eos
    assert [c.size for c in col.chunks[rid]] == sizes
    pcm = _i16(want.pcm) if i16 else want.pcm
    assert _same_pcm(col.joined(rid, pcm.dtype), pcm)


def _session(eng, i16=False, swap=True):
    from q3tts import _abi, native
    return native.NativeSession(eng, _abi.PCM_I16 if i16 else _abi.PCM_F32, swap_mb=ARENA / (1 << 20) if swap else 0)


# ---- 1. pacing alone -------------------------------------------------------------------------------------------------------------------
def test_pacing_alone(eng):
    pairs = [_req(eng, i, 24) for i in range(2)]
    kws = [kw for kw, _ in pairs]
    want, sizes = _references(eng, kws)
    with _session(eng, swap=False) as sess:
        col = Col(sess)
        ids = [sess.submit(credit_frames=8, **kw) for kw in kws]
        col.until(lambda: all(col.n(r) == 2 for r in ids))
        assert sess.next(QUIET_MS) is None
        for r in ids:
            sess.grant(r, 8)
        col.until(lambda: all(col.n(r) == 4 for r in ids))
        assert sess.next(QUIET_MS) is None and not col.fin
        for r in ids:
            sess.grant(r, -1)
        col.until(lambda: len(col.fin) == 2)
        assert all(v == 0 for v in sess.swap_stats().values())
    for r, w, s in zip(ids, want, sizes):
        _check(col, r, w, s)


# ---- 2. more open requests than slots ----------------------------------------------------------------------------------------------------
def test_oversubscription(eng):
    pairs = [_req(eng, i, 24) for i in range(5)]
    kws = [kw for kw, _ in pairs]
    want, sizes = _references(eng, kws)
    with _session(eng) as sess:
        col = Col(sess)
        ids = [sess.submit(credit_frames=8, **kw) for kw in kws]
        col.until(lambda: all(col.n(r) == 2 for r in ids))   # all five, on two slots, before any grant
        assert sess.next(QUIET_MS) is None
        st = sess.swap_stats()
        assert st["swap_outs"] >= 3 and st["arena_used"] > 0
        for r in ids:
            sess.grant(r, 4)
        col.until(lambda: all(col.n(r) == 3 for r in ids))
        for r in reversed(ids):
            sess.grant(r, 12)
        col.until(lambda: all(col.n(r) == 6 for r in ids))
        assert sess.next(QUIET_MS) is None and not col.fin   # 24 frames, credit 24: the step that finds the end is not covered
        for r in ids[1::2] + ids[0::2]:
            sess.grant(r, -1)
        col.until(lambda: len(col.fin) == 5)
        st = sess.swap_stats()
        assert st["swap_outs"] >= 3 and st["swap_ins"] == st["swap_outs"] and st["arena_used"] == 0 and st["arena_peak"] > 0 and st["skipped"] == 0
    for r, w, s in zip(ids, want, sizes):
        _check(col, r, w, s)


# ---- 3. the same under each mode that adds state to a slot -------------------------------------------------------------------------------
def _oversubscribed(eng, kws, i16=False, n_out=2):
    """Four paced requests on two slots: everything runs to its credit (the first two leave their slots for the others), then the limits
    are lifted. Every request against its references."""
    want, sizes = _references(eng, kws, i16)
    with _session(eng, i16) as sess:
        col = Col(sess)
        ids = [sess.submit(credit_frames=8, **kw) for kw in kws]
        col.quiet()
        assert all(col.n(r) >= 1 for r in ids) and not col.fin
        assert sess.swap_stats()["swap_outs"] >= n_out
        for r in ids:
            sess.grant(r, -1)
        col.until(lambda: len(col.fin) == len(ids))
        st = sess.swap_stats()
        assert st["swap_ins"] == st["swap_outs"] >= n_out and st["arena_used"] == 0
    for r, w, s in zip(ids, want, sizes):
        _check(col, r, w, s, i16)


MODES = {
    "kv_q8_0": dict(cfg=dict(kv_q8_0=1)),
    "talker_q8a8": dict(cfg=dict(talker_q8_0=2)),
    "rate8000_f32": dict(rate=8000),
    "rate8000_i16": dict(rate=8000, i16=True),
    "lookahead2": dict(cfg=dict(voc_lookahead_frames=2), frames=[24, 22, 24, 22]),
    "lookahead2_flush": dict(cfg=dict(voc_lookahead_frames=2, vocoder_flush_tail=1), frames=[24, 22, 24, 22]),
    "pred_sampler_penalty": dict(pred=True),
    "prefix": dict(prefix=True),
}


@pytest.mark.parametrize("mode", sorted(MODES))
def test_oversubscription_in_mode(mode):
    from q3tts import native
    m = MODES[mode]
    e = _engine(_cfg(**m.get("cfg", {})))
    px = None
    try:
        if m.get("rate"):
            e.set_output_rate(m["rate"])
        if m.get("pred"):
            e.set_predictor_sampler(*TS.PRED_SAMPLER)
            e.set_repetition_penalty(1.05)
        frames = m.get("frames", [24] * 4)
        pairs = [_req(e, i, frames[i]) for i in range(4)]
        kws = [kw for kw, _ in pairs]
        if m.get("prefix"):
            vdesc, vk = native.make_prompt_desc(None, spk_emb=TS.S.spk(e.cfg.model.d_embed), part="voice")
            px = e.create_prefix(desc=vdesc)
            texts = [native.make_prompt_desc(np.arange(400 + 31 * i, 406 + 31 * i), part="text") for i in range(4)]
            kws = [dict(kw, desc=t[0], prefix=px) for kw, t in zip(kws, texts)]
        _oversubscribed(e, kws, m.get("i16", False))
    finally:
        if px is not None:
            px.close()
        e.close()


def test_keep_voice_request_swapped_out(eng):
    """A keep-voice request (streamed text, open) runs out of text, is swapped out by waiting requests and comes back: its prefix is the
    store q3tts_prefix_create makes, byte for byte, and requests behind it give the whole prompt's bits."""
    from q3tts import native
    d = eng.cfg.model.d_embed
    ids = TS.TEXTS["n40"]
    kw = TS.request("sampled")

    def store(x):
        n = C.c_int64(0)
        assert x.lib.q3tts_k_prefix_read(x.h, None, None, 0, C.byref(n)) == 0 and n.value > 0
        k, v = np.zeros(n.value, np.uint8), np.zeros(n.value, np.uint8)
        assert x.lib.q3tts_k_prefix_read(x.h, k.ctypes.data_as(C.c_void_p), v.ctypes.data_as(C.c_void_p), n.value, C.byref(n)) == 0
        return k, v
    vdesc, vk = native.make_prompt_desc(None, spk_emb=TS.S.spk(d), part="voice")
    with eng.create_prefix(desc=vdesc) as ref_px:
        ref_k, ref_v = store(ref_px)
    desc, keep = TS.stream_desc(ids, d)
    want = eng.generate(desc=desc, text_stream=True, want_pcm=1, **kw)
    fill = [_req(eng, 20 + i, 8) for i in range(2)]
    fwant, fsizes = _references(eng, [k for k, _ in fill])
    desc5, keep5 = TS.stream_desc(ids[:5], d)
    with _session(eng) as sess:
        col = Col(sess)
        rid, px = sess.submit(desc=desc5, keep_voice=True, text_stream=True, text_open=True, **kw)
        col.quiet()
        assert col.n(rid) == 1 and px.state == 1
        fids = [sess.submit(credit_frames=4, **k) for k, _ in fill]
        col.quiet()
        assert sess.swap_stats()["swap_outs"] >= 1 and all(col.n(f) == 1 for f in fids)
        sess.append_text(rid, ids[5:], close=True)
        for f in fids:
            sess.grant(f, -1)
        col.until(lambda: len(col.fin) == 3)
        assert sess.swap_stats()["swap_ins"] >= 1
    kind, res = col.fin[rid]
    assert np.array_equal(res.codes, want.codes) and res.hit_eos == want.hit_eos and _same_pcm(col.joined(rid, np.float32), want.pcm)
    for f, w, s in zip(fids, fwant, fsizes):
        _check(col, f, w, s)
    k1, v1 = store(px)   # (the hook is refused while a session owns the engine; the prefix outlives it)
    assert np.array_equal(k1, ref_k) and np.array_equal(v1, ref_v)
    px.close()


# ---- 4. positions at which the key-block copy can go wrong -------------------------------------------------------------------------------
def test_positions_around_key_blocks(eng):
    """cur_pos at swap-out = prompt rows + credit: 63, 64, 65 (one key block, short of it, past it) and 129; the last request has 24 frames
    behind it when it leaves and 20 more after it returns, so the vocoder's ring of 8 + 4 positions has wrapped on both sides."""
    d = eng.cfg.model.d_embed
    rng = np.random.default_rng(5)
    shapes = [(55, 8, 12), (56, 8, 12), (57, 8, 12), (105, 24, 44), (9, 4, 8), (9, 4, 8)]   # prompt rows, credit, frames
    assert [n + c for n, c, _ in shapes[:4]] == [63, 64, 65, 129]
    kws = [dict(embd=(rng.standard_normal((n, d)) * 0.05).astype(np.float32), temperature=0.7, top_k=40, top_p=0.9, seed=40 + i,
                max_steps=f + 8, min_frames=f, force_eos_at=f) for i, (n, c, f) in enumerate(shapes)]
    want, sizes = _references(eng, kws)
    with _session(eng) as sess:
        col = Col(sess)
        sub = lambda i: sess.submit(credit_frames=shapes[i][1], **kws[i])
        ids = {3: sub(3), 0: sub(0)}               # the long one and the first run to their credits and park
        col.quiet()
        ids.update({1: sub(1), 2: sub(2)})         # two more want slots: positions 63 and 129 leave
        col.quiet()
        assert sess.swap_stats()["swap_outs"] == 2
        ids.update({4: sub(4), 5: sub(5)})         # and two more: positions 64 and 65 leave
        col.quiet()
        ids = [ids[i] for i in range(6)]
        assert [col.n(r) for r in ids] == [c // 4 for _, c, _ in shapes] and not col.fin
        assert sess.swap_stats()["swap_outs"] == 4
        for r in ids:
            sess.grant(r, -1)
        col.until(lambda: len(col.fin) == len(ids))
        st = sess.swap_stats()
        assert st["swap_ins"] == st["swap_outs"] and st["arena_used"] == 0
    for r, w, s in zip(ids, want, sizes):
        _check(col, r, w, s)


# ---- 5. back into another slot -----------------------------------------------------------------------------------------------------------
def test_returns_into_a_different_slot(eng):
    pairs = [_req(eng, 30, 12), _req(eng, 31, 12), _req(eng, 32, 24)]
    kws = [kw for kw, _ in pairs]
    want, sizes = _references(eng, kws)
    with _session(eng) as sess:
        col = Col(sess)
        a = sess.submit(credit_frames=4, **kws[0])   # slot 0, parked first
        b = sess.submit(credit_frames=8, **kws[1])   # slot 1, parked one boundary later
        col.quiet()
        assert (col.n(a), col.n(b)) == (1, 2)
        c = sess.submit(credit_frames=8, **kws[2])   # waits: the longest-parked slot, A's, is swapped out for it
        col.quiet()
        assert col.n(c) == 2 and sess.swap_stats()["swap_outs"] == 1
        sess.grant(b, -1)                            # B finishes and frees slot 1; C stays parked in slot 0
        col.until(lambda: b in col.fin)
        sess.grant(a, -1)
        col.until(lambda: a in col.fin)
        st = sess.swap_stats()
        assert st["swap_ins"] == 1 and st["moved"] >= 1
        sess.grant(c, -1)
        col.until(lambda: c in col.fin)
    for r, w, s in zip([a, b, c], want, sizes):
        _check(col, r, w, s)


# ---- 6. streamed text --------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def oracle_env(oracle, eng):
    om = oracle.OracleModel(eng.cfg.model, seed=0, n_ctx=TS.N_CTX, n_threads=8)
    yield om, TS.mats_from_model(om, False, False)
    om.close()


def test_text_arrives_while_swapped_out(eng, oracle_env):
    om, pred = oracle_env
    d = eng.cfg.model.d_embed
    ids, kw = TS.TEXTS["n40"], TS.request("sampled")
    rows, T = TS.prompt(om, ids)
    ref, ref_eos = TS.generate(om, pred, rows, T, **kw)
    desc, keep = TS.stream_desc(ids, d)
    one = eng.generate(desc=desc, text_stream=True, want_pcm=1, **kw)
    desc5, keep5 = TS.stream_desc(ids[:5], d)
    fill = [_req(eng, 50 + i, 8) for i in range(2)]
    fwant, fsizes = _references(eng, [k for k, _ in fill])
    with _session(eng) as sess:
        col = Col(sess)
        x = sess.submit(desc=desc5, text_stream=True, text_open=True, **kw)   # len(T) = 4: one chunk, then starved
        col.quiet()
        assert col.n(x) == 1
        fids = [sess.submit(credit_frames=4, **k) for k, _ in fill]            # the second one needs x's slot
        col.quiet()
        assert all(col.n(f) == 1 for f in fids) and sess.swap_stats()["swap_outs"] == 1
        sess.append_text(x, ids[5:9])                                           # len(T) = 8: frames 4 .. 7 can run once it has a slot
        sess.append_text(x, ids[9:], close=True)
        col.until(lambda: x in col.fin)
        st = sess.swap_stats()
        assert st["swap_ins"] >= 1 and st["swap_outs"] >= 2                     # a parked filler made room for it
        for f in fids:
            sess.grant(f, -1)
        col.until(lambda: len(col.fin) == 3)
        assert sess.swap_stats()["arena_used"] == 0
    kind, res = col.fin[x]
    assert np.array_equal(res.codes, ref) and res.hit_eos == ref_eos and np.array_equal(res.codes, one.codes)
    assert _same_pcm(col.joined(x, np.float32), one.pcm)
    for f, w, s in zip(fids, fwant, fsizes):
        _check(col, f, w, s)


def test_paced_text_stream_obeys_both_rules(eng, oracle_env):
    om, pred = oracle_env
    d = eng.cfg.model.d_embed
    ids, kw = TS.TEXTS["n40"], TS.request("sampled", frames=16)
    rows, T = TS.prompt(om, ids)
    ref, ref_eos = TS.generate(om, pred, rows, T, **kw)
    desc9, keep9 = TS.stream_desc(ids[:9], d)
    with _session(eng, swap=False) as sess:
        col = Col(sess)
        x = sess.submit(desc=desc9, text_stream=True, text_open=True, credit_frames=4, **kw)   # text reaches 8 frames, the credit 4
        col.quiet()
        assert col.n(x) == 1
        sess.grant(x, 8)                                                                       # credit 12, text still 8
        col.quiet()
        assert col.n(x) == 2
        sess.append_text(x, ids[9:], close=True)                                               # text unlimited, credit 12
        col.quiet()
        assert col.n(x) == 3 and not col.fin
        sess.grant(x, -1)
        col.until(lambda: x in col.fin)
    kind, res = col.fin[x]
    assert res.codes.shape[0] == 16 and np.array_equal(res.codes, ref) and res.hit_eos == ref_eos


def test_paced_text_stream_returns_on_a_grant_alone(eng, oracle_env):
    """A text_stream request with all its text, stopped by its credit in the middle of the text, leaves its slot and comes back on a
    grant: its text rows and the cursor at frame 4 are uploaded again from the session's copy, not carried in the block."""
    om, pred = oracle_env
    d = eng.cfg.model.d_embed
    ids, kw = TS.TEXTS["n40"], TS.request("sampled", frames=16)
    rows, T = TS.prompt(om, ids)
    ref, ref_eos = TS.generate(om, pred, rows, T, **kw)
    desc, keep = TS.stream_desc(ids, d)
    fill = [_req(eng, 90 + i, 8) for i in range(2)]
    fwant, fsizes = _references(eng, [k for k, _ in fill])
    with _session(eng) as sess:
        col = Col(sess)
        x = sess.submit(desc=desc, text_stream=True, credit_frames=4, **kw)
        col.quiet()
        assert col.n(x) == 1
        fids = [sess.submit(credit_frames=4, **k) for k, _ in fill]   # the second one takes x's slot
        col.quiet()
        assert all(col.n(f) == 1 for f in fids) and sess.swap_stats()["swap_outs"] == 1
        sess.grant(x, -1)
        col.until(lambda: x in col.fin)
        st = sess.swap_stats()
        assert st["swap_ins"] >= 1 and st["swap_outs"] >= 2
        for f in fids:
            sess.grant(f, -1)
        col.until(lambda: len(col.fin) == 3)
        assert sess.swap_stats()["arena_used"] == 0
    kind, res = col.fin[x]
    assert res.codes.shape[0] == 16 and np.array_equal(res.codes, ref) and res.hit_eos == ref_eos
    for f, w, s in zip(fids, fwant, fsizes):
        _check(col, f, w, s)


# ---- 7. ends -----------------------------------------------------------------------------------------------------------------------------
def _two_out(eng, sess, col, base):
    """A and B (credit 4) swapped out by C and D; returns the ids and the fillers' keepalives."""
    pairs = [_req(eng, base + i, 12) for i in range(4)]
    ids = [sess.submit(credit_frames=4, **kw) for kw, _ in pairs]
    col.quiet()
    assert all(col.n(r) == 1 for r in ids)
    return ids, pairs


def test_cancel_and_close_with_swapped_out_requests(eng):
    from q3tts import _abi
    before = eng.device_bytes()
    sess = _session(eng)
    try:
        assert eng.device_bytes() >= before + ARENA
        col = Col(sess)
        ids, pairs = _two_out(eng, sess, col, 60)
        st = sess.swap_stats()
        assert st["swap_outs"] == 2 and st["arena_used"] > 0
        sess.cancel(ids[0])
        col.until(lambda: ids[0] in col.fin)
        assert col.fin[ids[0]][0] == _abi.EV_CANCELLED
        assert sess.next(QUIET_MS) is None   # exactly one final event, and nothing else moves
        st2 = sess.swap_stats()
        assert 0 < st2["arena_used"] < st["arena_used"] and st2["swap_ins"] == 0
        with pytest.raises(_abi.Q3Error):
            sess.grant(ids[0], 4)            # finished
    finally:
        th = threading.Thread(target=sess.close, daemon=True)   # one request is still swapped out, two are parked
        th.start()
        th.join(30)
    assert not th.is_alive(), "q3tts_session_close hangs on a swapped-out request"
    assert eng.device_bytes() == before
    kw, keep = _req(eng, 60, 12)
    again = eng.generate_batch([dict(kw, want_pcm=1)])[0]   # the engine serves as before
    assert again.status == 0 and again.codes.shape[0] == 12


def test_arena_with_room_for_one_block(eng):
    from q3tts import native
    pairs = [_req(eng, 70 + i, 12) for i in range(4)]
    kws = [kw for kw, _ in pairs]
    want, sizes = _references(eng, kws)
    with _session(eng) as sess:   # the size of one such block: what one swap-out takes from a large arena
        col = Col(sess)
        ids = [sess.submit(credit_frames=4, **kw) for kw in kws[:3]]
        col.quiet()
        st = sess.swap_stats()
        assert st["swap_outs"] == 1
        block = st["arena_used"]
    assert block > 0 and block % 256 == 0
    with native.NativeSession(eng) as sess:
        sess.set_swap(block)
        col = Col(sess)
        ids = [sess.submit(credit_frames=4, **kw) for kw in kws]
        col.quiet()
        st = sess.swap_stats()
        assert st["swap_outs"] == 1 and st["skipped"] > 0 and st["arena_used"] == block == st["arena_peak"]
        assert [col.n(r) for r in ids] == [1, 1, 1, 0] and not col.fin   # the fourth waits for a slot: nothing failed
        for r in ids:
            sess.grant(r, -1)
        col.until(lambda: len(col.fin) == 4)
        assert sess.swap_stats()["arena_used"] == 0
    for r, w, s in zip(ids, want, sizes):
        _check(col, r, w, s)


def test_refusals(eng):
    from q3tts import _abi, native
    kw, keep = _req(eng, 80, 8)
    with native.NativeSession(eng) as sess:
        for bad in (0, 3, -1):
            with pytest.raises(_abi.Q3Error, match="credit_frames"):
                sess.submit(credit_frames=bad, **kw)
        assert sess.lib.q3tts_session_set_swap(sess.h, -1) == INVALID
        sess.set_swap(1 << 20)
        sess.set_swap(0)                       # off again: still before the first submission
        col = Col(sess)
        plain = sess.submit(**kw)
        assert sess.lib.q3tts_session_set_swap(sess.h, 1 << 20) == STATE
        assert sess.lib.q3tts_session_grant(sess.h, plain, 4) == INVALID
        assert b"not submitted paced" in sess.lib.q3tts_session_last_error(sess.h)
        paced = sess.submit(credit_frames=4, **kw)
        assert sess.lib.q3tts_session_grant(sess.h, paced, 0) == INVALID
        assert sess.lib.q3tts_session_grant(sess.h, 12345, 4) == INVALID
        sess.grant(paced, -1)
        col.until(lambda: len(col.fin) == 2)
        assert sess.lib.q3tts_session_grant(sess.h, paced, 4) == INVALID   # finished
        assert all(v == 0 for v in sess.swap_stats().values())


# ---- 8. the wall-clock convenience of the reference-style API ----------------------------------------------------------------------------
def test_api_realtime_lead():
    from q3tts import api
    cfg = _cfg()
    e = api.TtsEngine(cfg)
    try:
        e.set_max_steps(8)
        e.set_sampler_config(api.SamplerConfig(temperature=0.7, top_k=40, top_p=0.9, seed=21))
        voice = api.VoiceFile.new("", [], TS.S.spk(cfg.model.d_embed).tolist())
        texts = [[int(i) for i in TS.TEXTS["n6"]], [int(i) for i in TS.TEXTS["n40"][:9]]]

        def run(**kw):
            out = defaultdict(list)
            for i, pcm, fin in e.stream_batch_with_voice(texts, [voice, voice], seeds=[5, 6], **kw):
                out[i].append(pcm)
            return [np.concatenate(out[i]) for i in range(2)]
        plain, paced = run(), run(realtime_lead_s=0.1)
        assert all(p.size > 0 and _same_pcm(q, p) for p, q in zip(plain, paced))
    finally:
        e.close()

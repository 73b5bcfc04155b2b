"""Speed and output rate of a streamed document on the GPU ("the pipeline"; include/q3tts.h, "documents in a session").
Kernel level, through q3tts_k_doc_stream_rate: scan -> plan -> join into the ring RJ -> k_doc_tempo into the ring RT -> k_doc_resample
(or k_doc_emit) into the staging buffer, boundary by boundary, equals resample32(stretch(join(rows))) of tests/_long_ref.py,
_tempo_ref.py and _resample_ref.py bit for bit, every chosen delta included, and the device one-shots q3tts_pcm_join ->
q3tts_time_stretch -> q3tts_resample — with the rings at their minimum, a staging buffer down to one sample, both formats and both lags.
Session level: a document with a speed, a rate and both equals q3tts_generate_long of a second engine with the same options."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _doc_ref as D  # noqa: E402
import _long_ref as R  # noqa: E402
import _resample_ref as RS  # noqa: E402
import _tempo_ref as T  # noqa: E402
from test_doc_gpu import (KINDS, MAX_STEPS, OPTION_SETS, SAMPLER, SEED, Got, _bits, _consume, _engine, _pcm, _plain_requests,  # noqa: E402,F401
                          _rows_bytes, _segments)

pytestmark = pytest.mark.gpu

NATIVE = 24000
THR = 0.01
LENS = [0, 241, 3001, 6000, 1500, 479]
ROW_KIND = [1, 2, 1, 1, 3, 0]        # test_doc_gpu's kinds of rows: 0 silent, 1 noise, 2 loud at both ends, 3 loud on a block boundary only
STRIDE = 6001                        # odd: every row has another 16-byte alignment
STEPS = [777, 1920, 5000, 1001]
COMBOS = [(500, 0), (1250, 0), (2000, 0), (0, 8000), (0, 16000), (0, 44100), (0, 48000), (1250, 8000), (800, 44100)]
PAUSES = (0, 10, 40, 90, 150)        # short, so that the restated stretch of a document stays a fraction of a second


def _make_rows():
    rng = np.random.default_rng(2817)
    x = np.full((len(LENS), STRIDE), np.nan, dtype=np.float32)
    for r, n in enumerate(LENS):
        row = rng.uniform(-0.004, 0.004, n).astype(np.float32)
        if ROW_KIND[r] == 1:
            row = rng.uniform(-1.0, 1.0, n).astype(np.float32)
        elif ROW_KIND[r] == 2 and n:
            row[0], row[n - 1] = 0.5, -0.5
        elif ROW_KIND[r] == 3 and n:
            row[R.W * ((n // R.W) // 2)] = 0.25
        x[r, :n] = row
    sched = [D.schedule(n, STEPS[r % len(STEPS)]) if n else [0] for r, n in enumerate(LENS)]
    return x, sched, [x[r, :n] for r, n in enumerate(LENS)], [3, 2, 4, 1, 3, 0]


_TABLES, _EXPECT = {}, {}


def _table(rate):
    from q3tts import native
    if rate not in _TABLES:
        _TABLES[rate] = native.k_resample_table(NATIVE, rate)
    return _TABLES[rate]


def _compose(J, speed, rate):
    """resample32(stretch(J)): (f32 row, the deltas or None)."""
    y, dl = np.asarray(J, dtype=np.float32), None
    if speed:
        y, dl = T.stretch(y, speed)
    if rate:
        L, M, H, tab = _table(rate)
        y = RS.resample32(y, y.size, tab, L, M, H, 0, RS.N(y.size, L, M))
    return y, dl


def _expect(key, rows, kinds, kw, speed, rate):
    """The restatement composition of one (rows, options, speed, rate): computed once, shared, never written to."""
    k = (key, speed, rate)
    if k not in _EXPECT:
        J, plan, N = R.join(rows, kinds, **kw)
        y, dl = _compose(J, speed, rate)
        y.setflags(write=False)
        _EXPECT[k] = (J, plan, y, dl)
    return _EXPECT[k]


def _rings(speed, rate, how):
    """how 0: both at their minimum (0 asks the hook for it); 1: a session-like default; 2: minimum + 4; 3: room for a whole test document."""
    from q3tts import native
    if how == 0:
        return 0, 0
    mins = native.k_doc_ring_plan(np.zeros(4, dtype=np.int64), 0, 0, 1, speed_permille=speed, output_rate=rate)
    add = {1: 15360, 2: 4, 3: 40000}[how]
    return mins["min_j"] + add, (mins["min_t"] + (4 if how == 2 else 2 * add + 256)) if speed else 0


def _check(out, fmt, want):
    if fmt:
        assert out.dtype == np.int16 and np.array_equal(out, D.pack_i16(want))
    else:
        assert out.size == want.size and np.array_equal(_bits(out), _bits(want)), (out.size, want.size, np.flatnonzero(_bits(out[:want.size]) != _bits(want[:out.size]))[:4])


@pytest.fixture(scope="module")
def rate_rows():
    return _make_rows()


@pytest.fixture(scope="module")
def engines():
    """Two engines of the tiny shape: one for sessions, one for q3tts_generate_long and the one-shots (the expected side)."""
    eng, vdesc, vkeep = _engine(2)
    ref, rdesc, rkeep = _engine(2)
    px = eng.create_prefix(desc=vdesc)
    from q3tts import native
    with native.NativeSession(eng) as ses:      # (what an engine allocates for its life at its first session is in bytes0)
        ses.submit_document(_segments()[:1], prefix=px, seed=SEED, **SAMPLER)
        _consume(ses)
    yield dict(eng=eng, vdesc=vdesc, px=px, ref=ref, rdesc=rdesc, keep=(vkeep, rkeep), bytes0=eng.device_bytes(), want={})
    px.close()
    eng.close()
    ref.close()


# ---- kernel level ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("speed,rate", COMBOS)
def test_options_and_formats(rate_rows, speed, rate):
    """Each speed and rate alone and two pairs, f32 and i16, lag 0 and 1, the rings at their minimum, at a default and at minimum + 4:
    the concatenation is the restatement composition bit for bit and so is every delta_k; nothing outside a chunk is written."""
    from q3tts import native
    x, sched, rows, kinds = rate_rows
    kw = dict(trim=1, threshold=THR, keep=480, fade=120, pause_ms=PAUSES)
    J, plan, want, dl = _expect("default", rows, kinds, kw, speed, rate)
    i = 0
    for fmt in (0, 1):
        for lag in (0, 1):
            for how in (0, 1, 2):     # every format and lag at every ring size; staging, dst0 and ahead go round beside them
                rj, rt = _rings(speed, rate, how)
                staging, dst0, ahead = (7680, 2001, 30000, 250, 1000)[i % 5], (0, 5, 3, 1, 2)[i % 5], (2, 1, 6, 3, 4)[i % 5]
                out, chunks, got_plan, bad, got_dl = native.k_doc_stream_rate(x, kinds, sched, ahead, staging + dst0, speed, rate, rj, rt, dst0=dst0, lag=lag, fmt=fmt, **kw)
                _check(out, fmt, want)
                assert np.array_equal(got_plan, plan) and bad == 0 and chunks.max() <= staging, (fmt, lag, how, i)
                if speed:
                    assert np.array_equal(got_dl, dl), (fmt, lag, how, np.flatnonzero(got_dl[:dl.size] != dl[:got_dl.size])[:4])
                i += 1


@pytest.mark.parametrize("part", range(3))
def test_every_join_option_set(rate_rows, engines, part):
    """test_doc_gpu's option sets, each with another speed / rate pair and the rings at their minimum: against the device one-shots
    q3tts_pcm_join -> q3tts_time_stretch -> q3tts_resample of the same rows, and against the restatement composition wherever the joined
    row is short enough to restate in a second (the 60 s pause is compared with the one-shots only: 5 600 frames in numpy take too long;
    test_a_long_pause_with_rings_at_their_minimum restates a 3 s one)."""
    from q3tts import native
    x, sched, rows, kinds = rate_rows
    ref = engines["ref"]
    for i, base in enumerate(OPTION_SETS):
        if i % 3 != part:
            continue
        kw = dict(base, threshold=THR)
        speed, rate = COMBOS[(i * 5 + 7) % len(COMBOS)]
        big = max(kw["pause_ms"]) == 60000
        staging = (7680, 30721)[i % 2]
        rj, rt = _rings(speed, rate, 0)
        out, chunks, got_plan, bad, got_dl = native.k_doc_stream_rate(x, kinds, sched, (1, 2, 6)[i % 3], staging, speed, rate, rj, rt, lag=i % 2, delta_cap=1 << 15, **kw)
        y, edges = ref.pcm_join(rows, kinds, **kw)
        assert np.array_equal(got_plan, edges) and bad == 0
        if speed:
            y = ref.time_stretch(y, speed) if y.size else y
        if rate:
            y = ref.resample(y, NATIVE, rate) if y.size else y
        _check(out, 0, y)
        if not big:
            J, plan, want, dl = _expect(("set", i), rows, kinds, kw, speed, rate)
            _check(out, 0, want)
            assert np.array_equal(got_plan, plan) and (dl is None or np.array_equal(got_dl, dl))


@pytest.mark.parametrize("speed,rate", [(2000, 0), (0, 16000), (1250, 8000)])
def test_a_long_pause_with_rings_at_their_minimum(rate_rows, speed, rate):
    """A 3 s pause (72 000 zeros, many ring turns, tens of boundaries) with both rings at their minimum, f32 and i16, both lags: against
    the restatement composition — the independent reference that the 60 s pause of the option-set sweep, compared with the device
    one-shots only, does not have."""
    from q3tts import native
    x, sched, rows, kinds = rate_rows
    kw = dict(trim=1, threshold=THR, keep=480, fade=120, pause_ms=(0, 3000, 0, 0, 0))
    J, plan, want, dl = _expect("pause3s", rows, kinds, kw, speed, rate)
    assert J.size > 72000
    for fmt, lag, staging in ((0, 1, 7680), (1, 0, 2001)):
        out, chunks, got_plan, bad, got_dl = native.k_doc_stream_rate(x, kinds, sched, 3, staging, speed, rate, 0, 0, lag=lag, fmt=fmt, **kw)
        _check(out, fmt, want)
        assert np.array_equal(got_plan, plan) and bad == 0 and chunks.max() <= staging and len(chunks) > 10
        assert dl is None or np.array_equal(got_dl, dl)


@pytest.mark.parametrize("staging,nr,speed,rate", [(1, 2, 1250, 0), (1, 2, 0, 8000), (1, 2, 800, 44100), (3, 4, 2000, 16000), (3, 4, 500, 0),
                                                   (250, 6, 1250, 8000), (250, 6, 0, 48000), (250, 6, 2000, 0)])
def test_small_staging_with_rings_at_their_minimum(rate_rows, staging, nr, speed, rate):
    """A staging buffer of 1, 3 and 250 samples (a one-sample buffer takes a boundary per output: one short document), rings at their
    minimum, steps of 7 and 100 samples: the wrap falls inside template windows, candidate spans, tile spans and 16-byte groups."""
    from q3tts import native
    x, _, rows, kinds = rate_rows
    sel = [1, 5, 4, 0, 2, 3][:nr]     # 241 and 479 samples first
    xs = np.ascontiguousarray(x[sel])
    rs_, ks = [rows[r] for r in sel], [kinds[r] for r in sel]
    sched = [D.schedule(int(r.size), 7 if staging == 1 else 100) if r.size else [0] for r in rs_]
    kw = dict(trim=staging % 2, threshold=THR, keep=100, fade=50, pause_ms=(1, 0, 1, 0, 2))
    J, plan, want, dl = _expect(("small", nr, kw["trim"]), rs_, ks, kw, speed, rate)
    for fmt, lag in ((0, 1), (1, 0)):
        out, chunks, got_plan, bad, got_dl = native.k_doc_stream_rate(xs, ks, sched, 3, staging + 3, speed, rate, 0, 0, dst0=3, lag=lag, fmt=fmt, chunk_cap=1 << 18, **kw)
        _check(out, fmt, want)
        assert np.array_equal(got_plan, plan) and bad == 0 and chunks.max() <= staging
        assert dl is None or np.array_equal(got_dl, dl)


@pytest.mark.parametrize("speed,rate", [(1250, 0), (0, 16000), (800, 8000)])
def test_a_segment_closed_late_holds_the_tail_back(rate_rows, speed, rate):
    """The last segment reaches its full length at the first boundary and is closed five boundaries later: until then exactly the outputs
    that the joined prefix decides are out (the stretch's HOLD plus a hop and the resampler's H stay behind), nothing follows while it
    stays open, and closing delivers the exact tail."""
    from q3tts import native
    x, _, rows, kinds = rate_rows
    sel = [2, 4, 3]
    xs, rs_, ks = np.ascontiguousarray(x[sel]), [rows[r] for r in sel], [kinds[r] for r in sel]
    sched = [[r.size] for r in rs_]
    sched[-1] = [rs_[-1].size] * 6
    kw = dict(trim=0, threshold=THR, keep=0, fade=120, pause_ms=PAUSES)
    J, plan, want, dl = _expect("late", rs_, ks, kw, speed, rate)
    rj, rt = _rings(speed, rate, 3)
    out, chunks, got_plan, bad, got_dl = native.k_doc_stream_rate(xs, ks, sched, 3, 1 << 17, speed, rate, rj, rt, lag=0, **kw)
    _check(out, 0, want)
    nj = J.size - kw["fade"]                      # what an open last segment lets the join hand out
    nt = T.D_t(nj, speed) if speed else nj
    L, M, H = _table(rate)[:3] if rate else (1, 1, 0)
    decided = RS.D(nt, L, M, H) if rate else nt
    assert len(chunks) == 6 and chunks[0] == decided and list(chunks[1:5]) == [0] * 4 and chunks[5] == want.size - decided and chunks[5] > 0
    assert bad == 0 and (dl is None or np.array_equal(got_dl, dl))


def test_the_existing_kernels_still_equal_their_restatements(rate_rows):
    """k_pcm_tempo and k_pcm_resample now share their staging loops and chains with the ring forms: one case of each, as before."""
    from q3tts import native
    x, _, rows, _ = rate_rows
    lens = np.array([[1500, 0, 1000, 2000, 700, 100], LENS], dtype=np.int32)
    lens = np.minimum(lens, np.array(LENS, dtype=np.int32)[None, :])
    got = native.k_pcm_tempo(x, lens, [1] * len(LENS), 1250, 6144, delta_stride=32)
    out, n_valid, delta = got[0], got[1], got[2]
    ref = T.Tempo(np.nan_to_num(x, nan=0.0), 1250)
    for t in range(2):
        nv = ref.feed(lens[t], [t == 1] * len(LENS))
        assert list(n_valid[t]) == list(nv)
        for r in range(len(LENS)):
            assert np.array_equal(_bits(out[t, r, :nv[r]]), _bits(ref.y[r, :nv[r]]))
    for r in range(len(LENS)):
        assert list(delta[r, :len(ref.delta[r])]) == ref.delta[r]
    L, M, H, tab = _table(16000)
    n = LENS[3]
    cnt = RS.N(n, L, M)
    y = native.k_pcm_resample(x, LENS, [1] * len(LENS), [(3, 0, cnt, 5)], cnt + 9, NATIVE, 16000)
    y = y[0] if isinstance(y, tuple) else y
    assert np.array_equal(_bits(y[5:5 + cnt]), _bits(RS.resample32(x[3], n, tab, L, M, H, 0, cnt)))


def test_stream_rate_hook_refuses_bad_rings(rate_rows):
    from q3tts import _abi, native
    x, sched, rows, kinds = rate_rows
    for kw in (dict(speed_permille=1250, ring_j=1276), dict(speed_permille=1250, ring_j=1282), dict(speed_permille=1250, ring_t=252),
               dict(output_rate=8000, ring_j=208), dict(), dict(speed_permille=1000, output_rate=NATIVE), dict(speed_permille=2001), dict(output_rate=3999)):
        with pytest.raises(_abi.Q3Error):
            native.k_doc_stream_rate(x, kinds, sched, 2, 7680, **kw)


# ---- the session ------------------------------------------------------------------------------------------------------------------
OPTS = {"speed": dict(speed_permille=1250), "rate": dict(output_rate=16000), "both": dict(speed_permille=800, output_rate=8000), "plain": dict()}


def _want(engines, name, join=None):
    """q3tts_generate_long of the second engine for one option set: computed once, before or between sessions."""
    key = (name, None if join is None else tuple(sorted(join.items())))
    if key not in engines["want"]:
        engines["want"][key] = engines["ref"].generate_long(_segments(), voice=engines["rdesc"], seed=SEED, join=join, **OPTS[name], **SAMPLER)
    return engines["want"][key]


def _check_rated(g, want, name, ses=None, did=None):
    """A finished document against generate_long's result: the bits, document_info field for field, the SEGMENT events, DONE."""
    from q3tts import _abi
    o = OPTS[name]
    assert g.final == _abi.EV_DONE and g.order_ok and g.last_chunk_final
    got = _pcm(g)
    assert got.size == want.n_samples and np.array_equal(_bits(got), _bits(want.pcm)), (got.size, want.n_samples)
    plan = [(0, 0, f["begin"], f["end"]) for f in want.info]
    maps = R.out_maps(plan, o.get("speed_permille", 0), o.get("output_rate", 0))
    assert [(f["out_begin"], f["out_end"]) for f in want.info] == maps
    assert [s.segment for s in g.segs] == list(range(len(want.info)))
    assert [s.n_samples for s in g.segs] == [e - b for b, e in maps]
    rate = o.get("output_rate", 0) or NATIVE
    for s, f, (b, e) in zip(g.segs, want.info, maps):
        assert (s.status, s.codes.shape[0], int(s.hit_eos), s.sample_rate) == (0, f["n_frames"], f["hit_eos"], rate)
        assert s.at >= e                              # the chunk that brought the delivered count to out_end was out
    assert g.res.status == 0 and g.res.n_samples == want.n_samples and g.res.sample_rate == rate == want.sample_rate
    if ses is not None:
        info, n_del = ses.document_info(did)
        assert info == want.info and n_del == want.n_samples


def _stream(eng, name, fmt=0, **kw):
    from q3tts import native
    with native.NativeSession(eng, fmt) as ses:
        did = ses.submit_document(_segments(), seed=SEED, **OPTS[name], **SAMPLER, **kw)
        got = _consume(ses)
        return got[did], ses.document_info(did)


@pytest.mark.parametrize("name", ["speed", "rate", "both"])
@pytest.mark.parametrize("ahead", [1, 7])
def test_rated_document_equals_generate_long(engines, name, ahead):
    from q3tts import native
    d = engines
    want = _want(d, name)
    with native.NativeSession(d["eng"]) as ses:
        did = ses.submit_document(_segments(), prefix=d["px"], seed=SEED, ahead=ahead, **OPTS[name], **SAMPLER)
        got = _consume(ses)
        _check_rated(got[did], want, name, ses, did)
    assert d["eng"].device_bytes() == d["bytes0"]


def test_both_fields_zero_is_the_document_of_today(engines):
    d = engines
    for o in (dict(), dict(speed_permille=1000, output_rate=NATIVE)):
        from q3tts import native
        with native.NativeSession(d["eng"]) as ses:
            did = ses.submit_document(_segments(), voice=d["vdesc"], seed=SEED, **o, **SAMPLER)
            got = _consume(ses)
            _check_rated(got[did], _want(d, "plain"), "plain", ses, did)


@pytest.mark.parametrize("slots", [1, 4])
def test_rated_document_on_other_slot_counts(engines, slots):
    eng, vdesc, keep = _engine(slots)
    try:
        g, (info, n_del) = _stream(eng, "both", voice=vdesc)
        _check_rated(g, _want(engines, "both"), "both")
        assert info == _want(engines, "both").info
    finally:
        eng.close()


def test_rated_document_in_an_i16_session(engines):
    from q3tts import _abi
    d = engines
    for name in ("speed", "both"):
        g, _ = _stream(d["eng"], name, fmt=_abi.PCM_I16, prefix=d["px"])
        got = _pcm(g, np.int16)
        assert g.final == _abi.EV_DONE and got.dtype == np.int16 and np.array_equal(got, D.pack_i16(_want(d, name).pcm))


def test_rated_document_beside_plain_requests_and_a_plain_document(engines):
    """A plain request before the document and two once its first chunk is out; then a speed document beside a plain document."""
    from q3tts import _abi, native
    d = engines
    reqs, keep = _plain_requests(d["px"])
    outs = None
    with native.NativeSession(d["eng"]) as ses:
        first = ses.submit(**reqs[3])
        did = ses.submit_document(_segments(), prefix=d["px"], seed=SEED, **OPTS["both"], **SAMPLER)
        got = _consume(ses, stop=lambda got, ev: ev[0] == did and ev[1] == _abi.EV_CHUNK)
        late = [ses.submit(**reqs[5]), ses.submit(**reqs[2])]
        _consume(ses, got=got)
        _check_rated(got[did], _want(d, "both"), "both", ses, did)
        outs = {i: got[rid] for rid, i in zip([first] + late, (3, 5, 2))}
        assert all(g.final == _abi.EV_DONE for g in outs.values())
    with native.NativeSession(d["eng"]) as ses:     # the plain requests' own PCM: the same requests alone
        ids = {i: ses.submit(**reqs[i]) for i in (3, 5, 2)}
        alone = _consume(ses)
        for i, rid in ids.items():
            assert np.array_equal(_bits(_pcm(alone[rid])), _bits(_pcm(outs[i]))) and _pcm(outs[i]).size > 0
    with native.NativeSession(d["eng"]) as ses:
        a = ses.submit_document(_segments(), prefix=d["px"], seed=SEED, ahead=2, **OPTS["speed"], **SAMPLER)
        b = ses.submit_document(_segments(), voice=d["vdesc"], seed=SEED, ahead=3, **SAMPLER)
        got = _consume(ses)
        _check_rated(got[a], _want(d, "speed"), "speed", ses, a)
        _check_rated(got[b], _want(d, "plain"), "plain", ses, b)


def test_rated_append_with_a_late_close(engines):
    """Open with three segments; when the third is out the document is silent with the held-back tail undelivered; four more and the
    close give the bits of the seven at once."""
    from q3tts import _abi, native
    d = engines
    segs = _segments()
    want = _want(d, "both")
    with native.NativeSession(d["eng"]) as ses:
        did = ses.submit_document(segs[:3], prefix=d["px"], seed=SEED, open=True, **OPTS["both"], **SAMPLER)
        got = _consume(ses, stop=lambda got, ev: ev[1] == _abi.EV_SEGMENT and ev[4].segment == 1)
        while True:                                               # what is decidable drains, then nothing
            ev = ses.next(300)
            if ev is None:
                break
            assert ev[1] in (_abi.EV_CHUNK, _abi.EV_SEGMENT) and ev[0] == did
            if ev[1] == _abi.EV_CHUNK:
                got[did].chunks.append(ev[2])
            else:
                ev[4].at = sum(c.size for c in got[did].chunks)
                got[did].segs.append(ev[4])
        assert did in ses.open_ids
        info, n_del = ses.document_info(did)
        part = _pcm(got[did])
        assert n_del == part.size < want.info[2]["out_end"] and len(info) == 2      # the third piece's tail is held back: no SEGMENT yet
        assert np.array_equal(_bits(part), _bits(want.pcm[:part.size]))
        ses.append_document(did, segs[3:5])
        ses.append_document(did, segs[5:], close=True)
        _consume(ses, got=got)
        _check_rated(got[did], want, "both", ses, did)


def _ring_bytes(eng, speed, rate):
    """What a rated document's rings add to q3tts_k_device_bytes in a session of this engine: the minimum plus twice one slot's share of
    the staging buffer (RT: that share stretched, and a hop); with a speed the stretch's window and 16 bytes for the p of its last frame,
    with a rate the resampler's L x T table."""
    from q3tts import native
    win = 2 * (4 + max(0, eng.cfg.vocoder.lookahead_frames)) * 1920
    mins = native.k_doc_ring_plan(np.zeros(4, dtype=np.int64), 0, 0, 1, speed_permille=speed, output_rate=rate)
    cj = (mins["min_j"] + win + 3) & ~3
    ct = (mins["min_t"] + T.N_t(win, speed) + T.HS + 3) & ~3 if speed else 0
    return 4 * (cj + ct) + (4 * T.WN + 16 if speed else 0) + (4 * _table(rate)[3].size if rate else 0)


def test_rated_cancel_at_the_first_chunk_frees_the_rings(engines):
    from q3tts import _abi, native
    d = engines
    with native.NativeSession(d["eng"]) as ses:
        did = ses.submit_document(_segments(), prefix=d["px"], seed=SEED, ahead=2, **OPTS["both"], **SAMPLER)
        got = _consume(ses, stop=lambda got, ev: ev[0] == did and ev[1] == _abi.EV_CHUNK)
        assert d["eng"].device_bytes() == d["bytes0"] + _rows_bytes(d["eng"], 2) + _ring_bytes(d["eng"], 800, 8000)
        ses.cancel(did)
        rest = _consume(ses)[did]
        assert rest.chunks == [] and rest.segs == [] and rest.final == _abi.EV_CANCELLED
        assert d["eng"].device_bytes() == d["bytes0"]
        part = _pcm(got[did])
        assert np.array_equal(_bits(part), _bits(_want(d, "both").pcm[:part.size]))
        again = ses.submit_document(_segments(), voice=d["vdesc"], seed=SEED, **OPTS["speed"], **SAMPLER)
        _check_rated(_consume(ses)[again], _want(d, "speed"), "speed", ses, again)
    assert d["eng"].device_bytes() == d["bytes0"]


def test_rated_document_refused_for_memory_counts_the_rings(engines):
    from q3tts import _abi, native
    d = engines
    need = _rows_bytes(d["eng"], 4) + _ring_bytes(d["eng"], 1250, 0)
    with native.NativeSession(d["eng"]) as ses:
        ses.doc_mem_cap(need - 1)
        did = ses.submit_document(_segments(), prefix=d["px"], seed=SEED, ahead=4, **OPTS["speed"], **SAMPLER)
        got = _consume(ses)
        assert got[did].final == _abi.EV_FAILED and got[did].res.status == -3 and got[did].chunks == []
        msg = d["eng"].lib.q3tts_last_error(d["eng"].h).decode()
        assert str(need) in msg and str(need - 1) in msg, msg
        assert d["eng"].device_bytes() == d["bytes0"]
        plain = ses.submit_document(_segments(), prefix=d["px"], seed=SEED, ahead=4, **SAMPLER)   # (its rows alone fit)
        _check_rated(_consume(ses)[plain], _want(d, "plain"), "plain", ses, plain)
        ses.doc_mem_cap(need)
        ok = ses.submit_document(_segments(), prefix=d["px"], seed=SEED, ahead=4, **OPTS["speed"], **SAMPLER)
        _check_rated(_consume(ses)[ok], _want(d, "speed"), "speed", ses, ok)


def test_rated_refusals(engines):
    from q3tts import _abi, native
    d = engines
    eng, segs = d["eng"], _segments()
    with native.NativeSession(eng) as ses:
        for kw in (dict(speed_permille=499), dict(speed_permille=2001), dict(output_rate=3999), dict(output_rate=96001)):
            with pytest.raises(_abi.Q3Error, match=r"\(-1\)"):
                ses.submit_document(segs, prefix=d["px"], seed=SEED, **kw, **SAMPLER)
        with pytest.raises(_abi.Q3Error, match=r"\(-6\)"):
            ses.submit_document(segs, prefix=d["px"], seed=SEED, output_rate=44099, **SAMPLER)     # L x T past the table's bound
        assert not ses.open_ids
    for setter, val in ((eng.set_speed, 1250), (eng.set_output_rate, 16000)):
        setter(val)
        try:
            with native.NativeSession(eng) as ses:
                with pytest.raises(_abi.Q3Error, match=r"\(-5\)"):
                    ses.submit_document(segs, prefix=d["px"], seed=SEED, **OPTS["both"], **SAMPLER)
        finally:
            setter(0)

"""Documents in a session on the GPU (include/q3tts.h, "documents in a session: the streaming join"): k_doc_scan and
k_doc_emit, driven boundary by boundary with the host plan between them through q3tts_k_doc_stream, against the numpy join of
tests/_long_ref.py bit for bit — whatever the schedule, the look-ahead, the staging size, the plan's lag and the format — and against the
session model of tests/_doc_ref.py chunk by chunk; what a launch must not write keeps its uploaded value."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _doc_ref as D  # noqa: E402
import _long_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

LENS = [0, 1, 239, 240, 241, 479, 481, 7680, 23057]
STRIDE = 23059  # odd: every row has another 16-byte alignment
THR = np.float32(0.01)
N_KINDS = 4     # silent, noise, loud at 0 and at n - 1, loud on a block boundary only
STEPS = [777, 1920, 5000, 1001]   # per row, cycling: no multiple of 240 but the second


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _rows():
    """Per length four rows, so that rows without a loud block lie between the others; NaN behind every valid length."""
    rng = np.random.default_rng(27)
    lens = np.repeat(np.array(LENS, dtype=np.int64), N_KINDS)
    x = np.full((lens.size, STRIDE), np.nan, dtype=np.float32)
    for r, n in enumerate(lens):
        kind = r % N_KINDS
        row = rng.uniform(-0.004, 0.004, n).astype(np.float32)   # below the threshold
        if kind == 1:
            row = rng.uniform(-1.0, 1.0, n).astype(np.float32)
        elif kind == 2 and n:
            row[0], row[n - 1] = 0.5, -0.5
        elif kind == 3 and n:
            row[min(R.W * max(1, (n // R.W) // 2), n - 1)] = 0.25   # the first sample of a block (or the row's last sample)
        x[r, :n] = row
    sched = [D.schedule(int(n), STEPS[r % len(STEPS)]) for r, n in enumerate(lens)]
    return x, lens, sched


@pytest.fixture(scope="module")
def doc_rows():
    x, lens, sched = _rows()
    return x, lens, sched, [x[r, :n] for r, n in enumerate(lens)], [r % 5 for r in range(lens.size)]


OPTION_SETS = [dict(trim=0, keep=480, fade=f, pause_ms=p) for f in (0, 1, 120, 10**6) for p in ((0, 0, 0, 0, 0), (0, 0, 150, 300, 600))] + \
              [dict(trim=1, keep=k, fade=f, pause_ms=(0, 0, 150, 300, 600)) for k in (0, 480, 10**6) for f in (0, 1, 120, 10**6)] + \
              [dict(trim=1, keep=480, fade=120, pause_ms=(0, 60000, 0, 0, 0))]


@pytest.mark.parametrize("lag", [0, 1])
def test_stream_kernels_equal_the_join(doc_rows, lag):
    """Every option set over 36 rows of 0 .. 23 057 samples: the concatenation, the plan and N equal the join's; the chunks equal the
    session model's; no boundary exceeds the staging buffer; nothing outside a chunk's window or a scanned range is written."""
    from q3tts import native
    x, lens, sched, rows, kinds = doc_rows
    for i, kw in enumerate(OPTION_SETS):
        kw = dict(kw, threshold=float(THR))
        ahead, staging, dst0 = (1, 2, 7, 64)[i % 4], (30721, 7680, 100003)[i % 3], (0, 5, 3)[i % 3]
        if max(kw["pause_ms"]) == 60000:
            staging = 600001
        J, plan, N = R.join(rows, kinds, **kw)
        out, chunks, got_plan, bad = native.k_doc_stream(x, kinds, sched, ahead, staging, dst0=dst0, lag=lag, check_rows=int(i % 5 == 0), **kw)
        assert out.size == N and np.array_equal(_bits(out), _bits(J)), (kw, ahead, staging, np.flatnonzero(_bits(out[:N]) != _bits(J[:out.size]))[:4])
        assert np.array_equal(got_plan, plan), kw
        assert bad == 0 and chunks.max() <= staging - dst0
        if i % 4 == 0:   # (the model walks the rows in Python: a quarter of the sets)
            _, want_chunks, _, _ = D.drive(rows, kinds, sched, ahead, staging - dst0, lag=lag, **kw)
            assert list(chunks) == want_chunks, kw


def test_small_staging_and_a_block_across_every_boundary(doc_rows):
    """A staging buffer of a few samples, steps of 7 and 100 samples (a block is scanned over many boundaries), rows of up to 481 samples."""
    from q3tts import native
    x, lens, _, rows, kinds = doc_rows
    sel = [r for r, n in enumerate(lens) if n <= 481]
    xs, rs, ks = x[sel][:, :483], [rows[r] for r in sel], [kinds[r] for r in sel]
    xs = np.ascontiguousarray(xs)
    for step, staging, ahead, lag, nr in ((7, 1, 3, 1, 14), (100, 3, 2, 0, 16), (7, 250, 5, 1, len(sel))):   # (nr: a one-sample buffer takes a boundary per sample)
        r_, k_, x_ = rs[:nr], ks[:nr], np.ascontiguousarray(xs[:nr])
        sched = [D.schedule(int(r.size), step) for r in r_]
        for trim in (0, 1):
            kw = dict(trim=trim, threshold=float(THR), keep=100, fade=50, pause_ms=(1, 0, 1, 0, 2))
            J, plan, N = R.join(r_, k_, **kw)
            out, chunks, got_plan, bad = native.k_doc_stream(x_, k_, sched, ahead, staging + 3, dst0=3, lag=lag, check_rows=1, **kw)
            assert np.array_equal(_bits(out), _bits(J)) and np.array_equal(got_plan, plan) and bad == 0, (step, staging, trim)
            assert chunks.max() <= staging


def test_one_boundary_emits_a_tail_two_pieces_and_two_pauses():
    """Segment 0 runs for five boundaries while segments 1 and 2 finish behind it: its last boundary emits its tail, then both pauses and
    both whole pieces in one launch."""
    from q3tts import native
    rng = np.random.default_rng(3)
    lens = [9001, 777, 1203]
    x = np.full((3, 9003), np.nan, dtype=np.float32)
    for r, n in enumerate(lens):
        x[r, :n] = rng.uniform(-1.0, 1.0, n).astype(np.float32)
    rows = [x[r, :n] for r, n in enumerate(lens)]
    kinds, sched = [3, 4, 0], [D.schedule(9001, 1920), [777], [700, 1203]]
    kw = dict(trim=1, threshold=float(THR), keep=480, fade=120, pause_ms=(0, 0, 150, 300, 600))
    J, plan, N = R.join(rows, kinds, **kw)
    S, want_chunks, _, trace = D.drive(rows, kinds, sched, 3, 10**5, lag=0, **kw)
    assert [p[0] for p in trace[4]] == [0, -1, 1, -1, 2] and trace[4][0][2] > 0 and len(trace) == 5
    for fmt in (0, 1):
        out, chunks, got_plan, bad = native.k_doc_stream(x, kinds, sched, 3, 10**5 + 1, dst0=1, lag=0, fmt=fmt, check_rows=1, **kw)
        assert list(chunks) == want_chunks and bad == 0 and np.array_equal(got_plan, plan)
        if fmt == 0:
            assert np.array_equal(_bits(out), _bits(J))
        else:
            assert out.dtype == np.int16 and np.array_equal(out, D.pack_i16(J))


def test_i16_is_the_pack_conversion_of_the_f32_result(doc_rows):
    """Samples beyond +-1 among them (the conversion clamps), an odd destination offset, fades and pauses."""
    from q3tts import native
    x, lens, sched, rows, kinds = doc_rows
    x = x.copy()
    x[5, 0] = 1.5
    x[21, 100] = -1.25   # (inside row 21's fade-in)
    rows = [x[r, :n] for r, n in enumerate(lens)]
    for kw in (dict(trim=1, threshold=float(THR), keep=480, fade=120), dict(trim=0, fade=0, pause_ms=(0, 0, 0, 0, 0))):
        J, plan, N = R.join(rows, kinds, **kw)
        want = D.pack_i16(J)
        assert want.min() == -32768 and want.max() == 32767
        out, _, got_plan, bad = native.k_doc_stream(x, kinds, sched, 4, 30001, dst0=1, lag=1, fmt=1, **kw)
        assert np.array_equal(out, want) and np.array_equal(got_plan, plan) and bad == 0


def test_stream_hook_refuses_what_would_leave_the_buffers(doc_rows):
    from q3tts import _abi, native
    x, lens, sched, rows, kinds = doc_rows
    bad_sched = [list(s) for s in sched]
    bad_sched[-1][-1] = STRIDE + 1
    for kw in (dict(sched=bad_sched), dict(ahead=0), dict(ahead=65), dict(staging=4, dst0=4), dict(lag=2), dict(fmt=2), dict(out_cap=10)):
        args = dict(sched=sched, ahead=2, staging=30000)
        args.update(kw)
        with pytest.raises(_abi.Q3Error):
            native.k_doc_stream(x, kinds, args.pop("sched"), args.pop("ahead"), args.pop("staging"), **args)


# ---- the session ---------------------------------------------------------------------------------------------------------------
# tests/test_longdoc_gpu.py's seven segments: EOS masked by min_frames, so every length is known and none is a multiple of the 4-frame chunk
MAX_STEPS = [4, 5, 8, 12, 4, 9, 1]
KINDS = [3, 2, 4, 1, 3, 2, 0]
SAMPLER = dict(temperature=0.7, top_k=40, top_p=0.9, min_frames=64)
SEED = 900
WAIT_MS = 30000   # (a bound against a hang, never reached by a passing run)
INVALID, STATE = -1, -5


def _segments():
    return [(np.arange(100 + 10 * i, 105 + 11 * i, dtype=np.uint32), k, m) for i, (k, m) in enumerate(zip(KINDS, MAX_STEPS))]


def _engine(max_batch=2):
    from q3tts import _abi, native
    cfg = _abi.tiny_config(max_batch=max_batch, n_ctx=256, with_vocoder=1)
    eng = native.NativeEngine(cfg)
    d = cfg.model.d_embed
    vdesc, vkeep = native.make_prompt_desc(None, spk_emb=((np.arange(d) % 13 - 6) * 0.03125).astype(np.float32), part="voice")
    return eng, vdesc, vkeep


def _plain_requests(px):
    from q3tts import native
    reqs, keep = [], []
    for i, (ids, _, ms) in enumerate(_segments()):
        desc, k = native.make_prompt_desc(ids, part="text")
        keep.append(k)
        reqs.append(dict(desc=desc, prefix=px, seed=SEED + i, max_steps=ms, want_pcm=1, **SAMPLER))
    return reqs, keep


@pytest.fixture(scope="module")
def ses_doc():
    """The engine, a ready prefix, the seven segments' own PCM (generate_batch) and the expected document for the default options:
    q3tts_generate_long on the same engine, before any session opens."""
    eng, vdesc, vkeep = _engine(2)
    px = eng.create_prefix(desc=vdesc)
    reqs, rkeep = _plain_requests(px)
    outs = eng.generate_batch(reqs)
    assert [o.status for o in outs] == [0] * 7 and [o.codes.shape[0] for o in outs] == MAX_STEPS
    want = eng.generate_long(_segments(), prefix=px, seed=SEED, **SAMPLER)
    yield dict(eng=eng, vdesc=vdesc, px=px, outs=outs, pcm=[o.pcm for o in outs], want=want, keep=(vkeep, rkeep), bytes0=eng.device_bytes())
    px.close()
    eng.close()


class Got:
    def __init__(self):
        self.chunks, self.segs, self.final, self.res, self.last_chunk_final, self.order_ok = [], [], None, None, False, True


def _consume(ses, stop=None, got=None):
    """Events until every submitted id has its final event (or stop(got, event) says so): {id: Got}; got: what an earlier call collected."""
    from q3tts import _abi
    got = {} if got is None else got
    while ses.open_ids:
        ev = ses.next(WAIT_MS)
        assert ev is not None, "no event within the bound"
        rid, kind, pcm, fin, res = ev
        g = got.setdefault(rid, Got())
        assert g.final is None, "an event behind the final one"
        if kind == _abi.EV_CHUNK:
            g.order_ok &= not g.last_chunk_final
            g.chunks.append(pcm); g.last_chunk_final = fin
        elif kind == _abi.EV_SEGMENT:
            g.order_ok &= res.segment == len(g.segs)
            res.at = sum(c.size for c in g.chunks)      # the samples delivered when the event came
            g.segs.append(res)
        elif kind != _abi.EV_PREFIX:
            g.final, g.res = kind, res
        if stop is not None and stop(got, ev):
            break
    return got


def _pcm(g, dtype=np.float32):
    return np.concatenate(g.chunks) if g.chunks else np.zeros(0, dtype=dtype)


def _check_document(g, want, ses=None, did=None, outs=None):
    """A finished document against q3tts_generate_long's result: the bits, the SEGMENT events and document_info."""
    from q3tts import _abi
    assert g.final == _abi.EV_DONE and g.order_ok and g.last_chunk_final
    got = _pcm(g)
    assert [s.segment for s in g.segs] == list(range(len(want.info)))
    if ses is not None:
        info, n_del = ses.document_info(did)
        assert info == want.info, [(a, b) for a, b in zip(info, want.info) if a != b][:2]
    assert [s.n_samples for s in g.segs] == [f["end"] - f["begin"] for f in want.info]
    assert got.size == want.n_samples and np.array_equal(_bits(got), _bits(want.pcm)), (got.size, want.n_samples, [c.size for c in g.chunks])
    for s, f in zip(g.segs, want.info):
        assert (s.status, s.codes.shape[0], int(s.hit_eos), s.n_samples) == (0, f["n_frames"], f["hit_eos"], f["end"] - f["begin"])
        assert s.at >= f["end"]                          # the piece was out when its event came
    if outs is not None:
        assert all(np.array_equal(s.codes, o.codes) for s, o in zip(g.segs, outs))
    assert g.res.status == 0 and g.res.n_samples == want.n_samples and g.res.codes.shape[0] == 0
    assert g.res.hit_eos == all(f["hit_eos"] for f in want.info)
    if ses is not None:
        info, n_del = ses.document_info(did)
        assert info == want.info and n_del == want.n_samples


def _stream(eng, fmt=0, **kw):
    from q3tts import native
    with native.NativeSession(eng, fmt) as ses:
        did = ses.submit_document(_segments(), seed=SEED, **SAMPLER, **kw)
        got = _consume(ses)
        return got[did], ses.document_info(did)


@pytest.mark.parametrize("how", ["voice", "prefix", "pending"])
def test_document_equals_generate_long(ses_doc, how):
    """Default options, the voice given as a desc, as a ready prefix and as a session prefix that is still pending at submit."""
    from q3tts import native
    d = ses_doc
    with native.NativeSession(d["eng"]) as ses:
        if how == "voice":
            did = ses.submit_document(_segments(), voice=d["vdesc"], seed=SEED, **SAMPLER)
        elif how == "prefix":
            did = ses.submit_document(_segments(), prefix=d["px"], seed=SEED, **SAMPLER)
        else:
            _, spx = ses.create_prefix(desc=d["vdesc"])
            did = ses.submit_document(_segments(), prefix=spx, seed=SEED, **SAMPLER)
        got = _consume(ses)
        _check_document(got[did], d["want"], ses, did, d["outs"])
        assert d["want"].n_samples > 0 and sum(f["hit_eos"] for f in d["want"].info) == 0
        assert got[did].res.n_frames == sum(s.codes.shape[0] for s in got[did].segs) == sum(MAX_STEPS)


def test_identity_options_and_a_trimmed_document(ses_doc):
    d = ses_doc
    eng = d["eng"]
    ident = dict(trim=0, fade=0, pause_ms=(0,) * 5)
    want = eng.generate_long(_segments(), prefix=d["px"], seed=SEED, join=ident, **SAMPLER)
    assert np.array_equal(_bits(want.pcm), _bits(np.concatenate(d["pcm"])))
    g, _ = _stream(eng, prefix=d["px"], join=ident)
    _check_document(g, want)
    # a threshold from the batch's own PCM: the median of the segments' peaks empties the quieter pieces (the comparison is strict)
    peaks = sorted(float(np.abs(x).max()) for x in d["pcm"])
    kw = dict(trim=1, threshold=peaks[3], keep=0, fade=120)
    want = eng.generate_long(_segments(), prefix=d["px"], seed=SEED, join=kw, **SAMPLER)
    empty = [f["begin"] == f["end"] for f in want.info]
    assert any(empty) and not all(empty)
    g, (info, n_del) = _stream(eng, prefix=d["px"], join=kw)
    _check_document(g, want)
    assert info == want.info and n_del == want.n_samples


@pytest.mark.parametrize("ahead", [1, 2, 7])
def test_look_ahead(ses_doc, ahead):
    d = ses_doc
    g, (info, _) = _stream(d["eng"], voice=d["vdesc"], ahead=ahead)
    _check_document(g, d["want"])
    assert info == d["want"].info


@pytest.mark.parametrize("slots", [1, 4])
def test_other_slot_counts(ses_doc, slots):
    eng, vdesc, keep = _engine(slots)
    try:
        want = eng.generate_long(_segments(), voice=vdesc, seed=SEED, **SAMPLER)
        assert np.array_equal(_bits(want.pcm), _bits(ses_doc["want"].pcm))     # (generate_long's own contract)
        g, (info, _) = _stream(eng, voice=vdesc)
        _check_document(g, want)
        assert info == want.info
    finally:
        eng.close()


def test_i16_session(ses_doc):
    from q3tts import _abi
    d = ses_doc
    g, _ = _stream(d["eng"], fmt=_abi.PCM_I16, prefix=d["px"])
    got = _pcm(g, np.int16)
    assert g.final == _abi.EV_DONE and got.dtype == np.int16 and np.array_equal(got, D.pack_i16(d["want"].pcm))


def test_beside_plain_requests_and_two_documents(ses_doc):
    """Three plain requests, one submitted before the document and two once its first chunk is out: their chunks joined are
    generate_batch's PCM and the document is generate_long's. Then two documents at once, with other look-aheads."""
    from q3tts import _abi, native
    d = ses_doc
    reqs, keep = _plain_requests(d["px"])
    with native.NativeSession(d["eng"]) as ses:
        first = ses.submit(**reqs[3])
        did = ses.submit_document(_segments(), prefix=d["px"], seed=SEED, **SAMPLER)
        got = _consume(ses, stop=lambda got, ev: ev[0] == did and ev[1] == _abi.EV_CHUNK)
        late = [ses.submit(**reqs[5]), ses.submit(**reqs[2])]
        _consume(ses, got=got)
        _check_document(got[did], d["want"], ses, did)
        for rid, i in zip([first] + late, (3, 5, 2)):
            assert got[rid].final == _abi.EV_DONE and np.array_equal(_bits(_pcm(got[rid])), _bits(d["pcm"][i]))
            assert np.array_equal(got[rid].res.codes, d["outs"][i].codes)
    with native.NativeSession(d["eng"]) as ses:
        a = ses.submit_document(_segments(), prefix=d["px"], seed=SEED, ahead=2, **SAMPLER)
        b = ses.submit_document(_segments(), voice=d["vdesc"], seed=SEED, ahead=3, **SAMPLER)
        got = _consume(ses)
        _check_document(got[a], d["want"], ses, a)
        _check_document(got[b], d["want"], ses, b)


def test_append(ses_doc):
    """Open with three segments, append four at the first SEGMENT event and close: the bits of the seven at once. An open document
    whose segments are all delivered stays open and silent until it is appended to."""
    from q3tts import _abi, native
    d = ses_doc
    segs = _segments()
    with native.NativeSession(d["eng"]) as ses:
        did = ses.submit_document(segs[:3], prefix=d["px"], seed=SEED, open=True, **SAMPLER)
        got = _consume(ses, stop=lambda got, ev: ev[1] == _abi.EV_SEGMENT)
        ses.append_document(did, segs[3:], close=True)
        _consume(ses, got=got)
        _check_document(got[did], d["want"], ses, did)
    with native.NativeSession(d["eng"]) as ses:
        did = ses.submit_document(segs[:3], prefix=d["px"], seed=SEED, open=True, **SAMPLER)
        got = _consume(ses, stop=lambda got, ev: ev[1] == _abi.EV_SEGMENT and ev[4].segment == 2)
        assert ses.next(100) is None and did in ses.open_ids          # silent, and not finished
        info, n_del = ses.document_info(did)
        assert info == d["want"].info[:3] and n_del == d["want"].info[2]["end"]
        ses.append_document(did, [], close=False)
        ses.append_document(did, segs[3:5])
        ses.append_document(did, segs[5:], close=True)
        _consume(ses, got=got)
        _check_document(got[did], d["want"], ses, did)
        with pytest.raises(_abi.Q3Error, match=r"\(-1\)"):
            ses.append_document(did, segs[:1])                        # finished


def test_cancel(ses_doc):
    """Cancelled after the second SEGMENT event: no chunk follows, the final event is CANCELLED, what was delivered is a prefix of the
    expected row; a second document is exact afterwards (rows and slots came back); the engine's device bytes are as before."""
    from q3tts import _abi, native
    d = ses_doc
    with native.NativeSession(d["eng"]) as ses:
        did = ses.submit_document(_segments(), prefix=d["px"], seed=SEED, ahead=2, **SAMPLER)
        got = _consume(ses, stop=lambda got, ev: ev[1] == _abi.EV_SEGMENT and ev[4].segment == 1)
        assert d["eng"].device_bytes() == d["bytes0"] + _rows_bytes(d["eng"], 2)     # the document's two rows are counted while it lives
        ses.cancel(did)
        rest = _consume(ses)[did]
        assert rest.chunks == [] and rest.segs == [] and rest.final == _abi.EV_CANCELLED
        assert d["eng"].device_bytes() == d["bytes0"]                                # ... and gone with its final event
        part = _pcm(got[did])
        assert d["want"].info[1]["end"] <= part.size < d["want"].n_samples
        assert np.array_equal(_bits(part), _bits(d["want"].pcm[:part.size]))
        with pytest.raises(_abi.Q3Error, match=r"\(-1\)"):
            ses.append_document(did, _segments()[:1])
        again = ses.submit_document(_segments(), voice=d["vdesc"], seed=SEED, ahead=2, **SAMPLER)
        _check_document(_consume(ses)[again], d["want"], ses, again)
    assert d["eng"].device_bytes() == d["bytes0"]


def _rows_bytes(eng, ahead):
    """What a document of `ahead` rows adds to q3tts_k_device_bytes: the rows (max_steps_cap x 1920 samples, f32) and the edge table."""
    stride = (eng.cfg.max_steps_cap * 1920 + 3) // 4 * 4
    return ahead * stride * 4 + ahead * 8


@pytest.mark.parametrize("when", ["at_once", "first_chunk", "first_segment"])
def test_cancel_while_segments_wait_beside_a_live_document(ses_doc, when):
    """ahead = 7 on two slots: most of the cancelled document's segments wait in the FIFO, and the cancel may meet the very boundary that
    pops one of them. Beside a second, live document whose scans go on: that one is exact, so is a third submitted afterwards, no segment
    of the cancelled one holds a slot, and every row is gone at the end."""
    from q3tts import _abi, native
    d = ses_doc
    with native.NativeSession(d["eng"]) as ses:
        live = ses.submit_document(_segments(), prefix=d["px"], seed=SEED, ahead=3, **SAMPLER)
        gone = ses.submit_document(_segments(), prefix=d["px"], seed=SEED, ahead=7, **SAMPLER)
        got = {}
        if when == "first_chunk":
            _consume(ses, got=got, stop=lambda g, ev: ev[0] == gone and ev[1] == _abi.EV_CHUNK)
        elif when == "first_segment":
            _consume(ses, got=got, stop=lambda g, ev: ev[0] == gone and ev[1] == _abi.EV_SEGMENT)
        ses.cancel(gone)
        n_before = len(got[gone].chunks) if gone in got else 0
        _consume(ses, got=got, stop=lambda g, ev: ev[0] == gone and ev[1] == _abi.EV_CANCELLED)
        assert got[gone].final == _abi.EV_CANCELLED and len(got[gone].chunks) == n_before
        part = _pcm(got[gone])
        assert np.array_equal(_bits(part), _bits(d["want"].pcm[:part.size]))
        third = ses.submit_document(_segments(), prefix=d["px"], seed=SEED, ahead=7, **SAMPLER)
        _consume(ses, got=got)
        _check_document(got[live], d["want"], ses, live)
        _check_document(got[third], d["want"], ses, third)
        assert d["eng"].device_bytes() == d["bytes0"]
    assert d["eng"].device_bytes() == d["bytes0"]


def test_document_refused_for_memory(ses_doc):
    """With the worker told that the device has fewer bytes free than the rows need, the document is FAILED with Q3TTS_ERR_OOM and the
    message names both numbers; nothing was allocated, a plain request beside it is exact, and with the limit lifted a document runs."""
    from q3tts import _abi, native
    d = ses_doc
    reqs, keep = _plain_requests(d["px"])
    need = _rows_bytes(d["eng"], 4)
    with native.NativeSession(d["eng"]) as ses:
        ses.doc_mem_cap(need - 1)
        plain = ses.submit(**reqs[0])
        did = ses.submit_document(_segments(), prefix=d["px"], seed=SEED, ahead=4, **SAMPLER)
        got = _consume(ses)
        assert got[did].final == _abi.EV_FAILED and got[did].res.status == -3 and got[did].chunks == []
        msg = d["eng"].lib.q3tts_last_error(d["eng"].h).decode()
        assert str(need) in msg and str(need - 1) in msg, msg
        assert d["eng"].device_bytes() == d["bytes0"]
        assert got[plain].final == _abi.EV_DONE and np.array_equal(_bits(_pcm(got[plain])), _bits(d["pcm"][0]))
        with pytest.raises(_abi.Q3Error, match=r"\(-1\)"):
            ses.append_document(did, _segments()[:1])
        ses.doc_mem_cap(need)
        ok = ses.submit_document(_segments(), prefix=d["px"], seed=SEED, ahead=4, **SAMPLER)
        _check_document(_consume(ses)[ok], d["want"], ses, ok)


def test_a_failing_segment_fails_the_document(ses_doc):
    """Segment 2 asks for more steps than n_ctx holds behind its prompt: the document is FAILED with the status a plain request of that
    kind gets; a plain request in the same session is unaffected."""
    from q3tts import _abi, native
    d = ses_doc
    segs = _segments()
    segs[2] = (segs[2][0], segs[2][1], 255)
    reqs, keep = _plain_requests(d["px"])
    with native.NativeSession(d["eng"]) as ses:
        bad = ses.submit(**dict(reqs[2], max_steps=255))
        good = ses.submit(**reqs[1])
        did = ses.submit_document(segs, prefix=d["px"], seed=SEED, **SAMPLER)
        got = _consume(ses)
        assert got[bad].final == _abi.EV_FAILED and got[bad].res.status != 0
        assert got[did].final == _abi.EV_FAILED and got[did].res.status == got[bad].res.status
        part = _pcm(got[did])
        assert np.array_equal(_bits(part), _bits(d["want"].pcm[:part.size]))   # what was delivered stays a prefix
        assert got[good].final == _abi.EV_DONE and np.array_equal(_bits(_pcm(got[good])), _bits(d["pcm"][1]))


def test_refusals(ses_doc):
    from q3tts import _abi, native
    d = ses_doc
    eng, segs = d["eng"], _segments()
    bad_kind = [(segs[0][0], 5, 4)]
    with native.NativeSession(eng) as ses:
        base = dict(seed=SEED, **SAMPLER)
        for kw in (dict(prefix=d["px"], ahead=65), dict(prefix=d["px"], ahead=-1), dict(prefix=d["px"], voice=d["vdesc"]), dict(),
                   dict(prefix=d["px"], join=dict(trim=2)), dict(prefix=d["px"], join=dict(fade=-1)), dict(prefix=d["px"], join=dict(threshold=-0.5)),
                   dict(prefix=d["px"], join=dict(pause_ms=(0, 0, 0, 0, 60001))), dict(prefix=d["px"], segments=bad_kind), dict(prefix=d["px"], segments=[]),
                   dict(prefix=d["px"], text_stream=True)):
            kw = dict(kw)
            with pytest.raises(_abi.Q3Error, match=r"\(-1\)"):
                ses.submit_document(kw.pop("segments", segs), **base, **kw)
        assert not ses.open_ids
        with pytest.raises(_abi.Q3Error, match=r"\(-1\)"):
            ses.append_document(12345, segs[:1])                       # unknown
        did = ses.submit_document(segs[:1], prefix=d["px"], **base)    # closed at submit
        with pytest.raises(_abi.Q3Error, match=r"\(-1\)"):
            ses.append_document(did, segs[:1])
        op = ses.submit_document([], prefix=d["px"], open=True, **base)   # (open: no segment yet is fine)
        with pytest.raises(_abi.Q3Error, match=r"\(-1\)"):
            ses.append_document(op, bad_kind)
        ses.append_document(op, [], close=True)
        with pytest.raises(_abi.Q3Error, match=r"\(-5\)"):
            eng.generate_long(segs, prefix=d["px"], **base)            # still refused while the session is open
        got = _consume(ses)
        assert got[did].final == _abi.EV_DONE and got[op].final == _abi.EV_DONE and got[op].res.n_samples == 0 and got[op].last_chunk_final
    for setter, val in ((eng.set_speed, 1250), (eng.set_output_rate, 16000)):
        setter(val)
        try:
            with native.NativeSession(eng) as ses:
                with pytest.raises(_abi.Q3Error, match=r"\(-5\)"):
                    ses.submit_document(segs, prefix=d["px"], seed=SEED, **SAMPLER)
        finally:
            setter(0)

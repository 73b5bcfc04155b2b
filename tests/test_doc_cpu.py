"""Documents in a session without a GPU (include/q3tts.h, "documents in a session: the streaming join"): the streaming
rule restated in tests/_doc_ref.py equals _long_ref.join bit for bit over seeded documents however the segments advance, however many run
ahead, however small the staging buffer is and whether the plan lags a boundary or not; the library's planner, driven the same way
through the host-only hook q3tts_k_doc_plan, returns the model's pieces; the two properties of the pause; the refusal rules."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _doc_ref as D  # noqa: E402
import _long_ref as R  # noqa: E402
from q3tts import _abi, native  # noqa: E402

INVALID, STATE = -1, -5
LENS = [0, 1, 239, 240, 241, 479, 700, 1500, 3001, 5000]
STEPS = [7, 100, 240, 777, 1920]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


class LibPlanner:
    """q3_doc_plan behind tests/_doc_ref.py's planner interface: one q3tts_k_doc_plan call per boundary, the state kept by the caller."""

    def __init__(self, o, rate=24000):
        self.o, self.rate = o, rate
        self.state = np.zeros(7, dtype=np.int64)

    @property
    def head(self):
        return int(self.state[0])

    def step(self, segs, room):
        sg = np.array([[n, f, l, int(c), k] for n, f, l, c, k in segs], dtype=np.int32)
        pieces, done = native.k_doc_plan(sg, room, self.state, rate=self.rate, **self.o)
        return [tuple(int(v) for v in p) for p in pieces], [tuple(int(v) for v in d) for d in done]


def _row(rng, n, mode):
    """mode 0: silent (below the threshold); 1: a loud stretch somewhere; 2: loud from the first to the last sample; 3: loud in the middle only."""
    x = (rng.standard_normal(n) * 0.002).astype(np.float32)
    if n and mode == 1:
        a = int(rng.integers(0, n)); b = int(rng.integers(a, n)) + 1
        x[a:b] += (rng.standard_normal(b - a) * 0.3).astype(np.float32)
    elif n and mode == 2:
        x[0], x[n - 1] = 0.5, -0.5
    elif n and mode == 3:
        x[n // 2] = 0.7
    return x


def _case(t):
    """Case t of the sweep. Every 8th document is built to a pattern (silent rows first / in the middle / last, only empty pieces);
    staging 1 goes with short rows and short pauses, a 60 000 ms pause with a staging buffer that takes it in a few boundaries."""
    rng = np.random.default_rng(27000 + t)
    ns = int(rng.integers(1, 7))
    tiny = t % 5 == 0                      # a staging buffer of 1..7 samples
    lens = [int(rng.choice(LENS[:6] if tiny else LENS)) for _ in range(ns)]
    modes = [int(rng.integers(0, 4)) for _ in range(ns)]
    pat = t % 8
    if pat == 1:
        modes[0] = 0
    elif pat == 2 and ns > 2:
        modes[ns // 2] = 0
    elif pat == 3:
        modes[-1] = 0
    elif pat == 4:
        modes = [0] * ns
    rows = [_row(rng, n, m) for n, m in zip(lens, modes)]
    for x in rows:
        if x.size and rng.integers(0, 5) == 0:
            x[int(rng.integers(0, x.size))] = np.nan
    kinds = [int(rng.integers(0, 5)) for _ in range(ns)]
    sched = [D.schedule(n, int(rng.choice(STEPS))) for n in lens]
    fade = int(rng.choice([0, 1, 120, 500, 4000]))          # 4000: above L / 2 of every row, and 2 * fade above every row
    kw = dict(trim=int(rng.integers(0, 2)), keep=int(rng.choice([0, 100, 480, 10**6])), fade=fade,
              threshold=float(rng.choice([0.0, 0.01, 0.5])))
    if tiny:
        kw["pause_ms"] = tuple(int(p) for p in rng.choice([0, 1, 5], 5))
        staging = int(rng.choice([1, 2, 7]))
    elif t % 49 == 7:
        kw["pause_ms"] = (0, 60000, 60000, 0, 60000)
        staging = 700000
    else:
        kw["pause_ms"] = tuple(int(p) for p in rng.choice([0, 10, 150, 600], 5))
        staging = int(rng.choice([240, 1000, 7680, 30720]))
    return rows, kinds, sched, int(rng.integers(1, 4)), staging, int(rng.integers(0, 2)), kw


N_CASES = 2400


@pytest.mark.parametrize("part", range(8))
def test_stream_equals_join_and_library_plans_the_same(part):
    """N_CASES seeded documents in eight parts: the model's concatenation == _long_ref.join (samples, plan, N); every boundary fits the
    staging buffer; the library's planner returns the model's pieces, boundary by boundary, and the same plan."""
    seen = dict(empty_doc=0, some_empty=0, nan=0, tiny=0, long_pause=0, lag=0, fade_over=0)
    for t in range(part, N_CASES, 8):
        rows, kinds, sched, ahead, staging, lag, kw = _case(t)
        J, plan, N = R.join(rows, kinds, **kw)
        S, chunks, got_plan, trace = D.drive(rows, kinds, sched, ahead, staging, lag=lag, **kw)
        assert S.size == N and np.array_equal(_bits(S), _bits(J)), (t, kw)
        assert np.array_equal(got_plan, plan), (t, kw)
        assert max(chunks) <= staging and sum(chunks) == N
        S2, chunks2, lib_plan, lib_trace = D.drive(rows, kinds, sched, ahead, staging, lag=lag, planner=LibPlanner(R.opts(**kw)), **kw)
        assert lib_trace == trace, (t, kw, next((a, b) for a, b in zip(lib_trace, trace) if a != b))
        assert np.array_equal(lib_plan, plan) and chunks2 == chunks
        empty = [int(p[2] == p[3]) for p in plan]
        seen["empty_doc"] += all(empty); seen["some_empty"] += 0 < sum(empty) < len(empty)
        seen["nan"] += any(np.isnan(x).any() for x in rows); seen["tiny"] += staging <= 7; seen["long_pause"] += max(kw["pause_ms"]) == 60000
        seen["lag"] += lag; seen["fade_over"] += any(0 < p[1] - p[0] < 2 * kw["fade"] for p in plan)
    assert all(v > 0 for v in seen.values()), seen


def test_lengths_around_the_block_and_under_two_fades():
    """Every length of the list as a document of its own and as the middle of three, trim on and off, fades 0 / 1 / 120 / above L / 2,
    keep 0 and beyond the row, a staging buffer of one sample, steps that are no multiple of 240."""
    rng = np.random.default_rng(5)
    for n in (0, 1, 239, 240, 241, 479, 100, 3001):
        for trim in (0, 1):
            for fade in (0, 1, 120, 2000):
                for keep in (0, 10**6):
                    mid = _row(rng, n, 2)
                    rows = [_row(rng, 300, 2), mid, _row(rng, 250, 2)]
                    kinds = [4, 1, 0]
                    kw = dict(trim=trim, keep=keep, fade=fade, pause_ms=(0, 2, 1, 0, 3))
                    for doc, kd in ((rows, kinds), ([mid], [0])):
                        J, plan, N = R.join(doc, kd, **kw)
                        for ahead, staging, step, lag in ((1, 1, 7, 0), (2, 100, 77, 1), (3, 10**6, 1920, 1)):
                            S, chunks, got, _ = D.drive(doc, kd, [D.schedule(x.size, step) for x in doc], ahead, staging, lag=lag, **kw)
                            assert np.array_equal(_bits(S), _bits(J)) and np.array_equal(got, plan), (n, kw, ahead, staging)


def _segs(*s):
    return np.array(s, dtype=np.int32)


def test_pause_waits_for_a_non_empty_piece():
    """A pause is never emitted before the piece behind it is known to be non-empty: with the first piece delivered and the second
    segment open but silent so far, nothing goes out, however long that lasts; the first loud block releases the pause."""
    kw = dict(trim=1, threshold=0.01, keep=0, fade=0, pause_ms=(0, 0, 0, 300, 0))
    for planner in (D.Planner(R.opts(**kw)), LibPlanner(R.opts(**kw))):
        first = (480, 0, 1, True, 3)
        pieces, done = planner.step([first, (0,) + D.NONE + (False, 0)], 10**6)
        assert pieces == [(0, 0, 0, 480, 480, 0)] and done == [(0, 0, 480, 0, 480)]
        for n in (240, 2400, 24000):                       # silent so far: no pause yet
            assert planner.step([first, (n,) + D.NONE + (False, 0)], 10**6) == ([], [])
        pieces, done = planner.step([first, (24240, 100, 100, False, 0)], 10**6)
        assert pieces == [(-1, 0, 0, 7200, 0, 0), (1, 24000, 0, 240, -1, 0)] and done == []


def test_dropped_piece_does_not_swallow_a_paragraph_pause():
    """Three segments, the middle one silent and of kind PARAGRAPH, the first of kind CLAUSE: the pause in front of the third piece is the
    paragraph's. The same when the silent segment closes boundaries after the first piece went out."""
    kw = dict(trim=1, threshold=0.01, keep=0, fade=0, pause_ms=(0, 0, 150, 300, 600))
    for planner in (D.Planner(R.opts(**kw)), LibPlanner(R.opts(**kw))):
        a, c = (240, 0, 0, True, R.CLAUSE), (240, 0, 0, True, R.END)
        pieces, done = planner.step([a, (480,) + D.NONE + (False, R.PARAGRAPH), c], 10**6)
        assert pieces == [(0, 0, 0, 240, 240, 0)] and done == [(0, 0, 240, 0, 240)]
        pieces, done = planner.step([a, (960,) + D.NONE + (True, R.PARAGRAPH), c], 10**6)
        assert pieces == [(-1, 0, 0, 14400, 0, 0), (2, 0, 0, 240, 240, 0)]
        assert done == [(1, 0, 0, 240, 240), (2, 0, 240, 240 + 14400, 480 + 14400)]
    # and against the join: rows, not states
    rng = np.random.default_rng(9)
    rows = [_row(rng, 500, 2), _row(rng, 700, 0), _row(rng, 300, 2)]
    kinds = [R.CLAUSE, R.PARAGRAPH, R.END]
    J, plan, N = R.join(rows, kinds)
    S, _, got, _ = D.drive(rows, kinds, [D.schedule(x.size, 100) for x in rows], 2, 1000, lag=1)
    assert np.array_equal(_bits(S), _bits(J)) and np.array_equal(got, plan)
    assert plan[2][2] - plan[0][3] == 600 * 24 and plan[1][2] == plan[1][3] == plan[0][3]


def test_clipping_to_the_staging_buffer():
    """A boundary that could emit a tail, two whole pieces and two pauses hands out exactly `room` samples per call, pause included, and
    picks up where it stopped."""
    kw = dict(trim=0, keep=0, fade=0, pause_ms=(0, 0, 0, 1, 0))
    segs = [(100, 0, 0, True, 3), (50, 0, 0, True, 3), (30, 0, 0, True, 0)]
    for mk in (lambda: D.Planner(R.opts(**kw)), lambda: LibPlanner(R.opts(**kw))):
        p = mk()
        pieces, done = p.step(segs, 10**6)
        assert pieces == [(0, 0, 0, 100, 100, 0), (-1, 0, 0, 24, 0, 0), (1, 0, 0, 50, 50, 0), (-1, 0, 0, 24, 0, 0), (2, 0, 0, 30, 30, 0)]
        assert done == [(0, 0, 100, 0, 100), (1, 0, 50, 124, 174), (2, 0, 30, 198, 228)]
        p, got, n_done = mk(), [], 0
        while p.head < 3:
            pieces, done = p.step(segs, 10)
            assert sum(c for _, _, _, c, _, _ in pieces) == min(10, 228 - sum(got))
            got.append(sum(c for _, _, _, c, _, _ in pieces)); n_done += len(done)
        assert sum(got) == 228 and n_done == 3 and len(got) == 23


def test_document_length_limit():
    """A delivered length that would pass 2^28 samples is Q3TTS_ERR_INVALID at the segment that would pass it; the model raises there too."""
    kw = dict(trim=0, keep=0, fade=0, pause_ms=(0, 0, 0, 60000, 0))
    segs = [(100, 0, 0, True, 3), (50, 0, 0, True, 0)]
    rate = 5_000_000                                   # 60 000 ms are 3e8 samples: past 2^28 on their own
    with pytest.raises(OverflowError):
        D.Planner(R.opts(**kw), rate).step(segs, 10**6)
    p = LibPlanner(R.opts(**kw), rate)
    with pytest.raises(_abi.Q3Error, match="2\\^28 samples at segment 1"):
        p.step(segs, 10**6)
    ok = LibPlanner(R.opts(**kw), 24000)
    assert len(ok.step(segs, 10**7)[1]) == 2            # (1 440 000 zeros and both pieces)


def test_document_rules():
    lib = _abi.load_library()
    for s in ("q3tts_doc_default_opts", "q3tts_k_doc_rules", "q3tts_k_doc_plan", "q3tts_k_doc_stream"):
        assert s in _abi.SYMBOLS and hasattr(lib, s), s
    d = native.doc_opts()
    assert (d.ahead, d.open, d.join.trim, d.join.keep, d.join.fade, list(d.join.pause_ms)) == (0, 0, 1, 480, 120, [0, 0, 150, 300, 600])
    assert abs(d.join.threshold - 0.01) < 1e-9
    K = [3, 2, 4, 1, 0]
    assert native.k_doc_rules(d, K) == (0, "")
    assert native.k_doc_rules(d, K, have_voice=0, have_prefix=1) == (0, "")
    assert native.k_doc_rules(native.doc_opts(ahead=64, open=1), []) == (0, "")
    assert native.k_doc_rules(native.doc_opts(ahead=1), [0] * 1024) == (0, "")
    refused = [
        (dict(o=d, engine_speed=1250), STATE, "q3tts_set_speed"),
        (dict(o=d, engine_rate=16000), STATE, "q3tts_set_output_rate"),
        (dict(o=native.doc_opts(trim=2)), INVALID, "trim"),
        (dict(o=native.doc_opts(threshold=-1.0)), INVALID, "threshold"),
        (dict(o=native.doc_opts(threshold=float("nan"))), INVALID, "threshold"),
        (dict(o=native.doc_opts(keep=-1)), INVALID, "keep"),
        (dict(o=native.doc_opts(fade=-1)), INVALID, "fade"),
        (dict(o=native.doc_opts(pause_ms=(0, 0, 0, 60001, 0))), INVALID, "pause"),
        (dict(o=native.doc_opts(pause_ms=(-1, 0, 0, 0, 0))), INVALID, "pause"),
        (dict(o=native.doc_opts(ahead=-1)), INVALID, "ahead"),
        (dict(o=native.doc_opts(ahead=65)), INVALID, "ahead"),
        (dict(o=native.doc_opts(open=2)), INVALID, "open"),
        (dict(o=d, kinds=[0, 5]), INVALID, "break kind"),
        (dict(o=d, kinds=[-1]), INVALID, "break kind"),
        (dict(o=d, kinds=[]), INVALID, "n_segs"),
        (dict(o=d, kinds=[0] * 1025), INVALID, "n_segs"),
        (dict(o=d, have_voice=1, have_prefix=1), INVALID, "exactly one"),
        (dict(o=d, have_voice=0, have_prefix=0), INVALID, "exactly one"),
        (dict(o=None), INVALID, "NULL"),
    ]
    for kw, status, word in refused:
        kw = dict(kw)
        rc, msg = native.k_doc_rules(kw.pop("o"), kw.pop("kinds", K), **kw)
        assert rc == status and word in msg, (kw, rc, msg)
    assert lib.q3tts_k_doc_rules(None, None, 0, 1, 0, 0, 0, None, 0) == INVALID    # (no message buffer)
    buf = C.create_string_buffer(8)                                                # (a short one: cut, NUL-terminated)
    assert lib.q3tts_k_doc_rules(C.byref(native.doc_opts(ahead=99)), None, 0, 1, 0, 0, 0, buf, 8) == INVALID and len(buf.value) == 7

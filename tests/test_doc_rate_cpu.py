"""Speed and output rate of a streamed document without a GPU ("the pipeline"; include/q3tts.h, "documents in a session"):
the two new option fields and their rules, a Python model of the three-stage flow control (join -> ring RJ -> stretch -> ring RT -> exit;
counts only, no samples) over seeded schedules with the rings at their stated minimum and at a session-like default, the library's
q3tts_k_doc_ring_plan held to the model boundary for boundary, and the output-time maps of q3tts_session_document_info's arithmetic."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _doc_ref as D  # noqa: E402
import _long_ref as R  # noqa: E402
import _resample_ref as RS  # noqa: E402
import _tempo_ref as T  # noqa: E402
from q3tts import _abi, native  # noqa: E402

INVALID = -1
NATIVE = 24000
LENS = [0, 1, 239, 240, 241, 479, 700, 1500, 3001, 5000]
STEPS = [7, 100, 240, 777, 1920]
RATES = [4000, 8000, 16000, 22050, 44100, 48000, 96000]


def test_doc_opts_have_the_two_fields_and_default_to_off():
    names = [f[0] for f in _abi.DocOpts._fields_]
    assert names[-2:] == ["speed_permille", "output_rate"] and names.index("open") == len(names) - 3
    o = native.doc_opts()
    assert (o.speed_permille, o.output_rate) == (0, 0)
    o = _abi.DocOpts()
    o.speed_permille, o.output_rate = 777, 999
    _abi.load_library().q3tts_doc_default_opts(o)
    assert (o.speed_permille, o.output_rate, o.ahead, o.open) == (0, 0, 0, 0)
    o = native.doc_opts(ahead=3, open=1, speed_permille=1250, output_rate=16000, fade=7)
    assert (o.ahead, o.open, o.speed_permille, o.output_rate, o.join.fade) == (3, 1, 1250, 16000, 7)


def test_rules_accept_and_refuse_speed_and_rate():
    for s in (0, 1000, 500, 2000):
        for r in (0, 24000, 4000, 96000):
            assert native.k_doc_rules(native.doc_opts(speed_permille=s, output_rate=r), [0, 3]) == (0, "")
    for s in (499, 2001, -1, 1):
        rc, msg = native.k_doc_rules(native.doc_opts(speed_permille=s), [0])
        assert rc == INVALID and "speed_permille" in msg, (s, rc, msg)
    for r in (3999, 96001, -1, 1):
        rc, msg = native.k_doc_rules(native.doc_opts(output_rate=r), [0])
        assert rc == INVALID and "output_rate" in msg, (r, rc, msg)
    # an engine-level speed or rate still refuses the document, whatever it carries itself
    assert native.k_doc_rules(native.doc_opts(speed_permille=1250), [0], engine_speed=1250)[0] == -5
    assert native.k_doc_rules(native.doc_opts(output_rate=8000), [0], engine_rate=16000)[0] == -5


# ---- the flow control's model ---------------------------------------------------------------------------------------------------
def _ring_min(speed, L, M, H):
    """include/q3tts.h, Q3_DOC_RING_MIN_*: the span over which one frame, or one output, becomes decidable, up to a multiple of 4."""
    step = -(-M // L) if L else 0
    up4 = lambda v: (v + 3) & ~3  # noqa: E731
    mj = T.HS * T.SPEED_MAX // 1000 + T.HOLD - T.DMIN if speed else up4(2 * H + 1 + step)
    mt = 0 if not speed else (up4(2 * H + 1 + step + T.HS) if L else T.HS)
    return mj, mt


class Flow:
    """Three counts — nj samples joined, kt frames decided, m outputs delivered — and what one boundary may move. Every read a stage
    performs is asserted to lie in what its source ring still holds at that moment, [written - C, written), from the worst case of the
    arithmetic itself (delta = DMIN for a frame's template, (m M) div L - H for an output) rather than from the bound the host uses."""

    def __init__(self, speed, L, M, H, cj, ct):
        self.speed, self.L, self.M, self.H, self.cj, self.ct = speed, L, M, H, cj, ct
        self.nj = self.kt = self.m = 0
        self.fin_j = False
        self.wt = 0  # stretched samples written

    def _rate_low(self):
        return max(0, self.m * self.M // self.L - self.H)

    def room(self):
        if self.speed:
            low = 0 if self.kt == 0 else max(0, T.a_k(self.kt - 1, self.speed) + T.DMIN)
        else:
            low = self._rate_low()
        return max(0, low + self.cj - self.nj)

    def _frames(self, fin):
        if fin:
            return -(-T.N_t(self.nj, self.speed) // T.HS)
        k = self.kt
        while T.need(k, self.speed) + T.HOLD <= self.nj:
            k += 1
        return k

    def step(self, joined, fin_j, room_out):
        assert 0 <= joined <= self.room() and (not self.fin_j or (joined == 0 and fin_j))
        self.nj += joined
        self.fin_j = fin_j
        held_j = self.nj - self.cj        # RJ holds [held_j, nj)
        k_from = k_to = self.kt
        nx, fin_x = self.nj, fin_j
        if self.speed:
            s = self.speed
            low_t = self._rate_low() if self.L else self.m
            k_to = max(self.kt, min(self._frames(fin_j), (low_t + self.ct) // T.HS))
            for k in range(k_from, k_to):
                if k >= 1:  # the template at p_{k-1} + Hs with delta_{k-1} = DMIN at the worst, the candidates from a_k + DMIN
                    lowest = min(T.a_k(k - 1, s) + T.DMIN + T.HS, T.a_k(k, s) + T.DMIN)
                    assert max(0, lowest) >= held_j, ("a frame reads an overwritten sample of RJ", k, lowest, held_j)
                assert fin_j or T.need(k, s) + T.HOLD <= self.nj
            NT = T.N_t(self.nj, s)
            self.kt = k_to
            fin_x = fin_j and k_to == -(-NT // T.HS)
            nx = min(k_to * T.HS, NT) if fin_j else k_to * T.HS
            if k_to > k_from:  # the exit's oldest unread position of RT survives these frames
                assert k_to * T.HS - self.ct <= low_t, ("the stretch overwrites an unread sample of RT", k_to, low_t)
            self.wt = max(self.wt, nx)
        if self.L:
            avail = RS.N(nx, self.L, self.M) if fin_x else RS.D(nx, self.L, self.M, self.H)
        else:
            avail = nx
        first, count = self.m, max(0, min(avail - self.m, room_out))
        held_x = (self.wt - self.ct) if self.speed else held_j
        if count > 0:
            lowest = first * self.M // self.L - self.H if self.L else first
            assert max(0, lowest) >= held_x, ("an output reads an overwritten sample", first, lowest, held_x)
            if self.L and not fin_x:
                assert (first + count - 1) * self.M // self.L + self.H < nx
        self.m += count
        # decidable work that needs no new input and was held back by the free space of RT or by room_out alone
        pending = self.m < avail or (bool(self.speed) and self.kt < self._frames(fin_j))
        return dict(joined=joined, k_from=k_from, k_to=k_to, nt=nx if self.speed else 0, nx=nx, fin_x=int(fin_x), first=first, count=count,
                    all_out=int(fin_x and self.m == avail), pending=int(pending))


def _case(t):
    rng = np.random.default_rng(31000 + t)
    ns = int(rng.integers(1, 6))
    tiny = t % 5 == 0                      # a staging room of 1..7 output samples
    lens = [int(rng.choice(LENS[:7] if tiny else LENS)) for _ in range(ns)]
    modes = [int(rng.integers(0, 3)) for _ in range(ns)]
    if t % 8 == 1:
        modes[0] = 0
    elif t % 8 == 2:
        modes[-1] = 0
    rows = []
    for n, mode in zip(lens, modes):
        x = np.zeros(n, dtype=np.float32)
        if n and mode == 1:
            x[int(rng.integers(0, n))] = 0.5
        elif n and mode == 2:
            x[0], x[n - 1] = 0.5, -0.5
        rows.append(x)
    kinds = [int(rng.integers(0, 5)) for _ in range(ns)]
    long_pause = t % 16 == 7 and not tiny
    pause = [int(rng.integers(0, 60001 if long_pause else 200)) for _ in range(5)]
    o = dict(trim=int(rng.integers(0, 2)), keep=int(rng.choice([0, 100, 480])), fade=int(rng.choice([0, 1, 120, 400])), pause_ms=tuple(pause))
    sched = [D.schedule(n, int(rng.choice(STEPS))) if n else [0] for n in lens]
    which = t % 3                          # a speed, a rate, both
    speed = 0 if which == 1 else int(rng.choice([500, 501, 800, 999, 1001, 1250, 1999, 2000]))
    rate = 0 if which == 0 else int(rng.choice(RATES))
    room_out = int(rng.integers(1, 8)) if tiny else int(rng.choice([250, 1000, 7680, 40000]))
    at_min = t % 2 == 0
    # every 7th case: the staging buffer is full of other requests' chunks (no room at all) at boundaries chosen by the seed, and always at
    # the last boundary at which one of the document's segments still runs
    zeros = rng.integers(0, 2, size=4096).astype(bool) if t % 7 == 3 else None
    return rows, kinds, sched, o, speed, rate, (room_out, zeros), at_min, int(rng.integers(1, 4)), int(rng.integers(0, 2))


@pytest.mark.parametrize("block", range(6))
def test_flow_control_model_and_library(block):
    """60 seeded schedules per block: no write passes a read, every schedule ends with all outputs delivered — also with both rings at
    their minimum and a staging room of one sample —, the total is N(N_t(|J|)), and q3tts_k_doc_ring_plan agrees at every boundary.
    The worker's rule: a boundary after which no segment runs, no snapshot is on its way, nothing moved and nothing is `pending` is one
    after which the session sleeps — it must not come before the document is out, also when a boundary had no staging room at all."""
    for t in range(block * 60, block * 60 + 60):
        rows, kinds, sched, o, speed, rate, (room_base, zeros), at_min, ahead, lag = _case(t)
        L = M = H = 0
        if rate:
            L, M, H = RS.plan(NATIVE, rate)[:3]
        mj, mt = _ring_min(speed, L, M, H)
        cj, ct = (mj, mt) if at_min else (mj + 2 * 7680 + (4 if t % 4 == 1 else 0), (mt + 2 * T.N_t(7680, speed) + T.HS + 3) & ~3 if speed else 0)
        fl = Flow(speed, L, M, H, cj, ct)
        state = np.zeros(4, dtype=np.int64)
        oo = R.opts(**o)
        pl = D.Planner(oo)
        ed = [D.Edges(oo["threshold"]) for _ in rows]
        ns = len(rows)
        pos, n, closed = [-1] * ns, [0] * ns, [False] * ns
        prev = [(0,) + D.NONE + (False, kinds[i]) for i in range(ns)]
        bounds, total, ran = 0, 0, True
        while True:
            bounds += 1
            assert bounds < 400000, t
            for i in range(pl.head, min(ns, pl.head + ahead)):
                if not closed[i]:
                    pos[i] += 1
                    nn = sched[i][pos[i]]
                    closed[i] = pos[i] == len(sched[i]) - 1
                    ed[i].update(rows[i], n[i], nn)
                    n[i] = nn
            now = [(n[i], ed[i].first, ed[i].last, closed[i], kinds[i]) for i in range(ns)]
            last_run = ran and all(closed)              # the last boundary at which a segment of the document ran
            ran = not all(closed)
            room_out = 0 if zeros is not None and (last_run or zeros[bounds % zeros.size]) else room_base
            room = fl.room()
            pieces, _ = pl.step(prev if lag else now, room)
            in_flight = bool(lag) and prev != now       # (lag 1: this boundary's snapshot rides its copy and is planned from at the next)
            prev = now
            joined = sum(p[3] for p in pieces)
            fin_j = pl.head >= ns
            want = fl.step(joined, fin_j, room_out)
            got = native.k_doc_ring_plan(state, joined, int(fin_j), room_out, speed_permille=speed, output_rate=rate, ring_j=cj, ring_t=ct)
            assert (got["min_j"], got["min_t"], got["room"]) == (mj, mt, room), (t, bounds, got)
            assert {k: got[k] for k in want} == want, (t, bounds, got, want)
            assert list(state) == [fl.nj, int(fl.fin_j), fl.kt, fl.m]
            total += want["count"]
            moved = joined > 0 or want["k_to"] > want["k_from"] or want["count"] > 0
            if fin_j and room_out > 0:  # nothing new can arrive: every boundary with room moves something until the document is out
                assert moved or want["all_out"], (t, bounds, want)
            awake = ran or in_flight or moved or want["pending"]
            assert awake or want["all_out"], ("the worker would sleep with audio undelivered", t, bounds, want)
            if want["all_out"]:
                break
        J, _, NJ = R.join([r for r in rows], kinds, **o)
        assert fl.nj == NJ
        nt = T.N_t(NJ, speed) if speed else NJ
        assert total == (RS.N(nt, L, M) if rate else nt), t


def test_ring_minima_cover_the_decidable_span():
    """The header's figures, recomputed: over every speed and k < 1200 a frame becomes decidable within 1280 samples of the lowest
    position it may read; an output within T = 2 H + 1 samples of its own."""
    worst = 0
    for s in range(T.SPEED_MIN, T.SPEED_MAX + 1):
        a = (np.arange(1200, dtype=np.int64) * T.HS * s) // 1000
        need = np.maximum(a[1:], a[:-1] + T.HS)
        worst = max(worst, int((need + T.HOLD - (a[:-1] + T.DMIN)).max()))
    assert worst <= 1280 == _ring_min(1000, 0, 0, 0)[0]
    for rate, H in ((4000, 207), (8000, 104), (48000, 35), (96000, 35)):
        L, M, h = RS.plan(NATIVE, rate)[:3]
        assert h == H and _ring_min(0, L, M, H)[0] >= 2 * H + 1 + -(-M // L)


def test_ring_plan_refuses_small_or_misaligned_rings():
    st = np.zeros(4, dtype=np.int64)
    for kw in (dict(speed_permille=1250, ring_j=1276), dict(speed_permille=1250, ring_j=1282), dict(speed_permille=1250, ring_t=252),
               dict(output_rate=8000, ring_j=208), dict(speed_permille=800, output_rate=8000, ring_t=464), dict()):
        with pytest.raises(_abi.Q3Error):
            native.k_doc_ring_plan(st, 10, 0, 10, **kw)
    assert native.k_doc_ring_plan(st, 10, 0, 10, speed_permille=1250, ring_j=1280, ring_t=256)["joined"] == 10


def test_out_maps_of_the_library_equal_the_restatement():
    """out_begin / out_end: ceil(s 1000 / speed), then ceil(s L / M) — the session's own function (q3tts_k_doc_out_pos) against
    _long_ref.out_maps."""
    import ctypes as C
    lib = _abi.load_library()
    rng = np.random.default_rng(5)
    plan = np.zeros((40, 4), dtype=np.int64)
    plan[:, 2] = np.sort(rng.integers(0, 1 << 27, size=40))
    plan[:, 3] = plan[:, 2] + rng.integers(0, 100000, size=40)
    plan[0, 2:] = 0
    for speed, rate in ((0, 0), (1000, 24000), (1250, 0), (0, 8000), (800, 44100), (2000, 96000), (500, 4000)):
        want = R.out_maps(plan, speed, rate)
        for (b, e), (wb, we) in zip(plan[:, 2:], want):
            got = []
            for s in (int(b), int(e)):
                v = C.c_int64(-1)
                assert lib.q3tts_k_doc_out_pos(s, speed, NATIVE, rate, C.byref(v)) == 0
                got.append(v.value)
            assert tuple(got) == (wb, we)

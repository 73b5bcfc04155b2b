"""Documents in a session (include/q3tts.h, "documents in a session: the streaming join") restated over numpy: the
streaming rule as a planner that sees the segments' state boundary by boundary, and a model of a session around it — segments advance
by given per-boundary lengths, at most `ahead` of them run, a boundary's emission is clipped to a staging size, and the plan may be made
from the previous boundary's state (lag = 1, the session's form). The join itself is _long_ref's: what the model emits, concatenated,
must equal _long_ref.join with `==`. The library's q3_doc_plan is driven through the same `drive` and held to the model's pieces."""
import numpy as np

import _long_ref as R

W = R.W
NONE = (2**31 - 1, -1)
MAX_SAMPLES = R.MAX_SAMPLES


class Edges:
    """first / last loud block of x[0, n) kept up to date range by range, as k_doc_scan keeps it: every block that intersects the new
    range is looked at again, over its valid part."""

    def __init__(self, threshold):
        self.thr = np.float32(threshold)
        self.first, self.last = NONE

    def update(self, x, n_prev, n_now):
        for b in range(n_prev // W, -(-n_now // W)):
            blk = np.abs(np.asarray(x[b * W:min((b + 1) * W, n_now)], dtype=np.float32))
            with np.errstate(invalid="ignore"):
                if (blk > self.thr).any():      # strict; a NaN compares false
                    self.first, self.last = min(self.first, b), max(self.last, b)


class Planner:
    """The streaming rule. step(segs, room): segs[j] = (n, first, last, closed, kind) as of the snapshot; returns (pieces, done) with
    pieces = [(seg, src, j0, count, L, F)] (seg -1: `count` zeros; L -1: the segment is open) and done = [(seg, lo, hi, begin, end)]."""

    def __init__(self, o, rate=24000):
        self.o, self.rate = o, rate
        self.head = self.emitted = self.delivered = self.begin = 0
        self.pause = None          # zeros still owed in front of the head's first sample (None: not fixed yet)
        self.prev, self.kmax = False, 0

    def _advance(self):
        self.head += 1
        self.emitted, self.pause = 0, None

    def step(self, segs, room):
        o, pieces, done = self.o, [], []
        while self.head < len(segs):
            n, first, last, closed, kind = segs[self.head]
            if o["trim"]:
                known = last >= 0
                lo = max(0, first * W - o["keep"]) if known else 0
                hi = min(n, (last + 1) * W + o["keep"]) if known else 0
            else:
                known, lo, hi = n > 0 or not closed, 0, n
            if not known:
                if not closed:
                    break                                   # rule 1: nothing is known about the piece yet
                done.append((self.head, lo, hi, self.delivered, self.delivered))
                if self.prev:
                    self.kmax = max(self.kmax, kind)
                self._advance()
                continue
            if closed:                                      # rule 5
                L = hi - lo
                F, upto = min(o["fade"], L // 2), L
            elif hi - lo >= 2 * o["fade"]:                  # rule 4
                L, F, upto = -1, o["fade"], hi - lo - o["fade"]
            else:
                break
            if upto > self.emitted:
                if self.emitted == 0:                       # rule 6
                    if self.pause is None:
                        self.pause = o["pause_ms"][self.kmax] * self.rate // 1000 if self.prev else 0
                        if self.delivered + self.pause > MAX_SAMPLES:
                            raise OverflowError(self.head)
                    c = min(self.pause, room)
                    if c:
                        pieces.append((-1, 0, 0, c, 0, 0))
                        self.pause -= c; room -= c; self.delivered += c
                    if self.pause:
                        break
                    self.begin = self.delivered
                c = min(upto - self.emitted, room)
                if self.delivered + c > MAX_SAMPLES:
                    raise OverflowError(self.head)
                if c:
                    pieces.append((self.head, lo + self.emitted, self.emitted, c, L, F))
                    self.emitted += c; room -= c; self.delivered += c
                if self.emitted < upto:
                    break
            if not closed:
                break
            done.append((self.head, lo, hi, self.begin, self.begin + L))
            self.prev, self.kmax = True, kind
            self._advance()
        return pieces, done


def render(pieces, rows):
    """The samples of a boundary's pieces: the piece's own with the gains g(j, F) of _long_ref.piece, +0.0 for a pause."""
    out = []
    for seg, src, j0, count, L, F in pieces:
        if seg < 0:
            out.append(np.zeros(count, dtype=np.float32))
            continue
        p = np.array(np.asarray(rows[seg], dtype=np.float32)[src:src + count], dtype=np.float32)
        assert p.size == count
        if F > 0:
            j = np.arange(j0, j0 + count, dtype=np.int64)
            den = np.float32(F + 1)
            m = j < F
            p[m] = p[m] * ((j[m] + 1).astype(np.float32) / den)
            if L >= 0:
                m = j >= L - F
                p[m] = p[m] * ((L - j[m]).astype(np.float32) / den)
        out.append(p)
    return np.concatenate(out) if out else np.zeros(0, dtype=np.float32)


def pack_i16(x):
    """k_pcm_pack's conversion (the reference's WAV rule): (x * 32767) clamped to [-32768, 32767], truncated toward zero."""
    with np.errstate(invalid="ignore"):
        v = np.asarray(x, dtype=np.float32) * np.float32(32767.0)
        v = np.minimum(np.maximum(v, np.float32(-32768.0)), np.float32(32767.0))
    assert not np.isnan(v).any()
    return np.trunc(v).astype(np.int16)


def schedule(n, step):
    """A segment's valid lengths boundary by boundary: multiples of `step`, then n."""
    return list(range(step, n, step)) + [n]


def drive(rows, kinds, sched, ahead, staging, lag=0, rate=24000, planner=None, max_bounds=1 << 20, **kw):
    """The session's model. sched[i]: segment i's valid length after each boundary at which it runs. Returns (out, chunks per boundary,
    plan [n][4] = lo, hi, begin, end, the pieces of every boundary)."""
    o = R.opts(**kw)
    pl = planner if planner is not None else Planner(o, rate)
    ns = len(rows)
    ed = [Edges(o["threshold"]) for _ in rows]
    pos, n, closed = [-1] * ns, [0] * ns, [False] * ns
    now = [(0,) + NONE + (False, kinds[i]) for i in range(ns)]
    prev = list(now)
    out, chunks, trace = [], [], []
    plan = np.zeros((ns, 4), dtype=np.int64)
    while pl.head < ns:
        assert len(chunks) < max_bounds
        for i in range(pl.head, min(ns, pl.head + ahead)):
            if closed[i]:
                continue
            pos[i] += 1
            nn = sched[i][pos[i]]
            closed[i] = pos[i] == len(sched[i]) - 1
            ed[i].update(rows[i], n[i], nn)
            n[i] = nn
        now = [(n[i], ed[i].first, ed[i].last, closed[i], kinds[i]) for i in range(ns)]
        pieces, done = pl.step(prev if lag else now, staging)
        prev = now
        for seg, lo, hi, b, e in done:
            plan[seg] = (lo, hi, b, e)
        y = render(pieces, rows)
        assert y.size <= staging
        out.append(y); chunks.append(y.size); trace.append(pieces)
    return (np.concatenate(out) if out else np.zeros(0, dtype=np.float32)), chunks, plan, trace

"""Long documents (include/q3tts.h, "long documents") restated on the CPU: the splitter's rules over Python strings and
regular expressions, and the join's arithmetic in numpy f32. The library's q3tts_text_split and the two device kernels are held to these
with `==`. The caps below are conditions of the restatement (asserted), not measurements."""
import math
import re
import unicodedata

import numpy as np

END, HARD, CLAUSE, SENTENCE, PARAGRAPH = 0, 1, 2, 3, 4
W = 240                      # the join's block length (10 ms at 24 kHz)
MAX_SEGMENTS = 1024
MAX_SAMPLES = 1 << 28
DEFAULT_TARGET, DEFAULT_MAX = 120, 240
DEFAULTS = dict(trim=1, threshold=0.01, keep=480, fade=120, pause_ms=(0, 0, 150, 300, 600))

WS = " \t\r\n 　"
TERM_ASCII = ".!?"
TERM = TERM_ASCII + "…。！？"
CLOSERS = "\"')]}”’」』）】》"
CLAUSE_WIDE = "，、；："
ABBREVIATIONS = {"mr", "mrs", "ms", "dr", "prof", "sr", "jr", "st", "vs"}

_ws_run = re.compile("[%s]+" % re.escape(WS))
_sentence_end = re.compile("([%s]+)[%s]*" % (re.escape(TERM), re.escape(CLOSERS)))
_letters_before = re.compile(r"[A-Za-z]+\Z")
_clause_mark = re.compile("[,;:](?=[%s])|[%s]" % (re.escape(WS), CLAUSE_WIDE))


class BadUtf8(ValueError):
    def __init__(self, offset):
        super().__init__(f"invalid UTF-8 at byte {offset}")
        self.offset = offset


def speakable(ch):
    return unicodedata.category(ch)[0] in "LN"


def split(raw, target=0, maxb=0):
    """raw: bytes. Returns [(begin, end, kind)] in bytes of raw. Raises BadUtf8 (with .offset) and ValueError for limits out of range."""
    target, maxb = target or DEFAULT_TARGET, maxb or DEFAULT_MAX
    if not 16 <= target <= maxb <= 4096:
        raise ValueError("16 <= target <= max <= 4096")
    try:
        s = bytes(raw).decode("utf-8")
    except UnicodeDecodeError as ex:
        raise BadUtf8(ex.start)
    off = [0]
    for ch in s:
        off.append(off[-1] + len(ch.encode("utf-8")))
    n = len(s)

    # cut events: (position where the unit ends, position where the next begins, kind)
    cuts = []
    for m in _ws_run.finditer(s):
        if m.group().count("\n") >= 2:
            cuts.append((m.start(), m.end(), PARAGRAPH))
    for m in _sentence_end.finditer(s):
        run = m.group(1)
        if all(c in TERM_ASCII for c in run) and not (m.end() == n or s[m.end()] in WS):
            continue
        if run == ".":
            before = _letters_before.search(s[:m.start()])
            if before and (len(before.group()) == 1 or before.group().lower() in ABBREVIATIONS):
                continue
        cuts.append((m.end(), m.end(), SENTENCE))
    cuts.sort()
    cuts.append((n, n, END))

    units, begin = [], 0
    for stop, resume, kind in cuts:
        piece = s[begin:stop]
        b = begin + len(piece) - len(piece.lstrip(WS))
        e = b + len(piece.strip(WS))
        begin = resume
        if not any(speakable(ch) for ch in s[b:e]):
            if kind == PARAGRAPH and units:
                units[-1][2] = PARAGRAPH
            continue
        while off[e] - off[b] > maxb:   # an over-long unit: forced cuts
            lo, hi = off[b] + maxb // 4, off[b] + maxb
            marks = [m.end() for m in _clause_mark.finditer(s, b, e) if lo < off[m.end()] <= hi]
            spaces = [k for k in range(b, e) if s[k] in WS and lo < off[k] <= hi]
            if marks:
                cut, k = marks[-1], CLAUSE
            elif spaces:
                cut, k = spaces[-1], HARD
            else:
                cut, k = max(j for j in range(b, e + 1) if off[j] <= hi), HARD
            units.append([b, b + len(s[b:cut].rstrip(WS)), k])
            b = cut + len(s[cut:e]) - len(s[cut:e].lstrip(WS))
        units.append([b, e, kind])

    spans = []
    for b, e, kind in units:
        if spans and spans[-1][2] != PARAGRAPH and off[e] - off[spans[-1][0]] <= target:
            spans[-1][1], spans[-1][2] = e, kind
        else:
            spans.append([b, e, kind])
    if spans:
        spans[-1][2] = END
    return [(off[b], off[e], k) for b, e, k in spans]


# ---- the join ---------------------------------------------------------------------------------------------------------------
def opts(**kw):
    o = dict(DEFAULTS)
    o.update(kw)
    assert o["trim"] in (0, 1) and o["threshold"] >= 0 and o["keep"] >= 0 and o["fade"] >= 0
    assert len(o["pause_ms"]) == 5 and all(0 <= p <= 60000 for p in o["pause_ms"])
    return o


def loud_edges(x, threshold):
    """(first, last) loud block of the row x, or (2^31 - 1, -1)."""
    x = np.asarray(x, dtype=np.float32)
    nb = -(-x.size // W)
    a = np.zeros(nb * W, dtype=np.float32)
    a[:x.size] = np.abs(x)
    with np.errstate(invalid="ignore"):
        loud = np.flatnonzero((a.reshape(nb, W) > np.float32(threshold)).any(axis=1))   # strict; a NaN compares false
    return (int(loud[0]), int(loud[-1])) if loud.size else (2**31 - 1, -1)


def kept_range(x, o):
    n = int(np.asarray(x).size)
    if not o["trim"]:
        return 0, n
    first, last = loud_edges(x, o["threshold"])
    if last < 0:
        return 0, 0
    return max(0, first * W - o["keep"]), min(n, (last + 1) * W + o["keep"])


def piece(x, lo, hi, fade):
    p = np.array(np.asarray(x, dtype=np.float32)[lo:hi], dtype=np.float32)
    L = hi - lo
    F = min(fade, L // 2)
    if F > 0:
        g = np.arange(1, F + 1, dtype=np.int64).astype(np.float32) / np.float32(F + 1)   # the correctly rounded f32 quotient
        p[:F] = p[:F] * g
        p[L - F:] = p[L - F:] * g[::-1]
    return p


def join(rows, kinds, rate=24000, **kw):
    """rows: the segments' PCM (each its valid samples only). Returns (J f32, plan int64 [n][4] = lo, hi, begin, end, N)."""
    o = opts(**kw)
    assert 1 <= len(rows) <= MAX_SEGMENTS and len(kinds) == len(rows) and all(0 <= k <= 4 for k in kinds)
    parts, plan = [], np.zeros((len(rows), 4), dtype=np.int64)
    cur, prev, kmax = 0, None, 0
    for i, (x, kind) in enumerate(zip(rows, kinds)):
        lo, hi = kept_range(x, o)
        if hi > lo:
            if prev is not None:
                gap = o["pause_ms"][kmax] * rate // 1000
                parts.append(np.zeros(gap, dtype=np.float32))
                cur += gap
            parts.append(piece(x, lo, hi, o["fade"]))
            plan[i] = (lo, hi, cur, cur + hi - lo)
            cur += hi - lo
            prev, kmax = i, kind
        else:
            plan[i] = (lo, hi, cur, cur)
            if prev is not None:
                kmax = max(kmax, kind)
    assert cur <= MAX_SAMPLES
    J = np.concatenate(parts) if parts else np.zeros(0, dtype=np.float32)
    assert J.size == cur
    return J, plan, cur


def out_maps(plan, speed_permille=0, output_rate=0, native=24000):
    """begin / end of every piece through the speed and rate maps: ceil(s 1000 / speed), then ceil(s L / M)."""
    def m(s):
        s = int(s)
        if speed_permille not in (0, 1000):
            s = -(-s * 1000 // speed_permille)
        if output_rate not in (0, native):
            g = math.gcd(native, output_rate)
            s = -(-s * (output_rate // g) // (native // g))
        return s
    return [(m(b), m(e)) for _, _, b, e in np.asarray(plan)]

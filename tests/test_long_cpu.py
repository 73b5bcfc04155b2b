"""Long documents without a GPU (include/q3tts.h, "long documents"): the library's splitter q3tts_text_split against
the restatement tests/_long_ref.py on written-out cases and on seeded random texts, the spans' invariants on every text, and the
properties of the restated join that the device tests then hold the kernels to."""
import ctypes as C

import numpy as np
import pytest

import _long_ref as R
from q3tts import _abi, native

INVALID = -1
E, H, CL, S, P = R.END, R.HARD, R.CLAUSE, R.SENTENCE, R.PARAGRAPH

LONG_COMMAS = ", ".join(["the quick brown fox jumps over the lazy dog"] * 16)[:699] + "."   # one 700-byte sentence with commas
LONG_CJK = "天" * 233 + "好"                                                                # 702 bytes, no marks (234 characters)
LONG_WORD = "a" * 300

# (text, target, max, expected [(slice, kind)])
TABLE = [
    ("Hello world. How are you?", 120, 0, [("Hello world. How are you?", E)]),
    ("Hello world. How are you?", 16, 0, [("Hello world.", S), ("How are you?", E)]),
    ("Dr. Smith paid 3.50 dollars. J. K. Rowling agreed.", 16, 0, [("Dr. Smith paid 3.50 dollars.", S), ("J. K. Rowling agreed.", E)]),
    ("你好。今天天气很好！我们走吧", 16, 0, [("你好。", S), ("今天天气很好！", S), ("我们走吧", E)]),
    ('He said "go." Then left.', 16, 0, [('He said "go."', S), ("Then left.", E)]),
    ("A\n\nB", 120, 0, [("A", P), ("B", E)]),
    ("a\nb", 120, 0, [("a\nb", E)]),
    ("...", 0, 0, []),
    ("   ", 0, 0, []),
    ("", 0, 0, []),
    ("Wait... what?! Yes.", 16, 0, [("Wait... what?!", S), ("Yes.", E)]),
    ("e.g. this and a.b stay. Next one.", 16, 0, [("e.g. this and a.b stay.", S), ("Next one.", E)]),
    ("One.\n\n...\n\nTwo.", 120, 0, [("One.", P), ("Two.", E)]),           # the dropped unit's paragraph break moves back
    ("Mrs. Jones vs. Prof. Lee won. Done.", 16, 0, [("Mrs. Jones vs. Prof. Lee won.", S), ("Done.", E)]),
    ("First.\n \n Second. Third.", 120, 0, [("First.", P), ("Second. Third.", E)]),
    ("完了……好的。", 16, 0, [("完了……", S), ("好的。", E)]),                # U+2026 counts without whitespace behind it
]


def _lib_split(raw, target=0, maxb=0):
    return native.text_split(raw, target, maxb)


def _slices(raw, spans):
    return [(raw[b:e].decode("utf-8"), k) for b, e, k in spans]


@pytest.mark.parametrize("text,target,maxb,want", TABLE)
def test_written_out_cases(text, target, maxb, want):
    raw = text.encode("utf-8")
    got = _lib_split(raw, target, maxb)
    assert _slices(raw, got) == want
    assert got == R.split(raw, target, maxb)


def test_forced_cuts():
    raw = LONG_COMMAS.encode()
    assert len(raw) == 700
    sp = _lib_split(raw)
    assert sp == R.split(raw) and len(sp) >= 3
    assert [k for _, _, k in sp] == [CL] * (len(sp) - 1) + [E]
    assert all(e - b <= 240 and raw[e - 1:e] == b"," for b, e, _ in sp[:-1]) and sp[-1][1] - sp[-1][0] <= 240
    raw = LONG_CJK.encode()
    assert len(raw) == 702
    sp = _lib_split(raw)
    assert sp == R.split(raw) == [(0, 240, H), (240, 480, H), (480, 702, E)]
    raw[0:240].decode("utf-8"), raw[240:480].decode("utf-8")   # code-point boundaries
    sp = _lib_split(("天" * 79 + "a" + "天" * 100).encode())     # 238 bytes, then a 3-byte character across the limit: the cut falls back
    assert sp[0] == (0, 238, H)
    raw = LONG_WORD.encode()
    assert _lib_split(raw) == R.split(raw) == [(0, 240, H), (240, 300, E)]
    raw = ("word " * 80).encode()                               # no marks: the last whitespace in (begin + 60, begin + 240]
    sp = _lib_split(raw)
    assert sp == R.split(raw) and sp[0] == (0, 239, H) and sp[1][0] == 240


def test_bad_input():
    lib = _abi.load_library()
    err = C.create_string_buffer(128)
    n = C.c_int32(-1)
    spans = (_abi.TextSpan * 8)()
    for raw, where in ((b"abc \xff def", 4), (b"ab\xe4\xbd", 2), (b"\xc0\x80", 0), (b"x\xed\xa0\x80", 1), (b"ok. \x80", 4)):
        assert lib.q3tts_text_split(raw, len(raw), 0, 0, spans, 8, C.byref(n), err, len(err)) == INVALID
        assert ("byte %d" % where) in err.value.decode() and n.value == 0
        with pytest.raises(R.BadUtf8) as ex:
            R.split(raw)
        assert ex.value.offset == where
    for target, maxb in ((15, 0), (121, 120), (16, 4097), (300, 0), (-1, 0)):
        assert lib.q3tts_text_split(b"hello", 5, target, maxb, spans, 8, C.byref(n), err, len(err)) == INVALID
        with pytest.raises(ValueError):
            R.split(b"hello", target, maxb)
    assert lib.q3tts_text_split(b"hello", 5, 16, 16, spans, 8, C.byref(n), err, len(err)) == 0 and n.value == 1
    # the count is set even when cap is too small
    raw = b"One. Two. Three! Four. Five. Sixty-six."
    assert len(R.split(raw, 16, 16)) == 3
    assert lib.q3tts_text_split(raw, len(raw), 16, 16, spans, 2, C.byref(n), err, len(err)) == INVALID and n.value == 3
    assert lib.q3tts_text_split(raw, len(raw), 16, 16, None, 0, C.byref(n), None, 0) == INVALID and n.value == 3
    assert lib.q3tts_text_split(b"...", 3, 0, 0, None, 0, C.byref(n), None, 0) == 0 and n.value == 0


ALPHABET = (list("abcdefgHIJKLmrsdtvpof0123456789") + list("天地人你好我们今走吧") + list(R.TERM) + list(R.CLOSERS) + list(",;:") + list(R.CLAUSE_WIDE)
            + [" "] * 10 + ["\n"] * 3 + ["\t", " ", "　", "\r", "-", "(", "“"])


def _check_invariants(raw, spans, maxb):
    text = raw.decode("utf-8")
    bounds = {0}
    for ch in text:
        bounds.add(max(bounds) + len(ch.encode("utf-8")))
    pos = 0
    for b, e, k in spans:
        assert pos <= b < e <= len(raw) and e - b <= maxb and b in bounds and e in bounds and 0 <= k <= 4
        assert not any(R.speakable(ch) for ch in raw[pos:b].decode("utf-8"))
        pos = e
    assert not any(R.speakable(ch) for ch in raw[pos:].decode("utf-8"))
    assert [k for _, _, k in spans][-1:] in ([], [E]) and all(k != E for _, _, k in spans[:-1])


def test_random_texts_equal_the_restatement():
    rng = np.random.default_rng(26)
    for it in range(2000):
        n = int(rng.integers(0, 160))
        raw = "".join(ALPHABET[i] for i in rng.integers(0, len(ALPHABET), n)).encode("utf-8")
        target, maxb = ((0, 0), (16, 16), (16, 40), (40, 64), (120, 240))[it % 5]
        got = _lib_split(raw, target, maxb)
        assert got == R.split(raw, target, maxb), (raw, target, maxb)
        _check_invariants(raw, got, maxb or 240)
    for text, target, maxb, _ in TABLE:
        _check_invariants(text.encode(), _lib_split(text.encode(), target, maxb), maxb or 240)
    for text in (LONG_COMMAS, LONG_CJK, LONG_WORD, "word " * 80):
        _check_invariants(text.encode(), _lib_split(text.encode()), 240)


# ---- the restated join --------------------------------------------------------------------------------------------------------
def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _rows(seed=3, lens=(0, 1, 239, 240, 241, 1000, 4801)):
    rng = np.random.default_rng(seed)
    return [rng.uniform(-1.0, 1.0, n).astype(np.float32) for n in lens]


def test_join_identity_is_the_concatenation():
    rows = _rows()
    rows[3][5] = -0.0
    kinds = [k % 5 for k in range(len(rows))]
    J, plan, N = R.join(rows, kinds, trim=0, fade=0, pause_ms=(0,) * 5)
    want = np.concatenate(rows)
    assert N == want.size and np.array_equal(_bits(J), _bits(want))
    assert [tuple(p) for p in plan[:, :2]] == [(0, r.size) for r in rows]
    assert list(plan[:, 3]) == list(np.cumsum([r.size for r in rows])) and list(plan[:, 2]) == [0] + list(plan[:-1, 3])


def test_threshold_is_strict_and_nan_is_not_loud():
    thr = np.float32(0.01)
    x = np.zeros(1000, dtype=np.float32)
    x[300] = thr
    x[700] = -thr
    assert R.loud_edges(x, thr) == (2**31 - 1, -1) and R.kept_range(x, R.opts()) == (0, 0)
    x[500] = np.nextafter(thr, np.float32(1))
    assert R.loud_edges(x, thr) == (2, 2) and R.kept_range(x, R.opts(keep=0)) == (480, 720)
    x[500] = np.nan
    assert R.loud_edges(x, thr) == (2**31 - 1, -1)
    x[999] = 1.0   # the last, short block; keep reaches past the row's end
    assert R.loud_edges(x, thr) == (4, 4) and R.kept_range(x, R.opts(keep=480)) == (480, 1000)


def test_fades_and_gain():
    x = np.ones(1000, dtype=np.float32)
    p = R.piece(x, 100, 900, 120)
    g = [np.float32(j + 1) / np.float32(121) for j in range(120)]
    assert p.size == 800 and list(p[:120]) == g and list(p[:-121:-1]) == g and np.all(p[120:680] == 1.0)
    assert list(R.piece(x, 0, 3, 120)) == [np.float32(0.5), 1.0, np.float32(0.5)]          # F = L div 2 = 1
    assert list(R.piece(x, 0, 2, 120)) == [np.float32(0.5), np.float32(0.5)] and list(R.piece(x, 0, 1, 120)) == [1.0]


def test_empty_pieces_keep_the_larger_pause():
    loud, quiet = np.full(480, 0.5, dtype=np.float32), np.zeros(480, dtype=np.float32)
    # SENTENCE, then an empty PARAGRAPH segment, then the next: the pause is the paragraph's
    J, plan, N = R.join([loud, quiet, loud], [S, P, E], keep=0, fade=0)
    assert N == 480 + 600 * 24 + 480 and np.all(J[480:480 + 14400] == 0) and J[480 + 14400] == 0.5
    assert [tuple(p) for p in plan] == [(0, 480, 0, 480), (0, 0, 480, 480), (0, 480, 14880, 15360)]
    # the empty one's smaller kind does not shrink it; leading and trailing empties add nothing
    J, plan, N = R.join([quiet, loud, quiet, loud, quiet], [P, S, CL, E, P], keep=0, fade=0)
    assert N == 480 + 300 * 24 + 480 and [tuple(p[2:]) for p in plan] == [(0, 0), (0, 480), (480, 480), (7680, 8160), (8160, 8160)]
    J, plan, N = R.join([quiet, quiet], [P, E])
    assert N == 0 and J.size == 0


def test_offsets_are_consistent_with_n():
    rng = np.random.default_rng(9)
    for it in range(50):
        rows = []
        for n in rng.integers(0, 3000, 6):
            x = np.zeros(n, dtype=np.float32)
            if n and rng.random() < 0.7:
                a, b = sorted(rng.integers(0, n, 2))
                x[a:b + 1] = rng.uniform(-1, 1, b + 1 - a)
            rows.append(x)
        kinds = list(rng.integers(0, 5, 6))
        kw = dict(trim=int(it % 3 > 0), keep=int(rng.integers(0, 600)), fade=int(rng.integers(0, 200)))
        J, plan, N = R.join(rows, kinds, **kw)
        assert J.size == N
        ends = 0
        for (lo, hi, b, e), x in zip(plan, rows):
            assert 0 <= lo <= hi <= x.size and e - b == hi - lo and b >= ends
            ends = e if e > b else ends
        assert ends == N
        maps = R.out_maps(plan, 1250, 8000)
        assert all(ob == -(-(-(-b * 1000 // 1250)) // 3) and oe >= ob for (ob, oe), (_, _, b, e) in zip(maps, plan))

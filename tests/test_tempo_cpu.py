"""The time-stretch without a GPU (include/q3tts.h, "speaking rate"): the counts N_t / D_t of the restatement
tests/_tempo_ref.py and of the library against a brute-force count, chunked feeding against one-shot, every chosen offset against the
float64 sums, tones against the table TEMPO_R (and plain overlap-add failing it), and the refusals that need no device."""
import ctypes as C

import numpy as np
import pytest

import _tempo_ref as R
from q3tts import _abi, native

SPEEDS = (500, 800, 1001, 1250, 2000)
LENS_A = [7680, 15360, 23040]
LENS_B = [1, 255, 640, 641, 7680, 7681, 20000]


def _rows():
    """The four tones and white noise, R.TONE_N samples each."""
    rng = np.random.default_rng(20)
    return np.stack([R.tone(f) for f in R.TONES] + [rng.uniform(-0.5, 0.5, R.TONE_N)]).astype(np.float32)


@pytest.fixture(scope="module")
def one_shot():
    """{speed: the finished rows stretched in one step (the Tempo object)}, shared and left unchanged."""
    out = {}
    x = _rows()
    for s in R.TONE_SPEEDS:
        t = R.Tempo(x, s)
        t.feed([x.shape[1]] * x.shape[0], [True] * x.shape[0])
        out[s] = t
    return out


def test_counts_against_brute_force():
    lib = _abi.load_library()
    for s in SPEEDS:
        last = 0
        for n in range(0, 3001):
            # N_t: the least N with N s >= n 1000
            N = 0
            while N * s < n * 1000:
                N += 1
            # D_t: every frame k is asked on its own; the decidable ones must be the leading ones
            dec = []
            for k in range(0, 40):
                a, a1 = (k * 256 * s) // 1000, ((k - 1) * 256 * s) // 1000
                nd = 0 if k == 0 else max(a, a1 + 256)
                dec.append(nd + 640 <= n)
            lead = dec.index(False)
            assert not any(dec[lead:]), (s, n)
            assert (R.N_t(n, s), R.D_t(n, s)) == (N, 256 * lead), (s, n)
            assert native.k_tempo_counts(n, s) == (N, 256 * lead), (s, n)
            assert 256 * lead >= last and 256 * lead <= N
            last = 256 * lead
    for s, f in ((500, 55), (1000, 28), (2000, 14)):
        assert R.D_t(640, s) == 256 and R.D_t(639, s) == 0 and R.D_t(7680, s) == f * 256
        assert native.k_tempo_counts(7680, s)[1] == f * 256
    big = 1 << 28
    for s in SPEEDS:  # the closed form of the library at a length the loop of the restatement still walks
        assert native.k_tempo_counts(big, s)[0] == -(-big * 1000 // s)
        d = native.k_tempo_counts(big, s)[1] // 256
        assert R.need(d - 1, s) + 640 <= big < R.need(d, s) + 640
    for bad in ((-1, 1000), (10, 499), (10, 2001)):
        n_, d_ = C.c_int64(), C.c_int64()
        assert lib.q3tts_k_tempo_counts(bad[0], bad[1], C.byref(n_), C.byref(d_)) == -1


def test_window():
    w = R.window()
    assert w.dtype == np.float32 and w.size == R.WN and w[0] == 0.0 and w[R.HS] == 1.0
    assert np.max(np.abs((w[:R.HS].astype(np.float64) + w[R.HS:]) - 1.0)) <= 2.0 ** -24
    assert R.HOLD == 640 and R.SPAN == 767


@pytest.mark.parametrize("s", R.TONE_SPEEDS)
def test_chunked_equals_one_shot(one_shot, s):
    x = _rows()
    ref = one_shot[s]
    n = x.shape[1]
    rng = np.random.default_rng(s)
    rand = sorted(int(v) for v in rng.integers(1, n, size=9))
    for lens in (LENS_A, LENS_B, rand):
        t = R.Tempo(x, s)
        for ln in lens:
            nv = t.feed([ln] * x.shape[0], [False] * x.shape[0])
            assert np.all(nv == R.D_t(ln, s))
            # what is out early is final already
            assert t.y[:, :int(nv[0])].tobytes() == ref.y[:, :int(nv[0])].tobytes()
        nv = t.feed([n] * x.shape[0], [True] * x.shape[0])
        assert np.all(nv == R.N_t(n, s))
        assert t.y.tobytes() == ref.y.tobytes() and t.delta == ref.delta
        assert not np.any(np.isnan(t.y[:, :R.N_t(n, s)])) and np.all(np.isnan(t.y[:, R.N_t(n, s):]))


def test_nothing_beyond_the_valid_length_is_read():
    x = _rows()[:, :8000].copy()
    ref = R.Tempo(x, 800)
    ref.feed([8000] * 5, [True] * 5)
    y = x.copy()
    t = R.Tempo(y, 800)
    for ln in (640, 3000, 7681):
        t.x[:, ln:] = np.nan
        nv = int(t.feed([ln] * 5, [False] * 5)[0])
        assert t.y[:, :nv].tobytes() == ref.y[:, :nv].tobytes()
        t.x[:, ln:] = x[:, ln:]


@pytest.mark.parametrize("s", (500, 1250))
def test_every_offset_is_admissible_in_float64(s):
    x = _rows()[[0, 2, 4], :7680 + 17]
    t = R.Tempo(x, s, audit=True)
    t.feed([x.shape[1]] * 3, [True] * 3)
    checked = 0
    for r in range(3):
        assert len(t.audits[r]) == len(t.delta[r]) - 1
        for c64, mag, best in t.audits[r]:
            slack = 2.0 * (R.WN + 1) * 2.0 ** -24 * float(mag.max())
            assert c64[best] >= c64.max() - slack
            checked += 1
    assert checked > 50


def _bounds(f, s):
    """Twice the table's distance from 1; the table is printed to four decimals, so each entry stands for a value up to 5e-5 away (which
    also covers the f32 rounding of the samples, 2^-24 relative). The peak: twice its distance, or one bin, the measurement's resolution."""
    lo, hi, pk = R.TEMPO_R[(f, s)]
    return 1.0 - 2.0 * (1.0 - lo + 5e-5), 1.0 + 2.0 * (hi - 1.0 + 5e-5), max(2.0 * pk, 1.0)


def test_tones_keep_level_and_pitch_and_plain_overlap_add_does_not(one_shot):
    n = R.TONE_N
    for s in R.TONE_SPEEDS:
        for i, f in enumerate(R.TONES):
            lo, hi, pk = R.tone_measures(one_shot[s].y[i, :R.N_t(n, s)], n, s, f)
            blo, bhi, bpk = _bounds(f, s)
            assert blo <= lo and hi <= bhi and pk <= bpk, (f, s, lo, hi, pk)
            y, d = R.stretch(R.tone(f).astype(np.float32), s, search=False)
            assert np.all(d == 0)
            lo, hi, pk = R.tone_measures(y, n, s, f)
            assert R.ola_exact(f, s) or not (blo <= lo and hi <= bhi and pk <= bpk), (f, s, lo, hi, pk)
    assert sum(not R.ola_exact(f, s) for f in R.TONES for s in R.TONE_SPEEDS) >= 13


def test_symbols_and_refusals_without_a_device():
    lib = _abi.load_library()
    for name in ("q3tts_set_speed", "q3tts_get_speed", "q3tts_time_stretch", "q3tts_k_tempo_counts", "q3tts_k_pcm_tempo"):
        assert name in _abi.SYMBOLS and hasattr(lib, name), name
    v = C.c_int32(7)
    n = C.c_int64(7)
    buf = np.zeros(4, dtype=np.float32)
    fp = buf.ctypes.data_as(C.POINTER(C.c_float))
    assert lib.q3tts_set_speed(None, 1250) == -1
    assert lib.q3tts_get_speed(None, C.byref(v)) == -1 and v.value == 7
    assert lib.q3tts_time_stretch(None, fp, 4, 1250, fp, 4, C.byref(n)) == -1 and n.value == 7
    i32 = np.zeros(4, dtype=np.int32)
    ip = i32.ctypes.data_as(C.POINTER(C.c_int32))
    for permille, rows in ((499, 1), (2001, 1), (1250, 0)):  # refused before any device call
        assert lib.q3tts_k_pcm_tempo(0, fp, rows, 4, ip, 1, ip, permille, fp, 4, ip, None, 0, 0, None) == -1

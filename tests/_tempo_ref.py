"""The device time-stretch restated in numpy (include/q3tts.h, "speaking rate"): WSOLA at the vocoder's rate.

    Hs = 256, Wn = 512, delta in [-128, 127], HOLD = 640; s: the speed in per mille, 500..2000; all indices are Python / 64-bit integers
    x[j] = the row, 0 for j < 0 and j >= n;  a_k = (k Hs s) div 1000;  p_{-1} = -Hs, p_0 = 0, p_k = a_k + delta_k
    t[j] = x[p_{k-1} + Hs + j];  c(delta) = sum_{j < Wn} x[a_k + delta + j] t[j], one sequential chain in ascending j, acc = acc + x * t
    delta_k = the first maximum of c in ascending delta
    w[j] = 0.5 - 0.5 cos(2 pi j / Wn) in double, rounded once to f32
    y[k Hs + j] = (w[j + Hs] * x[p_{k-1} + j + Hs]) + (w[j] * x[p_k + j])
    N_t(n) = ceil(n 1000 / s);  frame k decidable iff need_k + HOLD <= n, need_0 = 0, need_k = max(a_k, a_{k-1} + Hs);  D_t(n) = Hs x leading decidable frames

Tempo is the restatement the kernel must equal bit for bit (dtype float32: every product and every sum is one rounded f32 operation), its
float64 twin (dtype float64), and with search = False plain overlap-add (every delta 0). It takes rows in steps of growing valid length,
as the engine feeds the kernel, and never reads at or beyond a row's valid length.

Run as a script (`python tests/_tempo_ref.py`) it measures the float64 twin on tones and prints the TEMPO_R table below."""
import numpy as np

HS, WN, DMIN, ND = 256, 512, -128, 256
HOLD = DMIN + ND - 1 + WN + 1  # 640
SPAN = ND - 1 + WN             # 767
SPEED_MIN, SPEED_MAX = 500, 2000

RATE = 24000
TONES = (110.0, 220.0, 997.0, 3000.0)
TONE_SPEEDS = (500, 800, 1250, 2000)
TONE_N = 3 * 7680 + 17
TONE_AMP = 0.5
RMS_BLOCK = 1024


def window():
    return (0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(WN, dtype=np.float64) / WN)).astype(np.float32)


def N_t(n, s):
    return -(-n * 1000 // s) if n > 0 else 0


def a_k(k, s):
    return (k * HS * s) // 1000


def need(k, s):
    return 0 if k <= 0 else max(a_k(k, s), a_k(k - 1, s) + HS)


def frames(n, s, final):
    """Frames decided for a row of n samples: all of a finished row's, else the leading decidable ones."""
    if final:
        return -(-N_t(n, s) // HS)
    k = 0
    while need(k, s) + HOLD <= n:
        k += 1
    return k


def D_t(n, s):
    return HS * frames(n, s, False)


def valid(n, s, final):
    return N_t(n, s) if final else D_t(n, s)


def _gather(x, n, start, count):
    """x[r, start[r] + i] for i < count, 0 outside [0, n[r]): rows x count; nothing at or beyond n is read."""
    idx = start[:, None] + np.arange(count, dtype=np.int64)[None, :]
    ok = (idx >= 0) & (idx < n[:, None])
    return np.where(ok, np.take_along_axis(x, np.clip(idx, 0, x.shape[1] - 1), axis=1), x.dtype.type(0))


class Tempo:
    """rows [R][stride] stretched at s per mille. feed(lens, final) brings every row up to what lens[r] valid samples (final[r]: all there
    are) decide and returns the outputs each row holds then; y [R][cap] holds them, delta[r] the chosen offsets of the frames decided so
    far. audit = True (with float32): per decided frame k >= 1 of row r, audits[r] gets (c64 [ND], mag [ND], index chosen) — the same
    sums in float64 and sum |x t|, for the sequential-sum bound."""

    def __init__(self, rows, s, dtype=np.float32, search=True, audit=False):
        self.x = np.ascontiguousarray(np.atleast_2d(rows), dtype=dtype)
        self.R, self.stride = self.x.shape
        self.s, self.dtype, self.search, self.audit = int(s), dtype, search, audit
        self.w = window().astype(dtype)
        self.done = np.zeros(self.R, dtype=np.int64)
        self.p = np.zeros(self.R, dtype=np.int64)  # p of the last decided frame (p_0 = 0)
        self.cap = frames(self.stride, self.s, True) * HS
        self.y = np.full((self.R, max(self.cap, 1)), np.nan, dtype=dtype)
        self.delta = [[] for _ in range(self.R)]
        self.audits = [[] for _ in range(self.R)]

    def feed(self, lens, final):
        lens = np.asarray(lens, dtype=np.int64).reshape(self.R)
        final = np.asarray(final, dtype=bool).reshape(self.R)
        assert np.all(lens <= self.stride)
        x, s, w = self.x, self.s, self.w
        target = np.array([frames(int(lens[r]), s, bool(final[r])) for r in range(self.R)], dtype=np.int64)
        lim = np.array([valid(int(lens[r]), s, bool(final[r])) for r in range(self.R)], dtype=np.int64)
        while True:
            act = np.nonzero(self.done < target)[0]
            if act.size == 0:
                break
            k, n, fin = self.done[act], lens[act], final[act]
            first = act[k == 0]
            if first.size:  # p_{-1} = -Hs, p_0 = 0: both terms read x[j]
                x0 = _gather(x[first], lens[first], np.zeros(first.size, dtype=np.int64), HS)
                assert np.all(final[first] | (HS <= lens[first]))
                self._put(first, np.zeros(first.size, dtype=np.int64), (w[None, HS:] * x0) + (w[None, :HS] * x0), lim[first])
                for r in first:
                    self.delta[r].append(0)
                self.p[first] = 0
                self.done[first] = 1
                continue
            ak = np.array([a_k(int(kk), s) for kk in k], dtype=np.int64)
            t0, s0 = self.p[act] + HS, ak + DMIN
            assert np.all(fin | ((t0 + WN <= n) & (s0 + SPAN <= n))), "a decidable frame reads at or beyond n"
            tm, sp = _gather(x[act], n, t0, WN), _gather(x[act], n, s0, SPAN)
            if self.search:
                acc = np.zeros((act.size, ND), dtype=self.dtype)
                for j in range(WN):
                    acc = acc + (sp[:, j:j + ND] * tm[:, j:j + 1])  # one multiply, one add, each rounded
                assert acc.dtype == self.dtype
                best = np.argmax(acc, axis=1)  # the first maximum
                if self.audit:
                    for i, r in enumerate(act):
                        win = np.lib.stride_tricks.sliding_window_view(sp[i].astype(np.float64), WN)  # [ND][WN]
                        t64 = tm[i].astype(np.float64)
                        self.audits[r].append((win @ t64, np.abs(win) @ np.abs(t64), int(best[i])))
            else:
                best = np.full(act.size, -DMIN, dtype=np.int64)
            new = np.take_along_axis(sp, best[:, None] + np.arange(HS)[None, :], axis=1)
            self._put(act, k, (w[None, HS:] * tm[:, :HS]) + (w[None, :HS] * new), lim[act])
            for i, r in enumerate(act):
                self.delta[r].append(DMIN + int(best[i]))
            self.p[act] = ak + DMIN + best
            self.done[act] = k + 1
        return lim

    def _put(self, rows, k, frame, lim):
        assert frame.dtype == self.dtype
        for i, r in enumerate(rows):
            m0 = int(k[i]) * HS
            c = int(min(HS, lim[i] - m0))
            if c > 0:
                self.y[r, m0:m0 + c] = frame[i, :c]


def stretch(x, s, dtype=np.float32, search=True, lens=None):
    """One row: the finished clip x stretched; lens: the valid lengths fed before the final one (chunked feeding)."""
    x = np.asarray(x).reshape(1, -1)
    t = Tempo(x, s, dtype=dtype, search=search)
    for n in (lens or []):
        if n < x.shape[1]:
            t.feed([n], [False])
    nv = t.feed([x.shape[1]], [True])
    return t.y[0, :int(nv[0])].copy(), np.array(t.delta[0], dtype=np.int32)


def tone(f, n=TONE_N):
    return TONE_AMP * np.sin(2.0 * np.pi * f * np.arange(n, dtype=np.float64) / RATE + 0.3)


def tone_measures(y, n, s, f):
    """(lowest, highest block-RMS of y over the input's RMS; the spectral peak's distance from the tone in FFT bins), over the outputs
    decided without the zeros behind the clip (m < D_t(n))."""
    m = (D_t(n, s) // RMS_BLOCK) * RMS_BLOCK
    yy = np.asarray(y[:m], dtype=np.float64)
    r = np.sqrt(np.mean(yy.reshape(-1, RMS_BLOCK) ** 2, axis=1)) / (TONE_AMP / np.sqrt(2.0))
    spec = np.abs(np.fft.rfft(yy * np.hanning(m)))
    return float(r.min()), float(r.max()), float(abs(int(np.argmax(spec)) - f * m / RATE))


# measured by this file's script path on the float64 twin (never on the device); the tests bound the f32 restatement at twice the distance
# from 1 of each RMS ratio, and the peak at the larger of twice its distance and one bin (the measurement's resolution).
# {(tone Hz, speed): (lowest RMS ratio, highest RMS ratio, peak distance in bins)}. The script prints plain overlap-add (search = False) on
# the same inputs beside it, for comparison only: its lowest ratios lie between 0.71 and 0.96 wherever the hop is not a whole number of
# periods of the tone (ola_exact).
TEMPO_R = {
    (110.0, 500): (0.9835, 1.0151, 0.187), (110.0, 800): (0.9838, 1.0152, 0.280), (110.0, 1250): (0.9839, 1.0150, 0.213), (110.0, 2000): (0.9841, 1.0139, 0.373),
    (220.0, 500): (0.9941, 1.0057, 0.627), (220.0, 800): (0.9944, 1.0057, 0.440), (220.0, 1250): (0.9947, 1.0055, 0.427), (220.0, 2000): (0.9946, 1.0053, 0.253),
    (997.0, 500): (0.9994, 1.0006, 0.163), (997.0, 800): (0.9995, 1.0006, 0.456), (997.0, 1250): (0.9995, 1.0005, 0.157), (997.0, 2000): (0.9997, 1.0004, 0.075),
    (3000.0, 500): (1.0000, 1.0000, 0.000), (3000.0, 800): (1.0000, 1.0000, 0.000), (3000.0, 1250): (1.0000, 1.0000, 0.000), (3000.0, 2000): (1.0000, 1.0000, 0.000),
}


def ola_exact(f, s):
    """Plain overlap-add is exact on a tone whose every analysis position is a whole number of periods: a_k = k Hs s / 1000 without a
    remainder, and Hs s / 1000 samples a whole number of periods of f."""
    return (HS * s) % 1000 == 0 and (f * (HS * s // 1000)) % RATE == 0


if __name__ == "__main__":
    for name, search in (("TEMPO_R", True), ("plain overlap-add", False)):
        print(f"{name} = {{")
        for f in TONES:
            x = tone(f)
            cells = []
            for s in TONE_SPEEDS:
                y, _ = stretch(x, s, dtype=np.float64, search=search)
                lo, hi, pk = tone_measures(y, x.size, s, f)
                cells.append(f"({f}, {s}): ({lo:.4f}, {hi:.4f}, {pk:.3f})")
            print("    " + ", ".join(cells) + ",")
        print("}")

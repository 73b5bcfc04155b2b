"""The device resampler's filter restated in numpy: the float64 table formula, the f32 restatement the kernel must equal bit
for bit (one f32 multiply and one f32 add per tap, taps in ascending order), the same sum in float64, and the counts N and D.

    g = gcd(rate_in, rate_out), L = rate_out / g, M = rate_in / g, c = 0.93 min(1, L / M), W = 32 / c, H = ceil(W), T = 2 H + 1
    tab[p][k] = f32(h(H - k + p / L)),  h(d) = c sinc(c d) I0(9 sqrt(1 - (d / W)^2)) / I0(9) for |d| <= W, else 0
    y[m] = sum_k x[i - H + k] tab[p][k],  i = (m M) div L, p = (m M) mod L,  x = 0 outside [0, n)

Run as a script (`python tests/_resample_ref.py`) it measures the tone errors of the float64 version and prints the TONE_R table below."""
import math

import numpy as np

RHO, ZEROS, BETA = 0.93, 32.0, 9.0
MAX_COEF = 32768

# the pairs the tests cover: the vocoder's rate to the usual output rates, and the usual recording rates to the encoders' rate
PAIRS = [(24000, r) for r in (8000, 16000, 22050, 32000, 44100, 48000, 11025)] + [(r, 24000) for r in (8000, 16000, 44100, 48000)]
# tones, as a fraction of the lower of the two Nyquist frequencies (pass band) and of the output Nyquist frequency (stop band, down-sampling)
PASS_TONES, STOP_TONE = (0.0, 0.5, 0.8), 1.05
TONE_N = 4096  # input samples of a tone


def plan(rate_in, rate_out):
    g = math.gcd(rate_in, rate_out)
    L, M = rate_out // g, rate_in // g
    c = RHO * min(1.0, L / M)
    W = ZEROS / c
    H = int(math.ceil(W))
    return L, M, H, 2 * H + 1, c, W


def _i0(x):
    """sum_j ((x / 2)^j / j!)^2 in float64: every term is positive, so nothing cancels."""
    x = np.asarray(x, dtype=np.float64)
    q = 0.25 * x * x
    term, total = np.ones_like(x), np.ones_like(x)
    for j in range(1, 64):
        term = term * (q / (j * j))
        total = total + term
    return total


def table64(rate_in, rate_out):
    """(L, M, H, tab [L][T] float64) by the formula above."""
    L, M, H, T, c, W = plan(rate_in, rate_out)
    d = (H - np.arange(T, dtype=np.float64))[None, :] + (np.arange(L, dtype=np.float64) / L)[:, None]
    inside = np.abs(d) <= W
    r = np.where(inside, d / W, 0.0)
    h = c * np.sinc(c * d) * _i0(BETA * np.sqrt(np.maximum(0.0, 1.0 - r * r))) / _i0(BETA)
    return L, M, H, np.where(inside, h, 0.0)


def N(n, L, M):
    return -(-n * L // M) if n > 0 else 0


def D(n, L, M, H):
    return -(-(n - H) * L // M) if n > H else 0


def _windows(x, n, L, M, H, first, count):
    """x[:n] zero-padded so that every window of outputs [first, first + count) can be sliced; (xp, start index of each window in xp, phase)."""
    m = np.arange(first, first + count, dtype=np.int64)
    i, p = (m * M) // L, (m * M) % L
    lo = int(i[0]) - H if count else 0
    hi = int(i[-1]) + H + 1 if count else 0
    xp = np.zeros(max(hi - lo, 0), dtype=x.dtype)
    a, b = max(lo, 0), min(hi, n)
    if b > a:
        xp[a - lo:b - lo] = x[a:b]
    return xp, i - H - lo, p


def resample32(x, n, tab, L, M, H, first, count):
    """The f32 restatement: outputs [first, first + count) of the row x with n valid samples (what lies beyond is not read). tab: [L][T] f32."""
    x = np.asarray(x, dtype=np.float32)
    tab = np.asarray(tab, dtype=np.float32)
    xp, s, p = _windows(x, n, L, M, H, first, count)
    acc = np.zeros(count, dtype=np.float32)
    for k in range(2 * H + 1):
        acc = acc + (xp[s + k] * tab[p, k])  # one f32 multiply, one f32 add
    assert acc.dtype == np.float32
    return acc


def resample64(x, n, tab, L, M, H, first, count, with_abs=False):
    """The same sum in float64 (the table's values as given); with_abs: also sum_k |x_k tab_k|, the scale of the sequential-sum bound."""
    x = np.asarray(x, dtype=np.float64)
    tab = np.asarray(tab, dtype=np.float64)
    xp, s, p = _windows(x, n, L, M, H, first, count)
    acc, mag = np.zeros(count), np.zeros(count)
    for k in range(2 * H + 1):
        t = xp[s + k] * tab[p, k]
        acc += t
        mag += np.abs(t)
    return (acc, mag) if with_abs else acc


def to_i16(y):
    """The Q3TTS_PCM_I16 rule on f32 values: (x * 32767).clamp(-32768, 32767) as i16, truncation toward zero."""
    return np.trunc(np.clip(np.asarray(y, dtype=np.float32) * np.float32(32767), -32768, 32767)).astype(np.int16)


def tone_error(rate_in, rate_out, frac, stop=False):
    """A unit tone through the float64 version with the f32-rounded table: max |y - ideal tone| (pass) or max |y| (stop) over the outputs
    whose windows lie inside the data. frac: of min(rate_in, rate_out) / 2 (pass), of rate_out / 2 (stop)."""
    L, M, H, tab = table64(rate_in, rate_out)
    tab = tab.astype(np.float32)
    f = frac * (rate_out if stop else min(rate_in, rate_out)) / 2.0
    n = TONE_N
    x = np.cos(2 * np.pi * f * np.arange(n) / rate_in + 0.3)
    y = resample64(x, n, tab, L, M, H, 0, N(n, L, M))
    m = np.arange(y.size)
    inside = ((m * M) // L >= H) & (m < D(n, L, M, H))
    ideal = 0.0 if stop else np.cos(2 * np.pi * f * m / rate_out + 0.3)
    return float(np.max(np.abs(y - ideal)[inside]))


# max error of tone_error(), measured by this file's script path on this restatement (never on the device); the tests bound each at twice it.
# {(rate_in, rate_out): {fraction: error}}; the 1.05 entry is the stop-band tone and exists for down-sampling pairs only
TONE_R = {
    (24000, 8000): {0.0: 5.06e-06, 0.5: 1.79e-06, 0.8: 5.15e-06, 1.05: 2.35e-05},
    (24000, 16000): {0.0: 6.03e-06, 0.5: 2.80e-06, 0.8: 5.23e-06, 1.05: 2.53e-05},
    (24000, 22050): {0.0: 6.68e-06, 0.5: 2.46e-06, 0.8: 1.06e-05, 1.05: 3.61e-05},
    (24000, 32000): {0.0: 6.42e-06, 0.5: 3.19e-06, 0.8: 1.23e-05},
    (24000, 44100): {0.0: 6.44e-06, 0.5: 3.39e-06, 0.8: 1.28e-05},
    (24000, 48000): {0.0: 6.42e-06, 0.5: 2.65e-06, 0.8: 1.23e-05},
    (24000, 11025): {0.0: 5.42e-06, 0.5: 2.10e-06, 0.8: 5.59e-06, 1.05: 2.38e-05},
    (8000, 24000): {0.0: 6.42e-06, 0.5: 3.39e-06, 0.8: 1.16e-05},
    (16000, 24000): {0.0: 6.42e-06, 0.5: 3.39e-06, 0.8: 1.16e-05},
    (44100, 24000): {0.0: 5.47e-06, 0.5: 2.31e-06, 0.8: 5.61e-06, 1.05: 2.41e-05},
    (48000, 24000): {0.0: 5.10e-06, 0.5: 1.95e-06, 0.8: 5.54e-06, 1.05: 2.37e-05},
}


if __name__ == "__main__":
    print("TONE_R = {")
    for ri, ro in PAIRS:
        row = {fr: tone_error(ri, ro, fr) for fr in PASS_TONES}
        if ro < ri:
            row[STOP_TONE] = tone_error(ri, ro, STOP_TONE, stop=True)
        print(f"    ({ri}, {ro}): {{" + ", ".join(f"{k}: {v:.2e}" for k, v in row.items()) + "},")
    print("}")

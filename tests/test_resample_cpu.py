"""The resampler's filter without a GPU: the library's host table against the float64 formula, the refusals, the f32
restatement against float64 within the sequential-sum bound, tones through the float64 version, and the counts N and D."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _resample_ref as RR  # noqa: E402


@pytest.mark.parametrize("rate_in,rate_out", RR.PAIRS)
def test_table_hook_equals_float64_formula(rate_in, rate_out):
    """q3tts_k_resample_table == the float64 formula rounded to f32, within 6e-8 absolute: one ulp at the table's peak (c <= 0.93 < 1, ulp =
    2^-24 = 5.96e-8), since libm and numpy may differ in the last bit of the double that is rounded. L, M, H and the length are exact."""
    from q3tts import native
    L, M, H, tab = native.k_resample_table(rate_in, rate_out)
    rl, rm, rh, ref = RR.table64(rate_in, rate_out)
    assert (L, M, H) == (rl, rm, rh) and tab.shape == (L, 2 * H + 1) and tab.dtype == np.float32
    assert L * rate_in == M * rate_out and np.gcd(L, M) == 1
    err = np.abs(tab.astype(np.float64) - ref.astype(np.float32).astype(np.float64)).max()
    print(f"{rate_in}->{rate_out}: L {L} M {M} H {H} T {2 * H + 1}, max |table - formula| {err:.3g}")
    assert err <= 6e-8


def test_table_hook_refusals():
    from q3tts import _abi, native
    L, M, H, T, _, _ = RR.plan(24000, 44101)
    assert L * T > RR.MAX_COEF
    for ri, ro, status in ((24000, 44101, -6), (24000, 3999, -1), (3999, 24000, -1), (24000, 96001, -1), (96001, 24000, -1)):
        with pytest.raises(_abi.Q3Error) as ei:
            native.k_resample_table(ri, ro)
        assert ei.value.status == status, (ri, ro)
    # the limits themselves are inside
    assert native.k_resample_table(24000, 4000)[0] == 1 and native.k_resample_table(24000, 96000)[:2] == (4, 1)


@pytest.mark.parametrize("rate_in,rate_out", RR.PAIRS)
def test_restatement_within_sequential_sum_bound_of_float64(rate_in, rate_out):
    """Uniform +-1 noise, 2 x 7680 samples: every f32 output is within (T + 1) 2^-24 sum_k |x_k tab_k| of the float64 sum over the same f32
    operands. That is the bound of a sequential sum of T products (each product and each partial sum rounds once, half an ulp of a value no
    larger than the sum of magnitudes); nothing is measured for it."""
    L, M, H, tab = RR.table64(rate_in, rate_out)
    tab = tab.astype(np.float32)
    T = 2 * H + 1
    n = 2 * 7680
    x = np.random.default_rng(rate_in + rate_out).uniform(-1.0, 1.0, n).astype(np.float32)
    cnt = RR.N(n, L, M)
    y32 = RR.resample32(x, n, tab, L, M, H, 0, cnt)
    y64, mag = RR.resample64(x, n, tab, L, M, H, 0, cnt, with_abs=True)
    ratio = np.abs(y32.astype(np.float64) - y64) / np.maximum((T + 1) * 2.0 ** -24 * mag, 1e-300)
    print(f"{rate_in}->{rate_out}: worst error / bound {ratio.max():.3g}")
    assert np.isfinite(y32).all() and ratio.max() <= 1.0


@pytest.mark.parametrize("rate_in,rate_out", RR.PAIRS)
def test_tones_through_float64_version(rate_in, rate_out):
    """Pass band: a unit tone at 0, 0.5 and 0.8 of the lower Nyquist frequency comes back as the ideal tone; stop band (down-sampling): a
    tone at 1.05 of the output Nyquist frequency is removed. Each within twice the error _resample_ref's script path measured (TONE_R)."""
    rec = RR.TONE_R[(rate_in, rate_out)]
    for frac in RR.PASS_TONES:
        err = RR.tone_error(rate_in, rate_out, frac)
        print(f"{rate_in}->{rate_out}: pass {frac}: {err:.3g} (recorded {rec[frac]:.3g})")
        assert err <= 2 * rec[frac]
    assert (RR.STOP_TONE in rec) == (rate_out < rate_in)
    if rate_out < rate_in:
        err = RR.tone_error(rate_in, rate_out, RR.STOP_TONE, stop=True)
        print(f"{rate_in}->{rate_out}: stop {RR.STOP_TONE}: {err:.3g} (recorded {rec[RR.STOP_TONE]:.3g})")
        assert err <= 2 * rec[RR.STOP_TONE]
    assert max(rec.values()) < 1e-4  # the filter's design: 80 dB


def _brute(n, L, M, H, final):
    """Outputs m = 0, 1, ... at time m M / L: the finished row has those with time < n; the unfinished one those whose window's last tap,
    i + H, is a sample it holds."""
    m = 0
    while (m * M < n * L) if final else ((m * M) // L + H <= n - 1):
        m += 1
    return m


@pytest.mark.parametrize("rate_in,rate_out", RR.PAIRS)
def test_counts_against_brute_force(rate_in, rate_out):
    L, M, H, _, _, _ = RR.plan(rate_in, rate_out)
    for n in (0, 1, H, H + 1, H + 2, 1920, 7680, 7681):
        assert RR.N(n, L, M) == _brute(n, L, M, H, True), n
        assert RR.D(n, L, M, H) == _brute(n, L, M, H, False), n


@pytest.mark.parametrize("rate_in,rate_out", RR.PAIRS)
def test_delivery_windows_tile_the_output(rate_in, rate_out):
    """D is monotone, D(n) <= N(n), and the chunks [D(n_j), D(n_j+1)) of a growing row, closed by [D(n_last), N(n_last)), tile [0, N)."""
    L, M, H, _, _, _ = RR.plan(rate_in, rate_out)
    ns = np.arange(0, 3 * 1920 + 50)
    d = np.array([RR.D(int(n), L, M, H) for n in ns])
    nn = np.array([RR.N(int(n), L, M) for n in ns])
    assert (np.diff(d) >= 0).all() and (d <= nn).all() and (np.diff(nn) >= 0).all()
    for steps in ([1920, 3840, 5760], [1, H, H + 1, H + 2, 1920, 1921, 5000], [7680, 7681]):
        edges = [0] + [RR.D(n, L, M, H) for n in steps] + [RR.N(steps[-1], L, M)]
        assert all(b >= a for a, b in zip(edges, edges[1:]))
        covered = np.concatenate([np.arange(a, b) for a, b in zip(edges, edges[1:])])
        assert np.array_equal(covered, np.arange(RR.N(steps[-1], L, M)))

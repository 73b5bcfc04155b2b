"""The sampler (sample_row in csrc/q3_kernels.hip, q3o_sample in oracle/q3_oracle.c) against its definition — test infrastructure.

`admissible` states the sampler from the definition in numpy float64 and shares no code with the oracle; `cases` generates the hook calls
that tests/test_sampler_cpu.py (the oracle, no GPU) and tests/test_sampler_gpu.py (the kernel) walk.

The definition (src/models/llama/mod.rs:666-772 of the program this project follows): stable descending order of the first `limit`
logits; the first top_k of them when 0 < top_k < limit (a negative top_k is "all", as `top_k as usize`); softmax of
(x - max) / float32(T); cut at the first cumulative sum >= top_p (only when top_p < 1) and renormalise; the first index with r < cum, and
the first candidate when there is none. T <= 0: the first maximum (NaN entries are skipped; a row of NaNs gives 0).

The admissible set. An f32 sequential sum of n non-negative terms differs from the exact sum by at most n * 2^-24 relative, so every
cumulative sum c_i the f32 programs compare stands for some value in c_i * (1 -+ delta), delta = C * (n + 8) * 2^-23, n = the candidate
count after top-k (the 8 is room for the exp's own error, measured below). `admissible` returns every id that some such perturbation
selects:
  - the cut ranges over every position between the first c_i (1 + delta) >= top_p and the first c_i (1 - delta) >= top_p;
  - for a cut after m candidates the renormalised sums are c_i / c_(m-1); id i is selected by some perturbation iff p_i > 0 and
    c_(i-1) (1 - delta) <= r c_(m-1) < c_i (1 + delta) for an m > i in that range (a term of probability 0 cannot move the sum past r,
    whatever the rounding: that is what keeps the set small when every exp but the first is 0);
  - the fallback (first candidate) is in the set when r >= 1 - delta.
Two sharpenings, both from the arithmetic and not from any output:
  - exp(x) is taken as 0 below x = -104: e^-104 < 2^-150, so no f32 exp, flushed (q3_expf returns 0 below -87) or not, is positive there;
  - when every exp is exactly 0 or 1 and the number of ones is a power of two, every f32 operation of the chain is exact (1 / 2^k, its
    partial sums and the renormalisation by a dyadic sum round nothing), no perturbation exists, and delta = 0. These are the only rows
    on which `>=` against `>` at the cut and `r <` against `r <=` at the pick are decidable at all; the `flat` family supplies them.

C, measured against q3o_sample on the CPU and never against the device (tests/test_sampler_cpu.py asserts all three lines):
  C = 1: q3o_sample lies in the admissible set on every row of cases(0); nothing forced a raise.
  q3o_expf against np.exp over [-87, 0]: worst relative error 2.2e-7 (bound asserted: EXPF_REL_BOUND = 2^-22), inside the 8 * 2^-23 room.
  Rows of cases(0) with a single admissible id, over SINGLETON_FAMILIES and every T: 96.2 % of 17 248 (asserted: >= 90 %). Widest set
  among the rows with T <= 1 and at most 257 candidates after top-k: 3 ids (asserted: <= 3); see _draws for the 29 draws this moved.

Out of scope for T > 0: NaN logits (the kernel orders NaN last, the oracle's merge keeps it in place, q3_expf of NaN is undefined) and
rows whose first `limit` entries are all -inf. Greedy with NaN entries is in scope (both skip NaN): the `nan` case. (A greedy row that
holds nothing but NaN and -inf is out of scope as well: the oracle's strict `>` never leaves index 0 there, the kernel's key order takes
the first -inf.)
"""
import numpy as np

C_WIDEN = 1.0
EXPF_REL_BOUND = 2.0 ** -22
SINGLETON_FAMILIES = ("gauss2", "peaked", "masked", "huge", "asc", "desc", "zeros")

LD = 4096
ROWS = 16
PER_PAIR = 10
LIMITS = (1, 2, 63, 64, 65, 255, 256, 257, 1000, 2048, 2049, 2160, 4095, 4096)
TOP_PS = (0.0, 1e-6, 0.5, 0.9, 0.999999, 1.0, 1.5)
TEMPS = (0.0, 1e-3, 0.7, 1.0, 5.0, 100.0)
FAMILIES = ("gauss2", "peaked", "flat", "levels", "overflow", "masked", "huge", "asc", "desc", "zeros")
OVERFLOW_LOW, OVERFLOW_FLOOR = 77, 200   # residue classes mod 256 of the `overflow` family
BEYOND = np.float32(3e38)                # what every column >= limit holds: a kernel that reads past `limit` picks it
ONE_BELOW = np.nextafter(np.float32(1.0), np.float32(0.0))


def top_ks(limit):
    return tuple(sorted({-1, 0, 1, 2, 40, 255, 256, 257, limit - 1, limit, limit + 1}))


def kept(limit, top_k):
    """The candidate count after top-k."""
    return top_k if 0 < top_k < limit else limit


# ---- the float64 statement ---------------------------------------------------------------------------------------------------------------
def greedy(logits, limit):
    x = np.asarray(logits[:limit], dtype=np.float64)
    x = np.where(np.isnan(x), -np.inf, x)
    return int(np.argmax(x))


def distribution(logits, limit, T, top_k):
    """(candidate ids in order, their probabilities, exact): the definition up to the first normalisation, in float64."""
    x = np.asarray(logits[:limit], dtype=np.float64)
    order = np.argsort(-x, kind="stable")
    cand = order[:kept(limit, top_k)]
    v = x[cand]
    with np.errstate(invalid="ignore", over="ignore"):
        z = (v - v[0]) / float(np.float32(T))
    e = np.where(z < -104.0, 0.0, np.exp(np.maximum(z, -104.0)))
    ones = int(np.count_nonzero(e == 1.0))
    exact = bool(np.all((e == 0.0) | (e == 1.0))) and (ones & (ones - 1)) == 0
    return cand, e / e.sum(), exact


def _cut_range(cum, top_p, delta):
    """(lo, hi): the cut keeps m candidates for some lo <= m <= hi."""
    n = cum.size
    tp = float(np.float32(top_p))
    if not tp < 1.0:
        return n, n
    a = np.nonzero(cum * (1.0 + delta) >= tp)[0]
    b = np.nonzero(cum * (1.0 - delta) >= tp)[0]
    return (int(a[0]) + 1 if a.size else n), (int(b[0]) + 1 if b.size else n)


def admissible(logits, limit, T, top_k, top_p, r, c=C_WIDEN):
    if float(np.float32(T)) <= 0.0:
        return {greedy(logits, limit)}
    cand, p, exact = distribution(logits, limit, T, top_k)
    n = cand.size
    delta = 0.0 if exact else c * (n + 8) * 2.0 ** -23
    cum = np.cumsum(p)
    lo, hi = _cut_range(cum, top_p, delta)
    if exact and np.frexp(cum[lo - 1])[0] != 0.5:            # the cut's renormalising sum is no power of two: p / sum rounds
        delta = c * (n + 8) * 2.0 ** -23
        lo, hi = _cut_range(cum, top_p, delta)
    r = float(np.float32(r))
    out = set()
    if r >= 1.0 - delta:
        out.add(int(cand[0]))
    prev = np.concatenate(([0.0], cum[:-1]))
    if r == 0.0:
        ok = (prev == 0.0) & (p > 0.0)                       # 0 < c_i (1 + delta) needs nothing more; i < hi holds for i = 0
    else:
        cs = cum[lo - 1:hi]                                  # the renormalising sum of every admissible cut, ascending
        j = np.searchsorted(cs, prev * (1.0 - delta) / r, side="left")
        j = np.maximum(j, np.arange(n) - (lo - 1))           # the cut lies behind candidate i
        inside = j < cs.size
        ok = inside & (cs[np.minimum(j, cs.size - 1)] * r < cum * (1.0 + delta)) & (p > 0.0)
    out.update(int(i) for i in cand[ok])
    return out


def expf_rel_error(n=20001):
    """Worst relative error of q3o_expf against np.exp on [-87, 0] (f32 arguments)."""
    import _oracle as O
    L = O.lib()
    xs = np.linspace(-87.0, 0.0, n).astype(np.float32)
    ys = np.array([L.q3o_expf(float(x)) for x in xs], dtype=np.float64)
    ref = np.exp(xs.astype(np.float64))
    return float(np.max(np.abs(ys - ref) / ref))


# ---- the select path's list length, from the comment in sample_row ----------------------------------------------------------------------
def select_list_length(row, limit, top_k):
    """Thread t of 256 owns the candidates t, t + 256, ...; the threshold is the top_k-th largest of the thread maxima in the order
    (value descending, index ascending); every candidate at or above it is listed, every candidate when fewer than top_k threads hold one."""
    x = np.asarray(row[:limit], dtype=np.float64)
    x = np.where(x == 0.0, 0.0, x)
    rank = np.empty(limit, dtype=np.int64)
    rank[np.argsort(-x, kind="stable")] = np.arange(limit)   # 0 = the largest key
    best = np.full(256, limit, dtype=np.int64)
    np.minimum.at(best, np.arange(limit) % 256, rank)
    best = np.sort(best[best < limit])
    if best.size < top_k:
        return limit
    return int(np.count_nonzero(rank <= best[top_k - 1]))


# ---- the case generator ------------------------------------------------------------------------------------------------------------------
def family_rows(name, rng, limit, rows):
    g = lambda s: (rng.standard_normal((rows, LD)) * s).astype(np.float32)
    if name == "gauss2":
        x = g(2.0)
    elif name == "peaked":
        x = g(0.5)
        for row in x:
            at = rng.choice(limit, size=min(6, limit), replace=False)
            row[at] += np.linspace(4.0, 9.0, 6, dtype=np.float32)[:at.size]
    elif name == "flat":
        x = np.full((rows, LD), 1.25, dtype=np.float32)
    elif name == "levels":
        x = (rng.integers(-3, 4, size=(rows, LD)) * 0.5).astype(np.float32)
    elif name == "overflow":
        # 3.0 + jitter in (0, 1e-2]; class OVERFLOW_FLOOR sits on the jitter band's floor and class OVERFLOW_LOW near -5.0, so that the
        # 255th and the 256th largest thread maxima both lie below (nearly) every other candidate
        x = (3.0 + 1e-2 * (1.0 - rng.random((rows, LD)))).astype(np.float32)
        x[:, OVERFLOW_FLOOR::256] = np.float32(3.0) - (1e-4 * rng.random((rows, LD // 256))).astype(np.float32)
        x[:, OVERFLOW_LOW::256] = np.float32(-5.0) + (1e-2 * rng.random((rows, LD // 256))).astype(np.float32)
    elif name == "masked":
        x = g(1.0)
        x[rng.random((rows, LD)) < 0.98] = -np.inf
        x[:, min(3, limit - 1)] = g(1.0)[:, 0]               # index 3 (the last index of a narrower row) is finite
    elif name == "huge":
        x = g(1.0) * np.float32(1e30)
    elif name == "asc":
        x = np.tile((np.arange(LD) * 0.01).astype(np.float32), (rows, 1))
    elif name == "desc":
        x = np.tile((np.arange(LD) * -0.01).astype(np.float32), (rows, 1))
    elif name == "zeros":
        x = g(1.0)
        x[:, 0::7] = np.float32(0.0)
        x[:, 3::7] = np.float32(-0.0)
    else:
        raise KeyError(name)
    x[:, limit:] = BEYOND
    return x


def _draws(rng, family, logits, limit, T, top_k, top_p):
    """Row 0: r = 0; row 1: the largest f32 below 1 (*); rows 2, 3: uniform draws (`flat`: rounded down to a multiple of 1/64, which is a
    boundary of the cumulative sum when the candidate count is a multiple of 64); the other rows: a uniform draw moved to the middle of the
    interval of the cumulative sum it falls in (float64, nominal cut), away from the boundaries.
    (*) With T <= 1 and at most 257 candidates, a row whose tail probabilities lie below delta leaves that draw more than three admissible ids
    (29 rows of cases(0)): nothing in float64 can narrow it, so such a row takes a draw of the last kind instead. The draw stays on every
    other row, and the fallback it aims at is reached there whenever the f32 sum ends below 1."""
    rows = logits.shape[0]
    r = np.zeros(rows, dtype=np.float32)
    if T <= 0.0:
        return r
    u = rng.random(rows)
    r[1] = ONE_BELOW
    r[2:4] = np.floor(u[2:4] * 64.0) / 64.0 if family == "flat" else u[2:4]
    small = T <= 1.0 and kept(limit, top_k) <= 257
    for i in range(1, rows):
        if i < 4 and not (i == 1 and small and len(admissible(logits[1], limit, T, top_k, top_p, ONE_BELOW)) > 3):
            continue
        cand, p, _ = distribution(logits[i], limit, T, top_k)
        cum = np.cumsum(p)
        m, _ = _cut_range(cum, top_p, 0.0)
        cq = cum[:m] / cum[m - 1]
        k = min(int(np.searchsorted(cq, u[i], side="right")), m - 1)
        r[i] = min(np.float32(0.5 * ((cq[k - 1] if k else 0.0) + cq[k])), ONE_BELOW)
    return r


# (family, limit, T, top_k, top_p) that every run carries whatever the rotation below picks
def _pinned():
    for limit in (2049, 2160, 4096):
        for top_k in (255, 256, 257):
            for top_p in (1.0, 0.9):
                yield "overflow", limit, 1.0, top_k, top_p
    for limit, top_k in ((64, 0), (256, 0), (256, 64), (2048, -1), (4096, 256), (4096, 0)):   # `flat` with a power-of-two candidate count
        for top_p in (0.5, 1.0):
            yield "flat", limit, 1.0, top_k, top_p


def nan_case(seed=0):
    """One greedy call with NaN entries: row 0 all NaN (id 0), row 1 NaN over the largest values, row 2 NaN first, the rest sprinkled."""
    rng = np.random.default_rng([seed, 999])
    limit = 2160
    x = (rng.standard_normal((ROWS, LD)) * 2.0).astype(np.float32)
    x[0, :] = np.nan
    x[1, np.argsort(-x[1, :limit])[:40]] = np.nan
    x[2, 0] = np.nan
    x[3:][rng.random((ROWS - 3, LD)) < 0.3] = np.nan
    x[:, limit:] = BEYOND
    return "nan", limit, 0.0, 40, 0.9, x, np.zeros(ROWS, dtype=np.float32)


def cases(seed=0):
    """Yields (family, limit, T, top_k, top_p, logits[ROWS][LD] f32, r[ROWS] f32), one call of the q3tts_k_sample hook each.

    The product limit x top_k x top_p x T x family is 64 680 calls. Kept: per (family, limit) one greedy call and PER_PAIR sampled ones,
    taken from the (T > 0, top_k, top_p) product of that limit at a stride coprime to its length, the starting point advancing from pair
    to pair, so that the pairs together walk the product several times over; plus the pinned calls of _pinned() and nan_case().
    The logits of a (family, limit) are drawn once and shared by its calls; the draws differ per call."""
    temps = [t for t in TEMPS if t > 0.0]
    pinned = list(_pinned())
    for fi, family in enumerate(FAMILIES):
        for li, limit in enumerate(LIMITS):
            logits = family_rows(family, np.random.default_rng([seed, fi, li]), limit, ROWS)
            logits.setflags(write=False)
            tks = top_ks(limit)
            total = len(temps) * len(tks) * len(TOP_PS)
            combos = [(0.0, 40, 0.9)]
            for j in range(PER_PAIR):
                idx = (((fi * len(LIMITS) + li) * PER_PAIR + j) * 37) % total
                combos.append((temps[idx // (len(TOP_PS) * len(tks))], tks[(idx // len(TOP_PS)) % len(tks)], TOP_PS[idx % len(TOP_PS)]))
            combos += [(T, k, p) for (f, l, T, k, p) in pinned if f == family and l == limit and (T, k, p) not in combos]
            for ci, (T, top_k, top_p) in enumerate(combos):
                r = _draws(np.random.default_rng([seed, fi, li, ci]), family, logits, limit, T, top_k, top_p)
                yield family, limit, T, top_k, top_p, logits, r
    yield nan_case(seed)

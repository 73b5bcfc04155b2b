"""Operands and float64 judgement for the split residual VQ of the clone audio encoder (tests/test_clone_rvq_{cpu,gpu}.py).

k_rvq (q3_clone.hip) and q3o_rvq (oracle/q3_oracle_clone.c) take ps / pa [T][D], books [ncb][CS][D] and return codes [T][ncb]: codebook 0 on
ps[t], codebooks 1.. on pa[t] and then on its running residual; nearest codeword in squared Euclidean distance, ties to the smaller index.

Two kinds of operands:
  random      judged in float64 along the picks of the implementation under test (judge): the residual is one IEEE f32 subtraction per element,
              which numpy reproduces exactly, so the float64 distances are those of the very vectors the implementation compared.
  constructed every value is a multiple of 1/8 of magnitude <= 16.25, D = 16: a squared distance is a multiple of 1/64 below 2^13, exact in f32
              under any summation order, so ties are ties on every implementation and the expected ids are known by construction.
"""
import numpy as np

U = 2.0 ** -24
RVQ_T, RVQ_CW = 1024, 2   # k_rvq: lanes per workgroup, codewords per lane and trip

# (codebook_size, vq_dim, n_codebooks): the vq shapes of _clone_shapes.py and the full config's
RANDOM_SIZES = ((1, 16, 1), (63, 16, 2), (1000, 48, 3), (1025, 16, 64), (2049, 32, 3), (3000, 48, 3), (5000, 272, 2), (2048, 256, 16))
RANDOM_T = (1, 5)


def random_case(CS, D, ncb, T):
    rng = np.random.default_rng([CS, D, ncb, T])
    books = (rng.standard_normal((ncb, CS, D)) / np.sqrt(D)).astype(np.float32)
    ps = (rng.standard_normal((T, D)) / np.sqrt(D)).astype(np.float32)
    pa = (rng.standard_normal((T, D)) / np.sqrt(D)).astype(np.float32)
    return ps, (pa if ncb > 1 else None), books


def bound(D):
    """picked float64 distance <= bound * float64 minimum. A computed distance is a D-term chain of positive fmaf terms e*e on once-rounded
    differences e: each term carries (1 + d)^2 from e's rounding and every partial sum one rounding more, so computed = exact * (1 + h) with
    |h| <= g = (D + 2) u / (1 - (D + 2) u). The picked codeword's computed distance is <= the computed distance of the float64-nearest one."""
    g = (D + 2) * U / (1.0 - (D + 2) * U)
    return (1.0 + g) / (1.0 - g)


def judge(ps, pa, books, codes):
    """Every (t, q) of `codes` against float64, following those picks. Returns the worst picked / minimum ratio found (1.0 when all picks
    are the float64 argmin); raises AssertionError at the first entry outside the bound or the codebook. No entry is exempt."""
    ncb, CS, D = books.shape
    b64 = books.astype(np.float64)
    lim, worst = bound(D), 1.0
    for t in range(ps.shape[0]):
        r = None
        for q in range(ncb):
            if q < 2:
                r = np.array((ps if q == 0 else pa)[t], dtype=np.float32)
            d = ((r.astype(np.float64)[None, :] - b64[q]) ** 2).sum(axis=1)
            k = int(codes[t, q])
            assert 0 <= k < CS, (t, q, k)
            assert d[k] <= lim * d.min(), "t %d q %d: picked %d at %.17g, float64 nearest %d at %.17g" % (t, q, k, d[k], int(d.argmin()), d.min())
            if d.min() > 0.0:
                worst = max(worst, d[k] / d.min())
            if q > 0:
                r = (r - books[q, k]).astype(np.float32)   # one f32 subtraction per element, as both implementations do
    return worst


# ---- constructed operands ---------------------------------------------------------------------------------------------------------------
TIE_D, TIE_CS, TIE_NCB = 16, 2100, 4
# the nearest codeword twice; the answer is the smaller index. What of k_rvq decides each: one lane's two codewords of a trip (5, 1029); one
# lane, two trips (5, 2053); two lanes of one wave (64, 70); the last lane of wave 0 and the first of wave 1 (63, 64); the last lane's first
# codeword and lane 0's second (1023, 1024); a lane's first trip and the codebook's last codeword, second trip, second codeword (3, 2099)
TIE_PAIRS = ((5, 1029), (5, 2053), (64, 70), (63, 64), (1023, 1024), (3, 2099))
# the nearest codeword once: the answer is that index, although a runner-up sits in the same lane one codeword earlier (index - 1024)
TIE_ALONE = (1024, 2048, 2099)
SIZES_CS = (1, 1023, 1024, 1025, 2047, 2048, 2049)


def _far(rng, CS, D):
    """codewords nowhere near a residual of magnitude <= 1.25: coordinate 0 is +-16, the rest multiples of 1/8 in [-1, 1]"""
    b = rng.integers(-8, 9, size=(CS, D)).astype(np.float32) / 8.0
    b[:, 0] = np.where(rng.integers(0, 2, size=CS) == 0, -16.0, 16.0)
    return b


def _small(rng, D):
    """a vector of multiples of 1/8 in [-1, 1]"""
    return rng.integers(-8, 9, size=D).astype(np.float32) / 8.0


def _place(rng, r, CS, at, runner_up=()):
    """a codebook whose nearest codeword to r (distance 1/64) sits at every index of `at`, a second-nearest (4/64) at `runner_up`, the rest far"""
    D = r.size
    b = _far(rng, CS, D)
    e = np.zeros(D, dtype=np.float32); e[int(rng.integers(1, D))] = 0.125
    for i in runner_up:
        b[i] = r + 2 * e
    for i in at:
        b[i] = r + e
    return b, (r - (r + e)).astype(np.float32)   # the book, and the residual it leaves: -e


def tie_case(at, seed=0, CS=TIE_CS, ncb=TIE_NCB):
    """One frame. The nearest codeword of every codebook sits at the indices `at` (a pair: the smaller one is the answer). Codebook 0 sees
    ps as loaded; codebook 1 sees pa as loaded; codebooks 2.. see the residual k_rvq carries in LDS. Returns ps, pa, books, expected [1][ncb]."""
    rng = np.random.default_rng([seed, CS] + list(at))
    D = TIE_D
    at = [i for i in at if i < CS]
    ru = sorted({7 % CS} | {i - RVQ_T for i in at if i - RVQ_T >= 0})
    ru = [i for i in ru if i not in at]
    ps, pa = _small(rng, D), _small(rng, D)
    books = np.zeros((ncb, CS, D), dtype=np.float32)
    books[0], _ = _place(rng, ps, CS, at, ru)
    r = pa
    for q in range(1, ncb):
        books[q], r = _place(rng, r, CS, at, ru)
    assert np.abs(books * 8 - np.round(books * 8)).max() == 0 and np.abs(books).max() <= 16.25
    return ps[None], pa[None], books, np.full((1, ncb), min(at), dtype=np.int64)


def identical_case(seed=0, CS=TIE_CS, ncb=TIE_NCB):
    """every codeword of a codebook is the same vector: every distance ties, the answer is 0 in every codebook"""
    rng = np.random.default_rng([seed, 1])
    D = TIE_D
    books = np.stack([np.repeat(_small(rng, D)[None], CS, axis=0) for _ in range(ncb)])
    ps, pa = np.stack([_small(rng, D) for _ in range(3)]), np.stack([_small(rng, D) for _ in range(3)])
    return ps, pa, books, np.zeros((3, ncb), dtype=np.int64)


def zero_residual_case(seed=0, CS=TIE_CS):
    """pa equals codeword 1500 of codebook 1, so the residual is exactly 0; codebook 2 then picks its codeword nearest the origin (placed at
    2053 and 5: the answer is 5), and codebook 3 the one nearest the residual that leaves. ps equals codeword 2099 of codebook 0."""
    rng = np.random.default_rng([seed, 2])
    D, ncb = TIE_D, 4
    ps, pa = _small(rng, D), _small(rng, D)
    books = np.zeros((ncb, CS, D), dtype=np.float32)
    books[0] = _far(rng, CS, D); books[0][2099] = ps
    books[1] = _far(rng, CS, D); books[1][1500] = pa
    books[2], r = _place(rng, np.zeros(D, dtype=np.float32), CS, (5, 2053), (7, 1029))
    books[3], _ = _place(rng, r, CS, (1024,), (0,))
    return ps[None], pa[None], books, np.array([[2099, 1500, 5, 1024]], dtype=np.int64)


def size_case(CS, seed=0):
    """one distinguished nearest codeword at CS - 1 in each of three codebooks"""
    return tie_case((CS - 1,), seed=seed, CS=CS, ncb=3)

"""Pins tests/_sampler_ref.py before a GPU is involved: q3o_sample lies in the float64 admissible set on every generated row, the sets are
narrow enough to mean something, and a sampler with one of six classic mistakes leaves them (so tests/test_sampler_gpu.py would fail for
a kernel with the same mistake, whether or not the oracle shared it)."""
import collections

import numpy as np
import pytest

import _sampler_ref as R

f32 = np.float32


# ---- the sampler restated in f32 (numpy: element-wise f32 operations, np.cumsum for the sequential f32 sums), with six switches ---------
def _fma(a, b, c):
    """fmaf on f32 arrays: the product is exact in float64; the sum is rounded to odd there, so that the rounding to f32 is the only one."""
    prod = a.astype(np.float64) * b.astype(np.float64)
    c = c.astype(np.float64)
    s = prod + c
    bb = s - prod
    err = (prod - (s - bb)) + (c - bb)
    even = (s.view(np.int64) & 1) == 0
    s = np.where((err != 0.0) & even, np.nextafter(s, np.where(err > 0.0, np.inf, -np.inf)), s)
    return s.astype(f32)


def expf(x):
    """q3o_expf on an f32 array."""
    x = np.asarray(x, dtype=f32)
    zero = x < f32(-87.0)
    xc = np.where(zero, f32(0.0), x)
    n = np.rint(xc * f32(1.44269504088896341))
    r = _fma(n, np.full_like(n, f32(-0.693145751953125)), xc)
    r = _fma(n, np.full_like(n, f32(-1.42860682030941723212e-6)), r)
    p = np.full_like(r, f32(1.0) / f32(720.0))
    for d in (f32(1.0) / f32(120.0), f32(1.0) / f32(24.0), f32(1.0) / f32(6.0), f32(0.5), f32(1.0), f32(1.0)):
        p = _fma(p, r, np.full_like(r, d))
    out = (p.astype(np.float64) * np.exp2(n.astype(np.float64))).astype(f32)
    return np.where(zero, f32(0.0), out)


MUTATIONS = ("cut_gt", "top_k_plus_1", "tie_order", "divide_after_exp", "no_renormalisation", "pick_le")


def restated(logits, limit, T, top_k, top_p, r, wrong=None):
    x = np.asarray(logits[:limit], dtype=f32)
    T, top_p, r = f32(T), f32(top_p), f32(r)
    if T <= 0:
        return int(np.argmax(np.where(np.isnan(x), f32(-np.inf), x)))
    if wrong == "tie_order":
        order = (limit - 1) - np.argsort(-x[::-1], kind="stable")
    else:
        order = np.argsort(-x, kind="stable")
    n = limit
    if top_k < 0:
        top_k = 1 << 62
    if 0 < top_k < limit:
        n = min(top_k + 1, limit) if wrong == "top_k_plus_1" else top_k
    order = order[:n]
    v = x[order]
    with np.errstate(invalid="ignore", over="ignore"):
        p = expf(v - v[0]) / T if wrong == "divide_after_exp" else expf((v - v[0]) / T)
        s = np.cumsum(p)[-1]
        if s > 0:
            p = p / s
        if top_p < 1:
            cum = np.cumsum(p)
            hit = np.nonzero(cum > top_p if wrong == "cut_gt" else cum >= top_p)[0]
            n = int(hit[0]) + 1 if hit.size else n
            p = p[:n]
            ns = np.cumsum(p)[-1]
            if ns > 0 and wrong != "no_renormalisation":
                p = p / ns
        cum = np.cumsum(p)
    hit = np.nonzero(r <= cum if wrong == "pick_le" else r < cum)[0]
    return int(order[hit[0]]) if hit.size else int(order[0])


# ---- one walk over the cases, shared ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def calls():
    return list(R.cases(0))   # the logits of a (family, limit) are one shared array: ~37 MB in all


@pytest.fixture(scope="module")
def walked(oracle, calls):
    """Per call: (the oracle's ids, the admissible sets)."""
    L = oracle.lib()
    out = []
    for (fam, limit, T, k, p, lg, r) in calls:
        ids = [L.q3o_sample(oracle.ptr(lg[i], oracle.f32p), limit, T, k, p, float(r[i])) for i in range(lg.shape[0])]
        out.append((ids, [R.admissible(lg[i], limit, T, k, p, r[i]) for i in range(lg.shape[0])]))
    return out


def test_expf_error_fits_the_room_left_for_it():
    e = R.expf_rel_error()
    print("q3o_expf against np.exp, worst relative error: %.3g" % e)
    assert e <= R.EXPF_REL_BOUND < 8 * 2.0 ** -23


def test_restated_expf_is_the_oracles(oracle):
    L = oracle.lib()
    rng = np.random.default_rng(1)
    xs = np.concatenate([rng.uniform(-90.0, 0.0, 20000), -np.exp(rng.uniform(-30.0, 4.5, 20000)), [0.0, -0.0, -87.0, -np.inf]]).astype(f32)
    ref = np.array([L.q3o_expf(float(x)) for x in xs], dtype=f32)
    assert np.array_equal(expf(xs).view(np.uint32), ref.view(np.uint32))


def test_generator_reaches_every_pair_of_axis_values(calls):
    seen = collections.defaultdict(set)
    for (fam, limit, T, k, p, lg, r) in calls:
        assert lg.shape == (R.ROWS, R.LD) and lg.dtype == np.float32 and r.shape == (R.ROWS,) and r.dtype == np.float32
        if fam == "nan":
            continue
        assert np.all(lg[:, limit:] == R.BEYOND) and not np.isnan(lg).any() and np.isfinite(lg[:, :limit]).any(axis=1).all()
        seen["fl"].add((fam, limit))
        if T > 0:
            seen["lk"].add((limit, k)); seen["lp"].add((limit, p)); seen["lT"].add((limit, T))
            seen["fk"].add((fam, k if k <= 257 else "limit")); seen["fp"].add((fam, p)); seen["fT"].add((fam, T))
            seen["kp"].add((k if k <= 257 else "limit", p)); seen["kT"].add((k if k <= 257 else "limit", T)); seen["pT"].add((p, T))
            assert r[0] == 0.0 and np.all((r >= 0.0) & (r < 1.0))
        else:
            seen["greedy"].add((fam, limit))
    temps = [t for t in R.TEMPS if t > 0]
    both = [(f, l) for f in R.FAMILIES for l in R.LIMITS]
    assert seen["fl"] == set(both) == seen["greedy"]
    assert seen["lk"] >= {(l, k) for l in R.LIMITS for k in R.top_ks(l)}
    assert seen["lp"] == {(l, p) for l in R.LIMITS for p in R.TOP_PS} and seen["lT"] == {(l, t) for l in R.LIMITS for t in temps}
    assert seen["fp"] == {(f, p) for f in R.FAMILIES for p in R.TOP_PS} and seen["fT"] == {(f, t) for f in R.FAMILIES for t in temps}
    ks = [-1, 0, 1, 2, 40, 255, 256, 257, "limit"]
    assert seen["fk"] >= {(f, k) for f in R.FAMILIES for k in ks}
    assert seen["kp"] >= {(k, p) for k in ks for p in R.TOP_PS} and seen["kT"] >= {(k, t) for k in ks for t in temps}
    assert seen["pT"] == {(p, t) for p in R.TOP_PS for t in temps}


def test_oracle_lies_in_the_admissible_set_on_every_row(calls, walked):
    out = [(c[:5], i, float(c[6][i]), ids[i], sorted(sets[i])[:4]) for c, (ids, sets) in zip(calls, walked)
           for i in range(R.ROWS) if ids[i] not in sets[i]]
    assert not out, (len(out), out[:5])
    assert all(0 <= i < c[1] for c, (ids, _) in zip(calls, walked) for i in ids)


def test_admissible_sets_are_narrow(calls, walked):
    """Conditions on the inputs: >= 90 % of the rows of SINGLETON_FAMILIES have one admissible id, and no row with T <= 1 and at most 257
    candidates after top-k (top_k of 0 or below keeps `limit` of them) has more than 3. Achieved on cases(0): 96.2 % and 3."""
    single = total = widest = 0
    for (fam, limit, T, k, p, lg, r), (_, sets) in zip(calls, walked):
        if fam in R.SINGLETON_FAMILIES:
            total += len(sets)
            single += sum(len(s) == 1 for s in sets)
        if T <= 1.0 and R.kept(limit, k) <= 257:
            widest = max(widest, max(len(s) for s in sets))
    print("singleton share %.4f over %d rows, widest small set %d" % (single / total, total, widest))
    assert single >= 0.9 * total and widest <= 3


def test_restatement_equals_the_oracle_on_every_row(calls, walked):
    for (fam, limit, T, k, p, lg, r), (ids, _) in zip(calls, walked):
        got = [restated(lg[i], limit, T, k, p, r[i]) for i in range(R.ROWS)]
        assert got == ids, (fam, limit, T, k, p)


@pytest.mark.parametrize("wrong", MUTATIONS)
def test_a_wrong_sampler_leaves_the_admissible_set(calls, walked, wrong):
    for (fam, limit, T, k, p, lg, r), (_, sets) in zip(calls, walked):
        if T <= 0:
            continue
        for i in range(R.ROWS):
            got = restated(lg[i], limit, T, k, p, r[i], wrong=wrong)
            if got not in sets[i]:
                print("%s: caught by %s limit %d T %g top_k %d top_p %g row %d r %.9g: id %d, admissible %s"
                      % (wrong, fam, limit, T, k, p, i, r[i], got, sorted(sets[i])))
                return
    pytest.fail("no generated case tells a sampler with '%s' from the definition" % wrong)


def test_overflow_cases_overflow_the_select_list(calls):
    """The select path lists more than Q3_SAMP_MAX / 2 = 2048 keys on these rows (and must then take the sort); 2049 cannot overflow (the
    thread whose maximum is the threshold always holds smaller keys), it fills the list to its last places instead."""
    n = 0
    for (fam, limit, T, k, p, lg, r) in calls:
        if fam == "overflow" and T > 0 and limit in (2049, 2160, 4096) and k in (255, 256):
            lens = [R.select_list_length(row, limit, k) for row in lg]
            n += 1
            if limit == 2049:
                assert all(2048 - 16 <= m <= 2048 for m in lens), (limit, k, lens)
            else:
                assert all(m > 2048 for m in lens), (limit, k, lens)
    assert n >= 12
    # (the usual case, Gaussian logits at top_k = 40, lists about 2 k keys)
    assert all(40 <= R.select_list_length(row, 2160, 40) <= 400 for row in R.family_rows("gauss2", np.random.default_rng(0), 2160, 4))

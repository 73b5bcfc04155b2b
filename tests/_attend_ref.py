"""The attention kernels of csrc/q3_attend.hip against a two-stage float64 reference: the cases, their inputs and the checks that
tests/test_attend_cpu.py (the oracle alone) and tests/test_attend_gpu.py (the device) share.

A single-stage float64 reference (float64 all the way, K rounded to bf16 at the end: _f64_decode of tests/test_long_gpu.py) cannot carry
a tight bound over many rows: where a key element's float64 value lies next to a bf16 rounding midpoint, the f32 path and the float64
path cache different bf16 neighbours and a peaked softmax amplifies the difference to 1e-3. So the reference is split at the cache:
  stage 1 (preparation): q / k after RMSNorm + M-RoPE in float64 from the f32 tables. A cached K element must be RNE-to-bf16 of the float64
    value, except within STAGE1_MIDPOINT (relative) of a rounding midpoint, where either neighbour passes; the share of such elements is
    capped at STAGE1_SHARE_CAP. V must be bf16 of the input exactly.
  stage 2 (attention proper): scores, softmax and the value sum in float64 from the f32 q of stage 1 and the bf16 K / V AS CACHED; the
    error is relative to max |V| of the (slot, KV head), the bound is ATT_STAGE2_TOL of tests/_oracle.py.
A sequence is (pos0, n): rows 0 .. pos0 - 1 are only cached (a voice prefix, or the earlier decode steps), rows pos0 .. pos0 + n - 1 attend.
"""
import zlib

import numpy as np

HD = 128
SECTIONS = np.array([24, 20, 20, 0], dtype=np.int32)
THETA, EPS = 1e6, 1e-6
STAGE1_MIDPOINT = 2.0 ** -20
STAGE1_SHARE_CAP = 5e-3
KINDS = ("normal", "wide", "first", "newest", "uniform", "outliers", "zero_block")
ZERO_BLOCK = 1          # kind zero_block: value columns 32 .. 63 of every KV head are zero in every key
SEED = 20


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def bf16_bits(a):
    u = np.ascontiguousarray(a, dtype=np.float32).view(np.uint32).astype(np.uint64)
    u = u + 0x7FFF + ((u >> 16) & 1)
    return (u >> 16).astype(np.uint16)


def bf16_value(b):
    return (np.ascontiguousarray(b, dtype=np.uint16).astype(np.uint32) << 16).view(np.float32)


def rope_tables(n, hd=HD, theta=THETA, sections=SECTIONS):
    """The device's / oracle's table: angle in double, cos / sin rounded to f32."""
    half = hd // 2
    s3 = int(sections[:3].sum())
    i = np.arange(half)
    inv = np.power(float(theta), -2.0 * i / hd)
    ang = np.arange(n)[:, None].astype(np.float64) * inv[None, :]
    ang[:, i >= s3] = 0.0
    return np.cos(ang).astype(np.float32), np.sin(ang).astype(np.float32)


TABLES = rope_tables(320)


# ---- the cases ----------------------------------------------------------------------------------------------------------------------
def _v(n_ctx, kernel, decode=None, prefill=None):
    return dict(n_ctx=n_ctx, kernel=kernel, decode=decode, prefill=prefill)


_DEC13 = [1, 2, 3, 15, 16, 17, 18, 31, 32, 33, 48, 63, 64]
_RUNS_B = [(1, 1), (63, 1), (64, 64), (65, 63), (100, 28), (128, 128), (129, 127), (192, 64), (255, 1), (0, 5), (0, 128)]
_EDGES = (63, 64, 127, 128, 191, 192, 255, 256)


def _out_small(i, pos0, n):      # the end of k_attend_small's pre-requested value rows, and the newest key
    return (15, 16, pos0)


def _out_runs(i, pos0, n):       # key-block edges, the first row of the run and the key before it, the newest key of the last row
    return _EDGES + (pos0 - 1, pos0, pos0 + n - 1)


def _out_pair(i, pos0, n):
    return (i % 2,)


# hook: "decode" (one fused launch, q3tts_k_attention_decode_ex), "runs" (q3tts_k_attention_runs), "pair" (q3tts_k_attention_pair).
# Every variant of a spec runs the same inputs through another kernel (a policy or an n_ctx that the launcher's choice depends on).
SPECS = [
    dict(name="decode13", hook="decode", heads=(4, 2), seqs=[(n - 1, 1) for n in _DEC13], outliers=_out_small,
         variants=[_v(64, "k_attend_small<2>"), _v(128, "k_attend_gqa2", decode=0), _v(128, "k_attend<2, true>", decode=1)]),
] + [
    dict(name="rowidx%d" % n, hook="decode", heads=(4, 2), seqs=[(n - 1, 1)] * 3, outliers=_out_small, row_indexed=True,
         variants=[_v(64, "k_attend_small<2>")]) for n in (1, 2, 17, 18, 64)
] + [
    dict(name="decode_r4", hook="decode", heads=(4, 1), seqs=[(n - 1, 1) for n in (1, 2, 17, 64, 65, 128)], outliers=_out_runs,
         variants=[_v(128, "k_attend<4, true>")]),
] + [
    dict(name="pair%d" % b, hook="pair", heads=(4, 2), seqs=[(0, 2)] * b, outliers=_out_pair, variants=[_v(64, "k_attend_pair")])
    for b in (1, 2, 5, 64)
] + [
    dict(name="prefill_a", hook="runs", heads=(4, 2), seqs=[(0, n) for n in (1, 2, 7, 8, 9, 63, 64, 65, 127, 128)], outliers=_out_runs,
         variants=[_v(128, "k_attend_prefill", prefill=2), _v(128, "k_attend<2, false>", prefill=1)]),
    dict(name="prefill_b", hook="runs", heads=(4, 2), seqs=_RUNS_B, outliers=_out_runs,
         variants=[_v(256, "k_attend_prefill", prefill=2), _v(256, "k_attend<2, false>", prefill=1)]),
    dict(name="runs_129", hook="runs", heads=(4, 2), seqs=[(0, 129)], outliers=_out_runs, variants=[_v(192, "k_attend<2, false>", prefill=2)]),
    dict(name="runs_200_100", hook="runs", heads=(4, 2), seqs=[(200, 100)], outliers=_out_runs, variants=[_v(320, "k_attend<2, false>", prefill=2)]),
    dict(name="runs_r1", hook="runs", heads=(2, 2), seqs=[(0, 70), (250, 10)], outliers=_out_runs, variants=[_v(320, "k_attend<1, false>", prefill=2)]),
    dict(name="runs_r4", hook="runs", heads=(4, 1), seqs=[(0, 70), (250, 10)], outliers=_out_runs, variants=[_v(320, "k_attend<4, false>", prefill=2)]),
]
SPEC = {s["name"]: s for s in SPECS}


def pick_args(spec, variant):
    """The arguments of q3tts_k_attend_pick (native.k_attend_pick) for a variant's launch."""
    Hq, Hkv = spec["heads"]
    a = dict(fused={"decode": 1, "pair": 2, "runs": 0}[spec["hook"]], gqa_ratio=Hq // Hkv, n_ctx=variant["n_ctx"], n_kv_head=Hkv)
    if spec["hook"] == "runs":
        a.update(n_seg=len(spec["seqs"]), seg_max_n=max(n for _, n in spec["seqs"]), seg_max_t=max(p + n for p, n in spec["seqs"]))
    return a


# ---- inputs -------------------------------------------------------------------------------------------------------------------------
def _rot(x, pos):
    half = HD // 2
    c, s = TABLES[0][pos].astype(np.float64), TABLES[1][pos].astype(np.float64)
    a, b = x[..., :half].astype(np.float64), x[..., half:].astype(np.float64)
    return np.concatenate([a * c - b * s, b * c + a * s], axis=-1)


def make_inputs(spec, kind, seed=SEED):
    """(xs, qn, kn): the qkv rows [pos0 + n][(Hq + 2 Hkv) HD] of every sequence and the norm weights, for one input kind — the
    constructions of tests/test_long_gpu.py::_decode_case: standard normals; `wide` (norm weights x 4: a score spread > 100); `first` (the
    key at t = 0 is the last row's query, rotated: score ~ 45); `newest` (every row's key is its own query); `uniform` (k_norm_w = 0);
    `outliers` (+-300 value rows at spec["outliers"]); `zero_block` (a value column block that is zero in every key)."""
    Hq, Hkv = spec["heads"]
    R = Hq // Hkv
    rng = np.random.default_rng([seed, zlib.crc32(spec["name"].encode()), KINDS.index(kind)])
    qn = (1.0 + rng.standard_normal(HD) * 0.05).astype(np.float32)
    kn = (1.0 + rng.standard_normal(HD) * 0.05).astype(np.float32)
    if kind == "wide":
        qn, kn = qn * 4.0, kn * 4.0
    if kind in ("first", "newest"):
        qn = kn = np.full(HD, 2.0, dtype=np.float32)   # uniform weights: the norm commutes with the rotation
    if kind == "uniform":
        kn = np.zeros(HD, dtype=np.float32)
    xs = []
    for i, (pos0, n) in enumerate(spec["seqs"]):
        tot = pos0 + n
        x = rng.standard_normal((tot, (Hq + 2 * Hkv) * HD)).astype(np.float32)
        q = x[:, :Hq * HD].reshape(tot, Hkv, R, HD)
        k = x[:, Hq * HD:(Hq + Hkv) * HD].reshape(tot, Hkv, HD)
        v = x[:, (Hq + Hkv) * HD:].reshape(tot, Hkv, HD)
        if kind in ("first", "newest"):
            q[:] = q[:, :, :1]          # every query head of a group the same: the dominant key dominates all of them
        if kind == "newest":
            k[:] = q[:, :, 0]
        if kind == "first" and tot > 1:
            k[0] = _rot(q[tot - 1, :, 0], tot - 1).astype(np.float32)
        if kind == "outliers":
            for j, t in enumerate(sorted(set(spec["outliers"](i, pos0, n)))):
                if 0 <= t < tot:
                    v[t] = 300.0 if (j + i) % 2 == 0 else -300.0
        if kind == "zero_block":
            v[:, :, 32 * ZERO_BLOCK:32 * ZERO_BLOCK + 32] = 0.0
        xs.append(x)
    return xs, qn, kn


def hook_rows(spec, xs):
    """The sequences' rows in the order the spec's hook takes them."""
    if spec["hook"] == "pair":
        return np.concatenate([np.stack([x[0] for x in xs]), np.stack([x[1] for x in xs])])
    return np.concatenate(xs)


def hook_out_split(spec, out):
    """A hook's output rows, per sequence: [n][...] each."""
    if spec["hook"] == "pair":
        b = len(spec["seqs"])
        return [np.stack([out[i], out[b + i]]) for i in range(b)]
    res, r = [], 0
    for _, n in spec["seqs"]:
        res.append(out[r:r + n])
        r += n
    return res


# ---- the oracle ---------------------------------------------------------------------------------------------------------------------
def oracle_seq(O, x, pos0, n, Hq, Hkv, qn, kn):
    """The oracle on one sequence: out [n][Hq HD] of the attending rows (q3o_attention over the whole sequence), and its preparation stage
    for ALL rows: q f32 [tot][Hq][HD], K / V as cached, bf16 bits [tot][Hkv][HD]."""
    L = O.lib()
    tot = pos0 + n
    x = np.ascontiguousarray(x, dtype=np.float32)
    sec = np.ascontiguousarray(SECTIONS)
    out = np.zeros((tot, Hq * HD), dtype=np.float32)
    L.q3o_attention(O.ptr(x, O.f32p), tot, 0, Hq, Hkv, HD, O.ptr(qn, O.f32p), O.ptr(kn, O.f32p), EPS, THETA, O.ptr(sec, O.i32p), O.ptr(out, O.f32p))
    q = np.zeros((tot, Hq, HD), dtype=np.float32)
    k = np.zeros((tot, Hkv, HD), dtype=np.float32)
    v = np.zeros((tot, Hkv, HD), dtype=np.float32)
    L.q3o_attention_prep(O.ptr(x, O.f32p), tot, 0, Hq, Hkv, HD, O.ptr(qn, O.f32p), O.ptr(kn, O.f32p), EPS, THETA, O.ptr(sec, O.i32p),
                         O.ptr(q, O.f32p), O.ptr(k, O.f32p), O.ptr(v, O.f32p))
    assert not (bits(k) & 0xFFFF).any() and not (bits(v) & 0xFFFF).any()
    return out[pos0:].copy(), q, (bits(k) >> 16).astype(np.uint16), (bits(v) >> 16).astype(np.uint16)


_ORACLE_CACHE = {}


def oracle_case(O, spec, kind):
    """(xs, qn, kn, per-sequence oracle_seq results) of one (spec, kind): computed once, shared, never changed."""
    key = (spec["name"], kind)
    if key not in _ORACLE_CACHE:
        xs, qn, kn = make_inputs(spec, kind)
        Hq, Hkv = spec["heads"]
        res = [oracle_seq(O, x, p, n, Hq, Hkv, qn, kn) for x, (p, n) in zip(xs, spec["seqs"])]
        for a in xs + [qn, kn] + [r for t in res for r in t]:
            a.setflags(write=False)
        _ORACLE_CACHE[key] = (xs, qn, kn, res)
    return _ORACLE_CACHE[key]


# ---- stage 1 ------------------------------------------------------------------------------------------------------------------------
def prep64(h, w, pos, defect=None, want_mag=False):
    """RMSNorm + M-RoPE of heads h [rows][heads][HD] at positions pos [rows] in float64 from the f32 tables. want_mag: also the magnitude
    of the rotated pair each element belongs to, |(y_i, y_{i + HD/2})| (the rotation keeps it)."""
    half = HD // 2
    h = h.astype(np.float64)
    y = h / np.sqrt(np.mean(h * h, axis=-1, keepdims=True) + EPS) * w.astype(np.float64)
    c, s = TABLES[0][pos].astype(np.float64)[:, None, :], TABLES[1][pos].astype(np.float64)[:, None, :]
    if defect == "rope_adjacent":   # pairs (2 i, 2 i + 1) instead of (i, i + HD / 2)
        a, b = y[..., 0::2], y[..., 1::2]
        o = np.empty_like(y)
        o[..., 0::2], o[..., 1::2] = a * c - b * s, b * c + a * s
        return o
    a, b = y[..., :half], y[..., half:]
    o = np.concatenate([a * c - b * s, b * c + a * s], axis=-1)
    if want_mag:
        m = np.hypot(a, b)
        return o, np.concatenate([m, m], axis=-1)
    return o


def rne_bf16(x):
    """float64 -> the nearest bf16 value, ties to even (normal range; 0 stays 0)."""
    _, e = np.frexp(np.abs(x))
    ulp = np.ldexp(1.0, e - 8)                  # |x| in [2^(e-1), 2^e): 8 significant bits
    return np.rint(x / ulp) * ulp


def bf16_window(x, mag=None):
    """(lo, hi, near): the bf16 values that RNE gives for x - w and x + w, w = STAGE1_MIDPOINT x |x| (or x mag >= |x| where given) — a cached
    element passes when it lies in [lo, hi] —, and near = lo != hi: a rounding midpoint lies within w of x, the exception is in use."""
    w = STAGE1_MIDPOINT * (np.abs(x) if mag is None else np.maximum(np.abs(x), mag))
    lo, hi = rne_bf16(x - w), rne_bf16(x + w)
    return lo, hi, lo != hi


def check_stage1(x, Hq, Hkv, kn, k_bits, v_bits, strict_count=None):
    """The cached K / V (bf16 bits [tot][Hkv][HD]) of a sequence against stage 1. Returns (elements, near-midpoint elements, of those: the
    ones not cached as RNE of the float64 value); raises on a K element outside the rule or a V element that is not bf16 of its input.
    The midpoint window is relative to the magnitude of the rotated PAIR, not of the element: the rotation a c - b s cancels, and an f32
    path carries an error of a few 2^-24 of |(a, b)| whatever is left of the element (an element of 3.5e-5 out of a pair of 4 sits 1e-7
    from its midpoint: 2^-18 of itself, 2^-25 of the pair; an element of 1e-5 has a bf16 spacing of 6e-8, below that error). strict_count
    (a list): collects the number of elements that are not RNE of the float64 value and lie OUTSIDE a window relative to the element alone."""
    tot = x.shape[0]
    xr = x.reshape(tot, Hq + 2 * Hkv, HD)
    assert np.array_equal(v_bits, bf16_bits(xr[:, Hq + Hkv:])), "V is not bf16 of the input"
    k64, mag = prep64(xr[:, Hq:Hq + Hkv], kn, np.arange(tot), want_mag=True)
    lo, hi, near = bf16_window(k64, mag)
    got = bf16_value(k_bits).astype(np.float64)
    ok = (lo <= got) & (got <= hi)
    if not ok.all():
        i = tuple(int(t) for t in np.argwhere(~ok)[0])
        raise AssertionError(f"cached K element {i}: float64 {k64[i]!r}, accepted bf16 values {lo[i]!r} .. {hi[i]!r}, cached {got[i]!r}")
    flipped = got != rne_bf16(k64)
    if strict_count is not None:
        slo, shi, _ = bf16_window(k64)
        strict_count.append(int((flipped & ~((slo <= got) & (got <= shi))).sum()))
    return k64.size, int(near.sum()), int((near & flipped).sum())


# ---- stage 2 ------------------------------------------------------------------------------------------------------------------------
def attend64(q, k, v, pos0, Hq, Hkv, defect=None):
    """Attention proper in float64: q [n][Hq][HD] of the rows at positions pos0 .., k / v [tot][Hkv][HD] as cached. out [n][Hq HD]."""
    n, tot = q.shape[0], k.shape[0]
    R = Hq // Hkv
    q, k, v = q.astype(np.float64), k.astype(np.float64), v.astype(np.float64)
    pos = pos0 + np.arange(n)
    last = pos + {"long": 1, "short": -1, "no_newest": -1}.get(defect, 0)      # the last key a row attends to
    last = np.clip(last, 0, tot - 1)
    mask = np.arange(tot)[None, :] <= last[:, None]
    out = np.zeros((n, Hq, HD))
    for h in range(Hq):
        g = h % Hkv if defect == "group_mod" else h // R
        sc = q[:, h] @ k[:, g].T
        if defect != "no_scale":
            sc = sc / np.sqrt(HD)
        sc = np.where(mask, sc, -np.inf)
        p = np.exp(sc - sc.max(axis=1, keepdims=True))
        out[:, h] = (p @ v[:, g]) / p.sum(axis=1, keepdims=True)
    return out.reshape(n, Hq * HD)


def vmax_per_head(v_bits, Hq, Hkv):
    """max |V| of the sequence's KV heads, repeated per output column: [Hq HD]."""
    m = np.abs(bf16_value(v_bits).astype(np.float64)).max(axis=(0, 2))
    return np.repeat(np.maximum(m, 1e-30), (Hq // Hkv) * HD)


def stage2_error(out, q, k_bits, v_bits, pos0, Hq, Hkv):
    """Worst |out - float64| / max |V| over the sequence's attending rows; q: stage 1's f32 q of those rows, k / v as cached."""
    ref = attend64(q, bf16_value(k_bits), bf16_value(v_bits), pos0, Hq, Hkv)
    return float((np.abs(out.astype(np.float64) - ref) / vmax_per_head(v_bits, Hq, Hkv)).max())


def full64(x, pos0, n, Hq, Hkv, qn, kn, defect=None):
    """Both stages in float64 (K / V rounded to bf16 as the cache stores them), with one planted defect or none. out [n][Hq HD]."""
    tot = pos0 + n
    xr = x.reshape(tot, Hq + 2 * Hkv, HD)
    pos = np.arange(tot)
    if defect == "rope_pos_r":      # the run's rows rotated at r instead of pos0 + r (the prefix rows keep their positions)
        pos = np.concatenate([np.arange(pos0), np.arange(n)])
    pd = defect if defect == "rope_adjacent" else None
    k = rne_bf16(prep64(xr[:, Hq:Hq + Hkv], kn, pos, pd))
    v = bf16_value(bf16_bits(xr[:, Hq + Hkv:]))
    q = prep64(xr[pos0:, :Hq], qn, pos[pos0:], pd)
    return attend64(q, k, v, pos0, Hq, Hkv, defect)


# the defects a wrong kernel could have, and the specs on which each is planted (a spec where the defect can show: a key after the row's
# own for `long`, pos0 > 0 for `rope_pos_r`, a fused kernel — newest key served from LDS — for `no_newest`)
DEFECTS = {
    "long": ("prefill_a", "prefill_b"),
    "short": ("prefill_a", "prefill_b"),
    "group_mod": ("prefill_a", "decode13"),
    "rope_adjacent": ("prefill_a", "decode13"),
    "rope_pos_r": ("prefill_b", "runs_200_100"),
    "no_scale": ("prefill_a", "decode13"),
    "no_newest": ("decode13", "pair5"),
}

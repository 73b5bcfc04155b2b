"""The Talker's K/V cache as ggml Q8_0 blocks (q3tts_engine_config.kv_q8_0, csrc/q3_attend_kv8.hip): the cases and the
two-stage float64 checks that tests/test_kv_q8_cpu.py (numpy alone) and tests/test_kv_q8_gpu.py (the device) share. The reference is the
one of tests/_attend_ref.py, split at the cache:
  stage 1, K: with k64 = prep64(...) (RMSNorm + M-RoPE in float64) and a64 = max |k64| of a block of 32 dims, the cached scale must be
    f16-RNE of a64 / 127 — or any f16 value RNE gives inside (a64 / 127)(1 +- SCALE_WINDOW) —, each quant round-half-away of
    u = k64 * 127 / a64 — where u lies within QUANT_WINDOW of a half-integer either neighbour passes —, a zero block exactly d = 0, q = 0.
    At most SHARE_CAP of the elements and of the blocks may lie where their exception applies.
  stage 1, V: quants and scales equal q3o_quantize_q8_0 of the f32 input rows, bit for bit.
  stage 2: attend64 from the oracle's f32 q and the cache AS RETURNED, x^ = f32(d) * q (exact in f32); error relative to max |v^| of the
    (slot, KV head); bound ATT_STAGE2_TOL of tests/_oracle.py — the same f32 chains over exactly represented values.
Checked on the CPU with the numpy-f32 restatement below on every non-pair, non-row-indexed spec x kind of tests/_attend_ref.py
(6 247 808 elements, 195 244 blocks): 12 quants differ from the float64 rounding, the worst 1.5e-5 from its half-integer; 1.7e-3 of the
elements lie inside the quant window; 17 scales differ, none outside the scale window; 2.4e-3 of the blocks lie inside it.
test_kv_q8_cpu.py prints its own counts the same way."""
import numpy as np

import _attend_ref as A
from _attend_ref import SPECS, KINDS, make_inputs, prep64, attend64, oracle_seq, hook_rows  # noqa: F401 (re-exported for the two test files)

HD = A.HD
NB = HD // 32
SCALE_WINDOW = 2.0 ** -20
QUANT_WINDOW = 2.0 ** -10
SHARE_CAP = 5e-3

# the kernels of csrc/q3_attend_kv8.hip as q3tts_k_attend_pick_kv8 numbers them
KERNELS = {9: "k_attend_kv8<1, false>", 10: "k_attend_kv8<2, false>", 11: "k_attend_kv8<4, false>", 12: "k_attend_kv8<2, true>",
           13: "k_attend_kv8<4, true>", 14: "k_attend_gqa2_kv8"}

# decode_long: k_attend_gqa2_kv8's loops beyond 256 keys and the key-block edges around them
DECODE_LONG = dict(name="decode_long", hook="decode", heads=(4, 2), seqs=[(n - 1, 1) for n in (255, 256, 257, 300, 320)], outliers=A._out_runs,
                   variants=[])
SPEC = dict(A.SPEC, decode_long=DECODE_LONG)


def _c(spec, n_ctx, *variants, forms=(0,)):
    return dict(spec=SPEC[spec], n_ctx=n_ctx, variants=list(variants), forms=forms)


# (decode policy or prefill policy, expected kernel): every case names its kernel; together all six
CASES = {c["spec"]["name"]: c for c in [
    _c("decode13", 128, (0, 14), (1, 12), forms=(0, 1, 2)),
    _c("decode_r4", 128, (-1, 13)),
    _c("decode_long", 320, (0, 14), (1, 12)),
    _c("prefill_a", 128, (2, 10), forms=(0, 1, 2)),
    _c("prefill_b", 256, (2, 10)),
    _c("runs_129", 192, (2, 10)),
    _c("runs_200_100", 320, (2, 10)),
    _c("runs_r1", 320, (2, 9)),
    _c("runs_r4", 320, (2, 11)),
]}


def pick_args(case):
    spec = case["spec"]
    Hq, Hkv = spec["heads"]
    a = dict(fused=1 if spec["hook"] == "decode" else 0, gqa_ratio=Hq // Hkv, n_ctx=case["n_ctx"], n_kv_head=Hkv)
    if spec["hook"] == "runs":
        a.update(n_seg=len(spec["seqs"]), seg_max_n=max(n for _, n in spec["seqs"]), seg_max_t=max(p + n for p, n in spec["seqs"]))
    return a


def launch(native, case, policy, xs, qn, kn, form=0):
    """One launch of the case through its _kv8 hook: the dict of native.k_attention_runs_kv8."""
    spec = case["spec"]
    Hq, Hkv = spec["heads"]
    tail = (case["n_ctx"], Hq, Hkv, HD, qn, kn, A.EPS, A.THETA, A.SECTIONS)
    if spec["hook"] == "decode":
        return native.k_attention_decode_kv8(hook_rows(spec, xs), [p + n for p, n in spec["seqs"]], *tail, policy=policy, out_form=form)
    return native.k_attention_runs_kv8(hook_rows(spec, xs), spec["seqs"], *tail, policy=policy, out_form=form)


# ---- the layout (csrc/q3_kernels.h: q3_kv8_k_off / q3_kv8_kd_idx), restated ----------------------------------------------------------------
def k_off(pos, d):
    """Byte offset of key element (pos, d) inside a head's K quants: [64-key block][HD / 16 chunks][64 keys][16]."""
    return (((pos >> 6) * (HD >> 4) + (d >> 4)) * 64 + (pos & 63)) * 16 + (d & 15)


def k_off_inv(off):
    e, kl, c, blk = off & 15, (off >> 4) & 63, (off >> 10) % (HD >> 4), (off >> 10) // (HD >> 4)
    return blk * 64 + kl, c * 16 + e


def kd_idx(pos, j):
    """Index of the scale of (pos, block j) inside a head's K scales: [64-key block][HD / 32][64 keys]."""
    return ((pos >> 6) * NB + j) * 64 + (pos & 63)


def kd_idx_inv(i):
    return (i // (NB * 64)) * 64 + (i & 63), (i >> 6) % NB


# ---- values ---------------------------------------------------------------------------------------------------------------------------
def f16_value(dbits):
    return np.ascontiguousarray(dbits, dtype=np.uint16).view(np.float16).astype(np.float32)


def dequant(q, dbits):
    """x^ = f32(d) * float(q), in f32 (exact: 11 x 7 significant bits). q [..., HD] int8, dbits [..., HD / 32] f16 bits -> f32 [..., HD]."""
    d = np.repeat(f16_value(dbits), 32, axis=-1)
    x = d * q.astype(np.float32)
    assert np.array_equal(x.astype(np.float64), d.astype(np.float64) * q.astype(np.float64))
    return x


def round_half_away(u):
    return np.sign(u) * np.floor(np.abs(u) + 0.5)


# ---- the numpy-f32 restatement of the preparation and the quantiser -----------------------------------------------------------------------
def prep32(h, w, pos):
    """RMSNorm + M-RoPE of heads h [rows][heads][HD] in plain f32 (not the device's summation order: a restatement, not an oracle)."""
    f = np.float32
    half = HD // 2
    h = h.astype(f)
    rinv = f(1.0) / np.sqrt((h * h).mean(axis=-1, keepdims=True, dtype=f) + f(A.EPS))
    y = (h * rinv) * w.astype(f)
    c, s = A.TABLES[0][pos][:, None, :], A.TABLES[1][pos][:, None, :]
    a, b = y[..., :half], y[..., half:]
    return np.concatenate([a * c - b * s, b * c + a * s], axis=-1).astype(f)


def quant32(x, defect=None):
    """ggml's quantize_row_q8_0 in f32 on the last axis (blocks of 32): (q int8 same shape, d f16 bits [..., n / 32]). defect: a planted
    mistake (tests/test_kv_q8_cpu.py)."""
    f = np.float32
    xb = np.ascontiguousarray(x, dtype=f).reshape(x.shape[:-1] + (x.shape[-1] // 32, 32))
    amax = np.abs(xb).max(axis=-1)
    d = (amax / f(128.0 if defect == "d128" else 127.0)).astype(f)
    with np.errstate(divide="ignore"):
        idv = np.where(d != 0, f(1.0) / d, f(0.0)).astype(f)
    u = (xb * idv[..., None]).astype(f)
    q = np.trunc(u) if defect == "trunc" else round_half_away(u)
    if defect == "neighbour_scale":
        d = d[..., np.arange(d.shape[-1]) ^ 1]
    return q.astype(np.int8).reshape(x.shape), d.astype(np.float16).view(np.uint16)


def cache32(x, Hq, Hkv, kn, defect=None):
    """The Q8_0 cache of a sequence's rows x [tot][(Hq + 2 Hkv) HD] by the restatement: k_q, k_d, v_q, v_d as [tot][Hkv][...]."""
    tot = x.shape[0]
    xr = x.reshape(tot, Hq + 2 * Hkv, HD)
    k = prep32(xr[:, Hq:Hq + Hkv], kn, np.arange(tot))
    v = xr[:, Hq + Hkv:]
    if defect == "v_bf16":
        v = A.bf16_value(A.bf16_bits(v))
    if defect == "blocks_along_keys":   # 32 consecutive KEYS of one dim share a scale (the sequence is padded to whole blocks of keys)
        pad = (-tot) % 32
        kp = np.concatenate([k, np.zeros((pad,) + k.shape[1:], dtype=np.float32)])
        q, d = quant32(np.ascontiguousarray(kp.transpose(1, 2, 0)))                      # [Hkv][HD][tot']
        k_q = np.ascontiguousarray(q.transpose(2, 0, 1))[:tot]
        dd = np.repeat(d, 32, axis=-1).transpose(2, 0, 1)[:tot]                          # the scale each element was quantised with
        k_d = np.ascontiguousarray(dd[:, :, ::32])                                       # ... reported per block of dims: its first element's
    else:
        k_q, k_d = quant32(k, defect if defect in ("d128", "trunc", "neighbour_scale") else None)
    v_q, v_d = quant32(v)
    return k_q, k_d, v_q, v_d


# ---- stage 1 ------------------------------------------------------------------------------------------------------------------------------
class Counts:
    """What stage 1 saw over the cases of one test: elements / blocks, how many lie inside their window, how many differ from the float64
    rounding, and the closest a differing quant came to the edge of its window."""

    def __init__(self):
        self.elems = self.near_q = self.diff_q = self.blocks = self.near_d = self.diff_d = 0
        self.worst_q = 0.0

    def line(self, what):
        return (f"{what}: {self.elems} elements, {self.blocks} blocks; quants: {self.diff_q} differ from the float64 rounding (worst "
                f"{self.worst_q:.1e} from its half-integer, window {QUANT_WINDOW:.1e}), share inside the window "
                f"{self.near_q / max(self.elems, 1):.1e}; scales: {self.diff_d} differ, share inside the window "
                f"{self.near_d / max(self.blocks, 1):.1e} (cap {SHARE_CAP:.0e} each)")

    def check_caps(self, what):
        assert self.near_q <= SHARE_CAP * self.elems, self.line(what)
        assert self.near_d <= SHARE_CAP * self.blocks, self.line(what)


def check_stage1_k(x, Hq, Hkv, kn, k_q, k_d, counts):
    """The cached keys of a sequence (k_q int8 [tot][Hkv][HD], k_d f16 bits [tot][Hkv][NB]) against stage 1; raises on a scale or a quant
    outside the rule, adds to counts."""
    tot = x.shape[0]
    k64 = prep64(x.reshape(tot, Hq + 2 * Hkv, HD)[:, Hq:Hq + Hkv], kn, np.arange(tot)).reshape(tot, Hkv, NB, 32)
    a64 = np.abs(k64).max(axis=-1)
    zero = a64 == 0
    got_d = np.ascontiguousarray(k_d, dtype=np.uint16)
    q = k_q.reshape(tot, Hkv, NB, 32).astype(np.float64)
    assert not got_d[zero].any() and not q[zero].any(), "a zero block must be exactly d = 0, q = 0"
    t = a64 / 127.0
    with np.errstate(over="ignore"):
        lo, hi, want = (t * (1 - SCALE_WINDOW)).astype(np.float16), (t * (1 + SCALE_WINDOW)).astype(np.float16), t.astype(np.float16)
    gv = got_d.view(np.float16)
    ok = (lo <= gv) & (gv <= hi)
    if not ok.all():
        i = tuple(int(v) for v in np.argwhere(~ok)[0])
        raise AssertionError(f"K scale of block {i}: a64 / 127 = {t[i]!r}, accepted f16 {lo[i]!r} .. {hi[i]!r}, cached {gv[i]!r}")
    with np.errstate(divide="ignore", invalid="ignore"):
        u = np.where(zero[..., None], 0.0, k64 * 127.0 / a64[..., None])
    strict = round_half_away(u)
    dist = np.abs(np.abs(u) - np.floor(np.abs(u)) - 0.5)          # distance of |u| from the half-integer inside its unit
    near = dist < QUANT_WINDOW
    other = np.sign(u) * (np.floor(np.abs(u)) + (np.abs(strict) == np.floor(np.abs(u))))   # the neighbour across the half-integer
    okq = (q == strict) | (near & (q == other))
    if not okq.all():
        i = tuple(int(v) for v in np.argwhere(~okq)[0])
        raise AssertionError(f"K quant {i}: u = {u[i]!r}, cached {q[i]!r}")
    dq = q != strict
    counts.elems += q.size; counts.near_q += int(near.sum()); counts.diff_q += int(dq.sum())
    counts.blocks += a64.size; counts.near_d += int((lo != hi).sum()); counts.diff_d += int((gv != want).sum())
    if dq.any():
        counts.worst_q = max(counts.worst_q, float(dist[dq].max()))


def check_stage1_v(oracle, x, Hq, Hkv, v_q, v_d):
    """V: quants and scales equal q3o_quantize_q8_0 of the f32 input rows, bit for bit."""
    tot = x.shape[0]
    want_q, want_d = oracle.quantize_q8_0(x.reshape(tot, Hq + 2 * Hkv, HD)[:, Hq + Hkv:])
    assert np.array_equal(v_q, want_q), "V quants are not q3o_quantize_q8_0 of the f32 rows"
    assert np.array_equal(np.ascontiguousarray(v_d, dtype=np.uint16), want_d), "V scales are not q3o_quantize_q8_0 of the f32 rows"


# ---- stage 2 ------------------------------------------------------------------------------------------------------------------------------
def stage2_error(out, q, k_q, k_d, v_q, v_d, pos0, Hq, Hkv):
    """Worst |out - float64| / max |v^| over the sequence's attending rows; q: the oracle's f32 q of those rows; the cache as returned."""
    kh, vh = dequant(k_q, k_d), dequant(v_q, v_d)
    ref = attend64(q, kh, vh, pos0, Hq, Hkv)
    vmax = np.repeat(np.maximum(np.abs(vh.astype(np.float64)).max(axis=(0, 2)), 1e-30), (Hq // Hkv) * HD)
    return float((np.abs(out.astype(np.float64) - ref) / vmax).max())


def attend32(q, k, v, pos0, Hq, Hkv):
    """Attention proper in plain f32 (numpy's summation order): what the CPU tests take for `the device's output`."""
    f = np.float32
    n, tot = q.shape[0], k.shape[0]
    R = Hq // Hkv
    mask = np.arange(tot)[None, :] <= (pos0 + np.arange(n))[:, None]
    out = np.zeros((n, Hq, HD), dtype=f)
    for h in range(Hq):
        g = h // R
        sc = (q[:, h].astype(f) @ k[:, g].astype(f).T) * f(1.0 / np.sqrt(HD))
        sc = np.where(mask, sc, f(-np.inf))
        p = np.exp(sc - sc.max(axis=1, keepdims=True)).astype(f)
        out[:, h] = (p @ v[:, g].astype(f)) / p.sum(axis=1, keepdims=True, dtype=f)
    return out.reshape(n, Hq * HD)


# ---- the grid inputs ----------------------------------------------------------------------------------------------------------------------
def grid_inputs(spec, seed=A.SEED):
    """Kind `uniform` (k_norm_w = 0: every score 0) with V on an int8 grid: v = 2^e * q, |q| <= 127, one |q| = 127 in every block, e
    varying per block. Then d = 2^e and x^ = v = bf16(v): the Q8_0 cache holds what the bf16 cache holds, and the output must be the
    oracle's (q3o_attention), all 32 bits."""
    Hq, Hkv = spec["heads"]
    xs, qn, kn = make_inputs(spec, "uniform", seed)
    rng = np.random.default_rng([seed, 8, len(spec["name"])])
    for x in xs:
        tot = x.shape[0]
        q = rng.integers(-127, 128, size=(tot, Hkv, NB, 32))
        at = rng.integers(0, 32, size=(tot, Hkv, NB))
        np.put_along_axis(q, at[..., None], np.where(rng.integers(0, 2, size=at.shape) == 1, 127, -127)[..., None], axis=-1)
        e = rng.integers(-6, 7, size=(tot, Hkv, NB, 1))
        v = np.ldexp(q.astype(np.float64), e).astype(np.float32)
        x.reshape(tot, Hq + 2 * Hkv, HD)[:, Hq + Hkv:] = v.reshape(tot, Hkv, HD)
        assert np.array_equal(A.bf16_value(A.bf16_bits(v)), v)
    return xs, qn, kn


# ---- the oracle's Q8_0 cache mode (q3o_attention_kv_q8; OracleModel.set_talker_kv_q8) ------------------------------------------------------
def oracle_q(O, x, Hq, Hkv, qn, kn):
    """The oracle's f32 q after RMSNorm + RoPE of every row of a sequence, [tot][Hq][HD] (q3o_attention_prep; its K / V outputs are the
    bf16 cache's and are not used here)."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    tot = x.shape[0]
    sec = np.ascontiguousarray(A.SECTIONS)
    q = np.zeros((tot, Hq, HD), dtype=np.float32)
    k = np.zeros((tot, Hkv, HD), dtype=np.float32)
    v = np.zeros((tot, Hkv, HD), dtype=np.float32)
    O.lib().q3o_attention_prep(O.ptr(x, O.f32p), tot, 0, Hq, Hkv, HD, O.ptr(qn, O.f32p), O.ptr(kn, O.f32p), A.EPS, A.THETA, O.ptr(sec, O.i32p),
                               O.ptr(q, O.f32p), O.ptr(k, O.f32p), O.ptr(v, O.f32p))
    return q


def oracle_seq_kv8(O, x, pos0, n, Hq, Hkv, qn, kn):
    """The oracle over a Q8_0 cache on one sequence: out [n][Hq HD] of the attending rows, and the cache k_q, k_d, v_q, v_d of ALL rows in
    natural order ([tot][Hkv][HD] int8, [tot][Hkv][NB] f16 bits) — the form test_kv_q8_gpu.py::_per_seq gives the hooks' cache."""
    assert x.shape[0] == pos0 + n
    return O.attention_kv_q8(x, pos0, Hq, Hkv, HD, qn, kn, A.EPS, A.THETA, A.SECTIONS)


_ORACLE_KV8 = {}


def oracle_case_kv8(O, spec, kind):
    """(xs, qn, kn, per-sequence oracle_seq_kv8 results) of one (spec, kind): computed once, shared, never changed. kind "grid": grid_inputs."""
    key = (spec["name"], kind)
    if key not in _ORACLE_KV8:
        xs, qn, kn = grid_inputs(spec) if kind == "grid" else make_inputs(spec, kind)
        Hq, Hkv = spec["heads"]
        res = [oracle_seq_kv8(O, x, p, n, Hq, Hkv, qn, kn) for x, (p, n) in zip(xs, spec["seqs"])]
        for a in xs + [qn, kn] + [t for r in res for t in r]:
            a.setflags(write=False)
        _ORACLE_KV8[key] = (xs, qn, kn, res)
    return _ORACLE_KV8[key]


# ---- whole engines against the oracle (tests/test_kv_q8_gpu.py, tests/test_shapes_gpu.py): the inputs, made by the oracle alone ------------------
def spk(d):
    return ((np.arange(d) % 13 - 6) * 0.03125).astype(np.float32)


def prompt_rows(O, om, rows, seed):
    """The last `rows` rows of a prompt the oracle builds from `rows` random text ids (a prompt has about ten rows more than its text)."""
    desc, keep = O.make_prompt_desc(np.random.default_rng([seed, rows]).integers(0, 151643, size=rows), spk_emb=spk(om.cfg.d_embed))
    return np.ascontiguousarray(om.build_prompt(desc)[-rows:])


GREEDY = dict(temperature=0.0)
SAMPLED = dict(temperature=0.9, top_k=0, top_p=1.0)   # the whole distribution: the ids follow every logit, not the top few


def batch_requests(O, om, n, lo=40, hi=130, frames=(6, 12), seed=77):
    """n sampled requests of mixed prompt length (lo .. hi rows, both ends present) and forced lengths (frames[0] .. frames[1]): more than an
    engine's slots, so that slots are reused."""
    rng = np.random.default_rng(seed)
    rows = [lo, hi] + [int(r) for r in rng.integers(lo, hi + 1, size=n - 2)]
    reqs = []
    for i, r in enumerate(rows):
        t = int(rng.integers(frames[0], frames[1] + 1))
        reqs.append(dict(embd=prompt_rows(O, om, r, seed + i), seed=seed + i, max_steps=t + 2, min_frames=t, force_eos_at=t, **SAMPLED))
    return reqs


def oracle_kw(r):
    return {k: v for k, v in r.items() if k not in ("embd", "want_pcm", "desc", "prefix")}

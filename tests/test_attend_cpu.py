"""CPU half of the attention kernel tests (tests/_attend_ref.py, tests/test_attend_gpu.py): the oracle against the two-stage float64
reference on every case of the GPU file — where ATT_STAGE2_TOL is measured and the midpoint-exception share is checked —, the reference's
power to notice a wrong kernel (seven planted defects), and the host-only parts of the hooks: the launcher's rule through
q3tts_k_attend_pick and the hooks' refusals (the library loads without a device; no compute call is made)."""
import ctypes as C

import numpy as np
import pytest

import _attend_ref as A
from _oracle import ATT_STAGE2_MEASURED, ATT_STAGE2_TOL


def test_bound_is_twice_the_measured_value():
    assert set(ATT_STAGE2_MEASURED) == set(A.KINDS)
    assert ATT_STAGE2_TOL == pytest.approx(2.0 * max(ATT_STAGE2_MEASURED.values()), rel=1e-6)
    assert ATT_STAGE2_TOL <= 2e-5


def test_rne_bf16_matches_the_bit_rule():
    """The float64 rounding helper against the integer rule on f32 values (ties included), and the midpoint window."""
    rng = np.random.default_rng(1)
    x = np.concatenate([rng.standard_normal(4096).astype(np.float32), A.bf16_value(np.arange(0x3F00, 0x4100, dtype=np.uint16)),
                        (A.bits(A.bf16_value(np.arange(0x3F00, 0x4000, dtype=np.uint16))) | 0x8000).view(np.float32), np.zeros(1, np.float32)])
    r = A.rne_bf16(x.astype(np.float64))
    assert np.array_equal(A.bf16_bits(r.astype(np.float32)), A.bf16_bits(x)) and np.array_equal(A.bits(r), A.bits(A.bf16_value(A.bf16_bits(x))))
    lo, hi, near = A.bf16_window(x.astype(np.float64))
    ties = (A.bits(x) & 0xFFFF) == 0x8000
    assert near[ties].all() and not near[(A.bits(x) & 0xFFFF) == 0].any() and (lo <= r).all() and (r <= hi).all()
    m = 1.0 + 2.0 ** -8                                      # the midpoint between 1 and 1 + 2^-7
    xs = np.array([m * (1 + 2.0 ** -21), m * (1 - 2.0 ** -21), m * (1 + 2.0 ** -19), m * (1 - 2.0 ** -19)])
    lo, hi, near = A.bf16_window(xs)
    assert near.tolist() == [True, True, False, False]
    assert lo.tolist() == [1.0, 1.0, 1.0 + 2.0 ** -7, 1.0] and hi.tolist() == [1.0 + 2.0 ** -7, 1.0 + 2.0 ** -7, 1.0 + 2.0 ** -7, 1.0]
    lo, hi, near = A.bf16_window(xs[2:], np.array([8.0, 1.0]))   # relative to a magnitude of 8: the first is inside the window again
    assert near.tolist() == [True, False]


def test_oracle_against_the_two_stage_reference(oracle):
    """Every (spec, kind) of the GPU file through the oracle alone: stage 1 holds for its cache with the exception share under the cap, and
    its worst stage-2 error — per input kind — is what tests/_oracle.py records (ATT_STAGE2_TOL is twice the largest)."""
    worst = {k: 0.0 for k in A.KINDS}
    by_spec = {}
    elems = near = flipped = 0
    strict = []
    worst_share = 0.0
    for spec in A.SPECS:
        Hq, Hkv = spec["heads"]
        for kind in A.KINDS:
            xs, qn, kn, res = A.oracle_case(oracle, spec, kind)
            ce = cn = 0
            for x, (pos0, n), (out, q, kb, vb) in zip(xs, spec["seqs"], res):
                e, nr, fl = A.check_stage1(x, Hq, Hkv, kn, kb, vb, strict)
                ce += e; cn += nr; flipped += fl
                err = A.stage2_error(out, q[pos0:], kb, vb, pos0, Hq, Hkv)
                worst[kind] = max(worst[kind], err)
                if kind in ("first", "newest") and pos0 + n > 1:   # the construction works: the dominant key carries the last row's output
                    t = 0 if kind == "first" else pos0 + n - 1
                    vt = np.repeat(A.bf16_value(vb[t]).astype(np.float64), Hq // Hkv, axis=0).reshape(-1)
                    assert np.abs(out[-1] - vt).max() <= 1e-3 * np.abs(vt).max(), (spec["name"], kind, pos0, n)
                by_spec[spec["name"]] = max(by_spec.get(spec["name"], 0.0), err)
            elems += ce; near += cn
            if ce >= 100000:     # a share needs a population: the expected one is ~5e-4
                worst_share = max(worst_share, cn / ce)
    share = near / elems
    print("oracle vs float64, stage 2, worst error / max|V| per kind: " + ", ".join(f"{k} {v:.2e}" for k, v in worst.items())
          + f" (bound {ATT_STAGE2_TOL:.1e})")
    print("  per spec: " + ", ".join(f"{k} {v:.1e}" for k, v in by_spec.items()))
    print(f"stage 1: {elems} cached K elements, {near} within 2^-20 of a bf16 midpoint (share {share:.2e}, worst case of >= 1e5 elements "
          f"{worst_share:.2e}, cap {A.STAGE1_SHARE_CAP:.0e}), {flipped} of them cached as the other neighbour "
          f"({sum(strict)} of those lie outside a window relative to the element alone: RoPE cancellation)")
    assert share <= A.STAGE1_SHARE_CAP and worst_share <= A.STAGE1_SHARE_CAP
    for k, v in worst.items():
        assert v <= ATT_STAGE2_MEASURED[k] * 1.01, (k, v, ATT_STAGE2_MEASURED[k])
    assert max(worst.values()) <= ATT_STAGE2_TOL


@pytest.mark.parametrize("defect", sorted(A.DEFECTS))
def test_reference_notices_a_planted_defect(oracle, defect):
    """One defect at a time in the float64 reference: on its specs the clean reference stays next to the oracle (5e-2: single-stage, so
    a key element cached as the other bf16 neighbour moves a score of the `wide` kind by 4 * 4 * 2^-8 / sqrt(128) = 5.5e-3) while the defect moves at least one case by >= 10 x ATT_STAGE2_TOL, relative to max |V|."""
    moved = 0.0
    for name in A.DEFECTS[defect]:
        spec = A.SPEC[name]
        Hq, Hkv = spec["heads"]
        for kind in A.KINDS:
            xs, qn, kn, res = A.oracle_case(oracle, spec, kind)
            for x, (pos0, n), (out, q, kb, vb) in zip(xs, spec["seqs"], res):
                vm = A.vmax_per_head(vb, Hq, Hkv)
                clean = A.full64(x, pos0, n, Hq, Hkv, qn, kn)
                assert (np.abs(clean - out) / vm).max() <= 5e-2, (name, kind, pos0, n)
                moved = max(moved, float((np.abs(A.full64(x, pos0, n, Hq, Hkv, qn, kn, defect) - clean) / vm).max()))
    print(f"defect {defect}: moves the reference by {moved:.2e} of max|V| (needed: {10 * ATT_STAGE2_TOL:.1e})")
    assert moved >= 10 * ATT_STAGE2_TOL


# ---- host-only: the launcher's rule and the hooks' refusals ---------------------------------------------------------------------------
@pytest.fixture()
def policies():
    from q3tts import _abi
    lib = _abi.load_library()

    def set_(decode, prefill):
        assert lib.q3tts_k_attend_policy(decode, prefill) == 0
    yield set_
    lib.q3tts_k_attend_policy(0, 0)


def test_attend_pick_follows_the_launchers_rule(policies):
    from q3tts.native import k_attend_pick as pick
    N1, N2, N4, F2, F4 = "k_attend<1, false>", "k_attend<2, false>", "k_attend<4, false>", "k_attend<2, true>", "k_attend<4, true>"
    for dec in (0, 1):
        for pre in (0, 1, 2):
            policies(dec, pre)
            # refusals: a ratio outside {1, 2, 4}, a fused launch with one head per KV head, the pair kernel for another ratio than 2
            assert pick(0, 3, 128, 2) is None and pick(1, 1, 128, 2) is None and pick(2, 1, 64, 2) is None and pick(2, 4, 64, 2) is None
            assert pick(2, 2, 64, 2) == pick(2, 2, 4096, 8) == "k_attend_pair"
            # fused, two heads per KV head: short caches first, then the decode policy
            assert pick(1, 2, 64, 2) == "k_attend_small<2>"
            assert pick(1, 2, 128, 2) == pick(1, 2, 8192, 8) == ("k_attend_gqa2", F2)[dec]
            assert pick(1, 4, 64, 1) == pick(1, 4, 128, 1) == F4
            # not fused: whole runs from LDS for two heads per KV head, n <= 128, pos0 + n <= 256, and enough workgroups (or policy 2)
            assert pick(0, 1, 128, 2, 200, 8, 8) == N1 and pick(0, 4, 128, 1, 200, 8, 8) == N4 and pick(0, 2, 128, 2) == N2
            many, few = "k_attend_prefill" if pre != 1 else N2, "k_attend_prefill" if pre == 2 else N2
            assert pick(0, 2, 256, 2, 64, 128, 256) == many and pick(0, 2, 256, 8, 16, 128, 256) == many
            assert pick(0, 2, 256, 2, 63, 128, 256) == few and pick(0, 2, 256, 2, 1, 1, 1) == few
            assert pick(0, 2, 320, 2, 64, 129, 129) == N2 and pick(0, 2, 320, 2, 64, 100, 257) == N2
    from q3tts import _abi
    lib = _abi.load_library()
    k = C.c_int32(0)
    for bad in ((3, 2, 64, 0, 0, 0, 2), (-1, 2, 64, 0, 0, 0, 2), (1, 0, 64, 0, 0, 0, 2), (1, 2, 0, 0, 0, 0, 2), (1, 2, 64, -1, 0, 0, 2), (1, 2, 64, 0, 0, 0, 0)):
        assert lib.q3tts_k_attend_pick(*bad, C.byref(k)) == -1, bad
    assert lib.q3tts_k_attend_pick(1, 2, 64, 0, 0, 0, 2, None) == -1


def test_every_case_names_its_kernel_and_all_nine_are_covered(policies):
    """The pick hook on every variant of every spec of the GPU file, under the variant's policy: the kernel the case is meant for — and
    over the whole file all nine kernels of csrc/q3_attend.hip."""
    from q3tts import native
    seen = set()
    for spec in A.SPECS:
        for v in spec["variants"]:
            policies(v["decode"] or 0, v["prefill"] or 0)
            got = native.k_attend_pick(**A.pick_args(spec, v))
            assert got == v["kernel"], (spec["name"], v, got)
            seen.add(got)
    assert seen == set(native.ATTEND_KERNELS)


def _expect_invalid(fn, *a, **kw):
    from q3tts import _abi
    with pytest.raises(_abi.Q3Error, match=r"failed \(-1\)"):
        fn(*a, **kw)


def test_hooks_refuse_bad_arguments_on_the_host():
    """Every refusal comes back as Q3TTS_ERR_INVALID before the device is touched (this machine needs none)."""
    from q3tts import native
    w = np.ones(A.HD, dtype=np.float32)
    tail = (w, w, A.EPS, A.THETA, A.SECTIONS)

    def rows(n, Hq=4, Hkv=2, hd=A.HD):
        return np.zeros((n, (Hq + 2 * Hkv) * hd), dtype=np.float32)
    runs, dec, pair = native.k_attention_runs, native.k_attention_decode_ex, native.k_attention_pair
    _expect_invalid(runs, rows(5), [(0, 5)], 100, 4, 2, A.HD, *tail)                 # n_ctx % 64
    _expect_invalid(runs, rows(5), [(0, 5)], 0, 4, 2, A.HD, *tail)
    _expect_invalid(runs, rows(65), [(0, 65)], 64, 4, 2, A.HD, *tail)                # pos0 + n > n_ctx
    _expect_invalid(runs, rows(65), [(60, 5)], 64, 4, 2, A.HD, *tail)
    _expect_invalid(runs, rows(5), [(5, 0)], 64, 4, 2, A.HD, *tail)                  # an empty run
    _expect_invalid(runs, rows(5), [(0, 5)], 64, 6, 2, A.HD, *tail)                  # GQA ratio 3
    _expect_invalid(runs, rows(5, 5, 2), [(0, 5)], 64, 5, 2, A.HD, *tail)            # Hq % Hkv
    _expect_invalid(runs, rows(5, hd=64), [(0, 5)], 64, 4, 2, 64, *tail)             # head_dim
    _expect_invalid(runs, rows(5), [(0, 5)], 64, 4, 2, A.HD, *tail, policy=3)
    _expect_invalid(runs, rows(5), [(0, 5)], 64, 4, 2, A.HD, *tail, out_form=3)
    _expect_invalid(runs, rows(0), [], 64, 4, 2, A.HD, *tail)                        # no run
    _expect_invalid(dec, rows(3), [3], 100, 4, 2, A.HD, *tail)
    _expect_invalid(dec, rows(65), [65], 64, 4, 2, A.HD, *tail)                      # a length above n_ctx
    _expect_invalid(dec, rows(0), [0], 64, 4, 2, A.HD, *tail)
    _expect_invalid(dec, rows(3, 2, 2), [3], 64, 2, 2, A.HD, *tail)                  # fused needs two heads per KV head
    _expect_invalid(dec, rows(3), [3], 64, 4, 2, A.HD, *tail, policy=2)
    _expect_invalid(dec, rows(5), [2, 3], 64, 4, 2, A.HD, *tail, row_indexed=True)   # row-indexed: equal lengths
    _expect_invalid(dec, rows(3), [3], 64, 4, 2, A.HD, *tail, out_form=-1)
    _expect_invalid(pair, rows(2, 4, 1), 1, 64, 4, 1, A.HD, *tail)                   # the pair kernel: ratio 2 only
    _expect_invalid(pair, rows(2), 1, 96, 4, 2, A.HD, *tail)
    _expect_invalid(pair, rows(0), 0, 64, 4, 2, A.HD, *tail)
    from q3tts import _abi
    lib = _abi.load_library()
    x = rows(2)
    out = np.zeros((2, 4 * A.HD), dtype=np.int8)
    # Q8_0 output without a place for the scales; a null output
    assert lib.q3tts_k_attention_pair(0, x.ctypes.data_as(C.POINTER(C.c_float)), 1, 64, 4, 2, A.HD, w.ctypes.data_as(C.POINTER(C.c_float)),
                                      w.ctypes.data_as(C.POINTER(C.c_float)), A.EPS, A.THETA, None, 2, out.ctypes.data, None, None, None) == -1
    assert lib.q3tts_k_attention_pair(0, x.ctypes.data_as(C.POINTER(C.c_float)), 1, 64, 4, 2, A.HD, w.ctypes.data_as(C.POINTER(C.c_float)),
                                      w.ctypes.data_as(C.POINTER(C.c_float)), A.EPS, A.THETA, None, 0, None, None, None, None) == -1

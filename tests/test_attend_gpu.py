"""The nine attention kernels of csrc/q3_attend.hip one launch at a time, through q3tts_k_attention_decode_ex / _runs / _pair: the cases of
tests/_attend_ref.py (Predictor decode on short caches with both addressings, pass A, whole prompt runs with and without a voice prefix,
the Talker's decode kernels on the same slots, the GQA ratios 1 and 4) on seven input kinds. Every case asserts the same six things:
  1. the f32 output equals the oracle bit for bit;
  2. the bf16 operand equals bf16(f32 output);
  3. the Q8_0 blocks equal q3o_quantize_q8_0_act of the f32 output, quants and scales, bit for bit;
  4. the cache the launch leaves equals the oracle's preparation stage (and is untouched past each sequence's end);
  5. stage 1 and stage 2 of the float64 reference hold for the device's cache and output (ATT_STAGE2_TOL: measured on the CPU oracle,
     tests/_oracle.py);
  6. q3tts_k_attend_pick names the kernel the case is meant for.
tests/test_attend_cpu.py runs the same cases through the oracle alone, shows what the reference notices, and checks that the cases cover
all nine kernels."""
import numpy as np
import pytest

import _attend_ref as A
from _oracle import ATT_STAGE2_TOL

pytestmark = pytest.mark.gpu


def _pick(native, spec, v):
    from q3tts import _abi
    lib = _abi.load_library()
    assert lib.q3tts_k_attend_policy(v["decode"] or 0, v["prefill"] or 0) == 0
    try:
        return native.k_attend_pick(**A.pick_args(spec, v))
    finally:
        lib.q3tts_k_attend_policy(0, 0)


def _launch(native, spec, v, xs, qn, kn, form):
    Hq, Hkv = spec["heads"]
    rows = A.hook_rows(spec, xs)
    tail = (v["n_ctx"], Hq, Hkv, A.HD, qn, kn, A.EPS, A.THETA, A.SECTIONS)
    if spec["hook"] == "decode":
        return native.k_attention_decode_ex(rows, [p + n for p, n in spec["seqs"]], *tail, policy=-1 if v["decode"] is None else v["decode"],
                                            row_indexed=bool(spec.get("row_indexed")), out_form=form)
    if spec["hook"] == "pair":
        return native.k_attention_pair(rows, len(xs), *tail, out_form=form)
    return native.k_attention_runs(rows, spec["seqs"], *tail, policy=-1 if v["prefill"] is None else v["prefill"], out_form=form)


def _check_case(oracle, native, spec, kind, worst):
    Hq, Hkv = spec["heads"]
    xs, qn, kn, res = A.oracle_case(oracle, spec, kind)
    first = None
    for v in spec["variants"]:
        what = (spec["name"], kind, v["kernel"])
        assert _pick(native, spec, v) == v["kernel"], what                                                     # 6
        r0 = _launch(native, spec, v, xs, qn, kn, 0)
        r1 = _launch(native, spec, v, xs, qn, kn, 1)
        r2 = _launch(native, spec, v, xs, qn, kn, 2)
        assert np.array_equal(r1["out"], A.bf16_bits(r0["out"])), what                                         # 2
        q8, d8 = oracle.quantize_q8_0_act(r0["out"])
        assert np.array_equal(r2["out"], q8) and np.array_equal(A.bits(r2["scale"]), A.bits(d8)), what         # 3
        if kind == "zero_block":   # amax = 0: d = 0 and every quant 0, in every head's block ZERO_BLOCK
            blk = np.arange(Hq) * (A.HD // 32) + A.ZERO_BLOCK
            assert not r2["scale"][:, blk].any() and not r2["out"].reshape(-1, Hq * A.HD // 32, 32)[:, blk].any(), what
        for r in (r1, r2):
            assert np.array_equal(r["k_cache"], r0["k_cache"]) and np.array_equal(r["v_cache"], r0["v_cache"]), what
        err = 0.0
        for i, (x, (pos0, n), (out, q, kb, vb), dev) in enumerate(zip(xs, spec["seqs"], res, A.hook_out_split(spec, r0["out"]))):
            tot = pos0 + n
            assert np.array_equal(A.bits(dev), A.bits(out)), what + (i, pos0, n)                               # 1
            dk, dv = r0["k_cache"][i].transpose(1, 0, 2), r0["v_cache"][i].transpose(1, 0, 2)                  # [position][Hkv][HD]
            assert np.array_equal(dk[:tot], kb) and np.array_equal(dv[:tot], vb), what + (i, pos0, n)          # 4
            assert not dk[tot:].any() and not dv[tot:].any(), what + (i, pos0, n)
            A.check_stage1(x, Hq, Hkv, kn, dk[:tot], dv[:tot])                                                 # 5
            err = max(err, A.stage2_error(dev, q[pos0:], dk[:tot], dv[:tot], pos0, Hq, Hkv))
        assert err <= ATT_STAGE2_TOL, what + (err,)
        worst[(v["kernel"], kind)] = max(worst.get((v["kernel"], kind), 0.0), err)
        if first is None:
            first = r0["out"]
        else:   # another kernel, the same answer
            assert np.array_equal(A.bits(r0["out"]), A.bits(first)), what


@pytest.mark.parametrize("name", [s["name"] for s in A.SPECS])
def test_attention_kernel_case(oracle, name):
    """One spec of tests/_attend_ref.py on every input kind through every variant (kernel) it names: the six assertions of the module
    docstring, and all variants give the same f32 bits.
      decode13: slots of 1 .. 64 keys in one launch — k_attend_small<2> at n_ctx 64 (the value-pass branch for cached keys t >= 16 that are
        not the newest runs from 18 keys on; +-300 value rows at 15 / 16 and at the newest key), k_attend_gqa2 and k_attend<2, true> at 128;
      rowidx*: k_attend_small<2> with the Predictor's row-indexed addressing; decode_r4: k_attend<4, true>;
      pair*: k_attend_pair on 1, 2, 5, 64 slots, +-300 rows at position 0 or 1;
      prefill_a / prefill_b: k_attend_prefill with seg_max_t <= 128 / = 256 (pos0 > 0: a prefix of 1 .. 255 rows) against k_attend<2, false>;
      runs_129, runs_200_100: runs the prefill kernel is not eligible for, under policy 2; runs_r1 / runs_r4: k_attend<1 / 4, false>."""
    from q3tts import native
    spec = A.SPEC[name]
    worst = {}
    for kind in A.KINDS:
        _check_case(oracle, native, spec, kind, worst)
    for kernel in dict.fromkeys(v["kernel"] for v in spec["variants"]):
        print(f"{name} {kernel}: worst error vs float64 / max|V|: " + ", ".join(f"{k} {worst[(kernel, k)]:.1e}" for k in A.KINDS)
              + f" (bound {ATT_STAGE2_TOL:.1e})")


@pytest.mark.parametrize("b", [1, 2, 5, 64])
def test_pair_equals_the_decode_hook_row_by_row(oracle, b):
    """k_attend_pair's two rows per slot against the same rows fed one at a time through the fused decode launch (k_attend_small<2>: first
    row b on an empty cache, then row n_slots + b on the cache that holds row b): the same f32 bits, and the same cache for positions 0 and
    1 — the Predictor's later passes read what the pair kernel appended."""
    from q3tts import native
    spec = A.SPEC["pair%d" % b]
    Hq, Hkv = spec["heads"]
    for kind in A.KINDS:
        xs, qn, kn, _ = A.oracle_case(oracle, spec, kind)
        tail = (64, Hq, Hkv, A.HD, qn, kn, A.EPS, A.THETA, A.SECTIONS)
        pair = native.k_attention_pair(A.hook_rows(spec, xs), b, *tail)
        one = native.k_attention_decode_ex(np.stack([x[0] for x in xs]), [1] * b, *tail, row_indexed=True)
        two = native.k_attention_decode_ex(np.concatenate(xs), [2] * b, *tail, row_indexed=True)
        assert np.array_equal(A.bits(pair["out"][:b]), A.bits(one["out"])), kind
        assert np.array_equal(A.bits(pair["out"][b:]), A.bits(two["out"])), kind
        assert np.array_equal(pair["k_cache"], two["k_cache"]) and np.array_equal(pair["v_cache"], two["v_cache"]), kind
        assert np.array_equal(pair["k_cache"][:, :, :1], one["k_cache"][:, :, :1]), kind


def test_the_cases_cover_all_nine_kernels():
    """The kernels q3tts_k_attend_pick names over every variant of every spec of this file, under the variant's policy: each is the one the
    case is meant for, and together they are all nine kernels of csrc/q3_attend.hip."""
    from q3tts import native
    seen = set()
    for spec in A.SPECS:
        for v in spec["variants"]:
            got = _pick(native, spec, v)
            assert got == v["kernel"], (spec["name"], v, got)
            seen.add(got)
    assert seen == set(native.ATTEND_KERNELS) and len(seen) == 9

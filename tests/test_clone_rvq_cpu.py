"""q3o_rvq (oracle/q3_oracle_clone.c), the quantiser lifted out of q3o_audio_encode, to the expectations tests/test_clone_rvq_gpu.py holds the
kernel to: float64 along its own picks on random operands, the smaller index on constructed exact ties. CPU only."""
import numpy as np
import pytest

import _rvq_ref as R


@pytest.mark.parametrize("T", R.RANDOM_T)
@pytest.mark.parametrize("CS,D,ncb", R.RANDOM_SIZES)
def test_oracle_rvq_random_operands_against_float64(oracle, CS, D, ncb, T):
    ps, pa, books = R.random_case(CS, D, ncb, T)
    codes = oracle.rvq(ps, pa, books)
    assert codes.shape == (T, ncb)
    assert 1.0 <= R.judge(ps, pa, books, codes) <= R.bound(D)


def test_oracle_rvq_constructed_cases(oracle):
    cases = [R.tie_case(at) for at in R.TIE_PAIRS] + [R.tie_case((i,)) for i in R.TIE_ALONE] + [R.identical_case(), R.zero_residual_case()]
    cases += [R.size_case(CS) for CS in R.SIZES_CS]
    for ps, pa, books, want in cases:
        codes = oracle.rvq(ps, pa, books)
        assert np.array_equal(codes, want), (codes, want)
        R.judge(ps, pa, books, codes)


def test_judge_refuses_a_second_nearest_pick(oracle):
    """the float64 judgement is not vacuous: the runner-up of a constructed case (4x the distance) and an index one off on random operands fail it"""
    ps, pa, books, want = R.tie_case((1024,))
    bad = want.copy(); bad[0, 2] = 0   # the runner-up sits at index 1024 - 1024
    with pytest.raises(AssertionError):
        R.judge(ps, pa, books, bad)
    ps, pa, books = R.random_case(1000, 48, 3, 1)
    codes = oracle.rvq(ps, pa, books)
    codes[0, 1] = (codes[0, 1] + 1) % 1000
    with pytest.raises(AssertionError):
        R.judge(ps, pa, books, codes)


def test_audio_encode_still_calls_the_same_quantiser(oracle):
    """q3o_audio_encode's ids are q3o_rvq's on its own projections: the lift changed no id (the golden ids of the tiny config stand in
    tests/test_clone_family_cpu.py); here the entry is driven with pa = None for one codebook and refuses a missing pa for two."""
    ps, pa, books = R.random_case(63, 16, 2, 5)
    one = oracle.rvq(ps, None, books[:1])
    assert np.array_equal(one[:, 0], oracle.rvq(ps, pa, books)[:, 0])
    import ctypes as C
    L = oracle.lib()
    codes = np.zeros((5, 2), dtype=np.int32)
    assert L.q3o_rvq(oracle.ptr(ps, oracle.f32p), None, 5, 16, oracle.ptr(books, oracle.f32p), 2, 63, oracle.ptr(codes, oracle.i32p)) < 0

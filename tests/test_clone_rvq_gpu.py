"""k_cb_transpose + k_rvq (q3_clone.hip) through q3tts_k_rvq: the clone audio encoder's quantiser on its own, against q3o_rvq and float64.

The encoders' end-to-end tests reach the quantiser only with seeded random codebooks of 64 or 2048 codewords, which never tie. Here:
random operands at the codebook sizes of tests/_clone_shapes.py (ids equal to the oracle's, every pick within the f32 rounding bound of the
float64 minimum, _rvq_ref.judge), and constructed operands whose distances are exact in f32, so that every tie rule of the kernel — within a
lane, across the trips of the j0 loop, across lanes and waves in the tree — has one expected answer: the smaller index. tests/test_clone_rvq_cpu.py
holds the oracle entry to the same expectations. Non-finite operands are not run: DESIGN.md §14 states where kernel and oracle differ on them.
"""
import numpy as np
import pytest

import _rvq_ref as R

pytestmark = pytest.mark.gpu


def _device(ps, pa, books):
    from q3tts import native
    codes = native.k_rvq(ps, pa, books)
    assert codes.dtype == np.int64 and codes.shape == (ps.shape[0], books.shape[0])
    return codes


@pytest.mark.parametrize("T", R.RANDOM_T)
@pytest.mark.parametrize("CS,D,ncb", R.RANDOM_SIZES)
def test_rvq_random_operands_equal_oracle_and_float64(oracle, CS, D, ncb, T):
    ps, pa, books = R.random_case(CS, D, ncb, T)
    codes = _device(ps, pa, books)
    assert np.array_equal(codes, oracle.rvq(ps, pa, books).astype(np.int64))
    worst = R.judge(ps, pa, books, codes)
    print("CS %d D %d ncb %d T %d: worst picked / float64 minimum = 1 + %.3g (bound 1 + %.3g)" % (CS, D, ncb, T, worst - 1.0, R.bound(D) - 1.0))


@pytest.mark.parametrize("at", R.TIE_PAIRS + tuple((i,) for i in R.TIE_ALONE), ids=lambda at: "-".join(map(str, at)))
def test_rvq_constructed_ties_take_the_smaller_index(oracle, at):
    ps, pa, books, want = R.tie_case(at)
    codes = _device(ps, pa, books)
    assert np.array_equal(codes, want), (codes, want)
    assert np.array_equal(codes, oracle.rvq(ps, pa, books).astype(np.int64))
    assert R.judge(ps, pa, books, codes) == 1.0


def test_rvq_identical_codewords_give_zero(oracle):
    ps, pa, books, want = R.identical_case()
    codes = _device(ps, pa, books)
    assert np.array_equal(codes, want) and np.array_equal(codes, oracle.rvq(ps, pa, books).astype(np.int64))


def test_rvq_zero_residual_picks_the_codeword_nearest_the_origin(oracle):
    ps, pa, books, want = R.zero_residual_case()
    codes = _device(ps, pa, books)
    assert np.array_equal(codes, want), (codes, want)
    assert np.array_equal(codes, oracle.rvq(ps, pa, books).astype(np.int64))
    assert R.judge(ps, pa, books, codes) == 1.0


@pytest.mark.parametrize("CS", R.SIZES_CS)
def test_rvq_last_codeword_at_sizes_around_the_workgroup(oracle, CS):
    ps, pa, books, want = R.size_case(CS)
    assert (want == CS - 1).all()
    codes = _device(ps, pa, books)
    assert np.array_equal(codes, want), (codes, want)
    assert np.array_equal(codes, oracle.rvq(ps, pa, books).astype(np.int64))


def test_rvq_hook_refuses_bad_shapes(oracle):
    from q3tts import _abi, native
    ps, pa, books = R.random_case(63, 16, 2, 1)
    with pytest.raises(_abi.Q3Error, match="rvq hook: bad shape"):
        native.k_rvq(ps, None, books)                                   # two codebooks need pa
    with pytest.raises(_abi.Q3Error, match="rvq hook: bad shape"):
        native.k_rvq(np.zeros((1, 24), np.float32), np.zeros((1, 24), np.float32), np.zeros((2, 8, 24), np.float32))   # D % 16
    assert native.k_rvq(ps, None, books[:1]).shape == (1, 1)            # one codebook: pa is never read

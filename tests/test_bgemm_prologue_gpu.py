"""The decoder's GEMM (csrc/q3_bgemm.hip) at the small shapes where its prologue can go wrong, bit for bit against the oracle.

Every (row tiles, column tiles) instance of k_bgemm is forced in turn (q3tts_k_bgemm_force) and run through the GEMM hook of
tests/test_parity_gpu.py with each epilogue the decode path launches — STORE with row scales, RESID with nw_next, SWIGLU, ARGMAX keys and
STORE without row scales (ssp = null): the five epilogues that are compiled into k_bgemm_epi — at
  rows 1, 15, 16, 17, 33, 64: the clamped min(.., B - 1) rows, a partial last row tile, rows wave + 8 i past B in the partials' reduction;
  K 256, 512, 2048: at 256 a K slice is one step, so every ring slot behind step 0 is the clamped re-read;
  N 16 NT, 48 NT, 2048: one column group, three (no XCD remap), 128 tiles (remap whenever the rows make more than one chunk);
  16, 64, 128 tiles of sums of squares per row; operand rows that start at row 0 or at row 64 of their buffer (Q3BGemm.a_row0).
An epilogue runs at the N it can take: RESID's bf16 output needs N % 32 == 0, SWIGLU N % 64 == 0; 2048 has no whole number of three-tile
column groups, so the NT = 3 instances take 2112 (132 tiles) in its place. Once at 65 rows the launcher's own choice for many rows runs.
The comparison is == on raw bits: a row's result never depends on the tile instance, the row count or where the rows start."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROWS = (1, 15, 16, 17, 33, 64)
KS = (256, 512, 2048)
NTILES = (16, 64, 128)
A_ROW0 = (0, 64)
EPIS = ("store", "resid_nw", "swiglu", "argmax", "store_raw")   # store_raw: STORE from ssp = null
EPI_CODE = {"store": 0, "resid_nw": 1, "swiglu": 2, "argmax": 3, "store_raw": 0}
EK = {"store": 0 | 8, "resid_nw": 1 | 16, "swiglu": 2 | 8, "argmax": 3 | 8, "store_raw": 0}   # the epilogue compiled into k_bgemm_epi
INSTANCES = [(rt, nt) for rt in (1, 2, 3, 4) for nt in (1, 2, 3)]
RING_DEPTH = {2: 8, 3: 8, 4: 5, 5: 4, 6: 3, 7: 2}   # by RT + NT (BgInst::D)


def _n_ok(epi, N):
    return N % 64 == 0 if epi == "swiglu" else (N % 32 == 0 if epi == "resid_nw" else True)


def _cases():
    """Per instance every epilogue at every N it can take; rows, K, tiles per row and a_row0 rotate with the case index, at a different pace
    each, so every instance sees every value of each."""
    out = []
    for inst, (rt, nt) in enumerate(INSTANCES):
        n = 0
        for N in (16 * nt, 48 * nt, 2112 if nt == 3 else 2048):
            for epi in EPIS:
                if not _n_ok(epi, N):
                    continue
                i = n + inst
                out.append((rt, nt, ROWS[i % 6], KS[(i // 2) % 3], N, NTILES[(i // 3) % 3], A_ROW0[(n // 2 + inst) % 2], epi))
                n += 1
    return out


CASES = _cases()


def test_case_list_covers_what_it_says():
    for rt, nt in INSTANCES:
        mine = [c for c in CASES if c[:2] == (rt, nt)]
        assert {c[2] for c in mine} == set(ROWS) and {c[3] for c in mine} == set(KS) and {c[5] for c in mine} == set(NTILES)
        assert {c[6] for c in mine} == set(A_ROW0) and {c[7] for c in mine} == set(EPIS)
        assert {c[4] for c in mine} == {16 * nt, 48 * nt, 2112 if nt == 3 else 2048}


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _bf16_bits(a):
    u = np.ascontiguousarray(a, dtype=np.float32).view(np.uint32).astype(np.uint64)
    u = u + 0x7FFF + ((u >> 16) & 1)
    return (u >> 16).astype(np.uint16)


@pytest.fixture(scope="module")
def native():
    from q3tts import native
    return native


@pytest.fixture(scope="module")
def lib(native):
    return native._abi.load_library()


def _operands(B, K, N, ntiles, epi, seed):
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((B, K)) * 1.5).astype(np.float32); x[:, :7] *= 300.0; x[:, 100:140] *= 1e-3
    xb, wb = _bf16_bits(x), _bf16_bits((rng.standard_normal((N, K)) * 0.02).astype(np.float32))
    ssp = None if epi in ("resid_nw", "store_raw") else (np.abs(rng.standard_normal((B, ntiles)) * 4.0) + 0.5).astype(np.float32)
    nw_next = (1.0 + rng.standard_normal(N) * 0.05).astype(np.float32) if epi == "resid_nw" else None
    y0 = (rng.standard_normal((B, N)) * 2.0).astype(np.float32) if epi == "resid_nw" else None
    junk = _bf16_bits((rng.standard_normal((64, K)) * 50.0).astype(np.float32))   # the rows in front of the operand when a_row0 = 64
    return xb, wb, ssp, nw_next, y0, junk


def _assert_equal(epi, got, ref):
    if epi in ("store", "store_raw"):
        assert np.array_equal(_bits(got["y"]), _bits(ref["y"]))
    elif epi == "resid_nw":
        assert np.array_equal(_bits(got["y"]), _bits(ref["y"]))
        assert np.array_equal(got["yb"], ref["yb"])
        assert np.array_equal(_bits(got["ssp_out"]), _bits(ref["ssp_out"]))
    elif epi == "swiglu":
        assert np.array_equal(got["yb"], ref["yb"])
    else:
        assert np.array_equal(got["keys"], ref["keys"])


def _last(lib):
    o6 = (C.c_int32 * 6)()
    assert lib.q3tts_k_bgemm_last(o6) == 0
    return list(o6)


@pytest.mark.parametrize("rt,nt", INSTANCES)
def test_every_instance_at_the_prologue_edge_shapes(oracle, native, lib, rt, nt):
    assert lib.q3tts_k_bgemm_force(rt, nt) == 0
    try:
        for (_, _, B, K, N, ntiles, a_row0, epi) in [c for c in CASES if c[:2] == (rt, nt)]:
            xb, wb, ssp, nw_next, y0, junk = _operands(B, K, N, ntiles, epi, 7000 + 100 * rt + 10 * nt + B + K + N + ntiles + a_row0)
            d_norm = 16 * ntiles
            ref = oracle.bgemm(xb, wb, ssp, d_norm, 1e-6, EPI_CODE[epi], nw_next, y0)
            xin = np.concatenate([junk, xb]) if a_row0 else xb
            got = native.k_bgemm(xin, wb, ssp, d_norm, 1e-6, EPI_CODE[epi], nw_next, y0, a_row0=a_row0)
            what = (rt, nt, B, K, N, ntiles, a_row0, epi)
            assert _last(lib) == [rt, nt, RING_DEPTH[rt + nt], 0, 0, EK[epi]], what   # the forced instance with this epilogue compiled in ran
            try:
                _assert_equal(epi, got, ref)
            except AssertionError:
                raise AssertionError("k_bgemm differs from the oracle at (RT, NT, rows, K, N, tiles, a_row0, epilogue) = %r" % (what,))
    finally:
        assert lib.q3tts_k_bgemm_force(0, 0) == 0


@pytest.mark.parametrize("epi", EPIS)
def test_many_row_choice_at_65_rows(oracle, native, lib, epi):
    """65 rows: the launcher's own choice among the instances for more than 64 rows (five row chunks of RT = 1, three of 2, two of 3 or 4),
    the last chunk holding one live row."""
    B, K, N, ntiles = 65, 512, 2048, 64
    xb, wb, ssp, nw_next, y0, _ = _operands(B, K, N, ntiles, epi, 65)
    o5 = (C.c_int32 * 5)()
    assert lib.q3tts_k_bgemm_pick(B, K, N, EPI_CODE[epi], 0, 0, o5) == 0 and o5[4] == 0
    ref = oracle.bgemm(xb, wb, ssp, 16 * ntiles, 1e-6, EPI_CODE[epi], nw_next, y0)
    got = native.k_bgemm(xb, wb, ssp, 16 * ntiles, 1e-6, EPI_CODE[epi], nw_next, y0)
    assert _last(lib) == list(o5) + [EK[epi]]
    _assert_equal(epi, got, ref)


def test_the_picker_names_the_instance_that_is_launched(oracle, native, lib):
    """bench.py prints k_bgemm<RT, NT, D, NTW, false> from q3tts_k_bgemm_pick's answer: the launch that follows runs that tile instance —
    the Predictor's QKV shape at 64 rows (a decode epilogue: k_bgemm_epi of the same instance) and a launch whose epilogue stays a run-time
    choice (RESID without nw_next: k_bgemm itself)."""
    def symbol(o):
        return "k_bgemm_big" if o[4] else "k_bgemm<%d, %d, %d, %s, false>" % (o[0], o[1], o[2], "true" if o[3] else "false")
    B, K, N = 64, 1024, 4096
    xb, wb, ssp, _, _, _ = _operands(B, K, N, K // 16, "store", 1)
    o5 = (C.c_int32 * 5)()
    assert lib.q3tts_k_bgemm_pick(B, K, N, 0, 0, 0, o5) == 0
    got = native.k_bgemm(xb, wb, ssp, K, 1e-6, 0)
    last = _last(lib)
    assert symbol(last) == symbol(list(o5)) == "k_bgemm<2, 2, 5, false, false>" and last[5] == EK["store"]
    assert np.array_equal(_bits(got["y"]), _bits(oracle.bgemm(xb, wb, ssp, K, 1e-6, 0)["y"]))
    B, K, N = 33, 512, 96
    xb, wb, _, _, y0, _ = _operands(B, K, N, 16, "resid_nw", 2)
    assert lib.q3tts_k_bgemm_pick(B, K, N, 1, 0, 0, o5) == 0
    got = native.k_bgemm(xb, wb, None, K, 1e-6, 1, None, y0)
    last = _last(lib)
    assert symbol(last) == symbol(list(o5)) and last[5] == -1
    assert np.array_equal(_bits(got["y"]), _bits(oracle.bgemm(xb, wb, None, K, 1e-6, 1, None, y0)["y"]))

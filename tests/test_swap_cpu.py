"""Paced requests and swapping on the CPU (include/q3tts.h, "paced requests and swapping"): the new symbols, the request
struct's pinned layout, the null-session refusals, the credit rule against its one line of Python, and the swap arena's allocator
(first fit over 256-byte units, neighbours coalesced on free) through its host-only hook."""
import ctypes as C

import numpy as np
import pytest

INVALID = -1   # Q3TTS_ERR_INVALID
NEW = ["q3tts_session_submit_paced", "q3tts_session_grant", "q3tts_session_set_swap", "q3tts_session_swap_stats",
       "q3tts_k_credit_ready", "q3tts_k_swap_arena", "q3tts_k_swap_phase_ms"]


@pytest.fixture(scope="module")
def lib():
    from q3tts import _abi
    return _abi.load_library()


def test_symbols_and_request_layout(lib):
    from q3tts import _abi
    for s in NEW:
        assert s in _abi.SYMBOLS and hasattr(lib, s), s
    assert C.sizeof(_abi.Request) == 80 and _abi.Request.prefix.offset == 72   # everything new is a call


def test_null_session_is_refused(lib):
    from q3tts import _abi
    r, rid, out = _abi.Request(), C.c_uint64(0), (C.c_int64 * 6)()
    calls = [lambda: lib.q3tts_session_submit_paced(None, C.byref(r), 8, C.byref(rid)),
             lambda: lib.q3tts_session_grant(None, 1, 4),
             lambda: lib.q3tts_session_set_swap(None, 1 << 20),
             lambda: lib.q3tts_session_swap_stats(None, out),
             lambda: lib.q3tts_k_swap_phase_ms(None, (C.c_double * 3)())]
    for call in calls:
        lib.q3tts_session_next(None, 0, None)   # (leaves "null argument" behind, so the next message is the call's)
        assert b"null session" not in lib.q3tts_session_last_error(None)
        assert call() == INVALID
        assert b"null session" in lib.q3tts_session_last_error(None)


def test_credit_rule(lib):
    for credit in range(4, 13):
        for n in range(0, 13):
            assert lib.q3tts_k_credit_ready(credit, n) == int(n + 4 <= credit), (credit, n)
    assert lib.q3tts_k_credit_ready(-1, 10 ** 6) == 1   # a lifted limit


def _arena(lib, cap, ops):
    a = np.asarray(ops, dtype=np.int64)
    off = np.full(a.size, -7, dtype=np.int64)
    rc = lib.q3tts_k_swap_arena(cap, a.ctypes.data_as(C.POINTER(C.c_int64)), a.size, off.ctypes.data_as(C.POINTER(C.c_int64)))
    return rc, [int(x) for x in off]


def test_arena_first_fit_and_coalescing(lib):
    U = 256
    cap = 8 * U
    # fill with eight one-unit blocks (sizes that are no multiple of the unit round up), then nothing fits
    ops = [1, U, U - 1, 100, U, 17, U, U, 1]
    rc, off = _arena(lib, cap, ops)
    assert rc == 0 and off[:8] == [i * U for i in range(8)] and off[8] == -1
    assert all(o % U == 0 for o in off[:8])
    # free every other block: four holes of one unit. Two units fit nowhere; one unit takes the FIRST hole
    frees = [-(k + 1) for k in (1, 3, 5, 7)]
    rc, off = _arena(lib, cap, ops[:8] + frees + [2 * U, U])
    assert rc == 0 and off[8:12] == [U, 3 * U, 5 * U, 7 * U] and off[12] == -1 and off[13] == U
    # free block 2 as well: the holes at 1, 2, 3 coalesce (both neighbours) and three units fit at unit 1, only there
    rc, off = _arena(lib, cap, ops[:8] + frees + [-(2 + 1), 3 * U, 2 * U])
    assert rc == 0 and off[13] == U and off[14] == -1
    # a free whose right-hand neighbour only is free, then the left-hand one only
    rc, off = _arena(lib, cap, ops[:8] + [-(7 + 1), -(6 + 1), 2 * U, -(0 + 1), -(1 + 1), 2 * U])
    assert rc == 0 and off[10] == 6 * U and off[13] == 0
    # everything freed, in an order that merges on both sides: one block of cap again
    order = [0, 2, 4, 6, 1, 5, 3, 7]
    rc, off = _arena(lib, cap, ops[:8] + [-(k + 1) for k in order] + [cap, 1])
    assert rc == 0 and off[16] == 0 and off[17] == -1


def test_arena_edges(lib):
    rc, off = _arena(lib, 1000, [768, 1, -1, 769])   # cap is used in whole units: 3 of them
    assert rc == 0 and off == [0, -1, 0, -1]
    rc, off = _arena(lib, 0, [1])
    assert rc == 0 and off == [-1]
    for bad in ([0], [-1], [256, -1, -1], [256, -3], [2048, -1]):   # zero, nothing to free, freed twice, a later index, a failed allocation
        rc, _ = _arena(lib, 1024, bad)
        assert rc == INVALID, bad
    assert lib.q3tts_k_swap_arena(-1, None, 0, None) == INVALID

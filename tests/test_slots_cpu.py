"""The row-bucket rule of engines with up to 256 slots (q3tts_k_row_buckets: host only, no GPU)."""
import ctypes as C

import pytest

import _slots as SL


@pytest.fixture(scope="module")
def lib():
    from q3tts import _abi
    return _abi.load_library()


def _buckets(lib, nb, cap=32):
    out = (C.c_int32 * cap)()
    n = lib.q3tts_k_row_buckets(nb, out, cap)
    return n, [int(out[i]) for i in range(max(n, 0))]


def test_up_to_64_slots_the_buckets_are_what_they_were(lib):
    for nb in range(1, 65):
        n, got = _buckets(lib, nb)
        assert n == len(got) and got == SL.buckets_le64(nb), nb
    assert _buckets(lib, 64)[1] == [1, 2, 4, 8, 16, 32, 48, 64]


def test_above_64_slots_multiples_of_32_then_the_slot_count(lib):
    for nb in range(65, 257):
        n, got = _buckets(lib, nb)
        assert n == len(got) and got[-1] == nb, nb
        assert all(a < b for a, b in zip(got, got[1:])), nb
        assert got[:8] == [1, 2, 4, 8, 16, 32, 48, 64], nb
        assert all(r % 32 == 0 for r in got[:-1] if r > 64), nb
        # every multiple of 32 between 64 and the slot count is there: a draining batch never pays for more than 31 idle rows above 64
        assert [r for r in got if r > 64][:-1] == [r for r in range(96, nb, 32)], nb
    assert _buckets(lib, 256)[1] == [1, 2, 4, 8, 16, 32, 48, 64, 96, 128, 160, 192, 224, 256]
    assert _buckets(lib, 200)[1] == [1, 2, 4, 8, 16, 32, 48, 64, 96, 128, 160, 192, 200]


def test_refusals(lib):
    assert _buckets(lib, 0)[0] == -1 and _buckets(lib, 257)[0] == -1 and _buckets(lib, -3)[0] == -1
    assert _buckets(lib, 256, cap=13)[0] == -1    # 14 buckets do not fit
    assert lib.q3tts_k_row_buckets(8, None, 32) == -1


def test_python_wrapper_and_api_parameter():
    from q3tts import _abi, native
    assert native.row_buckets(96) == [1, 2, 4, 8, 16, 32, 48, 64, 96]
    with pytest.raises(_abi.Q3Error):
        native.row_buckets(257)
    import inspect
    from q3tts import api
    assert "max_batch" in inspect.signature(api.TtsEngine.new).parameters

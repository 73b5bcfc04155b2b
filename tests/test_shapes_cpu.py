"""Model shapes without a device: q3tts_engine_create refuses, before it looks for a device, every shape the kernels of
tests/test_shapes_gpu.py do not cover, and its message names the field — the shape comes from a user's model files. The admitted ones (GQA
ratios 1, 2, 4 in either transformer, 2 .. 16 codebooks) run against the oracle in tests/test_shapes_gpu.py."""
import ctypes as C

import pytest

INVALID = -1   # Q3TTS_ERR_INVALID


def _create(**fields):
    from q3tts import _abi
    lib = _abi.load_library()
    cfg = _abi.tiny_config(max_batch=4, n_ctx=256, with_vocoder=0)
    for k, v in fields.items():
        setattr(cfg.model, k, v)
    h = C.c_void_p()
    rc = lib.q3tts_engine_create(C.byref(cfg), C.byref(h))
    assert not h.value or rc != INVALID
    if h.value:   # (a machine with a device: an admitted shape was created)
        lib.q3tts_engine_destroy(h)
    return rc, lib.q3tts_last_error(None).decode()


@pytest.mark.parametrize("fields,names", [
    (dict(t_n_head=12, t_n_kv_head=4), ("t_n_head", "t_n_kv_head")),      # three query heads per KV head
    (dict(t_n_head=8, t_n_kv_head=1), ("t_n_head", "t_n_kv_head")),       # eight
    (dict(t_n_head=4, t_n_kv_head=3), ("t_n_head", "t_n_kv_head")),       # not a whole number
    (dict(t_n_kv_head=0), ("t_n_kv_head",)),                              # (was a division by zero in the check itself)
    (dict(p_n_kv_head=0), ("p_n_kv_head",)),
    (dict(p_n_head=12, p_n_kv_head=4), ("p_n_head", "p_n_kv_head")),
    (dict(p_n_head=8, p_n_kv_head=1), ("p_n_head", "p_n_kv_head")),
    (dict(n_codebooks=1), ("n_codebooks",)),
    (dict(n_codebooks=17), ("n_codebooks",)),
])
def test_a_shape_without_kernels_is_refused_by_name(fields, names):
    rc, msg = _create(**fields)
    assert rc == INVALID and all(n in msg for n in names), (fields, msg)


@pytest.mark.parametrize("fields", [dict(t_n_head=4, t_n_kv_head=4, p_n_head=4, p_n_kv_head=4), dict(t_n_head=8, t_n_kv_head=2, p_n_head=8, p_n_kv_head=2),
                                    dict(t_n_head=4, t_n_kv_head=1), dict(p_n_head=4, p_n_kv_head=4), dict(n_codebooks=2), dict(n_codebooks=3)])
def test_the_shapes_of_test_shapes_gpu_pass_the_config_check(fields):
    """... and those are not refused by the config check (without a device the call then fails for that reason; with one it succeeds)."""
    rc, msg = _create(**fields)
    assert rc != INVALID and (rc == 0 or "config check" not in msg), (fields, rc, msg)

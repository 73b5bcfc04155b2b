"""Voices in a session on the host side (include/q3tts.h, "voices in a session"): the new entry points are exported and refuse NULL handles,
Q3TTS_EV_PREFIX has the header's value, and q3tts_request kept its size."""
import ctypes as C
import os
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW = ("q3tts_session_prefix_create", "q3tts_session_submit_keep_voice", "q3tts_session_prefix_release", "q3tts_session_clone",
       "q3tts_prefix_state", "q3tts_k_prefix_read")


def test_ev_prefix_and_struct_sizes_match_the_header(tmp_path):
    from q3tts import _abi
    cc = shutil.which("cc") or shutil.which("gcc")
    if cc is None:
        pytest.fail("no C compiler on PATH")
    src = tmp_path / "voices.c"
    src.write_text("""
#include <stdio.h>
#include "q3tts.h"
int main(void) { printf("%d %zu %zu\\n", Q3TTS_EV_PREFIX, sizeof(q3tts_request), sizeof(q3tts_session_event)); return 0; }
""")
    exe = tmp_path / "voices"
    subprocess.check_call([cc, "-I", os.path.join(REPO, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert got == [_abi.EV_PREFIX, 80, C.sizeof(_abi.SessionEvent)]
    assert _abi.EV_PREFIX == 5 and C.sizeof(_abi.Request) == 80
    assert _abi.EV_PREFIX not in (_abi.EV_NONE, _abi.EV_CHUNK, _abi.EV_DONE, _abi.EV_FAILED, _abi.EV_CANCELLED)


def test_new_entry_points_are_exported_and_refuse_null_handles():
    from q3tts import _abi
    lib = _abi.load_library()
    for s in NEW:
        assert hasattr(lib, s), s
        assert s in _abi.SYMBOLS, s
    h, rid, n, nb = C.c_void_p(), C.c_uint64(0), C.c_int32(0), C.c_int64(0)
    req = _abi.Request()
    assert lib.q3tts_session_prefix_create(None, None, None, 0, C.byref(h), C.byref(rid)) == -1 and not h.value
    assert lib.q3tts_session_submit_keep_voice(None, C.byref(req), 0, C.byref(rid), C.byref(h)) == -1 and not h.value
    assert lib.q3tts_session_prefix_release(None, None) == -1
    assert lib.q3tts_session_clone(None, None, 0, 24000, None, 0, C.byref(n), None) == -1
    assert b"null" in lib.q3tts_session_last_error(None)
    assert lib.q3tts_prefix_state(None) == -1
    assert lib.q3tts_prefix_rows(None) == 0
    assert lib.q3tts_k_prefix_read(None, None, None, 0, C.byref(nb)) == -1

"""Sessions on the host side: the ctypes mirror of q3tts_session_event has the C layout, and the session entry points are exported."""
import ctypes as C
import os
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_session_event_layout_matches_the_header(tmp_path):
    from q3tts import _abi
    cc = shutil.which("cc") or shutil.which("gcc")
    if cc is None:
        pytest.fail("no C compiler on PATH")
    src = tmp_path / "layout.c"
    src.write_text("""
#include <stddef.h>
#include <stdio.h>
#include "q3tts.h"
int main(void) {
    printf("%zu %zu %zu %zu %zu %zu %zu %zu %d %d %d %d %d %d\\n", sizeof(q3tts_session_event), offsetof(q3tts_session_event, kind),
           offsetof(q3tts_session_event, status), offsetof(q3tts_session_event, pcm), offsetof(q3tts_session_event, n_samples),
           offsetof(q3tts_session_event, is_final), offsetof(q3tts_session_event, result), sizeof(q3tts_result),
           Q3TTS_EV_CHUNK, Q3TTS_EV_DONE, Q3TTS_EV_FAILED, Q3TTS_EV_CANCELLED, Q3TTS_PCM_I16, Q3TTS_SESSION_RING_DEPTH);
    return 0;
}
""")
    exe = tmp_path / "layout"
    subprocess.check_call([cc, "-I", os.path.join(REPO, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    E = _abi.SessionEvent
    want = [C.sizeof(E), E.kind.offset, E.status.offset, E.pcm.offset, E.n_samples.offset, E.is_final.offset, E.result.offset,
            C.sizeof(_abi.Result), _abi.EV_CHUNK, _abi.EV_DONE, _abi.EV_FAILED, _abi.EV_CANCELLED, _abi.PCM_I16, _abi.SESSION_RING_DEPTH]
    assert got == want


def test_session_entry_points_are_exported_and_refuse_null_handles():
    from q3tts import _abi
    lib = _abi.load_library()
    for s in ("q3tts_session_create", "q3tts_session_submit", "q3tts_session_cancel", "q3tts_session_next", "q3tts_session_close",
              "q3tts_session_last_error", "q3tts_k_pcm_pack"):
        assert hasattr(lib, s), s
    ev = _abi.SessionEvent()
    assert lib.q3tts_session_next(None, 0, C.byref(ev)) == -1
    assert lib.q3tts_session_cancel(None, 1) == -1
    assert lib.q3tts_session_close(None) == -1
    assert b"null" in lib.q3tts_session_last_error(None)
    h = C.c_void_p()
    assert lib.q3tts_session_create(None, 0, C.byref(h)) == -1

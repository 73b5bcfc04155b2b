"""The rules of a well-formed request that a session's submit and every admission refuse alike (q3_request_rules in q3_admit.hip), through
the host-only hook q3tts_k_request_rules: a table of accepted and refused requests, the message buffer's bounds, the export."""
import ctypes as C

import numpy as np

INVALID = -1


def _request(embd=False, n_text=None, text_stream=0, text_open=0, prefix=False, keep=None):
    """A request with prompt_embd (embd) or a prompt of n_text ids (None: neither); everything it points at is returned with it."""
    from q3tts import _abi
    r, alive = _abi.Request(), []
    if embd:
        rows = np.zeros((4, 8), dtype=np.float32)
        r.prompt_embd, r.n_tok = rows.ctypes.data_as(C.POINTER(C.c_float)), 4
        alive.append(rows)
    if n_text is not None:
        ids, d = np.arange(100, 100 + max(n_text, 1), dtype=np.uint32), _abi.PromptDesc()
        d.text_ids, d.n_text = ids.ctypes.data_as(C.POINTER(C.c_uint32)), n_text
        r.prompt = C.pointer(d)
        alive += [ids, d]
    r.text_stream, r.text_open = text_stream, text_open
    if prefix:   # the rules look at the pointer only: is one named or not
        alive.append(C.create_string_buffer(64))
        r.prefix = C.addressof(alive[-1])
    return r, alive


ACCEPTED = [
    ("prompt_embd", dict(embd=True), None),
    ("a prompt from ids", dict(n_text=5), None),
    ("text_stream with n_text = 1", dict(n_text=1, text_stream=1), None),
    ("text_stream + text_open", dict(n_text=3, text_stream=1, text_open=1), None),
    ("keep-voice, voice_rows = 3 on prompt_embd", dict(embd=True), 3),
    ("keep-voice, voice_rows = 0 on a prompt from ids", dict(n_text=5), 0),
]
REFUSED = [   # (what, request, keep's voice_rows or None, a word of the rule's message)
    ("text_open without text_stream", dict(n_text=3, text_open=1), None, "text_open"),
    ("text_stream with prompt_embd", dict(embd=True, text_stream=1), None, "prompt_embd"),
    ("text_stream with no prompt", dict(text_stream=1), None, "text_stream"),
    ("text_stream with n_text = 0", dict(n_text=0, text_stream=1), None, "n_text"),
    ("keep-voice together with a prefix", dict(n_text=5, prefix=True), 0, "names a prefix"),
    ("keep-voice with voice_rows = -1", dict(n_text=5), -1, "voice_rows"),
    ("keep-voice with voice_rows = 0 on prompt_embd", dict(embd=True), 0, "voice_rows"),
]


def _rules(lib, r, keep_rows, cap=256):
    msg = C.create_string_buffer(b"\x7f" * (cap + 8), cap + 9)
    st = lib.q3tts_k_request_rules(C.byref(r) if r is not None else None, 0 if keep_rows is None else 1, keep_rows or 0, msg, cap)
    assert msg.raw[cap:cap + 8] == b"\x7f" * 8, "the hook wrote past cap"
    return st, msg.value.decode()


def test_request_rules_table():
    from q3tts import _abi
    lib = _abi.load_library()
    assert "q3tts_k_request_rules" in _abi.SYMBOLS and hasattr(lib, "q3tts_k_request_rules")
    for what, kw, keep_rows in ACCEPTED:
        r, alive = _request(**kw)
        assert _rules(lib, r, keep_rows) == (0, ""), what
    for what, kw, keep_rows, word in REFUSED:
        r, alive = _request(**kw)
        st, msg = _rules(lib, r, keep_rows)
        assert st == INVALID and word in msg, (what, st, msg)
    # without keep the same requests pass the keep-voice rules' side: they are rules of keeping, not of the request
    for what, kw, keep_rows, word in REFUSED[4:]:
        r, alive = _request(**kw)
        assert _rules(lib, r, None) == (0, ""), what
    st, msg = _rules(lib, None, None)
    assert st == INVALID and "null" in msg
    # cap = 1 holds the empty string; cap = 8 a cut message; neither is overrun (checked in _rules); a NULL buffer is allowed
    r, alive = _request(n_text=3, text_open=1)
    assert _rules(lib, r, None, cap=1) == (INVALID, "")
    assert _rules(lib, r, None, cap=8) == (INVALID, "text_op")
    assert lib.q3tts_k_request_rules(C.byref(r), 0, 0, None, 0) == INVALID

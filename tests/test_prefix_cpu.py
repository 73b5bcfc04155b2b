"""Voice prefixes without a GPU: the request struct's layout agrees across the C header, the Python ABI and the Rust shim (arrays of requests
keep their stride), and the Python helpers refuse descs that mix the voice part and the text part."""
import ctypes as C
import os
import re

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _c_fields(src, name):
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), src, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    out = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            out += [re.sub(r"[\s*]", "", v.split()[-1] if " " in v.strip() else v) for v in decl.split(",")]
    return [re.sub(r".*[\s*]", "", f) for f in out]


def _rust_fields(src, name):
    body = re.search(r"pub struct %s \{(.*?)\n\}" % name, src, re.S).group(1)
    body = re.sub(r"//[^\n]*", "", body)
    return re.findall(r"pub (\w+):", body)


def test_request_field_order_agrees():
    from q3tts import _abi
    with open(os.path.join(REPO, "include", "q3tts.h")) as f:
        c = _c_fields(f.read(), "q3tts_request")
    with open(os.path.join(REPO, "rust", "src", "lib.rs")) as f:
        rs = _rust_fields(f.read(), "q3tts_request")
    py = [n for n, _ in _abi.Request._fields_]
    assert c == py == rs, (c, py, rs)
    assert c[-1] == "prefix"
    assert _abi.Request.prefix.offset == _abi.Request.want_pcm.offset + 4 == 72   # appended: every earlier field keeps its offset
    assert _abi.Request.prefix.size == 8 and C.sizeof(_abi.Request) == 80


def test_prefix_symbols_are_declared():
    from q3tts import _abi
    with open(os.path.join(REPO, "include", "q3tts.h")) as f:
        h = f.read()
    for s in ("q3tts_prefix_create", "q3tts_prefix_rows", "q3tts_prefix_destroy", "q3tts_k_talker_prefill_prefix"):
        assert s in _abi.SYMBOLS and re.search(r"\b%s\(" % s, h), s


def test_make_prompt_desc_parts():
    from q3tts import native
    spk = np.zeros(16, dtype=np.float32)
    d, keep = native.make_prompt_desc(None, part="voice", spk_emb=spk)
    assert d.n_text == 0 and d.lang_id == 2055 and bool(d.spk_emb)
    d, keep = native.make_prompt_desc(np.arange(5), part="text")
    assert d.n_text == 5 and d.lang_id == -1 and d.spk_id == -1
    assert not d.spk_emb and not d.instruct_ids and not d.ref_codes and not d.ref_text_ids
    d, keep = native.make_prompt_desc(np.arange(5), part="text", lang_id=None, spk_id=-1)
    assert d.lang_id == -1
    d, keep = native.make_prompt_desc(np.arange(5), spk_emb=spk)   # the whole prompt keeps its defaults
    assert d.lang_id == 2055 and d.n_text == 5


def test_make_prompt_desc_refuses_mixed_parts():
    from q3tts import native
    spk = np.zeros(16, dtype=np.float32)
    with pytest.raises(ValueError, match="text"):
        native.make_prompt_desc(np.arange(3), part="voice", spk_emb=spk)
    for kw, field in ((dict(spk_emb=spk), "spk_emb"), (dict(lang_id=2055), "lang_id"), (dict(spk_id=7), "spk_id"),
                      (dict(instruct_ids=[1, 2]), "instruct_ids"), (dict(ref_codes=np.zeros((1, 16))), "ref_codes"),
                      (dict(ref_text_ids=[1]), "ref_text_ids")):
        with pytest.raises(ValueError, match=field):
            native.make_prompt_desc(np.arange(3), part="text", **kw)
    with pytest.raises(ValueError, match="part"):
        native.make_prompt_desc(np.arange(3), part="both")


def test_create_prefix_needs_exactly_one_source():
    from q3tts import native
    eng = native.NativeEngine.__new__(native.NativeEngine)   # argument checks come before any library call
    with pytest.raises(ValueError):
        eng.create_prefix()
    with pytest.raises(ValueError):
        eng.create_prefix(desc=object(), embd=np.zeros((1, 4), dtype=np.float32))


def test_api_prefix_keywords():
    import inspect
    from q3tts import api
    for name in ("generate_with_voice", "generate_batch_with_voice", "stream_batch_with_voice"):
        p = inspect.signature(getattr(api.TtsEngine, name)).parameters["prefix"]
        assert p.kind == p.KEYWORD_ONLY and p.default is None, name
    assert list(inspect.signature(api.TtsEngine.voice_prefix).parameters) == ["self", "voice", "instruct"]

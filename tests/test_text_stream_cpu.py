"""Streamed text input on the CPU (include/q3tts.h, "streaming text input"): the restatement tests/_text_stream.py pinned to the oracle, the
streamed prompt rows, the readiness rule, the C ABI's new fields and symbols, and the condition on the inputs of
tests/test_text_stream_gpu.py — a build that kept the whole text in the prompt, or added tts_pad to every feedback row, must not be able
to pass them."""
import ctypes as C

import numpy as np
import pytest

import _text_stream as TS

S = TS.S
INVALID = -1   # Q3TTS_ERR_INVALID


@pytest.fixture(scope="module")
def tiny(oracle):
    cfg = TS.tiny_cfg()
    om = oracle.OracleModel(cfg.model, seed=0, n_ctx=TS.N_CTX, n_threads=8)
    yield om, TS.mats_from_model(om, False, False)
    om.close()


# ---- 1. no trailing rows and today's prompt: the oracle --------------------------------------------------------------------------------
@pytest.mark.parametrize("talker", sorted(TS.TALKERS))
def test_restatement_without_trailing_rows_is_the_oracle(tiny, talker):
    om, pred = tiny
    pe = TS.whole_prompt(om, TS.TEXTS["n6"])
    ref, ref_eos = om.generate(pe, **TS.request(talker))
    got, eos = TS.generate(om, pred, pe, (), **TS.request(talker))
    assert ref.shape[0] == TS.FRAMES and eos == ref_eos and np.array_equal(got, ref)


# ---- 2. the streamed prompt ------------------------------------------------------------------------------------------------------------
def test_streamed_text_part_rows(tiny, oracle):
    om, _ = tiny
    ids = TS.TEXTS["oob"]
    rows, T = TS.prompt(om, ids)
    whole = TS.whole_prompt(om, ids)
    nv = whole.shape[0] - (len(ids) + 3)
    assert rows.shape[0] == nv + 2 and np.array_equal(rows[:nv], whole[:nv])   # the voice part is today's
    bos = (TS.text_row(om, TS.TTS_BOS) + TS.codec_row(om, 0, TS.CODEC_PAD)).astype(np.float32)
    first = (TS.text_row(om, ids[0]) + TS.codec_row(om, 0, TS.CODEC_BOS)).astype(np.float32)
    assert np.array_equal(rows[nv], bos) and np.array_equal(rows[nv], whole[nv]) and np.array_equal(rows[nv + 1], first)
    assert T == [int(i) for i in ids[1:]] + [TS.TTS_EOS] and TS.trailing(ids, closed=False) == [int(i) for i in ids[1:]]
    assert TS.trailing(TS.TEXTS["n1"]) == [TS.TTS_EOS]
    # an id beyond the table takes the reference's pattern, not a table row
    d = om.cfg.d_embed
    pat = (np.fmod((np.float64(200000) * 17 + np.arange(d)), 2.0) - 1.0).astype(np.float32)
    assert om.cfg.text_vocab <= 200000 and np.array_equal(TS.text_row(om, 200000), pat)


# ---- 3. the GPU tests' inputs tell the two layouts apart -------------------------------------------------------------------------------
@pytest.mark.parametrize("talker", sorted(TS.TALKERS))
@pytest.mark.parametrize("name", sorted(TS.TEXTS))
def test_gpu_inputs_the_whole_text_layout_would_fail(tiny, name, talker):
    om, pred = tiny
    ids = TS.TEXTS[name]
    rows, T = TS.prompt(om, ids)
    kw = TS.request(talker)
    streamed, _ = TS.generate(om, pred, rows, T, **kw)
    whole, _ = om.generate(TS.whole_prompt(om, ids), **kw)
    padded, _ = TS.generate(om, pred, rows, (), **kw)   # the streamed prompt with tts_pad on every row: the kernel's default last pass
    assert streamed.shape[0] == TS.FRAMES
    assert not np.array_equal(streamed, whole) and not np.array_equal(streamed, padded)
    assert not np.array_equal(streamed[:4], padded[:4])   # ... already inside the first chunk (the session tests look at it alone)


def test_gpu_batch_inputs_the_whole_text_layout_would_fail(tiny):
    om, pred = tiny
    for i, r in enumerate(TS.batch_requests()):
        if not r["stream"]:
            continue
        rows, T = TS.prompt(om, r["ids"])
        streamed, _ = TS.generate(om, pred, rows, T, **r["kw"])
        whole, _ = om.generate(TS.whole_prompt(om, r["ids"]), **r["kw"])
        assert streamed.shape[0] == r["kw"]["min_frames"], i
        assert not np.array_equal(streamed, whole), i


# ---- 4. the readiness rule -------------------------------------------------------------------------------------------------------------
READY = [
    # (n_text, closed, n_frames) -> ready
    ((1, 0, 0), 0), ((1, 0, 4), 0), ((1, 0, 60), 0),      # one id, open: len(T) = 0, never ready
    ((1, 1, 0), 1), ((1, 1, 12), 1),                      # closed text is always ready
    ((4, 0, 0), 0),                                       # len(T) = 3 < 4
    ((5, 0, 0), 1), ((5, 0, 4), 0), ((5, 1, 4), 1),       # len(T) = 4: frames 0..3 and no further, until it is closed
    ((8, 0, 0), 1), ((8, 0, 4), 0), ((9, 0, 4), 1), ((9, 0, 8), 0),
    ((41, 0, 36), 1), ((41, 0, 40), 0), ((40, 1, 40), 1),
    ((2 ** 31 - 1, 0, 2 ** 31 - 8), 1), ((5, 0, 2 ** 31 - 1), 0),   # no overflow in f + 4
]


def test_readiness_rule():
    from q3tts import _abi
    lib = _abi.load_library()
    for (n_text, closed, f), want in READY:
        assert lib.q3tts_k_text_ready(n_text, closed, f) == want, (n_text, closed, f)
        lenT = n_text - 1 + (1 if closed else 0)
        assert want == (1 if closed or lenT >= f + 4 else 0)   # the rule as include/q3tts.h words it


# ---- 5. the ABI ------------------------------------------------------------------------------------------------------------------------
def test_abi_fields_and_append_text():
    from q3tts import _abi
    names = [n for n, _ in _abi.Request._fields_]
    assert "text_stream" in names and "text_open" in names and names[-1] == "prefix"
    # the two fields fill the alignment gaps the struct always had: no other field moved and the size is what it was
    assert _abi.Request.text_stream.offset == _abi.Request.n_tok.offset + 4 == 12 and _abi.Request.prompt.offset == 16
    assert _abi.Request.text_open.offset == _abi.Request.has_seed.offset + 4 == 44 and _abi.Request.seed.offset == 48
    assert _abi.Request.prefix.offset == 72 and C.sizeof(_abi.Request) == 80
    r = _abi.Request()
    assert r.text_stream == 0 and r.text_open == 0   # zero = today's behaviour
    assert "q3tts_session_append_text" in _abi.SYMBOLS and "q3tts_k_text_ready" in _abi.SYMBOLS
    lib = _abi.load_library()
    ids = (C.c_uint32 * 2)(1, 2)
    assert lib.q3tts_session_append_text(None, 1, ids, 2, 0) == INVALID
    assert lib.q3tts_session_append_text(None, 1, None, 2, 0) == INVALID
    assert lib.q3tts_session_append_text(None, 1, None, 0, 1) == INVALID
    assert b"null session" in lib.q3tts_session_last_error(None)

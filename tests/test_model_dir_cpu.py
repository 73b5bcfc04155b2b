"""Opening a model directory from its files alone (host only): typed GGUF metadata through the reader's test hook, and
q3tts_config_from_model_dir on directories written by tests/_model_dir.py.

Nothing here has a tolerance: every comparison is equality of integers, bytes or message substrings. The library loads without a GPU
(as in test_host_cpu.py); no engine is created.
"""
import ctypes as C
import os
import shutil
import struct
import subprocess
import sys
import textwrap

import numpy as np
import pytest

import _gguf as G
import _model_dir as MD
from _model_dir import DROP, Typed

OK, INVALID, IO = 0, -1, -4
A = "qwen3"


# ---- 1. typed metadata through q3tts_k_gguf_meta ----------------------------------------------------------------------
TYPED = {
    "t.u8": (Typed(MD.U8, 200), "u8", 200.0), "t.i8": (Typed(MD.I8, -5), "i8", -5.0),
    "t.u16": (Typed(MD.U16, 60000), "u16", 60000.0), "t.i16": (Typed(MD.I16, -30000), "i16", -30000.0),
    "t.u32": (Typed(MD.U32, 4000000000), "u32", 4000000000.0), "t.i32": (Typed(MD.I32, -2000000000), "i32", -2000000000.0),
    "t.f32": (Typed(MD.F32, 1.5), "f32", 1.5), "t.bool": (Typed(MD.BOOL, True), "bool", 1.0),
    "t.u64": (Typed(MD.U64, 2 ** 53), "u64", float(2 ** 53)), "t.i64": (Typed(MD.I64, -(2 ** 53)), "i64", -float(2 ** 53)),
    "t.f64": (Typed(MD.F64, 1e-300), "f64", 1e-300),   # not representable in f32: a reader that narrows gives 0
    "t.str": (Typed(MD.STR, "héllo wörld"), "str", "héllo wörld".encode()), "t.empty": (Typed(MD.STR, ""), "str", b""),
}
ARRAYS = {
    "a.i32": (Typed(MD.ARR, [-1, 2, 3], elem=MD.I32), "i32", [-1.0, 2.0, 3.0]),
    "a.u8": (Typed(MD.ARR, [0, 255], elem=MD.U8), "u8", [0.0, 255.0]),
    "a.i64": (Typed(MD.ARR, [-(2 ** 40), 2 ** 40], elem=MD.I64), "i64", [-float(2 ** 40), float(2 ** 40)]),
    "a.u16": (Typed(MD.ARR, [1, 65535], elem=MD.U16), "u16", [1.0, 65535.0]),
    "a.f32": (Typed(MD.ARR, [0.5, -2.0], elem=MD.F32), "f32", [0.5, -2.0]),
    "a.f64": (Typed(MD.ARR, [1e-300, 3.0], elem=MD.F64), "f64", [1e-300, 3.0]),
    "a.bool": (Typed(MD.ARR, [True, False, True], elem=MD.BOOL), "bool", [1.0, 0.0, 1.0]),
    "a.str": (Typed(MD.ARR, ["a", "", "日本語", "x" * 300], elem=MD.STR), "str", [b"a", b"", "日本語".encode(), b"x" * 300]),
    "a.none": (Typed(MD.ARR, [], elem=MD.I32), "i32", []),
}


@pytest.mark.parametrize("version,alignment", [(3, 32), (2, 32), (3, 64), (2, 128)])
def test_typed_metadata_round_trips(tmp_path, version, alignment):
    """Every scalar type, strings, and integer / float / bool / string arrays come back with their own type and exact value, in GGUF v2
    and v3; the tensor behind a non-default general.alignment is still found where the alignment puts it."""
    from q3tts import _abi, native
    rng = np.random.default_rng(version * 1000 + alignment)
    w = rng.standard_normal((4, 64)).astype(np.float32)       # 1024 bytes: a multiple of every alignment used
    v = rng.standard_normal((128,)).astype(np.float32)
    meta = {"general.architecture": "qwen3", "general.alignment": alignment}
    meta.update({k: t for k, (t, _, _) in TYPED.items()})
    meta.update({k: t for k, (t, _, _) in ARRAYS.items()})
    meta["tokenizer.ggml.tokens"] = ["<%d>" % i for i in range(150000)]   # the bulk of a real file: walked, never copied
    meta["z.last"] = Typed(MD.I16, -2)                                    # a value behind the bulk
    p = str(tmp_path / "m.gguf")
    MD.write_gguf(p, [("w", w, G.F32), ("v", v, G.F32)], meta=meta, version=version)
    for k, (_, tname, want) in TYPED.items():
        assert native.k_gguf_meta(p, k) == (tname, tname, want), k
    for k, (_, ename, want) in ARRAYS.items():
        assert native.k_gguf_meta(p, k) == ("array", ename, want), k
    assert native.k_gguf_meta(p, "general.alignment") == ("u32", "u32", float(alignment))
    assert native.k_gguf_meta(p, "z.last") == ("i16", "i16", -2.0)
    ty, ety, toks = native.k_gguf_meta(p, "tokenizer.ggml.tokens")
    assert (ty, ety, len(toks), toks[0], toks[-1]) == ("array", "str", 150000, b"<0>", b"<149999>")
    for name, want in (("w", w), ("v", v)):
        got, gty = native.k_gguf_read(p, name)
        assert gty == G.F32 and np.array_equal(got.view(np.uint32), want.view(np.uint32)), name
    with pytest.raises(_abi.Q3Error, match="'t.nope' is missing"):
        native.k_gguf_meta(p, "t.nope")
    # a NULL buffer queries type and count; a buffer that is too small is refused
    lib = _abi.load_library()
    vt, et, n, nb = C.c_int32(-1), C.c_int32(-1), C.c_int64(-1), C.c_int64(-1)
    assert lib.q3tts_k_gguf_meta(p.encode(), b"a.f64", C.byref(vt), C.byref(et), C.byref(n), None, 0, None, 0, C.byref(nb)) == OK
    assert (vt.value, et.value, n.value, nb.value) == (MD.ARR, MD.F64, 2, 0)
    one = (C.c_double * 1)()
    assert lib.q3tts_k_gguf_meta(p.encode(), b"a.f64", None, None, None, one, 1, None, 0, None) == INVALID
    assert lib.q3tts_k_gguf_meta(p.encode(), b"t.str", C.byref(vt), None, C.byref(n), None, 0, None, 0, C.byref(nb)) == OK
    assert (vt.value, n.value, nb.value) == (MD.STR, 1, len("héllo wörld".encode()))
    small = C.create_string_buffer(4)
    assert lib.q3tts_k_gguf_meta(p.encode(), b"t.str", None, None, None, None, 0, small, 4, None) == INVALID


def test_metadata_lengths_past_the_file_name_the_key(tmp_path):
    """An array or string length that runs past the file is an error naming the key — the byte offset when the key itself is cut —
    and nested arrays are refused."""
    from q3tts import _abi, native
    v = np.arange(64, dtype=np.float32)
    p = str(tmp_path / "m.gguf")

    def refused(meta, match, patch=None):
        MD.write_gguf(p, [("v", v, G.F32)], meta=meta)
        if patch:
            raw = bytearray(open(p, "rb").read())
            patch(raw)
            open(p, "wb").write(bytes(raw))
        with pytest.raises(_abi.Q3Error, match=match):
            native.k_gguf_meta(p, "general.architecture")

    def set_u64(at):
        return lambda raw: raw.__setitem__(slice(at, at + 8), struct.pack("<Q", 1 << 40))

    head = {"general.architecture": "qwen3"}
    key_at = 24 + len(MD.encode_meta(head))          # where the second key's length field starts
    val_at = key_at + 8 + len("some.key") + 4        # ... and its value
    refused({**head, "some.key": "text"}, "'some.key'.*string length runs past the file", set_u64(val_at))
    refused({**head, "some.key": [1, 2, 3]}, "'some.key'.*array length 1099511627776 runs past the file", set_u64(val_at + 4))
    refused({**head, "some.key": ["a", "b"]}, "'some.key'.*array length 1099511627776 runs past the file", set_u64(val_at + 4))
    refused({**head, "some.key": ["a", "b"]}, "'some.key'.*string length of element 1 runs past the file", set_u64(val_at + 12 + 9))
    refused({**head, "some.key": "text"}, "key at byte offset %d runs past the file" % key_at, set_u64(key_at))
    refused({**head, "some.key": Typed(MD.ARR, [Typed(MD.ARR, [1], elem=MD.I32)], elem=MD.ARR)}, "'some.key'.*nested arrays")
    refused({**head, "some.key": Typed(MD.ARR, [1], elem=MD.I32)}, "'some.key'.*unknown array element type 77",
            lambda raw: raw.__setitem__(slice(val_at, val_at + 4), struct.pack("<I", 77)))


# ---- 2. q3tts_config_from_model_dir: the good directories -----------------------------------------------------------------
def _model_bytes_except_files(cfg):
    """Everything of an EngineConfig the call must leave alone, as bytes: the protocol fields, the vocoder block and the engine fields
    (weights_path excluded: it is the one non-model field the call sets)."""
    m = cfg.model
    return (struct.pack("<3i", m.sample_limit, m.eos_code, m.tts_pad_id) + bytes(cfg.vocoder) +
            struct.pack("<5iQ2i", cfg.device, cfg.max_batch, cfg.n_ctx, cfg.max_steps_cap, cfg.with_vocoder, cfg.synth_seed, cfg.talker_q8_0,
                        cfg.vocoder_flush_tail))


@pytest.mark.parametrize("shape", ["tiny", "b"])
@pytest.mark.parametrize("quant,sub", [(None, "gguf"), ("none", "gguf"), ("q8_0", "gguf_q8_0"), ("q5_k_m", "gguf_q5_k_m"), ("Q8_0", "gguf")])
def test_config_reproduces_the_shape_the_directory_was_written_from(tmp_path, shape, quant, sub):
    m = (MD.shape_tiny if shape == "tiny" else MD.shape_b)(text_vocab=1536)
    MD.write_dir(str(tmp_path / sub), m, seed=3, version=2 if quant == "q8_0" else 3)
    cfg = MD.base_config()
    keep = _model_bytes_except_files(cfg)
    rc, msg, buf = MD.call(tmp_path, quant, cfg)
    assert (rc, msg) == (OK, "")
    assert MD.file_fields(cfg.model) == MD.file_fields(m)
    assert _model_bytes_except_files(cfg) == keep
    assert buf.value == os.fsencode(str(tmp_path / sub)) and cfg.weights_path == buf.value
    assert C.cast(C.byref(cfg, type(cfg).weights_path.offset), C.POINTER(C.c_void_p))[0] == C.addressof(buf)   # points INTO path_buf
    if quant != "Q8_0":   # any other spelling is the plain directory
        rc, msg, _ = MD.call(tmp_path, "Q8_0" if sub != "gguf" else "q8_0", MD.base_config())
        assert rc == IO and "qwen3_tts_talker.gguf" in msg and ("gguf/" if sub != "gguf" else "gguf_q8_0/") in msg


def test_optional_keys_default_as_llama_cpp_does(tmp_path):
    """Without attention.key_length head_dim is embedding_length / head_count; without rope.freq_base theta is 10000; an architecture
    other than "qwen3" prefixes the keys; fewer than four sections leave the rest 0; f64 floats and u64 / i16 counts are taken as they are."""
    m = MD.shape_tiny(text_vocab=1024)   # 512 / 4 = 128: the default rule gives the same head_dim
    m.t_mrope_sections[:] = [40, 24, 0, 0]
    arch = "qwen3vlmoe"
    MD.write_dir(str(tmp_path / "gguf"), m, arch=arch,
                 talker_meta={arch + ".attention.key_length": DROP, arch + ".rope.freq_base": DROP, arch + ".rope.dimension_sections": Typed(MD.ARR, [40, 24], elem=MD.U16),
                              arch + ".block_count": Typed(MD.U64, m.t_n_layer), arch + ".attention.layer_norm_rms_epsilon": Typed(MD.F64, float(m.rms_eps))},
                 pred_meta={arch + ".attention.key_length": DROP, arch + ".attention.head_count": Typed(MD.I16, m.p_n_head)})
    cfg = MD.base_config()
    rc, msg, _ = MD.call(tmp_path, None, cfg)
    assert (rc, msg) == (OK, "")
    want = MD.file_fields(m)
    want["t_rope_theta"] = 10000.0
    assert MD.file_fields(cfg.model) == want


@pytest.mark.parametrize("with_text", [True, False])
def test_npy_assets_and_a_directory_without_a_text_table(tmp_path, with_text):
    m = MD.shape_b(text_vocab=640)
    for assets in ("gguf", "npy"):
        d = tmp_path / assets
        MD.write_dir(str(d / "gguf"), m, assets=assets, with_text=with_text)
        cfg = MD.base_config()
        rc, msg, _ = MD.call(d, None, cfg)
        assert (rc, msg) == (OK, "")
        want = MD.file_fields(m)
        want["text_vocab"] = 640 if with_text else 0
        assert MD.file_fields(cfg.model) == want, assets


# ---- 3. every way a directory can be wrong --------------------------------------------------------------------------------
def _k(s):
    return A + "." + s


REQUIRED = ["general.architecture", _k("block_count"), _k("embedding_length"), _k("feed_forward_length"), _k("attention.head_count"),
            _k("attention.head_count_kv"), _k("attention.layer_norm_rms_epsilon")]
SECTIONS = _k("rope.dimension_sections")


def _retyped(key):
    if key == "general.architecture":
        return 7
    if key == SECTIONS:
        return [24.0, 20.0, 20.0]      # a float array
    if key.endswith("epsilon") or key.endswith("freq_base"):
        return 1                       # an integer where a float belongs
    return "2"                         # a string where a count belongs


def _rows(name, n):
    """replace tensor `name` by one with n rows (same row length)"""
    return lambda t: t.__setitem__(name, np.zeros((n, t[name].shape[1]), np.float32))


def _cols(name, n):
    return lambda t: t.__setitem__(name, np.zeros((t[name].shape[0], n), np.float32))


def _all_codec_cols(n):
    def edit(t):
        for k in list(t):
            if k.startswith("codec_embd."):
                t[k] = np.zeros((t[k].shape[0], n), np.float32)
    return edit


CASES = {}
for _key in REQUIRED + [SECTIONS]:
    CASES["talker absent " + _key] = (dict(talker_meta={_key: DROP}), ["qwen3_tts_talker.gguf", "'%s'" % _key, "is missing"])
    CASES["talker retyped " + _key] = (dict(talker_meta={_key: _retyped(_key)}), ["qwen3_tts_talker.gguf", "'%s'" % _key, "is not"])
for _key in REQUIRED:
    CASES["predictor absent " + _key] = (dict(pred_meta={_key: DROP}), ["qwen3_tts_predictor.gguf", "'%s'" % _key, "is missing"])
    CASES["predictor retyped " + _key] = (dict(pred_meta={_key: _retyped(_key)}), ["qwen3_tts_predictor.gguf", "'%s'" % _key, "is not"])
CASES.update({
    "key_length retyped": (dict(talker_meta={_k("attention.key_length"): "128"}), ["qwen3_tts_talker.gguf", "'%s'" % _k("attention.key_length"), "is not an integer"]),
    "freq_base retyped": (dict(pred_meta={_k("rope.freq_base"): 1000000}), ["qwen3_tts_predictor.gguf", "'%s'" % _k("rope.freq_base"), "is not a float"]),
    "bool is no count": (dict(talker_meta={_k("block_count"): True}), ["'%s'" % _k("block_count"), "is not an integer"]),
    "zero layers": (dict(talker_meta={_k("block_count"): 0}), ["'%s'" % _k("block_count"), "out of range"]),
    "sections sum": (dict(talker_meta={SECTIONS: [24, 20, 19, 0]}), ["qwen3_tts_talker.gguf", "'%s'" % SECTIONS, "sums to 63", "64"]),
    "sections five": (dict(talker_meta={SECTIONS: [24, 20, 20, 0, 0]}), ["'%s'" % SECTIONS, "5 entries"]),
    "sections negative": (dict(talker_meta={SECTIONS: [65, -1]}), ["'%s'" % SECTIONS, "-1"]),
    "two rms_eps": (dict(pred_meta={_k("attention.layer_norm_rms_epsilon"): 1e-5}), ["qwen3_tts_predictor.gguf", "'%s'" % _k("attention.layer_norm_rms_epsilon"), "1e-05", "1e-06"]),
    # tensor shapes against the metadata (tiny: d 512, 4 x 128 query / 2 x 128 key rows, FFN 1024 / 512)
    "talker attn_q": (dict(talker_tensors=_rows("blk.0.attn_q.weight", 640)), ["qwen3_tts_talker.gguf", "'blk.0.attn_q.weight'", "640", "'%s'" % _k("attention.head_count"), "512"]),
    "talker attn_k": (dict(talker_tensors=_rows("blk.0.attn_k.weight", 128)), ["qwen3_tts_talker.gguf", "'blk.0.attn_k.weight'", "128", "'%s'" % _k("attention.head_count_kv"), "256"]),
    "talker attn_output": (dict(talker_tensors=_cols("blk.0.attn_output.weight", 1024)), ["'blk.0.attn_output.weight'", "1024", "'%s'" % _k("attention.head_count"), "512"]),
    "talker ffn_gate": (dict(talker_tensors=_rows("blk.0.ffn_gate.weight", 1536)), ["'blk.0.ffn_gate.weight'", "1536", "'%s'" % _k("feed_forward_length"), "1024"]),
    "talker ffn_down": (dict(talker_tensors=_cols("blk.0.ffn_down.weight", 2048)), ["'blk.0.ffn_down.weight'", "2048", "'%s'" % _k("feed_forward_length"), "1024"]),
    "talker embedding_length": (dict(talker_meta={_k("embedding_length"): 1024}), ["qwen3_tts_talker.gguf", "'blk.0.attn_q.weight'", "row length 512", "'%s'" % _k("embedding_length"), "1024"]),
    "talker head_count": (dict(talker_meta={_k("attention.head_count"): 8}), ["'blk.0.attn_q.weight'", "512 rows", "'%s'" % _k("attention.head_count"), "1024"]),
    "talker output": (dict(talker_tensors=_cols("output.weight", 256)), ["qwen3_tts_talker.gguf", "'output.weight'", "256", "'%s'" % _k("embedding_length"), "512"]),
    "talker tensor missing": (dict(talker_tensors={"blk.0.ffn_down.weight": DROP}), ["qwen3_tts_talker.gguf", "'blk.0.ffn_down.weight'", "is missing"]),
    "predictor attn_k": (dict(pred_tensors=_rows("blk.0.attn_k.weight", 512)), ["qwen3_tts_predictor.gguf", "'blk.0.attn_k.weight'", "512", "'%s'" % _k("attention.head_count_kv"), "256"]),
    "predictor ffn_gate": (dict(pred_meta={_k("feed_forward_length"): 1024}), ["qwen3_tts_predictor.gguf", "'blk.0.ffn_gate.weight'", "512 rows", "'%s'" % _k("feed_forward_length"), "1024"]),
    "predictor head": (dict(pred_tensors=_rows("output.weight", 15 * 64 + 1)), ["qwen3_tts_predictor.gguf", "'output.weight'", "961", "n_codebooks - 1 = 15"]),
    "proj rows": (dict(asset_tensors=_rows("proj.weight", 256)), ["'proj.weight'", "256 rows", "'%s'" % _k("embedding_length"), "512"]),
    "proj cols": (dict(asset_tensors=_cols("proj.weight", 1024)), ["'proj.weight'", "1024", "'codec_embd.0'", "512"]),
    "proj missing": (dict(asset_tensors={"proj.weight": DROP}), ["'proj.weight'", "is missing"]),
    "d_embed": (dict(asset_tensors=_all_codec_cols(256)), ["'codec_embd.0'", "256", "'%s'" % _k("embedding_length"), "512"]),
    "codec row length": (dict(asset_tensors=_cols("codec_embd.9", 256)), ["'codec_embd.9'", "256", "512"]),
    "codec rows": (dict(asset_tensors=_rows("codec_embd.5", 48)), ["'codec_embd.5'", "48 rows", "'codec_embd.1'", "64"]),
    "text row length": (dict(asset_tensors=_cols("text_embd", 256)), ["text table", "256", "512"]),
    "codec gap": (dict(asset_tensors={"codec_embd.7": DROP}), ["'codec_embd.7' is missing", "contiguous"]),
    "codec from one": (dict(asset_tensors={"codec_embd.0": DROP}), ["'codec_embd.0' is missing", "contiguous"]),
    "codec gap npy": (dict(assets="npy", asset_tensors={"codec_embd.7": DROP}), ["'codec_embedding_7.npy' is missing", "contiguous"]),
    "proj rows npy": (dict(assets="npy", asset_tensors=_rows("proj.weight", 256)), ["'proj_weight.npy'", "256 rows", "512"]),
})


@pytest.mark.parametrize("case", sorted(CASES))
def test_a_wrong_directory_is_refused_by_name_and_leaves_cfg_alone(tmp_path, case):
    kw, needles = CASES[case]
    MD.write_dir(str(tmp_path / "gguf"), MD.shape_tiny(text_vocab=1024), **kw)
    cfg = MD.base_config()
    cfg.weights_path = b"/somewhere/else"
    before = bytes(cfg)
    rc, msg, buf = MD.call(tmp_path, "none", cfg)
    assert rc == INVALID, (rc, msg)
    for n in needles:
        assert n in msg, (n, msg)
    assert bytes(cfg) == before
    assert buf.raw[:-1] == b"\x55" * (len(buf) - 1)   # path_buf untouched as well


def test_a_directory_with_block_count_only_fails_with_the_first_missing_key(tmp_path):
    """tests/_oracle.py's write_model_dir (the writer every earlier test uses) states general.architecture and block_count only."""
    import _oracle as O
    O.write_model_dir(str(tmp_path / "gguf"), MD.shape_tiny(text_vocab=1024), 0)
    cfg = MD.base_config()
    before = bytes(cfg)
    rc, msg, _ = MD.call(tmp_path, None, cfg)
    assert rc == INVALID and "qwen3_tts_talker.gguf" in msg and "'qwen3.embedding_length' is missing" in msg, msg
    assert bytes(cfg) == before


def test_missing_files_small_buffers_and_null_arguments(tmp_path):
    from q3tts import _abi
    m = MD.shape_tiny(text_vocab=1024)
    good = tmp_path / "good"
    MD.write_dir(str(good / "gguf"), m)
    for name in (MD.TALKER, MD.PRED, MD.ASSETS):
        d = tmp_path / ("no_" + name)
        shutil.copytree(good, d)
        os.remove(d / "gguf" / name)
        cfg = MD.base_config()
        before = bytes(cfg)
        rc, msg, _ = MD.call(d, None, cfg)
        assert rc == IO and (name in msg or (name == MD.ASSETS and "qwen3_assets.gguf" in msg)), (name, rc, msg)
        assert bytes(cfg) == before
    rc, msg, _ = MD.call(tmp_path / "nowhere", None, MD.base_config())
    assert rc == IO and "qwen3_tts_talker.gguf" in msg
    # a file that is not a GGUF at all
    d = tmp_path / "junk"
    shutil.copytree(good, d)
    (d / "gguf" / MD.PRED).write_bytes(b"GGML" + b"\0" * 100)
    rc, msg, _ = MD.call(d, None, MD.base_config())
    assert rc == IO and MD.PRED in msg and "not a GGUF" in msg
    # path_cap: the needed size is model_dir + "/gguf" + NUL, and is reported
    need = len(os.fsencode(str(good))) + len("/gguf") + 1
    for cap in (0, 1, need - 1):
        cfg = MD.base_config()
        before = bytes(cfg)
        rc, msg, buf = MD.call(good, None, cfg, path_cap=cap)
        assert rc == INVALID and str(need) in msg and "path_buf" in msg, (cap, msg)
        assert bytes(cfg) == before and buf.raw[:max(cap, 1)] == b"\x55" * max(cap, 1)
    rc, msg, buf = MD.call(good, None, MD.base_config(), path_cap=need)
    assert (rc, msg) == (OK, "") and buf.value == os.fsencode(str(good / "gguf"))
    # err_cap 0 / 1 / short: safe (MD.call checks the guard byte and the terminator), the status still tells
    bad = tmp_path / "bad"
    MD.write_dir(str(bad / "gguf"), m, talker_meta={_k("block_count"): DROP})
    for cap in (0, 1, 2, 17):
        rc, msg, _ = MD.call(bad, None, MD.base_config(), err_cap=cap)
        assert rc == INVALID and msg == ("qwen3_tts_talker.gguf: metadata key 'qwen3.block_count' is missing")[:max(cap - 1, 0)]
    lib = _abi.load_library()
    cfg = MD.base_config()
    assert lib.q3tts_config_from_model_dir(os.fsencode(str(bad)), None, C.byref(cfg), C.create_string_buffer(512), 512, None, 0) == INVALID   # err may be NULL
    assert lib.q3tts_config_from_model_dir(None, None, C.byref(cfg), C.create_string_buffer(512), 512, None, 0) == INVALID
    assert lib.q3tts_config_from_model_dir(os.fsencode(str(good)), None, None, C.create_string_buffer(512), 512, None, 0) == INVALID
    assert lib.q3tts_config_from_model_dir(os.fsencode(str(good)), None, C.byref(cfg), None, 512, None, 0) == INVALID


# ---- 4. robustness: the Talker file cut at every byte of its header, KV and tensor-info sections ---------------------------
TRUNC_DRIVER = textwrap.dedent('''
    import ctypes as C, os, sys
    lib = C.CDLL(sys.argv[1]); model_dir = sys.argv[2]; end = int(sys.argv[3])
    lib.q3tts_config_from_model_dir.argtypes = [C.c_char_p, C.c_char_p, C.c_void_p, C.c_char_p, C.c_int32, C.c_char_p, C.c_int32]
    path = os.path.join(model_dir, "gguf", "qwen3_tts_talker.gguf")
    good = open(path, "rb").read()
    cfg = (C.c_char * 512)(); buf = C.create_string_buffer(4096); err = C.create_string_buffer(512)   # (512 bytes > sizeof(q3tts_engine_config))
    for c in range(end + 1):
        with open(path, "wb") as f:
            f.write(good[:c])
        before = bytes(cfg)
        rc = lib.q3tts_config_from_model_dir(model_dir.encode(), None, cfg, buf, len(buf), err, len(err))
        assert rc in (-1, -4) and len(err.value) > 10 and b"qwen3_tts_talker.gguf" in err.value, (c, rc, err.value)
        assert bytes(cfg) == before, c
    with open(path, "wb") as f:
        f.write(good)
    assert lib.q3tts_config_from_model_dir(model_dir.encode(), None, cfg, buf, len(buf), err, len(err)) == 0, err.value
    print("DONE", end + 1)
''')


def _truncation_dir(tmp_path):
    """A small header (64 tokens) so that every byte offset up to the start of the data section can be tried."""
    d = tmp_path / "cut"
    MD.write_dir(str(d / "gguf"), MD.shape_tiny(text_vocab=1024), n_tokens=64)
    raw = open(d / "gguf" / MD.TALKER, "rb").read()
    _, info_start, info_end, al = MD.sections(raw)
    data_start = (info_end + al - 1) // al * al
    assert 24 < info_start < info_end <= data_start < len(raw)
    return d, data_start


def test_truncated_talker_file_always_fails_with_a_message(tmp_path):
    from q3tts import _abi
    d, data_start = _truncation_dir(tmp_path)
    drv = tmp_path / "driver.py"
    drv.write_text(TRUNC_DRIVER)
    r = subprocess.run([sys.executable, str(drv), _abi.LIB_PATH, str(d), str(data_start)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "DONE %d" % (data_start + 1) in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])


import test_host_sanitized_cpu as HS  # noqa: E402  (the host AddressSanitizer mechanism: compiler check, runtime lookup, child-process environment)


@pytest.mark.skipif(shutil.which("g++") is None or HS._asan_runtime() is None, reason="g++ with libasan is needed")
def test_truncated_talker_file_under_the_host_sanitizers(tmp_path):
    """The same walk against the host-only sources compiled with -fsanitize=address,undefined (CPU build; no GPU code is involved): no
    read past the mapping at any truncation point."""
    lib = tmp_path / "libq3host_asan.so"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fPIC", "-shared", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-o", str(lib), os.path.join(HS.CSRC, "q3_gguf.cpp"), os.path.join(HS.CSRC, "q3_model_dir.cpp"),
                           os.path.join(HS.REPO, "tests", "asan_stub.cpp")])
    d, data_start = _truncation_dir(tmp_path)
    drv = tmp_path / "driver.py"
    drv.write_text(TRUNC_DRIVER)
    env = dict(os.environ, LD_PRELOAD=HS._asan_runtime(), ASAN_OPTIONS="detect_leaks=0:abort_on_error=0:exitcode=86", UBSAN_OPTIONS="halt_on_error=1:exitcode=87")
    r = subprocess.run([sys.executable, str(drv), str(lib), str(d), str(data_start)], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0 and "DONE %d" % (data_start + 1) in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])


# ---- 5. the Python callers ---------------------------------------------------------------------------------------------
def test_native_wrapper_returns_a_config_that_owns_its_path(tmp_path):
    import gc
    from q3tts import _abi, native
    m = MD.shape_b(text_vocab=1024)
    MD.write_dir(str(tmp_path / "gguf_q8_0"), m)
    base = MD.base_config()
    before = bytes(base)
    cfg = native.config_from_model_dir(str(tmp_path), "q8_0", base=base)
    gc.collect()
    assert bytes(base) == before and cfg is not base
    assert MD.file_fields(cfg.model) == MD.file_fields(m) and cfg.max_batch == 7 and cfg.model.tts_pad_id == 77
    assert cfg.weights_path == os.fsencode(str(tmp_path / "gguf_q8_0"))
    assert native.config_from_model_dir(str(tmp_path), "q8_0").max_batch == _abi.default_config().max_batch
    with pytest.raises(_abi.Q3Error, match=r"\(-4\).*qwen3_tts_talker.gguf"):
        native.config_from_model_dir(str(tmp_path), "q5_k_m")


def test_tts_engine_new_copies_the_config_and_reads_the_shape_from_the_files(tmp_path, monkeypatch):
    """TtsEngine.new with the engine stubbed out (no GPU here): a caller's config object is not modified (api.py used to set talker_q8_0
    and weights_path on it); without a config the shape comes from the files; without files it is the default shape."""
    from q3tts import _abi, api, native
    seen = []

    class Stub:
        def __init__(self, cfg):
            seen.append(cfg)

        def close(self):
            pass

    monkeypatch.setattr(native, "NativeEngine", Stub)
    monkeypatch.chdir(tmp_path)   # (TtsEngine.new also looks for ./speakers)
    m = MD.shape_b(text_vocab=1024)
    wdir = MD.write_dir(str(tmp_path / "model" / "gguf_q8_0"), m)
    cfg = _abi.tiny_config()
    before = bytes(cfg)
    eng = api.TtsEngine.new(str(tmp_path / "model"), "q8_0", config=cfg)
    assert bytes(cfg) == before and cfg.talker_q8_0 == 0 and cfg.weights_path is None
    got = seen[-1]
    assert got is not cfg and got is eng.cfg and got.talker_q8_0 == 2 and got.weights_path == os.fsencode(wdir)
    assert bytes(got.model) == bytes(cfg.model) and bytes(got.vocoder) == bytes(cfg.vocoder) and got.max_batch == cfg.max_batch
    cfg.talker_q8_0 = 1   # a mode the caller chose stays
    api.TtsEngine.new(str(tmp_path / "model"), "q8_0", config=cfg)
    assert seen[-1].talker_q8_0 == 1 and cfg.talker_q8_0 == 1
    # no config: the files decide
    eng = api.TtsEngine.new(str(tmp_path / "model"), "q8_0")
    got, dflt = seen[-1], _abi.default_config()
    assert MD.file_fields(got.model) == MD.file_fields(m) and got.talker_q8_0 == 2 and got.weights_path == os.fsencode(wdir)
    assert bytes(got.vocoder) == bytes(dflt.vocoder) and (got.max_batch, got.n_ctx, got.model.tts_pad_id) == (dflt.max_batch, dflt.n_ctx, dflt.model.tts_pad_id)
    # no GGUF in the quant directory: synthetic weights of the default shape, as before
    api.TtsEngine.new(str(tmp_path / "model"), "none")
    got = seen[-1]
    assert bytes(got.model) == bytes(dflt.model) and got.weights_path is None and got.talker_q8_0 == 0
    # a directory the library refuses: Q3Error with its message
    os.makedirs(tmp_path / "model" / "gguf")
    MD.write_dir(str(tmp_path / "model" / "gguf"), m, talker_meta={_k("rope.dimension_sections"): DROP})
    with pytest.raises(_abi.Q3Error, match="'qwen3.rope.dimension_sections' is missing"):
        api.TtsEngine.new(str(tmp_path / "model"), "none")


def test_rust_shim_declares_and_calls_the_function():
    src = open(os.path.join(HS.REPO, "rust", "src", "lib.rs")).read()
    decl = src[src.index("pub fn q3tts_config_from_model_dir("):]
    decl = decl[:decl.index(";")]
    assert [a.split(":")[0].strip() for a in decl[decl.index("(") + 1:decl.rindex(")")].split(",")] == ["model_dir", "quant", "cfg", "path_buf", "path_cap", "err", "err_cap"]
    new = src[src.index("pub fn new(model_dir: &str, quant: &str)"):src.index("pub fn set_max_steps")]
    assert new.index("q3tts_default_config(") < new.index("q3tts_config_from_model_dir(") < new.index("q3tts_engine_create(")

"""A quant directory with the metadata a real llama.cpp file carries — test infrastructure for q3tts_config_from_model_dir.

The tensors are the synthetic model of tests/_oracle.py (synth_transformer_tensors / synth_asset_tensors) and the container is written by
tests/_gguf.py's `write`; this module adds what that writer cannot express: metadata of every GGUF value type, a non-default
general.alignment, and the full key set of a Talker / Predictor file (plus the bulk: tokenizer.ggml.tokens, token_type, general.name).
Any key can be dropped, retyped or falsified, and any tensor replaced, to write the directories the negative tests need.
`_oracle.write_model_dir` (block_count only) stays as it is: it is the "old" directory those tests must see refused.
"""
import ctypes as C
import os
import struct

import numpy as np

import _gguf as G
import _oracle as O
from q3tts import _abi

U8, I8, U16, I16, U32, I32, F32, BOOL, STR, ARR, U64, I64, F64 = range(13)
TYPE_NAMES = ("u8", "i8", "u16", "i16", "u32", "i32", "f32", "bool", "str", "array", "u64", "i64", "f64")
_FMT = {U8: "<B", I8: "<b", U16: "<H", I16: "<h", U32: "<I", I32: "<i", F32: "<f", BOOL: "<B", U64: "<Q", I64: "<q", F64: "<d"}


class Typed:
    """A metadata value with an explicit GGUF type: Typed(U16, 7), Typed(STR, "x"), Typed(ARR, [..], elem=F64),
    Typed(ARR, [Typed(ARR, [1], elem=I32)], elem=ARR) (nested: refused by the reader)."""

    def __init__(self, ty, value, elem=None):
        self.ty, self.value, self.elem = ty, value, elem


def _s(b):
    return struct.pack("<Q", len(b)) + b


def _payload(ty, v, elem=None):
    if ty == STR:
        return _s(v if isinstance(v, bytes) else str(v).encode())
    if ty == ARR:
        if elem == ARR:  # nested: every element is a Typed(ARR, values, elem=inner) -> inner type, count, payloads
            body = b"".join(_payload(ARR, e.value, e.elem) for e in v)
        else:
            body = b"".join(_payload(elem, e) for e in v)
        return struct.pack("<IQ", elem, len(v)) + body
    return struct.pack(_FMT[ty], (int(bool(v)) if ty == BOOL else v))


def encode_value(v):
    """Python value -> (type id + payload) bytes. Plain values take the types tests/_gguf.py's writer gives them (int: u32, or i64 when it
    does not fit; float: f32; str; list of str / int / float: string / i32 / f32 array)."""
    if isinstance(v, Typed):
        return struct.pack("<I", v.ty) + _payload(v.ty, v.value, v.elem)
    if isinstance(v, bool):
        return struct.pack("<I", BOOL) + _payload(BOOL, v)
    if isinstance(v, int):
        ty = U32 if 0 <= v < 2 ** 32 else I64
        return struct.pack("<I", ty) + _payload(ty, v)
    if isinstance(v, float):
        return struct.pack("<I", F32) + _payload(F32, v)
    if isinstance(v, (str, bytes)):
        return struct.pack("<I", STR) + _payload(STR, v)
    if isinstance(v, (list, tuple)):
        elem = STR if v and all(isinstance(e, (str, bytes)) for e in v) else F32 if v and all(isinstance(e, float) for e in v) else I32
        return struct.pack("<I", ARR) + _payload(ARR, list(v), elem)
    raise TypeError(type(v))


def encode_meta(meta):
    return b"".join(_s(k.encode()) + encode_value(v) for k, v in meta.items())


def sections(raw):
    """Byte offsets of a GGUF file's parts: (kv_start, info_start, info_end, alignment). Walks every KV without decoding it."""
    nt, nkv = struct.unpack_from("<QQ", raw, 8)
    pos, align = 24, 32
    size = {U8: 1, I8: 1, U16: 2, I16: 2, U32: 4, I32: 4, F32: 4, BOOL: 1, U64: 8, I64: 8, F64: 8}

    def skip_str(p):
        return p + 8 + struct.unpack_from("<Q", raw, p)[0]

    for _ in range(nkv):
        key_end = skip_str(pos)
        key = raw[pos + 8:key_end].decode()
        (vt,) = struct.unpack_from("<I", raw, key_end)
        pos = key_end + 4
        if vt == STR:
            pos = skip_str(pos)
        elif vt == ARR:
            et, cnt = struct.unpack_from("<IQ", raw, pos)
            pos += 12
            if et == STR:
                for _ in range(cnt):
                    pos = skip_str(pos)
            else:
                pos += size[et] * cnt
        else:
            if key == "general.alignment":
                align = int.from_bytes(raw[pos:pos + size[vt]], "little")
            pos += size[vt]
    info_start = pos
    for _ in range(nt):
        pos = skip_str(pos)
        (nd,) = struct.unpack_from("<I", raw, pos)
        pos += 4 + 8 * nd + 12
    return 24, info_start, pos, align


def write_gguf(path, tensors, meta=None, version=3):
    """tests/_gguf.py's `write` for the tensors, then the metadata block spliced in with every value type available. The data section
    starts at a multiple of meta["general.alignment"] (default 32); tensor offsets stay those of `write` (multiples of 32), so a larger
    alignment needs tensors whose byte sizes are multiples of it."""
    meta = dict(meta or {})
    G.write(path, tensors, meta=None, version=version)
    raw = open(path, "rb").read()
    _, info_start, info_end, _ = sections(raw)
    assert info_start == 24
    al = meta.get("general.alignment", 32)
    al = al.value if isinstance(al, Typed) else al
    data = raw[(info_end + 31) // 32 * 32:]
    if al != 32:
        pos = 24
        for _ in range(struct.unpack_from("<Q", raw, 8)[0]):  # every tensor offset must suit the alignment
            pos += 8 + struct.unpack_from("<Q", raw, pos)[0]
            (nd,) = struct.unpack_from("<I", raw, pos)
            pos += 4 + 8 * nd + 4
            assert struct.unpack_from("<Q", raw, pos)[0] % al == 0, "tensor sizes must be multiples of the alignment"
            pos += 8
    head = raw[:16] + struct.pack("<Q", len(meta)) + encode_meta(meta) + raw[24:info_end]
    head += b"\0" * ((-len(head)) % al)
    with open(path, "wb") as f:
        f.write(head)
        f.write(data)


# ---- shapes ----------------------------------------------------------------------------------------------------------
def shape_tiny(text_vocab=151936):
    """The parity suite's tiny shape (q3tts._abi.tiny_config)."""
    m = _abi.ModelConfig.from_buffer_copy(_abi.tiny_config().model)
    m.text_vocab = text_vocab
    return m


def shape_b(text_vocab=151936):
    """A second shape that differs from the tiny one in the layer, head, KV-head, FFN and vocabulary counts of both transformers, and has a
    head_dim that is NOT embedding_length / head_count (so attention.key_length has to be honoured). It stays inside what
    q3tts_engine_create accepts (csrc/q3_engine.hip validate): head_dim 128; d_model, d_ffn and n_head * head_dim multiples of 512;
    n_head / n_kv_head in {1, 2, 4}; t_vocab % 32 == 0 and >= the default sample_limit 2160; codebook_size % 16 == 0;
    d_embed == t_d_model."""
    m = shape_tiny(text_vocab)
    m.t_n_layer, m.t_d_model, m.t_n_head, m.t_n_kv_head, m.t_head_dim, m.t_d_ffn, m.t_vocab = 3, 512, 8, 4, 128, 1536, 2176
    m.t_rope_theta = 500000.0
    m.t_mrope_sections[:] = [16, 24, 24, 0]
    m.p_n_layer, m.p_d_model, m.p_n_head, m.p_n_kv_head, m.p_head_dim, m.p_d_ffn = 1, 1024, 8, 4, 128, 1024
    m.p_rope_theta = 10000.0
    m.n_codebooks, m.codebook_size = 16, 32
    m.rms_eps = 1e-5
    m.d_embed, m.codec0_rows, m.codecq_rows = 512, 2304, 32
    return m


FILE_FIELDS = [n for n, _ in _abi.ModelConfig._fields_ if n not in ("sample_limit", "eos_code", "tts_pad_id")]


def file_fields(m):
    """The fields of a model config that the files determine, as comparable Python values."""
    return {n: (list(getattr(m, n)) if n == "t_mrope_sections" else getattr(m, n)) for n in FILE_FIELDS}


# ---- the directory ---------------------------------------------------------------------------------------------------
TALKER, PRED, ASSETS = "qwen3_tts_talker.gguf", "qwen3_tts_predictor.gguf", "qwen3_assets.gguf"


def tfm_meta(m, talker, arch="qwen3", n_tokens=1000):
    """The metadata of a llama.cpp-converted Talker / Predictor file, in the value types llama.cpp's converter writes (u32 counts, f32
    floats, an i32 array of four sections), with the bulk such a file carries."""
    p = "t_" if talker else "p_"
    meta = {
        "general.architecture": arch,
        "general.name": "Qwen3-TTS synthetic " + ("talker" if talker else "predictor"),
        "general.alignment": 32,
        "general.file_type": 32,
        arch + ".context_length": 32768,
        arch + ".block_count": getattr(m, p + "n_layer"),
        arch + ".embedding_length": getattr(m, p + "d_model"),
        arch + ".feed_forward_length": getattr(m, p + "d_ffn"),
        arch + ".attention.head_count": getattr(m, p + "n_head"),
        arch + ".attention.head_count_kv": getattr(m, p + "n_kv_head"),
        arch + ".attention.key_length": getattr(m, p + "head_dim"),
        arch + ".attention.value_length": getattr(m, p + "head_dim"),
        arch + ".rope.freq_base": float(getattr(m, p + "rope_theta")),
        arch + ".attention.layer_norm_rms_epsilon": float(m.rms_eps),
        "tokenizer.ggml.model": "gpt2",
        "tokenizer.ggml.tokens": ["<tok%d>" % i for i in range(n_tokens)],
        "tokenizer.ggml.token_type": [1] * n_tokens,
        "tokenizer.ggml.bos_token_id": 1,
    }
    if talker:
        meta[arch + ".rope.dimension_sections"] = [int(x) for x in m.t_mrope_sections]
    return meta


DROP = object()
_CACHE = {}


def _tensors(m, seed, which, with_text=True):
    """The synthetic tensors of one file (cached: the negative tests write the same model many times)."""
    key = (bytes(m), seed, which, with_text)
    if key not in _CACHE:
        _CACHE[key] = O.synth_asset_tensors(m, seed, with_text) if which == "assets" else O.synth_transformer_tensors(m, seed, which == "talker")
    return dict(_CACHE[key])


def _apply(meta, edit):
    """edit: None, a dict (key -> new value; the value DROP removes the key), or a callable that changes the dict in place."""
    if callable(edit):
        edit(meta)
    elif edit:
        for k, v in edit.items():
            if v is DROP:
                meta.pop(k, None)
            else:
                meta[k] = v
    return meta


def write_dir(path, m, seed=0, matrix_type=G.BF16, predictor_type=None, assets="gguf", with_text=True, arch="qwen3", n_tokens=1000, version=3,
              talker_meta=None, pred_meta=None, talker_tensors=None, pred_tensors=None, asset_tensors=None):
    """The synthetic model `m` as a quant directory with full metadata. *_meta / *_tensors edit one file's metadata / tensors (see
    _apply): drop, retype (Typed) or falsify anything. assets: "gguf" or "npy" (the legacy layout, src/assets_manager.rs:267-300)."""
    os.makedirs(path, exist_ok=True)
    for talker, fname, me, te in ((True, TALKER, talker_meta, talker_tensors), (False, PRED, pred_meta, pred_tensors)):
        tens = _apply(_tensors(m, seed, "talker" if talker else "pred"), te)
        mt = matrix_type if (talker or predictor_type is None) else predictor_type
        write_gguf(os.path.join(path, fname), [(k, v, mt if np.asarray(v).ndim == 2 else G.F32) for k, v in tens.items()],
                   meta=_apply(tfm_meta(m, talker, arch, n_tokens), me), version=version)
    at = _apply(_tensors(m, seed, "assets", with_text), asset_tensors)
    if assets == "gguf":
        write_gguf(os.path.join(path, ASSETS), [(k, v, G.F32) for k, v in at.items()], meta={"general.architecture": "qwen3-tts-assets"}, version=version)
    else:
        names = {"proj.weight": "proj_weight.npy", "proj.bias": "proj_bias.npy", "text_embd": "text_embedding_projected.npy"}
        for k, v in at.items():
            np.save(os.path.join(path, names.get(k) or "codec_embedding_%s.npy" % k.split(".")[1]), v)
    return path


# ---- the call --------------------------------------------------------------------------------------------------------
def base_config():
    """A default config whose non-model and protocol fields all hold recognisable non-default values: the call must leave them alone."""
    cfg = _abi.default_config()
    cfg.device, cfg.max_batch, cfg.n_ctx, cfg.max_steps_cap, cfg.with_vocoder, cfg.synth_seed = 3, 7, 1024, 99, 0, 1234
    cfg.talker_q8_0, cfg.vocoder_flush_tail = 1, 1
    cfg.vocoder.n_layer, cfg.vocoder.lookahead_frames = 5, 2
    cfg.model.sample_limit, cfg.model.eos_code, cfg.model.tts_pad_id = 2000, 1999, 77
    return cfg


def call(model_dir, quant, cfg, path_cap=None, err_cap=1024, lib=None):
    """q3tts_config_from_model_dir -> (status, message, path buffer). path_cap: None = large enough."""
    lib = lib or _abi.load_library()
    md = os.fsencode(str(model_dir))
    buf = C.create_string_buffer(b"\x55" * ((len(md) + 32) if path_cap is None else max(path_cap, 1)))
    err = C.create_string_buffer(b"\x55" * max(err_cap, 1) + b"#")  # one guard byte past err_cap
    q = None if quant is None else quant.encode()
    rc = lib.q3tts_config_from_model_dir(md, q, C.byref(cfg), buf, len(buf) - 1 if path_cap is None else path_cap, err, err_cap)
    assert err.raw[max(err_cap, 1)] == ord("#"), "the call wrote past err_cap"
    if err_cap > 0:
        assert b"\0" in err.raw[:err_cap], "the message is not terminated inside err_cap"
    else:
        assert err.raw[0] == 0x55, "the call wrote into a buffer of err_cap 0"
    msg = err.value.decode("utf-8", "replace") if err_cap > 0 else ""
    return rc, msg, buf

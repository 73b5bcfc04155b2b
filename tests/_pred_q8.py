"""The decoder with a W8A8 Predictor (q3tts_engine_config.predictor_q8_0 = 2) on the CPU — test infrastructure.

The oracle can switch only its Talker to Q8_0 x Q8_0 (q3o_set_talker_q8a8); it exports every primitive its own layer code is made of.
This module restates that layer code (oracle/q3_oracle.c tfm_layers, head_row, q3o_generate) in numpy + ctypes calls of those exports
only, generic over the arithmetic as the C code is over tfm.a8, so that the Predictor can run it with a8 = True.
tests/test_pred_q8_cpu.py pins the restatement to the untouched oracle, bit for bit: generate() with a bf16 Predictor equals
q3o_generate, and layers() / head() with a8 = True on the Talker's matrices equal q3o_talker_prefill under q3o_set_talker_q8a8.
"""
import ctypes as C

import numpy as np

import _oracle as O


def _bf16_bits(w):
    """bf16-exact f32 values -> their bf16 bit patterns."""
    return (np.ascontiguousarray(w, dtype=np.float32).view(np.uint32) >> 16).astype(np.uint16)


def _round_bf16(x):
    """q3o_bf16 on finite f32 values: round to nearest even, as bit patterns."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7fff + ((u >> 16) & 1)) >> 16).astype(np.uint16)


class Mats:
    """One transformer's weights in the form layers() / head() multiply: per matrix either bf16 bits [N][K] (a8 = False) or ggml
    Q8_0 blocks (q int8 [N][K], d f16 bits [N][K/32]) (a8 = True). Names: qkv (rows q | k | v), o, gate, up, down per layer; head."""

    def __init__(self, L, d, Hq, Hkv, hd, F, theta, eps, a8):
        self.L, self.d, self.Hq, self.Hkv, self.hd, self.F, self.theta, self.eps, self.a8 = L, d, Hq, Hkv, hd, F, float(theta), float(eps), a8
        self.attn_norm, self.ffn_norm, self.qn, self.kn = [], [], [], []
        self.qkv, self.o, self.gate, self.up, self.down = [], [], [], [], []
        self.out_norm = None
        self.head = None
        self._gu = {}

    def gate_up(self, l):
        if l not in self._gu:
            g, u = self.gate[l], self.up[l]
            self._gu[l] = (np.concatenate([g[0], u[0]]), np.concatenate([g[1], u[1]])) if self.a8 else np.concatenate([g, u])
        return self._gu[l]

    def _mat(self, w=None, qd=None):
        if not self.a8:
            return _bf16_bits(w)
        if qd is not None:
            return (np.ascontiguousarray(qd[0], dtype=np.int8), np.ascontiguousarray(qd[1], dtype=np.uint16))
        return O.quantize_q8_0(w)   # ggml's reference rule on natural rows: a block = 32 consecutive input columns of one output row


def mats_from_model(om, talker, a8):
    """The oracle model's synthetic Talker (talker = True) or Predictor; a8: its matrices quantised by q3o_quantize_q8_0."""
    c = om.cfg
    if talker:
        m = Mats(c.t_n_layer, c.t_d_model, c.t_n_head, c.t_n_kv_head, c.t_head_dim, c.t_d_ffn, c.t_rope_theta, c.rms_eps, a8)
    else:
        m = Mats(c.p_n_layer, c.p_d_model, c.p_n_head, c.p_n_kv_head, c.p_head_dim, c.p_d_ffn, c.p_rope_theta, c.rms_eps, a8)
    for l in range(m.L):
        m.attn_norm.append(om.norm_weight(talker, l, 0, m.d)); m.ffn_norm.append(om.norm_weight(talker, l, 1, m.d))
        m.qn.append(om.norm_weight(talker, l, 2, m.hd)); m.kn.append(om.norm_weight(talker, l, 3, m.hd))
        m.qkv.append(m._mat(om.matrix(talker, l, 0))); m.o.append(m._mat(om.matrix(talker, l, 1)))
        m.gate.append(m._mat(om.matrix(talker, l, 2))); m.up.append(m._mat(om.matrix(talker, l, 3))); m.down.append(m._mat(om.matrix(talker, l, 4)))
    m.out_norm = om.norm_weight(talker, -1, 0, m.d)
    m.head = m._mat(om.matrix(talker, 0, 5))
    return m


def mats_from_tensors(cfg, tensors, blocks=None):
    """A W8A8 Predictor from llama.cpp-named tensors (what a qwen3_tts_predictor.gguf holds). blocks: name -> (q int8 [N][K], d f16 bits
    [N][K/32]) for matrices whose Q8_0 blocks are given (a Q8_0 file's own blocks); the others are quantised from `tensors`."""
    c = cfg
    m = Mats(c.p_n_layer, c.p_d_model, c.p_n_head, c.p_n_kv_head, c.p_head_dim, c.p_d_ffn, c.p_rope_theta, c.rms_eps, True)
    blocks = blocks or {}

    def one(name):
        return m._mat(tensors[name], blocks.get(name))

    def cat(names):
        parts = [one(n) for n in names]
        return (np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts]))
    for l in range(m.L):
        b = "blk.%d." % l
        m.attn_norm.append(np.asarray(tensors[b + "attn_norm.weight"], dtype=np.float32)); m.ffn_norm.append(np.asarray(tensors[b + "ffn_norm.weight"], dtype=np.float32))
        m.qn.append(np.asarray(tensors[b + "attn_q_norm.weight"], dtype=np.float32)); m.kn.append(np.asarray(tensors[b + "attn_k_norm.weight"], dtype=np.float32))
        m.qkv.append(cat([b + "attn_q.weight", b + "attn_k.weight", b + "attn_v.weight"])); m.o.append(one(b + "attn_output.weight"))
        m.gate.append(one(b + "ffn_gate.weight")); m.up.append(one(b + "ffn_up.weight")); m.down.append(one(b + "ffn_down.weight"))
    m.out_norm = np.asarray(tensors["output_norm.weight"], dtype=np.float32)
    m.head = one("output.weight")
    return m


def split_q8_0(raw, N, K):
    """block_q8_0 rows as a GGUF file holds them (f16 d + 32 int8 per block) -> (q int8 [N][K], d f16 bits [N][K/32])."""
    blk = (np.frombuffer(raw, dtype=np.uint8) if isinstance(raw, (bytes, bytearray, memoryview)) else np.asarray(raw, dtype=np.uint8)).reshape(N, K // 32, 34)
    d = np.ascontiguousarray(blk[:, :, :2]).view(np.uint16).reshape(N, K // 32)
    q = np.ascontiguousarray(blk[:, :, 2:]).view(np.int8).reshape(N, K)
    return q, d


# ---- the GEMM of one arithmetic: RAW of rows against one matrix (oracle bgemm_rows / bgemm_rows_a8) -----------------------------
def _raw(mats, xb, v, w, rows=None):
    """bf16: xb = the rows' bf16 operand bits; a8: v = the f32 rows the quantiser sees. rows: a row slice (lo, hi) of the matrix."""
    if mats.a8:
        q, d = w
        if rows is not None:
            q, d = q[rows[0]:rows[1]], d[rows[0]:rows[1]]
        aq, ad = O.quantize_q8_0_act(v)
        return O.bgemm_q8a8(aq, ad, q, d, None, mats.d, mats.eps, 0)["y"]
    if rows is not None:
        w = w[rows[0]:rows[1]]
    return O.bgemm(xb, w, None, mats.d, mats.eps, 0)["y"]


def _scale_rows(y, sc):
    return (y * np.asarray(sc, dtype=np.float32)[:, None]).astype(np.float32)


def _expf(x):
    L = O.lib()
    return np.array([L.q3o_expf(float(t)) for t in x.ravel()], dtype=np.float32).reshape(x.shape)


def _swiglu(g, u):
    one = np.float32(1.0)
    return ((g / (one + _expf(-g))) * u).astype(np.float32)


def _attention(mats, qkv, pos0, l, mrope):
    qkv = np.ascontiguousarray(qkv, dtype=np.float32)
    n = qkv.shape[0]
    out = np.zeros((n, mats.Hq * mats.hd), dtype=np.float32)
    sec = None if mrope is None else (C.c_int32 * 4)(*mrope)
    O.lib().q3o_attention(O.ptr(qkv, O.f32p), n, pos0, mats.Hq, mats.Hkv, mats.hd, O.ptr(np.ascontiguousarray(mats.qn[l]), O.f32p),
                          O.ptr(np.ascontiguousarray(mats.kn[l]), O.f32p), mats.eps, mats.theta, sec, O.ptr(out, O.f32p))
    return out


def layers(mats, rows, pos0, a8=None, mrope=None, cache=None):
    """tfm_layers (oracle/q3_oracle.c:653-705) over the rows [n][d] of one sequence at positions pos0 .. pos0 + n - 1. Returns the residual
    rows after the last block. cache: a list of per-layer lists holding the QKV rows of the sequence's earlier positions 0 .. pos0 - 1
    (extended in place); attention then runs over all rows of the sequence and the last n are taken. None: nothing cached (pos0 rows
    of zeros would be wrong: pos0 must then be 0 unless the caller wants positions to start there with an empty cache)."""
    assert a8 is None or a8 == mats.a8
    x = np.ascontiguousarray(rows, dtype=np.float32).copy()
    n, d, nt = x.shape[0], mats.d, mats.d // 16
    xb, ssp = O.norm_inputs(x, mats.attn_norm[0])
    for l in range(mats.L):
        sc = [O.row_scale(ssp[r], d, mats.eps) for r in range(n)]
        vf = (x * mats.attn_norm[l][None, :]).astype(np.float32) if mats.a8 else None   # a8: the quantiser sees v = x * nw in f32
        qkv = _scale_rows(_raw(mats, xb, vf, mats.qkv[l]), sc)
        if cache is not None:
            prev = cache[l]
            allrows = np.concatenate(prev + [qkv]) if prev else qkv
            p0 = pos0 - (allrows.shape[0] - n)
            att = _attention(mats, allrows, p0, l, mrope)[-n:]
            prev.append(qkv)
        else:
            att = _attention(mats, qkv, pos0, l, mrope)
        y = _raw(mats, None if mats.a8 else _round_bf16(att), att, mats.o[l])     # a8: the attention output stays f32 into the quantiser
        x = (x + y).astype(np.float32)
        xb, ssp = O.norm_inputs(x, mats.ffn_norm[l])
        sc = [O.row_scale(ssp[r], d, mats.eps) for r in range(n)]
        vf = (x * mats.ffn_norm[l][None, :]).astype(np.float32) if mats.a8 else None
        gu = _scale_rows(_raw(mats, xb, vf, mats.gate_up(l)), sc)   # (gate rows, then up rows, in one call: a GEMM's columns are independent)
        g, u = np.ascontiguousarray(gu[:, :mats.F]), np.ascontiguousarray(gu[:, mats.F:])
        h = _swiglu(g, u)                                                                # a8: h stays f32, the quantiser's input
        y = _raw(mats, None if mats.a8 else _round_bf16(h), h, mats.down[l])
        x = (x + y).astype(np.float32)
        nxt = mats.attn_norm[l + 1] if l + 1 < mats.L else mats.out_norm
        xb, ssp = O.norm_inputs(x, nxt)
    return x


def head(mats, xrow, col0, ncols, a8=None):
    """head_row (oracle/q3_oracle.c:936-956): final norm + columns [col0, col0 + ncols) of the head matrix on one residual row."""
    assert a8 is None or a8 == mats.a8
    x = np.ascontiguousarray(xrow, dtype=np.float32).reshape(1, -1)
    xb, ssp = O.norm_inputs(x, mats.out_norm)
    sc = O.row_scale(ssp[0], mats.d, mats.eps)
    v = (x * mats.out_norm[None, :]).astype(np.float32) if mats.a8 else None
    return _scale_rows(_raw(mats, xb, v, mats.head, rows=(col0, col0 + ncols)), [sc])[0]


def hidden(mats, xrow):
    """The standalone canonical RMSNorm of head_row's hidden_out (q3o_rmsnorm)."""
    x = np.ascontiguousarray(xrow, dtype=np.float32)
    out = np.zeros_like(x)
    O.lib().q3o_rmsnorm(O.ptr(x, O.f32p), x.size, O.ptr(np.ascontiguousarray(mats.out_norm), O.f32p), mats.eps, O.ptr(out, O.f32p))
    return out


def generate(om, pred, prompt, temperature=0.0, top_k=40, top_p=0.9, seed=0, max_steps=16, min_frames=0, force_eos_at=-1):
    """q3o_generate (oracle/q3_oracle.c:978-1019) with the Predictor `pred` (a Mats of either arithmetic). The Talker is the oracle
    model's own, in whichever mode the caller selected, through q3o_talker_prefill on the growing row list (the prompt's rows, then one
    feedback row per frame). Returns (codes [n_frames][n_codebooks], hit_eos)."""
    c, L = om.cfg, O.lib()
    dp, de, ncb, cbs = c.p_d_model, c.d_embed, c.n_codebooks, c.codebook_size
    rows = [np.ascontiguousarray(prompt, dtype=np.float32)]
    draws = np.zeros(max(max_steps, 1), dtype=np.float32)
    L.q3o_rng_f32(seed, draws.size, O.ptr(draws, O.f32p))
    n_draw = 0
    pad = np.zeros(de, dtype=np.float32)
    if c.tts_pad_id < c.text_vocab:
        L.q3o_text_embedding(om.h, c.tts_pad_id, O.ptr(pad, O.f32p))

    def codec(q, code):
        e = np.zeros(de, dtype=np.float32)
        L.q3o_codec_embedding(om.h, q, int(code), O.ptr(e, O.f32p))
        return e

    def project(x):
        y = np.zeros(dp, dtype=np.float32)
        L.q3o_project(om.h, O.ptr(np.ascontiguousarray(x, dtype=np.float32), O.f32p), O.ptr(y, O.f32p))
        return y
    codes, hit_eos = [], False
    hid, logits = om.talker_prefill(np.concatenate(rows))
    for step in range(max_steps):
        if force_eos_at >= 0 and step == force_eos_at:
            code0 = c.eos_code
        else:
            if step < min_frames and c.eos_code < c.sample_limit:
                logits[c.eos_code] = -np.inf
            r = 0.0
            if temperature > 0.0:
                r = float(draws[n_draw]); n_draw += 1
            code0 = L.q3o_sample(O.ptr(logits, O.f32p), c.sample_limit, temperature, top_k, top_p, r)
        if code0 == c.eos_code:
            hit_eos = True
            break
        frame = [code0]
        emb = codec(0, code0)
        pin = np.stack([project(hid), project(emb)])
        fb = (np.float32(0.0) + emb).astype(np.float32)
        cache = [[] for _ in range(pred.L)]   # the Predictor's cache lives for one frame: positions restart at 0
        px = layers(pred, pin, 0, cache=cache)
        pl = head(pred, px[1], 0, cbs)
        for q in range(1, ncb):
            mi = int(np.argmax(pl))           # greedy: the first maximum (`>` over ascending columns)
            frame.append(mi)
            emb = codec(q, mi)
            fb = (fb + emb).astype(np.float32)
            if q < ncb - 1:
                px = layers(pred, project(emb)[None, :], q + 1, cache=cache)
                pl = head(pred, px[0], q * cbs, cbs)
        codes.append(frame)
        fb = (fb + pad).astype(np.float32)
        rows.append(fb[None, :])
        hid, logits = om.talker_prefill(np.concatenate(rows))
    return np.array(codes, dtype=np.int32).reshape(-1, ncb), hit_eos

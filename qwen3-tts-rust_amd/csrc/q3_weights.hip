// q3_weights.hip — everything q3tts_engine_create puts on the device before the first request and never touches again: the two
// transformers' weights, KV caches and RoPE tables (q3_tfm_init) and the embedding tables, the projection and the pre-projected codec
// tables (q3_assets_init). Source: the reference's quant directory (src/tts/engine.rs:91-131), or seeded synthetic tensors.
#include "q3_engine.h"
#include "q3_gguf.h"

#include <cmath>
#include <cstdio>

// RoPE tables in double on the host (same formula the oracle restates)
void q3_rope_tables(int n_pos, int hd, float theta, const int* sections, std::vector<float>& cs, std::vector<float>& sn) {
    const int half = hd / 2;
    int s3 = half;
    if (sections) s3 = sections[0] + sections[1] + sections[2];
    cs.resize((size_t)n_pos * half); sn.resize((size_t)n_pos * half);
    for (int p = 0; p < n_pos; ++p)
        for (int i = 0; i < half; ++i) {
            const double inv = pow((double)theta, -2.0 * (double)i / (double)hd);
            const double ang = (i < s3) ? (double)p * inv : 0.0;
            cs[(size_t)p * half + i] = (float)cos(ang);
            sn[(size_t)p * half + i] = (float)sin(ang);
        }
}

// ---- real weights: llama.cpp's tensor names for the qwen3 architecture --------------------------
// (the staging buffers regrow and live for one q3_tfm_init: their own hipMalloc / hipFree, not q3_dalloc)
struct GgSrc {
    q3tts_engine* e; const Q3Gguf* g; const char* file;
    std::vector<uint16_t> host; uint16_t* dev[2] = {nullptr, nullptr}; size_t dev_cap[2] = {0, 0};
    ~GgSrc() { for (auto p : dev) if (p) hipFree(p); for (auto p : dev8) if (p) hipFree(p); }
    int fail(const std::string& msg) { return q3_set_err(e, Q3TTS_ERR_INVALID, std::string(file) + ": " + msg); }
    const Q3GgufTensor* need(const std::string& name, uint64_t ne0, uint64_t ne1, int* rc) {
        const Q3GgufTensor* t = g->find(name);
        if (!t) { *rc = fail("tensor '" + name + "' is missing"); return nullptr; }
        const uint64_t d1 = t->dims.size() > 1 ? t->dims[1] : 1;
        if (t->dims[0] != ne0 || d1 != ne1 || t->dims.size() > 2) {
            *rc = fail("tensor '" + name + "' has shape [" + std::to_string(d1) + "][" + std::to_string(t->dims[0]) + "], the configuration needs [" +
                       std::to_string(ne1) + "][" + std::to_string(ne0) + "]");
            return nullptr;
        }
        *rc = Q3TTS_OK;
        return t;
    }
    // f32 vector -> device
    int vec(const std::string& name, size_t n, float* dst) {
        int rc; const Q3GgufTensor* t = need(name, n, 1, &rc);
        if (!t) return rc;
        std::vector<float> h(n); std::string err;
        if (q3_gguf_to_f32(*t, h.data(), err)) return fail(err);
        Q3_HIP(e, hipMemcpy(dst, h.data(), n * 4, hipMemcpyHostToDevice));  // (h is a local: synchronous copy)
        return Q3TTS_OK;
    }
    // Q8_0 mode: a tensor stored as Q8_0 goes to the device as it is ([N][K/32] blocks of 34 bytes) into staging buffer `which`
    // (raw[which] = true); any other type is widened to bf16 as below and quantised on the device
    uint8_t* dev8[2] = {nullptr, nullptr}; size_t dev8_cap[2] = {0, 0}; bool raw[2] = {false, false};
    int mat_q8(const std::string& name, size_t N, size_t K, int which) {
        int rc; const Q3GgufTensor* t = need(name, K, N, &rc);
        if (!t) return rc;
        raw[which] = false;
        if (t->type != Q3_GGML_Q8_0) return mat(name, N, K, which);
        const size_t bytes = N * (K / 32) * 34;
        if (t->nbytes < bytes) return fail("tensor '" + name + "' is shorter than its Q8_0 shape");
        if (dev8_cap[which] < bytes) {
            if (dev8[which]) hipFree(dev8[which]);
            dev8[which] = nullptr; dev8_cap[which] = 0;
            void* p = nullptr;
            if (hipMalloc(&p, bytes) != hipSuccess) return q3_set_err(e, Q3TTS_ERR_OOM, "hipMalloc (Q8_0 staging)");
            dev8[which] = (uint8_t*)p; dev8_cap[which] = bytes;
        }
        Q3_HIP(e, hipMemcpy(dev8[which], t->data, bytes, hipMemcpyHostToDevice));
        raw[which] = true;
        return Q3TTS_OK;
    }
    // [N][K] matrix -> bf16 row-major staging buffer `which` on the device
    int mat(const std::string& name, size_t N, size_t K, int which) {
        int rc; const Q3GgufTensor* t = need(name, K, N, &rc);
        if (!t) return rc;
        host.resize(N * K); std::string err;
        if (q3_gguf_to_bf16(*t, host.data(), err)) return fail(err);
        if (dev_cap[which] < N * K) {
            if (dev[which]) hipFree(dev[which]);
            dev[which] = nullptr; dev_cap[which] = 0;
            void* p = nullptr;
            if (hipMalloc(&p, N * K * 2) != hipSuccess) return q3_set_err(e, Q3TTS_ERR_OOM, "hipMalloc (weight staging)");
            dev[which] = (uint16_t*)p; dev_cap[which] = N * K;
        }
        Q3_HIP(e, hipMemcpy(dev[which], host.data(), N * K * 2, hipMemcpyHostToDevice));
        return Q3TTS_OK;
    }
    // staging slot i as a Q3Fill source pair: the Q8_0 blocks as stored (raw: only mat_q8 sets it), else the bf16 rows
    void source(int i, const uint16_t** src, const uint8_t** src8) const { *src = raw[i] ? nullptr : dev[i]; *src8 = raw[i] ? dev8[i] : nullptr; }
};

int q3_tfm_init(q3tts_engine* e, Q3Tfm& t, const Q3TfmShape& sh, const Q3Gguf* g, const char* file, int q8mode) {
    const bool q8 = q8mode != 0;
    const int grp = sh.grp, L = sh.L, d = sh.d, hd = sh.hd, F = sh.F;
    t.L = L; t.d = d; t.Hq = sh.Hq; t.Hkv = sh.Hkv; t.hd = hd; t.F = F; t.nq = sh.Hq * hd; t.nkv = sh.Hkv * hd; t.nqkv = t.nq + 2 * t.nkv;
    t.head_n = sh.head_n; t.q8 = q8; t.a8 = q8mode == 2;
    GgSrc src{e, g, file};
    GgSrc* gg = g ? &src : nullptr;
    const uint64_t seed = e->cfg.synth_seed;
    const float ms = 0.02f / Q3_IH4_STD, ns = 0.05f / Q3_IH4_STD;
    hipStream_t s = e->stream;
    t.attn_norm.resize(L); t.ffn_norm.resize(L); t.qn.resize(L); t.kn.resize(L);
    t.wqkv.resize(L); t.wo.resize(L); t.wgu.resize(L); t.wd.resize(L);
    if (q8) { t.sqkv.assign(L, nullptr); t.so.assign(L, nullptr); t.sgu.assign(L, nullptr); t.sd.assign(L, nullptr); }
    // a matrix [N][K]: bf16 tiles (2 bytes per weight), or in Q8_0 mode block quants (1 byte) + f16 block scales [N][K/32]
    const size_t wdiv = q8 ? 16 : 8;  // weights per uint4
    auto alloc_mat = [&](uint4** w, uint16_t** sc, size_t N, size_t K) -> int {
        TRY(q3_dalloc(e, w, N * K / wdiv));
        if (q8) TRY(q3_dalloc(e, sc, N * K / 32));
        return Q3TTS_OK;
    };
    auto fill = [&](Q3Fill& f, uint16_t* sc) { if (q8) { f.dst_scale = sc; q3_launch_fill_tiled_q8(f, s); } else q3_launch_fill_tiled(f, s); };
    auto stage = [&](const std::string& name, size_t N, size_t K, int which) -> int { return q8 ? gg->mat_q8(name, N, K, which) : gg->mat(name, N, K, which); };
    // rows [row0, row0 + rows) of dst [Ntot][K] <- the file's tensor `name` (through staging slot 0, which the next tensor reuses)
    auto put = [&](const std::string& name, uint4* dst, uint16_t* sc, int Ntot, int K, int row0, int rows) -> int {
        TRY(stage(name, rows, K, 0));
        Q3Fill f{}; f.dst = dst; f.N = Ntot; f.K = K; f.mode = 0; f.row0 = row0; f.rows = rows;
        gg->source(0, &f.src_a, &f.src8_a);
        fill(f, sc);
        Q3_HIP(e, hipStreamSynchronize(s));
        return Q3TTS_OK;
    };
    const double bpw = q8 ? 1.0625 : 2.0;  // bytes per weight streamed by a GEMM
    for (int l = 0; l < L; ++l) {
        TRY(q3_dalloc(e, &t.attn_norm[l], (size_t)d)); TRY(q3_dalloc(e, &t.ffn_norm[l], (size_t)d));
        TRY(q3_dalloc(e, &t.qn[l], (size_t)hd)); TRY(q3_dalloc(e, &t.kn[l], (size_t)hd));
        uint16_t *sc_qkv = nullptr, *sc_o = nullptr, *sc_gu = nullptr, *sc_d = nullptr;
        TRY(alloc_mat(&t.wqkv[l], &sc_qkv, t.nqkv, d)); TRY(alloc_mat(&t.wo[l], &sc_o, d, t.nq));
        TRY(alloc_mat(&t.wgu[l], &sc_gu, (size_t)2 * F, d)); TRY(alloc_mat(&t.wd[l], &sc_d, d, F));
        if (q8) { t.sqkv[l] = sc_qkv; t.so[l] = sc_o; t.sgu[l] = sc_gu; t.sd[l] = sc_d; }
        t.weight_bytes += (size_t)(bpw * (double)((size_t)t.nqkv * d + (size_t)d * t.nq + 3ull * F * d));
        if (gg) {  // blk.N.* of a llama.cpp qwen3 GGUF (weights [out][in], NeoX RoPE: no q/k permutation)
            const std::string b = "blk." + std::to_string(l) + ".";
            Q3_HIP(e, hipStreamSynchronize(s));
            TRY(gg->vec(b + "attn_norm.weight", d, t.attn_norm[l])); TRY(gg->vec(b + "ffn_norm.weight", d, t.ffn_norm[l]));
            TRY(gg->vec(b + "attn_q_norm.weight", hd, t.qn[l])); TRY(gg->vec(b + "attn_k_norm.weight", hd, t.kn[l]));
            TRY(put(b + "attn_q.weight", t.wqkv[l], sc_qkv, t.nqkv, d, 0, t.nq));
            TRY(put(b + "attn_k.weight", t.wqkv[l], sc_qkv, t.nqkv, d, t.nq, t.nkv));
            TRY(put(b + "attn_v.weight", t.wqkv[l], sc_qkv, t.nqkv, d, t.nq + t.nkv, t.nkv));
            TRY(put(b + "attn_output.weight", t.wo[l], sc_o, d, t.nq, 0, d));
            TRY(stage(b + "ffn_gate.weight", F, d, 0)); TRY(stage(b + "ffn_up.weight", F, d, 1));
            Q3Fill f{}; f.dst = t.wgu[l]; f.N = 2 * F; f.K = d; f.mode = 1; f.row0 = 0; f.rows = d;
            gg->source(0, &f.src_a, &f.src8_a); gg->source(1, &f.src_b, &f.src8_b);
            if (gg->raw[0] != gg->raw[1]) return gg->fail("ffn_gate / ffn_up of block " + std::to_string(l) + " differ in type (one Q8_0, one not)");
            fill(f, sc_gu);
            Q3_HIP(e, hipStreamSynchronize(s));
            TRY(put(b + "ffn_down.weight", t.wd[l], sc_d, d, F, 0, d));
            continue;
        }
        q3_launch_fill_f32(t.attn_norm[l], d, seed, Q3_TID(grp, l, Q3W_ATTN_NORM), 1.0f, ns, 0, s);
        q3_launch_fill_f32(t.ffn_norm[l], d, seed, Q3_TID(grp, l, Q3W_FFN_NORM), 1.0f, ns, 0, s);
        q3_launch_fill_f32(t.qn[l], hd, seed, Q3_TID(grp, l, Q3W_QNORM), 1.0f, ns, 0, s);
        q3_launch_fill_f32(t.kn[l], hd, seed, Q3_TID(grp, l, Q3W_KNORM), 1.0f, ns, 0, s);
        Q3Fill f{}; f.seed = seed; f.scale = ms;
        f.dst = t.wqkv[l]; f.N = t.nqkv; f.K = d; f.mode = 0;
        f.row0 = 0; f.rows = t.nq; f.tid_a = Q3_TID(grp, l, Q3W_Q); fill(f, sc_qkv);
        f.row0 = t.nq; f.rows = t.nkv; f.tid_a = Q3_TID(grp, l, Q3W_K); fill(f, sc_qkv);
        f.row0 = t.nq + t.nkv; f.rows = t.nkv; f.tid_a = Q3_TID(grp, l, Q3W_V); fill(f, sc_qkv);
        f.dst = t.wo[l]; f.N = d; f.K = t.nq; f.row0 = 0; f.rows = d; f.tid_a = Q3_TID(grp, l, Q3W_O); fill(f, sc_o);
        f.dst = t.wgu[l]; f.N = 2 * F; f.K = d; f.mode = 1; f.tid_a = Q3_TID(grp, l, Q3W_GATE); f.tid_b = Q3_TID(grp, l, Q3W_UP);
        fill(f, sc_gu);
        f.dst = t.wd[l]; f.N = d; f.K = F; f.mode = 0; f.row0 = 0; f.rows = d; f.tid_a = Q3_TID(grp, l, Q3W_DOWN); fill(f, sc_d);
    }
    TRY(q3_dalloc(e, &t.out_norm, (size_t)d));
    TRY(alloc_mat(&t.head, &t.shead, (size_t)t.head_n, d));
    t.weight_bytes += (size_t)(bpw * (double)((size_t)t.head_n * d));
    if (gg) {
        Q3_HIP(e, hipStreamSynchronize(s));
        TRY(gg->vec("output_norm.weight", d, t.out_norm));
        TRY(put("output.weight", t.head, t.shead, t.head_n, d, 0, t.head_n));
    } else {
        q3_launch_fill_f32(t.out_norm, d, seed, Q3_TID(grp, Q3_L_MODEL, Q3WM_OUT_NORM), 1.0f, ns, 0, s);
        Q3Fill f{}; f.seed = seed; f.scale = ms; f.dst = t.head; f.N = t.head_n; f.K = d; f.mode = 0; f.row0 = 0; f.rows = t.head_n;
        f.tid_a = Q3_TID(grp, Q3_L_MODEL, Q3WM_HEAD); fill(f, t.shead);
    }
    Q3KvCache& c = t.cache; c.n_ctx = sh.n_ctx; c.n_slots = sh.n_slots;
    c.layer_stride = (size_t)c.n_slots * t.Hkv * c.n_ctx * hd;
    c.kv8 = sh.kv8 != 0;
    if (c.kv8) {  // Q8_0 cache: per element one byte of quants + 1/16 byte of f16 block scales, the scales behind the quants in one allocation
        int8_t *kq = nullptr, *vq = nullptr;
        const size_t nq = c.layer_stride * L;
        TRY(q3_dalloc(e, &kq, nq + nq / 16)); TRY(q3_dalloc(e, &vq, nq + nq / 16));
        c.kc = (uint16_t*)kq; c.vc = (uint16_t*)vq; c.kd = (uint16_t*)(kq + nq); c.vd = (uint16_t*)(vq + nq);
    } else {
    TRY(q3_dalloc(e, &c.kc, c.layer_stride * L)); TRY(q3_dalloc(e, &c.vc, c.layer_stride * L));
    }
    std::vector<float> cs, sn;
    q3_rope_tables(c.n_ctx, hd, sh.theta, sh.sections, cs, sn);
    TRY(q3_dalloc(e, &t.cs, cs.size())); TRY(q3_dalloc(e, &t.sn, sn.size()));
    Q3_HIP(e, hipMemcpyAsync(t.cs, cs.data(), cs.size() * 4, hipMemcpyHostToDevice, s));
    Q3_HIP(e, hipMemcpyAsync(t.sn, sn.data(), sn.size() * 4, hipMemcpyHostToDevice, s));
    Q3_HIP(e, hipStreamSynchronize(s));
    return Q3TTS_OK;
}

// ---- assets (F32 tables like qwen3_assets.gguf: src/assets_manager.rs:212-241) -----------------------------------------
static bool file_exists(const std::string& p) { FILE* f = fopen(p.c_str(), "rb"); if (f) fclose(f); return f != nullptr; }
static int upload_table(q3tts_engine* e, float** dst, const float* host, size_t n) {
    TRY(q3_dalloc(e, dst, n));
    Q3_HIP(e, hipMemcpy(*dst, host, n * 4, hipMemcpyHostToDevice));  // `host` may be a temporary of the caller: synchronous copy
    return Q3TTS_OK;
}
static int upload_proj(q3tts_engine* e, const float* w, const float* b) {  // proj.weight stays f32 (src/assets_manager.rs:212-241, :383-399)
    const q3tts_model_config& m = e->cfg.model;
    TRY(upload_table(e, &e->proj_w, w, (size_t)m.p_d_model * m.d_embed));
    return upload_table(e, &e->proj_b, b, (size_t)m.p_d_model);
}
// Assets::load (src/assets_manager.rs:14-26): qwen3_assets.gguf if present, else the NPY files. Table row counts come from
// the files (they define the out-of-range rules, :419-460); a missing text table means "every id is out of range".
static int load_assets_files(q3tts_engine* e, const std::string& dir) {
    q3tts_model_config& m = e->cfg.model;
    const size_t d = (size_t)m.d_embed;
    std::vector<std::vector<float>> tabs(1 + m.n_codebooks);  // text, codec 0..
    std::vector<size_t> rows(1 + m.n_codebooks, 0);
    std::vector<float> pw, pb;
    std::string err;
    const std::string gpath = dir + "/qwen3_assets.gguf";
    if (file_exists(gpath)) {
        Q3Gguf g;
        if (g.open(gpath, err)) return q3_set_err(e, Q3TTS_ERR_INVALID, err);
        auto fetch = [&](const std::string& name, uint64_t ne0, bool required, std::vector<float>& out, size_t* nrows) -> int {
            const Q3GgufTensor* t = g.find(name);
            if (!t) return required ? q3_set_err(e, Q3TTS_ERR_INVALID, gpath + ": " + name + " (tensor) missing") : Q3TTS_OK;
            if (t->dims[0] != ne0 || t->dims.size() > 2) return q3_set_err(e, Q3TTS_ERR_INVALID, gpath + ": tensor '" + name + "' has the wrong row length");
            out.resize(t->nelem);
            if (q3_gguf_to_f32(*t, out.data(), err)) return q3_set_err(e, Q3TTS_ERR_INVALID, gpath + ": " + err);
            if (nrows) *nrows = t->dims.size() > 1 ? (size_t)t->dims[1] : 1;
            return Q3TTS_OK;
        };
        size_t pr = 0;
        TRY(fetch("proj.weight", d, true, pw, &pr));
        if (pr != (size_t)m.p_d_model) return q3_set_err(e, Q3TTS_ERR_INVALID, gpath + ": proj.weight does not have p_d_model rows");
        TRY(fetch("proj.bias", (uint64_t)m.p_d_model, true, pb, nullptr));
        TRY(fetch("text_embd", d, false, tabs[0], &rows[0]));
        for (int q = 0; q < m.n_codebooks; ++q) TRY(fetch("codec_embd." + std::to_string(q), d, true, tabs[1 + q], &rows[1 + q]));
    } else {
        auto fetch = [&](const std::string& file, bool required, std::vector<float>& out, size_t* nrows, size_t row_len) -> int {
            const std::string path = dir + "/" + file;
            if (!file_exists(path)) return required ? q3_set_err(e, Q3TTS_ERR_INVALID, "neither qwen3_assets.gguf nor " + file + " in " + dir) : Q3TTS_OK;
            std::vector<size_t> shape;
            if (q3_npy_load_f32(path, out, shape, err)) return q3_set_err(e, Q3TTS_ERR_INVALID, err);
            if (out.size() % row_len) return q3_set_err(e, Q3TTS_ERR_INVALID, path + ": size is not a multiple of the row length");
            if (nrows) *nrows = out.size() / row_len;
            return Q3TTS_OK;
        };
        size_t pr = 0, br = 0;
        TRY(fetch("proj_weight.npy", true, pw, &pr, d));
        TRY(fetch("proj_bias.npy", true, pb, &br, 1));
        if (pr != (size_t)m.p_d_model || br != (size_t)m.p_d_model) return q3_set_err(e, Q3TTS_ERR_INVALID, dir + ": projection shape does not match p_d_model");
        TRY(fetch("text_embedding_projected.npy", false, tabs[0], &rows[0], d));
        for (int q = 0; q < m.n_codebooks; ++q) TRY(fetch("codec_embedding_" + std::to_string(q) + ".npy", true, tabs[1 + q], &rows[1 + q], d));
    }
    for (int q = 2; q < m.n_codebooks; ++q)
        if (rows[1 + q] != rows[2]) return q3_set_err(e, Q3TTS_ERR_INVALID, dir + ": codec tables 1.." + std::to_string(m.n_codebooks - 1) + " differ in size");
    m.text_vocab = (int32_t)rows[0]; m.codec0_rows = (int32_t)rows[1];
    if (m.n_codebooks > 1) m.codecq_rows = (int32_t)rows[2];
    if (rows[0]) TRY(upload_table(e, &e->text, tabs[0].data(), tabs[0].size()));
    for (int q = 0; q < m.n_codebooks; ++q) TRY(upload_table(e, &e->codec[q], tabs[1 + q].data(), tabs[1 + q].size()));
    TRY(upload_proj(e, pw.data(), pb.data()));
    // tts_pad = row 151671 of the text table when it is that large, else zeros (src/assets_manager.rs:244-249)
    if ((size_t)m.tts_pad_id < rows[0]) e->tts_pad = e->text + (size_t)m.tts_pad_id * d;
    else TRY(q3_dalloc(e, &e->tts_pad, d));
    return Q3TTS_OK;
}
// the same members from seeded fills (values bf16-representable like every synthetic matrix; proj_w f32 [out][in])
static int fill_assets_synthetic(q3tts_engine* e) {
    const q3tts_model_config& m = e->cfg.model;
    const uint64_t seed = e->cfg.synth_seed;
    const float es = 0.05f / Q3_IH4_STD, ps = 0.02f / Q3_IH4_STD;
    hipStream_t s = e->stream;
    TRY(q3_dalloc(e, &e->text, (size_t)m.text_vocab * m.d_embed));
    q3_launch_fill_f32(e->text, (size_t)m.text_vocab * m.d_embed, seed, Q3_TID(Q3G_ASSET, 0, Q3WA_TEXT), 0.0f, es, 1, s);
    for (int q = 0; q < m.n_codebooks; ++q) {
        const size_t rows = q == 0 ? m.codec0_rows : m.codecq_rows;
        TRY(q3_dalloc(e, &e->codec[q], rows * m.d_embed));
        q3_launch_fill_f32(e->codec[q], rows * m.d_embed, seed, Q3_TID(Q3G_ASSET, 1 + q, 0), 0.0f, es, 1, s);
    }
    TRY(q3_dalloc(e, &e->proj_w, (size_t)m.p_d_model * m.d_embed));
    q3_launch_fill_f32(e->proj_w, (size_t)m.p_d_model * m.d_embed, seed, Q3_TID(Q3G_ASSET, 0, Q3WA_PROJ_W), 0.0f, ps, 1, s);
    TRY(q3_dalloc(e, &e->proj_b, (size_t)m.p_d_model));
    q3_launch_fill_f32(e->proj_b, m.p_d_model, seed, Q3_TID(Q3G_ASSET, 0, Q3WA_PROJ_B), 0.0f, ps, 0, s);
    e->tts_pad = e->text + (size_t)m.tts_pad_id * m.d_embed;  // src/assets_manager.rs:244-249
    return Q3TTS_OK;
}

int q3_assets_init(q3tts_engine* e, const std::string& wdir) {
    const q3tts_model_config& m = e->cfg.model;  // (table row counts follow the files when wdir is given)
    hipStream_t s = e->stream;
    e->codec.assign(m.n_codebooks, nullptr);
    TRY(wdir.empty() ? fill_assets_synthetic(e) : load_assets_files(e, wdir));
    TRY(q3_dalloc(e, &e->codec_dev, 16));
    Q3_HIP(e, hipMemcpyAsync((void*)e->codec_dev, e->codec.data(), sizeof(float*) * m.n_codebooks, hipMemcpyHostToDevice, s));
    // pre-projected codec tables: proj(codec_q[code]) for every code, computed once with the projection kernel (a row's result
    // does not depend on the other rows, so a table row equals the on-the-fly projection bit for bit): the 15 Predictor passes
    // after the first read their input with a gather instead of a projection launch each
    e->pproj.assign(m.n_codebooks, nullptr);
    for (int q = 0; q < m.n_codebooks; ++q) {
        const int rows = q == 0 ? m.codec0_rows : m.codecq_rows;
        TRY(q3_dalloc(e, &e->pproj[q], (size_t)rows * m.p_d_model));
        Q3Project pj{}; pj.x = e->codec[q]; pj.ldx = m.d_embed; pj.rows = rows; pj.w = e->proj_w; pj.bias = e->proj_b; pj.n_in = m.d_embed; pj.n_out = m.p_d_model;
        pj.y = e->pproj[q]; pj.ldy = m.p_d_model;
        q3_launch_project(pj, s);
    }
    Q3_HIP(e, hipStreamSynchronize(s));
    return Q3TTS_OK;
}

// ---- the Predictor's layer-0 QKV table --------------------------------------------------------------------------------
// In passes 1 .. n_codebooks - 2 of the greedy Predictor the first block's input is no computed activation but a row of pproj[q] (or
// proj_b), chosen by the code of the pass before: block 0's raw q / k / v are a function of (q, code) and of the weights alone. They are
// computed here once, with the decode path's own kernels — q3_norm_out on every element of the row, as k_pred_next applies it, then
// the QKV GEMM descriptor of q3_run_layers with its STORE epilogue pointed at the table — so a table row holds the bits the two launches
// left in sc.qkv (a GEMM row depends on no other row, and every k_bgemm instance computes the one canonical order).
// Q3TTS_PRED_TABLE=0: no table. Q3TTS_PRED_TABLE_MAX_MB (default 1024): a larger table is not built. Both read here, once per engine.
int q3_pred_table_init(q3tts_engine* e) {
    const q3tts_model_config& m = e->cfg.model;
    const Q3Tfm& P = e->P;
    const int nq = m.n_codebooks - 2, rows = m.codecq_rows, R = rows + 1, dp = m.p_d_model;
    if (const char* ev = getenv("Q3TTS_PRED_TABLE")) if (!atoi(ev)) return Q3TTS_OK;
    if (P.a8 || nq < 1 || rows < 1) return Q3TTS_OK;
    {   // the gathering form exists for k_attend_small<2> only: a Predictor whose decode attention is another kernel keeps its launches
        Q3Attend at{}; at.hd = P.hd; at.Hq = P.Hq; at.Hkv = P.Hkv; at.fused = 1; at.n_ctx = P.cache.n_ctx;
        if (q3_attend_pick(at) != Q3_ATT_SMALL2 || (m.d_embed & 3) || (dp & 3)) return Q3TTS_OK;
    }
    long long max_mb = 1024;
    if (const char* ev = getenv("Q3TTS_PRED_TABLE_MAX_MB")) max_mb = atoll(ev);
    const size_t n = (size_t)nq * R * P.nqkv;
    if ((double)n * 4.0 > (double)max_mb * 1048576.0) return Q3TTS_OK;
    TRY(q3_dalloc(e, &e->qkv0, n));
    // the rows' norm inputs: staging that lives for this call (its own hipMalloc / hipFree pair)
    const size_t r16 = ((size_t)R + 15) & ~(size_t)15;
    struct Stage { void* p = nullptr; ~Stage() { if (p) hipFree(p); } } xb, ssp;
    if (hipMalloc(&xb.p, r16 * dp * 2) != hipSuccess || hipMalloc(&ssp.p, (size_t)R * (dp / 16) * 4) != hipSuccess)
        return q3_set_err(e, Q3TTS_ERR_OOM, "hipMalloc (Predictor QKV table staging)");
    hipStream_t s = e->stream;
    Q3_HIP(e, hipMemsetAsync(xb.p, 0, r16 * dp * 2, s));
    Q3Rows r{}; r.xb = (uint16_t*)xb.p; r.ssp = (float*)ssp.p;
    for (int q = 1; q <= nq; ++q) {
        q3_launch_pred_table_rows(e->pproj[q], rows, e->proj_b, dp, P.attn_norm[0], r.xb, r.ssp, s);
        Q3Scratch sc{}; sc.qkv = e->qkv0 + (size_t)(q - 1) * R * P.nqkv;
        if (q3_launch_gemm(e, P, q3_gemm_qkv(P, 0, r, sc, R, m.rms_eps, 0), s))
            return q3_set_err(e, Q3TTS_ERR_INVALID, "Predictor QKV table: the GEMM launch was refused for this model shape");
    }
    Q3_HIP(e, hipGetLastError());
    Q3_HIP(e, hipStreamSynchronize(s));
    return Q3TTS_OK;
}

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
    int mat_q8(const std::string& name, size_t N, size_t K, int which) { return mat_blocks(name, N, K, which, Q3_GGML_Q8_0, 34); }
    // MXFP4 mode: the same for a tensor stored as MXFP4 (ggml type 39: [N][K/32] blocks of 17 bytes)
    int mat_mx4(const std::string& name, size_t N, size_t K, int which) { return mat_blocks(name, N, K, which, Q3_GGML_MXFP4, 17); }
    int mat_blocks(const std::string& name, size_t N, size_t K, int which, uint32_t type, size_t block_bytes) {
        int rc; const Q3GgufTensor* t = need(name, K, N, &rc);
        if (!t) return rc;
        raw[which] = false;
        if (t->type != type) return mat(name, N, K, which);
        const size_t bytes = N * (K / 32) * block_bytes;
        if (t->nbytes < bytes) return fail("tensor '" + name + "' is shorter than its block shape");
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
    // K-quant resident mode: the tensor's super-blocks as stored into staging buffer `which` (the caller has checked type and shape)
    int raw_k(const Q3GgufTensor& t, int which) {
        if (dev8_cap[which] < t.nbytes) {
            if (dev8[which]) hipFree(dev8[which]);
            dev8[which] = nullptr; dev8_cap[which] = 0;
            void* p = nullptr;
            if (hipMalloc(&p, t.nbytes) != hipSuccess) return q3_set_err(e, Q3TTS_ERR_OOM, "hipMalloc (K-quant staging)");
            dev8[which] = (uint8_t*)p; dev8_cap[which] = t.nbytes;
        }
        Q3_HIP(e, hipMemcpy(dev8[which], t.data, t.nbytes, hipMemcpyHostToDevice));
        return Q3TTS_OK;
    }
    // [N][K] matrix -> bf16 row-major staging buffer `which` on the device
    int mat(const std::string& name, size_t N, size_t K, int which) {
        int rc; const Q3GgufTensor* t = need(name, K, N, &rc);
        if (!t) return rc;
        raw[which] = false;  // (the slot may have held a tensor's blocks: with talker_mxfp4 the head follows MXFP4 matrices through slot 0)
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

// ---- K-quant resident matrices (q3tts_engine_options.kquant_resident; q3_bgemmk.hip) -----------------------------------
// A matrix of the engine is one or more file tensors stacked by rows (q | k | v), or two interleaved 8 + 8 inside every tile (gate / up).
// It stays quantised when every part is Q4_K / Q5_K / Q6_K with whole tile rows and K % 512 == 0 — interleaved parts of one type, since a
// tile row has one type. Anything else is bf16 as before, silently. which: 0 QKV, 1 O, 2 gate / up, 3 down, 4 the head(s).
struct KqPart { std::string name; int rows; };
struct KqSpec { std::vector<KqPart> parts; int K; bool interleave; };
static KqSpec kq_spec(const Q3TfmShape& sh, int l, int which) {
    const std::string b = "blk." + std::to_string(l) + ".";
    const int nq = sh.Hq * sh.hd, nkv = sh.Hkv * sh.hd;
    switch (which) {
        case 0: return {{{b + "attn_q.weight", nq}, {b + "attn_k.weight", nkv}, {b + "attn_v.weight", nkv}}, sh.d, false};
        case 1: return {{{b + "attn_output.weight", sh.d}}, nq, false};
        case 2: return {{{b + "ffn_gate.weight", sh.F}, {b + "ffn_up.weight", sh.F}}, sh.d, true};
        case 3: return {{{b + "ffn_down.weight", sh.d}}, sh.F, false};
        default: return {{{"output.weight", sh.head_n}}, sh.d, false};
    }
}
static int kq_type_of(uint32_t ggml) { return ggml == Q3_GGML_Q4_K ? Q3_KQ_Q4 : ggml == Q3_GGML_Q5_K ? Q3_KQ_Q5 : ggml == Q3_GGML_Q6_K ? Q3_KQ_Q6 : -1; }
// the parts' types and the matrix's tiled bytes when it qualifies
static bool kq_plan(const Q3Gguf& g, const KqSpec& sp, std::vector<int>* types, size_t* bytes) {
    types->clear(); *bytes = 0;
    if (sp.K < 512 || sp.K % 512) return false;
    for (const KqPart& p : sp.parts) {
        const Q3GgufTensor* t = g.find(p.name);
        const int ty = t ? kq_type_of(t->type) : -1;
        if (ty < 0 || !t->data || t->dims.size() != 2 || t->dims[0] != (uint64_t)sp.K || t->dims[1] != (uint64_t)p.rows) return false;
        if (p.rows % (sp.interleave ? 8 : 16)) return false;
        if (sp.interleave && !types->empty() && ty != (*types)[0]) return false;
        types->push_back(ty);
        *bytes += (size_t)p.rows * (sp.K >> 6) * q3_kq_pair_bytes(ty) / 16;
    }
    return true;
}
size_t q3_tfm_kq_saving(const Q3TfmShape& sh, const Q3Gguf& g) {
    size_t saved = 0;
    std::vector<int> types; size_t bytes;
    auto one = [&](int l, int which) {
        const KqSpec sp = kq_spec(sh, l, which);
        if (!kq_plan(g, sp, &types, &bytes)) return;
        size_t n = 0;
        for (const KqPart& p : sp.parts) n += (size_t)p.rows;
        saved += 2 * n * sp.K - bytes;
    };
    for (int l = 0; l < sh.L; ++l) for (int w = 0; w < 4; ++w) one(l, w);
    one(0, 4);
    return saved;
}

size_t q3_tfm_mx_saving(const Q3TfmShape& sh, int mx) {
    const size_t nq = (size_t)sh.Hq * sh.hd, nqkv = nq + 2 * (size_t)sh.Hkv * sh.hd;
    size_t n = 0;  // weights that leave bf16
    if (q3_mx4_ok(sh.d)) n += (nqkv + 2 * (size_t)sh.F) * sh.d;
    if (q3_mx4_ok((int)nq)) n += (size_t)sh.d * nq;
    if (q3_mx4_ok(sh.F)) n += (size_t)sh.d * sh.F;
    return (size_t)sh.L * (2 * n - (mx == 2 ? q3_mx8_bytes(n, 1) : q3_mx4_bytes(n, 1)));
}

int q3_tfm_init(q3tts_engine* e, Q3Tfm& t, const Q3TfmShape& sh, const Q3Gguf* g, const char* file, int q8mode, int kq, int mx) {
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
    // talker_mxfp4 (mx = 1) / talker_mxfp8 (mx = 2): a block matrix with whole 128-steps is 17 / 33 bytes per 32 weights in the tiled MX /
    // MX8 layout; the others stay bf16
    if (mx) { t.mx_d = q3_mx4_ok(d) ? mx : 0; t.mx_nq = q3_mx4_ok(sh.Hq * hd) ? mx : 0; t.mx_F = q3_mx4_ok(F) ? mx : 0; }
    auto is_mx = [&](size_t K) { return mx && q3_mx4_ok((int)K); };
    auto mx_bytes = [&](size_t N, size_t K) { return mx == 2 ? q3_mx8_bytes(N, K) : q3_mx4_bytes(N, K); };
    auto alloc_mat = [&](uint4** w, uint16_t** sc, size_t N, size_t K) -> int {
        if (is_mx(K) && w != &t.head) { uint8_t* p = nullptr; TRY(q3_dalloc(e, &p, mx_bytes(N, K))); *w = (uint4*)p; return Q3TTS_OK; }
        TRY(q3_dalloc(e, w, N * K / wdiv));
        if (q8) TRY(q3_dalloc(e, sc, N * K / 32));
        return Q3TTS_OK;
    };
    auto fill = [&](Q3Fill& f, uint16_t* sc) {
        if (is_mx(f.K) && f.dst != t.head) {  // quantised on the device from the bf16 rows / the synthetic tensor (ggml's quantize_row_mxfp4)
            Q3FillMx m{}; m.dst = (uint8_t*)f.dst; m.N = f.N; m.K = f.K; m.mode = f.mode; m.row0 = f.row0; m.rows = f.rows; m.tid_a = f.tid_a; m.tid_b = f.tid_b;
            m.seed = f.seed; m.scale = f.scale; m.src_a = f.src_a; m.src_b = f.src_b; m.src4_a = f.src8_a; m.src4_b = f.src8_b;  // (a type-39 tensor: its blocks as stored)
            if (mx == 2) q3_launch_fill_tiled_mx8(m, s);  // (MXFP8: always from the bf16 staging rows; no tensor type is taken as stored)
            else q3_launch_fill_tiled_mx4(m, s);
        } else if (q8) { f.dst_scale = sc; q3_launch_fill_tiled_q8(f, s); } else q3_launch_fill_tiled(f, s);
    };
    auto stage = [&](const std::string& name, size_t N, size_t K, int which, bool mxdst) -> int {
        return mxdst && mx == 1 ? gg->mat_mx4(name, N, K, which) : (q8 ? gg->mat_q8(name, N, K, which) : gg->mat(name, N, K, which));
    };
    // rows [row0, row0 + rows) of dst [Ntot][K] <- the file's tensor `name` (through staging slot 0, which the next tensor reuses)
    auto put = [&](const std::string& name, uint4* dst, uint16_t* sc, int Ntot, int K, int row0, int rows) -> int {
        TRY(stage(name, rows, K, 0, is_mx(K) && dst != t.head));
        Q3Fill f{}; f.dst = dst; f.N = Ntot; f.K = K; f.mode = 0; f.row0 = row0; f.rows = rows;
        gg->source(0, &f.src_a, &f.src8_a);
        fill(f, sc);
        Q3_HIP(e, hipStreamSynchronize(s));
        return Q3TTS_OK;
    };
    const double bpw = q8 ? 1.0625 : 2.0;  // bytes per weight streamed by a GEMM
    t.kqkv.assign(L, {}); t.ko.assign(L, {}); t.kgu.assign(L, {}); t.kdn.assign(L, {});
    // Matrix `which` of block l: kept quantised when it qualifies (*w = the tiled K layout, *k its table; returns its bytes through *res),
    // else *res = 0 and nothing is done. The relayout runs on the device from the file's super-blocks (staging slots 0 / 1).
    auto resident = [&](int l, int which, uint4** w, Q3Tfm::Kq* k, size_t* res) -> int {
        *res = 0;
        if (!kq || !gg || q8) return Q3TTS_OK;
        const KqSpec sp = kq_spec(sh, l, which);
        std::vector<int> types; size_t bytes;
        if (!kq_plan(*g, sp, &types, &bytes)) return Q3TTS_OK;
        uint8_t* dst = nullptr;
        TRY(q3_dalloc(e, &dst, bytes));
        std::vector<uint2> tab;
        size_t off = 0;
        if (sp.interleave) {
            TRY(gg->raw_k(*g->find(sp.parts[0].name), 0)); TRY(gg->raw_k(*g->find(sp.parts[1].name), 1));
            Q3FillKq f{}; f.dst = dst; f.K = sp.K; f.type = types[0]; f.ntr = (sp.parts[0].rows + sp.parts[1].rows) / 16; f.mode = 1;
            f.src_a = gg->dev8[0]; f.src_b = gg->dev8[1];
            q3_launch_fill_tiled_kq(f, s);
            for (int r = 0; r < f.ntr; ++r) tab.push_back(make_uint2((uint32_t)((size_t)r * q3_kq_row_bytes(types[0], sp.K) / 16), (uint32_t)types[0]));
            Q3_HIP(e, hipStreamSynchronize(s));
            t.fmt_bytes[1 + types[0]] += bytes;
        } else
            for (size_t i = 0; i < sp.parts.size(); ++i) {
                TRY(gg->raw_k(*g->find(sp.parts[i].name), 0));
                Q3FillKq f{}; f.dst = dst + off; f.K = sp.K; f.type = types[i]; f.ntr = sp.parts[i].rows / 16; f.src_a = gg->dev8[0];
                q3_launch_fill_tiled_kq(f, s);
                const size_t rb = q3_kq_row_bytes(types[i], sp.K);
                for (int r = 0; r < f.ntr; ++r) tab.push_back(make_uint2((uint32_t)((off + (size_t)r * rb) / 16), (uint32_t)types[i]));
                Q3_HIP(e, hipStreamSynchronize(s));  // (the staging slot is reused by the next part)
                off += (size_t)f.ntr * rb; t.fmt_bytes[1 + types[i]] += (size_t)f.ntr * rb;
            }
        void* dtab = nullptr;
        if (hipMalloc(&dtab, tab.size() * sizeof(uint2)) != hipSuccess) return q3_set_err(e, Q3TTS_ERR_OOM, "hipMalloc (K-quant tile-row table)");
        e->allocs.push_back(dtab);
        Q3_HIP(e, hipMemcpy(dtab, tab.data(), tab.size() * sizeof(uint2), hipMemcpyHostToDevice));
        *w = (uint4*)dst; k->tab = (const uint2*)dtab; k->bpp = (int)(bytes / (tab.size() * (size_t)(sp.K >> 6)));
        *res = bytes;
        return Q3TTS_OK;
    };
    for (int l = 0; l < L; ++l) {
        TRY(q3_dalloc(e, &t.attn_norm[l], (size_t)d)); TRY(q3_dalloc(e, &t.ffn_norm[l], (size_t)d));
        TRY(q3_dalloc(e, &t.qn[l], (size_t)hd)); TRY(q3_dalloc(e, &t.kn[l], (size_t)hd));
        uint16_t *sc_qkv = nullptr, *sc_o = nullptr, *sc_gu = nullptr, *sc_d = nullptr;
        size_t r_qkv, r_o, r_gu, r_d;  // bytes of the matrices kept as K-quants (0: bf16 / Q8_0 as before)
        if (gg) Q3_HIP(e, hipStreamSynchronize(s));
        TRY(resident(l, 0, &t.wqkv[l], &t.kqkv[l], &r_qkv)); TRY(resident(l, 1, &t.wo[l], &t.ko[l], &r_o));
        TRY(resident(l, 2, &t.wgu[l], &t.kgu[l], &r_gu)); TRY(resident(l, 3, &t.wd[l], &t.kdn[l], &r_d));
        if (!r_qkv) TRY(alloc_mat(&t.wqkv[l], &sc_qkv, t.nqkv, d));
        if (!r_o) TRY(alloc_mat(&t.wo[l], &sc_o, d, t.nq));
        if (!r_gu) TRY(alloc_mat(&t.wgu[l], &sc_gu, (size_t)2 * F, d));
        if (!r_d) TRY(alloc_mat(&t.wd[l], &sc_d, d, F));
        if (q8) { t.sqkv[l] = sc_qkv; t.so[l] = sc_o; t.sgu[l] = sc_gu; t.sd[l] = sc_d; }
        {
            auto mb = [&](size_t N, size_t K) { return is_mx(K) ? mx_bytes(N, K) : (size_t)(bpw * (double)(N * K)); };
            const size_t b_qkv = r_qkv ? r_qkv : mb(t.nqkv, d), b_o = r_o ? r_o : mb(d, t.nq);
            const size_t b_gu = r_gu ? r_gu : mb(2ull * F, d), b_d = r_d ? r_d : mb(d, F);
            if (mx) {  // (never together with Q8_0 or K-quants) the MXFP4 / MXFP8 matrices are counted apart from the bf16 ones
                const size_t m4 = (t.mx_d ? b_qkv + b_gu : 0) + (t.mx_nq ? b_o : 0) + (t.mx_F ? b_d : 0);
                t.mx_bytes += m4; t.fmt_bytes[0] -= m4;
            }
            t.weight_bytes += b_qkv + b_o + b_gu + b_d;
            t.fmt_bytes[0] += (r_qkv ? 0 : b_qkv) + (r_o ? 0 : b_o) + (r_gu ? 0 : b_gu) + (r_d ? 0 : b_d);
            if (l == 0) t.qkv0_bytes = b_qkv;
        }
        if (gg) {  // blk.N.* of a llama.cpp qwen3 GGUF (weights [out][in], NeoX RoPE: no q/k permutation)
            const std::string b = "blk." + std::to_string(l) + ".";
            Q3_HIP(e, hipStreamSynchronize(s));
            TRY(gg->vec(b + "attn_norm.weight", d, t.attn_norm[l])); TRY(gg->vec(b + "ffn_norm.weight", d, t.ffn_norm[l]));
            TRY(gg->vec(b + "attn_q_norm.weight", hd, t.qn[l])); TRY(gg->vec(b + "attn_k_norm.weight", hd, t.kn[l]));
            if (!r_qkv) {
            TRY(put(b + "attn_q.weight", t.wqkv[l], sc_qkv, t.nqkv, d, 0, t.nq));
            TRY(put(b + "attn_k.weight", t.wqkv[l], sc_qkv, t.nqkv, d, t.nq, t.nkv));
            TRY(put(b + "attn_v.weight", t.wqkv[l], sc_qkv, t.nqkv, d, t.nq + t.nkv, t.nkv));
            }
            if (!r_o) TRY(put(b + "attn_output.weight", t.wo[l], sc_o, d, t.nq, 0, d));
            if (!r_gu) {
            TRY(stage(b + "ffn_gate.weight", F, d, 0, is_mx(d))); TRY(stage(b + "ffn_up.weight", F, d, 1, is_mx(d)));
            Q3Fill f{}; f.dst = t.wgu[l]; f.N = 2 * F; f.K = d; f.mode = 1; f.row0 = 0; f.rows = d;
            gg->source(0, &f.src_a, &f.src8_a); gg->source(1, &f.src_b, &f.src8_b);
            if (gg->raw[0] != gg->raw[1]) return gg->fail("ffn_gate / ffn_up of block " + std::to_string(l) + " differ in type (one kept as blocks, one not)");
            fill(f, sc_gu);
            Q3_HIP(e, hipStreamSynchronize(s));
            }
            if (!r_d) TRY(put(b + "ffn_down.weight", t.wd[l], sc_d, d, F, 0, d));
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
    size_t r_head;
    if (gg) Q3_HIP(e, hipStreamSynchronize(s));
    TRY(resident(0, 4, &t.head, &t.khead, &r_head));
    if (!r_head) TRY(alloc_mat(&t.head, &t.shead, (size_t)t.head_n, d));
    t.head_bytes = r_head ? r_head : (size_t)(bpw * (double)((size_t)t.head_n * d));
    t.weight_bytes += t.head_bytes;
    if (!r_head) t.fmt_bytes[0] += t.head_bytes;
    if (gg) {
        Q3_HIP(e, hipStreamSynchronize(s));
        TRY(gg->vec("output_norm.weight", d, t.out_norm));
        if (!r_head) TRY(put("output.weight", t.head, t.shead, t.head_n, d, 0, t.head_n));
    } else {
        q3_launch_fill_f32(t.out_norm, d, seed, Q3_TID(grp, Q3_L_MODEL, Q3WM_OUT_NORM), 1.0f, ns, 0, s);
        Q3Fill f{}; f.seed = seed; f.scale = ms; f.dst = t.head; f.N = t.head_n; f.K = d; f.mode = 0; f.row0 = 0; f.rows = t.head_n;
        f.tid_a = Q3_TID(grp, Q3_L_MODEL, Q3WM_HEAD); fill(f, t.shead);
    }
    Q3KvCache& c = t.cache; c.n_ctx = sh.n_ctx; c.n_slots = sh.n_slots;
    c.layer_stride = (size_t)c.n_slots * t.Hkv * c.n_ctx * hd;
    c.kv8 = sh.kv8 != 0; c.kv4 = sh.kv4;
    if (sh.kv_pages > 0) {  // paged: a pool of kv_pages + 1 pages per layer (page 0 stays zero) and the slots' table, all zero = nothing owned
        c.n_pages = sh.kv_pages; c.tbl_stride = c.n_ctx / 64;
        c.layer_stride = (size_t)(c.n_pages + 1) * t.Hkv * 64 * hd;
        TRY(q3_dalloc(e, &c.tbl, (size_t)c.n_slots * c.tbl_stride));
    }
    if (c.kv8) {  // Q8_0 cache: per element one byte of quants + 1/16 byte of f16 block scales, the scales behind the quants in one allocation
        int8_t *kq = nullptr, *vq = nullptr;
        const size_t nq = c.layer_stride * L;
        const size_t nk = q3_kv4_bytes(c.kv4, 0, nq), nv = q3_kv4_bytes(c.kv4, 1, nq);  // (a Q4_0 side: half a byte of quants per element)
        TRY(q3_dalloc(e, &kq, nk + nq / 16)); TRY(q3_dalloc(e, &vq, nv + nq / 16));
        c.kc = (uint16_t*)kq; c.vc = (uint16_t*)vq; c.kd = (uint16_t*)(kq + nk); c.vd = (uint16_t*)(vq + nv);
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

// q3_engine.hip — host side of libq3tts: errors, configuration and validation, the footprint, engine creation and teardown, the setters
// and the prompt builder: the engine part of the C ABI of include/q3tts.h (prefill and voice prefixes: q3_admit.hip; the continuous batching loop:
// q3_generate.hip; weights and assets: q3_weights.hip; the transformers' launches and the frame step: q3_layers.hip; the kernel-level
// test hooks q3tts_k_*: q3_hooks.hip).
#include "q3_engine.h"
#include "q3_gguf.h"

#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>

static thread_local std::string g_err;

int q3_set_err(q3tts_engine* e, int code, const std::string& msg) {
    if (e) { std::lock_guard<std::mutex> lk(e->err_mu); e->err = msg; }
    g_err = msg;
    return code;
}
extern "C" const char* q3tts_last_error(const q3tts_engine* e) {
    if (!e) return g_err.c_str();
    if (!e->session.load()) return e->err.c_str();
    static thread_local std::string copy;  // a session worker may set e->err meanwhile: the caller reads its own copy
    std::lock_guard<std::mutex> lk(const_cast<q3tts_engine*>(e)->err_mu);
    copy = e->err;
    return copy.c_str();
}
int q3_refuse_in_session(q3tts_engine* e) {
    return q3_set_err(e, Q3TTS_ERR_STATE, "the engine is owned by an open session (q3tts_session_close first)");
}

// ------------------------------------------------------------------------------------------------
// configuration
// ------------------------------------------------------------------------------------------------
extern "C" void q3tts_default_config(q3tts_engine_config* c) {
    memset(c, 0, sizeof(*c));
    q3tts_model_config& m = c->model;
    m.t_n_layer = 28; m.t_d_model = 2048; m.t_n_head = 16; m.t_n_kv_head = 8; m.t_head_dim = 128; m.t_d_ffn = 6144;
    m.t_vocab = 3072; m.t_rope_theta = 1000000.0f;
    m.t_mrope_sections[0] = 24; m.t_mrope_sections[1] = 20; m.t_mrope_sections[2] = 20; m.t_mrope_sections[3] = 0;
    m.p_n_layer = 5; m.p_d_model = 1024; m.p_n_head = 16; m.p_n_kv_head = 8; m.p_head_dim = 128; m.p_d_ffn = 3072;
    m.p_rope_theta = 1000000.0f;
    m.n_codebooks = 16; m.codebook_size = 2048; m.rms_eps = 1e-6f;
    m.d_embed = 2048; m.text_vocab = 151936; m.codec0_rows = 3072; m.codecq_rows = 2048;
    m.sample_limit = 2160; m.eos_code = 2150; m.tts_pad_id = 151671;
    q3tts_vocoder_config& v = c->vocoder;
    v.n_codebooks = 16; v.codebook_size = 2048; v.codebook_dim = 512; v.latent_dim = 1024; v.pre_conv_kernel = 3;
    v.n_layer = 8; v.n_head = 16; v.head_dim = 64; v.d_ffn = 3072; v.sliding_window = 72;
    v.rope_theta = 10000.0f; v.rms_eps = 1e-5f; v.layer_scale_init = 0.01f;
    v.n_upsample = 2; v.upsample_ratios[0] = 2; v.upsample_ratios[1] = 2;
    v.decoder_dim = 1536; v.n_dec_blocks = 4;
    v.dec_rates[0] = 8; v.dec_rates[1] = 5; v.dec_rates[2] = 4; v.dec_rates[3] = 3;
    v.lookahead_frames = 0; v.sample_rate = 24000;
    c->device = 0; c->max_batch = 1; c->n_ctx = 4096; c->max_steps_cap = 512; c->with_vocoder = 1;
    c->synth_seed = 0; c->weights_path = nullptr; c->talker_q8_0 = 0; c->vocoder_flush_tail = 0; c->predictor_q8_0 = 0; c->kv_q8_0 = 0;
}

static int validate(const q3tts_engine_config& c, std::string& why) {
    const q3tts_model_config& m = c.model;
#define REQ(cond) do { if (!(cond)) { why = "config check failed: " #cond; return Q3TTS_ERR_INVALID; } } while (0)
    REQ(m.t_n_layer > 0 && m.p_n_layer > 0);
    REQ(m.t_head_dim == 128 && m.p_head_dim == 128);  // exact attention kernel: 16 lanes x 8 dims per key
    REQ(m.t_d_model % 512 == 0 && m.p_d_model % 512 == 0 && m.t_d_ffn % 512 == 0 && m.p_d_ffn % 512 == 0);
    REQ(m.t_d_model <= 8192 && m.p_d_model <= 8192);  // fused RMSNorm: a wave's share of the norm weights is one LDS strip of <= 1024 floats
    REQ((m.t_n_head * m.t_head_dim) % 512 == 0 && (m.p_n_head * m.p_head_dim) % 512 == 0);
    REQ(m.t_n_head > 0 && m.t_n_kv_head > 0 && m.p_n_head > 0 && m.p_n_kv_head > 0);
    REQ(m.t_n_head % m.t_n_kv_head == 0 && m.p_n_head % m.p_n_kv_head == 0);
    // the attention kernels serve 1, 2 or 4 query heads per KV head (spelled with the fields, so that the message names them)
    REQ(m.t_n_head == m.t_n_kv_head || m.t_n_head == 2 * m.t_n_kv_head || m.t_n_head == 4 * m.t_n_kv_head);
    REQ(m.p_n_head == m.p_n_kv_head || m.p_n_head == 2 * m.p_n_kv_head || m.p_n_head == 4 * m.p_n_kv_head);
    REQ(m.t_vocab % 16 == 0 && m.codebook_size % 16 == 0 && m.t_d_ffn % 8 == 0);
    REQ(m.d_embed == m.t_d_model);  // feedback row feeds the Talker directly (src/tts/engine.rs:631)
    REQ(m.d_embed % 512 == 0);
    REQ(m.n_codebooks >= 2 && m.n_codebooks <= 16);
    REQ(m.sample_limit > 0 && m.sample_limit <= m.t_vocab && m.sample_limit <= 4096);
    REQ(m.t_mrope_sections[0] + m.t_mrope_sections[1] + m.t_mrope_sections[2] + m.t_mrope_sections[3] == m.t_head_dim / 2);
    REQ(m.tts_pad_id >= 0 && (c.weights_path || m.tts_pad_id < m.text_vocab));  // with weights_path the text table's row count is the file's (0 without one: tts_pad is then zeros)
    REQ(c.max_batch >= 1 && c.max_batch <= Q3TTS_MAX_BATCH);
    REQ(c.n_ctx >= 64 && c.n_ctx % 64 == 0 && c.n_ctx <= 8192);
    REQ(c.max_steps_cap >= 1 && c.max_steps_cap < c.n_ctx);
    REQ(m.n_codebooks + 1 <= 64);
    REQ(c.talker_q8_0 >= 0 && c.talker_q8_0 <= 2);
    if (c.talker_q8_0) REQ(m.t_d_model % 512 == 0 && m.t_d_ffn % 512 == 0 && (m.t_n_head * m.t_head_dim) % 512 == 0);  // Q8_0: an even number of 32-blocks per K slice
    if (c.talker_q8_0 == 2) REQ(m.t_vocab % 32 == 0 && ((m.t_n_head + 2 * m.t_n_kv_head) * m.t_head_dim) % 32 == 0 && m.t_d_ffn % 64 == 0);  // W8A8: whole 32-column blocks per workgroup
    REQ(c.predictor_q8_0 >= 0 && c.predictor_q8_0 <= 2);
    REQ(c.kv_q8_0 == 0 || c.kv_q8_0 == 1);
    if (c.predictor_q8_0 == 2) {  // W8A8 Predictor: an even number of 32-blocks per K slice, whole 32-column blocks per workgroup
        REQ(m.p_d_model % 512 == 0); REQ(m.p_d_ffn % 512 == 0); REQ((m.p_n_head * m.p_head_dim) % 512 == 0);
        REQ(m.codebook_size % 32 == 0); REQ(((m.p_n_head + 2 * m.p_n_kv_head) * m.p_head_dim) % 32 == 0); REQ(m.p_d_ffn % 64 == 0);
    }
#undef REQ
    return Q3TTS_OK;
}

// Row buckets of an engine with max_batch slots (host only; also the test hook q3tts_k_row_buckets): 1, 2, 4, 8, then the multiples of 16
// (the GEMM's row tiles are 16 wide: a 48-row step costs 3/4 of a 64-row one) up to 64; above 64 the multiples of 32 (a frame step is
// captured per bucket x Predictor variant x text form: capture time and graph memory grow with the count — 14 sets at 256 slots, not 20);
// last max_batch itself. For max_batch <= 64 this is the list the engine always had.
static void row_buckets(int nb, std::vector<int>& out) {
    out.clear();
    for (int r = 1; r < nb && r < 16; r *= 2) out.push_back(r);
    for (int r = 16; r < nb && r <= 64; r += 16) out.push_back(r);
    for (int r = 96; r < nb; r += 32) out.push_back(r);
    out.push_back(nb);
}
extern "C" int q3tts_k_row_buckets(int32_t max_batch, int32_t* out, int32_t cap) {
    if (max_batch < 1 || max_batch > Q3TTS_MAX_BATCH || !out) return q3_set_err(nullptr, Q3TTS_ERR_INVALID, "row buckets: max_batch outside 1..256 or null output");
    std::vector<int> b;
    row_buckets(max_batch, b);
    if ((int)b.size() > cap) return q3_set_err(nullptr, Q3TTS_ERR_INVALID, "row buckets: output too small");
    for (size_t i = 0; i < b.size(); ++i) out[i] = b[i];
    return (int)b.size();
}

// The device bytes an engine of this config allocates for what the config alone sizes (include/q3tts.h, "memory"): the two transformers'
// weights and caches, the per-slot decode state, the lane's and the prefill's rows and scratch, the vocoder's per-slot state. A lower
// bound of the real total (tables, the vocoder's weights and work buffers, RoPE tables are left out): it refuses only what cannot fit.
static unsigned long long tfm_weight_bytes(int L, int d, int Hq, int Hkv, int hd, int F, int head_n, int q8) {
    const unsigned long long per = (unsigned long long)d * (Hq + 2 * Hkv) * hd + (unsigned long long)Hq * hd * d + 3ull * d * F;
    const unsigned long long n = per * L + (unsigned long long)head_n * d;
    return q8 ? n + n / 16 : 2 * n;  // Q8_0: 34 bytes per 32 weights
}
static unsigned long long engine_footprint(const q3tts_engine_config& c) {
    const q3tts_model_config& m = c.model;
    const unsigned long long B = c.max_batch, nctx = c.n_ctx, cap = c.max_steps_cap;
    unsigned long long t = tfm_weight_bytes(m.t_n_layer, m.t_d_model, m.t_n_head, m.t_n_kv_head, m.t_head_dim, m.t_d_ffn, m.t_vocab, c.talker_q8_0) +
                           tfm_weight_bytes(m.p_n_layer, m.p_d_model, m.p_n_head, m.p_n_kv_head, m.p_head_dim, m.p_d_ffn, (m.n_codebooks - 1) * m.codebook_size, c.predictor_q8_0);
    // Talker KV: bf16, or (kv_q8_0) Q8_0 blocks — 2 * t_n_layer * t_n_kv_head * n_ctx * (t_head_dim + 2 * t_head_dim / 32) bytes per slot
    if (c.kv_q8_0) t += B * 2ull * m.t_n_layer * m.t_n_kv_head * nctx * (m.t_head_dim + 2ull * m.t_head_dim / 32);
    else t += B * 2ull * m.t_n_layer * m.t_n_kv_head * m.t_head_dim * nctx * 2;
    t += B * 2ull * m.p_n_layer * m.p_n_kv_head * m.p_head_dim * 64 * 2;    // Predictor cache (64 positions, one frame)
    t += B * cap * 4ull * (m.n_codebooks + 1 + (m.n_codebooks - 1));        // codes, rng, prng
    t += B * 4ull * ((m.sample_limit + 31) / 32 + cap + 2ull * m.t_vocab + 2ull * m.t_d_model);  // seen, streamed text ids, the parked and the lane's logits / rows
    const unsigned long long nqkv = std::max((m.t_n_head + 2 * m.t_n_kv_head) * m.t_head_dim, (m.p_n_head + 2 * m.p_n_kv_head) * m.p_head_dim);
    const unsigned long long nq = std::max(m.t_n_head * m.t_head_dim, m.p_n_head * m.p_head_dim), F = std::max(m.t_d_ffn, m.p_d_ffn);
    t += 2 * B * (4 * nqkv + 2 * nq + 2 * F) + B * 6ull * m.t_d_model + 2 * B * 6ull * m.p_d_model;  // lane scratch and rows
    t += nctx * (4ull * (m.t_n_head + 2 * m.t_n_kv_head) * m.t_head_dim + 2ull * m.t_n_head * m.t_head_dim + 2ull * m.t_d_ffn + 6ull * m.t_d_model);  // prefill scratch and rows
    if (c.with_vocoder) {
        const q3tts_vocoder_config& v = c.vocoder;
        unsigned long long spf = 1;
        for (int i = 0; i < v.n_upsample; ++i) spf *= v.upsample_ratios[i];
        for (int i = 0; i < v.n_dec_blocks; ++i) spf *= v.dec_rates[i];
        t += B * cap * spf * 4;                                                           // PCM rows
        t += B * 2ull * v.n_layer * v.sliding_window * v.n_head * v.head_dim * 4;        // attention rings
    }
    return t;
}

extern "C" int q3tts_k_engine_footprint(const q3tts_engine_config* cfg, int64_t* bytes) {
    std::string why;
    if (!cfg || !bytes) return q3_set_err(nullptr, Q3TTS_ERR_INVALID, "null argument");
    if (validate(*cfg, why) != Q3TTS_OK) return q3_set_err(nullptr, Q3TTS_ERR_INVALID, why);
    *bytes = (int64_t)engine_footprint(*cfg);
    return Q3TTS_OK;
}

// Zero-filled device memory. The fill has COMPLETED when the pointer is handed out: an upload on any stream (the null stream, the
// vocoder stream, a caller's) can never be overtaken by it. (Rounds 1 and 2 filled asynchronously on e->stream, a non-blocking stream,
// and patched three call sites whose uploads were zeroed again; the allocator is the one place to close that race.)
int q3_dev_alloc_zeroed(q3tts_engine* e, void** p, size_t bytes) {
    void* q = nullptr;
    hipError_t err = hipMalloc(&q, bytes);
    if (err != hipSuccess) return q3_set_err(e, Q3TTS_ERR_OOM, std::string("hipMalloc: ") + hipGetErrorString(err));
    err = hipMemsetAsync(q, 0, bytes, e->stream);
    if (err == hipSuccess) err = hipStreamSynchronize(e->stream);
    if (err != hipSuccess) { hipFree(q); return q3_set_err(e, Q3TTS_ERR_DEVICE, std::string("hipMemset: ") + hipGetErrorString(err)); }
    if (e) e->dev_bytes += bytes;
    *p = q;
    return Q3TTS_OK;
}
extern "C" int q3tts_k_bucket_steps(const q3tts_engine* e, int64_t* out, int32_t cap) {
    if (!e || !out || cap < (int)e->bucket_steps.size()) return q3_set_err(nullptr, Q3TTS_ERR_INVALID, "bucket steps: null argument or output too small");
    for (size_t i = 0; i < e->bucket_steps.size(); ++i) out[i] = e->bucket_steps[i].load(std::memory_order_relaxed);
    return (int)e->bucket_steps.size();
}
extern "C" int q3tts_k_prefix_stats(const q3tts_engine* e, int64_t* out2) {
    if (!e || !out2) return q3_set_err(nullptr, Q3TTS_ERR_INVALID, "null argument");
    out2[0] = e->kvp_launches.load(std::memory_order_relaxed); out2[1] = e->kvp_group_max.load(std::memory_order_relaxed);
    return Q3TTS_OK;
}
extern "C" int q3tts_get_vocoder_source(const q3tts_engine* e, int32_t* source) {
    if (!e || !source) return q3_set_err(nullptr, Q3TTS_ERR_INVALID, "null argument");
    *source = e->voc_source;
    return Q3TTS_OK;
}
extern "C" int q3tts_k_device_bytes(const q3tts_engine* e, int64_t* bytes) {
    if (!e || !bytes) return q3_set_err(nullptr, Q3TTS_ERR_INVALID, "null argument");
    *bytes = (int64_t)e->dev_bytes;
    return Q3TTS_OK;
}
static int alloc_scratch(q3tts_engine* e, Q3Scratch& sc, int rows, int nqkv, int nq, int F) {
    sc.rows = rows;
    const size_t r16 = ((size_t)rows + 15) & ~(size_t)15;  // A-tiled buffers hold whole 16-row tiles
    TRY(q3_dalloc(e, &sc.qkv, (size_t)rows * nqkv)); TRY(q3_dalloc(e, &sc.att, r16 * nq)); TRY(q3_dalloc(e, &sc.h, r16 * F));
    sc.rt16 = (int)(r16 / 16);
    if (e->T.a8 || e->P.a8) { TRY(q3_dalloc(e, &sc.asc_att, r16 * (nq / 32))); TRY(q3_dalloc(e, &sc.asc_h, r16 * (F / 32))); }  // W8A8 (either model; nq / F are the larger of the two): block scales of both operands
    return Q3TTS_OK;
}

// `rows` residual rows of width d with their norm inputs (the A-tiled operand holds whole 16-row tiles); scales: the W8A8 block scales too
static int alloc_rows(q3tts_engine* e, Q3Rows& r, size_t rows, int d, bool scales) {
    const size_t r16 = (rows + 15) & ~(size_t)15;
    TRY(q3_dalloc(e, &r.x, rows * d)); TRY(q3_dalloc(e, &r.xb, r16 * d)); TRY(q3_dalloc(e, &r.ssp, rows * (d / 16)));
    r.rt16 = (int)(r16 / 16);
    if (scales) TRY(q3_dalloc(e, &r.ascale, r16 * (d / 32)));
    return Q3TTS_OK;
}

extern "C" int q3tts_engine_create(const q3tts_engine_config* cfg, q3tts_engine** out) {
    if (!cfg || !out) return q3_set_err(nullptr, Q3TTS_ERR_INVALID, "null argument");
    std::string why;
    if (validate(*cfg, why) != Q3TTS_OK) return q3_set_err(nullptr, Q3TTS_ERR_INVALID, why);
    if (cfg->predictor_q8_0 == 1)
        return q3_set_err(nullptr, Q3TTS_ERR_UNSUPPORTED, "predictor_q8_0 = 1 (Q8_0 weights x bf16 activations) is not implemented for the Predictor: use 0 (bf16) or 2 (Q8_0 x Q8_0)");
    // what the Q8_0-cache kernels (q3_attend_kv8.hip) cannot run is refused here, not at the first launch. (Today validate() above admits
    // no such shape — it already holds t_head_dim to 128, the GQA ratio to 1, 2, 4 and n_ctx to whole key blocks for every engine — so this
    // cannot be reached through the ABI yet; it is the place a wider validate() falls back on. The launcher's own refusals are tested
    // through q3tts_k_attend_pick_kv8.)
    if (cfg->kv_q8_0) {
        const q3tts_model_config& mm = cfg->model;
        Q3Attend pa{}; pa.kv8 = 1; pa.hd = mm.t_head_dim; pa.Hq = mm.t_n_head; pa.Hkv = mm.t_n_kv_head; pa.n_ctx = cfg->n_ctx;
        const int R = mm.t_n_head / mm.t_n_kv_head;
        const bool prefill_ok = q3_attend_pick_kv8(pa) != Q3_ATT_REFUSED;
        pa.fused = R >= 2 ? 1 : 0;
        if (!prefill_ok || q3_attend_pick_kv8(pa) == Q3_ATT_REFUSED || mm.t_head_dim % 32 || cfg->n_ctx % 64)
            return q3_set_err(nullptr, Q3TTS_ERR_UNSUPPORTED, "kv_q8_0 = 1: the Q8_0-cache attention kernels need t_head_dim = 128, a GQA ratio of 1, 2 or 4 and n_ctx in whole 64-key blocks; this model has t_head_dim = " +
                              std::to_string(mm.t_head_dim) + ", ratio " + std::to_string(R) + ", n_ctx = " + std::to_string(cfg->n_ctx));
    }
    // The vocoder's weights file, found beside the model (q3_voc_file_find), is opened and checked in full here, on the host, before the
    // device is touched: a file that is there but wrong fails the create, it never falls back to synthetic weights and never reaches a kernel.
    Q3Gguf gv;
    std::string vfile;
    if (cfg->with_vocoder && cfg->weights_path) {
        vfile = q3_voc_file_find(cfg->weights_path);
        std::string er;
        if (!vfile.empty() && (gv.open(vfile, er) || q3_voc_file_check(gv, vfile, cfg->vocoder, er))) return q3_set_err(nullptr, Q3TTS_ERR_INVALID, er);
    }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return q3_set_err(nullptr, Q3TTS_ERR_DEVICE, "no HIP device: libq3tts has no CPU fallback");
    if (cfg->device < 0 || cfg->device >= ndev) return q3_set_err(nullptr, Q3TTS_ERR_INVALID, "device ordinal out of range");
    q3tts_engine* e = new q3tts_engine();
    e->cfg = *cfg; e->cfg.weights_path = nullptr;
    e->weights_dir = cfg->weights_path ? cfg->weights_path : "";
    e->max_steps = cfg->max_steps_cap < 512 ? cfg->max_steps_cap : 512;
    auto fail = [&](int rc) { std::string m = e->err; q3tts_engine_destroy(e); g_err = m; return rc; };
#define TRYC(x) do { int rc__ = (x); if (rc__ != Q3TTS_OK) return fail(rc__); } while (0)
#define HIPC(call) do { hipError_t er__ = (call); if (er__ != hipSuccess) { q3_set_err(e, Q3TTS_ERR_DEVICE, std::string(#call) + ": " + hipGetErrorString(er__)); return fail(Q3TTS_ERR_DEVICE); } } while (0)
    HIPC(hipSetDevice(cfg->device));
    {   // before the first allocation: what the config sizes against the device's free memory (not a failure half-way through q3_dalloc)
        size_t free_b = 0, total_b = 0;
        HIPC(hipMemGetInfo(&free_b, &total_b));
        const unsigned long long need = engine_footprint(*cfg);
        if (need > (unsigned long long)free_b) {
            q3_set_err(e, Q3TTS_ERR_OOM, "engine needs at least " + std::to_string(need) + " bytes of device memory for max_batch = " + std::to_string(cfg->max_batch) +
                       ", n_ctx = " + std::to_string(cfg->n_ctx) + (cfg->kv_q8_0 ? " (Q8_0 cache)" : "") + "; the device has " + std::to_string((unsigned long long)free_b) +
                       (cfg->kv_q8_0 ? " bytes free (fewer slots or a smaller n_ctx)" : " bytes free (fewer slots, a smaller n_ctx, or kv_q8_0 = 1: the cache in 0.53 of the bytes)"));
            return fail(Q3TTS_ERR_OOM);
        }
    }
    q3_bgemm_prepare();
    if (cfg->talker_q8_0 == 2 || cfg->predictor_q8_0 == 2) q3_bgemm8_prepare();  // kernel attributes: never inside the captures below
    HIPC(hipStreamCreateWithFlags(&e->stream, hipStreamNonBlocking));
    // Q3TTS_VOC_SERIAL=1: the vocoder shares the decoder stream (no overlap): isolates its kernels in a profile
    // (highest / lowest stream priority for the decoder / vocoder streams was measured in both rounds: no change, left out)
    // Q3TTS_VOC_CUMASK=<hex word>: experiment — the vocoder stream only runs on the CUs whose bit is set in the word (repeated over the
    // 256 CUs), so that decoder workgroups always find CUs without long-lived vocoder workgroups (profiles/README.md, r03)
    if (getenv("Q3TTS_VOC_SERIAL") && atoi(getenv("Q3TTS_VOC_SERIAL"))) e->vstream = e->stream;
    else if (getenv("Q3TTS_VOC_CUMASK")) {
        uint32_t w = (uint32_t)strtoul(getenv("Q3TTS_VOC_CUMASK"), nullptr, 16), mask[8];
        for (auto& x : mask) x = w;
        HIPC(hipExtStreamCreateWithCUMask(&e->vstream, 8, mask));
    } else HIPC(hipStreamCreateWithFlags(&e->vstream, hipStreamNonBlocking));
    HIPC(hipEventCreate(&e->ev0)); HIPC(hipEventCreate(&e->ev1)); HIPC(hipEventCreate(&e->ev2)); HIPC(hipEventCreate(&e->ev3));
    e->fin_ev.resize(cfg->max_batch, nullptr);
    for (auto& ev : e->fin_ev) HIPC(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
    const q3tts_model_config& m = e->cfg.model;  // (q3_assets_init: the table row counts follow the files when weights_path is given)
    const int B = cfg->max_batch;
    e->B = B;
    hipStream_t s = e->stream;
    // weights_path: the reference's quant directory (q3_weights.hip); NULL: seeded synthetic weights
    const std::string wdir = cfg->weights_path ? cfg->weights_path : "";
    Q3Gguf gt, gp;
    std::string er;
    if (!wdir.empty() && (gt.open(wdir + "/qwen3_tts_talker.gguf", er) || gp.open(wdir + "/qwen3_tts_predictor.gguf", er))) { q3_set_err(e, Q3TTS_ERR_INVALID, er); return fail(Q3TTS_ERR_INVALID); }
    TRYC(q3_tfm_init(e, e->T, {.grp = Q3G_TALKER, .L = m.t_n_layer, .d = m.t_d_model, .Hq = m.t_n_head, .Hkv = m.t_n_kv_head, .hd = m.t_head_dim, .F = m.t_d_ffn,
                               .head_n = m.t_vocab, .theta = m.t_rope_theta, .sections = m.t_mrope_sections, .n_ctx = cfg->n_ctx, .n_slots = B, .kv8 = cfg->kv_q8_0},
                     wdir.empty() ? nullptr : &gt, "qwen3_tts_talker.gguf", cfg->talker_q8_0));
    TRYC(q3_tfm_init(e, e->P, {.grp = Q3G_PRED, .L = m.p_n_layer, .d = m.p_d_model, .Hq = m.p_n_head, .Hkv = m.p_n_kv_head, .hd = m.p_head_dim, .F = m.p_d_ffn,
                               .head_n = (m.n_codebooks - 1) * m.codebook_size, .theta = m.p_rope_theta, .sections = nullptr, .n_ctx = 64, .n_slots = B, .kv8 = 0},
                     wdir.empty() ? nullptr : &gp, "qwen3_tts_predictor.gguf", cfg->predictor_q8_0));
    TRYC(q3_assets_init(e, wdir));
    TRYC(q3_pred_table_init(e));
    // decode state
    TRYC(q3_dalloc(e, &e->slots, (size_t)B));
    HIPC(hipHostMalloc((void**)&e->slots_host, sizeof(Q3Slot) * 2 * B, hipHostMallocDefault));
    memset(e->slots_host, 0, sizeof(Q3Slot) * 2 * B);
    TRYC(q3_dalloc(e, &e->codes, (size_t)B * cfg->max_steps_cap * m.n_codebooks)); TRYC(q3_dalloc(e, &e->rng, (size_t)B * cfg->max_steps_cap));
    TRYC(q3_dalloc(e, &e->prng, (size_t)B * cfg->max_steps_cap * (m.n_codebooks - 1)));
    e->seen_words = (m.sample_limit + 31) / 32;
    TRYC(q3_dalloc(e, &e->seen, (size_t)B * e->seen_words));
    // streamed text (Q3TextRows) and a parked slot's rows: zero = no slot streams, every cursor says tts_pad
    TRYC(q3_dalloc(e, &e->ts_ids, (size_t)B * cfg->max_steps_cap)); TRYC(q3_dalloc(e, &e->ts_cnt, (size_t)B)); TRYC(q3_dalloc(e, &e->ts_cur, (size_t)B));
    TRYC(q3_dalloc(e, &e->park_logits, (size_t)B * m.t_vocab)); TRYC(q3_dalloc(e, &e->park_x, (size_t)B * m.t_d_model));
    e->ts_slot.assign(B, 0);
    {
        const int nb = B;
        const int nqkv_max = std::max(e->T.nqkv, e->P.nqkv), nq_max = std::max(e->T.nq, e->P.nq), F_max = std::max(e->T.F, e->P.F);
        Q3Lane& L = e->lane;
        L.nb = nb;
        HIPC(hipStreamCreateWithFlags(&L.stream, hipStreamNonBlocking));
        HIPC(hipEventCreate(&L.ev_begin)); HIPC(hipEventCreate(&L.ev_end));
        TRYC(alloc_rows(e, L.T, (size_t)nb, m.t_d_model, e->T.a8)); TRYC(alloc_rows(e, L.P, (size_t)2 * nb, m.p_d_model, e->P.a8));
        TRYC(q3_dalloc(e, &L.logits, (size_t)nb * m.t_vocab)); TRYC(q3_dalloc(e, &L.logits_tmp, (size_t)nb * std::max(m.t_vocab, m.t_d_model)));
        TRYC(q3_dalloc(e, &L.fb, (size_t)nb * m.d_embed)); TRYC(q3_dalloc(e, &L.keys, (size_t)nb * (m.codebook_size / 16)));
        TRYC(q3_dalloc(e, &L.plogits, (size_t)nb * m.codebook_size));
        TRYC(q3_dalloc(e, &L.row_pos_t, (size_t)nb)); TRYC(q3_dalloc(e, &L.slot_id, (size_t)nb)); TRYC(q3_dalloc(e, &L.perm, (size_t)nb));
        std::vector<int> sid(nb), rp(nb, -1);
        for (int b = 0; b < nb; ++b) sid[b] = b;
        HIPC(hipMemcpyAsync(L.slot_id, sid.data(), nb * 4, hipMemcpyHostToDevice, s));
        HIPC(hipMemcpyAsync(L.row_pos_t, rp.data(), nb * 4, hipMemcpyHostToDevice, s));
        HIPC(hipStreamSynchronize(s));
        TRYC(alloc_scratch(e, L.sc, 2 * nb, nqkv_max, nq_max, F_max));
        row_buckets(nb, e->buckets);
        e->bucket_steps = std::vector<std::atomic<long long>>(e->buckets.size());
        e->cur_bucket = (int)e->buckets.size() - 1;
        e->row_of_slot = sid; e->slot_of_row = sid;
    }
    TRYC(alloc_scratch(e, e->sc_pre, cfg->n_ctx, e->T.nqkv, e->T.nq, e->T.F));
    TRYC(alloc_rows(e, e->pf, (size_t)cfg->n_ctx, m.t_d_model, e->T.a8));
    TRYC(q3_dalloc(e, &e->pf_pos, (size_t)cfg->n_ctx)); TRYC(q3_dalloc(e, &e->pf_slot, (size_t)cfg->n_ctx)); TRYC(q3_dalloc(e, &e->pf_seg, (size_t)4 * cfg->max_batch));
    { std::vector<int> pp(cfg->n_ctx); for (int i = 0; i < cfg->n_ctx; ++i) pp[i] = i;
      HIPC(hipMemcpyAsync(e->pf_pos, pp.data(), pp.size() * 4, hipMemcpyHostToDevice, s)); HIPC(hipStreamSynchronize(s)); }
    e->prow_cap = cfg->n_ctx;
    TRYC(q3_dalloc(e, &e->prow_dev, (size_t)e->prow_cap)); TRYC(q3_dalloc(e, &e->spk_dev, (size_t)m.d_embed));
    TRYC(q3_dalloc(e, &e->refcodes_dev, (size_t)cfg->n_ctx * 16));
    {   // the marker row text[151671] through the table's out-of-range rule (src/assets_manager.rs:444-460): a missing or short text
        // table gives the fallback pattern, never a null / out-of-bounds read (the clone prompt adds this row to every reference frame)
        TRYC(q3_dalloc(e, &e->marker_row, (size_t)m.d_embed));
        const Q3PromptRow mr{1, m.tts_pad_id, 0, 0};
        HIPC(hipMemcpyAsync(e->prow_dev, &mr, sizeof(mr), hipMemcpyHostToDevice, s));
        HIPC(hipStreamSynchronize(s));
        q3_launch_prompt_rows(e->prow_dev, 1, e->text, m.text_vocab, e->codec_dev, m.codec0_rows, m.codecq_rows, m.n_codebooks, e->spk_dev, m.d_embed, e->marker_row, s);
        HIPC(hipStreamSynchronize(s));
    }
    if (cfg->with_vocoder) {
        TRYC(q3_voc_create(e, vfile.empty() ? nullptr : &gv, vfile));
        HIPC(hipHostMalloc((void**)&e->first_chunk_host, sizeof(float) * 4 * (size_t)q3_voc_samples_per_frame(e), hipHostMallocDefault));
    }
    // capture the frame step once per row-count bucket; every later frame is a replay (Q3TTS_NO_GRAPH=1: eager launches, for profilers)
    HIPC(hipStreamSynchronize(s));
    if (!(getenv("Q3TTS_NO_GRAPH") && atoi(getenv("Q3TTS_NO_GRAPH")))) TRYC(q3_capture_frames(e, e->lane.graphs, e->lane.execs));
#undef TRYC
#undef HIPC
    *out = e;
    return Q3TTS_OK;
}

extern "C" void q3tts_engine_destroy(q3tts_engine* e) {
    if (!e) return;
    if (q3tts_session* ss = e->session.load()) q3tts_session_close(ss);
    hipSetDevice(e->cfg.device);
    if (e->stream) hipStreamSynchronize(e->stream);
    if (e->vstream) hipStreamSynchronize(e->vstream);
    if (e->voc) q3_voc_destroy(e);
    q3_mel_destroy(e);
    q3_clone_destroy(e);
    if (e->first_chunk_host) hipHostFree(e->first_chunk_host);
    {
        Q3Lane& L = e->lane;
        if (L.stream) hipStreamSynchronize(L.stream);
        for (auto ge : L.execs) if (ge) hipGraphExecDestroy(ge);
        for (auto gr : L.graphs) if (gr) hipGraphDestroy(gr);
        for (auto ge : L.execs_s) if (ge) hipGraphExecDestroy(ge);
        for (auto gr : L.graphs_s) if (gr) hipGraphDestroy(gr);
        for (int v = 0; v < 2; ++v) {
            for (auto ge : L.execs_t[v]) if (ge) hipGraphExecDestroy(ge);
            for (auto gr : L.graphs_t[v]) if (gr) hipGraphDestroy(gr);
        }
        if (L.ev_begin) hipEventDestroy(L.ev_begin); if (L.ev_end) hipEventDestroy(L.ev_end);
        if (L.stream) hipStreamDestroy(L.stream);
    }
    for (void* p : e->allocs) hipFree(p);  // every q3_dalloc: weights, tables, caches, rows, scratch, decode and prefill state
    hipFree(e->dev_pcm);                   // regrows per batch: its own pair (q3tts_generate_batch)
    hipFree(e->rs_stage);                  // regrows with the output rate: its own pair (q3tts_set_output_rate)
    hipFree(e->tp_row);                    // regrows with the speed: its own pair (q3tts_set_speed)
    if (e->slots_host) hipHostFree(e->slots_host);
    for (auto ev : e->fin_ev) if (ev) hipEventDestroy(ev);
    for (auto ev : e->probe_ev) if (ev) hipEventDestroy(ev);
    if (e->ev0) hipEventDestroy(e->ev0); if (e->ev1) hipEventDestroy(e->ev1); if (e->ev2) hipEventDestroy(e->ev2); if (e->ev3) hipEventDestroy(e->ev3);
    if (e->stream) hipStreamDestroy(e->stream);
    if (e->vstream && e->vstream != e->stream) hipStreamDestroy(e->vstream);
    delete e;
}

extern "C" int q3tts_set_sampler(q3tts_engine* e, float temperature, int32_t top_k, float top_p, int32_t has_seed, uint64_t seed) {
    if (!e) return q3_set_err(nullptr, Q3TTS_ERR_INVALID, "null engine");
    Q3_NOT_IN_SESSION(e);
    e->temperature = temperature; e->top_k = top_k; e->top_p = top_p; e->has_seed = has_seed; e->seed = seed;
    return Q3TTS_OK;
}
// Predictor sampler + repetition penalty (include/q3tts.h). Engine state like the sampler's above; refused while a session or a stream is
// open, so every live slot was admitted under the state the frame step's variant was chosen from.
static int refuse_busy(q3tts_engine* e) {
    if (e->streams_open > 0) return q3_set_err(e, Q3TTS_ERR_STATE, "a stream is open on this engine (q3tts_stream_end first)");
    return Q3TTS_OK;
}
// the frame step e->pred_variant names must exist before the next frame: the sampling kernel's attributes (never inside a capture) and,
// when frames are replayed from graphs, its own set of them — captured the first time the variant is needed, kept afterwards
static int set_pred_variant(q3tts_engine* e, int variant) {
    if (variant && e->cfg.model.codebook_size > Q3_SAMP_MAX) return q3_set_err(e, Q3TTS_ERR_INVALID, "the Predictor sampler needs codebook_size <= 4096");
    if (!variant) { e->pred_variant = 0; return Q3TTS_OK; }
    Q3_HIP(e, hipSetDevice(e->cfg.device));
    if (q3_pred_next_prepare() != 0) return q3_set_err(e, Q3TTS_ERR_DEVICE, "the Predictor sampler's kernel: the device refused its LDS size (hipFuncSetAttribute)");
    e->pred_variant = variant;
    Q3Lane& L = e->lane;
    if (!L.execs.empty() && L.execs_s.empty()) {
        Q3_HIP(e, hipStreamSynchronize(e->stream));
        const int rc = q3_capture_frames(e, L.graphs_s, L.execs_s);
        if (rc != Q3TTS_OK) {
            for (auto ge : L.execs_s) if (ge) hipGraphExecDestroy(ge);
            for (auto gr : L.graphs_s) if (gr) hipGraphDestroy(gr);
            L.execs_s.clear(); L.graphs_s.clear(); e->pred_variant = 0;
            return rc;
        }
    }
    return Q3TTS_OK;
}
extern "C" int q3tts_set_predictor_sampler(q3tts_engine* e, float temperature, int32_t top_k, float top_p) {
    if (!e) return q3_set_err(nullptr, Q3TTS_ERR_INVALID, "null engine");
    Q3_NOT_IN_SESSION(e);
    TRY(refuse_busy(e));
    if (!std::isfinite(temperature) || temperature < 0.0f) return q3_set_err(e, Q3TTS_ERR_INVALID, "predictor sampler: temperature must be finite and >= 0");
    if (!std::isfinite(top_p)) return q3_set_err(e, Q3TTS_ERR_INVALID, "predictor sampler: top_p must be finite");
    if (temperature > 0.0f && e->cfg.model.codebook_size > Q3_SAMP_MAX) return q3_set_err(e, Q3TTS_ERR_INVALID, "the Predictor sampler needs codebook_size <= 4096");
    TRY(set_pred_variant(e, (temperature > 0.0f || e->pred_force) ? 1 : 0));
    e->p_temperature = temperature; e->p_top_k = top_k; e->p_top_p = top_p;
    return Q3TTS_OK;
}
extern "C" int q3tts_get_predictor_sampler(const q3tts_engine* e, float* temperature, int32_t* top_k, float* top_p) {
    if (!e) return q3_set_err(nullptr, Q3TTS_ERR_INVALID, "null engine");
    if (temperature) *temperature = e->p_temperature;
    if (top_k) *top_k = e->p_top_k;
    if (top_p) *top_p = e->p_top_p;
    return Q3TTS_OK;
}
extern "C" int q3tts_set_repetition_penalty(q3tts_engine* e, float penalty) {
    if (!e) return q3_set_err(nullptr, Q3TTS_ERR_INVALID, "null engine");
    Q3_NOT_IN_SESSION(e);
    TRY(refuse_busy(e));
    if (!std::isfinite(penalty) || !(penalty > 0.0f)) return q3_set_err(e, Q3TTS_ERR_INVALID, "repetition penalty must be finite and > 0");
    e->rep_penalty = penalty;
    return Q3TTS_OK;
}
extern "C" int q3tts_get_repetition_penalty(const q3tts_engine* e, float* penalty) {
    if (!e) return q3_set_err(nullptr, Q3TTS_ERR_INVALID, "null engine");
    if (penalty) *penalty = e->rep_penalty;
    return Q3TTS_OK;
}
int q3_pred_force_variant(q3tts_engine* e, int force) {
    TRY(refuse_busy(e));
    const int was = e->pred_force;
    e->pred_force = force ? 1 : 0;
    const int rc = set_pred_variant(e, (e->p_temperature > 0.0f || e->pred_force) ? 1 : 0);
    if (rc != Q3TTS_OK) e->pred_force = was;
    return rc;
}
extern "C" int q3tts_set_max_steps(q3tts_engine* e, int32_t n) {
    if (!e) return q3_set_err(nullptr, Q3TTS_ERR_INVALID, "null engine");
    Q3_NOT_IN_SESSION(e);
    if (n < 0 || n > e->cfg.max_steps_cap) return q3_set_err(e, Q3TTS_ERR_INVALID, "max_steps exceeds max_steps_cap");
    e->max_steps = n;
    return Q3TTS_OK;
}
extern "C" void q3tts_free(void* p) { free(p); }
// Device-resident results for multi-GPU gathers: with enable = 1 every q3tts_generate_batch call also keeps each
// request's PCM in row i of an engine-owned device buffer [n][stride] f32 (valid until the next call); requests with want_pcm = 2
// skip the host copy altogether.
extern "C" int q3tts_set_device_pcm(q3tts_engine* e, int32_t enable) {
    Q3_NOT_IN_SESSION(e);
    if (!e) return q3_set_err(nullptr, Q3TTS_ERR_INVALID, "null engine");
    if (enable && e->out_rate) return q3_set_err(e, Q3TTS_ERR_STATE, "device-resident PCM is native-rate only (q3tts_set_output_rate(engine, 0) first)");
    if (enable && e->speed) return q3_set_err(e, Q3TTS_ERR_STATE, "device-resident PCM is unstretched (q3tts_set_speed(engine, 0) first)");
    e->dev_pcm_on = enable ? 1 : 0;
    return Q3TTS_OK;
}
extern "C" int q3tts_get_device_pcm(q3tts_engine* e, float** base, int64_t* stride_samples, int32_t* n_rows) {
    if (!e || !base || !stride_samples || !n_rows) return q3_set_err(e, Q3TTS_ERR_INVALID, "null argument");
    *base = e->dev_pcm; *stride_samples = (int64_t)e->dev_pcm_stride; *n_rows = e->dev_pcm_n;
    return Q3TTS_OK;
}

// ------------------------------------------------------------------------------------------------
// H1 prompt builder: row list on the host (src/tts/prompt.rs:141-277, :28-118), gathers on the device
// ------------------------------------------------------------------------------------------------
enum { PAD = 2148, BOS = 2149, THINK = 2154, NOTHINK = 2155, THINK_BOS = 2156, THINK_EOS = 2157, CODEC_BOS_ICL = 2160 };

// part: which rows to build. The voice part (instruct, role, control, speaker, clone blocks) comes first and the text part (BOS, text,
// EOS, activation row) last, so PROMPT_VOICE ++ PROMPT_TEXT is PROMPT_WHOLE row for row (voice prefixes: include/q3tts.h).
// text_stream: the text part in the streamed layout (include/q3tts.h, "streaming text input"): BOS, then text[x[0]] + codec0[BOS] in place of
// the activation row; x[1 ..) and EOS join the feedback rows (q3_text_trailing, Q3TextRows). The voice part is the same either way.
int build_prompt_dev(q3tts_engine* e, const q3tts_prompt_desc* p, float* out, int max_rows, int* n_out, int part, bool text_stream) {
    const q3tts_model_config& m = e->cfg.model;
    if (!p || (p->n_text > 0 && !p->text_ids)) return q3_set_err(e, Q3TTS_ERR_INVALID, "prompt: text_ids missing");
    if (text_stream && (part == PROMPT_VOICE || p->n_text < 1)) return q3_set_err(e, Q3TTS_ERR_INVALID, "text_stream: the prompt needs n_text >= 1 (its first text id is the prompt's last row)");
    if (part == PROMPT_VOICE && p->n_text != 0) return q3_set_err(e, Q3TTS_ERR_INVALID, "prefix: a voice desc has n_text == 0");
    if (part == PROMPT_TEXT) {  // behind a prefix: the voice is the prefix's
        const char* f = p->instruct_ids ? "instruct_ids" : p->lang_id >= 0 ? "lang_id" : p->spk_id >= 0 ? "spk_id" : p->spk_emb ? "spk_emb"
                      : p->ref_codes ? "ref_codes" : p->ref_text_ids ? "ref_text_ids" : nullptr;
        if (f) return q3_set_err(e, Q3TTS_ERR_INVALID, std::string("prompt: ") + f + " must be None in a request with a prefix (the voice is the prefix's)");
    }
    const int marker = m.tts_pad_id;
    std::vector<Q3PromptRow> rows;
    int ref_row0 = -1;
    auto T1 = [&](int id) { rows.push_back({1, id, 0, 0}); };
    auto MC = [&](int cid) { rows.push_back({1, marker, 2, cid}); };       // marker + codec0[cid]
    auto TP = [&](int tid) { rows.push_back({1, tid, 2, PAD}); };          // text[tid] + codec0[PAD]
    if (part != PROMPT_TEXT) {  // the voice part
        if (p->instruct_ids) {  // :153-169
            T1(151644); T1(872); T1(198);
            for (int i = 0; i < p->n_instruct; ++i) T1((int)p->instruct_ids[i]);
            T1(151645); T1(198);
        }
        T1(151644); T1(77091); T1(198);  // :171-175
        if (p->lang_id >= 0) { MC(THINK); MC(THINK_BOS); MC(p->lang_id); MC(THINK_EOS); }  // :180-191
        else { MC(NOTHINK); MC(THINK_BOS); MC(THINK_EOS); }                                // :192-204
        if (p->spk_id >= 0) MC(p->spk_id);                                                 // :207-214
        else if (p->spk_emb) rows.push_back({1, marker, -1, 0});                           // :215-222
        if (p->ref_codes) {  // build_clone_prompt :38-106
            TP(BOS_TOKEN);
            for (int i = 0; i < p->n_ref_text; ++i) TP((int)p->ref_text_ids[i]);
            TP(EOS_TOKEN);
            MC(CODEC_BOS_ICL);
            ref_row0 = (int)rows.size();
            for (int i = 0; i < p->n_ref_frames; ++i) rows.push_back({-2, 0, 0, 0});  // filled by the frame kernel
            MC(PAD);
        }
    }
    if (part != PROMPT_VOICE && text_stream) {  // the streamed text part
        TP(BOS_TOKEN);
        rows.push_back({1, (int)p->text_ids[0], 2, BOS});
    } else if (part != PROMPT_VOICE) {  // the text part
        TP(BOS_TOKEN);                                             // :229-239
        for (int i = 0; i < p->n_text; ++i) TP((int)p->text_ids[i]);  // :241-245
        TP(EOS_TOKEN);                                             // :247-254
        MC(BOS);                                                   // :256-264
    }
    const int n = (int)rows.size();
    if (n > max_rows || n > e->prow_cap) return q3_set_err(e, Q3TTS_ERR_INVALID, "prompt longer than n_ctx");
    hipStream_t s = e->stream;
    Q3_HIP(e, hipMemcpyAsync(e->prow_dev, rows.data(), sizeof(Q3PromptRow) * n, hipMemcpyHostToDevice, s));
    if (p->spk_emb) Q3_HIP(e, hipMemcpyAsync(e->spk_dev, p->spk_emb, (size_t)m.d_embed * 4, hipMemcpyHostToDevice, s));
    Q3_HIP(e, hipStreamSynchronize(s));  // rows is a stack vector
    q3_launch_prompt_rows(e->prow_dev, n, e->text, m.text_vocab, e->codec_dev, m.codec0_rows, m.codecq_rows, m.n_codebooks, e->spk_dev,
                          m.d_embed, out, s);
    if (ref_row0 >= 0 && p->n_ref_frames > 0) {
        Q3_HIP(e, hipMemcpyAsync(e->refcodes_dev, p->ref_codes, (size_t)p->n_ref_frames * 16 * 4, hipMemcpyHostToDevice, s));
        Q3_HIP(e, hipStreamSynchronize(s));
        q3_launch_prompt_ref_frames(e->refcodes_dev, p->n_ref_frames, e->marker_row, e->codec_dev, m.codec0_rows,
                                    m.codecq_rows, m.n_codebooks, m.d_embed, out + (size_t)ref_row0 * m.d_embed, s);
    }
    *n_out = n;
    return Q3TTS_OK;
}

extern "C" int q3tts_build_prompt(q3tts_engine* e, const q3tts_prompt_desc* p, float** out_embd, int32_t* out_n) {
    Q3_NOT_IN_SESSION(e);
    if (!e || !p || !out_embd || !out_n) return q3_set_err(e, Q3TTS_ERR_INVALID, "null argument");
    Q3_HIP(e, hipSetDevice(e->cfg.device));
    int n = 0;
    TRY(build_prompt_dev(e, p, e->pf.x, e->cfg.n_ctx, &n));
    const size_t bytes = (size_t)n * e->cfg.model.d_embed * 4;
    float* h = (float*)malloc(bytes);
    if (!h) return q3_set_err(e, Q3TTS_ERR_OOM, "malloc");
    hipError_t er = hipMemcpyAsync(h, e->pf.x, bytes, hipMemcpyDeviceToHost, e->stream);
    if (er == hipSuccess) er = hipStreamSynchronize(e->stream);
    if (er != hipSuccess) { free(h); return q3_set_err(e, Q3TTS_ERR_DEVICE, hipGetErrorString(er)); }
    *out_embd = h; *out_n = n;
    return Q3TTS_OK;
}

// q3_engine.hip — host side of libq3tts: engine creation and teardown, batched prefill, voice prefixes, the continuous batching loop
// and the engine part of the C ABI of include/q3tts.h (weights and assets: q3_weights.hip; the transformers' launches and the
// frame step: q3_layers.hip; the kernel-level test hooks q3tts_k_*: q3_hooks.hip). The loop restates the reference's run_inference_stream (src/tts/engine.rs:445-656) with every
// per-frame decision on the device: one graph replay = sample -> 15 predictor passes -> feedback -> Talker step, no host
// round trip (the reference crosses the host<->backend boundary >= 33 times per frame).
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
extern "C" int q3tts_k_device_bytes(const q3tts_engine* e, int64_t* bytes) {
    if (!e || !bytes) return q3_set_err(nullptr, Q3TTS_ERR_INVALID, "null argument");
    *bytes = (int64_t)e->dev_bytes;
    return Q3TTS_OK;
}
#define TRY(x) do { int rc__ = (x); if (rc__ != Q3TTS_OK) return rc__; } while (0)

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
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return q3_set_err(nullptr, Q3TTS_ERR_DEVICE, "no HIP device: libq3tts has no CPU fallback");
    if (cfg->device < 0 || cfg->device >= ndev) return q3_set_err(nullptr, Q3TTS_ERR_INVALID, "device ordinal out of range");
    q3tts_engine* e = new q3tts_engine();
    e->cfg = *cfg; e->cfg.weights_path = nullptr;
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
        TRYC(q3_voc_create(e));
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
enum { PROMPT_WHOLE = 0, PROMPT_VOICE = 1, PROMPT_TEXT = 2 };
static int build_prompt_dev(q3tts_engine* e, const q3tts_prompt_desc* p, float* out, int max_rows, int* n_out, int part = PROMPT_WHOLE, bool text_stream = false) {
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

// ------------------------------------------------------------------------------------------------
// generation
// ------------------------------------------------------------------------------------------------
// Map the live slots onto rows [0, n) of the smallest bucket that holds them (idle slots fill the rest: every row keeps
// a distinct, valid slot). Row-indexed state that outlives a frame (the Talker logits) moves with its slot.
static int plan_rows(q3tts_engine* e, const std::vector<int>& live_in) {
    Q3Lane& L = e->lane;
    const int B = e->B;
    std::vector<int> live(live_in);
    std::sort(live.begin(), live.end());
    int bi = 0;
    while (bi + 1 < (int)e->buckets.size() && e->buckets[bi] < (int)live.size()) ++bi;
    bool ok = bi == e->cur_bucket;
    if (ok) for (int b : live) if (e->row_of_slot[b] >= e->buckets[bi]) { ok = false; break; }
    if (ok) return Q3TTS_OK;
    std::vector<int> slot_of_row(B, -1), perm(B), used(B, 0);
    int r = 0;
    for (int b : live) { slot_of_row[r++] = b; used[b] = 1; }
    for (int b = 0; b < B && r < B; ++b) if (!used[b]) slot_of_row[r++] = b;
    for (r = 0; r < B; ++r) perm[r] = e->row_of_slot[slot_of_row[r]];
    hipStream_t s = e->stream;
    Q3_HIP(e, hipMemcpyAsync(L.perm, perm.data(), (size_t)B * 4, hipMemcpyHostToDevice, s));
    Q3_HIP(e, hipMemcpyAsync(L.slot_id, slot_of_row.data(), (size_t)B * 4, hipMemcpyHostToDevice, s));
    // row state that outlives a frame: the Talker logits (sampled at the next frame) and its last hidden row (the
    // Predictor's first input)
    q3_launch_gather_rows(L.logits_tmp, L.logits, L.perm, B, e->cfg.model.t_vocab, s);
    Q3_HIP(e, hipMemcpyAsync(L.logits, L.logits_tmp, (size_t)B * e->cfg.model.t_vocab * 4, hipMemcpyDeviceToDevice, s));
    q3_launch_gather_rows(L.logits_tmp, L.T.x, L.perm, B, e->cfg.model.t_d_model, s);
    Q3_HIP(e, hipMemcpyAsync(L.T.x, L.logits_tmp, (size_t)B * e->cfg.model.t_d_model * 4, hipMemcpyDeviceToDevice, s));
    Q3_HIP(e, hipStreamSynchronize(s));  // the uploads read locals
    for (r = 0; r < B; ++r) e->row_of_slot[slot_of_row[r]] = r;
    e->slot_of_row = slot_of_row;
    e->cur_bucket = bi;
    return Q3TTS_OK;
}

// CH frame steps over the current row bucket; afterwards the slot mirror is on the host. Returns the device time (ms).
static double now_ms();
static int run_chunk(q3tts_engine* e, int CH, float* dev_ms) {
    hipStream_t s = e->stream;
    Q3Lane& L = e->lane;
    const double hp0 = now_ms();
    Q3_HIP(e, hipEventRecord(e->ev1, s));  // admissions (prefill, state uploads) precede the frames
    Q3_HIP(e, hipStreamWaitEvent(L.stream, e->ev1, 0));
    Q3_HIP(e, hipEventRecord(L.ev_begin, L.stream));
    e->probe_i = 0;
    if (e->probe) { hipEventRecord(e->probe_ev[8], L.stream); hipEventRecord(e->probe_ev[9], L.stream); }  // empty bracket
    // while a slot streams its text the frames come from the text form's own sets (ensure_text_frames captured them); without one the
    // choice, the sets and so every launch are what they were before text streaming existed
    bool ts = false;
    for (char f : e->ts_slot) ts |= f != 0;
    e->ts_variant = ts ? 1 : 0;
    const std::vector<hipGraphExec_t>& execs = ts ? L.execs_t[e->pred_variant ? 1 : 0] : e->pred_variant ? L.execs_s : L.execs;  // (set_pred_variant captured the second set)
    for (int i = 0; i < CH; ++i) {
        if (!execs.empty() && !e->probe) { Q3_HIP(e, hipGraphLaunch(execs[e->cur_bucket], L.stream)); }
        else {
            if (q3_record_frame(e, L, L.stream, e->buckets[e->cur_bucket])) return q3_set_err(e, Q3TTS_ERR_INVALID, "frame step: a kernel launch was refused for this model shape");
            Q3_HIP(e, hipGetLastError());
        }
    }
    e->row_steps += (long long)CH * e->buckets[e->cur_bucket];
    e->bucket_steps[e->cur_bucket].fetch_add(CH, std::memory_order_relaxed);
    Q3_HIP(e, hipEventRecord(L.ev_end, L.stream));
    Q3_HIP(e, hipStreamWaitEvent(s, L.ev_end, 0));
    Q3_HIP(e, hipEventRecord(e->ev3, s));  // the vocoder stream waits on this
    Q3_HIP(e, hipMemcpyAsync(e->slots_host, e->slots, sizeof(Q3Slot) * e->B, hipMemcpyDeviceToHost, s));
    const double hp1 = now_ms();
    Q3_HIP(e, hipStreamSynchronize(s));
    e->hp_launch += hp1 - hp0; e->hp_sync += now_ms() - hp1;  // Q3TTS_HOST_PROF: host wall of the launch part / of the wait
    if (dev_ms) { *dev_ms = 0.0f; hipEventElapsedTime(dev_ms, L.ev_begin, L.ev_end); }
    for (int i = 0; i + 1 < e->probe_i; i += 2) {
        float ms = 0.0f;
        if (hipEventElapsedTime(&ms, e->probe_ev[i], e->probe_ev[i + 1]) == hipSuccess) { e->probe_ms += ms; ++e->probe_cnt; }
    }
    if (e->probe) {
        float ms = 0.0f;
        if (hipEventElapsedTime(&ms, e->probe_ev[8], e->probe_ev[9]) == hipSuccess) { e->probe_empty_ms += ms; ++e->probe_empty_cnt; }
    }
    return Q3TTS_OK;
}

static uint64_t wall_seed() {
    return (uint64_t)std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::system_clock::now().time_since_epoch()).count();
}

// Talker prefill (src/tts/engine.rs:455-462) of several requests at once: their prompt rows are concatenated into one
// batch (row -> (slot, position) maps), so the weights stream once for all of them; then per request the last row
// seeds the slot (logits, state, sampler draws). rc[i] receives the per-request status.
// A request behind a voice prefix (P > 0 rows) brings only its own n rows: they sit at positions P .. P + n - 1 of its slot, whose first
// P positions receive a copy of the prefix's K/V (k_kv_prefix, one launch for the group) before the layers run.
// keep (sessions): after the group's layers, positions 0 .. keep_rows - 1 of the slot are copied into that prefix's store
// (k_kv_prefix_save, one launch for the group). r == null: a prefill-only prefix job — its voice rows ride the group's prefill into a
// free slot and are saved; no head GEMM, no draws, no slot record, no vocoder reset: the slot never becomes active.
struct Adm { int b; const q3tts_request* r; int n, row0, max_steps, P; q3tts_prefix* keep; int keep_rows; };

// ---- streamed text (include/q3tts.h, "streaming text input") ----
void q3_text_trailing(const q3tts_request* r, std::vector<int32_t>& T) {
    T.clear();
    const q3tts_prompt_desc* p = r->prompt;
    for (int i = 1; p && i < p->n_text; ++i) T.push_back((int32_t)p->text_ids[i]);
    if (!(r->text_open == 1)) T.push_back(EOS_TOKEN);
}
int q3_text_rows_set(q3tts_engine* e, int b, const int32_t* T, int from, int n, int n_frames) {
    const int cap = e->cfg.max_steps_cap, c = std::min(std::max(n, 0), cap);  // (frames stop at max_steps <= cap: later rows are never read)
    hipStream_t s = e->stream;
    from = std::max(from, 0);
    if (from < c) Q3_HIP(e, hipMemcpyAsync(e->ts_ids + (size_t)b * cap + from, T + from, (size_t)(c - from) * 4, hipMemcpyHostToDevice, s));
    const int2 cur = n_frames >= 0 && n_frames < c ? make_int2(1, T[n_frames]) : make_int2(0, 0);
    Q3_HIP(e, hipMemcpyAsync(e->ts_cnt + b, &c, 4, hipMemcpyHostToDevice, s));
    Q3_HIP(e, hipMemcpyAsync(e->ts_cur + b, &cur, sizeof(cur), hipMemcpyHostToDevice, s));
    Q3_HIP(e, hipStreamSynchronize(s));  // the uploads read locals
    return Q3TTS_OK;
}
int q3_park_rows(q3tts_engine* e, int b, bool save) {
    const q3tts_model_config& m = e->cfg.model;
    Q3Lane& L = e->lane;
    const size_t row = (size_t)e->row_of_slot[b], nl = (size_t)m.t_vocab, nx = (size_t)m.t_d_model;
    float *lg = L.logits + row * nl, *x = L.T.x + row * nx, *plg = e->park_logits + (size_t)b * nl, *px = e->park_x + (size_t)b * nx;
    Q3_HIP(e, hipMemcpyAsync(save ? plg : lg, save ? lg : plg, nl * 4, hipMemcpyDeviceToDevice, e->stream));
    Q3_HIP(e, hipMemcpyAsync(save ? px : x, save ? x : px, nx * 4, hipMemcpyDeviceToDevice, e->stream));
    return Q3TTS_OK;
}
// The text form of the frame step exists before a text_stream request's first frame: its own graph sets for the current Predictor
// variant, captured the first time one is needed and kept (the variant cannot change while anything is in flight). The sets of the
// default path are not touched. Without graphs (Q3TTS_NO_GRAPH, the probe) frames are issued eagerly and nothing is captured.
static int ensure_text_frames(q3tts_engine* e) {
    e->ts_used = 1;
    Q3Lane& L = e->lane;
    const int v = e->pred_variant ? 1 : 0;
    if (L.execs.empty() || !L.execs_t[v].empty()) return Q3TTS_OK;
    Q3_HIP(e, hipStreamSynchronize(e->stream));
    const int was = e->ts_variant;
    e->ts_variant = 1;
    const int rc = q3_capture_frames(e, L.graphs_t[v], L.execs_t[v]);
    e->ts_variant = was;
    if (rc != Q3TTS_OK) {
        for (auto ge : L.execs_t[v]) if (ge) hipGraphExecDestroy(ge);
        for (auto gr : L.graphs_t[v]) if (gr) hipGraphDestroy(gr);
        L.execs_t[v].clear(); L.graphs_t[v].clear();
    }
    return rc;
}

// The Talker's layers over the first pos.size() prefill rows (e->pf.x holds them): row i sits at position pos[i] of slot slot[i]; seg: the
// same rows as per-slot runs (pf_seg), seg_max_n the longest run, seg_max_t the furthest position + 1. The maps are uploaded and the stream
// is synchronised (they are the caller's locals); kp (admission only): the voice prefixes' K/V enter their slots before the layers run.
// Returns the number of refused launches, or -1 when an upload failed (e->err says which).
static int prefill_layers(q3tts_engine* e, const std::vector<int>& pos, const std::vector<int>& slot, const std::vector<int>& seg, int seg_max_n,
                          int seg_max_t, const Q3KvPrefix* kp) {
    const int rows = (int)pos.size(), d = e->T.d;
    hipStream_t s = e->stream;
    hipError_t er = hipMemcpyAsync(e->pf_pos, pos.data(), (size_t)rows * 4, hipMemcpyHostToDevice, s);
    if (er == hipSuccess) er = hipMemcpyAsync(e->pf_slot, slot.data(), (size_t)rows * 4, hipMemcpyHostToDevice, s);
    if (er == hipSuccess) er = hipMemcpyAsync(e->pf_seg, seg.data(), seg.size() * 4, hipMemcpyHostToDevice, s);
    if (er == hipSuccess) er = hipStreamSynchronize(s);
    if (er != hipSuccess) { q3_set_err(e, Q3TTS_ERR_DEVICE, std::string("prefill row maps: ") + hipGetErrorString(er)); return -1; }
    if (kp) q3_launch_kv_prefix(*kp, s);
    const Q3Rows& r = e->pf;
    if (e->T.a8) q3_launch_norm_inputs_q8(r.x, d, rows, d, e->T.attn_norm[0], (int8_t*)r.xb, r.ascale, r.rt16, r.ssp, d / 16, s);
    else q3_launch_norm_inputs(r.x, d, rows, d, e->T.attn_norm[0], r.xb, 0, r.ssp, d / 16, s);
    return q3_run_layers(e, e->T, r, {.rows = rows, .row_pos = e->pf_pos, .row_slot = e->pf_slot, .seg = e->pf_seg, .n_seg = (int)seg.size() / 4,
                                   .seg_max_n = seg_max_n, .seg_max_t = seg_max_t}, e->sc_pre, s);
}

static int admit_group(q3tts_engine* e, std::vector<Adm>& grp, int total) {
    const q3tts_model_config& m = e->cfg.model;
    hipStream_t s = e->stream;
    if (grp.empty()) return Q3TTS_OK;
    std::vector<int> pos(total), slot(total);
    for (const Adm& a : grp) for (int i = 0; i < a.n; ++i) { pos[a.row0 + i] = a.P + i; slot[a.row0 + i] = a.b; }
    int n_kvp_launch = 0; long long n_prefixed = 0;
    std::vector<int> seg; int seg_max = 0, seg_max_t = 0;  // the same rows as runs: every request's rows are consecutive, positions P .. P + n - 1
    Q3KvPrefix kp{}; kp.kc = e->T.kc; kp.vc = e->T.vc; kp.layer_stride = e->T.layer_stride; kp.n_ctx = e->T.n_ctx; kp.L = e->T.L; kp.Hkv = e->T.Hkv; kp.hd = e->T.hd;
    kp.kv8 = e->T.kv8 ? 1 : 0; kp.kd = e->T.kd; kp.vd = e->T.vd;
    for (const Adm& a : grp) {
        seg.push_back(a.row0); seg.push_back(a.n); seg.push_back(a.b); seg.push_back(a.P);
        seg_max = std::max(seg_max, a.n); seg_max_t = std::max(seg_max_t, a.P + a.n);
        if (a.P > 0) {
            if (kp.n == Q3_KVP_MAX) { q3_launch_kv_prefix(kp, s); kp.n = 0; ++n_kvp_launch; }  // the descriptor is full (more than 64 prefixed requests in a group): these copies go now, ahead of the group's layers on the same stream
            const q3tts_prefix* x = a.r->prefix;
            kp.pk[kp.n] = x->k; kp.pv[kp.n] = x->v; kp.P[kp.n] = x->P; kp.slot[kp.n] = a.b; ++kp.n; ++n_prefixed;
        }
    }
    e->kvp_launches.fetch_add(n_kvp_launch + (kp.n > 0 ? 1 : 0), std::memory_order_relaxed);  // (prefill_layers launches the rest)
    if (n_prefixed > e->kvp_group_max.load(std::memory_order_relaxed)) e->kvp_group_max.store(n_prefixed, std::memory_order_relaxed);
    const int rl = prefill_layers(e, pos, slot, seg, seg_max, seg_max_t, &kp);
    if (rl < 0) return Q3TTS_ERR_DEVICE;
    if (rl) return q3_set_err(e, Q3TTS_ERR_INVALID, "prefill: a kernel launch was refused for this model shape");
    Q3_HIP(e, hipGetLastError());
    bool keeps = false;
    for (const Adm& a : grp) keeps |= a.keep != nullptr;
    if (keeps) {  // the slots' voice rows into their prefix stores, behind the layers on the same stream
        Q3KvPrefix sv = kp; sv.n = 0;
        for (const Adm& a : grp) {
            if (!a.keep) continue;
            if (sv.n == Q3_KVP_MAX) { if (q3_launch_kv_prefix_save(sv, s)) return q3_set_err(e, Q3TTS_ERR_INVALID, "prefix save: launch refused for this model shape"); sv.n = 0; }
            sv.pk[sv.n] = a.keep->k; sv.pv[sv.n] = a.keep->v; sv.P[sv.n] = a.keep_rows; sv.slot[sv.n] = a.b; ++sv.n;
        }
        if (q3_launch_kv_prefix_save(sv, s)) return q3_set_err(e, Q3TTS_ERR_INVALID, "prefix save: launch refused for this model shape");
        Q3_HIP(e, hipGetLastError());
    }
    for (const Adm& a : grp) {
        const q3tts_request* r = a.r;
        if (!r) continue;  // a prefix job: the slot stays free
        const int b = a.b;
        Q3Lane& L = e->lane;
        const int row = e->row_of_slot[b];
        q3_launch_copy_rows(L.T.x + (size_t)row * m.t_d_model, m.t_d_model, e->pf.x + (size_t)(a.row0 + a.n - 1) * m.t_d_model, m.t_d_model, 1, m.t_d_model, s);
        // the last prompt row's norm inputs for out_norm came out of the last block
        if (q3_launch_gemm(e, e->T, q3_gemm_head(e->T, 0, m.t_vocab, e->pf, a.row0 + a.n - 1, 1, m.rms_eps, 0, L.logits + (size_t)row * m.t_vocab), s))
            return q3_set_err(e, Q3TTS_ERR_INVALID, "prefill head: launch refused for this model shape");
        // sampler stream (src/tts/engine.rs:473-485)
        float temperature = e->temperature, top_p = e->top_p; int top_k = e->top_k, has_seed = e->has_seed; uint64_t seed = e->seed;
        if (!r->use_engine_sampler) { temperature = r->temperature; top_k = r->top_k; top_p = r->top_p; has_seed = r->has_seed; seed = r->seed; }
        if (!has_seed) seed = wall_seed();
        if (temperature > 0.0f) {
            std::vector<float> draws(a.max_steps);
            q3_stdrng_f32(seed, a.max_steps, draws.data());
            Q3_HIP(e, hipMemcpyAsync(e->rng + (size_t)b * e->cfg.max_steps_cap, draws.data(), (size_t)a.max_steps * 4, hipMemcpyHostToDevice, s));
            Q3_HIP(e, hipStreamSynchronize(s));
        }
        if (e->p_temperature > 0.0f) {  // the Predictor's own stream: draw frame * (n_codebooks - 1) + (q - 1) serves code q of that frame
            const size_t per = (size_t)(m.n_codebooks - 1), nd = (size_t)a.max_steps * per;
            std::vector<float> draws(nd);
            q3_stdrng_f32(seed ^ 0x9E3779B97F4A7C15ull, (int)nd, draws.data());
            Q3_HIP(e, hipMemcpyAsync(e->prng + (size_t)b * e->cfg.max_steps_cap * per, draws.data(), nd * 4, hipMemcpyHostToDevice, s));
            Q3_HIP(e, hipStreamSynchronize(s));
        }
        if (e->rep_penalty != 1.0f) Q3_HIP(e, hipMemsetAsync(e->seen + (size_t)b * e->seen_words, 0, (size_t)e->seen_words * 4, s));  // generated codes only: a prompt or a voice prefix leaves it empty
        Q3Slot* st = e->slots_host + e->B + b;  // pinned staging half
        memset(st, 0, sizeof(*st));
        st->active = 1; st->cur_pos = a.P + a.n; st->n_frames = 0; st->max_steps = a.max_steps; st->min_frames = r->min_frames;
        st->force_eos_at = r->force_eos_at; st->top_k = top_k; st->temperature = temperature; st->top_p = top_p;
        st->rng_base = b * e->cfg.max_steps_cap;
        st->p_temperature = e->p_temperature; st->p_top_k = e->p_top_k; st->p_top_p = e->p_top_p; st->rep_penalty = e->rep_penalty;
        Q3_HIP(e, hipMemcpyAsync(e->slots + b, st, sizeof(Q3Slot), hipMemcpyHostToDevice, s));
        if (r->text_stream == 1) {  // the slot's trailing rows; (nothing here until a text_stream request has been seen: the arrays are zero)
            std::vector<int32_t> T;
            q3_text_trailing(r, T);
            TRY(q3_text_rows_set(e, b, T.data(), 0, (int)T.size(), 0));
        } else if (e->ts_used) TRY(q3_text_rows_set(e, b, nullptr, 0, 0, 0));
        e->ts_slot[b] = (r->text_stream == 1) ? 1 : 0;
        if (e->voc) TRY(q3_voc_reset(e, b));
    }
    return Q3TTS_OK;
}

// bytes of one of a prefix's two stores of np positions, in the slots' format: bf16, or Q8_0 quants with their f16 scales behind them
size_t q3_prefix_store_bytes(const q3tts_engine* e, int np) {
    const size_t per = (size_t)e->T.L * e->T.Hkv * np * e->T.hd;
    return e->T.kv8 ? per + per / 16 : per * 2;
}
// the zero-filled store of a prefix that a slot's first `rows` positions will be saved into (k_kv_prefix_save)
static int prefix_store_alloc(q3tts_engine* e, q3tts_prefix* x, int rows) {
    if (e->T.hd != Q3_ATT_HD) return q3_set_err(e, Q3TTS_ERR_INVALID, "prefix: the save kernel needs head_dim 128");
    if (x->k || x->v || x->e != e) return q3_set_err(e, Q3TTS_ERR_INVALID, "prefix: the handle to fill is not an empty one of this engine");
    const int np = (rows + 63) & ~63;
    const size_t store = q3_prefix_store_bytes(e, np);
    int rc = q3_dev_alloc_zeroed(e, (void**)&x->k, store);
    if (rc == Q3TTS_OK) { rc = q3_dev_alloc_zeroed(e, (void**)&x->v, store); if (rc != Q3TTS_OK) e->dev_bytes -= store; }
    if (rc != Q3TTS_OK) { hipFree(x->k); x->k = x->v = nullptr; return rc; }
    x->P = rows; x->np = np;
    return Q3TTS_OK;
}

// items[i] enters its slot; rc[i] = status of item i (a failing item does not stop the others)
static int admit_items(q3tts_engine* e, const Q3AdmItem* items, int count, int* rc) {
    const q3tts_model_config& m = e->cfg.model;
    hipStream_t s = e->stream;
    std::vector<Adm> grp;
    int total = 0;
    for (int i = 0; i < count; ++i) {
        const Q3AdmItem& it = items[i];
        const q3tts_request* r = it.r;
        rc[i] = Q3TTS_OK;
        if (!r) {  // a prefill-only prefix job: 1 <= rows < n_ctx, as q3tts_prefix_create
            if (!it.keep || (it.voice != nullptr) == (it.embd != nullptr)) { rc[i] = q3_set_err(e, Q3TTS_ERR_INVALID, "prefix: give exactly one of a voice desc or host rows"); continue; }
            int n = 0;
            for (int attempt = 0; attempt < 2; ++attempt) {
                const int room = std::min(e->cfg.n_ctx - total, e->cfg.n_ctx - 1);
                if (it.embd) {
                    n = it.n_tok;
                    if (n <= 0 || n >= e->cfg.n_ctx) { rc[i] = q3_set_err(e, Q3TTS_ERR_INVALID, "prefix: n_tok outside 1 .. n_ctx - 1"); break; }
                    if (n <= room) { Q3_HIP(e, hipMemcpyAsync(e->pf.x + (size_t)total * m.d_embed, it.embd, (size_t)n * m.d_embed * 4, hipMemcpyHostToDevice, s)); break; }
                } else {
                    const int brc = build_prompt_dev(e, it.voice, e->pf.x + (size_t)total * m.d_embed, room, &n, PROMPT_VOICE);
                    if (brc == Q3TTS_OK) break;
                    if (total == 0) { rc[i] = brc; break; }
                }
                TRY(admit_group(e, grp, total));  // batch full: flush, then retry this job in an empty batch
                grp.clear(); total = 0;
            }
            if (rc[i] == Q3TTS_OK && n < 1) rc[i] = q3_set_err(e, Q3TTS_ERR_INVALID, "prefix: the voice part has no rows");
            if (rc[i] == Q3TTS_OK) rc[i] = prefix_store_alloc(e, it.keep, n);
            if (rc[i] != Q3TTS_OK) continue;
            grp.push_back(Adm{it.slot, nullptr, n, total, 0, 0, it.keep, n});
            total += n;
            continue;
        }
        const int max_steps = r->max_steps > 0 ? r->max_steps : e->max_steps;
        if (max_steps > e->cfg.max_steps_cap) { rc[i] = q3_set_err(e, Q3TTS_ERR_INVALID, "max_steps exceeds max_steps_cap"); continue; }
        const q3tts_prefix* x = r->prefix;
        if (x && x->e != e) { rc[i] = q3_set_err(e, Q3TTS_ERR_INVALID, "prefix: made by another engine"); continue; }
        if (x && x->state.load(std::memory_order_acquire) != 1) { rc[i] = q3_set_err(e, Q3TTS_ERR_INVALID, "prefix: not ready (a session's pending or failed prefix)"); continue; }
        if (x && it.keep) { rc[i] = q3_set_err(e, Q3TTS_ERR_INVALID, "keep-voice: a request that names a prefix cannot keep one"); continue; }
        if (it.keep && it.keep_rows == 0 && (r->prompt_embd || !r->prompt)) { rc[i] = q3_set_err(e, Q3TTS_ERR_INVALID, "keep-voice: a prompt_embd request states its voice rows"); continue; }
        if (it.keep && it.keep_rows < 0) { rc[i] = q3_set_err(e, Q3TTS_ERR_INVALID, "keep-voice: voice_rows is negative"); continue; }
        const int P = x ? x->P : 0;  // the prefix's rows come first; only the request's own rows enter the prefill buffer
        if ((r->text_open == 1) && !(r->text_stream == 1)) { rc[i] = q3_set_err(e, Q3TTS_ERR_INVALID, "text_open needs text_stream = 1"); continue; }
        if (r->text_stream == 1) {
            if (r->prompt_embd || !r->prompt) { rc[i] = q3_set_err(e, Q3TTS_ERR_INVALID, "text_stream needs a prompt built from ids (prompt), not prompt_embd"); continue; }
            if (r->prompt->n_text < 1 || !r->prompt->text_ids) { rc[i] = q3_set_err(e, Q3TTS_ERR_INVALID, "text_stream: the prompt needs n_text >= 1 (its first text id is the prompt's last row)"); continue; }
            const int trc = ensure_text_frames(e);
            if (trc != Q3TTS_OK) { rc[i] = trc; continue; }
        }
        int n = 0;
        for (int attempt = 0; attempt < 2; ++attempt) {
            const int room = e->cfg.n_ctx - total;
            if (r->prompt_embd) {
                n = r->n_tok;
                if (n <= 0 || P + n > e->cfg.n_ctx) { rc[i] = q3_set_err(e, Q3TTS_ERR_INVALID, "n_tok out of range"); break; }
                if (n > room) { if (total == 0) { rc[i] = q3_set_err(e, Q3TTS_ERR_INVALID, "n_tok out of range"); break; } }
                else { Q3_HIP(e, hipMemcpyAsync(e->pf.x + (size_t)total * m.d_embed, r->prompt_embd, (size_t)n * m.d_embed * 4, hipMemcpyHostToDevice, s)); break; }
            } else if (r->prompt) {
                const int brc = build_prompt_dev(e, r->prompt, e->pf.x + (size_t)total * m.d_embed, room, &n, x ? PROMPT_TEXT : PROMPT_WHOLE, r->text_stream == 1);
                if (brc == Q3TTS_OK) break;
                if (total == 0) { rc[i] = brc; break; }
            } else { rc[i] = q3_set_err(e, Q3TTS_ERR_INVALID, "request has neither prompt_embd nor prompt"); break; }
            TRY(admit_group(e, grp, total));  // batch full: flush, then retry this request in an empty batch
            grp.clear(); total = 0;
        }
        if (rc[i] != Q3TTS_OK) continue;
        if (P + n > e->cfg.n_ctx) { rc[i] = q3_set_err(e, Q3TTS_ERR_INVALID, "prefix + prompt longer than n_ctx"); continue; }
        if (P + n + max_steps > e->cfg.n_ctx) { rc[i] = q3_set_err(e, Q3TTS_ERR_INVALID, "prompt + max_steps exceeds n_ctx"); continue; }
        int keep_rows = 0;
        if (it.keep) {  // the voice part of a whole prompt: everything in front of the text part's n_text + 3 rows (text_stream: 2)
            keep_rows = it.keep_rows > 0 ? it.keep_rows : n - (r->text_stream == 1 ? 2 : r->prompt->n_text + 3);
            if (keep_rows < 1 || keep_rows >= n) { rc[i] = q3_set_err(e, Q3TTS_ERR_INVALID, "keep-voice: voice_rows outside 1 .. n - 1"); continue; }
            rc[i] = prefix_store_alloc(e, it.keep, keep_rows);
            if (rc[i] != Q3TTS_OK) continue;
        }
        grp.push_back(Adm{it.slot, r, n, total, max_steps, P, it.keep, keep_rows});
        total += n;
    }
    return admit_group(e, grp, total);
}

// slots[i] <- reqs[i]; rc[i] = status of request i (a failing request does not stop the others)
static int admit_many(q3tts_engine* e, const int* slots, const q3tts_request* const* reqs, int count, int* rc) {
    std::vector<Q3AdmItem> items(count);
    for (int i = 0; i < count; ++i) { items[i] = Q3AdmItem{}; items[i].slot = slots[i]; items[i].r = reqs[i]; }
    return admit_items(e, items.data(), count, rc);
}

static int admit(q3tts_engine* e, int b, const q3tts_request* r) {
    int rc = Q3TTS_OK;
    int st = admit_many(e, &b, &r, 1, &rc);
    return st != Q3TTS_OK ? st : rc;
}

// ------------------------------------------------------------------------------------------------
// voice prefixes (include/q3tts.h): the Talker runs the voice rows once, at positions 0 .. P - 1, straight into the prefix store — for
// that one run the Talker's cache fields point at the store, a cache of one slot and np = ceil(P / 64) * 64 positions — so no slot's
// state changes. Same launches, same rows, same positions as the whole prompt's prefill: the same K/V bits.
// ------------------------------------------------------------------------------------------------
extern "C" int q3tts_prefix_create(q3tts_engine* e, const q3tts_prompt_desc* p, const float* embd, int32_t n_tok, q3tts_prefix** out) {
    if (!e || !out) return q3_set_err(e, Q3TTS_ERR_INVALID, "null argument");
    Q3_NOT_IN_SESSION(e);
    *out = nullptr;
    if ((p != nullptr) == (embd != nullptr)) return q3_set_err(e, Q3TTS_ERR_INVALID, "prefix: give exactly one of a voice desc or host rows");
    Q3_HIP(e, hipSetDevice(e->cfg.device));
    const q3tts_model_config& m = e->cfg.model;
    hipStream_t s = e->stream;
    const int n_ctx = e->cfg.n_ctx;
    int n = 0;
    if (p) TRY(build_prompt_dev(e, p, e->pf.x, n_ctx - 1, &n, PROMPT_VOICE));
    else {
        if (n_tok <= 0 || n_tok >= n_ctx) return q3_set_err(e, Q3TTS_ERR_INVALID, "prefix: n_tok outside 1 .. n_ctx - 1");
        n = n_tok;
        Q3_HIP(e, hipMemcpyAsync(e->pf.x, embd, (size_t)n * m.d_embed * 4, hipMemcpyHostToDevice, s));
    }
    Q3Tfm& t = e->T;
    q3tts_prefix* x = new q3tts_prefix();
    x->e = e; x->P = n; x->np = (n + 63) & ~63;
    const size_t per = (size_t)t.L * t.Hkv * x->np * t.hd;
    const size_t store = t.kv8 ? per + per / 16 : per * 2;  // the slots' format: bf16, or Q8_0 quants with their f16 scales behind them
    int rc = q3_dev_alloc_zeroed(e, (void**)&x->k, store);
    if (rc == Q3TTS_OK) rc = q3_dev_alloc_zeroed(e, (void**)&x->v, store);
    if (rc != Q3TTS_OK) { hipFree(x->k); hipFree(x->v); delete x; return rc; }
    auto fail = [&](int code, const std::string& msg) { hipStreamSynchronize(s); hipFree(x->k); hipFree(x->v); delete x; return q3_set_err(e, code, msg); };
    std::vector<int> pos(n), zero(n, 0);
    for (int i = 0; i < n; ++i) pos[i] = i;
    uint16_t *kc = t.kc, *vc = t.vc, *kd = t.kd, *vd = t.vd; const size_t ls = t.layer_stride; const int nc = t.n_ctx;
    t.kc = x->k; t.vc = x->v; t.layer_stride = (size_t)t.Hkv * x->np * t.hd; t.n_ctx = x->np;
    if (t.kv8) { t.kd = (uint16_t*)((int8_t*)x->k + per); t.vd = (uint16_t*)((int8_t*)x->v + per); }
    const int rl = prefill_layers(e, pos, zero, {0, n, 0, 0}, n, n, nullptr);
    t.kc = kc; t.vc = vc; t.kd = kd; t.vd = vd; t.layer_stride = ls; t.n_ctx = nc;
    if (rl < 0) return fail(Q3TTS_ERR_DEVICE, std::string(e->err));
    if (rl) return fail(Q3TTS_ERR_INVALID, "prefix: a kernel launch was refused for this model shape");
    hipError_t er = hipGetLastError();
    if (er == hipSuccess) er = hipStreamSynchronize(s);
    if (er != hipSuccess) return fail(Q3TTS_ERR_DEVICE, hipGetErrorString(er));
    *out = x;
    return Q3TTS_OK;
}
extern "C" int32_t q3tts_prefix_rows(const q3tts_prefix* x) { return x && x->state.load(std::memory_order_acquire) == 1 ? x->P : 0; }
extern "C" int32_t q3tts_prefix_state(const q3tts_prefix* x) { return x ? x->state.load(std::memory_order_acquire) : Q3TTS_ERR_INVALID; }
extern "C" int q3tts_prefix_destroy(q3tts_prefix* x) {
    if (!x) return Q3TTS_OK;
    q3tts_engine* e = x->e;
    Q3_NOT_IN_SESSION(e);  // an open session may still admit requests that name it
    hipSetDevice(e->cfg.device);
    hipStreamSynchronize(e->stream);
    hipFree(x->k); hipFree(x->v);
    delete x;
    return Q3TTS_OK;
}

static double now_ms() {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

struct SlotRun { int req = -1; double t_first = 0; };

// H8: the vocoder consumes 4-frame chunks (src/tts/engine.rs:507-541). One chunk boundary of it, shared by q3tts_generate_batch and the
// session worker (q3_session.hip): on the vocoder stream behind ev3 (the frames just decoded), batched over every slot that has a chunk
// ready, so chunk k's PCM overlaps the decoding of chunk k+1. live[b]: slot b holds a request; want[b]: it wants PCM; voc_frames[b]:
// its frames handed to the vocoder so far (advanced here); more: requests wait for a slot. Finished slots (live, inactive) then get
// is_last by the reference's flush rule. *first: some slot got its first frames in this call.
int q3_voc_dispatch(q3tts_engine* e, const char* live, const char* want, int* voc_frames, bool more, bool* first) {
    const int B = e->B;
    hipStream_t vs = e->vstream;
    bool waited = false;
    *first = false;
    auto ensure_wait = [&]() -> int { if (!waited) { Q3_HIP(e, hipStreamWaitEvent(vs, e->ev3, 0)); waited = true; } return Q3TTS_OK; };
    // ONE batched call per chunk: every slot with new frames runs nf = 4. A finished utterance whose tail is
    // shorter is padded with throw-away frames: the vocoder is causal, so they cannot change the samples already
    // due, their own samples are never reported, and the slot's vocoder state is reset at its next admission.
    std::vector<int> list(B), real(B);  // (q3_voc_decode_batch runs more than 64 slots as several calls)
    for (;;) {
        int ns = 0;
        for (int b = 0; b < B; ++b) {
            if (!live[b] || !want[b]) continue;
            const int pend = e->slots_host[b].n_frames - voc_frames[b];
            if (pend >= 4 || (pend > 0 && !e->slots_host[b].active)) { real[ns] = std::min(pend, 4); list[ns++] = b; }
        }
        if (!ns) break;
        TRY(ensure_wait());
        int still = 0;  // slots that go on decoding while this call runs
        for (int b = 0; b < B; ++b) if (live[b] && e->slots_host[b].active) ++still;
        TRY(q3_voc_decode_batch(e, list.data(), real.data(), ns, 4, vs, (still > 0 || more) ? 1 : 0));
        for (int i = 0; i < ns; ++i) { if (voc_frames[list[i]] == 0) *first = true; voc_frames[list[i]] += real[i]; }
    }
    // V4 flush: the reference sends is_last only when its final buffer is not empty, i.e. n_frames % 4 != 0 (src/tts/engine.rs:510-536,
    // restated by q3o_chunk_plan); with lookahead_frames > 0 an utterance of n_frames % 4 == 0 keeps its withheld tail (vocoder_flush_tail = 1: always flush)
    for (int b = 0; b < B; ++b)
        if (live[b] && !e->slots_host[b].active && (e->cfg.vocoder_flush_tail || e->slots_host[b].n_frames % 4 != 0)) q3_voc_mark_last(e, b);
    return Q3TTS_OK;
}

// Pinned result buffers are recycled through a small process-wide pool: hipHostMalloc / hipHostFree cost ~0.3 ms each, and a
// batch hands out one PCM buffer per utterance. A 64-byte header in front of the payload remembers the capacity.
#include <mutex>
namespace {
struct PinHdr { size_t cap; size_t magic; };
std::mutex g_pin_mu;
std::vector<PinHdr*> g_pin_pool;
size_t g_pin_bytes = 0;
float* pin_alloc(size_t bytes) {
    {
        std::lock_guard<std::mutex> lk(g_pin_mu);
        for (size_t i = 0; i < g_pin_pool.size(); ++i)
            if (g_pin_pool[i]->cap >= bytes && g_pin_pool[i]->cap <= 2 * bytes + 4096) {
                PinHdr* h = g_pin_pool[i];
                g_pin_pool[i] = g_pin_pool.back(); g_pin_pool.pop_back(); g_pin_bytes -= h->cap;
                return (float*)((char*)h + 64);
            }
    }
    void* p = nullptr;
    const size_t cap = (bytes + 65535) & ~(size_t)65535;
    if (hipHostMalloc(&p, cap + 64, hipHostMallocDefault) != hipSuccess) return nullptr;
    PinHdr* h = (PinHdr*)p; h->cap = cap; h->magic = 0x5133505043ull;
    return (float*)((char*)p + 64);
}
void pin_free(float* q) {
    if (!q) return;
    PinHdr* h = (PinHdr*)((char*)q - 64);
    if (h->magic != 0x5133505043ull) return;  // not ours: leave it alone
    std::lock_guard<std::mutex> lk(g_pin_mu);
    if (g_pin_pool.size() < 256 && g_pin_bytes + h->cap <= ((size_t)1 << 30)) { g_pin_pool.push_back(h); g_pin_bytes += h->cap; return; }
    hipHostFree(h);
}
}  // namespace

// Results of a finished slot. The codes come back on the decoder stream at once; the PCM (pinned host buffer) is copied
// on the vocoder stream. With `defer` the call does not wait for the vocoder: the copy is enqueued behind the slot's last
// vocoder chunk, `fin_ev` is recorded after it and the caller completes the result later (complete_result), so the next
// decode chunk is launched while the vocoder is still working.
static int finalize(q3tts_engine* e, int b, const q3tts_request* r, q3tts_result* o, const SlotRun& sr, double t0, bool defer = false,
                    hipEvent_t fin_ev = nullptr, int ri = -1) {
    const int ncb = e->cfg.model.n_codebooks;
    const Q3Slot& st = e->slots_host[b];
    o->n_frames = st.n_frames; o->hit_eos = st.hit_eos;
    o->codes = (int32_t*)malloc(sizeof(int32_t) * (size_t)std::max(1, st.n_frames * ncb));
    if (!o->codes) return q3_set_err(e, Q3TTS_ERR_OOM, "malloc");
    if (st.n_frames > 0)
        Q3_HIP(e, hipMemcpyAsync(o->codes, e->codes + (size_t)b * e->cfg.max_steps_cap * ncb, sizeof(int32_t) * (size_t)st.n_frames * ncb,
                                 hipMemcpyDeviceToHost, e->stream));
    o->sample_rate = e->out_rate && e->voc ? e->out_rate : e->cfg.vocoder.sample_rate;
    if (r->want_pcm && e->voc && e->dev_pcm && ri >= 0 && ri < e->dev_pcm_n) {
        // device copy of the utterance's PCM (q3tts_set_device_pcm): row ri of the packed buffer, for collectives that read device memory
        const int ns = q3_voc_samples(e, b);
        if (ns > 0) Q3_HIP(e, hipMemcpyAsync(e->dev_pcm + (size_t)ri * e->dev_pcm_stride, q3_voc_pcm(e, b), sizeof(float) * (size_t)ns, hipMemcpyDeviceToDevice, e->vstream));
    }
    if (r->want_pcm == 2 && e->voc) {  // device only: no host copy
        o->n_samples = q3_voc_samples(e, b);
        if (defer) Q3_HIP(e, hipEventRecord(fin_ev, e->vstream));
        else Q3_HIP(e, hipStreamSynchronize(e->vstream));
    } else if (r->want_pcm && e->voc) {
        int ns = q3_voc_samples(e, b);
        const float* from = q3_voc_pcm(e, b);
        if (e->out_rate) {  // the finished row at the output rate: N(ns) samples through the slot's staging row
            const int no = (int)q3_resample_N(ns, e->rs_out.L, e->rs_out.M);
            TRY(q3_resample_slot(e, b, 0, no, ns, true, e->vstream));
            ns = no; from = e->rs_stage + (size_t)b * e->rs_stage_stride;
        }
        o->n_samples = ns;
        o->pcm = pin_alloc(sizeof(float) * (size_t)std::max(1, ns));
        if (!o->pcm) return q3_set_err(e, Q3TTS_ERR_OOM, "hipHostMalloc");
        if (ns > 0) Q3_HIP(e, hipMemcpyAsync(o->pcm, from, sizeof(float) * (size_t)ns, hipMemcpyDeviceToHost, e->vstream));
        if (defer) Q3_HIP(e, hipEventRecord(fin_ev, e->vstream));
        else Q3_HIP(e, hipStreamSynchronize(e->vstream));
    } else if (defer) {
        Q3_HIP(e, hipEventRecord(fin_ev, e->vstream));
    }
    Q3_HIP(e, hipStreamSynchronize(e->stream));
    o->first_chunk_ms = sr.t_first > 0 ? (float)(sr.t_first - t0) : 0.0f;
    o->total_ms = (float)(now_ms() - t0);
    o->status = defer ? Q3TTS_ERR_STATE : Q3TTS_OK;  // a deferred result becomes OK in complete_result
    return Q3TTS_OK;
}

static int complete_result(q3tts_engine* e, q3tts_result* o, hipEvent_t fin_ev, double t0) {
    Q3_HIP(e, hipEventSynchronize(fin_ev));
    o->total_ms = (float)(now_ms() - t0);
    o->status = Q3TTS_OK;
    return Q3TTS_OK;
}

extern "C" int q3tts_generate_batch(q3tts_engine* e, const q3tts_request* reqs, int32_t n, q3tts_result* outs) {
    if (!e || !reqs || !outs || n <= 0) return q3_set_err(e, Q3TTS_ERR_INVALID, "null/empty argument");
    Q3_NOT_IN_SESSION(e);
    Q3_HIP(e, hipSetDevice(e->cfg.device));
    for (int i = 0; i < n; ++i) { memset(&outs[i], 0, sizeof(outs[i])); outs[i].status = Q3TTS_ERR_STATE; }
    for (int i = 0; i < n; ++i) {
        if (reqs[i].want_pcm && !e->voc) return q3_set_err(e, Q3TTS_ERR_STATE, "want_pcm on an engine created with with_vocoder = 0");
        if (reqs[i].want_pcm == 2 && !e->dev_pcm_on) return q3_set_err(e, Q3TTS_ERR_STATE, "want_pcm = 2 (device only) needs q3tts_set_device_pcm(engine, 1)");
        if (reqs[i].text_open == 1) return q3_set_err(e, Q3TTS_ERR_INVALID, "text_open = 1 is for sessions (q3tts_session_append_text): this call takes closed text and never waits");
    }
    std::fill(e->ts_slot.begin(), e->ts_slot.end(), 0);  // nothing is in flight
    if (e->dev_pcm_on && e->voc) {  // one row of max_steps_cap frames per request of this call
        const size_t stride = (size_t)e->cfg.max_steps_cap * q3_voc_samples_per_frame(e);
        if (e->dev_pcm_n < n || e->dev_pcm_stride != stride) {
            if (e->dev_pcm) { Q3_HIP(e, hipStreamSynchronize(e->vstream)); hipFree(e->dev_pcm); e->dev_pcm = nullptr; e->dev_pcm_n = 0; }
            void* p = nullptr;
            if (hipMalloc(&p, (size_t)n * stride * sizeof(float)) != hipSuccess) return q3_set_err(e, Q3TTS_ERR_OOM, "hipMalloc (device PCM)");
            e->dev_pcm = (float*)p; e->dev_pcm_n = n; e->dev_pcm_stride = stride;
        }
    }
    const int B = e->B, CH = 4;  // 4-frame chunks: src/tts/engine.rs:509-512
    const int spf = e->voc ? q3_voc_samples_per_frame(e) : 0;
    std::vector<SlotRun> run(B);
    std::vector<int> voc_frames(B, 0);
    std::vector<char> live(B, 0), want(B, 0);
    const double t0 = now_ms();
    std::vector<int> pending(B, -1);  // request whose PCM copy is still in flight on the vocoder stream, per slot
    auto drain = [&](int b) -> int {
        if (pending[b] >= 0) { TRY(complete_result(e, &outs[pending[b]], e->fin_ev[b], t0)); pending[b] = -1; }
        return Q3TTS_OK;
    };
    int next = 0, done = 0;
    double dec_ms = 0, pre_ms = 0, voc_ms = 0;
    static const bool host_prof = [] { const char* ev = getenv("Q3TTS_HOST_PROF"); return ev && atoi(ev); }();  // host wall time per phase of this loop, to stderr
    double hp_admit = 0, hp_chunk = 0, hp_voc = 0, hp_fin = 0, hp_tail = 0, hp_t = now_ms();
    auto hp_lap = [&](double& acc) { if (host_prof) { const double t = now_ms(); acc += t - hp_t; hp_t = t; } };
    long long steps = 0, ctx_tokens = 0, live_slot_steps = 0;
    e->probe_ms = 0; e->probe_cnt = 0; e->row_steps = 0; e->probe_empty_ms = 0; e->probe_empty_cnt = 0;
    hipStream_t s = e->stream;
    while (done < n) {
        bool admitted = false;
        {
            std::vector<int> as, ai; std::vector<const q3tts_request*> ar;
            for (int b = 0; b < B && next < n; ++b)
                if (run[b].req < 0) { TRY(drain(b)); as.push_back(b); ar.push_back(&reqs[next]); ai.push_back(next++); }
            {
                std::vector<int> live(as);
                for (int b = 0; b < B; ++b) if (run[b].req >= 0) live.push_back(b);
                TRY(plan_rows(e, live));
            }
            if (!as.empty()) {
                Q3_HIP(e, hipEventRecord(e->ev0, s));
                admitted = true;
                std::vector<int> rcs(as.size());
                TRY(admit_many(e, as.data(), ar.data(), (int)as.size(), rcs.data()));
                for (size_t i = 0; i < as.size(); ++i) {
                    if (rcs[i] != Q3TTS_OK) { outs[ai[i]].status = rcs[i]; ++done; }
                    else { run[as[i]] = SlotRun{}; run[as[i]].req = ai[i]; voc_frames[as[i]] = 0; }
                }
            }
        }
        if (admitted) { Q3_HIP(e, hipEventRecord(e->ev2, s)); }
        hp_lap(hp_admit);
        bool any = false;
        for (int b = 0; b < B; ++b) if (run[b].req >= 0) any = true;
        if (!any) break;
        float ms = 0;
        TRY(run_chunk(e, CH, &ms));
        hp_lap(hp_chunk);
        dec_ms += ms; steps += CH;
        if (admitted) { hipEventElapsedTime(&ms, e->ev0, e->ev2); pre_ms += ms; }
        for (int b = 0; b < B; ++b) if (run[b].req >= 0) { ctx_tokens += (long long)e->slots_host[b].cur_pos * CH; live_slot_steps += CH; }
        if (e->voc) {
            const double tv0 = now_ms();
            hipStream_t vs = e->vstream;
            for (int b = 0; b < B; ++b) { live[b] = run[b].req >= 0; want[b] = live[b] && reqs[run[b].req].want_pcm; }
            bool first = false;
            TRY(q3_voc_dispatch(e, live.data(), want.data(), voc_frames.data(), next < n, &first));
            if (first) {  // first-chunk latency: the first chunk's PCM resident on the host
                for (int b = 0; b < B; ++b)
                    if (run[b].req >= 0 && run[b].t_first == 0 && voc_frames[b] > 0) {
                        const int nsmp = std::min(voc_frames[b], 4) * spf;
                        Q3_HIP(e, hipMemcpyAsync(e->first_chunk_host, q3_voc_pcm(e, b), sizeof(float) * (size_t)nsmp, hipMemcpyDeviceToHost, vs));
                    }
                Q3_HIP(e, hipStreamSynchronize(vs));
                const double tn = now_ms();
                for (int b = 0; b < B; ++b) if (run[b].req >= 0 && run[b].t_first == 0 && voc_frames[b] > 0) run[b].t_first = tn;
            }
            voc_ms += now_ms() - tv0;
        }
        hp_lap(hp_voc);
        // results whose PCM copy has landed are completed now, so total_ms is an utterance's own latency (to one chunk's granularity)
        for (int j = 0; j < B; ++j)
            if (pending[j] >= 0 && hipEventQuery(e->fin_ev[j]) == hipSuccess) TRY(drain(j));
        for (int b = 0; b < B; ++b) {
            if (run[b].req < 0 || e->slots_host[b].active) continue;
            // (the V4 flush rule was applied by q3_voc_dispatch)
            // hand the slot's results over without waiting for the vocoder (completed at slot reuse / at the end)
            for (int j = 0; j < B; ++j)
                if (pending[j] >= 0 && hipEventQuery(e->fin_ev[j]) == hipSuccess) TRY(drain(j));
            TRY(finalize(e, b, &reqs[run[b].req], &outs[run[b].req], run[b], t0, true, e->fin_ev[b], run[b].req));
            pending[b] = run[b].req;
            run[b].req = -1; ++done;
            e->ts_slot[b] = 0;
        }
        hp_lap(hp_fin);
    }
    for (int b = 0; b < B; ++b) TRY(drain(b));
    hp_lap(hp_tail);
    if (host_prof) {
        fprintf(stderr, "q3tts_generate_batch host wall (ms): admit + plan %.1f | chunks (launch + wait) %.1f = launch %.1f + wait %.1f, device events %.1f over %lld steps | vocoder issue %.1f | finalize %.1f | tail (last results) %.1f | total %.1f\n",
                hp_admit, hp_chunk, e->hp_launch, e->hp_sync, dec_ms, steps, hp_voc, hp_fin, hp_tail, now_ms() - t0);
        e->hp_launch = e->hp_sync = 0;
    }
    e->tm.prefill_ms = (float)pre_ms; e->tm.decode_ms = (float)dec_ms; e->tm.vocoder_ms = (float)voc_ms;
    e->tm.total_ms = (float)(now_ms() - t0); e->tm.frame_steps = steps; e->tm.frame_step_ms = steps ? (float)(dec_ms / steps) : 0.0f;
    // bytes = 2*W_T + 15*2*W_P(layers) + 15*2*h + 16*2*pj + KV bytes of the live context + gathers
    {
        const q3tts_model_config& m = e->cfg.model;
        const long long wt = (long long)e->T.weight_bytes;  // includes lm_head
        const double bpw_p = e->P.q8 ? 1.0625 : 2.0;  // the Predictor's bytes per weight (predictor_q8_0 = 2: Q8_0 blocks)
        const long long wp_layers = (long long)e->P.weight_bytes - (long long)(bpw_p * (double)((size_t)e->P.head_n * m.p_d_model));
        const long long head1 = (long long)(bpw_p * (double)((size_t)m.codebook_size * m.p_d_model)), pj = 2ll * m.p_d_model * m.d_embed;
        const long long kv_per_tok = 2ll * m.t_n_layer * 2 * m.t_n_kv_head * m.t_head_dim;
        long long fixed = wt + (m.n_codebooks - 1) * (wp_layers + head1) + pj;  // one projection GEMM per frame (hidden rows); codes come pre-projected
        e->tm.mean_live_slots = steps ? (float)((double)live_slot_steps / (double)steps) : 0.0f;
        long long gathered = 0;  // with the layer-0 QKV table, passes 1 .. n_codebooks - 2 do not stream wqkv[0]: every live row reads its table row instead
        if (q3_pred_table_on(e)) {
            fixed -= (long long)(m.n_codebooks - 2) * (long long)(bpw_p * (double)((size_t)e->P.nqkv * m.p_d_model));
            gathered = (long long)((double)(m.n_codebooks - 2) * (double)e->tm.mean_live_slots * (double)e->P.nqkv * 4.0);
        }
        e->tm.algo_bytes_per_step = fixed + gathered + (steps ? kv_per_tok * (ctx_tokens / steps) : 0);
        e->tm.algo_flops_per_step = (long long)((double)fixed * (double)e->tm.mean_live_slots);  // 2 flop per bf16 weight (2 bytes) per live row
        e->tm.mean_rows = steps ? (float)((double)e->row_steps / (double)steps) : 0.0f;
        e->tm.mean_ctx_tokens = steps ? (float)((double)ctx_tokens / (double)steps) : 0.0f;
        e->tm.probe_kernel_ms = e->probe_cnt ? (float)(e->probe_ms / (double)e->probe_cnt) : 0.0f;
        e->tm.probe_count = e->probe_cnt;
        e->tm.probe_empty_ms = e->probe_empty_cnt ? (float)(e->probe_empty_ms / (double)e->probe_empty_cnt) : 0.0f;
    }
    return Q3TTS_OK;
}

// the scheduler steps as the session worker drives them (q3_session.hip)
int q3_plan_rows(q3tts_engine* e, const std::vector<int>& live) { return plan_rows(e, live); }
int q3_admit_many(q3tts_engine* e, const int* slots, const q3tts_request* const* reqs, int count, int* rc) { return admit_many(e, slots, reqs, count, rc); }
int q3_admit_items(q3tts_engine* e, const Q3AdmItem* items, int count, int* rc) { return admit_items(e, items, count, rc); }
int q3_run_chunk(q3tts_engine* e, int CH) { return run_chunk(e, CH, nullptr); }
double q3_now_ms() { return now_ms(); }

extern "C" int q3tts_generate(q3tts_engine* e, const q3tts_request* req, q3tts_result* out) {
    int rc = q3tts_generate_batch(e, req, 1, out);
    if (rc != Q3TTS_OK) return rc;
    return out->status;
}

extern "C" void q3tts_result_free(q3tts_result* r) {
    if (!r) return;
    free(r->codes);
    pin_free(r->pcm);  // pinned (filled by an asynchronous device-to-host copy); goes back to the pool
    r->codes = nullptr; r->pcm = nullptr;
}

extern "C" int q3tts_get_timings(const q3tts_engine* e, q3tts_timings* out) {
    if (!e || !out) return Q3TTS_ERR_INVALID;
    *out = e->tm;
    return Q3TTS_OK;
}

// ------------------------------------------------------------------------------------------------
// streaming (H8): 4-frame chunks
// ------------------------------------------------------------------------------------------------
struct q3tts_stream {
    q3tts_engine* e; q3tts_request req; int voc_frames = 0; bool finished = false; bool final_sent = false;
    std::vector<float> chunk; double t0 = 0, t_first = 0;
    long long delivered = 0;  // output-rate samples handed out so far (q3tts_set_output_rate)
};

// the samples a poll hands out into st->chunk: the slot's new PCM [before, after), or with an output rate set the outputs the row can
// deliver now (D(after), N(after) when `fin`) beyond those delivered
static int stream_emit(q3tts_stream* st, int before, int after, bool fin, const float** chunk, int32_t* n_samples) {
    q3tts_engine* e = st->e;
    hipStream_t s = e->stream;
    const float* from = q3_voc_pcm(e, 0) + before;
    int c = after - before;
    if (e->out_rate) {
        const Q3Resamp& r = e->rs_out;
        c = (int)((fin ? q3_resample_N(after, r.L, r.M) : q3_resample_D(after, r.L, r.M, r.H)) - st->delivered);
        TRY(q3_resample_slot(e, 0, st->delivered, c, after, fin, s));
        from = e->rs_stage;
        st->delivered += std::max(c, 0);
    }
    st->chunk.resize((size_t)std::max(1, c));
    if (c > 0) Q3_HIP(e, hipMemcpyAsync(st->chunk.data(), from, sizeof(float) * (size_t)c, hipMemcpyDeviceToHost, s));
    Q3_HIP(e, hipStreamSynchronize(s));
    *chunk = st->chunk.data(); *n_samples = std::max(c, 0);
    return Q3TTS_OK;
}

extern "C" int q3tts_stream_begin(q3tts_engine* e, const q3tts_request* req, q3tts_stream** out) {
    if (!e || !req || !out) return q3_set_err(e, Q3TTS_ERR_INVALID, "null argument");
    Q3_NOT_IN_SESSION(e);
    if (!e->voc) return q3_set_err(e, Q3TTS_ERR_STATE, "streaming needs with_vocoder = 1");
    if (req->text_open == 1) return q3_set_err(e, Q3TTS_ERR_INVALID, "text_open = 1 is for sessions (q3tts_session_append_text): a stream takes closed text and never waits");
    Q3_HIP(e, hipSetDevice(e->cfg.device));
    std::fill(e->ts_slot.begin(), e->ts_slot.end(), 0);  // nothing else is in flight
    q3tts_stream* st = new q3tts_stream();
    st->e = e; st->req = *req; st->t0 = now_ms();
    int rc = plan_rows(e, std::vector<int>{0});
    if (rc == Q3TTS_OK) rc = admit(e, 0, req);
    if (rc != Q3TTS_OK) { delete st; return rc; }
    ++e->streams_open;
    *out = st;
    return Q3TTS_OK;
}

extern "C" int q3tts_stream_poll(q3tts_stream* st, const float** chunk, int32_t* n_samples, int32_t* is_final) {
    if (!st || !chunk || !n_samples || !is_final) return q3_set_err(nullptr, Q3TTS_ERR_INVALID, "null argument");
    q3tts_engine* e = st->e;
    *chunk = nullptr; *n_samples = 0; *is_final = 0;
    if (st->final_sent) { *is_final = 1; return Q3TTS_OK; }
    hipStream_t s = e->stream;
    const int spf = q3_voc_samples_per_frame(e);
    for (;;) {
        const Q3Slot& sl = e->slots_host[0];
        if (!st->finished) {
            TRY(run_chunk(e, 4, nullptr));
            if (!sl.active) st->finished = true;
        }
        int nf = 0, last = 0;
        if (sl.n_frames - st->voc_frames >= 4) nf = 4;
        else if (st->finished && sl.n_frames > st->voc_frames) { nf = sl.n_frames - st->voc_frames; last = 1; }
        // (a last chunk of exactly 4 frames goes without is_last, as the reference's vocoder thread sends it: src/tts/engine.rs:510-536;
        // vocoder_flush_tail = 1 flushes the look-ahead tail with it)
        if (nf == 4 && st->finished && st->voc_frames + 4 >= sl.n_frames && e->cfg.vocoder_flush_tail) last = 1;
        if (nf > 0) {
            const int before = q3_voc_samples(e, 0);
            TRY(q3_voc_decode(e, 0, st->voc_frames, nf, last, s));
            st->voc_frames += nf;
            const int after = q3_voc_samples(e, 0);
            const bool fin = st->finished && st->voc_frames >= sl.n_frames;
            TRY(stream_emit(st, before, after, fin, chunk, n_samples));
            if (st->t_first == 0) st->t_first = now_ms();
            if (fin) { *is_final = 1; st->final_sent = true; }
            (void)spf;
            return Q3TTS_OK;
        }
        if (st->finished) {
            // EOS arrived with no frames left over: the withheld look-ahead tail (vocoder_flush_tail) and, with an output rate set, the
            // outputs whose windows waited for more input go out as a last chunk of their own
            const int before = q3_voc_samples(e, 0);
            if (e->cfg.vocoder_flush_tail) q3_voc_mark_last(e, 0);
            const int after = q3_voc_samples(e, 0);
            if (after > before || (e->out_rate && q3_resample_N(after, e->rs_out.L, e->rs_out.M) > st->delivered))
                TRY(stream_emit(st, before, after, true, chunk, n_samples));
            *is_final = 1; st->final_sent = true; return Q3TTS_OK;
        }
    }
}

extern "C" int q3tts_stream_end(q3tts_stream* st, q3tts_result* out) {
    if (!st) return Q3TTS_ERR_INVALID;
    q3tts_engine* e = st->e;
    int rc = Q3TTS_OK;
    // make sure the slot is retired even if the caller stops early
    Q3Slot* stage = e->slots_host + e->B;
    memset(stage, 0, sizeof(Q3Slot));
    hipMemcpyAsync(e->slots_host, e->slots, sizeof(Q3Slot), hipMemcpyDeviceToHost, e->stream);
    hipStreamSynchronize(e->stream);
    if (out) {
        memset(out, 0, sizeof(*out));
        SlotRun sr; sr.t_first = st->t_first;
        q3tts_request r = st->req; r.want_pcm = 1;
        rc = finalize(e, 0, &r, out, sr, st->t0);
    }
    hipMemcpyAsync(e->slots, stage, sizeof(Q3Slot), hipMemcpyHostToDevice, e->stream);
    hipStreamSynchronize(e->stream);
    --e->streams_open;
    e->ts_slot[0] = 0;
    delete st;
    return rc;
}

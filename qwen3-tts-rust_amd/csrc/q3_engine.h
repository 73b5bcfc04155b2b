// q3_engine.h — internal engine state of libq3tts (host side, C++). The public surface is include/q3tts.h.
#pragma once
#include <algorithm>
#include <cstddef>
#include <atomic>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/q3tts.h"
#include "q3_kernels.h"

// text_stream / text_open live in the alignment gaps of q3tts_request (include/q3tts.h): the struct's size and every other offset are what they were
static_assert(sizeof(q3tts_request) == 80 && offsetof(q3tts_request, text_stream) == 12 && offsetof(q3tts_request, prompt) == 16 &&
              offsetof(q3tts_request, text_open) == 44 && offsetof(q3tts_request, seed) == 48 && offsetof(q3tts_request, prefix) == 72, "q3tts_request layout");

struct Q3Voc;  // vocoder (q3_vocoder.hip)
struct Q3Mel;  // log-mel front-end (q3_mel.hip)
struct Q3Clone;  // voice-clone encoders (q3_clone.hip)

// a K/V cache: the engine's own (Q3Tfm::cache, q3_tfm_init) or a voice prefix's store seen as one (q3_admit.hip)
struct Q3KvCache {
    uint16_t *kc = nullptr, *vc = nullptr;  // [L][slots][Hkv][n_ctx*hd]
    size_t layer_stride = 0;
    // cfg.kv_q8_0 (the Talker only): the cache is ggml Q8_0 blocks — kc / vc hold int8 quants (layer_stride BYTES per layer) and
    // kd / vd the f16 block scales [L][slots][Hkv][n_ctx*hd/32], which follow the quants in the same allocation. q3_layer_cache does the arithmetic.
    bool kv8 = false; uint16_t *kd = nullptr, *vd = nullptr;
    int n_ctx = 0, n_slots = 0;
};

struct Q3Tfm {
    int L = 0, d = 0, Hq = 0, Hkv = 0, hd = 0, F = 0, nq = 0, nkv = 0, nqkv = 0, head_n = 0;
    std::vector<float*> attn_norm, ffn_norm, qn, kn;
    std::vector<uint4*> wqkv, wo, wgu, wd;
    float* out_norm = nullptr;
    uint4* head = nullptr;
    // Q8_0 mode (cfg.talker_q8_0 / cfg.predictor_q8_0): the matrices above hold ggml block quants in the tiled Q8 layout (q3_kernels.h) and
    // these the f16 block scales [N][K/32]; empty / null = bf16 weights
    std::vector<uint16_t*> sqkv, so, sgu, sd; uint16_t* shead = nullptr; bool q8 = false;
    bool a8 = false;  // cfg.talker_q8_0 = 2 / cfg.predictor_q8_0 = 2: the GEMMs' ACTIVATIONS are Q8_0 blocks as well (W8A8, q3_bgemm8.hip): every operand buffer then holds int8 quants + f32 block scales (11-bit significand: q3_q8_sig11)
    Q3KvCache cache;
    float *cs = nullptr, *sn = nullptr;  // RoPE tables [cache.n_ctx][hd/2]
    size_t weight_bytes = 0;              // bf16 matrix bytes of all layers + head
};

struct Q3Scratch {
    float* qkv = nullptr;                   // [rows][nqkv] f32 (the attention kernel's input)
    uint16_t *att = nullptr, *h = nullptr;  // bf16 rows: attention output [rows][nq], SwiGLU output [rows][F] (GEMM operands)
    float *asc_att = nullptr, *asc_h = nullptr; int rt16 = 0;  // W8A8: the f32 block scales of att / h (q3_q8_scale_idx), row tiles of the buffers
    int rows = 0;
};

// a set of f32 residual rows and the operand of the GEMMs that read them: their norm inputs for the next RMSNorm weight
struct Q3Rows {
    float* x = nullptr;                        // [rows][d] f32
    uint16_t* xb = nullptr;                    // bf16(x * nw), A-tiled in whole 16-row tiles (W8A8: int8 quants)
    float* ssp = nullptr;                      // per-tile sums of squares [rows][d / 16]
    float* ascale = nullptr; int rt16 = 0;     // W8A8: the f32 block scales of xb (null otherwise); row tiles of xb
};

// the decode rows: per-row buffers, the row -> slot map and one captured frame-step graph per row-count bucket
struct Q3Lane {
    int nb = 0;                       // row capacity = max_batch
    hipStream_t stream = nullptr;
    Q3Rows T, P;                      // the Talker's rows [nb] and the Predictor's [2 nb]
    float *logits = nullptr, *logits_tmp = nullptr, *fb = nullptr;
    unsigned long long* keys = nullptr;
    int *row_pos_t = nullptr, *slot_id = nullptr, *perm = nullptr;
    Q3Scratch sc;
    float* plogits = nullptr;                // [nb][codebook_size] f32: a Predictor head's logits when the Predictor samples (Q3_EPI_STORE)
    std::vector<hipGraph_t> graphs;          // per bucket
    std::vector<hipGraphExec_t> execs;
    std::vector<hipGraph_t> graphs_s;        // the same frame step with the sampling Predictor (captured when it is first turned on)
    std::vector<hipGraphExec_t> execs_s;
    // the frame step whose last k_pred_next pass takes streamed text rows, per Predictor variant: captured when the first
    // text_stream request is admitted under that variant, kept afterwards. graphs / execs / graphs_s / execs_s are never touched by it.
    std::vector<hipGraph_t> graphs_t[2];
    std::vector<hipGraphExec_t> execs_t[2];
    hipEvent_t ev_begin = nullptr, ev_end = nullptr;
};

struct q3tts_engine {
    q3tts_engine_config cfg;
    std::string err;
    hipStream_t stream = nullptr, vstream = nullptr;
    std::vector<void*> allocs;          // every q3_dalloc of this engine, freed by q3tts_engine_destroy
    size_t dev_bytes = 0;               // bytes handed out by q3_dev_alloc_zeroed so far (q3tts_k_device_bytes)
    Q3Tfm T, P;
    // assets
    float* text = nullptr;
    std::vector<float*> codec;            // host array of device pointers
    const float** codec_dev = nullptr;    // device array of the same pointers
    std::vector<float*> pproj;            // proj(codec table q) [rows_q][p_d_model] f32: the Predictor's inputs are gathers
    float* proj_w = nullptr;              // f32 [p_d_model][d_embed], as the reference keeps it (src/assets_manager.rs:212-241)
    float* proj_b = nullptr;
    // The Predictor's layer-0 QKV of every input row a code can select (q3_pred_table_init): qkv0 [n_codebooks - 2][codecq_rows + 1]
    // [P.nqkv] f32 — slice q - 1, row c = block 0's raw q / k / v for the row pproj[q][c], its last row the same for proj_b (a code out of range).
    // Null: no table (Q3TTS_PRED_TABLE=0, a table above Q3TTS_PRED_TABLE_MAX_MB, a W8A8 Predictor): the frame step keeps k_pred_next(q) and block 0's QKV GEMM.
    float* qkv0 = nullptr;
    float* tts_pad = nullptr;             // = text[tts_pad_id] (or a row of zeros of its own, when the loaded text table is too small)
    float* marker_row = nullptr;          // text[tts_pad_id] through the out-of-range rule (the clone prompt's per-frame marker)
    // decode state: B = max_batch slots. A frame step runs on `rows` = the smallest bucket (1, 2, 4, ... B) that holds
    // the live slots: rows [0, n_live) carry the live slots, the rest carry distinct idle slots (row -> slot map on the
    // device), so a draining batch stops paying for rows it no longer has.
    int B = 0;
    std::vector<int> buckets; int cur_bucket = -1;
    std::vector<std::atomic<long long>> bucket_steps;  // frame steps run on each bucket since creation (q3tts_k_bucket_steps: read from any thread while a session's worker counts)
    std::atomic<long long> kvp_launches{0}, kvp_group_max{0};  // k_kv_prefix launches since creation; the most prefixed requests one prefill group held (q3tts_k_prefix_stats)
    std::vector<int> row_of_slot, slot_of_row;
    Q3Slot* slots = nullptr;              // device [B]
    Q3Slot* slots_host = nullptr;         // pinned mirror [B] + staging [B]
    int* codes = nullptr;                 // [B][max_steps_cap][ncb]
    float* rng = nullptr;                 // [B][max_steps_cap]
    Q3Lane lane;
    Q3Scratch sc_pre;
    // prefill
    Q3Rows pf;                            // the prefill rows [n_ctx] (x also receives the prompt builder's rows)
    int *pf_pos = nullptr, *pf_slot = nullptr;
    int* pf_seg = nullptr;              // the prefill launch's rows as per-slot runs {first row, n, slot, first position} (device, 4 ints each): prefill_layers uploads it and hands it to q3_run_layers
    Q3PromptRow* prow_dev = nullptr; int prow_cap = 0;
    float* spk_dev = nullptr; int* refcodes_dev = nullptr;
    // sampler defaults (SamplerConfig::default: src/tts/engine.rs:25-34)
    float temperature = 0.7f; int top_k = 40; float top_p = 0.9f; int has_seed = 0; uint64_t seed = 0;
    int max_steps = 512;
    // the Predictor's sampler and the code-0 repetition penalty (include/q3tts.h; the reference has neither): snapshotted into a request's
    // slot at admission. pred_variant: which frame step runs — 0 the ARGMAX heads + k_pred_next<false>, 1 STORE heads + k_pred_next<true>;
    // = (p_temperature > 0 || pred_force), fixed while anything is in flight (the setters are refused then)
    float p_temperature = 0.0f; int p_top_k = 0; float p_top_p = 1.0f; float rep_penalty = 1.0f;
    int pred_force = 0, pred_variant = 0;
    int streams_open = 0;                 // q3tts_stream_begin .. q3tts_stream_end
    // streamed text (include/q3tts.h, "streaming text input"; Q3TextRows): the slots' trailing ids, counts and cursors on the device.
    // ts_slot[b]: slot b's last admission was a text_stream request — while any is set, run_chunk runs the text form of the frame step
    // (ts_variant = 1: what q3_record_frame issues / q3_capture_frames captures). ts_used: a text_stream request was admitted at some time
    // (from then on every admission resets its slot's count and cursor).
    int* ts_ids = nullptr; int* ts_cnt = nullptr; int2* ts_cur = nullptr;
    std::vector<char> ts_slot; int ts_variant = 0, ts_used = 0;
    float* prng = nullptr;                // [B][max_steps_cap * (n_codebooks - 1)] the Predictor's draws, positional
    uint32_t* seen = nullptr; int seen_words = 0;  // [B][ceil(sample_limit / 32)] codes 0 generated so far, per slot
    // timing
    hipEvent_t ev0 = nullptr, ev1 = nullptr, ev2 = nullptr, ev3 = nullptr;
    std::vector<hipEvent_t> fin_ev;     // per slot: PCM of a finished utterance copied to the host (vocoder stream)
    q3tts_timings tm{};
    Q3Voc* voc = nullptr;
    int voc_source = 0;                 // q3tts_get_vocoder_source: 0 no vocoder, 1 synthetic weights, 2 qwen3_tts_vocoder.gguf
    Q3Mel* mel = nullptr;               // created on first use
    Q3Clone* clone = nullptr;           // q3tts_clone_init / q3tts_clone_load
    int clone_source = 0;               // q3tts_get_clone_source: 0 not loaded, 1 synthetic weights, 2 the two encoder files
    std::string weights_dir;            // the config's weights_path ("" without one): where q3tts_clone_load(e, NULL) looks
    // q3tts_k_probe: eager frame steps, events around the Predictor gate/up GEMM (pass 1, layer 0) of every frame
    int probe = 0, probe_kind = 0;      // probe: 0 off, 1 Predictor (pass 1, block 0), 2 Talker (block 0); kind: 0 gate/up, 1 QKV, 2 attention, 3 O, 4 down
    std::vector<hipEvent_t> probe_ev;   // 2 per frame of a chunk
    int probe_i = 0;
    double probe_ms = 0, probe_empty_ms = 0; long long probe_cnt = 0, probe_empty_cnt = 0, row_steps = 0;
    // q3tts_set_device_pcm: packed device copy of the last batch's PCM, one row of dev_pcm_stride samples per request
    int dev_pcm_on = 0; float* dev_pcm = nullptr; int dev_pcm_n = 0; size_t dev_pcm_stride = 0;
    // q3tts_set_output_rate (q3_resample.hip): out_rate 0 = off (every launch and bit as without it). rs_out: the vocoder's rate -> out_rate.
    // rs_stage [B][rs_stage_stride] f32: the resampled PCM of a slot on its way to the host (q3tts_generate_batch, streams)
    int out_rate = 0; Q3Resamp rs_out{}; std::vector<Q3Resamp> rs_cache;
    float* rs_stage = nullptr; size_t rs_stage_stride = 0, rs_stage_cap = 0;
    // q3tts_set_speed (q3_tempo.hip): speed 0 = off (every launch and bit as without it), else per mille. tp_row
    // [B][tp_stride] f32: the slots' stretched PCM, which every PCM exit then reads instead of the vocoder's rows (q3_pcm_rows). The rest is
    // a memo of a pure function of a vocoder row's prefix: tp_done[b] frames of slot b are in its tempo row (host; 0 for a new occupant and
    // after a swap-in, which rebuilds), tp_last[b] = p of the last of them (device). tp_win: the window (device).
    int speed = 0; float* tp_row = nullptr; size_t tp_stride = 0, tp_cap = 0;
    long long* tp_last = nullptr; float* tp_win = nullptr; std::vector<int> tp_done;
    double hp_launch = 0, hp_sync = 0;  // Q3TTS_HOST_PROF: host wall of run_chunk's launch part / of its wait (per engine: the node drives several from threads)
    float *park_logits = nullptr, *park_x = nullptr;  // [B][t_vocab], [B][t_d_model]: a parked slot's rows (q3_park_rows)
    float* first_chunk_host = nullptr;  // pinned landing buffer of the first 4-frame PCM chunk (first-chunk latency)
    std::atomic<q3tts_session*> session{nullptr};  // an open session owns the engine (q3_session.hip)
    std::mutex err_mu;                  // err is written by the session worker too
};

// A voice prefix (include/q3tts.h, "voice prefixes"): the Talker's K/V of a prompt's first P rows, laid out as one slot's cache of
// np = ceil(P / 64) * 64 positions — k / v [L][Hkv][np * hd] bf16 — and copied into a slot by k_kv_prefix at admission.
struct q3tts_prefix {
    q3tts_engine* e = nullptr;          // the engine that made it (and whose slots it may enter)
    int P = 0, np = 0;
    uint16_t *k = nullptr, *v = nullptr;  // (kv_q8_0: int8 quants [L][Hkv][np * hd], then their f16 scales [L][Hkv][np * hd / 32])
    // A prefix made through a session (q3_session.hip) exists before its store does. state: 0 pending, 1 ready, < 0 the
    // status it failed with; the worker writes P / np / k / v and then state (release), any thread reads state first (acquire).
    // released / qrefs (the session's mutex): q3tts_session_prefix_release was called; queued requests of the session that name it.
    std::atomic<int> state{1};
    bool released = false; int qrefs = 0;
};
size_t q3_prefix_store_bytes(const q3tts_engine* e, int np);  // bytes of ONE of a prefix's two stores (k or v) of np positions

// helpers shared with q3_vocoder.hip and the kernel-level test hooks (q3_hooks.hip)
int q3_set_err(q3tts_engine* e, int code, const std::string& msg);
// calls that drive an engine return Q3TTS_ERR_STATE (with a message) while a session owns it
int q3_refuse_in_session(q3tts_engine* e);
#define Q3_NOT_IN_SESSION(e) do { if ((e) && (e)->session.load()) return q3_refuse_in_session(e); } while (0)
#define Q3_HIP(e, call)                                                                                         \
    do {                                                                                                        \
        hipError_t err__ = (call);                                                                              \
        if (err__ != hipSuccess)                                                                                \
            return q3_set_err((e), Q3TTS_ERR_DEVICE, std::string(#call) + ": " + hipGetErrorString(err__));     \
    } while (0)
#define TRY(x) do { int rc__ = (x); if (rc__ != Q3TTS_OK) return rc__; } while (0)

// zero-filled device memory whose fill has completed on return (the one allocator of engine, vocoder, mel and clone state)
int q3_dev_alloc_zeroed(q3tts_engine* e, void** p, size_t bytes);

// Device memory that lives as long as the engine: n zero-filled elements (+ 64 bytes of slack), recorded in e->allocs and freed in one loop
// by q3tts_engine_destroy (of a whole or a half-built engine). The rule: engine lifetime -> q3_dalloc; anything shorter, or that regrows
// (weight staging, dev_pcm, a prefix's K/V, a session's staging) -> its own hipMalloc / hipFree pair.
template <class T>
int q3_dalloc(q3tts_engine* e, T** p, size_t n) {
    void* q = nullptr;
    const int rc = q3_dev_alloc_zeroed(e, &q, n * sizeof(T) + 64);
    if (rc != Q3TTS_OK) return rc;
    e->allocs.push_back(q);
    *p = (T*)q;
    return Q3TTS_OK;
}

// weights and assets (q3_weights.hip), used by q3tts_engine_create only
class Q3Gguf;
struct Q3TfmShape {
    int grp;                  // Q3G_TALKER / Q3G_PRED: the synthetic tensors' id group
    int L, d, Hq, Hkv, hd, F, head_n;
    float theta; const int* sections;  // RoPE base; M-RoPE sections (null: every dimension rotates)
    int n_ctx, n_slots;       // KV cache: positions per slot, slots
    int kv8;                  // cfg.kv_q8_0: the cache as Q8_0 blocks
};
// layer l's part of the cache t: bf16 elements, or (t.kv8) int8 quants and their scales
inline void q3_layer_cache(const Q3KvCache& t, int l, uint16_t** kc, uint16_t** vc, uint16_t** kd, uint16_t** vd) {
    if (t.kv8) {
        *kc = (uint16_t*)((int8_t*)t.kc + l * t.layer_stride); *vc = (uint16_t*)((int8_t*)t.vc + l * t.layer_stride);
        *kd = t.kd + l * (t.layer_stride >> 5); *vd = t.vd + l * (t.layer_stride >> 5);
    } else { *kc = t.kc + l * t.layer_stride; *vc = t.vc + l * t.layer_stride; *kd = *vd = nullptr; }
}
// the descriptor of K/V copies between t's cache and stores (voice prefixes, swap blocks): everything but the entries
inline Q3KvPrefix q3_kv_prefix_of(const Q3Tfm& t) {
    const Q3KvCache& c = t.cache;
    Q3KvPrefix kp{c.kc, c.vc, c.layer_stride, c.n_ctx, t.L, t.Hkv, t.hd}; kp.kv8 = c.kv8 ? 1 : 0; kp.kd = c.kd; kp.vd = c.vd;
    return kp;
}
// the transformer's weights, KV cache and RoPE tables. g: the opened GGUF `file` (null: seeded synthetic weights);
// q8mode: cfg.talker_q8_0 / cfg.predictor_q8_0
int q3_tfm_init(q3tts_engine* e, Q3Tfm& t, const Q3TfmShape& sh, const Q3Gguf* g, const char* file, int q8mode);
// text / codec tables, codec_dev, proj_w / proj_b, tts_pad and the pre-projected codec tables, from the files of wdir (empty: synthetic)
int q3_assets_init(q3tts_engine* e, const std::string& wdir);
// e->qkv0 (after both of the above), or nothing where the switches or the model say so; a refused launch is an error
int q3_pred_table_init(q3tts_engine* e);
// slice q (1 .. n_codebooks - 2) of e->qkv0 and its rows without the fallback row
inline int q3_pred_table_rows(const q3tts_engine* e) { return e->cfg.model.codecq_rows; }
inline const float* q3_pred_table_slice(const q3tts_engine* e, int q) { return e->qkv0 + (size_t)(q - 1) * (q3_pred_table_rows(e) + 1) * e->P.nqkv; }
// whether the frame step e->pred_variant names gathers from the table: the greedy heads only (the sampling form keeps every launch)
inline bool q3_pred_table_on(const q3tts_engine* e) { return e->qkv0 && !e->P.a8 && e->pred_variant == 0; }

// the two transformers' launches (q3_layers.hip)
// What one call runs them on; a zero member means "not used":
struct Q3LayerRun {
    int rows;                                       // the first `rows` rows of the Q3Rows
    const int *row_pos, *row_slot;                  // per-row position / slot maps (device); null: slot = row % slot_mod, position = pos_const (+ row / slot_mod)
    bool one_row_per_slot;                          // decode rows: q/k prep and the K/V append are fused into the attention launch
    hipEvent_t* probe;                              // q3tts_k_probe: two events that bracket launch e->probe_kind of block 0
    int slot_mod, pos_const;
    const int* seg; int n_seg, seg_max_n, seg_max_t;  // prefill of whole prompts: the rows as per-slot runs (pf_seg), the longest run, the furthest position + 1
    const Q3AttGather* gather;                      // block 0 takes its q / k / v rows from the table: no QKV launch, the gathering attention (q3_launch_attend_gather)
    const Q3KvCache* cache;                         // the K/V cache the blocks append to and attend over; null: t's own
};
// `a.rows` rows of r through every block of t; returns the number of launches the GEMM launcher refused
int q3_run_layers(q3tts_engine* e, const Q3Tfm& t, const Q3Rows& r, const Q3LayerRun& a, Q3Scratch& sc, hipStream_t s);
// one frame step over the first B rows of the lane, issued on s; returns the number of refused launches (0 = the frame was issued completely)
int q3_record_frame(q3tts_engine* e, Q3Lane& L, hipStream_t s, int B);
// one captured frame step per row bucket, of the variant e->pred_variant names
int q3_capture_frames(q3tts_engine* e, std::vector<hipGraph_t>& graphs, std::vector<hipGraphExec_t>& execs);
// block l's QKV GEMM of t on the first `rows` rows of r into sc.qkv
Q3BGemm q3_gemm_qkv(const Q3Tfm& t, int l, const Q3Rows& r, const Q3Scratch& sc, int rows, float eps, int once);
// the descriptor of head q ([q N, (q + 1) N) of t's output.weight) on rows [row0, row0 + rows) of r, and the one launch helper of t's GEMMs
Q3BGemm q3_gemm_head(const Q3Tfm& t, int q, int N, const Q3Rows& r, int row0, int rows, float eps, int once, float* y);
int q3_launch_gemm(q3tts_engine* e, const Q3Tfm& t, const Q3BGemm& g, hipStream_t s, hipEvent_t* probe = nullptr, int kind = -1);

// RoPE tables [n_pos][hd / 2] in double on the host (q3_weights.hip; the attention hooks build their own)
void q3_rope_tables(int n_pos, int hd, float theta, const int* sections, std::vector<float>& cs, std::vector<float>& sn);

// host ChaCha12 StdRng (q3_rng.cpp)
void q3_stdrng_f32(uint64_t seed, int n, float* out);

void q3_mel_destroy(q3tts_engine* e);
int q3_mel_run(q3tts_engine* e, const float* audio, int64_t n_samples, int32_t* n_frames, float** out_dev);
void q3_clone_destroy(q3tts_engine* e);
// vocoder interface (q3_vocoder.hip)
// voc_file: the opened and checked qwen3_tts_vocoder.gguf (q3_voc_file_check has passed) whose tensors fill the weights, `file` its path for
// messages; nullptr: the seeded synthetic generator. One creation path: only the source of each array differs.
int q3_voc_create(q3tts_engine* e, const Q3Gguf* voc_file, const std::string& file);
void q3_voc_destroy(q3tts_engine* e);
// reset the streaming state of a slot
int q3_voc_reset(q3tts_engine* e, int slot);
// decode frames [f0, f0+nf) of slot (codes already on device in e->codes) into the slot's PCM buffer on stream
int q3_voc_decode(q3tts_engine* e, int slot, int f0, int nf, int is_last, hipStream_t s);
// batched: nf (<= 4) frames for every listed slot in one set of launches; real[i] <= nf of them are real for slot i (the
// rest are throw-away padding behind a finished utterance's last frame)
// beside_decoder: frame steps will run while this call executes (its long-lived workgroups are then launched one per CU: q3_vocoder.hip, "polite")
int q3_voc_decode_batch(q3tts_engine* e, const int* slots, const int* real, int ns, int nf, hipStream_t s, int beside_decoder);
void q3_voc_mark_last(q3tts_engine* e, int slot);
// PCM buffer of a slot (device) and samples produced so far
float* q3_voc_pcm(q3tts_engine* e, int slot);
int q3_voc_samples(q3tts_engine* e, int slot);
int q3_voc_samples_per_frame(const q3tts_engine* e);
size_t q3_voc_pcm_stride(const q3tts_engine* e);  // samples between the PCM buffers of consecutive slots
// a piece of per-slot device state: slot b's part is [base + b * stride, + bytes)
struct Q3SlotBlock { char* base; unsigned long long stride, bytes; };
// the vocoder's per-slot state that outlives a call: its history blocks (the list q3_voc_reset zeroes) and every layer's ring slices
void q3_voc_slot_blocks(q3tts_engine* e, std::vector<Q3SlotBlock>& out);
// a slot's frames_done / last_flag, read (set = false) or written
void q3_voc_host_state(q3tts_engine* e, int slot, int* frames_done, int* last_flag, bool set);

// Swapping (q3_swap.hip; include/q3tts.h, "paced requests and swapping"): one device arena carved on the host, and the moves
// of a slot's whole state into a block of it and back into any slot.
struct Q3Swap;
// the arena (arena_bytes > 0) and the state table, checked against the device's free memory; counted in e->dev_bytes until q3_swap_destroy
int q3_swap_create(q3tts_engine* e, long long arena_bytes, Q3Swap** out);
void q3_swap_destroy(q3tts_engine* e, Q3Swap* sw);
// bytes of the block of a request at Talker position cur_pos whose vocoder has taken voc_frames frames (the formula of include/q3tts.h)
long long q3_swap_block_bytes(const q3tts_engine* e, const Q3Swap* sw, int cur_pos, int voc_frames);
// first-fit over 256-byte units: the block's offset or -1 (no room); q3_swap_release coalesces with the free neighbours
long long q3_swap_alloc(Q3Swap* sw, long long bytes);
void q3_swap_release(Q3Swap* sw, long long off, long long bytes);
long long q3_swap_used(const Q3Swap* sw);
// One group's moves, one launch per kernel and Q3_KVP_MAX items: the K/V of positions < cur_pos (q3_launch_kv_prefix_save / q3_launch_kv_prefix)
// and the decoder's per-slot state on e->stream, the vocoder's on e->vstream. save: slot -> block; else block -> slot.
struct Q3SwapItem { int slot, cur_pos, voc_frames; long long off; };
// *ticket names the move: q3_swap_done(sw, ticket) says (without waiting) whether both streams' halves of it, and of every earlier move,
// have run. A block goes back to q3_swap_release only then — whatever is carved over its bytes next has another layout, so stream order
// alone does not keep the new block's decode-stream half off the old block's vocoder-stream half.
int q3_swap_move(q3tts_engine* e, Q3Swap* sw, const Q3SwapItem* items, int n, bool save, unsigned long long* ticket);
bool q3_swap_done(Q3Swap* sw, unsigned long long ticket);
// streamed text for several slots behind ONE synchronise of the decode stream (q3_text_rows_set is the group of one)
struct Q3TextSet { int b; const int32_t* T; int from, n, n_frames; };
int q3_text_rows_set_group(q3tts_engine* e, const Q3TextSet* items, int count);

// the resampler's engine side (q3_resample.hip): the cached table of a rate pair (built and uploaded on first use), and outputs
// [first_out, first_out + count) of slot b's PCM row (n_valid samples so far) at e->out_rate into the start of the slot's row of e->rs_stage
int q3_resample_get(q3tts_engine* e, int rate_in, int rate_out, Q3Resamp* out);
int q3_resample_slot(q3tts_engine* e, int b, long long first_out, int count, int n_valid, bool is_final, hipStream_t s);
// the slots' staging rows sized for rs over the rows the PCM exits read now (q3_pcm_rows_stride); regrows, never shrinks
int q3_rs_stage_fit(q3tts_engine* e, const Q3Resamp& rs, size_t* stride);

// the time-stretch's engine side (q3_tempo.hip). The rows every PCM exit reads: the vocoder's, or with a speed set the tempo rows
inline const float* q3_pcm_rows(q3tts_engine* e) { return e->speed ? e->tp_row : q3_voc_pcm(e, 0); }
inline size_t q3_pcm_rows_stride(const q3tts_engine* e) { return e->speed ? e->tp_stride : q3_voc_pcm_stride(e); }
// what a PCM row of ns vocoder samples (done: all there are) holds for the exits: ns, or with a speed set N_t(ns) / D_t(ns)
inline long long q3_pcm_valid(const q3tts_engine* e, long long ns, bool done) { return e->speed ? q3_tempo_valid(ns, e->speed, done) : ns; }
// one launch (per 64 slots) on s that brings the listed slots' tempo rows up to what ns[i] vocoder samples (done[i]: all there are) decide
int q3_tempo_slots(q3tts_engine* e, const int* slots, const int* ns, const char* done, int count, hipStream_t s);
// slot b's memo is forgotten: a new occupant, or a swapped-in request whose tempo row is rebuilt from its PCM row (host state only)
inline void q3_tempo_forget(q3tts_engine* e, int b) { if ((size_t)b < e->tp_done.size()) e->tp_done[b] = 0; }
// the body of q3tts_time_stretch without the session check
int q3_time_stretch_run(q3tts_engine* e, const float* in, int64_t n_in, int32_t permille, float* out, int64_t cap, int64_t* n_out);

// the one-shots' launches over device rows (what q3tts_time_stretch / q3tts_resample run between their upload and their copy back):
// dst[0, N_t(n_in)) from src[0, n_in) with the window and one long long of scratch on the device; dst[0, N(n_in)) at rs's output rate
// (-1, nothing launched: one tile's input span does not fit the LDS)
void q3_time_stretch_dev(const float* src, long long n_in, int permille, float* dst, const float* win, long long* p_last, hipStream_t s);
int q3_resample_dev(const float* src, long long n_in, const Q3Resamp& rs, float* dst, hipStream_t s);

// long documents (q3_long.hip). The plan is a pure function of the edges and the options (host): per row lo, hi, begin,
// end (plan [rows][4]) and the join kernel's table (segs [rows], *max_span = the longest piece + gap); returns N
long long q3_join_plan(const int32_t* lens, const int32_t* kinds, const int32_t* edges, int rows, const q3tts_join_opts& o, int rate,
                       long long* plan, Q3JoinSeg* segs, long long* max_span);
// Q3TTS_OK, or Q3TTS_ERR_INVALID with *msg naming the rule
int q3_join_opts_rules(const q3tts_join_opts& o, const char** msg);
// documents in a session (q3_doc.hip): the streaming join's host plan, a pure function. segs[j]: segment j as of the
// snapshot the plan is made from — n valid samples, first / last the loud-block edges of x[0, n) ({INT32_MAX, -1}: none), closed (n is
// final), kind. st: the document's state between calls (all zero at the start). One call hands out at most `room` samples: pieces in
// order (seg -1: `count` zeros; else samples [j0, j0 + count) of segment seg's piece, the first one at row offset src, fades F, final
// length L or LLONG_MAX while the segment is open; dst is the caller's) and one Q3DocDone per segment whose piece, possibly empty, is
// now wholly handed out: lo, hi, begin, end as q3_join_plan reports them. Q3TTS_ERR_INVALID: the delivered length would pass 2^28
// samples at segment st->head (nothing of that piece or pause is handed out).
struct Q3DocSegNow { int32_t n, first, last, closed, kind; };
struct Q3DocState { long long head, e, pause_left, have_prev, kmax, delivered, begin; };
struct Q3DocOut { int32_t seg, F; long long src, j0, count, L, dst; };
struct Q3DocDone { int32_t seg, pad; long long lo, hi, begin, end; };
int q3_doc_plan(const q3tts_join_opts& o, int rate, const Q3DocSegNow* segs, int n_segs, long long room, Q3DocState* st,
                std::vector<Q3DocOut>* pieces, std::vector<Q3DocDone>* done);
// what a well-formed document is as far as no engine is needed to say (q3tts_k_doc_rules is this as a test hook): Q3TTS_OK,
// Q3TTS_ERR_STATE (an engine-level speed or output rate is set) or Q3TTS_ERR_INVALID, with *msg naming the rule
int q3_doc_rules(const q3tts_doc_opts& o, const int32_t* kinds, int n_segs, bool have_voice, bool have_prefix, int engine_speed, int engine_rate,
                 const char** msg);
// A document with a speed or an output rate ("the pipeline"): join -> ring RJ -> [stretch -> ring RT] -> exit into the
// staging buffer. Every stage's progress is a host count, so flow control reads nothing back: nj samples joined (fin_j: J is whole), kt
// frames decided, m outputs delivered. q3_doc_ring_room: what the join may write now without passing the lowest position a frame or an
// output not yet decided may read. q3_doc_ring_step: after the join has brought nj up by `joined`, the frames to stretch (clipped to the
// free space of RT) and the outputs to deliver (clipped to room_out, the staging room in output samples); updates r.
struct Q3DocRing {
    int32_t speed, L, M, H;  // speed 0: no stretch; L 0: no resampler (H 0 then)
    long long cj, ct;        // the rings' capacities in samples, multiples of 4 (ct: 0 without a speed)
    long long nj, kt, m;
    int32_t fin_j, pad;
};
struct Q3DocRingStep {
    int32_t k_from, k_to;    // k_doc_tempo's frames (none: equal)
    long long nt;            // the stretched samples there are after them (the launch's n_out)
    long long nx;            // the exit's source: valid samples ...
    int32_t fin_x, all_out;  // ... all there will be; every output of the document is delivered with this step
    long long first, count;  // the exit's outputs
    int32_t pending, pad;    // decidable work is left that needs no new input: frames that did not fit RT, outputs that did not fit room_out
};
long long q3_doc_ring_min_j(int speed, int L, int M, int H);  // Q3_DOC_RING_MIN_* (include/q3tts.h) for these options
long long q3_doc_ring_min_t(int speed, int L, int M, int H);
long long q3_doc_ring_room(const Q3DocRing& r);
void q3_doc_ring_step(Q3DocRing* r, long long joined, bool fin_j, long long room_out, Q3DocRingStep* out);
// k_doc_emit entries around a ring of C samples, split in two where they cross the wrap (count <= C): a plan's piece (from: its first
// sample, NULL for a pause) to stream position pos of the ring the launch writes, and samples [first, first + count) of `ring`, bit
// copies, to dst[at, ...). q3_launch_doc_emit_all: the entries in launches of at most Q3_DOC_MAX_ENT.
void q3_doc_ring_put(const Q3DocOut& p, const float* from, long long pos, long long C, std::vector<Q3DocPiece>* ents);
void q3_doc_ring_get(const float* ring, long long C, long long first, long long count, long long at, std::vector<Q3DocPiece>* ents);
void q3_launch_doc_emit_all(const std::vector<Q3DocPiece>& ents, int i16, void* dst, hipStream_t s);
inline long long q3_doc_out_pos(long long s, int speed, int L, int M) {  // a position of J through the speed and rate maps
    if (speed) s = q3_tempo_N(s, speed);
    return L ? q3_resample_N(s, L, M) : s;
}
// pinned host memory of a result's PCM (q3_generate.hip's pool): what q3tts_result_free gives back
float* q3_pin_alloc(size_t bytes);
void q3_pin_free(float* p);

enum { BOS_TOKEN = 151672, EOS_TOKEN = 151673 };  // tts_bos, tts_eos (src/tts/prompt.rs); tts_pad is the model's tts_pad_id

// the prompt builder (q3_engine.hip): the rows of `part` of p on the device at out; text_stream: the text part in the streamed layout
enum { PROMPT_WHOLE = 0, PROMPT_VOICE = 1, PROMPT_TEXT = 2 };
int build_prompt_dev(q3tts_engine* e, const q3tts_prompt_desc* p, float* out, int max_rows, int* n_out, int part = PROMPT_WHOLE, bool text_stream = false);

// the scheduler steps that the session worker (q3_session.hip) drives between 4-frame chunks: row planning, the chunk, the vocoder boundary
// and the result helpers in q3_generate.hip; admission, the streamed-text rows, parking and the voice prefixes in q3_admit.hip
// (q3_plan_rows + q3_admit_many are also the single-request admission of the talker-prefill hook; q3_admit is that of a stream)
int q3_plan_rows(q3tts_engine* e, const std::vector<int>& live);
int q3_admit_many(q3tts_engine* e, const int* slots, const q3tts_request* const* reqs, int count, int* rc);
int q3_admit(q3tts_engine* e, int b, const q3tts_request* r);
// What a well-formed request / voice job is, as far as no engine is needed to say: the rules every entry refuses alike (pure host code).
// keep: the request's voice part is to be kept as a prefix, keep_rows rows of it (0: taken from r->prompt). Q3TTS_OK, or Q3TTS_ERR_INVALID
// with *msg naming the rule; the session sites put their "submit: " / "prefix: " in front (q3tts_k_request_rules is the first as a test hook).
int q3_request_rules(const q3tts_request* r, bool keep, int keep_rows, const char** msg);
int q3_voice_job_rules(const q3tts_prompt_desc* p, const float* embd, int n_tok, const char** msg);
// One entry of an admission group in its general form (q3_admit_many passes requests only). keep != null: after the group's layers the
// slot's first rows are saved into that (empty) prefix — a request's voice part (keep_rows, 0: taken from r->prompt; 1 <= rows < n), or
// with r == null a prefill-only prefix job: voice / embd + n_tok as q3tts_prefix_create takes them, into a free slot that stays free.
// The store is allocated here; the caller marks the prefix ready once the call has succeeded for the item.
struct Q3AdmItem {
    int slot; const q3tts_request* r;
    q3tts_prefix* keep; int keep_rows;
    const q3tts_prompt_desc* voice; const float* embd; int n_tok;
};
int q3_admit_items(q3tts_engine* e, const Q3AdmItem* items, int count, int* rc);
// CH frame steps over the current row bucket; afterwards the slot mirror is on the host. *dev_ms: the device time
int q3_run_chunk(q3tts_engine* e, int CH, float* dev_ms = nullptr);
// finished slot b's n_frames, hit_eos and codes (malloc) into o: the copy runs on the decode stream, whose next synchronise completes it
int q3_codes_back(q3tts_engine* e, int b, q3tts_result* o);
// a free record (active = 0) for slot b from the pinned staging half admissions use; fin_ev[b] on evs, the stream of the slot's vocoder work
int q3_retire_slot(q3tts_engine* e, int b, hipStream_t evs);
// what a boundary hands out of a PCM row of ns samples (done: all there are) beyond `delivered`: the new ones, or at an output rate the outputs it can deliver by now
int q3_emit_count(const q3tts_engine* e, int ns, bool done, long long delivered);
// x's two stores freed and taken off e->dev_bytes, the handle deleted (nothing on the device reads the stores any more)
void q3_prefix_free(q3tts_prefix* x);
// the bodies of q3tts_clone_audio_encode / q3tts_clone_speaker_encode / q3tts_resample without the session check: the session worker
// runs them on the engine's stream between two chunk boundaries (q3tts_session_clone)
int q3_clone_audio_encode_run(q3tts_engine* e, const float* audio, int64_t n_samples, int64_t* codes, int32_t cap_frames, int32_t* n_frames);
int q3_clone_speaker_encode_run(q3tts_engine* e, const float* audio, int64_t n_samples, float* spk_emb);
int q3_resample_run(q3tts_engine* e, const float* in, int64_t n_in, int32_t rate_in, int32_t rate_out, float* out, int64_t cap, int64_t* n_out);
// streamed text, between frame steps: slot b's trailing ids become T[0, n) (entries [from, n) are uploaded; the first max_steps_cap count)
// and its cursor the row of frame n_frames. n = 0: the slot takes tts_pad (a request without text_stream).
int q3_text_rows_set(q3tts_engine* e, int b, const int32_t* T, int from, int n, int n_frames);
// parking a slot between chunks (q3_session.hip): its Talker logits row and hidden row, which outlive a frame, to / from the slot's side rows
int q3_park_rows(q3tts_engine* e, int b, bool save);
// the ids behind a text_stream request's first one, with tts_eos when its text is closed: T of include/q3tts.h
void q3_text_trailing(const q3tts_request* r, std::vector<int32_t>& T);
// test hook (q3tts_k_pred_variant): force = 1 runs the sampling frame step whatever the temperature
int q3_pred_force_variant(q3tts_engine* e, int force);
int q3_voc_dispatch(q3tts_engine* e, const char* live, const char* want, int* voc_frames, bool more, bool* first);
double q3_now_ms();

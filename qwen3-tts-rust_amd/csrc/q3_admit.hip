// q3_admit.hip — admission of libq3tts: what turns a request into a running slot. The rules of a well-formed request and voice job, the
// batched Talker prefill (src/tts/engine.rs:455-462) of a group of requests and prefix jobs in named steps, the per-slot state that stays
// in step with it (streamed-text rows, parked rows), and the voice prefixes: their stores and the q3tts_prefix_* entries.
#include "q3_engine.h"

#include <chrono>
#include <cstring>

// ---- what a well-formed request is: the rules every entry refuses alike, with no engine and no device (q3_engine.h) ----
int q3_request_rules(const q3tts_request* r, bool keep, int keep_rows, const char** msg) {
    *msg = !r ? "null request"
         : keep && r->prefix ? "keep-voice: a request that names a prefix cannot keep one"
         : keep && (keep_rows < 0 || (keep_rows == 0 && (r->prompt_embd || !r->prompt))) ? "keep-voice: voice_rows >= 1 with prompt_embd (a prompt_embd request states its voice rows), >= 0 with a prompt built from ids"
         : (r->text_open == 1) && !(r->text_stream == 1) ? "text_open needs text_stream = 1"
         : (r->text_stream == 1) && (r->prompt_embd || !r->prompt || r->prompt->n_text < 1 || !r->prompt->text_ids) ? "text_stream needs a prompt built from ids (prompt), not prompt_embd, with n_text >= 1 (its first text id is the prompt's last row)"
         : "";
    return **msg ? Q3TTS_ERR_INVALID : Q3TTS_OK;
}
int q3_voice_job_rules(const q3tts_prompt_desc* p, const float* embd, int n_tok, const char** msg) {
    *msg = (p != nullptr) == (embd != nullptr) ? "give exactly one of a voice desc or host rows" : embd && n_tok < 1 ? "host rows come with n_tok >= 1" : "";
    return **msg ? Q3TTS_ERR_INVALID : Q3TTS_OK;
}
// a voice job before any row is built: the rules above, and 1 <= rows < n_ctx (q3tts_prefix_create and a session's prefix job at admission)
static int voice_job_check(q3tts_engine* e, const q3tts_prompt_desc* p, const float* embd, int n_tok) {
    const char* msg = "";
    if (q3_voice_job_rules(p, embd, n_tok, &msg) != Q3TTS_OK) return q3_set_err(e, Q3TTS_ERR_INVALID, std::string("prefix: ") + msg);
    if (embd && n_tok >= e->cfg.n_ctx) return q3_set_err(e, Q3TTS_ERR_INVALID, "prefix: n_tok outside 1 .. n_ctx - 1");
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
int q3_text_rows_set_group(q3tts_engine* e, const Q3TextSet* items, int count) {
    if (count <= 0) return Q3TTS_OK;
    const int cap = e->cfg.max_steps_cap;
    hipStream_t s = e->stream;
    std::vector<int> cs(count); std::vector<int2> curs(count);
    for (int i = 0; i < count; ++i) {
        const Q3TextSet& it = items[i];
        const int c = std::min(std::max(it.n, 0), cap), from = std::max(it.from, 0);  // (frames stop at max_steps <= cap: later rows are never read)
        if (from < c) Q3_HIP(e, hipMemcpyAsync(e->ts_ids + (size_t)it.b * cap + from, it.T + from, (size_t)(c - from) * 4, hipMemcpyHostToDevice, s));
        cs[i] = c; curs[i] = it.n_frames >= 0 && it.n_frames < c ? make_int2(1, it.T[it.n_frames]) : make_int2(0, 0);
        Q3_HIP(e, hipMemcpyAsync(e->ts_cnt + it.b, &cs[i], 4, hipMemcpyHostToDevice, s));
        Q3_HIP(e, hipMemcpyAsync(e->ts_cur + it.b, &curs[i], sizeof(int2), hipMemcpyHostToDevice, s));
    }
    Q3_HIP(e, hipStreamSynchronize(s));  // the uploads read locals
    return Q3TTS_OK;
}
int q3_text_rows_set(q3tts_engine* e, int b, const int32_t* T, int from, int n, int n_frames) {
    const Q3TextSet it{b, T, from, n, n_frames};
    return q3_text_rows_set_group(e, &it, 1);
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

// ---- one group's admission, step by step (admit_group) ----
// the group's rows as row -> (position, slot) maps and as runs: every request's rows are consecutive, positions P .. P + n - 1
struct GroupMaps { std::vector<int> pos, slot, seg; int seg_max = 0, seg_max_t = 0; };
static GroupMaps group_maps(const std::vector<Adm>& grp, int total) {
    GroupMaps m{std::vector<int>(total), std::vector<int>(total)};
    for (const Adm& a : grp) {
        for (int i = 0; i < a.n; ++i) { m.pos[a.row0 + i] = a.P + i; m.slot[a.row0 + i] = a.b; }
        m.seg.push_back(a.row0); m.seg.push_back(a.n); m.seg.push_back(a.b); m.seg.push_back(a.P);
        m.seg_max = std::max(m.seg_max, a.n); m.seg_max_t = std::max(m.seg_max_t, a.P + a.n);
    }
    return m;
}
// The Talker's layers over the first m.pos.size() prefill rows (e->pf.x holds them): row i sits at position pos[i] of slot slot[i]; seg: the
// same rows as per-slot runs (pf_seg), seg_max the longest run, seg_max_t the furthest position + 1. The maps are uploaded and the stream
// is synchronised (they are the caller's locals); kp (admission only): the voice prefixes' K/V enter their slots before the layers run.
// cache: where the K/V go (a prefix store's view), null: the engine's own cache.
// Returns the number of refused launches, or -1 when an upload failed (e->err says which).
static int prefill_layers(q3tts_engine* e, const GroupMaps& m, const Q3KvPrefix* kp, const Q3KvCache* cache) {
    const int rows = (int)m.pos.size(), d = e->T.d;
    hipStream_t s = e->stream;
    hipError_t er = hipMemcpyAsync(e->pf_pos, m.pos.data(), (size_t)rows * 4, hipMemcpyHostToDevice, s);
    if (er == hipSuccess) er = hipMemcpyAsync(e->pf_slot, m.slot.data(), (size_t)rows * 4, hipMemcpyHostToDevice, s);
    if (er == hipSuccess) er = hipMemcpyAsync(e->pf_seg, m.seg.data(), m.seg.size() * 4, hipMemcpyHostToDevice, s);
    if (er == hipSuccess) er = hipStreamSynchronize(s);
    if (er != hipSuccess) { q3_set_err(e, Q3TTS_ERR_DEVICE, std::string("prefill row maps: ") + hipGetErrorString(er)); return -1; }
    if (kp) q3_launch_kv_prefix(*kp, s);
    const Q3Rows& r = e->pf;
    if (e->T.a8) q3_launch_norm_inputs_q8(r.x, d, rows, d, e->T.attn_norm[0], (int8_t*)r.xb, r.ascale, r.rt16, r.ssp, d / 16, s);
    else q3_launch_norm_inputs(r.x, d, rows, d, e->T.attn_norm[0], r.xb, 0, r.ssp, d / 16, s);
    return q3_run_layers(e, e->T, r, {.rows = rows, .row_pos = e->pf_pos, .row_slot = e->pf_slot, .seg = e->pf_seg, .n_seg = (int)m.seg.size() / 4,
                                   .seg_max_n = m.seg_max, .seg_max_t = m.seg_max_t, .cache = cache}, e->sc_pre, s);
}
// K/V copies between stores and slots, Q3_KVP_MAX entries to a launch. save: slot -> store (k_kv_prefix_save), else store -> slot
// (k_kv_prefix). Nonzero: the launch was refused for this model shape.
static int kvp_launch(const Q3KvPrefix& d, bool save, hipStream_t s) { return save ? q3_launch_kv_prefix_save(d, s) : (q3_launch_kv_prefix(d, s), 0); }
// {x's store, rows, slot} joins d. The descriptor is full (more than 64 such entries in a group): its copies go now, on the same stream,
// and it starts again (*n_launch counts these).
static int kvp_add(Q3KvPrefix& d, bool save, const q3tts_prefix* x, int rows, int slot, hipStream_t s, int* n_launch) {
    int bad = 0;
    if (d.n == Q3_KVP_MAX) { bad = kvp_launch(d, save, s); d.n = 0; ++*n_launch; }
    d.pk[d.n] = x->k; d.pv[d.n] = x->v; d.P[d.n] = rows; d.slot[d.n] = slot; ++d.n;
    return bad;
}
// the voice prefixes of the group's requests into kp: full descriptors are launched here, ahead of the group's layers
static void copy_prefixes(q3tts_engine* e, const std::vector<Adm>& grp, Q3KvPrefix& kp) {
    int n_launch = 0; long long n_prefixed = 0;
    for (const Adm& a : grp) if (a.P > 0) { kvp_add(kp, false, a.r->prefix, a.r->prefix->P, a.b, e->stream, &n_launch); ++n_prefixed; }
    e->kvp_launches.fetch_add(n_launch + (kp.n > 0 ? 1 : 0), std::memory_order_relaxed);  // (prefill_layers launches the rest)
    if (n_prefixed > e->kvp_group_max.load(std::memory_order_relaxed)) e->kvp_group_max.store(n_prefixed, std::memory_order_relaxed);
}
// the slots' voice rows into their prefix stores, behind the layers on the same stream
static int save_keeps(q3tts_engine* e, const std::vector<Adm>& grp, const Q3KvPrefix& kp) {
    Q3KvPrefix sv = kp; sv.n = 0;
    int bad = 0, n_launch = 0;
    for (const Adm& a : grp) if (a.keep && !bad) bad = kvp_add(sv, true, a.keep, a.keep_rows, a.b, e->stream, &n_launch);
    if (sv.n == 0) return Q3TTS_OK;  // nothing to keep
    if (bad || kvp_launch(sv, true, e->stream)) return q3_set_err(e, Q3TTS_ERR_INVALID, "prefix save: launch refused for this model shape");
    Q3_HIP(e, hipGetLastError());
    return Q3TTS_OK;
}
// the request's last prompt row seeds its slot: the Talker logits, both samplers' draws, the slot record, the text rows, the vocoder reset
static int seed_slot(q3tts_engine* e, const Adm& a) {
    const q3tts_model_config& m = e->cfg.model;
    hipStream_t s = e->stream;
    const q3tts_request* r = a.r;
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
    return Q3TTS_OK;
}
static int admit_group(q3tts_engine* e, std::vector<Adm>& grp, int total) {
    if (grp.empty()) return Q3TTS_OK;
    const GroupMaps m = group_maps(grp, total);
    Q3KvPrefix kp = q3_kv_prefix_of(e->T);
    copy_prefixes(e, grp, kp);
    const int rl = prefill_layers(e, m, &kp, nullptr);  // (the rest of the copies, behind its uploads)
    if (rl < 0) return Q3TTS_ERR_DEVICE;
    if (rl) return q3_set_err(e, Q3TTS_ERR_INVALID, "prefill: a kernel launch was refused for this model shape");
    Q3_HIP(e, hipGetLastError());
    TRY(save_keeps(e, grp, kp));
    for (const Adm& a : grp) if (a.r) TRY(seed_slot(e, a));  // (a prefix job's slot stays free)
    return Q3TTS_OK;
}

// bytes of one of a prefix's two stores of np positions, in the slots' format: bf16, or Q8_0 quants with their f16 scales behind them
size_t q3_prefix_store_bytes(const q3tts_engine* e, int np) {
    const size_t per = (size_t)e->T.L * e->T.Hkv * np * e->T.hd;
    return e->T.cache.kv8 ? per + per / 16 : per * 2;
}
// x's store seen as a K/V cache: one slot of np positions; Q8_0: the scales follow the L layers of quants in the same allocation
static Q3KvCache prefix_cache_view(const Q3Tfm& t, const q3tts_prefix* x) {
    Q3KvCache c;
    c.kc = x->k; c.vc = x->v; c.layer_stride = (size_t)t.Hkv * x->np * t.hd; c.n_ctx = x->np; c.n_slots = 1; c.kv8 = t.cache.kv8;
    if (c.kv8) { const size_t quants = t.L * c.layer_stride; c.kd = (uint16_t*)((int8_t*)x->k + quants); c.vd = (uint16_t*)((int8_t*)x->v + quants); }
    return c;
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
void q3_prefix_free(q3tts_prefix* x) {
    for (uint16_t* p : {x->k, x->v}) if (p) { x->e->dev_bytes -= q3_prefix_store_bytes(x->e, x->np); hipFree(p); }
    delete x;
}

// One item's rows join the prefill batch behind the `total` rows it holds: n_tok host rows (embd), or `part` of p built on the device; at
// most max_rows of them. A batch too full for them is flushed (admit_group) and the item placed in the empty one. *n: the row count, or
// the item's status (< 0) when even that fails. The return value is the admission's own status (a failed flush or upload ends it).
static int place_rows(q3tts_engine* e, std::vector<Adm>& grp, int& total, int max_rows, const float* embd, int n_tok, const q3tts_prompt_desc* p,
                      int part, bool text_stream, int* n) {
    const size_t d = (size_t)e->cfg.model.d_embed;
    for (;;) {
        const int room = std::min(e->cfg.n_ctx - total, max_rows);
        int st = Q3TTS_OK;
        if (!embd) st = build_prompt_dev(e, p, e->pf.x + total * d, room, n, part, text_stream);
        else if (n_tok > room) st = total ? Q3TTS_ERR_INVALID : q3_set_err(e, Q3TTS_ERR_INVALID, "n_tok out of range");
        else { *n = n_tok; Q3_HIP(e, hipMemcpyAsync(e->pf.x + total * d, embd, n_tok * d * 4, hipMemcpyHostToDevice, e->stream)); }
        if (st == Q3TTS_OK) return Q3TTS_OK;
        if (total == 0) { *n = st; return Q3TTS_OK; }
        TRY(admit_group(e, grp, total));  // batch full: flush, then retry this item in an empty batch
        grp.clear(); total = 0;
    }
}

// One item of each kind joins the group: the engine-dependent rules, its rows, its store. Each returns the item's status; *fatal: the
// admission's own (place_rows), which ends it.
// a prefill-only prefix job: 1 <= rows < n_ctx, as q3tts_prefix_create
static int admit_job(q3tts_engine* e, std::vector<Adm>& grp, int& total, const Q3AdmItem& it, int* fatal) {
    if (!it.keep) return q3_set_err(e, Q3TTS_ERR_INVALID, "prefix: a job without a handle to fill");
    TRY(voice_job_check(e, it.voice, it.embd, it.n_tok));
    int n = 0;
    if ((*fatal = place_rows(e, grp, total, e->cfg.n_ctx - 1, it.embd, it.n_tok, it.voice, PROMPT_VOICE, false, &n)) != Q3TTS_OK) return *fatal;
    if (n < 0) return n;
    if (n < 1) return q3_set_err(e, Q3TTS_ERR_INVALID, "prefix: the voice part has no rows");
    TRY(prefix_store_alloc(e, it.keep, n));
    grp.push_back(Adm{it.slot, nullptr, n, total, 0, 0, it.keep, n});
    total += n;
    return Q3TTS_OK;
}
static int admit_request(q3tts_engine* e, std::vector<Adm>& grp, int& total, const Q3AdmItem& it, int* fatal) {
    const q3tts_request* r = it.r;
    const char* msg = "";
    if (q3_request_rules(r, it.keep != nullptr, it.keep_rows, &msg) != Q3TTS_OK) return q3_set_err(e, Q3TTS_ERR_INVALID, msg);
    const int max_steps = r->max_steps > 0 ? r->max_steps : e->max_steps;
    if (max_steps > e->cfg.max_steps_cap) return q3_set_err(e, Q3TTS_ERR_INVALID, "max_steps exceeds max_steps_cap");
    const q3tts_prefix* x = r->prefix;
    if (x && x->e != e) return q3_set_err(e, Q3TTS_ERR_INVALID, "prefix: made by another engine");
    if (x && x->state.load(std::memory_order_acquire) != 1) return q3_set_err(e, Q3TTS_ERR_INVALID, "prefix: not ready (a session's pending or failed prefix)");
    const int P = x ? x->P : 0;  // the prefix's rows come first; only the request's own rows enter the prefill buffer
    if (r->text_stream == 1) TRY(ensure_text_frames(e));
    if (r->prompt_embd && (r->n_tok <= 0 || P + r->n_tok > e->cfg.n_ctx)) return q3_set_err(e, Q3TTS_ERR_INVALID, "n_tok out of range");
    if (!r->prompt_embd && !r->prompt) return q3_set_err(e, Q3TTS_ERR_INVALID, "request has neither prompt_embd nor prompt");
    int n = 0;
    if ((*fatal = place_rows(e, grp, total, e->cfg.n_ctx, r->prompt_embd, r->n_tok, r->prompt, x ? PROMPT_TEXT : PROMPT_WHOLE, r->text_stream == 1, &n)) != Q3TTS_OK) return *fatal;
    if (n < 0) return n;
    if (P + n > e->cfg.n_ctx) return q3_set_err(e, Q3TTS_ERR_INVALID, "prefix + prompt longer than n_ctx");
    if (P + n + max_steps > e->cfg.n_ctx) return q3_set_err(e, Q3TTS_ERR_INVALID, "prompt + max_steps exceeds n_ctx");
    int keep_rows = 0;
    if (it.keep) {  // the voice part of a whole prompt: everything in front of the text part's n_text + 3 rows (text_stream: 2)
        keep_rows = it.keep_rows > 0 ? it.keep_rows : n - (r->text_stream == 1 ? 2 : r->prompt->n_text + 3);
        if (keep_rows < 1 || keep_rows >= n) return q3_set_err(e, Q3TTS_ERR_INVALID, "keep-voice: voice_rows outside 1 .. n - 1");
        TRY(prefix_store_alloc(e, it.keep, keep_rows));
    }
    grp.push_back(Adm{it.slot, r, n, total, max_steps, P, it.keep, keep_rows});
    total += n;
    return Q3TTS_OK;
}

// items[i] enters its slot; rc[i] = status of item i (a failing item does not stop the others)
int q3_admit_items(q3tts_engine* e, const Q3AdmItem* items, int count, int* rc) {
    std::vector<Adm> grp;
    int total = 0;
    for (int i = 0; i < count; ++i) {
        int fatal = Q3TTS_OK;
        rc[i] = items[i].r ? admit_request(e, grp, total, items[i], &fatal) : admit_job(e, grp, total, items[i], &fatal);
        TRY(fatal);
    }
    return admit_group(e, grp, total);
}

// slots[i] <- reqs[i]; rc[i] = status of request i (a failing request does not stop the others)
int q3_admit_many(q3tts_engine* e, const int* slots, const q3tts_request* const* reqs, int count, int* rc) {
    std::vector<Q3AdmItem> items(count);
    for (int i = 0; i < count; ++i) { items[i] = Q3AdmItem{}; items[i].slot = slots[i]; items[i].r = reqs[i]; }
    return q3_admit_items(e, items.data(), count, rc);
}

int q3_admit(q3tts_engine* e, int b, const q3tts_request* r) {
    int rc = Q3TTS_OK;
    int st = q3_admit_many(e, &b, &r, 1, &rc);
    return st != Q3TTS_OK ? st : rc;
}

// ------------------------------------------------------------------------------------------------
// voice prefixes (include/q3tts.h): the Talker runs the voice rows once, at positions 0 .. P - 1, straight into the prefix store — the
// layers of that one run are handed the store's view, a cache of one slot and np = ceil(P / 64) * 64 positions — so no slot's
// state changes. Same launches, same rows, same positions as the whole prompt's prefill: the same K/V bits.
// ------------------------------------------------------------------------------------------------
extern "C" int q3tts_prefix_create(q3tts_engine* e, const q3tts_prompt_desc* p, const float* embd, int32_t n_tok, q3tts_prefix** out) {
    if (!e || !out) return q3_set_err(e, Q3TTS_ERR_INVALID, "null argument");
    Q3_NOT_IN_SESSION(e);
    *out = nullptr;
    TRY(voice_job_check(e, p, embd, n_tok));
    Q3_HIP(e, hipSetDevice(e->cfg.device));
    hipStream_t s = e->stream;
    int n = n_tok;
    if (p) TRY(build_prompt_dev(e, p, e->pf.x, e->cfg.n_ctx - 1, &n, PROMPT_VOICE));
    else Q3_HIP(e, hipMemcpyAsync(e->pf.x, embd, (size_t)n * e->cfg.model.d_embed * 4, hipMemcpyHostToDevice, s));
    q3tts_prefix* x = new q3tts_prefix();
    x->e = e;
    const int rc = prefix_store_alloc(e, x, n);
    if (rc != Q3TTS_OK) { q3_prefix_free(x); return rc; }
    auto fail = [&](int code, const std::string& msg) { hipStreamSynchronize(s); q3_prefix_free(x); return q3_set_err(e, code, msg); };
    const Q3KvCache store = prefix_cache_view(e->T, x);
    const int rl = prefill_layers(e, group_maps({Adm{0, nullptr, n, 0, 0, 0, nullptr, 0}}, n), nullptr, &store);  // one run: rows 0 .. n - 1 of slot 0
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
    q3_prefix_free(x);
    return Q3TTS_OK;
}

// q3_generate.hip — the scheduler of libq3tts: row planning, the frame-step chunk, batched prefill and admission, voice prefixes, the
// vocoder's chunk boundary, and the drivers built on them: q3tts_generate_batch and q3tts_stream_* here, the session worker in
// q3_session.hip. The loop restates the reference's run_inference_stream (src/tts/engine.rs:445-656) with every per-frame decision on
// the device: one graph replay = sample -> 15 predictor passes -> feedback -> Talker step, no host round trip (the reference crosses
// the host<->backend boundary >= 33 times per frame).
#include "q3_engine.h"

#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>

// Map the live slots onto rows [0, n) of the smallest bucket that holds them (idle slots fill the rest: every row keeps
// a distinct, valid slot). Row-indexed state that outlives a frame (the Talker logits) moves with its slot.
int q3_plan_rows(q3tts_engine* e, const std::vector<int>& live_in) {
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

double q3_now_ms() {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

// CH frame steps over the current row bucket; afterwards the slot mirror is on the host. *dev_ms: the device time (ms).
int q3_run_chunk(q3tts_engine* e, int CH, float* dev_ms) {
    hipStream_t s = e->stream;
    Q3Lane& L = e->lane;
    const double hp0 = q3_now_ms();
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
    const double hp1 = q3_now_ms();
    Q3_HIP(e, hipStreamSynchronize(s));
    e->hp_launch += hp1 - hp0; e->hp_sync += q3_now_ms() - hp1;  // Q3TTS_HOST_PROF: host wall of the launch part / of the wait
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

// items[i] enters its slot; rc[i] = status of item i (a failing item does not stop the others)
int q3_admit_items(q3tts_engine* e, const Q3AdmItem* items, int count, int* rc) {
    std::vector<Adm> grp;
    int total = 0;
    for (int i = 0; i < count; ++i) {
        const Q3AdmItem& it = items[i];
        const q3tts_request* r = it.r;
        rc[i] = Q3TTS_OK;
        if (!r) {  // a prefill-only prefix job: 1 <= rows < n_ctx, as q3tts_prefix_create
            if (!it.keep || (it.voice != nullptr) == (it.embd != nullptr)) { rc[i] = q3_set_err(e, Q3TTS_ERR_INVALID, "prefix: give exactly one of a voice desc or host rows"); continue; }
            if (it.embd && (it.n_tok <= 0 || it.n_tok >= e->cfg.n_ctx)) { rc[i] = q3_set_err(e, Q3TTS_ERR_INVALID, "prefix: n_tok outside 1 .. n_ctx - 1"); continue; }
            int n = 0;
            TRY(place_rows(e, grp, total, e->cfg.n_ctx - 1, it.embd, it.n_tok, it.voice, PROMPT_VOICE, false, &n));
            if (n < 0) rc[i] = n;
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
        if (r->prompt_embd && (r->n_tok <= 0 || P + r->n_tok > e->cfg.n_ctx)) { rc[i] = q3_set_err(e, Q3TTS_ERR_INVALID, "n_tok out of range"); continue; }
        if (!r->prompt_embd && !r->prompt) { rc[i] = q3_set_err(e, Q3TTS_ERR_INVALID, "request has neither prompt_embd nor prompt"); continue; }
        int n = 0;
        TRY(place_rows(e, grp, total, e->cfg.n_ctx, r->prompt_embd, r->n_tok, r->prompt, x ? PROMPT_TEXT : PROMPT_WHOLE, r->text_stream == 1, &n));
        if (n < 0) rc[i] = n;
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
int q3_admit_many(q3tts_engine* e, const int* slots, const q3tts_request* const* reqs, int count, int* rc) {
    std::vector<Q3AdmItem> items(count);
    for (int i = 0; i < count; ++i) { items[i] = Q3AdmItem{}; items[i].slot = slots[i]; items[i].r = reqs[i]; }
    return q3_admit_items(e, items.data(), count, rc);
}

static int admit(q3tts_engine* e, int b, const q3tts_request* r) {
    int rc = Q3TTS_OK;
    int st = q3_admit_many(e, &b, &r, 1, &rc);
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
    x->e = e;
    const int rc = prefix_store_alloc(e, x, n);
    if (rc != Q3TTS_OK) { q3_prefix_free(x); return rc; }
    auto fail = [&](int code, const std::string& msg) { hipStreamSynchronize(s); q3_prefix_free(x); return q3_set_err(e, code, msg); };
    std::vector<int> pos(n), zero(n, 0);
    for (int i = 0; i < n; ++i) pos[i] = i;
    uint16_t *kc = t.kc, *vc = t.vc, *kd = t.kd, *vd = t.vd; const size_t ls = t.layer_stride; const int nc = t.n_ctx;
    t.kc = x->k; t.vc = x->v; t.layer_stride = (size_t)t.Hkv * x->np * t.hd; t.n_ctx = x->np;
    if (t.kv8) { const size_t quants = t.L * t.layer_stride; t.kd = (uint16_t*)((int8_t*)x->k + quants); t.vd = (uint16_t*)((int8_t*)x->v + quants); }  // (the scales follow the quants)
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
    q3_prefix_free(x);
    return Q3TTS_OK;
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

// the pieces of a chunk boundary that the three drivers share (q3_engine.h)
int q3_codes_back(q3tts_engine* e, int b, q3tts_result* o) {
    const int ncb = e->cfg.model.n_codebooks;
    const Q3Slot& st = e->slots_host[b];
    o->n_frames = st.n_frames; o->hit_eos = st.hit_eos;
    o->codes = (int32_t*)malloc(sizeof(int32_t) * (size_t)std::max(1, st.n_frames * ncb));
    if (!o->codes) return q3_set_err(e, Q3TTS_ERR_OOM, "malloc");
    if (st.n_frames > 0)
        Q3_HIP(e, hipMemcpyAsync(o->codes, e->codes + (size_t)b * e->cfg.max_steps_cap * ncb, sizeof(int32_t) * (size_t)st.n_frames * ncb,
                                 hipMemcpyDeviceToHost, e->stream));
    return Q3TTS_OK;
}
int q3_retire_slot(q3tts_engine* e, int b, hipStream_t evs) {
    Q3Slot* st = e->slots_host + e->B + b;
    memset(st, 0, sizeof(*st));
    Q3_HIP(e, hipMemcpyAsync(e->slots + b, st, sizeof(Q3Slot), hipMemcpyHostToDevice, e->stream));
    Q3_HIP(e, hipEventRecord(e->fin_ev[b], evs));
    return Q3TTS_OK;
}
int q3_emit_count(const q3tts_engine* e, int ns, bool done, long long delivered) {
    const Q3Resamp& r = e->rs_out;
    return (int)((e->out_rate ? (done ? q3_resample_N(ns, r.L, r.M) : q3_resample_D(ns, r.L, r.M, r.H)) : ns) - delivered);
}
// Results of a finished slot. The codes come back on the decoder stream at once; the PCM (pinned host buffer) is copied
// on the vocoder stream. With `defer` the call does not wait for the vocoder: the copy is enqueued behind the slot's last
// vocoder chunk, `fin_ev` is recorded after it and the caller completes the result later (complete_result), so the next
// decode chunk is launched while the vocoder is still working.
static int finalize(q3tts_engine* e, int b, const q3tts_request* r, q3tts_result* o, const SlotRun& sr, double t0, bool defer = false,
                    hipEvent_t fin_ev = nullptr, int ri = -1) {
    TRY(q3_codes_back(e, b, o));
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
    o->total_ms = (float)(q3_now_ms() - t0);
    o->status = defer ? Q3TTS_ERR_STATE : Q3TTS_OK;  // a deferred result becomes OK in complete_result
    return Q3TTS_OK;
}

static int complete_result(q3tts_engine* e, q3tts_result* o, hipEvent_t fin_ev, double t0) {
    Q3_HIP(e, hipEventSynchronize(fin_ev));
    o->total_ms = (float)(q3_now_ms() - t0);
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
    const double t0 = q3_now_ms();
    std::vector<int> pending(B, -1);  // request whose PCM copy is still in flight on the vocoder stream, per slot
    auto drain = [&](int b) -> int {
        if (pending[b] >= 0) { TRY(complete_result(e, &outs[pending[b]], e->fin_ev[b], t0)); pending[b] = -1; }
        return Q3TTS_OK;
    };
    int next = 0, done = 0;
    double dec_ms = 0, pre_ms = 0, voc_ms = 0;
    static const bool host_prof = [] { const char* ev = getenv("Q3TTS_HOST_PROF"); return ev && atoi(ev); }();  // host wall time per phase of this loop, to stderr
    double hp_admit = 0, hp_chunk = 0, hp_voc = 0, hp_fin = 0, hp_tail = 0, hp_t = q3_now_ms();
    auto hp_lap = [&](double& acc) { if (host_prof) { const double t = q3_now_ms(); acc += t - hp_t; hp_t = t; } };
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
                TRY(q3_plan_rows(e, live));
            }
            if (!as.empty()) {
                Q3_HIP(e, hipEventRecord(e->ev0, s));
                admitted = true;
                std::vector<int> rcs(as.size());
                TRY(q3_admit_many(e, as.data(), ar.data(), (int)as.size(), rcs.data()));
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
        TRY(q3_run_chunk(e, CH, &ms));
        hp_lap(hp_chunk);
        dec_ms += ms; steps += CH;
        if (admitted) { hipEventElapsedTime(&ms, e->ev0, e->ev2); pre_ms += ms; }
        for (int b = 0; b < B; ++b) if (run[b].req >= 0) { ctx_tokens += (long long)e->slots_host[b].cur_pos * CH; live_slot_steps += CH; }
        if (e->voc) {
            const double tv0 = q3_now_ms();
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
                const double tn = q3_now_ms();
                for (int b = 0; b < B; ++b) if (run[b].req >= 0 && run[b].t_first == 0 && voc_frames[b] > 0) run[b].t_first = tn;
            }
            voc_ms += q3_now_ms() - tv0;
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
                hp_admit, hp_chunk, e->hp_launch, e->hp_sync, dec_ms, steps, hp_voc, hp_fin, hp_tail, q3_now_ms() - t0);
        e->hp_launch = e->hp_sync = 0;
    }
    e->tm.prefill_ms = (float)pre_ms; e->tm.decode_ms = (float)dec_ms; e->tm.vocoder_ms = (float)voc_ms;
    e->tm.total_ms = (float)(q3_now_ms() - t0); e->tm.frame_steps = steps; e->tm.frame_step_ms = steps ? (float)(dec_ms / steps) : 0.0f;
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
    const int c = q3_emit_count(e, after, fin, e->out_rate ? st->delivered : before);
    if (e->out_rate) {
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
    st->e = e; st->req = *req; st->t0 = q3_now_ms();
    int rc = q3_plan_rows(e, std::vector<int>{0});
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
            TRY(q3_run_chunk(e, 4, nullptr));
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
            if (st->t_first == 0) st->t_first = q3_now_ms();
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
    hipMemcpyAsync(e->slots_host, e->slots, sizeof(Q3Slot), hipMemcpyDeviceToHost, e->stream);
    hipStreamSynchronize(e->stream);
    if (out) {
        memset(out, 0, sizeof(*out));
        SlotRun sr; sr.t_first = st->t_first;
        q3tts_request r = st->req; r.want_pcm = 1;
        rc = finalize(e, 0, &r, out, sr, st->t0);
    }
    q3_retire_slot(e, 0, e->stream);  // the slot is retired even if the caller stops early (a stream's vocoder work runs on the decode stream)
    hipStreamSynchronize(e->stream);
    --e->streams_open;
    e->ts_slot[0] = 0;
    delete st;
    return rc;
}

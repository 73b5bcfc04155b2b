// q3_generate.hip — the scheduler of libq3tts: row planning, the frame-step chunk, the vocoder's chunk boundary, the pinned result pool
// and result helpers, and the drivers built on them: q3tts_generate_batch and q3tts_stream_* here, the session worker in
// q3_session.hip. Admission (batched prefill, voice prefixes) is q3_admit.hip. The loop restates the reference's run_inference_stream (src/tts/engine.rs:445-656) with every per-frame decision on
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
float* q3_pin_alloc(size_t bytes) { return pin_alloc(bytes); }
void q3_pin_free(float* p) { pin_free(p); }

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
    const long long nt = q3_pcm_valid(e, ns, done);  // with a speed set the resampler's row is the tempo row: N_t(ns) / D_t(ns) valid samples, the same `done`
    return (int)((e->out_rate ? (done ? q3_resample_N(nt, r.L, r.M) : q3_resample_D(nt, r.L, r.M, r.H)) : nt) - delivered);
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
        if (e->speed) {  // the finished row stretched: N_t(ns) samples in the slot's tempo row
            const char fin = 1;
            TRY(q3_tempo_slots(e, &b, &ns, &fin, 1, e->vstream));
            ns = (int)q3_tempo_N(ns, e->speed); from = e->tp_row + (size_t)b * e->tp_stride;
        }
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
    const int c = q3_emit_count(e, after, fin, e->out_rate || e->speed ? st->delivered : before);
    if (e->speed) {  // the tempo row first: what `after` samples decide, on the stream the vocoder just ran on
        const int b0 = 0; const char f = fin ? 1 : 0;
        TRY(q3_tempo_slots(e, &b0, &after, &f, 1, s));
        from = e->tp_row + st->delivered;
    }
    if (e->out_rate) {
        TRY(q3_resample_slot(e, 0, st->delivered, c, (int)q3_pcm_valid(e, after, fin), fin, s));
        from = e->rs_stage;
    }
    if (e->out_rate || e->speed) st->delivered += std::max(c, 0);
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
    if (rc == Q3TTS_OK) rc = q3_admit(e, 0, req);
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
            if (after > before || ((e->out_rate || e->speed) && q3_emit_count(e, after, true, st->delivered) > 0))
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

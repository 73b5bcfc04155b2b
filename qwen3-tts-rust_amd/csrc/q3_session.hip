// q3_session.hip — sessions (include/q3tts.h): continuous batching with per-request streaming, the serving form of
// run_inference_stream (src/tts/engine.rs:445-656) for many utterances at once. One worker thread per session drives the engine's slots
// between 4-frame chunks, one named phase after the other (step): cancellations, admissions (q3_plan_rows + q3_admit_items), the frame
// steps (q3_run_chunk), the batched vocoder (q3_voc_dispatch, shared with q3tts_generate_batch), then ONE PCM gather launch and ONE
// device-to-host copy of every slot's new samples into a ring of pinned staging buffers. Chunk events are published when that copy's event has fired (queried, never waited
// for while slots are decoding), so decode keeps overlapping the vocoder as in q3tts_generate_batch. DESIGN.md §"Streams".
// Paced requests and swapping: a request whose frame credit is used up is parked like a text-starved one, and with a swap
// arena parked requests leave their slots for waiting ones (swap_out) and return into any free slot (swap_in); q3_swap.hip moves the state.
#include "q3_engine.h"

#include <chrono>
#include <condition_variable>
#include <cstring>
#include <deque>
#include <map>
#include <memory>
#include <thread>

namespace {

constexpr int kRing = Q3TTS_SESSION_RING_DEPTH;
constexpr int kStopping = 1;  // (positive: the worker was told to stop while it waited for staging)

// a submitted request with everything it points to copied
struct SReq {
    uint64_t id = 0;
    q3tts_request r{};
    q3tts_prompt_desc desc{};
    std::vector<float> embd, spk;
    std::vector<uint32_t> text, instr, ref_text;
    std::vector<int32_t> ref_codes;
    // voice work (include/q3tts.h, "voices in a session"). kind 1: a standalone prefix job — desc / embd hold its voice rows (n_tok of
    // them for embd), r is unused. keep: the prefix this entry fills (a job's, or a keep-voice request's with voice_rows as submitted)
    int kind = 0, voice_rows = 0, n_tok = 0;
    q3tts_prefix* keep = nullptr;
    // documents (include/q3tts.h, "documents in a session"): segment `seg` of doc, or (seg < 0) the job that makes doc's voice prefix.
    // Such an entry is internal: its id is in no IdState, so deliver() drops whatever event names it
    struct Doc* doc = nullptr;
    int seg = -1;
};

// One segment of a document (the worker's; append hands new ones over through Doc::incoming)
struct DocSeg {
    std::vector<uint32_t> ids;
    int kind = 0, max_steps = 0;
    bool fresh = true;    // its document row's edges are not reset yet
    bool ended = false;   // its request is done: n is final
    int n = 0;            // valid samples in its document row
    q3tts_result res{};   // its own result (codes), from finish_slots to its SEGMENT event
};

// A document. Its segments run as internal requests behind px; their samples are scanned into `ahead` device rows (segment j: row
// j mod ahead), and the plan (q3_doc_plan) of boundary t is made from the lengths and edges of boundary t - 1, whose table rode that
// boundary's copy into the staging ring.
struct Doc {
    uint64_t id = 0;
    q3tts_request tmpl{};
    q3tts_join_opts join{};
    int ahead = 8;
    q3tts_prefix* px = nullptr;
    bool own_px = false;
    // (mu)
    std::vector<DocSeg> incoming;         // appended, not yet seen by the worker
    bool open = false, finished = false;  // more segments may follow; its final event is on its way
    int n_given = 0;                      // segments submitted so far
    std::vector<q3tts_long_info> info;    // the delivered segments (q3tts_session_document_info)
    long long n_delivered = 0;
    // worker only
    bool accepted = false, w_open = true, ended = false;
    int failed = Q3TTS_OK;                // a segment failed by itself, or the document's own refusal: torn down at the next boundary
    std::vector<DocSeg> segs;
    int queued = 0;                       // segments [0, queued) are in the FIFO, in a slot or done
    float* rows = nullptr; int32_t* edges = nullptr; size_t stride = 0, bytes = 0;  // bytes: what e->dev_bytes carries for the rows
    Q3DocState st{};
    std::vector<Q3DocSegNow> snap;        // per segment: the latest snapshot whose table has landed
    struct Pend { int seg, n; bool ended; };
    std::vector<Pend> pend; int pend_ring = -1; size_t pend_off = 0;  // the snapshot on its way: ring buffer, byte offset of its table
    bool touch = false, clipped = false;  // a segment's length or end changed at this boundary; the last plan ran out of room
    long long frames = 0; bool all_eos = true;
    // its own speed / output rate (both 0: nothing below is touched). rg: the pipeline's counts (q3_doc_ring_step); ring_j / ring_t: the
    // two rings, allocations of their own; aux: the stretch's window and the p of the last decided frame
    int speed = 0, out_rate = 0;
    Q3DocRing rg{}; Q3Resamp rs{};
    float* ring_j = nullptr; float* ring_t = nullptr; float* aux = nullptr;
    std::vector<Q3DocDone> due;           // segments whose piece is joined and whose outputs are not all delivered yet, in order
    bool flow = false;                    // a stage moved at the last boundary and the document is not out yet: the next one may move again
    bool ringed() const { return speed || out_rate; }
};
// a rate's exit of one document at this boundary (k_doc_resample writes the staging buffer: issued behind take_ring, with the pieces)
struct DocExit { Doc* d; Q3DocRingStep st; size_t at; };

// a q3tts_session_clone call waiting for the worker (the caller's stack; mu guards done)
struct CloneJob {
    const float* audio = nullptr; int64_t n = 0; int rate = 0;
    int64_t* codes = nullptr; int cap = 0; int32_t* n_frames = nullptr; float* spk = nullptr;
    int rc = Q3TTS_OK; bool done = false; std::string err;
};

struct SEv {  // an event on its way to the consumer
    uint64_t id = 0;
    int kind = Q3TTS_EV_NONE, status = Q3TTS_OK, ring = -1, n = 0, is_final = 0;
    size_t off = 0;      // CHUNK: first sample in the ring buffer
    q3tts_result res{};  // final events
};

struct Batch {  // the events of one chunk boundary, published together once the copy into ring buffer `ring` has landed (-1: no copy)
    int ring = -1;
    std::vector<SEv> evs;
};

struct IdState {
    bool cancelled = false, queued = true, final_ready = false;
    double t_submit = 0, t_first = 0;
    // streamed text (include/q3tts.h, "streaming text input"): the request's trailing ids T so far (tts_eos last once closed)
    bool ts = false, closed = true;
    std::vector<int32_t> T;
    // pacing (include/q3tts.h, "paced requests and swapping"): the frame credit granted so far; kNoLimit once the limit is lifted
    bool paced = false;
    long long credit = 0;
};

constexpr long long kNoLimit = -1;   // a paced request's credit after q3tts_session_grant(frames < 0)
constexpr long long kNotPaced = -2;  // (Boundary::cr_adm) the popped entry was submitted without a credit

struct SSlot {
    std::unique_ptr<SReq> req;  // null: the slot is free
    int delivered = 0;          // samples handed out in chunks so far
    // streamed text: t_len / t_closed: the worker's view of T; t_up: entries of T on the device. parked: the slot sits out of the frame
    // steps (its device record is idle) until its text suffices; rec: its real record meanwhile
    bool ts = false, t_closed = true, parked = false;
    int t_len = 0, t_up = 0;
    Q3Slot rec{};
    // pacing: the worker's view of the credit (collect refreshes it). parked_at: the boundary count when the slot was parked
    bool paced = false;
    long long credit = 0;
    uint64_t parked_at = 0;
};

struct TextNow { bool have = false, closed = true; std::vector<int32_t> T; };  // a streamed request's text as of this boundary

// A request that left its slot: the slot's bookkeeping as it was when parked, the vocoder's host state, and its block
struct Swapped {
    SSlot sl;
    int voc_frames = 0, frames_done = 0, last_flag = 0, from_slot = -1;
    long long off = -1, bytes = 0;
    unsigned long long ticket = 0;  // the move that wrote the block (q3_swap_move)
    uint64_t ready_at = 0;  // the boundary count when its rule was first seen satisfied again (0: it is not)
    TextNow tn;             // a text_stream request's whole text as of the last collect that saw it change
};

}  // namespace

struct q3tts_session {
    q3tts_engine* e = nullptr;
    int fmt = 0; size_t es = 4;
    size_t ring_cap = 0;            // samples per staging buffer: max_batch x (4 + lookahead_frames) x samples per frame
    void* host[kRing] = {};         // pinned staging ring
    hipEvent_t ev[kRing] = {};      // its copies
    int refs[kRing] = {};           // (mu) chunks of a buffer in the ready queue or held by the consumer
    bool inflight[kRing] = {};      // (worker) its copy is not published yet
    int ring_next = 0;
    void* dev = nullptr;            // the gather's device output (one copy in flight at a time: stream order on the vocoder stream)
    std::mutex mu;                  // guards everything below up to `slots`
    std::condition_variable cv_work, cv_ev, cv_space;
    std::deque<std::unique_ptr<SReq>> pending;
    std::vector<uint64_t> cancels;
    std::map<uint64_t, IdState> ids;  // accepted ids whose final event has not been delivered
    std::deque<SEv> ready;
    std::deque<CloneJob*> clones;        // q3tts_session_clone calls the worker has not run yet
    int clone_waiters = 0;               // callers inside q3tts_session_clone (close waits for them to leave)
    std::condition_variable cv_clone;
    std::vector<q3tts_prefix*> made;     // the prefixes this session created and has not freed
    std::vector<q3tts_prefix*> trash;    // released and no longer named by a queued request: the worker frees them at the next boundary
    std::map<uint64_t, std::shared_ptr<Doc>> doc_ids;  // every document of this session (kept until close: document_info stays readable)
    std::vector<std::shared_ptr<Doc>> docs_new;        // submitted, not yet accepted by the worker
    bool doc_dirty = false;              // a document was submitted, appended to or closed since the worker last looked
    uint64_t next_internal = 1;          // ids of internal entries: bit 63 set
    std::atomic<int> docs_waiting{0};    // entries of docs_new: accept_docs takes mu only when there are some
    std::atomic<long long> doc_mem_cap{-1};  // q3tts_k_session_doc_mem_cap: documents are accepted as if the device had at most this free (< 0: off)
    uint64_t next_id = 1;
    bool stop = false, dead = false;
    bool text_dirty = false;        // q3tts_session_append_text added something the worker has not seen
    int held_ring = -1;             // ring buffer of the chunk the consumer holds (released at its next call)
    int worker_rc = Q3TTS_OK;
    std::string err;
    bool grant_dirty = false;       // q3tts_session_grant changed a credit the worker has not seen
    std::atomic<Q3Swap*> swap{nullptr};  // q3tts_session_set_swap (before the first submission; then the worker's)
    std::atomic<long long> st_out{0}, st_in{0}, st_moved{0}, st_used{0}, st_peak{0}, st_skipped{0};  // q3tts_session_swap_stats
    std::atomic<long long> st_out_us{0}, st_in_us{0}, st_bounds{0};  // q3tts_k_swap_phase_ms: host microseconds in the two phases; boundaries that moved a block
    // worker only
    std::vector<Swapped> out;       // swapped-out requests
    std::vector<std::shared_ptr<Doc>> docs;  // accepted documents without their final event
    struct Limbo { long long off, bytes; unsigned long long ticket; };
    std::vector<Limbo> limbo;       // blocks nobody owns any more whose last move may still be running on a stream (reap_blocks)
    uint64_t seq = 0;               // chunk boundaries so far
    bool evict_stuck = false;       // the last swap_out found no room in the arena; cleared when a block or a slot is freed
    std::vector<SSlot> slots;
    std::vector<int> voc_frames;
    std::deque<Batch> flight;
    std::thread th;
};

namespace {

thread_local std::string g_serr;

int serr(q3tts_session* s, int code, const std::string& m) {
    if (s) s->err = m;
    g_serr = m;
    return code;
}

void copy_result_free(q3tts_result& r) { q3tts_result_free(&r); r = q3tts_result{}; }

// (mu held) an event reaches the ready queue; a cancelled id's chunks are dropped and its DONE / FAILED become CANCELLED
void deliver(q3tts_session* s, SEv& v, double t) {
    auto it = s->ids.find(v.id);
    if (it == s->ids.end() || it->second.final_ready) { copy_result_free(v.res); return; }
    IdState& st = it->second;
    if (v.kind == Q3TTS_EV_PREFIX) {  // a job's only event, or the one in front of a keep-voice request's own (cancelled or not: the store's fate is news)
        if (v.is_final) st.final_ready = true;
        s->ready.push_back(v);
        return;
    }
    if (v.kind == Q3TTS_EV_SEGMENT) {  // a document's segment is out: not a final event; a cancelled document publishes no more of them
        if (st.cancelled) copy_result_free(v.res); else s->ready.push_back(v);
        return;
    }
    if (st.cancelled) {
        if (v.kind == Q3TTS_EV_CHUNK) return;
        if (v.kind != Q3TTS_EV_CANCELLED) { copy_result_free(v.res); v.kind = Q3TTS_EV_CANCELLED; v.status = Q3TTS_OK; }
    }
    if (v.kind == Q3TTS_EV_CHUNK) {
        if (v.ring >= 0) ++s->refs[v.ring];
        if (st.t_first == 0) st.t_first = t;
    } else {
        v.is_final = 1;
        v.res.first_chunk_ms = st.t_first > 0 ? (float)(st.t_first - st.t_submit) : 0.0f;
        v.res.total_ms = (float)(t - st.t_submit);
        st.final_ready = true;
    }
    s->ready.push_back(v);
}

SEv final_ev(uint64_t id, int kind, int status) {
    SEv v; v.id = id; v.kind = kind; v.status = status; v.is_final = 1; v.res.status = status;
    return v;
}

SEv prefix_ev(uint64_t id, int status, bool is_final) {
    SEv v; v.id = id; v.kind = Q3TTS_EV_PREFIX; v.status = status; v.is_final = is_final ? 1 : 0; v.res.status = status;
    return v;
}

// (mu held) a released prefix that is settled and that no queued request names goes to the worker, which frees it at the next boundary
void maybe_reap(q3tts_session* s, q3tts_prefix* x) {
    if (!x->released || x->qrefs > 0 || x->state.load() == 0) return;
    if (std::find(s->trash.begin(), s->trash.end(), x) == s->trash.end()) s->trash.push_back(x);
}
// (mu held) a queued request that named x has left the queue
void unref_prefix(q3tts_session* s, const q3tts_prefix* cx) {
    q3tts_prefix* x = const_cast<q3tts_prefix*>(cx);
    if (!x || x->e != s->e) return;
    if (x->qrefs > 0) --x->qrefs;
    maybe_reap(s, x);
}
// (mu held) the prefix of an entry that will not be admitted fails with `status`
void fail_keep(q3tts_session* s, q3tts_prefix* x, int status) {
    if (!x || x->state.load() != 0) return;
    x->state.store(status, std::memory_order_release);
    maybe_reap(s, x);
}

// one q3tts_session_clone call, on the engine's stream between two chunk boundaries: the bodies of q3tts_resample (a clip at another
// rate first, as create_voice_file(resample=True) does), q3tts_clone_audio_encode and q3tts_clone_speaker_encode, in that order
void run_clone(q3tts_session* s, CloneJob& j) {
    q3tts_engine* e = s->e;
    const float* a = j.audio; int64_t n = j.n;
    std::vector<float> rs;
    int rc = Q3TTS_OK;
    if (j.rate != 24000) {
        int L = 0, M = 0, H = 0, T = 0;
        if (q3_resample_plan(j.rate, 24000, &L, &M, &H, &T) != Q3TTS_OK) rc = q3_set_err(e, Q3TTS_ERR_INVALID, "clone: the resampler cannot convert the clip's rate to 24000 Hz");
        else {
            rs.resize((size_t)std::max<long long>(1, q3_resample_N(n, L, M)));
            int64_t n_out = 0;
            rc = q3_resample_run(e, a, n, j.rate, 24000, rs.data(), (int64_t)rs.size(), &n_out);
            a = rs.data(); n = n_out;
        }
    }
    if (rc == Q3TTS_OK && j.codes) rc = q3_clone_audio_encode_run(e, a, n, j.codes, j.cap, j.n_frames);
    if (rc == Q3TTS_OK && j.spk) rc = q3_clone_speaker_encode_run(e, a, n, j.spk);
    if (rc != Q3TTS_OK) { std::lock_guard<std::mutex> lk(e->err_mu); j.err = e->err; }
    j.rc = rc;
}

// (worker) A swapped-out request gives its block up. The bytes return to the arena only when the last move that touched them — `ticket`:
// the save that wrote the block, or the load that read it — has run on BOTH streams: the next block carved over them has another layout,
// so its decode-stream half may cover what was this block's vocoder-stream half, and nothing orders the two streams. Until then the
// block waits in limbo (and counts as in use).
void drop_block(q3tts_session* s, Swapped& o, unsigned long long ticket) {
    if (o.off < 0) return;
    s->limbo.push_back({o.off, o.bytes, ticket});
    o.off = -1;
}
// (worker) limbo blocks whose move is over go back to the arena; never waits
void reap_blocks(q3tts_session* s) {
    if (s->limbo.empty()) return;
    Q3Swap* sw = s->swap;
    size_t keep = 0;
    for (const auto& l : s->limbo) {
        if (q3_swap_done(sw, l.ticket)) q3_swap_release(sw, l.off, l.bytes);
        else s->limbo[keep++] = l;
    }
    if (keep == s->limbo.size()) return;
    s->limbo.resize(keep);
    s->st_used.store(q3_swap_used(sw), std::memory_order_relaxed);
    s->evict_stuck = false;
}

// publish finished batches in order; wait: block on the first one's copy
int publish(q3tts_session* s, bool wait) {
    q3tts_engine* e = s->e;
    reap_blocks(s);  // (before any event leaves: q3tts_session_swap_stats read behind a final event sees the blocks of finished moves returned)
    while (!s->flight.empty()) {
        Batch& b = s->flight.front();
        if (b.ring >= 0) {
            const hipError_t q = wait ? hipEventSynchronize(s->ev[b.ring]) : hipEventQuery(s->ev[b.ring]);
            if (q == hipErrorNotReady) break;
            if (q != hipSuccess) return q3_set_err(e, Q3TTS_ERR_DEVICE, std::string("session: PCM copy: ") + hipGetErrorString(q));
            s->inflight[b.ring] = false;
        }
        wait = false;
        reap_blocks(s);  // (again behind the batch's copy: what ran in front of it on the vocoder stream is over)
        const double t = q3_now_ms();
        {
            std::lock_guard<std::mutex> lk(s->mu);
            for (SEv& v : b.evs) deliver(s, v, t);
        }
        s->cv_ev.notify_all();
        s->flight.pop_front();
    }
    return Q3TTS_OK;
}

// the waiting q3tts_session_clone calls, run and their callers woken
void serve_clones(q3tts_session* s, const std::vector<CloneJob*>& clones) {
    if (clones.empty()) return;
    for (CloneJob* j : clones) run_clone(s, *j);
    { std::lock_guard<std::mutex> lk(s->mu); for (CloneJob* j : clones) j->done = true; }
    s->cv_clone.notify_all();
}

// ring buffer k free: its copy published and every chunk in it released by the consumer (the worker waits: memory does not grow).
// Clone calls are served while it waits: their caller may be the consumer itself, which reads no event until its call returns. (This
// boundary's frame steps are complete by now — q3_run_chunk synchronised the engine's stream — and the next have not begun.)
int take_ring(q3tts_session* s, int k) {
    while (s->inflight[k]) { const int rc = publish(s, true); if (rc) return rc; }
    for (;;) {
        std::vector<CloneJob*> clones;
        {
            std::unique_lock<std::mutex> lk(s->mu);
            s->cv_space.wait(lk, [&] { return s->stop || s->refs[k] == 0 || !s->clones.empty(); });
            if (s->stop) return kStopping;
            if (s->clones.empty()) return Q3TTS_OK;
            clones.assign(s->clones.begin(), s->clones.end()); s->clones.clear();
        }
        serve_clones(s, clones);
    }
}

void free_slot(q3tts_session* s, int b) {
    SSlot& sl = s->slots[b];
    sl.req.reset(); sl.ts = false; sl.parked = false; sl.paced = false;
    s->e->ts_slot[b] = 0;
    s->evict_stuck = false;
}

// the slot's device record (between chunks; the caller synchronises the stream before `rec` can change)
int put_record(q3tts_engine* e, int b, const Q3Slot* rec) {
    Q3_HIP(e, hipMemcpyAsync(e->slots + b, rec, sizeof(Q3Slot), hipMemcpyHostToDevice, e->stream));
    return Q3TTS_OK;
}
// Parking: the slot leaves the frame steps with everything it needs to come back. Its K/V, codes and vocoder state stay
// where they are; the two rows that outlive a frame go to the slot's side rows (any row of the bucket is overwritten by the GEMMs, and
// q3_plan_rows may move it), the real record stays on the host (q3_run_chunk refreshes the mirror from the idle one on the device).
int park(q3tts_session* s, int b, const Q3Slot& rec) {
    static const Q3Slot idle{};
    q3tts_engine* e = s->e;
    SSlot& sl = s->slots[b];
    TRY(q3_park_rows(e, b, true));
    sl.rec = rec; sl.parked = true; sl.parked_at = s->seq;
    return put_record(e, b, &idle);
}
// after q3_plan_rows with the slot among the live ones: the rows into its row, the record back
int resume(q3tts_session* s, int b) {
    q3tts_engine* e = s->e;
    SSlot& sl = s->slots[b];
    TRY(q3_park_rows(e, b, false));
    sl.parked = false;
    e->slots_host[b] = sl.rec;
    return put_record(e, b, &sl.rec);
}
bool text_ready(const SSlot& sl, int n_frames) {
    return !sl.ts || q3tts_k_text_ready(sl.t_len + (sl.t_closed ? 0 : 1), sl.t_closed ? 1 : 0, n_frames) != 0;  // x = the prompt's id + T without tts_eos
}
// the two rules of taking the next chunk at n_frames: the text reaches it (streaming text input) and the credit covers it (pacing)
bool slot_ready(const SSlot& sl, int n_frames) {
    return text_ready(sl, n_frames) && (!sl.paced || q3tts_k_credit_ready(sl.credit, n_frames) != 0);
}
bool gated(const SSlot& sl) { return sl.ts || sl.paced; }

// What one chunk boundary (step) carries from phase to phase, destroyed when step returns. Per member: the phase that fills it and,
// where an asynchronous upload reads host memory, the synchronisation that memory outlives. (The slots' records live in SSlot and in
// the engine's staging half: `moved` and `retired` say that an upload of one is in flight.)
struct Boundary {
    explicit Boundary(int B) : tn(B), cool(B, 0), nf(B, 0), run(B, 0) {}
    std::vector<long long> cr_adm;               // collect: adm[i]'s credit as of the pop (kNotPaced: submitted without one)
    int waiting = 0;                             // collect: admissible entries left at the queue's head for want of a slot (swap_out)
    // collect, under one hold of mu
    std::vector<uint64_t> cancels;               // ids to retire (cancel_slots)
    std::vector<q3tts_prefix*> trash;            // released prefixes: voice_work frees them behind a synchronise of the decode stream
    std::vector<CloneJob*> clones;               // q3tts_session_clone calls (voice_work)
    std::vector<std::unique_ptr<SReq>> orphans;  // popped entries whose prefix failed: FAILED without a slot (voice_work)
    // the popped entries that get a slot, in FIFO order. The admission's uploads read their rows: an entry that does not move into a slot
    // (a prefix job, a refused request) lives until step returns, behind the synchronise plan_and_admit makes for exactly these
    std::vector<std::unique_ptr<SReq>> adm;
    // the text of slot b / of adm[i], from the same hold of mu as the pop. plan_and_admit moves tn_adm[i] to its slot's tn; resume_and_feed
    // uploads from tn[b].T (q3_text_rows_set synchronises before it returns)
    std::vector<TextNow> tn, tn_adm;
    // the worker's phases
    Batch bt;                  // the boundary's events in order: orphans' FAILED, CANCELLED, per admitted item PREFIX then FAILED, CHUNKs, DONE
    std::vector<char> cool;    // cancel_slots: retired at this boundary, so not admitted into before the next (its staging record is being uploaded)
    std::vector<int> nf;       // park_starved, plan_and_admit: a text_stream slot's frames so far (a parked slot's from the record it kept)
    bool retired = false;      // cancel_slots: a staging-half record is being uploaded; until q3_run_chunk's synchronise or the idle return's
    bool moved = false;        // park / resume: an upload reads SSlot::rec; until the synchronise that ends resume_and_feed
    bool made_prefix = false;  // plan_and_admit: a PREFIX event says a store is written; it leaves behind q3_run_chunk's synchronise or the idle return's
    std::vector<char> run;     // run_frames: the slots that take this boundary's frame steps (vocoder dispatch, gather_pcm)
    std::vector<int> fin;      // gather_pcm: slots whose utterance ended. finish_slots' copies into their DONE events' codes end at its synchronise
};

// the documents' phases (below, in front of step)
void feed_docs(q3tts_session* s);
void doc_slot_scan(q3tts_session* s, int b, int ns, bool done, std::vector<Q3DocScan>& scans, std::vector<int32_t*>& resets);
int doc_emit(q3tts_session* s, Boundary& bd, size_t* cur, std::vector<Q3DocPiece>& ents, std::vector<DocExit>& exits, std::vector<SEv>& evs,
             std::vector<std::shared_ptr<Doc>>& finished);
hipError_t doc_free(q3tts_engine* e, Doc& d);
int end_doc(q3tts_session* s, Boundary& bd, const std::shared_ptr<Doc>& dp, int kind, int status, const q3tts_result* res);

// (mu held) id's streamed text; T is copied only when the device lacks some of it (it holds t_up entries)
void text_now(q3tts_session* s, uint64_t id, int t_up, TextNow& t) {
    auto it = s->ids.find(id);
    if (it == s->ids.end() || !it->second.ts) return;
    t.have = true; t.closed = it->second.closed;
    if ((int)it->second.T.size() != t_up) t.T = it->second.T;
}

// 1. what the callers left since the last boundary, under one hold of mu: cancels, released prefixes, clone calls, the queue's head, and
// the text of the running slots and of the entries just popped
void collect(q3tts_session* s, Boundary& bd) {
    q3tts_engine* e = s->e;
    const int B = e->B;
    int nfree = 0;
    for (int b = 0; b < B; ++b) if (!s->slots[b].req) ++nfree;
    std::lock_guard<std::mutex> lk(s->mu);
    // credits first: a swapped-out request whose rule holds again takes a free slot ahead of the queue's head
    s->grant_dirty = false;
    for (int b = 0; b < B; ++b)
        if (s->slots[b].req && s->slots[b].paced) { auto it = s->ids.find(s->slots[b].req->id); if (it != s->ids.end()) s->slots[b].credit = it->second.credit; }
    for (Swapped& o : s->out) {
        auto it = s->ids.find(o.sl.req->id);
        if (it == s->ids.end()) continue;
        if (o.sl.paced) o.sl.credit = it->second.credit;
        if (o.sl.ts && ((int)it->second.T.size() != o.sl.t_len || it->second.closed != o.sl.t_closed || !o.tn.have)) {
            o.tn.have = true; o.tn.closed = it->second.closed; o.tn.T = it->second.T;
            o.sl.t_closed = o.tn.closed; o.sl.t_len = (int)o.tn.T.size();
        }
        const bool rdy = !it->second.cancelled && slot_ready(o.sl, o.sl.rec.n_frames);
        if (!rdy) o.ready_at = 0;
        else { if (!o.ready_at) o.ready_at = s->seq; --nfree; }
    }
    bd.cancels.swap(s->cancels);
    bd.trash.swap(s->trash);
    bd.clones.assign(s->clones.begin(), s->clones.end()); s->clones.clear();
    feed_docs(s);
    // the FIFO's head: a request that names a pending prefix waits, and so does everything behind it; one whose prefix failed
    // fails without a slot; a prefix job takes a free slot for this boundary as a request does
    while (!s->pending.empty()) {
        SReq& f = *s->pending.front();
        const q3tts_prefix* x = f.kind == 0 ? f.r.prefix : nullptr;
        const int xs = x && x->e == e ? x->state.load(std::memory_order_acquire) : 1;
        if (xs == 0) break;
        if (xs == 1 && nfree <= 0) break;
        const bool own = f.doc == nullptr;  // (a document's entries are internal: no IdState)
        if (own) s->ids[f.id].queued = false;
        unref_prefix(s, x);
        if (xs < 0) bd.orphans.push_back(std::move(s->pending.front()));
        else { --nfree; bd.cr_adm.push_back(own && s->ids[f.id].paced ? s->ids[f.id].credit : kNotPaced); bd.adm.push_back(std::move(s->pending.front())); }
        s->pending.pop_front();
    }
    if (s->swap)  // what still waits at the head and could enter a slot: swap_out makes room for it
        for (const auto& q : s->pending) {
            const q3tts_prefix* x = q->kind == 0 ? q->r.prefix : nullptr;
            if ((x && x->e == e ? x->state.load(std::memory_order_acquire) : 1) != 1) break;
            ++bd.waiting;
        }
    s->text_dirty = false;
    for (int b = 0; b < B; ++b) if (s->slots[b].req && s->slots[b].ts) text_now(s, s->slots[b].req->id, s->slots[b].t_up, bd.tn[b]);
    bd.tn_adm.resize(bd.adm.size());
    for (size_t i = 0; i < bd.adm.size(); ++i) if (bd.adm[i]->r.text_stream == 1) text_now(s, bd.adm[i]->id, -1, bd.tn_adm[i]);
}

// 2. voice work that needs no slot: requests whose prefix failed, released prefixes (the admissions that copied them are behind us on
// the stream), clone calls
int voice_work(q3tts_session* s, Boundary& bd) {
    q3tts_engine* e = s->e;
    for (auto& q : bd.orphans) {
        q3_set_err(e, Q3TTS_ERR_INVALID, "prefix: the request names a prefix that failed");
        if (q->doc) { if (q->doc->failed == Q3TTS_OK) q->doc->failed = Q3TTS_ERR_INVALID; continue; }
        bd.bt.evs.push_back(final_ev(q->id, Q3TTS_EV_FAILED, Q3TTS_ERR_INVALID));
    }
    if (!bd.trash.empty()) {
        Q3_HIP(e, hipStreamSynchronize(e->stream));
        std::lock_guard<std::mutex> lk(s->mu);
        for (q3tts_prefix* x : bd.trash) {
            s->made.erase(std::remove(s->made.begin(), s->made.end(), x), s->made.end());
            q3_prefix_free(x);
        }
    }
    serve_clones(s, bd.clones);
    return Q3TTS_OK;
}

// 3. cancellations: the slot is retired now and admitted into again from the next boundary on
int cancel_slots(q3tts_session* s, Boundary& bd) {
    for (uint64_t id : bd.cancels)
        for (int b = 0; b < s->e->B; ++b)
            if (s->slots[b].req && s->slots[b].req->id == id) {
                TRY(q3_retire_slot(s->e, b, s->e->vstream)); free_slot(s, b);
                bd.cool[b] = 1; bd.retired = true;
                bd.bt.evs.push_back(final_ev(id, Q3TTS_EV_CANCELLED, Q3TTS_OK));
            }
    for (uint64_t id : bd.cancels)  // a swapped-out request holds no slot: its block returns to the arena
        for (size_t i = 0; i < s->out.size(); ++i)
            if (s->out[i].sl.req->id == id) {
                drop_block(s, s->out[i], s->out[i].ticket);
                s->out.erase(s->out.begin() + i);
                bd.bt.evs.push_back(final_ev(id, Q3TTS_EV_CANCELLED, Q3TTS_OK));
                break;
            }
    return Q3TTS_OK;
}

// 4. streamed text and pacing: what arrived since the last boundary, and the two rules — a running slot whose text does not reach 4 more
// frames, or whose credit does not cover them, is parked before the rows are planned without it
int park_starved(q3tts_session* s, Boundary& bd) {
    q3tts_engine* e = s->e;
    for (int b = 0; b < e->B; ++b) {
        SSlot& sl = s->slots[b];
        if (!sl.req || !gated(sl)) continue;
        const TextNow& t = bd.tn[b];
        if (t.have) { sl.t_closed = t.closed; if (!t.T.empty()) sl.t_len = (int)t.T.size(); }
        bd.nf[b] = sl.parked ? sl.rec.n_frames : e->slots_host[b].n_frames;
        if (!sl.parked && !slot_ready(sl, bd.nf[b])) { TRY(park(s, b, e->slots_host[b])); bd.moved = true; }
    }
    return Q3TTS_OK;
}

// 4a. swapping out: while the slots wanted — swapped-out requests whose rule holds again, and what waits at the queue's
// head — exceed the free ones, parked slots leave, longest-parked first, each into a block of the arena; one group of launches for all
// of them. A running slot is never touched, and a slot the arena has no room for simply stays parked. The slot is free from the next
// boundary on (cool, as a cancelled one): fin_ev orders its next occupant behind the vocoder-state copy.
int swap_out(q3tts_session* s, Boundary& bd) {
    q3tts_engine* e = s->e;
    Q3Swap* sw = s->swap;
    if (!sw) return Q3TTS_OK;
    reap_blocks(s);
    int nfree = 0, ready_out = 0;
    for (int b = 0; b < e->B; ++b) if (!s->slots[b].req && !bd.cool[b]) ++nfree;
    for (const Swapped& o : s->out) if (o.ready_at) ++ready_out;
    int need = ready_out + (int)bd.adm.size() + bd.waiting - nfree;
    if (need <= 0) return Q3TTS_OK;
    std::vector<int> cand;
    for (int b = 0; b < e->B; ++b) if (s->slots[b].req && s->slots[b].parked && !slot_ready(s->slots[b], bd.nf[b])) cand.push_back(b);
    std::stable_sort(cand.begin(), cand.end(), [&](int a, int b) { return s->slots[a].parked_at < s->slots[b].parked_at; });
    std::vector<Q3SwapItem> items;
    for (int b : cand) {
        if (need <= 0) break;
        SSlot& sl = s->slots[b];
        Swapped o;
        q3_voc_host_state(e, b, &o.frames_done, &o.last_flag, false);
        o.bytes = q3_swap_block_bytes(e, sw, sl.rec.cur_pos, o.frames_done);
        o.off = q3_swap_alloc(sw, o.bytes);
        if (o.off < 0) { s->st_skipped.fetch_add(1, std::memory_order_relaxed); s->evict_stuck = true; continue; }
        items.push_back(Q3SwapItem{b, sl.rec.cur_pos, o.frames_done, o.off});
        o.voc_frames = s->voc_frames[b]; o.from_slot = b;
        o.sl = std::move(sl);
        s->out.push_back(std::move(o));
        free_slot(s, b);
        bd.cool[b] = 1;
        --need;
    }
    if (items.empty()) return Q3TTS_OK;
    unsigned long long ticket = 0;
    TRY(q3_swap_move(e, sw, items.data(), (int)items.size(), true, &ticket));
    for (size_t i = s->out.size() - items.size(); i < s->out.size(); ++i) s->out[i].ticket = ticket;
    for (const Q3SwapItem& it : items) Q3_HIP(e, hipEventRecord(e->fin_ev[it.slot], e->vstream));
    s->st_out.fetch_add((long long)items.size(), std::memory_order_relaxed);
    const long long used = q3_swap_used(sw);
    s->st_used.store(used, std::memory_order_relaxed);
    if (used > s->st_peak.load(std::memory_order_relaxed)) s->st_peak.store(used, std::memory_order_relaxed);
    return Q3TTS_OK;
}

// 4b. swapping in: swapped-out requests whose rule holds again take free slots, oldest-ready first and ahead of the admissions (collect
// kept these slots from the queue's head). Each arrives as a parked slot — its rows in the slot's side rows, its record on the host with
// rng_base re-pointed — so plan_and_admit plans a row for it and resume_and_feed brings it back like any parked slot. Its block goes to
// limbo behind the load (drop_block).
int swap_in(q3tts_session* s, Boundary& bd) {
    q3tts_engine* e = s->e;
    Q3Swap* sw = s->swap;
    if (!sw || s->out.empty()) return Q3TTS_OK;
    std::vector<size_t> order;
    for (size_t i = 0; i < s->out.size(); ++i) if (s->out[i].ready_at) order.push_back(i);
    if (order.empty()) return Q3TTS_OK;
    std::stable_sort(order.begin(), order.end(), [&](size_t a, size_t b) { return s->out[a].ready_at < s->out[b].ready_at; });
    std::vector<Q3SwapItem> items;
    std::vector<size_t> taken;
    int b = 0;
    for (size_t i : order) {
        while (b < e->B && (s->slots[b].req || bd.cool[b])) ++b;
        if (b >= e->B) break;
        Swapped& o = s->out[i];
        Q3_HIP(e, hipEventSynchronize(e->fin_ev[b]));  // the previous occupant's vocoder work is done, as before an admission
        items.push_back(Q3SwapItem{b, o.sl.rec.cur_pos, o.frames_done, o.off});
        taken.push_back(i);
        SSlot& sl = s->slots[b];
        sl = std::move(o.sl);
        sl.parked = true; sl.parked_at = s->seq;
        sl.rec.rng_base = b * e->cfg.max_steps_cap;
        s->voc_frames[b] = o.voc_frames;
        q3_voc_host_state(e, b, &o.frames_done, &o.last_flag, true);
        q3_tempo_forget(e, b);  // (the tempo row is rebuilt from the PCM row the block carries: DESIGN.md §24)
        e->ts_slot[b] = sl.ts ? 1 : 0;
        bd.nf[b] = sl.rec.n_frames;
        if (b != o.from_slot) s->st_moved.fetch_add(1, std::memory_order_relaxed);
        ++b;
    }
    if (items.empty()) return Q3TTS_OK;
    unsigned long long ticket = 0;
    TRY(q3_swap_move(e, sw, items.data(), (int)items.size(), false, &ticket));
    std::vector<Q3TextSet> texts;  // the text, whole, from IdState::T as collect copied it; every slot's behind one synchronise
    for (size_t k = 0; k < taken.size(); ++k) {
        Swapped& o = s->out[taken[k]];
        const int sb = items[k].slot;
        SSlot& sl = s->slots[sb];
        if (sl.ts) { texts.push_back(Q3TextSet{sb, o.tn.T.data(), 0, (int)o.tn.T.size(), bd.nf[sb]}); sl.t_up = sl.t_len = (int)o.tn.T.size(); }
        else if (e->ts_used) texts.push_back(Q3TextSet{sb, nullptr, 0, 0, 0});
        drop_block(s, o, ticket);
    }
    TRY(q3_text_rows_set_group(e, texts.data(), (int)texts.size()));
    std::sort(taken.begin(), taken.end());
    for (size_t k = taken.size(); k-- > 0;) s->out.erase(s->out.begin() + taken[k]);
    s->st_in.fetch_add((long long)items.size(), std::memory_order_relaxed);
    return Q3TTS_OK;
}

// 5. the rows are planned for the slots that will run and the popped entries admitted into free slots in one batched prefill; then
// what became of each: PREFIX events, FAILED, or a running slot with its text-stream bookkeeping
int plan_and_admit(q3tts_session* s, Boundary& bd) {
    q3tts_engine* e = s->e;
    const int B = e->B;
    std::vector<int> as;
    std::vector<Q3AdmItem> ar;
    for (int b = 0; b < B && as.size() < bd.adm.size(); ++b)
        if (!s->slots[b].req && !bd.cool[b]) {
            const SReq& q = *bd.adm[as.size()];
            Q3AdmItem it{};
            it.slot = b; it.keep = q.keep;
            if (q.kind == 1) { it.voice = q.embd.empty() ? &q.desc : nullptr; it.embd = q.embd.empty() ? nullptr : q.embd.data(); it.n_tok = q.n_tok; }
            else { it.r = &q.r; it.keep_rows = q.voice_rows; }
            as.push_back(b); ar.push_back(it);
        }
    for (int b : as) Q3_HIP(e, hipEventSynchronize(e->fin_ev[b]));  // the previous occupant's vocoder work is done before the slot's reset
    std::vector<int> live;
    for (size_t i = 0; i < as.size(); ++i) if (bd.adm[i]->kind == 0) live.push_back(as[i]);  // (a prefix job's slot takes no frame step)
    for (int b = 0; b < B; ++b) if (s->slots[b].req && (!s->slots[b].parked || slot_ready(s->slots[b], bd.nf[b]))) live.push_back(b);
    if (!live.empty()) TRY(q3_plan_rows(e, live));
    if (as.empty()) return Q3TTS_OK;
    std::vector<int> rcs(as.size());
    TRY(q3_admit_items(e, ar.data(), (int)as.size(), rcs.data()));
    bool failed = false;
    for (int rc : rcs) failed |= rc != Q3TTS_OK;
    for (size_t i = 0; i < as.size(); ++i) failed |= bd.adm[i]->kind == 1;  // (a job's rows are freed with the boundary as a refused request's are)
    if (failed) Q3_HIP(e, hipStreamSynchronize(e->stream));  // (a refused request's uploads may still read its copy)
    for (size_t i = 0; i < as.size(); ++i) {
        std::unique_ptr<SReq>& q = bd.adm[i];
        const int b = as[i];
        if (q->keep) {  // the store is written behind the group's layers on the stream: ready for everything the worker issues from now on
            q->keep->state.store(rcs[i] == Q3TTS_OK ? 1 : rcs[i], std::memory_order_release);
            if (!q->doc) bd.bt.evs.push_back(prefix_ev(q->id, rcs[i], q->kind == 1));
            bd.made_prefix = true;
            std::lock_guard<std::mutex> lk(s->mu);
            maybe_reap(s, q->keep);
        }
        if (q->kind == 1) continue;  // the slot stays free
        if (rcs[i] != Q3TTS_OK && q->doc) { if (q->doc->failed == Q3TTS_OK) q->doc->failed = rcs[i]; continue; }  // (torn down at the next boundary)
        if (rcs[i] != Q3TTS_OK) { bd.bt.evs.push_back(final_ev(q->id, Q3TTS_EV_FAILED, rcs[i])); continue; }
        SSlot& sl = s->slots[b];
        sl.req = std::move(q); sl.delivered = 0; s->voc_frames[b] = 0;
        sl.ts = sl.req->r.text_stream == 1; sl.parked = false;
        sl.paced = bd.cr_adm[i] != kNotPaced; sl.credit = sl.paced ? bd.cr_adm[i] : 0;  // (a credit is >= 4: frame 0 never waits for it)
        if (!sl.ts) continue;
        std::vector<int32_t> T0;  // what the admission put on the device: the request as submitted
        q3_text_trailing(&sl.req->r, T0);
        sl.t_up = sl.t_len = (int)T0.size(); sl.t_closed = !(sl.req->r.text_open == 1);
        bd.tn[b] = std::move(bd.tn_adm[i]);
        const TextNow& t = bd.tn[b];
        if (t.have) { sl.t_closed = t.closed; if ((int)t.T.size() > sl.t_len) sl.t_len = (int)t.T.size(); }
        bd.nf[b] = 0;
        if (!text_ready(sl, 0)) { TRY(park(s, b, e->slots_host[e->B + b])); bd.moved = true; }  // (the staging half holds the record just admitted)
    }
    return Q3TTS_OK;
}

// 6. parked slots whose text and credit suffice come back (the rows were planned with them), and new text goes to the device
int resume_and_feed(q3tts_session* s, Boundary& bd) {
    q3tts_engine* e = s->e;
    for (int b = 0; b < e->B; ++b) {
        SSlot& sl = s->slots[b];
        if (!sl.req || !gated(sl)) continue;
        if (sl.parked) {
            if (!slot_ready(sl, bd.nf[b])) continue;
            TRY(resume(s, b)); bd.moved = true;
        }
        if (sl.ts && sl.t_len > sl.t_up && (int)bd.tn[b].T.size() >= sl.t_len) {
            TRY(q3_text_rows_set(e, b, bd.tn[b].T.data(), sl.t_up, sl.t_len, bd.nf[b]));
            sl.t_up = sl.t_len;
        }
    }
    if (bd.moved) Q3_HIP(e, hipStreamSynchronize(e->stream));  // (the record uploads read the slots' host copies)
    return Q3TTS_OK;
}

// 7. nothing runs (*idle): what the boundary's events promise is on the device before they leave. Otherwise four frame steps, then
// the vocoder on its stream
int run_frames(q3tts_session* s, Boundary& bd, bool* idle) {
    q3tts_engine* e = s->e;
    *idle = true;
    for (int b = 0; b < e->B; ++b) if (s->slots[b].req && !s->slots[b].parked) { bd.run[b] = 1; *idle = false; }
    if (*idle) {
        if (bd.retired || bd.made_prefix) Q3_HIP(e, hipStreamSynchronize(e->stream));  // (the staging half is rewritten by the next admission; a PREFIX event says the store is written)
        return Q3TTS_OK;
    }
    TRY(q3_run_chunk(e, 4));
    bool more, first = false;
    { std::lock_guard<std::mutex> lk(s->mu); more = !s->pending.empty(); }
    return q3_voc_dispatch(e, bd.run.data(), bd.run.data(), s->voc_frames.data(), more, &first);
}

// 8. every running slot's new window [delivered, samples) as a gather entry and a CHUNK event; the entries (by-value kernel arguments)
// in launches of at most Q3_PCM_MAX_ENT, all into the one staging buffer; one copy to the ring, one event
int gather_pcm(q3tts_session* s, Boundary& bd) {
    q3tts_engine* e = s->e;
    hipStream_t vs = e->vstream;
    const Q3Resamp* rs = e->out_rate ? &e->rs_out : nullptr;
    std::vector<Q3PcmEnt> ents; std::vector<int> ent_len; std::vector<char> ent_fin;
    size_t tot = 0;
    std::vector<SEv> chunks;
    if (e->speed) {  // one tempo launch for all running slots in front of the gather: their tempo rows up to what their PCM decides by now
        std::vector<int> tb, tn; std::vector<char> td;
        for (int b = 0; b < e->B; ++b)
            if (bd.run[b]) { tb.push_back(b); tn.push_back(q3_voc_samples(e, b)); td.push_back(e->slots_host[b].active ? 0 : 1); }
        TRY(q3_tempo_slots(e, tb.data(), tn.data(), td.data(), (int)tb.size(), vs));
    }
    std::vector<Q3DocScan> scans; std::vector<int32_t*> resets;
    for (int b = 0; b < e->B; ++b) {
        if (!bd.run[b]) continue;
        SSlot& sl = s->slots[b];
        const bool done = !e->slots_host[b].active;
        const int ns = q3_voc_samples(e, b);
        if (sl.req->doc && sl.req->doc->ended) {  // (end_doc leaves none behind; should one exist it must not run on to max_steps)
            TRY(q3_retire_slot(e, b, vs)); free_slot(s, b);
            Q3_HIP(e, hipStreamSynchronize(e->stream));  // (the staging-half record is rewritten by the next admission)
            continue;
        }
        if (sl.req->doc) {  // a document's segment: scanned into its document row, no chunk of its own
            if (ns > (int)q3_voc_pcm_stride(e)) return q3_set_err(e, Q3TTS_ERR_STATE, "session: a chunk window exceeds the staging bound");
            doc_slot_scan(s, b, ns, done, scans, resets);
            if (done) bd.fin.push_back(b);
            continue;
        }
        const int c = q3_emit_count(e, ns, done, sl.delivered);
        if (c < 0 || tot + (size_t)std::max(c, 0) > s->ring_cap || ns > (int)q3_voc_pcm_stride(e))
            return q3_set_err(e, Q3TTS_ERR_STATE, "session: a chunk window exceeds the staging bound");
        if (c > 0 || done) {
            SEv v; v.id = sl.req->id; v.kind = Q3TTS_EV_CHUNK; v.n = c; v.is_final = done ? 1 : 0; v.off = tot;
            chunks.push_back(v);
        }
        if (c > 0) {
            ent_len.push_back((int)q3_pcm_valid(e, ns, done)); ent_fin.push_back(done ? 1 : 0);
            ents.push_back(Q3PcmEnt{b, sl.delivered, c, 0, (long long)tot});
            tot += (size_t)c; sl.delivered += c;
        }
        if (done) bd.fin.push_back(b);
    }
    const int ne = (int)ents.size(), k = s->ring_next;
    // documents: at most two launches more, no copy more (the pieces and the edge tables lie behind the plain chunks in the same buffer)
    std::vector<Q3DocPiece> pieces; std::vector<DocExit> exits; std::vector<std::shared_ptr<Doc>> finished;
    if (!s->docs.empty()) {
        for (int32_t* p : resets) {  // a segment's first boundary in its row: {INT32_MAX, -1}, by device fills in stream order in front of the scan
            Q3_HIP(e, hipMemsetD32Async((hipDeviceptr_t)p, INT32_MAX, 1, vs));
            Q3_HIP(e, hipMemsetD32Async((hipDeviceptr_t)(p + 1), -1, 1, vs));
        }
        for (size_t g0 = 0; g0 < scans.size(); g0 += Q3_DOC_MAX_ENT) {
            Q3DocScanPack sp{};
            const int n = (int)std::min<size_t>(scans.size() - g0, Q3_DOC_MAX_ENT);
            for (int i = 0; i < n; ++i) sp.e[i] = scans[g0 + i];
            q3_launch_doc_scan(sp, n, vs);
        }
        TRY(doc_emit(s, bd, &tot, pieces, exits, chunks, finished));
    }
    if (ne > 0 || !pieces.empty() || !exits.empty()) {
        const int rc = take_ring(s, k);
        if (rc) return rc;
        for (int g0 = 0; g0 < ne; g0 += Q3_PCM_MAX_ENT) {
            const int n = std::min(ne - g0, (int)Q3_PCM_MAX_ENT);
            Q3PcmPack pk{}; Q3PcmSrc src{};
            int mx = 0;
            for (int i = 0; i < n; ++i) {
                pk.e[i] = ents[g0 + i]; src.len[i] = ent_len[g0 + i]; mx = std::max(mx, ents[g0 + i].count);
                if (ent_fin[g0 + i]) src.final_mask |= 1ull << i;
            }
            if (!rs) q3_launch_pcm_pack(q3_pcm_rows(e), q3_pcm_rows_stride(e), pk, n, mx, s->fmt, s->dev, vs);
            else if (q3_launch_pcm_resample(q3_pcm_rows(e), q3_pcm_rows_stride(e), pk, src, n, mx, *rs, s->fmt, s->dev, vs) != 0)
                return q3_set_err(e, Q3TTS_ERR_UNSUPPORTED, "session: the resampler's input span does not fit the LDS");
        }
        for (size_t g0 = 0; g0 < pieces.size(); g0 += Q3_DOC_MAX_ENT) {
            Q3DocPiecePack pk{};
            const int n = (int)std::min<size_t>(pieces.size() - g0, Q3_DOC_MAX_ENT);
            for (int i = 0; i < n; ++i) pk.e[i] = pieces[g0 + i];
            q3_launch_doc_emit(pk, n, s->fmt, s->dev, vs);
        }
        for (const DocExit& x : exits) {  // a document with a rate: its outputs from its ring, behind its stretch (issued by doc_emit, in stream order)
            const Doc& d = *x.d;
            if (q3_launch_doc_resample(d.speed ? d.ring_t : d.ring_j, d.speed ? d.rg.ct : d.rg.cj, x.st.nx, x.st.fin_x != 0, x.st.first, x.st.count, d.rs, s->fmt,
                                       s->dev, (long long)x.at, vs) != 0)
                return q3_set_err(e, Q3TTS_ERR_UNSUPPORTED, "session: the resampler's input span does not fit the LDS");
        }
        for (auto& d : s->docs) if (d->touch && d->failed == Q3TTS_OK) { d->pend_ring = k; d->touch = false; }
        Q3_HIP(e, hipGetLastError());
        Q3_HIP(e, hipMemcpyAsync(s->host[k], s->dev, tot * s->es, hipMemcpyDeviceToHost, vs));
        Q3_HIP(e, hipEventRecord(s->ev[k], vs));
        s->inflight[k] = true;
        s->ring_next = (k + 1) % kRing;
        bd.bt.ring = k;
        for (SEv& v : chunks) if (v.kind == Q3TTS_EV_CHUNK && v.n > 0) v.ring = k;  // (a SEGMENT event's n is an index: it holds no reference)
    }
    for (SEv& v : chunks) bd.bt.evs.push_back(v);
    for (auto& d : finished) {  // the last segment of a closed document is out: DONE behind its last chunk, the rows freed
        q3tts_result r{};
        r.n_frames = (int32_t)d->frames; r.hit_eos = d->all_eos ? 1 : 0;
        r.n_samples = (int32_t)(d->ringed() ? d->rg.m : d->st.delivered); r.sample_rate = d->out_rate ? d->out_rate : e->cfg.vocoder.sample_rate;
        TRY(end_doc(s, bd, d, Q3TTS_EV_DONE, Q3TTS_OK, &r));
    }
    return Q3TTS_OK;
}

// 9. finished utterances: codes back on the decoder stream, the slot free from the next boundary on
int finish_slots(q3tts_session* s, Boundary& bd) {
    q3tts_engine* e = s->e;
    for (int b : bd.fin) {
        if (Doc* d = s->slots[b].req->doc) {  // a document's segment: its result waits for the SEGMENT event; the slot is free as any other
            DocSeg& g = d->segs[s->slots[b].req->seg];
            if (d->ended || d->failed != Q3TTS_OK) { q3tts_result tmp{}; TRY(q3_codes_back(e, b, &tmp)); Q3_HIP(e, hipStreamSynchronize(e->stream)); q3tts_result_free(&tmp); }
            else { TRY(q3_codes_back(e, b, &g.res)); g.res.status = Q3TTS_OK; }
            Q3_HIP(e, hipEventRecord(e->fin_ev[b], e->vstream));  // (behind the scan that read the slot's PCM)
            free_slot(s, b);
            continue;
        }
        SEv v = final_ev(s->slots[b].req->id, Q3TTS_EV_DONE, Q3TTS_OK);
        TRY(q3_codes_back(e, b, &v.res));
        v.res.n_samples = s->slots[b].delivered; v.res.sample_rate = e->out_rate ? e->out_rate : e->cfg.vocoder.sample_rate;
        Q3_HIP(e, hipEventRecord(e->fin_ev[b], e->vstream));  // (behind the gather that read the slot's PCM)
        free_slot(s, b);
        bd.bt.evs.push_back(v);
    }
    if (!bd.fin.empty()) Q3_HIP(e, hipStreamSynchronize(e->stream));
    return Q3TTS_OK;
}

// ---- documents (include/q3tts.h, "documents in a session") -------------------------------------------------------
// the table of a document's edges in the staging buffer, in samples of the session's format (2 int32 per row)
size_t doc_table_samples(const q3tts_session* s, const Doc& d) { return (size_t)d.ahead * 8 / s->es; }

// does a boundary have document work although no slot runs? (the worker does not sleep then)
bool doc_work(const q3tts_session* s) {
    for (const auto& d : s->docs) {
        if (d->failed != Q3TTS_OK || d->pend_ring >= 0 || d->clipped || d->touch || d->flow) return true;
        if (!d->w_open && d->st.head >= (long long)d->segs.size()) return true;  // its last event is due
        if (d->queued < std::min<long long>((long long)d->segs.size(), d->st.head + d->ahead)) return true;  // a segment became eligible
    }
    return false;
}

// 0. new documents: the rows of each, checked against the device's free memory first (the one boundary that allocates for a document)
int accept_docs(q3tts_session* s, Boundary& bd) {
    q3tts_engine* e = s->e;
    std::vector<std::shared_ptr<Doc>> fresh;
    if (s->docs_waiting.load(std::memory_order_acquire) == 0) return Q3TTS_OK;  // (no document: the boundary is what it was)
    {
        std::lock_guard<std::mutex> lk(s->mu);
        fresh.swap(s->docs_new);
        s->docs_waiting.store(0, std::memory_order_release);
        for (auto& d : fresh) { auto it = s->ids.find(d->id); if (it != s->ids.end()) it->second.queued = false; }
    }
    for (auto& d : fresh) {
        d->stride = ((size_t)e->cfg.max_steps_cap * q3_voc_samples_per_frame(e) + 3) & ~(size_t)3;
        const size_t rows_b = (size_t)d->ahead * d->stride * sizeof(float) + (size_t)d->ahead * 2 * sizeof(int32_t);
        size_t need = rows_b;
        int rrc = Q3TTS_OK;
        std::vector<float> aux;  // what the two kernels read beside the rings: the stretch's window and 16 bytes for its p, the resampler's table
        if (d->ringed()) {  // its rings: the minimum plus what one boundary can produce (twice one slot's share of the staging buffer)
            Q3DocRing& g = d->rg;
            g = Q3DocRing{};
            g.speed = d->speed;
            if (g.speed) { q3_tempo_window(aux); aux.resize(aux.size() + 4, 0.0f); }
            if (d->out_rate) {  // the table is the document's own (freed with it), not the engine's cache of q3tts_set_output_rate
                Q3Resamp r{};
                std::vector<float> tab;
                rrc = q3_resample_table(e->cfg.vocoder.sample_rate, d->out_rate, &r.L, &r.M, &r.H, tab);
                if (rrc != Q3TTS_OK) q3_set_err(e, rrc, "document: the resampler refuses this output rate");
                else {
                    r.rate_in = e->cfg.vocoder.sample_rate; r.rate_out = d->out_rate; r.T = 2 * r.H + 1;
                    const std::vector<float> dl = q3_resample_device_layout(tab, r.L, r.M, r.T);
                    aux.insert(aux.end(), dl.begin(), dl.end());
                    d->rs = r; g.L = r.L; g.M = r.M; g.H = r.H;
                }
            }
            const long long win = 2 * (long long)(s->ring_cap / (size_t)e->B);
            g.cj = (q3_doc_ring_min_j(g.speed, g.L, g.M, g.H) + win + 3) & ~3ll;
            g.ct = g.speed ? (q3_doc_ring_min_t(g.speed, g.L, g.M, g.H) + q3_tempo_N(win, g.speed) + Q3_TEMPO_HS + 3) & ~3ll : 0;
            need += sizeof(float) * ((size_t)(g.cj + g.ct) + aux.size());
        }
        size_t free_b = 0, total_b = 0;
        Q3_HIP(e, hipMemGetInfo(&free_b, &total_b));
        const long long cap = s->doc_mem_cap.load(std::memory_order_relaxed);
        if (cap >= 0) free_b = std::min(free_b, (size_t)cap);
        int rc = Q3TTS_OK;
        // The edge table rides the staging buffer beside the plain chunks. It is emitted only at a boundary at which one of the document's
        // segments ran, and a running segment emits no chunk of its own: its slot's share of the buffer (ring_cap / B samples) is unused
        // then. So a table that fits one slot's share always fits (doc_emit fails the document, not the session, should it ever not).
        if (doc_table_samples(s, *d) * (size_t)e->B > s->ring_cap)
            rc = q3_set_err(e, Q3TTS_ERR_INVALID, "document: the edge table of ahead = " + std::to_string(d->ahead) + " rows exceeds one slot's share of the staging buffer");
        else if (rrc != Q3TTS_OK) rc = rrc;  // (the resampler's table; submit has checked the plan, so this does not happen)
        else if (need > free_b || hipMalloc((void**)&d->rows, rows_b) != hipSuccess)
            rc = q3_set_err(e, Q3TTS_ERR_OOM, "document: its " + std::to_string(d->ahead) + " rows" + (d->ringed() ? " and rings" : "") + " need " + std::to_string(need) + " bytes, the device has " + std::to_string(free_b) + " bytes free");
        else if (d->ringed()) {
            if (hipMalloc((void**)&d->ring_j, sizeof(float) * (size_t)d->rg.cj) != hipSuccess ||
                (d->speed && hipMalloc((void**)&d->ring_t, sizeof(float) * (size_t)d->rg.ct) != hipSuccess) ||
                hipMalloc((void**)&d->aux, sizeof(float) * aux.size()) != hipSuccess ||
                hipMemcpy(d->aux, aux.data(), sizeof(float) * aux.size(), hipMemcpyHostToDevice) != hipSuccess) {
                (void)hipGetLastError();
                rc = q3_set_err(e, Q3TTS_ERR_OOM, "document: its " + std::to_string(d->ahead) + " rows and rings need " + std::to_string(need) + " bytes, the device has " + std::to_string(free_b) + " bytes free");
                d->bytes = 0; doc_free(e, *d);
            }
        }
        if (rc != Q3TTS_OK) {
            d->rows = nullptr; d->ended = true;
            std::lock_guard<std::mutex> lk(s->mu);
            d->finished = true; d->open = false;
            if (d->own_px) { d->px->released = true; maybe_reap(s, d->px); }
            bd.bt.evs.push_back(final_ev(d->id, Q3TTS_EV_FAILED, rc));
            continue;
        }
        d->edges = (int32_t*)(d->rows + (size_t)d->ahead * d->stride);
        if (d->out_rate) d->rs.tab = d->aux + (d->speed ? Q3_TEMPO_WN + 4 : 0);  // (16-byte aligned behind the window and the p)
        d->bytes = need; e->dev_bytes += need;  // (q3tts_k_device_bytes sees a document's rows while they live)
        d->accepted = true;
        s->docs.push_back(d);
    }
    return Q3TTS_OK;
}

// (mu held, collect) appended segments reach the worker, and every segment j < head + ahead that is not queued yet joins the FIFO as an
// internal request behind the document's prefix
void feed_docs(q3tts_session* s) {
    q3tts_engine* e = s->e;
    s->doc_dirty = false;
    for (auto& dp : s->docs) {
        Doc& d = *dp;
        for (DocSeg& g : d.incoming) { d.segs.push_back(std::move(g)); d.snap.push_back(Q3DocSegNow{0, INT32_MAX, -1, 0, d.segs.back().kind}); }
        d.incoming.clear();
        d.w_open = d.open;
        if (d.failed != Q3TTS_OK) continue;
        const long long lim = std::min<long long>((long long)d.segs.size(), d.st.head + d.ahead);
        for (; d.queued < lim; ++d.queued) {
            const DocSeg& g = d.segs[d.queued];
            std::unique_ptr<SReq> q(new SReq());
            q->id = (1ull << 63) | s->next_internal++;
            q->doc = &d; q->seg = d.queued;
            q->text = g.ids;
            q->desc.text_ids = q->text.data(); q->desc.n_text = (int32_t)q->text.size(); q->desc.lang_id = -1; q->desc.spk_id = -1;
            q->r = d.tmpl;
            q->r.prompt = &q->desc; q->r.prompt_embd = nullptr; q->r.prefix = d.px; q->r.want_pcm = 1; q->r.text_stream = 0; q->r.text_open = 0;
            if (g.max_steps) q->r.max_steps = g.max_steps;
            if (d.tmpl.has_seed) q->r.seed = d.tmpl.seed + (uint64_t)d.queued;
            if (d.px->e == e) ++d.px->qrefs;
            s->pending.push_back(std::move(q));
        }
    }
}

// a document leaves: its slots are retired, its queued entries dropped, its rows freed (hipFree waits for the launches that read them), its
// own prefix released; `kind` is its final event. The caller has made sure no launch of this boundary still needs to be issued for it.
int end_doc(q3tts_session* s, Boundary& bd, const std::shared_ptr<Doc>& dp, int kind, int status, const q3tts_result* res) {
    q3tts_engine* e = s->e;
    Doc& d = *dp;
    for (int b = 0; b < e->B; ++b)
        if (s->slots[b].req && s->slots[b].req->doc == &d) {
            TRY(q3_retire_slot(e, b, e->vstream)); free_slot(s, b);
            bd.cool[b] = 1; bd.retired = true;
        }
    {
        std::lock_guard<std::mutex> lk(s->mu);
        for (auto p = s->pending.begin(); p != s->pending.end();) {
            if ((*p)->doc != &d || (*p)->kind != 0) { ++p; continue; }
            unref_prefix(s, (*p)->r.prefix);
            p = s->pending.erase(p);
        }
        d.finished = true; d.open = false;
        if (d.own_px && !d.px->released) { d.px->released = true; maybe_reap(s, d.px); }
    }
    // ... and its segments that collect popped at this very boundary (a cancel and the pop share one hold of mu): they would be admitted
    // into slots behind the rows' free. Their prefix reference went with the pop; cr_adm and tn_adm stay aligned with adm.
    for (size_t i = bd.adm.size(); i-- > 0;)
        if (bd.adm[i] && bd.adm[i]->doc == &d && bd.adm[i]->kind == 0) {  // (null: plan_and_admit moved it into its slot — end_doc from gather_pcm)
            bd.adm.erase(bd.adm.begin() + i); bd.cr_adm.erase(bd.cr_adm.begin() + i);
            if (i < bd.tn_adm.size()) bd.tn_adm.erase(bd.tn_adm.begin() + i);
        }
    Q3_HIP(e, doc_free(e, d));  // (hipFree waits for the launches that read the rows and rings)
    for (DocSeg& g : d.segs) copy_result_free(g.res);
    d.ended = true; d.pend_ring = -1; d.touch = d.clipped = d.flow = false; d.due.clear();
    SEv v = final_ev(d.id, kind, status);
    if (res) { v.res = *res; v.res.status = status; }
    bd.bt.evs.push_back(v);
    s->docs.erase(std::remove(s->docs.begin(), s->docs.end(), dp), s->docs.end());
    return Q3TTS_OK;
}

// a document's device memory goes: its rows, its rings and their window (the caller knows that no launch reads them any more)
hipError_t doc_free(q3tts_engine* e, Doc& d) {
    hipError_t first = hipSuccess;
    for (float* p : {d.rows, d.ring_j, d.ring_t, d.aux})
        if (p) { const hipError_t r = hipFree(p); if (first == hipSuccess) first = r; }
    e->dev_bytes -= d.bytes; d.bytes = 0;
    d.rows = d.ring_j = d.ring_t = d.aux = nullptr; d.edges = nullptr;
    return first;  // (the first failure, as the one hipFree of the rows reported it)
}

// 3a. documents that were cancelled, or that failed at the last boundary (a segment failed by itself, the length limit): torn down here,
// where slots are retired anyway
int drop_docs(q3tts_session* s, Boundary& bd) {
    for (size_t i = 0; i < s->docs.size();) {
        std::shared_ptr<Doc> d = s->docs[i];
        const bool cancelled = std::find(bd.cancels.begin(), bd.cancels.end(), d->id) != bd.cancels.end();
        if (!cancelled && d->failed == Q3TTS_OK) { ++i; continue; }
        TRY(end_doc(s, bd, d, cancelled ? Q3TTS_EV_CANCELLED : Q3TTS_EV_FAILED, cancelled ? Q3TTS_OK : d->failed, nullptr));
    }
    return Q3TTS_OK;
}

// a running document slot at gather time: no CHUNK of its own; its new samples become a scan entry into the segment's document row
void doc_slot_scan(q3tts_session* s, int b, int ns, bool done, std::vector<Q3DocScan>& scans, std::vector<int32_t*>& resets) {
    q3tts_engine* e = s->e;
    SSlot& sl = s->slots[b];
    Doc& d = *sl.req->doc;
    DocSeg& g = d.segs[sl.req->seg];
    if (d.failed != Q3TTS_OK || d.ended || !d.rows) return;  // (nothing is scanned for a document on its way out)
    const int row = sl.req->seg % d.ahead;
    if (g.fresh) { resets.push_back(d.edges + 2 * row); g.fresh = false; }
    if (ns > g.n) {
        scans.push_back(Q3DocScan{q3_pcm_rows(e) + (size_t)b * q3_pcm_rows_stride(e), d.rows + (size_t)row * d.stride, d.edges + 2 * row, g.n, ns, d.join.threshold, 0});
        g.n = ns; d.touch = true;
    }
    if (done) { g.ended = true; d.touch = true; }
    sl.delivered = ns;
}

// 8a. the documents' part of a boundary. Per document: the snapshot of the last boundary lands (its table rode that boundary's copy;
// its event is waited for, which a whole chunk of frame steps later costs nothing), q3_doc_plan turns it into pieces clipped to what
// the staging buffer has left behind the plain requests' chunks and the tables, and the pieces, with this boundary's tables, become
// entries of ONE k_doc_emit launch (per 64 entries). *cur: the staging samples used so far, in and out.
int doc_emit(q3tts_session* s, Boundary& bd, size_t* cur, std::vector<Q3DocPiece>& ents, std::vector<DocExit>& exits, std::vector<SEv>& evs,
             std::vector<std::shared_ptr<Doc>>& finished) {
    q3tts_engine* e = s->e;
    const int rate = e->cfg.vocoder.sample_rate;
    // the last boundary's snapshots land first (pend_off still names THAT boundary's table: the plain chunks in front of it differ in size)
    for (auto& dp : s->docs) {
        Doc& d = *dp;
        if (d.failed != Q3TTS_OK || d.pend_ring < 0) continue;
        const hipError_t q = hipEventSynchronize(s->ev[d.pend_ring]);
        if (q != hipSuccess) return q3_set_err(e, Q3TTS_ERR_DEVICE, std::string("session: a document's table: ") + hipGetErrorString(q));
        const int32_t* tab = (const int32_t*)((const char*)s->host[d.pend_ring] + d.pend_off);
        for (const Doc::Pend& p : d.pend) {
            const int row = p.seg % d.ahead;
            d.snap[p.seg] = Q3DocSegNow{p.n, tab[2 * row], tab[2 * row + 1], p.ended ? 1 : 0, d.segs[p.seg].kind};
        }
        d.pend_ring = -1; d.pend.clear();
    }
    // this boundary's tables: 4-byte aligned, directly behind the plain chunks
    for (auto& dp : s->docs) {
        Doc& d = *dp;
        if (d.failed != Q3TTS_OK || !d.touch) continue;
        const size_t at = *cur + (s->es == 2 ? (*cur & 1) : 0);
        if (at + doc_table_samples(s, d) > s->ring_cap) {  // (accept_docs states why this does not happen; the document fails, the session goes on)
            q3_set_err(e, Q3TTS_ERR_STATE, "document: its edge table exceeds the staging bound");
            d.failed = Q3TTS_ERR_STATE;
            continue;
        }
        *cur = at;
        ents.push_back(Q3DocPiece{(const float*)d.edges, 0, 0, (long long)(*cur * s->es), 2 * d.ahead, -1});
        d.pend_off = *cur * s->es;
        *cur += doc_table_samples(s, d);
    }
    for (auto& dp : s->docs) {
        Doc& d = *dp;
        if (d.failed != Q3TTS_OK) continue;
        std::vector<Q3DocOut> pc; std::vector<Q3DocDone> dn;
        const long long room = d.ringed() ? q3_doc_ring_room(d.rg) : (long long)(s->ring_cap - *cur);
        const int prc = q3_doc_plan(d.join, rate, d.snap.data(), (int)d.snap.size(), room, &d.st, &pc, &dn);
        if (prc != Q3TTS_OK) {
            q3_set_err(e, prc, "document: the delivered length would pass 2^28 samples at segment " + std::to_string(d.st.head));
            d.failed = prc;
            continue;
        }
        const size_t c0 = *cur;
        bool last = false;
        long long delivered = 0;
        std::vector<Q3DocDone> pub;  // the segments to publish at this boundary
        if (d.ringed()) {  // its own speed or rate: the pieces go into RJ, the stretch and the exit run behind them (the pipeline)
            Q3DocRing& g = d.rg;
            std::vector<Q3DocPiece> je;
            long long pos = g.nj;
            if (q3_doc_out_pos(d.st.delivered, g.speed, g.L, g.M) > 0x7fffffffll) {  // (the counts of the events are int32)
                q3_set_err(e, Q3TTS_ERR_INVALID, "document: the delivered length would pass 2^31 - 1 output samples at segment " + std::to_string(d.st.head));
                d.failed = Q3TTS_ERR_INVALID;
                continue;
            }
            for (const Q3DocOut& p : pc) {
                q3_doc_ring_put(p, p.seg < 0 ? nullptr : d.rows + (size_t)(p.seg % d.ahead) * d.stride + p.src, pos, g.cj, &je);
                pos += p.count;
            }
            q3_launch_doc_emit_all(je, 0, d.ring_j, e->vstream);
            const bool fin_j = !d.w_open && d.st.head >= (long long)d.segs.size();
            DocExit x{&d, Q3DocRingStep{}, *cur};
            q3_doc_ring_step(&g, pos - g.nj, fin_j, (long long)(s->ring_cap - *cur), &x.st);
            if (g.speed)
                q3_launch_doc_tempo(d.ring_j, g.cj, d.ring_t, g.ct, (long long*)(d.aux + Q3_TEMPO_WN), d.aux, g.speed, g.nj, x.st.k_from, x.st.k_to, x.st.nt, nullptr, 0, e->vstream);
            if (x.st.count > 0) {
                if (g.L) exits.push_back(x);
                else q3_doc_ring_get(d.ring_t, g.ct, x.st.first, x.st.count, (long long)*cur, &ents);
                *cur += (size_t)x.st.count;
            }
            last = x.st.all_out != 0;
            // awake while the document is not out and a stage moved, or decidable work is left that only RT's space or the staging room held back
            d.flow = !last && (!pc.empty() || x.st.k_to > x.st.k_from || x.st.count > 0 || x.st.pending);
            for (const Q3DocDone& y : dn) d.due.push_back(y);
            size_t nd = 0;  // the segments whose last output went out with this chunk
            while (nd < d.due.size() && q3_doc_out_pos(d.due[nd].end, g.speed, g.L, g.M) <= g.m) ++nd;
            pub.assign(d.due.begin(), d.due.begin() + (long)nd);
            d.due.erase(d.due.begin(), d.due.begin() + (long)nd);
            delivered = g.m;
        } else {
            for (const Q3DocOut& p : pc) {
                const float* from = p.seg < 0 ? nullptr : d.rows + (size_t)(p.seg % d.ahead) * d.stride + p.src;
                ents.push_back(Q3DocPiece{from, p.j0, p.L, (long long)*cur, (int32_t)p.count, p.F});
                *cur += (size_t)p.count;
            }
            d.clipped = *cur >= s->ring_cap && d.st.head < (long long)d.segs.size();
            last = !d.w_open && d.st.head >= (long long)d.segs.size();
            pub = dn; delivered = d.st.delivered;
        }
        // what both kinds of document publish: the chunk, then the segments that are wholly out, positions through the document's maps
        // (the identity without a speed or rate)
        const Q3DocRing& g = d.rg;
        if (*cur > c0 || last) {
            SEv v; v.id = d.id; v.kind = Q3TTS_EV_CHUNK; v.n = (int)(*cur - c0); v.is_final = last ? 1 : 0; v.off = c0;
            evs.push_back(v);
        }
        {
            std::lock_guard<std::mutex> lk(s->mu);
            d.n_delivered = delivered;
            for (const Q3DocDone& x : pub) {
                const DocSeg& sg = d.segs[x.seg];
                q3tts_long_info f{};
                f.status = sg.res.status; f.n_frames = sg.res.n_frames; f.hit_eos = sg.res.hit_eos; f.n_native = sg.n;
                f.lo = x.lo; f.hi = x.hi; f.begin = x.begin; f.end = x.end;
                f.out_begin = q3_doc_out_pos(x.begin, g.speed, g.L, g.M); f.out_end = q3_doc_out_pos(x.end, g.speed, g.L, g.M);
                d.info.push_back(f);
            }
        }
        for (const Q3DocDone& x : pub) {
            DocSeg& sg = d.segs[x.seg];
            SEv v; v.id = d.id; v.kind = Q3TTS_EV_SEGMENT; v.n = x.seg; v.res = sg.res;
            v.res.n_samples = (int32_t)(q3_doc_out_pos(x.end, g.speed, g.L, g.M) - q3_doc_out_pos(x.begin, g.speed, g.L, g.M));
            v.res.sample_rate = d.out_rate ? d.out_rate : rate;
            sg.res = q3tts_result{};  // (the codes went with the event)
            d.frames += v.res.n_frames; d.all_eos = d.all_eos && v.res.hit_eos;
            evs.push_back(v);
        }
        if (last) finished.push_back(dp);
    }
    // this boundary's snapshots: on their way with this boundary's copy
    for (auto& dp : s->docs) {
        Doc& d = *dp;
        if (d.failed != Q3TTS_OK || !d.touch) continue;
        d.pend.clear();
        for (long long j = d.st.head; j < std::min<long long>((long long)d.segs.size(), d.st.head + d.ahead); ++j)
            if (!d.segs[j].fresh) d.pend.push_back(Doc::Pend{(int)j, d.segs[j].n, d.segs[j].ended});
    }
    return Q3TTS_OK;
}

// one chunk boundary: the phases in their order, over one Boundary
int step(q3tts_session* s) {
    Boundary bd(s->e->B);
    bool idle = false;
    ++s->seq;
    TRY(accept_docs(s, bd));
    collect(s, bd);
    TRY(voice_work(s, bd));
    TRY(cancel_slots(s, bd));
    TRY(drop_docs(s, bd));
    TRY(park_starved(s, bd));
    if (s->swap) {  // (the two phases' host time, for q3tts_k_swap_phase_ms)
        const long long o0 = s->st_out.load(std::memory_order_relaxed), i0 = s->st_in.load(std::memory_order_relaxed);
        const double t0 = q3_now_ms();
        TRY(swap_out(s, bd));
        const double t1 = q3_now_ms();
        TRY(swap_in(s, bd));
        const double t2 = q3_now_ms();
        if (s->st_out.load(std::memory_order_relaxed) != o0 || s->st_in.load(std::memory_order_relaxed) != i0) {
            s->st_out_us.fetch_add((long long)((t1 - t0) * 1e3), std::memory_order_relaxed);
            s->st_in_us.fetch_add((long long)((t2 - t1) * 1e3), std::memory_order_relaxed);
            s->st_bounds.fetch_add(1, std::memory_order_relaxed);
        }
    }
    TRY(plan_and_admit(s, bd));
    TRY(resume_and_feed(s, bd));
    TRY(run_frames(s, bd, &idle));
    if (!idle || doc_work(s)) { TRY(gather_pcm(s, bd)); TRY(finish_slots(s, bd)); }  // (a document may emit while no slot runs)
    if (!idle || !bd.bt.evs.empty() || bd.bt.ring >= 0) s->flight.push_back(std::move(bd.bt));
    return Q3TTS_OK;
}

// the worker failed: every open request gets FAILED with the status; the session refuses new submissions
void fail_all(q3tts_session* s, int rc) {
    std::string m;
    { std::lock_guard<std::mutex> lk(s->e->err_mu); m = s->e->err; }
    std::lock_guard<std::mutex> lk(s->mu);
    s->dead = true; s->worker_rc = rc; s->err = "session worker: " + m;
    for (Batch& b : s->flight) for (SEv& v : b.evs) copy_result_free(v.res);
    s->flight.clear();
    for (auto& q : s->pending) { if (q->kind == 0) unref_prefix(s, q->r.prefix); fail_keep(s, q->keep, rc); }
    s->pending.clear();
    const double t = q3_now_ms();
    for (auto& kv : s->ids)
        if (!kv.second.final_ready) {
            SEv v = final_ev(kv.first, Q3TTS_EV_FAILED, rc);
            deliver(s, v, t);
        }
    s->cv_ev.notify_all();
}

void worker(q3tts_session* s) {
    q3tts_engine* e = s->e;
    int rc = hipSetDevice(e->cfg.device) == hipSuccess ? Q3TTS_OK : q3_set_err(e, Q3TTS_ERR_DEVICE, "session: hipSetDevice");
    while (rc == Q3TTS_OK) {
        bool running = false, room = false;  // running: a slot takes frame steps (parked slots wait for text or credit); room: a slot is free
        bool evictable = false, out_ready = false;  // swapping: a parked slot could leave; a swapped-out request's rule holds again
        if (!s->limbo.empty()) {  // about to go idle with blocks in limbo: their moves are waited for, so that a full arena cannot keep the worker asleep
            bool busy = !s->flight.empty();
            for (const SSlot& sl : s->slots) busy |= sl.req && !sl.parked;
            if (!busy) { hipStreamSynchronize(e->stream); hipStreamSynchronize(e->vstream); }
            reap_blocks(s);
        }
        for (const SSlot& sl : s->slots) { if (sl.req && !sl.parked) running = true; if (!sl.req) room = true; if (sl.req && sl.parked && s->swap && !s->evict_stuck) evictable = true; }
        for (const Swapped& o : s->out) if (o.ready_at) out_ready = true;
        if (doc_work(s)) running = true;  // (undelivered audio, a segment to queue, a document to end)
        bool work;
        {
            std::unique_lock<std::mutex> lk(s->mu);
            auto todo = [&] { return ((room || evictable) && (!s->pending.empty() || out_ready)) || !s->cancels.empty() || s->text_dirty || s->grant_dirty || !s->clones.empty() || !s->trash.empty() || s->doc_dirty; };
            if (!running && s->flight.empty())  // idle: sleep until a submission that fits, a cancel, new text or close
                s->cv_work.wait(lk, [&] { return s->stop || todo(); });
            if (s->stop) break;
            work = todo();
        }
        if (!running && !work) { rc = publish(s, true); continue; }  // only copies in flight: wait for the oldest
        rc = step(s);
        if (rc == Q3TTS_OK) rc = publish(s, false);
    }
    if (rc == kStopping) rc = Q3TTS_OK;
    if (rc != Q3TTS_OK) fail_all(s, rc);
    // close (or failure): retire the slots still decoding, so the engine is usable as before
    for (int b = 0; b < e->B; ++b) if (s->slots[b].req) { q3_retire_slot(e, b, e->vstream); free_slot(s, b); }
    hipStreamSynchronize(e->stream);
    hipStreamSynchronize(e->vstream);
    for (auto& d : s->docs) { doc_free(e, *d); for (DocSeg& g : d->segs) copy_result_free(g.res); }  // (both streams are idle)
    s->docs.clear();
    for (Swapped& o : s->out) drop_block(s, o, o.ticket);  // (their ids got FAILED above, or the session is closing)
    s->out.clear();
    reap_blocks(s);  // (every move is over)
    // voice work nobody will run any more: queued jobs' and keep-voice requests' prefixes read failed, waiting clone callers wake
    {
        std::lock_guard<std::mutex> lk(s->mu);
        for (q3tts_prefix* x : std::vector<q3tts_prefix*>(s->made)) fail_keep(s, x, rc != Q3TTS_OK ? rc : Q3TTS_ERR_STATE);  // (whatever is still pending)
        for (CloneJob* j : s->clones) { j->rc = Q3TTS_ERR_STATE; j->err = "clone: the session is closing, or its worker failed"; j->done = true; }
        s->clones.clear();
        s->dead = s->dead || !s->stop;
    }
    s->cv_clone.notify_all();
}

int copy_request(q3tts_engine* e, const q3tts_request* req, SReq* q) {
    const q3tts_model_config& m = e->cfg.model;
    q->r = *req;
    q->r.want_pcm = 1;
    q->r.prompt_embd = nullptr; q->r.prompt = nullptr;
    if (req->prompt_embd) {
        if (req->n_tok <= 0 || req->n_tok > e->cfg.n_ctx) return Q3TTS_ERR_INVALID;
        q->embd.assign(req->prompt_embd, req->prompt_embd + (size_t)req->n_tok * m.d_embed);
        q->r.prompt_embd = q->embd.data();
    } else if (req->prompt) {
        const q3tts_prompt_desc& p = *req->prompt;
        auto bad = [](const void* ptr, int32_t n) { return n < 0 || (n > 0 && !ptr); };
        if (bad(p.text_ids, p.n_text) || bad(p.instruct_ids, p.n_instruct) || bad(p.ref_codes, p.n_ref_frames) || bad(p.ref_text_ids, p.n_ref_text))
            return Q3TTS_ERR_INVALID;
        q->desc = p;
        q->text.assign(p.text_ids, p.text_ids + p.n_text);
        q->desc.text_ids = q->text.data();
        if (p.instruct_ids) { q->instr.assign(p.instruct_ids, p.instruct_ids + p.n_instruct); q->instr.push_back(0); q->desc.instruct_ids = q->instr.data(); }
        if (p.spk_emb) { q->spk.assign(p.spk_emb, p.spk_emb + m.d_embed); q->desc.spk_emb = q->spk.data(); }
        if (p.ref_codes) {
            q->ref_codes.assign(p.ref_codes, p.ref_codes + (size_t)p.n_ref_frames * 16); q->ref_codes.push_back(0); q->desc.ref_codes = q->ref_codes.data();
            q->ref_text.assign(p.ref_text_ids ? p.ref_text_ids : nullptr, p.ref_text_ids ? p.ref_text_ids + p.n_ref_text : nullptr);
            q->ref_text.push_back(0);
            q->desc.ref_text_ids = q->ref_text.data();
        } else {
            q->desc.ref_text_ids = nullptr; q->desc.n_ref_text = 0;
        }
        q->r.prompt = &q->desc;
    }
    return Q3TTS_OK;
}

}  // namespace

extern "C" int q3tts_session_create(q3tts_engine* e, int32_t pcm_format, q3tts_session** out) {
    if (!e || !out) return q3_set_err(e, Q3TTS_ERR_INVALID, "null argument");
    if (pcm_format != Q3TTS_PCM_F32 && pcm_format != Q3TTS_PCM_I16) return q3_set_err(e, Q3TTS_ERR_INVALID, "pcm_format must be 0 (f32) or 1 (i16)");
    Q3_NOT_IN_SESSION(e);
    if (!e->voc) return q3_set_err(e, Q3TTS_ERR_STATE, "a session needs with_vocoder = 1");
    Q3_HIP(e, hipSetDevice(e->cfg.device));
    Q3_HIP(e, hipStreamSynchronize(e->stream));
    Q3_HIP(e, hipStreamSynchronize(e->vstream));
    std::unique_ptr<q3tts_session> s(new q3tts_session());
    s->e = e; s->fmt = pcm_format; s->es = pcm_format ? 2 : 4;
    s->ring_cap = (size_t)e->B * (4 + std::max(0, e->cfg.vocoder.lookahead_frames)) * q3_voc_samples_per_frame(e);
    if (e->speed) {  // a boundary's window stretched (twice the samples at 500 per mille), plus the hold-back and the frames a final chunk releases
        const size_t per = (size_t)q3_tempo_N((long long)(s->ring_cap / e->B) + Q3_TEMPO_HOLD + 2 * Q3_TEMPO_HS, e->speed) + 2 * Q3_TEMPO_HS;
        s->ring_cap = std::max(s->ring_cap, (size_t)e->B * per);
    }
    if (e->out_rate) {  // the larger of the two rates: a boundary's window at the output rate, plus the H input samples a final chunk releases
        const Q3Resamp& r = e->rs_out;
        const size_t per = (size_t)q3_resample_N((long long)(s->ring_cap / e->B) + r.H, r.L, r.M) + 2;
        s->ring_cap = std::max(s->ring_cap, (size_t)e->B * per);
    }
    auto release = [&]() {
        for (int k = 0; k < kRing; ++k) { if (s->host[k]) hipHostFree(s->host[k]); if (s->ev[k]) hipEventDestroy(s->ev[k]); }
        if (s->dev) hipFree(s->dev);
    };
    for (int k = 0; k < kRing; ++k) {
        if (hipHostMalloc(&s->host[k], s->ring_cap * s->es, hipHostMallocDefault) != hipSuccess ||
            hipEventCreateWithFlags(&s->ev[k], hipEventDisableTiming) != hipSuccess) { release(); return q3_set_err(e, Q3TTS_ERR_OOM, "session: pinned staging"); }
    }
    if (hipMalloc(&s->dev, s->ring_cap * s->es) != hipSuccess) { release(); return q3_set_err(e, Q3TTS_ERR_OOM, "session: device staging"); }
    s->slots.resize(e->B);
    s->voc_frames.assign(e->B, 0);
    q3tts_session* raw = s.release();
    e->session.store(raw);
    raw->th = std::thread(worker, raw);
    *out = raw;
    return Q3TTS_OK;
}

// q3tts_session_submit, and with out != null q3tts_session_submit_keep_voice: *out receives a pending prefix the request's admission fills
// credit > 0: q3tts_session_submit_paced
static int submit_request(q3tts_session* s, const q3tts_request* req, uint64_t* id, int32_t voice_rows, q3tts_prefix** out, int32_t credit = 0) {
    if (!s || !req || !id) return serr(nullptr, Q3TTS_ERR_INVALID, "null argument");
    if (out) *out = nullptr;
    const char* why = "";
    if (q3_request_rules(req, out != nullptr, voice_rows, &why) != Q3TTS_OK) { std::lock_guard<std::mutex> lk(s->mu); return serr(s, Q3TTS_ERR_INVALID, std::string("submit: ") + why); }
    std::unique_ptr<SReq> q(new SReq());
    if (copy_request(s->e, req, q.get()) != Q3TTS_OK) {
        std::lock_guard<std::mutex> lk(s->mu);
        return serr(s, Q3TTS_ERR_INVALID, "submit: the request's prompt cannot be copied (n_tok outside 1..n_ctx or a null array with a length)");
    }
    {
        std::lock_guard<std::mutex> lk(s->mu);
        if (s->stop || s->dead) return serr(s, Q3TTS_ERR_STATE, s->dead ? "submit: the session's worker failed" : "submit: the session is closing");
        if (q3tts_prefix* x = const_cast<q3tts_prefix*>(req->prefix)) {
            if (x->e == s->e) {
                if (x->released) return serr(s, Q3TTS_ERR_INVALID, "submit: the prefix was released");
                ++x->qrefs;
            }
        }
        if (out) {
            q->keep = new q3tts_prefix();
            q->keep->e = s->e; q->keep->state.store(0);
            q->voice_rows = voice_rows;
            s->made.push_back(q->keep);
            *out = q->keep;
        }
        q->id = s->next_id++;
        IdState st; st.t_submit = q3_now_ms();
        if (q->r.text_stream == 1) { st.ts = true; st.closed = !(q->r.text_open == 1); q3_text_trailing(&q->r, st.T); }
        if (credit > 0) { st.paced = true; st.credit = credit; }
        s->ids[q->id] = st;
        *id = q->id;
        s->pending.push_back(std::move(q));
    }
    s->cv_work.notify_one();
    return Q3TTS_OK;
}

// ---- paced requests and swapping (include/q3tts.h) ----
extern "C" int q3tts_k_credit_ready(int64_t credit, int32_t n_frames) { return (credit < 0 || (long long)n_frames + 4 <= credit) ? 1 : 0; }

extern "C" int q3tts_session_submit_paced(q3tts_session* s, const q3tts_request* req, int32_t credit_frames, uint64_t* id) {
    if (!s) return serr(nullptr, Q3TTS_ERR_INVALID, "null session");
    if (credit_frames < 4) { std::lock_guard<std::mutex> lk(s->mu); return serr(s, Q3TTS_ERR_INVALID, "submit_paced: credit_frames >= 4 (a request takes its frames four at a time)"); }
    return submit_request(s, req, id, 0, nullptr, credit_frames);
}

extern "C" int q3tts_session_grant(q3tts_session* s, uint64_t id, int32_t frames) {
    if (!s) return serr(nullptr, Q3TTS_ERR_INVALID, "null session");
    {
        std::lock_guard<std::mutex> lk(s->mu);
        if (frames == 0) return serr(s, Q3TTS_ERR_INVALID, "grant: frames is 0 (> 0 adds to the credit, < 0 lifts the limit)");
        auto it = s->ids.find(id);
        if (it == s->ids.end() || it->second.final_ready || it->second.cancelled) return serr(s, Q3TTS_ERR_INVALID, "grant: unknown id, or the request has finished");
        IdState& st = it->second;
        if (!st.paced) return serr(s, Q3TTS_ERR_INVALID, "grant: the request was not submitted paced");
        if (frames < 0) st.credit = kNoLimit;
        else if (st.credit != kNoLimit) st.credit += frames;
        s->grant_dirty = true;
    }
    s->cv_work.notify_one();
    return Q3TTS_OK;
}

extern "C" int q3tts_session_set_swap(q3tts_session* s, int64_t arena_bytes) {
    if (!s) return serr(nullptr, Q3TTS_ERR_INVALID, "null session");
    std::lock_guard<std::mutex> lk(s->mu);  // (the worker is idle: nothing was submitted)
    if (s->next_id != 1) return serr(s, Q3TTS_ERR_STATE, "set_swap: valid before the first submission only");
    if (s->stop || s->dead) return serr(s, Q3TTS_ERR_STATE, "set_swap: the session is closing, or its worker failed");
    if (arena_bytes < 0) return serr(s, Q3TTS_ERR_INVALID, "set_swap: arena_bytes is negative (0 turns swapping off)");
    q3tts_engine* e = s->e;
    if (Q3Swap* old = s->swap.exchange(nullptr)) q3_swap_destroy(e, old);
    if (arena_bytes == 0) return Q3TTS_OK;
    Q3Swap* sw = nullptr;
    const int rc = q3_swap_create(e, arena_bytes, &sw);
    s->swap = sw;
    if (rc != Q3TTS_OK) { std::string m; { std::lock_guard<std::mutex> el(e->err_mu); m = e->err; } return serr(s, rc, m); }
    return Q3TTS_OK;
}

extern "C" int q3tts_session_swap_stats(const q3tts_session* s, int64_t out[6]) {
    if (!s) return serr(nullptr, Q3TTS_ERR_INVALID, "null session");
    if (!out) return serr(nullptr, Q3TTS_ERR_INVALID, "null argument");
    out[0] = s->st_out.load(std::memory_order_relaxed); out[1] = s->st_in.load(std::memory_order_relaxed); out[2] = s->st_moved.load(std::memory_order_relaxed);
    out[3] = s->st_used.load(std::memory_order_relaxed); out[4] = s->st_peak.load(std::memory_order_relaxed); out[5] = s->st_skipped.load(std::memory_order_relaxed);
    return Q3TTS_OK;
}

extern "C" int q3tts_k_swap_phase_ms(const q3tts_session* s, double out[3]) {
    if (!s) return serr(nullptr, Q3TTS_ERR_INVALID, "null session");
    if (!out) return serr(nullptr, Q3TTS_ERR_INVALID, "null argument");
    out[0] = s->st_out_us.load(std::memory_order_relaxed) * 1e-3; out[1] = s->st_in_us.load(std::memory_order_relaxed) * 1e-3;
    out[2] = (double)s->st_bounds.load(std::memory_order_relaxed);
    return Q3TTS_OK;
}

extern "C" int q3tts_session_submit(q3tts_session* s, const q3tts_request* req, uint64_t* id) { return submit_request(s, req, id, 0, nullptr); }

// ---- documents in a session (include/q3tts.h) ----
static int doc_segments(const q3tts_long_segment* segs, int32_t n, std::vector<DocSeg>& out, const char** why) {
    for (int i = 0; i < n; ++i) {
        if (segs[i].n_ids < 0 || (segs[i].n_ids > 0 && !segs[i].ids) || segs[i].max_steps < 0) { *why = "a segment's ids are null or a count is negative"; return Q3TTS_ERR_INVALID; }
        DocSeg g;
        g.ids.assign(segs[i].ids, segs[i].ids + segs[i].n_ids); g.kind = segs[i].kind; g.max_steps = segs[i].max_steps;
        out.push_back(std::move(g));
    }
    return Q3TTS_OK;
}

extern "C" int q3tts_session_submit_document(q3tts_session* s, const q3tts_request* tmpl, const q3tts_prompt_desc* voice, q3tts_prefix* prefix,
                                             const q3tts_long_segment* segs, int32_t n_segs, const q3tts_doc_opts* opts, uint64_t* id) {
    if (!s || !tmpl || !id || (n_segs > 0 && !segs)) return serr(nullptr, Q3TTS_ERR_INVALID, "null argument");
    auto refuse = [&](int code, const std::string& m) { std::lock_guard<std::mutex> lk(s->mu); return serr(s, code, m); };
    q3tts_engine* e = s->e;
    q3tts_doc_opts o;
    if (opts) o = *opts; else q3tts_doc_default_opts(&o);
    std::vector<int32_t> kinds;
    for (int i = 0; i < n_segs && i < Q3_JOIN_MAX_SEG + 1; ++i) kinds.push_back(segs[i].kind);
    const char* why = "";
    const int rrc = q3_doc_rules(o, kinds.data(), n_segs, voice != nullptr, prefix != nullptr, e->speed, e->out_rate, &why);
    if (rrc != Q3TTS_OK) return refuse(rrc, why);
    if (tmpl->text_stream == 1 || tmpl->prompt_embd || tmpl->prompt || tmpl->prefix)
        return refuse(Q3TTS_ERR_INVALID, "document: the template carries no prompt (prompt_embd, prompt, prefix NULL; text_stream off)");
    if (voice && (voice->n_text != 0 || q3_voice_job_rules(voice, nullptr, 0, &why) != Q3TTS_OK))
        return refuse(Q3TTS_ERR_INVALID, std::string("document: voice is a voice-only desc (n_text == 0)") + (*why ? std::string(": ") + why : std::string()));
    if (prefix && prefix->e != e) return refuse(Q3TTS_ERR_INVALID, "document: the prefix was made by another engine");
    std::shared_ptr<Doc> d(new Doc());
    if (doc_segments(segs, n_segs, d->incoming, &why) != Q3TTS_OK) return refuse(Q3TTS_ERR_INVALID, std::string("document: ") + why);
    d->tmpl = *tmpl;
    d->tmpl.prompt = nullptr; d->tmpl.prompt_embd = nullptr; d->tmpl.prefix = nullptr; d->tmpl.want_pcm = 1;
    if (d->tmpl.use_engine_sampler == 1) {
        d->tmpl.use_engine_sampler = 0;
        d->tmpl.temperature = e->temperature; d->tmpl.top_k = e->top_k; d->tmpl.top_p = e->top_p; d->tmpl.has_seed = e->has_seed; d->tmpl.seed = e->seed;
    }
    d->join = o.join; d->ahead = o.ahead ? o.ahead : 8; d->open = o.open == 1; d->n_given = n_segs;
    d->speed = o.speed_permille == 1000 ? 0 : o.speed_permille;
    d->out_rate = o.output_rate == e->cfg.vocoder.sample_rate ? 0 : o.output_rate;
    if (d->out_rate) {  // (host only: the table itself is made by the worker at the boundary that accepts the document)
        int L = 0, M = 0, H = 0, T = 0;
        const int prc = q3_resample_plan(e->cfg.vocoder.sample_rate, d->out_rate, &L, &M, &H, &T);
        if (prc != Q3TTS_OK) return refuse(prc, prc == Q3TTS_ERR_UNSUPPORTED ? "document: this output rate needs more than 32768 filter coefficients" : "document: output_rate is 0 (off) or 4000..96000 Hz");
    }
    std::unique_ptr<SReq> job;
    if (voice) {  // the document's own prefix: a §23 job in front of its segments, released when the document ends
        job.reset(new SReq());
        job->kind = 1;
        q3tts_request tmp{};
        tmp.prompt = voice;
        if (copy_request(e, &tmp, job.get()) != Q3TTS_OK) return refuse(Q3TTS_ERR_INVALID, "document: the voice cannot be copied (a null array with a length)");
        job->doc = d.get();
    }
    {
        std::lock_guard<std::mutex> lk(s->mu);
        if (s->stop || s->dead) return serr(s, Q3TTS_ERR_STATE, s->dead ? "document: the session's worker failed" : "document: the session is closing");
        if (prefix && prefix->released) return serr(s, Q3TTS_ERR_INVALID, "document: the prefix was released");
        if (job) {
            job->keep = new q3tts_prefix();
            job->keep->e = e; job->keep->state.store(0);
            s->made.push_back(job->keep);
            job->id = (1ull << 63) | s->next_internal++;
            d->px = job->keep; d->own_px = true;
            s->pending.push_back(std::move(job));
        } else d->px = prefix;
        d->id = s->next_id++;
        IdState st; st.t_submit = q3_now_ms();
        s->ids[d->id] = st;
        s->doc_ids[d->id] = d;
        s->docs_new.push_back(d);
        s->docs_waiting.fetch_add(1, std::memory_order_release);
        s->doc_dirty = true;
        *id = d->id;
    }
    s->cv_work.notify_one();
    return Q3TTS_OK;
}

extern "C" int q3tts_session_document_append(q3tts_session* s, uint64_t id, const q3tts_long_segment* segs, int32_t n_segs, int32_t close) {
    if (!s) return serr(nullptr, Q3TTS_ERR_INVALID, "null session");
    std::vector<DocSeg> add;
    const char* why = "";
    const bool bad = n_segs < 0 || n_segs > Q3_JOIN_MAX_SEG || (n_segs > 0 && !segs);
    if (!bad) for (int i = 0; i < n_segs && !*why; ++i) if (segs[i].kind < 0 || segs[i].kind > 4) why = "a break kind lies outside 0..4";
    if (!bad && !*why) doc_segments(segs, n_segs, add, &why);
    {
        std::lock_guard<std::mutex> lk(s->mu);
        if (bad) return serr(s, Q3TTS_ERR_INVALID, "document_append: n_segs is 0..1024 per call, with its segments");
        if (*why) return serr(s, Q3TTS_ERR_INVALID, std::string("document_append: ") + why);
        auto it = s->doc_ids.find(id);
        auto st = s->ids.find(id);
        if (it == s->doc_ids.end() || it->second->finished || st == s->ids.end() || st->second.cancelled || st->second.final_ready)
            return serr(s, Q3TTS_ERR_INVALID, "document_append: unknown id, or the document has finished");
        Doc& d = *it->second;
        if (!d.open) return serr(s, Q3TTS_ERR_INVALID, "document_append: the document is closed");
        if (s->stop || s->dead) return serr(s, Q3TTS_ERR_STATE, "document_append: the session is closing, or its worker failed");
        for (DocSeg& g : add) d.incoming.push_back(std::move(g));
        d.n_given += n_segs;
        if (close) d.open = false;
        s->doc_dirty = true;
    }
    s->cv_work.notify_one();
    return Q3TTS_OK;
}

extern "C" int q3tts_k_session_doc_mem_cap(q3tts_session* s, int64_t bytes) {
    if (!s) return serr(nullptr, Q3TTS_ERR_INVALID, "null session");
    s->doc_mem_cap.store(bytes < 0 ? -1 : (long long)bytes, std::memory_order_relaxed);
    return Q3TTS_OK;
}

extern "C" int q3tts_session_document_info(q3tts_session* s, uint64_t id, q3tts_long_info* info, int32_t cap, int32_t* n_known, int64_t* n_delivered) {
    if (!s) return serr(nullptr, Q3TTS_ERR_INVALID, "null session");
    std::lock_guard<std::mutex> lk(s->mu);
    if (cap < 0 || (cap > 0 && !info)) return serr(s, Q3TTS_ERR_INVALID, "document_info: info missing");
    auto it = s->doc_ids.find(id);
    if (it == s->doc_ids.end()) return serr(s, Q3TTS_ERR_INVALID, "document_info: unknown id");
    const Doc& d = *it->second;
    for (int i = 0; i < cap && i < (int)d.info.size(); ++i) info[i] = d.info[i];
    if (n_known) *n_known = (int32_t)d.info.size();
    if (n_delivered) *n_delivered = d.n_delivered;
    return Q3TTS_OK;
}

// ---- voices in a session (include/q3tts.h) ----
extern "C" int q3tts_session_submit_keep_voice(q3tts_session* s, const q3tts_request* req, int32_t voice_rows, uint64_t* id, q3tts_prefix** out) {
    if (!out) return serr(nullptr, Q3TTS_ERR_INVALID, "null argument");
    return submit_request(s, req, id, voice_rows, out);
}

extern "C" int q3tts_session_prefix_create(q3tts_session* s, const q3tts_prompt_desc* p, const float* embd, int32_t n_tok, q3tts_prefix** out, uint64_t* id) {
    if (!s || !out || !id) return serr(nullptr, Q3TTS_ERR_INVALID, "null argument");
    *out = nullptr;
    auto refuse = [&](int code, const std::string& m) { std::lock_guard<std::mutex> lk(s->mu); return serr(s, code, m); };
    const char* why = "";
    if (q3_voice_job_rules(p, embd, n_tok, &why) != Q3TTS_OK) return refuse(Q3TTS_ERR_INVALID, std::string("prefix: ") + why);
    if (p && p->n_text != 0) return refuse(Q3TTS_ERR_INVALID, "prefix: a voice desc has n_text == 0");
    std::unique_ptr<SReq> q(new SReq());
    q->kind = 1; q->n_tok = n_tok;
    if (embd && n_tok >= s->e->cfg.n_ctx) q->embd.assign(1, 0.0f);  // too long: refused at admission by its length (a PREFIX event says so); no row is read
    else {
        q3tts_request tmp{};
        tmp.prompt = p; tmp.prompt_embd = embd; tmp.n_tok = n_tok;
        if (copy_request(s->e, &tmp, q.get()) != Q3TTS_OK) return refuse(Q3TTS_ERR_INVALID, "prefix: the voice cannot be copied (a null array with a length)");
    }
    {
        std::lock_guard<std::mutex> lk(s->mu);
        if (s->stop || s->dead) return serr(s, Q3TTS_ERR_STATE, s->dead ? "prefix: the session's worker failed" : "prefix: the session is closing");
        q->keep = new q3tts_prefix();
        q->keep->e = s->e; q->keep->state.store(0);
        s->made.push_back(q->keep);
        *out = q->keep;
        q->id = s->next_id++;
        IdState st; st.t_submit = q3_now_ms();
        s->ids[q->id] = st;
        *id = q->id;
        s->pending.push_back(std::move(q));
    }
    s->cv_work.notify_one();
    return Q3TTS_OK;
}

extern "C" int q3tts_session_prefix_release(q3tts_session* s, q3tts_prefix* x) {
    if (!s || !x) return serr(nullptr, Q3TTS_ERR_INVALID, "null argument");
    {
        std::lock_guard<std::mutex> lk(s->mu);
        if (x->e != s->e) return serr(s, Q3TTS_ERR_INVALID, "prefix_release: made by another engine");
        if (x->released) return serr(s, Q3TTS_ERR_INVALID, "prefix_release: released already");
        if (std::find(s->made.begin(), s->made.end(), x) == s->made.end()) s->made.push_back(x);  // (made before the session opened: the session frees it now)
        x->released = true;
        maybe_reap(s, x);
    }
    s->cv_work.notify_one();
    return Q3TTS_OK;
}

extern "C" int q3tts_session_clone(q3tts_session* s, const float* audio, int64_t n_samples, int32_t rate, int64_t* codes, int32_t cap_frames,
                                   int32_t* n_frames, float* spk_emb) {
    if (!s) return serr(nullptr, Q3TTS_ERR_INVALID, "null session");
    std::unique_lock<std::mutex> lk(s->mu);
    if (!s->e->clone) return serr(s, Q3TTS_ERR_STATE, "AudioEncoder not loaded (q3tts_clone_init was not called)");
    if (n_samples < 0 || (n_samples > 0 && !audio) || (codes && !n_frames) || rate < 4000 || rate > 96000)
        return serr(s, Q3TTS_ERR_INVALID, "clone: null argument, negative length, or a rate outside 4000..96000 Hz");
    if (s->stop || s->dead) return serr(s, Q3TTS_ERR_STATE, s->dead ? "clone: the session's worker failed" : "clone: the session is closing");
    CloneJob j;
    j.audio = audio; j.n = n_samples; j.rate = rate; j.codes = codes; j.cap = cap_frames; j.n_frames = n_frames; j.spk = spk_emb;
    s->clones.push_back(&j);
    ++s->clone_waiters;
    s->cv_work.notify_one(); s->cv_space.notify_all();  // (the worker sleeps on the one when idle, on the other while it waits for staging)
    s->cv_clone.wait(lk, [&] { return j.done; });
    --s->clone_waiters;
    const int rc = j.rc;
    if (rc != Q3TTS_OK) serr(s, rc, j.err);
    lk.unlock();
    s->cv_clone.notify_all();
    return rc;
}

// the readiness rule (include/q3tts.h, "streaming text input"): the steps producing frames f .. f + 3 read T[f .. f + 3], and open text has
// len(T) = n_text - 1
extern "C" int q3tts_k_text_ready(int32_t n_text, int32_t closed, int32_t n_frames) {
    return (closed || (long long)n_text - 1 >= (long long)n_frames + 4) ? 1 : 0;
}

extern "C" int q3tts_session_append_text(q3tts_session* s, uint64_t id, const uint32_t* ids, int32_t n, int32_t close) {
    if (!s) return serr(nullptr, Q3TTS_ERR_INVALID, "null session");
    {
        std::lock_guard<std::mutex> lk(s->mu);
        if (n < 0 || (n > 0 && !ids)) return serr(s, Q3TTS_ERR_INVALID, "append_text: ids missing");
        auto it = s->ids.find(id);
        if (it == s->ids.end() || it->second.final_ready || it->second.cancelled) return serr(s, Q3TTS_ERR_INVALID, "append_text: unknown id, or the request has finished");
        IdState& st = it->second;
        if (!st.ts) return serr(s, Q3TTS_ERR_INVALID, "append_text: the request was submitted without text_stream");
        if (st.closed) return serr(s, Q3TTS_ERR_INVALID, "append_text: the request's text is closed");
        for (int i = 0; i < n; ++i) st.T.push_back((int32_t)ids[i]);
        if (close) { st.T.push_back(EOS_TOKEN); st.closed = true; }
        if (n > 0 || close) s->text_dirty = true;
    }
    s->cv_work.notify_one();
    return Q3TTS_OK;
}

extern "C" int q3tts_session_cancel(q3tts_session* s, uint64_t id) {
    if (!s) return serr(nullptr, Q3TTS_ERR_INVALID, "null session");
    {
        std::lock_guard<std::mutex> lk(s->mu);
        auto it = s->ids.find(id);
        if (it == s->ids.end()) return serr(s, Q3TTS_ERR_INVALID, "cancel: unknown id, or its final event was delivered");
        IdState& st = it->second;
        if (st.cancelled) return Q3TTS_OK;
        st.cancelled = true;
        if (st.queued) {
            bool job = false;
            for (auto p = s->pending.begin(); p != s->pending.end(); ++p)
                if ((*p)->id == id) {  // its prefix will never be written: the handle reads failed, a PREFIX event says so
                    job = (*p)->kind == 1;
                    if (!job) unref_prefix(s, (*p)->r.prefix);
                    if ((*p)->keep) {
                        fail_keep(s, (*p)->keep, Q3TTS_ERR_STATE);
                        SEv pv = prefix_ev(id, Q3TTS_ERR_STATE, job);
                        deliver(s, pv, q3_now_ms());
                    }
                    s->pending.erase(p);
                    break;
                }
            for (auto d = s->docs_new.begin(); d != s->docs_new.end(); ++d)
                if ((*d)->id == id) {  // a document the worker has not accepted: it never will
                    (*d)->finished = true; (*d)->open = false;
                    if ((*d)->own_px) { (*d)->px->released = true; maybe_reap(s, (*d)->px); }
                    s->docs_new.erase(d);
                    break;
                }
            SEv v = final_ev(id, Q3TTS_EV_CANCELLED, Q3TTS_OK);
            if (!job) deliver(s, v, q3_now_ms());
        } else {
            for (auto r = s->ready.begin(); r != s->ready.end();) {  // no further chunk from now on; a waiting final becomes CANCELLED
                if (r->id != id) { ++r; continue; }
                if (r->kind == Q3TTS_EV_SEGMENT) { copy_result_free(r->res); r = s->ready.erase(r); continue; }  // (a cancelled document's)
                if (r->kind == Q3TTS_EV_CHUNK) {
                    if (r->ring >= 0 && --s->refs[r->ring] == 0) s->cv_space.notify_all();
                    r = s->ready.erase(r);
                    continue;
                }
                if (r->kind != Q3TTS_EV_CANCELLED) { copy_result_free(r->res); r->res.status = Q3TTS_OK; r->kind = Q3TTS_EV_CANCELLED; r->status = Q3TTS_OK; }
                ++r;
            }
            if (!st.final_ready) s->cancels.push_back(id);
        }
    }
    s->cv_work.notify_one();
    s->cv_ev.notify_all();
    return Q3TTS_OK;
}

extern "C" int q3tts_session_next(q3tts_session* s, int32_t timeout_ms, q3tts_session_event* ev) {
    if (!s || !ev) return serr(s, Q3TTS_ERR_INVALID, "null argument");
    memset(ev, 0, sizeof(*ev));
    std::unique_lock<std::mutex> lk(s->mu);
    if (s->held_ring >= 0) {
        if (--s->refs[s->held_ring] == 0) s->cv_space.notify_all();
        s->held_ring = -1;
    }
    auto ready = [&] { return !s->ready.empty() || s->stop || s->dead; };
    if (timeout_ms < 0) s->cv_ev.wait(lk, ready);
    else s->cv_ev.wait_for(lk, std::chrono::milliseconds(timeout_ms), ready);
    if (s->ready.empty()) { ev->kind = Q3TTS_EV_NONE; return Q3TTS_OK; }
    SEv v = s->ready.front();
    s->ready.pop_front();
    ev->id = v.id; ev->kind = v.kind; ev->status = v.status; ev->n_samples = v.n; ev->is_final = v.is_final;
    if (v.kind == Q3TTS_EV_CHUNK) {
        if (v.ring >= 0) { ev->pcm = (const char*)s->host[v.ring] + v.off * s->es; s->held_ring = v.ring; }  // (its reference moves to the consumer)
    } else {
        ev->result = v.res;
        if (v.is_final) s->ids.erase(v.id);  // (a keep-voice request's PREFIX event is not its last)
    }
    return Q3TTS_OK;
}

extern "C" int q3tts_session_close(q3tts_session* s) {
    if (!s) return serr(nullptr, Q3TTS_ERR_INVALID, "null session");
    {
        std::lock_guard<std::mutex> lk(s->mu);
        s->stop = true;
    }
    s->cv_work.notify_all(); s->cv_space.notify_all(); s->cv_ev.notify_all();
    if (s->th.joinable()) s->th.join();
    q3tts_engine* e = s->e;
    hipSetDevice(e->cfg.device);
    {   // callers still inside q3tts_session_clone leave first (the worker woke them); released prefixes go, the others stay the engine's
        std::unique_lock<std::mutex> lk(s->mu);
        s->cv_clone.wait(lk, [&] { return s->clone_waiters == 0; });
        for (q3tts_prefix* x : s->made) if (x->released) q3_prefix_free(x);  // (the worker synchronised both streams before it left)
        s->made.clear(); s->trash.clear();
    }
    for (Batch& b : s->flight) for (SEv& v : b.evs) copy_result_free(v.res);
    for (SEv& v : s->ready) copy_result_free(v.res);
    for (int k = 0; k < kRing; ++k) { if (s->host[k]) hipHostFree(s->host[k]); if (s->ev[k]) hipEventDestroy(s->ev[k]); }
    if (s->dev) hipFree(s->dev);
    if (Q3Swap* sw = s->swap.exchange(nullptr)) q3_swap_destroy(e, sw);  // (the worker returned every block and synchronised both streams before it left)
    const int rc = s->worker_rc;
    e->session.store(nullptr);
    delete s;
    return rc;
}

extern "C" const char* q3tts_session_last_error(const q3tts_session* s) {
    if (!s) return g_serr.c_str();
    static thread_local std::string copy;
    std::lock_guard<std::mutex> lk(const_cast<q3tts_session*>(s)->mu);
    copy = s->err;
    return copy.c_str();
}

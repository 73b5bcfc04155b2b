// q3_long.hip — long documents: the segments of a split text run as one batch in one voice, their PCM stays in device
// rows, and two kernels turn the rows into one document row: k_pcm_edges finds every row's first and last loud block, k_pcm_join writes
// every piece with its fades and the zeros of every pause. The engine calls built on them: q3tts_generate_long / q3tts_pcm_join. The
// splitter is host code of its own (q3_split.cpp). The reference has no counterpart: generate_with_voice takes one text and truncates it
// at 512 steps (src/tts/engine.rs:152).
#include "q3_engine.h"

#include <climits>
#include <cmath>
#include <cstring>

namespace {
constexpr int W = Q3_JOIN_W;
constexpr int kThreads = 256, kWaves = kThreads / 64;
constexpr int kTileBlocks = 64;  // blocks of W samples per workgroup of k_pcm_edges: 16 per wave
constexpr int kJoinTile = 4 * kThreads;  // outputs per pass of a k_pcm_join workgroup: one 16-byte destination group per thread
static_assert(W % 4 == 0 && W + 3 <= 4 * 64, "a wave covers a block in one pass of 16-byte groups, whatever the row's alignment");
}  // namespace

// ---- the kernels --------------------------------------------------------------------------------------------------------------
// grid (tiles, rows): a workgroup takes kTileBlocks blocks of row blockIdx.y, one block per wave at a time. A lane loads one 16-byte group
// of the source row where the group lies inside the block and inside [0, n), single elements at the block's and the row's edges: nothing
// at or past n is loaded. max |x| of the block by a wave reduction (fmaxf drops a NaN: a NaN is not loud), the strict comparison once per
// block, and the row's first / last loud block by integer min / max: one LDS round over the four waves, one atomic pair per workgroup.
// The result does not depend on any order. LDS: 32 bytes.
__global__ __launch_bounds__(kThreads) void k_pcm_edges(const float* __restrict__ src, size_t stride, const int32_t* __restrict__ lens, float thr,
                                                        int32_t* __restrict__ edges) {
    __shared__ int s_first[kWaves], s_last[kWaves];
    const int r = blockIdx.y;
    const long long n = lens[r];
    const long long nb = (n + W - 1) / W, b0 = (long long)blockIdx.x * kTileBlocks;
    if (b0 >= nb) return;  // (uniform over the workgroup)
    const float* row = src + (size_t)r * stride;
    const int a = (int)(((uintptr_t)row >> 2) & 3);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int first = INT_MAX, last = -1;
    for (int t = wave; t < kTileBlocks && b0 + t < nb; t += kWaves) {
        const long long b = b0 + t, g0 = b * W, g1 = min(g0 + W, n);
        const long long g = g0 - (((long long)a + g0) & 3) + 4ll * lane;  // this lane's group, on a 16-byte boundary of the source row
        float m = 0.0f;
        if (g < g1) {
            if (g >= g0 && g + 4 <= g1) {
                const float4 v = *(const float4*)(row + g);
                m = fmaxf(fmaxf(m, fabsf(v.x)), fabsf(v.y));
                m = fmaxf(fmaxf(m, fabsf(v.z)), fabsf(v.w));
            } else {
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if (g + k >= g0 && g + k < g1) m = fmaxf(m, fabsf(row[g + k]));
            }
        }
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) m = fmaxf(m, __shfl_xor(m, off, 64));
        if (m > thr) { first = min(first, (int)b); last = max(last, (int)b); }
    }
    if (lane == 0) { s_first[wave] = first; s_last[wave] = last; }
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int w = 1; w < kWaves; ++w) { first = min(first, s_first[w]); last = max(last, s_last[w]); }
        if (last >= 0) { atomicMin(edges + 2 * r, first); atomicMax(edges + 2 * r + 1, last); }
    }
}

void q3_launch_pcm_edges(const float* src, size_t stride, const int32_t* lens, int rows, long long max_len, float threshold, int32_t* edges, hipStream_t s) {
    if (rows <= 0 || max_len <= 0) return;
    const long long tiles = ((max_len + W - 1) / W + kTileBlocks - 1) / kTileBlocks;
    hipLaunchKernelGGL(k_pcm_edges, dim3((unsigned)tiles, rows), dim3(kThreads), 0, s, src, stride, lens, threshold, edges);
}

// grid (x, rows): the workgroups of row blockIdx.y walk the 16-byte groups of the destination range [off, off + L + gap), one group per
// thread and pass: the piece's samples by dword loads (lo makes the source misaligned), the two fades' gain g = (float)(j + 1) / (float)(F
// + 1) by one correctly rounded division and one rounded multiply, +0.0f behind the piece; one 16-byte store where the group lies inside
// the range, single elements at its two ends (a group that two segments share is written by both, each its own elements). No LDS.
__global__ __launch_bounds__(kThreads) void k_pcm_join(const float* __restrict__ src, size_t stride, const Q3JoinSeg* __restrict__ segs, float* __restrict__ dst) {
    const Q3JoinSeg sg = segs[blockIdx.y];
    const long long L = sg.L, F = sg.F, T = sg.L + sg.gap;
    if (T <= 0) return;
    const float* x = src + (size_t)blockIdx.y * stride + sg.lo;
    const long long d_lo = sg.off, d_hi = sg.off + T;
    const long long gs = d_lo - (((long long)(((uintptr_t)dst >> 2) & 3) + d_lo) & 3);
    const long long groups = (d_hi - gs + 3) >> 2;
    const float den = (float)(F + 1);
    for (long long q = (long long)blockIdx.x * kThreads + threadIdx.x; q < groups; q += (long long)gridDim.x * kThreads) {
        const long long d = gs + 4 * q;
        float v[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const long long j = d + k - d_lo;
            float y = 0.0f;
            if (j >= 0 && j < L) {
                y = x[j];
                if (j < F) y = __fmul_rn(y, __fdiv_rn((float)(j + 1), den));
                else if (j >= L - F) y = __fmul_rn(y, __fdiv_rn((float)(L - j), den));
            }
            v[k] = y;
        }
        if (d >= d_lo && d + 4 <= d_hi) *(float4*)(dst + d) = make_float4(v[0], v[1], v[2], v[3]);
        else {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (d + k >= d_lo && d + k < d_hi) dst[d + k] = v[k];
        }
    }
}

void q3_launch_pcm_join(const float* src, size_t stride, const Q3JoinSeg* segs, int rows, long long max_span, float* dst, hipStream_t s) {
    if (rows <= 0 || max_span <= 0) return;
    const long long tiles = (max_span + 3 + kJoinTile - 1) / kJoinTile;
    const int gx = (int)std::max(1ll, std::min(tiles, (long long)std::max(1, 4096 / rows)));
    hipLaunchKernelGGL(k_pcm_join, dim3(gx, rows), dim3(kThreads), 0, s, src, stride, segs, dst);
}

// ---- the plan (host) ----------------------------------------------------------------------------------------------------------
int q3_join_opts_rules(const q3tts_join_opts& o, const char** msg) {
    *msg = nullptr;
    if (o.trim != 0 && o.trim != 1) *msg = "join: trim is 0 or 1";
    else if (!(o.threshold >= 0.0f)) *msg = "join: the threshold is negative or NaN";
    else if (o.keep < 0 || o.fade < 0) *msg = "join: keep and fade are sample counts (>= 0)";
    else for (int k = 0; k < 5; ++k) if (o.pause_ms[k] < 0 || o.pause_ms[k] > 60000) *msg = "join: a pause lies outside 0..60000 ms";
    return *msg ? Q3TTS_ERR_INVALID : Q3TTS_OK;
}

long long q3_join_plan(const int32_t* lens, const int32_t* kinds, const int32_t* edges, int rows, const q3tts_join_opts& o, int rate,
                       long long* plan, Q3JoinSeg* segs, long long* max_span) {
    long long cur = 0, span = 0;
    int prev = -1, kmax = 0;  // the last non-empty piece so far; the largest break kind since it (its own included)
    for (int i = 0; i < rows; ++i) {
        const long long n = lens[i];
        long long lo = 0, hi = n;
        if (o.trim) {
            const long long first = edges[2 * i], last = edges[2 * i + 1];
            if (last < 0) lo = hi = 0;
            else { lo = std::max(0ll, first * W - o.keep); hi = std::min(n, (last + 1) * W + o.keep); }
        }
        const long long L = hi - lo;
        segs[i] = Q3JoinSeg{lo, L, cur, 0, (int32_t)std::min<long long>(o.fade, L / 2), 0};
        if (L > 0) {
            if (prev >= 0) {  // the pause in front of this piece belongs to the piece before it
                const long long gap = (long long)o.pause_ms[kmax] * rate / 1000;
                segs[prev].gap = gap; span = std::max(span, segs[prev].L + gap);
                cur += gap; segs[i].off = cur;
            }
            cur += L;
            prev = i; kmax = kinds[i];
            span = std::max(span, L);
        } else if (prev >= 0) kmax = std::max(kmax, (int)kinds[i]);
        if (plan) { plan[4 * i] = lo; plan[4 * i + 1] = hi; plan[4 * i + 2] = segs[i].off; plan[4 * i + 3] = segs[i].off + L; }
    }
    if (max_span) *max_span = span;
    return cur;
}

// ---- the engine calls ---------------------------------------------------------------------------------------------------------
namespace {
struct Tmp {  // a device buffer of one call
    void* p = nullptr;
    ~Tmp() { if (p) hipFree(p); }
    int alloc(size_t bytes) { return hipMalloc(&p, std::max<size_t>(bytes, 4)) == hipSuccess ? 0 : -1; }
};

// rows [n][stride] on the device -> the document row: edges, plan, join, on e->stream (not synchronised after the join's launch).
// plan [n][4] (host) and *N are complete on return; doc is allocated here.
int join_rows(q3tts_engine* e, const float* rows, size_t stride, const int32_t* lens, const int32_t* kinds, int n, const q3tts_join_opts& o,
              long long* plan, long long* N, Tmp& doc) {
    hipStream_t s = e->stream;
    const int rate = e->cfg.vocoder.sample_rate;
    std::vector<int32_t> edges((size_t)2 * n);
    for (int i = 0; i < n; ++i) { edges[2 * i] = INT_MAX; edges[2 * i + 1] = -1; }
    Tmp dl, de, ds;
    if (dl.alloc(sizeof(int32_t) * n) || de.alloc(sizeof(int32_t) * 2 * n) || ds.alloc(sizeof(Q3JoinSeg) * n)) return q3_set_err(e, Q3TTS_ERR_OOM, "hipMalloc (join tables)");
    Q3_HIP(e, hipMemcpyAsync(dl.p, lens, sizeof(int32_t) * n, hipMemcpyHostToDevice, s));
    if (o.trim) {  // (without trim the edges are not read)
        Q3_HIP(e, hipMemcpyAsync(de.p, edges.data(), sizeof(int32_t) * 2 * n, hipMemcpyHostToDevice, s));
        long long mx = 0;
        for (int i = 0; i < n; ++i) mx = std::max<long long>(mx, lens[i]);
        q3_launch_pcm_edges(rows, stride, (const int32_t*)dl.p, n, mx, o.threshold, (int32_t*)de.p, s);
        Q3_HIP(e, hipGetLastError());
        Q3_HIP(e, hipMemcpyAsync(edges.data(), de.p, sizeof(int32_t) * 2 * n, hipMemcpyDeviceToHost, s));
    }
    Q3_HIP(e, hipStreamSynchronize(s));
    std::vector<Q3JoinSeg> segs((size_t)n);
    long long span = 0;
    *N = q3_join_plan(lens, kinds, edges.data(), n, o, rate, plan, segs.data(), &span);
    if (*N > (1ll << 28)) return q3_set_err(e, Q3TTS_ERR_INVALID, "join: the document exceeds 2^28 samples");
    if (doc.alloc(sizeof(float) * (size_t)*N)) return q3_set_err(e, Q3TTS_ERR_OOM, "hipMalloc (document row)");
    Q3_HIP(e, hipMemcpyAsync(ds.p, segs.data(), sizeof(Q3JoinSeg) * n, hipMemcpyHostToDevice, s));
    q3_launch_pcm_join(rows, stride, (const Q3JoinSeg*)ds.p, n, span, (float*)doc.p, s);
    Q3_HIP(e, hipGetLastError());
    Q3_HIP(e, hipStreamSynchronize(s));  // (segs and the tables outlive the launch)
    return Q3TTS_OK;
}

void default_join(q3tts_join_opts* j) {
    j->trim = 1; j->threshold = 0.01f; j->keep = 480; j->fade = 120;
    const int32_t p[5] = {0, 0, 150, 300, 600};
    memcpy(j->pause_ms, p, sizeof(p));
}
}  // namespace

extern "C" void q3tts_long_default_opts(q3tts_long_opts* o) {
    if (!o) return;
    memset(o, 0, sizeof(*o));
    default_join(&o->join);
}

extern "C" void q3tts_long_result_free(q3tts_long_result* r) {
    if (!r) return;
    q3_pin_free(r->pcm);
    free(r->info);
    r->pcm = nullptr; r->info = nullptr;
}

extern "C" int q3tts_pcm_join(q3tts_engine* e, const float* const* clips, const int64_t* n, const int32_t* kinds, int32_t n_clips,
                              const q3tts_join_opts* opts, float* out, int64_t cap, int64_t* n_out, int64_t* edges) {
    if (!e || !clips || !n || !kinds || !n_out || cap < 0 || (cap > 0 && !out)) return q3_set_err(e, Q3TTS_ERR_INVALID, "pcm join: null argument or negative capacity");
    Q3_NOT_IN_SESSION(e);
    if (n_clips <= 0 || n_clips > Q3_JOIN_MAX_SEG) return q3_set_err(e, Q3TTS_ERR_INVALID, "pcm join: n_clips outside 1..1024");
    q3tts_join_opts o;
    if (opts) o = *opts; else default_join(&o);
    const char* msg = nullptr;
    if (q3_join_opts_rules(o, &msg) != Q3TTS_OK) return q3_set_err(e, Q3TTS_ERR_INVALID, msg);
    long long mx = 0, total = 0;
    for (int i = 0; i < n_clips; ++i) {
        if (n[i] < 0 || (n[i] > 0 && !clips[i])) return q3_set_err(e, Q3TTS_ERR_INVALID, "pcm join: a clip is null or has a negative length");
        if (kinds[i] < 0 || kinds[i] > 4) return q3_set_err(e, Q3TTS_ERR_INVALID, "pcm join: a break kind lies outside 0..4");
        mx = std::max<long long>(mx, n[i]); total += n[i];
    }
    if (total > (1ll << 28)) return q3_set_err(e, Q3TTS_ERR_INVALID, "pcm join: more than 2^28 input samples");
    Q3_HIP(e, hipSetDevice(e->cfg.device));
    // the clips as rows of one buffer whose stride is the longest clip
    const size_t stride = (size_t)std::max(mx, 1ll);
    Tmp rows, doc;
    if (rows.alloc(sizeof(float) * stride * (size_t)n_clips)) return q3_set_err(e, Q3TTS_ERR_OOM, "hipMalloc (pcm join rows)");
    std::vector<int32_t> lens((size_t)n_clips);
    for (int i = 0; i < n_clips; ++i) {
        lens[i] = (int32_t)n[i];
        if (n[i] > 0) Q3_HIP(e, hipMemcpyAsync((float*)rows.p + (size_t)i * stride, clips[i], sizeof(float) * (size_t)n[i], hipMemcpyHostToDevice, e->stream));
    }
    std::vector<long long> plan((size_t)4 * n_clips);
    long long N = 0;
    TRY(join_rows(e, (const float*)rows.p, stride, lens.data(), kinds, n_clips, o, plan.data(), &N, doc));
    *n_out = N;
    if (edges) for (size_t k = 0; k < plan.size(); ++k) edges[k] = plan[k];
    if (cap < N) return q3_set_err(e, Q3TTS_ERR_INVALID, "pcm join: out holds fewer than N samples (*n_out says how many)");
    if (N > 0) Q3_HIP(e, hipMemcpy(out, doc.p, sizeof(float) * (size_t)N, hipMemcpyDeviceToHost));
    return Q3TTS_OK;
}

extern "C" int q3tts_generate_long(q3tts_engine* e, const q3tts_request* tmpl, const q3tts_prompt_desc* voice, const q3tts_prefix* prefix,
                                   const q3tts_long_segment* segs, int32_t n_segs, const q3tts_long_opts* opts, q3tts_long_result* out) {
    if (!e || !tmpl || !segs || !out) return q3_set_err(e, Q3TTS_ERR_INVALID, "generate long: null argument");
    memset(out, 0, sizeof(*out));
    out->status = Q3TTS_ERR_STATE;
    Q3_NOT_IN_SESSION(e);
    if (e->streams_open > 0) return q3_set_err(e, Q3TTS_ERR_STATE, "a stream is open on this engine (q3tts_stream_end first)");
    if (e->speed) return q3_set_err(e, Q3TTS_ERR_STATE, "q3tts_set_speed is the engine's, for plain requests: a document carries its own speed in opts (q3tts_set_speed(engine, 0) first)");
    if (e->out_rate) return q3_set_err(e, Q3TTS_ERR_STATE, "q3tts_set_output_rate is the engine's, for plain requests: a document carries its own rate in opts (q3tts_set_output_rate(engine, 0) first)");
    if (!e->voc) return q3_set_err(e, Q3TTS_ERR_INVALID, "a document needs with_vocoder = 1");
    if (n_segs <= 0 || n_segs > Q3_JOIN_MAX_SEG) return q3_set_err(e, Q3TTS_ERR_INVALID, "generate long: n_segs outside 1..1024");
    if ((voice != nullptr) == (prefix != nullptr)) return q3_set_err(e, Q3TTS_ERR_INVALID, "generate long: give exactly one of voice and prefix");
    if (voice && voice->n_text != 0) return q3_set_err(e, Q3TTS_ERR_INVALID, "generate long: voice is a voice-only desc (n_text == 0): the text is in the segments");
    if (tmpl->text_stream == 1 || tmpl->prompt_embd || tmpl->prompt || tmpl->prefix)
        return q3_set_err(e, Q3TTS_ERR_INVALID, "generate long: the template carries no prompt (prompt_embd, prompt, prefix NULL; text_stream off)");
    q3tts_long_opts o;
    if (opts) o = *opts; else q3tts_long_default_opts(&o);
    const char* msg = nullptr;
    if (q3_join_opts_rules(o.join, &msg) != Q3TTS_OK) return q3_set_err(e, Q3TTS_ERR_INVALID, msg);
    const int native = e->cfg.vocoder.sample_rate;
    const int speed = (o.speed_permille == 0 || o.speed_permille == 1000) ? 0 : o.speed_permille;
    const int rate = (o.output_rate == 0 || o.output_rate == native) ? 0 : o.output_rate;
    if (speed && (speed < Q3_TEMPO_MIN || speed > Q3_TEMPO_MAX)) return q3_set_err(e, Q3TTS_ERR_INVALID, "generate long: speed is 0 or 1000 (off), or 500..2000 per mille");
    if (rate && (rate < 4000 || rate > 96000)) return q3_set_err(e, Q3TTS_ERR_INVALID, "generate long: output rate is 0 (native) or 4000..96000 Hz");
    for (int i = 0; i < n_segs; ++i) {
        if (segs[i].kind < 0 || segs[i].kind > 4) return q3_set_err(e, Q3TTS_ERR_INVALID, "generate long: a break kind lies outside 0..4");
        if (segs[i].n_ids < 0 || (segs[i].n_ids > 0 && !segs[i].ids) || segs[i].max_steps < 0) return q3_set_err(e, Q3TTS_ERR_INVALID, "generate long: a segment's ids are null or a count is negative");
    }
    Q3_HIP(e, hipSetDevice(e->cfg.device));
    const double t0 = q3_now_ms();
    Q3Resamp rs{};
    if (rate) TRY(q3_resample_get(e, native, rate, &rs));  // (the table of a pair is kept on the engine, as q3tts_resample keeps it)

    // the bytes first: n_segs device rows and the document rows at their largest, against what the device has free
    const int spf = q3_voc_samples_per_frame(e), cap_steps = e->cfg.max_steps_cap;
    const size_t stride = (size_t)cap_steps * spf;
    int pmax = 0;
    for (int k = 0; k < 5; ++k) pmax = std::max(pmax, (int)o.join.pause_ms[k]);
    long long dmax = (long long)(n_segs - 1) * pmax * native / 1000;
    for (int i = 0; i < n_segs; ++i) {
        const int ms = segs[i].max_steps ? segs[i].max_steps : (tmpl->max_steps ? tmpl->max_steps : e->max_steps);
        dmax += (long long)std::min(ms, cap_steps) * spf;
    }
    {
        const bool regrow = e->dev_pcm_n < n_segs || e->dev_pcm_stride != stride;
        const size_t back = regrow ? (size_t)e->dev_pcm_n * e->dev_pcm_stride * sizeof(float) : 0;
        const long long st = speed ? q3_tempo_N(dmax, speed) : dmax;
        const size_t need = (regrow ? (size_t)n_segs * stride * sizeof(float) : 0) +
                            sizeof(float) * (size_t)(dmax + (speed ? st : 0) + (rate ? q3_resample_N(st, rs.L, rs.M) : 0));
        size_t free_b = 0, total_b = 0;
        Q3_HIP(e, hipMemGetInfo(&free_b, &total_b));
        if (need > free_b + back)
            return q3_set_err(e, Q3TTS_ERR_OOM, "generate long: the segments' rows and the document need " + std::to_string(need) + " bytes, the device has " + std::to_string(free_b + back) + " bytes free");
    }

    q3tts_prefix* own = nullptr;
    if (voice) TRY(q3tts_prefix_create(e, voice, nullptr, 0, &own));
    const q3tts_prefix* px = voice ? own : prefix;
    struct Own { q3tts_prefix* x; ~Own() { if (x) q3tts_prefix_destroy(x); } } own_guard{own};

    // the segments as requests
    std::vector<q3tts_prompt_desc> descs((size_t)n_segs);
    std::vector<q3tts_request> reqs((size_t)n_segs);
    std::vector<q3tts_result> res((size_t)n_segs);
    q3tts_request base = *tmpl;
    if (base.use_engine_sampler == 1) {
        base.use_engine_sampler = 0;
        base.temperature = e->temperature; base.top_k = e->top_k; base.top_p = e->top_p; base.has_seed = e->has_seed; base.seed = e->seed;
    }
    for (int i = 0; i < n_segs; ++i) {
        q3tts_prompt_desc& d = descs[i];
        memset(&d, 0, sizeof(d));
        d.text_ids = segs[i].ids; d.n_text = segs[i].n_ids; d.lang_id = -1; d.spk_id = -1;
        q3tts_request& r = reqs[i];
        r = base;
        r.prompt = &d; r.prefix = px; r.want_pcm = 2; r.text_stream = 0; r.text_open = 0;
        if (segs[i].max_steps) r.max_steps = segs[i].max_steps;
        if (base.has_seed) r.seed = base.seed + (uint64_t)i;
    }
    const int was_on = e->dev_pcm_on;
    e->dev_pcm_on = 1;
    const int brc = q3tts_generate_batch(e, reqs.data(), n_segs, res.data());
    e->dev_pcm_on = was_on;
    struct Res { std::vector<q3tts_result>& r; ~Res() { for (q3tts_result& x : r) q3tts_result_free(&x); } } res_guard{res};
    if (brc != Q3TTS_OK) { out->status = brc; return brc; }
    out->generate_ms = (float)(q3_now_ms() - t0);

    out->info = (q3tts_long_info*)calloc((size_t)n_segs, sizeof(q3tts_long_info));
    if (!out->info) return q3_set_err(e, Q3TTS_ERR_OOM, "malloc");
    out->n_segments = n_segs; out->sample_rate = rate ? rate : native;
    int failed = Q3TTS_OK, failed_i = -1;
    std::vector<int32_t> lens((size_t)n_segs), kinds((size_t)n_segs);
    for (int i = 0; i < n_segs; ++i) {
        q3tts_long_info& f = out->info[i];
        f.status = res[i].status; f.n_frames = res[i].n_frames; f.hit_eos = res[i].hit_eos; f.n_native = res[i].n_samples;
        if (res[i].status != Q3TTS_OK && failed == Q3TTS_OK) { failed = res[i].status; failed_i = i; }
        if (res[i].status == Q3TTS_OK && !res[i].hit_eos) ++out->n_truncated;
        lens[i] = res[i].n_samples; kinds[i] = segs[i].kind;
    }
    if (failed != Q3TTS_OK) {
        out->status = failed;
        return q3_set_err(e, failed, "generate long: segment " + std::to_string(failed_i) + " failed by itself: " + e->err);
    }

    // edges, join, speed, rate, one copy
    const double t1 = q3_now_ms();
    hipStream_t s = e->stream;
    std::vector<long long> plan((size_t)4 * n_segs);
    long long N = 0;
    Tmp doc, st, rsd, win, pl;
    TRY(join_rows(e, e->dev_pcm, e->dev_pcm_stride, lens.data(), kinds.data(), n_segs, o.join, plan.data(), &N, doc));
    const float* from = (const float*)doc.p;
    long long n_cur = N;
    std::vector<float> w;
    if (speed && n_cur > 0) {
        const long long Nt = q3_tempo_N(n_cur, speed);
        q3_tempo_window(w);
        if (st.alloc(sizeof(float) * (size_t)Nt) || win.alloc(sizeof(float) * w.size()) || pl.alloc(sizeof(long long))) return q3_set_err(e, Q3TTS_ERR_OOM, "hipMalloc (document row, stretched)");
        Q3_HIP(e, hipMemcpyAsync(win.p, w.data(), sizeof(float) * w.size(), hipMemcpyHostToDevice, s));
        q3_time_stretch_dev(from, n_cur, speed, (float*)st.p, (const float*)win.p, (long long*)pl.p, s);
        Q3_HIP(e, hipGetLastError());
        from = (const float*)st.p; n_cur = Nt;
    }
    if (rate && n_cur > 0) {
        const long long Nr = q3_resample_N(n_cur, rs.L, rs.M);
        if (rsd.alloc(sizeof(float) * (size_t)Nr)) return q3_set_err(e, Q3TTS_ERR_OOM, "hipMalloc (document row, resampled)");
        if (q3_resample_dev(from, n_cur, rs, (float*)rsd.p, s) != 0) return q3_set_err(e, Q3TTS_ERR_UNSUPPORTED, "resample: the input span of one tile does not fit the LDS");
        Q3_HIP(e, hipGetLastError());
        from = (const float*)rsd.p; n_cur = Nr;
    }
    out->pcm = q3_pin_alloc(sizeof(float) * (size_t)std::max(1ll, n_cur));
    if (!out->pcm) return q3_set_err(e, Q3TTS_ERR_OOM, "hipHostMalloc");
    if (n_cur > 0) Q3_HIP(e, hipMemcpyAsync(out->pcm, from, sizeof(float) * (size_t)n_cur, hipMemcpyDeviceToHost, s));
    Q3_HIP(e, hipStreamSynchronize(s));  // (w outlives its upload)
    out->n_samples = n_cur;
    auto map = [&](long long x) {
        if (speed) x = q3_tempo_N(x, speed);
        if (rate) x = q3_resample_N(x, rs.L, rs.M);
        return x;
    };
    for (int i = 0; i < n_segs; ++i) {
        q3tts_long_info& f = out->info[i];
        f.lo = plan[4 * i]; f.hi = plan[4 * i + 1]; f.begin = plan[4 * i + 2]; f.end = plan[4 * i + 3];
        f.out_begin = map(f.begin); f.out_end = map(f.end);
    }
    const double t2 = q3_now_ms();
    out->join_ms = (float)(t2 - t1); out->total_ms = (float)(t2 - t0);
    out->status = Q3TTS_OK;
    return Q3TTS_OK;
}

// q3_tempo.hip — the speaking rate: a WSOLA (waveform-similarity overlap-add) time-stretch of the PCM on the device, pitch
// kept. One kernel (k_pcm_tempo) that fills a slot's tempo row from its vocoder row, frame by frame, as a pure function of the row's prefix;
// every PCM exit then reads the tempo rows, through the same pack / resample launches as before. The engine calls built on it:
// q3tts_set_speed / q3tts_get_speed / q3tts_time_stretch. The reference has no counterpart: its only rate control is the instruct text.
#include "q3_engine.h"

#include <cmath>

namespace {
constexpr int Hs = Q3_TEMPO_HS, Wn = Q3_TEMPO_WN, Dmin = Q3_TEMPO_DMIN, Nd = Q3_TEMPO_ND, Hold = Q3_TEMPO_HOLD;
constexpr int kSpan = Nd - 1 + Wn;  // 767: the samples the 256 candidates of a frame cover
static_assert(Wn == 2 * Hs && Nd == 256 && Hs == Nd && Wn % 4 == 0, "one thread per candidate and per output of a frame");
static_assert(Hold == Dmin + Nd - 1 + Wn + 1 && Hold == 640, "the hold-back covers the furthest candidate's window");

inline long long analysis_pos(long long k, int s) { return (k * Hs * s) / 1000; }
// need_k: the first sample frame k may not have to wait for — everything it reads lies below need_k + Hold
inline long long need_of(long long k, int s) { return k <= 0 ? 0 : std::max(analysis_pos(k, s), analysis_pos(k - 1, s) + Hs); }
}  // namespace

long long q3_tempo_N(long long n, int s) { return n <= 0 ? 0 : (n * 1000 + s - 1) / s; }

long long q3_tempo_frames(long long n, int s, bool done) {
    if (done) return (q3_tempo_N(n, s) + Hs - 1) / Hs;
    const long long lim = n - Hold;
    if (lim < 0) return 0;
    long long k = (lim * 1000) / ((long long)Hs * s) + 2;  // a_k > lim from here on (need_k >= a_k, and both ascend with k)
    while (k > 0 && need_of(k, s) > lim) --k;
    return k + 1;
}

void q3_tempo_window(std::vector<float>& w) {
    const double pi = 3.14159265358979323846;
    w.resize(Wn);
    for (int j = 0; j < Wn; ++j) w[j] = (float)(0.5 - 0.5 * std::cos(2.0 * pi * (double)j / (double)Wn));
}

// ---- the kernels --------------------------------------------------------------------------------------------------------------
// Two addressings of one arithmetic. Ring = false: the row is linear (k_pcm_tempo, as ever). Ring = true (k_doc_tempo):
// the row is a ring of C samples that holds position g at g mod C, its base 16-byte aligned (a == 0) and C a multiple of 4, so an
// aligned group of four never crosses the wrap. Positions of J stay below 2^28 and those of the stretched audio below 2^29 (speed 500):
// the modulus is an unsigned 32-bit one.
template <bool Ring>
__device__ __forceinline__ long long tempo_at(long long g, unsigned C) { return Ring ? (long long)((unsigned)g % C) : g; }

// dst[0, count) = row[g0, g0 + count), zeros outside [0, n): whole 16-byte groups of the source row with one load where they lie inside
// [0, n), element by element at the edges. Nothing at or past n is loaded. a: the row's first sample's offset within its 16-byte group.
template <bool Ring>
__device__ __forceinline__ void tempo_stage(float* dst, const float* __restrict__ row, int a, unsigned C, long long g0, int count, long long n, int tid) {
    const long long gs = g0 - ((((long long)a + g0) % 4 + 4) % 4);
    const int n4 = (int)((g0 + count - gs + 3) >> 2);
    for (int j = tid; j < n4; j += Nd) {
        const long long g = gs + 4ll * j;
        float4 v;
        if (g >= 0 && g + 4 <= n) v = *(const float4*)(row + tempo_at<Ring>(g, C));
        else {
            v.x = (g >= 0 && g < n) ? row[tempo_at<Ring>(g, C)] : 0.0f;
            v.y = (g + 1 >= 0 && g + 1 < n) ? row[tempo_at<Ring>(g + 1, C)] : 0.0f;
            v.z = (g + 2 >= 0 && g + 2 < n) ? row[tempo_at<Ring>(g + 2, C)] : 0.0f;
            v.w = (g + 3 >= 0 && g + 3 < n) ? row[tempo_at<Ring>(g + 3, C)] : 0.0f;
        }
        const int d = (int)(g - g0);  // -3 .. count - 1
        if (d >= 0 && d < count) dst[d] = v.x;
        if (d + 1 >= 0 && d + 1 < count) dst[d + 1] = v.y;
        if (d + 2 >= 0 && d + 2 < count) dst[d + 2] = v.z;
        if (d + 3 >= 0 && d + 3 < count) dst[d + 3] = v.w;
    }
}

// One workgroup of 256 threads walks frames [k_from, k_to) of one row in order (delta_k needs p_{k-1}). For a frame it stages the template
// t[j] = x[p_{k-1} + Hs + j] (512) and the candidates' span x[a_k + Dmin + i] (767) in LDS; thread i runs the chain of candidate
// delta = Dmin + i alone — acc = acc + x * t over ascending j, one f32 multiply and one f32 add per step; the template word is an LDS
// broadcast (16 bytes at a time), the span word xs[i + j] lies in consecutive banks for consecutive lanes — then the first maximum over the
// 256 sums by comparisons (value, then the lower index), and thread j writes output j of the frame: the old frame's second window half
// times the template's first half, plus the new frame's first window half times the span at the winner. LDS: 2 KiB + 3 KiB + 32 bytes.
// y: the outputs' row (Ring: a ring of CT samples); *p_slot holds p of frame k_from - 1 (read when k_from >= 2) and receives p of
// frame k_to - 1; dl != null: dl[k] = delta_k for k < dl_cap.
template <bool Ring>
__device__ __forceinline__ void tempo_walk(const float* __restrict__ row, int a, unsigned C, long long n, float* __restrict__ y, unsigned CT,
                                           long long* __restrict__ p_slot, const float* __restrict__ win, int s, int k_from, int k_to, long long n_out,
                                           int32_t* __restrict__ dl, size_t dl_cap) {
    __shared__ float4 ts4[Wn / 4];
    __shared__ float xs[kSpan + 1];
    __shared__ float red_v[Nd / 64];
    __shared__ int red_i[Nd / 64];
    float* ts = (float*)ts4;
    const int tid = threadIdx.x;
    const float w0 = win[tid], w1 = win[tid + Hs];
    int k = k_from;
    long long pprev = k >= 2 ? *p_slot : 0;  // p_0 = 0
    if (k == 0) {  // p_{-1} = -Hs: both terms read x[j]
        const float x = tid < n ? row[tid] : 0.0f;
        if (tid < n_out) y[tid] = __fadd_rn(__fmul_rn(w1, x), __fmul_rn(w0, x));
        if (dl && tid == 0 && dl_cap > 0) dl[0] = 0;
        k = 1;
    }
    for (; k < k_to; ++k) {
        const long long ak = ((long long)k * Hs * s) / 1000;
        __syncthreads();  // the previous frame is done with ts, xs and red
        tempo_stage<Ring>(ts, row, a, C, pprev + Hs, Wn, n, tid);
        tempo_stage<Ring>(xs, row, a, C, ak + Dmin, kSpan, n, tid);
        __syncthreads();
        const float* xp = xs + tid;
        float acc = 0.0f;
#pragma unroll 4
        for (int j4 = 0; j4 < Wn / 4; ++j4) {
            const float4 t = ts4[j4];
            acc = __fadd_rn(acc, __fmul_rn(xp[4 * j4], t.x));
            acc = __fadd_rn(acc, __fmul_rn(xp[4 * j4 + 1], t.y));
            acc = __fadd_rn(acc, __fmul_rn(xp[4 * j4 + 2], t.z));
            acc = __fadd_rn(acc, __fmul_rn(xp[4 * j4 + 3], t.w));
        }
        float bv = acc; int bi = tid;
        for (int off = 1; off < 64; off <<= 1) {  // (value, lower index) is a total order on finite sums: every lane ends with the wave's first maximum
            const float ov = __shfl_xor(bv, off, 64);
            const int oi = __shfl_xor(bi, off, 64);
            if (ov > bv || (ov == bv && oi < bi)) { bv = ov; bi = oi; }
        }
        if ((tid & 63) == 0) { red_v[tid >> 6] = bv; red_i[tid >> 6] = bi; }
        __syncthreads();
        bv = red_v[0]; bi = red_i[0];
#pragma unroll
        for (int w = 1; w < Nd / 64; ++w) {
            const float ov = red_v[w];
            if (ov > bv) { bv = ov; bi = red_i[w]; }  // (a later wave's indices are higher: a tie keeps the earlier one)
        }
        const long long m = (long long)k * Hs + tid;
        if (m < n_out) y[tempo_at<Ring>(m, CT)] = __fadd_rn(__fmul_rn(w1, ts[tid]), __fmul_rn(w0, xs[bi + tid]));
        if (dl && tid == 0 && (size_t)k < dl_cap) dl[k] = Dmin + bi;
        pprev = ak + Dmin + bi;
    }
    if (tid == 0) *p_slot = pprev;
}

// grid (n_ent): one workgroup per entry, rows linear
__global__ __launch_bounds__(Nd) void k_pcm_tempo(const float* __restrict__ src, size_t stride, float* __restrict__ dst, size_t dst_stride,
                                                  long long* __restrict__ p_last, const float* __restrict__ win, int s, const Q3TempoPack ents,
                                                  int32_t* __restrict__ delta, size_t delta_stride) {
    const Q3TempoEnt en = ents.e[blockIdx.x];
    if (en.k_to <= en.k_from || en.k_from < 0) return;  // (uniform over the workgroup)
    const float* row = src + (size_t)en.row * stride;
    tempo_walk<false>(row, (int)(((uintptr_t)row >> 2) & 3), 0u, en.n, dst + (size_t)en.row * dst_stride, 0u, p_last + en.row, win, s, en.k_from, en.k_to,
                      en.n_out, delta ? delta + (size_t)en.row * delta_stride : nullptr, delta_stride);
}

// grid (1): the ring form, one document. Frames [k_from, k_to) of the joined audio J, of which rj (C_J samples, J at positions mod C_J)
// holds the last C_J of the n joined so far, into rt (C_T samples, the stretched audio at positions mod C_T); outputs m >= n_out are not
// written. The host guarantees that every position a frame reads is still in rj and that no frame overwrites a position of rt that the
// exit still reads (q3_doc_ring_step).
__global__ __launch_bounds__(Nd) void k_doc_tempo(const float* __restrict__ rj, unsigned cj, float* __restrict__ rt, unsigned ct, long long* __restrict__ p_last,
                                                  const float* __restrict__ win, int s, long long n, int k_from, int k_to, long long n_out,
                                                  int32_t* __restrict__ delta, size_t delta_cap) {
    if (k_to <= k_from || k_from < 0) return;
    tempo_walk<true>(rj, 0, cj, n, rt, ct, p_last, win, s, k_from, k_to, n_out, delta, delta_cap);
}

void q3_launch_doc_tempo(const float* rj, long long cj, float* rt, long long ct, long long* p_last, const float* win, int permille, long long n,
                         int k_from, int k_to, long long n_out, int32_t* delta, size_t delta_cap, hipStream_t s) {
    if (k_to <= k_from) return;
    hipLaunchKernelGGL(k_doc_tempo, dim3(1), dim3(Nd), 0, s, rj, (unsigned)cj, rt, (unsigned)ct, p_last, win, permille, n, k_from, k_to, n_out, delta, delta_cap);
}

void q3_launch_pcm_tempo(const float* src, size_t stride, float* dst, size_t dst_stride, long long* p_last, const float* win, int permille,
                         const Q3TempoPack& ents, int n_ent, int32_t* delta, size_t delta_stride, hipStream_t s) {
    if (n_ent <= 0) return;
    hipLaunchKernelGGL(k_pcm_tempo, dim3(n_ent), dim3(Nd), 0, s, src, stride, dst, dst_stride, p_last, win, permille, ents, delta, delta_stride);
}

// ---- engine state -------------------------------------------------------------------------------------------------------------
int q3_tempo_slots(q3tts_engine* e, const int* slots, const int* ns, const char* done, int count, hipStream_t s) {
    if (!e->speed) return Q3TTS_OK;
    Q3TempoPack pk{};
    int n = 0;
    auto flush = [&]() {
        q3_launch_pcm_tempo(q3_voc_pcm(e, 0), q3_voc_pcm_stride(e), e->tp_row, e->tp_stride, e->tp_last, e->tp_win, e->speed, pk, n, nullptr, 0, s);
        n = 0;
    };
    for (int i = 0; i < count; ++i) {
        const int b = slots[i];
        const long long kt = q3_tempo_frames(ns[i], e->speed, done[i] != 0), nv = q3_tempo_valid(ns[i], e->speed, done[i] != 0);
        if (b < 0 || b >= e->B || ns[i] < 0 || (size_t)ns[i] > q3_voc_pcm_stride(e) || (size_t)nv > e->tp_stride)
            return q3_set_err(e, Q3TTS_ERR_STATE, "speed: a slot's PCM exceeds its tempo row");
        if (kt <= e->tp_done[b]) continue;
        pk.e[n++] = Q3TempoEnt{b, ns[i], e->tp_done[b], (int32_t)kt, (int32_t)nv, 0};
        e->tp_done[b] = (int)kt;
        if (n == Q3_PCM_MAX_ENT) flush();
    }
    if (n) flush();
    Q3_HIP(e, hipGetLastError());
    return Q3TTS_OK;
}

extern "C" int q3tts_set_speed(q3tts_engine* e, int32_t permille) {
    if (!e) return q3_set_err(nullptr, Q3TTS_ERR_INVALID, "null engine");
    Q3_NOT_IN_SESSION(e);
    if (e->streams_open > 0) return q3_set_err(e, Q3TTS_ERR_STATE, "a stream is open on this engine (q3tts_stream_end first)");
    const int want = (permille == 0 || permille == 1000) ? 0 : permille;
    if (want && (want < Q3_TEMPO_MIN || want > Q3_TEMPO_MAX)) return q3_set_err(e, Q3TTS_ERR_INVALID, "speed: 0 or 1000 (off), or 500..2000 per mille");
    if (want && !e->voc) return q3_set_err(e, Q3TTS_ERR_INVALID, "a speed needs with_vocoder = 1");
    if (want && e->dev_pcm_on) return q3_set_err(e, Q3TTS_ERR_STATE, "device-resident PCM is unstretched (q3tts_set_device_pcm(engine, 0) first)");
    if (want == e->speed) return Q3TTS_OK;
    Q3_HIP(e, hipSetDevice(e->cfg.device));
    Q3_HIP(e, hipStreamSynchronize(e->vstream));
    Q3_HIP(e, hipStreamSynchronize(e->stream));
    const int was = e->speed; const size_t was_stride = e->tp_stride;
    if (want) {
        if (!e->tp_win) {  // engine lifetime: the window and the slots' p
            std::vector<float> w;
            q3_tempo_window(w);
            float* dw = nullptr; long long* dp = nullptr;
            TRY(q3_dalloc(e, &dw, w.size()));
            TRY(q3_dalloc(e, &dp, (size_t)e->B));
            Q3_HIP(e, hipMemcpy(dw, w.data(), sizeof(float) * w.size(), hipMemcpyHostToDevice));
            e->tp_win = dw; e->tp_last = dp;
        }
        // a row holds what the slowest use of this speed makes of a whole vocoder row, in whole frames
        const size_t stride = (size_t)q3_tempo_frames((long long)q3_voc_pcm_stride(e), want, true) * Hs + 4;
        if (e->tp_cap < stride * (size_t)e->B) {  // regrows with the speed: its own hipMalloc / hipFree pair
            const size_t bytes = stride * (size_t)e->B * sizeof(float);
            size_t free_b = 0, total_b = 0;
            Q3_HIP(e, hipMemGetInfo(&free_b, &total_b));
            const size_t back = e->tp_cap * sizeof(float);  // (the old rows go first)
            void* p = nullptr;
            if (bytes > free_b + back || hipMalloc(&p, bytes) != hipSuccess) {
                (void)hipGetLastError();
                return q3_set_err(e, Q3TTS_ERR_OOM, "speed: the tempo rows need " + std::to_string(bytes) + " bytes, the device has " + std::to_string(free_b + back) + " bytes free");
            }
            if (e->tp_row) hipFree(e->tp_row);
            e->tp_row = (float*)p; e->tp_cap = stride * (size_t)e->B;
        }
        e->tp_stride = stride;
    }
    e->speed = want;
    e->tp_done.assign((size_t)e->B, 0);
    if (e->out_rate) {  // the resampler's staging rows follow the rows it reads
        size_t st = 0;
        const int rc = q3_rs_stage_fit(e, e->rs_out, &st);
        if (rc != Q3TTS_OK) { e->speed = was; e->tp_stride = was_stride; return rc; }
        e->rs_stage_stride = st;
    }
    return Q3TTS_OK;
}

extern "C" int q3tts_get_speed(const q3tts_engine* e, int32_t* permille) {
    if (!e || !permille) return q3_set_err(nullptr, Q3TTS_ERR_INVALID, "null argument");
    *permille = e->speed;
    return Q3TTS_OK;
}

namespace {
struct Tmp {  // a device buffer of one call
    void* p = nullptr;
    ~Tmp() { if (p) hipFree(p); }
};
}  // namespace

extern "C" int q3tts_time_stretch(q3tts_engine* e, const float* in, int64_t n_in, int32_t permille, float* out, int64_t cap, int64_t* n_out) {
    if (!e || !n_out || n_in < 0 || (n_in > 0 && !in) || cap < 0 || (cap > 0 && !out)) return q3_set_err(e, Q3TTS_ERR_INVALID, "time stretch: null argument or negative length");
    Q3_NOT_IN_SESSION(e);
    return q3_time_stretch_run(e, in, n_in, permille, out, cap, n_out);
}
void q3_time_stretch_dev(const float* src, long long n_in, int permille, float* dst, const float* win, long long* p_last, hipStream_t s) {
    const long long N = q3_tempo_N(n_in, permille);
    Q3TempoPack pk{};
    pk.e[0] = Q3TempoEnt{0, (int32_t)n_in, 0, (int32_t)q3_tempo_frames(n_in, permille, true), (int32_t)N, 0};
    q3_launch_pcm_tempo(src, (size_t)n_in, dst, (size_t)N, p_last, win, permille, pk, 1, nullptr, 0, s);
}
int q3_time_stretch_run(q3tts_engine* e, const float* in, int64_t n_in, int32_t permille, float* out, int64_t cap, int64_t* n_out) {
    if (permille < Q3_TEMPO_MIN || permille > Q3_TEMPO_MAX || permille == 1000) return q3_set_err(e, Q3TTS_ERR_INVALID, "time stretch: 500..2000 per mille, and not 1000");
    if (n_in > (1ll << 28)) return q3_set_err(e, Q3TTS_ERR_INVALID, "time stretch: more than 2^28 input samples");
    Q3_HIP(e, hipSetDevice(e->cfg.device));
    const long long N = q3_tempo_N(n_in, permille);
    *n_out = N;
    if (cap < N) return q3_set_err(e, Q3TTS_ERR_INVALID, "time stretch: out holds fewer than ceil(n_in * 1000 / permille) samples (*n_out says how many)");
    if (N == 0) return Q3TTS_OK;
    std::vector<float> w;
    q3_tempo_window(w);
    Tmp src, dst, win, pl;
    if (hipMalloc(&src.p, sizeof(float) * (size_t)n_in) != hipSuccess || hipMalloc(&dst.p, sizeof(float) * (size_t)N) != hipSuccess ||
        hipMalloc(&win.p, sizeof(float) * w.size()) != hipSuccess || hipMalloc(&pl.p, sizeof(long long)) != hipSuccess)
        return q3_set_err(e, Q3TTS_ERR_OOM, "hipMalloc (time stretch)");
    hipStream_t s = e->stream;
    Q3_HIP(e, hipMemcpyAsync(src.p, in, sizeof(float) * (size_t)n_in, hipMemcpyHostToDevice, s));
    Q3_HIP(e, hipMemcpyAsync(win.p, w.data(), sizeof(float) * w.size(), hipMemcpyHostToDevice, s));
    q3_time_stretch_dev((const float*)src.p, n_in, permille, (float*)dst.p, (const float*)win.p, (long long*)pl.p, s);
    Q3_HIP(e, hipGetLastError());
    Q3_HIP(e, hipMemcpyAsync(out, dst.p, sizeof(float) * (size_t)N, hipMemcpyDeviceToHost, s));
    Q3_HIP(e, hipStreamSynchronize(s));  // (w outlives the upload)
    return Q3TTS_OK;
}

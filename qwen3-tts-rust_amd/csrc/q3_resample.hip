// q3_resample.hip — the device resampler: rational polyphase, Kaiser-windowed sinc. One coefficient table per
// (rate_in, rate_out), one kernel (k_pcm_resample, the sibling of k_pcm_pack: same entry list, output rate instead of a copy), and the
// engine calls built on it: q3tts_set_output_rate / q3tts_get_output_rate / q3tts_resample. The reference has no counterpart: it emits
// 24 kHz only and refuses clone clips at any other rate (src/tts/engine.rs:341).
#include "q3_engine.h"

#include <cmath>
#include <numeric>

// ---- the filter (host, double; rounded once to f32) ---------------------------------------------------------------------------
namespace {
constexpr double kRho = 0.93, kZeros = 32.0, kBeta = 9.0, kPi = 3.14159265358979323846;
constexpr int kOut = 256;  // outputs per tile = threads per workgroup: one T-tap chain per thread

double bessel_i0(double x) {  // sum_j ((x/2)^j / j!)^2: every term positive, converged to the last bit well before j = 64 for x <= 9
    const double q = 0.25 * x * x;
    double term = 1.0, sum = 1.0;
    for (int j = 1; j < 64; ++j) { term *= q / ((double)j * (double)j); sum += term; }
    return sum;
}
}  // namespace

int q3_resample_plan(int rate_in, int rate_out, int* L, int* M, int* H, int* T) {
    if (rate_in < 4000 || rate_in > 96000 || rate_out < 4000 || rate_out > 96000 || rate_in == rate_out) return Q3TTS_ERR_INVALID;
    const int g = std::gcd(rate_in, rate_out);
    *L = rate_out / g; *M = rate_in / g;
    const double c = kRho * std::min(1.0, (double)*L / (double)*M), W = kZeros / c;
    *H = (int)std::ceil(W); *T = 2 * *H + 1;
    if ((long long)*L * *T > Q3_RESAMPLE_MAX_COEF) return Q3TTS_ERR_UNSUPPORTED;
    return Q3TTS_OK;
}

int q3_resample_table(int rate_in, int rate_out, int* L, int* M, int* H, std::vector<float>& tab) {
    int T = 0;
    TRY(q3_resample_plan(rate_in, rate_out, L, M, H, &T));
    const double c = kRho * std::min(1.0, (double)*L / (double)*M), W = kZeros / c, i0b = bessel_i0(kBeta);
    tab.assign((size_t)*L * T, 0.0f);
    for (int p = 0; p < *L; ++p)
        for (int k = 0; k < T; ++k) {
            const double d = (double)(*H - k) + (double)p / (double)*L;
            if (std::fabs(d) > W) continue;
            const double x = c * d, r = d / W;
            const double sinc = x == 0.0 ? 1.0 : std::sin(kPi * x) / (kPi * x);
            tab[(size_t)p * T + k] = (float)(c * sinc * bessel_i0(kBeta * std::sqrt(std::max(0.0, 1.0 - r * r))) / i0b);
        }
    return Q3TTS_OK;
}

// tab[p][k] -> the kernel's layout [k][q], q = m mod L of the output m that uses phase p = (m M) mod L (p = (q M) mod L: M is invertible
// mod L). Consecutive outputs then read consecutive words of a tap's row, whatever M is.
std::vector<float> q3_resample_device_layout(const std::vector<float>& tab, int L, int M, int T) {
    std::vector<float> d((size_t)L * T);
    for (int q = 0; q < L; ++q) {
        const int p = (int)(((long long)q * M) % L);
        for (int k = 0; k < T; ++k) d[(size_t)k * L + q] = tab[(size_t)p * T + k];
    }
    return d;
}

long long q3_resample_N(long long n, int L, int M) { return n <= 0 ? 0 : (n * L + M - 1) / M; }
long long q3_resample_D(long long n, int L, int M, int H) { return n <= H ? 0 : ((n - H) * L + M - 1) / M; }

// ---- the kernel ---------------------------------------------------------------------------------------------------------------
// grid (x, n_ent): blockIdx.y = entry, a workgroup walks the entry's 256-output tiles blockIdx.x, + gridDim.x, ... For a tile it stages
// the input span the tile's windows cover in LDS — whole aligned float4 groups of the source row with one 16-byte load, the groups that
// straddle 0 or the row's valid length n element by element, zeros outside [0, n): nothing past n is ever loaded — and then every thread
// runs the T-tap chain of one output, in ascending k, one f32 multiply and one f32 add per tap (the canonical order of DESIGN.md §19).
// LDS: [span_cap floats][the table, when tab_lds]. Outputs past what the row can deliver (N(n) when final, D(n) otherwise) are not written.
// The body is shared by two addressings. Ring = false: the row is linear (k_pcm_resample, as ever). Ring = true (k_doc_resample,
// DESIGN.md §28): the row is a ring of C samples that holds position g at g mod C, its base 16-byte aligned (a == 0) and C a multiple of
// 4, so an aligned group of four never crosses the wrap; its positions stay below 2^29 (J below 2^28, stretched at speed 500 at the
// most), so the modulus is an unsigned 32-bit one.
template <bool Ring>
__device__ __forceinline__ long long rs_at(long long g, unsigned C) { return Ring ? (long long)((unsigned)g % C) : g; }

// outputs [first, first + count) of one row (n valid samples, finished or not) to d[0, ...): the workgroups blockIdx.x, + gridDim.x, ...
template <bool Ring, typename T>
__device__ __forceinline__ void rs_tiles(const float* __restrict__ row, int a, unsigned C, long long n, bool fin, long long first, long long count,
                                         T* __restrict__ d, const Q3Resamp& rs, int span_cap, int tab_lds) {
    extern __shared__ float4 q3_rs_lds[];
    float* xs = (float*)q3_rs_lds;
    const long long L = rs.L, M = rs.M;
    const int H = rs.H, nt = rs.T, tid = threadIdx.x;
    const long long lim = fin ? (n <= 0 ? 0 : (n * L + M - 1) / M) : (n <= H ? 0 : ((n - H) * L + M - 1) / M);
    const long long cnt = min(count, lim - first);
    if (first < 0 || cnt <= 0) return;  // (uniform over the workgroup, as every exit below)
    const int ntiles = (int)((cnt + kOut - 1) / kOut);
    if ((int)blockIdx.x >= ntiles) return;
    const float* tab = rs.tab;
    if (tab_lds) {
        float* ts = xs + span_cap;
        const int lt = rs.L * nt, lt4 = lt >> 2;
        const float4* t4 = (const float4*)rs.tab;  // (16-byte aligned: an allocation of its own, or a document's table behind its window)
        for (int j = tid; j < lt4; j += kOut) ((float4*)ts)[j] = t4[j];
        for (int j = 4 * lt4 + tid; j < lt; j += kOut) ts[j] = rs.tab[j];
        tab = ts;
    }
    for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const long long m0 = first + (long long)tile * kOut;
        const int c = (int)min((long long)kOut, cnt - (long long)tile * kOut);
        const long long i0 = (m0 * M) / L, i1 = ((m0 + c - 1) * M) / L;
        const long long g0 = i0 - H;                                   // the first sample a window of this tile reads
        const long long gs = g0 - ((((long long)a + g0) % 4 + 4) % 4);  // moved down to a 16-byte boundary of the source row
        const int n4 = (int)((i1 + H - gs + 4) >> 2);                  // float4 groups up to the last sample read, i1 + H
        __syncthreads();  // the previous tile's chains are done with xs
        for (int j = tid; j < n4; j += kOut) {
            const long long g = gs + 4ll * j;
            float4 v;
            if (g >= 0 && g + 4 <= n) v = *(const float4*)(row + rs_at<Ring>(g, C));
            else {
                v.x = (g >= 0 && g < n) ? row[rs_at<Ring>(g, C)] : 0.0f;
                v.y = (g + 1 >= 0 && g + 1 < n) ? row[rs_at<Ring>(g + 1, C)] : 0.0f;
                v.z = (g + 2 >= 0 && g + 2 < n) ? row[rs_at<Ring>(g + 2, C)] : 0.0f;
                v.w = (g + 3 >= 0 && g + 3 < n) ? row[rs_at<Ring>(g + 3, C)] : 0.0f;
            }
            q3_rs_lds[j] = v;
        }
        __syncthreads();
        if (tid < c) {
            const long long m = m0 + tid, i = (m * M) / L;
            const float* x = xs + (int)(i - H - gs);
            const float* t = tab + (int)(m % L);
            float acc = 0.0f;
#pragma unroll 4
            for (int k = 0; k < nt; ++k) acc = __fadd_rn(acc, __fmul_rn(x[k], t[(size_t)k * rs.L]));
            q3_pcm_put(d + (m - first), acc);
        }
    }
}

template <typename T>
__global__ __launch_bounds__(kOut) void k_pcm_resample(const float* __restrict__ src, size_t stride, const Q3PcmPack ents, const Q3PcmSrc rows,
                                                       const Q3Resamp rs, int span_cap, int tab_lds, T* __restrict__ dst) {
    const Q3PcmEnt en = ents.e[blockIdx.y];
    const float* row = src + (size_t)en.row * stride;
    rs_tiles<false, T>(row, (int)(((uintptr_t)row >> 2) & 3), 0u, rows.len[blockIdx.y], (rows.final_mask >> blockIdx.y) & 1ull, en.first, en.count,
                       dst + en.dst_off, rs, span_cap, tab_lds);
}

// grid (x): the ring form, one document. Outputs [first, first + count) of the audio of which ring (C samples, position g at g mod C)
// holds the last C of the n there are so far (fin: all there will be) into dst[dst_off, ...). The host guarantees that every position an
// output reads is still in the ring (q3_doc_ring_step); nothing at or past n is loaded.
template <typename T>
__global__ __launch_bounds__(kOut) void k_doc_resample(const float* __restrict__ ring, unsigned C, long long n, int fin, long long first, long long count,
                                                       const Q3Resamp rs, int span_cap, int tab_lds, T* __restrict__ dst, long long dst_off) {
    rs_tiles<true, T>(ring, 0, C, n, fin != 0, first, count, dst + dst_off, rs, span_cap, tab_lds);
}

namespace {
// the LDS of a launch: one tile's span, and the table when it fits beside it. false: the span alone does not fit
bool rs_launch_shape(const Q3Resamp& rs, long long* span, int* tab_lds, size_t* lds, long long* lt4) {
    // a tile's span: (kOut - 1) M / L + 1 input steps between its first and last output, T taps, up to 3 samples of alignment, whole float4s
    *span = (((long long)(kOut - 1) * rs.M) / rs.L + 1 + rs.T + 3 + 3) & ~3ll;
    *lt4 = ((long long)rs.L * rs.T + 3) & ~3ll;
    if (*span * 4 > Q3_RESAMPLE_LDS_BYTES) return false;
    *tab_lds = (*span + *lt4) * 4 <= Q3_RESAMPLE_LDS_BYTES ? 1 : 0;
    *lds = (size_t)(*tab_lds ? *span + *lt4 : *span) * 4;
    return true;
}
}  // namespace

int q3_launch_pcm_resample(const float* src, size_t stride, const Q3PcmPack& ents, const Q3PcmSrc& rows, int n_ent, int max_count, const Q3Resamp& rs,
                           int i16, void* dst, hipStream_t s) {
    if (n_ent <= 0 || max_count <= 0) return 0;
    long long span, lt4; int tab_lds; size_t lds;
    if (!rs_launch_shape(rs, &span, &tab_lds, &lds, &lt4)) return -1;
    const int tiles = (max_count + kOut - 1) / kOut;
    int gx = std::min(tiles, std::max(1, 1024 / n_ent));
    if (tab_lds && lt4 > 2048) gx = std::min(gx, (tiles + 3) / 4);  // a large table's copy is spread over four tiles or more
    gx = std::max(gx, 1);
    if (i16) hipLaunchKernelGGL(k_pcm_resample<int16_t>, dim3(gx, n_ent), dim3(kOut), lds, s, src, stride, ents, rows, rs, (int)span, tab_lds, (int16_t*)dst);
    else hipLaunchKernelGGL(k_pcm_resample<float>, dim3(gx, n_ent), dim3(kOut), lds, s, src, stride, ents, rows, rs, (int)span, tab_lds, (float*)dst);
    return 0;
}

int q3_launch_doc_resample(const float* ring, long long C, long long n, bool fin, long long first, long long count, const Q3Resamp& rs, int i16,
                           void* dst, long long dst_off, hipStream_t s) {
    if (count <= 0) return 0;
    long long span, lt4; int tab_lds; size_t lds;
    if (!rs_launch_shape(rs, &span, &tab_lds, &lds, &lt4)) return -1;
    const int tiles = (int)((count + kOut - 1) / kOut);
    int gx = std::min(tiles, 1024);
    if (tab_lds && lt4 > 2048) gx = std::min(gx, (tiles + 3) / 4);
    gx = std::max(gx, 1);
    if (i16) hipLaunchKernelGGL(k_doc_resample<int16_t>, dim3(gx), dim3(kOut), lds, s, ring, (unsigned)C, n, fin ? 1 : 0, first, count, rs, (int)span, tab_lds, (int16_t*)dst, dst_off);
    else hipLaunchKernelGGL(k_doc_resample<float>, dim3(gx), dim3(kOut), lds, s, ring, (unsigned)C, n, fin ? 1 : 0, first, count, rs, (int)span, tab_lds, (float*)dst, dst_off);
    return 0;
}

// ---- engine state -------------------------------------------------------------------------------------------------------------
// the table of a rate pair: built and uploaded the first time the pair is asked for, kept for the engine's life (e->allocs)
int q3_resample_get(q3tts_engine* e, int rate_in, int rate_out, Q3Resamp* out) {
    for (const Q3Resamp& r : e->rs_cache)
        if (r.rate_in == rate_in && r.rate_out == rate_out) { *out = r; return Q3TTS_OK; }
    Q3Resamp r{};
    std::vector<float> tab;
    const int rc = q3_resample_table(rate_in, rate_out, &r.L, &r.M, &r.H, tab);
    if (rc == Q3TTS_ERR_UNSUPPORTED) return q3_set_err(e, rc, "resample: this rate pair needs more than 32768 filter coefficients");
    if (rc != Q3TTS_OK) return q3_set_err(e, rc, "resample: rates must lie in 4000..96000 Hz and differ");
    if (e->rs_cache.size() >= 64) return q3_set_err(e, Q3TTS_ERR_UNSUPPORTED, "resample: more than 64 distinct rate pairs on one engine");
    r.rate_in = rate_in; r.rate_out = rate_out; r.T = 2 * r.H + 1;
    const std::vector<float> dl = q3_resample_device_layout(tab, r.L, r.M, r.T);
    float* dev = nullptr;
    TRY(q3_dalloc(e, &dev, dl.size()));
    Q3_HIP(e, hipMemcpy(dev, dl.data(), sizeof(float) * dl.size(), hipMemcpyHostToDevice));
    r.tab = dev;
    e->rs_cache.push_back(r);
    *out = r;
    return Q3TTS_OK;
}

// outputs [first_out, first_out + count) of slot b's PCM row (n_valid samples so far, final or not) at the engine's output rate, f32,
// into the start of the slot's staging row
int q3_resample_slot(q3tts_engine* e, int b, long long first_out, int count, int n_valid, bool is_final, hipStream_t s) {
    if (count <= 0) return Q3TTS_OK;
    if ((size_t)count > e->rs_stage_stride) return q3_set_err(e, Q3TTS_ERR_STATE, "resample: a window exceeds the staging row");
    Q3PcmPack pk{}; Q3PcmSrc rows{};
    pk.e[0] = Q3PcmEnt{b, (int32_t)first_out, count, 0, (long long)((size_t)b * e->rs_stage_stride)};
    rows.len[0] = n_valid; rows.final_mask = is_final ? 1ull : 0ull;
    if (q3_launch_pcm_resample(q3_pcm_rows(e), q3_pcm_rows_stride(e), pk, rows, 1, count, e->rs_out, 0, e->rs_stage, s) != 0)
        return q3_set_err(e, Q3TTS_ERR_UNSUPPORTED, "resample: the input span of one tile does not fit the LDS");
    Q3_HIP(e, hipGetLastError());
    return Q3TTS_OK;
}

// the staging rows for rs over the rows the PCM exits read (the vocoder's, or the tempo rows when a speed is set)
int q3_rs_stage_fit(q3tts_engine* e, const Q3Resamp& rs, size_t* stride_out) {
    const size_t stride = ((size_t)q3_resample_N((long long)q3_pcm_rows_stride(e), rs.L, rs.M) + 3) & ~(size_t)3;
    if (e->rs_stage_cap < stride * (size_t)e->B) {  // regrows with the rate: its own hipMalloc / hipFree pair
        Q3_HIP(e, hipStreamSynchronize(e->vstream));
        Q3_HIP(e, hipStreamSynchronize(e->stream));
        if (e->rs_stage) { hipFree(e->rs_stage); e->rs_stage = nullptr; e->rs_stage_cap = 0; }
        void* p = nullptr;
        if (hipMalloc(&p, stride * (size_t)e->B * sizeof(float)) != hipSuccess) return q3_set_err(e, Q3TTS_ERR_OOM, "hipMalloc (resampler staging)");
        e->rs_stage = (float*)p; e->rs_stage_cap = stride * (size_t)e->B;
    }
    *stride_out = stride;
    return Q3TTS_OK;
}

extern "C" int q3tts_set_output_rate(q3tts_engine* e, int32_t rate) {
    if (!e) return q3_set_err(nullptr, Q3TTS_ERR_INVALID, "null engine");
    Q3_NOT_IN_SESSION(e);
    if (e->streams_open > 0) return q3_set_err(e, Q3TTS_ERR_STATE, "a stream is open on this engine (q3tts_stream_end first)");
    const int native = e->cfg.vocoder.sample_rate;
    if (rate == 0 || rate == native) { e->out_rate = 0; return Q3TTS_OK; }
    if (rate < 4000 || rate > 96000) return q3_set_err(e, Q3TTS_ERR_INVALID, "output rate: 0 (off) or 4000..96000 Hz");
    if (!e->voc) return q3_set_err(e, Q3TTS_ERR_STATE, "an output rate needs with_vocoder = 1");
    if (e->dev_pcm_on) return q3_set_err(e, Q3TTS_ERR_STATE, "device-resident PCM is native-rate only (q3tts_set_device_pcm(engine, 0) first)");
    Q3_HIP(e, hipSetDevice(e->cfg.device));
    Q3Resamp rs{};
    TRY(q3_resample_get(e, native, rate, &rs));
    size_t stride = 0;
    TRY(q3_rs_stage_fit(e, rs, &stride));
    e->rs_stage_stride = stride; e->rs_out = rs; e->out_rate = rate;
    return Q3TTS_OK;
}

extern "C" int q3tts_get_output_rate(const q3tts_engine* e, int32_t* rate) {
    if (!e || !rate) return q3_set_err(nullptr, Q3TTS_ERR_INVALID, "null argument");
    *rate = e->out_rate;
    return Q3TTS_OK;
}

namespace {
struct Tmp {  // a device buffer of one call
    void* p = nullptr;
    ~Tmp() { if (p) hipFree(p); }
};
}  // namespace

extern "C" int q3tts_resample(q3tts_engine* e, const float* in, int64_t n_in, int32_t rate_in, int32_t rate_out, float* out, int64_t cap, int64_t* n_out) {
    if (!e || !n_out || n_in < 0 || (n_in > 0 && !in) || cap < 0 || (cap > 0 && !out)) return q3_set_err(e, Q3TTS_ERR_INVALID, "resample: null argument or negative length");
    Q3_NOT_IN_SESSION(e);
    return q3_resample_run(e, in, n_in, rate_in, rate_out, out, cap, n_out);
}
int q3_resample_dev(const float* src, long long n_in, const Q3Resamp& rs, float* dst, hipStream_t s) {
    const long long N = q3_resample_N(n_in, rs.L, rs.M);
    Q3PcmPack pk{}; Q3PcmSrc rows{};
    pk.e[0] = Q3PcmEnt{0, 0, (int32_t)N, 0, 0};
    rows.len[0] = (int32_t)n_in; rows.final_mask = 1ull;
    return q3_launch_pcm_resample(src, (size_t)n_in, pk, rows, 1, (int)N, rs, 0, dst, s);
}
int q3_resample_run(q3tts_engine* e, const float* in, int64_t n_in, int32_t rate_in, int32_t rate_out, float* out, int64_t cap, int64_t* n_out) {
    Q3_HIP(e, hipSetDevice(e->cfg.device));
    Q3Resamp rs{};
    TRY(q3_resample_get(e, rate_in, rate_out, &rs));
    if (n_in > (1ll << 28)) return q3_set_err(e, Q3TTS_ERR_INVALID, "resample: more than 2^28 input samples");
    const long long N = q3_resample_N(n_in, rs.L, rs.M);
    *n_out = N;
    if (N > 0x7fffffffll) return q3_set_err(e, Q3TTS_ERR_INVALID, "resample: the output does not fit 2^31 samples");
    if (cap < N) return q3_set_err(e, Q3TTS_ERR_INVALID, "resample: out holds fewer than ceil(n_in * L / M) samples (*n_out says how many)");
    if (N == 0) return Q3TTS_OK;
    Tmp src, dst;
    if (hipMalloc(&src.p, sizeof(float) * (size_t)n_in) != hipSuccess || hipMalloc(&dst.p, sizeof(float) * (size_t)N) != hipSuccess)
        return q3_set_err(e, Q3TTS_ERR_OOM, "hipMalloc (resample)");
    hipStream_t s = e->stream;
    Q3_HIP(e, hipMemcpyAsync(src.p, in, sizeof(float) * (size_t)n_in, hipMemcpyHostToDevice, s));
    if (q3_resample_dev((const float*)src.p, n_in, rs, (float*)dst.p, s) != 0)
        return q3_set_err(e, Q3TTS_ERR_UNSUPPORTED, "resample: the input span of one tile does not fit the LDS");
    Q3_HIP(e, hipGetLastError());
    Q3_HIP(e, hipMemcpyAsync(out, dst.p, sizeof(float) * (size_t)N, hipMemcpyDeviceToHost, s));
    Q3_HIP(e, hipStreamSynchronize(s));
    return Q3TTS_OK;
}

// q3_kernels.hip — hand-written gfx950 (CDNA4) kernels of the Qwen3-TTS codec-token decoder.
//
// Numerics contract: every reduction has ONE canonical order that the CPU oracle restates.
//  * GEMM: v_mfma_f32_16x16x4_f32 (f32 in / f32 accumulate) is bit-for-bit a k-ordered fmaf chain
//    (measured: tools/probe_mfma.hip, 0/256 mismatches at K=2048), so the 8-slice / (t, kq) order below is exact.
//  * norms / softmax: 64-lane butterflies (xor 32,16,8,4,2,1) over per-lane sequential partials.
// Built with -ffp-contract=off: every fused multiply-add is an explicit fmaf.
#include "q3_kernels.h"

// (the exact GEMM lives in q3_gemm.hip, attention in q3_attend.hip)

// ---------------------------------------------------------------------------------------------------
// weight / table initialisation
// ---------------------------------------------------------------------------------------------------
__global__ void k_fill_tiled(Q3Fill f, int nb0, int nb_count) {
    const size_t gid = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int kblocks = f.K >> 5;
    const size_t total = (size_t)nb_count * kblocks * 64;
    if (gid >= total) return;
    const int lane = (int)(gid & 63);
    const size_t t = gid >> 6;
    const int kb = (int)(t % kblocks), nb = nb0 + (int)(t / kblocks);
    const int n = nb * 16 + (lane & 15), k0 = kb * 32 + (lane >> 4) * 4;  // element e <-> k = k0 + (e/4)*16 + (e%4)
    uint32_t tid; int lr; const uint16_t* src;
    if (f.mode == 0) { tid = f.tid_a; lr = n - f.row0; src = f.src_a; }
    else {
        const int tile = n >> 4, c = n & 15;
        if (c < 8) { tid = f.tid_a; lr = tile * 8 + c; src = f.src_a; }
        else { tid = f.tid_b; lr = tile * 8 + c - 8; src = f.src_b; }
    }
    uint16_t h[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const size_t idx = (size_t)lr * f.K + k0 + (e >> 2) * 16 + (e & 3);
        h[e] = src ? src[idx] : q3_bf16(q3_synth(f.seed, tid, idx, f.scale));
    }
    uint4 v;
    v.x = (uint32_t)h[0] | ((uint32_t)h[1] << 16); v.y = (uint32_t)h[2] | ((uint32_t)h[3] << 16);
    v.z = (uint32_t)h[4] | ((uint32_t)h[5] << 16); v.w = (uint32_t)h[6] | ((uint32_t)h[7] << 16);
    f.dst[((size_t)nb * kblocks + kb) * 64 + lane] = v;
}
void q3_launch_fill_tiled(const Q3Fill& f, hipStream_t s) {
    int nb0, nbc;
    if (f.mode == 0) { nb0 = f.row0 / 16; nbc = f.rows / 16; } else { nb0 = 0; nbc = f.N / 16; }
    const size_t total = (size_t)nbc * (f.K >> 5) * 64;
    hipLaunchKernelGGL(k_fill_tiled, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, f, nb0, nbc);
}
// The same matrices as ggml Q8_0 blocks in the tiled Q8 layout (q3_kernels.h): one thread per (column tile, k-block pair, lane) = 16 output
// bytes. A thread needs the scale of both of its blocks, i.e. the largest magnitude of all 32 weights of each: it re-reads them (8 x
// redundant: load-time only). Quantiser = ggml's quantize_row_q8_0_ref: d = amax / 127, id = d ? 1 / d : 0, q = roundf(x * id), d kept as f16.
__global__ void k_fill_tiled_q8(Q3Fill f, int nb0, int nb_count) {
    const size_t gid = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int kpairs = f.K >> 6, kblocks = f.K >> 5;
    const size_t total = (size_t)nb_count * kpairs * 64;
    if (gid >= total) return;
    const int lane = (int)(gid & 63);
    const size_t t = gid >> 6;
    const int kp = (int)(t % kpairs), nb = nb0 + (int)(t / kpairs);
    const int n = nb * 16 + (lane & 15), kq = lane >> 4;
    uint32_t tid; int lr; const uint16_t* src; const uint8_t* src8;
    if (f.mode == 0) { tid = f.tid_a; lr = n - f.row0; src = f.src_a; src8 = f.src8_a; }
    else {
        const int tile = n >> 4, c = n & 15;
        if (c < 8) { tid = f.tid_a; lr = tile * 8 + c; src = f.src_a; src8 = f.src8_a; }
        else { tid = f.tid_b; lr = tile * 8 + c - 8; src = f.src_b; src8 = f.src8_b; }
    }
    uint32_t out[4];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int kb = 2 * kp + h;
        int8_t q[8]; uint16_t d16;
        if (src8) {  // a block_q8_0 as stored: f16 d, 32 x int8
            const uint8_t* blk = src8 + ((size_t)lr * kblocks + kb) * 34;
            d16 = (uint16_t)blk[0] | ((uint16_t)blk[1] << 8);
#pragma unroll
            for (int e = 0; e < 8; ++e) q[e] = (int8_t)blk[2 + (e >> 2) * 16 + kq * 4 + (e & 3)];
        } else {
            float amax = 0.0f, mine[8];
            for (int k = 0; k < 32; ++k) {
                const size_t idx = (size_t)lr * f.K + (size_t)kb * 32 + k;
                const float v = src ? q3_bf16f(src[idx]) : q3_round_bf16(q3_synth(f.seed, tid, idx, f.scale));
                amax = fmaxf(amax, fabsf(v));
                const int kk = k & 15;
                if ((kk >> 2) == kq) mine[((k >> 4) << 2) + (kk & 3)] = v;
            }
            const float d = amax / 127.0f, id = d != 0.0f ? 1.0f / d : 0.0f;
            d16 = __builtin_bit_cast(unsigned short, (_Float16)d);
#pragma unroll
            for (int e = 0; e < 8; ++e) q[e] = (int8_t)(int)roundf(mine[e] * id);
        }
        out[2 * h] = (uint32_t)(uint8_t)q[0] | ((uint32_t)(uint8_t)q[1] << 8) | ((uint32_t)(uint8_t)q[2] << 16) | ((uint32_t)(uint8_t)q[3] << 24);
        out[2 * h + 1] = (uint32_t)(uint8_t)q[4] | ((uint32_t)(uint8_t)q[5] << 8) | ((uint32_t)(uint8_t)q[6] << 16) | ((uint32_t)(uint8_t)q[7] << 24);
        if (kq == 0) f.dst_scale[(size_t)n * kblocks + kb] = d16;
    }
    f.dst[((size_t)nb * kpairs + kp) * 64 + lane] = make_uint4(out[0], out[1], out[2], out[3]);
}
void q3_launch_fill_tiled_q8(const Q3Fill& f, hipStream_t s) {
    int nb0, nbc;
    if (f.mode == 0) { nb0 = f.row0 / 16; nbc = f.rows / 16; } else { nb0 = 0; nbc = f.N / 16; }
    const size_t total = (size_t)nbc * (f.K >> 6) * 64;
    hipLaunchKernelGGL(k_fill_tiled_q8, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, f, nb0, nbc);
}
__global__ void k_fill_f32(float* dst, size_t n, uint64_t seed, uint32_t tid, float base, float scale, int rb) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (; i < n; i += stride) {
        float v = base + q3_synth(seed, tid, i, scale);
        dst[i] = rb ? q3_round_bf16(v) : v;
    }
}
void q3_launch_fill_f32(float* dst, size_t n, uint64_t seed, uint32_t tid, float base, float scale, int rb, hipStream_t s) {
    size_t blocks = (n + 255) / 256;
    if (blocks > 65536) blocks = 65536;
    hipLaunchKernelGGL(k_fill_f32, dim3((unsigned)blocks), dim3(256), 0, s, dst, n, seed, tid, base, scale, rb);
}

// ---------------------------------------------------------------------------------------------------
// Sampler (H4: src/models/llama/mod.rs:666-772). 256 threads; keys sorted by (logit desc, index asc) which is
// what the reference's stable descending sort of an index-ordered list produces.
// ---------------------------------------------------------------------------------------------------
#define SAMP_MAX Q3_SAMP_MAX
__device__ int sample_row(const float* logits, int limit, float temperature, int top_k_i, float top_p, float r,
                          unsigned long long* keys, float* probs) {
    const int tid = threadIdx.x;
    __shared__ unsigned long long wbest[4];
    if (temperature <= 0.0f) {  // :690-701
        unsigned long long best = 0;
        for (int i = tid; i < limit; i += 256) { const unsigned long long k = q3_argmax_key(logits[i], (uint32_t)i); best = k > best ? k : best; }
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) { const unsigned long long o = __shfl_xor(best, m); best = o > best ? o : best; }
        if ((tid & 63) == 0) wbest[tid >> 6] = best;
        __syncthreads();
        unsigned long long b = wbest[0];
        for (int w = 1; w < 4; ++w) b = wbest[w] > b ? wbest[w] : b;
        __syncthreads();
        return q3_argmax_idx(b);
    }
    bool select = top_k_i > 0 && top_k_i <= 256 && top_k_i < limit;
    if (select) {
        // top-k without k block-wide reductions (each one is a chain of cross-lane steps: 40 rounds cost ~50 us). Only the k largest
        // keys are ever read below (:711-713); keys are unique (the index is part of the key) except 0 = "not a candidate".
        //  A  every thread's 16 candidates and their maximum; the k-th largest of the 256 thread maxima, T, is a lower bound of the
        //     k-th largest key (the k thread maxima >= T are k distinct keys >= T), found by counting: rank = #{maxima > mine}
        //  B  the candidates >= T (the top k are among them; typically ~2k of the 2160) are appended to a short list
        //  C  the list is ranked by counting (#{larger}) — ranks are a permutation because keys are unique — and rank r < k lands in keys[r]
        __shared__ unsigned long long lm[256];
        __shared__ unsigned long long thr_s;
        __shared__ int n_sel;
        unsigned long long* sel = (unsigned long long*)probs;  // SAMP_MAX floats = SAMP_MAX / 2 keys
        unsigned long long loc[SAMP_MAX / 256];
        unsigned long long lmax = 0;
#pragma unroll
        for (int j = 0; j < SAMP_MAX / 256; ++j) { const int i = tid + j * 256; loc[j] = i < limit ? q3_argmax_key(logits[i], (uint32_t)i) : 0ull; lmax = loc[j] > lmax ? loc[j] : lmax; }
        lm[tid] = lmax;
        if (tid == 0) { thr_s = 0ull; n_sel = 0; }
        __syncthreads();
        int cnt = 0;
        for (int j = 0; j < 256; ++j) cnt += lm[j] > lmax ? 1 : 0;
        if (cnt == top_k_i - 1 && lmax != 0ull) thr_s = lmax;  // (stays 0 when fewer than k threads hold a candidate: then everything is listed)
        __syncthreads();
        const unsigned long long T = thr_s;
#pragma unroll
        for (int j = 0; j < SAMP_MAX / 256; ++j)
            if (loc[j] != 0ull && loc[j] >= T) { const int pos = atomicAdd(&n_sel, 1); if (pos < SAMP_MAX / 2) sel[pos] = loc[j]; }
        __syncthreads();
        const int n = n_sel;
        if (n > SAMP_MAX / 2) select = false;  // (uniform) pathological input: the list does not fit, take the full sort below
        else {
            for (int i = tid; i < top_k_i; i += 256) keys[i] = 0ull;
            __syncthreads();
            for (int i = tid; i < n; i += 256) {
                const unsigned long long mine = sel[i];
                int rank = 0;
                for (int j = 0; j < n; ++j) rank += sel[j] > mine ? 1 : 0;
                if (rank < top_k_i) keys[rank] = mine;
            }
        }
        __syncthreads();
    }
    int NP = 64;
    while (NP < limit) NP <<= 1;
    if (!select) {
    for (int i = tid; i < NP; i += 256) keys[i] = i < limit ? q3_argmax_key(logits[i], (uint32_t)i) : 0ull;
    __syncthreads();
    }
    for (int k = 2; !select && k <= NP; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = tid; i < NP; i += 256) {
                const int ixj = i ^ j;
                if (ixj > i) {
                    const unsigned long long x = keys[i], y = keys[ixj];
                    const bool desc = (i & k) == 0;
                    if (desc ? (x < y) : (x > y)) { keys[i] = y; keys[ixj] = x; }
                }
            }
            __syncthreads();
        }
    __shared__ int result;
    int n_all = limit;
    {
        const size_t top_k = (size_t)(long long)top_k_i;                 // `top_k as usize` :646
        if (top_k > 0 && top_k < (size_t)n_all) n_all = (int)top_k;      // :711-713
    }
    {   // :717-723, element-wise: evaluated by all threads; the sums below stay sequential in the reference's order
        const float max_logit = n_all > 0 ? q3_key_value(keys[0]) : 0.0f;    // :716
        for (int i = tid; i < n_all; i += 256) probs[i] = q3_expf((q3_key_value(keys[i]) - max_logit) / temperature);
    }
    __syncthreads();
    // :726-764. The reference's sums are sequential f32 adds and stay so (thread 0, in order); the divisions between them are
    // element-wise and run on all threads — one thread doing everything spent ~15 us of this kernel walking LDS five times.
    __shared__ float bc_s; __shared__ int cut_s;
    int n = n_all;
    if (tid == 0) { float sum = 0.0f; for (int i = 0; i < n; ++i) sum += probs[i]; bc_s = sum; }
    __syncthreads();
    { const float sum = bc_s; if (sum > 0.0f) for (int i = tid; i < n; i += 256) probs[i] /= sum; }     // :726-731
    __syncthreads();
    if (top_p < 1.0f) {                                                  // :734-753
        if (tid == 0) {
            float cum = 0.0f; int cutoff = n;
            for (int i = 0; i < n; ++i) { cum += probs[i]; if (cum >= top_p) { cutoff = i + 1; break; } }
            float ns = 0.0f;
            for (int i = 0; i < cutoff; ++i) ns += probs[i];
            cut_s = cutoff; bc_s = ns;
        }
        __syncthreads();
        n = cut_s;
        { const float ns = bc_s; if (ns > 0.0f) for (int i = tid; i < n; i += 256) probs[i] /= ns; }
        __syncthreads();
    }
    if (tid == 0) {
        float cum = 0.0f; int res = -1;                                  // :756-764
        for (int i = 0; i < n; ++i) { cum += probs[i]; if (r < cum) { res = q3_argmax_idx(keys[i]); break; } }
        if (res < 0) res = n > 0 ? q3_argmax_idx(keys[0]) : 0;           // :767-770
        result = res;
    }
    __syncthreads();
    const int res = result;
    __syncthreads();
    return res;
}

// H4 / H5 for row b; returns the sampled code, or -1 when the row produces no frame (inactive slot, step bound, EOS)
__device__ int sample_frame(const Q3Sample& a, int b, unsigned long long* keys, float* probs) {
    const int tid = threadIdx.x, slot = a.row_slot[b];
    Q3Slot* sl = a.slots + slot;
    if (!sl->active) return -1;
    const int step = sl->n_frames;
    if (step >= sl->max_steps) {  // loop bound: src/tts/engine.rs:545
        __syncthreads();
        if (tid == 0) sl->active = 0;
        return -1;
    }
    float* lg = a.logits + (size_t)b * a.ld;
    int code0;
    if (sl->force_eos_at >= 0 && step == sl->force_eos_at) code0 = a.eos;
    else {
        if (step < sl->min_frames && a.eos < a.limit) { if (tid == 0) lg[a.eos] = -INFINITY; }
        __syncthreads();
        const float pen = sl->rep_penalty;
        uint32_t* seen = a.seen + (size_t)slot * a.seen_words;
        if (pen != 1.0f) {  // (uniform) the codes 0 this utterance has produced so far: IEEE division, as the restatement's
            for (int i = tid; i < a.limit; i += 256)
                if ((seen[i >> 5] >> (i & 31)) & 1u) { const float v = lg[i]; lg[i] = v > 0.0f ? v / pen : v * pen; }
            __syncthreads();
        }
        const float temperature = sl->temperature;
        const float r = temperature > 0.0f ? a.rng[sl->rng_base + step] : 0.0f;
        code0 = sample_row(lg, a.limit, temperature, sl->top_k, sl->top_p, r, keys, probs);
        if (pen != 1.0f && tid == 0 && code0 >= 0 && code0 < a.limit) seen[code0 >> 5] |= 1u << (code0 & 31);
    }
    __syncthreads();
    if (tid == 0) {
        if (code0 == a.eos) { sl->hit_eos = 1; sl->active = 0; }  // :558-561
        else { a.codes[((size_t)slot * a.max_steps_cap + step) * a.ncb] = code0; sl->code0 = code0; }
    }
    return code0 == a.eos ? -1 : code0;
}
__global__ __launch_bounds__(256) void k_sample(Q3Sample a) {
    __shared__ unsigned long long keys[SAMP_MAX];
    __shared__ float probs[SAMP_MAX];
    sample_frame(a, blockIdx.x, keys, probs);
}
void q3_launch_sample(const Q3Sample& a, hipStream_t s) { hipLaunchKernelGGL(k_sample, dim3(a.B), dim3(256), 0, s, a); }

__global__ __launch_bounds__(256) void k_sample_rows(const float* logits, int ld, int limit, float temperature, int top_k,
                                                     float top_p, const float* r, int* out) {
    __shared__ unsigned long long keys[SAMP_MAX];
    __shared__ float probs[SAMP_MAX];
    const int b = blockIdx.x;
    const int id = sample_row(logits + (size_t)b * ld, limit, temperature, top_k, top_p, r ? r[b] : 0.0f, keys, probs);
    if (threadIdx.x == 0) out[b] = id;
}
void q3_launch_sample_rows(const float* logits, int n, int ld, int limit, float temperature, int top_k, float top_p,
                           const float* r, int* out, hipStream_t s) {
    hipLaunchKernelGGL(k_sample_rows, dim3(n), dim3(256), 0, s, logits, ld, limit, temperature, top_k, top_p, r, out);
}

// ---------------------------------------------------------------------------------------------------
// Predictor glue (H6/H7: src/tts/engine.rs:565-631)
// ---------------------------------------------------------------------------------------------------
__device__ void pred_input_row(const Q3PredInput& a, int b, int code0) {
    __shared__ float rinv_s;
    const int tid = threadIdx.x, d = a.d;
    const float* x = a.xT + (size_t)b * d;
    const bool wantX = a.X != nullptr;  // (uniform) the frame step normalises inside the projection tile instead
    if (wantX && tid < 64) {
        float acc = 0.0f;
        for (int c = tid; c < (d >> 2); c += 64) {
            const float4 v = ((const float4*)x)[c];
            acc = fmaf(v.x, v.x, acc); acc = fmaf(v.y, v.y, acc); acc = fmaf(v.z, v.z, acc); acc = fmaf(v.w, v.w, acc);
        }
        acc = wave_sum(acc);
        if (tid == 0) rinv_s = 1.0f / sqrtf(acc / (float)d + a.eps);
    }
    __syncthreads();
    const float rinv = wantX ? rinv_s : 0.0f;
    const bool ok = code0 >= 0 && code0 < a.codec0_rows;  // OOB rows embed as zeros: src/assets_manager.rs:419-437
    const float* e = a.codec0 + (size_t)(ok ? code0 : 0) * d;
    const float* pr = ok ? a.pproj0 + (size_t)code0 * a.dp : a.proj_b;  // proj(0) = bias
    // every operand of the row is requested before anything is stored (a loop of load, store, load, store ... paid one memory round
    // trip per 256 elements: 12 in a row, ~10 us of this kernel)
    constexpr int NI = 8, NP = 4;  // d <= 8 * 256, dp <= 4 * 256 (checked at engine creation for the shipped shapes; larger: extra trips)
    for (int i0 = 0; i0 < d; i0 += NI * 256) {
        float xv[NI], nv[NI], ev[NI];
#pragma unroll
        for (int u = 0; u < NI; ++u) {
            const int i = min(i0 + tid + u * 256, d - 1);
            xv[u] = wantX ? x[i] : 0.0f; nv[u] = wantX ? a.out_norm[i] : 0.0f; ev[u] = ok ? e[i] : 0.0f;
        }
#pragma unroll
        for (int u = 0; u < NI; ++u) {
            const int i = i0 + tid + u * 256;
            if (i < d) { if (wantX) a.X[(size_t)b * d + i] = (xv[u] * rinv) * nv[u]; a.fb[(size_t)b * d + i] = 0.0f + ev[u]; }
        }
    }
    const int r1 = a.B + b;  // pass A rows: [0, B) the projected hidden rows, [B, 2B) the code rows
    for (int i0 = 0; i0 < a.dp; i0 += NP * 256) {  // (dp % 256 == 0: whole waves, 16 consecutive lanes per norm tile)
        float pv[NP], wv[NP];
#pragma unroll
        for (int u = 0; u < NP; ++u) { const int i = min(i0 + tid + u * 256, a.dp - 1); pv[u] = pr[i]; wv[u] = a.nw[i]; }
#pragma unroll
        for (int u = 0; u < NP; ++u) {
            const int i = i0 + tid + u * 256;
            if (i < a.dp) {  // (uniform per wave: dp % 256 == 0)
                a.px[(size_t)r1 * a.dp + i] = pv[u];
                if (a.xscale) q3_norm_out_q8(pv[u], wv[u], r1, i, a.dp >> 6, a.x_rt16, (int8_t*)a.xb, a.xscale, a.ssp + (size_t)r1 * (a.dp >> 4) + (i >> 4), (i & 15) == 0);
                else q3_norm_out(pv[u], wv[u], a.xb + q3_atile_off(r1, i, a.dp >> 5), a.ssp + (size_t)r1 * (a.dp >> 4) + (i >> 4), (i & 15) == 0);
            }
        }
    }
}
__global__ __launch_bounds__(256) void k_pred_input(Q3PredInput a) {
    const Q3Slot* sl = a.slots + a.row_slot[blockIdx.x];
    if (!sl->active) return;
    pred_input_row(a, blockIdx.x, sl->code0);
}
void q3_launch_pred_input(const Q3PredInput& a, hipStream_t s) { hipLaunchKernelGGL(k_pred_input, dim3(a.B), dim3(256), 0, s, a); }

// ---------------------------------------------------------------------------------------------------------------------
// H6 — Assets::project (/root/reference/src/assets_manager.rs:383-399) in the reference's OWN arithmetic: f32 weights, the
// accumulator starts from the bias and takes `sum += h * w` (one f32 multiply, one f32 add: the build has -ffp-contract=off)
// over the inputs in ascending order. One thread per output element (a 2048-long dependent chain: latency-bound by design);
// 16 consecutive lanes = 16 consecutive outputs of one row, so the same kernel can emit the Predictor's norm inputs.
// tile = 16 rows x 16 outputs; the operands of 64 inputs at a time are staged through LDS by coalesced loads (a thread reading
// its own weight row straight from memory touches 16 cache lines per wave-load). The row stride of 68 floats keeps the 16 weight
// rows of a 128-bit LDS read on distinct banks.
// p.norm_w != nullptr: x holds RAW rows and the tile applies the RMSNorm itself while staging, x' = (x * rinv) * norm_w with rinv from
// the canonical 64-lane chain (the same operations pred_input_row used to store as X), so that the projection
// does not wait for another kernel's normalised copy.
// ---------------------------------------------------------------------------------------------------------------------
constexpr int PJ_KC = 64, PJ_LD = PJ_KC + 4, PJ_LDS_FLOATS = 4 * 16 * PJ_LD, PJ_LDS_FLOATS_Q8 = 6 * 16 * PJ_LD;
// NO = outputs per thread: 1 — the 16 x 16 tile above; 2 — a W8A8 consumer (p.xscale): a thread owns outputs o and o + 16 of a 16 x 32 tile
// (two independent chains, each the same sequence as before), so that a 16-lane group holds one whole Q8_0 block of y * nw
template <int NO>
__device__ void project_tile(const Q3Project& p, int bx, int by, float* lds) {
    constexpr int KC = PJ_KC, LD = PJ_LD;
    float* ws = lds; float* xs = lds + 2 * NO * 16 * LD;  // ws [2][NO * 16 * LD], xs [2][16 * LD]
    __shared__ float rinv16[16];
    const int tid = threadIdx.x, oc = tid & 15, rr = tid >> 4;
    const int o = bx * (16 * NO) + oc, row = by * 16 + rr;
    // staging role: thread t loads 4 consecutive inputs (t & 15) of weight row(s) / activation row (t >> 4)
    const float* wsrc = p.w + (size_t)(bx * (16 * NO) + rr) * p.n_in + 4 * oc;
    const float* xsrc = p.x + (size_t)min(by * 16 + rr, p.rows - 1) * p.ldx + 4 * oc;
    const float* nsrc = p.norm_w ? p.norm_w + 4 * oc : nullptr;
    float sum[NO];
#pragma unroll
    for (int j = 0; j < NO; ++j) sum[j] = p.bias[o + 16 * j];
    const int nch = p.n_in / KC;
    float4 wv[NO], xv = *(const float4*)xsrc, nv = nsrc ? *(const float4*)nsrc : float4{1.0f, 1.0f, 1.0f, 1.0f};
#pragma unroll
    for (int j = 0; j < NO; ++j) wv[j] = *(const float4*)(wsrc + (size_t)16 * j * p.n_in);
    float rinv = 1.0f;
    if (nsrc) {  // (uniform) wave w owns rows 4w .. 4w + 3 of the tile: four chains side by side, lane c takes the float4 chunks c, c + 64, ...
        const int wave = tid >> 6, lane = tid & 63;
        const float4* xr[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) xr[u] = (const float4*)(p.x + (size_t)min(by * 16 + wave * 4 + u, p.rows - 1) * p.ldx);
        float acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        for (int c = lane; c < (p.n_in >> 2); c += 64) {
            float4 v[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) v[u] = xr[u][c];
#pragma unroll
            for (int u = 0; u < 4; ++u) { acc[u] = fmaf(v[u].x, v[u].x, acc[u]); acc[u] = fmaf(v[u].y, v[u].y, acc[u]); acc[u] = fmaf(v[u].z, v[u].z, acc[u]); acc[u] = fmaf(v[u].w, v[u].w, acc[u]); }
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) { const float t = wave_sum(acc[u]); if (lane == 0) rinv16[wave * 4 + u] = 1.0f / sqrtf(t / (float)p.n_in + p.eps); }
        __syncthreads();
        rinv = rinv16[rr];
    }
    for (int c = 0; c < nch; ++c) {
        float* wl = ws + (c & 1) * (NO * 16 * LD); float* xl = xs + (c & 1) * 16 * LD;
        if (nsrc) { xv.x = (xv.x * rinv) * nv.x; xv.y = (xv.y * rinv) * nv.y; xv.z = (xv.z * rinv) * nv.z; xv.w = (xv.w * rinv) * nv.w; }
#pragma unroll
        for (int j = 0; j < NO; ++j) *(float4*)(wl + (rr + 16 * j) * LD + 4 * oc) = wv[j];
        *(float4*)(xl + rr * LD + 4 * oc) = xv;
        if (c + 1 < nch) {
#pragma unroll
            for (int j = 0; j < NO; ++j) wv[j] = *(const float4*)(wsrc + (size_t)16 * j * p.n_in + (c + 1) * KC);
            xv = *(const float4*)(xsrc + (c + 1) * KC);
            if (nsrc) nv = *(const float4*)(nsrc + (c + 1) * KC);
        }
        __syncthreads();  // (two buffers: the stores of chunk c + 2 come after the barrier of chunk c + 1, which every reader of chunk c has passed)
        const float* xr = xl + rr * LD;
#pragma unroll
        for (int k = 0; k < KC; k += 4) {
            const float4 a = *(const float4*)(xr + k);
#pragma unroll
            for (int j = 0; j < NO; ++j) {
                const float4 w4 = *(const float4*)(wl + (oc + 16 * j) * LD + k);
                sum[j] += a.x * w4.x; sum[j] += a.y * w4.y; sum[j] += a.z * w4.z; sum[j] += a.w * w4.w;
            }
        }
    }
    const bool live = row < p.rows;
#pragma unroll
    for (int j = 0; j < NO; ++j)
        if (live) p.y[(size_t)row * p.ldy + o + 16 * j] = sum[j];
    if (p.nw) {
        float sq[NO];
#pragma unroll
        for (int j = 0; j < NO; ++j) {
            sq[j] = sum[j] * sum[j];
            sq[j] = sq[j] + __shfl_xor(sq[j], 1); sq[j] = sq[j] + __shfl_xor(sq[j], 2); sq[j] = sq[j] + __shfl_xor(sq[j], 4); sq[j] = sq[j] + __shfl_xor(sq[j], 8);
            if (live && oc == 0) p.ssp[(size_t)row * p.ld_ssp + ((o + 16 * j) >> 4)] = sq[j];
        }
        if constexpr (NO == 2) {  // the block = the 32 outputs of this row's 16 lanes: ggml's quantiser on v = y * nw
            const float u0 = sum[0] * p.nw[o], u1 = sum[1] * p.nw[o + 16];
            float amax = fmaxf(fabsf(u0), fabsf(u1));
#pragma unroll
            for (int m = 1; m <= 8; m <<= 1) amax = fmaxf(amax, __shfl_xor(amax, m));
            const float d = amax / 127.0f, id = d != 0.0f ? 1.0f / d : 0.0f;
            if (live) {
                ((int8_t*)p.xb)[q3_q8_off(row, o, p.n_out >> 6)] = (int8_t)(int)roundf(u0 * id);
                ((int8_t*)p.xb)[q3_q8_off(row, o + 16, p.n_out >> 6)] = (int8_t)(int)roundf(u1 * id);
                if (oc == 0) p.xscale[q3_q8_scale_idx(row, o >> 5, p.x_rt16)] = q3_q8_sig11(d);
            }
        } else if (live) p.xb[q3_atile_off(row, o, p.n_out >> 5)] = q3_bf16(sum[0] * p.nw[o]);
    }
}
__global__ __launch_bounds__(256) void k_project(Q3Project p) {
    __shared__ __attribute__((aligned(16))) float lds[PJ_LDS_FLOATS];
    project_tile<1>(p, blockIdx.x, blockIdx.y, lds);
}
static bool project_ok(const Q3Project& p) { return p.rows >= 1 && p.n_out % 16 == 0 && p.n_in % 64 == 0 && p.ldx % 4 == 0 && !(p.xscale && (!p.nw || p.n_out % 32 || p.x_rt16 < 1)); }
int q3_launch_project(const Q3Project& p, hipStream_t s) {
    if (!project_ok(p) || p.xscale) return -1;  // (the Q8_0 output exists in the frame's first launch only: q3_launch_sample_input)
    hipLaunchKernelGGL(k_project, dim3(p.n_out / 16, (p.rows + 15) / 16), dim3(256), 0, s, p);
    return 0;
}

// the frame's first launch, two kinds of workgroup side by side (they touch disjoint data, so neither waits for the other):
//  [0, B)   H4/H5 (sample, EOS, bookkeeping) and, for rows that go on, the code row of the Predictor's pass A and the feedback start
//  [B, ...) H6 for the hidden rows, normalised in the tile (project_tile with norm_w)
static_assert(PJ_LDS_FLOATS_Q8 * sizeof(float) <= SAMP_MAX * sizeof(unsigned long long), "the projection tile stages through the sampler's key array");
__global__ __launch_bounds__(256) void k_sample_input(Q3Sample a, Q3PredInput p, Q3Project pj) {
    __shared__ __attribute__((aligned(16))) unsigned long long keys[SAMP_MAX];
    __shared__ float probs[SAMP_MAX];
    if ((int)blockIdx.x >= a.B) {  // (uniform over the workgroup)
        const int t = blockIdx.x - a.B;
        if (pj.xscale) { const int nx = pj.n_out >> 5; project_tile<2>(pj, t % nx, t / nx, (float*)keys); }   // (uniform) W8A8 Predictor: 16 x 32 tiles
        else { const int nx = pj.n_out >> 4; project_tile<1>(pj, t % nx, t / nx, (float*)keys); }
        return;
    }
    const int code0 = sample_frame(a, blockIdx.x, keys, probs);  // (uniform over the workgroup)
    if (code0 < 0) return;
    pred_input_row(p, blockIdx.x, code0);
}
int q3_launch_sample_input(const Q3Sample& a, const Q3PredInput& p, const Q3Project& pj, hipStream_t s) {
    if (!project_ok(pj) || !pj.norm_w) return -1;
    hipLaunchKernelGGL(k_sample_input, dim3(a.B + (pj.n_out / (pj.xscale ? 32 : 16)) * ((pj.rows + 15) / 16)), dim3(256), 0, s, a, p, pj);
    return 0;
}

// SAMPLE = false: code_q = argmax, from the per-tile keys of the head GEMM's ARGMAX epilogue. SAMPLE = true: the head GEMM stored its
// logits (plogits) and code_q = sample_row on them with the slot's Predictor sampler — the reference's sampler (H4) on codebook_size
// logits; a slot whose p_temperature is 0 takes sample_row's greedy branch: the same q3_argmax_key maximum as the keys' (ties -> smaller
// index, NaN never wins). The sampler's 48 KiB of LDS (+ the row, dynamic: cbs floats) exist in the SAMPLE instantiation only.
// text[id][i] through the table's out-of-range rule (src/assets_manager.rs:444-460): the prompt builder's and the streamed text rows'
__device__ __forceinline__ float text_elem(const float* text, int text_vocab, int id, int i, int d) {
    if (id >= 0 && id < text_vocab) return text[(size_t)id * d + i];
    return fmodf((float)((unsigned long long)id * 17ull + (unsigned long long)i), 2.0f) - 1.0f;
}
__device__ __forceinline__ const Q3TextRows& text_rows(const Q3TextRows& t) { return t; }
// TX: nothing (the kernel every pass of the default frame step runs: its arguments are Q3PredNext alone), or Q3TextRows — the last pass
// of the text form (q3_launch_pred_last_text): the addend row is the slot's streamed text row t.cur[slot] instead of tts_pad
template <bool SAMPLE, class... TX>
__global__ __launch_bounds__(256) void k_pred_next(Q3PredNext a, TX... tx) {
    constexpr bool TEXT = sizeof...(TX) != 0;
    const int b = blockIdx.x, tid = threadIdx.x, d = a.d;
    // the per-tile keys / the logits row do not depend on the slot: requested before the slot state is looked at (one round trip less on the chain)
    unsigned long long kk = 0ull;
    float lv[SAMPLE ? SAMP_MAX / 256 : 1];
    if constexpr (SAMPLE) {
#pragma unroll
        for (int j = 0; j < SAMP_MAX / 256; ++j) { const int i = tid + j * 256; lv[j] = i < a.cbs ? a.plogits[(size_t)b * a.cbs + i] : 0.0f; }
    } else kk = tid < a.n_key_parts ? a.keys[(size_t)b * a.n_key_parts + tid] : 0ull;
    const int slot = a.row_slot[b];
    Q3Slot* sl = a.slots + slot;
    const bool last = a.q == a.ncb - 1;
    // the slot's text cursor and count travel with the slot record (both hang off `slot` alone)
    int2 cur = make_int2(0, 0); int tcnt = 0;
    if constexpr (TEXT) { const Q3TextRows& t = text_rows(tx...); cur = t.cur[slot]; tcnt = min(t.cnt[slot], t.cap); }
    if (!sl->active) {
        if (last && tid == 0) a.row_pos_t[b] = -1;
        return;
    }
    int code;
    if constexpr (SAMPLE) {
        __shared__ unsigned long long keys[SAMP_MAX];
        __shared__ float probs[SAMP_MAX];
        extern __shared__ float lrow[];  // [cbs]: sample_row reads the row up to three times
#pragma unroll
        for (int j = 0; j < SAMP_MAX / 256; ++j) { const int i = tid + j * 256; if (i < a.cbs) lrow[i] = lv[j]; }
        const float temperature = sl->p_temperature;
        // positional draw index: the same stream whatever the batch, the slot and the number of GPUs
        const float r = temperature > 0.0f ? a.prng[(size_t)slot * a.prng_stride + (size_t)sl->n_frames * (a.ncb - 1) + (a.q - 1)] : 0.0f;
        const int top_k = sl->p_top_k; const float top_p = sl->p_top_p;
        __syncthreads();
        code = sample_row(lrow, a.cbs, temperature, top_k, top_p, r, keys, probs);
    } else {
    // code_q = argmax of the head's logits: the maximum of the per-tile keys the head GEMM left (ties -> smaller index, NaN never wins)
    __shared__ unsigned long long kmax_s[4];
    for (int t = tid + 256; t < a.n_key_parts; t += 256) { const unsigned long long o = a.keys[(size_t)b * a.n_key_parts + t]; kk = o > kk ? o : kk; }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) { const unsigned long long o = __shfl_xor(kk, m); kk = o > kk ? o : kk; }
    if ((tid & 63) == 0) kmax_s[tid >> 6] = kk;
    __syncthreads();
    kk = kmax_s[0];
#pragma unroll
    for (int w = 1; w < 4; ++w) kk = kmax_s[w] > kk ? kmax_s[w] : kk;
    code = q3_argmax_idx(kk);
    }
    const bool ok = code >= 0 && code < a.rows_q;
    const float* e = a.codec_q + (size_t)(ok ? code : 0) * d;
    const int frame = sl->n_frames;
    if (tid == 0) a.codes[((size_t)slot * a.max_steps_cap + frame) * a.ncb + a.q] = code;
    // operands of the whole row first, stores after (see pred_input_row): the table rows and the running feedback sum in one round trip
    constexpr int NI = 8, NP = 4;
    const float* pr = ok ? a.pproj_q + (size_t)code * a.dp : a.proj_b;
    const bool trow = cur.x != 0;  // (uniform over the workgroup; TEXT only)
    float pv[NP], wv[NP];
    if (!last) {
#pragma unroll
        for (int u = 0; u < NP; ++u) { const int i = min(tid + u * 256, a.dp - 1); pv[u] = pr[i]; wv[u] = a.nw[i]; }
    }
    for (int i0 = 0; i0 < d; i0 += NI * 256) {
        float ev[NI], fv[NI], tp[NI], nv[NI];
#pragma unroll
        for (int u = 0; u < NI; ++u) {
            const int i = min(i0 + tid + u * 256, d - 1);
            ev[u] = ok ? e[i] : 0.0f; fv[u] = a.fb[(size_t)b * d + i];
            if (last) {
                if constexpr (TEXT) tp[u] = trow ? text_elem(text_rows(tx...).text, text_rows(tx...).text_vocab, cur.y, i, d) : a.tts_pad[i];
                else tp[u] = a.tts_pad[i];
                nv[u] = a.nw[i];
            }
        }
#pragma unroll
        for (int u = 0; u < NI; ++u) {
            const int i = i0 + tid + u * 256;
            if (i >= d) continue;  // (uniform per wave: d % 256 == 0)
            float f = fv[u] + ev[u];
            if (!last) a.fb[(size_t)b * d + i] = f;
            else {  // the Talker's next input row and its norm inputs for layer 0
                f = f + tp[u]; a.xT[(size_t)b * d + i] = f;
                // W8A8 consumer: the row as Q8_0 blocks (a half wave = 32 consecutive columns = one block)
                if (a.xscale) q3_norm_out_q8(f, nv[u], b, i, d >> 6, a.x_rt16, (int8_t*)a.xb, a.xscale, a.ssp + (size_t)b * (d >> 4) + (i >> 4), (i & 15) == 0);
                else q3_norm_out(f, nv[u], a.xb + q3_atile_off(b, i, d >> 5), a.ssp + (size_t)b * (d >> 4) + (i >> 4), (i & 15) == 0);
            }
        }
    }
    if (!last) {
#pragma unroll
        for (int u = 0; u < NP; ++u) {
            const int i = tid + u * 256;
            if (i < a.dp) {
                a.px[(size_t)b * a.dp + i] = pv[u];
                if (a.xscale) q3_norm_out_q8(pv[u], wv[u], b, i, a.dp >> 6, a.x_rt16, (int8_t*)a.xb, a.xscale, a.ssp + (size_t)b * (a.dp >> 4) + (i >> 4), (i & 15) == 0);
                else q3_norm_out(pv[u], wv[u], a.xb + q3_atile_off(b, i, a.dp >> 5), a.ssp + (size_t)b * (a.dp >> 4) + (i >> 4), (i & 15) == 0);
            }
        }
        for (int i = tid + NP * 256; i < a.dp; i += 256) {  // (dp > 1024: not a shipped shape)
            const float v = pr[i];
            a.px[(size_t)b * a.dp + i] = v;
            if (a.xscale) q3_norm_out_q8(v, a.nw[i], b, i, a.dp >> 6, a.x_rt16, (int8_t*)a.xb, a.xscale, a.ssp + (size_t)b * (a.dp >> 4) + (i >> 4), (i & 15) == 0);
            else q3_norm_out(v, a.nw[i], a.xb + q3_atile_off(b, i, a.dp >> 5), a.ssp + (size_t)b * (a.dp >> 4) + (i >> 4), (i & 15) == 0);
        }
    }
    if (last) {
        __syncthreads();
        if (tid == 0) {
            a.row_pos_t[b] = sl->cur_pos; sl->cur_pos = sl->cur_pos + 1; sl->n_frames = frame + 1;
            if constexpr (TEXT) {  // the next frame's row
                const Q3TextRows& t = text_rows(tx...);
                t.cur[slot] = frame + 1 < tcnt ? make_int2(1, t.ids[(size_t)slot * t.cap + frame + 1]) : make_int2(0, 0);
            }
        }
    }
}
// the sampling variant's LDS: 48 KiB static + the row; above 64 KiB in all when cbs > ~3500, so the attribute is set once per device.
// A device that refuses it is reported (-1) and asked again by the next call: nothing may launch the kernel on the strength of a failed call.
int q3_pred_next_prepare() {
    static std::mutex mu;
    static bool done[64] = {false};
    int dev = 0; if (hipGetDevice(&dev) != hipSuccess) dev = 0;
    std::lock_guard<std::mutex> lk(mu);
    if (done[dev & 63]) return 0;
    if (hipFuncSetAttribute((const void*)k_pred_next<true>, hipFuncAttributeMaxDynamicSharedMemorySize, SAMP_MAX * (int)sizeof(float)) != hipSuccess ||
        hipFuncSetAttribute((const void*)k_pred_next<true, Q3TextRows>, hipFuncAttributeMaxDynamicSharedMemorySize, SAMP_MAX * (int)sizeof(float)) != hipSuccess) {
        (void)hipGetLastError();
        return -1;
    }
    done[dev & 63] = true;
    return 0;
}
int q3_launch_pred_next(const Q3PredNext& a, hipStream_t s, bool sample) {
    if (!sample) { hipLaunchKernelGGL(k_pred_next<false>, dim3(a.B), dim3(256), 0, s, a); return 0; }
    if (a.cbs < 1 || a.cbs > SAMP_MAX || !a.plogits || !a.prng || a.q < 1) return -1;
    hipLaunchKernelGGL(k_pred_next<true>, dim3(a.B), dim3(256), (size_t)a.cbs * sizeof(float), s, a);
    return 0;
}
// One workgroup per table row: what k_pred_next<false> writes into xb / ssp for px = that row (the same q3_norm_out per element; a tile's
// 16 lanes are all active since dp % 16 == 0).
__global__ __launch_bounds__(256) void k_pred_table_rows(const float* tab, int rows, const float* bias, int dp, const float* nw, uint16_t* xb, float* ssp) {
    const int c = blockIdx.x;
    const float* pr = c < rows ? tab + (size_t)c * dp : bias;
    for (int i = threadIdx.x; i < dp; i += 256)
        q3_norm_out(pr[i], nw[i], xb + q3_atile_off(c, i, dp >> 5), ssp + (size_t)c * (dp >> 4) + (i >> 4), (i & 15) == 0);
}
void q3_launch_pred_table_rows(const float* tab, int rows, const float* bias, int dp, const float* nw, uint16_t* xb, float* ssp, hipStream_t s) {
    hipLaunchKernelGGL(k_pred_table_rows, dim3(rows + 1), dim3(256), 0, s, tab, rows, bias, dp, nw, xb, ssp);
}
int q3_launch_pred_last_text(const Q3PredNext& a, const Q3TextRows& t, hipStream_t s, bool sample) {
    if (a.q != a.ncb - 1 || !t.ids || !t.cnt || !t.cur || t.cap < 1 || (t.text_vocab > 0 && !t.text)) return -1;
    if (!sample) { hipLaunchKernelGGL((k_pred_next<false, Q3TextRows>), dim3(a.B), dim3(256), 0, s, a, t); return 0; }
    if (a.cbs < 1 || a.cbs > SAMP_MAX || !a.plogits || !a.prng || a.q < 1) return -1;
    hipLaunchKernelGGL((k_pred_next<true, Q3TextRows>), dim3(a.B), dim3(256), (size_t)a.cbs * sizeof(float), s, a, t);
    return 0;
}

// ---------------------------------------------------------------------------------------------------
// Prompt builder (H1: src/tts/prompt.rs:141-277)
// ---------------------------------------------------------------------------------------------------
__device__ __forceinline__ float prompt_elem(int kind, int id, int i, const float* text, int text_vocab,
                                             const float* const* codec, int codec0_rows, int codecq_rows, int ncb,
                                             const float* spk, int d) {
    if (kind == 1) return text_elem(text, text_vocab, id, i, d);
    if (kind >= 2) {  // src/assets_manager.rs:419-437
        const int q = kind - 2;
        const int rows = q == 0 ? codec0_rows : codecq_rows;
        if (id < 0) id = 0;
        if (q < ncb && id < rows) return codec[q][(size_t)id * d + i];
        return 0.0f;
    }
    if (kind == -1) return spk[i];
    return 0.0f;
}
__global__ void k_prompt_rows(const Q3PromptRow* rows, const float* text, int text_vocab, const float* const* codec,
                              int codec0_rows, int codecq_rows, int ncb, const float* spk, int d, float* out) {
    const Q3PromptRow r = rows[blockIdx.x];
    for (int i = threadIdx.x; i < d; i += blockDim.x) {
        const float a = prompt_elem(r.kindA, r.idA, i, text, text_vocab, codec, codec0_rows, codecq_rows, ncb, spk, d);
        float v = a;
        if (r.kindB != 0) v = a + prompt_elem(r.kindB, r.idB, i, text, text_vocab, codec, codec0_rows, codecq_rows, ncb, spk, d);
        out[(size_t)blockIdx.x * d + i] = v;
    }
}
void q3_launch_prompt_rows(const Q3PromptRow* rows, int n, const float* text, int text_vocab, const float* const* codec,
                           int codec0_rows, int codecq_rows, int ncb, const float* spk, int d, float* out, hipStream_t s) {
    hipLaunchKernelGGL(k_prompt_rows, dim3(n), dim3(256), 0, s, rows, text, text_vocab, codec, codec0_rows, codecq_rows, ncb, spk, d, out);
}
__global__ void k_prompt_ref_frames(const int* codes, const float* marker, const float* const* codec, int codec0_rows,
                                    int codecq_rows, int ncb, int d, float* out) {
    const int f = blockIdx.x;
    for (int i = threadIdx.x; i < d; i += blockDim.x) {
        float sum = 0.0f;
        for (int q = 0; q < 16; ++q)
            sum += prompt_elem(2 + q, codes[f * 16 + q], i, nullptr, 0, codec, codec0_rows, codecq_rows, ncb, nullptr, d);
        out[(size_t)f * d + i] = marker[i] + sum;
    }
}
void q3_launch_prompt_ref_frames(const int* codes, int n_frames, const float* marker, const float* const* codec,
                                 int codec0_rows, int codecq_rows, int ncb, int d, float* out, hipStream_t s) {
    hipLaunchKernelGGL(k_prompt_ref_frames, dim3(n_frames), dim3(256), 0, s, codes, marker, codec, codec0_rows, codecq_rows, ncb, d, out);
}

__global__ void k_copy_rows(float* dst, int ldd, const float* src, int lds, int cols) {
    const int r = blockIdx.x;
    for (int i = threadIdx.x; i < cols; i += blockDim.x) dst[(size_t)r * ldd + i] = src[(size_t)r * lds + i];
}
// dst[r] = src[perm[r]] (row compaction of the decode rows)
__global__ void k_gather_rows(float* dst, const float* src, const int* perm, int cols) {
    const int r = blockIdx.y;
    const float* sp = src + (size_t)perm[r] * cols;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < cols; i += gridDim.x * blockDim.x) dst[(size_t)r * cols + i] = sp[i];
}
void q3_launch_gather_rows(float* dst, const float* src, const int* perm, int rows, int cols, hipStream_t s) {
    hipLaunchKernelGGL(k_gather_rows, dim3((cols + 255) / 256, rows), dim3(256), 0, s, dst, src, perm, cols);
}
void q3_launch_copy_rows(float* dst, int ldd, const float* src, int lds, int rows, int cols, hipStream_t s) {
    hipLaunchKernelGGL(k_copy_rows, dim3(rows), dim3(256), 0, s, dst, ldd, src, lds, cols);
}

// One wave per row, 4 rows per workgroup. CPL = float4 chunks per lane (d = 256*CPL) held in registers so the row is
// read once: all loads issue first, then the canonical per-lane fmaf chain (chunks lane, lane+64, ...), the butterfly
// and one float4 store per chunk. CPL = 0: generic two-pass loop.
template <int CPL>
__global__ __launch_bounds__(256) void k_rmsnorm_rows(const float* x, int ldx, const float* w, float eps, int d, int rows, float* out, int ldo) {
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (r >= rows) return;
    const float4* xr = (const float4*)(x + (size_t)r * ldx);
    float4* orow = (float4*)(out + (size_t)r * ldo);
    const float4* w4 = (const float4*)w;
    if constexpr (CPL > 0) {
        float4 v[CPL], g[CPL];
#pragma unroll
        for (int i = 0; i < CPL; ++i) { v[i] = xr[lane + 64 * i]; g[i] = w4[lane + 64 * i]; }
        float acc = 0.0f;
#pragma unroll
        for (int i = 0; i < CPL; ++i) { acc = fmaf(v[i].x, v[i].x, acc); acc = fmaf(v[i].y, v[i].y, acc); acc = fmaf(v[i].z, v[i].z, acc); acc = fmaf(v[i].w, v[i].w, acc); }
        acc = wave_sum(acc);
        const float rinv = 1.0f / sqrtf(acc / (float)d + eps);
#pragma unroll
        for (int i = 0; i < CPL; ++i)
            orow[lane + 64 * i] = make_float4((v[i].x * rinv) * g[i].x, (v[i].y * rinv) * g[i].y, (v[i].z * rinv) * g[i].z, (v[i].w * rinv) * g[i].w);
    } else {
        float acc = 0.0f;
        for (int c = lane; c < (d >> 2); c += 64) {
            const float4 v = xr[c];
            acc = fmaf(v.x, v.x, acc); acc = fmaf(v.y, v.y, acc); acc = fmaf(v.z, v.z, acc); acc = fmaf(v.w, v.w, acc);
        }
        acc = wave_sum(acc);
        const float rinv = 1.0f / sqrtf(acc / (float)d + eps);
        for (int c = lane; c < (d >> 2); c += 64) {
            const float4 v = xr[c], g = w4[c];
            orow[c] = make_float4((v.x * rinv) * g.x, (v.y * rinv) * g.y, (v.z * rinv) * g.z, (v.w * rinv) * g.w);
        }
    }
}
void q3_launch_rmsnorm_rows(const float* x, int ldx, const float* w, float eps, int d, int rows, float* out, int ldo, hipStream_t s) {
    dim3 grid((rows + 3) / 4);
    if (d == 2048) hipLaunchKernelGGL((k_rmsnorm_rows<8>), grid, dim3(256), 0, s, x, ldx, w, eps, d, rows, out, ldo);
    else if (d == 1024) hipLaunchKernelGGL((k_rmsnorm_rows<4>), grid, dim3(256), 0, s, x, ldx, w, eps, d, rows, out, ldo);
    else if (d == 512) hipLaunchKernelGGL((k_rmsnorm_rows<2>), grid, dim3(256), 0, s, x, ldx, w, eps, d, rows, out, ldo);
    else hipLaunchKernelGGL((k_rmsnorm_rows<0>), grid, dim3(256), 0, s, x, ldx, w, eps, d, rows, out, ldo);
}

// ---- PCM gather (sessions, the node's i16 gather) -----------------------------------------------------------------------------
// grid (x, n_ent): blockIdx.y = entry. The window's head up to the first 16-byte boundary of the source row is copied element-wise,
// the body with one float4 load per thread and iteration, the tail element-wise.
template <typename T>
__global__ __launch_bounds__(256) void k_pcm_pack(const float* __restrict__ src, size_t stride, const Q3PcmPack ents, T* __restrict__ dst) {
    const Q3PcmEnt en = ents.e[blockIdx.y];
    const int n = en.count;
    if (n <= 0) return;
    const float* s = src + (size_t)en.row * stride + en.first;
    T* d = dst + en.dst_off;
    const int head = min(n, (int)((4 - (((uintptr_t)s >> 2) & 3)) & 3));
    const int nv = (n - head) >> 2;
    const int tid = blockIdx.x * blockDim.x + threadIdx.x, nth = gridDim.x * blockDim.x;
    if (tid < head) q3_pcm_put(d + tid, s[tid]);
    const float4* sv = (const float4*)(s + head);
    for (int i = tid; i < nv; i += nth) {
        const float4 v = sv[i];
        T* o = d + head + 4 * i;
        q3_pcm_put(o, v.x); q3_pcm_put(o + 1, v.y); q3_pcm_put(o + 2, v.z); q3_pcm_put(o + 3, v.w);
    }
    for (int i = head + 4 * nv + tid; i < n; i += nth) q3_pcm_put(d + i, s[i]);
}
void q3_launch_pcm_pack(const float* src, size_t stride, const Q3PcmPack& ents, int n_ent, int max_count, int i16, void* dst, hipStream_t s) {
    if (n_ent <= 0) return;
    const int gx = std::max(1, std::min(64, (max_count / 4 + 255) / 256));
    if (i16) hipLaunchKernelGGL(k_pcm_pack<int16_t>, dim3(gx, n_ent), dim3(256), 0, s, src, stride, ents, (int16_t*)dst);
    else hipLaunchKernelGGL(k_pcm_pack<float>, dim3(gx, n_ent), dim3(256), 0, s, src, stride, ents, (float*)dst);
}

// q3_attend_kv8.hip — the Talker's attention over a K/V cache of ggml Q8_0 blocks (q3tts_engine_config.kv_q8_0 = 1): the
// quantising append, the attention kernels in the ONE canonical order of DESIGN.md §4.4 applied to the cached values x^ = f32(d) * q, their
// launcher and the voice-prefix copy. The bf16 kernels of q3_attend.hip are untouched; their launchers hand over here when kv8 is set.
// Built with -ffp-contract=off: every fused multiply-add is an explicit fmaf, and d * q stays a multiplication of its own (exact in f32:
// 11 x 7 significant bits), so a chain step fmaf(a, x^, s) sees exactly the value a dequantised cache would hold.
//
// Layout per (slot, KV head), q3_kernels.h (q3_kv8_k_off / q3_kv8_kd_idx):
//   K quants [64-key block][hd/16 chunks][64 keys][16] int8, K scales [64-key block][hd/32][64 keys] f16,
//   V quants [t][hd] int8, V scales [t][hd/32] f16. Positions of a key block that are not written yet stay zero.
// The newest key and value of a fused launch take part as x^ too: they reach their lanes through LDS in the cache's packed form
// (32 words of quants in dim order, then the 4 f16 scales), so every kernel here gives the same bits as every other, and a row sees the same
// keys whether it was decoded or prefilled.
#include "q3_kernels.h"

namespace {
constexpr int HD = Q3_ATT_HD;

__device__ __forceinline__ float kv8_d(uint16_t h) { return (float)__builtin_bit_cast(_Float16, h); }
__device__ __forceinline__ float kv8_q(uint32_t w, int i) { return (float)(int8_t)(w >> (8 * i)); }

// ggml's quantize_row_q8_0 (f32) on one block held by 8 consecutive lanes x 4 elements: d = amax / 127, id = d ? 1 / d : 0,
// q = roundf(x * id), d kept as f16. *qw: the lane's four quants, element e in byte e; *d16: the block's scale (the same in all 8 lanes).
__device__ __forceinline__ void kv8_quant4(const float x[4], uint32_t* qw, uint16_t* d16) {
    float amax = fmaxf(fmaxf(fabsf(x[0]), fabsf(x[1])), fmaxf(fabsf(x[2]), fabsf(x[3])));
    amax = fmaxf(amax, __shfl_xor(amax, 1)); amax = fmaxf(amax, __shfl_xor(amax, 2)); amax = fmaxf(amax, __shfl_xor(amax, 4));
    const float d = amax / 127.0f, id = d != 0.0f ? 1.0f / d : 0.0f;
    uint32_t w = 0;
#pragma unroll
    for (int e = 0; e < 4; ++e) w |= (uint32_t)(uint8_t)(int8_t)(int)roundf(x[e] * id) << (8 * e);
    *qw = w;
    *d16 = __builtin_bit_cast(unsigned short, (_Float16)d);
}
// dims 4 lane .. 4 lane + 3 of position pos into a head's K / V cache (kq / vq: the head's quants, kd / vd: its scales), lanes [0, hd/4)
__device__ __forceinline__ void kv8_put_k(int8_t* kq, uint16_t* kd, int pos, int lane, uint32_t w, uint16_t d16) {
    *(uint32_t*)(kq + q3_kv8_k_off(pos, 4 * lane)) = w;
    if ((lane & 7) == 0) kd[q3_kv8_kd_idx(pos, lane >> 3)] = d16;
}
__device__ __forceinline__ void kv8_put_v(int8_t* vq, uint16_t* vd, int pos, int lane, uint32_t w, uint16_t d16) {
    *(uint32_t*)(vq + (size_t)pos * HD + 4 * lane) = w;
    if ((lane & 7) == 0) vd[(size_t)pos * (HD >> 5) + (lane >> 3)] = d16;
}
// ... and into LDS in the packed form: words [0, 32) the quants in dim order (key chunk c = 16 bytes at l + 4 c), then the 4 scales
__device__ __forceinline__ void kv8_put_lds(uint32_t* l, int lane, uint32_t w, uint16_t d16) {
    l[lane] = w;
    if ((lane & 7) == 0) ((uint16_t*)(l + 32))[lane >> 3] = d16;
}
__device__ __forceinline__ uint16_t kv8_lds_d(const uint32_t* l, int j) { return ((const uint16_t*)(l + 32))[j]; }
// A key as its lane holds it, made opaque to the optimiser once the newest key has been put in place of the cached one. Without it the
// compiler dequantises the newest key ahead of the key-block loop (it is loop-invariant) and keeps all 128 floats live beside the cached key's
// registers: k_attend_kv8<2, true> took 180 VGPRs instead of 63, k_attend_gqa2_kv8 ran out of its 256 and spilled.
// Nothing enforces this: after a compiler upgrade, or a change to these kernels, compile this file with
// -Rpass-analysis=kernel-resource-usage (plus the Makefile's FLAGS) and look for 79 VGPRs in k_attend_kv8<2, true> / <4, true>, about 170
// in k_attend_gqa2_kv8, and ScratchSize 0 in every kernel here.
__device__ __forceinline__ void kv8_opaque(uint4 kv[8], uint16_t ks[4]) {
#pragma unroll
    for (int c = 0; c < 8; ++c) asm volatile("" : "+v"(kv[c].x), "+v"(kv[c].y), "+v"(kv[c].z), "+v"(kv[c].w));
#pragma unroll
    for (int j = 0; j < 4; ++j) { uint32_t t = ks[j]; asm volatile("" : "+v"(t)); ks[j] = (uint16_t)t; }
}

// The two chains of the canonical order on x^ = d * q. Score: 16 dims of a key (one chunk, d ascending; one block scale).
__device__ __forceinline__ float att8_dot4(const float4 q, uint32_t w, float d, float s) {
    s = fmaf(q.x, d * kv8_q(w, 0), s); s = fmaf(q.y, d * kv8_q(w, 1), s);
    s = fmaf(q.z, d * kv8_q(w, 2), s); s = fmaf(q.w, d * kv8_q(w, 3), s);
    return s;
}
__device__ __forceinline__ float att8_dot16(const float* q, const uint4 k, float d, float s) {
    s = att8_dot4(*(const float4*)q, k.x, d, s); s = att8_dot4(*(const float4*)(q + 4), k.y, d, s);
    s = att8_dot4(*(const float4*)(q + 8), k.z, d, s); s = att8_dot4(*(const float4*)(q + 12), k.w, d, s);
    return s;
}
// Value: 8 dims of one value row (8 bytes inside one block) times the key's weight pt onto the lane's 8 partial sums.
__device__ __forceinline__ void att8_pv8(float pt, const uint2 v, float d, float o[8]) {
#pragma unroll
    for (int e = 0; e < 4; ++e) { o[e] = fmaf(pt, d * kv8_q(v.x, e), o[e]); o[4 + e] = fmaf(pt, d * kv8_q(v.y, e), o[4 + e]); }
}
// ... for two heads that share the row (k_attend_gqa2_kv8): the row is decoded once, head 0's sums first, then head 1's.
__device__ __forceinline__ void att8_pv8x2(float pa, float pb, const uint2 v, float d, float o0[8], float o1[8]) {
    float x[8];
#pragma unroll
    for (int e = 0; e < 4; ++e) { x[e] = d * kv8_q(v.x, e); x[4 + e] = d * kv8_q(v.y, e); }
#pragma unroll
    for (int e = 0; e < 8; ++e) o0[e] = fmaf(pa, x[e], o0[e]);
#pragma unroll
    for (int e = 0; e < 8; ++e) o1[e] = fmaf(pb, x[e], o1[e]);
}

// k_qk_prep with a quantising append: one wave per (row, head). A block is 8 lanes of 4 elements, so amax takes three __shfl_xor steps.
__global__ __launch_bounds__(64) void k_qk_prep_kv8(Q3QkPrep a) {
    const int row = blockIdx.x, hx = blockIdx.y, lane = threadIdx.x;
    int pos, slot;
    q3_row_map(row, a.row_pos, a.row_slot, a.slot_mod, a.pos_const, &pos, &slot);
    if (pos < 0) return;
    constexpr int half = HD >> 1, nl = HD >> 2;
    const bool isq = hx < a.Hq;
    const int g = hx - a.Hq;
    float* src = a.qkv + (size_t)row * a.ld + (size_t)hx * HD;  // (a k head: column block Hq + g = hx)
    float o[4];
    prep_head(src, isq ? a.qnw : a.knw, a.eps, a.cs + (size_t)pos * half, a.sn + (size_t)pos * half, HD, lane, o);
    if (isq) {
        if (lane < nl) ((float4*)src)[lane] = (float4){o[0], o[1], o[2], o[3]};
        return;
    }
    float4 vv = (float4){0.f, 0.f, 0.f, 0.f};
    if (lane < nl) vv = ((const float4*)(a.qkv + (size_t)row * a.ld + (size_t)(a.Hq + a.Hkv + g) * HD))[lane];
    const float xv[4] = {vv.x, vv.y, vv.z, vv.w};
    uint32_t kw, vw; uint16_t kd16, vd16;
    kv8_quant4(o, &kw, &kd16);   // (the whole wave: lanes >= hd/4 hold zeros and form blocks of their own)
    kv8_quant4(xv, &vw, &vd16);
    if (lane >= nl) return;
    const size_t hb = ((size_t)slot * a.Hkv + g) * a.n_ctx;
    kv8_put_k((int8_t*)a.kc + hb * HD, a.kd + hb * (HD >> 5), pos, lane, kw, kd16);
    kv8_put_v((int8_t*)a.vc + hb * HD, a.vd + hb * (HD >> 5), pos, lane, vw, vd16);
}

// ---------------------------------------------------------------------------------------------------
// k_attend's structure over the Q8_0 cache: workgroup (kv head g, row), 4 waves per query head of the GQA group. Scores: one key per lane
// (8 chunk loads of 16 bytes + 4 scales per key block), the d-ascending fmaf chain. PV: 16 key-partials (u = t mod 16: wave u/4, lane group
// u%4), 16 lanes x 8 dims per key (8 bytes + one scale). FUSED: the workgroup prepares, quantises and appends its own row first.
// LDS: att_lds (q3_kernels.h); kh / vh hold the newest key / value in the packed form.
// ---------------------------------------------------------------------------------------------------
template <int R, bool FUSED>
__global__ __launch_bounds__(R * 256) void k_attend_kv8(Q3Attend a) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int g = blockIdx.x, row = blockIdx.y;
    int pos, slot;
    q3_row_map(row, a.row_pos, a.row_slot, a.slot_mod, a.pos_const, &pos, &slot);
    if (pos < 0) return;
    const int T = pos + 1, Tcap = a.n_ctx;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, hh = wave >> 2, sw = wave & 3;
    const AttLds L = att_lds(R, Tcap);
    float* p_all = smem, * qh = smem + L.qh, * ow = smem + L.ow, * lw = smem + L.lw, * mw = smem + L.mw;
    uint32_t* kh = (uint32_t*)(smem + L.kh), * vh = (uint32_t*)(smem + L.vh);
    const size_t hb = ((size_t)slot * a.Hkv + g) * a.n_ctx;
    if constexpr (FUSED) {
        const Q3QkPrep& pr = a.prep;
        constexpr int half = HD >> 1, nl = HD >> 2;
        const float* rowp = a.qkv + (size_t)row * a.ld;
        float o[4];
        if (sw == 0) {  // first wave of each query head: q-norm + RoPE -> LDS
            prep_head(rowp + (size_t)(g * R + hh) * HD, pr.qnw, pr.eps, pr.cs + (size_t)pos * half, pr.sn + (size_t)pos * half, HD, lane, o);
            if (lane < nl) *(float4*)(qh + hh * HD + 4 * lane) = (float4){o[0], o[1], o[2], o[3]};
        }
        if (wave == 1) {  // a second wave: k-norm + RoPE, the quantiser on k and on the raw v row, append, and the LDS copies
            prep_head(rowp + (size_t)(a.Hq + g) * HD, pr.knw, pr.eps, pr.cs + (size_t)pos * half, pr.sn + (size_t)pos * half, HD, lane, o);
            float4 vv = (float4){0.f, 0.f, 0.f, 0.f};
            if (lane < nl) vv = ((const float4*)(rowp + (size_t)(a.Hq + a.Hkv + g) * HD))[lane];
            const float xv[4] = {vv.x, vv.y, vv.z, vv.w};
            uint32_t kw, vw; uint16_t kd16, vd16;
            kv8_quant4(o, &kw, &kd16);
            kv8_quant4(xv, &vw, &vd16);
            if (lane < nl) {
                kv8_put_k((int8_t*)pr.kc + hb * HD, pr.kd + hb * (HD >> 5), pos, lane, kw, kd16);
                kv8_put_v((int8_t*)pr.vc + hb * HD, pr.vd + hb * (HD >> 5), pos, lane, vw, vd16);
                kv8_put_lds(kh, lane, kw, kd16);
                kv8_put_lds(vh, lane, vw, vd16);
            }
        }
    } else {
        for (int i = tid; i < R * HD; i += R * 256) qh[i] = a.qkv[(size_t)row * a.ld + (size_t)g * R * HD + i];
    }
    __syncthreads();
    const int8_t* kb = (const int8_t*)a.kc + hb * HD;
    const uint16_t* ksb = a.kd + hb * (HD >> 5);
    const int8_t* vb = (const int8_t*)a.vc + hb * HD;
    const uint16_t* vsb = a.vd + hb * (HD >> 5);
    const float scale = 1.0f / sqrtf((float)HD);
    float* p = p_all + (size_t)hh * Tcap;
    const float* q = qh + hh * HD;
    float mloc = -INFINITY;
    for (int blk = sw; blk * 64 < T; blk += 4) {
        const int t = blk * 64 + lane;
        const uint4* kp = (const uint4*)(kb + (size_t)blk * 64 * HD) + lane;
        const uint16_t* sp = ksb + (size_t)blk * 64 * (HD >> 5) + lane;
        float s = 0.0f;
        uint4 kv[8]; uint16_t ks[4];  // the whole key in flight at once
#pragma unroll
        for (int c = 0; c < 8; ++c) kv[c] = kp[c * 64];
#pragma unroll
        for (int j = 0; j < 4; ++j) ks[j] = sp[j * 64];
        if (FUSED && t == pos) {
#pragma unroll
            for (int c = 0; c < 8; ++c) kv[c] = *(const uint4*)(kh + 4 * c);
#pragma unroll
            for (int j = 0; j < 4; ++j) ks[j] = kv8_lds_d(kh, j);
        }
        if (FUSED) kv8_opaque(kv, ks);
#pragma unroll
        for (int c = 0; c < 8; ++c) s = att8_dot16(q + c * 16, kv[c], kv8_d(ks[c >> 1]), s);
        s = s * scale;
        if (t < T) { p[t] = s; mloc = fmaxf(mloc, s); }
    }
    mloc = wave_max(mloc);
    if (lane == 0) mw[hh * 4 + sw] = mloc;
    __syncthreads();
    const float m = fmaxf(fmaxf(mw[hh * 4], mw[hh * 4 + 1]), fmaxf(mw[hh * 4 + 2], mw[hh * 4 + 3]));
    float lsum = 0.0f;
    for (int blk = sw; blk * 64 < T; blk += 4) {
        const int t = blk * 64 + lane;
        if (t < T) { const float e = q3_expf(p[t] - m); p[t] = e; lsum += e; }
    }
    lsum = wave_sum(lsum);
    if (lane == 0) lw[hh * 4 + sw] = lsum;
    __syncthreads();
    const int kg = lane >> 4, dl = lane & 15;
    float o[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) o[e] = 0.0f;
    // four value rows per trip, loaded together; the chain of a lane still sees its keys in ascending order
    for (int t0 = 4 * sw + kg; t0 < T; t0 += 64) {
        uint2 vv[4]; uint16_t vs[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const size_t tt = (size_t)min(t0 + 16 * u, T - 1);
            vv[u] = *(const uint2*)(vb + tt * HD + dl * 8);
            vs[u] = vsb[tt * (HD >> 5) + (dl >> 2)];
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int t = t0 + 16 * u;
            if (t < T) {
                const float pt = p[t];
                uint2 w = vv[u]; uint16_t d16 = vs[u];
                if (FUSED && t == pos) { w = *(const uint2*)(vh + 2 * dl); d16 = kv8_lds_d(vh, dl >> 2); }  // newest value: from LDS
                att8_pv8(pt, w, kv8_d(d16), o);
            }
        }
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        o[e] = o[e] + __shfl_xor(o[e], 16);
        o[e] = o[e] + __shfl_xor(o[e], 32);
    }
    if (kg == 0) {
#pragma unroll
        for (int e = 0; e < 8; ++e) ow[(hh * 4 + sw) * HD + dl * 8 + e] = o[e];
    }
    __syncthreads();
    for (int i = tid; i < R * HD; i += R * 256) {
        const int h2 = i / HD, d = i - h2 * HD;
        const float r0 = ow[(h2 * 4 + 0) * HD + d], r1 = ow[(h2 * 4 + 1) * HD + d], r2 = ow[(h2 * 4 + 2) * HD + d],
                    r3 = ow[(h2 * 4 + 3) * HD + d];
        const float ov = ((r0 + r1) + r2) + r3;
        const float l = ((lw[h2 * 4] + lw[h2 * 4 + 1]) + lw[h2 * 4 + 2]) + lw[h2 * 4 + 3];
        att_out1(a, row, g * R + h2, d, ov / l);  // (Q8 output: a half wave = one block)
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// The Talker's decode step over the Q8_0 cache, laid out as k_attend_gqa2: FOUR waves per (slot, KV head), wave sw owns the key blocks
// sw, sw + 4, ... for BOTH query heads — a key block and a value row are loaded and decoded once and used twice —; the row's own operands
// are requested before the cache operands, and the cache operands of the first key block and the first two value trips before the first
// barrier; the newest key / value reach their lanes through LDS in the packed form. Same bits as k_attend_kv8<2, true>.
// A key block is 8 KiB + 512 B here (16 KiB in bf16): kv[8] + vv[4][4] take 64 registers where k_attend_gqa2's take 128.
// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256, 2) void k_attend_gqa2_kv8(Q3Attend a) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int g = blockIdx.x, row = blockIdx.y;
    int pos, slot;
    q3_row_map(row, a.row_pos, a.row_slot, a.slot_mod, a.pos_const, &pos, &slot);
    if (pos < 0) return;
    constexpr int half = HD >> 1, nl = HD >> 2, nb = HD >> 5;
    const int T = pos + 1, Tcap = a.n_ctx;
    const int tid = threadIdx.x, sw = tid >> 6, lane = tid & 63, kg = lane >> 4, dl = lane & 15;
    float* p0 = smem;                          // [Tcap] scores / probabilities of head 0
    float* p1 = p0 + Tcap;                     // [Tcap] head 1
    float* qh = p1 + Tcap;                     // [2][hd]
    float* ow = qh + 2 * HD;                   // [2][4][hd]
    float* lw = ow + 2 * 4 * HD;               // [2][4]
    float* mw = lw + 8;                        // [2][4]
    uint32_t* knew = (uint32_t*)(mw + 8);      // [64] newest key, packed form (32 words of quants, 4 f16 scales)
    uint32_t* vnew = knew + 64;                // [64] newest value, packed form
    const Q3QkPrep& pr = a.prep;
    const size_t hb = ((size_t)slot * a.Hkv + g) * a.n_ctx;
    const int8_t* kb = (const int8_t*)a.kc + hb * HD;
    const uint16_t* ksb = a.kd + hb * nb;
    const int8_t* vb = (const int8_t*)a.vc + hb * HD;
    const uint16_t* vsb = a.vd + hb * nb;
    // the row's own operands first (L2, short latency): waves 0, 1 the two query heads, wave 2 k, wave 3 v
    const float* rowp = a.qkv + (size_t)row * a.ld;
    const float* src = rowp + (size_t)(sw < 2 ? g * 2 + sw : (sw == 2 ? a.Hq + g : a.Hq + a.Hkv + g)) * HD;
    float4 x4 = (float4){0.f, 0.f, 0.f, 0.f}, w4 = x4, c4 = (float4){1.f, 1.f, 1.f, 1.f}, s4 = x4;
    if (lane < nl) {
        x4 = ((const float4*)src)[lane];
        if (sw < 3) {
            w4 = ((const float4*)(sw < 2 ? pr.qnw : pr.knw))[lane];
            c4 = *(const float4*)(pr.cs + (size_t)pos * half + 4 * (lane & 15)); s4 = *(const float4*)(pr.sn + (size_t)pos * half + 4 * (lane & 15));
        }
    }
    __builtin_amdgcn_sched_barrier(0);
    {   // preparation of this row: q heads (waves 0, 1), k (wave 2: norm + RoPE + quantiser + append), v (wave 3: quantiser + append)
        float o[4] = {x4.x, x4.y, x4.z, x4.w};
        if (sw < 3) prep_arith(x4, w4, c4, s4, pr.eps, lane, o);
        if (sw < 2) {
            if (lane < nl) *(float4*)(qh + sw * HD + 4 * lane) = (float4){o[0], o[1], o[2], o[3]};
        } else {
            uint32_t w; uint16_t d16;
            kv8_quant4(o, &w, &d16);  // (the whole wave)
            if (lane < nl) {
                if (sw == 2) { kv8_put_k((int8_t*)pr.kc + hb * HD, pr.kd + hb * nb, pos, lane, w, d16); kv8_put_lds(knew, lane, w, d16); }
                else { kv8_put_v((int8_t*)pr.vc + hb * HD, pr.vd + hb * nb, pos, lane, w, d16); kv8_put_lds(vnew, lane, w, d16); }
            }
        }
    }
    // the cache operands only now (k_attend_gqa2: HBM misses issued ahead of the preparation's L2 hits held every wave's preparation back):
    // the wave's first key block and the value rows of its first two trips; trips 2, 3 (keys 128 .. 255) follow under the softmax phases
    __builtin_amdgcn_sched_barrier(0);
    uint4 kv[8]; uint16_t ks[4];
    uint2 vv[4][4]; uint16_t vs[4][4];
    {
        const int b0 = min(sw, (T - 1) >> 6);
        const uint4* kp = (const uint4*)(kb + (size_t)b0 * 64 * HD) + lane;
        const uint16_t* sp = ksb + (size_t)b0 * 64 * nb + lane;
#pragma unroll
        for (int c = 0; c < 8; ++c) kv[c] = kp[c * 64];
#pragma unroll
        for (int j = 0; j < 4; ++j) ks[j] = sp[j * 64];
#pragma unroll
        for (int tr = 0; tr < 2; ++tr)
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const size_t tt = (size_t)min(64 * tr + 4 * sw + kg + 16 * u, T - 1);
                vv[tr][u] = *(const uint2*)(vb + tt * HD + dl * 8);
                vs[tr][u] = vsb[tt * nb + (dl >> 2)];
            }
    }
    __builtin_amdgcn_sched_barrier(0);
    Q3_LDS_BARRIER();
    const float scale = 1.0f / sqrtf((float)HD);
    float ml0 = -INFINITY, ml1 = -INFINITY;
    for (int blk = sw; blk * 64 < T; blk += 4) {
        const int t = blk * 64 + lane;
        if (blk != sw) {  // (contexts beyond 256 keys: the following blocks of this wave)
            const uint4* kp = (const uint4*)(kb + (size_t)blk * 64 * HD) + lane;
            const uint16_t* sp = ksb + (size_t)blk * 64 * nb + lane;
#pragma unroll
            for (int c = 0; c < 8; ++c) kv[c] = kp[c * 64];
#pragma unroll
            for (int j = 0; j < 4; ++j) ks[j] = sp[j * 64];
        }
        if (t == pos) {
#pragma unroll
            for (int c = 0; c < 8; ++c) kv[c] = *(const uint4*)(knew + 4 * c);
#pragma unroll
            for (int j = 0; j < 4; ++j) ks[j] = kv8_lds_d(knew, j);
        }
        kv8_opaque(kv, ks);
        float s0 = 0.0f, s1 = 0.0f;
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            const float d = kv8_d(ks[c >> 1]);
            s0 = att8_dot16(qh + c * 16, kv[c], d, s0);
            s1 = att8_dot16(qh + HD + c * 16, kv[c], d, s1);
        }
        s0 = s0 * scale; s1 = s1 * scale;
        if (t < T) { p0[t] = s0; p1[t] = s1; ml0 = fmaxf(ml0, s0); ml1 = fmaxf(ml1, s1); }
    }
#pragma unroll
    for (int tr = 2; tr < 4; ++tr)
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const size_t tt = (size_t)min(64 * tr + 4 * sw + kg + 16 * u, T - 1);
            vv[tr][u] = *(const uint2*)(vb + tt * HD + dl * 8);
            vs[tr][u] = vsb[tt * nb + (dl >> 2)];
        }
    ml0 = wave_max(ml0); ml1 = wave_max(ml1);
    if (lane == 0) { mw[sw] = ml0; mw[4 + sw] = ml1; }
    Q3_LDS_BARRIER();
    const float m0 = fmaxf(fmaxf(mw[0], mw[1]), fmaxf(mw[2], mw[3])), m1 = fmaxf(fmaxf(mw[4], mw[5]), fmaxf(mw[6], mw[7]));
    float ls0 = 0.0f, ls1 = 0.0f;
    for (int blk = sw; blk * 64 < T; blk += 4) {
        const int t = blk * 64 + lane;
        if (t < T) {
            const float e0 = q3_expf(p0[t] - m0), e1 = q3_expf(p1[t] - m1);
            p0[t] = e0; p1[t] = e1; ls0 += e0; ls1 += e1;
        }
    }
    ls0 = wave_sum(ls0); ls1 = wave_sum(ls1);
    if (lane == 0) { lw[sw] = ls0; lw[4 + sw] = ls1; }
    Q3_LDS_BARRIER();
    float o0[8], o1[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) { o0[e] = 0.0f; o1[e] = 0.0f; }
    const uint2 vn = *(const uint2*)(vnew + 2 * dl);
    const uint16_t vnd = kv8_lds_d(vnew, dl >> 2);
#pragma unroll
    for (int tr = 0; tr < 4; ++tr) {  // the first four trips: value rows already in registers
        const int t0 = 64 * tr + 4 * sw + kg;
        if (64 * tr >= T) break;  // (uniform)
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int t = t0 + 16 * u;
            if (t < T) {
                const float pa = p0[t], pb = p1[t];
                const bool nw = t == pos;
                att8_pv8x2(pa, pb, nw ? vn : vv[tr][u], kv8_d(nw ? vnd : vs[tr][u]), o0, o1);
            }
        }
    }
    for (int t0 = 256 + 4 * sw + kg; t0 < T; t0 += 64) {  // contexts beyond 256 keys: four value rows loaded together per trip
        uint2 vl[4]; uint16_t sl[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const size_t tt = (size_t)min(t0 + 16 * u, T - 1);
            vl[u] = *(const uint2*)(vb + tt * HD + dl * 8);
            sl[u] = vsb[tt * nb + (dl >> 2)];
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int t = t0 + 16 * u;
            if (t < T) {
                const float pa = p0[t], pb = p1[t];
                const bool nw = t == pos;
                att8_pv8x2(pa, pb, nw ? vn : vl[u], kv8_d(nw ? vnd : sl[u]), o0, o1);
            }
        }
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        o0[e] = o0[e] + __shfl_xor(o0[e], 16); o0[e] = o0[e] + __shfl_xor(o0[e], 32);
        o1[e] = o1[e] + __shfl_xor(o1[e], 16); o1[e] = o1[e] + __shfl_xor(o1[e], 32);
    }
    if (kg == 0) {
        *(float4*)(ow + (0 * 4 + sw) * HD + dl * 8) = (float4){o0[0], o0[1], o0[2], o0[3]}; *(float4*)(ow + (0 * 4 + sw) * HD + dl * 8 + 4) = (float4){o0[4], o0[5], o0[6], o0[7]};
        *(float4*)(ow + (1 * 4 + sw) * HD + dl * 8) = (float4){o1[0], o1[1], o1[2], o1[3]}; *(float4*)(ow + (1 * 4 + sw) * HD + dl * 8 + 4) = (float4){o1[4], o1[5], o1[6], o1[7]};
    }
    Q3_LDS_BARRIER();
    if (tid < 128) {  // two consecutive dims of one head per thread (Q8 output: 16 lanes x 2 dims = one block, both waves whole)
        const int h2 = tid >> 6, d0 = 2 * (tid & 63);
        const float l = ((lw[h2 * 4] + lw[h2 * 4 + 1]) + lw[h2 * 4 + 2]) + lw[h2 * 4 + 3];
        float ov[2];
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const int d = d0 + q;
            const float r0 = ow[(h2 * 4 + 0) * HD + d], r1 = ow[(h2 * 4 + 1) * HD + d], r2 = ow[(h2 * 4 + 2) * HD + d], r3 = ow[(h2 * 4 + 3) * HD + d];
            ov[q] = (((r0 + r1) + r2) + r3) / l;
        }
        att_out2(a, row, g * 2 + h2, d0, ov[0], ov[1]);
    }
}

// Voice prefixes: one workgroup per (layer, K or V, KV head) and entry copies quants and scales of a prefix store into its slot: whole key
// blocks for K, positions < P for V (q3_kernels.h, Q3KvPrefix).
__global__ __launch_bounds__(256) void k_kv_prefix_kv8(Q3KvPrefix a) {
    const int j = blockIdx.y, isv = blockIdx.x & 1, lg = blockIdx.x >> 1, l = lg / a.Hkv, g = lg - l * a.Hkv;
    const int P = a.P[j], np = (P + 63) & ~63, nb = a.hd >> 5;
    const size_t store_q = (size_t)a.L * a.Hkv * np * a.hd;            // bytes of quants in the store; its scales follow
    const size_t sh = ((size_t)l * a.Hkv + g) * np;                    // the head's first position in the store ...
    const size_t dh = ((size_t)a.slot[j] * a.Hkv + g) * a.n_ctx;       // ... and in the layer's cache
    const int8_t* sq = (const int8_t*)(isv ? a.pv[j] : a.pk[j]);
    const uint16_t* ss = (const uint16_t*)(sq + store_q);
    int8_t* dq = (int8_t*)(isv ? a.vc : a.kc) + (size_t)l * a.layer_stride + dh * a.hd;
    uint16_t* ds = (isv ? a.vd : a.kd) + (size_t)l * (a.layer_stride >> 5) + dh * nb;
    const int n = isv ? P : np;
    const uint4* s16 = (const uint4*)(sq + sh * a.hd); uint4* d16 = (uint4*)dq;
    for (int i = threadIdx.x; i < n * (a.hd >> 4); i += 256) d16[i] = s16[i];
    const uint2* s8 = (const uint2*)(ss + sh * nb); uint2* d8 = (uint2*)ds;   // hd / 32 = 4 scales per position: 8 bytes
    for (int i = threadIdx.x; i < n; i += 256) d8[i] = s8[i];
}

// The inverse (k_kv_prefix_save, q3_attend.hip): quants and scales of positions < P of slot[j] into the store, zeros for the keys
// P .. np - 1 of the last block (quants and scales), values only below P. 16-byte unit i of a head's key quants holds key (i & 63) of
// block i / (4 hd); scale i of a head's keys (q3_kv8_kd_idx) belongs to key (i & 63) of block i / (64 hd / 32), four per 8-byte unit.
__global__ __launch_bounds__(256) void k_kv_prefix_save_kv8(Q3KvPrefix a) {
    const int j = blockIdx.y, isv = blockIdx.x & 1, lg = blockIdx.x >> 1, l = lg / a.Hkv, g = lg - l * a.Hkv;
    const int P = a.P[j], np = (P + 63) & ~63, nb = a.hd >> 5;
    const size_t store_q = (size_t)a.L * a.Hkv * np * a.hd;
    const size_t dh = ((size_t)l * a.Hkv + g) * np;                    // the head's first position in the store ...
    const size_t sh = ((size_t)a.slot[j] * a.Hkv + g) * a.n_ctx;       // ... and in the layer's cache
    int8_t* dq = const_cast<int8_t*>((const int8_t*)(isv ? a.pv[j] : a.pk[j]));
    uint16_t* dsc = (uint16_t*)(dq + store_q);
    const int8_t* sq = (const int8_t*)(isv ? a.vc : a.kc) + (size_t)l * a.layer_stride + sh * a.hd;
    const uint16_t* ssc = (isv ? a.vd : a.kd) + (size_t)l * (a.layer_stride >> 5) + sh * nb;
    const uint4* s16 = (const uint4*)sq; uint4* d16 = (uint4*)(dq + dh * a.hd);
    const uint2* s8 = (const uint2*)ssc; uint2* d8 = (uint2*)(dsc + dh * nb);
    if (isv) {
        for (int i = threadIdx.x; i < P * (a.hd >> 4); i += 256) d16[i] = s16[i];
        for (int i = threadIdx.x; i < P; i += 256) d8[i] = s8[i];
        return;
    }
    const int per_blk = a.hd * 4;
    for (int i = threadIdx.x; i < np * (a.hd >> 4); i += 256) {
        const int pos = (i / per_blk) * 64 + (i & 63);
        uint4 v = make_uint4(0u, 0u, 0u, 0u);
        if (pos < P) v = s16[i];
        d16[i] = v;
    }
    const int sc_blk = nb * 64;
    for (int i = threadIdx.x; i < np; i += 256) {  // np * nb scales, nb = 4 per unit: keys p0 .. p0 + 3 of one 32-dim block
        const int k0 = i * 4, p0 = (k0 / sc_blk) * 64 + (k0 & 63);
        uint2 v = make_uint2(0u, 0u);
        if (p0 < P) {
            v = s8[i];
            if (p0 + 1 >= P) v.x &= 0xffffu;
            if (p0 + 2 >= P) v.y = 0u;
            else if (p0 + 3 >= P) v.y &= 0xffffu;
        }
        d8[i] = v;
    }
}
}  // namespace

int q3_launch_qk_prep_kv8(const Q3QkPrep& a, hipStream_t s) {
    if (a.hd != Q3_ATT_HD || !a.kd || !a.vd || a.n_ctx <= 0 || a.n_ctx % 64) return 1;
    hipLaunchKernelGGL(k_qk_prep_kv8, dim3(a.rows, a.Hq + a.Hkv), dim3(64), 0, s, a);
    return 0;
}
void q3_launch_kv_prefix_kv8(const Q3KvPrefix& a, hipStream_t s) {
    if (a.n <= 0 || a.hd != Q3_ATT_HD) return;
    hipLaunchKernelGGL(k_kv_prefix_kv8, dim3(a.L * 2 * a.Hkv, a.n), dim3(256), 0, s, a);
}
int q3_launch_kv_prefix_save_kv8(const Q3KvPrefix& a, hipStream_t s) {
    if (a.n <= 0) return 0;
    if (a.hd != Q3_ATT_HD || a.n > Q3_KVP_MAX || !a.kd || !a.vd) return 1;
    hipLaunchKernelGGL(k_kv_prefix_save_kv8, dim3(a.L * 2 * a.Hkv, a.n), dim3(256), 0, s, a);
    return 0;
}

// The kernel q3_launch_attend_kv8 takes (q3_attend_pick asks here when a.kv8 is set; q3tts_k_attend_pick_kv8 reports it). Whole prompt runs
// (admission, prefix creation; with or without a run table) take the non-fused k_attend_kv8<R, false>: there is no Q8 form of
// k_attend_prefill, k_attend_small or k_attend_pair. One row per slot: k_attend_gqa2_kv8 for two query heads per KV head (decode policy 1:
// k_attend_kv8<2, true>, the same bits), k_attend_kv8<4, true> for four. Q3_ATT_REFUSED: a head size other than Q3_ATT_HD, a GQA ratio
// outside {1, 2, 4}, a fused launch without a second wave for k / v (R == 1), the Predictor's pass A (fused == 2).
int q3_attend_pick_kv8(const Q3Attend& a) {
    if (a.hd != Q3_ATT_HD || a.Hkv <= 0 || a.Hq % a.Hkv) return Q3_ATT_REFUSED;
    const int R = a.Hq / a.Hkv;
    if ((R != 1 && R != 2 && R != 4) || (a.fused && R == 1) || a.fused < 0 || a.fused > 1) return Q3_ATT_REFUSED;
    if (a.fused) {
        int decode = 0, prefill = 0;
        q3_attend_policy_get(&decode, &prefill);
        if (R == 2) return decode == 0 ? Q3_ATT8_GQA2 : Q3_ATT8_F2;
        return Q3_ATT8_F4;
    }
    return R == 1 ? Q3_ATT8_N1 : (R == 2 ? Q3_ATT8_N2 : Q3_ATT8_N4);
}

static hipError_t att8_allow_lds(const void* kernel, size_t lds) { return hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds); }

// 0: launched. Nonzero: refused, nothing launched — a shape q3_attend_pick_kv8 refuses, a cache without scales or with an n_ctx that is not
// whole key blocks, or a device that refuses the LDS size.
int q3_launch_attend_kv8(const Q3Attend& a, hipStream_t s) {
    const int pick = q3_attend_pick_kv8(a);
    if (pick == Q3_ATT_REFUSED || !a.kd || !a.vd || a.n_ctx <= 0 || a.n_ctx % 64) return 1;
    if (a.fused && (!a.prep.kd || !a.prep.vd)) return 1;
    const int R = a.Hq / a.Hkv;
    const dim3 grid(a.Hkv, a.rows);
    if (pick == Q3_ATT8_GQA2) {
        const size_t lds2 = ((size_t)2 * a.n_ctx + 2 * Q3_ATT_HD + 8 * Q3_ATT_HD + 16 + 128) * sizeof(float);  // as k_attend_gqa2_kv8 lays it out
        static Q3PerDevice pd2;
        if (lds2 > 65536 && !pd2.ensure(lds2, [&]() { return att8_allow_lds((const void*)k_attend_gqa2_kv8, lds2); })) return 1;
        hipLaunchKernelGGL(k_attend_gqa2_kv8, grid, dim3(256), lds2, s, a);
        return 0;
    }
    const size_t lds = att_lds(R, a.n_ctx).bytes;
    static Q3PerDevice pd;
    if (lds > 65536 && !pd.ensure(lds, [&]() {
            hipError_t e = hipSuccess;
            for (const void* k : {(const void*)k_attend_kv8<2, true>, (const void*)k_attend_kv8<4, true>, (const void*)k_attend_kv8<1, false>,
                                  (const void*)k_attend_kv8<2, false>, (const void*)k_attend_kv8<4, false>})
                if (e == hipSuccess) e = att8_allow_lds(k, lds);
            return e;
        })) return 1;
    if (pick == Q3_ATT8_F2) hipLaunchKernelGGL((k_attend_kv8<2, true>), grid, dim3(512), lds, s, a);
    else if (pick == Q3_ATT8_F4) hipLaunchKernelGGL((k_attend_kv8<4, true>), grid, dim3(1024), lds, s, a);
    else if (pick == Q3_ATT8_N1) hipLaunchKernelGGL((k_attend_kv8<1, false>), grid, dim3(256), lds, s, a);
    else if (pick == Q3_ATT8_N2) hipLaunchKernelGGL((k_attend_kv8<2, false>), grid, dim3(512), lds, s, a);
    else hipLaunchKernelGGL((k_attend_kv8<4, false>), grid, dim3(1024), lds, s, a);  // Q3_ATT8_N4
    return 0;
}

// q3_attend_kvq.hip — the Talker's attention over a K/V cache of ggml blocks: Q8_0 keys with Q8_0 values
// (q3tts_engine_config.kv_q8_0 = 1), Q8_0 keys with Q4_0 values (llama.cpp's --cache-type-k q8_0 --cache-type-v q4_0) or both in Q4_0
// (q3tts_engine_options.kv_type_k / kv_type_v). The quantising append, the attention kernels in the ONE canonical order of DESIGN.md §4.4
// applied to the cached values x^, their pick rule and launcher, and the voice-prefix copies: each exactly once, a template on a key
// policy Key<Q4> and a value policy Val<Q4>, instantiated for the three accepted pairs. A Q8_0 V beside a Q4_0 K is refused. The bf16
// kernels (q3_attend.hip) are untouched; their launchers hand over here when kv8 is set.
// Built with -ffp-contract=off: every fused multiply-add is an explicit fmaf, and x^ = f32(d) * q (Q8_0; exact in f32: 11 x 7 significant
// bits) or f32(d) * float(q - 8) (Q4_0; 11 x 4) stays a multiplication of its own, so a chain step fmaf(a, x^, s) sees exactly the value a
// dequantised cache would hold.
//
// Layout per (slot, KV head), q3_kernels.h (q3_kv8_k_off / q3_kv4_k_off / q3_kv4_v_off; every scale at q3_kv8_kd_idx):
//   K quants  Q8_0 [64-key block][hd/16 chunks][64 keys][16] int8      Q4_0 [64-key block][hd/32 blocks][64 keys][16 bytes]
//   V quants  Q8_0 [t][hd] int8                                        Q4_0 [t][hd/2 bytes]
//   K scales [64-key block][hd/32][64 keys] f16, V scales [t][hd/32] f16. Dim d of a Q4_0 block: nibble d & 7 of word (d & 31) >> 3.
// Positions of a key block that are not written yet stay zero.
// The newest key and value of a fused launch take part as x^ too: they reach their lanes through LDS in the cache's packed form (the
// quants in dim order from word 0 — 32 words of a Q8_0 vector, 16 of a Q4_0 one — and the 4 f16 scales at word 32), so every kernel here
// gives the same bits as every other, and a row sees the same keys whether it was decoded or prefilled. A policy's bits do not depend on
// the policy beside it: a Q8_0 K holds the same bytes next to either V, a Q4_0 V next to either K.
#include "q3_kernels.h"
#include <type_traits>

namespace {
constexpr int HD = Q3_ATT_HD, NB = HD >> 5;

// a block scale, and the value of quant e of a word: Q8_0 float(int8), Q4_0 float(q - 8) with q = 0 .. 15
__device__ __forceinline__ float kv8_d(uint16_t h) { return (float)__builtin_bit_cast(_Float16, h); }
__device__ __forceinline__ float kv8_q(uint32_t w, int i) { return (float)(int8_t)(w >> (8 * i)); }
__device__ __forceinline__ float kv4_q(uint32_t w, int e) { return (float)((int)((w >> (4 * e)) & 15u) - 8); }

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
// ggml's quantize_row_q4_0 (f32) on one block held by 8 consecutive lanes x 4 elements. max is the element of largest magnitude WITH its
// sign, the first such element in dim order (ggml's loop replaces its candidate only on a strictly larger magnitude): inside a lane the
// loop itself, across lanes three __shfl_xor steps in which a tie goes to the lower lane. d = max / -8, id = d ? 1 / d : 0,
// q = min(15, (int)(x * id + 8.5f)) by truncation, d kept as f16; a zero block has d = 0 and every nibble 8.
// *qw: the 8 nibbles of dims 8 (lane / 2) .. + 7 in dim order — the lane's own four packed with its neighbour's (lane ^ 1) —, the same
// word in both lanes of the pair; *d16: the block's scale, the same in all 8 lanes.
__device__ __forceinline__ void kv4_quant4(const float x[4], int lane, uint32_t* qw, uint16_t* d16) {
    float amax = 0.0f, mx = 0.0f;
#pragma unroll
    for (int e = 0; e < 4; ++e) if (amax < fabsf(x[e])) { amax = fabsf(x[e]); mx = x[e]; }
#pragma unroll
    for (int m = 1; m <= 4; m <<= 1) {
        const float oa = __shfl_xor(amax, m), om = __shfl_xor(mx, m);
        if (oa > amax || (oa == amax && (lane & m))) { amax = oa; mx = om; }
    }
    const float d = mx / -8.0f, id = d != 0.0f ? 1.0f / d : 0.0f;
    uint32_t n = 0;
#pragma unroll
    for (int e = 0; e < 4; ++e) n |= (uint32_t)min(15, (int)(x[e] * id + 8.5f)) << (4 * e);
    const uint32_t o = __shfl_xor(n, 1);
    *qw = (lane & 1) ? (o | (n << 16)) : (n | (o << 16));
    *d16 = __builtin_bit_cast(unsigned short, (_Float16)d);
}
// One vector of either type: the quantiser on the lane's 4 dims (the whole wave calls: lanes >= hd/4 hold zeros and form blocks of their
// own), and the packed LDS form — a Q8_0 lane stores its own word, a Q4_0 pair's even lane the pair's; the block's first lane its scale.
template <bool Q4>
__device__ __forceinline__ void kvq_quant4(const float x[4], int lane, uint32_t* qw, uint16_t* d16) {
    if constexpr (Q4) kv4_quant4(x, lane, qw, d16); else kv8_quant4(x, qw, d16);
}
template <bool Q4>
__device__ __forceinline__ void kvq_put_lds(uint32_t* l, int lane, uint32_t w, uint16_t d16) {
    if (!Q4 || (lane & 1) == 0) l[Q4 ? lane >> 1 : lane] = w;
    if ((lane & 7) == 0) ((uint16_t*)(l + 32))[lane >> 3] = d16;
}
// the quantised dims 4 lane .. + 3 of position pos into a head's K / V cache (kq / vq: the head's quants, kd / vd: its scales), lanes
// [0, hd/4): a Q8_0 lane stores its word, a Q4_0 pair's even lane the pair's; the block's first lane its scale
__device__ __forceinline__ void kv8_put_k(uint8_t* kq, uint16_t* kd, int pos, int lane, uint32_t w, uint16_t d16) {
    *(uint32_t*)(kq + q3_kv8_k_off(pos, 4 * lane)) = w;
    if ((lane & 7) == 0) kd[q3_kv8_kd_idx(pos, lane >> 3)] = d16;
}
__device__ __forceinline__ void kv8_put_v(uint8_t* vq, uint16_t* vd, int pos, int lane, uint32_t w, uint16_t d16) {
    *(uint32_t*)(vq + (size_t)pos * HD + 4 * lane) = w;
    if ((lane & 7) == 0) vd[(size_t)pos * NB + (lane >> 3)] = d16;
}
__device__ __forceinline__ void kv4_put_k(uint8_t* kq, uint16_t* kd, int pos, int lane, uint32_t w, uint16_t d16) {
    if ((lane & 1) == 0) *(uint32_t*)(kq + q3_kv4_k_off(pos, 4 * lane)) = w;
    if ((lane & 7) == 0) kd[q3_kv8_kd_idx(pos, lane >> 3)] = d16;
}
__device__ __forceinline__ void kv4_put_v(uint8_t* vq, uint16_t* vd, int pos, int lane, uint32_t w, uint16_t d16) {
    if ((lane & 1) == 0) *(uint32_t*)(vq + q3_kv4_v_off(pos, 4 * lane)) = w;
    if ((lane & 7) == 0) vd[(size_t)pos * NB + (lane >> 3)] = d16;
}
__device__ __forceinline__ uint16_t kv8_lds_d(const uint32_t* l, int j) { return ((const uint16_t*)(l + 32))[j]; }

// A key as its lane holds it, made opaque to the optimiser once the newest key has been put in place of the cached one. Without it the
// compiler dequantises the newest key ahead of the key-block loop (it is loop-invariant) and keeps all 128 floats live beside the cached
// key's registers: the fused Q8_0 kernel took 180 VGPRs instead of 63, the gqa2 one ran out of its 256 and spilled. (N units: 8 of a Q8_0
// key, 4 of a Q4_0 key.) Nothing enforces this: after a compiler upgrade, or a change to these kernels, compile this file with
// -Rpass-analysis=kernel-resource-usage (plus the Makefile's FLAGS) and look for ScratchSize 0 in every kernel and, in the instances of
// Key<false>, Val<false>, at most 80 VGPRs (six waves per SIMD) in k_attend_kvq<2, true> / <4, true> and about 170 in k_attend_gqa2_kvq.
// How a value row reaches its registers matters in the same way: Val::load assigns through a reference and Val::from_lds returns by
// value because those are the forms in which every instance keeps the registers and occupancy it was measured with.
template <int N> __device__ __forceinline__ void kv8_opaque(uint4 (&kv)[N], uint16_t (&ks)[4]) {
#pragma unroll
    for (int c = 0; c < N; ++c) asm volatile("" : "+v"(kv[c].x), "+v"(kv[c].y), "+v"(kv[c].z), "+v"(kv[c].w));
#pragma unroll
    for (int j = 0; j < 4; ++j) { uint32_t t = ks[j]; asm volatile("" : "+v"(t)); ks[j] = (uint16_t)t; }
}

// The score chain of the canonical order on x^, d ascending: 16 dims of a Q8_0 key (one chunk, one block scale) ...
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
// ... and the 32 dims of one block of a Q4_0 key
__device__ __forceinline__ float att4_dot8(const float4 qa, const float4 qb, uint32_t w, float d, float s) {
    s = fmaf(qa.x, d * kv4_q(w, 0), s); s = fmaf(qa.y, d * kv4_q(w, 1), s); s = fmaf(qa.z, d * kv4_q(w, 2), s); s = fmaf(qa.w, d * kv4_q(w, 3), s);
    s = fmaf(qb.x, d * kv4_q(w, 4), s); s = fmaf(qb.y, d * kv4_q(w, 5), s); s = fmaf(qb.z, d * kv4_q(w, 6), s); s = fmaf(qb.w, d * kv4_q(w, 7), s);
    return s;
}
__device__ __forceinline__ float att4_dot32(const float* q, const uint4 k, float d, float s) {
    s = att4_dot8(*(const float4*)q, *(const float4*)(q + 4), k.x, d, s); s = att4_dot8(*(const float4*)(q + 8), *(const float4*)(q + 12), k.y, d, s);
    s = att4_dot8(*(const float4*)(q + 16), *(const float4*)(q + 20), k.z, d, s); s = att4_dot8(*(const float4*)(q + 24), *(const float4*)(q + 28), k.w, d, s);
    return s;
}

// The key policy. A key as one lane holds it: NK 16-byte units (8 chunks of Q8_0, 4 blocks of Q4_0) and the 4 block scales. One place for
// what differs between the two K types: where a head's keys start, the loads, the newest key's LDS form, the score chain, the append.
template <bool Q4>
struct Key {
    static constexpr int NK = Q4 ? 4 : 8;
    uint4 kv[NK]; uint16_t ks[4];
    static __device__ __forceinline__ size_t head_bytes(size_t hb) { return Q4 ? hb * (HD >> 1) : hb * HD; }  // hb: the head's first position
    // key (64 blk + lane) of a head whose quants start at kb and scales at ksb
    __device__ __forceinline__ void load(const uint8_t* kb, const uint16_t* ksb, int blk, int lane) {
        const uint4* kp = (const uint4*)(kb + (size_t)blk * 64 * (Q4 ? HD >> 1 : HD)) + lane;
        const uint16_t* sp = ksb + (size_t)blk * 64 * NB + lane;
#pragma unroll
        for (int c = 0; c < NK; ++c) kv[c] = kp[c * 64];
#pragma unroll
        for (int j = 0; j < 4; ++j) ks[j] = sp[j * 64];
    }
    __device__ __forceinline__ void from_lds(const uint32_t* l) {
#pragma unroll
        for (int c = 0; c < NK; ++c) kv[c] = *(const uint4*)(l + 4 * c);
#pragma unroll
        for (int j = 0; j < 4; ++j) ks[j] = kv8_lds_d(l, j);
    }
    __device__ __forceinline__ float dot(const float* q) const {  // the d-ascending chain over all hd dims, from 0
        float s = 0.0f;
        if constexpr (Q4) {
#pragma unroll
            for (int j = 0; j < 4; ++j) s = att4_dot32(q + j * 32, kv[j], kv8_d(ks[j]), s);
        } else {
#pragma unroll
            for (int c = 0; c < 8; ++c) s = att8_dot16(q + c * 16, kv[c], kv8_d(ks[c >> 1]), s);
        }
        return s;
    }
    // ... for the two query heads that share the key (k_attend_gqa2_kvq): each block is decoded once, between the two chains' steps
    __device__ __forceinline__ void dot2(const float* q0, const float* q1, float* s0, float* s1) const {
        float a = 0.0f, b = 0.0f;
        if constexpr (Q4) {
#pragma unroll
            for (int j = 0; j < 4; ++j) { const float d = kv8_d(ks[j]); a = att4_dot32(q0 + j * 32, kv[j], d, a); b = att4_dot32(q1 + j * 32, kv[j], d, b); }
        } else {
#pragma unroll
            for (int c = 0; c < 8; ++c) { const float d = kv8_d(ks[c >> 1]); a = att8_dot16(q0 + c * 16, kv[c], d, a); b = att8_dot16(q1 + c * 16, kv[c], d, b); }
        }
        *s0 = a; *s1 = b;
    }
    // the quantiser on the lane's 4 prepared dims (the whole wave calls), the append at pos into a head's K cache and (lds != null) the
    // packed LDS copy
    static __device__ __forceinline__ void append(const float o[4], uint8_t* kq, uint16_t* kd, int pos, int lane, uint32_t* lds) {
        uint32_t w; uint16_t d16;
        kvq_quant4<Q4>(o, lane, &w, &d16);
        if (lane >= (HD >> 2)) return;
        if constexpr (Q4) kv4_put_k(kq, kd, pos, lane, w, d16); else kv8_put_k(kq, kd, pos, lane, w, d16);
        if (lds) kvq_put_lds<Q4>(lds, lane, w, d16);
    }
};

// The value policy, the key policy's mirror. A value-pass lane holds the 8 dims 8 dl .. + 7 of a row — inside one block — as one Row: 8
// bytes of Q8_0, one word of Q4_0. One place for what differs between the two V types: where a head's values start, the row load, the
// newest value's LDS form, the value step of the canonical order, the append.
template <bool Q4>
struct Val {
    using Row = std::conditional_t<Q4, uint32_t, uint2>;
    static constexpr bool Q4_0 = Q4;
    static constexpr int BPP = Q4 ? HD >> 1 : HD;  // bytes per position
    static __device__ __forceinline__ size_t head_bytes(size_t hb) { return hb * BPP; }
    // the lane's 8 dims of position t of a head whose quants start at vb; of the newest value in its packed LDS form
    static __device__ __forceinline__ void load(Row& r, const uint8_t* vb, size_t t, int dl) { r = *(const Row*)(vb + t * BPP + dl * sizeof(Row)); }
    static __device__ __forceinline__ Row from_lds(const uint32_t* l, int dl) { return *(const Row*)(l + dl * (sizeof(Row) / 4)); }
    // 8 dims of one value row times the key's weight pt onto the lane's 8 partial sums
    static __device__ __forceinline__ void pv8(float pt, const Row v, float d, float o[8]) {
        if constexpr (Q4) {
#pragma unroll
            for (int e = 0; e < 8; ++e) o[e] = fmaf(pt, d * kv4_q(v, e), o[e]);
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) { o[e] = fmaf(pt, d * kv8_q(v.x, e), o[e]); o[4 + e] = fmaf(pt, d * kv8_q(v.y, e), o[4 + e]); }
        }
    }
    // ... for two heads that share the row (k_attend_gqa2_kvq): the row is decoded once, head 0's sums first, then head 1's
    static __device__ __forceinline__ void pv8x2(float pa, float pb, const Row v, float d, float o0[8], float o1[8]) {
        float x[8];
        if constexpr (Q4) {
#pragma unroll
            for (int e = 0; e < 8; ++e) x[e] = d * kv4_q(v, e);
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) { x[e] = d * kv8_q(v.x, e); x[4 + e] = d * kv8_q(v.y, e); }
        }
#pragma unroll
        for (int e = 0; e < 8; ++e) o0[e] = fmaf(pa, x[e], o0[e]);
#pragma unroll
        for (int e = 0; e < 8; ++e) o1[e] = fmaf(pb, x[e], o1[e]);
    }
    // the quantiser on the lane's 4 raw dims (the whole wave calls), the append at pos into a head's V cache and (lds != null) the LDS copy
    static __device__ __forceinline__ void append(const float x[4], uint8_t* vq, uint16_t* vd, int pos, int lane, uint32_t* lds) {
        uint32_t w; uint16_t d16;
        kvq_quant4<Q4>(x, lane, &w, &d16);
        if (lane >= (HD >> 2)) return;
        if constexpr (Q4) kv4_put_v(vq, vd, pos, lane, w, d16); else kv8_put_v(vq, vd, pos, lane, w, d16);
        if (lds) kvq_put_lds<Q4>(lds, lane, w, d16);
    }
};

// k_qk_prep with the quantising append: one wave per (row, head). A block is 8 lanes of 4 elements.
template <class K, class V>
__global__ __launch_bounds__(64) void k_qk_prep_kvq(Q3QkPrep a) {
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
    const size_t hb = ((size_t)slot * a.Hkv + g) * a.n_ctx;
    K::append(o, (uint8_t*)a.kc + K::head_bytes(hb), a.kd + hb * NB, pos, lane, nullptr);
    V::append(xv, (uint8_t*)a.vc + V::head_bytes(hb), a.vd + hb * NB, pos, lane, nullptr);
}

// ---------------------------------------------------------------------------------------------------
// k_attend's structure over the cache: workgroup (kv head g, row), 4 waves per query head of the GQA group. Scores: one key per lane
// (K::NK loads of 16 bytes + 4 scales per key block), the d-ascending fmaf chain. PV: 16 key-partials (u = t mod 16: wave u/4, lane
// group u%4), 16 lanes x 8 dims per key (one V::Row + one scale). FUSED: the workgroup prepares, quantises and appends its own row
// first. LDS: att_lds (q3_kernels.h); kh / vh hold the newest key / value in the packed form.
// ---------------------------------------------------------------------------------------------------
template <int R, bool FUSED, class K, class V>
__global__ __launch_bounds__(R * 256) void k_attend_kvq(Q3Attend a) {
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
        if (wave == 1) {  // a second wave: k-norm + RoPE, the quantisers on k and on the raw v row, append, and the LDS copies
            prep_head(rowp + (size_t)(a.Hq + g) * HD, pr.knw, pr.eps, pr.cs + (size_t)pos * half, pr.sn + (size_t)pos * half, HD, lane, o);
            float4 vv = (float4){0.f, 0.f, 0.f, 0.f};
            if (lane < nl) vv = ((const float4*)(rowp + (size_t)(a.Hq + a.Hkv + g) * HD))[lane];
            const float xv[4] = {vv.x, vv.y, vv.z, vv.w};
            uint8_t* kq = (uint8_t*)pr.kc + K::head_bytes(hb), * vq = (uint8_t*)pr.vc + V::head_bytes(hb);
            if constexpr (V::Q4_0) {
                K::append(o, kq, pr.kd + hb * NB, pos, lane, kh);
                V::append(xv, vq, pr.vd + hb * NB, pos, lane, vh);
            } else {
                // Q8_0 / Q8_0 runs both quantisers ahead of the stores: the same bits, and the order in which this instance stays within
                // 80 VGPRs, six waves per SIMD (two appends in a row: 81 / 83 and five). The instances with a Q4_0 V keep the two appends,
                // the order their speed was measured in (83 .. 86 VGPRs, five waves; this order would give them 77 .. 84 and six or five).
                uint32_t kw, vw; uint16_t kd16, vd16;
                kvq_quant4<false>(o, lane, &kw, &kd16);
                kvq_quant4<false>(xv, lane, &vw, &vd16);
                if (lane < nl) {
                    kv8_put_k(kq, pr.kd + hb * NB, pos, lane, kw, kd16);
                    kv8_put_v(vq, pr.vd + hb * NB, pos, lane, vw, vd16);
                    kvq_put_lds<false>(kh, lane, kw, kd16);
                    kvq_put_lds<false>(vh, lane, vw, vd16);
                }
            }
        }
    } else {
        for (int i = tid; i < R * HD; i += R * 256) qh[i] = a.qkv[(size_t)row * a.ld + (size_t)g * R * HD + i];
    }
    __syncthreads();
    const uint8_t* kb = (const uint8_t*)a.kc + K::head_bytes(hb);
    const uint16_t* ksb = a.kd + hb * NB;
    const uint8_t* vb = (const uint8_t*)a.vc + V::head_bytes(hb);
    const uint16_t* vsb = a.vd + hb * NB;
    const float scale = 1.0f / sqrtf((float)HD);
    float* p = p_all + (size_t)hh * Tcap;
    const float* q = qh + hh * HD;
    float mloc = -INFINITY;
    for (int blk = sw; blk * 64 < T; blk += 4) {
        const int t = blk * 64 + lane;
        K key;  // the whole key in flight at once
        key.load(kb, ksb, blk, lane);
        if (FUSED && t == pos) key.from_lds(kh);
        if (FUSED) kv8_opaque(key.kv, key.ks);
        const float s = key.dot(q) * scale;
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
        typename V::Row vv[4]; uint16_t vs[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const size_t tt = (size_t)min(t0 + 16 * u, T - 1);
            V::load(vv[u], vb, tt, dl);
            vs[u] = vsb[tt * NB + (dl >> 2)];
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int t = t0 + 16 * u;
            if (t < T) {
                const float pt = p[t];
                typename V::Row w = vv[u]; uint16_t d16 = vs[u];
                if (FUSED && t == pos) { w = V::from_lds(vh, dl); d16 = kv8_lds_d(vh, dl >> 2); }  // newest value: from LDS
                V::pv8(pt, w, kv8_d(d16), o);
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
// The Talker's decode step, laid out as k_attend_gqa2: FOUR waves per (slot, KV head), wave sw owns the key blocks sw, sw + 4, ... for
// BOTH query heads — a key block and a value row are loaded and decoded once and used twice —; the row's own operands are requested
// before the cache operands, and the cache operands of the first key block and the first two value trips before the first barrier; the
// newest key / value reach their lanes through LDS in the packed form. Same bits as k_attend_kvq<2, true, K, V>. LDS: att_lds_gqa2.
// A key block is 8 KiB + 512 B in Q8_0 and 4 KiB + 512 B in Q4_0 (16 KiB in bf16), a value row 128 B or 64 B + 8 B: kv[NK] + vv[4][4]
// take 64 registers in Q8_0 / Q8_0 and 32 with both in Q4_0, where k_attend_gqa2's take 128.
// ---------------------------------------------------------------------------------------------------------------------
template <class K, class V>
__global__ __launch_bounds__(256, 2) void k_attend_gqa2_kvq(Q3Attend a) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int g = blockIdx.x, row = blockIdx.y;
    int pos, slot;
    q3_row_map(row, a.row_pos, a.row_slot, a.slot_mod, a.pos_const, &pos, &slot);
    if (pos < 0) return;
    constexpr int half = HD >> 1, nl = HD >> 2;
    const int T = pos + 1, Tcap = a.n_ctx;
    const int tid = threadIdx.x, sw = tid >> 6, lane = tid & 63, kg = lane >> 4, dl = lane & 15;
    float* p0 = smem;                          // [Tcap] scores / probabilities of head 0 (the layout att_lds_gqa2 sizes, q3_kernels.h)
    float* p1 = p0 + Tcap;                     // [Tcap] head 1
    float* qh = p1 + Tcap;                     // [2][hd]
    float* ow = qh + 2 * HD;                   // [2][4][hd]
    float* lw = ow + 2 * 4 * HD;               // [2][4]
    float* mw = lw + 8;                        // [2][4]
    uint32_t* knew = (uint32_t*)(mw + 8);      // [64] newest key, packed form (quants from word 0, 4 f16 scales at word 32)
    uint32_t* vnew = knew + 64;                // [64] newest value, packed form
    const Q3QkPrep& pr = a.prep;
    const size_t hb = ((size_t)slot * a.Hkv + g) * a.n_ctx;
    const uint8_t* kb = (const uint8_t*)a.kc + K::head_bytes(hb);
    const uint16_t* ksb = a.kd + hb * NB;
    const uint8_t* vb = (const uint8_t*)a.vc + V::head_bytes(hb);
    const uint16_t* vsb = a.vd + hb * NB;
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
        } else if (sw == 2) K::append(o, (uint8_t*)pr.kc + K::head_bytes(hb), pr.kd + hb * NB, pos, lane, knew);  // (the whole wave)
        else V::append(o, (uint8_t*)pr.vc + V::head_bytes(hb), pr.vd + hb * NB, pos, lane, vnew);
    }
    // the cache operands only now (k_attend_gqa2: HBM misses issued ahead of the preparation's L2 hits held every wave's preparation back):
    // the wave's first key block and the value rows of its first two trips; trips 2, 3 (keys 128 .. 255) follow under the softmax phases
    __builtin_amdgcn_sched_barrier(0);
    K key;
    typename V::Row vv[4][4]; uint16_t vs[4][4];
    key.load(kb, ksb, min(sw, (T - 1) >> 6), lane);
#pragma unroll
    for (int tr = 0; tr < 2; ++tr)
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const size_t tt = (size_t)min(64 * tr + 4 * sw + kg + 16 * u, T - 1);
            V::load(vv[tr][u], vb, tt, dl);
            vs[tr][u] = vsb[tt * NB + (dl >> 2)];
        }
    __builtin_amdgcn_sched_barrier(0);
    Q3_LDS_BARRIER();
    const float scale = 1.0f / sqrtf((float)HD);
    float ml0 = -INFINITY, ml1 = -INFINITY;
    for (int blk = sw; blk * 64 < T; blk += 4) {
        const int t = blk * 64 + lane;
        if (blk != sw) key.load(kb, ksb, blk, lane);  // (contexts beyond 256 keys: the following blocks of this wave)
        if (t == pos) key.from_lds(knew);
        kv8_opaque(key.kv, key.ks);
        float s0, s1;
        key.dot2(qh, qh + HD, &s0, &s1);
        s0 = s0 * scale; s1 = s1 * scale;
        if (t < T) { p0[t] = s0; p1[t] = s1; ml0 = fmaxf(ml0, s0); ml1 = fmaxf(ml1, s1); }
    }
#pragma unroll
    for (int tr = 2; tr < 4; ++tr)
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const size_t tt = (size_t)min(64 * tr + 4 * sw + kg + 16 * u, T - 1);
            V::load(vv[tr][u], vb, tt, dl);
            vs[tr][u] = vsb[tt * NB + (dl >> 2)];
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
    const typename V::Row vn = V::from_lds(vnew, dl);
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
                V::pv8x2(pa, pb, nw ? vn : vv[tr][u], kv8_d(nw ? vnd : vs[tr][u]), o0, o1);
            }
        }
    }
    for (int t0 = 256 + 4 * sw + kg; t0 < T; t0 += 64) {  // contexts beyond 256 keys: four value rows loaded together per trip
        typename V::Row vl[4]; uint16_t sl[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const size_t tt = (size_t)min(t0 + 16 * u, T - 1);
            V::load(vl[u], vb, tt, dl);
            sl[u] = vsb[tt * NB + (dl >> 2)];
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int t = t0 + 16 * u;
            if (t < T) {
                const float pa = p0[t], pb = p1[t];
                const bool nw = t == pos;
                V::pv8x2(pa, pb, nw ? vn : vl[u], kv8_d(nw ? vnd : sl[u]), o0, o1);
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

// Voice prefixes: one workgroup per (layer, K or V, KV head) and entry. A store is one slot's cache of np = ceil(P / 64) * 64 positions —
// k / v [L][Hkv][np * bpp] bytes of quants (bpp = hd for a Q8_0 side, hd / 2 for a Q4_0 side), then its scales [L][Hkv][np * hd / 32] f16 —
// and a.layer_stride counts the cache's ELEMENTS per layer (with kv4 = 0 those are its bytes). 16-byte unit i of a head's key quants
// holds key (i & 63) of block i / (4 bpp); scale i of a head's keys (q3_kv8_kd_idx) belongs to key (i & 63) of block i / (64 hd / 32),
// four per 8-byte unit.
struct PrefixSide { const uint4* sq; uint4* cq; const uint2* ss; uint2* cs; int upp; };  // store / cache quants and scales of one head; 16-byte units per position
__device__ __forceinline__ PrefixSide prefix_side(const Q3KvPrefix& a, int j, int isv, int l, int g, int np) {
    const int nb = a.hd >> 5;
    const size_t bpp = q3_kv4_bytes(a.kv4, isv, (size_t)a.hd);
    const size_t sh = ((size_t)l * a.Hkv + g) * np;                    // the head's first position in the store ...
    const size_t ch = ((size_t)a.slot[j] * a.Hkv + g) * a.n_ctx;       // ... and in the layer's cache
    const uint8_t* sq = (const uint8_t*)(isv ? a.pv[j] : a.pk[j]);
    const uint16_t* ss = (const uint16_t*)(sq + (size_t)a.L * a.Hkv * np * bpp);
    uint8_t* cq = (uint8_t*)(isv ? a.vc : a.kc) + q3_kv4_bytes(a.kv4, isv, (size_t)l * a.layer_stride) + ch * bpp;
    uint16_t* cs = (isv ? a.vd : a.kd) + (size_t)l * (a.layer_stride >> 5) + ch * nb;
    return {(const uint4*)(sq + sh * bpp), (uint4*)cq, (const uint2*)(ss + sh * nb), (uint2*)cs, (int)(bpp >> 4)};
}
// store -> slot: whole key blocks for K, positions < P for V
__global__ __launch_bounds__(256) void k_kv_prefix_kvq(Q3KvPrefix a) {
    const int j = blockIdx.y, isv = blockIdx.x & 1, lg = blockIdx.x >> 1, l = lg / a.Hkv, g = lg - l * a.Hkv;
    const int P = a.P[j], np = (P + 63) & ~63, n = isv ? P : np;
    const PrefixSide s = prefix_side(a, j, isv, l, g, np);
    for (int i = threadIdx.x; i < n * s.upp; i += 256) s.cq[i] = s.sq[i];
    for (int i = threadIdx.x; i < n; i += 256) s.cs[i] = s.ss[i];   // hd / 32 = 4 scales per position: 8 bytes
}
// slot -> store (which comes zero-filled; k_kv_prefix_save, q3_attend.hip): quants and scales of positions < P, zeros for the keys
// P .. np - 1 of the last block, values only below P — byte for byte the store q3tts_prefix_create makes of the same rows
__global__ __launch_bounds__(256) void k_kv_prefix_save_kvq(Q3KvPrefix a) {
    const int j = blockIdx.y, isv = blockIdx.x & 1, lg = blockIdx.x >> 1, l = lg / a.Hkv, g = lg - l * a.Hkv;
    const int P = a.P[j], np = (P + 63) & ~63, nb = a.hd >> 5;
    const PrefixSide s = prefix_side(a, j, isv, l, g, np);
    uint4* dq = const_cast<uint4*>(s.sq); uint2* ds = const_cast<uint2*>(s.ss);
    if (isv) {
        for (int i = threadIdx.x; i < P * s.upp; i += 256) dq[i] = s.cq[i];
        for (int i = threadIdx.x; i < P; i += 256) ds[i] = s.cs[i];
        return;
    }
    const int per_blk = 64 * s.upp;
    for (int i = threadIdx.x; i < np * s.upp; i += 256) {
        const int pos = (i / per_blk) * 64 + (i & 63);
        uint4 v = make_uint4(0u, 0u, 0u, 0u);
        if (pos < P) v = s.cq[i];
        dq[i] = v;
    }
    const int sc_blk = nb * 64;
    for (int i = threadIdx.x; i < np; i += 256) {  // np * nb scales, nb = 4 per unit: keys p0 .. p0 + 3 of one 32-dim block
        const int k0 = i * 4, p0 = (k0 / sc_blk) * 64 + (k0 & 63);
        uint2 v = make_uint2(0u, 0u);
        if (p0 < P) {
            v = s.cs[i];
            if (p0 + 1 >= P) v.x &= 0xffffu;
            if (p0 + 2 >= P) v.y = 0u;
            else if (p0 + 3 >= P) v.y &= 0xffffu;
        }
        ds[i] = v;
    }
}

// The accepted caches. Without Q4_0 blocks (kv4 = 0) the Q8_0 / Q8_0 pair, checked no further than before Q4_0 came; with them the
// scales' flag, V in Q4_0, K in Q8_0 or Q4_0, and no page table.
bool kvq_ok(int kv8, int kv4, const int* tbl) { return !kv4 || (kv8 == 1 && (kv4 == Q3_KV4_V || kv4 == (Q3_KV4_K | Q3_KV4_V)) && !tbl); }
// f<Key, Val>(args...) in the instance of the cache's pair
#define KVQ_PAIR(kv4, f, ...) \
    (!(kv4) ? f<Key<false>, Val<false>>(__VA_ARGS__) : ((kv4) & Q3_KV4_K) ? f<Key<true>, Val<true>>(__VA_ARGS__) : f<Key<false>, Val<true>>(__VA_ARGS__))

template <class K, class V>
int launch_qk_prep(const Q3QkPrep& a, hipStream_t s) {
    hipLaunchKernelGGL((k_qk_prep_kvq<K, V>), dim3(a.rows, a.Hq + a.Hkv), dim3(64), 0, s, a);
    return 0;
}

// the six kernels of a pair in the order of their codes: Q3_ATT8_N1 + k for Q8_0 / Q8_0, Q3_ATT4_N1 + k with Q4_0 blocks
enum { KVQ_N1, KVQ_N2, KVQ_N4, KVQ_F2, KVQ_F4, KVQ_GQA2 };
static_assert(Q3_ATT8_N1 + KVQ_N2 == Q3_ATT8_N2 && Q3_ATT8_N1 + KVQ_N4 == Q3_ATT8_N4 && Q3_ATT8_N1 + KVQ_F2 == Q3_ATT8_F2 &&
              Q3_ATT8_N1 + KVQ_F4 == Q3_ATT8_F4 && Q3_ATT8_N1 + KVQ_GQA2 == Q3_ATT8_GQA2, "pick codes of the Q8_0 cache");
static_assert(Q3_ATT4_N1 + KVQ_N2 == Q3_ATT4_N2 && Q3_ATT4_N1 + KVQ_N4 == Q3_ATT4_N4 && Q3_ATT4_N1 + KVQ_F2 == Q3_ATT4_F2 &&
              Q3_ATT4_N1 + KVQ_F4 == Q3_ATT4_F4 && Q3_ATT4_N1 + KVQ_GQA2 == Q3_ATT4_GQA2, "pick codes of the Q4_0 caches");
int kvq_code_base(int kv4) { return kv4 ? Q3_ATT4_N1 : Q3_ATT8_N1; }

// (the statics are per pair: each pair's kernels need the LDS permission of their own)
template <class K, class V>
int launch_attend(const Q3Attend& a, int k, hipStream_t s) {
    const int R = a.Hq / a.Hkv;
    const dim3 grid(a.Hkv, a.rows);
    if (k == KVQ_GQA2) {
        const size_t lds2 = att_lds_gqa2(a.n_ctx).bytes;
        static Q3PerDevice pd2;
        if (lds2 > 65536 && !pd2.ensure(lds2, [&]() { return att_allow_lds((const void*)k_attend_gqa2_kvq<K, V>, lds2); })) return 1;
        hipLaunchKernelGGL((k_attend_gqa2_kvq<K, V>), grid, dim3(256), lds2, s, a);
        return 0;
    }
    const size_t lds = att_lds(R, a.n_ctx).bytes;
    static Q3PerDevice pd;
    if (lds > 65536 && !pd.ensure(lds, [&]() {
            hipError_t e = hipSuccess;
            for (const void* f : {(const void*)k_attend_kvq<2, true, K, V>, (const void*)k_attend_kvq<4, true, K, V>, (const void*)k_attend_kvq<1, false, K, V>,
                                  (const void*)k_attend_kvq<2, false, K, V>, (const void*)k_attend_kvq<4, false, K, V>})
                if (e == hipSuccess) e = att_allow_lds(f, lds);
            return e;
        })) return 1;
    if (k == KVQ_F2) hipLaunchKernelGGL((k_attend_kvq<2, true, K, V>), grid, dim3(512), lds, s, a);
    else if (k == KVQ_F4) hipLaunchKernelGGL((k_attend_kvq<4, true, K, V>), grid, dim3(1024), lds, s, a);
    else if (k == KVQ_N1) hipLaunchKernelGGL((k_attend_kvq<1, false, K, V>), grid, dim3(256), lds, s, a);
    else if (k == KVQ_N2) hipLaunchKernelGGL((k_attend_kvq<2, false, K, V>), grid, dim3(512), lds, s, a);
    else hipLaunchKernelGGL((k_attend_kvq<4, false, K, V>), grid, dim3(1024), lds, s, a);  // KVQ_N4
    return 0;
}
}  // namespace

int q3_launch_qk_prep_kvq(const Q3QkPrep& a, hipStream_t s) {
    if (a.hd != Q3_ATT_HD || !kvq_ok(a.kv8, a.kv4, a.tbl) || !a.kd || !a.vd || a.n_ctx <= 0 || a.n_ctx % 64) return 1;
    return KVQ_PAIR(a.kv4, launch_qk_prep, a, s);
}
// 0: launched (or n == 0); nonzero: refused, nothing launched
int q3_launch_kv_prefix_kvq(const Q3KvPrefix& a, hipStream_t s) {
    if (a.n <= 0) return 0;
    if (a.hd != Q3_ATT_HD || a.n > Q3_KVP_MAX || !kvq_ok(a.kv8, a.kv4, a.tbl) || !a.kd || !a.vd) return 1;
    hipLaunchKernelGGL(k_kv_prefix_kvq, dim3(a.L * 2 * a.Hkv, a.n), dim3(256), 0, s, a);
    return 0;
}
int q3_launch_kv_prefix_save_kvq(const Q3KvPrefix& a, hipStream_t s) {
    if (a.n <= 0) return 0;
    if (a.hd != Q3_ATT_HD || a.n > Q3_KVP_MAX || !kvq_ok(a.kv8, a.kv4, a.tbl) || !a.kd || !a.vd) return 1;
    hipLaunchKernelGGL(k_kv_prefix_save_kvq, dim3(a.L * 2 * a.Hkv, a.n), dim3(256), 0, s, a);
    return 0;
}

// The kernel q3_launch_attend_kvq takes (q3_attend_pick asks here when a.kv8 or a.kv4 is set; q3tts_k_attend_pick_kv8 / _kv4 report it),
// in the instance of the cache's pair: Q3_ATT8_* for Q8_0 / Q8_0, Q3_ATT4_* with Q4_0 blocks — one rule, two code bases. Whole prompt
// runs (admission, prefix creation; with or without a run table) take the non-fused k_attend_kvq<R, false>: there is no quantised form of
// k_attend_prefill, k_attend_small or k_attend_pair. One row per slot: k_attend_gqa2_kvq for two query heads per KV head (decode policy
// 1: k_attend_kvq<2, true>, the same bits), k_attend_kvq<4, true> for four. Q3_ATT_REFUSED: a pair kvq_ok refuses, a head size other
// than Q3_ATT_HD, a GQA ratio outside {1, 2, 4}, a fused launch without a second wave for k / v (R == 1), the Predictor's pass A
// (fused == 2).
int q3_attend_pick_kvq(const Q3Attend& a) {
    if (!kvq_ok(a.kv8, a.kv4, a.tbl) || a.hd != Q3_ATT_HD || a.Hkv <= 0 || a.Hq % a.Hkv) return Q3_ATT_REFUSED;
    const int R = a.Hq / a.Hkv;
    if ((R != 1 && R != 2 && R != 4) || (a.fused && R == 1) || a.fused < 0 || a.fused > 1) return Q3_ATT_REFUSED;
    const int base = kvq_code_base(a.kv4);
    if (a.fused) {
        int decode = 0, prefill = 0;
        q3_attend_policy_get(&decode, &prefill);
        if (R == 2) return base + (decode == 0 ? KVQ_GQA2 : KVQ_F2);
        return base + KVQ_F4;
    }
    return base + (R == 1 ? KVQ_N1 : (R == 2 ? KVQ_N2 : KVQ_N4));
}

// 0: launched. Nonzero: refused, nothing launched — a launch q3_attend_pick_kvq refuses, a cache without scales or with an n_ctx that is
// not whole key blocks, a fused launch whose append names other Q4_0 blocks than the cache, or a device that refuses the LDS size.
int q3_launch_attend_kvq(const Q3Attend& a, hipStream_t s) {
    const int pick = q3_attend_pick_kvq(a);
    if (pick == Q3_ATT_REFUSED || !a.kd || !a.vd || a.n_ctx <= 0 || a.n_ctx % 64) return 1;
    if (a.fused && (!a.prep.kd || !a.prep.vd || (a.kv4 && a.prep.kv4 != a.kv4))) return 1;
    return KVQ_PAIR(a.kv4, launch_attend, a, pick - kvq_code_base(a.kv4), s);
}

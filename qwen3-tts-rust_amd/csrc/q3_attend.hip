// q3_attend.hip — attention of the codec-token decoder on gfx950 (CDNA4): q/k RMSNorm + RoPE + KV append, the attention kernels over the
// cache in the ONE canonical order of DESIGN.md §4.4 (every variant gives the same bits), their launcher and the voice-prefix copy.
// Built with -ffp-contract=off: every fused multiply-add is an explicit fmaf.
#include "q3_kernels.h"

// ---------------------------------------------------------------------------------------------------
// q/k RMSNorm + RoPE + KV append. One wave per (row, head); hd == Q3_ATT_HD = 128 (lanes 0..31 own 4 elements each).
// K cache layout: per (slot, kv head) blocks of 64 keys, [block][hd/8 chunks][64 keys][8] bf16,
// so that the score kernel reads 1 KiB contiguous per wave-load with one key per lane. V is row-major [t][hd].
// ---------------------------------------------------------------------------------------------------
// four floats as two bf16 pairs (element i in the low half of word i / 2): 8 bytes of a K / V cache row
__device__ __forceinline__ uint2 pack_bf16x4(float a, float b, float c, float d) {
    return make_uint2((uint32_t)q3_bf16(a) | ((uint32_t)q3_bf16(b) << 16), (uint32_t)q3_bf16(c) | ((uint32_t)q3_bf16(d) << 16));
}
// where dims 4 lane .. 4 lane + 3 of the key at `pos` live in a head's K cache (khead = kc + hb * hd): chunk lane / 2, half lane & 1
__device__ __forceinline__ uint16_t* k_cache_elem(uint16_t* khead, int pos, int lane) {
    const int blk = pos >> 6, kl = pos & 63, c = lane >> 1, e0 = 4 * (lane & 1);
    return khead + ((size_t)(blk * (Q3_ATT_HD >> 3) + c) * 64 + kl) * 8 + e0;
}
// (prep_rinv / prep_norm / prep_rope / prep_arith / prep_head — RMSNorm + RoPE of one head by one wave — are in q3_kernels.h: the Q8_0-cache
// kernels of q3_attend_kv8.hip run the same statements)
// bf16 K (key-interleaved blocks; k_cache_elem's address for a run-time hd) and V (row-major) append of one kv head by lanes [0, hd/4)
__device__ __forceinline__ void kv_append(uint16_t* kc, uint16_t* vc, size_t hb, int hd, int pos, int lane, const float o[4], const float4 vv) {
    const int blk = pos >> 6, kl = pos & 63, c = lane >> 1, e0 = 4 * (lane & 1);
    *(uint2*)(kc + hb * hd + ((size_t)(blk * (hd >> 3) + c) * 64 + kl) * 8 + e0) = pack_bf16x4(o[0], o[1], o[2], o[3]);
    *(uint2*)(vc + (hb + pos) * hd + 4 * lane) = pack_bf16x4(vv.x, vv.y, vv.z, vv.w);
}

// The two chains of the canonical order. Hand copies remain only where calling the helper changed the compiled schedule
// of a decode-path kernel: prep_rope's loop in k_attend_gqa2 and k_attend_small's query wave, the output choice in k_attend_gqa2,
// k_attend_prefill and k_attend_pair, the K address in k_attend_pair (whose chains read float operands from LDS).
// Score: one 16-byte chunk of a key (8 bf16 dims, d ascending) onto the chain s; qa / qb = the query's 8 dims.
__device__ __forceinline__ float att_dot8(const float4 qa, const float4 qb, const uint4 k, float s) {
    s = fmaf(qa.x, q3_u2f(k.x << 16), s); s = fmaf(qa.y, q3_u2f(k.x & 0xffff0000u), s);
    s = fmaf(qa.z, q3_u2f(k.y << 16), s); s = fmaf(qa.w, q3_u2f(k.y & 0xffff0000u), s);
    s = fmaf(qb.x, q3_u2f(k.z << 16), s); s = fmaf(qb.y, q3_u2f(k.z & 0xffff0000u), s);
    s = fmaf(qb.z, q3_u2f(k.w << 16), s); s = fmaf(qb.w, q3_u2f(k.w & 0xffff0000u), s);
    return s;
}
// Value: 8 dims of one value row (16 bytes, bf16) times the key's weight pt onto the lane's 8 partial sums.
__device__ __forceinline__ void att_pv8(float pt, const uint4 v, float o[8]) {
    o[0] = fmaf(pt, q3_u2f(v.x << 16), o[0]); o[1] = fmaf(pt, q3_u2f(v.x & 0xffff0000u), o[1]);
    o[2] = fmaf(pt, q3_u2f(v.y << 16), o[2]); o[3] = fmaf(pt, q3_u2f(v.y & 0xffff0000u), o[3]);
    o[4] = fmaf(pt, q3_u2f(v.z << 16), o[4]); o[5] = fmaf(pt, q3_u2f(v.z & 0xffff0000u), o[5]);
    o[6] = fmaf(pt, q3_u2f(v.w << 16), o[6]); o[7] = fmaf(pt, q3_u2f(v.w & 0xffff0000u), o[7]);
}
// The value step for two heads that share the row (k_attend_gqa2): the row is decoded once, head 0's sums first, then head 1's.
__device__ __forceinline__ void att_pv8x2(float pa, float pb, const uint4 w, float o0[8], float o1[8]) {
    const float v0 = q3_u2f(w.x << 16), v1 = q3_u2f(w.x & 0xffff0000u), v2 = q3_u2f(w.y << 16), v3 = q3_u2f(w.y & 0xffff0000u);
    const float v4 = q3_u2f(w.z << 16), v5 = q3_u2f(w.z & 0xffff0000u), v6 = q3_u2f(w.w << 16), v7 = q3_u2f(w.w & 0xffff0000u);
    o0[0] = fmaf(pa, v0, o0[0]); o0[1] = fmaf(pa, v1, o0[1]); o0[2] = fmaf(pa, v2, o0[2]); o0[3] = fmaf(pa, v3, o0[3]);
    o0[4] = fmaf(pa, v4, o0[4]); o0[5] = fmaf(pa, v5, o0[5]); o0[6] = fmaf(pa, v6, o0[6]); o0[7] = fmaf(pa, v7, o0[7]);
    o1[0] = fmaf(pb, v0, o1[0]); o1[1] = fmaf(pb, v1, o1[1]); o1[2] = fmaf(pb, v2, o1[2]); o1[3] = fmaf(pb, v3, o1[3]);
    o1[4] = fmaf(pb, v4, o1[4]); o1[5] = fmaf(pb, v5, o1[5]); o1[6] = fmaf(pb, v6, o1[6]); o1[7] = fmaf(pb, v7, o1[7]);
}
// (att_out1 / att_out2 — the attention output in the form Q3Attend.out_bf16 names — are in q3_kernels.h)

// hd stays the run-time a.hd here (the launcher admits only Q3_ATT_HD): with the constant folded in, the kernel traced 80-140 ns per launch
// slower (4.76 -> 4.84-4.89 us at 31 rows x 24 heads; two runs of the same build differ by 0.02 us)
__global__ __launch_bounds__(64) void k_qk_prep(Q3QkPrep a) {
    const int row = blockIdx.x, hx = blockIdx.y, lane = threadIdx.x;
    int pos, slot;
    q3_row_map(row, a.row_pos, a.row_slot, a.slot_mod, a.pos_const, &pos, &slot);
    if (pos < 0) return;
    const int hd = a.hd, half = hd >> 1, nl = hd >> 2;
    const bool isq = hx < a.Hq;
    const int g = hx - a.Hq;
    float* src = a.qkv + (size_t)row * a.ld + (size_t)(isq ? hx : a.Hq + g) * hd;
    float o[4];
    prep_head(src, isq ? a.qnw : a.knw, a.eps, a.cs + (size_t)pos * half, a.sn + (size_t)pos * half, hd, lane, o);
    if (lane >= nl) return;
    if (isq) {
        ((float4*)src)[lane] = (float4){o[0], o[1], o[2], o[3]};
    } else {
        const float4 vv = ((const float4*)(a.qkv + (size_t)row * a.ld + (size_t)(a.Hq + a.Hkv + g) * hd))[lane];
        kv_append(a.kc, a.vc, ((size_t)slot * a.Hkv + g) * a.n_ctx, hd, pos, lane, o, vv);
    }
}
int q3_launch_qk_prep(const Q3QkPrep& a, hipStream_t s) {
    if (a.kv8) return q3_launch_qk_prep_kv8(a, s);  // Q8_0 cache: the quantising append of q3_attend_kv8.hip
    if (a.hd != Q3_ATT_HD) return 1;
    hipLaunchKernelGGL(k_qk_prep, dim3(a.rows, a.Hq + a.Hkv), dim3(64), 0, s, a);
    return 0;
}

// ---------------------------------------------------------------------------------------------------
// Attention over the cache, canonical order of DESIGN.md §4.4. Workgroup (kv head g, row): 4 waves per query
// head of the GQA group. Scores: one key per lane (256 virtual lanes = 4 waves), dot over d ascending.
// PV: 16 key-partials (u = t mod 16: wave u/4, lane group u%4), 16 lanes x 8 dims per key.
// ---------------------------------------------------------------------------------------------------
// FUSED (one row per slot, e.g. every decode step): the workgroup first does the q/k RMSNorm + RoPE + KV append of
// its own row (k_qk_prep's work) and serves the newest key/value from LDS, saving one launch per layer.
// its dynamic LDS: AttLds / att_lds of q3_kernels.h (the kernel and q3_launch_attend both ask there)
template <int R, bool FUSED>
__global__ __launch_bounds__(R * 256) void k_attend(Q3Attend a) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int g = blockIdx.x, row = blockIdx.y;
    Q3_STAMP(a, 0);
    int pos, slot;
    q3_row_map(row, a.row_pos, a.row_slot, a.slot_mod, a.pos_const, &pos, &slot);
    if (pos < 0) return;
    constexpr int hd = Q3_ATT_HD;
    const int T = pos + 1, Tcap = a.n_ctx;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, hh = wave >> 2, sw = wave & 3;
    const AttLds L = att_lds(R, Tcap);
    float* p_all = smem, * qh = smem + L.qh, * ow = smem + L.ow, * lw = smem + L.lw, * mw = smem + L.mw, * kh = smem + L.kh, * vh = smem + L.vh;
    const size_t hb = ((size_t)slot * a.Hkv + g) * a.n_ctx;
    if constexpr (FUSED) {
        const Q3QkPrep& pr = a.prep;
        constexpr int half = hd >> 1, nl = hd >> 2;
        const float* rowp = a.qkv + (size_t)row * a.ld;
        float o[4];
        if (sw == 0) {  // first wave of each query head: q-norm + RoPE -> LDS
            prep_head(rowp + (size_t)(g * R + hh) * hd, pr.qnw, pr.eps, pr.cs + (size_t)pos * half, pr.sn + (size_t)pos * half, hd, lane, o);
            if (lane < nl) *(float4*)(qh + hh * hd + 4 * lane) = (float4){o[0], o[1], o[2], o[3]};
        }
        if (wave == 1 || (R * 4 == 1)) {  // a second wave: k-norm + RoPE + append, v append
            prep_head(rowp + (size_t)(a.Hq + g) * hd, pr.knw, pr.eps, pr.cs + (size_t)pos * half, pr.sn + (size_t)pos * half, hd, lane, o);
            if (lane < nl) {
                const float4 vv = ((const float4*)(rowp + (size_t)(a.Hq + a.Hkv + g) * hd))[lane];
                kv_append(pr.kc, pr.vc, hb, hd, pos, lane, o, vv);
                // the newest key in the cache's own packed form (bf16 pairs, chunk c = 16 bytes at kh + 4 c words): the lane that owns it
                // then runs the same chain as every cached key (an LDS-fed float chain of its own cost ~1.5 us of this kernel)
                *(uint2*)((uint32_t*)kh + 2 * lane) = pack_bf16x4(o[0], o[1], o[2], o[3]);
                *(float4*)(vh + 4 * lane) = (float4){q3_round_bf16(vv.x), q3_round_bf16(vv.y), q3_round_bf16(vv.z), q3_round_bf16(vv.w)};
            }
        }
    } else {
        for (int i = tid; i < R * hd; i += R * 256) qh[i] = a.qkv[(size_t)row * a.ld + (size_t)g * R * hd + i];
    }
    __syncthreads();
    Q3_STAMP(a, 1);
    const uint16_t* kb = a.kc + hb * hd;
    const uint16_t* vb = a.vc + hb * hd;
    const float scale = 1.0f / sqrtf((float)hd);
    float* p = p_all + (size_t)hh * Tcap;
    const float* q = qh + hh * hd;
    float mloc = -INFINITY;
    for (int blk = sw; blk * 64 < T; blk += 4) {
        const int t = blk * 64 + lane;
        const uint4* kp = (const uint4*)(kb + (size_t)blk * 64 * hd) + lane;
        float s = 0.0f;
        // all 16 key chunks in flight at once (a runtime-bound loop issues load, use, load, use ...: measured 10 k of the kernel's 20 k
        // cycles at T <= 17 with in-kernel timestamps)
        uint4 kv[16];
#pragma unroll
        for (int c = 0; c < 16; ++c) kv[c] = kp[c * 64];
        if (FUSED && t == pos) {
#pragma unroll
            for (int c = 0; c < 16; ++c) kv[c] = *(const uint4*)((const uint32_t*)kh + 4 * c);
        }
#pragma unroll
        for (int c = 0; c < 16; ++c) s = att_dot8(*(const float4*)(q + c * 8), *(const float4*)(q + c * 8 + 4), kv[c], s);
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
    Q3_STAMP(a, 2);
    const int kg = lane >> 4, dl = lane & 15;
    float o[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) o[e] = 0.0f;
    // four value rows per trip, loaded together (a one-row loop issues load, use, load, use ... : one memory round trip per
    // 16 cached tokens); the chain of a lane still sees its keys in ascending order
    for (int t0 = 4 * sw + kg; t0 < T; t0 += 64) {
        uint4 vv[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) vv[u] = *(const uint4*)(vb + (size_t)min(t0 + 16 * u, T - 1) * hd + dl * 8);
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int t = t0 + 16 * u;
            if (t < T) {
                const float pt = p[t];
                if (FUSED && t == pos) {  // newest value: from LDS
#pragma unroll
                    for (int e = 0; e < 8; ++e) o[e] = fmaf(pt, vh[dl * 8 + e], o[e]);
                } else att_pv8(pt, vv[u], o);
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
        for (int e = 0; e < 8; ++e) ow[(hh * 4 + sw) * hd + dl * 8 + e] = o[e];
    }
    __syncthreads();
    Q3_STAMP(a, 3);
    for (int i = tid; i < R * hd; i += R * 256) {
        const int h2 = i / hd, d = i - h2 * hd;
        const float r0 = ow[(h2 * 4 + 0) * hd + d], r1 = ow[(h2 * 4 + 1) * hd + d], r2 = ow[(h2 * 4 + 2) * hd + d],
                    r3 = ow[(h2 * 4 + 3) * hd + d];
        const float ov = ((r0 + r1) + r2) + r3;
        const float l = ((lw[h2 * 4] + lw[h2 * 4 + 1]) + lw[h2 * 4 + 2]) + lw[h2 * 4 + 3];
        att_out1(a, row, g * R + h2, d, ov / l);  // (Q8: a half wave = one block)
    }
#ifdef Q3_STAMPS
    Q3_STAMP(a, 4);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    Q3_STAMP(a, 5);
#endif
}
// ---------------------------------------------------------------------------------------------------------------------
// Decode attention of a GQA PAIR (two query heads per KV head, hd = 128, one row per slot: every Talker step). Same canonical order as
// k_attend<2, true>, bit for bit, with the work laid out around what the in-kernel timestamps showed (tools/chain_stamps.hip: scores
// 5.2 us and value pass 3.4 us of a 12 us kernel at 150 cached keys, against ~6.3 us for its K / V bytes at the HBM rate):
//  * FOUR waves per (slot, KV head) instead of eight: wave sw owns the key blocks sw, sw + 4, ... for BOTH heads — a key block (and a
//    value row) is loaded once and used twice; the two heads' d-ascending fmaf chains are independent and interleave in the pipeline
//  * every wave requests its first key block and its first four value rows before the q / k / v preparation (waves 0, 1: the two query
//    heads; wave 2: k; wave 3: v), so the preparation runs under the memory latency instead of in front of it
//  * the newest key / value reach their lane through LDS in the cache's packed form: one code path for cached and newest keys
// ---------------------------------------------------------------------------------------------------------------------
// (Q3_LDS_BARRIER: q3_kernels.h)
__global__ __launch_bounds__(256, 2) void k_attend_gqa2(Q3Attend a) {  // (<= 256 registers: two workgroups per CU; unconstrained the compiler took 405)
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int g = blockIdx.x, row = blockIdx.y;
    Q3_STAMP(a, 0);
    int pos, slot;
    q3_row_map(row, a.row_pos, a.row_slot, a.slot_mod, a.pos_const, &pos, &slot);
    if (pos < 0) return;
    constexpr int hd = Q3_ATT_HD, half = hd >> 1, nl = hd >> 2;
    const int T = pos + 1, Tcap = a.n_ctx;
    const int tid = threadIdx.x, sw = tid >> 6, lane = tid & 63, kg = lane >> 4, dl = lane & 15;
    float* p0 = smem;                          // [Tcap] scores / probabilities of head 0
    float* p1 = p0 + Tcap;                     // [Tcap] head 1
    float* qh = p1 + Tcap;                     // [2][hd]
    float* ow = qh + 2 * hd;                   // [2][4][hd]
    float* lw = ow + 2 * 4 * hd;               // [2][4]
    float* mw = lw + 8;                        // [2][4]
    uint32_t* knew = (uint32_t*)(mw + 8);      // [64] newest key, bf16 pairs, chunk c = 16 bytes at knew + 4 c
    uint32_t* vnew = knew + 64;                // [64] newest value, bf16 pairs
    const Q3QkPrep& pr = a.prep;
    const size_t hb = ((size_t)slot * a.Hkv + g) * a.n_ctx;
    const uint16_t* kb = a.kc + hb * hd;
    const uint16_t* vb = a.vc + hb * hd;
    // Load order = the order of use (vmcnt retires in order): the row's own operands (L2, short latency) first, then the wave's first
    // key block (one key per lane, 16 KiB) and the value rows of its first FOUR trips (8 dims per lane; every cached key of a context of
    // <= 256) — all from HBM, all in flight while the preparation runs. (Cache loads first made the preparation wait ~5 us for them.)
    const float* rowp = a.qkv + (size_t)row * a.ld;
    const float* src = rowp + (size_t)(sw < 2 ? g * 2 + sw : (sw == 2 ? a.Hq + g : a.Hq + a.Hkv + g)) * hd;
    float4 x4 = (float4){0.f, 0.f, 0.f, 0.f}, w4 = x4, c4 = (float4){1.f, 1.f, 1.f, 1.f}, s4 = x4;
    if (lane < nl) {
        x4 = ((const float4*)src)[lane];
        if (sw < 3) {
            w4 = ((const float4*)(sw < 2 ? pr.qnw : pr.knw))[lane];
            c4 = *(const float4*)(pr.cs + (size_t)pos * half + 4 * (lane & 15)); s4 = *(const float4*)(pr.sn + (size_t)pos * half + 4 * (lane & 15));
        }
    }
    __builtin_amdgcn_sched_barrier(0);
    {   // preparation of this row: q heads (waves 0, 1), k (wave 2: norm + RoPE + append), v (wave 3: append)
        if (sw < 3) {  // prep_arith's steps, the rotation written out (see the note at att_dot8)
            float y[4];
            prep_norm(x4, prep_rinv(x4, pr.eps, hd), w4, y);
            const float cc[4] = {c4.x, c4.y, c4.z, c4.w}, ss[4] = {s4.x, s4.y, s4.z, s4.w};
            float o[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float other = __shfl_xor(y[e], 16);
                o[e] = (lane < 16) ? fmaf(-other, ss[e], y[e] * cc[e]) : fmaf(other, ss[e], y[e] * cc[e]);
            }
            if (lane < nl) {
                if (sw < 2) *(float4*)(qh + sw * hd + 4 * lane) = (float4){o[0], o[1], o[2], o[3]};
                else {
                    const uint2 kk = pack_bf16x4(o[0], o[1], o[2], o[3]);
                    *(uint2*)k_cache_elem(pr.kc + hb * hd, pos, lane) = kk;
                    *(uint2*)(knew + 2 * lane) = kk;
                }
            }
        } else if (lane < nl) {
            const uint2 vk = pack_bf16x4(x4.x, x4.y, x4.z, x4.w);
            *(uint2*)(pr.vc + (hb + pos) * hd + 4 * lane) = vk;
            *(uint2*)(vnew + 2 * lane) = vk;
        }
    }
    // The cache operands are requested only now: the vector L1 returns loads in issue order across the waves of a CU, so HBM misses issued
    // ahead of the preparation's (L2-hit) operands held every wave's preparation back by the HBM latency (first barrier at 4.9 us instead of 1.9).
    // vv[0..1]: value rows of the first two trips; vv[2..3] (keys 128..255) follow once the key block's registers are free, under the softmax phases
    __builtin_amdgcn_sched_barrier(0);
    uint4 kv[16], vv[4][4];
    {
        const uint4* kp = (const uint4*)(kb + (size_t)min(sw, (T - 1) >> 6) * 64 * hd) + lane;
#pragma unroll
        for (int c = 0; c < 16; ++c) kv[c] = kp[c * 64];
#pragma unroll
        for (int tr = 0; tr < 2; ++tr)
#pragma unroll
            for (int u = 0; u < 4; ++u) vv[tr][u] = *(const uint4*)(vb + (size_t)min(64 * tr + 4 * sw + kg + 16 * u, T - 1) * hd + dl * 8);
    }
    __builtin_amdgcn_sched_barrier(0);
    Q3_LDS_BARRIER();
    Q3_STAMP(a, 1);
    const float scale = 1.0f / sqrtf((float)hd);
    float ml0 = -INFINITY, ml1 = -INFINITY;
    for (int blk = sw; blk * 64 < T; blk += 4) {
        const int t = blk * 64 + lane;
        if (blk != sw) {  // (contexts beyond 256 keys: the following blocks of this wave)
            const uint4* kp = (const uint4*)(kb + (size_t)blk * 64 * hd) + lane;
#pragma unroll
            for (int c = 0; c < 16; ++c) kv[c] = kp[c * 64];
        }
        if (t == pos) {
#pragma unroll
            for (int c = 0; c < 16; ++c) kv[c] = *(const uint4*)(knew + 4 * c);
        }
        float s0 = 0.0f, s1 = 0.0f;
#pragma unroll
        for (int c = 0; c < 16; ++c) {
            const float4 qa = *(const float4*)(qh + c * 8), qb = *(const float4*)(qh + c * 8 + 4);
            const float4 ra = *(const float4*)(qh + hd + c * 8), rb = *(const float4*)(qh + hd + c * 8 + 4);
            s0 = att_dot8(qa, qb, kv[c], s0);
            s1 = att_dot8(ra, rb, kv[c], s1);
        }
        s0 = s0 * scale; s1 = s1 * scale;
        if (t < T) { p0[t] = s0; p1[t] = s1; ml0 = fmaxf(ml0, s0); ml1 = fmaxf(ml1, s1); }
    }
#pragma unroll
    for (int tr = 2; tr < 4; ++tr)
#pragma unroll
        for (int u = 0; u < 4; ++u) vv[tr][u] = *(const uint4*)(vb + (size_t)min(64 * tr + 4 * sw + kg + 16 * u, T - 1) * hd + dl * 8);
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
    Q3_STAMP(a, 2);
    float o0[8], o1[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) { o0[e] = 0.0f; o1[e] = 0.0f; }
    const uint4 vn = *(const uint4*)(vnew + 4 * dl);
#pragma unroll
    for (int tr = 0; tr < 4; ++tr) {  // the first four trips: value rows already in registers
        const int t0 = 64 * tr + 4 * sw + kg;
        if (64 * tr >= T) break;  // (uniform)
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int t = t0 + 16 * u;
            if (t < T) {
                const float pa = p0[t], pb = p1[t];
                const uint4 w = (t == pos) ? vn : vv[tr][u];
                att_pv8x2(pa, pb, w, o0, o1);
            }
        }
    }
    for (int t0 = 256 + 4 * sw + kg; t0 < T; t0 += 64) {  // contexts beyond 256 keys: four value rows loaded together per trip (ascending keys per lane, as above)
        uint4 vl[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) vl[u] = *(const uint4*)(vb + (size_t)min(t0 + 16 * u, T - 1) * hd + dl * 8);
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int t = t0 + 16 * u;
            if (t < T) {
                const float pa = p0[t], pb = p1[t];
                const uint4 w = (t == pos) ? vn : vl[u];
                att_pv8x2(pa, pb, w, o0, o1);
            }
        }
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        o0[e] = o0[e] + __shfl_xor(o0[e], 16); o0[e] = o0[e] + __shfl_xor(o0[e], 32);
        o1[e] = o1[e] + __shfl_xor(o1[e], 16); o1[e] = o1[e] + __shfl_xor(o1[e], 32);
    }
    if (kg == 0) {
        *(float4*)(ow + (0 * 4 + sw) * hd + dl * 8) = (float4){o0[0], o0[1], o0[2], o0[3]}; *(float4*)(ow + (0 * 4 + sw) * hd + dl * 8 + 4) = (float4){o0[4], o0[5], o0[6], o0[7]};
        *(float4*)(ow + (1 * 4 + sw) * hd + dl * 8) = (float4){o1[0], o1[1], o1[2], o1[3]}; *(float4*)(ow + (1 * 4 + sw) * hd + dl * 8 + 4) = (float4){o1[4], o1[5], o1[6], o1[7]};
    }
    Q3_LDS_BARRIER();
    Q3_STAMP(a, 3);
    if (tid < 128) {  // two consecutive dims of one head per thread: one 4-byte store of the bf16 pair
        const int h2 = tid >> 6, d0 = 2 * (tid & 63);
        const float l = ((lw[h2 * 4] + lw[h2 * 4 + 1]) + lw[h2 * 4 + 2]) + lw[h2 * 4 + 3];
        float ov[2];
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const int d = d0 + q;
            const float r0 = ow[(h2 * 4 + 0) * hd + d], r1 = ow[(h2 * 4 + 1) * hd + d], r2 = ow[(h2 * 4 + 2) * hd + d], r3 = ow[(h2 * 4 + 3) * hd + d];
            ov[q] = (((r0 + r1) + r2) + r3) / l;
        }
        const int hq = g * 2 + h2;
        if (a.out_bf16 == 2) q3_q8_out2x16(ov[0], ov[1], row, hq * hd + d0, (a.Hq * hd) >> 6, a.out_rt16, (int8_t*)a.out, a.out_scale);  // W8A8: Q8_0 blocks (16 lanes x 2 dims)
        else if (a.out_bf16) *(uint32_t*)((uint16_t*)a.out + q3_atile_off(row, hq * hd + d0, (a.Hq * hd) >> 5)) = (uint32_t)q3_bf16(ov[0]) | ((uint32_t)q3_bf16(ov[1]) << 16);
        else *(float2*)(a.out + (size_t)row * a.ldo + (size_t)hq * hd + d0) = make_float2(ov[0], ov[1]);
    }
#ifdef Q3_STAMPS
    Q3_STAMP(a, 4);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    Q3_STAMP(a, 5);
#endif
}

// ---------------------------------------------------------------------------------------------------------------------
// The same attention for short caches (n_ctx <= 64: the Predictor's <= 17 keys per frame), one row per slot. Every output follows the
// canonical order of k_attend bit for bit. Built around the kernel's dependent chain, measured with in-kernel timestamps
// (tools/chain_stamps.hip: the round-2 kernel spent 3.2 us before its first barrier on three dependent load round trips, 2.0 us on two
// divergent LDS-fed score chains and 1.7 us on the value pass with 64 cross-lane shuffles):
//  * workgroup = R query-head waves + ONE wave for k (lanes 0-31: RMSNorm + RoPE + append) and v (lanes 32-63: append); every global
//    operand of a wave — row segments, norm weights, RoPE entries, the cached keys (one key per lane, 16 chunks) and the first 16 cached
//    value rows (2 dims per lane) — is requested before anything is computed: one round trip
//  * the newest key reaches lane `pos` of the query waves through LDS in the cache's own packed layout, so cached and newest keys run the
//    SAME d-ascending fmaf chain (one code path); q is read back from LDS as broadcast 16-byte reads
//  * value pass without shuffles: a lane owns 2 output dims and keeps all 16 key partials u = t mod 16 of them in registers; p_t comes
//    from v_readlane (a scalar); r_w = (o_4w + o_4w+1) + (o_4w+2 + o_4w+3), o = ((r0 + r1) + r2) + r3 are plain adds in the lane
//  * l = the 64-lane butterfly of wave 0 of k_attend (+0 +0 +0 for the three absent waves is exact)
// ---------------------------------------------------------------------------------------------------------------------
//
// The GATHERING form (TX = Q3AttGather: q3_launch_attend_gather) serves block 0 of the greedy Predictor's passes q >= 1,
// whose input row is a table row chosen by the code of pass q - 1: every wave requests the row's per-tile argmax keys FIRST, then the
// operands that do not depend on the code (cached keys / values, norm weights, RoPE entries) — still one round trip — reduces the keys to
// the code k_pred_next<false> takes (the largest key; q3_argmax_idx) and only then requests its segment of tab[code]: the one added
// dependent round trip. From rowp on the two forms are the same statements: same chains, same append, same bits as the plain form fed
// that row. Workgroup column blockIdx.x == Hkv is att_gather_book: k_pred_next's bookkeeping, off the query waves' chain.
__device__ __forceinline__ const Q3AttGather& att_gather(const Q3AttGather& t) { return t; }
// the wave's share of the row's keys (parts lane, lane + 64: every part of a codebook of <= 2048 codes), requested; the rest by loop.
// Unconditional loads (a lane past the end re-reads the last part, which changes no maximum): straight-line code, nothing waits here.
__device__ __forceinline__ void att_keys_load(const Q3AttGather& t, int row, int lane, unsigned long long kk[2]) {
    const unsigned long long* kr = t.keys + (size_t)row * t.n_key_parts;
    kk[0] = kr[min(lane, t.n_key_parts - 1)];
    kk[1] = kr[min(lane + 64, t.n_key_parts - 1)];
}
// ... reduced to the row's code as k_pred_next<false> does (a maximum: any order gives the same key), and the table row it selects. Any
// 64-bit pattern in the keys (an idle row's leftovers) gives a row inside the table.
__device__ __forceinline__ int att_keys_code(const Q3AttGather& t, int row, int lane, const unsigned long long kk[2]) {
    unsigned long long k = kk[1] > kk[0] ? kk[1] : kk[0];
    for (int p = lane + 128; p < t.n_key_parts; p += 64) { const unsigned long long o = t.keys[(size_t)row * t.n_key_parts + p]; k = o > k ? o : k; }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) { const unsigned long long o = __shfl_xor(k, m); k = o > k ? o : k; }
    return __builtin_amdgcn_readfirstlane(q3_argmax_idx(k));
}
__device__ __forceinline__ bool att_code_ok(const Q3AttGather& t, int code) { return code >= 0 && code < t.tab_rows; }
// What k_pred_next<false>(q) does besides the row's norm inputs, for row b, by one workgroup of NT threads: the same values, element by element
// (fb + codec_q[code], or + 0 for a code out of range, in f32; the px row copied). Skips a row whose slot is not active, as k_pred_next does.
template <int NT>
__device__ __forceinline__ void att_gather_book(const Q3AttGather& t, int b, int tid) {
    unsigned long long kk[2];
    att_keys_load(t, b, tid & 63, kk);
    const int slot = t.row_slot[b];
    const Q3Slot* sl = t.slots + slot;
    const int active = sl->active, frame = sl->n_frames;
    const int code = att_keys_code(t, b, tid & 63, kk);  // (every wave reduces the whole row: no LDS, no barrier)
    if (!active) return;
    const bool ok = att_code_ok(t, code);
    if (tid == 0) t.codes[((size_t)slot * t.max_steps_cap + frame) * t.ncb + t.q] = code;
    const float4* e = (const float4*)(t.codec_q + (size_t)(ok ? code : 0) * t.d);
    const float4* pr = (const float4*)(ok ? t.pproj_q + (size_t)code * t.dp : t.proj_b);
    float4* fb = (float4*)(t.fb + (size_t)b * t.d);
    float4* px = (float4*)(t.px + (size_t)b * t.dp);
    for (int i = tid; i < (t.d >> 2); i += NT) {
        const float4 f = fb[i], ev = ok ? e[i] : (float4){0.f, 0.f, 0.f, 0.f};
        fb[i] = (float4){f.x + ev.x, f.y + ev.y, f.z + ev.z, f.w + ev.w};
    }
    for (int i = tid; i < (t.dp >> 2); i += NT) px[i] = pr[i];
}
template <int R, class... TX>
__global__ __launch_bounds__((R + 1) * 64) void k_attend_small(Q3Attend a, TX... tx) {
    constexpr bool GATHER = sizeof...(TX) != 0;
    __shared__ __attribute__((aligned(16))) float qh[R][Q3_ATT_HD]; // q after norm + RoPE (f32)
    __shared__ __attribute__((aligned(16))) uint32_t knew[64];     // newest key, bf16 pairs in the cache's chunk order: chunk c = 16 bytes at knew + 4 c
    __shared__ __attribute__((aligned(16))) uint32_t vnew[64];     // newest value, bf16 pairs: dims 2 i, 2 i + 1 in word i
    const int g = blockIdx.x, row = blockIdx.y, wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if constexpr (GATHER) {
        if (g == a.Hkv) { att_gather_book<(R + 1) * 64>(att_gather(tx...), row, threadIdx.x); return; }
    }
    Q3_STAMP(a, 0);
    int pos, slot;
    q3_row_map(row, a.row_pos, a.row_slot, a.slot_mod, a.pos_const, &pos, &slot);
    if (pos < 0) return;
    constexpr int hd = Q3_ATT_HD, half = hd >> 1, nl = hd >> 2;
    const int T = pos + 1;
    const Q3QkPrep& pr = a.prep;
    const size_t hb = ((size_t)slot * a.Hkv + g) * a.n_ctx;
    const uint16_t* kb = a.kc + hb * hd;
    const uint16_t* vb = a.vc + hb * hd;
    const float* rowp = a.qkv + (size_t)row * a.ld;
    const float* csp = pr.cs + (size_t)pos * half + 4 * (lane & 15);
    const float* snp = pr.sn + (size_t)pos * half + 4 * (lane & 15);
    unsigned long long kk[2] = {0ull, 0ull};
    if constexpr (GATHER) att_keys_load(att_gather(tx...), row, lane, kk);
    if (wv == R) {
        // ---- k (lanes 0..31) and v (lanes 32..63) of this row: norm + RoPE, bf16, append, and the LDS copies the query waves read
        const bool isk = lane < nl;
        float4 w4 = (float4){0.f, 0.f, 0.f, 0.f}, c4 = (float4){1.f, 1.f, 1.f, 1.f}, s4 = (float4){0.f, 0.f, 0.f, 0.f};
        if constexpr (GATHER) {  // (the code-independent operands go out before the keys are waited for)
            if (isk) { w4 = ((const float4*)pr.knw)[lane]; c4 = *(const float4*)csp; s4 = *(const float4*)snp; }
            const Q3AttGather& t = att_gather(tx...);
            __builtin_amdgcn_sched_barrier(0);  // (keep the reduction, and its wait, behind every request above)
            const int code = att_keys_code(t, row, lane, kk);
            rowp = t.tab + (size_t)(att_code_ok(t, code) ? code : t.tab_rows) * a.ld;
        }
        const float4 x4 = isk ? ((const float4*)(rowp + (size_t)(a.Hq + g) * hd))[lane] : ((const float4*)(rowp + (size_t)(a.Hq + a.Hkv + g) * hd))[lane - nl];
        if constexpr (!GATHER) {
            if (isk) { w4 = ((const float4*)pr.knw)[lane]; c4 = *(const float4*)csp; s4 = *(const float4*)snp; }
        }
        // (lanes >= 32, which hold v, contribute +0 to the sum of squares, as in prep_head)
        const float4 v = isk ? x4 : (float4){0.f, 0.f, 0.f, 0.f};
        float o[4];
        prep_arith(v, w4, c4, s4, pr.eps, lane, o);
        if (isk) {
            const uint2 kk = pack_bf16x4(o[0], o[1], o[2], o[3]);
            *(uint2*)k_cache_elem(pr.kc + hb * hd, pos, lane) = kk;
            *(uint2*)(knew + 2 * lane) = kk;   // elements 4 lane .. 4 lane + 3 = chunk lane / 2, half lane & 1
        } else {
            const int j = lane - nl;
            const uint2 vk = pack_bf16x4(x4.x, x4.y, x4.z, x4.w);
            *(uint2*)(pr.vc + (hb + pos) * hd + 4 * j) = vk;
            *(uint2*)(vnew + 2 * j) = vk;
        }
        Q3_STAMP(a, 1);
        __syncthreads();
        return;
    }
    // ---- query head wv: operands first
    const int hq = g * R + wv;
    uint4 kv[16];
    uint32_t vv[16];
#pragma unroll
    for (int c = 0; c < 16; ++c) kv[c] = lane < pos ? ((const uint4*)kb)[c * 64 + lane] : make_uint4(0, 0, 0, 0);
#pragma unroll
    for (int u = 0; u < 16; ++u) vv[u] = u < pos ? *(const uint32_t*)(vb + (size_t)u * hd + 2 * lane) : 0u;
    float4 x4 = (float4){0.f, 0.f, 0.f, 0.f}, w4 = x4, c4 = (float4){1.f, 1.f, 1.f, 1.f}, s4 = x4;
    if constexpr (GATHER) {  // the row segment alone waits for the code
        if (lane < nl) { w4 = ((const float4*)pr.qnw)[lane]; c4 = *(const float4*)csp; s4 = *(const float4*)snp; }
        const Q3AttGather& t = att_gather(tx...);
        __builtin_amdgcn_sched_barrier(0);
        const int code = att_keys_code(t, row, lane, kk);
        rowp = t.tab + (size_t)(att_code_ok(t, code) ? code : t.tab_rows) * a.ld;
        if (lane < nl) x4 = ((const float4*)(rowp + (size_t)hq * hd))[lane];
    } else {
    if (lane < nl) { x4 = ((const float4*)(rowp + (size_t)hq * hd))[lane]; w4 = ((const float4*)pr.qnw)[lane]; c4 = *(const float4*)csp; s4 = *(const float4*)snp; }
    }
    {
        float y[4];
        prep_norm(x4, prep_rinv(x4, pr.eps, hd), w4, y);
        const float cc[4] = {c4.x, c4.y, c4.z, c4.w}, ss[4] = {s4.x, s4.y, s4.z, s4.w};
        float o[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float other = __shfl_xor(y[e], 16);
            o[e] = (lane < 16) ? fmaf(-other, ss[e], y[e] * cc[e]) : fmaf(other, ss[e], y[e] * cc[e]);
        }
        if (lane < nl) *(float4*)(qh[wv] + 4 * lane) = (float4){o[0], o[1], o[2], o[3]};
    }
    Q3_STAMP(a, 1);
    __syncthreads();
    Q3_STAMP(a, 2);
    if (lane == pos) {  // the newest key, in the packed form the cached keys arrive in
#pragma unroll
        for (int c = 0; c < 16; ++c) kv[c] = *(const uint4*)(knew + 4 * c);
    }
    const float* q = qh[wv];
    float sc = 0.0f;
#pragma unroll
    for (int c = 0; c < 16; ++c)
        sc = att_dot8(*(const float4*)(q + c * 8), *(const float4*)(q + c * 8 + 4), kv[c], sc);
    sc = sc * (1.0f / sqrtf((float)hd));
    const float m = wave_max(lane < T ? sc : -INFINITY);
    const float e = lane < T ? q3_expf(sc - m) : 0.0f;
    float l = wave_sum(e);
    l = ((l + 0.0f) + 0.0f) + 0.0f;
#ifdef Q3_STAMPS
    asm volatile("" :: "v"(l)); Q3_STAMP(a, 3);
#endif
    // value pass: this lane's dims d0 = 2 lane, d0 + 1; partial u holds the keys t = u, u + 16, ... in ascending order
    float o0[16], o1[16];
#pragma unroll
    for (int u = 0; u < 16; ++u) { o0[u] = 0.0f; o1[u] = 0.0f; }
    const uint32_t vn = vnew[lane];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        if (16 * c >= T) break;  // (uniform)
#pragma unroll
        for (int u = 0; u < 16; ++u) {
            const int t = 16 * c + u;
            if (t >= T) break;  // (uniform)
            uint32_t w;
            if (t == pos) w = vn;
            else if (c == 0) w = vv[u];
            else w = *(const uint32_t*)(vb + (size_t)t * hd + 2 * lane);  // (caches beyond 16 keys: not the shipped Predictor)
            const float pt = __uint_as_float(__builtin_amdgcn_readlane(__float_as_uint(e), t));  // (t is uniform: a scalar broadcast, no LDS)
            o0[u] = fmaf(pt, q3_u2f(w << 16), o0[u]);
            o1[u] = fmaf(pt, q3_u2f(w & 0xffff0000u), o1[u]);
        }
    }
    float r0[4], r1[4];
#pragma unroll
    for (int w = 0; w < 4; ++w) {
        r0[w] = (o0[4 * w] + o0[4 * w + 1]) + (o0[4 * w + 2] + o0[4 * w + 3]);
        r1[w] = (o1[4 * w] + o1[4 * w + 1]) + (o1[4 * w + 2] + o1[4 * w + 3]);
    }
    const float ov0 = (((r0[0] + r0[1]) + r0[2]) + r0[3]) / l, ov1 = (((r1[0] + r1[1]) + r1[2]) + r1[3]) / l;
    const int d0 = 2 * lane;
    att_out2(a, row, hq, d0, ov0, ov1);  // (Q8: the whole query wave is here)
#ifdef Q3_STAMPS
    Q3_STAMP(a, 4);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    Q3_STAMP(a, 5);
#endif
}

// ---------------------------------------------------------------------------------------------------------------------
// Pass A of the Predictor: TWO rows per slot in one launch — row b at position 0 (the projected hidden row), row slot_mod + b at
// position 1 (the first code row) — and nothing cached yet. One workgroup per (KV group, slot): its four waves are (row, query head);
// k / v of both rows are prepared into LDS (and appended to the cache for the later passes), so no wave reads the cache and the
// separate k_qk_prep launch is not needed. Scores, softmax and PV follow k_attend_small's expressions term by term with every key
// served from LDS (the bf16-rounded values the cache holds): same chains, same order, same bits.
// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_attend_pair(Q3Attend a) {
    __shared__ __attribute__((aligned(16))) float kh[2][128], vh[2][128], qh[2][2][128], ps[2][2][64];
    const int g = blockIdx.x, b = blockIdx.y, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int rr = wave >> 1, hh = wave & 1, R = 2, hd = 128;
    const int row = rr * a.slot_mod + b, slot = b, pos = rr;
    const Q3QkPrep& pr = a.prep;
    const size_t hb = ((size_t)slot * a.Hkv + g) * a.n_ctx;
    const float* rowp = a.qkv + (size_t)row * a.ld;
    const int half = hd >> 1, nl = hd >> 2;
    float qo[4], o4[4];
    prep_head(rowp + (size_t)(g * R + hh) * hd, pr.qnw, pr.eps, pr.cs + (size_t)pos * half, pr.sn + (size_t)pos * half, hd, lane, qo);
    if (lane < nl) *(float4*)(qh[rr][hh] + 4 * lane) = (float4){qo[0], qo[1], qo[2], qo[3]};
    if (hh == 0) {  // k of this row: norm + RoPE + append
        prep_head(rowp + (size_t)(a.Hq + g) * hd, pr.knw, pr.eps, pr.cs + (size_t)pos * half, pr.sn + (size_t)pos * half, hd, lane, o4);
        if (lane < nl) {
            const int blk = pos >> 6, kl = pos & 63, c = lane >> 1, e0 = 4 * (lane & 1);
            *(uint2*)(pr.kc + hb * hd + ((size_t)(blk * (hd >> 3) + c) * 64 + kl) * 8 + e0) = pack_bf16x4(o4[0], o4[1], o4[2], o4[3]);
            *(float4*)(kh[rr] + 4 * lane) = (float4){q3_round_bf16(o4[0]), q3_round_bf16(o4[1]), q3_round_bf16(o4[2]), q3_round_bf16(o4[3])};
        }
    } else if (lane < nl) {  // v of this row: append
        const float4 v4 = ((const float4*)(rowp + (size_t)(a.Hq + a.Hkv + g) * hd))[lane];
        *(float4*)(vh[rr] + 4 * lane) = (float4){q3_round_bf16(v4.x), q3_round_bf16(v4.y), q3_round_bf16(v4.z), q3_round_bf16(v4.w)};
        *(uint2*)(pr.vc + (hb + pos) * hd + 4 * lane) = pack_bf16x4(v4.x, v4.y, v4.z, v4.w);
    }
    __syncthreads();
    const int T = pos + 1;
    const float* q = qh[rr][hh];
    const float scale = 1.0f / sqrtf((float)hd);
    float sc = 0.0f;
    if (lane < T) {  // key `lane`: the d-ascending chain
        const float* kk = kh[lane];
        for (int d = 0; d < hd; d += 4) {
            const float4 qa = *(const float4*)(q + d), ka = *(const float4*)(kk + d);
            sc = fmaf(qa.x, ka.x, sc); sc = fmaf(qa.y, ka.y, sc); sc = fmaf(qa.z, ka.z, sc); sc = fmaf(qa.w, ka.w, sc);
        }
    }
    sc = sc * scale;
    const float m = wave_max(lane < T ? sc : -INFINITY);
    const float e = lane < T ? q3_expf(sc - m) : 0.0f;
    ps[rr][hh][lane] = e;
    float l = wave_sum(e);
    l = ((l + 0.0f) + 0.0f) + 0.0f;
    const int kg = lane >> 4, dl = lane & 15;
    float out8[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) out8[i] = 0.0f;
#pragma unroll
    for (int uu = 0; uu < 4; ++uu) {
        float o[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) o[i] = 0.0f;
        for (int t = 4 * uu + kg; t < T; t += 16) {
            const float pt = ps[rr][hh][t];
#pragma unroll
            for (int i = 0; i < 8; ++i) o[i] = fmaf(pt, vh[t][dl * 8 + i], o[i]);
        }
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            float r = o[i] + __shfl_xor(o[i], 16);
            r = r + __shfl_xor(r, 32);
            out8[i] = uu == 0 ? r : out8[i] + r;
        }
    }
    if (a.out_bf16 == 2) {  // W8A8: Q8_0 blocks — a lane owns 8 consecutive dims, lanes dl ^ 1, dl ^ 2 the rest of its block (every lane group holds the same sums)
        float ov8[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) ov8[i] = out8[i] / l;
        q3_q8_out8x4(ov8, row, (g * R + hh) * hd + dl * 8, (a.Hq * hd) >> 6, a.out_rt16, (int8_t*)a.out, a.out_scale, kg == 0);
    } else if (kg == 0) {
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int d = dl * 8 + i;
            const float ov = out8[i] / l;
            if (a.out_bf16) ((uint16_t*)a.out)[q3_atile_off(row, (g * R + hh) * hd + d, (a.Hq * hd) >> 5)] = q3_bf16(ov);
            else a.out[(size_t)row * a.ldo + (size_t)(g * R + hh) * hd + d] = ov;
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// Prefill attention of a whole prompt run: one workgroup per (KV head, slot) keeps the run's keys (in the cache's packed block form) and
// values in LDS and its 8 waves each take (row, query head) tasks — k_attend<2, false> starts one 8-wave workgroup per (row, KV head) that
// fetches the same keys again (23 500 workgroups for 64 prompts: 220 us per layer). hd = 128, two query heads per KV head, runs of
// n <= 128 rows at positions pos0 .. pos0 + n - 1 with pos0 + n <= 256 (what admit_group builds; pos0 > 0 behind a voice prefix, whose keys
// and values are already in the slot's cache). Row r attends to keys [0, pos0 + r]; the workgroup stages all pos0 + n of them.
// The canonical order is k_attend's, element for element:
//   score t: the d-ascending fmaf chain of lane t % 64 over block t / 64, times the scale; maximum over all t;
//   weights: q3_expf(score - max); their sum: per key-block class sw = block % 4 the lanes' sums in block order, the 64-lane butterfly,
//            then ((l0 + l1) + l2) + l3;
//   value pass: 16 partials per (row, head, 8 dims) — class u = t % 16 lives in lane group kg = u % 4 of class sw = u / 4, keys ascending —
//            combined (kg0 + kg1) + (kg2 + kg3) by the two shuffles, then ((r0 + r1) + r2) + r3 over sw; output = sum / l.
// A wave runs the four sw classes one after the other where k_attend runs them on four waves: the same sums in the same order.
// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(512) void k_attend_prefill(Q3Attend a) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int g = blockIdx.x, sg = blockIdx.y, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int row0 = a.seg[4 * sg], n = a.seg[4 * sg + 1], slot = a.seg[4 * sg + 2], pos0 = a.seg[4 * sg + 3];
    constexpr int hd = Q3_ATT_HD;
    const int nk = pos0 + n;                                    // keys (and values) the run attends to
    const int nblk = (nk + 63) >> 6;
    const int pw = a.seg_max_t > 128 ? (a.seg_max_t + 63) & ~63 : 128;  // weights per wave: the launch's longest run (q3_launch_attend sizes LDS alike)
    uint4* kl = (uint4*)smem;                                  // [nblk][16 chunks][64 lanes]: a key block as the cache stores it
    uint4* vl = kl + (size_t)nblk * 1024;                       // [nk][16]: value rows
    float* scr = (float*)(vl + (size_t)nk * 16) + wave * (pw + 128);  // per wave: weights p[pw] | query q[128]
    float* p = scr; float* q = scr + pw;
    const size_t hb = ((size_t)slot * a.Hkv + g) * a.n_ctx;
    {
        const uint4* kb = (const uint4*)(a.kc + hb * hd);
        const uint4* vb = (const uint4*)(a.vc + hb * hd);
        for (int i = tid; i < nblk * 1024; i += 512) kl[i] = kb[i];
        for (int i = tid; i < nk * 16; i += 512) vl[i] = vb[i];
    }
    __syncthreads();
    const float scale = 1.0f / sqrtf((float)hd);
    const int kg = lane >> 4, dl = lane & 15;
    for (int task = wave; task < 2 * n; task += 8) {
        const int r = task >> 1, hh = task & 1, row = row0 + r, T = pos0 + r + 1;
        {
            const float2 qv = *(const float2*)(a.qkv + (size_t)row * a.ld + (size_t)(g * 2 + hh) * hd + 2 * lane);
            *(float2*)(q + 2 * lane) = qv;
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // (one wave: its LDS operations complete in order; the compiler must not reorder around this)
        float mloc = -INFINITY;
        for (int blk = 0; blk * 64 < T; ++blk) {
            const int t = blk * 64 + lane;
            const uint4* kp = kl + (size_t)blk * 1024 + lane;
            float s = 0.0f;
#pragma unroll
            for (int c = 0; c < 16; ++c) s = att_dot8(*(const float4*)(q + c * 8), *(const float4*)(q + c * 8 + 4), kp[c * 64], s);
            s = s * scale;
            if (t < T) { p[t] = s; mloc = fmaxf(mloc, s); }
        }
        const float m = wave_max(mloc);
        float lw[4] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
        for (int sw = 0; sw < 4; ++sw) {
            float lsum = 0.0f;
            for (int blk = sw; blk * 64 < T; blk += 4) {
                const int t = blk * 64 + lane;
                if (t < T) { const float e = q3_expf(p[t] - m); p[t] = e; lsum += e; }
            }
            lw[sw] = wave_sum(lsum);
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        float rsw[4][8];
#pragma unroll
        for (int sw = 0; sw < 4; ++sw) {
            float o[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) o[e] = 0.0f;
            for (int t0 = 4 * sw + kg; t0 < T; t0 += 64) {
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int t = t0 + 16 * u;
                    if (t < T) { const uint4 vv = vl[(size_t)t * 16 + dl]; att_pv8(p[t], vv, o); }
                }
            }
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                o[e] = o[e] + __shfl_xor(o[e], 16);
                o[e] = o[e] + __shfl_xor(o[e], 32);
                rsw[sw][e] = o[e];
            }
        }
        const float l = ((lw[0] + lw[1]) + lw[2]) + lw[3];
        if (a.out_bf16 == 2) {  // W8A8: the head's output as Q8_0 blocks — a lane owns 8 consecutive dims, lanes dl ^ 1, dl ^ 2 the rest of its block
            float ov8[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) ov8[e] = (((rsw[0][e] + rsw[1][e]) + rsw[2][e]) + rsw[3][e]) / l;
            q3_q8_out8x4(ov8, row, (g * 2 + hh) * hd + dl * 8, (a.Hq * hd) >> 6, a.out_rt16, (int8_t*)a.out, a.out_scale, kg == 0);
        } else if (kg == 0) {
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const float ov = ((rsw[0][e] + rsw[1][e]) + rsw[2][e]) + rsw[3][e];
                const int d = dl * 8 + e, col = (g * 2 + hh) * hd + d;
                if (a.out_bf16) ((uint16_t*)a.out)[q3_atile_off(row, col, (a.Hq * hd) >> 5)] = q3_bf16(ov / l);
                else a.out[(size_t)row * a.ldo + col] = ov / l;
            }
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // the next task overwrites p / q
    }
}

// Which kernel serves the Talker's decode attention / the prefill of whole prompts. The variants produce the same bits
// (tests/test_parity_gpu.py compares them in one process through q3tts_k_attend_policy); the environment variables Q3TTS_ATT_OLD /
// Q3TTS_ATT_PREFILL_OLD give the initial values once per process (A/B runs).
//   decode:  0 = k_attend_gqa2 (default), 1 = k_attend<2, true>
//   prefill: 0 = k_attend_prefill when the launch has >= 128 (run, KV head) workgroups (default), 1 = never (k_attend<2, false>), 2 = whenever eligible
static int g_att_decode = 0, g_att_prefill = 0;
static std::once_flag g_att_once;
static void att_policy_init() {
    std::call_once(g_att_once, []() {
        const char* ev = getenv("Q3TTS_ATT_OLD"); g_att_decode = (ev && atoi(ev)) ? 1 : 0;
        ev = getenv("Q3TTS_ATT_PREFILL_OLD"); g_att_prefill = (ev && atoi(ev)) ? 1 : 0;
    });
}
void q3_attend_policy(int decode, int prefill) { att_policy_init(); g_att_decode = decode; g_att_prefill = prefill; }
void q3_attend_policy_get(int* decode, int* prefill) { att_policy_init(); *decode = g_att_decode; *prefill = g_att_prefill; }

// dynamic LDS above 64 KiB has to be allowed per kernel (and per device); a refused attribute is a refused launch
static hipError_t att_allow_lds(const void* kernel, size_t lds) { return hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds); }

// The kernel q3_launch_attend takes for a launch, under the current policies (the one place that decides; q3tts_k_attend_pick asks here too).
// Q3_ATT_REFUSED: a head size other than Q3_ATT_HD, a GQA ratio outside {1, 2, 4}, a fused launch without a second wave for k / v (R == 1),
// or the pair kernel for another ratio than 2.
int q3_attend_pick(const Q3Attend& a) {
    att_policy_init();
    if (a.kv8) return q3_attend_pick_kv8(a);  // Q8_0 cache: one of the six kernels of q3_attend_kv8.hip, never one of the nine below
    if (a.hd != Q3_ATT_HD || a.Hkv <= 0 || a.Hq % a.Hkv) return Q3_ATT_REFUSED;
    const int R = a.Hq / a.Hkv;
    if ((R != 1 && R != 2 && R != 4) || (a.fused && R == 1) || (a.fused == 2 && R != 2)) return Q3_ATT_REFUSED;
    if (a.fused == 2) return Q3_ATT_PAIR;  // two rows per slot, empty cache (the Predictor's pass A): see k_attend_pair
    if (a.fused && a.n_ctx <= 64 && R == 2) return Q3_ATT_SMALL2;  // short caches (the Predictor): one wave per query head
    // the Talker's decode step: one workgroup of four waves per (slot, KV head), both query heads
    // (1: k_attend<2, true> below — same bits: test_attention_kernel_variants_agree)
    if (a.fused && R == 2 && g_att_decode == 0) return Q3_ATT_GQA2;
    // whole prompt runs (admit_group): keys and values once per run — when there are enough runs to occupy the chip (one workgroup per run and
    // KV head walks its rows 8 at a time: a single prompt of 31 rows took 45 us per layer on 8 workgroups against 9 us on k_attend's 248)
    // With voice prefixes a run attends to pos0 + n keys: up to 256 of them still fit (4 key blocks of 16 KiB + 256 values of 256 B + 8 waves
    // x (256 + 128) floats = 140 KiB); without prefixes seg_max_t = seg_max_n and the rule and the LDS size are what they were.
    if (!a.fused && R == 2 && a.seg && a.seg_max_n <= 128 && a.seg_max_t <= 256 && g_att_prefill != 1 &&
        (a.n_seg * a.Hkv >= 128 || g_att_prefill == 2)) return Q3_ATT_PREFILL;
    if (a.fused) return R == 2 ? Q3_ATT_F2 : Q3_ATT_F4;
    return R == 1 ? Q3_ATT_N1 : (R == 2 ? Q3_ATT_N2 : Q3_ATT_N4);
}

// 0: launched. Nonzero: refused, nothing launched — a shape q3_attend_pick refuses, or a device that refuses the LDS size.
int q3_launch_attend(const Q3Attend& a, hipStream_t s) {
    if (a.kv8) return q3_launch_attend_kv8(a, s);
    const int pick = q3_attend_pick(a);
    if (pick == Q3_ATT_REFUSED) return 1;
    const int R = a.Hq / a.Hkv;
    const dim3 grid(a.Hkv, a.rows);
    if (pick == Q3_ATT_PAIR) {
        hipLaunchKernelGGL(k_attend_pair, dim3(a.Hkv, a.slot_mod), dim3(256), 0, s, a);
        return 0;
    }
    if (pick == Q3_ATT_SMALL2) {
        hipLaunchKernelGGL((k_attend_small<2>), grid, dim3(192), 0, s, a);
        return 0;
    }
    if (pick == Q3_ATT_GQA2) {
        const size_t lds2 = ((size_t)2 * a.n_ctx + 2 * Q3_ATT_HD + 8 * Q3_ATT_HD + 16 + 128) * sizeof(float);  // as k_attend_gqa2 lays it out
        static Q3PerDevice pd2;
        if (lds2 > 65536 && !pd2.ensure(lds2, [&]() { return att_allow_lds((const void*)k_attend_gqa2, lds2); })) return 1;
        hipLaunchKernelGGL(k_attend_gqa2, grid, dim3(256), lds2, s, a);
        return 0;
    }
    if (pick == Q3_ATT_PREFILL) {
        const int nblk = (a.seg_max_t + 63) / 64;
        const int pw = a.seg_max_t > 128 ? (a.seg_max_t + 63) & ~63 : 128;  // as k_attend_prefill computes it
        const size_t lds3 = (size_t)nblk * 16384 + (size_t)a.seg_max_t * 256 + (size_t)8 * (pw + 128) * sizeof(float);
        static Q3PerDevice pd3;
        if (lds3 > 65536 && !pd3.ensure(lds3, [&]() { return att_allow_lds((const void*)k_attend_prefill, lds3); })) return 1;
        hipLaunchKernelGGL(k_attend_prefill, dim3(a.Hkv, a.n_seg), dim3(512), lds3, s, a);
        return 0;
    }
    // k_attend: R * 4 waves per (row, KV head); the score buffer is R * n_ctx floats
    const size_t lds = att_lds(R, a.n_ctx).bytes;
    static Q3PerDevice pd;
    if (lds > 65536 && !pd.ensure(lds, [&]() {
            hipError_t e = hipSuccess;
            for (const void* k : {(const void*)k_attend<2, true>, (const void*)k_attend<4, true>, (const void*)k_attend<1, false>,
                                  (const void*)k_attend<2, false>, (const void*)k_attend<4, false>})
                if (e == hipSuccess) e = att_allow_lds(k, lds);
            return e;
        })) return 1;
    if (pick == Q3_ATT_F2) hipLaunchKernelGGL((k_attend<2, true>), grid, dim3(512), lds, s, a);
    else if (pick == Q3_ATT_F4) hipLaunchKernelGGL((k_attend<4, true>), grid, dim3(1024), lds, s, a);
    else if (pick == Q3_ATT_N1) hipLaunchKernelGGL((k_attend<1, false>), grid, dim3(256), lds, s, a);
    else if (pick == Q3_ATT_N2) hipLaunchKernelGGL((k_attend<2, false>), grid, dim3(512), lds, s, a);
    else hipLaunchKernelGGL((k_attend<4, false>), grid, dim3(1024), lds, s, a);  // Q3_ATT_N4
    return 0;
}

// The gathering form exists for k_attend_small<2> only: any other launch is refused, as is one whose table or bookkeeping is incomplete.
int q3_launch_attend_gather(const Q3Attend& a, const Q3AttGather& t, hipStream_t s) {
    if (q3_attend_pick(a) != Q3_ATT_SMALL2 || a.rows < 1) return 1;
    if (!t.tab || t.tab_rows < 1 || !t.keys || t.n_key_parts < 1 || t.q < 1 || t.q >= t.ncb || !t.codec_q || !t.slots || !t.row_slot || !t.codes ||
        t.max_steps_cap < 1 || !t.fb || !t.pproj_q || !t.proj_b || !t.px || t.d < 4 || (t.d & 3) || t.dp < 4 || (t.dp & 3)) return 1;
#ifdef Q3_STAMPS
    if (a.dbg) return 1;  // (the stamp buffer is laid out for Hkv workgroup columns)
#endif
    hipLaunchKernelGGL((k_attend_small<2, Q3AttGather>), dim3(a.Hkv + 1, a.rows), dim3(192), 0, s, a, t);
    return 0;
}

// Voice prefixes: one workgroup per (layer, K or V, KV head) and entry copies a prefix store into its slot with 16-byte loads and stores.
// The store is read once per entry, so its loads stay cacheable (plain loads, plain stores).
__global__ __launch_bounds__(256) void k_kv_prefix(Q3KvPrefix a) {
    const int j = blockIdx.y, isv = blockIdx.x & 1, lg = blockIdx.x >> 1, l = lg / a.Hkv, g = lg - l * a.Hkv;
    const int P = a.P[j], np = (P + 63) & ~63;
    const size_t src = ((size_t)l * a.Hkv + g) * np * a.hd;
    const size_t dst = (size_t)l * a.layer_stride + ((size_t)a.slot[j] * a.Hkv + g) * a.n_ctx * a.hd;
    const int n16 = (isv ? P : np) * (a.hd >> 3);  // whole key blocks; values of positions < P
    const uint4* sp = (const uint4*)((isv ? a.pv[j] : a.pk[j]) + src);
    uint4* dp = (uint4*)((isv ? a.vc : a.kc) + dst);
    for (int i = threadIdx.x; i < n16; i += 256) dp[i] = sp[i];
}
void q3_launch_kv_prefix(const Q3KvPrefix& a, hipStream_t s) {
    if (a.n <= 0) return;
    if (a.kv8) { q3_launch_kv_prefix_kv8(a, s); return; }
    hipLaunchKernelGGL(k_kv_prefix, dim3(a.L * 2 * a.Hkv, a.n), dim3(256), 0, s, a);
}

// The inverse (sessions): the first P positions of slot[j] into the store pk[j] / pv[j], which becomes byte for byte what
// q3tts_prefix_create writes for the same rows. That store is zero outside positions < P, so the keys P .. np - 1 of the last block —
// in the slot they are the request's own rows, or an earlier occupant's — are written as zeros, and values stop at P (the store comes
// zero-filled from its allocator). 16-byte unit i of a head's keys holds key (i & 63) of block i / (8 hd).
__global__ __launch_bounds__(256) void k_kv_prefix_save(Q3KvPrefix a) {
    const int j = blockIdx.y, isv = blockIdx.x & 1, lg = blockIdx.x >> 1, l = lg / a.Hkv, g = lg - l * a.Hkv;
    const int P = a.P[j], np = (P + 63) & ~63;
    const size_t dst = ((size_t)l * a.Hkv + g) * np * a.hd;
    const size_t src = (size_t)l * a.layer_stride + ((size_t)a.slot[j] * a.Hkv + g) * a.n_ctx * a.hd;
    const uint4* sp = (const uint4*)((isv ? a.vc : a.kc) + src);
    uint4* dp = (uint4*)(const_cast<uint16_t*>(isv ? a.pv[j] : a.pk[j]) + dst);
    if (isv) {
        const int n16 = P * (a.hd >> 3);
        for (int i = threadIdx.x; i < n16; i += 256) dp[i] = sp[i];
        return;
    }
    const int n16 = np * (a.hd >> 3), per_blk = a.hd * 8;
    for (int i = threadIdx.x; i < n16; i += 256) {
        const int pos = (i / per_blk) * 64 + (i & 63);
        uint4 v = make_uint4(0u, 0u, 0u, 0u);
        if (pos < P) v = sp[i];
        dp[i] = v;
    }
}
int q3_launch_kv_prefix_save(const Q3KvPrefix& a, hipStream_t s) {
    if (a.n <= 0) return 0;
    if (a.hd != Q3_ATT_HD || a.n > Q3_KVP_MAX) return 1;
    if (a.kv8) return q3_launch_kv_prefix_save_kv8(a, s);
    hipLaunchKernelGGL(k_kv_prefix_save, dim3(a.L * 2 * a.Hkv, a.n), dim3(256), 0, s, a);
    return 0;
}

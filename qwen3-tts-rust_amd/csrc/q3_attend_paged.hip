// q3_attend_paged.hip — the Talker's attention over a PAGED bf16 K/V cache (q3tts_engine_options.kv_pages): the append, the
// attention kernels in the ONE canonical order of DESIGN.md §4.4, their launcher and the voice-prefix copies. The kernels of q3_attend.hip
// are untouched; their launchers hand over here when a table is set (Q3QkPrep / Q3Attend / Q3KvPrefix .tbl).
//
// Layout. A layer's pool is [pages][Hkv][64 * hd] bf16 for K and the same for V: page p of KV head g starts at (p * Hkv + g) * 64 * hd. A K
// page is one 64-key block in the contiguous cache's interleaved form ([hd/8 chunks][64 keys][8]), a V page 64 row-major rows, so inside a
// page every address is the contiguous kernels' with the block number taken out. tbl[slot * tbl_stride + (pos >> 6)] names the page that
// holds pos; one entry serves every layer, every head and both K and V. Page 0 is never handed out and stays zero: an entry a slot does
// not own is 0, so the loads some kernels issue before they know whether they need them stay inside the pool (no result depends on them).
//
// What paging costs a kernel: ONE table entry per 64-position block, read at a wave-uniform address (the slot's row, the block number) and
// held in a scalar register; the page's base replaces blk * 64 * hd in the address. Every kernel here walks K and V 64 positions at a
// time as its contiguous form does — a trip of the value pass never crosses a 64-boundary, clamped rows (min(t, T - 1)) stay in the trip's
// block — so no arithmetic changes: order, LDS layout, wave split and output forms are q3_attend.hip's, and so is every bit.
// Built with -ffp-contract=off as q3_attend.hip.
#include "q3_kernels.h"

namespace {
constexpr int HD = Q3_ATT_HD;
constexpr int PG = 64 * HD;  // bf16 elements of one (page, KV head): a 64-key block, or 64 value rows

// entry blk of a slot's table row, in a scalar register (the address is the same in every lane)
__device__ __forceinline__ int pg_of(const int* trow, int blk) { return __builtin_amdgcn_readfirstlane(trow[blk]); }
// where (page, KV head g) starts in a layer's pool, in elements
__device__ __forceinline__ size_t pg_off(int page, int Hkv, int g) { return ((size_t)page * Hkv + g) * PG; }
// dims 4 lane .. 4 lane + 3 of the key / value at `pos` into their page (kpage / vpage: the page of block pos >> 6), lanes [0, hd/4)
__device__ __forceinline__ void pg_put_k(uint16_t* kpage, int pos, int lane, uint2 kk) { *(uint2*)k_cache_elem(kpage, pos & 63, lane) = kk; }
__device__ __forceinline__ void pg_put_v(uint16_t* vpage, int pos, int lane, uint2 vk) { *(uint2*)(vpage + (size_t)(pos & 63) * HD + 4 * lane) = vk; }

// k_qk_prep with the append through the table: one wave per (row, head)
__global__ __launch_bounds__(64) void k_qk_prep_paged(Q3QkPrep a) {
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
    if (lane >= nl) return;
    if (isq) {
        ((float4*)src)[lane] = (float4){o[0], o[1], o[2], o[3]};
    } else {
        const float4 vv = ((const float4*)(a.qkv + (size_t)row * a.ld + (size_t)(a.Hq + a.Hkv + g) * HD))[lane];
        const size_t po = pg_off(pg_of(a.tbl + (size_t)slot * a.tbl_stride, pos >> 6), a.Hkv, g);
        pg_put_k(a.kc + po, pos, lane, pack_bf16x4(o[0], o[1], o[2], o[3]));
        pg_put_v(a.vc + po, pos, lane, pack_bf16x4(vv.x, vv.y, vv.z, vv.w));
    }
}

// ---------------------------------------------------------------------------------------------------
// k_attend's structure over pages: workgroup (kv head g, row), 4 waves per query head of the GQA group. Scores: one key per lane, wave sw
// owns the key blocks sw, sw + 4, ... — one table entry per block. PV: 16 key-partials, 16 lanes x 8 dims per key; a trip covers the 64
// positions of one block — one entry per trip. FUSED: the workgroup prepares and appends its own row first. LDS: att_lds (q3_kernels.h).
// ---------------------------------------------------------------------------------------------------
template <int R, bool FUSED>
__global__ __launch_bounds__(R * 256) void k_attend_paged(Q3Attend a) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int g = blockIdx.x, row = blockIdx.y;
    int pos, slot;
    q3_row_map(row, a.row_pos, a.row_slot, a.slot_mod, a.pos_const, &pos, &slot);
    if (pos < 0) return;
    constexpr int hd = HD;
    const int T = pos + 1, Tcap = a.n_ctx;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, hh = wave >> 2, sw = wave & 3;
    const AttLds L = att_lds(R, Tcap);
    float* p_all = smem, * qh = smem + L.qh, * ow = smem + L.ow, * lw = smem + L.lw, * mw = smem + L.mw, * kh = smem + L.kh, * vh = smem + L.vh;
    const int* trow = a.tbl + (size_t)slot * a.tbl_stride;
    if constexpr (FUSED) {
        const Q3QkPrep& pr = a.prep;
        constexpr int half = hd >> 1, nl = hd >> 2;
        const float* rowp = a.qkv + (size_t)row * a.ld;
        float o[4];
        if (sw == 0) {  // first wave of each query head: q-norm + RoPE -> LDS
            prep_head(rowp + (size_t)(g * R + hh) * hd, pr.qnw, pr.eps, pr.cs + (size_t)pos * half, pr.sn + (size_t)pos * half, hd, lane, o);
            if (lane < nl) *(float4*)(qh + hh * hd + 4 * lane) = (float4){o[0], o[1], o[2], o[3]};
        }
        if (wave == 1) {  // a second wave: k-norm + RoPE + append, v append
            prep_head(rowp + (size_t)(a.Hq + g) * hd, pr.knw, pr.eps, pr.cs + (size_t)pos * half, pr.sn + (size_t)pos * half, hd, lane, o);
            const size_t po = pg_off(pg_of(trow, pos >> 6), a.Hkv, g);
            if (lane < nl) {
                const float4 vv = ((const float4*)(rowp + (size_t)(a.Hq + a.Hkv + g) * hd))[lane];
                const uint2 kk = pack_bf16x4(o[0], o[1], o[2], o[3]);
                pg_put_k(pr.kc + po, pos, lane, kk);
                pg_put_v(pr.vc + po, pos, lane, pack_bf16x4(vv.x, vv.y, vv.z, vv.w));
                *(uint2*)((uint32_t*)kh + 2 * lane) = kk;  // the newest key in the cache's packed form, as k_attend keeps it
                *(float4*)(vh + 4 * lane) = (float4){q3_round_bf16(vv.x), q3_round_bf16(vv.y), q3_round_bf16(vv.z), q3_round_bf16(vv.w)};
            }
        }
    } else {
        for (int i = tid; i < R * hd; i += R * 256) qh[i] = a.qkv[(size_t)row * a.ld + (size_t)g * R * hd + i];
    }
    __syncthreads();
    const float scale = 1.0f / sqrtf((float)hd);
    float* p = p_all + (size_t)hh * Tcap;
    const float* q = qh + hh * hd;
    float mloc = -INFINITY;
    for (int blk = sw; blk * 64 < T; blk += 4) {
        const int t = blk * 64 + lane;
        const uint4* kp = (const uint4*)(a.kc + pg_off(pg_of(trow, blk), a.Hkv, g)) + lane;
        float s = 0.0f;
        uint4 kv[16];  // all 16 key chunks in flight at once
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
    const int kg = lane >> 4, dl = lane & 15;
    float o[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) o[e] = 0.0f;
    // four value rows per trip, loaded together; trip n reads positions [64 n, 64 n + 64): one page (4 sw + kg + 48 < 64, and a row
    // clamped to T - 1 lies between t0 and t0 + 48)
    for (int trip = 0, t0 = 4 * sw + kg; t0 < T; ++trip, t0 += 64) {
        const uint16_t* vp = a.vc + pg_off(pg_of(trow, trip), a.Hkv, g) + dl * 8;
        uint4 vv[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) vv[u] = *(const uint4*)(vp + (size_t)(min(t0 + 16 * u, T - 1) & 63) * hd);
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
    for (int i = tid; i < R * hd; i += R * 256) {
        const int h2 = i / hd, d = i - h2 * hd;
        const float r0 = ow[(h2 * 4 + 0) * hd + d], r1 = ow[(h2 * 4 + 1) * hd + d], r2 = ow[(h2 * 4 + 2) * hd + d],
                    r3 = ow[(h2 * 4 + 3) * hd + d];
        const float ov = ((r0 + r1) + r2) + r3;
        const float l = ((lw[h2 * 4] + lw[h2 * 4 + 1]) + lw[h2 * 4 + 2]) + lw[h2 * 4 + 3];
        att_out1(a, row, g * R + h2, d, ov / l);
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// k_attend_gqa2 over pages (two query heads per KV head, one row per slot: every Talker step): four waves per (slot, KV head), wave sw owns
// the key blocks sw, sw + 4, ... for both heads; every wave requests its first key block and the value rows of its first trips around the
// q / k / v preparation exactly where k_attend_gqa2 does. Those requests need pages, and a page is a dependent load — so the five table
// entries a wave can need before its first barrier (blocks 0 .. 3, each clamped to the last block the row reaches, and the last block
// itself for the append) are requested FIRST, ahead of the row's own operands: they are scalar loads of one cache line that L2 holds (the
// host wrote the row once, at admission) and have returned long before the preparation's operands have. Blocks 4 and up (contexts
// beyond 256 keys) are looked up in their loops, one entry per block.
// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256, 2) void k_attend_gqa2_paged(Q3Attend a) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int g = blockIdx.x, row = blockIdx.y;
    int pos, slot;
    q3_row_map(row, a.row_pos, a.row_slot, a.slot_mod, a.pos_const, &pos, &slot);
    if (pos < 0) return;
    constexpr int hd = HD, half = hd >> 1, nl = hd >> 2;
    const int T = pos + 1, Tcap = a.n_ctx;
    const int tid = threadIdx.x, sw = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63, kg = lane >> 4, dl = lane & 15;
    float* p0 = smem;                          // [Tcap] scores / probabilities of head 0
    float* p1 = p0 + Tcap;                     // [Tcap] head 1
    float* qh = p1 + Tcap;                     // [2][hd]
    float* ow = qh + 2 * hd;                   // [2][4][hd]
    float* lw = ow + 2 * 4 * hd;               // [2][4]
    float* mw = lw + 8;                        // [2][4]
    uint32_t* knew = (uint32_t*)(mw + 8);      // [64] newest key, bf16 pairs, chunk c = 16 bytes at knew + 4 c
    uint32_t* vnew = knew + 64;                // [64] newest value, bf16 pairs
    const Q3QkPrep& pr = a.prep;
    const int* trow = a.tbl + (size_t)slot * a.tbl_stride;
    const int last = pos >> 6;                 // the last block the row reaches: the append's, and what every early request clamps to
    const int pg0 = pg_of(trow, 0), pg1 = pg_of(trow, min(1, last)), pg2 = pg_of(trow, min(2, last)), pg3 = pg_of(trow, min(3, last)),
              pgw = pg_of(trow, last);
    const size_t hs = (size_t)a.Hkv * PG, go = (size_t)g * PG;  // page stride and this head's offset inside a page, in elements
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
        if (sw < 3) {
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
                    pg_put_k(pr.kc + pgw * hs + go, pos, lane, kk);
                    *(uint2*)(knew + 2 * lane) = kk;
                }
            }
        } else if (lane < nl) {
            const uint2 vk = pack_bf16x4(x4.x, x4.y, x4.z, x4.w);
            pg_put_v(pr.vc + pgw * hs + go, pos, lane, vk);
            *(uint2*)(vnew + 2 * lane) = vk;
        }
    }
    // the cache operands are requested only now, as in k_attend_gqa2 (HBM misses ahead of the preparation's operands held it back)
    __builtin_amdgcn_sched_barrier(0);
    uint4 kv[16], vv[4][4];
    {
        const int pgk = sw == 0 ? pg0 : (sw == 1 ? pg1 : (sw == 2 ? pg2 : pg3));  // block min(sw, last)
        const uint4* kp = (const uint4*)(a.kc + pgk * hs + go) + lane;
#pragma unroll
        for (int c = 0; c < 16; ++c) kv[c] = kp[c * 64];
#pragma unroll
        for (int tr = 0; tr < 2; ++tr) {
            const uint16_t* vp = a.vc + (tr == 0 ? pg0 : pg1) * hs + go + dl * 8;  // rows clamped to T - 1 lie in block min(tr, last)
#pragma unroll
            for (int u = 0; u < 4; ++u) vv[tr][u] = *(const uint4*)(vp + (size_t)(min(64 * tr + 4 * sw + kg + 16 * u, T - 1) & 63) * hd);
        }
    }
    __builtin_amdgcn_sched_barrier(0);
    Q3_LDS_BARRIER();
    const float scale = 1.0f / sqrtf((float)hd);
    float ml0 = -INFINITY, ml1 = -INFINITY;
    for (int blk = sw; blk * 64 < T; blk += 4) {
        const int t = blk * 64 + lane;
        if (blk != sw) {  // (contexts beyond 256 keys: the following blocks of this wave)
            const uint4* kp = (const uint4*)(a.kc + pg_of(trow, blk) * hs + go) + lane;
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
    for (int tr = 2; tr < 4; ++tr) {
        const uint16_t* vp = a.vc + (tr == 2 ? pg2 : pg3) * hs + go + dl * 8;
#pragma unroll
        for (int u = 0; u < 4; ++u) vv[tr][u] = *(const uint4*)(vp + (size_t)(min(64 * tr + 4 * sw + kg + 16 * u, T - 1) & 63) * hd);
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
    for (int trip = 4, t0 = 256 + 4 * sw + kg; t0 < T; ++trip, t0 += 64) {  // contexts beyond 256 keys: one page per trip
        const uint16_t* vp = a.vc + pg_of(trow, trip) * hs + go + dl * 8;
        uint4 vl[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) vl[u] = *(const uint4*)(vp + (size_t)(min(t0 + 16 * u, T - 1) & 63) * hd);
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
    if (tid < 128) {  // two consecutive dims of one head per thread
        const int h2 = tid >> 6, d0 = 2 * (tid & 63);
        const float l = ((lw[h2 * 4] + lw[h2 * 4 + 1]) + lw[h2 * 4 + 2]) + lw[h2 * 4 + 3];
        float ov[2];
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const int d = d0 + q;
            const float r0 = ow[(h2 * 4 + 0) * hd + d], r1 = ow[(h2 * 4 + 1) * hd + d], r2 = ow[(h2 * 4 + 2) * hd + d], r3 = ow[(h2 * 4 + 3) * hd + d];
            ov[q] = (((r0 + r1) + r2) + r3) / l;
        }
        att_out2(a, row, g * 2 + h2, d0, ov[0], ov[1]);
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// k_attend_prefill over pages: one workgroup per (KV head, run) stages the run's keys and values in LDS — block by block, one table entry
// each, into the places the contiguous kernel copies them to — and its 8 waves then take (row, query head) tasks from LDS alone: from
// the first barrier on this is k_attend_prefill statement for statement.
// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(512) void k_attend_prefill_paged(Q3Attend a) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int g = blockIdx.x, sg = blockIdx.y, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int row0 = a.seg[4 * sg], n = a.seg[4 * sg + 1], slot = a.seg[4 * sg + 2], pos0 = a.seg[4 * sg + 3];
    constexpr int hd = HD;
    const int nk = pos0 + n;                                    // keys (and values) the run attends to
    const int nblk = (nk + 63) >> 6;
    const int pw = a.seg_max_t > 128 ? (a.seg_max_t + 63) & ~63 : 128;  // weights per wave: the launch's longest run
    uint4* kl = (uint4*)smem;                                  // [nblk][16 chunks][64 lanes]: a key block as its page stores it
    uint4* vl = kl + (size_t)nblk * 1024;                       // [nk][16]: value rows
    float* scr = (float*)(vl + (size_t)nk * 16) + wave * (pw + 128);  // per wave: weights p[pw] | query q[128]
    float* p = scr; float* q = scr + pw;
    const int* trow = a.tbl + (size_t)slot * a.tbl_stride;
    for (int blk = 0; blk < nblk; ++blk) {
        const size_t po = pg_off(pg_of(trow, blk), a.Hkv, g);
        const uint4* kb = (const uint4*)(a.kc + po);
        const uint4* vb = (const uint4*)(a.vc + po);
        const int nv = min(nk - blk * 64, 64) * 16;            // 16-byte units of the block's value rows below nk
        for (int i = tid; i < 1024; i += 512) kl[blk * 1024 + i] = kb[i];
        for (int i = tid; i < nv; i += 512) vl[blk * 1024 + i] = vb[i];
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
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // (one wave: its LDS operations complete in order)
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
        if (a.out_bf16 == 2) {  // W8A8: a lane owns 8 consecutive dims, lanes dl ^ 1, dl ^ 2 the rest of its Q8_0 block
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

// Voice prefixes through the table: one workgroup per (layer, K or V, KV head) and entry, block by block. The store keeps its contiguous
// form ([L][Hkv][np * hd], np = ceil(P / 64) * 64): block b of a head is 1024 16-byte units of keys, or 64 rows x 16 units of values, at
// unit 1024 b of the head — and at unit 0 of page tbl[slot][b]. Whole key blocks and the values of positions < P are copied, as
// k_kv_prefix copies them.
__global__ __launch_bounds__(256) void k_kv_prefix_paged(Q3KvPrefix a) {
    const int j = blockIdx.y, isv = blockIdx.x & 1, lg = blockIdx.x >> 1, l = lg / a.Hkv, g = lg - l * a.Hkv;
    const int P = a.P[j], np = (P + 63) & ~63;
    const uint4* sp = (const uint4*)((isv ? a.pv[j] : a.pk[j]) + ((size_t)l * a.Hkv + g) * np * HD);
    uint16_t* pool = (isv ? a.vc : a.kc) + (size_t)l * a.layer_stride;
    const int* trow = a.tbl + (size_t)a.slot[j] * a.tbl_stride;
    for (int blk = 0; blk * 64 < np; ++blk) {
        uint4* dp = (uint4*)(pool + pg_off(pg_of(trow, blk), a.Hkv, g));
        const int n16 = isv ? min(P - blk * 64, 64) * 16 : 1024;
        for (int i = threadIdx.x; i < n16; i += 256) dp[i] = sp[blk * 1024 + i];
    }
}
// The inverse (k_kv_prefix_save's rules): positions < P of the slot into the zero-filled store; the keys P .. np - 1 of the last block are
// written as zeros (in the slot they are the request's own rows), values stop at P. Unit i of a key block holds key i & 63.
__global__ __launch_bounds__(256) void k_kv_prefix_save_paged(Q3KvPrefix a) {
    const int j = blockIdx.y, isv = blockIdx.x & 1, lg = blockIdx.x >> 1, l = lg / a.Hkv, g = lg - l * a.Hkv;
    const int P = a.P[j], np = (P + 63) & ~63;
    uint4* dp = (uint4*)(const_cast<uint16_t*>(isv ? a.pv[j] : a.pk[j]) + ((size_t)l * a.Hkv + g) * np * HD);
    const uint16_t* pool = (isv ? a.vc : a.kc) + (size_t)l * a.layer_stride;
    const int* trow = a.tbl + (size_t)a.slot[j] * a.tbl_stride;
    for (int blk = 0; blk * 64 < np; ++blk) {
        const uint4* sp = (const uint4*)(pool + pg_off(pg_of(trow, blk), a.Hkv, g));
        if (isv) {
            const int n16 = min(P - blk * 64, 64) * 16;
            for (int i = threadIdx.x; i < n16; i += 256) dp[blk * 1024 + i] = sp[i];
        } else {
            for (int i = threadIdx.x; i < 1024; i += 256) {
                uint4 v = make_uint4(0u, 0u, 0u, 0u);
                if (blk * 64 + (i & 63) < P) v = sp[i];
                dp[blk * 1024 + i] = v;
            }
        }
    }
}

// what every paged launch needs beyond its contiguous form's checks: a bf16 cache in whole blocks and a row stride that covers n_ctx
bool attp_table_ok(const int* tbl, int tbl_stride, int n_ctx, int kv8) { return tbl && !kv8 && n_ctx > 0 && n_ctx % 64 == 0 && tbl_stride >= n_ctx / 64; }
}  // namespace

int q3_launch_qk_prep_paged(const Q3QkPrep& a, hipStream_t s) {
    if (a.hd != Q3_ATT_HD || !attp_table_ok(a.tbl, a.tbl_stride, a.n_ctx, a.kv8)) return 1;
    hipLaunchKernelGGL(k_qk_prep_paged, dim3(a.rows, a.Hq + a.Hkv), dim3(64), 0, s, a);
    return 0;
}

// The kernel q3_launch_attend_paged takes (q3_attend_pick asks here when a.tbl is set; q3tts_k_attend_pick_paged reports it): the choice
// q3_attend_pick makes for the same launch over a contiguous cache, under the same policies, in its paged form. The Predictor's kernels
// (k_attend_small, k_attend_pair) have none: its per-frame cache is not paged, such a launch is refused.
int q3_attend_pick_paged(const Q3Attend& a) {
    if (!attp_table_ok(a.tbl, a.tbl_stride, a.n_ctx, a.kv8)) return Q3_ATT_REFUSED;
    Q3Attend c = a; c.tbl = nullptr;
    switch (q3_attend_pick(c)) {
        case Q3_ATT_N1: return Q3_ATTP_N1;
        case Q3_ATT_N2: return Q3_ATTP_N2;
        case Q3_ATT_N4: return Q3_ATTP_N4;
        case Q3_ATT_F2: return Q3_ATTP_F2;
        case Q3_ATT_F4: return Q3_ATTP_F4;
        case Q3_ATT_GQA2: return Q3_ATTP_GQA2;
        case Q3_ATT_PREFILL: return Q3_ATTP_PREFILL;
        default: return Q3_ATT_REFUSED;
    }
}

// 0: launched. Nonzero: refused, nothing launched. LDS sizes are the contiguous kernels' (q3_launch_attend).
int q3_launch_attend_paged(const Q3Attend& a, hipStream_t s) {
    const int pick = q3_attend_pick_paged(a);
    if (pick == Q3_ATT_REFUSED) return 1;
    const int R = a.Hq / a.Hkv;
    const dim3 grid(a.Hkv, a.rows);
    if (pick == Q3_ATTP_GQA2) {
        const size_t lds2 = att_lds_gqa2(a.n_ctx).bytes;
        static Q3PerDevice pd2;
        if (lds2 > 65536 && !pd2.ensure(lds2, [&]() { return att_allow_lds((const void*)k_attend_gqa2_paged, lds2); })) return 1;
        hipLaunchKernelGGL(k_attend_gqa2_paged, grid, dim3(256), lds2, s, a);
        return 0;
    }
    if (pick == Q3_ATTP_PREFILL) {
        const int nblk = (a.seg_max_t + 63) / 64;
        const int pw = a.seg_max_t > 128 ? (a.seg_max_t + 63) & ~63 : 128;  // as k_attend_prefill_paged computes it
        const size_t lds3 = (size_t)nblk * 16384 + (size_t)a.seg_max_t * 256 + (size_t)8 * (pw + 128) * sizeof(float);
        static Q3PerDevice pd3;
        if (lds3 > 65536 && !pd3.ensure(lds3, [&]() { return att_allow_lds((const void*)k_attend_prefill_paged, lds3); })) return 1;
        hipLaunchKernelGGL(k_attend_prefill_paged, dim3(a.Hkv, a.n_seg), dim3(512), lds3, s, a);
        return 0;
    }
    const size_t lds = att_lds(R, a.n_ctx).bytes;
    static Q3PerDevice pd;
    if (lds > 65536 && !pd.ensure(lds, [&]() {
            hipError_t e = hipSuccess;
            for (const void* k : {(const void*)k_attend_paged<2, true>, (const void*)k_attend_paged<4, true>, (const void*)k_attend_paged<1, false>,
                                  (const void*)k_attend_paged<2, false>, (const void*)k_attend_paged<4, false>})
                if (e == hipSuccess) e = att_allow_lds(k, lds);
            return e;
        })) return 1;
    if (pick == Q3_ATTP_F2) hipLaunchKernelGGL((k_attend_paged<2, true>), grid, dim3(512), lds, s, a);
    else if (pick == Q3_ATTP_F4) hipLaunchKernelGGL((k_attend_paged<4, true>), grid, dim3(1024), lds, s, a);
    else if (pick == Q3_ATTP_N1) hipLaunchKernelGGL((k_attend_paged<1, false>), grid, dim3(256), lds, s, a);
    else if (pick == Q3_ATTP_N2) hipLaunchKernelGGL((k_attend_paged<2, false>), grid, dim3(512), lds, s, a);
    else hipLaunchKernelGGL((k_attend_paged<4, false>), grid, dim3(1024), lds, s, a);  // Q3_ATTP_N4
    return 0;
}

static bool kvp_paged_ok(const Q3KvPrefix& a) {
    return a.hd == Q3_ATT_HD && a.n <= Q3_KVP_MAX && attp_table_ok(a.tbl, a.tbl_stride, a.n_ctx, a.kv8);
}
int q3_launch_kv_prefix_paged(const Q3KvPrefix& a, hipStream_t s) {
    if (a.n <= 0) return 0;
    if (!kvp_paged_ok(a)) return 1;
    hipLaunchKernelGGL(k_kv_prefix_paged, dim3(a.L * 2 * a.Hkv, a.n), dim3(256), 0, s, a);
    return 0;
}
int q3_launch_kv_prefix_save_paged(const Q3KvPrefix& a, hipStream_t s) {
    if (a.n <= 0) return 0;
    if (!kvp_paged_ok(a)) return 1;
    hipLaunchKernelGGL(k_kv_prefix_save_paged, dim3(a.L * 2 * a.Hkv, a.n), dim3(256), 0, s, a);
    return 0;
}

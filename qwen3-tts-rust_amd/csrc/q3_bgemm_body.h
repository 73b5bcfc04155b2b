// q3_bgemm_body.h — the body of the decoder GEMM (q3_bgemm.hip has the description): one workgroup of k_bgemm, shared by the bf16 / Q8_0
// kernels of q3_bgemm.hip and the K-quant kernels of q3_bgemmk.hip.
#pragma once
#include "q3_kernels.h"
#include <type_traits>

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ float bg_wave_sum(float v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v = v + __shfl_xor(v, m);
    return v;
}

__device__ __forceinline__ size_t bg_yoff(const Q3BGemm& g, int row) {
    return g.seg_rows ? (size_t)(row / g.seg_rows) * g.seg_stride + (size_t)(row % g.seg_rows) * g.ldy : (size_t)row * g.ldy;
}
__device__ __forceinline__ float bg_gelu_erf(float x) { return 0.5f * x * (1.0f + erff(x * 0.70710678118654752f)); }

__device__ __forceinline__ u32x4 bg_ldw(const u32x4* p, bool nt) { return nt ? __builtin_nontemporal_load(p) : *p; }

// 8 int8 quants (lo = elements 0..3, hi = 4..7 of the lane's fragment) as a bf16 MFMA operand: f32(int8) has an exact bf16 in its upper half
__device__ __forceinline__ bf16x8 bg_q8_frag(uint32_t lo, uint32_t hi) {
    union { u32x4 u; bf16x8 v; } r;
#define Q8F(w_, b_) __float_as_uint((float)(int)(signed char)((w_) >> (8 * (b_))))
    r.u.x = (Q8F(lo, 0) >> 16) | (Q8F(lo, 1) & 0xffff0000u); r.u.y = (Q8F(lo, 2) >> 16) | (Q8F(lo, 3) & 0xffff0000u);
    r.u.z = (Q8F(hi, 0) >> 16) | (Q8F(hi, 1) & 0xffff0000u); r.u.w = (Q8F(hi, 2) >> 16) | (Q8F(hi, 3) & 0xffff0000u);
#undef Q8F
    return r.v;
}
__device__ __forceinline__ float bg_f16(uint32_t bits) { return (float)__builtin_bit_cast(_Float16, (unsigned short)bits); }

// Q8: the weights are ggml Q8_0 blocks in the tiled Q8 layout (q3_kernels.h): 1.06 bytes per weight instead of 2 through
// the same ring; every 32-wide K step is one block: P = MFMA from a zero accumulator, acc = fmaf(f32(d), P, acc).
#define BG_PH(RT_, NT_) ((8 * (RT_) * (NT_) > 64 && ((RT_) * (NT_)) % 2 == 0) ? 2 : 1)  // slice-reduction phases (k_bgemm, BgInst::lds)
// EK: the epilogue as a compile-time constant. BG_EK_ANY = everything the struct can ask for, decided at run time (k_bgemm); otherwise
// epilogue | BG_EK_SSP (row scales from ssp) | BG_EK_NW (RESID with nw_next), nothing else set (k_bgemm_epi: bg_ek below names the launches).
// Same loads in the same order, same arithmetic: what a fixed EK removes is the run-time branches around the partials' reduction and the
// epilogue operands — every one of them a join at which the compiler's load counters wait for more than the code behind it needs —
// and the registers of operands the epilogue never reads (0.2 - 0.8 us per launch by the in-kernel stamps).
#define BG_EK_ANY (-1)
#define BG_EK_SSP 8
#define BG_EK_NW 16
// KQ: the weights are ggml K-quant super-blocks in the tiled K layout (q3_kernels.h): the ring holds a pair's nibbles, high
// bits, scale word and d word (5 registers per column tile and 64 k instead of 8), and bg_kq_frag decodes a step's 8 weights to the bf16
// fragment the bf16 path would have loaded — deq_q4_k / deq_q5_k / deq_q6_k of q3_gguf.cpp operation for operation (two roundings for
// Q4_K / Q5_K: d1 = d * sc, m1 = dmin * m once per block, w = d1 * q - m1; Q6_K: ds = d * sc, w = ds * q), then round to nearest even.
// nib: the block's 8 nibbles; hi: its high bits (Q5_K 8 x 1, Q6_K 8 x 2); sc2: its two scale bytes; dw: f16 d | f16 dmin << 16.
__device__ __forceinline__ bf16x8 bg_kq_frag(uint32_t type, uint32_t nib, uint32_t hi, uint32_t sc2, uint32_t dw) {
    bf16x8 v;
    if (type == Q3_KQ_Q6) {
        const float d = bg_f16(dw & 0xffffu);
        const float ds0 = __fmul_rn(d, (float)(int)(signed char)(sc2 & 0xffu)), ds1 = __fmul_rn(d, (float)(int)(signed char)((sc2 >> 8) & 0xffu));
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int q = (int)(((nib >> (4 * e)) & 15u) | (((hi >> (2 * e)) & 3u) << 4)) - 32;
            v[e] = (__bf16)__fmul_rn(e < 4 ? ds0 : ds1, (float)q);
        }
    } else {
        const float d1 = __fmul_rn(bg_f16(dw & 0xffffu), (float)(sc2 & 0xffu)), m1 = __fmul_rn(bg_f16(dw >> 16), (float)((sc2 >> 8) & 0xffu));
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const uint32_t q = ((nib >> (4 * e)) & 15u) + (((hi >> e) & 1u) << 4);
            v[e] = (__bf16)__fsub_rn(__fmul_rn(d1, (float)q), m1);
        }
    }
    return v;
}
// one column tile's row of the K layout as a wave sees it: plane pointers at the lane's own bytes of pair 0
struct BgKqRow {
    uint32_t type; const u32x2* nib; const char* hi; const uint32_t* sc; const char* dd;
    __device__ __forceinline__ void open(const Q3BGemm& g, int tile, int lane) {
        const uint2 te = g.kq[tile];  // (uniform: a scalar load)
        const char* base = (const char*)g.w + (size_t)te.x * 16;
        const size_t P = (size_t)(g.K >> 6);
        type = te.y;
        nib = (const u32x2*)base + lane;
        hi = base + 512 * P + (size_t)lane * q3_kq_hb((int)type);
        sc = (const uint32_t*)(base + (512 + 64 * (size_t)q3_kq_hb((int)type)) * P) + (lane & 15);
        dd = base + (576 + 64 * (size_t)q3_kq_hb((int)type)) * P + (size_t)(lane & 15) * (type == Q3_KQ_Q6 ? 2 : 4);
    }
    // pair p of the tile row -> the ring's registers
    template <bool NTW>
    __device__ __forceinline__ void load(int p, u32x2& n_, uint32_t& h_, uint32_t& s_, uint32_t& d_) const {
        n_ = NTW ? __builtin_nontemporal_load(nib + (size_t)p * 64) : nib[(size_t)p * 64];
        if (type == Q3_KQ_Q6) { h_ = *(const uint32_t*)(hi + (size_t)p * 256); d_ = *(const uint16_t*)(dd + (size_t)(p >> 2) * 32); }
        else {
            h_ = type == Q3_KQ_Q5 ? (uint32_t)*(const uint16_t*)(hi + (size_t)p * 128) : 0u;
            d_ = *(const uint32_t*)(dd + (size_t)(p >> 2) * 64);
        }
        s_ = sc[(size_t)p * 16];
    }
};
// MX: the weights are MX blocks and the K loop runs on the block-scaled MFMA — 1: ggml MXFP4 blocks, BgMx; 2: MXFP8 (E4M3) blocks, BgMx8
// (both in q3_bgemm4.hip, the only file that instantiates MX != 0, which defines them before it does). The struct owns the loop's
// operands; open() issues its first loads, run() is the loop. Every other instantiation holds the empty BgNoMx.
template <int RT, int NT, int D, bool NTW> struct BgMx;
template <int RT, int NT, int D, bool NTW> struct BgMx8;
struct BgNoMx {};
template <int RT, int NT, int D, bool NTW, bool Q8, int EK, bool KQ = false, int MX = 0>
__device__ __forceinline__ void bg_body(const Q3BGemm& g) {
    static_assert(!(Q8 && KQ) && !(MX && (Q8 || KQ)) && MX >= 0 && MX <= 2, "one weight format");
    extern __shared__ float part[];  // [8 waves][RT*NT*4 regs][64 lanes]; MX: then [8 waves][RT][128] x 16 bytes of FP8 exchange
    __shared__ float srow[64];
    Q3_STAMP(g, 0);
    constexpr bool ANY = EK < 0;
    const int epi = ANY ? g.epi : (EK & 7);
    const bool h_ssp = ANY ? g.ssp != nullptr : (EK & BG_EK_SSP) != 0;
    const bool h_nw = ANY ? g.nw_next != nullptr : (EK & BG_EK_NW) != 0;
    const bool h_cs = ANY ? g.col_scale != nullptr : false, h_bias = ANY ? g.bias != nullptr : false, h_seg = ANY ? g.seg_rows != 0 : false;
    const bool h_ybcopy = ANY ? (g.yb && !g.nw_next) : false;  // RESID without nw_next: yb = bf16(y)
#define BG_YOFF(row_) (h_seg ? bg_yoff(g, row_) : (size_t)(row_) * g.ldy)
    constexpr int TR = RT * NT * 4;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, kq = lane >> 4, r = lane & 15;
    // workgroups are dealt round-robin to the 8 XCDs in linear-id order: the row chunks of one column group get ids 8 apart
    // (same XCD, neighbours in time), so the group's weight tiles are fetched into that L2 once
    int cg = blockIdx.x, rc = blockIdx.y;
    if (gridDim.y > 1 && (gridDim.x & 7) == 0) {
        const int id = blockIdx.x + gridDim.x * blockIdx.y, G = gridDim.y;
        rc = (id >> 3) % G; cg = (id & 7) + (id / (8 * G)) * 8;
    }
    const int nb0 = cg * NT, row0 = rc * RT * 16, kblocks = g.K >> 5, per = g.K >> 8, kb0 = wave * per;
    const int B = g.B;
    const u32x4* ap[RT];  // A-tiled rows: one contiguous KiB per (row tile, k block) when the row tile is aligned, 16 B per lane always
#pragma unroll
    for (int i = 0; i < RT; ++i) {
        const int R = g.a_row0 + min(row0 + 16 * i + r, B - 1);
        ap[i] = (const u32x4*)g.a + ((size_t)(R >> 4) * kblocks + kb0) * 64 + kq * 16 + (R & 15);
    }
    const u32x4* wp[NT];
#pragma unroll
    for (int j = 0; j < NT; ++j) wp[j] = (const u32x4*)g.w + ((size_t)(nb0 + j) * kblocks + kb0) * 64 + lane;
    // Load order = the order the results are needed in (vmcnt retires in order): first the norm GEMMs' tile partials (a few hundred
    // bytes per wave from L2), whose reduction to the row scales then runs WHILE the operands are in flight (in-kernel timestamps,
    // tools/chain_stamps.hip: done after the main loop it cost ~1 us of every norm GEMM); then the weights (HBM / Infinity Cache: the
    // long latency) and the rows (L2), D steps of both; last what only the epilogue reads (residual, next norm weight, bias, scale).
    // Every load below is unconditional (out-of-range steps re-read step per - 1): straight-line code, so the counted waits are exact.
    // Measured again with the ring covering the whole K slice (profiles/r07/bgemm_prologue_stamps.txt): the weights in FRONT of the
    // partials shorten the Predictor's launches by 0 - 0.35 us and lengthen the Talker's gate/up and down by 1.1 and 0.35 us (the
    // reduction then waits behind D weight steps from HBM): the order stays. Of the 1.5 - 2.4 us up to "loads issued" 0.1 - 0.4 us were
    // the run-time epilogue branches (gone with a fixed EK), at most 0.6 us the kernel-argument loads and the address arithmetic, the
    // rest the CU's vector-memory path taking in the ring itself (14 - 24 KiB per wave, eight waves): not removable here.
    // norm GEMMs: wave w owns the row scales of rows w, w + 8, ...: lane j adds its tiles j, j + 64, ... in ascending order, then the
    // 64-lane butterfly
    constexpr int NR = 2 * RT;
    float sp0[NR], sp1[NR];
    if (h_ssp) {
#pragma unroll
        for (int i = 0; i < NR; ++i) {
            const float* sp = g.ssp + (size_t)min(row0 + wave + 8 * i, B - 1) * g.ld_ssp;
            sp0[i] = lane < g.ntiles ? sp[lane] : 0.0f;
            sp1[i] = lane + 64 < g.ntiles ? sp[lane + 64] : 0.0f;
        }
    }
    constexpr int DQ = (D + 1) & ~1, DP = DQ / 2;  // Q8: an even number of steps in flight = DP block pairs (one 16-byte weight load covers two steps)
    u32x4 aq[(Q8 || KQ) ? DQ : D][RT], bq[Q8 ? DP : (KQ ? 1 : D)][NT];
    uint32_t sc8[Q8 ? DP : 1][NT];                 // Q8: the two f16 block scales of a pair
    const u32x4* wq[NT]; const uint32_t* sq[NT];
    const int npair = per >> 1;
    BgKqRow kr[KQ ? NT : 1];                        // KQ: DP pairs in flight, as Q8
    u32x2 kn[KQ ? DP : 1][NT]; uint32_t kh[KQ ? DP : 1][NT], ks[KQ ? DP : 1][NT], kd[KQ ? DP : 1][NT];
    const int kp0 = kb0 >> 1;                       // the slice's first pair in the tile row
    std::conditional_t<MX == 2, BgMx8<RT, NT, D, NTW>, std::conditional_t<MX == 1, BgMx<RT, NT, D, NTW>, BgNoMx>> mx;
    if constexpr (MX) {
        mx.open(g, nb0, row0, wave, lane);
    } else if constexpr (KQ) {
#pragma unroll
        for (int j = 0; j < NT; ++j) kr[j].open(g, nb0 + j, lane);
#pragma unroll
        for (int p = 0; p < DP; ++p) {
            const int pc = kp0 + min(p, npair - 1);
#pragma unroll
            for (int j = 0; j < NT; ++j) kr[j].template load<NTW>(pc, kn[p][j], kh[p][j], ks[p][j], kd[p][j]);
        }
#pragma unroll
        for (int s = 0; s < DQ; ++s) {
            const size_t so = (size_t)min(s, per - 1) * 64;
#pragma unroll
            for (int i = 0; i < RT; ++i) aq[s][i] = ap[i][so];
        }
    } else if constexpr (Q8) {
#pragma unroll
        for (int j = 0; j < NT; ++j) {
            wq[j] = (const u32x4*)g.w + ((size_t)(nb0 + j) * (kblocks >> 1) + (kb0 >> 1)) * 64 + lane;
            sq[j] = (const uint32_t*)(g.wscale + (size_t)((nb0 + j) * 16 + r) * kblocks + kb0);
        }
#pragma unroll
        for (int p = 0; p < DP; ++p) {
            const int pc = min(p, npair - 1);
#pragma unroll
            for (int j = 0; j < NT; ++j) { bq[p][j] = bg_ldw(wq[j] + (size_t)pc * 64, NTW); sc8[p][j] = sq[j][pc]; }
        }
#pragma unroll
        for (int s = 0; s < DQ; ++s) {
            const size_t so = (size_t)min(s, per - 1) * 64;
#pragma unroll
            for (int i = 0; i < RT; ++i) aq[s][i] = ap[i][so];
        }
    } else {
#pragma unroll
        for (int s = 0; s < D; ++s) {
            const size_t so = (size_t)min(s, per - 1) * 64;
#pragma unroll
            for (int j = 0; j < NT; ++j) bq[s][j] = bg_ldw(wp[j] + so, NTW);
        }
#pragma unroll
        for (int s = 0; s < D; ++s) {
            const size_t so = (size_t)min(s, per - 1) * 64;
#pragma unroll
            for (int i = 0; i < RT; ++i) aq[s][i] = ap[i][so];
        }
    }
    // epilogue operands, fetched up front instead of at the very end (each was a dependent round trip behind the slice reduction)
    constexpr int NOUT = (TR * 64 + 511) / 512;
    float yres[NOUT], nwv[NOUT], bsv[NOUT], csv[NOUT];
#pragma unroll
    for (int it = 0; it < NOUT; ++it) { yres[it] = 0.0f; nwv[it] = 0.0f; bsv[it] = 0.0f; csv[it] = 1.0f; }
    if (epi == Q3_EPI_RESID) {
#pragma unroll
        for (int it = 0; it < NOUT; ++it) {
            const int o = threadIdx.x + it * 512;
            const int l = o & 63, e = (o >> 6) & 3, t = o >> 8, i = t / NT, j = t - i * NT;
            const int row = row0 + 16 * i + 4 * (l >> 4) + e, col = (nb0 + min(j, NT - 1)) * 16 + (l & 15);
            const bool in = o < TR * 64;
            yres[it] = (in && row < B) ? g.y[BG_YOFF(row) + col] : 0.0f;
            if (h_nw) nwv[it] = in ? g.nw_next[col] : 0.0f;
            if (h_cs) csv[it] = in ? g.col_scale[col] : 1.0f;
        }
    }
    if (h_bias && epi != Q3_EPI_SWIGLU) {
#pragma unroll
        for (int it = 0; it < NOUT; ++it) {
            const int o = threadIdx.x + it * 512;
            const int l = o & 63, t = o >> 8, i = t / NT, j = t - i * NT;
            const int col = (nb0 + min(j, NT - 1)) * 16 + (l & 15);
            bsv[it] = o < TR * 64 ? g.bias[col % g.bias_n] : 0.0f;
        }
    }
    __builtin_amdgcn_sched_barrier(0);
    Q3_STAMP(g, 1);
    if (h_ssp) {  // the NR butterflies are independent chains: interleaved; they wait for the partials only (the first loads issued)
        float av[NR];
#pragma unroll
        for (int i = 0; i < NR; ++i) {
            float a = sp0[i];
            if (lane + 64 < g.ntiles) a = a + sp1[i];
            if (g.ntiles > 128) {
                const float* sp = g.ssp + (size_t)min(row0 + wave + 8 * i, B - 1) * g.ld_ssp;
                for (int t = lane + 128; t < g.ntiles; t += 64) a = a + sp[t];
            }
            av[i] = a;
        }
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1)
#pragma unroll
            for (int i = 0; i < NR; ++i) av[i] = av[i] + __shfl_xor(av[i], m);
        if (lane == 0) {
#pragma unroll
            for (int i = 0; i < NR; ++i) srow[wave + 8 * i] = 1.0f / sqrtf(av[i] / (float)g.d_norm + g.eps);
        }
    }
    __builtin_amdgcn_sched_barrier(0);
    f32x4 acc[RT][NT];
#pragma unroll
    for (int i = 0; i < RT; ++i)
#pragma unroll
        for (int j = 0; j < NT; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
    if constexpr (MX) {
        mx.run(acc, (u32x4*)(part + (size_t)8 * (RT * NT * 4 / BG_PH(RT, NT)) * 64) + (size_t)wave * RT * 128, lane);
    } else if constexpr (KQ) {
        for (int p0 = 0; p0 < npair; p0 += DP) {
#pragma unroll
            for (int dp = 0; dp < DP; ++dp) {
                const int p = p0 + dp;
                if (p < npair) {
#pragma unroll
                    for (int h = 0; h < 2; ++h) {
                        bf16x8 bf[NT];
#pragma unroll
                        for (int j = 0; j < NT; ++j) {  // (the type branch is wave-uniform)
                            const uint32_t hi = kr[j].type == Q3_KQ_Q6 ? (kh[dp][j] >> (16 * h)) & 0xffffu : (kh[dp][j] >> (8 * h)) & 0xffu;
                            bf[j] = bg_kq_frag(kr[j].type, h ? kn[dp][j].y : kn[dp][j].x, hi, (ks[dp][j] >> (16 * h)) & 0xffffu, kd[dp][j]);
                        }
#pragma unroll
                        for (int i = 0; i < RT; ++i) {
                            union { u32x4 u; bf16x8 v; } a; a.u = aq[2 * dp + h][i];
#pragma unroll
                            for (int j = 0; j < NT; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a.v, bf[j], acc[i][j], 0, 0, 0);
                        }
                    }
                    __builtin_amdgcn_sched_barrier(0);
                    if (p + DP < npair) {
#pragma unroll
                        for (int j = 0; j < NT; ++j) kr[j].template load<NTW>(kp0 + p + DP, kn[dp][j], kh[dp][j], ks[dp][j], kd[dp][j]);
#pragma unroll
                        for (int h = 0; h < 2; ++h)
#pragma unroll
                            for (int i = 0; i < RT; ++i) aq[2 * dp + h][i] = ap[i][(size_t)(2 * (p + DP) + h) * 64];
                    }
                    __builtin_amdgcn_sched_barrier(0);
                }
            }
        }
    } else if constexpr (Q8) {
        const f32x4 zero4 = (f32x4){0.f, 0.f, 0.f, 0.f};
        for (int p0 = 0; p0 < npair; p0 += DP) {
#pragma unroll
            for (int dp = 0; dp < DP; ++dp) {
                const int p = p0 + dp;
                if (p < npair) {
#pragma unroll
                    for (int h = 0; h < 2; ++h) {
                        float dsc[NT]; bf16x8 bf[NT];
#pragma unroll
                        for (int j = 0; j < NT; ++j) {
                            dsc[j] = bg_f16(h ? sc8[dp][j] >> 16 : sc8[dp][j] & 0xffffu);
                            bf[j] = h ? bg_q8_frag(bq[dp][j].z, bq[dp][j].w) : bg_q8_frag(bq[dp][j].x, bq[dp][j].y);
                        }
#pragma unroll
                        for (int i = 0; i < RT; ++i) {
                            union { u32x4 u; bf16x8 v; } a; a.u = aq[2 * dp + h][i];
#pragma unroll
                            for (int j = 0; j < NT; ++j) {
                                const f32x4 P = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a.v, bf[j], zero4, 0, 0, 0);
                                acc[i][j][0] = fmaf(dsc[j], P[0], acc[i][j][0]); acc[i][j][1] = fmaf(dsc[j], P[1], acc[i][j][1]);
                                acc[i][j][2] = fmaf(dsc[j], P[2], acc[i][j][2]); acc[i][j][3] = fmaf(dsc[j], P[3], acc[i][j][3]);
                            }
                        }
                    }
                    __builtin_amdgcn_sched_barrier(0);
                    if (p + DP < npair) {
#pragma unroll
                        for (int j = 0; j < NT; ++j) { bq[dp][j] = bg_ldw(wq[j] + (size_t)(p + DP) * 64, NTW); sc8[dp][j] = sq[j][p + DP]; }
#pragma unroll
                        for (int h = 0; h < 2; ++h)
#pragma unroll
                            for (int i = 0; i < RT; ++i) aq[2 * dp + h][i] = ap[i][(size_t)(2 * (p + DP) + h) * 64];
                    }
                    __builtin_amdgcn_sched_barrier(0);
                }
            }
        }
    } else
    for (int s0 = 0; s0 < per; s0 += D) {
#pragma unroll
        for (int d = 0; d < D; ++d) {
            const int s = s0 + d;
            if (s < per) {
#pragma unroll
                for (int i = 0; i < RT; ++i) {
                    union { u32x4 u; bf16x8 v; } a; a.u = aq[d][i];
#pragma unroll
                    for (int j = 0; j < NT; ++j) {
                        union { u32x4 u; bf16x8 v; } b; b.u = bq[d][j];
                        acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a.v, b.v, acc[i][j], 0, 0, 0);
                    }
                }
                __builtin_amdgcn_sched_barrier(0);
#ifdef Q3_STAMPS
                if (s == 0) { asm volatile("" :: "v"(acc[0][0][0])); Q3_STAMP(g, 2); }
#endif
                if (s + D < per) {
#pragma unroll
                    for (int j = 0; j < NT; ++j) bq[d][j] = bg_ldw(wp[j] + (size_t)(s + D) * 64, NTW);
#pragma unroll
                    for (int i = 0; i < RT; ++i) aq[d][i] = ap[i][(size_t)(s + D) * 64];
                }
                __builtin_amdgcn_sched_barrier(0);
            }
        }
    }
#ifdef Q3_STAMPS
    asm volatile("" :: "v"(acc[0][0][0])); Q3_STAMP(g, 3);
#endif
    // The slice buffer holds TRP = TR / PH registers per wave: instances whose 8 x TR x 256 bytes exceed 64 KiB ((4,3): 96) reduce in PH = 2
    // phases of half their tiles, so that no decode workgroup needs more than 64 KiB of LDS — what is left beside one resident vocoder
    // workgroup. Same sums in the same slice order per element; a thread's elements keep their places (o = tid + 512 it).
    constexpr int PH = BG_PH(RT, NT), TP = RT * NT / PH, TRP = TR / PH, NOUTP = NOUT / PH;
    static_assert(PH == 1 || ((RT * NT) % 2 == 0 && (TRP * 64) % 512 == 0), "two phases need an even tile count and whole items per phase");
#pragma unroll
    for (int ph = 0; ph < PH; ++ph) {
        if (ph) __syncthreads();  // every wave is done reading the previous phase's partials
#pragma unroll
        for (int i = 0; i < RT; ++i)
#pragma unroll
            for (int j = 0; j < NT; ++j) {
                if ((i * NT + j) / TP != ph) continue;
#pragma unroll
                for (int e = 0; e < 4; ++e) part[((size_t)wave * TRP + ((i * NT + j) - ph * TP) * 4 + e) * 64 + lane] = acc[i][j][e];
            }
        __syncthreads();
        if (ph == 0) Q3_STAMP(g, 4);
        // slice partials combined in slice order; element (tile t, reg e, lane l) -> row 16 i + 4 (l >> 4) + e, col 16 j + (l & 15)
        if (epi == Q3_EPI_SWIGLU) {
            // one thread per (gate, up) pair: pair p of the 32 in a (tile, register) block of 64 lanes sits in lanes l = 16 (p / 8) + p % 8 (gate,
            // column c = p % 8 < 8 of the tile) and l + 8 (up, the same row 8 columns further); every thread has work (a loop over all
            // TR * 64 elements left the up lanes idle: half of the epilogue's issue slots)
            constexpr int NP = (TRP * 32 + 511) / 512;
#pragma unroll
            for (int it = 0; it < NP; ++it) {
                const int p = threadIdx.x + it * 512;
                if (p >= TRP * 32) break;  // (TRP * 32 is a multiple of 128: whole waves leave together)
                const int q = p & 31, l = ((q >> 3) << 4) + (q & 7), o = ((p >> 5) << 6) + l;
                const int e = (o >> 6) & 3, t = ph * TP + (o >> 8), i = t / NT, j = t - i * NT;
                const int rl = 16 * i + 4 * (l >> 4) + e, row = row0 + rl, c = l & 15;
                const float sc = h_ssp ? srow[rl] : 1.0f;
                float gt = part[o], up = part[o + 8];
#pragma unroll
                for (int wv = 1; wv < 8; ++wv) { gt = gt + part[(size_t)wv * (TRP * 64) + o]; up = up + part[(size_t)wv * (TRP * 64) + o + 8]; }
                if (row < B) g.yb[q3_atile_off(row, (nb0 + j) * 8 + c, g.N >> 6)] = q3_bf16(q3_swiglu(sc * gt, sc * up));
            }
            continue;
        }
#pragma unroll
        for (int itp = 0; itp < NOUTP; ++itp) {
            const int it = ph * NOUTP + itp, o = threadIdx.x + itp * 512;  // o: place in this phase's buffer; tid + 512 it in the whole tile set
            if (o >= TRP * 64) break;  // whole waves leave together (TRP * 64 is a multiple of 256)
            const int l = o & 63, e = (o >> 6) & 3, t = ph * TP + (o >> 8), i = t / NT, j = t - i * NT;
            const int rl = 16 * i + 4 * (l >> 4) + e, row = row0 + rl, c = l & 15;
            const int col = (nb0 + j) * 16 + c;
            const bool live = row < B;
            const float sc = h_ssp ? srow[rl] : 1.0f;
            float v = part[o];
#pragma unroll
            for (int wv = 1; wv < 8; ++wv) v = v + part[(size_t)wv * (TRP * 64) + o];
            if (h_bias) v = v + bsv[it];
            if (epi == Q3_EPI_STORE) {
                if (live) g.y[BG_YOFF(row) + col] = h_ssp ? sc * v : v;
            } else if (epi == Q3_EPI_GELU) {
                if (live) g.yb[q3_atile_off(row, col, g.N >> 5)] = q3_bf16(bg_gelu_erf(v));
            } else if (epi == Q3_EPI_RESID) {
                const float xv = h_cs ? yres[it] + csv[it] * v : yres[it] + v;
                if (live) g.y[BG_YOFF(row) + col] = xv;
                if (h_ybcopy && live) g.yb[q3_atile_off(row, col, g.N >> 5)] = q3_bf16(xv);
                if (h_nw) {  // the consumer's norm inputs: bf16(x * nw) and the tile's sum of squares (16-lane butterfly)
                    if (live) g.yb[q3_atile_off(row, col, g.N >> 5)] = q3_bf16(xv * nwv[it]);
                    float sq = xv * xv;
                    sq = sq + __shfl_xor(sq, 1); sq = sq + __shfl_xor(sq, 2); sq = sq + __shfl_xor(sq, 4); sq = sq + __shfl_xor(sq, 8);
                    if (live && c == 0) g.ssp_out[(size_t)row * g.ld_ssp_out + (nb0 + j)] = sq;
                }
            } else {  // Q3_EPI_ARGMAX: the largest key of the tile's 16 columns goes to keys[row][column tile]; the consumer takes the maximum
                      // over the row's N/16 entries (an atomicMax per (row, tile) on one word per row cost ~8 us of the launch)
                unsigned long long key = q3_argmax_key(h_ssp ? sc * v : v, (uint32_t)col);
#pragma unroll
                for (int m = 1; m <= 8; m <<= 1) { const unsigned long long ok = __shfl_xor(key, m); key = ok > key ? ok : key; }
                if (live && c == 0) g.keys[(size_t)row * g.key_stride + (nb0 + j)] = key;
            }
        }
    }
#ifdef Q3_STAMPS
    Q3_STAMP(g, 5);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    Q3_STAMP(g, 6);
#endif
#undef BG_YOFF
}

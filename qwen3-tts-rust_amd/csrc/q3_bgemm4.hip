// q3_bgemm4.hip — the decoder's GEMM on ggml MXFP4 weights (32 x E2M1 + one E8M0 scale: 4.25 bits per weight) on gfx950's block-scaled
// matrix instruction v_mfma_scale_f32_16x16x128_f8f6f4: the weights enter as FP4 with their file scales, the bf16 row
// operand is turned into MXFP8 (E4M3, one E8M0 scale per 32 k) inside the kernel, and the hardware applies both scales — no per-block
// vector work behind the MFMA (Q8_0, §4.1c) and no decode in front of it (K-quants, §30).
//
// Split of the work: k_bgemm's — a workgroup = 8 waves = 8 K-slices of one (RT*16) x (NT*16) output tile, partials meet in LDS and are
// added in wave order, every epilogue is bg_body's own code. The K loop is bg_body<..., MX = 1> (q3_bgemm_body.h): a wave's slice is
// whole 128-steps, ceil(K / 1024) of them, so the split depends on K alone; per step the wave converts its RT row tiles once (lane = one
// 32-block of one row: amax, scale, 16 packed conversions, all in the lane), passes the bytes through 2 KiB of its own LDS into the
// instruction's operand order, and reuses them for the NT column tiles. Weights stream through a register ring D steps deep (5 registers
// per column tile and 128 k against the bf16 ring's 16), with non-temporal loads when a tile is read by one workgroup.
// Here: the kernels, their launch (the tile instance is q3_bgemm.hip's choice) and the quantising / relayout kernel.
//
// Second half of the file: the same instruction with FP8 on BOTH sides (talker_mxfp8) — the weights are MXFP8 blocks (32 x
// E4M3 + one E8M0 scale: 8.25 bits per weight), made at load from the bf16 weights by the very conversion the rows get (bg_mx_block: one
// copy). k_bgemm_mx8 = bg_body<..., MX = 2>; its K loop is BgMx8, a sibling of BgMx that shares the row side (BgMxRows) and differs in the
// weight ring: two 16-byte loads and a scale byte per column tile and step (9 registers against 5), so the rings are shallower.
#include "q3_bgemm_body.h"

// MX: the weights are ggml MXFP4 blocks in the tiled MX layout (q3_kernels.h) and the K loop runs on the block-scaled
// v_mfma_scale_f32_16x16x128_f8f6f4: one instruction covers 128 k, the rows enter as MXFP8 (E4M3 elements, one E8M0 scale per 32 k), made
// here from the bf16 row operand. A wave owns the 128-steps [wave * per4, (wave + 1) * per4) of K/128, per4 = ceil(K / 1024): a function of K
// alone. bg_mx_rows: lane (b, r) turns 32-block b of the step of row r into FP8 — E = max(exponent field of the block's largest magnitude
// - 8, 0) (OCP MX v1.0: 2^(floor(log2 amax) - 8); 0 for a zero block), magnitudes above 448 * 2^(E - 127) set to it (the hardware conversion
// gives NaN there, it does not saturate: probed), then v_cvt_scalef32_pk_fp8_bf16 (round to nearest even) — and hands the 32 bytes to the two
// lanes whose operand registers hold them (the FP8 operand of lane (g, r) is k = 16 g .. 16 g + 15 and 64 + 16 g .. 64 + 16 g + 15 of the
// step; its scale operand is block g's: the converting lane's own E) through the wave's own 2 KiB of LDS per row tile.
typedef int i32x8 __attribute__((ext_vector_type(8)));
typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));
typedef short s16x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ uint32_t bg_pk_max(uint32_t a, uint32_t b) { return __builtin_bit_cast(uint32_t, __builtin_elementwise_max(__builtin_bit_cast(u16x2, a), __builtin_bit_cast(u16x2, b))); }
__device__ __forceinline__ uint32_t bg_pk_min(uint32_t a, uint32_t b) { return __builtin_bit_cast(uint32_t, __builtin_elementwise_min(__builtin_bit_cast(u16x2, a), __builtin_bit_cast(u16x2, b))); }
// the E8M0 scale of a block from the largest magnitude's bf16 bits
__device__ __forceinline__ uint32_t bg_mx_e(uint32_t amax_bits) { const int ea = (int)(amax_bits >> 7) & 0xff; return (uint32_t)max(ea - 8, 0); }
// four bf16 (two words) -> four E4M3 bytes, scaled by 2^-(E - 127) (sc = E << 23 as a float), magnitudes limited to lim first
__device__ __forceinline__ uint32_t bg_mx_cvt4(uint32_t w0, uint32_t w1, uint32_t lim, float sc) {
    const uint32_t c0 = (w0 & 0x80008000u) | bg_pk_min(w0 & 0x7fff7fffu, lim), c1 = (w1 & 0x80008000u) | bg_pk_min(w1 & 0x7fff7fffu, lim);
    s16x2 lo = {0, 0}, hi = {0, 0};
    lo = __builtin_amdgcn_cvt_scalef32_pk_fp8_bf16(lo, __builtin_bit_cast(bf16x2, c0), sc, false);
    hi = __builtin_amdgcn_cvt_scalef32_pk_fp8_bf16(hi, __builtin_bit_cast(bf16x2, c1), sc, false);
    return ((uint32_t)__builtin_bit_cast(uint32_t, lo) & 0xffffu) | ((uint32_t)__builtin_bit_cast(uint32_t, hi) << 16);
}
// raw: the lane's block as the A-tiled layout holds it (raw[j].x, .y = k 4j .. 4j + 3, .z, .w = k 16 + 4j .. 16 + 4j + 3).
// bg_mx_block: one 32-block of bf16 bits -> its E8M0 scale (returned) and its E4M3 bytes, k 0 .. 15 in lo and 16 .. 31 in hi (the rows of
// both kernels and the MXFP8 weights at load go through this one copy). bg_mx_rows: xw = the wave's exchange area for this row tile,
// 128 x 16 bytes; returns the operand registers and the scale byte of the lane.
__device__ __forceinline__ uint32_t bg_mx_block(const u32x4 (&raw)[4], u32x4& lo, u32x4& hi) {
    uint32_t m = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        m = bg_pk_max(m, raw[j].x & 0x7fff7fffu); m = bg_pk_max(m, raw[j].y & 0x7fff7fffu);
        m = bg_pk_max(m, raw[j].z & 0x7fff7fffu); m = bg_pk_max(m, raw[j].w & 0x7fff7fffu);
    }
    const uint32_t E = bg_mx_e(max(m & 0xffffu, m >> 16)), lim = (((E + 8u) << 7) | 0x60u) * 0x10001u;
    const float sc = __uint_as_float(E << 23);
    lo.x = bg_mx_cvt4(raw[0].x, raw[0].y, lim, sc); lo.y = bg_mx_cvt4(raw[1].x, raw[1].y, lim, sc);
    lo.z = bg_mx_cvt4(raw[2].x, raw[2].y, lim, sc); lo.w = bg_mx_cvt4(raw[3].x, raw[3].y, lim, sc);
    hi.x = bg_mx_cvt4(raw[0].z, raw[0].w, lim, sc); hi.y = bg_mx_cvt4(raw[1].z, raw[1].w, lim, sc);
    hi.z = bg_mx_cvt4(raw[2].z, raw[2].w, lim, sc); hi.w = bg_mx_cvt4(raw[3].z, raw[3].w, lim, sc);
    return E;
}
__device__ __forceinline__ void bg_mx_rows(const u32x4 (&raw)[4], u32x4* xw, int lane, i32x8* a8, uint32_t* e8) {
    u32x4 lo, hi;
    const uint32_t E = bg_mx_block(raw, lo, hi);
    const int b = lane >> 4, r = lane & 15, g0 = 2 * (b & 1), vg = b >> 1;  // block b: lanes (g0, r) and (g0 + 1, r), registers 4 vg .. 4 vg + 3
    // a wave-synchronous exchange: nothing may move across the two barriers (the area is the wave's own; LDS operations of a wave complete in order)
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); __builtin_amdgcn_wave_barrier();  // the last step's loads are behind us
    xw[((g0 * 16 + r) << 1) + vg] = lo;
    xw[(((g0 + 1) * 16 + r) << 1) + vg] = hi;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); __builtin_amdgcn_wave_barrier(); __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    const u32x4 p0 = xw[lane << 1], p1 = xw[(lane << 1) + 1];
    *a8 = (i32x8){(int)p0.x, (int)p0.y, (int)p0.z, (int)p0.w, (int)p1.x, (int)p1.y, (int)p1.z, (int)p1.w};
    *e8 = E;
}
// The row side of both MX K loops (BgMx, BgMx8): one step of bf16 rows in registers, converted per step.
template <int RT>
struct BgMxRows {
    u32x4 mraw[RT][4]; const u32x4* map[RT];
    // lane (kq, r): block kq of the step, row r of the tile: 4 x 16 bytes, 256 apart; s40: the wave's first step; kblocks = K / 32
    __device__ __forceinline__ void rows_open(const Q3BGemm& g, int row0, int s40, int kblocks, int kq, int r) {
#pragma unroll
        for (int i = 0; i < RT; ++i) {
            const int R = g.a_row0 + min(row0 + 16 * i + r, g.B - 1);
            map[i] = (const u32x4*)g.a + ((size_t)(R >> 4) * kblocks + 4 * s40 + kq) * 64 + (R & 15);
        }
    }
    __device__ __forceinline__ void rows_load(int s) {  // step s of the wave's slice
#pragma unroll
        for (int i = 0; i < RT; ++i)
#pragma unroll
            for (int q = 0; q < 4; ++q) mraw[i][q] = map[i][(size_t)s * 256 + q * 16];
    }
    __device__ __forceinline__ void rows_convert(u32x4* xw, int lane, i32x8 (&a8)[RT], uint32_t (&e8)[RT]) {
#pragma unroll
        for (int i = 0; i < RT; ++i) bg_mx_rows(mraw[i], xw + i * 128, lane, &a8[i], &e8[i]);
    }
};
// The MX K loop's operands (bg_body holds one as `mx`): D steps of weights in a register ring (16 bytes of FP4 + a scale byte per column
// tile and step) and, in BgMxRows, one step of bf16 rows.
template <int RT, int NT, int D, bool NTW>
struct BgMx : BgMxRows<RT> {
    u32x4 mw[D][NT]; uint32_t ms[D][NT];
    const u32x4* mwp[NT]; const uint8_t* msp[NT];
    int n4;  // the wave's steps
    __device__ __forceinline__ void open(const Q3BGemm& g, int nb0, int row0, int wave, int lane) {
        const int S4 = g.K >> 7, per4 = (S4 + 7) >> 3, s40 = wave * per4, kblocks = g.K >> 5, kq = lane >> 4, r = lane & 15;
        n4 = max(0, min(per4, S4 - s40));
        const uint8_t* splane = (const uint8_t*)g.w + (size_t)g.N * (g.K >> 1);
#pragma unroll
        for (int j = 0; j < NT; ++j) {
            mwp[j] = (const u32x4*)g.w + ((size_t)(nb0 + j) * S4 + s40) * 64 + lane;
            msp[j] = splane + ((size_t)(nb0 + j) * S4 + s40) * 64 + lane;
        }
        this->rows_open(g, row0, s40, kblocks, kq, r);
        if (n4 > 0) {  // (a K of fewer than 8 steps leaves the last waves without work: they add zeros)
#pragma unroll
            for (int d = 0; d < D; ++d) {
                const size_t so = (size_t)min(d, n4 - 1) * 64;
#pragma unroll
                for (int j = 0; j < NT; ++j) { mw[d][j] = bg_ldw(mwp[j] + so, NTW); ms[d][j] = msp[j][so]; }
            }
            this->rows_load(0);
        }
    }
    // xw: the wave's exchange area, RT x 2 KiB
    __device__ __forceinline__ void run(f32x4 (&acc)[RT][NT], u32x4* xw, int lane) {
        for (int s0 = 0; s0 < n4; s0 += D) {
#pragma unroll
            for (int d = 0; d < D; ++d) {
                const int s = s0 + d;
                if (s < n4) {
                    i32x8 a8[RT]; uint32_t e8[RT];
                    this->rows_convert(xw, lane, a8, e8);
                    __builtin_amdgcn_sched_barrier(0);
                    if (s + 1 < n4) this->rows_load(s + 1);  // the next step's rows travel while this step's MFMAs run
#pragma unroll
                    for (int j = 0; j < NT; ++j) {
                        const i32x8 b4 = (i32x8){(int)mw[d][j].x, (int)mw[d][j].y, (int)mw[d][j].z, (int)mw[d][j].w, 0, 0, 0, 0};
#pragma unroll
                        for (int i = 0; i < RT; ++i)
                            acc[i][j] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(a8[i], b4, acc[i][j], 0, 4, 0, (int)e8[i], 0, (int)ms[d][j]);
                    }
                    __builtin_amdgcn_sched_barrier(0);
                    if (s + D < n4) {
#pragma unroll
                        for (int j = 0; j < NT; ++j) { mw[d][j] = bg_ldw(mwp[j] + (size_t)(s + D) * 64, NTW); ms[d][j] = msp[j][(size_t)(s + D) * 64]; }
                    }
                    __builtin_amdgcn_sched_barrier(0);
                }
            }
        }
    }
};

template <int RT, int NT, int D, bool NTW>
__global__ __launch_bounds__(512) void k_bgemm_mx4(Q3BGemm g) { bg_body<RT, NT, D, NTW, false, BG_EK_ANY, false, true>(g); }

template <int RT, int NT>
struct BgInst4 {
    static constexpr int D = NT == 1 ? 6 : (NT == 2 ? 4 : (RT == 4 ? 2 : 3));  // steps of weights in flight, 5 NT registers each ((4,3) at 3 steps spilled 36 bytes)
    // the slice partials, then the FP8 exchange: 8 waves x RT row tiles x 2 KiB
    static constexpr size_t lds = (size_t)8 * RT * NT * 4 * 64 * 4 / BG_PH(RT, NT) + (size_t)8 * RT * 2048;
    static void prepare() {
        if (lds > 65536) {
            hipFuncSetAttribute((const void*)k_bgemm_mx4<RT, NT, D, false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
            hipFuncSetAttribute((const void*)k_bgemm_mx4<RT, NT, D, true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        }
    }
    static void launch(const Q3BGemm& g, dim3 grid, bool nt, hipStream_t s) {
        if (nt) hipLaunchKernelGGL((k_bgemm_mx4<RT, NT, D, true>), grid, dim3(512), lds, s, g);
        else hipLaunchKernelGGL((k_bgemm_mx4<RT, NT, D, false>), grid, dim3(512), lds, s, g);
    }
};
#define BG4_EACH(X) X(1, 1) X(1, 2) X(1, 3) X(2, 1) X(2, 2) X(2, 3) X(3, 1) X(3, 2) X(3, 3) X(4, 1) X(4, 2) X(4, 3)
void q3_bgemm4_prepare() {
#define P(RT_, NT_) BgInst4<RT_, NT_>::prepare();
    BG4_EACH(P)
#undef P
}
int q3_bgemm4_depth(int rt, int nt) {
#define X(RT_, NT_) if (rt == RT_ && nt == NT_) return BgInst4<RT_, NT_>::D;
    BG4_EACH(X)
#undef X
    return 0;
}
// the (rt, nt) instance on g (checked by q3_launch_bgemm); d / ntw: what ran, as q3_bgemm_pick names it
int q3_bgemm4_launch(const Q3BGemm& g, int rt, int nt, hipStream_t s, int* d, int* ntw) {
    const dim3 grid(g.N / 16 / nt, (g.B + 16 * rt - 1) / (16 * rt));
    const bool once = g.w_once && grid.y == 1;
    *d = q3_bgemm4_depth(rt, nt); *ntw = once ? 1 : 0;
#define L(RT_, NT_) if (rt == RT_ && nt == NT_) { BgInst4<RT_, NT_>::launch(g, grid, once, s); return 0; }
    BG4_EACH(L)
#undef L
    return -1;
}

// ---------------------------------------------------------------------------------------------------------------------
// Quantiser + relayout: one thread per (column tile, step, lane) = one ggml block of one matrix row -> 16 bytes of elements and the scale
// byte. ggml's quantize_row_mxfp4 in f32, operation for operation: amax = max |x|; e = amax > 0 ? floor(log2(amax)) - 2 + 127 : 0, the
// floor taken from the float's exponent field and e held at 0 from below; d = 2^(e - 128) (GGML_E8M0_TO_FP32_HALF: a subnormal for
// e < 2); per element the FIRST index i of kvalues_mxfp4 = {0, 1, 2, 3, 4, 6, 8, 12, 0, -1, ...} with the smallest |kvalues[i] * d - x|
// (strict <: a tie keeps the lower index, so +0 wins over -0 and the smaller magnitude over the larger).
// ---------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t mx4_best(float x, float d) {
    const float kv[16] = {0.f, 1.f, 2.f, 3.f, 4.f, 6.f, 8.f, 12.f, 0.f, -1.f, -2.f, -3.f, -4.f, -6.f, -8.f, -12.f};
    uint32_t best = 0; float be = fabsf(__fsub_rn(__fmul_rn(kv[0], d), x));
#pragma unroll
    for (uint32_t i = 1; i < 16; ++i) {
        const float err = fabsf(__fsub_rn(__fmul_rn(kv[i], d), x));
        if (err < be) { best = i; be = err; }
    }
    return best;
}
// where row c of column tile nb of a fill comes from: the tensor, the row's index in it, and that tensor's sources (Q3FillMx)
__device__ __forceinline__ void mx_fill_src(const Q3FillMx& f, int nb, int c, uint32_t& tid, size_t& lr, const uint16_t*& src, const float*& srcf, const uint8_t*& src4) {
    if (f.mode == 0) { tid = f.tid_a; lr = (size_t)(nb * 16 + c - f.row0); src = f.src_a; srcf = f.srcf_a; src4 = f.src4_a; }
    else if (c < 8) { tid = f.tid_a; lr = (size_t)nb * 8 + c; src = f.src_a; srcf = f.srcf_a; src4 = f.src4_a; }
    else { tid = f.tid_b; lr = (size_t)nb * 8 + c - 8; src = f.src_b; srcf = f.srcf_b; src4 = f.src4_b; }
}
__global__ __launch_bounds__(256) void k_fill_tiled_mx4(Q3FillMx f, int nb0, int nb_count) {
    const size_t gid = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int S = f.K >> 7, kblocks = f.K >> 5;
    if (gid >= (size_t)nb_count * S * 64) return;
    const int lane = (int)(gid & 63), g = lane >> 4, c = lane & 15;
    const int s = (int)((gid >> 6) % S), nb = nb0 + (int)((gid >> 6) / S);
    const int kb = 4 * s + g;
    uint32_t tid; size_t lr; const uint16_t* src; const float* srcf; const uint8_t* src4;
    mx_fill_src(f, nb, c, tid, lr, src, srcf, src4);
    uint32_t q[4] = {0u, 0u, 0u, 0u}, e;
    if (src4) {  // a block_mxfp4 as stored: e, then qs[j] = element j | element j + 16 << 4
        const uint8_t* blk = src4 + (lr * kblocks + kb) * 17;
        e = blk[0];
#pragma unroll
        for (int p = 0; p < 32; ++p) q[p >> 3] |= (uint32_t)((p & 16) ? blk[1 + (p & 15)] >> 4 : blk[1 + p] & 0xF) << (4 * (p & 7));
    } else {
        float x[32], amax = 0.0f;
#pragma unroll
        for (int p = 0; p < 32; ++p) {
            const size_t idx = lr * f.K + (size_t)kb * 32 + p;
            x[p] = srcf ? srcf[idx] : (src ? q3_bf16f(src[idx]) : q3_round_bf16(q3_synth(f.seed, tid, idx, f.scale)));
            amax = fmaxf(amax, fabsf(x[p]));
        }
        const int ef = (int)(q3_f2u(amax) >> 23) & 0xff;  // floor(log2(amax)) + 127 of a normal float (a subnormal amax: 0, e = 0)
        e = amax > 0.0f ? (uint32_t)max(ef - 2, 0) : 0u;
        const float d = q3_u2f(e < 2 ? 0x00200000u << e : (e - 1) << 23);
#pragma unroll
        for (int p = 0; p < 32; ++p) q[p >> 3] |= mx4_best(x[p], d) << (4 * (p & 7));
    }
    ((uint4*)f.dst)[((size_t)nb * S + s) * 64 + lane] = make_uint4(q[0], q[1], q[2], q[3]);
    f.dst[(size_t)f.N * (f.K >> 1) + ((size_t)nb * S + s) * 64 + lane] = (uint8_t)e;
}
void q3_launch_fill_tiled_mx4(const Q3FillMx& f, hipStream_t s) {
    int nb0, nbc;
    if (f.mode == 0) { nb0 = f.row0 / 16; nbc = f.rows / 16; } else { nb0 = 0; nbc = f.N / 16; }
    const size_t total = (size_t)nbc * (f.K >> 7) * 64;
    if (!total) return;
    hipLaunchKernelGGL(k_fill_tiled_mx4, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, f, nb0, nbc);
}

// ---------------------------------------------------------------------------------------------------------------------
// The rows as the GEMM sees them (test hook): bg_mx_rows on every (row tile, step) of an A-tiled operand, written out in natural order —
// q8 [rows16][K] E4M3 bytes, e8 [rows16][K/32] E8M0 bytes. One wave per (row tile, step).
// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void k_mx_rows(const uint16_t* a, int K, uint8_t* q8, uint8_t* e8) {
    __shared__ u32x4 xw[128];
    const int lane = threadIdx.x, g = lane >> 4, r = lane & 15, s = blockIdx.x, rt = blockIdx.y, kblocks = K >> 5;
    const u32x4* ap = (const u32x4*)a + ((size_t)rt * kblocks + 4 * s + g) * 64 + r;
    u32x4 raw[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) raw[q] = ap[q * 16];
    i32x8 a8; uint32_t E;
    bg_mx_rows(raw, xw, lane, &a8, &E);
    uint8_t* row = q8 + (size_t)(rt * 16 + r) * K + 128 * s + 16 * g;
    *(u32x4*)row = (u32x4){(uint32_t)a8[0], (uint32_t)a8[1], (uint32_t)a8[2], (uint32_t)a8[3]};
    *(u32x4*)(row + 64) = (u32x4){(uint32_t)a8[4], (uint32_t)a8[5], (uint32_t)a8[6], (uint32_t)a8[7]};
    e8[(size_t)(rt * 16 + r) * kblocks + 4 * s + g] = (uint8_t)E;
}
void q3_launch_mx_rows(const uint16_t* a, int rows, int K, uint8_t* q8, uint8_t* e8, hipStream_t s) {
    hipLaunchKernelGGL(k_mx_rows, dim3(K >> 7, (rows + 15) / 16), dim3(64), 0, s, a, K, q8, e8);
}

// =====================================================================================================================
// MXFP8 weights: FP8 x FP8 on the same instruction.
// The FP8 operand of lane (g, c) is 32 bytes = two 16-byte halves, half h = k 64 h + 16 g .. + 15 of the step, and the lane's scale byte
// is block g's (k = 32 g .. 32 g + 31): the weight side mirrors the row side with columns for rows (pinned by the exact-grid test). The
// tiled MX8 layout (q3_kernels.h) stores exactly that: per (column tile, step) two wave-loads of one contiguous KiB, then 64 scale bytes.
// BgMx8: the ring holds D steps of 8 + 1 registers per column tile; everything on the row side is BgMxRows, as in BgMx.
// =====================================================================================================================
template <int RT, int NT, int D, bool NTW>
struct BgMx8 : BgMxRows<RT> {
    u32x4 mw[D][NT][2]; uint32_t ms[D][NT];
    const u32x4* mwp[NT]; const uint8_t* msp[NT];
    int n4;  // the wave's steps
    __device__ __forceinline__ void load_w(int d, int s) {  // step s of the slice into ring slot d
#pragma unroll
        for (int j = 0; j < NT; ++j) {
            mw[d][j][0] = bg_ldw(mwp[j] + (size_t)s * 128, NTW); mw[d][j][1] = bg_ldw(mwp[j] + (size_t)s * 128 + 64, NTW);
            ms[d][j] = msp[j][(size_t)s * 64];
        }
    }
    __device__ __forceinline__ void open(const Q3BGemm& g, int nb0, int row0, int wave, int lane) {
        const int S4 = g.K >> 7, per4 = (S4 + 7) >> 3, s40 = wave * per4, kblocks = g.K >> 5, kq = lane >> 4, r = lane & 15;
        n4 = max(0, min(per4, S4 - s40));
        const uint8_t* splane = (const uint8_t*)g.w + (size_t)g.N * g.K;
#pragma unroll
        for (int j = 0; j < NT; ++j) {
            mwp[j] = (const u32x4*)g.w + ((size_t)(nb0 + j) * S4 + s40) * 128 + lane;
            msp[j] = splane + ((size_t)(nb0 + j) * S4 + s40) * 64 + lane;
        }
        this->rows_open(g, row0, s40, kblocks, kq, r);
        if (n4 > 0) {  // (as BgMx: waves past the last step load nothing and add zeros; a short slice re-reads its last step)
#pragma unroll
            for (int d = 0; d < D; ++d) load_w(d, min(d, n4 - 1));
            this->rows_load(0);
        }
    }
    // xw: the wave's exchange area, RT x 2 KiB
    __device__ __forceinline__ void run(f32x4 (&acc)[RT][NT], u32x4* xw, int lane) {
        for (int s0 = 0; s0 < n4; s0 += D) {
#pragma unroll
            for (int d = 0; d < D; ++d) {
                const int s = s0 + d;
                if (s < n4) {
                    i32x8 a8[RT]; uint32_t e8[RT];
                    this->rows_convert(xw, lane, a8, e8);
                    __builtin_amdgcn_sched_barrier(0);
                    if (s + 1 < n4) this->rows_load(s + 1);  // the next step's rows travel while this step's MFMAs run
#pragma unroll
                    for (int j = 0; j < NT; ++j) {
                        const u32x4 w0 = mw[d][j][0], w1 = mw[d][j][1];
                        const i32x8 b8 = (i32x8){(int)w0.x, (int)w0.y, (int)w0.z, (int)w0.w, (int)w1.x, (int)w1.y, (int)w1.z, (int)w1.w};
#pragma unroll
                        for (int i = 0; i < RT; ++i)  // cbsz = blgp = 0: E4M3 on both sides
                            acc[i][j] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(a8[i], b8, acc[i][j], 0, 0, 0, (int)e8[i], 0, (int)ms[d][j]);
                    }
                    __builtin_amdgcn_sched_barrier(0);
                    if (s + D < n4) load_w(d, s + D);
                    __builtin_amdgcn_sched_barrier(0);
                }
            }
        }
    }
};

template <int RT, int NT, int D, bool NTW>
__global__ __launch_bounds__(512) void k_bgemm_mx8(Q3BGemm g) { bg_body<RT, NT, D, NTW, false, BG_EK_ANY, false, 2>(g); }

template <int RT, int NT>
struct BgInstMx8 {
    static constexpr int D = NT == 1 ? 4 : (NT == 2 ? 3 : (RT == 4 ? 1 : 2));  // steps of weights in flight, 9 NT registers each
    static constexpr size_t lds = BgInst4<RT, NT>::lds;  // the slice partials, then the FP8 exchange of the rows
    static void prepare() {
        if (lds > 65536) {
            hipFuncSetAttribute((const void*)k_bgemm_mx8<RT, NT, D, false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
            hipFuncSetAttribute((const void*)k_bgemm_mx8<RT, NT, D, true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        }
    }
    static void launch(const Q3BGemm& g, dim3 grid, bool nt, hipStream_t s) {
        if (nt) hipLaunchKernelGGL((k_bgemm_mx8<RT, NT, D, true>), grid, dim3(512), lds, s, g);
        else hipLaunchKernelGGL((k_bgemm_mx8<RT, NT, D, false>), grid, dim3(512), lds, s, g);
    }
};
void q3_bgemm_mx8_prepare() {
#define P(RT_, NT_) BgInstMx8<RT_, NT_>::prepare();
    BG4_EACH(P)
#undef P
}
int q3_bgemm_mx8_depth(int rt, int nt) {
#define X(RT_, NT_) if (rt == RT_ && nt == NT_) return BgInstMx8<RT_, NT_>::D;
    BG4_EACH(X)
#undef X
    return 0;
}
int q3_bgemm_mx8_launch(const Q3BGemm& g, int rt, int nt, hipStream_t s, int* d, int* ntw) {
    const dim3 grid(g.N / 16 / nt, (g.B + 16 * rt - 1) / (16 * rt));
    const bool once = g.w_once && grid.y == 1;
    *d = q3_bgemm_mx8_depth(rt, nt); *ntw = once ? 1 : 0;
#define L(RT_, NT_) if (rt == RT_ && nt == NT_) { BgInstMx8<RT_, NT_>::launch(g, grid, once, s); return 0; }
    BG4_EACH(L)
#undef L
    return -1;
}

// Quantiser + relayout: one thread per (column tile, step, lane (g, c)) = 32-block 4 s + g of one matrix row -> its 32 E4M3 bytes, which
// go to halves of lanes (2 (g & 1), c) and (2 (g & 1) + 1, c) of half-plane g >> 1, and its scale byte, which stays with lane (g, c).
// The values are the bf16 weights the default loader uploads (f32 sources rounded to nearest even first); the rule is bg_mx_block's.
__global__ __launch_bounds__(256) void k_fill_tiled_mx8(Q3FillMx f, int nb0, int nb_count) {
    const size_t gid = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int S = f.K >> 7;
    if (gid >= (size_t)nb_count * S * 64) return;
    const int lane = (int)(gid & 63), g = lane >> 4, c = lane & 15;
    const int s = (int)((gid >> 6) % S), nb = nb0 + (int)((gid >> 6) / S);
    uint32_t tid; size_t lr; const uint16_t* src; const float* srcf; const uint8_t* src4;
    mx_fill_src(f, nb, c, tid, lr, src, srcf, src4);
    const size_t idx0 = lr * f.K + (size_t)(4 * s + g) * 32;
    auto two = [&](int p) {  // k = p, p + 1 of the block as one word of bf16 bits
        uint32_t b[2];
#pragma unroll
        for (int t = 0; t < 2; ++t) b[t] = srcf ? q3_bf16(srcf[idx0 + p + t]) : (src ? src[idx0 + p + t] : q3_bf16(q3_synth(f.seed, tid, idx0 + p + t, f.scale)));
        return b[0] | (b[1] << 16);
    };
    u32x4 raw[4], lo, hi;
#pragma unroll
    for (int j = 0; j < 4; ++j) raw[j] = (u32x4){two(4 * j), two(4 * j + 2), two(16 + 4 * j), two(18 + 4 * j)};
    const uint32_t E = bg_mx_block(raw, lo, hi);
    u32x4* el = (u32x4*)f.dst + (((size_t)nb * S + s) * 2 + (g >> 1)) * 64 + 2 * (g & 1) * 16 + c;
    el[0] = lo; el[16] = hi;
    f.dst[(size_t)f.N * f.K + ((size_t)nb * S + s) * 64 + lane] = (uint8_t)E;
}
void q3_launch_fill_tiled_mx8(const Q3FillMx& f, hipStream_t s) {
    int nb0, nbc;
    if (f.mode == 0) { nb0 = f.row0 / 16; nbc = f.rows / 16; } else { nb0 = 0; nbc = f.N / 16; }
    const size_t total = (size_t)nbc * (f.K >> 7) * 64;
    if (!total) return;
    hipLaunchKernelGGL(k_fill_tiled_mx8, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, f, nb0, nbc);
}

// q3_bgemmk.hip — the decoder's GEMM on K-quant weights that stay quantised on the device: ggml Q4_K / Q5_K / Q6_K
// super-blocks (the reference's gguf_q5_k_m directory, src/tts/engine.rs:91-95) in the tiled K layout of q3_kernels.h, decoded in registers
// inside k_bgemm's operand ring (bg_body<..., KQ = true>, q3_bgemm_body.h). A decoded weight is the bf16 the host loader (q3_gguf.cpp
// deq_q*_k + round to nearest even) would have uploaded, and it enters the same MFMA chain: RAW and every epilogue keep their bits, so the
// oracle of the bf16 path is the oracle of this one. What changes is the bytes a frame step streams (4.63 / 5.63 / 6.56 bits per weight
// instead of 16) and the load-time work (no host loop over the weights). Here: the kernels and their launch (the tile instance is
// q3_bgemm.hip's choice) and the relayout kernel from the file's super-blocks.
#include "q3_bgemm_body.h"

// the epilogue is decided at run time (BG_EK_ANY), as for Q8_0 weights: one kernel per tile instance and load kind
template <int RT, int NT, int D, bool NTW>
__global__ __launch_bounds__(512) void k_bgemm_kq(Q3BGemm g) { bg_body<RT, NT, D, NTW, false, BG_EK_ANY, true>(g); }

// Pairs in flight per wave: a pair is 8 RT + 5 NT registers (two steps of rows, one pair of quants per column tile) against the bf16
// ring's 8 (RT + NT); the depths below keep every instance under the bf16 instances' register count (decoding needs ~20 temporaries).
template <int RT, int NT>
struct BgInstK {
    static constexpr int S = RT + NT;
    static constexpr int D = S <= 3 ? 8 : (S == 4 ? 6 : (S == 5 ? 4 : 2));  // steps = 2 x pairs
    static constexpr size_t lds = (size_t)8 * RT * NT * 4 * 64 * 4 / BG_PH(RT, NT);
    static void prepare() {
        if (lds > 65536) {
            hipFuncSetAttribute((const void*)k_bgemm_kq<RT, NT, D, false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
            hipFuncSetAttribute((const void*)k_bgemm_kq<RT, NT, D, true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        }
    }
    static void launch(const Q3BGemm& g, dim3 grid, bool nt, hipStream_t s) {
        if (nt) hipLaunchKernelGGL((k_bgemm_kq<RT, NT, D, true>), grid, dim3(512), lds, s, g);
        else hipLaunchKernelGGL((k_bgemm_kq<RT, NT, D, false>), grid, dim3(512), lds, s, g);
    }
};
#define BGK_EACH(X) X(1, 1) X(1, 2) X(1, 3) X(2, 1) X(2, 2) X(2, 3) X(3, 1) X(3, 2) X(3, 3) X(4, 1) X(4, 2) X(4, 3)
void q3_bgemmk_prepare() {
#define P(RT_, NT_) BgInstK<RT_, NT_>::prepare();
    BGK_EACH(P)
#undef P
}
int q3_bgemmk_depth(int rt, int nt) {
#define X(RT_, NT_) if (rt == RT_ && nt == NT_) return BgInstK<RT_, NT_>::D;
    BGK_EACH(X)
#undef X
    return 0;
}
// the (rt, nt) instance on g (checked by q3_launch_bgemm); d / ntw: what ran, as q3_bgemm_pick names it
int q3_bgemmk_launch(const Q3BGemm& g, int rt, int nt, hipStream_t s, int* d, int* ntw) {
    const dim3 grid(g.N / 16 / nt, (g.B + 16 * rt - 1) / (16 * rt));
    const bool once = g.w_once && grid.y == 1;
    *d = q3_bgemmk_depth(rt, nt); *ntw = once ? 1 : 0;
#define L(RT_, NT_) if (rt == RT_ && nt == NT_) { BgInstK<RT_, NT_>::launch(g, grid, once, s); return 0; }
    BGK_EACH(L)
#undef L
    return -1;
}

// ---------------------------------------------------------------------------------------------------------------------
// Relayout: the file's super-blocks (row-major [rows][K/256], as stored) -> tile rows in the tiled K layout. One thread per (tile row,
// pair, lane): its 16 quants (nibbles + high bits); the lanes kq = 0 also write their column's scale word, those of a super-block's
// first pair its d word. Element i of a super-block sits, in ggml's block layouts (dequantize_row_q4_K / q5_K / q6_K):
//   Q4_K { f16 d, dmin; u8 scales[12]; u8 qs[128] }, Q5_K { ..., u8 qh[32], u8 qs[128] }: 32-block b = i / 32: qs[32 (b / 2) + i % 32],
//     low nibble for even b; Q5_K's fifth bit = bit b of qh[i % 32]; (sc, m) of block b = get_scale_min_k4(b)
//   Q6_K { u8 ql[128]; u8 qh[64]; i8 scales[16]; f16 d }: i = 128 h + 32 g + l: ql[64 h + l + 32 (g & 1)], high nibble for g >= 2;
//     bits 2g, 2g + 1 of qh[32 h + l]; scale i / 16
// ---------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void kq_scale_min_k4(int j, const uint8_t* q, uint32_t* sc, uint32_t* m) {
    if (j < 4) { *sc = q[j] & 63u; *m = q[j + 4] & 63u; }
    else { *sc = (q[j + 4] & 0xFu) | ((uint32_t)(q[j - 4] >> 6) << 4); *m = (uint32_t)(q[j + 4] >> 4) | ((uint32_t)(q[j] >> 6) << 4); }
}
__global__ __launch_bounds__(256) void k_fill_tiled_kq(Q3FillKq f) {
    const size_t gid = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int P = f.K >> 6, S = f.K >> 8;
    if (gid >= (size_t)f.ntr * P * 64) return;
    const int lane = (int)(gid & 63), kq = lane >> 4, c = lane & 15;
    const int p = (int)((gid >> 6) % P), t = (int)((gid >> 6) / P);
    const uint8_t* src; size_t row;
    if (f.mode == 0) { src = f.src_a; row = (size_t)t * 16 + c; }
    else if (c < 8) { src = f.src_a; row = (size_t)t * 8 + c; }
    else { src = f.src_b; row = (size_t)t * 8 + c - 8; }
    const int bs = q3_kq_block_bytes(f.type), hb = q3_kq_hb(f.type);
    const uint8_t* blk = src + (row * S + (p >> 2)) * bs;  // the pair's super-block
    uint8_t* base = f.dst + (size_t)t * q3_kq_row_bytes(f.type, f.K);
    uint32_t nib[2] = {0u, 0u}, hi = 0u, scw = 0u;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int b = 2 * (p & 3) + h;  // 32-block of the super-block
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int l = 4 * kq + (e & 3) + 16 * (e >> 2);  // element of the 32-block
            if (f.type == Q3_KQ_Q6) {
                const int hh = b >> 2, g = b & 3;
                const uint8_t ql = blk[64 * hh + l + 32 * (g & 1)], qh = blk[128 + 32 * hh + l];
                nib[h] |= (uint32_t)(g >= 2 ? ql >> 4 : ql & 0xF) << (4 * e);
                hi |= (uint32_t)((qh >> (2 * g)) & 3) << (16 * h + 2 * e);
            } else {
                const uint8_t* qs = blk + (f.type == Q3_KQ_Q5 ? 48 : 16);
                const uint8_t q = qs[32 * (b >> 1) + l];
                nib[h] |= (uint32_t)((b & 1) ? q >> 4 : q & 0xF) << (4 * e);
                if (f.type == Q3_KQ_Q5) hi |= (uint32_t)((blk[16 + l] >> b) & 1) << (8 * h + e);
            }
        }
        if (f.type == Q3_KQ_Q6) scw |= ((uint32_t)blk[192 + 2 * b] | ((uint32_t)blk[192 + 2 * b + 1] << 8)) << (16 * h);
        else { uint32_t sc, m; kq_scale_min_k4(b, blk + 4, &sc, &m); scw |= (sc | (m << 8)) << (16 * h); }
    }
    ((uint2*)base)[(size_t)p * 64 + lane] = make_uint2(nib[0], nib[1]);
    uint8_t* hp = base + (size_t)512 * P;
    if (f.type == Q3_KQ_Q5) ((uint16_t*)hp)[(size_t)p * 64 + lane] = (uint16_t)hi;
    else if (f.type == Q3_KQ_Q6) ((uint32_t*)hp)[(size_t)p * 64 + lane] = hi;
    if (kq == 0) {
        ((uint32_t*)(base + (size_t)(512 + 64 * hb) * P))[(size_t)p * 16 + c] = scw;
        if ((p & 3) == 0) {
            uint8_t* dp = base + (size_t)(576 + 64 * hb) * P;
            if (f.type == Q3_KQ_Q6) ((uint16_t*)dp)[(size_t)(p >> 2) * 16 + c] = (uint16_t)((uint32_t)blk[208] | ((uint32_t)blk[209] << 8));
            else ((uint32_t*)dp)[(size_t)(p >> 2) * 16 + c] = (uint32_t)blk[0] | ((uint32_t)blk[1] << 8) | ((uint32_t)blk[2] << 16) | ((uint32_t)blk[3] << 24);
        }
    }
}
void q3_launch_fill_tiled_kq(const Q3FillKq& f, hipStream_t s) {
    const size_t total = (size_t)f.ntr * (f.K >> 6) * 64;
    if (!total) return;
    hipLaunchKernelGGL(k_fill_tiled_kq, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, f);
}

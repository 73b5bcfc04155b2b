// q3_kernels.h — launchers of the hand-written gfx950 kernels of the codec-token decoder.
#pragma once
#include "q3_common.h"

enum { Q3_EPI_STORE = 0, Q3_EPI_RESID = 1, Q3_EPI_SWIGLU = 2, Q3_EPI_ARGMAX = 3, Q3_EPI_GELU = 4 };

// Experiment builds (-DQ3_STAMPS, tools/chain_stamps.hip): every workgroup's first thread records up to 8 constant-rate (100 MHz)
// timestamps at dbg[(linear workgroup id) * 8 + i]. Compiled out of the product library.
#ifdef Q3_STAMPS
#define Q3_STAMP_FIELD unsigned long long* dbg;
#define Q3_STAMP(p, i) do { if ((p).dbg && threadIdx.x == 0) (p).dbg[((size_t)blockIdx.x + (size_t)gridDim.x * blockIdx.y) * 8 + (i)] = __builtin_amdgcn_s_memrealtime(); } while (0)
#else
#define Q3_STAMP_FIELD
#define Q3_STAMP(p, i) do { } while (0)
#endif

// Kernel attributes (dynamic LDS above 64 KiB) belong to a function ON A DEVICE: a process that drives several GPUs (q3tts_node_*)
// has to set them once per device, not once per process. ensure(want, set_attr) runs set_attr when the current device has not yet been
// given a value >= want. set_attr returns nothing, or a hipError_t: then a failure is not recorded and ensure returns false (the caller
// refuses its launch). One lock per launch site, uncontended.
#include <mutex>
#include <type_traits>
#include <vector>
struct Q3PerDevice {
    std::mutex mu; size_t have[64] = {0};
    template <class F> bool ensure(size_t want, F set_attr) {
        int dev = 0; if (hipGetDevice(&dev) != hipSuccess) dev = 0;
        std::lock_guard<std::mutex> lk(mu);
        if (have[dev & 63] >= want) return true;
        if constexpr (std::is_void_v<decltype(set_attr())>) set_attr();
        else if (set_attr() != hipSuccess) return false;
        have[dev & 63] = want;
        return true;
    }
};

// Exact GEMM y[B][N] = x[B][K] * W[N][K]^T in the canonical order of DESIGN.md §4.1.
// W is bf16 in the tiled HBM layout of DESIGN.md §2.1: tile (nb = n/16, kb = k/32) is 1 KiB,
// lane l = (kq = l>>4, n = l&15) owns the 8 weights W[nb*16+n][kb*32+kq*8 .. +8].
struct Q3Gemm {
    const float* x; int ldx; int B;
    const uint4* w; int K, N;
    const float* norm_w; float eps;   // RMSNorm fused into the prologue when norm_w != nullptr
    const float* bias;                // STORE only
    float* y; int ldy;                // SWIGLU writes [B][N/2]
    unsigned long long* keys; int key_stride;  // ARGMAX: atomicMax(keys[row*key_stride])
    int epi;
#ifdef Q3_STAMPS
    unsigned long long* dbg;          // experiment builds only (tools/exp): s_memtime stamps of workgroup 0 / wave 0
#endif
};
void q3_launch_gemm(const Q3Gemm& g, hipStream_t s);
// The decoder's GEMM (q3_bgemm.hip): bf16 rows x tiled bf16 weights on v_mfma_f32_16x16x32_bf16 in the canonical
// order RAW = (((s_0 + s_1) + ...) + s_7) over 8 K-slices. K % 256 == 0, N % 16 == 0.
//   STORE   y[B][N] f32 = s_r * RAW (s_r from the producer's tile partials ssp; no scale when ssp == nullptr)
//   RESID   y[B][N] f32 += RAW (+= col_scale[column] * RAW when col_scale is given: the vocoder's LayerScale); with nw_next also yb = bf16(y * nw_next) (A-tiled) and ssp_out[B][N/16] (the consumer's norm inputs)
//   SWIGLU  yb = bf16(swiglu(s_r * RAW_gate, s_r * RAW_up)) (A-tiled, N/2 columns); each 16-column weight tile = 8 gate + 8 up columns
//   GELU    yb = bf16(gelu_erf(RAW + bias)) (A-tiled, N columns): the vocoder's ConvNeXt pointwise pair
//   ARGMAX  keys[row * key_stride + column tile] = the largest key(s_r * RAW, column) of that 16-column tile (key_stride >= N/16)
// bf16 activation rows live in the SAME fragment-tiled layout as the weights ("A-tiled"): tile (rt = row/16, kb = k/32) is 1 KiB,
// lane l = (kq = l>>4, r = l&15) owns the 16 bytes holding A[rt*16 + r][kb*32 + {4kq..4kq+3, 16+4kq..16+4kq+3}], so one wave-load of
// an A fragment is one contiguous KiB (a row-major load would touch 16 cache lines for 32 bytes each). Buffers hold
// ceil(rows/16)*16 rows. q3_atile_off(row, k, K/32) = element offset of A[row][k].
Q3_HD size_t q3_atile_off(int row, int k, int kblocks) {
    const int c = k & 31;
    return ((((size_t)(row >> 4) * kblocks + (k >> 5)) * 64 + ((c & 15) >> 2) * 16 + (row & 15)) << 3) + (c & 3) + ((c & 16) >> 2);
}
// Q8_0 ACTIVATIONS (W8A8: q3_bgemm8.hip). The int8 quants of a row operand live in the weights' tiled Q8 form with rows in
// place of columns: tile PAIR (rt = row/16, kp = k/64) is 1 KiB, lane (kq, r) owns 16 bytes — the 8 int8 of k-block 2 kp that its MFMA
// fragment holds (k = 4kq..4kq+3, 16+4kq..16+4kq+3), then the 8 of block 2 kp + 1. q3_q8_off = BYTE offset of element (row, k); kpairs = K/64.
Q3_HD size_t q3_q8_off(int row, int k, int kpairs) {
    const int c = k & 31;
    return ((((size_t)(row >> 4) * kpairs + (k >> 6)) * 64 + ((c & 15) >> 2) * 16 + (row & 15)) << 4) + ((k >> 5) & 1) * 8 + (c & 3) + ((c & 16) >> 2);
}
// ... and their block scales, f32 (q3_q8_sig11 below), as [K/64][row tiles][4 row quads][2 blocks][4 rows]: the 8 scales an MFMA lane needs for
// one (row tile, block pair) — rows 4 kq .. 4 kq + 3 of the tile, both blocks — are 32 consecutive bytes, two 16-byte loads. Index (in f32
// elements) of the scale of (row, k-block kb); rt16 = row tiles of the buffer (rows padded to 16).
Q3_HD size_t q3_q8_scale_idx(int row, int kb, int rt16) {
    return ((((size_t)(kb >> 1) * rt16 + (row >> 4)) * 4 + ((row & 15) >> 2)) << 3) + (kb & 1) * 4 + (row & 3);
}
// The scale of an ACTIVATION block: d = amax / 127 rounded to f16's 11-bit significand, nearest even — bit for bit what the f16 conversion
// gives for a d in f16's normal range — but kept in f32, so it has no f16 exponent limit: the activations are quantised from the
// UN-normalised v = x * nw and carry the magnitude of the residual stream (an f16 scale is subnormal below amax = 127 * 2^-14, zero below
// 127 * 2^-25, infinite above 127 * 65504). Integer code: the carry runs into the exponent; d <= FLT_MAX / 127 cannot overflow. Oracle:
// q3o_round_sig11. Weight scales stay f16 as the file stores them.
Q3_HD float q3_q8_sig11(float d) {
    const uint32_t u = q3_f2u(d);
    return q3_u2f((u + 0xfffu + ((u >> 13) & 1u)) & ~0x1fffu);
}
struct Q3BGemm {
    const uint16_t* a; int a_row0; int B;       // A-tiled bf16 rows [a_row0, a_row0 + B) of a buffer with K columns
    const uint4* w; int K, N;                   // tiled bf16
    int w_once;                                 // 1: the weights are read once per long interval (Talker decode): non-temporal loads when one workgroup owns a tile
    const float* ssp; int ld_ssp; int ntiles; int d_norm; float eps;  // row scale: s_r = 1 / sqrtf(SS(ssp[row][0..ntiles)) / d_norm + eps)
    int epi;
    float* y; int ldy;
    uint16_t* yb;                               // A-tiled bf16 output (RESID: N columns; SWIGLU: N/2 columns), rows as y
    const float* nw_next; float* ssp_out; int ld_ssp_out;
    const float* col_scale;                     // RESID only, optional
    // vocoder extras (all optional, zero = off): a bias added to RAW first (column % bias_n); f32 rows that live in per-slot segments
    // (row m at y + (m / seg_rows) * seg_stride + (m % seg_rows) * ldy); RESID without nw_next but with yb: yb = bf16(y) (A-tiled)
    const float* bias; int bias_n;
    int seg_rows; size_t seg_stride;
    unsigned long long* keys; int key_stride;   // ARGMAX: per-tile maxima, [B][key_stride]
    // Q8_0 weights (the Talker with q3tts_engine_config.talker_q8_0): w then holds ggml block_q8_0 quants in the tiled
    // Q8 layout — tile PAIR (nb = n/16, kp = k/64) is 1 KiB, lane l = (kq, n) owns 16 bytes: the 8 int8 of k-block 2 kp that its bf16
    // fragment would hold (k = 4kq..4kq+3, 16+4kq..16+4kq+3), then the 8 of k-block 2 kp + 1 — and wscale the f16 block scales
    // [N][K/32] (physical column order). RAW = the canonical Q8 order: per block P = MFMA from zero, t = fmaf(f32(d), P, t). K % 512 == 0.
    const uint16_t* wscale;
    // W8A8 (q3_launch_bgemm8; the Talker with talker_q8_0 = 2): `a` then holds the rows' int8 quants (q3_q8_off) and ascale their block scales
    // (q3_q8_scale_idx, a_rt16 row tiles); RESID / SWIGLU write the consumer's operand the same way: yb = int8 quants, yscale / y_rt16.
    const float* ascale; int a_rt16; float* yscale; int y_rt16;
    Q3_STAMP_FIELD
};
int q3_launch_bgemm(const Q3BGemm& g, hipStream_t s);
int q3_launch_bgemm8(const Q3BGemm& g, hipStream_t s);   // the same launch in ggml's Q8_0 x Q8_0 arithmetic (STORE / RESID / SWIGLU / ARGMAX)
void q3_bgemm8_prepare();  // its kernel attributes, once per device; call outside stream capture
void q3_bgemm8_pick(const Q3BGemm& g, int* rt, int* nt);
void q3_bgemm_pick(const Q3BGemm& g, int* rt, int* nt, int* d, int* ntw, int* big);  // the instance q3_launch_bgemm takes for g (no launch)
void q3_bgemm_force(int rt, int nt);  // tuning only: force a tile instance (0, 0: back to the cost model)
void q3_bgemm_prepare();  // kernel attributes + the Q3TTS_BG_BIG policy (read once); call once outside stream capture
void q3_bgemm_big_policy(int policy);  // 1 / -1 / 0: k_bgemm_big always / never / when it fills the chip (tests, A/B runs)
// producer side of the split RMSNorm for plain f32 rows: xb = bf16(x * nw), ssp[row][t] = sum of squares of columns 16t..16t+15
void q3_launch_norm_inputs(const float* x, int ldx, int rows, int d, const float* nw, uint16_t* xb, int xb_row0, float* ssp, int ld_ssp, hipStream_t s);
// the same for a W8A8 consumer: v = x * nw as Q8_0 blocks (int8 quants at xq, f32 block scales at xscale, rt16 row tiles) + ssp
void q3_launch_norm_inputs_q8(const float* x, int ldx, int rows, int d, const float* nw, int8_t* xq, float* xscale, int rt16, float* ssp, int ld_ssp, hipStream_t s);
// H6 (src/assets_manager.rs:383-399) in the reference's own f32 sequence: y[row][o] = bias[o]; for i: y += x[row][i] * w[o][i].
// nw != nullptr: also the norm inputs of y (xb, ssp) for the Predictor's first layer.
struct Q3Project {
    const float* x; int ldx; int rows;
    const float* w; const float* bias; int n_in, n_out;   // w f32 row-major [n_out][n_in]
    float* y; int ldy;
    const float* nw; uint16_t* xb; float* ssp; int ld_ssp;   // xb A-tiled (n_out columns), rows as y
    const float* norm_w; float eps;   // != nullptr: x holds raw rows, the kernel projects rmsnorm(x) * norm_w (normalised while staging)
    float* xscale; int x_rt16;        // W8A8 Predictor (with nw): xb takes y * nw as Q8_0 blocks (int8 quants + these f32 block scales); n_out % 32 == 0
};
int q3_launch_project(const Q3Project& p, hipStream_t s);
// Workgroup barrier that orders LDS traffic only. __syncthreads() also fences global memory, and on gfx9-family parts loads and stores
// share one counter: with global loads (or LDS-DMA) in flight it becomes s_waitcnt vmcnt(0) — the barrier waits for the wave's slowest
// outstanding load and a software pipeline of loads collapses to a depth of one (k_attend_gqa2: first barrier 4.9 us after the start;
// the vocoder's LDS-DMA ring: every K step waited for the stage issued one step earlier). Use it only where nothing read after the barrier
// was written to GLOBAL memory by another wave of the workgroup; data brought by LDS-DMA needs its own s_waitcnt vmcnt(N) before it.
#define Q3_LDS_BARRIER() do { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); __builtin_amdgcn_s_barrier(); asm volatile("" ::: "memory"); } while (0)
#ifdef __HIPCC__
// 64-lane butterflies (xor 32, 16, 8, 4, 2, 1): the canonical order of every wave-wide sum / maximum
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v = v + __shfl_xor(v, m);
    return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v = fmaxf(v, __shfl_xor(v, m));
    return v;
}
__device__ __forceinline__ void q3_row_map(int row, const int* row_pos, const int* row_slot, int slot_mod, int pos_const, int* pos, int* slot) {
    if (slot_mod > 0) { *slot = row % slot_mod; *pos = pos_const + row / slot_mod; }
    else { *pos = row_pos[row]; *slot = *pos < 0 ? 0 : row_slot[row]; }
}
// one element of a norm-input row: 16 consecutive lanes own one tile (all of them must be active); xb_elem = the A-tiled slot
__device__ __forceinline__ void q3_norm_out(float v, float nwv, uint16_t* xb_elem, float* ssp_tile, bool tile_leader) {
    *xb_elem = q3_bf16(v * nwv);
    float sq = v * v;
    sq = sq + __shfl_xor(sq, 1); sq = sq + __shfl_xor(sq, 2); sq = sq + __shfl_xor(sq, 4); sq = sq + __shfl_xor(sq, 8);
    if (tile_leader) *ssp_tile = sq;
}
#endif

#ifdef __HIPCC__
// Q8_0 activation producers (W8A8): ggml's quantiser on a block of 32 consecutive columns of one row, from the f32 values; the block's
// scale is stored as q3_q8_sig11(d) (f32).
// q3_q8_out32: lane <-> column — the 32 lanes of a half wave hold v for columns k .. k + 31 (k % 32 == lane % 32), all active.
__device__ __forceinline__ void q3_q8_out32(float v, int row, int k, int kpairs, int rt16, int8_t* q, float* sc) {
    float amax = fabsf(v);
#pragma unroll
    for (int m = 1; m <= 16; m <<= 1) amax = fmaxf(amax, __shfl_xor(amax, m));
    const float d = amax / 127.0f, id = d != 0.0f ? 1.0f / d : 0.0f;
    q[q3_q8_off(row, k, kpairs)] = (int8_t)(int)roundf(v * id);
    if ((k & 31) == 0) sc[q3_q8_scale_idx(row, k >> 5, rt16)] = q3_q8_sig11(d);
}
// one element of a norm-input row for a W8A8 consumer (q3_norm_out's counterpart): v * nwv into the Q8_0 block of the half wave, the tile's
// sum of squares of v to *ssp_tile
__device__ __forceinline__ void q3_norm_out_q8(float v, float nwv, int row, int k, int kpairs, int rt16, int8_t* q, float* sc, float* ssp_tile, bool tile_leader) {
    q3_q8_out32(v * nwv, row, k, kpairs, rt16, q, sc);
    float sq = v * v;
    sq = sq + __shfl_xor(sq, 1); sq = sq + __shfl_xor(sq, 2); sq = sq + __shfl_xor(sq, 4); sq = sq + __shfl_xor(sq, 8);
    if (tile_leader) *ssp_tile = sq;
}
// q3_q8_out2x16: a lane holds columns k0, k0 + 1 (k0 even), 16 consecutive lanes the block
__device__ __forceinline__ void q3_q8_out2x16(float v0, float v1, int row, int k0, int kpairs, int rt16, int8_t* q, float* sc) {
    float amax = fmaxf(fabsf(v0), fabsf(v1));
#pragma unroll
    for (int m = 1; m <= 8; m <<= 1) amax = fmaxf(amax, __shfl_xor(amax, m));
    const float d = amax / 127.0f, id = d != 0.0f ? 1.0f / d : 0.0f;
    q[q3_q8_off(row, k0, kpairs)] = (int8_t)(int)roundf(v0 * id);
    q[q3_q8_off(row, k0 + 1, kpairs)] = (int8_t)(int)roundf(v1 * id);
    if ((k0 & 31) == 0) sc[q3_q8_scale_idx(row, k0 >> 5, rt16)] = q3_q8_sig11(d);
}
// q3_q8_out8x4: a lane holds 8 consecutive columns k0 .. k0 + 7 (k0 % 8 == 0), four neighbouring lanes (lane ^ 1, lane ^ 2) the block
__device__ __forceinline__ void q3_q8_out8x4(const float* v, int row, int k0, int kpairs, int rt16, int8_t* q, float* sc, bool store) {
    float amax = 0.0f;
#pragma unroll
    for (int i = 0; i < 8; ++i) amax = fmaxf(amax, fabsf(v[i]));
    amax = fmaxf(amax, __shfl_xor(amax, 1)); amax = fmaxf(amax, __shfl_xor(amax, 2));
    const float d = amax / 127.0f, id = d != 0.0f ? 1.0f / d : 0.0f;
    if (store) {
#pragma unroll
        for (int i = 0; i < 8; ++i) q[q3_q8_off(row, k0 + i, kpairs)] = (int8_t)(int)roundf(v[i] * id);
        if ((k0 & 31) == 0) sc[q3_q8_scale_idx(row, k0 >> 5, rt16)] = q3_q8_sig11(d);
    }
}
#endif

// weight tiling: dst tiled [N/16][K/32][64 lanes][8], source either synthetic or a row-major bf16 staging buffer
struct Q3Fill {
    uint4* dst; int N, K;            // physical (fused) matrix
    int mode;                        // 0: rows [row0, row0+rows) come from one logical tensor; 1: gate/up interleave
    int row0, rows;                  // mode 0: physical row range filled by this call
    uint32_t tid_a, tid_b;           // synthetic tensor ids (mode 1: a = gate, b = up)
    const uint16_t* src_a; const uint16_t* src_b;  // row-major [rows][K] bf16 or nullptr -> synthetic
    uint64_t seed; float scale;
    // Q8_0 destination (q3_launch_fill_tiled_q8): dst = the tiled Q8 layout above, dst_scale = f16 [N][K/32]. Sources: raw ggml block_q8_0
    // rows (src8_a / src8_b: [rows][K/32] blocks of 34 bytes, kept as stored), else the bf16 / synthetic sources above, quantised with
    // ggml's reference rule (d = amax / 127, q = roundf(x / d))
    uint16_t* dst_scale; const uint8_t* src8_a; const uint8_t* src8_b;
};
void q3_launch_fill_tiled(const Q3Fill& f, hipStream_t s);
void q3_launch_fill_tiled_q8(const Q3Fill& f, hipStream_t s);
void q3_launch_fill_f32(float* dst, size_t n, uint64_t seed, uint32_t tid, float base, float scale, int round_bf16, hipStream_t s);

// The one head size of the attention kernels (q3_attend.hip). The hd fields of Q3QkPrep / Q3Attend say what the caller has; the launchers
// refuse anything else.
constexpr int Q3_ATT_HD = 128;
// q/k RMSNorm + RoPE (q in place) + bf16 K/V append. One wave per (row, head).
struct Q3QkPrep {
    float* qkv; int ld; int rows;
    int Hq, Hkv, hd;
    const float* qnw; const float* knw; float eps;
    const float* cs; const float* sn;      // [n_ctx][hd/2]
    uint16_t* kc; uint16_t* vc; int n_ctx;  // layer base; per (slot, kv head): n_ctx*hd elements
    const int* row_pos; const int* row_slot;
    int slot_mod, pos_const;  // slot_mod > 0: slot = row % slot_mod, pos = pos_const + row / slot_mod (no loads: the Predictor's per-frame cache is indexed by row)
    // Q8_0 cache (kv8 = 1; q3_attend_kv8.hip): kc / vc then hold the int8 quants (one byte per element, layouts at q3_kv8_k_off)
    // and kd / vd the f16 block scales, per (slot, kv head) n_ctx * hd / 32 of them
    int kv8; uint16_t* kd; uint16_t* vd;
};
int q3_launch_qk_prep(const Q3QkPrep& a, hipStream_t s);  // 0: launched; nonzero: refused (hd != Q3_ATT_HD), nothing launched

// decode / prefill attention over the cache (canonical order DESIGN.md §4.4). One workgroup per (kv head, row).
struct Q3Attend {
    const float* qkv; int ld; int rows;
    float* out; int ldo;
    int out_bf16;     // 1: out is an A-tiled bf16 buffer with Hq*hd columns (the O projection's operand); 0: f32 rows [row][ldo] (test hook)
                      // 2: W8A8 — out holds the rows as Q8_0 blocks (int8 quants, q3_q8_off) and out_scale / out_rt16 their f32 block scales
    float* out_scale; int out_rt16;
    int Hq, Hkv, hd;
    const uint16_t* kc; const uint16_t* vc; int n_ctx;
    const int* row_pos; const int* row_slot;
    int slot_mod, pos_const;  // as in Q3QkPrep
    int kv8; const uint16_t* kd; const uint16_t* vd;  // Q8_0 cache, as in Q3QkPrep: q3_launch_attend then takes the kernels of q3_attend_kv8.hip
    int fused;        // 1: every slot has exactly one row in this launch -> q/k prep + KV append done in-kernel (R >= 2)
                      // 2: rows b (position 0) and slot_mod + b (position 1) of every slot, nothing cached yet (R == 2): k_attend_pair
    Q3QkPrep prep;    // used when fused
    // prefill (fused == 0): the launch's rows as per-slot runs of consecutive positions pos0 .. pos0 + n - 1 — seg[i] = {first row, n, slot,
    // pos0}, device memory; pos0 > 0 when the slot's first pos0 positions hold a voice prefix (q3tts_prefix). seg_max_n = max n,
    // seg_max_t = max (pos0 + n). With it (and two query heads per KV head, every n <= 128, every pos0 + n <= 256) one workgroup
    // serves a whole run from LDS: k_attend_prefill
    const int* seg; int n_seg; int seg_max_n; int seg_max_t;
    Q3_STAMP_FIELD
};
int q3_launch_attend(const Q3Attend& a, hipStream_t s);  // 0: launched; nonzero: refused (see its definition), nothing launched
// k_attend's dynamic LDS (and k_attend_kv8's), offsets in floats: the kernels and their launchers both ask here
struct AttLds { size_t qh, ow, lw, mw, kh, vh, bytes; };
Q3_HD AttLds att_lds(int R, int n_ctx) {
    constexpr int hd = Q3_ATT_HD;
    AttLds L;
    L.qh = (size_t)R * n_ctx;       // [R][n_ctx] scores / probabilities in front of it; qh: [R][hd] the query heads
    L.ow = L.qh + R * hd;           // [R][4][hd] per-wave value sums
    L.lw = L.ow + R * 4 * hd;       // [R][4] per-wave weight sums
    L.mw = L.lw + R * 4;            // [R][4] per-wave score maxima
    L.kh = L.mw + R * 4;            // [hd] newest key (the cache's packed form in front), FUSED only
    L.vh = L.kh + hd;               // [hd] newest value (bf16 cache: bf16-rounded floats; Q8_0 cache: the packed form), FUSED only
    L.bytes = (L.vh + hd) * sizeof(float);
    return L;
}
#ifdef __HIPCC__
// RMSNorm(hd) + RoPE of one head by one wave, the arithmetic in its three steps. Lane (< hd/4) holds its 4 consecutive elements x4, their
// norm weights w4 and RoPE entries c4 / s4; every other lane holds x4 = 0 (+0 to the sum of squares).
__device__ __forceinline__ float prep_rinv(const float4 x4, float eps, int hd) {  // 1 / rms of the head
    float acc = 0.0f;
    acc = fmaf(x4.x, x4.x, acc); acc = fmaf(x4.y, x4.y, acc); acc = fmaf(x4.z, x4.z, acc); acc = fmaf(x4.w, x4.w, acc);
    acc = wave_sum(acc);
    return 1.0f / sqrtf(acc / (float)hd + eps);
}
__device__ __forceinline__ void prep_norm(const float4 x4, float rinv, const float4 w4, float y[4]) {
    y[0] = (x4.x * rinv) * w4.x; y[1] = (x4.y * rinv) * w4.y; y[2] = (x4.z * rinv) * w4.z; y[3] = (x4.w * rinv) * w4.w;
}
// RoPE (NeoX pairing i <-> i + hd/2): lanes [0, hd/8) hold the first halves, partner lane = lane ^ (hd/8)
__device__ __forceinline__ void prep_rope(const float y[4], const float4 c4, const float4 s4, int hl, int lane, float o[4]) {  // hl = hd/8
    const float cc[4] = {c4.x, c4.y, c4.z, c4.w}, ss[4] = {s4.x, s4.y, s4.z, s4.w};
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const float other = __shfl_xor(y[e], hl);
        o[e] = (lane < hl) ? fmaf(-other, ss[e], y[e] * cc[e])     // x_i*c - x_{i+half}*s
                           : fmaf(other, ss[e], y[e] * cc[e]);     // x_{i+half}*c + x_i*s
    }
}
// All three on operands that are already there: kernels that request their operands early (k_attend_gqa2, k_attend_small) call this.
__device__ __forceinline__ void prep_arith(const float4 x4, const float4 w4, const float4 c4, const float4 s4, float eps, int lane, float o[4]) {
    float y[4];
    prep_norm(x4, prep_rinv(x4, eps, Q3_ATT_HD), w4, y);
    prep_rope(y, c4, s4, Q3_ATT_HD >> 3, lane, o);
}
// The same with its loads, each in front of the step that needs it: lanes [0, hd/4) own 4 consecutive elements each; result in o[4]
__device__ __forceinline__ void prep_head(const float* src, const float* nw, float eps, const float* cs, const float* sn, int hd,
                                          int lane, float o[4]) {
    const int nl = hd >> 2, hl = nl >> 1;
    float4 x4 = (float4){0.f, 0.f, 0.f, 0.f}, w4 = x4, c4 = (float4){1.f, 1.f, 1.f, 1.f}, s4 = x4;
    if (lane < nl) x4 = ((const float4*)src)[lane];
    const float rinv = prep_rinv(x4, eps, hd);
    if (lane < nl) w4 = ((const float4*)nw)[lane];
    float y[4];
    prep_norm(x4, rinv, w4, y);
    const int i0 = 4 * (lane & (hl - 1));
    if (lane < nl) { c4 = *(const float4*)(cs + i0); s4 = *(const float4*)(sn + i0); }
    prep_rope(y, c4, s4, hl, lane, o);
}
// The attention output in the form Q3Attend.out_bf16 names, for a lane that holds 1 or 2 consecutive dims of `row` from dim `d` of query
// head `head` on: f32 rows (0), the O projection's A-tiled bf16 operand (1), W8A8 Q8_0 blocks (2: 32 lanes x 1 / 16 lanes x 2, all active).
__device__ __forceinline__ void att_out1(const Q3Attend& a, int row, int head, int d, float v) {
    const int col = head * Q3_ATT_HD + d;
    if (a.out_bf16 == 2) q3_q8_out32(v, row, col, (a.Hq * Q3_ATT_HD) >> 6, a.out_rt16, (int8_t*)a.out, a.out_scale);
    else if (a.out_bf16) ((uint16_t*)a.out)[q3_atile_off(row, col, (a.Hq * Q3_ATT_HD) >> 5)] = q3_bf16(v);
    else a.out[(size_t)row * a.ldo + (size_t)head * Q3_ATT_HD + d] = v;
}
__device__ __forceinline__ void att_out2(const Q3Attend& a, int row, int head, int d, float v0, float v1) {  // d even: one 4-byte store of the bf16 pair
    if (a.out_bf16 == 2) q3_q8_out2x16(v0, v1, row, head * Q3_ATT_HD + d, (a.Hq * Q3_ATT_HD) >> 6, a.out_rt16, (int8_t*)a.out, a.out_scale);
    else if (a.out_bf16) *(uint32_t*)((uint16_t*)a.out + q3_atile_off(row, head * Q3_ATT_HD + d, (a.Hq * Q3_ATT_HD) >> 5)) = (uint32_t)q3_bf16(v0) | ((uint32_t)q3_bf16(v1) << 16);
    else *(float2*)(a.out + (size_t)row * a.ldo + (size_t)head * Q3_ATT_HD + d) = make_float2(v0, v1);
}
#endif
// The Talker's cache as ggml Q8_0 blocks (q3_attend_kv8.hip; q3tts_engine_config.kv_q8_0). A block is 32 consecutive dims of
// one (position, KV head) vector: four per key (after q/k-norm and RoPE), four per value (the raw f32 row). Per (slot, KV head):
//   K quants [64-key block][hd / 16 chunks][64 keys][16] int8 — one key per lane, one 16-byte load per chunk, 1 KiB contiguous per wave-load
//   K scales [64-key block][hd / 32][64 keys] f16;  V quants [t][hd] int8 row-major;  V scales [t][hd / 32] f16
// Byte offset of key element (pos, d) / f16 index of the scale of (pos, block j) inside a head's K cache:
Q3_HD size_t q3_kv8_k_off(int pos, int d) { return ((size_t)((pos >> 6) * (Q3_ATT_HD >> 4) + (d >> 4)) * 64 + (pos & 63)) * 16 + (d & 15); }
Q3_HD size_t q3_kv8_kd_idx(int pos, int j) { return ((size_t)(pos >> 6) * (Q3_ATT_HD >> 5) + j) * 64 + (pos & 63); }
// the launches of q3_attend_kv8.hip: q3_launch_qk_prep / q3_attend_pick / q3_launch_attend / q3_launch_kv_prefix hand over when kv8 is set
int q3_launch_qk_prep_kv8(const Q3QkPrep& a, hipStream_t s);
int q3_attend_pick_kv8(const Q3Attend& a);
int q3_launch_attend_kv8(const Q3Attend& a, hipStream_t s);
// The gathering form of k_attend_small (block 0 of passes q >= 1 of the greedy bf16 Predictor): the row's q / k / v are not
// read from a.qkv but from a table of every possible input row's layer-0 QKV, tab[code], where code is the argmax k_pred_next<false>(q)
// takes from the same per-tile keys (largest key of the row, q3_argmax_idx); a code outside [0, tab_rows) reads the fallback row tab_rows.
// One more workgroup column (blockIdx.x == Hkv) does what k_pred_next(q) did besides the row's norm inputs, for rows whose slot is active:
// codes[slot][n_frames][q] = code, fb[row] += codec_q[code] (+ 0 out of range), px[row] = pproj_q[code] (proj_b out of range).
struct Q3AttGather {
    const float* tab; int tab_rows;                    // [tab_rows + 1][a.ld] f32
    const unsigned long long* keys; int n_key_parts;   // keys[row][n_key_parts]: the head GEMM's per-tile maxima of pass q - 1
    int q, ncb;
    const float* codec_q; int d;                       // [tab_rows][d]; d % 4 == 0
    const Q3Slot* slots; const int* row_slot;          // the slot RECORD of a row (the cache stays indexed as a says)
    int* codes; int max_steps_cap;
    float* fb;
    const float* pproj_q; const float* proj_b; int dp; float* px;  // [tab_rows][dp], [dp]; dp % 4 == 0
};
// 0: launched; nonzero: refused, nothing launched — a launch q3_attend_pick does not give to k_attend_small<2>, or a missing table / pointer
int q3_launch_attend_gather(const Q3Attend& a, const Q3AttGather& t, hipStream_t s);
// the nine attention kernels of q3_attend.hip as q3_attend_pick names them (q3tts_k_attend_pick reports these numbers)
enum { Q3_ATT_REFUSED = -1, Q3_ATT_N1 = 0, Q3_ATT_N2 = 1, Q3_ATT_N4 = 2,   // k_attend<1 / 2 / 4, false>
       Q3_ATT_F2 = 3, Q3_ATT_F4 = 4,                                       // k_attend<2 / 4, true>
       Q3_ATT_GQA2 = 5, Q3_ATT_SMALL2 = 6, Q3_ATT_PAIR = 7, Q3_ATT_PREFILL = 8,
       // the six of q3_attend_kv8.hip (Q3Attend.kv8; q3tts_k_attend_pick_kv8): k_attend_kv8<1 / 2 / 4, false>, k_attend_kv8<2 / 4, true>, k_attend_gqa2_kv8
       Q3_ATT8_N1 = 9, Q3_ATT8_N2 = 10, Q3_ATT8_N4 = 11, Q3_ATT8_F2 = 12, Q3_ATT8_F4 = 13, Q3_ATT8_GQA2 = 14 };
int q3_attend_pick(const Q3Attend& a);  // the kernel q3_launch_attend takes for a under the current policies (no launch); reads hd, Hq, Hkv,
                                        // fused, n_ctx and the seg fields only
// Voice prefixes (q3tts_prefix): copy a prefix store into slots before their prefill. A store is laid out as one slot's cache of
// np = ceil(P / 64) * 64 positions: k / v [L][Hkv][np * hd] bf16 (keys in 64-position blocks, values row-major). Entry j copies every
// layer's whole key blocks and the values of positions < P[j] into slot[j]; keys at positions P .. np - 1 of the slot are overwritten.
#define Q3_KVP_MAX 64
struct Q3KvPrefix {
    uint16_t* kc; uint16_t* vc; size_t layer_stride; int n_ctx;  // the Talker's cache: [L][slots][Hkv][n_ctx * hd]
    int L, Hkv, hd, n;
    const uint16_t* pk[Q3_KVP_MAX]; const uint16_t* pv[Q3_KVP_MAX]; int P[Q3_KVP_MAX]; int slot[Q3_KVP_MAX];
    // Q8_0 cache (kv8 = 1): kc / vc hold int8 quants (layer_stride in bytes), kd / vd the cache's f16 scales (layer_stride / 32 per layer). A
    // store then is k / v [L][Hkv][np * hd] int8 followed by its scales [L][Hkv][np * hd / 32] f16 in the same allocation: pk / pv name the
    // quants. Whole key blocks (quants and scales) are copied for K, positions < P for V.
    int kv8; uint16_t* kd; uint16_t* vd;
};
void q3_launch_kv_prefix(const Q3KvPrefix& a, hipStream_t s);
void q3_launch_kv_prefix_kv8(const Q3KvPrefix& a, hipStream_t s);  // (q3_attend_kv8.hip; q3_launch_kv_prefix hands over when kv8 is set)
// The other direction (k_kv_prefix_save / k_kv_prefix_save_kv8): positions < P[j] of slot[j] into the store pk[j] / pv[j] (written, though
// the struct names them const), which must come zero-filled: the result is byte for byte the store q3tts_prefix_create makes of the same
// rows — the keys P[j] .. np - 1 of the last block are written as zeros, values and (Q8_0) scales likewise stop at P[j].
// 0: launched (or n == 0); nonzero: refused, nothing launched (hd != Q3_ATT_HD, more than Q3_KVP_MAX entries, a Q8_0 cache without scales)
int q3_launch_kv_prefix_save(const Q3KvPrefix& a, hipStream_t s);
int q3_launch_kv_prefix_save_kv8(const Q3KvPrefix& a, hipStream_t s);
void q3_attend_policy(int decode, int prefill);  // test hook (q3tts_k_attend_policy): which kernel variant serves decode / prefill attention (same bits)
void q3_attend_policy_get(int* decode, int* prefill);

// Talker sampler + frame bookkeeping (H4/H5). One workgroup per slot.
struct Q3Sample {
    float* logits; int ld; int limit; int eos;
    Q3Slot* slots; int B;             // slots: ALL slots of the engine; row b works for slot row_slot[b]
    const int* row_slot;
    const float* rng;                 // per-slot draws: rng[slot.rng_base + step]
    int* codes; int max_steps_cap; int ncb;
    // repetition penalty (Q3Slot.rep_penalty != 1): seen[slot][seen_words] holds one bit per code 0 generated so far in the utterance
    // (cleared at admission); a seen logit v becomes v > 0 ? v / p : v * p before the sample, the chosen code's bit is set after it
    uint32_t* seen; int seen_words;
};
void q3_launch_sample(const Q3Sample& a, hipStream_t s);
// stand-alone sampler for the test hook: n rows, explicit draws
void q3_launch_sample_rows(const float* logits, int n, int ld, int limit, float temperature, int top_k, float top_p,
                           const float* r, int* out, hipStream_t s);

// predictor input of pass A (rows [0, B): the projected hidden rows, rows [B, 2B): the code rows):
// X[b] = rmsnorm(xT[b]) (X == nullptr: left to the projection tile, Q3Project.norm_w); px[B + b] = proj(codec0[code0]) taken
// from the pre-projected table (row-independent exact GEMM: the table row IS what projecting on the fly gives);
// fb[b] = 0 + codec0[code0]
struct Q3PredInput {
    const float* xT; const float* out_norm; float eps; int d;
    const float* codec0; int codec0_rows;
    const float* pproj0; const float* proj_b; int dp;  // proj(codec0) table [codec0_rows][dp]; bias = proj(0)
    const Q3Slot* slots; const int* row_slot; float* X; float* px; float* fb; int B;
    const float* nw; uint16_t* xb; float* ssp;         // norm inputs of px row B + b (the code row; A-tiled xb, ssp ld dp/16)
    float* xscale; int x_rt16;                         // W8A8 Predictor: xb takes the row as Q8_0 blocks (int8 quants + these f32 block scales)
};
void q3_launch_pred_input(const Q3PredInput& a, hipStream_t s);
// the frame's first kernel: sampler + code rows (B workgroups) and the H6 tiles of the hidden rows (pj, with norm_w) side by side in one launch
int q3_launch_sample_input(const Q3Sample& a, const Q3PredInput& p, const Q3Project& pj, hipStream_t s);

// after pass q-1: code_q from the argmax key, record it, fb += codec_q[code_q]; q<ncb-1: px[b] = projected emb;
// last: fb += tts_pad -> xT[b], row_pos_t[b] = cur_pos++, n_frames++
// sample = true (q3_launch_pred_next): code_q is drawn from the head's stored logits instead — plogits[b][cbs] (the head GEMM ran Q3_EPI_STORE),
// the slot's Predictor sampler (Q3Slot.p_*), draw prng[slot * prng_stride + frame * (ncb - 1) + (q - 1)]; keys is not read
struct Q3PredNext {
    const unsigned long long* keys; int n_key_parts; int q; int ncb;  // keys[b][n_key_parts]: the head GEMM's per-tile maxima of pass q - 1
    const float* codec_q; int rows_q; int d;
    Q3Slot* slots; const int* row_slot; int B;
    int* codes; int max_steps_cap;
    float* fb; const float* tts_pad; float* xT; int* row_pos_t;
    const float* pproj_q; const float* proj_b; int dp; float* px;  // q < ncb-1: px[b] = proj(codec_q[code]) from the table
    const float* nw; uint16_t* xb; float* ssp;  // norm inputs of the row just written: px[b] (Predictor layer 0) or, last, xT[b] (Talker layer 0)
    float* xscale; int x_rt16;                  // the row's consumer is W8A8 (the Predictor for q < ncb - 1, the Talker for the last pass): xb then takes the row as Q8_0 blocks (int8 quants + these f32 block scales)
    const float* plogits; int cbs; const float* prng; int prng_stride;   // the sampling variant only
    Q3_STAMP_FIELD
};
int q3_launch_pred_next(const Q3PredNext& a, hipStream_t s, bool sample = false);  // -1: the sampling variant refuses cbs > Q3_SAMP_MAX
// The norm inputs for nw (A-tiled xb with dp columns, ssp [rows + 1][dp / 16]) of the rows k_pred_next<false> can write into px from one
// pre-projected table: row c < rows = tab[c], row `rows` = bias (a code out of range). q3_norm_out on every element, as k_pred_next applies it.
void q3_launch_pred_table_rows(const float* tab, int rows, const float* bias, int dp, const float* nw, uint16_t* xb, float* ssp, hipStream_t s);
int q3_pred_next_prepare();  // the sampling variant's kernel attributes, once per device; call outside stream capture. -1: the device refused them
// Streamed text (include/q3tts.h, "streaming text input"): the last pass's addend row is text[id] (the prompt builder's out-of-range rule)
// instead of tts_pad, per slot and frame. ids[slot][cap]: the slot's trailing ids T; cnt[slot] <= cap: how many are valid; cur[slot]: the
// row of the slot's NEXT frame, {1, T[n_frames]} or {0, 0} = tts_pad — kept beside the slot record so that the kernel loads it with the
// record (the row load is the one added dependent round trip) and advanced by the kernel: after frame f it becomes T[f + 1] or tts_pad.
// The host rewrites cur whenever it changes cnt (between frame steps only). A slot with cnt = 0 gets tts_pad: q3_launch_pred_next's bits.
struct Q3TextRows {
    const float* text; int text_vocab;
    const int* ids; const int* cnt; int2* cur; int cap;
};
// the last pass (a.q == a.ncb - 1) of q3_launch_pred_next with the addend row from t; -1: refused (not the last pass / the sampling variant's checks)
int q3_launch_pred_last_text(const Q3PredNext& a, const Q3TextRows& t, hipStream_t s, bool sample);

// prompt builder (H1): out[row] = tabA[idA] (+ tabB[idB]) with the reference's OOB rules
struct Q3PromptRow { int32_t kindA, idA, kindB, idB; };  // kind: 0 none, 1 text, 2.. codec table (kind-2), -1 spk_emb, -2 zero
void q3_launch_prompt_rows(const Q3PromptRow* rows, int n, const float* text, int text_vocab, const float* const* codec,
                           int codec0_rows, int codecq_rows, int ncb, const float* spk, int d, float* out, hipStream_t s);
// clone prompt frame rows: out[row] = marker + sum_q codec_q[codes[row*16+q]] (src/tts/prompt.rs:79-96)
void q3_launch_prompt_ref_frames(const int* codes, int n_frames, const float* marker, const float* const* codec,
                                 int codec0_rows, int codecq_rows, int ncb, int d, float* out, hipStream_t s);

void q3_launch_copy_rows(float* dst, int ldd, const float* src, int lds, int rows, int cols, hipStream_t s);

// Split residual VQ of the clone audio encoder (q3_clone.hip: k_rvq): frame t takes codebook 0 on ps[t], codebooks 1.. on the
// residual of pa[t] (pa may be NULL when ncb == 1); nearest codeword in squared Euclidean distance, ties to the smaller index; codes [T][ncb].
// cbT: device table of the ncb codebooks in k_cb_transpose's layout [D/4][CS][4]. books (optional): row-major [ncb][CS][D], transposed into
// booksT ([ncb] x that layout, the memory cbT's entries point into) before the quantiser runs.
struct Q3Rvq {
    const float* ps; const float* pa; int T, D;
    const float* const* cbT; int ncb, CS;
    long long* codes;
    const float* books; float* booksT;
};
int q3_launch_rvq(const Q3Rvq& a, hipStream_t s);  // 0: launched; -1: refused (see its definition), nothing launched

// canonical RMSNorm of rows (test hook / hidden read-back)
void q3_launch_gather_rows(float* dst, const float* src, const int* perm, int rows, int cols, hipStream_t s);
void q3_launch_rmsnorm_rows(const float* x, int ldx, const float* w, float eps, int d, int rows, float* out, int ldo, hipStream_t s);

// PCM gather: windows of f32 sample rows -> one contiguous f32 or i16 buffer. Entry j copies src[row][first, first + count) to
// dst[dst_off, dst_off + count); i16 follows the reference's WAV rule (src/utils/audio.rs:35-37): (x * 32767).clamp(-32768, 32767) as i16,
// truncation toward zero. Up to Q3_PCM_MAX_ENT entries per launch (passed by value); the caller guarantees the windows lie inside
// src and dst. i16 = 0: f32 out, 1: i16 out.
#define Q3_PCM_MAX_ENT 64
struct Q3PcmEnt { int32_t row, first, count, pad; long long dst_off; };
struct Q3PcmPack { Q3PcmEnt e[Q3_PCM_MAX_ENT]; };
void q3_launch_pcm_pack(const float* src, size_t stride, const Q3PcmPack& ents, int n_ent, int max_count, int i16, void* dst, hipStream_t s);
// the i16 rule above (and the f32 store) as the two PCM kernels apply it to one sample
__device__ __forceinline__ void q3_pcm_put(float* d, float v) { *d = v; }
__device__ __forceinline__ void q3_pcm_put(int16_t* d, float v) {
    v = v * 32767.0f;
    v = fminf(fmaxf(v, -32768.0f), 32767.0f);
    *d = (int16_t)(int)truncf(v);
}

// PCM resampler (q3_resample.hip): k_pcm_pack's sibling. Entry j writes outputs [first, first + count) of src[row] AT THE
// OUTPUT RATE to dst[dst_off, ...); Q3PcmSrc adds what the filter needs to know about the entry's row: len[j] valid samples (nothing past
// them is loaded; they count as zeros) and whether the row is finished (bit j of final_mask). A finished row of n samples has
// N(n) = ceil(n L / M) outputs; an unfinished one can deliver the D(n) = ceil((n - H) L / M) whose windows end inside the data.
#define Q3_RESAMPLE_MAX_COEF 32768     // L x T coefficients at the most (128 KiB)
#define Q3_RESAMPLE_LDS_BYTES 65536    // a workgroup's LDS: one tile's input span and, when it fits beside it, the table
struct Q3Resamp { int32_t rate_in, rate_out, L, M, H, T; const float* tab; };  // tab (device): [T][L], tab[k * L + (m mod L)] = tap k of output m
struct Q3PcmSrc { int32_t len[Q3_PCM_MAX_ENT]; unsigned long long final_mask; };
// the plan of a rate pair; Q3TTS_ERR_INVALID outside 4000..96000 Hz (or equal rates), Q3TTS_ERR_UNSUPPORTED past Q3_RESAMPLE_MAX_COEF
int q3_resample_plan(int rate_in, int rate_out, int* L, int* M, int* H, int* T);
// the table as DESIGN.md §19 states it, tab[p][k] (host, double, rounded once), and the same values in the kernel's layout
int q3_resample_table(int rate_in, int rate_out, int* L, int* M, int* H, std::vector<float>& tab);
std::vector<float> q3_resample_device_layout(const std::vector<float>& tab, int L, int M, int T);
long long q3_resample_N(long long n, int L, int M);
long long q3_resample_D(long long n, int L, int M, int H);
// i16 as q3_launch_pcm_pack; -1 (nothing launched): one tile's input span does not fit the LDS
int q3_launch_pcm_resample(const float* src, size_t stride, const Q3PcmPack& ents, const Q3PcmSrc& rows, int n_ent, int max_count, const Q3Resamp& rs,
                           int i16, void* dst, hipStream_t s);

// PCM time-stretch (q3_tempo.hip): WSOLA at the vocoder's rate, pitch kept. Frame k of a row is Q3_TEMPO_HS outputs, read
// from p_k = a_k + delta_k with a_k = (k Hs s) div 1000 (s: the speed in per mille) and delta_k the first maximum of the 256 correlations
// with the previous frame's continuation. The constants are quality parameters nobody has listened to yet; they live here and nowhere else.
#define Q3_TEMPO_HS 256                                           // synthesis hop = outputs per frame
#define Q3_TEMPO_WN (2 * Q3_TEMPO_HS)                             // window, template and chain length
#define Q3_TEMPO_DMIN (-128)                                      // candidates delta in [DMIN, DMIN + ND)
#define Q3_TEMPO_ND 256                                           // = threads per workgroup: one chain per thread
#define Q3_TEMPO_HOLD (Q3_TEMPO_DMIN + Q3_TEMPO_ND - 1 + Q3_TEMPO_WN + 1)  // 640: input samples behind need_k a frame waits for
#define Q3_TEMPO_MIN 500
#define Q3_TEMPO_MAX 2000
// Entry j: frames [k_from, k_to) of src[row] (n valid samples: nothing at or past n is loaded, it counts as zeros) into dst[row]; outputs
// m >= n_out are not written. p_last[row] holds p of frame k_from - 1 (read when k_from >= 2) and receives p of frame k_to - 1.
struct Q3TempoEnt { int32_t row, n, k_from, k_to, n_out, pad; };
struct Q3TempoPack { Q3TempoEnt e[Q3_PCM_MAX_ENT]; };
long long q3_tempo_N(long long n, int permille);        // outputs of a finished row of n samples: ceil(n 1000 / s)
long long q3_tempo_frames(long long n, int permille, bool done);  // frames decided: all ceil(N / Hs) of a finished row, else the leading decidable ones
inline long long q3_tempo_valid(long long n, int permille, bool done) { return done ? q3_tempo_N(n, permille) : Q3_TEMPO_HS * q3_tempo_frames(n, permille, false); }
void q3_tempo_window(std::vector<float>& w);            // the periodic Hann of Q3_TEMPO_WN points, double rounded once
// win: the window on the device. delta != null: delta[row * delta_stride + k] = delta_k of every frame the launch decides (k < delta_stride)
void q3_launch_pcm_tempo(const float* src, size_t stride, float* dst, size_t dst_stride, long long* p_last, const float* win, int permille,
                         const Q3TempoPack& ents, int n_ent, int32_t* delta, size_t delta_stride, hipStream_t s);

// Long documents (q3_long.hip): the two kernels that turn the segments' PCM rows into one document row.
// k_pcm_edges: edges[2 r] / edges[2 r + 1] = the first / last block of Q3_JOIN_W samples of row r (lens[r] valid samples: nothing at or
// past them is loaded) that holds a sample with fabsf(x) > threshold, by integer min / max; the caller fills edges with {INT32_MAX, -1}.
// k_pcm_join: piece r is dst[off, off + L) = src[r][lo, lo + L) with fades of F samples at both ends, then `gap` samples of +0.0f.
// The block length is a quality parameter nobody has listened to yet; it lives here and nowhere else.
#define Q3_JOIN_W 240
#define Q3_JOIN_MAX_SEG 1024
struct Q3JoinSeg { long long lo, L, off, gap; int32_t F, pad; };
void q3_launch_pcm_edges(const float* src, size_t stride, const int32_t* lens, int rows, long long max_len, float threshold, int32_t* edges, hipStream_t s);
void q3_launch_pcm_join(const float* src, size_t stride, const Q3JoinSeg* segs, int rows, long long max_span, float* dst, hipStream_t s);

// Documents in a session (q3_doc.hip): the streaming form of the two kernels above, entries by value as Q3PcmPack.
// k_doc_scan: entry j is a running segment whose valid length grew from n_prev to n_now: dst[n_prev, n_now) = src[n_prev, n_now) (nothing at
// or past n_now is loaded, nothing else is written), and edges[0] / edges[1] (the caller's {INT32_MAX, -1} at the segment's start; NULL:
// not kept) take every block of Q3_JOIN_W samples that intersects the range, by k_pcm_edges' rules against thr.
// k_doc_emit: piece j is dst[dst, dst + count) = samples [j0, j0 + count) of a piece of final length L (LLONG_MAX: not known yet, and no
// sample of the fade-out among them) with fades of F samples, read from src[0, count) (NULL: +0.0f, a pause); i16 as q3_launch_pcm_pack.
// F < 0: the entry is a table, `count` 32-bit words copied bit for bit from src to the BYTE offset dst (a multiple of 4) of the buffer:
// a document's edges ride the boundary's copy to the host this way.
#define Q3_DOC_MAX_ENT 64
struct Q3DocScan { const float* src; float* dst; int32_t* edges; int32_t n_prev, n_now; float thr; int32_t pad; };
struct Q3DocScanPack { Q3DocScan e[Q3_DOC_MAX_ENT]; };
struct Q3DocPiece { const float* src; long long j0, L, dst; int32_t count, F; };
struct Q3DocPiecePack { Q3DocPiece e[Q3_DOC_MAX_ENT]; };
void q3_launch_doc_scan(const Q3DocScanPack& ents, int n_ent, hipStream_t s);
void q3_launch_doc_emit(const Q3DocPiecePack& pcs, int n_pc, int i16, void* dst, hipStream_t s);
// A document with a speed or an output rate: the ring forms of k_pcm_tempo / k_pcm_resample (q3_tempo.hip, q3_resample.hip; one copy of
// each arithmetic, two addressings). A ring of C f32 (C a multiple of 4, an allocation of its own) holds position g of a stream at
// g mod C. k_doc_tempo: frames [k_from, k_to) of the n joined samples in rj into rt, outputs m >= n_out not written, *p_last as
// Q3TempoEnt's, delta[k] for k < delta_cap. k_doc_resample: outputs [first, first + count) of the n samples in `ring` (fin: all there
// will be) to dst[dst_off, ...), f32 or i16; -1 (nothing launched): one tile's span does not fit the LDS. What may be read and what may
// be overwritten is the host's arithmetic: q3_doc_ring_step (q3_engine.h).
void q3_launch_doc_tempo(const float* rj, long long cj, float* rt, long long ct, long long* p_last, const float* win, int permille, long long n,
                         int k_from, int k_to, long long n_out, int32_t* delta, size_t delta_cap, hipStream_t s);
int q3_launch_doc_resample(const float* ring, long long C, long long n, bool fin, long long first, long long count, const Q3Resamp& rs, int i16,
                           void* dst, long long dst_off, hipStream_t s);

// Tile sweep of the decoder's GEMM (csrc/q3_bgemm.hip) at the row counts of engines with more than 64 slots: every decode
// shape of both transformers and the two heads at 96, 128, 192 and 256 rows (the Predictor's pass A runs twice the rows: 192 .. 512), every
// (RT, NT) instance forced (q3_bgemm_force), the launcher's own choice, and k_bgemm_big where it is eligible (>= 256 rows, N % 128 == 0).
// Weights cold (rotating through copies larger than L2 + Infinity Cache: the Talker) or hot (one copy: the Predictor). Prints us per
// launch inside a replayed hipGraph of 40 dependent launches; tools/bgemm_tune.hip is the same measurement at 1 .. 64 rows.
// Build: hipcc --offload-arch=gfx950 -O3 -std=c++17 -I qwen3-tts-rust_amd/csrc -o tools/slots_gemm_sweep tools/slots_gemm_sweep.hip -L qwen3-tts-rust_amd/csrc -lq3tts -Wl,-rpath,'$ORIGIN/../qwen3-tts-rust_amd/csrc'
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "q3_kernels.h"
#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("%s: %s\n", #x, hipGetErrorString(e_)); return 1; } } while (0)

struct Shape { const char* name; int K, N, epi, scaled, cold, pass_a; };
static const int MAX_ROWS = 512, MAX_K = 8192, MAX_N = 16384;

int main() {
    hipStream_t s; CK(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
    const Shape shapes[] = {
        {"T qkv", 2048, 4096, Q3_EPI_STORE, 1, 1, 0}, {"T o", 2048, 2048, Q3_EPI_RESID, 0, 1, 0}, {"T gate/up", 2048, 12288, Q3_EPI_SWIGLU, 1, 1, 0},
        {"T down", 6144, 2048, Q3_EPI_RESID, 0, 1, 0}, {"T head", 2048, 3072, Q3_EPI_STORE, 1, 1, 0},
        {"P qkv", 1024, 4096, Q3_EPI_STORE, 1, 0, 0}, {"P o", 2048, 1024, Q3_EPI_RESID, 0, 0, 0}, {"P gate/up", 1024, 6144, Q3_EPI_SWIGLU, 1, 0, 0},
        {"P down", 3072, 1024, Q3_EPI_RESID, 0, 0, 0}, {"P head", 1024, 2048, Q3_EPI_ARGMAX, 1, 0, 0},
        {"PA qkv", 1024, 4096, Q3_EPI_STORE, 1, 0, 1}, {"PA o", 2048, 1024, Q3_EPI_RESID, 0, 0, 1}, {"PA gate/up", 1024, 6144, Q3_EPI_SWIGLU, 1, 0, 1},
        {"PA down", 3072, 1024, Q3_EPI_RESID, 0, 0, 1},
    };
    const size_t WBYTES = (size_t)2 << 30;
    uint4* w; CK(hipMalloc(&w, WBYTES)); CK(hipMemset(w, 0x3c, WBYTES));
    uint16_t *a, *yb; float *y, *ssp, *sso, *nw; unsigned long long* keys;
    CK(hipMalloc(&a, (size_t)MAX_ROWS * MAX_K * 2)); CK(hipMemset(a, 0x3c, (size_t)MAX_ROWS * MAX_K * 2));
    CK(hipMalloc(&yb, (size_t)MAX_ROWS * MAX_N * 2)); CK(hipMalloc(&y, (size_t)MAX_ROWS * MAX_N * 4)); CK(hipMemset(y, 0, (size_t)MAX_ROWS * MAX_N * 4));
    CK(hipMalloc(&ssp, (size_t)MAX_ROWS * 512 * 4)); CK(hipMemset(ssp, 0x3c, (size_t)MAX_ROWS * 512 * 4)); CK(hipMalloc(&sso, (size_t)MAX_ROWS * 1024 * 4));
    CK(hipMalloc(&nw, MAX_N * 4)); CK(hipMemset(nw, 0x3c, MAX_N * 4)); CK(hipMalloc(&keys, (size_t)MAX_ROWS * 1024 * 8));
    q3_bgemm_prepare();
    hipEvent_t e0, e1; CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
    const int iters = 40;
    // one configuration: force (rt, nt) (0, 0: the launcher's choice) under big policy `big`; us per launch, or < 0 when refused
    auto measure = [&](const Shape& sh, int M, int rt, int nt, int big, float* us) -> int {
        if (M > MAX_ROWS || sh.K > MAX_K || sh.N > MAX_N || sh.K / 16 > 512 || sh.N / 16 > 1024) return 1;  // the buffers above
        const size_t wb = (size_t)sh.N * sh.K * 2;
        const int copies = sh.cold ? (int)(WBYTES / wb) : 1;
        q3_bgemm_force(rt, nt); q3_bgemm_big_policy(big);
        hipGraph_t g; hipGraphExec_t ge;
        CK(hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal));
        int refused = 0;
        for (int i = 0; i < iters && !refused; ++i) {
            Q3BGemm q{}; q.a = a; q.B = M; q.w = (const uint4*)((const char*)w + (size_t)(i % copies) * wb); q.K = sh.K; q.N = sh.N; q.w_once = sh.cold;
            if (sh.scaled) { q.ssp = ssp; q.ld_ssp = sh.K / 16; q.ntiles = sh.K / 16; q.d_norm = sh.K; q.eps = 1e-6f; }
            q.epi = sh.epi; q.y = y; q.ldy = sh.N; q.yb = yb; q.keys = keys; q.key_stride = sh.N / 16;
            if (sh.epi == Q3_EPI_RESID) { q.nw_next = nw; q.ssp_out = sso; q.ld_ssp_out = sh.N / 16; }
            refused = q3_launch_bgemm(q, s);
        }
        CK(hipStreamEndCapture(s, &g));
        if (refused) { hipGraphDestroy(g); *us = -1.0f; return 0; }
        CK(hipGraphInstantiate(&ge, g, nullptr, nullptr, 0));
        CK(hipGraphLaunch(ge, s)); CK(hipStreamSynchronize(s));
        float tot = 0;
        for (int rep = 0; rep < 3; ++rep) {
            CK(hipEventRecord(e0, s)); CK(hipGraphLaunch(ge, s)); CK(hipEventRecord(e1, s)); CK(hipEventSynchronize(e1));
            float ms = 0; hipEventElapsedTime(&ms, e0, e1); tot += ms;
        }
        *us = tot * 1e3f / (3 * iters);
        hipGraphExecDestroy(ge); hipGraphDestroy(g);
        return 0;
    };
    for (const Shape& sh : shapes)
        for (int slots : {96, 128, 192, 256}) {
            const int M = sh.pass_a ? 2 * slots : slots;
            int prt, pnt, pd, pntw, pbig;
            q3_bgemm_force(0, 0); q3_bgemm_big_policy(0);
            { Q3BGemm q{}; q.B = M; q.K = sh.K; q.N = sh.N; q.epi = sh.epi; q.w_once = sh.cold; q3_bgemm_pick(q, &prt, &pnt, &pd, &pntw, &pbig); }
            float chosen = 0;
            if (measure(sh, M, 0, 0, 0, &chosen)) return 1;
            printf("%-10s M=%3d K=%4d N=%5d %s: launcher %s(%d,%d) %6.2f |", sh.name, M, sh.K, sh.N, sh.cold ? "cold" : "hot ", pbig ? "big" : "", prt, pnt, chosen);
            float best = 1e9f; int brt = 0, bnt = 0;
            for (int rt = 1; rt <= 4; ++rt)
                for (int nt = 1; nt <= 3; ++nt) {
                    if ((sh.N / 16) % nt) continue;
                    float us = 0;
                    if (measure(sh, M, rt, nt, -1, &us)) return 1;
                    printf(" (%d,%d) %6.2f", rt, nt, us);
                    if (us > 0 && us < best) { best = us; brt = rt; bnt = nt; }
                }
            if (M >= 256 && sh.N % 128 == 0 && sh.epi != Q3_EPI_ARGMAX) {
                float us = 0;
                if (measure(sh, M, 0, 0, 1, &us)) return 1;
                printf(" big %6.2f", us);
                if (us > 0 && us < best) { best = us; brt = 8; bnt = 8; }
            }
            printf("  -> best %s(%d,%d) %.2f us (launcher %+.0f%%)\n", brt == 8 ? "big" : "", brt, bnt, best, 100.0f * (chosen - best) / best);
            fflush(stdout);
        }
    q3_bgemm_force(0, 0); q3_bgemm_big_policy(0);
    return 0;
}

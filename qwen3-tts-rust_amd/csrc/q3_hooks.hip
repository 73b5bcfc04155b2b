// q3_hooks.hip — the kernel-level test hooks q3tts_k_* of include/q3tts.h: each uploads its arguments, launches one kernel (or one engine
// step) through the launcher the engine uses, and reads the result back. No engine code: the tests and the benchmarks of single kernels
// call these. (The hooks of the vocoder, the clone encoders and the GGUF reader that need an engine's state are in those files, beside it;
// the clone quantiser's hook needs none and is here.)
#include "q3_engine.h"

#include <cstdio>
#include <cstring>

#define HK(call) do { hipError_t er__ = (call); if (er__ != hipSuccess) return q3_set_err(nullptr, Q3TTS_ERR_DEVICE, std::string(#call) + ": " + hipGetErrorString(er__)); } while (0)

// A device buffer of a hook, freed on every return path. put: `bytes` (+ 64 of slack) of zero-filled memory, then the host's `bytes` when
// host != NULL; get: the first `bytes` back. Synchronous copies on the NULL stream. Both return a Q3TTS_ status (error text set).
struct DevBuf {
    void* p = nullptr;
    ~DevBuf() { if (p) hipFree(p); }
    template <class T> operator T*() const { return (T*)p; }
    int put(const void* host, size_t bytes) {
        if (hipMalloc(&p, bytes + 64) != hipSuccess || hipMemset(p, 0, bytes + 64) != hipSuccess) return q3_set_err(nullptr, Q3TTS_ERR_OOM, "hipMalloc");
        if (host) HK(hipMemcpy(p, host, bytes, hipMemcpyHostToDevice));
        return Q3TTS_OK;
    }
    int alloc(size_t bytes) { return put(nullptr, bytes); }
    int get(void* host, size_t bytes) const { HK(hipMemcpy(host, p, bytes, hipMemcpyDeviceToHost)); return Q3TTS_OK; }
};

// mean time of a launch: one untimed warm-up, then `iters` launches between two events on the NULL stream (nothing when iters <= 0 or !mean_ms)
template <class F>
static int time_launches(int iters, F launch, float* mean_ms) {
    if (iters <= 0 || !mean_ms) return Q3TTS_OK;
    hipEvent_t a, b; HK(hipEventCreate(&a)); HK(hipEventCreate(&b));
    launch();
    HK(hipEventRecord(a, nullptr));
    for (int i = 0; i < iters; ++i) launch();
    HK(hipEventRecord(b, nullptr)); HK(hipEventSynchronize(b));
    float ms = 0; hipEventElapsedTime(&ms, a, b); *mean_ms = ms / iters;
    hipEventDestroy(a); hipEventDestroy(b);
    return Q3TTS_OK;
}

static size_t pad16(size_t rows) { return (rows + 15) & ~(size_t)15; }
// natural row-major bf16 rows <-> the A-tiled layout of the device buffers (q3_kernels.h)
static std::vector<uint16_t> atile_host(const uint16_t* src, int rows, int K) {
    std::vector<uint16_t> out(pad16(rows) * K, 0);
    for (int r = 0; r < rows; ++r) for (int k = 0; k < K; ++k) out[q3_atile_off(r, k, K >> 5)] = src[(size_t)r * K + k];
    return out;
}
static int untile_host(const DevBuf& d, int rows, int K, uint16_t* dst) {  // (reads the device buffer back first)
    std::vector<uint16_t> t(pad16(rows) * K);
    TRY(d.get(t.data(), t.size() * 2));
    for (int r = 0; r < rows; ++r) for (int k = 0; k < K; ++k) dst[(size_t)r * K + k] = t[q3_atile_off(r, k, K >> 5)];
    return Q3TTS_OK;
}
// q int8 [N][K] + d_f16 [N][K/32] -> the rows as a GGUF file holds them: block_q8_0 = f16 d, 32 x int8
static std::vector<uint8_t> pack_q8_0(const int8_t* q, const uint16_t* d_f16, int N, int K) {
    const int kb = K / 32;
    std::vector<uint8_t> blocks((size_t)N * kb * 34);
    for (size_t n = 0; n < (size_t)N; ++n)
        for (int b = 0; b < kb; ++b) {
            uint8_t* blk = &blocks[(n * kb + b) * 34];
            const uint16_t dd = d_f16[n * kb + b];
            blk[0] = (uint8_t)(dd & 0xff); blk[1] = (uint8_t)(dd >> 8);
            memcpy(blk + 2, q + n * K + (size_t)b * 32, 32);
        }
    return blocks;
}
// Tile a row-major [N][K] weight on the device for the GEMM kernels. sc == NULL: src holds bf16 bits; else src holds block_q8_0 rows and
// sc receives the f16 block scales. swiglu: src is the N/2 gate rows, then the N/2 up rows (interleaved in dst).
static void tile_weight(const DevBuf& src, const DevBuf& dst, const DevBuf* sc, int N, int K, bool swiglu) {
    Q3Fill f{}; f.dst = dst; f.N = N; f.K = K; f.mode = swiglu ? 1 : 0;
    if (!swiglu) { f.row0 = 0; f.rows = N; }
    const size_t up = (size_t)(N / 2) * (sc ? (size_t)(K / 32) * 34 : (size_t)K * 2);  // byte offset of the up rows
    if (sc) {
        f.dst_scale = *sc; f.src8_a = src; if (swiglu) f.src8_b = f.src8_a + up;
        q3_launch_fill_tiled_q8(f, nullptr);
    } else {
        f.src_a = src; if (swiglu) f.src_b = (const uint16_t*)((const char*)src.p + up);
        q3_launch_fill_tiled(f, nullptr);
    }
}

extern "C" int q3tts_k_gemm_exact(int32_t device, const float* x, int32_t B, int32_t K, const uint16_t* w, int32_t N, const float* norm_w,
                                  float eps, const float* bias, int32_t epi, float* y, uint64_t* keys, int32_t iters, float* mean_ms) {
    if (!x || !w || !y || B <= 0 || K % 512 || N % 16 || (norm_w && K > 8192)) return q3_set_err(nullptr, Q3TTS_ERR_INVALID, "gemm hook: bad shape");
    if (epi == Q3_EPI_SWIGLU && (N % 32)) return q3_set_err(nullptr, Q3TTS_ERR_INVALID, "swiglu needs N % 32 == 0");
    HK(hipSetDevice(device));
    const int F = N / 2;
    const size_t ny = epi == Q3_EPI_SWIGLU ? (size_t)B * F : (size_t)B * N;
    DevBuf dx, dw, dwt, dn, db, dy, dk;
    TRY(dx.put(x, (size_t)B * K * 4)); TRY(dw.put(w, (size_t)N * K * 2)); TRY(dwt.alloc((size_t)N * K * 2)); TRY(dn.put(norm_w, (size_t)K * 4));
    TRY(db.put(bias, (size_t)N * 4)); TRY(dy.put(epi == Q3_EPI_RESID ? y : nullptr, ny * 4)); TRY(dk.alloc((size_t)B * 8));
    tile_weight(dw, dwt, nullptr, N, K, epi == Q3_EPI_SWIGLU);
    Q3Gemm g{}; g.x = dx; g.ldx = K; g.B = B; g.w = dwt; g.K = K; g.N = N; g.eps = eps; g.epi = epi;
    if (norm_w) g.norm_w = dn;
    if (bias) g.bias = db;
    g.y = dy; g.ldy = epi == Q3_EPI_SWIGLU ? F : N; g.keys = dk; g.key_stride = 1;
    q3_launch_gemm(g, nullptr);
    HK(hipDeviceSynchronize());
    if (epi == Q3_EPI_ARGMAX) {
        if (keys) TRY(dk.get(keys, (size_t)B * 8));
    } else TRY(dy.get(y, ny * 4));
#ifdef Q3_STAMPS
    {  // experiment builds: phase stamps of workgroup 0 / wave 0 of one warm launch (shader-clock cycles from kernel entry)
        DevBuf dd; dd.alloc(64 * 8);
        g.dbg = nullptr; q3_launch_gemm(g, nullptr); q3_launch_gemm(g, nullptr);
        g.dbg = (unsigned long long*)dd.p; hipMemset(dd.p, 0, 64 * 8);
        q3_launch_gemm(g, nullptr); hipDeviceSynchronize();
        unsigned long long st[8]; hipMemcpy(st, dd.p, 64, hipMemcpyDeviceToHost);
        fprintf(stderr, "stamps B=%d K=%d N=%d norm=%d epi=%d: entry->loop %llu | first operands %llu | loop end %llu | barrier %llu | sums %llu | stores done %llu\n",
                B, K, N, norm_w ? 1 : 0, epi, st[1] - st[0], st[2] - st[0], st[3] - st[0], st[4] - st[0], st[5] - st[0], st[6] - st[0]);
        unsigned long long ws[64]; hipMemcpy(ws, dd.p, 64 * 8, hipMemcpyDeviceToHost);
        for (int w = 0; w < 8; ++w)
            fprintf(stderr, "   wave %d: first operands %llu, mid loop %llu, loop end %llu\n", w, ws[8 + w * 4] - st[0], ws[8 + w * 4 + 1] - st[0], ws[8 + w * 4 + 2] - st[0]);
        g.dbg = nullptr;
    }
#endif
    g.epi = epi == Q3_EPI_RESID ? Q3_EPI_STORE : epi;
    return time_launches(iters, [&] { q3_launch_gemm(g, nullptr); }, mean_ms);
}

extern "C" int q3tts_k_attention(int32_t device, const float* qkv, int32_t n_rows, int32_t pos0, int32_t Hq, int32_t Hkv, int32_t hd,
                                 const float* qnw, const float* knw, float eps, float theta, const int32_t* sections, float* out) {
    if (!qkv || !out || hd != 128 || n_rows <= 0 || Hkv <= 0 || Hq % Hkv) return q3_set_err(nullptr, Q3TTS_ERR_INVALID, "attention hook: bad shape");
    HK(hipSetDevice(device));
    const int n_ctx = ((pos0 + n_rows + 63) / 64) * 64, ld = (Hq + 2 * Hkv) * hd;
    std::vector<float> cs, sn;
    q3_rope_tables(n_ctx, hd, theta, sections, cs, sn);
    std::vector<int> rp(n_rows), rs(n_rows, 0);
    for (int i = 0; i < n_rows; ++i) rp[i] = pos0 + i;
    DevBuf dq, dout, dqn, dkn, dcs, dsn, dkc, dvc, drp, drs;
    TRY(dq.put(qkv, (size_t)n_rows * ld * 4)); TRY(dout.alloc((size_t)n_rows * Hq * hd * 4)); TRY(dqn.put(qnw, hd * 4)); TRY(dkn.put(knw, hd * 4));
    TRY(dcs.put(cs.data(), cs.size() * 4)); TRY(dsn.put(sn.data(), sn.size() * 4));
    TRY(dkc.alloc((size_t)Hkv * n_ctx * hd * 2)); TRY(dvc.alloc((size_t)Hkv * n_ctx * hd * 2));
    TRY(drp.put(rp.data(), n_rows * 4)); TRY(drs.put(rs.data(), n_rows * 4));
    Q3QkPrep qp{}; qp.qkv = dq; qp.ld = ld; qp.rows = n_rows; qp.Hq = Hq; qp.Hkv = Hkv; qp.hd = hd; qp.qnw = dqn; qp.knw = dkn; qp.eps = eps;
    qp.cs = dcs; qp.sn = dsn; qp.kc = dkc; qp.vc = dvc; qp.n_ctx = n_ctx; qp.row_pos = drp; qp.row_slot = drs;
    if (q3_launch_qk_prep(qp, nullptr)) return q3_set_err(nullptr, Q3TTS_ERR_INVALID, "attention hook: the q/k prep launch was refused");
    Q3Attend at{}; at.qkv = dq; at.ld = ld; at.rows = n_rows; at.out = dout; at.ldo = Hq * hd; at.Hq = Hq; at.Hkv = Hkv; at.hd = hd;
    at.kc = dkc; at.vc = dvc; at.n_ctx = n_ctx; at.row_pos = qp.row_pos; at.row_slot = qp.row_slot;
    if (q3_launch_attend(at, nullptr)) return q3_set_err(nullptr, Q3TTS_ERR_INVALID, "attention hook: the attention launch was refused");
    HK(hipDeviceSynchronize());
    return dout.get(out, (size_t)n_rows * Hq * hd * 4);
}

// Decode attention as the engine's frame step runs it: per slot, rows 0 .. len - 2 go through k_qk_prep into a cache of n_ctx positions,
// then ONE fused decode launch (one row per slot at pos = len - 1; q/k prep and the K/V append in-kernel) through q3_launch_attend under
// decode policy `policy` (-1: the current one). qkv holds the slots' rows back to back ([sum lens][(Hq + 2 Hkv) hd]); out_f32 [n_slots][Hq hd];
// out_bf16 (optional): the same launch writing the A-tiled bf16 operand of the O projection, untiled here to [n_slots][Hq hd].
extern "C" int q3tts_k_attention_decode(int32_t device, const float* qkv, int32_t n_slots, const int32_t* lens, int32_t n_ctx, int32_t Hq,
                                        int32_t Hkv, int32_t hd, const float* qnw, const float* knw, float eps, float theta,
                                        const int32_t* sections, int32_t policy, float* out_f32, uint16_t* out_bf16) {
    if (!qkv || !lens || !out_f32 || hd != 128 || n_slots <= 0 || Hkv <= 0 || Hq % Hkv || Hq / Hkv < 2 || n_ctx <= 0 || n_ctx % 64 || policy < -1 || policy > 1)
        return q3_set_err(nullptr, Q3TTS_ERR_INVALID, "attention decode hook: bad shape");
    long long total = 0;
    for (int s = 0; s < n_slots; ++s) {
        if (lens[s] < 1 || lens[s] > n_ctx) return q3_set_err(nullptr, Q3TTS_ERR_INVALID, "attention decode hook: a length outside 1 .. n_ctx");
        total += lens[s];
    }
    HK(hipSetDevice(device));
    const int ld = (Hq + 2 * Hkv) * hd, nq = Hq * hd, npre = (int)(total - n_slots);
    std::vector<float> cs, sn;
    q3_rope_tables(n_ctx, hd, theta, sections, cs, sn);
    std::vector<float> last((size_t)n_slots * ld);
    std::vector<int> pp, ps, dp(n_slots), ds(n_slots);
    pp.reserve(npre); ps.reserve(npre);
    {
        size_t r0 = 0;
        for (int s = 0; s < n_slots; ++s) {
            for (int r = 0; r < lens[s] - 1; ++r) { pp.push_back(r); ps.push_back(s); }
            memcpy(&last[(size_t)s * ld], qkv + (r0 + lens[s] - 1) * ld, (size_t)ld * 4);
            dp[s] = lens[s] - 1; ds[s] = s;
            r0 += lens[s];
        }
    }
    DevBuf dpre, dlast, dout, dob, dqn, dkn, dcs, dsn, dkc, dvc, dpp, dps, ddp, dds;
    const size_t cache = (size_t)n_slots * Hkv * n_ctx * hd * 2, npre1 = (size_t)std::max(npre, 1);
    TRY(dpre.alloc(npre1 * ld * 4)); TRY(dlast.alloc(last.size() * 4)); TRY(dout.alloc((size_t)n_slots * nq * 4)); TRY(dob.alloc(pad16(n_slots) * nq * 2));
    TRY(dqn.put(qnw, hd * 4)); TRY(dkn.put(knw, hd * 4)); TRY(dcs.put(cs.data(), cs.size() * 4)); TRY(dsn.put(sn.data(), sn.size() * 4));
    TRY(dkc.alloc(cache)); TRY(dvc.alloc(cache)); TRY(dpp.alloc(npre1 * 4)); TRY(dps.alloc(npre1 * 4));
    TRY(ddp.put(dp.data(), n_slots * 4)); TRY(dds.put(ds.data(), n_slots * 4));
    {
        size_t r0 = 0, o = 0;
        for (int s = 0; s < n_slots; ++s) {
            const size_t n = lens[s] - 1;
            if (n) HK(hipMemcpy((float*)dpre.p + o * ld, qkv + r0 * ld, n * ld * 4, hipMemcpyHostToDevice));
            o += n; r0 += lens[s];
        }
    }
    if (npre) { HK(hipMemcpy(dpp.p, pp.data(), npre * 4, hipMemcpyHostToDevice)); HK(hipMemcpy(dps.p, ps.data(), npre * 4, hipMemcpyHostToDevice)); }
    Q3QkPrep qp{}; qp.qkv = dpre; qp.ld = ld; qp.rows = npre; qp.Hq = Hq; qp.Hkv = Hkv; qp.hd = hd; qp.qnw = dqn; qp.knw = dkn; qp.eps = eps;
    qp.cs = dcs; qp.sn = dsn; qp.kc = dkc; qp.vc = dvc; qp.n_ctx = n_ctx; qp.row_pos = dpp; qp.row_slot = dps;
    if (npre && q3_launch_qk_prep(qp, nullptr)) return q3_set_err(nullptr, Q3TTS_ERR_INVALID, "attention decode hook: the q/k prep launch was refused");
    int old_dec = 0, old_pre = 0;
    q3_attend_policy_get(&old_dec, &old_pre);
    if (policy >= 0) q3_attend_policy(policy, old_pre);
    for (int pass = 0; pass < (out_bf16 ? 2 : 1); ++pass) {
        // both passes start from the same cache: the fused launch's append rewrites position len - 1 with the same bits
        HK(hipMemcpy(dlast.p, last.data(), last.size() * 4, hipMemcpyHostToDevice));
        Q3QkPrep dq = qp; dq.qkv = dlast; dq.rows = n_slots; dq.row_pos = ddp; dq.row_slot = dds;
        Q3Attend at{}; at.qkv = dlast; at.ld = ld; at.rows = n_slots; at.ldo = nq; at.Hq = Hq; at.Hkv = Hkv; at.hd = hd;
        at.kc = dkc; at.vc = dvc; at.n_ctx = n_ctx; at.row_pos = dq.row_pos; at.row_slot = dq.row_slot;
        at.fused = 1; at.prep = dq;
        if (pass == 0) { at.out = dout; at.out_bf16 = 0; }
        else { at.out = dob; at.out_bf16 = 1; }
        if (q3_launch_attend(at, nullptr)) { q3_attend_policy(old_dec, old_pre); return q3_set_err(nullptr, Q3TTS_ERR_INVALID, "attention decode hook: the attention launch was refused"); }
        const hipError_t er = hipDeviceSynchronize();
        if (er != hipSuccess) { q3_attend_policy(old_dec, old_pre); return q3_set_err(nullptr, Q3TTS_ERR_DEVICE, std::string("attention decode hook: ") + hipGetErrorString(er)); }
    }
    q3_attend_policy(old_dec, old_pre);
    HK(hipGetLastError());
    TRY(dout.get(out_f32, (size_t)n_slots * nq * 4));
    return out_bf16 ? untile_host(dob, n_slots, nq, out_bf16) : Q3TTS_OK;
}

// ---- the attention hooks with every output form and the cache returned (q3tts_k_attention_runs / _decode_ex / _pair) ----------------
// What the three share: the norm weights and RoPE tables of a cache of n_slots x Hkv x n_ctx positions, the output buffers of one form
// (0: f32 rows; 1: the A-tiled bf16 operand; 2: Q8_0 blocks + f32 block scales), the read-back in natural order and the un-blocked cache.
struct AttHook {
    int n_slots = 0, n_ctx = 0, Hq = 0, Hkv = 0, ld = 0, nq = 0, form = 0, out_rows = 0, rt16 = 0;
    int kv8 = 0;  // the cache as Q8_0 blocks (the _kv8 hooks; set before init): kc / vc then hold int8 quants, kd / vd their f16 scales
    DevBuf qn, kn, cs, sn, kc, vc, kd, vd, out, osc;
    // the arguments every attention hook checks before anything is allocated or launched
    static const char* check(const float* qkv, int n_slots, int n_ctx, int Hq, int Hkv, int hd, const float* qnw, const float* knw, int form, const void* out,
                             const float* out_scale) {
        if (!qkv || !qnw || !knw || !out) return "a null argument";
        if (hd != Q3_ATT_HD) return "head_dim must be 128";
        if (n_slots <= 0 || n_slots > 4096) return "1 .. 4096 slots";
        if (n_ctx <= 0 || n_ctx % 64 || n_ctx > 8192) return "n_ctx must be a multiple of 64 in 64 .. 8192";
        if (Hkv <= 0 || Hq <= 0 || Hq % Hkv || Hq > 64) return "n_head must be a multiple of n_kv_head";
        const int R = Hq / Hkv;
        if (R != 1 && R != 2 && R != 4) return "the GQA ratio must be 1, 2 or 4";
        if (form < 0 || form > 2) return "out_form 0 (f32), 1 (bf16) or 2 (Q8_0)";
        if (form == 2 && !out_scale) return "out_form 2 needs out_scale";
        return nullptr;
    }
    int init(int slots, int nctx, int hq, int hkv, const float* qnw, const float* knw, float theta, const int32_t* sections, int out_form, int rows) {
        n_slots = slots; n_ctx = nctx; Hq = hq; Hkv = hkv; ld = (hq + 2 * hkv) * Q3_ATT_HD; nq = hq * Q3_ATT_HD; form = out_form; out_rows = rows;
        rt16 = (int)(pad16(rows) / 16);
        std::vector<float> c, s;
        q3_rope_tables(n_ctx, Q3_ATT_HD, theta, sections, c, s);
        TRY(qn.put(qnw, Q3_ATT_HD * 4)); TRY(kn.put(knw, Q3_ATT_HD * 4)); TRY(cs.put(c.data(), c.size() * 4)); TRY(sn.put(s.data(), s.size() * 4));
        const size_t cache = (size_t)n_slots * Hkv * n_ctx * Q3_ATT_HD * (kv8 ? 1 : 2);
        TRY(kc.alloc(cache)); TRY(vc.alloc(cache));
        if (kv8) { TRY(kd.alloc(cache / 16)); TRY(vd.alloc(cache / 16)); }
        TRY(out.alloc(form == 0 ? (size_t)rows * nq * 4 : pad16(rows) * nq * (form == 1 ? 2 : 1)));
        if (form == 2) TRY(osc.alloc((size_t)(nq / 32 + 2) * pad16(rows) * 4));
        return Q3TTS_OK;
    }
    Q3QkPrep prep(float* rows_dev, int rows, float eps) const {
        Q3QkPrep qp{}; qp.qkv = rows_dev; qp.ld = ld; qp.rows = rows; qp.Hq = Hq; qp.Hkv = Hkv; qp.hd = Q3_ATT_HD; qp.qnw = qn; qp.knw = kn; qp.eps = eps;
        qp.cs = cs; qp.sn = sn; qp.kc = kc; qp.vc = vc; qp.n_ctx = n_ctx;
        if (kv8) { qp.kv8 = 1; qp.kd = kd; qp.vd = vd; }
        return qp;
    }
    Q3Attend attend(const float* rows_dev, int rows) const {
        Q3Attend at{}; at.qkv = rows_dev; at.ld = ld; at.rows = rows; at.out = out; at.ldo = nq; at.out_bf16 = form; at.Hq = Hq; at.Hkv = Hkv; at.hd = Q3_ATT_HD;
        at.kc = kc; at.vc = vc; at.n_ctx = n_ctx;
        if (kv8) { at.kv8 = 1; at.kd = kd; at.vd = vd; }
        if (form == 2) { at.out_scale = osc; at.out_rt16 = rt16; }
        return at;
    }
    // the output rows in natural order: f32 / bf16 bits [rows][nq], or int8 [rows][nq] + f32 [rows][nq / 32]
    int read_out(void* host, float* host_scale) const {
        if (form == 0) return out.get(host, (size_t)out_rows * nq * 4);
        if (form == 1) return untile_host(out, out_rows, nq, (uint16_t*)host);
        const size_t B16 = pad16(out_rows);
        std::vector<int8_t> qt(B16 * nq); std::vector<float> st((size_t)(nq / 32) * B16);
        TRY(out.get(qt.data(), qt.size())); TRY(osc.get(st.data(), st.size() * 4));
        for (int r = 0; r < out_rows; ++r) {
            for (int k = 0; k < nq; ++k) ((int8_t*)host)[(size_t)r * nq + k] = qt[q3_q8_off(r, k, nq >> 6)];
            for (int b = 0; b < nq / 32; ++b) host_scale[(size_t)r * (nq / 32) + b] = st[q3_q8_scale_idx(r, b, rt16)];
        }
        return Q3TTS_OK;
    }
    // the cache of every slot as bf16 bits [slot][Hkv][n_ctx][hd]: keys out of their 64-key blocks (k_cache_elem), values as stored
    int read_cache(uint16_t* k_host, uint16_t* v_host) const {
        constexpr int hd = Q3_ATT_HD;
        const size_t n = (size_t)n_slots * Hkv * n_ctx * hd;
        if (v_host) TRY(vc.get(v_host, n * 2));
        if (!k_host) return Q3TTS_OK;
        std::vector<uint16_t> t(n);
        TRY(kc.get(t.data(), n * 2));
        for (size_t h = 0; h < (size_t)n_slots * Hkv; ++h)
            for (int pos = 0; pos < n_ctx; ++pos)
                for (int d = 0; d < hd; ++d)
                    k_host[(h * n_ctx + pos) * hd + d] = t[h * n_ctx * hd + ((size_t)((pos >> 6) * (hd >> 3) + (d >> 3)) * 64 + (pos & 63)) * 8 + (d & 7)];
        return Q3TTS_OK;
    }
    // the Q8_0 cache of every slot, un-blocked: quants int8 [slot][Hkv][n_ctx][hd], scales f16 bits [slot][Hkv][n_ctx][hd / 32] (each optional)
    int read_cache_kv8(int8_t* kq_host, int8_t* vq_host, uint16_t* kd_host, uint16_t* vd_host) const {
        constexpr int hd = Q3_ATT_HD, nb = hd / 32;
        const size_t n = (size_t)n_slots * Hkv * n_ctx * hd, heads = (size_t)n_slots * Hkv;
        if (vq_host) TRY(vc.get(vq_host, n));
        if (vd_host) TRY(vd.get(vd_host, n / 16));
        if (kq_host) {
            std::vector<int8_t> t(n);
            TRY(kc.get(t.data(), n));
            for (size_t h = 0; h < heads; ++h)
                for (int pos = 0; pos < n_ctx; ++pos)
                    for (int d = 0; d < hd; ++d) kq_host[(h * n_ctx + pos) * hd + d] = t[h * n_ctx * hd + q3_kv8_k_off(pos, d)];
        }
        if (kd_host) {
            std::vector<uint16_t> t(n / 32);
            TRY(kd.get(t.data(), n / 16));
            for (size_t h = 0; h < heads; ++h)
                for (int pos = 0; pos < n_ctx; ++pos)
                    for (int j = 0; j < nb; ++j) kd_host[(h * n_ctx + pos) * nb + j] = t[h * n_ctx * nb + q3_kv8_kd_idx(pos, j)];
        }
        return Q3TTS_OK;
    }
};
// what a hook hands back of the cache: bf16 bits (k16 / v16), or with kv8 the quants and scales
struct AttCacheOut { int kv8 = 0; uint16_t *k16 = nullptr, *v16 = nullptr; int8_t *kq = nullptr, *vq = nullptr; uint16_t *kd = nullptr, *vd = nullptr; };
static int att_read_cache(const AttHook& h, const AttCacheOut& c) {
    return c.kv8 ? h.read_cache_kv8(c.kq, c.vq, c.kd, c.vd) : h.read_cache(c.k16, c.v16);
}
// one attention launch of a hook under a temporary policy (-1: keep), then the device's verdict
static int att_hook_launch(const char* name, const Q3Attend& at, int decode, int prefill) {
    int old_dec = 0, old_pre = 0;
    q3_attend_policy_get(&old_dec, &old_pre);
    q3_attend_policy(decode >= 0 ? decode : old_dec, prefill >= 0 ? prefill : old_pre);
    const int refused = q3_launch_attend(at, nullptr);
    q3_attend_policy(old_dec, old_pre);
    if (refused) return q3_set_err(nullptr, Q3TTS_ERR_INVALID, std::string(name) + ": the attention launch was refused");
    hipError_t er = hipGetLastError();
    if (er == hipSuccess) er = hipDeviceSynchronize();
    if (er != hipSuccess) return q3_set_err(nullptr, Q3TTS_ERR_DEVICE, std::string(name) + ": " + hipGetErrorString(er));
    return Q3TTS_OK;
}

// Whole prompt runs as admit_group launches them: run i has run_pos0[i] prefix rows (prepared into slot i's cache by k_qk_prep: they stand for
// a voice prefix) followed by run_n[i] rows; qkv holds run 0's run_pos0[0] + run_n[0] rows, then run 1's, ... The runs' rows go through
// k_qk_prep and ONE non-fused q3_launch_attend that carries the seg table, seg_max_n and seg_max_t, under prefill policy `policy`.
static int attention_runs(int32_t device, const float* qkv, int32_t n_runs, const int32_t* run_n, const int32_t* run_pos0, int32_t n_ctx, int32_t Hq,
                          int32_t Hkv, int32_t hd, const float* qnw, const float* knw, float eps, float theta, const int32_t* sections,
                          int32_t policy, int32_t out_form, void* out, float* out_scale, const AttCacheOut& cache) {
    const std::string hook = cache.kv8 ? "attention runs_kv8 hook" : "attention runs hook";   // (the exported entry that was called)
    if (const char* why = AttHook::check(qkv, n_runs, n_ctx, Hq, Hkv, hd, qnw, knw, out_form, out, out_scale))
        return q3_set_err(nullptr, Q3TTS_ERR_INVALID, hook + ": " + why);
    if (!run_n || !run_pos0 || policy < -1 || policy > 2) return q3_set_err(nullptr, Q3TTS_ERR_INVALID, hook + ": run tables, prefill policy -1 .. 2");
    long long n_pre = 0, n_run = 0;
    int seg_max_n = 0, seg_max_t = 0;
    for (int i = 0; i < n_runs; ++i) {
        if (run_n[i] < 1 || run_pos0[i] < 0 || (long long)run_pos0[i] + run_n[i] > n_ctx)
            return q3_set_err(nullptr, Q3TTS_ERR_INVALID, hook + ": a run needs n >= 1, pos0 >= 0 and pos0 + n <= n_ctx");
        n_pre += run_pos0[i]; n_run += run_n[i];
        seg_max_n = std::max(seg_max_n, run_n[i]); seg_max_t = std::max(seg_max_t, run_pos0[i] + run_n[i]);
    }
    HK(hipSetDevice(device));
    AttHook h; h.kv8 = cache.kv8;
    TRY(h.init(n_runs, n_ctx, Hq, Hkv, qnw, knw, theta, sections, out_form, (int)n_run));
    const int ld = h.ld;
    std::vector<float> pre((size_t)std::max<long long>(n_pre, 1) * ld), run((size_t)n_run * ld);
    std::vector<int> pp, ps, rp, rs, seg;
    {
        size_t src = 0, ip = 0, ir = 0;
        for (int i = 0; i < n_runs; ++i) {
            seg.push_back((int)ir); seg.push_back(run_n[i]); seg.push_back(i); seg.push_back(run_pos0[i]);
            for (int r = 0; r < run_pos0[i]; ++r, ++src, ++ip) { memcpy(&pre[ip * ld], qkv + src * ld, (size_t)ld * 4); pp.push_back(r); ps.push_back(i); }
            for (int r = 0; r < run_n[i]; ++r, ++src, ++ir) { memcpy(&run[ir * ld], qkv + src * ld, (size_t)ld * 4); rp.push_back(run_pos0[i] + r); rs.push_back(i); }
        }
    }
    DevBuf dpre, drun, dpp, dps, drp, drs, dseg;
    TRY(dpre.put(pre.data(), pre.size() * 4)); TRY(drun.put(run.data(), run.size() * 4));
    TRY(dpp.put(pp.data(), pp.size() * 4)); TRY(dps.put(ps.data(), ps.size() * 4));
    TRY(drp.put(rp.data(), rp.size() * 4)); TRY(drs.put(rs.data(), rs.size() * 4)); TRY(dseg.put(seg.data(), seg.size() * 4));
    if (n_pre) {
        Q3QkPrep qp = h.prep(dpre, (int)n_pre, eps); qp.row_pos = dpp; qp.row_slot = dps;
        if (q3_launch_qk_prep(qp, nullptr)) return q3_set_err(nullptr, Q3TTS_ERR_INVALID, hook + ": the q/k prep launch was refused");
    }
    Q3QkPrep qp = h.prep(drun, (int)n_run, eps); qp.row_pos = drp; qp.row_slot = drs;
    if (q3_launch_qk_prep(qp, nullptr)) return q3_set_err(nullptr, Q3TTS_ERR_INVALID, hook + ": the q/k prep launch was refused");
    Q3Attend at = h.attend(drun, (int)n_run); at.row_pos = drp; at.row_slot = drs;
    at.seg = dseg; at.n_seg = n_runs; at.seg_max_n = seg_max_n; at.seg_max_t = seg_max_t;
    TRY(att_hook_launch(hook.c_str(), at, -1, policy));
    TRY(h.read_out(out, out_scale));
    return att_read_cache(h, cache);
}
extern "C" int q3tts_k_attention_runs(int32_t device, const float* qkv, int32_t n_runs, const int32_t* run_n, const int32_t* run_pos0, int32_t n_ctx, int32_t Hq,
                                      int32_t Hkv, int32_t hd, const float* qnw, const float* knw, float eps, float theta, const int32_t* sections,
                                      int32_t policy, int32_t out_form, void* out, float* out_scale, uint16_t* k_cache, uint16_t* v_cache) {
    AttCacheOut c; c.k16 = k_cache; c.v16 = v_cache;
    return attention_runs(device, qkv, n_runs, run_n, run_pos0, n_ctx, Hq, Hkv, hd, qnw, knw, eps, theta, sections, policy, out_form, out, out_scale, c);
}
// ... over a Q8_0 cache (kv_q8_0): the same rows, the quantising append, one launch through q3_launch_attend with kv8 set
extern "C" int q3tts_k_attention_runs_kv8(int32_t device, const float* qkv, int32_t n_runs, const int32_t* run_n, const int32_t* run_pos0, int32_t n_ctx, int32_t Hq,
                                          int32_t Hkv, int32_t hd, const float* qnw, const float* knw, float eps, float theta, const int32_t* sections,
                                          int32_t policy, int32_t out_form, void* out, float* out_scale, int8_t* k_q, int8_t* v_q, uint16_t* k_d, uint16_t* v_d) {
    AttCacheOut c; c.kv8 = 1; c.kq = k_q; c.vq = v_q; c.kd = k_d; c.vd = v_d;
    return attention_runs(device, qkv, n_runs, run_n, run_pos0, n_ctx, Hq, Hkv, hd, qnw, knw, eps, theta, sections, policy, out_form, out, out_scale, c);
}

// q3tts_k_attention_decode with one output form of the three per call, the cache returned, and (row_indexed = 1) the Predictor's addressing:
// no row tables, slot = row % n_slots, every slot at the same length (pos_const = lens[0] - 1)
static int attention_decode_ex(int32_t device, const float* qkv, int32_t n_slots, const int32_t* lens, int32_t n_ctx, int32_t Hq, int32_t Hkv,
                               int32_t hd, const float* qnw, const float* knw, float eps, float theta, const int32_t* sections, int32_t policy,
                               int32_t row_indexed, int32_t out_form, void* out, float* out_scale, const AttCacheOut& cache) {
    const std::string hook = cache.kv8 ? "attention decode_kv8 hook" : "attention decode_ex hook";
    if (const char* why = AttHook::check(qkv, n_slots, n_ctx, Hq, Hkv, hd, qnw, knw, out_form, out, out_scale))
        return q3_set_err(nullptr, Q3TTS_ERR_INVALID, hook + ": " + why);
    if (!lens || Hq / Hkv < 2 || policy < -1 || policy > 1 || row_indexed < 0 || row_indexed > 1)
        return q3_set_err(nullptr, Q3TTS_ERR_INVALID, hook + ": lens, a GQA ratio of 2 or 4, decode policy -1 .. 1, row_indexed 0 / 1");
    long long total = 0;
    for (int s = 0; s < n_slots; ++s) {
        if (lens[s] < 1 || lens[s] > n_ctx) return q3_set_err(nullptr, Q3TTS_ERR_INVALID, hook + ": a length outside 1 .. n_ctx");
        if (row_indexed && lens[s] != lens[0]) return q3_set_err(nullptr, Q3TTS_ERR_INVALID, hook + ": row-indexed addressing needs equal lengths");
        total += lens[s];
    }
    HK(hipSetDevice(device));
    AttHook h; h.kv8 = cache.kv8;
    TRY(h.init(n_slots, n_ctx, Hq, Hkv, qnw, knw, theta, sections, out_form, n_slots));
    const int ld = h.ld, npre = (int)(total - n_slots);
    std::vector<float> pre((size_t)std::max(npre, 1) * ld), last((size_t)n_slots * ld);
    std::vector<int> pp, ps, dp(n_slots), ds(n_slots);
    {
        size_t src = 0, ip = 0;
        for (int s = 0; s < n_slots; ++s) {
            for (int r = 0; r < lens[s] - 1; ++r, ++src, ++ip) { memcpy(&pre[ip * ld], qkv + src * ld, (size_t)ld * 4); pp.push_back(r); ps.push_back(s); }
            memcpy(&last[(size_t)s * ld], qkv + src * ld, (size_t)ld * 4); ++src;
            dp[s] = lens[s] - 1; ds[s] = s;
        }
    }
    DevBuf dpre, dlast, dpp, dps, ddp, dds;
    TRY(dpre.put(pre.data(), pre.size() * 4)); TRY(dlast.put(last.data(), last.size() * 4));
    TRY(dpp.put(pp.data(), pp.size() * 4)); TRY(dps.put(ps.data(), ps.size() * 4)); TRY(ddp.put(dp.data(), n_slots * 4)); TRY(dds.put(ds.data(), n_slots * 4));
    if (npre) {
        Q3QkPrep qp = h.prep(dpre, npre, eps); qp.row_pos = dpp; qp.row_slot = dps;
        if (q3_launch_qk_prep(qp, nullptr)) return q3_set_err(nullptr, Q3TTS_ERR_INVALID, hook + ": the q/k prep launch was refused");
    }
    Q3QkPrep dq = h.prep(dlast, n_slots, eps);
    Q3Attend at = h.attend(dlast, n_slots);
    if (row_indexed) { dq.slot_mod = at.slot_mod = n_slots; dq.pos_const = at.pos_const = lens[0] - 1; }
    else { dq.row_pos = at.row_pos = ddp; dq.row_slot = at.row_slot = dds; }
    at.fused = 1; at.prep = dq;
    TRY(att_hook_launch(hook.c_str(), at, policy, -1));
    TRY(h.read_out(out, out_scale));
    return att_read_cache(h, cache);
}
extern "C" int q3tts_k_attention_decode_ex(int32_t device, const float* qkv, int32_t n_slots, const int32_t* lens, int32_t n_ctx, int32_t Hq, int32_t Hkv,
                                           int32_t hd, const float* qnw, const float* knw, float eps, float theta, const int32_t* sections, int32_t policy,
                                           int32_t row_indexed, int32_t out_form, void* out, float* out_scale, uint16_t* k_cache, uint16_t* v_cache) {
    AttCacheOut c; c.k16 = k_cache; c.v16 = v_cache;
    return attention_decode_ex(device, qkv, n_slots, lens, n_ctx, Hq, Hkv, hd, qnw, knw, eps, theta, sections, policy, row_indexed, out_form, out, out_scale, c);
}
extern "C" int q3tts_k_attention_decode_kv8(int32_t device, const float* qkv, int32_t n_slots, const int32_t* lens, int32_t n_ctx, int32_t Hq, int32_t Hkv,
                                            int32_t hd, const float* qnw, const float* knw, float eps, float theta, const int32_t* sections, int32_t policy,
                                            int32_t out_form, void* out, float* out_scale, int8_t* k_q, int8_t* v_q, uint16_t* k_d, uint16_t* v_d) {
    AttCacheOut c; c.kv8 = 1; c.kq = k_q; c.vq = v_q; c.kd = k_d; c.vd = v_d;
    return attention_decode_ex(device, qkv, n_slots, lens, n_ctx, Hq, Hkv, hd, qnw, knw, eps, theta, sections, policy, 0, out_form, out, out_scale, c);
}

// The Predictor's pass A: 2 * n_slots rows — row b at position 0, row n_slots + b at position 1 of slot b — in ONE launch with fused = 2 on an
// empty cache (k_attend_pair); out rows in the same order
extern "C" int q3tts_k_attention_pair(int32_t device, const float* qkv, int32_t n_slots, int32_t n_ctx, int32_t Hq, int32_t Hkv, int32_t hd, const float* qnw,
                                      const float* knw, float eps, float theta, const int32_t* sections, int32_t out_form, void* out, float* out_scale,
                                      uint16_t* k_cache, uint16_t* v_cache) {
    if (const char* why = AttHook::check(qkv, n_slots, n_ctx, Hq, Hkv, hd, qnw, knw, out_form, out, out_scale))
        return q3_set_err(nullptr, Q3TTS_ERR_INVALID, std::string("attention pair hook: ") + why);
    if (Hq / Hkv != 2) return q3_set_err(nullptr, Q3TTS_ERR_INVALID, "attention pair hook: the GQA ratio must be 2");
    HK(hipSetDevice(device));
    AttHook h;
    TRY(h.init(n_slots, n_ctx, Hq, Hkv, qnw, knw, theta, sections, out_form, 2 * n_slots));
    DevBuf drows;
    TRY(drows.put(qkv, (size_t)2 * n_slots * h.ld * 4));
    Q3QkPrep qp = h.prep(drows, 2 * n_slots, eps); qp.slot_mod = n_slots; qp.pos_const = 0;
    Q3Attend at = h.attend(drows, 2 * n_slots); at.slot_mod = n_slots; at.pos_const = 0;
    at.fused = 2; at.prep = qp;
    TRY(att_hook_launch("attention pair hook", at, -1, -1));
    TRY(h.read_out(out, out_scale));
    return h.read_cache(k_cache, v_cache);
}

// The kernel q3_launch_attend takes for a shape under the current policies, without launching: *kernel = 0 / 1 / 2 k_attend<1 / 2 / 4, false>,
// 3 / 4 k_attend<2 / 4, true>, 5 k_attend_gqa2, 6 k_attend_small<2>, 7 k_attend_pair, 8 k_attend_prefill, -1 a launch the launcher refuses
extern "C" int q3tts_k_attend_pick(int32_t fused, int32_t gqa_ratio, int32_t n_ctx, int32_t n_seg, int32_t seg_max_n, int32_t seg_max_t, int32_t n_kv_head,
                                   int32_t* kernel) {
    if (!kernel || fused < 0 || fused > 2 || gqa_ratio <= 0 || gqa_ratio > 64 || n_ctx <= 0 || n_seg < 0 || seg_max_n < 0 || seg_max_t < 0 || n_kv_head <= 0 ||
        n_kv_head > 4096)
        return q3_set_err(nullptr, Q3TTS_ERR_INVALID, "attend pick: bad shape");
    Q3Attend a{}; a.hd = Q3_ATT_HD; a.Hkv = n_kv_head; a.Hq = n_kv_head * gqa_ratio; a.fused = fused; a.n_ctx = n_ctx;
    if (n_seg > 0) { a.seg = (const int*)16; a.n_seg = n_seg; a.seg_max_n = seg_max_n; a.seg_max_t = seg_max_t; }  // (never dereferenced: nothing is launched)
    *kernel = q3_attend_pick(a);
    return Q3TTS_OK;
}
extern "C" int q3tts_k_attend_pick_kv8(int32_t fused, int32_t gqa_ratio, int32_t n_ctx, int32_t n_seg, int32_t seg_max_n, int32_t seg_max_t, int32_t n_kv_head,
                                       int32_t* kernel) {
    if (!kernel || fused < 0 || fused > 2 || gqa_ratio <= 0 || gqa_ratio > 64 || n_ctx <= 0 || n_seg < 0 || seg_max_n < 0 || seg_max_t < 0 || n_kv_head <= 0 ||
        n_kv_head > 4096)
        return q3_set_err(nullptr, Q3TTS_ERR_INVALID, "attend pick (Q8_0 cache): bad shape");
    Q3Attend a{}; a.hd = Q3_ATT_HD; a.Hkv = n_kv_head; a.Hq = n_kv_head * gqa_ratio; a.fused = fused; a.n_ctx = n_ctx; a.kv8 = 1;
    if (n_seg > 0) { a.seg = (const int*)16; a.n_seg = n_seg; a.seg_max_n = seg_max_n; a.seg_max_t = seg_max_t; }  // (never dereferenced: nothing is launched)
    *kernel = q3_attend_pick(a);
    return Q3TTS_OK;
}

// ---- the Predictor's layer-0 QKV table and the gathering attention ----------------------------------------------------
extern "C" int q3tts_k_pred_table_row(q3tts_engine* e, int32_t q, int32_t code, float* out) {
    if (!e || !out) return q3_set_err(e, Q3TTS_ERR_INVALID, "pred table row: null argument");
    Q3_NOT_IN_SESSION(e);
    if (!e->qkv0) return q3_set_err(e, Q3TTS_ERR_STATE, "pred table row: this engine has no layer-0 QKV table");
    if (q < 1 || q > e->cfg.model.n_codebooks - 2) return q3_set_err(e, Q3TTS_ERR_INVALID, "pred table row: q outside 1 .. n_codebooks - 2");
    const int rows = q3_pred_table_rows(e), r = (code >= 0 && code < rows) ? code : rows;  // the kernel's rule: anything else is the fallback row
    Q3_HIP(e, hipSetDevice(e->cfg.device));
    Q3_HIP(e, hipStreamSynchronize(e->stream));
    Q3_HIP(e, hipMemcpy(out, q3_pred_table_slice(e, q) + (size_t)r * e->P.nqkv, (size_t)e->P.nqkv * 4, hipMemcpyDeviceToHost));
    return Q3TTS_OK;
}

// The state one k_pred_next<false>(q) launch, or the bookkeeping column of one gathering attention launch, works on (row b = slot b)
struct PredStepHook {
    DevBuf keys, slots, row_slot, codec, pproj, bias, fb, px, codes;
    static const char* check(const q3tts_k_pred_step* st) {
        if (!st || !st->keys || !st->active || !st->n_frames || !st->codec_q || !st->pproj_q || !st->proj_b || !st->fb || !st->px || !st->codes) return "a null argument";
        if (st->n_rows < 1 || st->n_rows > 4096 || st->n_key_parts < 1 || st->n_key_parts > 4096 || st->rows_q < 1) return "1 .. 4096 rows and key parts, rows_q >= 1";
        if (st->n_codebooks < 3 || st->q < 1 || st->q > st->n_codebooks - 2) return "q in 1 .. n_codebooks - 2";
        if (st->d_embed < 256 || st->d_embed % 256 || st->d_proj < 32 || st->d_proj % 32) return "d_embed % 256 == 0, d_proj % 32 == 0";
        if (st->max_steps_cap < 1) return "max_steps_cap >= 1";
        for (int b = 0; b < st->n_rows; ++b) if (st->n_frames[b] < 0 || st->n_frames[b] >= st->max_steps_cap) return "n_frames in [0, max_steps_cap)";
        return nullptr;
    }
    int init(const q3tts_k_pred_step* st) {
        const size_t B = st->n_rows;
        std::vector<Q3Slot> sl(B); std::vector<int> id(B);
        memset(sl.data(), 0, B * sizeof(Q3Slot));
        for (size_t b = 0; b < B; ++b) { sl[b].active = st->active[b] ? 1 : 0; sl[b].n_frames = st->n_frames[b]; id[b] = (int)b; }
        TRY(keys.put(st->keys, B * st->n_key_parts * 8)); TRY(slots.put(sl.data(), B * sizeof(Q3Slot))); TRY(row_slot.put(id.data(), B * 4));
        TRY(codec.put(st->codec_q, (size_t)st->rows_q * st->d_embed * 4)); TRY(pproj.put(st->pproj_q, (size_t)st->rows_q * st->d_proj * 4));
        TRY(bias.put(st->proj_b, (size_t)st->d_proj * 4)); TRY(fb.put(st->fb, B * st->d_embed * 4)); TRY(px.put(st->px, B * st->d_proj * 4));
        return codes.put(st->codes, B * st->max_steps_cap * st->n_codebooks * 4);
    }
    int read(q3tts_k_pred_step* st) const {
        const size_t B = st->n_rows;
        TRY(fb.get(st->fb, B * st->d_embed * 4)); TRY(px.get(st->px, B * st->d_proj * 4));
        return codes.get(st->codes, B * st->max_steps_cap * st->n_codebooks * 4);
    }
};

extern "C" int q3tts_k_pred_next(int32_t device, q3tts_k_pred_step* st, const float* norm_w, uint16_t* xb, float* ssp) {
    if (const char* why = PredStepHook::check(st)) return q3_set_err(nullptr, Q3TTS_ERR_INVALID, std::string("pred next hook: ") + why);
    if (!norm_w || !xb || !ssp) return q3_set_err(nullptr, Q3TTS_ERR_INVALID, "pred next hook: a null argument");
    HK(hipSetDevice(device));
    PredStepHook h;
    TRY(h.init(st));
    const int B = st->n_rows, dp = st->d_proj;
    DevBuf dnw, dxb, dssp;
    TRY(dnw.put(norm_w, (size_t)dp * 4)); TRY(dxb.alloc(pad16(B) * dp * 2)); TRY(dssp.alloc((size_t)B * (dp / 16) * 4));
    Q3PredNext pn{}; pn.keys = h.keys; pn.n_key_parts = st->n_key_parts; pn.q = st->q; pn.ncb = st->n_codebooks; pn.codec_q = h.codec; pn.rows_q = st->rows_q;
    pn.d = st->d_embed; pn.slots = h.slots; pn.row_slot = h.row_slot; pn.B = B; pn.codes = h.codes; pn.max_steps_cap = st->max_steps_cap; pn.fb = h.fb;
    pn.pproj_q = h.pproj; pn.proj_b = h.bias; pn.dp = dp; pn.px = h.px; pn.nw = dnw; pn.xb = dxb; pn.ssp = dssp;
    if (q3_launch_pred_next(pn, nullptr, false)) return q3_set_err(nullptr, Q3TTS_ERR_INVALID, "pred next hook: the launch was refused");
    HK(hipGetLastError()); HK(hipDeviceSynchronize());
    TRY(h.read(st)); TRY(untile_host(dxb, B, dp, xb));
    return dssp.get(ssp, (size_t)B * (dp / 16) * 4);
}

// One gathering attention launch as block 0 of pass st->q issues it: row b (= slot b, position len - 1, the Predictor's row-indexed cache) takes its
// q / k / v from table[code of keys[b]] ([rows_q + 1][ld]; row rows_q = the fallback) and the extra workgroup column does st's bookkeeping.
// qkv: n_rows runs of len rows as q3tts_k_attention_decode_ex takes them — the first len - 1 fill the slot's cache, the last one is NOT read.
extern "C" int q3tts_k_attention_gather(int32_t device, q3tts_k_pred_step* st, const float* table, const float* qkv, int32_t len, int32_t n_ctx, int32_t Hq,
                                        int32_t Hkv, int32_t hd, const float* qnw, const float* knw, float eps, float theta, const int32_t* sections,
                                        int32_t out_form, void* out, float* out_scale, uint16_t* k_cache, uint16_t* v_cache) {
    if (const char* why = PredStepHook::check(st)) return q3_set_err(nullptr, Q3TTS_ERR_INVALID, std::string("attention gather hook: ") + why);
    const int n_slots = st->n_rows;
    if (const char* why = AttHook::check(qkv, n_slots, n_ctx, Hq, Hkv, hd, qnw, knw, out_form, out, out_scale))
        return q3_set_err(nullptr, Q3TTS_ERR_INVALID, std::string("attention gather hook: ") + why);
    if (!table || len < 1 || len > n_ctx) return q3_set_err(nullptr, Q3TTS_ERR_INVALID, "attention gather hook: table, 1 <= len <= n_ctx");
    HK(hipSetDevice(device));
    AttHook h;
    TRY(h.init(n_slots, n_ctx, Hq, Hkv, qnw, knw, theta, sections, out_form, n_slots));
    PredStepHook ps;
    TRY(ps.init(st));
    const int ld = h.ld, npre = n_slots * (len - 1);
    std::vector<float> pre((size_t)std::max(npre, 1) * ld);
    std::vector<int> pp, psl;
    for (int s = 0, ip = 0; s < n_slots; ++s)
        for (int r = 0; r < len - 1; ++r, ++ip) { memcpy(&pre[(size_t)ip * ld], qkv + ((size_t)s * len + r) * ld, (size_t)ld * 4); pp.push_back(r); psl.push_back(s); }
    DevBuf dpre, dpp, dps, dtab;
    TRY(dpre.put(pre.data(), pre.size() * 4)); TRY(dpp.put(pp.data(), pp.size() * 4)); TRY(dps.put(psl.data(), psl.size() * 4));
    TRY(dtab.put(table, (size_t)(st->rows_q + 1) * ld * 4));
    if (npre) {
        Q3QkPrep qp = h.prep(dpre, npre, eps); qp.row_pos = dpp; qp.row_slot = dps;
        if (q3_launch_qk_prep(qp, nullptr)) return q3_set_err(nullptr, Q3TTS_ERR_INVALID, "attention gather hook: the q/k prep launch was refused");
    }
    Q3QkPrep dq = h.prep(nullptr, n_slots, eps);   // (no row buffer: the gathering form reads the table)
    Q3Attend at = h.attend(nullptr, n_slots);
    dq.slot_mod = at.slot_mod = n_slots; dq.pos_const = at.pos_const = len - 1;
    at.fused = 1; at.prep = dq;
    Q3AttGather gt{}; gt.tab = dtab; gt.tab_rows = st->rows_q; gt.keys = ps.keys; gt.n_key_parts = st->n_key_parts; gt.q = st->q; gt.ncb = st->n_codebooks;
    gt.codec_q = ps.codec; gt.d = st->d_embed; gt.slots = ps.slots; gt.row_slot = ps.row_slot; gt.codes = ps.codes; gt.max_steps_cap = st->max_steps_cap;
    gt.fb = ps.fb; gt.pproj_q = ps.pproj; gt.proj_b = ps.bias; gt.dp = st->d_proj; gt.px = ps.px;
    if (q3_launch_attend_gather(at, gt, nullptr)) return q3_set_err(nullptr, Q3TTS_ERR_INVALID, "attention gather hook: the launch was refused (two query heads per KV head, n_ctx 64)");
    hipError_t er = hipGetLastError();
    if (er == hipSuccess) er = hipDeviceSynchronize();
    if (er != hipSuccess) return q3_set_err(nullptr, Q3TTS_ERR_DEVICE, std::string("attention gather hook: ") + hipGetErrorString(er));
    TRY(h.read_out(out, out_scale)); TRY(h.read_cache(k_cache, v_cache));
    return ps.read(st);
}

extern "C" int q3tts_k_sample(int32_t device, const float* logits, int32_t n, int32_t ld, int32_t limit, float temperature, int32_t top_k,
                              float top_p, const float* r, int32_t* out) {
    if (!logits || !out || n <= 0 || limit <= 0 || limit > 4096 || limit > ld) return q3_set_err(nullptr, Q3TTS_ERR_INVALID, "sample hook: bad shape");
    HK(hipSetDevice(device));
    DevBuf dl, dr, dout;
    TRY(dl.put(logits, (size_t)n * ld * 4)); TRY(dr.put(r, (size_t)n * 4)); TRY(dout.alloc((size_t)n * 4));
    q3_launch_sample_rows(dl, n, ld, limit, temperature, top_k, top_p, r ? (const float*)dr.p : nullptr, dout, nullptr);
    HK(hipDeviceSynchronize());
    return dout.get(out, (size_t)n * 4);
}

// The decoder's GEMM on bf16 rows through its launcher (q3_bgemm.hip), behind q3tts_k_bgemm (w: bf16 bits row-major [N][K]) and
// q3tts_k_bgemm_q8 (q8: w holds block_q8_0 rows). The entry points have checked the arguments.
static int bgemm_hook(const char* name, int device, const uint16_t* xb, int B, int K, const void* w, bool q8, int N, const float* ssp, int ntiles, int d_norm,
                      float eps, int epi, const float* nw_next, float* y, uint16_t* yb, float* ssp_out, uint64_t* keys, int iters, float* mean_ms) {
    HK(hipSetDevice(device));
    const int F = N / 2, nt = N / 16;
    DevBuf dx, dw, dwt, dsc, ds, dn, dy, dyb, dso, dk;
    { const std::vector<uint16_t> xt = atile_host(xb, B, K); TRY(dx.put(xt.data(), xt.size() * 2)); }
    TRY(dw.put(w, q8 ? (size_t)N * (K / 32) * 34 : (size_t)N * K * 2)); TRY(dwt.alloc(q8 ? (size_t)N * K : (size_t)N * K * 2));
    if (q8) TRY(dsc.alloc((size_t)N * (K / 32) * 2));
    TRY(ds.put(ntiles > 0 ? ssp : nullptr, (size_t)B * std::max(ntiles, 1) * 4)); TRY(dn.put(nw_next, (size_t)N * 4));
    TRY(dy.put(epi == Q3_EPI_RESID ? y : nullptr, (size_t)B * N * 4)); TRY(dyb.alloc(pad16(B) * N * 2)); TRY(dso.alloc((size_t)B * nt * 4)); TRY(dk.alloc((size_t)B * nt * 8));
    tile_weight(dw, dwt, q8 ? &dsc : nullptr, N, K, epi == Q3_EPI_SWIGLU);
    Q3BGemm g{}; g.a = dx; g.a_row0 = 0; g.B = B; g.w = dwt; g.K = K; g.N = N;
    if (q8) g.wscale = dsc;
    if (ssp) g.ssp = ds;
    g.ld_ssp = ntiles; g.ntiles = ntiles; g.d_norm = d_norm; g.eps = eps; g.epi = epi;
    g.y = dy; g.ldy = N; g.yb = dyb;
    if (nw_next) g.nw_next = dn;
    g.ssp_out = dso; g.ld_ssp_out = nt; g.keys = dk; g.key_stride = nt;
    if (q3_launch_bgemm(g, nullptr)) return q3_set_err(nullptr, Q3TTS_ERR_INVALID, std::string(name) + ": shape");
    HK(hipDeviceSynchronize());
    if (epi == Q3_EPI_STORE || epi == Q3_EPI_RESID) TRY(dy.get(y, (size_t)B * N * 4));
    if (epi == Q3_EPI_SWIGLU) TRY(untile_host(dyb, B, F, yb));
    if (epi == Q3_EPI_RESID && nw_next) { TRY(untile_host(dyb, B, N, yb)); TRY(dso.get(ssp_out, (size_t)B * nt * 4)); }
    if (epi == Q3_EPI_ARGMAX) {  // the kernel leaves one maximum per (row, 16-column tile); the consumer (here: the hook) takes the row maximum
        std::vector<uint64_t> parts((size_t)B * nt);
        TRY(dk.get(parts.data(), parts.size() * 8));
        for (int b = 0; b < B; ++b) { uint64_t m = 0; for (int t = 0; t < nt; ++t) m = std::max(m, parts[(size_t)b * nt + t]); keys[b] = m; }
    }
    if (epi == Q3_EPI_RESID) { g.epi = Q3_EPI_STORE; g.nw_next = nullptr; }
    return time_launches(iters, [&] { q3_launch_bgemm(g, nullptr); }, mean_ms);
}

// xb bf16 bits [B][K]; w bf16 bits row-major [N][K] (epi 2: the F gate rows, then the F up rows); ssp [B][ntiles] or NULL; y in/out for
// epi 1. Mirrors oracle/q3_oracle_bf16.c q3o_bgemm.
extern "C" int q3tts_k_bgemm(int32_t device, const uint16_t* xb, int32_t B, int32_t K, const uint16_t* w, int32_t N, const float* ssp, int32_t ntiles,
                             int32_t d_norm, float eps, int32_t epi, const float* nw_next, float* y, uint16_t* yb, float* ssp_out, uint64_t* keys,
                             int32_t iters, float* mean_ms) {
    if (!xb || !w || B <= 0 || K % 256 || K < 256 || N % 16 || epi < 0 || epi > 3) return q3_set_err(nullptr, Q3TTS_ERR_INVALID, "bgemm hook: K % 256 == 0, N % 16 == 0");
    if (epi == Q3_EPI_SWIGLU && (N % 64 || !yb)) return q3_set_err(nullptr, Q3TTS_ERR_INVALID, "bgemm hook: swiglu needs N % 64 == 0 and yb");
    if (epi == Q3_EPI_RESID && nw_next && N % 32) return q3_set_err(nullptr, Q3TTS_ERR_INVALID, "bgemm hook: norm outputs need N % 32 == 0");
    if ((epi == Q3_EPI_STORE || epi == Q3_EPI_RESID) && !y) return q3_set_err(nullptr, Q3TTS_ERR_INVALID, "bgemm hook: y missing");
    if (epi == Q3_EPI_ARGMAX && !keys) return q3_set_err(nullptr, Q3TTS_ERR_INVALID, "bgemm hook: keys missing");
    if (epi == Q3_EPI_RESID && nw_next && (!yb || !ssp_out)) return q3_set_err(nullptr, Q3TTS_ERR_INVALID, "bgemm hook: norm outputs missing");
    return bgemm_hook("bgemm", device, xb, B, K, w, false, N, ssp, ntiles, d_norm, eps, epi, nw_next, y, yb, ssp_out, keys, iters, mean_ms);
}

// the same launch with ggml Q8_0 weights kept in block form: q int8 [N][K], d_f16 [N][K/32]. Mirrors oracle q3o_bgemm_q8.
extern "C" int q3tts_k_bgemm_q8(int32_t device, const uint16_t* xb, int32_t B, int32_t K, const int8_t* q, const uint16_t* d_f16, int32_t N, const float* ssp,
                                int32_t ntiles, int32_t d_norm, float eps, int32_t epi, const float* nw_next, float* y, uint16_t* yb, float* ssp_out,
                                uint64_t* keys, int32_t iters, float* mean_ms) {
    if (!xb || !q || !d_f16 || B <= 0 || K % 512 || K < 512 || N % 16 || epi < 0 || epi > 3) return q3_set_err(nullptr, Q3TTS_ERR_INVALID, "bgemm_q8 hook: K % 512 == 0, N % 16 == 0");
    if (epi == Q3_EPI_SWIGLU && (N % 64 || !yb)) return q3_set_err(nullptr, Q3TTS_ERR_INVALID, "bgemm_q8 hook: swiglu needs N % 64 == 0 and yb");
    if (epi == Q3_EPI_RESID && nw_next && (N % 32 || !yb || !ssp_out)) return q3_set_err(nullptr, Q3TTS_ERR_INVALID, "bgemm_q8 hook: norm outputs");
    if ((epi == Q3_EPI_STORE || epi == Q3_EPI_RESID) && !y) return q3_set_err(nullptr, Q3TTS_ERR_INVALID, "bgemm_q8 hook: y missing");
    if (epi == Q3_EPI_ARGMAX && !keys) return q3_set_err(nullptr, Q3TTS_ERR_INVALID, "bgemm_q8 hook: keys missing");
    const std::vector<uint8_t> blocks = pack_q8_0(q, d_f16, N, K);
    return bgemm_hook("bgemm_q8", device, xb, B, K, blocks.data(), true, N, ssp, ntiles, d_norm, eps, epi, nw_next, y, yb, ssp_out, keys, iters, mean_ms);
}

// W8A8 (q3_bgemm8.hip): activations and weights as ggml Q8_0 blocks in natural order in / out; the hook tiles them for the device
extern "C" int q3tts_k_bgemm_q8a8(int32_t device, const int8_t* aq, const float* ad, int32_t B, int32_t K, const int8_t* q, const uint16_t* d_f16, int32_t N,
                                  const float* ssp, int32_t ntiles, int32_t d_norm, float eps, int32_t epi, const float* nw_next, float* y, int8_t* yq, float* yd,
                                  float* ssp_out, int32_t iters, float* mean_ms) {
    if (!aq || !ad || !q || !d_f16 || B <= 0 || K % 512 || K < 512 || N % 32 || epi < 0 || epi > 2) return q3_set_err(nullptr, Q3TTS_ERR_INVALID, "bgemm_q8a8 hook: K % 512 == 0, N % 32 == 0, epilogue 0..2");
    if (epi == Q3_EPI_SWIGLU && (N % 128 || !yq || !yd)) return q3_set_err(nullptr, Q3TTS_ERR_INVALID, "bgemm_q8a8 hook: swiglu needs N % 128 == 0, yq, yd");
    if (epi == Q3_EPI_RESID && (N % 64 || !nw_next || !yq || !yd || !ssp_out || !y)) return q3_set_err(nullptr, Q3TTS_ERR_INVALID, "bgemm_q8a8 hook: residual needs N % 64 == 0, nw_next, y, yq, yd, ssp_out");
    if (epi == Q3_EPI_STORE && !y) return q3_set_err(nullptr, Q3TTS_ERR_INVALID, "bgemm_q8a8 hook: y missing");
    HK(hipSetDevice(device));
    const int F = N / 2, kb = K / 32, Nout = epi == Q3_EPI_SWIGLU ? F : N;
    const size_t B16 = pad16(B); const int rt16 = (int)(B16 / 16);
    const std::vector<uint8_t> blocks = pack_q8_0(q, d_f16, N, K);
    std::vector<int8_t> at(B16 * K, 0); std::vector<float> ast((size_t)kb * B16, 0.0f);
    for (int r = 0; r < B; ++r) {
        for (int k = 0; k < K; ++k) at[q3_q8_off(r, k, K >> 6)] = aq[(size_t)r * K + k];
        for (int b = 0; b < kb; ++b) ast[q3_q8_scale_idx(r, b, rt16)] = ad[(size_t)r * kb + b];
    }
    DevBuf dx, dxs, dw, dwt, dsc, ds, dn, dy, dyq, dys, dso;
    TRY(dx.put(at.data(), at.size())); TRY(dxs.put(ast.data(), ast.size() * 4)); TRY(dw.put(blocks.data(), blocks.size())); TRY(dwt.alloc((size_t)N * K));
    TRY(dsc.alloc((size_t)N * kb * 2)); TRY(ds.put(ntiles > 0 ? ssp : nullptr, (size_t)B * std::max(ntiles, 1) * 4)); TRY(dn.put(nw_next, (size_t)N * 4));
    TRY(dy.put(epi == Q3_EPI_RESID ? y : nullptr, (size_t)B * N * 4)); TRY(dyq.alloc(B16 * Nout)); TRY(dys.alloc((size_t)(Nout / 32 + 2) * B16 * 4));
    TRY(dso.alloc((size_t)B * (N / 16) * 4));
    tile_weight(dw, dwt, &dsc, N, K, epi == Q3_EPI_SWIGLU);
    Q3BGemm g{}; g.a = dx; g.ascale = dxs; g.a_rt16 = rt16; g.a_row0 = 0; g.B = B; g.w = dwt; g.wscale = dsc; g.K = K; g.N = N;
    if (ssp) g.ssp = ds;
    g.ld_ssp = ntiles; g.ntiles = ntiles; g.d_norm = d_norm; g.eps = eps; g.epi = epi;
    g.y = dy; g.ldy = N; g.yb = dyq; g.yscale = dys; g.y_rt16 = rt16;
    if (nw_next) g.nw_next = dn;
    g.ssp_out = dso; g.ld_ssp_out = N / 16;
    if (q3_launch_bgemm8(g, nullptr)) return q3_set_err(nullptr, Q3TTS_ERR_INVALID, "bgemm_q8a8: shape");
    HK(hipDeviceSynchronize());
    if (epi == Q3_EPI_STORE || epi == Q3_EPI_RESID) TRY(dy.get(y, (size_t)B * N * 4));
    if (epi != Q3_EPI_STORE) {
        std::vector<int8_t> qt(B16 * Nout); std::vector<float> st((size_t)(Nout / 32) * B16);
        TRY(dyq.get(qt.data(), qt.size())); TRY(dys.get(st.data(), st.size() * 4));
        for (int r = 0; r < B; ++r) {
            for (int k = 0; k < Nout; ++k) yq[(size_t)r * Nout + k] = qt[q3_q8_off(r, k, Nout >> 6)];
            for (int b = 0; b < Nout / 32; ++b) yd[(size_t)r * (Nout / 32) + b] = st[q3_q8_scale_idx(r, b, rt16)];
        }
        if (epi == Q3_EPI_RESID) TRY(dso.get(ssp_out, (size_t)B * (N / 16) * 4));
    }
    if (epi == Q3_EPI_RESID) g.epi = Q3_EPI_STORE;
    return time_launches(iters, [&] { q3_launch_bgemm8(g, nullptr); }, mean_ms);
}

// The same launch with the ARGMAX epilogue (the heads of a W8A8 Predictor: predictor_q8_0 = 2): one launch through q3_launch_bgemm8, then the
// reduction k_pred_next applies to the per-tile keys it leaves — the largest key of the row, first maximum wins — and the winning column per row
extern "C" int q3tts_k_bgemm_q8a8_argmax(int32_t device, const int8_t* aq, const float* ad, int32_t B, int32_t K, const int8_t* q, const uint16_t* d_f16, int32_t N,
                                         const float* ssp, int32_t ntiles, int32_t d_norm, float eps, int32_t* ids_out) {
    if (!aq || !ad || !q || !d_f16 || !ids_out || B <= 0 || K % 512 || K < 512 || N % 32 || N < 32 || (ssp && ntiles < 1))
        return q3_set_err(nullptr, Q3TTS_ERR_INVALID, "bgemm_q8a8_argmax hook: K % 512 == 0, N % 32 == 0, ids_out");
    HK(hipSetDevice(device));
    const int kb = K / 32, nt = N / 16;
    const size_t B16 = pad16(B); const int rt16 = (int)(B16 / 16);
    const std::vector<uint8_t> blocks = pack_q8_0(q, d_f16, N, K);
    std::vector<int8_t> at(B16 * K, 0); std::vector<float> ast((size_t)kb * B16, 0.0f);
    for (int r = 0; r < B; ++r) {
        for (int k = 0; k < K; ++k) at[q3_q8_off(r, k, K >> 6)] = aq[(size_t)r * K + k];
        for (int b = 0; b < kb; ++b) ast[q3_q8_scale_idx(r, b, rt16)] = ad[(size_t)r * kb + b];
    }
    DevBuf dx, dxs, dw, dwt, dsc, ds, dk;
    TRY(dx.put(at.data(), at.size())); TRY(dxs.put(ast.data(), ast.size() * 4)); TRY(dw.put(blocks.data(), blocks.size())); TRY(dwt.alloc((size_t)N * K));
    TRY(dsc.alloc((size_t)N * kb * 2)); TRY(ds.put(ssp, (size_t)B * std::max(ntiles, 1) * 4)); TRY(dk.alloc((size_t)B * nt * 8));
    tile_weight(dw, dwt, &dsc, N, K, false);
    Q3BGemm g{}; g.a = dx; g.ascale = dxs; g.a_rt16 = rt16; g.a_row0 = 0; g.B = B; g.w = dwt; g.wscale = dsc; g.K = K; g.N = N;
    if (ssp) g.ssp = ds;
    g.ld_ssp = ntiles; g.ntiles = ntiles; g.d_norm = d_norm; g.eps = eps; g.epi = Q3_EPI_ARGMAX; g.keys = dk; g.key_stride = nt;
    if (q3_launch_bgemm8(g, nullptr)) return q3_set_err(nullptr, Q3TTS_ERR_INVALID, "bgemm_q8a8_argmax: shape");
    HK(hipDeviceSynchronize());
    std::vector<uint64_t> parts((size_t)B * nt);
    TRY(dk.get(parts.data(), parts.size() * 8));
    for (int b = 0; b < B; ++b) { uint64_t m = 0; for (int t = 0; t < nt; ++t) m = std::max(m, parts[(size_t)b * nt + t]); ids_out[b] = q3_argmax_idx(m); }
    return Q3TTS_OK;
}

// The vocoder's extras of the decoder GEMM (bias, GELU -> bf16, LayerScale column scale, per-slot row segments, a bf16 copy of the
// residual result) through one hook: epi 0 (store) / 1 (residual) / 4 (GELU). y0 / y are dense [B][N]; with seg_rows > 0 the kernel
// works on a buffer of B / seg_rows segments, each preceded by gap_rows sentinel rows that must come back untouched.
extern "C" int q3tts_k_bgemm_voc(int32_t device, const uint16_t* xb, int32_t B, int32_t K, const uint16_t* w, int32_t N, int32_t epi, const float* bias,
                                 int32_t bias_n, const float* col_scale, int32_t seg_rows, int32_t gap_rows, float* y, uint16_t* yb, int32_t want_yb) {
    if (!xb || !w || B <= 0 || K % 256 || K < 256 || N % 32 || (epi != Q3_EPI_STORE && epi != Q3_EPI_RESID && epi != Q3_EPI_GELU))
        return q3_set_err(nullptr, Q3TTS_ERR_INVALID, "bgemm_voc hook: K % 256 == 0, N % 32 == 0, epilogue 0 / 1 / 4");
    if ((epi != Q3_EPI_GELU && !y) || ((epi == Q3_EPI_GELU || want_yb) && !yb)) return q3_set_err(nullptr, Q3TTS_ERR_INVALID, "bgemm_voc hook: output missing");
    if (seg_rows < 0 || gap_rows < 0 || (seg_rows > 0 && B % seg_rows) || (bias && bias_n < 1)) return q3_set_err(nullptr, Q3TTS_ERR_INVALID, "bgemm_voc hook: segments / bias");
    HK(hipSetDevice(device));
    const int T = seg_rows > 0 ? seg_rows : B, S = B / T, P = T + (seg_rows > 0 ? gap_rows : 0);
    std::vector<float> seg((size_t)S * P * N, -12345.5f);  // sentinel in the gap rows
    if (epi != Q3_EPI_GELU)
        for (int sidx = 0; sidx < S; ++sidx)
            for (int t = 0; t < T; ++t) memcpy(&seg[((size_t)sidx * P + (P - T) + t) * N], y + ((size_t)sidx * T + t) * N, (size_t)N * 4);
    DevBuf dx, dw, dwt, db, dc, dy, dyb;
    { const std::vector<uint16_t> xt = atile_host(xb, B, K); TRY(dx.put(xt.data(), xt.size() * 2)); }
    TRY(dw.put(w, (size_t)N * K * 2)); TRY(dwt.alloc((size_t)N * K * 2)); TRY(db.put(bias, (size_t)(bias ? bias_n : 1) * 4)); TRY(dc.put(col_scale, (size_t)N * 4));
    TRY(dy.put(seg.data(), seg.size() * 4)); TRY(dyb.alloc(pad16(B) * N * 2));
    tile_weight(dw, dwt, nullptr, N, K, false);
    Q3BGemm g{}; g.a = dx; g.B = B; g.w = dwt; g.K = K; g.N = N; g.epi = epi;
    g.y = (float*)dy.p + (size_t)(P - T) * N; g.ldy = N;
    if (seg_rows > 0) { g.seg_rows = T; g.seg_stride = (size_t)P * N; }
    if (bias) g.bias = db;
    g.bias_n = bias_n;
    if (col_scale) g.col_scale = dc;
    if (epi == Q3_EPI_GELU || want_yb) g.yb = dyb;
    if (q3_launch_bgemm(g, nullptr)) return q3_set_err(nullptr, Q3TTS_ERR_INVALID, "bgemm_voc: shape");
    HK(hipDeviceSynchronize());
    if (epi != Q3_EPI_GELU) {
        TRY(dy.get(seg.data(), seg.size() * 4));
        for (int sidx = 0; sidx < S; ++sidx) {
            for (int t = 0; t < P - T; ++t)
                for (int c = 0; c < N; ++c)
                    if (seg[((size_t)sidx * P + t) * N + c] != -12345.5f) return q3_set_err(nullptr, Q3TTS_ERR_DEVICE, "bgemm_voc: a gap row was written");
            for (int t = 0; t < T; ++t) memcpy(y + ((size_t)sidx * T + t) * N, &seg[((size_t)sidx * P + (P - T) + t) * N], (size_t)N * 4);
        }
    }
    return (epi == Q3_EPI_GELU || want_yb) ? untile_host(dyb, B, N, yb) : Q3TTS_OK;
}

// H6 through the projection kernel: y[rows][n_out] = bias + sum x * w (reference order); nw != NULL: the rows' norm inputs too
extern "C" int q3tts_k_project(int32_t device, const float* x, int32_t rows, int32_t n_in, const float* w, const float* bias, int32_t n_out, const float* nw,
                               float* y, uint16_t* xb, float* ssp) {
    if (!x || !w || !bias || !y || rows <= 0 || n_in % 64 || n_out % 16 || (nw && (!xb || !ssp))) return q3_set_err(nullptr, Q3TTS_ERR_INVALID, "project hook: n_in % 64 == 0, n_out % 16 == 0");
    HK(hipSetDevice(device));
    DevBuf dx, dw, db, dn, dy, dxb, dss;
    TRY(dx.put(x, (size_t)rows * n_in * 4)); TRY(dw.put(w, (size_t)n_out * n_in * 4)); TRY(db.put(bias, (size_t)n_out * 4)); TRY(dn.put(nw, (size_t)n_out * 4));
    TRY(dy.alloc((size_t)rows * n_out * 4)); TRY(dxb.alloc(pad16(rows) * n_out * 2)); TRY(dss.alloc((size_t)rows * (n_out / 16) * 4));
    Q3Project pj{}; pj.x = dx; pj.ldx = n_in; pj.rows = rows; pj.w = dw; pj.bias = db; pj.n_in = n_in; pj.n_out = n_out;
    pj.y = dy; pj.ldy = n_out; pj.xb = dxb; pj.ssp = dss; pj.ld_ssp = n_out / 16;
    if (nw) pj.nw = dn;
    if (q3_launch_project(pj, nullptr)) return q3_set_err(nullptr, Q3TTS_ERR_INVALID, "project: shape");
    HK(hipDeviceSynchronize());
    TRY(dy.get(y, (size_t)rows * n_out * 4));
    if (nw) {
        if (n_out % 32) return q3_set_err(nullptr, Q3TTS_ERR_INVALID, "project hook: norm outputs need n_out % 32 == 0");
        TRY(untile_host(dxb, rows, n_out, xb));
        TRY(dss.get(ssp, (size_t)rows * (n_out / 16) * 4));
    }
    return Q3TTS_OK;
}

// producer side of the split RMSNorm for plain f32 rows (d % 256 == 0)
extern "C" int q3tts_k_norm_inputs(int32_t device, const float* x, int32_t rows, int32_t d, const float* nw, uint16_t* xb, float* ssp) {
    if (!x || !nw || !xb || !ssp || rows <= 0 || d % 256) return q3_set_err(nullptr, Q3TTS_ERR_INVALID, "norm-inputs hook: d % 256 == 0");
    HK(hipSetDevice(device));
    DevBuf dx, dn, dxb, dss;
    TRY(dx.put(x, (size_t)rows * d * 4)); TRY(dn.put(nw, (size_t)d * 4)); TRY(dxb.alloc(pad16(rows) * d * 2)); TRY(dss.alloc((size_t)rows * (d / 16) * 4));
    q3_launch_norm_inputs(dx, d, rows, d, dn, dxb, 0, dss, d / 16, nullptr);
    HK(hipDeviceSynchronize());
    TRY(untile_host(dxb, rows, d, xb));
    return dss.get(ssp, (size_t)rows * (d / 16) * 4);
}

// one v_mfma_f32_16x16x32_bf16 chain per case (test hook: pins the instruction's accumulation arithmetic against the
// oracle's integer restatement, oracle/q3_oracle.c q3o_mfma_bf16_dot32)
typedef float q3_f32x4 __attribute__((ext_vector_type(4)));
typedef __bf16 q3_bf16x8 __attribute__((ext_vector_type(8)));
__global__ void k_mfma_bf16_cases(const uint16_t* A, const uint16_t* B, const float* C, float* D, int chain) {
    const int l = threadIdx.x, cs = blockIdx.x;
    const uint16_t* a = A + (size_t)cs * chain * 512; const uint16_t* b = B + (size_t)cs * chain * 512;
    q3_f32x4 acc;
    for (int j = 0; j < 4; ++j) acc[j] = C[(size_t)cs * 256 + (4 * (l >> 4) + j) * 16 + (l & 15)];
    for (int st = 0; st < chain; ++st) {
        union { q3_bf16x8 v; uint16_t u[8]; } af, bf;
        for (int j = 0; j < 8; ++j) {  // lane l holds A[row l & 15][k = 8 (l >> 4) + j] and B[k = 8 (l >> 4) + j][col l & 15]
            af.u[j] = a[(size_t)st * 512 + (l & 15) * 32 + 8 * (l >> 4) + j];
            bf.u[j] = b[(size_t)st * 512 + (8 * (l >> 4) + j) * 16 + (l & 15)];
        }
        acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af.v, bf.v, acc, 0, 0, 0);
    }
    for (int j = 0; j < 4; ++j) D[(size_t)cs * 256 + (4 * (l >> 4) + j) * 16 + (l & 15)] = acc[j];
}
extern "C" int q3tts_k_mfma_bf16(int32_t device, const uint16_t* a, const uint16_t* b, const float* c, float* d, int32_t n_cases, int32_t chain) {
    if (!a || !b || !c || !d || n_cases <= 0 || chain <= 0) return q3_set_err(nullptr, Q3TTS_ERR_INVALID, "mfma hook: bad shape");
    HK(hipSetDevice(device));
    const size_t nab = (size_t)n_cases * chain * 512 * 2, ncd = (size_t)n_cases * 256 * 4;
    DevBuf da, db, dc, dd;
    TRY(da.put(a, nab)); TRY(db.put(b, nab)); TRY(dc.put(c, ncd)); TRY(dd.alloc(ncd));
    hipLaunchKernelGGL(k_mfma_bf16_cases, dim3(n_cases), dim3(64), 0, nullptr, (const uint16_t*)da.p, (const uint16_t*)db.p, (const float*)dc.p, (float*)dd.p, chain);
    HK(hipDeviceSynchronize());
    return dd.get(d, ncd);
}

// Talker prefill of one prompt (behind a voice prefix, if given) through the engine's own admission into slot 0; the slot is retired again
static int talker_prefill(q3tts_engine* e, const q3tts_prefix* prefix, const float* embd, int32_t n_tok, float* hidden_out, float* logits_out) {
    Q3_NOT_IN_SESSION(e);
    if (!e || !embd || n_tok <= 0) return q3_set_err(e, Q3TTS_ERR_INVALID, "null argument");
    Q3_HIP(e, hipSetDevice(e->cfg.device));
    q3tts_request r{}; r.prompt_embd = embd; r.n_tok = n_tok; r.use_engine_sampler = 0; r.temperature = 0; r.max_steps = 1; r.prefix = prefix;
    const q3tts_request* rp = &r;
    const int slot = 0;
    int rc = Q3TTS_OK;
    TRY(q3_plan_rows(e, std::vector<int>{slot}));
    TRY(q3_admit_many(e, &slot, &rp, 1, &rc));
    TRY(rc);
    const q3tts_model_config& m = e->cfg.model;
    const Q3Lane& L = e->lane;
    hipStream_t s = e->stream;
    if (hidden_out) {
        q3_launch_rmsnorm_rows(L.T.x, m.t_d_model, e->T.out_norm, m.rms_eps, m.t_d_model, 1, L.logits_tmp, m.t_d_model, s);
        Q3_HIP(e, hipMemcpyAsync(hidden_out, L.logits_tmp, (size_t)m.t_d_model * 4, hipMemcpyDeviceToHost, s));
    }
    if (logits_out) Q3_HIP(e, hipMemcpyAsync(logits_out, L.logits, (size_t)m.t_vocab * 4, hipMemcpyDeviceToHost, s));
    TRY(q3_retire_slot(e, slot, s));  // retire the slot again
    Q3_HIP(e, hipStreamSynchronize(s));
    return Q3TTS_OK;
}
extern "C" int q3tts_k_talker_prefill(q3tts_engine* e, const float* embd, int32_t n_tok, float* hidden_out, float* logits_out) {
    return talker_prefill(e, nullptr, embd, n_tok, hidden_out, logits_out);
}
extern "C" int q3tts_k_talker_prefill_prefix(q3tts_engine* e, const q3tts_prefix* prefix, const float* embd, int32_t n_tok, float* hidden_out,
                                             float* logits_out) {
    if (!prefix) return q3_set_err(e, Q3TTS_ERR_INVALID, "null prefix");
    return talker_prefill(e, prefix, embd, n_tok, hidden_out, logits_out);
}
// q3_request_rules (q3_admit.hip) with its message copied into msg[cap] (host only)
extern "C" int q3tts_k_request_rules(const q3tts_request* r, int32_t keep, int32_t keep_rows, char* msg, int32_t cap) {
    const char* why = "";
    const int st = q3_request_rules(r, keep != 0, keep_rows, &why);
    if (msg && cap > 0) { strncpy(msg, why, (size_t)cap - 1); msg[cap - 1] = 0; }
    return st;
}

// a ready prefix's two stores as bytes, padding included (*bytes: the size of each; k / v may be null to ask for it)
extern "C" int q3tts_k_prefix_read(const q3tts_prefix* x, void* k, void* v, int64_t cap, int64_t* bytes) {
    if (!x || !bytes) return q3_set_err(nullptr, Q3TTS_ERR_INVALID, "null argument");
    q3tts_engine* e = x->e;
    Q3_NOT_IN_SESSION(e);
    if (x->state.load() != 1 || !x->k || !x->v) return q3_set_err(e, Q3TTS_ERR_STATE, "prefix read: the prefix is not ready");
    const size_t n = q3_prefix_store_bytes(e, x->np);
    *bytes = (int64_t)n;
    if (!k && !v) return Q3TTS_OK;
    if (cap < (int64_t)n) return q3_set_err(e, Q3TTS_ERR_INVALID, "prefix read: the buffers hold fewer than *bytes bytes");
    Q3_HIP(e, hipSetDevice(e->cfg.device));
    Q3_HIP(e, hipStreamSynchronize(e->stream));
    if (k) Q3_HIP(e, hipMemcpy(k, x->k, n, hipMemcpyDeviceToHost));
    if (v) Q3_HIP(e, hipMemcpy(v, x->v, n, hipMemcpyDeviceToHost));
    return Q3TTS_OK;
}

extern "C" int q3tts_k_probe(q3tts_engine* e, int32_t enable) {
    Q3_NOT_IN_SESSION(e);
    if (!e) return Q3TTS_ERR_INVALID;
    Q3_HIP(e, hipSetDevice(e->cfg.device));
    if (enable && e->probe_ev.empty()) {
        e->probe_ev.resize(10, nullptr);  // 4 frames x 2 + one empty bracket per chunk (event overhead calibration)
        for (auto& ev : e->probe_ev) Q3_HIP(e, hipEventCreate(&ev));
    }
    const int model = enable & 15, kind = enable >> 4;
    if (model > 2 || kind < 0 || kind > 4) return q3_set_err(e, Q3TTS_ERR_INVALID, "probe: model 0..2, kind 0..4");
    e->probe = model; e->probe_kind = kind;
    return Q3TTS_OK;
}

// The allocator's contract (q3_dev_alloc_zeroed): the zero fill has completed when the pointer is handed out. The hook allocates
// `bytes` through it, uploads a pattern into the first and last 4 KiB on the NULL stream at once (the stream an unsuspecting call
// site would use), and counts the bytes that do not read back as written / as zero. An asynchronous fill on e->stream — the state
// of rounds 1 and 2 — loses this race on large buffers.
extern "C" int q3tts_k_alloc_upload(q3tts_engine* e, int64_t bytes, int64_t* mismatches) {
    Q3_NOT_IN_SESSION(e);
    if (!e || !mismatches || bytes < 16384) return q3_set_err(e, Q3TTS_ERR_INVALID, "alloc hook: bytes >= 16384");
    Q3_HIP(e, hipSetDevice(e->cfg.device));
    void* q = nullptr;
    TRY(q3_dev_alloc_zeroed(e, &q, (size_t)bytes));
    std::vector<uint8_t> pat(4096), back(12288);
    for (int i = 0; i < 4096; ++i) pat[i] = (uint8_t)(1 + i % 251);
    hipError_t er = hipMemcpyAsync(q, pat.data(), 4096, hipMemcpyHostToDevice, nullptr);
    if (er == hipSuccess) er = hipMemcpyAsync((char*)q + bytes - 4096, pat.data(), 4096, hipMemcpyHostToDevice, nullptr);
    if (er == hipSuccess) er = hipDeviceSynchronize();
    if (er == hipSuccess) er = hipMemcpy(back.data(), q, 8192, hipMemcpyDeviceToHost);
    if (er == hipSuccess) er = hipMemcpy(back.data() + 8192, (char*)q + bytes - 4096, 4096, hipMemcpyDeviceToHost);
    hipFree(q);
    if (er != hipSuccess) return q3_set_err(e, Q3TTS_ERR_DEVICE, hipGetErrorString(er));
    int64_t bad = 0;
    for (int i = 0; i < 4096; ++i) bad += (back[i] != pat[i]) + (back[4096 + i] != 0) + (back[8192 + i] != pat[i]);
    *mismatches = bad;
    return Q3TTS_OK;
}

extern "C" int q3tts_k_bgemm_policy(int32_t big) {
    if (big < -1 || big > 1) return q3_set_err(nullptr, Q3TTS_ERR_INVALID, "bgemm policy: -1, 0 or 1");
    q3_bgemm_big_policy(big);
    return Q3TTS_OK;
}

extern "C" int q3tts_k_attend_policy(int32_t decode, int32_t prefill) {
    if (decode < 0 || decode > 1 || prefill < 0 || prefill > 2) return q3_set_err(nullptr, Q3TTS_ERR_INVALID, "attend policy: decode 0..1, prefill 0..2");
    q3_attend_policy(decode, prefill);
    return Q3TTS_OK;
}

extern "C" int q3tts_k_pred_variant(q3tts_engine* e, int32_t force) {
    if (!e) return q3_set_err(nullptr, Q3TTS_ERR_INVALID, "null engine");
    Q3_NOT_IN_SESSION(e);
    if (force < 0 || force > 1) return q3_set_err(e, Q3TTS_ERR_INVALID, "pred variant: 0 or 1");
    return q3_pred_force_variant(e, force);
}

extern "C" int q3tts_k_bgemm_pick(int32_t B, int32_t K, int32_t N, int32_t epilogue, int32_t w_once, int32_t q8, int32_t* out5) {
    if (!out5 || B < 1 || K < 256 || K % 256 || N % 16) return q3_set_err(nullptr, Q3TTS_ERR_INVALID, "bgemm pick: bad shape");
    Q3BGemm g{}; g.B = B; g.K = K; g.N = N; g.epi = epilogue; g.w_once = w_once;
    g.a = (const uint16_t*)16; g.w = (const uint4*)16; g.wscale = q8 ? (const uint16_t*)16 : nullptr;  // (never dereferenced: nothing is launched)
    if (epilogue == Q3_EPI_SWIGLU || epilogue == Q3_EPI_GELU) g.yb = (uint16_t*)16;
    if (epilogue == Q3_EPI_RESID) { g.yb = (uint16_t*)16; g.nw_next = (const float*)16; }
    int rt, nt, d, ntw, big;
    q3_bgemm_pick(g, &rt, &nt, &d, &ntw, &big);
    out5[0] = rt; out5[1] = nt; out5[2] = d; out5[3] = ntw; out5[4] = big;
    return Q3TTS_OK;
}

extern "C" int q3tts_k_pcm_pack(int32_t device, const float* src, int32_t rows, int64_t stride, const int32_t* ent_row, const int32_t* ent_first,
                                const int32_t* ent_count, const int64_t* ent_dst, int32_t n_ent, int32_t format, void* out, int64_t out_n) {
    if (!src || !out || rows <= 0 || stride <= 0 || stride > (1 << 28) || n_ent < 0 || n_ent > Q3_PCM_MAX_ENT || (format != 0 && format != 1) || out_n < 0 ||
        (n_ent > 0 && (!ent_row || !ent_first || !ent_count || !ent_dst)))
        return q3_set_err(nullptr, Q3TTS_ERR_INVALID, "pcm pack hook: bad arguments");
    Q3PcmPack pk{};
    int mx = 0;
    for (int j = 0; j < n_ent; ++j) {
        const long long r = ent_row[j], f = ent_first[j], c = ent_count[j], d = ent_dst[j];
        if (r < 0 || r >= rows || f < 0 || c < 0 || f + c > stride || d < 0 || d + c > out_n)
            return q3_set_err(nullptr, Q3TTS_ERR_INVALID, "pcm pack hook: a window lies outside src or out");
        pk.e[j] = Q3PcmEnt{(int32_t)r, (int32_t)f, (int32_t)c, 0, d};
        mx = std::max(mx, (int)c);
    }
    const size_t es = format ? 2 : 4;
    HK(hipSetDevice(device));
    DevBuf s, o;
    TRY(s.put(src, sizeof(float) * (size_t)rows * stride)); TRY(o.alloc(es * (size_t)std::max<int64_t>(out_n, 1)));
    if (out_n > 0) HK(hipMemcpy(o.p, out, es * (size_t)out_n, hipMemcpyHostToDevice));  // samples outside every window keep their values
    q3_launch_pcm_pack(s, (size_t)stride, pk, n_ent, mx, format, o.p, nullptr);
    HK(hipGetLastError());
    HK(hipDeviceSynchronize());
    return out_n > 0 ? o.get(out, es * (size_t)out_n) : Q3TTS_OK;
}

extern "C" int q3tts_k_resample_table(int32_t rate_in, int32_t rate_out, int32_t* L, int32_t* M, int32_t* H, float* tab, int64_t cap, int64_t* n) {
    if (!L || !M || !H || !n || cap < 0 || (cap > 0 && !tab)) return q3_set_err(nullptr, Q3TTS_ERR_INVALID, "resample table hook: null argument");
    std::vector<float> t;
    int l = 0, m = 0, h = 0;
    const int rc = q3_resample_table(rate_in, rate_out, &l, &m, &h, t);
    if (rc != Q3TTS_OK) return q3_set_err(nullptr, rc, rc == Q3TTS_ERR_UNSUPPORTED ? "resample: this rate pair needs more than 32768 filter coefficients"
                                                                                  : "resample: rates must lie in 4000..96000 Hz and differ");
    *L = l; *M = m; *H = h; *n = (int64_t)t.size();
    if (cap < (int64_t)t.size()) return q3_set_err(nullptr, Q3TTS_ERR_INVALID, "resample table hook: tab holds fewer than L x T values (*n says how many)");
    memcpy(tab, t.data(), sizeof(float) * t.size());
    return Q3TTS_OK;
}

extern "C" int q3tts_k_pcm_resample(int32_t device, const float* src, int32_t rows, int64_t stride, const int32_t* row_len, const int32_t* row_final,
                                    const int32_t* ent_row, const int32_t* ent_first, const int32_t* ent_count, const int64_t* ent_dst, int32_t n_ent,
                                    int32_t rate_in, int32_t rate_out, int32_t format, void* out, int64_t out_n, int32_t iters, float* mean_ms) {
    if (!src || !out || !row_len || !row_final || rows <= 0 || stride <= 0 || stride > (1 << 28) || n_ent < 0 || n_ent > Q3_PCM_MAX_ENT ||
        (format != 0 && format != 1) || out_n < 0 || (n_ent > 0 && (!ent_row || !ent_first || !ent_count || !ent_dst)))
        return q3_set_err(nullptr, Q3TTS_ERR_INVALID, "pcm resample hook: bad arguments");
    Q3Resamp rs{};
    std::vector<float> t;
    const int prc = q3_resample_table(rate_in, rate_out, &rs.L, &rs.M, &rs.H, t);
    if (prc != Q3TTS_OK) return q3_set_err(nullptr, prc, "pcm resample hook: the rate pair is refused");
    rs.rate_in = rate_in; rs.rate_out = rate_out; rs.T = 2 * rs.H + 1;
    for (int r = 0; r < rows; ++r)
        if (row_len[r] < 0 || row_len[r] > stride) return q3_set_err(nullptr, Q3TTS_ERR_INVALID, "pcm resample hook: a row's valid length lies outside its row");
    Q3PcmPack pk{}; Q3PcmSrc ps{};
    int mx = 0;
    for (int j = 0; j < n_ent; ++j) {
        const long long r = ent_row[j], f = ent_first[j], c = ent_count[j], d = ent_dst[j];
        if (r < 0 || r >= rows || f < 0 || c < 0 || d < 0 || d + c > out_n)
            return q3_set_err(nullptr, Q3TTS_ERR_INVALID, "pcm resample hook: a window lies outside src or out");
        const long long lim = row_final[r] ? q3_resample_N(row_len[r], rs.L, rs.M) : q3_resample_D(row_len[r], rs.L, rs.M, rs.H);
        if (f + c > lim) return q3_set_err(nullptr, Q3TTS_ERR_INVALID, "pcm resample hook: a window asks for outputs the row cannot deliver yet (N or D of its length)");
        pk.e[j] = Q3PcmEnt{(int32_t)r, (int32_t)f, (int32_t)c, 0, d};
        ps.len[j] = row_len[r]; if (row_final[r]) ps.final_mask |= 1ull << j;
        mx = std::max(mx, (int)c);
    }
    const size_t es = format ? 2 : 4;
    HK(hipSetDevice(device));
    const std::vector<float> dl = q3_resample_device_layout(t, rs.L, rs.M, rs.T);
    DevBuf s, o, tb;
    TRY(s.put(src, sizeof(float) * (size_t)rows * stride)); TRY(o.alloc(es * (size_t)std::max<int64_t>(out_n, 1)));
    TRY(tb.put(dl.data(), sizeof(float) * dl.size()));
    rs.tab = tb;
    if (out_n > 0) HK(hipMemcpy(o.p, out, es * (size_t)out_n, hipMemcpyHostToDevice));  // samples outside every window keep their values
    if (q3_launch_pcm_resample(s, (size_t)stride, pk, ps, n_ent, mx, rs, format, o.p, nullptr) != 0)
        return q3_set_err(nullptr, Q3TTS_ERR_UNSUPPORTED, "pcm resample hook: the input span of one tile does not fit the LDS");
    HK(hipGetLastError());
    HK(hipDeviceSynchronize());
    TRY(time_launches(iters, [&] { q3_launch_pcm_resample(s, (size_t)stride, pk, ps, n_ent, mx, rs, format, o.p, nullptr); }, mean_ms));
    return out_n > 0 ? o.get(out, es * (size_t)out_n) : Q3TTS_OK;
}

extern "C" int q3tts_k_tempo_counts(int64_t n, int32_t permille, int64_t* N, int64_t* D) {
    if (!N || !D || n < 0 || n > (1ll << 40) || permille < Q3_TEMPO_MIN || permille > Q3_TEMPO_MAX) return q3_set_err(nullptr, Q3TTS_ERR_INVALID, "tempo counts hook: bad arguments");
    *N = q3_tempo_N(n, permille); *D = q3_tempo_valid(n, permille, false);
    return Q3TTS_OK;
}

extern "C" int q3tts_k_pcm_tempo(int32_t device, const float* src, int32_t rows, int64_t stride, const int32_t* lens, int32_t n_steps, const int32_t* row_final,
                                 int32_t permille, float* out, int64_t out_stride, int32_t* n_valid, int32_t* delta, int64_t delta_stride, int32_t iters, float* mean_ms) {
    if (!src || !lens || !row_final || !out || !n_valid || rows <= 0 || rows > 4096 || stride <= 0 || stride > (1 << 28) || n_steps <= 0 || n_steps > 64 ||
        permille < Q3_TEMPO_MIN || permille > Q3_TEMPO_MAX || out_stride <= 0 || delta_stride < 0 || (delta_stride > 0 && !delta))
        return q3_set_err(nullptr, Q3TTS_ERR_INVALID, "pcm tempo hook: bad arguments");
    for (int r = 0; r < rows; ++r)
        for (int t = 0; t < n_steps; ++t) {
            const long long n = lens[(size_t)t * rows + r];
            if (n < 0 || n > stride || (t > 0 && n < lens[(size_t)(t - 1) * rows + r])) return q3_set_err(nullptr, Q3TTS_ERR_INVALID, "pcm tempo hook: a row's valid lengths must ascend inside its row");
            if (q3_tempo_valid(n, permille, t == n_steps - 1 && row_final[r]) > out_stride) return q3_set_err(nullptr, Q3TTS_ERR_INVALID, "pcm tempo hook: out_stride is below a row's outputs");
        }
    HK(hipSetDevice(device));
    std::vector<float> w;
    q3_tempo_window(w);
    DevBuf s, o, dw, pl, dd;
    const size_t ob = sizeof(float) * (size_t)rows * out_stride;
    TRY(s.put(src, sizeof(float) * (size_t)rows * stride)); TRY(o.alloc(ob)); TRY(dw.put(w.data(), sizeof(float) * w.size()));
    TRY(pl.alloc(sizeof(long long) * rows)); TRY(dd.alloc(sizeof(int32_t) * (size_t)rows * std::max<int64_t>(delta_stride, 1)));
    HK(hipMemset(o.p, 0xFF, ob));  // what no launch writes reads back as NaN
    if (delta_stride > 0) HK(hipMemset(dd.p, 0x7F, sizeof(int32_t) * (size_t)rows * delta_stride));
    std::vector<int> done(rows, 0);
    std::vector<Q3TempoPack> last; std::vector<int> last_n;
    for (int t = 0; t < n_steps; ++t) {
        std::vector<Q3TempoPack> pks; std::vector<int> cnt;
        for (int r = 0; r < rows; ++r) {
            const int n = lens[(size_t)t * rows + r];
            const bool fin = t == n_steps - 1 && row_final[r];
            const long long kt = q3_tempo_frames(n, permille, fin), nv = q3_tempo_valid(n, permille, fin);
            n_valid[(size_t)t * rows + r] = (int32_t)nv;
            if (kt <= done[r]) continue;
            if (pks.empty() || cnt.back() == Q3_PCM_MAX_ENT) { pks.push_back(Q3TempoPack{}); cnt.push_back(0); }
            pks.back().e[cnt.back()++] = Q3TempoEnt{r, n, done[r], (int32_t)kt, (int32_t)nv, 0};
            done[r] = (int)kt;
        }
        for (size_t g = 0; g < pks.size(); ++g)
            q3_launch_pcm_tempo(s, (size_t)stride, o, (size_t)out_stride, pl, dw, permille, pks[g], cnt[g], delta_stride > 0 ? (int32_t*)dd : nullptr, (size_t)delta_stride, nullptr);
        HK(hipGetLastError());
        HK(hipDeviceSynchronize());
        TRY(o.get(out + (size_t)t * rows * out_stride, ob));
        last = pks; last_n = cnt;
    }
    if (delta_stride > 0) TRY(dd.get(delta, sizeof(int32_t) * (size_t)rows * delta_stride));
    // (the timed launches repeat the last step's: its outputs were copied above)
    return time_launches(iters, [&] {
        for (size_t g = 0; g < last.size(); ++g) q3_launch_pcm_tempo(s, (size_t)stride, o, (size_t)out_stride, pl, dw, permille, last[g], last_n[g], nullptr, 0, nullptr);
    }, mean_ms);
}

static int long_hook_rows(const char* what, const float* src, int32_t rows, int64_t stride, const int32_t* lens, long long* max_len) {
    if (!src || !lens || rows <= 0 || rows > 4096 || stride <= 0 || stride > (1 << 28)) return q3_set_err(nullptr, Q3TTS_ERR_INVALID, std::string(what) + ": bad arguments");
    *max_len = 0;
    for (int r = 0; r < rows; ++r) {
        if (lens[r] < 0 || lens[r] > stride) return q3_set_err(nullptr, Q3TTS_ERR_INVALID, std::string(what) + ": a row's valid length lies outside its row");
        *max_len = std::max<long long>(*max_len, lens[r]);
    }
    return Q3TTS_OK;
}

extern "C" int q3tts_k_pcm_edges(int32_t device, const float* src, int32_t rows, int64_t stride, const int32_t* lens, float threshold, int32_t* edges,
                                 int32_t iters, float* mean_ms) {
    long long mx = 0;
    TRY(long_hook_rows("pcm edges hook", src, rows, stride, lens, &mx));
    if (!edges || !(threshold >= 0.0f)) return q3_set_err(nullptr, Q3TTS_ERR_INVALID, "pcm edges hook: bad arguments");
    HK(hipSetDevice(device));
    std::vector<int32_t> init((size_t)2 * rows);
    for (int r = 0; r < rows; ++r) { init[2 * r] = INT32_MAX; init[2 * r + 1] = -1; }
    DevBuf s, l, ed;
    TRY(s.put(src, sizeof(float) * (size_t)rows * stride)); TRY(l.put(lens, sizeof(int32_t) * rows)); TRY(ed.put(init.data(), sizeof(int32_t) * 2 * rows));
    q3_launch_pcm_edges(s, (size_t)stride, l, rows, mx, threshold, ed, nullptr);
    HK(hipGetLastError());
    HK(hipDeviceSynchronize());
    TRY(ed.get(edges, sizeof(int32_t) * 2 * rows));
    return time_launches(iters, [&] { q3_launch_pcm_edges(s, (size_t)stride, l, rows, mx, threshold, ed, nullptr); }, mean_ms);
}

extern "C" int q3tts_k_pcm_join(int32_t device, const float* src, int32_t rows, int64_t stride, const int32_t* lens, const int32_t* kinds, const int32_t* edges,
                                const q3tts_join_opts* opts, int32_t rate, float* out, int64_t out_cap, int64_t* plan, int64_t* N, int32_t iters, float* mean_ms) {
    long long mx = 0;
    TRY(long_hook_rows("pcm join hook", src, rows, stride, lens, &mx));
    if (!kinds || !edges || !opts || !out || !plan || !N || out_cap <= 0 || rate < 1000) return q3_set_err(nullptr, Q3TTS_ERR_INVALID, "pcm join hook: bad arguments");
    const char* msg = nullptr;
    if (q3_join_opts_rules(*opts, &msg) != Q3TTS_OK) return q3_set_err(nullptr, Q3TTS_ERR_INVALID, msg);
    for (int r = 0; r < rows; ++r) {
        if (kinds[r] < 0 || kinds[r] > 4) return q3_set_err(nullptr, Q3TTS_ERR_INVALID, "pcm join hook: a break kind lies outside 0..4");
        const long long nb = ((long long)lens[r] + Q3_JOIN_W - 1) / Q3_JOIN_W;
        if (edges[2 * r + 1] >= 0 && (edges[2 * r] < 0 || edges[2 * r] > edges[2 * r + 1] || edges[2 * r + 1] >= nb))
            return q3_set_err(nullptr, Q3TTS_ERR_INVALID, "pcm join hook: a row's edges lie outside its blocks");
    }
    std::vector<Q3JoinSeg> segs((size_t)rows);
    std::vector<long long> pl((size_t)4 * rows);
    long long span = 0;
    const long long n_doc = q3_join_plan(lens, kinds, edges, rows, *opts, rate, pl.data(), segs.data(), &span);
    *N = n_doc;
    for (size_t k = 0; k < pl.size(); ++k) plan[k] = pl[k];
    if (n_doc > out_cap) return q3_set_err(nullptr, Q3TTS_ERR_INVALID, "pcm join hook: out holds fewer than N samples (*N says how many)");
    HK(hipSetDevice(device));
    DevBuf s, sg, o;
    TRY(s.put(src, sizeof(float) * (size_t)rows * stride)); TRY(sg.put(segs.data(), sizeof(Q3JoinSeg) * rows)); TRY(o.put(out, sizeof(float) * (size_t)out_cap));
    q3_launch_pcm_join(s, (size_t)stride, sg, rows, span, o, nullptr);
    HK(hipGetLastError());
    HK(hipDeviceSynchronize());
    TRY(o.get(out, sizeof(float) * (size_t)out_cap));
    return time_launches(iters, [&] { q3_launch_pcm_join(s, (size_t)stride, sg, rows, span, o, nullptr); }, mean_ms);
}

// The streaming join boundary by boundary (q3_doc.hip): a model of a session in which the rows are the segments' PCM rows. With a speed
// or an output rate (q3tts_k_doc_stream_rate) the pieces go into the ring RJ and the pipeline's other stages run behind the join.
static int doc_stream_run(int32_t device, const float* src, int32_t rows, int64_t stride, const int32_t* kinds, const int32_t* sched,
                          const int32_t* sched_n, int32_t sched_stride, const q3tts_join_opts* opts, int32_t rate, int32_t ahead, int32_t lag,
                          int64_t staging, int64_t dst0, int32_t format, int32_t check_rows, void* out, int64_t out_cap, int64_t* n_out,
                          int64_t* chunks, int32_t chunk_cap, int32_t* n_bounds, int64_t* plan, int64_t* bad, int32_t speed_permille,
                          int32_t output_rate, int64_t ring_j, int64_t ring_t, int32_t* delta, int32_t delta_cap, int32_t* n_frames) {
    if (!src || !kinds || !sched || !sched_n || !opts || !out || !n_out || !chunks || !n_bounds || !plan || !bad || rows <= 0 || rows > Q3_JOIN_MAX_SEG ||
        stride <= 0 || stride > (1 << 28) || sched_stride <= 0 || rate < 1000 || ahead < 1 || ahead > Q3_DOC_MAX_ENT || (lag != 0 && lag != 1) ||
        dst0 < 0 || staging <= dst0 || staging > (1 << 28) || (format != 0 && format != 1) || out_cap < 0 || chunk_cap <= 0)
        return q3_set_err(nullptr, Q3TTS_ERR_INVALID, "doc stream hook: bad arguments");
    const char* msg = nullptr;
    if (q3_join_opts_rules(*opts, &msg) != Q3TTS_OK) return q3_set_err(nullptr, Q3TTS_ERR_INVALID, msg);
    for (int i = 0; i < rows; ++i) {
        if (kinds[i] < 0 || kinds[i] > 4 || sched_n[i] < 1 || sched_n[i] > sched_stride) return q3_set_err(nullptr, Q3TTS_ERR_INVALID, "doc stream hook: a break kind or a schedule's length is out of range");
        for (int k = 0; k < sched_n[i]; ++k) {
            const long long v = sched[(size_t)i * sched_stride + k];
            if (v < 0 || v > stride || (k > 0 && v < sched[(size_t)i * sched_stride + k - 1])) return q3_set_err(nullptr, Q3TTS_ERR_INVALID, "doc stream hook: a row's valid lengths must ascend inside its row");
        }
    }
    // the pipeline of a document with a speed or a rate: its flow control state, the resampler's table, the rings
    Q3DocRing rg{};
    Q3Resamp rs{};
    std::vector<float> rtab;
    rg.speed = (speed_permille == 0 || speed_permille == 1000) ? 0 : speed_permille;
    if (rg.speed && (rg.speed < Q3_TEMPO_MIN || rg.speed > Q3_TEMPO_MAX)) return q3_set_err(nullptr, Q3TTS_ERR_INVALID, "doc stream hook: speed_permille is 0 or 1000 (off), or 500..2000");
    if (output_rate != 0 && output_rate != rate) {
        const int prc = q3_resample_table(rate, output_rate, &rs.L, &rs.M, &rs.H, rtab);
        if (prc != Q3TTS_OK) return q3_set_err(nullptr, prc, "doc stream hook: the rate pair is refused");
        rs.rate_in = rate; rs.rate_out = output_rate; rs.T = 2 * rs.H + 1;
        rg.L = rs.L; rg.M = rs.M; rg.H = rs.H;
    }
    const bool ringed = rg.speed || rg.L;
    if (ringed) {
        const long long mj = q3_doc_ring_min_j(rg.speed, rg.L, rg.M, rg.H), mt = q3_doc_ring_min_t(rg.speed, rg.L, rg.M, rg.H);
        rg.cj = ring_j ? ring_j : mj; rg.ct = ring_t ? ring_t : mt;
        if (rg.cj < mj || rg.ct < mt || (rg.cj & 3) || (rg.ct & 3) || rg.cj > (1 << 28) || rg.ct > (1 << 28) || delta_cap < 0 || (delta_cap > 0 && !delta))
            return q3_set_err(nullptr, Q3TTS_ERR_INVALID, "doc stream hook: a ring is below its minimum (" + std::to_string(mj) + ", " + std::to_string(mt) + ") or no multiple of 4");
    }
    HK(hipSetDevice(device));
    DevBuf rj, rt, dw, dpl, dd, dtab;
    if (ringed) {
        TRY(rj.alloc(sizeof(float) * (size_t)rg.cj)); HK(hipMemset(rj.p, 0xFF, sizeof(float) * (size_t)rg.cj));
        if (rg.speed) {
            std::vector<float> w;
            q3_tempo_window(w);
            TRY(rt.alloc(sizeof(float) * (size_t)rg.ct)); HK(hipMemset(rt.p, 0xFF, sizeof(float) * (size_t)rg.ct));
            TRY(dw.put(w.data(), sizeof(float) * w.size())); TRY(dpl.alloc(sizeof(long long)));
            TRY(dd.alloc(sizeof(int32_t) * (size_t)std::max(delta_cap, 1))); HK(hipMemset(dd.p, 0x7F, sizeof(int32_t) * (size_t)std::max(delta_cap, 1)));
        }
        if (rg.L) {
            const std::vector<float> dl = q3_resample_device_layout(rtab, rs.L, rs.M, rs.T);
            TRY(dtab.put(dl.data(), sizeof(float) * dl.size()));
            rs.tab = dtab;
        }
    }
    bool all_out = false;
    const size_t es = format ? 2 : 4, dstride = ((size_t)stride + 3) & ~(size_t)3;
    std::vector<int32_t> ed((size_t)2 * rows);
    for (int i = 0; i < rows; ++i) { ed[2 * i] = INT32_MAX; ed[2 * i + 1] = -1; }
    std::vector<uint32_t> mirror((size_t)ahead * dstride, 0xFFFFFFFFu), back(check_rows ? mirror.size() : 0);
    // behind the staging samples (rounded up to 4 bytes) the edge table of all rows: with lag = 1 it rides the boundary's copy, as in a session
    const size_t stg_al = ((size_t)staging + 1) & ~(size_t)1, tab_bytes = sizeof(int32_t) * 2 * (size_t)rows;
    std::vector<unsigned char> fill(stg_al * es + tab_bytes, 0xA5), got(fill.size());
    DevBuf s, dr, de, stg;
    TRY(s.put(src, sizeof(float) * (size_t)rows * stride)); TRY(dr.put(mirror.data(), sizeof(float) * mirror.size()));
    TRY(de.put(ed.data(), sizeof(int32_t) * ed.size())); TRY(stg.alloc(fill.size()));
    std::vector<int> pos((size_t)rows, -1), n((size_t)rows, 0);
    std::vector<char> closed((size_t)rows, 0);
    std::vector<Q3DocSegNow> now((size_t)rows), prev((size_t)rows);
    for (int i = 0; i < rows; ++i) now[i] = prev[i] = Q3DocSegNow{0, INT32_MAX, -1, 0, kinds[i]};
    Q3DocState st{};
    long long total = 0;
    int nbd = 0;
    *bad = 0;
    while (st.head < rows || (ringed && !all_out)) {
        if (nbd >= chunk_cap) return q3_set_err(nullptr, Q3TTS_ERR_INVALID, "doc stream hook: more boundaries than chunk_cap");
        Q3DocScanPack sp{};
        int ns = 0;
        for (long long i = st.head; i < std::min<long long>(rows, st.head + ahead); ++i) {
            if (closed[i]) continue;
            const int nn = sched[(size_t)i * sched_stride + ++pos[i]];
            if (pos[i] == sched_n[i] - 1) closed[i] = 1;
            float* drow = (float*)dr + (size_t)(i % ahead) * dstride;
            sp.e[ns++] = Q3DocScan{(const float*)s + (size_t)i * stride, drow, (int32_t*)de + 2 * i, n[i], nn, opts->threshold, 0};
            memcpy(mirror.data() + (size_t)(i % ahead) * dstride + n[i], src + (size_t)i * stride + n[i], sizeof(float) * (size_t)(nn - n[i]));
            n[i] = nn;
        }
        q3_launch_doc_scan(sp, ns, nullptr);
        HK(hipGetLastError());
        if (!lag) TRY(de.get(ed.data(), sizeof(int32_t) * ed.size()));
        if (check_rows) {
            TRY(dr.get(back.data(), sizeof(float) * back.size()));
            for (size_t k = 0; k < back.size(); ++k) *bad += back[k] != mirror[k];
        }
        if (!lag) for (int i = 0; i < rows; ++i) now[i] = Q3DocSegNow{n[i], ed[2 * i], ed[2 * i + 1], closed[i], kinds[i]};
        std::vector<Q3DocOut> pc; std::vector<Q3DocDone> dn;
        const int prc = q3_doc_plan(*opts, rate, lag ? prev.data() : now.data(), rows, ringed ? q3_doc_ring_room(rg) : staging - dst0, &st, &pc, &dn);
        if (prc != Q3TTS_OK) return q3_set_err(nullptr, prc, "document: the delivered length would pass 2^28 samples at segment " + std::to_string(st.head));
        for (const Q3DocDone& d : dn) { int64_t* p = plan + 4 * d.seg; p[0] = d.lo; p[1] = d.hi; p[2] = d.begin; p[3] = d.end; }
        HK(hipMemcpy(stg.p, fill.data(), fill.size(), hipMemcpyHostToDevice));
        long long cur = dst0;
        if (ringed) {  // join into RJ, stretch into RT, exit into the staging buffer: three stages in stream order
            std::vector<Q3DocPiece> ents;
            long long pos = rg.nj;
            for (const Q3DocOut& p : pc) {
                q3_doc_ring_put(p, p.seg < 0 ? nullptr : (const float*)dr + (size_t)(p.seg % ahead) * dstride + p.src, pos, rg.cj, &ents);
                pos += p.count;
            }
            q3_launch_doc_emit_all(ents, 0, rj.p, nullptr);
            Q3DocRingStep rp{};
            q3_doc_ring_step(&rg, pos - rg.nj, st.head >= rows, staging - dst0, &rp);
            if (rg.speed) q3_launch_doc_tempo(rj, rg.cj, rt, rg.ct, dpl, dw, rg.speed, rg.nj, rp.k_from, rp.k_to, rp.nt, delta_cap > 0 ? (int32_t*)dd : nullptr, (size_t)delta_cap, nullptr);
            const float* xr = rg.speed ? (const float*)rt : (const float*)rj;
            const long long cx = rg.speed ? rg.ct : rg.cj;
            if (rg.L) {
                if (q3_launch_doc_resample(xr, cx, rp.nx, rp.fin_x != 0, rp.first, rp.count, rs, format, stg.p, dst0, nullptr) != 0)
                    return q3_set_err(nullptr, Q3TTS_ERR_UNSUPPORTED, "doc stream hook: the input span of one tile does not fit the LDS");
            } else {
                ents.clear();
                q3_doc_ring_get(xr, cx, rp.first, rp.count, dst0, &ents);
                q3_launch_doc_emit_all(ents, format, stg.p, nullptr);
            }
            cur = dst0 + rp.count;
            all_out = rp.all_out != 0;
        } else
        for (size_t g0 = 0; g0 < pc.size(); g0 += Q3_DOC_MAX_ENT) {
            Q3DocPiecePack pk{};
            const int np = (int)std::min<size_t>(pc.size() - g0, Q3_DOC_MAX_ENT);
            for (int k = 0; k < np; ++k) {
                const Q3DocOut& p = pc[g0 + k];
                const float* from = p.seg < 0 ? nullptr : (const float*)dr + (size_t)(p.seg % ahead) * dstride + p.src;
                pk.e[k] = Q3DocPiece{from, p.j0, p.L, cur, (int32_t)p.count, p.F};
                cur += p.count;
            }
            if (cur > staging) return q3_set_err(nullptr, Q3TTS_ERR_STATE, "doc stream hook: the plan exceeds the staging buffer");
            q3_launch_doc_emit(pk, np, format, stg.p, nullptr);
        }
        if (lag) {  // this boundary's edges, for the next boundary's plan
            Q3DocPiecePack pk{};
            pk.e[0] = Q3DocPiece{(const float*)de.p, 0, 0, (long long)(stg_al * es), 2 * rows, -1};
            q3_launch_doc_emit(pk, 1, format, stg.p, nullptr);
        }
        HK(hipGetLastError());
        TRY(stg.get(got.data(), got.size()));
        if (lag) {
            memcpy(ed.data(), got.data() + stg_al * es, tab_bytes);
            for (int i = 0; i < rows; ++i) now[i] = Q3DocSegNow{n[i], ed[2 * i], ed[2 * i + 1], closed[i], kinds[i]};
        }
        prev = now;
        const long long c = cur - dst0;
        for (size_t k = 0; k < stg_al * es + (lag ? 0 : tab_bytes); ++k)
            if ((k < (size_t)dst0 * es || k >= (size_t)cur * es) && got[k] != 0xA5) ++*bad;
        if (total + c > out_cap) return q3_set_err(nullptr, Q3TTS_ERR_INVALID, "doc stream hook: out is too small");
        memcpy((char*)out + (size_t)total * es, got.data() + (size_t)dst0 * es, (size_t)c * es);
        total += c;
        chunks[nbd++] = c;
    }
    *n_out = total; *n_bounds = nbd;
    if (n_frames) *n_frames = (int32_t)rg.kt;
    if (rg.speed && delta_cap > 0) TRY(dd.get(delta, sizeof(int32_t) * (size_t)delta_cap));
    return Q3TTS_OK;
}

extern "C" int q3tts_k_doc_stream(int32_t device, const float* src, int32_t rows, int64_t stride, const int32_t* kinds, const int32_t* sched,
                                  const int32_t* sched_n, int32_t sched_stride, const q3tts_join_opts* opts, int32_t rate, int32_t ahead, int32_t lag,
                                  int64_t staging, int64_t dst0, int32_t format, int32_t check_rows, void* out, int64_t out_cap, int64_t* n_out,
                                  int64_t* chunks, int32_t chunk_cap, int32_t* n_bounds, int64_t* plan, int64_t* bad) {
    return doc_stream_run(device, src, rows, stride, kinds, sched, sched_n, sched_stride, opts, rate, ahead, lag, staging, dst0, format, check_rows, out, out_cap,
                          n_out, chunks, chunk_cap, n_bounds, plan, bad, 0, 0, 0, 0, nullptr, 0, nullptr);
}

extern "C" int q3tts_k_doc_stream_rate(int32_t device, const float* src, int32_t rows, int64_t stride, const int32_t* kinds, const int32_t* sched,
                                       const int32_t* sched_n, int32_t sched_stride, const q3tts_join_opts* opts, int32_t rate, int32_t ahead, int32_t lag,
                                       int64_t staging, int64_t dst0, int32_t format, int32_t check_rows, void* out, int64_t out_cap, int64_t* n_out,
                                       int64_t* chunks, int32_t chunk_cap, int32_t* n_bounds, int64_t* plan, int64_t* bad, int32_t speed_permille,
                                       int32_t output_rate, int64_t ring_j, int64_t ring_t, int32_t* delta, int32_t delta_cap, int32_t* n_frames) {
    const bool off = (speed_permille == 0 || speed_permille == 1000) && (output_rate == 0 || output_rate == rate);
    if (off) return q3_set_err(nullptr, Q3TTS_ERR_INVALID, "doc stream rate hook: neither a speed nor a rate (q3tts_k_doc_stream is the plain form)");
    return doc_stream_run(device, src, rows, stride, kinds, sched, sched_n, sched_stride, opts, rate, ahead, lag, staging, dst0, format, check_rows, out, out_cap,
                          n_out, chunks, chunk_cap, n_bounds, plan, bad, speed_permille, output_rate, ring_j, ring_t, delta, delta_cap, n_frames);
}

extern "C" int q3tts_k_rng_f32(uint64_t seed, int32_t n, float* out) {
    if (!out || n < 0) return Q3TTS_ERR_INVALID;
    q3_stdrng_f32(seed, n, out);
    return Q3TTS_OK;
}

// The clone audio encoder's quantiser (q3_clone.hip) on given operands: ps / pa [T][D], books row-major [ncb][CS][D] f32; ONE q3_launch_rvq, which
// transposes every book with the production k_cb_transpose and runs the production k_rvq; codes [T][ncb]. pa may be NULL when ncb == 1.
extern "C" int q3tts_k_rvq(int32_t device, const float* ps, const float* pa, int32_t T, int32_t D, const float* books, int32_t ncb, int32_t CS, int64_t* codes) {
    if (!ps || (!pa && ncb > 1) || !books || !codes || T < 1 || T > 65536 || D < 16 || D % 16 || D > 4096 || ncb < 1 || ncb > 64 || CS < 1 || (int64_t)CS * D > ((int64_t)1 << 26))
        return q3_set_err(nullptr, Q3TTS_ERR_INVALID, "rvq hook: bad shape");
    HK(hipSetDevice(device));
    const size_t ne = (size_t)CS * D;
    DevBuf dps, dpa, dbk, dbt, dtab, dcodes;
    TRY(dps.put(ps, (size_t)T * D * 4)); TRY(dpa.put(pa, (size_t)T * D * 4)); TRY(dbk.put(books, (size_t)ncb * ne * 4)); TRY(dbt.alloc((size_t)ncb * ne * 4));
    std::vector<const float*> tab(ncb);
    for (int q = 0; q < ncb; ++q) tab[q] = (const float*)dbt.p + (size_t)q * ne;
    TRY(dtab.put(tab.data(), (size_t)ncb * sizeof(float*))); TRY(dcodes.alloc((size_t)T * ncb * 8));
    Q3Rvq a{}; a.ps = dps; a.pa = pa ? (const float*)dpa.p : nullptr; a.T = T; a.D = D; a.cbT = (const float* const*)dtab.p; a.ncb = ncb; a.CS = CS;
    a.codes = (long long*)dcodes.p; a.books = dbk; a.booksT = dbt;
    if (q3_launch_rvq(a, nullptr)) return q3_set_err(nullptr, Q3TTS_ERR_INVALID, "rvq hook: the launch was refused");
    HK(hipGetLastError()); HK(hipDeviceSynchronize());
    return dcodes.get(codes, (size_t)T * ncb * 8);
}

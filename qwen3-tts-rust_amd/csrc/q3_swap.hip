// q3_swap.hip — swapping a parked request out of its slot and into any free one (include/q3tts.h, "paced requests and swapping";
// DESIGN.md §24). Three parts: the arena's allocator (host only: first fit over 256-byte units, neighbours coalesced on free), the table
// of everything a slot owns besides its Talker K/V, and the moves. The K/V of positions < cur_pos travels as a prefix store of
// P = cur_pos rows through q3_launch_kv_prefix_save / q3_launch_kv_prefix (q3_attend.hip), which are pinned byte for byte; everything
// else through k_slot_state_save / k_slot_state_load below, table-driven like k_voc_zero and over the same list of history blocks.
#include "q3_engine.h"

#include <map>
#include <memory>

namespace {

constexpr long long kUnit = 256;

// free runs of the arena by first unit; allocation is first fit in address order
struct Arena {
    long long units = 0, used = 0;
    std::map<long long, long long> free_runs;  // first unit -> units
    explicit Arena(long long cap_bytes) : units(std::max(0ll, cap_bytes) / kUnit) { if (units > 0) free_runs[0] = units; }
    long long alloc(long long bytes) {
        if (bytes <= 0) return -1;
        const long long n = (bytes + kUnit - 1) / kUnit;
        for (auto it = free_runs.begin(); it != free_runs.end(); ++it) {
            if (it->second < n) continue;
            const long long at = it->first, rest = it->second - n;
            free_runs.erase(it);
            if (rest > 0) free_runs[at + n] = rest;
            used += n;
            return at * kUnit;
        }
        return -1;
    }
    void release(long long off, long long bytes) {
        long long at = off / kUnit, n = (bytes + kUnit - 1) / kUnit;
        used -= n;
        auto nx = free_runs.lower_bound(at);
        if (nx != free_runs.end() && at + n == nx->first) { n += nx->second; nx = free_runs.erase(nx); }
        if (nx != free_runs.begin()) {
            auto pv = std::prev(nx);
            if (pv->first + pv->second == at) { pv->second += n; return; }
        }
        free_runs[at] = n;
    }
};

// One table entry: slot b's bytes [base + b * stride, + bytes) live at `off` of a block's state part. var: the entry's length is the
// request's own (Q3SwapReq::var_bytes, at most `bytes`) — the produced part of the PCM row, always the table's last entry.
struct SwapEnt { char* base; unsigned long long stride, bytes, off; int var, pad; };
struct SwapReq { char* state[Q3_KVP_MAX]; unsigned long long var_bytes[Q3_KVP_MAX]; int slot[Q3_KVP_MAX]; };

constexpr int kSwapZ = 8;  // workgroups per (entry, request)

// grid (entries, requests, kSwapZ): entry e0 + blockIdx.x of request blockIdx.y, in 16-byte units where both ends and the length allow
// (every block offset is a multiple of 16, so that is whenever the slot's own address is), else in dwords (all state is whole dwords).
template <bool SAVE>
__device__ __forceinline__ void slot_state_move(const SwapEnt* __restrict__ tab, int e0, const SwapReq& rq) {
    const SwapEnt z = tab[e0 + blockIdx.x];
    const int j = blockIdx.y;
    char* dev = z.base + (size_t)rq.slot[j] * z.stride;
    char* blk = rq.state[j] + z.off;
    const unsigned long long n = z.var ? (rq.var_bytes[j] < z.bytes ? rq.var_bytes[j] : z.bytes) : z.bytes;
    const char* src = SAVE ? dev : blk;
    char* dst = SAVE ? blk : dev;
    const size_t t0 = (size_t)blockIdx.z * blockDim.x + threadIdx.x, step = (size_t)gridDim.z * blockDim.x;
    if ((((unsigned long long)(uintptr_t)src | (unsigned long long)(uintptr_t)dst | n) & 15ull) == 0) {
        const uint4* s16 = (const uint4*)src; uint4* d16 = (uint4*)dst;
        for (size_t i = t0; i < (size_t)(n >> 4); i += step) d16[i] = s16[i];
    } else {
        const uint32_t* s4 = (const uint32_t*)src; uint32_t* d4 = (uint32_t*)dst;
        for (size_t i = t0; i < (size_t)(n >> 2); i += step) d4[i] = s4[i];
    }
}
__global__ __launch_bounds__(256) void k_slot_state_save(const SwapEnt* __restrict__ tab, int e0, SwapReq rq) { slot_state_move<true>(tab, e0, rq); }
__global__ __launch_bounds__(256) void k_slot_state_load(const SwapEnt* __restrict__ tab, int e0, SwapReq rq) { slot_state_move<false>(tab, e0, rq); }

unsigned long long up16(unsigned long long n) { return (n + 15ull) & ~15ull; }

}  // namespace

struct Q3Swap {
    Arena arena;
    char* base = nullptr; long long cap = 0;
    SwapEnt* tab = nullptr; int n_dec = 0, n_voc = 0;   // device table: the decoder's entries [0, n_dec) (e->stream), then the vocoder's (e->vstream)
    unsigned long long fixed = 0, pcm_row = 0;         // bytes of a block's state part without the PCM; bytes of a whole PCM row
    size_t counted = 0;                                 // what e->dev_bytes carries for this
    // Every q3_swap_move gets a ticket and a pair of events behind its launches, one per stream: a block's bytes may be handed out again
    // only when both halves of the last move that touched them have RUN (q3_swap_done) — the next block over those bytes has another
    // layout, so its decode-stream half can cover what was this block's vocoder-stream half. The pairs are a ring made with the arena;
    // each stream completes its events in order, so a pair that is re-recorded stands for every ticket a ring's length back.
    static constexpr int kFences = 64;
    hipEvent_t ev_s[kFences] = {}, ev_v[kFences] = {};
    unsigned long long ticket = 0, done = 0;            // tickets issued; every ticket <= done has completed on both streams
    explicit Q3Swap(long long bytes) : arena(bytes) {}
};

bool q3_swap_done(Q3Swap* sw, unsigned long long t) {
    while (sw->done < t && sw->done < sw->ticket) {
        const int k = (int)((sw->done + 1) % Q3Swap::kFences);
        if (hipEventQuery(sw->ev_s[k]) != hipSuccess || hipEventQuery(sw->ev_v[k]) != hipSuccess) break;
        ++sw->done;
    }
    return sw->done >= t;
}

long long q3_swap_alloc(Q3Swap* sw, long long bytes) { return sw->arena.alloc(bytes); }
void q3_swap_release(Q3Swap* sw, long long off, long long bytes) { sw->arena.release(off, bytes); }
long long q3_swap_used(const Q3Swap* sw) { return sw->arena.used * kUnit; }

static unsigned long long pcm_bytes(const q3tts_engine* e, const Q3Swap* sw, int voc_frames) {
    const unsigned long long want = up16((unsigned long long)std::max(0, voc_frames) * q3_voc_samples_per_frame(e) * 4ull);
    return std::min(want, sw->pcm_row & ~15ull);
}
static int kv_np(int cur_pos) { return (std::max(cur_pos, 1) + 63) & ~63; }

long long q3_swap_block_bytes(const q3tts_engine* e, const Q3Swap* sw, int cur_pos, int voc_frames) {
    return (long long)(2 * q3_prefix_store_bytes(e, kv_np(cur_pos)) + sw->fixed + pcm_bytes(e, sw, voc_frames));
}

int q3_swap_create(q3tts_engine* e, long long arena_bytes, Q3Swap** out) {
    *out = nullptr;
    if (arena_bytes <= 0) return q3_set_err(e, Q3TTS_ERR_INVALID, "swap: the arena needs a positive size");
    if (!e->voc) return q3_set_err(e, Q3TTS_ERR_STATE, "swap: the engine has no vocoder");
    if (e->T.hd != Q3_ATT_HD || e->T.cache.n_ctx % 64) return q3_set_err(e, Q3TTS_ERR_UNSUPPORTED, "swap: the K/V copy needs head_dim 128 and n_ctx in whole key blocks");
    Q3_HIP(e, hipSetDevice(e->cfg.device));
    size_t free_b = 0, total_b = 0;
    Q3_HIP(e, hipMemGetInfo(&free_b, &total_b));
    if ((unsigned long long)arena_bytes > (unsigned long long)free_b)
        return q3_set_err(e, Q3TTS_ERR_OOM, "swap: the arena needs " + std::to_string(arena_bytes) + " bytes of device memory; the device has " + std::to_string((unsigned long long)free_b) + " bytes free");
    const q3tts_model_config& m = e->cfg.model;
    const unsigned long long cap = (unsigned long long)e->cfg.max_steps_cap, ncb = (unsigned long long)m.n_codebooks;
    std::vector<SwapEnt> tab;
    unsigned long long off = 0;
    auto add = [&](void* base, unsigned long long stride, unsigned long long bytes, int var) {
        tab.push_back(SwapEnt{(char*)base, stride, bytes, off, var, 0});
        off += up16(bytes);
    };
    // the decoder's: codes, the Talker's and the Predictor's draws, the repetition penalty's bitmap, the parked rows
    add(e->codes, cap * ncb * 4, cap * ncb * 4, 0);
    add(e->rng, cap * 4, cap * 4, 0);
    add(e->prng, cap * (ncb - 1) * 4, cap * (ncb - 1) * 4, 0);
    if (e->seen && e->seen_words > 0) add(e->seen, (unsigned long long)e->seen_words * 4, (unsigned long long)e->seen_words * 4, 0);
    add(e->park_logits, (unsigned long long)m.t_vocab * 4, (unsigned long long)m.t_vocab * 4, 0);
    add(e->park_x, (unsigned long long)m.t_d_model * 4, (unsigned long long)m.t_d_model * 4, 0);
    const int n_dec = (int)tab.size();
    // the vocoder's: history blocks and ring slices, then the PCM row (its produced part)
    std::vector<Q3SlotBlock> vb;
    q3_voc_slot_blocks(e, vb);
    for (const Q3SlotBlock& b : vb) add(b.base, b.stride, b.bytes, 0);
    std::unique_ptr<Q3Swap> sw(new Q3Swap(arena_bytes));
    sw->fixed = off;
    sw->pcm_row = (unsigned long long)q3_voc_pcm_stride(e) * 4;
    add(q3_voc_pcm(e, 0), sw->pcm_row, sw->pcm_row & ~15ull, 1);
    for (const SwapEnt& z : tab) if ((z.bytes | z.stride) & 3ull) return q3_set_err(e, Q3TTS_ERR_UNSUPPORTED, "swap: a per-slot block is not whole dwords");
    sw->n_dec = n_dec; sw->n_voc = (int)tab.size() - n_dec; sw->cap = arena_bytes;
    const size_t before = e->dev_bytes;
    int rc = q3_dev_alloc_zeroed(e, (void**)&sw->tab, tab.size() * sizeof(SwapEnt));
    if (rc == Q3TTS_OK) {
        void* p = nullptr;
        const hipError_t er = hipMalloc(&p, (size_t)arena_bytes);  // (not zeroed: a block is written before it is read)
        if (er != hipSuccess) rc = q3_set_err(e, Q3TTS_ERR_OOM, std::string("swap: hipMalloc of the arena: ") + hipGetErrorString(er));
        else { sw->base = (char*)p; e->dev_bytes += (size_t)arena_bytes; }
    }
    if (rc == Q3TTS_OK && hipMemcpy(sw->tab, tab.data(), tab.size() * sizeof(SwapEnt), hipMemcpyHostToDevice) != hipSuccess) rc = q3_set_err(e, Q3TTS_ERR_DEVICE, "swap: table upload");
    sw->counted = e->dev_bytes - before;
    for (int k = 0; k < Q3Swap::kFences && rc == Q3TTS_OK; ++k)
        if (hipEventCreateWithFlags(&sw->ev_s[k], hipEventDisableTiming) != hipSuccess || hipEventCreateWithFlags(&sw->ev_v[k], hipEventDisableTiming) != hipSuccess)
            rc = q3_set_err(e, Q3TTS_ERR_DEVICE, "swap: hipEventCreate");
    if (rc != Q3TTS_OK) { q3_swap_destroy(e, sw.release()); return rc; }
    *out = sw.release();
    return Q3TTS_OK;
}

void q3_swap_destroy(q3tts_engine* e, Q3Swap* sw) {
    if (!sw) return;
    for (int k = 0; k < Q3Swap::kFences; ++k) { if (sw->ev_s[k]) hipEventDestroy(sw->ev_s[k]); if (sw->ev_v[k]) hipEventDestroy(sw->ev_v[k]); }
    if (sw->tab) hipFree(sw->tab);
    if (sw->base) hipFree(sw->base);
    e->dev_bytes -= sw->counted;
    delete sw;
}

int q3_swap_move(q3tts_engine* e, Q3Swap* sw, const Q3SwapItem* items, int n, bool save, unsigned long long* ticket) {
    for (int g0 = 0; g0 < n; g0 += Q3_KVP_MAX) {
        const int c = std::min(n - g0, (int)Q3_KVP_MAX);
        Q3KvPrefix kp = q3_kv_prefix_of(e->T); kp.n = c;
        SwapReq rq{};
        for (int i = 0; i < c; ++i) {
            const Q3SwapItem& it = items[g0 + i];
            const long long need = q3_swap_block_bytes(e, sw, it.cur_pos, it.voc_frames);
            if (it.slot < 0 || it.slot >= e->B || it.cur_pos < 1 || it.cur_pos > e->T.cache.n_ctx || it.off < 0 || (it.off & 255) || it.off + need > sw->cap)
                return q3_set_err(e, Q3TTS_ERR_STATE, "swap: a block lies outside the arena, or a slot or position outside the engine's");
            const size_t store = q3_prefix_store_bytes(e, kv_np(it.cur_pos));
            char* blk = sw->base + it.off;
            kp.pk[i] = (const uint16_t*)blk; kp.pv[i] = (const uint16_t*)(blk + store); kp.P[i] = it.cur_pos; kp.slot[i] = it.slot;
            rq.state[i] = blk + 2 * store; rq.var_bytes[i] = pcm_bytes(e, sw, it.voc_frames); rq.slot[i] = it.slot;
        }
        if (save) { if (q3_launch_kv_prefix_save(kp, e->stream)) return q3_set_err(e, Q3TTS_ERR_INVALID, "swap: the K/V save was refused for this model shape"); }
        else q3_launch_kv_prefix(kp, e->stream);
        if (save) {
            hipLaunchKernelGGL(k_slot_state_save, dim3(sw->n_dec, c, kSwapZ), dim3(256), 0, e->stream, sw->tab, 0, rq);
            hipLaunchKernelGGL(k_slot_state_save, dim3(sw->n_voc, c, kSwapZ), dim3(256), 0, e->vstream, sw->tab, sw->n_dec, rq);
        } else {
            hipLaunchKernelGGL(k_slot_state_load, dim3(sw->n_dec, c, kSwapZ), dim3(256), 0, e->stream, sw->tab, 0, rq);
            hipLaunchKernelGGL(k_slot_state_load, dim3(sw->n_voc, c, kSwapZ), dim3(256), 0, e->vstream, sw->tab, sw->n_dec, rq);
        }
        Q3_HIP(e, hipGetLastError());
    }
    // the move's fence. Its ring entry last stood for the ticket kFences back: that one (and so every older one) has to be over first
    const unsigned long long t = sw->ticket + 1;
    const int k = (int)(t % Q3Swap::kFences);
    if (t > Q3Swap::kFences && !q3_swap_done(sw, t - Q3Swap::kFences)) {
        Q3_HIP(e, hipEventSynchronize(sw->ev_s[k])); Q3_HIP(e, hipEventSynchronize(sw->ev_v[k]));
        sw->done = std::max(sw->done, t - Q3Swap::kFences);
    }
    Q3_HIP(e, hipEventRecord(sw->ev_s[k], e->stream));
    Q3_HIP(e, hipEventRecord(sw->ev_v[k], e->vstream));
    sw->ticket = t;
    *ticket = t;
    return Q3TTS_OK;
}

// The arena's allocator alone, for tests (include/q3tts.h): ops[i] > 0 allocates that many bytes, ops[i] = -(k + 1) frees what ops[k] allocated
extern "C" int q3tts_k_swap_arena(int64_t cap, const int64_t* ops, int32_t n, int64_t* offsets) {
    if (cap < 0 || n < 0 || (n > 0 && (!ops || !offsets))) return q3_set_err(nullptr, Q3TTS_ERR_INVALID, "swap arena: null argument or a negative size");
    Arena a(cap);
    std::vector<char> held(n, 0);
    for (int i = 0; i < n; ++i) {
        if (ops[i] > 0) { offsets[i] = a.alloc(ops[i]); held[i] = offsets[i] >= 0; continue; }
        const long long k = -ops[i] - 1;
        if (ops[i] == 0 || k >= i || !held[k] || ops[k] <= 0) return q3_set_err(nullptr, Q3TTS_ERR_INVALID, "swap arena: a free names no live earlier allocation");
        a.release(offsets[k], ops[k]); held[k] = 0;
        offsets[i] = offsets[k];
    }
    return Q3TTS_OK;
}

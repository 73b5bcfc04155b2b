// q3_doc.hip — the streaming form of the long-document join (include/q3tts.h, "documents in a session: the streaming
// join"). A document's segments run as ordinary requests; what is the document's own lives here: k_doc_scan copies the samples of a
// running segment that became valid at a chunk boundary into the segment's document row and keeps the row's first / last loud block up
// to date, q3_doc_plan (host, pure) turns the segments' state into the pieces a boundary may emit, and k_doc_emit writes those pieces —
// fades, pauses, f32 or i16 — into the staging buffer. The arithmetic is q3_long.hip's, value for value: the concatenation of everything
// emitted is q3tts_generate_long's row. The reference has no counterpart (src/tts/engine.rs:152 truncates one text at 512 steps).
#include "q3_engine.h"

#include <climits>
#include <cstring>

namespace {
constexpr int W = Q3_JOIN_W;
constexpr int kThreads = 256, kWaves = kThreads / 64;
constexpr int kTileBlocks = 64;          // blocks of W samples per workgroup of k_doc_scan: 16 per wave
constexpr int kEmitTile = 4 * kThreads;  // outputs per pass of a k_doc_emit workgroup: one group of four per thread
static_assert(W % 4 == 0 && W + 3 <= 4 * 64, "a wave covers a block in one pass of 16-byte groups, whatever the row's alignment");
}  // namespace

// ---- the kernels --------------------------------------------------------------------------------------------------------------
// grid (tiles, entries): entry blockIdx.y is one running segment whose valid length grew from n_prev to n_now. Its workgroups take the
// blocks that intersect [n_prev, n_now), kTileBlocks per workgroup, one block per wave at a time, by k_pcm_edges' rules: a lane loads one
// 16-byte group of the source row where the group lies inside the block and inside [0, n_now), single elements at the edges, nothing at
// or past n_now; fmaxf drops a NaN; the comparison is strict. The block's first samples below n_prev are loaded again (the block was
// partial at the last boundary) but not stored: dst receives [n_prev, n_now) only. The integer atomicMin / atomicMax pair makes a block
// that is scanned twice harmless and the result independent of any order. LDS: 32 bytes.
__global__ __launch_bounds__(kThreads) void k_doc_scan(const Q3DocScanPack ents) {
    __shared__ int s_first[kWaves], s_last[kWaves];
    const Q3DocScan en = ents.e[blockIdx.y];
    const long long n0 = en.n_prev, n = en.n_now;
    const long long bf = n0 / W, nb = (n + W - 1) / W, b0 = bf + (long long)blockIdx.x * kTileBlocks;
    if (n <= n0 || b0 >= nb) return;  // (uniform over the workgroup)
    const float* row = en.src;
    float* out = en.dst;
    const int a = (int)(((uintptr_t)row >> 2) & 3);
    const bool same = ((((uintptr_t)out >> 2) & 3) == (unsigned)a);  // a 16-byte group of the source is one of the destination too
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int first = INT_MAX, last = -1;
    for (int t = wave; t < kTileBlocks && b0 + t < nb; t += kWaves) {
        const long long b = b0 + t, g0 = b * W, g1 = min(g0 + W, n);
        const long long g = g0 - (((long long)a + g0) & 3) + 4ll * lane;  // this lane's group, on a 16-byte boundary of the source row
        float m = 0.0f;
        if (g < g1) {
            if (g >= g0 && g + 4 <= g1) {
                const float4 v = *(const float4*)(row + g);
                m = fmaxf(fmaxf(m, fabsf(v.x)), fabsf(v.y));
                m = fmaxf(fmaxf(m, fabsf(v.z)), fabsf(v.w));
                if (same && g >= n0) *(float4*)(out + g) = v;
                else {
                    if (g >= n0) out[g] = v.x;
                    if (g + 1 >= n0) out[g + 1] = v.y;
                    if (g + 2 >= n0) out[g + 2] = v.z;
                    if (g + 3 >= n0) out[g + 3] = v.w;
                }
            } else {
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if (g + k >= g0 && g + k < g1) {
                        const float x = row[g + k];
                        m = fmaxf(m, fabsf(x));
                        if (g + k >= n0) out[g + k] = x;
                    }
            }
        }
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) m = fmaxf(m, __shfl_xor(m, off, 64));
        if (m > en.thr) { first = min(first, (int)b); last = max(last, (int)b); }
    }
    if (lane == 0) { s_first[wave] = first; s_last[wave] = last; }
    __syncthreads();
    if (threadIdx.x == 0 && en.edges) {
#pragma unroll
        for (int w = 1; w < kWaves; ++w) { first = min(first, s_first[w]); last = max(last, s_last[w]); }
        if (last >= 0) { atomicMin(en.edges, first); atomicMax(en.edges + 1, last); }
    }
}

void q3_launch_doc_scan(const Q3DocScanPack& ents, int n_ent, hipStream_t s) {
    if (n_ent <= 0) return;
    long long mx = 0;
    for (int i = 0; i < n_ent; ++i) {
        const Q3DocScan& en = ents.e[i];
        if (en.n_now > en.n_prev) mx = std::max(mx, ((long long)en.n_now + W - 1) / W - en.n_prev / W);
    }
    if (mx <= 0) return;
    hipLaunchKernelGGL(k_doc_scan, dim3((unsigned)((mx + kTileBlocks - 1) / kTileBlocks), n_ent), dim3(kThreads), 0, s, ents);
}

// grid (x, pieces): the workgroups of piece blockIdx.y walk dst[dst, dst + count) in groups of four outputs, one group per thread and
// pass, the groups laid on the 16-byte (f32) or 8-byte (i16) boundaries of the destination. Output t is sample j = j0 + t of the piece:
// src[t] by a dword load, times g(j, F) = (float)(j + 1) / (float)(F + 1) for j < F and times g(L - 1 - j, F) for j >= L - F — one
// correctly rounded division and one rounded multiply, as k_pcm_join — and copied bit for bit elsewhere; src == null: +0.0f (a pause).
// A piece of an open segment carries L = LLONG_MAX: the planner hands out nothing that the final fade-out could touch. The i16 form is
// k_pcm_pack's conversion of that f32 value. One vector store where the group lies inside the range, single elements at its ends. No LDS.
template <typename T>
__global__ __launch_bounds__(kThreads) void k_doc_emit(const Q3DocPiecePack pcs, T* __restrict__ dst) {
    const Q3DocPiece pc = pcs.e[blockIdx.y];
    const long long cnt = pc.count;
    if (cnt <= 0) return;
    if (pc.F < 0) {  // a table, not samples: count 32-bit words, bit for bit, to the BYTE offset dst (a multiple of 4) — the edges ride the copy
        const uint32_t* in = (const uint32_t*)pc.src;
        uint32_t* o = (uint32_t*)((char*)dst + pc.dst);
        for (long long q = (long long)blockIdx.x * kThreads + threadIdx.x; q < cnt; q += (long long)gridDim.x * kThreads) o[q] = in[q];
        return;
    }
    const float* x = pc.src;
    const long long F = pc.F, L = pc.L, j0 = pc.j0;
    const long long d_lo = pc.dst, d_hi = pc.dst + cnt;
    const long long gs = d_lo - (((long long)(((uintptr_t)dst / sizeof(T)) & 3) + d_lo) & 3);
    const long long groups = (d_hi - gs + 3) >> 2;
    const float den = (float)(F + 1);
    for (long long q = (long long)blockIdx.x * kThreads + threadIdx.x; q < groups; q += (long long)gridDim.x * kThreads) {
        const long long d = gs + 4 * q;
        float v[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const long long t = d + k - d_lo;
            float y = 0.0f;
            if (x && t >= 0 && t < cnt) {
                const long long j = j0 + t;
                y = x[t];
                if (j < F) y = __fmul_rn(y, __fdiv_rn((float)(j + 1), den));
                else if (j >= L - F) y = __fmul_rn(y, __fdiv_rn((float)(L - j), den));
            }
            v[k] = y;
        }
        if (d >= d_lo && d + 4 <= d_hi) {
            T o[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) q3_pcm_put(o + k, v[k]);
            if constexpr (sizeof(T) == 4) *(float4*)(dst + d) = make_float4(o[0], o[1], o[2], o[3]);
            else *(short4*)(dst + d) = make_short4(o[0], o[1], o[2], o[3]);
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (d + k >= d_lo && d + k < d_hi) q3_pcm_put(dst + d + k, v[k]);
        }
    }
}

void q3_launch_doc_emit(const Q3DocPiecePack& pcs, int n_pc, int i16, void* dst, hipStream_t s) {
    if (n_pc <= 0) return;
    long long mx = 0;
    for (int i = 0; i < n_pc; ++i) mx = std::max<long long>(mx, pcs.e[i].count);
    if (mx <= 0) return;
    const int gx = (int)std::max(1ll, std::min((mx + 3 + kEmitTile - 1) / kEmitTile, (long long)std::max(1, 4096 / n_pc)));
    if (i16) hipLaunchKernelGGL(k_doc_emit<int16_t>, dim3(gx, n_pc), dim3(kThreads), 0, s, pcs, (int16_t*)dst);
    else hipLaunchKernelGGL(k_doc_emit<float>, dim3(gx, n_pc), dim3(kThreads), 0, s, pcs, (float*)dst);
}

// ---- the plan (host) ----------------------------------------------------------------------------------------------------------
// One boundary of one document. Only the head — the first segment not fully delivered — emits; when it closes the next one becomes head
// in the same call, so one call may hand out the tail of a piece, whole pieces and their pauses, clipped to `room` samples.
int q3_doc_plan(const q3tts_join_opts& o, int rate, const Q3DocSegNow* segs, int n_segs, long long room, Q3DocState* st,
                std::vector<Q3DocOut>* pieces, std::vector<Q3DocDone>* done) {
    constexpr long long kMax = 1ll << 28;
    while (st->head < n_segs) {
        const Q3DocSegNow& sg = segs[st->head];
        const long long n = sg.n;
        long long lo = 0, hi = n;
        bool empty = false;
        if (o.trim) {
            if (sg.last < 0) { if (!sg.closed) break; empty = true; lo = hi = 0; }  // no loud block yet: nothing is known about the piece
            else { lo = std::max(0ll, (long long)sg.first * W - o.keep); hi = std::min(n, ((long long)sg.last + 1) * W + o.keep); }
        } else if (sg.closed && n == 0) empty = true;
        if (empty) {  // an empty piece: its kind is folded into the pause in front of the next non-empty one, as the join does
            done->push_back(Q3DocDone{(int32_t)st->head, 0, lo, hi, st->delivered, st->delivered});
            if (st->have_prev) st->kmax = std::max<long long>(st->kmax, sg.kind);
            ++st->head; st->e = 0; st->pause_left = -1;
            continue;
        }
        long long L = LLONG_MAX, F = o.fade, upto;
        if (sg.closed) { L = hi - lo; F = std::min<long long>(o.fade, L / 2); upto = L; }
        else {
            if (hi - lo < 2ll * o.fade) break;  // F is not final yet
            upto = hi - lo - o.fade;            // the final fade-out begins at or behind this sample
        }
        if (upto > st->e) {
            if (st->e == 0) {  // the pause goes out directly in front of the piece's first sample: the piece is known to be non-empty, kmax is final
                if (st->pause_left < 0) st->pause_left = st->have_prev ? (long long)o.pause_ms[st->kmax] * rate / 1000 : 0;
                const long long c = std::min(st->pause_left, room);
                if (st->delivered + st->pause_left > kMax) return Q3TTS_ERR_INVALID;
                if (c > 0) { pieces->push_back(Q3DocOut{-1, 0, 0, 0, c, 0, 0}); st->pause_left -= c; room -= c; st->delivered += c; }
                if (st->pause_left > 0) break;
                st->begin = st->delivered;
            }
            const long long c = std::min(upto - st->e, room);
            if (st->delivered + c > kMax) return Q3TTS_ERR_INVALID;
            if (c > 0) { pieces->push_back(Q3DocOut{(int32_t)st->head, (int32_t)F, lo + st->e, st->e, c, L, 0}); st->e += c; room -= c; st->delivered += c; }
            if (st->e < upto) break;
        }
        if (!sg.closed) break;
        done->push_back(Q3DocDone{(int32_t)st->head, 0, lo, hi, st->begin, st->begin + L});
        st->have_prev = 1; st->kmax = sg.kind;
        ++st->head; st->e = 0; st->pause_left = -1;
    }
    return Q3TTS_OK;
}

// ---- the pipeline of a document with a speed or a rate: flow control (host, pure) ----------------------------------------------
static_assert(Q3_DOC_RING_MIN_J_SPEED == Q3_TEMPO_HS * Q3_TEMPO_MAX / 1000 + Q3_TEMPO_HOLD - Q3_TEMPO_DMIN && Q3_DOC_RING_MIN_T_SPEED == Q3_TEMPO_HS,
              "the header's ring minima are written out from the time-stretch's constants");
namespace {
constexpr long long Hs = Q3_TEMPO_HS;
inline long long tempo_a(long long k, int s) { return (k * Hs * s) / 1000; }
// the lowest position of the exit's source that output m may read
inline long long rate_low(const Q3DocRing& r) { return std::max(0ll, (r.m * r.M) / r.L - r.H); }
}  // namespace

long long q3_doc_ring_min_j(int speed, int L, int M, int H) { return speed ? Q3_DOC_RING_MIN_J_SPEED : (L ? Q3_DOC_RING_MIN_RATE(H, L, M) : 0); }
long long q3_doc_ring_min_t(int speed, int L, int M, int H) { return !speed ? 0 : (L ? Q3_DOC_RING_MIN_T_RATE(H, L, M) : Q3_DOC_RING_MIN_T_SPEED); }

// The lowest position of RJ that may still be read: with a speed the next undecided frame k reads its template from p_{k-1} + Hs and
// its candidates from a_k + DMIN, both >= a_{k-1} + DMIN (delta >= DMIN, a ascends); without one, output m reads from (m M) div L - H.
long long q3_doc_ring_room(const Q3DocRing& r) {
    long long low;
    if (r.speed) low = r.kt == 0 ? 0 : std::max(0ll, tempo_a(r.kt - 1, r.speed) + Q3_TEMPO_DMIN);
    else low = rate_low(r);
    return std::max(0ll, low + r.cj - r.nj);
}

void q3_doc_ring_step(Q3DocRing* r, long long joined, bool fin_j, long long room_out, Q3DocRingStep* out) {
    r->nj += joined; r->fin_j = fin_j ? 1 : 0;
    *out = Q3DocRingStep{};
    long long nx = r->nj; bool fin_x = fin_j;
    if (r->speed) {
        // frame k writes RT[k Hs, (k + 1) Hs): it must end at or below low + ct, low the lowest position the exit may still read
        const long long low_t = r->L ? rate_low(*r) : r->m;
        const long long all = q3_tempo_frames(r->nj, r->speed, fin_j), fit = (low_t + r->ct) / Hs;
        const long long k_to = std::max(r->kt, std::min(all, fit));
        const long long NT = q3_tempo_N(r->nj, r->speed);
        out->k_from = (int32_t)r->kt; out->k_to = (int32_t)k_to;
        r->kt = k_to;
        fin_x = fin_j && k_to == all;
        nx = fin_j ? std::min(k_to * Hs, NT) : k_to * Hs;
        out->nt = nx;
    }
    const long long avail = r->L ? (fin_x ? q3_resample_N(nx, r->L, r->M) : q3_resample_D(nx, r->L, r->M, r->H)) : nx;
    out->nx = nx; out->fin_x = fin_x ? 1 : 0;
    out->first = r->m; out->count = std::max(0ll, std::min(avail - r->m, room_out));
    r->m += out->count;
    out->all_out = fin_x && r->m == avail ? 1 : 0;
    out->pending = (r->m < avail || (r->speed && r->kt < q3_tempo_frames(r->nj, r->speed, fin_j))) ? 1 : 0;
}

void q3_doc_ring_put(const Q3DocOut& p, const float* from, long long pos, long long C, std::vector<Q3DocPiece>* ents) {
    const long long at = pos % C, c1 = std::min(p.count, C - at);
    if (c1 > 0) ents->push_back(Q3DocPiece{from, p.j0, p.L, at, (int32_t)c1, p.F});
    if (p.count > c1) ents->push_back(Q3DocPiece{from ? from + c1 : nullptr, p.j0 + c1, p.L, 0, (int32_t)(p.count - c1), p.F});
}

void q3_doc_ring_get(const float* ring, long long C, long long first, long long count, long long at, std::vector<Q3DocPiece>* ents) {
    const long long from = first % C, c1 = std::min(count, C - from);
    if (c1 > 0) ents->push_back(Q3DocPiece{ring + from, 0, LLONG_MAX, at, (int32_t)c1, 0});
    if (count > c1) ents->push_back(Q3DocPiece{ring, 0, LLONG_MAX, at + c1, (int32_t)(count - c1), 0});
}

void q3_launch_doc_emit_all(const std::vector<Q3DocPiece>& ents, int i16, void* dst, hipStream_t s) {
    for (size_t g0 = 0; g0 < ents.size(); g0 += Q3_DOC_MAX_ENT) {
        Q3DocPiecePack pk{};
        const int n = (int)std::min<size_t>(ents.size() - g0, Q3_DOC_MAX_ENT);
        for (int i = 0; i < n; ++i) pk.e[i] = ents[g0 + i];
        q3_launch_doc_emit(pk, n, i16, dst, s);
    }
}

int q3_doc_rules(const q3tts_doc_opts& o, const int32_t* kinds, int n_segs, bool have_voice, bool have_prefix, int engine_speed, int engine_rate,
                 const char** msg) {
    *msg = nullptr;
    if (engine_speed) { *msg = "document: q3tts_set_speed is set on the engine (a document carries its own speed_permille; q3tts_set_speed(engine, 0) first)"; return Q3TTS_ERR_STATE; }
    if (engine_rate) { *msg = "document: q3tts_set_output_rate is set on the engine (a document carries its own output_rate; q3tts_set_output_rate(engine, 0) first)"; return Q3TTS_ERR_STATE; }
    if (q3_join_opts_rules(o.join, msg) != Q3TTS_OK) return Q3TTS_ERR_INVALID;
    if (o.ahead < 0 || o.ahead > 64) *msg = "document: ahead is 0 (the default, 8) or 1..64";
    else if (o.speed_permille != 0 && (o.speed_permille < Q3_TEMPO_MIN || o.speed_permille > Q3_TEMPO_MAX)) *msg = "document: speed_permille is 0 or 1000 (off), or 500..2000";
    else if (o.output_rate != 0 && (o.output_rate < 4000 || o.output_rate > 96000)) *msg = "document: output_rate is 0 (off) or 4000..96000 Hz";
    else if (o.open != 0 && o.open != 1) *msg = "document: open is 0 or 1";
    else if (n_segs > Q3_JOIN_MAX_SEG || n_segs < (o.open ? 0 : 1)) *msg = "document: n_segs is 1..1024 per call (0 only with open = 1)";
    else if (n_segs > 0 && !kinds) *msg = "document: the segments are missing";
    else if (have_voice == have_prefix) *msg = "document: give exactly one of voice and prefix";
    else for (int i = 0; i < n_segs; ++i) if (kinds[i] < 0 || kinds[i] > 4) *msg = "document: a break kind lies outside 0..4";
    return *msg ? Q3TTS_ERR_INVALID : Q3TTS_OK;
}

extern "C" void q3tts_doc_default_opts(q3tts_doc_opts* o) {
    if (!o) return;
    memset(o, 0, sizeof(*o));
    q3tts_long_opts l;
    q3tts_long_default_opts(&l);
    o->join = l.join;
}

// ---- host-only hooks ----------------------------------------------------------------------------------------------------------
extern "C" int q3tts_k_doc_rules(const q3tts_doc_opts* opts, const int32_t* kinds, int32_t n_segs, int32_t have_voice, int32_t have_prefix,
                                 int32_t engine_speed, int32_t engine_rate, char* msg, int32_t cap) {
    const char* why = "document: opts is NULL";
    const int rc = opts ? q3_doc_rules(*opts, kinds, n_segs, have_voice != 0, have_prefix != 0, engine_speed, engine_rate, &why) : Q3TTS_ERR_INVALID;
    if (msg && cap > 0) { strncpy(msg, rc == Q3TTS_OK ? "" : why, (size_t)cap - 1); msg[cap - 1] = 0; }
    return rc;
}

extern "C" int q3tts_k_doc_plan(const q3tts_join_opts* opts, int32_t rate, const int32_t* segs, int32_t n_segs, int64_t room, int64_t* state,
                                int64_t* pieces, int32_t cap, int32_t* n_pieces, int64_t* done, int32_t done_cap, int32_t* n_done) {
    if (!opts || !segs || !state || !pieces || !n_pieces || !done || !n_done || n_segs < 0 || n_segs > Q3_JOIN_MAX_SEG || room < 0 || rate < 1000 || cap < 0 || done_cap < 0)
        return q3_set_err(nullptr, Q3TTS_ERR_INVALID, "doc plan hook: bad arguments");
    const char* msg = nullptr;
    if (q3_join_opts_rules(*opts, &msg) != Q3TTS_OK) return q3_set_err(nullptr, Q3TTS_ERR_INVALID, msg);
    std::vector<Q3DocSegNow> sn((size_t)n_segs);
    for (int i = 0; i < n_segs; ++i) {
        sn[i] = Q3DocSegNow{segs[5 * i], segs[5 * i + 1], segs[5 * i + 2], segs[5 * i + 3], segs[5 * i + 4]};
        const long long nb = ((long long)sn[i].n + W - 1) / W;
        if (sn[i].n < 0 || sn[i].kind < 0 || sn[i].kind > 4 || (sn[i].last >= 0 && (sn[i].first < 0 || sn[i].first > sn[i].last || sn[i].last >= nb)))
            return q3_set_err(nullptr, Q3TTS_ERR_INVALID, "doc plan hook: a segment's length, kind or edges are out of range");
    }
    Q3DocState st{state[0], state[1], state[2], state[3], state[4], state[5], state[6]};
    if (st.head < 0 || st.head > n_segs || st.e < 0 || st.delivered < 0) return q3_set_err(nullptr, Q3TTS_ERR_INVALID, "doc plan hook: bad state");
    std::vector<Q3DocOut> pc; std::vector<Q3DocDone> dn;
    const int rc = q3_doc_plan(*opts, rate, sn.data(), n_segs, room, &st, &pc, &dn);
    if (rc != Q3TTS_OK) return q3_set_err(nullptr, rc, "document: the delivered length would pass 2^28 samples at segment " + std::to_string(st.head));
    *n_pieces = (int32_t)pc.size(); *n_done = (int32_t)dn.size();
    if ((int)pc.size() > cap || (int)dn.size() > done_cap) return q3_set_err(nullptr, Q3TTS_ERR_INVALID, "doc plan hook: pieces or done is too small (*n_pieces / *n_done say how many)");
    for (size_t i = 0; i < pc.size(); ++i) {
        int64_t* p = pieces + 6 * i;
        p[0] = pc[i].seg; p[1] = pc[i].src; p[2] = pc[i].j0; p[3] = pc[i].count; p[4] = pc[i].L == LLONG_MAX ? -1 : pc[i].L; p[5] = pc[i].F;
    }
    for (size_t i = 0; i < dn.size(); ++i) {
        int64_t* p = done + 5 * i;
        p[0] = dn[i].seg; p[1] = dn[i].lo; p[2] = dn[i].hi; p[3] = dn[i].begin; p[4] = dn[i].end;
    }
    state[0] = st.head; state[1] = st.e; state[2] = st.pause_left; state[3] = st.have_prev; state[4] = st.kmax; state[5] = st.delivered; state[6] = st.begin;
    return Q3TTS_OK;
}

// One boundary of the pipeline's flow control (host only): what q3_doc_ring_room / q3_doc_ring_step say for a join that has `want`
// more samples to hand out (fin_if_all: J is whole once they all are).
extern "C" int q3tts_k_doc_ring_plan(int32_t speed_permille, int32_t rate_in, int32_t rate_out, int64_t ring_j, int64_t ring_t, int64_t* state,
                                     int64_t want, int32_t fin_if_all, int64_t room_out, int64_t* out) {
    if (!state || !out || want < 0 || room_out < 0 || ring_j < 0 || ring_t < 0) return q3_set_err(nullptr, Q3TTS_ERR_INVALID, "doc ring plan hook: bad arguments");
    const int speed = (speed_permille == 0 || speed_permille == 1000) ? 0 : speed_permille;
    if (speed && (speed < Q3_TEMPO_MIN || speed > Q3_TEMPO_MAX)) return q3_set_err(nullptr, Q3TTS_ERR_INVALID, "doc ring plan hook: speed_permille is 0 or 1000 (off), or 500..2000");
    Q3DocRing r{};
    r.speed = speed;
    if (rate_out != 0 && rate_out != rate_in) {
        int L = 0, M = 0, H = 0, T = 0;
        const int rc = q3_resample_plan(rate_in, rate_out, &L, &M, &H, &T);
        if (rc != Q3TTS_OK) return q3_set_err(nullptr, rc, "doc ring plan hook: the rate pair is refused");
        r.L = L; r.M = M; r.H = H;
    }
    if (!r.speed && !r.L) return q3_set_err(nullptr, Q3TTS_ERR_INVALID, "doc ring plan hook: neither a speed nor a rate");
    const long long mj = q3_doc_ring_min_j(r.speed, r.L, r.M, r.H), mt = q3_doc_ring_min_t(r.speed, r.L, r.M, r.H);
    r.cj = ring_j ? ring_j : mj; r.ct = ring_t ? ring_t : mt;
    if (r.cj < mj || r.ct < mt || (r.cj & 3) || (r.ct & 3))
        return q3_set_err(nullptr, Q3TTS_ERR_INVALID, "doc ring plan hook: a ring is below its minimum (" + std::to_string(mj) + ", " + std::to_string(mt) + ") or no multiple of 4");
    r.nj = state[0]; r.fin_j = (int32_t)state[1]; r.kt = state[2]; r.m = state[3];
    if (r.nj < 0 || r.kt < 0 || r.m < 0 || (r.fin_j && want > 0)) return q3_set_err(nullptr, Q3TTS_ERR_INVALID, "doc ring plan hook: bad state (or J is whole and more is to be joined)");
    const long long room = q3_doc_ring_room(r), joined = std::min<long long>(want, room);
    Q3DocRingStep st{};
    q3_doc_ring_step(&r, joined, r.fin_j || (fin_if_all && joined == want), room_out, &st);
    out[0] = room; out[1] = joined; out[2] = st.k_from; out[3] = st.k_to; out[4] = st.nt; out[5] = st.nx; out[6] = st.fin_x; out[7] = st.first;
    out[8] = st.count; out[9] = st.all_out; out[10] = mj; out[11] = mt; out[12] = st.pending;
    state[0] = r.nj; state[1] = r.fin_j; state[2] = r.kt; state[3] = r.m;
    return Q3TTS_OK;
}

// out_begin / out_end of q3tts_session_document_info: a position of J through the document's speed and rate maps (host only)
extern "C" int q3tts_k_doc_out_pos(int64_t pos, int32_t speed_permille, int32_t rate_in, int32_t rate_out, int64_t* out) {
    const int speed = (speed_permille == 0 || speed_permille == 1000) ? 0 : speed_permille;
    if (!out || pos < 0 || pos > (1ll << 40) || (speed && (speed < Q3_TEMPO_MIN || speed > Q3_TEMPO_MAX))) return q3_set_err(nullptr, Q3TTS_ERR_INVALID, "doc out pos hook: bad arguments");
    int L = 0, M = 0, H = 0, T = 0;
    if (rate_out != 0 && rate_out != rate_in) {
        const int rc = q3_resample_plan(rate_in, rate_out, &L, &M, &H, &T);
        if (rc != Q3TTS_OK) return q3_set_err(nullptr, rc, "doc out pos hook: the rate pair is refused");
    }
    *out = q3_doc_out_pos(pos, speed, L, M);
    return Q3TTS_OK;
}

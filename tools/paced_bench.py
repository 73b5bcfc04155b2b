#!/usr/bin/env python3
"""paced_bench.py — how many real-time listeners 64 slots serve with pacing and swapping on one MI355X.

  python tools/paced_bench.py [--listeners 64,256,512,1024] [--slots 64] [--lead 0.5] [--arena-gb 64] [--max-frames 250] [--tiny]

The benchmark's shape (1.7B, synthetic weights, n_ctx 4096, max_steps_cap 512, i16 chunks), one process. Prints one JSON line per N.

For each N: N requests (n_text ~ U{8..64}, forced lengths ~ U{25..max-frames} frames) are submitted at t = 0 through one session of
`slots` slots with a swap arena, every one paced with a credit of 4 frames. Listener i starts to play at its first chunk (t0_i) and
plays 12.5 frames a second; the consumer thread grants each listener 4 more frames whenever its playback clock says that they would be
delivered at most `lead` seconds ahead: credit(t) = floor4((t - t0_i + lead) / frame_s), at least 4 (frame_s = 0.08 s at this shape). Chunk
k of a listener (frames 4k .. 4k + 3) is due at t0_i + 4k * frame_s; one that arrives later is an UNDERRUN. Reported: chunks and underruns (count, worst
lateness), first-chunk latency from t = 0 (p50 / p99), swap-outs, swap-ins, chunk boundaries that ran frame steps (from
q3tts_k_bucket_steps) and swap-outs per such boundary, the arena's peak, the wall time and audio-sec/s — and the same requests
submitted plainly (unpaced, no arena) for their audio-sec/s.

--roundtrip: the cost of a swap by itself. 2 x slots requests of 24 frames with a credit of 8 and no playback clock: every request of
the first half is swapped out once and in once; then all limits are lifted. Against the same requests submitted plainly the extra wall
time per swap-out is the round trip's cost at that K/V size (its bytes are reported). It is a difference of two wall times of a few
hundred milliseconds: an estimate, not a device timing. What a boundary adds on the HOST is reported per N from q3tts_k_swap_phase_ms
(the worker's wall time in swap_out and in swap_in per boundary that moved a block); the copies' device time is not timed separately.

Every request's chunks (CRC-32 of the i16 bytes in order, sample count), codes and hit_eos are compared between the paced and the
unpaced run: `requests_differing_from_unpaced` must be 0 (the contract of include/q3tts.h, here under load and with blocks of many sizes)."""
import argparse
import heapq
import json
import os
import sys
import time
import zlib

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "qwen3-tts-rust_amd"))
SPF, FRAME_S = 1920, 0.08   # samples and seconds per frame: main() takes both from the engine's vocoder config


def _spk(d):
    return ((np.arange(d) % 13 - 6) * 0.03125).astype(np.float32)


def _requests(native, d, n, max_frames, seed=0, fixed=None):
    rng = np.random.default_rng(seed)
    reqs, keep, frames = [], [], []
    for i in range(n):
        desc, k = native.make_prompt_desc(rng.integers(0, 151643, size=int(rng.integers(8, 65))).astype(np.uint32), spk_emb=_spk(d))
        f = fixed or int(rng.integers(25, max_frames + 1))
        reqs.append(dict(desc=desc, temperature=0.7, top_k=40, top_p=0.9, seed=1000 + i, max_steps=min(512, f + 6), min_frames=f, force_eos_at=f))
        keep.append(k); frames.append(f)
    return reqs, keep, frames


def _pct(v, p):
    v = sorted(v)
    return round(v[min(len(v) - 1, int(p / 100.0 * len(v)))], 1) if v else None


def _steps(eng):
    return sum(eng.bucket_steps().values())


class _Sig:
    """Per request, in submission order: (CRC-32 of its chunks' bytes in order, samples, CRC-32 of its codes, hit_eos)."""

    def __init__(self, ids):
        self.ids, self.crc, self.n, self.fin = ids, {r: 0 for r in ids}, {r: 0 for r in ids}, {}

    def add(self, rid, is_chunk, pcm, res):
        if is_chunk:
            self.crc[rid] = zlib.crc32(pcm.tobytes(), self.crc[rid]); self.n[rid] += pcm.size
        else:
            self.fin[rid] = (zlib.crc32(np.ascontiguousarray(res.codes).tobytes()), int(res.hit_eos))

    def out(self):
        return [(self.crc[r], self.n[r]) + self.fin[r] for r in self.ids]


def plain(eng, native, _abi, reqs, frames):
    t0 = time.perf_counter()
    with native.NativeSession(eng, _abi.PCM_I16) as sess:
        ids = [sess.submit(**kw) for kw in reqs]
        sig = _Sig(ids)
        for rid, kind, pcm, fin, res in sess.events(120000):
            assert kind in (_abi.EV_CHUNK, _abi.EV_DONE), kind
            sig.add(rid, kind == _abi.EV_CHUNK, pcm, res)
    wall = time.perf_counter() - t0
    return dict(wall_s=round(wall, 3), audio_sec_per_s=round(sum(frames) * FRAME_S / wall, 1)), sig.out()


def paced(eng, native, _abi, reqs, frames, lead, arena_gb):
    lead_f = lead / FRAME_S
    steps0 = _steps(eng)
    with native.NativeSession(eng, _abi.PCM_I16, swap_mb=arena_gb * 1024) as sess:
        t_sub = time.perf_counter()
        ids = [sess.submit(credit_frames=4, **kw) for kw in reqs]
        need = {r: f + 4 for r, f in zip(ids, frames)}    # the credit that lets the request reach its end
        credit, t0, got, first, late = {r: 4 for r in ids}, {}, {r: 0 for r in ids}, [], []
        sig = _Sig(ids)
        due = []                                          # (time of the next grant, id)
        n_chunks = 0
        while sess.open_ids:
            now = time.perf_counter()
            while due and due[0][0] <= now:
                _, r = heapq.heappop(due)
                if r not in sess.open_ids:
                    continue
                sess.grant(r, 4)
                credit[r] += 4
                if credit[r] < need[r]:
                    heapq.heappush(due, (t0[r] + (credit[r] + 4 - lead_f) * FRAME_S, r))
            wait = 50 if not due else max(0, min(50, int((due[0][0] - time.perf_counter()) * 1000)))
            ev = sess.next(wait)
            if ev is None:
                continue
            rid, kind, pcm, fin, res = ev
            now = time.perf_counter()
            sig.add(rid, kind == _abi.EV_CHUNK, pcm, res)
            if kind == _abi.EV_CHUNK:
                if rid not in t0:
                    t0[rid] = now
                    first.append((now - t_sub) * 1e3)
                    if credit[rid] < need[rid]:
                        heapq.heappush(due, (now + (credit[rid] + 4 - lead_f) * FRAME_S, rid))
                if pcm.size:
                    lateness = now - (t0[rid] + got[rid] * FRAME_S)   # got: frames delivered before this chunk
                    if lateness > 0:
                        late.append(lateness * 1e3)
                    got[rid] += pcm.size // SPF
                    n_chunks += 1
            else:
                assert kind == _abi.EV_DONE, kind
        wall = time.perf_counter() - t_sub
        st = sess.swap_stats()
        ms_out, ms_in, nb = sess.swap_phase_ms()
    bounds = (_steps(eng) - steps0) // 4
    return dict(wall_s=round(wall, 3), audio_sec_per_s=round(sum(frames) * FRAME_S / wall, 1), chunks=n_chunks, underruns=len(late),
                worst_late_ms=round(max(late), 1) if late else 0.0, first_chunk_ms_p50=_pct(first, 50), first_chunk_ms_p99=_pct(first, 99),
                swap_outs=st["swap_outs"], swap_ins=st["swap_ins"], skipped=st["skipped"], boundaries=int(bounds),
                swap_outs_per_boundary=round(st["swap_outs"] / max(1, bounds), 3), arena_peak_mb=round(st["arena_peak"] / 2 ** 20, 1),
                swap_boundaries=nb, host_ms_per_swap_boundary=dict(swap_out=round(ms_out / max(1, nb), 3), swap_in=round(ms_in / max(1, nb), 3))), sig.out()


def roundtrip(eng, native, _abi, slots, arena_gb):
    d = eng.cfg.model.d_embed
    reqs, keep, frames = _requests(native, d, 2 * slots, 0, seed=3, fixed=24)
    base = min(plain(eng, native, _abi, reqs, frames)[0]["wall_s"] for _ in range(3))
    walls, outs, peak = [], 0, 0
    for _ in range(3):
        with native.NativeSession(eng, _abi.PCM_I16, swap_mb=arena_gb * 1024) as sess:
            t = time.perf_counter()
            ids = [sess.submit(credit_frames=8, **kw) for kw in reqs]
            seen = {r: 0 for r in ids}
            while min(seen.values()) < 2:               # everyone has run to its credit: the first half left for the second
                rid, kind, pcm, fin, res = sess.next(120000)
                seen[rid] += kind == _abi.EV_CHUNK
            for r in ids:
                sess.grant(r, -1)
            for _ev in sess.events(120000):
                pass
            walls.append(time.perf_counter() - t)
            st = sess.swap_stats()
            outs, peak = st["swap_outs"], st["arena_peak"]
    extra = min(walls) - base
    return dict(requests=2 * slots, frames=24, plain_wall_s=round(base, 3), swapped_wall_s=round(min(walls), 3), swap_outs=outs,
                block_mb=round(peak / max(1, outs) / 2 ** 20, 2), extra_ms_per_swap_out=round(extra * 1e3 / max(1, outs), 3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--listeners", default="64,256,512,1024")
    ap.add_argument("--slots", type=int, default=64)
    ap.add_argument("--lead", type=float, default=0.5)
    ap.add_argument("--arena-gb", type=float, default=64.0)
    ap.add_argument("--max-frames", type=int, default=250)
    ap.add_argument("--roundtrip", action="store_true")
    ap.add_argument("--tiny", action="store_true", help="the parity tests' small shape (a smoke run of the tool, not a measurement)")
    a = ap.parse_args()
    from q3tts import _abi, native
    cfg = _abi.tiny_config(max_batch=a.slots, n_ctx=1024) if a.tiny else _abi.full_config_py()
    cfg.max_batch, cfg.n_ctx, cfg.max_steps_cap = a.slots, (1024 if a.tiny else 4096), 512
    eng = native.NativeEngine(cfg)
    d = cfg.model.d_embed
    global SPF, FRAME_S
    v = cfg.vocoder
    SPF = int(np.prod([v.upsample_ratios[i] for i in range(v.n_upsample)] + [v.dec_rates[i] for i in range(v.n_dec_blocks)]))
    FRAME_S = SPF / float(v.sample_rate)
    try:
        warm, wk, wf = _requests(native, d, a.slots, 40, seed=9)
        plain(eng, native, _abi, warm, wf)   # graphs and vocoder calls captured before anything is timed
        if a.roundtrip:
            print(json.dumps(dict(roundtrip=roundtrip(eng, native, _abi, a.slots, a.arena_gb))), flush=True)
        for n in [int(x) for x in a.listeners.split(",") if x]:
            reqs, keep, frames = _requests(native, d, n, a.max_frames, seed=n)
            pr, psig = paced(eng, native, _abi, reqs, frames, a.lead, a.arena_gb)
            ur, usig = plain(eng, native, _abi, reqs, frames)
            out = dict(listeners=n, slots=a.slots, lead_s=a.lead, audio_s=round(sum(frames) * FRAME_S, 1), paced=pr, unpaced=ur,
                       requests_differing_from_unpaced=sum(x != y for x, y in zip(psig, usig)))
            print(json.dumps(out), flush=True)
    finally:
        eng.close()


if __name__ == "__main__":
    main()

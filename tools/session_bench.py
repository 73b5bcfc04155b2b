#!/usr/bin/env python3
"""session_bench.py — bench.py's workload through a session (q3tts_session_*) on one MI355X.

  python tools/session_bench.py [--steps K] [--warmup W]

The same 64 seeded lengths, prompts and sampler seeds as bench.py (make_workload, 1.7B shape, temperature 0.7 / top-k 40 / top-p 0.9,
vocoder on). Per step it runs the 64 requests once through q3tts_generate_batch and once through a session (all submitted at once,
every chunk consumed as it arrives), and reports:
  - audio-sec/s of both (the batch figure from the same process, for comparison);
  - first-chunk latency over all session requests (submit -> first chunk ready for the consumer), p50 / p99;
  - late arrivals: with 63 requests decoding, the time from a late submit to its first chunk (a slot is free), and with 64 decoding the
    same for a 65th request (it waits for the first slot to free).
Prints one JSON line.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "qwen3-tts-rust_amd"))

import bench  # noqa: E402  (make_workload, vivian, FRAME_SEC: the benchmark's own workload)


def run_session(eng, reqs):
    """All requests at once; returns (wall seconds, per-request first-chunk ms, frames)."""
    from q3tts import _abi, native
    t0 = time.perf_counter()
    first, frames = [], 0
    with native.NativeSession(eng) as sess:
        for r in reqs:
            sess.submit(**r)
        for rid, kind, pcm, fin, res in sess.events(600000):
            if kind == _abi.EV_DONE:
                first.append(res.first_chunk_ms); frames += res.n_frames
            elif kind != _abi.EV_CHUNK:
                raise RuntimeError(f"request {rid} ended with event kind {kind}")
        if sess._open:
            raise RuntimeError("session events timed out")
    return time.perf_counter() - t0, first, frames


def late_arrival(eng, reqs, n_running):
    """n_running requests decoding (each has delivered a chunk), then one more submit: ms to its first chunk."""
    from q3tts import _abi, native
    with native.NativeSession(eng) as sess:
        ids = {sess.submit(**r) for r in reqs[:n_running]}
        seen = set()
        while seen != ids:
            ev = sess.next(600000)
            if ev is None:
                raise RuntimeError("timed out")
            seen.add(ev[0])
        t0 = time.perf_counter()
        late = sess.submit(**reqs[n_running % len(reqs)])
        while True:
            ev = sess.next(600000)
            if ev is None:
                raise RuntimeError("timed out")
            if ev[0] == late:
                return (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=2)
    ap.add_argument("--warmup", type=int, default=1)
    args = ap.parse_args()
    from q3tts import _abi, native
    cfg = _abi.full_config_py()
    cfg.device, cfg.max_batch, cfg.n_ctx, cfg.max_steps_cap, cfg.with_vocoder = 0, 64, 4096, 512, 1
    eng = native.NativeEngine(cfg)
    keep = []
    reqs, frames = bench.make_workload(64, 0, 1, bench.vivian()[:cfg.model.d_embed], keep, 1)
    audio = sum(frames) * bench.FRAME_SEC
    for _ in range(args.warmup):
        eng.generate_batch(reqs)
        run_session(eng, reqs)
    bt, st, firsts = [], [], []
    for _ in range(args.steps):
        t0 = time.perf_counter()
        outs = eng.generate_batch(reqs)
        bt.append(time.perf_counter() - t0)
        assert all(o.status == 0 for o in outs)
        dt, first, nfr = run_session(eng, reqs)
        assert nfr == sum(frames), (nfr, sum(frames))
        st.append(dt); firsts += first
    late_free = late_arrival(eng, reqs, 63)
    late_full = late_arrival(eng, reqs, 64)
    eng.close()
    f = np.asarray(firsts)
    print(json.dumps({
        "what": "bench.py's 64 utterances (1.7B shape, seeded synthetic weights, vocoder on) per step: q3tts_generate_batch vs one session",
        "audio_sec": round(audio, 2), "steps": args.steps,
        "generate_batch_audio_sec_per_s": round(audio / float(np.median(bt)), 2),
        "session_audio_sec_per_s": round(audio / float(np.median(st)), 2),
        "session_vs_batch": round(float(np.median(bt)) / float(np.median(st)), 4),
        "batch_s": [round(x, 4) for x in bt], "session_s": [round(x, 4) for x in st],
        "first_chunk_ms_p50": round(float(np.percentile(f, 50)), 2), "first_chunk_ms_p99": round(float(np.percentile(f, 99)), 2),
        "late_submit_first_chunk_ms_63_running": round(late_free, 2),
        "late_submit_first_chunk_ms_64_running": round(late_full, 2),
    }))


if __name__ == "__main__":
    main()

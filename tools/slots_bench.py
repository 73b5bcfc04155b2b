#!/usr/bin/env python3
"""slots_bench.py — 256 utterances of bench.py's workload through engines of 64, 128, 192 and 256 slots on one MI355X.

  python tools/slots_bench.py [--slots 64,128,192,256] [--repeats 5] [--warmup 1] [--timeout 600]

The workload is make_workload's (bench.py): 256 utterances over its 64 length classes, 1.7B shape, seeded synthetic weights, temperature
0.7 / top-k 40 / top-p 0.9, vocoder on, n_ctx 1024 (256 slots of 4096 positions do not fit a card: include/q3tts.h). For every slot
count one child process (its own time limit; a failed or hung child ends the run there) creates the engine and measures, `repeats` times:
  - q3tts_generate_batch over the 256 requests: audio-sec/s, the request's first-chunk latency p50 / p99;
  - one session with all 256 submitted at once, every chunk consumed as it arrives: audio-sec/s, first chunk p50 / p99;
and once: the frame step per row bucket (codes only, `bucket` identical requests of 24 frames: every step runs on that bucket), the
batched vocoder call at min(slots, 64), slots/2 and slots slots (q3tts_k_vocoder_bench: above 64 slots a call is several sets of launches,
64 slots each), the device bytes of the engine (q3tts_k_device_bytes). `frame_step_ms` comes from q3tts_get_timings, which reports the last
q3tts_generate_batch call alone. Prints one JSON line per slot count, then one summary line whose ratios are against the 64-slot row (against
the first row, and named so, when 64 is not among --slots).
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "qwen3-tts-rust_amd"))

N_UTT, N_CTX = 256, 1024


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


def spread(xs):
    return round(float(max(xs) - min(xs)), 2)


def child(slots, repeats, warmup):
    import bench  # (make_workload, vivian, FRAME_SEC: the benchmark's own workload)
    from q3tts import _abi, native
    cfg = _abi.full_config_py()
    cfg.device, cfg.max_batch, cfg.n_ctx, cfg.max_steps_cap, cfg.with_vocoder = 0, slots, N_CTX, 512, 1
    t0 = time.perf_counter()
    eng = native.NativeEngine(cfg)
    create_s = time.perf_counter() - t0
    keep = []
    reqs, frames = bench.make_workload(N_UTT, 0, 1, bench.vivian()[:cfg.model.d_embed], keep, 1)
    audio = sum(frames) * bench.FRAME_SEC
    out = {"max_batch": slots, "n_ctx": N_CTX, "utterances": N_UTT, "audio_sec": round(audio, 2), "engine_create_s": round(create_s, 2)}
    out["device_bytes"] = eng.device_bytes()
    for _ in range(warmup):
        eng.generate_batch(reqs)
        run_session(eng, reqs)
    b_rate, s_rate, b_first, s_first, step_ms = [], [], [], [], []
    for _ in range(repeats):
        t0 = time.perf_counter()
        outs = eng.generate_batch(reqs)
        dt = time.perf_counter() - t0
        assert all(o.status == 0 for o in outs) and sum(o.n_frames for o in outs) == sum(frames)
        b_rate.append(audio / dt); b_first += [o.first_chunk_ms for o in outs]
        step_ms.append(eng.timings().frame_step_ms)
        dt, first, nfr = run_session(eng, reqs)
        assert nfr == sum(frames), (nfr, sum(frames))
        s_rate.append(audio / dt); s_first += first
    pct = lambda a, p: round(float(np.percentile(np.asarray(a), p)), 2)   # noqa: E731
    out.update({
        "generate_batch_audio_sec_per_s": round(float(np.median(b_rate)), 2), "generate_batch_runs": [round(x, 2) for x in b_rate],
        "generate_batch_spread": spread(b_rate), "generate_batch_first_chunk_ms_p50": pct(b_first, 50), "generate_batch_first_chunk_ms_p99": pct(b_first, 99),
        "generate_batch_frame_step_ms_mean": round(float(np.mean(step_ms)), 3),
        "session_audio_sec_per_s": round(float(np.median(s_rate)), 2), "session_runs": [round(x, 2) for x in s_rate], "session_spread": spread(s_rate),
        "session_first_chunk_ms_p50": pct(s_first, 50), "session_first_chunk_ms_p99": pct(s_first, 99),
    })
    # the frame step per bucket: `bucket` identical codes-only requests of 24 frames keep every step on that bucket
    per_bucket = {}
    for b in native.row_buckets(slots):
        if b < 16:
            continue
        rs = [dict(reqs[i % N_UTT], max_steps=24, min_frames=24, force_eos_at=24, want_pcm=0) for i in range(b)]
        eng.generate_batch(rs)
        eng.generate_batch(rs)
        tm = eng.timings()
        assert abs(tm.mean_rows - b) < 1e-3, (b, tm.mean_rows)
        per_bucket[str(b)] = round(tm.frame_step_ms, 3)
    out["frame_step_ms_per_bucket"] = per_bucket
    out["vocoder_call_ms"] = {str(n): round(eng.vocoder_bench(n, 20), 3) for n in sorted({min(slots, 64), max(slots // 2, 1), slots})}
    eng.close()
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--slots", default="64,128,192,256")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--timeout", type=int, default=600, help="seconds per slot count (its own child process)")
    ap.add_argument("--child", type=int, default=0)
    args = ap.parse_args()
    if args.child:
        child(args.child, args.repeats, args.warmup)
        return 0
    rows = []
    for slots in [int(x) for x in args.slots.split(",")]:
        cmd = ["timeout", "-k", "10", str(args.timeout), sys.executable, os.path.abspath(__file__), "--child", str(slots), "--repeats", str(args.repeats),
               "--warmup", str(args.warmup)]
        p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        if p.returncode != 0:   # a fault, an abort or a time limit: nothing more is started on the GPU
            print(json.dumps({"max_batch": slots, "failed": p.returncode}))
            return p.returncode
        line = [l for l in p.stdout.splitlines() if l.startswith("{")][-1]
        print(line, flush=True)
        rows.append(json.loads(line))
    base = ([r for r in rows if r["max_batch"] == 64] or rows[:1])[0]
    vs = "vs_%d_slots" % base["max_batch"]
    print(json.dumps({"what": "256 utterances of bench.py's workload (1.7B shape, vocoder on, n_ctx 1024) per slot count",
                      "summary": [{"max_batch": r["max_batch"], "generate_batch_audio_sec_per_s": r["generate_batch_audio_sec_per_s"],
                                   vs: round(r["generate_batch_audio_sec_per_s"] / base["generate_batch_audio_sec_per_s"], 3),
                                   "session_audio_sec_per_s": r["session_audio_sec_per_s"],
                                   "first_chunk_ms_p50": r["session_first_chunk_ms_p50"], "first_chunk_ms_p99": r["session_first_chunk_ms_p99"],
                                   "device_GB": round(r.get("device_bytes", 0) / 1e9, 2)} for r in rows]}))
    return 0


if __name__ == "__main__":
    sys.exit(main())

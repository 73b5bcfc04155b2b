#!/usr/bin/env python3
"""tempo_bench.py — what a speaking rate costs (q3tts_set_speed) on one MI355X.

  python tools/tempo_bench.py [--steps K] [--warmup W] [--no-session]

From event brackets around repeated launches (q3tts_k_pcm_tempo, iters): the time-stretch launch of a first chunk boundary — 1, 64 and
256 rows, each with one 4-frame step of 7680 samples from an empty row — at 500, 1001 and 2000 per mille (55, 28 and 14 dependent frame
searches per row). Then tools/session_bench.py's workload (bench.py's 64 utterances, 1.7B shape, vocoder on, all submitted to one
session at once) with the speed off and at 1250: audio-sec/s of each (audio seconds are the unstretched ones) and the first-chunk
latency p50 / p99. With the speed off the session's launches are those of a build without the stage.
Prints one JSON line.
"""
import argparse
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "qwen3-tts-rust_amd"))
sys.path.insert(0, os.path.join(REPO, "tools"))


def step_launch_us(rows, permille, n=7680, iters=50):
    """One step of n samples for `rows` rows (ceil(rows / 64) launches): (mean microseconds over iters repetitions, frames per row)."""
    from q3tts import native
    src = np.random.default_rng(0).uniform(-1, 1, (rows, n)).astype(np.float32)
    out, nv, _, ms = native.k_pcm_tempo(src, [[n] * rows], [0] * rows, permille, 2 * n + 512, iters=iters)
    return ms * 1e3, int(nv[0, 0]) // 256


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--no-session", action="store_true")
    args = ap.parse_args()
    out = {"what": "k_pcm_tempo: one 7680-sample step from an empty row; session_bench.py's workload at speed off / 1250"}
    for permille in (500, 1001, 2000):
        for rows in (1, 64, 256):
            us, fr = step_launch_us(rows, permille)
            out[f"step_launch_us_{permille}_{rows}rows"] = round(us, 1)
            out[f"frames_per_row_{permille}"] = fr
    if not args.no_session:
        import bench
        import session_bench
        from q3tts import _abi, native
        cfg = _abi.full_config_py()
        cfg.device, cfg.max_batch, cfg.n_ctx, cfg.max_steps_cap, cfg.with_vocoder = 0, 64, 4096, 512, 1
        eng = native.NativeEngine(cfg)
        keep = []
        reqs, frames = bench.make_workload(64, 0, 1, bench.vivian()[:cfg.model.d_embed], keep, 1)
        audio = sum(frames) * bench.FRAME_SEC
        out["audio_sec"], out["steps"] = round(audio, 2), args.steps
        for speed in (0, 1250, 0):  # off, on, off again: the box's drift shows in the two off runs
            eng.set_speed(speed)
            for _ in range(args.warmup):
                session_bench.run_session(eng, reqs)
            ts, first = [], []
            for _ in range(args.steps):
                dt, f, nfr = session_bench.run_session(eng, reqs)
                assert nfr == sum(frames), (nfr, sum(frames))
                ts.append(dt)
                first += f
            key = ("off" if "session_s_off" not in out else "off_again") if speed == 0 else str(speed)
            out[f"session_audio_sec_per_s_{key}"] = round(audio / float(np.median(ts)), 2)
            out[f"session_s_{key}"] = [round(x, 4) for x in ts]
            out[f"first_chunk_ms_p50_{key}"] = round(float(np.percentile(first, 50)), 2)
            out[f"first_chunk_ms_p99_{key}"] = round(float(np.percentile(first, 99)), 2)
        eng.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()

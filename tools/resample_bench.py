#!/usr/bin/env python3
"""resample_bench.py — what an output sample rate costs a session (q3tts_set_output_rate) on one MI355X.

  python tools/resample_bench.py [--steps K] [--warmup W]

tools/session_bench.py's workload (bench.py's 64 utterances, 1.7B shape, vocoder on, all submitted to one session at once) three ways:
output rate off, 8000 Hz and 48000 Hz. Reports audio-sec/s of each (audio seconds do not depend on the rate) and, from event brackets
around repeated launches (q3tts_k_pcm_resample, iters), the time of the resampling launch of one full chunk boundary: 64 slots, each with
a 4-frame window of new PCM behind 8 frames already delivered (also at 44100 and 11025 Hz, the two table paths with L = 147). With the rate off the session's launches are those of a build without the
resampler, so that figure belongs inside the run-to-run spread of tools/session_bench.py on the same box.
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

import bench  # noqa: E402
import session_bench  # noqa: E402


def boundary_launch_us(rate, fmt, slots=64, spf=1920, iters=200):
    """One boundary's launch: every slot has 12 frames of PCM, 8 of them delivered earlier; mean microseconds over iters launches."""
    from q3tts import native
    L, M, H, _ = native.k_resample_table(24000, rate)
    stride = 512 * spf
    n_before, n_now = 8 * spf, 12 * spf
    src = np.zeros((slots, stride), dtype=np.float32)
    src[:, :n_now] = np.random.default_rng(0).uniform(-1, 1, (slots, n_now)).astype(np.float32)
    d0, d1 = -(-(n_before - H) * L // M), -(-(n_now - H) * L // M)
    entries = [(b, d0, d1 - d0, b * (d1 - d0)) for b in range(slots)]
    _, ms = native.k_pcm_resample(src, [n_now] * slots, [0] * slots, entries, slots * (d1 - d0), 24000, rate, fmt, iters=iters)
    return ms * 1e3, d1 - d0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    args = ap.parse_args()
    from q3tts import _abi, native
    cfg = _abi.full_config_py()
    cfg.device, cfg.max_batch, cfg.n_ctx, cfg.max_steps_cap, cfg.with_vocoder = 0, 64, 4096, 512, 1
    eng = native.NativeEngine(cfg)
    keep = []
    reqs, frames = bench.make_workload(64, 0, 1, bench.vivian()[:cfg.model.d_embed], keep, 1)
    audio = sum(frames) * bench.FRAME_SEC
    out = {"what": "tools/session_bench.py's session workload (64 utterances, 1.7B shape, vocoder on) at output rate off / 8000 / 48000",
           "audio_sec": round(audio, 2), "steps": args.steps}
    for rate in (0, 8000, 48000):
        eng.set_output_rate(rate)
        for _ in range(args.warmup):
            session_bench.run_session(eng, reqs)
        ts = []
        for _ in range(args.steps):
            dt, _, nfr = session_bench.run_session(eng, reqs)
            assert nfr == sum(frames), (nfr, sum(frames))
            ts.append(dt)
        key = "off" if rate == 0 else str(rate)
        out[f"session_audio_sec_per_s_{key}"] = round(audio / float(np.median(ts)), 2)
        out[f"session_s_{key}"] = [round(x, 4) for x in ts]
    eng.set_output_rate(0)
    eng.close()
    for rate in (8000, 48000, 44100, 11025):  # the last two: the table in LDS with L = 147, and the table read through the L2
        for fmt, name in ((0, "f32"), (1, "i16")):
            us, n = boundary_launch_us(rate, fmt)
            out[f"boundary_launch_us_{rate}_{name}"] = round(us, 2)
            out[f"boundary_outputs_per_slot_{rate}"] = n
    print(json.dumps(out))


if __name__ == "__main__":
    main()

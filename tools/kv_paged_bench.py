"""What the page-table lookup costs: bench.py's 64-utterance workload through a contiguous engine and a paged engine
(q3tts_engine_options.kv_pages) of the same build, in one process, the runs alternating (contiguous, paged, contiguous, ...) as
profiles/r07/bench_ab_parent_vs_new.txt alternates two builds. Prints one JSON line: per engine the frame step and the prefill time of
every run (ms; q3tts_get_timings) with their mean and spread (max - min), the device bytes, and whether the two engines' codes are equal.

    python tools/kv_paged_bench.py [--runs 4] [--n-ctx 1024] [--pages 448] [--tiny]
"""
import argparse
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "qwen3-tts-rust_amd"))
sys.path.insert(0, REPO)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=4, help="measured runs per engine (one more, unmeasured, warms each up)")
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--n-ctx", type=int, default=1024)
    ap.add_argument("--pages", type=int, default=0, help="the paged engine's pool (0: batch * ceil((75 + 256) / 64), what the workload can reach)")
    ap.add_argument("--tiny", action="store_true", help="the parity tests' small shape (a smoke run of the tool, not a measurement)")
    args = ap.parse_args()
    import bench
    from q3tts import _abi, native
    cfg = _abi.tiny_config(max_batch=args.batch, n_ctx=args.n_ctx, with_vocoder=0) if args.tiny else _abi.default_config()
    cfg.max_batch, cfg.n_ctx, cfg.max_steps_cap, cfg.with_vocoder = args.batch, args.n_ctx, min(256, args.n_ctx - 1), 0
    pages = args.pages or args.batch * 6   # prompts of <= 75 rows + max_steps 256 = 331 positions = 6 pages
    keep = []
    reqs, _ = bench.make_workload(args.batch, 0, 1, bench.vivian() if not args.tiny else np.zeros(cfg.model.d_embed, np.float32), keep, 0)
    if args.tiny:
        reqs = [dict(r, max_steps=63, min_frames=min(r["min_frames"], 60), force_eos_at=min(r["force_eos_at"], 60)) for r in reqs]
    engines = {"contiguous": native.NativeEngine(cfg), "paged": native.NativeEngine(cfg, kv_pages=pages)}
    out = {k: {"frame_step_ms": [], "prefill_ms": [], "device_bytes": e.device_bytes()} for k, e in engines.items()}
    codes = {}
    for run in range(args.runs + 1):
        for k, e in engines.items():
            res = e.generate_batch(reqs)
            assert all(r.status == 0 for r in res), k
            codes[k] = [r.codes for r in res]
            if run:   # (run 0 warms up)
                tm = e.timings()
                out[k]["frame_step_ms"].append(round(tm.frame_step_ms, 5))
                out[k]["prefill_ms"].append(round(tm.prefill_ms, 4))
    for k in out:
        for f in ("frame_step_ms", "prefill_ms"):
            v = out[k][f]
            out[k][f + "_mean"], out[k][f + "_spread"] = round(float(np.mean(v)), 5), round(float(max(v) - min(v)), 5)
    out["paged"]["kv_pages"] = list(engines["paged"].kv_pages)
    out["codes_equal"] = all(np.array_equal(a, b) for a, b in zip(codes["contiguous"], codes["paged"]))
    out["config"] = {"batch": args.batch, "n_ctx": args.n_ctx, "pages": pages, "runs": args.runs, "tiny": bool(args.tiny)}
    for e in engines.values():
        e.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()

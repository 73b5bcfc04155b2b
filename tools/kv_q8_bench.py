#!/usr/bin/env python3
"""kv_q8_bench.py — what kv_q8_0 = 1 (the Talker's K/V cache as ggml Q8_0 blocks) costs and saves on one MI355X.

  python tools/kv_q8_bench.py [--slots 64,256] [--ctx 200,900] [--frames 24] [--timeout 900]

Full 1.7B shape, seeded synthetic weights, n_ctx = 1024, vocoder off. For every slot count one child process (its own time limit; a failed
or hung child ends the run there) builds the bf16-cache engine, then the Q8_0-cache engine, and runs on each, per context length c:
`max_batch` identical-length sampled requests of c - frames / 2 prompt rows and `frames` forced frames — every frame step runs on all rows
and q3tts_timings' mean_ctx_tokens / mean_rows is about c — twice, reporting the second call's frame_step_ms. Also per engine:
q3tts_k_device_bytes, and the logits of q3tts_k_talker_prefill on one 64-row prompt; the child prints the largest |dlogit| / max |logit|
between the two formats. One JSON line per slot count. Ids with the Q8_0 cache may differ from the bf16 cache's: nothing here is asserted.
"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "qwen3-tts-rust_amd"))

N_CTX = 1024


def child(slots, ctxs, frames):
    from q3tts import _abi, native
    rng = np.random.default_rng(7)
    d = _abi.full_config_py().model.d_embed
    rows = {c: (rng.standard_normal((c - frames // 2, d)) * 0.05).astype(np.float32) for c in ctxs}
    prompt64 = (rng.standard_normal((64, d)) * 0.05).astype(np.float32)
    out = {"max_batch": slots, "n_ctx": N_CTX, "frames": frames}
    logits = {}
    for kv in (0, 1):
        cfg = _abi.full_config_py()
        cfg.device, cfg.max_batch, cfg.n_ctx, cfg.max_steps_cap, cfg.with_vocoder, cfg.kv_q8_0 = 0, slots, N_CTX, 64, 0, kv
        eng = native.NativeEngine(cfg)
        name = "q8_0" if kv else "bf16"
        res = {"device_bytes": eng.device_bytes()}
        _, logits[kv] = eng.talker_prefill(prompt64)
        for c in ctxs:
            reqs = [dict(embd=rows[c], temperature=0.7, top_k=40, top_p=0.9, seed=i, max_steps=frames, min_frames=frames, force_eos_at=frames,
                         want_pcm=0) for i in range(slots)]
            for _ in range(2):
                outs = eng.generate_batch(reqs)
                assert all(o.status == 0 and o.n_frames == frames for o in outs)
            tm = eng.timings()
            res["ctx_%d" % c] = {"frame_step_ms": round(tm.frame_step_ms, 4), "mean_rows": round(tm.mean_rows, 2),
                                 "mean_ctx_per_row": round(tm.mean_ctx_tokens / max(tm.mean_rows, 1e-9), 1)}
        eng.close()
        out[name] = res
    out["device_bytes_saved"] = out["bf16"]["device_bytes"] - out["q8_0"]["device_bytes"]
    out["prefill64_max_dlogit_over_max_logit"] = float(np.abs(logits[1] - logits[0]).max() / np.abs(logits[0]).max())
    for c in ctxs:
        out["q8_0_over_bf16_frame_step_ctx_%d" % c] = round(out["q8_0"]["ctx_%d" % c]["frame_step_ms"] / out["bf16"]["ctx_%d" % c]["frame_step_ms"], 3)
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--slots", default="64,256")
    ap.add_argument("--ctx", default="200,900")
    ap.add_argument("--frames", type=int, default=24)
    ap.add_argument("--timeout", type=int, default=900, help="seconds per slot count (its own child process)")
    ap.add_argument("--child", type=int, default=0)
    args = ap.parse_args()
    ctxs = [int(x) for x in args.ctx.split(",")]
    if args.child:
        child(args.child, ctxs, args.frames)
        return 0
    for slots in [int(x) for x in args.slots.split(",")]:
        cmd = ["timeout", "-k", "10", str(args.timeout), sys.executable, os.path.abspath(__file__), "--child", str(slots), "--ctx", args.ctx,
               "--frames", str(args.frames)]
        p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        if p.returncode != 0:   # a fault, an abort or a time limit: nothing more is started on the GPU
            print(json.dumps({"max_batch": slots, "failed": p.returncode}))
            return p.returncode
        print([l for l in p.stdout.splitlines() if l.startswith("{")][-1], flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())

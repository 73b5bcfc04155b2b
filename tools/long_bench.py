#!/usr/bin/env python3
"""long_bench.py — what a long document costs (q3tts_generate_long) on one MI355X.

  python tools/long_bench.py [--steps K] [--warmup W] [--segments N]

The 1.7B shape with 64 slots and the vocoder on. The document has 256 segments in one voice (a prefix made once, outside the timing):
bench.py's utterance mix four times over (its text lengths and frame counts by length class; the lengths are set through each segment's
max_steps with EOS masked, since a document's template has one force_eos_at for all). Measured in one process, alternating:
  - the wall time of q3tts_generate_long (default join options, no speed, native rate), its join_ms and the document's audio-sec/s;
  - the wall time of q3tts_generate_batch over the same requests with want_pcm = 1 (N host copies, no join), code this stage does not touch;
  - the device bytes of the segments' rows and of the document row;
  - the two kernels alone, from event brackets around repeated launches over 64 rows of 250 frames.
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--segments", type=int, default=256)
    args = ap.parse_args()
    import bench
    from q3tts import _abi, native
    cfg = _abi.full_config_py()
    cfg.device, cfg.max_batch, cfg.n_ctx, cfg.max_steps_cap, cfg.with_vocoder = 0, 64, 4096, 512, 1
    eng = native.NativeEngine(cfg)
    spk = bench.vivian()[:cfg.model.d_embed]
    keep = []
    bench.make_workload(args.segments, 0, 1, spk, keep, 1)
    meta = bench.make_workload.meta   # (index, ids, target frames, seed)
    vdesc, vkeep = native.make_prompt_desc(None, spk_emb=spk, part="voice")
    px = eng.create_prefix(desc=vdesc)
    sampler = dict(temperature=0.7, top_k=40, top_p=0.9, min_frames=512)
    segs = [(ids, _abi.BREAK_SENTENCE, target) for _, ids, target, _ in meta]
    reqs = []
    for i, (_, ids, target, _) in enumerate(meta):
        desc, k = native.make_prompt_desc(ids, part="text")
        keep.append(k)
        reqs.append(dict(desc=desc, prefix=px, seed=1000 + i, max_steps=target, want_pcm=1, **sampler))
    frames = sum(t for _, _, t, _ in meta)

    def run_long():
        t = time.perf_counter()
        r = eng.generate_long(segs, prefix=px, seed=1000, **sampler)
        return time.perf_counter() - t, r

    def run_batch():
        t = time.perf_counter()
        outs = eng.generate_batch(reqs)
        return time.perf_counter() - t, outs

    for _ in range(args.warmup):
        run_long()
        run_batch()
    tl, tb, tj, tg = [], [], [], []
    for _ in range(args.steps):
        dt, r = run_long()
        assert [f["n_frames"] for f in r.info] == [t for _, _, t, _ in meta]
        tl.append(dt); tj.append(r.join_ms); tg.append(r.generate_ms)
        dt, outs = run_batch()
        assert sum(o.codes.shape[0] for o in outs) == frames
        tb.append(dt)
    spf = r.info[0]["n_native"] // r.info[0]["n_frames"]
    out = {
        "what": "q3tts_generate_long vs q3tts_generate_batch (want_pcm = 1) over the same %d segments, 64 slots, 1.7B shape" % len(segs),
        "segments": len(segs), "frames": frames, "batch_audio_sec": round(frames * bench.FRAME_SEC, 2),
        "document_samples": r.n_samples, "document_sec": round(r.n_samples / 24000.0, 2),
        "long_wall_s": [round(x, 4) for x in tl], "batch_wall_s": [round(x, 4) for x in tb],
        "long_generate_ms": [round(x, 1) for x in tg], "join_ms": [round(x, 3) for x in tj],
        "document_audio_sec_per_s": round(r.n_samples / 24000.0 / float(np.median(tl)), 2),
        "batch_audio_sec_per_s": round(frames * bench.FRAME_SEC / float(np.median(tb)), 2),
        "device_bytes_rows": len(segs) * cfg.max_steps_cap * spf * 4, "device_bytes_document": r.n_samples * 4,
    }
    px.close()
    eng.close()
    # the kernels alone: 64 rows of 250 frames of noise whose first and last 20 ms are quiet
    rows, n = 64, 250 * 1920
    x = np.random.default_rng(0).uniform(-0.5, 0.5, (rows, n)).astype(np.float32)
    x[:, :480] = 0
    x[:, -480:] = 0
    lens = [n] * rows
    edges, ms_e = native.k_pcm_edges(x, lens, 0.01, iters=20)
    _, _, N, ms_j = native.k_pcm_join(x, lens, [3] * rows, edges, rows * (n + 7200), iters=20)
    out.update(kernel_rows=rows, kernel_samples_per_row=n, k_pcm_edges_us=round(ms_e * 1e3, 1), k_pcm_join_us=round(ms_j * 1e3, 1),
               k_pcm_join_gb_per_s=round(8.0 * N / (ms_j * 1e-3) / 1e9, 1))
    print(json.dumps(out))


if __name__ == "__main__":
    main()

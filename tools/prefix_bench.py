#!/usr/bin/env python3
"""prefix_bench.py — voice prefixes (q3tts_prefix_*) against whole prompts on one MI355X.

  python tools/prefix_bench.py [--steps K] [--warmup W] [--frames F]

Full 1.7B shape (seeded synthetic weights, vocoder on), 64 slots. 64 requests in ONE cloned voice: a voice part of 95 rows (63 reference
frames = 5 s at 12.5 Hz, 20 reference-text tokens, a language) and texts of 10-60 tokens, sampled (temperature 0.7, top-k 40, top-p 0.9, seeded),
every request F frames long (force_eos_at). Each is run as a whole prompt and as prefix + text; the codes must agree. Reports for both:
  - q3tts_get_timings().prefill_ms of a generate_batch call and the call's wall time (medians over the steps);
  - first-chunk latency of late submits: 32 requests decoding (each has delivered a chunk), then the other 32 submitted at once; p50 / p99
    of their submit -> first chunk times.
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


def late_first_chunks(eng, reqs, n_running):
    """n_running requests decoding (each has delivered a chunk), then the rest at once: their first-chunk ms."""
    from q3tts import _abi, native
    with native.NativeSession(eng) as sess:
        ids = {sess.submit(**r) for r in reqs[:n_running]}
        seen = set()
        while seen != ids:
            ev = sess.next(600000)
            if ev is None:
                raise RuntimeError("timed out")
            seen.add(ev[0])
        late = {sess.submit(**r) for r in reqs[n_running:]}
        first = []
        for rid, kind, pcm, fin, res in sess.events(600000):
            if kind == _abi.EV_DONE and rid in late:
                first.append(res.first_chunk_ms)
            elif kind not in (_abi.EV_CHUNK, _abi.EV_DONE):
                raise RuntimeError(f"request {rid} ended with event kind {kind}")
        if sess._open:
            raise RuntimeError("session events timed out")
    return first


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--frames", type=int, default=32)
    args = ap.parse_args()
    from q3tts import _abi, native
    cfg = _abi.full_config_py()
    cfg.device, cfg.max_batch, cfg.n_ctx, cfg.max_steps_cap, cfg.with_vocoder = 0, 64, 4096, 512, 1
    eng = native.NativeEngine(cfg)
    rng = np.random.default_rng(2024)
    spk = ((np.arange(cfg.model.d_embed) % 13 - 6) * 0.03125).astype(np.float32)
    voice = dict(spk_emb=spk, lang_id=2055, ref_codes=rng.integers(0, 2048, size=(63, 16)), ref_text_ids=rng.integers(0, 151643, size=20))
    dv, keep = native.make_prompt_desc(None, part="voice", **voice)
    x = eng.create_prefix(desc=dv)
    whole, pref = [], []
    for i in range(64):
        t = rng.integers(0, 151643, size=int(rng.integers(10, 61)))
        dw, kw = native.make_prompt_desc(t, **voice)
        dt, kt = native.make_prompt_desc(t, part="text")
        keep += [dw, kw, dt, kt]
        kws = dict(temperature=0.7, top_k=40, top_p=0.9, seed=7000 + i, max_steps=args.frames + 4, min_frames=args.frames,
                   force_eos_at=args.frames, want_pcm=1)
        whole.append(dict(desc=dw, **kws))
        pref.append(dict(desc=dt, prefix=x, **kws))
    out = {}
    codes = {}
    for name, reqs in (("whole", whole), ("prefix", pref)):
        for _ in range(args.warmup):
            eng.generate_batch(reqs)
        wall, pf = [], []
        for _ in range(args.steps):
            t0 = time.perf_counter()
            res = eng.generate_batch(reqs)
            wall.append((time.perf_counter() - t0) * 1e3)
            pf.append(eng.timings().prefill_ms)
            assert all(r.status == 0 for r in res)
        codes[name] = [r.codes for r in res]
        f = np.asarray(late_first_chunks(eng, reqs, 32))
        out[name] = {"prefill_ms": round(float(np.median(pf)), 3), "generate_batch_ms": round(float(np.median(wall)), 2),
                     "prefill_ms_all": [round(v, 3) for v in pf],
                     "late_first_chunk_ms_p50": round(float(np.percentile(f, 50)), 2),
                     "late_first_chunk_ms_p99": round(float(np.percentile(f, 99)), 2)}
    same = all(np.array_equal(a, b) for a, b in zip(codes["whole"], codes["prefix"]))
    prompt_rows = sum(int(r["desc"].n_text) + 3 for r in pref)
    x.close()
    eng.close()
    print(json.dumps({
        "what": "64 requests in one cloned voice (95-row voice part, texts 10-60 tokens), 1.7B shape, 64 slots, vocoder on: whole prompts "
                "vs voice prefix + text",
        "voice_rows": x.n_rows, "text_rows_total": prompt_rows, "frames_per_request": args.frames, "steps": args.steps,
        "codes_equal": same, "whole": out["whole"], "prefix": out["prefix"],
        "prefill_speedup": round(out["whole"]["prefill_ms"] / max(out["prefix"]["prefill_ms"], 1e-9), 3),
    }))


if __name__ == "__main__":
    main()

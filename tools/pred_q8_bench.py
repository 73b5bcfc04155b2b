#!/usr/bin/env python3
"""pred_q8_bench.py — what predictor_q8_0 = 2 (the Predictor in ggml's Q8_0 x Q8_0 arithmetic) costs per frame step on one MI355X.

  python tools/pred_q8_bench.py [--rows 64] [--frames 48] [--warmup 2] [--repeats 7]

Full 1.7B shape, synthetic weights, codes only (no vocoder), talker_q8_0 = 2, `rows` requests of `frames` frames each so that every
frame step runs on `rows` rows. One process builds both engines (predictor_q8_0 = 0, then 2), and alternates them: `warmup` untimed
batches each, then `repeats` timed ones; the quantity is q3tts_get_timings().frame_step_ms (device events around the captured frame
steps, mean over the batch). Reports the median, minimum and maximum of the repeats per mode, and the Predictor's weight bytes.
Prints one JSON line.
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "qwen3-tts-rust_amd"))


def pred_weight_bytes(m, q8):
    """(layer matrices, heads) of the Predictor in bytes: bf16, or Q8_0 blocks (34 bytes per 32 weights)."""
    nq, nkv = m.p_n_head * m.p_head_dim, m.p_n_kv_head * m.p_head_dim
    layers = m.p_n_layer * ((nq + 2 * nkv) * m.p_d_model + m.p_d_model * nq + 3 * m.p_d_ffn * m.p_d_model)
    heads = (m.n_codebooks - 1) * m.codebook_size * m.p_d_model
    bpw = 34.0 / 32.0 if q8 else 2.0
    return int(layers * bpw), int(heads * bpw)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=64)
    ap.add_argument("--frames", type=int, default=48)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=7)
    a = ap.parse_args()
    from q3tts import native
    engines = {}
    for mode in (0, 2):
        lib_cfg = native._abi.EngineConfig()
        native._abi.load_library().q3tts_default_config(lib_cfg)
        lib_cfg.max_batch, lib_cfg.n_ctx, lib_cfg.max_steps_cap, lib_cfg.with_vocoder = a.rows, 512, a.frames + 1, 0
        lib_cfg.talker_q8_0, lib_cfg.predictor_q8_0 = 2, mode
        engines[mode] = (lib_cfg, native.NativeEngine(lib_cfg))
    d = engines[0][0].model.d_embed
    rng = np.random.default_rng(0)
    reqs = []
    for i in range(a.rows):
        desc, keep = native.make_prompt_desc(rng.integers(0, 151643, size=24), spk_emb=((np.arange(d) % 13 - 6) * 0.03125).astype(np.float32))
        reqs.append(dict(desc=desc, temperature=0.7, top_k=40, top_p=0.9, seed=100 + i, max_steps=a.frames, min_frames=a.frames, force_eos_at=a.frames, _keep=keep))
    reqs = [{k: v for k, v in r.items() if k != "_keep"} for r in reqs]
    ms = {0: [], 2: []}
    for it in range(a.warmup + a.repeats):
        for mode in (0, 2):   # alternate: drift of clocks and temperature falls on both modes alike
            eng = engines[mode][1]
            outs = eng.generate_batch(reqs)
            assert all(o.status == 0 and o.codes.shape[0] == a.frames for o in outs)
            tm = eng.timings()
            if it >= a.warmup:
                ms[mode].append(float(tm.frame_step_ms))
    out = dict(rows=a.rows, frames=a.frames, warmup=a.warmup, repeats=a.repeats, talker_q8_0=2)
    for mode in (0, 2):
        lay, heads = pred_weight_bytes(engines[mode][0].model, mode == 2)
        out["predictor_q8_0=%d" % mode] = dict(frame_step_ms_median=round(statistics.median(ms[mode]), 4), frame_step_ms_min=round(min(ms[mode]), 4),
                                               frame_step_ms_max=round(max(ms[mode]), 4), predictor_layer_bytes=lay, predictor_head_bytes=heads)
        engines[mode][1].close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()

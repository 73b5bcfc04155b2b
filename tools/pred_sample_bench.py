#!/usr/bin/env python3
"""pred_sample_bench.py — what the Predictor sampler and the code-0 repetition penalty cost per frame step on one MI355X.

  python tools/pred_sample_bench.py [--rows 64] [--frames 48] [--warmup 2] [--repeats 7] [--no-check]

Full 1.7B shape, synthetic weights, codes only (no vocoder), `rows` requests of `frames` frames each so that every frame step runs on
`rows` rows. One engine, three states in turn: off (the default frame step: ARGMAX heads, k_pred_next<false>), the Predictor sampler on at
0.9 / 50 / 1.0 (STORE heads, k_pred_next<true>), and the sampler plus a repetition penalty of 1.05. `warmup` untimed batches each, then
`repeats` timed ones, alternating; the quantity is q3tts_get_timings().frame_step_ms (device events around the replayed frame steps, mean
over the batch). Reports the median, minimum and maximum per state. Prints one JSON line.

Before it times anything it asserts, once, that 4 frames of one request at 0.9 / 50 / 1.0 equal the CPU restatement tests/_pred_sample.py
at this shape — the one place the whole full shape is compared (the suite covers the real Predictor shape behind a tiny Talker). The CPU
side takes a while: the full Talker runs on the host. --no-check leaves it out; the JSON line says which ("checked").
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "qwen3-tts-rust_amd"))

STATES = [("off", (0.0, 0, 1.0), 1.0), ("sampler", (0.9, 50, 1.0), 1.0), ("sampler+penalty", (0.9, 50, 1.0), 1.05)]


def check(eng, cfg):
    sys.path.insert(0, os.path.join(REPO, "tests"))
    import _oracle as O
    import _pred_sample as S
    om = O.OracleModel(cfg.model, seed=0, n_ctx=256, n_threads=16)
    pred, pe = S.mats_from_model(om, False, False), S.prompt(om)
    kw = dict(temperature=0.7, top_k=40, top_p=0.9, seed=11, max_steps=4, min_frames=4)
    tr = []
    ref, _ = S.generate(om, pred, pe, pred_sampler=STATES[1][1], trace=tr, **kw)
    diff, n = S.differing(tr)
    assert 4 * diff >= n, (diff, n)
    eng.set_predictor_sampler(*STATES[1][1])
    got = eng.generate(embd=pe, **kw).codes
    assert np.array_equal(got, ref), "full shape: ids differ from the CPU restatement"
    om.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=64)
    ap.add_argument("--frames", type=int, default=48)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--no-check", action="store_true")
    a = ap.parse_args()
    from q3tts import native
    cfg = native._abi.EngineConfig()
    native._abi.load_library().q3tts_default_config(cfg)
    cfg.max_batch, cfg.n_ctx, cfg.max_steps_cap, cfg.with_vocoder = a.rows, 512, a.frames + 1, 0
    eng = native.NativeEngine(cfg)
    if not a.no_check:
        check(eng, cfg)
    d = cfg.model.d_embed
    rng = np.random.default_rng(0)
    reqs, keeps = [], []
    for i in range(a.rows):
        desc, keep = native.make_prompt_desc(rng.integers(0, 151643, size=24), spk_emb=((np.arange(d) % 13 - 6) * 0.03125).astype(np.float32))
        keeps.append(keep)
        reqs.append(dict(desc=desc, temperature=0.7, top_k=40, top_p=0.9, seed=100 + i, max_steps=a.frames, min_frames=a.frames, force_eos_at=a.frames))
    ms = {name: [] for name, _, _ in STATES}
    for it in range(a.warmup + a.repeats):
        for name, ps, pen in STATES:   # alternate: drift of clocks and temperature falls on every state alike
            eng.set_predictor_sampler(*ps)
            eng.set_repetition_penalty(pen)
            outs = eng.generate_batch(reqs)
            assert all(o.status == 0 and o.codes.shape[0] == a.frames for o in outs)
            if it >= a.warmup:
                ms[name].append(float(eng.timings().frame_step_ms))
    out = dict(rows=a.rows, frames=a.frames, warmup=a.warmup, repeats=a.repeats, checked=not a.no_check)
    for name, ps, pen in STATES:
        out[name] = dict(predictor_sampler=list(ps), repetition_penalty=pen, frame_step_ms_median=round(statistics.median(ms[name]), 4),
                         frame_step_ms_min=round(min(ms[name]), 4), frame_step_ms_max=round(max(ms[name]), 4))
    eng.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()

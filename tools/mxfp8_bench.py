#!/usr/bin/env python3
"""mxfp8_bench.py — what talker_mxfp8 (the Talker's block matrices as MXFP8, FP8 x FP8 on the block-scaled MFMA) costs or saves on one
MI355X, beside bf16 and talker_mxfp4.

  python tools/mxfp8_bench.py [--rows 64] [--frames 48] [--warmup 2] [--repeats 7] [--iters 200]

Full 1.7B shape, synthetic weights, codes only (no vocoder), `rows` requests of `frames` frames each so that every frame step runs on
`rows` rows. One process builds the three engines (bf16, talker_mxfp4, talker_mxfp8) and alternates them: `warmup` untimed batches each,
then `repeats` timed ones; the quantity is q3tts_get_timings().frame_step_ms (device events around the captured frame steps, mean over
the batch). Reports per mode the median, minimum and maximum of the repeats, the engine's device bytes and weight formats, and the share
of code-0 ids equal to the bf16 engine's over the same requests (all frames, and the first frame's, which no earlier id has influenced);
then the four block GEMMs at `rows` rows through the kernel hooks, mean of `iters` launches back to back in each of the three forms
(random weights and rows: times, not results). Prints one JSON line.
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "qwen3-tts-rust_amd"))
MODES = ("bf16", "talker_mxfp4", "talker_mxfp8")


def bf16_bits(x):
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def launch_times(native, m, rows, iters):
    """{matrix: {"bf16_us", "mxfp4_us", "mxfp8_us"}} for the Talker's QKV (STORE), O (RESID, timed as STORE), gate/up (SWIGLU) and down GEMMs"""
    nq, nqkv, d, F = m.t_n_head * m.t_head_dim, (m.t_n_head + 2 * m.t_n_kv_head) * m.t_head_dim, m.t_d_model, m.t_d_ffn
    rng = np.random.default_rng(1)
    out = {}
    for name, N, K, epi, norm in (("qkv", nqkv, d, 0, True), ("o", d, nq, 0, False), ("gate_up", 2 * F, d, 2, True), ("down", d, F, 0, False)):
        w = (rng.standard_normal((N, K)) * 0.02).astype(np.float32)
        xb = bf16_bits(rng.standard_normal((rows, K)))
        ssp = np.ones((rows, K // 16), dtype=np.float32) if norm else None
        out[name] = dict(N=N, K=K,
                         bf16_us=round(1e3 * native.k_bgemm(xb, bf16_bits(w), ssp, K, 1e-6, epi, iters=iters)["ms"], 2),
                         mxfp4_us=round(1e3 * native.k_bgemm_mxfp4(xb, w, ssp, K, 1e-6, epi, iters=iters)["ms"], 2),
                         mxfp8_us=round(1e3 * native.k_bgemm_mxfp8(xb, w, ssp, K, 1e-6, epi, iters=iters)["ms"], 2))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=64)
    ap.add_argument("--frames", type=int, default=48)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--iters", type=int, default=200)
    a = ap.parse_args()
    from q3tts import native
    engines = {}
    for mode in MODES:
        cfg = native._abi.EngineConfig()
        native._abi.load_library().q3tts_default_config(cfg)
        cfg.max_batch, cfg.n_ctx, cfg.max_steps_cap, cfg.with_vocoder = a.rows, 512, a.frames + 1, 0
        engines[mode] = native.NativeEngine(cfg, **({} if mode == "bf16" else {mode: True}))
    m = engines["bf16"].cfg.model
    rng = np.random.default_rng(0)
    reqs, keep = [], []   # (keep: the buffers the descriptors point into)
    for i in range(a.rows):
        desc, k = native.make_prompt_desc(rng.integers(0, 151643, size=24), spk_emb=((np.arange(m.d_embed) % 13 - 6) * 0.03125).astype(np.float32))
        keep.append(k)
        reqs.append(dict(desc=desc, temperature=0.7, top_k=40, top_p=0.9, seed=100 + i, max_steps=a.frames, min_frames=a.frames, force_eos_at=a.frames))
    ms, code0 = {mode: [] for mode in MODES}, {}
    for it in range(a.warmup + a.repeats):
        for mode in MODES:   # alternate: drift of clocks and temperature falls on all modes alike
            outs = engines[mode].generate_batch(reqs)
            assert all(o.status == 0 and o.codes.shape[0] == a.frames for o in outs)
            code0[mode] = np.stack([o.codes[:, 0] for o in outs])   # [rows][frames]
            if it >= a.warmup:
                ms[mode].append(float(engines[mode].timings().frame_step_ms))
    out = dict(rows=a.rows, frames=a.frames, warmup=a.warmup, repeats=a.repeats)
    for mode in MODES:
        out[mode] = dict(frame_step_ms_median=round(statistics.median(ms[mode]), 4), frame_step_ms_min=round(min(ms[mode]), 4),
                         frame_step_ms_max=round(max(ms[mode]), 4), device_bytes=engines[mode].device_bytes(),
                         weight_formats=engines[mode].weight_formats,
                         code0_equal_to_bf16_share=round(float(np.mean(code0[mode] == code0["bf16"])), 4),
                         first_frame_code0_equal_to_bf16_share=round(float(np.mean(code0[mode][:, 0] == code0["bf16"][:, 0])), 4))
        engines[mode].close()
    out["launch_us"] = launch_times(native, m, a.rows, a.iters)
    print(json.dumps(out))


if __name__ == "__main__":
    main()

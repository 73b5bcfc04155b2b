#!/usr/bin/env python3
"""text_stream_bench.py — what streamed text input buys and costs on one MI355X.

  python tools/text_stream_bench.py [--rate 20] [--sentences 6] [--tokens 30] [--rows 64] [--frames 48] [--warmup 2] [--repeats 7]

Full 1.7B shape, synthetic weights, one process, two measurements. Prints one JSON line.

1. First-chunk latency. One voice (a voice prefix), `sentences` sentences of `tokens` text ids each, whose ids become available one by
   one at `rate` ids per second, as a language model would emit them; t = 0 is the moment a sentence's first id exists. Streamed: the
   request is submitted at t = 0 with that id, open, and a feeder thread appends each further id when it exists and closes the text after
   the last; the first chunk can run once 5 ids exist. Whole text: the request is submitted when the last id exists, (tokens - 1) / rate
   seconds later, as a caller without text streaming must. For both, the latency is t = 0 -> the first CHUNK event in the consumer's
   hands; for the whole-text form the part behind the submission is reported too (`after_submit_ms`). One sentence at a time through one
   session per sentence; median, minimum and maximum over the sentences.

2. The frame step of the two graph sets. Codes only (no vocoder work in the step), `rows` requests of `frames` frames each so that every
   frame step runs on `rows` rows; the same engine runs the batch with text_stream = 0 (the default sets, captured at create) and with
   text_stream = 1 (the text form's sets: k_pred_last_text in the last pass), alternating, `warmup` untimed batches each and then
   `repeats` timed ones. The quantity is q3tts_get_timings().frame_step_ms (device events around the replayed frame steps).
"""
import argparse
import json
import os
import statistics
import sys
import threading
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "qwen3-tts-rust_amd"))


def _spk(d):
    return ((np.arange(d) % 13 - 6) * 0.03125).astype(np.float32)


def _stats(v):
    return dict(median=round(statistics.median(v), 2), min=round(min(v), 2), max=round(max(v), 2))


def first_chunk(eng, native, a):
    """-> (streamed ms list, whole-text ms list, whole-text ms behind the submission)"""
    from q3tts import _abi
    d = eng.cfg.model.d_embed
    rng = np.random.default_rng(1)
    vdesc, vk = native.make_prompt_desc(None, spk_emb=_spk(d), part="voice")
    kw = dict(temperature=0.7, top_k=40, top_p=0.9, max_steps=a.frames, min_frames=a.frames, force_eos_at=a.frames)   # (no EOS before the text ends)
    gap = 1.0 / a.rate
    streamed, whole, behind = [], [], []

    def first_event(sess):
        while True:
            ev = sess.next(60000)
            assert ev is not None and ev[1] in (_abi.EV_CHUNK, _abi.EV_DONE), ev
            if ev[1] == _abi.EV_CHUNK:
                return time.perf_counter()

    with eng.create_prefix(desc=vdesc) as px:
        for i in range(a.sentences + 1):   # (sentence 0 is a warm-up: the text form's graph sets are captured at its admission)
            ids = rng.integers(0, 151643, size=a.tokens).astype(np.uint32)
            for mode in ("streamed", "whole"):
                with native.NativeSession(eng) as sess:
                    t0 = time.perf_counter()
                    if mode == "streamed":
                        d0, k0 = native.make_prompt_desc(ids[:1], part="text")
                        rid = sess.submit(desc=d0, prefix=px, seed=10 + i, text_stream=True, text_open=True, **kw)

                        def feed():
                            for j in range(1, a.tokens):
                                time.sleep(max(0.0, t0 + j * gap - time.perf_counter()))
                                sess.append_text(rid, ids[j:j + 1], close=j == a.tokens - 1)
                        th = threading.Thread(target=feed)
                        th.start()
                        t1 = first_event(sess)
                        th.join()
                        if i:
                            streamed.append((t1 - t0) * 1e3)
                    else:
                        time.sleep(max(0.0, t0 + (a.tokens - 1) * gap - time.perf_counter()))
                        ts = time.perf_counter()
                        d1, k1 = native.make_prompt_desc(ids, part="text")
                        sess.submit(desc=d1, prefix=px, seed=10 + i, **kw)
                        t1 = first_event(sess)
                        if i:
                            whole.append((t1 - t0) * 1e3); behind.append((t1 - ts) * 1e3)
                    for _ in sess.events(60000):
                        pass
    return streamed, whole, behind


def frame_step(native, a):
    cfg = native._abi.default_config()
    cfg.max_batch, cfg.n_ctx, cfg.max_steps_cap, cfg.with_vocoder = a.rows, 512, a.frames + 1, 0
    eng = native.NativeEngine(cfg)
    d = cfg.model.d_embed
    rng = np.random.default_rng(0)
    reqs, keeps = {"default": [], "text": []}, []
    for i in range(a.rows):
        desc, keep = native.make_prompt_desc(rng.integers(0, 151643, size=a.tokens), spk_emb=_spk(d))
        keeps.append(keep)
        kw = dict(desc=desc, temperature=0.7, top_k=40, top_p=0.9, seed=100 + i, max_steps=a.frames, min_frames=a.frames, force_eos_at=a.frames)
        reqs["default"].append(kw)
        reqs["text"].append(dict(kw, text_stream=True))
    ms = {"default": [], "text": []}
    for it in range(a.warmup + a.repeats):
        for name in ("default", "text"):   # alternate: drift of clocks and temperature falls on both alike
            outs = eng.generate_batch(reqs[name])
            assert all(o.status == 0 and o.codes.shape[0] == a.frames for o in outs)
            if it >= a.warmup:
                ms[name].append(float(eng.timings().frame_step_ms))
    eng.close()
    return {k: dict(frame_step_ms_median=round(statistics.median(v), 4), frame_step_ms_min=round(min(v), 4), frame_step_ms_max=round(max(v), 4))
            for k, v in ms.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rate", type=float, default=20.0, help="text ids per second")
    ap.add_argument("--sentences", type=int, default=6)
    ap.add_argument("--tokens", type=int, default=30)
    ap.add_argument("--rows", type=int, default=64)
    ap.add_argument("--frames", type=int, default=48)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=7)
    a = ap.parse_args()
    from q3tts import native
    out = dict(rate=a.rate, sentences=a.sentences, tokens=a.tokens, rows=a.rows, frames=a.frames, warmup=a.warmup, repeats=a.repeats)
    out["frame_step"] = frame_step(native, a)
    cfg = native._abi.default_config()
    cfg.max_batch, cfg.n_ctx, cfg.max_steps_cap, cfg.with_vocoder = 4, 512, a.frames + 1, 1
    eng = native.NativeEngine(cfg)
    s, w, b = first_chunk(eng, native, a)
    eng.close()
    out["first_chunk_ms"] = dict(streamed=_stats(s), whole_text=_stats(w), whole_text_after_submit=_stats(b))
    print(json.dumps(out))


if __name__ == "__main__":
    main()

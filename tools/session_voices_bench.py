#!/usr/bin/env python3
"""session_voices_bench.py — what voice work inside a running session costs (include/q3tts.h, "voices in a session").

  python tools/session_voices_bench.py [--running N] [--frames F] [--repeats R]

Full 1.7B shape (seeded synthetic weights, vocoder on), 64 slots. N requests in one cloned voice (95-row voice part, texts of 10-60 tokens,
sampled, F frames each) stream through a session; one of them is watched: the arrival times of its chunks give the chunk interval of the
running streams. While they run, in this order, each a few boundaries after the last:
  1. a request in a NEW voice as a plain whole prompt                       -> its first-chunk latency
  2. the same request (another seed-equal copy) submitted keep-voice, and a second request naming the pending prefix
                                                                            -> first-chunk latency of both (1 vs 2: the save launch)
  3. a standalone prefix job for a third voice                              -> the watched interval that holds its PREFIX event
  4. q3tts_session_clone of a 3 s clip, from a second thread                -> the watched intervals that overlap the call, and its wall time
Then the alternative to (2) for the second request: close the session (cutting every live stream), q3tts_prefix_create, reopen, submit — wall
time from the close to that request's first chunk. Medians over R repeats. Prints one JSON line; no threshold is set anywhere.
"""
import argparse
import json
import os
import sys
import threading
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "qwen3-tts-rust_amd"))


def clip(n, seed):
    rng = np.random.default_rng(seed)
    t = np.arange(n, dtype=np.float64) / 24000.0
    ph = 2 * np.pi * np.cumsum(120.0 + 30.0 * np.sin(2 * np.pi * 1.3 * t)) / 24000.0
    return np.clip(sum(np.sin(k * ph) / k for k in range(1, 6)) * 0.2 + rng.standard_normal(n) * 0.02, -1, 1).astype(np.float32)


def voice(cfg, seed):
    rng = np.random.default_rng(seed)
    spk = ((np.arange(cfg.model.d_embed) % 13 - 6) * 0.03125 * (1.0 + 0.125 * (seed % 5))).astype(np.float32)
    return dict(spk_emb=spk, lang_id=2055, ref_codes=rng.integers(0, 2048, size=(63, 16)), ref_text_ids=rng.integers(0, 151643, size=20))


def scenario(eng, native, _abi, running, new_voice, job_voice, a3s, frames):
    """One session; returns the measurements of steps 1-4."""
    keep = []
    text = np.random.default_rng(5).integers(0, 151643, size=30)
    dw, k = native.make_prompt_desc(text, **new_voice); keep.append(k)
    dt, k = native.make_prompt_desc(text, part="text"); keep.append(k)
    dj, k = native.make_prompt_desc(None, part="voice", **job_voice); keep.append(k)
    kw = dict(temperature=0.7, top_k=40, top_p=0.9, seed=77, max_steps=12, min_frames=8, force_eos_at=8)
    out, marks, clone_t = {}, {}, {}
    with native.NativeSession(eng) as sess:
        ids = [sess.submit(**r) for r in running]
        watch, arrivals, n_w = ids[0], [], 0
        who = {}
        th = None

        def do_clone():
            t0 = time.perf_counter()
            sess.clone_voice(a3s)
            clone_t["t0"], clone_t["t1"] = t0, time.perf_counter()

        while sess._open:
            ev = sess.next(600000)
            if ev is None:
                raise RuntimeError("session events timed out")
            rid, kind, pcm, fin, res = ev
            now = time.perf_counter()
            if kind == _abi.EV_PREFIX:
                if res.status != 0:
                    raise RuntimeError(f"prefix entry {rid} failed with {res.status}")
                marks.setdefault(("prefix", rid), now)
            elif kind == _abi.EV_DONE:
                if rid in who:
                    out[who[rid] + "_first_chunk_ms"] = round(res.first_chunk_ms, 3)
            elif kind != _abi.EV_CHUNK:
                raise RuntimeError(f"request {rid} ended with event kind {kind}")
            if kind != _abi.EV_CHUNK or rid != watch:
                continue
            arrivals.append(now)
            n_w += 1
            if n_w == 6:
                who[sess.submit(desc=dw, **kw)] = "plain"; marks["plain"] = now
            elif n_w == 12:
                r1, x = sess.submit(desc=dw, keep_voice=True, **kw)
                who[r1] = "keep_voice"
                who[sess.submit(desc=dt, prefix=x, **kw)] = "second_behind_pending_prefix"
                marks["keep"] = now
            elif n_w == 18:
                jid, xj = sess.create_prefix(desc=dj); marks["job"] = now; marks["job_id"] = jid
            elif n_w == 24:
                th = threading.Thread(target=do_clone); th.start()
        if th is not None:
            th.join()
        if n_w < 30:
            raise RuntimeError("the watched stream ended before every step ran: raise --frames")
        x.close(); xj.close()
    iv = np.diff(np.asarray(arrivals)) * 1e3
    t_pref = marks[("prefix", marks["job_id"])]
    tag = {}
    for i in range(len(iv)):
        a, b = arrivals[i], arrivals[i + 1]
        if a < t_pref <= b:
            tag[i] = "job"
        elif clone_t and a < clone_t["t1"] and b > clone_t["t0"]:
            tag.setdefault(i, "clone")
        elif any(a <= marks[m] < b or (i > 0 and arrivals[i - 1] <= marks[m] < a) for m in ("plain", "keep")):
            tag.setdefault(i, "admit")
    plain = [float(v) for i, v in enumerate(iv) if i not in tag and i >= 2]
    out["interval_ms_without"] = round(float(np.median(plain)), 3)
    out["interval_ms_without_p95"] = round(float(np.percentile(plain, 95)), 3)
    out["interval_ms_with_prefix_job"] = round(float(max(v for i, v in enumerate(iv) if tag.get(i) == "job")), 3)
    cl = [float(v) for i, v in enumerate(iv) if tag.get(i) == "clone"]
    out["interval_ms_with_clone"] = round(max(cl), 3) if cl else None
    out["clone_call_ms"] = round((clone_t["t1"] - clone_t["t0"]) * 1e3, 3) if clone_t else None
    return out


def reopen(eng, native, _abi, running, new_voice):
    """The way without this feature: close (live streams are cut), prefix_create, reopen, submit; ms from the close to the first chunk."""
    keep = []
    text = np.random.default_rng(5).integers(0, 151643, size=30)
    dv, k = native.make_prompt_desc(None, part="voice", **new_voice); keep.append(k)
    dt, k = native.make_prompt_desc(text, part="text"); keep.append(k)
    kw = dict(temperature=0.7, top_k=40, top_p=0.9, seed=77, max_steps=12, min_frames=8, force_eos_at=8)
    sess = native.NativeSession(eng)
    ids = {sess.submit(**r) for r in running}
    seen = set()
    while seen != ids:
        seen.add(sess.next(600000)[0])
    t0 = time.perf_counter()
    sess.close()
    x = eng.create_prefix(desc=dv)
    with native.NativeSession(eng) as s2:
        s2.submit(desc=dt, prefix=x, **kw)
        while s2.next(600000)[1] != _abi.EV_CHUNK:
            pass
        ms = (time.perf_counter() - t0) * 1e3
        for _ in s2.events(600000):
            pass
    x.close()
    return ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--running", type=int, default=56)
    ap.add_argument("--frames", type=int, default=160)
    ap.add_argument("--repeats", type=int, default=3)
    args = ap.parse_args()
    from q3tts import _abi, native
    cfg = _abi.full_config_py()
    cfg.device, cfg.max_batch, cfg.n_ctx, cfg.max_steps_cap, cfg.with_vocoder = 0, 64, 4096, 512, 1
    eng = native.NativeEngine(cfg)
    ccfg = _abi.CloneConfig()
    eng.lib.q3tts_clone_default_config(ccfg)
    eng.clone_init(ccfg)
    rng = np.random.default_rng(2024)
    v0 = voice(cfg, 1)
    keep, running = [], []
    for i in range(args.running):
        d, k = native.make_prompt_desc(rng.integers(0, 151643, size=int(rng.integers(10, 61))), **v0)
        keep += [d, k]
        running.append(dict(desc=d, temperature=0.7, top_k=40, top_p=0.9, seed=7000 + i, max_steps=args.frames + 4, min_frames=args.frames,
                            force_eos_at=args.frames))
    a3s = clip(72000, 11)
    scenario(eng, native, _abi, running, voice(cfg, 2), voice(cfg, 3), a3s, args.frames)   # warm-up: graphs, clone arena, mel tables
    runs = [scenario(eng, native, _abi, running, voice(cfg, 2), voice(cfg, 3), a3s, args.frames) for _ in range(args.repeats)]
    re_ms = [reopen(eng, native, _abi, running, voice(cfg, 2)) for _ in range(args.repeats)]
    eng.close()
    med = {k: (round(float(np.median([r[k] for r in runs])), 3) if runs[0][k] is not None else None) for k in runs[0]}
    print(json.dumps({
        "what": "voice work inside a running session: 1.7B shape, 64 slots, vocoder on, %d streams of %d frames in one cloned voice; a new "
                "voice has a 95-row voice part and 30 text tokens" % (args.running, args.frames),
        "repeats": args.repeats, "median": med, "runs": runs,
        "second_request_by_close_create_reopen_ms": round(float(np.median(re_ms)), 3), "close_create_reopen_ms_all": [round(v, 3) for v in re_ms],
        "live_streams_cut_by_the_close": args.running,
    }))


if __name__ == "__main__":
    main()

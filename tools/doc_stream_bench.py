#!/usr/bin/env python3
"""doc_stream_bench.py — what streaming a long document through a session costs on one MI355X.

  python tools/doc_stream_bench.py [--steps K] [--warmup W] [--segments N] [--aheads 1,8,64] [--speed 1250] [--rate 16000] [--skip-beside]

tools/long_bench.py's document (the 1.7B shape, 64 slots, vocoder on; 256 segments in one voice behind a prefix made once; bench.py's
utterance mix four times over with the lengths set through max_steps, EOS masked). Measured in one process:
  - q3tts_generate_long: wall time = the time to the first audio (the call returns the whole row), audio-sec/s;
  - the same document as a session document at each `ahead`: time from submit to the first chunk, audio-sec/s over the whole document,
    chunks per second of audio, and the bits against q3tts_generate_long's row;
  - tools/session_bench.py's workload (bench.py's 64 requests through one session) alone, and again with the document at the default
    `ahead` submitted first into the same session: the plain requests' audio-sec/s (to their last final event) and first-chunk latencies.
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

import bench  # noqa: E402


def run_document(eng, segs, px, sampler, ahead, plain=(), speed=0, rate=0):
    """The document (and `plain` requests behind it) through one session; speed / rate: the document's own (0: off). Returns a dict of
    times and the document's PCM."""
    from q3tts import _abi, native
    out = dict(first_s=None, chunks=0)
    pcm, firsts, frames = [], [], 0
    t_plain_end = None
    with native.NativeSession(eng) as sess:
        t0 = time.perf_counter()
        did = sess.submit_document(segs, prefix=px, seed=1000, ahead=ahead, speed_permille=speed, output_rate=rate, **sampler) if segs else None
        ids = {sess.submit(**r) for r in plain}
        for rid, kind, chunk, fin, res in sess.events(600000):
            if rid == did:
                if kind == _abi.EV_CHUNK:
                    if out["first_s"] is None and chunk.size:
                        out["first_s"] = time.perf_counter() - t0
                    out["chunks"] += 1
                    pcm.append(chunk)
                elif kind not in (_abi.EV_SEGMENT, _abi.EV_DONE):
                    raise RuntimeError(f"the document ended with event kind {kind}, status {res.status}")
            elif kind == _abi.EV_DONE:
                firsts.append(res.first_chunk_ms); frames += res.n_frames
                ids.discard(rid)
                if not ids:
                    t_plain_end = time.perf_counter() - t0
            elif kind != _abi.EV_CHUNK:
                raise RuntimeError(f"request {rid} ended with event kind {kind}")
        if sess.open_ids:
            raise RuntimeError("session events timed out")
        out["wall_s"] = time.perf_counter() - t0
    out.update(plain_s=t_plain_end, plain_first_ms=firsts, plain_frames=frames)
    return out, (np.concatenate(pcm) if pcm else np.zeros(0, dtype=np.float32))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=2)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--segments", type=int, default=256)
    ap.add_argument("--aheads", default="1,8,64")
    ap.add_argument("--speed", type=int, default=0, help="per mille: adds legs with the document's own speed (and with --rate, both)")
    ap.add_argument("--rate", type=int, default=0, help="Hz: adds legs with the document's own output rate")
    ap.add_argument("--skip-beside", action="store_true", help="leave out the session_bench workload beside the document")
    args = ap.parse_args()
    aheads = [int(a) for a in args.aheads.split(",")]
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
    plain, plain_frames = bench.make_workload(64, 0, 1, spk, keep, 1)
    plain_audio = sum(plain_frames) * bench.FRAME_SEC

    def run_long():
        t = time.perf_counter()
        r = eng.generate_long(segs, prefix=px, seed=1000, **sampler)
        return time.perf_counter() - t, r

    for _ in range(args.warmup):
        run_long()
        run_document(eng, segs, px, sampler, 8)
    tl = []
    for _ in range(args.steps):
        dt, want = run_long()
        tl.append(dt)
    doc_sec = want.n_samples / 24000.0
    out = {
        "what": "a %d-segment document (long_bench.py's) through q3tts_generate_long and as a session document; 64 slots, 1.7B shape" % len(segs),
        "segments": len(segs), "document_sec": round(doc_sec, 2), "steps": args.steps,
        "generate_long": {"first_audio_s": round(float(np.median(tl)), 4), "audio_sec_per_s": round(doc_sec / float(np.median(tl)), 2)},
        "session_document": {},
    }
    for a in aheads:
        first, wall, chunks = [], [], 0
        for _ in range(args.steps):
            r, pcm = run_document(eng, segs, px, sampler, a)
            assert pcm.size == want.n_samples and np.array_equal(pcm.view(np.uint32), want.pcm.view(np.uint32)), "the streamed document differs from generate_long's"
            first.append(r["first_s"]); wall.append(r["wall_s"]); chunks = r["chunks"]
        out["session_document"]["ahead_%d" % a] = {
            "first_audio_s": round(float(np.median(first)), 4), "audio_sec_per_s": round(doc_sec / float(np.median(wall)), 2),
            "chunks_per_audio_sec": round(chunks / doc_sec, 3), "rows_bytes": a * cfg.max_steps_cap * 1920 * 4}
    # the document with its own speed and / or output rate at ahead = 8, against this build's plain document at ahead = 8 measured here
    legs = ([(args.speed, 0)] if args.speed else []) + ([(0, args.rate)] if args.rate else []) + ([(args.speed, args.rate)] if args.speed and args.rate else [])
    if legs:
        base = [run_document(eng, segs, px, sampler, 8)[0] for _ in range(args.steps)]
        base_wall, base_chunks = float(np.median([b["wall_s"] for b in base])), base[-1]["chunks"]
        out["session_document_rated"] = {"plain_ahead_8": {"wall_s": round(base_wall, 4), "chunks": base_chunks,
                                                            "spread_s": round(max(b["wall_s"] for b in base) - min(b["wall_s"] for b in base), 4)}}
        for s, r in legs:
            ref = eng.generate_long(segs, prefix=px, seed=1000, speed_permille=s, output_rate=r, **sampler)
            first, wall, chunks = [], [], 0
            for _ in range(args.steps):
                got, pcm = run_document(eng, segs, px, sampler, 8, speed=s, rate=r)
                assert pcm.size == ref.n_samples and np.array_equal(pcm.view(np.uint32), ref.pcm.view(np.uint32)), "the rated document differs from generate_long's"
                first.append(got["first_s"]); wall.append(got["wall_s"]); chunks = got["chunks"]
            w = float(np.median(wall))
            out["session_document_rated"]["speed_%d_rate_%d" % (s, r)] = {
                "first_audio_s": round(float(np.median(first)), 4), "wall_s": round(w, 4), "source_audio_sec_per_s": round(doc_sec / w, 2),
                "out_samples": int(ref.n_samples), "out_rate": int(ref.sample_rate), "chunks": chunks,
                "added_ms_per_chunk_boundary": round(1e3 * (w - base_wall) / max(chunks, 1), 4)}
    if args.skip_beside:
        px.close()
        eng.close()
        print(json.dumps(out))
        return
    alone, beside, doc_beside = [], [], []
    f_alone, f_beside = [], []
    for _ in range(args.steps):
        r, _ = run_document(eng, [], px, sampler, 8, plain)
        alone.append(r["plain_s"]); f_alone += r["plain_first_ms"]
        r, pcm = run_document(eng, segs, px, sampler, 8, plain)
        assert np.array_equal(pcm.view(np.uint32), want.pcm.view(np.uint32))
        beside.append(r["plain_s"]); f_beside += r["plain_first_ms"]; doc_beside.append(r["wall_s"])
    out["beside_session_bench_workload"] = {
        "plain_audio_sec": round(plain_audio, 2),
        "plain_alone_audio_sec_per_s": round(plain_audio / float(np.median(alone)), 2),
        "plain_beside_document_audio_sec_per_s": round(plain_audio / float(np.median(beside)), 2),
        "both_audio_sec_per_s": round((plain_audio + doc_sec) / float(np.median(doc_beside)), 2),
        "plain_first_chunk_ms_p50_alone": round(float(np.percentile(f_alone, 50)), 2),
        "plain_first_chunk_ms_p50_beside": round(float(np.percentile(f_beside, 50)), 2),
        "plain_first_chunk_ms_p99_beside": round(float(np.percentile(f_beside, 99)), 2),
    }
    px.close()
    eng.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()

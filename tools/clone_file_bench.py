#!/usr/bin/env python3
"""What loading the clone encoders' weights files costs (numbers in profiles/README.md).

Writes a FULL-shape pair qwen3_tts_speaker_encoder.gguf / qwen3_tts_codec_encoder.gguf from the synthetic generator (tests/_clone_file.py;
BF16 matrices by default, --f32 for an F32 container). Then, on a tiny synthetic engine: the host-only check (q3tts_k_clone_load_check: open,
shape, cross-checks, finite values), q3tts_clone_load and, beside it, q3tts_clone_init of the same shape — one untimed call of each first,
then the median of 3, the files in the page cache. Prints the files' sizes and one JSON line.

    python tools/clone_file_bench.py [--dir DIR] [--f32]
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "qwen3-tts-rust_amd"))
sys.path.insert(0, os.path.join(REPO, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dir", default=None, help="where the pair is written (default: a temporary directory)")
    ap.add_argument("--f32", action="store_true", help="F32 containers instead of BF16 matrices")
    a = ap.parse_args()
    import _clone_file as CF
    from q3tts import _abi, native

    root = a.dir or tempfile.mkdtemp(prefix="clone_file_bench_")
    c = _abi.full_clone_config_py()
    t0 = time.perf_counter()
    paths = CF.write(root, root, c, 0, "f32" if a.f32 else "bf16")
    sizes = [os.path.getsize(p) for p in paths]
    print(f"wrote {paths[0]} ({sizes[0]} bytes) and {paths[1]} ({sizes[1]} bytes) in {time.perf_counter() - t0:.1f} s", flush=True)
    for p in paths:   # into the page cache
        with open(p, "rb") as f:
            while f.read(1 << 24):
                pass

    def timed(fn):
        fn()
        ts = []
        for _ in range(3):
            t = time.perf_counter()
            fn()
            ts.append(time.perf_counter() - t)
        return ts

    def check():
        rc, msg = native.k_clone_load_check(root)
        assert rc == 0, msg

    host = timed(check)
    print(f"host check: {', '.join('%.3f' % t for t in host)} s", flush=True)
    eng = native.NativeEngine(_abi.tiny_config(max_batch=1, n_ctx=128, with_vocoder=0))
    try:
        load = timed(lambda: eng._check(eng.lib.q3tts_clone_load(eng.h, os.fsencode(root)), "q3tts_clone_load"))   # (the C call alone)
        assert eng.clone_source == 2
        print(f"q3tts_clone_load: {', '.join('%.3f' % t for t in load)} s", flush=True)
        init = timed(lambda: eng.clone_init(c))
        assert eng.clone_source == 1
        print(f"q3tts_clone_init: {', '.join('%.3f' % t for t in init)} s", flush=True)
    finally:
        eng.close()
    print(json.dumps({"file_bytes": sum(sizes), "speaker_file_bytes": sizes[0], "codec_file_bytes": sizes[1], "container": "f32" if a.f32 else "bf16",
                      "host_check_s": round(statistics.median(host), 3), "clone_load_s": round(statistics.median(load), 3),
                      "clone_init_s": round(statistics.median(init), 3)}))


if __name__ == "__main__":
    main()

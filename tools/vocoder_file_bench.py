#!/usr/bin/env python3
"""What loading the vocoder's weights file costs at engine creation (numbers in profiles/README.md).

Writes a FULL-shape qwen3_tts_vocoder.gguf from the synthetic generator (tests/_voc_file.py; BF16 matrices by default, --f32 for an F32
container) beside a tiny synthetic Talker / Predictor / assets directory, so that the vocoder dominates the create. Then times
q3tts_engine_create on that directory with the file and on the same model files without it (seeded synthetic vocoder of the same shape):
one untimed create first, then the median of 3 each, the file in the page cache. Prints the file's size, the host-only check
(q3tts_vocoder_config_from_file) and one JSON line.

    python tools/vocoder_file_bench.py [--dir DIR] [--f32]
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
    ap.add_argument("--dir", default=None, help="where the model directories are written (default: a temporary directory)")
    ap.add_argument("--f32", action="store_true", help="an F32 container instead of BF16 matrices")
    a = ap.parse_args()
    import _model_dir as MD
    import _oracle as O
    import _voc_file as VF
    from q3tts import _abi, native

    root = a.dir or tempfile.mkdtemp(prefix="voc_file_bench_")
    vc = _abi.VocoderConfig.from_buffer_copy(_abi.default_config().vocoder)
    dirs = {}
    for name in ("with_file", "without_file"):
        dirs[name] = os.path.join(root, name)
        MD.write_dir(os.path.join(dirs[name], "gguf"), MD.shape_tiny(text_vocab=1024), seed=0)
    t0 = time.perf_counter()
    path = VF.write(os.path.join(dirs["with_file"], VF.FILE), O, vc, 0, "f32" if a.f32 else "bf16")
    size = os.path.getsize(path)
    print(f"wrote {path}: {size} bytes ({size / 2 ** 20:.0f} MiB) in {time.perf_counter() - t0:.1f} s", flush=True)
    t0 = time.perf_counter()
    with open(path, "rb") as f:   # into the page cache, and what reading it costs from there
        while f.read(1 << 24):
            pass
    read_s = time.perf_counter() - t0
    t0 = time.perf_counter()
    native.vocoder_config_from_file(path)
    shape_s = time.perf_counter() - t0

    def create(name):
        base = _abi.tiny_config(max_batch=1, n_ctx=256, with_vocoder=1)
        base.vocoder = vc
        cfg = native.config_from_model_dir(dirs[name], None, base=base)
        t = time.perf_counter()
        eng = native.NativeEngine(cfg)
        dt = time.perf_counter() - t
        src = eng.vocoder_source
        eng.close()
        return dt, src

    create("without_file")   # HIP initialisation, code object load
    res = {}
    for name, want in (("without_file", 1), ("with_file", 2)):
        ts = []
        for _ in range(3):
            dt, src = create(name)
            assert src == want, (name, src)
            ts.append(dt)
        res[name] = ts
        print(f"{name}: q3tts_engine_create {', '.join('%.3f' % t for t in ts)} s", flush=True)
    out = {"file_bytes": size, "container": "f32" if a.f32 else "bf16", "read_cached_s": round(read_s, 3), "config_from_file_s": round(shape_s, 3),
           "create_with_file_s": round(statistics.median(res["with_file"]), 3), "create_without_file_s": round(statistics.median(res["without_file"]), 3)}
    out["extra_s"] = round(out["create_with_file_s"] - out["create_without_file_s"], 3)
    print(json.dumps(out))


if __name__ == "__main__":
    main()

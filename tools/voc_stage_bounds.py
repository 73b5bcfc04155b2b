"""Measures the table VOC_STAGE_R of tests/_oracle.py on the CPU: per vocoder shape and stage kind, the worst normalised error of the CPU
restatement (tests/_voc_ref.py restatement_R) against float64, on the bf16-input oracle's own activations. No GPU, no device output.

    python tools/voc_stage_bounds.py            # tiny, narrow and full shapes; prints the table"""
import ctypes as C
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, os.path.join(REPO, "qwen3-tts-rust_amd"))
import _oracle as O  # noqa: E402
import _voc_ref as VR  # noqa: E402
from q3tts import _abi  # noqa: E402


def shapes():
    tiny = _abi.tiny_config(max_batch=1, n_ctx=128, with_vocoder=1).vocoder
    narrow = _abi.tiny_config(max_batch=1, n_ctx=128, with_vocoder=1).vocoder
    narrow.decoder_dim, narrow.n_dec_blocks = 768, 3
    for i, r in enumerate((8, 5, 3)):
        narrow.dec_rates[i] = r
    return {"tiny": tiny, "narrow": narrow, "full": _abi.full_config_py().vocoder}


if __name__ == "__main__":
    L = VR.bind(O.lib())
    for name, vc in shapes().items():
        v = L.q3o_vocoder_create(C.byref(vc), 0, 8)
        W = VR.Weights(L, v, vc)
        R = {}
        for seed, repeat in ((1, False), (2, True)):
            codes = np.random.default_rng(seed).integers(0, vc.codebook_size, size=(4, 16)).astype(np.int32)
            if repeat:
                codes[:] = codes[0]
            for k, val in VR.restatement_R(W, codes).items():
                R[k] = max(R.get(k, 0.0), val)
        L.q3o_vocoder_destroy(v)
        print(f'    "{name}": {{' + ", ".join(f'"{k}": {val:.2e}' for k, val in sorted(R.items())) + "},", flush=True)

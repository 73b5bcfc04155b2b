"""Measures the table VOC_STAGE_R of tests/_oracle.py on the CPU: per vocoder shape and stage kind, the worst normalised error of the CPU
restatement (tests/_voc_ref.py restatement_R for the convolution half, tests/_voc_tfm_ref.py restatement_R for the front half) against
float64, on the bf16-input oracle's own activations. No GPU, no device output.

    python tools/voc_stage_bounds.py            # prints the table: tiny, narrow and full carry both halves, the other shapes the front half
    python tools/voc_stage_bounds.py tfm        # the front half's entries only (seconds to a minute per shape)"""
import ctypes as C
import math
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, os.path.join(REPO, "qwen3-tts-rust_amd"))
import _oracle as O  # noqa: E402
import _voc_ref as VR  # noqa: E402
import _voc_tfm_ref as TR  # noqa: E402
from q3tts import _abi  # noqa: E402


def up3(x):
    """x rounded up to three significant digits."""
    if x <= 0.0:
        return 0.0
    q = 10.0 ** (math.floor(math.log10(x)) - 2)
    return math.ceil(x / q) * q


def shapes():
    tiny = _abi.tiny_config(max_batch=1, n_ctx=128, with_vocoder=1).vocoder
    narrow = _abi.tiny_config(max_batch=1, n_ctx=128, with_vocoder=1).vocoder
    narrow.decoder_dim, narrow.n_dec_blocks = 768, 3
    for i, r in enumerate((8, 5, 3)):
        narrow.dec_rates[i] = r
    out = {"tiny": tiny, "narrow": narrow, "full": _abi.full_config_py().vocoder}
    for name in TR.SHAPES:   # the front half's shapes (tests/test_vocoder_tfm_stages_gpu.py)
        if name not in out:
            out[name] = TR.shape_vocoder(_abi.tiny_config(max_batch=1, n_ctx=128, with_vocoder=1).vocoder, name)
    return out


if __name__ == "__main__":
    L = TR.bind(O.lib())
    tfm_only = sys.argv[1:] == ["tfm"]
    for name, vc in shapes().items():
        if tfm_only and name == "narrow":
            continue
        v = L.q3o_vocoder_create(C.byref(vc), 0, 8)
        W = VR.Weights(L, v, vc)
        R = {}
        for seed, repeat in ((1, False), (2, True)):
            codes = np.random.default_rng(seed).integers(0, vc.codebook_size, size=(4, 16)).astype(np.int32)
            if repeat:
                codes[:] = codes[0]
            if name in ("tiny", "narrow", "full") and not tfm_only:
                for k, val in VR.restatement_R(W, codes).items():
                    R[k] = max(R.get(k, 0.0), val)
            if name == "narrow":   # its front half is the tiny shape's
                continue
            # the front half over every call of a drive that goes past the window and once round the ring
            n = vc.sliding_window + 2 * TR.FCAP + 4
            codes = np.random.default_rng(seed).integers(0, vc.codebook_size, size=(n, 16)).astype(np.int32)
            if repeat:
                codes[:] = codes[0]
            for k, val in TR.restatement_R(W, codes).items():
                R[k] = max(R.get(k, 0.0), val)
        L.q3o_vocoder_destroy(v)
        # (the front half's figures are rounded up to the printed digits: the oracle's own data must pass its own bound)
        print(f'    "{name}": {{' + ", ".join(f'"{k}": {up3(val) if k in TR.R_KINDS else val:.2e}' for k, val in sorted(R.items())) + "},", flush=True)

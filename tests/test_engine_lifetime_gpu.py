"""Engines come and go in one process: q3tts_engine_destroy frees a whole engine, and a failed q3tts_engine_create a half-built one,
through the engine's one list of device allocations.

The test does not read the device's free memory (the machines are shared: that number is not ours). It pins what a wrong teardown
breaks: a double free or a free of a live buffer faults or corrupts the next engine, whose codes would then differ.
"""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

Q3TTS_ERR_INVALID = -1


def _spk(d):
    return ((np.arange(d) % 13 - 6) * 0.03125).astype(np.float32)


def test_engines_created_destroyed_and_half_built_in_one_process(oracle, tmp_path):
    import _model_dir as MD
    from q3tts import _abi, native

    def config():
        cfg = _abi.tiny_config(max_batch=2, n_ctx=64, with_vocoder=0)
        cfg.max_steps_cap = 16
        return cfg

    def utterance():
        cfg = config()
        eng = native.NativeEngine(cfg)
        try:
            desc, keep = oracle.make_prompt_desc(np.arange(900, 905), spk_emb=_spk(cfg.model.d_embed))
            out = eng.generate(desc=desc, temperature=0.7, top_k=40, top_p=0.9, seed=23, max_steps=8, min_frames=8)
        finally:
            eng.close()
        return out

    outs = [utterance() for _ in range(3)]

    # a create that fails late: the Talker and the Predictor's blocks are on the device when the Predictor's last tensor turns out missing
    cfg = config()
    MD.write_dir(str(tmp_path), MD.shape_tiny(), with_text=False, pred_tensors={"output.weight": MD.DROP})
    cfg.weights_path = str(tmp_path).encode()
    lib = _abi.load_library()
    h = C.c_void_p()
    rc = lib.q3tts_engine_create(C.byref(cfg), C.byref(h))
    msg = lib.q3tts_last_error(None).decode()
    assert rc == Q3TTS_ERR_INVALID and not h.value
    assert "qwen3_tts_predictor.gguf: tensor 'output.weight' is missing" in msg

    outs.append(utterance())
    assert all(o.status == 0 for o in outs)
    assert outs[0].codes.shape == (8, cfg.model.n_codebooks)
    assert all(np.array_equal(o.codes, outs[0].codes) for o in outs[1:])

"""tests/_pred_q8.py (the CPU statement of predictor_q8_0 = 2) pinned to the untouched oracle, bit for bit, and the new config field's
place in the ABI. No GPU."""
import ctypes as C

import numpy as np
import pytest

import _oracle as O
import _pred_q8 as P
from q3tts import _abi

CFG = _abi.tiny_config()
SPK = ((np.arange(CFG.model.d_embed) % 13 - 6) * 0.03125).astype(np.float32)


def _prompt(om, n_text=12, first=100):
    desc, _keep = O.make_prompt_desc(np.arange(first, first + n_text), spk_emb=SPK)
    return om.build_prompt(desc)


@pytest.fixture(scope="module", params=[0, 2], ids=["talker_bf16", "talker_q8a8"])
def model(request):
    om = O.OracleModel(CFG.model, seed=0, n_ctx=256, n_threads=4)
    if request.param == 2:
        om.set_talker_q8a8()
    yield om, P.mats_from_model(om, False, False)
    om.close()


@pytest.mark.parametrize("kw", [dict(temperature=0.0), dict(temperature=0.9, seed=7), dict(temperature=0.9, seed=3, min_frames=4, force_eos_at=13)],
                         ids=["greedy", "sampled", "min_frames_force_eos"])
def test_generate_with_bf16_predictor_is_q3o_generate(model, kw):
    om, pred = model
    pe = _prompt(om)
    ref, ref_eos = om.generate(pe, max_steps=14, **kw)
    got, got_eos = P.generate(om, pred, pe, max_steps=14, **kw)
    assert ref.shape[0] >= (13 if "force_eos_at" in kw else 12)
    assert got_eos == ref_eos and np.array_equal(got, ref)


@pytest.mark.parametrize("n_rows", [1, 2, 17])
def test_a8_layers_and_head_on_the_talker_are_q3o_talker_prefill(n_rows):
    om = O.OracleModel(CFG.model, seed=0, n_ctx=256, n_threads=4)
    m = CFG.model
    tm = P.mats_from_model(om, True, True)   # (before the switch: it replaces the oracle's bf16 matrices by their quants)
    om.set_talker_q8a8()
    pe = _prompt(om, n_text=17)[:n_rows]
    assert pe.shape[0] == n_rows
    hid_ref, logits_ref = om.talker_prefill(pe)
    x = P.layers(tm, pe, 0, a8=True, mrope=list(m.t_mrope_sections))
    logits = P.head(tm, x[-1], 0, m.t_vocab, a8=True)
    assert np.array_equal(P.hidden(tm, x[-1]).view(np.uint32), hid_ref.view(np.uint32))
    assert np.array_equal(logits.view(np.uint32), logits_ref.view(np.uint32))
    om.close()


def test_cache_form_of_layers_equals_whole_sequence():
    """Rows fed one by one with the per-layer QKV cache (how generate() drives the Predictor) = the same rows in one call."""
    om = O.OracleModel(CFG.model, seed=0, n_ctx=256, n_threads=4)
    pm = P.mats_from_model(om, False, True)
    rows = (np.random.default_rng(0).standard_normal((4, CFG.model.p_d_model)) * 0.5).astype(np.float32)
    whole = P.layers(pm, rows, 0)
    cache = [[] for _ in range(pm.L)]
    a = P.layers(pm, rows[:2], 0, cache=cache)
    b = P.layers(pm, rows[2:3], 2, cache=cache)
    c = P.layers(pm, rows[3:4], 3, cache=cache)
    assert np.array_equal(np.concatenate([a, b, c]).view(np.uint32), whole.view(np.uint32))
    om.close()


def test_default_config_leaves_predictor_q8_0_off_and_struct_sizes_agree():
    lib = _abi.load_library()
    # the field is the struct's last: poison a buffer one int32 longer than the Python layout; the library must write the field (0) and
    # nothing behind it
    n = C.sizeof(_abi.EngineConfig)
    buf = (C.c_ubyte * (n + 4))(*([0xA5] * (n + 4)))
    lib.q3tts_default_config(C.cast(buf, C.POINTER(_abi.EngineConfig)))
    cfg = _abi.EngineConfig.from_buffer(buf)
    assert _abi.EngineConfig.predictor_q8_0.offset + 4 <= n and n - _abi.EngineConfig.predictor_q8_0.offset <= 8   # last field (+ tail padding)
    assert cfg.predictor_q8_0 == 0 and cfg.talker_q8_0 == 0
    assert bytes(buf[n:]) == b"\xa5" * 4
    assert cfg.model.p_d_model == 1024 and cfg.max_batch == 1
    for c in (_abi.tiny_config(), _abi.full_config_py()):
        assert c.predictor_q8_0 == 0

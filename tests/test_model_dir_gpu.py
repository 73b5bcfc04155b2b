"""An engine opened from the files of a model directory alone computes the oracle's bits.

q3tts_config_from_model_dir fills the model's shape from the GGUFs' metadata and tensor shapes; nobody passes a shape in. The files hold
the synthetic model (tests/_model_dir.py), so the codes must equal the CPU oracle created from the shape the directory was WRITTEN from,
bit for bit — the comparison test_parity_gpu.py::test_engine_from_model_files makes for a weights_path whose shape the caller knows.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

PROMPTS = [(np.arange(900, 905), 11), (np.arange(300, 317), 12), (np.arange(5000, 5041), 13)]   # three lengths, three seeds


def _spk(d):
    return ((np.arange(d) % 13 - 6) * 0.03125).astype(np.float32)


def _default_config(max_batch=4, n_ctx=256, max_steps_cap=64):
    """The default configuration with only the four fields a caller sizes an engine by."""
    from q3tts import _abi
    cfg = _abi.default_config()
    cfg.max_batch, cfg.n_ctx, cfg.max_steps_cap, cfg.with_vocoder = max_batch, n_ctx, max_steps_cap, 0
    return cfg


def _check_against_oracle(oracle, eng, om, d_embed, min_frames=0):
    reqs, want = [], []
    for ids, seed in PROMPTS:
        desc, keep = oracle.make_prompt_desc(ids, spk_emb=_spk(d_embed))
        pe = om.build_prompt(desc)
        assert np.array_equal(eng.build_prompt(desc).view(np.uint32), pe.view(np.uint32))
        kw = dict(temperature=0.7, top_k=40, top_p=0.9, seed=seed, max_steps=6, min_frames=min_frames)
        want.append(om.generate(pe, **kw))
        reqs.append(dict(desc=desc, **kw))
        reqs[-1]["_keep"] = keep
    outs = eng.generate_batch([{k: v for k, v in r.items() if k != "_keep"} for r in reqs])
    for o, (codes, eos) in zip(outs, want):
        assert o.status == 0 and np.array_equal(o.codes, codes) and bool(o.hit_eos) == eos


@pytest.mark.parametrize("shape,with_text", [("tiny", True), ("b", True), ("b", False)])
def test_engine_from_a_directory_nobody_described(oracle, tmp_path, shape, with_text):
    """Two shapes (the second differs in every count, and its head_dim is not embedding_length / head_count), and the second again without
    a text table (text_vocab 0: every text id follows the out-of-range formula, tts_pad is zeros — src/assets_manager.rs:244-249)."""
    import _model_dir as MD
    from q3tts import native
    m = (MD.shape_tiny if shape == "tiny" else MD.shape_b)()
    MD.write_dir(str(tmp_path / "gguf"), m, seed=5, with_text=with_text)
    cfg = _default_config()
    rc, msg, buf = MD.call(tmp_path, None, cfg)
    assert (rc, msg) == (0, "")
    want = MD.file_fields(m)
    if not with_text:
        want["text_vocab"] = 0
    assert MD.file_fields(cfg.model) == want
    eng = native.NativeEngine(cfg)
    om_cfg = MD.shape_tiny() if shape == "tiny" else MD.shape_b()
    if not with_text:
        om_cfg.text_vocab = 0
    om = oracle.OracleModel(om_cfg, seed=5, n_ctx=256, n_threads=8)
    try:
        _check_against_oracle(oracle, eng, om, m.d_embed)
    finally:
        eng.close()
        om.close()


def test_tts_engine_new_opens_a_q8_0_directory_without_a_config(oracle, tmp_path, monkeypatch):
    """TtsEngine.new(model_dir, "q8_0"), no config: the shape comes from gguf_q8_0's files and the api selects talker_q8_0 = 2 (W8A8), so
    the codes equal the oracle's q3o_set_talker_q8a8 mode. The Talker file is Q8_0, the Predictor's BF16 (it keeps bf16 weights)."""
    import _gguf as G
    import _model_dir as MD
    from q3tts import api
    monkeypatch.chdir(tmp_path)
    m = MD.shape_tiny()
    MD.write_dir(str(tmp_path / "gguf_q8_0"), m, seed=0, matrix_type=G.Q8_0, predictor_type=G.BF16)
    eng = api.TtsEngine.new(str(tmp_path), "q8_0")
    om = oracle.OracleModel(MD.shape_tiny(), seed=0, n_ctx=256, n_threads=8)
    om.set_talker_q8a8()
    try:
        assert eng.cfg.talker_q8_0 == 2 and MD.file_fields(eng.cfg.model) == MD.file_fields(m)
        _check_against_oracle(oracle, eng._native, om, m.d_embed, min_frames=6)
    finally:
        eng.close()
        om.close()


def test_a_shape_the_engine_cannot_run_is_refused_by_engine_create(tmp_path):
    """Metadata that is valid but outside the engine's divisibility rules (an FFN of 768 is not a multiple of 512): the config call reports
    the files as they are, and q3tts_engine_create refuses with the message it has always given."""
    import _model_dir as MD
    from q3tts import _abi, native
    m = MD.shape_tiny(text_vocab=1024)
    m.t_d_ffn = 768
    MD.write_dir(str(tmp_path / "gguf"), m)
    cfg = _default_config()
    rc, msg, buf = MD.call(tmp_path, None, cfg)
    assert (rc, msg) == (0, "") and cfg.model.t_d_ffn == 768
    with pytest.raises(_abi.Q3Error, match=r"config check failed: m\.t_d_model % 512 == 0 && m\.p_d_model % 512 == 0 && m\.t_d_ffn % 512 == 0"):
        native.NativeEngine(cfg)

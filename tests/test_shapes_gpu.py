"""Engines of the model shapes q3tts_engine_create admits beside the two every other test runs (tiny 4/2 heads and the full 16/8: both a
GQA ratio of 2, both 16 codebooks), against the CPU oracle built from the same model config, `==` on f32 bits and ids, with the bf16
cache and with kv_q8_0 = 1 (the oracle then has set_talker_kv_q8). Since a model directory's files set the shape, these are shapes a
user can open. What each shape runs that nothing else in tests/ does (q3_run_layers: a decode step fuses q/k prep into the attention
launch only from two query heads per KV head on; the Predictor's pass A has a kernel of its own, and its layer-0 QKV table, only at
ratio 2):
  r1     ratio 1 in both transformers: decode rows through k_qk_prep + k_attend<1, false> (k_qk_prep_kv8 + k_attend_kv8<1, false>), in the
         Predictor on its 64-position per-frame cache with the slot_mod / pos_const row mapping, pass A included;
  r4     ratio 4 in both: k_attend<4, true> (k_attend_kv8<4, true>) as the Talker's decode step, k_attend<4, true> on the Predictor's
         per-frame cache, its pass A through k_qk_prep + k_attend<4, false>, no table;
  t4_p2  ratio 4 with ONE KV head in the Talker beside today's Predictor;
  t2_p1  today's Talker beside a ratio-1 Predictor;
  cb2    n_codebooks = 2: one Predictor pass (pass A alone), k_pred_next's first pass is its last, no table pass;
  cb3    n_codebooks = 3: two passes, one table pass, k_pred_next's first and last pass adjacent.
r1 and r4 also run with talker_q8_0 = 2: there the attention kernels write their output as Q8_0 blocks (att_out1 / att_out2)."""
import numpy as np
import pytest

import _kv_q8 as K
import _pred_sample as S

pytestmark = pytest.mark.gpu

SHAPES = {
    "r1": dict(t_n_head=4, t_n_kv_head=4, p_n_head=4, p_n_kv_head=4),
    "r4": dict(t_n_head=8, t_n_kv_head=2, p_n_head=8, p_n_kv_head=2),
    "t4_p2": dict(t_n_head=4, t_n_kv_head=1, p_n_head=4, p_n_kv_head=2),
    "t2_p1": dict(t_n_head=4, t_n_kv_head=2, p_n_head=4, p_n_kv_head=4),
    "cb2": dict(n_codebooks=2),
    "cb3": dict(n_codebooks=3),
}
RUNS = [(s, kv, 0) for s in SHAPES for kv in (0, 1)] + [(s, kv, 2) for s in ("r1", "r4") for kv in (0, 1)]

# the attention kernel of each of an engine's five kinds of launch, per (transformer's GQA ratio, Q8_0 cache): what q3_run_layers asks the
# launcher for (fused only from ratio 2 on; pass A fused only at ratio 2; the Predictor's cache is bf16 and 64 positions long)
TALKER = {(1, 0): ("k_attend<1, false>", "k_attend<1, false>"), (2, 0): ("k_attend<2, false>", "k_attend_gqa2"), (4, 0): ("k_attend<4, false>", "k_attend<4, true>"),
          (1, 1): ("k_attend_kv8<1, false>", "k_attend_kv8<1, false>"), (2, 1): ("k_attend_kv8<2, false>", "k_attend_gqa2_kv8"),
          (4, 1): ("k_attend_kv8<4, false>", "k_attend_kv8<4, true>")}           # (a prompt run, a decode step)
PREDICTOR = {1: ("k_attend<1, false>", "k_attend<1, false>"), 2: ("k_attend_pair", "k_attend_small<2>"), 4: ("k_attend<4, false>", "k_attend<4, true>")}  # (pass A, a later pass)


def _cfg(shape, kv=0, talker_q8=0):
    from q3tts import _abi
    cfg = _abi.tiny_config(max_batch=4, n_ctx=256, with_vocoder=0)
    for k, v in SHAPES[shape].items():
        setattr(cfg.model, k, v)
    cfg.kv_q8_0, cfg.talker_q8_0 = kv, talker_q8
    return cfg


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def engine_kernels(native, m, kv, prompt_rows=70, n_ctx=256):
    """The attention kernels an engine of model m launches, by asking the launcher's own rule (q3tts_k_attend_pick / _pick_kv8, host
    only) with the arguments q3_run_layers gives it: Talker prompt run, Talker decode step, Predictor pass A, Predictor later pass."""
    rt, rp = m.t_n_head // m.t_n_kv_head, m.p_n_head // m.p_n_kv_head
    tpick = (lambda **kw: native.k_attend_pick_kv8(**kw)) if kv else native.k_attend_pick
    return dict(
        t_prompt=tpick(fused=0, gqa_ratio=rt, n_ctx=n_ctx, n_kv_head=m.t_n_kv_head, n_seg=1, seg_max_n=prompt_rows, seg_max_t=prompt_rows),
        t_decode=tpick(fused=1 if rt >= 2 else 0, gqa_ratio=rt, n_ctx=n_ctx, n_kv_head=m.t_n_kv_head),
        p_pass_a=native.k_attend_pick(fused=2 if rp == 2 else 0, gqa_ratio=rp, n_ctx=64, n_kv_head=m.p_n_kv_head),
        p_later=native.k_attend_pick(fused=1 if rp >= 2 else 0, gqa_ratio=rp, n_ctx=64, n_kv_head=m.p_n_kv_head))


@pytest.mark.parametrize("shape", list(SHAPES))
def test_the_kernels_each_shape_launches(shape):
    """Covers: that the engines below run the kernels the module docstring names — k_attend<1, false> / k_attend_kv8<1, false> on decode
    rows for r1 and for t2_p1's Predictor, k_attend<4, true> / k_attend_kv8<4, true> for r4, no k_attend_pair / k_attend_small<2> for a
    Predictor whose ratio is not 2 — by the launcher's own choice for the launches q3_run_layers makes of such a model; and that the fused
    and the pair launch do not exist at the ratios where q3_run_layers does not ask for them (so a change to its rule is a refused launch
    and a failed engine creation, not another kernel). Prints the kernels per shape and cache."""
    from q3tts import native
    for kv in (0, 1):
        m = _cfg(shape, kv).model
        rt, rp = m.t_n_head // m.t_n_kv_head, m.p_n_head // m.p_n_kv_head
        got = engine_kernels(native, m, kv)
        print(f"{shape} kv_q8_0 = {kv}: " + ", ".join(f"{k} {v}" for k, v in got.items()))
        assert (got["t_prompt"], got["t_decode"]) == TALKER[rt, kv] and (got["p_pass_a"], got["p_later"]) == PREDICTOR[rp], (shape, kv, got)
    for pick in (native.k_attend_pick, native.k_attend_pick_kv8):
        assert pick(fused=1, gqa_ratio=1, n_ctx=256, n_kv_head=4) is None and pick(fused=1, gqa_ratio=1, n_ctx=64, n_kv_head=4) is None
        assert pick(fused=2, gqa_ratio=1, n_ctx=64, n_kv_head=4) is None and pick(fused=2, gqa_ratio=4, n_ctx=64, n_kv_head=2) is None


@pytest.mark.parametrize("shape,kv,talker_q8", RUNS)
def test_engine_of_the_shape_equals_the_oracle(oracle, shape, kv, talker_q8):
    """talker_prefill bits of a 70-row prompt; one greedy and one sampled generate of 10 frames; six mixed requests on the four slots, each
    == the oracle alone. With kv_q8_0 = 1 the bf16-cache oracle gives other logits and other sampled ids."""
    from q3tts import native
    cfg = _cfg(shape, kv, talker_q8)
    oms = [oracle.OracleModel(cfg.model, seed=0, n_ctx=256, n_threads=8) for _ in range(2 if kv else 1)]
    eng = None
    try:
        for m in oms:
            if talker_q8 == 2:
                m.set_talker_q8a8()
        om = oms[-1]
        if kv:
            om.set_talker_kv_q8()
        eng = native.NativeEngine(cfg)
        what = (shape, kv, talker_q8)
        pe = K.prompt_rows(oracle, om, 70, 1)
        h_ref, l_ref = om.talker_prefill(pe)
        h, l = eng.talker_prefill(pe)
        assert np.array_equal(_bits(l), _bits(l_ref)) and np.array_equal(_bits(h), _bits(h_ref)), what
        if kv:
            assert not np.array_equal(_bits(l_ref), _bits(oms[0].talker_prefill(pe)[1])), what
        for kw in (K.GREEDY, K.SAMPLED):
            r = dict(embd=pe, seed=4, max_steps=10, min_frames=10, **kw)
            ref, eos = om.generate(pe, **K.oracle_kw(r))
            got = eng.generate(**r)
            assert ref.shape == (10, cfg.model.n_codebooks), what
            if kw is K.SAMPLED:   # (varied frames: a model that repeats one frame, as the greedy cb2 does, tests little)
                assert len(np.unique(ref)) > 8 and len(np.unique(ref[:, 0])) > 5, what
            assert got.status == 0 and np.array_equal(got.codes, ref) and got.hit_eos == eos, what + (kw["temperature"],)
            if kv and kw is K.SAMPLED:
                assert not np.array_equal(ref, oms[0].generate(pe, **K.oracle_kw(r))[0]), what
        reqs = K.batch_requests(oracle, om, 6, lo=20, hi=90, frames=(3, 8), seed=50)
        for i, (g, r) in enumerate(zip(eng.generate_batch(reqs), reqs)):
            ref, eos = om.generate(r["embd"], **K.oracle_kw(r))
            assert g.status == 0 and ref.shape[0] == r["force_eos_at"] and np.array_equal(g.codes, ref) and g.hit_eos == eos, what + (i,)
    finally:
        if eng is not None:
            eng.close()
        for m in oms:
            m.close()


@pytest.mark.parametrize("shape", ["r4", "cb3", "cb2"])
def test_predictor_sampler_on_the_shape(oracle, shape):
    """One sampled Predictor run (set_predictor_sampler; the restatement of tests/_pred_sample.py on the oracle's model) on a Predictor of
    ratio 4 and on one of three codebooks — the sampling form of k_pred_next and the heads that store logits, whose passes the shape
    changes. The restatement with a greedy Predictor equals q3o_generate on this shape, and the sampler changes ids. Also two codebooks:
    there the synthetic model's greedy Predictor gives one and the same code in every frame, the sampled one does not."""
    from q3tts import native
    cfg = _cfg(shape)
    om = oracle.OracleModel(cfg.model, seed=0, n_ctx=256, n_threads=8)
    eng = None
    try:
        pred = S.mats_from_model(om, False, False)
        pe = K.prompt_rows(oracle, om, 30, 1)
        kw = dict(seed=11, max_steps=8, min_frames=8, **K.SAMPLED)
        greedy, _ = S.generate(om, pred, pe, pred_sampler=(0.0, 0, 1.0), **kw)
        assert np.array_equal(greedy, om.generate(pe, **kw)[0])
        ps = S.PRED_CONFIGS["select"]
        ref, _ = S.generate(om, pred, pe, pred_sampler=ps, **kw)
        assert ref.shape == greedy.shape and not np.array_equal(ref, greedy)
        eng = native.NativeEngine(cfg)
        eng.set_predictor_sampler(*ps)
        got = eng.generate(embd=pe, **kw)
        assert got.status == 0 and np.array_equal(got.codes, ref), shape
        eng.set_predictor_sampler(0.0, 0, 1.0)
        assert np.array_equal(eng.generate(embd=pe, **kw).codes, greedy), shape
    finally:
        if eng is not None:
            eng.close()
        om.close()

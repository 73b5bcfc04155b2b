"""The Q8_0 K/V cache (kv_q8_0) without a device: the checks of tests/_kv_q8.py on a numpy-f32 restatement of the
preparation and the quantiser, planted defects they must reject, the layout's index functions, the launcher's choice
(q3tts_k_attend_pick_kv8), the hooks' argument checks and the configuration field in its three mirrors; and the oracle's own Q8_0 cache
mode (q3o_attention_kv_q8, OracleModel.set_talker_kv_q8) under the same checks, since the device is compared with it bit for bit."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import _attend_ref as A
import _kv_q8 as K
from _oracle import ATT_STAGE2_TOL

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLAIN = [s for s in K.SPECS if s["hook"] != "pair" and not s.get("row_indexed")] + [K.DECODE_LONG]


def _restated(spec, kind, defect=None):
    """Per sequence of (spec, kind): x, and the restatement's cache."""
    Hq, Hkv = spec["heads"]
    xs, qn, kn = K.make_inputs(spec, kind)
    return [(x, K.cache32(x, Hq, Hkv, kn, defect)) for x in xs], qn, kn


def test_restatement_passes_stage1_on_all_cases(oracle):
    """Plain numpy f32 against float64 on every non-pair, non-row-indexed spec x kind (and decode_long): K within the windows and the
    caps, V equal to q3o_quantize_q8_0 bit for bit. Prints the counts the module docstring of tests/_kv_q8.py quotes."""
    total = K.Counts()
    for spec in PLAIN:
        Hq, Hkv = spec["heads"]
        c = K.Counts()
        for kind in K.KINDS:
            seqs, qn, kn = _restated(spec, kind)
            for x, (k_q, k_d, v_q, v_d) in seqs:
                K.check_stage1_k(x, Hq, Hkv, kn, k_q, k_d, c)
                K.check_stage1_v(oracle, x, Hq, Hkv, v_q, v_d)
        c.check_caps(spec["name"])
        for f in ("elems", "near_q", "diff_q", "blocks", "near_d", "diff_d"):
            setattr(total, f, getattr(total, f) + getattr(c, f))
        total.worst_q = max(total.worst_q, c.worst_q)
    print(total.line("numpy-f32 restatement, all cases"))
    total.check_caps("all cases")
    assert total.elems >= 6_247_808 and total.blocks >= 195_244


def test_restatement_passes_stage2():
    """A plain-f32 attention over the restatement's Q8-valued cache against float64 over the same cache: inside ATT_STAGE2_TOL on every
    kind (the bound was measured over bf16-valued caches; x^ is as exactly represented as a bf16 value)."""
    for name in ("decode13", "prefill_a"):
        spec = K.SPEC[name]
        Hq, Hkv = spec["heads"]
        worst = 0.0
        for kind in K.KINDS:
            seqs, qn, kn = _restated(spec, kind)
            for (x, (k_q, k_d, v_q, v_d)), (pos0, n) in zip(seqs, spec["seqs"]):
                tot = pos0 + n
                q = K.prep32(x.reshape(tot, Hq + 2 * Hkv, K.HD)[pos0:, :Hq], qn, pos0 + np.arange(n))
                out = K.attend32(q, K.dequant(k_q, k_d), K.dequant(v_q, v_d), pos0, Hq, Hkv)
                worst = max(worst, K.stage2_error(out, q, k_q, k_d, v_q, v_d, pos0, Hq, Hkv))
        print(f"{name}: plain f32 over the Q8-valued cache vs float64: {worst:.1e} (bound {ATT_STAGE2_TOL:.1e})")
        assert worst <= ATT_STAGE2_TOL


@pytest.mark.parametrize("defect", ["d128", "trunc", "neighbour_scale", "blocks_along_keys", "v_bf16"])
def test_stage1_rejects_a_planted_defect(oracle, defect):
    """d = amax / 128; truncation instead of rounding; the scale of the neighbouring block; blocks along keys instead of dims; V quantised
    after bf16 rounding: stage 1 refuses each."""
    spec = K.SPEC["prefill_a"]
    Hq, Hkv = spec["heads"]
    seqs, qn, kn = _restated(spec, "normal", defect)
    x, (k_q, k_d, v_q, v_d) = seqs[-1]   # the run of 128 rows
    with pytest.raises(AssertionError):
        K.check_stage1_k(x, Hq, Hkv, kn, k_q, k_d, K.Counts())
        K.check_stage1_v(oracle, x, Hq, Hkv, v_q, v_d)
    good = K.cache32(x, Hq, Hkv, kn)
    K.check_stage1_k(x, Hq, Hkv, kn, good[0], good[1], K.Counts())
    K.check_stage1_v(oracle, x, Hq, Hkv, good[2], good[3])


def test_stage2_rejects_an_unquantised_newest_key():
    """A fused kernel that served the newest key and value as the unquantised row: the cache is right, the output is not. Stage 2 refuses
    it on every slot of decode13 (1 .. 64 keys), and accepts the same attention over x^."""
    spec = K.SPEC["decode13"]
    Hq, Hkv = spec["heads"]
    seqs, qn, kn = _restated(spec, "normal")
    for (x, (k_q, k_d, v_q, v_d)), (pos0, n) in zip(seqs, spec["seqs"]):
        tot = pos0 + n
        xr = x.reshape(tot, Hq + 2 * Hkv, K.HD)
        q = K.prep32(xr[pos0:, :Hq], qn, pos0 + np.arange(n))
        kh, vh = K.dequant(k_q, k_d), K.dequant(v_q, v_d)
        assert K.stage2_error(K.attend32(q, kh, vh, pos0, Hq, Hkv), q, k_q, k_d, v_q, v_d, pos0, Hq, Hkv) <= ATT_STAGE2_TOL
        kh[-1], vh[-1] = K.prep32(xr[-1:, Hq:Hq + Hkv], kn, np.array([tot - 1]))[0], xr[-1, Hq + Hkv:]
        assert K.stage2_error(K.attend32(q, kh, vh, pos0, Hq, Hkv), q, k_q, k_d, v_q, v_d, pos0, Hq, Hkv) > ATT_STAGE2_TOL, tot


def test_deblocking_index_functions_round_trip():
    n_ctx = 320
    pos, d = np.meshgrid(np.arange(n_ctx), np.arange(K.HD), indexing="ij")
    off = K.k_off(pos, d)
    assert np.array_equal(np.sort(off.ravel()), np.arange(n_ctx * K.HD))          # a bijection onto the head's bytes
    p2, d2 = K.k_off_inv(off)
    assert np.array_equal(p2, pos) and np.array_equal(d2, d)
    assert off[65, 0] - off[64, 0] == 16 and off[0, 16] - off[0, 0] == 1024 and off[64, 0] == 64 * K.HD   # one key per lane; 1 KiB per chunk; whole blocks
    pos, j = np.meshgrid(np.arange(n_ctx), np.arange(K.NB), indexing="ij")
    idx = K.kd_idx(pos, j)
    assert np.array_equal(np.sort(idx.ravel()), np.arange(n_ctx * K.NB))
    p2, j2 = K.kd_idx_inv(idx)
    assert np.array_equal(p2, pos) and np.array_equal(j2, j)


def test_pick_kv8_follows_the_rule():
    """q3tts_k_attend_pick_kv8 (host only): runs take k_attend_kv8<R, false> whatever the run table and the prefill policy (never 8:
    there is no Q8 k_attend_prefill; never one of the bf16 kernels); one row per slot takes k_attend_gqa2_kv8 (decode policy 1:
    k_attend_kv8<2, true>) or k_attend_kv8<4, true>, also on a cache of 64 positions (no Q8 k_attend_small); pass A, a fused launch with
    one query head per KV head and other ratios are refused. The cases of tests/_kv_q8.py name all six kernels."""
    from q3tts import _abi, native
    lib = _abi.load_library()
    pick = lambda **kw: native.k_attend_pick_kv8(want_code=True, **kw)
    try:
        for dec in (0, 1):
            for pre in (0, 1, 2):
                assert lib.q3tts_k_attend_policy(dec, pre) == 0
                for n_ctx in (64, 128, 4096):
                    for hkv in (1, 2, 8):
                        for R, code in ((1, 9), (2, 10), (4, 11)):
                            assert pick(fused=0, gqa_ratio=R, n_ctx=n_ctx, n_kv_head=hkv) == code
                            assert pick(fused=0, gqa_ratio=R, n_ctx=n_ctx, n_kv_head=hkv, n_seg=200, seg_max_n=100, seg_max_t=100) == code
                        assert pick(fused=1, gqa_ratio=2, n_ctx=n_ctx, n_kv_head=hkv) == (14 if dec == 0 else 12)
                        assert pick(fused=1, gqa_ratio=4, n_ctx=n_ctx, n_kv_head=hkv) == 13
                        assert pick(fused=1, gqa_ratio=1, n_ctx=n_ctx, n_kv_head=hkv) is None
                        assert pick(fused=2, gqa_ratio=2, n_ctx=n_ctx, n_kv_head=hkv) is None
                        assert pick(fused=0, gqa_ratio=3, n_ctx=n_ctx, n_kv_head=hkv) is None
        seen = set()
        for case in K.CASES.values():
            for policy, code in case["variants"]:
                fused = case["spec"]["hook"] == "decode"
                assert lib.q3tts_k_attend_policy(max(policy, 0) if fused else 0, 0 if fused else max(policy, 0)) == 0
                assert pick(**K.pick_args(case)) == code, (case["spec"]["name"], policy)
                seen.add(code)
        assert seen == set(K.KERNELS) and native.ATTEND_KERNELS_KV8 == K.KERNELS
        k = C.c_int32(0)
        assert lib.q3tts_k_attend_pick_kv8(3, 2, 128, 0, 0, 0, 2, C.byref(k)) == -1 and lib.q3tts_k_attend_pick_kv8(1, 2, 128, 0, 0, 0, 2, None) == -1
    finally:
        lib.q3tts_k_attend_policy(0, 0)


def test_hooks_refuse_bad_arguments_on_the_host():
    """head_dim != 128, n_ctx % 64, lengths outside 1 .. n_ctx, runs past n_ctx, a GQA ratio of 1 for the fused launch, a policy out of
    range: Q3TTS_ERR_INVALID before anything touches a device. Null cache outputs are not an error."""
    from q3tts import _abi
    lib = _abi.load_library()
    f32p, i32p = C.POINTER(C.c_float), C.POINTER(C.c_int32)
    x = np.zeros((4, 8 * 128), dtype=np.float32)
    w = np.ones(128, dtype=np.float32)
    out = np.zeros((4, 4 * 128), dtype=np.float32)
    P = lambda a, t: a.ctypes.data_as(t)
    lens = np.array([2, 2], dtype=np.int32)
    sec = np.ascontiguousarray(A.SECTIONS)

    def dec(n_ctx=128, hq=4, hkv=2, hd=128, ln=lens, policy=-1, form=0, o=out):
        return lib.q3tts_k_attention_decode_kv8(0, P(x, f32p), ln.size, P(ln, i32p), n_ctx, hq, hkv, hd, P(w, f32p), P(w, f32p), 1e-6, 1e6, P(sec, i32p),
                                                policy, form, None if o is None else o.ctypes.data, None, None, None, None, None)

    def runs(n_ctx=128, hd=128, rn=(2, 2), rp=(0, 0), policy=-1, form=0):
        rn, rp = np.array(rn, dtype=np.int32), np.array(rp, dtype=np.int32)
        return lib.q3tts_k_attention_runs_kv8(0, P(x, f32p), rn.size, P(rn, i32p), P(rp, i32p), n_ctx, 4, 2, hd, P(w, f32p), P(w, f32p), 1e-6, 1e6,
                                              P(sec, i32p), policy, form, out.ctypes.data, None, None, None, None, None)
    INVALID = -1
    assert dec(hd=64) == INVALID and b"head_dim" in lib.q3tts_last_error(None)
    assert b"decode_kv8 hook" in lib.q3tts_last_error(None)     # the message names the entry that was called
    assert runs(hd=64) == INVALID and b"runs_kv8 hook" in lib.q3tts_last_error(None)
    assert dec(n_ctx=100) == INVALID and b"n_ctx" in lib.q3tts_last_error(None)
    assert dec(ln=np.array([0, 4], dtype=np.int32)) == INVALID and dec(ln=np.array([129, 1], dtype=np.int32)) == INVALID
    assert dec(hq=2, hkv=2) == INVALID and dec(policy=2) == INVALID and dec(form=3) == INVALID and dec(form=2) == INVALID and dec(o=None) == INVALID
    assert runs(hd=64) == INVALID and runs(n_ctx=96) == INVALID and runs(rn=(0, 4)) == INVALID and runs(rp=(127, 0)) == INVALID
    assert runs(policy=3) == INVALID and runs(form=2) == INVALID
    assert dec() != INVALID and runs() != INVALID   # (null cache outputs: accepted — what follows depends on whether there is a device)


def _header_fields():
    src = open(os.path.join(REPO, "include", "q3tts.h")).read()
    body = re.search(r"typedef struct q3tts_engine_config \{(.*?)\} q3tts_engine_config;", src, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    return [m.group(1) for m in re.finditer(r"(\w+)\s*;", body)]


def test_config_field_in_header_abi_and_rust():
    """kv_q8_0 is the last member of q3tts_engine_config in include/q3tts.h, q3tts/_abi.py and rust/src/lib.rs, the three list the same
    fields in the same order, and the compiled library agrees with ctypes on the struct's size: q3tts_default_config writes kv_q8_0 = 0
    into the struct's last four bytes and nothing behind them."""
    from q3tts import _abi
    hdr = _header_fields()
    py = _abi.ENGINE_CONFIG_FIELD_ORDER   # (_fields_ + the member that lives in the former tail padding, as a property: q3tts/_abi.py)
    assert py[:-1] == [f[0] for f in _abi.EngineConfig._fields_]
    rs = open(os.path.join(REPO, "rust", "src", "lib.rs")).read()
    rs_body = re.search(r"pub struct q3tts_engine_config \{(.*?)\n\}", rs, re.S).group(1)
    rs_fields = re.findall(r"pub (\w+):", re.sub(r"//[^\n]*", "", rs_body))
    assert hdr == py == rs_fields and hdr[-1] == "kv_q8_0"
    size = C.sizeof(_abi.EngineConfig)
    assert _abi.KV_Q8_0_OFFSET == size - 4 == _abi.EngineConfig.predictor_q8_0.offset + 4 and size % 8 == 0
    buf = (C.c_ubyte * (size + 64))(*([0xAA] * (size + 64)))
    lib = _abi.load_library()
    lib.q3tts_default_config(C.cast(buf, C.POINTER(_abi.EngineConfig)))
    cfg = _abi.EngineConfig.from_buffer(buf)
    assert cfg.kv_q8_0 == 0 and cfg.predictor_q8_0 == 0 and cfg.talker_q8_0 == 0 and cfg.n_ctx == 4096
    assert bytes(buf[size - 4:size]) == b"\0" * 4           # the library wrote the member where the property reads it
    cfg.kv_q8_0 = 1
    assert bytes(buf[size - 4:size]) == b"\1\0\0\0" and cfg.predictor_q8_0 == 0 and _abi.copy_config(cfg).kv_q8_0 == 1
    cfg.kv_q8_0 = 0
    assert bytes(buf[size:]) == b"\xAA" * 64
    assert _abi.default_config().kv_q8_0 == 0 and _abi.tiny_config().kv_q8_0 == 0 and _abi.full_config_py().kv_q8_0 == 0
    fp = C.c_int64()
    c = _abi.full_config_py()
    c.with_vocoder = 0
    assert lib.q3tts_k_engine_footprint(C.byref(c), C.byref(fp)) == 0
    bf16 = fp.value
    c.kv_q8_0 = 1
    assert lib.q3tts_k_engine_footprint(C.byref(c), C.byref(fp)) == 0
    m = c.model   # the footprint follows the per-slot formula of the header
    assert bf16 - fp.value == c.max_batch * m.t_n_layer * m.t_n_kv_head * c.n_ctx * (2 * m.t_head_dim * 2 - 2 * (m.t_head_dim + m.t_head_dim // 16))
    c.kv_q8_0 = 2
    assert lib.q3tts_k_engine_footprint(C.byref(c), C.byref(fp)) == -1


def test_api_kv_cache_argument():
    from q3tts import api
    for bad in ("q4", "Q8_0", "f16", ""):
        with pytest.raises(ValueError):
            api.TtsEngine.new(None, "none", kv_cache=bad)


# ---- the oracle's own Q8_0 cache mode (q3o_attention_kv_q8, OracleModel.set_talker_kv_q8): what tests/test_kv_q8_gpu.py and
# tests/test_shapes_gpu.py compare the device with, bit for bit — held to the same float64 checks as the device, so that the two cannot be
# wrong in the same way ----------------------------------------------------------------------------------------------------------------------
def test_oracle_kv_q8_passes_stage1_and_stage2_on_all_cases(oracle):
    """q3o_attention_kv_q8 on every spec x kind of test_restatement_passes_stage1_on_all_cases: its K cache within the windows and the
    caps, its V cache equal to q3o_quantize_q8_0 of the f32 rows, its output within ATT_STAGE2_TOL of float64 over its own cache."""
    total, worst = K.Counts(), 0.0
    for spec in PLAIN:
        Hq, Hkv = spec["heads"]
        c = K.Counts()
        for kind in K.KINDS:
            xs, qn, kn, res = K.oracle_case_kv8(oracle, spec, kind)
            for x, (pos0, n), (out, k_q, k_d, v_q, v_d) in zip(xs, spec["seqs"], res):
                K.check_stage1_k(x, Hq, Hkv, kn, k_q, k_d, c)
                K.check_stage1_v(oracle, x, Hq, Hkv, v_q, v_d)
                q = K.oracle_q(oracle, x, Hq, Hkv, qn, kn)
                err = K.stage2_error(out, q[pos0:], k_q, k_d, v_q, v_d, pos0, Hq, Hkv)
                assert err <= ATT_STAGE2_TOL, (spec["name"], kind, pos0, n, err)
                worst = max(worst, err)
        c.check_caps(spec["name"])
        for f in ("elems", "near_q", "diff_q", "blocks", "near_d", "diff_d"):
            setattr(total, f, getattr(total, f) + getattr(c, f))
        total.worst_q = max(total.worst_q, c.worst_q)
    print(total.line("oracle, Q8_0 cache mode, all cases"))
    print(f"oracle, Q8_0 cache mode: worst error vs float64 / max|v^|: {worst:.1e} (bound {ATT_STAGE2_TOL:.1e})")
    total.check_caps("all cases")
    assert total.elems >= 6_247_808 and total.blocks >= 195_244


def test_oracle_kv_q8_equals_the_bf16_oracle_on_the_grid(oracle):
    """On grid_inputs the Q8_0 cache holds exactly what the bf16 cache holds (x^ = v = bf16(v), K all zeros): the Q8 oracle's output equals
    q3o_attention's in all 32 bits, and its cache dequantises to the bf16 oracle's V."""
    for spec in PLAIN:
        Hq, Hkv = spec["heads"]
        xs, qn, kn, res = K.oracle_case_kv8(oracle, spec, "grid")
        for x, (pos0, n), (out, k_q, k_d, v_q, v_d) in zip(xs, spec["seqs"], res):
            want, _, _, vb = K.oracle_seq(oracle, x, pos0, n, Hq, Hkv, qn, kn)
            assert not k_q.any() and not k_d.any() and np.array_equal(K.dequant(v_q, v_d), A.bf16_value(vb)), (spec["name"], pos0, n)
            assert np.array_equal(A.bits(out), A.bits(want)), (spec["name"], pos0, n)


def test_oracle_kv_q8_entry_points_agree(oracle):
    """attend_from selects rows and nothing else: the last row alone (as q3o_attention_last) and no row at all (the preparation stage)
    give the same bits and the same cache as the whole sequence."""
    spec = K.SPEC["prefill_a"]
    Hq, Hkv = spec["heads"]
    xs, qn, kn = K.make_inputs(spec, "normal")
    x = xs[-2]   # 127 rows
    every = K.oracle_seq_kv8(oracle, x, 0, x.shape[0], Hq, Hkv, qn, kn)
    last = K.oracle_seq_kv8(oracle, x, x.shape[0] - 1, 1, Hq, Hkv, qn, kn)
    none = K.oracle_seq_kv8(oracle, x, x.shape[0], 0, Hq, Hkv, qn, kn)
    assert np.array_equal(A.bits(last[0]), A.bits(every[0][-1:])) and none[0].shape[0] == 0
    for a, b, c in zip(every[1:], last[1:], none[1:]):
        assert np.array_equal(a, b) and np.array_equal(a, c)


def _model_prompt(oracle, om, rows, seed):
    desc, keep = oracle.make_prompt_desc(np.random.default_rng(seed).integers(0, 151643, size=rows), spk_emb=((np.arange(om.cfg.d_embed) % 13 - 6) * 0.03125).astype(np.float32))
    return om.build_prompt(desc)[-rows:]


@pytest.mark.parametrize("combine", [0, 1, 2])
def test_oracle_model_kv_q8_changes_the_talker_and_is_deterministic(oracle, combine):
    """Tiny shape, prompts of 5, 40 and 130 rows: with set_talker_kv_q8 the prefill logits differ in bits from the bf16-cache model's (alone,
    and combined with set_talker_q8 / set_talker_q8a8 against the same mode without it), and two runs of generate give the same ids."""
    from q3tts import _abi
    cfg = _abi.tiny_config(max_batch=1, n_ctx=256, with_vocoder=0)
    om, om8 = (oracle.OracleModel(cfg.model, seed=0, n_ctx=256, n_threads=8) for _ in range(2))
    try:
        for m in (om, om8):
            if combine:
                (m.set_talker_q8, m.set_talker_q8a8)[combine - 1]()
        om8.set_talker_kv_q8()
        for rows in (5, 40, 130):
            pe = _model_prompt(oracle, om, rows, 700 + rows)
            (h, l), (h8, l8) = om.talker_prefill(pe), om8.talker_prefill(pe)
            assert np.all(np.isfinite(l8)) and not np.array_equal(A.bits(l8), A.bits(l)) and not np.array_equal(A.bits(h8), A.bits(h)), rows
            assert np.abs(l8 - l).max() < 0.25 * np.abs(l).max(), rows   # another rounding of the cache, not another model
            kw = dict(temperature=0.7, top_k=40, top_p=0.9, seed=rows, max_steps=6, min_frames=6)
            a, b = om8.generate(pe, **kw), om8.generate(pe, **kw)
            assert a[0].shape == (6, cfg.model.n_codebooks) and np.array_equal(a[0], b[0]) and a[1] == b[1], rows
    finally:
        om.close()
        om8.close()


def test_oracle_model_kv_q8_leaves_the_predictor_alone(oracle):
    """A Talker of NO layers has no cache: there set_talker_kv_q8 must change nothing at all — the Predictor (five layers, 2 .. 16 keys per
    frame, a bf16 cache as on the device) computes every code after the first, and all logits and ids stay the same. With the Talker's
    layers back the same flag changes the logits of the same prompt."""
    from q3tts import _abi
    kw = dict(temperature=0.7, top_k=40, top_p=0.9, seed=3, max_steps=8, min_frames=8)
    got = {}
    for layers in (0, None):
        cfg = _abi.tiny_config(max_batch=1, n_ctx=256, with_vocoder=0)
        if layers is not None:
            cfg.model.t_n_layer = layers
        for kv in (0, 1):
            om = oracle.OracleModel(cfg.model, seed=0, n_ctx=256, n_threads=8)
            try:
                if kv:
                    om.set_talker_kv_q8()
                pe = _model_prompt(oracle, om, 40, 740)
                got[layers, kv] = (om.talker_prefill(pe)[1], om.generate(pe, **kw)[0])
            finally:
                om.close()
    assert np.array_equal(A.bits(got[0, 0][0]), A.bits(got[0, 1][0])) and np.array_equal(got[0, 0][1], got[0, 1][1])
    assert got[0, 0][1].shape[0] == 8 and len(np.unique(got[0, 0][1])) > 16
    assert not np.array_equal(A.bits(got[None, 0][0]), A.bits(got[None, 1][0]))


def test_equality_with_the_oracle_kv_q8_pins_the_summation_order(oracle):
    """What `==` against q3o_attention_kv_q8 adds to the float64 bound: the same attention over the SAME cache and the same q in another
    f32 summation order (numpy's) is inside ATT_STAGE2_TOL — the float64 checks accept it — and differs from the oracle in the bits of
    most outputs. And a cache read with the scales of the neighbouring block is outside the bound."""
    spec = K.SPEC["prefill_a"]
    Hq, Hkv = spec["heads"]
    xs, qn, kn, res = K.oracle_case_kv8(oracle, spec, "normal")
    x, (out, k_q, k_d, v_q, v_d) = xs[-1], res[-1]   # the run of 128 rows
    q = K.oracle_q(oracle, x, Hq, Hkv, qn, kn)
    other = K.attend32(q, K.dequant(k_q, k_d), K.dequant(v_q, v_d), 0, Hq, Hkv)
    assert K.stage2_error(other, q, k_q, k_d, v_q, v_d, 0, Hq, Hkv) <= ATT_STAGE2_TOL
    assert (A.bits(other) != A.bits(out)).mean() > 0.5
    swapped = K.attend32(q, K.dequant(k_q, k_d[..., ::-1]), K.dequant(v_q, v_d), 0, Hq, Hkv)
    assert K.stage2_error(swapped, q, k_q, k_d, v_q, v_d, 0, Hq, Hkv) > ATT_STAGE2_TOL

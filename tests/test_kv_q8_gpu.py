"""The Q8_0 K/V cache (q3tts_engine_config.kv_q8_0, csrc/q3_attend_kv8.hip) on the device.
Kernel level, one launch at a time through q3tts_k_attention_runs_kv8 / _decode_kv8 (the cases of tests/_kv_q8.py, every input kind):
  1. stage 1 (the cache: K within the windows of tests/_kv_q8.py, V equal to q3o_quantize_q8_0) and stage 2 (the output against float64
     over the cache as returned, ATT_STAGE2_TOL of tests/_oracle.py);
  2. k_attend_gqa2_kv8 and k_attend_kv8<2, true> agree bit for bit, output and cache;
  3. the last row of a sequence through the decode hook equals the same row of the sequence run as one prefill run, all 32 bits;
  4. on the int8 grid (x^ = v = bf16(v), every score 0) the output equals q3o_attention's, all 32 bits;
  5. output forms 1 and 2 are the form-0 output converted by the existing rules.
Engine level (tiny shape, kv_q8_0 = 1): ids and PCM do not depend on the batch, the slot count, sessions or voice prefixes; the memory
formula; kv_q8_0 = 0 is today's engine; kv_q8_0 = 2 is refused. Ids with the Q8_0 cache may differ from the bf16 cache's: that is
recorded by tools/kv_q8_bench.py, not asserted."""
import ctypes as C

import numpy as np
import pytest

import _attend_ref as A
import _kv_q8 as K
import _slots as SL
from _oracle import ATT_STAGE2_TOL

pytestmark = pytest.mark.gpu


def _policy(lib, case, policy):
    fused = case["spec"]["hook"] == "decode"
    assert lib.q3tts_k_attend_policy(max(policy, 0) if fused else 0, 0 if fused else max(policy, 0)) == 0


def _per_seq(case, r, i):
    """Slot i's cache as [position][Hkv][...]: k_q, k_d, v_q, v_d."""
    return tuple(np.ascontiguousarray(r[k][i].transpose(1, 0, 2)) for k in ("k_q", "k_d", "v_q", "v_d"))


_ORACLE = {}


def _oracle_case(oracle, spec, kind):
    key = (spec["name"], kind)
    if key not in _ORACLE:
        xs, qn, kn = K.make_inputs(spec, kind)
        Hq, Hkv = spec["heads"]
        res = [K.oracle_seq(oracle, x, p, n, Hq, Hkv, qn, kn) for x, (p, n) in zip(xs, spec["seqs"])]
        for a in xs + [qn, kn] + [t for r in res for t in r]:
            a.setflags(write=False)
        _ORACLE[key] = (xs, qn, kn, res)
    return _ORACLE[key]


@pytest.mark.parametrize("name", list(K.CASES))
def test_kv8_kernel_case(oracle, name):
    """One case on every input kind through every kernel it names (checks 1, 2 and 5 of the module docstring; the pick hook names the
    kernel). Prints the stage-1 counts and the worst stage-2 error per kernel."""
    from q3tts import _abi, native
    lib = _abi.load_library()
    case = K.CASES[name]
    spec = case["spec"]
    Hq, Hkv = spec["heads"]
    counts, worst = K.Counts(), {}
    try:
        for kind in K.KINDS:
            xs, qn, kn, res = _oracle_case(oracle, spec, kind)
            first = None
            for policy, code in case["variants"]:
                what = (name, kind, K.KERNELS[code])
                _policy(lib, case, policy)
                assert native.k_attend_pick_kv8(want_code=True, **K.pick_args(case)) == code, what
                r0 = K.launch(native, case, policy, xs, qn, kn, 0)
                outs = A.hook_out_split(spec, r0["out"])
                err = 0.0
                for i, (x, (pos0, n), (_, q, _, _)) in enumerate(zip(xs, spec["seqs"], res)):
                    tot = pos0 + n
                    k_q, k_d, v_q, v_d = _per_seq(case, r0, i)
                    for a in (k_q, k_d, v_q, v_d):
                        assert not a[tot:].any(), what + (i, "the cache past the sequence's end was written")
                    if first is None:   # (the second kernel's cache is compared with the first's, bit for bit, below)
                        K.check_stage1_k(x, Hq, Hkv, kn, k_q[:tot], k_d[:tot], counts)
                        K.check_stage1_v(oracle, x, Hq, Hkv, v_q[:tot], v_d[:tot])
                    err = max(err, K.stage2_error(outs[i], q[pos0:], k_q[:tot], k_d[:tot], v_q[:tot], v_d[:tot], pos0, Hq, Hkv))
                assert err <= ATT_STAGE2_TOL, what + (err,)
                worst[code] = max(worst.get(code, 0.0), err)
                if kind == "zero_block":   # value block ZERO_BLOCK of every key: d = 0, q = 0, and the output columns are exactly 0
                    assert not r0["v_d"][..., A.ZERO_BLOCK].any() and not r0["v_q"][..., 32 * A.ZERO_BLOCK:32 * A.ZERO_BLOCK + 32].any(), what
                    assert not r0["out"].reshape(-1, Hq, K.NB, 32)[:, :, A.ZERO_BLOCK].any(), what
                if first is None:
                    first = r0
                else:                                                                                           # 2
                    for k in ("out", "k_q", "k_d", "v_q", "v_d"):
                        assert np.array_equal(r0[k].view(np.uint8), first[k].view(np.uint8)), what + (k,)
                if 1 in case["forms"]:                                                                          # 5
                    r1 = K.launch(native, case, policy, xs, qn, kn, 1)
                    r2 = K.launch(native, case, policy, xs, qn, kn, 2)
                    assert np.array_equal(r1["out"], A.bf16_bits(r0["out"])), what
                    q8, d8 = oracle.quantize_q8_0_act(r0["out"])
                    assert np.array_equal(r2["out"], q8) and np.array_equal(A.bits(r2["scale"]), A.bits(d8)), what
                    for r in (r1, r2):
                        for k in ("k_q", "k_d", "v_q", "v_d"):
                            assert np.array_equal(r[k], r0[k]), what + (k,)
    finally:
        lib.q3tts_k_attend_policy(0, 0)
    counts.check_caps(name)
    print(counts.line(name))
    print(f"{name}: worst error vs float64 / max|v^|: " + ", ".join(f"{K.KERNELS[c]} {e:.1e}" for c, e in worst.items()) + f" (bound {ATT_STAGE2_TOL:.1e})")


@pytest.mark.parametrize("name", ["decode13", "decode_long", "decode_r4"])
def test_decode_equals_prefill(oracle, name):
    """Check 3: every slot's sequence once through the decode hook (rows 0 .. len - 2 cached by k_qk_prep_kv8, the last row by the fused
    kernel, newest key and value from LDS) and once as one prefill run of len rows (every key from the cache): the last row's output and
    the whole cache agree in every bit, under both decode policies."""
    from q3tts import native
    case = K.CASES[name]
    spec = case["spec"]
    Hq, Hkv = spec["heads"]
    tail = (case["n_ctx"], Hq, Hkv, K.HD)
    for kind in ("normal", "wide", "newest", "outliers"):
        xs, qn, kn = K.make_inputs(spec, kind)
        lens = [p + n for p, n in spec["seqs"]]
        run = native.k_attention_runs_kv8(np.concatenate(xs), [(0, t) for t in lens], *tail, qn, kn, A.EPS, A.THETA, A.SECTIONS, policy=2)
        last = np.cumsum(lens) - 1
        for policy, _ in case["variants"]:
            dec = native.k_attention_decode_kv8(np.concatenate(xs), lens, *tail, qn, kn, A.EPS, A.THETA, A.SECTIONS, policy=policy)
            assert np.array_equal(A.bits(dec["out"]), A.bits(run["out"][last])), (name, kind, policy)
            for k in ("k_q", "k_d", "v_q", "v_d"):
                assert np.array_equal(dec[k], run[k]), (name, kind, policy, k)


@pytest.mark.parametrize("name", ["decode13", "decode_long", "decode_r4", "prefill_a", "prefill_b", "runs_r1", "runs_r4"])
def test_grid_equals_the_oracle(oracle, name):
    """Check 4: V on the int8 grid and k_norm_w = 0 — the Q8_0 cache holds exactly the values the bf16 cache holds — so the value chain and
    the combination must give q3o_attention's output, all 32 bits, in the decode and the runs kernels."""
    from q3tts import _abi, native
    lib = _abi.load_library()
    case = K.CASES[name]
    spec = case["spec"]
    Hq, Hkv = spec["heads"]
    xs, qn, kn = K.grid_inputs(spec)
    want = [K.oracle_seq(oracle, x, p, n, Hq, Hkv, qn, kn) for x, (p, n) in zip(xs, spec["seqs"])]
    try:
        for policy, code in case["variants"]:
            _policy(lib, case, policy)
            r = K.launch(native, case, policy, xs, qn, kn, 0)
            for i, (dev, (out, _, _, vb)) in enumerate(zip(A.hook_out_split(spec, r["out"]), want)):
                tot = sum(spec["seqs"][i])
                k_q, k_d, v_q, v_d = _per_seq(case, r, i)
                assert np.array_equal(K.dequant(v_q[:tot], v_d[:tot]), A.bf16_value(vb)) and not k_q.any(), (name, i)
                assert np.array_equal(A.bits(dev), A.bits(out)), (name, K.KERNELS[code], i)
    finally:
        lib.q3tts_k_attend_policy(0, 0)


# ---- engine level -----------------------------------------------------------------------------------------------------------------------
def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _same(got, want, what):
    assert got.status == 0 and want.status == 0, (what, got.status, want.status)
    assert got.codes.shape == want.codes.shape and np.array_equal(got.codes, want.codes), what
    assert got.hit_eos == want.hit_eos, what
    assert (got.pcm is None) == (want.pcm is None), what
    if want.pcm is not None:
        assert got.pcm.shape == want.pcm.shape and np.array_equal(_bits(got.pcm), _bits(want.pcm)), what


def _cfg(max_batch, kv=1, talker_q8=0):
    from q3tts import _abi
    cfg = _abi.tiny_config(max_batch=max_batch, n_ctx=256)
    cfg.kv_q8_0, cfg.talker_q8_0 = kv, talker_q8
    return cfg


class _Engines:
    def __init__(self):
        self.engs = {}

    def get(self, max_batch, kv=1, talker_q8=0):
        from q3tts import native
        key = (max_batch, kv, talker_q8)
        if key not in self.engs:
            self.engs[key] = native.NativeEngine(_cfg(*key))
        return self.engs[key]

    def close(self):
        for e in self.engs.values():
            e.close()


@pytest.fixture(scope="module")
def engines():
    e = _Engines()
    yield e
    e.close()


@pytest.fixture(scope="module")
def requests20(oracle):
    """20 sampled, forced-length requests of tests/_slots.py (prompts of 1 .. 40 rows, at most 24 frames), all with PCM; and the two base
    prompts they are cut from."""
    om = oracle.OracleModel(_cfg(8).model, seed=0, n_ctx=256, n_threads=8)
    try:
        bases = SL.base_rows(oracle, om)
    finally:
        om.close()
    reqs = [dict(r, want_pcm=1) for r in SL.mixed_requests(bases)[:20]]
    return reqs, bases


def _session_pcm(eng, reqs):
    from q3tts import _abi, native
    chunks, final = {}, {}
    s = native.NativeSession(eng)
    try:
        ids = [s.submit(**r) for r in reqs]
        for rid, kind, pcm, is_final, res in s.events(timeout_ms=60000):
            if kind == _abi.EV_CHUNK:
                chunks.setdefault(rid, []).append(pcm)
            else:
                final[rid] = res
    finally:
        s.close()
    assert set(final) == set(ids)
    return [(np.concatenate(chunks[i]) if i in chunks else np.zeros(0, dtype=np.float32), final[i]) for i in ids]


def _invariants(eng, big, reqs, bases, what):
    """Checks 1 - 3 of the engine level on one engine (and a larger one, when given)."""
    want = eng.generate_batch(reqs)
    assert all(w.status == 0 and w.codes.shape[0] == r["force_eos_at"] for w, r in zip(want, reqs)), what
    for i, r in enumerate(reqs):                                                    # 1: alone
        _same(eng.generate(**r), want[i], (what, "alone", i))
    if big is not None:                                                             # 1: a 65-slot engine
        for i, g in enumerate(big.generate_batch(reqs)):
            _same(g, want[i], (what, "65 slots", i))
    for i, (pcm, res) in enumerate(_session_pcm(eng, reqs)):                        # 2: a session's joined chunks
        assert np.array_equal(res.codes, want[i].codes), (what, "session", i)
        assert pcm.shape == want[i].pcm.shape and np.array_equal(_bits(pcm), _bits(want[i].pcm)), (what, "session", i)
    P = 40                                                                          # 3: a voice prefix of 40 rows + a text part
    whole = [bases[0][-(P + k):] for k in (1, 7, 24)]
    kw = dict(temperature=0.7, top_k=40, top_p=0.9, max_steps=20, min_frames=9, force_eos_at=9, want_pcm=1)
    for i, w in enumerate(whole):
        with eng.create_prefix(embd=w[:P]) as x:
            full, pre = eng.generate_batch([dict(embd=w, seed=50 + i, **kw), dict(embd=w[P:], prefix=x, seed=50 + i, **kw)])
            _same(pre, full, (what, "prefix", i))
            assert full.codes.shape[0] == 9
            h0, l0 = eng.talker_prefill(w)
            h1, l1 = eng.talker_prefill_prefix(x, w[P:])
            assert np.array_equal(_bits(h1), _bits(h0)) and np.array_equal(_bits(l1), _bits(l0)), (what, "prefill_prefix", i)


def test_engine_results_do_not_depend_on_batch_slots_session_or_prefix(engines, requests20):
    reqs, bases = requests20
    _invariants(engines.get(8), engines.get(65), reqs, bases, "kv_q8_0")


def test_the_same_with_a_w8a8_talker(engines, requests20):
    """kv_q8_0 is independent of talker_q8_0: the invariants hold with the Talker's GEMMs in Q8_0 x Q8_0 (the attention kernels then write
    their output as Q8_0 blocks): all 20 requests, alone, on a 65-slot W8A8 engine, through a session and behind prefixes."""
    reqs, bases = requests20
    _invariants(engines.get(8, talker_q8=2), engines.get(65, talker_q8=2), reqs, bases, "kv_q8_0 + talker_q8_0 = 2")


def test_memory_formula():
    """q3tts_k_device_bytes of freshly created engines (the counter also takes what an engine allocates later: prefix stores, staging): bf16
    engine minus Q8_0 engine = L * B * Hkv * n_ctx * (2 * hd * 2 - 2 * (hd + hd / 16)) bytes, exactly."""
    from q3tts import native
    for B in (8, 65):
        got = []
        for kv in (0, 1):
            eng = native.NativeEngine(_cfg(B, kv=kv))
            got.append(eng.device_bytes())
            eng.close()
        cfg = _cfg(B)
        m = cfg.model
        assert got[0] - got[1] == m.t_n_layer * B * m.t_n_kv_head * cfg.n_ctx * (2 * m.t_head_dim * 2 - 2 * (m.t_head_dim + m.t_head_dim // 16)), B


def test_kv_q8_0_off_is_the_engine_as_it_was(engines, requests20):
    """kv_q8_0 = 0 against a config whose kv_q8_0 was never written (a zero-initialised struct filled field by field without it): the same
    bytes allocated, the same ids and PCM."""
    from q3tts import _abi, native
    reqs, _ = requests20
    src = _cfg(8, kv=0)
    cfg = _abi.EngineConfig()
    for name, _t in _abi.EngineConfig._fields_:   # (kv_q8_0 is not among them: q3tts/_abi.py keeps it in the former tail padding)
        setattr(cfg, name, getattr(src, name))
    eng = native.NativeEngine(cfg)
    try:
        ref = native.NativeEngine(src)
        try:
            assert eng.device_bytes() == ref.device_bytes()
        finally:
            ref.close()
        for i, (g, w) in enumerate(zip(eng.generate_batch(reqs[:8]), engines.get(8, kv=0).generate_batch(reqs[:8]))):
            _same(g, w, i)
    finally:
        eng.close()


def test_kv_q8_0_other_values_are_refused():
    from q3tts import _abi
    lib = _abi.load_library()
    for bad in (2, -1):
        cfg = _cfg(4, kv=bad)
        h = C.c_void_p()
        assert lib.q3tts_engine_create(C.byref(cfg), C.byref(h)) == -1 and not h.value   # Q3TTS_ERR_INVALID
        assert b"kv_q8_0" in lib.q3tts_last_error(None)

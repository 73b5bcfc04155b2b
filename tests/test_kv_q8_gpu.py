"""The Q8_0 K/V cache (q3tts_engine_config.kv_q8_0, csrc/q3_attend_kv8.hip) on the device.
Kernel level, one launch at a time through q3tts_k_attention_runs_kv8 / _decode_kv8 (the cases of tests/_kv_q8.py, every input kind):
  1. stage 1 (the cache: K within the windows of tests/_kv_q8.py, V equal to q3o_quantize_q8_0) and stage 2 (the output against float64
     over the cache as returned, ATT_STAGE2_TOL of tests/_oracle.py);
  2. k_attend_gqa2_kv8 and k_attend_kv8<2, true> agree bit for bit, output and cache;
  3. the last row of a sequence through the decode hook equals the same row of the sequence run as one prefill run, all 32 bits;
  4. on the int8 grid (x^ = v = bf16(v), every score 0) the output equals q3o_attention's, all 32 bits;
  5. output forms 1 and 2 are the form-0 output converted by the existing rules.
  6. cache and output equal the oracle's Q8_0 cache mode (q3o_attention_kv_q8), every bit, on every case, kind and kernel.
Engine level (tiny shape, kv_q8_0 = 1): ids and PCM do not depend on the batch, the slot count, sessions or voice prefixes; the memory
formula; kv_q8_0 = 0 is today's engine; kv_q8_0 = 2 is refused; prefill hidden / logits and ids equal the oracle's with
set_talker_kv_q8 (prompts over the key-block edges, greedy and sampled, a batch with reused slots, voice prefixes, three layers,
talker_q8_0 = 2, the full shape), and the bf16-cache oracle gives other logits and other sampled ids."""
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


# ---- the kernels against the oracle's Q8_0 cache mode, bit for bit ----------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(K.CASES))
def test_kv8_kernel_case_equals_the_oracle(oracle, name):
    """Every case x input kind x kernel the case names against q3o_attention_kv_q8 with `==`: the cache (quants and f16 scale bits of K and
    V, nothing written past the sequence's end) and the f32 output, all 32 bits. K is not zero here (unlike the grid case), so this is what
    pins the ORDER of the score chain over x^ = f32(d) * q, and the quantiser's f32 input (the norm's and the rotation's own order), to
    DESIGN.md §4.4 / §22; decode_long runs k_attend_gqa2_kv8 past 256 keys on every kind, `wide` and `newest` among them, with the
    newest key served from LDS. The float64 checks of test_kv8_kernel_case stay: they keep the oracle and the device from being wrong
    together (tests/test_kv_q8_cpu.py holds the oracle to them too)."""
    from q3tts import _abi, native
    lib = _abi.load_library()
    case = K.CASES[name]
    spec = case["spec"]
    try:
        for kind in K.KINDS:
            xs, qn, kn, res = K.oracle_case_kv8(oracle, spec, kind)
            for policy, code in case["variants"]:
                what = (name, kind, K.KERNELS[code])
                _policy(lib, case, policy)
                assert native.k_attend_pick_kv8(want_code=True, **K.pick_args(case)) == code, what
                r = K.launch(native, case, policy, xs, qn, kn, 0)
                for i, (dev, (pos0, n), want) in enumerate(zip(A.hook_out_split(spec, r["out"]), spec["seqs"], res)):
                    tot = pos0 + n
                    for key, got, ref in zip(("k_q", "k_d", "v_q", "v_d"), _per_seq(case, r, i), want[1:]):
                        assert np.array_equal(got[:tot], ref) and not got[tot:].any(), what + (i, key)
                    assert np.array_equal(A.bits(dev), A.bits(want[0])), what + (i, "out")
    finally:
        lib.q3tts_k_attend_policy(0, 0)


# ---- engines with kv_q8_0 = 1 against the oracle with set_talker_kv_q8 ---------------------------------------------------------------------
# Everything above the kernels — the scale pointers behind the quants in one allocation, the per-layer cache pointers, the prefix store's
# scales, the layer and head a scale belongs to — is wrong in the same way for every batch size and slot count, so the invariants above
# cannot see it. These tests tie one engine of each kind to the oracle; the invariants then carry that to 65 slots and sessions.
class _Oracles:
    """Pairs (bf16-cache model, Q8_0-cache model) of the tiny shape per (talker_q8_0, t_n_layer)."""

    def __init__(self, oracle):
        self.O, self.pairs = oracle, {}

    def get(self, talker_q8=0, layers=None):
        key = (talker_q8, layers)
        if key not in self.pairs:
            cfg = _cfg(1, talker_q8=talker_q8)
            if layers is not None:
                cfg.model.t_n_layer = layers
            pair = tuple(self.O.OracleModel(cfg.model, seed=0, n_ctx=256, n_threads=8) for _ in range(2))
            for m in pair:
                if talker_q8 == 2:
                    m.set_talker_q8a8()
            pair[1].set_talker_kv_q8()
            self.pairs[key] = pair
        return self.pairs[key]

    def close(self):
        for pair in self.pairs.values():
            for m in pair:
                m.close()


@pytest.fixture(scope="module")
def oracles(oracle):
    o = _Oracles(oracle)
    yield o
    o.close()


def _prefill_equal(eng, om, om8, pe, what):
    """eng.talker_prefill(pe) == the Q8_0-cache oracle's, hidden and logits, all bits; and the bf16-cache oracle's logits are others."""
    h_ref, l_ref = om8.talker_prefill(pe)
    assert not np.array_equal(_bits(l_ref), _bits(om.talker_prefill(pe)[1])), what   # an engine that ignored kv_q8_0 fails below
    h, l = eng.talker_prefill(pe)
    assert np.array_equal(_bits(l), _bits(l_ref)) and np.array_equal(_bits(h), _bits(h_ref)), what
    return h_ref, l_ref


def _generate_equal(eng, om, om8, r, what, prefix=None):
    """One request through eng == the Q8_0-cache oracle alone (ids and hit_eos); a sampled request's ids differ from the bf16-cache
    oracle's (a greedy one's need not: on the CPU oracle greedy ids of some prompts are the same under both caches)."""
    ref, eos = om8.generate(r["embd"], **K.oracle_kw(r))
    if r["temperature"] > 0:
        assert not np.array_equal(ref, om.generate(r["embd"], **K.oracle_kw(r))[0]), what
    got = eng.generate(**r) if prefix is None else eng.generate(**dict(r, embd=r["embd"][prefix[1]:], prefix=prefix[0]))
    assert got.status == 0 and got.codes.shape == ref.shape and np.array_equal(got.codes, ref) and got.hit_eos == eos, what
    return ref


@pytest.mark.parametrize("talker_q8", [0, 2])
def test_engine_prefill_equals_the_oracle(oracle, engines, oracles, talker_q8):
    """Prompts of 1, 5, 63, 64, 65, 130 and 200 rows (the 64-key block edges) under prefill policies 0 and 2 and decode policies 0 and 1:
    hidden and logits of the last row, all bits. With talker_q8_0 = 2 the attention kernels write Q8_0 blocks (att_out1 / att_out2)."""
    from q3tts import _abi
    lib = _abi.load_library()
    eng = engines.get(8, talker_q8=talker_q8)
    om, om8 = oracles.get(talker_q8)
    try:
        for rows in (1, 5, 63, 64, 65, 130, 200):
            pe = K.prompt_rows(oracle, om, rows, 300)
            ref = None
            for dec, pre in ((0, 0), (1, 2), (0, 2), (1, 0)):
                assert lib.q3tts_k_attend_policy(dec, pre) == 0
                if ref is None:
                    ref = _prefill_equal(eng, om, om8, pe, (rows, dec, pre))
                else:
                    h, l = eng.talker_prefill(pe)
                    assert np.array_equal(_bits(l), _bits(ref[1])) and np.array_equal(_bits(h), _bits(ref[0])), (rows, dec, pre)
    finally:
        lib.q3tts_k_attend_policy(0, 0)


@pytest.mark.parametrize("rows", [60, 130])
def test_engine_generate_equals_the_oracle(oracle, engines, oracles, rows):
    """Greedy and sampled, 12 frames: from 60 rows the decode step appends across position 64 (a new key block, its scales behind the
    quants); from 130 rows it starts in the third block. Ids and hit_eos."""
    eng = engines.get(8)
    om, om8 = oracles.get()
    pe = K.prompt_rows(oracle, om, rows, 5)
    _prefill_equal(eng, om, om8, pe, rows)
    for kw in (K.GREEDY, K.SAMPLED):
        ref = _generate_equal(eng, om, om8, dict(embd=pe, seed=9, max_steps=12, min_frames=12, **kw), (rows, kw))
        assert ref.shape[0] == 12
    r = dict(embd=pe, seed=10, max_steps=12, min_frames=12, force_eos_at=7, **K.SAMPLED)
    assert _generate_equal(eng, om, om8, r, (rows, "eos")).shape[0] == 7


@pytest.mark.parametrize("talker_q8", [0, 2])
def test_engine_batch_equals_the_oracle_alone(oracle, engines, oracles, talker_q8):
    """11 sampled requests of 40 .. 130 prompt rows and forced lengths on 8 slots (three slots are used again): each == the oracle run
    alone. With this the invariants above (65 slots, sessions) are tied to the reference."""
    eng = engines.get(8, talker_q8=talker_q8)
    om, om8 = oracles.get(talker_q8)
    reqs = K.batch_requests(oracle, om, 11)
    refs = [om8.generate(r["embd"], **K.oracle_kw(r)) for r in reqs]
    for i, (r, ref) in enumerate(zip(reqs, refs)):
        assert ref[0].shape[0] == r["force_eos_at"] and not np.array_equal(ref[0], om.generate(r["embd"], **K.oracle_kw(r))[0]), i
    for i, (g, ref) in enumerate(zip(eng.generate_batch(reqs), refs)):
        assert g.status == 0 and g.codes.shape == ref[0].shape and np.array_equal(g.codes, ref[0]) and g.hit_eos == ref[1], (talker_q8, i)


@pytest.mark.parametrize("P,rows", [(40, 90), (64, 100)])
def test_engine_voice_prefix_equals_the_oracle(oracle, engines, oracles, P, rows):
    """create_prefix(w[:P]) + w[P:] == the oracle on the whole prompt w: P = 40 ends inside a key block (k_kv_prefix_kv8 copies the whole
    block and the store's scales), P = 64 on its edge. Also talker_prefill_prefix == the oracle's prefill of w."""
    eng = engines.get(8)
    om, om8 = oracles.get()
    w = K.prompt_rows(oracle, om, rows, P)
    with eng.create_prefix(embd=w[:P]) as x:
        _generate_equal(eng, om, om8, dict(embd=w, seed=P, max_steps=9, min_frames=9, **K.SAMPLED), (P, "prefix"), prefix=(x, P))
        h_ref, l_ref = om8.talker_prefill(w)
        assert not np.array_equal(_bits(l_ref), _bits(om.talker_prefill(w)[1]))
        h, l = eng.talker_prefill_prefix(x, w[P:])
        assert np.array_equal(_bits(l), _bits(l_ref)) and np.array_equal(_bits(h), _bits(h_ref)), P


def test_engine_of_three_layers_equals_the_oracle(oracle, oracles):
    """t_n_layer = 3: with two layers a wrong layer stride of the cache (or of its scales) can land on the other layer's rows of the same
    slot and cancel in no test above; with three it cannot."""
    from q3tts import native
    cfg = _cfg(2)
    cfg.model.t_n_layer, cfg.with_vocoder = 3, 0
    om, om8 = oracles.get(0, 3)
    eng = native.NativeEngine(cfg)
    try:
        pe = K.prompt_rows(oracle, om, 70, 3)
        _prefill_equal(eng, om, om8, pe, "3 layers")
        _generate_equal(eng, om, om8, dict(embd=pe, seed=3, max_steps=10, min_frames=10, **K.SAMPLED), "3 layers")
        reqs = K.batch_requests(oracle, om, 4, frames=(4, 6), seed=33)
        for i, (g, r) in enumerate(zip(eng.generate_batch(reqs), reqs)):
            assert g.status == 0 and np.array_equal(g.codes, om8.generate(r["embd"], **K.oracle_kw(r))[0]), i
    finally:
        eng.close()


def test_full_shape_kv_q8_0_prefill_and_frames(oracle):
    """The benchmarked shape (Hkv = 8, 28 layers: the tiny shape covers neither) with kv_q8_0 = 1, laid out as
    test_parity_gpu.py::test_talker_q8_0_full_shape_prefill_and_frames: prefill hidden / logits bits and 4 greedy frames == the oracle; the
    bf16-cache oracle (the same model before the flag is set) gives other logits."""
    from q3tts import _abi, native
    cfg = _abi.full_config_py()
    cfg.max_batch, cfg.n_ctx, cfg.max_steps_cap, cfg.with_vocoder, cfg.kv_q8_0 = 2, 128, 16, 0, 1
    eng = native.NativeEngine(cfg)
    om = oracle.OracleModel(cfg.model, seed=0, n_ctx=128, n_threads=16)
    try:
        desc, keep = oracle.make_prompt_desc(np.random.default_rng(1234).integers(0, 151643, size=12), spk_emb=K.spk(cfg.model.d_embed))
        pe = om.build_prompt(desc)
        l_bf16 = om.talker_prefill(pe)[1]
        om.set_talker_kv_q8()
        h_ref, l_ref = om.talker_prefill(pe)
        assert not np.array_equal(_bits(l_ref), _bits(l_bf16))
        h, l = eng.talker_prefill(pe)
        assert np.array_equal(_bits(l), _bits(l_ref)) and np.array_equal(_bits(h), _bits(h_ref))
        ref, _ = om.generate(pe, temperature=0.0, max_steps=4, min_frames=4)
        res = eng.generate(desc=desc, temperature=0.0, max_steps=4, min_frames=4)
        assert ref.shape == (4, 16) and np.array_equal(res.codes, ref)
    finally:
        eng.close()
        om.close()

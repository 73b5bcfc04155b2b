"""The Talker's K/V cache with ggml Q4_0 blocks (q3tts_engine_options.kv_type_k / kv_type_v, csrc/q3_attend_kvq.hip) on the
device, in both accepted modes: K Q8_0 with V Q4_0, and both Q4_0.
Kernel level (q3tts_k_attention_runs_kv4 / _decode_kv4; the quants come back one per element, a Q4_0 quant as its nibble 0 .. 15):
  1. stage 1 — V equals the numpy-f32 restatement of quantize_row_q4_0 below bit for bit; K is held to the quantiser applied to the
     float64-prepared keys with the two exceptions and the cap of tests/_kv_q8.py (a Q8_0 K: its own check_stage1_k) — and stage 2, the f32
     output against float64 attention over the cache as returned, ATT_STAGE2_TOL;
  2. the non-fused run, the fused kernels under both decode policies and the gqa2 kernel give == outputs and == caches;
  3. on the exact grid (v = 2^e q, q in [-8, 7], a -8 in every block, k_norm_w = 0) the output equals q3o_attention's, all 32 bits;
  4. a prefix store copied into a slot and saved again: exact below P, zero-filled from P on.
Engine level (tiny shape, n_ctx = 256): ids and PCM do not depend on slot count, voice prefixes or sessions; they are not the Q8_0
cache's; the refusals; the memory formula."""
import numpy as np
import pytest

import _attend_ref as A
import _kv_q8 as K
from _oracle import ATT_STAGE2_TOL

pytestmark = pytest.mark.gpu

Q4, Q8 = 2, 8
MODES = {"q8_q4": (Q8, Q4), "q4_q4": (Q4, Q4)}
N_CTX = 320
PARTNER = {1: 65, 63: 257, 64: 1, 65: 63, 257: 64}     # the other slot's length: two slots of different length in every launch
TAIL = (A.EPS, A.THETA, A.SECTIONS)


def quant4_32(x):
    """ggml's quantize_row_q4_0 in f32 on the last axis (blocks of 32): nibbles int8 0 .. 15 (same shape), d f16 bits [..., n / 32]."""
    f = np.float32
    xb = np.ascontiguousarray(x, dtype=f).reshape(x.shape[:-1] + (x.shape[-1] // 32, 32))
    mx = np.take_along_axis(xb, np.abs(xb).argmax(axis=-1)[..., None], axis=-1)    # the FIRST element of largest magnitude, with its sign
    d = (mx / f(-8.0)).astype(f)
    with np.errstate(divide="ignore"):
        idv = np.where(d != 0, f(1.0) / d, f(0.0)).astype(f)
    q = np.minimum(15, np.trunc((xb * idv).astype(f) + f(8.5))).astype(np.int8)
    return q.reshape(x.shape), d[..., 0].astype(np.float16).view(np.uint16)


def dequant(q, dbits, typ):
    """x^ of a cache side as returned: f32(d) * (q - 8) for Q4_0, f32(d) * q for Q8_0."""
    return K.dequant(q - 8 if typ == Q4 else q, dbits)


def check_stage1_k4(x, Hq, Hkv, kn, k_q, k_d, counts):
    """The cached Q4_0 keys against the quantiser applied to the float64-prepared keys: the scale inside (max / -8)(1 +- SCALE_WINDOW) as
    f16, each quant floor(u), u = k64 / (max / -8) + 8.5 capped at 15 — either neighbour where u lies within QUANT_WINDOW of an integer."""
    tot = x.shape[0]
    k64 = A.prep64(x.reshape(tot, Hq + 2 * Hkv, A.HD)[:, Hq:Hq + Hkv], kn, np.arange(tot)).reshape(tot, Hkv, K.NB, 32)
    t = np.take_along_axis(k64, np.abs(k64).argmax(axis=-1)[..., None], axis=-1)[..., 0] / -8.0
    e = np.stack([(t * (1 - K.SCALE_WINDOW)).astype(np.float16), (t * (1 + K.SCALE_WINDOW)).astype(np.float16)])
    gv = np.ascontiguousarray(k_d, dtype=np.uint16).view(np.float16)
    assert ((e.min(axis=0) <= gv) & (gv <= e.max(axis=0))).all(), "a K scale outside its window"
    u = k64 / t[..., None] + 8.5
    lo, hi = np.minimum(15, np.floor(u - K.QUANT_WINDOW)), np.minimum(15, np.floor(u + K.QUANT_WINDOW))
    q = k_q.reshape(tot, Hkv, K.NB, 32)
    assert ((lo <= q) & (q <= hi)).all(), "a K quant outside the rule"
    counts.elems += q.size; counts.near_q += int((lo != hi).sum()); counts.diff_q += int((q != np.minimum(15, np.floor(u))).sum())
    counts.blocks += t.size; counts.near_d += int((e[0] != e[1]).sum()); counts.diff_d += int((gv != t.astype(np.float16)).sum())


def _slot(r, i, tot):
    """Slot i's cache as [position][Hkv][...]; nothing may be written past the sequence's end."""
    c = [np.ascontiguousarray(r[k][i].transpose(1, 0, 2)) for k in ("k_q", "k_d", "v_q", "v_d")]
    assert not any(a[tot:].any() for a in c), "the cache past the sequence's end was written"
    return [a[:tot] for a in c]


@pytest.mark.parametrize("T", sorted(PARTNER))
@pytest.mark.parametrize("Hkv,R", [(1, 1), (2, 2), (1, 4)])
@pytest.mark.parametrize("mode", list(MODES))
def test_kv4_kernels(oracle, mode, Hkv, R, T):
    """Checks 1 and 2 on slots of T and PARTNER[T] keys, kinds normal and zero_block, f32 and bf16 outputs, every kernel of the ratio."""
    from q3tts import _abi, native
    lib = _abi.load_library()
    kt = MODES[mode]
    Hq, lens = Hkv * R, [T, PARTNER[T]]
    spec = dict(name=f"kv4_{Hkv}_{R}_{T}", hook="runs", heads=(Hq, Hkv), seqs=[(0, n) for n in lens])
    shape = (N_CTX, Hq, Hkv, A.HD)
    last = np.cumsum(lens) - 1
    counts = K.Counts()
    try:
        for kind in ("normal", "zero_block"):
            xs, qn, kn = A.make_inputs(spec, kind)
            rows = np.concatenate(xs)
            assert native.k_attend_pick_kv8(0, R, N_CTX, Hkv, n_seg=2, seg_max_n=max(lens), seg_max_t=max(lens), want_code=True, kv_types=kt) == {1: 22, 2: 23, 4: 24}[R]
            run = native.k_attention_runs_kv8(rows, spec["seqs"], *shape, qn, kn, *TAIL, policy=2, kv_types=kt)
            for i, (x, tot, out) in enumerate(zip(xs, lens, A.hook_out_split(spec, run["out"]))):
                k_q, k_d, v_q, v_d = _slot(run, i, tot)
                want_q, want_d = quant4_32(x.reshape(tot, Hq + 2 * Hkv, A.HD)[:, Hq + Hkv:])
                assert np.array_equal(v_q, want_q) and np.array_equal(v_d, want_d), (kind, i, "V is not quantize_row_q4_0 of the f32 rows")
                (check_stage1_k4 if kt[0] == Q4 else K.check_stage1_k)(x, Hq, Hkv, kn, k_q, k_d, counts)
                kh, vh = dequant(k_q, k_d, kt[0]), dequant(v_q, v_d, Q4)
                ref = A.attend64(K.oracle_q(oracle, x, Hq, Hkv, qn, kn), kh, vh, 0, Hq, Hkv)
                vmax = np.repeat(np.maximum(np.abs(vh.astype(np.float64)).max(axis=(0, 2)), 1e-30), R * A.HD)
                err = float((np.abs(out.astype(np.float64) - ref) / vmax).max())
                print(f"{mode} {spec['name']} {kind} slot {i}: stage 2 error {err:.2e} (bound {ATT_STAGE2_TOL:.1e})")
                assert err <= ATT_STAGE2_TOL, (kind, i, err)
            bf = native.k_attention_runs_kv8(rows, spec["seqs"], *shape, qn, kn, *TAIL, policy=2, out_form=1, kv_types=kt)
            assert np.array_equal(bf["out"], A.bf16_bits(run["out"])), kind
            for policy, code in ([] if R == 1 else [(0, 27), (1, 25)] if R == 2 else [(0, 26), (1, 26)]):          # 2: one order
                assert lib.q3tts_k_attend_policy(policy, 0) == 0
                assert native.k_attend_pick_kv8(1, R, N_CTX, Hkv, want_code=True, kv_types=kt) == code
                dec = native.k_attention_decode_kv8(rows, lens, *shape, qn, kn, *TAIL, policy=policy, kv_types=kt)
                assert np.array_equal(A.bits(dec["out"]), A.bits(run["out"][last])), (kind, policy)
                for k in ("k_q", "k_d", "v_q", "v_d"):
                    assert np.array_equal(dec[k], run[k]), (kind, policy, k)
                db = native.k_attention_decode_kv8(rows, lens, *shape, qn, kn, *TAIL, policy=policy, out_form=1, kv_types=kt)
                assert np.array_equal(db["out"], A.bf16_bits(dec["out"])), (kind, policy)
    finally:
        lib.q3tts_k_attend_policy(0, 0)
    print(counts.line(spec["name"]))
    counts.check_caps(spec["name"])


def test_kv4_policies_are_independent():
    """What lets one key policy and one value policy serve three caches: on the same rows a Q8_0 K holds the same quants and scales beside a
    Q8_0 V and beside a Q4_0 V, and a Q4_0 V the same beside a Q8_0 K and beside a Q4_0 K — from the run kernel and from the decode step
    under both policies (the gqa2 kernel and the fused one). Slots of 65 and 257 keys: past one key block, past 256 keys, at a block edge."""
    from q3tts import _abi, native
    lib = _abi.load_library()
    Hkv, R, lens = 2, 2, [65, 257]
    Hq = Hkv * R
    spec = dict(name="kv4_pairs", hook="runs", heads=(Hq, Hkv), seqs=[(0, n) for n in lens])
    shape = (N_CTX, Hq, Hkv, A.HD)
    xs, qn, kn = A.make_inputs(spec, "normal")
    rows = np.concatenate(xs)
    pairs = (None, MODES["q8_q4"], MODES["q4_q4"])
    calls = [("runs", lambda kt: native.k_attention_runs_kv8(rows, spec["seqs"], *shape, qn, kn, *TAIL, policy=2, kv_types=kt))]
    for policy in (0, 1):
        calls.append((f"decode policy {policy}", lambda kt, p=policy: native.k_attention_decode_kv8(rows, lens, *shape, qn, kn, *TAIL, policy=p, kv_types=kt)))
    try:
        for what, call in calls:
            q8_q8, q8_q4, q4_q4 = (call(kt) for kt in pairs)
            for k in ("k_q", "k_d"):
                assert np.array_equal(q8_q8[k], q8_q4[k]), (what, k, "a Q8_0 K depends on the V beside it")
            for k in ("v_q", "v_d"):
                assert np.array_equal(q8_q4[k], q4_q4[k]), (what, k, "a Q4_0 V depends on the K beside it")
    finally:
        lib.q3tts_k_attend_policy(0, 0)


@pytest.mark.parametrize("Hkv,R", [(1, 1), (2, 2), (1, 4)])
@pytest.mark.parametrize("mode", list(MODES))
def test_grid_equals_the_oracle(oracle, mode, Hkv, R):
    """Check 3: the Q4_0 V cache holds exactly what the bf16 cache holds and every score is 0, so the value chain and the combination must
    give q3o_attention's output, all 32 bits, from every kernel."""
    from q3tts import _abi, native
    lib = _abi.load_library()
    kt = MODES[mode]
    Hq, lens = Hkv * R, [65, 257]
    spec = dict(name=f"grid_{Hkv}_{R}", hook="runs", heads=(Hq, Hkv), seqs=[(0, n) for n in lens])
    xs, qn, kn = A.make_inputs(spec, "uniform")
    rng = np.random.default_rng([A.SEED, 4, Hkv, R])
    for x in xs:
        tot = x.shape[0]
        q = rng.integers(-8, 8, size=(tot, Hkv, K.NB, 32))
        np.put_along_axis(q, rng.integers(0, 32, size=(tot, Hkv, K.NB, 1)), -8, axis=-1)
        v = np.ldexp(q.astype(np.float64), rng.integers(-6, 7, size=(tot, Hkv, K.NB, 1))).astype(np.float32)
        x.reshape(tot, Hq + 2 * Hkv, A.HD)[:, Hq + Hkv:] = v.reshape(tot, Hkv, A.HD)
    want = [K.oracle_seq(oracle, x, 0, n, Hq, Hkv, qn, kn) for x, n in zip(xs, lens)]
    shape = (N_CTX, Hq, Hkv, A.HD)
    run = native.k_attention_runs_kv8(np.concatenate(xs), spec["seqs"], *shape, qn, kn, *TAIL, policy=2, kv_types=kt)
    for i, (dev, (out, _, _, vb)) in enumerate(zip(A.hook_out_split(spec, run["out"]), want)):
        k_q, k_d, v_q, v_d = _slot(run, i, lens[i])
        assert np.array_equal(dequant(v_q, v_d, Q4), A.bf16_value(vb)) and not dequant(k_q, k_d, kt[0]).any(), i
        assert np.array_equal(A.bits(dev), A.bits(out)), i
    try:
        for policy in ([] if R == 1 else [0, 1]):
            assert lib.q3tts_k_attend_policy(policy, 0) == 0
            dec = native.k_attention_decode_kv8(np.concatenate(xs), lens, *shape, qn, kn, *TAIL, policy=policy, kv_types=kt)
            assert np.array_equal(A.bits(dec["out"]), A.bits(np.stack([w[0][-1] for w in want]))), policy
    finally:
        lib.q3tts_k_attend_policy(0, 0)


@pytest.mark.parametrize("mode", list(MODES))
def test_prefix_copy_and_save_round_trip(mode):
    """Check 4: P = 70 over two key blocks, L = 2, Hkv = 2. A store of random bytes goes into a slot (whole key blocks) and the slot's first
    P positions come back: every byte of a position < P, zeros for the keys 70 .. 127 (quants and scales) and for the values from 70 on."""
    from q3tts import native
    kt = MODES[mode]
    L, Hkv, P, NP = 2, 2, 70, 128
    rng = np.random.default_rng(70)
    stores, want = [], []
    for side, typ in enumerate(kt):
        bpp = A.HD // 2 if typ == Q4 else A.HD                       # bytes of quants per position; 16-byte units: bpp / 16
        qb, sb = L * Hkv * NP * bpp, L * Hkv * NP * K.NB * 2
        s = rng.integers(0, 256, size=qb + sb, dtype=np.uint8)
        if side == 0:   # keys: unit i of a head holds key (i & 63) of block i // (64 units per position); scale i key (i & 63) of block i // 256
            uq, us = np.arange(NP * bpp // 16), np.arange(NP * K.NB)
            keep_q = np.repeat((uq // (4 * bpp)) * 64 + (uq & 63) < P, 16)
            keep_s = np.repeat((us // (64 * K.NB)) * 64 + (us & 63) < P, 2)
        else:           # values: row-major
            keep_q, keep_s = np.repeat(np.arange(NP) < P, bpp), np.repeat(np.arange(NP) < P, K.NB * 2)
        stores.append(s)
        want.append(s * np.concatenate([np.tile(keep_q, L * Hkv), np.tile(keep_s, L * Hkv)]))
    got = native.k_kv_prefix_roundtrip_kv4(stores[0], stores[1], L, Hkv, P, 192, kt)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


# ---- engine level -----------------------------------------------------------------------------------------------------------------------
def _cfg(max_batch, n_ctx=256, kv_q8=0):
    from q3tts import _abi
    cfg = _abi.tiny_config(max_batch=max_batch, n_ctx=n_ctx)
    cfg.kv_q8_0 = kv_q8
    return cfg


def _same(got, want, what):
    assert got.status == 0 and want.status == 0 and np.array_equal(got.codes, want.codes) and got.hit_eos == want.hit_eos, what
    assert got.pcm.shape == want.pcm.shape and np.array_equal(A.bits(got.pcm), A.bits(want.pcm)), what


@pytest.mark.parametrize("mode", list(MODES))
def test_engine_results_do_not_depend_on_slots_prefix_or_session(oracle, mode):
    """Five sampled requests whose decode crosses position 64: 1 slot == 3 slots == a session; a whole prompt == the same prompt behind a
    40-row and a 64-row voice prefix; and the ids are not those of the kv_q8_0 = 1 engine (an engine that ignored the option fails)."""
    from q3tts import _abi, native
    kt = MODES[mode]
    om = oracle.OracleModel(_cfg(1).model, seed=0, n_ctx=256, n_threads=8)
    try:
        reqs = [dict(r, want_pcm=1) for r in K.batch_requests(oracle, om, 5, lo=56, hi=63, frames=(10, 14), seed=41)]
        whole = K.prompt_rows(oracle, om, 90, 7)
    finally:
        om.close()
    one, three, q8 = native.NativeEngine(_cfg(1), kv_types=kt), native.NativeEngine(_cfg(3), kv_types=kt), native.NativeEngine(_cfg(3, kv_q8=1))
    try:
        want = one.generate_batch(reqs)
        assert all(w.status == 0 and w.codes.shape[0] == r["force_eos_at"] for w, r in zip(want, reqs))
        for i, g in enumerate(three.generate_batch(reqs)):
            _same(g, want[i], (mode, "3 slots", i))
        assert any(not np.array_equal(g.codes, w.codes) for g, w in zip(q8.generate_batch(reqs), want)), "the ids are the Q8_0 cache's"
        kw = dict(temperature=0.7, top_k=40, top_p=0.9, seed=5, max_steps=12, min_frames=9, force_eos_at=9, want_pcm=1)
        full = three.generate(embd=whole, **kw)
        for P in (40, 64):
            with three.create_prefix(embd=whole[:P]) as x:
                _same(three.generate(embd=whole[P:], prefix=x, **kw), full, (mode, "prefix", P))
        s = native.NativeSession(three)
        chunks, final = {}, {}
        try:
            with pytest.raises(_abi.Q3Error, match=r"Q4_0.*kv_type_k"):
                s.set_swap(1 << 20)
            ids = [s.submit(**r) for r in reqs]
            for rid, kind, pcm, is_final, res in s.events(timeout_ms=60000):
                if kind == _abi.EV_CHUNK:
                    chunks.setdefault(rid, []).append(pcm)
                else:
                    final[rid] = res
        finally:
            s.close()
        for i, rid in enumerate(ids):
            assert np.array_equal(final[rid].codes, want[i].codes), (mode, "session", i)
            assert np.array_equal(A.bits(np.concatenate(chunks[rid])), A.bits(want[i].pcm)), (mode, "session", i)
    finally:
        for e in (one, three, q8):
            e.close()


def test_refusals_and_memory_formula():
    from q3tts import _abi, native
    for bad in ((Q4, Q8), (Q8, Q8), (Q4, 0), (0, Q4), (1, 1)):
        with pytest.raises(_abi.Q3Error, match=r"kv_type_k = .*kv_type_v = .*not an accepted pair"):
            native.NativeEngine(_cfg(1), kv_types=bad)
    with pytest.raises(_abi.Q3Error, match=r"kv_pages = 8.*kv_type_k"):
        native.NativeEngine(_cfg(1), kv_pages=8, kv_types=MODES["q4_q4"])
    with pytest.raises(_abi.Q3Error, match=r"kv_type_k.*kv_q8_0 = 1.*ambiguous"):
        native.NativeEngine(_cfg(1, kv_q8=1), kv_types=MODES["q8_q4"])
    m = _cfg(1).model
    for kt in MODES.values():                    # bytes per position and KV head: Q8_0 hd + hd / 16, Q4_0 hd / 2 + hd / 16
        got = []
        for n_ctx in (128, 256):
            eng = native.NativeEngine(_cfg(3, n_ctx=n_ctx), kv_types=kt)
            got.append(eng.device_bytes())
            eng.close()
        bf = []
        for n_ctx in (128, 256):
            eng = native.NativeEngine(_cfg(3, n_ctx=n_ctx))
            bf.append(eng.device_bytes())
            eng.close()
        per = sum(m.t_head_dim // 2 + m.t_head_dim // 16 if t == Q4 else m.t_head_dim + m.t_head_dim // 16 for t in kt)
        # (everything else that grows with n_ctx — RoPE tables, prefill rows — is the bf16 engine's: the difference of differences is the cache's)
        assert (bf[1] - bf[0]) - (got[1] - got[0]) == 3 * m.t_n_layer * m.t_n_kv_head * 128 * (4 * m.t_head_dim - per), kt

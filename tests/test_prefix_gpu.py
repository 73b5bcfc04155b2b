"""Voice prefixes (include/q3tts.h, "voice prefixes"): a prompt's voice part prefilled once, its Talker K/V copied into every slot that uses it.

The contract is bit equality with the whole prompt: a request behind prefix(V) with text T gives the codes, hit_eos and PCM of the same request
without a prefix whose desc is V with text T. The oracle for every test here is therefore the engine's own whole-prompt path (and through it
oracle/ for a few replays). The tiny shape has hd 128 and two query heads per KV head, so every attention variant is reachable through
q3tts_k_attend_policy.
"""
import ctypes as C
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N_CTX = 512   # room for prefix + suffix runs past 256 keys


def _spk(d):
    return ((np.arange(d) % 13 - 6) * 0.03125).astype(np.float32)


def _bits_equal(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def _voices(cfg):
    """name -> voice fields of make_prompt_desc: a clone voice with instruct and ref_text, a spk_id voice with no language, a spk_emb voice."""
    rng = np.random.default_rng(77)
    m = cfg.model
    return {
        "clone": dict(spk_emb=_spk(m.d_embed), lang_id=2055, instruct_ids=rng.integers(0, 151643, size=5),
                      ref_codes=rng.integers(0, m.codecq_rows, size=(21, 16)), ref_text_ids=rng.integers(0, 151643, size=9)),
        "spk_id": dict(spk_id=3000, lang_id=None),
        "spk_emb": dict(spk_emb=_spk(m.d_embed) * 0.5),
    }


def _texts(n, lo=4, hi=24, seed=5):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 151643, size=int(rng.integers(lo, hi))) for _ in range(n)]


def _attend_policy(decode, prefill):
    from q3tts import _abi
    assert _abi.load_library().q3tts_k_attend_policy(decode, prefill) == 0


def _engine(mode=0, max_batch=4, n_ctx=N_CTX, kv8=0):
    from q3tts import _abi, native
    cfg = _abi.tiny_config(max_batch=max_batch, n_ctx=n_ctx, with_vocoder=1)
    cfg.talker_q8_0, cfg.kv_q8_0 = mode, kv8
    return cfg, native.NativeEngine(cfg)


def _pairs(oracle, voice, texts, keep):
    """(whole desc, text-only desc) per text."""
    out = []
    for t in texts:
        dw, kw = oracle.make_prompt_desc(t, **voice)
        dt, kt = oracle.make_prompt_desc(t, part="text")
        keep += [dw, kw, dt, kt]
        out.append((dw, dt))
    return out


def _sampled(i, max_steps=20):
    target = 3 + (i * 5) % 13
    return dict(temperature=0.7, top_k=40, top_p=0.9, seed=300 + i, max_steps=max_steps, min_frames=target if i % 2 else 0,
                force_eos_at=target if i % 3 else -1)


def _check_same(got, want, what):
    assert got.status == 0 and want.status == 0, (what, got.status, want.status)
    assert np.array_equal(got.codes, want.codes), what
    assert got.hit_eos == want.hit_eos, what
    if want.pcm is not None:
        assert got.pcm is not None and _bits_equal(got.pcm, want.pcm), what


@pytest.fixture(scope="module")
def tiny(oracle):
    cfg, eng = _engine()
    om = oracle.OracleModel(cfg.model, seed=0, n_ctx=N_CTX, n_threads=4)
    yield cfg, eng, om
    eng.close()
    om.close()


@pytest.fixture(scope="module")
def clone_prefix(oracle, tiny):
    cfg, eng, om = tiny
    v = _voices(cfg)["clone"]
    dv, keep = oracle.make_prompt_desc(None, part="voice", **v)
    x = eng.create_prefix(desc=dv)
    yield v, x
    x.close()


# ---- 1. the prefill hook: hidden row and logits of the last row, bit for bit ------------------------------------------------------------
@pytest.mark.parametrize("name", ["clone", "spk_id", "spk_emb"])
def test_prefill_prefix_equals_whole_prompt(oracle, tiny, name):
    cfg, eng, om = tiny
    v = _voices(cfg)[name]
    dv, kv = oracle.make_prompt_desc(None, part="voice", **v)
    with eng.create_prefix(desc=dv) as x:
        for t in _texts(3, seed=len(name)):
            dw, kw = oracle.make_prompt_desc(t, **v)
            whole = eng.build_prompt(dw)
            P = x.n_rows
            assert whole.shape[0] == P + len(t) + 3
            h0, l0 = eng.talker_prefill(whole)
            h1, l1 = eng.talker_prefill_prefix(x, whole[P:])
            assert _bits_equal(h1, h0) and _bits_equal(l1, l0), name
            with eng.create_prefix(embd=whole[:P]) as xr:   # the same prefix given as host rows
                assert xr.n_rows == P
                h2, l2 = eng.talker_prefill_prefix(xr, whole[P:])
                assert _bits_equal(h2, h0) and _bits_equal(l2, l0), name
        if name == "clone":
            ins, F, R = len(v["instruct_ids"]), v["ref_codes"].shape[0], len(v["ref_text_ids"])
            assert x.n_rows == F + R + 12 + ins + 5
            h_ref, l_ref = om.talker_prefill(whole)
            assert _bits_equal(h0, h_ref) and _bits_equal(l0, l_ref)


# ---- 2. sampled requests through generate_batch --------------------------------------------------------------------------------------
def test_generate_batch_with_clone_prefix(oracle, tiny, clone_prefix):
    """8 seeded requests (min_frames / force_eos_at mixed) share one clone prefix on 4 slots: codes and PCM equal the whole prompts' bit
    for bit, and two equal the oracle's replay of the whole prompt."""
    cfg, eng, om = tiny
    v, x = clone_prefix
    keep = []
    pairs = _pairs(oracle, v, _texts(8), keep)
    want = eng.generate_batch([dict(desc=dw, want_pcm=1, **_sampled(i)) for i, (dw, dt) in enumerate(pairs)])
    got = eng.generate_batch([dict(desc=dt, prefix=x, want_pcm=1, **_sampled(i)) for i, (dw, dt) in enumerate(pairs)])
    for i in range(8):
        _check_same(got[i], want[i], i)
    assert len({g.n_frames for g in got}) > 2
    for i in (1, 6):
        ref, eos = om.generate(om.build_prompt(pairs[i][0]), **_sampled(i))
        assert np.array_equal(got[i].codes, ref) and got[i].hit_eos == eos, i


# ---- 3. two prefixes and none in one batch ------------------------------------------------------------------------------------------------
def test_generate_batch_mixes_prefixes(oracle, tiny):
    cfg, eng, om = tiny
    vs = _voices(cfg)
    keep = []
    reqs_p, reqs_w = [], []
    prefixes = []
    for j, name in enumerate(("clone", "spk_id")):
        dv, kv = oracle.make_prompt_desc(None, part="voice", **vs[name])
        keep += [dv, kv]
        prefixes.append(eng.create_prefix(desc=dv))
    texts = _texts(9, seed=9)
    for i, t in enumerate(texts):
        kind = i % 3   # 0: clone prefix, 1: spk_id prefix, 2: spk_emb voice without a prefix
        v = vs[("clone", "spk_id", "spk_emb")[kind]]
        dw, kw = oracle.make_prompt_desc(t, **v)
        keep += [dw, kw]
        reqs_w.append(dict(desc=dw, want_pcm=1, **_sampled(i)))
        if kind == 2:
            reqs_p.append(reqs_w[-1])
        else:
            dt, kt = oracle.make_prompt_desc(t, part="text")
            keep += [dt, kt]
            reqs_p.append(dict(desc=dt, prefix=prefixes[kind], want_pcm=1, **_sampled(i)))
    want = eng.generate_batch(reqs_w)
    got = eng.generate_batch(reqs_p)
    for i in range(len(texts)):
        _check_same(got[i], want[i], i)
    for x in prefixes:
        x.close()


# ---- 4. prefix lengths around the key blocks, suffixes past 128 and 256 keys, every attention variant ----------------------------------
CASES = [(1, 20), (63, 70), (64, 64), (65, 100), (130, 100), (130, 140), (65, 200)]


def test_prefix_lengths_and_attention_variants(oracle, tiny):
    cfg, eng, om = tiny
    desc, keep = oracle.make_prompt_desc(np.random.default_rng(4).integers(0, 151643, size=400), spk_emb=_spk(cfg.model.d_embed))
    pe = om.build_prompt(desc)
    assert pe.shape[0] >= 340
    base = {}
    try:
        for pol in ((0, 0), (0, 2), (1, 1)):
            _attend_policy(*pol)
            for P, n in CASES:
                whole = np.ascontiguousarray(pe[:P + n])
                with eng.create_prefix(embd=whole[:P]) as x:
                    h0, l0 = eng.talker_prefill(whole)
                    h1, l1 = eng.talker_prefill_prefix(x, whole[P:])
                    assert _bits_equal(h1, h0) and _bits_equal(l1, l0), (pol, P, n)
                    kw = dict(temperature=0.7, top_k=40, top_p=0.9, seed=P + n, max_steps=8, want_pcm=1)
                    w, g = eng.generate_batch([dict(embd=whole, **kw), dict(embd=whole[P:], prefix=x, **kw)])
                    _check_same(g, w, (pol, P, n))
                    if (P, n) in base:   # the same bits under every variant
                        hb, lb, cb = base[(P, n)]
                        assert _bits_equal(h1, hb) and _bits_equal(l1, lb) and np.array_equal(g.codes, cb), (pol, P, n)
                    else:
                        base[(P, n)] = (h1, l1, g.codes)
    finally:
        _attend_policy(0, 0)
    h_ref, l_ref = om.talker_prefill(np.ascontiguousarray(pe[:130 + 100]))
    assert _bits_equal(base[(130, 100)][0], h_ref) and _bits_equal(base[(130, 100)][1], l_ref)


# ---- 5. Q8_0 Talker modes ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [1, 2])
def test_q8_0_modes(oracle, mode):
    cfg, eng = _engine(mode)
    om = oracle.OracleModel(cfg.model, seed=0, n_ctx=N_CTX, n_threads=4)
    (om.set_talker_q8a8 if mode == 2 else om.set_talker_q8)()
    try:
        v = _voices(cfg)["clone"]
        dv, kv = oracle.make_prompt_desc(None, part="voice", **v)
        keep = []
        pairs = _pairs(oracle, v, _texts(8, seed=mode), keep)
        with eng.create_prefix(desc=dv) as x:
            whole = eng.build_prompt(pairs[0][0])
            h0, l0 = eng.talker_prefill(whole)
            h1, l1 = eng.talker_prefill_prefix(x, whole[x.n_rows:])
            assert _bits_equal(h1, h0) and _bits_equal(l1, l0)
            want = eng.generate_batch([dict(desc=dw, want_pcm=1, **_sampled(i)) for i, (dw, dt) in enumerate(pairs)])
            got = eng.generate_batch([dict(desc=dt, prefix=x, want_pcm=1, **_sampled(i)) for i, (dw, dt) in enumerate(pairs)])
            for i in range(8):
                _check_same(got[i], want[i], (mode, i))
            for i in (2, 5):
                ref, eos = om.generate(om.build_prompt(pairs[i][0]), **_sampled(i))
                assert np.array_equal(got[i].codes, ref), (mode, i)
    finally:
        eng.close()
        om.close()


# ---- 5b. the store's bytes come and go in q3tts_k_device_bytes -------------------------------------------------------------------------------
@pytest.mark.parametrize("kv8", [0, 1])
def test_destroy_gives_device_bytes_back(oracle, kv8):
    """q3tts_prefix_create adds its two stores (K and V, each the size q3tts_k_prefix_read reports) to the engine's device bytes, and
    q3tts_prefix_destroy takes exactly them off again, in the bf16 and the Q8_0 cache format."""
    cfg, eng = _engine(kv8=kv8)
    try:
        dv, keep = oracle.make_prompt_desc(None, part="voice", spk_id=3000, lang_id=None)
        b0 = eng.device_bytes()
        x = eng.create_prefix(desc=dv)
        n = C.c_int64(0)
        assert x.lib.q3tts_k_prefix_read(x.h, None, None, 0, C.byref(n)) == 0 and n.value > 0
        assert eng.device_bytes() == b0 + 2 * n.value
        x.close()
        assert eng.device_bytes() == b0
    finally:
        eng.close()


# ---- 6. streams and sessions -------------------------------------------------------------------------------------------------------------
def test_stream_and_session_with_prefixes(oracle, tiny, clone_prefix):
    from q3tts import _abi, native
    cfg, eng, om = tiny
    v, x = clone_prefix
    vs = _voices(cfg)
    dv2, kv2 = oracle.make_prompt_desc(None, part="voice", **vs["spk_emb"])
    keep = []
    with eng.create_prefix(desc=dv2) as x2:
        texts = _texts(8, seed=66)
        reqs = []
        for i, t in enumerate(texts):
            which = (x, v) if i % 2 == 0 else (x2, vs["spk_emb"])
            dt, kt = oracle.make_prompt_desc(t, part="text")
            dw, kw = oracle.make_prompt_desc(t, **which[1])
            keep += [dt, kt, dw, kw]
            reqs.append((dict(desc=dt, prefix=which[0], **_sampled(i)), dict(desc=dw, **_sampled(i))))
        want = eng.generate_batch([dict(w, want_pcm=1) for p, w in reqs])
        got = eng.generate_batch([dict(p, want_pcm=1) for p, w in reqs])
        for i in range(len(reqs)):
            _check_same(got[i], want[i], i)
        for i in (0, 3):   # q3tts_stream_*
            chunks = [c for c, _ in native.stream_chunks(eng, **dict(reqs[i][0], want_pcm=1))]
            assert _bits_equal(np.concatenate(chunks), want[i].pcm), i
            assert np.array_equal(eng.last_stream_result.codes, want[i].codes)
        with native.NativeSession(eng) as sess:   # submits at different times: three at once, the rest after the first chunk
            ids = [sess.submit(**p) for p, w in reqs[:3]]
            parts = {}
            first = sess.next(60000)
            assert first is not None
            evs = [first]
            ids += [sess.submit(**p) for p, w in reqs[3:]]
            evs += list(sess.events(120000))
            assert not sess._open
            for rid, kind, pcm, fin, res in evs:
                g = parts.setdefault(rid, dict(chunks=[], res=None))
                if kind == _abi.EV_CHUNK:
                    g["chunks"].append(pcm)
                else:
                    assert kind == _abi.EV_DONE, kind
                    g["res"] = res
        for i, rid in enumerate(ids):
            g = parts[rid]
            assert np.array_equal(g["res"].codes, want[i].codes), i
            assert _bits_equal(np.concatenate(g["chunks"]), want[i].pcm), i


# ---- 7. errors: each fails alone and the engine still serves ---------------------------------------------------------------------------
def test_errors(oracle, tiny, clone_prefix):
    from q3tts import _abi, native
    cfg, eng, om = tiny
    v, x = clone_prefix
    lib = eng.lib
    keep = []
    (dw, dt), = _pairs(oracle, v, _texts(1, seed=12), keep)
    good = dict(desc=dt, prefix=x, want_pcm=1, **_sampled(1))
    want = eng.generate_batch([dict(desc=dw, want_pcm=1, **_sampled(1))])[0]

    def still_serves():
        _check_same(eng.generate_batch([good])[0], want, "after an error")

    # a prefix of another engine
    cfg2, eng2 = _engine(max_batch=1, n_ctx=256)
    try:
        dv, kv = oracle.make_prompt_desc(None, part="voice", **v)
        x_other = eng2.create_prefix(desc=dv)
        out = eng.generate_batch([dict(good, prefix=x_other), good])
        assert out[0].status == -1
        assert "another engine" in lib.q3tts_last_error(eng.h).decode()
        _check_same(out[1], want, "beside a foreign prefix")
        x_other.close()
    finally:
        eng2.close()
    still_serves()

    # voice fields set together with a prefix: each is named
    spk = _spk(cfg.model.d_embed)
    u32 = np.arange(3, dtype=np.uint32)
    codes = np.zeros((2, 16), dtype=np.int32)
    keep += [spk, u32, codes]
    for field, setv in (("instruct_ids", lambda d: setattr(d, "instruct_ids", u32.ctypes.data_as(C.POINTER(C.c_uint32)))),
                        ("lang_id", lambda d: setattr(d, "lang_id", 2055)),
                        ("spk_id", lambda d: setattr(d, "spk_id", 3000)),
                        ("spk_emb", lambda d: setattr(d, "spk_emb", spk.ctypes.data_as(C.POINTER(C.c_float)))),
                        ("ref_codes", lambda d: setattr(d, "ref_codes", codes.ctypes.data_as(C.POINTER(C.c_int32)))),
                        ("ref_text_ids", lambda d: setattr(d, "ref_text_ids", u32.ctypes.data_as(C.POINTER(C.c_uint32))))):
        d, kd = oracle.make_prompt_desc(_texts(1, seed=13)[0], part="text")
        setv(d)
        out = eng.generate_batch([dict(good, desc=d)])[0]
        assert out.status == -1, field
        assert field in lib.q3tts_last_error(eng.h).decode(), field
    still_serves()

    # prefix + prompt + max_steps > n_ctx fails that request only, in a batch and in a session
    long_t = np.arange(N_CTX - x.n_rows - 3 - 10, dtype=np.uint32) % 151643
    dl, kl = oracle.make_prompt_desc(long_t, part="text")
    keep += [dl, kl]
    over = dict(good, desc=dl, max_steps=20)
    out = eng.generate_batch([over, good])
    assert out[0].status == -1 and "n_ctx" in lib.q3tts_last_error(eng.h).decode()
    _check_same(out[1], want, "beside an oversized request")
    with native.NativeSession(eng) as sess:
        bad_id, ok_id = sess.submit(**over), sess.submit(**good)
        finals = {rid: (kind, res) for rid, kind, pcm, fin, res in sess.events(60000) if kind != _abi.EV_CHUNK}
        assert finals[bad_id][0] == _abi.EV_FAILED and finals[bad_id][1].status == -1
        assert finals[ok_id][0] == _abi.EV_DONE and np.array_equal(finals[ok_id][1].codes, want.codes)
        # create / destroy while the session owns the engine
        dv, kv = oracle.make_prompt_desc(None, part="voice", **v)
        h = C.c_void_p()
        assert lib.q3tts_prefix_create(eng.h, C.byref(dv), None, 0, C.byref(h)) == -5 and not h.value
        assert lib.q3tts_prefix_destroy(x.h) == -5
    still_serves()

    # a node refuses requests with a prefix
    node = native.NativeNode(_abi.tiny_config(max_batch=1, n_ctx=256, with_vocoder=0), [0])
    try:
        with pytest.raises(_abi.Q3Error, match=r"\(-1\)"):
            node.generate_batch([good])
    finally:
        node.close()
    still_serves()


# ---- full shape ------------------------------------------------------------------------------------------------------------------------
def test_full_shape_64_slots_clone_prefix(oracle):
    """The benchmarked shape: 64 requests in one cloned voice (95-row voice part: 63 reference frames, 20 reference-text tokens, a language)
    with texts of 10-60 tokens on 64 slots. Codes equal the whole-prompt run; three equal the oracle's replay."""
    from q3tts import _abi, native
    cfg = _abi.full_config_py()
    cfg.max_batch, cfg.n_ctx, cfg.max_steps_cap, cfg.with_vocoder = 64, 256, 32, 0
    threads = min(16, os.cpu_count() or 4)
    eng = native.NativeEngine(cfg)
    om = None
    try:
        with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "speakers", "vivian.json")) as f:
            spk = np.asarray(json.load(f)["spk_emb"], dtype=np.float32)
        rng = np.random.default_rng(9595)
        v = dict(spk_emb=spk, lang_id=2055, ref_codes=rng.integers(0, 2048, size=(63, 16)), ref_text_ids=rng.integers(0, 151643, size=20))
        dv, kv = oracle.make_prompt_desc(None, part="voice", **v)
        keep = []
        texts = [rng.integers(0, 151643, size=int(rng.integers(10, 61))) for _ in range(64)]
        pairs = _pairs(oracle, v, texts, keep)
        kws = [dict(temperature=0.7, top_k=40, top_p=0.9, seed=5000 + i, max_steps=16, min_frames=4 + i % 9, force_eos_at=4 + i % 9)
               for i in range(64)]
        with eng.create_prefix(desc=dv) as x:
            assert x.n_rows == 95
            want = eng.generate_batch([dict(desc=dw, **kw) for (dw, dt), kw in zip(pairs, kws)])
            got = eng.generate_batch([dict(desc=dt, prefix=x, **kw) for (dw, dt), kw in zip(pairs, kws)])
        for i in range(64):
            _check_same(got[i], want[i], i)
        om = oracle.OracleModel(cfg.model, seed=0, n_ctx=256, n_threads=threads)
        for i in sorted(range(64), key=lambda i: len(texts[i]))[:3]:
            ref, _ = om.generate(om.build_prompt(pairs[i][0]), **kws[i])
            assert np.array_equal(got[i].codes, ref), i
    finally:
        eng.close()
        if om is not None:
            om.close()


# ---- the reference-style API -----------------------------------------------------------------------------------------------------------
def test_api_voice_prefix():
    """TtsEngine.voice_prefix + prefix= on generate_batch_with_voice / generate_with_voice / stream_batch_with_voice: the same audio, bit for
    bit, as the calls without it; a prefix of another voice or instruct is refused."""
    from q3tts import _abi, api
    cfg = _abi.tiny_config(max_batch=4, n_ctx=256, with_vocoder=1)
    eng = api.TtsEngine(cfg)
    try:
        eng.set_max_steps(12)
        eng.set_sampler_config(api.SamplerConfig(temperature=0.7, top_k=40, top_p=0.9, seed=11))
        rng = np.random.default_rng(31)
        voice = api.VoiceFile.new([int(i) for i in rng.integers(0, 151643, size=6)], [int(c) for c in rng.integers(0, 64, size=12 * 16)],
                                  _spk(cfg.model.d_embed).tolist())
        other = api.VoiceFile.new("", [], (_spk(cfg.model.d_embed) * 0.25).tolist())
        ins = [5, 6, 7]
        texts = [list(t) for t in _texts(5, seed=31)]
        seeds = [40 + i for i in range(5)]
        want = eng.generate_batch_with_voice(texts, [voice] * 5, [ins] * 5, seeds)
        with eng.voice_prefix(voice, ins) as x:
            got = eng.generate_batch_with_voice(texts, [voice] * 5, [ins] * 5, seeds, prefix=x)
            for w, g in zip(want, got):
                assert _bits_equal(g.samples, w.samples)
            one = eng.generate_with_voice(texts[0], voice, ins, prefix=x)
            assert _bits_equal(one.samples, eng.generate_with_voice(texts[0], voice, ins).samples)
            parts = {}
            for i, pcm, fin in eng.stream_batch_with_voice(texts, [voice] * 5, [ins] * 5, seeds, prefix=x):
                parts.setdefault(i, []).append(pcm)
            for i in range(5):
                assert _bits_equal(np.concatenate(parts[i]), want[i].samples), i
            with pytest.raises(ValueError):
                eng.generate_batch_with_voice(texts[:1], [other], [ins], prefix=x)
            with pytest.raises(ValueError):
                eng.generate_batch_with_voice(texts[:1], [voice], [None], prefix=x)
    finally:
        eng.close()

"""Long documents on the GPU (include/q3tts.h, "long documents"): k_pcm_edges and k_pcm_join against the numpy
restatement bit for bit (tests/_long_ref.py), q3tts_pcm_join on host clips, and q3tts_generate_long on a tiny engine with fewer slots
than segments: against the join of q3tts_generate_batch's PCM, with a voice desc and with a prefix, trimmed, with identity options, with
a speed and an output rate, on engines of other slot counts, and its refusals."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _long_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

INVALID, STATE = -1, -5
LENS = [0, 1, 239, 240, 241, 479, 481, 7680, 23057]
STRIDE = 23059  # odd: every row has another 16-byte alignment
THR = np.float32(0.01)
N_KINDS = 6     # zeros, noise, loud at 0, loud at n - 1, loud on a block boundary, peaks equal to the threshold


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _kernel_rows():
    """Per length six rows, content kind by kind, so that rows without a loud block lie between the others; NaN behind every valid length."""
    rng = np.random.default_rng(26)
    lens = np.repeat(np.array(LENS, dtype=np.int64), N_KINDS)
    x = np.full((lens.size, STRIDE), np.nan, dtype=np.float32)
    for r, n in enumerate(lens):
        kind = r % N_KINDS
        row = (rng.uniform(-0.004, 0.004, n)).astype(np.float32)   # below the threshold
        if kind == 0:
            row[:] = 0.0
        elif kind == 1:
            row = rng.uniform(-1.0, 1.0, n).astype(np.float32)
        elif kind == 2 and n:
            row[0] = 0.5
        elif kind == 3 and n:
            row[n - 1] = -0.5
        elif kind == 4 and n:
            row[min(R.W * max(1, (n // R.W) // 2), n - 1)] = 0.25   # the first sample of a block (or the row's last sample, when it is shorter)
            if n > R.W:
                row[R.W - 1] = -0.25                                # and the last sample of block 0
        elif kind == 5 and n:
            row[::97] = THR
            row[50::131] = -THR
        x[r, :n] = row
    return x, lens


@pytest.fixture(scope="module")
def kernel_rows():
    from q3tts import native
    x, lens = _kernel_rows()
    edges = native.k_pcm_edges(x, lens, THR)
    return x, lens, edges


def test_edges_kernel_equals_restatement(kernel_rows):
    x, lens, edges = kernel_rows
    want = [R.loud_edges(x[r, :n], THR) for r, n in enumerate(lens)]
    assert [tuple(e) for e in edges] == want
    none = (2**31 - 1, -1)
    assert all(want[r] == none for r in range(lens.size) if r % N_KINDS in (0, 5) or lens[r] == 0)
    assert all(want[r] != none for r in range(lens.size) if r % N_KINDS in (1, 2, 3, 4) and lens[r] > 0)
    from q3tts import native
    # another threshold over the same rows: exactly the peak is not loud, just below it is
    e2 = native.k_pcm_edges(x, lens, 0.5)
    assert [tuple(e) for e in e2] == [R.loud_edges(x[r, :n], 0.5) for r, n in enumerate(lens)]
    assert all(tuple(e2[r]) == none for r in range(lens.size) if r % N_KINDS in (2, 3))


@pytest.mark.parametrize("trim", [0, 1])
def test_join_kernel_equals_restatement(kernel_rows, trim):
    """Every output sample, lo, hi, the offsets and N; NaN stays behind N. Kinds cycle 0..4 over rows of which every sixth is all zeros."""
    from q3tts import native
    x, lens, edges = kernel_rows
    rows = [x[r, :n] for r, n in enumerate(lens)]
    kinds = [r % 5 for r in range(lens.size)]
    cap = int(lens.sum()) + lens.size * 14400 + 8
    for keep in ((480,) if not trim else (0, 480, 10**6)):
        for fade in (0, 1, 120, 10**6):
            for pauses in ((0, 0, 0, 0, 0), (0, 0, 150, 300, 600)):
                kw = dict(trim=trim, threshold=float(THR), keep=keep, fade=fade, pause_ms=pauses)
                J, plan, N = R.join(rows, kinds, **kw)
                out, got_plan, got_N = native.k_pcm_join(x, lens, kinds, edges, cap, **kw)
                assert got_N == N and np.array_equal(got_plan, plan), kw
                assert np.array_equal(_bits(out[:N]), _bits(J)), (kw, np.flatnonzero(_bits(out[:N]) != _bits(J))[:4])
                assert np.all(np.isnan(out[N:])), kw
                if trim and keep == 0 and not any(pauses):
                    assert 0 < N < int(lens.sum())   # (trimming happened)


# ---- the engine ---------------------------------------------------------------------------------------------------------------
MAX_STEPS = [4, 5, 8, 12, 4, 9, 1]
KINDS = [3, 2, 4, 1, 3, 2, 0]
SAMPLER = dict(temperature=0.7, top_k=40, top_p=0.9, min_frames=64)   # EOS masked: every segment runs to its max_steps
SEED = 900


def _segments():
    return [(np.arange(100 + 10 * i, 105 + 11 * i, dtype=np.uint32), k, m) for i, (k, m) in enumerate(zip(KINDS, MAX_STEPS))]


def _voice(cfg):
    from q3tts import native
    d = cfg.model.d_embed
    return native.make_prompt_desc(None, spk_emb=((np.arange(d) % 13 - 6) * 0.03125).astype(np.float32), part="voice")


def _batch(eng, px, want_pcm=1):
    """The seven segments as plain requests behind the prefix px."""
    from q3tts import native
    reqs, keep = [], []
    for i, (ids, _, ms) in enumerate(_segments()):
        desc, k = native.make_prompt_desc(ids, part="text")
        keep.append(k)
        reqs.append(dict(desc=desc, prefix=px, seed=SEED + i, max_steps=ms, want_pcm=want_pcm, **SAMPLER))
    return eng.generate_batch(reqs)


@pytest.fixture(scope="module")
def doc():
    from q3tts import _abi, native
    cfg = _abi.tiny_config(max_batch=2, n_ctx=256, with_vocoder=1)
    eng = native.NativeEngine(cfg)
    vdesc, vkeep = _voice(cfg)
    px = eng.create_prefix(desc=vdesc)
    outs = _batch(eng, px)
    assert [o.status for o in outs] == [0] * 7 and [o.codes.shape[0] for o in outs] == MAX_STEPS
    pcm = [o.pcm for o in outs]
    yield dict(cfg=cfg, eng=eng, vdesc=vdesc, px=px, pcm=pcm, outs=outs, keep=vkeep)
    px.close()
    eng.close()


def _long(eng, voice=None, prefix=None, **kw):
    return eng.generate_long(_segments(), voice=voice, prefix=prefix, seed=SEED, **SAMPLER, **kw)


def _check_doc(res, d, J, plan, N, speed=0, rate=0):
    assert res.status == 0 and res.n_samples == res.pcm.size and res.n_truncated == 7
    assert [f["status"] for f in res.info] == [0] * 7 and [f["n_frames"] for f in res.info] == MAX_STEPS
    assert [f["hit_eos"] for f in res.info] == [0] * 7 and [f["n_native"] for f in res.info] == [p.size for p in d["pcm"]]
    assert [(f["lo"], f["hi"], f["begin"], f["end"]) for f in res.info] == [tuple(int(v) for v in p) for p in plan]
    assert [(f["out_begin"], f["out_end"]) for f in res.info] == R.out_maps(plan, speed, rate)
    assert res.info[-1]["out_end"] <= res.n_samples or N == 0


def test_generate_long_equals_the_join_of_the_batch(doc):
    """Seven segments on two slots, lengths that are no multiples of the 4-frame chunk: the document is the restated join of the PCM
    generate_batch returns for the same requests; a voice desc and a prefix made from it give the same bits; the device PCM flag is as
    it was (off: a want_pcm = 2 request is still refused; on: it still runs)."""
    from q3tts import _abi
    d = doc
    eng = d["eng"]
    J, plan, N = R.join(d["pcm"], KINDS)
    a = _long(eng, voice=d["vdesc"])
    b = _long(eng, prefix=d["px"])
    for res in (a, b):
        assert res.sample_rate == 24000 and res.n_samples == N and np.array_equal(_bits(res.pcm), _bits(J))
        _check_doc(res, d, J, plan, N)
    assert a.info == b.info and a.join_ms >= 0 and a.generate_ms > 0
    with pytest.raises(_abi.Q3Error):
        _batch(eng, d["px"], want_pcm=2)   # device PCM is still off
    eng.set_device_pcm(True)
    try:
        c = _long(eng, prefix=d["px"])
        assert np.array_equal(_bits(c.pcm), _bits(J))
        assert [o.status for o in _batch(eng, d["px"], want_pcm=2)] == [0] * 7   # ... and still on
    finally:
        eng.set_device_pcm(False)
    d["J"], d["plan"], d["N"] = J, plan, N


def test_trimmed(doc):
    """The threshold is a value of the segments' own |PCM|: the quietest peak among their first and last blocks, which (the comparison
    being strict) takes that block away and leaves no segment empty. Then a threshold above every sample: an empty document."""
    d = doc
    eng = d["eng"]

    def peaks(x):
        nb = -(-x.size // R.W)
        a = np.zeros(nb * R.W, dtype=np.float32)
        a[:x.size] = np.abs(x)
        return a.reshape(nb, R.W).max(axis=1)
    thr = float(min(min(peaks(x)[0], peaks(x)[-1]) for x in d["pcm"]))
    kw = dict(trim=1, threshold=thr, keep=0, fade=120)
    J, plan, N = R.join(d["pcm"], KINDS, **kw)
    assert all(hi > lo for lo, hi, _, _ in plan), "precondition: no segment is empty"
    assert any(lo > 0 or hi < x.size for (lo, hi, _, _), x in zip(plan, d["pcm"])), "precondition: something is trimmed"
    res = _long(eng, prefix=d["px"], join=kw)
    assert res.n_samples == N and np.array_equal(_bits(res.pcm), _bits(J))
    _check_doc(res, d, J, plan, N)
    top = float(max(np.abs(x).max() for x in d["pcm"])) * 2.0
    res = _long(eng, prefix=d["px"], join=dict(threshold=top))
    assert res.n_samples == 0 and res.pcm.size == 0 and all(f["begin"] == f["end"] == 0 and f["lo"] == f["hi"] == 0 for f in res.info)


def test_identity_options_concatenate(doc):
    d = doc
    res = _long(d["eng"], voice=d["vdesc"], join=dict(trim=0, fade=0, pause_ms=(0,) * 5))
    want = np.concatenate(d["pcm"])
    assert res.n_samples == want.size and np.array_equal(_bits(res.pcm), _bits(want))


def test_speed_and_rate(doc):
    d = doc
    eng = d["eng"]
    J, plan, N = R.join(d["pcm"], KINDS)
    want = eng.resample(eng.time_stretch(J, 1250), 24000, 8000)
    res = _long(eng, prefix=d["px"], speed_permille=1250, output_rate=8000)
    assert res.sample_rate == 8000 and res.n_samples == want.size and np.array_equal(_bits(res.pcm), _bits(want))
    _check_doc(res, d, J, plan, N, 1250, 8000)
    assert res.info[-1]["out_end"] <= res.n_samples
    only = _long(eng, prefix=d["px"], speed_permille=800)
    assert only.sample_rate == 24000 and np.array_equal(_bits(only.pcm), _bits(eng.time_stretch(J, 800)))
    only = _long(eng, prefix=d["px"], output_rate=48000, speed_permille=1000)
    assert only.sample_rate == 48000 and np.array_equal(_bits(only.pcm), _bits(eng.resample(J, 24000, 48000)))
    assert eng.get_speed() == 0 and eng.get_output_rate() == 0


@pytest.mark.parametrize("slots", [1, 4])
def test_independent_of_the_slot_count(doc, slots):
    from q3tts import _abi, native
    d = doc
    J, plan, N = R.join(d["pcm"], KINDS)
    eng = native.NativeEngine(_abi.tiny_config(max_batch=slots, n_ctx=256, with_vocoder=1))
    try:
        vdesc, keep = _voice(eng.cfg)
        res = _long(eng, voice=vdesc)
        assert res.n_samples == N and np.array_equal(_bits(res.pcm), _bits(J))
        _check_doc(res, d, J, plan, N)
    finally:
        eng.close()


def test_pcm_join_on_host_clips(doc, kernel_rows):
    """q3tts_pcm_join == the restatement, on the kernel test's rows (every third) and on the engine's own PCM; its edges add up to N."""
    from q3tts import native
    x, lens, _ = kernel_rows
    eng = doc["eng"]
    clips = [x[r, :n] for r, n in enumerate(lens)][::3]
    kinds = [r % 5 for r in range(len(clips))]
    for kw in (dict(threshold=float(THR)), dict(threshold=float(THR), keep=0, fade=7, pause_ms=(5, 4, 3, 2, 1)), dict(trim=0)):
        J, plan, N = R.join(clips, kinds, **kw)
        out, edges = eng.pcm_join(clips, kinds, **kw)
        assert out.size == N and np.array_equal(_bits(out), _bits(J)) and np.array_equal(edges, plan)
        kept = [(b, e) for _, _, b, e in edges if e > b]
        assert kept[-1][1] == N and all(e - b == hi - lo for lo, hi, b, e in edges)
    J, plan, N = R.join(doc["pcm"], KINDS)
    out, edges = native.pcm_join(eng, doc["pcm"], KINDS)
    assert np.array_equal(_bits(out), _bits(J)) and np.array_equal(edges, plan)


def test_refusals(doc):
    from q3tts import _abi, native
    d = doc
    eng, px, vdesc = d["eng"], d["px"], d["vdesc"]
    before = _batch(eng, px)
    assert all(np.array_equal(_bits(o.pcm), _bits(p)) for o, p in zip(before, d["pcm"]))

    def same_batch():   # a plain batch still gives the bits it gave before
        after = _batch(eng, px)
        assert all(np.array_equal(o.codes, p.codes) and np.array_equal(_bits(o.pcm), _bits(p.pcm)) for o, p in zip(after, before))

    def refused(status, match=None, engine=eng, segments=None, check=True, **kw):
        with pytest.raises(_abi.Q3Error, match=match) as ex:
            engine.generate_long(_segments() if segments is None else segments, seed=SEED, **SAMPLER, **kw)
        assert ex.value.status == status and ex.value.pcm_is_null
        if engine is eng and check:
            same_batch()

    with native.NativeSession(eng) as sess:
        refused(STATE, "session", check=False, prefix=px)
        assert sess is not None
    same_batch()
    eng.set_speed(1250)
    try:
        refused(STATE, "q3tts_set_speed", check=False, prefix=px)
        assert eng.get_speed() == 1250
    finally:
        eng.set_speed(0)
    same_batch()
    eng.set_output_rate(8000)
    try:
        refused(STATE, "q3tts_set_output_rate", check=False, prefix=px)
        assert eng.get_output_rate() == 8000
    finally:
        eng.set_output_rate(0)
    same_batch()
    refused(INVALID, "exactly one", voice=vdesc, prefix=px)
    refused(INVALID, "exactly one")
    refused(INVALID, "break kind", prefix=px, segments=[(np.arange(100, 105), 5, 4)])
    refused(INVALID, "n_segs", prefix=px, segments=[])
    refused(INVALID, "speed", prefix=px, speed_permille=499)
    refused(INVALID, "rate", prefix=px, output_rate=3999)
    refused(INVALID, "threshold", prefix=px, join=dict(threshold=-1.0))
    bare = native.NativeEngine(_abi.tiny_config(max_batch=2, n_ctx=256, with_vocoder=0))
    try:
        vd, keep = _voice(bare.cfg)
        refused(INVALID, "with_vocoder", engine=bare, voice=vd)
    finally:
        bare.close()
    # a segment that fails by itself (prefix rows + its own + max_steps > n_ctx): its status comes back, every status is set, no PCM
    segs = _segments()
    segs[2] = (np.arange(100, 350, dtype=np.uint32), 3, 8)
    with pytest.raises(_abi.Q3Error, match="segment 2") as ex:
        eng.generate_long(segs, prefix=px, seed=SEED, **SAMPLER)
    err = ex.value
    assert err.status != 0 and err.pcm_is_null and len(err.info) == 7
    assert [f["status"] for f in err.info] == [0, 0, err.status, 0, 0, 0, 0]
    after = _batch(eng, px)
    assert all(np.array_equal(_bits(o.pcm), _bits(p.pcm)) for o, p in zip(after, before))
    res = _long(eng, prefix=px)   # and the engine still makes the document
    J, plan, N = R.join(d["pcm"], KINDS)
    assert np.array_equal(_bits(res.pcm), _bits(J))

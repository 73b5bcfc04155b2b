"""The device time-stretch on the GPU: k_pcm_tempo against the numpy restatement bit for bit (tests/_tempo_ref.py),
q3tts_time_stretch, the engine's speed through generate_batch, streams and sessions (f32 and i16), with an output rate on top, through a
paced session whose requests are swapped out between chunks, turned off again, and the setter's refusals."""
import os
import sys
from collections import defaultdict

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _tempo_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

INVALID, STATE = -1, -5
FINAL_LENS = [1, 255, 256, 639, 640, 641, 7680, 7681, 23057]
STEPS = [640, 641, 7680, 15360]
STRIDE = 23059  # odd: every row has another 16-byte alignment


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _i16(pcm):
    return np.trunc(np.clip(np.asarray(pcm, dtype=np.float32) * np.float32(32767), -32768, 32767)).astype(np.int16)


def _kernel_rows():
    """Per final length a row of seeded noise, a tone and zeros; NaN behind every valid length."""
    rng = np.random.default_rng(11)
    lens = np.array(FINAL_LENS * 3, dtype=np.int64)
    x = np.full((lens.size, STRIDE), np.nan, dtype=np.float32)
    for r, n in enumerate(lens):
        kind = r // len(FINAL_LENS)
        x[r, :n] = (rng.uniform(-1.0, 1.0, n), R.tone(220.0, n), np.zeros(n))[kind]
    return x, lens


def _check_steps(x, lens_steps, final, s, ref):
    """The hook over the steps against the finished restatement `ref`: after every step a row holds exactly valid(len) outputs, each the
    one-shot bits, and nothing else of the row was written; every decided frame's offset is the restatement's."""
    from q3tts import native
    cap = ref.y.shape[1]
    dcap = max(len(d) for d in ref.delta) + 1
    out, nv, dl = native.k_pcm_tempo(x, lens_steps, final, s, cap, dcap)
    for t, ln in enumerate(lens_steps):
        for r in range(x.shape[0]):
            fin = bool(final[r]) and t == len(lens_steps) - 1
            v = R.valid(int(ln[r]), s, fin)
            assert nv[t, r] == v
            assert np.array_equal(_bits(out[t, r, :v]), _bits(ref.y[r, :v])), (s, t, r, np.flatnonzero(_bits(out[t, r, :v]) != _bits(ref.y[r, :v]))[:4])
            assert np.all(np.isnan(out[t, r, v:])), (s, t, r)
    for r in range(x.shape[0]):
        k = R.frames(int(lens_steps[-1][r]), s, bool(final[r]))
        assert list(dl[r, :k]) == ref.delta[r][:k], (s, r)
        assert np.all(dl[r, k:] == 0x7F7F7F7F)


@pytest.mark.parametrize("s", [500, 800, 1001, 1250, 2000])
def test_kernel_equals_restatement(s):
    """Rows of 1 .. 23057 samples (below, at and above the hop, the hold-back and a chunk; the long one several hundred frames), noise, a
    tone and zeros (every sum ties: the first maximum, offset -128, must win), fed in one step and in the steps 640 / 641 / 7680 / 15360 /
    final."""
    x, lens = _kernel_rows()
    ref = R.Tempo(x, s)
    ref.feed(lens, [True] * lens.size)
    zero_rows = range(2 * len(FINAL_LENS), 3 * len(FINAL_LENS))
    assert all(d == R.DMIN for r in zero_rows for d in ref.delta[r][1:]) and len(ref.delta[zero_rows[-1]]) > 40
    final = np.ones(lens.size, dtype=np.int32)
    _check_steps(x, [lens], final, s, ref)
    _check_steps(x, [np.minimum(lens, st) for st in STEPS] + [lens], final, s, ref)


def test_kernel_many_rows_in_one_launch():
    """64 rows in one launch, their lengths all different, some empty, some left unfinished; then 65 rows (two launches per step)."""
    rng = np.random.default_rng(12)
    for rows in (64, 65):
        lens = rng.permutation(np.arange(rows) * 47 % 3001)
        lens[[3, 17, 40]] = 0
        x = np.full((rows, 3001), np.nan, dtype=np.float32)
        for r, n in enumerate(lens):
            x[r, :n] = rng.uniform(-1.0, 1.0, n)
        final = (np.arange(rows) % 3 != 0).astype(np.int32)
        ref = R.Tempo(x, 1250)
        ref.feed(lens, final.astype(bool))
        part = ref.y.copy()
        ref.feed(lens, [True] * rows)   # (the prefix an unfinished row holds is the finished row's)
        assert np.array_equal(np.isnan(part) | (_bits(part) == _bits(ref.y)), np.ones_like(part, dtype=bool))
        _check_steps(x, [lens // 2, lens], final, 1250, ref)


@pytest.fixture(scope="module")
def engines():
    from q3tts import _abi, native
    cfg = _abi.tiny_config(max_batch=4, n_ctx=256, with_vocoder=1)
    eng_s, eng_n = native.NativeEngine(cfg), native.NativeEngine(cfg)
    d = cfg.model.d_embed
    desc, keep = native.make_prompt_desc(np.arange(100, 112), spk_emb=((np.arange(d) % 13 - 6) * 0.03125).astype(np.float32))
    pe = eng_n.build_prompt(desc)
    frames = [12, 16, 13, 20, 12, 17]  # six requests over four slots: refilled slots; three chunks or more before the last
    reqs = [dict(embd=pe, temperature=0.7, top_k=40, top_p=0.9, seed=500 + i, max_steps=24, min_frames=f, force_eos_at=f)
            for i, f in enumerate(frames)]
    native_out = eng_n.generate_batch([dict(r, want_pcm=1) for r in reqs])
    assert [o.codes.shape[0] for o in native_out] == frames
    bounds = [np.cumsum([c.size for c, _ in g["chunks"]]).tolist() for g in _session(eng_n, reqs, _abi.PCM_F32)]
    yield cfg, eng_s, eng_n, reqs, native_out, bounds
    eng_s.close()
    eng_n.close()


def _session(eng, reqs, fmt):
    from q3tts import _abi, native
    got = {}
    with native.NativeSession(eng, fmt) as sess:
        ids = [sess.submit(**r) for r in reqs]
        for rid, kind, pcm, fin, res in sess.events(120000):
            g = got.setdefault(rid, dict(chunks=[], res=None))
            if kind == _abi.EV_CHUNK:
                assert g["res"] is None
                g["chunks"].append((pcm, fin))
            else:
                assert kind == _abi.EV_DONE and res.status == 0
                g["res"] = res
        assert not sess._open, "events timed out"
    return [got[i] for i in ids]


@pytest.mark.parametrize("s", [800, 1500])
def test_one_shot_time_stretch_equals_restatement(engines, s):
    from q3tts import _abi
    cfg, eng_s, eng_n, reqs, native_out, bounds = engines
    n = 20001
    x = (0.5 * np.sin(2 * np.pi * 180.0 * np.arange(n) / 24000.0) + 0.05 * np.random.default_rng(5).standard_normal(n)).astype(np.float32)
    y = eng_n.time_stretch(x, s)
    want, _ = R.stretch(x, s)
    assert y.size == R.N_t(n, s) == want.size and np.array_equal(_bits(y), _bits(want))
    assert eng_n.time_stretch(np.zeros(0, np.float32), s).size == 0
    for bad in (499, 1000, 2001):
        with pytest.raises(_abi.Q3Error):
            eng_n.time_stretch(x[:100], bad)


@pytest.mark.parametrize("s", [800, 1500])
def test_engine_speed(engines, s):
    """generate_batch at a speed == q3tts_time_stretch of the unstretched PCM of an engine without one (codes equal); session chunks (f32
    and i16) and stream chunks, joined, equal that PCM bit for bit, a chunk that is not the last carrying D_t(ns) - delivered samples."""
    from q3tts import _abi, native
    cfg, eng_s, eng_n, reqs, native_out, bounds = engines
    want = [eng_n.time_stretch(o.pcm, s) for o in native_out]
    # the restatement on the engine's own PCM, for the longest utterance
    assert np.array_equal(_bits(want[3]), _bits(R.stretch(native_out[3].pcm, s)[0]))
    assert eng_s.get_speed() == 0
    eng_s.set_speed(s)
    try:
        assert eng_s.get_speed() == s
        outs = eng_s.generate_batch([dict(r, want_pcm=1) for r in reqs])
        for o, w, nat in zip(outs, want, native_out):
            assert o.status == 0 and np.array_equal(o.codes, nat.codes) and o.hit_eos == nat.hit_eos
            assert o.sample_rate == 24000 and o.n_samples == R.N_t(nat.pcm.size, s) == w.size
            assert np.array_equal(_bits(o.pcm), _bits(w))
        for fmt in (_abi.PCM_F32, _abi.PCM_I16):
            for g, w, b, nat in zip(_session(eng_s, reqs, fmt), want, bounds, native_out):
                chunks = g["chunks"]
                assert len(chunks) >= 3 and chunks[-1][1] and not any(f for _, f in chunks[:-1])
                pcm = np.concatenate([c for c, _ in chunks])
                if fmt == _abi.PCM_F32:
                    assert pcm.dtype == np.float32 and np.array_equal(_bits(pcm), _bits(w))
                else:
                    assert pcm.dtype == np.int16 and np.array_equal(pcm, _i16(w))
                edges = [0] + [R.D_t(ns, s) for ns in b[:-1]] + [R.N_t(b[-1], s)]
                assert [c.size for c, _ in chunks] == [q - p for p, q in zip(edges, edges[1:])]
                assert g["res"].sample_rate == 24000 and g["res"].n_samples == w.size and np.array_equal(g["res"].codes, nat.codes)
        for r, w in zip(reqs, want):
            chunks = list(native.stream_chunks(eng_s, **dict(r, want_pcm=1)))
            assert len(chunks) >= 3 and chunks[-1][1] and not any(f for _, f in chunks[:-1])
            assert np.array_equal(_bits(np.concatenate([c for c, _ in chunks])), _bits(w))
            assert np.array_equal(_bits(eng_s.last_stream_result.pcm), _bits(w))
    finally:
        eng_s.set_speed(0)


def test_speed_and_output_rate_together(engines):
    from q3tts import _abi
    cfg, eng_s, eng_n, reqs, native_out, bounds = engines
    want = [eng_n.resample(eng_n.time_stretch(o.pcm, 1250), 24000, 8000) for o in native_out]
    for order in (0, 1):  # whichever setter comes first sizes the staging rows for both
        (eng_s.set_speed(1250), eng_s.set_output_rate(8000)) if order == 0 else (eng_s.set_output_rate(8000), eng_s.set_speed(1250))
        try:
            outs = eng_s.generate_batch([dict(r, want_pcm=1) for r in reqs])
            for o, w, nat in zip(outs, want, native_out):
                assert o.sample_rate == 8000 and o.n_samples == w.size and np.array_equal(o.codes, nat.codes)
                assert np.array_equal(_bits(o.pcm), _bits(w))
            if order == 0:
                for g, w in zip(_session(eng_s, reqs, _abi.PCM_F32), want):
                    assert len(g["chunks"]) >= 3 and np.array_equal(_bits(np.concatenate([c for c, _ in g["chunks"]])), _bits(w))
                from q3tts import native
                chunks = list(native.stream_chunks(eng_s, **dict(reqs[3], want_pcm=1)))
                assert np.array_equal(_bits(np.concatenate([c for c, _ in chunks])), _bits(want[3]))
        finally:
            eng_s.set_speed(0)
            eng_s.set_output_rate(0)


def test_paced_session_with_swapping(engines):
    """Six paced requests (credit 4 frames) on four slots with a swap arena: requests leave their slots between chunks and come back, into
    whichever slot is free. Every request's chunks are those of the unpaced run, and joined the one-shot stretch of the unstretched PCM."""
    from q3tts import _abi, native
    cfg, eng_s, eng_n, reqs, native_out, bounds = engines
    want = [eng_n.time_stretch(o.pcm, 800) for o in native_out]
    eng_s.set_speed(800)
    try:
        plain = _session(eng_s, reqs, _abi.PCM_F32)
        chunks, fin = defaultdict(list), {}
        with native.NativeSession(eng_s, _abi.PCM_F32, swap_mb=32) as sess:
            def until(done):
                while not done():
                    ev = sess.next(60000)
                    assert ev is not None, "no event"
                    rid, kind, pcm, is_fin, res = ev
                    if kind == _abi.EV_CHUNK:
                        chunks[rid].append(pcm)
                    else:
                        assert kind == _abi.EV_DONE and res.status == 0
                        fin[rid] = res
            ids = [sess.submit(credit_frames=4, **r) for r in reqs]
            until(lambda: all(len(chunks[r]) == 1 for r in ids))   # all six on four slots before any grant
            assert sess.swap_stats()["swap_outs"] >= 2
            for r in reversed(ids):
                sess.grant(r, 4)
            until(lambda: all(len(chunks[r]) == 2 for r in ids))
            assert not fin
            for r in ids[1::2] + ids[0::2]:
                sess.grant(r, -1)
            until(lambda: len(fin) == len(ids))
            st = sess.swap_stats()
            assert st["swap_ins"] == st["swap_outs"] >= 3 and st["arena_used"] == 0
        for r, g, w, nat in zip(ids, plain, want, native_out):
            assert [c.size for c in chunks[r]] == [c.size for c, _ in g["chunks"]]
            assert np.array_equal(_bits(np.concatenate(chunks[r])), _bits(w))
            assert np.array_equal(fin[r].codes, nat.codes) and fin[r].n_samples == w.size
    finally:
        eng_s.set_speed(0)


def test_off_after_on(engines):
    from q3tts import _abi
    cfg, eng_s, eng_n, reqs, native_out, bounds = engines
    eng_s.set_speed(1250)
    eng_s.set_speed(1000)
    assert eng_s.get_speed() == 0
    outs = eng_s.generate_batch([dict(r, want_pcm=1) for r in reqs])
    for o, nat in zip(outs, native_out):
        assert o.n_samples == nat.pcm.size and np.array_equal(o.codes, nat.codes) and np.array_equal(_bits(o.pcm), _bits(nat.pcm))
    for g, nat, b in zip(_session(eng_s, reqs, _abi.PCM_F32), native_out, bounds):
        assert np.cumsum([c.size for c, _ in g["chunks"]]).tolist() == b
        assert np.array_equal(_bits(np.concatenate([c for c, _ in g["chunks"]])), _bits(nat.pcm))


def test_refusals_leave_the_state_unchanged(engines):
    from q3tts import _abi, api, native
    cfg, eng_s, eng_n, reqs, native_out, bounds = engines
    lib = eng_s.lib
    for bad in (499, 2001, -5, 1):
        assert lib.q3tts_set_speed(eng_s.h, bad) == INVALID and eng_s.get_speed() == 0
    eng_s.set_speed(1250)
    try:
        for bad in (499, 2001):
            assert lib.q3tts_set_speed(eng_s.h, bad) == INVALID and eng_s.get_speed() == 1250
        with native.NativeSession(eng_s) as sess:
            assert lib.q3tts_set_speed(eng_s.h, 800) == STATE and lib.q3tts_set_speed(eng_s.h, 0) == STATE
            assert sess is not None
        assert eng_s.get_speed() == 1250
        assert lib.q3tts_set_device_pcm(eng_s.h, 1) == STATE  # device-resident PCM stays unstretched
        it = native.stream_chunks(eng_s, **dict(reqs[0], want_pcm=1))
        next(it)
        assert lib.q3tts_set_speed(eng_s.h, 800) == STATE  # a stream is open
        it.close()
        assert eng_s.get_speed() == 1250
    finally:
        eng_s.set_speed(0)
    eng_s.set_device_pcm(True)
    try:
        assert lib.q3tts_set_speed(eng_s.h, 800) == STATE and eng_s.get_speed() == 0
        assert lib.q3tts_set_speed(eng_s.h, 1000) == 0  # off stays allowed
    finally:
        eng_s.set_device_pcm(False)
    # the Python surface: a float in, per mille inside
    te = api.TtsEngine.__new__(api.TtsEngine)
    te._native, te.cfg = eng_s, cfg
    te.set_speed(1.25)
    assert eng_s.get_speed() == 1250 and te.get_speed() == 1.25
    te.set_speed(1.0)
    assert eng_s.get_speed() == 0 and te.get_speed() == 1.0
    bare = native.NativeEngine(_abi.tiny_config(max_batch=2, n_ctx=256, with_vocoder=0))
    try:
        assert lib.q3tts_set_speed(bare.h, 1250) == INVALID and bare.get_speed() == 0
        assert lib.q3tts_set_speed(bare.h, 0) == 0
    finally:
        bare.close()

"""The device resampler on the GPU: k_pcm_resample against the numpy restatement bit for bit (tests/_resample_ref.py, fed
the library's own table), q3tts_resample, the engine's output rate through generate_batch, sessions (f32 and i16) and streams, the
setter's refusals, and the clone path's resample keyword."""
import os
import struct
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _resample_ref as RR  # noqa: E402

pytestmark = pytest.mark.gpu

KERNEL_PAIRS = [(24000, 8000), (24000, 16000), (24000, 48000), (24000, 44100), (16000, 24000), (44100, 24000)]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _expect(src, row_len, tab, L, M, H, entries, out_n):
    out = np.zeros(out_n, dtype=np.float32)
    for r, first, count, dst in entries:
        out[dst:dst + count] = RR.resample32(src[r], int(row_len[r]), tab, L, M, H, first, count)
    return out


def _run_both(src, row_len, row_final, entries, out_n, rate_in, rate_out, tab, L, M, H):
    from q3tts import native
    want = _expect(src, row_len, tab, L, M, H, entries, out_n)
    assert np.isfinite(want).all()
    got = native.k_pcm_resample(src, row_len, row_final, entries, out_n, rate_in, rate_out, 0)
    assert np.isfinite(got).all()
    assert np.array_equal(_bits(got), _bits(want)), np.flatnonzero(_bits(got) != _bits(want))[:8]
    got16 = native.k_pcm_resample(src, row_len, row_final, entries, out_n, rate_in, rate_out, 1)
    assert got16.dtype == np.int16 and np.array_equal(got16, RR.to_i16(want))


@pytest.mark.parametrize("rate_in,rate_out", KERNEL_PAIRS)
def test_kernel_equals_restatement(rate_in, rate_out):
    """Rows of 1, H, H + 1, H + 2, 7680 and 7681 valid samples, final and not, NaN beyond them, in a buffer whose odd stride gives every row
    another 16-byte alignment; windows at output 0, in the middle and at the last output, counts 1 / 255 / 256 / 257 and whole rows (several
    workgroups, several tiles each), an empty entry; 64 entries in one launch, the destinations one sample apart so that every gap must
    stay untouched. f32 bit for bit, i16 equal."""
    from q3tts import native
    L, M, H, tab = native.k_resample_table(rate_in, rate_out)
    rng = np.random.default_rng(rate_in * 7 + rate_out)
    lens = [1, H, H + 1, H + 2, 7680, 7681]
    row_len = np.array(lens + lens, dtype=np.int32)
    row_final = np.array([1] * 6 + [0] * 6, dtype=np.int32)
    stride = 7683
    src = np.full((12, stride), np.nan, dtype=np.float32)
    for r in range(12):
        src[r, :row_len[r]] = rng.uniform(-1.0, 1.0, row_len[r]).astype(np.float32)
    lim = [RR.N(int(n), L, M) if f else RR.D(int(n), L, M, H) for n, f in zip(row_len, row_final)]
    assert lim[6] == 0 and lim[7] == 0 and lim[8] > 0  # an unfinished row of <= H samples delivers nothing, one of H + 1 does
    entries, dst = [], 3
    def add(r, first, count):
        nonlocal dst
        count = max(0, min(count, lim[r] - first))
        entries.append((r, first, count, dst))
        dst += count + 1
    for r in range(12):  # every row whole (the long ones: several workgroups and several tiles per workgroup)
        add(r, 0, lim[r])
    for r in (4, 5, 10, 11):
        for count in (1, 255, 256, 257):
            add(r, (0, lim[r] // 2 + 1, lim[r] - count)[len(entries) % 3], count)
        add(r, lim[r] - 1, 1)      # the last output
        add(r, lim[r] // 3, 1500)  # from the middle, several tiles
    for r in (0, 1, 2, 3, 8, 9):
        add(r, lim[r] - 1, 1)
        add(r, 0, 1)
    add(4, 17, 0)                  # an empty entry writes nothing
    while len(entries) < 64:
        r = (4, 5, 10, 11)[len(entries) % 4]
        add(r, int(rng.integers(0, lim[r] - 300)), int(rng.integers(1, 300)))
    assert len(entries) == 64 and sum(1 for e in entries if e[2] == 0) >= 3
    _run_both(src, row_len, row_final, entries, dst + 5, rate_in, rate_out, tab, L, M, H)
    # one entry alone: the launch is as wide as the entry has tiles
    _run_both(src, row_len, row_final, [(5, 0, lim[5], 1)], lim[5] + 2, rate_in, rate_out, tab, L, M, H)
    # a window the row cannot deliver yet is refused
    from q3tts import _abi
    with pytest.raises(_abi.Q3Error):
        native.k_pcm_resample(src, row_len, row_final, [(10, 0, lim[10] + 1, 0)], lim[10] + 1, rate_in, rate_out, 0)


@pytest.fixture(scope="module")
def engines():
    from q3tts import _abi, native
    cfg = _abi.tiny_config(max_batch=4, n_ctx=256, with_vocoder=1)
    eng_r, eng_n = native.NativeEngine(cfg), native.NativeEngine(cfg)
    d = cfg.model.d_embed
    desc, keep = native.make_prompt_desc(np.arange(100, 112), spk_emb=((np.arange(d) % 13 - 6) * 0.03125).astype(np.float32))
    pe = eng_n.build_prompt(desc)
    frames = [1, 4, 5, 9, 9, 5, 4, 1, 5]  # single chunk, exact multiple, tail; nine requests over four slots: refilled slots
    reqs = [dict(embd=pe, temperature=0.7, top_k=40, top_p=0.9, seed=300 + i, max_steps=20, min_frames=f, force_eos_at=f)
            for i, f in enumerate(frames)]
    native_out = eng_n.generate_batch([dict(r, want_pcm=1) for r in reqs])
    assert [o.codes.shape[0] for o in native_out] == frames
    # the native-rate sample counts after every chunk event of a session (an empty final one included): the boundaries at which a
    # session hands samples out, whatever the rate
    bounds = [np.cumsum([c.size for c, _ in g["chunks"]]).tolist() for g in _session(eng_n, reqs, _abi.PCM_F32)]
    yield cfg, eng_r, eng_n, reqs, native_out, bounds
    eng_r.close()
    eng_n.close()


@pytest.mark.parametrize("rate_in,rate_out", [(16000, 24000), (44100, 24000)])
def test_one_shot_resample_equals_restatement(engines, rate_in, rate_out):
    from q3tts import native
    cfg, eng_r, eng_n, reqs, native_out, bounds = engines
    L, M, H, tab = native.k_resample_table(rate_in, rate_out)
    n = 3 * rate_in
    t = np.arange(n) / rate_in
    x = (0.6 * np.sin(2 * np.pi * 220.0 * t) + 0.05 * np.random.default_rng(5).standard_normal(n)).astype(np.float32)
    y = eng_n.resample(x, rate_in, rate_out)
    assert y.size == RR.N(n, L, M) == 72000
    assert np.array_equal(_bits(y), _bits(RR.resample32(x, n, tab, L, M, H, 0, y.size)))
    assert eng_n.resample(np.zeros(0, np.float32), rate_in, rate_out).size == 0


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


@pytest.mark.parametrize("rate", [8000, 44100])
def test_engine_output_rate(engines, rate):
    """generate_batch at an output rate == q3tts_resample of the native-rate PCM of an engine without one (codes equal); session chunks
    (f32 and i16) and stream chunks, joined, equal that PCM bit for bit, a chunk that is not the last carrying D(ns) - delivered samples;
    the rate turned off again restores the native PCM bit for bit."""
    from q3tts import _abi, native
    cfg, eng_r, eng_n, reqs, native_out, bounds = engines
    L, M, H, tab = native.k_resample_table(24000, rate)
    want = [eng_n.resample(o.pcm, 24000, rate) for o in native_out]
    assert eng_r.get_output_rate() == 0
    eng_r.set_output_rate(rate)
    try:
        assert eng_r.get_output_rate() == rate
        outs = eng_r.generate_batch([dict(r, want_pcm=1) for r in reqs])
        for o, w, nat in zip(outs, want, native_out):
            assert o.status == 0 and np.array_equal(o.codes, nat.codes)
            assert o.sample_rate == rate and o.n_samples == RR.N(nat.pcm.size, L, M) == w.size
            assert np.array_equal(_bits(o.pcm), _bits(w))
        # the restatement on the engine's native PCM, for the longest utterance: the engine path reads the slot's row as the hook reads its rows
        assert np.array_equal(_bits(want[3]), _bits(RR.resample32(native_out[3].pcm, native_out[3].pcm.size, tab, L, M, H, 0, want[3].size)))
        for fmt in (_abi.PCM_F32, _abi.PCM_I16):
            for g, w, b in zip(_session(eng_r, reqs, fmt), want, bounds):
                chunks = g["chunks"]
                assert chunks and chunks[-1][1] and not any(f for _, f in chunks[:-1])
                pcm = np.concatenate([c for c, _ in chunks])
                if fmt == _abi.PCM_F32:
                    assert pcm.dtype == np.float32 and np.array_equal(_bits(pcm), _bits(w))
                else:
                    assert pcm.dtype == np.int16 and np.array_equal(pcm, RR.to_i16(w))
                edges = [0] + [RR.D(ns, L, M, H) for ns in b[:-1]] + [RR.N(b[-1], L, M)]
                assert [c.size for c, _ in chunks] == [q - p for p, q in zip(edges, edges[1:])]
                assert g["res"].sample_rate == rate and g["res"].n_samples == w.size
        for r, w in zip(reqs, want):
            chunks = list(native.stream_chunks(eng_r, **dict(r, want_pcm=1)))
            assert chunks[-1][1] and not any(f for _, f in chunks[:-1])
            assert np.array_equal(_bits(np.concatenate([c for c, _ in chunks])), _bits(w))
            res = eng_r.last_stream_result
            assert res.sample_rate == rate and np.array_equal(_bits(res.pcm), _bits(w))
    finally:
        eng_r.set_output_rate(0)
    assert eng_r.get_output_rate() == 0
    outs = eng_r.generate_batch([dict(r, want_pcm=1) for r in reqs])
    for o, nat in zip(outs, native_out):
        assert o.sample_rate == 24000 and np.array_equal(o.codes, nat.codes) and np.array_equal(_bits(o.pcm), _bits(nat.pcm))
    for g, nat in zip(_session(eng_r, reqs, _abi.PCM_F32), native_out):
        assert np.array_equal(_bits(np.concatenate([c for c, _ in g["chunks"]])), _bits(nat.pcm))


def test_setter_refusals_leave_the_state_unchanged(engines):
    from q3tts import _abi, native
    cfg, eng_r, eng_n, reqs, native_out, bounds = engines
    lib = eng_r.lib
    assert lib.q3tts_set_output_rate(eng_r.h, 3999) == -1 and lib.q3tts_set_output_rate(eng_r.h, 96001) == -1
    assert lib.q3tts_set_output_rate(eng_r.h, 44101) == -6 and eng_r.get_output_rate() == 0
    assert lib.q3tts_set_output_rate(eng_r.h, 24000) == 0 and eng_r.get_output_rate() == 0  # the vocoder's own rate = off
    eng_r.set_output_rate(16000)
    try:
        with native.NativeSession(eng_r) as sess:
            assert lib.q3tts_set_output_rate(eng_r.h, 8000) == -5 and lib.q3tts_set_output_rate(eng_r.h, 0) == -5
            assert sess is not None
        assert eng_r.get_output_rate() == 16000
        assert lib.q3tts_set_device_pcm(eng_r.h, 1) == -5  # device-resident PCM is native-rate only
        it = native.stream_chunks(eng_r, **dict(reqs[2], want_pcm=1))
        next(it)
        assert lib.q3tts_set_output_rate(eng_r.h, 8000) == -5  # a stream is open
        it.close()
        assert eng_r.get_output_rate() == 16000
    finally:
        eng_r.set_output_rate(0)
    eng_r.set_device_pcm(True)
    try:
        assert lib.q3tts_set_output_rate(eng_r.h, 8000) == -5 and eng_r.get_output_rate() == 0
    finally:
        eng_r.set_device_pcm(False)
    eng_r.set_output_rate(8000)
    assert eng_r.get_output_rate() == 8000
    eng_r.set_output_rate(0)


def _write_f32_wav(path, samples, rate):
    body = np.asarray(samples, dtype="<f4").tobytes()
    hdr = b"RIFF" + struct.pack("<I", 36 + len(body)) + b"WAVE" + b"fmt " + struct.pack("<IHHIIHH", 16, 3, 1, rate, rate * 4, 4, 32)
    with open(path, "wb") as f:
        f.write(hdr + b"data" + struct.pack("<I", len(body)) + body)


def test_create_voice_file_resample_keyword(tmp_path):
    """A 16 kHz clip with resample = True gives the codes and the embedding of the same clip resampled by q3tts_resample and stored as a
    24 kHz WAV; without the keyword the reference's error stays."""
    from q3tts import _abi, api, native
    cfg = _abi.tiny_config(max_batch=2, n_ctx=256, with_vocoder=1)
    eng = native.NativeEngine(cfg)
    try:
        eng.clone_init(_abi.tiny_clone_config(cfg.model.d_embed))
        te = api.TtsEngine.__new__(api.TtsEngine)
        te._native, te.cfg, te.tokenizer, te.speakers, te.max_steps, te.sampler_config = eng, cfg, None, {}, 6, api.SamplerConfig(0.0, 40, 0.9, 7)
        n = 6000
        t = np.arange(n) / 16000.0
        a16 = (0.3 * np.sin(2 * np.pi * 150.0 * t) + 0.1 * np.sin(2 * np.pi * 1900.0 * t) + 0.02 * np.random.default_rng(2).standard_normal(n)).astype(np.float32)
        _write_f32_wav(tmp_path / "ref16.wav", a16, 16000)
        a24 = eng.resample(a16, 16000, 24000)
        assert a24.size == 9000
        _write_f32_wav(tmp_path / "ref24.wav", a24, 24000)
        v16 = te.create_voice_file(tmp_path / "ref16.wav", [9, 8, 7], resample=True)
        v24 = te.create_voice_file(tmp_path / "ref24.wav", [9, 8, 7])
        assert len(v24.audio_codes) == 5 * 16 and v16.audio_codes == v24.audio_codes
        assert np.array_equal(_bits(np.asarray(v16.speaker_embedding)), _bits(np.asarray(v24.speaker_embedding)))
        with pytest.raises(_abi.Q3Error, match="Expected 24000Hz audio, found 16000Hz"):
            te.create_voice_file(tmp_path / "ref16.wav", [9, 8, 7])
    finally:
        eng.close()

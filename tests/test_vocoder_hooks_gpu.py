"""The three vocoder hooks (q3tts_k_vocoder, _latent, _taps) are one drive of slot 0: the same reset, the same split into chunks and into calls
of at most 4 frames, the same launches. Pinned here on the tiny vocoder: the "pcm" taps of a drive's calls, concatenated, are the PCM of
q3tts_k_vocoder bit for bit; a tap_call past the last call is refused on the host and leaves the engine usable; and the vocoder call's graph
cache, keyed by (slots, frames, launch switches), gives the same bits eagerly, at capture and at replay in both launch modes. No tolerance is
involved: every comparison is between two paths of the same code that the design declares identical."""
import contextlib
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

# (n_frames, chunk_frames, frames of each call): chunks of 3 + 3 + 3 + 1, and one shot split 4 + 4 + 1
DRIVES = [(10, 3, (3, 3, 3, 1)), (9, 0, (4, 4, 1))]


@contextlib.contextmanager
def _env(name, value):
    old = os.environ.pop(name, None)
    if value is not None:
        os.environ[name] = value
    try:
        yield
    finally:
        os.environ.pop(name, None)
        if old is not None:
            os.environ[name] = old


def _engine():
    from q3tts import _abi, native
    return native.NativeEngine(_abi.tiny_config(max_batch=2, n_ctx=128, with_vocoder=1))


@pytest.fixture(scope="module")
def eng():
    e = _engine()
    yield e
    e.close()


def _codes(eng, n):
    return np.random.default_rng(5).integers(0, eng.cfg.vocoder.codebook_size, size=(n, 16)).astype(np.int32)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.mark.parametrize("n,chunk,calls", DRIVES)
def test_pcm_taps_of_every_call_are_the_vocoder_pcm(eng, n, chunk, calls):
    codes = _codes(eng, n)
    pcm = eng.vocoder(codes, chunk)
    spf = pcm.size // n
    assert pcm.size == n * spf
    parts = []
    for i, frames in enumerate(calls):
        tap, hist_rows = eng.vocoder_taps(codes, chunk_frames=chunk, tap_call=i)["pcm"]
        assert hist_rows == 0 and tap.shape == (frames * spf, 1), (i, hist_rows, tap.shape)
        parts.append(tap[:, 0])
    got = np.concatenate(parts)
    assert got.size == pcm.size
    assert np.array_equal(_bits(got), _bits(pcm))


@pytest.mark.parametrize("n,chunk,calls", DRIVES)
def test_tap_call_past_the_last_call_is_refused(eng, n, chunk, calls):
    from q3tts import _abi
    codes = _codes(eng, n)
    pcm = eng.vocoder(codes, chunk)
    with pytest.raises(_abi.Q3Error, match=r"\(-1\).*tap_call is past the last call of this drive"):   # Q3TTS_ERR_INVALID
        eng.vocoder_taps(codes, chunk_frames=chunk, tap_call=len(calls))
    assert np.array_equal(_bits(eng.vocoder(codes, chunk)), _bits(pcm))


def test_graph_cache_is_keyed_by_the_launch_switches():
    eng = _engine()   # a fresh engine: no call shape has been seen yet
    try:
        codes = _codes(eng, 10)
        pcms = []
        for polite in (None, "1"):
            with _env("Q3TTS_VOC_POLITE", polite):
                pcms += [eng.vocoder(codes, 3) for _ in range(3)]   # per mode: every call shape eager, then captured, then replayed
    finally:
        eng.close()
    assert all(p.size == pcms[0].size and np.array_equal(_bits(p), _bits(pcms[0])) for p in pcms[1:])

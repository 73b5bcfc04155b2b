"""Shapes of the voice-clone encoders beyond the tiny and the full config (tests/test_clone_shapes_{cpu,gpu}.py; tests/_rvq_ref.py takes the
quantiser alone through the same codebook sizes).

Every shape is _abi.tiny_clone_config() with a few fields changed and short clips; all of them pass q3_clone.hip's validate(). What each group is
for (the paths of q3_clone.hip that the tiny and the full config never reach):
  win        150 transformer rows and a window of 1 .. 200: k_enc_attn with a window that slides past 64 keys (more than one lane trip of the
             score loop while j0 > 0), exactly at 63 / 64 / 65 and 128 / 129 keys, a window equal to and wider than the clip, and ae_window == 1
  heads      head_dim 4 .. 256 (lanes idle below 64, two to four trips of the q staging and PV loops above), n_head * head_dim != ae_hidden
  ln         k_layernorm with d < 64 and with d = 528, no multiple of 64
  l0 / r1    no transformer layer; one SEANet stage
  down3      the frame-rate convolution with stride 3 (kernel 6, replicate padding) at row counts 0, 1, 2 mod 3
  vq         codebook sizes around RVQ_T = 1024 and RVQ_T * RVQ_CW = 2048 (the clamp, the second trip of the j0 loop), one codeword, one codebook
             (pa never read), 64 codebooks, vq_dim != 16 k
  rope_edge  the last row of the RoPE table (16 384 rows); one more sample is refused
  speaker    se_res2net_scale 2 (src2 never set) and 8, a Res2Net convolution with k == 1, an aggregation convolution with k == 3, and T around
             the multiples of CS_B = 16 of k_colstats / k_softmax_time
Clips of a shape are listed in running order: a short one, a longer one, the short one again, so the arena grows and is then reused larger than
the call needs.
"""
import functools

import numpy as np

from q3tts import _abi

_ARRAYS = {"se_channels": 5, "se_kernels": 5, "se_dilations": 5, "ae_ratios": 4}


def make(**kw):
    c = _abi.tiny_clone_config()
    for k, v in kw.items():
        if k in _ARRAYS:
            v = list(v) + [0] * (_ARRAYS[k] - len(v))
            getattr(c, k)[:] = v
        else:
            assert hasattr(c, k), k
            setattr(c, k, v)
    return c


WINDOWS = (1, 63, 64, 65, 80, 128, 129, 150, 200)
HEADS = ((4, 4), (1, 16), (1, 96), (2, 128), (1, 256), (8, 32))
VQ = ((1, 16, 1), (63, 16, 2), (1000, 48, 3), (1025, 16, 64), (2049, 32, 3), (3000, 48, 3), (5000, 272, 2), (4096, 16, 2))
_LN16 = dict(ae_hidden=16, ae_d_ffn=16, ae_n_head=1, ae_head_dim=16)

# name -> (config fields, clip lengths in running order)
AUDIO = {}
for _w in WINDOWS:
    AUDIO["win%d" % _w] = (dict(ae_n_ratios=2, ae_ratios=[4, 5], ae_window=_w), (400, 3000, 400))
for _nh, _hd in HEADS:
    AUDIO["heads%dx%d" % (_nh, _hd)] = (dict(ae_hidden=128, ae_n_head=_nh, ae_head_dim=_hd), (1921, 24000, 1921))
AUDIO["ln16"] = (dict(_LN16), (1921, 24000, 1921))
AUDIO["ln528"] = (dict(ae_hidden=528), (1921, 24000, 1921))
AUDIO["l0"] = (dict(ae_n_layer=0), (1921, 24000, 1921))
AUDIO["r1"] = (dict(ae_n_ratios=1, ae_ratios=[8]), (100, 1600, 100))
AUDIO["down3"] = (dict(ae_down_stride=3), (960 * 6, 960 * 7 + 1, 960 * 6, 960 * 7))  # 6, 8, 6, 7 rows
for _cs, _d, _ncb in VQ:
    AUDIO["vq%dx%dx%d" % (_cs, _d, _ncb)] = (dict(ae_codebook_size=_cs, ae_vq_dim=_d, ae_n_codebooks=_ncb), (1921, 9000, 1921))
ROPE_EDGE = dict(ae_n_ratios=1, ae_ratios=[1], ae_window=4, ae_n_layer=1, **_LN16)
ROPE_MAX_T = 16384
AUDIO["rope_edge"] = (ROPE_EDGE, (ROPE_MAX_T,))

SPEAKER_T = (16, 65, 16, 1, 2, 3, 15, 17, 31, 32, 33, 64)   # {1, 2, 3, 15, 16, 17, 31, 32, 33, 64, 65}: short, the longest, short again, the rest
SPEAKER = {
    "tiny": dict(),
    "s2": dict(se_res2net_scale=2, se_kernels=[7, 5, 3, 1, 3], se_dilations=[2, 1, 5, 1, 2], se_attn_channels=16, se_se_channels=16, se_dim=16),
    "s8": dict(se_channels=[128, 128, 128, 128, 384], se_res2net_scale=8),
}


def audio_cases():
    """[(shape, clip index, n)] in running order"""
    return [(name, i, n) for name, (_, clips) in AUDIO.items() for i, n in enumerate(clips)]


def speaker_cases():
    return [(name, i, T) for name in SPEAKER for i, T in enumerate(SPEAKER_T)]


def audio_config(name):
    return make(**AUDIO[name][0])


def speaker_config(name):
    return make(**SPEAKER[name])


def rows(c, n):
    """transformer rows of an n-sample clip"""
    for i in range(c.ae_n_ratios):
        n = -(-n // c.ae_ratios[i])
    return n


def clip(n, seed=0):
    """speech-shaped synthetic clip: a few drifting harmonics plus noise, in [-1, 1]"""
    rng = np.random.default_rng(seed)
    t = np.arange(n, dtype=np.float64) / 24000.0
    f0 = 120.0 + 30.0 * np.sin(2 * np.pi * 1.3 * t)
    ph = 2 * np.pi * np.cumsum(f0) / 24000.0
    x = sum(np.sin(k * ph) / k for k in range(1, 6)) * 0.2 + rng.standard_normal(n) * 0.02
    return np.clip(x, -1, 1).astype(np.float32)


def mel(T, seed=None):
    """log-mel-like rows [T][128]"""
    rng = np.random.default_rng(T if seed is None else seed)
    return (rng.standard_normal((T, 128)) * 2.0 - 4.0).astype(np.float32)


@functools.lru_cache(maxsize=None)
def audio_ref(name, n):
    """the oracle's (codes, pre-quantiser rows) of clip(n, n) at a shape; computed once, shared, never written to"""
    import _oracle as O
    codes, lat = O.audio_encode(audio_config(name), 0, clip(n, n))
    codes.setflags(write=False); lat.setflags(write=False)
    return codes, lat


@functools.lru_cache(maxsize=None)
def speaker_ref(name, T):
    import _oracle as O
    out = O.speaker_encode(speaker_config(name), 0, mel(T))
    out.setflags(write=False)
    return out

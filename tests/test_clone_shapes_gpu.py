"""The voice-clone encoders at the shapes of tests/_clone_shapes.py: HIP path through the C ABI against the CPU oracle, bit for bit.

The same assertions as tests/test_clone_gpu.py (latent rows and speaker embedding equal on raw bits, codec ids equal, frame counts equal), at
shapes that reach the paths of q3_clone.hip which the tiny and the full config leave out (listed in _clone_shapes.py). One engine for the
module; q3tts_clone_init runs once per shape, and the clips of a shape run short, long, short again on it, so the arena grows and is then
reused larger than a call needs. tests/test_clone_shapes_cpu.py holds the oracle itself against the model family's modules at these shapes.
"""
import numpy as np
import pytest

import _clone_shapes as S

pytestmark = pytest.mark.gpu


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


class _Shapes:
    """the module's engine and the shape its encoders were last built for"""
    def __init__(self, eng):
        self.eng, self.current = eng, None

    def use(self, kind, name):
        if self.current != (kind, name):
            self.current = None
            self.eng.clone_init(S.audio_config(name) if kind == "audio" else S.speaker_config(name))
            self.current = (kind, name)
        return self.eng


@pytest.fixture(scope="module")
def shapes(oracle):
    from q3tts import _abi, native
    eng = native.NativeEngine(_abi.tiny_config(max_batch=1, n_ctx=128, with_vocoder=0))
    yield _Shapes(eng)
    eng.close()


@pytest.mark.parametrize("name,i,n", S.audio_cases(), ids=["%s-%d-n%d" % c for c in S.audio_cases()])
def test_audio_encoder_shapes_bits(shapes, name, i, n):
    eng = shapes.use("audio", name)
    c = S.audio_config(name)
    codes_ref, lat_ref = S.audio_ref(name, n)
    a = S.clip(n, n)
    assert eng.clone_audio_frames(n) == codes_ref.shape[0] == -(-S.rows(c, n) // c.ae_down_stride)
    lat = eng.audio_latent(a)
    assert lat.shape == lat_ref.shape and np.isfinite(lat).all()
    assert np.array_equal(_bits(lat), _bits(lat_ref)), "pre-quantiser rows differ in %d of %d frames" % (
        int((_bits(lat) != _bits(lat_ref)).any(axis=1).sum()), lat.shape[0])
    codes = eng.audio_encode(a)
    assert codes.dtype == np.int64 and codes.shape == codes_ref.shape
    assert np.array_equal(codes, codes_ref.astype(np.int64))
    assert codes.min() >= 0 and codes.max() < c.ae_codebook_size


def test_rope_table_one_row_past_the_end_is_refused(shapes):
    """16 384 rows use the last row of the position table (the rope_edge case above); one more sample is one more row, refused on the host
    before anything is copied or launched — the encoders still answer afterwards."""
    from q3tts import _abi
    eng = shapes.use("audio", "rope_edge")
    assert S.rows(S.audio_config("rope_edge"), S.ROPE_MAX_T + 1) == S.ROPE_MAX_T + 1
    with pytest.raises(_abi.Q3Error, match="position table"):
        eng.audio_encode(np.zeros(S.ROPE_MAX_T + 1, dtype=np.float32))
    with pytest.raises(_abi.Q3Error, match="position table"):
        eng.audio_latent(np.zeros(S.ROPE_MAX_T + 1, dtype=np.float32))
    a = S.clip(64, 64)
    import _oracle as O
    codes_ref, lat_ref = O.audio_encode(S.audio_config("rope_edge"), 0, a)
    assert np.array_equal(_bits(eng.audio_latent(a)), _bits(lat_ref)) and np.array_equal(eng.audio_encode(a), codes_ref.astype(np.int64))


@pytest.mark.parametrize("name,i,T", S.speaker_cases(), ids=["%s-%d-T%d" % c for c in S.speaker_cases()])
def test_speaker_encoder_shapes_bits(shapes, name, i, T):
    eng = shapes.use("speaker", name)
    ref = S.speaker_ref(name, T)
    out = eng.speaker_from_mel(S.mel(T))
    assert out.shape == ref.shape and np.isfinite(out).all() and np.abs(out).max() > 1e-3
    assert np.array_equal(_bits(out), _bits(ref))


# One offending config per rule of validate() (q3_clone.hip): (fields of the tiny config to change, what the refusal says). The depth rule
# — kernel x input channels <= 8192 for EVERY convolution q3tts_clone_init builds — names the convolution; MFA, Res2Net, the first audio
# conv, the residual conv and the O projection were unbounded before it became one rule.
_DEEP = ".*: GEMM depth .* exceeds 8192"
REFUSALS = [
    (dict(mel_dim=80), "mel_dim must be 128"),
    (dict(se_channels=[64, 64, 24, 64, 192]), "se_channels must be positive multiples of 16"),
    (dict(se_channels=[64, 64, 64, 64, 0]), "se_channels must be positive multiples of 16"),
    (dict(se_kernels=[5, 4, 3, 3, 1]), "se_kernels must be odd"),
    (dict(se_dilations=[1, 2, 0, 4, 1]), "se_dilations >= 1"),
    (dict(se_channels=[64, 64, 128, 64, 192]), "share one width"),
    (dict(se_channels=[64, 64, 64, 64, 128]), "3 x the block width"),
    (dict(se_res2net_scale=1), "block width / se_res2net_scale"),
    (dict(se_res2net_scale=3), "block width / se_res2net_scale"),
    (dict(se_res2net_scale=8), "block width / se_res2net_scale"),
    (dict(se_attn_channels=24), "se_attn_channels, se_se_channels, se_dim"),
    (dict(se_se_channels=0), "se_attn_channels, se_se_channels, se_dim"),
    (dict(se_dim=40), "se_attn_channels, se_se_channels, se_dim"),
    (dict(se_kernels=[65, 3, 3, 3, 1]), "speaker TDNN" + _DEEP),                                    # 65 x 128
    (dict(se_kernels=[5, 513, 3, 3, 1]), "Res2Net conv" + _DEEP),                                   # 513 x 16
    (dict(se_kernels=[5, 3, 3, 3, 43]), r"aggregation \(MFA\) conv" + _DEEP),                       # 43 x 192
    (dict(se_se_channels=8208), "squeeze-excitation conv" + _DEEP),
    (dict(se_attn_channels=8208), "attentive pooling conv" + _DEEP),
    (dict(se_channels=[912, 912, 912, 912, 2736], se_res2net_scale=3), "attentive pooling TDNN" + _DEEP),   # 3 x 2736
    (dict(se_channels=[8208, 8208, 8208, 8208, 24624], se_res2net_scale=3), "SE-Res2Net 1x1 conv" + _DEEP),
    (dict(ae_filters=48), "ae_filters must be a positive multiple of 32"),
    (dict(ae_n_ratios=0), r"ae_n_ratios must be 1\.\.4"),
    (dict(ae_n_ratios=5), r"ae_n_ratios must be 1\.\.4"),
    (dict(ae_kernel=0), "must be >= 1"),
    (dict(ae_res_kernel=0), "must be >= 1"),
    (dict(ae_last_kernel=0), "must be >= 1"),
    (dict(ae_ratios=[4, 0, 6, 8]), "ae_ratios must be >= 1"),
    (dict(ae_kernel=8193), "first audio conv" + _DEEP),                                             # 8193 x 1
    (dict(ae_res_kernel=33), "residual conv" + _DEEP),                                              # 33 x 256 in the last stage
    (dict(ae_ratios=[4, 5, 6, 200]), "strided conv" + _DEEP),                                       # 400 x 256
    (dict(ae_last_kernel=17), "last audio conv" + _DEEP),                                           # 17 x 512
    (dict(ae_hidden=24), "ae_hidden / ae_d_ffn"),
    (dict(ae_d_ffn=0), "ae_hidden / ae_d_ffn"),
    (dict(ae_n_layer=-1), "bad transformer shape"),
    (dict(ae_n_layer=65), "bad transformer shape"),
    (dict(ae_n_head=0), "bad transformer shape"),
    (dict(ae_head_dim=0), "bad transformer shape"),
    (dict(ae_head_dim=6, ae_n_head=8), "bad transformer shape"),
    (dict(ae_head_dim=260, ae_n_head=4), "bad transformer shape"),
    (dict(ae_head_dim=8, ae_n_head=1), "bad transformer shape"),
    (dict(ae_window=0), r"ae_window must be 1\.\.8192"),
    (dict(ae_window=8193), r"ae_window must be 1\.\.8192"),
    (dict(ae_down_stride=0), "ae_down_stride must be >= 1"),
    (dict(ae_hidden=8208), "QKV / FC1 / VQ projection" + _DEEP),
    (dict(ae_n_head=33, ae_head_dim=256), "O projection" + _DEEP),                                  # 33 x 256
    (dict(ae_d_ffn=8208), "FC2" + _DEEP),
    (dict(ae_down_stride=33), "frame-rate conv" + _DEEP),                                           # 66 x 128
    (dict(ae_vq_dim=24), "ae_vq_dim must be a multiple of 16"),
    (dict(ae_vq_dim=0), "ae_vq_dim must be a multiple of 16"),
    (dict(ae_vq_dim=4112), "ae_vq_dim must be a multiple of 16"),
    (dict(ae_n_codebooks=0), "bad codebook shape"),
    (dict(ae_n_codebooks=65), "bad codebook shape"),
    (dict(ae_codebook_size=0), "bad codebook shape"),
]


def test_every_rule_of_validate_refuses_on_the_host(shapes):
    """q3tts_clone_init validates before it touches the device or the encoders it holds: every refusal leaves the loaded shape answering
    with the oracle's bits."""
    from q3tts import _abi
    eng = shapes.use("audio", "down3")
    for fields, msg in REFUSALS:
        with pytest.raises(_abi.Q3Error, match="clone config: .*" + msg):
            eng.clone_init(S.make(**fields))
    n = 960 * 6
    codes_ref, lat_ref = S.audio_ref("down3", n)
    assert np.array_equal(_bits(eng.audio_latent(S.clip(n, n))), _bits(lat_ref))
    assert np.array_equal(eng.audio_encode(S.clip(n, n)), codes_ref.astype(np.int64))

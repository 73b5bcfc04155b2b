"""ctypes loader for oracle/libq3oracle.so — the CPU restatement used ONLY as the checker.

Imported by tests/, __graft_entry__.smoke() and bench.py's cpu_baseline leg; never by the product package.
"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "qwen3-tts-rust_amd"))
from q3tts import _abi  # noqa: E402  (struct layouts only; the oracle restates the same fields)

ORACLE_DIR = os.path.join(REPO, "oracle")
ORACLE_LIB = os.path.join(ORACLE_DIR, "libq3oracle.so")

f32p, i32p, u32p = C.POINTER(C.c_float), C.POINTER(C.c_int32), C.POINTER(C.c_uint32)
_lib = None

# The vocoder transformer's rows on the device against the bf16-input oracle (tests/test_long_gpu.py): per frame, RMS(device - oracle) /
# RMS(oracle) after the final norm. Measured on MI355X over 160 frames: <= 2.3e-5 from position 71 on (where the window cuts), 5.9e-5 at
# frame 0 (the noise floor of bf16 operand roundings that flip with the accumulation order). tests/test_vocoder_family_cpu.py shows that
# a sliding window off by one moves the oracle's own rows by >= 10x VOC_LATENT_TOL at every position past the window.
VOC_LATENT_TOL = 4e-5         # frames >= 71
VOC_LATENT_TOL_EARLY = 1e-4   # frames < 71

# The attention kernels against the two-stage float64 reference (tests/_attend_ref.py, tests/test_attend_{cpu,gpu}.py), stage 2: scores, softmax
# and the value sum in float64 from the f32 q and the bf16 K / V as cached; worst |out - float64| / max |V| of the (slot, KV head). MEASURED is
# the CPU oracle's own worst error per input kind over exactly the cases of the GPU file (tests/test_attend_cpu.py prints and re-checks it),
# never device output; the bound is twice the largest. The device must equal the oracle bit for bit, so on these seeds it has these errors:
# the margin is for other seeds only.
# Stage 1 on the same run: 7 054 208 cached K elements, 1.86e-3 of them within the midpoint window (cap 5e-3), 105 cached as the other neighbour.
ATT_STAGE2_MEASURED = {"normal": 3.48e-07, "wide": 8.00e-06, "first": 1.71e-06, "newest": 2.07e-12, "uniform": 1.87e-08, "outliers": 3.43e-07,
                       "zero_block": 3.17e-07}
ATT_STAGE2_TOL = 1.6e-05      # 2 x 8.00e-06 (wide); the issue's ceiling for it is 2e-5

# The vocoder's convolution half, stage by stage against float64 (tests/_voc_ref.py, tests/test_vocoder_stages_{cpu,gpu}.py). R below is
# NOT taken from device output: it is the worst error of the CPU restatement of each stage against float64 on the bf16-input oracle's
# own activations (4 frames, random codes and one repeated frame), per element, normalised by sqrt(sum_i (x_i w_i)^2) — for the GEMM
# stages the chain of q3o_mfma_bf16_dot32 (the pinned model of v_mfma_f32_16x16x32_bf16, which truncates) over K in the kernels' vstep
# order, for k_voc_dw_ln and the output convolution the oracle's sequential f32 code on the scale written in _voc_ref.check_call.
# Produced by `python tools/voc_stage_bounds.py` (CPU only, ~4 minutes). The device's bound for a stage is 4 R (VOC_STAGE_MARGIN): it
# sums the same K in another grouping (K slices, split accumulators), so its error has this scale but not this value, while an
# indexing error is of order 1 on it. Element-wise f32 roundings, sinf / erff and the bf16 output step are added as stated in _voc_ref.
# The front half (tests/_voc_tfm_ref.py, tests/test_vocoder_tfm_stages_{cpu,gpu}.py) adds the keys pre / qkv / o / gu / down (the chain of
# q3o_mfma_bf16_dot32 over the 32-wide K steps, on sqrt(sum_i (x_i w_i)^2)), rmsnorm and attn (the oracle's sequential f32 code on the scales
# written in _voc_tfm_ref.check_tfm_call), measured over every 4-frame call of sliding_window + 12 frames, rounded up to the printed digits;
# `python tools/voc_stage_bounds.py tfm` prints them alone (~2 minutes). Shapes without a convolution-half entry share the tiny one's.
VOC_STAGE_MARGIN = 4.0
VOC_STAGE_R = {
    "tiny": {"blk_ct": 1.84e-06, "dec_in": 1.30e-06, "dw_ln": 1.17e-07, "out": 4.35e-07, "pw1": 3.93e-07, "pw2": 6.29e-07, "res_c1": 2.79e-06, "res_c2": 1.05e-06, "up_ct": 3.08e-07,
             "attn": 5.97e-08, "down": 5.38e-07, "gu": 4.54e-07, "o": 2.88e-07, "pre": 3.98e-07, "qkv": 3.32e-07, "rmsnorm": 2.45e-07},
    "narrow": {"blk_ct": 2.56e-06, "dec_in": 9.05e-07, "dw_ln": 1.17e-07, "out": 5.85e-07, "pw1": 3.93e-07, "pw2": 6.29e-07, "res_c1": 3.13e-06, "res_c2": 1.31e-06, "up_ct": 3.08e-07},
    "full": {"blk_ct": 3.48e-06, "dec_in": 5.05e-06, "dw_ln": 2.02e-07, "out": 4.99e-07, "pw1": 1.97e-06, "pw2": 4.31e-06, "res_c1": 5.12e-06, "res_c2": 1.95e-06, "up_ct": 1.69e-06,
             "attn": 1.56e-07, "down": 4.65e-06, "gu": 2.52e-06, "o": 2.43e-06, "pre": 2.19e-06, "qkv": 2.51e-06, "rmsnorm": 1.13e-06},
    "hd128": {"attn": 6.58e-08, "down": 1.25e-06, "gu": 9.64e-07, "o": 7.90e-07, "pre": 4.14e-07, "qkv": 9.96e-07, "rmsnorm": 4.63e-07},
    "hd64t": {"attn": 9.78e-08, "down": 8.03e-07, "gu": 7.36e-07, "o": 7.26e-07, "pre": 4.14e-07, "qkv": 9.96e-07, "rmsnorm": 4.18e-07},
    "hd96": {"attn": 5.14e-08, "down": 3.71e-07, "gu": 3.15e-07, "o": 3.50e-07, "pre": 3.98e-07, "qkv": 4.47e-07, "rmsnorm": 2.18e-07},
    "hd48": {"attn": 6.77e-08, "down": 3.93e-07, "gu": 3.56e-07, "o": 3.71e-07, "pre": 3.98e-07, "qkv": 4.47e-07, "rmsnorm": 2.59e-07},
    "w1": {"attn": 0.00e+00, "down": 4.69e-07, "gu": 2.61e-07, "o": 2.41e-07, "pre": 3.98e-07, "qkv": 3.32e-07, "rmsnorm": 2.15e-07},
    "w508": {"attn": 5.00e-07, "down": 6.13e-07, "gu": 4.46e-07, "o": 3.95e-07, "pre": 4.44e-07, "qkv": 4.44e-07, "rmsnorm": 3.52e-07},
}

# The Q8_0 Talker away from O(1) magnitudes (tests/_q8_scales.py, tests/test_q8_scales_{cpu,gpu}.py). W8A8 quantises an activation from the
# UN-normalised v = x * nw; ggml quantises the normalised row. Entries are (mean, sample standard deviation) at e = 0 (rows of O(1)), taken
# on the CPU oracle, never from device output; `python tests/_q8_scales.py` prints the table (CPU only, ~5 s).
#   gemm / resid / swiglu: (error of this design against float64) / (error of ggml's order against float64), 8 seeds. The two orders
#     round different f32 values to int8, so the ratio is 1 up to the sampling noise of those roundings; the producers' ratio is exactly 1
#     (the same values are rounded) and borrows the GEMM's spread. A magnitude passes when ratio <= mean + Q8_SCALE_SIGMAS * std.
#   talker_1 / talker_2: relative RMS of the tiny model's prefill logits in mode 1 (W8A16) / 2 (W8A8) against the bf16 mode, 5 prompts.
#     The prompt's magnitude changes which term dominates the residual stream (rms_eps, the first block's output), so the figure moves with
#     it in EVERY mode: the bound on a mode's figure at 2^e is Q8_TALKER_MARGIN x its e = 0 mean (a lost block or a flushed scale is an O(1)
#     error, > 50 x the figure), and mode 2 may exceed mode 1 AT THE SAME e by no more than sqrt(2) (two independent Q8_0 roundings of equal
#     relative size add in quadrature) times 1 + Q8_SCALE_SIGMAS x the combined relative spread below.
Q8_SCALE_SIGMAS = 4.0
Q8_TALKER_MARGIN = 2.0
Q8_SCALE_RATIO = {
    "gemm": (0.999223, 0.00143),
    "resid": (1.0, 0.00143),
    "swiglu": (1.0, 0.00143),
    "talker_1": (0.0131648, 0.000192),
    "talker_2": (0.0175642, 0.000311),
}


def build():
    subprocess.check_call(["make", "-C", ORACLE_DIR, "libq3oracle.so"], stdout=subprocess.DEVNULL)


def lib():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(ORACLE_LIB):
        build()
    L = C.CDLL(ORACLE_LIB)
    vp = C.c_void_p
    L.q3o_create.argtypes = [C.POINTER(_abi.ModelConfig), C.c_uint64, C.c_int32, C.c_int32]
    L.q3o_create.restype = vp
    L.q3o_destroy.argtypes = [vp]
    L.q3o_destroy.restype = None
    L.q3o_expf.argtypes = [C.c_float]
    L.q3o_expf.restype = C.c_float
    L.q3o_synth.argtypes = [C.c_uint64, C.c_uint32, C.c_uint64, C.c_float]
    L.q3o_synth.restype = C.c_float
    L.q3o_bf16.argtypes = [C.c_float]
    L.q3o_bf16.restype = C.c_uint16
    L.q3o_synth_fill.argtypes = [C.c_uint64, C.c_uint32, C.c_uint64, C.c_float, C.c_float, C.c_int32, f32p]
    L.q3o_synth_fill.restype = None
    L.q3o_gemm_exact.argtypes = [f32p, C.c_int32, C.c_int32, C.POINTER(C.c_uint16), C.c_int32, f32p, C.c_float, f32p,
                                 C.c_int32, f32p, C.POINTER(C.c_uint64)]
    L.q3o_gemm_exact.restype = None
    L.q3o_rmsnorm.argtypes = [f32p, C.c_int32, f32p, C.c_float, f32p]
    L.q3o_rmsnorm.restype = None
    L.q3o_attention.argtypes = [f32p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, f32p, f32p, C.c_float,
                                C.c_float, i32p, f32p]
    L.q3o_attention.restype = None
    L.q3o_attention_last.argtypes = [f32p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, f32p, f32p, C.c_float, C.c_float, i32p, f32p]
    L.q3o_attention_last.restype = None
    L.q3o_attention_prep.argtypes = [f32p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, f32p, f32p, C.c_float, C.c_float, i32p,
                                     f32p, f32p, f32p]
    L.q3o_attention_prep.restype = None
    L.q3o_attention_kv_q8.argtypes = [f32p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, f32p, f32p, C.c_float, C.c_float, i32p,
                                      C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.q3o_attention_kv_q8.restype = None
    L.q3o_sample.argtypes = [f32p, C.c_int32, C.c_float, C.c_int32, C.c_float, C.c_float]
    L.q3o_sample.restype = C.c_int32
    L.q3o_rng_f32.argtypes = [C.c_uint64, C.c_int32, f32p]
    L.q3o_rng_f32.restype = None
    L.q3o_chacha_block.argtypes = [u32p, C.c_int32, u32p]
    L.q3o_chacha_block.restype = None
    L.q3o_qwen3_position.argtypes = [C.c_int32, C.c_int32, i32p]
    L.q3o_qwen3_position.restype = None
    L.q3o_build_prompt.argtypes = [vp, C.POINTER(_abi.PromptDesc), f32p, C.c_int32]
    L.q3o_build_prompt.restype = C.c_int32
    L.q3o_text_embedding.argtypes = [vp, C.c_int64, f32p]
    L.q3o_text_embedding.restype = None
    L.q3o_codec_embedding.argtypes = [vp, C.c_int32, C.c_int32, f32p]
    L.q3o_codec_embedding.restype = None
    L.q3o_project.argtypes = [vp, f32p, f32p]
    L.q3o_project.restype = None
    L.q3o_talker_prefill.argtypes = [vp, f32p, C.c_int32, f32p, f32p]
    L.q3o_talker_prefill.restype = None
    L.q3o_generate.argtypes = [vp, f32p, C.c_int32, C.c_float, C.c_int32, C.c_float, C.c_uint64, C.c_int32, C.c_int32,
                               C.c_int32, i32p, i32p]
    L.q3o_generate.restype = C.c_int32
    L.q3o_chunk_plan.argtypes = [C.c_int32, i32p, i32p, C.c_int32]
    L.q3o_chunk_plan.restype = C.c_int32
    L.q3o_mel_frames.argtypes = [C.c_int64]
    L.q3o_mel_frames.restype = C.c_int32
    L.q3o_mel.argtypes = [f32p, C.c_int64, f32p, f32p]
    L.q3o_mel.restype = C.c_int32
    L.q3o_audio_frames.argtypes = [C.POINTER(_abi.CloneConfig), C.c_int64]
    L.q3o_audio_frames.restype = C.c_int32
    L.q3o_speaker_encode.argtypes = [C.POINTER(_abi.CloneConfig), C.c_uint64, f32p, C.c_int32, f32p]
    L.q3o_speaker_encode.restype = C.c_int32
    L.q3o_audio_encode.argtypes = [C.POINTER(_abi.CloneConfig), C.c_uint64, f32p, C.c_int64, i32p, C.c_int32, f32p]
    L.q3o_audio_encode.restype = C.c_int32
    L.q3o_rvq.argtypes = [f32p, f32p, C.c_int32, C.c_int32, f32p, C.c_int32, C.c_int32, i32p]
    L.q3o_rvq.restype = C.c_int32
    u16p = C.POINTER(C.c_uint16)
    L.q3o_mfma_bf16_dot32.argtypes = [u16p, u16p, C.c_float]
    L.q3o_mfma_bf16_dot32.restype = C.c_float
    L.q3o_mfma_bf16_dot32_ref.argtypes = [u16p, u16p, C.c_float]
    L.q3o_mfma_bf16_dot32_ref.restype = C.c_float
    L.q3o_bgemm.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.c_float, C.c_int32,
                            C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.q3o_bgemm.restype = None
    L.q3o_bgemm_q8.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.c_float, C.c_int32,
                               C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.q3o_bgemm_q8.restype = None
    L.q3o_quantize_q8_0.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
    L.q3o_quantize_q8_0.restype = None
    L.q3o_quantize_q8_0_act.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
    L.q3o_quantize_q8_0_act.restype = None
    L.q3o_round_sig11.argtypes = [C.c_float]
    L.q3o_round_sig11.restype = C.c_float
    L.q3o_bgemm_q8a8.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.c_float, C.c_int32,
                                 C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.q3o_bgemm_q8a8.restype = None
    L.q3o_bgemm_q8a8_f32.argtypes = L.q3o_bgemm_q8a8.argtypes
    L.q3o_bgemm_q8a8_f32.restype = None
    L.q3o_set_talker_q8a8.argtypes = [vp]
    L.q3o_set_talker_q8a8.restype = None
    L.q3o_set_talker_kv_q8.argtypes = [vp]
    L.q3o_set_talker_kv_q8.restype = None
    L.q3o_set_talker_q8.argtypes = [vp]
    L.q3o_set_talker_q8.restype = None
    L.q3o_project_rows.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p]
    L.q3o_project_rows.restype = None
    L.q3o_norm_inputs.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
    L.q3o_norm_inputs.restype = None
    L.q3o_row_scale.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_float]
    L.q3o_row_scale.restype = C.c_float
    L.q3o_set_threads.argtypes = [C.c_int32]
    L.q3o_set_threads.restype = None
    L.q3o_set_arith.argtypes = [vp, C.c_int32]
    L.q3o_set_arith.restype = None
    L.q3o_norm_weight.argtypes = [vp, C.c_int32, C.c_int32, C.c_int32]
    L.q3o_norm_weight.restype = f32p
    L.q3o_matrix.argtypes = [vp, C.c_int32, C.c_int32, C.c_int32, C.c_void_p]
    L.q3o_matrix.restype = C.c_int32
    if hasattr(L, "q3o_vocoder_create"):
        L.q3o_vocoder_create.argtypes = [C.POINTER(_abi.VocoderConfig), C.c_uint64, C.c_int32]
        L.q3o_vocoder_create.restype = vp
        L.q3o_vocoder_destroy.argtypes = [vp]
        L.q3o_vocoder_destroy.restype = None
        L.q3o_vocoder_reset.argtypes = [vp]
        L.q3o_vocoder_reset.restype = None
        L.q3o_vocoder_set_arith.argtypes = [vp, C.c_int32]
        L.q3o_vocoder_set_arith.restype = None
        L.q3o_vocoder_decode.argtypes = [vp, i32p, C.c_int32, C.c_int32, f32p, C.c_int32]
        L.q3o_vocoder_decode.restype = C.c_int32
    _lib = L
    return L


def ptr(a, typ):
    return a.ctypes.data_as(typ)


from q3tts.native import make_prompt_desc  # noqa: E402,F401  (struct packing helper of the product package)


class OracleModel:
    def __init__(self, model_cfg, seed=0, n_ctx=256, n_threads=4):
        self.cfg = model_cfg
        self.L = lib()
        self.h = self.L.q3o_create(C.byref(model_cfg), seed, n_ctx, n_threads)
        if not self.h:
            raise RuntimeError("q3o_create failed")

    def close(self):
        if self.h:
            self.L.q3o_destroy(self.h)
            self.h = None

    def __del__(self):
        self.close()

    def set_talker_q8(self):
        """The Talker's matrices + lm_head as ggml Q8_0 blocks in the canonical Q8 order (device: q3tts_engine_config.talker_q8_0 = 1). One-way."""
        self.L.q3o_set_talker_q8(self.h)

    def set_talker_q8a8(self):
        """... and every Talker GEMM's activations as Q8_0 blocks as well: ggml's W8A8 (device: talker_q8_0 = 2). One-way."""
        self.L.q3o_set_talker_q8a8(self.h)

    def set_talker_kv_q8(self):
        """The Talker's K/V cache as ggml Q8_0 blocks (device: q3tts_engine_config.kv_q8_0 = 1). One-way; combines with
        set_talker_q8 / set_talker_q8a8. The Predictor's cache stays bf16."""
        self.L.q3o_set_talker_kv_q8(self.h)

    def set_arith(self, mode):
        """0: the canonical bf16-MFMA order (default); 1: plain f32 of the same structure (family pinning)."""
        self.L.q3o_set_arith(self.h, mode)

    def matrix(self, talker, layer, which):
        """Natural-order f32 copy of one synthetic matrix: which 0 qkv, 1 o, 2 gate, 3 up, 4 down, 5 head."""
        n = self.L.q3o_matrix(self.h, int(talker), layer, which, None)
        c = self.cfg
        d, nq, F = (c.t_d_model, c.t_n_head * c.t_head_dim, c.t_d_ffn) if talker else (c.p_d_model, c.p_n_head * c.p_head_dim, c.p_d_ffn)
        K = {0: d, 1: nq, 2: d, 3: d, 4: F, 5: d}[which]
        out = np.zeros((n, K), dtype=np.float32)
        self.L.q3o_matrix(self.h, int(talker), layer, which, out.ctypes.data)
        return out

    def norm_weight(self, talker, layer, which, n):
        """which 0 attn_norm, 1 ffn_norm, 2 q_norm, 3 k_norm; layer < 0: the output norm."""
        return np.ctypeslib.as_array(self.L.q3o_norm_weight(self.h, int(talker), layer, which), shape=(n,)).copy()

    def build_prompt(self, desc):
        n = self.L.q3o_build_prompt(self.h, C.byref(desc), None, 0)
        out = np.zeros((n, self.cfg.d_embed), dtype=np.float32)
        self.L.q3o_build_prompt(self.h, C.byref(desc), ptr(out, f32p), n)
        return out

    def talker_prefill(self, embd):
        embd = np.ascontiguousarray(embd, dtype=np.float32)
        hid = np.zeros(self.cfg.t_d_model, dtype=np.float32)
        logits = np.zeros(self.cfg.t_vocab, dtype=np.float32)
        self.L.q3o_talker_prefill(self.h, ptr(embd, f32p), embd.shape[0], ptr(hid, f32p), ptr(logits, f32p))
        return hid, logits

    def generate(self, embd, temperature=0.0, top_k=40, top_p=0.9, seed=0, max_steps=16, min_frames=0, force_eos_at=-1):
        embd = np.ascontiguousarray(embd, dtype=np.float32)
        codes = np.zeros((max_steps, self.cfg.n_codebooks), dtype=np.int32)
        eos = C.c_int32(0)
        n = self.L.q3o_generate(self.h, ptr(embd, f32p), embd.shape[0], temperature, top_k, top_p, seed, max_steps,
                                min_frames, force_eos_at, ptr(codes, i32p), C.byref(eos))
        return codes[:n].copy(), bool(eos.value)


def bgemm(xb, wb, ssp, d_norm, eps, epi, nw_next=None, y0=None):
    """oracle/q3_oracle_bf16.c q3o_bgemm on natural-order bf16 bit arrays; returns the outputs of the epilogue as a dict."""
    xb = np.ascontiguousarray(xb, dtype=np.uint16); wb = np.ascontiguousarray(wb, dtype=np.uint16)
    B, K = xb.shape
    N = wb.shape[0]
    y = np.zeros((B, N), dtype=np.float32) if y0 is None else np.ascontiguousarray(y0, dtype=np.float32).copy()
    yb = np.zeros((B, N // 2 if epi == 2 else N), dtype=np.uint16)
    sso = np.zeros((B, N // 16), dtype=np.float32)
    keys = np.zeros(B, dtype=np.uint64)
    sp = None if ssp is None else np.ascontiguousarray(ssp, dtype=np.float32)
    nw = None if nw_next is None else np.ascontiguousarray(nw_next, dtype=np.float32)
    lib().q3o_bgemm(xb.ctypes.data, B, K, wb.ctypes.data, N, None if sp is None else sp.ctypes.data, 0 if sp is None else sp.shape[1], d_norm, eps, epi,
                    None if nw is None else nw.ctypes.data, y.ctypes.data, yb.ctypes.data, sso.ctypes.data, keys.ctypes.data)
    return dict(y=y, yb=yb, ssp_out=sso, keys=keys)


def attention_kv_q8(x, attend_from, Hq, Hkv, hd, qn, kn, eps, theta, sections):
    """q3o_attention_kv_q8 on one sequence's qkv rows x [tot][(Hq + 2 Hkv) hd] at positions 0 .. tot - 1: (out [tot - attend_from][Hq hd] f32,
    k_q, k_d, v_q, v_d) — the cache in natural order, [tot][Hkv][hd] int8 and [tot][Hkv][hd / 32] f16 bits."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    qn = np.ascontiguousarray(qn, dtype=np.float32); kn = np.ascontiguousarray(kn, dtype=np.float32)
    sec = np.ascontiguousarray(sections, dtype=np.int32)
    tot = x.shape[0]
    assert x.shape[1] == (Hq + 2 * Hkv) * hd and 0 <= attend_from <= tot
    out = np.zeros((tot - attend_from, Hq * hd), dtype=np.float32)
    k_q = np.zeros((tot, Hkv, hd), dtype=np.int8); v_q = np.zeros((tot, Hkv, hd), dtype=np.int8)
    k_d = np.zeros((tot, Hkv, hd // 32), dtype=np.uint16); v_d = np.zeros((tot, Hkv, hd // 32), dtype=np.uint16)
    lib().q3o_attention_kv_q8(ptr(x, f32p), tot, attend_from, Hq, Hkv, hd, ptr(qn, f32p), ptr(kn, f32p), eps, theta, ptr(sec, i32p),
                              out.ctypes.data, k_q.ctypes.data, k_d.ctypes.data, v_q.ctypes.data, v_d.ctypes.data)
    return out, k_q, k_d, v_q, v_d


def quantize_q8_0(x):
    """ggml's reference Q8_0 quantiser through the oracle's C restatement: x [..., K] f32 -> (q int8 same shape, d f16 bits [..., K/32])."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    q = np.zeros(x.shape, dtype=np.int8); d = np.zeros(x.shape[:-1] + (x.shape[-1] // 32,), dtype=np.uint16)
    lib().q3o_quantize_q8_0(x.ctypes.data, x.size, q.ctypes.data, d.ctypes.data)
    return q, d


def quantize_q8_0_act(x):
    """ggml's quantiser on ACTIVATION rows as the W8A8 producers apply it (q3o_quantize_q8_0_act): x [..., K] f32 -> (q int8 same shape,
    d f32 [..., K/32]) with d = amax / 127 rounded to f16's 11-bit significand but kept in f32."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    q = np.zeros(x.shape, dtype=np.int8); d = np.zeros(x.shape[:-1] + (x.shape[-1] // 32,), dtype=np.float32)
    lib().q3o_quantize_q8_0_act(x.ctypes.data, x.size, q.ctypes.data, d.ctypes.data)
    return q, d


def bgemm_q8a8(aq, ad, q, d16, ssp, d_norm, eps, epi, nw_next=None, y0=None):
    """oracle/q3_oracle_bf16.c q3o_bgemm_q8a8: ggml's Q8_0 x Q8_0 arithmetic (exact int32 block sums x f32(d_w) * f32(d_x)), the quantising epilogues.
    ad: the activation scales — f32 as the kernels hold them (q3o_bgemm_q8a8_f32; yd comes back as f32), or f16 bit patterns (uint16: widened
    exactly, yd comes back as f16 bit patterns, exact wherever the produced scale is a normal f16)."""
    aq = np.ascontiguousarray(aq, dtype=np.int8); ad = np.ascontiguousarray(ad)
    assert ad.dtype in (np.uint16, np.float32), ad.dtype
    f32 = ad.dtype == np.float32
    q = np.ascontiguousarray(q, dtype=np.int8); d16 = np.ascontiguousarray(d16, dtype=np.uint16)
    B, K = aq.shape
    N = q.shape[0]
    nout = N // 2 if epi == 2 else N
    y = np.zeros((B, N), dtype=np.float32) if y0 is None else np.ascontiguousarray(y0, dtype=np.float32).copy()
    yq = np.zeros((B, nout), dtype=np.int8); yd = np.zeros((B, nout // 32), dtype=np.float32 if f32 else np.uint16)
    sso = np.zeros((B, N // 16), dtype=np.float32)
    sp = None if ssp is None else np.ascontiguousarray(ssp, dtype=np.float32)
    nw = None if nw_next is None else np.ascontiguousarray(nw_next, dtype=np.float32)
    (lib().q3o_bgemm_q8a8_f32 if f32 else lib().q3o_bgemm_q8a8)(aq.ctypes.data, ad.ctypes.data, B, K, q.ctypes.data, d16.ctypes.data, N, None if sp is None else sp.ctypes.data,
                         0 if sp is None else sp.shape[1], d_norm, eps, epi, None if nw is None else nw.ctypes.data, y.ctypes.data, yq.ctypes.data,
                         yd.ctypes.data, sso.ctypes.data)
    return dict(y=y, yq=yq, yd=yd, ssp_out=sso)


def bgemm_q8(xb, q, d16, ssp, d_norm, eps, epi, nw_next=None, y0=None):
    """oracle/q3_oracle_bf16.c q3o_bgemm_q8: the canonical Q8_0 order (per block P = MFMA from zero, t = fmaf(f32(d), P, t))."""
    xb = np.ascontiguousarray(xb, dtype=np.uint16); q = np.ascontiguousarray(q, dtype=np.int8); d16 = np.ascontiguousarray(d16, dtype=np.uint16)
    B, K = xb.shape
    N = q.shape[0]
    y = np.zeros((B, N), dtype=np.float32) if y0 is None else np.ascontiguousarray(y0, dtype=np.float32).copy()
    yb = np.zeros((B, N // 2 if epi == 2 else N), dtype=np.uint16)
    sso = np.zeros((B, N // 16), dtype=np.float32)
    keys = np.zeros(B, dtype=np.uint64)
    sp = None if ssp is None else np.ascontiguousarray(ssp, dtype=np.float32)
    nw = None if nw_next is None else np.ascontiguousarray(nw_next, dtype=np.float32)
    lib().q3o_bgemm_q8(xb.ctypes.data, B, K, q.ctypes.data, d16.ctypes.data, N, None if sp is None else sp.ctypes.data, 0 if sp is None else sp.shape[1],
                       d_norm, eps, epi, None if nw is None else nw.ctypes.data, y.ctypes.data, yb.ctypes.data, sso.ctypes.data, keys.ctypes.data)
    return dict(y=y, yb=yb, ssp_out=sso, keys=keys)


def project_rows(w, b, x):
    w = np.ascontiguousarray(w, dtype=np.float32); b = np.ascontiguousarray(b, dtype=np.float32); x = np.ascontiguousarray(x, dtype=np.float32)
    y = np.zeros((x.shape[0], w.shape[0]), dtype=np.float32)
    lib().q3o_project_rows(w.ctypes.data, b.ctypes.data, w.shape[1], w.shape[0], x.ctypes.data, x.shape[0], y.ctypes.data)
    return y


def norm_inputs(x, nw):
    x = np.ascontiguousarray(x, dtype=np.float32); nw = np.ascontiguousarray(nw, dtype=np.float32)
    rows, d = x.shape
    xb = np.zeros((rows, d), dtype=np.uint16); ssp = np.zeros((rows, d // 16), dtype=np.float32)
    for r in range(rows):
        lib().q3o_norm_inputs(x[r].ctypes.data, d, nw.ctypes.data, xb[r].ctypes.data, ssp[r].ctypes.data)
    return xb, ssp


def row_scale(ssp_row, d, eps):
    sp = np.ascontiguousarray(ssp_row, dtype=np.float32)
    return float(lib().q3o_row_scale(sp.ctypes.data, sp.size, d, eps))


# ---- the synthetic model as files (loader parity): same tensor ids / scales as oracle/q3_oracle.c tfm_init, q3o_create
_G_TALKER, _G_PRED, _G_ASSET = 1, 2, 3
_W = dict(attn_norm=0, q=1, k=2, v=3, qnorm=4, knorm=5, o=6, ffn_norm=7, gate=8, up=9, down=10)
_L_MODEL = 255


def _tid(g, l, w):
    return (g << 16) | (l << 8) | w


def synth_tensor(seed, tid, shape, base, std, round_bf16):
    out = np.zeros(int(np.prod(shape)), dtype=np.float32)
    lib().q3o_synth_fill(seed, tid, out.size, base, std, 1 if round_bf16 else 0, ptr(out, f32p))
    return out.reshape(shape)


def synth_transformer_tensors(m, seed, talker):
    """llama.cpp qwen3 tensor names -> f32 arrays of the synthetic Talker / Predictor (matrices are bf16-exact)."""
    if talker:
        g, L, d, Hq, Hkv, hd, F, head_n = _G_TALKER, m.t_n_layer, m.t_d_model, m.t_n_head, m.t_n_kv_head, m.t_head_dim, m.t_d_ffn, m.t_vocab
    else:
        g, L, d, Hq, Hkv, hd, F = _G_PRED, m.p_n_layer, m.p_d_model, m.p_n_head, m.p_n_kv_head, m.p_head_dim, m.p_d_ffn
        head_n = (m.n_codebooks - 1) * m.codebook_size
    nq, nkv = Hq * hd, Hkv * hd
    t = {}
    for l in range(L):
        b = "blk.%d." % l
        t[b + "attn_norm.weight"] = synth_tensor(seed, _tid(g, l, _W["attn_norm"]), (d,), 1.0, 0.05, False)
        t[b + "ffn_norm.weight"] = synth_tensor(seed, _tid(g, l, _W["ffn_norm"]), (d,), 1.0, 0.05, False)
        t[b + "attn_q_norm.weight"] = synth_tensor(seed, _tid(g, l, _W["qnorm"]), (hd,), 1.0, 0.05, False)
        t[b + "attn_k_norm.weight"] = synth_tensor(seed, _tid(g, l, _W["knorm"]), (hd,), 1.0, 0.05, False)
        t[b + "attn_q.weight"] = synth_tensor(seed, _tid(g, l, _W["q"]), (nq, d), 0.0, 0.02, True)
        t[b + "attn_k.weight"] = synth_tensor(seed, _tid(g, l, _W["k"]), (nkv, d), 0.0, 0.02, True)
        t[b + "attn_v.weight"] = synth_tensor(seed, _tid(g, l, _W["v"]), (nkv, d), 0.0, 0.02, True)
        t[b + "attn_output.weight"] = synth_tensor(seed, _tid(g, l, _W["o"]), (d, nq), 0.0, 0.02, True)
        t[b + "ffn_gate.weight"] = synth_tensor(seed, _tid(g, l, _W["gate"]), (F, d), 0.0, 0.02, True)
        t[b + "ffn_up.weight"] = synth_tensor(seed, _tid(g, l, _W["up"]), (F, d), 0.0, 0.02, True)
        t[b + "ffn_down.weight"] = synth_tensor(seed, _tid(g, l, _W["down"]), (d, F), 0.0, 0.02, True)
    t["output_norm.weight"] = synth_tensor(seed, _tid(g, _L_MODEL, 0), (d,), 1.0, 0.05, False)
    t["output.weight"] = synth_tensor(seed, _tid(g, _L_MODEL, 1), (head_n, d), 0.0, 0.02, True)
    return t


def synth_asset_tensors(m, seed, with_text=True):
    """qwen3_assets.gguf tensor names (src/assets_manager.rs:212-241) -> f32 arrays of the synthetic assets."""
    d = m.d_embed
    t = {"proj.weight": synth_tensor(seed, _tid(_G_ASSET, 0, 1), (m.p_d_model, d), 0.0, 0.02, True),
         "proj.bias": synth_tensor(seed, _tid(_G_ASSET, 0, 2), (m.p_d_model,), 0.0, 0.02, False)}
    if with_text:
        t["text_embd"] = synth_tensor(seed, _tid(_G_ASSET, 0, 0), (m.text_vocab, d), 0.0, 0.05, True)
    for q in range(m.n_codebooks):
        rows = m.codec0_rows if q == 0 else m.codecq_rows
        t["codec_embd.%d" % q] = synth_tensor(seed, _tid(_G_ASSET, 1 + q, 0), (rows, d), 0.0, 0.05, True)
    return t


def write_model_dir(path, m, seed, matrix_type=30, assets="gguf", with_text=True, predictor_type=None):
    """The synthetic model as the reference's quant directory: two llama.cpp-style GGUFs + qwen3_assets.gguf (or NPY).
    predictor_type: tensor type of the Predictor's matrices when it differs from the Talker's (matrix_type)."""
    import _gguf as G
    os.makedirs(path, exist_ok=True)
    for talker, fname in ((True, "qwen3_tts_talker.gguf"), (False, "qwen3_tts_predictor.gguf")):
        tens = synth_transformer_tensors(m, seed, talker)
        mt = matrix_type if (talker or predictor_type is None) else predictor_type
        G.write(os.path.join(path, fname), [(k, v, mt if v.ndim == 2 else G.F32) for k, v in tens.items()],
                meta={"general.architecture": "qwen3", "general.alignment": 32, "qwen3.block_count": m.t_n_layer if talker else m.p_n_layer,
                      "tokenizer.ggml.tokens": ["<a>", "<b>"], "tokenizer.ggml.token_type": [1, 1]})
    at = synth_asset_tensors(m, seed, with_text)
    if assets == "gguf":
        G.write(os.path.join(path, "qwen3_assets.gguf"), [(k, v, G.F32) for k, v in at.items()], meta={"general.architecture": "qwen3-tts-assets"})
    else:  # the legacy NPY layout (src/assets_manager.rs:267-300)
        np.save(os.path.join(path, "proj_weight.npy"), at["proj.weight"])
        np.save(os.path.join(path, "proj_bias.npy"), at["proj.bias"])
        if with_text:
            np.save(os.path.join(path, "text_embedding_projected.npy"), at["text_embd"])
        for q in range(m.n_codebooks):
            np.save(os.path.join(path, "codec_embedding_%d.npy" % q), at["codec_embd.%d" % q])


def mel(audio, want_pre_log=False):
    """Oracle log-mel (oracle/q3_oracle_mel.c): [n_frames][128]."""
    a = np.ascontiguousarray(audio, dtype=np.float32)
    cap = max(1, int(lib().q3o_mel_frames(a.size)))
    out = np.zeros((cap, 128), dtype=np.float32)
    pre = np.zeros((cap, 128), dtype=np.float32)
    n = lib().q3o_mel(ptr(a, f32p) if a.size else None, a.size, ptr(out, f32p), ptr(pre, f32p))
    return (out[:n].copy(), pre[:n].copy()) if want_pre_log else out[:n].copy()


def speaker_encode(ccfg, seed, mel_rows):
    """Oracle speaker encoder (oracle/q3_oracle_clone.c) on a log-mel [T][128] -> [se_dim]."""
    m = np.ascontiguousarray(mel_rows, dtype=np.float32)
    out = np.zeros(ccfg.se_dim, dtype=np.float32)
    rc = lib().q3o_speaker_encode(C.byref(ccfg), seed, ptr(m, f32p), m.shape[0], ptr(out, f32p))
    assert rc == 0
    return out


def audio_encode(ccfg, seed, audio):
    """Oracle audio encoder: (codes [frames][ncb] int32, pre-quantiser rows [frames][ae_hidden])."""
    a = np.ascontiguousarray(audio, dtype=np.float32)
    cap = max(1, int(lib().q3o_audio_frames(C.byref(ccfg), a.size)))
    codes = np.zeros((cap, ccfg.ae_n_codebooks), dtype=np.int32)
    lat = np.zeros((cap, ccfg.ae_hidden), dtype=np.float32)
    n = lib().q3o_audio_encode(C.byref(ccfg), seed, ptr(a, f32p) if a.size else None, a.size, ptr(codes, i32p), cap, ptr(lat, f32p))
    assert n >= 0
    return codes[:n].copy(), lat[:n].copy()


def rvq(ps, pa, books):
    """Oracle split residual VQ (q3o_rvq): ps / pa [T][D], books [ncb][CS][D] -> codes int32 [T][ncb]. pa may be None when ncb == 1."""
    bk = np.ascontiguousarray(books, dtype=np.float32)
    s = np.ascontiguousarray(ps, dtype=np.float32)
    a = None if pa is None else np.ascontiguousarray(pa, dtype=np.float32)
    ncb, CS, D = bk.shape
    codes = np.zeros((s.shape[0], ncb), dtype=np.int32)
    rc = lib().q3o_rvq(ptr(s, f32p), None if a is None else ptr(a, f32p), s.shape[0], D, ptr(bk, f32p), ncb, CS, ptr(codes, i32p))
    assert rc == 0
    return codes

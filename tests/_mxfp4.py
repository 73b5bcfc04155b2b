"""numpy restatements of the MXFP4 Talker's two quantisers: ggml's quantize_row_mxfp4 for the weights and the
OCP MX v1.0 MXFP8 (E4M3) conversion of the bf16 row operand. Nothing here imports the library."""
import numpy as np

KVALUES = np.array([0, 1, 2, 3, 4, 6, 8, 12, 0, -1, -2, -3, -4, -6, -8, -12], dtype=np.float32)  # ggml's kvalues_mxfp4: doubled E2M1


def quantize_row_mxfp4(w):
    """f32 [N][K] -> ggml block_mxfp4 rows uint8 [N][K/32][17]. e = floor(log2(amax)) - 2 + 127 from the float's exponent field, held at 0 from
    below, 0 for a zero block; d = 2^(e - 128); q = the FIRST index of KVALUES with the smallest |KVALUES[i] * d - x| in f32 (strict <)."""
    w = np.ascontiguousarray(w, dtype=np.float32)
    N, K = w.shape
    x = w.reshape(N, K // 32, 32)
    amax = np.abs(x).max(axis=2)
    ef = (amax.view(np.uint32) >> 23).astype(np.int64) & 0xff
    e = np.where(amax > 0, np.maximum(ef - 2, 0), 0).astype(np.uint8)
    eu = e.astype(np.uint32)      # GGML_E8M0_TO_FP32_HALF: 2^(e - 128) as f32, a subnormal for e < 2
    d = np.where(eu < 2, np.uint32(0x00200000) << eu, (eu - 1) << 23).astype(np.uint32).view(np.float32)[:, :, None, None]
    err = np.abs((KVALUES[None, None, None, :] * d).astype(np.float32) - x[:, :, :, None]).astype(np.float32)
    q = err.argmin(axis=3).astype(np.uint8)  # (argmin returns the first minimum)
    return pack_mxfp4(q.reshape(N, K), e)


def dequant_mxfp4(blocks):
    """block_mxfp4 rows [N][K/32][17] -> float64 [N][K]: 2^(e - 127) * KVALUES[q] / 2."""
    q = np.concatenate([blocks[:, :, 1:] & 0xF, blocks[:, :, 1:] >> 4], axis=2)
    return (KVALUES[q].astype(np.float64) * 0.5 * np.ldexp(1.0, blocks[:, :, 0].astype(np.int64) - 127)[:, :, None]).reshape(blocks.shape[0], -1)


def pack_mxfp4(codes, e):
    """E2M1 codes [N][K] (0..15) and scales [N][K/32] -> block_mxfp4 rows."""
    N, K = codes.shape
    q = codes.reshape(N, K // 32, 32).astype(np.uint8)
    out = np.empty((N, K // 32, 17), dtype=np.uint8)
    out[:, :, 0] = e
    out[:, :, 1:] = q[:, :, :16] | (q[:, :, 16:] << 4)
    return out


_C = np.arange(0x7f)
E4M3 = np.where(_C < 8, np.ldexp(_C.astype(np.float64), -9), np.ldexp(1.0 + (_C & 7) / 8.0, (_C >> 3) - 7))  # the 127 finite values >= 0, by code


def mx_fp8_rows(xb):
    """bf16 bits [B][K] -> (E4M3 [B][K], E8M0 [B][K/32]): E = max(exponent field of amax - 8, 0); x * 2^(127 - E) to nearest even, saturating at 448."""
    xb = np.ascontiguousarray(xb, dtype=np.uint16)
    B, K = xb.shape
    x = (xb.astype(np.uint32) << 16).view(np.float32).astype(np.float64).reshape(B, K // 32, 32)
    amax_bits = (xb & 0x7fff).reshape(B, K // 32, 32).max(axis=2).astype(np.int64)
    E = np.maximum((amax_bits >> 7) - 8, 0)
    a = np.minimum(np.abs(x) * np.ldexp(1.0, 127 - E)[:, :, None], 448.0)
    hi = np.searchsorted(E4M3, a, side="left").clip(0, 0x7e)  # first value >= a
    lo = np.maximum(hi - 1, 0)
    dl, dh = a - E4M3[lo], E4M3[hi] - a
    code = np.where((dl < dh) | ((dl == dh) & (lo % 2 == 0)), lo, hi)
    code = np.where(E4M3[hi] == a, hi, code)
    q = (code | np.where(np.signbit(x), 0x80, 0)).astype(np.uint8)
    return q.reshape(B, K), E.astype(np.uint8)


def dequant_fp8_rows(q, E):
    """(E4M3 bytes [B][K], E8M0 bytes [B][K/32]) -> float64 [B][K]."""
    v = E4M3[q & 0x7f] * np.where(q & 0x80, -1.0, 1.0)
    return v * np.repeat(np.ldexp(1.0, E.astype(np.int64) - 127), 32, axis=1)

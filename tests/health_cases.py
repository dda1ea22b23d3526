"""Cases and the numpy model of the headroom scan (include/ltk.h: ltk_health_scan; csrc/misc_kernels.hip health_scan_kernel).

A tensor is its raw codes: uint16 [N][cbt][P][16] (fp16) or uint8 [N][cbt][P][32] (e4m3fn); a view is channel blocks [cb0, cb0 + CB).
The model counts on the magnitude codes (the bits without the sign), as the kernel does: the integers are exact, max_abs is the
largest finite code decoded to float32.
"""
import numpy as np

F16_LIMIT, F16_NEAR, F16_INF = 0x7BFF, 0x7800, 0x7C00        # 65504; 32768 (first code of the top binade); inf, NaNs above
E4M3_LIMIT, E4M3_NEAR, E4M3_NAN = 0x7E, 0x78, 0x7F           # 448; 256; the one NaN code per sign (e4m3fn has no inf)


def decode_f16(code: int) -> np.float32:
    return np.array([code & 0x7FFF], dtype=np.uint16).view(np.float16).astype(np.float32)[0]


def decode_e4m3(code: int) -> np.float32:
    code &= 0x7F
    ex, m = code >> 3, code & 7
    v = np.ldexp(np.float64(m), -9) if ex == 0 else np.ldexp(1.0 + m / 8.0, ex - 7)
    return np.float32(v)


def scan_model(codes: np.ndarray, cb0: int, CB: int, q8: bool) -> dict:
    """What ltk_health_scan returns for the view (the fields of ltk_health_op that the kernel fills)."""
    assert codes.ndim == 4 and codes.dtype == (np.uint8 if q8 else np.uint16) and codes.shape[3] == (32 if q8 else 16)
    mag = codes[:, cb0:cb0 + CB].astype(np.uint32) & (0x7F if q8 else 0x7FFF)
    limit, near, first_bad = (E4M3_LIMIT, E4M3_NEAR, E4M3_NAN) if q8 else (F16_LIMIT, F16_NEAR, F16_INF)
    finite = mag < first_bad
    max_code = int(mag[finite].max()) if finite.any() else 0
    return {"elements": int(mag.size), "at_limit": int((mag == limit).sum()), "near_limit": int(((mag >= near) & finite).sum()),
            "nonfinite": int((~finite).sum()), "max_abs": (decode_e4m3 if q8 else decode_f16)(max_code), "limit": 448.0 if q8 else 65504.0,
            "q8": 1 if q8 else 0}


# (N, cbt, cb0, CB, P): the smallest shapes at which the kernel's index arithmetic can go wrong
KERNEL_SHAPES = [
    (1, 1, 0, 1, 1),          # two 16-byte loads: less than a wave
    (2, 1, 0, 1, 63),         # P odd, below a wave of loads per image
    (2, 1, 0, 1, 257),        # more than one block, P no multiple of anything
    (2, 5, 2, 2, 63),         # a view inside a wider tensor: the neighbouring blocks hold inf and the limit and must not be counted
    (6, 4, 0, 4, 25600),      # 1 228 800 loads against a grid of 4096 x 256 threads: the grid-stride loop runs
]


def build_tensor(N, cbt, cb0, CB, P, q8, seed):
    """Codes of a benign tensor (|v| well inside the range) with special values planted at the view's first element, its last element
    and the first element of the second image; the blocks outside the view are filled with non-finite values and values at the limit."""
    rng = np.random.default_rng(seed)
    lanes = 32 if q8 else 16
    if q8:
        codes = rng.integers(0, 0x60, size=(N, cbt, P, lanes), dtype=np.uint8) | (rng.integers(0, 2, size=(N, cbt, P, lanes), dtype=np.uint8) << 7)
        pos_limit, neg_limit, bad_a, bad_b, near = 0x7E, 0xFE, 0x7F, 0xFF, 0x79
    else:
        codes = (rng.standard_normal((N, cbt, P, lanes)) * 40.0).astype(np.float16).view(np.uint16).copy()
        pos_limit, neg_limit, bad_a, bad_b, near = 0x7BFF, 0xFBFF, 0xFC00, 0x7E01, 0xF900      # -inf, a NaN with a payload, -40960
    outside = np.ones(cbt, dtype=bool)
    outside[cb0:cb0 + CB] = False
    fill = np.array([bad_a, pos_limit, bad_b, neg_limit], dtype=codes.dtype)
    codes[:, outside] = np.resize(fill, (N, int(outside.sum()), P, lanes))
    codes[0, cb0, 0, 0] = pos_limit                        # the view's first element
    codes[N - 1, cb0 + CB - 1, P - 1, lanes - 1] = bad_a   # ... and its last
    if N > 1:
        codes[1, cb0, 0, 0] = neg_limit                    # the first element of the second image
        codes[1, cb0, P // 2, 3] = near
        codes[1, cb0 + CB - 1, P - 1, 5] = bad_b
    return codes


# one layer scaled in each model test: BatchNorm / GroupNorm affine times this (gain-1 peaks are ~70, so 1e4 is past 4 x 65504)
PLANT_SCALE = 1.0e4
W2L_PLANTED = "face_decoder_blocks.5.0"          # a non-residual layer two thirds into the decoder: gain-1 peak 50
W2L_EARLIER = ("audio_encoder.10", "face_encoder_blocks.3.1", "face_decoder_blocks.4.2")      # taps compared with max_abs

"""Numpy oracle of the OCP MX block-scaled dispatch modes ("mx_fp8_e4m3", "mx_fp8_e5m2", "mx_fp4_e2m1"), the contract of
include/mi_ep.h (reference quantize_functions.h ComputeMaxExp / ComputeScale / ComputeFp8Data / ComputeFp4Data for bf16 input):

  blocks of 32 consecutive elements; e = max of the bf16 exponent fields of the block;
  e == 0xFF -> scale byte 0xFF, elements unspecified;  e == 0 -> scale byte 0, elements +-0;
  else s = max(e - emax, 0), element = x * 2^(127 - s) rounded to nearest even in the format, saturated to +-max, sign of x.

Routing and row order are those of oracle.ep.normal_dispatch (quantisation is per token, so quantise-then-route equals
route-then-quantise).  Test infrastructure only."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import ep as O  # noqa: E402

MODES = ("mx_fp8_e4m3", "mx_fp8_e5m2", "mx_fp4_e2m1")
QM = {"mx_fp8_e4m3": 4, "mx_fp8_e5m2": 5, "mx_fp4_e2m1": 6}          # MI_EP_QUANT_MX*
BLOCK = 32


class Fmt:
    def __init__(self, ebits, mbits, bias, emax, maxval):
        self.ebits, self.mbits, self.bias, self.emax, self.max = ebits, mbits, bias, emax, maxval
        self.emin = 1 - bias                   # exponent of the smallest normal


FORMATS = {
    "mx_fp8_e4m3": Fmt(4, 3, 7, 8, 448.0),
    "mx_fp8_e5m2": Fmt(5, 2, 15, 15, 57344.0),
    "mx_fp4_e2m1": Fmt(2, 1, 1, 2, 6.0),
}


def encode(v: np.ndarray, f: Fmt) -> np.ndarray:
    """Finite float64 values -> codes of format f (uint8, sign in bit ebits + mbits): round to nearest even, saturate to +-max.
    The sign of zero results is that of v."""
    v = np.asarray(v, np.float64)
    sign = np.signbit(v).astype(np.uint8)
    a = np.abs(v)
    # binade of |v|, at least the smallest normal's (subnormals share its quantum)
    _, ex = np.frexp(np.where(a > 0, a, 1.0))
    e = np.maximum(ex - 1, f.emin)
    quantum = np.ldexp(1.0, e - f.mbits)
    r = np.minimum(np.rint(a / quantum) * quantum, f.max)           # np.rint: ties to even
    # value -> code
    _, rex = np.frexp(np.where(r > 0, r, 1.0))
    re_ = rex - 1
    normal = (r > 0) & (re_ >= f.emin)
    expf = np.where(normal, re_ + f.bias, 0)
    mant = np.where(normal, np.rint((r / np.ldexp(1.0, re_) - 1.0) * (1 << f.mbits)),
                    np.rint(r / np.ldexp(1.0, f.emin - f.mbits)))
    code = (expf.astype(np.int64) << f.mbits) | mant.astype(np.int64)
    return (code | (sign.astype(np.int64) << (f.ebits + f.mbits))).astype(np.uint8)


def decode(code: np.ndarray, f: Fmt) -> np.ndarray:
    """codes of format f -> float64 (the formats here have no Inf; E4M3 0x7F / 0xFF is NaN, E5M2 exponent 31 is Inf / NaN)."""
    c = np.asarray(code, np.int64)
    sign = np.where((c >> (f.ebits + f.mbits)) & 1, -1.0, 1.0)
    expf = (c >> f.mbits) & ((1 << f.ebits) - 1)
    mant = c & ((1 << f.mbits) - 1)
    val = np.where(expf == 0, np.ldexp(mant.astype(np.float64), f.emin - f.mbits),
                   np.ldexp(1.0 + mant / (1 << f.mbits), expf - f.bias))
    if f.ebits == 4:
        val = np.where((expf == 15) & (mant == 7), np.nan, val)
    elif f.ebits == 5:
        val = np.where(expf == 31, np.where(mant == 0, np.inf, np.nan), val)
    return sign * val


def bf16_bits_to_f64(bits: np.ndarray) -> np.ndarray:
    return (np.asarray(bits, np.uint16).astype(np.uint32) << 16).view(np.float32).astype(np.float64)


def quant_mx_rows(x_bits: np.ndarray, mode: str):
    """bf16 rows [N, H] (uint16 bits) -> (data uint8 [N, H] (FP8) or [N, H/2] (FP4, element 2i in the low nibble),
    scales uint8 [N, H/32], finite bool [N, H/32]: False for the blocks whose elements are unspecified (scale 0xFF))."""
    f = FORMATS[mode]
    x_bits = np.asarray(x_bits, np.uint16)
    N, H = x_bits.shape
    assert H % BLOCK == 0, H
    nb = H // BLOCK
    blk = x_bits.reshape(N, nb, BLOCK)
    e = ((blk >> 7) & 0xFF).max(axis=2).astype(np.int64)                  # [N, nb]
    s = np.maximum(e - f.emax, 0)
    scales = np.where(e == 0xFF, 0xFF, s).astype(np.uint8)
    finite = e != 0xFF
    x = bf16_bits_to_f64(blk)
    mul = np.where(e == 0, 0.0, np.ldexp(1.0, 127 - np.minimum(s, 254)))[:, :, None]
    v = np.where(finite[:, :, None], x, 0.0) * mul
    # products below 2^-126 would be flushed / rounded to +-0 by every format here: the same as exact arithmetic
    v = np.where(np.abs(v) < 2.0 ** -126, np.copysign(0.0, np.where(finite[:, :, None], x, 0.0)), v)
    codes = encode(v, f).reshape(N, H)
    if f.ebits + f.mbits == 3:                                            # FP4: two codes per byte
        codes = (codes[:, 0::2] & 0xF) | ((codes[:, 1::2] & 0xF) << 4)
    return codes.astype(np.uint8), scales, finite


def dequant_mx_rows(data: np.ndarray, scales: np.ndarray, mode: str) -> np.ndarray:
    """value * 2^(scale - 127) (reference tests/python/deepep/utils.py per_token_cast_back, E8M0 branch), as float32 [N, H];
    scale 0xFF gives NaN."""
    f = FORMATS[mode]
    data = np.asarray(data, np.uint8)
    N = data.shape[0]
    if f.ebits + f.mbits == 3:
        codes = np.empty((N, data.shape[1] * 2), np.uint8)
        codes[:, 0::2] = data & 0xF
        codes[:, 1::2] = data >> 4
    else:
        codes = data
    H = codes.shape[1]
    vals = decode(codes, f).reshape(N, H // BLOCK, BLOCK)
    sc = np.asarray(scales, np.uint8).reshape(N, H // BLOCK).astype(np.int64)
    mul = np.where(sc == 0xFF, np.nan, np.ldexp(1.0, sc - 127))[:, :, None]
    return (vals * mul).reshape(N, H).astype(np.float32)


def calc_diff(x: np.ndarray, y: np.ndarray) -> float:
    """1 - cosine-like similarity of x + 1 and y + 1 (reference tests/python/deepep/utils.py calc_diff)."""
    x = np.asarray(x, np.float64) + 1
    y = np.asarray(y, np.float64) + 1
    return float(1 - 2 * (x * y).sum() / (x * x + y * y).sum())


def mx_dispatch(xs_bits, topk_idxs, num_experts, mode, expert_token_nums_type=1):
    """-> per rank: (DispatchResult of the bf16 exchange (routing, triples, counts), data [R, ...], scales [R, H/32], finite [R, H/32])
    in receive-row order, R = total_recv."""
    res = O.normal_dispatch(xs_bits, topk_idxs, num_experts, False, expert_token_nums_type)
    out = []
    for r in res:
        n = r.total_recv
        d, s, fin = quant_mx_rows(r.recv_x[:n], mode)
        out.append((r, d, s, fin))
    return out


def bf16_round(x_f32: np.ndarray) -> np.ndarray:
    """float32 -> bf16 bits, round to nearest even (the conversion torch's .to(torch.bfloat16) makes)."""
    from oracle.bf16 import f32_to_bf16_bits_rne
    return f32_to_bf16_bits_rne(np.asarray(x_f32, np.float32))

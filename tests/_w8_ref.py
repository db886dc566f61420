"""Plain torch restatement of the FP8 decode-weight quantiser (csrc/decode_w8.hip, include/afk.h afk_quantize_rows_fp8); CPU or device tensors.

Format: OCP e4m3fn (max finite 448, no infinities), one power-of-two scale per row.  With a = max |w| of the row = m * 2^x, m in [0.5, 1) (torch.frexp):
    scale = 2^e,  e = x - 9 where m <= 0.875, else x - 8     the smallest power of two with a / 2^e <= 448 (= 0.875 * 2^9)
    e >= -117 (rows of subnormal weights only: the smallest code times the scale stays a normal bf16);  a == 0: scale 1
    code = RNE(w / 2^e) to e4m3fn, by torch's own cast; clamped to +-448 in front of it because torch's cast turns overflow into NaN (by construction the
    clamp never moves a value)
code * scale is exactly representable in bf16 (3 mantissa bits, an exponent inside bf16's range)."""
import torch

FP8_MAX = 448.0
E_MIN = -117


def row_exponent(w):
    """e [N] (int32) of every row of w [N, K]"""
    a = w.float().abs().amax(dim=1)
    m, x = torch.frexp(a)
    e = torch.where(m <= 0.875, x - 9, x - 8).clamp_min(E_MIN)
    return torch.where(a == 0, torch.zeros_like(e), e).to(torch.int32)


def quantize(w):
    """w [N, K] (bf16, finite) -> (codes uint8 [N, K], scale fp32 [N])"""
    if not bool(torch.isfinite(w.float()).all()):
        raise ValueError("quantize: NaN or infinite weight")
    e = row_exponent(w)
    v = torch.ldexp(w.float(), -e[:, None])   # exact: a power of two
    codes = v.clamp(-FP8_MAX, FP8_MAX).to(torch.float8_e4m3fn).view(torch.uint8)
    return codes, torch.ldexp(torch.ones_like(e, dtype=torch.float32), e)


def dequantize(codes, scale, dtype=torch.bfloat16):
    """codes uint8 [N, K], scale fp32 [N] -> the weights they stand for, in fp32 arithmetic, as `dtype`"""
    return (codes.view(torch.float8_e4m3fn).float() * scale[:, None].float()).to(dtype)


def snap(w):
    """w onto the FP8 grid of its rows: dequantize(quantize(w)) in w's dtype - a weight the FP8 copy restates without loss"""
    return dequantize(*quantize(w), dtype=w.dtype)

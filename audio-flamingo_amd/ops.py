"""Tensor-level wrappers over the C ABI (include/afk.h).

PyTorch is used only as plumbing here: device memory (caching allocator), the current HIP stream, tensor
metadata.  Every function enqueues hand-written gfx950 kernels on ``torch.cuda.current_stream()``.
No function has a CPU / eager fallback: inputs must live on a HIP device (AfkError otherwise).
"""
from __future__ import annotations

import os

import torch

from . import _lib
from ._lib import AfkError

BF16 = torch.bfloat16

GEMM_BIAS, GEMM_GELU, GEMM_RESIDUAL, GEMM_OUT_F32, GEMM_ACCUM, GEMM_SWIGLU_BWD, GEMM_SWIGLU_FWD = 1, 2, 4, 8, 16, 32, 64


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _p(t):
    return 0 if t is None else t.data_ptr()


def _chk(t: torch.Tensor, dtype=None, name="tensor"):
    if not t.is_cuda:
        raise AfkError(f"{name}: expected a HIP device tensor, got {t.device} (no CPU fallback in this package)")
    if dtype is not None and t.dtype != dtype:
        raise AfkError(f"{name}: expected dtype {dtype}, got {t.dtype}")
    return t


def pad64(n: int) -> int:
    return (n + 63) // 64 * 64


# ---------------------------------------------------------------------------------------------- GEMM
GEMM_FUSE_ROPE = os.environ.get("AFK_FUSE_ROPE_FWD", "1") != "0"   # rotary embedding inside the qkv GEMM's epilogue (afk_gemm_nt_bf16_rope, round 6)


def gemm_nt_rope(a, b, bias, cos, sin, *, S, rope_cols, D, pos=None):
    """qkv = a @ b^T + bias with rotate-half RoPE on the first rope_cols columns (heads of D columns): one launch (afk_gemm_nt_bf16_rope) when the shape allows -
    head_dim 128, N and rope_cols multiples of 256, enough tiles for the 256 x 256 kernel - else afk_gemm_nt_bf16 + afk_rope_inplace.  The same bits either way
    (tests/test_ops_gpu.py::test_gemm_rope_epilogue_bit_equal)."""
    M, N, K = a.shape[0], b.shape[0], a.shape[1]
    fused = (GEMM_FUSE_ROPE and D == 128 and N % 256 == 0 and rope_cols % 256 == 0 and K % 64 == 0 and ((M + 255) // 256) * (N // 256) >= 192
             and cos.data_ptr() % 16 == 0 and sin.data_ptr() % 16 == 0 and a.stride(1) == 1 and b.stride(1) == 1)
    if fused:
        _chk(a, BF16, "gemm a"), _chk(b, BF16, "gemm b"), _chk(cos, BF16, "rope cos"), _chk(sin, BF16, "rope sin")
        out = torch.empty((M, N), device=a.device, dtype=BF16)
        lanes = pos is None and S % 32 == 0 and cos.shape[0] >= S and sin.shape[0] >= S   # positions = row % S and no 32-row block straddles two samples
        cl, sl = (_rope_lanes(cos, S, D, 1), _rope_lanes(sin, S, D, 1)) if lanes else (None, None)
        _lib.call("afk_gemm_nt_bf16_rope", a.data_ptr(), a.stride(0), b.data_ptr(), b.stride(0), out.data_ptr(), out.stride(0), M, N, K,
                  _p(bias), cos.data_ptr(), sin.data_ptr(), _p(pos), S, rope_cols, _p(cl), _p(sl), _stream())
        return out
    out = gemm_nt(a, b, bias=bias)
    rope_(out, cos, sin, S=S, nheads=rope_cols // D, D=D, pos=pos)
    return out


def gemm_nt(a, b, out=None, *, bias=None, residual=None, res_mod=0, gelu=False, preact_out=None, out_f32=False,
            accumulate=False, alpha=1.0, M=None, N=None, K=None, swiglu_bwd=None, swiglu_fwd_out=None):
    """out[M,N] = epi(alpha * a[M,K] @ b[N,K]^T).  a, b: 2-D bf16 with unit inner stride (row stride free).
    swiglu_fwd_out: b is the fused gate|up weight [2I, K]; out [M, 2I] = gate|up as usual and swiglu_fwd_out [M, I] (contiguous) receives
    bf16(bf16(silu(gate)) * up) from the same launch (AFK_GEMM_SWIGLU_FWD; I % 128 == 0)"""
    _chk(a, BF16, "gemm a"), _chk(b, BF16, "gemm b")
    assert a.dim() == 2 and b.dim() == 2 and a.stride(1) == 1 and b.stride(1) == 1
    M = a.shape[0] if M is None else M
    N = b.shape[0] if N is None else N
    K = a.shape[1] if K is None else K
    assert K <= a.shape[1] and K <= b.shape[1]
    if swiglu_fwd_out is not None:
        assert bias is None and residual is None and not gelu and not accumulate and not out_f32 and preact_out is None and swiglu_bwd is None
        _chk(swiglu_fwd_out, BF16, "gemm swiglu_fwd_out")
        assert N % 256 == 0 and swiglu_fwd_out.is_contiguous() and tuple(swiglu_fwd_out.shape) == (M, N // 2)
        if out is None:
            out = torch.empty((M, N), device=a.device, dtype=BF16)
        _lib.call("afk_gemm_nt_bf16", a.data_ptr(), a.stride(0), b.data_ptr(), b.stride(0), out.data_ptr(), out.stride(0), M, N, K, 0, 0, 0, 0,
                  swiglu_fwd_out.data_ptr(), float(alpha), GEMM_SWIGLU_FWD, _stream())
        return out
    if swiglu_bwd is not None:
        # fused SwiGLU backward epilogue: out [M, 2N] = (dgate | dup), swiglu_bwd = saved gate|up [M, 2N]
        assert bias is None and residual is None and not gelu and not accumulate and not out_f32 and swiglu_bwd.shape[1] == 2 * N
        _chk(swiglu_bwd, BF16, "gemm swiglu_bwd")
        if out is None:
            out = torch.empty((M, 2 * N), device=a.device, dtype=BF16)
        _lib.call("afk_gemm_nt_bf16", a.data_ptr(), a.stride(0), b.data_ptr(), b.stride(0), out.data_ptr(), out.stride(0), M, N, K, 0,
                  swiglu_bwd.data_ptr(), swiglu_bwd.stride(0), 0, 0, float(alpha), GEMM_SWIGLU_BWD, _stream())
        return out
    if out is None:
        out = torch.empty((M, N), device=a.device, dtype=torch.float32 if out_f32 else BF16)
    assert out.dim() == 2 and out.stride(1) == 1 and out.shape[0] >= M and out.shape[1] >= N
    flags = 0
    if bias is not None:
        flags |= GEMM_BIAS
        _chk(bias, BF16, "gemm bias")
    if gelu:
        flags |= GEMM_GELU
    if residual is not None:
        flags |= GEMM_RESIDUAL
        _chk(residual, BF16, "gemm residual")
        assert residual.stride(-1) == 1
    if out.dtype == torch.float32:
        flags |= GEMM_OUT_F32
    if accumulate:
        flags |= GEMM_ACCUM
    if preact_out is not None:
        assert preact_out.stride(0) == out.stride(0) and preact_out.dtype == BF16
    splits = splitk_plan(M, N, K)
    if splits > 1 or M <= GEMV_MAX_M:
        ws = torch.empty(splits * M * N, device=a.device, dtype=torch.float32)
        _lib.call("afk_gemm_nt_bf16_splitk", a.data_ptr(), a.stride(0), b.data_ptr(), b.stride(0), out.data_ptr(), out.stride(0),
                  M, N, K, _p(bias), _p(residual), residual.stride(0) if residual is not None else 0, res_mod,
                  _p(preact_out), float(alpha), flags, splits, ws.data_ptr(), _stream())
        return out
    _lib.call("afk_gemm_nt_bf16", a.data_ptr(), a.stride(0), b.data_ptr(), b.stride(0), out.data_ptr(), out.stride(0),
              M, N, K, _p(bias), _p(residual), residual.stride(0) if residual is not None else 0, res_mod,
              _p(preact_out), float(alpha), flags, _stream())
    return out


GEMV_MAX_M = 1  # AFK_GEMV_MAX_M in csrc/gemm.hip
if os.environ.get("AFK_GEMM_NARROW") == "1":  # A/B knob: 8-byte GEMM epilogue
    _lib.call("afk_gemm_set_variant", 16)
SPLITK = os.environ.get("AFK_SPLITK", "1") != "0"


def splitk_plan(M, N, K):
    """number of K splits for an NT GEMM: > 1 only when the output has too few 128x128 tiles to fill the chip (2 x 256 workgroup
    slots) and the reduction is long enough to share - decode-time Linears (M = batch) and weight gradients of narrow layers"""
    if M <= GEMV_MAX_M and SPLITK:  # decode: weight-streaming kernel (csrc/gemm.hip gemv_nt_bf16_kernel), 32 weight rows per workgroup
        blocks = (N + 31) // 32
        return max(1, min(16, (K + 511) // 512, (1536 + blocks - 1) // blocks))
    if not SPLITK or K < 1024:
        return 1
    t256 = ((M + 255) // 256) * ((N + 255) // 256)
    t128 = ((M + 127) // 128) * ((N + 127) // 128)
    if t256 >= 192 or t128 > 300:
        return 1
    return max(1, min(16, K // 256, (512 + t128 - 1) // t128))


def gemm(a, b, out=None, *, trans_a=False, trans_b=False, bias=None, residual=None, res_mod=0, gelu=False, preact_out=None,
         accumulate=False, alpha=1.0, _splits=None):
    """General form of the MFMA GEMM (C ABI afk_gemm_bf16).
        NT: a [M,K],  b [N,K]            (forward)
        NN: a [M,K],  b [K,N]  trans_b   (dgrad: dX = dY . W)
        TN: a [K,M],  b [K,N]  both      (wgrad: dW = dY^T . X; reduction length K free)"""
    _chk(a, BF16, "gemm a"), _chk(b, BF16, "gemm b")
    assert a.dim() == 2 and b.dim() == 2 and a.stride(1) == 1 and b.stride(1) == 1
    if trans_a:
        K, M = a.shape
    else:
        M, K = a.shape
    if trans_b:
        Kb, N = b.shape
    else:
        N, Kb = b.shape
    assert K == Kb, (a.shape, b.shape, trans_a, trans_b)
    if out is None:
        out = torch.empty((M, N), device=a.device, dtype=BF16)
    assert out.dim() == 2 and out.stride(1) == 1 and out.shape[0] >= M and out.shape[1] >= N
    flags = 0
    if bias is not None:
        flags |= GEMM_BIAS
    if gelu:
        flags |= GEMM_GELU
    if residual is not None:
        flags |= GEMM_RESIDUAL
    if out.dtype == torch.float32:
        flags |= GEMM_OUT_F32
    if accumulate:
        flags |= GEMM_ACCUM
    if _splits is None and trans_a and trans_b and PEEL_TAIL and bias is None and residual is None and not gelu and preact_out is None:
        plan = peel_plan_256(M, N, K)
        if plan is not None:
            # wave quantisation: T = 8.09 (gate|up wgrad) or 4.05 (down wgrad) rounds of 256 tiles pay for a nearly empty last round.  Peel
            # the last tile rows (or columns) off: the main launch fills whole rounds, the strip runs split-K in one short round.
            axis, cut, s = plan
            kw = dict(trans_a=True, trans_b=True, accumulate=accumulate, alpha=alpha)
            if axis == 0:
                gemm(a[:, :cut], b, out[:cut], _splits=1, **kw)
                gemm(a[:, cut:M], b, out[cut:M], _splits=s, **kw)
            else:
                gemm(a, b[:, :cut], out[:, :cut], _splits=1, **kw)
                gemm(a, b[:, cut:N], out[:, cut:N], _splits=s, **kw)
            return out
    splits = _splits if _splits is not None else (splitk_plan_256(M, N, K) if trans_b else 1)
    if splits > 1:
        ws = torch.empty(splits * M * N, device=a.device, dtype=torch.float32)
        _lib.call("afk_gemm_bf16_splitk", int(trans_a), int(trans_b), a.data_ptr(), a.stride(0), b.data_ptr(), b.stride(0), out.data_ptr(),
                  out.stride(0), M, N, K, _p(bias), _p(residual), residual.stride(0) if residual is not None else 0, res_mod,
                  _p(preact_out), float(alpha), flags, splits, ws.data_ptr(), _stream())
        return out
    _lib.call("afk_gemm_bf16", int(trans_a), int(trans_b), a.data_ptr(), a.stride(0), b.data_ptr(), b.stride(0), out.data_ptr(),
              out.stride(0), M, N, K, _p(bias), _p(residual), residual.stride(0) if residual is not None else 0, res_mod,
              _p(preact_out), float(alpha), flags, _stream())
    return out


SPLITK_ROUND = int(os.environ.get("AFK_SPLITK_ROUND", "256"))
# Off by default - measured on the full step (same box, 2 runs each): the serial GEMM time falls 314.7 -> 309.8 ms/step (gate|up and down
# weight gradients lose their nearly empty ninth / fifth round), but the default three-stream schedule gets SLOWER, 431.4 -> 433.7 / 437.1 ms:
# its second stream was already filling those tails, and the strip adds two launches and a 60 MB fp32 workspace per weight gradient.
PEEL_TAIL = os.environ.get("AFK_PEEL_TAIL", "0") == "1"


def peel_plan_256(M, N, K):
    """TN GEMM whose 256x256 tiles end in a nearly empty round of 256 workgroups: -> (axis, cut, splits) = run rows (axis 0) / columns
    (axis 1) [0, cut) as the main launch (whole rounds) and the remaining strip with `splits` K-splits in one short round; None = leave it.
    Cost model in rounds: ceil(main tiles / 256) + 1 / splits + 0.08 (second launch + fold) against ceil(tiles / 256)."""
    tm, tn = (M + 255) // 256, (N + 255) // 256
    T = tm * tn
    if T <= 256 or K < 2048:
        return None
    base = (T + 255) // 256
    best = None
    for axis, (t_long, t_other) in enumerate(((tm, tn), (tn, tm))):
        for r in range(1, 9):
            t_tail = r * t_other
            t_main = T - t_tail
            if r >= t_long or t_tail > 128:
                break
            sp = min(16, (K // 64) // 8, SPLITK_ROUND // t_tail)
            if sp < 2:
                continue
            cost = (t_main + 255) // 256 + 1.0 / sp + 0.08
            if cost < base - 0.3 and (best is None or cost < best[0]):
                best = (cost, axis, (t_long - r) * 256, sp)
    return None if best is None else best[1:]


def splitk_plan_256(M, N, K):
    """K splits for the 256x256 transposed-operand kernels (one workgroup per CU): only for outputs with < 128 tiles and K >= 2048"""
    if not SPLITK or K < 2048:
        return 1
    t256 = ((M + 255) // 256) * ((N + 255) // 256)
    if t256 >= 128:
        return 1
    # as many splits as still fit ONE round of 256 workgroups (one per CU): ceil() here gave 275-300 workgroups for the encoder's weight
    # gradients - a second round for 19-44 of them, 55-59 % of the CUs over the launch
    return max(1, min(16, K // 512, SPLITK_ROUND // t256))


COLSUM_FUSED = os.environ.get("AFK_COLSUM_FUSED", "1") == "1"   # one launch (the last row slice folds); 0: partial + fold launches (rounds 1-3)
_COLSUM_COUNTERS = {}


def _colsum_counters(dev, n):
    """arrival counters of afk_colsum_bf16_fused: zero before the first launch, left at zero by every launch; one array per (device, stream) because
    launches on different streams may overlap in time"""
    key = (dev.index, torch.cuda.current_stream(dev).cuda_stream)
    t = _COLSUM_COUNTERS.get(key)
    if t is None or t.numel() < n:
        t = _COLSUM_COUNTERS[key] = torch.zeros(max(n, 4096), device=dev, dtype=torch.int32)
    return t


def colsum(x, out, *, accumulate=False):
    """out[c] (+)= sum_r x[r][c]   (bias gradient)"""
    rows, cols = x.shape
    ns = _lib.load().afk_colsum_slices(rows)
    ws = torch.empty(ns * cols, device=x.device, dtype=torch.float32)
    if COLSUM_FUSED:
        cnt = _colsum_counters(x.device, (cols + 63) // 64)
        _lib.call("afk_colsum_bf16_fused", x.data_ptr(), x.stride(0), rows, cols, out.data_ptr(), int(accumulate), ws.data_ptr(), cnt.data_ptr(), _stream())
    else:
        _lib.call("afk_colsum_bf16", x.data_ptr(), x.stride(0), rows, cols, out.data_ptr(), int(accumulate), ws.data_ptr(), _stream())
    return out


THIN_BLOCKS = 0  # > 0: cap transposes to that many persistent blocks (set while enqueueing on a side stream beside GEMMs)


def transpose(x, out=None, *, rpad=None):
    """x [R, C] (row stride free) -> out [C, Rpad] with zero-filled tail columns."""
    _chk(x, BF16, "transpose x")
    assert x.dim() == 2 and x.stride(1) == 1
    R, C = x.shape
    rpad = pad64(R) if rpad is None else rpad
    if out is None:
        out = torch.empty((C, rpad), device=x.device, dtype=BF16)
    _lib.call("afk_transpose_bf16", x.data_ptr(), out.data_ptr(), R, C, rpad, x.stride(0), out.stride(0), 1, 1, 0, 0, 0, 0,
              THIN_BLOCKS, _stream())
    return out


def transpose_heads(x, B, S, H, D, ld, spad, out=None):
    """x addressed [b][s][h][d] = base + (b*S+s)*ld + h*D + d  ->  out [B, H, D, spad] (zero padded)."""
    _chk(x, BF16, "transpose_heads x")
    if out is None:
        out = torch.empty((B, H, D, spad), device=x.device, dtype=BF16)
    _lib.call("afk_transpose_bf16", x.data_ptr(), out.data_ptr(), S, D, spad, ld, spad, B, H, S * ld, D, H * D * spad,
              D * spad, 0, _stream())
    return out


# ---------------------------------------------------------------------------------------------- norms
def _dense(*named):
    """the norm kernels address row r at base + r * D: a strided view would be read (and empty_like of it written) as if it were dense"""
    for name, t in named:
        assert t is None or t.is_contiguous(), f"{name} must be contiguous (got strides {tuple(t.stride())} for shape {tuple(t.shape)})"


def layernorm_fwd(x, w, b, eps=1e-5):
    _dense(("layernorm x", x))
    _chk(x, BF16, "layernorm x")
    D = x.shape[-1]
    rows = x.numel() // D
    y = torch.empty_like(x)
    mean = torch.empty(rows, device=x.device, dtype=torch.float32)
    rstd = torch.empty(rows, device=x.device, dtype=torch.float32)
    _lib.call("afk_layernorm_fwd", x.data_ptr(), w.data_ptr(), b.data_ptr(), y.data_ptr(), mean.data_ptr(), rstd.data_ptr(),
              rows, D, float(eps), _stream())
    return y, mean, rstd


def _norm_ws(rows, D, device):
    nb = _lib.load().afk_norm_bwd_blocks(rows)
    return torch.empty(nb * 2 * D, device=device, dtype=torch.float32)


def layernorm_bwd(x, w, dy, mean, rstd, dw, db, *, dx_add=None, accumulate=False, colsum_out=None, colsum_accumulate=False):
    """colsum_out (with dx_add, D % 8 == 0): also colsum_out[c] (+)= sum_r dx[r][c] - the bias gradient of the Linear whose output this norm normalised"""
    _dense(("layernorm_bwd x", x), ("layernorm_bwd dy", dy), ("layernorm_bwd dx_add", dx_add))
    D = x.shape[-1]
    rows = x.numel() // D
    dx = torch.empty_like(x)
    if colsum_out is not None:
        assert dx_add is not None and D % 8 == 0 and D <= 4096
        nb = _lib.load().afk_norm_bwd_blocks(rows)
        ws = torch.empty(nb * 3 * D, device=x.device, dtype=torch.float32)
        _lib.call("afk_layernorm_bwd_colsum", x.data_ptr(), w.data_ptr(), dy.data_ptr(), mean.data_ptr(), rstd.data_ptr(), dx.data_ptr(), dx_add.data_ptr(),
                  dw.data_ptr(), db.data_ptr(), int(accumulate), colsum_out.data_ptr(), int(colsum_accumulate), ws.data_ptr(), rows, D, _stream())
        return dx
    ws = _norm_ws(rows, D, x.device)
    _lib.call("afk_layernorm_bwd", x.data_ptr(), w.data_ptr(), dy.data_ptr(), mean.data_ptr(), rstd.data_ptr(), dx.data_ptr(),
              _p(dx_add), dw.data_ptr(), db.data_ptr(), int(accumulate), ws.data_ptr(), rows, D, _stream())
    return dx


def rmsnorm_fwd(x, w, eps=1e-6):
    _dense(("rmsnorm x", x))
    _chk(x, BF16, "rmsnorm x")
    D = x.shape[-1]
    rows = x.numel() // D
    y = torch.empty_like(x)
    rstd = torch.empty(rows, device=x.device, dtype=torch.float32)
    _lib.call("afk_rmsnorm_fwd", x.data_ptr(), w.data_ptr(), y.data_ptr(), rstd.data_ptr(), rows, D, float(eps), _stream())
    return y, rstd


def rmsnorm_bwd(x, w, dy, rstd, dw, *, dx_add=None, accumulate=False):
    _dense(("rmsnorm_bwd x", x), ("rmsnorm_bwd dy", dy), ("rmsnorm_bwd dx_add", dx_add))
    D = x.shape[-1]
    rows = x.numel() // D
    dx = torch.empty_like(x)
    ws = _norm_ws(rows, D, x.device)
    _lib.call("afk_rmsnorm_bwd", x.data_ptr(), w.data_ptr(), dy.data_ptr(), rstd.data_ptr(), dx.data_ptr(), _p(dx_add),
              dw.data_ptr(), int(accumulate), ws.data_ptr(), rows, D, _stream())
    return dx


# ---------------------------------------------------------------------------------------------- elementwise
def gelu_fwd(x):
    y = torch.empty_like(_chk(x, BF16))
    _lib.call("afk_gelu_fwd", x.data_ptr(), y.data_ptr(), x.numel(), _stream())
    return y


def gelu_bwd(dy, pre, *, colsum_out=None, colsum_accumulate=False):
    """colsum_out: also colsum_out[c] (+)= sum_r dx[r][c] (the bias gradient of the Linear that produced `pre`), by a column-owned form of the same arithmetic"""
    dx = torch.empty_like(_chk(dy, BF16))
    if colsum_out is not None:
        rows, C = dy.shape
        ws = torch.empty(_lib.load().afk_gelu_bwd_colsum_parts(rows) * C, device=dy.device, dtype=torch.float32)
        _lib.call("afk_gelu_bwd_colsum", dy.data_ptr(), pre.data_ptr(), dx.data_ptr(), rows, C, colsum_out.data_ptr(), int(colsum_accumulate), ws.data_ptr(), _stream())
        return dx
    _lib.call("afk_gelu_bwd", dy.data_ptr(), pre.data_ptr(), dx.data_ptr(), dy.numel(), _stream())
    return dx


def silu_mul_fwd(gu):
    rows, I2 = _chk(gu, BF16).shape
    h = torch.empty((rows, I2 // 2), device=gu.device, dtype=BF16)
    _lib.call("afk_silu_mul_fwd", gu.data_ptr(), h.data_ptr(), rows, I2 // 2, _stream())
    return h


def silu_mul_bwd(gu, dh):
    rows, I2 = gu.shape
    dgu = torch.empty_like(gu)
    _lib.call("afk_silu_mul_bwd", gu.data_ptr(), dh.data_ptr(), dgu.data_ptr(), rows, I2 // 2, _stream())
    return dgu


def rope_(buf, cos, sin, *, S, nheads, D, pos=None, backward=False):
    """in-place rotate-half RoPE on the first nheads*D columns of buf [rows, ld]."""
    _chk(buf, BF16, "rope buf")
    rows, ld = buf.shape[0], buf.stride(0)
    _lib.call("afk_rope_inplace", buf.data_ptr(), cos.data_ptr(), sin.data_ptr(), _p(pos), rows, S, ld, nheads, D,
              int(backward), _stream())
    return buf


def rotary_time(x, cos, sin, *, backward=False):
    """Music Flamingo rotary time embedding on encoder rows: x [rows, E] bf16, cos / sin [rows, R] fp32 (R <= E, even)"""
    _chk(x, BF16, "rotary_time x"), _chk(cos, torch.float32, "rotary_time cos"), _chk(sin, torch.float32, "rotary_time sin")
    rows, E = x.shape
    R = cos.shape[-1]
    assert x.is_contiguous() and cos.is_contiguous() and sin.is_contiguous() and cos.numel() == rows * R == sin.numel()
    y = torch.empty_like(x)
    _lib.call("afk_rotary_time", x.data_ptr(), cos.data_ptr(), sin.data_ptr(), y.data_ptr(), rows, E, R, int(backward), _stream())
    return y


def add(a, b, out=None):
    out = torch.empty_like(a) if out is None else out
    _lib.call("afk_add_bf16", a.data_ptr(), b.data_ptr(), out.data_ptr(), a.numel(), _stream())
    return out


def scale_add_(x, y, scale_dev, *, accumulate=False):
    """y = (accumulate ? y : 0) + scale_dev[0] * x  (scale on the device)"""
    _lib.call("afk_scale_add_bf16", x.data_ptr(), y.data_ptr(), x.numel(), _chk(scale_dev, torch.float32).data_ptr(),
              int(accumulate), _stream())
    return y


def cast_f32_bf16(x):
    out = torch.empty(x.shape, device=x.device, dtype=BF16)
    _lib.call("afk_cast_f32_bf16", _chk(x, torch.float32).data_ptr(), out.data_ptr(), x.numel(), _stream())
    return out


def rowsum(xt, C, out, *, accumulate=False):
    """out[r] (+)= sum_{c<C} xt[r][c]"""
    _lib.call("afk_rowsum_bf16", xt.data_ptr(), xt.stride(0), C, out.data_ptr(), xt.shape[0], int(accumulate), _stream())
    return out


# ---------------------------------------------------------------------------------------------- conv stem helpers
def im2col_conv1(x):
    """x [W, C, T] (f32 or bf16, channel-major) -> col [W*T, 3*C] bf16"""
    W, C, T = x.shape
    assert x.is_contiguous() and x.is_cuda
    col = torch.empty((W * T, 3 * C), device=x.device, dtype=BF16)
    _lib.call("afk_im2col_conv1", x.data_ptr(), int(x.dtype == torch.float32), col.data_ptr(), W, C, T, _stream())
    return col


def im2col_conv2(h, W, Tin, C):
    Tout = (Tin - 1) // 2 + 1
    col = torch.empty((W * Tout, 3 * C), device=h.device, dtype=BF16)
    _lib.call("afk_im2col_conv2", h.data_ptr(), col.data_ptr(), W, Tin, Tout, C, _stream())
    return col


def col2im_conv2(dcol, W, Tin, C):
    Tout = (Tin - 1) // 2 + 1
    dh = torch.empty((W * Tin, C), device=dcol.device, dtype=BF16)
    _lib.call("afk_col2im_conv2", dcol.data_ptr(), dh.data_ptr(), W, Tin, Tout, C, _stream())
    return dh


def conv_weight_to_gemm(w, out=None):
    """[Co, Ci, 3] -> [Co, 3*Ci] (tap-major)"""
    Co, Ci, _ = w.shape
    out = torch.empty((Co, 3 * Ci), device=w.device, dtype=BF16) if out is None else out
    _lib.call("afk_conv_weight_permute", w.data_ptr(), out.data_ptr(), Co, Ci, 0, 0, _stream())
    return out


def conv_weight_grad_from_gemm(dwp, dw, *, accumulate=False):
    Co, Ci, _ = dw.shape
    _lib.call("afk_conv_weight_permute", dwp.data_ptr(), dw.data_ptr(), Co, Ci, 1, int(accumulate), _stream())
    return dw


def avgpool2_fwd(x, out_rows, C):
    y = torch.empty((out_rows, C), device=x.device, dtype=BF16)
    _lib.call("afk_avgpool2_fwd", x.data_ptr(), y.data_ptr(), out_rows, C, _stream())
    return y


def avgpool2_bwd(dy, out_rows, C):
    dx = torch.empty((out_rows * 2, C), device=dy.device, dtype=BF16)
    _lib.call("afk_avgpool2_bwd", dy.data_ptr(), dx.data_ptr(), out_rows, C, _stream())
    return dx


# ---------------------------------------------------------------------------------------------- embedding
def placeholder_scan(ids, audio_id):
    ids = _chk(ids.contiguous(), torch.int64, "input_ids")
    n = ids.numel()
    src = torch.empty(n, device=ids.device, dtype=torch.int32)
    cnt = torch.empty(1, device=ids.device, dtype=torch.int32)
    _lib.call("afk_placeholder_scan", ids.data_ptr(), n, int(audio_id), src.data_ptr(), cnt.data_ptr(), _stream())
    return src, cnt


def embed_scatter_fwd(ids, src, embed, audio):
    n, H = ids.numel(), embed.shape[1]
    out = torch.empty((n, H), device=embed.device, dtype=BF16)
    _lib.call("afk_embed_scatter_fwd", ids.data_ptr(), _p(src), embed.data_ptr(), _p(audio), out.data_ptr(), n, H, _stream())
    return out


def embed_scatter_bwd(ids, src, dout, d_embed, d_audio, perm=None):
    """perm: int32 row indices sorted stably by token id (index plumbing: torch.sort) - built here when d_embed is wanted"""
    n, H = ids.numel(), dout.shape[-1]
    if d_embed is not None and perm is None:
        perm = torch.sort(ids.reshape(-1), stable=True).indices.to(torch.int32)
    _lib.call("afk_embed_scatter_bwd", ids.data_ptr(), _p(src), dout.data_ptr(), _p(d_embed), _p(d_audio), _p(perm), n, H, _stream())


# ---------------------------------------------------------------------------------------------- attention
def _row_stat_buffer(B, H, S, spad, device, kernel_writes_tail=True):
    """fp32 [B, H, spad] per-query statistic (lse, delta) of the LDS-staged attention kernels.  The kernels write every query < S, and the
    padding tail [S, spad) of a ragged last tile must read as zero: afk_attn2_fwd (lse) and afk_attn2_bwd_fused (delta) write that tail
    themselves since round 4 - no fill launch at all (the encoder's S = 1500 paid two ATen fills per attention call: 64 of the ~96 per step);
    only the separate delta pass (afk_attn2_delta) leaves it to the host."""
    t = torch.empty((B, H, spad), device=device, dtype=torch.float32)
    if spad > S and not kernel_writes_tail:
        t[:, :, S:].zero_()
    return t


ATTN_PERSIST = os.environ.get("AFK_ATTN_PERSIST", "0") == "1"   # forward on resident blocks + work queue (afk_attn2_fwd_persistent); restrictions in include/afk.h
_ATTN_QUEUES = {}


def _attn_queue(dev):
    """work-queue words of afk_attn2_fwd_persistent: zero before the first launch, left at zero by every launch; one pair per (device, stream)"""
    key = (dev.index, torch.cuda.current_stream(dev).cuda_stream)
    t = _ATTN_QUEUES.get(key)
    if t is None:
        t = _ATTN_QUEUES[key] = torch.zeros(2, device=dev, dtype=torch.int32)
    return t


ATTN_FUSE_DELTA = os.environ.get("AFK_ATTN_FUSE_DELTA", "1") == "1"   # afk_attn2_bwd_fused (delta inside the dQ kernel) vs delta pass + afk_attn2_bwd
ATTN_IMPL = "lds"  # "lds" = attention_lds.hip (head_dim 64/128), "direct" = attention.hip (also head_dim 32; A/B reference)


def _use_lds(D):
    return ATTN_IMPL == "lds" and D in (64, 128)


def attn_fwd(qkv, B, S, Hq, Hkv, D, *, scale, causal, kv_len=None, kv_lo=None):
    """qkv [B*S, (Hq+2Hkv)*D] fused projection output (q | k | v).  -> o [B*S, Hq*D], lse [B,Hq,Spad]
    kv_len / kv_lo: int32 [B], sample b exposes keys [kv_lo[b], kv_len[b]) (right / left padding; kv_lo needs causal and head_dim 64 / 128)"""
    if kv_lo is not None and not (_use_lds(D) and causal):
        raise _lib.AfkError("attn_fwd: kv_lo (left padding) runs on the LDS-staged causal kernels only; use attn_interval_fwd")
    _chk(qkv, BF16, "qkv")
    ld = qkv.stride(0)
    spad = pad64(S)
    q = qkv
    k = qkv[:, Hq * D:]
    v = qkv[:, (Hq + Hkv) * D:]
    o = torch.empty((B * S, Hq * D), device=qkv.device, dtype=BF16)
    if _use_lds(D):
        lse = _row_stat_buffer(B, Hq, S, spad, qkv.device)
        if ATTN_PERSIST and kv_len is None and kv_lo is None and S % 128 == 0:
            _lib.call("afk_attn2_fwd_persistent", q.data_ptr(), S * ld, D, ld, k.data_ptr(), S * ld, D, ld, v.data_ptr(), S * ld, D, ld,
                      o.data_ptr(), S * Hq * D, D, Hq * D, lse.data_ptr(), None, None, B, Hq, Hkv, S, spad, D, float(scale),
                      int(causal), _attn_queue(qkv.device).data_ptr(), _stream())
            return o, lse
        _lib.call("afk_attn2_fwd", q.data_ptr(), S * ld, D, ld, k.data_ptr(), S * ld, D, ld, v.data_ptr(), S * ld, D, ld,
                  o.data_ptr(), S * Hq * D, D, Hq * D, lse.data_ptr(), _p(kv_len), _p(kv_lo), B, Hq, Hkv, S, spad, D, float(scale),
                  int(causal), _stream())
        return o, lse
    vt = transpose_heads(v, B, S, Hkv, D, ld, spad)
    lse = torch.empty((B, Hq, S), device=qkv.device, dtype=torch.float32)
    _lib.call("afk_attn_fwd", q.data_ptr(), S * ld, D, ld, k.data_ptr(), S * ld, D, ld, vt.data_ptr(), o.data_ptr(),
              S * Hq * D, D, Hq * D, lse.data_ptr(), _p(kv_len), B, Hq, Hkv, S, spad, D, float(scale), int(causal), _stream())
    return o, lse


ATTN_FUSE_ROPE_BWD = os.environ.get("AFK_FUSE_ROPE_BWD", "1") != "0"   # rotary backward inside the attention backward (afk_attn2_bwd_fused_rope, round 6)


_ROPE_LANES = {}   # (table data_ptr, version, rows, D) -> lane-major copy (afk_rope_lanes_table); a handful of entries (one per table the model caches)


def _rope_lanes(table, S, D, form=0):
    """lane-major copy of a rotary table for the dQ epilogue of afk_attn2_bwd_fused_rope, cached per table tensor (weakly: a new tensor at the same address gets
    a fresh copy because its version / shape is part of the key and the entry holds a weak reference to the source)"""
    import weakref

    key = (table.data_ptr(), table._version, int(table.shape[0]), D, form)
    hit = _ROPE_LANES.get(key)
    if hit is not None and hit[0]() is table:
        return hit[1]
    rows = int(table.shape[0])
    out = torch.empty(((rows + 31) // 32) * 32 * D, device=table.device, dtype=BF16)
    _lib.call("afk_rope_lanes_table", table.data_ptr(), out.data_ptr(), rows, D, form, _stream())
    if len(_ROPE_LANES) > 64:
        _ROPE_LANES.clear()
    _ROPE_LANES[key] = (weakref.ref(table), out)
    return out


def _attn_bwd_impl(qkv, o, do, lse, B, S, Hq, Hkv, D, *, scale, causal, kv_len=None, kv_lo=None, rope=None):
    """-> (dqkv, rotated): rotated = the rotary backward has been applied inside the kernels"""
    if kv_lo is not None and not (_use_lds(D) and causal and lse.shape[-1] == pad64(S)):
        raise _lib.AfkError("attn_bwd: kv_lo (left padding) runs on the LDS-staged causal kernels only; use attn_interval_bwd")
    ld = qkv.stride(0)
    spad = pad64(S)
    q = qkv
    k = qkv[:, Hq * D:]
    v = qkv[:, (Hq + Hkv) * D:]
    dev = qkv.device
    ldo = Hq * D
    dqkv = torch.empty_like(qkv)
    ldd = dqkv.stride(0)
    dq = dqkv
    dk = dqkv[:, Hq * D:]
    dv = dqkv[:, (Hq + Hkv) * D:]
    if _use_lds(D) and lse.shape[-1] == spad:
        delta = _row_stat_buffer(B, Hq, S, spad, dev, kernel_writes_tail=ATTN_FUSE_DELTA)
        scratch = torch.empty((2, B * S, Hq * D), device=dev, dtype=BF16) if Hq != Hkv else None
        if ATTN_FUSE_DELTA and rope is not None and ATTN_FUSE_ROPE_BWD and rope[0].data_ptr() % 16 == 0 and rope[1].data_ptr() % 16 == 0:
            cos, sin, pos = rope
            _chk(cos, BF16, "rope cos"), _chk(sin, BF16, "rope sin")
            cl, sl = _rope_lanes(cos, S, D) if pos is None and cos.shape[0] >= S else None, _rope_lanes(sin, S, D) if pos is None and sin.shape[0] >= S else None
            _lib.call("afk_attn2_bwd_fused_rope", q.data_ptr(), S * ld, D, ld, k.data_ptr(), S * ld, D, ld, v.data_ptr(), S * ld, D, ld,
                      o.data_ptr(), S * ldo, D, ldo, do.data_ptr(), S * ldo, D, ldo, lse.data_ptr(), delta.data_ptr(), dq.data_ptr(), S * ldd, D, ldd,
                      dk.data_ptr(), S * ldd, D, ldd, dv.data_ptr(), S * ldd, D, ldd, _p(kv_len), _p(kv_lo), B, Hq, Hkv, S, spad, D,
                      float(scale), int(causal), _p(scratch), cos.data_ptr(), sin.data_ptr(), _p(pos), _p(cl), _p(sl), _stream())
            return dqkv, True
        if ATTN_FUSE_DELTA:   # delta = rowsum(dO o O) inside the dQ kernel, which runs ahead of the dK/dV sweep: one pass over O and dO less
            _lib.call("afk_attn2_bwd_fused", q.data_ptr(), S * ld, D, ld, k.data_ptr(), S * ld, D, ld, v.data_ptr(), S * ld, D, ld,
                      o.data_ptr(), S * ldo, D, ldo, do.data_ptr(), S * ldo, D, ldo, lse.data_ptr(), delta.data_ptr(), dq.data_ptr(), S * ldd, D, ldd,
                      dk.data_ptr(), S * ldd, D, ldd, dv.data_ptr(), S * ldd, D, ldd, _p(kv_len), _p(kv_lo), B, Hq, Hkv, S, spad, D,
                      float(scale), int(causal), _p(scratch), _stream())
            return dqkv, False
        _lib.call("afk_attn2_delta", o.data_ptr(), S * ldo, D, ldo, do.data_ptr(), S * ldo, D, ldo, delta.data_ptr(), B, Hq, S,
                  spad, D, _stream())
        _lib.call("afk_attn2_bwd", q.data_ptr(), S * ld, D, ld, k.data_ptr(), S * ld, D, ld, v.data_ptr(), S * ld, D, ld,
                  do.data_ptr(), S * ldo, D, ldo, lse.data_ptr(), delta.data_ptr(), dq.data_ptr(), S * ldd, D, ldd,
                  dk.data_ptr(), S * ldd, D, ldd, dv.data_ptr(), S * ldd, D, ldd, _p(kv_len), _p(kv_lo), B, Hq, Hkv, S, spad, D,
                  float(scale), int(causal), _p(scratch), _stream())
        return dqkv, False
    delta = torch.empty((B, Hq, S), device=dev, dtype=torch.float32)
    _lib.call("afk_attn_delta", o.data_ptr(), S * ldo, D, ldo, do.data_ptr(), S * ldo, D, ldo, delta.data_ptr(), B, Hq, S, D,
              _stream())
    qt = transpose_heads(q, B, S, Hq, D, ld, spad)
    kt = transpose_heads(k, B, S, Hkv, D, ld, spad)
    dot = transpose_heads(do, B, S, Hq, D, ldo, spad)
    _lib.call("afk_attn_bwd", q.data_ptr(), S * ld, D, ld, k.data_ptr(), S * ld, D, ld, v.data_ptr(), S * ld, D, ld,
              do.data_ptr(), S * ldo, D, ldo, qt.data_ptr(), kt.data_ptr(), dot.data_ptr(), lse.data_ptr(), delta.data_ptr(),
              dq.data_ptr(), S * ldd, D, ldd, dk.data_ptr(), S * ldd, D, ldd, dv.data_ptr(), S * ldd, D, ldd, _p(kv_len),
              B, Hq, Hkv, S, spad, D, float(scale), int(causal), _stream())
    return dqkv, False


def attn_bwd(qkv, o, do, lse, B, S, Hq, Hkv, D, *, scale, causal, kv_len=None, kv_lo=None, rope=None):
    """-> dqkv [B*S, (Hq+2Hkv)*D].  rope = (cos, sin, pos or None): the gradient of the rotary embedding is applied to the q | k columns as well - inside the
    attention backward kernels where the path allows (afk_attn2_bwd_fused_rope: LDS kernels with the fused delta), by afk_rope_inplace(backward) otherwise:
    the same bits either way (tests/test_ops_gpu.py::test_attention_backward_fused_rope_bit_equal)."""
    dqkv, rotated = _attn_bwd_impl(qkv, o, do, lse, B, S, Hq, Hkv, D, scale=scale, causal=causal, kv_len=kv_len, kv_lo=kv_lo, rope=rope)
    if rope is not None and not rotated:
        rope_(dqkv, rope[0], rope[1], S=S, nheads=Hq + Hkv, D=D, pos=rope[2], backward=True)
    return dqkv


def xattn_fwd(q, k, v, krange, B, Sq, Sk, Hq, Hkv, D, scale):
    """interval attention (afk_xattn_fwd): query row i of sample b sees keys [krange[b,i,0], krange[b,i,1]) (None: all Sk keys; an empty
    interval yields a zero row).  q [B*Sq, >=Hq*D], k / v [B*Sk, >=Hkv*D] row-strided views.  -> o [B*Sq, Hq*D], lse [B, Hq, Sq]"""
    sqp, skp = pad64(Sq), pad64(Sk)
    vt = transpose_heads(v, B, Sk, Hkv, D, v.stride(0), skp)
    o = torch.empty((B * Sq, Hq * D), device=q.device, dtype=BF16)
    lse = torch.empty((B, Hq, Sq), device=q.device, dtype=torch.float32)
    _lib.call("afk_xattn_fwd", q.data_ptr(), Sq * q.stride(0), D, q.stride(0), k.data_ptr(), Sk * k.stride(0), D, k.stride(0),
              vt.data_ptr(), o.data_ptr(), Sq * Hq * D, D, Hq * D, lse.data_ptr(), 0, _p(krange), B, Hq, Hkv, Sq, Sk, sqp, skp, D,
              float(scale), _stream())
    return o, lse


def xattn_bwd(q, k, v, o, do, lse, krange, B, Sq, Sk, Hq, Hkv, D, scale, dq, dk, dv):
    """backward of xattn_fwd; dq [B*Sq, >=Hq*D], dk / dv [B*Sk, >=Hkv*D] are written in place (row-strided views allowed)"""
    dev = q.device
    sqp, skp = pad64(Sq), pad64(Sk)
    ldo = Hq * D
    delta = torch.empty((B, Hq, Sq), device=dev, dtype=torch.float32)
    _lib.call("afk_attn_delta", o.data_ptr(), Sq * ldo, D, ldo, do.data_ptr(), Sq * ldo, D, ldo, delta.data_ptr(), B, Hq, Sq, D, _stream())
    qt = transpose_heads(q, B, Sq, Hq, D, q.stride(0), sqp)
    kt = transpose_heads(k, B, Sk, Hkv, D, k.stride(0), skp)
    dot = transpose_heads(do, B, Sq, Hq, D, ldo, sqp)
    _lib.call("afk_xattn_bwd", q.data_ptr(), Sq * q.stride(0), D, q.stride(0), k.data_ptr(), Sk * k.stride(0), D, k.stride(0),
              v.data_ptr(), Sk * v.stride(0), D, v.stride(0), do.data_ptr(), Sq * ldo, D, ldo, qt.data_ptr(), kt.data_ptr(),
              dot.data_ptr(), lse.data_ptr(), delta.data_ptr(), dq.data_ptr(), Sq * dq.stride(0), D, dq.stride(0),
              dk.data_ptr(), Sk * dk.stride(0), D, dk.stride(0), dv.data_ptr(), Sk * dv.stride(0), D, dv.stride(0), 0, _p(krange),
              B, Hq, Hkv, Sq, Sk, sqp, skp, D, float(scale), _stream())


ATTN_APPEND_MAX_SPLITS = 64      # afk_attn_append refuses more (csrc/attention_append.hip APPEND_MAX_SPLITS)
ATTN_APPEND_GROUPS = (1, 2, 4, 7, 8)
ATTN_APPEND_TARGET_BLOCKS = 256  # one block per CU: where the measured sweep turns (profiles/attn_append.md: 8 tiles x 32, 64 tiles x 4, 768 tiles x 1)
ATTN_APPEND_MIN_CHUNK = 128      # keys: the shortest chunk that still paid for its block and its share of the merge (1 032 keys: 8 splits)
ATTN_APPEND_RULE_SPLITS = 16     # most splits the rule asks for: no measured shape was faster by more than 3 % with more, and few-tile launches lost 60 % at 64


def attn_append_supported(Hq, Hkv, D):
    """the geometries afk_attn_append takes"""
    return D in (64, 128) and Hkv > 0 and Hq % Hkv == 0 and Hq // Hkv in ATTN_APPEND_GROUPS


def attn_append_nsplit(B, Hq, Hkv, n, keys):
    """key splits of afk_attn_append from the shape alone (no device read): the launch has B * Hkv * ceil(n / rows per tile) query tiles; split until
    ATTN_APPEND_TARGET_BLOCKS blocks exist, but never into chunks shorter than ATTN_APPEND_MIN_CHUNK of the `keys` a row can see at most, and never more
    than ATTN_APPEND_RULE_SPLITS (the kernel itself takes up to ATTN_APPEND_MAX_SPLITS).  Always >= 1."""
    tiles = max(1, B * Hkv * -(-max(int(n), 1) // (32 // max(Hq // Hkv, 1))))
    ns = -(-ATTN_APPEND_TARGET_BLOCKS // tiles)
    return max(1, min(ns, max(int(keys), 0) // ATTN_APPEND_MIN_CHUNK, ATTN_APPEND_RULE_SPLITS))


def attn_append_chunks(lo, hi, ns):
    """the key chunks afk_attn_append cuts the hull [lo, hi) of a query tile into: a0 = lo & ~31, chunk = round32(ceil((hi - a0) / ns)), split s = keys
    [max(a0 + s * chunk, lo), min(a0 + (s + 1) * chunk, hi)) -> [(begin, end)], empty splits as (x, x)"""
    if hi <= lo:
        return [(lo, lo)] * ns
    a0 = lo & ~31
    chunk = ((-(-(hi - a0) // ns)) + 31) & ~31
    out = []
    for s in range(ns):
        c0, c1 = a0 + s * chunk, min(a0 + (s + 1) * chunk, hi)
        out.append((max(c0, lo), c1) if c1 > c0 else (hi, hi))
    return out


def attn_append(q, Kc, Vt, krange, B, n, Hq, Hkv, D, scale, nsplit=None, ws=None, out=None):
    """append attention (afk_attn_append): n new query rows per sample against the KV cache, split-KV, two launches.  q [B*n, >= Hq*D] row-strided view
    (post-RoPE), Kc [B, Smax, Hkv*D], Vt [B, Hkv, D, spad] (one layer of the cache), krange [B, n, 2] int32 on the device: row i of sample b sees keys
    [krange[b,i,0], krange[b,i,1]).  nsplit None: attn_append_nsplit over the cache rows.  ws: a float32 workspace of at least
    afk_attn_append_workspace_floats(B, Hq, n, D, nsplit) elements (None: allocated here).  -> o [B*n, Hq*D] bf16"""
    _chk(q, BF16, "q"), _chk(Kc, BF16, "Kc"), _chk(Vt, BF16, "Vt")
    if krange is not None:
        _chk(krange, torch.int32, "krange")
    if q.dim() != 2 or q.shape[0] != B * n or q.shape[1] < Hq * D or q.stride(1) != 1:
        raise AfkError(f"attn_append: q {tuple(q.shape)} strides {q.stride()} is not [B*n = {B * n}, >= Hq*D = {Hq * D}] with unit column stride")
    if tuple(Kc.shape) != (B, Kc.shape[1], Hkv * D) or Kc.stride(2) != 1:
        raise AfkError(f"attn_append: Kc {tuple(Kc.shape)} strides {Kc.stride()} is not [B = {B}, Smax, Hkv*D = {Hkv * D}] with unit column stride")
    Smax, spad = Kc.shape[1], Vt.shape[3]
    if tuple(Vt.shape) != (B, Hkv, D, spad) or Vt.stride()[1:] != (D * spad, spad, 1):
        raise AfkError(f"attn_append: Vt {tuple(Vt.shape)} strides {Vt.stride()} is not [B = {B}, Hkv = {Hkv}, D = {D}, spad] with its heads and features contiguous")
    if krange is not None and (tuple(krange.shape) != (B, n, 2) or not krange.is_contiguous()):
        raise AfkError(f"attn_append: krange {tuple(krange.shape)} is not a contiguous [B = {B}, n = {n}, 2]")
    ns = attn_append_nsplit(B, Hq, Hkv, n, Smax) if nsplit is None else int(nsplit)
    if ws is None:
        ws = torch.empty(int(_lib.load().afk_attn_append_workspace_floats(B, Hq, n, D, max(min(ns, ATTN_APPEND_MAX_SPLITS), 1))), device=q.device, dtype=torch.float32)
    else:
        _chk(ws, torch.float32, "ws")
    if out is None:
        o = torch.empty((B * n, Hq * D), device=q.device, dtype=BF16)
    else:
        o = _chk(out, BF16, "out")
        if tuple(o.shape) != (B * n, Hq * D) or o.stride(1) != 1:
            raise AfkError(f"attn_append: out {tuple(o.shape)} strides {o.stride()} is not [B*n, Hq*D] with unit column stride")
    # the strides are the tensors' own: a cache view with a longer row or sample pitch is read as it lies
    _lib.call("afk_attn_append", q.data_ptr(), n * q.stride(0), D, q.stride(0), Kc.data_ptr(), Kc.stride(0), Kc.stride(1), D, Vt.data_ptr(), Vt.stride(0), spad,
              o.data_ptr(), n * o.stride(0), D, o.stride(0), _p(krange), B, Hq, Hkv, n, D, float(scale), ns, ws.data_ptr(), ws.numel(), _stream())
    return o


ATTN_SHARED_MAX_SPLITS = 64      # afk_attn_decode_shared refuses more (csrc/attention_shared.hip SHARED_MAX_SPLITS)
ATTN_SHARED_MAX_COPIES = 16      # continuations per prompt row (SHARED_MAX_COPIES)
ATTN_SHARED_TARGET_BLOCKS = 256  # one block per CU, attn_append_nsplit's target: the prompt blocks have the append kernel's shape
ATTN_SHARED_MIN_CHUNK = 128      # keys: no prompt chunk shorter than this
ATTN_SHARED_RULE_SPLITS = 16     # most splits the rule asks for


def attn_shared_supported(Hq, Hkv, D, n):
    """the geometries and copy counts afk_attn_decode_shared takes"""
    return attn_append_supported(Hq, Hkv, D) and 1 <= int(n) <= ATTN_SHARED_MAX_COPIES


def attn_shared_nsplit(B0, n, Hq, Hkv, keys):
    """prompt key splits of afk_attn_decode_shared from the shape alone (no device read), modelled on attn_append_nsplit: the launch has B0 * Hkv *
    ceil(n / copies per tile) prompt tiles; split until ATTN_SHARED_TARGET_BLOCKS blocks exist, but never into chunks shorter than ATTN_SHARED_MIN_CHUNK of
    the `keys` prompt positions, and never more than ATTN_SHARED_RULE_SPLITS (the kernel itself takes up to ATTN_SHARED_MAX_SPLITS).  Always >= 1."""
    tiles = max(1, int(B0) * int(Hkv) * -(-max(int(n), 1) // (32 // max(Hq // Hkv, 1))))
    ns = -(-ATTN_SHARED_TARGET_BLOCKS // tiles)
    return max(1, min(ns, max(int(keys), 0) // ATTN_SHARED_MIN_CHUNK, ATTN_SHARED_RULE_SPLITS))


def attn_shared_check(Kp, Vtp, Kt, Vtt, prange, trange, B0, n, Hkv, D):
    """the shape and stride checks of attn_decode_shared on what stays the same from step to step: one layer of the prompt cache and of the tail cache, and
    the two interval tensors (a decode loop checks them once and then calls afk_attn_decode_shared itself)"""
    R = int(B0) * int(n)
    for t_, name in ((Kp, "Kp"), (Vtp, "Vtp"), (Kt, "Kt"), (Vtt, "Vtt")):
        _chk(t_, BF16, name)
    _chk(prange, torch.int32, "prange"), _chk(trange, torch.int32, "trange")
    for K_, V_, rows, kn, vn in ((Kp, Vtp, B0, "Kp", "Vtp"), (Kt, Vtt, R, "Kt", "Vtt")):
        if K_.dim() != 3 or tuple(K_.shape) != (rows, K_.shape[1], Hkv * D) or K_.stride(2) != 1:
            raise AfkError(f"attn_decode_shared: {kn} {tuple(K_.shape)} strides {K_.stride()} is not [{rows}, positions, Hkv*D = {Hkv * D}] with unit column stride")
        if (V_.dim() != 4 or tuple(V_.shape) != (rows, Hkv, D, V_.shape[3]) or V_.shape[3] < K_.shape[1]
                or (V_.numel() and V_.stride()[1:] != (D * V_.shape[3], V_.shape[3], 1))):   # a cache of no positions has no strides to speak of
            raise AfkError(f"attn_decode_shared: {vn} {tuple(V_.shape)} strides {V_.stride()} is not [{rows}, Hkv = {Hkv}, D = {D}, spad >= {K_.shape[1]}] with its "
                           f"heads and features contiguous")
    if tuple(prange.shape) != (B0, 2) or not prange.is_contiguous() or tuple(trange.shape) != (R, 2) or not trange.is_contiguous():
        raise AfkError(f"attn_decode_shared: prange {tuple(prange.shape)} / trange {tuple(trange.shape)} are not contiguous [B0 = {B0}, 2] / [B0*n = {R}, 2]")


def attn_decode_shared(q, Kp, Vtp, Kt, Vtt, prange, trange, B0, n, Hq, Hkv, D, scale, nsplit=None, ws=None, out=None):
    """shared-prompt decode attention (afk_attn_decode_shared): one query row per continuation r = b0 * n + c over the prompt keys of row b0 and its own tail
    keys, two launches.  q [B0*n, >= Hq*D] row-strided view (post-RoPE); Kp [B0, Sp, Hkv*D], Vtp [B0, Hkv, D, spad_p] (one layer of the prompt cache);
    Kt [B0*n, T, Hkv*D], Vtt [B0*n, Hkv, D, spad_t] (one layer of the tail cache); prange [B0, 2] / trange [B0*n, 2] int32 on the device: the visible
    intervals.  nsplit None: attn_shared_nsplit over the prompt rows.  ws: a float32 workspace of at least afk_attn_decode_shared_workspace_floats(B0, n, Hq, D,
    nsplit) elements (None: allocated here).  -> o [B0*n, Hq*D] bf16"""
    B0, n = int(B0), int(n)
    R = B0 * n
    _chk(q, BF16, "q")
    if q.dim() != 2 or q.shape[0] != R or q.shape[1] < Hq * D or q.stride(1) != 1:
        raise AfkError(f"attn_decode_shared: q {tuple(q.shape)} strides {q.stride()} is not [B0*n = {R}, >= Hq*D = {Hq * D}] with unit column stride")
    attn_shared_check(Kp, Vtp, Kt, Vtt, prange, trange, B0, n, Hkv, D)
    Sp, T = Kp.shape[1], Kt.shape[1]
    ns = attn_shared_nsplit(B0, n, Hq, Hkv, Sp) if nsplit is None else int(nsplit)
    if ws is None:
        ws = torch.empty(int(_lib.load().afk_attn_decode_shared_workspace_floats(B0, max(min(n, ATTN_SHARED_MAX_COPIES), 1), Hq, D,
                                                                                max(min(ns, ATTN_SHARED_MAX_SPLITS), 1))), device=q.device, dtype=torch.float32)
    else:
        _chk(ws, torch.float32, "ws")
    if out is None:
        o = torch.empty((R, Hq * D), device=q.device, dtype=BF16)
    else:
        o = _chk(out, BF16, "out")
        if tuple(o.shape) != (R, Hq * D) or o.stride(1) != 1:
            raise AfkError(f"attn_decode_shared: out {tuple(o.shape)} strides {o.stride()} is not [B0*n, Hq*D] with unit column stride")
    # the strides are the tensors' own: a cache view with a longer row or sample pitch is read as it lies; a cache of no positions is never dereferenced
    kp, vp, kt, vt = ((t_.data_ptr() if t_.numel() else None) for t_ in (Kp, Vtp, Kt, Vtt))
    _lib.call("afk_attn_decode_shared", q.data_ptr(), q.stride(0), D, kp, Kp.stride(0), Kp.stride(1), D, vp, Vtp.stride(0), Vtp.shape[3], Sp,
              kt, Kt.stride(0), Kt.stride(1), D, vt, Vtt.stride(0), Vtt.shape[3], T, o.data_ptr(), o.stride(0), D, prange.data_ptr(), trange.data_ptr(),
              B0, n, Hq, Hkv, D, float(scale), ns, ws.data_ptr(), ws.numel(), _stream())
    return o


def attn_interval_fwd(qkv, krange, B, S, Hq, Hkv, D, *, scale):
    """self-attention on a fused q|k|v projection with a per-query key interval (left / right / both-side padding, causal or not)"""
    _chk(qkv, BF16, "qkv")
    return xattn_fwd(qkv, qkv[:, Hq * D:], qkv[:, (Hq + Hkv) * D:], krange, B, S, S, Hq, Hkv, D, scale)


def attn_interval_bwd(qkv, o, do, lse, krange, B, S, Hq, Hkv, D, *, scale):
    dqkv = torch.empty_like(qkv)
    xattn_bwd(qkv, qkv[:, Hq * D:], qkv[:, (Hq + Hkv) * D:], o, do, lse, krange, B, S, S, Hq, Hkv, D, scale,
              dqkv, dqkv[:, Hq * D:], dqkv[:, (Hq + Hkv) * D:])
    return dqkv


# ---------------------------------------------------------------------------------------------- row gather / scatter
def gather_rows(x, rows):
    """out[i] = x[rows[i]]   (x [M, H] contiguous bf16, rows int64 on the device): the embedding-gather kernel on an activation matrix"""
    _chk(x, BF16, "gather_rows x")
    assert x.is_contiguous() and rows.dtype == torch.int64
    return embed_scatter_fwd(rows, None, x, None)


def scatter_rows(src, rows, M):
    """out [M, H] zeros except out[rows[i]] = src[i]   (rows unique, ascending)"""
    out = torch.zeros((M, src.shape[1]), device=src.device, dtype=BF16)
    perm = torch.arange(rows.numel(), device=src.device, dtype=torch.int32)
    embed_scatter_bwd(rows, None, src, out, None, perm=perm)
    return out


# ---------------------------------------------------------------------------------------------- token sampling
def decode_sample(logits, *, temperature=1.0, top_k=0, top_p=1.0, seed=0, u=None, step_base=None, step_off=0, out=None, probs_out=None, kept_out=None,
                  tokens_out=None, tok_off=0, state=None, emb=None, x_out=None, min_p=0.0, typical_p=1.0, epsilon_cutoff=0.0, eta_cutoff=0.0, scores_out=None,
                  n_steps=None):
    """next_token [B] (int64) drawn from the fp32 logits [B, V]: temperature -> top-k -> top-p -> min_p -> typical_p -> epsilon_cutoff -> eta_cutoff -> draw in
    one launch (afk_decode_sample_filtered; the contract is in include/afk.h; min_p <= 0, typical_p >= 1, epsilon_cutoff / eta_cutoff outside (0, 1): off).  u [B] fp32 on the device supplies the uniforms; without it they come from Philox4x32-10 keyed by the 64-bit `seed`, counter
    (*step_base + step_off, row).  probs_out [B, V] fp32 / kept_out [B] int32: the distribution drawn from and the size of its support.  state (int32
    [start, end, slot, position], B == 1) with emb / x_out (and tokens_out / tok_off): the step bookkeeping of afk_decode_select_greedy in the same launch.
    scores_out [n_steps, B, V] fp32 (n_steps: the slots the launch may write, default all of them): slot *step_base + step_off receives the warped row - logits /
    temperature on the kept set, -inf elsewhere (afk_decode_sample_scored; without scores_out the launch is afk_decode_sample_filtered's)."""
    _chk(logits, torch.float32, "decode_sample logits")
    if logits.dim() != 2 or logits.stride(1) != 1:
        raise AfkError(f"decode_sample logits: [B, V] with unit column stride, got {tuple(logits.shape)} strides {logits.stride()}")
    B, V = logits.shape
    if out is None:
        out = torch.empty(B, device=logits.device, dtype=torch.int64)
    for t_, dt, n, name in ((out, torch.int64, B, "out"), (u, torch.float32, B, "u"), (kept_out, torch.int32, B, "kept_out"), (step_base, torch.int32, 1, "step_base"),
                            (tokens_out, torch.int64, 1, "tokens_out"), (state, torch.int32, 4, "state")):
        if t_ is not None:
            _chk(t_, dt, f"decode_sample {name}")
            if t_.numel() < n or not t_.is_contiguous():
                raise AfkError(f"decode_sample {name}: a contiguous tensor of at least {n} elements, got {tuple(t_.shape)}")
    if probs_out is not None:
        _chk(probs_out, torch.float32, "decode_sample probs_out")
        if probs_out.shape != logits.shape or probs_out.stride(1) != 1:
            raise AfkError(f"decode_sample probs_out: {tuple(logits.shape)} with unit column stride, got {tuple(probs_out.shape)}")
    H = 0
    if state is not None:
        if emb is None or x_out is None:
            raise AfkError("decode_sample: state needs emb and x_out (the embedding row of the token is the next step's input)")
        _chk(emb, BF16, "decode_sample emb"), _chk(x_out, BF16, "decode_sample x_out")
        H = emb.shape[1]
        if x_out.numel() < H or not x_out.is_contiguous() or V > emb.shape[0]:
            raise AfkError(f"decode_sample: x_out holds {x_out.numel()} elements, emb is {tuple(emb.shape)} for V = {V}")
    scored = ()
    if scores_out is not None:
        n_steps = _step_buffer_chk(scores_out, B, V, n_steps, "decode_sample scores_out")
        scored = (scores_out.data_ptr(), scores_out.stride(0), scores_out.stride(1), n_steps)
    elif n_steps is not None:
        raise AfkError("decode_sample: n_steps counts the slots of scores_out, which was not given")
    seed = int(seed) & (2 ** 64 - 1)
    _lib.call("afk_decode_sample_scored" if scored else "afk_decode_sample_filtered", logits.data_ptr(), logits.stride(0), B, V, float(temperature), int(top_k or 0),
              float(top_p), float(min_p), float(typical_p), float(epsilon_cutoff), float(eta_cutoff), _p(u),
              seed - 2 ** 64 if seed >= 2 ** 63 else seed, _p(step_base), int(step_off), out.data_ptr(), _p(probs_out),
              probs_out.stride(0) if probs_out is not None else 0, _p(kept_out), _p(tokens_out), int(tok_off), _p(state), _p(emb),
              emb.stride(0) if emb is not None else 0, H, _p(x_out), *scored, _stream())
    return out


def _step_buffer_chk(buf, B, V, n_steps, name):
    """buf: the [slots, B, V] fp32 buffer a decode step writes one slot of (unit column stride, rows and slots that do not overlap) -> the slot count to pass"""
    _chk(buf, torch.float32, name)
    if buf.dim() != 3 or tuple(buf.shape[1:]) != (B, V) or buf.shape[0] < 1 or buf.stride(2) != 1 or buf.stride(1) < V or buf.stride(0) < (B - 1) * buf.stride(1) + V:
        raise AfkError(f"{name}: [n_steps, {B}, {V}] with unit column stride and non-overlapping rows, got {tuple(buf.shape)} strides {buf.stride()}")
    n = buf.shape[0] if n_steps is None else int(n_steps)
    if not 1 <= n <= buf.shape[0]:
        raise AfkError(f"{name}: n_steps {n} outside the buffer's {buf.shape[0]} slots")
    return n


def decode_record(src, dst, *, step_base=None, step_off=0, n_steps=None):
    """dst[t] = src, a bit copy of the fp32 rows [B, V] into slot t = *step_base + step_off of dst [n_steps, B, V] in one launch (afk_decode_record; the contract
    is in include/afk.h): how generate() keeps a step's logits / scores from inside the captured step.  step_base: int32 on the device (None = 0); a t outside
    [0, n_steps) writes nothing (refused here where the host knows t, i.e. without step_base).  -> dst"""
    _chk(src, torch.float32, "decode_record src")
    if src.dim() != 2 or src.stride(1) != 1 or src.stride(0) < src.shape[1]:
        raise AfkError(f"decode_record src: [B, V] with unit column stride, got {tuple(src.shape)} strides {src.stride()}")
    B, V = src.shape
    n_steps = _step_buffer_chk(dst, B, V, n_steps, "decode_record dst")
    if step_base is not None:
        _chk(step_base, torch.int32, "decode_record step_base")
        if step_base.numel() < 1 or not step_base.is_contiguous():
            raise AfkError(f"decode_record step_base: a contiguous tensor of at least 1 element, got {tuple(step_base.shape)}")
    elif not 0 <= int(step_off) < n_steps:
        raise AfkError(f"decode_record: step {int(step_off)} outside the buffer's {n_steps} slots")
    _lib.call("afk_decode_record", src.data_ptr(), src.stride(0), B, V, dst.data_ptr(), dst.stride(0), dst.stride(1), n_steps, _p(step_base), int(step_off), _stream())
    return dst


def decode_cfg_workspace(B, V, device):
    """the workspace of decode_cfg for B rows of V columns (afk_decode_cfg_workspace_floats): uninitialised fp32; a decode step allocates it once"""
    return torch.empty(int(_lib.load().afk_decode_cfg_workspace_floats(int(B), int(V))), device=device, dtype=torch.float32)


def decode_cfg(cond, uncond, scale, out=None, *, ws=None):
    """classifier-free guidance on fp32 logits rows [B, V] in one call of two launches (afk_decode_cfg; the contract is in include/afk.h):
    out = scale * (log_softmax(cond) - log_softmax(uncond)) + log_softmax(uncond), a NaN logit counting as -inf.  out: None (a new tensor), cond itself (in
    place) or any other [B, V] fp32 tensor that overlaps neither input; rows need unit column stride only.  ws: decode_cfg_workspace(B, V) (None: allocated
    here - a captured step passes its own).  -> out"""
    _chk(cond, torch.float32, "decode_cfg cond"), _chk(uncond, torch.float32, "decode_cfg uncond")
    if cond.dim() != 2 or cond.shape[0] < 1 or cond.shape[1] < 1:
        raise AfkError(f"decode_cfg cond: [B >= 1, V >= 1], got {tuple(cond.shape)}")
    B, V = cond.shape
    if out is None:
        out = torch.empty((B, V), device=cond.device, dtype=torch.float32)
    _chk(out, torch.float32, "decode_cfg out")
    for t_, name in ((cond, "cond"), (uncond, "uncond"), (out, "out")):
        if tuple(t_.shape) != (B, V) or t_.stride(1) != 1 or (B > 1 and t_.stride(0) < V) or t_.device != cond.device:
            raise AfkError(f"decode_cfg {name}: [{B}, {V}] on {cond.device} with unit column stride and non-overlapping rows, got {tuple(t_.shape)} strides "
                           f"{t_.stride()} on {t_.device}")
    span = lambda t_: (t_.data_ptr(), t_.data_ptr() + 4 * ((B - 1) * t_.stride(0) + V))
    overlap = lambda a, b: span(a)[0] < span(b)[1] and span(b)[0] < span(a)[1]
    if overlap(out, uncond) or (overlap(out, cond) and not (out.data_ptr() == cond.data_ptr() and (B == 1 or out.stride(0) == cond.stride(0)))):
        raise AfkError("decode_cfg out: it may be cond itself (in place); it must not overlap uncond, or cond in any other way")
    if ws is None:
        ws = decode_cfg_workspace(B, V, cond.device)
    _chk(ws, torch.float32, "decode_cfg ws")
    if not ws.is_contiguous() or ws.device != cond.device:
        raise AfkError(f"decode_cfg ws: a contiguous fp32 tensor on {cond.device} (decode_cfg_workspace), got strides {ws.stride()} on {ws.device}")
    ld = lambda t_: t_.stride(0) if B > 1 else V
    _lib.call("afk_decode_cfg", cond.data_ptr(), ld(cond), uncond.data_ptr(), ld(uncond), float(scale), out.data_ptr(), ld(out), B, V, ws.data_ptr(), ws.numel(),
              _stream())
    return out


def transition_scores(scores, tokens, *, normalize=False, out=None):
    """out [B, T] fp32 = scores[t, b, tokens[b, t]] - (normalize: logsumexp of that row), scores [T, B, V] fp32 with unit column stride, tokens [B, T] int64
    (afk_transition_scores: GenerationMixin.compute_transition_scores without beam_indices).  The ids are validated on the host (one sync: a post-hoc call)."""
    _chk(scores, torch.float32, "transition_scores scores")
    if scores.dim() != 3 or scores.stride(2) != 1 or scores.stride(1) < scores.shape[2] or scores.shape[0] < 1:
        raise AfkError(f"transition_scores scores: [T, B, V] with unit column stride, got {tuple(scores.shape)} strides {scores.stride()}")
    T, B, V = scores.shape
    _chk(tokens, torch.int64, "transition_scores tokens")
    if tuple(tokens.shape) != (B, T) or tokens.stride(1) != 1:
        raise AfkError(f"transition_scores tokens: [{B}, {T}] with unit column stride, got {tuple(tokens.shape)} strides {tokens.stride()}")
    if bool(((tokens < 0) | (tokens >= V)).any()):
        raise AfkError(f"transition_scores tokens: ids outside the vocabulary [0, {V})")
    if out is None:
        out = torch.empty((B, T), device=scores.device, dtype=torch.float32)
    _chk(out, torch.float32, "transition_scores out")
    if tuple(out.shape) != (B, T) or out.stride(1) != 1:
        raise AfkError(f"transition_scores out: [{B}, {T}] with unit column stride, got {tuple(out.shape)} strides {out.stride()}")
    _lib.call("afk_transition_scores", scores.data_ptr(), scores.stride(0), scores.stride(1), T, B, V, tokens.data_ptr(), tokens.stride(0), 1 if normalize else 0,
              out.data_ptr(), out.stride(0), _stream())
    return out


def decode_process(logits, hist, seen, *, S0, penalty=1.0, ngram=0, suppress=None, begin_suppress=None, eos=None, min_new_tokens=0, next_token=None,
                   step_base=None, step_off=0, select=False, tokens_out=None, tok_off=0, state=None, emb=None, x_out=None):
    """the fp32 logits [B, V] processed IN PLACE for token t = *step_base + step_off: repetition penalty -> no-repeat n-gram -> eos / suppress / begin-suppress bans
    in one launch (afk_decode_process; the contract is in include/afk.h).  hist [B, ld] int32: the S0 prompt ids then the selected tokens; seen [B, ld_seen] int32:
    one bit per vocabulary id of the row's history (decode_process.build_state fills both from the prompt); next_token [B] int64: the token selected for t - 1,
    appended by the launch (only token 0 has none).  suppress / begin_suppress / eos: int32 id lists on the device.  select (B == 1; state, emb, x_out, and
    tokens_out / tok_off): greedy selection from the processed row and the step bookkeeping of afk_decode_select_greedy in the same launch.  -> logits"""
    _lib.call("afk_decode_process", *_decode_process_args(logits, hist, seen, S0, penalty, ngram, suppress, begin_suppress, eos, min_new_tokens, next_token,
                                                          step_base, step_off, select, tokens_out, tok_off, state, emb, x_out), _stream())
    return logits


def _decode_process_args(logits, hist, seen, S0, penalty, ngram, suppress, begin_suppress, eos, min_new_tokens, next_token, step_base, step_off, select,
                         tokens_out, tok_off, state, emb, x_out):
    """the checks of decode_process / decode_process_ex -> the 29 arguments their entry points share"""
    _chk(logits, torch.float32, "decode_process logits")
    if logits.dim() != 2 or logits.stride(1) != 1:
        raise AfkError(f"decode_process logits: [B, V] with unit column stride, got {tuple(logits.shape)} strides {logits.stride()}")
    B, V = logits.shape
    for t_, name, cols in ((hist, "hist", int(S0)), (seen, "seen", (V + 31) // 32)):
        _chk(t_, torch.int32, f"decode_process {name}")
        if t_.dim() != 2 or t_.shape[0] != B or t_.stride(1) != 1 or t_.shape[1] < cols:
            raise AfkError(f"decode_process {name}: [{B}, >= {cols}] with unit column stride, got {tuple(t_.shape)} strides {t_.stride()}")
    for t_, dt, n, name in ((next_token, torch.int64, B, "next_token"), (step_base, torch.int32, 1, "step_base"), (tokens_out, torch.int64, 1, "tokens_out"),
                            (state, torch.int32, 4, "state"), (suppress, torch.int32, 0, "suppress"), (begin_suppress, torch.int32, 0, "begin_suppress"),
                            (eos, torch.int32, 0, "eos")):
        if t_ is not None:
            _chk(t_, dt, f"decode_process {name}")
            if t_.numel() < n or not t_.is_contiguous():
                raise AfkError(f"decode_process {name}: a contiguous tensor of at least {n} elements, got {tuple(t_.shape)}")
    if next_token is None and (step_base is not None or step_off != 0 or select):
        raise AfkError("decode_process: next_token (the token selected for t - 1) is needed for every token but token 0 without selection")
    H = 0
    if select:
        if state is None or emb is None or x_out is None:
            raise AfkError("decode_process: select needs state, emb and x_out (the embedding row of the token is the next step's input)")
        _chk(emb, BF16, "decode_process emb"), _chk(x_out, BF16, "decode_process x_out")
        H = emb.shape[1]
        if x_out.numel() < H or not x_out.is_contiguous() or V > emb.shape[0]:
            raise AfkError(f"decode_process: x_out holds {x_out.numel()} elements, emb is {tuple(emb.shape)} for V = {V}")
    n_of = lambda t_: 0 if t_ is None else t_.numel()
    return (logits.data_ptr(), logits.stride(0), B, V, hist.data_ptr(), hist.stride(0), int(S0), seen.data_ptr(), seen.stride(0),
            _p(step_base), int(step_off), _p(next_token), float(penalty), int(ngram), _p(suppress) if n_of(suppress) else None, n_of(suppress),
            _p(begin_suppress) if n_of(begin_suppress) else None, n_of(begin_suppress), _p(eos) if n_of(eos) else None, n_of(eos), int(min_new_tokens),
            1 if select else 0, _p(tokens_out) if select else None, int(tok_off), _p(state) if select else None, _p(emb) if select else None,
            emb.stride(0) if select else 0, H, _p(x_out) if select else None)


def _sequence_table_args(tb, name, dev):
    """a packed sequence table (decode_process.pack_sequences, as device tensors; None = empty) -> its 8 arguments, the shapes checked against each other: the
    kernel trusts the offsets"""
    if tb is None:
        return (None, None, None, 0, None, None, None, 0)
    for k, dt in (("ids", torch.int32), ("seq_off", torch.int32), ("seq_bias", torch.float32), ("group_id", torch.int32), ("group_l1", torch.float32),
                  ("group_off", torch.int32)):
        _chk(tb[k], dt, f"decode_process_ex {name}.{k}")
        if tb[k].dim() != 1 or not tb[k].is_contiguous() or tb[k].device != dev:
            raise AfkError(f"decode_process_ex {name}.{k}: a contiguous 1-d tensor on {dev}, got {tuple(tb[k].shape)} on {tb[k].device}")
    n_seqs, n_groups = tb["seq_bias"].numel(), tb["group_id"].numel()
    if n_groups < 1 or tb["group_l1"].numel() != n_groups or tb["group_off"].numel() != n_groups + 1 or tb["seq_off"].numel() != n_seqs + 1:
        raise AfkError(f"decode_process_ex {name}: {n_groups} groups (>= 1) need group_l1 [{n_groups}], group_off [{n_groups + 1}]; {n_seqs} sequences need "
                       f"seq_off [{n_seqs + 1}]")
    return (_p(tb["ids"]) if tb["ids"].numel() else None, _p(tb["seq_off"]), _p(tb["seq_bias"]) if n_seqs else None, n_seqs, _p(tb["group_id"]),
            _p(tb["group_l1"]), _p(tb["group_off"]), n_groups)


def decode_process_ex(logits, hist, seen, *, S0, max_new_tokens, bias=None, bad=None, min_length=0, forced_eos=None, decay=None, decay_start=0, penalty=1.0,
                      ngram=0, suppress=None, begin_suppress=None, eos=None, min_new_tokens=0, next_token=None, step_base=None, step_off=0, select=False,
                      tokens_out=None, tok_off=0, state=None, emb=None, x_out=None):
    """decode_process with the other built-in processors in the reference's order, still one launch (afk_decode_process_ex; the contract is in include/afk.h):
    sequence bias -> repetition penalty -> no-repeat n-gram -> bad words -> min_length / min_new_tokens -> forced EOS at token max_new_tokens - 1 -> exponential
    decay length penalty -> suppress / begin-suppress.  bias / bad: packed sequence tables as dicts of device tensors (decode_process.pack_sequences, which
    refuses ids outside the vocabulary; bad's biases are -inf); forced_eos: int32 id list; decay: fp32 [>= max_new_tokens], decay[t] = pow(factor, t -
    decay_start) - 1, applied to the eos ids when t > decay_start.  The offsets inside a table are trusted: build it with pack_sequences.  -> logits"""
    common = _decode_process_args(logits, hist, seen, S0, penalty, ngram, suppress, begin_suppress, eos, min_new_tokens, next_token, step_base, step_off,
                                  select, tokens_out, tok_off, state, emb, x_out)
    for t_, dt, name in ((forced_eos, torch.int32, "forced_eos"), (decay, torch.float32, "decay")):
        if t_ is not None:
            _chk(t_, dt, f"decode_process_ex {name}")
            if t_.dim() != 1 or not t_.is_contiguous():
                raise AfkError(f"decode_process_ex {name}: a contiguous 1-d tensor, got {tuple(t_.shape)}")
    n_of = lambda t_: 0 if t_ is None else t_.numel()
    _lib.call("afk_decode_process_ex", *common, *_sequence_table_args(bias, "bias", logits.device), *_sequence_table_args(bad, "bad", logits.device),
              int(min_length), _p(forced_eos) if n_of(forced_eos) else None, n_of(forced_eos), _p(decay), n_of(decay), int(decay_start), int(max_new_tokens),
              _stream())
    return logits


def decode_stop(next_token, ids, stop_at, *, S0, max_new, status=None, step_base=None, step_off=0, eos=None, pad=0, feed_pad=False, table=None, P=0, E=0, S=0,
                target_lens=None, W=0):
    """the stopping rule for token t = *step_base + step_off, the one JUST SELECTED into next_token [B] int64, in one launch (afk_decode_stop; the contract is in
    include/afk.h): a row that finished earlier emits `pad` (and, feed_pad, has it written to next_token); the token joins ids [B, >= S0 + max_new] int32; a row
    still open is judged - tok in eos (int32 id list on the device), or a stop string matched by StopStringCriteria's rule over its own table [rows, S * (P + E) + 1]
    int32 with target_lens [S] int32 and W = maximum_token_len - and a hit sets stop_at[b] = t (int32, INT_MAX = open).  status [2] int32 receives
    {t, rows still open}.  A t outside [0, max_new) writes nothing.  -> stop_at"""
    _chk(next_token, torch.int64, "decode_stop next_token")
    if next_token.dim() != 1 or not next_token.is_contiguous():
        raise AfkError(f"decode_stop next_token: a contiguous [B] tensor, got {tuple(next_token.shape)}")
    B = next_token.shape[0]
    _chk(ids, torch.int32, "decode_stop ids")
    if ids.dim() != 2 or ids.shape[0] != B or ids.stride(1) != 1 or (B > 1 and ids.stride(0) < ids.shape[1]):
        raise AfkError(f"decode_stop ids: [{B}, >= S0 + max_new] with unit column stride, got {tuple(ids.shape)} strides {ids.stride()}")
    if int(S0) < 0 or int(max_new) < 1 or int(S0) + int(max_new) > ids.shape[1]:
        raise AfkError(f"decode_stop: S0 + max_new = {int(S0)} + {int(max_new)} ids in rows of {ids.shape[1]} (S0 >= 0, max_new >= 1, S0 + max_new <= ids.shape[1])")
    S = int(S)
    for t_, dt, n, name in ((stop_at, torch.int32, B, "stop_at"), (status, torch.int32, 2, "status"), (step_base, torch.int32, 1, "step_base"),
                            (eos, torch.int32, 0, "eos"), (target_lens, torch.int32, max(S, 0), "target_lens")):
        if t_ is not None:
            _chk(t_, dt, f"decode_stop {name}")
            if t_.numel() < n or not t_.is_contiguous():
                raise AfkError(f"decode_stop {name}: a contiguous tensor of at least {n} elements, got {tuple(t_.shape)}")
    if stop_at is None:
        raise AfkError("decode_stop: stop_at is needed")
    rows = vec = 0
    if S != 0:
        if table is None or target_lens is None:
            raise AfkError("decode_stop: stop strings (S > 0) need table and target_lens")
        _chk(table, torch.int32, "decode_stop table")
        if table.dim() != 2 or not table.is_contiguous():
            raise AfkError(f"decode_stop table: a contiguous [rows, vec] tensor, got {tuple(table.shape)} strides {table.stride()}")
        rows, vec = table.shape
    n_eos = 0 if eos is None else eos.numel()
    _lib.call("afk_decode_stop", next_token.data_ptr(), B, ids.data_ptr(), ids.stride(0) if B > 1 else ids.shape[1], int(S0), int(max_new), stop_at.data_ptr(),
              _p(status), _p(step_base), int(step_off), _p(eos) if n_eos else None, n_eos, int(pad), 1 if feed_pad else 0, _p(table) if S else None, rows, vec,
              int(P), int(E), S, _p(target_lens) if S else None, int(W), _stream())
    return stop_at


BEAM_MAX_BEAMS, BEAM_MAX_KEEP = 16, 64   # AFK_BEAM_MAX_BEAMS / AFK_BEAM_MAX_KEEP of include/afk.h
_BEAM_STATE = (("run_score", torch.float32), ("fin_score", torch.float32), ("fin_len", torch.int32), ("fin_done", torch.int32), ("fin_slot", torch.int32),
               ("fin_seq", torch.int32), ("can_improve", torch.int32), ("bp", torch.int32), ("next_token", torch.int64), ("src", torch.int32),
               ("status", torch.int32), ("ws", torch.int32))


def beam_caps_ok(nb, n_eos, V):
    """does afk_beam_step take nb beams with n_eos eos ids over a vocabulary of V?  (2 <= nb <= 16, keep = (n_eos + 1) * nb <= 64, keep <= nb * V < 2^31)"""
    keep = (int(n_eos) + 1) * int(nb)
    return 2 <= int(nb) <= BEAM_MAX_BEAMS and keep <= BEAM_MAX_KEEP and keep <= int(nb) * int(V) < 2 ** 31


def beam_state(B, nb, max_new, *, device, eos=(), length_penalty=1.0, early_stopping=False):
    """the device state of one beam search over B rows x nb beams x max_new tokens, initialised as afk_beam_step's contract asks (include/afk.h): a dict of
    the kernel's buffers - run_score [B, nb], fin_score / fin_len / fin_done / fin_slot [B, nb], fin_seq [B, nb, max_new] (row fin_slot[b, k] holds the tokens
    of the hypothesis ranked k), can_improve [B], bp [max_new, B, nb, 2], next_token / src [B * nb], status [2], ws - and of its constants: eos (int32 on the
    device, or None), early (0 False, 1 True, 2 "never") and the divisor tables div / hdiv [max_new] fp32, computed here in double:
    div[t] = (t + 1) ** length_penalty, hdiv[t] = max_new ** length_penalty under early_stopping == "never" with a positive penalty, else div[t]."""
    B, nb, max_new = int(B), int(nb), int(max_new)
    eos = [int(e) for e in eos]
    if early_stopping not in (False, True, "never"):
        raise AfkError(f"beam_state: early_stopping must be False, True or 'never', got {early_stopping!r}")
    if B < 1 or max_new < 1 or not 2 <= nb <= BEAM_MAX_BEAMS or (len(eos) + 1) * nb > BEAM_MAX_KEEP:
        raise AfkError(f"beam_state: B = {B}, max_new = {max_new}, {nb} beams, {len(eos)} eos ids (B, max_new >= 1, 2 <= nb <= {BEAM_MAX_BEAMS}, "
                       f"(n_eos + 1) * nb <= {BEAM_MAX_KEEP})")
    lp = float(length_penalty)
    div = [float((t + 1) ** lp) for t in range(max_new)]
    hdiv = [float(max_new ** lp)] * max_new if (early_stopping == "never" and lp > 0.0) else div
    i32 = lambda *shape: torch.zeros(shape, device=device, dtype=torch.int32)
    run_score = torch.full((B, nb), -1.0e9, device=device, dtype=torch.float32)
    run_score[:, 0] = 0.0   # all beams of a row start identical: only the first one is live
    return dict(B=B, nb=nb, max_new=max_new, n_eos=len(eos), early=2 if early_stopping == "never" else int(bool(early_stopping)),
                eos=torch.tensor(eos, device=device, dtype=torch.int32) if eos else None,
                div=torch.tensor(div, dtype=torch.float64).to(torch.float32).to(device), hdiv=torch.tensor(hdiv, dtype=torch.float64).to(torch.float32).to(device),
                run_score=run_score, fin_score=torch.full((B, nb), -1.0e9, device=device, dtype=torch.float32), fin_len=i32(B, nb), fin_done=i32(B, nb),
                fin_slot=torch.arange(nb, device=device, dtype=torch.int32).repeat(B, 1).contiguous(), fin_seq=i32(B, nb, max_new),
                can_improve=torch.ones(B, device=device, dtype=torch.int32), bp=i32(max_new, B, nb, 2),
                next_token=torch.zeros(B * nb, device=device, dtype=torch.int64), src=torch.arange(B * nb, device=device, dtype=torch.int32),
                status=torch.tensor([-1, 1], device=device, dtype=torch.int32), ws=i32(int(_lib.load().afk_beam_step_workspace_ints(B, nb, len(eos)))))


def beam_step(logits, st, *, step_base=None, step_off=0):
    """one beam-search step for token t = *step_base + step_off on the fp32 logits [B * nb, V] (beam j of row b at b * nb + j), in one call of two launches
    (afk_beam_step; the contract is in include/afk.h): the row's best (n_eos + 1) * nb continuations by accumulated log-probability (equal scores: the lower
    flat index j * V + token), the finished slots, the running beams with their tokens in st["next_token"] and their parents' cache rows in st["src"], the
    early-stop heuristic, and st["status"] = {t, open}.  st: a dict from beam_state().  A t outside [0, max_new) and a call whose status says closed write
    nothing.  -> st"""
    _chk(logits, torch.float32, "beam_step logits")
    if logits.dim() != 2 or logits.stride(1) != 1 or (logits.shape[0] > 1 and logits.stride(0) < logits.shape[1]):
        raise AfkError(f"beam_step logits: [B * nb, V] with unit column stride, got {tuple(logits.shape)} strides {logits.stride()}")
    B, nb, max_new = int(st["B"]), int(st["nb"]), int(st["max_new"])
    R, V = logits.shape
    if R != B * nb:
        raise AfkError(f"beam_step logits: {R} rows for {B} rows x {nb} beams")
    if not beam_caps_ok(nb, st["n_eos"], V):
        raise AfkError(f"beam_step: {nb} beams, {st['n_eos']} eos ids, V = {V} (2 <= nb <= {BEAM_MAX_BEAMS}, keep = (n_eos + 1) * nb <= {BEAM_MAX_KEEP}, "
                       f"keep <= nb * V < 2^31)")
    sizes = dict(run_score=R, fin_score=R, fin_len=R, fin_done=R, fin_slot=R, fin_seq=R * max_new, can_improve=B, bp=2 * max_new * R, next_token=R, src=R,
                 status=2, ws=int(_lib.load().afk_beam_step_workspace_ints(B, nb, int(st["n_eos"]))))
    for name, dt in _BEAM_STATE + (("div", torch.float32), ("hdiv", torch.float32)):
        t_ = st.get(name)
        if t_ is None:
            raise AfkError(f"beam_step: the state holds no {name} (ops.beam_state builds it)")
        _chk(t_, dt, f"beam_step {name}")
        if t_.numel() < sizes.get(name, max_new) or not t_.is_contiguous():
            raise AfkError(f"beam_step {name}: a contiguous tensor of at least {sizes.get(name, max_new)} elements, got {tuple(t_.shape)}")
    eos = st.get("eos")
    if (0 if eos is None else eos.numel()) != int(st["n_eos"]):
        raise AfkError(f"beam_step eos: {st['n_eos']} ids announced, got {None if eos is None else tuple(eos.shape)}")
    if eos is not None:
        _chk(eos, torch.int32, "beam_step eos")
        if not eos.is_contiguous():
            raise AfkError("beam_step eos: a contiguous int32 list")
    if step_base is not None:
        _chk(step_base, torch.int32, "beam_step step_base")
        if step_base.numel() < 1 or not step_base.is_contiguous():
            raise AfkError(f"beam_step step_base: a contiguous tensor of at least 1 element, got {tuple(step_base.shape)}")
    _lib.call("afk_beam_step", logits.data_ptr(), logits.stride(0) if R > 1 else V, B, nb, V, max_new, _p(step_base), int(step_off), _p(eos) if eos is not None else None,
              int(st["n_eos"]), int(st["early"]), st["div"].data_ptr(), st["hdiv"].data_ptr(), st["run_score"].data_ptr(), st["fin_score"].data_ptr(),
              st["fin_len"].data_ptr(), st["fin_done"].data_ptr(), st["fin_slot"].data_ptr(), st["fin_seq"].data_ptr(), st["can_improve"].data_ptr(),
              st["bp"].data_ptr(), st["next_token"].data_ptr(), st["src"].data_ptr(), st["status"].data_ptr(), st["ws"].data_ptr(), st["ws"].numel(), _stream())
    return st


def beam_finished(st):
    """-> (seq [B, nb, max_new] int64, len [B, nb] int64, score [B, nb] fp32, done [B, nb] bool): the finished hypotheses of a beam_state in ranking order (the
    token rows gathered through fin_slot); entries of a hypothesis behind its length are unspecified"""
    B, nb, max_new = int(st["B"]), int(st["nb"]), int(st["max_new"])
    slot = st["fin_slot"].view(B, nb).long().clamp(0, nb - 1)
    seq = st["fin_seq"].view(B, nb, max_new).gather(1, slot[:, :, None].expand(B, nb, max_new)).long()
    return seq, st["fin_len"].view(B, nb).long(), st["fin_score"].view(B, nb).clone(), st["fin_done"].view(B, nb) != 0


def beam_reorder_cache(Kc, Vt, src, cur, *, nb, S0, max_new):
    """the KV cache moved by beam parentage in place (afk_beam_reorder_cache; the contract is in include/afk.h): Kc [L, B * nb, Smax, Hkv * D] and
    Vt [L, B * nb, Hkv, D, pad64(Smax)] bf16, src [B * nb] int32 = each beam's parent as a flat cache row (clamped into its own row's group), cur: int32 on the
    device - the slots S0 .. *cur move, the prompt slots (shared by a row's beams bit for bit) and everything behind *cur stay.  -> (Kc, Vt)"""
    _chk(Kc, BF16, "beam_reorder_cache Kc"), _chk(Vt, BF16, "beam_reorder_cache Vt")
    nb = int(nb)
    if Kc.dim() != 4 or Vt.dim() != 5 or not Kc.is_contiguous() or not Vt.is_contiguous():
        raise AfkError(f"beam_reorder_cache: contiguous Kc [L, R, Smax, Hkv * D] and Vt [L, R, Hkv, D, spad], got {tuple(Kc.shape)} and {tuple(Vt.shape)}")
    L, R, Smax, nk = Kc.shape
    _, _, Hkv, D, spad = Vt.shape
    if tuple(Vt.shape[:2]) != (L, R) or Hkv * D != nk or spad < Smax or nb < 2 or R % nb:
        raise AfkError(f"beam_reorder_cache: Kc {tuple(Kc.shape)} and Vt {tuple(Vt.shape)} do not describe one cache of rows in groups of {nb}")
    if int(S0) < 0 or int(max_new) < 1 or int(S0) + int(max_new) > Smax:
        raise AfkError(f"beam_reorder_cache: S0 + max_new = {int(S0)} + {int(max_new)} slots in a cache of {Smax}")
    for t_, n, name in ((src, R, "src"), (cur, 1, "cur")):
        _chk(t_, torch.int32, f"beam_reorder_cache {name}")
        if t_.numel() < n or not t_.is_contiguous():
            raise AfkError(f"beam_reorder_cache {name}: a contiguous tensor of at least {n} elements, got {tuple(t_.shape)}")
    _lib.call("afk_beam_reorder_cache", Kc.data_ptr(), Vt.data_ptr(), L, R // nb, nb, Smax, spad, Hkv, D, int(S0), int(max_new), src.data_ptr(), cur.data_ptr(),
              _stream())
    return Kc, Vt


# ---------------------------------------------------------------------------------------------- loss
def count_valid(labels):
    out = torch.empty(1, device=labels.device, dtype=torch.float32)
    _lib.call("afk_count_valid", labels.data_ptr(), labels.numel(), out.data_ptr(), _stream())
    return out


def ce_fwd_bwd_(logits, shift_labels, row_loss, denom, *, upstream=1.0, write_grad=True):
    rows, V = logits.shape
    _lib.call("afk_ce_fwd_bwd", logits.data_ptr(), logits.stride(0), rows, V, shift_labels.data_ptr(), row_loss.data_ptr(),
              denom.data_ptr(), float(upstream), int(write_grad), _stream())


def _chk_logprob_args(who, logits, shift_labels, vectors):
    """logits: 2-D bf16 rows with unit inner stride; shift_labels int64 and every (name, fp32 vector) contiguous with one element per row"""
    _chk(logits, BF16, f"{who} logits"), _chk(shift_labels, torch.int64, f"{who} shift_labels")
    if logits.dim() != 2 or logits.stride(1) != 1 or logits.shape[0] < 1 or logits.shape[1] < 1:
        raise AfkError(f"{who} logits: a non-empty 2-D chunk with unit inner stride, got shape {tuple(logits.shape)} strides {tuple(logits.stride())}")
    rows = logits.shape[0]
    for name, t in (("shift_labels", shift_labels), *vectors):
        if name != "shift_labels":
            _chk(t, torch.float32, f"{who} {name}")
        if t.dim() != 1 or t.shape[0] != rows or not t.is_contiguous():
            raise AfkError(f"{who} {name}: a contiguous vector of {rows} elements (one per row of the chunk), got shape {tuple(t.shape)}")
    return rows, logits.shape[1]


def token_logprob(logits, shift_labels, logp, lse, entropy=None):
    """per row of the bf16 chunk: logp = log_softmax(logits)[label], lse = logsumexp(logits), entropy (optional) = -sum p log p; an ignored row
    (label < 0) gives 0 in all three.  The chunk is not written (afk_token_logprob; the contract is in include/afk.h).  -> logp"""
    vectors = [("logp", logp), ("lse", lse)] + ([("entropy", entropy)] if entropy is not None else [])
    rows, V = _chk_logprob_args("token_logprob", logits, shift_labels, vectors)
    _lib.call("afk_token_logprob", logits.data_ptr(), logits.stride(0), rows, V, shift_labels.data_ptr(), logp.data_ptr(), lse.data_ptr(), _p(entropy),
              _stream())
    return logp


def token_logprob_bwd_(logits, shift_labels, lse, u):
    """in place on the RECOMPUTED chunk: logits <- bf16(u_row * (onehot(label) - exp(logits - lse_row))), u = d L / d logp per row; an ignored row
    becomes zeros whatever u holds (afk_token_logprob_bwd).  -> logits"""
    rows, V = _chk_logprob_args("token_logprob_bwd_", logits, shift_labels, [("lse", lse), ("u", u)])
    _lib.call("afk_token_logprob_bwd", logits.data_ptr(), logits.stride(0), rows, V, shift_labels.data_ptr(), lse.data_ptr(), u.data_ptr(), _stream())
    return logits


def loss_reduce(row_loss, denom, loss, *, accumulate=False):
    _lib.call("afk_loss_reduce", row_loss.data_ptr(), row_loss.numel(), denom.data_ptr(), loss.data_ptr(), int(accumulate),
              _stream())
    return loss


# ---------------------------------------------------------------------------------------------- optimizer
def _chk_adamw32(who, master, m, v, grad, param, numel, shadow=None, NK=None):
    """the five streams of the fp32-state AdamW launches: fp32 master / m / v, bf16 grad / param, contiguous, `numel` elements each, and (transposed
    form) a bf16 shadow that can hold [K, N]; all on the device.  The kernels index the five streams by one offset: a short or a wrongly typed
    buffer would be read and written out of bounds."""
    streams = ((master, torch.float32, "master"), (m, torch.float32, "m"), (v, torch.float32, "v"), (grad, BF16, "grad"), (param, BF16, "param"))
    for t, dtype, what in streams:
        if t.dtype != dtype:
            raise AfkError(f"{who} {what}: expected dtype {dtype}, got {t.dtype}")
        if not t.is_contiguous():
            raise AfkError(f"{who} {what}: not contiguous (shape {tuple(t.shape)}, strides {t.stride()})")
        if t.numel() != numel:
            raise AfkError(f"{who} {what}: {t.numel()} elements, expected {numel}")
    if shadow is not None:
        N, K = NK
        if shadow.dtype != BF16:
            raise AfkError(f"{who} shadow: expected dtype {BF16}, got {shadow.dtype}")
        if shadow.dim() != 2 or shadow.stride(1) != 1 or shadow.shape[0] < K or shadow.shape[1] < N or shadow.stride(0) < N:
            raise AfkError(f"{who} shadow: {tuple(shadow.shape)} (strides {shadow.stride()}) cannot hold [K, N] = [{K}, {N}]")
        streams += ((shadow, BF16, "shadow"),)
    for t, _, what in streams:
        _chk(t, None, f"{who} {what}")


def adamw_step(master, m, v, grad, param, *, lr, beta1, beta2, eps, weight_decay, step, grad_scale=1.0, max_blocks=0, gate=None, hyper=None):
    """gate: optional device int32[1]; the launch leaves every buffer untouched when it reads 0.
    hyper: optional device float32[4] = (lr, 1 - beta1^t, sqrt(1 - beta2^t), gradient multiplier) overriding lr / step (HIP-graph replay);
    hyper[3] multiplies every gradient (global-norm clip coefficient, 1 = off)"""
    _chk_adamw32("adamw", master, m, v, grad, param, param.numel())
    _lib.call("afk_adamw_step", master.data_ptr(), m.data_ptr(), v.data_ptr(), grad.data_ptr(), param.data_ptr(), param.numel(),
              float(lr), float(beta1), float(beta2), float(eps), float(weight_decay), int(step), float(grad_scale),
              int(max_blocks), _p(gate), _p(hyper), _stream())


def adamw_step_t(master, m, v, grad, param, shadow, N, K, *, lr, beta1, beta2, eps, weight_decay, step, grad_scale=1.0, max_blocks=0, gate=None, hyper=None):
    """afk_adamw_step on one 2-D weight [N, K] (flat views of the arena) that also writes shadow [K, ld] = the K-major copy of the updated weight"""
    _chk_adamw32("adamw_t", master, m, v, grad, param, int(N) * int(K), shadow, (int(N), int(K)))
    _lib.call("afk_adamw_step_t", master.data_ptr(), m.data_ptr(), v.data_ptr(), grad.data_ptr(), param.data_ptr(), shadow.data_ptr(), int(N), int(K),
              shadow.stride(0), float(lr), float(beta1), float(beta2), float(eps), float(weight_decay), int(step), float(grad_scale), int(max_blocks),
              _p(gate), _p(hyper), _stream())


def adamw16_step(m, v, grad, param, *, lr, beta1, beta2, eps, weight_decay, step, grad_scale=1.0, max_blocks=0, gate=None, hyper=None):
    """AdamW with bf16 state (torch.optim.AdamW(fused=True) on bf16 tensors; 14 B/param): param / m / v are bf16 and updated in place, there is no
    fp32 master.  gate / hyper / max_blocks as adamw_step."""
    for t, what in ((m, "adamw16 m"), (v, "adamw16 v"), (grad, "adamw16 grad"), (param, "adamw16 param")):
        _chk(t, BF16, what)
        if t.numel() != param.numel():
            raise AfkError(f"{what}: {t.numel()} elements, param has {param.numel()}")
    _lib.call("afk_adamw16_step", m.data_ptr(), v.data_ptr(), grad.data_ptr(), param.data_ptr(), param.numel(),
              float(lr), float(beta1), float(beta2), float(eps), float(weight_decay), int(step), float(grad_scale),
              int(max_blocks), _p(gate), _p(hyper), _stream())


def adamw16_step_t(m, v, grad, param, shadow, N, K, *, lr, beta1, beta2, eps, weight_decay, step, grad_scale=1.0, max_blocks=0, gate=None, hyper=None):
    """adamw16_step on one 2-D weight [N, K] (flat views of the arena) that also writes shadow [K, ld] = the K-major copy of the updated weight"""
    for t, what in ((m, "adamw16_t m"), (v, "adamw16_t v"), (grad, "adamw16_t grad"), (param, "adamw16_t param")):
        _chk(t, BF16, what)
        if t.numel() != int(N) * int(K):
            raise AfkError(f"{what}: {t.numel()} elements, [N, K] = [{N}, {K}]")
    _chk(shadow, BF16, "adamw16_t shadow")
    if shadow.shape[0] < int(K) or shadow.stride(0) < int(N):
        raise AfkError(f"adamw16_t shadow: {tuple(shadow.shape)} (row stride {shadow.stride(0)}) cannot hold [K, N] = [{K}, {N}]")
    _lib.call("afk_adamw16_step_t", m.data_ptr(), v.data_ptr(), grad.data_ptr(), param.data_ptr(), shadow.data_ptr(), int(N), int(K),
              shadow.stride(0), float(lr), float(beta1), float(beta2), float(eps), float(weight_decay), int(step), float(grad_scale), int(max_blocks),
              _p(gate), _p(hyper), _stream())


def sumsq_workspace_floats() -> int:
    return int(_lib.load().afk_sumsq_workspace_floats())


def sumsq_(x, acc, *, gate=None, ws=None):
    """acc[0] += sum(x^2) over a bf16 range (fp32, deterministic); skipped on the device when gate (int32[1]) reads 0"""
    _chk(x, BF16, "sumsq x")
    if ws is None:
        ws = torch.empty(_lib.load().afk_sumsq_workspace_floats(), device=x.device, dtype=torch.float32)
    _lib.call("afk_sumsq_bf16", x.data_ptr(), x.numel(), _chk(acc, torch.float32).data_ptr(), _p(gate), ws.data_ptr(), _stream())
    return acc


def clip_coef_(sumsq, coef, *, max_norm, scale=1.0, norm_out=None):
    """coef[0] = min(1, max_norm / (sqrt(sum(sumsq)) * scale + 1e-6))   (torch.nn.utils.clip_grad_norm_); norm_out[0] = the norm.
    sumsq: float32 [n] partial sums, folded in index order"""
    _lib.call("afk_clip_coef", _chk(sumsq, torch.float32).data_ptr(), sumsq.numel(), float(scale), float(max_norm), coef.data_ptr(), _p(norm_out), _stream())


def set_f32(dst, values):
    """dst[:len(values)] = values (<= 4 floats), by a kernel launch on the current stream"""
    v = [float(x) for x in values] + [0.0] * (4 - len(values))
    _lib.call("afk_set_f32", _chk(dst, torch.float32).data_ptr(), len(values), v[0], v[1], v[2], v[3], _stream())


def gemm_set_variant(v: int):
    """0 auto, 1 = 128x128 kernel, 2 = 256x256 ping-pong kernel (tests / microbenchmarks)"""
    _lib.call("afk_gemm_set_variant", int(v))


def gemm_set_mfma(v: int):
    """MFMA shape of the 256x256 kernels: 0 = the dispatch rule, 1 = 32x32x16, 2 = 16x16x32 (tests / A-B measurements; env AFK_GEMM_MFMA for a whole run)"""
    _lib.call("afk_gemm_set_mfma", int(v))


def gemm_mfma_shapes(form: str) -> tuple:
    """which of the shapes (1 = 32x32x16, 2 = 16x16x32) the loaded library carries for form "nt" | "nn" | "tn" (the other one: make PROBES=1)"""
    mask = _lib.load().afk_gemm_mfma_shapes(("nt", "nn", "tn").index(form))
    return tuple(v for v in (1, 2) if mask >> (v - 1) & 1)


# ---------------------------------------------------------------------------------------------- profiling
KERNEL_FAMILIES = ("gemm_nt128", "gemm_nt256", "gemm_nn256", "gemm_tn256", "gemm_splitk", "gemv", "attn2_fwd_d64", "attn2_fwd_d128",
                   "attn2_bwd_d64", "attn2_bwd_d128", "gqa_reduce", "xattn_fwd", "xattn_bwd", "attn1_fwd", "attn1_bwd", "gemm_generic_epilogue")


def kernel_counts(reset: bool = False) -> dict:
    """launches per kernel family since the last reset (include/afk.h AFK_CNT_*): lets a test assert which kernel served a shape"""
    import ctypes

    buf = (ctypes.c_int64 * len(KERNEL_FAMILIES))()
    _lib.call("afk_kernel_counts", ctypes.addressof(buf), len(KERNEL_FAMILIES))
    if reset:
        _lib.call("afk_kernel_counts_reset")
    return dict(zip(KERNEL_FAMILIES, list(buf)))


def prof_enable(on: bool):
    _lib.call("afk_prof_enable", int(on))


def prof_reset():
    _lib.call("afk_prof_reset")


def prof_collect():
    import ctypes
    ms, fl, n = ctypes.c_double(), ctypes.c_double(), ctypes.c_int64()
    _lib.call("afk_prof_collect", ctypes.addressof(ms), ctypes.addressof(fl), ctypes.addressof(n))
    return ms.value, fl.value, n.value

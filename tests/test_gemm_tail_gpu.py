"""The peeled K-loop tail of the 256x256 GEMM kernels (NT, NN, TN): the last two K-tiles run outside the steady-state loop, stage nothing past tile T-1
and carry their own vmcnt waits (csrc/gemm256.hip k_tile), so a wrong wait shows up as a stale or half-landed LDS tile.  Shapes are the smallest that
reach every tail path with the 256x256 kernel forced (afk_gemm_set_variant(2)): T = 1 (prologue -> last tile), T = 2 (prologue -> tile T-2 -> last tile),
T = 3, 4 (one and two steady tiles in front) and T = 20 (the encoder's K = 1280); full and ragged output tiles; every epilogue the step instantiates,
SwiGLU-forward and RoPE included (they reuse the operand buffers right behind the loop); split-K with local T = 1 and 6 - 7; TN's ragged last tile.

Operands are N(0, 1) bf16 on fixed seeds.  References are torch fp64 products of the same operands, rounded as tests/test_ops_gpu.py rounds its GEMM
references and held to that file's tolerance (_cmp, atol = 0.02 sqrt(K), rtol = 1e-2 - tests/_tol.py carries the model-level bars only, none for a GEMM);
the fused SwiGLU / RoPE outputs are in addition bit-equal to the elementwise kernel applied to the GEMM output.  Every call is repeated three times and
must return the same bits.  test_previous_k_loop_bit_equal compares every case bit for bit with the previous K loop (afk_gemm_set_variant(15)), which
only a `make PROBES=1` library named by AFK_LIB_PATH carries.
"""
import math
import os
from contextlib import contextmanager

import pytest
import torch

from test_ops_gpu import BF, _cmp, _ops, _rand

pytestmark = pytest.mark.gpu

NT_K = [64, 128, 192, 256, 1280]
NT_MN = [(256, 256), (300, 520)]
XT_K = {"nn": [64, 128, 192, 1280], "tn": [64, 128, 192, 200, 1280]}
XT_MN = [(256, 256), (256, 264), (264, 256), (264, 264)]
SPLIT_CASES = [(192, 2), (192, 3), (1280, 2), (1280, 3)]   # local T: 1 | 2, 1 | 1 | 1, 10 | 10, 6 | 7 | 7


@contextmanager
def _forced(ops, variant=2, mfma=0):
    """the 256x256 kernel whatever the tile count; the NT split-K plan (128x128 kernel) off"""
    old = ops.SPLITK
    ops.gemm_set_variant(variant)
    ops.gemm_set_mfma(mfma)
    ops.SPLITK = False
    try:
        yield
    finally:
        ops.SPLITK = old
        ops.gemm_set_mfma(0)
        ops.gemm_set_variant(0)


def _randn(shape, dev, seed):
    return _rand(shape, dev, seed=seed).to(BF)


def _thrice(name, fn):
    """one call repeated three times on the same operands: the same bits each time"""
    first = fn()
    for _ in range(2):
        again = fn()
        for x, y in zip(first, again):
            assert torch.equal(x, y), f"{name}: non-deterministic result (LDS race?)"
    return first


# ------------------------------------------------------------------------------------------------ the cases: name -> (call, [(reference, output index)])
def _nt_cases(ops, dev, M, N, K):
    """plain, bias, residual, bias + GELU with preact_out, accumulate"""
    a, b = _randn((M, K), dev, 101), _randn((N, K), dev, 102)
    bias, res = _randn((N,), dev, 103), _randn((M, N), dev, 104)
    prod = a.double() @ b.double().t()
    lin = (prod + bias.double()).to(BF).double()

    def gelu_call():
        pre = torch.empty((M, N), device=dev, dtype=BF)
        return ops.gemm_nt(a, b, bias=bias, gelu=True, preact_out=pre), pre

    return {
        "plain": (lambda: (ops.gemm_nt(a, b),), [prod]),
        "bias": (lambda: (ops.gemm_nt(a, b, bias=bias),), [prod + bias.double()]),
        "residual": (lambda: (ops.gemm_nt(a, b, residual=res),), [prod.to(BF).double() + res.double()]),
        "bias+gelu": (gelu_call, [torch.nn.functional.gelu(lin), lin]),
        "accumulate": (lambda: (ops.gemm_nt(a, b, out=res.clone(), accumulate=True),), [prod + res.double()]),
    }


def _swiglu_case(ops, dev, M, K):
    """N = 512: gate | up of 256 features, two N tiles of 128 + 128 weight rows"""
    x, w = _randn((M, K), dev, 111), _randn((512, K), dev, 112)

    def call():
        h = torch.full((M, 256), float("nan"), device=dev, dtype=BF)
        return ops.gemm_nt(x, w, swiglu_fwd_out=h), h

    return call, x.double() @ w.double().t()


def _rope_tables(dev, S, D=128):
    inv = 1.0 / (1e6 ** (torch.arange(0, D, 2, device=dev, dtype=torch.float32) / D))
    fr = torch.arange(S + 16, device=dev, dtype=torch.float32)[:, None] * inv[None]
    emb = torch.cat([fr, fr], -1)
    return emb.cos().to(BF).contiguous(), emb.sin().to(BF).contiguous()


def _rope_case(ops, dev, M, K, with_pos):
    """N = 512, rope_cols = 256, S = 32: tile 0 holds two rotated heads, tile 1 two untouched ones.  ops.gemm_nt_rope only fuses from 192 tiles up, so the
    C entry is called directly; the forced variant routes it to the 256x256 kernel"""
    from audio_flamingo_amd import _lib
    S, D, N, rc = 32, 128, 512, 256
    a, w, bias = _randn((M, K), dev, 121), _randn((N, K), dev, 122), _randn((N,), dev, 123)
    cos, sin = _rope_tables(dev, S)
    pos = ((torch.arange(M, device=dev, dtype=torch.int32) * 7) % (S + 16)).contiguous() if with_pos else None
    cl, sl = (None, None) if with_pos else (ops._rope_lanes(cos, S, D, 1), ops._rope_lanes(sin, S, D, 1))

    def call():
        out = torch.full((M, N), float("nan"), device=dev, dtype=BF)
        _lib.call("afk_gemm_nt_bf16_rope", a.data_ptr(), a.stride(0), w.data_ptr(), w.stride(0), out.data_ptr(), out.stride(0), M, N, K, bias.data_ptr(),
                  cos.data_ptr(), sin.data_ptr(), ops._p(pos), S, rc, ops._p(cl), ops._p(sl), ops._stream())
        return (out,)

    def unfused(lin):
        ref = lin.clone()
        ops.rope_(ref, cos, sin, S=S, nheads=rc // D, D=D, pos=pos)
        return ref

    return call, unfused, a.double() @ w.double().t() + bias.double(), lambda: ops.gemm_nt(a, w, bias=bias), rc


def _xt_case(ops, dev, form, M, N, K, splits):
    a = _randn((K, M) if form == "tn" else (M, K), dev, 131)
    b = _randn((K, N), dev, 132)
    prod = (a.double().t() if form == "tn" else a.double()) @ b.double()
    return (lambda: (ops.gemm(a, b, trans_a=form == "tn", trans_b=True, _splits=splits),)), prod


def _tol(K):
    return dict(atol=0.02 * math.sqrt(K), rtol=1e-2)


# ------------------------------------------------------------------------------------------------ against fp64
@pytest.mark.parametrize("K", NT_K)
def test_nt_tail_epilogues(dev, K):
    ops = _ops()
    shapes = ops.gemm_mfma_shapes("nt")
    assert shapes
    for M, N in NT_MN:
        cases = _nt_cases(ops, dev, M, N, K)
        for shape in shapes:
            with _forced(ops, mfma=shape):
                ops.kernel_counts(reset=True)
                for name, (call, refs) in cases.items():
                    outs = _thrice(f"nt {name} {M}x{N}x{K} mfma {shape}", call)
                    for out, ref in zip(outs, refs):
                        _cmp(f"nt {name} {M}x{N}x{K} mfma {shape}", out, ref, **_tol(K))
                cnt = ops.kernel_counts()
                assert cnt["gemm_nt256"] == 3 * len(cases) and cnt["gemm_generic_epilogue"] == 0, cnt


@pytest.mark.parametrize("K", NT_K)
def test_nt_tail_swiglu_fwd(dev, K):
    ops = _ops()
    for M in (256, 300):
        call, prod = _swiglu_case(ops, dev, M, K)
        for shape in ops.gemm_mfma_shapes("nt"):
            with _forced(ops, mfma=shape):
                gu, h = _thrice(f"swiglu {M}x512x{K}", call)
                _cmp(f"swiglu gate|up {M}x512x{K} mfma {shape}", gu, prod, **_tol(K))
                assert torch.equal(h, ops.silu_mul_fwd(gu)), "h differs from silu_mul on the gate|up output of the same launch"


@pytest.mark.parametrize("K", NT_K)
def test_nt_tail_rope_bias(dev, K):
    ops = _ops()
    for M, with_pos in ((256, False), (300, False), (300, True)):
        call, unfused, lin64, plain, rc = _rope_case(ops, dev, M, K, with_pos)
        for shape in ops.gemm_mfma_shapes("nt"):
            with _forced(ops, mfma=shape):
                ops.kernel_counts(reset=True)
                (got,) = _thrice(f"rope {M}x512x{K}", call)
                assert ops.kernel_counts()["gemm_nt256"] == 3
                lin = plain()
                _cmp(f"rope: plain qkv {M}x512x{K} mfma {shape}", lin, lin64, **_tol(K))
                assert torch.equal(got, unfused(lin)), float((got.float() - unfused(lin).float()).abs().max())
                _cmp(f"rope: v columns {M}x512x{K} mfma {shape}", got[:, rc:], lin64[:, rc:], **_tol(K))
                assert not torch.equal(got[:, :rc], lin[:, :rc])


@pytest.mark.parametrize("form,K", [(f, K) for f in ("nn", "tn") for K in XT_K[f]])
def test_xt_tail(dev, form, K):
    ops = _ops()
    shapes = ops.gemm_mfma_shapes(form)
    assert shapes
    for M, N in XT_MN:
        call, prod = _xt_case(ops, dev, form, M, N, K, 1)
        for shape in shapes:
            with _forced(ops, mfma=shape):
                ops.kernel_counts(reset=True)
                (c,) = _thrice(f"{form} {M}x{N}x{K}", call)
                assert ops.kernel_counts()[f"gemm_{form}256"] == 3
                _cmp(f"{form} {M}x{N}x{K} mfma {shape}", c, prod, **_tol(K))


@pytest.mark.parametrize("form", ["nn", "tn"])
@pytest.mark.parametrize("K,splits", SPLIT_CASES)
def test_xt_tail_splitk(dev, form, K, splits):
    ops = _ops()
    for M, N in ((256, 256), (264, 264)):
        call, prod = _xt_case(ops, dev, form, M, N, K, splits)
        for shape in ops.gemm_mfma_shapes(form):
            with _forced(ops, mfma=shape):
                ops.kernel_counts(reset=True)
                (c,) = _thrice(f"{form} split-K {M}x{N}x{K}/{splits}", call)
                assert ops.kernel_counts()["gemm_splitk"] == 3
                _cmp(f"{form} split-K {M}x{N}x{K}/{splits} mfma {shape}", c, prod, **_tol(K))


# ------------------------------------------------------------------------------------------------ against the previous K loop
def test_previous_k_loop_bit_equal(dev):
    """every case above, new K loop (variant 2) against the previous one (variant 15: clamped tail prefetches and a drain in front of the epilogue)"""
    from audio_flamingo_amd import _lib
    if not os.environ.get("AFK_LIB_PATH") or not _lib.has_probes():
        pytest.skip("needs AFK_LIB_PATH = a `make PROBES=1` library (the previous K loop is not in the default build)")
    ops = _ops()
    calls = []
    for K in NT_K:
        for M, N in NT_MN:
            calls += [("nt", f"nt {name} {M}x{N}x{K}", call) for name, (call, _) in _nt_cases(ops, dev, M, N, K).items()]
        for M in (256, 300):
            calls.append(("nt", f"swiglu {M}x512x{K}", _swiglu_case(ops, dev, M, K)[0]))
            calls.append(("nt", f"rope {M}x512x{K}", _rope_case(ops, dev, M, K, False)[0]))
    for form in ("nn", "tn"):
        for K in XT_K[form]:
            calls += [(form, f"{form} {M}x{N}x{K}", _xt_case(ops, dev, form, M, N, K, 1)[0]) for M, N in XT_MN]
        calls += [(form, f"{form} split-K 264x264x{K}/{s}", _xt_case(ops, dev, form, 264, 264, K, s)[0]) for K, s in SPLIT_CASES]
    for form, name, call in calls:
        for shape in ops.gemm_mfma_shapes(form):
            with _forced(ops, variant=2, mfma=shape):
                new = call()
            with _forced(ops, variant=15, mfma=shape):
                old = call()
            for x, y in zip(new, old):
                assert torch.equal(x, y), f"{name} mfma {shape}: the peeled tail changed the result"

"""The 256x256 GEMM kernels (NT, NN, TN) on each MFMA shape the library carries (ops.gemm_set_mfma: 1 = 32x32x16, 2 = 16x16x32), with the variant
forced to the 256x256 kernel.  Only fragments, MFMA calls and the accumulator -> (m, n) map differ between the shapes, so every case checks values
against the fp32 product, bit-equal repeats (LDS race check) and - on operands from {-1, 0, 1} with K <= 192, where every partial sum is a small integer
and no rounding happens anywhere - exact equality with the fp32 product and between the shapes: any row / column / k permutation shows up exactly.
A shape that a kernel carries only under `make PROBES=1` is covered by tools/probes/test_probe_gemm_mfma_shape.py, which runs this file on such a build.
"""
import math
from contextlib import contextmanager

import pytest
import torch

from test_ops_gpu import BF, _cmp, _ops, _rand

pytestmark = pytest.mark.gpu

SHAPE_NAME = {1: "32x32x16", 2: "16x16x32"}


@contextmanager
def _forced(ops, shape, splitk=False):
    """variant 2 = the 256x256 kernel; the NT split-K plan (which runs on the 128x128 kernel) is off unless a test is about it"""
    old = ops.SPLITK
    ops.gemm_set_variant(2)
    ops.gemm_set_mfma(shape)
    ops.SPLITK = splitk
    try:
        yield
    finally:
        ops.SPLITK = old
        ops.gemm_set_mfma(0)
        ops.gemm_set_variant(0)


def _tri(shape, dev, seed):
    """operands from {-1, 0, 1}"""
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randint(0, 3, shape, generator=g) - 1).to(dev).to(BF)


def _run(ops, form, a, b, **kw):
    if form == "nt":
        return ops.gemm_nt(a, b, **kw)
    return ops.gemm(a, b, trans_a=form == "tn", trans_b=True, **kw)


def _operands(form, M, N, K, dev, make):
    a = make((K, M) if form == "tn" else (M, K), dev, 11)
    b = make((N, K) if form == "nt" else (K, N), dev, 12)
    af = a.float().t() if form == "tn" else a.float()
    bf = b.float().t() if form == "nt" else b.float()
    return a, b, af @ bf


def _randn(shape, dev, seed):
    return _rand(shape, dev, seed=seed).to(BF)


# K-tiles 1 / 2 / 3 / 5 / many (prologue and tail of the vmcnt ladder), M and N tails, tiny M, 4-wide narrow stores (N % 8 == 4), ragged K (TN)
CASES = ([("nt", *s) for s in [(256, 256, 64), (256, 256, 128), (512, 768, 192), (300, 260, 320), (8, 512, 4096), (777, 1028, 64)]] +
         [("nn", *s) for s in [(256, 256, 64), (304, 264, 320), (8, 512, 4096)]] +
         [("tn", *s) for s in [(256, 256, 64), (304, 264, 320), (8, 512, 100)]])


@pytest.mark.parametrize("form,M,N,K", CASES)
def test_gemm_mfma_shapes(dev, form, M, N, K):
    ops = _ops()
    a, b, ref = _operands(form, M, N, K, dev, _randn)
    bias = _rand((N,), dev, seed=13).to(BF)
    shapes = ops.gemm_mfma_shapes(form)
    assert shapes, "the library carries no MFMA shape for this kernel"
    for shape in shapes:
        with _forced(ops, shape):
            ops.kernel_counts(reset=True)
            c = _run(ops, form, a, b, bias=bias, **({} if form == "nt" else {"_splits": 1}))
            assert ops.kernel_counts()[f"gemm_{form}256"] == 1      # the 256x256 kernel served it
            _cmp(f"gemm {form} {SHAPE_NAME[shape]} {M}x{N}x{K}", c, ref + bias.float(), atol=0.02 * math.sqrt(K), rtol=1e-2)
            for _ in range(3):
                assert torch.equal(_run(ops, form, a, b, bias=bias, **({} if form == "nt" else {"_splits": 1})), c), "non-deterministic GEMM (LDS race?)"


@pytest.mark.parametrize("form,M,N,K,splits", [("nt", 130, 260, 2048, None), ("nn", 304, 264, 8192, 16), ("tn", 520, 264, 4100, 4)])
def test_gemm_mfma_shapes_splitk(dev, form, M, N, K, splits):
    """fp32 partials (the 4-wide f32 store of the accumulators as they lie) + the fixed-order fold; the NT split-K plan runs on the 128x128 kernel"""
    ops = _ops()
    a, b, ref = _operands(form, M, N, K, dev, _randn)
    bias = _rand((N,), dev, seed=13).to(BF)
    for shape in ops.gemm_mfma_shapes(form):
        with _forced(ops, shape, splitk=True):
            if form == "nt":
                ops.gemm_set_variant(0)
                assert ops.splitk_plan(M, N, K) > 1
            kw = {} if form == "nt" else {"_splits": splits}
            ops.kernel_counts(reset=True)
            c = _run(ops, form, a, b, bias=bias, **kw)
            assert ops.kernel_counts()["gemm_splitk"] == 1
            _cmp(f"split-K {form} {SHAPE_NAME[shape]}", c, ref + bias.float(), atol=0.02 * math.sqrt(K), rtol=1e-2)
            for _ in range(3):
                assert torch.equal(_run(ops, form, a, b, bias=bias, **kw), c), "non-deterministic split-K GEMM"


@pytest.mark.parametrize("form,M,N,K,splits", [("nt", 300, 260, 192, 1), ("nt", 777, 1028, 64, 1), ("nn", 304, 264, 192, 1), ("tn", 304, 264, 192, 1), ("tn", 264, 520, 100, 1),
                                               ("nn", 304, 264, 192, 3), ("tn", 304, 264, 192, 2)])
def test_gemm_mfma_shapes_exact(dev, form, M, N, K, splits):
    """{-1, 0, 1} operands, K <= 192: every partial sum is an integer of magnitude <= 192, exact in fp32 and in bf16, whatever the summation order"""
    ops = _ops()
    a, b, ref = _operands(form, M, N, K, dev, _tri)
    assert ref.abs().max() <= 192 and torch.equal(ref.to(BF).float(), ref)
    outs = []
    for shape in ops.gemm_mfma_shapes(form):
        with _forced(ops, shape):
            c = _run(ops, form, a, b, **({} if form == "nt" else {"_splits": splits}))
        assert torch.equal(c, ref.to(BF)), f"{form} {SHAPE_NAME[shape]}: {int((c.float() != ref).sum())} wrong elements, first {(c.float() != ref).nonzero()[:4].tolist()}"
        outs.append(c)
    for c in outs[1:]:
        assert torch.equal(c, outs[0])


def _nt_shapes(ops):
    shapes = ops.gemm_mfma_shapes("nt")
    assert shapes
    return shapes


def test_gemm_mfma_shapes_epilogues(dev):
    """bias; residual with res_mod; bias + GELU with the pre-activation output; ACCUM; fp32 output; the generic (runtime-flag, narrow) form"""
    ops = _ops()
    M, N, K = 384, 512, 256
    a = _rand((M, K), dev, 0.5, 3).to(BF)
    b = _rand((N, K), dev, 0.1, 4).to(BF)
    bias = _rand((N,), dev, 1.0, 5).to(BF)
    res = _rand((M, N), dev, 1.0, 6).to(BF)
    tab = _rand((96, N), dev, 1.0, 7).to(BF)
    prod = a.float() @ b.float().t()
    lin = (prod + bias.float()).to(BF).float()
    for shape in _nt_shapes(ops):
        with _forced(ops, shape):
            ops.kernel_counts(reset=True)
            _cmp("bias", ops.gemm_nt(a, b, bias=bias), lin, atol=2e-2, rtol=1e-2)
            pre = torch.empty((M, N), device=dev, dtype=BF)
            c = ops.gemm_nt(a, b, bias=bias, gelu=True, preact_out=pre)
            _cmp("preact", pre, lin, atol=2e-2, rtol=1e-2)
            _cmp("bias+gelu", c, torch.nn.functional.gelu(lin), atol=2e-2, rtol=1e-2)
            _cmp("bias+res", ops.gemm_nt(a, b, bias=bias, residual=res), lin + res.float(), atol=3e-2, rtol=1e-2)
            _cmp("res_mod", ops.gemm_nt(a, b, residual=tab, res_mod=96), prod.to(BF).float() + tab.float().repeat(M // 96, 1), atol=3e-2, rtol=1e-2)
            cb = res.clone()
            ops.gemm_nt(a, b, out=cb, accumulate=True)
            _cmp("bf16 accum", cb, prod + res.float(), atol=4e-2, rtol=1e-2)
            assert ops.kernel_counts()["gemm_generic_epilogue"] == 0 and ops.kernel_counts()["gemm_nt256"] == 5
            # fp32 output (+ accumulate) is outside the step's instantiations: the runtime-flag form, wide
            c32 = torch.ones((M, N), device=dev, dtype=torch.float32)
            ops.gemm_nt(a, b, out=c32, accumulate=True)
            _cmp("f32 accum", c32, prod + 1.0, atol=1e-2, rtol=1e-3)
            # N % 8 == 4: no 16-byte epilogue -> the generic instantiation with 4-wide stores, bias + residual
            ops.kernel_counts(reset=True)
            c = ops.gemm_nt(a, b[:260], bias=bias[:260], residual=res[:, :260].contiguous())
            assert ops.kernel_counts()["gemm_generic_epilogue"] == 1
            _cmp("generic narrow", c, lin[:, :260] + res[:, :260].float(), atol=3e-2, rtol=1e-2)


@pytest.mark.parametrize("M,I,K", [(700, 512, 256), (1000, 128, 64)])
def test_gemm_mfma_shapes_swiglu_fwd(dev, M, I, K):
    """SwiGLU forward in the epilogue == silu_mul on the plain GEMM output of the same shape, bit for bit, on both outputs"""
    ops = _ops()
    x = _rand((M, K), dev, 1.0, 1).to(BF)
    w = _rand((2 * I, K), dev, 0.5, 2).to(BF)
    for shape in _nt_shapes(ops):
        with _forced(ops, shape):
            gu_ref = ops.gemm_nt(x, w)
            h_ref = ops.silu_mul_fwd(gu_ref)
            h = torch.full((M, I), float("nan"), device=dev, dtype=BF)
            gu = ops.gemm_nt(x, w, swiglu_fwd_out=h)
            assert torch.equal(gu, gu_ref), "gate|up pre-activations differ"
            assert torch.equal(h, h_ref), "fused silu(gate) * up differs from the two-kernel form"


@pytest.mark.parametrize("M,S,Hq,Hkv,K,with_pos,with_bias", [(3072, 1024, 28, 4, 512, False, True), (3000, 1000, 28, 4, 512, False, False), (6000, 750, 14, 2, 1024, True, False)])
def test_gemm_mfma_shapes_rope(dev, M, S, Hq, Hkv, K, with_pos, with_bias):
    """RoPE in the epilogue == GEMM + rope kernel, bit for bit: lane-major tables (S % 32 == 0, no positions), per-row tables (S % 32 != 0 / explicit
    positions), with and without bias; the v heads right of rope_cols stay the plain GEMM's"""
    ops = _ops()
    D = 128
    N, rc = (Hq + 2 * Hkv) * D, (Hq + Hkv) * D
    a = _rand((M, K), dev, 1.0, 31).to(BF)
    w = _rand((N, K), dev, K ** -0.5, 32).to(BF)
    bias = _rand((N,), dev, 0.5, 33).to(BF) if with_bias else None
    inv = 1.0 / (1e6 ** (torch.arange(0, D, 2, device=dev, dtype=torch.float32) / D))
    fr = torch.arange(S + 16, device=dev, dtype=torch.float32)[:, None] * inv[None]
    emb = torch.cat([fr, fr], -1)
    cos, sin = emb.cos().to(BF).contiguous(), emb.sin().to(BF).contiguous()
    pos = ((torch.arange(M, device=dev, dtype=torch.int32) * 7) % (S + 16)).contiguous() if with_pos else None
    old = ops.GEMM_FUSE_ROPE
    try:
        for shape in _nt_shapes(ops):
            with _forced(ops, shape):
                ops.GEMM_FUSE_ROPE = False
                ref = ops.gemm_nt_rope(a, w, bias, cos, sin, S=S, rope_cols=rc, D=D, pos=pos)
                plain = ops.gemm_nt(a, w, bias=bias)
                ops.GEMM_FUSE_ROPE = True
                got = ops.gemm_nt_rope(a, w, bias, cos, sin, S=S, rope_cols=rc, D=D, pos=pos)
                assert torch.equal(got, ref), float((got.float() - ref.float()).abs().max())
                assert torch.equal(got[:, rc:], plain[:, rc:]) and not torch.equal(got[:, :rc], plain[:, :rc])
    finally:
        ops.GEMM_FUSE_ROPE = old


def test_gemm_set_mfma_refuses_what_the_build_lacks(dev):
    from audio_flamingo_amd import _lib
    ops = _ops()
    carried = set(ops.gemm_mfma_shapes("nt")) | set(ops.gemm_mfma_shapes("nn")) | set(ops.gemm_mfma_shapes("tn"))
    try:
        for v in (1, 2):
            if v in carried:
                ops.gemm_set_mfma(v)
            else:
                with pytest.raises(_lib.AfkError, match="PROBES"):
                    ops.gemm_set_mfma(v)
        with pytest.raises(_lib.AfkError):
            ops.gemm_set_mfma(3)
    finally:
        ops.gemm_set_mfma(0)

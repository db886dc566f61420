"""GPU: the training / prefill GEMMs (csrc/gemm.hip, gemm256.hip, gemm256t.hip) bit for bit against integer references, at the edges of their tiles and guards.

tests/_gemm_ref.py draws operands on which every rounding point of the kernels is exact ({-1, 0, 1} operands and cos / sin tables, small integer bias, residual
and accumulate base, alpha in {1, 0.5, 2, -1}), so the expected output is integer arithmetic and every launch - whatever its kernel, K split, MFMA shape or
epilogue form - must equal it with torch.equal.  tests/test_gemm_ref_cpu.py shows on the reference alone that a dropped or doubled k element, a dropped K tile, a
dropped or twice-folded split, a neighbouring row / column / bias element, a ragged mask one off, an unwrapped residual row, an ignored accumulate or alpha,
swapped SwiGLU halves and the rotate-half partner of the wrong head each change it.  The comparisons with a bound are the two activations, on exact inputs:
  * bias + GELU: `preact` is exact; the output is BIT-EQUAL to ops.gelu_fwd(preact) - both kernels evaluate gelu_f (csrc/common.h) on the same fp32 value, the
    bf16-rounded Linear output - and is in addition held to the bound of tests/_norm_ref.gelu_ref, as tests/test_activations_gpu.py holds the elementwise kernel;
  * SwiGLU forward: gate|up exact, h bit-equal to ops.silu_mul_fwd(gate|up) and inside the SwiGLU bound of _norm_ref against fp64 (for a gate <= -88, where fp32
    exp(-g) overflows and both kernels return h = 0 for an exact |silu| of ~1e-37, between 0 and the exact value: the integer gates reach -100 at K = 1280);
  * SwiGLU backward: bit-equal to ops.silu_mul_bwd(gate|up, the exact dh).

Every launch writes into sentinel-filled buffers - the output (an inner block of a buffer with a guard row above and below, and guard columns where the case is
strided), preact_out, swiglu_fwd_out, the split-K workspace with a tail behind it - and everything outside the written [M, N] must keep the sentinel bit for bit.
The split-K partials themselves are held to the per-split integer sums.  Operands sit in sentinel-filled buffers as column slices at a non-zero offset in every
second case; `ops.kernel_counts` says which kernel and which epilogue instantiation ran.  Each shape was read against the guards of gemm_impl and the kernel
that takes it before it was launched; the shapes gemm_impl refuses are in test_refused_shapes."""
from collections import Counter
from contextlib import contextmanager

import pytest
import torch

from tests import _gemm_ref as R
from tests import _norm_ref as NR

pytestmark = pytest.mark.gpu

BF, F32, F64 = torch.bfloat16, torch.float32, torch.float64
SENT = 768.0                     # 3 x 2^8: a bf16 / fp32 value, and none an exact case writes (|v| <= 256 there)
WS_TAIL = 64                     # floats behind the split-K workspace
GEMM_FAMILIES = ("gemm_nt128", "gemm_nt256", "gemm_nn256", "gemm_tn256", "gemv")
EXACT = Counter()                # launches compared exactly, per kernel family


def _ops():
    from audio_flamingo_amd import ops

    return ops


@contextmanager
def _forced(ops, variant=0, mfma=0, gm=None):
    """the kernel a case names whatever its tile count (1 = 128x128, 2 = 256x256), the MFMA shape, the group height of the tile map; ops' own split-K plan off"""
    old = ops.SPLITK
    ops.gemm_set_variant(variant + 256 * (gm or 0))
    ops.gemm_set_mfma(mfma)
    ops.SPLITK = False
    try:
        yield
    finally:
        ops.SPLITK = old
        ops.gemm_set_mfma(0)
        ops.gemm_set_variant(0)


def _full(shape, dev, dtype=BF):
    return torch.full(shape, SENT, device=dev, dtype=dtype)


def _vec(t, dev, dtype=BF):
    v = t.to(dev).to(dtype).contiguous()
    assert torch.equal(v.double(), t.to(dev).double()), "an operand is not a value of its format"
    return v


def _rows(t, dev, pad=0, off=0, vec=8):
    """t [R, C] as the columns off .. off + C of a sentinel-filled [R, C + pad] bf16 buffer, rows aligned to vectors of `vec` elements"""
    t = t.to(dev)
    buf = _full((t.shape[0], t.shape[1] + pad), dev)
    view = buf[:, off:off + t.shape[1]]
    view.copy_(t)
    assert torch.equal(view.double(), t.double()), "an operand is not a bf16 value"
    assert view.data_ptr() % (2 * vec) == 0 and view.stride(0) % vec == 0 and off <= pad
    return view


class Want:
    """what a buffer must hold after the launch: the sentinel everywhere but in the written block"""

    def __init__(self, shape, dev):
        self.exp = torch.full(shape, SENT, device=dev, dtype=F64)
        self.mask = torch.zeros(shape, device=dev, dtype=torch.bool)

    def put(self, index, value):
        self.exp[index] = value
        self.mask[index] = True
        return self

    def hold(self, tag, got, bound=None):
        """bound None: torch.equal.  bound [written block]: |got - want| <= bound inside the block, the sentinel bit for bit outside it"""
        g = got.double().reshape(self.exp.shape)
        if bound is None:
            ok = torch.equal(g, self.exp)
            bad = (g != self.exp) if not ok else None
        else:
            full = torch.zeros_like(self.exp)
            full[self.mask] = bound.reshape(-1)
            bad = ~((g - self.exp).abs() <= full)
            ok = not bool(bad.any())
        if not ok:
            at = bad.nonzero()[0].tolist()
            i = tuple(at)
            raise AssertionError(f"{tag}: {int(bad.sum())} of {bad.numel()} elements differ ({int((bad & ~self.mask).sum())} outside the written block); "
                                 f"first at {at}: got {float(g[i])}, want {float(self.exp[i])}")


def _tag(c):
    return f"{c.kernel} {c.M}x{c.N}x{c.K} {c.epi} splits={c.splits} alpha={c.alpha}{' strided' if c.strided else ''}{' gm=' + str(c.gm) if c.gm else ''}"


def _prepare(c, dev):
    """buffers, expected contents and the argument list of one case -> go(tag): launch into fresh sentinel-filled outputs and hold them to the reference"""
    from audio_flamingo_amd import _lib

    ops = _ops()
    st = ops._stream()
    M, N, K, form = c.M, c.N, c.K, c.form
    ref = R.reference(c, dev)
    pad = 8 if c.strided else 0
    A = _rows(c.a.T if form == "tn" else c.a, dev, pad, pad)             # NT / NN: [M, K]; TN: [K, M], reduction-major
    B = _rows(c.b if form == "nt" else c.b.T, dev, pad, pad)             # NT: [N, K]; NN / TN: [K, N]
    f32 = bool(c.flags & R.GEMM_OUT_F32)
    cols = 2 * N if c.epi == "swiglu_bwd" else N
    # the output: rows 1 .. M of [M + 2, ld], columns off .. off + cols.  "narrow" / "f32_half": C 8- / 16-byte aligned only, which takes the launch off the 16-byte form
    off = (8 if c.strided else 0) + (4 if c.epi in ("narrow", "f32_half") else 0)
    ld = cols + (16 if c.strided else 0) + (8 if c.epi in ("narrow", "f32_half") else 0)
    block = (slice(1, 1 + M), slice(off, off + cols))
    odt = F32 if f32 else BF
    bias = _vec(c.bias, dev) if c.bias is not None else None
    res = None
    if c.res is not None:
        rp = 8 if (c.strided or c.epi == "residual") else 0             # ldr larger than the extent
        res = _rows(c.res[:c.res_mod] if c.res_mod else c.res[:M], dev, rp, rp, vec=8 if N % 8 == 0 else 4)   # N % 8 = 4: the 8-byte form anyway
    if c.gu is not None:
        res = _rows(c.gu, dev, pad, pad)
    ldr = res.stride(0) if res is not None else 0
    base = c.base.to(dev) if c.base is not None else None
    with_ws = c.splits > 1 or c.kernel == "gemv"
    ta, tb = int(form == "tn"), int(form != "nt")
    keep = [A, B, bias, res]
    rope = None
    if c.epi.startswith("rope"):
        cos, sin = _vec(c.cos, dev), _vec(c.sin, dev)
        pos = c.pos.to(dev).to(torch.int32).contiguous() if c.pos is not None else None
        cl, sl = (None, None) if pos is not None else (ops._rope_lanes(cos, c.S, R.HEAD, 1), ops._rope_lanes(sin, c.S, R.HEAD, 1))
        rope = (cos, sin, pos, cl, sl)
        keep.append(rope)
        assert N % 256 == 0 and c.rope_cols % 256 == 0 and c.S % 32 == 0 and cos.shape == (R.P_TABLE, R.HEAD) and (pos is None or int(pos.max()) < R.P_TABLE)
    # what the guards of gemm_impl ask of the buffers
    assert A.stride(0) % 8 == 0 and B.stride(0) % 8 == 0 and ld % 4 == 0 and ldr % 4 == 0 and (c.epi != "swiglu_bwd" or ld >= 2 * N)

    want_out = Want((M + 2, ld), dev)
    if c.epi == "gelu":
        act = NR.gelu_ref(ref["preact"].cpu())          # _norm_ref is evaluated on the CPU, as tests/test_activations_gpu.py evaluates it
        want_out.put(block, act.y.to(dev))
    else:
        want_out.put(block, ref["out"])
    want_pre = Want((M + 2, ld), dev).put(block, ref["preact"]) if c.epi == "gelu" else None
    if c.epi == "swiglu_fwd":
        I = N // 2
        sw = NR.swiglu_fwd_ref(ref["out"].cpu())
        # the bound's model of the sigmoid (a relative error of __expf) ends where fp32 exp(-g) overflows, g <= -88: there sigmoid_f is 1 / (1 + inf) = 0 and
        # h = 0, where the exact |silu| is still 90 e^-90 ~ 7e-38 (above the smallest normal, so TINY does not cover it): anything from 0 to the exact value
        h_bound = torch.where(ref["out"][:, :I].cpu() <= -88, sw.h.abs() + sw.h_bound, sw.h_bound).to(dev)
        want_h = Want((M + 2, I), dev).put((slice(1, 1 + M), slice(None)), sw.h.to(dev))
    if with_ws:
        want_ws = Want((c.splits * M * N + WS_TAIL,), dev).put(slice(0, c.splits * M * N), ref["ws"].reshape(-1))

    def go(tag):
        buf = _full((M + 2, ld), dev, odt)
        out = buf[block]
        if base is not None:
            out.copy_(base)
        assert out.data_ptr() % 8 == 0 and (not R.is_wide(c)) == (c.N % 8 != 0 or out.data_ptr() % (32 if f32 else 16) != 0), "the buffers do not select the form the case names"
        pre = _full((M + 2, ld), dev) if c.epi == "gelu" else None
        hbuf = _full((M + 2, N // 2), dev) if c.epi == "swiglu_fwd" else None
        second = pre[block].data_ptr() if pre is not None else hbuf[1:1 + M].data_ptr() if hbuf is not None else None
        ws = _full((c.splits * M * N + WS_TAIL,), dev, F32) if with_ws else None
        common = (M, N, K, ops._p(bias), ops._p(res), ldr, c.res_mod, second, c.alpha, c.flags)
        ops.kernel_counts(reset=True)
        if rope is not None:
            cos, sin, pos, cl, sl = rope
            _lib.call("afk_gemm_nt_bf16_rope", A.data_ptr(), A.stride(0), B.data_ptr(), B.stride(0), out.data_ptr(), ld, M, N, K, ops._p(bias), cos.data_ptr(), sin.data_ptr(),
                      ops._p(pos), c.S, c.rope_cols, ops._p(cl), ops._p(sl), st)
        elif form == "nt" and with_ws:
            _lib.call("afk_gemm_nt_bf16_splitk", A.data_ptr(), A.stride(0), B.data_ptr(), B.stride(0), out.data_ptr(), ld, *common, c.splits, ws.data_ptr(), st)
        elif form == "nt":
            _lib.call("afk_gemm_nt_bf16", A.data_ptr(), A.stride(0), B.data_ptr(), B.stride(0), out.data_ptr(), ld, *common, st)
        elif with_ws:
            _lib.call("afk_gemm_bf16_splitk", ta, tb, A.data_ptr(), A.stride(0), B.data_ptr(), B.stride(0), out.data_ptr(), ld, *common, c.splits, ws.data_ptr(), st)
        else:
            _lib.call("afk_gemm_bf16", ta, tb, A.data_ptr(), A.stride(0), B.data_ptr(), B.stride(0), out.data_ptr(), ld, *common, st)
        cnt = ops.kernel_counts()
        expect = {f: int(f == c.family) for f in GEMM_FAMILIES}
        expect.update(gemm_splitk=int(c.splits > 1), gemm_generic_epilogue=int(R.generic(c)))
        assert {k: cnt[k] for k in expect} == expect, f"{tag}: launched {({k: v for k, v in cnt.items() if v})}, expected {({k: v for k, v in expect.items() if v})}"
        if c.epi == "gelu":
            want_pre.hold(f"{tag} preact", pre)
            want_out.hold(f"{tag} gelu", buf, act.y_bound.to(dev))
            assert torch.equal(out, ops.gelu_fwd(pre[block].contiguous())), f"{tag}: the fused GELU differs from gelu_fwd on the preact of the same launch"
        elif c.epi == "swiglu_bwd":
            dh = ref["dh"].to(BF).contiguous()
            assert torch.equal(out, ops.silu_mul_bwd(res.contiguous(), dh)), f"{tag}: differs from silu_mul_bwd(gate|up, exact dh)"
            want_out.hold(f"{tag} guard", buf, NR.swiglu_bwd_ref(res.cpu(), dh.cpu()).dgu_bound.to(dev))
        else:
            want_out.hold(f"{tag} out", buf)
        if c.epi == "swiglu_fwd":
            want_h.hold(f"{tag} h", hbuf, h_bound)
            assert torch.equal(hbuf[1:1 + M], ops.silu_mul_fwd(out.contiguous())), f"{tag}: h differs from silu_mul on the gate|up output of the same launch"
        if with_ws:
            want_ws.hold(f"{tag} split-K workspace", ws)
        EXACT[c.family] += 1
    go.keep = keep
    return go


def _run_group(dev, group):
    ops = _ops()
    cases = [c for c in R.grid() if c.group == group]
    assert cases
    for c in cases:
        go = _prepare(c, dev)
        shapes = ops.gemm_mfma_shapes(c.form) if c.kernel.endswith("256") else (0,)
        assert shapes
        for shape in shapes:
            with _forced(ops, variant={"nt128": 1, "nt256": 2}.get(c.kernel, 0), mfma=shape, gm=c.gm):
                go(f"{_tag(c)} mfma {shape}")


# ------------------------------------------------------------------------------------------------ the K loops at every tile edge
@pytest.mark.parametrize("group", ["nt128", "nt256", "nn256", "tn256"])
def test_shapes_equal_the_integer_reference(dev, group):
    """one, two, three, four, five and twenty K tiles (K = 4160 on the 256x256 NT kernel: 65) under full tiles, ragged tiles in M and N, one 8-row / 8-column tile,
    N % 8 = 4 (the 8-byte epilogue); TN: reduction lengths 8 .. 1288 that end inside a K tile, odd ones included (the in-kernel mask of the last tile)"""
    _run_group(dev, group)


@pytest.mark.parametrize("group", ["nt128_splitk", "nn256_splitk", "tn256_splitk"])
def test_splitk_equals_the_integer_reference(dev, group):
    """afk_gemm_nt_bf16_splitk / afk_gemm_bf16_splitk on a workspace the test owns: 2, 3, 16 and as many splits as K tiles, a last split of another length, a ragged
    last tile inside the last split, bias and accumulate in the fold kernel, its grid-stride loop (1544 x 1360); the fp32 partials are the per-split integer sums
    and the floats behind splits * M * N keep the sentinel"""
    _run_group(dev, group)


def test_gemv_equals_the_integer_reference(dev):
    """M = 1 with a workspace: gemv_nt_bf16_kernel, every split count 1 .. ceil(K / 512), N = 32 .. 1000 (a last workgroup with idle waves, a last wave with idle
    rows), bias + residual in the fold kernel"""
    _run_group(dev, "gemv")


# ------------------------------------------------------------------------------------------------ epilogues
@pytest.mark.parametrize("kernel", ["nt128", "nt256", "nn256", "tn256"])
def test_epilogues_equal_the_integer_reference(dev, kernel):
    """bias, residual (ldr larger than the extent), bias + residual, the residual table of 96 rows under M = 300 (TN: 304; the last block of rows is ragged) and
    M = 96, bias + GELU with preact_out, an fp32 C 32-byte aligned and 16- but not 32-byte aligned, bf16 and fp32 accumulate, alpha = 0.5 / 2 / -1, the
    runtime-flag instantiations of test_gemm_generic_epilogue_instantiations, the SwiGLU backward"""
    _run_group(dev, "epilogues_" + kernel)


def test_swiglu_forward_equals_the_integer_reference(dev):
    """AFK_GEMM_SWIGLU_FWD (256x256 NT kernel only): N = 2 I with one and two tiles of 128 gate + 128 up rows, 8 .. 300 rows, K = 64 .. 1280; gate|up exact, h
    (contiguous [M, I] inside a buffer with guard rows) as the module docstring says"""
    _run_group(dev, "swiglu_fwd")


def test_rope_equals_the_integer_reference(dev):
    """afk_gemm_nt_bf16_rope called directly (ops.gemm_nt_rope fuses from 192 tiles up): the lane-major tables and explicit positions, with and without a bias,
    M not a multiple of S, on {-1, 0, 1} tables: two rotated heads in the first tile, two untouched ones in the second"""
    _run_group(dev, "rope")


def test_tile_map_every_tile_once(dev):
    """6 x 3 tiles of 128 (18 workgroups: nwg % 8 = 2, ntm % 4 = 2) and 6 x 4 tiles of 256 under the default group height and 1, 3, 8, accumulating onto an integer
    base: a tile computed twice shows as well as one left out"""
    _run_group(dev, "tile_map")


# ------------------------------------------------------------------------------------------------ a problem smaller than its operands
def test_problem_smaller_than_the_operands(dev):
    """ops.gemm_nt(a, b, out, M=, N=, K=) on operands and an output larger than the problem: the extra rows and the k columns behind K hold +-1 and would change
    the result if a kernel read them; out keeps the sentinel outside [M, N]"""
    ops = _ops()
    for c in (c for c in R.grid() if c.group == "sub"):
        M, N, K = c.M, c.N, c.K
        g = torch.Generator().manual_seed(c.seed)
        big = lambda t, rows: torch.cat([torch.cat([t, R._signs((t.shape[0], 64), g).to(F64)], 1), R._signs((rows, K + 64), g).to(F64)], 0)
        A, B = _rows(big(c.a, 3), dev, 8 if c.strided else 0, 8 if c.strided else 0), _rows(big(c.b, 5), dev)
        bias = _vec(c.bias, dev) if c.bias is not None else None
        want = Want((M + 2, N + 8), dev).put((slice(0, M), slice(0, N)), R.reference(c, dev)["out"])
        for shape in (ops.gemm_mfma_shapes("nt") if c.kernel == "nt256" else (0,)):
            with _forced(ops, variant=1 if c.kernel == "nt128" else 2, mfma=shape):
                out = _full((M + 2, N + 8), dev)
                ops.kernel_counts(reset=True)
                ops.gemm_nt(A, B, out, bias=bias, M=M, N=N, K=K)
                assert ops.kernel_counts()[c.family] == 1
                want.hold(f"{_tag(c)} inside larger operands, mfma {shape}", out)
                EXACT[c.family] += 1


# ------------------------------------------------------------------------------------------------ what gemm_impl refuses
def test_refused_shapes(dev):
    """the nearest shapes gemm_impl does not take: refused with an AfkError, and the output left untouched"""
    from audio_flamingo_amd import _lib

    ops = _ops()
    for kernel, M, N, K, splits, what in R.REFUSED:
        form = R.FORM[kernel]
        up8 = lambda v: v + (-v) % 8                     # what is refused is the shape, not a leading dimension: whole rows of lda / ldb / ldc elements
        a = torch.ones((K, up8(M)) if form == "tn" else (M, up8(K)), device=dev, dtype=BF)
        b = torch.ones((N, up8(K)) if form == "nt" else (K, up8(N)), device=dev, dtype=BF)
        lda, ldb = a.stride(0), b.stride(0)
        out = _full((M, up8(N)), dev)
        ws = torch.zeros(max(splits, 1) * M * N, device=dev, dtype=F32)
        with _forced(ops, variant=1 if kernel == "nt128" else 0):
            with pytest.raises(_lib.AfkError):
                _lib.call("afk_gemm_bf16_splitk", int(form == "tn"), int(form != "nt"), a.data_ptr(), lda, b.data_ptr(), ldb, out.data_ptr(), out.stride(0), M, N, K,
                          None, None, 0, 0, None, 1.0, 0, splits, ws.data_ptr(), ops._stream())
        assert bool((out == SENT).all()), what
    # the SwiGLU forward off its 16-byte form, the RoPE epilogue off the 256x256 kernel
    x, w = torch.ones((8, 64), device=dev, dtype=BF), torch.ones((256, 64), device=dev, dtype=BF)
    gu, h = _full((8, 264), dev), _full((8, 128), dev)
    with pytest.raises(_lib.AfkError):
        _lib.call("afk_gemm_nt_bf16", x.data_ptr(), 64, w.data_ptr(), 64, gu[:, 4:].data_ptr(), 264, 8, 256, 64, None, None, 0, 0, h.data_ptr(), 1.0, R.GEMM_SWIGLU_FWD, ops._stream())
    cs = torch.ones((R.P_TABLE, R.HEAD), device=dev, dtype=BF)
    with _forced(ops, variant=1):
        with pytest.raises(_lib.AfkError):
            _lib.call("afk_gemm_nt_bf16_rope", x.data_ptr(), 64, w.data_ptr(), 64, gu.data_ptr(), 264, 8, 256, 64, None, cs.data_ptr(), cs.data_ptr(), None, 32, 256, None, None,
                      ops._stream())
    assert bool((gu == SENT).all()) and bool((h == SENT).all())

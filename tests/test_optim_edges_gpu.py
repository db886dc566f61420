"""The kernels that end the default training step, at their edges on MI355X: AdamW with fp32 master and moments (afk_adamw_step, afk_adamw_step_t),
the bf16-state kernels at the lengths their own suite leaves out, the gradient sum of squares (afk_sumsq_bf16), the clip coefficient (afk_clip_coef)
and afk_set_f32.  Every result is held per element to the float64 reference and the derived bar of tests/_optim_ref.py (the bf16-state kernels to the
bar of tests/_adamw16_ref.py, unchanged), or bit for bit to a sibling launch that must compute the same thing.  Every buffer a launch may write is
an inner slice of a sentinel-filled buffer, and everything outside the slice must keep the sentinel bit for bit.  The worst ratios each test measures
are printed as one JSON line; those of the first full run are on record in profiles/optim_edges.md.

Left out: the 16 384-block cap of the transposed launches, which needs a weight of more than 67 M elements (several GB of state); max_blocks drives
the same tile-stride loop and is covered."""
import json

import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import _adamw16_ref as R16
from tests import _optim_ref as R

BF = torch.bfloat16
F32 = torch.float32
FILL = -3.0   # the sentinel: exact in bf16 and fp32, and nothing the updates produce by accident

A_NS = [1, 2, 3, 4, 5, 7, 1023, 1024, 1025, 4 * 256 * 3 + 1, 4 * 4096 * 256 + 4 * 3 + 3]   # the last: three vectors and a tail past the 4096-block cap
A_CASES = [(n, 0) for n in A_NS] + [(n, h) for h in (1, 2) for n in (1025, 4 * 256 * 3 + 1)]
T_SHAPES = [(64, 64), (64, 192), (192, 64), (128, 256)]
C_NS = [1, 7, 8, 9, 2047, 2049, 8 * 4096 * 256 + 8 * 3 + 5]
D_NS = [1, 7, 8, 9, 2047, 2048, 2049, 8 * 256 * 1024 - 8, 8 * 256 * 1024, 8 * 256 * 1024 + 8, 2 * 8 * 256 * 1024 + 13]
HP16 = dict(lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.01)
HYPER = [3e-3, 0.5, 0.25, 0.37]   # lr, 1 - beta1^t, sqrt(1 - beta2^t), multiplier: all unlike the scalar arguments of any step here


def _ops():
    from audio_flamingo_amd import ops

    return ops


def _afk_error():
    from audio_flamingo_amd._lib import AfkError

    return AfkError


def _bits(t):
    return t.view({2: torch.int16, 4: torch.int32}[t.element_size()])


class Guarded:
    """a copy of `src` as the slice [off, off + n) of a sentinel-filled buffer"""

    def __init__(self, src, off, pad=16):
        self.off, self.n = off, src.numel()
        self.buf = torch.full((off + self.n + pad,), FILL, dtype=src.dtype, device=src.device)
        self.t = self.buf[off: off + self.n]
        self.t.copy_(src.reshape(-1))
        self.fill = int(_bits(torch.full((1,), FILL, dtype=src.dtype))[0])

    def intact(self):
        b = _bits(self.buf)
        return bool((b[:self.off] == self.fill).all()) and bool((b[self.off + self.n:] == self.fill).all())


class Streams:
    """the five streams of an fp32-state launch (or the four of a bf16-state one: master=None), each guarded; `offs` = element offsets of the slices"""
    NAMES = ("master", "m", "v", "grad", "param")

    def __init__(self, master, m, v, grad, param, offs=(4, 4, 4, 4, 4)):
        for name, src, off in zip(self.NAMES, (master, m, v, grad, param), offs):
            setattr(self, name, None if src is None else Guarded(src, off))

    def items(self):
        return [(k, getattr(self, k)) for k in self.NAMES if getattr(self, k) is not None]

    def snapshot(self):
        return {k: g.buf.clone() for k, g in self.items()}

    def assert_guards(self, what):
        for k, g in self.items():
            assert g.intact(), f"{what}: the launch wrote outside its slice of {k}"

    def assert_same(self, other, what):
        for k, g in self.items():
            assert torch.equal(_bits(g.t), _bits(getattr(other, k).t)), f"{what}: {k} differs"

    def assert_untouched(self, snap, what):
        for k, g in self.items():
            assert torch.equal(_bits(g.buf), _bits(snap[k])), f"{what}: {k} was written"


def _gate(dev, v):
    return torch.full((1,), v, device=dev, dtype=torch.int32)


def _check32(S, before, g, what, **kw):
    """the fp32-state result in S against float64 from `before` = (w0, m0, v0) -> worst ratios; the bf16 parameter is the rounded master"""
    ref = R.ref64(*before, g, **kw)
    out = {k: R.worst_ratio(x.t, *ref[k]) for k, x in (("w", S.master), ("m", S.m), ("v", S.v))}
    assert torch.equal(_bits(S.param.t), _bits(S.master.t.to(BF))), f"{what}: param != master.to(bfloat16)"
    S.assert_guards(what)
    return out


def _step32(ops, S, **kw):
    ops.adamw_step(S.master.t, S.m.t, S.v.t, S.grad.t, S.param.t, **kw)


# ------------------------------------------------------------------------------------------------ A. flat fp32 AdamW
@pytest.mark.parametrize("n,hset", A_CASES)
def test_adamw32_flat_against_fp64(dev, n, hset):
    """ops.adamw_step on slices that start 4 elements into their buffers (16 bytes for the fp32 streams, 8 for the bf16 ones: the weakest alignment
    the C ABI admits, and what ShardedAdamW may hand it).  Steps 1, 2, 3, 4 and 1000, each from the kernel's own previous state, against float64
    computed from that state: worst |x - X| / tolerance <= 1 for master, m and v, param == master.to(bfloat16), a zero gradient on zero moments keeps
    them exactly zero.  Then one launch each from the same cloned state: max_blocks 1 and 3 and an open gate bit-equal to the plain launch, a closed
    gate leaves all five buffers alone, grad_scale = 0.37 and device hyper-parameters (with grad_scale = 0.5 beside them) against float64.  Refused
    with nothing written: a master or a gradient offset by one element, step = 0."""
    ops, AfkError = _ops(), _afk_error()
    hp = R.HYPER_SETS[hset]
    w, m, v = R.make_state(n, dev, seed=n % 89)
    S = Streams(w, m, v, torch.zeros(n, device=dev, dtype=BF), w.to(BF))
    worst = {"w": 0.0, "m": 0.0, "v": 0.0}
    for step in R.STEPS:
        g = R.make_grad(n, step, dev, seed=n % 89)
        S.grad.t.copy_(g)
        before = (S.master.t.clone(), S.m.t.clone(), S.v.t.clone())
        _step32(ops, S, step=step, **hp)
        r = _check32(S, before, g, f"n={n} step {step}", step=step, **hp)
        worst = {k: max(worst[k], r[k]) for k in worst}
        still = (g.float() == 0) & (before[1] == 0) & (before[2] == 0)
        if step <= 2:
            assert bool(still[0]), "the walk must hold a zero gradient on zero moments"
        assert not bool((S.m.t[still] != 0).any()) and not bool((S.v.t[still] != 0).any()), f"step {step}: zero gradient on zero moments must stay exactly zero"
    rec = {"n": n, "hyper": hp, "steps": R.STEPS, "worst_error_over_tolerance": worst}
    assert all(x <= 1.0 for x in worst.values()), rec

    # ---- one launch each from the same state
    step = 5
    g = R.make_grad(n, step, dev, seed=n % 89)
    state = (S.master.t.clone(), S.m.t.clone(), S.v.t.clone())
    p0 = S.param.t.clone()
    fresh = lambda: Streams(*state, g, p0)
    base = fresh()
    _step32(ops, base, step=step, **hp)
    rec["plain_step_5"] = _check32(base, state, g, f"n={n} step 5", step=step, **hp)
    for label, kw in (("max_blocks=1", dict(max_blocks=1)), ("max_blocks=3", dict(max_blocks=3)), ("open gate", dict(gate=_gate(dev, 1)))):
        X = fresh()
        _step32(ops, X, step=step, **hp, **kw)
        X.assert_same(base, f"n={n} {label} against the plain launch")
        X.assert_guards(label)
    X = fresh()
    snap = X.snapshot()
    _step32(ops, X, step=step, gate=_gate(dev, 0), **hp)
    torch.cuda.synchronize()
    X.assert_untouched(snap, f"n={n} closed gate")
    X = fresh()
    _step32(ops, X, step=step, grad_scale=0.37, **hp)
    rec["grad_scale_0.37"] = _check32(X, state, g, f"n={n} grad_scale", step=step, grad_scale=0.37, **hp)
    hyper = torch.tensor(HYPER, device=dev, dtype=F32)
    H = fresh()
    _step32(ops, H, step=step, grad_scale=0.5, hyper=hyper, **hp)
    rec["device_hyper"] = _check32(H, state, g, f"n={n} hyper", step=step, grad_scale=0.5, hyper=hyper, **hp)
    if n > 7:   # (a handful of elements can all hold a zero gradient)
        assert not torch.equal(H.master.t, X.master.t) and not torch.equal(X.master.t, base.master.t)
    print("optim_edges adamw32_flat", json.dumps(rec))
    for k in ("plain_step_5", "grad_scale_0.37", "device_hyper"):
        assert all(x <= 1.0 for x in rec[k].values()), (k, rec)

    # ---- refused, nothing written
    del base, H
    for label, offs, st in (("master offset by one element", (5, 4, 4, 4, 4), step), ("grad offset by one element", (4, 4, 4, 5, 4), step),
                            ("step = 0", (4, 4, 4, 4, 4), 0)):
        X = Streams(*state, g, p0, offs=offs)
        snap = X.snapshot()
        with pytest.raises(AfkError):
            _step32(ops, X, step=st, **hp)
        torch.cuda.synchronize()
        X.assert_untouched(snap, f"n={n} refused ({label})")


# ------------------------------------------------------------------------------------------------ B. transposed-shadow fp32 AdamW
class Shadow:
    """[K, ld] shadow as an inner slice (8 elements in: 16 bytes) of a sentinel-filled buffer with two spare rows behind it"""

    def __init__(self, K, ld, dev, off=8):
        self.K, self.ld, self.off = K, ld, off
        self.buf = torch.full((off + (K + 2) * ld + 8,), FILL, device=dev, dtype=BF)
        self.t = self.buf[off: off + K * ld].view(K, ld)
        self.fill = int(_bits(torch.full((1,), FILL, dtype=BF))[0])

    def check(self, param, N, what):
        assert torch.equal(_bits(self.t[:, :N]), _bits(param.view(N, self.K).t())), f"{what}: shadow != transpose(param)"
        b = _bits(self.buf)
        assert bool((_bits(self.t)[:, N:] == self.fill).all()), f"{what}: shadow columns >= N were written"
        assert bool((b[:self.off] == self.fill).all()) and bool((b[self.off + self.K * self.ld:] == self.fill).all()), f"{what}: shadow rows >= K (or the bytes before it) were written"

    def untouched(self):
        return bool((_bits(self.buf) == self.fill).all())


def _t_state(N, K, dev, seed):
    n = N * K
    w = R.make_state(n, dev, seed=seed)[0]
    m = R.make_grad(n, 11, dev, seed=seed).float() * 0.5
    v = R.make_grad(n, 12, dev, seed=seed).float() ** 2
    return w, m, v, R.make_grad(n, 13, dev, seed=seed)


T_OFFS = (4, 4, 4, 8, 8)   # the transposed launches need 16 bytes on every stream


@pytest.mark.parametrize("N,K", T_SHAPES)
def test_adamw32_transposed_equals_flat(dev, N, K):
    """ops.adamw_step_t on one [N, K] weight - a single tile, a row of tiles, a column of tiles, 2 x 4 tiles - with ld_shadow = N, N + 8, N + 64 and a full,
    a one-block and a five-block grid: master / m / v / param bit-identical to the flat launch of the same step, shadow[:, :N] == param.view(N, K).t(),
    shadow columns >= N and rows >= K keep the sentinel.  Closed gate: nothing written, the shadow included; open gate and device hyper-parameters:
    bit-identical to the flat launch with the same arguments."""
    ops = _ops()
    hp, step = R.HYPER_SETS[0], 4
    w, m, v, g = _t_state(N, K, dev, seed=N + K)
    p0 = w.to(BF)
    flat = Streams(w, m, v, g, p0, offs=T_OFFS)
    _step32(ops, flat, step=step, **hp)
    r = _check32(flat, (w, m, v), g, f"[{N}, {K}] flat", step=step, **hp)
    assert all(x <= 1.0 for x in r.values()), r
    hyper = torch.tensor(HYPER, device=dev, dtype=F32)
    flat_h = Streams(w, m, v, g, p0, offs=T_OFFS)
    _step32(ops, flat_h, step=step, grad_scale=0.5, hyper=hyper, **hp)

    def launch(ld, **kw):
        X, sh = Streams(w, m, v, g, p0, offs=T_OFFS), Shadow(K, ld, dev)
        snap = X.snapshot()
        ops.adamw_step_t(X.master.t, X.m.t, X.v.t, X.grad.t, X.param.t, sh.t, N, K, step=step, **hp, **kw)
        return X, sh, snap

    for ld in (N, N + 8, N + 64):
        for mb in (0, 1, 5):
            what = f"[{N}, {K}] ld_shadow={ld} max_blocks={mb}"
            X, sh, _ = launch(ld, max_blocks=mb)
            X.assert_same(flat, what + " against the flat launch")
            X.assert_guards(what)
            sh.check(X.param.t, N, what)
        X, sh, snap = launch(ld, max_blocks=5, gate=_gate(dev, 0))
        torch.cuda.synchronize()
        X.assert_untouched(snap, f"[{N}, {K}] ld_shadow={ld} closed gate")
        assert sh.untouched(), "a closed gate must leave the shadow alone"
        X, sh, _ = launch(ld, gate=_gate(dev, 1))
        X.assert_same(flat, f"[{N}, {K}] ld_shadow={ld} open gate")
        sh.check(X.param.t, N, "open gate")
        for mb in (0, 1):
            X, sh, _ = launch(ld, max_blocks=mb, grad_scale=0.5, hyper=hyper)
            X.assert_same(flat_h, f"[{N}, {K}] ld_shadow={ld} max_blocks={mb} device hyper")
            sh.check(X.param.t, N, "device hyper")
    assert not torch.equal(flat.master.t, flat_h.master.t) and not torch.equal(flat.master.t, w)
    print("optim_edges adamw32_transposed", json.dumps({"N": N, "K": K, "flat_worst_error_over_tolerance": r, "transposed": "bit-identical"}))


def _refused_t_cases(dev):
    """(label, N, K, shadow tensor, the buffer behind it)"""
    def sh(K, ld, off=8):
        buf = torch.full((off + (K + 2) * ld + 8,), FILL, device=dev, dtype=BF)
        return buf[off: off + K * ld].view(K, ld), buf

    return [("N = 96", 96, 64, *sh(64, 96)), ("K = 32", 64, 32, *sh(32, 64)), ("ld_shadow = N - 8", 64, 64, *sh(64, 56)),
            ("ld_shadow = N + 4", 64, 64, *sh(64, 68)), ("shadow offset by 4 elements", 64, 64, *sh(64, 64, off=4))]


@pytest.mark.parametrize("state16", [False, True], ids=["fp32-state", "bf16-state"])
def test_transposed_launches_refuse_bad_shapes(dev, state16):
    """N = 96, K = 32, ld_shadow = N - 8, ld_shadow = N + 4 and a shadow 8 bytes off: AfkError, and neither a stream nor the shadow buffer is written"""
    ops, AfkError = _ops(), _afk_error()
    for label, N, K, shadow, buf in _refused_t_cases(dev):
        w, m, v, g = _t_state(N, K, dev, seed=3)
        X = Streams(None, m.to(BF), v.to(BF), g, w.to(BF), offs=(8, 8, 8, 8, 8)) if state16 else Streams(w, m, v, g, w.to(BF), offs=T_OFFS)
        snap = X.snapshot()
        with pytest.raises(AfkError):
            if state16:
                ops.adamw16_step_t(X.m.t, X.v.t, X.grad.t, X.param.t, shadow, N, K, step=2, **HP16)
            else:
                ops.adamw_step_t(X.master.t, X.m.t, X.v.t, X.grad.t, X.param.t, shadow, N, K, step=2, **R.HYPER_SETS[0])
        torch.cuda.synchronize()
        X.assert_untouched(snap, label)
        assert bool((buf == FILL).all()), f"{label}: the refused launch wrote the shadow"


# ------------------------------------------------------------------------------------------------ C. bf16-state edges
def _check16(S, before, g, what, **kw):
    ref = R16.ref64(*before, g, **kw)
    out = {k: R16.worst_ratio(x.t, *ref[k]) for k, x in (("p", S.param), ("m", S.m), ("v", S.v))}
    S.assert_guards(what)
    return out


@pytest.mark.parametrize("n", C_NS)
def test_adamw16_flat_edges(dev, n):
    """ops.adamw16_step below one vector, round the first block boundary and past the 4096-block cap (three vectors and a tail behind it), two steps from
    the kernel's own state, against the float64 reference and the bar of tests/_adamw16_ref.py; a thin grid is bit-equal"""
    ops = _ops()
    p = R16.make_params(n, dev, seed=n % 97)
    z = torch.zeros(n, device=dev, dtype=BF)
    S = Streams(None, z, z, z, p, offs=(8, 8, 8, 8, 8))
    worst = {"p": 0.0, "m": 0.0, "v": 0.0}
    for step in (1, 2):
        g = R16.make_grad(n, step, dev, seed=n % 97)
        S.grad.t.copy_(g)
        before = (S.param.t.clone(), S.m.t.clone(), S.v.t.clone())
        thin = Streams(None, before[1], before[2], g, before[0], offs=(8, 8, 8, 8, 8))
        ops.adamw16_step(S.m.t, S.v.t, S.grad.t, S.param.t, step=step, **HP16)
        ops.adamw16_step(thin.m.t, thin.v.t, thin.grad.t, thin.param.t, step=step, max_blocks=3, **HP16)
        bc1, bc2s = R16.bias_corrections(HP16["beta1"], HP16["beta2"], step)
        r = _check16(S, before, g, f"adamw16 n={n} step {step}", bc1=bc1, bc2_sqrt=bc2s, **HP16)
        worst = {k: max(worst[k], r[k]) for k in worst}
        thin.assert_same(S, f"adamw16 n={n} step {step} max_blocks=3")
        thin.assert_guards("max_blocks=3")
    print("optim_edges adamw16_flat", json.dumps({"n": n, "steps": [1, 2], "worst_error_over_tolerance": worst}))
    assert all(x <= 1.0 for x in worst.values()), worst
    assert not torch.equal(S.param.t, p) or n < 8


@pytest.mark.parametrize("N,K", T_SHAPES)
def test_adamw16_transposed_equals_flat(dev, N, K):
    """ops.adamw16_step_t at the shapes and shadow strides of the fp32 test: p / m / v bit-identical to the flat launch, shadow == transpose(param), the
    sentinel kept round it"""
    ops = _ops()
    n, seed, step = N * K, N + K + 1, 2
    offs = (8, 8, 8, 8, 8)
    z = torch.zeros(n, device=dev, dtype=BF)
    first = Streams(None, z, z, R16.make_grad(n, 1, dev, seed=seed), R16.make_params(n, dev, seed=seed), offs=offs)   # moments of a real first step
    ops.adamw16_step(first.m.t, first.v.t, first.grad.t, first.param.t, step=1, **HP16)
    p0, m0, v0, g = first.param.t.clone(), first.m.t.clone(), first.v.t.clone(), R16.make_grad(n, step, dev, seed=seed)
    flat = Streams(None, m0, v0, g, p0, offs=offs)
    ops.adamw16_step(flat.m.t, flat.v.t, flat.grad.t, flat.param.t, step=step, **HP16)
    bc1, bc2s = R16.bias_corrections(HP16["beta1"], HP16["beta2"], step)
    r = _check16(flat, (p0, m0, v0), g, f"adamw16 [{N}, {K}] flat", bc1=bc1, bc2_sqrt=bc2s, **HP16)
    assert all(x <= 1.0 for x in r.values()), r
    for ld in (N, N + 8, N + 64):
        for mb in (0, 1):
            what = f"adamw16 [{N}, {K}] ld_shadow={ld} max_blocks={mb}"
            X, sh = Streams(None, m0, v0, g, p0, offs=offs), Shadow(K, ld, dev)
            ops.adamw16_step_t(X.m.t, X.v.t, X.grad.t, X.param.t, sh.t, N, K, step=step, max_blocks=mb, **HP16)
            X.assert_same(flat, what + " against the flat launch")
            X.assert_guards(what)
            sh.check(X.param.t, N, what)
    assert not torch.equal(flat.param.t, p0)
    print("optim_edges adamw16_transposed", json.dumps({"N": N, "K": K, "flat_worst_error_over_tolerance": r, "transposed": "bit-identical"}))


# ------------------------------------------------------------------------------------------------ D. sum of squares
WS_SENTINEL = -12345.0


def _sumsq(ops, x, acc, ws=None, **kw):
    """-> the grid the call must have used; ws[grid:] must keep its sentinel"""
    ws = torch.full((R.SUMSQ_BLOCKS + 8,), WS_SENTINEL, device=x.device, dtype=F32) if ws is None else ws
    ops.sumsq_(x, acc, ws=ws, **kw)
    grid = R.sumsq_grid(x.numel())
    assert bool((ws[grid:] == WS_SENTINEL).all()), f"n={x.numel()}: the workspace was written behind its {grid} partial sums"
    return ws


@pytest.mark.parametrize("n", D_NS)
def test_sumsq_edges(dev, n):
    """ops.sumsq_ at lengths below one vector, round a block boundary, round the 1024-block cap and two strides past it: all-ones input gives exactly n
    (and n + 5 on a preloaded accumulator), every one-hot probe of tests/_optim_ref.py gives exactly 1, N(0,1) * 10^k data lands inside the derived
    bar and is bit-equal across two runs, a closed gate leaves the accumulator alone and an open one changes nothing; only acc[0] and the first
    `grid` workspace floats are written; an x one element off 16 bytes is refused"""
    ops, AfkError = _ops(), _afk_error()
    assert ops.sumsq_workspace_floats() == R.SUMSQ_BLOCKS
    X = Guarded(torch.ones(n, device=dev, dtype=BF), 8)
    acc = Guarded(torch.tensor([0.0, 5.0], device=dev), 4)
    _sumsq(ops, X.t, acc.t[0:1])
    _sumsq(ops, X.t, acc.t[1:2])
    assert acc.t.tolist() == [float(n), float(n + 5)], (n, acc.t.tolist())
    assert acc.intact() and X.intact()

    probes = R.sumsq_probes(n)
    X.t.zero_()
    hits = Guarded(torch.zeros(len(probes), device=dev), 4)
    for j, i in enumerate(probes):
        X.t[i] = 1.0
        _sumsq(ops, X.t, hits.t[j: j + 1])
        X.t[i] = 0.0
    missed = [i for i, hit in zip(probes, hits.t.tolist()) if hit != 1.0]
    assert not missed, f"n={n}: one-hot elements {missed} are not counted exactly once: {hits.t.tolist()}"
    assert hits.intact()

    gen = torch.Generator(device="cpu").manual_seed(n)
    data = (torch.randn(n, generator=gen) * 10.0 ** torch.randint(-2, 2, (n,), generator=gen).float()).to(BF).to(dev)
    X.t.copy_(data)
    ref, tol = R.sumsq_ref(data)
    out = Guarded(torch.zeros(4, device=dev), 4)
    _sumsq(ops, X.t, out.t[0:1])
    _sumsq(ops, X.t, out.t[1:2])
    _sumsq(ops, X.t, out.t[2:3], gate=_gate(dev, 1))
    out.t[3] = 7.5
    _sumsq(ops, X.t, out.t[3:4], gate=_gate(dev, 0))
    a, b, c, d = out.t.tolist()
    ratio = abs(a - ref) / tol
    print("optim_edges sumsq", json.dumps({"n": n, "grid": R.sumsq_grid(n), "terms_per_thread": R.sumsq_terms_per_thread(n), "probes": len(probes),
                                           "error_over_tolerance": ratio, "relative_error": abs(a - ref) / ref}))
    assert ratio <= 1.0, (n, a, ref, tol)
    assert a == b, "the sum of squares is not bit-equal across two runs"
    assert a == c, "an open gate changed the sum"
    assert d == 7.5, "a closed gate must leave the accumulator alone"
    assert out.intact() and X.intact()

    off1 = Guarded(data, 9)   # 18 bytes into the buffer
    before = out.buf.clone()
    with pytest.raises(AfkError):
        ops.sumsq_(off1.t, out.t[0:1])
    torch.cuda.synchronize()
    assert torch.equal(_bits(out.buf), _bits(before))


# ------------------------------------------------------------------------------------------------ E. clip coefficient, set_f32
@pytest.mark.parametrize("slots", [1, 2, 5])
def test_clip_coef_edges(dev, slots):
    """ops.clip_coef_ over 1, 2 and 5 slots with NaN behind them: norm below, above and far above max_norm, scale 0.5 and 1/3, with and without norm_out,
    against float64 at 4u relative; the coefficient is exactly 1 below max_norm; only coef[0] and norm_out[0] are written"""
    ops = _ops()
    gen = torch.Generator(device="cpu").manual_seed(slots)
    worst = {"norm": 0.0, "coef": 0.0}
    for scale in (0.5, 1.0 / 3.0):
        for target in (0.3, 2.7, 4.0e4):   # the norm to aim at; max_norm = 1
            parts = torch.rand(slots, generator=gen) + 0.1
            parts = (parts / parts.sum() * (target / scale) ** 2).to(F32)
            buf = torch.full((slots + 3,), float("nan"), device=dev, dtype=F32)
            buf[:slots] = parts.to(dev)
            for with_norm in (True, False):
                coef, norm = Guarded(torch.full((1,), 9.0, device=dev), 4), Guarded(torch.full((1,), 9.0, device=dev), 4)
                ops.clip_coef_(buf[:slots], coef.t, max_norm=1.0, scale=scale, norm_out=norm.t if with_norm else None)
                got_n, got_c = norm.t.item(), coef.t.item()
                assert coef.intact() and norm.intact() and (with_norm or got_n == 9.0)
                rn, rc = R.clip_coef_check(got_n if with_norm else None, got_c, parts, scale, 1.0)
                assert (got_c == 1.0) == (target < 1.0), (target, got_c)
                worst = {"norm": max(worst["norm"], rn or 0.0), "coef": max(worst["coef"], rc)}
    print("optim_edges clip_coef", json.dumps({"slots": slots, "worst_error_over_4u": worst}))
    assert worst["norm"] <= 1.0 and worst["coef"] <= 1.0, worst


def test_clip_coef_exact_case(dev):
    """sumsq = [4, 12], scale = 0.5: the norm is exactly 2"""
    ops = _ops()
    buf = torch.tensor([4.0, 12.0, float("nan")], device=dev)
    coef, norm = torch.zeros(1, device=dev), torch.zeros(1, device=dev)
    ops.clip_coef_(buf[:2], coef, max_norm=1.0, scale=0.5, norm_out=norm)
    assert norm.item() == 2.0
    _, rc = R.clip_coef_check(2.0, coef.item(), buf[:2], 0.5, 1.0)
    assert rc <= 1.0, (coef.item(), rc)
    ops.clip_coef_(buf[:2], coef, max_norm=2.5, scale=0.5)
    assert coef.item() == 1.0


def test_set_f32_edges(dev):
    """ops.set_f32 writes exactly the 1..4 floats it is given into the head of its destination, bit-equal to torch's fp32 rounding of them, and nothing
    else of a sentinel-filled 8-float buffer; 0 and 5 values are refused with nothing written"""
    ops, AfkError = _ops(), _afk_error()
    values = [1e-3, 1.0 - 0.9 ** 7, (1.0 - 0.999 ** 7) ** 0.5, 1.0 / 3.0]
    for k in range(1, 5):
        buf = torch.full((8,), FILL, device=dev, dtype=F32)
        ops.set_f32(buf[2:], values[:k])
        want = torch.full((8,), FILL, dtype=F32)
        want[2: 2 + k] = torch.tensor(values[:k], dtype=F32)
        assert torch.equal(_bits(buf.cpu()), _bits(want)), (k, buf.tolist())
    buf = torch.full((8,), FILL, device=dev, dtype=F32)
    for bad in ([], values + [2.0]):
        with pytest.raises(AfkError):
            ops.set_f32(buf[2:], bad)
    torch.cuda.synchronize()
    assert bool((buf == FILL).all())


# ------------------------------------------------------------------------------------------------ F. negative controls on the kernel
def test_bar_rejects_a_wrong_step_on_the_kernel(dev):
    """the bar has teeth on the device too: the flat kernel called (legally) with step + 1, with weight_decay = 0 against the wd = 0.1 reference, and
    with hyper[3] left at 1 against the reference of a 0.37 multiplier - each must FAIL the bar the correct call passes"""
    ops = _ops()
    hp, n = R.HYPER_SETS[0], 4 * 256 * 3 + 1
    w, m, v = R.make_state(n, dev, seed=1)
    S = Streams(w, m, v, torch.zeros(n, device=dev, dtype=BF), w.to(BF))
    for step in (1, 2):
        S.grad.t.copy_(R.make_grad(n, step, dev, seed=1))
        _step32(ops, S, step=step, **hp)
    step = 3
    g = R.make_grad(n, step, dev, seed=1)
    state, p0 = (S.master.t.clone(), S.m.t.clone(), S.v.t.clone()), S.param.t.clone()
    bc = [hp["lr"], 1.0 - hp["beta1"] ** step, (1.0 - hp["beta2"] ** step) ** 0.5]
    hyper_ref = torch.tensor(bc + [0.37], device=dev, dtype=F32)
    hyper_one = torch.tensor(bc + [1.0], device=dev, dtype=F32)

    def run(ref_kw, **kw):
        X = Streams(*state, g, p0)
        _step32(ops, X, **{**hp, "step": step, **kw})
        ref = R.ref64(*state, g, **{**hp, "step": step, **ref_kw})
        return R.worst_ratio(X.master.t, *ref["w"])

    rec = {"correct": run({}), "correct_with_hyper": run(dict(hyper=hyper_ref), hyper=hyper_ref), "step_plus_1": run({}, step=step + 1),
           "weight_decay_0": run({}, weight_decay=0.0), "hyper3_left_at_1": run(dict(hyper=hyper_ref), hyper=hyper_one)}
    print("optim_edges negative_controls", json.dumps({"n": n, "worst_master_error_over_tolerance": rec}))
    assert rec["correct"] <= 1.0 and rec["correct_with_hyper"] <= 1.0, rec
    assert rec["step_plus_1"] > 1.0 and rec["weight_decay_0"] > 1.0 and rec["hyper3_left_at_1"] > 1.0, rec

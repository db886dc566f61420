"""Float64 references, error bounds, input builders and launch geometry of the kernels between the GEMMs: csrc/norm.hip (LayerNorm / RMSNorm
forward and backward, fold_partials, gelu_bwd_colsum) and the activation / reduction part of csrc/elementwise.hip (GELU, SwiGLU, RoPE, add,
ReLU, colsum, rowsum).  Plain torch, no kernel calls: importable on the CPU (tests/test_norm_ref_cpu.py holds every reference to float64
autograd of the operation it restates).  Every reference takes the bf16 (and, for the backwards, the fp32 mean / rstd) tensors the kernel reads.

BOUNDS - derived here, none measured, no free atol.  A kernel output is bf16(v^) where v^ is the kernel's fp32 value of the exact value v:

    |bf16(v^) - v|  <=  hu(|v| + err32) + err32                                                              (round_bound)

hu - ONE BF16 ROUNDING.  bf16 keeps 8 significant bits, so round-to-nearest moves a value by at most half a unit in the last place:
    hu(v) = 2^-9 * mag2(v),   mag2(v) = the power of two above |v|  (|v| = f * 2^ex, 1/2 <= f < 1: mag2 = 2^ex),
that is between 2^-9 |v| and 2^-8 |v|; it is attained (1 + 2^-8 is a tie), so nothing smaller holds for a correct kernel.  Where the kernel
rounds twice (RMSNorm y = bf16(w * bf16(x rstd)), SwiGLU h = bf16(bf16(silu g) * u), dx = bf16(bf16(norm branch) + dx_add)) the reference
rounds at the same first point, and the kernel's first rounding can only differ from the reference's when the exact value lies within err32
of a bf16 tie - which is known per element:
    flip(v, err32) = one whole unit (2 hu) where hu(v) - |v - bf16(v)| <= err32, else 0.
So away from ties the first rounding point costs nothing against the rounded reference and the bound is the second rounding alone.

err32 - FP32 ARITHMETIC.  e = 2^-24 is fp32's unit roundoff; a sum of n fp32 terms is off by at most gamma(n) * sum|terms|, gamma(n) = n e,
IN ANY ORDER (Higham, Accuracy and Stability, 4.2) - so the bounds do not depend on the wave / block / fold order a kernel picks.  Per op:
    LayerNorm forward   mean:   gamma(D) mean|x| + 2 e |mean|             (D terms in any order; 1 / D and the product.  The first term is 0 where the sum is
                                EXACT in any order - sum_err: small integers, constant rows, the `offset` rows)
                        rstd:   relative  (gamma(D + 6) + err(mean)^2 / (var + eps)) / 2 + 4 e
                                (two-pass: d = x - mean^ [e], d^2 [2 e + e], D terms, 1 / D [2 e], + eps [e]; sum (x - m^)^2 = sum (x - m)^2 + D (m - m^)^2
                                 exactly, so the mean's error enters squared; rsqrtf within 2 ulp = 4 e)
                        y:      |w| rstd err(mean)  +  p (rel(rstd) + 4 e)  +  e (p + |b|),   p = |(x - mean) rstd w|
                                the first term is the statistic's own error carried through: a constant row is nothing else (x - mean^ = -err).
    RMSNorm forward     rstd:   relative  gamma(D + 4) / 2 + 4 e;   xh^ = x rstd^: relative rel(rstd) + e;   w * bf16(xh) is exact in fp32
                                (two 8-bit significands): y is flip(xh) |w| + hu(y) - bit-equal to the reference away from ties.
    backward            g = dy w is exact; xh = (x - mean) rstd from the fp32 statistics the kernel is GIVEN (they are inputs here): relative 2 e;
                        c1 = mean(g): gamma(D + 2) mean|g|;   c2 = mean(g xh): gamma(D + 5) mean|g xh|;
                        v = rstd (g - c1 - xh c2):  rstd (err c1 + |xh| err c2 + |c2| err xh + 8 e (|g| + |c1| + |xh c2|))
                        dx = bf16(v), or bf16(bf16(v) + dx_add): flip(v) + e |T| inside round_bound of T = bf16(v) + dx_add.
                        dw = sum_rows dy xh (LayerNorm: terms relative 3 e; RMSNorm: dy * bf16(xh) exact, flip(xh) |dy| per term), db = sum_rows dy
                        (exact terms): gamma(rows) sum|terms| + the terms' own errors + e |total| for the fp32 add of the accumulated old value.
    column / row sums   of bf16 values (exact terms): gamma(n) sum|terms| + e |total|.
    GELU                0.5 x (1 + erf(x / sqrt 2)):  0.5 |x| (1 + |erf|) 12 e + 2 e |gelu|   (erff within 4 ulp = 8 e, its argument's rounding at most
                        e / 2 of erf, the sum 1 + erf, the products: 1 + erf CANCELS for x < -3, which is why the term is not relative to gelu)
    GELU'               cdf + x pdf:  0.5 (1 + |erf|) 12 e + |x pdf| (x^2 / 2 + 8) e + e |gelu'|   (__expf(t) = exp2(t log2 e): the rounding of t log2 e
                        is a RELATIVE error |t| e of the result);   dx = bf16(dy gelu'): |dy| err + e |dx|.
    SwiGLU              sigmoid = 1 / (1 + __expf(-g)): silu relative (|g| + 8) e;  h = bf16(bf16(silu) u): flip(silu) |u| + hu(h)  (the product is exact);
                        backward, ONE rounding each (the kernel header: dgu = dh u silu'(g) | dh silu(g), silu unrounded):
                        dg: |dh u| s (1 + |g| (1 - s)) (|g| + 12) e  (1 + g (1 - s) cancels at g = -1.28), du: |dh silu| (|g| + 10) e.
    add                 e |a + b|;   ReLU and RoPE are exact / bit-defined (RoPE is the torch bf16 expression itself, see rope_reference).
Every bound also carries TINY = 2^-126, the smallest normal fp32 / bf16 magnitude: below it the formats (and a kernel flushing subnormals) have no
relative precision.  Bounds come back as float64 tensors shaped like the output.
"""
import functools
import math
from types import SimpleNamespace as NS

import torch

BF = torch.bfloat16
U = 2.0 ** -9        # half a bf16 unit in the last place, relative to the power of two above the value
E32 = 2.0 ** -24     # fp32 unit roundoff
TINY = 2.0 ** -126   # smallest normal fp32 / bf16
LN_EPS, RMS_EPS = 1e-5, 1e-6
SHARE_CAP = 5e-3     # GPU: share of outputs allowed to differ from the rounded emulation
HEADROOM_CAP = 1e-3  # CPU: share by which an fp32 torch version rounded at the same points may differ from it


# ---------------------------------------------------------------------------------------------- rounding and bounds
def rb(v):
    """float64 -> the nearest bf16 value (ties to even), as float64.  torch converts through fp32; where that fp32 image is exactly a bf16 tie but v was
    not, it is moved one fp32 step back towards v first, so the result is the single correct rounding of v"""
    f = v.to(torch.float32)
    res = v - f.double()
    tie = ((f.view(torch.int32) & 0xFFFF) == 0x8000) & (res != 0)
    toward = torch.where(res > 0, torch.full_like(f, float("inf")), torch.full_like(f, float("-inf")))
    return torch.where(tie, torch.nextafter(f, toward), f).to(BF).double()


def mag2(v):
    m, ex = torch.frexp(v.abs().double())
    return torch.where(m == 0, torch.zeros_like(m), torch.ldexp(torch.ones_like(m), ex))


def hu(v):
    return U * mag2(v)


def gamma(n):
    return n * E32


def round_bound(v, err32):
    """bound of |bf16(v^) - v| for |v^ - v| <= err32"""
    return hu(v.abs() + err32) + err32 + TINY


def flip(v, err32):
    """what an earlier rounding point costs against a reference rounded at the same point: a whole unit where v is within err32 of a tie"""
    near = hu(v) - (v - rb(v)).abs() <= err32
    return torch.where(near, 2 * hu(v.abs() + err32), torch.zeros_like(v))


def quantum(X):
    """per row, the largest power of two that divides every element (inf for a row of zeros)"""
    m, ex = torch.frexp(X.abs())
    i = (m * 2.0 ** 24).long()           # bf16 and fp32 significands are integers at this scale
    q = torch.ldexp((i & -i).double(), ex - 24)
    return torch.where(X == 0, torch.full_like(X, float("inf")), q).min(-1).values


def sum_err(X):
    """fp32 error bound of a row sum in any order: gamma(D) sum|x| - or 0 where every partial sum is exactly representable: all elements are multiples
    of the row's quantum q and sum|x| / q < 2^24 (small integers, constant rows, the `offset` rows: such sums are exact in any order)"""
    a = X.abs().sum(-1)
    return torch.where(a / quantum(X) < 2.0 ** 24, torch.zeros_like(a), gamma(X.shape[-1]) * a)


def ratio(got, ref, bound):
    """max |got - ref| / bound (what the GPU modules print and assert <= 1)"""
    return float(((got.double() - ref).abs() / bound).max())


def mismatch_share(got, emu):
    return float((got.double() != emu).double().mean())


# ---------------------------------------------------------------------------------------------- norms, forward
def ln_fwd(x, w, b, eps=LN_EPS):
    X, W, B = x.double(), w.double(), b.double()
    D = X.shape[-1]
    mean = X.mean(-1)
    xc = X - mean[:, None]
    var = (xc * xc).mean(-1)
    rstd = (var + eps).rsqrt()
    y = xc * rstd[:, None] * W + B
    e_mean = sum_err(X) / D + 2 * E32 * mean.abs()
    rel_rstd = 0.5 * (gamma(D + 6) + e_mean ** 2 / (var + eps)) + 4 * E32
    p = (xc * rstd[:, None] * W).abs()
    e_y = W.abs() * (rstd * e_mean)[:, None] + p * (rel_rstd[:, None] + 4 * E32) + E32 * (p + B.abs())
    return NS(mean=mean, rstd=rstd, var=var, y=y, y_r=rb(y), mean_bound=e_mean + TINY, rstd_bound=rstd * rel_rstd, y_bound=round_bound(y, e_y))


def rms_fwd(x, w, eps=RMS_EPS):
    X, W = x.double(), w.double()
    D = X.shape[-1]
    rstd = ((X * X).mean(-1) + eps).rsqrt()
    rel_rstd = 0.5 * gamma(D + 4) + 4 * E32
    xh = X * rstd[:, None]
    e_xh = xh.abs() * (rel_rstd + E32)
    xh_b = rb(xh)
    y = W * xh_b
    fl = W.abs() * flip(xh, e_xh)
    return NS(rstd=rstd, xh=xh, xh_b=xh_b, y=y, y_r=rb(y), y_once=rb(W * xh), rstd_bound=rstd * rel_rstd, y_bound=fl + hu(y.abs() + fl) + TINY)


# ---------------------------------------------------------------------------------------------- norms, backward
def _old(t, like):
    return torch.zeros_like(like) if t is None else t.double()


def _parts(terms, e_terms):
    return terms.sum(0), terms.abs().sum(0), e_terms.sum(0)


def total(parts, old, n):
    """(total, bound) of bf16(old + sum of n terms), the sum in fp32 in any order; parts = (sum, sum |terms|, sum of the terms' own errors)"""
    s, a, e = parts
    t = s + _old(old, s)
    return t, round_bound(t, gamma(n) * a + e + E32 * t.abs())


def _sum_bound(terms, e_terms, old, n):
    return total(_parts(terms, e_terms), old, n)


def norm_bwd(x, w, dy, mean, rstd, *, rms, dx_add=None, dw_old=None, db_old=None, n_terms=None):
    """mean / rstd: the fp32 statistics the kernel is given (mean ignored for rms).  dx comes back as its two branches: dx_norm (float64, unrounded) and
    dx_add; dx = what the kernel rounds last (dx_norm, or bf16(dx_norm) + dx_add), dx_r its bf16 emulation.  dw_parts / db_parts with total() give the
    accumulated forms without a second pass.  n_terms: the non-zero rows of dy where that is fewer than all (one_hot_rows: 1 - no accumulation error)."""
    X, W, DY, R = x.double(), w.double(), dy.double(), rstd.double()[:, None]
    rows, D = X.shape
    n = rows if n_terms is None else n_terms
    M = torch.zeros_like(R) if rms else mean.double()[:, None]
    xh = (X - M) * R
    g = DY * W
    c1 = torch.zeros_like(R) if rms else g.mean(-1, keepdim=True)
    c2 = (g * xh).mean(-1, keepdim=True)
    v = R * (g - c1 - xh * c2)
    e_xh = xh.abs() * 2 * E32
    e_c1 = gamma(D + 2) * g.abs().mean(-1, keepdim=True) * (0.0 if rms else 1.0)
    e_c2 = gamma(D + 5) * (g * xh).abs().mean(-1, keepdim=True)
    e_v = R * (e_c1 + xh.abs() * e_c2 + c2.abs() * e_xh + 8 * E32 * (g.abs() + c1.abs() + (xh * c2).abs()))
    if dx_add is None:
        add, dx, dx_bound = None, v, round_bound(v, e_v)
    else:
        add = dx_add.double()
        dx = rb(v) + add
        dx_bound = round_bound(dx, flip(v, e_v) + E32 * dx.abs())
    out = NS(xh=xh, dx_norm=v, dx_add=add, dx=dx, dx_r=rb(dx), dx_bound=dx_bound, n=n)
    if rms:
        out.xh_b = rb(xh)
        out.dw_parts = _parts(DY * out.xh_b, DY.abs() * flip(xh, e_xh))
        out.dw_unrounded = (DY * xh).sum(0) + _old(dw_old, X[0])      # what a kernel using the unrounded xh would return
    else:
        t = DY * xh
        out.dw_parts = _parts(t, t.abs() * 3 * E32)
        out.db_parts = _parts(DY, torch.zeros_like(DY))
        out.db, out.db_bound = total(out.db_parts, db_old, n)
    out.dw, out.dw_bound = total(out.dw_parts, dw_old, n)
    return out


def colsum_ref(x, old=None):
    """column sums of bf16 values (the dx a kernel returned, a grad_output): (total float64, bound)"""
    X = x.double()
    return _sum_bound(X, torch.zeros_like(X), _old(old, X[0]), X.shape[0])


def rowsum_ref(x, C, old=None):
    X = x.double()[:, :C]
    total = X.sum(1) + _old(old, X[:, 0])
    return total, round_bound(total, gamma(C) * X.abs().sum(1) + E32 * total.abs())


# ---------------------------------------------------------------------------------------------- activations
SQRT1_2 = math.sqrt(0.5)
INV_SQRT_2PI = 1.0 / math.sqrt(2.0 * math.pi)


def gelu_ref(x):
    X = x.double()
    erf = torch.erf(X * SQRT1_2)
    y = 0.5 * X * (1 + erf)
    e = 0.5 * X.abs() * (1 + erf.abs()) * 12 * E32 + 2 * E32 * y.abs()
    return NS(y=y, y_r=rb(y), y_bound=round_bound(y, e))


def gelu_grad(x):
    """(gelu'(x) float64, its fp32 error bound)"""
    X = x.double()
    erf = torch.erf(X * SQRT1_2)
    xpdf = X * INV_SQRT_2PI * torch.exp(-0.5 * X * X)
    d = 0.5 * (1 + erf) + xpdf
    return d, 0.5 * (1 + erf.abs()) * 12 * E32 + xpdf.abs() * (0.5 * X * X + 8) * E32 + E32 * d.abs()


def gelu_bwd_ref(dy, pre):
    DY = dy.double()
    d, e_d = gelu_grad(pre)
    dx = DY * d
    return NS(dx=dx, dx_r=rb(dx), dx_bound=round_bound(dx, DY.abs() * e_d + E32 * dx.abs()))


def swiglu_fwd_ref(gu):
    I = gu.shape[1] // 2
    G, Uu = gu[:, :I].double(), gu[:, I:].double()
    silu = G * torch.sigmoid(G)
    e_silu = silu.abs() * (G.abs() + 8) * E32 + TINY
    silu_b = rb(silu)
    h = silu_b * Uu
    fl = Uu.abs() * flip(silu, e_silu)
    return NS(silu=silu, silu_b=silu_b, h=h, h_r=rb(h), h_once=rb(silu * Uu), h_bound=fl + hu(h.abs() + fl) + TINY)


def swiglu_bwd_ref(gu, dh):
    I = gu.shape[1] // 2
    G, Uu, DH = gu[:, :I].double(), gu[:, I:].double(), dh.double()
    s = torch.sigmoid(G)
    dg = DH * Uu * (s * (1 + G * (1 - s)))
    du = DH * (G * s)
    e_dg = (DH * Uu).abs() * s * (1 + G.abs() * (1 - s)) * (G.abs() + 12) * E32
    e_du = du.abs() * (G.abs() + 10) * E32
    dgu = torch.cat([dg, du], 1)
    return NS(dgu=dgu, dgu_r=rb(dgu), dgu_bound=round_bound(dgu, torch.cat([e_dg, e_du], 1)))


def add_ref(a, b):
    s = a.double() + b.double()
    return NS(y=s, y_r=rb(s), y_bound=round_bound(s, E32 * s.abs()))


def rotate_half(t):
    h = t.shape[-1] // 2
    return torch.cat([-t[..., h:], t[..., :h]], -1)


def rope_reference(x, cos, sin, backward=False):
    """apply_rotary_pos_emb as bf16 tensor ops, every product and sum rounded (run it on the device the kernel ran on).  x [rows, heads, D], cos / sin
    [rows, D] bf16 rows already gathered by position; backward = the rotation by -theta"""
    c, s = cos[:, None, :], sin[:, None, :]
    return x * c + rotate_half(x) * (-s if backward else s)


# ---------------------------------------------------------------------------------------------- input builders (fp32 on the CPU unless said; each asserts its property)
def _gen(seed):
    return torch.Generator().manual_seed(seed)


def gauss(shape, seed, sigma=2.0):
    x = (torch.randn(shape, generator=_gen(seed)) * sigma).to(BF)
    if x.numel() >= 64:
        assert abs(float(x.float().mean())) < sigma and 0.5 * sigma < float(x.float().std()) < 1.5 * sigma
    return x


def onepass_rstd_f32(x, eps=LN_EPS):
    """the one-pass fp32 statistic E[x^2] - mean^2 a careless LayerNorm would use"""
    xf = x.float()
    m = xf.mean(-1)
    return torch.rsqrt((xf * xf).mean(-1) - m * m + eps)


def offset(rows, D, seed):
    """1024 + 8 k, k an integer in [-3, 3]: D // 16 pairs (+k, -k) per row, 0 elsewhere - every value exact in bf16, the mean exactly 1024, the spread a few
    units.  The two-pass variance sees the small integers 8 k and is exact to fp32; the one-pass form E[x^2] - mean^2 loses them in the rounding of
    E[x^2] ~ 2^20 (ulp 1/8 against a variance of ~30)."""
    g = _gen(seed)
    k = torch.zeros((rows, D))
    n = max(D // 16, 1)
    for r in range(rows):
        pos = torch.randperm(D, generator=g)[: 2 * n]
        v = torch.randint(1, 4, (n,), generator=g).float()
        k[r, pos[:n]], k[r, pos[n:]] = v, -v
    xf = 1024.0 + 8.0 * k
    x = xf.to(BF)
    assert torch.equal(x.float(), xf), "offset: values must be exact in bf16"
    r = ln_fwd(x, torch.ones(D), torch.zeros(D))
    assert bool((r.mean == 1024).all()) and bool((r.var.sqrt() < 24).all()) and bool((r.var > 0).all())
    xf = x.float()
    two_pass = torch.rsqrt(((xf - xf.mean(-1, keepdim=True)) ** 2).mean(-1) + LN_EPS)
    assert bool(((two_pass.double() - r.rstd).abs() <= r.rstd_bound).all()), "offset: the two-pass fp32 variance must hold the bound"
    miss = (onepass_rstd_f32(x).double() - r.rstd).abs() > r.rstd_bound
    assert float(miss.double().mean()) >= 0.5, "offset: the one-pass fp32 variance must miss the rstd bound on most rows"
    return x


def zero_row_ids(rows):
    return sorted({0, rows - 1, rows // 2})


def zero_rows(rows, D, seed):
    x = gauss((rows, D), seed)
    x[zero_row_ids(rows)] = 0
    assert bool((x[0] == 0).all()) and bool((x[rows - 1] == 0).all())
    return x


CONST_POW2 = [1.0, -0.5, 128.0, -0.0078125, 4.0, -32.0, 0.25]
CONST_ANY = [3.140625, -0.5, 100.0, -2.71875, 0.0078125, 1.0, -7.0]


def _const(rows, D, vals):
    v = torch.tensor(vals)[torch.arange(rows) % len(vals)]
    x = v.to(BF)[:, None].repeat(1, D).contiguous()
    assert bool((x == x[:, :1]).all()) and torch.equal(x[:, 0].float(), v)
    return x


def const_rows(rows, D, seed):
    """rows of one repeated value, a power of two: sum = D c is exact and D c fl(1 / D) rounds back to c at the widths the cases use (asserted in fp32), so
    x - mean is exactly 0, and LayerNorm's y is b bit for bit - the emulation can be held to it"""
    x = _const(rows, D, CONST_POW2)
    assert torch.equal((x.float().sum(-1) * torch.tensor(1.0 / D, dtype=torch.float32)), x[:, 0].float()), "const_rows: mean must be exact in fp32"
    return x


def const_rows_any(rows, D, seed):
    """rows of one repeated value that is no power of two: mean^ = c (1 + delta), so LayerNorm's y = b - c delta rstd w is all cancellation noise; only
    the bound (its carried statistic term) can hold it, no emulation"""
    return _const(rows, D, CONST_ANY)


def massive(rows, D, seed, n=3, value=3000.0):
    g = _gen(seed)
    x = torch.randn((rows, D), generator=g)
    for r in range(rows):
        cols = torch.randperm(D, generator=g)[: min(n, D)]
        x[r, cols] = value * (torch.randint(0, 2, (len(cols),), generator=g).float() * 2 - 1)
    x = x.to(BF)
    assert bool(((x.float().abs() > 0.9 * value).sum(-1) == min(n, D)).all())
    return x


EXTREME_VALUES = [0.0, -0.0, 2.0 ** -100, -(2.0 ** -100), 20.0, -20.0, 200.0, -200.0, 2.0 ** 100, -(2.0 ** 100)]


def extremes(shape, seed, sigma=2.0):
    """the values where x * x overflows fp32 inside gelu', __expf overflows inside the sigmoid, and the signed zeros, mixed into a Gaussian; finite"""
    g = _gen(seed)
    x = torch.randn(shape, generator=g) * sigma
    flat = x.view(-1)
    n = flat.numel()
    assert n >= len(EXTREME_VALUES)
    reps = max(1, min(n // (4 * len(EXTREME_VALUES)), 64))
    pos = torch.randperm(n, generator=g)[: reps * len(EXTREME_VALUES)]
    flat[pos] = torch.tensor(EXTREME_VALUES).repeat(reps)
    x = x.to(BF)
    assert bool(torch.isfinite(x.float()).all())
    for v in EXTREME_VALUES:
        assert bool((x.float() == v).any()), v
    assert bool(((x.view(torch.int16) & 0x7FFF) == 0).any()) and bool((x.view(torch.int16) == -0x8000).any()), "both signed zeros"
    return x


def balanced_int(rows, cols, seed):
    """non-zero integers in {-2, -1, 1, 2}: a block P, its negation under a row permutation, and one (odd rows) or two (even rows) extra rows of 1 / {1, 2}
    LAST.  Every column sums to a small integer and every fp32 partial sum, in any order, is an exact integer: a correct column sum IS that integer, and a
    dropped, doubled or misplaced row changes every column."""
    g = _gen(seed)
    extra = 1 if rows % 2 else 2
    h = (rows - extra) // 2
    P = torch.tensor([-2.0, -1.0, 1.0, 2.0])[torch.randint(0, 4, (h, cols), generator=g)]
    tail = [torch.ones(1, cols)]
    if extra == 2:
        tail.insert(0, torch.randint(1, 3, (1, cols), generator=g).float())
    m = torch.cat([P, -P[torch.randperm(h, generator=g)]] + tail, 0)
    assert m.shape == (rows, cols) and bool((m != 0).all()) and bool((m.abs() <= 2).all()) and bool((m == m.round()).all())
    s = m.double().sum(0)
    assert bool((s.abs() <= 16).all()) and bool((s == s.round()).all()) and 2 * rows < 2 ** 24
    return m.to(BF)


def small_int(n, seed, lo=-8, hi=8):
    return torch.randint(lo, hi + 1, (n,), generator=_gen(seed)).float().to(BF)


def one_hot_rows(rows, r, D, seed):
    dy = torch.zeros((rows, D))
    dy[r] = torch.randn(D, generator=_gen(seed))
    dy = dy.to(BF)
    assert bool((dy[r] != 0).any()) and int((dy != 0).any(-1).sum()) == 1
    return dy


def norm_weights(D, seed):
    g = _gen(seed)
    return (1 + 0.1 * torch.randn(D, generator=g)).to(BF), (0.1 * torch.randn(D, generator=g)).to(BF)


NORM_BUILDERS = {"gauss": lambda rows, D, seed: gauss((rows, D), seed), "offset": offset, "zero_rows": zero_rows, "const_rows": const_rows, "const_rows_any": const_rows_any,
                 "massive": massive}


@functools.lru_cache(maxsize=None)
def norm_input(builder, rows, D, seed=11):
    """the bf16 input of a case, built once, never to be written to"""
    return NORM_BUILDERS[builder](rows, D, seed)


# ---------------------------------------------------------------------------------------------- launch geometry (csrc/norm.hip, csrc/elementwise.hip restated)
def cdiv(a, b):
    return -(-a // b)


FWD_D8 = [8, 512, 520, 1536, 1544, 3584, 3592, 8192]
FWD_D4 = [4, 100, 508, 516, 1276, 1284, 3580, 3588, 8188]
FWD_GRID_CAP_ROWS = 2048 * 4   # norm_grid: 4 rows per block, 2048 blocks


def fwd_vpl_vw(D):
    """(VPL, VW) of launch_fwd: vectors per lane and elements per vector"""
    assert D % 4 == 0 and D <= 8192
    if D % 8 == 0:
        return (1 if D <= 512 else 3 if D <= 1536 else 7 if D <= 3584 else 16), 8
    return (2 if D <= 512 else 5 if D <= 1280 else 14 if D <= 3584 else 32), 4


def fwd_grid_strides(rows):
    return rows > FWD_GRID_CAP_ROWS


def bwd_form(D, knob_rows=False):
    return "cols" if (not knob_rows and D % 8 == 0 and D // 8 <= 512) else "rows"


def norm_bwd_blocks(rows):
    """afk_norm_bwd_blocks: the workspace bound both forms are clamped to"""
    return min(cdiv(rows, 2), 1024)


def cols_geometry(rows, D, R=2):
    """column-owned backward: (blocks = fold part count, groups, cap, ragged last group)"""
    cap = 512 if D // 8 > 256 else 1024
    groups = cdiv(rows, R)
    return NS(blocks=min(groups, cap, norm_bwd_blocks(rows)), groups=groups, cap=cap, ragged=rows % R != 0)


def rows_form_blocks(rows):
    """row-per-wave backward: partial rows (4 rows per block, cap 512)"""
    return min(cdiv(rows, 4), 512, norm_bwd_blocks(rows))


def bwd_parts(rows, D, rms=False, knob_rows=False, R=2):
    return cols_geometry(rows, D, R if rms else 2).blocks if bwd_form(D, knob_rows) == "cols" else rows_form_blocks(rows)


def fold_paths(nparts):
    """fold_partials_kernel, over its 16 part-slices: (the 4-way unrolled loop runs, the tail loop runs)"""
    unrolled = tail = False
    for sl in range(16):
        p = sl
        while p + 48 < nparts:
            unrolled, p = True, p + 64
        while p < nparts:
            tail, p = True, p + 16
    return unrolled, tail


def gelu_cs_geometry(rows, cap=512):
    """gelu_bwd_colsum_kernel: parts (= blocks over rows: block b owns rows b, b + parts, ...), fewest / most rows of a block, and which of its loops
    (4 rows unrolled, one-row tail) run in some block"""
    parts = min(max(rows, 1), cap)
    lo = rows // parts
    hi = lo + (1 if rows % parts else 0)
    return NS(parts=parts, min_rows=lo, max_rows=hi, unrolled=hi >= 4, tail=bool(lo % 4 or hi % 4))


def colsum_geometry(rows):
    slices = min(max(cdiv(rows, 512), 1), 64)
    return NS(slices=slices, rows_per_slice=cdiv(rows, slices))


EW_CAP_BLOCKS, EW_THREADS = 4096, 256
EW_CAP_ITEMS = EW_CAP_BLOCKS * EW_THREADS


def ew_blocks(n_items):
    return min(max(cdiv(n_items, EW_THREADS), 1), EW_CAP_BLOCKS)


def ew_past_cap(n_items):
    return n_items > EW_CAP_ITEMS


# ---------------------------------------------------------------------------------------------- the cases the CPU and the GPU modules share
FWD_ROWS = (1, 3, 5)
STAT_D = (1280, 3584, 100)          # widths of the statistic builders (VPL 3 / 7 at 8-wide vectors, VPL 2 at 4-wide)
FWD_STRIDE_CASES = ((FWD_GRID_CAP_ROWS + 5, 64), (FWD_GRID_CAP_ROWS + 5, 100))   # one grid-stride step with a ragged block


def fwd_cases():
    """(kind, builder, rows, D, share): share = the output is also held to the rounded emulation"""
    out = []
    for kind in ("ln", "rms"):
        out += [(kind, "gauss", rows, D, True) for D in FWD_D8 + FWD_D4 for rows in FWD_ROWS]
        out += [(kind, "gauss", rows, D, True) for rows, D in FWD_STRIDE_CASES]
        for b in ("offset", "zero_rows", "const_rows", "const_rows_any") + (("massive",) if kind == "rms" else ()):
            out += [(kind, b, 5, D, not (kind == "ln" and b == "const_rows_any")) for D in STAT_D]
    return out


BWD_COLS_D = (8, 64, 520, 2048, 2056, 4096)
BWD_COLS_FOLD_ROWS = (1, 2, 3, 31, 33, 97, 127, 129)                 # at D = 64: fold part counts 1, 1, 2, 16, 17, 49, 64, 65
BWD_COLS_PAST_CAP = ((2051, 64), (1027, 2056), (1027, 4096))         # three groups past the cap of 1024 / two past the cap of 512; ragged last group
BWD_ROWS_D = (4, 100, 516, 1284, 3580)
BWD_ROWS_ROWS = (1, 5, 2051)                                         # 2051: past the cap of 512 blocks


def bwd_cols_cases():
    c = [(rows, 64) for rows in BWD_COLS_FOLD_ROWS] + [(rows, D) for D in BWD_COLS_D for rows in (3, 5)] + list(BWD_COLS_PAST_CAP)
    return list(dict.fromkeys(c))


def bwd_rows_cases():
    return [(rows, D) for D in BWD_ROWS_D for rows in BWD_ROWS_ROWS]


def second_step_row(rows, D, rms=False, knob_rows=False, R=2):
    """the first row a block reaches in its second grid-stride step (None if no block takes one)"""
    if bwd_form(D, knob_rows) == "cols":
        g = cols_geometry(rows, D, R if rms else 2)
        return g.blocks * (R if rms else 2) if g.groups > g.blocks else None
    nb = rows_form_blocks(rows)
    return nb * 4 if cdiv(rows, 4) > nb else None


def sharp_rows(rows, D, **kw):
    """the rows where a grid-stride or ragged-group slip shows: 0, the last two, the first of the second step"""
    r = [0, rows - 1, rows - 2, second_step_row(rows, D, **kw)]
    return sorted({v for v in r if v is not None and 0 <= v < rows})


COLSUM_ROWS = (1, 31, 32, 33, 512, 513, 1025, 3585, 4097, 32769)     # slice counts 1, 1, 1, 1, 1, 2, 3, 8, 9, 64
COLSUM_SLICES = (1, 1, 1, 1, 1, 2, 3, 8, 9, 64)
COLSUM_COLS = (8, 64, 72, 200)
ROWSUM_C = (1, 7, 8, 150, 512, 513)
ROWSUM_ROWS = (1, 4, 5)
GELU_CS_ROWS = (1, 5, 511, 512, 513, 1541, 2049)
GELU_CS_WIDE_C = (2048, 2056)                                        # 2056: the second blockIdx.y has one live thread

ACT_ONE = 8
ACT_BIG = 8 * (EW_CAP_ITEMS + 3)
SWIGLU_SHAPES = ((1, 8), (5, 8), (EW_CAP_ITEMS // 3 + 1, 24))        # (rows, I): one vector; I = 8; three vectors per row, rows * 3 just past the cap
ACT_SIGMA = 1.0   # activations are held to the emulation on N(0, 1): at N(0, 2^2) 4 % of the inputs sit below -3.5, where 1 + erf cancels to a few fp32 ulps
                  # and the bf16 rounding of gelu follows the erff implementation, not the operation (the bound covers it, an emulation cannot)


@functools.lru_cache(maxsize=None)
def act_input(kind, shape, seed):
    return {"gauss": lambda: gauss(shape, seed, ACT_SIGMA), "gauss2": lambda: gauss(shape, seed), "extremes": lambda: extremes(shape, seed)}[kind]()

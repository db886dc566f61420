"""References and numerical bars for the default optimizer step - AdamW with fp32 master and fp32 moments (afk_adamw_step / afk_adamw_step_t), the
gradient sum of squares (afk_sumsq_bf16) and the clip coefficient (afk_clip_coef) - shared by tests/test_optim_ref_cpu.py and
tests/test_optim_edges_gpu.py.

AdamW.  X is the update evaluated in float64 from the inputs the kernel reads: the fp32 master / m / v, the bf16 gradient times the gradient
multiplier (grad_scale, times hyper[3] when hyper is given), lr / betas / eps / wd as the doubles the caller passed, and the bias corrections in
double from `step` (or hyper[1], hyper[2] widened exactly):

    M = b1 m0 + (1 - b1) g        V = b2 v0 + (1 - b2) g^2        U = (lr / bc1) M / (sqrt(V) / bc2s + eps)        W = w0 (1 - lr wd) - U

The bar is derived, not tuned.  u = 2^-24 bounds the relative error of one fp32 rounding (of an operation, or of a double argument narrowed to
the float the C ABI takes).  h(b) = 2^-25 / (1 - b) is the relative error of `1.f - (float)b`, which the kernel forms in fp32: (float)b is off by
at most half an ulp of [0.5, 1), 2^-25, and the subtraction itself is exact.  The gradient the kernel uses, g * multiplier, is exact for a
multiplier of 1 and carries at most 3u otherwise ((float)grad_scale, its product with hyper[3], the product with g).

    tol_m = 4u |M| + (4u + h(b1)) (b1 |m0| + (1 - b1) |g|) + 2^-126
        b1 |m0|: (float)b1 and the product, 2u.  (1 - b1) |g|: h(b1), up to 3u in g, the product: 4u + h.  The rounding of the sum: u |M|.  The
        operand term is what covers g ~ -m, where |M| is far below the operands.
    tol_v = (8u + h(b2)) V + 2^-126
        no cancellation, every term is positive.  b2 v0: 2u.  (1 - b2) g g: h(b2), two products 2u, g twice 4u (6u with hyper AND an inexact
        grad_scale: the tests that pass hyper use grad_scale = 0.5).  The sum: u.  7u + h in all.
    tol_w = 4u |w0| + |U| (tol_v / (2V) + 2^-22 / (1 - b1^t) + 2^-22 / (1 - b2^t) + 16u) + (lr / bc1) tol_m / denom
        4u |w0|: 1 - lr wd (lr wd carries 3u of itself, below u of 1; the subtraction rounds by 2^-25), the product, and the final subtraction
        (u |W| <= u |w0| + u |U|).
        tol_v / (2V): the relative error of sqrt(v), which bounds the relative error it causes in denom (denom >= sqrt(V) / bc2s); 0 where
        V = 0, since then v = 0 exactly.
        2^-22 / (1 - b^t): the bias corrections 1.f - powf((float)b, (float)t): (float)b moves b^t by t 2^-25 b^(t-1), powf adds an ulp or two
        of b^t, and both stay below 2^-22 in absolute terms for every t (t b^(t-1) <= 1 / (e (1 - b)) is reached only where b^t is small against
        1 - b^t); relative to the correction that is 2^-22 / (1 - b^t).  At t = 1 this is 4 h(b).  The square root halves the second one.
        16u: (float)lr, lr / bc1, sqrtf, / bc2s, (float)eps, + eps, m / denom, the product, the final subtraction: 9 roundings.
        (lr / bc1) tol_m / denom: the error of m carried through the quotient.
    The 2^-126 floors (the smallest normal fp32) admit a flushed or gradually underflowed product.  An element whose tolerance is 0 must be
    exact (worst_ratio).  The bf16 parameter has no tolerance: it equals master.to(bfloat16) bit for bit.

restated_fp32 is csrc/elementwise.hip adamw_elem written with fp32 tensors, in the kernel's operation order and without contraction: the CPU
stand-in for the kernel.  MUTATIONS are single plausible mistakes of that code; the CPU test shows that the bar catches each of them.

Sum of squares.  The partial kernel runs grid = min(ceil(ceil(n / 8) / 256), 1024) blocks of 256 lanes, 8 elements per lane and grid stride,
block 0 adds the n % 8 tail; a block fold and a second one-block fold follow.  With positive terms only, the error of a thread's sum of k terms
is below k u times it (the standard gamma_k bound, products included in the slack), and the two folds add at most 6 + 4 + 4 + 6 + 4 = 24 more
additions per path: |x - X| <= (k + 32) u X, k = 8 ceil(ceil(n / 8) / (256 grid)).

Clip coefficient.  norm = sqrt(sum of the slots) * scale, coef = min(1, max_norm / (norm + 1e-6)), in float64; 4u relative on both, and the
coefficient is exactly 1.0f wherever the float64 quotient is >= 1 + 2^-20 (far outside the 4u band round 1).
"""
import math

import torch

U = 2.0 ** -24
FLOOR = 2.0 ** -126
SUMSQ_BLOCKS = 1024   # the grid cap of afk_sumsq_bf16 (afk_sumsq_workspace_floats)

# (beta1, beta2, lr, weight_decay); eps = 1e-8 throughout
HYPER_SETS = [dict(beta1=0.9, beta2=0.999, lr=1e-2, weight_decay=0.1, eps=1e-8),
              dict(beta1=0.9, beta2=0.95, lr=1e-3, weight_decay=0.01, eps=1e-8),
              dict(beta1=0.8, beta2=0.9999, lr=1e-5, weight_decay=0.0, eps=1e-8)]
STEPS = (1, 2, 3, 4, 1000)

MUTATIONS = ("bc_next_step", "no_bc2", "eps_in_sqrt", "eps_over_sqrt_bc2", "decay_after_update", "l2_decay", "v_with_beta1", "multiplier_dropped",
             "hyper3_ignored")


def h(beta):
    return 2.0 ** -25 / (1.0 - beta)


def _widen(hyper):
    """the four fp32 values the kernel reads, as python floats (exact)"""
    return [float(x) for x in hyper.detach().double().cpu()]


def ref64(w0, m0, v0, g, *, lr, beta1, beta2, eps, weight_decay, step, grad_scale=1.0, hyper=None):
    """one step in float64 -> {"w" | "m" | "v": (X, tolerance)}"""
    mult = float(grad_scale)
    if hyper is not None:
        hv = _widen(hyper)
        lr, bc1, bc2s, mult = hv[0], hv[1], hv[2], mult * hv[3]
        bc1_t, bc2_t = bc1, bc2s * bc2s
    else:
        bc1_t, bc2_t = 1.0 - beta1 ** step, 1.0 - beta2 ** step
        bc1, bc2s = bc1_t, math.sqrt(bc2_t)
    w, m, v, gr = w0.double(), m0.double(), v0.double(), g.double() * mult
    M = beta1 * m + (1.0 - beta1) * gr
    V = beta2 * v + (1.0 - beta2) * gr * gr
    denom = V.sqrt() / bc2s + eps
    upd = (lr / bc1) * M / denom
    W = w * (1.0 - lr * weight_decay) - upd
    tol_m = 4 * U * M.abs() + (4 * U + h(beta1)) * (beta1 * m.abs() + (1.0 - beta1) * gr.abs()) + FLOOR
    tol_v = (8 * U + h(beta2)) * V + FLOOR
    rel_sqrt = torch.where(V > 0, tol_v / (2.0 * V.clamp_min(1e-300)), torch.zeros_like(V))
    tol_w = 4 * U * w.abs() + upd.abs() * (rel_sqrt + 2.0 ** -22 / bc1_t + 2.0 ** -22 / bc2_t + 16 * U) + (lr / bc1) * tol_m / denom
    return {"w": (W, tol_w), "m": (M, tol_m), "v": (V, tol_v)}


def ratios(x, X, tol):
    """per element |x - X| / tolerance; an element whose tolerance is 0 must be exact and counts as 0 or inf"""
    err = (x.double() - X).abs()
    return torch.where(tol > 0, err / tol.clamp_min(1e-300), torch.where(err == 0, torch.zeros_like(err), torch.full_like(err, float("inf"))))


def worst_ratio(x, X, tol):
    """max over the elements of |x - X| / tolerance (<= 1 passes)"""
    return float(ratios(x, X, tol).max())


def make_state(n, device="cpu", seed=0):
    """fp32 master 0.02 N(0,1), every 5th exactly 0; m = v = 0"""
    gen = torch.Generator(device="cpu").manual_seed(77 + seed)
    w = 0.02 * torch.randn(n, generator=gen)
    w[::5] = 0.0
    return w.to(device), torch.zeros(n, device=device), torch.zeros(n, device=device)


def make_grad(n, step, device="cpu", seed=0):
    """bf16 N(0,1) * 10^k, k uniform in -9..-1 per element; every 7th gradient zero on steps 1 and 2 (those elements keep m = v = 0 for two steps)
    and another 7th on step 4.  Small gradients bring sqrt(v) down to eps and below, where a misplaced eps shows."""
    gen = torch.Generator(device="cpu").manual_seed(1000 * seed + step + 1)
    x = torch.randn(n, generator=gen) * 10.0 ** torch.randint(-9, 0, (n,), generator=gen).float()
    if step in (1, 2):
        x[::7] = 0.0
    elif step == 4:
        x[3::7] = 0.0
    return x.to(torch.bfloat16).to(device)


def restated_fp32(w0, m0, v0, g, *, lr, beta1, beta2, eps, weight_decay, step, grad_scale=1.0, hyper=None, mutation=None):
    """adamw_elem of csrc/elementwise.hip with fp32 tensors: same operation order, every product and sum rounded to fp32, 1 - beta and 1 - lr wd
    formed in fp32, bias corrections 1.f - powf(beta, (float)t) as afk_adamw_step forms them.  -> (master, m, v, param).  `mutation`: one of
    MUTATIONS, a single mistake."""
    assert mutation is None or mutation in MUTATIONS, mutation
    f = lambda c: torch.tensor(c, dtype=torch.float32, device=w0.device)
    one = f(1.0)
    t = step + 1 if mutation == "bc_next_step" else step
    lr_, b1, b2, eps_, wd = f(lr), f(beta1), f(beta2), f(eps), f(weight_decay)
    bc1 = one - torch.pow(b1, f(float(t)))
    bc2s = (one - torch.pow(b2, f(float(t)))).sqrt()
    mult = f(grad_scale)
    if hyper is not None:
        hy = hyper.detach().float().to(w0.device)
        lr_, bc1, bc2s = hy[0], hy[1], hy[2]
        if mutation != "hyper3_ignored":
            mult = mult * hy[3]
    if mutation == "multiplier_dropped":
        mult = one
    if mutation == "no_bc2":
        bc2s = one
    w, mm, vv = w0.float(), m0.float(), v0.float()
    gr = g.float() * mult
    if mutation == "l2_decay":
        gr = gr + wd * w
    elif mutation != "decay_after_update":
        w = w * (one - lr_ * wd)
    mm = b1 * mm + (one - b1) * gr
    if mutation == "v_with_beta1":
        vv = b1 * vv + ((one - b1) * gr) * gr
    else:
        vv = b2 * vv + ((one - b2) * gr) * gr
    if mutation == "eps_in_sqrt":
        denom = (vv + eps_).sqrt() / bc2s
    elif mutation == "eps_over_sqrt_bc2":
        denom = (vv.sqrt() + eps_) / bc2s
    else:
        denom = vv.sqrt() / bc2s + eps_
    w = w - (lr_ / bc1) * (mm / denom)
    if mutation == "decay_after_update":
        w = w * (one - lr_ * wd)
    return w, mm, vv, w.to(torch.bfloat16)


# ---------------------------------------------------------------------------------------------- sum of squares
def _cdiv(a, b):
    return -(-a // b)


def sumsq_grid(n):
    return min(_cdiv(_cdiv(n, 8), 256), SUMSQ_BLOCKS)


def sumsq_terms_per_thread(n):
    return 8 * _cdiv(_cdiv(n, 8), 256 * sumsq_grid(n))


def sumsq_ref(x):
    """-> (float64 sum of squares, tolerance)"""
    ref = float(x.double().pow(2).sum())
    return ref, (sumsq_terms_per_thread(x.numel()) + 32) * U * ref


def sumsq_probe_edges(n):
    """{name: index} of the edges of afk_sumsq_bf16 at length n that exist (see sumsq_probes)"""
    nv, grid = n // 8, sumsq_grid(n)
    stride = 8 * 256 * grid
    e = {"first": 0, "last": n - 1}
    for name, i in (("vec0_last", 7), ("vec1_first", 8), ("stride1_first", stride)):
        if i < n:
            e[name] = i
    if nv >= 1:
        e["last_vec_first"], e["last_vec_last"] = 8 * (nv - 1), 8 * nv - 1
    for j in range(n % 8):
        e[f"tail{j}"] = 8 * nv + j
    if nv > 256 * SUMSQ_BLOCKS:   # beyond the grid cap: the same edges in the last grid stride
        s = (nv - 1) // (256 * grid) * stride
        for name, i in (("last_stride_first", s), ("last_stride_vec0_last", s + 7), ("last_stride_vec1_first", s + 8)):
            if i < n:
                e[name] = i
    return e


def sumsq_probes(n):
    """sorted one-hot probe indices for length n: 0, 7, 8; the first element of the second grid stride; the first and the last element of the
    last full vector; every tail element; beyond the grid cap the same in the last stride"""
    return sorted(set(sumsq_probe_edges(n).values()))


# ---------------------------------------------------------------------------------------------- clip coefficient
def clip_coef(sumsq, scale, max_norm):
    """-> (norm, coefficient) in float64 from the fp32 slots"""
    norm = math.sqrt(float(sumsq.double().sum())) * scale
    return norm, min(1.0, max_norm / (norm + 1e-6))


def clip_coef_check(norm_got, coef_got, sumsq, scale, max_norm):
    """-> (|norm error| / (4u norm) or None, |coef error| / (4u coef)); the coefficient must be exactly 1 where the float64 quotient is >= 1 + 2^-20
    (reported as inf otherwise)"""
    norm, coef = clip_coef(sumsq, scale, max_norm)
    rn = None if norm_got is None else abs(norm_got - norm) / (4 * U * norm)
    if max_norm / (norm + 1e-6) >= 1.0 + 2.0 ** -20:
        rc = 0.0 if coef_got == 1.0 else float("inf")
    else:
        rc = abs(coef_got - coef) / (4 * U * coef)
    return rn, rc

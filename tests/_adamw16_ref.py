"""Reference and numerical bar for AdamW with bf16 state (afk_adamw16_step), shared by tests/test_adamw16_cpu.py and tests/test_adamw16_gpu.py.

The bar is derived, not tuned.  Let x be a stored result (p, m or v) and X the same update evaluated in float64 from the same bf16 inputs.  Both
torch's fused kernel and ours compute in fp32 and round once to bf16, so each must satisfy, per element,

    |x - X| <= 2^-8 * |X|  +  2^-20 * A          A_p = |p0| + |update|     A_m = |m0| + |g|     A_v = |v0| + g*g

The first term is half a bf16 ulp (relative to X at most 2^-8); the second is 16 fp32 ulps of the operands of the final sum: it covers the fp32
evaluation order and the cancellation when g ~ -m (near zero a plain ulp distance between two correct results reaches thousands of ulps).  Where
the tolerance is exactly 0 (all operands zero) x must equal X.
"""
import torch


def ref64(p0, m0, v0, g, *, lr, beta1, beta2, eps, weight_decay, bc1, bc2_sqrt, grad_scale=1.0):
    """the update in float64 from the bf16 inputs -> {name: (X, A)} for p, m, v.  bc1 = 1 - beta1^t, bc2_sqrt = sqrt(1 - beta2^t)."""
    p, m, v, g = p0.double(), m0.double(), v0.double(), g.double() * grad_scale
    p1 = p - lr * weight_decay * p
    m1 = m + (1.0 - beta1) * (g - m)
    v1 = beta2 * v + (1.0 - beta2) * g * g
    upd = (lr / bc1) * m1 / (v1.sqrt() / bc2_sqrt + eps)
    return {"p": (p1 - upd, p.abs() + upd.abs()), "m": (m1, m.abs() + g.abs()), "v": (v1, v.abs() + g * g)}


def worst_ratio(x, X, A):
    """max over the elements of |x - X| / tolerance (<= 1 passes); an element whose tolerance is 0 must be exact and counts as 0 or inf"""
    err = (x.double() - X).abs()
    tol = 2.0 ** -8 * X.abs() + 2.0 ** -20 * A
    ratio = torch.where(tol > 0, err / tol.clamp_min(1e-300), torch.where(err == 0, torch.zeros_like(err), torch.full_like(err, float("inf"))))
    return float(ratio.max())


def bias_corrections(beta1, beta2, step):
    return 1.0 - beta1 ** step, (1.0 - beta2 ** step) ** 0.5


def make_params(n, device, seed=0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (0.02 * torch.randn(n, generator=g)).to(torch.bfloat16).to(device)


def make_grad(n, step, device, seed=0):
    """N(0,1) * 10^k, k uniform in -6..-1 per element; every 7th gradient zero on every third step.  (1-b2) * g^2 stays far from bf16 denormals."""
    g = torch.Generator(device="cpu").manual_seed(1000 * seed + step + 1)
    x = torch.randn(n, generator=g) * 10.0 ** torch.randint(-6, 0, (n,), generator=g).float()
    if step % 3 == 2:
        x[::7] = 0.0
    return x.to(torch.bfloat16).to(device)


def restated_fp32(p0, m0, v0, g, *, lr, beta1, beta2, eps, weight_decay, bc1, bc2_sqrt, grad_scale=1.0):
    """csrc/elementwise.hip adamw16_elem restated with fp32 tensors (every product and sum rounded to fp32, no contraction; 1 - beta taken in double and
    rounded to fp32 once, as the C ABI does), rounded to bf16 once: the stand-in the CPU tests launch instead of the kernel"""
    f = lambda c: torch.tensor(c, dtype=torch.float32, device=p0.device)
    w, mm, vv, gr = p0.float(), m0.float(), v0.float(), g.float() * f(grad_scale)
    w = w - (f(lr) * f(weight_decay)) * w
    mm = mm + f(1.0 - beta1) * (gr - mm)
    vv = f(beta2) * vv + (f(1.0 - beta2) * gr) * gr
    denom = vv.sqrt() / f(bc2_sqrt) + f(eps)
    w = w - ((f(lr) / f(bc1)) * mm) / denom
    return w.to(torch.bfloat16), mm.to(torch.bfloat16), vv.to(torch.bfloat16)

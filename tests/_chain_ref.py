"""Operands and references for the decode-chain Linears (csrc/decode_chain.hip) on which every rounding point of the kernels is exact.

x and W hold {-1, 0, 1}, the bias {-2 .. 2}, the residual {-8 .. 8}, the cos / sin tables {-1, 0, 1} drawn independently per (pos, d): every product and every
fp32 sum is a small integer, and every bf16 rounding point of the kernels (the sum, + bias, + residual, the three roundings of rotate-half) is the identity while the
value is an integer with |v| <= 256.  The expected output is then integer arithmetic, whatever the summation order, K split or MFMA shape, and a kernel must return
it bit for bit.  RMSNorm in a prologue: sequence m holds x[m, k] = +-s_m, s_m a power of two that differs between neighbours, so mean(x^2) = s_m^2 and
bf16(x * rstd) = +-1 exactly (eps / s_m^2 <= 1.6e-5 is far inside half a bf16 ulp); the norm weight holds {-1, 1, 2}.  SwiGLU is the one inexact epilogue: the gate
and up sums are exact, the reference is fp64 g * sigmoid(g) * u.

What the integer form cannot see - a row statistic that misses part of a row moves x * rstd by less than half an ulp - is covered by the gaussian cases
(`gaussian()`): all of a row's energy in one window of k, against the same restatement with bf16 roundings where the kernels round.

Everything is torch fp64 / int64 on the device it is given (fp64 sums of small integers are exact); `reference()` asserts the conditions above for every case, and
takes the mutations the CPU test states its sensitivity controls with."""
from types import SimpleNamespace

import torch

F64, I64 = torch.float64, torch.int64
LIMIT = 256          # integers up to here are bf16 values (8 significant bits)
EPS = 1e-6
VAR = 256.0          # target variance of a dot product: sigma 16, six sigma inside LIMIT / 2 (rotate-half adds two of them)
P_TABLE = 128        # rows of the cos / sin tables

M_ALL = (1, 2, 3, 4, 5, 7, 8, 9, 12, 16, 17, 23, 32)
K_MFMA = (64, 128, 576, 1088, 4160)      # 1 / 2 / 9 / 17 / 65 blocks of 64
K_DOT = (8, 520) + K_MFMA                # the dot-product and single-sequence forms also take K % 8
HEADS = ((4, 2, 64), (2, 1, 32), (3, 1, 128), (1, 1, 16))   # (Hq, Hkv, D); D = 16: dot-product forms only

SINGLE = ("qkv", "linear_residual", "gate_up", "lm_head")
PLAIN_BATCHED = ("qkv_batched", "linear_residual_batched", "gate_up_batched", "lm_head_batched")
NORM_BATCHED = ("qkv_norm_batched", "gate_up_norm_batched", "lm_head_norm_batched")
PIPE_ONLY = NORM_BATCHED + ("linear_residual_ss_batched", "linear_residual_norm_batched")
ENTRIES = SINGLE + PLAIN_BATCHED + PIPE_ONLY
KIND = {"qkv": "qkv", "linear_residual": "lin", "gate_up": "gu", "lm_head": "head"}
NORM_IN_PROLOGUE = ("qkv", "gate_up", "lm_head") + NORM_BATCHED

MUTATIONS = ("drop_last_8", "drop_last_64", "double_k", "row_last", "neighbour_pos", "neighbour_s", "swap_table_halves", "swap_gate_up")


def kind_of(entry):
    return KIND[entry.replace("_norm_batched", "").replace("_ss_batched", "").replace("_batched", "")]


# ------------------------------------------------------------------------------------------------ operands
def _ternary(shape, g, density):
    v = torch.randint(0, 2, shape, generator=g, dtype=I64) * 2 - 1
    return v * (torch.rand(shape, generator=g) < density)


def _weights(N, K, g, ex2):
    """[N, K] in {-1, 0, 1}: as dense as keeps the variance of a dot product at VAR, every column used by some row, every row by some column"""
    W = _ternary((N, K), g, min(2.0 / 3.0, VAR / (K * ex2)))
    cols = (~(W != 0).any(0)).nonzero().flatten()
    W[cols % N, cols] = 1 - 2 * (cols % 2)
    rows = (~(W != 0).any(1)).nonzero().flatten()
    W[rows, rows % K] = 1
    return W


def make(kind, M, K, seed, norm=False, N=None, I=None, heads=None, target=False, n2=False, rows=None, s_e0=-2):
    """one case: kind "qkv" | "lin" | "gu" | "head", M sequences, reduction length K.
    norm: the rows arrive raw (+-s_m) and the Linear's prologue normalises them;  rows (with s_e0): these raw rows instead of drawn ones;
    target (lin): the residual is chosen so that out[m] = +-2^(m % 5) - rows the NEXT norm is exact on;  n2 (lin): that norm's weight, its output is expected"""
    g = torch.Generator().manual_seed(seed)
    c = SimpleNamespace(kind=kind, M=M, K=K, norm=norm, seed=seed, gauss=False, heads=heads, I=I, target=target, n2w=None)
    m = torch.arange(M)
    if norm:
        c.s = 2.0 ** ((m % 5) + s_e0).to(F64)
        sign = rows.sign().to(F64) if rows is not None else (torch.randint(0, 2, (M, K), generator=g, dtype=I64) * 2 - 1).to(F64)
        c.x = sign * c.s[:, None]
        c.nw = torch.tensor([-1, 1, 2], dtype=I64)[torch.randint(0, 3, (K,), generator=g)].to(F64)
        ex2 = 2.0
    else:
        c.x = torch.randint(-1, 2, (M, K), generator=g, dtype=I64).to(F64)
        ex2 = 2.0 / 3.0
    if kind == "qkv":
        Hq, Hkv, D = heads
        c.N = (Hq + 2 * Hkv) * D
        c.bias = torch.randint(-2, 3, (c.N,), generator=g, dtype=I64).to(F64)
        c.cos = torch.randint(-1, 2, (P_TABLE, D), generator=g, dtype=I64).to(F64)
        c.sin = torch.randint(-1, 2, (P_TABLE, D), generator=g, dtype=I64).to(F64)
        c.pos = (7 * m + 3) % P_TABLE            # every sequence its own position
    elif kind == "gu":
        c.N = 2 * I
    else:
        c.N = N
    c.W = _weights(c.N, K, g, ex2).to(F64)
    if kind == "lin":
        if target:   # out = +-s2_m with integer s2_m: the rows of the launch that follows are exact for ITS norm
            c.s2 = 2.0 ** (m % 5).to(F64)
            c.out_rows = (torch.randint(0, 2, (M, c.N), generator=g, dtype=I64) * 2 - 1).to(F64) * c.s2[:, None]
            c.res = c.out_rows - c.x @ c.W.T
        else:
            c.res = torch.randint(-8, 9, (M, c.N), generator=g, dtype=I64).to(F64)
        if n2:
            assert target
            c.n2w = torch.tensor([-1, 1, 2], dtype=I64)[torch.randint(0, 3, (c.N,), generator=g)].to(F64)
    # the k element the "doubled" mutation doubles: one that sequence 0 does not multiply by zero
    nz = (c.x[0] != 0).nonzero().flatten()
    c.k_mut = int(nz[len(nz) // 2]) if len(nz) else 0
    return c


def gaussian(kind, M, K, seed, window, norm=True, N=None, I=None, heads=None, n2=False):
    """a case of bf16 gaussians at the scale the project's bars were set at (weights 1.2 / sqrt(K)): all of a row's energy in x[:, window[0]:window[1]].
    n2 (lin): the energy of the OUTPUT rows sits in their last 8 columns instead (the statistic of the norm that follows the Linear)"""
    g = torch.Generator().manual_seed(seed)
    bf = lambda t: t.to(torch.bfloat16).to(F64)
    c = SimpleNamespace(kind=kind, M=M, K=K, norm=norm, seed=seed, gauss=True, heads=heads, I=I, target=False, n2w=None, s=None)
    c.x = torch.zeros((M, K), dtype=F64)
    lo, hi = window
    c.x[:, lo:hi] = bf(torch.randn((M, hi - lo), generator=g) * (1.0 + torch.arange(M)[:, None]))   # rows of different norms
    c.nw = bf(1 + 0.1 * torch.randn((K,), generator=g))
    if kind == "qkv":
        Hq, Hkv, D = heads
        c.N = (Hq + 2 * Hkv) * D
        c.bias = bf(0.1 * torch.randn((c.N,), generator=g))
        c.cos = bf(torch.rand((P_TABLE, D), generator=g) * 2 - 1)
        c.sin = bf(torch.rand((P_TABLE, D), generator=g) * 2 - 1)
        c.pos = (7 * torch.arange(M) + 3) % P_TABLE
    elif kind == "gu":
        c.N = 2 * I
    else:
        c.N = N
    scale = 1.2 / K ** 0.5 if norm else 1.2 / (hi - lo) ** 0.5
    c.W = bf(torch.randn((c.N, K), generator=g) * scale)
    if kind == "lin":
        c.res = bf(torch.randn((M, c.N), generator=g))
        if n2:
            c.W[:-8] = 0
            c.res[:, :-8] = 0
            c.n2w = bf(1 + 0.1 * torch.randn((c.N,), generator=g))
    c.k_mut = lo
    return c


# ------------------------------------------------------------------------------------------------ the reference
def _rb(v):
    """round to bf16 (the gaussian cases)"""
    return v.to(torch.float32).to(torch.bfloat16).to(F64)


def _exact(v, what):
    """a rounding point of an integer case: the value must be an integer with |v| <= LIMIT, so that the kernel's bf16 rounding is the identity"""
    assert bool((v == v.round()).all()), f"{what}: not an integer"
    assert float(v.abs().max()) <= LIMIT, f"{what}: |v| = {float(v.abs().max())} > {LIMIT}: lower the weight density for this K or change the seed"
    return v


def _normalise(rows, w, s, r, check, blind=False):
    """w * bf16(rows * rstd), cast before the weight multiply.  Integer cases (s given): rows = +-s_m, so the cast value is +-1 exactly"""
    if s is not None:
        xn = rows / s[:, None]
        if check:
            assert bool((xn.abs() == 1).all()), "a row in front of a norm is not +-s_m"
            assert EPS / float(s.min()) ** 2 <= 1.6e-5
        return xn * w
    stat = rows * 0 if blind else rows        # blind: a statistic that misses the window holding the row's energy
    rstd = (1.0 / ((stat * stat).mean(1) + EPS).sqrt()).to(torch.float32).to(F64)
    return r(w * r(rows * rstd[:, None]))


def reference(c, dev="cpu", mut=None):
    """-> dict of fp64 tensors on dev: what the launch must write.  mut: one of MUTATIONS (a wrong kernel, stated on the reference; no exactness asserts)"""
    f = lambda t: t.to(dev, F64)
    strict = mut is None and not c.gauss
    # a rounding point: bf16 rounding (gaussian cases), the identity - asserted to be (integer cases), or nothing (a mutated reference)
    rr = (lambda v, what="": _rb(v)) if c.gauss else _exact if strict else (lambda v, what="": v)
    x, W = f(c.x), f(c.W)
    M, K = c.M, c.K
    if strict:
        assert bool((W != 0).any(0).all()) and bool((W != 0).any(1).all()), "every k column and every row needs a nonzero weight"
        if c.kind == "qkv":
            assert len({(int(p), float(s)) for p, s in zip(c.pos, c.s if c.norm else [1.0] * M)}) == M, "two sequences share (pos, s_m)"
    if c.norm:
        s = None if c.gauss else f(c.s)
        if mut == "neighbour_s":
            s = s.roll(1)
        h = _normalise(x, f(c.nw), s, rr, strict, blind=mut == "stat_misses_window")
    else:
        h = x
    h = h.clone()
    if mut == "drop_last_8":
        h[:, -8:] = 0
    elif mut == "drop_last_64":
        h[:, -64:] = 0
    elif mut == "double_k":
        h[:, c.k_mut] *= 2
    elif mut == "row_last":
        h = h[M - 1:].expand(M, K)
    if mut == "swap_gate_up":
        W = torch.cat([W[c.I:], W[:c.I]])
    y = h @ W.T
    if c.kind == "qkv":
        Hq, Hkv, D = c.heads
        nq, nk, half = Hq * D, Hkv * D, D // 2
        y = rr(y + f(c.bias), "sum + bias")
        pos = c.pos.roll(1) if mut == "neighbour_pos" else c.pos
        cos, sin = f(c.cos)[pos.to(dev)], f(c.sin)[pos.to(dev)]      # [M, D]
        if mut == "swap_table_halves":
            cos, sin = torch.cat([cos[:, half:], cos[:, :half]], 1), torch.cat([sin[:, half:], sin[:, :half]], 1)
        rot = y[:, :nq + nk].reshape(M, Hq + Hkv, D)
        a, b = rot[..., :half], rot[..., half:]
        c1, c2, s1, s2 = cos[:, None, :half], cos[:, None, half:], sin[:, None, :half], sin[:, None, half:]
        first = rr(rr(a * c1, "a cos") + rr(-b * s1, "b sin"), "first half")      # a cos[d] - b sin[d]
        second = rr(rr(b * c2, "b cos") + rr(a * s2, "a sin"), "second half")     # b cos[d + D/2] + a sin[d + D/2]
        rot = torch.cat([first, second], -1).reshape(M, nq + nk)
        return dict(q=rot[:, :nq], k=rot[:, nq:], v=y[:, nq + nk:])
    if c.kind == "lin":
        out = rr(rr(y, "sum") + f(c.res), "sum + residual")
        if strict:
            _exact(f(c.res), "residual")
        d = dict(out=out)
        if c.N % 16 == 0:   # what the ss form leaves: every 16-column block's share of sum(out^2) per sequence
            d["ss"] = (out * out).reshape(M, c.N // 16, 16).sum(-1)
            assert c.gauss or float(d["ss"].max()) < 2 ** 24
        if c.n2w is not None:
            s2 = None if c.gauss else f(c.s2)
            if mut == "neighbour_s":
                s2 = s2.roll(1)
            d["h"] = _normalise(out, f(c.n2w), s2, rr, strict, blind=mut == "stat_misses_window")
        return d
    if c.kind == "gu":
        gate, up = rr(y[:, :c.I], "gate sum"), rr(y[:, c.I:], "up sum")
        act = gate * torch.sigmoid(gate) * up
        if c.gauss:
            act = _rb(_rb(gate * torch.sigmoid(gate)) * up)
        return dict(act=act, gate=gate, up=up)
    logits = rr(y, "logit")
    d = dict(logits=logits)
    if c.N % 8 == 0:        # per eight rows: (max, first index of the max)
        g8 = logits.reshape(M, c.N // 8, 8)
        d["part_val"] = g8.max(-1).values
        d["part_idx"] = g8.argmax(-1) + 8 * torch.arange(c.N // 8, device=logits.device)   # torch.argmax: the first of equals
        d["token"] = (logits == logits.max(-1, keepdim=True).values).to(torch.int8).argmax(-1)
    return d


def applies(c, mut):
    if mut == "drop_last_64":
        return c.K % 64 == 0
    if mut == "row_last":
        return c.M >= 2
    if mut == "neighbour_pos":
        return c.kind == "qkv" and c.M >= 2
    if mut == "neighbour_s":
        return c.M >= 2 and (c.norm or c.n2w is not None)
    if mut == "swap_table_halves":
        return c.kind == "qkv"
    if mut == "swap_gate_up":
        return c.kind == "gu"
    return True


# ------------------------------------------------------------------------------------------------ the shape grid
def _seed(entry, n):
    return 1000 * (ENTRIES.index(entry) + 1) + n


def grid(entry, M=None):
    """the cases of an entry point, each list of the issue against it where its guard admits the value: every M with two K's (the single-sequence entries: every
    K), the other sizes cycling.  Every second case is strided.  -> list of (case, strided)"""
    kind = kind_of(entry)
    single, pipe_only = entry in SINGLE, entry in PIPE_ONLY
    norm = entry in NORM_IN_PROLOGUE
    out = []
    if single:
        pairs = [(1, K, n) for n, K in enumerate(K_DOT)]
    else:
        Ms = M_ALL[:7] if entry == "linear_residual_norm_batched" else M_ALL
        pairs = []
        for i, m in enumerate(Ms):
            Ks = K_DOT if (not pipe_only and m <= 8) else K_MFMA
            pairs += [(m, Ks[(2 * i + j) % len(Ks)], 2 * i + j) for j in range(2)]
    for m, K, n in pairs:
        if M is not None and m != M:
            continue
        dot = not pipe_only and m <= 8       # shapes only the dot-product / single-sequence forms take
        pick = lambda full, pipe: (full if dot else pipe)[n % len(full if dot else pipe)]
        kw = {}
        if kind == "qkv":
            kw["heads"] = pick(HEADS, HEADS[:3])
        elif kind == "lin":
            if entry == "linear_residual_ss_batched":
                kw.update(N=(64, 192)[(n // 2 + n) % 2], target=n % 2 == 1)
            elif entry == "linear_residual_norm_batched":
                kw.update(N=(32, 160)[(n // 2 + n) % 2], target=True, n2=True)
            else:
                kw["N"] = pick((8, 32, 160), (32, 160))
        elif kind == "gu":
            kw["I"] = pick((4, 16, 48, 528), (16, 48, 528))
        else:
            kw["N"] = pick((8, 32, 1000, 1056), (32, 1056))
        out.append((make(kind, m, K, _seed(entry, n), norm=norm, **kw), n % 2 == 1))
    if kind == "head" and (M is None or M == (1 if single else 8 if not pipe_only else 32)):
        # the forms that switch at rows / 32 >= 1024 (matrix pipe: four K slices of 32-row groups) and rows / 8 >= 2048 (single sequence: one wave per group)
        out.append((make("head", 1 if single else 8 if not pipe_only else 32, 128, _seed(entry, 99), norm=norm, N=32768), False))
    return out

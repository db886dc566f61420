"""Operands and references for the training / prefill GEMMs (csrc/gemm.hip, gemm256.hip, gemm256t.hip) on which every rounding point of the kernels is exact.

a and b hold {-1, 0, 1}, bias {-4 .. 4}, residual, accumulate base and the saved gate|up of the SwiGLU backward {-8 .. 8}, the cos / sin tables {-1, 0, 1} per
(position, d), alpha is one of {1, 0.5, 2, -1}.  Every product and every fp32 partial sum is a small integer, alpha * sum a multiple of 1/2, and every value a kernel
stores as bf16 - the output, bf16(alpha * sum + bias) in front of a residual or a GELU (`preact`), the three roundings of rotate-half - is a bf16 value with
|v| <= 256, asserted here on the reference (`_exact`): a condition on the inputs, not a tolerance.  The expected output is then arithmetic in fp64 whatever the
tile, K split, MFMA shape or summation order, and a kernel must return it bit for bit.  The density of non-zeros falls with K (`density`) so that the sums stay
inside the bound.  The two activations are the inexact epilogues: their inputs (preact, gate|up, dh) are exact, their outputs are held to tests/_norm_ref.py.

Edge planting: the k indices at the first and last place of every 64-wide K tile (every split starts and ends on one) and the last 8 in front of the end of the
reduction are non-zero in every row of a and b; the rows of a / b at the first and last place of every 128-wide output tile (hence of every 256-wide one) and
the last row are non-zero at every k.  A mistake confined to one (m, n, k) triple on such edges changes the output for certain; in the interior a dropped k changes a
density^2 share of the outputs it touches.

`reference(c, mut=)` restates one way a kernel could be wrong (MUTATIONS); tests/test_gemm_ref_cpu.py shows that each changes the reference of every case it
applies to.  `grid()` is the list of cases tests/test_gemm_exact_gpu.py launches, each with the kernel it must run on (a `kernel_counts` family).  `tile_of` is the
host mirror of gemm_tile_of (csrc/gemm_common.h).  torch only, no GPU import."""
import zlib
from types import SimpleNamespace

import torch

F64, I64, BF = torch.float64, torch.int64, torch.bfloat16
LIMIT = 256          # integers up to here are bf16 values (8 significant bits)
VAR = 400.0          # target variance of alpha * (a dot product) in the interior: sigma 20; an edge row against an edge column has variance alpha^2 K
BK = 64              # K tile of every MFMA kernel
GEMV_BK = 512        # K block of the weight-streaming kernel
P_TABLE = 48         # rows of the cos / sin tables (S = 32 and 16 positions behind it)
HEAD = 128           # columns of a rotated head

KERNELS = ("nt128", "nt256", "nn256", "tn256", "gemv")
FAMILY = {"nt128": "gemm_nt128", "nt256": "gemm_nt256", "nn256": "gemm_nn256", "tn256": "gemm_tn256", "gemv": "gemv"}
FORM = {"nt128": "nt", "nt256": "nt", "nn256": "nn", "tn256": "tn", "gemv": "nt"}
GEMM_BIAS, GEMM_GELU, GEMM_RESIDUAL, GEMM_OUT_F32, GEMM_ACCUM, GEMM_SWIGLU_BWD, GEMM_SWIGLU_FWD = 1, 2, 4, 8, 16, 32, 64   # include/afk.h
# epilogue -> flags.  "narrow" is plain with C 8- but not 16-byte aligned; "f32_half" an fp32 C 16- but not 32-byte aligned: both leave the 16-byte epilogue form
EPI_FLAGS = {"plain": 0, "narrow": 0, "bias": GEMM_BIAS, "residual": GEMM_RESIDUAL, "bias_residual": GEMM_BIAS | GEMM_RESIDUAL, "res_mod": GEMM_RESIDUAL,
             "gelu": GEMM_BIAS | GEMM_GELU, "f32": GEMM_OUT_F32, "f32_half": GEMM_OUT_F32, "accum": GEMM_ACCUM, "accum_bias": GEMM_ACCUM | GEMM_BIAS,
             "accum_f32": GEMM_ACCUM | GEMM_OUT_F32, "swiglu_fwd": GEMM_SWIGLU_FWD, "swiglu_bwd": GEMM_SWIGLU_BWD, "rope_lanes": 0, "rope_pos": 0, "rope_bias": GEMM_BIAS}
NT256_OWN = (0, 1, 4, 5, 3, 7, 16, 64, 32)       # epilogues with an instantiation of their own in gemm256.hip (AFK_EPI_LIST; the RoPE pair goes by its own entry)
XT_OWN = (0, 16)                                 # gemm256t.hip

MUTATIONS = ("drop_k", "double_k", "drop_k_tile", "drop_split", "double_split", "row_next", "row_prev", "col_next", "col_prev", "ragged_short", "ragged_long",
             "bias_next", "bias_prev", "res_row_unwrapped", "ignore_accumulate", "ignore_alpha", "swap_swiglu_halves", "rope_partner_head")


def cdiv(a, b):
    return -(-a // b)


# ------------------------------------------------------------------------------------------------ the launch geometry, restated
def tile_of(bid, nwg, ntm, ntn, gm):
    """gemm_tile_of (csrc/gemm_common.h), line by line (default build: no raw dispatch order) -> (tm, tn)"""
    xcd, idx, q, r = bid & 7, bid >> 3, nwg >> 3, nwg & 7
    swz = (xcd * (q + 1) if xcd < r else r * (q + 1) + (xcd - r) * q) + idx
    GM = (gm & 0x3f) if (gm & 0x3f) > 0 else 4
    per_group = GM * ntn
    g = swz // per_group
    rem = swz - g * per_group
    first_m = g * GM
    gsz = min(ntm - first_m, GM)
    return first_m + rem % gsz, rem // gsz


def split_ranges(kernel, K, splits):
    """[k0, k1) of every split: K tiles (gemv: blocks of 512) [all * s / splits, all * (s + 1) / splits), the last one cut at K"""
    unit = GEMV_BK if kernel == "gemv" else BK
    n = cdiv(K, unit)
    return [(min(K, n * s // splits * unit), min(K, n * (s + 1) // splits * unit)) for s in range(splits)]


def is_wide(c):
    """GemmArgs::wide with the buffers the GPU test lays out (every leading dimension a multiple of 8, every pointer 16-byte aligned but C of the two forms below)"""
    return c.N % 8 == 0 and c.epi not in ("narrow", "f32_half")


def generic(c):
    """does the launch run a runtime-flag instantiation of a 256x256 kernel (counted as gemm_generic_epilogue)?"""
    flags = EPI_FLAGS[c.epi]
    if c.kernel == "nt256":
        return not is_wide(c) or (flags not in NT256_OWN and not c.epi.startswith("rope"))
    if c.kernel in ("nn256", "tn256"):
        return c.splits == 1 and (not is_wide(c) or flags not in XT_OWN)
    return False


def edge_k(K):
    ks = {k for k in range(K) if k % BK in (0, BK - 1)} | set(range(max(0, K - 8), K))
    return sorted(ks)


def edge_rows(R):
    return sorted({r for r in range(R) if r % 128 in (0, 127)} | {R - 1})


def density(K, alpha):
    return min(2.0 / 3.0, (VAR / (K * max(1.0, alpha * alpha))) ** 0.5)


# ------------------------------------------------------------------------------------------------ operands
def _ternary(shape, g, d):
    v = torch.randint(0, 2, shape, generator=g, dtype=I64) * 2 - 1
    return v * (torch.rand(shape, generator=g) < d)


def _signs(shape, g):
    return torch.randint(0, 2, shape, generator=g, dtype=I64) * 2 - 1


def _operand(R, K, g, d):
    """[R, K] in {-1, 0, 1} at density d, the edge rows and the edge k columns fully +-1"""
    t = _ternary((R, K), g, d)
    rows, ks = torch.tensor(edge_rows(R)), torch.tensor(edge_k(K))
    t[rows] = _signs((len(rows), K), g)
    t[:, ks] = _signs((R, len(ks)), g)
    return t.to(F64)


def _ints(shape, g, lim):
    return torch.randint(-lim, lim + 1, shape, generator=g, dtype=I64).to(F64)


def make(kernel, M, N, K, seed, epi="plain", splits=1, alpha=1.0, res_mod=0, group="", gm=None, strided=False, sub=False):
    """one case.  a [M, K] and b [N, K] are the LOGICAL operands (out = a b^T); the GPU test stores them as the form wants them"""
    assert kernel in KERNELS and epi in EPI_FLAGS
    g = torch.Generator().manual_seed(seed)
    flags = EPI_FLAGS[epi]
    c = SimpleNamespace(kernel=kernel, form=FORM[kernel], family=FAMILY[kernel], M=M, N=N, K=K, seed=seed, epi=epi, flags=flags, splits=splits, alpha=float(alpha),
                        res_mod=res_mod, group=group, gm=gm, strided=strided, sub=sub, bias=None, res=None, base=None, gu=None, cos=None, sin=None, pos=None,
                        rope_cols=0, S=0)
    d = density(K, alpha)
    c.a, c.b = _operand(M, K, g, d), _operand(N, K, g, d)
    c.a_next, c.b_next = _signs((M,), g).to(F64), _signs((N,), g).to(F64)      # the k = K column a mask one too long would let in
    if flags & GEMM_BIAS:
        c.bias = _ints((N,), g, 4)
        c.bias[::2] = c.bias[::2].abs() + 1                                     # no two neighbours equal: a bias read one column off always shows
        c.bias[1::2] = -c.bias[1::2].abs()
    if flags & GEMM_RESIDUAL:
        c.res = _ints((max(M, res_mod), N), g, 8)                               # rows [0, res_mod) are the table; the rest is what an unwrapped row index would read
        if res_mod and M > res_mod:
            c.res[res_mod:] = c.res[res_mod:] + 17
    if flags & GEMM_ACCUM:
        c.base = _ints((M, N), g, 8)
        c.base[c.base == 0] = 3                                                 # an ignored accumulate shows everywhere
    if flags & GEMM_SWIGLU_BWD:
        c.gu = _ints((M, 2 * N), g, 8)
    if epi.startswith("rope"):
        c.cos, c.sin = _ints((P_TABLE, HEAD), g, 1), _ints((P_TABLE, HEAD), g, 1)
        c.S, c.rope_cols = 32, 256
        c.pos = (7 * torch.arange(M)) % P_TABLE if epi == "rope_pos" else None
    live = (c.a != 0).any(0) & (c.b != 0).any(0)
    live[torch.tensor(edge_k(K))] = False
    interior = live.nonzero().flatten().tolist()
    c.k_mut = interior[len(interior) // 2] if interior else K // 2              # the k the "dropped" / "doubled" mutations take: an interior one where there is one
    return c


# ------------------------------------------------------------------------------------------------ the reference
def _exact(v, what, f32=False):
    """a rounding point: the value must be one of its format with |v| <= LIMIT, so that the kernel's rounding is the identity"""
    back = v.to(torch.float32).double() if f32 else v.to(BF).double()
    assert torch.equal(back, v), f"{what}: not a {'fp32' if f32 else 'bf16'} value"
    assert float(v.abs().max()) <= LIMIT, f"{what}: |v| = {float(v.abs().max())} > {LIMIT}: lower the density for this K or change the seed"
    return v


def reference(c, dev="cpu", mut=None):
    """-> dict of fp64 tensors on dev: what the launch must write.  mut: one of MUTATIONS (a wrong kernel, stated on the reference; no exactness asserts)"""
    f = lambda t: None if t is None else t.to(dev, F64)
    strict = mut is None
    rr = _exact if strict else (lambda v, what="", f32=False: v)
    a, b = f(c.a).clone(), f(c.b).clone()
    M, N, K = c.M, c.N, c.K
    if strict:
        for t, what in ((a, "a"), (b, "b")):
            assert bool((t.abs() <= 1).all()) and bool((t[:, edge_k(K)] != 0).all()) and bool((t[edge_rows(t.shape[0])] != 0).all()), f"{what}: edges not planted"
        assert c.splits == 1 or all(k0 < k1 and k0 % BK == 0 for k0, k1 in split_ranges(c.kernel, K, c.splits)), "an empty split"
    ranges = split_ranges(c.kernel, K, c.splits)
    if mut == "drop_k":
        a[:, c.k_mut] = 0
    elif mut == "double_k":
        a[:, c.k_mut] *= 2
    elif mut == "drop_k_tile":
        t = (K - 1) // BK // 2
        a[:, t * BK:(t + 1) * BK] = 0
    elif mut in ("drop_split", "double_split"):
        k0, k1 = ranges[c.splits // 2]
        a[:, k0:k1] *= 0 if mut == "drop_split" else 2
    elif mut in ("row_next", "row_prev"):
        a = a.roll(-1 if mut == "row_next" else 1, 0)
    elif mut in ("col_next", "col_prev"):
        b = b.roll(-1 if mut == "col_next" else 1, 0)
    elif mut == "ragged_short":
        a[:, K - 1] = 0
    elif mut == "swap_swiglu_halves" and c.epi == "swiglu_fwd":
        b = torch.cat([b[N // 2:], b[:N // 2]])
    parts = torch.stack([a[:, k0:k1] @ b[:, k0:k1].T for k0, k1 in ranges])      # fp64 sums of small integers are exact
    prod = parts.sum(0)
    if mut == "ragged_long":
        prod = prod + f(c.a_next)[:, None] * f(c.b_next)[None, :]
    d = {}
    if c.splits > 1 or c.kernel == "gemv":
        d["ws"] = parts                                                           # the fp32 partials of the first pass, [splits, M, N]
        if strict:
            _exact(parts, "split-K partial", f32=True)
    v = prod * (1.0 if mut == "ignore_alpha" else c.alpha)
    if c.bias is not None:
        bias = f(c.bias)
        v = v + (bias.roll(-1) if mut == "bias_next" else bias.roll(1) if mut == "bias_prev" else bias)
    if c.epi == "swiglu_fwd":
        gu = rr(v, "gate|up")
        gate, up = gu[:, :N // 2], gu[:, N // 2:]
        return dict(d, out=gu, h=gate * torch.sigmoid(gate) * up)
    if c.epi == "swiglu_bwd":
        dh, gu = rr(v, "dh"), f(c.gu)
        if mut == "swap_swiglu_halves":
            gu = torch.cat([gu[:, N:], gu[:, :N]], 1)
        G, U = gu[:, :N], gu[:, N:]
        s = torch.sigmoid(G)
        return dict(d, dh=dh, out=torch.cat([dh * U * (s * (1 + G * (1 - s))), dh * (G * s)], 1))
    if c.epi.startswith("rope"):
        y = rr(v, "sum + bias")
        pos = (c.pos if c.pos is not None else torch.arange(M) % c.S).to(dev)
        cos, sin = f(c.cos)[pos], f(c.sin)[pos]                                  # [M, 128]
        nh, half = c.rope_cols // HEAD, HEAD // 2
        rot = y[:, :c.rope_cols].reshape(M, nh, HEAD)
        x1, x2 = rot[..., :half], rot[..., half:]
        p1, p2 = (x1.roll(1, 1), x2.roll(1, 1)) if mut == "rope_partner_head" else (x1, x2)      # the rotate-half partner, from the neighbouring head
        c1, c2, s1, s2 = cos[:, None, :half], cos[:, None, half:], sin[:, None, :half], sin[:, None, half:]
        first = rr(rr(x1 * c1, "x1 cos") + rr(-p2 * s1, "x2 sin"), "first half")
        second = rr(rr(x2 * c2, "x2 cos") + rr(p1 * s2, "x1 sin"), "second half")
        return dict(d, out=torch.cat([torch.cat([first, second], -1).reshape(M, c.rope_cols), y[:, c.rope_cols:]], 1))
    if c.flags & GEMM_GELU:
        pre = rr(v, "preact")
        X = pre
        return dict(d, preact=pre, out=0.5 * X * (1 + torch.erf(X * 0.5 ** 0.5)))
    if c.res is not None:
        res = f(c.res)
        rows = torch.arange(M, device=res.device)
        if c.res_mod and mut != "res_row_unwrapped":
            rows = rows % c.res_mod
        v = rr(v, "sum + bias") + res[rows]
    if c.base is not None and mut != "ignore_accumulate":
        v = v + f(c.base)
    return dict(d, out=rr(v, "out", f32=bool(c.flags & GEMM_OUT_F32)))


def applies(c, mut):
    if mut in ("drop_split", "double_split"):
        return c.splits > 1
    if mut in ("row_next", "row_prev"):
        return c.M >= 2
    if mut in ("ragged_short", "ragged_long"):
        return c.K % BK != 0
    if mut in ("bias_next", "bias_prev"):
        return c.bias is not None
    if mut == "res_row_unwrapped":
        return c.res_mod > 0 and c.M > c.res_mod
    if mut == "ignore_accumulate":
        return c.base is not None
    if mut == "ignore_alpha":
        return c.alpha != 1.0
    if mut == "swap_swiglu_halves":
        return c.epi in ("swiglu_fwd", "swiglu_bwd")
    if mut == "rope_partner_head":
        return c.epi.startswith("rope")
    return True


# ------------------------------------------------------------------------------------------------ the shape grid
NT128_MN = ((128, 128), (129, 132), (136, 260), (8, 128))          # (129, 132): N % 8 = 4, the narrow epilogue
NT128_K = (64, 128, 192, 256, 320, 1280)                           # ring prologue, wrap, steady state
NT128_SPLITS = ((192, 2), (192, 3), (320, 2), (320, 3), (320, 5), (1280, 2), (1280, 3), (1280, 20))   # 2 | 3 tiles, 6 | 7 | 7: ragged last splits; K / 64
NT256_MN = ((256, 256), (264, 260), (8, 512), (520, 264))
NT256_K = (64, 128, 192, 256, 1280)
NT256_K_LONG = 4160
XT_MN = ((8, 8), (256, 256), (264, 264), (520, 264))
NN_K = (64, 128, 192, 1280)
TN_K = (8, 56, 64, 72, 100, 200, 1288, 13, 77, 203)                # the last three: odd reduction lengths, which the guard admits
XT_SPLITS = {"nn256": ((192, 2), (192, 3), (1280, 3), (1280, 16), (1280, 20)),            # 20 = the number of K tiles
             "tn256": ((200, 2), (200, 4), (1288, 3), (1288, 16), (1288, 21), (77, 2))}   # ragged last tile in the last split; 4, 21, 2 = the number of K tiles
REDUCE_CAP = (1544, 1360, 128, 2)                                  # M N / 4 / 256 = 2050.6 blocks: the fold kernel's grid-stride loop runs
GEMV_N = (32, 36, 72, 1000)
GEMV_K = (64, 512, 576, 1088, 4160)
ALPHAS = (0.5, 2.0, -1.0)
EPI_BASIC = ("bias", "residual", "bias_residual", "gelu", "f32", "f32_half", "accum", "accum_f32", "narrow")
EPI_MN = {"nt128": (136, 264), "nt256": (264, 264), "nn256": (264, 264), "tn256": (264, 264)}
RES_MOD, RES_MOD_M = 96, (300, 96)                               # 300 = 3 x 96 + 12: the ragged case (TN wants M % 8 == 0: 304)
TILE_MAP = {"nt128": (648, 384), "nt256": (1288, 776)}             # 6 x 3 tiles of 128 (nwg % 8 = 2, ntm % 4 = 2); 6 x 4 tiles of 256
TILE_MAP_GM = (None, 1, 3, 8)
# refused by gemm_impl: (kernel, M, N, K, splits, what)
REFUSED = (("nt128", 128, 128, 100, 1, "NT: K % 64"), ("nt128", 128, 130, 64, 1, "N % 4"), ("nn256", 256, 260, 64, 1, "NN: N % 8"),
           ("nn256", 256, 256, 72, 1, "NN: K % 64"), ("tn256", 260, 256, 64, 1, "TN: M % 8"), ("tn256", 300, 264, 128, 1, "TN: M % 8"), ("tn256", 8, 8, 64, 2, "more splits than K tiles"),
           ("gemv", 1, 32, 512, 2, "gemv: more splits than blocks of 512"), ("nt128", 128, 128, 4160, 65, "more than 64 splits"))

_GRID = None


def grid():
    """every case the GPU test launches, built once.  c.group names the test that takes it; every second case of a group is strided"""
    global _GRID
    if _GRID is not None:
        return _GRID
    out = []

    def add(kernel, M, N, K, group, **kw):
        k = sum(1 for c in out if c.group == group)
        seed = zlib.crc32(repr((kernel, M, N, K, group, sorted(kw.items()))).encode())     # of the case alone: a case added later moves no other case's operands
        out.append(make(kernel, M, N, K, seed, group=group, strided=k % 2 == 1, **kw))

    for M, N in NT128_MN:
        for K in NT128_K:
            add("nt128", M, N, K, "nt128")
    for i, (K, s) in enumerate(NT128_SPLITS):
        M, N = NT128_MN[i % 3]
        add("nt128", M, N, K, "nt128_splitk", splits=s, epi=("plain", "bias", "accum")[i % 3])
    for M, N in NT256_MN:
        for K in NT256_K:
            add("nt256", M, N, K, "nt256")
    add("nt256", 264, 264, NT256_K_LONG, "nt256")
    for kernel, Ks in (("nn256", NN_K), ("tn256", TN_K)):
        for M, N in XT_MN:
            for K in Ks:
                add(kernel, M, N, K, kernel)
        for i, (K, s) in enumerate(XT_SPLITS[kernel]):
            M, N = XT_MN[1 + i % 3]
            add(kernel, M, N, K, kernel + "_splitk", splits=s, epi=("plain", "bias", "accum")[i % 3])
        add(kernel, 8, 8, XT_SPLITS[kernel][0][0], kernel + "_splitk", splits=2)
        M, N, K, s = REDUCE_CAP
        add(kernel, M, N, K, kernel + "_splitk", splits=s, epi="bias")
    i = 0
    for K in GEMV_K:
        for s in range(1, cdiv(K, GEMV_BK) + 1):
            add("gemv", 1, GEMV_N[i % 4], K, "gemv", splits=s, epi="bias_residual" if i % 3 else "plain")
            i += 1
    for kernel, (M, N) in EPI_MN.items():
        for epi in EPI_BASIC:
            add(kernel, M, N, 128, "epilogues_" + kernel, epi=epi)
        for m in RES_MOD_M:
            add(kernel, 304 if (kernel, m) == ("tn256", 300) else m, N, 128, "epilogues_" + kernel, epi="res_mod", res_mod=RES_MOD)
        for al in ALPHAS:
            add(kernel, M, N, 128, "epilogues_" + kernel, epi=("bias", "accum_bias", "plain")[ALPHAS.index(al)], alpha=al)
        # the shapes of test_gemm_generic_epilogue_instantiations: N % 8 = 4 on NT, bias + residual / accumulate on the transposed-operand kernels
        gN = 260 if kernel.startswith("nt") else 264
        add(kernel, 520, gN, 320, "epilogues_" + kernel, epi="bias_residual")
        add(kernel, 520, gN, 320, "epilogues_" + kernel, epi="accum_bias")
        add(kernel, M, 128, 128, "epilogues_" + kernel, epi="swiglu_bwd")
        add(kernel, 304 if kernel == "tn256" else 300, 256, 192, "epilogues_" + kernel, epi="swiglu_bwd")
    for M, N, K in ((8, 256, 64), (264, 256, 128), (264, 512, 192), (300, 512, 1280)):
        add("nt256", M, N, K, "swiglu_fwd", epi="swiglu_fwd")
    for M, K, epi in ((256, 64, "rope_lanes"), (300, 128, "rope_lanes"), (300, 192, "rope_pos"), (300, 1280, "rope_bias"), (520, 256, "rope_pos"), (72, 64, "rope_bias")):
        add("nt256", M, 512, K, "rope", epi=epi)
    for kernel, (M, N, K) in (("nt128", (129, 132, 128)), ("nt128", (136, 264, 192)), ("nt256", (264, 264, 128)), ("nt256", (8, 512, 64))):
        add(kernel, M, N, K, "sub", sub=True, epi="bias" if N % 8 == 0 else "plain")
    for kernel, (M, N) in TILE_MAP.items():
        for gm in TILE_MAP_GM:
            add(kernel, M, N, 64, "tile_map", epi="accum", gm=gm)
    _GRID = out
    return out

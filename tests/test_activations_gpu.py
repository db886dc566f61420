"""The activation kernels of csrc/elementwise.hip on an MI355X against tests/_norm_ref.py: GELU, SwiGLU, add and ReLU, forward and backward, at one
vector and past the ew_grid cap of 4096 blocks (where every training launch runs), held to float64 within the derived bounds and to the rounded
emulation on all but 5e-3 of the outputs; the values where x * x overflows fp32 inside gelu' and __expf overflows inside the sigmoid; ops.rope_
bit-equal to the torch bf16 expression with and without position ids.

Measured on an MI355X, max error / bound per family (the module prints them):
  gelu 0.999   gelu_bwd 1.000   swiglu 1.000   swiglu_bwd 1.000   add 1.000   (8.4 M outputs each: one of them is always next to a tie of its one
  bf16 rounding, which is the bound; at one vector: 0.72 / 0.89 / 0.94 / 0.87 / 1.000)      extreme inputs: 0.999 - 1.000, all finite
  share off the rounded emulation: gelu 4.7e-6, gelu_bwd 3.4e-5, swiglu 0, swiglu_bwd 1.7e-5, add 0 (cap 5e-3; the fp32 torch versions on the CPU: 1e-4)
  ReLU exact; RoPE bit-equal to the torch bf16 expression in all seven cases, forward and backward.
Module wall time 6 s; the two 8.4 M-element cases take 1.4 s and 2.3 s (float64 references).
"""
import pytest
import torch

from tests import _norm_ref as R

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
NAN = float("nan")
WORST = {}


def _note(family, value):
    WORST[family] = max(WORST.get(family, 0.0), value)
    return value


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    print("\n[activations] max error / bound: " + "; ".join(f"{k} {v:.3f}" for k, v in sorted(WORST.items())))


def _ops():
    from audio_flamingo_amd import ops

    return ops


def _held(family, got, exact, bound, emu, what):
    got = got.cpu()
    assert bool(torch.isfinite(got.float()).all()), (what, "not finite")
    r, sh = _note(family, R.ratio(got, exact, bound)), R.mismatch_share(got, emu)
    print(f"{what}: {r:.3f} of the bound, {sh:.2e} differ from the emulation")
    assert r <= 1.0, (what, r)
    assert sh <= R.SHARE_CAP, (what, "share that differs from the rounded emulation", sh)


SIZES = [R.ACT_ONE, R.ACT_BIG]


@pytest.mark.parametrize("n", SIZES)
def test_gelu(dev, n):
    ops = _ops()
    assert R.ew_past_cap(n // 8) == (n == R.ACT_BIG)
    x, dy = R.act_input("gauss", (n,), 21), R.act_input("gauss", (n,), 22)
    f = R.gelu_ref(x)
    _held("gelu", ops.gelu_fwd(x.to(dev)), f.y, f.y_bound, f.y_r, f"gelu {n}")
    g = R.gelu_bwd_ref(dy, x)
    _held("gelu_bwd", ops.gelu_bwd(dy.to(dev), x.to(dev)), g.dx, g.dx_bound, g.dx_r, f"gelu_bwd {n}")


@pytest.mark.parametrize("n", SIZES)
def test_add_and_relu(dev, n):
    from audio_flamingo_amd import _lib

    ops = _ops()
    a, b = R.act_input("gauss2", (n,), 23), R.act_input("gauss", (n,), 24)
    f = R.add_ref(a, b)
    _held("add", ops.add(a.to(dev), b.to(dev)), f.y, f.y_bound, f.y_r, f"add {n}")
    x = a.clone()
    x[:4] = torch.tensor([0.0, -0.0, 2.0 ** -100, -(2.0 ** -100)]).to(BF)
    xd, dyd = x.to(dev), b.to(dev)
    y = torch.full_like(xd, NAN)
    _lib.call("afk_relu_fwd", xd.data_ptr(), y.data_ptr(), n, ops._stream())
    assert torch.equal(y.cpu().float(), torch.relu(x.float())), "relu"
    dx = torch.full_like(xd, NAN)
    _lib.call("afk_relu_bwd", dyd.data_ptr(), y.data_ptr(), dx.data_ptr(), n, ops._stream())
    assert torch.equal(dx.cpu().float(), torch.where(x.float() > 0, b.float(), torch.zeros(n))), "relu backward"


@pytest.mark.parametrize("rows,I", R.SWIGLU_SHAPES, ids=[f"{r}x{i}" for r, i in R.SWIGLU_SHAPES])
def test_swiglu(dev, rows, I):
    ops = _ops()
    gu, dh = R.act_input("gauss", (rows, 2 * I), 25), R.act_input("gauss", (rows, I), 26)
    f = R.swiglu_fwd_ref(gu)
    _held("swiglu", ops.silu_mul_fwd(gu.to(dev)), f.h, f.h_bound, f.h_r, f"silu_mul_fwd {rows}x{I}")
    g = R.swiglu_bwd_ref(gu, dh)
    _held("swiglu_bwd", ops.silu_mul_bwd(gu.to(dev), dh.to(dev)), g.dgu, g.dgu_bound, g.dgu_r, f"silu_mul_bwd {rows}x{I}")


def test_extreme_inputs(dev):
    """+-0, +-2^-100, +-20, +-200, +-2^100: x * x overflows fp32 inside gelu' (the pdf must come out 0, not NaN), __expf(-g) overflows inside the sigmoid
    (which must come out 0): every output finite and within the bound"""
    ops = _ops()
    x, dy = R.extremes((37, 520), 31), R.gauss((37, 520), 32, 1.0)
    f, g = R.gelu_ref(x), R.gelu_bwd_ref(dy, x)
    y, dx = ops.gelu_fwd(x.to(dev)).cpu(), ops.gelu_bwd(dy.to(dev), x.to(dev)).cpu()
    big = (x.float().abs() >= 200)
    assert int(big.sum()) >= 4 and bool(torch.isfinite(y.float()).all()) and bool(torch.isfinite(dx.float()[big]).all()) and bool(torch.isfinite(dx.float()).all())
    assert _note("gelu [extremes]", R.ratio(y, f.y, f.y_bound)) <= 1.0 and _note("gelu_bwd [extremes]", R.ratio(dx, g.dx, g.dx_bound)) <= 1.0
    I = 520
    gu = torch.cat([R.extremes((37, I), 33), R.gauss((37, I), 34)], 1).contiguous()
    dh = R.gauss((37, I), 35, 1.0)
    fs, gs = R.swiglu_fwd_ref(gu), R.swiglu_bwd_ref(gu, dh)
    h, dgu = ops.silu_mul_fwd(gu.to(dev)).cpu(), ops.silu_mul_bwd(gu.to(dev), dh.to(dev)).cpu()
    low = gu[:, :I].float() == -(2.0 ** 100)
    assert int(low.sum()) >= 1 and bool(torch.isfinite(h.float()).all()) and bool(torch.isfinite(dgu.float()).all())
    assert bool((dgu[:, :I][low] == 0).all()) and bool((dgu[:, I:][low] == 0).all()) and bool((h[low] == 0).all()), "a gate of -2^100: silu and silu' are 0"
    assert _note("swiglu [extremes]", R.ratio(h, fs.h, fs.h_bound)) <= 1.0 and _note("swiglu_bwd [extremes]", R.ratio(dgu, gs.dgu, gs.dgu_bound)) <= 1.0


# ---------------------------------------------------------------------------------------------- RoPE
def _tables(S, D, dev):
    inv = 1.0 / (1e6 ** (torch.arange(0, D, 2, device=dev).float() / D))
    fr = torch.arange(S, device=dev).float()[:, None] * inv[None]
    emb = torch.cat([fr, fr], -1)
    return emb.cos().to(BF), emb.sin().to(BF)


ROPE_CASES = [(64, 4, 2, 8, "none"), (64, 4, 2, 8, "pos"), (128, 28, 4, 8, "none"), (128, 28, 4, 8, "pos"), (64, 28, 4, 5, "pos"), (128, 4, 2, 5, "none"),
              (128, 28, 4, 683, "none")]


@pytest.mark.parametrize("D,Hq,Hkv,S,mode", ROPE_CASES, ids=[f"D{D}-h{Hq}+{Hkv}-S{S}-{m}" for D, Hq, Hkv, S, m in ROPE_CASES])
def test_rope_is_the_torch_bf16_expression(dev, D, Hq, Hkv, S, mode):
    ops = _ops()
    nheads, rows = Hq + Hkv, 3 * S
    n = nheads * D
    ld = n + Hkv * D + 32                      # q | k | v columns and 32 pad columns: only q | k may change
    assert R.ew_past_cap(rows * nheads * (D // 8)) == (S == 683)
    buf = R.gauss((rows, ld), 41, 1.0).to(dev)
    T = S if mode == "none" else 40
    cos, sin = _tables(T, D, dev)
    if mode == "pos":
        # left-padded rows restarting at 0, repeated positions, the last table row, nothing monotone
        p = torch.cat([torch.zeros(3, dtype=torch.int32), torch.arange(S - 3, dtype=torch.int32), torch.full((S,), T - 1, dtype=torch.int32),
                       torch.randint(0, T, (S,), generator=torch.Generator().manual_seed(1), dtype=torch.int32)])
        assert p.numel() == rows and int(p.max()) == T - 1 and bool((p[1:] < p[:-1]).any()) and bool((p[1:] == p[:-1]).any())
        pos, idx = p.to(dev), p.long().to(dev)
    else:
        pos, idx = None, (torch.arange(rows, device=dev) % S)
    for backward in (False, True):
        out = buf.clone()
        ops.rope_(out, cos, sin, S=S, nheads=nheads, D=D, pos=pos, backward=backward)
        want = R.rope_reference(buf[:, :n].reshape(rows, nheads, D), cos[idx], sin[idx], backward).reshape(rows, n)
        assert want.dtype == BF
        diff = out[:, :n].view(torch.int16) != want.view(torch.int16)
        same_value = out[:, :n].float() == want.float()          # +0 and -0 are the same output
        assert bool((~diff | same_value).all()), (f"backward={backward}", "share of outputs off the torch bf16 expression", float((diff & ~same_value).float().mean()))
        assert torch.equal(out[:, n:].view(torch.int16), buf[:, n:].view(torch.int16)), "rope touched the v / pad columns"

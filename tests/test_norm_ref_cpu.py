"""tests/_norm_ref.py held to float64 autograd of the operations it restates (F.layer_norm, transformers' Qwen2RMSNorm, F.gelu, F.silu(g) * u), its
builders' own assertions at the shapes of the GPU cases, its geometry helpers at the values the cases are named for, and the EMULATION HEADROOM: an
fp32 torch version of each operation, rounded at the kernel's rounding points, may differ from the float64 emulation on at most 1e-3 of the outputs
(the GPU modules allow 5e-3) and never by more than the bound.  No GPU."""
import pytest
import torch
import torch.nn.functional as F

from tests import _norm_ref as R

BF = torch.bfloat16
TIGHT = 1e-11


def _close(a, b, what):
    err = float((a - b).abs().max() / b.abs().max().clamp_min(1.0))
    assert err < TIGHT, (what, err)


# ---------------------------------------------------------------------------------------------- references against float64 autograd
@pytest.mark.parametrize("rows,D", [(5, 100), (3, 1280), (7, 8)])
def test_layernorm_reference_is_float64_layer_norm(rows, D):
    x, dy, add = R.gauss((rows, D), 1), R.gauss((rows, D), 2, 1.0), R.gauss((rows, D), 3, 1.0)
    w, b = R.norm_weights(D, 4)
    f = R.ln_fwd(x, w, b)
    xr, wr, br = x.double().requires_grad_(True), w.double().requires_grad_(True), b.double().requires_grad_(True)
    y = F.layer_norm(xr, (D,), wr, br, R.LN_EPS)
    _close(f.y, y.detach(), "y")
    y.backward(dy.double())
    old = R.small_int(D, 5)
    g = R.norm_bwd(x, w, dy, f.mean, f.rstd, rms=False, dx_add=add, dw_old=old, db_old=old)
    _close(g.dx_norm, xr.grad, "dx")
    _close(g.dw, wr.grad + old.double(), "dw")
    _close(g.db, br.grad + old.double(), "db")
    assert torch.equal(g.dx_add, add.double()) and torch.equal(g.dx, R.rb(g.dx_norm) + add.double()) and torch.equal(g.dx_r, R.rb(g.dx))
    plain = R.norm_bwd(x, w, dy, f.mean, f.rstd, rms=False)
    assert torch.equal(plain.dx, plain.dx_norm) and plain.dx_add is None
    cs, _ = R.colsum_ref(g.dx_r.to(BF), old)
    _close(cs, g.dx_r.sum(0) + old.double(), "colsum")


@pytest.mark.parametrize("rows,D", [(5, 100), (3, 1280), (7, 8)])
def test_rmsnorm_reference_is_qwen2_rmsnorm(rows, D):
    from transformers.models.qwen2.modeling_qwen2 import Qwen2RMSNorm

    x, dy = R.gauss((rows, D), 1), R.gauss((rows, D), 2, 1.0)
    w, _ = R.norm_weights(D, 4)
    f = R.rms_fwd(x, w)
    # the module as the model runs it, bf16 in and out: its cast BEFORE the weight multiply is our first rounding point.  Its statistics are fp32, so a
    # few outputs may round the other way - within the bound; a single rounding (y_once) is far from it
    m = Qwen2RMSNorm(D, eps=R.RMS_EPS).to(BF)
    with torch.no_grad():
        m.weight.copy_(w)
        y_bf = m(x)
    assert y_bf.dtype == BF
    assert R.mismatch_share(y_bf, f.y_r) <= R.HEADROOM_CAP and R.ratio(y_bf, f.y, f.y_bound) <= 1.0
    if D >= 100:
        assert R.mismatch_share(y_bf, f.y_once) > 0.05, "rounding once must be told from rounding twice"
    # the unrounded operation and its gradients: the module in float64 (its .to(float32) only touches the statistics' INPUT, so feed it fp32-exact
    # bf16 values and a float64 weight; the product and autograd then run in fp32 / float64) against the plain formula
    xr, wr = x.double().requires_grad_(True), w.double().requires_grad_(True)
    y = wr * (xr * torch.rsqrt(xr.pow(2).mean(-1, keepdim=True) + R.RMS_EPS))
    _close(f.xh * w.double(), y.detach(), "y")
    m32 = Qwen2RMSNorm(D, eps=R.RMS_EPS)
    with torch.no_grad():
        m32.weight.copy_(w.float())
        assert float((m32(x.float()).double() - y.detach()).abs().max()) < 1e-5 * float(y.detach().abs().max())
    y.backward(dy.double())
    g = R.norm_bwd(x, w, dy, None, f.rstd, rms=True)
    _close(g.dx_norm, xr.grad, "dx")
    _close(g.dw_unrounded, wr.grad, "dw from the unrounded xh")
    _close(g.dw, (dy.double() * R.rb(f.xh)).sum(0), "dw from bf16(xh)")
    assert torch.equal(g.xh_b, f.xh_b)


def test_gelu_and_swiglu_references():
    x = R.extremes((40, 64), 1)
    dy = R.gauss((40, 64), 2, 1.0)
    xr = x.double().requires_grad_(True)
    y = F.gelu(xr)
    _close(R.gelu_ref(x).y, y.detach(), "gelu")
    y.backward(dy.double())
    _close(R.gelu_bwd_ref(dy, x).dx, xr.grad, "gelu'")
    gu = torch.cat([R.extremes((40, 24), 3), R.gauss((40, 24), 4)], 1)
    dh = R.gauss((40, 24), 5, 1.0)
    gr = gu.double().requires_grad_(True)
    h = F.silu(gr[:, :24]) * gr[:, 24:]
    f = R.swiglu_fwd_ref(gu)
    _close(f.silu * gu[:, 24:].double(), h.detach(), "swiglu")
    assert torch.equal(f.h, R.rb(f.silu) * gu[:, 24:].double()) and torch.equal(f.h_r, R.rb(f.h))
    h.backward(dh.double())
    _close(R.swiglu_bwd_ref(gu, dh).dgu, gr.grad, "swiglu backward")
    for t in (R.gelu_ref(x).y_bound, R.gelu_bwd_ref(dy, x).dx_bound, f.h_bound, R.swiglu_bwd_ref(gu, dh).dgu_bound):
        assert bool(torch.isfinite(t).all()) and bool((t > 0).all())


def test_rounding_helpers():
    v = torch.tensor([1.0, 1.0 + 2.0 ** -8, 1.99, 2.0, 3.0, -0.75, 0.0, 2.0 ** -100], dtype=torch.float64)
    assert torch.equal(R.hu(v), torch.tensor([2.0 ** -8, 2.0 ** -8, 2.0 ** -8, 2.0 ** -7, 2.0 ** -7, 2.0 ** -9, 0.0, 2.0 ** -108], dtype=torch.float64))
    assert float((R.rb(v) - v).abs()[1]) == 2.0 ** -8, "1 + 2^-8 is a tie: the half unit is attained"
    r = torch.rand(100000, dtype=torch.float64, generator=torch.Generator().manual_seed(0)) * 8 - 4
    assert bool(((R.rb(r) - r).abs() <= R.hu(r)).all()) and float(((R.rb(r) - r).abs() / R.hu(r)).max()) > 0.99
    assert torch.equal(R.flip(v[:3], torch.full((3,), 1e-9, dtype=torch.float64)), torch.tensor([0.0, 2.0 ** -7, 0.0], dtype=torch.float64))
    # exact-sum rule
    assert float(R.sum_err(torch.full((1, 3584), 3.140625, dtype=torch.float64))) == 0 and float(R.sum_err(R.gauss((1, 3584), 1).double())) > 0
    assert float(R.sum_err(torch.zeros((1, 8), dtype=torch.float64))) == 0


# ---------------------------------------------------------------------------------------------- builders at the shapes of the GPU cases
def test_builders_hold_their_properties():
    for kind, builder, rows, D, _ in R.fwd_cases():
        if rows <= 8:
            x = R.norm_input(builder, rows, D)
            assert x.shape == (rows, D) and x.dtype == BF and x.is_contiguous()
    for rows, cols in [(r, c) for r in R.COLSUM_ROWS for c in (8, 200)] + [(5, 4096), (2051, 64), (1027, 2056), (3, 8), (2, 8)]:
        m = R.balanced_int(rows, cols, rows)
        drop, dbl = m[:-1].double().sum(0), torch.cat([m, m[-1:]]).double().sum(0)
        assert bool((drop != m.double().sum(0)).all()) and bool((dbl != m.double().sum(0)).all())
    for rows in (3, 5, 2051):
        for r in R.sharp_rows(rows, 64):
            R.one_hot_rows(rows, r, 64, 7)
    R.extremes((R.ACT_ONE * 2,), 3), R.extremes((37, 520), 4)
    x = R.massive(5, 3584, 1)
    assert float(R.rms_fwd(x, torch.ones(3584)).xh.abs().max()) > 30, "massive: three channels carry the row's energy"
    for rows in (5, 6, 7, 2051):
        z = R.zero_rows(rows, 64, 1)
        assert int((z == 0).all(-1).sum()) == len(R.zero_row_ids(rows))


def test_geometry_helpers():
    assert [R.fwd_vpl_vw(D) for D in R.FWD_D8] == [(1, 8), (1, 8), (3, 8), (3, 8), (7, 8), (7, 8), (16, 8), (16, 8)]
    assert [R.fwd_vpl_vw(D) for D in R.FWD_D4] == [(2, 4), (2, 4), (2, 4), (5, 4), (5, 4), (14, 4), (14, 4), (32, 4), (32, 4)]
    assert all(R.fwd_vpl_vw(D)[0] * 64 * R.fwd_vpl_vw(D)[1] >= D for D in R.FWD_D8 + R.FWD_D4)
    assert all(R.fwd_grid_strides(rows) and R.cdiv(rows, 4) == 2048 + 2 and rows % 4 for rows, _ in R.FWD_STRIDE_CASES)
    assert [R.cols_geometry(rows, 64).blocks for rows in R.BWD_COLS_FOLD_ROWS] == [1, 1, 2, 16, 17, 49, 64, 65]
    assert [R.fold_paths(n) for n in (1, 15, 16, 17, 48, 49, 64, 65)] == [(False, True)] * 5 + [(True, True), (True, False), (True, True)]
    g = R.cols_geometry(2051, 64)
    assert (g.blocks, g.groups, g.cap, g.ragged) == (1024, 1026, 1024, True) and R.second_step_row(2051, 64) == 2048
    for D in (2056, 4096):
        g = R.cols_geometry(1027, D)
        assert (g.blocks, g.groups, g.cap, g.ragged) == (512, 514, 512, True) and R.second_step_row(1027, D) == 1024
    assert R.cols_geometry(5, 2048).cap == 1024 and all(R.bwd_form(D) == "cols" for D in R.BWD_COLS_D)
    assert all(R.bwd_form(D) == "rows" for D in R.BWD_ROWS_D) and R.bwd_form(3584, knob_rows=True) == "rows"
    assert R.rows_form_blocks(2051) == 512 and R.second_step_row(2051, 100) == 2048 and R.rows_form_blocks(5) == 2 and R.rows_form_blocks(1) == 1
    assert [R.cols_geometry(rows, 64, 4).ragged for rows in (1, 5, 6, 7, 2051, 8)] == [True] * 5 + [False]
    assert [R.colsum_geometry(rows).slices for rows in R.COLSUM_ROWS] == list(R.COLSUM_SLICES)
    gs = {rows: R.gelu_cs_geometry(rows) for rows in R.GELU_CS_ROWS}
    assert [gs[r].parts for r in R.GELU_CS_ROWS] == [1, 5, 511, 512, 512, 512, 512]
    assert (gs[513].min_rows, gs[513].max_rows) == (1, 2) and (gs[1541].unrolled, gs[1541].tail) == (True, True) and gs[2049].max_rows == 5
    assert not gs[512].unrolled and gs[2049].unrolled and gs[2049].tail
    assert not R.ew_past_cap(R.ACT_ONE // 8) and R.ew_past_cap(R.ACT_BIG // 8) and R.ew_blocks(R.ACT_BIG // 8) == R.EW_CAP_BLOCKS
    rows, I = R.SWIGLU_SHAPES[-1]
    assert R.ew_past_cap(rows * (I // 8)) and not R.ew_past_cap((rows - 1) * (I // 8)) and (I // 8) & (I // 8 - 1)


# ---------------------------------------------------------------------------------------------- emulation headroom
def _f32_ln(x, w, b):
    xf = x.float()
    m = xf.mean(-1, keepdim=True)
    return ((xf - m) * torch.rsqrt(((xf - m) ** 2).mean(-1, keepdim=True) + R.LN_EPS) * w.float() + b.float()).to(BF)


def _f32_rms(x, w):
    xf = x.float()
    return (w.float() * (xf * torch.rsqrt((xf * xf).mean(-1, keepdim=True) + R.RMS_EPS)).to(BF).float()).to(BF)


def test_emulation_headroom_norms():
    worst = {}
    for kind, builder, rows, D, share in R.fwd_cases():
        x = R.norm_input(builder, rows, D)
        w, b = R.norm_weights(D, 2)
        if kind == "ln":
            f, y32 = R.ln_fwd(x, w, b), _f32_ln(x, w, b)
        else:
            f, y32 = R.rms_fwd(x, w), _f32_rms(x, w)
        assert R.ratio(y32, f.y, f.y_bound) <= 1.0, (kind, builder, rows, D)
        if share:
            k = (kind, builder)
            bad, n, top = worst.get(k, (0, 0, 0.0))
            one = R.mismatch_share(y32, f.y_r)
            assert one <= R.HEADROOM_CAP, (kind, builder, rows, D, one)
            worst[k] = (bad + int((y32.double() != f.y_r).sum()), n + y32.numel(), max(top, one))
    for k, (bad, n, top) in sorted(worst.items()):
        print(f"headroom {k[0]:>3} {k[1]:<14} largest share of a case {top:.2e}, over all its cases {bad / n:.2e}  ({bad} of {n})")


def test_emulation_headroom_activations():
    n = R.ACT_BIG // 8   # an eighth of the GPU's large case: 1 M outputs resolve 1e-3 well
    x, dy = R.act_input("gauss", (n,), 21), R.act_input("gauss", (n,), 22)
    res = {}
    res["gelu"] = R.mismatch_share(F.gelu(x.float()).to(BF), R.gelu_ref(x).y_r)
    xr = x.float().requires_grad_(True)
    F.gelu(xr).backward(dy.float())
    res["gelu_bwd"] = R.mismatch_share(xr.grad.to(BF), R.gelu_bwd_ref(dy, x).dx_r)
    I = 24
    gu, dh = R.act_input("gauss", (n // 48, 2 * I), 23), R.act_input("gauss", (n // 48, I), 24)
    g, u = gu[:, :I].float(), gu[:, I:].float()
    res["swiglu"] = R.mismatch_share((F.silu(g).to(BF).float() * u).to(BF), R.swiglu_fwd_ref(gu).h_r)
    s = torch.sigmoid(g)
    res["swiglu_bwd"] = R.mismatch_share(torch.cat([dh.float() * u * (s * (1 + g * (1 - s))), dh.float() * (g * s)], 1).to(BF), R.swiglu_bwd_ref(gu, dh).dgu_r)
    res["add"] = R.mismatch_share((x.float() + dy.float()).to(BF), R.add_ref(x, dy).y_r)
    for k, v in res.items():
        print(f"headroom {k:<10} {v:.2e}")
        assert v <= R.HEADROOM_CAP, (k, v)


# ---------------------------------------------------------------------------------------------- the wrappers refuse strided tensors
def test_norm_wrappers_refuse_strided_tensors():
    from audio_flamingo_amd import ops

    x = torch.zeros((8, 16), dtype=BF)
    w = torch.zeros(8, dtype=BF)
    st = torch.zeros(16, dtype=torch.float32)
    for call in (lambda: ops.layernorm_fwd(x.t(), w, w), lambda: ops.rmsnorm_fwd(x.t(), w),
                 lambda: ops.layernorm_bwd(x.t(), w, x.t().contiguous(), st, st, w, w), lambda: ops.layernorm_bwd(x.t().contiguous(), w, x.t(), st, st, w, w),
                 lambda: ops.layernorm_bwd(x.t().contiguous(), w, x.t().contiguous(), st, st, w, w, dx_add=x.t()),
                 lambda: ops.rmsnorm_bwd(x.t(), w, x.t().contiguous(), st, w), lambda: ops.rmsnorm_bwd(x.t().contiguous(), w, x.t(), st, w),
                 lambda: ops.rmsnorm_bwd(x.t().contiguous(), w, x.t().contiguous(), st, w, dx_add=x.t())):
        with pytest.raises(AssertionError, match="contiguous"):
            call()

"""csrc/norm.hip on an MI355X against the float64 references and derived bounds of tests/_norm_ref.py (its docstring holds the derivation): both
sides of every launch_fwd boundary, the grid-stride step of the forward, statistics on offset / zero / constant / massive-channel rows, the
column-owned and the row-per-wave backward at every fold part count, ragged last groups and rows past their block caps, one-hot and exact-integer
gradients that make a dropped or doubled row visible, the fused column sums, bit-determinism, and the A/B knobs in fresh child processes.
Inputs and outputs of the forward, and dx of the backward, sit between NaN sentinels; outputs start as NaN, so an unwritten element shows.

Measured on an MI355X, max error / bound per family (the module prints them):
  forward y     1.000 (LayerNorm 0.987-1.000 per builder, RMSNorm 1.000; const_rows 0.000 = bit-equal to the bias, const_rows_any 0.844)
  forward mean  0.736        rstd  0.151 (LayerNorm), 0.106 (RMSNorm)
  dx 1.000   dw 1.000   db 1.000   fused column sums 1.000   RMSNorm dw on the aligned-sign case 0.983
  share of y off the rounded emulation: LayerNorm gauss at most 1.7e-4 of a case, RMSNorm 3.8e-6, every other builder 0 - except const_rows_any under
  LayerNorm (0.3: y = b + cancellation noise there, which is why that builder is held to the bound only)
Every bf16 output sits AT its bound: the bound is one bf16 rounding plus a much smaller fp32 term, and among thousands of outputs one always lands
next to a tie - 1.000 says the bound has no slack, not that the kernel is close to failing.  The fp32 statistics use 11-74 % of their worst-case
bounds: rstd sums D squares whose rounding errors mostly cancel (worst case grows with D, the measured error with sqrt D); the mean is at 0.74 on the
exact-sum rows, where the bound is only the two roundings of sum * (1 / D).
Module wall time 21 s (264 cases); the slowest are the 2051 x 3580 row-per-wave cases (2-3 s, float64 reference) and the two child processes (2 s, 5 s).
"""
import math
import os
import subprocess
import sys

import pytest
import torch

from tests import _norm_ref as R

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
NAN = float("nan")
PAD = 64          # sentinel elements either side (keeps the 16-byte alignment the kernels ask for)
WORST = {}


def _note(family, value):
    WORST[family] = max(WORST.get(family, 0.0), value)
    return value


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    print("\n[norm edges] max error / bound: " + "; ".join(f"{k} {v:.3f}" for k, v in sorted(WORST.items())))


def _ops():
    from audio_flamingo_amd import ops

    return ops


def _lib():
    from audio_flamingo_amd import _lib

    return _lib


class Guarded:
    """a tensor inside a larger allocation whose neighbouring elements are NaN; NaN itself until written"""

    def __init__(self, dev, shape, dtype, src=None):
        self.n = math.prod(shape)
        self.buf = torch.full((self.n + 2 * PAD,), NAN, device=dev, dtype=dtype)
        self.t = self.buf[PAD: PAD + self.n].view(shape)
        if src is not None:
            self.t.copy_(src)

    def intact(self):
        return bool(torch.isnan(self.buf[:PAD]).all()) and bool(torch.isnan(self.buf[PAD + self.n:]).all())


def _same_bits(a, b):
    return torch.equal(a.view(torch.int16), b.view(torch.int16))


# ---------------------------------------------------------------------------------------------- forward
def _fwd(dev, kind, x, w, b):
    rows, D = x.shape
    gx, gy = Guarded(dev, x.shape, BF, x), Guarded(dev, x.shape, BF)
    gm, gr = Guarded(dev, (rows,), torch.float32), Guarded(dev, (rows,), torch.float32)
    wd, bd = w.to(dev), b.to(dev)
    st = _ops()._stream()
    if kind == "ln":
        _lib().call("afk_layernorm_fwd", gx.t.data_ptr(), wd.data_ptr(), bd.data_ptr(), gy.t.data_ptr(), gm.t.data_ptr(), gr.t.data_ptr(), rows, D, R.LN_EPS, st)
    else:
        _lib().call("afk_rmsnorm_fwd", gx.t.data_ptr(), wd.data_ptr(), gy.t.data_ptr(), gr.t.data_ptr(), rows, D, R.RMS_EPS, st)
    torch.cuda.synchronize()
    assert gx.intact() and gy.intact() and gr.intact() and gm.intact(), "a sentinel next to x / y / mean / rstd changed"
    assert _same_bits(gx.t.cpu(), x), "x changed"
    return gy.t.cpu(), (gm.t.cpu() if kind == "ln" else None), gr.t.cpu()


@pytest.mark.parametrize("kind,builder,rows,D,share", R.fwd_cases(), ids=[f"{k}-{b}-{r}x{D}" for k, b, r, D, _ in R.fwd_cases()])
def test_forward(dev, kind, builder, rows, D, share):
    x = R.norm_input(builder, rows, D)
    w, b = R.norm_weights(D, 2)
    vpl, vw = R.fwd_vpl_vw(D)
    assert (vw == 8) == (D % 8 == 0) and vpl * 64 * vw >= D and R.fwd_grid_strides(rows) == (rows > 8192)
    f = R.ln_fwd(x, w, b) if kind == "ln" else R.rms_fwd(x, w)
    y, mean, rstd = _fwd(dev, kind, x, w, b)
    assert bool(torch.isfinite(y.float()).all()) and bool(torch.isfinite(rstd).all()), "an output element was not written (or is not finite)"
    ry = _note(f"{kind} fwd y [{builder}]", R.ratio(y, f.y, f.y_bound))
    rr = _note(f"{kind} fwd rstd", R.ratio(rstd, f.rstd, f.rstd_bound))
    rm = _note("ln fwd mean", R.ratio(mean, f.mean, f.mean_bound)) if kind == "ln" else 0.0
    sh = R.mismatch_share(y, f.y_r)
    print(f"{kind} {builder} {rows}x{D} VPL{vpl}x{vw}: y {ry:.3f} rstd {rr:.3f} mean {rm:.3f} of the bound; {sh:.2e} of y differ from the emulation")
    assert ry <= 1.0, ("y", ry)
    assert rr <= 1.0, ("rstd", rr)
    assert rm <= 1.0, ("mean", rm)
    if share:
        assert sh <= R.SHARE_CAP, ("share of y that differs from the rounded emulation", sh)
    if builder in ("zero_rows", "const_rows") and kind == "ln":
        rows_b = R.zero_row_ids(rows) if builder == "zero_rows" else list(range(rows))
        assert _same_bits(y[rows_b], b.expand(len(rows_b), D).contiguous()), "x - mean is exactly 0 on these rows: y is the bias, bit for bit"
    if builder == "zero_rows":
        eps = R.LN_EPS if kind == "ln" else R.RMS_EPS
        assert bool(((rstd[R.zero_row_ids(rows)].double() - eps ** -0.5).abs() <= 8 * R.E32 * eps ** -0.5).all()), "a padded row: rstd = eps^-1/2"


# ---------------------------------------------------------------------------------------------- backward
def _stats(kind, x, w, b):
    """the fp32 statistics handed to the backward: the float64 ones, rounded (inputs of the reference as well)"""
    if kind == "ln":
        f = R.ln_fwd(x, w, b)
        return f.mean.float(), f.rstd.float()
    return None, R.rms_fwd(x, w).rstd.float()


class Bwd:
    """device copies of one case and the direct C-ABI launch; dx lands in a guarded NaN buffer"""

    def __init__(self, dev, kind, x, w, mean, rstd):
        self.dev, self.kind, self.rows, self.D = dev, kind, x.shape[0], x.shape[1]
        self.x, self.w, self.rstd = x.to(dev), w.to(dev), rstd.to(dev)
        self.mean = mean.to(dev) if mean is not None else None
        self.ws = torch.empty(_lib().load().afk_norm_bwd_blocks(self.rows) * 2 * self.D, device=dev, dtype=torch.float32)

    def __call__(self, dy, add=None, dw_old=None, db_old=None):
        """dy / add on the device; -> dx, dw, db on the CPU (db None for rms)"""
        acc = dw_old is not None
        dw = dw_old.to(self.dev).clone() if acc else torch.full((self.D,), NAN, device=self.dev, dtype=BF)
        db = db_old.to(self.dev).clone() if acc else torch.full((self.D,), NAN, device=self.dev, dtype=BF)
        gdx = Guarded(self.dev, (self.rows, self.D), BF)
        pa = add.data_ptr() if add is not None else 0
        st = _ops()._stream()
        if self.kind == "ln":
            _lib().call("afk_layernorm_bwd", self.x.data_ptr(), self.w.data_ptr(), dy.data_ptr(), self.mean.data_ptr(), self.rstd.data_ptr(), gdx.t.data_ptr(), pa,
                        dw.data_ptr(), db.data_ptr(), int(acc), self.ws.data_ptr(), self.rows, self.D, st)
        else:
            _lib().call("afk_rmsnorm_bwd", self.x.data_ptr(), self.w.data_ptr(), dy.data_ptr(), self.rstd.data_ptr(), gdx.t.data_ptr(), pa, dw.data_ptr(), int(acc),
                        self.ws.data_ptr(), self.rows, self.D, st)
        torch.cuda.synchronize()
        assert gdx.intact(), "a sentinel next to dx changed"
        return gdx.t.cpu(), dw.cpu(), (db.cpu() if self.kind == "ln" else None)


def _check(tag, kind, ref, dx, dw, db, dw_old=None, db_old=None):
    assert bool(torch.isfinite(dx.float()).all()) and bool(torch.isfinite(dw.float()).all()), (tag, "an element of dx / dw was not written")
    r = {"dx": R.ratio(dx, ref.dx, ref.dx_bound)}
    t, bound = R.total(ref.dw_parts, dw_old, ref.n)
    r["dw"] = R.ratio(dw, t, bound)
    if kind == "ln":
        assert bool(torch.isfinite(db.float()).all()), (tag, "an element of db was not written")
        t, bound = R.total(ref.db_parts, db_old, ref.n)
        r["db"] = R.ratio(db, t, bound)
    for k, v in r.items():
        _note(f"{kind} bwd {k}", v)
    print(f"{tag}: " + " ".join(f"{k} {v:.3f}" for k, v in r.items()))
    for k, v in r.items():
        assert v <= 1.0, (tag, k, v)


def _bwd_case(dev, kind, rows, D, x=None, tag=""):
    x = R.gauss((rows, D), 31) if x is None else x
    w, b = R.norm_weights(D, 2)
    dy, add, old = R.gauss((rows, D), 32, 1.0), R.gauss((rows, D), 33, 1.0), R.gauss((D,), 34, 0.5)
    mean, rstd = _stats(kind, x, w, b)
    run = Bwd(dev, kind, x, w, mean, rstd)
    dyd, addd = dy.to(dev), add.to(dev)
    for with_add in (False, True):
        ref = R.norm_bwd(x, w, dy, mean, rstd, rms=kind == "rms", dx_add=add if with_add else None)
        for acc in (False, True):
            o = old if acc else None
            got = run(dyd, addd if with_add else None, o, o)
            _check(f"{kind} {tag}{rows}x{D} add={int(with_add)} acc={int(acc)}", kind, ref, *got, dw_old=o, db_old=o)
            again = run(dyd, addd if with_add else None, o, o)
            assert all(a is None or _same_bits(a, g) for a, g in zip(again, got)), "two launches of the backward differ (not bit-deterministic)"


@pytest.mark.parametrize("kind", ["ln", "rms"])
@pytest.mark.parametrize("rows,D", R.bwd_cols_cases(), ids=[f"{r}x{D}" for r, D in R.bwd_cols_cases()])
def test_backward_column_owned(dev, kind, rows, D):
    g = R.cols_geometry(rows, D)
    assert R.bwd_form(D) == "cols" and g.cap == (512 if D >= 2056 else 1024) and g.ragged == bool(rows % 2)
    if (rows, D) in R.BWD_COLS_PAST_CAP:
        assert g.groups - g.cap == 2 and g.blocks == g.cap and g.ragged   # 1026 groups on 1024 blocks, 514 on 512: two blocks take a second group (other LDS parity)
    print(f"{g.blocks} blocks = fold parts (unrolled, tail) = {R.fold_paths(g.blocks)}, {g.groups} groups")
    _bwd_case(dev, kind, rows, D)


@pytest.mark.parametrize("kind", ["ln", "rms"])
@pytest.mark.parametrize("rows,D", R.bwd_rows_cases(), ids=[f"{r}x{D}" for r, D in R.bwd_rows_cases()])
def test_backward_row_per_wave(dev, kind, rows, D):
    assert R.bwd_form(D) == "rows" and R.fwd_vpl_vw(D)[1] == 4
    assert R.rows_form_blocks(rows) == (512 if rows == 2051 else R.cdiv(rows, 4))
    _bwd_case(dev, kind, rows, D)


def test_workspace_bound_matches_the_library(dev):
    lib = _lib().load()
    for rows in (1, 2, 3, 5, 31, 129, 1027, 2047, 2048, 2049, 2051, 12000):
        assert lib.afk_norm_bwd_blocks(rows) == R.norm_bwd_blocks(rows)
        for D in (64, 2056, 100):
            assert R.bwd_parts(rows, D) <= R.norm_bwd_blocks(rows)


@pytest.mark.parametrize("kind", ["ln", "rms"])
@pytest.mark.parametrize("builder,rows,D", [(b, 5, D) for b in ("zero_rows", "offset") for D in (520, 2056, 100)])   # 64 would make E[x^2] of `offset` an exact integer
def test_backward_statistic_rows(dev, kind, builder, rows, D):
    """a padded (all-zero) row has rstd = eps^-1/2 and xh = 0; an offset row has x - mean a small integer next to |x| ~ 1024"""
    _bwd_case(dev, kind, rows, D, x=R.norm_input(builder, rows, D), tag=builder + " ")


SHARP = [(2051, 64), (1027, 2056), (1027, 4096), (3, 64), (5, 64), (2051, 100), (2051, 3580), (3, 100), (5, 100)]


@pytest.mark.parametrize("kind", ["ln", "rms"])
@pytest.mark.parametrize("rows,D", SHARP, ids=[f"{r}x{D}-{R.bwd_form(D)}" for r, D in SHARP])
def test_backward_edges_made_sharp(dev, kind, rows, D):
    """dy with one live row: dw, db and dx[r] have one term (the rounding bound alone), every other row of dx is its dx_add, or zero.  dy of balanced
    integers: LayerNorm's db IS the exact integer, fresh and accumulated - a dropped, doubled or misplaced row changes every column."""
    x = R.gauss((rows, D), 41)
    w, b = R.norm_weights(D, 2)
    add = R.gauss((rows, D), 43, 1.0)
    mean, rstd = _stats(kind, x, w, b)
    run = Bwd(dev, kind, x, w, mean, rstd)
    addd = add.to(dev)
    live = R.sharp_rows(rows, D)
    if rows > 1024:
        assert R.second_step_row(rows, D) in live and len(live) == 4
    for r in live:
        dy = R.one_hot_rows(rows, r, D, 50 + r)
        dyd = dy.to(dev)
        for with_add in (False, True):
            one = slice(r, r + 1)
            ref = R.norm_bwd(x[one], w, dy[one], None if mean is None else mean[one], rstd[one], rms=kind == "rms", dx_add=add[one] if with_add else None, n_terms=1)
            dx, dw, db = run(dyd, addd if with_add else None)
            _check(f"{kind} {rows}x{D} one-hot row {r} add={int(with_add)}", kind, ref, dx[one], dw, db)
            others = torch.ones(rows, dtype=torch.bool)
            others[r] = False
            want = add[others].float() if with_add else torch.zeros((rows - 1, D))
            assert torch.equal(dx[others].float(), want), f"rows with dy = 0 must come back as their dx_add (or zero): live row {r}"
    if kind == "ln":
        dy = R.balanced_int(rows, D, 61)
        exact = dy.double().sum(0)
        old = R.small_int(D, 62)
        _, _, db = run(dy.to(dev), addd)
        assert torch.equal(db.double(), exact), ("db is not the exact integer column sum", (db.double() - exact).abs().max())
        _, _, db = run(dy.to(dev), None, old, old)
        assert torch.equal(db.double(), exact + old.double()), ("accumulated db is not the exact integer", (db.double() - exact - old.double()).abs().max())


@pytest.mark.parametrize("rows,D", [(129, 64), (129, 100)], ids=["cols", "rows"])
def test_rmsnorm_dw_uses_the_rounded_xh(dev, rows, D):
    """the oracle multiplies dy with the bf16 xh.  dy = sign(xh - bf16(xh)) lines the rounding errors up, so sum dy bf16(xh) and sum dy xh differ by more
    than twice the bound: a kernel within the bound of the first is provably outside the bound of the second"""
    x = R.gauss((rows, D), 71)
    w, _ = R.norm_weights(D, 2)
    f = R.rms_fwd(x, w)
    rstd = f.rstd.float()
    xh = x.double() * rstd.double()[:, None]
    dy = torch.where(xh - R.rb(xh) >= 0, 1.0, -1.0).to(BF)
    ref = R.norm_bwd(x, w, dy, None, rstd, rms=True)
    apart = (ref.dw - ref.dw_unrounded).abs() > 2 * ref.dw_bound
    assert int(apart.sum()) >= D // 2, "the case must separate the two references"
    _, dw, _ = Bwd(dev, "rms", x, w, None, rstd)(dy.to(dev))
    r = _note("rms bwd dw [aligned]", R.ratio(dw, ref.dw, ref.dw_bound))
    assert r <= 1.0, r
    assert bool(((dw.double() - ref.dw_unrounded).abs() > ref.dw_bound)[apart].all()), "dw matches the unrounded xh"


# ---------------------------------------------------------------------------------------------- fused column sums
@pytest.mark.parametrize("rows,D", R.bwd_cols_cases(), ids=[f"{r}x{D}" for r, D in R.bwd_cols_cases()])
def test_layernorm_bwd_colsum(dev, rows, D):
    ops = _ops()
    x, dy, add = R.gauss((rows, D), 31), R.gauss((rows, D), 32, 1.0), R.gauss((rows, D), 33, 1.0)
    w, b = R.norm_weights(D, 2)
    old = R.gauss((D,), 34, 0.5)
    mean, rstd = _stats("ln", x, w, b)
    xd, wd, dyd, addd, md, rd = (t.to(dev) for t in (x, w, dy, add, mean, rstd))

    def run(dyd, addd, acc, fused):
        dw = old.to(dev).clone() if acc else torch.full((D,), NAN, device=dev, dtype=BF)
        db, cs = dw.clone(), dw.clone()
        dx = ops.layernorm_bwd(xd, wd, dyd, md, rd, dw, db, dx_add=addd, accumulate=acc, **(dict(colsum_out=cs, colsum_accumulate=acc) if fused else {}))
        torch.cuda.synchronize()
        return dx.cpu(), dw.cpu(), db.cpu(), cs.cpu()

    for acc in (False, True):
        plain, fused = run(dyd, addd, acc, False), run(dyd, addd, acc, True)
        assert all(_same_bits(a, c) for a, c in zip(plain[:3], fused[:3])), "dx / dw / db of the fused entry differ from the plain entry"
        t, bound = R.colsum_ref(fused[0], old if acc else None)
        assert bool(torch.isfinite(fused[3].float()).all())
        r = _note("ln bwd colsum", R.ratio(fused[3], t, bound))
        print(f"colsum {rows}x{D} acc={int(acc)}: {r:.3f} of the bound")
        assert r <= 1.0, r
        assert all(_same_bits(a, c) for a, c in zip(run(dyd, addd, acc, True), fused)), "two fused launches differ"
    zero = torch.zeros_like(addd)
    for r_ in R.sharp_rows(rows, D):
        dx, _, _, cs = run(R.one_hot_rows(rows, r_, D, 50 + r_).to(dev), zero, False, True)
        t, bound = R.colsum_ref(dx[r_: r_ + 1])
        assert R.ratio(cs, t, bound) <= 1.0 and torch.equal(cs.float(), dx[r_].float()), f"one live row {r_}: the column sums are that row of dx"


# ---------------------------------------------------------------------------------------------- A/B knobs, each in a fresh child process
def _child(tmp_path, env, cases):
    src, dst = tmp_path / "cases.pt", tmp_path / "out.pt"
    torch.save(cases, src)
    child = os.path.join(os.path.dirname(os.path.abspath(__file__)), "_norm_knob_child.py")
    p = subprocess.run([sys.executable, child, str(src), str(dst)], env={**os.environ, **env}, timeout=300, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-2000:]
    return torch.load(dst)


def _knob_case(kind, rows, D, with_add, acc):
    x, dy = R.gauss((rows, D), 81), R.gauss((rows, D), 82, 1.0)
    w, b = R.norm_weights(D, 2)
    mean, rstd = _stats(kind, x, w, b)
    return dict(kind=kind, x=x, w=w, dy=dy, mean=mean, rstd=rstd, dx_add=R.gauss((rows, D), 83, 1.0) if with_add else None,
                dw_old=R.gauss((D,), 84, 0.5) if acc else None)


def _knob_check(tag, c, got):
    ref = R.norm_bwd(c["x"], c["w"], c["dy"], c["mean"], c["rstd"], rms=c["kind"] == "rms", dx_add=c["dx_add"])
    _check(tag, c["kind"], ref, got["dx"], got["dw"], got["db"] if c["kind"] == "ln" else None, dw_old=c["dw_old"], db_old=c["dw_old"])


def test_knob_row_per_wave_form(dev, tmp_path):
    """AFK_NORM_BWD=rows: the row-per-wave form at D % 8 == 0.  It keeps a row in 7 x 64 x 8 = 3584 columns; D = 4096 must be served correctly or
    refused with an error - never a dx with unwritten columns"""
    cases = [_knob_case(kind, 5, D, a, a) for kind in ("ln", "rms") for D in (64, 1280, 3584) for a in (False, True)]
    wide = [_knob_case(kind, 5, 4096, True, False) for kind in ("ln", "rms")]
    out = _child(tmp_path, {"AFK_NORM_BWD": "rows"}, cases + wide)
    assert R.bwd_form(3584, knob_rows=True) == "rows"
    for c, got in zip(cases, out):
        assert "error" not in got, got
        _knob_check(f"knob rows {c['kind']} 5x{c['x'].shape[1]}", c, got)
    for c, got in zip(wide, out[len(cases):]):
        if "error" in got:
            assert "3584" in got["error"] and "row-per-wave" in got["error"], got["error"]
        else:
            _knob_check(f"knob rows {c['kind']} 5x4096", c, got)


def test_knob_four_row_groups(dev, tmp_path):
    """AFK_NORM_BWD_R=4: RMSNorm's 4-row groups; rows 1, 5, 6, 7, 2051 leave ragged last groups of 1, 1, 2, 3 and 3 rows"""
    shapes = [(rows, D) for D in (64, 3584) for rows in (1, 5, 6, 7, 2051)]
    assert [R.cols_geometry(rows, 64, 4).ragged for rows, _ in shapes[:5]] == [True] * 5 and R.cols_geometry(2051, 3584, 4).groups > 512
    cases = [_knob_case("rms", rows, D, a, a) for rows, D in shapes for a in (False, True) if a or rows <= 7]
    out = _child(tmp_path, {"AFK_NORM_BWD_R": "4"}, cases)
    for c, got in zip(cases, out):
        assert "error" not in got, got
        _knob_check(f"knob R=4 rms {c['x'].shape[0]}x{c['x'].shape[1]} add={int(c['dx_add'] is not None)}", c, got)

"""The bias-gradient reductions on an MI355X: ops.colsum (fused and two-launch), ops.rowsum, ops.gelu_bwd(colsum_out=...) against tests/_norm_ref.py.
Integer inputs whose every fp32 partial sum is exact make the column sums EXACT integers - a dropped, doubled or misplaced row changes every column,
where the old sqrt(rows) tolerance hid it; Gaussian inputs are held to the float64 sum within the derived bound; strided views sit in NaN-filled buffers.

Measured on an MI355X, max error / bound per family (the module prints them):
  colsum 0.993   rowsum 1.000   gelu_bwd column sums 0.999   gelu_bwd dx on the extreme inputs 1.000
One bf16 rounding of the total is the whole bound (the fp32 term is gamma(rows) sum|x|, under a percent of it up to 32769 rows), and some column always
rounds from next to a tie: the families sit at the bound because it has no slack.  The integer cases are exact: 0 error, no bound.  Module wall time 2 s.
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
    print("\n[bias grad sums] max error / bound: " + "; ".join(f"{k} {v:.3f}" for k, v in sorted(WORST.items())))


def _ops():
    from audio_flamingo_amd import ops

    return ops


def _same_bits(a, b):
    return torch.equal(a.view(torch.int16), b.view(torch.int16))


def test_geometry_matches_the_library(dev):
    from audio_flamingo_amd import _lib

    lib = _lib.load()
    for rows in R.COLSUM_ROWS + (2, 1024, 1537, 32768, 100000):
        assert lib.afk_colsum_slices(rows) == R.colsum_geometry(rows).slices
    for rows in R.GELU_CS_ROWS + (2, 12000):
        assert lib.afk_gelu_bwd_colsum_parts(rows) == R.gelu_cs_geometry(rows).parts


# ---------------------------------------------------------------------------------------------- colsum
LAYOUTS = ("contiguous", "strided")


def _layout(dev, m, layout):
    """the matrix contiguous, or as a column slice of a wider, longer NaN-filled buffer (ld = cols + 16, 64 NaN rows below the last)"""
    if layout == "contiguous":
        return m.to(dev)
    rows, cols = m.shape
    wide = torch.full((rows + 64, cols + 16), NAN, device=dev, dtype=BF)
    wide[:rows, 8: 8 + cols] = m
    return wide[:rows, 8: 8 + cols]


def _colsum_both(x, base):
    """fused and two-launch form from the same starting out (None = fresh, over NaN); -> out (CPU), asserting the two are bit-equal"""
    ops = _ops()
    cols = x.shape[1]
    res = []
    for fused in (True, False):
        out = base.to(x.device).clone() if base is not None else torch.full((cols,), NAN, device=x.device, dtype=BF)
        assert ops.COLSUM_FUSED
        try:
            ops.COLSUM_FUSED = fused
            ops.colsum(x, out, accumulate=base is not None)
        finally:
            ops.COLSUM_FUSED = True
        res.append(out.cpu())
    assert _same_bits(res[0], res[1]), "the fused colsum differs from the partial + fold launches"
    assert int(ops._colsum_counters(x.device, (cols + 63) // 64).abs().sum()) == 0, "arrival counters not back at zero"
    return res[0]


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("rows,slices", list(zip(R.COLSUM_ROWS, R.COLSUM_SLICES)))
def test_colsum_exact_integers(dev, rows, slices, layout):
    assert R.colsum_geometry(rows).slices == slices
    for cols in R.COLSUM_COLS:
        m = R.balanced_int(rows, cols, rows + cols)
        exact = m.double().sum(0)
        old = R.small_int(cols, cols)
        x = _layout(dev, m, layout)
        got = _colsum_both(x, None)
        assert torch.equal(got.double(), exact), (cols, "fresh column sums are not the exact integers", float((got.double() - exact).abs().max()))
        got = _colsum_both(x, old)
        assert torch.equal(got.double(), exact + old.double()), (cols, "accumulated column sums are not the exact integers")


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("rows,slices", [(33, 1), (513, 2), (1025, 3), (3585, 8), (4097, 9), (32769, 64)])
def test_colsum_gauss(dev, rows, slices, layout):
    assert R.colsum_geometry(rows).slices == slices
    m, old = R.gauss((rows, 72), rows), R.gauss((72,), 5, 0.5)
    for base in (None, old):
        t, bound = R.colsum_ref(m, base)
        r = _note("colsum", R.ratio(_colsum_both(_layout(dev, m, layout), base), t, bound))
        print(f"colsum {rows}x72 {layout} acc={int(base is not None)}: {r:.3f} of the bound")
        assert r <= 1.0, r


# ---------------------------------------------------------------------------------------------- rowsum
@pytest.mark.parametrize("C", R.ROWSUM_C)
def test_rowsum(dev, C):
    ops = _ops()
    ld = (C + 7) // 8 * 8 + 8
    for rows in R.ROWSUM_ROWS:
        for kind in ("int", "gauss"):
            m = R.balanced_int(C, rows, 10 * C + rows).t().contiguous() if kind == "int" else R.gauss((rows, C), C + rows)
            xt = torch.full((rows, ld), NAN, device=dev, dtype=BF)
            xt[:, :C] = m
            old = R.small_int(rows, rows)
            for base in (None, old):
                buf = torch.full((rows + 16,), NAN, device=dev, dtype=BF)
                out = buf[8: 8 + rows]
                if base is not None:
                    out.copy_(base)
                ops.rowsum(xt, C, out, accumulate=base is not None)
                torch.cuda.synchronize()
                assert bool(torch.isnan(buf[:8]).all()) and bool(torch.isnan(buf[8 + rows:]).all()), "rowsum wrote outside its rows"
                t, bound = R.rowsum_ref(m, C, base)
                got = out.cpu()
                if kind == "int":
                    assert torch.equal(got.double(), t), (rows, C, "row sums of exact integers", got.tolist())
                r = _note("rowsum", R.ratio(got, t, bound))
                assert r <= 1.0, (rows, C, kind, r)


# ---------------------------------------------------------------------------------------------- GELU backward with the bias gradient
GELU_CS_CASES = [(rows, 8) for rows in R.GELU_CS_ROWS] + [(513, C) for C in R.GELU_CS_WIDE_C]


def _pre(rows, C):
    if rows * C >= 4 * len(R.EXTREME_VALUES):
        return R.extremes((rows, C), rows + C)
    return torch.tensor(R.EXTREME_VALUES[2:2 + rows * C]).to(BF).view(rows, C)


@pytest.mark.parametrize("rows,C", GELU_CS_CASES, ids=[f"{r}x{c}" for r, c in GELU_CS_CASES])
def test_gelu_bwd_colsum(dev, rows, C):
    ops = _ops()
    g = R.gelu_cs_geometry(rows)
    print(f"{g.parts} parts, {g.min_rows}..{g.max_rows} rows per block, unrolled={g.unrolled} tail={g.tail}; fold (unrolled, tail) = {R.fold_paths(g.parts)}")
    pre, dy, old = _pre(rows, C), R.gauss((rows, C), 7, 1.0), R.gauss((C,), 8, 0.5)
    pred, dyd = pre.to(dev), dy.to(dev)
    plain = ops.gelu_bwd(dyd, pred).cpu()
    ref = R.gelu_bwd_ref(dy, pre)
    assert bool(torch.isfinite(plain.float()).all()), "gelu_bwd is not finite on the extreme inputs"
    r = _note("gelu_bwd dx [extremes]", R.ratio(plain, ref.dx, ref.dx_bound))
    assert r <= 1.0, r
    for base in (None, old):
        cs = base.to(dev).clone() if base is not None else torch.full((C,), NAN, device=dev, dtype=BF)
        dx = ops.gelu_bwd(dyd, pred, colsum_out=cs, colsum_accumulate=base is not None).cpu()
        assert _same_bits(dx, plain), "dx of the column-owned form differs from gelu_bwd"
        t, bound = R.colsum_ref(dx, base)
        assert bool(torch.isfinite(cs.float()).all())
        rc = _note("gelu_bwd colsum", R.ratio(cs.cpu(), t, bound))
        print(f"gelu_bwd colsum {rows}x{C} acc={int(base is not None)}: {rc:.3f} of the bound")
        assert rc <= 1.0, rc
    for r_ in sorted({0, rows - 1, 512} & set(range(rows))):
        one = R.one_hot_rows(rows, r_, C, 9 + r_)
        cs = torch.full((C,), NAN, device=dev, dtype=BF)
        dx = ops.gelu_bwd(one.to(dev), pred, colsum_out=cs).cpu()
        t, bound = R.colsum_ref(dx[r_: r_ + 1])
        assert R.ratio(cs.cpu(), t, bound) <= 1.0 and torch.equal(cs.cpu().float(), dx[r_].float()), f"one live row {r_}: the column sums are that row of dx"
        others = torch.ones(rows, dtype=torch.bool)
        others[r_] = False
        assert bool((dx[others] == 0).all())

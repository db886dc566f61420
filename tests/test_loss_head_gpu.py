"""The training loss head on an MI355X against the float64 reference of tests/_ce_ref.py: ce_fwd_bwd_kernel at real vocabulary shapes, scalar
tails, strided rows and extreme inputs; count_valid / loss_reduce; the chunk loop of autograd_ops.lm_head_loss.  All through the C ABI.

Bounds (derived, not measured):
  row_loss   |got - ref| <= 2e-4 |ref| + 1e-5                          (the bar tests/test_ops_gpu.py::test_cross_entropy holds the mean to)
  dlogits    |got - ref| <= 2^-7 |ref| + 1e-6 scale,  scale = upstream / max(denom, 1)
             the output is ONE bf16 rounding of an fp32 value and fp32 noise may flip that rounding by an ulp: 2^-7 relative; at the label
             p - 1 cancels in fp32: a few 2^-24 scale absolute.
Measured on an MI355X, worst over every argument combination of a case, as FRACTIONS OF THE BOUND, row_loss / gradient (the test prints them):
  rows x V      9x5        9x8        70x2048     16x2048 ld2112  24x2053     24x6285     8x152064
  random3       .0012/.44  .0097/.47  .0003/.48   .0002/.48       .0004/.49   .0002/.48   .0003/.46
  offset_up     .011/.43   .019/.44   .0039/.47   .0033/.49       .0033/.48   .0039/.46   .0020/.43
  offset_down   .059/.42   .057/.44   .0045/.47   .0044/.43       .0047/.45   .0030/.45   .0042/.43
  spike         0/.25      0/.25      0/.25       0/.38           0/.23       0/.23       0/.25
  ramp_up       .0002/.25  .0035/.25  .0019/.47   .0019/.40       .0010/.46   .0016/.46   .0006/.27
  ramp_down     .0002/.25  .0035/.25  .0019/.47   .0019/.40       .0010/.46   .0016/.46   .0006/.27
  ramp_perm     .0002/.25  .0035/.25  .0013/.47   .0007/.39       .0004/.46   .0010/.46   .0005/.27
  masked        -          -          .0004/.49   .0002/.48       .0005/.48   .0003/.48   .0003/.46
The gradient sits at half its bound - one bf16 rounding (2^-8) and nothing else; the row loss uses at most 6 % of its bound (the +-200 offsets,
where one fp32 ulp of the log-sum-exp is 1.5e-5).  Before the kernel skipped vectors with nothing finite yet, the masked cases at V = 2053,
6285 and 152064 returned NaN losses and gradients on every labelled row.
The chunked lm_head_loss: loss 9.887560 against 9.887560, relative L2 error of dX 1.7e-3 and of dW 2.4e-3 (rows given) / 2.6e-3 (rows=None).
"""
import itertools

import pytest
import torch

from tests import _ce_ref as R
from tests._tol import GRAD_REL_L2, LOSS_ATOL

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
SENTINEL_BITS = 0x7B7B        # a finite, huge bf16 (1.3e36): read by mistake it wrecks the row, written over it shows
ROW_LOSS_SENTINEL = -12345.0
GIVEN_DENOM = 37.0            # a denominator that is not the label count (the reference's num_items_in_batch path)


def _ops():
    from audio_flamingo_amd import ops

    return ops


def _launch(dev, case, x, labels, denom, upstream, write_grad):
    """the case's rows as a view [1 : rows + 1, :V] of a sentinel-filled [rows + 2, ld] buffer -> (buffer, its state before the call, row_loss
    buffer [rows + 2])"""
    buf = torch.empty((case.rows + 2, case.ld), device=dev, dtype=BF)
    buf.view(torch.int16).fill_(SENTINEL_BITS)
    buf[1: case.rows + 1, : case.V] = x
    before = buf.clone()
    row_loss = torch.full((case.rows + 2,), ROW_LOSS_SENTINEL, device=dev, dtype=torch.float32)
    _ops().ce_fwd_bwd_(buf[1: case.rows + 1, : case.V], labels, row_loss[1: case.rows + 1], denom, upstream=upstream, write_grad=write_grad)
    return buf, before, row_loss


def _outside_untouched(case, buf, before, row_loss, what):
    keep = torch.ones(buf.shape, dtype=torch.bool, device=buf.device)
    keep[1: case.rows + 1, : case.V] = False
    moved = (buf.view(torch.int16) != before.view(torch.int16)) & keep
    assert not bool(moved.any()), (case.name, what, "wrote outside the rows' V columns at (buffer row, column)", moved.nonzero()[:8].tolist())
    assert float(row_loss[0]) == ROW_LOSS_SENTINEL and float(row_loss[-1]) == ROW_LOSS_SENTINEL, (case.name, what, "row_loss written out of range")


@pytest.mark.parametrize("name", [c.name for c in R.CASES])
def test_ce_kernel_against_float64(dev, name):
    ops = _ops()
    case = R.CASE_BY_NAME[name]
    x_cpu, lab_cpu = R.inputs(name)
    ref_loss, ref_g = R.expected(name)
    x, labels = x_cpu.to(dev), lab_cpu.to(dev)
    valid = lab_cpu >= 0
    counted = ops.count_valid(labels)
    assert float(counted) == int(valid.sum())
    worst_loss = worst_grad = 0.0
    first = None
    for upstream, denom_kind in itertools.product((1.0, 0.25), ("count", GIVEN_DENOM, 0.0)):
        if denom_kind == 0.0 and upstream != 1.0:
            continue
        denom = counted if denom_kind == "count" else torch.tensor([denom_kind], device=dev, dtype=torch.float32)
        scale = upstream / max(float(denom), 1.0)
        what = f"upstream={upstream} denom={float(denom)}"
        buf, before, row_loss = _launch(dev, case, x, labels, denom, upstream, True)
        _outside_untouched(case, buf, before, row_loss, what)
        got_loss = row_loss[1:-1].cpu().double()
        got_g = buf[1: case.rows + 1, : case.V].cpu().double()
        assert bool(torch.isfinite(got_loss).all()) and bool(torch.isfinite(got_g).all()), (name, what, "non-finite loss or gradient",
                                                                                            (~torch.isfinite(got_loss)).nonzero().flatten().tolist())
        assert bool((got_loss[~valid] == 0).all()) and bool((got_g[~valid] == 0).all()), (name, what, "ignored rows: loss 0, gradient 0")
        e_loss = (got_loss - ref_loss).abs() / (2e-4 * ref_loss.abs() + 1e-5)
        e_grad = (got_g - ref_g * scale).abs() / (2.0 ** -7 * (ref_g * scale).abs() + 1e-6 * scale)
        worst_loss, worst_grad = max(worst_loss, float(e_loss.max())), max(worst_grad, float(e_grad.max()))
        r, (gr, gc) = int(e_loss.argmax()), divmod(int(e_grad.argmax()), case.V)
        msg = (f"{name} {what}: worst row_loss error {float(e_loss.max()):.3g} of its bound (row {r}: {float(got_loss[r]):.9g} vs {float(ref_loss[r]):.9g}); "
               f"worst gradient error {float(e_grad.max()):.3g} of its bound (row {gr} col {gc} label {int(lab_cpu[gr])}: {float(got_g[gr, gc]):.6g} vs "
               f"{float(ref_g[gr, gc] * scale):.6g})")
        assert float(e_loss.max()) <= 1.0 and float(e_grad.max()) <= 1.0, msg
        if first is None:
            first = (buf, row_loss, denom)
    print(f"CE_MARGIN {name}: row_loss {worst_loss:.3g} gradient {worst_grad:.3g} (fractions of the bounds)")
    # two runs on the same input are bit-equal
    buf, row_loss, denom = first
    buf2, _, row_loss2 = _launch(dev, case, x, labels, denom, 1.0, True)
    assert torch.equal(buf.view(torch.int16), buf2.view(torch.int16)) and torch.equal(row_loss, row_loss2), (name, "not bit-deterministic")
    # write_grad = False: the logits (and everything around them) bit-identical, the same row_loss as with the gradient
    buf3, before3, row_loss3 = _launch(dev, case, x, labels, denom, 1.0, False)
    assert torch.equal(buf3.view(torch.int16), before3.view(torch.int16)), (name, "write_grad=False changed the buffer")
    assert torch.equal(row_loss3, row_loss), (name, "write_grad=False wrote another row_loss")


@pytest.mark.parametrize("rows,V,ld", R.SHAPES)
@pytest.mark.parametrize("write_grad", [True, False])
def test_ce_kernel_all_rows_ignored(dev, rows, V, ld, write_grad):
    """every label -100: count 0 (the kernel divides by max(denom, 1)), zero gradient in the V columns only, zero row losses, zero loss"""
    ops = _ops()
    case = R.Case("all-ignored", None, rows, V, ld)
    x = R.inputs(f"random3-{rows}x{V}" + (f"-ld{ld}" if ld != V else ""))[0].to(dev)
    labels = torch.full((rows,), R.IGNORE, device=dev, dtype=torch.int64)
    denom = ops.count_valid(labels)
    assert float(denom) == 0.0
    buf, before, row_loss = _launch(dev, case, x, labels, denom, 1.0, write_grad)
    _outside_untouched(case, buf, before, row_loss, f"write_grad={write_grad}")
    inner = buf[1: rows + 1, :V]
    if write_grad:
        assert bool((inner.view(torch.int16) == 0).all()), "ignored rows: +0 in every one of the V columns"
    else:
        assert torch.equal(inner, x)
    assert bool((row_loss[1:-1] == 0).all())
    loss = torch.full((1,), float("nan"), device=dev)
    ops.loss_reduce(row_loss[1:-1], denom, loss)
    assert float(loss) == 0.0


# ---------------------------------------------------------------------------------------------- count_valid / loss_reduce
@pytest.mark.parametrize("n", [1, 1023, 1024, 4099])
def test_count_valid_and_loss_reduce(dev, n):
    """single-block reductions over more elements than the block has threads, with a ragged count: the exact count; the loss against a float64
    sum within 1e-6 relative (fp32 sums of positive terms: <= 5 per thread, then a 1024-leaf tree - a few 2^-24); accumulate adds to the prior
    value and overwrite ignores a garbage one; bit-deterministic"""
    ops = _ops()
    g = torch.Generator().manual_seed(n)
    labels = torch.randint(0, 152064, (n,), generator=g)
    labels[torch.rand(n, generator=g) < 0.3] = R.IGNORE
    if n > 1:
        labels[-1], labels[0] = 5, R.IGNORE
    count = int((labels >= 0).sum())
    denom = ops.count_valid(labels.to(dev))
    assert float(denom) == count
    assert torch.equal(ops.count_valid(labels.to(dev)), denom)
    row_loss = (torch.rand(n, generator=g) * 12.0).float()
    row_loss[labels < 0] = 0.0
    want = float(row_loss.double().sum()) / max(count, 1)
    rl = row_loss.to(dev)
    loss = torch.full((1,), float("nan"), device=dev)          # garbage that accumulate=False must not read
    ops.loss_reduce(rl, denom, loss, accumulate=False)
    assert abs(float(loss) - want) <= 1e-6 * abs(want), (float(loss), want)
    again = torch.full((1,), 7.0, device=dev)
    ops.loss_reduce(rl, denom, again, accumulate=False)
    assert torch.equal(again, loss), "loss_reduce not bit-deterministic"
    prior = 3.25
    acc = torch.full((1,), prior, device=dev)
    ops.loss_reduce(rl, denom, acc, accumulate=True)
    assert abs(float(acc) - (prior + want)) <= 1e-6 * abs(prior + want), (float(acc), prior + want)
    # a denominator that is not the count, and one below 1
    for d in (GIVEN_DENOM, 0.0):
        out = torch.zeros(1, device=dev)
        ops.loss_reduce(rl, torch.tensor([d], device=dev), out)
        w = float(row_loss.double().sum()) / max(d, 1.0)
        assert abs(float(out) - w) <= 1e-6 * abs(w), (d, float(out), w)


# ---------------------------------------------------------------------------------------------- the chunk loop of autograd_ops.lm_head_loss
CHUNK, H, V_CHUNKED, M_ALL, M_LABELLED = 128, 128, 4160, 500, 356


@pytest.fixture(scope="module")
def chunk_problem():
    """x [500, 128], w [4160, 128] (2 or 3 vectors per thread), 356 labelled rows: chunks of 128, 128 and 100 rows.  Reference in float64 from
    the bf16 x and w with the logits rounded to bf16 (as the kernel path and the oracle's bf16 lm_head round them): loss, dX = dlogits . W,
    dW = dlogits^T . X"""
    assert R.vectors_per_thread(V_CHUNKED) == (2, 3) and V_CHUNKED % 64 == 0
    g = torch.Generator().manual_seed(5)
    x = torch.randn(M_ALL, H, generator=g).to(BF)
    w = (torch.randn(V_CHUNKED, H, generator=g) * 0.15).to(BF)
    labels = torch.full((M_ALL,), R.IGNORE, dtype=torch.int64)
    rows = torch.randperm(M_ALL, generator=g)[:M_LABELLED].sort().values
    labels[rows] = torch.randint(0, V_CHUNKED, (M_LABELLED,), generator=g)
    logits = (x.double() @ w.double().t()).to(BF)
    _, dlogits, loss = R.reference(logits, labels, M_LABELLED, 1.0)
    return dict(x=x, w=w, labels=labels, rows=rows, loss=float(loss), dx=dlogits @ w.double(), dw=dlogits.t() @ x.double())


def _rel_l2(got, ref):
    return float((got.double().cpu() - ref).norm() / ref.norm())


@pytest.mark.parametrize("with_rows", [True, False], ids=["rows", "rows_none"])
def test_lm_head_loss_chunk_loop(dev, monkeypatch, chunk_problem, with_rows):
    """autograd_ops.lm_head_loss with three or four chunks, the last one ragged: the weight gradient accumulates across chunks, the label and
    row-loss slices follow the chunk, unlabelled rows get an exactly zero dX, and an upstream gradient of 0.5 scales both gradients exactly"""
    from audio_flamingo_amd import autograd_ops as A

    P = chunk_problem
    monkeypatch.setattr(A._LMHeadLoss, "CHUNK", CHUNK)
    seen = []
    real = A.ops.ce_fwd_bwd_

    def spy(logits, *a, **k):
        seen.append(logits.shape[0])
        return real(logits, *a, **k)

    monkeypatch.setattr(A.ops, "ce_fwd_bwd_", spy)
    labels = P["labels"].to(dev)
    rows = P["rows"].to(dev) if with_rows else None

    def run(upstream):
        x = P["x"].to(dev).requires_grad_(True)
        w = P["w"].to(dev).requires_grad_(True)
        del seen[:]
        loss = A.lm_head_loss(x, w, labels, rows)
        chunks = list(seen)
        (upstream * loss).backward()
        torch.cuda.synchronize()
        return float(loss.detach()), x.grad, w.grad, chunks

    loss, dx, dw, chunks = run(1.0)
    assert chunks == ([128, 128, 100] if with_rows else [128, 128, 128, 116]), chunks
    assert len(chunks) >= 3 and chunks[-1] < CHUNK, "at least three chunks, the last one ragged"
    e_dx, e_dw = _rel_l2(dx, P["dx"]), _rel_l2(dw, P["dw"])
    msg = f"loss {loss:.6f} vs {P['loss']:.6f}; rel-L2 dX {e_dx:.4g}, dW {e_dw:.4g}"
    print("CHUNK_MARGIN", "rows" if with_rows else "rows_none", msg)
    assert abs(loss - P["loss"]) <= LOSS_ATOL and e_dx <= GRAD_REL_L2 and e_dw <= GRAD_REL_L2, msg
    unlabelled = (P["labels"] < 0).to(dev)
    assert bool((dx[unlabelled] == 0).all()), "unlabelled rows of dX are exactly zero"
    loss_h, dx_h, dw_h, _ = run(0.5)
    assert loss_h == loss
    assert torch.equal(dx_h.float(), 0.5 * dx.float()) and torch.equal(dw_h.float(), 0.5 * dw.float()), "upstream 0.5 is an exact scaling"

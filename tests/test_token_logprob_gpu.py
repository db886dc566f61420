"""Differentiable per-token log-probabilities from the fused lm_head on an MI355X: the two kernels of csrc/token_logprob.hip through the C ABI against the
float64 reference of tests/_logprob_ref.py, the chunk loop of autograd_ops.lm_head_logprob, and forward(labels=, return_token_logprobs=True) of the model.

Bounds of the kernel tests (derived, not measured; eps = 2^-24):
  logp, lse  |got - ref| <= 2e-4 |ref| + 1e-5: the bound tests/test_loss_head_gpu.py holds row_loss to - the arithmetic is the same sweep, and logp is
             asserted BIT-EQUAL to -row_loss of afk_ce_fwd_bwd(write_grad = 0), with and without the entropy output.
  gradient   |got - ref| <= 2^-7 |ref| + 1e-6 |u_row|: ONE bf16 rounding of an fp32 value (fp32 noise may flip it by an ulp); at the label 1 - p cancels
             in fp32: a few eps |u| absolute.  (That file's derivation with the row's u in place of scale.)
  entropy    H = log s - t / s with d_c = x_c - m <= 0 (exact in fp32: both are bf16 values), s = sum e^d, t = sum e^d d.  Every term of both sums has one
             sign, so a relative error delta_c of term c moves the sum by at most its share.  Per term, in units of eps:
               e^d from __expf = exp2(d log2 e): the argument's rounding scaled by the derivative |d|, + 2 for the instruction          |d| + 2
               the product e^d d                                                                                                       1
               the online rescales e^(m - mx): a thread rescales at most once per vector it walks, per tail step and once to the block
               maximum - R <= n + 1 factors (n = ceil(V / 8 / 256) + 1), each (|step| + 2), the steps summing to at most |d|:           |d| + 2 R
               additions: 8 inside a vector + n down the thread + 10 across the block, half an ulp each:                               (n + 18) / 2
             (a term below 2^-126 is flushed to zero: V such terms weigh less than 1e-30 against s >= 1)
             delta_c <= (2 |d_c| + C) eps,  C = 3 + 2 (n + 1) + (n + 18) / 2.  With E[.] the mean under p = softmax(x):
               |ds| / s <= (2 E|d| + C) eps,   |dt| / s <= (2 E d^2 + C E|d|) eps,   |t| / s = E|d|,  (E|d|)^2 <= E d^2
               |d(t / s)| <= |dt| / s + E|d| |ds| / s <= (4 E d^2 + 2 C E|d|) eps
               |d log s|  <= |ds| / s + 2 eps |log s|;   the division and the subtraction: eps (E|d| + |log s|)
             |dH| <= eps (4 E d^2 + (2 C + 3) E|d| + C + 3 |log s|)            (tests/_logprob_ref.py::entropy_bound; 1.3e-4 at 8 x 152064 random3)
             The +-200 offset cases are compared with the float64 entropy of the row with the offset taken out again: what the shifted form is for.
Measured on an MI355X, worst fractions of the bounds over the 55 cases (the test prints them per case as LOGPROB_MARGIN): logp <= 0.059 (the +-200 offsets at
V = 5), lse <= 0.00055, entropy <= 0.11 (ramp_perm 16 x 2048; 0.0003 - 0.025 at V = 152064), gradient 0.15 - 0.49 - one bf16 rounding and nothing else.
The chunked lm_head_logprob: max |logp - ref| 3.5e-5, relative L2 error of dX 2.3e-3 and of dW 2.8e-3 (rows given) / 2.9e-3 (rows=None).

The model tests use the smooth tiny golden (tiny64_smooth_state_bf16.pt, case D: B = 2, S = 792, 41 scored positions per row) at the bars of tests/_tol.py.
"""
import os

import pytest
import torch

from tests import _logprob_ref as L
from tests._tol import FLOOR_FACTOR, GRAD_REL_L2, LOSS_ATOL, logit_tol

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
SENTINEL_BITS = 0x7B7B        # a finite, huge bf16 (1.3e36): read by mistake it wrecks the row, written over it shows
VEC_SENTINEL = -12345.0
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, "tests", "golden")


def _ops():
    from audio_flamingo_amd import ops

    return ops


def _afk_error():
    from audio_flamingo_amd._lib import AfkError

    return AfkError


# ---------------------------------------------------------------------------------------------- the kernels
def _buffer(dev, case, x):
    """the case's rows as a view [1 : rows + 1, :V] of a sentinel-filled [rows + 2, ld] buffer"""
    buf = torch.empty((case.rows + 2, case.ld), device=dev, dtype=BF)
    buf.view(torch.int16).fill_(SENTINEL_BITS)
    buf[1: case.rows + 1, : case.V] = x
    return buf


def _vec(dev, case):
    return torch.full((case.rows + 2,), VEC_SENTINEL, device=dev, dtype=torch.float32)


def _forward(dev, case, x, labels, with_entropy):
    buf = _buffer(dev, case, x)
    before = buf.clone()
    logp, lse, ent = _vec(dev, case), _vec(dev, case), (_vec(dev, case) if with_entropy else None)
    r = slice(1, case.rows + 1)
    _ops().token_logprob(buf[r, : case.V], labels, logp[r], lse[r], None if ent is None else ent[r])
    assert torch.equal(buf.view(torch.int16), before.view(torch.int16)), (case.name, "the forward wrote to the chunk (or around it)")
    for name, v in (("logp", logp), ("lse", lse), ("entropy", ent)):
        if v is not None:
            assert float(v[0]) == VEC_SENTINEL and float(v[-1]) == VEC_SENTINEL, (case.name, name, "written outside [rows]")
    return logp[r], lse[r], None if ent is None else ent[r]


def _backward(dev, case, x, labels, lse, u):
    buf = _buffer(dev, case, x)
    before = buf.clone()
    lse_b, u_b = _vec(dev, case), _vec(dev, case)
    r = slice(1, case.rows + 1)
    lse_b[r], u_b[r] = lse, u
    lse_0, u_0 = lse_b.clone(), u_b.clone()
    _ops().token_logprob_bwd_(buf[r, : case.V], labels, lse_b[r], u_b[r])
    keep = torch.ones(buf.shape, dtype=torch.bool, device=dev)
    keep[r, : case.V] = False
    moved = (buf.view(torch.int16) != before.view(torch.int16)) & keep
    assert not bool(moved.any()), (case.name, "the backward wrote outside the rows' V columns at (buffer row, column)", moved.nonzero()[:8].tolist())
    assert torch.equal(lse_b.view(torch.int32), lse_0.view(torch.int32)) and torch.equal(u_b.view(torch.int32), u_0.view(torch.int32)), (case.name, "lse / u written")
    return buf[r, : case.V]


def _frac(got, ref, bound):
    return float(((got - ref).abs() / bound).max())


@pytest.mark.parametrize("name", [c.name for c in L.CASES])
def test_token_logprob_kernels_against_float64(dev, name):
    ops = _ops()
    case = L.CASE_BY_NAME[name]
    x_cpu, lab_cpu = L.inputs(name)
    ref_logp, ref_lse, ref_ent, ref_g = L.expected(name)
    x, labels = x_cpu.to(dev), lab_cpu.to(dev)
    valid = lab_cpu >= 0
    # ---- forward: without and with the entropy output
    logp0, lse0, _ = _forward(dev, case, x, labels, False)
    logp, lse, ent = _forward(dev, case, x, labels, True)
    assert torch.equal(logp0, logp) and torch.equal(lse0, lse), (name, "the entropy output changed logp / lse")
    # bit-equal to the loss head's pass 1
    buf = _buffer(dev, case, x)
    row_loss = torch.empty(case.rows, device=dev, dtype=torch.float32)
    ops.ce_fwd_bwd_(buf[1: case.rows + 1, : case.V], labels, row_loss, ops.count_valid(labels), write_grad=False)
    assert torch.equal(logp, -row_loss), (name, "logp is not -row_loss of afk_ce_fwd_bwd(write_grad=0) bit for bit",
                                          (logp != -row_loss).nonzero().flatten().tolist()[:8])
    g_logp, g_lse, g_ent = logp.cpu().double(), lse.cpu().double(), ent.cpu().double()
    for what, t in (("logp", g_logp), ("lse", g_lse), ("entropy", g_ent)):
        assert bool(torch.isfinite(t).all()), (name, what, "non-finite", (~torch.isfinite(t)).nonzero().flatten().tolist())
        assert bool((t[~valid] == 0).all()), (name, what, "ignored rows give 0")
    f_logp = _frac(g_logp, ref_logp, 2e-4 * ref_logp.abs() + 1e-5)
    f_lse = _frac(g_lse, ref_lse, 2e-4 * ref_lse.abs() + 1e-5)
    # the +-200 cases: the entropy of the row with the offset taken out again (exact in float64: the offset rows are multiples of 2^-6 or coarser)
    off = {"offset_up": 200.0, "offset_down": -200.0}.get(case.builder, 0.0)
    xd = x_cpu.double() - off
    ent_target = L.reference(xd, lab_cpu)[2] if off else ref_ent
    if off:
        assert float((ent_target - ref_ent).abs().max()) <= 1e-9
    f_ent = _frac(g_ent, ent_target, L.entropy_bound(xd, lab_cpu))
    # ---- backward: u random per row, one labelled row with u = 0, one ignored row with u = NaN
    u_cpu = L.upstream(name)
    got = _backward(dev, case, x, labels, lse, u_cpu.to(dev))
    got_d = got.cpu().double()
    want = L.dlogits(ref_g, u_cpu, lab_cpu)
    assert bool(torch.isfinite(got_d).all()), (name, "non-finite gradient")
    assert bool((got_d[~valid] == 0).all()), (name, "ignored rows are exactly zero whatever u holds")
    u_abs = torch.nan_to_num(u_cpu.double().abs(), nan=0.0)[:, None]
    e_grad = (got_d - want).abs() / (2.0 ** -7 * want.abs() + 1e-6 * u_abs).clamp_min(1e-300)
    e_grad = torch.where((got_d - want) == 0, torch.zeros_like(e_grad), e_grad)      # u = 0 rows: 0 against 0
    f_grad = float(e_grad.max())
    gr, gc = divmod(int(e_grad.argmax()), case.V)
    print(f"LOGPROB_MARGIN {name}: logp {f_logp:.3g} lse {f_lse:.3g} entropy {f_ent:.3g} gradient {f_grad:.3g} (fractions of the bounds)")
    msg = (f"{name}: logp {f_logp:.3g}, lse {f_lse:.3g}, entropy {f_ent:.3g} (row {int(((g_ent - ent_target).abs() / L.entropy_bound(xd, lab_cpu)).argmax())}), "
           f"gradient {f_grad:.3g} of their bounds (row {gr} col {gc} label {int(lab_cpu[gr])} u {float(u_cpu[gr]):.4g}: {float(got_d[gr, gc]):.6g} vs {float(want[gr, gc]):.6g})")
    assert f_logp <= 1.0 and f_lse <= 1.0 and f_ent <= 1.0 and f_grad <= 1.0, msg
    # ---- two runs are bit-equal
    logp2, lse2, ent2 = _forward(dev, case, x, labels, True)
    assert torch.equal(logp, logp2) and torch.equal(lse, lse2) and torch.equal(ent, ent2), (name, "forward not bit-deterministic")
    got2 = _backward(dev, case, x, labels, lse, u_cpu.to(dev))
    assert torch.equal(got.view(torch.int16), got2.view(torch.int16)), (name, "backward not bit-deterministic")


@pytest.mark.parametrize("rows,V,ld", L.SHAPES)
def test_token_logprob_kernels_all_rows_ignored(dev, rows, V, ld):
    case = L.R.Case("all-ignored", None, rows, V, ld)
    x = L.inputs(f"random3-{rows}x{V}" + (f"-ld{ld}" if ld != V else ""))[0].to(dev)
    labels = torch.full((rows,), L.IGNORE, device=dev, dtype=torch.int64)
    logp, lse, ent = _forward(dev, case, x, labels, True)
    assert not bool(logp.any()) and not bool(lse.any()) and not bool(ent.any())
    u = torch.full((rows,), float("nan"), device=dev)
    got = _backward(dev, case, x, labels, torch.full((rows,), float("nan"), device=dev), u)
    assert bool((got.view(torch.int16) == 0).all()), "ignored rows: +0 in every one of the V columns"


def test_token_logprob_refusals_name_the_entry(dev):
    ops, AfkError = _ops(), _afk_error()
    rows, V = 4, 5
    labels = torch.zeros(rows, device=dev, dtype=torch.int64)
    f = lambda: torch.zeros(rows, device=dev, dtype=torch.float32)
    odd = torch.zeros((rows, 12), device=dev, dtype=BF)[:, :V]             # ld % 8 != 0
    off = torch.zeros((rows, 16), device=dev, dtype=BF)[:, 1: 1 + V]       # rows start 2 bytes off a 16-byte boundary
    for bad in (odd, off):
        with pytest.raises(AfkError, match=r"afk_token_logprob: logits rows must be 16-byte aligned"):
            ops.token_logprob(bad, labels, f(), f(), f())
        with pytest.raises(AfkError, match=r"afk_token_logprob_bwd: logits rows must be 16-byte aligned"):
            ops.token_logprob_bwd_(bad, labels, f(), f())
    good = torch.zeros((rows, 8), device=dev, dtype=BF)[:, :V]
    with pytest.raises(AfkError, match="token_logprob logits: expected dtype"):
        ops.token_logprob(good.float(), labels, f(), f())
    with pytest.raises(AfkError, match="token_logprob shift_labels: expected dtype"):
        ops.token_logprob(good, labels.int(), f(), f())
    with pytest.raises(AfkError, match="token_logprob lse: a contiguous vector of 4"):
        ops.token_logprob(good, labels, f(), torch.zeros(rows + 1, device=dev))
    with pytest.raises(AfkError, match="token_logprob entropy: expected dtype"):
        ops.token_logprob(good, labels, f(), f(), f().double())
    with pytest.raises(AfkError, match="token_logprob_bwd_ u: a contiguous vector of 4"):
        ops.token_logprob_bwd_(good, labels, f(), torch.zeros(2 * rows, device=dev)[::2])
    with pytest.raises(AfkError, match="token_logprob_bwd_ logits: expected a HIP device tensor"):
        ops.token_logprob_bwd_(good.cpu(), labels, f(), f())


# ---------------------------------------------------------------------------------------------- the chunk loop of autograd_ops.lm_head_logprob
from tests.test_loss_head_gpu import CHUNK, H, M_ALL, M_LABELLED, V_CHUNKED   # noqa: E402  (the chunk_problem shapes of the loss route's test)


@pytest.fixture(scope="module")
def logprob_chunk_problem():
    """x [500, 128], w [4160, 128], 356 labelled rows (chunks of 128, 128 and 100 rows), a random upstream u per row.  Reference in float64 from the bf16
    x and w with the logits rounded to bf16 (as the kernel path rounds them): logp, and - the rounding passed straight through, as the kernel path differentiates
    it - dlogits = u (onehot - softmax), dX = dlogits . W, dW = dlogits^T . X"""
    g = torch.Generator().manual_seed(5)
    x = torch.randn(M_ALL, H, generator=g).to(BF)
    w = (torch.randn(V_CHUNKED, H, generator=g) * 0.15).to(BF)
    labels = torch.full((M_ALL,), L.IGNORE, dtype=torch.int64)
    rows = torch.randperm(M_ALL, generator=g)[:M_LABELLED].sort().values
    labels[rows] = torch.randint(0, V_CHUNKED, (M_LABELLED,), generator=g)
    u = torch.randn(M_ALL, generator=g)
    logits = (x.double() @ w.double().t()).to(BF)
    logp, _, ent, gl = L.reference(logits, labels)
    dlogits = L.dlogits(gl, u, labels)
    return dict(x=x, w=w, labels=labels, rows=rows, u=u, logp=logp, entropy=ent, dx=dlogits @ w.double(), dw=dlogits.t() @ x.double())


def _rel_l2(got, ref):
    return float((got.double().cpu() - ref).norm() / ref.norm())


@pytest.mark.parametrize("with_rows", [True, False], ids=["rows", "rows_none"])
def test_lm_head_logprob_chunk_loop(dev, monkeypatch, logprob_chunk_problem, with_rows):
    """autograd_ops.lm_head_logprob with three or four chunks, the last one ragged, against the float64 reference at the bars the loss route's chunk test uses
    (LOSS_ATOL per log-probability, GRAD_REL_L2 per gradient; that test records 1.7e-3 for dX and 2.4e-3 / 2.6e-3 for dW on the loss route)"""
    from audio_flamingo_amd import autograd_ops as A

    P = logprob_chunk_problem
    monkeypatch.setattr(A._LMHeadLogprob, "CHUNK", CHUNK)
    seen_f, seen_b = [], []
    real_f, real_b = A.ops.token_logprob, A.ops.token_logprob_bwd_
    monkeypatch.setattr(A.ops, "token_logprob", lambda lg, *a, **k: (seen_f.append(lg.shape[0]), real_f(lg, *a, **k))[1])
    monkeypatch.setattr(A.ops, "token_logprob_bwd_", lambda lg, *a, **k: (seen_b.append(lg.shape[0]), real_b(lg, *a, **k))[1])
    labels = P["labels"].to(dev)
    rows = P["rows"].to(dev) if with_rows else None
    sel = P["rows"] if with_rows else slice(None)
    x = P["x"].to(dev).requires_grad_(True)
    w = P["w"].to(dev).requires_grad_(True)
    logp, ent = A.lm_head_logprob(x, w, labels, rows, entropy=True)
    assert logp.dtype == torch.float32 and logp.shape == ((M_LABELLED,) if with_rows else (M_ALL,)) and logp.requires_grad and not ent.requires_grad
    (logp * P["u"][sel].to(dev)).sum().backward()
    torch.cuda.synchronize()
    want_chunks = [128, 128, 100] if with_rows else [128, 128, 128, 116]
    assert seen_f == want_chunks and seen_b == want_chunks, (seen_f, seen_b)
    e_lp = float((logp.detach().cpu().double() - P["logp"][sel]).abs().max())
    e_h = float((ent.cpu().double() - P["entropy"][sel]).abs().max())
    e_dx, e_dw = _rel_l2(x.grad, P["dx"]), _rel_l2(w.grad, P["dw"])
    msg = (f"max |logp - ref| {e_lp:.4g} (bar {LOSS_ATOL}), max |entropy - ref| {e_h:.4g}; rel-L2 dX {e_dx:.4g}, dW {e_dw:.4g} (bar {GRAD_REL_L2}; the loss route: "
           f"dX 1.7e-3, dW 2.4e-3 / 2.6e-3)")
    print("LOGPROB_CHUNK_MARGIN", "rows" if with_rows else "rows_none", msg)
    assert e_lp <= LOSS_ATOL and e_dx <= GRAD_REL_L2 and e_dw <= GRAD_REL_L2, msg
    unlabelled = (P["labels"] < 0).to(dev)
    assert bool((x.grad[unlabelled] == 0).all()), "unlabelled rows of dX are exactly zero"
    if not with_rows:
        assert bool((logp.detach()[unlabelled] == 0).all()) and bool((ent[unlabelled] == 0).all())


def test_lm_head_logprob_twice_on_one_weight_and_no_grad(dev, monkeypatch, logprob_chunk_problem):
    """two calls on one weight in one graph add their dW (and each x gets its own dX); under no_grad nothing is saved and backward raises torch's own error"""
    from audio_flamingo_amd import autograd_ops as A

    P = logprob_chunk_problem
    monkeypatch.setattr(A._LMHeadLogprob, "CHUNK", CHUNK)
    labels, rows, u = P["labels"].to(dev), P["rows"].to(dev), P["u"][P["rows"]].to(dev)

    def run(weights):
        x = P["x"].to(dev).requires_grad_(True)
        w = P["w"].to(dev).requires_grad_(True)
        total = sum(c * (A.lm_head_logprob(x, w, labels, rows) * u).sum() for c in weights)
        total.backward()
        torch.cuda.synchronize()
        return x.grad.float(), w.grad.float()

    dx1, dw1 = run([1.0])
    dx2, dw2 = run([1.0, -0.5])
    # dW = 1.0 dW1 - 0.5 dW1, each term rounded to bf16 before autograd adds them: two bf16 roundings of the terms and one of the sum
    for got, one, what in ((dw2, dw1, "dW"), (dx2, dx1, "dX")):
        err = (got - 0.5 * one).abs()
        assert bool((err <= 2.0 ** -7 * one.abs() + 1e-30).all()), (what, float((err / one.abs().clamp_min(1e-30)).max()))
    x = P["x"].to(dev).requires_grad_(True)
    w = P["w"].to(dev).requires_grad_(True)
    with torch.no_grad():
        lp = A.lm_head_logprob(x, w, labels, rows)
    assert not lp.requires_grad and lp.grad_fn is None
    assert torch.equal(lp, A.lm_head_logprob(x.detach(), w.detach(), labels, rows))
    with pytest.raises(RuntimeError, match="does not require grad"):
        lp.sum().backward()


# ---------------------------------------------------------------------------------------------- the model
def _smooth(dev):
    from audio_flamingo_amd.modeling import AudioFlamingo3ForConditionalGeneration as Mine
    from tests.test_model_gpu import _cfg

    m = Mine(_cfg(), device=dev)
    m.load_state_dict(torch.load(os.path.join(G, "tiny64_smooth_state_bf16.pt")))
    return m


def _batch(dev, case="D"):
    g = torch.load(os.path.join(G, f"tiny64_case{case}.pt"))
    kw = dict(input_ids=g["ids"].to(dev), input_features=g["feats"].to(dev), input_features_mask=g["fmask"].to(dev), labels=g["labels"].to(dev))
    if case == "E":
        kw["attention_mask"] = g["att"].to(dev)
    return g, kw


def _grads(m):
    m.arena.join_streams()
    torch.cuda.synchronize()
    return {k: p.grad.detach().float().cpu().clone() for k, p in m.named_parameters() if p.requires_grad and p.grad is not None}


def _rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-30))


def _scored(labels):
    """bool [B, S]: the positions out.token_logprobs fills (t >= 1 and labels[b, t] != -100)"""
    s = labels != -100
    s[:, 0] = False
    return s


BETA = 0.5   # the fp32 reference gives sum lp[row 0] - sum lp[row 1] = 1.78 on case D: sigmoid(0.5 * 1.78) = 0.71, far from saturation (asserted below)


@pytest.fixture(scope="module")
def reference_runs(dev):
    """case D on the smooth state, computed once: the reference (transformers' model) in fp32 on the CPU - logits, token log-probabilities, entropies, the
    pairwise loss L = -logsigmoid(BETA (sum lp[row 0] - sum lp[row 1])) and every parameter's gradient of it - and the reference's own bf16 run of the same
    loss on this device (the noise floor of tests/_tol.py for a statistic of one batch)"""
    from transformers import AudioFlamingo3ForConditionalGeneration

    from tests.test_model_gpu import _cfg
    from tools.parity_fulldepth import restore_rope_buffers

    g, _ = _batch("cpu")
    sd = torch.load(os.path.join(G, "tiny64_smooth_state_bf16.pt"))
    labels = g["labels"]

    def pair_loss(model, where, feats):
        out = model(input_ids=g["ids"].to(where), input_features=feats.to(where), input_features_mask=g["fmask"].to(where), attention_mask=g["att"].to(where))
        logits = out.logits.float()
        lp = torch.log_softmax(logits[:, :-1], -1).gather(-1, labels[:, 1:].clamp_min(0)[..., None].to(where)).squeeze(-1)
        lp = torch.where((labels[:, 1:] != -100).to(where), lp, torch.zeros_like(lp))
        delta = lp[0].sum() - lp[1].sum()
        loss = -torch.nn.functional.logsigmoid(BETA * delta)
        model.zero_grad()
        loss.backward()
        return logits.detach(), float(delta.detach()), float(loss.detach()), {k: p.grad.detach().float().cpu().clone() for k, p in model.named_parameters() if p.grad is not None}

    ref32 = AudioFlamingo3ForConditionalGeneration(_cfg())
    ref32.load_state_dict(sd)
    ref32 = ref32.float().train()
    logits, delta, loss, grads = pair_loss(ref32, "cpu", g["feats"].float())
    refb = AudioFlamingo3ForConditionalGeneration(_cfg())
    refb.load_state_dict(sd)
    refb = restore_rope_buffers(refb.to(dev).to(BF)).train()
    _, delta_b, loss_b, grads_b = pair_loss(refb, dev, g["feats"])
    return dict(logits=logits, token_logprobs=L.token_logprobs_reference(logits, labels), token_entropy=L.token_entropy_reference(logits, labels), delta=delta, loss=loss,
                grads=grads, bf16=dict(delta=delta_b, loss=loss_b, grads=grads_b))


def test_model_loss_route_equality(dev, monkeypatch):
    """(a) out.loss of the new route against the loss route within LOSS_ATOL, every parameter gradient of out.loss.backward() within GRAD_REL_L2 per tensor, and
    last_layer_rows_only on / off give the same token_logprobs at the scored positions: a log-probability is a logit minus a log-sum-exp of logits, so two runs
    whose logits agree to the logits bar agree to twice that bar (printed: whether they are bit-equal)"""
    from audio_flamingo_amd.modeling import AudioFlamingo3ForConditionalGeneration as Mine

    g, kw = _batch(dev)
    m = _smooth(dev)
    m.zero_grad()
    out0 = m(**kw)
    out0.loss.backward()
    g0 = _grads(m)
    m.zero_grad()
    out1 = m(**kw, return_token_logprobs=True)
    assert out0.token_logprobs is None and out0.token_entropy is None and out1.token_entropy is None
    assert "token_logprobs" in out1.keys() and "token_logprobs" not in out0.keys()
    lp = out1.token_logprobs
    assert lp.shape == g["labels"].shape and lp.dtype == torch.float32 and lp.requires_grad
    out1.loss.backward()
    g1 = _grads(m)
    scored = _scored(g["labels"])
    assert bool((lp.detach().cpu()[~scored] == 0).all()) and bool((lp.detach().cpu()[scored] < 0).all())
    assert abs(float(out1.loss.detach()) - float(-lp.detach().sum() / scored.sum())) <= 1e-5
    rel = {k: _rel(g1[k], v) for k, v in g0.items()}
    worst = max(rel, key=rel.get)
    print(f"LOGPROB_MODEL loss {float(out1.loss):.6f} vs the loss route {float(out0.loss):.6f}; {len(rel)} gradient tensors, worst rel-L2 {rel[worst]:.4g} ({worst})")
    assert set(g1) == set(g0) and len(g0) >= 60
    assert abs(float(out1.loss) - float(out0.loss)) <= LOSS_ATOL
    assert rel[worst] <= GRAD_REL_L2, (worst, rel[worst])
    # the lazy logits and return_logits=True behave as beside `loss`
    assert not out1.logits_materialized and out1.logits.shape == (*g["labels"].shape, m.V)
    out2 = m(**kw, return_token_logprobs=True, return_logits=True)
    assert out2.logits_materialized and _rel(out1.logits.float().cpu(), out2.logits.float().cpu()) < 1e-2   # the bar of test_last_decoder_layer_on_labelled_rows_matches_all_rows
    via_logits = L.token_logprobs_reference(out2.logits.detach().cpu(), g["labels"])
    tol = 2 * logit_tol(float(out2.logits.detach().abs().max()))
    assert float((out2.token_logprobs.detach().cpu().double() - via_logits).abs().max()) <= tol
    res = {}
    for rows_only in (True, False):
        monkeypatch.setattr(Mine, "last_layer_rows_only", rows_only)
        res[rows_only] = m(**kw, return_token_logprobs=True).token_logprobs.detach().cpu()
    d = float((res[True] - res[False])[scored].abs().max())
    print(f"LOGPROB_MODEL last_layer_rows_only on / off: max |d token_logprobs| {d:.3g} (bit-equal: {torch.equal(res[True], res[False])}), bar {tol:.3g}")
    assert d <= tol and torch.equal(res[True], lp.detach().cpu())


def test_model_pairwise_loss_against_reference(dev, reference_runs):
    """(b) a loss mean CE cannot express: L = -logsigmoid(BETA (sum lp[row 0] - sum lp[row 1])) on out.token_logprobs, every parameter's gradient against the
    reference's fp32 CPU run, per tensor rel-L2 <= max(GRAD_REL_L2, FLOOR_FACTOR x the reference's own bf16 run of the same loss on this device)"""
    R = reference_runs
    s = float(torch.sigmoid(torch.tensor(BETA * R["delta"])))
    assert 0.1 < s < 0.9, ("BETA saturates the sigmoid", s)
    g, kw = _batch(dev)
    m = _smooth(dev)
    m.zero_grad()
    out = m(**kw, return_token_logprobs=True)
    lp = out.token_logprobs
    delta = lp[0].sum() - lp[1].sum()
    loss = -torch.nn.functional.logsigmoid(BETA * delta)
    loss.backward()
    got = _grads(m)
    scored = _scored(g["labels"])
    e_lp = float((lp.detach().cpu().double() - R["token_logprobs"])[scored].abs().max())
    tol = 2 * logit_tol(float(R["logits"].abs().max()))
    print(f"LOGPROB_PAIR delta {float(delta):.5f} (reference fp32 {R['delta']:.5f}, its bf16 run {R['bf16']['delta']:.5f}); loss {float(loss):.6f} vs {R['loss']:.6f} "
          f"({R['bf16']['loss']:.6f}); max |token_logprobs - ref| {e_lp:.4g} (bar {tol:.3g})")
    assert e_lp <= tol
    # (the loss itself is reported: |dL / d delta| <= BETA, so it is as good as the log-probabilities above and the gradients below)
    assert len(got) >= 60 and set(got) <= set(R["grads"]), "every trainable tensor of ours has a reference gradient"
    bad = {}
    for k in sorted(got):
        ref = R["grads"][k]
        ours, floor = _rel(got[k], ref), _rel(R["bf16"]["grads"][k], ref)
        bar = max(GRAD_REL_L2, FLOOR_FACTOR * floor)
        print(f"LOGPROB_PAIR_GRAD {k}: ours {ours:.4g}, reference bf16 {floor:.4g}, bar {bar:.4g}")
        if ours > bar:
            bad[k] = (ours, floor, bar)
    assert not bad, bad


def test_model_token_entropy(dev, reference_runs):
    """(c) out.token_entropy against the reference's fp32 logits.  If every logit of a row is within tau of the reference's (tau = logit_tol(|ref|max), the bar
    the logits themselves are held to) then, with I_c = -log p_c the surprisal and dH / dx_c = -p_c (log p_c + H) = p_c (I_c - H), the mean value theorem gives
    |dH| <= tau sup sum_c p_c |I_c - H| <= tau sup 2 H over the segment between the two rows, where H <= H_ref + |dH|: |dH| <= 2 tau H_ref / (1 - 2 tau).  (The
    shorter tau (1 + H_ref) is printed beside it; nothing derives it.)  Detached, zero off the scored positions."""
    R = reference_runs
    g, kw = _batch(dev)
    m = _smooth(dev)
    out = m(**kw, return_token_logprobs=True, return_token_entropy=True)
    h = out.token_entropy
    assert h.shape == g["labels"].shape and h.dtype == torch.float32 and not h.requires_grad and h.grad_fn is None
    assert out.token_logprobs.requires_grad and "token_entropy" in out.keys()
    scored = _scored(g["labels"])
    hc = h.cpu().double()
    assert bool((hc[~scored] == 0).all()) and bool((hc[scored] > 0).all())
    tau = logit_tol(float(R["logits"].abs().max()))
    ref = R["token_entropy"]
    err = (hc - ref).abs()[scored]
    bound = (2 * tau * ref / (1 - 2 * tau))[scored]
    short = (tau * (1 + ref))[scored]
    print(f"LOGPROB_ENTROPY max |dH| {float(err.max()):.4g}; worst fraction of 2 tau H / (1 - 2 tau) {float((err / bound).max()):.3g}, of tau (1 + H) {float((err / short).max()):.3g}; "
          f"tau {tau:.4g}, H_ref in [{float(ref[scored].min()):.3f}, {float(ref[scored].max()):.3f}]")
    assert bool((err <= bound).all())
    # the same log-probabilities with and without the entropy output, and a backward through them
    m.zero_grad()
    out.loss.backward()
    plain = m(**kw, return_token_logprobs=True)
    assert torch.equal(plain.token_logprobs.detach(), out.token_logprobs.detach())


@pytest.mark.parametrize("order", ["loss_first", "logprob_first"])
def test_model_both_stages_in_one_step(dev, order):
    """(d) the loss route on one batch and the new route on another, one backward over the sum: the lm_head gradient equals the sum of the two single runs
    within GRAD_REL_L2 (the loss route parks its unscaled dW in the arena slice; the new route's announced write moves it out first), every other gradient too"""
    from tests.test_model_gpu import _fresh_model

    _, kw_a = _batch(dev, "D")
    _, kw_b = _batch(dev, "E")
    m = _fresh_model(dev)
    single = {}
    for name, kw, extra in (("a", kw_a, {}), ("b", kw_b, dict(return_token_logprobs=True))):
        m.zero_grad()
        m(**kw, **extra).loss.backward()
        single[name] = _grads(m)
    m.zero_grad()
    if order == "loss_first":
        la = m(**kw_a).loss
        lb = m(**kw_b, return_token_logprobs=True).loss
    else:
        lb = m(**kw_b, return_token_logprobs=True).loss
        la = m(**kw_a).loss
    (la + lb).backward()
    both = _grads(m)
    assert not m.arena.parked, "a parked lm_head gradient survived the step"
    rel = {k: _rel(both[k], single["a"][k] + single["b"][k]) for k in both}
    worst = max(rel, key=rel.get)
    print(f"LOGPROB_BOTH {order}: lm_head.weight rel-L2 {rel['lm_head.weight']:.4g}; worst {rel[worst]:.4g} ({worst})")
    assert rel["lm_head.weight"] <= GRAD_REL_L2 and rel[worst] <= GRAD_REL_L2, (worst, rel[worst])


def test_model_stale_lse_raises(dev):
    """(e) an optimizer step between the forward and its backward: the saved log-sum-exp belongs to weights that no longer exist"""
    from audio_flamingo_amd.arena import FusedAdamW
    from tests.test_model_gpu import _fresh_model

    _, kw = _batch(dev)
    m = _fresh_model(dev)
    opt = FusedAdamW(m.arena, lr=1e-3)
    m.zero_grad()
    m(**kw, return_token_logprobs=True).loss.backward()      # a gradient for the step
    m.arena.join_streams()
    out = m(**kw, return_token_logprobs=True)
    opt.step()
    with pytest.raises(_afk_error(), match="parameters changed between this stage's forward and its backward"):
        out.loss.backward()


def test_model_refusals(dev, monkeypatch):
    """(f)"""
    from audio_flamingo_amd import exact
    from audio_flamingo_amd.arena import FusedAdamW
    from audio_flamingo_amd.dp import BackwardOverlap
    from audio_flamingo_amd.graphs import GraphedTrainStep
    from tests.test_model_gpu import _fresh_model

    AfkError = _afk_error()
    _, kw = _batch(dev)
    m = _fresh_model(dev)
    no_labels = {k: v for k, v in kw.items() if k != "labels"}
    with pytest.raises(ValueError, match="return_token_logprobs=True needs labels"):
        m(**no_labels, return_token_logprobs=True)
    with pytest.raises(ValueError, match="return_token_entropy=True needs return_token_logprobs=True"):
        m(**kw, return_token_entropy=True)
    with pytest.raises(AfkError, match=r"return_token_logprobs=True, use_cache=True / past_key_values"):
        m(**kw, return_token_logprobs=True, use_cache=True)
    with pytest.raises(AfkError, match=r"return_token_logprobs=True, use_cache=True / past_key_values"):
        m(input_ids=kw["input_ids"][:, -1:], labels=kw["labels"][:, -1:], past_key_values=object(), return_token_logprobs=True)   # refused before the cache is looked at
    monkeypatch.setattr(exact, "ENABLED", True)
    with pytest.raises(AfkError, match="return_token_logprobs=True. under AFK_EXACT_FP32=1"):
        m(**kw, return_token_logprobs=True)
    monkeypatch.setattr(exact, "ENABLED", False)
    m.check_placeholders = False
    opt = FusedAdamW(m.arena, lr=1e-3)
    ov = BackwardOverlap(m.arena, opt)

    def body():
        m.zero_grad()
        ov.begin_step()
        loss = m(**kw, return_token_logprobs=True).loss
        loss.backward()
        ov.finish()
        return loss

    with pytest.raises(AfkError, match="inside GraphedTrainStep"):
        GraphedTrainStep(m, opt, ov, body, warmup=1)
    assert m._graphed_step is False
    assert float(m(**kw, return_token_logprobs=True).loss) > 0      # and the eager route still runs


def test_model_dispatch_counts(dev):
    """(g) a step through the new route dispatches lm_head_logprob and lm_head_logprob_bwd once each and lm_head_loss not at all; a step without the flag
    dispatches exactly the stages it did before (counted as tests/test_custom_ops_gpu.py counts them)"""
    from audio_flamingo_amd import stage_ops
    from tests.test_model_gpu import _fresh_model

    _, kw = _batch(dev)
    m = _fresh_model(dev)

    def counted(**extra):
        counts, orig = {}, {}
        for name, st in stage_ops._STAGES.items():
            orig[name] = (st.op, st.op_bwd)

            def wrap(op, nm):
                def call(*a):
                    counts[nm] = counts.get(nm, 0) + 1
                    return op(*a)
                return call
            st.op, st.op_bwd = wrap(st.op, name), wrap(st.op_bwd, name + "_bwd")
        try:
            m.zero_grad()
            m(**kw, **extra).loss.backward()
            torch.cuda.synchronize()
        finally:
            for name, st in stage_ops._STAGES.items():
                st.op, st.op_bwd = orig[name]
        return counts

    base = {"conv_stem": 1, "encoder_layer": m.enc_layers, "pool_norm": 1, "projector": 1, "embed_scatter": 1, "decoder_layer": m.dec_layers, "final_rms_norm": 1}
    full = lambda d: {**d, **{k + "_bwd": v for k, v in d.items()}}
    assert counted() == full({**base, "lm_head_loss": 1})
    assert counted(return_token_logprobs=True) == full({**base, "lm_head_logprob": 1})
    assert counted(return_token_logprobs=True, return_token_entropy=True) == full({**base, "lm_head_logprob": 1})
    assert "lm_head_logprob" in stage_ops.registered_stages()
    assert "Tensor(a!) grads" in str(torch.ops.afk.lm_head_logprob_bwd.default._schema)


def test_step_with_the_new_stage_traces_under_torch_compile(dev):
    """final RMSNorm -> lm_head_logprob -> a loss that mean CE cannot express, as ONE graph under torch.compile(fullgraph=True) (aot_eager: the stage stays an
    opaque operator node with its schema and fake implementation): the eager log-probabilities and gradients bit for bit"""
    from audio_flamingo_amd import functional as F_
    from tests.test_model_gpu import _fresh_model

    m = _fresh_model(dev)
    a, lm = m.arena, m._lm
    M = 96
    g = torch.Generator().manual_seed(9)
    x0 = torch.randn(M, m.H, generator=g).to(BF).to(dev)
    shift = torch.randint(0, m.V, (M,), generator=g)
    shift[::5] = -100
    shift = shift.to(dev)
    rows = (shift >= 0).nonzero().reshape(-1)
    anchors = (m._anchor(lm + "norm.weight"), m._anchor("lm_head.weight"))

    def chain(x, shift_, rows_):
        h = F_.RMSNormFn.apply(x, anchors[0], a, lm + "norm.weight", m.rms_eps)
        out = F_.LMHeadLogprobFn.apply(h, anchors[1], a, "lm_head.weight", shift_, True, rows_)
        lp = out[0]
        half = lp.shape[0] // 2
        return -torch.nn.functional.logsigmoid(0.1 * (lp[:half].sum() - lp[half:].sum())), lp, out[1]

    def run(fn):
        m.zero_grad()
        x = x0.clone().requires_grad_(True)
        loss, lp, ent = fn(x, shift, rows)
        loss.backward()
        a.join_streams()
        torch.cuda.synchronize()
        return float(loss.detach()), lp.detach().clone(), ent.detach().clone(), x.grad.clone(), a.grads.clone()

    eager = run(chain)      # also records the stage geometries the fake implementations answer from
    # the models of the tests before this one are cyclic garbage by now; a collection in the middle of the trace would purge their stage keys
    # (stage_ops._purge) from the very tables dynamo is writing guards for
    import gc

    gc.collect()
    torch._dynamo.reset()
    traced = run(torch.compile(chain, fullgraph=True, backend="aot_eager"))
    assert traced[0] == eager[0]
    for what, t, e in zip(("logp", "entropy", "dX", "gradient arena"), traced[1:], eager[1:]):
        assert torch.equal(t, e), f"traced step: {what} differs from the eager step"
    assert bool(eager[4].any()) and bool((eager[3][shift < 0] == 0).all())

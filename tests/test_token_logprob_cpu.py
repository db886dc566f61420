"""The float64 restatement of the per-token log-probability kernels (tests/_logprob_ref.py) against torch's own float64 functions, and the
[B, S] alignment rule of forward(labels=, return_token_logprobs=True) against a five-line torch reference.  No GPU."""
import pytest
import torch

from tests import _logprob_ref as L

TOL = 1e-9   # float64 against float64: two orders of summation


def _close(a, b, what):
    assert bool(torch.isfinite(a).all()), (what, "non-finite")
    err = (a - b).abs() / (1.0 + b.abs())
    assert float(err.max()) <= TOL, (what, float(err.max()), int(err.argmax()))


def _against_torch(name, x, lab):
    logp, lse, ent, g = L.reference(x, lab)
    xd = x.double()
    valid = lab >= 0
    zero = torch.zeros(x.shape[0], dtype=torch.float64)
    lsm = torch.log_softmax(xd, -1)
    _close(logp, torch.where(valid, lsm.gather(1, lab.clamp_min(0)[:, None]).squeeze(1), zero), (name, "logp"))
    _close(lse, torch.where(valid, torch.logsumexp(xd, -1), zero), (name, "lse"))
    _close(ent, torch.where(valid, torch.distributions.Categorical(logits=xd, validate_args=False).entropy(), zero), (name, "entropy"))
    # the gradient of sum(u * logp) by autograd
    gen = torch.Generator().manual_seed(3)
    u = torch.randn(x.shape[0], generator=gen, dtype=torch.float64)
    xa = xd.clone().requires_grad_(True)
    picked = torch.log_softmax(xa, -1).gather(1, lab.clamp_min(0)[:, None]).squeeze(1)
    (torch.where(valid, picked, zero) * u).sum().backward()
    want = torch.nan_to_num(xa.grad, nan=0.0)   # autograd forms 0 * -inf on masked columns; the gradient there is 0
    got = L.dlogits(g, u, lab)
    assert float((got - want).abs().max()) <= TOL, (name, "dlogits", float((got - want).abs().max()))
    assert bool((got[~valid] == 0).all())


@pytest.mark.parametrize("name", [c.name for c in L.CASES])
def test_restatement_against_torch_float64(name):
    x, lab = L.inputs(name)
    _against_torch(name, x, lab)
    logp, lse, ent, g = L.expected(name)
    row_loss, _ = L.R.expected(name)
    assert torch.equal(logp, -row_loss)
    assert bool((ent >= -1e-12).all()) and bool((ent <= torch.log(torch.tensor(float(x.shape[1]))) + 1e-9).all())
    ign = lab < 0
    assert bool(ign.any()) and bool((logp[ign] == 0).all()) and bool((lse[ign] == 0).all()) and bool((ent[ign] == 0).all())
    u = L.upstream(name)
    assert int(torch.isnan(u).sum()) == 1 and bool(ign[torch.isnan(u)].all()) and int((u == 0).sum()) >= 1
    d = L.dlogits(g, u, lab)
    assert bool(torch.isfinite(d).all()) and bool((d[ign] == 0).all()) and bool((d[u == 0] == 0).all())
    assert bool((L.entropy_bound(x, lab) > 0).all())


@pytest.mark.parametrize("rows,V,ld", L.SHAPES)
def test_restatement_all_rows_ignored(rows, V, ld):
    x = L.inputs(f"random3-{rows}x{V}" + (f"-ld{ld}" if ld != V else ""))[0]
    lab = torch.full((rows,), L.IGNORE, dtype=torch.int64)
    _against_torch("all-ignored", x, lab)
    logp, lse, ent, g = L.reference(x, lab)
    assert not bool(logp.any()) and not bool(lse.any()) and not bool(ent.any()) and not bool(g.any())


def test_offsets_do_not_move_the_entropy():
    """the +-200 cases are the random3 rows of their own seed plus a constant: in exact arithmetic the entropy ignores it; at bf16 the offset rows are
    other rows (spacing 1 at 200), so the statement is made on the float64 reference of ONE row set"""
    x, lab = L.inputs("random3-24x2053-ld2064")
    base = L.reference(x.double(), lab)[2]
    for off in (200.0, -200.0):
        moved = L.reference(x.double() + off, lab)[2]
        assert float((moved - base).abs().max()) <= 1e-10


def test_alignment_rule():
    """out.token_logprobs[b, t] = log softmax(logits[b, t - 1])[labels[b, t]] where t >= 1 and labels[b, t] != -100, 0 elsewhere: -100 runs at the
    start, in the middle and at the end of a row, a label at t = 0 (never scored: nothing precedes it) and a fully ignored row"""
    B, S, V = 4, 9, 13
    gen = torch.Generator().manual_seed(11)
    logits = torch.randn(B, S, V, generator=gen, dtype=torch.float64)
    labels = torch.randint(0, V, (B, S), generator=gen)
    labels[0, :3] = -100          # a run at the start
    labels[1, 4:6] = -100         # in the middle; labels[1, 0] is a real label at t = 0
    labels[2, 6:] = -100          # at the end
    labels[3, :] = -100           # nothing to score
    assert int(labels[1, 0]) >= 0
    # the rule, written out position by position
    want = torch.zeros(B, S, dtype=torch.float64)
    want_h = torch.zeros(B, S, dtype=torch.float64)
    for b in range(B):
        for t in range(1, S):
            if int(labels[b, t]) != -100:
                lsm = torch.log_softmax(logits[b, t - 1], -1)
                want[b, t] = lsm[labels[b, t]]
                want_h[b, t] = -(lsm.exp() * lsm).sum()
    got = L.token_logprobs_reference(logits, labels)
    assert float((got - want).abs().max()) <= 1e-12
    assert float((L.token_entropy_reference(logits, labels) - want_h).abs().max()) <= 1e-12
    assert bool((got[:, 0] == 0).all()) and bool((got[labels == -100] == 0).all()) and not bool(got[3].any())
    # what the model does: per-row values at the positions of the SHIFTED labels, moved one step to the right
    shift = torch.nn.functional.pad(labels, (0, 1), value=-100)[:, 1:].reshape(-1)
    flat_lsm = torch.log_softmax(logits.reshape(B * S, V), -1)
    per_row = torch.where(shift >= 0, flat_lsm.gather(1, shift.clamp_min(0)[:, None]).squeeze(1), torch.zeros(B * S, dtype=torch.float64))
    assert float((L.align(per_row, B, S) - want).abs().max()) <= 1e-12
    # ... and when only the labelled rows were computed and scattered back
    rows = (shift != -100).nonzero().reshape(-1)
    scattered = torch.zeros(B * S, dtype=torch.float64).index_copy(0, rows, per_row[rows])
    assert torch.equal(L.align(scattered, B, S), L.align(per_row, B, S))
    # mean CE from the same tensor
    ce = torch.nn.functional.cross_entropy(logits[:, :-1].reshape(-1, V), labels[:, 1:].reshape(-1), ignore_index=-100)
    assert abs(float(-(got.sum() / max(int((shift != -100).sum()), 1))) - float(ce)) <= 1e-12

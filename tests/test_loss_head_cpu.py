"""The float64 reference of the loss-head tests (tests/_ce_ref.py) against torch.nn.functional.cross_entropy, and the conditions under which
each input builder reaches the kernel path it is named after - so a builder can never silently stop reaching it.  No GPU."""
import pytest
import torch

from tests import _ce_ref as R

NAMES = [c.name for c in R.CASES]


@pytest.mark.parametrize("name", NAMES)
def test_reference_matches_torch_cross_entropy(name):
    x, lab = R.inputs(name)
    n_valid = int((lab >= 0).sum())
    for upstream, denom in ((1.0, n_valid), (0.25, 37.0), (1.0, 0.0)):
        row_loss, g, loss = R.reference(x, lab, denom, upstream)
        xr = x.double().requires_grad_(True)
        total = torch.nn.functional.cross_entropy(xr, lab, ignore_index=-100, reduction="sum")
        (upstream * total / max(denom, 1.0)).backward()
        per_row = torch.nn.functional.cross_entropy(xr.detach(), lab, ignore_index=-100, reduction="none")
        assert torch.isfinite(total) and bool(torch.isfinite(xr.grad).all()), "the reference's own result must be finite on every builder"
        torch.testing.assert_close(loss, total.detach() / max(denom, 1.0), rtol=1e-12, atol=1e-13)
        torch.testing.assert_close(row_loss, per_row, rtol=1e-12, atol=1e-13)
        torch.testing.assert_close(g, xr.grad, rtol=1e-12, atol=1e-15 * upstream / max(denom, 1.0))
        assert bool((g[lab < 0] == 0).all()) and bool((row_loss[lab < 0] == 0).all())


def test_shapes_reach_every_path():
    """the vector / tail geometry the shapes were chosen for"""
    per_thread = {V: R.vectors_per_thread(V) for (_, V, _) in R.SHAPES}
    assert per_thread[5] == (0, 0) and list(R.tail_columns(5)) == [0, 1, 2, 3, 4]        # no vector at all: the tail alone
    assert per_thread[8] == (0, 1) and not R.tail_columns(8)
    assert per_thread[2048] == (1, 1)                                                     # exactly one vector per thread
    assert per_thread[2053] == (1, 1) and len(R.tail_columns(2053)) == 5
    assert per_thread[6285] == (3, 4) and len(R.tail_columns(6285)) == 5                  # the online update runs 2-3 times, plus a tail
    assert per_thread[152064] == (74, 75) and not R.tail_columns(152064)                 # the real vocabulary
    for rows, V, ld in R.SHAPES:
        assert 8 <= rows <= 70 and ld % 8 == 0 and ld >= V
        if V % 8:
            assert ld >= (V + 7) // 8 * 8 + 8, "room for a store that runs past V to land on sentinels"
    assert any(V % 8 == 0 and ld == V + 64 for (_, V, ld) in R.SHAPES)


@pytest.mark.parametrize("name", NAMES)
def test_labels_are_placed_where_they_should_be(name):
    c = R.CASE_BY_NAME[name]
    x, lab = R.inputs(name)
    V = c.V
    assert lab.shape == (c.rows,) and x.shape == (c.rows, V) and x.dtype == torch.bfloat16
    valid = lab[lab >= 0]
    assert bool(((valid >= 0) & (valid < V)).all()), "in-range labels only"
    assert 0 < int((lab < 0).sum()) < c.rows, "a mix of ignored and labelled rows"
    have = set(valid.tolist())
    if c.builder != "masked":
        want = set(R.deliberate_labels(V))
        assert len(want) + 1 < c.rows, "the deliberate positions and the ignored row fit before the row a builder may overwrite"
        if c.builder == "spike":
            assert int(lab[-1]) == R.spike_column(V)
        assert want <= have, (sorted(want - have), "deliberate label positions missing")
        assert {0, V - 1} <= want
        tail = list(R.tail_columns(V))
        if tail:
            assert {tail[0], tail[-1]} <= have, "first and last tail element carry a label"
        if R.n_vectors(V):
            assert any(c_ % 8 == 7 and c_ < R.n_vectors(V) * 8 for c_ in have), "last lane of a vector"
        if R.n_vectors(V) >= R.THREADS:
            assert any(R.owner_thread(c_, V) == R.THREADS - 1 and c_ < R.n_vectors(V) * 8 for c_ in have), "a column of thread 255"


@pytest.mark.parametrize("name", [n for n in NAMES if n.startswith("masked")])
def test_masked_rows_keep_a_finite_label_logit(name):
    c = R.CASE_BY_NAME[name]
    x, lab = R.inputs(name)
    xf = x.float()
    mask = R.masked_columns(c.V)
    assert bool(mask[:64].all())
    assert bool(torch.isinf(xf[:, mask]).all()) and not bool(torch.isposinf(xf).any()) and not bool(torch.isnan(xf).any())
    rows = (lab >= 0).nonzero().flatten()
    assert bool(torch.isfinite(xf[rows, lab[rows]]).all()), "every masked-row label has a finite logit"
    lo, hi = R.vectors_per_thread(c.V)
    if hi >= 2:
        # threads 0..7 meet an all -inf vector while their running max is still -inf, and finite vectors after it
        assert bool(torch.isfinite(xf[:-1, 8 * R.THREADS: 8 * R.THREADS + 64]).all())
    if lo >= 3:
        v = R.THREADS + 100
        assert bool(mask[8 * v: 8 * v + 8].all()) and not bool(mask[8 * (v - R.THREADS): 8 * (v - R.THREADS) + 8].any()) \
            and not bool(mask[8 * (v + R.THREADS): 8 * (v + R.THREADS) + 8].any()), "a whole -inf vector between two finite ones of thread 100"
        # the last row's label sits behind two all -inf vectors of its own thread
        only = int(lab[-1])
        t = R.owner_thread(only, c.V)
        assert only // 8 >= 2 * R.THREADS and bool(torch.isinf(xf[-1, 8 * t: 8 * t + 8]).all())
    assert int(torch.isfinite(xf[-1]).sum()) == 1 and bool(torch.isfinite(xf[-1, lab[-1]]))
    if c.V % 8:
        assert bool(mask[R.n_vectors(c.V) * 8]), "a -inf tail element"


def test_ramps_move_the_running_max_on_every_vector_or_never():
    for name in NAMES:
        c = R.CASE_BY_NAME[name]
        if c.builder not in ("ramp_up", "ramp_down") or R.vectors_per_thread(c.V)[0] < 2:
            continue
        x = R.inputs(name)[0][0].float()
        assert 79.0 <= float(x.max() - x.min()) <= 81.0
        nv = R.n_vectors(c.V)
        vmax = x[: nv * 8].reshape(nv, 8).max(1).values
        for t in (0, 100, 255):
            seq = vmax[t::R.THREADS]
            assert len(seq) >= 2
            if c.builder == "ramp_up":
                assert bool((seq[1:] > seq[:-1]).all()), "ascending: the running max changes on every vector of a thread"
            else:
                assert bool((seq[1:] < seq[:-1]).all()), "descending: the running max never changes after a thread's first vector"


def test_spike_is_late_and_offsets_are_large():
    for name in NAMES:
        c = R.CASE_BY_NAME[name]
        x = R.inputs(name)[0].float()
        if c.builder == "spike":
            col = R.spike_column(c.V)
            assert col >= c.V // 2 and bool((x[:, col] == 60).all()) and int((x == -60).sum()) == c.rows * (c.V - 1)
        if c.builder == "offset_up":
            assert float(x.min()) > 170 and float(x.max()) < 230
        if c.builder == "offset_down":
            assert float(x.max()) < -170 and float(x.min()) > -230

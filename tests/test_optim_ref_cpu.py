"""The premises of tests/test_optim_edges_gpu.py, checked where no GPU is needed (tests/_optim_ref.py holds the references and the derivation of the
bar): the fp32 restatement of adamw_elem stays well inside the derived per-element bar, every single-mistake mutation of it leaves the bar by a
wide margin, the one-hot probes of the sum of squares name every edge of the launch, and ops.adamw_step / ops.adamw_step_t refuse wrongly typed
or short buffers before the C call."""
import json

import pytest
import torch

from tests import _optim_ref as R

N = 1 << 18
# the lengths tests/test_optim_edges_gpu.py runs afk_sumsq_bf16 at
SUMSQ_NS = [1, 7, 8, 9, 2047, 2048, 2049, 8 * 256 * 1024 - 8, 8 * 256 * 1024, 8 * 256 * 1024 + 8, 2 * 8 * 256 * 1024 + 13]


def _walk(hp, n=N):
    """(step, state before, gradient) for STEPS, each continued from the restated state of the step before"""
    w, m, v = R.make_state(n)
    for step in R.STEPS:
        g = R.make_grad(n, step)
        yield step, (w, m, v), g
        w, m, v, _ = R.restated_fp32(w, m, v, g, step=step, **hp)


@pytest.fixture(scope="module")
def walk0():
    """the walk of the first hyper-parameter set, shared by the mutation tests"""
    return list(_walk(R.HYPER_SETS[0]))


@pytest.mark.parametrize("hp", R.HYPER_SETS, ids=lambda hp: f"b1={hp['beta1']}-b2={hp['beta2']}-lr={hp['lr']}-wd={hp['weight_decay']}")
def test_restatement_stays_inside_the_bar(hp):
    """2^18 elements, steps 1, 2, 3, 4 and 1000: worst |x - X| / tolerance of the restatement <= 0.75 for master, m and v (a bar the correct
    formula only just meets would be a fitted one); the bf16 parameter is the rounded master; zero gradient on zero moments stays exactly zero"""
    worst = {"w": 0.0, "m": 0.0, "v": 0.0}
    for step, (w, m, v), g in _walk(hp):
        ref = R.ref64(w, m, v, g, step=step, **hp)
        w1, m1, v1, p1 = R.restated_fp32(w, m, v, g, step=step, **hp)
        for name, x in (("w", w1), ("m", m1), ("v", v1)):
            worst[name] = max(worst[name], R.worst_ratio(x, *ref[name]))
        assert torch.equal(p1, w1.to(torch.bfloat16))
        still = (g.float() == 0) & (m == 0) & (v == 0)
        if step <= 2:
            assert int(still.sum()) >= N // 7
        assert not bool(m1[still].any()) and not bool(v1[still].any())
    print("optim_ref restatement", json.dumps({"hyper": hp, "n": N, "steps": R.STEPS, "worst_error_over_tolerance": worst}))
    assert all(r <= 0.75 for r in worst.values()), worst


def test_restatement_with_multiplier_and_hyper_stays_inside_the_bar(walk0):
    """the same bar with grad_scale = 0.37, and with device hyper-parameters that override lr and the bias corrections and carry a multiplier
    (grad_scale = 0.5 at the same time)"""
    hp = R.HYPER_SETS[0]
    hyper = torch.tensor([3e-3, 0.5, 0.25, 0.37], dtype=torch.float32)
    worst = {}
    for label, kw in (("grad_scale", dict(grad_scale=0.37)), ("hyper", dict(grad_scale=0.5, hyper=hyper))):
        worst[label] = {"w": 0.0, "m": 0.0, "v": 0.0}
        for step, (w, m, v), g in walk0:
            ref = R.ref64(w, m, v, g, step=step, **hp, **kw)
            got = R.restated_fp32(w, m, v, g, step=step, **hp, **kw)
            for name, x in zip("wmv", got):
                worst[label][name] = max(worst[label][name], R.worst_ratio(x, *ref[name]))
    print("optim_ref restatement multiplier", json.dumps(worst))
    assert all(r <= 0.75 for d in worst.values() for r in d.values()), worst


@pytest.mark.parametrize("mutation", R.MUTATIONS)
def test_every_mutation_leaves_the_bar(walk0, mutation):
    """hyper-parameters (0.9, 0.999, lr 1e-2, wd 0.1): one mistake in the formula puts the worst master element >= 3x over the bar on EVERY step and
    >= 25 % of the elements over it on at least one step.  The dropped-multiplier mutations run with a multiplier of 0.37 (as grad_scale, and as
    hyper[3] beside the scalar lr and bias corrections of the step)."""
    hp = R.HYPER_SETS[0]
    per_step, share = {}, {}
    for step, (w, m, v), g in walk0:
        kw = {}
        if mutation == "multiplier_dropped":
            kw = dict(grad_scale=0.37)
        elif mutation == "hyper3_ignored":
            kw = dict(hyper=torch.tensor([hp["lr"], 1.0 - hp["beta1"] ** step, (1.0 - hp["beta2"] ** step) ** 0.5, 0.37], dtype=torch.float32))
        ref = R.ref64(w, m, v, g, step=step, **hp, **kw)
        w1 = R.restated_fp32(w, m, v, g, step=step, mutation=mutation, **hp, **kw)[0]
        r = R.ratios(w1, *ref["w"])
        per_step[step], share[step] = float(r.max()), float((r > 1).double().mean())
    print("optim_ref mutation", json.dumps({"mutation": mutation, "worst_master_error_over_tolerance": per_step, "share_of_elements_over_the_bar": share}))
    assert all(x >= 3.0 for x in per_step.values()), per_step
    assert max(share.values()) >= 0.25, share


@pytest.mark.parametrize("n", SUMSQ_NS)
def test_sumsq_probes_name_every_edge(n):
    """the one-hot index set of length n: inside [0, n), and holding 0, 7, 8, the first element of the second grid stride, both ends of the last
    full vector, every tail element and (beyond the grid cap) the same edges of the last stride - stated here independently of sumsq_probe_edges"""
    probes = R.sumsq_probes(n)
    assert probes == sorted(set(probes)) and 0 <= probes[0] and probes[-1] < n
    nv = n // 8
    grid = min(-(-(-(-n // 8)) // 256), 1024)
    assert grid == R.sumsq_grid(n)
    want = [i for i in (0, 7, 8, 8 * 256 * grid) if i < n]
    if nv:
        want += [8 * (nv - 1), 8 * nv - 1]
    want += list(range(8 * nv, n))
    if nv > 256 * 1024:
        last = (nv - 1) // (256 * 1024) * (8 * 256 * 1024)
        assert last > 0 and last + 8 * 256 * 1024 >= 8 * nv
        want += [i for i in (last, last + 7, last + 8) if i < n]
    assert set(want) <= set(probes), sorted(set(want) - set(probes))
    assert len(probes) <= 24
    # all-ones input: the count and count + 5 are exact in fp32
    assert n + 5 < 2 ** 24 and float(torch.tensor(float(n + 5), dtype=torch.float32)) == n + 5
    assert R.sumsq_terms_per_thread(n) == 8 * -(-(-(-n // 8)) // (256 * grid))


def test_sumsq_probe_list_reaches_both_sides_of_the_cap():
    assert R.sumsq_grid(8 * 256 * 1024 - 8) == R.sumsq_grid(8 * 256 * 1024) == 1024 and R.sumsq_terms_per_thread(8 * 256 * 1024) == 8
    assert R.sumsq_terms_per_thread(8 * 256 * 1024 + 8) == 16 and 8 * 256 * 1024 in R.sumsq_probes(8 * 256 * 1024 + 8)
    assert R.sumsq_grid(2047) == 1 and R.sumsq_grid(2049) == 2 and R.sumsq_probes(7) == list(range(7))


def test_clip_coef_reference():
    s = torch.tensor([4.0, 12.0], dtype=torch.float32)
    assert R.clip_coef(s, 0.5, 1.0) == (2.0, 1.0 / (2.0 + 1e-6))
    assert R.clip_coef(s, 0.5, 10.0)[1] == 1.0
    assert R.clip_coef_check(2.0, 0.9, s, 0.5, 10.0)[1] == float("inf")   # far below max_norm the coefficient must be exactly 1
    rn, rc = R.clip_coef_check(2.0, float(torch.tensor(1.0 / (2.0 + 1e-6), dtype=torch.float32)), s, 0.5, 1.0)
    assert rn == 0.0 and rc <= 0.25


def test_adamw_ops_refuse_bad_buffers_before_the_c_call(monkeypatch):
    """ops.adamw_step / ops.adamw_step_t: a wrongly typed, short or strided buffer, or a shadow that cannot hold [K, N], raises AfkError without the
    library being loaded or called"""
    from audio_flamingo_amd import _lib, ops
    from audio_flamingo_amd._lib import AfkError

    def boom(*a, **k):
        raise AssertionError("the C library was reached")

    monkeypatch.setattr(_lib, "call", boom)
    monkeypatch.setattr(_lib, "load", boom)
    hp = dict(lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.01, step=1)
    N_, K_ = 64, 128
    n = N_ * K_
    f32 = lambda k=n: torch.zeros(k, dtype=torch.float32)
    b16 = lambda k=n: torch.zeros(k, dtype=torch.bfloat16)
    good = dict(master=f32(), m=f32(), v=f32(), grad=b16(), param=b16())
    bad = [("master", b16(), "master: expected dtype"), ("m", b16(), " m: expected dtype"), ("v", f32().double(), " v: expected dtype"),
           ("grad", f32(), "grad: expected dtype"), ("param", f32(), "param: expected dtype"),
           ("master", f32(n - 1), "master: .* elements"), ("m", f32(n - 4), " m: .* elements"), ("v", f32(n + 4), " v: .* elements"),
           ("grad", b16(n - 8), "grad: .* elements"), ("m", f32(2 * n)[::2], " m: not contiguous"), ("grad", b16(2 * n)[::2], "grad: not contiguous")]
    shadow = torch.zeros(K_, N_, dtype=torch.bfloat16)
    for name, t, msg in bad:
        a = dict(good, **{name: t})
        with pytest.raises(AfkError, match=msg):
            ops.adamw_step(a["master"], a["m"], a["v"], a["grad"], a["param"], **hp)
        with pytest.raises(AfkError, match=msg):
            ops.adamw_step_t(a["master"], a["m"], a["v"], a["grad"], a["param"], shadow, N_, K_, **hp)
    g = good
    with pytest.raises(AfkError, match="master: 8192 elements, expected 12288"):   # the transposed form: every stream holds N * K elements
        ops.adamw_step_t(g["master"], g["m"], g["v"], g["grad"], g["param"], shadow, N_, K_ + 64, **hp)
    for sh, msg in ((torch.zeros(K_, N_, dtype=torch.float32), "shadow: expected dtype"), (torch.zeros(K_ - 1, N_, dtype=torch.bfloat16), "cannot hold"),
                    (torch.zeros(K_, N_ - 8, dtype=torch.bfloat16), "cannot hold"), (torch.zeros(N_, K_, dtype=torch.bfloat16).t(), "cannot hold"),
                    (torch.zeros(K_ * N_, dtype=torch.bfloat16), "cannot hold")):
        with pytest.raises(AfkError, match=msg):
            ops.adamw_step_t(g["master"], g["m"], g["v"], g["grad"], g["param"], sh, N_, K_, **hp)
    # well-formed CPU buffers get as far as the device check: there is no CPU fallback
    with pytest.raises(AfkError, match="HIP device tensor"):
        ops.adamw_step(g["master"], g["m"], g["v"], g["grad"], g["param"], **hp)
    with pytest.raises(AfkError, match="HIP device tensor"):
        ops.adamw_step_t(g["master"], g["m"], g["v"], g["grad"], g["param"], shadow, N_, K_, **hp)

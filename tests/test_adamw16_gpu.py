"""AdamW with bf16 optimizer state (state_dtype="bf16": afk_adamw16_step / afk_adamw16_step_t, 14 B/param) on MI355X: the kernels against
torch.optim.AdamW(fused=True) on bf16 tensors and against the float64 restatement (tests/_adamw16_ref.py holds the derived per-element bar), the
flat and the transposed-shadow launch against each other bit for bit, and the mode through FusedAdamW / AfkAdamW / AfkTrainer: plain step,
overlapped per-bucket schedule, HIP-graph replay, checkpoint round trip.  Every device step runs once."""
import json
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

from tests._adamw16_ref import bias_corrections, make_grad, make_params, ref64, worst_ratio
from tests.test_model_gpu import G, _cfg, _fresh_model

HP = dict(lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.01)


@pytest.fixture(autouse=True)
def _collect_models_after_each_test():
    """model <-> arena reference cycles die only in a garbage collection; the arena's finalizer drops its entries from the stage-operator tables
    (stage_ops._purge).  Collect here, so that no dead arena of this file is finalized in the middle of a later test's torch.compile trace, which
    guards on those tables."""
    yield
    import gc

    gc.collect()
    torch.cuda.empty_cache()


def _assert_bound(got, ref, label):
    """got = (p, m, v) stored results, ref = ref64(...) of the same inputs"""
    out = {}
    for name, x in zip("pmv", got):
        out[name] = worst_ratio(x, *ref[name])
    print(f"{label}: worst |x - X| / tolerance  p {out['p']:.4f}  m {out['m']:.4f}  v {out['v']:.4f}")
    return out


@pytest.mark.parametrize("n", [1000003, (1 << 22) + 8])
def test_adamw16_matches_torch_fused(dev, n):
    """the op against torch.optim.AdamW(fused=True) on bf16 clones on the device, step by step from IDENTICAL state (every step continues from torch's
    state, so one rounding-tie flip cannot compound): ours and torch's results both inside the derived bound on every element of p / m / v; the share
    of elements where the two differ in any bit is measured (printed as one JSON line; on record in profiles/adamw16_parity.md) and must stay <= 1e-2 per
    tensor (a wrong-but-close formula, e.g. m = b1*m + (1-b1)*g, measures 2.5e-3; torch's forms 3e-5 on the CPU).  Then one step each with a thin
    grid, a closed gate, an open gate, and device-side hyper-parameters that differ from the scalar arguments."""
    from audio_flamingo_amd import ops

    steps = 8
    p_t = make_params(n, dev, seed=n % 97).clone().requires_grad_(True)
    topt = torch.optim.AdamW([p_t], lr=HP["lr"], betas=(HP["beta1"], HP["beta2"]), eps=HP["eps"], weight_decay=HP["weight_decay"], fused=True)
    m0, v0 = torch.zeros(n, device=dev, dtype=torch.bfloat16), torch.zeros(n, device=dev, dtype=torch.bfloat16)
    differ = {"p": 0, "m": 0, "v": 0}
    worst_ours, worst_torch = {"p": 0.0, "m": 0.0, "v": 0.0}, {"p": 0.0, "m": 0.0, "v": 0.0}
    for step in range(1, steps + 1):
        g = make_grad(n, step, dev, seed=n % 97)
        p0 = p_t.detach().clone()
        if step > 1:
            st = topt.state[p_t]
            m0, v0 = st["exp_avg"].clone(), st["exp_avg_sq"].clone()
        p_t.grad = g.clone()
        topt.step()
        st = topt.state[p_t]
        assert st["exp_avg"].dtype == torch.bfloat16 and int(st["step"]) == step
        p, m, v = p0.clone(), m0.clone(), v0.clone()
        ops.adamw16_step(m, v, g, p, step=step, **HP)
        torch.cuda.synchronize()
        bc1, bc2s = bias_corrections(HP["beta1"], HP["beta2"], step)
        ref = ref64(p0, m0, v0, g, bc1=bc1, bc2_sqrt=bc2s, **HP)
        ro = _assert_bound((p, m, v), ref, f"n={n} step {step} ours ")
        rt = _assert_bound((p_t.detach(), st["exp_avg"], st["exp_avg_sq"]), ref, f"n={n} step {step} torch")
        for name, a, b in (("p", p, p_t.detach()), ("m", m, st["exp_avg"]), ("v", v, st["exp_avg_sq"])):
            differ[name] += int((a.view(torch.int16) != b.view(torch.int16)).sum())
            worst_ours[name], worst_torch[name] = max(worst_ours[name], ro[name]), max(worst_torch[name], rt[name])
    share = {k: c / (n * steps) for k, c in differ.items()}
    print("adamw16 parity", json.dumps({"n": n, "steps": steps, "share_of_elements_differing_from_torch": share,
                                        "worst_error_over_tolerance_ours": worst_ours, "worst_error_over_tolerance_torch": worst_torch}))
    assert all(r <= 1.0 for r in worst_torch.values()), f"torch's own fused AdamW leaves the derived bound ({worst_torch}): the premise of this test is wrong, not the kernel"
    assert all(r <= 1.0 for r in worst_ours.values()), f"adamw16_step leaves the derived bound: {worst_ours}"
    assert all(s <= 1e-2 for s in share.values()), f"adamw16_step differs from torch's fused AdamW on too many elements for the same formula: {share}"

    # ---- one step each: thin grid, closed gate, open gate, device-side hyper
    step = steps + 1
    g = make_grad(n, step, dev, seed=n % 97)
    st = topt.state[p_t]
    p0, m0, v0 = p_t.detach().clone(), st["exp_avg"].clone(), st["exp_avg_sq"].clone()
    bc1, bc2s = bias_corrections(HP["beta1"], HP["beta2"], step)
    full = [p0.clone(), m0.clone(), v0.clone()]
    ops.adamw16_step(full[1], full[2], g, full[0], step=step, **HP)
    thin = [p0.clone(), m0.clone(), v0.clone()]
    ops.adamw16_step(thin[1], thin[2], g, thin[0], step=step, max_blocks=3, **HP)
    gate = torch.zeros(1, device=dev, dtype=torch.int32)
    shut, g_shut = [p0.clone(), m0.clone(), v0.clone()], g.clone()
    ops.adamw16_step(shut[1], shut[2], g_shut, shut[0], step=step, gate=gate, **HP)
    gate1 = torch.ones(1, device=dev, dtype=torch.int32)
    opened = [p0.clone(), m0.clone(), v0.clone()]
    ops.adamw16_step(opened[1], opened[2], g, opened[0], step=step, gate=gate1, **HP)
    torch.cuda.synchronize()
    ref = ref64(p0, m0, v0, g, bc1=bc1, bc2_sqrt=bc2s, **HP)
    ro = _assert_bound(full, ref, f"n={n} step {step} full grid")
    assert all(r <= 1.0 for r in ro.values()), ro
    for a, b, c, d, e in zip(full, thin, opened, shut, (p0, m0, v0)):
        assert torch.equal(a, b), "max_blocks=3 (grid-stride over the whole range) changed the result"
        assert torch.equal(a, c), "an open gate changed the result"
        assert torch.equal(d, e), "a closed gate must leave every buffer bit-unchanged"
    assert torch.equal(g_shut, g)
    # hyper = (lr, 1 - beta1^t, sqrt(1 - beta2^t), gradient multiplier) on the device wins over the scalar arguments
    hyper = torch.tensor([3e-3, 0.5, 0.25, 0.5], device=dev, dtype=torch.float32)
    hv = [float(x) for x in hyper.double().cpu()]   # the fp32 values the kernel reads, widened exactly
    hy = [p0.clone(), m0.clone(), v0.clone()]
    ops.adamw16_step(hy[1], hy[2], g, hy[0], step=step, grad_scale=2.0, hyper=hyper, **HP)
    torch.cuda.synchronize()
    ref_h = ref64(p0, m0, v0, g, bc1=hv[1], bc2_sqrt=hv[2], grad_scale=2.0 * hv[3], **dict(HP, lr=hv[0]))
    rh = _assert_bound(hy, ref_h, f"n={n} step {step} device hyper")
    assert all(r <= 1.0 for r in rh.values()), rh
    assert not torch.equal(hy[0], full[0])


@pytest.mark.parametrize("N,K", [(256, 192), (3584, 512)])
def test_adamw16_transposed_shadow(dev, N, K):
    """afk_adamw16_step_t on one [N, K] weight: p / m / v bit-identical to the flat launch and shadow == p.t() exactly (mirrors
    tests/test_model_gpu.py::test_adamw_fused_transposed_shadow at the op level), for a full and a thin grid"""
    from audio_flamingo_amd import ops

    n = N * K
    p0 = make_params(n, dev, seed=5)
    m0 = (make_grad(n, 0, dev, seed=6).float() * 0.5).to(torch.bfloat16)
    v0 = (make_grad(n, 1, dev, seed=7).float() ** 2).to(torch.bfloat16)
    g = make_grad(n, 3, dev, seed=8)
    flat = [p0.clone(), m0.clone(), v0.clone()]
    ops.adamw16_step(flat[1], flat[2], g, flat[0], step=4, **HP)
    for max_blocks in (0, 5):
        tr = [p0.clone(), m0.clone(), v0.clone()]
        shadow = torch.full((K, N), 7.0, device=dev, dtype=torch.bfloat16)
        ops.adamw16_step_t(tr[1], tr[2], g, tr[0], shadow, N, K, step=4, max_blocks=max_blocks, **HP)
        torch.cuda.synchronize()
        for name, a, b in zip("pmv", tr, flat):
            assert torch.equal(a, b), f"{name}: the transposed-shadow launch differs from the flat launch (max_blocks={max_blocks})"
        assert torch.equal(shadow, tr[0].view(N, K).t()), f"shadow != transpose(param) (max_blocks={max_blocks})"
    assert not torch.equal(flat[0], p0)


def _batch(dev, case="tiny64_caseB.pt"):
    g = torch.load(os.path.join(G, case))
    return dict(input_ids=g["ids"].to(dev), input_features=g["feats"].to(dev), input_features_mask=g["fmask"].to(dev), labels=g["labels"].to(dev))


def test_bf16_state_optimizer_on_the_tiny_model(dev):
    """AfkAdamW(state_dtype="bf16") through the tiny model, three steps with clipping on (the third on a text-only batch): per arena block the new
    p / m / v against the float64 restatement of the update (gradient x clip coefficient in float64, wd = 0 on the non-decayed blocks) inside the
    derived bound; blocks whose gradient was not written keep p / m / v bit-unchanged; no master, 4 B/param of state.  Cross-check with clipping
    off: torch.optim.AdamW(fused=True) on bf16 clones of one decayed 2-D weight and one non-decayed vector, held to the same bound."""
    from audio_flamingo_amd.trainer import AfkAdamW

    m = _fresh_model(dev, seed=21)
    A = m.arena
    lr, wd = 1e-3, 0.01
    opt = AfkAdamW(m, lr=lr, weight_decay=wd, state_dtype="bf16")
    f = opt.fused
    assert f.master is None and f.m.dtype == f.v.dtype == torch.bfloat16 and f.state_bytes() == 4 * A.total
    f.clip_norm = 1.0
    kw = _batch(dev)
    text_only = dict(input_ids=kw["input_ids"].clamp(max=1000), labels=kw["labels"])
    hp = dict(lr=lr, beta1=0.9, beta2=0.999, eps=1e-8)
    saw_fresh = False
    for step in range(1, 4):
        opt.zero_grad()
        m(**(text_only if step == 3 else kw)).loss.backward()
        A.join_streams()
        torch.cuda.synchronize()
        before = [t.detach().clone() for t in (A.params, A.grads, f.m, f.v)]
        fresh = {b.key: b.fresh for b in A.order}
        opt.step()
        torch.cuda.synchronize()
        coef = float(f.hyper[3].double())
        assert 0.0 < coef <= 1.0
        bc1, bc2s = bias_corrections(0.9, 0.999, step)
        worst = {"p": (0.0, ""), "m": (0.0, ""), "v": (0.0, "")}
        tiny_v = 0
        for b in A.order:
            sl = slice(b.offset, b.offset + b.numel)
            now = (A.params.detach()[sl], f.m[sl], f.v[sl])
            if fresh[b.key]:
                saw_fresh = True
                for name, x, old in zip("pmv", now, (before[0][sl], before[2][sl], before[3][sl])):
                    assert torch.equal(x, old), f"step {step}: {b.key} got no gradient this step but its {name} changed"
                continue
            ref = ref64(before[0][sl], before[2][sl], before[3][sl], before[1][sl], bc1=bc1, bc2_sqrt=bc2s, grad_scale=coef,
                        weight_decay=wd if b.decay else 0.0, **hp)
            tiny_v += int(((ref["v"][0] > 0) & (ref["v"][0] < 2.0 ** -126)).sum())
            for name, x in zip("pmv", now):
                r = worst_ratio(x, *ref[name])
                if r > worst[name][0]:
                    worst[name] = (r, b.key)
        print(f"model step {step}: clip coefficient {coef:.5f}; worst |x - X| / tolerance {worst}; v elements below the bf16 normal range: {tiny_v}")
        for name, (r, key) in worst.items():
            assert r <= 1.0, f"step {step}: {name} of {key} leaves the derived bound ({r:.3f} x the tolerance)"
        if step == 3:
            assert any(fresh[k] for k in fresh if k.startswith("model.audio_tower")), "the text-only step must leave the audio tower without gradients"
    assert saw_fresh and f.t == 3

    # cross-check against torch on two blocks, clipping off (torch applies no coefficient)
    f.clip_norm = None
    opt.zero_grad()
    m(**kw).loss.backward()
    A.join_streams()
    torch.cuda.synchronize()
    blocks = [next(b for b in A.order if b.decay and len(b.shape) == 2 and "language_model.layers.0" in b.key),
              next(b for b in A.order if not b.decay and len(b.shape) == 1 and "language_model.layers.0" in b.key)]
    snaps = []
    for b in blocks:
        sl = slice(b.offset, b.offset + b.numel)
        snaps.append([t.detach()[sl].clone() for t in (A.params, A.grads, f.m, f.v)])
    opt.step()
    torch.cuda.synchronize()
    assert float(f.hyper[3]) == 1.0
    bc1, bc2s = bias_corrections(0.9, 0.999, 4)
    for b, (p0, g0, m0, v0) in zip(blocks, snaps):
        sl = slice(b.offset, b.offset + b.numel)
        wd_b = wd if b.decay else 0.0
        p_t = p0.clone().requires_grad_(True)
        topt = torch.optim.AdamW([p_t], lr=lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=wd_b, fused=True)
        topt.state[p_t] = {"step": torch.tensor(3.0, device=dev), "exp_avg": m0.clone(), "exp_avg_sq": v0.clone()}
        p_t.grad = g0.clone()
        topt.step()
        torch.cuda.synchronize()
        ref = ref64(p0, m0, v0, g0, bc1=bc1, bc2_sqrt=bc2s, weight_decay=wd_b, **hp)
        st = topt.state[p_t]
        for who, got in (("ours", (A.params.detach()[sl], f.m[sl], f.v[sl])), ("torch", (p_t.detach(), st["exp_avg"], st["exp_avg_sq"]))):
            for name, x in zip("pmv", got):
                r = worst_ratio(x, *ref[name])
                print(f"cross-check {b.key} {who} {name}: {r:.4f} x the tolerance")
                assert r <= 1.0, f"{b.key}: {who} {name} leaves the derived bound ({r:.3f} x the tolerance)"


def test_bf16_state_overlap_and_graph_match_plain_step(dev):
    """bf16 state: the overlapped per-bucket schedule (thin AdamW launches on the side stream inside backward) and a GraphedTrainStep replay give
    bit-identical parameters and m / v to the plain step(), over two steps (the fp32-mode twins: tests/test_model_gpu.py
    test_wgrad_stream_and_optimizer_overlap_match_serial_path / test_graphed_step_matches_eager)"""
    from audio_flamingo_amd.arena import FusedAdamW
    from audio_flamingo_amd.dp import BackwardOverlap
    from audio_flamingo_amd.graphs import GraphedTrainStep

    kw = _batch(dev)
    ms, opts, ovs = [], [], []
    for i in range(3):   # 0: plain step, 1: overlapped eager, 2: overlapped + graph replay
        m = _fresh_model(dev, seed=23)
        m.check_placeholders = False
        if i:
            m.arena.enable_wgrad_stream(True)
        o = FusedAdamW(m.arena, lr=1e-3, weight_decay=0.01, state_dtype="bf16")
        assert o.master is None
        ms.append(m), opts.append(o), ovs.append(BackwardOverlap(m.arena, o) if i else None)

    def plain():
        ms[0].zero_grad()
        loss = ms[0](**kw).loss
        loss.backward()
        opts[0].step()
        return loss

    def body(i):
        def f():
            ms[i].zero_grad()
            ovs[i].begin_step()
            loss = ms[i](**kw).loss
            loss.backward()
            ovs[i].finish()
            return loss
        return f

    over = body(1)
    gstep = GraphedTrainStep(ms[2], opts[2], ovs[2], body(2), warmup=2)   # two eager warm-up steps, then the capture
    for _ in range(2):
        plain(), over()
    for k in range(2):
        for o in opts:
            o.lr = 1e-3 * (1 + k)   # a schedule: must reach the captured launches through hyper
        la, lb, lc = plain(), over(), gstep()
        torch.cuda.synchronize()
        la, lb, lc = float(la.detach()), float(lb.detach()), float(lc.detach())
        assert la == lb == lc, (k, la, lb, lc)
        assert opts[0].t == opts[1].t == opts[2].t
        for i, what in ((1, "overlapped schedule"), (2, "graph replay")):
            assert torch.equal(ms[0].arena.params, ms[i].arena.params), f"step {k}: parameters of the {what} differ from the plain step"
            assert torch.equal(opts[0].m, opts[i].m) and torch.equal(opts[0].v, opts[i].v), f"step {k}: m / v of the {what} differ from the plain step"
    assert bool(opts[0].m.any()) and bool(opts[0].v.any())
    for key in ("model.language_model.layers.0.mlp.gate_up.weight", "model.audio_tower.conv2.weight"):
        for i in (1, 2):
            assert torch.equal(ms[0].arena.shadow(key), ms[i].arena.shadow(key)), f"stale W^T shadow for {key}"


def test_bf16_state_checkpoint_roundtrip(dev):
    """state_dict() -> a fresh model with the same weights -> load_state_dict() -> one more step: parameters bit-identical to the uninterrupted run;
    the checkpoint holds m / v / t only (the weights travel in the model checkpoint and load_state_dict does not write them); a checkpoint of the
    other state mode is refused with an AfkError that names both dtypes"""
    from audio_flamingo_amd._lib import AfkError
    from audio_flamingo_amd.trainer import AfkAdamW

    kw = _batch(dev)
    m = _fresh_model(dev, seed=29)
    opt = AfkAdamW(m, lr=1e-3, weight_decay=0.01, state_dtype="bf16")
    for _ in range(2):
        opt.zero_grad(); m(**kw).loss.backward(); opt.step()
    torch.cuda.synchronize()
    sd = opt.state_dict()
    assert sorted(sd["state"]) == ["m", "t", "v"] and sd["state_dtype"] == "bf16" and "param_groups" in sd
    sd = {"state": {k: (v.clone() if torch.is_tensor(v) else v) for k, v in sd["state"].items()}, "state_dtype": sd["state_dtype"],
          "param_groups": sd["param_groups"]}
    weights = {k: v.detach().clone() for k, v in m.state_dict().items()}
    opt.zero_grad(); m(**kw).loss.backward(); opt.step()
    torch.cuda.synchronize()

    m2 = _fresh_model(dev, seed=31)   # other weights until the model checkpoint is loaded
    m2.load_state_dict(weights)
    opt2 = AfkAdamW(m2, lr=1e-3, weight_decay=0.01, state_dtype="bf16")
    held = m2.arena.params.detach().clone()
    opt2.load_state_dict(sd)
    assert torch.equal(m2.arena.params, held), "load_state_dict of the bf16 mode must not write the parameters"
    assert opt2.fused.t == 2 and torch.equal(opt2.fused.m, sd["state"]["m"]) and torch.equal(opt2.fused.v, sd["state"]["v"])
    opt2.zero_grad(); m2(**kw).loss.backward(); opt2.step()
    torch.cuda.synchronize()
    assert torch.equal(m2.arena.params, m.arena.params), "resumed run differs from the uninterrupted run"
    assert torch.equal(opt2.fused.m, opt.fused.m) and torch.equal(opt2.fused.v, opt.fused.v)

    opt32 = AfkAdamW(_fresh_model(dev, seed=29), lr=1e-3, weight_decay=0.01, state_dtype="fp32")
    with pytest.raises(AfkError, match="(?s)bf16.*fp32"):
        opt32.load_state_dict(sd)
    with pytest.raises(AfkError, match="(?s)fp32.*bf16"):
        opt2.load_state_dict(opt32.state_dict())


def test_trainer_builds_bf16_state_from_optim_args(dev, tmp_path):
    """AfkTrainer with optim_args="state_dtype=bf16": the stock training-script shape of tests/test_model_gpu.py::test_hf_trainer_runs_unchanged_script
    runs two optimizer steps (LR schedule, clipping, gradient accumulation 2) on an optimizer with bf16 state and no master"""
    from transformers import TrainingArguments

    from audio_flamingo_amd.modeling import AudioFlamingo3ForConditionalGeneration as Mine
    from audio_flamingo_amd.trainer import AfkAdamW, AfkTrainer

    g = torch.load(os.path.join(G, "tiny64_caseA.pt"))
    rows = [dict(input_ids=g["ids"][i % 2], input_features=g["feats"][i % 2].float(), input_features_mask=g["fmask"][i % 2], labels=g["labels"][i % 2])
            for i in range(8)]
    args = TrainingArguments(output_dir=str(tmp_path / "afk16"), per_device_train_batch_size=2, gradient_accumulation_steps=2, max_steps=2,
                             learning_rate=2e-3, weight_decay=0.01, lr_scheduler_type="linear", warmup_steps=1, logging_steps=1,
                             save_strategy="no", report_to=[], remove_unused_columns=False, dataloader_pin_memory=False, max_grad_norm=1.0,
                             seed=0, optim_args="state_dtype=bf16")
    m = Mine(_cfg(), device=dev, init_seed=7)
    start = m.arena.params.detach().clone()
    tr = AfkTrainer(model=m, args=args, train_dataset=rows)
    tr.train()
    opt = getattr(tr.optimizer, "optimizer", tr.optimizer)
    assert isinstance(opt, AfkAdamW) and opt.fused.t == 2
    assert opt.fused.state_dtype == "bf16" and opt.fused.master is None and opt.fused.m.dtype == opt.fused.v.dtype == torch.bfloat16
    assert opt.fused.state_bytes() == 4 * m.arena.total
    log = [(h["loss"], h["grad_norm"]) for h in tr.state.log_history if "loss" in h]
    assert len(log) == 2 and all(l == l and gn > 0 for l, gn in log), log
    assert not torch.equal(m.arena.params, start) and bool(torch.isfinite(m.arena.params.float()).all())

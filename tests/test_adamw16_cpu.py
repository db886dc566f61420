"""AdamW with bf16 optimizer state, host side (no GPU): the state_dtype switch of FusedAdamW / ShardedAdamW / AfkAdamW - launch plans, which operator
every launch goes to, the environment default, checkpoint layout and refusal across modes - with the launch replaced by a recording torch stand-in
(there is no CPU kernel path); and the premise of the GPU test's numerical bar, on the CPU: torch.optim.AdamW(fused=True) on bf16 tensors and the
fp32 restatement of csrc/elementwise.hip adamw16_elem both stay inside the derived per-element bound (tests/_adamw16_ref.py)."""
import os
import subprocess
import sys

import pytest
import torch

from tests._adamw16_ref import bias_corrections, make_grad, make_params, ref64, restated_fp32, worst_ratio

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the tiny configuration of the model tests
TINY = dict(
    audio_config=dict(num_mel_bins=128, num_hidden_layers=2, num_attention_heads=4, intermediate_size=256, hidden_size=128,
                      max_source_positions=1500),
    text_config=dict(vocab_size=1024, hidden_size=256, intermediate_size=512, num_hidden_layers=2, num_attention_heads=4,
                     num_key_value_heads=2, max_position_embeddings=4096),
    audio_token_id=1023,
)


def _tiny_model(seed=5):
    from transformers import AudioFlamingo3Config

    from audio_flamingo_amd.modeling import AudioFlamingo3ForConditionalGeneration as Mine

    return Mine(AudioFlamingo3Config(**TINY), device="cpu", init_seed=seed)


def _stubs(monkeypatch, calls):
    """recording stand-ins for the four AdamW launches: (operator name, arena offset of param, numel); the bf16-state one applies the update"""
    from audio_flamingo_amd import ops

    def adamw16(m, v, grad, param, *, lr, beta1, beta2, eps, weight_decay, step, grad_scale=1.0, max_blocks=0, gate=None, hyper=None):
        assert m.dtype == v.dtype == grad.dtype == param.dtype == torch.bfloat16 and m.numel() == v.numel() == grad.numel() == param.numel()
        calls.append(("adamw16_step", param.data_ptr(), param.numel(), weight_decay))
        if gate is not None and int(gate[0]) == 0:
            return
        bc1, bc2s = bias_corrections(beta1, beta2, step)
        p, mm, vv = restated_fp32(param, m, v, grad, lr=lr, beta1=beta1, beta2=beta2, eps=eps, weight_decay=weight_decay, bc1=bc1, bc2_sqrt=bc2s,
                                  grad_scale=grad_scale)
        param.copy_(p), m.copy_(mm), v.copy_(vv)

    def adamw32(master, m, v, grad, param, **kw):
        assert master.dtype == m.dtype == v.dtype == torch.float32
        calls.append(("adamw_step", param.data_ptr(), param.numel(), kw["weight_decay"]))

    def adamw16_t(m, v, grad, param, shadow, N, K, **kw):
        assert m.dtype == v.dtype == torch.bfloat16
        calls.append(("adamw16_step_t", param.data_ptr(), param.numel(), kw["weight_decay"]))

    def adamw32_t(master, m, v, grad, param, shadow, N, K, **kw):
        calls.append(("adamw_step_t", param.data_ptr(), param.numel(), kw["weight_decay"]))

    monkeypatch.setattr(ops, "adamw16_step", adamw16, raising=True)   # raising: the operator must exist
    monkeypatch.setattr(ops, "adamw16_step_t", adamw16_t, raising=True)
    monkeypatch.setattr(ops, "adamw_step", adamw32)
    monkeypatch.setattr(ops, "adamw_step_t", adamw32_t)


def test_c_abi_declares_the_bf16_state_entries():
    """include/afk.h declares afk_adamw16_step / afk_adamw16_step_t without a master and with void* moments; the built library exports them
    (_lib derives the argtypes from the header)"""
    from audio_flamingo_amd import _lib, ops

    lib = _lib.load()
    assert hasattr(lib, "afk_adamw16_step") and hasattr(lib, "afk_adamw16_step_t")
    hdr = open(os.path.join(ROOT, "include", "afk.h")).read()
    decl = hdr[hdr.index("int afk_adamw16_step("):]
    decl = decl[:decl.index(";")]
    assert "master" not in decl and "void* m, void* v" in decl and "const float* hyper" in decl and "const int* gate" in decl
    assert callable(ops.adamw16_step) and callable(ops.adamw16_step_t)
    with pytest.raises(_lib.AfkError):   # no CPU fallback
        z = torch.zeros(64, dtype=torch.bfloat16)
        ops.adamw16_step(z, z.clone(), z.clone(), z.clone(), lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.0, step=1)


def test_custom_op_is_registered():
    import audio_flamingo_amd.custom_ops  # noqa: F401

    schema = str(torch.ops.afk.adamw16_step.default._schema)
    import re

    assert re.match(r"afk::adamw16_step\(Tensor\(a\d!\) m, Tensor\(a\d!\) v, Tensor grad, Tensor\(a\d!\) param, float lr", schema), schema   # m, v, param mutated
    assert "master" not in schema and "Tensor? gate=None, Tensor? hyper=None" in schema


def test_state_dtype_switch_plans_and_launch_targets(monkeypatch):
    """FusedAdamW(arena, state_dtype="bf16") on a CPU arena: launch plans identical to the fp32 mode (flat and with the transposed-shadow option),
    every launch goes to adamw16_step[_t], master is None, 4 B/param of state; AFK_ADAMW_STATE picks the mode when the argument is None and an
    unknown value raises"""
    from audio_flamingo_amd._lib import AfkError
    from audio_flamingo_amd.arena import FusedAdamW

    monkeypatch.delenv("AFK_ADAMW_STATE", raising=False)
    m = _tiny_model()
    A = m.arena
    o32 = FusedAdamW(A, lr=1e-3, weight_decay=0.01)
    o16 = FusedAdamW(A, lr=1e-3, weight_decay=0.01, state_dtype="bf16")
    assert o32.state_dtype == "fp32" and o32.master is not None and o32.master.dtype == torch.float32 and o32.state_bytes() == 12 * A.total
    assert o16.state_dtype == "bf16" and o16.master is None and o16.m.dtype == o16.v.dtype == torch.bfloat16
    assert o16.m.numel() == o16.v.numel() == A.total and o16.state_bytes() == 4 * A.total
    key = lambda plan: [(op[0], op[1].key if op[0] == "T" else op[1], op[2], op[3] if op[0] == "flat" else None) for op in plan]
    assert key(o16.segments) == key(o32.segments) and len(o16.segments) > 1
    assert [key(p) for p in o16.bucket_segments] == [key(p) for p in o32.bucket_segments]
    o16.fuse_shadow = o32.fuse_shadow = True
    assert key(o16.segments) == key(o32.segments) and any(op[0] == "T" for op in o16.segments)
    o16.fuse_shadow = o32.fuse_shadow = False
    # no-ops without a master
    o16.sync_master(), o16._check_master(), o16._mark_synced()
    A.params.data.add_(0)   # a rewrite behind the optimizer's back: nothing to re-derive
    o16._check_master()
    assert o16.master is None

    calls = []
    _stubs(monkeypatch, calls)
    for b in A.order:
        b.grad.copy_(torch.full(b.shape, 1e-3)); A.grad_written(b)
    base = A.params.data_ptr()
    for opt, name in ((o16, "adamw16_step"), (o32, "adamw_step")):
        calls.clear()
        opt.step(refresh_shadows=False)
        assert calls and all(c[0] == name for c in calls), {c[0] for c in calls}
        assert [((c[1] - base) // 2, c[2], c[3]) for c in calls] == [(op[1], op[2] - op[1], op[3]) for op in opt.segments]
    calls.clear()
    o16.step_bucket(1)
    assert calls and all(c[0] == "adamw16_step" for c in calls) and sum(c[2] for c in calls) == A.bucket_range(1)[1] - A.bucket_range(1)[0]
    assert bool(o16.m.any()) and bool(o16.v.any()) and o16.t == 1

    monkeypatch.setenv("AFK_ADAMW_STATE", "bf16")
    assert FusedAdamW(A).state_dtype == "bf16" and FusedAdamW(A).master is None
    assert FusedAdamW(A, state_dtype="fp32").master is not None   # the argument wins over the environment
    monkeypatch.setenv("AFK_ADAMW_STATE", "fp32")
    assert FusedAdamW(A).master is not None
    monkeypatch.setenv("AFK_ADAMW_STATE", "fp8")
    with pytest.raises(AfkError, match="AFK_ADAMW_STATE"):
        FusedAdamW(A)
    monkeypatch.delenv("AFK_ADAMW_STATE")
    with pytest.raises(AfkError, match="state_dtype"):
        FusedAdamW(A, state_dtype="half")


def test_afkadamw_bf16_checkpoint_layout_and_refusal(monkeypatch):
    """trainer.AfkAdamW(state_dtype="bf16"): state_dict() = {"state": {m, v, t}, "state_dtype": "bf16", "param_groups"}; load_state_dict() restores
    m / v / t and leaves the parameters alone; a checkpoint of the other mode is refused (both dtypes named), in both directions"""
    from audio_flamingo_amd._lib import AfkError
    from audio_flamingo_amd.trainer import AfkAdamW, _optim_arg

    monkeypatch.delenv("AFK_ADAMW_STATE", raising=False)
    calls = []
    _stubs(monkeypatch, calls)
    m = _tiny_model()
    A = m.arena
    opt = AfkAdamW(m, lr=1e-3, weight_decay=0.01, state_dtype="bf16")
    for b in A.order:
        b.grad.copy_(torch.full(b.shape, 2e-3)); A.grad_written(b)
    opt.fused.step(refresh_shadows=False)
    sd = opt.state_dict()
    assert sorted(sd["state"]) == ["m", "t", "v"] and sd["state_dtype"] == "bf16" and sd["state"]["t"] == 1 and len(sd["param_groups"]) == 1
    assert sd["state"]["m"].dtype == torch.bfloat16 and sd["state"]["m"].numel() == A.total
    m2 = _tiny_model(seed=9)
    o2 = AfkAdamW(m2, lr=1e-3, weight_decay=0.01, state_dtype="bf16")
    held = m2.arena.params.detach().clone()
    o2.load_state_dict(sd)
    assert torch.equal(m2.arena.params, held) and o2.fused.t == 1
    assert torch.equal(o2.fused.m, opt.fused.m) and torch.equal(o2.fused.v, opt.fused.v)
    o32 = AfkAdamW(m2, lr=1e-3, weight_decay=0.01)
    assert "state_dtype" not in o32.state_dict() and sorted(o32.state_dict()["state"]) == ["m", "master", "t", "v"]   # the fp32 layout is unchanged
    with pytest.raises(AfkError, match="(?s)bf16.*fp32"):
        o32.load_state_dict(sd)
    with pytest.raises(AfkError, match="(?s)fp32.*bf16"):
        o2.load_state_dict(o32.state_dict())

    class Args:
        optim_args = "foo=1, state_dtype=bf16"
    assert _optim_arg(Args, "state_dtype") == "bf16" and _optim_arg(Args, "bar") is None
    Args.optim_args = None
    assert _optim_arg(Args, "state_dtype") is None


def test_bound_holds_for_torch_fused_and_the_fp32_restatement_on_cpu():
    """premise of tests/test_adamw16_gpu.py::test_adamw16_matches_torch_fused, checked where no GPU is needed: over eight consecutive steps from
    identical state, torch.optim.AdamW(fused=True) on bf16 CPU tensors AND the fp32 restatement of adamw16_elem stay inside
    |x - X| <= 2^-8 |X| + 2^-20 A on every element, and the two differ in at most 1e-2 of the elements of each tensor"""
    n, steps = (1 << 18) + 3, 8
    hp = dict(lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.01)
    p_t = make_params(n, "cpu").clone().requires_grad_(True)
    topt = torch.optim.AdamW([p_t], lr=hp["lr"], betas=(0.9, 0.999), eps=hp["eps"], weight_decay=hp["weight_decay"], fused=True)
    m0, v0 = torch.zeros(n, dtype=torch.bfloat16), torch.zeros(n, dtype=torch.bfloat16)
    differ = {"p": 0, "m": 0, "v": 0}
    for step in range(1, steps + 1):
        g = make_grad(n, step, "cpu")
        p0 = p_t.detach().clone()
        if step > 1:
            m0, v0 = topt.state[p_t]["exp_avg"].clone(), topt.state[p_t]["exp_avg_sq"].clone()
        p_t.grad = g.clone()
        topt.step()
        st = topt.state[p_t]
        bc1, bc2s = bias_corrections(0.9, 0.999, step)
        ref = ref64(p0, m0, v0, g, bc1=bc1, bc2_sqrt=bc2s, **hp)
        ours = restated_fp32(p0, m0, v0, g, bc1=bc1, bc2_sqrt=bc2s, **hp)
        for name, a, b in zip("pmv", ours, (p_t.detach(), st["exp_avg"], st["exp_avg_sq"])):
            ra, rb = worst_ratio(a, *ref[name]), worst_ratio(b, *ref[name])
            assert rb <= 1.0, f"step {step}: torch's fused AdamW leaves the bound on {name} ({rb:.3f} x the tolerance): the bound is wrong"
            assert ra <= 1.0, f"step {step}: the fp32 restatement leaves the bound on {name} ({ra:.3f} x the tolerance)"
            differ[name] += int((a.view(torch.int16) != b.view(torch.int16)).sum())
    share = {k: c / (n * steps) for k, c in differ.items()}
    print("share of elements where the fp32 restatement and torch's fused CPU kernel differ:", share)
    assert all(s <= 1e-2 for s in share.values()), share


SHARDED16_WORKER = r'''
import os, sys, torch, torch.distributed as dist
sys.path.insert(0, sys.argv[1])
from audio_flamingo_amd import ops
from audio_flamingo_amd._lib import AfkError
from audio_flamingo_amd.arena import FusedAdamW, ShardedAdamW, comm_share
from audio_flamingo_amd.dp import DataParallelEngine
import tests.test_adamw16_cpu as T
from tests._adamw16_ref import bias_corrections, restated_fp32

# no CPU kernel path: the bf16-state launch is a recording stand-in (adamw16_elem restated in fp32 tensors) shared by the replicated and the sharded optimizer
launches = []
def adamw16_stub(m, v, grad, param, *, lr, beta1, beta2, eps, weight_decay, step, grad_scale=1.0, max_blocks=0, gate=None, hyper=None):
    assert m.dtype == v.dtype == grad.dtype == param.dtype == torch.bfloat16 and m.numel() == v.numel() == grad.numel() == param.numel()
    launches.append((param.data_ptr(), param.numel()))
    if gate is not None and int(gate[0]) == 0:
        return
    bc1, bc2s = bias_corrections(beta1, beta2, step)
    p, mm, vv = restated_fp32(param, m, v, grad, lr=lr, beta1=beta1, beta2=beta2, eps=eps, weight_decay=weight_decay, bc1=bc1, bc2_sqrt=bc2s, grad_scale=grad_scale)
    param.copy_(p), m.copy_(mm), v.copy_(vv)
def fp32_launch(*a, **k):
    raise AssertionError("a bf16-state optimizer launched the fp32-master kernel")
ops.adamw16_step = adamw16_stub
ops.adamw_step = fp32_launch

dist.init_process_group("gloo")
rank, world = dist.get_rank(), dist.get_world_size()

def run(form):
    os.environ["AFK_DP_FORM"] = form
    m = T._tiny_model(seed=5 + rank)       # different init per rank on purpose
    a = m.arena
    eng = DataParallelEngine(a)
    eng.poison_unowned = True
    eng.broadcast_parameters(0)
    opt = eng.make_optimizer(lr=1e-2, weight_decay=0.01, state_dtype="bf16")
    opt.sync_master()                      # a no-op in this mode
    assert isinstance(opt, ShardedAdamW) == (form == "rs_adamw_ag") and opt.master is None and opt.state_dtype == "bf16"
    seq = []
    for step in range(3):
        a.zero_grad(); eng.begin_backward()
        g = torch.Generator().manual_seed(1000 * step + rank)
        local = (torch.randn(a.total, generator=g) * 0.1).to(torch.bfloat16)
        skip_audio = step == 2                       # all-text step on every rank: the audio buckets' gate reads 0
        for blk in reversed(a.order):
            if skip_audio and (blk.key.startswith("model.audio_tower") or blk.key.startswith("model.multi_modal_projector")):
                continue
            blk.grad.copy_(local[blk.offset: blk.offset + blk.numel].view(blk.shape)); a.grad_written(blk)
        eng.finish()
        launches.clear()
        opt.step(grad_scale=eng.grad_scale, gates=eng.bucket_gate, refresh_shadows=False)
        seq.append((a.params.clone(), list(launches)))
        assert bool(torch.isfinite(a.params.float()).all()), (form, step, "non-finite parameters")
    return m, opt, seq

m_rep, opt_rep, rep = run("rs_ag")
m_sh, opt_sh, sh = run("rs_adamw_ag")
a = m_sh.arena
for step, ((p_rep, l_rep), (p_sh, l_sh)) in enumerate(zip(rep, sh)):
    assert torch.equal(p_rep, p_sh), (step, "sharded bf16-state AdamW + parameter all-gather != replicated", float((p_rep.float() - p_sh.float()).abs().max()))
    base = a.params.data_ptr()
    covered = 0
    for ptr, n in l_sh:
        lo = (ptr - base) // 2
        assert lo % 8 == 0, (step, lo, "a launch that is not 16-byte aligned")
        assert any(a0 <= lo and lo + n <= a1 for a0, a1, _ in opt_sh.owned), (step, lo, n)
        covered += n
    assert covered == opt_sh.state_numel, (covered, opt_sh.state_numel)
    assert sum(n for _, n in l_rep) == a.total
assert not torch.equal(rep[0][0], rep[1][0])
# 1 / world of the optimizer state (+ the replicated tails), bf16, no compact master
tails = sum((e - s) - comm_share(e - s, world) * world for s, e in (a.bucket_range(i) for i in range(len(a.bucket_names))))
assert opt_sh.state_numel == (a.total - tails) // world + tails, (opt_sh.state_numel, a.total, tails)
assert opt_sh.m.dtype == opt_sh.v.dtype == torch.bfloat16 and opt_sh.m.numel() == opt_sh.v.numel() == opt_sh.state_numel < 0.55 * opt_rep.m.numel()
assert opt_sh.state_bytes() == 4 * opt_sh.state_numel and opt_rep.state_bytes() == 4 * a.total
# replicas identical
chk = [None] * world
dist.all_gather_object(chk, [float(a.params.float().sum()), float(a.params.float().abs().sum())])
assert all(c == chk[0] for c in chk), chk
# the consolidated state of the sharded optimizer IS the replicated optimizer's state, bit for bit, on every rank ...
sd = opt_sh.state_dict()
assert sorted(sd["state"]) == ["m", "t", "v"] and sd["state_dtype"] == "bf16" and sd["state"]["t"] == opt_rep.t == 3 and sd["layout"]["numel"] == a.total
for name in ("m", "v"):
    assert sd["state"][name].dtype == torch.bfloat16 and sd["state"][name].shape == (a.total,) and torch.equal(sd["state"][name], getattr(opt_rep, name)), name
# ... and loads back into a fresh sharded optimizer: compact state and step count restored, the parameters left to the model checkpoint
os.environ["AFK_DP_FORM"] = "rs_adamw_ag"
m2 = T._tiny_model(seed=99 + rank)
e2 = DataParallelEngine(m2.arena)
o2 = e2.make_optimizer(lr=1e-2, weight_decay=0.01, state_dtype="bf16")
held = m2.arena.params.detach().clone()
o2.load_state_dict(sd)
assert o2.t == 3 and torch.equal(o2.m, opt_sh.m) and torch.equal(o2.v, opt_sh.v) and torch.equal(m2.arena.params, held)
# a checkpoint of the other mode is refused
o32 = e2.make_optimizer(lr=1e-2, weight_decay=0.01, state_dtype="fp32")
try:
    o32.load_state_dict(sd)
    raise SystemExit("an fp32-state ShardedAdamW loaded a bf16 checkpoint")
except AfkError as e:
    assert "bf16" in str(e) and "fp32" in str(e), str(e)
dist.destroy_process_group()
print("OK", rank)
'''


def test_sharded_bf16_state_equals_replicated_gloo_world2(tmp_path):
    """ShardedAdamW(state_dtype="bf16") at gloo world 2 on CPU arenas: parameters bit-identical to the replicated bf16-state optimizer over three steps
    (the third an all-text step whose audio buckets are gated off), every launch goes to adamw16_step on a 16-byte aligned owned piece, state is
    1 / world plus tails in bf16 with no compact master, state_dict() consolidates to the replicated layout and loads back, the other mode's
    checkpoint is refused.  (The ownership map itself is covered at worlds 2 / 4 / 8 by tests/test_host_cpu.py and does not change.)"""
    script = tmp_path / "sharded16_worker.py"
    script.write_text(SHARDED16_WORKER)
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", PYTHONPATH=ROOT)
    env.pop("AFK_DP_FORM", None)
    env.pop("AFK_ADAMW_STATE", None)
    env["OMP_NUM_THREADS"] = "2"
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1",
           "--master-port", "29561", str(script), ROOT]
    r = subprocess.run(cmd, capture_output=True, text=True, env=env, timeout=900)
    assert r.returncode == 0 and r.stdout.count("OK") == 2, r.stdout[-2000:] + r.stderr[-3000:]

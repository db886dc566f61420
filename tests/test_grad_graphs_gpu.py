"""Gradients per tensor under gradient accumulation and multi-use autograd graphs (MI355X).

The gradient arena (arena.py) is filled by host-side bookkeeping, not by PyTorch's own accumulation: the `fresh` flag of a block (first write
after zero_grad() overwrites, later ones accumulate), the per-bucket write counters that hand a finished bucket to the overlapped optimizer or
the all-reduce, lm_head + loss parking its unscaled weight gradient in the arena during the forward, and the hand-over of column sums from an
encoder layer's LayerNorm backward to the fc2 bias of the layer below.  These tests hold every arena block, per element, to a plain reference:

  accumulation of n parts:  |acc - sum_i g_i| <= (n + 1) * 2^-8 * sum_i |g_i| + 2^-17 * max(sum_i |g_i|)
                            (g_i = the same micro-batch run alone, summed in fp32)

The kernels are bit-deterministic, so a contribution differs from its standalone value only by rounding: bf16 rounds to nearest with a relative
error of at most 2^-8, each of the n - 1 accumulating writes rounds the running sum once, each standalone part was rounded once, and the paths
that keep a bf16 partial (lm_head's private dW buffer, the column-sum hand-over row) round once more - (n + 1) * 2^-8 * sum |g_i| in all.
(2^-7 for every n, tried first, is exceeded by rounding alone on 0.1 % of the elements of some blocks with three parts.)  A dropped, doubled or
overwritten contribution breaks the bar on almost every element.  Multi-use graphs (two labelled forwards in one backward,
a loss beside a term on out.logits, a second consumer of an encoder stage's output, a partial backward) are also held to fp32 CPU autograd
through the oracle (tests/_tol.py GRAD_REL_L2 per tensor) and, under the overlapped optimizer, to the serial schedule bit for bit.
"""
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

from tests._tol import GRAD_REL_L2
from tests.test_model_gpu import ROOT, _fresh_model, _rel

BF = torch.bfloat16
ORACLE_CFG = dict(enc_heads=4, heads=4, kv_heads=2, eps=1e-6, theta=10000.0, audio_token_id=1023)
UNTOUCHED_ROWS = (1000, 1023)   # embed_tokens rows no micro-batch below reads (1023 is the audio placeholder: its rows are replaced by audio)


# ---------------------------------------------------------------------------------------------- inputs and references
def _micro_batches():
    """three micro-batches with disjoint vocabulary ranges: audio + text (two ragged windows), audio only (one short window, a few tokens
    around it), text only (two samples)"""
    g = torch.Generator().manual_seed(21)
    feats1 = (torch.randn(2, 128, 3000, generator=g) * 0.5).to(BF)
    fm1 = torch.ones(2, 3000, dtype=torch.int32)
    fm1[1, 1000:] = 0                                   # 750 + 250 audio tokens
    ids1 = torch.randint(0, 300, (1, 6 + 1000 + 16), generator=g)
    ids1[0, 6:1006] = 1023
    lab1 = torch.full_like(ids1, -100)
    lab1[:, -16:] = ids1[:, -16:]
    feats2 = (torch.randn(1, 128, 3000, generator=g) * 0.5).to(BF)
    fm2 = torch.zeros(1, 3000, dtype=torch.int32)
    fm2[0, :600] = 1                                    # 150 audio tokens
    ids2 = torch.randint(300, 600, (1, 2 + 150 + 4), generator=g)
    ids2[0, 2:152] = 1023
    lab2 = torch.full_like(ids2, -100)
    lab2[:, -4:] = ids2[:, -4:]
    ids3 = torch.randint(600, 1000, (2, 48), generator=g)
    return [dict(input_ids=ids1, input_features=feats1, input_features_mask=fm1, labels=lab1),
            dict(input_ids=ids2, input_features=feats2, input_features_mask=fm2, labels=lab2),
            dict(input_ids=ids3, labels=ids3.clone())]


SCALES = (0.3, 1.7, 0.6)


def _on(kw, dev):
    return {k: v.to(dev) for k, v in kw.items()}


def _snapshot(m):
    """every WRITTEN arena block as fp32 (blocks backward did not reach since zero_grad(): absent)"""
    m.arena.join_streams()
    torch.cuda.synchronize()
    return {k: b.grad.float().clone() for k, b in m.arena.blocks.items() if not b.fresh}


def _bar(ab, n):
    return (n + 1) * 2.0 ** -8 * ab + 2.0 ** -17 * float(ab.max())


def _check_sum(acc, parts, label):
    """the accumulation bar of the module doc, per element of every block; a block no part wrote must be unwritten in `acc` too"""
    bad = {}
    keys = set(acc) | {k for p in parts for k in p}
    for k in sorted(keys):
        ps = [p[k] for p in parts if k in p]
        if not ps:
            bad[k] = "written by the accumulated run only"
            continue
        if k not in acc:
            bad[k] = "not written by the accumulated run"
            continue
        s = torch.stack(ps).sum(0)
        ab = torch.stack([p.abs() for p in ps]).sum(0)
        err = (acc[k] - s).abs()
        n = int((err > _bar(ab, len(ps))).sum())
        if n:
            bad[k] = dict(n_over=n, of=err.numel(), rel_l2=float((acc[k] - s).norm() / s.norm().clamp_min(1e-30)),
                          worst_err_over_abs_sum=float((err / ab.clamp_min(1e-30)).max()))
    assert not bad, (label, bad)


def _check_bits(a, b, label, keys=None):
    bad = [k for k in (keys or sorted(set(a) | set(b))) if k not in a or k not in b or not torch.equal(a[k], b[k])]
    assert not bad, (label, bad)


def _standalone(m, mbs, scales, dev):
    out = []
    for kw, c in zip(mbs, scales):
        m.zero_grad()
        (c * m(**_on(kw, dev)).loss).backward()
        out.append(_snapshot(m))
    return out


def _oracle_grads(m, objective):
    """fp32 CPU autograd through oracle/af3_oracle.forward on the model's own (bf16-rounded) weights; objective(fwd) -> scalar, where
    fwd(**batch) returns the oracle's dict(loss, logits, audio)"""
    from oracle import af3_oracle as O

    leaves = {k: v.detach().float().cpu().requires_grad_(True) for k, v in m.state_dict().items()}

    def fwd(input_ids, input_features=None, input_features_mask=None, labels=None):
        return O.forward(leaves, ORACLE_CFG, input_ids, None if input_features is None else input_features.float(),
                         None if input_features_mask is None else input_features_mask.long(), labels=labels)

    objective(fwd).backward()
    return leaves


def _check_oracle(m, leaves, label):
    params = dict(m.named_parameters())
    bad, n = {}, 0
    for k, v in leaves.items():
        if v.grad is None or not params[k].requires_grad:
            continue
        n += 1
        r = _rel(params[k].grad, v.grad)
        if not r <= GRAD_REL_L2:
            bad[k] = r
    assert n >= 60 and not bad, (label, n, bad)


def _check_untouched_rows(m, label):
    g = m.arena["model.language_model.embed_tokens.weight"].grad
    lo, hi = UNTOUCHED_ROWS
    assert int(g[lo: hi + 1].float().abs().sum()) == 0 and not bool(g[lo: hi + 1].isnan().any()), (label, "embed_tokens rows nobody read moved")


def _set_forms(monkeypatch, fuse, form):
    import audio_flamingo_amd.functional as F

    monkeypatch.setattr(F, "FUSE_BIAS_SUMS", fuse)
    monkeypatch.setattr(F, "BWD_FORM", form)
    if form != "nt":
        # the transposed-operand kernels take every tiny shape (tests/test_ops_gpu.py: ragged TN / NN forms): let them serve every GEMM they can
        monkeypatch.setattr(F, "DIRECT_MIN_TILES", 1)


# ---------------------------------------------------------------------------------------------- A. accumulation, per tensor
@pytest.mark.parametrize("ckpt", [False, True], ids=["keep", "ckpt_full"])
@pytest.mark.parametrize("stream", [False, True], ids=["serial", "wgrad_stream"])
@pytest.mark.parametrize("form", ["nt", "wgrad_direct", "direct"])
@pytest.mark.parametrize("fuse", [False, True], ids=["colsum", "fused_bias"])
def test_accumulation_matches_sum_of_micro_batches(dev, monkeypatch, fuse, form, stream, ckpt):
    """zero_grad(), then three scaled micro-batches (audio + text, audio only, text only) accumulated in the arena == the same micro-batches
    run alone, summed in fp32 - per element of every block; embed_tokens rows nobody read stay exactly zero"""
    _set_forms(monkeypatch, fuse, form)
    m = _fresh_model(dev)
    if stream:
        m.arena.enable_wgrad_stream(True)
    if ckpt:
        m.gradient_checkpointing_enable()
    mbs = _micro_batches()
    parts = _standalone(m, mbs, SCALES, dev)
    m.zero_grad()
    for kw, c in zip(mbs, SCALES):
        (c * m(**_on(kw, dev)).loss).backward()
    acc = _snapshot(m)
    _check_sum(acc, parts, (fuse, form, stream, ckpt))
    _check_untouched_rows(m, (fuse, form, stream, ckpt))
    # the audio tower's sum must survive the text-only micro-batch: it is in `parts[0] + parts[1]` only, and the check above holds it there
    assert all(k in parts[0] for k in acc) and not any("audio_tower" in k for k in parts[2])


LOSS_CHUNK, LOSS_LABELLED = 128, 356
_CHUNK_ORACLE = {}


@pytest.mark.parametrize("form", ["nt", "wgrad_direct", "direct"])
def test_loss_head_chunk_loop_matches_oracle(dev, monkeypatch, form):
    """functional.LMHeadLossFn with its chunk loop running three times, the last chunk ragged (356 labelled rows in chunks of 128: 128, 128,
    100): the lm_head weight gradient accumulates across chunks, the label and row-loss slices follow the chunk.  One audio window plus text;
    every parameter gradient against fp32 autograd through the oracle, the loss within LOSS_ATOL"""
    import audio_flamingo_amd.functional as F
    from tests._tol import LOSS_ATOL

    _set_forms(monkeypatch, True, form)
    monkeypatch.setattr(F.LMHeadLossFn, "CHUNK", LOSS_CHUNK)
    g = torch.Generator().manual_seed(33)
    feats = (torch.randn(1, 128, 3000, generator=g) * 0.5).to(BF)
    fm = torch.zeros(1, 3000, dtype=torch.int32)
    fm[0, :600] = 1                                     # 150 audio tokens
    ids = torch.randint(0, 1000, (1, 2 + 150 + 360), generator=g)
    ids[0, 2:152] = 1023
    labels = torch.full_like(ids, -100)
    labels[:, -LOSS_LABELLED:] = ids[:, -LOSS_LABELLED:]
    kw = dict(input_ids=ids, input_features=feats, input_features_mask=fm, labels=labels)
    n_labelled = int((labels[:, 1:] != -100).sum())     # rows whose shifted label counts
    sizes = [min(LOSS_CHUNK, n_labelled - s) for s in range(0, n_labelled, LOSS_CHUNK)]
    assert n_labelled == LOSS_LABELLED and len(sizes) >= 3 and sizes[-1] < LOSS_CHUNK, (n_labelled, sizes)
    seen = []
    real = F.ops.ce_fwd_bwd_

    def spy(logits, *a, **k):
        seen.append(logits.shape[0])
        return real(logits, *a, **k)

    monkeypatch.setattr(F.ops, "ce_fwd_bwd_", spy)
    m = _fresh_model(dev)
    m.zero_grad()
    loss = m(**_on(kw, dev)).loss
    loss.backward()
    m.arena.join_streams()
    torch.cuda.synchronize()
    assert seen == sizes, (seen, sizes)
    if not _CHUNK_ORACLE:   # the same weights (seed) and batch for every form: one oracle run serves all three

        def objective(fwd):
            _CHUNK_ORACLE["loss"] = fwd(**kw)["loss"]
            return _CHUNK_ORACLE["loss"]

        _CHUNK_ORACLE["leaves"] = _oracle_grads(m, objective)
    got, want = float(loss.detach()), float(_CHUNK_ORACLE["loss"].detach())
    assert abs(got - want) <= LOSS_ATOL, (got, want)
    _check_oracle(m, _CHUNK_ORACLE["leaves"], ("loss head in chunks", form))


@pytest.mark.parametrize("last", [1, 2], ids=["audio_only_last", "text_only_last"])
def test_last_micro_step_under_backward_overlap_matches_serial(dev, last):
    """plain micro-steps, then the LAST one under BackwardOverlap + FusedAdamW (per-bucket AdamW inside backward): parameters bit-identical to
    serial accumulation followed by opt.step()"""
    from audio_flamingo_amd.arena import FusedAdamW
    from audio_flamingo_amd.dp import BackwardOverlap

    mbs = _micro_batches()
    order = [i for i in range(3) if i != last] + [last]
    ma, mb = _fresh_model(dev), _fresh_model(dev)
    oa, ob = FusedAdamW(ma.arena, lr=1e-3, weight_decay=0.01), FusedAdamW(mb.arena, lr=1e-3, weight_decay=0.01)
    mb.arena.enable_wgrad_stream(True)
    ov = BackwardOverlap(mb.arena, ob)
    for step in range(2):
        ma.zero_grad()
        for i in order:
            (SCALES[i] * ma(**_on(mbs[i], dev)).loss).backward()
        oa.step()
        mb.zero_grad()
        for i in order[:-1]:
            (SCALES[i] * mb(**_on(mbs[i], dev)).loss).backward()
        ov.begin_step()
        (SCALES[last] * mb(**_on(mbs[last], dev)).loss).backward()
        ov.finish()
        torch.cuda.synchronize()
        assert torch.equal(ma.arena.params, mb.arena.params), (step, "overlapped last micro-step differs from serial accumulation + step")


# ---------------------------------------------------------------------------------------------- C1 / C3. two labelled forwards, one backward
def _two_forwards(m, mbs, dev):
    return 0.3 * m(**_on(mbs[0], dev)).loss + 0.7 * m(**_on(mbs[2], dev)).loss


@pytest.mark.parametrize("stream", [False, True], ids=["serial", "wgrad_stream"])
def test_two_labelled_forwards_one_backward(dev, stream):
    """(0.3 m(A).loss + 0.7 m(B).loss).backward(): every block == the two micro-batches as separate backwards (accumulation bar), and == fp32
    autograd through the oracle per tensor"""
    mbs = _micro_batches()
    m = _fresh_model(dev)
    if stream:
        m.arena.enable_wgrad_stream(True)
    parts = _standalone(m, [mbs[0], mbs[2]], (0.3, 0.7), dev)
    m.zero_grad()
    _two_forwards(m, mbs, dev).backward()
    acc = _snapshot(m)
    _check_sum(acc, parts, "two forwards")
    _check_untouched_rows(m, "two forwards")
    leaves = _oracle_grads(m, lambda f: 0.3 * f(**mbs[0])["loss"] + 0.7 * f(**mbs[2])["loss"])
    _check_oracle(m, leaves, "two forwards vs oracle")


def test_two_labelled_forwards_under_backward_overlap(dev):
    """the same objective with the optimizer inside backward: a bucket must not be stepped before its second set of writes has landed"""
    from audio_flamingo_amd.arena import FusedAdamW
    from audio_flamingo_amd.dp import BackwardOverlap

    mbs = _micro_batches()
    ma, mb = _fresh_model(dev), _fresh_model(dev)
    oa, ob = FusedAdamW(ma.arena, lr=1e-3, weight_decay=0.01), FusedAdamW(mb.arena, lr=1e-3, weight_decay=0.01)
    ov = BackwardOverlap(mb.arena, ob)
    for step in range(2):
        ma.zero_grad()
        _two_forwards(ma, mbs, dev).backward()
        oa.step()
        mb.zero_grad()
        ov.begin_step()
        _two_forwards(mb, mbs, dev).backward()
        ov.finish()
        torch.cuda.synchronize()
        assert torch.equal(ma.arena.params, mb.arena.params), (step, "overlapped step differs from the serial one")


# ---------------------------------------------------------------------------------------------- C2. loss beside a term on out.logits
C_LOGITS = 0.5


def _loss_and_logits(m, kw, dev):
    out = m(**_on(kw, dev), return_logits=True)
    return out.loss + C_LOGITS * (out.logits.float() ** 2).mean()


def test_loss_and_logits_term_in_one_backward(dev):
    """out = m(..., labels, return_logits=True); (out.loss + c * mean(out.logits^2)).backward().  lm_head.weight receives the two heads'
    gradients from the same activations: it must equal the two terms as separate backwards (accumulation bar).  The trunk below the heads
    sees the bf16 sum of both upstream gradients, so there the separate runs are a rel-L2 reference only (2^-7); every tensor also against
    fp32 autograd through the oracle"""
    mbs = _micro_batches()
    kw = mbs[0]
    m = _fresh_model(dev)
    m.last_layer_rows_only = False          # the separate labelled run below computes the last layer on every row, as return_logits=True does
    m.zero_grad()
    m(**_on(kw, dev)).loss.backward()
    p_loss = _snapshot(m)
    m.zero_grad()
    nolab = {k: v for k, v in kw.items() if k != "labels"}
    (C_LOGITS * (m(**_on(nolab, dev)).logits.float() ** 2).mean()).backward()
    p_logits = _snapshot(m)
    m.zero_grad()
    _loss_and_logits(m, kw, dev).backward()
    acc = _snapshot(m)
    _check_sum({"lm_head.weight": acc["lm_head.weight"]}, [{"lm_head.weight": p["lm_head.weight"]} for p in (p_loss, p_logits)], "lm_head")
    assert set(acc) == set(p_loss) | set(p_logits)
    for k in acc:
        s = p_loss.get(k, 0) + p_logits.get(k, 0)
        assert float((acc[k] - s).norm()) <= 2.0 ** -7 * float(s.norm()) + 1e-30, (k, _rel(acc[k], s))
    leaves = _oracle_grads(m, lambda f: (lambda o: o["loss"] + C_LOGITS * (o["logits"] ** 2).mean())(f(**kw)))
    _check_oracle(m, leaves, "loss + logits term vs oracle")


def test_loss_and_logits_term_under_backward_overlap(dev):
    """the head bucket (final norm + lm_head) receives three writes in this backward: the overlapped optimizer must wait for all of them -
    parameters bit-identical to the serial step"""
    from audio_flamingo_amd.arena import FusedAdamW
    from audio_flamingo_amd.dp import BackwardOverlap

    kw = _micro_batches()[0]
    ma, mb = _fresh_model(dev), _fresh_model(dev)
    oa, ob = FusedAdamW(ma.arena, lr=1e-3, weight_decay=0.01), FusedAdamW(mb.arena, lr=1e-3, weight_decay=0.01)
    mb.arena.enable_wgrad_stream(True)
    ov = BackwardOverlap(mb.arena, ob)
    for step in range(2):
        ma.zero_grad()
        _loss_and_logits(ma, kw, dev).backward()
        oa.step()
        mb.zero_grad()
        ov.begin_step()
        _loss_and_logits(mb, kw, dev).backward()
        ov.finish()
        torch.cuda.synchronize()
        assert torch.equal(ma.arena.params, mb.arena.params), (step, "overlapped step differs from the serial one")


DP_WORKER = r'''
import os, sys, torch, torch.distributed as dist
sys.path.insert(0, sys.argv[1])
os.environ.setdefault("AFK_DP_COMM", "torch")
dist.init_process_group("gloo")
rank, world = dist.get_rank(), dist.get_world_size()
import tests.test_grad_graphs_gpu as T
from tests.test_model_gpu import _fresh_model
from audio_flamingo_amd.dp import BackwardOverlap, DataParallelEngine
dev = torch.device("cuda:0")
kw = T._micro_batches()[0]
m = _fresh_model(dev, seed=7 + rank)                 # replicas differ until the broadcast
eng = DataParallelEngine(m.arena, overlap=True, form="rs_ag")
eng.broadcast_parameters(0)
opt = eng.make_optimizer(lr=1e-3, weight_decay=0.01)
opt.sync_master()
ov = BackwardOverlap(m.arena, opt, eng)
m.arena.enable_wgrad_stream(True)
for step in range(2):
    m.zero_grad()
    ov.begin_step()
    T._loss_and_logits(m, kw, dev).backward()
    ov.finish()
    torch.cuda.synchronize()
torch.save(m.arena.params.cpu(), os.path.join(sys.argv[2], f"params{rank}.pt"))
dist.destroy_process_group()
'''


def test_loss_and_logits_term_data_parallel_overlap_gloo(dev, tmp_path):
    """two gloo ranks on one GPU, DataParallelEngine + BackwardOverlap (all-reduce and AdamW per bucket inside backward), the loss + logits
    objective on the same batch on both ranks: the averaged gradient (g + g) / 2 is g exactly, so both ranks must end bit-identical to each other
    AND to a single-process serial run of the same objective (a bucket exchanged before all its writes landed steps part of it with zeros)"""
    from audio_flamingo_amd.arena import FusedAdamW

    script = tmp_path / "worker.py"
    script.write_text(DP_WORKER)
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(29650 + os.getpid() % 200), WORLD_SIZE="2")
    procs = [subprocess.Popen([sys.executable, str(script), ROOT, str(tmp_path)], env=dict(env, RANK=str(r)), stdout=subprocess.PIPE,
                              stderr=subprocess.STDOUT) for r in range(2)]
    outs = []
    for p in procs:
        try:
            out, _ = p.communicate(timeout=300)
        except subprocess.TimeoutExpired:
            for q in procs:
                q.kill()
            raise
        outs.append(out.decode(errors="replace")[-3000:])
    assert all(p.returncode == 0 for p in procs), outs
    p0, p1 = (torch.load(tmp_path / f"params{r}.pt") for r in range(2))
    assert torch.equal(p0, p1), "ranks diverged"
    kw = _micro_batches()[0]
    m = _fresh_model(dev)
    opt = FusedAdamW(m.arena, lr=1e-3, weight_decay=0.01)
    for step in range(2):
        m.zero_grad()
        _loss_and_logits(m, kw, dev).backward()
        opt.step()
    torch.cuda.synchronize()
    ref = m.arena.params.cpu()
    assert torch.equal(p0, ref), ("data-parallel step differs from the serial one", float((p0.float() - ref.float()).abs().max()))


# ---------------------------------------------------------------------------------------------- C4 / C5. encoder stage output with two consumers
def _enc_setup(dev, seed=3):
    m = _fresh_model(dev, seed=seed)
    g = torch.Generator(device=dev).manual_seed(seed)
    with torch.no_grad():   # biases / norm weights off their trivial init so that every gradient path carries signal
        for blk in m.arena.order:
            if "audio_tower.layers" in blk.key and blk.key.endswith(".bias"):
                blk.data.copy_((0.02 * torch.randn(blk.shape, device=dev, generator=g)).to(BF))
            elif "audio_tower.layers" in blk.key and blk.key.endswith("norm.weight"):
                blk.data.copy_((1 + 0.05 * torch.randn(blk.shape, device=dev, generator=g)).to(BF))
        for i in range(2):
            m.arena[f"model.audio_tower.layers.{i}.self_attn.qkv.bias"].data[m.E: 2 * m.E].zero_()   # k_proj has no bias
    m.arena.step_counter += 1
    W, S = 2, 1500
    x0 = torch.randn(W * S, m.E, device=dev, generator=g).to(BF)
    r1 = torch.randn(W * S, m.E, device=dev, generator=g)
    r2 = torch.randn(W * S, m.E, device=dev, generator=g)
    return m, x0, r1, r2, W, S


def _enc(m, i, x, W, S):
    import audio_flamingo_amd.functional as F

    p = f"{m._at}layers.{i}."
    return F.EncoderLayerFn.apply(x, m._anchor(p + "fc1.weight"), m.arena, p, W, S, m.enc_heads, None)


def _enc_ref32(m, x, W, S):
    """fp32 torch restatement of two encoder layers (AudioFlamingo3EncoderLayer: pre-LN attention, pre-LN GELU MLP) on the arena's weights;
    -> (x1, y1, leaves by arena key)"""
    import torch.nn.functional as Fn

    E, H = m.E, m.enc_heads
    D = E // H
    P = {b.key: b.data.detach().float().requires_grad_(True) for b in m.arena.order if "audio_tower.layers." in b.key}
    outs = []
    for i in range(2):
        p = f"{m._at}layers.{i}."
        h = Fn.layer_norm(x, (E,), P[p + "self_attn_layer_norm.weight"], P[p + "self_attn_layer_norm.bias"])
        q, k, v = Fn.linear(h, P[p + "self_attn.qkv.weight"], P[p + "self_attn.qkv.bias"]).split(E, -1)
        q, k, v = (t.reshape(W, S, H, D).transpose(1, 2) for t in (q, k, v))
        o = Fn.scaled_dot_product_attention(q, k, v, scale=D ** -0.5).transpose(1, 2).reshape(W * S, E)
        x = x + Fn.linear(o, P[p + "self_attn.out_proj.weight"], P[p + "self_attn.out_proj.bias"])
        h = Fn.layer_norm(x, (E,), P[p + "final_layer_norm.weight"], P[p + "final_layer_norm.bias"])
        x = x + Fn.linear(Fn.gelu(Fn.linear(h, P[p + "fc1.weight"], P[p + "fc1.bias"])), P[p + "fc2.weight"], P[p + "fc2.bias"])
        outs.append(x)
    return outs[0], outs[1], P


def _enc_grads(m):
    m.arena.join_streams()
    torch.cuda.synchronize()
    return {b.key: b.grad.float().clone() for b in m.arena.order if "audio_tower.layers." in b.key}


@pytest.mark.parametrize("x1_term_first", [False, True], ids=["y1_term_first", "x1_term_first"])
def test_encoder_output_with_a_second_consumer(dev, monkeypatch, x1_term_first):
    """<y1, r1> + <x1, r2> with x1 = layer 0's output and y1 = layer 1(x1): autograd adds r2 into the gradient layer 1 hands down - possibly
    IN PLACE into that very tensor (same storage).  The fc2 bias of layer 0 must be the column sums of the SUM.  Against an fp32 torch encoder
    (GRAD_REL_L2 per tensor); FUSE_BIAS_SUMS 1 vs 0: every non-bias gradient bit-equal, the biases within the accumulation bar.  Both orders of
    building the two terms (the engine runs the later-built branch first, which decides which gradient the other is added into)"""
    import audio_flamingo_amd.functional as F

    got = {}
    for fuse in (False, True):
        monkeypatch.setattr(F, "FUSE_BIAS_SUMS", fuse)
        m, x0, r1, r2, W, S = _enc_setup(dev)
        m.zero_grad()
        xin = x0.clone().requires_grad_(True)
        x1 = _enc(m, 0, xin, W, S)
        if x1_term_first:
            t2 = (x1.float() * r2).sum()
            y1 = _enc(m, 1, x1, W, S)
            obj = t2 + (y1.float() * r1).sum()
        else:
            y1 = _enc(m, 1, x1, W, S)
            obj = (y1.float() * r1).sum() + (x1.float() * r2).sum()
        obj.backward()
        got[fuse] = _enc_grads(m)
        got[fuse]["x0"] = xin.grad.float().clone()
    xr = x0.float().requires_grad_(True)
    x1r, y1r, P = _enc_ref32(m, xr, W, S)
    ((y1r * r1).sum() + (x1r * r2).sum()).backward()
    ref = {k: v.grad for k, v in P.items()}
    ref["x0"] = xr.grad
    for fuse in (False, True):
        bad = {k: _rel(got[fuse][k], ref[k]) for k in ref if not _rel(got[fuse][k], ref[k]) <= GRAD_REL_L2}
        assert not bad, (fuse, "vs fp32 torch", bad)
    bias = [k for k in got[True] if k.endswith(".bias")]
    _check_bits(got[True], got[False], "fuse 1 vs 0, non-bias", [k for k in got[True] if k not in bias])
    for k in bias:
        _check_sum({k: got[True][k]}, [{k: got[False][k]}], ("fuse 1 vs 0", k))


@pytest.mark.parametrize("fuse", [False, True], ids=["colsum", "fused_bias"])
def test_encoder_partial_backward_leaves_no_stale_hand_over(dev, monkeypatch, fuse):
    """torch.autograd.grad(obj, inputs=x1) runs layer 1's backward only; a backward from x1 with another gradient - the returned tensor changed in
    place, or a new tensor the allocator may place at the same address - must give layer 0 the gradients of THAT upstream (a fresh forward +
    backward of layer 0 with the same upstream is the reference).  The hand-over slot is empty after zero_grad() and at the start of a forward"""
    import audio_flamingo_amd.functional as F

    monkeypatch.setattr(F, "FUSE_BIAS_SUMS", fuse)
    m, x0, r1, r2, W, S = _enc_setup(dev)
    a = m.arena
    l0 = [b.key for b in a.order if f"{m._at}layers.0." in b.key]
    for how in ("in_place", "new_tensor"):
        a.zero_grad()
        assert not a.presums
        xin = x0.clone().requires_grad_(True)
        x1 = _enc(m, 0, xin, W, S)
        y1 = _enc(m, 1, x1, W, S)
        (gx1,) = torch.autograd.grad((y1.float() * r1).sum(), inputs=x1)
        if how == "in_place":
            up = gx1.mul_(2.0)
        else:
            keep = (gx1.float() * 2.0 + 0.5).to(BF)
            del gx1
            up = torch.empty_like(keep)       # the allocator hands back the block gx1 just left, in the usual case
            up.copy_(keep)
        x1.backward(up)
        got = {k: v for k, v in _enc_grads(m).items() if k in l0}
        got["x0"] = xin.grad.float().clone()
        a.zero_grad()
        assert not a.presums, "zero_grad() left a hand-over slot"
        xr = x0.clone().requires_grad_(True)
        x1r = _enc(m, 0, xr, W, S)
        x1r.backward(up.clone())
        ref = {k: v for k, v in _enc_grads(m).items() if k in l0}
        ref["x0"] = xr.grad.float().clone()
        bias = [k for k in ref if k.endswith("fc2.bias")]
        _check_bits(got, ref, (how, "layer 0 after a partial backward"), [k for k in ref if k not in bias])
        for k in bias:
            _check_sum({k: got[k]}, [{k: ref[k]}], (how, k))
    # a forward starts with an empty slot
    a.zero_grad()
    xin = x0.clone().requires_grad_(True)
    x1 = _enc(m, 0, xin, W, S)
    torch.autograd.grad((_enc(m, 1, x1, W, S).float() * r1).sum(), inputs=x1)
    assert bool(a.presums) == fuse
    _enc(m, 0, x0.clone().requires_grad_(True), W, S)
    assert not a.presums, "a forward kept the hand-over slot of an earlier backward"


def test_every_announced_write_lands(dev):
    """after a full backward every bucket's expected-write counter is back at zero (the forward announced exactly the writes backward made)"""
    mbs = _micro_batches()
    m = _fresh_model(dev)
    m.zero_grad()
    _loss_and_logits(m, mbs[0], dev).backward()
    _two_forwards(m, mbs, dev).backward()
    assert list(m.arena._bucket_pending) == [0] * len(m.arena.bucket_names), m.arena._bucket_pending


# ---------------------------------------------------------------------------------------------- B. accumulation at full width
def test_accumulation_at_full_width(dev, monkeypatch):
    """bench.af3_7b_config with 2 encoder layers and 1 decoder layer, B = 2, S = 1024: two scaled micro-batches accumulated == the two run alone,
    per element of every block; the accumulating launches ran on the TN wgrad kernel, the split-K fold and the fused bias column sums (E = 1280)"""
    import bench
    from audio_flamingo_amd import functional as F
    from audio_flamingo_amd import ops
    from audio_flamingo_amd.modeling import AudioFlamingo3ForConditionalGeneration as Mine

    cfg = bench.af3_7b_config(enc_layers=2, dec_layers=1)
    m = Mine(cfg, device=dev, init_seed=3)
    g = torch.Generator(device=dev).manual_seed(4)
    with torch.no_grad():
        for blk in m.arena.order:
            if blk.key.endswith(".bias"):
                blk.data.copy_((0.02 * torch.randn(blk.shape, device=dev, generator=g)).to(BF))
            elif blk.key.endswith("norm.weight"):
                blk.data.copy_((1 + 0.05 * torch.randn(blk.shape, device=dev, generator=g)).to(BF))
        for i in range(2):
            m.arena[f"model.audio_tower.layers.{i}.self_attn.qkv.bias"].data[m.E: 2 * m.E].zero_()
    m.arena.step_counter += 1
    assert F.FUSE_BIAS_SUMS and F.BWD_FORM == "wgrad_direct"
    gen = torch.Generator().manual_seed(11)
    B, S = 2, 1024
    mbs = []
    for j in range(2):
        feats = (torch.randn(B, 128, 3000, generator=gen) * 0.5).to(BF)
        ids = torch.randint(0, 151643, (B, S), generator=gen)
        ids[:, 9: 9 + 750] = bench.AUDIO_ID
        labels = ids.clone()
        labels[:, : S - 256] = -100
        mbs.append(dict(input_ids=ids, input_features=feats, labels=labels))
    scales = (0.3, 1.7)
    calls = {"ln_colsum": 0}
    ln = ops.layernorm_bwd

    def counted(*a, **k):
        if k.get("colsum_out") is not None:
            calls["ln_colsum"] += 1
        return ln(*a, **k)

    monkeypatch.setattr(ops, "layernorm_bwd", counted)
    parts = []
    for kw, c in zip(mbs, scales):
        m.zero_grad()
        (c * m(**_on(kw, dev)).loss).backward()
        m.arena.join_streams()
        torch.cuda.synchronize()
        parts.append({k: b.grad.float().clone() for k, b in m.arena.blocks.items() if not b.fresh})
    m.zero_grad()
    (scales[0] * m(**_on(mbs[0], dev)).loss).backward()
    calls["ln_colsum"] = 0
    ops.kernel_counts(reset=True)
    (scales[1] * m(**_on(mbs[1], dev)).loss).backward()      # the accumulating backward
    m.arena.join_streams()
    torch.cuda.synchronize()
    cnt = ops.kernel_counts()
    assert cnt["gemm_tn256"] >= 6 and cnt["gemm_splitk"] >= 1, cnt
    assert calls["ln_colsum"] >= 2 * 2 - 1, calls       # out_proj bias in each layer + the hand-over to layer 0's fc2
    bad = {}
    for k, b in m.arena.blocks.items():
        assert not b.fresh, k
        acc = b.grad.float()
        s = parts[0][k] + parts[1][k]
        ab = parts[0][k].abs() + parts[1][k].abs()
        n = int(((acc - s).abs() > _bar(ab, 2)).sum())
        if n:
            bad[k] = n
        del acc, s, ab
    assert not bad, bad

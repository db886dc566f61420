"""GPU: generate(return_dict_in_generate=True, output_scores=True, output_logits=True) - the three kernels behind it (afk_decode_record,
afk_decode_sample_scored, afk_transition_scores) on synthetic rows, then generate() itself on the tiny64 goldens: every step form (the one-sequence chain greedy,
with processors and sampled; the batched step; the hook loop), eager, graph-replayed and hook-driven.

Bounds.  Copies, recorded rows and `logits / temperature` are compared bit for bit: all routes run the same launches on the same inputs.  Kept sets are exact on
steps whose decision margins exceed the floors of tests/test_warpers_gpu.py.  Normalised transition scores: 1e-5 x max(1, |value|) against an fp64 log_softmax
(a fixed-order fp32 sum of <= 2^20 positive terms is off by at most ~20 ulps relative, ~1.2e-6 in the log; expf and the subtraction add a few ulps: a factor ~5 of
headroom).  Against the live fp32 reference: tests/_tol.py floor_bar(logit_tol(|ref row|max), [the reference's own bf16 deviation at that step])."""
import json
import os

import numpy as np
import pytest
import torch

from tests import _logits_process_ref as P
from tests import _sampler_ref as R
from tests import _tol
from tests import _warpers_ref as W

pytestmark = pytest.mark.gpu

FLAGS = dict(return_dict_in_generate=True, output_scores=True, output_logits=True)
NEW = 12
NINF_BITS = -8388608                       # 0xff800000 as int32
SENTINEL_BITS = 0x7FA55A5A                 # a signalling-NaN pattern no kernel here produces
FILTERS = ("min_p", "typical_p", "epsilon_cutoff", "eta_cutoff")
HALF_GAP = 5e-5
FLOORS = dict(top_p=HALF_GAP, min_p=W.REL_GAP, typical_mass=W.MASS_GAP, typical_d=W.D_GAP, epsilon=W.REL_GAP, eta=W.REL_GAP)   # test_warpers_gpu.py's
_CACHE = {}


def bits(x):
    return x.contiguous().view(torch.int32)


def _div(x, T):
    """x / T as one IEEE fp32 division per element on x's device - what the kernel's `logits / temperature` and the reference's warper on the host compute.  (A
    device tensor divided by a Python scalar is multiplied by the rounded reciprocal instead, which is off by one ulp on about a third of the values.)"""
    return x / torch.full_like(x, T)


def _sentinel(shape, dev):
    return torch.full(shape, SENTINEL_BITS, dtype=torch.int32, device=dev).view(torch.float32)


# ---------------------------------------------------------------------------------------------- 1. afk_decode_record
@pytest.mark.parametrize("same_alignment", [False, True], ids=["src-misaligned", "src-aligned-like-dst"])
@pytest.mark.parametrize("V", [1000, 1003, 5, 9001])
def test_decode_record_copies_bits_into_the_slot_the_device_counter_names(dev, V, same_alignment):
    """ld_dst is odd, so rows 1 and 2 of every slot start off a 16-byte boundary (scalar head, 16-byte body, scalar tail); the source rows either share that
    alignment (16-byte loads) or do not (word loads); V = 9001 takes three column chunks per row, V = 5 has no 16-byte body in some rows"""
    from audio_flamingo_amd import ops

    B, n_steps = 3, 4
    ld_dst = V + (1 if V % 4 in (0, 2) else 2)
    assert ld_dst % 4 in (1, 3)
    if same_alignment:
        ld_src, step_stride = ld_dst, (B * ld_dst + 3) // 4 * 4 + 4
    else:
        ld_src, step_stride = V + 7 - (1 if (V + 7 - ld_dst) % 4 == 0 else 0), B * ld_dst + 2
        assert (ld_src - ld_dst) % 4 != 0
    g = torch.Generator().manual_seed(V)
    src_buf = torch.randn((B, ld_src), generator=g)
    special = torch.tensor([0x7FC12345, -2147483648, 0x7F800000, NINF_BITS, 0x7F800001], dtype=torch.int32).view(torch.float32)   # NaN + payload, -0.0, +inf, -inf, sNaN
    for b in range(B):
        src_buf[b, torch.arange(special.numel()) * 7 % V] = special[: V] if V < special.numel() else special
    src = src_buf.to(dev)[:, :V]
    counter = torch.tensor([5], dtype=torch.int32, device=dev)
    for t in (0, 2, 3, -1, n_steps):
        flat = _sentinel((n_steps * step_stride + 8,), dev)
        dst = torch.as_strided(flat, (n_steps, B, V), (step_stride, ld_dst, 1))
        ops.decode_record(src, dst, step_base=counter, step_off=t - 5)
        want = _sentinel((n_steps * step_stride + 8,), dev)
        if 0 <= t < n_steps:
            torch.as_strided(want, (n_steps, B, V), (step_stride, ld_dst, 1))[t] = src
            assert torch.equal(bits(dst[t]), bits(src)), (V, t)
        assert torch.equal(bits(flat), bits(want)), (V, t, "a word outside slot t's rows was written" if 0 <= t < n_steps else "a step outside the buffer wrote")
    flat = _sentinel((n_steps * step_stride,), dev)                       # the host knows t: no counter
    dst = torch.as_strided(flat, (n_steps, B, V), (step_stride, ld_dst, 1))
    ops.decode_record(src, dst, step_off=1)
    assert torch.equal(bits(dst[1]), bits(src)) and bool((bits(dst[0]) == SENTINEL_BITS).all()) and bool((bits(dst[2:]) == SENTINEL_BITS).all())


def test_decode_record_refuses_bad_arguments(dev):
    from audio_flamingo_amd import ops
    from audio_flamingo_amd._lib import AfkError

    src, dst = torch.zeros((2, 40), device=dev), torch.zeros((3, 2, 40), device=dev)
    for bad in (dict(step_off=3), dict(step_off=-1), dict(n_steps=4), dict(n_steps=0), dict(step_base=torch.zeros(1, device=dev, dtype=torch.int64))):
        with pytest.raises(AfkError):
            ops.decode_record(src, dst, **bad)
    for s, d in ((src.double(), dst), (src, dst.double()), (src[:, :39], dst), (src, dst[:, :1]), (src.t().contiguous().t(), dst), (src.cpu(), dst)):
        with pytest.raises(AfkError):
            ops.decode_record(s, d)
    ops.decode_record(src + 1.0, dst, step_off=2, n_steps=3)
    assert bool((dst[2] == 1.0).all()) and not dst[:2].any()


# ---------------------------------------------------------------------------------------------- 2. decode_sample(scores_out=...)
SCORED_COMBOS = [("top-k/top-p", 20, 0.95, {}), ("min_p", 20, 0.95, dict(min_p=0.05)), ("typical_p+eta", 20, 0.95, dict(typical_p=0.6, eta_cutoff=0.01)),
                 ("all four", 50, 0.9, dict(min_p=0.05, typical_p=0.9, epsilon_cutoff=3e-4, eta_cutoff=3e-4))]


def _snapped(x_row, T, k, p, targets):
    """-> (the restatement's result, keywords of ops.decode_sample, every gap met): the parameters moved into gaps of the row's own statistics"""
    row = R.Row(x_row, T)
    top_p, half = (1.0, np.inf) if p >= 1.0 else row.snap_top_p(k, p)
    chain, kw, ok = W.snap_chain(row, k, top_p, targets)
    return chain.result(), dict(kw, temperature=T, top_k=k, top_p=top_p), bool(ok and half >= HALF_GAP)


@pytest.mark.parametrize("name,k,p,targets", SCORED_COMBOS, ids=[c[0] for c in SCORED_COMBOS])
@pytest.mark.parametrize("T", [1.0, 1.5])
def test_scored_sampler_leaves_the_warped_row_in_one_slot(dev, T, name, k, p, targets):
    from audio_flamingo_amd import ops

    V, B = 1000, 2
    x = torch.stack([R.bf16_logits(V, 4.0, seed=31 + b) for b in range(B)])
    xd = x.to(dev)
    z = _div(xd, T) if T != 1.0 else xd                                      # the fp32 division, on the device
    u = torch.tensor([0.37, 0.81], device=dev)
    counter = torch.tensor([7], dtype=torch.int32, device=dev)
    for b in range(B):                                                       # the parameters are snapped per row: one launch of both rows per row's values
        ref, kw, ok = _snapped(x[b], T, k, p, targets)
        assert ok, (name, T, b, ref["margins"])
        plain = ops.decode_sample(xd, u=u, **kw)
        plain_seeded = ops.decode_sample(xd, seed=0xFEED, step_base=counter, step_off=-6, **kw)
        scores, probs, kept = _sentinel((3, B, V), dev), torch.full((B, V), -1.0, device=dev), torch.full((B,), -1, device=dev, dtype=torch.int32)
        tok = ops.decode_sample(xd, u=u, probs_out=probs, kept_out=kept, scores_out=scores, step_base=counter, step_off=-6, **kw)
        assert torch.equal(tok, plain), (name, T, b)
        s2 = _sentinel((3, B, V), dev)
        assert torch.equal(ops.decode_sample(xd, seed=0xFEED, step_base=counter, step_off=-6, scores_out=s2, **kw), plain_seeded)
        assert torch.equal(bits(s2), bits(scores))
        assert bool((bits(scores[0]) == SENTINEL_BITS).all()) and bool((bits(scores[2]) == SENTINEL_BITS).all()), "a slot other than t = 1 was written"
        row = scores[1, b]
        fin = torch.isfinite(row)
        keep = torch.from_numpy(ref["keep"]).to(dev)
        assert torch.equal(fin, keep) and torch.equal(fin, probs[b] > 0) and int(fin.sum()) == int(kept[b]), (name, T, b, int(fin.sum()), int(keep.sum()), int(kept[b]))
        assert torch.equal(bits(row[fin]), bits(z[b][fin])), (name, T, b)
        assert bool((bits(row[~fin]) == NINF_BITS).all()), (name, T, b)
        assert bool(fin[tok[b]])


def test_scored_sampler_degenerate_rows_and_steps_outside_the_buffer(dev):
    from audio_flamingo_amd import ops
    from audio_flamingo_amd._lib import AfkError

    V = 1000
    y = R.bf16_logits(V, 4.0, seed=6)
    y[613] = float("inf")
    y[800] = float("inf")
    w = torch.full((V,), float("-inf"))
    w[3::5] = float("nan")
    x = torch.stack([y, w]).to(dev)
    for kw in (dict(), dict(temperature=1.5, top_k=20, top_p=0.9, min_p=0.05, typical_p=0.6, epsilon_cutoff=3e-4, eta_cutoff=3e-4)):
        scores, probs = _sentinel((3, 2, V), dev), torch.full((2, V), -1.0, device=dev)
        tok = ops.decode_sample(x, u=torch.tensor([0.3, 0.9], device=dev), scores_out=scores, probs_out=probs, step_off=2, **kw)
        assert tok.tolist() == [613, 0] and torch.equal(tok, ops.decode_sample(x, u=torch.tensor([0.3, 0.9], device=dev), **kw))
        assert torch.equal(torch.isfinite(scores[2]) | (scores[2] == float("inf")), probs > 0)     # exactly where the draw has positive probability
        assert float(scores[2, 0, 613]) == float("inf") and int((bits(scores[2, 0]) == NINF_BITS).sum()) == V - 1
        assert bool((bits(scores[2, 1]) == NINF_BITS).all())
        assert bool((bits(scores[:2]) == SENTINEL_BITS).all())
    # a counter that runs past the buffer (a graph replayed once too often) draws as ever and writes no score
    good = R.bf16_logits(V, 4.0, seed=8)[None].to(dev)
    for t in (-1, 3):
        scores = _sentinel((3, 1, V), dev)
        counter = torch.tensor([t + 9], dtype=torch.int32, device=dev)
        tok = ops.decode_sample(good, seed=5, top_k=20, step_base=counter, step_off=-9, scores_out=scores)
        assert torch.equal(tok, ops.decode_sample(good, seed=5, top_k=20, step_base=counter, step_off=-9)) and bool((bits(scores) == SENTINEL_BITS).all())
    for bad in (dict(scores_out=torch.zeros((3, 1, V + 1), device=dev)), dict(scores_out=torch.zeros((3, 1, V), device=dev), n_steps=4), dict(n_steps=2),
                dict(scores_out=torch.zeros((3, 1, V), device=dev, dtype=torch.float64))):
        with pytest.raises(AfkError):
            ops.decode_sample(good, **bad)


# ---------------------------------------------------------------------------------------------- 3. afk_transition_scores
def _sparse_scores(T, B, V, ld, seed):
    """[T, B, V] fp32 rows of which ~95 % are -inf, inside a buffer of row pitch ld; tokens [B, T]: finite entries but one, which sits on a -inf"""
    g = torch.Generator().manual_seed(seed)
    s = torch.randn((T, B, ld), generator=g) * 4.0
    s[torch.rand((T, B, ld), generator=g) < 0.95] = float("-inf")
    s = s[:, :, :V]
    tokens = torch.zeros((B, T), dtype=torch.int64)
    for t in range(T):
        for b in range(B):
            ids = torch.nonzero(torch.isfinite(s[t, b]))[:, 0]
            assert ids.numel() >= 8
            tokens[b, t] = ids[int(torch.randint(0, ids.numel(), (1,), generator=g))]
    tokens[1, 2] = int(torch.nonzero(torch.isinf(s[2, 1]))[0, 0])
    return s, tokens


@pytest.mark.parametrize("V", [1000, 1003])
def test_transition_scores_gather_and_log_softmax(dev, V):
    from types import SimpleNamespace

    from transformers.generation.utils import GenerationMixin

    from audio_flamingo_amd import ops
    from audio_flamingo_amd._lib import AfkError

    T, B = 3, 2
    s, tokens = _sparse_scores(T, B, V, V + 5, seed=V)
    sd, td = torch.zeros((T, B, V + 5), device=dev)[:, :, :V], tokens.to(dev)
    sd.copy_(s)
    assert sd.stride() == (B * (V + 5), V + 5, 1)
    gathered = torch.stack([s[t, torch.arange(B), tokens[:, t]] for t in range(T)], 1)
    raw = ops.transition_scores(sd, td, normalize=False)
    assert raw.shape == (B, T) and torch.equal(bits(raw.cpu()), bits(gathered))
    want = torch.stack([torch.log_softmax(s[t].double(), -1)[torch.arange(B), tokens[:, t]] for t in range(T)], 1)
    got = ops.transition_scores(sd, td, normalize=True).cpu().double()
    seqs = torch.cat([torch.zeros((B, 4), dtype=torch.int64), tokens], 1)
    fake = SimpleNamespace(config=SimpleNamespace(get_text_config=lambda: SimpleNamespace(vocab_size=V)))
    ref_raw = GenerationMixin.compute_transition_scores(fake, seqs, tuple(s[t].contiguous() for t in range(T)), normalize_logits=False)
    ref_norm = GenerationMixin.compute_transition_scores(fake, seqs, tuple(s[t].contiguous() for t in range(T)), normalize_logits=True).double()
    assert torch.equal(bits(raw.cpu()), bits(ref_raw))
    for name, ref in (("fp64 log_softmax", want), ("the reference's compute_transition_scores", ref_norm)):
        inf = torch.isinf(ref)
        assert inf.sum() == 1 and torch.equal(inf, torch.isinf(got)) and torch.equal(got[inf], ref[inf]), name
        err = ((got - ref).abs() / ref.abs().clamp_min(1.0))[~inf]
        print(V, name, "max err / max(1, |v|)", float(err.max()))
        assert float(err.max()) <= 1e-5, (name, float(err.max()))
    # a row with no finite entry: NaN under normalize, as log_softmax answers; -inf gathered as it stands without
    empty = torch.full((1, 1, V), float("-inf"), device=dev)
    tok0 = torch.zeros((1, 1), dtype=torch.int64, device=dev)
    assert bool(torch.isnan(ops.transition_scores(empty, tok0, normalize=True)).all()) and float(ops.transition_scores(empty, tok0)[0, 0]) == float("-inf")
    for bad_tok in (V, -1):
        with pytest.raises(AfkError, match="vocabulary"):
            ops.transition_scores(sd, torch.full_like(td, bad_tok))


# ---------------------------------------------------------------------------------------------- generate()
BASE = dict(do_sample=True, temperature=1.5, top_k=20, top_p=0.95, seed=0xFEED_0000_0007, max_new_tokens=NEW)    # test_warpers_gpu.py's
WARPS = (dict(), dict(min_p=0.05), dict(typical_p=0.6, eta_cutoff=0.01))
A_, C_ = 144, 165                          # tokens 3 and 5 of the golden greedy continuation of case A (test_decode_process_gpu.py)
PROC = dict(repetition_penalty=1.3, no_repeat_ngram_size=2, suppress_tokens=[A_], min_new_tokens=3, eos_token_id=C_)


class _Collect:
    def put(self, v):
        pass

    def end(self):
        pass


class _Recorder:
    """a logits processor that clones what it is handed: the only route to the per-step rows before generate() had output flags"""

    def __init__(self):
        self.rows = []

    def __call__(self, input_ids, scores):
        self.rows.append(scores.detach().clone())
        return scores


def _case_a(dev):
    if "case_a" not in _CACHE:
        from tests.test_model_gpu import G, _gen_prompt, _model

        g = torch.load(os.path.join(G, "tiny64_caseA.pt"))
        _CACHE["case_a"] = (_model(dev), _gen_prompt(g).to(dev), dict(input_features=g["feats"][:1].to(dev), input_features_mask=g["fmask"][:1].to(dev)), g)
    return _CACHE["case_a"][:3]


def _padded_batch(dev):
    """test_warpers_gpu.py:283-289"""
    g = torch.Generator().manual_seed(3)
    lens = (40, 23, 31)
    ids, att = torch.zeros((3, 40), dtype=torch.long), torch.zeros((3, 40), dtype=torch.long)
    for i, n in enumerate(lens):
        ids[i, 40 - n:] = torch.randint(0, 256, (n,), generator=g)
        att[i, 40 - n:] = 1
    return ids.to(dev), att.to(dev)


def _three_routes(m, p, **kw):
    """-> the flagged runs [eager, graph-replayed, hook-driven (a streamer)]"""
    return [m.generate(p, use_graph=False, **FLAGS, **kw), m.generate(p, use_graph=True, **FLAGS, **kw), m.generate(p, streamer=_Collect(), **FLAGS, **kw)]


def _greedy_runs(dev):
    """run 4 of the module: greedy, one sequence, no processor - shared by the tests that compare against it"""
    if "greedy" not in _CACHE:
        m, p, audio = _case_a(dev)
        _CACHE["greedy"] = (m.generate(p, max_new_tokens=NEW, **audio), _three_routes(m, p, max_new_tokens=NEW, **audio))
    return _CACHE["greedy"]


def _same_rows(a, b, n=None):
    n = min(len(a), len(b)) if n is None else n
    return all(torch.equal(bits(a[i]), bits(b[i])) for i in range(n))


def _check_shape(out, plain, S0, B, V):
    from audio_flamingo_amd.generation_output import AfkGenerateOutput

    assert isinstance(out, AfkGenerateOutput) and torch.equal(out.sequences, plain)
    n = out.sequences.shape[1] - S0
    for tup in (out.scores, out.logits):
        assert isinstance(tup, tuple) and len(tup) == n and all(r.shape == (B, V) and r.dtype == torch.float32 for r in tup)
    return n


def test_greedy_one_sequence_eager_graph_and_hooks(dev):
    from transformers import LogitsProcessorList

    m, p, audio = _case_a(dev)
    S0, V = p.shape[1], m.V
    plain, runs = _greedy_runs(dev)
    for out in runs:
        assert _check_shape(out, plain, S0, 1, V) == NEW
        for t in range(NEW):
            assert torch.equal(bits(out.scores[t]), bits(out.logits[t])), "no processor: scores are the logits"
            assert int(out.logits[t].argmax(-1)) == int(out.sequences[0, S0 + t]), t
    assert _same_rows(runs[0].logits, runs[1].logits, NEW) and _same_rows(runs[0].logits, runs[2].logits, NEW)
    rec = _Recorder()
    assert torch.equal(m.generate(p, max_new_tokens=NEW, logits_processor=LogitsProcessorList([rec]), **audio), plain)
    assert len(rec.rows) == NEW and _same_rows(runs[1].logits, rec.rows, NEW), "the recorded rows are not what a recording logits_processor sees"
    # the views share one buffer, which compute_transition_scores reads in place; un-normalised it is a gather
    from audio_flamingo_amd.generation_output import step_buffer_view

    out = runs[1]
    assert step_buffer_view(out.logits) is not None
    ts = m.compute_transition_scores(out.sequences, out.scores)
    assert ts.shape == (1, NEW) and torch.equal(bits(ts[0]), bits(torch.stack([out.scores[t][0, out.sequences[0, S0 + t]] for t in range(NEW)])))
    stacked = m.compute_transition_scores(out.sequences.cpu(), tuple(r.cpu().clone() for r in out.scores), normalize_logits=True)    # not views of one buffer
    assert torch.equal(bits(stacked), bits(m.compute_transition_scores(out.sequences, out.scores, normalize_logits=True)))
    want = torch.stack([torch.log_softmax(out.scores[t].double(), -1)[0, out.sequences[0, S0 + t]] for t in range(NEW)])
    assert float(((stacked[0].double() - want).abs() / want.abs().clamp_min(1.0)).max()) <= 1e-5
    # one flag alone
    only = m.generate(p, max_new_tokens=NEW, return_dict_in_generate=True, output_scores=True, **audio)
    assert only.logits is None and list(only.keys()) == ["sequences", "scores", "past_key_values"] and _same_rows(only.scores, out.scores, NEW)
    only = m.generate(p, max_new_tokens=NEW, return_dict_in_generate=True, output_logits=True, **audio)
    assert only.scores is None and _same_rows(only.logits, out.logits, NEW)
    bare = m.generate(p, max_new_tokens=NEW, return_dict_in_generate=True, **audio)
    assert bare.scores is None and bare.logits is None and torch.equal(bare.sequences, plain)
    assert torch.equal(m.generate(p, max_new_tokens=NEW, output_scores=True, output_logits=True, **audio), plain), "without return_dict_in_generate: the plain tensor"


def test_generation_config_switches_the_output_object_on(dev):
    from types import SimpleNamespace

    m, p, audio = _case_a(dev)
    plain, runs = _greedy_runs(dev)
    out = m.generate(p, max_new_tokens=NEW, generation_config=SimpleNamespace(return_dict_in_generate=True, output_logits=True), **audio)
    assert torch.equal(out.sequences, plain) and out.scores is None and _same_rows(out.logits, runs[1].logits, NEW)
    assert torch.equal(m.generate(p, max_new_tokens=NEW, return_dict_in_generate=False, generation_config=SimpleNamespace(return_dict_in_generate=True), **audio), plain)


def _judged_until(seq_row, S0, eos):
    """steps that can be judged: up to and including the row's first EOS (behind it the fed token is not the one in `sequences`)"""
    new = seq_row[S0:].tolist()
    return new.index(eos) + 1 if eos in new else len(new)


def test_greedy_with_processors_scores_are_the_processed_rows(dev):
    m, p, audio = _case_a(dev)
    S0, V = p.shape[1], m.V
    plain = m.generate(p, max_new_tokens=NEW, **PROC, **audio)
    runs = _three_routes(m, p, max_new_tokens=NEW, **PROC, **audio)
    base = _greedy_runs(dev)[1][1]
    n = _check_shape(runs[0], plain, S0, 1, V)
    assert _check_shape(runs[1], plain, S0, 1, V) == n
    nj = _judged_until(runs[0].sequences[0], S0, C_)
    hook_n = runs[2].sequences.shape[1] - S0            # the hook loop stops at the EOS itself; the device loops look for it every eighth step
    assert nj >= 4 and hook_n >= nj and torch.equal(runs[2].sequences[:, : S0 + nj], plain[:, : S0 + nj]) and len(runs[2].scores) == len(runs[2].logits) == hook_n
    print("processors: new tokens", plain[0, S0:].tolist(), "judged steps", nj)
    for a in ("scores", "logits"):
        assert _same_rows(getattr(runs[0], a), getattr(runs[1], a), nj) and _same_rows(getattr(runs[0], a), getattr(runs[2], a), nj), a
    out = runs[1]
    agree = 0
    for t in range(nj):
        seq = out.sequences[:, : S0 + t].cpu()
        want = P.reference_chain(out.logits[t].cpu(), seq, S0, penalty=1.3, ngram=2, suppress=(A_,), eos=(C_,), min_new_tokens=3)
        assert torch.equal(bits(out.scores[t].cpu()), bits(want)), t
        assert int(out.scores[t].argmax(-1)) == int(out.sequences[0, S0 + t])
        assert float(out.scores[t][0, A_]) == float("-inf") and (t >= 3 or float(out.scores[t][0, C_]) == float("-inf"))
        if torch.equal(out.sequences[:, : S0 + t], base.sequences[:, : S0 + t]):   # the same history so far: the raw row is the unprocessed run's
            assert torch.equal(bits(out.logits[t]), bits(base.logits[t])), t
            agree += 1
    assert agree >= 1 and not _same_rows(out.scores, out.logits, nj), "the processors changed nothing"


def _check_sampled_rows(out, S0, kw, rows):
    """per row and step: finite support of scores == the restatement's kept set on logits, finite values == logits / temperature, the drawn id is finite.
    -> (judged, skipped)"""
    T = kw["temperature"]
    params = [kw.get(f, d) for f, d in zip(FILTERS, (0.0, 1.0, 0.0, 0.0))]
    judged = skipped = 0
    for t in range(len(out.scores)):
        z = _div(out.logits[t], T)
        for b in rows:
            assert bool(torch.isfinite(out.scores[t][b, out.sequences[b, S0 + t]])), (t, b)
            ref = W.reference(out.logits[t][b].cpu(), T, kw["top_k"], kw["top_p"], *params)
            if any(v < FLOORS[n] for n, v in ref["margins"].items()):
                skipped += 1
                continue
            judged += 1
            fin = torch.isfinite(out.scores[t][b])
            assert torch.equal(fin.cpu(), torch.from_numpy(ref["keep"])), (t, b, int(fin.sum()), int(ref["keep"].sum()))
            assert torch.equal(bits(out.scores[t][b][fin]), bits(z[b][fin])) and bool((bits(out.scores[t][b][~fin]) == NINF_BITS).all()), (t, b)
    return judged, skipped


@pytest.mark.parametrize("warp", WARPS, ids=lambda w: "+".join(w) or "base")
def test_sampled_one_sequence_scores_are_the_warped_rows(dev, monkeypatch, warp):
    m, p, audio = _case_a(dev)
    S0, V = p.shape[1], m.V
    kw = dict(BASE, **warp)
    plain = m.generate(p, **audio, **kw)

    def refuse(*a, **k):
        raise AssertionError("token selection went through torch")

    captured = []
    real = torch.cuda.graph

    class Counting(real):
        def __init__(self, *a, **k):
            captured.append(1)
            super().__init__(*a, **k)

    with monkeypatch.context() as mp:
        for owner in (torch, torch.Tensor):
            mp.setattr(owner, "multinomial", refuse)
            mp.setattr(owner, "sort", refuse)
        mp.setattr(torch.cuda, "graph", Counting)
        out = m.generate(p, **FLAGS, **audio, **kw)
    assert len(captured) == 1
    assert _check_shape(out, plain, S0, 1, V) == NEW
    judged, skipped = _check_sampled_rows(out, S0, kw, [0])
    print("sampled", warp, "judged", judged, "skipped", skipped)
    assert skipped <= NEW // 3, (judged, skipped)
    eager, hooked = m.generate(p, use_graph=False, **FLAGS, **audio, **kw), m.generate(p, streamer=_Collect(), **FLAGS, **audio, **kw)
    for o in (eager, hooked):
        assert torch.equal(o.sequences, plain) and _same_rows(o.scores, out.scores, NEW) and _same_rows(o.logits, out.logits, NEW)
    assert _same_rows(out.logits, _greedy_runs(dev)[1][1].logits, 1), "token 0: the raw row does not depend on how the token is selected"


def test_sampled_with_processors_scores_hold_both(dev):
    """the built-in processors run in front of the sampler: their -inf bans are in `scores` and not in `logits`"""
    m, p, audio = _case_a(dev)
    S0 = p.shape[1]
    kw = dict(BASE, suppress_tokens=[A_], repetition_penalty=1.3)
    plain = m.generate(p, **audio, **kw)
    runs = _three_routes(m, p, **audio, **kw)
    for o in runs:
        assert torch.equal(o.sequences, plain) and _same_rows(o.scores, runs[0].scores, NEW) and _same_rows(o.logits, runs[0].logits, NEW)
    out = runs[1]
    for t in range(NEW):
        processed = P.reference_chain(out.logits[t].cpu(), out.sequences[:, : S0 + t].cpu(), S0, penalty=1.3, suppress=(A_,)).to(dev)
        fin = torch.isfinite(out.scores[t])
        assert torch.equal(bits(out.scores[t][fin]), bits(_div(processed, 1.5)[fin])) and not bool(fin[0, A_]) and bool(torch.isfinite(out.logits[t][0, A_]))
        assert bool(fin[0, out.sequences[0, S0 + t]]) and 1 <= int(fin.sum()) <= 20 + 8


@pytest.mark.parametrize("mode", ["greedy", "sampled"])
def test_left_padded_batch_of_three_takes_the_batched_step(dev, mode):
    from transformers import LogitsProcessorList

    m, _, _ = _case_a(dev)
    ids, att = _padded_batch(dev)
    S0, V = 40, m.V
    kw = dict(BASE, min_p=0.05) if mode == "sampled" else dict(max_new_tokens=NEW)
    plain = m.generate(ids, attention_mask=att, **kw)
    runs = _three_routes(m, ids, attention_mask=att, **kw)
    for o in runs:
        assert _check_shape(o, plain, S0, 3, V) == NEW
        assert _same_rows(o.scores, runs[0].scores, NEW) and _same_rows(o.logits, runs[0].logits, NEW)
    out = runs[1]
    rec = _Recorder()
    assert torch.equal(m.generate(ids, attention_mask=att, logits_processor=LogitsProcessorList([rec]), **kw), plain)
    assert len(rec.rows) == NEW and _same_rows(out.logits, rec.rows, NEW)
    if mode == "greedy":
        for t in range(NEW):
            assert torch.equal(bits(out.scores[t]), bits(out.logits[t])) and torch.equal(out.logits[t].argmax(-1), out.sequences[:, S0 + t]), t
        ts = m.compute_transition_scores(out.sequences, out.scores, normalize_logits=True)
        want = torch.stack([torch.log_softmax(out.scores[t].double(), -1).gather(1, out.sequences[:, S0 + t: S0 + t + 1])[:, 0] for t in range(NEW)], 1)
        assert ts.shape == (3, NEW) and float(((ts.double() - want).abs() / want.abs().clamp_min(1.0)).max()) <= 1e-5
    else:
        for b in range(3):                                                  # the cap on unjudged steps holds for every row on its own
            judged, skipped = _check_sampled_rows(out, S0, kw, [b])
            print("sampled batch: row", b, "judged", judged, "skipped", skipped)
            assert skipped <= NEW // 3, (b, judged, skipped)


def test_eos_lengths_follow_the_plain_call(dev):
    m, p, audio = _case_a(dev)
    S0, V = p.shape[1], m.V
    base = _greedy_runs(dev)[1][1]
    eos = int(base.sequences[0, S0 + 6])                                   # the 7th greedy token of case A
    kw = dict(max_new_tokens=NEW, eos_token_id=eos, pad_token_id=0, **audio)
    plain = m.generate(p, **kw)
    first = plain[0, S0:].tolist().index(eos)
    assert first <= 6 and plain.shape[1] - S0 < NEW, "the EOS must actually be hit, and stop the loop early, for this case to mean anything"
    for use_graph in (False, True):
        out = m.generate(p, use_graph=use_graph, **FLAGS, **kw)
        n = _check_shape(out, plain, S0, 1, V)
        assert n == plain.shape[1] - S0 and _same_rows(out.logits, base.logits, first + 1) and _same_rows(out.scores, base.scores, first + 1)
        assert out.past_key_values.get_seq_length() == out.sequences.shape[1] - 1
    hooked = m.generate(p, streamer=_Collect(), **FLAGS, **kw)
    assert len(hooked.scores) == len(hooked.logits) == hooked.sequences.shape[1] - S0 == first + 1 and _same_rows(hooked.logits, base.logits, first + 1)


def test_past_key_values_continue_the_sequence(dev):
    """forward(past_key_values=out.past_key_values) on the last token against logits[0] of a fresh generate() whose prompt is `sequences`.  Both are a pass over the
    same cache contents, but the two routes do not share their launches: the fresh call prefills the whole sequence (GEMM + causal attention kernels, and its
    cache rows of the generated tokens come from that prefill), forward() runs one decode step on the cache the chain kernels filled.  They are held to
    tests/_tol.py logit_tol of the row - two bf16 ulps of its largest logit."""
    from audio_flamingo_amd.modeling import AfkKVCache

    m, p, audio = _case_a(dev)
    out = _greedy_runs(dev)[1][1]
    seq = out.sequences
    pkv = out.past_key_values
    assert isinstance(pkv, AfkKVCache) and pkv.get_seq_length() == seq.shape[1] - 1
    for o in _greedy_runs(dev)[1]:
        assert o.past_key_values.get_seq_length() == seq.shape[1] - 1
    nxt = m(input_ids=seq[:, -1:], past_key_values=pkv)
    assert nxt.past_key_values.get_seq_length() == seq.shape[1]
    got = nxt.logits[:, -1].float()
    fresh = m.generate(seq, max_new_tokens=1, **FLAGS, **audio)
    want = fresh.logits[0]
    tol = _tol.logit_tol(float(want.abs().max()))
    err = float((got - want).abs().max())
    print("past_key_values: max |d logit|", err, "bar", tol)
    assert err <= tol and int(got.argmax(-1)) == int(fresh.sequences[0, -1])


def test_against_the_live_reference(dev):
    """the reference model in fp32 on the host, greedy, case A, 12 tokens, the three flags.  Per step max |ours.logits[t] - ref.logits[t]| <= floor_bar(logit_tol(
    |ref.logits[t]|max), [d_t]), d_t = the deviation of the reference's own bf16 run on the device from its fp32 run at that step (ours <= 2 x the
    reference's own bf16 deviation, capped at 3 x the absolute bar); d_t exists while the bf16 run agrees with the fp32 run on the ids so far - behind that point
    the bar is the absolute one."""
    from transformers import AudioFlamingo3ForConditionalGeneration

    from tests.test_model_gpu import G, _cfg, _ref_bf16

    m, p, audio = _case_a(dev)
    g = _CACHE["case_a"][3]
    S0 = p.shape[1]
    ref = AudioFlamingo3ForConditionalGeneration(_cfg())
    ref.load_state_dict(torch.load(os.path.join(G, "tiny64_state_bf16.pt")))
    ref = ref.float().eval()
    kw = dict(max_new_tokens=NEW, do_sample=False, **FLAGS)
    feats = g["feats"][:1].to(torch.bfloat16).float()
    with torch.no_grad():
        want = ref.generate(input_ids=p.cpu(), input_features=feats, input_features_mask=g["fmask"][:1], **kw)
        rb = _ref_bf16(dev).eval()
        own = rb.generate(input_ids=p, input_features=g["feats"][:1].to(dev).to(torch.bfloat16), input_features_mask=g["fmask"][:1].to(dev), **kw)
    out = _greedy_runs(dev)[1][1]
    assert out.sequences.cpu().tolist() == want.sequences.tolist()
    assert len(want.logits) == len(want.scores) == NEW
    ours_ts = m.compute_transition_scores(out.sequences, out.scores, normalize_logits=True).cpu()
    ref_ts = ref.compute_transition_scores(want.sequences, want.scores, normalize_logits=True)
    report = []
    for t in range(NEW):
        r = want.logits[t].float()
        abs_bar = _tol.logit_tol(float(r.abs().max()))
        agrees = own.sequences[:, : S0 + t].cpu().tolist() == want.sequences[:, : S0 + t].tolist()
        d_t = float((own.logits[t].float().cpu() - r).abs().max()) if agrees else 0.0
        bar = _tol.floor_bar(abs_bar, [d_t])
        dev_logits = float((out.logits[t].cpu() - r).abs().max())
        dev_ts = float((ours_ts[0, t] - ref_ts[0, t]).abs())
        report.append(dict(t=t, ref_absmax=float(r.abs().max()), abs_bar=abs_bar, ref_bf16_agrees=agrees, d_t=d_t, bar=bar, ours=dev_logits, ours_transition=dev_ts))
        print(report[-1])
    print("generate_outputs_reference " + json.dumps(report))   # the figures of profiles/generate_outputs.md
    for r in report:
        assert r["ours"] <= r["bar"], r
        assert r["ours_transition"] <= r["bar"] + 1e-5, r


def test_nothing_extra_is_enqueued_with_the_flags_off(dev, monkeypatch):
    from audio_flamingo_amd import _lib

    m, p, audio = _case_a(dev)
    ids, att = _padded_batch(dev)
    names = []
    real = _lib.call

    def spy(name, *a):
        names.append(name)
        return real(name, *a)

    monkeypatch.setattr(_lib, "call", spy)
    new = ("afk_decode_record", "afk_decode_sample_scored", "afk_transition_scores")
    m.generate(p, max_new_tokens=4, use_graph=False, **audio)
    m.generate(p, max_new_tokens=4, use_graph=False, output_scores=True, output_logits=True, **audio)     # no return_dict_in_generate: collects nothing
    assert "afk_decode_select_greedy" in names and not [n for n in names if n in new]
    names.clear()
    m.generate(ids, attention_mask=att, use_graph=False, **dict(BASE, max_new_tokens=4))
    assert names.count("afk_decode_sample_filtered") == 4 and not [n for n in names if n in new]
    names.clear()
    m.generate(p, max_new_tokens=4, use_graph=False, **FLAGS, **audio)                                     # ... and on: one record per step, token 0 included
    assert names.count("afk_decode_record") == 4 and "afk_decode_select_greedy" in names
    names.clear()
    m.generate(ids, attention_mask=att, use_graph=False, **FLAGS, **dict(BASE, max_new_tokens=4))          # sampled: the logits record, the scores ride in the sampler
    assert names.count("afk_decode_record") == 4 and names.count("afk_decode_sample_scored") == 4 and "afk_decode_sample_filtered" not in names


def test_refused_combinations_name_themselves(dev, monkeypatch):
    from audio_flamingo_amd import exact
    from audio_flamingo_amd._lib import AfkError

    m, p, audio = _case_a(dev)
    for how, word in ((dict(num_beams=2), "num_beams"), (dict(use_cache=False), "use_cache=False"), (dict(output_attentions=True), "output_attentions"),
                      (dict(output_hidden_states=True), "output_hidden_states")):
        with pytest.raises(AfkError, match=word):
            m.generate(p, max_new_tokens=4, **dict(FLAGS, **how), **audio)
    with monkeypatch.context() as mp:
        mp.setattr(exact, "ENABLED", True)
        with pytest.raises(AfkError, match="AFK_EXACT_FP32"):
            m.generate(p, max_new_tokens=4, **FLAGS, **audio)
    out = _greedy_runs(dev)[1][1]
    with pytest.raises(AfkError, match="beam_indices"):
        m.compute_transition_scores(out.sequences, out.scores, beam_indices=torch.zeros((1, NEW), dtype=torch.long, device=dev))

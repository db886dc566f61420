"""GPU: generate(guidance_scale=, negative_prompt_ids=, negative_prompt_attention_mask=) - classifier-free guidance inside the decode step - on the trained tiny
golden model, case A (S0 = 772 with 750 audio rows).  `neg` is the prompt without its audio ids (22 ids).

  setting   scale   negative prompt                 (the live fp32 reference on the host: 1 - 3 part from the plain greedy ids at token 0, 4 gives the plain ids)
  1         3.0     neg
  2         0.5     neg
  3         3.0     the last four prompt ids
  4         1.5     None (the last prompt id)

The bar ("item 2"): a guided row rebuilt in fp64 from two no-cache forward() calls of the same model on the returned sequence - prompt + generated[:t] with the
audio, negative + generated[:t] without - is within (|s| + |1 - s|) * 2 * logit_tol(max(|z_c|max, |z_u|max)) of scores[t]: row = s * c + (1 - s) * u, and each
branch's bf16 logits carry logit_tol (tests/_tol.py), which enters c (or u) once through z and once through the log-sum."""
import json
import os

import numpy as np
import pytest
import torch

from tests import _cfg_ref as R
from tests import _logits_process_ref as P
from tests import _tol

pytestmark = pytest.mark.gpu

FLAGS = dict(return_dict_in_generate=True, output_scores=True, output_logits=True)
NEW = 12
SETTINGS = {1: (3.0, "neg"), 2: (0.5, "neg"), 3: (3.0, "last4"), 4: (1.5, None)}
_CACHE = {}


def bits(x):
    return x.contiguous().view(torch.int32)


def _ctx(dev):
    if "ctx" not in _CACHE:
        from tests.test_generate_output_gpu import _case_a

        m, p, audio = _case_a(dev)
        neg = p[:, p[0] != m.audio_token_id].contiguous()
        assert neg.shape == (1, 22)
        _CACHE["ctx"] = (m, p, audio, dict(neg=neg, last4=p[:, -4:].contiguous()))
    return _CACHE["ctx"]


def _setting(dev, i):
    m, p, audio, negs = _ctx(dev)
    s, which = SETTINGS[i]
    return s, (negs[which] if which else None)


def _guided(dev, i, **kw):
    """the flagged greedy call of setting i, replayed from the graph (shared by the tests that compare against it)"""
    key = ("run", i, tuple(sorted(kw.items())))
    if key not in _CACHE:
        m, p, audio, _ = _ctx(dev)
        s, neg = _setting(dev, i)
        _CACHE[key] = m.generate(p, max_new_tokens=NEW, guidance_scale=s, negative_prompt_ids=neg, use_graph=True, **FLAGS, **audio, **kw)
    return _CACHE[key]


def _plain(dev):
    if "plain" not in _CACHE:
        m, p, audio, _ = _ctx(dev)
        _CACHE["plain"] = m.generate(p, max_new_tokens=NEW, **audio)
    return _CACHE["plain"]


def _branch_logits(m, ids, n, **audio):
    """the no-cache forward of ids [1, S]: the fp32 values of the bf16 logits of its last n positions -> numpy [n, V]"""
    with torch.no_grad():
        return m.forward(input_ids=ids, logits_to_keep=n, **audio).logits[0].float().cpu().numpy()


def _rebuilt(m, seq, S0, neg, s, **audio):
    """seq [1, S0 + n] as generate() returned it, neg [1, Sn] (None: the last prompt id) -> (the guided rows [n, V] in fp64, the bar per step, z_c, z_u)"""
    n = seq.shape[1] - S0
    neg = seq[:, S0 - 1:S0] if neg is None else neg
    zc = _branch_logits(m, seq[:, :-1].contiguous(), n, **audio)
    zu = _branch_logits(m, torch.cat([neg, seq[:, S0:-1]], 1).contiguous(), n)
    bars = [(abs(s) + abs(1.0 - s)) * 2.0 * _tol.logit_tol(max(np.abs(zc[t]).max(), np.abs(zu[t]).max())) for t in range(n)]
    return R.guided(zc, zu, s), bars, zc, zu


def _lowest_argmax(row):
    row = row.reshape(-1)
    return int((row == row.max()).nonzero()[0])


def _hold_item2(tag, m, out_seq_row, scores_rows, S0, neg, s, n_tokens=None, **audio):
    """item 2 for one row: scores_rows[t] [V] against the rebuilt guided row, every step; the token is the lowest-id argmax of our own scores for t < n_tokens"""
    want, bars, _, _ = _rebuilt(m, out_seq_row, S0, neg, s, **audio)
    n = len(scores_rows)
    n_tokens = n if n_tokens is None else n_tokens
    worst = 0.0
    for t in range(n):
        got = scores_rows[t].double().cpu().numpy()
        assert np.isfinite(got).all() and np.isfinite(want[t]).all()
        err = float(np.abs(got - want[t]).max())
        worst = max(worst, err / bars[t])
        print(f"{tag} t={t}: max |scores - rebuilt| {err:.4f} bar {bars[t]:.4f}")
        assert err <= bars[t], (tag, t, err, bars[t])
        if t < n_tokens:
            assert int(out_seq_row[0, S0 + t]) == _lowest_argmax(scores_rows[t]), (tag, t)
    return worst


# ---------------------------------------------------------------------------------------------- 1
@pytest.mark.parametrize("i", [1, 4])
def test_eager_against_graph_launches_and_one_capture(dev, monkeypatch, i):
    from audio_flamingo_amd import _lib

    m, p, audio, _ = _ctx(dev)
    s, neg = _setting(dev, i)
    kw = dict(max_new_tokens=NEW, guidance_scale=s, negative_prompt_ids=neg, **audio)
    names, captured, real_call, real_graph = [], [], _lib.call, torch.cuda.graph

    class Counting(real_graph):
        def __init__(self, *a, **k):
            captured.append(1)
            super().__init__(*a, **k)

    def spy(name, *a):
        names.append(name)
        return real_call(name, *a)

    monkeypatch.setattr(torch.cuda, "graph", Counting)
    monkeypatch.setattr(_lib, "call", spy)
    eager = m.generate(p, use_graph=False, **FLAGS, **kw)
    assert names.count("afk_decode_cfg") == NEW and not captured, "one fold per token, token 0 included"
    names.clear()
    graph = m.generate(p, use_graph=True, **FLAGS, **kw)
    assert len(captured) == 1 and names.count("afk_decode_cfg") == 3, "token 0, the eager step, the captured step"
    monkeypatch.undo()
    assert torch.equal(eager.sequences, graph.sequences) and eager.sequences.shape == (1, p.shape[1] + NEW)
    for t in range(NEW):
        assert torch.equal(bits(eager.scores[t]), bits(graph.scores[t])) and torch.equal(bits(eager.logits[t]), bits(graph.logits[t])), t
        assert eager.scores[t].shape == (1, m.V) and not torch.equal(bits(eager.scores[t]), bits(eager.logits[t]))
    assert torch.equal(m.generate(p, **kw), eager.sequences), "with the flags off the ids are the same"
    assert m.last_cfg_stats == dict(rows=2, prompt_slots=p.shape[1], negative_slots=1 if neg is None else neg.shape[1], cache_bytes=m.last_cfg_stats["cache_bytes"])
    assert torch.equal(graph.sequences, _guided(dev, i).sequences)
    if i == 4:
        assert torch.equal(eager.sequences, _plain(dev)), "setting 4 keeps the plain greedy ids"
    else:
        assert int(eager.sequences[0, p.shape[1]]) != int(_plain(dev)[0, p.shape[1]]), "the guidance must visibly act at token 0"


# ---------------------------------------------------------------------------------------------- 2
@pytest.mark.parametrize("i", [1, 2, 3, 4])
def test_scores_are_the_guided_rows_of_two_plain_forwards(dev, i):
    m, p, audio, _ = _ctx(dev)
    s, neg = _setting(dev, i)
    out = _guided(dev, i)
    assert len(out.scores) == len(out.logits) == NEW
    worst = _hold_item2(f"setting {i}", m, out.sequences, [r[0] for r in out.scores], p.shape[1], neg, s, **audio)
    print(f"setting {i}: worst error / bar {worst:.3f}")
    # `logits` keeps the raw conditional rows
    _, _, zc, _ = _rebuilt(m, out.sequences, p.shape[1], neg, s, **audio)
    for t in range(NEW):
        assert float(np.abs(out.logits[t][0].cpu().numpy() - zc[t]).max()) <= _tol.logit_tol(np.abs(zc[t]).max()), t
    differs = int(out.sequences[0, p.shape[1]]) != int(_plain(dev)[0, p.shape[1]])
    assert differs == (i != 4), "settings 1 - 3 part from the plain ids at token 0, setting 4 keeps them"


# ---------------------------------------------------------------------------------------------- 3
@pytest.mark.parametrize("i", [1, 2, 3, 4])
def test_against_the_live_reference(dev, i):
    """ref.generate(guidance_scale=, negative_prompt_ids=) in fp32 on the host.  For every step t before which the ids agree (token 0 always):
    max |ours.scores[t] - ref.scores[t]| over the entries finite in both <= floor_bar(abs_bar_t, [d_t]); abs_bar_t: the bar of item 2 on the reference's logits,
    d_t: the deviation of the reference's own bf16 run on the device at that step while it agrees on the ids.  At least 2 compared steps (expected: 12)."""
    from transformers import AudioFlamingo3ForConditionalGeneration

    from tests.test_model_gpu import G, _cfg, _ref_bf16

    m, p, audio, _ = _ctx(dev)
    s, neg = _setting(dev, i)
    S0 = p.shape[1]
    from tests import test_generate_output_gpu as TO

    g = TO._CACHE["case_a"][3]
    if "ref" not in _CACHE:
        ref = AudioFlamingo3ForConditionalGeneration(_cfg())
        ref.load_state_dict(torch.load(os.path.join(G, "tiny64_state_bf16.pt")))
        _CACHE["ref"] = (ref.float().eval(), _ref_bf16(dev).eval())
    ref, rb = _CACHE["ref"]
    kw = dict(max_new_tokens=NEW, do_sample=False, guidance_scale=s, **FLAGS)
    with torch.no_grad():
        want = ref.generate(input_ids=p.cpu(), input_features=g["feats"][:1].to(torch.bfloat16).float(), input_features_mask=g["fmask"][:1],
                            negative_prompt_ids=None if neg is None else neg.cpu(), **kw)
        own = rb.generate(input_ids=p, input_features=g["feats"][:1].to(dev).to(torch.bfloat16), input_features_mask=g["fmask"][:1].to(dev),
                          negative_prompt_ids=neg, **kw)
        # the reference's unconditional logits along its own sequence, for the bar
        nref = p.cpu()[:, -1:] if neg is None else neg.cpu()
        zu = ref(input_ids=torch.cat([nref, want.sequences[:, S0:-1]], 1)).logits[0, -NEW:].float().numpy()
    out = _guided(dev, i)
    report, compared = [], 0
    for t in range(NEW):
        if out.sequences[:, :S0 + t].cpu().tolist() != want.sequences[:, :S0 + t].tolist():
            break
        zc = want.logits[t][0].float().numpy()
        abs_bar = (abs(s) + abs(1.0 - s)) * 2.0 * _tol.logit_tol(max(np.abs(zc).max(), np.abs(zu[t]).max()))
        agrees = own.sequences[:, :S0 + t].cpu().tolist() == want.sequences[:, :S0 + t].tolist()
        r = want.scores[t][0].float()
        d_t = 0.0
        if agrees:
            o = own.scores[t][0].float().cpu()
            f = torch.isfinite(o) & torch.isfinite(r)
            d_t = float((o - r)[f].abs().max())
        bar = _tol.floor_bar(abs_bar, [d_t])
        ours = out.scores[t][0].cpu()
        f = torch.isfinite(ours) & torch.isfinite(r)
        err = float((ours - r)[f].abs().max())
        top = r.topk(2).values
        report.append(dict(t=t, abs_bar=abs_bar, d_t=d_t, bar=bar, ours=err, ref_gap=float(top[0] - top[1]), same_token=int(out.sequences[0, S0 + t]) == int(want.sequences[0, S0 + t])))
        print(report[-1])
        compared += 1
    print(f"cfg_reference setting {i}: compared {compared} steps " + json.dumps(report))
    for rep in report:
        assert rep["ours"] <= rep["bar"], rep
    assert compared >= 2, (i, compared)
    differs = int(want.sequences[0, S0]) != int(_plain(dev)[0, S0])
    assert differs == (i != 4), "the reference: settings 1 - 3 part from the plain ids at token 0, setting 4 keeps them"


# ---------------------------------------------------------------------------------------------- 4
@pytest.mark.parametrize("i", [1, 4])
def test_against_the_hook_route_with_the_reference_class(dev, i):
    """today's route: the reference's class around our model as a logits_processor, no guidance_scale - both sides are our bf16 kernels, batched differently"""
    from transformers import LogitsProcessorList, UnbatchedClassifierFreeGuidanceLogitsProcessor

    m, p, audio, _ = _ctx(dev)
    s, neg = _setting(dev, i)
    S0 = p.shape[1]
    hook = m.generate(p, max_new_tokens=NEW, logits_processor=LogitsProcessorList([UnbatchedClassifierFreeGuidanceLogitsProcessor(s, m, neg)]), **FLAGS, **audio)
    assert m.last_cfg_stats is None
    out = _guided(dev, i)
    _, bars, _, _ = _rebuilt(m, out.sequences, S0, neg, s, **audio)
    compared = 0
    for t in range(min(NEW, hook.sequences.shape[1] - S0)):
        if hook.sequences[:, :S0 + t].tolist() != out.sequences[:, :S0 + t].tolist():
            break
        err = float((hook.scores[t].float() - out.scores[t]).abs().max())
        print(f"hook route setting {i} t={t}: max |d scores| {err:.4f} bar {bars[t]:.4f}")
        assert err <= bars[t], (t, err, bars[t])
        compared += 1
    assert compared >= 2


# ---------------------------------------------------------------------------------------------- 5
def test_padded_batch_with_ragged_negatives_and_an_eos_list(dev):
    m = _ctx(dev)[0]
    g = torch.Generator().manual_seed(11)
    lens, nlens, S0, Sn, s, pad = (40, 23), (50, 9), 40, 50, 2.0, 0       # negative 0 is longer than its prompt row, negative 1 shorter: Smax = 50 > S0
    ids, att = torch.zeros((2, S0), dtype=torch.long), torch.zeros((2, S0), dtype=torch.long)
    neg, natt = torch.zeros((2, Sn), dtype=torch.long), torch.zeros((2, Sn), dtype=torch.long)
    for b in range(2):
        ids[b, S0 - lens[b]:], att[b, S0 - lens[b]:] = torch.randint(1, 256, (lens[b],), generator=g), 1
        neg[b, Sn - nlens[b]:], natt[b, Sn - nlens[b]:] = torch.randint(1, 256, (nlens[b],), generator=g), 1
    ids, att, neg, natt = ids.to(dev), att.to(dev), neg.to(dev), natt.to(dev)
    kw = dict(attention_mask=att, max_new_tokens=NEW, guidance_scale=s, negative_prompt_ids=neg, negative_prompt_attention_mask=natt, pad_token_id=pad)
    free = m.generate(ids, **kw)
    assert free.shape == (2, S0 + NEW)
    # an eos pair: row 0's token 3 (if row 1 emitted it no later, take row 1's view) and an id nobody emits - the stop launch runs and one row ends early
    e0 = int(free[0, S0 + 3])
    first = [free[b, S0:].tolist().index(e0) if e0 in free[b, S0:].tolist() else NEW for b in range(2)]
    unused = next(v for v in range(300, 1000) if v not in free[:, S0:].tolist()[0] + free[:, S0:].tolist()[1])
    assert min(first) <= 3 and max(first) > min(first), (first, "one row must end early and the other later for this case to mean anything")
    for use_graph in (False, True):
        out = m.generate(ids, eos_token_id=[e0, unused], use_graph=use_graph, **FLAGS, **kw)
        n = out.sequences.shape[1] - S0
        assert n == min(max(first) + 1, NEW) and len(out.scores) == len(out.logits) == n, "the reference's shape: cut at the step at which the last row finished"
        assert m.last_cfg_stats["rows"] == 4 and m.last_cfg_stats["prompt_slots"] == S0 and m.last_cfg_stats["negative_slots"] == Sn
        for b in range(2):
            end = min(first[b], n - 1)
            new = out.sequences[b, S0:].tolist()
            assert new[:end + 1] == free[b, S0:S0 + end + 1].tolist() and all(v == pad for v in new[end + 1:]), (b, new, first)
            # item 2 on the row's real ids: the rebuild runs on the returned sequence, pad ids behind the row's end included - so the rows behind the end hold
            # only if BOTH cache rows of the pair were fed pad_token_id
            seq_b = torch.cat([ids[b:b + 1, S0 - lens[b]:], out.sequences[b:b + 1, S0:]], 1)
            _hold_item2(f"batch row {b} graph={use_graph}", m, seq_b, [r[b] for r in out.scores], lens[b], neg[b:b + 1, Sn - nlens[b]:], s, n_tokens=end + 1)
        kv = out.past_key_values
        assert kv.K.shape[1] == 2 and kv.lo.tolist() == [S0 - lens[0], S0 - lens[1]] and kv.get_seq_length() == S0 + n - 1


# ---------------------------------------------------------------------------------------------- 6
def test_sampled_three_routes_and_copies(dev):
    class _Collect:
        def put(self, v):
            pass

        def end(self):
            pass

    m, p, audio, _ = _ctx(dev)
    s, neg = _setting(dev, 1)
    S0, T = p.shape[1], 0.8
    kw = dict(max_new_tokens=NEW, guidance_scale=s, negative_prompt_ids=neg, do_sample=True, seed=1234, top_k=20, temperature=T, **audio)
    eager = m.generate(p, use_graph=False, **FLAGS, **kw)
    graph = m.generate(p, use_graph=True, **FLAGS, **kw)
    hooked = m.generate(p, streamer=_Collect(), **FLAGS, **kw)
    assert torch.equal(eager.sequences, graph.sequences) and torch.equal(eager.sequences, hooked.sequences)
    want, bars, _, _ = _rebuilt(m, eager.sequences, S0, neg, s, **audio)
    for t in range(NEW):
        assert torch.equal(bits(eager.scores[t]), bits(graph.scores[t])) and torch.equal(bits(eager.scores[t]), bits(hooked.scores[t])), t
        row = eager.scores[t][0].double().cpu().numpy()
        keep = np.isfinite(row)
        kept = np.sort(row[keep])
        extra = int(keep.sum()) - 20     # TopKLogitsWarper removes scores < the 20th largest: ids that tie with it stay, so a tie at the edge keeps more than 20
        assert extra >= 0 and (kept[:extra + 1] == kept[0]).all() and np.isneginf(row[~keep]).all(), (t, int(keep.sum()), kept[:extra + 2])
        err = float(np.abs(row[keep] * T - want[t][keep]).max())
        print(f"sampled t={t}: max |scores * T - rebuilt| {err:.4f} bar {bars[t]:.4f}")
        assert err <= bars[t], (t, err, bars[t])
        assert want[t][keep].min() >= want[t][~keep].max() - 2 * bars[t], (t, "the kept ids are no top-20 set of the guided row")
        assert bool(keep[int(eager.sequences[0, S0 + t])])
    two = m.generate(p, num_return_sequences=2, **FLAGS, **kw)
    assert two.sequences.shape == (2, S0 + NEW) and two.scores[0].shape == (2, m.V) and m.last_cfg_stats["rows"] == 4
    for b in range(2):   # the negative prompt was repeated row by row like the other inputs
        want_b, bars_b, _, _ = _rebuilt(m, two.sequences[b:b + 1], S0, neg, s, **audio)
        for t in range(NEW):
            row = two.scores[t][b].double().cpu().numpy()
            keep = np.isfinite(row)
            assert float(np.abs(row[keep] * T - want_b[t][keep]).max()) <= bars_b[t], (b, t)


# ---------------------------------------------------------------------------------------------- 7
def test_guidance_runs_in_front_of_the_built_in_processors(dev):
    m, p, audio, _ = _ctx(dev)
    s, neg = _setting(dev, 1)
    S0 = p.shape[1]
    out = _guided(dev, 1, repetition_penalty=1.3, no_repeat_ngram_size=2)
    want, bars, _, _ = _rebuilt(m, out.sequences, S0, neg, s, **audio)
    for t in range(NEW):
        guided = torch.from_numpy(want[t][None].astype(np.float32))
        ref = P.restated(guided, out.sequences[:, :S0 + t], t, penalty=1.3, ngram=2)
        got = out.scores[t].cpu()
        assert torch.equal(torch.isneginf(got), torch.isneginf(ref)), (t, "the banned ids differ")
        f = torch.isfinite(ref)
        err = float((got - ref)[f].abs().max())
        print(f"processors t={t}: max |scores - restated(rebuilt)| {err:.4f} bar {1.3 * bars[t]:.4f} banned {int((~f).sum())}")
        assert err <= 1.3 * bars[t], (t, err)
        assert int(out.sequences[0, S0 + t]) == _lowest_argmax(out.scores[t])


# ---------------------------------------------------------------------------------------------- 8
def test_past_key_values_are_the_conditional_rows(dev):
    from audio_flamingo_amd.modeling import AfkKVCache

    m, p, audio, _ = _ctx(dev)
    out = _guided(dev, 1)
    seq, pkv = out.sequences, out.past_key_values
    assert isinstance(pkv, AfkKVCache) and pkv.K.shape[1] == 1 and pkv.Vt.shape[1] == 1 and pkv.get_seq_length() == seq.shape[1] - 1 and pkv.lo.tolist() == [0]
    nxt = m(input_ids=seq[:, -1:], past_key_values=pkv)
    got = nxt.logits[:, -1].float()
    fresh = m.generate(seq, max_new_tokens=1, **FLAGS, **audio)
    want = fresh.logits[0]
    tol = _tol.logit_tol(float(want.abs().max()))
    err = float((got - want).abs().max())
    print("guided past_key_values: max |d logit|", err, "bar", tol)
    assert err <= tol


# ---------------------------------------------------------------------------------------------- 9
def test_inactive_guidance_changes_no_launch(dev, monkeypatch):
    from audio_flamingo_amd import _lib

    m, p, audio, negs = _ctx(dev)
    names, real = [], _lib.call

    def spy(name, *a):
        names.append(name)
        return real(name, *a)

    _guided(dev, 1)
    monkeypatch.setattr(_lib, "call", spy)
    runs = []
    for kw in (dict(), dict(guidance_scale=None, negative_prompt_ids=negs["neg"]), dict(guidance_scale=1.0, negative_prompt_ids=negs["neg"]),
               dict(guidance_scale=1, negative_prompt_ids=negs["neg"], negative_prompt_attention_mask=torch.ones_like(negs["neg"]))):
        names.clear()
        ids = m.generate(p, max_new_tokens=6, use_graph=False, **audio, **kw)
        assert m.last_cfg_stats is None
        runs.append((list(names), ids))
    for got, ids in runs[1:]:
        assert got == runs[0][0] and torch.equal(ids, runs[0][1])
    assert "afk_decode_cfg" not in runs[0][0] and "afk_decode_select_greedy" in runs[0][0]


# ---------------------------------------------------------------------------------------------- 10
def test_refusals_name_the_combination(dev, monkeypatch):
    from audio_flamingo_amd import exact
    from audio_flamingo_amd._lib import AfkError

    m, p, audio, negs = _ctx(dev)
    base = dict(max_new_tokens=4, guidance_scale=2.0, negative_prompt_ids=negs["neg"], **audio)
    prev = _guided(dev, 1)
    for how, word in ((dict(num_beams=2), "num_beams > 1"), (dict(use_cache=False), "use_cache=False"), (dict(prompt_lookup_num_tokens=3), "prompt_lookup_num_tokens"),
                      (dict(share_prompt=True), "share_prompt=True")):
        with pytest.raises(AfkError, match=word) as e:
            m.generate(p, **dict(base, **how))
        assert "guidance_scale" in str(e.value)
    seq = prev.sequences
    with pytest.raises(AfkError, match="past_key_values") as e:
        m.generate(torch.cat([seq, seq[:, -1:]], 1), past_key_values=prev.past_key_values, **dict(base, input_features=None, input_features_mask=None))
    assert "guidance_scale" in str(e.value)
    with monkeypatch.context() as mp:
        mp.setattr(exact, "ENABLED", True)
        with pytest.raises(AfkError, match="AFK_EXACT_FP32=1"):
            m.generate(p, **base)
    with pytest.raises(AfkError, match=f"audio placeholder id {m.audio_token_id}"):
        m.generate(p, **dict(base, negative_prompt_ids=p[:, -30:]))
    with pytest.raises(ValueError, match=r"holds 2 rows.*holds 1"):
        m.generate(p, **dict(base, negative_prompt_ids=negs["neg"].repeat(2, 1)))
    with pytest.raises(ValueError, match="negative_prompt_attention_mask"):
        m.generate(p, negative_prompt_attention_mask=torch.ones((1, 5), dtype=torch.long, device=dev), **base)
    holes = torch.ones_like(negs["neg"])
    holes[0, 3] = 0
    with pytest.raises(AfkError, match="attention masks with holes"):
        m.generate(p, negative_prompt_attention_mask=holes, **base)
    with monkeypatch.context() as mp:   # the class attribute on, the keyword unset: the unshared route, silently
        mp.setattr(type(m), "share_prompt_cache", True)
        out = m.generate(p, do_sample=True, seed=5, num_return_sequences=2, **base)
        assert out.shape[0] == 2 and m.last_share_stats is None and m.last_cfg_stats["rows"] == 4
    assert m.last_cfg_stats is not None
    m.generate(p, max_new_tokens=2, **audio)
    assert m.last_cfg_stats is None

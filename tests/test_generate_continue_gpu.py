"""GPU: generate(past_key_values=cache) - a chat turn continued on the cache the previous turn returned - against the from-scratch call on the whole
conversation, on the trained tiny golden model (case A: one 750-row audio clip + text).

The conversations walk the golden greedy continuation g[0:24] of case A, where the tiny model is decisive: a turn's answer is what the model emits, the
next turn's "user text" is the stretch of g behind it.  The CPU oracle (fp32) puts the top-1 / top-2 gap of positions 0 .. 19 at >= 6.4 x the logit bar of
tests/_tol.py (position 20: 2.7 x), so every emitted position here lies in 0 .. 19 - and each comparison of a continued call with the from-scratch call
asserts, from the from-scratch call's own logits, that EVERY emitted position has a gap above 2 x that bar: then a difference of ids is a bug, not a tie.

  turn 1   prompt p (audio + text)          -> g[0:5]
  turn 2   + g[0:5] + g[5:8]                -> g[8:13]
  turn 3   + g[8:13] + g[13:15]             -> g[15:20]"""
import os

import pytest
import torch

from tests import _stop_ref as R
from tests._tol import logit_tol
from tests.test_sampler_gpu import _case_a

pytestmark = pytest.mark.gpu

N = 5
# turn 2 with a second clip: (window of the golden batch used as that clip, start and length of the stretch of g behind its <sound> rows, tokens emitted).
# A clip in the middle of the text is outside what the tiny model was trained on and most suffixes leave it undecided; a search with the CPU oracle over
# the stretches of g found this one, whose three emitted positions have gaps of 8.4, 8.8 and 10.2 x the logit bar.
CLIP = (1, 3, 3, 3)
FLAGS = dict(return_dict_in_generate=True, output_logits=True)
_CTX = {}


def _ctx(dev):
    if dev not in _CTX:
        from tests.test_model_gpu import G, N_GEN

        g = torch.load(os.path.join(G, "tiny64_caseA.pt"))
        m, p, audio = _case_a(dev)
        gold = g["generate"][0, -N_GEN:].to(dev)
        full2 = torch.cat([p, gold[None, :8]], 1)
        full3 = torch.cat([p, gold[None, :15]], 1)
        _CTX[dev] = (m, p, audio, gold, full2, full3, g)
    return _CTX[dev]


def _turn1(m, p, audio, **kw):
    """turn 1 -> its cache (a fresh object every time: a continuation updates it in place)"""
    out = m.generate(p, max_new_tokens=N, return_dict_in_generate=True, **audio, **kw)
    return out.past_key_values, out.sequences


def _decisive(tag, logits):
    """every emitted position of the from-scratch call: top-1 / top-2 gap above 2 x the logit bar; none excused"""
    gaps = []
    for i, row in enumerate(logits):
        row = row.float()
        top = row.topk(2, -1).values
        bar = logit_tol(float(row[torch.isfinite(row)].abs().max()))
        gaps.append(float((top[..., 0] - top[..., 1]).min()) / bar)
    print(f"{tag}: top-1 / top-2 gaps in units of the logit bar: {[round(x, 2) for x in gaps]}")
    assert min(gaps) > 2.0, f"{tag}: an emitted position is not decisive (gaps / bar {[round(x, 2) for x in gaps]}): the comparison cannot tell a bug from a tie"


def test_two_turns_equal_the_from_scratch_call(dev):
    m, p, audio, gold, full2, _, _ = _ctx(dev)
    A = m.generate(full2, max_new_tokens=N, **audio, **FLAGS)
    _decisive("from scratch, turn 2", A.logits)
    assert A.sequences[0, full2.shape[1]:].tolist() == gold[8:13].tolist()
    cache, seq1 = _turn1(m, p, audio)
    assert seq1[0, p.shape[1]:].tolist() == gold[:5].tolist() and cache.get_seq_length() == p.shape[1] + N - 1
    B = m.generate(full2, past_key_values=cache, max_new_tokens=N, **FLAGS)
    assert B.sequences.shape == A.sequences.shape and torch.equal(B.sequences, A.sequences)
    a0, b0 = A.logits[0].float(), B.logits[0].float()
    err, bar = float((a0 - b0).abs().max()), logit_tol(float(a0.abs().max()))
    print(f"first-step logits: max |continued - from scratch| = {err:.4f}, bar {bar:.4f}")
    assert err <= bar
    assert B.past_key_values is cache and cache.get_seq_length() == full2.shape[1] + N - 1


def test_turn_two_with_a_second_clip(dev):
    """the suffix holds <sound> ids: the continuation is given the NEW clip's features only, the from-scratch call both clips"""
    m, p, audio, gold, _, _, g = _ctx(dev)
    n_sound = int((p == m.audio_token_id).sum())
    f2, m2 = g["feats"][CLIP[0]:CLIP[0] + 1].to(dev), g["fmask"][CLIP[0]:CLIP[0] + 1].to(dev)
    suffix = torch.cat([gold[5:7], torch.full((n_sound,), m.audio_token_id, device=dev), gold[CLIP[1]:CLIP[1] + CLIP[2]]])
    full = torch.cat([p, gold[None, :5], suffix[None]], 1)
    both = dict(input_features=torch.cat([audio["input_features"], f2]), input_features_mask=torch.cat([audio["input_features_mask"], m2]))
    A = m.generate(full, max_new_tokens=CLIP[3], **both, **FLAGS)
    _decisive("from scratch, two clips", A.logits)
    cache, _ = _turn1(m, p, audio)
    B = m.generate(full, past_key_values=cache, max_new_tokens=CLIP[3], input_features=f2, input_features_mask=m2)
    assert torch.equal(B, A.sequences)
    assert cache.get_seq_length() == full.shape[1] + CLIP[3] - 1


def test_growth_updates_the_passed_cache_in_place(dev):
    m, p, audio, gold, full2, _, _ = _ctx(dev)
    cache, _ = _turn1(m, p, audio)
    K0, cap0 = cache.K, cache.K.shape[2]
    assert cap0 == p.shape[1] + N and cache.length == cap0 - 1, "turn 1 leaves one free slot: turn 2 cannot fit"
    out = m.generate(full2, past_key_values=cache, max_new_tokens=N, return_dict_in_generate=True)
    assert out.past_key_values is cache and cache.K is not K0 and cache.K.shape[2] >= full2.shape[1] + N
    assert cache.Vt.shape[4] >= cache.K.shape[2] and cache.length == full2.shape[1] + N - 1
    assert torch.equal(cache.K[:, :, : cap0 - 1], K0[:, :, : cap0 - 1]), "the past was copied"
    assert out.sequences[0, full2.shape[1]:].tolist() == gold[8:13].tolist()


def test_three_turns_in_a_loop_on_one_cache(dev):
    m, p, audio, gold, full2, full3, _ = _ctx(dev)
    scratch = [m.generate(ids, max_new_tokens=N, **audio) for ids in (p, full2, full3)]
    cache, got = None, []
    for ids in (p, full2, full3):
        out = m.generate(ids, past_key_values=cache, max_new_tokens=N, return_dict_in_generate=True, **(audio if cache is None else {}))
        assert cache is None or out.past_key_values is cache
        cache = out.past_key_values
        got.append(out.sequences)
        assert cache.get_seq_length() == ids.shape[1] + N - 1
    for a, b in zip(scratch, got):
        assert torch.equal(a, b)
    assert got[2][0, full3.shape[1]:].tolist() == gold[15:20].tolist()


def test_composition_with_the_other_features(dev):
    m, p, audio, gold, full2, _, _ = _ctx(dev)
    cont = lambda **kw: m.generate(full2, past_key_values=_turn1(m, p, audio)[0], **kw)
    # the step on and off the HIP graph, against the from-scratch call (decisive: test_two_turns)
    plain = m.generate(full2, max_new_tokens=N, **audio)
    for ug in (False, True):
        assert torch.equal(cont(max_new_tokens=N, use_graph=ug), plain)
    # sampled with a seed: the continued call against itself, graph against eager, bit for bit
    kw = dict(do_sample=True, temperature=1.5, top_k=20, top_p=0.95, seed=0xFEED_0000_0007, max_new_tokens=8)
    s_eager, s_graph = cont(use_graph=False, **kw), cont(use_graph=True, **kw)
    assert s_eager.shape[1] == full2.shape[1] + 8 and torch.equal(s_eager, s_graph)
    # processors whose history is the whole conversation as passed
    kw = dict(repetition_penalty=1.3, no_repeat_ngram_size=2, max_new_tokens=N)
    A = m.generate(full2, **audio, **kw, return_dict_in_generate=True, output_scores=True)
    _decisive("from scratch, repetition_penalty + no_repeat_ngram_size", A.scores)
    assert torch.equal(cont(**kw), A.sequences)
    # a stop string that ends inside the turn
    new = gold[8:13].tolist()
    assert len(set(new[1:4])) == 3
    tok = R.tiny_tokenizer({new[1]: "Hel", new[2]: "lo", new[3]: " world"})
    kw = dict(stop_strings=["lo w"], tokenizer=tok, max_new_tokens=N)
    A = m.generate(full2, **audio, **kw)
    assert A.shape[1] == full2.shape[1] + 4 and torch.equal(cont(**kw), A)
    # prompt-lookup decoding: the drafted slots go into the headroom
    kw = dict(prompt_lookup_num_tokens=3, max_new_tokens=N)
    A = m.generate(full2, **audio, **kw)
    assert torch.equal(A, plain)
    stats_a = dict(m.last_lookup_stats)
    cache = _turn1(m, p, audio)[0]
    assert torch.equal(m.generate(full2, past_key_values=cache, **kw), plain)
    assert m.last_lookup_stats["emitted"] == stats_a["emitted"] == N and cache.get_seq_length() == full2.shape[1] + N - 1
    assert cache.K.shape[2] >= full2.shape[1] + N + 3


def test_left_padded_batch_and_refusals(dev):
    from audio_flamingo_amd._lib import AfkError

    m, p, audio, gold, full2, _, _ = _ctx(dev)
    pad = torch.zeros((2, 3), dtype=p.dtype, device=dev)
    rep = lambda x: x.repeat(2, *([1] * (x.dim() - 1)))
    ids1, att1 = torch.cat([pad, rep(p)], 1), torch.cat([torch.zeros_like(pad), torch.ones_like(rep(p))], 1)
    audio2 = {k: rep(v) for k, v in audio.items()}
    out1 = m.generate(ids1, attention_mask=att1, max_new_tokens=N, return_dict_in_generate=True, **audio2)
    cache = out1.past_key_values
    assert cache.lo.tolist() == [3, 3] and out1.sequences[:, ids1.shape[1]:].tolist() == [gold[:5].tolist()] * 2
    ids2 = torch.cat([pad, rep(full2)], 1)
    att2 = torch.cat([torch.zeros_like(pad), torch.ones_like(rep(full2))], 1)
    A = m.generate(ids2, attention_mask=att2, max_new_tokens=N, **audio2, **FLAGS)
    _decisive("from scratch, left-padded batch of two", A.logits)
    hole = att2.clone()
    hole[1, 20] = 0
    with pytest.raises(AfkError, match="attention masks with holes"):
        m.generate(ids2, attention_mask=hole, past_key_values=cache, max_new_tokens=N)
    with pytest.raises(AfkError, match="attention masks with holes"):
        m.generate(ids2, attention_mask=torch.ones_like(att2), past_key_values=cache, max_new_tokens=N)
    assert cache.get_seq_length() == ids1.shape[1] + N - 1, "a refused call leaves the cache as it was"
    B = m.generate(ids2, attention_mask=att2, past_key_values=cache, max_new_tokens=N)
    assert torch.equal(B, A.sequences)
    # refusals
    c1 = _turn1(m, p, audio)[0]
    with pytest.raises(AfkError, match="num_beams"):
        m.generate(full2, past_key_values=c1, num_beams=2, max_new_tokens=N)
    with pytest.raises(AfkError, match="use_cache=False"):
        m.generate(full2, past_key_values=c1, use_cache=False, max_new_tokens=N)
    for ids in (full2[:, : c1.get_seq_length()], full2[:, : c1.get_seq_length() - 2]):
        with pytest.raises(ValueError, match=rf"{c1.get_seq_length()} positions.*{ids.shape[1]}"):
            m.generate(ids, past_key_values=c1, max_new_tokens=N)
    with pytest.raises(AfkError, match="past_key_values"):
        m.generate(full2, past_key_values=(1, 2), max_new_tokens=N)
    assert torch.equal(m.generate(full2, past_key_values=c1, max_new_tokens=N), m.generate(full2, max_new_tokens=N, **audio)), "the refusals left the cache usable"


def test_a_reference_dynamic_cache(dev):
    from transformers import DynamicCache

    m, p, audio, gold, full2, _, _ = _ctx(dev)
    plain = m.generate(full2, max_new_tokens=N, **audio)
    # this model prefills the reference's cache object; generate() continues on it (P = the prompt: the turn-1 answer is part of the suffix)
    rc = DynamicCache()
    o = m(input_ids=p, past_key_values=rc, use_cache=True, logits_to_keep=1, **audio)
    assert o.past_key_values is rc and rc.get_seq_length() == p.shape[1]
    out = m.generate(full2, past_key_values=rc, max_new_tokens=N, return_dict_in_generate=True)
    assert torch.equal(out.sequences, plain) and out.past_key_values is rc
    assert rc.get_seq_length() == full2.shape[1] + N - 1 and tuple(rc.layers[0].keys.shape) == (1, m.Hkv, full2.shape[1] + N - 1, m.D)
    # an EMPTY reference cache: the ordinary fresh prefill - the launches of the call without a cache - written back; left padding included
    from audio_flamingo_amd import _lib

    def traced(**kw):
        names, real = [], _lib.call
        _lib.call = lambda name, *a: (names.append(name), real(name, *a))[1]
        try:
            return m.generate(full2, max_new_tokens=N, **audio, **kw), names
        finally:
            _lib.call = real

    rc = DynamicCache()
    (a, na), (b, nb) = traced(), traced(past_key_values=rc)
    assert torch.equal(b, plain) and torch.equal(a, plain) and na == nb and "afk_attn_append" not in nb
    assert rc.get_seq_length() == full2.shape[1] + N - 1
    pad = torch.zeros((1, 3), dtype=full2.dtype, device=dev)
    ids_p, att_p = torch.cat([pad, full2], 1), torch.cat([torch.zeros_like(pad), torch.ones_like(full2)], 1)
    rc = DynamicCache()
    out_p = m.generate(ids_p, attention_mask=att_p, past_key_values=rc, max_new_tokens=N, **audio)
    assert torch.equal(out_p, m.generate(ids_p, attention_mask=att_p, max_new_tokens=N, **audio)) and rc.get_seq_length() == ids_p.shape[1] + N - 1
    # the reverse direction: the REFERENCE prefills its cache, generate() continues on it
    from tests.test_model_gpu import _ref_bf16

    ref = _ref_bf16(dev).eval()
    rc = DynamicCache()
    with torch.no_grad():
        ref(input_ids=p, input_features=audio["input_features"].to(torch.bfloat16), input_features_mask=audio["input_features_mask"], past_key_values=rc, use_cache=True)
    assert rc.get_seq_length() == p.shape[1]
    assert torch.equal(m.generate(full2, past_key_values=rc, max_new_tokens=N), plain) and rc.get_seq_length() == full2.shape[1] + N - 1


def test_without_a_cache_nothing_changes(dev, monkeypatch):
    """past_key_values=None is the call without the keyword: the same launches in the same order, the same ids, the same lookup counters (what the call
    without the keyword enqueues is pinned against the recording by tests/test_generate_trace_gpu.py)"""
    from audio_flamingo_amd import _lib

    m, p, audio, gold, full2, _, _ = _ctx(dev)
    m.generate(p, max_new_tokens=N, **audio)   # warm every per-model cache
    real = _lib.call

    def traced(**kw):
        names = []
        monkeypatch.setattr(_lib, "call", lambda name, *a: (names.append(name), real(name, *a))[1])
        try:
            return m.generate(p, **audio, **kw), names
        finally:
            monkeypatch.undo()

    for kw in (dict(max_new_tokens=12), dict(max_new_tokens=12, prompt_lookup_num_tokens=3), dict(max_new_tokens=8, do_sample=True, seed=5)):
        a, na = traced(**kw)
        sa = dict(getattr(m, "last_lookup_stats", {}))
        b, nb = traced(past_key_values=None, **kw)
        assert torch.equal(a, b) and na == nb and "afk_attn_append" not in na, kw
        assert dict(getattr(m, "last_lookup_stats", {})) == sa
    # and a continuation does go through the new kernel
    names = []
    cache = _turn1(m, p, audio)[0]
    monkeypatch.setattr(_lib, "call", lambda name, *a: (names.append(name), real(name, *a))[1])
    m.generate(full2, past_key_values=cache, max_new_tokens=N)
    monkeypatch.undo()
    assert names.count("afk_attn_append") == m.dec_layers and "afk_xattn_fwd" not in names

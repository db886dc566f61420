"""GPU: generate(share_prompt=True) on the trained tiny model - the sampled copies and the device beams of a row on ONE prefill and ONE copy of the prompt's keys
(decode_share.py, afk_attn_decode_shared).  The yardstick holds whatever the draws were: every recorded logits row against the no-cache forward() of the
returned sequence.  The id comparisons against the unshared call hold where the draws are not near-ties (the prefill runs on other row counts, so the two calls'
logits differ by rounding): their seeds were chosen once on the GPU, and a failure shows the two calls' logits at the first differing step."""
import pytest
import torch

from tests._tol import logit_tol

pytestmark = pytest.mark.gpu

NEW = 12   # a poll at step 8 is crossed
FLAGS = dict(return_dict_in_generate=True, output_logits=True)
SAMPLED = dict(do_sample=True, temperature=1.5, top_k=0)
# chosen once on an MI355X out of 1 .. 8: with 2 and 6 the shared and the unshared call draw the same ids in every comparison below (the other six part
# somewhere at a draw whose two logits rows are 0.03 .. 0.13 apart, inside logit_tol of about 0.22: near-ties)
SEED = 2
SEED_ROUTES = 2


def _cases(dev):
    from tests.test_beam_gpu import _cases as beam_cases

    return beam_cases(dev)


def _att(ids, audio):
    return audio.get("attention_mask", torch.ones_like(ids))


def _first_difference(a, b, S0):
    """where two output objects' sequences part, with both calls' logits there: inside logit_tol the draw was a near-tie, outside it is a bug"""
    if a.sequences.shape == b.sequences.shape and torch.equal(a.sequences, b.sequences):
        return None
    n = min(a.sequences.shape[1], b.sequences.shape[1])
    diff = (a.sequences[:, :n] != b.sequences[:, :n]).nonzero()
    if not len(diff):
        return f"lengths {a.sequences.shape[1]} and {b.sequences.shape[1]}"
    col = int(diff[:, 1].min())
    row = int(diff[diff[:, 1] == col][0, 0])
    t = col - S0
    la, lb = a.logits[t][row].float(), b.logits[t][row].float()
    err, bar = float((la - lb).abs().max()), logit_tol(float(lb.abs().max()))
    return (f"row {row} parts at generated token {t}: ids {int(a.sequences[row, col])} / {int(b.sequences[row, col])}; the two calls' logits of that step differ by "
            f"{err:.4f} at most (logit_tol {bar:.4f}: {'a near-tie in the draw' if err <= bar else 'A BUG'})")


def _pair(m, ids, audio, **kw):
    """(shared, unshared) output objects of one call"""
    kw = dict(audio, max_new_tokens=NEW, **FLAGS, **kw)
    return m.generate(ids, share_prompt=True, **kw), m.generate(ids, share_prompt=False, **kw)


# ------------------------------------------------------------------------------------------------ sampled copies
@pytest.mark.parametrize("case", ["A", "Apad"])
def test_sampled_copies_against_the_no_cache_forward(dev, case):
    """the yardstick: every recorded logits row of every generated position within logit_tol of forward() on the returned sequence - the single prefill,
    the positions, the left padding and the two-cache attention, whatever the draws were"""
    m, cases, _, _ = _cases(dev)
    ids, audio = cases[case]
    n, (B0, S0) = 3, ids.shape
    out = m.generate(ids, num_return_sequences=n, seed=77, share_prompt=True, max_new_tokens=NEW, **SAMPLED, **FLAGS, **audio)
    st = m.last_share_stats
    assert st is not None and st["prompt_rows"] == B0 and st["copies"] == n and st["prompt_slots"] == S0 and st["tail_slots"] == NEW
    assert st["cache_bytes"] < st["unshared_cache_bytes"]
    seq = out.sequences
    assert seq.shape == (B0 * n, S0 + NEW) and torch.equal(seq[:, :S0], ids.repeat_interleave(n, 0)) and len(out.logits) == NEW
    for b0 in range(B0):
        assert len({tuple(r) for r in seq[b0 * n:(b0 + 1) * n, S0:].tolist()}) == n, "the draw is keyed by (step, row): the copies differ"
    att = torch.cat([_att(ids, audio).repeat_interleave(n, 0), torch.ones((B0 * n, NEW), device=dev, dtype=torch.long)], 1)
    with torch.no_grad():
        ref = m(input_ids=seq, input_features=audio["input_features"].repeat_interleave(n, 0), input_features_mask=audio["input_features_mask"].repeat_interleave(n, 0),
                attention_mask=att, position_ids=(att.cumsum(-1) - 1).clamp_min(0)).logits.float()
    worst = 0.0
    for t in range(NEW):
        want, got = ref[:, S0 - 1 + t], out.logits[t].float()
        for r in range(B0 * n):
            err, bar = float((got[r] - want[r]).abs().max()), logit_tol(float(want[r].abs().max()))
            worst = max(worst, err / bar)
            assert err <= bar, f"case {case}: row {r}, generated token {t}: max |d logit| {err:.4f} > logit_tol {bar:.4f}"
    print(f"case {case}: worst |d logit| / logit_tol over {NEW} x {B0 * n} rows: {worst:.3f}")
    # the materialised cache continues the sequences: one more position through forward(past_key_values=...)
    pkv = out.past_key_values
    assert pkv.get_seq_length() == S0 + NEW - 1 and pkv.K.shape[1] == B0 * n and pkv.lo.tolist() == [int(x) for x in (S0 - _att(ids, audio).sum(-1)).repeat_interleave(n).tolist()]
    nxt = m(input_ids=seq[:, -1:], past_key_values=pkv).logits[:, -1].float()
    want = ref[:, -1]   # the no-cache forward's next-token logits behind the whole sequence
    for r in range(B0 * n):
        err, bar = float((nxt[r] - want[r]).abs().max()), logit_tol(float(want[r].abs().max()))
        assert err <= bar, f"case {case}: forward(past_key_values=<materialised cache>) row {r}: max |d logit| {err:.4f} > logit_tol {bar:.4f}"


def sampled_ids_difference(m, ids, audio, seed):
    a, b = _pair(m, ids, audio, num_return_sequences=3, seed=seed, **SAMPLED)
    return _first_difference(a, b, ids.shape[1])


@pytest.mark.parametrize("case", ["A", "Apad"])
def test_sampled_ids_equal_the_unshared_call(dev, case):
    m, cases, _, _ = _cases(dev)
    ids, audio = cases[case]
    diff = sampled_ids_difference(m, ids, audio, SEED)
    assert diff is None, f"case {case}, seed {SEED}: {diff}"


# ------------------------------------------------------------------------------------------------ beams
@pytest.mark.parametrize("case", ["A", "Apad"])
def test_beams_equal_the_unshared_call(dev, case):
    m, cases, eos, eos2 = _cases(dev)
    ids, audio = cases[case]
    lengths = set()
    for stop in ({}, dict(eos_token_id=[eos, eos2], pad_token_id=0)):
        for n_ret in (1, 3):
            kw = dict(audio, max_new_tokens=NEW, num_beams=4, num_return_sequences=n_ret, **stop)
            want = m.generate(ids, share_prompt=False, **kw)
            assert m.last_share_stats is None
            for use_graph in (False, True):
                got = m.generate(ids, share_prompt=True, use_graph=use_graph, **kw)
                assert torch.equal(got, want), (case, stop, n_ret, use_graph, got.tolist(), want.tolist())
                st = m.last_share_stats
                assert st["prompt_rows"] == ids.shape[0] and st["copies"] == 4 and st["tail_slots"] == NEW and st["cache_bytes"] < st["unshared_cache_bytes"]
            lengths.add(want.shape[1] - ids.shape[1])
    print(f"case {case}: generated lengths {sorted(lengths)}")


# ------------------------------------------------------------------------------------------------ routes
def test_eager_and_graph_replay_give_the_same_bits(dev):
    m, cases, _, _ = _cases(dev)
    ids, audio = cases["Apad"]
    kw = dict(audio, num_return_sequences=3, seed=5, share_prompt=True, max_new_tokens=NEW, **SAMPLED, **FLAGS)
    eager, replayed = m.generate(ids, use_graph=False, **kw), m.generate(ids, use_graph=True, **kw)
    assert torch.equal(eager.sequences, replayed.sequences)
    for a, b in zip(eager.logits, replayed.logits):
        assert torch.equal(a, b)
    assert torch.equal(eager.past_key_values.K, replayed.past_key_values.K) and torch.equal(eager.past_key_values.Vt, replayed.past_key_values.Vt)


def routes_ids_difference(m, ids, audio, seed):
    """processors, an eos list and a stop string together, taken from the unshared call's own tokens so that they bite"""
    from tests import _stop_ref as R

    S0 = ids.shape[1]
    base = dict(num_return_sequences=3, seed=seed, repetition_penalty=1.3, no_repeat_ngram_size=2, **SAMPLED)
    plain = m.generate(ids, share_prompt=False, max_new_tokens=NEW, **audio, **base)
    new = plain[0, S0:].tolist()
    used = set(plain.flatten().tolist())
    free = [i for i in range(1, 1023) if i not in used][:1]
    pieces = {}
    for i, s in ((new[3], "Hel"), (new[4], "lo"), (new[5], " world")):
        pieces.setdefault(i, s)
    tok = R.tiny_tokenizer(pieces)
    stop = dict(eos_token_id=free + [plain[1, S0 + 7].item()], pad_token_id=0, stop_strings=["lo w"], tokenizer=tok)
    a, b = _pair(m, ids, audio, **base, **stop)
    diff = _first_difference(a, b, S0)
    if diff is None:
        assert b.sequences.shape[1] <= S0 + NEW and bool((b.sequences[:, S0:] == 0).any()), "neither the eos list nor the stop string ended a row: the case is toothless"
    return diff


def test_processors_eos_list_and_stop_string_give_the_ids_of_the_unshared_call(dev):
    m, cases, _, _ = _cases(dev)
    ids, audio = cases["Apad"]
    diff = routes_ids_difference(m, ids, audio, SEED_ROUTES)
    assert diff is None, f"seed {SEED_ROUTES}: {diff}"


# ------------------------------------------------------------------------------------------------ off means off
def test_off_means_off(dev, monkeypatch):
    from audio_flamingo_amd import _lib

    m, cases, _, _ = _cases(dev)
    assert type(m).share_prompt_cache is False, "the switch is off by default"
    ids, audio = cases["Apad"]
    names = []
    real_call = _lib.call

    def spy(name, *a):
        names.append(name)
        return real_call(name, *a)

    monkeypatch.setattr(_lib, "call", spy)
    for kw in (dict(num_return_sequences=3, seed=9, **SAMPLED), dict(num_beams=4, num_return_sequences=2)):
        kw = dict(audio, max_new_tokens=NEW, **kw)
        m.generate(ids, **kw)   # one-time initialisation inside the library happens here
        names.clear()
        plain = m.generate(ids, **kw)
        plain_names = list(names)
        for how in (dict(share_prompt=None), dict(share_prompt=False)):
            names.clear()
            got = m.generate(ids, **how, **kw)
            assert torch.equal(got, plain) and m.last_share_stats is None
            assert names == plain_names and "afk_attn_decode_shared" not in names, "with the switch off the call enqueues what it did without the keyword"
        names.clear()
        m.generate(ids, share_prompt=True, **kw)
        assert "afk_attn_decode_shared" in names and "afk_attn_decode_fused" not in names and m.last_share_stats is not None
    # nothing to share: one sequence per row is today's route whatever the keyword says
    names.clear()
    one = m.generate(ids, max_new_tokens=4, share_prompt=True, **audio)
    assert "afk_attn_decode_shared" not in names and m.last_share_stats is None and torch.equal(one, m.generate(ids, max_new_tokens=4, **audio))
    # the class attribute switches the default; an explicit False wins
    m.share_prompt_cache = True
    try:
        names.clear()
        m.generate(ids, max_new_tokens=4, num_beams=4, **audio)
        assert "afk_attn_decode_shared" in names
        names.clear()
        m.generate(ids, max_new_tokens=4, num_beams=4, share_prompt=False, **audio)
        assert "afk_attn_decode_shared" not in names
        # what sharing does not run with falls back silently under the attribute
        names.clear()
        m.beam_on_device = False
        m.generate(ids, max_new_tokens=4, num_beams=4, **audio)
        assert "afk_attn_decode_shared" not in names and m.last_share_stats is None
    finally:
        del m.share_prompt_cache
        if "beam_on_device" in m.__dict__:
            del m.beam_on_device


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals_name_the_combination(dev, monkeypatch):
    from transformers.generation.stopping_criteria import MaxLengthCriteria, StoppingCriteriaList

    from audio_flamingo_amd import exact
    from audio_flamingo_amd._lib import AfkError

    m, cases, _, _ = _cases(dev)
    ids, audio = cases["A"]
    sampled = dict(audio, max_new_tokens=4, num_return_sequences=2, share_prompt=True, **SAMPLED)
    with pytest.raises(AfkError, match=r"share_prompt=True\) with use_cache=False"):
        m.generate(ids, use_cache=False, **sampled)
    with pytest.raises(AfkError, match=r"share_prompt=True\) with logits_processor= / stopping_criteria= / streamer="):
        m.generate(ids, stopping_criteria=StoppingCriteriaList([MaxLengthCriteria(ids.shape[1] + 2)]), **sampled)
    one = m.generate(ids, max_new_tokens=2, return_dict_in_generate=True, **audio)
    # a passed cache refuses more than one continuation per row itself, in front of decode_share.resolve: that message names the combination
    with pytest.raises(AfkError, match=r"generate\(past_key_values=\.\.\.\) with num_return_sequences > 1"):
        m.generate(one.sequences, past_key_values=one.past_key_values, **{k: v for k, v in sampled.items() if not k.startswith("input_features")})
    m.beam_on_device = False
    try:
        with pytest.raises(AfkError, match=r"share_prompt=True\) with the host beam loop"):
            m.generate(ids, max_new_tokens=4, num_beams=4, share_prompt=True, **audio)
    finally:
        del m.beam_on_device
    with pytest.raises(AfkError, match=r"share_prompt=True\) with the host beam loop"):   # 17 beams: outside afk_beam_step's caps (and the kernel's 16 copies)
        m.generate(ids, max_new_tokens=4, num_beams=17, share_prompt=True, **audio)
    with pytest.raises(AfkError, match=r"share_prompt=True\) with a geometry or row count outside the batched decode chain"):
        m.generate(ids, **dict(sampled, num_return_sequences=33))   # 33 rows: above the chain's cap of 32
    m.decode_chain = False
    try:
        with pytest.raises(AfkError, match=r"share_prompt=True\) with a geometry or row count outside the batched decode chain"):
            m.generate(ids, **sampled)
    finally:
        del m.decode_chain
    # prompt-lookup decoding runs one greedy sequence: decode_lookup.resolve comes first and names the combination
    with pytest.raises(AfkError, match=r"generate\(prompt_lookup_num_tokens=\.\.\.\) with num_beams > 1"):
        m.generate(ids, max_new_tokens=4, num_beams=4, share_prompt=True, prompt_lookup_num_tokens=3, **audio)
    # AFK_EXACT_FP32=1: refused for copies and for beams, in front of the exact-fp32 greedy branch and the host beam loop; under the class attribute the
    # call falls back to that host loop silently
    with monkeypatch.context() as mp:
        mp.setattr(exact, "ENABLED", True)
        with pytest.raises(AfkError, match=r"share_prompt=True\) with AFK_EXACT_FP32=1"):
            m.generate(ids, **sampled)
        with pytest.raises(AfkError, match=r"share_prompt=True\) with AFK_EXACT_FP32=1"):
            m.generate(ids, max_new_tokens=4, num_beams=2, share_prompt=True, **audio)
        m.share_prompt_cache = True
        try:
            out = m.generate(ids, max_new_tokens=2, num_beams=2, **audio)
        finally:
            del m.share_prompt_cache
        assert out.shape == (ids.shape[0], ids.shape[1] + 2) and m.last_share_stats is None
    with pytest.raises(ValueError, match="share_prompt"):
        m.generate(ids, **dict(sampled, share_prompt="yes"))
    assert m.last_share_stats is None

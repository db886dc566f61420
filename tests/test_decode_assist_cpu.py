"""CPU: assisted decoding's host code.  decode_assist.resolve - the keyword, the assistant's generation config, the value checks, every refusal, the silent
fall-backs of the class defaults in decode_share / decode_w8 / decode_cfg - which is pure; the staging rule as tests/_assist_ref.py restates it (the GPU
tests hold afk_assist_stage to that restatement exactly) against decode_assist.kept; and a host simulation of the whole step for scripted models, which must
emit the target's greedy ids whatever the draft model says.

The simulation tests and test_stage_restatement_* run tests/_assist_ref.py alone: they specify the reference the GPU tests compare with and touch no project
code, so they say nothing about generate().  What guards the draft model's extra pass in generate() is the GPU assertion of
tests/test_decode_assist_gpu.py::test_same_weights_every_draft_is_accepted (rejecting == 0 and accepted == emitted - 1 - steps)."""
import itertools
import types

import numpy as np
import pytest

from tests import _assist_ref as R
from tests import _lookup_ref as L


def _assistant(k=None):
    return types.SimpleNamespace(generation_config=None if k is None else types.SimpleNamespace(num_assistant_tokens=k))


def test_resolve_off_defaults_and_values():
    from audio_flamingo_amd import decode_assist as A
    from audio_flamingo_amd._lib import AfkError

    assert A.resolve(None) is None and A.resolve(None, 7) is None and A.resolve(None, 0, do_sample=True, batch_size=4) is None   # off: nothing is looked at
    a = _assistant()
    assert A.resolve(a) == A.AssistSpec(a, 5) and A.DEFAULT_K == 5
    assert A.resolve(_assistant(9)).k == 9 and A.resolve(_assistant(9), 3).k == 3      # the assistant's generation config; an explicit keyword wins
    assert A.resolve(_assistant(20)).k == 20                                             # the reference's own default passes
    assert A.resolve(a, 1).k == 1 and A.resolve(a, 31).k == 31 and A.MAX_K == 31
    for bad in (0, -1):
        with pytest.raises(ValueError, match="num_assistant_tokens"):
            A.resolve(a, bad)
    with pytest.raises(ValueError, match="num_assistant_tokens"):
        A.resolve(_assistant(0))
    for bad in (2.0, "3", True, [3]):
        with pytest.raises(ValueError, match="integer"):
            A.resolve(a, bad)
    with pytest.raises(AfkError, match="num_assistant_tokens=32.*at most 31"):
        A.resolve(a, 32)
    with pytest.raises(AfkError, match="at most 31"):
        A.resolve(_assistant(40))
    with pytest.raises(ValueError, match="assisted generate is only supported for batch_size = 1"):
        A.resolve(a, 3, batch_size=2)
    # the position limit of either model: prompt + max_new_tokens + k + 1 positions, refused before anything runs
    fits = dict(prompt_len=100, max_new_tokens=20, max_positions=(124, 124))
    assert A.resolve(a, 3, **fits).k == 3 and A.resolve(a, 3, prompt_len=100, max_new_tokens=20).k == 3
    with pytest.raises(AfkError, match=r"prompt 100 \+ max_new_tokens 20 \+ 5 drafted positions exceed the target's max_position_embeddings 124"):
        A.resolve(a, 4, **fits)
    with pytest.raises(AfkError, match="the assistant's max_position_embeddings 123"):
        A.resolve(a, 3, **dict(fits, max_positions=(4096, 123)))


def test_resolve_refusals_name_the_combination():
    from audio_flamingo_amd import decode_assist as A
    from audio_flamingo_amd._lib import AfkError

    a = _assistant()
    refusals = [(dict(do_sample=True), "do_sample=True"), (dict(num_beams=2), "num_beams > 1"), (dict(copies=2), "num_return_sequences > 1"),
                (dict(use_cache=False), "use_cache=False"), (dict(exact_fp32=True), "AFK_EXACT_FP32=1"), (dict(processors=True), "logits processors"),
                (dict(hooks=True), "stopping_criteria= / streamer="), (dict(stop_strings=True), "stop_strings="),
                (dict(output_object=True), "return_dict_in_generate"), (dict(past=True), "past_key_values="), (dict(share_prompt=True), "share_prompt=True"),
                (dict(guidance=True), "guidance_scale="), (dict(decode_weights="fp8"), "decode_weights='fp8'"), (dict(lookup=True), "prompt_lookup_num_tokens=")]
    for kw, word in refusals:
        with pytest.raises(AfkError, match="assistant_model.*" + word.replace("(", r"\(")):
            A.resolve(a, 3, **kw)
        assert A.resolve(None, 3, **kw) is None
    # what is only a default, or switched off by keyword, refuses nothing
    assert A.resolve(a, 3, share_prompt=None).k == 3 and A.resolve(a, 3, share_prompt=False).k == 3
    assert A.resolve(a, 3, decode_weights=None).k == 3 and A.resolve(a, 3, decode_weights="bf16").k == 3
    # the assistant itself: its class, its device, its vocabulary - both numbers named
    with pytest.raises(AfkError, match="assistant_model.*AudioFlamingo3ForConditionalGeneration.*object"):
        A.resolve(object(), 3, is_model=False)
    with pytest.raises(AfkError, match="assistant_model.*AudioFlamingo3ForConditionalGeneration"):
        A.resolve(object(), 3, is_model=False, lookup=True)   # the combination tests/test_decode_lookup_gpu.py asserts
    with pytest.raises(AfkError, match="device"):
        A.resolve(a, 3, same_device=False)
    ok = (1024, 1024, 1023)
    assert A.resolve(a, 3, target_vocab=ok, assistant_vocab=ok).k == 3
    for other, word in (((1088, 1024, 1023), r"embedding rows \(1088\).*\(1024\)"), ((1024, 960, 1023), r"lm_head rows \(960\).*\(1024\)"),
                        ((1024, 1024, 7), r"audio_token_id \(7\).*\(1023\)")):
        with pytest.raises(AfkError, match=word):
            A.resolve(a, 3, target_vocab=ok, assistant_vocab=other)


def test_the_class_defaults_fall_back_silently_and_the_keywords_refuse():
    from audio_flamingo_amd import decode_cfg, decode_share, decode_w8
    from audio_flamingo_amd._lib import AfkError

    assert decode_w8.resolve(None, "fp8", assist=True) is False and decode_w8.resolve(None, "fp8") is True and decode_w8.resolve("fp8", assist=False) is True
    with pytest.raises(AfkError, match="assistant_model="):
        decode_w8.resolve("fp8", assist=True)
    assert decode_share.resolve(None, True, copies=3, assist=True) is None and decode_share.resolve(None, True, copies=3) is not None
    assert decode_share.resolve(True, copies=3, assist=False) is not None
    with pytest.raises(AfkError, match="assistant_model="):
        decode_share.resolve(True, copies=3, assist=True)
    assert decode_cfg.resolve(None, batch_size=1, assist=True) is None and decode_cfg.resolve(1.0, batch_size=1, assist=True) is None
    assert decode_cfg.resolve(2.0, batch_size=1, assist=False) is not None
    with pytest.raises(AfkError, match="assistant_model="):
        decode_cfg.resolve(2.0, batch_size=1, assist=True)


EOS = (7, 99)


@pytest.mark.parametrize("drafts,eos,budget,done,want", [
    ([7, 1, 2, 3], EOS, None, False, 1),      # eos first: it stays, alone
    ([1, 2, 99, 3], EOS, None, False, 3),     # eos in the middle: cut behind it
    ([1, 2, 3, 7], EOS, None, False, 4),      # eos last
    ([1, 2, 3, 4], EOS, None, False, 4),      # no eos
    ([1, 2, 3, 4], (), None, False, 4),
    ([1, 2, 3, 4], EOS, 0, False, 0),         # emitted == max_new - 1: only the one token every step emits is left
    ([1, 2, 3, 4], EOS, 1, False, 1),
    ([7, 2, 3, 4], EOS, 1, False, 1),
    ([1, 7, 3, 4], EOS, 1, False, 1),         # the budget cuts in front of the eos
    ([1, 7, 3, 4], EOS, 3, False, 2),
    ([1, 2, 3, 4], EOS, -2, False, 0),
    ([1, 2, 3, 4], EOS, None, True, 0),       # done
    ([7], EOS, 5, True, 0),
])
def test_the_staging_rule(drafts, eos, budget, done, want):
    from audio_flamingo_amd import decode_assist as A

    assert R.kept(drafts, eos, budget, done) == want
    assert A.kept(drafts, eos, budget, done) == want


def test_the_two_statements_of_the_rule_agree_everywhere():
    from audio_flamingo_amd import decode_assist as A

    for k in (1, 2, 4):
        for drafts in itertools.product((1, 7, 9), repeat=k):
            for eos in ((), (7,), (7, 9)):
                for budget in (None, -1, 0, 1, 2, 5):
                    for done in (False, True):
                        assert A.kept(list(drafts), eos, budget, done) == R.kept(list(drafts), eos, budget, done), (drafts, eos, budget, done)


def test_stage_restatement_rows_positions_and_key_ranges():
    ids = np.array([5, 6, 7, 8, 0, 0, 0, 0], dtype=np.int32)
    draft = np.zeros(20, dtype=np.int64)
    draft[9:13] = [11, 99, 12, 13]
    state = np.array([2, 10, 9, 7], dtype=np.int32)
    st = L.new_status(4, emitted=2)
    out = R.stage(ids, st, state, draft, 4, 10, eos=(99,))
    assert st[L.N_CAND] == 2 and out["cand"].tolist() == [11, 99, 8, 8] and out["rows"].tolist() == [8, 11, 99, 8, 8]
    assert out["pos"].tolist() == [7, 8, 9, 10, 11] and out["krange"].tolist() == [[2, 10], [2, 11], [2, 12], [2, 13], [2, 14]]
    st = L.new_status(4, emitted=8)
    assert R.stage(ids, st, state, draft, 4, 10)["cand"].tolist() == [11, 8, 8, 8] and st[L.N_CAND] == 1
    st = L.new_status(4, emitted=9)
    assert R.stage(ids, st, state, draft, 4, 10)["cand"].tolist() == [8] * 4 and st[L.N_CAND] == 0
    st = L.new_status(4, emitted=2, done=1)
    assert R.stage(ids, st, state, draft, 4, 10)["rows"].tolist() == [8] * 5 and st[L.N_CAND] == 0
    dstate, tok = R.begin(ids, L.new_status(4), state, 8)
    assert dstate.tolist() == state.tolist() and tok == 7   # id 8 clamped to the vocabulary


def _chain(seed, vocab=50):
    """a scripted greedy model: the next id is a fixed function of the last two ids and the length"""
    return lambda hist: (hist[-1] * 31 + hist[-2] * 17 + len(hist) * seed + seed) % vocab


@pytest.mark.parametrize("k", [1, 2, 3, 5, 8])
def test_simulated_step_emits_the_targets_greedy_ids(k):
    """every mix of accepted and rejected rounds: a draft model that is the target (all accepted), one that never agrees, and ones that agree on a schedule -
    the ids are the target's plain greedy ids in every case, for every budget, with and without an eos id inside the span"""
    target = _chain(3)
    prompt = [4, 9, 2]

    def plain(max_new, eos=()):
        hist, out = list(prompt), []
        while len(out) < max_new:
            out.append(target(hist))
            hist.append(out[-1])
            if out[-1] in eos:
                break
        return out

    never = lambda hist: (target(hist) + 1) % 50
    schedules = [lambda hist, p=p: target(hist) if (len(hist) % p) else never(hist) for p in (2, 3, 4, 7)]
    gold = plain(24)
    seen = set()
    for max_new in (1, 2, 3, k, k + 1, k + 2, 12, 24):
        for eos in ((), (gold[5],), (gold[0],), (gold[11], 1000)):
            want = plain(max_new, eos)
            for name, draft in [("same", target), ("never", never)] + [(f"schedule{i}", s) for i, s in enumerate(schedules)]:
                got, stats = R.simulate(prompt, target, draft, k, max_new, eos)
                assert got == want, (k, max_new, eos, name)
                assert stats["drafted"] == k * stats["steps"]
                if name == "same" and not eos:
                    assert stats["rejecting"] == 0 and stats["accepted"] == len(got) - 1 - stats["steps"], stats
                if name == "never" and max_new > 2 and not eos:
                    assert stats["accepted"] == 0 and stats["steps"] == max_new - 1 and stats["rejecting"] >= stats["steps"] - 1, stats
                if name.startswith("schedule") and max_new == 24 and not eos:
                    seen.add((stats["accepted"] > 0, stats["rejecting"] > 0))
    assert (True, True) in seen, "a schedule must both accept and reject"


def test_the_simulation_sees_a_draft_cache_with_a_hole():
    """(the reference alone: this shows the simulation's own assertion, not generate() - the GPU test of the same-weights assistant guards that)
    without the pass behind the last draft the draft model's cache lacks that draft's keys whenever every draft is accepted: the simulation's draft
    model refuses to run behind a hole.  With the pass it never meets one; a draft model that is never fully accepted does not need it."""
    target = _chain(3)
    never = lambda hist: (target(hist) + 1) % 50
    want, _ = R.simulate([4, 9, 2], target, target, 3, 12)
    with pytest.raises(AssertionError, match="hole"):
        R.simulate([4, 9, 2], target, target, 3, 12, extra_pass=False)
    assert R.simulate([4, 9, 2], target, never, 3, 12, extra_pass=False)[0] == want

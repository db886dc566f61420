"""CPU: the restatement of prompt-lookup decoding's two launches (tests/_lookup_ref.py) against the reference's own code - the draft rule against
PromptLookupCandidateGenerator.get_candidates, exactly, on seeded histories; the accept rule against the tensor expression of _assisted_decoding's greedy branch -
then decode_lookup.resolve(): config pickup, the reference's ValueErrors, every refusal; the host route's own draft rule; and the two symbols in the header and
the library."""
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import _lookup_ref as R

N_HISTORIES = 2400


def _histories(seed, count):
    gen = np.random.default_rng(seed)
    for _ in range(count):
        vocab = int(gen.integers(2, 10))
        n = int(gen.integers(1, 41))
        hist = gen.integers(0, vocab, size=n).tolist()
        k, ngram = int(gen.integers(1, 11)), int(gen.integers(1, 5))
        eos = tuple(sorted(set(gen.integers(0, vocab, size=int(gen.integers(0, 3))).tolist())))
        yield hist, k, ngram, eos


def test_draft_rule_equals_the_reference_class():
    from transformers.generation.candidate_generator import PromptLookupCandidateGenerator

    some = none = 0
    for hist, k, ngram, eos in _histories(11, N_HISTORIES):
        gen = PromptLookupCandidateGenerator(eos_token_id=torch.tensor(eos) if eos else None, num_output_tokens=k, max_matching_ngram_size=ngram, max_length=10 ** 9)
        ids = torch.tensor([hist])
        want = gen.get_candidates(ids)[0][0, len(hist):].tolist()
        got = R.candidates(hist, k, ngram, eos)
        assert got == want, (hist, k, ngram, eos)
        some += bool(want)
        none += not want
    print("histories with candidates", some, "without", none)
    assert some >= N_HISTORIES / 3 and none > 0


def test_host_route_draft_rule_equals_the_restatement():
    from audio_flamingo_amd import decode_lookup as D

    for hist, k, ngram, eos in _histories(12, 800):
        assert D.candidates(hist, k, ngram, eos) == R.candidates(hist, k, ngram, eos)
        assert D.candidates(hist, k, ngram, eos, budget=2) == R.candidates(hist, k, ngram, eos)[:2]
        assert D.candidates(hist, k, ngram, eos, budget=0) == []


def test_draft_restatement_edges():
    st4 = np.array([0, 8, 7, 7], dtype=np.int32)
    # a match only at the tail: the trailing window has no continuation
    assert R.candidates([1, 2, 3, 4], 3, 2) == []
    # two matches: the leftmost wins, the longer n-gram first
    assert R.candidates([5, 6, 1, 9, 5, 6, 2, 8, 5, 6], 2, 2) == [1, 9]
    assert R.candidates([7, 6, 1, 9, 5, 6, 2, 8, 5, 6], 2, 2) == [2, 8]      # the 2-gram (5, 6) only matches at 4; g = 1 is never tried
    # a continuation shorter than k at the end of the history
    assert R.candidates([3, 4, 3], 5, 1) == [4, 3]
    # an eos as the first candidate: none, and no second match is tried
    assert R.candidates([3, 9, 1, 3, 7, 2, 3], 3, 1, eos=(9,)) == []
    assert R.candidates([3, 7, 9, 3, 5, 2, 3], 3, 1, eos=(9,)) == [7]
    # the budget crop, done
    ids = np.array([3, 7, 1, 3, 5, 2, 3, 0, 0, 0, 0], dtype=np.int32)
    for emitted, want in ((1, 3), (7, 2), (8, 1), (9, 0)):
        st = R.new_status(7, emitted=emitted)
        d = R.draft(ids, st, st4, k=3, ngram=1, max_new=10)
        assert st[R.N_CAND] == want and d["cand"].tolist() == [7, 1, 3][:want] + [3] * (3 - want)
        assert d["rows"].tolist() == [3] + d["cand"].tolist() and d["pos"].tolist() == [7, 8, 9, 10] and d["krange"].tolist() == [[0, 8], [0, 9], [0, 10], [0, 11]]
    st = R.new_status(7, done=1)
    assert R.draft(ids, st, st4, k=3, ngram=1, max_new=10)["cand"].tolist() == [3, 3, 3] and st[R.N_CAND] == 0


def test_accept_rule_equals_the_reference_expression():
    """transformers/generation/utils.py:3771-3779, the greedy branch of _assisted_decoding (inline in its loop, restated here with its own tensor operations):
    selected_tokens = new_logits.argmax(-1); n_matches = ((~(candidate_new_tokens == selected_tokens[:, :-1])).cumsum(-1) < 1).sum(); valid_tokens =
    selected_tokens[:, : n_matches + 1]"""
    gen = np.random.default_rng(21)
    seen = set()
    for _ in range(600):
        V, n_cand, k = int(gen.integers(2, 6)), int(gen.integers(0, 8)), 8
        logits = gen.standard_normal((k + 1, V)).astype(np.float32)
        sel = logits.argmax(-1)
        cand = np.where(gen.random(k) < 0.75, sel[:k], gen.integers(0, V, size=k)).astype(np.int32)
        new_logits = torch.from_numpy(logits[None, :n_cand + 1])
        selected_tokens = new_logits.argmax(dim=-1)
        candidate_new_tokens = torch.from_numpy(cand[None, :n_cand].astype(np.int64))
        n_matches = int(((~(candidate_new_tokens == selected_tokens[:, :-1])).cumsum(dim=-1) < 1).sum())
        valid_tokens = selected_tokens[:, : n_matches + 1]
        ids, tokens = np.zeros(40, dtype=np.int32), np.zeros(30, dtype=np.int64)
        st, state = R.new_status(10), np.array([0, 11, 10, 10], dtype=np.int32)
        st[R.N_CAND] = n_cand
        R.accept(logits, cand, ids, tokens, st, state, max_new=30)
        e = n_matches + 1
        assert st[R.N_MATCH] == n_matches and st[R.EMITTED] == 1 + e and st[R.LEN] == 10 + e and ids[10:10 + e].tolist() == valid_tokens[0].tolist()
        assert tokens[1:1 + e].tolist() == valid_tokens[0].tolist() and state.tolist() == [0, 11 + e, 10 + e, 10 + e] and st[R.ACCEPTED] == n_matches
        seen.add("none" if n_matches == 0 and n_cand else "all" if n_matches == n_cand and n_cand else "part" if n_cand else "empty")
    assert seen == {"none", "all", "part", "empty"}


def test_accept_restatement_edges():
    z = np.full((3, 5), -1.0, dtype=np.float32)
    assert R.argmax_row(np.array([1.0, 3.0, 3.0, np.nan])) == 1 and R.argmax_row(np.array([-np.inf, -np.inf])) == 0 and R.argmax_row(np.array([np.nan, np.nan])) == 0
    assert R.argmax_row(np.array([np.nan, -np.inf, -5.0])) == 2 and R.argmax_row(np.array([0.0, np.inf, np.inf])) == 1
    z[0, 2], z[1, 4], z[2, 1] = 1, 1, 1      # sel = [2, 4, 1]
    # an eos on an accepted row cuts the step there; the budget end; done: nothing moves
    for cand, eos, max_new, want, done in (([2, 4], (4,), 9, [2, 4], 1), ([2, 4], (1,), 9, [2, 4, 1], 1), ([2, 4], (), 9, [2, 4, 1], 0), ([2, 4], (), 3, [2, 4], 1),
                                           ([2, 0], (), 9, [2, 4], 0), ([0, 4], (), 9, [2], 0)):
        ids, tokens, st, state = np.zeros(16, dtype=np.int32), np.zeros(9, dtype=np.int64), R.new_status(4), np.array([1, 5, 4, 3], dtype=np.int32)
        st[R.N_CAND] = 2
        sel = R.accept(z, np.array(cand, dtype=np.int32), ids, tokens, st, state, max_new, eos)
        assert sel.tolist() == [2, 4, 1] and ids[4:4 + len(want)].tolist() == want and not ids[4 + len(want):].any() and st[R.DONE] == done
        assert st[R.EMITTED] == 1 + len(want) and state.tolist() == [1, 5 + len(want), 4 + len(want), 3 + len(want)] and st[R.STEPS] == 1
        before = (ids.copy(), tokens.copy(), st.copy(), state.copy())
        if done:
            assert R.accept(z, np.array(cand, dtype=np.int32), ids, tokens, st, state, max_new, eos) is None
            assert all(np.array_equal(a, b) for a, b in zip(before, (ids, tokens, st, state)))


# ---------------------------------------------------------------------------------------------- resolver
def test_resolve_off_defaults_and_the_generation_config():
    from audio_flamingo_amd import decode_lookup as D

    assert D.resolve() is None and D.resolve(max_matching_ngram_size=3) is None
    assert D.resolve(4) == D.LookupSpec(k=4, ngram=2) and D.resolve(4, 3) == D.LookupSpec(4, 3)
    gc = SimpleNamespace(prompt_lookup_num_tokens=5, max_matching_ngram_size=None)
    assert D.resolve(generation_config=gc) == D.LookupSpec(5, 2)
    assert D.resolve(2, generation_config=SimpleNamespace(prompt_lookup_num_tokens=5, max_matching_ngram_size=4)) == D.LookupSpec(2, 4)
    from transformers import GenerationConfig

    assert D.resolve(generation_config=GenerationConfig(prompt_lookup_num_tokens=3, max_matching_ngram_size=1)) == D.LookupSpec(3, 1)
    assert D.resolve(generation_config=GenerationConfig()) is None


def test_resolve_raises_where_the_reference_does():
    from transformers.generation.candidate_generator import PromptLookupCandidateGenerator

    from audio_flamingo_amd import decode_lookup as D

    for k, n in ((0, 2), (-1, 2), (3, 0), (3, -2)):
        with pytest.raises(ValueError, match="Invalid max_matching_ngram_size or num_output_tokens"):
            D.resolve(k, n)
    for k, n in ((0, 2), (3, -2)):   # the class itself, same message
        with pytest.raises(ValueError, match="Invalid max_matching_ngram_size or num_output_tokens"):
            PromptLookupCandidateGenerator(num_output_tokens=k, max_matching_ngram_size=n)
    with pytest.raises(ValueError, match="assisted generate is only supported for batch_size = 1"):
        D.resolve(3, batch_size=2)
    with pytest.raises(ValueError, match="integers"):
        D.resolve(2.5)


def test_resolve_refusals_name_the_combination():
    from audio_flamingo_amd import decode_lookup as D
    from audio_flamingo_amd._lib import AfkError

    for how, what in ((dict(do_sample=True), "do_sample=True"), (dict(num_beams=2), "num_beams > 1"), (dict(use_cache=False), "use_cache=False"),
                      (dict(exact_fp32=True), "AFK_EXACT_FP32=1"), (dict(processors=True), "logits processors"), (dict(hooks=True), "streamer="),
                      (dict(stop_strings=True), "stop_strings="), (dict(output_object=True), "return_dict_in_generate")):
        with pytest.raises(AfkError, match=r"prompt_lookup_num_tokens=\.\.\.\) with [^:]*" + re.escape(what)):
            D.resolve(3, **how)
        assert D.resolve(**how) is None   # off: nothing is refused
    with pytest.raises(AfkError, match="at most 31 drafted tokens"):
        D.resolve(32)
    with pytest.raises(AfkError, match="n-grams of at most 16"):
        D.resolve(3, 17)


def test_both_launches_are_declared_and_exported():
    from audio_flamingo_amd import _lib
    from audio_flamingo_amd import decode_lookup as D

    protos = _lib.parse_header()
    assert len(protos["afk_lookup_draft"][1]) == 20 and len(protos["afk_lookup_accept"][1]) == 16
    assert protos["afk_lookup_draft"][2][-1] == "stream" and protos["afk_lookup_accept"][2][:4] == ["logits", "ld_logits", "V", "M"]
    src = open(_lib.HEADER_PATH).read()
    for name, val in (("AFK_LOOKUP_MAX_K", D.MAX_K), ("AFK_LOOKUP_MAX_NGRAM", D.MAX_NGRAM), ("AFK_LOOKUP_STATUS_WORDS", D.STATUS_WORDS), ("AFK_LOOKUP_WS_WORDS", D.WS_WORDS)):
        assert f"#define {name} {val}\n" in src
    assert (D.LEN, D.EMITTED, D.DONE, D.N_CAND, D.STEPS, D.ACCEPTED, D.REJECTING, D.N_MATCH) == (R.LEN, R.EMITTED, R.DONE, R.N_CAND, R.STEPS, R.ACCEPTED, R.REJECTING, R.N_MATCH)
    lib = _lib.load()   # binds every declared symbol: a missing export raises here
    assert lib.afk_lookup_draft.argtypes == protos["afk_lookup_draft"][1] and lib.afk_lookup_accept.argtypes == protos["afk_lookup_accept"][1]

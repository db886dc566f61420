"""CPU: the integer restatement of afk_decode_stop's rule (tests/_stop_ref.py) against the reference's own StopStringCriteria and EosTokenCriteria, exactly, and
decode_stop.resolve() - eos forms, pad default, config pickup, the reference's ValueError, the refusals."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import _stop_ref as R

# tokens of the grid's tokenizer: whole strings, their fragments, multi-byte characters and their halves
PIECES = {0: "a", 1: "b", 2: "c", 3: "ab", 4: "bc", 5: "abc", 6: "\n", 7: "\n\n", 8: "User", 9: ":", 10: "er:", 11: " ", 12: "Us", 13: "é", 14: b"\xc3", 15: b"\xa9",
          16: "aa", 17: "aaa", 18: "x", 19: "stop!", 20: "st", 21: "op", 22: "!x", 23: "日", 24: b"\xe6\x97", 25: b"\xa5"}
BEYOND = 5000   # an id above the table's rows: clamped to the dummy row
# (stop strings, ids the random rows draw from)
SETS = {
    "single character": (["\n"], [6, 7, 0, 1, 18, 11, 9, BEYOND]),
    "ends mid-token": (["sto"], [19, 20, 21, 22, 18, 0, BEYOND]),
    "multi-byte": (["é", "日"], [13, 14, 15, 23, 24, 25, 0, 18]),
    "different lengths": (["abc", "\n\n", "User:"], [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 12]),
    "several end overlaps": (["aa"], [0, 16, 17, 1, 18, BEYOND]),
}
LENGTHS = (1, 2, 3, 5, 9)
ROWS = 400


@pytest.fixture(scope="module")
def tokenizer():
    return R.tiny_tokenizer(PIECES, vocab_size=64)


def test_tiny_tokenizer_places_the_pieces(tokenizer):
    vocab = tokenizer.get_vocab()
    assert len(vocab) == 64 + 256 and sorted(vocab.values()) == list(range(320))
    assert tokenizer.decode([8, 9]) == "User:" and tokenizer.decode([14, 15]) == "é" and tokenizer.decode([24, 25]) == "日"
    assert tokenizer("ax", add_special_tokens=False)["input_ids"] == [0, 18] and tokenizer("d", add_special_tokens=False)["input_ids"] == [64 + ord("d")]


def test_restatement_equals_the_reference_classes(tokenizer):
    from transformers.generation.stopping_criteria import EosTokenCriteria, StopStringCriteria

    gen = np.random.default_rng(5)
    hits = total = 0
    for name, (strings, pool) in SETS.items():
        crit = StopStringCriteria(tokenizer=tokenizer, stop_strings=strings)
        tab = R.table_of(crit)
        assert tab["table"].shape[1] == tab["S"] * (tab["P"] + tab["E"]) + 1
        if name == "several end overlaps":
            assert tab["E"] >= 2
        eos = (int(pool[0]), int(pool[-1]))
        eos_crit = EosTokenCriteria(list(eos))
        set_hits = 0
        for L in LENGTHS:   # 1, 2, 3: histories shorter than W for the longer strings
            ids = torch.from_numpy(gen.choice(np.asarray(pool), size=(ROWS, L)))
            want = crit(ids, None).tolist()
            got = [R.string_match(row, tab) for row in ids.tolist()]
            assert got == want, (name, L)
            assert [int(r[-1]) in eos for r in ids.tolist()] == eos_crit(ids, None).tolist()
            assert [R.judge(r, eos, tab) for r in ids.tolist()] == (crit(ids, None) | eos_crit(ids, None)).tolist()
            set_hits += sum(want)
        print(name, "hits", set_hits, "of", ROWS * len(LENGTHS))
        assert 0 < set_hits < ROWS * len(LENGTHS), name   # every stop set shows both answers
        hits += set_hits
        total += ROWS * len(LENGTHS)
    print("hits", hits, "of", total)
    assert hits >= 0.05 * total


def test_step_bookkeeping_of_the_restatement():
    """pad substitution, stop_at, status and the rerun on the plain-integer model the GPU test compares the kernel with"""
    nxt = np.array([5, 9, 5], dtype=np.int64)
    ids = np.zeros((3, 6), dtype=np.int32)
    stop_at = np.full(3, R.INT_MAX, dtype=np.int32)
    status = np.array([-1, 3], dtype=np.int32)
    R.step(nxt, ids, stop_at, status, 0, S0=2, max_new=4, eos=(9,), pad=1)
    assert stop_at.tolist() == [R.INT_MAX, 0, R.INT_MAX] and status.tolist() == [0, 2] and ids[:, 2].tolist() == [5, 9, 5]
    nxt[:] = (9, 7, 5)
    for _ in range(2):   # the rerun reproduces the state
        R.step(nxt, ids, stop_at, status, 1, S0=2, max_new=4, eos=(9,), pad=1, feed_pad=True)
        assert stop_at.tolist() == [1, 0, R.INT_MAX] and status.tolist() == [1, 1] and ids[:, 3].tolist() == [9, 1, 5] and nxt.tolist() == [9, 1, 5]
    R.step(nxt, ids, stop_at, status, 4, S0=2, max_new=4, eos=(9,), pad=1)
    assert status.tolist() == [1, 1]


# ---------------------------------------------------------------------------------------------- resolver
def test_resolve_eos_forms_and_the_pad_default():
    from audio_flamingo_amd import decode_stop as D

    assert D.resolve() == D.StopSpec((), None, ()) and not D.resolve().device
    for form in (7, [7], (7,), torch.tensor(7), torch.tensor([7])):
        s = D.resolve(eos_token_id=form)
        assert s.eos == (7,) and s.pad == 7 and not s.device          # one id, however it is written, is the scalar case
    for form in ([151645, 151643], (151645, 151643), torch.tensor([151645, 151643])):
        s = D.resolve(eos_token_id=form)
        assert s.eos == (151645, 151643) and s.pad == 151645 and s.device
    assert D.resolve(eos_token_id=[4, 5], pad_token_id=0).pad == 0
    assert D.resolve(pad_token_id=3) == D.StopSpec((), 3, ())
    for bad in (-1, [3, -2], "7", [True], 1.5):
        with pytest.raises(ValueError, match="eos_token_id"):
            D.resolve(eos_token_id=bad)


def test_resolve_takes_the_generation_config_and_a_keyword_wins():
    from audio_flamingo_amd import decode_stop as D

    gc = SimpleNamespace(eos_token_id=[151645, 151643], pad_token_id=151643, stop_strings=["User:"])
    tok = object()
    s = D.resolve(generation_config=gc, tokenizer=tok)
    assert s == D.StopSpec((151645, 151643), 151643, ("User:",)) and s.device
    s = D.resolve(eos_token_id=9, pad_token_id=2, stop_strings="\n\n", tokenizer=tok, generation_config=gc)
    assert s == D.StopSpec((9,), 2, ("\n\n",)) and s.device
    from transformers import GenerationConfig

    s = D.resolve(generation_config=GenerationConfig(eos_token_id=[5, 6]))
    assert s.eos == (5, 6) and s.pad == 5 and s.stop_strings == ()


def test_resolve_stop_strings_need_a_tokenizer_and_the_refusals():
    from audio_flamingo_amd import decode_stop as D
    from audio_flamingo_amd._lib import AfkError

    with pytest.raises(ValueError, match="could not locate a tokenizer"):
        D.resolve(stop_strings=["x"])
    with pytest.raises(ValueError, match="could not locate a tokenizer"):
        D.resolve(generation_config=SimpleNamespace(stop_strings="x"))
    with pytest.raises(AfkError, match=r"generate\(tokenizer=\.\.\.\) is not supported"):
        D.resolve(tokenizer=object())
    with pytest.raises(AfkError, match=r"generate\(tokenizer=\.\.\.\) is not supported"):
        D.resolve(eos_token_id=[1, 2], tokenizer=object(), stop_strings=[])
    for how, what in ((dict(num_beams=2), "num_beams > 1"), (dict(use_cache=False), "use_cache=False"), (dict(exact_fp32=True), "AFK_EXACT_FP32=1")):
        with pytest.raises(AfkError, match=what):
            D.resolve(stop_strings=["x"], tokenizer=object(), **how)
        assert D.resolve(eos_token_id=[1, 2], **how).device   # an eos list alone is refused nowhere
    with pytest.raises(ValueError, match="stop_strings"):
        D.resolve(stop_strings=["x", ""], tokenizer=object())


def test_build_table_reads_the_class(tokenizer):
    from transformers.generation.stopping_criteria import StopStringCriteria

    from audio_flamingo_amd import decode_stop as D

    strings = ["abc", "\n\n", "User:"]
    t = D.build_table(tokenizer, strings)
    c = StopStringCriteria(tokenizer=tokenizer, stop_strings=strings)
    assert torch.equal(t["table"], c.embedding_vec.to(torch.int32)) and t["table"].dtype == torch.int32 and t["table"].is_contiguous()
    assert (t["P"], t["E"], t["S"], t["W"]) == (c.max_valid_positions, c.max_valid_end_lens, 3, 5) and t["target_lens"].tolist() == [3, 2, 5]
    assert t["table"].shape == (64 + 256 + 1, 3 * (t["P"] + t["E"]) + 1)

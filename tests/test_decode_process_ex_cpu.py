"""CPU: the restatement of afk_decode_process_ex's nine-stage contract (tests/_logits_process_ex_ref.py) against the reference's own logits processors chained
in GenerationMixin._get_logits_processor's order, bit for bit, and the resolver of generate()'s five further processor keywords - sequence_bias, bad_words_ids,
min_length, forced_eos_token_id, exponential_decay_length_penalty (audio_flamingo_amd/decode_process.py).  No tolerance anywhere."""
import os
from types import SimpleNamespace

import pytest
import torch

from tests import _logits_process_ex_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _same(logits, ids, S0, t, kw, **more):
    want = R.reference_chain(logits, ids, S0, **kw, **more)
    got = R.restated(logits, ids, t, **kw, **more)
    assert torch.equal(R.bits(got), R.bits(want)), (logits.shape, S0, t, kw, more)
    return want


@pytest.mark.parametrize("V", R.VS)
def test_restatement_equals_the_reference_chain_bit_for_bit(V):
    """all ten processors on, every grid point"""
    n = 0
    for (V_, S0, t) in R.grid():
        if V_ == V:
            _same(*R.case(V, S0, t)[:2], S0, t, R.case(V, S0, t)[2])
            n += 1
    assert n == len(R.S0S) * len(R.TS)


@pytest.mark.parametrize("name", R.EX_KEYS)
def test_each_new_processor_alone(name):
    for (V, S0, t) in R.grid():
        logits, ids, kw = R.case(V, S0, t)
        _same(logits, ids, S0, t, R.alone(kw, name))


def test_grid_holds_what_it_claims():
    assert len(R.grid()) == 64
    logits, ids, kw = R.case(1000, 40, 3)
    sb, bad, eos = kw["sequence_bias"], kw["bad_words_ids"], kw["eos"]
    assert {len(s) for s in sb} == {1, 2, 3, 5, 50} and {len(w) for w in bad} >= {1, 2, 3, 5}
    assert [list(eos[:1])] == bad[:1] and bad[1][-1] == eos[1] and float("inf") in sb.values()
    by_last = {}
    for s, v in sb.items():
        by_last.setdefault(s[-1], []).append(v)
    shared = [v for v in by_last.values() if len(v) >= 3][0][:3]   # the one-id bias, then the 2- and the 3-id sequence (the 50-id one ends there too)
    f = torch.tensor(shared, dtype=torch.float32)
    assert float((f[0] + f[1]) + f[2]) != float(f[0] + (f[1] + f[2]))         # the order of the fp32 sum shows
    for b in range(2):                                                         # rows 0 and 1 end in the tail the sequences were cut from
        hits = [s for s in sb if 2 <= len(s) <= 5 and tuple(ids[b, 43 - (len(s) - 1):].tolist()) == s[:-1]]
        assert len(hits) >= 4 and len(set(ids[b].tolist())) < 12
    row = logits[0]
    assert (R.bits(row) == -2 ** 31).sum() >= 1 and (row == float("-inf")).sum() >= 1 and (row == float("inf")).sum() >= 1
    out = R.restated(logits, ids, 3, **kw)
    assert bool(out.isnan().any())                                             # +inf bias on a -inf logit
    assert len({R.case(33, S0, t)[2]["min_length"] - (S0 + t) for S0 in R.S0S for t in R.TS}) == 2
    assert len({t - R.case(33, S0, t)[2]["decay"][0] for S0 in R.S0S for t in R.TS}) == 2


def test_boundaries_one_step_either_side():
    V, S0 = 256, 5
    for t in (R.MAX_NEW - 2, R.MAX_NEW - 1):
        logits, ids, kw = R.case(V, S0, 3)
        gen = torch.Generator().manual_seed(t)
        ids = torch.cat([ids, ids[:, : t - 3]], 1) if t > 3 else ids
        assert ids.shape[1] == S0 + t
        n = S0 + t
        eos, forced = kw["eos"], kw["forced_eos"]
        # forced EOS: nothing at max_new - 2, the whole row at max_new - 1; a forced id that is suppressed ends at -inf
        out = _same(logits, ids, S0, t, dict(R.OFF, forced_eos=forced, suppress=kw["suppress"]))
        if t == R.MAX_NEW - 1:
            assert forced[1] in kw["suppress"] and out[0, forced[1]] == float("-inf") and out[0, forced[0]] == 0.0
            assert int((out[0] == float("-inf")).sum()) == V - 1
        else:
            assert int((out[0] == float("-inf")).sum()) < V // 2
        # min_length: cur_len = min_length - 1 bans, cur_len = min_length does not
        for ml, banned in ((n + 1, True), (n, False)):
            x = torch.ones_like(logits)
            out = _same(x, ids, S0, t, dict(R.OFF, min_length=ml, eos=eos))
            assert bool((out[:, list(eos)] == float("-inf")).all()) == banned
        # decay: t = start leaves the values, t = start + 1 scales the eos entries (negative and positive alike)
        for start, on in ((t, False), (t - 1, True)):
            x = torch.full_like(logits, -2.0)
            x[:, eos[1]] = 3.0
            x[:, 0] = -0.0
            out = _same(x, ids, S0, t, dict(R.OFF, decay=(start, 1.5), eos=eos))
            assert torch.equal(out[:, list(eos)], x[:, list(eos)] + (x[:, list(eos)].abs() * 0.5 if on else 0))
            assert (int(R.bits(out)[0, 0]) == 0) == on and 0 not in eos          # -0.0 + 0.0 only where the penalty ran
        _same(x, ids, S0, t, dict(R.OFF, decay=(t - 1, 0.5), eos=(eos[0], eos[0])))   # an eos id listed twice is scaled once
        out = _same(x, ids, S0, t, dict(R.OFF, bad_words_ids=[[eos[0]]], eos=eos))   # the eos filter empties the list: the processor still adds its zero bias
        assert int(R.bits(out)[0, 0]) == 0
    # order: the bias stands in front of the penalty, which scales it
    logits, ids, kw = R.case(256, 5, 1)
    i = int(ids[0, 0])
    out = _same(torch.zeros_like(logits), ids, 5, 1, dict(R.OFF, sequence_bias={(i,): 2.0}, penalty=4.0))
    assert float(out[0, i]) == 0.5


# ---------------------------------------------------------------------------------------------- the resolver
def test_resolver_defaults_stay_inactive():
    from audio_flamingo_amd.decode_process import EX_DEFAULTS, ProcessSpec, resolve

    assert not ProcessSpec().active and not ProcessSpec().extended and resolve() == ProcessSpec()
    assert resolve(**EX_DEFAULTS) == ProcessSpec()
    assert not resolve(min_length=5).active                                     # no EOS id known: nothing to ban
    assert resolve(min_length=5, eos_token_id=3).extended and resolve(min_length=5, eos_token_id=3).eos == (3,)
    assert resolve(forced_eos_token_id=4).forced_eos == (4,) and resolve(forced_eos_token_id=[4, 5]).extended   # needs no eos_token_id
    assert resolve(sequence_bias={(1, 2): 1.5}).sequence_bias == (((1, 2), 1.5),) and resolve(sequence_bias=[[[1, 2], 1.5]]).extended
    s = resolve(bad_words_ids=[[7], [3, 4], [3, 4], [8]], eos_token_id=[7, 9])
    assert s.bad_words == ((3, 4), (8,)) and s.extended and s.eos == ()        # [eos] filtered, duplicates once, eos not kept for the launch
    s = resolve(exponential_decay_length_penalty=(3, 1.2), eos_token_id=9)
    assert s.decay == (3, 1.2) and s.eos == (9,) and s.extended
    s = resolve(repetition_penalty=1.3)                                         # the existing five alone: not extended
    assert s.active and not s.extended


def _both_raise(ours, theirs):
    with pytest.raises(ValueError) as a:
        ours()
    with pytest.raises(ValueError) as b:
        theirs()
    assert str(a.value) == str(b.value)


def test_resolver_validates_with_the_reference_messages():
    from transformers import (ExponentialDecayLengthPenalty, ForcedEOSTokenLogitsProcessor, MinLengthLogitsProcessor, NoBadWordsLogitsProcessor,
                              SequenceBiasLogitsProcessor)

    from audio_flamingo_amd.decode_process import pack_sequences, resolve

    for bad in ({}, [], "x", {1: 1.0}, {(1, -2): 1.0}, {(): 1.0}, {(1, 2): 1}, {(1.5,): 1.0}, [[[1, 2], 1]], [[[1, -2], 1.0]], [[[0, 2], 1.0]], [[(1, 2), 1.0]]):
        _both_raise(lambda: resolve(sequence_bias=bad), lambda: SequenceBiasLogitsProcessor(sequence_bias=bad))
    for bad in ([], "x", [3], [[3], 4], [[3, -1]], [[1.5]], {}):
        _both_raise(lambda: resolve(bad_words_ids=bad), lambda: NoBadWordsLogitsProcessor(bad))
    s = resolve(bad_words_ids=[[5]], eos_token_id=5)   # nothing left behind the eos filter: the reference keeps a processor that adds a zero bias
    assert s.bad_words == () and s.extended and pack_sequences((), 7)["group_id"] == [0]
    for bad in (-1, 2.0, "3"):
        _both_raise(lambda: resolve(min_length=bad, eos_token_id=1), lambda: MinLengthLogitsProcessor(bad, 1))
    for bad in ([1, -2], [1.5], -3):
        _both_raise(lambda: resolve(forced_eos_token_id=bad), lambda: ForcedEOSTokenLogitsProcessor(10, bad))
        _both_raise(lambda: resolve(exponential_decay_length_penalty=(1, 1.1), eos_token_id=bad), lambda: ExponentialDecayLengthPenalty((1, 1.1), bad, 4))
    with pytest.raises(ValueError, match="needs an EOS id"):
        resolve(exponential_decay_length_penalty=(1, 1.1))
    for bad in (3, (1,), (1.5, 1.1), (1, "x"), (1, 0.0)):
        with pytest.raises(ValueError, match="exponential_decay_length_penalty"):
            resolve(exponential_decay_length_penalty=bad, eos_token_id=2)
    for empty in (dict(bad_words_ids=[[1], []]), dict(sequence_bias=[[[], 1.0]])):   # the reference accepts an empty sequence and fails on it at the first step
        with pytest.raises(ValueError, match="non-empty"):
            resolve(**empty)


def test_resolver_keyword_wins_over_the_generation_config():
    from transformers import GenerationConfig

    from audio_flamingo_amd.decode_process import resolve

    gc = SimpleNamespace(sequence_bias={(1,): 1.0}, bad_words_ids=[[2, 3]], min_length=9, forced_eos_token_id=4, exponential_decay_length_penalty=(2, 1.1),
                         eos_token_id=[6])
    s = resolve(generation_config=gc)
    assert (s.sequence_bias, s.bad_words, s.min_length, s.forced_eos, s.decay, s.eos) == ((((1,), 1.0),), ((2, 3),), 9, (4,), (2, 1.1), (6,))
    s = resolve(generation_config=gc, sequence_bias={(5,): 2.0}, bad_words_ids=[[8]], min_length=3, forced_eos_token_id=[7], exponential_decay_length_penalty=(1, 1.5))
    assert (s.sequence_bias, s.bad_words, s.min_length, s.forced_eos, s.decay) == ((((5,), 2.0),), ((8,),), 3, (7,), (1, 1.5))
    # a real GenerationConfig that bans a sequence and forces a closing EOS resolves to an active spec
    s = resolve(generation_config=GenerationConfig(bad_words_ids=[[3, 4]], forced_eos_token_id=5))
    assert s.active and s.extended and s.bad_words == ((3, 4),) and s.forced_eos == (5,)
    assert not resolve(generation_config=GenerationConfig()).active


def test_generate_takes_the_five_keywords_with_the_reference_defaults():
    import inspect

    from audio_flamingo_amd.decode_process import EX_DEFAULTS
    from audio_flamingo_amd.modeling import AudioFlamingo3ForConditionalGeneration as Mine

    sig = inspect.signature(Mine.generate)
    assert EX_DEFAULTS == dict(sequence_bias=None, bad_words_ids=None, min_length=0, forced_eos_token_id=None, exponential_decay_length_penalty=None)
    for k, v in EX_DEFAULTS.items():
        assert sig.parameters[k].default == v, k


def test_pack_sequences_groups_by_last_id_in_a_stable_order():
    from audio_flamingo_amd.decode_process import decay_table, pack_sequences

    tb = pack_sequences((((9,), 1.0), ((1, 2, 5), 2.0), ((3, 9), 3.0), ((4, 5), 4.0), ((7, 8, 9), 5.0), ((5,), 6.0)), 10)
    assert tb == dict(group_id=[9, 5], group_l1=[1.0, 6.0], group_off=[0, 2, 4], seq_bias=[3.0, 5.0, 2.0, 4.0], seq_off=[0, 1, 3, 5, 6], ids=[3, 7, 8, 1, 2, 4])
    from transformers import SequenceBiasLogitsProcessor

    _both_raise(lambda: pack_sequences((((1, 12), 1.0), ((10,), 1.0)), 10),
                lambda: SequenceBiasLogitsProcessor({(1, 12): 1.0, (10,): 1.0})(torch.zeros((1, 2), dtype=torch.long), torch.zeros((1, 10))))
    c = decay_table(1, 1.37, 5)
    assert c.dtype == torch.float32 and c.tolist()[:2] == [0.0, 0.0] and torch.equal(c[2:], torch.tensor([1.37 ** k - 1 for k in (1, 2, 3)], dtype=torch.float64).float())


def test_c_abi_declares_and_exports_the_entry():
    """include/afk.h declares afk_decode_process_ex next to afk_decode_process (still 30 arguments); the built library exports both"""
    from audio_flamingo_amd import _lib

    lib = _lib.load()
    assert hasattr(lib, "afk_decode_process_ex") and hasattr(lib, "afk_decode_process")
    protos = _lib.prototypes()
    assert len(protos["afk_decode_process"][1]) == 30
    old, new = protos["afk_decode_process"][2], protos["afk_decode_process_ex"][2]
    assert new[:29] == old[:29] and new[-1] == old[-1] == "stream"
    for name in ("bias_ids", "bias_seq_off", "bias_seq_bias", "bias_group_id", "bias_group_l1", "bias_group_off", "bad_ids", "bad_group_off", "min_length",
                 "forced_eos", "n_forced_eos", "decay", "n_decay", "decay_start", "max_new_tokens"):
        assert name in new, name

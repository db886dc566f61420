"""CPU: the restatement of afk_decode_process's contract (tests/_logits_process_ref.py) against the reference's own logits processors, bit for bit, and the
argument resolver of generate()'s five processor keywords (audio_flamingo_amd/decode_process.py).  No tolerance anywhere: the processing is one IEEE fp32
multiply or divide, or a store of -inf."""
import os
from types import SimpleNamespace

import pytest
import torch

from tests import _logits_process_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("V", R.VS)
def test_restatement_equals_the_reference_classes_bit_for_bit(V):
    n = 0
    for (V_, S0, t, g) in R.grid():
        if V_ != V:
            continue
        logits, ids, kw = R.case(V, S0, t, g)
        want = R.reference_chain(logits, ids, S0, **kw)
        got = R.restated(logits, ids, t, **kw)
        assert torch.equal(R.bits(got), R.bits(want)), (V, S0, t, g, kw)
        n += 1
    assert n == len(R.S0S) * len(R.TS) * len(R.GS)


def test_grid_plants_the_special_values_and_repeats():
    assert len(R.grid()) == 240
    logits, ids, kw = R.case(1000, 40, 3, 3)
    for b in range(R.B):
        row = logits[b]
        assert (row == float("-inf")).sum() == 1 and (R.bits(row) == -2 ** 31).sum() == 1 and ((row == 0) & (R.bits(row) == 0)).sum() >= 1
        assert len(set(ids[b].tolist())) < 12 < ids.shape[1]
    assert {R.case(33, 5, 1, g)[2]["penalty"] for g in R.GS} == set(R.PENALTIES)
    # a history shorter than g bans nothing through the n-gram step
    logits, ids, kw = R.case(256, 2, 0, 7)
    plain = R.restated(logits, ids, 0, **dict(kw, ngram=0))
    assert torch.equal(R.bits(R.restated(logits, ids, 0, **kw)), R.bits(plain))


# ---------------------------------------------------------------------------------------------- the resolver
def test_resolver_defaults_are_inactive():
    from audio_flamingo_amd.decode_process import ProcessSpec, resolve

    spec = resolve()
    assert spec == ProcessSpec() and not spec.active
    assert not resolve(min_new_tokens=5).active                      # no EOS id known: nothing to ban
    assert not resolve(repetition_penalty=1).active                  # the reference builds no processor for 1 / 1.0
    assert resolve(min_new_tokens=5, eos_token_id=7).active and resolve(repetition_penalty=1.05).active and resolve(no_repeat_ngram_size=2).active
    assert resolve(suppress_tokens=[3]).active and resolve(begin_suppress_tokens=[3]).active


def test_resolver_validates_as_the_reference_does():
    from transformers import RepetitionPenaltyLogitsProcessor

    from audio_flamingo_amd.decode_process import resolve

    for bad in (0.0, -1.0, 2, "1.3"):
        with pytest.raises(ValueError) as ours:
            resolve(repetition_penalty=bad)
        with pytest.raises(ValueError) as theirs:
            RepetitionPenaltyLogitsProcessor(bad)
        assert str(ours.value) == str(theirs.value)
    for bad in (-1, 2.0, "2", True):
        with pytest.raises(ValueError):
            resolve(no_repeat_ngram_size=bad)
    for bad in (-1, 1.5):
        with pytest.raises(ValueError):
            resolve(min_new_tokens=bad, eos_token_id=3)
    for name in ("suppress_tokens", "begin_suppress_tokens"):
        with pytest.raises(ValueError):
            resolve(**{name: [1, -2]})
        with pytest.raises(ValueError):
            resolve(**{name: [1.5]})


def test_resolver_eos_int_or_list_and_tensors():
    from audio_flamingo_amd.decode_process import resolve

    assert resolve(min_new_tokens=4, eos_token_id=9).eos == (9,)
    assert resolve(min_new_tokens=4, eos_token_id=[9, 11]).eos == (9, 11)
    assert resolve(min_new_tokens=4, eos_token_id=torch.tensor([9, 11])).eos == (9, 11)
    assert resolve(min_new_tokens=0, eos_token_id=[9, 11]).eos == ()
    s = resolve(suppress_tokens=torch.tensor([5, 6]), begin_suppress_tokens=(7,))
    assert s.suppress == (5, 6) and s.begin_suppress == (7,)


def test_resolver_merges_the_generation_config():
    from audio_flamingo_amd.decode_process import resolve

    gc = SimpleNamespace(repetition_penalty=1.05, no_repeat_ngram_size=3, min_new_tokens=2, suppress_tokens=[4], begin_suppress_tokens=None, eos_token_id=[1, 2])
    s = resolve(generation_config=gc)
    assert (s.penalty, s.ngram, s.min_new_tokens, s.eos, s.suppress, s.begin_suppress) == (1.05, 3, 2, (1, 2), (4,), ())
    s = resolve(repetition_penalty=1.3, suppress_tokens=[8], eos_token_id=5, generation_config=gc)       # an explicit keyword wins
    assert (s.penalty, s.ngram, s.eos, s.suppress) == (1.3, 3, (5,), (8,))
    assert not resolve(generation_config=SimpleNamespace(repetition_penalty=None, no_repeat_ngram_size=None, min_new_tokens=None)).active
    from transformers import GenerationConfig

    s = resolve(generation_config=GenerationConfig(repetition_penalty=1.05, no_repeat_ngram_size=2))
    assert (s.penalty, s.ngram) == (1.05, 2)
    with pytest.raises(ValueError):
        resolve(generation_config=SimpleNamespace(repetition_penalty=-1.0))


def test_generate_takes_the_five_keywords():
    import inspect

    from audio_flamingo_amd.decode_process import DEFAULTS
    from audio_flamingo_amd.modeling import AudioFlamingo3ForConditionalGeneration as Mine

    sig = inspect.signature(Mine.generate)
    for k, v in DEFAULTS.items():
        assert sig.parameters[k].default == v, k


def test_c_abi_declares_and_exports_the_entry():
    """include/afk.h declares afk_decode_process; the built library exports it (_lib derives the argtypes from the header); no CPU fallback"""
    from audio_flamingo_amd import _lib, ops

    lib = _lib.load()
    assert hasattr(lib, "afk_decode_process")
    hdr = open(os.path.join(ROOT, "include", "afk.h")).read()
    decl = hdr[hdr.index("int afk_decode_process("):]
    decl = decl[:decl.index(";")]
    for piece in ("float* logits", "int* hist", "int64_t ld_hist", "unsigned int* seen", "const int* step_base", "int step_off", "int64_t* next_token",
                  "float penalty", "int no_repeat_ngram_size", "int min_new_tokens", "int select", "int* state", "void* stream"):
        assert piece in decl, piece
    assert len(_lib.prototypes()["afk_decode_process"][1]) == 30
    with pytest.raises(_lib.AfkError):
        z = torch.zeros((1, 8))
        ops.decode_process(z, torch.zeros((1, 4), dtype=torch.int32), torch.zeros((1, 1), dtype=torch.int32), S0=1)

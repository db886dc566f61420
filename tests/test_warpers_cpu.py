"""CPU: the fp64 restatement of the sampler's steps 3a-3d (tests/_warpers_ref.py) pinned to the real classes - MinPLogitsWarper, TypicalLogitsWarper,
EpsilonLogitsWarper, EtaLogitsWarper (transformers/generation/logits_process.py) - alone and chained in GenerationMixin's order; the argument rules of
generate() for the four keywords (decode_process.resolve_warpers); the host side of afk_decode_sample_filtered.

Every parameter is snapped into the middle of a gap of the statistic its filter compares against (relative half-gap >= 1e-4 for the probability floors, mass
half-gap >= 5e-5 and d separation >= 5e-5 for typical_p), so the classes' fp32 arithmetic cannot decide a case: kept sets are required to be exactly equal.  A
case that misses its gap is skipped, and at most 5 % of a test's cases may be."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import _sampler_ref as R
from tests import _warpers_ref as W

TEMPS = (0.7, 1.0, 1.3)
TARGETS = dict(min_p=(0.05, 0.3), typical_p=(0.2, 0.9), epsilon_cutoff=(3e-4, 2e-2), eta_cutoff=(3e-4, 2e-2))
FILTERS = tuple(TARGETS)


def _hf_kept(z, top_k, top_p, kw):
    """the support the real warpers leave on the fp32 row z (temperature already applied), in the reference's order"""
    from transformers import (EpsilonLogitsWarper, EtaLogitsWarper, MinPLogitsWarper, TopKLogitsWarper, TopPLogitsWarper, TypicalLogitsWarper)

    procs = []
    if top_k:
        procs.append(TopKLogitsWarper(top_k=top_k))
    if top_p < 1.0:
        procs.append(TopPLogitsWarper(top_p=top_p))
    if "min_p" in kw:
        procs.append(MinPLogitsWarper(min_p=kw["min_p"]))
    if "typical_p" in kw:
        procs.append(TypicalLogitsWarper(mass=kw["typical_p"]))
    if "epsilon_cutoff" in kw:
        procs.append(EpsilonLogitsWarper(epsilon=kw["epsilon_cutoff"]))
    if "eta_cutoff" in kw:
        procs.append(EtaLogitsWarper(epsilon=kw["eta_cutoff"]))
    s = z[None].clone()
    for p in procs:
        s = p(None, s)
    return (s[0] > float("-inf")).numpy()


def _check(rows, combos, top_k, p_target):
    """rows: [(tag, fp32 logits)]; combos: tuples of filter names; the restatement's kept set equals the real chain's for every snapped case
    -> (cases, skipped)"""
    cases = skipped = 0
    for tag, x in rows:
        for T in TEMPS:
            row = R.Row(x, T)
            z = x if T == 1.0 else x / T
            top_p = 1.0
            if p_target < 1.0:
                top_p, half = row.snap_top_p(top_k, p_target)
                assert half >= 5e-5, (tag, T, half)
            for combo in combos:
                for pick in (0, 1):
                    cases += 1
                    chain, kw, ok = W.snap_chain(row, top_k, top_p, {f: TARGETS[f][pick] for f in combo})
                    if not ok:
                        skipped += 1
                        continue
                    ref = chain.result()
                    assert ref["keep"].any() and abs(ref["r"].sum() - 1.0) < 1e-12
                    assert np.array_equal(ref["keep"], _hf_kept(z, top_k, top_p, kw)), (tag, T, combo, kw, ref["margins"])
    return np.array([cases, skipped])


def _few_skipped(counts):
    assert counts[0] > 0 and counts[1] <= 0.05 * counts[0], counts.tolist()


@pytest.mark.parametrize("V", [37, 1000, 152064])
def test_each_filter_alone_and_behind_top_k_equals_the_real_class_on_bf16_valued_logits(V):
    rows = [((V, scale, b), R.bf16_logits(V, scale, seed=1000 * b + V % 997 + int(scale))) for scale in (1.0, 4.0) for b in range(3)]
    _few_skipped(_check(rows, [(f,) for f in FILTERS], 0, 1.0) + _check(rows, [(f,) for f in FILTERS] + [FILTERS], 50, 1.0))


@pytest.mark.parametrize("V", [37, 1000, 152064])
def test_chains_behind_top_p_equal_the_real_classes_on_tie_free_logits(V):
    """fp32 randn rows have singleton classes, so top-p's one deviation (a class stays or goes as a whole) cannot show.  Without top-k the P-set of such a row at
    V = 152 064 holds ~1e5 distinct values a relative 1e-5 apart - no gap to snap into - so that size runs behind top-k = 50 only"""
    g = torch.Generator().manual_seed(V)
    rows = [((V, scale, b), torch.randn(V, generator=g) * scale) for scale in (1.0, 4.0) for b in range(2)]
    combos = [(f,) for f in FILTERS] + [FILTERS]
    counts = _check(rows, combos, 50, 0.9)
    if V <= 1000:
        counts = counts + _check(rows, combos, 0, 0.9)
    _few_skipped(counts)


def test_restatement_known_answers():
    x = torch.log(torch.tensor([0.5, 0.25, 0.125, 0.0625, 0.0625]))
    assert W.reference(x, min_p=0.26)["keep"].tolist() == [True, True, False, False, False]          # 0.25 / 0.5 = 0.5 >= 0.26; 0.125 / 0.5 = 0.25 < 0.26
    assert W.reference(x, min_p=1.0)["keep"].tolist() == [True, False, False, False, False]
    assert W.reference(x, epsilon_cutoff=0.1)["keep"].tolist() == [True, True, True, False, False]
    assert W.reference(x, epsilon_cutoff=0.9)["keep"].tolist() == [True, False, False, False, False]  # above every probability: the top class stays
    # H = 1.875 bits: -log2 r = 1, 2, 3, 4, 4 -> d = .875, .125, 1.125, 2.125, 2.125 bits; by ascending d the cumulative mass is .25, .75, .875, 1
    assert W.reference(x, typical_p=0.2)["keep"].tolist() == [False, True, False, False, False]       # the band excludes the row maximum
    assert W.reference(x, typical_p=0.5)["keep"].tolist() == [True, True, False, False, False]
    assert W.reference(x, typical_p=0.9)["keep"].tolist() == [True, True, True, True, True]          # ties in d stay together
    # each filter's softmax is over what the one in front left: after min_p keeps {.5, .25}, r = (2/3, 1/3) and epsilon 0.4 drops the second
    assert W.reference(x, min_p=0.26, epsilon_cutoff=0.4)["keep"].tolist() == [True, False, False, False, False]
    # eta = min(eps, sqrt(eps) e^-H), H = 1.875 ln 2: eps = 0.09 -> min(0.09, 0.3 x 0.2726) = 0.0818 keeps 0.125 and drops 0.0625
    assert W.reference(x, eta_cutoff=0.09)["keep"].tolist() == [True, True, True, False, False]
    inf = W.reference(torch.tensor([1.0, float("inf"), 3.0]), min_p=0.5, typical_p=0.5, epsilon_cutoff=0.1, eta_cutoff=0.1)
    assert inf["keep"].tolist() == [False, True, False]
    assert not W.reference(torch.tensor([float("-inf"), float("nan")]), typical_p=0.5)["keep"].any()


def test_generate_resolves_and_validates_the_four_keywords_as_the_reference_does():
    import inspect

    from transformers import GenerationConfig

    from audio_flamingo_amd.decode_process import WARPER_DEFAULTS, WARPERS_OFF, resolve_warpers
    from audio_flamingo_amd.modeling import AudioFlamingo3ForConditionalGeneration as Mine

    sig = inspect.signature(Mine.generate)
    for k, v in WARPER_DEFAULTS.items():
        assert sig.parameters[k].default == v, k
    assert resolve_warpers() == WARPERS_OFF == dict(min_p=0.0, typical_p=1.0, epsilon_cutoff=0.0, eta_cutoff=0.0)
    assert resolve_warpers(min_p=0.05, typical_p=0.9, epsilon_cutoff=3e-4, eta_cutoff=2e-3) == dict(min_p=0.05, typical_p=0.9, epsilon_cutoff=3e-4, eta_cutoff=2e-3)
    # a generation config supplies what is left at its default; a keyword wins
    gc = GenerationConfig(do_sample=True, min_p=0.1, typical_p=0.8, epsilon_cutoff=1e-3)
    assert resolve_warpers(generation_config=gc) == dict(min_p=0.1, typical_p=0.8, epsilon_cutoff=1e-3, eta_cutoff=0.0)
    assert resolve_warpers(min_p=0.3, eta_cutoff=0.01, generation_config=gc) == dict(min_p=0.3, typical_p=0.8, epsilon_cutoff=1e-3, eta_cutoff=0.01)
    assert resolve_warpers(generation_config=SimpleNamespace(min_p=None, typical_p=None, epsilon_cutoff=None, eta_cutoff=None)) == WARPERS_OFF
    # inactive ranges, as _get_logits_processor gates them
    for off in (dict(typical_p=1.0), dict(typical_p=1.5), dict(epsilon_cutoff=0.0), dict(epsilon_cutoff=1.0), dict(epsilon_cutoff=-0.1), dict(eta_cutoff=1.0),
                dict(eta_cutoff=7.0), dict(min_p=0.0), dict(min_p=0)):
        assert resolve_warpers(**off) == WARPERS_OFF, off
    assert resolve_warpers(min_p=1)["min_p"] == 1.0
    # the classes' own errors, with their wording
    for bad in (-0.1, 1.5):
        with pytest.raises(ValueError, match=r"`min_p` has to be a float in the \[0, 1\] interval, but is"):
            resolve_warpers(min_p=bad)
    for bad in (0.0, -0.5):
        with pytest.raises(ValueError, match="`typical_p` has to be a float > 0 and < 1, but is"):
            resolve_warpers(typical_p=bad)
    with pytest.raises(ValueError, match="min_p"):
        resolve_warpers(generation_config=SimpleNamespace(min_p=2.0))
    # do_sample=False builds no warper: nothing acts and nothing is validated
    assert resolve_warpers(min_p=5.0, typical_p=-1.0, epsilon_cutoff=0.5, do_sample=False) == WARPERS_OFF


def test_filtered_entry_is_declared_exported_and_validates_without_a_device():
    from audio_flamingo_amd import _lib, ops

    protos = _lib.prototypes()
    assert hasattr(_lib.load(), "afk_decode_sample_filtered")
    old, new = protos["afk_decode_sample"][2], protos["afk_decode_sample_filtered"][2]
    assert new == old[:7] + ["min_p", "typical_p", "epsilon_cutoff", "eta_cutoff"] + old[7:]        # afk_decode_sample keeps its signature
    buf = torch.zeros(64, dtype=torch.float32)     # host memory: never touched - validation fails first
    p = buf.data_ptr()

    def call(min_p=0.0, typical_p=1.0, eps=0.0, eta=0.0, logits=p):
        _lib.call("afk_decode_sample_filtered", logits, 64, 1, 64, 1.0, 0, 1.0, min_p, typical_p, eps, eta, None, 0, None, 0, p, None, 0, None, None, 0, None, None,
                  0, 0, None, 0)

    nan = float("nan")
    with pytest.raises(_lib.AfkError, match="null"):
        call(logits=None)
    for kw in (dict(min_p=1.5), dict(min_p=nan)):
        with pytest.raises(_lib.AfkError, match="min_p <= 1"):
            call(**kw)
    for kw in (dict(typical_p=0.0), dict(typical_p=-1.0), dict(typical_p=nan)):
        with pytest.raises(_lib.AfkError, match="typical_p > 0"):
            call(**kw)
    for kw in (dict(eps=nan), dict(eta=nan)):
        with pytest.raises(_lib.AfkError, match="not a number"):
            call(**kw)
    with pytest.raises(_lib.AfkError, match="HIP device tensor"):
        ops.decode_sample(torch.zeros(2, 64), min_p=0.1)

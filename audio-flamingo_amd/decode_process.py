"""generate()'s logits processors on the device: repetition_penalty, no_repeat_ngram_size, min_new_tokens, suppress_tokens, begin_suppress_tokens - the
processors GenerationMixin._get_logits_processor (transformers/generation/utils.py:1174-1290) puts in front of the sampling warpers, applied by one launch per
step (afk_decode_process, csrc/decode_process.hip; the contract is in include/afk.h) so that the decode step stays capturable.

  resolve(...)      pure, CPU-runnable: merges the keywords with a generation config, validates as the reference does -> ProcessSpec
  build_state(...)  the device state of a prompt batch: id history, seen-set bitmap, id lists
  apply(...)        one launch on a [B, V] fp32 logits row block
  resolve_warpers(...)  pure, CPU-runnable: min_p / typical_p / epsilon_cutoff / eta_cutoff merged and validated the same way.  These four are no processors of
                    this file's launch: they sit behind top-p inside the sampler (afk_decode_sample_filtered, csrc/decode_sample.hip), where generate() sends them

Deliberately not covered (generate() keeps refusing them as keywords; in a generation config they stay ignored, as before):
  * bad_words_ids - its reference class adds a bias tensor to the whole row (which turns -0.0 into +0.0) and handles multi-token sequences; single ids are what
    suppress_tokens does;
  * top_h - its warper sits in front of top-k inside the sampler and is a sequential scan;
  * forced_eos_token_id, encoder_repetition_penalty / encoder_no_repeat_ngram_size, sequence_bias, exponential_decay_length_penalty."""
from __future__ import annotations

from typing import NamedTuple

NAMES = ("repetition_penalty", "no_repeat_ngram_size", "min_new_tokens", "suppress_tokens", "begin_suppress_tokens")
DEFAULTS = dict(repetition_penalty=1.0, no_repeat_ngram_size=0, min_new_tokens=0, suppress_tokens=None, begin_suppress_tokens=None)


class ProcessSpec(NamedTuple):
    penalty: float = 1.0          # 1.0: off
    ngram: int = 0                # 0: off
    min_new_tokens: int = 0       # 0 whenever no EOS id is known: the ban has nothing to act on
    eos: tuple = ()
    suppress: tuple = ()
    begin_suppress: tuple = ()

    @property
    def active(self) -> bool:
        return bool(self.penalty != 1.0 or self.ngram > 0 or (self.min_new_tokens > 0 and self.eos) or self.suppress or self.begin_suppress)


def _id_list(v, name):
    if v is None:
        return ()
    if hasattr(v, "tolist"):
        v = v.tolist()
    if isinstance(v, int) and not isinstance(v, bool):
        v = [v]
    if not isinstance(v, (list, tuple)) or any(isinstance(i, bool) or not isinstance(i, int) or i < 0 for i in v):
        raise ValueError(f"`{name}` has to be a list of positive integers, but is {v}")
    return tuple(int(i) for i in v)


def resolve(repetition_penalty=1.0, no_repeat_ngram_size=0, min_new_tokens=0, suppress_tokens=None, begin_suppress_tokens=None, eos_token_id=None,
            generation_config=None) -> ProcessSpec:
    """keywords (+ a generation config for the ones left at their default, as GenerationMixin merges them; an explicit keyword wins) -> ProcessSpec.
    Validation is the reference's: the penalty must be a float > 0 (RepetitionPenaltyLogitsProcessor.__init__, its message), the n-gram size an int >= 0
    (0 = off; NoRepeatNGramLogitsProcessor refuses what is not a positive int), min_new_tokens an int >= 0 that only acts when an EOS id is known
    (utils.py:1227-1230); eos_token_id an int or a list of ints (taken from the config when the argument is None)."""
    kw = dict(repetition_penalty=repetition_penalty, no_repeat_ngram_size=no_repeat_ngram_size, min_new_tokens=min_new_tokens, suppress_tokens=suppress_tokens,
              begin_suppress_tokens=begin_suppress_tokens)
    gc = generation_config
    if gc is not None:
        for k in NAMES:
            if kw[k] == DEFAULTS[k] and getattr(gc, k, None) is not None:
                kw[k] = getattr(gc, k)
        if eos_token_id is None:
            eos_token_id = getattr(gc, "eos_token_id", None)
    for k in ("repetition_penalty", "no_repeat_ngram_size", "min_new_tokens"):   # None = "unset" in a GenerationConfig
        if kw[k] is None:
            kw[k] = DEFAULTS[k]
    p = kw["repetition_penalty"]
    if p == 1 and not isinstance(p, bool):   # utils.py:1174 builds no processor for 1 / 1.0, so nothing validates it
        p = 1.0
    if not isinstance(p, float) or not (p > 0):
        raise ValueError(f"`penalty` has to be a strictly positive float, but is {p}")
    g = kw["no_repeat_ngram_size"]
    if isinstance(g, bool) or not isinstance(g, int) or g < 0:
        raise ValueError(f"`ngram_size` has to be a strictly positive integer, but is {g}")
    mn = kw["min_new_tokens"]
    if isinstance(mn, bool) or not isinstance(mn, int) or mn < 0:
        raise ValueError(f"`min_new_tokens` has to be a positive integer, but is {mn}")
    eos = _id_list(eos_token_id, "eos_token_id")
    return ProcessSpec(penalty=float(p), ngram=int(g), min_new_tokens=int(mn) if eos else 0, eos=eos if mn > 0 else (),
                       suppress=_id_list(kw["suppress_tokens"], "suppress_tokens"), begin_suppress=_id_list(kw["begin_suppress_tokens"], "begin_suppress_tokens"))


WARPER_DEFAULTS = dict(min_p=None, typical_p=1.0, epsilon_cutoff=0.0, eta_cutoff=0.0)
WARPERS_OFF = dict(min_p=0.0, typical_p=1.0, epsilon_cutoff=0.0, eta_cutoff=0.0)


def resolve_warpers(min_p=None, typical_p=1.0, epsilon_cutoff=0.0, eta_cutoff=0.0, generation_config=None, do_sample=True) -> dict:
    """keywords (+ a generation config for the ones left at their default; an explicit keyword wins) -> the four values as ops.decode_sample takes them, an
    inactive filter at its "off" value.  As GenerationMixin._get_logits_processor gates them (utils.py:1323-1343): min_p whenever it is set, typical_p when
    < 1, epsilon_cutoff / eta_cutoff only inside (0, 1); the classes' own validation and wording (MinPLogitsWarper / TypicalLogitsWarper.__init__): min_p
    outside [0, 1] and typical_p <= 0 raise ValueError.  do_sample=False: nothing is built, so nothing is validated and all four are off."""
    kw = dict(min_p=min_p, typical_p=typical_p, epsilon_cutoff=epsilon_cutoff, eta_cutoff=eta_cutoff)
    gc = generation_config
    if gc is not None:
        for k in kw:
            if kw[k] == WARPER_DEFAULTS[k] and getattr(gc, k, None) is not None:
                kw[k] = getattr(gc, k)
    out = dict(WARPERS_OFF)
    if not do_sample:
        return out
    if kw["min_p"] is not None:
        if not (0 <= kw["min_p"] <= 1.0):
            raise ValueError(f"`min_p` has to be a float in the [0, 1] interval, but is {kw['min_p']}")
        out["min_p"] = float(kw["min_p"])
    if kw["typical_p"] is not None and kw["typical_p"] < 1.0:
        mass = float(kw["typical_p"])
        if not (mass > 0 and mass < 1):
            raise ValueError(f"`typical_p` has to be a float > 0 and < 1, but is {mass}")
        out["typical_p"] = mass
    for k in ("epsilon_cutoff", "eta_cutoff"):
        if kw[k] is not None and 0.0 < kw[k] < 1.0:
            out[k] = float(kw[k])
    return out


def build_state(spec: ProcessSpec, ids, max_new_tokens: int, V: int):
    """device state of afk_decode_process for the prompt batch ids [B, S0] (exactly what generate() was given: the reference's processors see padding and
    <sound> ids too): hist [B, S0 + max_new_tokens] int32 with the prompt in front, seen [B, ceil(V / 32)] int32 = the prompt's ids as a bitmap, the id lists.
    One-time setup in torch ops, outside the captured step."""
    import torch

    B, S0 = ids.shape
    dev = ids.device
    hist = torch.zeros((B, S0 + int(max_new_tokens)), device=dev, dtype=torch.int32)
    hist[:, :S0] = ids
    nwords = (V + 31) // 32
    mask = torch.zeros((B, nwords * 32), device=dev, dtype=torch.bool)
    rows, cols = torch.nonzero((ids >= 0) & (ids < V), as_tuple=True)   # an id outside the vocabulary marks nothing (the kernel skips it as well)
    mask[rows, ids[rows, cols].long()] = True
    weights = torch.tensor([1 << i for i in range(31)] + [-(1 << 31)], device=dev, dtype=torch.int64)   # bit 31 is the sign bit of the int32 word
    seen = (mask.view(B, nwords, 32).to(torch.int64) * weights).sum(-1).to(torch.int32).contiguous()
    lst = lambda t: torch.tensor(t, device=dev, dtype=torch.int32) if t else None
    return dict(spec=spec, S0=S0, hist=hist, seen=seen, suppress=lst(spec.suppress), begin_suppress=lst(spec.begin_suppress), eos=lst(spec.eos))


def apply(ps, logits, *, next_token=None, step_base=None, step_off=0, **select_kw):
    """one afk_decode_process launch on the fp32 logits [B, V] (in place) for token t = *step_base + step_off; select_kw: ops.decode_process's selection block"""
    from . import ops

    spec = ps["spec"]
    return ops.decode_process(logits, ps["hist"], ps["seen"], S0=ps["S0"], penalty=spec.penalty, ngram=spec.ngram, suppress=ps["suppress"],
                              begin_suppress=ps["begin_suppress"], eos=ps["eos"], min_new_tokens=spec.min_new_tokens, next_token=next_token,
                              step_base=step_base, step_off=step_off, **select_kw)

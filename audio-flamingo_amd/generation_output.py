"""What generate(return_dict_in_generate=True) returns, and the pure (CPU-runnable) resolution of the flags that ask for it.

  AfkGenerateOutput        GenerateDecoderOnlyOutput's contract (transformers/generation/utils.py:169): sequences, scores, logits, attentions, hidden_states,
                           past_key_values with the ModelOutput access surface modeling.AF3Output implements
  resolve_output_flags()   keyword first, else generation config (utils.py:2829-2837); the combinations generate() refuses
"""
from __future__ import annotations

from typing import NamedTuple

from ._lib import AfkError


class AfkGenerateOutput:
    """sequences [B, S0 + n] int64; scores / logits: tuples of n tensors [B, V] fp32 (processed-and-warped scores / raw lm_head logits of every generated
    token), views of ONE [max_new_tokens, B, V] buffer each - the decode graph writes a slot per step -, or None when not asked for; attentions /
    hidden_states: always None (generate() refuses output_attentions / output_hidden_states); past_key_values: the AfkKVCache of every token but the last,
    as the reference's cache holds them - forward(past_key_values=...) takes it as is.

    ModelOutput access: attribute, key, integer and slice access; keys() / items() / iteration / len() over the fields that are not None; to_tuple()."""

    _FIELDS = ("sequences", "scores", "logits", "attentions", "hidden_states", "past_key_values")

    def __init__(self, sequences=None, scores=None, logits=None, attentions=None, hidden_states=None, past_key_values=None):
        self.sequences, self.scores, self.logits = sequences, scores, logits
        self.attentions, self.hidden_states, self.past_key_values = attentions, hidden_states, past_key_values

    def keys(self):
        return [f for f in self._FIELDS if getattr(self, f) is not None]

    def values(self):
        return [getattr(self, f) for f in self.keys()]

    def items(self):
        return [(f, getattr(self, f)) for f in self.keys()]

    def to_tuple(self):
        return tuple(self.values())

    def get(self, k, default=None):
        return getattr(self, k) if k in self else default

    def __contains__(self, k):
        return k in self._FIELDS and getattr(self, k) is not None

    def __getitem__(self, k):
        if isinstance(k, str):
            if k not in self:   # ModelOutput keeps only the fields that are set in its dict
                raise KeyError(k)
            return getattr(self, k)
        return self.to_tuple()[k]

    def __iter__(self):
        return iter(self.keys())

    def __len__(self):
        return len(self.keys())

    def __repr__(self):
        return f"AfkGenerateOutput({', '.join(self.keys())})"


class OutputFlags(NamedTuple):
    return_dict: bool = False
    scores: bool = False   # collect the processed / warped scores (only ever True with return_dict)
    logits: bool = False   # collect the raw lm_head logits (only ever True with return_dict)

    @property
    def collect(self) -> bool:
        return self.scores or self.logits


_FLAG_NAMES = ("return_dict_in_generate", "output_scores", "output_logits", "output_attentions", "output_hidden_states")


def resolve_output_flags(return_dict_in_generate=None, output_scores=None, output_logits=None, output_attentions=None, output_hidden_states=None, *,
                         generation_config=None, num_beams=1, use_cache=True, exact_fp32=False) -> OutputFlags:
    """The reference's rule (transformers/generation/utils.py:2829-2837): a keyword that is not None wins, else the generation config's attribute, else False;
    scores and logits are collected only under return_dict_in_generate (output_scores=True alone returns the plain tensor, silently, as the reference does).
    Refused with an AfkError that names the combination, whenever an output object is asked for - by keyword or by the generation config, so a config that
    sets return_dict_in_generate=True together with one of these used to be ignored and now raises; a call that asks for no output object is unaffected:
    num_beams > 1 (the reference returns another class with beam_indices), use_cache=False, AFK_EXACT_FP32=1 (both are verification paths that keep no
    cache and no device rows); output_attentions / output_hidden_states are refused whenever they are set, in a generation config too (where they were ignored
    before)."""
    kw = dict(zip(_FLAG_NAMES, (return_dict_in_generate, output_scores, output_logits, output_attentions, output_hidden_states)))
    val = {k: bool(v if v is not None else (getattr(generation_config, k, None) if generation_config is not None else None)) for k, v in kw.items()}
    for k in ("output_attentions", "output_hidden_states"):
        if val[k]:
            raise AfkError(f"generate({k}=True) is not supported: the fused decode step keeps no attention maps or per-layer hidden states")
    if not val["return_dict_in_generate"]:
        return OutputFlags()
    if num_beams > 1:
        raise AfkError("generate(return_dict_in_generate=True, num_beams > 1) is not supported: beam search returns the plain sequences only (no "
                       "sequences_scores / beam_indices)")
    if not use_cache:
        raise AfkError("generate(return_dict_in_generate=True, use_cache=False) is not supported: the recompute path keeps no cache and no per-step rows")
    if exact_fp32:
        raise AfkError("generate(return_dict_in_generate=True) with AFK_EXACT_FP32=1 is not supported: the exact-fp32 path keeps no cache and no per-step rows")
    return OutputFlags(True, val["output_scores"], val["output_logits"])


def resolve_num_return_sequences(num_return_sequences=None, *, generation_config=None, num_beams=1, do_sample=False) -> int:
    """num_return_sequences of a generate() call: the keyword when it is given (not None), else the generation config's attribute, else 1, validated as
    GenerationConfig.validate does (transformers/generation/configuration_utils.py, 2.4) and with its messages: more than one sequence needs sampling or beam
    search, and beam search returns at most num_beams per row."""
    n = num_return_sequences if num_return_sequences is not None else (getattr(generation_config, "num_return_sequences", None) if generation_config is not None else None)
    n = 1 if n is None else n
    if not isinstance(n, int) or isinstance(n, bool) or n < 1:
        raise ValueError(f"`num_return_sequences` must be a strictly positive integer, but is {n}.")
    num_beams = 1 if num_beams is None else int(num_beams)
    if n > 1:
        if num_beams == 1:
            if not do_sample:
                raise ValueError(f"Greedy methods (do_sample != True) without beam search do not support `num_return_sequences` different than 1 (got {n}).")
        elif n > num_beams:
            raise ValueError(f"`num_return_sequences` ({n}) has to be smaller or equal to `num_beams` ({num_beams}).")
    return n


def step_buffer_view(rows):
    """rows: a tuple of [B, V] fp32 tensors.  When they are consecutive views of one buffer (same storage, constant positive stride between them, unit column
    stride) -> that buffer as a [T, B, V] view, without a copy; else None (the caller stacks them)."""
    import torch

    r0 = rows[0]
    if r0.dim() != 2 or r0.stride(1) != 1 or r0.dtype != torch.float32:
        return None
    step = None
    for a, b in zip(rows, rows[1:]):
        if (b.shape != r0.shape or b.stride() != r0.stride() or b.dtype != r0.dtype or b.device != r0.device
                or b.untyped_storage().data_ptr() != r0.untyped_storage().data_ptr()):
            return None
        d = b.storage_offset() - a.storage_offset()
        if step is None:
            step = d
        if d != step or d <= 0:
            return None
    if step is None:
        step = r0.shape[0] * r0.stride(0)
    return torch.as_strided(r0, (len(rows),) + tuple(r0.shape), (step,) + tuple(r0.stride()), r0.storage_offset())

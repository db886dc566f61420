"""generate()'s stopping rule on the device: eos_token_id as a list and stop_strings= / tokenizer=, decided by one launch per step (afk_decode_stop,
csrc/decode_stop.hip; the contract is in include/afk.h) so that the decode step stays capturable - what GenerationMixin._get_stopping_criteria
(transformers/generation/utils.py:1340-1395) builds as EosTokenCriteria and StopStringCriteria, plus the pad substitution of its loop.

  resolve(...)      pure, CPU-runnable: merges the keywords with a generation config, validates as the reference does -> StopSpec
  build_table(...)  StopStringCriteria(tokenizer, stop_strings) constructed on the host; its run-time table is read, nothing of it is restated here
  build_state(...)  the device state of a prompt batch: uploaded table, eos ids, ids, stop_at, status
  apply(...)        one launch for the token just selected

Deliberately not covered: max_time, ConfidenceCriteria, user criteria objects inside the graph (they run in the eager hook loop, behind this launch), beam
search with stop strings."""
from __future__ import annotations

from typing import NamedTuple

INT_MAX = 2 ** 31 - 1
NO_TOKENIZER = ("There are one or more stop strings, either in the arguments to `generate` or in the model's generation config, but we could not locate a "
                "tokenizer. When generating with stop strings, you must pass the model's tokenizer to the `tokenizer` argument of `generate`.")


class StopSpec(NamedTuple):
    eos: tuple = ()             # () = no EOS id known
    pad: int | None = None      # pad_token_id, defaulted to the first eos id as the reference does; None only when neither is known
    stop_strings: tuple = ()

    @property
    def device(self) -> bool:
        """the rule runs as a launch inside the step: more than one eos id, or stop strings (one id and no string is generate()'s scalar case)"""
        return len(self.eos) > 1 or bool(self.stop_strings)


def _eos_ids(v):
    if v is None:
        return ()
    if hasattr(v, "tolist"):
        v = v.tolist()
    if isinstance(v, int) and not isinstance(v, bool):
        v = [v]
    if not isinstance(v, (list, tuple)) or any(isinstance(i, bool) or not isinstance(i, int) or i < 0 for i in v):
        raise ValueError(f"`eos_token_id` has to be a list of positive integers, but is {v}")
    return tuple(int(i) for i in v)


def resolve(eos_token_id=None, pad_token_id=None, stop_strings=None, tokenizer=None, generation_config=None, num_beams=1, use_cache=True,
            exact_fp32=False) -> StopSpec:
    """keywords (+ a generation config for the ones left at None, as GenerationMixin merges them; an explicit keyword wins) -> StopSpec.  eos_token_id: an
    int, list, tuple or tensor; pad_token_id defaults to the first eos id (utils.py:1795-1800); stop_strings: a string or a list of strings, which needs
    tokenizer= (the reference's ValueError without one).  Stop strings are refused - an AfkError that names the combination - with num_beams > 1, with
    use_cache=False and with AFK_EXACT_FP32=1; tokenizer= without an active stop string stays refused."""
    from ._lib import AfkError

    gc = generation_config
    if gc is not None:
        if eos_token_id is None:
            eos_token_id = getattr(gc, "eos_token_id", None)
        if pad_token_id is None:
            pad_token_id = getattr(gc, "pad_token_id", None)
        if stop_strings is None:
            stop_strings = getattr(gc, "stop_strings", None)
    eos = _eos_ids(eos_token_id)
    if hasattr(pad_token_id, "tolist"):
        pad_token_id = pad_token_id.tolist()
    if isinstance(pad_token_id, (list, tuple)) and len(pad_token_id) == 1:
        pad_token_id = pad_token_id[0]
    if pad_token_id is not None and (isinstance(pad_token_id, bool) or not isinstance(pad_token_id, int) or pad_token_id < 0):
        raise ValueError(f"`pad_token_id` has to be a positive integer, but is {pad_token_id}")
    pad = int(pad_token_id) if pad_token_id is not None else (eos[0] if eos else None)
    if isinstance(stop_strings, str):
        stop_strings = [stop_strings]
    strings = tuple(stop_strings) if stop_strings else ()
    if any(not isinstance(s, str) or not s for s in strings):
        raise ValueError(f"`stop_strings` has to be a string or a list of non-empty strings, but is {stop_strings}")
    if strings:
        if tokenizer is None:
            raise ValueError(NO_TOKENIZER)
        for bad, what in ((int(num_beams) > 1, "num_beams > 1"), (not use_cache, "use_cache=False"), (bool(exact_fp32), "AFK_EXACT_FP32=1")):
            if bad:
                raise AfkError(f"generate(stop_strings=...) with {what}: stop strings run in greedy or sampled decoding on the KV cache only")
    elif tokenizer is not None:
        raise AfkError("generate(tokenizer=...) is not supported by this implementation")
    return StopSpec(eos=eos, pad=pad, stop_strings=strings)


def build_table(tokenizer, stop_strings):
    """the run-time table of StopStringCriteria(tokenizer, stop_strings) as host tensors: the class is constructed and its fields are read"""
    import torch
    from transformers.generation.stopping_criteria import StopStringCriteria

    c = StopStringCriteria(tokenizer=tokenizer, stop_strings=list(stop_strings))
    table = c.embedding_vec.detach().to("cpu", torch.int32).contiguous()
    P, E, S = int(c.max_valid_positions), int(c.max_valid_end_lens), int(c.num_stop_strings)
    if table.dim() != 2 or table.shape[1] != S * (P + E) + 1:
        raise ValueError(f"StopStringCriteria: embedding_vec {tuple(table.shape)} is not [rows, S * (P + E) + 1] for S = {S}, P = {P}, E = {E}")
    return dict(table=table, P=P, E=E, S=S, target_lens=c.target_lens.detach().to("cpu", torch.int32).contiguous(), W=int(c.maximum_token_len))


def build_state(spec: StopSpec, ids, max_new_tokens: int, table=None):
    """device state of afk_decode_stop for the prompt batch ids [B, S0] (exactly what generate() was given): ids [B, S0 + max_new_tokens] int32 with the prompt
    in front, stop_at [B] = INT_MAX, status [2] = {-1, B}, the eos ids and - with stop strings - the table of build_table(), uploaded once.  One-time setup in
    torch ops, outside the captured step."""
    import torch

    B, S0 = ids.shape
    dev = ids.device
    buf = torch.zeros((B, S0 + int(max_new_tokens)), device=dev, dtype=torch.int32)
    buf[:, :S0] = ids
    st = dict(spec=spec, S0=S0, max_new=int(max_new_tokens), ids=buf, stop_at=torch.full((B,), INT_MAX, device=dev, dtype=torch.int32),
              status=torch.tensor([-1, B], device=dev, dtype=torch.int32), eos=torch.tensor(spec.eos, device=dev, dtype=torch.int32) if spec.eos else None,
              pad=int(spec.pad) if spec.pad is not None else 0, table=None, P=0, E=0, S=0, target_lens=None, W=0)
    if spec.stop_strings:
        if table is None:
            raise ValueError("decode_stop.build_state: stop strings need the table of build_table()")
        st.update(table=table["table"].to(dev), target_lens=table["target_lens"].to(dev), P=table["P"], E=table["E"], S=table["S"], W=table["W"])
    return st


def apply(ss, next_token, *, step_base=None, step_off=0, feed_pad=False):
    """one afk_decode_stop launch for token t = *step_base + step_off, the one just selected into next_token [B] int64"""
    from . import ops

    return ops.decode_stop(next_token, ss["ids"], ss["stop_at"], S0=ss["S0"], max_new=ss["max_new"], status=ss["status"], step_base=step_base, step_off=step_off,
                           eos=ss["eos"], pad=ss["pad"], feed_pad=feed_pad, table=ss["table"], P=ss["P"], E=ss["E"], S=ss["S"], target_lens=ss["target_lens"],
                           W=ss["W"])

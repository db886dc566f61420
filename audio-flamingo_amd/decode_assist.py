"""generate()'s assisted (speculative) decoding on the device: assistant_model= / num_assistant_tokens=, greedy, one sequence on the KV cache.  A small second
model of this package drafts k tokens per step on a cache of its own, the target runs them and the last emitted token through ONE pass over its weights and
keeps the leading drafts its own argmaxes confirm plus one more token - what GenerationMixin._assisted_decoding (transformers/generation/utils.py:3562-3830)
does with an AssistedCandidateGenerator (transformers/generation/candidate_generator.py).  The ids are the target's plain greedy ids; only the cost per token
changes.  The verify forward, the accept rule and the call's state are prompt-lookup decoding's (decode_lookup.py: _lookup_forward, afk_lookup_accept,
build_state); what is new is the candidate source - the draft model's own single-sequence decode chain, between two small launches (afk_assist_begin /
afk_assist_stage, csrc/decode_assist.hip; the contract is in include/afk.h).  docs/generate.md, "Assisted decoding".

  resolve(...)      pure, CPU-runnable: the keywords against the assistant's generation config, validated, with every refusal -> AssistSpec | None
  build_state(...)  the draft model's side of one call: its cache, its running step state, its input row, its token buffer, its workspaces
  begin(...)        one launch: the draft model's step state and input row as the target left the sequence
  stage(...)        one launch: the drafted tokens as candidates and as the M = k + 1 input rows of the verify forward
  kept / begin_host / stage_host   the same rules in plain Python and torch ops with host reads (generate()'s assist_on_device = False route)

Deviations from the reference's draft rule, neither of which can change the ids: num_assistant_tokens_schedule is "constant" (every step drafts exactly k
tokens), and assistant_confidence_threshold is ignored (a captured step enqueues its k draft steps whatever the draft model thinks of them, so ending a draft
early would save nothing).  They are why the default k is 5 and not the reference's 20.  Not covered: sampled assisted decoding, universal assisted decoding
(an assistant with another tokenizer), batches."""
from __future__ import annotations

from dataclasses import dataclass
from typing import NamedTuple

from .decode_lookup import BATCH, DONE, EMITTED, LEN, MAX_K, N_CAND

DEFAULT_K = 5


class AssistSpec(NamedTuple):
    model: object   # the draft model
    k: int          # num_assistant_tokens: drafted tokens per step (the verify forward runs k + 1 rows)


def resolve(assistant_model=None, num_assistant_tokens=None, *, is_model=True, same_device=True, target_vocab=None, assistant_vocab=None, batch_size=1,
            do_sample=False, num_beams=1, copies=1, use_cache=True, exact_fp32=False, processors=False, hooks=False, stop_strings=False, output_object=False,
            past=False, share_prompt=None, guidance=False, decode_weights=None, lookup=False, prompt_len=None, max_new_tokens=None, max_positions=None):
    """assistant_model (None: assisted decoding is off -> None, and num_assistant_tokens is ignored) + num_assistant_tokens (None: the assistant's
    generation_config.num_assistant_tokens, where the reference reads it; else 5) -> AssistSpec.
    is_model / same_device: the assistant is an instance of this package's model class, on the target's device; target_vocab / assistant_vocab:
    (embedding rows, lm_head rows, audio_token_id) of the two models - what only generate() can read off them.
    ValueError where the reference raises one: a k that is no integer or <= 0, a batch of more than one sequence (its message).  AfkError, naming the
    combination, for what this implementation does not run with an assistant: do_sample, num_beams > 1, num_return_sequences > 1 (copies), use_cache=False,
    AFK_EXACT_FP32=1, logits processors (built-in or logits_processor=), stopping_criteria= / streamer= (hooks), stop strings, the output object,
    past_key_values=, share_prompt=True, an active guidance_scale, decode_weights="fp8" (both only when asked for by keyword: the class defaults fall back
    silently, decode_share.resolve / decode_w8.resolve with assist=True), prompt_lookup_num_tokens; a k above the accept launch's cap; an assistant of
    another class or device; embedding rows, lm_head rows or an audio_token_id that differ from the target's (both numbers named); a prompt for which
    prompt_len + max_new_tokens + k + 1 exceeds max_positions = (the target's, the assistant's) max_position_embeddings - known before any launch."""
    from ._lib import AfkError

    if assistant_model is None:
        return None
    if not is_model:
        raise AfkError(f"generate(assistant_model=...) has to be an AudioFlamingo3ForConditionalGeneration (or MusicFlamingoForConditionalGeneration) of this "
                       f"package, but is a {type(assistant_model).__name__}")
    k = num_assistant_tokens
    if k is None:
        k = getattr(getattr(assistant_model, "generation_config", None), "num_assistant_tokens", None)
    if k is None:
        k = DEFAULT_K
    if isinstance(k, bool) or not isinstance(k, int):
        raise ValueError(f"`num_assistant_tokens` has to be an integer, but is {k!r}")
    if k <= 0:
        raise ValueError(f"`num_assistant_tokens` has to be a positive integer, but is {k}")
    if int(batch_size) != 1:
        raise ValueError(BATCH)
    for bad, what in ((bool(lookup), "prompt_lookup_num_tokens="), (bool(do_sample), "do_sample=True"), (int(num_beams) > 1, "num_beams > 1"),
                      (int(copies) > 1, "num_return_sequences > 1"), (not use_cache, "use_cache=False"), (bool(exact_fp32), "AFK_EXACT_FP32=1"),
                      (bool(processors), "logits processors (built-in or logits_processor=)"), (bool(hooks), "stopping_criteria= / streamer="),
                      (bool(stop_strings), "stop_strings="), (bool(output_object), "return_dict_in_generate / output_scores / output_logits"),
                      (bool(past), "past_key_values="), (share_prompt is True, "share_prompt=True"), (bool(guidance), "guidance_scale="),
                      (decode_weights == "fp8", "decode_weights='fp8'")):
        if bad:
            raise AfkError(f"generate(assistant_model=...) with {what}: assisted decoding runs greedy decoding of one sequence on a fresh bf16 KV cache only")
    if k > MAX_K:
        raise AfkError(f"generate(assistant_model=..., num_assistant_tokens={k}): at most {MAX_K} drafted tokens per step")
    if not same_device:
        raise AfkError("generate(assistant_model=...): the assistant has to live on the device of the model it assists")
    if target_vocab is not None and assistant_vocab is not None:
        for what, a, t in zip(("embedding rows", "lm_head rows", "audio_token_id"), assistant_vocab, target_vocab):
            if a != t:
                raise AfkError(f"generate(assistant_model=...): the assistant's {what} ({a}) differ from the target's ({t}); both models have to share one "
                               f"vocabulary (universal assisted decoding is not built)")
    if prompt_len is not None and max_new_tokens is not None and max_positions is not None:
        for whose, cap in zip(("the target's", "the assistant's"), max_positions):
            if int(prompt_len) + int(max_new_tokens) + k + 1 > int(cap):
                raise AfkError(f"generate(assistant_model=..., num_assistant_tokens={k}): prompt {int(prompt_len)} + max_new_tokens {int(max_new_tokens)} + {k + 1} "
                               f"drafted positions exceed {whose} max_position_embeddings {int(cap)}")
    return AssistSpec(model=assistant_model, k=int(k))


@dataclass
class AssistState:
    """the draft model's side of one call.  A record: no behaviour."""
    model: object
    k: int
    cache: tuple      # its own (K, Vt), prefilled with the same prompt: slots and positions agree with the target's
    dstate: object    # int32 [4]: its running copy of the target's [lo, key-range end, cache slot, position]
    x0: object        # bf16 [1, H_a]: its embedding row of the token it runs next
    nxt: object       # int64 [1]: the token it selected last
    draft: object     # int64 [cache slots]: drafted token j of a step at index (the target's cache slot) + j
    emb: object       # its embed_tokens weight
    head: object      # its lm_head weight
    part_val: object  # the lm_head launch's (max, argmax) per eight rows
    part_idx: object
    aws: object       # its attention workspace


def build_state(model, k, cache, dev):
    """the static buffers of the draft model's steps on `cache` (K [L, 1, Smax, nk], Vt): one-time setup in torch ops, outside the captured step"""
    import torch

    emb, head = model.arena[model._lm + "embed_tokens.weight"].data, model.arena["lm_head.weight"].data
    V, slots = head.shape[0], cache[0].shape[2]
    on_chain = model._chain_ok(1) and V % 8 == 0
    return AssistState(model=model, k=int(k), cache=cache, dstate=torch.zeros(4, device=dev, dtype=torch.int32),
                       x0=torch.zeros((1, emb.shape[1]), device=dev, dtype=torch.bfloat16), nxt=torch.zeros(1, device=dev, dtype=torch.int64),
                       draft=torch.zeros(slots, device=dev, dtype=torch.int64), emb=emb, head=head,
                       part_val=torch.empty(V // 8, device=dev, dtype=torch.float32) if on_chain else None,
                       part_idx=torch.empty(V // 8, device=dev, dtype=torch.int32) if on_chain else None,
                       aws=model._decode_attn_workspace(dev, cache[1].shape[4]) if on_chain else None)


def begin(ls, a):
    """one afk_assist_begin launch: a.dstate <- the target's step state, a.x0 <- the draft model's embedding row of the last emitted token"""
    from . import _lib, ops

    _lib.call("afk_assist_begin", ls["ids"].data_ptr(), ls["ids"].numel(), ls["status"].data_ptr(), ls["state"].data_ptr(), a.dstate.data_ptr(), a.emb.data_ptr(),
              a.emb.stride(0), a.emb.shape[0], a.emb.shape[1], a.x0.data_ptr(), ops._stream())


def stage(ls, a, emb):
    """one afk_assist_stage launch: the candidates of this step and the verify forward's inputs - ls["x"] (the TARGET's embedding rows), ls["pos"], ls["krange"]"""
    from . import _lib, ops

    n_eos = 0 if ls["eos"] is None else ls["eos"].numel()
    _lib.call("afk_assist_stage", ls["ids"].data_ptr(), ls["ids"].numel(), ls["status"].data_ptr(), ls["state"].data_ptr(), a.k, ls["max_new"], ops._p(ls["eos"]),
              n_eos, a.draft.data_ptr(), a.draft.numel(), ls["cand"].data_ptr(), ls["rows"].data_ptr(), ls["pos"].data_ptr(), ls["krange"].data_ptr(),
              emb.data_ptr(), emb.stride(0), emb.shape[0], ls["x"].shape[1], ls["x"].data_ptr(), ls["x"].stride(0), ops._stream())


# ------------------------------------------------------------------ the same rules on the host (assist_on_device = False)
def kept(drafts, eos=(), budget=None, done=False):
    """afk_assist_stage's rule on a list of ints -> n_cand, the number of leading drafts kept: all of them, cut BEHIND the first eos id and to `budget`
    (max_new - emitted - 1); none when the call is done"""
    if done or (budget is not None and budget <= 0):
        return 0
    n = len(drafts) if budget is None else min(len(drafts), budget)
    for i in range(n):
        if drafts[i] in eos:
            return i + 1
    return n


def begin_host(ls, a):
    """begin() by host reads and torch ops -> the last emitted token (the draft model's first input of the step)"""
    a.dstate.copy_(ls["state"])
    last = int(ls["ids"][int(ls["status"][LEN]) - 1])
    a.nxt.fill_(min(max(last, 0), a.emb.shape[0] - 1))
    a.x0.copy_(a.emb.index_select(0, a.nxt))
    return last


def stage_host(ls, a, emb):
    """stage() by host reads and torch ops: the same candidates, rows, positions, key ranges and embedding rows"""
    import torch

    st = ls["status"].tolist()
    lo, end, cur, position = ls["state"].tolist()
    last = int(ls["ids"][st[LEN] - 1])
    drafts = a.draft[cur:cur + a.k].tolist()
    n = kept(drafts, ls["eos_ids"], ls["max_new"] - st[EMITTED] - 1, bool(st[DONE]))
    dev = ls["ids"].device
    rows = [last] + drafts[:n] + [last] * (a.k - n)
    ls["status"][N_CAND] = n
    ls["cand"].copy_(torch.tensor(rows[1:], device=dev, dtype=torch.int32))
    ls["rows"].copy_(torch.tensor(rows, device=dev, dtype=torch.int64))
    ar = torch.arange(ls["M"], device=dev, dtype=torch.int32)
    ls["pos"].copy_(position + ar)
    ls["krange"].copy_(torch.stack([torch.full_like(ar, lo), end + ar], -1))
    ls["x"].copy_(emb.index_select(0, ls["rows"].clamp(0, emb.shape[0] - 1)))

"""generate()'s prompt-lookup decoding on the device: prompt_lookup_num_tokens= / max_matching_ngram_size=, greedy, one sequence on the KV cache.  A step drafts
up to k tokens by n-gram lookup in the ids seen so far, runs them and the last emitted token through the model in ONE pass over the weights, and keeps the
leading drafts the model's own argmaxes confirm plus one more token - what GenerationMixin._assisted_decoding (transformers/generation/utils.py:3562-3830) does with
a PromptLookupCandidateGenerator (transformers/generation/candidate_generator.py:1013-1150).  The two decisions are launches (afk_lookup_draft / afk_lookup_accept,
csrc/decode_lookup.hip; the contract is in include/afk.h), so the whole step stays capturable.

  resolve(...)      pure, CPU-runnable: merges the keywords with a generation config, validates as the reference does, refuses what is not built -> LookupSpec | None
  build_state(...)  the device state of one call: ids, status words, the step's rows / positions / key ranges, scratch
  draft(...)        one launch: the candidates and the M = k + 1 input rows of the verify forward
  accept(...)       one call: the row argmaxes, the accepted prefix, the bookkeeping
  draft_host / accept_host   the same two rules in torch ops with host reads (generate()'s lookup_on_device = False route)

Deliberately not covered: sampled lookup (the draw for token t on row j needs the counter (t + j, 0); the sampler keys its counter by row), logits processors
on candidate rows, batches.  A draft model as the candidate source - generate(assistant_model=) - is decode_assist.py: it reuses build_state, accept and the
verify forward of this route and replaces draft() by the draft model's own steps."""
from __future__ import annotations

from typing import NamedTuple

MAX_K, MAX_NGRAM, STATUS_WORDS, WS_WORDS = 31, 16, 8, 1024   # AFK_LOOKUP_* of include/afk.h
LEN, EMITTED, DONE, N_CAND, STEPS, ACCEPTED, REJECTING, N_MATCH = range(8)   # the status words
INVALID = "Invalid max_matching_ngram_size or num_output_tokens"   # PromptLookupCandidateGenerator.__init__ (candidate_generator.py:1054-1055)
BATCH = "assisted generate is only supported for batch_size = 1"   # _assisted_decoding (utils.py:3670)


class LookupSpec(NamedTuple):
    k: int       # prompt_lookup_num_tokens: drafted tokens per step (the verify forward runs k + 1 rows)
    ngram: int   # max_matching_ngram_size


def resolve(prompt_lookup_num_tokens=None, max_matching_ngram_size=None, generation_config=None, *, batch_size=1, do_sample=False, num_beams=1,
            use_cache=True, exact_fp32=False, processors=False, hooks=False, stop_strings=False, output_object=False):
    """keywords (+ a generation config for the ones left at None; an explicit keyword wins) -> LookupSpec, or None when prompt-lookup decoding is off
    (prompt_lookup_num_tokens None in both; max_matching_ngram_size alone switches nothing on, as in the reference).  An unset ngram size means 2
    (utils.py:1030).  ValueError where the reference raises one, with its message: a value <= 0, a batch of more than one sequence.  AfkError, naming the
    combination, for what this implementation does not run with lookup decoding: do_sample, num_beams > 1, use_cache=False, AFK_EXACT_FP32=1, logits processors
    (built-in or logits_processor=), the per-step hooks (stopping_criteria= / streamer=), stop strings, the output object - and k / ngram beyond the launches'
    caps.  (assistant_model= together with these keywords is refused by decode_assist.resolve.)"""
    from ._lib import AfkError

    gc = generation_config
    k, n = prompt_lookup_num_tokens, max_matching_ngram_size
    if gc is not None:
        if k is None:
            k = getattr(gc, "prompt_lookup_num_tokens", None)
        if n is None:
            n = getattr(gc, "max_matching_ngram_size", None)
    if k is None:
        return None
    if n is None:
        n = 2
    for v in (k, n):
        if isinstance(v, bool) or not isinstance(v, int):
            raise ValueError(f"`prompt_lookup_num_tokens` and `max_matching_ngram_size` have to be integers, but are {k!r} and {n!r}")
    if k <= 0 or n <= 0:
        raise ValueError(INVALID)
    if int(batch_size) != 1:
        raise ValueError(BATCH)
    for bad, what in ((bool(do_sample), "do_sample=True"), (int(num_beams) > 1, "num_beams > 1"), (not use_cache, "use_cache=False"),
                      (bool(exact_fp32), "AFK_EXACT_FP32=1"), (bool(processors), "logits processors (built-in or logits_processor=)"),
                      (bool(hooks), "stopping_criteria= / streamer="), (bool(stop_strings), "stop_strings="),
                      (bool(output_object), "return_dict_in_generate / output_scores / output_logits")):
        if bad:
            raise AfkError(f"generate(prompt_lookup_num_tokens=...) with {what}: prompt-lookup decoding runs greedy decoding of one sequence on the KV cache only")
    if k > MAX_K or n > MAX_NGRAM:
        raise AfkError(f"generate(prompt_lookup_num_tokens={k}, max_matching_ngram_size={n}): at most {MAX_K} drafted tokens per step and n-grams of at most {MAX_NGRAM}")
    return LookupSpec(k=int(k), ngram=int(n))


def build_state(spec: LookupSpec, ids, first_token, max_new_tokens: int, eos, state, H: int):
    """device state of one call for the prompt ids [1, S0] (exactly what generate() was given) and token 0 (first_token [1] int64, selected from the prefill's
    logits): ids [S0 + max_new] int32 = prompt, token 0; tokens [max_new] int64; status = {S0 + 1, 1, done, 0, 0, 0, 0, 0} with done set when token 0 is an eos
    id or max_new == 1; `state` = generate()'s [lo, key-range end, cache slot, position] tensor (advanced by accept); the step's rows / pos / krange / cand / sel,
    the embedding rows x [M, H] and the scratch.  One-time setup in torch ops, outside the captured step."""
    import torch

    S0, dev, M, max_new = ids.shape[1], ids.device, spec.k + 1, int(max_new_tokens)
    buf = torch.zeros(S0 + max_new, device=dev, dtype=torch.int32)
    buf[:S0] = ids[0]
    buf[S0] = first_token[0]
    tokens = torch.zeros(max_new, device=dev, dtype=torch.int64)
    tokens[0] = first_token[0]
    eos_t = torch.tensor(eos, device=dev, dtype=torch.int32) if eos else None
    done = torch.zeros((), device=dev, dtype=torch.int32) if max_new > 1 else torch.ones((), device=dev, dtype=torch.int32)
    if eos_t is not None:
        done = done | (first_token[0] == eos_t).any().to(torch.int32)
    status = torch.zeros(STATUS_WORDS, device=dev, dtype=torch.int32)
    status[LEN], status[EMITTED], status[DONE] = S0 + 1, 1, done
    z = lambda *shape, dtype=torch.int32: torch.zeros(shape, device=dev, dtype=dtype)
    return dict(spec=spec, S0=S0, max_new=max_new, M=M, ids=buf, tokens=tokens, status=status, state=state, eos=eos_t, eos_ids=tuple(eos or ()), cand=z(spec.k),
                rows=z(M, dtype=torch.int64), pos=z(M), krange=z(M, 2), sel=z(M), x=z(M, H, dtype=torch.bfloat16), ws=z(WS_WORDS))


def draft(ls, emb):
    """one afk_lookup_draft launch: the candidates of this step and the verify forward's inputs - ls["x"] (the embedding rows), ls["pos"], ls["krange"]"""
    from . import _lib, ops

    n_eos = 0 if ls["eos"] is None else ls["eos"].numel()
    _lib.call("afk_lookup_draft", ls["ids"].data_ptr(), ls["ids"].numel(), ls["status"].data_ptr(), ls["state"].data_ptr(), ls["spec"].k, ls["spec"].ngram,
              ls["max_new"], ops._p(ls["eos"]), n_eos, ls["cand"].data_ptr(), ls["rows"].data_ptr(), ls["pos"].data_ptr(), ls["krange"].data_ptr(),
              emb.data_ptr(), emb.stride(0), emb.shape[0], ls["x"].shape[1], ls["x"].data_ptr(), ls["x"].stride(0), ops._stream())


def accept(ls, logits):
    """one afk_lookup_accept call on the fp32 logits [M, V] of the verify forward: sel, the emitted tokens, the status words and the step state"""
    import torch

    from . import _lib, ops
    from ._lib import AfkError

    if logits.dtype != torch.float32 or logits.dim() != 2 or logits.shape[0] != ls["M"] or logits.stride(1) != 1:
        raise AfkError(f"decode_lookup.accept: fp32 logits [{ls['M']}, V] with unit column stride, got {logits.dtype} {tuple(logits.shape)} strides {logits.stride()}")
    n_eos = 0 if ls["eos"] is None else ls["eos"].numel()
    _lib.call("afk_lookup_accept", logits.data_ptr(), logits.stride(0), logits.shape[1], ls["M"], ls["cand"].data_ptr(), ls["ids"].data_ptr(), ls["ids"].numel(),
              ls["tokens"].data_ptr(), ls["max_new"], ls["status"].data_ptr(), ls["state"].data_ptr(), ops._p(ls["eos"]), n_eos, ls["sel"].data_ptr(),
              ls["ws"].data_ptr(), ops._stream())


# ------------------------------------------------------------------ the same two rules on the host (lookup_on_device = False)
def candidates(history, k: int, ngram: int, eos=(), budget=None):
    """afk_lookup_draft's rule on a list of ints -> the candidate ids (possibly none)"""
    n = len(history)
    if budget is not None and budget <= 0:
        return []
    for g in range(min(ngram, n - 1), 0, -1):
        tail = history[n - g:]
        for i in range(n - g):   # i + g < n: the continuation is not empty
            if history[i:i + g] == tail:
                cont = history[i + g:min(i + g + k, n)]
                for j, tok in enumerate(cont):
                    if tok in eos:
                        cont = cont[:j]
                        break
                return cont if budget is None else cont[:budget]
    return []


def draft_host(ls, emb):
    """draft() by host reads and torch ops: the same candidates, rows, positions, key ranges and embedding rows"""
    import torch

    st = ls["status"].tolist()
    hist = ls["ids"][:st[LEN]].tolist()
    cand = [] if st[DONE] else candidates(hist, ls["spec"].k, ls["spec"].ngram, ls["eos_ids"], ls["max_new"] - st[EMITTED] - 1)
    dev = ls["ids"].device
    rows = [hist[-1]] + cand + [hist[-1]] * (ls["spec"].k - len(cand))
    ls["status"][N_CAND] = len(cand)
    ls["cand"].copy_(torch.tensor(rows[1:], device=dev, dtype=torch.int32))
    ls["rows"].copy_(torch.tensor(rows, device=dev, dtype=torch.int64))
    lo, end, _, position = ls["state"].tolist()
    ar = torch.arange(ls["M"], device=dev, dtype=torch.int32)
    ls["pos"].copy_(position + ar)
    ls["krange"].copy_(torch.stack([torch.full_like(ar, lo), end + ar], -1))
    ls["x"].copy_(emb.index_select(0, ls["rows"].clamp(0, emb.shape[0] - 1)))


def accept_host(ls, logits):
    """accept() by torch.argmax and host arithmetic (rows with a NaN aside, where torch.argmax picks the NaN and the launch never does)"""
    st = ls["status"].tolist()
    if st[DONE]:
        return
    sel = logits.argmax(-1).tolist()
    cand = ls["cand"].tolist()
    n_match = 0
    while n_match < st[N_CAND] and cand[n_match] == sel[n_match]:
        n_match += 1
    e = min(n_match + 1, ls["max_new"] - st[EMITTED])
    hit = False
    for i in range(e):
        if sel[i] in ls["eos_ids"]:
            e, hit = i + 1, True
            break
    import torch

    new = torch.tensor(sel[:e], device=logits.device)
    ls["ids"][st[LEN]:st[LEN] + e] = new.to(torch.int32)
    ls["tokens"][st[EMITTED]:st[EMITTED] + e] = new
    ls["sel"].copy_(torch.tensor(sel, device=logits.device, dtype=torch.int32))
    ls["state"][1:4] += e
    upd = [st[LEN] + e, st[EMITTED] + e, int(hit or st[EMITTED] + e >= ls["max_new"]), st[N_CAND], st[STEPS] + 1, st[ACCEPTED] + min(n_match, e),
           st[REJECTING] + int(n_match < st[N_CAND]), n_match]
    ls["status"].copy_(torch.tensor(upd, device=logits.device, dtype=torch.int32))

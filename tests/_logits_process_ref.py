"""Plain numpy / torch restatement of the contract of afk_decode_process (include/afk.h, steps 1-3), the reference's own processor chain on CPU, and the
case grid both GPU and CPU tests walk.  Everything is exact: one IEEE fp32 multiply or divide, or a store of -inf, on identical inputs - comparisons are
bit for bit (`bits`)."""
import functools

import numpy as np
import torch

VS, S0S, TS, GS, B = (1, 33, 256, 1000), (1, 2, 5, 40), (0, 1, 3), (0, 1, 2, 3, 7), 3
PENALTIES = (1.0, 1.3, 0.7)
MIN_NEW = 2
NINF = float("-inf")


def bits(x):
    return x.contiguous().view(torch.int32)


def restated(logits, ids, t, *, penalty=1.0, ngram=0, suppress=(), begin_suppress=(), eos=(), min_new_tokens=0):
    """steps 1-3 on logits [B, V] fp32 for the histories ids [B, n] (prompt + the t tokens selected so far) -> a new tensor"""
    x = logits.detach().cpu().numpy().astype(np.float32).copy()
    h = ids.detach().cpu().numpy()
    p = np.float32(penalty)
    rows, n = h.shape
    V = x.shape[1]
    for b in range(rows):
        for i in sorted(set(int(v) for v in h[b])):          # the seen set: once per distinct id
            x[b, i] = x[b, i] * p if x[b, i] < 0 else x[b, i] / p
        g = ngram
        if g > 0 and n + 1 >= g:
            tail = tuple(h[b, n - g + 1:])
            for j in range(0, n - g + 1):
                if tuple(h[b, j:j + g - 1]) == tail:
                    x[b, int(h[b, j + g - 1])] = NINF
        banned = list(suppress) + (list(begin_suppress) if t == 0 else []) + (list(eos) if t < min_new_tokens else [])
        for i in banned:
            if 0 <= i < V:
                x[b, i] = NINF
    return torch.from_numpy(x)


def reference_chain(logits, ids, S0, *, penalty=1.0, ngram=0, suppress=(), begin_suppress=(), eos=(), min_new_tokens=0, device="cpu"):
    """the reference's classes in the order GenerationMixin._get_logits_processor chains them, as a LogitsProcessorList on `device`"""
    from transformers import (LogitsProcessorList, MinNewTokensLengthLogitsProcessor, NoRepeatNGramLogitsProcessor, RepetitionPenaltyLogitsProcessor,
                              SuppressTokensAtBeginLogitsProcessor, SuppressTokensLogitsProcessor)

    chain = [RepetitionPenaltyLogitsProcessor(float(penalty))]
    if ngram > 0:
        chain.append(NoRepeatNGramLogitsProcessor(ngram))
    if min_new_tokens > 0 and eos:
        chain.append(MinNewTokensLengthLogitsProcessor(S0, min_new_tokens, list(eos), device=device))
    if suppress:
        chain.append(SuppressTokensLogitsProcessor(list(suppress), device=device))
    if begin_suppress:
        chain.append(SuppressTokensAtBeginLogitsProcessor(list(begin_suppress), S0, device=device))
    chain = LogitsProcessorList(chain)
    return chain if logits is None else chain(ids, logits.clone())


@functools.lru_cache(maxsize=None)
def case(V, S0, t, g):
    """-> (logits [B, V] fp32 bf16-valued with a 0.0, a -inf and a -0.0 planted on ids of the history, ids [B, S0 + t], keyword dict).  The ids come from
    fewer than 12 values, so duplicates and repeated n-grams are the rule; the penalty cycles with the case."""
    k = (VS.index(V) * len(S0S) + S0S.index(S0)) * len(TS) * len(GS) + TS.index(t) * len(GS) + GS.index(g)
    gen = torch.Generator().manual_seed(1000 + k)
    pool = torch.randperm(V, generator=gen)[: min(V, 11)]
    ids = pool[torch.randint(0, pool.numel(), (B, S0 + t), generator=gen)]
    logits = (torch.randn((B, V), generator=gen) * 4.0).to(torch.bfloat16).float()
    for b in range(B):
        targets = list(dict.fromkeys(ids[b].tolist() + list(range(min(V, 3)))))[:3]   # three distinct ids, those the row has seen first
        for v, i in zip((-0.0, NINF, 0.0), targets):
            logits[b, i] = v
    kw = dict(penalty=PENALTIES[k % 3], ngram=g, suppress=(V // 3,), begin_suppress=(V // 5, V - 1), eos=(V // 2, (V // 7 + 1) % V), min_new_tokens=MIN_NEW)
    return logits, ids, kw


def grid():
    return [(V, S0, t, g) for V in VS for S0 in S0S for t in TS for g in GS]

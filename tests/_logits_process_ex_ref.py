"""Plain numpy restatement of the nine-stage contract of afk_decode_process_ex (include/afk.h), the reference's own processor classes chained in
GenerationMixin._get_logits_processor's order on CPU, and the case grid the CPU and GPU tests walk.  Everything is exact - IEEE fp32 adds, multiplies and
divides in a fixed order, or stores of -inf / 0.0, on identical inputs - so comparisons are bit for bit (`bits`)."""
import functools

import numpy as np
import torch

MAX_NEW = 6
VS, S0S, TS, B = (1, 33, 256, 1000), (1, 2, 5, 40), (0, 1, 3, MAX_NEW - 1), 3
PENALTIES, NGRAMS = (1.0, 1.3, 0.7), (0, 2, 3)
NINF, INF = float("-inf"), float("inf")
F = np.float32
EX_KEYS = ("sequence_bias", "bad_words_ids", "min_length", "forced_eos", "decay")
OFF = dict(penalty=1.0, ngram=0, suppress=(), begin_suppress=(), eos=(), min_new_tokens=0, sequence_bias=None, bad_words_ids=None, min_length=0, forced_eos=(),
           decay=None)


def bits(x):
    return x.contiguous().view(torch.int32)


def _bias_stage(x, h, seqs):
    """x = x + acc on every entry; acc[id] = 0.0f + the one-id bias, then + (match ? bias : 0.0f) for the longer sequences that end in id, in the given order"""
    n = len(h)
    acc = np.zeros(x.shape[0], dtype=F)
    for ids, bias in seqs:
        if len(ids) == 1:
            acc[ids[0]] = F(0.0) + F(bias)
    for ids, bias in seqs:
        L = len(ids)
        if L >= 2:
            hit = L <= n and tuple(h[n - (L - 1):]) == tuple(ids[:-1])
            acc[ids[-1]] = acc[ids[-1]] + (F(bias) if hit else F(0.0))
    return x + acc


def restated(logits, ids, t, *, max_new=MAX_NEW, penalty=1.0, ngram=0, suppress=(), begin_suppress=(), eos=(), min_new_tokens=0, sequence_bias=None,
             bad_words_ids=None, min_length=0, forced_eos=(), decay=None):
    """the nine stages on logits [B, V] fp32 for the histories ids [B, n] (prompt + the t tokens selected so far, n = cur_len) -> a new tensor"""
    x = logits.detach().cpu().numpy().astype(F).copy()
    h = ids.detach().cpu().numpy()
    rows, n = h.shape
    V = x.shape[1]
    p = F(penalty)
    bad = None
    if bad_words_ids is not None:   # [eos] sequences are filtered out; duplicates count once
        bad = [(w, NINF) for w in dict.fromkeys(tuple(w) for w in bad_words_ids if all(list(w) != [e] for e in eos))]
    with np.errstate(invalid="ignore", over="ignore"):
        for b in range(rows):
            hb = [int(v) for v in h[b]]
            if sequence_bias is not None:                                                        # 1
                x[b] = _bias_stage(x[b], hb, list(sequence_bias.items()))
            for i in sorted(set(hb)):                                                            # 2: once per distinct id
                x[b, i] = x[b, i] * p if x[b, i] < 0 else x[b, i] / p
            g = ngram                                                                            # 3
            if g > 0 and n + 1 >= g:
                tail = tuple(hb[n - g + 1:])
                for j in range(0, n - g + 1):
                    if tuple(hb[j:j + g - 1]) == tail:
                        x[b, hb[j + g - 1]] = NINF
            if bad is not None:                                                                  # 4
                x[b] = _bias_stage(x[b], hb, bad)
            if eos and (n < min_length or t < min_new_tokens):                                   # 5, 6
                for i in eos:
                    if 0 <= i < V:
                        x[b, i] = NINF
            if forced_eos and t == max_new - 1:                                                  # 7
                x[b, :] = NINF
                for i in forced_eos:
                    x[b, i] = 0.0
            if decay is not None and eos and t > decay[0]:                                       # 8
                c = F(pow(decay[1], t - decay[0]) - 1)
                old = x[b].copy()
                x[b] = old + F(0.0)
                for i in set(eos):
                    x[b, i] = old[i] + np.abs(old[i]) * c
            for i in list(suppress) + (list(begin_suppress) if t == 0 else []):                  # 9
                if 0 <= i < V:
                    x[b, i] = NINF
    return torch.from_numpy(x)


def reference_chain(logits, ids, S0, *, max_new=MAX_NEW, penalty=1.0, ngram=0, suppress=(), begin_suppress=(), eos=(), min_new_tokens=0, sequence_bias=None,
                    bad_words_ids=None, min_length=0, forced_eos=(), decay=None, device="cpu"):
    """the reference's classes in the order GenerationMixin._get_logits_processor chains them (utils.py:1154-1290), as a LogitsProcessorList on `device`; the
    processors are built on the conditions that method builds them on"""
    from transformers import (ExponentialDecayLengthPenalty, ForcedEOSTokenLogitsProcessor, LogitsProcessorList, MinLengthLogitsProcessor,
                              MinNewTokensLengthLogitsProcessor, NoBadWordsLogitsProcessor, NoRepeatNGramLogitsProcessor, RepetitionPenaltyLogitsProcessor,
                              SequenceBiasLogitsProcessor, SuppressTokensAtBeginLogitsProcessor, SuppressTokensLogitsProcessor)

    eos_t = torch.tensor(list(eos), device=device) if eos else None
    chain = []
    if sequence_bias is not None:
        chain.append(SequenceBiasLogitsProcessor(sequence_bias=dict(sequence_bias)))
    if penalty != 1.0:
        chain.append(RepetitionPenaltyLogitsProcessor(float(penalty)))
    if ngram > 0:
        chain.append(NoRepeatNGramLogitsProcessor(ngram))
    if bad_words_ids is not None:
        chain.append(NoBadWordsLogitsProcessor([list(w) for w in bad_words_ids], eos_t))
    if min_length > 0 and eos:
        chain.append(MinLengthLogitsProcessor(min_length, eos_t, device=device))
    if min_new_tokens > 0 and eos:
        chain.append(MinNewTokensLengthLogitsProcessor(S0, min_new_tokens, eos_t, device=device))
    if forced_eos:
        chain.append(ForcedEOSTokenLogitsProcessor(S0 + max_new, list(forced_eos), device=device))
    if decay is not None:
        chain.append(ExponentialDecayLengthPenalty(tuple(decay), eos_t, S0))
    if suppress:
        chain.append(SuppressTokensLogitsProcessor(list(suppress), device=device))
    if begin_suppress:
        chain.append(SuppressTokensAtBeginLogitsProcessor(list(begin_suppress), S0, device=device))
    chain = LogitsProcessorList(chain)
    return chain if logits is None else chain(ids, logits.clone())


def spec_of(kw, max_new=MAX_NEW):
    """the ProcessSpec of a case's keywords, through the resolver"""
    from audio_flamingo_amd.decode_process import resolve

    return resolve(repetition_penalty=float(kw["penalty"]), no_repeat_ngram_size=kw["ngram"], min_new_tokens=kw["min_new_tokens"],
                   suppress_tokens=list(kw["suppress"]) or None, begin_suppress_tokens=list(kw["begin_suppress"]) or None, eos_token_id=list(kw["eos"]) or None,
                   sequence_bias=kw["sequence_bias"], bad_words_ids=kw["bad_words_ids"], min_length=kw["min_length"],
                   forced_eos_token_id=list(kw["forced_eos"]) or None, exponential_decay_length_penalty=kw["decay"])


@functools.lru_cache(maxsize=None)
def case(V, S0, t):
    """-> (logits [B, V] fp32, ids [B, S0 + t], keywords of all ten processors).  The ids come from at most 11 values and rows 0 and 1 share their last four,
    and the sequences of both tables are cut from that tail, so suffix matches are the rule; row 2 matches by chance.  The tables hold one-id, 2-, 3- and 5-id
    sequences (the 5-id one is longer than a short history), a 50-id sequence no history reaches, three sequences on one last id whose biases (1, 1e8, -1e8) do
    not sum associatively in fp32, a +inf bias on an id whose logit is -inf, a bad word equal to [eos] and one that ends in an eos id.  A -0.0, a 0.0, a -inf
    and a +inf logit sit on ids the tables touch.  min_length, the decay start and the penalty / n-gram size cycle with the case so that both sides of every
    threshold occur; t == MAX_NEW - 1 is the forced step."""
    k = (VS.index(V) * len(S0S) + S0S.index(S0)) * len(TS) + TS.index(t)
    gen = torch.Generator().manual_seed(7000 + k)
    pool = torch.randperm(V, generator=gen)[: min(V, 11)].tolist()
    a = [pool[i % len(pool)] for i in range(11)]
    n = S0 + t
    ids = torch.tensor(pool)[torch.randint(0, len(pool), (B, n), generator=gen)]
    m = min(4, n)
    ids[1, n - m:] = ids[0, n - m:]
    T = ids[0].tolist()
    tail = lambda L, fallback: tuple(T[n - L:]) if n >= L else tuple(fallback)
    sb = {}
    sb[(a[0],)] = 2.5
    sb[tail(1, (a[1],)) + (a[1],)] = -1.25
    sb[tail(2, (a[3], a[4])) + (a[2],)] = 0.75
    sb[tail(4, (a[0], a[1], a[2], a[4])) + (a[3],)] = -3.0
    sb[(a[5],)] = 1.0
    sb[tail(1, (a[0],)) + (a[5],)] = 1.0e8
    sb[tail(2, (a[0], a[1])) + (a[5],)] = -1.0e8
    sb[(a[6],)] = INF
    sb[tuple(a[i % 11] for i in range(50))] = 5.0
    eos = (a[9], a[10])
    bad = [[eos[0]], list(tail(1, (a[2],))) + [eos[1]], [a[7]], list(tail(2, (a[1], a[0]))) + [a[8]], list(tail(4, (a[4], a[3], a[2], a[1]))) + [a[4]],
           list(tail(1, (a[6],))) + [a[2]], [a[7]]]
    logits = (torch.randn((B, V), generator=gen) * 4.0).to(torch.bfloat16).float()
    for v, i in ((-0.0, a[8]), (0.0, a[1]), (NINF, a[6]), (INF, a[7])):   # later plants win where a small vocabulary makes the ids collide
        logits[:, i] = v
    logits[2, a[3]] = -0.0
    kw = dict(penalty=PENALTIES[k % 3], ngram=NGRAMS[(k // 3) % 3], suppress=(V // 3, a[4]), begin_suppress=(V // 5, V - 1), eos=eos, min_new_tokens=2,
              sequence_bias=sb, bad_words_ids=bad, min_length=n + (k % 2), forced_eos=(eos[0], a[4]), decay=(t - (k // 2) % 2, 1.37))
    return logits, ids, kw


def grid():
    return [(V, S0, t) for V in VS for S0 in S0S for t in TS]


def alone(kw, name):
    """the keywords with only the new processor `name` on (eos stays where it needs it)"""
    out = dict(OFF, **{name: kw[name]})
    if name in ("min_length", "decay", "bad_words_ids"):
        out["eos"] = kw["eos"]
    return out

"""Plain-integer (numpy) restatement of the two launches of prompt-lookup decoding, afk_lookup_draft and afk_lookup_accept (include/afk.h holds the contract):
what the GPU tests compare the kernels with, exactly, and what tests/test_decode_lookup_cpu.py pins to the reference's own PromptLookupCandidateGenerator and to
the greedy branch of _assisted_decoding.  Written for clarity, one window at a time; nothing here is shared with the code under test."""
import numpy as np

LEN, EMITTED, DONE, N_CAND, STEPS, ACCEPTED, REJECTING, N_MATCH = range(8)
STATUS_WORDS = 8


def candidates(history, k, ngram, eos=()):
    """get_candidates (candidate_generator.py:1057-1150) on a list of ints -> the new candidate ids.  For g from min(ngram, len - 1) down to 1 the leftmost
    window equal to the last g ids whose continuation (at most k ids, inside the history) is not empty decides; the continuation is cropped in front of its
    first eos id, and an empty crop means no candidates at all."""
    n = len(history)
    for g in range(min(ngram, n - 1), 0, -1):
        for i in range(n - g + 1):
            if history[i:i + g] != history[n - g:]:
                continue
            cont = history[i + g:min(i + g + k, n)]
            if not cont:
                continue   # the trailing window
            for j, tok in enumerate(cont):
                if tok in eos:
                    return list(cont[:j])
            return list(cont)
    return []


def new_status(length, emitted=1, done=0):
    st = np.zeros(STATUS_WORDS, dtype=np.int32)
    st[LEN], st[EMITTED], st[DONE] = length, emitted, done
    return st


def draft(ids, status, state, k, ngram, max_new, eos=()):
    """afk_lookup_draft: status[N_CAND] is written; -> dict(cand [k], rows [k + 1], pos [k + 1], krange [k + 1, 2])"""
    n = int(status[LEN])
    hist = [int(v) for v in ids[:n]]
    budget = max_new - int(status[EMITTED]) - 1
    cand = [] if (status[DONE] or budget <= 0) else candidates(hist, k, ngram, eos)[:budget]
    status[N_CAND] = len(cand)
    last = hist[-1]
    full = cand + [last] * (k - len(cand))
    j = np.arange(k + 1, dtype=np.int32)
    return dict(cand=np.asarray(full, dtype=np.int32), rows=np.asarray([last] + full, dtype=np.int64), pos=(state[3] + j).astype(np.int32),
                krange=np.stack([np.full(k + 1, state[0], dtype=np.int32), (state[1] + j).astype(np.int32)], -1))


def argmax_row(z):
    """afk_decode_select_greedy's conventions: the largest value, ties to the lowest id, a NaN is never picked, nothing finite (or only -inf) -> 0"""
    z = np.where(np.isnan(z), -np.inf, z.astype(np.float32))
    return int(np.argmax(z)) if np.max(z) > -np.inf else 0


def accept(logits, cand, ids, tokens, status, state, max_new, eos=()):
    """afk_lookup_accept, in place on ids / tokens / status / state -> sel [M] (None when done was set: nothing is written)"""
    if status[DONE]:
        return None
    M = logits.shape[0]
    sel = [argmax_row(logits[j]) for j in range(M)]
    n_cand = int(status[N_CAND])
    n_match = 0
    while n_match < n_cand and int(cand[n_match]) == sel[n_match]:
        n_match += 1
    n, emitted = int(status[LEN]), int(status[EMITTED])
    e = min(n_match + 1, max_new - emitted)
    hit = False
    for i in range(e):
        if sel[i] in eos:
            e, hit = i + 1, True
            break
    ids[n:n + e] = sel[:e]
    tokens[emitted:emitted + e] = sel[:e]
    status[LEN], status[EMITTED] = n + e, emitted + e
    status[DONE] = int(hit or emitted + e >= max_new)
    status[STEPS] += 1
    status[ACCEPTED] += min(n_match, e)
    status[REJECTING] += int(n_match < n_cand)
    status[N_MATCH] = n_match
    state[1:4] += e
    return np.asarray(sel, dtype=np.int32)

"""Plain-integer restatement of the two launches of assisted decoding, afk_assist_begin and afk_assist_stage (include/afk.h holds the contract), and of the
step they stand in: what the GPU tests compare the kernels with, exactly.  Written for clarity on Python lists; nothing here is shared with the code under test.
The accept rule is prompt-lookup decoding's (tests/_lookup_ref.accept)."""
import numpy as np

from tests._lookup_ref import DONE, EMITTED, LEN, N_CAND


def kept(drafts, eos=(), budget=None, done=False):
    """the number of leading drafts that become candidates: all of them, cut BEHIND the first eos id (the eos itself stays: the draft model would have stopped
    there and the target may confirm it), cut to budget = max_new - emitted - 1; none when the call is done"""
    if done:
        return 0
    out = []
    for tok in drafts:
        out.append(tok)
        if tok in eos:
            break
    if budget is not None:
        out = out[:max(budget, 0)]
    return len(out)


def begin(ids, status, state, vocab):
    """afk_assist_begin -> (dstate, the id whose embedding row the draft model runs first)"""
    last = int(ids[int(status[LEN]) - 1])
    return np.asarray(state, dtype=np.int32).copy(), min(max(last, 0), vocab - 1)


def stage(ids, status, state, draft, k, max_new, eos=()):
    """afk_assist_stage: status[N_CAND] is written; -> dict(cand [k], rows [k + 1], pos [k + 1], krange [k + 1, 2]).  draft: the draft model's token buffer,
    drafted token j of this step at draft[state[2] + j]"""
    last = int(ids[int(status[LEN]) - 1])
    cur = int(state[2])
    drafts = [int(v) for v in draft[cur:cur + k]]
    n = kept(drafts, eos, max_new - int(status[EMITTED]) - 1, bool(status[DONE]))
    status[N_CAND] = n
    full = drafts[:n] + [last] * (k - n)
    j = np.arange(k + 1, dtype=np.int32)
    return dict(cand=np.asarray(full, dtype=np.int32), rows=np.asarray([last] + full, dtype=np.int64), pos=(state[3] + j).astype(np.int32),
                krange=np.stack([np.full(k + 1, state[0], dtype=np.int32), (state[1] + j).astype(np.int32)], -1))


def simulate(prompt, target, draft_model, k, max_new, eos=(), extra_pass=True):
    """assisted greedy decoding on the host for two scripted models - target(history) / draft_model(history) -> the next id after a list of ids.
    -> (the emitted ids, stats).  The draft model keeps a cache: `seen` is the number of history positions whose keys it holds, and it can only run a
    token whose predecessors it has all seen (the assertion is the reason for the extra pass behind the last draft; extra_pass=False leaves it out)."""
    hist = list(prompt)
    out = [target(hist)]
    hist.append(out[0])
    seen = len(prompt)   # the prefill
    stats = dict(steps=0, accepted=0, rejecting=0, drafted=0)
    done = out[0] in eos or max_new == 1
    while not done:
        # the draft model: k steps from the last emitted token, then one more pass for the last draft's keys
        work = list(hist)
        seen = min(seen, len(hist) - 1)   # the rewind: slots behind the accepted sequence are stale
        drafts = []
        for j in range(k):
            assert seen == len(work) - 1, "the draft model runs a token behind a hole in its cache"
            seen += 1   # the keys of work[-1]
            drafts.append(draft_model(work))
            work.append(drafts[-1])
        seen += int(extra_pass)   # the extra pass: the keys of the last draft
        n_cand = kept(drafts, eos, max_new - len(out) - 1)
        # the verify forward: row j is the target's answer behind hist + drafts[:j]
        sel = [target(hist + drafts[:j]) for j in range(k + 1)]
        n_match = 0
        while n_match < n_cand and drafts[n_match] == sel[n_match]:
            n_match += 1
        e = min(n_match + 1, max_new - len(out))
        for i in range(e):
            if sel[i] in eos:
                e, done = i + 1, True
                break
        out += sel[:e]
        hist += sel[:e]
        done = done or len(out) >= max_new
        stats["steps"] += 1
        stats["accepted"] += min(n_match, e)
        stats["rejecting"] += int(n_match < n_cand)
        stats["drafted"] += k
    return out, stats

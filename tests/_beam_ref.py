"""A numpy restatement of afk_beam_step's contract (include/afk.h) - one beam-search step, and the loop around it - which tests/test_beam_cpu.py pins to
GenerationMixin's own helpers and tests/test_beam_gpu.py compares the kernel with.  Plain loops over rows and candidates: nothing here is clever on purpose.

Where the reference leaves an order open (torch.topk among equal scores) the contract fixes one, and this file states it: among continuations the lower flat
index beam * V + token first; among [finished slots, candidates] and among the candidates the earlier position first."""
import numpy as np

GATE = np.float32(-1.0e9)
F32 = np.float32


def tables(max_new, length_penalty, early_stopping):
    """div[t] = float32((t + 1) ** length_penalty) and the heuristic's divisor, both computed in double"""
    div = np.array([float((t + 1) ** float(length_penalty)) for t in range(max_new)], dtype=np.float64).astype(F32)
    if early_stopping == "never" and length_penalty > 0.0:
        return div, np.full(max_new, float(max_new ** float(length_penalty)), dtype=np.float64).astype(F32)
    return div, div.copy()


def new_state(B, nb, max_new):
    run_score = np.full((B, nb), GATE, dtype=F32)
    run_score[:, 0] = 0.0
    return dict(run_score=run_score, run_seq=np.zeros((B, nb, max_new), dtype=np.int64), fin_score=np.full((B, nb), GATE, dtype=F32),
                fin_len=np.zeros((B, nb), dtype=np.int64), fin_done=np.zeros((B, nb), dtype=bool), fin_seq=np.zeros((B, nb, max_new), dtype=np.int64),
                can_improve=np.ones(B, dtype=bool), next_token=np.zeros(B * nb, dtype=np.int64), src=np.arange(B * nb, dtype=np.int64),
                status=np.array([-1, 1], dtype=np.int64))


def scores_of(logits, run_score):
    """[B * nb, V] fp32 logits -> accumulated log-probabilities [B * nb, V] fp32: log_softmax (NaN counts as -inf; the sum in double, rounded once), then the
    fp32 add of the beam's running score; a NaN result, and a row with no finite maximum, count as -inf"""
    z = np.where(np.isnan(logits), -np.inf, logits).astype(F32)
    zmax = z.max(-1, keepdims=True)
    ok = np.isfinite(zmax)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        d = (z - np.where(ok, zmax, 0)).astype(F32)
        lsum = np.log(np.exp(d.astype(np.float64)).sum(-1, keepdims=True)).astype(F32)
        s = ((d - lsum).astype(F32) + run_score.reshape(-1, 1).astype(F32)).astype(F32)
    s = np.where(ok & ~np.isnan(s), s, -np.inf).astype(F32)
    return s + F32(0)   # -0 -> +0


def _ranked(values, k):
    """positions of the k largest, equal values in ascending position"""
    return np.argsort(-values.astype(np.float64), kind="stable")[:k]


def step(st, logits, t, *, nb, max_new, eos, early_stopping, div, hdiv, trace=None):
    """token t for every row, in place.  trace (a dict): receives `top` = the row-wise sorted scores of the best keep + 1 continuations (how sharp the step's
    ranking is) and `ended` = whether a top-nb candidate ended in front of the length limit"""
    if t < 0 or t >= max_new or st["status"][1] == 0:
        return st
    B = st["run_score"].shape[0]
    V = logits.shape[1]
    keep = (len(eos) + 1) * nb
    assert keep <= nb * V
    last = t + 1 == max_new
    sc = scores_of(logits, st["run_score"]).reshape(B, nb * V)
    inv_div, inv_hdiv = F32(1) / div[t], F32(1) / hdiv[t]
    rows_ci, rows_done = [], []
    for b in range(B):
        order = _ranked(sc[b], min(keep + 1, nb * V))
        if trace is not None:
            trace.setdefault("top", []).append(sc[b][order].copy())
        order = order[:keep]
        cs, parent, tok = sc[b][order], order // V, order % V
        ends = np.array([last or int(x) in eos for x in tok])
        if trace is not None:
            trace.setdefault("ended", []).append(bool((ends[:nb] & (not last)).any()))
        cand_seq = st["run_seq"][b][parent].copy()
        cand_seq[:, t] = tok
        # finished slots
        full = bool(st["fin_done"][b].all()) and early_stopping is True
        ms = np.empty(2 * nb, dtype=F32)
        ms[:nb] = st["fin_score"][b]
        for c in range(nb):
            s = F32(cs[c] * inv_div)
            if full or not st["can_improve"][b] or not ends[c]:
                s = F32(s + GATE)
            ms[nb + c] = s
        pick = _ranked(ms, nb)
        st["fin_seq"][b] = np.concatenate([st["fin_seq"][b], cand_seq[:nb]])[pick]
        st["fin_len"][b] = np.concatenate([st["fin_len"][b], np.full(nb, t + 1)])[pick]
        st["fin_done"][b] = np.concatenate([st["fin_done"][b], ends[:nb]])[pick]
        st["fin_score"][b] = ms[pick]
        # running beams
        rs = np.where(ends, (cs + GATE).astype(F32), cs).astype(F32)
        run = _ranked(rs, nb)
        st["run_seq"][b], st["run_score"][b] = cand_seq[run], rs[run]
        st["next_token"][b * nb:(b + 1) * nb] = tok[run]
        st["src"][b * nb:(b + 1) * nb] = b * nb + parent[run]
        if not last:
            best = F32(st["run_score"][b, 0] * inv_hdiv)
            worst = np.where(st["fin_done"][b], st["fin_score"][b].min(), GATE)
            st["can_improve"][b] = bool(st["can_improve"][b]) and bool((best > worst).any())
        rows_ci.append(bool(st["can_improve"][b])), rows_done.append(bool(st["fin_done"][b].all()))
    is_open = (not last) and any(rows_ci) and not (early_stopping is True and all(rows_done))
    if not is_open:
        st["src"][:] = np.arange(B * nb)
    st["status"][:] = (t, int(is_open))
    return st


def search(logits_of, B, nb, max_new, *, eos=(), length_penalty=1.0, early_stopping=False):
    """the loop: logits_of(t, next_token, src) -> [B * nb, V] fp32 for token t (next_token / src of the step before; None for token 0) -> the final state"""
    st = new_state(B, nb, max_new)
    div, hdiv = tables(max_new, length_penalty, early_stopping)
    for t in range(max_new):
        step(st, logits_of(t, None if t == 0 else st["next_token"].copy(), None if t == 0 else st["src"].copy()), t, nb=nb, max_new=max_new, eos=tuple(eos),
             early_stopping=early_stopping, div=div, hdiv=hdiv)
        if st["status"][1] == 0:
            break
    return st


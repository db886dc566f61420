"""Planted-key probes of the attention kernels' masks, key ranges and decode splits (pure torch, CPU or GPU; imported like tests/_tol.py).

Most attention bugs are off by one: a kernel sees one key too many or too few at a range end, on the causal diagonal, at a 64 / 128 tile edge,
at a split-KV chunk edge, in the wrong KV head of a GQA group or in the neighbouring sample.  N(0, 1) inputs hide that: over a long range one key
moves a row by less than any sensible tolerance.  Here every boundary that matters carries a PLANTED key:

  background  q, k ~ 0.3 N(0, 1), v ~ N(0, 1);
  plant       key j of KV head hk and one or more query rows of the heads of hk's group point along a unit vector u of their own (an orthonormal
              basis per KV head, a different basis for every KV head, a different vector for every plant).  Their logit is L = ln(n) + 4, n the
              longest visible range of the case; background logits are O(0.3), so key j takes most of the row's softmax.  v_j = 4 x a sign pattern;
  probe       a planted (row, key) pair the row must SEE: dropping the key moves the row by O(1);
  decoy       a planted (row, key) pair the row must NOT see: including the key moves the row by O(1).
A decode query has one row per head, so its planted keys are spread over the heads of the sample and one query can carry several of them (q = the
sum of a u over them, no background: every planted key then gets the same logit L and an equal share of the row).

A case holds the bf16 inputs, the probed slots, the fp64 reference of the true masks and MUTATED references: the same inputs with a range end moved by
one, the causal diagonal moved by one, one split-KV chunk edge key dropped, query heads routed to the wrong KV head, the neighbouring sample's first
key made visible.  Column Sk of every visibility mask is the first key of sample (b + 1) % B - what a flat read one row past the end of sample b
returns - so "one key past the end" needs no special case.  tests/test_attn_probe_cpu.py checks that every mutation lands >= SEP x the bar away from
the truth on the probed slots; tests/test_attn_edges_gpu.py holds the kernels to the bar (bar() below; the justification is in its docstring)."""
import math

import torch

BAR_REL = 2.0 ** -6     # ||got - ref||_2 <= BAR_REL * ||ref||_2 + BAR_ABS * sqrt(D) on every probed (row, head) or (key, KV head) slice
BAR_ABS = 2.0 ** -8
SEP = 8.0               # every mutation must move at least one probed slice by SEP x its bar
TILE_KEYS = (63, 64, 127, 128)
LOGIT_MARGIN = 4.0      # planted logit L = ln(n) + LOGIT_MARGIN


def bar(ref_norm, D, rel=BAR_REL):
    """the per-slice bar.  Forward: the output is rounded to bf16 once (<= 2^-9 relative per element) and the LDS kernels round P to bf16 before P.V
    (<= 2^-9 relative per term of a sum of non-negative weights: <= 2^-9 * sum_j p_j |v_j|, about 2^-9 ||o|| on a probed row, which one key dominates):
    2^-8 in all, and the bar 2^-6 leaves 4x.  Gradients: dO is a bf16 input, P and dS = P o (dP - delta) are rounded to bf16 before their MFMAs and
    the reference takes delta = rowsum(dO o O) from the bf16 O the backward is given, as the kernels do (attend(): on a row one key dominates, the
    rounding of O alone would otherwise move dQ by several times the bar) - again a few 2^-9 relative terms.  The floor 2^-8 sqrt(D) (one bf16
    half-ulp per element at unit scale) covers slices whose own norm is at the rounding level: rows that average many background values, dK of keys
    no row favours."""
    return rel * ref_norm + BAR_ABS * math.sqrt(D)


# ------------------------------------------------------------------------------------------------ the fp64 reference
def attend(q, k, v, vis, hmap, scale, do=None, rows=None, o_bwd=None):
    """fp64 softmax attention.  q [B, Hq, Sq, D]; k, v [B, Hkv, Sk, D]; vis bool broadcastable to [B, Hq, Sq, Sk + 1] (column Sk: the first key of
    sample (b + 1) % B); hmap [Hq] long: the KV head of every query head.  A row that sees no key is a zero row.  rows: only these query rows
    (forward only).  -> o [B, Hq, Sq, D]; with do [B, Hq, Sq, D]: (o, dq, dk, dv), the gradients of sum(o * do).
    o_bwd: the (bf16) output the backward is GIVEN.  A FlashAttention backward forms delta_i = rowsum(dO_i o O_i) from it, and on a row that one key
    dominates dS = P o (dP - delta) cancels to (1 - p) of its terms, so the 2^-9 rounding of O moves dQ / dK by far more than 2^-9 of their norm.
    With o_bwd the reference takes delta from that output too - the exact backward of the attention given its stored forward: the gradient of
    sum(o * do) - sum_i (delta_given_i - delta_i) * logsumexp_i(s), since d logsumexp_i / d s_ij = p_ij."""
    grad = do is not None
    q, k, v = (t.detach().double().requires_grad_(grad) for t in (q, k, v))
    B, Hq, Sq, D = q.shape
    Sk = k.shape[2]
    vis = vis.expand(B, Hq, Sq, Sk + 1)
    qq = q if rows is None else q[:, :, rows]
    if rows is not None:
        vis = vis[:, :, rows]
    vx = _ext(v, hmap)
    o, s, has = _masked_softmax_v((qq @ _ext(k, hmap).transpose(-1, -2)) * scale, vis, vx)
    if not grad:
        return o.detach()
    loss = (o * do.double()).sum()
    if o_bwd is not None:
        dd = ((o_bwd.double() - o.detach()) * do.double()).sum(-1, keepdim=True)
        loss = loss - (dd * torch.where(has, torch.logsumexp(s, -1, keepdim=True), torch.zeros_like(dd))).sum()
    loss.backward()
    return o.detach(), q.grad, k.grad, v.grad


def _ext(t, hmap):
    """[B, Hkv, Sk, D] -> [B, Hq, Sk + 1, D]: key Sk is the first key of sample (b + 1) % B, KV head hmap[h] for query head h"""
    return torch.cat([t, t.roll(-1, 0)[:, :, :1]], 2)[:, hmap]


def _masked_softmax_v(s, vis, vx):
    """-> (softmax(s masked by vis) @ vx with zero rows where nothing is visible, the masked scores, the row mask)"""
    has = vis.any(-1, keepdim=True)
    s = torch.where(has, torch.where(vis, s, torch.tensor(float("-inf"), dtype=s.dtype, device=s.device)), torch.zeros((), dtype=s.dtype, device=s.device))
    return (torch.softmax(s, -1) * has) @ vx, s, has


class Case:
    """inputs (canonical [B, H, S, D] bf16 views), probed slots and the true / mutated visibility.  rows: probed (b, h, i) query slots; keys: planted
    (b, hk, j) key slots (j < Sk); mutations: name -> (vis, hmap) - only those whose mask or head map differs from the truth are kept."""

    def __init__(self, q, k, v, vis, hmap, scale, rows, keys, mutations, do=None, info=None):
        self.q, self.k, self.v, self.vis, self.hmap, self.scale = q, k, v, vis, hmap, scale
        self.rows, self.keys, self.do, self.info = sorted(set(rows)), sorted(set(keys)), do, info or {}
        self.mutations = {n: (m, h) for n, (m, h) in mutations.items() if not (torch.equal(h, hmap) and torch.equal(m.expand_as(vis), vis.expand_as(m)))}
        self._ref = None
        self._scores = {}   # KV-head map -> fp64 scores of the probed rows and the value rows they weigh (the mutation sweep reuses them)
        self._truth_rows = self._fwd = None

    @property
    def D(self):
        return self.q.shape[-1]

    def ref(self, grad=False, o_bwd=None):
        """fp64 reference of the true masks: o, or (o, dq, dk, dv) with delta taken from o_bwd (attend(); default: the reference output rounded
        to bf16, what a correct forward hands its backward)"""
        if not grad:
            if self._fwd is None:
                self._fwd = attend(self.q, self.k, self.v, self.vis, self.hmap, self.scale)
            return self._fwd
        if o_bwd is not None:
            return attend(self.q, self.k, self.v, self.vis, self.hmap, self.scale, do=self.do, o_bwd=o_bwd)
        if self._ref is None:
            o = attend(self.q, self.k, self.v, self.vis, self.hmap, self.scale)
            self._ref = attend(self.q, self.k, self.v, self.vis, self.hmap, self.scale, do=self.do, o_bwd=o.to(torch.bfloat16))
        return self._ref

    def probed_rows(self):
        return sorted({i for _, _, i in self.rows})

    def ref_rows(self, vis=None, hmap=None):
        """forward reference on the probed query rows only: [B, Hq, len(probed_rows()), D] (cheap: the mutation sweep)"""
        vis, hmap = self.vis if vis is None else vis, self.hmap if hmap is None else hmap
        rows = self.probed_rows()
        key = tuple(hmap.tolist())
        if key not in self._scores:
            self._scores[key] = ((self.q.double()[:, :, rows] @ _ext(self.k.double(), hmap).transpose(-1, -2)) * self.scale, _ext(self.v.double(), hmap))
        s, vx = self._scores[key]
        B, Hq, Sq, _ = self.q.shape
        return _masked_softmax_v(s, vis.expand(B, Hq, Sq, s.shape[-1])[:, :, rows], vx)[0]

    def separation(self, name):
        """max over the probed rows of ||mutated - true|| / bar(true) (forward)"""
        m, h = self.mutations[name]
        ri = {i: n for n, i in enumerate(self.probed_rows())}
        slots = [(b, hh, ri[i]) for b, hh, i in self.rows]
        if self._truth_rows is None:
            self._truth_rows = self.ref_rows()
        return slice_errors(self.ref_rows(m, h), self._truth_rows, slots, self.D)[0][0]

    def grad_separation(self, name):
        """the same on the gradients: dQ on the probed rows, dK / dV on the planted keys (full fp64 backward; small cases)"""
        m, h = self.mutations[name]
        t = self.ref(grad=True)
        mo = attend(self.q, self.k, self.v, m, h, self.scale)
        mu = attend(self.q, self.k, self.v, m, h, self.scale, do=self.do, o_bwd=mo.to(torch.bfloat16))
        return max(slice_errors(mu[1], t[1], self.rows, self.D)[0][0], *(slice_errors(mu[x], t[x], self.keys, self.D)[0][0] for x in (2, 3)))


def slice_errors(got, ref, slots, D, rel=BAR_REL):
    """-> [(ratio err / bar, slot, err, bar)] sorted worst first; got / ref [B, H, S, D] (any float dtype), slots (b, h, s)"""
    b, h, s = torch.tensor(slots, device=got.device).T
    g, r = got[b, h, s].double(), ref[b, h, s].to(got.device).double()
    err, rn = (g - r).norm(dim=-1).tolist(), r.norm(dim=-1).tolist()
    out = [(e / bar(n, D, rel), slot, e, bar(n, D, rel)) for e, n, slot in zip(err, rn, slots)]
    return sorted(out, key=lambda t: -t[0])


def check(name, got, ref, slots, D, rel=BAR_REL):
    """assert every probed slice is within the bar"""
    errs = slice_errors(got, ref, slots, D, rel)
    assert torch.isfinite(got.float()).all(), f"{name}: non-finite values"
    bad = [e for e in errs if not e[0] <= 1.0]
    assert not bad, (f"{name}: {len(bad)}/{len(errs)} probed slices out of the bar (rel {rel:.4g}); worst (b, h, s) = {bad[0][1]}: "
                     f"||err|| {bad[0][2]:.4g} > bar {bad[0][3]:.4g}; next {[(e[1], round(e[0], 2)) for e in bad[1:6]]}")
    return errs[0][0] if errs else 0.0


# ------------------------------------------------------------------------------------------------ planting
class _Planter:
    def __init__(self, B, Hq, Hkv, Sq, Sk, D, L, gen, device):
        self.B, self.Hq, self.Hkv, self.G, self.Sq, self.Sk, self.D = B, Hq, Hkv, Hq // Hkv, Sq, Sk, D
        self.scale = D ** -0.5
        self.a = math.sqrt(L / self.scale)
        self.gen = gen
        self.q = torch.randn(B, Hq, Sq, D, generator=gen) * 0.3
        self.k = torch.randn(B, Hkv, Sk, D, generator=gen) * 0.3
        self.v = torch.randn(B, Hkv, Sk, D, generator=gen)
        self.basis = [torch.linalg.qr(torch.randn(D, D, generator=gen, dtype=torch.float64))[0].float() for _ in range(Hkv)]
        self.next_dir = {}          # directions used per (sample, KV head): plants of different samples or KV heads never meet in one row
        self.key_dir = {}       # (b, hk, j) -> direction index
        self.used_rows = set()  # (b, h, i)
        self.rows, self.keys = [], []
        self.device = device

    def key(self, b, hk, j):
        """plant key j of sample b (j == Sk: the first key of sample b + 1) in KV head hk; -> its direction (an index into the KV head's basis)"""
        bb, jj = ((b + 1) % self.B, 0) if j == self.Sk else (b, j)
        if (bb, hk, jj) not in self.key_dir:
            # more plants than dimensions: keys share a direction, a row aligned with it sees both.  The first key of sample b + 1 is aligned with rows of
            # both samples: its direction is new to both
            n = max(self.next_dir.get((b, hk), 0), self.next_dir.get((bb, hk), 0))
            self.next_dir[(b, hk)] = self.next_dir[(bb, hk)] = n + 1
            n %= self.D
            self.key_dir[(bb, hk, jj)] = n
            self.k[bb, hk, jj] = self.a * self.basis[hk][:, n]
            self.v[bb, hk, jj] = 4.0 * (torch.randint(0, 2, (self.D,), generator=self.gen).float() * 2 - 1)
            self.keys.append((bb, hk, jj))
        return self.key_dir[(bb, hk, jj)]

    def row(self, b, h, i, n, exclusive=True):
        """align query row i of head h (sample b) with direction n of its KV head (exclusive: the row carries no other plant)"""
        if exclusive:
            assert (b, h, i) not in self.used_rows
        self.used_rows.add((b, h, i))
        self.q[b, h, i] += self.a * self.basis[h // self.G][:, n]
        self.rows.append((b, h, i))

    def free(self, b, i):
        return 0 <= i < self.Sq and all((b, h, i) not in self.used_rows for h in range(self.Hq))

    def tensors(self):
        bf = torch.bfloat16
        return self.q.to(bf).to(self.device), self.k.to(bf).to(self.device), self.v.to(bf).to(self.device)


def _key_cols(Sk, device):
    return torch.arange(Sk + 1, device=device)


def _row_range_vis(Sq, Sk, lo, hi, causal, device, shift=0):
    """[B, 1, Sq, Sk + 1]: keys [lo[b], hi[b]) (and j <= i + shift if causal)"""
    cols, rows = _key_cols(Sk, device), torch.arange(Sq, device=device)
    lo_t, hi_t = torch.tensor(lo, device=device), torch.tensor(hi, device=device)
    m = (cols[None, None, :] >= lo_t[:, None, None]) & (cols[None, None, :] < hi_t[:, None, None])
    m = m.expand(len(lo), Sq, Sk + 1)
    if causal:
        m = m & (cols[None, None, :] <= rows[None, :, None] + shift)
    return m[:, None].contiguous()


def _wrong_head(Hq, Hkv, device):
    G = Hq // Hkv
    return torch.tensor([(h // G + 1) % Hkv for h in range(Hq)], device=device)


# ------------------------------------------------------------------------------------------------ A: training attention (ops.attn_fwd / attn_bwd)
def training_case(B, S, Hq, Hkv, D, causal, kv_len=None, kv_lo=None, seed=0, device="cpu"):
    """self-attention on a fused q|k|v projection.  Sample b sees keys [kv_lo[b], kv_len[b]) (and j <= i if causal); rows < kv_lo[b] are zero rows.
    -> (Case, qkv [B*S, (Hq+2Hkv)*D] bf16, do [B*S, Hq*D] bf16)"""
    lo = list(kv_lo) if kv_lo is not None else [0] * B
    hi = list(kv_len) if kv_len is not None else [S] * B
    gen = torch.Generator().manual_seed(seed)
    P = _Planter(B, Hq, Hkv, S, S, D, math.log(S) + LOGIT_MARGIN, gen, "cpu")
    truth = _row_range_vis(S, S, lo, hi, causal, "cpu")

    def sees(b, i, j):
        return bool(truth[b, 0, i, j])

    def plant(b, j, want):
        """key j of sample b with rows [(row, kind)]: the first free candidate row of every group that has the wanted visibility"""
        if j < 0 or j > S or (j == S and B == 1):
            return
        picked = []
        for cands, kind in want:
            for i in cands:
                if P.free(b, i) and sees(b, i, j) == (kind == "probe") and (kind == "probe" or truth[b, 0, i].any()):
                    picked.append(i)
                    break
        if not picked:
            return
        for hk in range(Hkv):
            n = P.key(b, hk, j)
            for i in picked:
                for h in range(hk * P.G, (hk + 1) * P.G):
                    P.row(b, h, i, n)

    late = lambda start: list(range(start, -1, -1))
    for b in range(B):
        l, h_ = lo[b], hi[b]
        plant(b, l - 1, [(list(range(l + 2, S)), "decoy"), (late(S - 4), "decoy")])
        plant(b, l, [(list(range(l + 3, S)), "probe"), (late(S - 5), "probe")])
        plant(b, h_ - 1, [(list(range(max(h_ - 1, 0), S)) if causal else late(S - 6), "probe")])
        if h_ < S:
            plant(b, h_, [(late(S - 1) if causal else late(S - 7), "decoy")])
        if causal:   # the diagonal on the last query tile: key i seen by row i, key i + 1 not seen by row i
            plant(b, S - 2, [([S - 2], "probe")])
            plant(b, S - 3, [([S - 4], "decoy")])
        for j in TILE_KEYS:
            if j < S:
                plant(b, j, [(list(range(j + 1, S)) if causal else late(S - 9), "probe")] + ([([j - 1], "decoy")] if causal else []))
    for b in range(B - 1 if B > 1 else 0):   # the first key of sample b + 1 against the last query rows of sample b
        plant(b, S, [(late(S - 1), "decoy")])
    q, k, v = P.tensors()
    qkv = torch.cat([q.transpose(1, 2).reshape(B * S, Hq * D), k.transpose(1, 2).reshape(B * S, Hkv * D), v.transpose(1, 2).reshape(B * S, Hkv * D)], 1)
    do = (torch.randn(B * S, Hq * D, generator=gen)).to(torch.bfloat16)
    qkv, do = qkv.to(device).contiguous(), do.to(device)
    q, k, v, do_c = canon_qkv(qkv, B, S, Hq, Hkv, D) + (do.reshape(B, S, Hq, D).transpose(1, 2),)
    hmap = torch.arange(Hq, device=device) // (Hq // Hkv)
    vis = truth.to(device)
    muts = {}
    mk = lambda lo_, hi_, shift=0: _row_range_vis(S, S, lo_, hi_, causal, device, shift)
    muts["lo-1"] = (mk([max(x - 1, 0) for x in lo], hi), hmap)
    muts["lo+1"] = (mk([x + 1 for x in lo], hi), hmap)
    muts["hi-1"] = (mk(lo, [x - 1 for x in hi]), hmap)
    muts["hi+1"] = (mk(lo, [x + 1 for x in hi]), hmap)
    if causal:
        muts["diag-1"] = (mk(lo, hi, -1), hmap)
        muts["diag+1"] = (mk(lo, hi, +1), hmap)
    for j in TILE_KEYS:
        if j < S:
            m = vis.clone()
            m[..., j] = False
            muts[f"drop key {j}"] = (m, hmap)
    if Hkv > 1:
        muts["kv head"] = (vis, _wrong_head(Hq, Hkv, device))
    if B > 1:
        m = vis.clone()
        m[:B - 1, ..., S] = m[:B - 1].any(-1)   # every row of sample b that sees anything also sees the first key of sample b + 1
        muts["neighbour"] = (m, hmap)
    info = dict(lo=lo, hi=hi, causal=causal)
    return Case(q, k, v, vis, hmap, D ** -0.5, P.rows, P.keys, muts, do=do_c, info=info), qkv, do


def canon_qkv(qkv, B, S, Hq, Hkv, D):
    """fused [B*S, (Hq+2Hkv)*D] -> canonical q [B, Hq, S, D], k / v [B, Hkv, S, D] views"""
    q = qkv[:, : Hq * D].reshape(B, S, Hq, D).transpose(1, 2)
    k = qkv[:, Hq * D: (Hq + Hkv) * D].reshape(B, S, Hkv, D).transpose(1, 2)
    v = qkv[:, (Hq + Hkv) * D: (Hq + 2 * Hkv) * D].reshape(B, S, Hkv, D).transpose(1, 2)
    return q, k, v


def rope_backward(dx, cos, sin, pos):
    """transposed rotary rotation (the gradient of x' = x cos + rotate_half(x) sin) in fp64: dx [B, H, S, D], cos / sin [positions, D], pos [B, S] long"""
    c, s = cos.double()[pos][:, None], sin.double()[pos][:, None]
    D = dx.shape[-1]
    y = dx.double() * s
    return dx.double() * c + torch.cat([y[..., D // 2:], -y[..., : D // 2]], -1)


# ------------------------------------------------------------------------------------------------ B: interval / cross attention (ops.xattn_* / attn_interval_*)
def interval_case(B, Sq, Sk, Hq, Hkv, D, seed=0, device="cpu", n_empty=3):
    """query row i of sample b sees keys [krange[b,i,0], krange[b,i,1]).  Probed rows get their own intervals, chosen so that their four boundary keys
    (begin - 1, begin, end - 1, end; end == Sk: the first key of sample b + 1) are planted; n_empty rows per sample have empty intervals (zero rows).
    -> (Case, q [B, Hq, Sq, D], k, v [B, Hkv, Sk, D] bf16 canonical, krange [B, Sq, 2] int32, do [B, Hq, Sq, D] bf16)"""
    gen = torch.Generator().manual_seed(seed)
    P = _Planter(B, Hq, Hkv, Sq, Sk, D, math.log(Sk) + LOGIT_MARGIN, gen, device)
    kr = torch.zeros(B, Sq, 2, dtype=torch.int32)
    for b in range(B):   # background intervals: random, non-empty
        s0 = torch.randint(0, Sk, (Sq,), generator=gen)
        s1 = torch.randint(0, Sk, (Sq,), generator=gen)
        kr[b, :, 0], kr[b, :, 1] = torch.minimum(s0, s1), torch.maximum(s0, s1) + 1
    for b in range(B):
        rows = iter(torch.randperm(Sq, generator=gen).tolist())
        x = torch.randperm(Sk - 4, generator=gen)[:5].add(2).tolist()     # five distinct interior keys
        # (begin, end, planted key, kind) per probed row: the row sees [begin, end)
        specs = [(0, Sk, 0, "probe"),                                      # the whole range: its first key
                 (1 + x[0] % (Sk - 2), Sk, Sk - 1, "probe"),               # a range that ends at the last key
                 (x[1] + 1, min(x[1] + 2 + x[1] % 89, Sk), x[1], "decoy"),  # begin - 1
                 (x[2], min(x[2] + 1 + x[2] % 97, Sk), x[2], "probe"),     # begin
                 (max(x[3] - x[3] % 83, 0), x[3] + 1, x[3], "probe"),      # end - 1
                 (x[4] // 2, x[4], x[4], "decoy")]                         # end
        if B > 1:
            specs.append((x[0], Sk, Sk, "decoy"))                          # one past the end: the first key of sample b + 1
        for s0, s1, j, kind in specs:
            assert s0 < s1 and (s0 <= j < s1) == (kind == "probe")
            i = next(rows)
            kr[b, i, 0], kr[b, i, 1] = s0, s1
            for hk in range(Hkv):
                n = P.key(b, hk, j)
                for h in range(hk * P.G, (hk + 1) * P.G):
                    P.row(b, h, i, n)
        for _ in range(n_empty):
            i = next(rows)
            e = int(torch.randint(0, Sk + 1, (1,), generator=gen))
            kr[b, i, 0], kr[b, i, 1] = e, e
            P.rows += [(b, h, i) for h in range(Hq)]   # an empty interval: a zero row in every head
    q, k, v = P.tensors()
    do = torch.randn(B, Hq, Sq, D, generator=gen).to(torch.bfloat16).to(device)
    kr = kr.to(device)
    hmap = torch.arange(Hq, device=device) // (Hq // Hkv)
    cols = _key_cols(Sk, device)

    def mk(db=0, de=0):
        return ((cols[None, None, :] >= (kr[..., 0:1].long() + db)) & (cols[None, None, :] < (kr[..., 1:2].long() + de)))[:, None]

    vis = mk()
    muts = {"begin-1": (mk(db=-1), hmap), "begin+1": (mk(db=1), hmap), "end-1": (mk(de=-1), hmap), "end+1": (mk(de=1), hmap)}
    if Hkv > 1:
        muts["kv head"] = (vis, _wrong_head(Hq, Hkv, device))
    if B > 1:
        m = vis.clone()
        m[:B - 1, ..., Sk] = m[:B - 1].any(-1)
        muts["neighbour"] = (m, hmap)
    empty = (kr[..., 0] >= kr[..., 1])
    return Case(q, k, v, vis, hmap, D ** -0.5, P.rows, P.keys, muts, do=do, info=dict(empty=empty)), q, k, v, kr, do


# ------------------------------------------------------------------------------------------------ C: decode attention over a KV cache
def decode_chunks(lo, hi, ns, cap):
    """the key chunks the split-KV decode kernels derive (csrc/attention_decode.hip): a0 = lo & ~7, chunk = min(round8(ceil((hi - a0) / ns)), cap);
    chunk s = keys [max(a0 + s * chunk, lo), min(a0 + (s + 1) * chunk, hi)).  -> (a0, chunk, [chunk starts > a0 that lie below hi])"""
    a0 = lo & ~7
    total = max(hi - a0, 0)
    chunk = min(((-(-total // ns)) + 7) & ~7, cap)
    return a0, chunk, [a0 + s * chunk for s in range(1, ns) if a0 + s * chunk < hi]


def decode_case(B, Smax, Hq, Hkv, D, ranges, ns, cap=4096, seed=0, device="cpu"):
    """one query row per (sample, head) over a cache [B, Hkv, Smax, D]; sample b sees [lo, hi) = ranges[b].  Planted: lo - 1 and the keys [a0, lo)
    (decoys: the kernels start their chunks at a0 = lo & ~7), lo, every chunk edge the kernels derive for `ns` (the first and the last key of every
    chunk), hi - 1 (the newest key), hi (the next cache slot; hi == Smax: the first slot of sample b + 1) - spread over the sample's query heads.
    -> (Case, q [B, Hq, 1, D], k, v [B, Hkv, Smax, D] bf16 canonical)"""
    gen = torch.Generator().manual_seed(seed)
    nmax = max(h - l for l, h in ranges)
    P = _Planter(B, Hq, Hkv, 1, Smax, D, math.log(max(nmax, 2)) + LOGIT_MARGIN, gen, device)
    # no background in the queries: a query carries several plants, and a background term would spread their logits (+-0.35 at head_dim 64) so that
    # the weakest one moves the row by half of what the others do
    P.q.zero_()
    lo = [l for l, _ in ranges]
    hi = [h for _, h in ranges]
    truth = _row_range_vis(1, Smax, lo, hi, False, "cpu")
    edges = {}
    for b, (l, h_) in enumerate(ranges):
        a0, chunk, starts = decode_chunks(l, h_, ns, cap)
        targets = [l, h_ - 1, l - 1, a0, h_] + [c for s in starts for c in (s, s - 1)]
        edges[b] = starts
        seen = []
        for j in targets:
            if 0 <= j <= Smax and j not in seen and not (j == Smax and B == 1):
                seen.append(j)
        for t, j in enumerate(seen):
            h = t % Hq
            hk = h // P.G
            n = P.key(b, hk, j)
            P.row(b, h, 0, n, exclusive=False)
    for b in range(B):   # every head is a probed slot (heads without a plant check the background)
        for h in range(Hq):
            P.rows.append((b, h, 0))
    q, k, v = P.tensors()
    hmap = torch.arange(Hq, device=device) // (Hq // Hkv)
    mk = lambda lo_, hi_: _row_range_vis(1, Smax, lo_, hi_, False, device)
    vis = truth.to(device)
    muts = {"lo-1": (mk([max(x - 1, 0) for x in lo], hi), hmap), "lo+1": (mk([x + 1 for x in lo], hi), hmap),
            "hi-1": (mk(lo, [x - 1 for x in hi]), hmap), "hi+1": (mk(lo, [x + 1 for x in hi]), hmap),
            "from a0": (mk([x & ~7 for x in lo], hi), hmap)}
    for b in range(B):
        for s in edges[b]:
            for j, what in ((s, "first"), (s - 1, "last")):
                m = vis.clone()
                m[b, ..., j] = False
                muts[f"b{b} chunk edge {s}: {what} key dropped"] = (m, hmap)
    if Hkv > 1:
        muts["kv head"] = (vis, _wrong_head(Hq, Hkv, device))
    if B > 1:
        m = vis.clone()
        m[:B - 1, ..., Smax] = True
        muts["neighbour"] = (m, hmap)
    trunc = [min(h_, (l & ~7) + ns * cap) for l, h_ in ranges]
    if trunc != hi:   # keys behind ns * cap per sample not read (the per-head kernel before the spad <= nsplit * 4096 guard)
        muts["truncated"] = (mk(lo, trunc), hmap)
    return Case(q, k, v, vis, hmap, D ** -0.5, P.rows, P.keys, muts, info=dict(ranges=ranges, ns=ns, cap=cap)), q, k, v


# ------------------------------------------------------------------------------------------------ the layouts of tests/test_attn_edges_gpu.py
TRAIN_S = (63, 64, 65, 127, 128, 129, 1000, 1024, 1089)


def train_layouts(S):
    """(name, B, Hq, Hkv, causal, kv_len, kv_lo) of family A at sequence length S: GQA groups 1 / 2 / 7, right padding that ends inside a tile, left padding
    with kv_lo % 8 != 0; two samples each (the neighbour key)"""
    hi0 = max(2, S - 1 - S // 3)
    lo0 = min(S // 4 + 5, hi0 - 1)
    return [("encoder", 2, 2, 2, False, None, None),
            ("encoder right-padded", 2, 4, 2, False, [hi0, S], None),
            ("decoder", 2, 14, 2, True, None, None),
            ("decoder left/right-padded", 2, 4, 2, True, [hi0, S], [lo0, 0])]


# (B, Sq, Sk, Hq, Hkv, D, self_attention, row pitch slack): family B
INTERVAL_LAYOUTS = [(2, 100, 300, 4, 2, 64, False, 0), (2, 257, 64, 4, 4, 128, False, 64), (2, 64, 1000, 14, 2, 128, False, 8),
                    (2, 200, 200, 8, 2, 128, True, 0), (3, 129, 129, 2, 1, 64, True, 0)]

# family C: head groups (Hq, Hkv) per G, the ranges of the three samples of a cache of DECODE_SMAX positions (ragged, lo % 8 != 0, one ending at the last
# slot, one nearly empty), and the split counts
DECODE_HEADS = {1: (16, 16), 2: (16, 8), 4: (16, 4), 7: (28, 4), 8: (16, 2)}   # 16+ query heads: at most ~8 plants per decode query
DECODE_SMAX = 1000
DECODE_RANGES = [(0, 1000), (37, 801), (5, 9)]


def decode_splits(D, fused):
    """ns of family C: 1, 2, 3, 8, 13 and the largest the form allows (the one-launch merge: nsplit * (D + 2) <= 4096; two launches: 64)"""
    return (1, 2, 3, 8, 13, 4096 // (D + 2) if fused else 64)


LONG_SMAX, LONG_RANGES = 8000, [(3, 8000), (901, 7777)]   # the long-range decode case: ns = 2 covers it, ns = 1 must be refused

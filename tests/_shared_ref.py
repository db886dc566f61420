"""The fp64 restatement of afk_attn_decode_shared's contract and its planted-key cases (pure torch, CPU; imported like tests/_attn_probe.py).

Contract (include/afk.h): continuation r = b0 * n + c attends to the union of the prompt keys [prange[b0]) of prompt row b0 and the tail keys [trange[r]) of
its own tail row.  reference(): per continuation, the visible prompt keys of r // n concatenated with its visible tail keys, then _attn_probe.attend.

A case is built the _attn_probe way (its module docstring): queries carry no background, only plants; every planted key takes an equal share of its row.
Planted, spread over the continuation's query heads:
  prompt  the interval's first and last key, the 32-key tile edges next to its ends, the first and last key of every split chunk the kernel derives
          (ops.attn_append_chunks - the same chunking), and the two DECOYS lo - 1 and hi: aligned with a query, so they would dominate if they were seen
  tail    the interval's first and last key, the tile edge 31 | 32, and the decoys t0 - 1 and t1
Every other slot outside an interval, and every pad column of the transposed value caches, is NaN: one read of it shows in the output."""
import math

import torch

import _attn_probe as P

BF = torch.bfloat16
MAX_PLANTS = 40   # per (cache row, KV head): directions of one orthonormal basis (D >= 64)


def pad64(n):
    return (int(n) + 63) // 64 * 64


def chunks(lo, hi, ns):
    """the key chunks afk_attn_decode_shared cuts a prompt interval into (ops.attn_append_chunks restated: a0 = lo & ~31, chunk = round32(ceil((hi - a0) / ns)))"""
    if hi <= lo:
        return []
    a0 = lo & ~31
    chunk = ((-(-(hi - a0) // ns)) + 31) & ~31
    out = []
    for s in range(ns):
        c0, c1 = a0 + s * chunk, min(a0 + (s + 1) * chunk, hi)
        if c1 > max(c0, lo):
            out.append((max(c0, lo), c1))
    return out


def intervals(B0, n, Sp, T):
    """the intervals of a case: prompt rows with DIFFERENT first keys (not multiples of 8) that end one slot in front of the cache's last (the decoy hi);
    tails that end at different slots per copy, odd copies starting at slot 1 where the tail is long enough"""
    pr = []
    for b0 in range(B0):
        if Sp == 0:
            pr.append((0, 0))
        elif Sp < 16:
            pr.append((1, Sp - 1))
        else:
            pr.append(((3, 37)[b0 % 2] if Sp >= 64 else (3, 5)[b0 % 2], Sp - 1))
    tr = []
    for r in range(B0 * n):
        c = r % n
        if T == 0:
            tr.append((0, 0))
        elif T == 1:
            tr.append((0, 1))
        else:
            t1 = max(1, T - 1 - (c % 3))
            tr.append((1 if (c % 2 == 1 and t1 >= 4) else 0, t1))
    return pr, tr


class SharedCase:
    """inputs as the kernel takes them (bf16, CPU): qkv [R, (Hq + 2 Hkv) * D] with q its leading columns (a strided view), Kp [B0, Sp, Hkv * D],
    Vtp [B0, Hkv, D, pad64(Sp)], Kt [R, T, Hkv * D], Vtt [R, Hkv, D, pad64(T)], prange [B0, 2], trange [R, 2] int32"""

    def __init__(self, **kw):
        self.__dict__.update(kw)
        self._ref = {}

    @property
    def q(self):
        return self.qkv[:, : self.Hq * self.D]

    def slots(self):
        return [(r, h, 0) for r in range(self.B0 * self.n) for h in range(self.Hq)]

    def reference(self, dp=0, dt=0):
        """fp64 [R, Hq, 1, D]; dp / dt: the prompt / tail interval END moved by that many keys (the negative controls)"""
        if (dp, dt) not in self._ref:
            pr = self.prange.clone()
            tr = self.trange.clone()
            pr[:, 1] += dp
            tr[:, 1] += dt
            self._ref[(dp, dt)] = reference(self.q, self.Kp, self.Vtp, self.Kt, self.Vtt, pr, tr, self.n, self.Hq, self.Hkv, self.D, self.D ** -0.5)
        return self._ref[(dp, dt)]

    def to(self, device):
        return {k: getattr(self, k).to(device) for k in ("qkv", "Kp", "Vtp", "Kt", "Vtt", "prange", "trange")}


def reference(q, Kp, Vtp, Kt, Vtt, prange, trange, n, Hq, Hkv, D, scale):
    """the contract in fp64: q [R, Hq * D] (any row stride) -> o [R, Hq, 1, D].  A continuation that sees no key is a zero row."""
    R = q.shape[0]
    hmap = torch.arange(Hq) // (Hq // Hkv)
    out = torch.zeros(R, Hq, 1, D, dtype=torch.float64)
    for r in range(R):
        b0 = r // n
        (lo, hi), (t0, t1) = (max(int(a), 0) for a in prange[b0]), (max(int(a), 0) for a in trange[r])
        hi, t1 = min(hi, Kp.shape[1]), min(t1, Kt.shape[1])
        ks, vs = [], []
        if hi > lo:
            ks.append(Kp[b0, lo:hi].reshape(hi - lo, Hkv, D).transpose(0, 1))
            vs.append(Vtp[b0, :, :, lo:hi].transpose(-1, -2))
        if t1 > t0:
            ks.append(Kt[r, t0:t1].reshape(t1 - t0, Hkv, D).transpose(0, 1))
            vs.append(Vtt[r, :, :, t0:t1].transpose(-1, -2))
        if not ks:
            continue
        k, v = torch.cat(ks, 1)[None], torch.cat(vs, 1)[None]   # [1, Hkv, keys, D]
        vis = torch.ones(1, 1, 1, k.shape[2] + 1, dtype=torch.bool)
        vis[..., -1] = False   # attend()'s extra column: the neighbouring sample's first key - there is none here
        out[r] = P.attend(q[r].reshape(1, Hq, 1, D), k, v, vis, hmap, scale)[0]
    return out


def shared_case(B0, n, Hq, Hkv, D, Sp, T, nsplit, seed=0):
    """-> SharedCase; the cache rows hold Sp / T positions, the intervals are intervals(B0, n, Sp, T)"""
    gen = torch.Generator().manual_seed(seed)
    G, R, scale = Hq // Hkv, B0 * n, D ** -0.5
    pr, tr = intervals(B0, n, Sp, T)
    nmax = max([h - l for l, h in pr]) + max([h - l for l, h in tr])
    a = math.sqrt((math.log(max(nmax, 2)) + P.LOGIT_MARGIN) / scale)
    basis = [torch.linalg.qr(torch.randn(D, D, generator=gen, dtype=torch.float64))[0].float() for _ in range(Hkv)]
    nan = float("nan")
    Kp = torch.full((B0, Sp, Hkv, D), nan)
    Vp = torch.full((B0, Sp, Hkv, D), nan)
    Kt = torch.full((R, T, Hkv, D), nan)
    Vt_ = torch.full((R, T, Hkv, D), nan)
    q = torch.zeros(R, Hq, D)
    for b0, (lo, hi) in enumerate(pr):   # background inside the intervals
        Kp[b0, lo:hi] = torch.randn(hi - lo, Hkv, D, generator=gen) * 0.3
        Vp[b0, lo:hi] = torch.randn(hi - lo, Hkv, D, generator=gen)
    for r, (t0, t1) in enumerate(tr):
        Kt[r, t0:t1] = torch.randn(t1 - t0, Hkv, D, generator=gen) * 0.3
        Vt_[r, t0:t1] = torch.randn(t1 - t0, Hkv, D, generator=gen)
    planted = dict(prompt=[], tail=[])

    def plant(K, V, row, j, hk, ndir):
        if torch.isnan(K[row, j]).all():   # a decoy slot: background in the KV heads that carry no plant, so that a mutated reference is finite
            K[row, j] = torch.randn(Hkv, D, generator=gen) * 0.3
            V[row, j] = torch.randn(Hkv, D, generator=gen)
        K[row, j, hk] = a * basis[hk][:, ndir]
        V[row, j, hk] = 4.0 * (torch.randint(0, 2, (D,), generator=gen).float() * 2 - 1)

    for b0, (lo, hi) in enumerate(pr):
        targets = []
        if hi > lo:
            a0 = lo & ~31
            edges = [e for s in (a0 + 32, ((hi - 1) & ~31)) for e in (s - 1, s)]
            targets = [lo, hi - 1, lo - 1, hi] + edges
            for c0, c1 in chunks(lo, hi, nsplit):
                targets += [c0, c1 - 1]
        seen = []
        for j in targets:
            if 0 <= j < Sp and j not in seen and len(seen) < MAX_PLANTS - 8:
                seen.append(j)
        ndirs = {}   # KV head -> directions used by this prompt row (its copies' tails go on from there)
        for t_, j in enumerate(seen):
            h = t_ % Hq
            hk = h // G
            nd = ndirs[hk] = ndirs.get(hk, -1) + 1
            plant(Kp, Vp, b0, j, hk, nd)
            planted["prompt"].append((b0, hk, j, lo <= j < hi))
            for c in range(n):   # every copy of the row is aligned with the shared key
                q[b0 * n + c, h] += a * basis[hk][:, nd]
        for c in range(n):
            r = b0 * n + c
            t0, t1 = tr[r]
            seen = []
            for j in ([t0, t1 - 1, t0 - 1, t1, 31, 32] if t1 > t0 else []):
                if 0 <= j < T and j not in seen:
                    seen.append(j)
            used = dict(ndirs)
            for t_, j in enumerate(seen):
                h = (t_ + 1 + c) % Hq   # a different head per copy: the copies' rows differ
                hk = h // G
                nd = used[hk] = used.get(hk, -1) + 1
                assert nd < D
                plant(Kt, Vt_, r, j, hk, nd)
                planted["tail"].append((r, hk, j, t0 <= j < t1))
                q[r, h] += a * basis[hk][:, nd]
    k_new = torch.randn(R, 2 * Hkv * D, generator=gen)   # the k | v columns of the fused projection the query rows live in
    qkv = torch.cat([q.reshape(R, Hq * D), k_new], 1).to(BF)
    Vtp = torch.full((B0, Hkv, D, pad64(Sp)), nan)
    Vtp[..., :Sp] = Vp.permute(0, 2, 3, 1)
    Vtt = torch.full((R, Hkv, D, pad64(T)), nan)
    Vtt[..., :T] = Vt_.permute(0, 2, 3, 1)
    return SharedCase(B0=B0, n=n, Hq=Hq, Hkv=Hkv, D=D, Sp=Sp, T=T, nsplit=nsplit, qkv=qkv, Kp=Kp.reshape(B0, Sp, Hkv * D).to(BF), Vtp=Vtp.to(BF),
                      Kt=Kt.reshape(R, T, Hkv * D).to(BF), Vtt=Vtt.to(BF), prange=torch.tensor(pr, dtype=torch.int32).reshape(B0, 2),
                      trange=torch.tensor(tr, dtype=torch.int32).reshape(R, 2), planted=planted)


# (B0, n, Hq, Hkv, D, Sp, T, nsplit): each the smallest shape that reaches one edge
CASES = [(1, 2, 4, 4, 64, 64, 1, 1),         # G = 1, one split, a one-key tail
         (2, 3, 4, 2, 128, 100, 5, 3),       # two prompt rows with different lo, a partly filled column tile
         (2, 5, 28, 4, 64, 97, 33, 8),       # G = 7 with 5 copies: a full tile of 4 plus a tile of 1; a tail across a 32-key tile edge; empty prompt splits
         (2, 4, 16, 2, 128, 1000, 64, 8),    # G = 8, copies filling the tile exactly
         (1, 16, 28, 4, 128, 1000, 40, 3),   # 16 beams at the AF3 group
         (1, 2, 16, 4, 64, 7, 0, 8),         # a prompt shorter than one tile, every tail empty
         (1, 3, 4, 2, 64, 0, 9, 1)]          # an empty prompt interval, tail only

"""fp64 CPU restatement of steps 3a-3d of afk_decode_sample_filtered (include/afk.h) on top of _sampler_ref.Row: MinPLogitsWarper / TypicalLogitsWarper /
EpsilonLogitsWarper / EtaLogitsWarper (transformers/generation/logits_process.py) in the order GenerationMixin._get_logits_processor appends them, every
softmax taken over the set the filters in front left.  The yardstick of tests/test_warpers_cpu.py / test_warpers_gpu.py.

A Chain works on the row's classes of equal z (a filter's statistic is a function of z, so a class stays or goes as a whole).  Each filter records its decision
margin, and each has a snap_* that moves its parameter into the middle of a gap of the statistic it compares against, so that rounding cannot pick a case."""
import numpy as np

from tests import _sampler_ref as R


class Chain:
    def __init__(self, row, top_k=0, top_p=1.0):
        self.row, self.margins = row, {}
        self.base = row.result(top_k, top_p)
        self.degenerate = row.first_inf >= 0 or row.empty
        if self.degenerate:
            return
        self.margins["top_p"] = self.base["margin"]
        self.ck = np.zeros(row.vals.size, dtype=bool)
        self.ck[row.inv[self.base["keep"]]] = True
        self.ec = np.exp(row.vals - row.vals[-1])        # a token's exp(z - zmax), per class

    # ---- statistics over the current set S
    def _r(self):
        """per-token probability of every class under softmax_S (0 outside S)"""
        m = np.where(self.ck, self.row.cmass, 0.0)
        return np.where(self.ck, self.ec, 0.0) / m.sum(), m / m.sum()

    def entropy(self):
        r, cm = self._r()
        s = self.ck & (r > 0)
        return float(-(cm[s] * np.log(r[s])).sum())

    def _typical_order(self):
        """classes of S by ascending d = |-log r - H| -> (class ids, d, inclusive cumulative mass)"""
        r, cm = self._r()
        ids = np.nonzero(self.ck)[0]
        with np.errstate(divide="ignore"):
            d = np.abs(-np.log(r[ids]) - self.entropy())
        o = np.argsort(d, kind="stable")
        return ids[o], d[o], np.cumsum(cm[ids][o])

    # ---- snapping: -> (parameter, gap) with the gap the tests assert
    @staticmethod
    def _geo_gap(vals, target):
        """vals ascending, distinct, positive: the geometric midpoint of the two neighbours around target, and the relative half-gap sqrt(hi / lo) - 1"""
        vals = vals[vals > 0]
        if vals.size < 2:
            return float(vals[0]) * 0.5 if vals.size else target, np.inf        # one class: it is the set's maximum and stays whatever the floor
        j = int(np.clip(np.searchsorted(vals, target), 1, vals.size - 1))
        return float(np.sqrt(vals[j - 1] * vals[j])), float(np.sqrt(vals[j] / vals[j - 1]) - 1.0)

    def snap_min_p(self, target):
        return self._geo_gap(self.ec[self.ck], target)

    def snap_epsilon(self, target):
        return self._geo_gap(self._r()[0][self.ck], target)

    def snap_eta(self, target):
        """eta* in a gap of r, then the eps that yields it: eta = min(eps, sqrt(eps) e^-H) -> eps = eta* if eta* <= e^-2H else (eta* e^H)^2 (>= 1: no such eps, gap 0).
        No eps < 1 puts the floor at or above e^-H, so the target is capped at 0.3 e^-H (a flat row of 152 064 tokens has e^-H ~ 1e-5)"""
        H = self.entropy()
        eta, gap = self._geo_gap(self._r()[0][self.ck], min(target, 0.3 * np.exp(-H)))
        eps = eta if eta <= np.exp(-2.0 * H) else (eta * np.exp(H)) ** 2
        return (float(eps), gap) if 0.0 < eps < 1.0 else (0.5, 0.0)

    def snap_typical(self, target):
        """-> (typical_p, (mass half-gap, distance of d* to the neighbouring d classes))"""
        _, d, cum = self._typical_order()
        c = np.concatenate([[0.0], cum])
        j = int(np.clip(np.searchsorted(c, target, side="right"), 1, c.size - 1))
        p = 0.5 * (c[j - 1] + c[j])
        if not 0.0 < p < 1.0:
            return 0.5, (0.0, 0.0)
        lo = d[j - 1] - d[j - 2] if j >= 2 else np.inf
        hi = d[j] - d[j - 1] if j < d.size else np.inf
        return float(p), (float(0.5 * (c[j] - c[j - 1])), float(min(lo, hi)))

    # ---- the filters, in place; each returns self
    def min_p(self, p):
        if self.degenerate or not p > 0.0:
            return self
        s = self.ck
        self.margins["min_p"] = float(np.abs(self.ec[s] / p - 1.0).min())
        self.ck = s & (self.ec >= p)
        return self

    def typical(self, p):
        if self.degenerate or not p < 1.0:
            return self
        ids, d, cum = self._typical_order()
        last = min(int((cum < p).sum()), ids.size - 1)        # the reference's (cumulative_probs < mass).sum(), clamped
        dd = np.abs(d - d[last])
        self.margins["typical_mass"] = float(np.abs(cum - p).min())
        self.margins["typical_d"] = float(dd[dd > 0].min()) if (dd > 0).any() else np.inf
        ck = np.zeros_like(self.ck)
        ck[ids[d <= d[last]]] = True
        self.ck = ck
        return self

    def _floor(self, name, floor):
        r, _ = self._r()
        s = self.ck
        self.margins[name] = float(np.abs(r[s] / floor - 1.0).min())
        top = np.nonzero(s)[0][-1]                           # the class of the largest z in S always stays
        self.ck = s & ((r >= floor) | (np.arange(s.size) == top))
        return self

    def epsilon(self, eps):
        if self.degenerate or not 0.0 < eps < 1.0:
            return self
        return self._floor("epsilon", eps)

    def eta(self, eps):
        if self.degenerate or not 0.0 < eps < 1.0:
            return self
        return self._floor("eta", min(eps, np.sqrt(eps) * np.exp(-self.entropy())))

    def result(self):
        """keep [V] bool, r [V] fp64, cdf [V] in token-id order, margins {filter: distance of its parameter from the nearest value of its statistic}"""
        if self.degenerate:
            return dict(self.base, margins={})
        row = self.row
        keep = self.ck[row.inv] & (row.z > -np.inf)
        r = np.where(keep, row.e, 0.0)
        r = r / r.sum()
        return dict(keep=keep, r=r, cdf=np.cumsum(r), margins=dict(self.margins))


def reference(logits, T=1.0, top_k=0, top_p=1.0, min_p=0.0, typical_p=1.0, epsilon_cutoff=0.0, eta_cutoff=0.0):
    return Chain(R.Row(logits, T), top_k, top_p).min_p(min_p).typical(typical_p).epsilon(epsilon_cutoff).eta(eta_cutoff).result()


# the gaps the tests assert on a snapped parameter
REL_GAP = 1e-4        # min_p, epsilon_cutoff, eta_cutoff: relative half-gap of the statistic (fp32 exp / log of the floor are good to ~1e-6)
MASS_GAP = 5e-5       # typical_p: half-gap of the cumulative mass (test_sampler_gpu.HALF_GAP, same reason)
D_GAP = 5e-5          # typical_p: d* to both neighbouring d classes (d is an fp32 difference of values up to ~40: ~4e-6)


def snap_chain(row, top_k, top_p, targets):
    """targets: {filter: target} for the active filters -> (Chain applied, parameters as keywords, ok): every parameter snapped on the set in front of its
    filter, ok = every gap met"""
    c, kw, ok = Chain(row, top_k, top_p), {}, True
    if c.degenerate:
        return c, kw, ok
    if "min_p" in targets:
        kw["min_p"], g = c.snap_min_p(targets["min_p"])
        ok &= g >= REL_GAP and kw["min_p"] <= 1.0
        c.min_p(kw["min_p"])
    if "typical_p" in targets:
        kw["typical_p"], (gm, gd) = c.snap_typical(targets["typical_p"])
        ok &= gm >= MASS_GAP and gd >= D_GAP
        c.typical(kw["typical_p"])
    if "epsilon_cutoff" in targets:
        kw["epsilon_cutoff"], g = c.snap_epsilon(targets["epsilon_cutoff"])
        ok &= g >= REL_GAP and 0.0 < kw["epsilon_cutoff"] < 1.0
        c.epsilon(kw["epsilon_cutoff"])
    if "eta_cutoff" in targets:
        kw["eta_cutoff"], g = c.snap_eta(targets["eta_cutoff"])
        ok &= g >= REL_GAP
        c.eta(kw["eta_cutoff"])
    return c, kw, bool(ok)

"""fp64 CPU restatement of the sampling contract of afk_decode_sample (include/afk.h, steps 1-6) and an integer Philox4x32-10: the yardstick of
tests/test_sampler_cpu.py / test_sampler_gpu.py.  Steps 1-4 are TemperatureLogitsWarper / TopKLogitsWarper / TopPLogitsWarper
(transformers/generation/logits_process.py) with one deviation: a class of equal values is kept or dropped as a whole by top-p."""
import numpy as np
import torch

_MASK = 0xFFFFFFFF


def philox4x32_10(ctr, key):
    """Philox4x32-10 (Salmon, Moraes, Dror, Shaw: Parallel random numbers: as easy as 1, 2, 3, SC'11): four 32-bit counter words, two key words -> four words"""
    c, k = [int(x) & _MASK for x in ctr], [int(x) & _MASK for x in key]
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c[0], 0xCD9E8D57 * c[2]
        c = [((p1 >> 32) ^ c[1] ^ k[0]) & _MASK, p1 & _MASK, ((p0 >> 32) ^ c[3] ^ k[1]) & _MASK, p0 & _MASK]
        k = [(k[0] + 0x9E3779B9) & _MASK, (k[1] + 0xBB67AE85) & _MASK]
    return c


def uniform(seed, t, b):
    """the kernel's u for token number t of row b: key = (seed low, seed high), counter = (t, b, 0, 0), u = (word0 >> 8) * 2^-24"""
    return (philox4x32_10((t, b, 0, 0), (seed & _MASK, (seed >> 32) & _MASK))[0] >> 8) * 2.0 ** -24


class Row:
    """one row of logits at one temperature: the classes of equal z (ascending) with their sizes and masses; the K- and P-sets are whole classes"""

    def __init__(self, logits, T=1.0):
        x = torch.as_tensor(logits).detach().cpu().float().numpy().astype(np.float32).reshape(-1)
        with np.errstate(all="ignore"):
            z = x if T == 1.0 else (x / np.float32(T)).astype(np.float32)      # step 1: fp32 division
        z = np.where(np.isnan(z), np.float32(-np.inf), z).astype(np.float64)
        self.z, self.V = z, z.size
        self.first_inf = int(np.argmax(z == np.inf)) if bool((z == np.inf).any()) else -1
        self.empty = self.first_inf < 0 and not bool(np.isfinite(z).any())
        if self.first_inf >= 0 or self.empty:
            return
        self.vals, self.inv, self.cnt = np.unique(z, return_inverse=True, return_counts=True)
        with np.errstate(all="ignore"):
            self.e = np.exp(z - z.max())
        self.cmass = np.bincount(self.inv, weights=self.e, minlength=self.vals.size)

    def kset_start(self, top_k):
        """index of the lowest class of the K-set: the class of the min(top_k, V)-th largest value (ties at the threshold all stay)"""
        if not top_k or top_k <= 0 or top_k >= self.V:
            return 0
        above = np.cumsum(self.cnt[::-1])[::-1]        # elements in this class and higher ones
        return int(np.nonzero(above >= top_k)[0][-1])

    def class_cums(self, top_k):
        """[0, c_1, ..., 1]: cumulative softmax mass of the K-set's classes, ascending, each including the class itself"""
        m = self.cmass[self.kset_start(top_k):]
        return np.concatenate([[0.0], np.cumsum(m) / m.sum()])

    def snap_top_p(self, top_k, p_target):
        """-> (top_p, half_gap): 1 - top_p moved to the midpoint between the two adjacent class cumulative masses around 1 - p_target, so that
        a summation error below half_gap cannot change the kept set"""
        c = self.class_cums(top_k)
        j = int(np.searchsorted(c, 1.0 - p_target, side="right"))
        j = min(max(j, 1), c.size - 1)
        return 1.0 - 0.5 * (c[j - 1] + c[j]), 0.5 * (c[j] - c[j - 1])

    def result(self, top_k=0, top_p=1.0):
        """keep [V] bool, r [V] fp64, margin (distance of 1 - top_p from the nearest class cumulative mass; inf without top-p), cdf [V] in token-id order"""
        V = self.V
        if self.first_inf >= 0 or self.empty:
            keep = np.zeros(V, dtype=bool)
            if self.first_inf >= 0:
                keep[self.first_inf] = True
            r = keep.astype(np.float64)
            return dict(keep=keep, r=r, margin=np.inf, cdf=np.cumsum(r))
        s = self.kset_start(top_k)
        ckeep = np.zeros(self.vals.size, dtype=bool)
        ckeep[s:] = True
        margin = np.inf
        if top_p < 1.0:
            c = self.class_cums(top_k)[1:]
            ckeep[s:] = c > 1.0 - top_p
            ckeep[-1] = True                                  # the class of the row maximum always stays
            margin = float(np.abs(c - (1.0 - top_p)).min())
        keep = ckeep[self.inv] & (self.z > -np.inf)
        r = np.where(keep, self.e, 0.0)
        r = r / r.sum()
        return dict(keep=keep, r=r, margin=margin, cdf=np.cumsum(r))


def reference(logits, T=1.0, top_k=0, top_p=1.0):
    return Row(logits, T).result(top_k, top_p)


def draw(res, u):
    """step 5: the smallest kept id whose inclusive cdf exceeds u; the largest kept id if rounding leaves none; 0 for a row with no finite logit"""
    if not res["keep"].any():
        return 0
    hit = np.nonzero(res["keep"] & (res["cdf"] > u))[0]
    return int(hit[0]) if hit.size else int(np.nonzero(res["keep"])[0][-1])


def bf16_logits(V, scale, seed):
    """what the lm_head produces: bf16-valued fp32 (randn * scale rounded to bf16), from a generator of its own"""
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(V, generator=g) * scale).to(torch.bfloat16).float()

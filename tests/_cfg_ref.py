"""fp64 numpy restatement of classifier-free guidance as UnbatchedClassifierFreeGuidanceLogitsProcessor applies it (transformers/generation/logits_process.py:
2224-2339) and of the bookkeeping of its unconditional branch.  tests/test_decode_cfg_cpu.py holds it against the class itself; the GPU tests hold
afk_decode_cfg and generate(guidance_scale=...) against it.

  guided(zc, zu, s)      rows [B, V] -> scale * (log_softmax(zc) - log_softmax(zu)) + log_softmax(zu) in float64, IEEE throughout (-inf - -inf is NaN)
  bar(s, M, V)           the fp32 kernel's bound on the finite entries (derived in tests/test_decode_cfg_gpu.py)
  UncondBranch           what the unconditional branch is fed call by call: (ids, attention mask)
  same_class(got, want)  the non-finite entries agree in class (+inf, -inf, NaN) -> the mask of the entries finite in `want`"""
import numpy as np


def log_softmax64(z):
    """log_softmax over the last axis in float64 as torch evaluates it: (z - max) - log(sum(exp(z - max))); a row with no entry above -inf, or with a +inf, is NaN"""
    z = np.asarray(z, dtype=np.float64)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        d = z - z.max(-1, keepdims=True)
        return d - np.log(np.exp(d).sum(-1, keepdims=True))


def guided(zc, zu, s, nan_as_ninf=True):
    """the guided rows.  nan_as_ninf: a NaN logit counts as -inf before the formula (afk_decode_cfg's convention, that of the sampler and of afk_beam_step; the
    reference has no such rule - the CPU test plants no NaN)"""
    zc, zu = np.asarray(zc, dtype=np.float64).copy(), np.asarray(zu, dtype=np.float64).copy()
    if nan_as_ninf:
        zc[np.isnan(zc)] = -np.inf
        zu[np.isnan(zu)] = -np.inf
    c, u = log_softmax64(zc), log_softmax64(zu)
    with np.errstate(invalid="ignore", over="ignore"):
        return float(s) * (c - u) + u


def finite_absmax(*zs):
    """M: the largest finite |z| over the given arrays (0 where there is none)"""
    m = 0.0
    for z in zs:
        z = np.asarray(z, dtype=np.float64)
        f = np.isfinite(z)
        if f.any():
            m = max(m, float(np.abs(z[f]).max()))
    return m


def bar(s, M, V):
    """8 * (2|s| + 1) * 2^-23 * (2M + ln V): one fp32 rounding each in z - max, - log(sum), c - u, the product and the final add, each at most half an ulp of a
    magnitude <= 2M + ln V (|c|, |u| <= 2M + ln V; the product scales three of them by |s|, c - u doubles the magnitude); the relative error of the sum of
    exponentials enters log as an absolute error below one such ulp; the factor 8 covers the count with room for a 2-ulp expf / logf"""
    return 8.0 * (2.0 * abs(float(s)) + 1.0) * 2.0 ** -23 * (2.0 * float(M) + np.log(float(V)))


def same_class(got, want):
    """asserts that wherever `want` is +inf, -inf or NaN `got` is the same, and that `got` is finite elsewhere -> the mask of the finite entries"""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, (got.shape, want.shape)
    for name, f in (("NaN", np.isnan), ("+inf", np.isposinf), ("-inf", np.isneginf)):
        assert np.array_equal(f(got), f(want)), f"{name} entries differ: {int(f(got).sum())} against {int(f(want).sum())}"
    return np.isfinite(want)


class UncondBranch:
    """get_unconditional_logits' inputs (use_cache=True): the first call runs the negative prompt - None: input_ids[:, -1:] - under its mask (None: ones); every
    later call feeds input_ids[:, -1:] and a mask one column longer than the last one"""

    def __init__(self, negative_ids=None, negative_mask=None):
        self.ids = None if negative_ids is None else np.asarray(negative_ids)
        self.mask = None if negative_mask is None else np.asarray(negative_mask)
        self.first = True

    def step(self, input_ids):
        """input_ids [B, n]: everything selected so far behind the prompt -> (the ids the branch runs, its attention mask)"""
        input_ids = np.asarray(input_ids)
        if self.first:
            self.first = False
            if self.ids is None:
                self.ids = input_ids[:, -1:]
            if self.mask is None:
                self.mask = np.ones_like(self.ids)
            return self.ids, self.mask
        self.ids = input_ids[:, -1:]
        self.mask = np.concatenate([self.mask, np.ones_like(self.ids)], axis=1)
        return self.ids, self.mask

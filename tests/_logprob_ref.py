"""Float64 reference of the per-token log-probability kernels (csrc/token_logprob.hip), on top of tests/_ce_ref.py: its CASES, inputs and reference.

From the bf16 logits x [rows, V], labels (-100 = ignore) and a per-row upstream gradient u = d L / d logp:
    logp    = x[label] - logsumexp(x) = -row_loss                   0 on an ignored row
    lse     = logsumexp(x)                                          0 on an ignored row
    entropy = -sum p log p, p = softmax(x), 0 log 0 = 0             0 on an ignored row
    dlogits = u_row * (onehot(label) - softmax(x))                  0 on an ignored row, whatever u holds there
and the [B, S] alignment rule of forward(labels=, return_token_logprobs=True).
"""
import functools

import torch

from tests import _ce_ref as R

CASES, CASE_BY_NAME, SHAPES, IGNORE, inputs = R.CASES, R.CASE_BY_NAME, R.SHAPES, R.IGNORE, R.inputs
EPS32 = 2.0 ** -24


def reference(x, labels):
    """-> float64 (logp [rows], lse [rows], entropy [rows], g [rows, V]) with g = onehot - softmax (the gradient for u = 1), zeros on ignored rows"""
    row_loss, g, _ = R.reference(x, labels, 1.0, 1.0)     # g = softmax - onehot, 0 on ignored rows
    x = x.double()
    valid = labels >= 0
    m = x.max(1, keepdim=True).values
    d = x - m                                             # <= 0, -inf on a masked column
    e = torch.exp(d)
    s = e.sum(1)
    t = torch.where(torch.isfinite(d), e * d, torch.zeros_like(d)).sum(1)
    zero = torch.zeros_like(s)
    lse = torch.where(valid, m.squeeze(1) + s.log(), zero)
    entropy = torch.where(valid, s.log() - t / s, zero)
    return -row_loss, lse, entropy, -g


def dlogits(g, u, labels):
    """the gradient for a per-row upstream u [rows]; ignored rows are exactly zero even where u is NaN"""
    out = g * u.double()[:, None]
    out[labels < 0] = 0.0
    return out


@functools.lru_cache(maxsize=None)
def expected(name):
    """-> float64 (logp, lse, entropy, onehot - softmax) of a case of _ce_ref.CASES; built once, never to be written to"""
    x, lab = inputs(name)
    return reference(x, lab)


def upstream(name):
    """fp32 u [rows] of a case: random per row; the first labelled row gets u = 0, the (first) ignored row NaN"""
    c = CASE_BY_NAME[name]
    _, lab = inputs(name)
    gen = torch.Generator().manual_seed(77 + CASES.index(c))
    u = torch.randn(c.rows, generator=gen) * 2.0
    u[int((lab >= 0).nonzero()[0])] = 0.0
    u[int((lab < 0).nonzero()[0])] = float("nan")
    return u


def entropy_moments(x, labels):
    """float64 per row: (E|d|, E d^2, log s, n_steps) under p = softmax(x), d = x - max(x): what the entropy kernel's error bound is made of
    (tests/test_token_logprob_gpu.py); n_steps = the vectors one thread walks (+ the tail)"""
    x = x.double()
    m = x.max(1, keepdim=True).values
    d = x - m
    e = torch.exp(d)
    s = e.sum(1)
    fin = torch.isfinite(d)
    d0 = torch.where(fin, d, torch.zeros_like(d))
    return (e * d0.abs()).sum(1) / s, (e * d0 * d0).sum(1) / s, s.log(), R.vectors_per_thread(x.shape[1])[1] + 1


def entropy_bound(x, labels):
    """float64 [rows]: the derived bound on |entropy_kernel - entropy_fp64| (derivation: docstring of tests/test_token_logprob_gpu.py)"""
    a1, a2, logs, n = entropy_moments(x, labels)
    C = 3.0 + 2.0 * (n + 1) + 0.5 * (n + 18)
    return EPS32 * (4.0 * a2 + (2.0 * C + 3.0) * a1 + C + 3.0 * logs.abs())


def align(per_row, B, S):
    """the alignment rule: per_row [B * S] indexed by the position of the SHIFTED label (row b * S + t - 1 scores labels[b, t]) -> [B, S] aligned with
    labels: entry [b, t] = per_row[b * S + t - 1] for t >= 1, 0 at t = 0"""
    return torch.nn.functional.pad(per_row.reshape(B, S)[:, :-1], (1, 0))


def token_logprobs_reference(logits, labels):
    """the five-line torch statement of out.token_logprobs: logits [B, S, V] (any float dtype), labels [B, S] -> float64 [B, S]"""
    lp = torch.log_softmax(logits.double()[:, :-1], -1)
    tgt = labels[:, 1:]
    got = lp.gather(-1, tgt.clamp_min(0)[..., None]).squeeze(-1)
    got = torch.where(tgt != IGNORE, got, torch.zeros_like(got))
    return torch.nn.functional.pad(got, (1, 0))


def token_entropy_reference(logits, labels):
    lsm = torch.log_softmax(logits.double()[:, :-1], -1)
    h = -(lsm.exp() * torch.where(torch.isfinite(lsm), lsm, torch.zeros_like(lsm))).sum(-1)
    return torch.nn.functional.pad(torch.where(labels[:, 1:] != IGNORE, h, torch.zeros_like(h)), (1, 0))

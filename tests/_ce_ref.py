"""Float64 reference of the loss head's cross-entropy kernel (csrc/ce.hip) and the inputs its tests share.

The operation, from the bf16 logits x [rows, V], labels (-100 = ignore), a denominator and an upstream gradient:
    row_loss = logsumexp(x) - x[label]                                  0 on an ignored row
    dlogits  = (softmax(x) - onehot(label)) * upstream / max(denom, 1)  0 on an ignored row
    loss     = sum(row_loss) / max(denom, 1)
written out directly (tests/test_loss_head_cpu.py holds it to torch.nn.functional.cross_entropy in float64).

The kernel's geometry decides which inputs reach which code: one block of THREADS threads per row, VEC-wide vectors dealt round-robin to the
threads (vector v belongs to thread v % THREADS), the V % VEC last columns as a scalar tail (tail element i belongs to thread i).  The helpers
below restate that geometry so the CPU test can assert that every builder still reaches the path it is named after.
"""
import functools
from collections import namedtuple

import torch

THREADS, VEC = 256, 8
IGNORE = -100
NEG_INF = float("-inf")


# ---------------------------------------------------------------------------------------------- the reference
def reference(x, labels, denom, upstream=1.0):
    """-> (row_loss [rows], dlogits [rows, V], loss) in float64 from logits of any float dtype (used as they are: pass the bf16 tensor)"""
    x = x.double()
    rows = x.shape[0]
    m = x.max(1, keepdim=True).values
    e = torch.exp(x - m)
    s = e.sum(1, keepdim=True)
    valid = labels >= 0
    at = labels.clamp_min(0)
    row_loss = (m + s.log()).squeeze(1) - x.gather(1, at[:, None]).squeeze(1)
    row_loss = torch.where(valid, row_loss, torch.zeros_like(row_loss))
    g = e / s
    g[torch.arange(rows), at] -= 1.0
    g[~valid] = 0.0
    d = max(float(denom), 1.0)
    return row_loss, g * (float(upstream) / d), row_loss.sum() / d


# ---------------------------------------------------------------------------------------------- geometry of ce_fwd_bwd_kernel
def n_vectors(V):
    return V // VEC


def vectors_per_thread(V):
    """(fewest, most) vectors any of the block's threads walks"""
    nv = n_vectors(V)
    return nv // THREADS, -(-nv // THREADS)


def tail_columns(V):
    return range(n_vectors(V) * VEC, V)


def owner_thread(col, V):
    t0 = n_vectors(V) * VEC
    return (col // VEC) % THREADS if col < t0 else (col - t0) % THREADS


def deliberate_labels(V):
    """the label positions where an index slip shows: both ends of the row, both ends of the scalar tail, the last lane of the first and of the
    last vector, columns owned by thread 255 (in its first and, where it has one, its second vector); duplicates dropped, order kept"""
    nv = n_vectors(V)
    want = [0, V - 1]
    if V % VEC:
        want += [nv * VEC, V - 1]
    if nv:
        want += [VEC - 1, VEC * (nv - 1) + VEC - 1]
    if nv >= THREADS:
        want.append(VEC * (THREADS - 1) + 3)
    if nv >= 2 * THREADS:
        want.append(VEC * (2 * THREADS - 1) + 5)
    return list(dict.fromkeys(want))


def place_labels(rows, V, gen, allowed=None):
    """deliberate positions first, then one ignored row, then random columns with every fifth row ignored; `allowed` (bool [V]) keeps labels
    off masked columns"""
    ok = (lambda c: True) if allowed is None else (lambda c: bool(allowed[c]))
    head = [c for c in deliberate_labels(V) if ok(c)]
    if allowed is not None:
        cols = allowed.nonzero().flatten()
        head += [int(cols[0]), int(cols[-1])]
        head = list(dict.fromkeys(head))
    lab = head[: rows - 1] + [IGNORE]
    pool = torch.arange(V) if allowed is None else allowed.nonzero().flatten()
    while len(lab) < rows:
        lab.append(IGNORE if len(lab) % 5 == 4 else int(pool[torch.randint(0, len(pool), (1,), generator=gen)]))
    return torch.tensor(lab[:rows], dtype=torch.int64)


# ---------------------------------------------------------------------------------------------- input builders: (rows, V, gen) -> fp32 logits, labels
SPIKE_BACK = 3   # the spike sits this many columns before the end of the row


def spike_column(V):
    return max(V - SPIKE_BACK, 0)


def masked_columns(V):
    """bool [V], True = -inf: columns [0, 64) (the first vector of threads 0..7), one whole vector in the middle of thread 100's sequence where
    that thread has three or more, and the first tail element"""
    mask = torch.zeros(V, dtype=torch.bool)
    mask[: min(64, V)] = True
    if vectors_per_thread(V)[0] >= 3:
        v = THREADS + 100
        mask[VEC * v: VEC * v + VEC] = True
    if V % VEC:
        mask[n_vectors(V) * VEC] = True
    return mask


def _random3(rows, V, gen):
    return torch.randn(rows, V, generator=gen) * 3.0, place_labels(rows, V, gen)


def _offset_up(rows, V, gen):
    x, lab = _random3(rows, V, gen)
    return x + 200.0, lab


def _offset_down(rows, V, gen):
    x, lab = _random3(rows, V, gen)
    return x - 200.0, lab


def _spike(rows, V, gen):
    x = torch.full((rows, V), -60.0)
    x[:, spike_column(V)] = 60.0
    lab = place_labels(rows, V, gen)
    lab[rows - 1] = spike_column(V)   # one row whose label is the spike itself: loss ~ 0, gradient ~ 0
    return x, lab


def _ramp(V):
    return torch.linspace(-40.0, 40.0, V) if V > 1 else torch.zeros(1)


def _ramp_up(rows, V, gen):
    return _ramp(V).repeat(rows, 1), place_labels(rows, V, gen)


def _ramp_down(rows, V, gen):
    return _ramp(V).flip(0).repeat(rows, 1), place_labels(rows, V, gen)


def _ramp_perm(rows, V, gen):
    r = _ramp(V)
    return torch.stack([r[torch.randperm(V, generator=gen)] for _ in range(rows)]), place_labels(rows, V, gen)


def _masked(rows, V, gen):
    mask = masked_columns(V)
    x = torch.randn(rows, V, generator=gen) * 3.0
    x[:, mask] = NEG_INF
    lab = place_labels(rows, V, gen, allowed=~mask)
    # last row: nothing but the label's logit is finite (loss 0, gradient 0), the label behind masked vectors of its own thread where it can be
    only = VEC * (2 * THREADS + 7) + 2 if n_vectors(V) > 2 * THREADS + 7 else V - 1
    x[rows - 1] = NEG_INF
    x[rows - 1, only] = 1.5
    lab[rows - 1] = only
    return x, lab


BUILDERS = {"random3": _random3, "offset_up": _offset_up, "offset_down": _offset_down, "spike": _spike, "ramp_up": _ramp_up,
            "ramp_down": _ramp_down, "ramp_perm": _ramp_perm, "masked": _masked}

# (rows, V, ld).  V % 8 != 0 needs rows that are views into a wider buffer (the ABI wants ld % 8 == 0): ld = roundup(V, 8) + 8, so a vector
# store that ran on to roundup(V, 8), or one vector further, lands on sentinels inside the buffer.
SHAPES = [(9, 5, 16), (9, 8, 8), (70, 2048, 2048), (16, 2048, 2048 + 64), (24, 2053, 2064), (24, 6285, 6296), (8, 152064, 152064)]
MASKED_MIN_V = 2048   # below this the masked columns [0, 64) would leave (nearly) nothing to label

Case = namedtuple("Case", "name builder rows V ld")
CASES = [Case(f"{b}-{rows}x{V}" + (f"-ld{ld}" if ld != V else ""), b, rows, V, ld)
         for b in BUILDERS for (rows, V, ld) in SHAPES if b != "masked" or V >= MASKED_MIN_V]
CASE_BY_NAME = {c.name: c for c in CASES}


@functools.lru_cache(maxsize=None)
def inputs(name):
    """-> (bf16 logits [rows, V], int64 labels [rows]) of a case, on the CPU; built once, never to be written to"""
    c = CASE_BY_NAME[name]
    gen = torch.Generator().manual_seed(1000 + CASES.index(c))
    x, lab = BUILDERS[c.builder](c.rows, c.V, gen)
    return x.to(torch.bfloat16), lab


@functools.lru_cache(maxsize=None)
def expected(name):
    """-> float64 (row_loss, dlogits) of a case at upstream = denom = 1; every other (upstream, denom) is a multiple of it"""
    x, lab = inputs(name)
    row_loss, g, _ = reference(x, lab, 1.0, 1.0)
    return row_loss, g

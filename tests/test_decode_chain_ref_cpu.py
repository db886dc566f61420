"""CPU: the integer references of tests/_chain_ref.py, before anything reaches a GPU (tests/test_decode_chain_exact_gpu.py launches exactly these cases).

1. every case's exactness conditions hold (reference() asserts them: every value at a rounding point an integer with |v| <= 256, every k column and every row of W
   in use, no two sequences with the same (pos, s_m));
2. sensitivity controls, stated on the reference alone: each way a kernel could be subtly wrong - the last K block dropped, one k element doubled, sequence m
   reading row M - 1, a neighbour's pos or s_m, the table halves or the gate / up halves swapped - changes at least one output element of every case it applies to.
   A launch that is bit-equal to the reference therefore makes none of these mistakes."""
import pytest
import torch

from tests import _chain_ref as R


def _differs(a, b):
    return any(not torch.equal(a[k], b[k]) for k in a if k not in ("gate", "up", "ss", "part_val", "part_idx", "token"))


@pytest.mark.parametrize("entry", R.ENTRIES)
def test_every_case_is_exact_and_every_mutation_shows(entry):
    cases = R.grid(entry)
    assert len(cases) >= (7 if entry in R.SINGLE else 14)
    assert {s for _, s in cases} == {False, True}, "one contiguous and one strided case per entry at least"
    zeros = values = 0
    for c, _ in cases:
        ref = R.reference(c)
        tag = f"{entry} M={c.M} K={c.K} N={c.N} seed {c.seed}"
        for v in ref.values():
            assert v.dtype in (torch.float64, torch.int64) and bool(torch.isfinite(v.double()).all()), tag
        if c.kind == "gu":   # the zero rule of the SwiGLU check needs zeros, the 2^-7 rule needs values
            zero = (ref["gate"] == 0) | (ref["up"] == 0)
            assert torch.equal(ref["act"] == 0, zero), tag
            zeros, values = zeros + int(zero.sum()), values + int((~zero).sum())
        if c.kind == "head" and c.N >= 32:
            assert bool(((ref["logits"] == ref["logits"].max(-1, keepdim=True).values).sum(-1) >= 1).all())
        applied = 0
        for mut in R.MUTATIONS:
            if R.applies(c, mut):
                applied += 1
                assert _differs(ref, R.reference(c, mut=mut)), f"{tag}: the reference does not see '{mut}'"
        assert applied >= 2
    assert R.kind_of(entry) != "gu" or (zeros >= 4 and values >= 500), (zeros, values)


def test_the_grid_reaches_every_listed_size():
    """every value of every list of the issue appears with every entry whose guard admits it, every M with at least two K's"""
    for entry in R.ENTRIES:
        cases = [c for c, _ in R.grid(entry)]
        kind, pipe = R.kind_of(entry), entry in R.PIPE_ONLY
        Ms = {c.M for c in cases}
        if entry in R.SINGLE:
            assert Ms == {1} and {c.K for c in cases} >= set(R.K_DOT)
        else:
            assert Ms == set(R.M_ALL[:7] if entry == "linear_residual_norm_batched" else R.M_ALL), entry
            for M in Ms:
                assert len({c.K for c in cases if c.M == M}) >= 2, (entry, M)
            assert {c.K for c in cases} >= set(R.K_MFMA if pipe else R.K_DOT), entry
            assert {c.K for c in cases if c.M > 8} >= (set(R.K_MFMA) if 9 in Ms else set()), entry
        if kind == "qkv":
            assert {c.heads for c in cases} == set(R.HEADS[:3] if pipe else R.HEADS), entry
        elif kind == "gu":
            assert {c.I for c in cases} == ({16, 48, 528} if pipe else {4, 16, 48, 528}), entry
        elif kind == "head":
            assert {c.N for c in cases} == ({32, 1056, 32768} if pipe else {8, 32, 1000, 1056, 32768}), entry
        elif entry == "linear_residual_ss_batched":
            assert {c.N for c in cases} == {64, 192} and {c.target for c in cases} == {False, True}
        elif entry == "linear_residual_norm_batched":
            assert {c.N for c in cases} == {32, 160}
        else:
            assert {c.N for c in cases} == {8, 32, 160}, entry
        for c in cases:   # what only the dot-product forms take never meets more than eight sequences or a matrix-pipe-only entry
            small = c.K % 64 != 0 or c.N % 32 != 0 or (kind == "gu" and c.I % 16 != 0) or (kind == "qkv" and c.heads[2] % 32 != 0)
            assert not (small and (pipe or c.M > 8)), (entry, c.M, c.K, c.N)


def test_handover_rows_are_exact_for_the_consumer():
    """linear + residual with the chosen residual leaves rows +-2^(m % 5): a norm-in-prologue case built on those rows is exact, and its statistic is the producer's
    per-block sums"""
    for M in (3, 8, 17):
        p = R.make("lin", M, 128, 7, N=192, target=True)
        out = R.reference(p)["out"]
        assert torch.equal(out, p.out_rows) and torch.equal(R.reference(p)["ss"].sum(1), 192 * p.s2 ** 2)
        for kind, kw in (("qkv", dict(heads=(2, 1, 32))), ("gu", dict(I=16)), ("head", dict(N=32))):
            c = R.make(kind, M, 192, 8, norm=True, rows=out, s_e0=0, **kw)
            assert torch.equal(c.x, out)
            R.reference(c)


def test_gaussian_restatement_sees_a_missed_window():
    """the gaussian cases: outputs at the scale the project's bars were set at, and a statistic that misses the window (rstd ~ 1000) far outside those bars"""
    for K, win in ((520, (512, 520)), (4160, (4096, 4160))):
        for kind, kw, key in (("head", dict(N=32), "logits"), ("qkv", dict(heads=(2, 1, 32)), "v"), ("gu", dict(I=16), "act")):
            c = R.gaussian(kind, 3, K, 5, win, **kw)
            ref, blind = R.reference(c)[key], R.reference(c, mut="stat_misses_window")[key]
            assert 0.2 < float(ref.std()) < 4.0, (kind, K, float(ref.std()))
            bar = 3e-2 + 3e-2 * ref.abs()
            # (SwiGLU forgives a hugely negative gate: silu -> 0)
            assert float(((blind - ref).abs() > 10 * bar).double().mean()) > (0.4 if kind == "gu" else 0.9), (kind, K)
    c = R.gaussian("lin", 3, 64, 6, (0, 64), norm=False, N=160, n2=True)
    ref, blind = R.reference(c)["h"], R.reference(c, mut="stat_misses_window")["h"]
    live = ref != 0
    assert int(live.sum()) >= 3 * 6 and bool(((blind - ref).abs()[live] > 10 * (3e-2 + 2e-2 * ref.abs()[live])).all())

"""CPU: the integer references of tests/_gemm_ref.py, before anything reaches a GPU (tests/test_gemm_exact_gpu.py launches exactly these cases).

1. every case's exactness conditions hold (reference() asserts them: every operand in {-1, 0, 1} with its edges planted, every value at a rounding point a value
   of its format with |v| <= 256, no empty split);
2. sensitivity controls, stated on the reference alone: each way a kernel could be subtly wrong - one k element dropped or doubled, a K tile dropped, a split's
   partial dropped or folded twice, a neighbouring row / column / bias element, the ragged mask one short or one long, the residual row not wrapped, accumulate or
   alpha ignored, the SwiGLU halves swapped, the rotate-half partner of the neighbouring head - changes the reference of every case it applies to.  A launch that is
   bit-equal to the reference therefore makes none of these mistakes;
3. the grid reaches every shape, split count and epilogue the GPU test is meant to launch, on the kernel meant to take it;
4. the host mirror of gemm_tile_of maps the workgroups of a launch one-to-one onto its tiles, for every tile count and group height."""
import pytest
import torch

from tests import _gemm_ref as R

GROUPS = sorted({c.group for c in R.grid()})


def _tag(c):
    return f"{c.group}: {c.kernel} {c.M}x{c.N}x{c.K} {c.epi} splits {c.splits} alpha {c.alpha} seed {c.seed}"


def _differs(a, b):
    return any(not torch.equal(a[k], b[k]) for k in a)


@pytest.mark.parametrize("group", GROUPS)
def test_every_case_is_exact_and_every_mutation_shows(group):
    cases = [c for c in R.grid() if c.group == group]
    assert {c.strided for c in cases} == {False, True}, "one contiguous and one strided case per group at least"
    seen = set()
    for c in cases:
        ref = R.reference(c)
        for v in ref.values():
            assert v.dtype == torch.float64 and bool(torch.isfinite(v).all()), _tag(c)
        assert tuple(ref["out"].shape) == (c.M, 2 * c.N if c.epi == "swiglu_bwd" else c.N)
        assert bool((ref["out"] != 0).any()), _tag(c)
        for t in (c.a, c.b, c.bias, c.res, c.base, c.gu, c.cos, c.sin):   # the operands are bf16 values
            assert t is None or torch.equal(t.to(R.BF).double(), t), _tag(c)
        applied = 0
        for mut in R.MUTATIONS:
            if R.applies(c, mut):
                applied += 1
                seen.add(mut)
                assert _differs(ref, R.reference(c, mut=mut)), f"{_tag(c)}: the reference does not see '{mut}'"
        assert applied >= (7 if c.M >= 2 else 5), _tag(c)
    assert seen >= {"drop_k", "double_k", "drop_k_tile", "col_next", "col_prev"}


def test_every_mutation_applies_somewhere():
    for mut in R.MUTATIONS:
        assert any(R.applies(c, mut) for c in R.grid()), mut


def test_the_planted_edges_are_certain():
    """a mistake confined to one (m, n, k) triple on planted edges changes the output for certain: a[m, k] b[n, k] = +-1 there"""
    for c in R.grid():
        ek, em, en = R.edge_k(c.K), R.edge_rows(c.M), R.edge_rows(c.N)
        assert {0, c.K - 1} <= set(ek) and {0, c.M - 1} <= set(em) and {0, c.N - 1} <= set(en)
        assert set(range(max(0, c.K - 8), c.K)) <= set(ek)
        for k0, k1 in R.split_ranges(c.kernel, c.K, c.splits):
            assert {k0, k1 - 1} <= set(ek), _tag(c)
        for t, sz in ((em, c.M), (en, c.N)):
            assert {r for r in range(sz) if r % 128 in (0, 127) or r % 256 in (0, 255)} <= set(t)
        assert bool((c.a[:, ek] * c.b[:1, ek] != 0).all()) and bool((c.a[em] != 0).all()) and bool((c.b[en] != 0).all()), _tag(c)


def test_the_grid_reaches_every_listed_size():
    """every value of every list of the issue appears on the kernel meant to take it"""
    G = R.grid()
    by = lambda group: [c for c in G if c.group == group]
    mnk = lambda cs: {(c.M, c.N, c.K) for c in cs}
    assert mnk(by("nt128")) == {(M, N, K) for M, N in R.NT128_MN for K in R.NT128_K} and len(by("nt128")) == 24
    assert {(c.K, c.splits) for c in by("nt128_splitk")} == set(R.NT128_SPLITS)
    assert {c.splits for c in by("nt128_splitk")} >= {2, 3} and any(c.splits == c.K // 64 for c in by("nt128_splitk"))
    assert any((c.K // 64) % c.splits for c in by("nt128_splitk")), "a ragged last split"
    assert mnk(by("nt256")) == {(M, N, K) for M, N in R.NT256_MN for K in R.NT256_K} | {(264, 264, 4160)}
    assert mnk(by("nn256")) == {(M, N, K) for M, N in R.XT_MN for K in R.NN_K}
    assert mnk(by("tn256")) == {(M, N, K) for M, N in R.XT_MN for K in R.TN_K}
    assert {8, 56, 64, 72, 100, 200, 1288} <= set(R.TN_K) and any(K % 2 for K in R.TN_K) and any(K % 8 and not K % 2 for K in R.TN_K)
    for kernel in ("nn256", "tn256"):
        cs = by(kernel + "_splitk")
        tiles = lambda c: R.cdiv(c.K, R.BK)
        assert {c.splits for c in cs} >= {2, 3, 16} and any(c.splits == tiles(c) and c.splits > 2 for c in cs), kernel
        assert any(tiles(c) % c.splits for c in cs) and {c.epi for c in cs} >= {"plain", "bias", "accum"}, kernel
        assert any(c.M * (c.N // 4) > 2048 * 256 for c in cs), "the fold kernel's grid cap"
        assert all(c.M * c.N <= 3_000_000 and c.K <= 4160 for c in cs)
    assert any(c.K % R.BK for c in by("tn256_splitk")), "a ragged last tile inside a split"
    gv = by("gemv")
    assert {c.M for c in gv} == {1} and {c.N for c in gv} == set(R.GEMV_N) and {c.K for c in gv} == set(R.GEMV_K)
    assert {(c.K, c.splits) for c in gv} == {(K, s) for K in R.GEMV_K for s in range(1, R.cdiv(K, 512) + 1)}
    assert {c.epi for c in gv} == {"plain", "bias_residual"}
    for kernel in ("nt128", "nt256", "nn256", "tn256"):
        cs = by("epilogues_" + kernel)
        assert all(c.kernel == kernel for c in cs)
        assert {c.epi for c in cs} >= set(R.EPI_BASIC) | {"res_mod", "accum_bias"}, kernel
        assert {c.M for c in cs if c.epi == "res_mod"} == {304 if kernel == "tn256" else 300, 96} and {c.res_mod for c in cs if c.epi == "res_mod"} == {96}
        assert {c.alpha for c in cs} == {1.0, 0.5, 2.0, -1.0}, kernel
        assert sum(c.epi == "swiglu_bwd" for c in cs) == 2, kernel
        if kernel != "nt128":   # the 128x128 kernel has the runtime-flag epilogue only, and no counter for it
            assert {R.generic(c) for c in cs} == {False, True}, kernel
            assert any(R.generic(c) and (c.M, c.K) == (520, 320) for c in cs), kernel
    assert {c.epi for c in by("swiglu_fwd")} == {"swiglu_fwd"} and {c.N for c in by("swiglu_fwd")} == {256, 512} and all(c.N % 256 == 0 for c in by("swiglu_fwd"))
    rope = by("rope")
    assert {c.epi for c in rope} == {"rope_lanes", "rope_pos", "rope_bias"} and any(c.M % c.S for c in rope) and all(c.N % 256 == 0 and c.rope_cols == 256 for c in rope)
    assert all(c.sub for c in by("sub")) and {c.kernel for c in by("sub")} == {"nt128", "nt256"}
    tm = by("tile_map")
    assert {(c.kernel, c.M, c.N, c.gm) for c in tm} == {(k, *R.TILE_MAP[k], g) for k in R.TILE_MAP for g in R.TILE_MAP_GM} and all(c.base is not None for c in tm)
    c = next(c for c in tm if c.kernel == "nt128")
    assert (R.cdiv(c.M, 128), R.cdiv(c.N, 128)) == (6, 3) and (6 * 3) % 8 == 2 and 6 % 4 == 2
    c = next(c for c in tm if c.kernel == "nt256")
    assert (R.cdiv(c.M, 256), R.cdiv(c.N, 256)) == (6, 4)
    assert {c.family for c in G} == {"gemm_nt128", "gemm_nt256", "gemm_nn256", "gemm_tn256", "gemv"}
    assert len(G) == len({c.seed for c in G}) and all(c.M * c.N < 3_000_000 and c.K <= 4160 for c in G)


def test_every_case_meets_the_guards_of_gemm_impl():
    """the guards of gemm_impl (csrc/gemm.hip), restated: no case of the grid is refused, every entry of REFUSED is"""
    def admitted(kernel, M, N, K, splits, flags=0):
        form = R.FORM[kernel]
        ok = 1 <= splits <= 64 and (splits == 1 or splits <= R.cdiv(K, 64)) and M > 0 and N > 0 and K > 0 and N % 4 == 0
        if kernel == "gemv":
            ok = ok and M == 1 and splits <= R.cdiv(K, 512)
        if form != "tn":
            ok = ok and K % 64 == 0
        if form != "nt":
            ok = ok and N % 8 == 0
        if form == "tn":
            ok = ok and M % 8 == 0
        if flags & R.GEMM_SWIGLU_FWD:
            ok = ok and form == "nt" and N % 256 == 0 and splits == 1
        return ok
    for c in R.grid():
        assert admitted(c.kernel, c.M, c.N, c.K, c.splits, c.flags), _tag(c)
        assert c.kernel != "gemv" or c.M == 1
    for kernel, M, N, K, splits, what in R.REFUSED:
        assert not admitted(kernel, M, N, K, splits), what


@pytest.mark.parametrize("gm", [0, 64, 1, 2, 3, 4, 8, 63])
def test_tile_map_is_a_bijection(gm):
    """workgroups 0 .. nwg - 1 map one-to-one onto the ntm x ntn tiles: none missed, none computed twice - for both kernels' tile counts (the tile size only
    enters through ntm, ntn), every group height, and the default (gm & 0x3f == 0 reads as 4)"""
    for ntm in range(1, 41):
        for ntn in range(1, 41):
            nwg = ntm * ntn
            tiles = [R.tile_of(b, nwg, ntm, ntn, gm) for b in range(nwg)]
            assert all(0 <= tm < ntm and 0 <= tn < ntn for tm, tn in tiles), (ntm, ntn, gm)
            assert len(set(tiles)) == nwg, (ntm, ntn, gm)
    if gm in (0, 64):
        assert [R.tile_of(b, 18, 6, 3, gm) for b in range(18)] == [R.tile_of(b, 18, 6, 3, 4) for b in range(18)]


def test_tile_map_of_the_launched_cases():
    """the two shapes the GPU test runs under every group height: nwg % 8 != 0, ntm % GM != 0 for GM = 4 and 8, a last group shorter than the others"""
    for (M, N), t in ((R.TILE_MAP["nt128"], 128), (R.TILE_MAP["nt256"], 256)):
        ntm, ntn = R.cdiv(M, t), R.cdiv(N, t)
        for gm in R.TILE_MAP_GM:
            tiles = [R.tile_of(b, ntm * ntn, ntm, ntn, gm or 0) for b in range(ntm * ntn)]
            assert sorted(tiles) == [(i, j) for i in range(ntm) for j in range(ntn)]
    assert (6 * 3) % 8 and 6 % 4 and 6 % 8

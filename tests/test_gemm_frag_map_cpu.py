"""Host model of the lane maps of the 256x256 GEMM kernels for both MFMA shapes (csrc/gemm_common.h, gemm256.hip, gemm256t.hip).

Each map below is one small function that mirrors, line by line, the device function or formula of the same name; the kernels' comments cite the
same formulas.  Checked here, without a GPU:
  * every fragment read touches each of the 64 LDS banks at most once per lane group of the instruction (ds_read_b128: four 16-lane groups,
    ds_read_b64_tr_b16: two 32-lane halves; bank of byte address a = (a / 4) mod 64), for every tile, k-step and both reads of a tr pair;
  * every fragment read fetches the (row, k) elements the MFMA operand layout wants (an image that is not the identity would still be conflict-free);
  * the epilogue map (accumulator tile, register, lane) -> (m, n) after the lane-pair exchange is a bijection onto the wave's 128 x 64 block with
    8 consecutive columns of one row per lane and piece.
"""
import itertools

import pytest

# ds_read_b128 is serviced in four groups of 16 lanes, ds_read_b64_tr_b16 in two halves of 32 (LDS table of the machine guide)
B128_GROUPS = [
    [0, 1, 2, 3, 12, 13, 14, 15, 20, 21, 22, 23, 24, 25, 26, 27],
    [4, 5, 6, 7, 8, 9, 10, 11, 16, 17, 18, 19, 28, 29, 30, 31],
    [32, 33, 34, 35, 44, 45, 46, 47, 52, 53, 54, 55, 56, 57, 58, 59],
    [36, 37, 38, 39, 40, 41, 42, 43, 48, 49, 50, 51, 60, 61, 62, 63],
]
TR_GROUPS = [list(range(0, 32)), list(range(32, 64))]
ROWB = 128    # bytes per row of the k-contiguous image (64 bf16)
TROW = 512    # bytes per k-row of the reduction-major image (256 bf16)
SHAPES = (32, 16)


def banks(addr, nbytes):
    return [((addr + 4 * d) // 4) % 64 for d in range(nbytes // 4)]


def assert_conflict_free(addrs, nbytes, groups, what):
    assert sorted(l for g in groups for l in g) == list(range(64))
    for g in groups:
        seen = {}
        for lane in g:
            for b in banks(addrs[lane], nbytes):
                assert seen.setdefault(b, addrs[lane]) == addrs[lane], f"{what}: bank {b} hit twice in lane group {g[:4]}.. (lane {lane})"
        assert len(seen) == len(g) * nbytes // 4


# ---------------------------------------------------------------- k-contiguous image (gemm_common.h)
def image_off(row, chunk):
    """byte offset of 16-byte chunk `chunk` (8 k) of image row `row`: the chunk sits at position chunk ^ ((row >> 1) & 7)"""
    return row * ROWB + ((chunk ^ ((row >> 1) & 7)) << 4)


def gemm_frag_row(mf, lane):
    return lane & 15 if mf == 16 else lane & 31


def gemm_frag_koff(mf, x, lane):
    chunk = 4 * (x & 1) + (lane >> 4) if mf == 16 else 2 * x + (lane >> 5)
    return (chunk ^ ((lane >> 1) & 7)) << 4


def gemm_frag_rowoff(mf, x):
    return (x >> 1) * 16 if mf == 16 else 0


def frag_addr(mf, tile32, x, lane):
    """byte address (inside an operand image) that `lane` reads for fragment x of the 32-row tile tile32"""
    return (32 * tile32 + gemm_frag_row(mf, lane)) * ROWB + gemm_frag_rowoff(mf, x) * ROWB + gemm_frag_koff(mf, x, lane)


def frag_wants(mf, tile32, x, lane):
    """(row, first k) the MFMA operand layout wants in `lane`: 32x32x16 - row lane & 31, k = 16 s + 8 (lane >> 5); 16x16x32 - row lane & 15, k = 32 s + 8 (lane >> 4)"""
    if mf == 16:
        return 32 * tile32 + 16 * (x >> 1) + (lane & 15), 32 * (x & 1) + 8 * (lane >> 4)
    return 32 * tile32 + (lane & 31), 16 * x + 8 * (lane >> 5)


@pytest.mark.parametrize("mf", SHAPES)
def test_row_fragments_conflict_free_and_right(mf):
    ksteps = set()
    for tile32, x in itertools.product(range(8), range(4)):      # 8 tiles of 32 rows = one 256-row operand image
        addrs = [frag_addr(mf, tile32, x, lane) for lane in range(64)]
        assert_conflict_free(addrs, 16, B128_GROUPS, f"ds_read_b128 mf={mf} tile={tile32} x={x}")
        for lane in range(64):
            row, k0 = frag_wants(mf, tile32, x, lane)
            assert addrs[lane] == image_off(row, k0 // 8)
            ksteps.add((row, k0))
    assert len(ksteps) == 256 * 8     # the 32 fragments cover every (row, 8-k chunk) of the image once


# ---------------------------------------------------------------- reduction-major image (gemm256t.hip)
def tswz(r):
    return ((r & 3) << 2) | ((r >> 2) & 3)


def timage_off(krow, col):
    """byte offset of element (k-row, column): 16-byte chunk c = col / 8 of k-row r sits at c ^ tswz(r)"""
    return krow * TROW + (((col >> 3) ^ tswz(krow)) << 4) + 2 * (col & 7)


def tr_off(mf, tile, pc, lane):
    g, i = lane >> 4, lane & 15
    chunk = 2 * tile + ((i & 3) >> 1) if mf == 16 else 4 * tile + 2 * (g & 1) + ((i & 3) >> 1)
    r = (8 * g if mf == 16 else 8 * (g >> 1)) + (i >> 2) + 4 * pc
    return r * TROW + ((chunk ^ tswz(r)) << 4) + 8 * (i & 1)


def tr_kstep_bytes(mf, s):
    return s * (48 - mf) * TROW     # k-step s starts at k-row 16 s (32x32x16) / 32 s (16x16x32)


@pytest.mark.parametrize("mf", SHAPES)
def test_transposed_fragments_conflict_free_and_right(mf):
    ntiles, nsteps = (16, 2) if mf == 16 else (8, 4)
    covered = set()
    for tile, s, pc in itertools.product(range(ntiles), range(nsteps), range(2)):
        addrs = [tr_off(mf, tile, pc, lane) + tr_kstep_bytes(mf, s) for lane in range(64)]
        assert tr_kstep_bytes(mf, s) < 65536          # stays an immediate of the ds instruction
        assert all(a % 8 == 0 and a + 8 <= 64 * TROW for a in addrs)
        assert_conflict_free(addrs, 8, TR_GROUPS, f"ds_read_b64_tr_b16 mf={mf} tile={tile} s={s} pc={pc}")
        # the instruction: lane 4 q + p of a 16-lane group supplies 4 columns of row q; lane i of the group receives column i of rows 0..3 (element q)
        for lane in range(64):
            g, i = lane >> 4, lane & 15
            if mf == 16:
                col, k0 = 16 * tile + i, 32 * s + 8 * g + 4 * pc
            else:
                col, k0 = 32 * tile + 16 * (g & 1) + i, 16 * s + 8 * (g >> 1) + 4 * pc
            for q in range(4):
                src = 16 * g + 4 * q + (i >> 2)        # the lane of the group whose address covers column i of row q
                assert addrs[src] + 2 * (i & 3) == timage_off(k0 + q, col)
                covered.add((k0 + q, col))
    assert len(covered) == 64 * 256
    # the swizzle term must not depend on the k-step, or the offsets would not be lane constants
    for r in range(64):
        assert tswz(r) == tswz(r % 16) == tswz(r % 32)


def test_tn_tail_mask_follows_the_lane_k_map():
    """TN zeroes the A fragments of the last tile for k >= K: element e of fragment s of phase ph holds k = ..."""
    for mf in SHAPES:
        for ph, s, lane, e in itertools.product(range(2), range(2), range(64), range(8)):
            k_mask = (32 * ph + 8 * (lane >> 4) if mf == 16 else 16 * (2 * ph + s) + 8 * (lane >> 5)) + e
            # k the two tr reads of that fragment deliver into element e (pc = e >> 2, row q = e & 3)
            kstep = ph if mf == 16 else 2 * ph + s
            r0 = (8 * (lane >> 4) if mf == 16 else 8 * (lane >> 5)) + 4 * (e >> 2) + (e & 3)
            assert k_mask == r0 + kstep * (48 - mf)


# ---------------------------------------------------------------- epilogue (gemm_common.h)
def acc_pos(mf, it, jt, reg, lane):
    """(m, n) inside the wave's 128 x 64 block of accumulator register `reg` of tile (it, jt) after mfma(bfrag, afrag, acc)"""
    if mf == 16:       # 16 x 16 tiles, 4 registers
        return 16 * it + (lane & 15), 16 * jt + 4 * (lane >> 4) + reg
    return 32 * it + (lane & 31), 32 * jt + 8 * (reg >> 2) + 4 * (lane >> 5) + (reg & 3)      # 32 x 32 blocks, 16 registers


def block_reg(mf, i, j, idx):
    """GemmAcc<MF>::block(i, j)[idx], idx = 8 t + 4 h + e -> (tile row, tile column, register)"""
    if mf == 16:
        t, h, e = idx >> 3, (idx >> 2) & 1, idx & 3
        return 2 * i + h, 2 * j + t, e
    return i, j, idx


def lane_swap(mf, x, y):
    """gemm_lane_swap: x, y are 64-lane vectors; v_permlane32_swap / v_permlane16_swap exchange the odd rows of x with the even rows of y"""
    w = mf                       # row width of the exchange: 32 or 16 lanes
    lo, hi = list(x), list(y)
    for lane in range(64):
        if (lane // w) & 1 == 0:     # even row: y's even row goes to x's next (odd) row and the other way round
            lo[lane + w], hi[lane] = y[lane], x[lane + w]
    return lo, hi


@pytest.mark.parametrize("mf", SHAPES)
def test_epilogue_map_is_a_bijection_with_8_consecutive_columns(mf):
    seen = {}
    for i, j, t in itertools.product(range(4), range(2), range(2)):          # 16 pieces of a wave, as in the kernels' epilogues
        v = [[None] * 8 for _ in range(64)]
        for e in range(4):
            x = [acc_pos(mf, *block_reg(mf, i, j, 8 * t + e), lane) for lane in range(64)]
            y = [acc_pos(mf, *block_reg(mf, i, j, 8 * t + 4 + e), lane) for lane in range(64)]
            lo, hi = lane_swap(mf, x, y)
            for lane in range(64):
                v[lane][e], v[lane][4 + e] = lo[lane], hi[lane]
        for lane in range(64):
            m, n = 32 * i + (lane & 31), 32 * j + 16 * t + 8 * (lane >> 5)     # what gemm_store_block32_body / the SwiGLU and RoPE epilogues assume
            assert v[lane] == [(m, n + c) for c in range(8)], (mf, i, j, t, lane, v[lane])
            for pos in v[lane]:
                assert pos not in seen
                seen[pos] = (i, j, t, lane)
    assert sorted(seen) == [(m, n) for m in range(128) for n in range(64)]


@pytest.mark.parametrize("mf", SHAPES)
def test_narrow_and_partial_stores_cover_the_block_once(mf):
    """gemm_quad_pos: (row, column) of b[8 t + 4 h + 0..3] before any exchange (4-wide stores, split-K partials)"""
    seen = set()
    for i, j, t, h, lane in itertools.product(range(4), range(2), range(2), range(2), range(64)):
        row, col = (16 * h + (lane & 15), 16 * t + 4 * (lane >> 4)) if mf == 16 else (lane & 31, 8 * (2 * t + h) + 4 * (lane >> 5))
        for e in range(4):
            assert acc_pos(mf, *block_reg(mf, i, j, 8 * t + 4 * h + e), lane) == (32 * i + row, 32 * j + col + e)
            seen.add((32 * i + row, 32 * j + col + e))
    assert len(seen) == 128 * 64


@pytest.mark.parametrize("mf", SHAPES)
def test_mfma_schedule_uses_every_fragment_pair_once(mf):
    """the MFMA groups / slots of a K-tile (gemm256.hip mfma_group, mfma_slot; gemm256t.hip TN slots) multiply every A tile with every B tile over every k-step once"""
    def nt_ktile():
        out = []
        for acc0 in (0, 2):     # MFMA_a (groups) and MFMA_b (slots)
            for q in range(8):
                if mf == 32:
                    s, i = q >> 1, q & 1
                    out += [((acc0 + i, s), (j, s)) for j in range(2)]                     # (A 32-tile, k-step), (B 32-tile, k-step)
                else:
                    s, i, ih = q >> 2, (q >> 1) & 1, q & 1
                    out += [((2 * (acc0 + i) + ih, s), (jt, s)) for jt in range(4)]        # 16-tiles
        return out

    def tn_ktile():
        out = []
        for ph in range(2):
            for q in range(8):
                if mf == 32:
                    s, i = q >> 2, q & 3
                    out += [((i, 2 * ph + s), (j, 2 * ph + s)) for j in range(2)]
                else:
                    i, ih = q >> 1, q & 1
                    out += [((2 * i + ih, ph), (jt, ph)) for jt in range(4)]
        return out

    na, nb, nk = (8, 4, 2) if mf == 16 else (4, 2, 4)
    want = sorted(((a, s), (b, s)) for a in range(na) for b in range(nb) for s in range(nk))
    assert sorted(nt_ktile()) == want
    assert sorted(tn_ktile()) == want

"""tests/_frontend_ref.py held to something independent, on the CPU: logmel_ref against transformers' WhisperFeatureExtractor (numpy path), the derived
log-mel bound against four real mistakes (each must exceed it on at least 5 % of the outputs) and against a torch fp32 restatement of the kernel's steps
(within it everywhere), the share of outputs the bound leaves out (at most 1 %, from the reference alone), the data-movement references against
F.conv1d / autograd / their own adjoints at tiny shapes, and every case named for a seam against the geometry helper that says it sits on it.  No GPU.

Measured here: the fp32 restatement reaches 0.005 - 0.020 of the bound (median bound 6e-5 - 9e-5); left-out share at most 2.7e-3, near-floor share at most
2.4e-4; the four mutations exceed the bound on 7 % - 100 % of the outputs and by 83x - 790000x at their worst output; logmel_ref is within 0.31 - 0.76 of
what the extractor's own fp32 steps allow (at most 1.2e-7).  Module wall time 6 s."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import _frontend_ref as R
from tests import _norm_ref as N

BF = torch.bfloat16
CASE_IDS = [f"W{w}_T{n // R.HOP}_mels{m}" for w, n, m in R.LOGMEL_CASES]


@pytest.fixture(scope="module")
def bounds():
    cache = {}

    def get(W, nsamp, n_mels):
        if (W, nsamp, n_mels) not in cache:
            cache[(W, nsamp, n_mels)] = R.logmel_bound(R.logmel_wave(W, nsamp), n_mels)
        return cache[(W, nsamp, n_mels)]
    return get


# ---------------------------------------------------------------------------------------------- log-mel
def _half_ulp32(a):
    """half an fp32 unit in the last place of a"""
    return np.ldexp(1.0, np.frexp(np.abs(a) + N.TINY)[1] - 25)


def _extractor(n_mels):
    from transformers import WhisperFeatureExtractor

    return WhisperFeatureExtractor(feature_size=n_mels, sampling_rate=16000, hop_length=160, chunk_length=30, n_fft=400)


@pytest.mark.parametrize("n_mels", [128, 64])
def test_mel_bank_is_the_extractor_s(n_mels):
    from audio_flamingo_amd.frontend import mel_filter_bank

    assert np.array_equal(mel_filter_bank(n_mels), _extractor(n_mels).mel_filters)
    assert R.mel_bank(n_mels).dtype == np.float32 and R.mel_bank(n_mels).shape == (R.N_BINS, n_mels)


def test_logmel_ref_is_the_whisper_feature_extractor():
    """_np_extract_fbank_features itself takes any length (the padding to 30 s is done by its caller, the extractor's __call__), so the input of every
    case is compared whole, and one 30 s case (the first two window kinds at 480000 samples) with all of its 3000 frames.  The 264000-sample case is the
    same code path at a length in between and is left to the 30 s one."""
    for W, nsamp, n_mels in list(R.LOGMEL_CASES[:4]) + [(2, 480000, 128)]:
        wav = R.logmel_wave(W, nsamp)
        fe = _extractor(n_mels)
        theirs = np.stack([np.asarray(fe._np_extract_fbank_features(wav[w: w + 1], "cpu"))[0] for w in range(W)])   # one window per call: its max is per call
        ours = R.logmel_ref(wav, n_mels)
        assert theirs.shape == ours.shape == (W, n_mels, nsamp // R.HOP)
        err = np.abs(theirs.astype(np.float64) - ours)
        # the extractor works in float64 but STORES the spectrum as complex64 (re and im relative 2^-24 each: the power relative 2^-23), uses the float64
        # mel bank (ours: the fp32 bank the kernel reads, relative 2^-24 on non-negative terms), rounds log10 to fp32 and does the floor and (. + 4) / 4 in fp32
        v = np.log10(np.maximum(np.power(10.0, 4.0 * ours - 4.0), 1e-10))
        mx = v.max(axis=(1, 2), keepdims=True)
        e_v = 1.01 * 3 * R.E32 / np.log(10) + _half_ulp32(v)
        e_floor = 1.01 * 3 * R.E32 / np.log(10) + _half_ulp32(mx) + _half_ulp32(mx - 8.0)
        tol = 0.25 * (np.maximum(e_v, e_floor) + _half_ulp32(4.0 * ours))
        worst = float((err / tol).max())
        print(f"logmel_ref vs WhisperFeatureExtractor W={W} nsamp={nsamp} n_mels={n_mels}: max error {err.max():.3g}, {worst:.3f} of what its fp32 steps allow")
        assert worst <= 1.0


@pytest.mark.parametrize("W,nsamp,n_mels", R.LOGMEL_CASES, ids=CASE_IDS)
def test_left_out_share_and_fp32_restatement(bounds, W, nsamp, n_mels):
    b = bounds(W, nsamp, n_mels)
    assert b.left_out <= R.SHARE_CAP and b.near_floor <= R.SHARE_CAP, (b.left_out, b.near_floor)
    assert np.isfinite(b.bound[b.keep]).all() and (b.bound > 0).all()
    got = R.logmel_fp32_restatement(R.logmel_wave(W, nsamp), n_mels).numpy()
    r = R.logmel_ratio(got, b)
    print(f"fp32 restatement: {r:.4f} of the bound; left out {b.left_out:.2e}, near the floor {b.near_floor:.2e}, median bound {np.median(b.bound):.2e}")
    assert r <= 1.0


@pytest.mark.parametrize("mutation", R.MUTATIONS)
@pytest.mark.parametrize("W,nsamp,n_mels", [(3, 480, 128)] + list(R.LOGMEL_CASES[1:4]), ids=["W3_T3_mels128"] + CASE_IDS[1:4])
def test_bound_rejects_real_mistakes(bounds, W, nsamp, n_mels, mutation):
    """T = 3 is run with three windows here: one max over a batch of one window is no mistake"""
    b = bounds(W, nsamp, n_mels)
    wrong = R.logmel_ref(R.logmel_wave(W, nsamp), n_mels, mutation)
    over = (np.abs(wrong - b.ref) / b.bound)[b.keep]
    share = float((over > 1.0).mean())
    print(f"{mutation}: beyond the bound on {share:.3f} of the outputs, {over.max():.0f}x at the worst")
    assert share >= 0.05, (mutation, share)


@pytest.mark.parametrize("W,nsamp,n_mels", [(3, 480, 128)] + list(R.LOGMEL_CASES[1:4]), ids=["W3_T3_mels128"] + CASE_IDS[1:4])
def test_bound_rejects_a_mirror_off_by_one(bounds, W, nsamp, n_mels):
    """the mirrored index itself one sample off reaches only the frames that touch the padding: the first two and the last"""
    b = bounds(W, nsamp, n_mels)
    T = nsamp // R.HOP
    wrong = R.logmel_ref(R.logmel_wave(W, nsamp), n_mels, "reflect_off_by_one")
    over = np.where(b.keep, np.abs(wrong - b.ref) / b.bound, 0.0)
    edge = sorted({0, 1, T - 1})
    inner = [t for t in range(T) if t not in edge]
    assert float((over[:, :, edge] > 1.0).mean()) >= 0.05
    assert not (over[:2, :, inner] > 1.0).any(), "a frame clear of the padding moved (windows whose floor does not move)"


# ---------------------------------------------------------------------------------------------- rotary_time
@pytest.mark.parametrize("rows,E,Rr", R.ROTARY_CASES[:4])
def test_rotary_reference_is_the_formula_and_its_adjoint(rows, E, Rr):
    x, dy = R.gauss((rows, E), 1), R.gauss((rows, E), 2)
    ang = R.gauss((rows, Rr), 3, 3.0, torch.float32)
    cos, sin = ang.cos(), ang.sin()
    y, yb = R.rotary_time_ref(x, cos, sin)
    xr = x.double().requires_grad_(True)
    f = R.rotary_formula(xr, cos, sin)
    assert torch.equal(y, f.detach())
    f.backward(dy.double())
    dx, db = R.rotary_time_ref(dy, cos, sin, backward=True)
    assert float((dx - xr.grad).abs().max()) < 1e-14
    assert torch.equal(y[:, Rr:], x.double()[:, Rr:]) and bool((yb[:, Rr:] == 0).all()) and bool((yb[:, :Rr] > 0).all())
    # an fp32 evaluation rounded once is within the bound; a second bf16 rounding of a product is not
    c, s = cos.float(), sin.float()
    if Rr:
        x0, x1 = x.float()[:, 0:Rr:2], x.float()[:, 1:Rr:2]
        y0 = (x0 * c[:, 0::2] - x1 * s[:, 0::2]).to(BF)
        assert N.ratio(y0, y[:, 0:Rr:2], yb[:, 0:Rr:2]) <= 1.0
        if rows * Rr >= 200:
            twice = ((x0 * c[:, 0::2]).to(BF).float() - x1 * s[:, 0::2]).to(BF)
            assert N.ratio(twice, y[:, 0:Rr:2], yb[:, 0:Rr:2]) > 1.0


# ---------------------------------------------------------------------------------------------- data movement
def _int(shape, seed):
    return R.int_data(shape, seed)


@pytest.mark.parametrize("W,Tin,C", [(1, 1, 8), (2, 2, 8), (3, 3, 8), (2, 6, 16), (2, 7, 16)])
def test_col2im2_is_the_exact_adjoint_of_im2col2(W, Tin, C):
    To = R.tout(Tin)
    h, dcol = _int((W * Tin, C), 1), _int((W * To, 3 * C), 2)
    col, dh = R.im2col2(h, W, Tin, C), R.col2im2(dcol, W, Tin, C)
    assert col.shape == (W * To, 3 * C) and dh.shape == (W * Tin, C)
    assert float((col.double() * dcol.double()).sum()) == float((h.double() * dh.double()).sum())
    # and of float64 autograd through the definition
    hr = h.double().requires_grad_(True)
    R.im2col2(hr, W, Tin, C).backward(dcol.double())
    assert torch.equal(hr.grad, dh.double())


@pytest.mark.parametrize("W,C,T", [(2, 8, 1), (2, 3, 5), (1, 5, 7)])
def test_conv1_is_im2col1_times_the_permuted_weight(W, C, T):
    Co = 4
    x, w = _int((W, C, T), 3), _int((Co, C, 3), 4)
    ref = F.conv1d(x.double(), w.double(), padding=1)                                  # [W, Co, T]
    got = R.im2col1(x).double() @ R.weight_to_gemm(w).double().t()                      # [W T, Co]
    assert torch.equal(got.reshape(W, T, Co).permute(0, 2, 1), ref)
    assert torch.equal(R.im2col1(x.float()), R.im2col1(x))


@pytest.mark.parametrize("W,Tin,C", [(1, 1, 8), (2, 2, 8), (2, 3, 8), (2, 6, 8), (3, 7, 8)])
def test_conv2_is_im2col2_times_the_permuted_weight(W, Tin, C):
    Co = 4
    h, w = _int((W * Tin, C), 5), _int((Co, C, 3), 6)
    ref = F.conv1d(h.double().reshape(W, Tin, C).permute(0, 2, 1), w.double(), stride=2, padding=1)   # [W, Co, Tout]
    assert ref.shape[-1] == R.tout(Tin)
    got = R.im2col2(h, W, Tin, C).double() @ R.weight_to_gemm(w).double().t()
    assert torch.equal(got.reshape(W, R.tout(Tin), Co).permute(0, 2, 1), ref)


def test_weight_permutation_round_trip_and_accumulate():
    w, old = R.gauss((3, 5, 3), 1), R.gauss((3, 5, 3), 2)
    wp = R.weight_to_gemm(w)
    assert torch.equal(R.weight_grad_from_gemm(wp, torch.zeros_like(w), False), w)
    for co, ci, kk in [(0, 0, 0), (2, 4, 2), (1, 3, 1)]:
        assert wp[co, kk * 5 + ci] == w[co, ci, kk]
    acc = R.weight_grad_from_gemm(wp, old, True)
    assert torch.equal(acc, (old.float() + w.float()).to(BF)) and not torch.equal(acc, w)


def test_pool_references_and_their_special_inputs():
    x = R.pool_input(5, 72, 1)
    y = R.avgpool2_fwd(x, 5, 72)
    assert torch.equal(y.float(), F.avg_pool1d(x.float().t()[None], 2)[0].t().to(BF).float())
    assert y[0, 0] == 1.0 and y[0, 1] == 1.0 + 2.0 ** -6 and y[0, 2] == 0 and y[0, 3] == 0, "the two ties go to even; x + (-x) is 0"
    dy = R.gauss((5, 72), 2)
    xr = x.float().requires_grad_(True)
    F.avg_pool1d(xr.t()[None], 2)[0].t().backward(dy.float())
    assert torch.equal(R.avgpool2_bwd(dy, 5, 72).float(), xr.grad)


@pytest.mark.parametrize("n", R.SCAN_N[:8])
@pytest.mark.parametrize("pattern", R.SCAN_PATTERNS)
def test_placeholder_scan_reference_is_masked_scatter_order(n, pattern):
    ids = R.scan_ids(n, pattern)
    src, cnt = R.placeholder_scan(ids, R.AUDIO_ID)
    m = ids == R.AUDIO_ID
    assert cnt == int(m.sum()) and torch.equal(src[m].long(), torch.arange(cnt)) and bool((src[~m] == -1).all())
    H = 8
    embed, audio = R.gauss((50, H), 1), R.gauss((max(cnt, 1), H), 2)
    ref = embed[ids].clone()
    ref.masked_scatter_(m[:, None].expand(-1, H), audio[:cnt])
    assert torch.equal(R.embed_scatter_fwd(ids, src, embed, audio), ref)


def test_embed_scatter_bwd_reference():
    """small integers: equal to index_add_ exactly (any order); gaussian: equal to an explicit row-by-row fp32 loop, the kernel's stated order"""
    n, H, V = 300, 8, 50
    ids = R.scan_ids(n, "random_0.5")
    src, cnt = R.placeholder_scan(ids, R.AUDIO_ID)
    old = R.gauss((V, H), 3)
    for dout in (R.int_data((n, H), 4), R.gauss((n, H), 5)):
        de, da = R.embed_scatter_bwd(ids, src, dout, old, cnt)
        assert torch.equal(da, dout[src >= 0])
        acc = torch.zeros((V, H))
        for r in range(n):
            if src[r] < 0:
                acc[ids[r]] = acc[ids[r]] + dout[r].float()
        want = old.clone()
        seen = torch.unique(ids[src < 0])
        want[seen] = (old[seen].float() + acc[seen]).to(BF)
        assert torch.equal(R.bits(de), R.bits(want))
        never = torch.ones(V, dtype=torch.bool)
        never[seen] = False
        assert bool(never.any()) and torch.equal(R.bits(de[never]), R.bits(old[never]))
    ref = torch.zeros((V, H)).index_add_(0, ids[src < 0], R.int_data((n, H), 4)[src < 0].float())
    de, _ = R.embed_scatter_bwd(ids, src, R.int_data((n, H), 4), torch.zeros((V, H), dtype=BF), cnt)
    assert torch.equal(de.float(), ref)
    assert R.embed_scatter_bwd(ids, src, dout, None, cnt)[0] is None and R.embed_scatter_bwd(ids, None, dout, old, None)[1] is None


def test_transposes_kv_append_and_rows():
    x = R.gauss((5, 24), 1)
    t = R.transpose(x, 64)
    assert t.shape == (24, 64) and torch.equal(t[:, :5], x.t()) and bool((t[:, 5:] == 0).all())
    B, S, H, D, spad = 2, 3, 2, 8, 64
    xx = R.gauss((B * S, H * D + 8), 2)
    th = R.transpose_heads(xx, B, S, H, D, spad)
    for b, s, h, d in [(0, 0, 0, 0), (1, 2, 1, 7), (1, 0, 1, 3)]:
        assert th[b, h, d, s] == xx[b * S + s, h * D + d]
    assert bool((th[..., S:] == 0).all())
    n, Hkv, Hq, start, Smax, Spad = 2, 2, 3, 3, 7, 64
    nk = Hkv * D
    qkv = R.gauss((B * n, Hq * D + 2 * nk + 8), 3)
    Kc, Vt = torch.full((B, Smax, nk), R.NAN, dtype=BF), torch.full((B, Hkv, D, Spad), R.NAN, dtype=BF)
    K2, V2 = R.kv_append(Kc, Vt, qkv, Hq * D, start, B, n, Hkv, D)
    for b, i, h, d in [(0, 0, 0, 0), (1, 1, 1, 7), (1, 0, 0, 5)]:
        assert K2[b, start + i, h * D + d] == qkv[b * n + i, Hq * D + h * D + d] and V2[b, h, d, start + i] == qkv[b * n + i, Hq * D + nk + h * D + d]
    assert int(torch.isnan(K2.float()).sum()) == B * (Smax - n) * nk and int(torch.isnan(V2.float()).sum()) == B * nk * (Spad - n)
    rows = torch.tensor([0, 2, 4])
    assert torch.equal(R.scatter_rows(R.gather_rows(x, rows), rows, 5)[rows], x[rows]) and bool((R.scatter_rows(R.gather_rows(x, rows), rows, 5)[[1, 3]] == 0).all())


def test_cast_input_holds_what_it_is_named_for():
    x = R.cast_input(1000)
    b = x.to(BF)
    assert bool(torch.isnan(x).any()) and bool(torch.isinf(x).sum() == 2) and bool((x == 0).sum() >= 2)
    assert bool(((x != 0) & (x.abs() < 2.0 ** -126)).sum() >= 4), "subnormals"
    assert bool((torch.isfinite(x) & torch.isinf(b.float())).sum() >= 3), "the largest finite fp32 values round to inf"
    assert bool(((R.bits(x) & 0xFFFF) == 0x8000).sum() >= 5), "exact ties"
    one = R.ROUNDING_SPECIAL.to(BF).float()
    assert one.tolist() == [1.0, 1.015625, -1.0, -1.015625, 2.0, 2.0, 1.0078125, 1.0]
    assert bool(((R.bits(R.cast_input(1)) & 0xFFFF) == 0x8000).all())
    xf = R.conv1_input(2, 8, 1, 1, torch.float32)
    assert torch.equal(xf.view(-1)[:8], R.ROUNDING_SPECIAL) and R.conv1_input(2, 8, 1, 1, BF).dtype == BF


# ---------------------------------------------------------------------------------------------- every case named for a seam sits on it
def test_cases_sit_on_their_seams():
    assert [R.conv1_tiles(C, T) for C, T in R.CONV1_CASES] == [(1, 1), (1, 1), (2, 1), (2, 2), (3, 2), (4, 3)]
    assert R.CONV1_CASES[1][1] == R.CONV1_TILE_T and R.CONV1_CASES[2][1] == R.CONV1_TILE_T + 1 and R.CONV1_CASES[3][0] % 64 == 8 and R.CONV1_CASES[5][0] == 2 * 64 + 8
    v = R.CONV2_CAP_C // 8
    assert R.past_cap(R.CONV2_CAP_W * R.tout(R.IM2COL2_CAP_TIN) * 3 * v) and not R.past_cap(R.CONV2_CAP_W * (R.tout(R.IM2COL2_CAP_TIN) - 1) * 3 * v)
    assert R.past_cap(R.CONV2_CAP_W * R.COL2IM2_CAP_TIN * v) and not R.past_cap(R.CONV2_CAP_W * (R.COL2IM2_CAP_TIN - 1) * v)
    assert R.IM2COL2_CAP_TIN % 2 == 1 and R.COL2IM2_CAP_TIN % 2 == 1, "odd Tin: the last tap lands on Tin - 1"
    assert [R.past_cap(co * ci * 3) for co, ci in R.WEIGHT_CASES] == [False, False, False, True]
    assert [R.past_cap(r * (c // 8)) for r, c in R.POOL_CASES] == [False, False, True]
    assert [R.scan_chunks(n) for n in R.SCAN_N] == [1, 1, 1, 1, 1, 1, 2, 3, 129]
    assert {63, 64, 65} <= set(R.SCAN_N) and {1023, 1024, 1025} <= set(R.SCAN_N) and R.SCAN_WAVE == 64 and R.SCAN_CHUNK == 1024
    m = R.scan_ids(2049, "wave_seam") == R.AUDIO_ID
    assert m.nonzero().reshape(-1).tolist() == [62, 63, 64, 65]
    m = R.scan_ids(2049, "chunk_seam") == R.AUDIO_ID
    assert m.nonzero().reshape(-1).tolist() == [1022, 1023, 1024, 1025]
    assert not R.past_cap(R.EMBED_BIG_N * (8 // 8)) and R.past_cap(R.EMBED_BIG_N * (64 // 8)) and not R.past_cap(R.EMBED_SMALL_N * (3584 // 8))
    assert [R.transpose_tiles(r, c) for r, c in R.TRANSPOSE_CASES] == [1, 1, 1, 4, 8, 9]
    assert [R.transpose_tiles(r, c, R.pad64(r) + 64) for r, c in R.TRANSPOSE_CASES] == [2, 2, 2, 6, 12, 12]
    assert [R.past_cap(b * n * h * d) for b, n, h, d in R.KV_CASES] == [False, False, False, True]
    assert [R.past_cap(rows * (E // 2)) for rows, E, _ in R.ROTARY_CASES] == [False, False, False, False, True]
    assert [R.past_cap(n) for n in R.CAST_N] == [False, False, True]
    g = [R.logmel_geometry(*c) for c in R.LOGMEL_CASES]
    assert [x.T for x in g] == [3, 33, 64, 200, 1650] and [x.blocks for x in g] == [1, 2, 2, 7, 52] and [x.ragged for x in g] == [True, True, False, True, True]
    assert [x.fstep for x in g] == [2, 2, 2, 4, 2] and [R.past_cap(x.finish_items) for x in g] == [False, False, False, False, True] and g[4].finish_items == 1056000

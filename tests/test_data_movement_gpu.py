"""The kernels of csrc/elementwise.hip that only move data, on an MI355X against tests/_frontend_ref.py, BIT for bit (int16 views: -0 and NaN payloads
count): the conv stem's im2col / col2im / weight permutation / AvgPool, placeholder_scan, the embedding gather / scatter and its row gather / scatter
form, transpose (with the persistent loop ops.THIN_BLOCKS switches on) and transpose_heads, afk_kv_cache_append as decode_forward.py calls it, cast_f32_bf16 -
and rotary_time, the one kernel here that does arithmetic, within its derived bound of the float64 formula.  Every output is NaN before the call;
where the wrapper allocates it, the C entry point is called a second time on a view inside a larger NaN buffer whose guard must stay untouched.
Each family is run at one vector, at its tile / wave / chunk seams and past ew_grid's 1,048,576-item cap (tests/test_frontend_ref_cpu.py asserts that
every case sits where it is named for).

Measured on an MI355X: every data-movement result bit-equal to its reference in all 96 such cases, no guard touched, THIN_BLOCKS = 1 and 3 bit-equal to 0;
rotary_time max error / bound (the module prints them), forward / backward:  1x2 R=2: 0.422 / 0.796   5x128 R=52: 0.991 / 0.999   5x128 R=128: 0.999 / 0.999
16400x128 R=52: 1.000 / 1.000 (of 850 k rotated outputs one is always next to a tie of its one bf16 rounding, which is the bound).
Module wall time 3.5 s for 101 cases; the slowest are the first call (0.8 s, library load), col2im past the cap (0.3 s) and AvgPool past the cap (0.2 s).
"""
import numpy as np
import pytest
import torch

from tests import _frontend_ref as R
from tests import _norm_ref as N

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
NAN = float("nan")
GUARD = 64
WORST = {}


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    print("\n[data movement] rotary_time max error / bound: " + "; ".join(f"{k} {v:.3f}" for k, v in sorted(WORST.items())))


def _ops():
    from audio_flamingo_amd import ops

    return ops


def _call(name, *args):
    from audio_flamingo_amd import _lib

    return _lib.call(name, *args)


def _same(got, ref, what):
    assert tuple(got.shape) == tuple(ref.shape) and got.dtype == ref.dtype, (what, got.shape, ref.shape, got.dtype, ref.dtype)
    g, r = R.bits(got), R.bits(ref)
    if not torch.equal(g, r):
        bad = (g != r).nonzero()
        raise AssertionError(f"{what}: {len(bad)} of {g.numel()} elements differ in their bits; first at {bad[:6].tolist()}")


def _guarded(shape, dev, dtype=BF):
    """(buffer, view): a NaN-filled (int32: -7) buffer with GUARD elements before and after the view the kernel is given"""
    n = int(np.prod(shape))
    fill = -7 if dtype == torch.int32 else NAN
    buf = torch.full((n + 2 * GUARD,), fill, device=dev, dtype=dtype)
    return buf, buf[GUARD: GUARD + n].view(shape)


def _guard_untouched(buf, what):
    b = R.bits(buf)
    fresh = R.bits(torch.full((1,), -7 if buf.dtype == torch.int32 else NAN, dtype=buf.dtype))[0]
    assert bool((b[:GUARD] == fresh).all()) and bool((b[-GUARD:] == fresh).all()), (what, "wrote outside its output")


# ---------------------------------------------------------------------------------------------- conv stem
@pytest.mark.parametrize("dtype", [torch.float32, BF], ids=["f32", "bf16"])
@pytest.mark.parametrize("C,T", R.CONV1_CASES)
def test_im2col_conv1(dev, C, T, dtype):
    ops, W = _ops(), R.CONV1_W
    x = R.conv1_input(W, C, T, 11, dtype)
    ref = R.im2col1(x)
    xd = x.to(dev)
    _same(ops.im2col_conv1(xd), ref, "im2col_conv1")
    buf, col = _guarded((W * T, 3 * C), dev)
    _call("afk_im2col_conv1", xd.data_ptr(), int(dtype == torch.float32), col.data_ptr(), W, C, T, ops._stream())
    _same(col, ref, "afk_im2col_conv1")
    _guard_untouched(buf, "afk_im2col_conv1")


def _conv2(dev, W, Tin, C):
    ops, To = _ops(), R.tout(Tin)
    h = R.gauss((W * Tin, C), 12)
    ref = R.im2col2(h, W, Tin, C)
    hd = h.to(dev)
    _same(ops.im2col_conv2(hd, W, Tin, C), ref, "im2col_conv2")
    buf, col = _guarded((W * To, 3 * C), dev)
    _call("afk_im2col_conv2", hd.data_ptr(), col.data_ptr(), W, Tin, To, C, ops._stream())
    _same(col, ref, "afk_im2col_conv2")
    _guard_untouched(buf, "afk_im2col_conv2")


def _col2im(dev, W, Tin, C):
    ops, To = _ops(), R.tout(Tin)
    for name, dcol in (("gauss", R.gauss((W * To, 3 * C), 13)), ("int", R.int_data((W * To, 3 * C), 14))):
        ref = R.col2im2(dcol, W, Tin, C)
        dd = dcol.to(dev)
        got = ops.col2im_conv2(dd, W, Tin, C)
        _same(got, ref, f"col2im_conv2 {name}")
        buf, dh = _guarded((W * Tin, C), dev)
        _call("afk_col2im_conv2", dd.data_ptr(), dh.data_ptr(), W, Tin, To, C, ops._stream())
        _same(dh, ref, f"afk_col2im_conv2 {name}")
        _guard_untouched(buf, "afk_col2im_conv2")
    # small integers: the exact integer result, through float64 autograd of the definition
    hr = torch.zeros((W * Tin, C), dtype=torch.float64, requires_grad=True)
    R.im2col2(hr, W, Tin, C).backward(dcol.double())
    assert torch.equal(got.cpu().double(), hr.grad) and bool((hr.grad == hr.grad.round()).all()), "col2im on small integers is exact"


@pytest.mark.parametrize("W", R.CONV2_W)
@pytest.mark.parametrize("C", R.CONV2_C)
@pytest.mark.parametrize("Tin", R.CONV2_TIN)
def test_im2col_and_col2im_conv2(dev, Tin, C, W):
    _conv2(dev, W, Tin, C)
    _col2im(dev, W, Tin, C)


def test_im2col_conv2_past_the_grid_cap(dev):
    _conv2(dev, R.CONV2_CAP_W, R.IM2COL2_CAP_TIN, R.CONV2_CAP_C)


def test_col2im_conv2_past_the_grid_cap(dev):
    _col2im(dev, R.CONV2_CAP_W, R.COL2IM2_CAP_TIN, R.CONV2_CAP_C)


@pytest.mark.parametrize("Co,Ci", R.WEIGHT_CASES)
def test_conv_weight_permutation(dev, Co, Ci):
    ops = _ops()
    w, dwp, old = R.gauss((Co, Ci, 3), 15), R.gauss((Co, 3 * Ci), 16), R.gauss((Co, Ci, 3), 17)
    out = torch.full((Co, 3 * Ci), NAN, device=dev, dtype=BF)
    _same(ops.conv_weight_to_gemm(w.to(dev), out=out), R.weight_to_gemm(w), "conv_weight_to_gemm")
    _same(ops.conv_weight_to_gemm(w.to(dev)), R.weight_to_gemm(w), "conv_weight_to_gemm, own output")
    dw = torch.full((Co, Ci, 3), NAN, device=dev, dtype=BF)
    _same(ops.conv_weight_grad_from_gemm(dwp.to(dev), dw), R.weight_grad_from_gemm(dwp, old, False), "conv_weight_grad_from_gemm")
    dw = old.to(dev)
    _same(ops.conv_weight_grad_from_gemm(dwp.to(dev), dw, accumulate=True), R.weight_grad_from_gemm(dwp, old, True), "conv_weight_grad_from_gemm accumulate")
    buf, o = _guarded((Co, Ci, 3), dev)
    dwpd = dwp.to(dev)
    _call("afk_conv_weight_permute", dwpd.data_ptr(), o.data_ptr(), Co, Ci, 1, 0, ops._stream())
    _same(o, R.weight_grad_from_gemm(dwp, old, False), "afk_conv_weight_permute")
    _guard_untouched(buf, "afk_conv_weight_permute")


@pytest.mark.parametrize("out_rows,C", R.POOL_CASES)
def test_avgpool2(dev, out_rows, C):
    ops = _ops()
    x, dy = R.pool_input(out_rows, C, 18), R.gauss((out_rows, C), 19)
    xd, dyd = x.to(dev), dy.to(dev)
    _same(ops.avgpool2_fwd(xd, out_rows, C), R.avgpool2_fwd(x, out_rows, C), "avgpool2_fwd")
    _same(ops.avgpool2_bwd(dyd, out_rows, C), R.avgpool2_bwd(dy, out_rows, C), "avgpool2_bwd")
    buf, y = _guarded((out_rows, C), dev)
    _call("afk_avgpool2_fwd", xd.data_ptr(), y.data_ptr(), out_rows, C, ops._stream())
    _same(y, R.avgpool2_fwd(x, out_rows, C), "afk_avgpool2_fwd")
    _guard_untouched(buf, "afk_avgpool2_fwd")
    buf, dx = _guarded((2 * out_rows, C), dev)
    _call("afk_avgpool2_bwd", dyd.data_ptr(), dx.data_ptr(), out_rows, C, ops._stream())
    _same(dx, R.avgpool2_bwd(dy, out_rows, C), "afk_avgpool2_bwd")
    _guard_untouched(buf, "afk_avgpool2_bwd")


# ---------------------------------------------------------------------------------------------- placeholder scan, embedding
@pytest.mark.parametrize("n", R.SCAN_N)
def test_placeholder_scan(dev, n):
    ops = _ops()
    for pattern in R.SCAN_PATTERNS:
        ids = R.scan_ids(n, pattern)
        ref_src, ref_cnt = R.placeholder_scan(ids, R.AUDIO_ID)
        idd = ids.to(dev)
        src, cnt = ops.placeholder_scan(idd, R.AUDIO_ID)
        assert int(cnt.item()) == ref_cnt, (pattern, int(cnt.item()), ref_cnt)
        _same(src, ref_src, f"placeholder_scan {pattern}")
        buf, s = _guarded((n,), dev, torch.int32)
        cbuf, c = _guarded((1,), dev, torch.int32)
        _call("afk_placeholder_scan", idd.data_ptr(), n, R.AUDIO_ID, s.data_ptr(), c.data_ptr(), ops._stream())
        _same(s, ref_src, f"afk_placeholder_scan {pattern}")
        assert int(c.item()) == ref_cnt
        _guard_untouched(buf, "afk_placeholder_scan src"), _guard_untouched(cbuf, "afk_placeholder_scan count")


def _embed_ids(kind, n, V):
    g = torch.Generator().manual_seed(n + V)
    if kind == "distinct":
        ids = torch.randperm(V, generator=g)
        ids = ids[ids != R.AUDIO_ID][:n]
        assert len(ids) == n == len(torch.unique(ids))
        return ids
    if kind == "one_id":
        return torch.full((n,), 3, dtype=torch.int64)
    assert kind == "mixed"       # ids 0 and V - 1 present; placeholders first, last, interleaved (and scattered at 10 % when the ids are many)
    ids = torch.randint(0, V, (n,), generator=g)
    ids[ids == R.AUDIO_ID] = 0
    ids[1], ids[2] = 0, V - 1
    ids[0] = ids[n - 1] = R.AUDIO_ID
    ids[5:20:2] = R.AUDIO_ID
    if n > 1000:
        ids[20:][torch.rand(n - 20, generator=g) < 0.1] = R.AUDIO_ID
    return ids


EMBED_CASES = [("mixed", R.EMBED_SMALL_N, H, 50, "gauss") for H in R.EMBED_H] + \
              [("distinct", R.EMBED_SMALL_N, 8, 64, "gauss"), ("distinct", R.EMBED_SMALL_N, 64, 64, "gauss"),
               ("one_id", R.EMBED_ONE_ID_N, 8, 50, "int"), ("one_id", R.EMBED_ONE_ID_N, 8, 50, "gauss"),
               ("mixed", R.EMBED_BIG_N, 8, 1000, "gauss"), ("mixed", R.EMBED_BIG_N, 64, 1000, "gauss")]


@pytest.mark.parametrize("kind,n,H,V,data", EMBED_CASES, ids=[f"{k}-n{n}-H{h}-{d}" for k, n, h, _, d in EMBED_CASES])
def test_embed_scatter(dev, kind, n, H, V, data):
    ops = _ops()
    ids = _embed_ids(kind, n, V)
    src, cnt = R.placeholder_scan(ids, R.AUDIO_ID)
    assert (cnt > 0) == (kind == "mixed")
    embed, audio = R.gauss((V, H), 21), R.gauss((max(cnt, 1), H), 22)
    idd, srcd, embd, audd = ids.to(dev), src.to(dev), embed.to(dev), audio.to(dev)
    ref = R.embed_scatter_fwd(ids, src, embed, audio)
    _same(ops.embed_scatter_fwd(idd, srcd, embd, audd), ref, "embed_scatter_fwd")
    buf, out = _guarded((n, H), dev)
    _call("afk_embed_scatter_fwd", idd.data_ptr(), srcd.data_ptr(), embd.data_ptr(), audd.data_ptr(), out.data_ptr(), n, H, ops._stream())
    _same(out, ref, "afk_embed_scatter_fwd")
    _guard_untouched(buf, "afk_embed_scatter_fwd")
    # backward: onto a gaussian old d_embed; d_audio NaN before
    dout = R.int_data((n, H), 23) if data == "int" else R.gauss((n, H), 23)
    old = R.gauss((V, H), 24)
    ref_de, ref_da = R.embed_scatter_bwd(ids, src, dout, old, max(cnt, 1))
    if data == "int":       # exact in any order: the reference is also the plain index_add_
        text = src < 0
        exact = old.double().index_add_(0, ids[text], dout[text].double())
        assert torch.equal(ref_de.double(), N.rb(exact))
    never = torch.ones(V, dtype=torch.bool)
    never[ids[src < 0]] = False
    assert bool(never.any()), "some rows of d_embed must belong to ids that never occur"
    doutd = dout.to(dev)
    first = None
    for rep in range(3):
        de, da = old.to(dev), torch.full((max(cnt, 1), H), NAN, device=dev, dtype=BF)
        ops.embed_scatter_bwd(idd, srcd, doutd, de, da)
        _same(de, ref_de, "embed_scatter_bwd d_embed")
        _same(de[never.to(dev)], old[never], "rows of ids that never occur")
        if cnt:
            _same(da, ref_da, "embed_scatter_bwd d_audio")
        first = de if first is None else first
        _same(de, first, "embed_scatter_bwd is not bit-deterministic")
    de = old.to(dev)
    ops.embed_scatter_bwd(idd, srcd, doutd, de, None)
    _same(de, ref_de, "embed_scatter_bwd d_audio=None")
    if cnt:
        buf, da = _guarded((cnt, H), dev)
        ops.embed_scatter_bwd(idd, srcd, doutd, None, da)
        _same(da, ref_da, "embed_scatter_bwd d_embed=None")
        _guard_untouched(buf, "embed_scatter_bwd d_audio")


@pytest.mark.parametrize("which", ["one", "all", "every_other"])
def test_gather_and_scatter_rows(dev, which):
    ops = _ops()
    M, H = 70, 64
    x = R.gauss((M, H), 25)
    rows = {"one": torch.tensor([5]), "all": torch.arange(M), "every_other": torch.arange(0, M, 2)}[which]
    xs = ops.gather_rows(x.to(dev), rows.to(dev))
    _same(xs, R.gather_rows(x, rows), "gather_rows")
    _same(ops.scatter_rows(xs, rows.to(dev), M), R.scatter_rows(x[rows], rows, M), "scatter_rows")


# ---------------------------------------------------------------------------------------------- transposes
@pytest.mark.parametrize("wide", [False, True], ids=["rpad_default", "rpad_plus_64"])
@pytest.mark.parametrize("Rr,C", R.TRANSPOSE_CASES)
def test_transpose(dev, monkeypatch, Rr, C, wide):
    ops = _ops()
    rpad = R.pad64(Rr) + 64 if wide else None
    rp = R.pad64(Rr) if rpad is None else rpad
    xb = R.gauss((Rr, C + 24), 26)
    x = xb[:, 8: 8 + C]                                   # a column-offset view of a wider buffer
    ref = R.transpose(x, rpad)
    xd = xb.to(dev)[:, 8: 8 + C]
    assert xd.stride(0) == C + 24 and xd.storage_offset() == 8 and (Rr == 1 or not xd.is_contiguous())

    def run():
        ob = torch.full((C, rp + 16), NAN, device=dev, dtype=BF)
        out = ob[:, 8: 8 + rp]                            # the output is a view of a wider buffer too
        ops.transpose(xd, out, rpad=rpad)
        assert bool(torch.isnan(ob[:, :8].float()).all()) and bool(torch.isnan(ob[:, 8 + rp:].float()).all()), "transpose wrote outside its output columns"
        return out

    monkeypatch.setattr(ops, "THIN_BLOCKS", 0)
    plain = run()
    _same(plain, ref, "transpose")
    _same(ops.transpose(xd, rpad=rpad), ref, "transpose, own output")
    if R.transpose_tiles(Rr, C, rpad) > 3:
        for thin in (1, 3):                               # the persistent loop functional.py switches on beside every dgrad GEMM
            monkeypatch.setattr(ops, "THIN_BLOCKS", thin)
            _same(run(), plain, f"transpose THIN_BLOCKS={thin}")


@pytest.mark.parametrize("B,S,H,D,spad", R.HEADS_CASES)
def test_transpose_heads(dev, B, S, H, D, spad):
    ops = _ops()
    ld = H * D + 64
    x = R.gauss((B * S, ld), 27)
    out = torch.full((B, H, D, spad), NAN, device=dev, dtype=BF)
    _same(ops.transpose_heads(x.to(dev), B, S, H, D, ld, spad, out=out), R.transpose_heads(x, B, S, H, D, spad), "transpose_heads")
    _same(ops.transpose_heads(x.to(dev), B, S, H, D, ld, spad), R.transpose_heads(x, B, S, H, D, spad), "transpose_heads, own output")


# ---------------------------------------------------------------------------------------------- rotary_time
@pytest.mark.parametrize("rows,E,Rr", R.ROTARY_CASES)
def test_rotary_time(dev, rows, E, Rr):
    ops = _ops()
    x, dy = R.gauss((rows, E), 28), R.gauss((rows, E), 29)
    ang = R.gauss((rows, max(Rr, 1)), 30, 3.0, torch.float32)[:, :Rr]
    cos, sin = ang.cos().contiguous(), ang.sin().contiguous()
    cosd, sind = cos.to(dev), sin.to(dev)
    for backward, t in ((False, x), (True, dy)):
        ref, bound = R.rotary_time_ref(t, cos, sin, backward)
        td = t.to(dev)
        if Rr:
            y = ops.rotary_time(td, cosd, sind, backward=backward)
        else:
            # nothing to rotate: the tables are never read - one NaN each, and the output is the input
            table = torch.full((1,), NAN, device=dev, dtype=torch.float32)
            y = torch.full_like(td, NAN)
            _call("afk_rotary_time", td.data_ptr(), table.data_ptr(), table.data_ptr(), y.data_ptr(), rows, E, 0, int(backward), ops._stream())
        _same(y[:, Rr:], t[:, Rr:], "rotary_time: the columns past R")
        if Rr:
            yc = y.cpu()
            assert bool(torch.isfinite(yc.float()).all())
            r = N.ratio(yc[:, :Rr], ref[:, :Rr], bound[:, :Rr])
            key = f"{'bwd' if backward else 'fwd'} {rows}x{E}/{Rr}"
            WORST[key] = r
            print(f"rotary_time {key}: {r:.3f} of the bound")
            assert r <= 1.0, (key, r)
            buf, yg = _guarded((rows, E), dev)
            _call("afk_rotary_time", td.data_ptr(), cosd.data_ptr(), sind.data_ptr(), yg.data_ptr(), rows, E, Rr, int(backward), ops._stream())
            _same(yg, y, "afk_rotary_time")
            _guard_untouched(buf, "afk_rotary_time")


# ---------------------------------------------------------------------------------------------- KV-cache append
@pytest.mark.parametrize("from_device", [False, True], ids=["start_host", "start_dev"])
@pytest.mark.parametrize("start", R.KV_STARTS)
@pytest.mark.parametrize("B,n,Hkv,D", R.KV_CASES)
def test_kv_cache_append(dev, B, n, Hkv, D, start, from_device):
    """as decode_forward.py calls it: k_col0 = Hq D into a row wider than q | k | v, caches longer than start + n with Spad != Smax.  With start_dev given,
    start_host holds another (in-bounds) value: the device value must win"""
    ops = _ops()
    Hq, nk = 2 * Hkv, Hkv * D
    ld = (Hq + 2 * Hkv) * D + 64
    Smax, Spad = start + n + 3, R.pad64(start + n) + 64
    assert Spad != Smax and start + 2 + n <= min(Smax, Spad)
    qkv = R.gauss((B * n, ld), 31)
    Kc, Vt = torch.full((B, Smax, nk), NAN, dtype=BF), torch.full((B, Hkv, D, Spad), NAN, dtype=BF)
    ref_k, ref_v = R.kv_append(Kc, Vt, qkv, Hq * D, start, B, n, Hkv, D)
    qd = qkv.to(dev)
    kbuf, Kd = _guarded((B, Smax, nk), dev)
    vbuf, Vd = _guarded((B, Hkv, D, Spad), dev)
    start_dev = torch.tensor([start], device=dev, dtype=torch.int32) if from_device else None
    start_host = start + 2 if from_device else start
    _call("afk_kv_cache_append", qd.data_ptr(), qd.stride(0), Hq * D, Kd.data_ptr(), Smax * nk, Vd.data_ptr(), Hkv * D * Spad, Spad, ops._p(start_dev), start_host,
          B, n, Hkv, D, ops._stream())
    _same(Kd, ref_k, "K cache (row-major)")
    _same(Vd, ref_v, "V cache (transposed)")
    _guard_untouched(kbuf, "K cache"), _guard_untouched(vbuf, "V cache")


# ---------------------------------------------------------------------------------------------- fp32 -> bf16
@pytest.mark.parametrize("n", R.CAST_N)
def test_cast_f32_bf16(dev, n):
    ops = _ops()
    x = R.cast_input(n)
    ref = x.to(BF)
    xd = x.to(dev)
    buf, o = _guarded((n,), dev)
    _call("afk_cast_f32_bf16", xd.data_ptr(), o.data_ptr(), n, ops._stream())
    _guard_untouched(buf, "afk_cast_f32_bf16")
    for got in (ops.cast_f32_bf16(xd).cpu(), o.cpu()):
        nan = torch.isnan(ref.float())
        assert torch.equal(torch.isnan(got.float()), nan), "NaN stays NaN, and nothing else becomes one"
        _same(got[~nan], ref[~nan], "cast_f32_bf16")

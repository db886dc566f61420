"""GPU: afk_decode_cfg (csrc/decode_cfg.hip) against the fp64 restatement of tests/_cfg_ref.py.

Bar on the finite entries: 8 * (2|s| + 1) * 2^-23 * (2M + ln V), M the largest finite |z| of the pair of rows.  Derived, not measured: one fp32 rounding each in
z - max, in - log(sum), in c - u, in the product and in the final add, each at most half an ulp of a magnitude <= 2M + ln V; the relative error of the sum of
exponentials enters log as an absolute error below one such ulp; the factor 8 covers the count with room for a 2-ulp expf / logf.  A kernel that needs more has
used a fast intrinsic it should not use.  Entries whose exact value is +inf, -inf or NaN must have that class exactly.

Shapes: V = 1 (a row is its own maximum), 63 / 64 (below and at one wave), 1000 / 1025 (inside one 2 048-column chunk, word tail), 4099 (three chunks, the last
one three columns wide), 152 064 (the AF3 vocabulary: 75 chunks); B = 1, 3, 8.  Every buffer has a leading dimension above V that puts rows off the 16-byte
boundary (word loads and stores) and NaN in the unused columns; the contiguous case takes the 16-byte form."""
import numpy as np
import pytest
import torch

from tests import _cfg_ref as R

pytestmark = pytest.mark.gpu

SCALES = (0.5, 1.5, 3.0, 0.0, -1.0)
NINF = float("-inf")
PAD_BITS = 0x7FC00ABC   # the NaN the unused columns hold


def bits(x):
    return x.contiguous().view(torch.int32)


def _pair(B, V, seed):
    """cond, uncond [B, V] fp32 on the host, |z| <= 30, with the special entries planted where the shape has room for them"""
    g = torch.Generator().manual_seed(seed)
    zc, zu = (torch.randn((B, V), generator=g) * 10).clamp(-30, 30), (torch.randn((B, V), generator=g) * 10).clamp(-30, 30)
    if V >= 8:
        zc[0, 1], zu[0, 2] = NINF, NINF          # -inf in one branch
        zc[0, 3], zu[0, 3] = NINF, NINF          # ... in both
        zc[0, 4] = float("nan")                  # a NaN logit counts as -inf
        zc[0, V - 1] = 30.0
    if B >= 3:
        zc[1, :] = NINF                          # a row with nothing above -inf: NaN everywhere
        zu[2, V // 2] = float("inf")             # a +inf: NaN everywhere as well (inf - inf in the row's own log_softmax)
    if B >= 8 and V >= 8:
        zu[5, :] = NINF
        zu[5, 6] = -3.0                          # one survivor: u = 0 there, -inf elsewhere
    return zc, zu


def _strided(x, dev, ld):
    """x [B, V] inside a NaN-filled buffer of row pitch ld on the device -> (the [B, V] view, the whole buffer)"""
    B, V = x.shape
    buf = torch.full((B, ld), PAD_BITS, dtype=torch.int32).view(torch.float32).clone()
    buf[:, :V] = x
    buf = buf.to(dev)
    return buf[:, :V], buf


def _odd_ld(V, extra):
    ld = V + extra
    return ld if ld % 4 else ld + 1


def _check(got, zc, zu, s, what):
    want = R.guided(zc.numpy(), zu.numpy(), s)
    got = got.cpu().numpy()
    B, V = want.shape
    worst = 0.0
    for b in range(B):
        fin = R.same_class(got[b], want[b])
        if fin.any():
            bar = R.bar(s, R.finite_absmax(zc[b].numpy(), zu[b].numpy()), V)
            err = float(np.abs(got[b][fin] - want[b][fin]).max())
            worst = max(worst, err / bar)
            assert err <= bar, (what, s, b, err, bar)
    return worst


@pytest.mark.parametrize("B", [1, 3, 8])
@pytest.mark.parametrize("V", [1, 63, 64, 1000, 1025, 4099])
def test_kernel_against_the_restatement(dev, V, B):
    from audio_flamingo_amd import ops

    zc, zu = _pair(B, V, 1000 * V + B)
    worst = 0.0
    for i, s in enumerate(SCALES):
        # separate out, every row off the 16-byte boundary in its own way, NaN in the unused columns of all three buffers
        c, cbuf = _strided(zc, dev, _odd_ld(V, 1))
        u, ubuf = _strided(zu, dev, _odd_ld(V, 2))
        o, obuf = _strided(torch.zeros((B, V)), dev, _odd_ld(V, 5))
        c0, u0, o0 = cbuf.clone(), ubuf.clone(), obuf.clone()
        assert ops.decode_cfg(c, u, s, out=o) is o
        worst = max(worst, _check(o, zc, zu, s, "separate"))
        assert torch.equal(bits(cbuf), bits(c0)) and torch.equal(bits(ubuf), bits(u0)), "an input was written"
        assert torch.equal(bits(obuf[:, V:]), bits(o0[:, V:])), "a column >= V of out was written"
        # in place on cond; the same bits as the separate form, and the unused columns untouched
        assert ops.decode_cfg(c, u, s, out=c) is c
        assert torch.equal(bits(c), bits(o)), (s, "the aliased form differs from the separate one")
        assert torch.equal(bits(cbuf[:, V:]), bits(c0[:, V:])) and torch.equal(bits(ubuf), bits(u0))
        if i == 0:   # contiguous rows (16-byte loads and stores where V allows): the same values in the same threads, so the same bits
            fresh = ops.decode_cfg(zc.to(dev), zu.to(dev), s)
            assert fresh.shape == (B, V) and torch.equal(bits(fresh), bits(o))
    print(f"decode_cfg V={V} B={B}: worst error / bar {worst:.3f}")


def test_kernel_at_the_af3_vocabulary_twice_and_from_a_graph(dev):
    from audio_flamingo_amd import ops

    B, V, s = 2, 152064, 3.0
    zc, zu = _pair(B, V, 7)
    c, u = zc.to(dev), zu.to(dev)
    ws = ops.decode_cfg_workspace(B, V, dev)
    first = ops.decode_cfg(c, u, s, ws=ws)
    print(f"decode_cfg V={V}: worst error / bar {_check(first, zc, zu, s, 'af3'):.3f}")
    again = ops.decode_cfg(c, u, s, ws=ws)
    assert torch.equal(bits(first), bits(again)), "two launches, two results"
    out = torch.zeros_like(first)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ops.decode_cfg(c, u, s, out=out, ws=ws)
    out.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(bits(out), bits(first)), "the replayed launch differs from the eager one"
    inplace = c.clone()                                   # the decode step's form: in place on the conditional rows of one [2B, V] buffer
    both = torch.cat([inplace, u])
    ops.decode_cfg(both[:B], both[B:], s, out=both[:B], ws=ws)
    assert torch.equal(bits(both[:B]), bits(first)) and torch.equal(bits(both[B:]), bits(u))


def test_refusals(dev):
    from audio_flamingo_amd import _lib, ops
    from audio_flamingo_amd._lib import AfkError

    B, V = 2, 40
    c, u, o = torch.zeros((B, V), device=dev), torch.zeros((B, V), device=dev), torch.zeros((B, V), device=dev)
    ws = ops.decode_cfg_workspace(B, V, dev)
    assert ws.numel() == _lib.load().afk_decode_cfg_workspace_floats(B, V) == B * 4
    st = torch.cuda.current_stream().cuda_stream
    ok = [c.data_ptr(), V, u.data_ptr(), V, 2.0, o.data_ptr(), V, B, V, ws.data_ptr(), ws.numel(), st]
    _lib.call("afk_decode_cfg", *ok)
    for idx, val, word in ((0, None, "null pointer"), (2, None, "null pointer"), (5, None, "null pointer"), (9, None, "null pointer"), (7, 0, "B = 0"),
                           (8, 0, "V = 0"), (8, -1, "V = -1"), (1, V - 1, "leading dimension below V"), (3, V - 1, "leading dimension below V"),
                           (6, V - 1, "leading dimension below V"), (10, ws.numel() - 1, "workspace")):
        bad = list(ok)
        bad[idx] = val
        with pytest.raises(AfkError, match=word):
            _lib.call("afk_decode_cfg", *bad)
    for kw in (dict(cond=c.double()), dict(uncond=u.cpu()), dict(out=o[:, :39]), dict(uncond=u[:1]), dict(out=u), dict(cond=c.t().contiguous().t()),
               dict(ws=ws[:1]), dict(ws=ws.double())):
        args = dict(dict(cond=c, uncond=u, out=o, ws=ws), **kw)
        with pytest.raises(AfkError):
            ops.decode_cfg(args["cond"], args["uncond"], 2.0, out=args["out"], ws=args["ws"])
    shared = torch.zeros((3, V), device=dev)
    with pytest.raises(AfkError, match="overlap"):
        ops.decode_cfg(shared[:2], u, 2.0, out=shared[1:])      # out overlaps cond without being cond
    with pytest.raises(AfkError, match="overlap"):
        ops.decode_cfg(c, shared[:2], 2.0, out=shared[1:])      # out overlaps uncond

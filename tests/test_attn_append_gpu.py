"""GPU: the append attention (afk_attn_append, csrc/attention_append.hip) - n new query rows per sample against a KV cache, split-KV in two launches -
against the fp64 reference and the bars of tests/_attn_probe.py (||got - ref||_2 <= 2^-6 ||ref||_2 + 2^-8 sqrt(D) on every probed slice; the bar's
justification is _attn_probe.bar's: one bf16 rounding of P and one of O), and against the interval kernel it replaces (afk_xattn_fwd).

  staircase  the causal-with-past shape of a chat turn: a planted causal case over S = past + n positions (_attn_probe.training_case: the diagonal, both range
             ends, the 64 / 128 tile edges and the neighbouring sample's first key carry planted keys), of which the LAST n rows are the queries; two samples
             with different left padding; every (row, head) of the suffix is a probed slice.  Q rows are views inside a fused q|k|v buffer, the cache has
             more slots than keys, and every slot behind the keys - and every pad column of V^T - holds NaN.
  intervals  arbitrary per-row intervals with empty rows (_attn_probe.interval_case at the INTERVAL_LAYOUTS shapes)."""
import pytest
import torch

import _attn_probe as P

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
NAN = float("nan")

# (n, past, Hq, Hkv, D, nsplit): every n, past, head pair, head size and split count of the issue appears; (33, 1000, 28:4, 128) is the flagship turn;
# (31, 0, ..., 8) and (32, 7, ..., 8): splits that are empty for the early rows
STAIRS = [(1, 64, 4, 4, 64, 1), (2, 64, 4, 2, 128, 3), (31, 0, 16, 2, 64, 8), (32, 7, 28, 4, 64, 8), (33, 1000, 28, 4, 128, 3), (33, 1000, 28, 4, 128, 8),
          (65, 7, 4, 4, 128, 1), (65, 1000, 16, 2, 128, 8), (32, 1000, 4, 2, 64, 1)]
_STAIR = {}


def _mods():
    from audio_flamingo_amd import _lib, ops

    return ops, _lib


def _canon(o, B, n, Hq, D):
    return o[:, : Hq * D].reshape(B, n, Hq, D).transpose(1, 2)


def _lo(past, n):
    return [0, min(3, max(past + n - 2, 0))]


def _stair(dev, n, past, Hq, Hkv, D):
    """the planted staircase case, built and referenced ONCE per shape: (case, fused qkv rows of the suffix [B*n, (Hq+2Hkv)*D], k, v canonical over S keys,
    krange [B, n, 2], the fp64 reference of the suffix rows [B, Hq, n, D], the slots)"""
    key = (n, past, Hq, Hkv, D)
    if key not in _STAIR:
        B, S = 2, past + n
        lo = _lo(past, n)
        case, qkv, _ = P.training_case(B, S, Hq, Hkv, D, True, kv_lo=lo, seed=S + D + Hq, device=dev)
        suffix = list(range(past, S))
        ref = P.attend(case.q, case.k, case.v, case.vis, case.hmap, case.scale, rows=suffix)
        rows = qkv.reshape(B, S, -1)[:, past:].reshape(B * n, -1).contiguous()
        ar = torch.arange(past, S, device=dev, dtype=torch.int32)
        lo_t = torch.tensor(lo, device=dev, dtype=torch.int32)
        kr = torch.stack([lo_t[:, None].expand(B, n), torch.maximum(ar[None, :] + 1, lo_t[:, None])], -1).contiguous()
        slots = [(b, h, i) for b in range(B) for h in range(Hq) for i in range(n)]
        _STAIR[key] = (case, rows, case.k, case.v, kr, ref, slots)
    return _STAIR[key]


def _cache(k, v, slack, fill):
    """canonical k, v [B, Hkv, Sk, D] -> K cache [B, Sk + slack, Hkv*D], V^T cache [B, Hkv, D, pad64(Sk + slack)]; everything that is not a key = fill"""
    ops, _ = _mods()
    B, Hkv, Sk, D = k.shape
    Smax = Sk + slack
    kc = torch.full((B, Smax, Hkv * D), fill, device=k.device, dtype=BF)
    kc[:, :Sk] = k.transpose(1, 2).reshape(B, Sk, Hkv * D)
    vt = torch.full((B, Hkv, D, ops.pad64(Smax)), fill, device=k.device, dtype=BF)
    vt[..., :Sk] = v.transpose(-1, -2)
    return kc, vt


def _append(q, kc, vt, kr, B, n, Hq, Hkv, D, ns):
    ops, _ = _mods()
    o = ops.attn_append(q, kc, vt, kr, B, n, Hq, Hkv, D, D ** -0.5, nsplit=ns)
    torch.cuda.synchronize()
    return o


def _xattn(q, kc, vt, kr, B, n, Hq, Hkv, D, Sk):
    """the launch of decode_forward._decode_layers' last branch"""
    ops, lib = _mods()
    nq, nk = Hq * D, Hkv * D
    Smax, spad = kc.shape[1], vt.shape[3]
    o = torch.full((B * n, nq), 7.0, device=q.device, dtype=BF)
    lse = torch.empty((B, Hq, n), device=q.device, dtype=torch.float32)
    lib.call("afk_xattn_fwd", q.data_ptr(), n * q.stride(0), D, q.stride(0), kc.data_ptr(), Smax * nk, D, nk, vt.data_ptr(), o.data_ptr(), n * nq, D, nq,
             lse.data_ptr(), 0, kr.data_ptr(), B, Hq, Hkv, n, Sk, ops.pad64(n), spad, D, float(D ** -0.5), ops._stream())
    torch.cuda.synchronize()
    return o


@pytest.mark.parametrize("n,past,Hq,Hkv,D,ns", STAIRS, ids=lambda x: str(x))
def test_staircase_against_fp64(dev, n, past, Hq, Hkv, D, ns):
    """a turn of n rows behind `past` cached positions, Q inside the fused projection, a cache pitch beyond the keys, NaN in every unused slot"""
    case, rows, k, v, kr, ref, slots = _stair(dev, n, past, Hq, Hkv, D)
    kc, vt = _cache(k, v, 37, NAN)
    assert torch.isnan(kc[:, k.shape[2]:].float()).all() and torch.isnan(vt[..., k.shape[2]:].float()).all()
    q = rows[:, : Hq * D]
    assert not q.is_contiguous()
    o = _append(q, kc, vt, kr, 2, n, Hq, Hkv, D, ns)
    worst = P.check(f"append staircase n={n} past={past} {Hq}:{Hkv} D={D} ns={ns}", _canon(o, 2, n, Hq, D), ref, slots, D)
    print(f"staircase n={n} past={past} {Hq}:{Hkv} D={D} ns={ns}: worst slice at {worst:.3f} x the bar")
    # left-padded rows in front of the sample's first real position see nothing: exact zeros
    empty = (kr[..., 1] <= kr[..., 0])
    for b, i in empty.nonzero().tolist():
        assert (_canon(o, 2, n, Hq, D)[b, :, i] == 0).all()


@pytest.mark.parametrize("layout", P.INTERVAL_LAYOUTS, ids=lambda l: f"B{l[0]}-Sq{l[1]}-Sk{l[2]}-H{l[3]}:{l[4]}-D{l[5]}")
@pytest.mark.parametrize("ns", [1, 3, 8])
def test_arbitrary_intervals_against_fp64_and_the_interval_kernel(dev, layout, ns):
    """any per-row interval, empty ones included: within the bar of fp64 - and so is afk_xattn_fwd on the same inputs; rows with an empty interval carry
    the interval kernel's bits"""
    ops, _ = _mods()
    B, Sq, Sk, Hq, Hkv, D, _, slack = layout
    assert ops.attn_append_supported(Hq, Hkv, D), "every INTERVAL_LAYOUTS geometry is one the kernel takes"
    case, q, k, v, kr, _ = P.interval_case(B, Sq, Sk, Hq, Hkv, D, seed=Sq + Sk, device=dev)
    qbuf = torch.full((B * Sq, Hq * D + 2 * Hkv * D + slack), NAN, device=dev, dtype=BF)
    qbuf[:, : Hq * D] = q.transpose(1, 2).reshape(B * Sq, Hq * D)
    qv = qbuf[:, : Hq * D]
    tag = f"append interval {layout} ns={ns}"
    kc, vt = _cache(k, v, slack + 5, NAN)
    o = _append(qv, kc, vt, kr, B, Sq, Hq, Hkv, D, ns)
    P.check(tag, _canon(o, B, Sq, Hq, D), case.ref(), case.rows, D)
    # the kernel it replaces, on the same inputs with a zero-filled cache (it multiplies 0 x the pad columns)
    kc0, vt0 = _cache(k, v, slack + 5, 0.0)
    o0 = _append(qv, kc0, vt0, kr, B, Sq, Hq, Hkv, D, ns)
    assert torch.equal(o0, o), f"{tag}: the unused cache slots reached the output"
    ox = _xattn(qv, kc0, vt0, kr, B, Sq, Hq, Hkv, D, Sk)
    P.check(f"{tag} (afk_xattn_fwd)", _canon(ox, B, Sq, Hq, D), case.ref(), case.rows, D)
    empty = case.info["empty"]
    assert int(empty.sum()) >= B
    oc, oxc = _canon(o, B, Sq, Hq, D), _canon(ox, B, Sq, Hq, D)
    for b, i in empty.nonzero().tolist():
        assert torch.equal(oc[b, :, i].view(torch.int16), oxc[b, :, i].view(torch.int16)), f"{tag}: empty row ({b}, {i}) differs from afk_xattn_fwd bit for bit"
        assert (oc[b, :, i].view(torch.int16) == 0).all()


def test_staircase_against_the_kernel_it_replaces(dev):
    n, past, Hq, Hkv, D = 33, 1000, 28, 4, 128
    case, rows, k, v, kr, ref, slots = _stair(dev, n, past, Hq, Hkv, D)
    kc, vt = _cache(k, v, 37, 0.0)
    q = rows[:, : Hq * D]
    o = _append(q, kc, vt, kr, 2, n, Hq, Hkv, D, 8)
    ox = _xattn(q, kc, vt, kr, 2, n, Hq, Hkv, D, past + n)
    P.check("append", _canon(o, 2, n, Hq, D), ref, slots, D)
    P.check("afk_xattn_fwd", _canon(ox, 2, n, Hq, D), ref, slots, D)


def test_same_bits_every_launch_and_split_counts_agree(dev):
    n, past, Hq, Hkv, D = 33, 1000, 28, 4, 128
    case, rows, k, v, kr, ref, slots = _stair(dev, n, past, Hq, Hkv, D)
    kc, vt = _cache(k, v, 37, NAN)
    q = rows[:, : Hq * D]
    outs = {}
    for ns in (1, 8):
        a = _append(q, kc, vt, kr, 2, n, Hq, Hkv, D, ns)
        b = _append(q, kc, vt, kr, 2, n, Hq, Hkv, D, ns)
        assert torch.equal(a.view(torch.int16), b.view(torch.int16)), f"nsplit {ns}: two launches differ"
        P.check(f"nsplit {ns}", _canon(a, 2, n, Hq, D), ref, slots, D)
        outs[ns] = a
    # nsplit 1 against nsplit 8: the same inputs, another merge order and one bf16 rounding of O - within the bar of each other
    worst = P.check("nsplit 1 against nsplit 8", _canon(outs[1], 2, n, Hq, D), _canon(outs[8], 2, n, Hq, D).double(), slots, D)
    print(f"nsplit 1 against nsplit 8: worst slice at {worst:.3f} x the bar")


def test_negative_control_a_staircase_shifted_by_one_key(dev):
    """the probe can tell: the fp64 reference of the staircase that ends one key early lies >= SEP x the bar from the truth on some suffix slice, and the
    kernel given that staircase (only ever shrunk: every read stays in bounds) fails the bar"""
    n, past, Hq, Hkv, D = 33, 1000, 28, 4, 128
    case, rows, k, v, kr, ref, slots = _stair(dev, n, past, Hq, Hkv, D)
    suffix = list(range(past, past + n))
    vis, hmap = case.mutations["diag-1"]
    shifted = P.attend(case.q, case.k, case.v, vis, hmap, case.scale, rows=suffix)
    sep = P.slice_errors(shifted, ref, slots, D)[0][0]
    assert sep >= P.SEP, f"the shifted staircase moves the worst slice by {sep:.2f} x its bar only"
    kr2 = kr.clone()
    kr2[..., 1] -= (kr2[..., 1] > kr2[..., 0]).int()
    kc, vt = _cache(k, v, 37, NAN)
    o = _append(rows[:, : Hq * D], kc, vt, kr2, 2, n, Hq, Hkv, D, 3)
    worst = P.slice_errors(_canon(o, 2, n, Hq, D), ref, slots, D)[0]
    assert worst[0] > 1.0, f"the kernel given a staircase shifted by one key passed the bar (worst slice at {worst[0]:.2f} x)"


def test_contract_refusals(dev):
    ops, lib = _mods()
    B, n, Hq, Hkv, D, Sk = 1, 4, 4, 2, 64, 64
    q = torch.zeros((B * n, Hq * D), device=dev, dtype=BF)
    kc = torch.zeros((B, Sk, Hkv * D), device=dev, dtype=BF)
    vt = torch.zeros((B, Hkv, D, 64), device=dev, dtype=BF)
    kr = torch.zeros((B, n, 2), device=dev, dtype=torch.int32)
    o = torch.zeros((B * n, Hq * D), device=dev, dtype=BF)
    ws = torch.zeros(int(lib.load().afk_attn_append_workspace_floats(B, Hq, n, D, 8)), device=dev, dtype=torch.float32)
    assert ws.numel() == B * Hq * n * 8 * (D + 4)

    def call(q=q, kr=kr, Hq=Hq, Hkv=Hkv, D=D, ns=2, ws_floats=None, ws=ws):
        lib.call("afk_attn_append", q.data_ptr() if q is not None else 0, n * Hq * D, D, Hq * D, kc.data_ptr(), Sk * Hkv * D, Hkv * D, D, vt.data_ptr(),
                 Hkv * D * 64, 64, o.data_ptr(), n * Hq * D, D, Hq * D, kr.data_ptr() if kr is not None else 0, B, Hq, Hkv, n, D, float(D ** -0.5), ns,
                 ws.data_ptr() if ws is not None else 0, ws.numel() if ws_floats is None else ws_floats, ops._stream())

    call()   # the accepted form
    torch.cuda.synchronize()
    for kw in (dict(q=None), dict(kr=None), dict(ws=None, ws_floats=1 << 20), dict(D=32), dict(D=256), dict(Hq=6, Hkv=2), dict(Hq=5, Hkv=2), dict(ns=0),
               dict(ns=65), dict(ns=8, ws_floats=ws.numel() - 1), dict(ns=2, ws_floats=0)):
        with pytest.raises(lib.AfkError, match="afk_attn_append"):
            call(**kw)
    torch.cuda.synchronize()

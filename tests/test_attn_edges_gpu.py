"""GPU: the attention kernels' masks, key ranges and decode splits at their edges, against the planted-key probes of tests/_attn_probe.py.

Every probed slice - an output / dQ row of a (sample, query head), a dK / dV row of a planted key - must satisfy ||got - ref||_2 <= 2^-6 ||ref||_2 +
2^-8 sqrt(D) against the fp64 reference computed from the bf16 inputs (_attn_probe.bar: bf16 rounding of P and O costs at most about 2^-8; the floor
is one half-ulp per element at unit scale).  The backward reference takes delta = rowsum(dO o O) from the bf16 O the backward kernels are given, as they
do (_attn_probe.attend).  tests/test_attn_probe_cpu.py shows that every one-key mistake - a range end or the causal diagonal moved by one, a tile-edge or
chunk-edge key dropped, the wrong KV head, the neighbouring sample's first key - lands >= 8x this bar away, and the negative controls below show it on
the kernels themselves.  The whole-tensor comparisons of tests/test_ops_gpu.py stay as they are.

  A  training attention (ops.attn_fwd / attn_bwd): S in {63, 64, 65, 127, 128, 129, 1000, 1024, 1089}, head_dim 64 / 128, causal or not, right padding
     (kv_len), left padding (kv_lo), GQA groups 1 / 2 / 7 - under every schedule knob of tests/test_ops_gpu.py: instruction schedule x XCD block map,
     the persistent forward and its paired form, the dK/dV part counts, the separate delta pass, the rotary backward fused or not (against the rotated
     fp64 reference).  Padded keys get exact-zero dK / dV, left-padded rows exact-zero O / dQ.
  B  interval / cross attention (ops.xattn_* / attn_interval_*): per-query key intervals, empty ones (exact-zero rows), Sq != Sk, GQA, row-strided views.
  C  decode attention (afk_attn_decode, afk_attn_decode_fused in every afk_attn_decode_set_group form): nsplit 1, 2, 3, 8, 13 and the largest each entry
     takes; ragged [lo, hi) with lo % 8 != 0; G = 1, 2, 4, 7, 8; every chunk edge the kernels derive is planted.
  D  negative controls: the kernels called once with a range shifted by one FAIL the bar.
  and the long-range decode: nsplit * 4096 keys must cover the cache (refused otherwise), nsplit = 2 over 8 000 keys is exact to the bar."""
import contextlib

import pytest
import torch

import _attn_probe as P

pytestmark = pytest.mark.gpu

BF = torch.bfloat16


def _mods():
    from audio_flamingo_amd import _lib, ops

    return ops, _lib


def _c(x, B, S, H, D):
    """kernel rows [B*S, >= H*D] -> canonical [B, H, S, D]"""
    return x[:, : H * D].reshape(B, S, H, D).transpose(1, 2)


@contextlib.contextmanager
def _knobs(sched=1, xcd=1, persist=False, paired=0, parts=0, fuse_delta=True, fuse_rope=True):
    ops, lib = _mods()
    old = (ops.ATTN_PERSIST, ops.ATTN_FUSE_DELTA, ops.ATTN_FUSE_ROPE_BWD)
    try:
        lib.call("afk_attn_set_sched", sched)
        lib.call("afk_attn_set_xcd_map", xcd)
        lib.call("afk_attn_set_persist_paired", paired)
        lib.call("afk_attn_set_dkdv_parts", parts)
        ops.ATTN_PERSIST, ops.ATTN_FUSE_DELTA, ops.ATTN_FUSE_ROPE_BWD = persist, fuse_delta, fuse_rope
        yield
    finally:
        ops.ATTN_PERSIST, ops.ATTN_FUSE_DELTA, ops.ATTN_FUSE_ROPE_BWD = old
        lib.call("afk_attn_set_sched", 1)
        lib.call("afk_attn_set_xcd_map", 1)
        lib.call("afk_attn_set_persist_paired", 0)
        lib.call("afk_attn_set_dkdv_parts", 0)


def _train_knobs(S, Hq, Hkv, kv_len, kv_lo):
    """the knob settings of test_attention_schedules_bit_equal, test_attention_forward_persistent_form_bit_equal and
    test_attention_backward_fused_rope_bit_equal (the rotary ones run separately), plus the separate delta pass"""
    ks = [dict(), dict(sched=0, xcd=0), dict(sched=0, xcd=1), dict(sched=1, xcd=0), dict(fuse_delta=False)]
    if kv_len is None and kv_lo is None and S % 128 == 0:
        ks += [dict(persist=True), dict(persist=True, paired=1)]
    if Hq != Hkv:
        ks += [dict(parts=p) for p in (1, 2, 3, 7)]
    return ks


def _rope_tables(S, D, dev):
    inv = 1.0 / (10000.0 ** (torch.arange(0, D, 2, device=dev, dtype=torch.float32) / D))
    fr = torch.arange(S + 8, device=dev, dtype=torch.float32)[:, None] * inv[None]
    emb = torch.cat([fr, fr], -1)
    return emb.cos().to(BF).contiguous(), emb.sin().to(BF).contiguous()


def _check_train(tag, case, o, dqkv, B, S, Hq, Hkv, D, refs, rope=None):
    """forward on the probed rows, dQ on the probed rows, dK / dV on the planted keys, exact zeros where padding must be zero.  refs: [(o, fp64
    gradients with delta from that o)] - the forward is bit-identical across the knobs (tests/test_ops_gpu.py), so one backward reference serves them"""
    lo, hi = case.info["lo"], case.info["hi"]
    oc = _c(o, B, S, Hq, D)
    P.check(f"{tag} O", oc, case.ref(), case.rows, D)
    g = next((g_ for o_, g_ in refs if torch.equal(o_, o)), None)
    if g is None:
        g = case.ref(grad=True, o_bwd=oc)
        refs.append((o.clone(), g))
    dq, dk, dv = _c(dqkv, B, S, Hq, D), _c(dqkv[:, Hq * D:], B, S, Hkv, D), _c(dqkv[:, (Hq + Hkv) * D:], B, S, Hkv, D)
    rdq, rdk = g[1], g[2]
    if rope is not None:
        pos = torch.arange(S, device=o.device)[None].expand(B, S)
        rdq, rdk = P.rope_backward(rdq, rope[0], rope[1], pos), P.rope_backward(rdk, rope[0], rope[1], pos)
    P.check(f"{tag} dQ", dq, rdq, case.rows, D)
    P.check(f"{tag} dK", dk, rdk, case.keys, D)
    P.check(f"{tag} dV", dv, g[3], case.keys, D)
    for b in range(B):
        assert (dk[b, :, : lo[b]] == 0).all() and (dk[b, :, hi[b]:] == 0).all(), f"{tag}: padded keys of sample {b} must get exact-zero dK"
        assert (dv[b, :, : lo[b]] == 0).all() and (dv[b, :, hi[b]:] == 0).all(), f"{tag}: padded keys of sample {b} must get exact-zero dV"
        if case.info["causal"]:
            assert (oc[b, :, : lo[b]] == 0).all() and (dq[b, :, : lo[b]] == 0).all(), f"{tag}: left-padded rows of sample {b} must be exact zeros"


# ------------------------------------------------------------------------------------------------ A: training attention
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("S", P.TRAIN_S)
def test_training_attention_edges(dev, S, D):
    ops, _ = _mods()
    for name, B, Hq, Hkv, causal, kv_len, kv_lo in P.train_layouts(S):
        case, qkv, do = P.training_case(B, S, Hq, Hkv, D, causal, kv_len=kv_len, kv_lo=kv_lo, seed=S + D, device=dev)
        kl = torch.tensor(kv_len, device=dev, dtype=torch.int32) if kv_len else None
        kb = torch.tensor(kv_lo, device=dev, dtype=torch.int32) if kv_lo else None
        refs = []
        for kn in _train_knobs(S, Hq, Hkv, kv_len, kv_lo):
            with _knobs(**kn):
                o, lse = ops.attn_fwd(qkv, B, S, Hq, Hkv, D, scale=D ** -0.5, causal=causal, kv_len=kl, kv_lo=kb)
                dqkv = ops.attn_bwd(qkv, o, do, lse, B, S, Hq, Hkv, D, scale=D ** -0.5, causal=causal, kv_len=kl, kv_lo=kb)
                torch.cuda.synchronize()
            _check_train(f"S={S} D={D} {name} {kn}", case, o, dqkv, B, S, Hq, Hkv, D, refs)
        if causal:   # the decoder's rotary backward, inside the attention backward or behind it
            cos, sin = _rope_tables(S, D, dev)
            for fuse in (True, False):
                with _knobs(fuse_rope=fuse, parts=7 if fuse and Hq != Hkv else 0):
                    o, lse = ops.attn_fwd(qkv, B, S, Hq, Hkv, D, scale=D ** -0.5, causal=True, kv_len=kl, kv_lo=kb)
                    dqkv = ops.attn_bwd(qkv, o, do, lse, B, S, Hq, Hkv, D, scale=D ** -0.5, causal=True, kv_len=kl, kv_lo=kb, rope=(cos, sin, None))
                    torch.cuda.synchronize()
                _check_train(f"S={S} D={D} {name} rope fused={fuse}", case, o, dqkv, B, S, Hq, Hkv, D, refs, rope=(cos, sin))


# ------------------------------------------------------------------------------------------------ B: interval / cross attention
def _interval_run(layout, q, k, v, kr, do):
    """-> (o rows, o, dq, dk, dv canonical), through ops.attn_interval_* (fused q|k|v) or ops.xattn_* on row-strided views"""
    ops, _ = _mods()
    B, Sq, Sk, Hq, Hkv, D, self_attn, slack = layout
    rows = lambda t, S, H: t.transpose(1, 2).reshape(B * S, H * D)
    dor = rows(do, Sq, Hq).contiguous()
    if self_attn:
        qkv = torch.cat([rows(q, Sq, Hq), rows(k, Sk, Hkv), rows(v, Sk, Hkv)], 1).contiguous()
        o, lse = ops.attn_interval_fwd(qkv, kr, B, Sq, Hq, Hkv, D, scale=D ** -0.5)
        dqkv = ops.attn_interval_bwd(qkv, o, dor, lse, kr, B, Sq, Hq, Hkv, D, scale=D ** -0.5)
        torch.cuda.synchronize()
        return o, _c(o, B, Sq, Hq, D), _c(dqkv, B, Sq, Hq, D), _c(dqkv[:, Hq * D:], B, Sk, Hkv, D), _c(dqkv[:, (Hq + Hkv) * D:], B, Sk, Hkv, D)
    # row pitch H * D + slack: the views the model hands the kernels
    wide = lambda t, S, H: torch.cat([rows(t, S, H), torch.full((B * S, slack), 3.0, device=t.device, dtype=BF)], 1)[:, : H * D]
    q2, k2, v2 = wide(q, Sq, Hq), wide(k, Sk, Hkv), wide(v, Sk, Hkv)
    o, lse = ops.xattn_fwd(q2, k2, v2, kr, B, Sq, Sk, Hq, Hkv, D, D ** -0.5)
    dq, dk, dv = (torch.full((B * S, H * D + slack), 5.0, device=q.device, dtype=BF)[:, : H * D] for S, H in ((Sq, Hq), (Sk, Hkv), (Sk, Hkv)))
    ops.xattn_bwd(q2, k2, v2, o, dor, lse, kr, B, Sq, Sk, Hq, Hkv, D, D ** -0.5, dq, dk, dv)
    torch.cuda.synchronize()
    return o, _c(o, B, Sq, Hq, D), _c(dq, B, Sq, Hq, D), _c(dk, B, Sk, Hkv, D), _c(dv, B, Sk, Hkv, D)


@pytest.mark.parametrize("layout", P.INTERVAL_LAYOUTS, ids=lambda l: f"B{l[0]}-Sq{l[1]}-Sk{l[2]}-H{l[3]}:{l[4]}-D{l[5]}{'-self' if l[6] else ''}")
def test_interval_attention_edges(dev, layout):
    """afk_xattn_fwd / afk_xattn_bwd - the per-query key intervals of the gated cross-attention, of the interval left-padding path and of the multi-row
    decode against a cache: forward, dQ, dK and dV against fp64 autograd on every planted boundary; empty intervals give exact-zero rows and dQ"""
    B, Sq, Sk, Hq, Hkv, D, _, _ = layout
    case, q, k, v, kr, do = P.interval_case(B, Sq, Sk, Hq, Hkv, D, seed=Sq + Sk, device=dev)
    _, oc, dq, dk, dv = _interval_run(layout, q, k, v, kr, do)
    tag = f"interval {layout}"
    P.check(f"{tag} O", oc, case.ref(), case.rows, D)
    g = case.ref(grad=True, o_bwd=oc)
    P.check(f"{tag} dQ", dq, g[1], case.rows, D)
    P.check(f"{tag} dK", dk, g[2], case.keys, D)
    P.check(f"{tag} dV", dv, g[3], case.keys, D)
    empty = case.info["empty"]
    assert int(empty.sum()) >= B
    for b, i in empty.nonzero().tolist():
        assert (oc[b, :, i] == 0).all() and (dq[b, :, i] == 0).all(), f"{tag}: empty interval (sample {b}, row {i}) must give exact zeros"


# ------------------------------------------------------------------------------------------------ C: decode attention
def _decode_layout(q, k, v, Smax):
    """canonical -> the kernels' layout: Q [B][Hq][D], K cache [B][pos][Hkv][D], V^T cache [B][Hkv][D][spad] (zero padded)"""
    ops, _ = _mods()
    spad = ops.pad64(Smax)
    B, Hkv, _, D = k.shape
    vt = torch.zeros((B, Hkv, D, spad), device=k.device, dtype=BF)
    vt[..., :Smax] = v.transpose(-1, -2)
    return q[:, :, 0].contiguous(), k.transpose(1, 2).contiguous(), vt, spad


def _decode_call(fused, qd, kc, vt, kr, Hq, Hkv, D, Smax, spad, ns):
    ops, lib = _mods()
    assert all(t.is_cuda for t in (qd, kc, vt, kr)), "the decode kernels take device pointers only"
    B = qd.shape[0]
    nq, nk = Hq * D, Hkv * D
    ws = torch.zeros(lib.load().afk_attn_decode_workspace_floats(B, Hq, D, ns), device=qd.device, dtype=torch.float32)
    o = torch.full((B, Hq, D), 7.0, device=qd.device, dtype=BF)
    lib.call("afk_attn_decode_fused" if fused else "afk_attn_decode", qd.data_ptr(), nq, D, kc.data_ptr(), Smax * nk, nk, D, vt.data_ptr(), Hkv * D * spad,
             spad, o.data_ptr(), nq, D, kr.data_ptr(), B, Hq, Hkv, D, float(D ** -0.5), ns, ws.data_ptr(), ops._stream())
    torch.cuda.synchronize()
    if fused:
        assert int(ws[-B * Hq:].view(torch.int32).abs().sum()) == 0, "arrival counters must be left at zero"
    return o[:, :, None]


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("G", sorted(P.DECODE_HEADS))
def test_decode_attention_edges(dev, G, D):
    """split-KV decode over a cache: every chunk edge the kernels derive for nsplit, lo - 1 and [lo & ~7, lo) (decoys), lo, hi - 1 (the newest key), hi
    (the next cache slot; for sample 0 the first slot of sample 1) - the two-launch form and the one-launch form in each afk_attn_decode_set_group mode"""
    _, lib = _mods()
    Hq, Hkv = P.DECODE_HEADS[G]
    kr = torch.tensor(P.DECODE_RANGES, device=dev, dtype=torch.int32)
    B, Smax = len(P.DECODE_RANGES), P.DECODE_SMAX
    try:
        for fused in (False, True):
            for ns in P.decode_splits(D, fused):
                case, q, k, v = P.decode_case(B, Smax, Hq, Hkv, D, P.DECODE_RANGES, ns, seed=ns, device=dev)
                qd, kc, vt, spad = _decode_layout(q, k, v, Smax)
                ref = case.ref()
                for mode in ((0, 1, 2, 3, -1) if fused else (-1,)):
                    lib.call("afk_attn_decode_set_group", mode)
                    o = _decode_call(fused, qd, kc, vt, kr, Hq, Hkv, D, Smax, spad, ns)
                    P.check(f"decode G={G} D={D} fused={fused} ns={ns} group mode {mode}", o, ref, case.rows, D)
    finally:
        lib.call("afk_attn_decode_set_group", -1)


def test_decode_long_range_needs_enough_splits(dev):
    """the per-head decode kernel holds at most 4 096 keys per split.  Over a cache of 8 000 positions nsplit = 1 must be REFUSED (it used to read the first
    4 096 keys of the range and drop the rest, the newest key included); nsplit = 2 must match the reference on every probe, hi - 1 included"""
    _, lib = _mods()
    Hq, Hkv, D = 4, 2, 128
    B, Smax = len(P.LONG_RANGES), P.LONG_SMAX
    kr = torch.tensor(P.LONG_RANGES, device=dev, dtype=torch.int32)
    case, q, k, v = P.decode_case(B, Smax, Hq, Hkv, D, P.LONG_RANGES, 2, seed=5, device=dev)
    qd, kc, vt, spad = _decode_layout(q, k, v, Smax)
    assert spad > 4096
    for fused in (False, True):
        with pytest.raises(lib.AfkError, match="spad"):
            _decode_call(fused, qd, kc, vt, kr, Hq, Hkv, D, Smax, spad, 1)
    ref = case.ref()
    try:
        for fused, mode in ((False, -1), (True, 0), (True, -1)):
            lib.call("afk_attn_decode_set_group", mode)
            o = _decode_call(fused, qd, kc, vt, kr, Hq, Hkv, D, Smax, spad, 2)
            P.check(f"decode long range ns=2 fused={fused} mode={mode}", o, ref, case.rows, D)
    finally:
        lib.call("afk_attn_decode_set_group", -1)


# ------------------------------------------------------------------------------------------------ D: negative controls
def _fails(tag, got, ref, slots, D):
    worst = P.slice_errors(got, ref, slots, D)[0]
    assert worst[0] > 1.0, f"{tag}: a kernel given a range shifted by one passed the probe bar (worst slice at {worst[0]:.2f} x the bar)"


def test_negative_controls_fail_the_bar(dev):
    """the comparison detects an off-by-one on the kernels themselves: each kernel is called once with a range shifted by one (only ever shrunk: every read
    stays in bounds) and its output must FAIL the bar against the true reference"""
    ops, _ = _mods()
    D, S = 128, 129
    # training: kv_len - 1 (right-padded encoder layout), kv_len - 1 and kv_lo + 1 (left-padded decoder layout)
    for name, B, Hq, Hkv, causal, kv_len, kv_lo in P.train_layouts(S)[1:4:2]:
        case, qkv, do = P.training_case(B, S, Hq, Hkv, D, causal, kv_len=kv_len, kv_lo=kv_lo, seed=S + D, device=dev)
        kl = torch.tensor([x - 1 for x in kv_len], device=dev, dtype=torch.int32)
        kb = torch.tensor([x + 1 for x in kv_lo], device=dev, dtype=torch.int32) if kv_lo else None
        o, _ = ops.attn_fwd(qkv, B, S, Hq, Hkv, D, scale=D ** -0.5, causal=causal, kv_len=kl, kv_lo=kb)
        torch.cuda.synchronize()
        _fails(f"training {name}", _c(o, B, S, Hq, D), case.ref(), case.rows, D)
    # interval: every non-empty interval ends one key early
    layout = P.INTERVAL_LAYOUTS[0]
    B, Sq, Sk, Hq, Hkv, Di, _, _ = layout
    case, q, k, v, kr, do = P.interval_case(B, Sq, Sk, Hq, Hkv, Di, seed=Sq + Sk, device=dev)
    kr2 = kr.clone()
    kr2[..., 1] -= (kr2[..., 1] > kr2[..., 0]).int()
    _fails("interval", _interval_run(layout, q, k, v, kr2, do)[1], case.ref(), case.rows, Di)
    # decode: every range ends one key early (the newest key dropped)
    Hq, Hkv = P.DECODE_HEADS[7]
    B, Smax = len(P.DECODE_RANGES), P.DECODE_SMAX
    case, q, k, v = P.decode_case(B, Smax, Hq, Hkv, D, P.DECODE_RANGES, 8, seed=8, device=dev)
    qd, kc, vt, spad = _decode_layout(q, k, v, Smax)
    kr = torch.tensor([(lo, hi - 1) for lo, hi in P.DECODE_RANGES], device=dev, dtype=torch.int32)
    _fails("decode", _decode_call(True, qd, kc, vt, kr, Hq, Hkv, D, Smax, spad, 8), case.ref(), case.rows, D)

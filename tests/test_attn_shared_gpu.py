"""GPU: afk_attn_decode_shared (csrc/attention_shared.hip) against the fp64 restatement of its contract (tests/_shared_ref.py) on planted-key cases, held to
the project's bar for the append and decode kernels (_attn_probe.check: ||got - ref||_2 <= 2^-6 ||ref||_2 + 2^-8 sqrt(D) per (continuation, head) slice).
Every slot outside an interval and every pad column is NaN; one key outside each interval end is a decoy that would dominate the row if it were seen."""
import functools

import pytest
import torch

import _attn_probe as P
import _shared_ref as S

pytestmark = pytest.mark.gpu

BF = torch.bfloat16


def _mods():
    from audio_flamingo_amd import _lib, ops

    return ops, _lib


@functools.lru_cache(maxsize=None)
def _case(case):
    """the CPU case and its fp64 reference, built once and shared by the tests (never written to)"""
    c = S.shared_case(*case)
    c.reference()
    return c


def _run(c, d, nsplit=None, prange=None, trange=None, **kw):
    ops, _ = _mods()
    Hq, D = c.Hq, c.D
    o = ops.attn_decode_shared(d["qkv"][:, : Hq * D], d["Kp"], d["Vtp"], d["Kt"], d["Vtt"], d["prange"] if prange is None else prange,
                               d["trange"] if trange is None else trange, c.B0, c.n, Hq, c.Hkv, D, D ** -0.5, nsplit=c.nsplit if nsplit is None else nsplit, **kw)
    torch.cuda.synchronize()
    return o.reshape(c.B0 * c.n, Hq, 1, D).cpu()   # the references live on the host


@pytest.mark.parametrize("case", S.CASES, ids=str)
def test_shared_attention_edges(dev, case):
    c = _case(case)
    d = c.to(dev)
    got = _run(c, d)
    worst = P.check(f"attn_decode_shared {case}", got, c.reference(), c.slots(), c.D)
    print(f"{case}: worst err / bar {worst:.3f}")
    again = _run(c, d)
    assert torch.equal(got.view(torch.int16), again.view(torch.int16)), "two launches on the same inputs differ"


@pytest.mark.parametrize("ns", [1, 3, 8])
def test_every_split_count_stays_inside_the_bar(dev, ns):
    for case in (S.CASES[1], S.CASES[3]):
        c = _case(case)
        P.check(f"attn_decode_shared {case} nsplit {ns}", _run(c, c.to(dev), nsplit=ns), c.reference(), c.slots(), c.D)


def test_rows_with_both_intervals_empty_are_exact_zeros(dev):
    c = _case(S.CASES[2])
    d = c.to(dev)
    pr, tr = d["prange"].clone(), d["trange"].clone()
    pr[1, 1] = pr[1, 0]                       # prompt row 1 sees no prompt key
    empty = [c.n + 1, c.n + 4]                # two of its continuations (one in each column tile) see no tail key either
    for r in empty:
        tr[r, 1] = tr[r, 0]
    tr[2, 0], tr[2, 1] = 7, 3                 # an interval that ends in front of its begin is empty too; row 2 still sees its prompt
    out = torch.full((c.B0 * c.n, c.Hq * c.D), 7.0, device=dev, dtype=BF)
    got = _run(c, d, prange=pr, trange=tr, out=out)
    for r in empty:
        assert torch.equal(got[r].view(torch.int16), torch.zeros_like(got[r]).view(torch.int16)), f"continuation {r} is not +0.0 everywhere"
    ref = S.reference(c.q, c.Kp, c.Vtp, c.Kt, c.Vtt, pr.cpu(), tr.cpu(), c.n, c.Hq, c.Hkv, c.D, c.D ** -0.5)
    P.check("attn_decode_shared with empty rows", got, ref, c.slots(), c.D)


@pytest.mark.parametrize("case", [S.CASES[1], S.CASES[2]], ids=str)
def test_negative_controls_fail_the_bar(dev, case):
    """one key more at the end of the prompt interval, and separately of the tail interval (the decoys), must break the bar: the planted keys have teeth"""
    c = _case(case)
    d = c.to(dev)
    one = torch.tensor([0, 1], device=dev, dtype=torch.int32)
    for kw in (dict(prange=d["prange"] + one), dict(trange=d["trange"] + one)):
        got = _run(c, d, **kw)
        worst = P.slice_errors(got, c.reference(), c.slots(), c.D)[0][0]
        assert worst >= P.SEP, f"{case} {list(kw)}: an interval end moved by one key goes unnoticed (worst err / bar {worst:.2f})"
        mut = c.reference(dp=1) if "prange" in kw else c.reference(dt=1)
        P.check(f"attn_decode_shared {case} mutated {list(kw)}", got, mut, c.slots(), c.D)   # and it is exactly the mutation that was computed


@pytest.mark.parametrize("case", [S.CASES[2], S.CASES[4]], ids=str)
def test_against_the_launch_it_replaces(dev, case):
    """the expanded cache (every continuation's visible prompt keys, then its tail keys, in a cache row of its own) through afk_attn_decode_fused: both
    results inside the bar of the same reference"""
    ops, lib = _mods()
    c = _case(case)
    d = c.to(dev)
    R, Hq, Hkv, D, nk = c.B0 * c.n, c.Hq, c.Hkv, c.D, c.Hkv * c.D
    Smax = c.Sp + c.T
    spad = ops.pad64(Smax)
    K = torch.zeros((R, Smax, nk), device=dev, dtype=BF)
    Vt = torch.zeros((R, Hkv, D, spad), device=dev, dtype=BF)
    kr = torch.zeros((R, 2), device=dev, dtype=torch.int32)
    for r in range(R):
        b0 = r // c.n
        (lo, hi), (t0, t1) = c.prange[b0].tolist(), c.trange[r].tolist()
        K[r, lo:hi], Vt[r, :, :, lo:hi] = d["Kp"][b0, lo:hi], d["Vtp"][b0, :, :, lo:hi]
        K[r, hi:hi + t1 - t0], Vt[r, :, :, hi:hi + t1 - t0] = d["Kt"][r, t0:t1], d["Vtt"][r, :, :, t0:t1]
        kr[r, 0], kr[r, 1] = lo, hi + t1 - t0
    q = d["qkv"][:, : Hq * D].contiguous()
    ns = 8
    ws = torch.zeros(lib.load().afk_attn_decode_workspace_floats(R, Hq, D, ns), device=dev, dtype=torch.float32)
    o = torch.empty((R, Hq * D), device=dev, dtype=BF)
    lib.call("afk_attn_decode_fused", q.data_ptr(), Hq * D, D, K.data_ptr(), Smax * nk, nk, D, Vt.data_ptr(), Hkv * D * spad, spad, o.data_ptr(), Hq * D, D,
             kr.data_ptr(), R, Hq, Hkv, D, float(D ** -0.5), ns, ws.data_ptr(), ops._stream())
    torch.cuda.synchronize()
    P.check(f"afk_attn_decode_fused on the expanded cache {case}", o.reshape(R, Hq, 1, D).cpu(), c.reference(), c.slots(), D)
    P.check(f"attn_decode_shared {case}", _run(c, d), c.reference(), c.slots(), D)


def test_contract_refusals(dev):
    ops, lib = _mods()
    c = _case(S.CASES[1])
    d = c.to(dev)
    B0, n, Hq, Hkv, D = c.B0, c.n, c.Hq, c.Hkv, c.D
    q = d["qkv"][:, : Hq * D]
    call = lambda **kw: ops.attn_decode_shared(*[kw.get(k, v) for k, v in (("q", q), ("Kp", d["Kp"]), ("Vtp", d["Vtp"]), ("Kt", d["Kt"]), ("Vtt", d["Vtt"]),
                                                                             ("prange", d["prange"]), ("trange", d["trange"]))],
                                               kw.get("B0", B0), kw.get("n", n), kw.get("Hq", Hq), kw.get("Hkv", Hkv), D, D ** -0.5, nsplit=kw.get("nsplit", 2), ws=kw.get("ws"))
    # the kernel's envelope, by its own messages
    for kw, msg in ((dict(nsplit=0), r"nsplit 0 outside \[1, 64\]"), (dict(nsplit=65), r"nsplit 65 outside \[1, 64\]"),
                    (dict(ws=torch.empty(16, device=dev)), "afk_attn_decode_shared_workspace_floats says")):
        with pytest.raises(lib.AfkError, match="afk_attn_decode_shared.*" + msg):
            call(**kw)
    R17 = 17
    z = lambda *s: torch.zeros(s, device=dev, dtype=BF)
    with pytest.raises(lib.AfkError, match=r"afk_attn_decode_shared: 17 continuations per prompt row outside \[1, 16\]"):
        ops.attn_decode_shared(z(R17, Hq * D), z(1, 32, Hkv * D), z(1, Hkv, D, 64), z(R17, 4, Hkv * D), z(R17, Hkv, D, 64),
                               torch.zeros((1, 2), device=dev, dtype=torch.int32), torch.zeros((R17, 2), device=dev, dtype=torch.int32), 1, R17, Hq, Hkv, D, 1.0,
                               nsplit=1, ws=torch.empty(1 << 20, device=dev))
    with pytest.raises(lib.AfkError, match=r"afk_attn_decode_shared: Hq / Hkv = 3 \(1 / 2 / 4 / 7 / 8 supported\)"):
        ops.attn_decode_shared(z(2, 6 * D), z(1, 32, 2 * D), z(1, 2, D, 64), z(2, 4, 2 * D), z(2, 2, D, 64), torch.zeros((1, 2), device=dev, dtype=torch.int32),
                               torch.zeros((2, 2), device=dev, dtype=torch.int32), 1, 2, 6, 2, D, 1.0, nsplit=1)
    with pytest.raises(lib.AfkError, match=r"afk_attn_decode_shared: head_dim 32 \(64 / 128 supported\)"):
        ops.attn_decode_shared(z(2, 64), z(1, 32, 64), z(1, 2, 32, 64), z(2, 4, 64), z(2, 2, 32, 64), torch.zeros((1, 2), device=dev, dtype=torch.int32),
                               torch.zeros((2, 2), device=dev, dtype=torch.int32), 1, 2, 2, 2, 32, 1.0, nsplit=1)
    with pytest.raises(lib.AfkError, match="spad_p / spad_t must be multiples of 32"):   # a value pitch of 40 columns
        ops.attn_decode_shared(q, d["Kp"], d["Vtp"], d["Kt"], z(B0 * n, Hkv, D, 40), d["prange"], d["trange"], B0, n, Hq, Hkv, D, 1.0, nsplit=1)
    with pytest.raises(lib.AfkError, match="strides and pointers must keep 16-byte alignment"):   # a query row pitch that is no multiple of 8 elements
        ops.attn_decode_shared(z(B0 * n, Hq * D + 4)[:, : Hq * D], d["Kp"], d["Vtp"], d["Kt"], d["Vtt"], d["prange"], d["trange"], B0, n, Hq, Hkv, D, 1.0, nsplit=1)
    # the op's shape and stride checks
    for kw, msg in ((dict(q=q[:-1]), "attn_decode_shared: q "), (dict(Kp=d["Kp"][:, :, :-8]), "attn_decode_shared: Kp "), (dict(Kt=d["Kt"][:-1]), "attn_decode_shared: Kt "),
                    (dict(Vtp=d["Vtp"][..., ::2]), "attn_decode_shared: Vtp "), (dict(Vtt=d["Vtt"][:, :1]), "attn_decode_shared: Vtt "),
                    (dict(prange=d["trange"]), "attn_decode_shared: prange "), (dict(trange=d["trange"][:-1]), "attn_decode_shared: prange .* trange ")):
        with pytest.raises(lib.AfkError, match=msg):
            call(**kw)
    with pytest.raises(lib.AfkError):
        call(prange=d["prange"].long())

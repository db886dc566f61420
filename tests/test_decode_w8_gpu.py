"""GPU: FP8 decode weights - afk_quantize_rows_fp8, the afk_decode_chain_*_w8 launches and generate(decode_weights="fp8").

The oracle is exact by construction: a power-of-two row scale makes code * scale representable in bf16, so the FP8 launches on (codes, scale) and the bf16
kernels on W_deq = codes * scale see the SAME weight values and differ only in summation order.  The kernel tests therefore compare each _w8 launch with the
stand-alone kernel sequence on W_deq at the tolerances of tests/test_ops_gpu.py::test_decode_chain_kernels_vs_standalone_sequence (atol 3e-2 / rtol 2e-2; gate|up
3e-2 / 3e-2), and the generate() tests run on the trained tiny golden (case A) with its decoder Linears and lm_head snapped onto the FP8 grid, where the FP8 copy is
lossless and the prefill is the same launches for both routes.  The CPU oracle (fp32) puts the top-1 / top-2 gap of that snapped model's first 14 greedy positions
at 6.3 .. 15.9 x the logit bar of tests/_tol.py and its ids at the golden's, so the ids of the two routes must be identical."""
import os
from collections import Counter

import pytest
import torch
import torch.nn.functional as F

from tests import _w8_ref as R
from tests._tol import logit_tol
from tests.test_ops_gpu import _cmp

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
TOL = dict(atol=3e-2, rtol=2e-2)        # test_decode_chain_kernels_vs_standalone_sequence's
TOL_GU = dict(atol=3e-2, rtol=3e-2)     # ... for gate|up
KNOBS = ["", "S=1,1,1,1,1", "S=8,8,8,8,8", "S=2,2,2,2,2 R=4,4,4,4,4"]
W8_NAMES = ("afk_decode_chain_qkv_w8", "afk_decode_chain_linear_residual_w8", "afk_decode_chain_gate_up_w8", "afk_decode_chain_lm_head_w8")
BF16_NAMES = tuple(n[:-3] for n in W8_NAMES)
EPS = 1e-6


def _ops():
    from audio_flamingo_amd import ops

    return ops


def _randn(shape, dev, scale, seed):
    g = torch.Generator(device=dev).manual_seed(seed)
    return (torch.randn(shape, generator=g, device=dev) * scale).to(BF)


def _quant(w, name="weight"):
    from audio_flamingo_amd import decode_w8

    return decode_w8.quantize_rows(w, name)


_LUT = {}


def _code_values(codes):
    """the fp32 value of every code, through a 256-entry table of torch's own e4m3fn decoding"""
    if codes.device not in _LUT:
        _LUT[codes.device] = torch.arange(256, dtype=torch.uint8).view(torch.float8_e4m3fn).float().to(codes.device)
    return _LUT[codes.device][codes.int()]


def _deq(q):
    """W_deq = codes x scale as a bf16 tensor - exact, and asserted to be"""
    prod = _code_values(q.codes) * q.scale[:, None]
    w = prod.to(BF)
    assert torch.equal(w.float(), prod), "code * scale must be representable in bf16"
    return w


def _gemm(a, w, **kw):
    """ops.gemm_nt; its K is a multiple of 64, so other widths are padded with zero columns on both operands (the sums are the same)"""
    K = a.shape[1]
    pad = -K % 64
    if pad:
        a, w = F.pad(a, (0, pad)), F.pad(w, (0, pad))
    return _ops().gemm_nt(a.contiguous(), w.contiguous(), **kw)


def _q8(q):
    return q.codes.data_ptr(), q.codes.stride(0), q.scale.data_ptr()


# ------------------------------------------------------------------------------------------------ 1. the quantiser
@pytest.mark.parametrize("N,K", [(8, 16), (24, 1040), (64, 3584)])
def test_quantiser_equals_the_restatement(dev, N, K):
    buf = torch.zeros((N, K + 24), device=dev, dtype=BF)   # a padded ldw
    w = buf[:, :K]
    w.copy_(_randn((N, K), dev, 0.02, N + K))
    w[1].zero_()                                           # an all-zero row
    w[2].clamp_(-1.0, 1.0)
    w[2, K // 2] = -448.0 * 2.0 ** -7                      # a row max exactly on the largest code
    w[3, 7] = 3.0e4                                        # one huge outlier: the rest of the row falls into the subnormals and to zero
    w[4, 0], w[4, 1] = -0.0, 2.0 ** -120
    assert w.stride(0) == K + 24
    q = _quant(w)
    codes, scale = R.quantize(w.cpu())
    assert q.codes.dtype == torch.uint8 and q.scale.dtype == torch.float32
    assert torch.equal(q.scale.cpu(), scale), f"scales differ at rows {(q.scale.cpu() != scale).nonzero().flatten().tolist()[:8]}"
    assert torch.equal(q.codes.cpu(), codes), f"{int((q.codes.cpu() != codes).sum())} codes differ"
    assert float(scale[1]) == 1.0 and float(scale[2]) == 2.0 ** -7 and int(codes[1].sum()) == 0
    assert torch.equal(buf[:, K:], torch.zeros_like(buf[:, K:]))


def test_quantiser_refuses_nan_and_names_the_tensor(dev):
    from audio_flamingo_amd._lib import AfkError

    for poison in (float("nan"), float("inf"), float("-inf")):
        w = _randn((24, 1040), dev, 0.02, 1)
        w[17, 1033] = poison
        with pytest.raises(AfkError, match="layers.3.mlp.down_proj.weight"):
            _quant(w, "layers.3.mlp.down_proj.weight")


# ------------------------------------------------------------------------------------------------ 2. the kernels against the bf16 kernels on W_deq
_CASES = {}


def _rope_tables(dev, D):
    inv = 1.0 / (1e6 ** (torch.arange(0, D, 2, device=dev, dtype=torch.float32) / D))
    fr = torch.arange(64, device=dev, dtype=torch.float32)[:, None] * inv[None]
    emb = torch.cat([fr, fr], -1)
    return emb.cos().to(BF).contiguous(), emb.sin().to(BF).contiguous()


def _cases(dev):
    """every input, quantised weight and stand-alone reference of the kernel test, computed once and left unchanged: the knob sets share them"""
    if _CASES:
        return _CASES
    ops = _ops()
    qkv, lin, gu, head = [], [], [], []
    pos_t = torch.tensor([37], device=dev, dtype=torch.int32)
    # K = 16: less than one lane-vector per lane, every other lane masked; 1040: one full chunk + a one-vector tail; 3584: 3.5 chunks, the AF3 hidden size,
    # the second-pass boundary of the row statistic; 18944 (linear + residual only): down_proj, 18.5 chunks
    for K in (16, 1040, 3584):
        x = _randn((1, K), dev, 1.0, 10 + K)
        nw = (1 + 0.1 * _randn((K,), dev, 1.0, 11 + K).float()).to(BF)
        h, _ = ops.rmsnorm_fwd(x, nw, EPS)
        for Hq, Hkv, D in ((4, 2, 64),) + (((28, 4, 128),) if K == 3584 else ()):   # rotating and plain groups, q / k / v destinations
            nq, nk = Hq * D, Hkv * D
            q8 = _quant(_randn((nq + 2 * nk, K), dev, 0.02, 12 + K + D))
            bias = _randn((nq + 2 * nk,), dev, 0.1, 13 + K)
            cos, sin = _rope_tables(dev, D)
            ref = _gemm(h, _deq(q8), bias=bias)
            ops.rope_(ref, cos, sin, S=1, nheads=Hq + Hkv, D=D, pos=pos_t)
            qkv.append(dict(K=K, geom=(Hq, Hkv, D), x=x, nw=nw, q8=q8, bias=bias, cos=cos, sin=sin, ref=ref))
        for I in (64,) + ((18944,) if K == 3584 else ()):
            q8 = _quant(_randn((2 * I, K), dev, 0.02, 14 + K + I))
            gu.append(dict(K=K, I=I, x=x, nw=nw, q8=q8, ref=ops.silu_mul_fwd(_gemm(h, _deq(q8)))))
        q8 = _quant(_randn((4096, K), dev, 0.02, 15 + K))
        head.append(dict(K=K, x=x, nw=nw, q8=q8, ref=_gemm(h, _deq(q8)).float()))
    for K in (16, 1040, 3584, 18944):
        N = 72   # nine row groups: with four groups per block the last block is partly idle
        a, res = _randn((1, K), dev, 1.0, 20 + K), _randn((1, N), dev, 1.0, 21 + K)
        q8 = _quant(_randn((N, K), dev, 0.02, 22 + K))
        lin.append(dict(K=K, N=N, a=a, res=res, q8=q8, ref=_gemm(a, _deq(q8), residual=res)))
    torch.cuda.synchronize()
    _CASES.update(qkv=qkv, lin=lin, gu=gu, head=head, pos_t=pos_t)
    return _CASES


@pytest.mark.parametrize("knobs", KNOBS)
def test_w8_kernels_vs_bf16_kernels_on_dequantised_weights(dev, knobs, monkeypatch):
    from audio_flamingo_amd import _lib

    ops, c = _ops(), _cases(dev)
    for kv in knobs.split():   # waves / rows per group of every launch form (csrc/decode_chain.hip chain_knob), as the bf16 test sets them
        monkeypatch.setenv("AFK_CHAIN_" + kv[0], kv[2:])
    st = ops._stream()
    Smax, start = 128, 41
    spad = ops.pad64(Smax)
    start_t = torch.tensor([start], device=dev, dtype=torch.int32)
    for t in c["qkv"]:
        Hq, Hkv, D = t["geom"]
        nq, nk, tag = Hq * D, Hkv * D, f"K={t['K']} heads {t['geom']}"
        Kc = torch.zeros((1, Smax, nk), device=dev, dtype=BF)
        Vt = torch.zeros((1, Hkv, D, spad), device=dev, dtype=BF)
        q = torch.zeros((1, nq), device=dev, dtype=BF)
        _lib.call("afk_decode_chain_qkv_w8", t["x"].data_ptr(), t["nw"].data_ptr(), EPS, *_q8(t["q8"]), t["K"], t["bias"].data_ptr(), t["cos"].data_ptr(),
                  t["sin"].data_ptr(), c["pos_t"].data_ptr(), q.data_ptr(), Kc.data_ptr(), Vt.data_ptr(), spad, start_t.data_ptr(), Hq, Hkv, D, st)
        ref = t["ref"]
        _cmp(f"w8 q {tag}", q[0], ref[0, :nq].float(), **TOL)
        _cmp(f"w8 k {tag}", Kc[0, start], ref[0, nq:nq + nk].float(), **TOL)
        _cmp(f"w8 v {tag}", Vt[0, :, :, start].reshape(-1), ref[0, nq + nk:].float(), **TOL)
        Kc[0, start].zero_(), Vt[0, :, :, start].zero_()
        assert int((Kc != 0).sum()) == 0 and int((Vt != 0).sum()) == 0, f"{tag}: only the new cache slot may be written"
    for t in c["lin"]:
        out = torch.empty((1, t["N"]), device=dev, dtype=BF)
        _lib.call("afk_decode_chain_linear_residual_w8", t["a"].data_ptr(), *_q8(t["q8"]), t["N"], t["K"], t["res"].data_ptr(), out.data_ptr(), st)
        _cmp(f"w8 linear+residual K={t['K']}", out, t["ref"].float(), **TOL)
    for t in c["gu"]:
        act = torch.empty((1, t["I"]), device=dev, dtype=BF)
        _lib.call("afk_decode_chain_gate_up_w8", t["x"].data_ptr(), t["nw"].data_ptr(), EPS, *_q8(t["q8"]), t["I"], t["K"], act.data_ptr(), st)
        _cmp(f"w8 gate|up K={t['K']} I={t['I']}", act, t["ref"].float(), **TOL_GU)
    for t in c["head"]:
        V = t["q8"].codes.shape[0]
        logits = torch.empty((1, V), device=dev, dtype=torch.float32)
        pv = torch.empty(V // 8, device=dev, dtype=torch.float32)
        pi = torch.empty(V // 8, device=dev, dtype=torch.int32)
        _lib.call("afk_decode_chain_lm_head_w8", t["x"].data_ptr(), t["nw"].data_ptr(), EPS, *_q8(t["q8"]), V, t["K"], logits.data_ptr(), pv.data_ptr(), pi.data_ptr(), st)
        assert torch.equal(logits, logits.to(BF).float()), "the logits hold bf16 values"
        _cmp(f"w8 lm_head K={t['K']}", logits, t["ref"], **TOL)
        assert torch.equal(pv, logits.view(V // 8, 8).max(-1).values)
        assert torch.equal(pi.long(), logits.view(V // 8, 8).argmax(-1) + 8 * torch.arange(V // 8, device=dev))
        pv2, pi2 = torch.empty_like(pv), torch.empty_like(pi)   # the partial pairs alone (plain greedy decoding writes no logits row)
        _lib.call("afk_decode_chain_lm_head_w8", t["x"].data_ptr(), t["nw"].data_ptr(), EPS, *_q8(t["q8"]), V, t["K"], 0, pv2.data_ptr(), pi2.data_ptr(), st)
        assert torch.equal(pv2, pv) and torch.equal(pi2, pi)


# ------------------------------------------------------------------------------------------------ 3. arbitrary scales
def test_the_row_scale_is_applied_in_fp32_before_the_first_rounding(dev):
    """scales that are NOT powers of two: against scale * (codes . x) in fp64, then the epilogue's rounding points (bf16 of the sum, + residual, bf16)"""
    from audio_flamingo_amd import _lib

    N, K = 72, 1040
    q8 = _quant(_randn((N, K), dev, 0.02, 31))
    g = torch.Generator(device=dev).manual_seed(32)
    wscale = (torch.rand((N,), generator=g, device=dev) * 3 + 0.5).float() * q8.scale   # 0.5 .. 3.5 x the row's own scale: sums of the usual size
    a, res = _randn((1, K), dev, 1.0, 33), _randn((1, N), dev, 1.0, 34)
    out = torch.empty((1, N), device=dev, dtype=BF)
    _lib.call("afk_decode_chain_linear_residual_w8", a.data_ptr(), q8.codes.data_ptr(), q8.codes.stride(0), wscale.data_ptr(), N, K, res.data_ptr(), out.data_ptr(),
              _ops()._stream())
    tot = wscale.double() * (_code_values(q8.codes).double() @ a[0].double())
    ref = (tot.float().to(BF).float() + res[0].float()).to(BF)
    _cmp("w8 linear+residual, arbitrary scales", out[0], ref.float(), **TOL)
    assert float((tot.abs()).max()) > 0.5, "the comparison must see sums the scale matters for"


# ------------------------------------------------------------------------------------------------ 4. refusals of the entries
def test_w8_entries_refuse_bad_arguments(dev):
    from audio_flamingo_amd import _lib
    from audio_flamingo_amd._lib import AfkError

    st = _ops()._stream()
    N, K = 64, 64
    codes = torch.zeros((N, K + 16), device=dev, dtype=torch.uint8)
    scale = torch.ones((N,), device=dev, dtype=torch.float32)
    x, res, out = (torch.zeros((1, 64), device=dev, dtype=BF) for _ in range(3))
    good = [x.data_ptr(), codes.data_ptr(), codes.stride(0), scale.data_ptr(), N, K, res.data_ptr(), out.data_ptr(), st]
    _lib.call("afk_decode_chain_linear_residual_w8", *good)
    for i, v, word in ((5, 24, "K % 16"), (5, 40, "K % 16"), (2, K + 8, "ldq % 16"), (2, K - 16, "ldq"), (1, codes.data_ptr() + 8, "16-byte-aligned"), (1, 0, "K % 16"),
                       (3, 0, "scale per row"), (0, 0, "bad arguments"), (4, 12, "N % 8")):
        bad = list(good)
        bad[i] = v
        with pytest.raises(AfkError, match=word):
            _lib.call("afk_decode_chain_linear_residual_w8", *bad)
    nw, act = torch.ones(64, device=dev, dtype=BF), torch.zeros((1, 32), device=dev, dtype=BF)
    logits = torch.zeros((1, N), device=dev, dtype=torch.float32)
    with pytest.raises(AfkError, match="afk_decode_chain_gate_up_w8"):
        _lib.call("afk_decode_chain_gate_up_w8", x.data_ptr(), nw.data_ptr(), EPS, codes.data_ptr(), codes.stride(0), scale.data_ptr(), 32, 24, act.data_ptr(), st)
    with pytest.raises(AfkError, match="afk_decode_chain_gate_up_w8"):
        _lib.call("afk_decode_chain_gate_up_w8", x.data_ptr(), nw.data_ptr(), EPS, 0, codes.stride(0), scale.data_ptr(), 32, K, act.data_ptr(), st)
    with pytest.raises(AfkError, match="afk_decode_chain_lm_head_w8"):
        _lib.call("afk_decode_chain_lm_head_w8", x.data_ptr(), nw.data_ptr(), EPS, codes.data_ptr(), K + 8, scale.data_ptr(), N, K, logits.data_ptr(), 0, 0, st)
    with pytest.raises(AfkError, match="afk_decode_chain_lm_head_w8"):
        _lib.call("afk_decode_chain_lm_head_w8", x.data_ptr(), nw.data_ptr(), EPS, codes.data_ptr(), codes.stride(0), scale.data_ptr(), N, K, 0, 0, 0, st)
    cos, sin = _rope_tables(dev, 16)
    pos = torch.zeros(1, device=dev, dtype=torch.int32)
    qkv_args = lambda wq, ldq, k: [x.data_ptr(), nw.data_ptr(), EPS, wq, ldq, scale.data_ptr(), k, res.data_ptr(), cos.data_ptr(), sin.data_ptr(), pos.data_ptr(),
                                   out.data_ptr(), out.data_ptr(), out.data_ptr(), 64, pos.data_ptr(), 2, 1, 16, st]
    for wq, ldq, k in ((0, codes.stride(0), K), (codes.data_ptr(), codes.stride(0), 24), (codes.data_ptr(), K + 8, K)):
        with pytest.raises(AfkError, match="afk_decode_chain_qkv_w8"):
            _lib.call("afk_decode_chain_qkv_w8", *qkv_args(wq, ldq, k))


# ------------------------------------------------------------------------------------------------ 5 .. 8. generate()
FLAGS = dict(return_dict_in_generate=True, output_logits=True)
NEW = 12   # crosses the poll at step 8
_CTX = {}


def _snap_in_place(m):
    """w <- dequantize(quantize(w)) on every tensor the FP8 copy restates: on this model the copy is lossless"""
    from audio_flamingo_amd import decode_w8

    keys = [f"{m._lm}layers.{i}.{k}" for i in range(m.dec_layers) for k in decode_w8.LAYER_KEYS] + ["lm_head.weight"]
    for key in keys:
        blk = m.arena[key].data
        blk.copy_(R.snap(blk.cpu()))
    return keys


def _snapped(dev):
    if dev not in _CTX:
        from tests.test_model_gpu import G, N_GEN
        from tests.test_sampler_gpu import _case_a

        m, p, audio = _case_a(dev)
        _snap_in_place(m)
        gold = torch.load(os.path.join(G, "tiny64_caseA.pt"))["generate"][0, -N_GEN:].to(dev)
        _CTX[dev] = (m, p, audio, gold)
    return _CTX[dev]


def _spy(monkeypatch):
    from audio_flamingo_amd import _lib

    names, real = [], _lib.call
    monkeypatch.setattr(_lib, "call", lambda name, *a: (names.append(name), real(name, *a))[1])
    return names


def _hold_to_the_bf16_route(tag, ref, got, S0, greedy=True):
    """the fp8 call against the bf16 call (the reference): the logits rows within the logit bar up to and including the first step at which the ids part
    (behind it the calls condition on different ids); greedy: at that step the reference's top-1 / top-2 gap is at most 2 x the bar (tests/_tol.py's
    "confident" rule) - otherwise the difference is a bug, not a tie.  -> the step at which the ids part, or None"""
    assert got.sequences.shape == ref.sequences.shape and len(got.logits) == len(ref.logits)
    a, b = ref.sequences[0, S0:], got.sequences[0, S0:]
    diff = (a != b).nonzero().flatten().tolist()
    first = diff[0] if diff else None
    worst = 0.0
    for t in range(len(ref.logits) if first is None else first + 1):
        r, g = ref.logits[t].float(), got.logits[t].float()
        assert tuple(g.shape) == tuple(r.shape)
        err, bar = float((g - r).abs().max()), logit_tol(float(r.abs().max()))
        worst = max(worst, err / bar)
        assert err <= bar, f"{tag}: step {t} logits differ by {err:.4f}, bar {bar:.4f}"
    print(f"{tag}: worst |fp8 - bf16| logit = {worst:.3f} x the bar over {len(ref.logits) if first is None else first + 1} steps; ids part at {first}")
    if first is not None and greedy:
        row = ref.logits[first].float()[0]
        top = row.topk(2).values
        gap, bar = float(top[0] - top[1]), logit_tol(float(row.abs().max()))
        assert gap <= 2 * bar, f"{tag}: the ids part at step {first}, where the bf16 route is confident (gap {gap:.4f}, bar {bar:.4f})"
    return first


@pytest.mark.parametrize("use_graph", [False, True])
def test_generate_fp8_equals_bf16_on_the_snapped_model(dev, use_graph):
    m, p, audio, gold = _snapped(dev)
    kw = dict(audio, max_new_tokens=NEW, use_graph=use_graph, **FLAGS)
    ref = m.generate(p, **kw)
    assert m.last_w8_stats is None
    got = m.generate(p, decode_weights="fp8", **kw)
    assert m.last_w8_stats is not None and m.last_w8_stats["tensors"] == 4 * m.dec_layers + 1
    first = _hold_to_the_bf16_route(f"greedy, use_graph={use_graph}", ref, got, p.shape[1])
    assert first is None and torch.equal(got.sequences, ref.sequences), "on the snapped golden the ids of the two routes are identical"
    assert got.sequences[0, p.shape[1]:].tolist() == gold[:NEW].tolist()
    other = m.generate(p, decode_weights="fp8", **dict(kw, use_graph=not use_graph))   # eager and replayed fp8 calls: bit-equal
    assert torch.equal(other.sequences, got.sequences) and torch.equal(torch.stack(other.logits), torch.stack(got.logits))
    plain = m.generate(p, decode_weights="fp8", **audio, max_new_tokens=NEW, use_graph=use_graph)   # no logits row is written: the partial (max, argmax) pairs alone
    assert torch.equal(plain, got.sequences)


def test_generate_fp8_composes_with_sampling_processors_and_a_passed_cache(dev, monkeypatch):
    m, p, audio, gold = _snapped(dev)
    names = _spy(monkeypatch)
    kw = dict(audio, max_new_tokens=8, do_sample=True, seed=5, top_k=8, repetition_penalty=1.3, **FLAGS)
    ref = m.generate(p, **kw)
    assert not any(n.endswith("_w8") for n in names)
    got = m.generate(p, decode_weights="fp8", **kw)
    assert names.count("afk_decode_chain_lm_head_w8") >= 2 and names.count("afk_decode_chain_qkv_w8") == m.dec_layers * names.count("afk_decode_chain_lm_head_w8")
    assert m.last_w8_stats is not None
    _hold_to_the_bf16_route("sampled + repetition_penalty", ref, got, p.shape[1], greedy=False)
    # a chat turn continued on the cache of the previous one: the suffix prefill is the bf16 launches, its n = 1 steps the fp8 ones
    full2 = torch.cat([p, gold[None, :8]], 1)
    turn1 = lambda: m.generate(p, max_new_tokens=5, return_dict_in_generate=True, **audio).past_key_values
    ref = m.generate(full2, past_key_values=turn1(), max_new_tokens=5, **FLAGS)
    names.clear()
    cache = turn1()
    assert not any(n.endswith("_w8") for n in names)
    got = m.generate(full2, past_key_values=cache, max_new_tokens=5, decode_weights="fp8", **FLAGS)
    assert names.count("afk_decode_chain_lm_head_w8") >= 2 and not any(n in BF16_NAMES for n in names[names.index("afk_decode_chain_qkv_w8"):])
    assert got.past_key_values is cache and cache.get_seq_length() == full2.shape[1] + 5 - 1
    first = _hold_to_the_bf16_route("past_key_values=", ref, got, full2.shape[1])
    assert first is None and got.sequences[0, full2.shape[1]:].tolist() == gold[8:13].tolist()


def test_launches_of_an_fp8_call_and_the_off_switch(dev, monkeypatch):
    m, p, audio, _ = _snapped(dev)
    L, n = m.dec_layers, 6
    m.drop_decode_weights()
    assert m._w8 is None
    names, marks = _spy(monkeypatch), []
    real_graph = torch.cuda.graph

    class Marking(real_graph):
        def __enter__(self):
            marks.append(len(names))
            return super().__enter__()

        def __exit__(self, *a):
            marks.append(len(names))
            return super().__exit__(*a)

    monkeypatch.setattr(torch.cuda, "graph", Marking)
    # the default call: no FP8 name, no FP8 copy
    base = m.generate(p, max_new_tokens=n, use_graph=False, **audio)
    default_names = list(names)
    assert not any(x.endswith("_w8") or x == "afk_quantize_rows_fp8" for x in names) and m._w8 is None and m.last_w8_stats is None
    assert names.count("afk_decode_chain_qkv") == L * (n - 1)
    # eager fp8 call of n tokens: every decode step is L x {1 qkv, 2 linear+residual, 1 gate|up} + 1 lm_head on the FP8 entries, none of the bf16 ones
    names.clear()
    eager = m.generate(p, max_new_tokens=n, use_graph=False, decode_weights="fp8", **audio)
    cnt = Counter(names)
    assert cnt["afk_quantize_rows_fp8"] == 4 * L + 1
    assert [cnt[x] for x in W8_NAMES] == [L * (n - 1), 2 * L * (n - 1), L * (n - 1), n - 1] and not any(cnt[x] for x in BF16_NAMES)
    first = lambda seq, which: min(seq.index(x) for x in which if x in seq)
    strip = lambda seq: [x for x in seq if x != "afk_quantize_rows_fp8"]
    assert strip(names)[:first(strip(names), W8_NAMES)] == default_names[:first(default_names, BF16_NAMES)], "the prefill is unchanged"
    assert torch.equal(eager, base)
    bytes8 = sum(q.codes.numel() + 4 * q.scale.numel() for lw in m._w8.layers for q in lw.values()) + m._w8.head.codes.numel() + 4 * m._w8.head.scale.numel()
    bytes16 = 2 * (sum(q.codes.numel() for lw in m._w8.layers for q in lw.values()) + m._w8.head.codes.numel())
    assert m.last_w8_stats == dict(tensors=4 * L + 1, bytes_fp8=bytes8, bytes_bf16=bytes16, rebuilt=True)
    assert m._w8.version == m.arena.version() and m._w8.head.codes.dtype == torch.uint8 and m._w8.head.scale.dtype == torch.float32
    # the captured step, exactly
    names.clear()
    replayed = m.generate(p, max_new_tokens=n, use_graph=True, decode_weights="fp8", **audio)
    assert len(marks) == 2 and torch.equal(replayed, eager)
    step = Counter(names[marks[0]:marks[1]])
    assert [step[x] for x in W8_NAMES] == [L, 2 * L, L, 1] and not any(step[x] for x in BF16_NAMES) and step["afk_attn_decode_fused"] == L
    assert "afk_quantize_rows_fp8" not in names and m.last_w8_stats["rebuilt"] is False
    # a default call afterwards: the copy stays, nothing reads it
    names.clear()
    assert torch.equal(m.generate(p, max_new_tokens=n, use_graph=False, **audio), base)
    assert not any(x.endswith("_w8") for x in names) and m.last_w8_stats is None and m._w8 is not None
    m.drop_decode_weights()
    assert m._w8 is None


def test_a_stale_copy_is_rebuilt(dev):
    from tests.test_model_gpu import G
    from tests.test_sampler_gpu import _case_a

    m, p, audio = _case_a(dev)
    _snap_in_place(m)
    kw = dict(audio, max_new_tokens=3, use_graph=False, **FLAGS)
    row = lambda out: out.logits[1].float()   # the first decode step's row: behind the same prefill and the same token 0 on every route
    first = m.generate(p, decode_weights="fp8", **kw)
    assert m.last_w8_stats["rebuilt"] is True
    assert m.generate(p, decode_weights="fp8", **kw) is not None and m.last_w8_stats["rebuilt"] is False
    # an in-place torch write: half the down projection's rows of the last layer change sign (still on the grid)
    m.arena[f"{m._lm}layers.{m.dec_layers - 1}.mlp.down_proj.weight"].data[::2].mul_(-1)
    ref = m.generate(p, **kw)
    got = m.generate(p, decode_weights="fp8", **kw)
    assert m.last_w8_stats["rebuilt"] is True
    bar = logit_tol(float(row(ref).abs().max()))
    assert torch.equal(got.logits[0], first.logits[0]) or float((got.logits[0].float() - ref.logits[0].float()).abs().max()) <= bar
    err, moved = float((row(got) - row(ref)).abs().max()), float((row(got) - row(first)).abs().max())
    print(f"in-place write: |fp8 - bf16| = {err:.4f} (bar {bar:.4f}); moved from the stale result by {moved:.4f}")
    assert err <= bar and moved > 4 * bar, "the logits follow the new weight"
    # load_state_dict, then the snap again: the model is the first one again, and so are the FP8 logits
    m.load_state_dict(torch.load(os.path.join(G, "tiny64_state_bf16.pt")))
    _snap_in_place(m)
    ref = m.generate(p, **kw)
    again = m.generate(p, decode_weights="fp8", **kw)
    assert m.last_w8_stats["rebuilt"] is True
    assert torch.equal(torch.stack(again.logits), torch.stack(first.logits)) and torch.equal(again.sequences, first.sequences)
    assert float((row(again) - row(ref)).abs().max()) <= logit_tol(float(row(ref).abs().max()))


def test_refused_combinations_name_themselves(dev, monkeypatch):
    from audio_flamingo_amd import exact
    from audio_flamingo_amd._lib import AfkError

    m, p, audio, _ = _snapped(dev)
    ids2 = torch.randint(0, 256, (2, 12), generator=torch.Generator().manual_seed(4)).to(dev)
    one = dict(audio, max_new_tokens=2, decode_weights="fp8")
    for kw, word in ((dict(num_beams=2), "num_beams > 1"), (dict(do_sample=True, num_return_sequences=2), "num_return_sequences > 1"),
                     (dict(guidance_scale=1.5), "guidance_scale"), (dict(prompt_lookup_num_tokens=3), "prompt_lookup_num_tokens"),
                     (dict(share_prompt=True), "share_prompt=True"), (dict(use_cache=False), "use_cache=False")):
        with pytest.raises(AfkError, match=word):
            m.generate(p, **one, **kw)
    with pytest.raises(AfkError, match="more than one row"):
        m.generate(ids2, max_new_tokens=2, decode_weights="fp8")
    with monkeypatch.context() as mp:
        mp.setattr(exact, "ENABLED", True)
        with pytest.raises(AfkError, match="AFK_EXACT_FP32=1"):
            m.generate(p, **one)
    with monkeypatch.context() as mp:
        mp.setattr(type(m), "decode_chain", False)
        with pytest.raises(AfkError, match="single-sequence decode chain"):
            m.generate(p, **one)
    with monkeypatch.context() as mp:
        mp.setattr(m, "I", 520)
        with pytest.raises(AfkError, match="multiple of 16"):
            m.generate(p, **one)
    with monkeypatch.context() as mp:
        blk = m.arena["lm_head.weight"]
        mp.setattr(blk, "data", blk.data[:1020])
        with pytest.raises(AfkError, match="multiple of 8"):
            m.generate(p, **one)
    for bad in ("int8", "FP8", 8):
        with pytest.raises(ValueError, match="decode_weights"):
            m.generate(p, **dict(one, decode_weights=bad))
    # the class attribute on: a two-row batch takes today's route, silently, and returns today's ids
    today = m.generate(ids2, max_new_tokens=4)
    with monkeypatch.context() as mp:
        mp.setattr(type(m), "decode_weight_dtype", "fp8")
        names = _spy(mp)
        assert torch.equal(m.generate(ids2, max_new_tokens=4), today) and m.last_w8_stats is None and not any(n.endswith("_w8") for n in names)
        assert torch.equal(m.generate(p, max_new_tokens=4, **audio), m.generate(p, max_new_tokens=4, decode_weights="fp8", **audio))
        assert m.last_w8_stats is not None and any(n.endswith("_w8") for n in names)

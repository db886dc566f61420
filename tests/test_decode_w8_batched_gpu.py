"""GPU: FP8 decode weights on the matrix-pipe decode chain, 1 .. 8 rows - the four afk_decode_chain_*_batched_w8 launches and
generate(decode_weights="fp8", decode_weights_batched=True).

Kernel level.  The integer operands of tests/_chain_ref.py make every rounding point exact, so each launch must return the integer reference with torch.equal,
whatever its K partition; the cases are R.grid()'s (K = 64 .. 4160: one block with seven idle slices, two blocks, 9 / 17 / 65 blocks - four of the five with
K % 128 == 64, where a 16-code load straddles the end of a row; every second case strided, the stride padding and the bytes between rows holding the code of
448).  The ternary weights would quantise to ONE scale for every row, so a scale taken from the wrong row would pass: the tests encode row r as
code = W * 2^(r % 7), scale = 2^-(r % 7) instead (decode_w8.quantize_rows patched; checked lossless on the CPU here and by _prepare on the device).  The gaussian
cases run on weights snapped onto the FP8 grid with rows scaled by 2^(r % 5 - 2), against the fp64 restatement at the project's bars.

Model level: the trained tiny golden (hidden 256, 4:2 heads of 64, I 512, V 1024 - the norm-in-prologue launches take it) with its decoder Linears and lm_head
snapped onto the FP8 grid (tests/test_decode_w8_gpu.py::_snapped), where the FP8 copy restates the weights without loss."""
from collections import Counter

import pytest
import torch

from tests import _chain_ref as R
from tests import _w8_ref as R8
from tests._tol import logit_tol
from tests.test_decode_chain_exact_gpu import BAR, BAR_GU, BF, EPS, F64, SENT, _cases, _full, _prepare
from tests.test_decode_w8_gpu import FLAGS, _snapped, _spy

pytestmark = pytest.mark.gpu

ENTRIES = ("qkv_norm_batched", "gate_up_norm_batched", "lm_head_norm_batched", "linear_residual_ss_batched")
MS = (1, 2, 3, 4, 5, 7, 8)
W8B = tuple("afk_decode_chain_" + e + "_w8" for e in ENTRIES)
TWINS = tuple(n[:-3] for n in W8B)


# ------------------------------------------------------------------------------------------------ kernel level
def _encode_per_row(w, name="weight"):
    """row r of an integer matrix as code = W * 2^(r % 7), scale = 2^-(r % 7): seven different scales among neighbouring rows, every code an e4m3fn value"""
    from audio_flamingo_amd import decode_w8

    e = (torch.arange(w.shape[0], device=w.device) % 7).to(torch.int32)
    codes = torch.ldexp(w.float(), e[:, None]).to(torch.float8_e4m3fn).view(torch.uint8)
    return decode_w8.Q8(codes.contiguous(), torch.ldexp(torch.ones_like(e, dtype=torch.float32), -e))


@pytest.fixture
def per_row_scales(monkeypatch):
    from audio_flamingo_amd import decode_w8

    monkeypatch.setattr(decode_w8, "quantize_rows", _encode_per_row)


def test_the_per_row_encoding_is_lossless_and_tells_rows_apart():
    """CPU arithmetic only: the encoding the integer tests feed the kernels restates {-1, 0, 1} weights exactly, with neighbouring rows on different scales"""
    c = R.make("lin", 2, 576, 7, N=64)
    q = _encode_per_row(c.W.to(BF))
    assert torch.equal(R8.dequantize(q.codes, q.scale, torch.float64), c.W), "code * scale must restate the weight"
    vals = q.codes.view(torch.float8_e4m3fn).float()
    assert float(vals.abs().max()) == 64.0 and torch.equal(vals.abs().amax(1), 2.0 ** (torch.arange(64) % 7).float())
    assert len(set(q.scale[:7].tolist())) == 7 and bool((q.scale[1:] != q.scale[:-1]).all())


@pytest.mark.parametrize("M", MS)
@pytest.mark.parametrize("entry", ENTRIES)
def test_batched_w8_entries_equal_the_integer_reference(dev, entry, M, per_row_scales):
    """every output with torch.equal, the sentinel outside the written slots, ss_part exact with zeros behind M (_prepare holds all three)"""
    cases = _cases(entry, M, dev, w8=True)
    assert len(cases) == 2 and all(c.K in R.K_MFMA for _, c, _ in cases)
    if entry == "lm_head_norm_batched" and M == 8:   # 1024 row groups and more: the shape at which the plain lm_head launch changes its form
        c = R.make("head", 8, 128, 4242, norm=True, N=32768)
        cases.append((f"{entry}_w8 M=8 K=128 N=32768", c, _prepare(entry, c, False, dev, w8=True)))
    for tag, c, go in cases:
        go(tag)


@pytest.mark.parametrize("M", (3, 8))
def test_ss_hand_over_between_the_w8_launches(dev, M, per_row_scales):
    """linear_residual_ss_batched_w8 leaves rows +-2^(m % 5) and their partial sums of squares; qkv / gate|up / lm_head _w8 take the rows as they lie, with
    ss_part and without: the same integer reference, hence the same bits"""
    ran = 0
    for tag, c, go in _cases("linear_residual_ss_batched", M, dev, w8=True):
        if not c.target:
            continue
        got = go(tag)
        rows = got["out"][:, :c.N]
        for entry, kw in (("qkv_norm_batched", dict(heads=(2, 1, 32))), ("gate_up_norm_batched", dict(I=16)), ("lm_head_norm_batched", dict(N=32))):
            cc = R.make(R.kind_of(entry), M, c.N, c.seed + 500, norm=True, rows=c.out_rows, s_e0=0, **kw)
            for ss in (None, (got["ss"], c.N // 16)):
                _prepare(entry, cc, False, dev, w8=True, x_dev=rows, ss=ss)(f"{tag} -> {entry}_w8 {'with' if ss else 'without'} ss_part")
                ran += 1
    assert ran == 6


@pytest.mark.parametrize("entry", ENTRIES)
def test_gaussian_weights_on_the_fp8_grid_with_scaled_rows(dev, entry):
    """M = 8, K = 576 (nine blocks: the last load of a row holds one block), gaussian rows and weights; the weights snapped onto the FP8 grid and row r scaled
    by 2^(r % 5 - 2), so the quantiser's own scales differ from row to row; against fp64 with bf16 roundings where the kernels round"""
    kind = R.kind_of(entry)
    kw = dict(qkv=dict(heads=(2, 1, 32)), lin=dict(N=192), gu=dict(I=48), head=dict(N=1056))[kind]
    c = R.gaussian(kind, 8, 576, 90 + ENTRIES.index(entry), (0, 576), norm=kind != "lin", **kw)
    rows = torch.arange(c.N)
    c.W = R8.snap(c.W.to(BF)).to(F64) * (2.0 ** ((rows % 5) - 2).to(F64))[:, None]
    assert len(set(R8.quantize(c.W.to(BF))[1][:5].tolist())) >= 3, "the rows must differ in their scales"
    _prepare(entry, c, False, dev, w8=True, tol=BAR_GU if kind == "gu" else BAR)(f"{entry}_w8 gaussian M=8 K=576 N={c.N}")


def _plain_args(entry, dev, M=2, K=64, ld_wq=None, scale=True):
    """a well-formed argument list of one entry at its smallest shape (x and the codes wide enough for every K the refusals try) -> (args, output buffers)"""
    from audio_flamingo_amd import ops

    st, KMAX = ops._stream(), 128
    Hq, Hkv, D = 2, 1, 32
    N = dict(qkv_norm_batched=(Hq + 2 * Hkv) * D, gate_up_norm_batched=64, lm_head_norm_batched=64, linear_residual_ss_batched=64)[entry]
    x = torch.zeros((9, KMAX), device=dev, dtype=BF)
    nw = torch.ones((KMAX,), device=dev, dtype=BF)
    codes = torch.zeros((N, KMAX + 16), device=dev, dtype=torch.uint8)
    sc = torch.ones((N,), device=dev, dtype=torch.float32)
    wa = (codes.data_ptr(), codes.stride(0) if ld_wq is None else ld_wq, sc.data_ptr() if scale else None)
    keep = [x, nw, codes, sc]
    if entry == "qkv_norm_batched":
        bias, tab = torch.zeros((N,), device=dev, dtype=BF), torch.zeros((4, D), device=dev, dtype=BF)
        pos, start = torch.zeros((9,), device=dev, dtype=torch.int32), torch.zeros((1,), device=dev, dtype=torch.int32)
        outs = [_full((9, Hq * D), dev), _full((9, 2 * Hkv * D), dev), _full((9, Hkv * D * 8), dev)]
        args = (x.data_ptr(), KMAX, M, nw.data_ptr(), EPS, *wa, K, bias.data_ptr(), tab.data_ptr(), tab.data_ptr(), pos.data_ptr(), outs[0].data_ptr(), Hq * D,
                outs[1].data_ptr(), 2 * Hkv * D, outs[2].data_ptr(), Hkv * D * 8, 8, start.data_ptr(), Hq, Hkv, D, None, 0, st)
        keep += [bias, tab, pos, start]
    elif entry == "gate_up_norm_batched":
        outs = [_full((9, N // 2), dev)]
        args = (x.data_ptr(), KMAX, M, nw.data_ptr(), EPS, *wa, N // 2, K, outs[0].data_ptr(), N // 2, None, 0, st)
    elif entry == "lm_head_norm_batched":
        outs = [_full((9, N), dev, torch.float32)]
        args = (x.data_ptr(), KMAX, M, nw.data_ptr(), EPS, *wa, N, K, outs[0].data_ptr(), N, None, 0, st)
    else:
        res = torch.zeros((9, N), device=dev, dtype=BF)
        outs = [_full((9, N), dev), _full((8, N // 16), dev, torch.float32)]
        args = (x.data_ptr(), KMAX, M, *wa, N, K, res.data_ptr(), N, outs[0].data_ptr(), N, outs[1].data_ptr(), st)
        keep.append(res)
    return args, outs, keep


@pytest.mark.parametrize("entry", ENTRIES)
def test_batched_w8_entries_refuse_bad_arguments_without_a_launch(dev, entry):
    from audio_flamingo_amd import _lib
    from audio_flamingo_amd._lib import AfkError

    name = "afk_decode_chain_" + entry + "_w8"
    args, outs, keep = _plain_args(entry, dev)
    _lib.call(name, *args)   # the well-formed call runs (zero codes: it writes zeros, or the bias)
    torch.cuda.synchronize()
    assert all(bool((o != SENT).any()) for o in outs)
    for what, kw in (("M = 9", dict(M=9)), ("K = 96", dict(K=96)), ("ld_wq = K + 8", dict(ld_wq=64 + 8)), ("a null scale", dict(scale=False))):
        args, outs, keep = _plain_args(entry, dev, **kw)
        with pytest.raises(AfkError, match=name):
            _lib.call(name, *args)
        torch.cuda.synchronize()
        assert all(bool((o == SENT).all()) for o in outs), f"{name} with {what} wrote something"


# ------------------------------------------------------------------------------------------------ model level
NEW = 12
ON = dict(decode_weights="fp8", decode_weights_batched=True)


def _twice(p, audio):
    return p.repeat(2, 1), {k: v.repeat(2, *([1] * (v.dim() - 1))) for k, v in audio.items()}


def _hold_rows(tag, ref, got, S0):
    """_hold_to_the_bf16_route's rule for a call of several rows: every row's logits within the logit bar up to and including the first step at which any id
    differs -> that step, or None"""
    assert got.sequences.shape == ref.sequences.shape and len(got.logits) == len(ref.logits)
    diff = (ref.sequences[:, S0:] != got.sequences[:, S0:]).any(0).nonzero().flatten().tolist()
    first = diff[0] if diff else None
    worst = 0.0
    for t in range(len(ref.logits) if first is None else first + 1):
        r, g = ref.logits[t].float(), got.logits[t].float()
        assert tuple(g.shape) == tuple(r.shape)
        err, bar = float((g - r).abs().max()), logit_tol(float(r.abs().max()))
        worst = max(worst, err / bar)
        assert err <= bar, f"{tag}: step {t} logits differ by {err:.4f}, bar {bar:.4f}"
    print(f"{tag}: worst |fp8 - bf16| logit = {worst:.3f} x the bar; ids part at {first}")
    return first


@pytest.mark.parametrize("use_graph", [False, True])
def test_a_batch_of_two_equals_the_golden_and_the_single_sequence_route(dev, use_graph):
    m, p, audio, gold = _snapped(dev)
    p2, audio2 = _twice(p, audio)
    S0 = p.shape[1]
    kw = dict(audio2, max_new_tokens=NEW, use_graph=use_graph, **FLAGS)
    ref = m.generate(p2, **kw)
    assert m.last_w8_stats is None
    got = m.generate(p2, **ON, **kw)
    assert m.last_w8_stats is not None and m.last_w8_stats["tensors"] == 4 * m.dec_layers + 1
    first = _hold_rows(f"batch of two, use_graph={use_graph}", ref, got, S0)
    one = m.generate(p, decode_weights="fp8", max_new_tokens=NEW, use_graph=use_graph, **audio)
    for row in (0, 1):   # the top-1 / top-2 gap of these positions is 6.3 .. 15.9 x the logit bar (tests/test_decode_w8_gpu.py): the ids cannot part
        assert got.sequences[row, S0:].tolist() == gold[:NEW].tolist() == one[0, S0:].tolist()
    assert first is None and torch.equal(got.sequences, ref.sequences)


def test_prompt_lookup_on_the_fp8_copy_gives_the_greedy_ids(dev, monkeypatch):
    m, p, audio, gold = _snapped(dev)
    names = _spy(monkeypatch)
    plain = m.generate(p, decode_weights="fp8", max_new_tokens=NEW, **audio)
    names.clear()
    got = m.generate(p, prompt_lookup_num_tokens=3, max_new_tokens=NEW, **ON, **audio)
    assert torch.equal(got, plain) and got[0, p.shape[1]:].tolist() == gold[:NEW].tolist()
    cnt = Counter(names)
    steps = cnt["afk_decode_chain_lm_head_norm_batched_w8"]
    assert steps >= 1 and cnt["afk_decode_chain_qkv_norm_batched_w8"] == m.dec_layers * steps and not any(cnt[n] for n in TWINS)
    assert m.last_w8_stats is not None


@pytest.mark.parametrize("what,kw,flags", [
    ("sampled copies", dict(do_sample=True, num_return_sequences=2, seed=11, top_k=8), True),
    ("guidance", dict(guidance_scale=1.5), True),
    ("shared prompt", dict(do_sample=True, num_return_sequences=2, seed=11, top_k=8, share_prompt=True), True),
    ("beams", dict(num_beams=2), False), ("host beams", dict(num_beams=2), False)], ids=["copies", "guidance", "share_prompt", "beams", "host_beams"])
def test_the_other_batched_routes_hold_to_their_bf16_calls(dev, what, kw, flags, monkeypatch):
    """beams return no output object (generate() refuses it there).  Their check is on the ids: the FP8 launches keep the bf16 kernels' K partition, so on
    weights the copy restates without loss every sum - and with it every id - is the bf16 route's"""
    m, p, audio, _ = _snapped(dev)
    names = _spy(monkeypatch)
    if what == "host beams":   # the torch loop over [B, nb * V] in place of afk_beam_step
        monkeypatch.setattr(type(m), "beam_on_device", False)
    call = dict(audio, max_new_tokens=8, **kw, **(FLAGS if flags else {}))
    ref = m.generate(p, **call)
    assert not any(n.endswith("_w8") for n in names) and m.last_w8_stats is None
    names.clear()
    got = m.generate(p, **ON, **call)
    cnt = Counter(names)
    assert cnt["afk_decode_chain_lm_head_norm_batched_w8"] >= 2 and not any(cnt[n] for n in TWINS), what
    assert cnt["afk_attn_decode_shared" if "share_prompt" in kw else "afk_attn_decode_fused"] == m.dec_layers * cnt["afk_decode_chain_lm_head_norm_batched_w8"]
    assert m.last_w8_stats is not None and (cnt["afk_beam_step"] > 0) == (what == "beams")
    if flags:
        _hold_rows(what, ref, got, p.shape[1])
    else:
        assert torch.equal(got, ref), what


def test_launches_with_the_switch_on_and_off(dev, monkeypatch):
    from audio_flamingo_amd._lib import AfkError

    m, p, audio, _ = _snapped(dev)
    p2, audio2 = _twice(p, audio)
    L, n = m.dec_layers, 5
    names = _spy(monkeypatch)
    kw = dict(audio2, max_new_tokens=n, use_graph=False)
    base = m.generate(p2, **kw)
    default_names = list(names)
    assert not any(x.endswith("_w8") for x in names) and [names.count(x) for x in TWINS] == [L * (n - 1), L * (n - 1), n - 1, 2 * L * (n - 1)]
    # the switch off, spelled or not: the same launches; "fp8" alone still refuses two rows
    names.clear()
    assert torch.equal(m.generate(p2, decode_weights_batched=False, **kw), base) and names == default_names
    names.clear()
    assert torch.equal(m.generate(p2, decode_weights_batched=True, **kw), base) and names == default_names and m.last_w8_stats is None   # nothing to apply it to
    with pytest.raises(AfkError, match="more than one row"):
        m.generate(p2, decode_weights="fp8", **kw)
    with pytest.raises(AfkError, match="more than one row"):
        m.generate(p2, decode_weights="fp8", decode_weights_batched=False, **kw)
    # on: per decode step and layer the four FP8 names in place of their twins, nothing else moved
    m.drop_decode_weights()
    names.clear()
    got = m.generate(p2, **ON, **kw)
    cnt = Counter(names)
    assert [cnt[x] for x in W8B] == [L * (n - 1), L * (n - 1), n - 1, 2 * L * (n - 1)] and not any(cnt[x] for x in TWINS)
    assert cnt["afk_quantize_rows_fp8"] == 4 * L + 1 and m.last_w8_stats is not None and m.last_w8_stats["rebuilt"] is True
    assert [x[:-3] if x in W8B else x for x in names if x != "afk_quantize_rows_fp8"] == default_names
    assert torch.equal(got, base)
    layer = [x for x in names if x in W8B or x == "afk_attn_decode_fused"][:5]
    assert layer == [W8B[0], "afk_attn_decode_fused", W8B[3], W8B[1], W8B[3]]
    # the class attributes in place of the keywords
    with monkeypatch.context() as mp:
        mp.setattr(type(m), "decode_weight_dtype", "fp8")
        names.clear()
        assert torch.equal(m.generate(p2, **kw), base) and names == default_names and m.last_w8_stats is None   # today's convention: two rows, silently bf16
        mp.setattr(type(m), "decode_weights_batched", True)
        names.clear()
        assert torch.equal(m.generate(p2, **kw), base) and Counter(names)[W8B[0]] == L * (n - 1) and m.last_w8_stats["rebuilt"] is False


def test_nine_rows_are_refused_by_name_or_take_the_bf16_route(dev, monkeypatch):
    from audio_flamingo_amd._lib import AfkError

    m, p, audio, _ = _snapped(dev)
    ids9 = torch.randint(0, 256, (9, 12), generator=torch.Generator().manual_seed(9)).to(dev)
    with pytest.raises(AfkError, match="9 rows in a decode step"):
        m.generate(ids9, max_new_tokens=3, **ON)
    today = m.generate(ids9, max_new_tokens=3)
    with monkeypatch.context() as mp:
        mp.setattr(type(m), "decode_weight_dtype", "fp8")
        mp.setattr(type(m), "decode_weights_batched", True)
        names = _spy(mp)
        assert torch.equal(m.generate(ids9, max_new_tokens=3), today) and m.last_w8_stats is None and not any(x.endswith("_w8") for x in names)

"""GPU: steps 3a-3d of afk_decode_sample_filtered (csrc/decode_sample.hip: min_p, typical_p, epsilon_cutoff, eta_cutoff behind top-p) against the fp64
restatement tests/_warpers_ref.py, and generate() with the four keywords.  The logits are bf16-valued fp32 - what the lm_head produces.

Bounds: the kept set and its size are exact.  Every parameter is snapped per row into the middle of a gap of the reference's own statistic, and the gap is
asserted (tests/_warpers_ref.py: relative half-gap >= 1e-4 for the min_p / epsilon / eta floors, mass half-gap >= 5e-5 and d separation >= 5e-5 for typical_p,
half-gap >= 5e-5 for top-p), so that fp32 exp / log / summation error (~1e-5 relative) cannot decide a case; a case that misses its gap is skipped and at most
5 % of a test's cases may be.  Probabilities: |r - r_ref| <= 1e-4 r_ref where r_ref >= 1e-6 (the bound of test_sampler_gpu.py, for the same reason: fp32 exp
of an argument up to ~40 is good to ~1e-5 relative)."""
import functools
import os

import numpy as np
import pytest
import torch

from tests import _sampler_ref as R
from tests import _warpers_ref as W

pytestmark = pytest.mark.gpu

VS, SCALES, TEMPS, ROWS = (1, 37, 1000, 9001, 152064), (1.0, 4.0), (0.7, 1.0, 1.3), 3
TARGETS = dict(min_p=(0.05, 0.3), typical_p=(0.2, 0.9), epsilon_cutoff=(3e-4, 2e-2), eta_cutoff=(3e-4, 2e-2))
FILTERS = tuple(TARGETS)
# (top_k, top-p target, filters): each filter alone, behind top-k = 50, behind a snapped top-p, and the full chain
COMBOS = [(k, p, (f,)) for k, p in ((0, 1.0), (50, 1.0), (0, 0.9)) for f in FILTERS] + [(50, 0.9, FILTERS)]
HALF_GAP = 5e-5
U_LAST = 1.0 - 2.0 ** -24


@functools.lru_cache(maxsize=None)
def _logits(V, scale):
    return torch.stack([R.bf16_logits(V, scale, seed=1000 * b + V % 997 + int(scale)) for b in range(ROWS)])


@functools.lru_cache(maxsize=None)
def _row(V, scale, b, T):
    return R.Row(_logits(V, scale)[b], T)


def _snapped(V, scale, b, T, k, p, targets):
    """-> (Chain applied, keywords of ops.decode_sample for this row, every gap met)"""
    top_p, half = 1.0, np.inf
    if p < 1.0:
        top_p, half = _row(V, scale, b, T).snap_top_p(k, p)
    chain, kw, ok = W.snap_chain(_row(V, scale, b, T), k, top_p, targets)
    return chain, dict(kw, temperature=T, top_k=k, top_p=top_p), ok and half >= HALF_GAP


def _sample(dev, x, rows=None, **kw):
    """-> tokens [B], probs (of `rows`, default all), kept [B]"""
    from audio_flamingo_amd import ops

    B, V = x.shape
    probs = torch.full((B, V), -1.0, device=dev)
    kept = torch.full((B,), -1, device=dev, dtype=torch.int32)
    if kw.get("u") is not None and not torch.is_tensor(kw["u"]):
        kw["u"] = torch.tensor(kw["u"], dtype=torch.float32, device=dev)
    tok = ops.decode_sample(x, probs_out=probs, kept_out=kept, **kw)
    return tok.cpu().numpy(), (probs if rows is None else probs[rows]).cpu().numpy(), kept.cpu().numpy()


def _few_skipped(cases, skipped):
    assert cases > 0 and skipped <= 0.05 * cases, (skipped, cases)


@pytest.mark.parametrize("scale", SCALES)
@pytest.mark.parametrize("V", VS)
def test_kept_set_and_probabilities(dev, V, scale):
    x = _logits(V, scale).to(dev)
    cases = skipped = 0
    for T in TEMPS:
        for ci, (k, p, combo) in enumerate(COMBOS):
            for b in range(ROWS):      # the parameters are snapped per row: one launch of all rows per row's values; both targets of a filter over the rows
                cases += 1
                chain, kw, ok = _snapped(V, scale, b, T, k, p, {f: TARGETS[f][(b + ci) % 2] for f in combo})
                if not ok:
                    skipped += 1
                    continue
                ref = chain.result()
                _, probs, kept = _sample(dev, x, rows=b, u=[0.5] * ROWS, **kw)
                tag = (V, scale, T, k, p, combo, b, kw, ref["margins"])
                assert np.array_equal(probs > 0, ref["keep"]), (tag, int((probs > 0).sum()), int(ref["keep"].sum()))
                assert int(kept[b]) == int(ref["keep"].sum()), tag
                big = ref["r"] >= 1e-6
                err = np.abs(probs.astype(np.float64) - ref["r"])[big] / ref["r"][big]
                assert err.max() <= 1e-4, (tag, float(err.max()))
    _few_skipped(cases, skipped)


def _draw_us(ref):
    """the u values of test_sampler_gpu's draw test: the middle of the cdf interval of the likeliest, the least likely, the first and the last of the tokens
    with r >= 1e-3, then 0 and the largest u"""
    likely = np.nonzero(ref["keep"] & (ref["r"] >= 1e-3))[0]
    assert likely.size
    want = sorted({int(likely[np.argmax(ref["r"][likely])]), int(likely[np.argmin(ref["r"][likely])]), int(likely[0]), int(likely[-1])})
    return want, [float(ref["cdf"][i] - 0.5 * ref["r"][i]) for i in want] + [0.0, U_LAST]


@pytest.mark.parametrize("V", VS)
def test_draw_hits_the_token_whose_cdf_interval_holds_u(dev, V):
    scale = 4.0
    cases = skipped = 0
    for T in TEMPS:
        for ci, (k, p, combo) in enumerate(COMBOS):
            b = ci % ROWS
            cases += 1
            chain, kw, ok = _snapped(V, scale, b, T, k, p, {f: TARGETS[f][ci % 2] for f in combo})
            if not ok:
                skipped += 1
                continue
            ref = chain.result()
            want, us = _draw_us(ref)
            x = _logits(V, scale)[b].to(dev).expand(len(us), V).contiguous()
            tok, _, _ = _sample(dev, x, rows=0, u=us, **kw)
            tag = (V, T, k, p, combo, b)
            assert tok[: len(want)].tolist() == want, tag
            assert int(tok[-2]) == int(np.nonzero(ref["keep"])[0][0]), tag          # u = 0: the lowest kept id
            assert ref["keep"][int(tok[-1])], tag
    _few_skipped(cases, skipped)


def test_draw_from_a_typical_band_that_excludes_the_row_maximum(dev):
    """typical_p keeps the tokens nearest the entropy: on these rows the likeliest token is outside, the kept set is a band in z, and the draw has to hit
    the tokens at both of its edges"""
    bands = 0
    for V, scale, k in ((37, 1.0, 0), (1000, 1.0, 50), (152064, 1.0, 50), (152064, 4.0, 50)):
        for b in range(ROWS):
            T = TEMPS[b]
            row = _row(V, scale, b, T)
            chain, kw, ok = _snapped(V, scale, b, T, k, 1.0, dict(typical_p=0.2))
            ref = chain.result()
            top = int(np.argmax(row.z))
            if not ok or ref["keep"][top]:
                continue
            bands += 1
            ids = np.nonzero(ref["keep"])[0]
            hi, lo = int(ids[np.argmax(row.z[ids])]), int(ids[np.argmin(row.z[ids])])     # the band's edges (the lowest id of each edge class)
            assert row.z[hi] < row.z[top] and ref["r"][lo] >= 1e-3
            want = sorted({hi, lo, int(ids[0]), int(ids[-1])})
            us = [float(ref["cdf"][i] - 0.5 * ref["r"][i]) for i in want] + [0.0, U_LAST]
            x = _logits(V, scale)[b].to(dev).expand(len(us), V).contiguous()
            tok, probs, kept = _sample(dev, x, rows=0, u=us, **kw)
            tag = (V, scale, b, T, k, kw)
            assert np.array_equal(probs > 0, ref["keep"]) and probs[top] == 0.0 and int(kept[0]) == ids.size, tag
            assert tok[: len(want)].tolist() == want, tag
            assert int(tok[-2]) == int(ids[0]) and ref["keep"][int(tok[-1])], tag
    assert bands >= 6, bands


@pytest.mark.parametrize("V", VS)
def test_filters_off_is_afk_decode_sample_bit_for_bit(dev, V):
    """ops.decode_sample goes through afk_decode_sample_filtered; with the four at their off values (and at other inactive values) it answers what
    afk_decode_sample answers on the top-k / top-p grid: tokens, probabilities, kept counts"""
    from audio_flamingo_amd import _lib, ops

    x = _logits(V, 4.0).to(dev)
    u = torch.tensor([0.1, 0.5, 0.93], device=dev)
    for T in TEMPS:
        for k in (0, 50, 1000):
            for p in (1.0, 0.9, 0.5):
                old_tok, old_kept = torch.zeros(ROWS, dtype=torch.int64, device=dev), torch.zeros(ROWS, dtype=torch.int32, device=dev)
                old_probs = torch.full((ROWS, V), -1.0, device=dev)
                _lib.call("afk_decode_sample", x.data_ptr(), x.stride(0), ROWS, V, T, k, p, u.data_ptr(), 0, None, 0, old_tok.data_ptr(), old_probs.data_ptr(),
                          old_probs.stride(0), old_kept.data_ptr(), None, 0, None, None, 0, 0, None, ops._stream())
                for off in (dict(), dict(min_p=0.0, typical_p=1.0, epsilon_cutoff=0.0, eta_cutoff=0.0), dict(min_p=-1.0, typical_p=2.0, epsilon_cutoff=1.0, eta_cutoff=-3.0)):
                    probs, kept = torch.full((ROWS, V), -1.0, device=dev), torch.zeros(ROWS, dtype=torch.int32, device=dev)
                    tok = ops.decode_sample(x, temperature=T, top_k=k, top_p=p, u=u, probs_out=probs, kept_out=kept, **off)
                    assert torch.equal(tok, old_tok) and torch.equal(kept, old_kept) and torch.equal(probs, old_probs), (V, T, k, p, off)


def test_edge_rows(dev):
    V = 1000
    allon = dict(min_p=0.05, typical_p=0.9, epsilon_cutoff=3e-4, eta_cutoff=3e-4)
    # one +inf (and two: the lowest index), whatever the filters; no finite logit: 0, as torch.argmax answers
    y = R.bf16_logits(V, 4.0, seed=6)
    y[613] = float("inf")
    z = y.clone()
    z[77] = float("inf")
    for kw in (allon, dict(allon, temperature=0.7, top_k=50, top_p=0.9), dict(typical_p=0.2), dict(min_p=1.0)):
        tok, probs, kept = _sample(dev, torch.stack([y, z]).to(dev), u=[0.3, 0.9], **kw)
        assert tok.tolist() == [613, 77] and kept.tolist() == [1, 1]
        assert probs[0, 613] == 1.0 and probs[1, 77] == 1.0 and probs.sum() == 2.0
    w = torch.full((2, V), float("-inf"))
    w[1, 3::5] = float("nan")
    for kw in (allon, dict(allon, top_k=50, top_p=0.9), dict(typical_p=0.2)):
        tok, probs, kept = _sample(dev, w.to(dev), u=[0.3, 0.9], **kw)
        assert tok.tolist() == [0, 0] and kept.tolist() == [0, 0] and not probs.any()
    # -inf and NaN entries are never kept and never drawn, with every filter in front of the draw
    x = R.bf16_logits(V, 4.0, seed=5)
    x[::2] = float("-inf")
    x[1::7] = float("nan")
    row = R.Row(x, 1.0)
    chain, kw, ok = W.snap_chain(row, 0, 1.0, {f: TARGETS[f][0] for f in FILTERS})
    assert ok
    ref = chain.result()
    us = np.linspace(0.0, U_LAST, 64).astype(np.float32)
    tok, probs, kept = _sample(dev, x.to(dev).expand(64, V).contiguous(), u=us.tolist(), **kw)
    assert ref["keep"][tok].all() and np.isfinite(x.numpy()[tok]).all()
    assert np.array_equal(probs[0] > 0, ref["keep"]) and int(kept[0]) == int(ref["keep"].sum())
    # min_p = 1: exactly the ties with the maximum stay (bf16-valued rows have them; here three are planted)
    t = R.bf16_logits(V, 1.0, seed=9)
    t[[5, 500, 999]] = float(t.max()) + 1.0
    for T in TEMPS:
        tok, probs, kept = _sample(dev, t[None].to(dev).expand(3, V).contiguous(), u=[0.0, 0.5, U_LAST], temperature=T, min_p=1.0)
        assert tok.tolist() == [5, 500, 999] and kept.tolist() == [3, 3, 3] and np.nonzero(probs[0])[0].tolist() == [5, 500, 999]
        assert np.abs(probs[0][[5, 500, 999]] - 1.0 / 3.0).max() <= 1e-6
    # a typical_p so small that one class stays: the one nearest the entropy; an epsilon above every probability: the top class stays
    s = R.bf16_logits(V, 1.0, seed=10)
    for T in TEMPS:
        ref = W.reference(s, T, typical_p=1e-6)
        assert np.unique(R.Row(s, T).z[ref["keep"]]).size == 1 and ref["margins"]["typical_d"] >= W.D_GAP
        _, probs, kept = _sample(dev, s[None].to(dev), u=[0.5], temperature=T, typical_p=1e-6)
        assert np.array_equal(probs[0] > 0, ref["keep"]) and int(kept[0]) == int(ref["keep"].sum())
        ref = W.reference(s, T, epsilon_cutoff=0.999)
        assert np.array_equal(ref["keep"], R.Row(s, T).z == R.Row(s, T).z.max())
        tok, probs, kept = _sample(dev, s[None].to(dev), u=[0.5], temperature=T, epsilon_cutoff=0.999)
        assert np.array_equal(probs[0] > 0, ref["keep"]) and int(kept[0]) == int(ref["keep"].sum()) and ref["keep"][int(tok[0])]


def test_single_sequence_bookkeeping_with_filters_equals_the_unfused_sequence(dev):
    """B = 1 with the state block and the filters active: the token of the plain launch, then tokens_out[state[2] + tok_off], state and x_out exactly as
    afk_decode_select_greedy leaves them for that token"""
    from audio_flamingo_amd import _lib, ops

    V, H, S0, seed = 1000, 64, 40, 99
    x = R.bf16_logits(V, 1.0, seed=8)
    chain, kw, ok = W.snap_chain(R.Row(x, 1.0), 50, 1.0, dict(min_p=0.3, typical_p=0.9, epsilon_cutoff=2e-2, eta_cutoff=2e-2))
    assert ok
    ref = chain.result()
    emb = torch.randn(V, H, generator=torch.Generator().manual_seed(1)).to(torch.bfloat16).to(dev)
    state0 = torch.tensor([0, S0 + 6, S0 + 5, S0 + 5], dtype=torch.int32)
    tok_off = 1 - S0                                  # token number t = state[2] + tok_off = 6
    u = R.uniform(seed, 6, 0)
    assert np.abs(ref["cdf"][ref["keep"]] - u).min() > 1e-4
    want = R.draw(ref, u)
    xd = x[None].to(dev)
    plain = ops.decode_sample(xd, top_k=50, seed=seed, step_off=6, **kw)           # the unfused launch: draw 6, no bookkeeping
    st = state0.to(dev)
    toks, x_out = torch.zeros(16, dtype=torch.int64, device=dev), torch.zeros(H, dtype=torch.bfloat16, device=dev)
    nxt = ops.decode_sample(xd, top_k=50, seed=seed, step_base=st[2:3], step_off=tok_off, tokens_out=toks, tok_off=tok_off, state=st, emb=emb, x_out=x_out, **kw)
    assert int(nxt[0]) == want == int(plain[0])
    y = x.clone()                                     # the greedy launch on logits whose argmax is that token
    y[want] = 100.0
    pv, pi = y.view(V // 8, 8).max(-1)
    pv, pi = pv.to(dev), (pi + 8 * torch.arange(V // 8)).to(torch.int32).to(dev)
    st2, toks2, x2, nxt2 = state0.to(dev), torch.zeros_like(toks), torch.zeros_like(x_out), torch.zeros(1, dtype=torch.int64, device=dev)
    _lib.call("afk_decode_select_greedy", pv.data_ptr(), pi.data_ptr(), V // 8, nxt2.data_ptr(), toks2.data_ptr(), tok_off, st2.data_ptr(), emb.data_ptr(),
              emb.stride(0), H, x2.data_ptr(), ops._stream())
    assert torch.equal(nxt, nxt2) and torch.equal(toks, toks2) and int(toks[6]) == want and torch.equal(st, st2) and torch.equal(x_out, x2)
    assert st.tolist() == [0, S0 + 7, S0 + 6, S0 + 6] and torch.equal(x_out, emb[want])


# ---------------------------------------------------------------------------------------------- generate() with the four keywords
BASE = dict(do_sample=True, temperature=1.5, top_k=20, top_p=0.95, seed=0xFEED_0000_0007, max_new_tokens=12)
WARPED = (dict(min_p=0.05), dict(typical_p=0.6, eta_cutoff=0.01))


class _Collect:
    def __init__(self):
        self.chunks = []

    def put(self, v):
        self.chunks.append(v.clone())

    def end(self):
        pass


def _case_a(dev):
    from tests.test_model_gpu import G, _gen_prompt, _model

    g = torch.load(os.path.join(G, "tiny64_caseA.pt"))
    return _model(dev), _gen_prompt(g).to(dev), dict(input_features=g["feats"][:1].to(dev), input_features_mask=g["fmask"][:1].to(dev))


@pytest.mark.parametrize("warp", WARPED, ids=lambda w: "+".join(w))
def test_generate_one_seed_one_sequence_of_ids_eager_graphed_and_streamed(dev, warp):
    m, p, audio = _case_a(dev)
    kw = dict(BASE, **warp)
    runs = [m.generate(p, use_graph=False, **audio, **kw), m.generate(p, use_graph=True, **audio, **kw), m.generate(p, streamer=_Collect(), **audio, **kw)]
    assert runs[0].shape[1] == p.shape[1] + 12 and torch.equal(runs[0], runs[1]) and torch.equal(runs[0], runs[2])
    # a left-padded batch of three
    g = torch.Generator().manual_seed(3)
    lens = (40, 23, 31)
    ids, att = torch.zeros((3, 40), dtype=torch.long), torch.zeros((3, 40), dtype=torch.long)
    for i, n in enumerate(lens):
        ids[i, 40 - n:] = torch.randint(0, 256, (n,), generator=g)
        att[i, 40 - n:] = 1
    kw = dict(attention_mask=att.to(dev), **kw)
    runs = [m.generate(ids.to(dev), use_graph=False, **kw), m.generate(ids.to(dev), use_graph=True, **kw), m.generate(ids.to(dev), streamer=_Collect(), **kw)]
    assert runs[0].shape == (3, 52) and torch.equal(runs[0], runs[1]) and torch.equal(runs[0], runs[2])


@pytest.mark.parametrize("warp", WARPED, ids=lambda w: "+".join(w))
def test_generate_samples_inside_one_captured_graph_without_torch_selection(dev, monkeypatch, warp):
    m, p, audio = _case_a(dev)

    def refuse(*a, **k):
        raise AssertionError("token selection went through torch")

    for owner in (torch, torch.Tensor):
        monkeypatch.setattr(owner, "multinomial", refuse)
        monkeypatch.setattr(owner, "sort", refuse)
    captured = []
    real = torch.cuda.graph

    class Counting(real):
        def __init__(self, *a, **k):
            captured.append(1)
            super().__init__(*a, **k)

    monkeypatch.setattr(torch.cuda, "graph", Counting)
    out = m.generate(p, **audio, **dict(BASE, **warp))
    assert out.shape[1] == p.shape[1] + 12 and len(captured) == 1


@pytest.mark.parametrize("warp", WARPED, ids=lambda w: "+".join(w))
def test_generate_sampled_ids_lie_in_the_reference_kept_set(dev, monkeypatch, warp):
    """the logits every draw of a no-graph run saw are recorded at ops.decode_sample; the graphed run's ids (equal to that run's) lie in the kept set the
    restatement computes from them.  A step whose logits put a parameter closer to a decision than the snapping gaps is not judged."""
    from audio_flamingo_amd import ops

    m, p, audio = _case_a(dev)
    kw = dict(BASE, **warp)
    seen, real = [], ops.decode_sample

    def recording(logits, **k):
        seen.append((logits.detach().float().cpu().clone(), {n: k[n] for n in ("temperature", "top_k", "top_p") + FILTERS}))
        return real(logits, **k)

    monkeypatch.setattr(ops, "decode_sample", recording)
    eager = m.generate(p, use_graph=False, **audio, **kw)
    monkeypatch.setattr(ops, "decode_sample", real)
    out = m.generate(p, **audio, **kw)
    assert torch.equal(out, eager) and len(seen) == 12
    S0, checked = p.shape[1], 0
    floor = dict(top_p=HALF_GAP, min_p=W.REL_GAP, typical_mass=W.MASS_GAP, typical_d=W.D_GAP, epsilon=W.REL_GAP, eta=W.REL_GAP)
    for t, (lg, params) in enumerate(seen):
        assert {f: params[f] for f in warp} == warp
        ref = W.reference(lg[0], params["temperature"], params["top_k"], params["top_p"], *(params[f] for f in FILTERS))
        if any(v < floor[n] for n, v in ref["margins"].items()):
            continue
        checked += 1
        assert ref["keep"][int(out[0, S0 + t])], (t, int(out[0, S0 + t]))
    assert checked >= 6


def test_generate_takes_min_p_from_the_generation_config(dev):
    from types import SimpleNamespace

    m, p, audio = _case_a(dev)
    by_keyword = m.generate(p, min_p=0.5, **audio, **BASE)
    by_config = m.generate(p, generation_config=SimpleNamespace(min_p=0.5), **audio, **BASE)
    plain = m.generate(p, **audio, **BASE)
    assert torch.equal(by_keyword, by_config)
    assert not torch.equal(by_keyword, plain), "min_p = 0.5 over 20 tokens at temperature 1.5 removes tokens the plain run draws"
    greedy = m.generate(p, do_sample=False, max_new_tokens=12, **audio)
    assert torch.equal(m.generate(p, do_sample=False, max_new_tokens=12, min_p=0.3, typical_p=0.5, epsilon_cutoff=0.1, eta_cutoff=0.1, **audio), greedy)

"""GPU: afk_decode_sample (csrc/decode_sample.hip) against the fp64 restatement of its contract (tests/_sampler_ref.py), and generate(do_sample=True)
on it.  The logits are bf16-valued fp32 - what the lm_head produces - so classes of equal values are the rule.

Bounds: the kept set and its size are exact; top-p cases have 1 - top_p snapped to the midpoint between two adjacent class cumulative masses of the
reference with a half-gap >= 5e-5 (asserted), so that fp32 exp / summation error (~1e-5 relative) cannot decide a case; probabilities
|r - r_ref| <= 1e-4 r_ref where r_ref >= 1e-6 (fp32 exp of an argument up to ~40 is good to ~1e-5 relative: one decade of margin)."""
import functools
import os

import numpy as np
import pytest
import torch

from tests import _sampler_ref as R

pytestmark = pytest.mark.gpu

VS, SCALES, TEMPS, KS, PS, ROWS = (1, 37, 1000, 152064), (1.0, 4.0), (0.7, 1.0, 1.3), (0, 50, 1000), (1.0, 0.9, 0.5), 3
HALF_GAP = 5e-5
U_LAST = 1.0 - 2.0 ** -24


@functools.lru_cache(maxsize=None)
def _logits(V, scale):
    return torch.stack([R.bf16_logits(V, scale, seed=1000 * b + V % 997 + int(scale)) for b in range(ROWS)])


@functools.lru_cache(maxsize=None)
def _row(V, scale, b, T):
    return R.Row(_logits(V, scale)[b], T)


def _snapped(V, scale, b, T, k, p):
    """-> top_p for this row (1 - top_p in the middle of a gap of the reference's class cumulative masses)"""
    if p >= 1.0:
        return 1.0
    top_p, half = _row(V, scale, b, T).snap_top_p(k, p)
    assert half >= HALF_GAP, (V, scale, b, T, k, p, half)
    return top_p


def _sample(dev, x, **kw):
    from audio_flamingo_amd import ops

    B, V = x.shape
    probs = torch.full((B, V), -1.0, device=dev)
    kept = torch.full((B,), -1, device=dev, dtype=torch.int32)
    if kw.get("u") is not None and not torch.is_tensor(kw["u"]):
        kw["u"] = torch.tensor(kw["u"], dtype=torch.float32, device=dev)
    tok = ops.decode_sample(x, probs_out=probs, kept_out=kept, **kw)
    return tok.cpu().numpy(), probs.cpu().numpy(), kept.cpu().numpy()


@pytest.mark.parametrize("V", VS)
def test_kept_set_and_probabilities(dev, V):
    for scale in SCALES:
        x = _logits(V, scale).to(dev)
        for T in TEMPS:
            for k in KS:
                for p in PS:
                    for b in range(ROWS if p < 1.0 else 1):      # top_p is snapped per row: one launch of all rows per row's value
                        top_p = _snapped(V, scale, b, T, k, p)
                        _, probs, kept = _sample(dev, x, temperature=T, top_k=k, top_p=top_p, u=[0.5] * ROWS)
                        for r_ in (range(ROWS) if p >= 1.0 else (b,)):
                            ref = _row(V, scale, r_, T).result(k, top_p)
                            tag = (V, scale, T, k, p, r_)
                            assert np.array_equal(probs[r_] > 0, ref["keep"]), tag
                            assert int(kept[r_]) == int(ref["keep"].sum()), tag
                            big = ref["r"] >= 1e-6
                            err = np.abs(probs[r_].astype(np.float64) - ref["r"])[big] / ref["r"][big]
                            assert err.max() <= 1e-4, (tag, float(err.max()))


@pytest.mark.parametrize("V", VS)
def test_draw_hits_the_token_whose_cdf_interval_holds_u(dev, V):
    scale = 4.0
    for T in TEMPS:
        for k in KS:
            for p in PS:
                for b in range(ROWS):
                    top_p = _snapped(V, scale, b, T, k, p)
                    ref = _row(V, scale, b, T).result(k, top_p)
                    likely = np.nonzero(ref["keep"] & (ref["r"] >= 1e-3))[0]
                    assert likely.size
                    want = sorted({int(likely[np.argmax(ref["r"][likely])]), int(likely[np.argmin(ref["r"][likely])]), int(likely[0]), int(likely[-1])})
                    us = [float(ref["cdf"][i] - 0.5 * ref["r"][i]) for i in want] + [0.0, U_LAST]
                    x = _logits(V, scale)[b].to(dev).expand(len(us), V).contiguous()
                    tok, _, _ = _sample(dev, x, temperature=T, top_k=k, top_p=top_p, u=us)
                    tag = (V, T, k, p, b)
                    assert tok[: len(want)].tolist() == want, tag
                    assert int(tok[-2]) == int(np.nonzero(ref["keep"])[0][0]), tag          # u = 0: the lowest kept id
                    assert ref["keep"][int(tok[-1])], tag


def test_philox_generator_matches_the_reference_stream(dev):
    """u = null: key = both seed words, counter = (*step_base + step_off, row): 32 rows x 128 draws against the test's own Philox"""
    V, k, rows, steps, seed = 1000, 8, 32, 128, 0x1234_5678_9ABC
    x1 = R.bf16_logits(V, 4.0, seed=77)
    ref = R.reference(x1, 1.0, k, 1.0)
    x = x1.to(dev).expand(rows, V).contiguous()
    edges = ref["cdf"][ref["keep"]]

    def run(seed_):
        out = []
        base = torch.zeros(1, device=dev, dtype=torch.int32)
        for t in range(steps):
            base.fill_(t + 5)
            out.append(_sample(dev, x, top_k=k, seed=seed_, step_base=base, step_off=-5)[0])
        return np.stack(out)        # [steps, rows]

    got = run(seed)
    skipped = 0
    for t in range(steps):
        for b in range(rows):
            u = R.uniform(seed, t, b)
            if np.abs(edges - u).min() < 1e-4:
                skipped += 1
                continue
            assert int(got[t, b]) == R.draw(ref, u), (t, b, u)
    assert skipped <= 0.01 * steps * rows, skipped
    assert len(set(got.reshape(-1).tolist())) >= 4
    assert not np.array_equal(got, run(seed & 0xFFFFFFFF)), "the high seed word must change the stream"
    assert not np.array_equal(got, run(seed + 1))
    assert np.array_equal(got, run(seed)), "the same seed must reproduce the stream bit for bit"


def test_edge_rows(dev):
    V = 1000
    x = R.bf16_logits(V, 4.0, seed=5)
    x[::2] = float("-inf")
    x[1::7] = float("nan")
    ref = R.reference(x, 1.0, 0, 1.0)
    us = np.linspace(0.0, U_LAST, 64).astype(np.float32)
    tok, probs, kept = _sample(dev, x.to(dev).expand(64, V).contiguous(), u=us.tolist())
    assert ref["keep"][tok].all() and np.isfinite(x.numpy()[tok]).all()
    assert np.array_equal(probs[0] > 0, ref["keep"]) and int(kept[0]) == int(ref["keep"].sum())
    # one +inf (and two: the lowest index), whatever the filters
    y = R.bf16_logits(V, 4.0, seed=6)
    y[613] = float("inf")
    z = y.clone()
    z[77] = float("inf")
    for kw in (dict(), dict(temperature=0.7, top_k=50, top_p=0.9)):
        tok, probs, kept = _sample(dev, torch.stack([y, z]).to(dev), u=[0.3, 0.9], **kw)
        assert tok.tolist() == [613, 77] and kept.tolist() == [1, 1]
        assert probs[0, 613] == 1.0 and probs[1, 77] == 1.0 and probs.sum() == 2.0
    # no finite logit: 0, as torch.argmax answers
    w = torch.full((2, V), float("-inf"))
    w[1, 3::5] = float("nan")
    tok, probs, kept = _sample(dev, w.to(dev), u=[0.3, 0.9], top_k=50, top_p=0.9)
    assert tok.tolist() == [0, 0] and kept.tolist() == [0, 0] and not probs.any()


def test_single_sequence_bookkeeping_equals_the_greedy_launch(dev):
    """B = 1 with the state block: next_token, tokens_out[state[2] + tok_off], state and x_out exactly as afk_decode_select_greedy leaves them for that token"""
    from audio_flamingo_amd import _lib, ops

    V, H, S0, seed = 1000, 64, 40, 99
    x = R.bf16_logits(V, 4.0, seed=8)
    ref = R.reference(x, 1.0, 8, 1.0)
    emb = torch.randn(V, H, generator=torch.Generator().manual_seed(1)).to(torch.bfloat16).to(dev)
    state0 = torch.tensor([0, S0 + 6, S0 + 5, S0 + 5], dtype=torch.int32)
    tok_off = 1 - S0                                  # token number t = state[2] + tok_off = 6
    u = R.uniform(seed, 6, 0)
    assert np.abs(ref["cdf"][ref["keep"]] - u).min() > 1e-4
    want = R.draw(ref, u)
    st = state0.to(dev)
    toks, x_out = torch.zeros(16, dtype=torch.int64, device=dev), torch.zeros(H, dtype=torch.bfloat16, device=dev)
    nxt = ops.decode_sample(x[None].to(dev), top_k=8, seed=seed, step_base=st[2:3], step_off=tok_off, tokens_out=toks, tok_off=tok_off, state=st, emb=emb,
                            x_out=x_out)
    assert int(nxt[0]) == want
    # the greedy launch on logits whose argmax is that token
    y = x.clone()
    y[want] = 100.0
    pv, pi = y.view(V // 8, 8).max(-1)
    pv, pi = pv.to(dev), (pi + 8 * torch.arange(V // 8)).to(torch.int32).to(dev)
    st2, toks2, x2, nxt2 = state0.to(dev), torch.zeros_like(toks), torch.zeros_like(x_out), torch.zeros(1, dtype=torch.int64, device=dev)
    _lib.call("afk_decode_select_greedy", pv.data_ptr(), pi.data_ptr(), V // 8, nxt2.data_ptr(), toks2.data_ptr(), tok_off, st2.data_ptr(), emb.data_ptr(),
              emb.stride(0), H, x2.data_ptr(), ops._stream())
    assert torch.equal(nxt, nxt2) and torch.equal(toks, toks2) and int(toks[6]) == want and torch.equal(st, st2) and torch.equal(x_out, x2)
    assert st.tolist() == [0, S0 + 7, S0 + 6, S0 + 6] and torch.equal(x_out, emb[want])


# ---------------------------------------------------------------------------------------------- generate(do_sample=True)
SAMPLED = dict(do_sample=True, temperature=1.5, top_k=20, top_p=0.95, seed=0xFEED_0000_0007, max_new_tokens=12)


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


def test_generate_one_seed_one_sequence_of_ids_eager_graphed_and_streamed(dev):
    m, p, audio = _case_a(dev)
    runs = [m.generate(p, use_graph=False, **audio, **SAMPLED), m.generate(p, use_graph=True, **audio, **SAMPLED), m.generate(p, streamer=_Collect(), **audio, **SAMPLED)]
    assert runs[0].shape[1] == p.shape[1] + 12 and torch.equal(runs[0], runs[1]) and torch.equal(runs[0], runs[2])
    # a left-padded batch of three
    g = torch.Generator().manual_seed(3)
    lens = (40, 23, 31)
    ids, att = torch.zeros((3, 40), dtype=torch.long), torch.zeros((3, 40), dtype=torch.long)
    for i, n in enumerate(lens):
        ids[i, 40 - n:] = torch.randint(0, 256, (n,), generator=g)
        att[i, 40 - n:] = 1
    kw = dict(attention_mask=att.to(dev), **SAMPLED)
    runs = [m.generate(ids.to(dev), use_graph=False, **kw), m.generate(ids.to(dev), use_graph=True, **kw), m.generate(ids.to(dev), streamer=_Collect(), **kw)]
    assert runs[0].shape == (3, 52) and torch.equal(runs[0], runs[1]) and torch.equal(runs[0], runs[2])


def test_generate_samples_inside_one_captured_graph_without_torch_selection(dev, monkeypatch):
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
    out = m.generate(p, **audio, **SAMPLED)
    assert out.shape[1] == p.shape[1] + 12 and len(captured) == 1


def test_generate_sampled_ids_lie_in_the_reference_kept_set(dev):
    m, p, audio = _case_a(dev)
    out = m.generate(p, **audio, **SAMPLED)
    S0, checked = p.shape[1], 0
    for t in range(12):
        lg = m(input_ids=out[:, : S0 + t], logits_to_keep=1, **audio).logits[0, -1].float().cpu()
        ref = R.reference(lg, SAMPLED["temperature"], SAMPLED["top_k"], SAMPLED["top_p"])
        if ref["margin"] < HALF_GAP:
            continue
        checked += 1
        assert ref["keep"][int(out[0, S0 + t])], (t, int(out[0, S0 + t]))
    assert checked >= 6


def test_generate_sampling_never_emits_a_suppressed_token(dev):
    from transformers import LogitsProcessorList, SuppressTokensLogitsProcessor

    m, p, audio = _case_a(dev)
    plain = m.generate(p, **audio, **SAMPLED)
    S0 = p.shape[1]
    banned = int(plain[0, S0 + 3])
    sup = m.generate(p, logits_processor=LogitsProcessorList([SuppressTokensLogitsProcessor([banned], device=dev)]), **audio, **SAMPLED)
    assert banned not in sup[0, S0:].tolist() and sup.shape == plain.shape

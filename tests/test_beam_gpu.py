"""GPU: afk_beam_step and afk_beam_reorder_cache (csrc/decode_beam.hip) against the numpy restatement of their contract (tests/_beam_ref.py, which
tests/test_beam_cpu.py pins to GenerationMixin's own helpers) and against torch.index_select, and generate(num_beams > 1) on them: the device route against
the host loop it replaces (still selectable: beam_on_device), eager and graph-replayed, its launch counts, and num_return_sequences."""
import itertools
import os

import numpy as np
import pytest
import torch

from tests import _beam_ref as R

pytestmark = pytest.mark.gpu
_CACHE = {}
STEPS = 6
PENALTIES, EARLY, N_EOS = (0.0, 1.0, 2.0), (False, True, "never"), (0, 1, 2)
SHARP = 1e-3     # every step of every case: consecutive scores among the row's best keep + 1 continuations are at least this far apart (asserted on the restatement)
SCORE_TOL = 1e-4   # a handful of fp32 operations on magnitudes below 50 is about 1e-5
# seeds picked on the CPU so that every case is SHARP at every step and, with eos ids, finishes a hypothesis in front of the length limit
SEEDS = {   # (B, nb, V, n_eos): seed
    (1, 2, 67, 0): 1, (1, 2, 67, 1): 40, (1, 2, 67, 2): 1, (1, 2, 1031, 0): 1, (1, 2, 1031, 1): 86, (1, 2, 1031, 2): 1,
    (1, 5, 67, 0): 2, (1, 5, 67, 1): 1, (1, 5, 67, 2): 2, (1, 5, 1031, 0): 1, (1, 5, 1031, 1): 1, (1, 5, 1031, 2): 2,
    (3, 2, 67, 0): 1, (3, 2, 67, 1): 2, (3, 2, 67, 2): 1, (3, 2, 1031, 0): 1, (3, 2, 1031, 1): 1, (3, 2, 1031, 2): 1,
    (3, 5, 67, 0): 1, (3, 5, 67, 1): 1, (3, 5, 67, 2): 4, (3, 5, 1031, 0): 1, (3, 5, 1031, 1): 2, (3, 5, 1031, 2): 7,
}


def case_logits(B, nb, V, n_eos, seed):
    """-> (eos ids, [STEPS] fp32 logits [B * nb, V]); in a third of the rows an eos id sits close under the row's maximum, so that hypotheses finish early"""
    gen = np.random.default_rng(seed)
    eos = tuple(int(e) for e in gen.choice(V, size=n_eos, replace=False))
    logits = [(4.0 * gen.standard_normal((B * nb, V))).astype(np.float32) for _ in range(STEPS)]
    for x in logits:
        for e in eos:
            rows = gen.random(B * nb) < 1.0 / 3.0
            x[rows, e] = x[rows].max(-1) - gen.uniform(0.5, 2.0, size=int(rows.sum())).astype(np.float32)
    return eos, logits


def case_is_sound(B, nb, V, n_eos, seed):
    """the two properties the comparison needs, on the restatement (the running beams, and so the scores, do not depend on the penalty or on early_stopping
    as long as the search stays open: False / 1.0 runs all STEPS)"""
    eos, logits = case_logits(B, nb, V, n_eos, seed)
    st, trace = R.new_state(B, nb, STEPS), {}
    div, hdiv = R.tables(STEPS, 1.0, False)
    for t in range(STEPS):
        R.step(st, logits[t], t, nb=nb, max_new=STEPS, eos=eos, early_stopping=False, div=div, hdiv=hdiv, trace=trace)
        if st["status"][1] == 0 and t + 1 < STEPS:
            return False   # closed early even without early_stopping: later steps would go unchecked
    gap = min(float((top[:-1] - top[1:]).min()) for top in trace["top"])
    return gap >= SHARP and (n_eos == 0 or any(trace["ended"]))


def _device_state(dev, B, nb, eos, lp, es, max_new=STEPS):
    from audio_flamingo_amd import ops

    return ops.beam_state(B, nb, max_new, device=dev, eos=eos, length_penalty=lp, early_stopping=es)


def _compare(d, st, where, B, nb):
    from audio_flamingo_amd import ops

    assert d["status"].tolist() == st["status"].tolist(), where
    run = d["run_score"].cpu().numpy()
    live = st["run_score"] > -1e8   # entries that carry -1e9 tie after the add absorbs their score: only their being there is compared
    assert np.array_equal(run > -1e8, live), where
    assert np.abs(run[live] - st["run_score"][live]).max(initial=0) <= SCORE_TOL, where
    assert np.array_equal(d["next_token"].cpu().numpy().reshape(B, nb)[live], st["next_token"].reshape(B, nb)[live]), where
    if live.all():
        assert d["src"].cpu().tolist() == st["src"].tolist(), where
    seq, ln, score, done = (x.cpu().numpy() for x in ops.beam_finished(d))
    assert np.array_equal(done, st["fin_done"]) and np.array_equal(ln, st["fin_len"]), where
    assert np.abs(score - st["fin_score"]).max() <= SCORE_TOL, where
    for b, k in zip(*np.nonzero(done)):
        assert np.array_equal(seq[b, k, : ln[b, k]], st["fin_seq"][b, k, : ln[b, k]]), where
    assert sorted(d["fin_slot"].view(B, nb)[0].tolist()) == list(range(nb)), where
    assert np.array_equal(d["can_improve"].cpu().numpy() != 0, st["can_improve"]), where


@pytest.mark.parametrize("V", [67, 1031])     # neither a multiple of 4 nor of 64; below and above one pass of the 1024 threads
@pytest.mark.parametrize("nb", [2, 5])
@pytest.mark.parametrize("B", [1, 3])
def test_step_equals_the_restatement_over_six_steps(dev, B, nb, V):
    from audio_flamingo_amd import ops

    base = torch.zeros(1, device=dev, dtype=torch.int32)
    for n_eos in N_EOS:
        seed = SEEDS[(B, nb, V, n_eos)]
        assert case_is_sound(B, nb, V, n_eos, seed), "a broken case: not sharp at every step, or nothing finishes early"
        eos, logits = case_logits(B, nb, V, n_eos, seed)
        dl = [torch.from_numpy(x).to(dev) for x in logits]
        closed_early = 0
        for lp, es in itertools.product(PENALTIES, EARLY):
            d = _device_state(dev, B, nb, eos, lp, es)
            st = R.new_state(B, nb, STEPS)
            div, hdiv = R.tables(STEPS, lp, es)
            assert np.array_equal(d["div"].cpu().numpy(), div) and np.array_equal(d["hdiv"].cpu().numpy(), hdiv)
            for t in range(STEPS):
                how = dict(step_base=base.fill_(t + 5), step_off=-5) if (t + nb) & 1 else dict(step_off=t)   # a device step_base with a nonzero step_off
                ops.beam_step(dl[t], d, **how)
                R.step(st, logits[t], t, nb=nb, max_new=STEPS, eos=eos, early_stopping=es, div=div, hdiv=hdiv)
                _compare(d, st, (B, nb, V, n_eos, lp, es, t), B, nb)
            closed_early += st["status"][0] + 1 < STEPS   # the launches behind the closing step were compared too: they moved nothing
            assert d["ws"][0].item() == 0   # the arrival counter is left at zero
        if n_eos and B == 1 and nb == 2:   # (more rows or beams would all have to fill their slots inside six steps)
            assert closed_early, "with eos ids some setting must close a one-row, two-beam search in front of the length limit"


def test_step_full_vocabulary(dev):
    """one step at the AF3 vocabulary: four live beams, an eos id among the best continuations"""
    from audio_flamingo_amd import ops

    B, nb, V, max_new, t = 1, 4, 152064, 4, 1
    gen = np.random.default_rng(11)
    logits = (3.0 * gen.standard_normal((nb, V))).astype(np.float32)
    logits[2, 77] = np.nan   # NaN counts as -inf
    run = np.array([[-0.5, -1.25, -1.75, -2.5]], dtype=np.float32)
    eos = (int(np.argsort(logits[0])[-2]),)
    d = _device_state(dev, B, nb, eos, 1.0, False, max_new)
    st, trace = R.new_state(B, nb, max_new), {}
    st["run_score"][:] = run
    st["status"][:] = (0, 1)
    d["run_score"].copy_(torch.from_numpy(run))
    d["status"].copy_(torch.tensor([0, 1], dtype=torch.int32))
    div, hdiv = R.tables(max_new, 1.0, False)
    ops.beam_step(torch.from_numpy(logits).to(dev), d, step_off=t)
    R.step(st, logits, t, nb=nb, max_new=max_new, eos=eos, early_stopping=False, div=div, hdiv=hdiv, trace=trace)
    assert float((trace["top"][0][:-1] - trace["top"][0][1:]).min()) >= SHARP and any(trace["ended"])
    _compare(d, st, "full vocabulary", B, nb)
    assert len(set(st["src"].tolist())) > 1, "the case must draw from more than one beam"


def test_tie_rule_lowest_flat_index(dev):
    """equal scores: the lower flat index beam * V + token first - inside one beam's row, across beams, and where the candidates run out (nb * V == keep)"""
    from audio_flamingo_amd import ops

    for nb, V, eos, live_all in ((3, 67, (), False), (3, 67, (), True), (5, 1031, (1,), True), (3, 2, (1,), True), (16, 4100, (0, 2, 4), True)):
        B, max_new = 2, 3
        d = _device_state(dev, B, nb, eos, 1.0, False, max_new)
        st = R.new_state(B, nb, max_new)
        if live_all:
            st["run_score"][:] = 0.0
            d["run_score"].zero_()
        logits = np.zeros((B * nb, V), dtype=np.float32)
        div, hdiv = R.tables(max_new, 1.0, False)
        ops.beam_step(torch.from_numpy(logits).to(dev), d, step_off=0)
        R.step(st, logits, 0, nb=nb, max_new=max_new, eos=eos, early_stopping=False, div=div, hdiv=hdiv)
        where = (nb, V, eos, live_all)
        assert d["next_token"].cpu().tolist() == st["next_token"].tolist() and d["src"].cpu().tolist() == st["src"].tolist(), where
        keep = (len(eos) + 1) * nb
        flat = [f for f in range(keep) if (f % V) not in eos][:nb]   # the first keep flat indices, the ending ones dropped
        if len(flat) == nb:
            assert st["next_token"][:nb].tolist() == [f % V for f in flat] and st["src"][:nb].tolist() == [f // V for f in flat], where
        _compare(d, st, where, B, nb)


def test_step_refusals(dev):
    from audio_flamingo_amd import _lib, ops
    from audio_flamingo_amd._lib import AfkError

    B, nb, V, max_new = 2, 3, 67, 4
    d = _device_state(dev, B, nb, (5,), 1.0, False, max_new)
    logits = torch.zeros((B * nb, V), device=dev)
    names = ("run_score", "fin_score", "fin_len", "fin_done", "fin_slot", "fin_seq", "can_improve", "bp", "next_token", "src", "status", "ws")
    good = [logits.data_ptr(), V, B, nb, V, max_new, None, 0, d["eos"].data_ptr(), 1, 0, d["div"].data_ptr(), d["hdiv"].data_ptr()] + \
           [d[k].data_ptr() for k in names] + [d["ws"].numel(), ops._stream()]
    _lib.call("afk_beam_step", *good)
    for at in [0, 11, 12] + list(range(13, 13 + len(names))):
        bad = list(good)
        bad[at] = None
        with pytest.raises(AfkError, match="null pointer"):
            _lib.call("afk_beam_step", *bad)
    for at, value, what in ((3, 1, "beams"), (3, 17, "beams"), (9, 40, "keep ="), (8, None, "eos list"), (9, -1, "eos list"), (25, 3, "workspace"), (1, V - 1, "shape")):
        bad = list(good)
        bad[at] = value
        with pytest.raises(AfkError, match=what):
            _lib.call("afk_beam_step", *bad)
    with pytest.raises(AfkError, match="continuations"):   # nb * V < keep
        _lib.call("afk_beam_step", *(good[:1] + [1, B, nb, 1] + good[5:]))
    assert _lib.load().afk_beam_step_workspace_ints(B, 17, 0) == -1 and _lib.load().afk_beam_step_workspace_ints(B, 16, 4) == -1
    assert not ops.beam_caps_ok(17, 0, V) and not ops.beam_caps_ok(16, 4, V) and not ops.beam_caps_ok(1, 0, V) and ops.beam_caps_ok(16, 3, V)
    with pytest.raises(AfkError, match="beam_step"):
        ops.beam_step(logits[:-1], d, step_off=0)
    with pytest.raises(AfkError, match="beam_step"):
        ops.beam_step(logits.double(), d, step_off=0)
    with pytest.raises(AfkError, match="beam_step"):
        ops.beam_step(logits, dict(d, fin_len=d["fin_len"].long()), step_off=0)
    with pytest.raises(AfkError, match="beam_state"):
        ops.beam_state(B, 17, max_new, device=dev)
    torch.cuda.synchronize()


def test_step_outside_the_range_and_behind_the_close_writes_nothing(dev):
    from audio_flamingo_amd import ops

    B, nb, V = 1, 2, 67
    seed = SEEDS[(B, nb, V, 1)]
    eos, logits = case_logits(B, nb, V, 1, seed)
    d = _device_state(dev, B, nb, eos, 1.0, True)
    dl = [torch.from_numpy(x).to(dev) for x in logits]
    keys = [k for k, v in d.items() if torch.is_tensor(v)]
    base = torch.zeros(1, device=dev, dtype=torch.int32)

    def unchanged(how):
        before = {k: d[k].clone() for k in keys}
        ops.beam_step(dl[0], d, **how)
        torch.cuda.synchronize()
        return all(torch.equal(before[k].view(torch.uint8), d[k].view(torch.uint8)) for k in keys)

    ops.beam_step(dl[0], d, step_off=0)
    for outside in (STEPS, -1, STEPS + 1000):
        assert unchanged(dict(step_base=base.fill_(outside), step_off=0)) and unchanged(dict(step_off=outside)), outside
    t = 1
    while d["status"].tolist()[1] and t < STEPS:
        ops.beam_step(dl[t], d, step_off=t)
        t += 1
    assert d["status"].tolist() == [t - 1, 0]
    assert t < STEPS, "early_stopping=True with a likely eos must close in front of the length limit"
    assert d["src"].cpu().tolist() == list(range(B * nb))   # the closing step hands the identity to the cache move
    for later in range(t, STEPS):
        assert unchanged(dict(step_off=later)), later


def test_reorder_cache_moves_the_tail_only(dev):
    from audio_flamingo_amd import ops
    from audio_flamingo_amd._lib import AfkError

    L, B, nb, Hkv, D, S0, max_new = 2, 2, 3, 2, 64, 62, 8
    Smax = S0 + max_new
    gen = torch.Generator().manual_seed(5)
    K0 = torch.randn((L, B * nb, Smax, Hkv * D), generator=gen).to(torch.bfloat16).to(dev)     # every beam its own bits, the prompt included: an
    V0 = torch.randn((L, B * nb, Hkv, D, ops.pad64(Smax)), generator=gen).to(torch.bfloat16).to(dev)   # untouched prompt is then visible as such
    for src_rows, last in (([0, 0, 2, 5, 3, 4], 66), ([0, 0, 2, 5, 3, 4], 67), ([0, 1, 2, 3, 4, 5], 66), ([0, 0, 2, 3, 4, 5], 66), ([-7, 9, 1, 5, 3, 99], 66),
                           ([0, 0, 2, 5, 3, 4], 5000)):
        K, V = K0.clone(), V0.clone()
        src = torch.tensor(src_rows, device=dev, dtype=torch.int32)
        cur = torch.tensor([last], device=dev, dtype=torch.int32)
        ops.beam_reorder_cache(K, V, src, cur, nb=nb, S0=S0, max_new=max_new)
        clamped = torch.stack([src[b * nb:(b + 1) * nb].clamp(b * nb, b * nb + nb - 1) for b in range(B)]).reshape(-1).long()
        hi = min(last, Smax - 1) + 1   # the slots S0 .. *cur move: the tail crosses the 64-slot pitch boundary of Vt
        assert torch.equal(K[:, :, S0:hi], K0.index_select(1, clamped)[:, :, S0:hi]), (src_rows, last)
        assert torch.equal(V[..., S0:hi], V0.index_select(1, clamped)[..., S0:hi]), (src_rows, last)
        assert torch.equal(K[:, :, :S0], K0[:, :, :S0]) and torch.equal(K[:, :, hi:], K0[:, :, hi:]), (src_rows, last)
        assert torch.equal(V[..., :S0], V0[..., :S0]) and torch.equal(V[..., hi:], V0[..., hi:]), (src_rows, last)
        if src_rows == [0, 1, 2, 3, 4, 5]:
            assert torch.equal(K, K0) and torch.equal(V, V0)
    src = torch.arange(B * nb, device=dev, dtype=torch.int32)
    cur = torch.tensor([S0], device=dev, dtype=torch.int32)
    with pytest.raises(AfkError, match="beam_reorder_cache"):
        ops.beam_reorder_cache(K0, V0, src, cur, nb=nb, S0=S0, max_new=max_new + 1)
    with pytest.raises(AfkError, match="beam_reorder_cache"):
        ops.beam_reorder_cache(K0, V0, src.long(), cur, nb=nb, S0=S0, max_new=max_new)
    with pytest.raises(AfkError, match="beam_reorder_cache"):
        ops.beam_reorder_cache(K0, V0, src, cur, nb=4, S0=S0, max_new=max_new)
    with pytest.raises(AfkError, match="beam_reorder_cache"):
        ops.beam_reorder_cache(K0[:, :, :, :64], V0, src, cur, nb=nb, S0=S0, max_new=max_new)
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------- generate()
NEW = 12   # a poll at step 8 is crossed


def _cases(dev):
    """cases A and Apad of test_generate_beam_search_matches_reference: (model, {case: (ids, kwargs)}, the eos id its with_eos cases use)"""
    if "cases" not in _CACHE:
        from tests.test_model_gpu import G, _gen_prompt, _model

        g = torch.load(os.path.join(G, "tiny64_caseA.pt"))
        ids = _gen_prompt(g)
        S0 = ids.shape[1]
        padded = ids.clone()
        padded[0, :5] = 1000
        ids2 = torch.cat([padded, ids], 0)
        att = torch.ones_like(ids2)
        att[0, :5] = 0
        feats, fmask = g["feats"][:1], g["fmask"][:1]
        _CACHE["cases"] = (_model(dev), {
            "A": (ids.to(dev), dict(input_features=feats.to(dev), input_features_mask=fmask.to(dev))),
            "Apad": (ids2.to(dev), dict(input_features=feats.repeat(2, 1, 1).to(dev), input_features_mask=fmask.repeat(2, 1).to(dev), attention_mask=att.to(dev))),
        }, int(g["generate"][0, S0 + 6]), int(g["generate"][0, S0 + 9]))
    return _CACHE["cases"]


def _host(m, ids, **kw):
    m.beam_on_device = False
    try:
        return m.generate(ids, **kw)
    finally:
        del m.beam_on_device


@pytest.mark.parametrize("case,num_beams,with_eos", [("A", 3, False), ("A", 4, True), ("Apad", 2, False), ("Apad", 3, True)])
def test_generate_device_route_equals_the_host_route(dev, case, num_beams, with_eos):
    m, cases, eos, eos2 = _cases(dev)
    assert type(m).beam_on_device, "the device route is the default"
    ids, audio = cases[case]
    stop = dict(eos_token_id=eos, pad_token_id=0) if with_eos else {}
    settings = [stop, dict(eos_token_id=[eos2, eos], pad_token_id=0), dict(stop, length_penalty=0.0), dict(stop, length_penalty=2.0),
                dict(stop, early_stopping=True), dict(stop, early_stopping="never")]
    lengths = set()
    for extra in settings:
        kw = dict(audio, max_new_tokens=NEW, num_beams=num_beams, **extra)
        want = _host(m, ids, **kw)
        for use_graph in (False, True):
            got = m.generate(ids, use_graph=use_graph, **kw)
            assert torch.equal(got, want), (case, num_beams, extra, use_graph, got.tolist(), want.tolist())
        lengths.add(want.shape[1] - ids.shape[1])
    if with_eos:
        assert min(lengths) < NEW, "the eos must end the search early for these cases to mean anything"
    else:
        assert NEW in lengths


def test_generate_launch_counts_and_one_graph(dev, monkeypatch):
    from audio_flamingo_amd import _lib

    m, cases, eos, _ = _cases(dev)
    ids, audio = cases["Apad"]
    captured, names = [], []
    real_graph, real_call = torch.cuda.graph, _lib.call

    class Counting(real_graph):
        def __init__(self, *a, **k):
            captured.append(1)
            super().__init__(*a, **k)

    def spy(name, *a):
        names.append(name)
        return real_call(name, *a)

    def refuse(*a, **k):
        raise AssertionError("the device route selects and reorders with its own launches")

    monkeypatch.setattr(torch.cuda, "graph", Counting)
    monkeypatch.setattr(_lib, "call", spy)
    for owner in (torch, torch.Tensor):
        monkeypatch.setattr(owner, "topk", refuse)
        monkeypatch.setattr(owner, "log_softmax", refuse)
    kw = dict(audio, max_new_tokens=NEW, num_beams=3)
    eager = m.generate(ids, use_graph=False, **kw)
    assert eager.shape[1] == ids.shape[1] + NEW   # no eos: every step runs
    assert names.count("afk_beam_step") == NEW and names.count("afk_beam_reorder_cache") == NEW - 1 and not captured
    names.clear()
    replayed = m.generate(ids, use_graph=True, **kw)
    assert len(captured) == 1 and names.count("afk_beam_step") == 3 and names.count("afk_beam_reorder_cache") == 2   # token 0, the eager step 1, the captured step
    assert torch.equal(replayed, eager)
    names.clear(), captured.clear()
    m.generate(ids, **kw)   # use_graph=None: more than 3 tokens are captured, as everywhere in generate()
    assert len(captured) == 1
    monkeypatch.undo()
    names.clear()
    monkeypatch.setattr(_lib, "call", spy)
    assert torch.equal(_host(m, ids, **kw), eager) and "afk_beam_step" not in names and "afk_beam_reorder_cache" not in names


def test_generate_num_return_sequences_with_beams(dev):
    m, cases, eos, eos2 = _cases(dev)
    for case in ("A", "Apad"):
        ids, audio = cases[case]
        B, S0 = ids.shape
        for stop in ({}, dict(eos_token_id=[eos, eos2], pad_token_id=0)):
            kw = dict(audio, max_new_tokens=NEW, num_beams=4, **stop)
            one = m.generate(ids, **kw)
            three = m.generate(ids, num_return_sequences=3, **kw)
            assert three.shape[0] == B * 3 and three.shape[1] >= one.shape[1] and torch.equal(three[:, :S0], ids.repeat_interleave(3, 0))
            best = three[0::3]
            assert torch.equal(best[:, : one.shape[1]], one) and bool((best[:, one.shape[1]:] == 0).all())   # row b * 3 is the n = 1 answer, padded to the longest
            assert len({tuple(r) for r in three[:3].tolist()}) == 3   # three different hypotheses
            assert torch.equal(_host(m, ids, num_return_sequences=3, **kw), three)
            assert torch.equal(m.generate(ids, num_return_sequences=4, use_graph=False, **kw)[0::4, : one.shape[1]], one)
    ids, audio = cases["A"]
    from types import SimpleNamespace

    gc = SimpleNamespace(num_return_sequences=3, num_beams=4, max_new_tokens=NEW)
    assert torch.equal(m.generate(ids, generation_config=gc, **audio), m.generate(ids, max_new_tokens=NEW, num_beams=4, num_return_sequences=3, **audio))
    with pytest.raises(ValueError, match="has to be smaller or equal to `num_beams`"):
        m.generate(ids, max_new_tokens=4, num_beams=4, num_return_sequences=5, **audio)
    with pytest.raises(ValueError, match="Greedy methods"):
        m.generate(ids, max_new_tokens=4, num_return_sequences=2, **audio)


def test_generate_num_return_sequences_sampled_equals_the_expanded_call(dev):
    m, cases, _, _ = _cases(dev)
    for case in ("A", "Apad"):
        ids, audio = cases[case]
        kw = dict(max_new_tokens=NEW, do_sample=True, seed=1234, temperature=1.5, top_k=0)
        got = m.generate(ids, num_return_sequences=2, **audio, **kw)
        by_hand = m.generate(ids.repeat_interleave(2, 0), **{k: v.repeat_interleave(2, 0) for k, v in audio.items()}, **kw)
        assert got.shape[0] == 2 * ids.shape[0] and torch.equal(got, by_hand)
        assert not torch.equal(got[0], got[1]), "the draw is keyed by (step, row): the copies differ"

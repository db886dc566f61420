"""GPU: assisted decoding.  The two launches (afk_assist_begin / afk_assist_stage) against their integer restatement (tests/_assist_ref.py) - exact integer
comparison, the gathered embedding rows bit-equal to index_select, no tolerance anywhere; generate(assistant_model=...) on the trained tiny model against the
plain greedy call of the same prompt and the golden ids, with an assistant of the same weights (every draft is accepted) and with a poor one of another
geometry (drafts are rejected); what a captured step launches."""
import json
import os
from collections import Counter

import numpy as np
import pytest
import torch

from tests import _assist_ref as R
from tests import _lookup_ref as L
from tests.test_sampler_gpu import _case_a

pytestmark = pytest.mark.gpu

VOCAB = 1024
_EMB = {}


def _i32(a, dev):
    return torch.tensor(np.asarray(a, dtype=np.int32), dtype=torch.int32, device=dev)


def _emb(dev, H):
    if (dev, H) not in _EMB:
        _EMB[dev, H] = torch.randn((VOCAB, H), generator=torch.Generator().manual_seed(H)).to(dev, torch.bfloat16)
    return _EMB[dev, H]


def _check_stage(dev, k, H, drafts, eos=(), *, emitted=1, max_new=10 ** 6, done=0, last=5, cur=8, lo=2):
    """one afk_assist_stage launch against R.stage: every output, every status word, and nothing else moved -> n_cand"""
    from audio_flamingo_amd import _lib, ops

    n, M = 11, k + 1
    ids = np.zeros(n + 5, dtype=np.int32)
    ids[:n] = np.arange(n) + 100
    ids[n - 1] = last
    st = L.new_status(n, emitted, done)
    st[L.N_CAND], st[L.STEPS], st[L.ACCEPTED], st[L.REJECTING] = 77, 5, 3, 2   # n_cand is overwritten, the others are not the stage's to touch
    state = np.array([lo, cur + 1, cur, cur - lo], dtype=np.int32)
    draft = np.full(cur + k + 3, -7, dtype=np.int64)
    draft[cur:cur + k] = drafts
    d_ids, d_st, d_state, d_draft = _i32(ids, dev), _i32(st, dev), _i32(state, dev), torch.from_numpy(draft).to(dev)
    cand, pos, kr = (torch.full(s, -1, device=dev, dtype=torch.int32) for s in ((k,), (M,), (M, 2)))
    rows = torch.full((M,), -1, device=dev, dtype=torch.int64)
    eos_t = _i32(eos, dev) if eos else None
    emb = _emb(dev, H)
    x = torch.zeros((M, H), device=dev, dtype=torch.bfloat16)
    _lib.call("afk_assist_stage", d_ids.data_ptr(), d_ids.numel(), d_st.data_ptr(), d_state.data_ptr(), k, max_new, ops._p(eos_t), len(eos), d_draft.data_ptr(),
              d_draft.numel(), cand.data_ptr(), rows.data_ptr(), pos.data_ptr(), kr.data_ptr(), emb.data_ptr(), emb.stride(0), VOCAB, H, x.data_ptr(), x.stride(0),
              ops._stream())
    want = R.stage(ids, st, state, draft, k, max_new, eos)
    what = (k, H, list(drafts), eos, emitted, max_new, done, last)
    assert d_st.cpu().numpy().tolist() == st.tolist(), what
    assert cand.cpu().numpy().tolist() == want["cand"].tolist(), what
    assert rows.cpu().numpy().tolist() == want["rows"].tolist() and pos.cpu().numpy().tolist() == want["pos"].tolist(), what
    assert kr.cpu().numpy().tolist() == want["krange"].tolist(), what
    assert d_ids.cpu().numpy().tolist() == ids.tolist() and d_state.cpu().numpy().tolist() == state.tolist() and d_draft.cpu().numpy().tolist() == draft.tolist(), what
    assert torch.equal(x, emb.index_select(0, rows.clamp(0, VOCAB - 1))), what
    return int(st[L.N_CAND])


def _drafts(k, seed, eos_at=None, eos=99, outside_at=None):
    d = (200 + 3 * np.arange(k) + seed) % (VOCAB - 100) + 100   # never an eos id, never id 5
    if eos_at is not None and eos_at < k:
        d[eos_at] = eos
    if outside_at is not None and outside_at < k:
        d[outside_at] = VOCAB + 17   # a drafted id outside the vocabulary: cand and rows keep it, the gather clamps it
    return d.tolist()


@pytest.mark.parametrize("H", [64, 72])
@pytest.mark.parametrize("k", [1, 4, 31])
def test_stage_equals_the_restatement(dev, k, H):
    c = lambda *a, **kw: _check_stage(dev, k, H, *a, **kw)
    eos = (99, 98)
    assert c(_drafts(k, 0)) == k                                        # no eos list
    assert c(_drafts(k, 1), eos) == k                                   # an eos list, no eos drafted
    assert c(_drafts(k, 2, eos_at=0), eos) == 1                         # eos at j = 0: it stays, alone
    assert c(_drafts(k, 3, eos_at=k // 2, eos=98), eos) == k // 2 + 1   # in the middle: cut behind it
    assert c(_drafts(k, 4, eos_at=k - 1), eos) == k                     # last
    assert c(_drafts(k, 5, outside_at=k // 2), eos) == k                # an id outside the vocabulary
    assert c(_drafts(k, 5, outside_at=0), eos, last=VOCAB + 3) == k     # ... and as the last emitted token (row 0)
    assert c(_drafts(k, 6), eos, emitted=9, max_new=10) == 0            # emitted == max_new - 1: no candidates
    assert c(_drafts(k, 7), eos, emitted=8, max_new=10) == 1            # max_new - 2: one
    assert c(_drafts(k, 7, eos_at=0), eos, emitted=8, max_new=10) == 1
    assert c(_drafts(k, 8), eos, emitted=3, max_new=3 + k) == min(k, k - 1)
    assert c(_drafts(k, 9), eos, done=1) == 0                           # done on entry: none
    assert c(_drafts(k, 9, eos_at=0), eos, done=1, emitted=4, max_new=4) == 0
    assert c(_drafts(k, 10), eos, cur=16000, lo=0) == k                 # a long cache: positions and key ranges follow the state


@pytest.mark.parametrize("H", [64, 72, 128])
def test_begin_equals_the_restatement(dev, H):
    """dstate <- state and x0 <- the DRAFT model's embedding row of the last emitted id (H = 128: a hidden size other than the target's 64 / 72 of the stage
    cases - the launch only ever sees the assistant's table), clamped to the vocabulary; with done set the launch rewrites the same values"""
    from audio_flamingo_amd import _lib, ops

    emb = _emb(dev, H)
    for last, done, n in ((5, 0, 11), (VOCAB - 1, 0, 1), (VOCAB + 40, 0, 7), (-3, 0, 7), (17, 1, 11)):
        ids = np.zeros(n + 4, dtype=np.int32)
        ids[:n] = np.arange(n) + 300
        ids[n - 1] = last
        st = L.new_status(n, 3, done)
        state = np.array([2, n + 1, n, n - 2], dtype=np.int32)
        d_ids, d_st, d_state = _i32(ids, dev), _i32(st, dev), _i32(state, dev)
        dstate = torch.full((4,), -1, device=dev, dtype=torch.int32)
        x0 = torch.zeros((1, H), device=dev, dtype=torch.bfloat16)
        for _ in range(2 if done else 1):
            _lib.call("afk_assist_begin", d_ids.data_ptr(), d_ids.numel(), d_st.data_ptr(), d_state.data_ptr(), dstate.data_ptr(), emb.data_ptr(), emb.stride(0), VOCAB, H,
                      x0.data_ptr(), ops._stream())
        want_state, tok = R.begin(ids, st, state, VOCAB)
        assert dstate.cpu().numpy().tolist() == want_state.tolist() and torch.equal(x0, emb[tok:tok + 1]), (H, last, done)
        assert d_ids.cpu().numpy().tolist() == ids.tolist() and d_st.cpu().numpy().tolist() == st.tolist() and d_state.cpu().numpy().tolist() == state.tolist()


def test_launches_refuse_what_the_contract_refuses(dev):
    from audio_flamingo_amd import _lib, ops
    from audio_flamingo_amd._lib import AfkError

    z = lambda *shape, dtype=torch.int32: torch.zeros(shape, device=dev, dtype=dtype)
    ids, status, state, dstate, cand, pos, kr = z(8), z(8), z(4), z(4), z(31), z(32), z(32, 2)
    rows, draft = z(32, dtype=torch.int64), z(64, dtype=torch.int64)
    emb_t, x_t = z(16, 64, dtype=torch.bfloat16), z(32, 64, dtype=torch.bfloat16)
    status[0] = 4
    P, s = (lambda t: t.data_ptr()), ops._stream()
    stage = lambda k=3, H=64, ids=P(ids), draft=P(draft), x=P(x_t), emb=P(emb_t), ldx=64, n_eos=0: _lib.call(
        "afk_assist_stage", ids, 8, P(status), P(state), k, 8, 0, n_eos, draft, 64, P(cand), P(rows), P(pos), P(kr), emb, 64, 16, H, x, ldx, s)
    begin = lambda H=64, ids=P(ids), dstate=P(dstate), x=P(x_t), emb=P(emb_t), ld=64: _lib.call("afk_assist_begin", ids, 8, P(status), P(state), dstate, emb, ld, 16, H, x, s)
    stage(), stage(k=31), begin()   # the good calls pass
    for kw in (dict(k=0), dict(k=32), dict(H=68), dict(H=0), dict(ids=0), dict(draft=0), dict(x=0), dict(emb=0), dict(ldx=60), dict(n_eos=2), dict(x=P(x_t) + 2)):
        with pytest.raises(AfkError, match="afk_assist_stage"):
            stage(**kw)
    for kw in (dict(H=68), dict(H=0), dict(ids=0), dict(dstate=0), dict(x=0), dict(emb=0), dict(ld=32), dict(emb=P(emb_t) + 4)):
        with pytest.raises(AfkError, match="afk_assist_begin"):
            begin(**kw)


# ---------------------------------------------------------------------------------------------- generate()
NEW = 12   # crosses the poll in front of step 8
_CTX = {}


def _ctx(dev):
    """the trained tiny model (case A), its prompt and audio, the plain greedy ids, a second instance of the same weights and a poor assistant"""
    if dev not in _CTX:
        from tests.test_model_gpu import G, _model

        m, p, audio = _case_a(dev)
        plain = m.generate(p, max_new_tokens=NEW, **audio)
        gold = torch.load(os.path.join(G, "tiny64_caseA.pt"))["generate"][0, -24:][:NEW].tolist()
        _CTX[dev] = (m, p, audio, plain, gold, _model(dev), _poor(dev))
    return _CTX[dev]


def _poor(dev, **text):
    """an assistant of another geometry: one decoder layer, half the hidden size (two query heads of 64 over one key head), seeded random weights, the
    same vocabulary and the same audio tower geometry (so its placeholder count is the target's)"""
    from transformers import AudioFlamingo3Config

    from audio_flamingo_amd.modeling import AudioFlamingo3ForConditionalGeneration as Mine
    from tests.test_host_cpu import TINY

    tc = dict(TINY["text_config"], hidden_size=128, intermediate_size=256, num_hidden_layers=1, num_attention_heads=2, num_key_value_heads=1, **text)
    return Mine(AudioFlamingo3Config(**dict(TINY, text_config=tc)), device=dev, init_seed=11)


@pytest.mark.parametrize("use_graph", [False, True])
@pytest.mark.parametrize("who", ["second instance", "self"])
@pytest.mark.parametrize("k", [1, 3, 7])
def test_same_weights_every_draft_is_accepted(dev, k, who, use_graph, monkeypatch):
    """The assistant holds the target's weights (a second instance loaded from the same state dict, or the target itself on a second cache): the ids are the
    plain greedy ids and the golden ids, eager and replayed runs are bit-equal, no step rejects a draft and every emitted token but token 0 and one per step
    was a draft: accepted == emitted - 1 - steps (token 0 comes from the prefill, outside every step).  That fails if the assistant's cache loses the
    last draft's keys: the step behind a fully accepted one then drafts behind a hole and the target rejects.  Measured on the MI355X with the pass
    behind the last draft left out: k = 1 rejects in 2 of its 7 steps (accepted 4, not 5); at k = 3 and k = 7 the hole - a zero key with a zero value in
    a fresh cache - does not move an argmax of this trained model and the counters stay as they are.  So the assistant's cache is also looked at
    directly: every slot of an emitted token but the last holds a key in every layer.

    The last two assertions rest on decisive argmaxes, because the draft runs the single-row chain and the verify forward the batched one.  The CPU oracle
    (fp32, teacher-forced on the golden ids) gives the top-1 / top-2 gap of the 12 positions used here as 6.31 x the logit bar of tests/_tol.py at the
    smallest (token 6; the others 8.57 .. 15.95), against the 2 x the rule asks for: all 12 tokens are kept.  (Of the golden's 24 tokens the smallest is
    2.73 x, at token 20.)"""
    m, p, audio, plain, gold, twin, _ = _ctx(dev)
    from audio_flamingo_amd import decode_assist as A

    a = m if who == "self" else twin
    states, real_build = [], A.build_state
    monkeypatch.setattr(A, "build_state", lambda *args: (states.append(real_build(*args)), states[-1])[1])   # a look at the draft model's side of the call
    got = m.generate(p, max_new_tokens=NEW, assistant_model=a, num_assistant_tokens=k, use_graph=use_graph, **audio)
    monkeypatch.undo()
    s = m.last_assist_stats
    S0, (Ka, Vta) = p.shape[1], states[0].cache
    assert len(states) == 1 and Ka.shape[2] == S0 + NEW + k + 1
    assert float(Ka[:, 0, S0:S0 + NEW - 1].float().abs().sum(-1).min()) > 0, "a cache slot of an emitted token holds no key: the draft model ran behind a hole"
    assert float(Vta[:, 0, :, :, S0:S0 + NEW - 1].float().abs().sum((1, 2)).min()) > 0
    print("assisted, same weights:", k, who, use_graph, s)
    assert torch.equal(got, plain) and got[0, p.shape[1]:].tolist() == gold, (k, who, got[0, p.shape[1]:].tolist(), gold)
    other = m.generate(p, max_new_tokens=NEW, assistant_model=a, num_assistant_tokens=k, use_graph=not use_graph, **audio)
    assert torch.equal(other, got) and {x: v for x, v in m.last_assist_stats.items() if x != "launched"} == {x: v for x, v in s.items() if x != "launched"}
    assert s["emitted"] == NEW and s["rejecting"] == 0 and s["accepted"] == s["emitted"] - 1 - s["steps"], s
    assert s["steps"] == -(-(NEW - 1) // (k + 1)) and s["drafted"] == k * s["steps"] and s["launched"] >= s["steps"], s
    m.generate(p, max_new_tokens=2, **audio)
    assert m.last_assist_stats is None


@pytest.mark.parametrize("k", [1, 4])
def test_a_poor_assistant_is_rejected_and_the_ids_stay(dev, k):
    m, p, audio, plain, gold, _, poor = _ctx(dev)
    assert (poor.H, poor.dec_layers, poor.V) == (m.H // 2, 1, m.V) and poor._chain_ok(1)
    got = m.generate(p, max_new_tokens=NEW, assistant_model=poor, num_assistant_tokens=k, use_graph=True, **audio)
    s = m.last_assist_stats
    print("assisted, poor assistant:", k, s)
    assert torch.equal(got, plain), (k, got[0, p.shape[1]:].tolist(), gold)
    assert s["rejecting"] > 0 and s["emitted"] == NEW and s["accepted"] == s["emitted"] - 1 - s["steps"], s
    eager = m.generate(p, max_new_tokens=NEW, assistant_model=poor, num_assistant_tokens=k, use_graph=False, **audio)
    assert torch.equal(eager, got)
    m.assist_on_device = False
    try:
        host = m.generate(p, max_new_tokens=NEW, assistant_model=poor, num_assistant_tokens=k, **audio)
        hs = m.last_assist_stats
    finally:
        del m.assist_on_device
    assert torch.equal(host, got), (k, host[0, p.shape[1]:].tolist(), got[0, p.shape[1]:].tolist())
    assert hs["emitted"] == NEW and hs["launched"] == hs["steps"], hs


def test_host_route_with_the_same_weights_and_an_assistant_outside_the_chain(dev):
    m, p, audio, plain, gold, twin, _ = _ctx(dev)
    m.assist_on_device = False
    try:
        host = m.generate(p, max_new_tokens=NEW, assistant_model=twin, num_assistant_tokens=3, **audio)
        hs = m.last_assist_stats
    finally:
        del m.assist_on_device
    assert torch.equal(host, plain) and hs["rejecting"] == 0 and hs["accepted"] == NEW - 1 - hs["steps"], hs
    # a geometry the single-sequence chain does not take (decode_chain off for the assistant): the host route, by itself
    twin.decode_chain = False
    try:
        assert not twin._chain_ok(1)
        got = m.generate(p, max_new_tokens=NEW, assistant_model=twin, num_assistant_tokens=3, **audio)
        s = m.last_assist_stats
    finally:
        del twin.decode_chain
    assert torch.equal(got, plain) and s["launched"] == s["steps"] and s["accepted"] > 0, s


def test_an_eos_inside_the_generated_span(dev):
    m, p, audio, plain, gold, twin, poor = _ctx(dev)
    at = 6
    assert gold[at] not in gold[:at]
    used = set(p.flatten().tolist()) | set(gold)
    unused = next(i for i in range(1, 1000) if i not in used)
    for eos in ([unused, gold[at]], gold[at]):
        want = m.generate(p, max_new_tokens=NEW, eos_token_id=eos, **audio)
        if isinstance(eos, list):   # the stop launch: the reference's shape - the sequence ends at the eos token
            assert want.shape[1] == p.shape[1] + at + 1
        else:                       # one eos id: the plain call learns of the end at its poll and pads behind it
            assert want[0, p.shape[1] + at + 1:].tolist() == [gold[at]] * (want.shape[1] - p.shape[1] - at - 1)
            want = want[:, :p.shape[1] + at + 1]
        assert want[0, p.shape[1]:].tolist() == gold[:at + 1]
        for a, k in ((twin, 3), (twin, 7), (poor, 3)):
            for ug in (False, True):
                got = m.generate(p, max_new_tokens=NEW, eos_token_id=eos, assistant_model=a, num_assistant_tokens=k, use_graph=ug, **audio)
                s = m.last_assist_stats
                assert torch.equal(got, want), (eos, k, ug, got[0, p.shape[1]:].tolist())
                assert s["emitted"] == at + 1 and s["launched"] == 7 > s["steps"], s   # the steps behind the end (up to the poll in front of step 8) changed nothing
    # the eos as token 0: every step runs behind the end
    got = m.generate(p, max_new_tokens=NEW, eos_token_id=gold[0], assistant_model=twin, num_assistant_tokens=3, **audio)
    assert got[0, p.shape[1]:].tolist() == gold[:1] and m.last_assist_stats["steps"] == 0


def _spy(monkeypatch):
    from audio_flamingo_amd import _lib

    names, real = [], _lib.call
    monkeypatch.setattr(_lib, "call", lambda name, *a: (names.append(name), real(name, *a))[1])
    return names


NEW_NAMES = ("afk_assist_begin", "afk_assist_stage")


@pytest.mark.parametrize("k", [1, 4])
def test_launches_of_a_captured_step(dev, k, monkeypatch):
    m, p, audio, plain, gold, _, poor = _ctx(dev)
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
    got = m.generate(p, max_new_tokens=NEW, assistant_model=poor, num_assistant_tokens=k, use_graph=True, **audio)
    assert len(marks) == 2 and torch.equal(got, plain)
    step = Counter(names[marks[0]:marks[1]])
    La, L_ = poor.dec_layers, m.dec_layers
    assert La != L_
    # the assistant: k selections, k + 1 passes over its layers on the single-sequence chain
    assert step["afk_decode_chain_lm_head"] == k and step["afk_decode_select_greedy"] == k and step["afk_decode_chain_qkv"] == (k + 1) * La, step
    assert step["afk_decode_chain_gate_up"] == (k + 1) * La and step["afk_decode_chain_linear_residual"] == 2 * (k + 1) * La, step
    assert step["afk_assist_begin"] == 1 and step["afk_assist_stage"] == 1 and step["afk_lookup_accept"] == 1 and step["afk_lookup_draft"] == 0, step
    # the target: one verify forward of k + 1 rows on the batched chain
    assert step["afk_decode_chain_qkv_norm_batched"] == L_ and step["afk_decode_chain_lm_head_norm_batched"] == 1, step
    assert step["afk_attn_decode_fused"] == (k + 1) * La + L_, step
    order = names[marks[0]:marks[1]]
    assert order[0] == "afk_assist_begin" and order[-1] == "afk_lookup_accept" and order.index("afk_assist_stage") == 1 + (k + 1) * 5 * La + 2 * k, order


def test_without_an_assistant_the_launch_list_is_the_recorded_one(dev, monkeypatch):
    """assistant_model=None: none of the new names, and launch for launch the list recorded in tests/golden/generate_trace.json for the plain greedy call"""
    m, p, audio, plain, gold, _, _ = _ctx(dev)
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "generate_trace.json")) as f:
        book = json.load(f)
    for mode, kw in (("greedy_graph", dict(use_graph=True)), ("greedy_eager", dict(use_graph=False))):
        names = _spy(monkeypatch)
        got = m.generate(p, max_new_tokens=NEW, assistant_model=None, num_assistant_tokens=4, **kw, **audio)
        monkeypatch.undo()
        want = [book["names"][i] for i in book["modes"][mode]["calls"]]
        assert not any(n in NEW_NAMES for n in names) and names == want, (mode, len(names), len(want))
        assert got[0, p.shape[1]:].tolist() == book["modes"][mode]["ids"][0] and m.last_assist_stats is None


def test_refusals_the_vocabulary_and_a_left_padded_prompt(dev):
    from transformers import GenerationConfig

    from audio_flamingo_amd._lib import AfkError

    m, p, audio, plain, gold, twin, poor = _ctx(dev)
    kw = dict(max_new_tokens=4, assistant_model=twin, **audio)
    for extra, word in ((dict(do_sample=True), "do_sample=True"), (dict(num_beams=2), "num_beams > 1"), (dict(repetition_penalty=1.2), "logits processors"),
                        (dict(logits_processor=[lambda i, s: s]), "logits processors"), (dict(streamer=object()), "streamer="),
                        (dict(stopping_criteria=[lambda i, s: False]), "stopping_criteria="), (dict(return_dict_in_generate=True), "return_dict_in_generate"),
                        (dict(output_scores=True, return_dict_in_generate=True), "output_scores"), (dict(share_prompt=True), "share_prompt=True"),
                        (dict(decode_weights="fp8"), "decode_weights='fp8'"), (dict(guidance_scale=2.0), "assistant_model="),
                        (dict(prompt_lookup_num_tokens=3), "prompt_lookup_num_tokens="), (dict(use_cache=False), "use_cache=False"),
                        (dict(num_assistant_tokens=32), "at most 31")):
        with pytest.raises(AfkError, match=word):
            m.generate(p, **dict(kw, **extra))
    cache = m.generate(p, max_new_tokens=2, return_dict_in_generate=True, **audio).past_key_values
    with pytest.raises(AfkError, match="assistant_model.*past_key_values="):
        m.generate(torch.cat([p, plain[:, p.shape[1]:p.shape[1] + 3]], 1), past_key_values=cache, max_new_tokens=4, assistant_model=twin)
    for bad in (0, -2):
        with pytest.raises(ValueError, match="num_assistant_tokens"):
            m.generate(p, **dict(kw, num_assistant_tokens=bad))
    with pytest.raises(ValueError, match="integer"):
        m.generate(p, **dict(kw, num_assistant_tokens=2.5))
    with pytest.raises(ValueError, match="batch_size = 1"):
        m.generate(torch.cat([p, p]), max_new_tokens=4, assistant_model=twin)
    with pytest.raises(AfkError, match="assistant_model.*AudioFlamingo3ForConditionalGeneration"):
        m.generate(p, **dict(kw, assistant_model=object()))
    with pytest.raises(AfkError, match="max_position_embeddings"):
        m.generate(p, **dict(kw, max_new_tokens=4096))
    # another vocabulary: both row counts named
    other = _poor(dev, vocab_size=1088)
    with pytest.raises(AfkError, match=r"embedding rows \(1088\).*\(1024\)"):
        m.generate(p, **dict(kw, assistant_model=other))
    # the class defaults on: the assisted call takes the unshared bf16 route, silently
    m.share_prompt_cache, m.decode_weight_dtype = True, "fp8"
    try:
        got = m.generate(p, max_new_tokens=NEW, assistant_model=twin, num_assistant_tokens=3, **audio)
        assert torch.equal(got, plain) and m.last_w8_stats is None and m.last_share_stats is None and m.last_assist_stats["rejecting"] == 0
    finally:
        del m.share_prompt_cache, m.decode_weight_dtype
        m.drop_decode_weights()
    # k from the assistant's generation config
    twin.generation_config = GenerationConfig(num_assistant_tokens=2)
    try:
        got = m.generate(p, max_new_tokens=NEW, assistant_model=twin, **audio)
        assert torch.equal(got, plain) and m.last_assist_stats["drafted"] == 2 * m.last_assist_stats["steps"]
    finally:
        del twin.generation_config
    # the golden prompt as a left-padded single row (nine pad ids in front, masked): both models see the mask, so slots and positions agree
    S0 = p.shape[1] + 9
    ids = torch.cat([torch.zeros((1, 9), dtype=p.dtype, device=dev), p], 1)
    att = torch.cat([torch.zeros((1, 9), dtype=torch.long, device=dev), torch.ones_like(p)], 1)
    want = m.generate(ids, attention_mask=att, max_new_tokens=NEW, **audio)
    assert want[0, S0:].tolist() == gold
    for a in (twin, poor):
        for ug in (False, True):
            got = m.generate(ids, attention_mask=att, max_new_tokens=NEW, assistant_model=a, num_assistant_tokens=3, use_graph=ug, **audio)
            assert torch.equal(got, want), (a is twin, ug, got[0, S0:].tolist(), gold)
            assert m.last_assist_stats["emitted"] == NEW and (a is poor or m.last_assist_stats["rejecting"] == 0)

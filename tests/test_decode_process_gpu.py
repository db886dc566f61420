"""GPU: afk_decode_process (csrc/decode_process.hip) against the reference's own logits processors run on CPU on the same tensors, and generate() with
repetition_penalty / no_repeat_ngram_size / min_new_tokens / suppress_tokens / begin_suppress_tokens on it.  Every comparison is exact - bit-equal floats
(one IEEE fp32 multiply or divide, or a store of -inf, on identical inputs) or equal ids."""
import os
from types import SimpleNamespace

import pytest
import torch

from tests import _logits_process_ref as R

pytestmark = pytest.mark.gpu


def _spec(kw):
    from audio_flamingo_amd.decode_process import ProcessSpec

    return ProcessSpec(penalty=kw["penalty"], ngram=kw["ngram"], min_new_tokens=kw["min_new_tokens"], eos=tuple(kw["eos"]), suppress=tuple(kw["suppress"]),
                       begin_suppress=tuple(kw["begin_suppress"]))


def _device_process(dev, logits, ids, S0, t, kw, *, pad_logits=0, pad_hist=0, use_step_base=False):
    """the device's row for token t: the state is built from the prompt ids[:, :S0]; the t selected tokens ids[:, S0:] reach the history the way they do in
    generate() - one launch per step appends the previous one from the next-token buffer (the steps before t run on a scratch row)"""
    from audio_flamingo_amd import decode_process as P

    Bn, V = logits.shape
    ps = P.build_state(_spec(kw), ids[:, :S0].to(dev), t + pad_hist, V)
    assert ps["hist"].shape[1] == S0 + t + pad_hist
    buf = torch.full((Bn, V + pad_logits), 7.0, device=dev)
    row = buf[:, :V]
    nxt = torch.zeros(Bn, device=dev, dtype=torch.int64)
    base = torch.zeros(1, device=dev, dtype=torch.int32)
    for s in range(t + 1):
        row.copy_(logits)
        step = dict(step_base=base.fill_(s + 5), step_off=-5) if use_step_base else dict(step_off=s)
        if s:
            nxt.copy_(ids[:, S0 + s - 1])
        P.apply(ps, row, next_token=nxt, **step)
    assert torch.equal(ps["hist"][:, : S0 + t].cpu().long(), ids) and (pad_logits == 0 or bool((buf[:, V:] == 7.0).all()))
    return row.cpu(), ps


@pytest.mark.parametrize("V", R.VS)
def test_grid_equals_the_reference_classes_bit_for_bit(dev, V):
    for k, (V_, S0, t, g) in enumerate(R.grid()):
        if V_ != V:
            continue
        logits, ids, kw = R.case(V, S0, t, g)
        want = R.reference_chain(logits, ids, S0, **kw)
        got, _ = _device_process(dev, logits, ids, S0, t, kw, use_step_base=bool(k & 1))
        assert torch.equal(R.bits(got), R.bits(want)), (V, S0, t, g, kw)


def test_af3_vocabulary_long_history_and_padded_strides(dev):
    """V = 152 064, B = 2, a history of 1 024 ids with the 750-fold <sound> id in it; ld_logits > V and ld_hist > n"""
    V, S0, t, sound = 152064, 1021, 3, 151669
    gen = torch.Generator().manual_seed(11)
    ids = torch.randint(0, V, (2, S0 + t), generator=gen)
    ids[:, 100:850] = sound
    ids[0, 900:903] = ids[0, -3:]                       # a repeated trigram in row 0: its continuation is banned
    ids[1, -1] = ids[1, 5]
    logits = (torch.randn((2, V), generator=gen) * 4.0).to(torch.bfloat16).float()
    logits[:, sound] = torch.tensor([3.0, -2.0])
    for g, pen in ((3, 1.05), (1, 0.7), (0, 1.3)):
        kw = dict(penalty=pen, ngram=g, suppress=(V - 1, 17), begin_suppress=(0,), eos=(151645, 151643), min_new_tokens=8)
        want = R.reference_chain(logits, ids, S0, **kw)
        got, _ = _device_process(dev, logits, ids, S0, t, kw, pad_logits=37, pad_hist=9, use_step_base=g == 3)
        assert torch.equal(R.bits(got), R.bits(want)), (g, pen)
        if g == 3:
            assert want[0, ids[0, 903]] == float("-inf") and float(want[0, sound]) == float(torch.tensor(3.0) / torch.tensor(1.05))


def test_six_consecutive_steps_on_static_buffers(dev):
    """the test dictates the fed tokens: a repeat of a prompt id (7), a repeat of a generated id (20), and a token that closes a repeated bigram (3, 7 -> the id
    that followed it is banned); after every step the row equals the reference classes on the grown id matrix, and running a step twice changes nothing"""
    from audio_flamingo_amd import decode_process as P

    V, S0 = 67, 5
    prompt = torch.tensor([[3, 7, 3, 9, 4], [1, 1, 2, 1, 1]])
    fed = torch.tensor([[7, 20, 20, 3, 7], [2, 1, 1, 2, 1]])
    kw = dict(penalty=1.3, ngram=3, suppress=(66,), begin_suppress=(0,), eos=(5,), min_new_tokens=4)
    gen = torch.Generator().manual_seed(5)
    rows = (torch.randn((6, 2, V), generator=gen) * 4.0).to(torch.bfloat16).float()
    ps = P.build_state(_spec(kw), prompt.to(dev), 6, V)
    logits, nxt, step = torch.empty((2, V), device=dev), torch.zeros(2, device=dev, dtype=torch.int64), torch.zeros(1, device=dev, dtype=torch.int32)
    for s in range(6):
        ids = torch.cat([prompt, fed[:, :s]], 1)
        want = R.reference_chain(rows[s], ids, S0, **kw)
        if s:
            nxt.copy_(fed[:, s - 1])
        step.fill_(S0 + s - 1)                          # generate()'s convention: the cache slot, with step_off = 1 - S0
        for _ in range(2):
            logits.copy_(rows[s])
            P.apply(ps, logits, next_token=nxt, step_base=step, step_off=1 - S0)
            assert torch.equal(R.bits(logits.cpu()), R.bits(want)), s
            assert torch.equal(ps["hist"][:, : S0 + s].cpu().long(), ids)
        assert ps["hist"][:, S0 + s:].eq(0).all()
        if s == 5:
            assert want[0, 3] == float("-inf")           # (3, 7) occurred at the start of the prompt, followed by 3
    seen = ps["seen"].cpu().long() & 0xFFFFFFFF
    for b in range(2):
        marked = {32 * w + i for w in range(seen.shape[1]) for i in range(32) if (int(seen[b, w]) >> i) & 1}
        assert marked == set(torch.cat([prompt, fed], 1)[b].tolist())


def test_greedy_selection_equals_the_greedy_launch(dev):
    """select: token, tokens_out[state[2] + tok_off], state and x_out exactly as afk_decode_select_greedy leaves them for a row whose argmax is that token; the
    raw row's maximum is suppressed, and a second row holds an exact tie of the processed maximum (lowest id wins)"""
    from audio_flamingo_amd import _lib, ops
    from audio_flamingo_amd import decode_process as P

    V, H, S0, t = 1000, 64, 40, 6
    gen = torch.Generator().manual_seed(8)
    emb = torch.randn(V, H, generator=gen).to(torch.bfloat16).to(dev)
    prompt = torch.randint(0, 50, (1, S0 + t - 1), generator=gen)     # the tokens selected before t - 1 are part of the state's prompt here
    prev = 33
    ids = torch.cat([prompt, torch.tensor([[prev]])], 1)
    kw = dict(penalty=1.3, ngram=2, suppress=(777,), begin_suppress=(), eos=(), min_new_tokens=0)
    state0 = torch.tensor([0, S0 + t, S0 + t - 1, S0 + t - 1], dtype=torch.int32)
    tok_off = 1 - S0
    for tie in (False, True):
        x = (torch.randn(V, generator=gen) * 4.0).to(torch.bfloat16).float()
        x[777] = 90.0                                                  # the raw maximum is banned
        if tie:
            x[612] = x[204] = 60.0                                     # ids outside the history (ids < 50): untouched by the penalty
        want_row = R.reference_chain(x[None], ids, S0, **kw)[0]
        want = int(torch.nonzero(want_row == want_row.max())[0])
        assert want != 777 and (not tie or (want == 204 and want_row[612] == want_row[204]))
        ps = P.build_state(_spec(kw), prompt.to(dev), 1, V)
        st, toks, x_out = state0.to(dev), torch.zeros(16, dtype=torch.int64, device=dev), torch.zeros(H, dtype=torch.bfloat16, device=dev)
        nxt = torch.tensor([prev], dtype=torch.int64, device=dev)
        row = x[None].to(dev)
        ops.decode_process(row, ps["hist"], ps["seen"], S0=S0 + t - 1, penalty=1.3, ngram=2, suppress=ps["suppress"], next_token=nxt, step_base=st[2:3],
                           step_off=2 - S0 - t, select=True, tokens_out=toks, tok_off=tok_off, state=st, emb=emb, x_out=x_out)   # token 1 of this state
        assert torch.equal(R.bits(row.cpu()[0]), R.bits(want_row)) and int(nxt[0]) == want
        y = x.clone()
        y[want] = 100.0
        pv, pi = y.view(V // 8, 8).max(-1)
        pv, pi = pv.to(dev), (pi + 8 * torch.arange(V // 8)).to(torch.int32).to(dev)
        st2, toks2, x2, nxt2 = state0.to(dev), torch.zeros_like(toks), torch.zeros_like(x_out), torch.zeros(1, dtype=torch.int64, device=dev)
        _lib.call("afk_decode_select_greedy", pv.data_ptr(), pi.data_ptr(), V // 8, nxt2.data_ptr(), toks2.data_ptr(), tok_off, st2.data_ptr(), emb.data_ptr(),
                  emb.stride(0), H, x2.data_ptr(), ops._stream())
        assert torch.equal(nxt, nxt2) and torch.equal(toks, toks2) and int(toks[t]) == want and torch.equal(st, st2) and torch.equal(x_out, x2)
        assert st.tolist() == [0, S0 + t + 1, S0 + t, S0 + t] and torch.equal(x_out, emb[want])
    # +inf wins at its lowest id; a row with no finite logit answers 0
    for x, want in ((torch.full((V,), float("-inf")), 0), (torch.cat([torch.zeros(500), torch.full((500,), float("inf"))]), 500)):
        ps = P.build_state(_spec(dict(kw, suppress=())), prompt.to(dev), 1, V)
        st, x_out, nxt = state0.to(dev), torch.zeros(H, dtype=torch.bfloat16, device=dev), torch.tensor([prev], dtype=torch.int64, device=dev)
        ops.decode_process(x[None].to(dev), ps["hist"], ps["seen"], S0=S0 + t - 1, next_token=nxt, step_off=1, select=True, state=st, emb=emb, x_out=x_out)
        assert int(nxt[0]) == want


def test_entry_point_refuses_bad_arguments(dev):
    from audio_flamingo_amd import ops
    from audio_flamingo_amd._lib import AfkError

    x, hist, seen = torch.zeros((2, 40), device=dev), torch.zeros((2, 8), device=dev, dtype=torch.int32), torch.zeros((2, 2), device=dev, dtype=torch.int32)
    nxt = torch.zeros(2, device=dev, dtype=torch.int64)
    for bad in (dict(penalty=0.0), dict(penalty=-1.0), dict(ngram=-1), dict(step_off=5), dict(step_off=1, next_token=None), dict(select=True)):
        with pytest.raises(AfkError):
            ops.decode_process(x, hist, seen, **dict(dict(S0=4, next_token=nxt), **bad))
    with pytest.raises(AfkError):
        ops.decode_process(x, hist, seen[:, :1], S0=4)
    ops.decode_process(x, hist, seen, S0=4, next_token=nxt, step_off=4)       # S0 + t == ld_hist: the last slot
    assert not x.any()


# ---------------------------------------------------------------------------------------------- generate()
A_, B_, C_ = 144, 51, 165          # tokens 3, 0 and 5 of the golden greedy continuation of case A (tests/golden/tiny64_caseA.pt)
FIVE = dict(repetition_penalty=1.3, no_repeat_ngram_size=2, suppress_tokens=[A_], begin_suppress_tokens=[B_], min_new_tokens=10)


def _five_reference(dev, S0, eos):
    return R.reference_chain(None, None, S0, penalty=1.3, ngram=2, suppress=(A_,), begin_suppress=(B_,), eos=(eos,) if eos is not None else (), min_new_tokens=10,
                             device=dev)


def _case_a(dev):
    from tests.test_sampler_gpu import _case_a as case_a

    return case_a(dev)


def test_golden_continuation_holds_the_banned_tokens():
    from tests.test_model_gpu import G, N_GEN

    cont = torch.load(os.path.join(G, "tiny64_caseA.pt"))["generate"][0, -N_GEN:].tolist()
    assert (cont[0], cont[3], cont[5]) == (B_, A_, C_)


@pytest.mark.parametrize("mode", ["greedy", "sampled"])
def test_generate_device_path_equals_the_hooks_path_with_the_reference_classes(dev, mode):
    from tests.test_sampler_gpu import SAMPLED

    m, p, audio = _case_a(dev)
    S0 = p.shape[1]
    how = dict(SAMPLED) if mode == "sampled" else dict(max_new_tokens=12)
    runs = [m.generate(p, use_graph=False, eos_token_id=C_, **FIVE, **audio, **how), m.generate(p, use_graph=True, eos_token_id=C_, **FIVE, **audio, **how),
            m.generate(p, logits_processor=_five_reference(dev, S0, C_), eos_token_id=C_, **audio, **how)]
    new = runs[0][0, S0:].tolist()
    print(mode, [r[0, S0:].tolist() for r in runs])
    assert torch.equal(runs[0], runs[1]) and torch.equal(runs[0], runs[2])
    assert A_ not in new and C_ not in new[:10]
    if mode == "greedy":
        assert new[0] != B_ and len(new) == 12


@pytest.mark.parametrize("mode", ["greedy", "sampled"])
def test_generate_left_padded_batch_equals_the_hooks_path(dev, mode):
    from tests.test_sampler_gpu import SAMPLED

    m, _, _ = _case_a(dev)
    g = torch.Generator().manual_seed(3)
    lens = (40, 23, 31)
    ids, att = torch.zeros((3, 40), dtype=torch.long), torch.zeros((3, 40), dtype=torch.long)
    for i, n in enumerate(lens):
        ids[i, 40 - n:] = torch.randint(0, 256, (n,), generator=g)
        att[i, 40 - n:] = 1
    how = dict(SAMPLED) if mode == "sampled" else dict(max_new_tokens=12)
    kw = dict(attention_mask=att.to(dev), **how)
    runs = [m.generate(ids.to(dev), use_graph=False, **FIVE, **kw), m.generate(ids.to(dev), use_graph=True, **FIVE, **kw),
            m.generate(ids.to(dev), logits_processor=_five_reference(dev, 40, None), **kw)]
    assert runs[0].shape == (3, 52) and torch.equal(runs[0], runs[1]) and torch.equal(runs[0], runs[2])
    assert not bool((runs[0][:, 40:] == A_).any()) and not bool((runs[0][:, 40] == B_).any())


def test_history_reaches_the_kernel_from_the_prompt_and_the_generated_tokens(dev):
    """a text-only prompt holding every id 0 .. 1022 once except three: with no_repeat_ngram_size=1 the three new tokens are exactly those three, each once.
    Id 1023, the audio token, cannot stand in a text-only prompt, so the n-gram step never bans it (and the tiny model does select it: [1023, 400, 901]
    without the next line's list); suppress_tokens takes it out, which leaves the three ids as the only finite logits."""
    m, _, _ = _case_a(dev)
    X = {77, 400, 901}
    perm = torch.randperm(1023, generator=torch.Generator().manual_seed(2)).tolist()
    p = torch.tensor([[i for i in perm if i not in X]], device=dev)
    assert p.shape[1] == 1020
    out = m.generate(p, no_repeat_ngram_size=1, suppress_tokens=[1023], max_new_tokens=3)
    print(out[0, 1020:].tolist())
    assert sorted(out[0, 1020:].tolist()) == sorted(X)


def test_generation_config_supplies_the_processors_and_a_keyword_wins(dev):
    m, p, audio = _case_a(dev)
    S0 = p.shape[1]
    assert int(m.generate(p, max_new_tokens=4, **audio)[0, S0]) == B_
    out = m.generate(p, max_new_tokens=4, generation_config=SimpleNamespace(suppress_tokens=[B_]), **audio)
    assert int(out[0, S0]) != B_
    other = int(out[0, S0])
    out = m.generate(p, max_new_tokens=4, suppress_tokens=[other], generation_config=SimpleNamespace(suppress_tokens=[B_]), **audio)
    assert int(out[0, S0]) == B_


def test_one_captured_graph_and_selection_on_the_device(dev, monkeypatch):
    from tests.test_sampler_gpu import SAMPLED

    m, p, audio = _case_a(dev)
    captured = []
    real = torch.cuda.graph

    class Counting(real):
        def __init__(self, *a, **k):
            captured.append(1)
            super().__init__(*a, **k)

    monkeypatch.setattr(torch.cuda, "graph", Counting)
    out = m.generate(p, repetition_penalty=1.3, max_new_tokens=12, **audio)
    assert out.shape[1] == p.shape[1] + 12 and len(captured) == 1

    def refuse(*a, **k):
        raise AssertionError("token selection went through torch")

    for owner in (torch, torch.Tensor):
        monkeypatch.setattr(owner, "multinomial", refuse)
        monkeypatch.setattr(owner, "sort", refuse)
    out = m.generate(p, repetition_penalty=1.3, no_repeat_ngram_size=2, **audio, **SAMPLED)
    assert out.shape[1] == p.shape[1] + 12 and len(captured) == 2


def test_nothing_active_enqueues_what_it_did(dev, monkeypatch):
    """default arguments: no processing launch, no logits row - the partial-argmax lm_head path"""
    from audio_flamingo_amd import _lib

    m, p, audio = _case_a(dev)
    names = []
    real = _lib.call

    def spy(name, *a):
        names.append(name)
        return real(name, *a)

    monkeypatch.setattr(_lib, "call", spy)
    m.generate(p, max_new_tokens=4, use_graph=False, repetition_penalty=1.0, no_repeat_ngram_size=0, min_new_tokens=3, **audio)   # min_new_tokens without an EOS id: inactive
    assert "afk_decode_process" not in names and "afk_decode_select_greedy" in names
    names.clear()
    m.generate(p, max_new_tokens=4, use_graph=False, repetition_penalty=1.3, **audio)
    assert names.count("afk_decode_process") == 4 and "afk_decode_select_greedy" not in names


def test_out_of_scope_combinations_raise(dev):
    from audio_flamingo_amd._lib import AfkError

    m, p, audio = _case_a(dev)
    for how in (dict(num_beams=2), dict(use_cache=False)):
        for five in (dict(repetition_penalty=1.3), dict(no_repeat_ngram_size=2), dict(min_new_tokens=2, eos_token_id=C_), dict(suppress_tokens=[A_]),
                     dict(begin_suppress_tokens=[B_])):
            with pytest.raises(AfkError, match="KV cache only"):
                m.generate(p, max_new_tokens=4, **how, **five, **audio)
    with pytest.raises(ValueError, match="strictly positive float"):
        m.generate(p, max_new_tokens=4, repetition_penalty=0.0, **audio)

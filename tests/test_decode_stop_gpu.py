"""GPU: afk_decode_stop (csrc/decode_stop.hip) against the plain-integer restatement of its contract (tests/_stop_ref.py, which tests/test_decode_stop_cpu.py
pins to the reference's StopStringCriteria / EosTokenCriteria), and generate() with an eos list and stop_strings= / tokenizer= on it: the eager, graph-replayed
and hook-driven loops against each other, against the existing hook route running the reference's own criteria classes, and against the live fp32 reference on
the host.  Every comparison is of integers or of bits."""
import os

import numpy as np
import pytest
import torch

from tests import _stop_ref as R

pytestmark = pytest.mark.gpu
_CACHE = {}
NEW = 12
BEYOND = 5000
FLAGS = dict(return_dict_in_generate=True, output_scores=True, output_logits=True)


def _grid_table():
    """the 'different lengths' stop set of the CPU grid: table for the device (torch) and for the restatement (numpy)"""
    if "table" not in _CACHE:
        from audio_flamingo_amd import decode_stop as D
        from tests.test_decode_stop_cpu import PIECES

        tok = R.tiny_tokenizer(PIECES, vocab_size=64)
        t = D.build_table(tok, ["abc", "\n\n", "User:"])
        _CACHE["table"] = (t, dict(table=t["table"].numpy().astype(np.int64), P=t["P"], E=t["E"], S=t["S"], target=t["target_lens"].tolist(), W=t["W"]))
    return _CACHE["table"]


POOL = [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 12, 18, BEYOND]   # ids of the stop set's tokens, one that belongs to no string, one above the table's rows
EOS = (18, 2)
PAD = 11
STEPS = 6


def _device_state(dev, ids_np, ld, t):
    big = torch.full((ids_np.shape[0], ld), -7, dtype=torch.int32)
    big[:, : ids_np.shape[1]] = torch.from_numpy(ids_np)
    B = ids_np.shape[0]
    return dict(ids=big.to(dev), stop_at=torch.full((B,), R.INT_MAX, device=dev, dtype=torch.int32), status=torch.tensor([-1, B], device=dev, dtype=torch.int32),
                eos=torch.tensor(EOS, device=dev, dtype=torch.int32), table=t["table"].to(dev), target_lens=t["target_lens"].to(dev))


def _launch(d, nxt, t, S0, *, tab, feed_pad, step_base=None, step_off=None, max_new=STEPS):
    from audio_flamingo_amd import ops

    ops.decode_stop(nxt, d["ids"], d["stop_at"], S0=S0, max_new=max_new, status=d["status"], step_base=step_base, step_off=t if step_off is None else step_off,
                    eos=d["eos"], pad=PAD, feed_pad=feed_pad, table=d["table"], P=tab["P"], E=tab["E"], S=tab["S"], target_lens=d["target_lens"], W=tab["W"])


def _same(d, nxt, ref):
    ids, stop_at, status, rn = ref
    S0n = ids.shape[1]
    got = d["ids"].cpu().numpy()
    return (np.array_equal(got[:, :S0n], ids) and bool((got[:, S0n:] == -7).all()) and d["stop_at"].cpu().tolist() == stop_at.tolist()
            and d["status"].cpu().tolist() == status.tolist() and nxt.cpu().tolist() == rn.tolist())


@pytest.mark.parametrize("S0", [1, 2, 8])    # W = 5 for this stop set: histories shorter than W, and W + 3
@pytest.mark.parametrize("B", [1, 3, 17])    # 17: more rows than the block has waves
def test_kernel_equals_the_restatement_over_six_steps(dev, B, S0):
    t, tab = _grid_table()
    assert tab["W"] == 5 and S0 in (1, 2, tab["W"] + 3)
    for feed_pad in (False, True):
        gen = np.random.default_rng(100 * B + 10 * S0 + int(feed_pad))
        prompt = gen.choice(np.asarray(POOL), size=(B, S0))
        toks = gen.choice(np.asarray(POOL), size=(B, STEPS))
        ids = np.full((B, S0 + STEPS), -7, dtype=np.int32)
        ids[:, :S0] = prompt
        stop_at, status = np.full(B, R.INT_MAX, dtype=np.int32), np.array([-1, B], dtype=np.int32)
        d = _device_state(dev, ids, S0 + STEPS + 5, t)                        # a padded ld_ids: five sentinel columns behind the row
        nxt = torch.zeros(B, device=dev, dtype=torch.int64)
        rn = np.zeros(B, dtype=np.int64)
        base = torch.zeros(1, device=dev, dtype=torch.int32)
        use_base = bool((B + S0 + int(feed_pad)) & 1)
        for s in range(STEPS):
            rn[:] = toks[:, s]
            nxt.copy_(torch.from_numpy(rn))
            how = dict(step_base=base.fill_(s + 3), step_off=-3) if use_base else {}   # a device step_base with a nonzero step_off
            _launch(d, nxt, s, S0, tab=tab, feed_pad=feed_pad, **how)
            R.step(rn, ids, stop_at, status, s, S0=S0, max_new=STEPS, eos=EOS, pad=PAD, feed_pad=feed_pad, tab=tab)
            assert _same(d, nxt, (ids, stop_at, status, rn)), (B, S0, feed_pad, s)
            if s == 3:   # the same step again: nothing moves
                _launch(d, nxt, s, S0, tab=tab, feed_pad=feed_pad, **how)
                assert _same(d, nxt, (ids, stop_at, status, rn)), (B, S0, feed_pad, "rerun")
        for outside in (STEPS, -1, STEPS + 100):   # a t outside [0, max_new): nothing is written, the sentinels and the status word stay
            _launch(d, nxt, outside, S0, tab=tab, feed_pad=True, step_base=base.fill_(outside), step_off=0)
            assert _same(d, nxt, (ids, stop_at, status, rn)), (B, S0, outside)
        fin = sorted(set(stop_at.tolist()) - {R.INT_MAX})
        print("B", B, "S0", S0, "feed_pad", feed_pad, "stop_at", stop_at.tolist())
        if B == 17:
            assert len(fin) >= 3 and (stop_at < STEPS - 1).any()              # rows finish at different steps, and pad was substituted behind some
            assert bool((ids[stop_at < STEPS - 1, -1] == PAD).all())


def test_kernel_hits_through_the_prompt_and_above_the_table(dev):
    """'User:' = [Us][er:] with 'Us' the prompt's last id; an id above the table's rows matches nothing and breaks a match that runs through it"""
    t, tab = _grid_table()
    for prompt, tok, want in (([0, 12], 10, 0), ([12, BEYOND], 10, R.INT_MAX), ([0, 8], 9, 0), ([8, 9], BEYOND, R.INT_MAX), ([3], 2, 0), ([BEYOND], 5, 0)):
        ids = np.full((1, len(prompt) + 2), -7, dtype=np.int32)
        ids[0, : len(prompt)] = prompt
        d = _device_state(dev, ids, len(prompt) + 2, t)
        nxt = torch.tensor([tok], device=dev)
        _launch(d, nxt, 0, len(prompt), tab=tab, feed_pad=False, max_new=2)
        assert d["stop_at"].tolist() == [want] and R.judge(prompt + [tok], (), tab) == (want == 0), (prompt, tok)
        assert d["status"].tolist() == [0, int(want != 0)]


def test_kernel_refusals(dev):
    from audio_flamingo_amd import _lib, ops
    from audio_flamingo_amd._lib import AfkError

    t, tab = _grid_table()
    d = _device_state(dev, np.zeros((2, 4), dtype=np.int32), 4, t)
    nxt = torch.zeros(2, device=dev, dtype=torch.int64)
    P, E, S, W = tab["P"], tab["E"], tab["S"], tab["W"]
    rows, vec = t["table"].shape
    good = [nxt.data_ptr(), 2, d["ids"].data_ptr(), 4, 2, 2, d["stop_at"].data_ptr(), d["status"].data_ptr(), None, 0, d["eos"].data_ptr(), 2, PAD, 0,
            d["table"].data_ptr(), rows, vec, P, E, S, d["target_lens"].data_ptr(), W, ops._stream()]
    _lib.call("afk_decode_stop", *good)
    for at, value, what in ((0, None, "null pointer"), (2, None, "null pointer"), (6, None, "null pointer"), (5, 3, "ld_ids"), (4, 3, "ld_ids"), (11, -1, "eos"),
                            (10, None, "eos"), (14, None, "null table"), (20, None, "null table"), (16, vec + 1, "vec =="), (17, P + 1, "vec ==")):
        bad = list(good)
        bad[at] = value
        with pytest.raises(AfkError, match=what):
            _lib.call("afk_decode_stop", *bad)
    off = list(good)     # no stop strings: the table may be null
    off[14], off[19], off[20] = None, 0, None
    _lib.call("afk_decode_stop", *off)
    kw = dict(S0=2, max_new=2, status=d["status"], eos=d["eos"], pad=PAD)
    with pytest.raises(AfkError, match="decode_stop"):
        ops.decode_stop(nxt, d["ids"], d["stop_at"], **dict(kw, max_new=3))
    with pytest.raises(AfkError, match="decode_stop"):
        ops.decode_stop(nxt.int(), d["ids"], d["stop_at"], **kw)
    with pytest.raises(AfkError, match="decode_stop"):
        ops.decode_stop(nxt, d["ids"], d["stop_at"], S=S, P=P, E=E, W=W, **kw)
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------- generate()
class _Collect:
    def put(self, v):
        pass

    def end(self):
        pass


def _case_a(dev):
    if "case_a" not in _CACHE:
        from tests.test_model_gpu import G, _gen_prompt, _model

        g = torch.load(os.path.join(G, "tiny64_caseA.pt"))
        m, p = _model(dev), _gen_prompt(g).to(dev)
        audio = dict(input_features=g["feats"][:1].to(dev), input_features_mask=g["fmask"][:1].to(dev))
        _CACHE["case_a"] = (m, p, audio, g, m.generate(p, max_new_tokens=NEW, **audio))   # the plain greedy run the tests take their tokens from
    return _CACHE["case_a"]


def _three_routes(m, p, **kw):
    """[eager, graph-replayed, hook-driven (a streamer)]"""
    return [m.generate(p, use_graph=False, **kw), m.generate(p, use_graph=True, **kw), m.generate(p, streamer=_Collect(), **kw)]


def _unused(seq, n=1):
    """n ids below the audio token that occur nowhere in seq"""
    used = set(int(i) for i in seq.flatten().tolist())
    free = [i for i in range(1, 1023) if i not in used][:n]
    return free[0] if n == 1 else free


def test_eos_list_stops_at_the_seventh_token_on_every_route(dev):
    """(a) fails on the parent: its graph / eager loop compares a tensor with a Python list"""
    m, p, audio, _, plain = _case_a(dev)
    S0 = p.shape[1]
    new = plain[0, S0:].tolist()
    assert len(new) == NEW and new[6] not in new[:6]
    eos = [_unused(plain), new[6]]
    runs = _three_routes(m, p, eos_token_id=eos, max_new_tokens=NEW, **audio)
    for r in runs:
        assert r.shape == (1, S0 + 7) and torch.equal(r, plain[:, : S0 + 7])
    for form in (tuple(eos), torch.tensor(eos)):
        assert torch.equal(m.generate(p, eos_token_id=form, max_new_tokens=NEW, **audio), runs[0])
    from types import SimpleNamespace

    assert torch.equal(m.generate(p, generation_config=SimpleNamespace(eos_token_id=eos), max_new_tokens=NEW, **audio), runs[0])   # Qwen2.5's shipped form
    out = m.generate(p, eos_token_id=eos, max_new_tokens=NEW, **FLAGS, **audio)
    assert torch.equal(out.sequences, runs[0]) and len(out.scores) == len(out.logits) == 7 and out.past_key_values.get_seq_length() == S0 + 6


def _reference_hook_run(m, p, tok, strings, **kw):
    from transformers.generation.stopping_criteria import StoppingCriteriaList, StopStringCriteria

    return m.generate(p, stopping_criteria=StoppingCriteriaList([StopStringCriteria(tokenizer=tok, stop_strings=strings)]), **kw)


def test_stop_strings_equal_the_hook_route_with_the_reference_class(dev):
    """(b) a match that ends inside the 6th token, and one that straddles the prompt's last id"""
    m, p, audio, _, plain = _case_a(dev)
    S0 = p.shape[1]
    new = plain[0, S0:].tolist()
    last = int(p[0, -1])
    assert len(set(new[:6] + [last])) == 7
    tok = R.tiny_tokenizer({new[0]: "A", new[1]: "B", new[2]: "C", new[3]: "Hel", new[4]: "lo", new[5]: " world", last: "Us"})
    kw = dict(max_new_tokens=NEW, **audio)
    want = _reference_hook_run(m, p, tok, ["lo w", "never"], **kw)
    assert want.shape == (1, S0 + 6)
    for r in _three_routes(m, p, stop_strings=["lo w", "never"], tokenizer=tok, **kw):
        assert torch.equal(r, want)
    assert torch.equal(m.generate(p, stop_strings="lo w", tokenizer=tok, **kw), want)
    tok = R.tiny_tokenizer({new[0]: "er: hi", last: "Us"})
    want = _reference_hook_run(m, p, tok, ["User:"], **kw)
    assert want.shape == (1, S0 + 1)
    for r in _three_routes(m, p, stop_strings=["User:"], tokenizer=tok, **kw):
        assert torch.equal(r, want)
    from types import SimpleNamespace

    assert torch.equal(m.generate(p, generation_config=SimpleNamespace(stop_strings=["User:"]), tokenizer=tok, **kw), want)


def _padded_batch(dev):
    g = torch.Generator().manual_seed(3)
    lens = (40, 23, 31)
    ids, att = torch.zeros((3, 40), dtype=torch.long), torch.zeros((3, 40), dtype=torch.long)
    for i, n in enumerate(lens):
        ids[i, 40 - n:] = torch.randint(0, 256, (n,), generator=g)
        att[i, 40 - n:] = 1
    return ids.to(dev), att.to(dev)


def test_left_padded_batch_rows_stop_at_different_steps_with_the_output_flags(dev):
    """(c) two rows finish on an eos id each, the third on a stop string; sequences, and scores / logits bit for bit at every step - those behind a row's stop
    included: both routes feed the pad id to a finished row and run the same launches on it"""
    from transformers.generation.stopping_criteria import EosTokenCriteria, StoppingCriteriaList, StopStringCriteria

    m = _case_a(dev)[0]
    ids, att = _padded_batch(dev)
    kw = dict(attention_mask=att, max_new_tokens=NEW, pad_token_id=0)
    plain = m.generate(ids, **kw)[:, 40:].cpu()
    assert plain.shape == (3, NEW)
    pick = None
    for k0, k1, k2 in ((2, 5, 8), (3, 6, 9), (1, 4, 7), (2, 6, 9), (4, 7, 10)):   # the first choice whose rows finish at three different steps
        eos = [int(plain[0, k0]), int(plain[1, k1])]
        a, b = int(plain[2, k2 - 1]), int(plain[2, k2])
        if a == b or a in eos or b in eos or 0 in eos + [a, b]:   # 0 is the batch's padding id
            continue
        tok = R.tiny_tokenizer({a: "en", b: "d!"})
        tab = R.table_of(StopStringCriteria(tokenizer=tok, stop_strings=["end"]))
        stops = [next((t for t in range(NEW) if R.judge(ids[r].tolist() + plain[r, : t + 1].tolist(), eos, tab)), None) for r in range(3)]
        if None not in stops and len(set(stops)) == 3 and max(stops) < NEW - 1:
            pick = (eos, tok, stops)
            break
    assert pick is not None
    eos, tok, stops = pick
    print("stops", stops)
    n = max(stops) + 1
    crit = StoppingCriteriaList([EosTokenCriteria(eos), StopStringCriteria(tokenizer=tok, stop_strings=["end"])])
    want = m.generate(ids, stopping_criteria=crit, **FLAGS, **kw)   # the parent's hook route, the reference's classes, no eos of its own
    assert want.sequences.shape == (3, 40 + n)
    for r in range(3):
        assert want.sequences[r, 40:].tolist() == plain[r, : stops[r] + 1].tolist() + [0] * (n - stops[r] - 1)
    for out in _three_routes(m, ids, eos_token_id=eos, stop_strings=["end"], tokenizer=tok, **FLAGS, **kw):
        assert torch.equal(out.sequences, want.sequences)
        assert len(out.scores) == len(out.logits) == n and out.past_key_values.get_seq_length() == 40 + n - 1
        for t in range(n):
            assert torch.equal(out.logits[t].view(torch.int32), want.logits[t].view(torch.int32)), t
            assert torch.equal(out.scores[t].view(torch.int32), want.scores[t].view(torch.int32)), t


def test_sampled_decoding_with_a_stop_string_one_seed_one_sequence(dev):
    """(d)"""
    from tests.test_sampler_gpu import SAMPLED

    m, p, audio, _, _ = _case_a(dev)
    S0 = p.shape[1]
    kw = dict(SAMPLED, **audio)
    new = m.generate(p, **kw)[0, S0:].tolist()
    k = next(k for k in range(3, NEW - 1) if new[k] != new[k - 1] and new[k] not in new[:k - 1] and new[k - 1] not in new[:k - 1])
    tok = R.tiny_tokenizer({new[k - 1]: "en", new[k]: "d of"})
    want = _reference_hook_run(m, p, tok, ["end"], **kw)
    assert want.shape == (1, S0 + k + 1) and want[0, S0:].tolist() == new[: k + 1]
    for r in _three_routes(m, p, stop_strings=["end"], tokenizer=tok, **kw):
        assert torch.equal(r, want)
    ids, att = _padded_batch(dev)
    kw = dict(SAMPLED, attention_mask=att, pad_token_id=0)
    new = m.generate(ids, **kw)[:, 40:]
    eos = [int(new[0, 3]), int(new[1, 6])]
    runs = _three_routes(m, ids, eos_token_id=eos, **kw)
    assert torch.equal(runs[0], runs[1]) and torch.equal(runs[0], runs[2]) and runs[0].shape[1] <= 40 + NEW


def test_against_the_live_reference(dev):
    """(e) the reference model in fp32 on the host with eos_token_id=[...], stop_strings= and tokenizer=: the same sequences, shape included"""
    from transformers import AudioFlamingo3ForConditionalGeneration

    from tests.test_model_gpu import G, _cfg

    m, p, audio, g, plain = _case_a(dev)
    S0 = p.shape[1]
    new = plain[0, S0:].tolist()
    ref = AudioFlamingo3ForConditionalGeneration(_cfg())
    ref.load_state_dict(torch.load(os.path.join(G, "tiny64_state_bf16.pt")))
    ref = ref.float().eval()
    tok = R.tiny_tokenizer({new[3]: "Hel", new[4]: "lo", new[5]: " world"})
    feats = g["feats"][:1].to(torch.bfloat16).float()
    eos = [_unused(plain), new[8]]
    for extra, n in ((dict(), 9), (dict(stop_strings=["lo w"], tokenizer=tok), 6)):
        with torch.no_grad():
            want = ref.generate(input_ids=p.cpu(), input_features=feats, input_features_mask=g["fmask"][:1], max_new_tokens=NEW, do_sample=False, eos_token_id=eos,
                                **extra)
        got = m.generate(p, max_new_tokens=NEW, eos_token_id=eos, **extra, **audio)
        assert tuple(want.shape) == (1, S0 + n) and got.cpu().tolist() == want.tolist()


def test_the_scalar_case_enqueues_what_it_did(dev, monkeypatch):
    """(f) one eos id and no stop string: the entry points of a run with no eos at all (which the stopping rule never touched), call for call, and no
    afk_decode_stop; an eos list: one launch per token, token 0 included"""
    from audio_flamingo_amd import _lib

    m, p, audio, _, plain = _case_a(dev)
    ids, att = _padded_batch(dev)
    names = []
    real = _lib.call

    def spy(name, *a):
        names.append(name)
        return real(name, *a)

    monkeypatch.setattr(_lib, "call", spy)
    free, free2 = _unused(plain, 2)
    for args, kw in (((p,), dict(audio)), ((ids,), dict(attention_mask=att)), ((p,), dict(audio, repetition_penalty=1.3)),
                     ((p,), dict(audio, do_sample=True, seed=3, top_k=20))):
        names.clear()
        m.generate(*args, max_new_tokens=4, use_graph=False, **kw)
        none = list(names)
        for eos in (free, [free], torch.tensor([free])):
            names.clear()
            m.generate(*args, max_new_tokens=4, use_graph=False, eos_token_id=eos, **kw)
            assert names == none and "afk_decode_stop" not in names
        names.clear()
        m.generate(*args, max_new_tokens=4, use_graph=False, eos_token_id=[free, free2], **kw)
        assert names.count("afk_decode_stop") == 4 and [n for n in names if n != "afk_decode_stop"] == none


def test_the_step_with_the_stop_launch_replays_from_one_graph(dev, monkeypatch):
    """(g)"""
    from audio_flamingo_amd import _lib

    m, p, audio, _, plain = _case_a(dev)
    S0 = p.shape[1]
    new = plain[0, S0:].tolist()
    tok = R.tiny_tokenizer({new[9]: "en", new[10]: "d."})
    captured, names = [], []
    real_graph, real_call = torch.cuda.graph, _lib.call

    class Counting(real_graph):
        def __init__(self, *a, **k):
            captured.append(1)
            super().__init__(*a, **k)

    def spy(name, *a):
        names.append(name)
        return real_call(name, *a)

    monkeypatch.setattr(torch.cuda, "graph", Counting)
    monkeypatch.setattr(_lib, "call", spy)
    kw = dict(eos_token_id=_unused(plain, 2), stop_strings=["end"], tokenizer=tok, max_new_tokens=NEW, **audio)
    out = m.generate(p, use_graph=True, **kw)
    assert len(captured) == 1 and names.count("afk_decode_stop") == 3   # token 0, the eager step 1, the captured step: every later one is a replay
    assert out.shape == (1, S0 + 11) and torch.equal(out, plain[:, : S0 + 11])
    ids, att = _padded_batch(dev)
    captured.clear()
    a = m.generate(ids, attention_mask=att, use_graph=True, **dict(kw, eos_token_id=[1022, 1021]))
    assert len(captured) == 1 and torch.equal(a, m.generate(ids, attention_mask=att, use_graph=False, **dict(kw, eos_token_id=[1022, 1021])))

"""GPU: afk_decode_process_ex (csrc/decode_process.hip) against the numpy restatement of its contract (tests/_logits_process_ex_ref.py, pinned to the reference's
own classes by tests/test_decode_process_ex_cpu.py), and generate() with sequence_bias / bad_words_ids / min_length / forced_eos_token_id /
exponential_decay_length_penalty against the hook route, which runs the reference's own chain as logits_processor= between eager steps.

Every comparison is exact.  Kernel rows are compared with CPU rows by their bits, except that an entry which is NaN on one side has to be NaN on the other: IEEE
754 leaves the sign and the payload of the NaN an invalid operation (-inf + +inf) produces to the implementation, and the host and the device choose differently.
The two generate() routes both run on the device, so there the scores are compared by bits alone."""
import os
from types import SimpleNamespace

import pytest
import torch

from tests import _logits_process_ex_ref as R

pytestmark = pytest.mark.gpu


def _same_bits(got, want):
    nan = want.isnan()
    same = torch.equal(got.isnan(), nan) and torch.equal(R.bits(got)[~nan], R.bits(want)[~nan])
    if not same:   # the first entries that differ, for the failure message
        bad = torch.nonzero((got.isnan() != nan) | ((R.bits(got) != R.bits(want)) & ~nan))[:8].tolist()
        print("differs at (row, id, got, want):", [(b, i, float(got[b, i]), float(want[b, i])) for b, i in bad])
    return same


def _device_process(dev, logits, ids, S0, t, kw, *, max_new=R.MAX_NEW, pad_logits=0, use_step_base=False):
    """the device's rows for token t: the state is built from the prompt ids[:, :S0]; the t selected tokens ids[:, S0:] reach the history the way they do in
    generate() - one launch per step appends the previous one from the next-token buffer (the steps before t run on a scratch row)"""
    from audio_flamingo_amd import decode_process as P

    Bn, V = logits.shape
    ps = P.build_state(R.spec_of(kw), ids[:, :S0].to(dev), max_new, V)
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
def test_grid_equals_the_restatement_bit_for_bit(dev, V):
    """all ten processors, B = 3 rows at a row stride > V, t from the host and t through step_base on the device"""
    for (V_, S0, t) in R.grid():
        if V_ != V:
            continue
        logits, ids, kw = R.case(V, S0, t)
        want = R.restated(logits, ids, t, **kw)
        for use_step_base in (False, True):
            got, _ = _device_process(dev, logits, ids, S0, t, kw, pad_logits=5, use_step_base=use_step_base)
            assert _same_bits(got, want), (V, S0, t, use_step_base, kw)


@pytest.mark.parametrize("name", R.EX_KEYS)
def test_each_new_processor_alone(dev, name):
    for (V, S0, t) in R.grid():
        if V in (33, 1000):
            logits, ids, kw = R.case(V, S0, t)
            kw = R.alone(kw, name)
            got, _ = _device_process(dev, logits, ids, S0, t, kw, use_step_base=bool(t & 1))
            assert _same_bits(got, R.restated(logits, ids, t, **kw)), (name, V, S0, t)


def test_boundaries_and_a_bad_word_list_the_eos_filter_empties(dev):
    V, S0 = 256, 5
    logits, ids3, kw = R.case(V, S0, 3)
    eos = kw["eos"]
    for t in (R.MAX_NEW - 2, R.MAX_NEW - 1):
        ids = torch.cat([ids3, ids3[:, : t - 3]], 1)
        n = S0 + t
        cases = [dict(R.OFF, forced_eos=kw["forced_eos"], suppress=kw["suppress"]), dict(R.OFF, min_length=n + 1, eos=eos), dict(R.OFF, min_length=n, eos=eos),
                 dict(R.OFF, decay=(t, 1.5), eos=eos), dict(R.OFF, decay=(t - 1, 1.5), eos=eos), dict(R.OFF, decay=(t - 1, 0.5), eos=(eos[0], eos[0])),
                 dict(R.OFF, bad_words_ids=[[eos[0]]], eos=eos)]
        for c in cases:
            got, _ = _device_process(dev, logits, ids, S0, t, c)
            assert _same_bits(got, R.restated(logits, ids, t, **c)), (t, c)
    got, _ = _device_process(dev, logits, ids3, S0, 3, dict(R.OFF, bad_words_ids=[[eos[0]]], eos=eos))
    assert int((R.bits(got) == -2 ** 31).sum()) == 0 and int((R.bits(logits) == -2 ** 31).sum()) > 0     # the empty table still adds its 0.0f: no -0.0 is left


def test_af3_vocabulary_thousands_of_bad_words(dev):
    """V = 152 064, B = 2, ld_logits > V: 3 500 bad words in more groups than the block has threads (the group walk takes several passes), 400 of them in ONE
    group, and a sequence_bias of 300 entries"""
    V, S0, t = 152064, 60, 3
    gen = torch.Generator().manual_seed(21)
    ids = torch.randint(0, V, (2, S0 + t), generator=gen)
    ids[1, -2:] = ids[0, -2:]
    T = ids[0].tolist()
    last = torch.randperm(V, generator=gen)[:3400].tolist()
    bad = [[i] for i in last[:600]] + [[T[-1], i] for i in last[600:1800]] + [[T[-2], T[-1], i] for i in last[1800:2600]] + [[(T[-1] + 1) % V, i] for i in last[2600:3100]]
    bad += [[(j * 7919) % V, T[-1], last[3100]] for j in range(400)] + [[17, last[3101]]] * 3
    sb = {(i,): 0.5 + 0.25 * (k % 9) for k, i in enumerate(last[3110:3300])}
    sb.update({(T[-1], i): -1.5 for i in last[3300:3400]})
    sb.update({(T[-1], last[3110]): 1.0e8, (T[-2], T[-1], last[3110]): -1.0e8})
    logits = (torch.randn((2, V), generator=gen) * 4.0).to(torch.bfloat16).float()
    logits[:, last[5]], logits[:, last[700]], logits[:, 0] = float("inf"), -0.0, -0.0
    kw = dict(R.OFF, penalty=1.05, ngram=2, bad_words_ids=bad, sequence_bias=sb, eos=(151645, 151643), min_length=S0 + 8, forced_eos=(151645,), decay=(1, 1.2),
              suppress=(V - 1, 17))
    for tt, step_base in ((t, True), (R.MAX_NEW - 1, False)):
        ids_t = torch.cat([ids, ids[:, : tt - t]], 1)
        want = R.restated(logits, ids_t, tt, **kw)
        got, ps = _device_process(dev, logits, ids_t, S0, tt, kw, pad_logits=37, use_step_base=step_base)
        assert _same_bits(got, want), tt
        assert ps["ex"]["bad"]["group_id"].numel() > 2048 and int(ps["ex"]["bad"]["group_off"].diff().max()) == 400
    assert int((want == 0.0).sum()) == 2 and bool(want[:, 151645].eq(0.0).all())          # the forced step: 0.0 on the forced id, scaled by the decay: still 0.0


def test_greedy_selection_equals_the_greedy_launch_and_a_rerun_changes_nothing(dev):
    """select at B = 1: the token, tokens_out, state[1 .. 3] and the embedding row are what afk_decode_select_greedy leaves for the processed row; the same step
    run a second time on the same inputs leaves the same row, history and seen set"""
    from audio_flamingo_amd import _lib
    from audio_flamingo_amd import decode_process as P
    from audio_flamingo_amd import ops

    V, H, S0, t = 1000, 64, 40, 3
    logits, ids, kw = R.case(V, S0, t)
    logits, ids = logits[:1].clone(), ids[:1]
    logits[logits == float("inf")] = 5.0
    # the state is built on the first S0 + t - 1 ids as its prompt, so the case's token t is its token 1: the decay start and max_new_tokens move with it
    kw = dict(kw, sequence_bias={k: v for k, v in kw["sequence_bias"].items() if v != float("inf")}, decay=(kw["decay"][0] - (t - 1), kw["decay"][1]))
    max_new = R.MAX_NEW - (t - 1)
    logits[0, kw["suppress"][1]] = 90.0                                    # the raw maximum is suppressed
    want_row = R.restated(logits, ids, 1, max_new=max_new, **kw)
    ranked = torch.where(want_row[0].isnan(), torch.full_like(want_row[0], float("-inf")), want_row[0])   # a NaN (a banned eos id under the decay) never wins
    assert bool(want_row.isnan().any())
    want = int(torch.nonzero(ranked == ranked.max())[0])
    emb = torch.randn(V, H, generator=torch.Generator().manual_seed(8)).to(torch.bfloat16).to(dev)
    state0 = torch.tensor([0, S0 + t, S0 + t - 1, S0 + t - 1], dtype=torch.int32)
    tok_off = 1 - S0
    ps = P.build_state(R.spec_of(kw), ids[:, : S0 + t - 1].to(dev), max_new, V)
    snap = None
    for _ in range(2):
        st, toks, x_out = state0.to(dev), torch.zeros(16, dtype=torch.int64, device=dev), torch.zeros(H, dtype=torch.bfloat16, device=dev)
        nxt = ids[:, -1].to(dev).clone()
        row = logits.to(dev)
        P.apply(ps, row, next_token=nxt, step_base=st[2:3], step_off=2 - S0 - t, select=True, tokens_out=toks, tok_off=tok_off, state=st, emb=emb, x_out=x_out)
        now = (R.bits(row.cpu()), ps["hist"].cpu(), ps["seen"].cpu(), int(nxt[0]), st.cpu(), toks.cpu(), x_out.cpu())
        assert snap is None or all(torch.equal(a, b) if torch.is_tensor(a) else a == b for a, b in zip(snap, now))
        snap = now
    assert _same_bits(snap[0].view(torch.float32), want_row) and snap[3] == want and want != kw["suppress"][1]
    pv, pi = ranked.view(V // 8, 8).max(-1)
    pv, pi = pv.to(dev), (pi + 8 * torch.arange(V // 8)).to(torch.int32).to(dev)
    st2, toks2, x2, nxt2 = state0.to(dev), torch.zeros(16, dtype=torch.int64, device=dev), torch.zeros(H, dtype=torch.bfloat16, device=dev), torch.zeros(1, dtype=torch.int64, device=dev)
    _lib.call("afk_decode_select_greedy", pv.data_ptr(), pi.data_ptr(), V // 8, nxt2.data_ptr(), toks2.data_ptr(), tok_off, st2.data_ptr(), emb.data_ptr(),
              emb.stride(0), H, x2.data_ptr(), ops._stream())
    assert int(nxt2[0]) == snap[3] and torch.equal(toks2.cpu(), snap[5]) and torch.equal(st2.cpu(), snap[4]) and torch.equal(x2.cpu(), snap[6])
    assert snap[4].tolist() == [0, S0 + t + 1, S0 + t, S0 + t] and torch.equal(snap[6], emb[want].cpu()) and int(snap[5][t]) == want


def test_entry_point_refuses_bad_arguments(dev):
    from audio_flamingo_amd import _lib, ops
    from audio_flamingo_amd import decode_process as P
    from audio_flamingo_amd._lib import AfkError

    V = 40
    x, hist, seen = torch.zeros((2, V), device=dev), torch.zeros((2, 8), device=dev, dtype=torch.int32), torch.zeros((2, 2), device=dev, dtype=torch.int32)
    nxt = torch.zeros(2, device=dev, dtype=torch.int64)
    ok = dict(S0=4, next_token=nxt, max_new_tokens=4)
    with pytest.raises(ValueError, match="vocabulary size is 40"):           # ids outside [0, V): refused where the table is packed, as the reference raises
        P.build_state(P.resolve(bad_words_ids=[[3, 40]]), torch.zeros((1, 4), dtype=torch.long, device=dev), 4, V)
    with pytest.raises(ValueError, match="vocabulary size is 40"):
        P.pack_sequences((((41,), 1.0),), V)
    decay = torch.zeros(3, device=dev)
    with pytest.raises(AfkError, match="decay table of 3 entries"):
        ops.decode_process_ex(x, hist, seen, decay=decay, eos=torch.tensor([1], device=dev, dtype=torch.int32), **ok)
    with pytest.raises(AfkError):
        ops.decode_process_ex(x, hist, seen, **dict(ok, max_new_tokens=0))
    with pytest.raises(AfkError):
        ops.decode_process_ex(x, hist, seen, min_length=-1, **ok)
    tb = P._table_to(P.pack_sequences((((1, 2), 1.0), ((3,), 2.0)), V), dev)
    for k in ("group_l1", "group_off", "seq_off"):
        with pytest.raises(AfkError):
            ops.decode_process_ex(x, hist, seen, bias=dict(tb, **{k: tb[k][:-1].contiguous()}), **ok)
    with pytest.raises(AfkError):
        ops.decode_process_ex(x, hist, seen, bad=dict(tb, ids=tb["ids"].cpu()), **ok)
    # null tables that come with counts: only the C entry can be handed those
    common = ops._decode_process_args(x, hist, seen, 4, 1.0, 0, None, None, None, 0, nxt, None, 0, False, None, 0, None, None, None)
    none8 = (None, None, None, 0, None, None, None, 0)
    for bias, bad, forced, dec in (((None, None, None, 0, None, None, None, 1), none8, (None, 0), (None, 0)),
                                   (none8, (None, tb["seq_off"].data_ptr(), tb["seq_bias"].data_ptr(), 1, tb["group_id"].data_ptr(), tb["group_l1"].data_ptr(),
                                            tb["group_off"].data_ptr(), 2), (None, 0), (None, 0)),
                                   (none8, none8, (None, 2), (None, 0)), (none8, none8, (None, 0), (None, 4))):
        with pytest.raises(AfkError, match="null pointer"):
            _lib.call("afk_decode_process_ex", *common, *bias, *bad, 0, *forced, *dec, 0, 4, ops._stream())
    assert not x.any()
    ops.decode_process_ex(x, hist, seen, bias=tb, **ok)                      # and the accepted call: ids 3 (its own bias) and nothing else, the history is all 0
    assert x[:, 3].eq(2.0).all() and int((x != 0).sum()) == 2


# ---------------------------------------------------------------------------------------------- generate()
N = 12
SPARE = 1000   # a second eos id: with two the stopping rule is a launch of the step, and the result has the reference's length on every route


def _case_a(dev):
    from tests.test_sampler_gpu import _case_a as case_a

    return case_a(dev)


def _batch(dev):
    g = torch.Generator().manual_seed(3)
    ids, att = torch.zeros((2, 40), dtype=torch.long), torch.zeros((2, 40), dtype=torch.long)
    for i, n in enumerate((40, 23)):
        ids[i, 40 - n:] = torch.randint(0, 256, (n,), generator=g)
        att[i, 40 - n:] = 1
    return ids.to(dev), dict(attention_mask=att.to(dev))


def _gen_kw(c):
    """a case in the restatement's keywords -> generate()'s"""
    names = dict(penalty="repetition_penalty", ngram="no_repeat_ngram_size", suppress="suppress_tokens", begin_suppress="begin_suppress_tokens",
                 forced_eos="forced_eos_token_id", decay="exponential_decay_length_penalty", eos="eos_token_id")
    off = dict(R.OFF)
    return {names.get(k, k): (list(v) if isinstance(v, tuple) and k != "decay" else v) for k, v in c.items() if v != off[k]}


def _cases(plain):
    """the processors' settings cut from the ids an unprocessed greedy run picks (plain: its N new tokens of row 0), so that each one changes the run"""
    c = dict(bad_one=dict(R.OFF, bad_words_ids=[[plain[3]]]), bad_pair=dict(R.OFF, bad_words_ids=[[plain[6], plain[7]]]),
             bias=dict(R.OFF, sequence_bias={(plain[1], plain[0]): 60.0, (plain[5],): -60.0}), min_length=dict(R.OFF, eos=(plain[4], SPARE), min_length=None),
             forced=dict(R.OFF, forced_eos=(plain[0],)), decay=dict(R.OFF, eos=(plain[11], SPARE), decay=(1, 6.0)))
    # all ten.  Two choices keep the hook route comparable bit for bit; both concern that route, not the launch (whose rows the grid tests pin to the CPU classes):
    # the penalty is a power of two, because torch divides by a scalar on the device by multiplying with its reciprocal, one ulp off the IEEE quotient that the
    # CPU classes and the kernel compute for 1.3; and no eos id is banned while the length penalty is active (it starts where min_length ends, and the forced ids
    # are the eos ids), because -inf + inf * c is NaN in the reference too, torch.argmax picks a NaN and the on-device selection never does.
    c["all_ten"] = dict(penalty=2.0, ngram=2, suppress=(plain[2],), begin_suppress=(plain[0],), eos=(plain[9], SPARE), min_new_tokens=3, min_length=None,
                        sequence_bias={(plain[1], plain[8]): 2.5, (plain[5],): -1.0}, bad_words_ids=[[plain[3]], [plain[6], plain[7]], [plain[9]]],
                        forced_eos=(plain[9], SPARE), decay=(8, 1.5))
    return c


def _three_routes(m, p, extra, c, S0, how, dev):
    """the device route eager and replayed, and the hook route with the reference's own chain -> (sequences, stacked scores) of each"""
    c = dict(c, min_length=S0 + 8) if c["min_length"] is None else c
    eos = dict(eos_token_id=list(c["eos"])) if c["eos"] else {}
    out_kw = dict(return_dict_in_generate=True, output_scores=True)
    kw = {k: v for k, v in _gen_kw(c).items() if k != "eos_token_id"}
    runs = [m.generate(p, use_graph=False, **kw, **eos, **extra, **how, **out_kw), m.generate(p, use_graph=True, **kw, **eos, **extra, **how, **out_kw),
            m.generate(p, logits_processor=R.reference_chain(None, None, S0, max_new=N, device=dev, **c), **eos, **extra, **how, **out_kw)]
    return [(r.sequences, torch.stack(r.scores)) for r in runs]


CASES = ("bad_one", "bad_pair", "bias", "min_length", "forced", "decay", "all_ten")


@pytest.mark.parametrize("mode", ["greedy", "sampled"])
@pytest.mark.parametrize("which", CASES)
def test_generate_one_sequence_equals_the_hook_route(dev, which, mode):
    from tests.test_sampler_gpu import SAMPLED

    m, p, audio = _case_a(dev)
    S0 = p.shape[1]
    plain = m.generate(p, max_new_tokens=N, **audio)[0, S0:].tolist()
    assert len(set(plain)) == N
    c = _cases(plain)[which]
    how = dict(SAMPLED) if mode == "sampled" else dict(max_new_tokens=N)
    assert how["max_new_tokens"] == N
    runs = _three_routes(m, p, audio, c, S0, how, dev)
    new = runs[0][0][0, S0:].tolist()
    print(which, mode, plain, new)
    for seq, scores in runs[1:]:
        assert torch.equal(seq, runs[0][0]) and torch.equal(R.bits(scores), R.bits(runs[0][1]))
    assert runs[0][1].shape == (len(new), 1, 1024)
    if which == "forced":
        assert len(new) == N and new[-1] == plain[0] and plain[-1] != plain[0]
    if which == "bad_one":
        assert plain[3] not in new
    if mode == "sampled":
        return
    first_change = next((i for i, (a, b) in enumerate(zip(plain, new)) if a != b), None)
    if which == "bad_one":
        assert first_change == 3
    if which == "bad_pair":
        assert first_change == 7 and new[6] == plain[6]
    if which == "bias":
        assert first_change == 2 and new[2] == plain[0]
    if which == "min_length":   # the plain run with this eos ends at token 4; min_length keeps the eos out until the length is S0 + 8
        short = m.generate(p, max_new_tokens=N, eos_token_id=list(c["eos"]), **audio)
        assert short.shape[1] == S0 + 5 and len(new) >= 8 and not set(c["eos"]) & set(new[:8]) and new[:4] == plain[:4]
    if which == "decay":        # the plain run reaches this eos only at its last token; the penalty brings it forward
        assert SPARE not in plain and len(new) < N and new[-1] in c["eos"] and not set(c["eos"]) & set(new[:-1])
    if which == "all_ten":
        assert new != plain and new[0] != plain[0] and plain[3] not in new and plain[2] not in new


@pytest.mark.parametrize("mode", ["greedy", "sampled"])
@pytest.mark.parametrize("which", CASES)
def test_generate_left_padded_batch_equals_the_hook_route(dev, which, mode):
    from tests.test_sampler_gpu import SAMPLED

    m, _, _ = _case_a(dev)
    ids, att = _batch(dev)
    plain = m.generate(ids, max_new_tokens=N, **att)[:, 40:]
    c = _cases(plain[0].tolist())[which]
    how = dict(SAMPLED) if mode == "sampled" else dict(max_new_tokens=N)
    runs = _three_routes(m, ids, att, c, 40, how, dev)
    new = runs[0][0][:, 40:]
    print(which, mode, plain.tolist(), new.tolist())
    for seq, scores in runs[1:]:
        assert torch.equal(seq, runs[0][0]) and torch.equal(R.bits(scores), R.bits(runs[0][1]))
    assert runs[0][1].shape == (new.shape[1], 2, 1024)
    if which == "forced":
        assert new.shape[1] == N and bool((new[:, -1] == c["forced_eos"][0]).all())
    if which == "bad_one":
        assert not bool((new == c["bad_words_ids"][0][0]).any())
    if which == "min_length":
        assert new.shape[1] >= 8 and not bool(torch.isin(new[:, :8], torch.tensor(c["eos"], device=dev)).any())
    if which == "decay" and mode == "greedy":
        assert new.shape[1] < N and bool(torch.isin(new, torch.tensor(c["eos"], device=dev)).any(1).all())
    if mode == "greedy" and which != "min_length":
        assert not torch.equal(new, plain[:, : new.shape[1]])


def test_launch_counts_one_graph_and_the_generation_config(dev, monkeypatch):
    from audio_flamingo_amd import _lib

    m, p, audio = _case_a(dev)
    S0 = p.shape[1]
    plain = m.generate(p, max_new_tokens=N, **audio)[0, S0:].tolist()
    names = []
    real = _lib.call

    def spy(name, *a):
        names.append(name)
        return real(name, *a)

    monkeypatch.setattr(_lib, "call", spy)
    by_kw = m.generate(p, max_new_tokens=N, use_graph=False, bad_words_ids=[[plain[3]]], **audio)
    assert names.count("afk_decode_process_ex") == N and "afk_decode_process" not in names and "afk_decode_select_greedy" not in names
    names.clear()
    m.generate(p, max_new_tokens=4, use_graph=False, repetition_penalty=1.3, min_length=0, **audio)     # none of the new five: the launch it was
    assert names.count("afk_decode_process") == 4 and "afk_decode_process_ex" not in names
    monkeypatch.setattr(_lib, "call", real)
    captured = []
    real_graph = torch.cuda.graph

    class Counting(real_graph):
        def __init__(self, *a, **k):
            captured.append(1)
            super().__init__(*a, **k)

    monkeypatch.setattr(torch.cuda, "graph", Counting)
    out = m.generate(p, max_new_tokens=N, forced_eos_token_id=plain[0], **audio)
    assert len(captured) == 1 and int(out[0, -1]) == plain[0] and out.shape[1] == S0 + N
    # a generation config that carries bad_words_ids is no longer ignored: the ids of the keyword
    from transformers import GenerationConfig

    for gc in (SimpleNamespace(bad_words_ids=[[plain[3]]]), GenerationConfig(bad_words_ids=[[plain[3]]], max_new_tokens=N)):
        by_gc = m.generate(p, max_new_tokens=N, generation_config=gc, **audio)
        assert torch.equal(by_gc, by_kw) and plain[3] not in by_gc[0, S0:].tolist()


def test_out_of_scope_combinations_raise(dev):
    from audio_flamingo_amd._lib import AfkError

    m, p, audio = _case_a(dev)
    for how in (dict(num_beams=2), dict(use_cache=False)):
        for five in (dict(sequence_bias={(3,): 1.0}), dict(bad_words_ids=[[3, 4]]), dict(min_length=900, eos_token_id=5), dict(forced_eos_token_id=5),
                     dict(exponential_decay_length_penalty=(1, 1.1), eos_token_id=5)):
            with pytest.raises(AfkError, match="KV cache only"):
                m.generate(p, max_new_tokens=4, **how, **five, **audio)
    with pytest.raises(ValueError, match="non-empty list"):
        m.generate(p, max_new_tokens=4, bad_words_ids=[], **audio)
    with pytest.raises(ValueError, match="vocabulary size is 1024"):
        m.generate(p, max_new_tokens=4, bad_words_ids=[[1024]], **audio)

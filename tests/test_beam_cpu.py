"""CPU: the numpy restatement of afk_beam_step's contract (tests/_beam_ref.py) against GenerationMixin's own beam-search helpers, chained over eight steps of
random logits exactly as GenerationMixin._beam_search chains them, and generate()'s num_return_sequences validation against GenerationConfig.validate."""
import numpy as np
import pytest
import torch

from tests import _beam_ref as R

STEPS = 8
S0 = 3   # a dummy prompt in front of the reference's [batch, beams, max_length] buffers


def _bare():
    from transformers.generation.utils import GenerationMixin

    class Bare(GenerationMixin):
        pass

    return Bare()


def _reference_chain(logits, B, nb, V, eos, length_penalty, early_stopping):
    """the body of GenerationMixin._beam_search's loop (transformers/generation/utils.py) on given logits [STEPS][B * nb, V], helper for helper -> one record
    per step that ran"""
    m = _bare()
    max_length, cur_len, keep = S0 + STEPS, S0, (len(eos) + 1) * nb
    running_sequences = torch.full((B, nb, max_length), -1, dtype=torch.int64)
    running_sequences[:, :, :S0] = 7
    sequences = running_sequences.clone()
    running_beam_scores = torch.zeros((B, nb))
    running_beam_scores[:, 1:] = -1e9
    beam_scores = torch.full((B, nb), -1e9)
    is_sent_finished = torch.zeros((B, nb), dtype=torch.bool)
    unsatisfied = torch.ones((B, 1), dtype=torch.bool)
    running_beam_indices = torch.full((B, nb, STEPS), -1, dtype=torch.int32)
    beam_indices = running_beam_indices.clone()
    top_mask = torch.cat([torch.ones(nb), torch.zeros(keep - nb)]).bool()
    eos_t = torch.tensor(list(eos), dtype=torch.int64)
    out = []
    for t in range(STEPS):
        log_probs = torch.log_softmax(torch.from_numpy(logits[t]), -1).view(B, nb, V) + running_beam_scores[:, :, None]
        topk_lp, topk_seq, topk_bi = m._get_top_k_continuations(
            accumulated_log_probs=log_probs.reshape(B, nb * V), running_sequences=running_sequences, running_beam_indices=running_beam_indices, cur_len=cur_len,
            decoder_prompt_len=S0, do_sample=False, beams_to_keep=keep, num_beams=nb, vocab_size=V, batch_size=B)
        hits = torch.isin(topk_seq[:, :, cur_len], eos_t) | (cur_len + 1 >= max_length)
        running_sequences, running_beam_scores, running_beam_indices = m._get_running_beams_for_next_iteration(
            topk_log_probs=topk_lp, topk_running_sequences=topk_seq, topk_running_beam_indices=topk_bi, next_token_hits_stopping_criteria=hits, num_beams=nb)
        sequences, beam_scores, beam_indices, is_sent_finished = m._update_finished_beams(
            sequences=sequences, topk_running_sequences=topk_seq, beam_scores=beam_scores, topk_log_probs=topk_lp, beam_indices=beam_indices,
            topk_running_beam_indices=topk_bi, is_early_stop_heuristic_unsatisfied=unsatisfied, is_sent_finished=is_sent_finished,
            next_token_hits_stopping_criteria=hits, top_num_beam_mask=top_mask, num_beams=nb, cur_len=cur_len, decoder_prompt_len=S0,
            length_penalty=length_penalty, early_stopping=early_stopping)
        cur_len += 1
        unsatisfied = m._check_early_stop_heuristic(
            is_early_stop_heuristic_unsatisfied=unsatisfied, running_beam_scores=running_beam_scores, beam_scores=beam_scores, is_sent_finished=is_sent_finished,
            cur_len=cur_len, max_length=max_length, decoder_prompt_len=S0, early_stopping=early_stopping, length_penalty=length_penalty)
        is_open = bool(m._beam_search_has_unfinished_sequences(unsatisfied, is_sent_finished, hits, early_stopping))
        out.append(dict(tok=running_sequences[:, :, cur_len - 1].numpy().copy(), src=running_beam_indices[:, :, t].numpy().copy(),
                        run_score=running_beam_scores.numpy().copy(), fin_seq=sequences[:, :, S0:].numpy().copy(), fin_score=beam_scores.numpy().copy(),
                        fin_done=is_sent_finished.numpy().copy(), fin_len=(beam_indices >= 0).sum(-1).numpy().copy(), can_improve=unsatisfied[:, 0].numpy().copy(),
                        open=is_open))
        if not is_open:
            break
    return out


@pytest.mark.parametrize("early_stopping", [False, True, "never"])
@pytest.mark.parametrize("length_penalty", [0.0, 1.0, 2.0])
@pytest.mark.parametrize("n_eos", [0, 1, 2])
def test_restatement_equals_the_reference_helpers_over_eight_steps(n_eos, length_penalty, early_stopping):
    V = 23
    early_stops = 0
    for B, nb in ((1, 2), (3, 5)):
        gen = np.random.default_rng(1000 * n_eos + 100 * int(length_penalty) + 10 * B + nb)
        eos = tuple(int(e) for e in gen.choice(V, size=n_eos, replace=False))
        logits = [(3.0 * gen.standard_normal((B * nb, V))).astype(np.float32) for _ in range(STEPS)]
        for x in logits:
            x[:, list(eos)] += 3.0   # likely enough that hypotheses finish in front of the length limit
        want = _reference_chain(logits, B, nb, V, eos, length_penalty, early_stopping)
        st = R.new_state(B, nb, STEPS)
        div, hdiv = R.tables(STEPS, length_penalty, early_stopping)
        for t, w in enumerate(want):
            R.step(st, logits[t], t, nb=nb, max_new=STEPS, eos=eos, early_stopping=early_stopping, div=div, hdiv=hdiv)
            where = (n_eos, length_penalty, early_stopping, B, nb, t)
            assert st["status"].tolist() == [t, int(w["open"])], where
            live = w["run_score"] > -1e8   # an ended candidate that had to fill the running set carries -1e9, which absorbs its score: such entries tie, and
            assert np.array_equal(st["run_score"] > -1e8, live), where   # torch.topk leaves their order open (at the length limit every entry is one)
            assert np.array_equal(st["next_token"].reshape(B, nb)[live], w["tok"][live]), where
            if not live.all():
                assert t + 1 == STEPS and not w["open"], where
            elif w["open"]:   # a closing step hands the identity on: the reference's loop is over in front of its cache move
                assert np.array_equal(st["src"].reshape(B, nb), w["src"]), where
            else:
                assert np.array_equal(st["src"], np.arange(B * nb)), where
            assert np.allclose(st["run_score"][live], w["run_score"][live], rtol=0, atol=1e-5), where
            done = w["fin_done"]
            assert np.array_equal(st["fin_done"], done), where
            assert np.allclose(st["fin_score"][done], w["fin_score"][done], rtol=1e-6, atol=1e-5), where
            assert np.array_equal(st["fin_len"][done], w["fin_len"][done]), where
            for b, k in zip(*np.nonzero(done)):
                n = st["fin_len"][b, k]
                assert np.array_equal(st["fin_seq"][b, k, :n], w["fin_seq"][b, k, :n]), where
            if t + 1 < STEPS:
                assert np.array_equal(st["can_improve"], w["can_improve"]), where
        assert st["status"][1] == 0 and len(want) == st["status"][0] + 1
        early_stops += len(want) < STEPS
        # a launch behind the closing step, and a t outside [0, max_new), move nothing
        before = {k: v.copy() for k, v in st.items()}
        for t in (len(want), -1, STEPS):
            R.step(st, logits[0], t, nb=nb, max_new=STEPS, eos=eos, early_stopping=early_stopping, div=div, hdiv=hdiv)
        assert all(np.array_equal(before[k], st[k]) for k in st)
    if n_eos and early_stopping is True:
        assert early_stops, "early_stopping=True with eos ids over 23 tokens must close a search in front of the length limit"


def test_the_loop_and_the_tie_rule():
    """search() drives step() to the closing step; a row of equal logits takes the lowest flat indices; -1e9 absorbs the dead beams of token 0"""
    st = R.search(lambda t, tok, src: np.zeros((2, 11), dtype=np.float32), 1, 2, 3)
    assert st["status"].tolist() == [2, 0] and st["fin_done"].all() and st["fin_len"].tolist() == [[3, 3]]
    assert st["fin_seq"].tolist() == [[[0, 0, 0], [0, 0, 1]]]   # token 0: ids 0, 1 of beam 0; afterwards beam 0's ids 0, 1 again (it leads by nothing: lower index)
    trace = {}
    one = R.new_state(1, 3, 4)
    div, hdiv = R.tables(4, 1.0, False)
    R.step(one, np.zeros((3, 7), dtype=np.float32), 0, nb=3, max_new=4, eos=(), early_stopping=False, div=div, hdiv=hdiv, trace=trace)
    assert one["next_token"].tolist() == [0, 1, 2] and one["src"].tolist() == [0, 0, 0]
    assert np.allclose(one["run_score"], -np.log(7.0), atol=1e-6) and len(trace["top"][0]) == 4


def test_divisor_tables_are_the_python_powers():
    for lp in (0.0, 1.0, 2.0, 0.7, -1.0):
        div, hdiv = R.tables(9, lp, False)
        assert div.dtype == np.float32 and [float(x) for x in div] == [float(np.float32((t + 1) ** lp)) for t in range(9)] and np.array_equal(div, hdiv)
        _, never = R.tables(9, lp, "never")
        assert np.array_equal(never, np.full(9, np.float32(9 ** lp)) if lp > 0 else div)


@pytest.mark.parametrize("do_sample", [False, True])
@pytest.mark.parametrize("num_beams", [1, 2, 4])
def test_num_return_sequences_validation_is_the_reference_one(num_beams, do_sample):
    from transformers import GenerationConfig

    from audio_flamingo_amd.generation_output import resolve_num_return_sequences as resolve

    for n in (1, 2, 4, 5):
        try:
            GenerationConfig(num_beams=num_beams, do_sample=do_sample, num_return_sequences=n).validate(strict=True)
            want = None
        except ValueError as e:
            want = str(e)
        if want is None:
            assert resolve(n, num_beams=num_beams, do_sample=do_sample) == n
        else:
            with pytest.raises(ValueError) as got:
                resolve(n, num_beams=num_beams, do_sample=do_sample)
            assert str(got.value) in want, (str(got.value), want)
    # keyword first, else the generation config, else 1
    gc = GenerationConfig(num_beams=4, num_return_sequences=3)
    assert resolve(None, generation_config=gc, num_beams=4) == 3 and resolve(2, generation_config=gc, num_beams=4) == 2 and resolve(None, num_beams=4) == 1
    assert resolve(None, generation_config=GenerationConfig(), num_beams=1) == 1
    for bad in (0, -1, 1.5, True):
        with pytest.raises(ValueError, match="num_return_sequences"):
            resolve(bad, num_beams=4)

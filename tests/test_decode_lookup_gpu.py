"""GPU: prompt-lookup decoding.  The two launches (afk_lookup_draft / afk_lookup_accept) against their integer restatement (tests/_lookup_ref.py, itself pinned to
the reference's classes in test_decode_lookup_cpu.py) - exact integer comparison, no tolerance anywhere; the verify forward teacher-forced on the trained tiny
model in both of its forms; generate(prompt_lookup_num_tokens=...) against the plain greedy call of the same prompt."""
import numpy as np
import pytest
import torch

from tests import _lookup_ref as R
from tests.test_sampler_gpu import _case_a

pytestmark = pytest.mark.gpu

H_EMB, VOCAB_EMB = 64, 97


def _i32(a, dev):
    return torch.tensor(np.asarray(a, dtype=np.int32), dtype=torch.int32, device=dev)


_EMB = {}


def _emb(dev):
    if dev not in _EMB:
        _EMB[dev] = torch.randn((VOCAB_EMB, H_EMB), generator=torch.Generator().manual_seed(1)).to(dev, torch.bfloat16)
    return _EMB[dev]


def _check_draft(dev, hist, k, ngram, eos=(), *, emitted=1, max_new=10 ** 6, done=0, state=(2, 9, 8, 6), gather=True):
    """one afk_lookup_draft launch on `hist` against R.draft: every output, every status word, and nothing else moved -> n_cand"""
    from audio_flamingo_amd import _lib, ops

    n, M = len(hist), k + 1
    ids = np.zeros(n + 5, dtype=np.int32)
    ids[:n] = hist
    st = R.new_status(n, emitted, done)
    st[R.N_CAND], st[R.STEPS], st[R.ACCEPTED] = 77, 5, 3   # n_cand is overwritten, the others are not the draft's to touch
    state = np.asarray(state, dtype=np.int32)
    d_ids, d_st, d_state = _i32(ids, dev), _i32(st, dev), _i32(state, dev)
    cand, pos, kr = (torch.full(s, -1, device=dev, dtype=torch.int32) for s in ((k,), (M,), (M, 2)))
    rows = torch.full((M,), -1, device=dev, dtype=torch.int64)
    eos_t = _i32(eos, dev) if eos else None
    emb = _emb(dev)
    x = torch.zeros((M, H_EMB), device=dev, dtype=torch.bfloat16) if gather else None
    _lib.call("afk_lookup_draft", d_ids.data_ptr(), d_ids.numel(), d_st.data_ptr(), d_state.data_ptr(), k, ngram, max_new, ops._p(eos_t), len(eos), cand.data_ptr(),
              rows.data_ptr(), pos.data_ptr(), kr.data_ptr(), emb.data_ptr(), emb.stride(0), VOCAB_EMB, H_EMB, ops._p(x), H_EMB, ops._stream())
    want = R.draft(ids, st, state, k, ngram, max_new, eos)
    what = (n, k, ngram, eos, emitted, max_new, done)
    assert d_st.cpu().numpy().tolist() == st.tolist(), what
    assert cand.cpu().numpy().tolist() == want["cand"].tolist(), what
    assert rows.cpu().numpy().tolist() == want["rows"].tolist() and pos.cpu().numpy().tolist() == want["pos"].tolist(), what
    assert kr.cpu().numpy().tolist() == want["krange"].tolist(), what
    assert d_ids.cpu().numpy().tolist() == ids.tolist() and d_state.cpu().numpy().tolist() == state.tolist(), what
    if gather:
        assert torch.equal(x, emb.index_select(0, rows.clamp(0, VOCAB_EMB - 1))), what
    return int(st[R.N_CAND])


def _planted(n, g, where):
    """a history of n distinct ids whose last g ids also stand at `where` (None, or no room in front of the tail: nowhere) -> (history, planted)"""
    hist = (1000 + 7 * np.arange(n)).tolist()
    planted = bool(g) and where is not None and 0 <= where and where + g <= n - g
    if planted:
        hist[where:where + g] = hist[n - g:]
    return hist, planted


@pytest.mark.parametrize("n", [1, 2, 3, 63, 64, 65, 257, 4099, 16001])
def test_draft_equals_the_restatement(dev, n):
    """every (k, ngram, eos count) on a random small-vocabulary history (matches everywhere: the leftmost wins, eos crops) and on histories of distinct ids with
    the trailing n-gram planted once - near the front, in the middle, right in front of the tail (a continuation shorter than k) - or nowhere (tail only)"""
    gen = np.random.default_rng(100 + n)
    some = none = 0
    for k in (1, 3, 7, 31):
        for ngram in (1, 2, 4):
            for n_eos in (0, 1, 2):
                vocab = int(gen.integers(3, 7))
                hist = gen.integers(0, vocab, size=n).tolist()
                eos = tuple(gen.choice(vocab, size=n_eos, replace=False).tolist())
                got = _check_draft(dev, hist, k, ngram, eos, gather=(k, ngram) in ((3, 2), (31, 1)))
                some, none = some + bool(got), none + (not got)
            g = min(ngram, n - 1)
            for where in (0, n // 2, n - 2 * g - 1, n - 2 * g, None):
                hist, planted = _planted(n, g, where)
                eos = (hist[where + g + 1],) if (planted and where + g + 1 < n and k > 1) else ()   # the second id of the continuation: one candidate is left
                got = _check_draft(dev, hist, k, ngram, eos, gather=False)
                assert bool(got) == planted, (n, k, ngram, where)
                some, none = some + bool(got), none + (not got)
    assert none > 0 and (some > 0 or n <= 2), (some, none)


def test_draft_named_cases(dev):
    c = lambda *a, **kw: _check_draft(dev, *a, **kw)
    assert c([1, 2, 3, 4], 3, 2) == 0                                   # a match only at the tail
    assert c([5, 6, 1, 9, 5, 6, 2, 8, 5, 6], 2, 2) == 2                 # two matches: the leftmost (R.candidates pins which)
    assert c([3, 4, 3], 5, 1) == 2                                      # a continuation shorter than k at the end of the history
    assert c([3, 9, 1, 3, 7, 2, 3], 3, 1, (9,)) == 0                    # an eos as the first candidate: none, no second match tried
    assert c([3, 7, 9, 3, 5, 2, 3], 3, 1, (9, 50)) == 1
    hist = [3, 7, 1, 3, 5, 2, 3]
    assert [c(hist, 3, 1, emitted=e, max_new=10) for e in (1, 7, 8, 9)] == [3, 2, 1, 0]   # the budget crop: max_new - 2 leaves one, max_new - 1 none
    assert c(hist, 3, 1, done=1) == 0
    assert c(hist, 31, 4, state=(0, 16001, 16000, 16000)) == 6


def _check_accept(dev, z, cand, n_cand, *, eos=(), emitted=1, max_new=64, n=10, done=0, twice=False):
    """one afk_lookup_accept call on the logits z [M, V] (numpy fp32) against R.accept: sel, ids, tokens, every status word and the state tensor"""
    from audio_flamingo_amd import _lib, ops
    from audio_flamingo_amd.decode_lookup import WS_WORDS

    M, V = z.shape
    ids = np.zeros(n + 40, dtype=np.int32)
    ids[:n] = np.arange(n) % 5
    tokens = np.zeros(max_new, dtype=np.int64)
    st = R.new_status(n, emitted, done)
    st[R.N_CAND], st[R.STEPS], st[R.ACCEPTED], st[R.REJECTING] = n_cand, 4, 9, 2
    state = np.array([1, n + 1, n, n - 1], dtype=np.int32)
    cand = np.asarray(cand, dtype=np.int32)
    d_z = torch.from_numpy(z).to(dev)
    d_ids, d_st, d_state, d_cand = _i32(ids, dev), _i32(st, dev), _i32(state, dev), _i32(cand, dev)
    d_tok = torch.from_numpy(tokens).to(dev)
    sel = torch.full((M,), -1, device=dev, dtype=torch.int32)
    ws = torch.zeros(WS_WORDS, device=dev, dtype=torch.float32)
    eos_t = _i32(eos, dev) if eos else None
    for _ in range(2 if twice else 1):
        _lib.call("afk_lookup_accept", d_z.data_ptr(), d_z.stride(0), V, M, d_cand.data_ptr(), d_ids.data_ptr(), d_ids.numel(), d_tok.data_ptr(), max_new, d_st.data_ptr(),
                  d_state.data_ptr(), ops._p(eos_t), len(eos), sel.data_ptr(), ws.data_ptr(), ops._stream())
    want_sel = R.accept(z, cand, ids, tokens, st, state, max_new, eos)
    if twice:
        assert st[R.DONE] == 1, "the second launch is only harmless behind the end: the case must end the call"
    what = (V, M, n_cand, eos, emitted, max_new, done)
    assert d_st.cpu().numpy().tolist() == st.tolist(), what
    assert d_ids.cpu().numpy().tolist() == ids.tolist() and d_tok.cpu().numpy().tolist() == tokens.tolist(), what
    assert d_state.cpu().numpy().tolist() == state.tolist(), what
    assert sel.cpu().numpy().tolist() == ([-1] * M if want_sel is None else want_sel.tolist()), what
    return st


@pytest.mark.parametrize("V", [67, 1031, 152064])
@pytest.mark.parametrize("M", [2, 8, 9, 32])
def test_accept_equals_the_restatement(dev, V, M):
    gen = np.random.default_rng(V + M)
    k = M - 1
    z = gen.standard_normal((M, V)).astype(np.float32)
    top = z.argmax(-1)
    far = lambda j: int((top[j] + V // 2 + 3) % V)   # an id in another slice of the row
    # a tie on row 0 (the lowest id wins), a NaN above everything on row 1 and more NaNs around (never picked)
    lo_id, hi_id = sorted((int(top[0]), far(0)))
    z[0, lo_id] = z[0, hi_id] = 9.0
    z[1, far(1)] = np.nan
    z[1, :3] = np.nan
    sel = np.array([R.argmax_row(z[j]) for j in range(M)])
    assert sel[0] == lo_id and not np.isnan(z[1, sel[1]])
    wrong = lambda j: int((sel[j] + 1) % V)
    full = sel[:k].copy()
    # full acceptance (and the bonus token), zero, partial (at every depth up to 3 and at the last candidate), fewer candidates than rows
    assert _check_accept(dev, z, full, k)[R.N_MATCH] == k
    first_wrong = full.copy()
    first_wrong[0] = wrong(0)
    assert _check_accept(dev, z, first_wrong, k)[R.N_MATCH] == 0
    for j in sorted({1, 2, 3, k - 1} & set(range(1, k))):
        c = full.copy()
        c[j] = wrong(j)
        assert _check_accept(dev, z, c, k)[R.N_MATCH] == j
    assert _check_accept(dev, z, full, 0)[R.N_MATCH] == 0
    if k >= 3:
        assert _check_accept(dev, z, full, k - 2)[R.N_MATCH] == k - 2
    # an eos as the bonus token, and on an accepted row: the step is cut there and the call is done; a second launch changes nothing
    st = _check_accept(dev, z, full, k, eos=(int(sel[k]), 10 ** 7), twice=True)
    assert st[R.DONE] == 1 and (st[R.EMITTED] == 1 + M or int(sel[k]) in sel[:k].tolist())
    st = _check_accept(dev, z, full, k, eos=(10 ** 7, int(sel[0])), twice=True)
    assert st[R.DONE] == 1 and st[R.EMITTED] == 2
    # the budget end: exactly max_new is reached (the draft never offers more; the launch cuts a longer acceptance all the same)
    st = _check_accept(dev, z, full, k, emitted=3, max_new=3 + M, twice=True)
    assert st[R.DONE] == 1 and st[R.EMITTED] == 3 + M
    st = _check_accept(dev, z, full, k, emitted=3, max_new=4, twice=True)
    assert st[R.DONE] == 1 and st[R.EMITTED] == 4 and st[R.N_MATCH] == k
    # done on entry: nothing at all is written
    _check_accept(dev, z, full, k, done=1)
    # rows with nothing finite answer 0: all -inf, all NaN
    z2 = z.copy()
    z2[0, :] = -np.inf
    z2[M - 1, :] = np.nan
    c = np.zeros(k, dtype=np.int32)
    c[1:] = sel[1:k]
    st = _check_accept(dev, z2, c, k)
    assert st[R.N_MATCH] == k   # candidate 0 is id 0, the answer of the all -inf row; the all-NaN bonus row emits 0
    # an unaligned row stride (the scalar path of the slices)
    if V % 4 == 0:
        zs = np.ascontiguousarray(np.concatenate([z, np.zeros((M, 1), np.float32)], 1))[:, :V]
        assert not zs.flags["C_CONTIGUOUS"]
        _check_accept_strided(dev, zs, full, k)


def _check_accept_strided(dev, z, cand, n_cand):
    from audio_flamingo_amd import _lib, ops
    from audio_flamingo_amd.decode_lookup import WS_WORDS

    M, V = z.shape
    base = torch.from_numpy(np.ascontiguousarray(z.base if z.base is not None else z)).to(dev)
    d_z = base[:, :V]
    assert d_z.stride(0) == V + 1
    ids, tokens, st, state = np.zeros(60, dtype=np.int32), np.zeros(64, dtype=np.int64), R.new_status(10), np.array([0, 11, 10, 10], dtype=np.int32)
    st[R.N_CAND] = n_cand
    d_ids, d_st, d_state, d_cand, d_tok = _i32(ids, dev), _i32(st, dev), _i32(state, dev), _i32(cand, dev), torch.from_numpy(tokens).to(dev)
    sel = torch.zeros(M, device=dev, dtype=torch.int32)
    ws = torch.zeros(WS_WORDS, device=dev, dtype=torch.float32)
    _lib.call("afk_lookup_accept", d_z.data_ptr(), d_z.stride(0), V, M, d_cand.data_ptr(), d_ids.data_ptr(), d_ids.numel(), d_tok.data_ptr(), 64, d_st.data_ptr(),
              d_state.data_ptr(), 0, 0, sel.data_ptr(), ws.data_ptr(), ops._stream())
    want = R.accept(np.ascontiguousarray(z), np.asarray(cand, dtype=np.int32), ids, tokens, st, state, 64)
    assert sel.cpu().numpy().tolist() == want.tolist() and d_st.cpu().numpy().tolist() == st.tolist() and d_ids.cpu().numpy().tolist() == ids.tolist()


def test_launches_refuse_what_the_contract_refuses(dev):
    from audio_flamingo_amd import _lib, ops
    from audio_flamingo_amd._lib import AfkError

    t = torch.zeros(64, device=dev, dtype=torch.int32)
    p = t.data_ptr()
    for k, ngram in ((0, 2), (32, 2), (3, 0), (3, 17)):
        with pytest.raises(AfkError, match="afk_lookup_draft"):
            _lib.call("afk_lookup_draft", p, 8, p, p, k, ngram, 8, 0, 0, p, p, p, p, 0, 0, 0, 0, 0, 0, ops._stream())
    for M, V in ((1, 8), (33, 8), (4, 0)):
        with pytest.raises(AfkError, match="afk_lookup_accept"):
            _lib.call("afk_lookup_accept", p, 8, V, M, p, p, 8, 0, 8, p, p, 0, 0, p, p, ops._stream())


# ---------------------------------------------------------------------------------------------- the verify forward, teacher-forced
N_PLAIN = 24   # the golden prompt's first 24 greedy tokens are decisive (see the last test); behind them the trained tiny model runs into ties
_CTX = {}


def _ctx(dev):
    """the trained tiny model (case A), its prompt and audio, and the plain greedy ids every case below is compared with"""
    if dev not in _CTX:
        m, p, audio = _case_a(dev)
        plain = m.generate(p, max_new_tokens=N_PLAIN, **audio)
        assert plain.shape[1] == p.shape[1] + N_PLAIN
        _CTX[dev] = (m, p, audio, plain[0, p.shape[1]:].tolist())
    return _CTX[dev]


def _prefill(m, p, audio, headroom):
    """generate()'s prefill -> (cache, lo, the fp32 logits behind the prompt)"""
    from audio_flamingo_amd import ops

    S0 = p.shape[1]
    lo, padded, Kc, Vt, pos_rows, krange, fast = m._prefill_setup(None, 1, S0, headroom, "test")
    x = m._merged_embeddings(p, audio["input_features"], audio["input_features_mask"])
    y = m._decode_layers(x, 1, S0, 0, (Kc, Vt), pos_rows, krange, fast)
    return (Kc, Vt), lo, ops.gemm_nt(y.reshape(1, S0, -1)[:, -1, :].contiguous(), m.arena["lm_head.weight"].data).float()


@pytest.mark.parametrize("M,cap", [(2, 32), (8, 32), (9, 32), (16, 32), (17, 32), (23, 32), (32, 32), (8, 8), (9, 8), (16, 16), (17, 16), (32, 8)])
def test_verify_forward_teacher_forced(dev, M, cap):
    """one verify step behind the prefill whose candidates are the plain greedy continuation itself: the row argmaxes are the next M greedy tokens; a wrong
    candidate at index j makes the step emit exactly j + 1 tokens; the cache below cur is bit-unchanged and from cur + M on still zero.  cap = the largest M of
    the aliased batched chain (decode_chain_batch_max): M <= cap runs it (one, two and four groups of eight), M > cap runs _decode_layers(n = M) + lm_head.
    Only the 23 decisive continuation tokens are offered as candidates: at M = 32 the rows behind them run on a valid id and nobody reads their logits."""
    from audio_flamingo_amd import _lib
    from audio_flamingo_amd import decode_lookup as D

    m, p, audio, g = _ctx(dev)
    S0, k = p.shape[1], M - 1
    n_cand = min(k, N_PLAIN - 2)
    head, emb = m.arena["lm_head.weight"].data, m.arena[m._lm + "embed_tokens.weight"].data
    m.decode_chain_batch_max = cap
    try:
        assert m._lookup_chain_ok(M, head) == (M <= cap)
        for j_wrong in (None, 0, n_cand // 2, n_cand - 1):
            cache, lo, logits0 = _prefill(m, p, audio, N_PLAIN + k)
            tok0 = logits0.argmax(-1)
            assert int(tok0) == g[0]
            before = (cache[0][:, :, :S0].clone(), cache[1][..., :S0].clone())
            state = torch.cat([lo, torch.tensor([S0 + 1, S0], device=dev, dtype=torch.int32), S0 - lo]).contiguous()
            ls = D.build_state(D.LookupSpec(k, 2), p, tok0, N_PLAIN, (), state, emb.shape[1])
            cand = list(g[1:1 + n_cand]) + [g[0]] * (k - n_cand)
            if j_wrong is not None:
                cand[j_wrong] = (cand[j_wrong] + 1) % 1000
            ls["cand"].copy_(_i32(cand, dev))
            ls["status"][D.N_CAND] = n_cand
            rows = torch.tensor([g[0]] + cand, device=dev)
            ar = torch.arange(M, device=dev, dtype=torch.int32)
            ls["pos"].copy_(state[3] + ar)
            ls["krange"].copy_(torch.stack([state[0].expand(M), state[1] + ar], -1))
            ls["x"].copy_(emb.index_select(0, rows))
            aws = m._decode_attn_workspace(dev, cache[1].shape[4], M) if M <= cap else None
            names = []
            real = _lib.call
            _lib.call = lambda name, *a: (names.append(name), real(name, *a))[1]
            try:
                logits = m._lookup_forward(ls["x"], cache, ls["pos"], ls["krange"], state[2:3], aws, head)
            finally:
                _lib.call = real
            assert (("afk_xattn_fwd" in names) != (M <= cap)) and (("afk_attn_decode_fused" in names) == (M <= cap)), names
            assert logits.shape == (M, head.shape[0]) and logits.dtype == torch.float32
            D.accept(ls, logits)
            n_ok = n_cand + 1 if j_wrong is None else j_wrong + 1
            sel = ls["sel"].tolist()
            assert sel[:n_ok] == g[1:1 + n_ok], (M, cap, j_wrong)
            st = ls["status"].tolist()
            assert st[D.EMITTED] == 1 + n_ok and st[D.N_MATCH] == n_ok - 1 and ls["tokens"][:1 + n_ok].tolist() == g[:1 + n_ok]
            assert state.tolist() == [int(lo), S0 + 1 + n_ok, S0 + n_ok, S0 - int(lo) + n_ok]
            assert torch.equal(cache[0][:, :, :S0], before[0]) and torch.equal(cache[1][..., :S0], before[1])
            assert not cache[0][:, :, S0 + M:].any() and not cache[1][..., S0 + M:].any()
            assert cache[0][:, :, S0:S0 + M].abs().sum(-1).min() > 0   # every row's key landed in its own slot
    finally:
        del m.decode_chain_batch_max


# ---------------------------------------------------------------------------------------------- generate()
def _self_repeating_prompt(p, g):
    """the prompt followed by a stretch of the model's own continuation and the first two ids of that stretch again: the tail 2-gram stands earlier in the
    history with the (permutation-chain) continuation behind it, so drafts are accepted - until the stretch ends and the history disagrees with the model"""
    return torch.cat([p, torch.tensor([g[4:14] + g[4:6]], device=p.device)], 1)


def _unused(p, new):
    used = set(p.flatten().tolist()) | set(new)
    return next(i for i in range(1, 1000) if i not in used)


@pytest.mark.parametrize("use_graph", [False, True])
@pytest.mark.parametrize("n", [1, 2])
@pytest.mark.parametrize("k", [1, 3, 7])
def test_generate_equals_plain_greedy(dev, k, n, use_graph):
    m, p, audio, g = _ctx(dev)
    for prompt in (p, _self_repeating_prompt(p, g)):
        plain = m.generate(prompt, max_new_tokens=24, **audio)
        got = m.generate(prompt, max_new_tokens=24, prompt_lookup_num_tokens=k, max_matching_ngram_size=n, use_graph=use_graph, **audio)
        assert torch.equal(got, plain), (k, n, use_graph, got[0, prompt.shape[1]:].tolist(), plain[0, prompt.shape[1]:].tolist())
        assert m.last_lookup_stats["emitted"] == 24


@pytest.mark.parametrize("k", [3, 7])
def test_generate_every_budget_and_an_eos_list(dev, k):
    m, p, audio, g = _ctx(dev)
    p2 = _self_repeating_prompt(p, g)
    for max_new in sorted({1, 2, k, k + 1, k + 2, 24}):
        for prompt in (p, p2):
            plain = m.generate(prompt, max_new_tokens=max_new, **audio)
            got = m.generate(prompt, max_new_tokens=max_new, prompt_lookup_num_tokens=k, **audio)
            assert got.shape[1] == prompt.shape[1] + max_new and torch.equal(got, plain), (k, max_new)
    # two eos ids: the plain call takes the stop launch and returns the reference's shape - the sequence ends at the eos token
    new2 = m.generate(p2, max_new_tokens=24, **audio)[0, p2.shape[1]:].tolist()
    for prompt, new in ((p, g[:24]), (p2, new2)):
        for at in (0, 6, 23):
            if new[at] in new[:at]:
                continue
            eos = [_unused(prompt, new), new[at]]
            plain = m.generate(prompt, max_new_tokens=24, eos_token_id=eos, **audio)
            assert plain.shape[1] == prompt.shape[1] + at + 1
            for ug in (False, True):
                got = m.generate(prompt, max_new_tokens=24, eos_token_id=eos, prompt_lookup_num_tokens=k, use_graph=ug, **audio)
                assert torch.equal(got, plain), (k, at, ug)


def test_generate_takes_the_fields_from_a_generation_config(dev):
    from transformers import GenerationConfig

    m, p, audio, g = _ctx(dev)
    p2 = _self_repeating_prompt(p, g)
    plain = m.generate(p2, max_new_tokens=24, **audio)
    got = m.generate(p2, generation_config=GenerationConfig(max_new_tokens=24, prompt_lookup_num_tokens=5, max_matching_ngram_size=2), **audio)
    assert torch.equal(got, plain) and m.last_lookup_stats["accepted"] > 0
    with pytest.raises(ValueError, match="batch_size = 1"):
        m.generate(torch.cat([p, p]), max_new_tokens=4, prompt_lookup_num_tokens=3)
    from audio_flamingo_amd._lib import AfkError

    with pytest.raises(AfkError, match="do_sample=True"):
        m.generate(p, max_new_tokens=4, prompt_lookup_num_tokens=3, do_sample=True, **audio)
    with pytest.raises(AfkError, match="logits processors"):
        m.generate(p, max_new_tokens=4, prompt_lookup_num_tokens=3, repetition_penalty=1.2, **audio)
    with pytest.raises(AfkError, match="assistant_model"):
        m.generate(p, max_new_tokens=4, prompt_lookup_num_tokens=3, assistant_model=object(), **audio)
    with pytest.raises(AfkError, match="return_dict_in_generate"):
        m.generate(p, max_new_tokens=4, prompt_lookup_num_tokens=3, return_dict_in_generate=True, **audio)
    with pytest.raises(AfkError, match="streamer="):
        m.generate(p, max_new_tokens=4, prompt_lookup_num_tokens=3, streamer=object(), **audio)


def test_device_route_equals_host_route_accepts_and_rejects(dev, monkeypatch):
    """The self-repeating prompt both accepts and rejects drafts; the device route (two launches inside the captured step) and the host route (torch ops and
    host reads around the same verify forward) give the same ids, steps and accepted counts; the captured step holds no torch selection op and no host rule.

    The id equalities of this file rest on decisive argmaxes, as the batched-versus-single id tests do: the host route's top-1 / top-2 gap at every emitted
    position is asserted to exceed twice the logit bar of tests/_tol.py (2 * 2^-6 * |logit|max, four bf16 ulps of the largest logit), the "confident position"
    rule of the model tests.  Smallest gap seen on the MI355X, in units of that bar: 2.71 on the golden prompt, 2.05 on the self-repeating one (the next
    ones: 2.20, 2.20, 4.12).  Other stretches of the continuation give prompts with gaps down to 0 (ties) and are not used; neither are the golden prompt's
    tokens behind the 24th."""
    from audio_flamingo_amd import _lib
    from audio_flamingo_amd import decode_lookup as D
    from tests._tol import logit_tol

    m, p, audio, g = _ctx(dev)
    p2 = _self_repeating_prompt(p, g)
    gaps, per_step = [], []
    real_accept_host = D.accept_host

    def recording_accept_host(ls, logits):
        before = ls["status"].tolist()
        real_accept_host(ls, logits)
        after = ls["status"].tolist()
        if after[D.STEPS] > before[D.STEPS]:
            e = after[D.EMITTED] - before[D.EMITTED]
            top = logits[:e].topk(2, -1).values
            gaps.extend(((top[:, 0] - top[:, 1]) / logit_tol(float(logits[:e].abs().max()))).tolist())
            per_step.append((after[D.N_MATCH], before[D.N_CAND]))

    for prompt in (p, p2):
        for k in (3, 7):
            plain = m.generate(prompt, max_new_tokens=24, **audio)
            monkeypatch.setattr(D, "accept_host", recording_accept_host)
            m.lookup_on_device = False
            try:
                host = m.generate(prompt, max_new_tokens=24, prompt_lookup_num_tokens=k, **audio)
                host_stats = {k_: v for k_, v in m.last_lookup_stats.items() if k_ != "launched"}
            finally:
                del m.lookup_on_device
                monkeypatch.setattr(D, "accept_host", real_accept_host)
            # the device route: the host rules must not run, torch.argmax runs once (token 0, in front of the steps)
            names, argmaxes = [], []
            real_call, real_argmax = _lib.call, torch.Tensor.argmax
            monkeypatch.setattr(_lib, "call", lambda name, *a: (names.append(name), real_call(name, *a))[1])
            monkeypatch.setattr(torch.Tensor, "argmax", lambda self, *a, **kw: (argmaxes.append(1), real_argmax(self, *a, **kw))[1])
            monkeypatch.setattr(D, "accept_host", None)
            monkeypatch.setattr(D, "draft_host", None)
            try:
                device = m.generate(prompt, max_new_tokens=24, prompt_lookup_num_tokens=k, use_graph=True, **audio)
            finally:
                monkeypatch.undo()
            assert torch.equal(device, host) and torch.equal(device, plain), (k, device[0, prompt.shape[1]:].tolist(), host[0, prompt.shape[1]:].tolist())
            assert {k_: v for k_, v in m.last_lookup_stats.items() if k_ != "launched"} == host_stats, (m.last_lookup_stats, host_stats)
            assert len(argmaxes) == 1 and names.count("afk_lookup_draft") == 2 and names.count("afk_lookup_accept") == 2, (len(argmaxes), names)   # the eager step and the captured one
            assert "afk_decode_select_greedy" not in names and "afk_decode_stop" not in names
            if prompt is p2:   # a condition on the test: a case that accepts nothing tests nothing
                s = host_stats
                assert s["steps"] < s["emitted"] and s["accepted"] > 0 and s["rejecting"] > 0, s
                assert any(nm < nc for nm, nc in per_step) and any(nm > 0 for nm, nc in per_step), per_step
    print("lookup decode: smallest top-1/top-2 gap at an emitted position, in units of the logit bar:", min(gaps), "over", len(gaps), "positions")
    assert min(gaps) > 2.0, min(gaps)

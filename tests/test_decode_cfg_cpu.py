"""CPU: classifier-free guidance of generate(guidance_scale=...) - the fp64 restatement (tests/_cfg_ref.py) against the reference's own class driven with a stub
model, decode_cfg.resolve (keyword against config, validation, refusals) and decode_cfg.layout (where the two prompts lie in the combined cache)."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import _cfg_ref as R

SCALES = (0.5, 1.5, 3.0, 0.0, -1.0)
NINF = float("-inf")


class _Out(dict):
    @property
    def logits(self):
        return self["logits"]


class _Stub:
    """a model that answers planted logits [B, n, V] and keeps what it was called with"""

    def __init__(self, planted):
        self.planted, self.calls = planted, []

    def __call__(self, input_ids, attention_mask=None, use_cache=None, past_key_values=None):
        k = len(self.calls)
        self.calls.append(dict(ids=input_ids.clone(), mask=attention_mask.clone(), use_cache=use_cache, past=past_key_values))
        row = self.planted[k]
        logits = torch.zeros((input_ids.shape[0], input_ids.shape[1], row.shape[-1]))
        logits[:, -1] = row
        return _Out(logits=logits, past_key_values=("cache", k))


def _rows(B, V, seed, scale=8.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn((B, V), generator=g) * scale


def _planted_cases(V=97):
    """(name, cond [B, V], uncond [B, V]): plain rows, -inf in one branch only, in both at the same ids, and rows that are -inf everywhere"""
    zc, zu = _rows(4, V, 1), _rows(4, V, 2)
    one = (zc.clone(), zu.clone())
    one[0][0, 5], one[1][1, 7] = NINF, NINF
    both = (zc.clone(), zu.clone())
    both[0][:, 11], both[1][:, 11] = NINF, NINF
    both[0][2, 3] = NINF
    every = (zc.clone(), zu.clone())
    every[0][1, :], every[1][2, :] = NINF, NINF
    every[0][3, :], every[1][3, :] = NINF, NINF
    return [("plain", zc, zu), ("one branch", *one), ("both branches", *both), ("everywhere", *every)]


@pytest.mark.parametrize("s", SCALES)
def test_restatement_equals_the_reference_class(s):
    from transformers import UnbatchedClassifierFreeGuidanceLogitsProcessor

    ids = torch.arange(4 * 6).reshape(4, 6)
    for name, zc, zu in _planted_cases():
        proc = UnbatchedClassifierFreeGuidanceLogitsProcessor(s, _Stub([zu]), unconditional_ids=ids[:, :3])
        got = proc(ids, zc.clone()).numpy()
        want = R.guided(zc.numpy(), zu.numpy(), s)
        fin = R.same_class(got, want)
        assert fin.any() or name == "everywhere"
        bar = R.bar(s, R.finite_absmax(zc.numpy(), zu.numpy()), zc.shape[1])   # the class computes in fp32: the kernel's bound holds for it as well
        err = float(np.abs(got[fin] - want[fin]).max()) if fin.any() else 0.0
        assert err <= bar, (name, s, err, bar)
        if name == "one branch" and s > 0:
            assert want[0, 5] == NINF and np.isnan(want[1, 7])      # -inf in the conditional row bans the id; in the unconditional row alone: inf - inf
        if name == "both branches":
            assert np.isnan(want[:, 11]).all()                       # -inf - -inf
        if name == "everywhere":
            assert np.isnan(want[1:]).all()


def test_first_pass_takes_the_last_id_and_later_passes_feed_it():
    from transformers import UnbatchedClassifierFreeGuidanceLogitsProcessor

    B, V, S0 = 2, 31, 5
    seq = torch.arange(B * S0).reshape(B, S0)
    for neg, mask in ((None, None), (torch.tensor([[0, 7, 8, 9], [4, 5, 6, 7]]), torch.tensor([[0, 1, 1, 1], [1, 1, 1, 1]])), (torch.tensor([[3], [4]]), None)):
        planted = [_rows(B, V, 10 + k) for k in range(4)]
        stub = _Stub(planted)
        proc = UnbatchedClassifierFreeGuidanceLogitsProcessor(1.5, stub, unconditional_ids=neg, unconditional_attention_mask=mask)
        book = R.UncondBranch(None if neg is None else neg.numpy(), None if mask is None else mask.numpy())
        ids = seq
        for k in range(4):
            zc = _rows(B, V, 50 + k)
            got = proc(ids, zc.clone()).numpy()
            want_ids, want_mask = book.step(ids.numpy())
            call = stub.calls[k]
            assert np.array_equal(call["ids"].numpy(), want_ids) and np.array_equal(call["mask"].numpy(), want_mask), (k, neg is None)
            assert call["use_cache"] is True and call["past"] == (None if k == 0 else ("cache", k - 1))
            want = R.guided(zc.numpy(), planted[k].numpy(), 1.5)
            assert float(np.abs(got - want).max()) <= R.bar(1.5, R.finite_absmax(zc.numpy(), planted[k].numpy()), V)
            ids = torch.cat([ids, torch.tensor([[100 + k], [200 + k]])], dim=1)
        if neg is None:
            assert np.array_equal(stub.calls[0]["ids"].numpy(), seq[:, -1:].numpy()) and stub.calls[0]["mask"].shape == (B, 1)
        assert stub.calls[3]["mask"].shape[1] == stub.calls[0]["mask"].shape[1] + 3 and stub.calls[3]["ids"].tolist() == [[102], [202]]


def test_scale_of_one_is_the_log_softmax_alone():
    zc = _rows(2, 40, 3).numpy()
    assert np.allclose(R.guided(zc, _rows(2, 40, 4).numpy(), 1.0), R.log_softmax64(zc), rtol=0, atol=1e-12)


# ---------------------------------------------------------------------------------------------- resolve
def _resolve(*a, **kw):
    from audio_flamingo_amd import decode_cfg

    return decode_cfg.resolve(*a, **dict(dict(batch_size=2, audio_token_id=1023), **kw))


def test_resolve_inactive_and_keyword_over_config():
    neg = torch.tensor([[1, 2, 3], [4, 5, 6]])
    assert _resolve() is None and _resolve(None, neg) is None and _resolve(1, neg) is None and _resolve(1.0, neg, torch.ones(5, 5)) is None
    gc = SimpleNamespace(guidance_scale=2.5)
    spec = _resolve(None, neg, None, gc)
    assert spec.scale == 2.5 and spec.negative_ids is neg and spec.negative_mask is None
    assert _resolve(3.0, None, None, gc).scale == 3.0, "the keyword wins"
    assert _resolve(1.0, None, None, gc) is None, "a keyword of 1 switches a config's guidance off"
    assert _resolve(None, neg, None, SimpleNamespace(guidance_scale=None)) is None and _resolve(None, neg, None, SimpleNamespace(guidance_scale=1.0)) is None
    for s in (0, 0.0, 0.5, -1.0, 7):
        assert _resolve(s).scale == float(s) and _resolve(s).negative_ids is None
    # inactive: nothing is validated - the reference ignores the negative prompt as well
    assert _resolve(None, torch.ones((5, 3), dtype=torch.long)) is None and _resolve(1.0, torch.full((2, 3), 1023)) is None
    with pytest.raises(ValueError, match="guidance_scale"):
        _resolve("3")


def test_resolve_validation():
    from audio_flamingo_amd._lib import AfkError

    neg = torch.tensor([[1, 2, 3], [4, 5, 6]])
    with pytest.raises(ValueError, match=r"holds 3 rows.*holds 2"):
        _resolve(2.0, torch.ones((3, 4), dtype=torch.long))
    with pytest.raises(ValueError, match="negative_prompt_ids"):
        _resolve(2.0, torch.ones(4, dtype=torch.long))
    with pytest.raises(ValueError, match=r"negative_prompt_attention_mask.*\(2, 4\).*\(2, 3\)"):
        _resolve(2.0, neg, torch.ones((2, 4), dtype=torch.long))
    for holes in ([[1, 0, 1], [1, 1, 1]], [[1, 1, 0], [1, 1, 1]], [[0, 0, 0], [1, 1, 1]]):
        with pytest.raises(AfkError, match="attention masks with holes"):
            _resolve(2.0, neg, torch.tensor(holes))
    left = torch.tensor([[0, 0, 1], [1, 1, 1]])
    assert _resolve(2.0, neg, left).negative_mask is left
    with pytest.raises(AfkError, match="audio placeholder id 1023"):
        _resolve(2.0, torch.tensor([[1, 1023, 3], [4, 5, 6]]))


@pytest.mark.parametrize("how,word", [(dict(num_beams=2), "num_beams > 1"), (dict(use_cache=False), "use_cache=False"), (dict(exact_fp32=True), "AFK_EXACT_FP32=1"),
                                      (dict(lookup=True), "prompt_lookup_num_tokens"), (dict(past=True), "past_key_values"),
                                      (dict(share_prompt=True), "share_prompt=True")])
def test_resolve_refusals_name_the_combination(how, word):
    from audio_flamingo_amd._lib import AfkError

    with pytest.raises(AfkError, match=word) as e:
        _resolve(2.0, **how)
    assert "guidance_scale" in str(e.value)
    assert _resolve(1.0, **how) is None and _resolve(None, **how) is None, "inactive guidance refuses nothing"
    if "share_prompt" in how:
        assert _resolve(2.0, share_prompt=None).scale == 2.0 and _resolve(2.0, share_prompt=False).scale == 2.0


# ---------------------------------------------------------------------------------------------- layout
@pytest.mark.parametrize("S0,lo_c,Sn,lo_u", [(772, [0], 22, [0]), (22, [0], 772, [0]), (40, [0, 0], 1, [0, 0]), (40, [0, 17], 30, [9, 0]), (12, [3, 0], 30, [0, 25])],
                         ids=["Sn<S0", "Sn>S0", "Sn=1", "both-left-padded", "padded-and-longer-negative"])
def test_layout_aligns_both_prompts_to_the_right(S0, lo_c, Sn, lo_u):
    from audio_flamingo_amd import decode_cfg

    lay = decode_cfg.layout(S0, lo_c, Sn, lo_u)
    B, Smax = len(lo_c), max(S0, Sn)
    assert (lay.Smax, lay.off_c, lay.off_u) == (Smax, Smax - S0, Smax - Sn) and min(lay.off_c, lay.off_u) == 0
    lo = lay.lo.tolist()
    assert len(lo) == 2 * B
    for b in range(B):
        # a row's real keys are [lo, Smax): as many as its prompt has real ids, so the first step's rotary position (Smax - lo) is the prompt's real length
        assert Smax - lo[b] == S0 - lo_c[b] and Smax - lo[B + b] == Sn - lo_u[b]
        assert lay.off_c <= lo[b] < Smax and lay.off_u <= lo[B + b] < Smax
    t = decode_cfg.layout(S0, torch.tensor(lo_c, dtype=torch.int32), Sn, torch.tensor(lo_u, dtype=torch.int32))
    assert t.lo.dtype == torch.int32 and t.lo.tolist() == lo
    with pytest.raises(ValueError):
        decode_cfg.layout(S0, lo_c, Sn, lo_u + [0])


def test_materialize_moves_the_conditional_rows_to_slot_zero():
    from audio_flamingo_amd import decode_cfg
    from audio_flamingo_amd.ops import pad64

    L, B, Hkv, D, S0, Sn, T = 2, 2, 2, 4, 5, 9, 12        # the negative prompt is the longer one: the conditional rows start at slot 4
    K = torch.arange(L * 2 * B * T * Hkv * D, dtype=torch.float32).reshape(L, 2 * B, T, Hkv * D)
    Vt = torch.arange(L * 2 * B * Hkv * D * 64, dtype=torch.float32).reshape(L, 2 * B, Hkv, D, 64)
    cfg = decode_cfg.CfgState(scale=2.0, B=B, ws=None, Smax=9, S0=S0, Sn=Sn)
    lo = torch.tensor([4, 6, 0, 3], dtype=torch.int32)
    kv = decode_cfg.materialize(K, Vt, lo, cfg, 7)
    assert kv.get_seq_length() == 7 and kv.lo.tolist() == [0, 2]
    assert kv.K.shape == (L, B, T - 4, Hkv * D) and torch.equal(kv.K, K[:, :B, 4:])
    assert kv.Vt.shape == (L, B, Hkv, D, pad64(T - 4)) and torch.equal(kv.Vt[..., :T - 4], Vt[:, :B, :, :, 4:T]) and not kv.Vt[..., T - 4:].any()

"""CPU: the host side of the shared prompt cache - the fp64 restatement of afk_attn_decode_shared's contract and the teeth of its planted cases
(tests/_shared_ref.py), the split rule, the materialisation of the two caches as one, and decode_share.resolve with its refusals."""
import math

import pytest
import torch

import _attn_probe as P
import _shared_ref as S
from audio_flamingo_amd import decode_share, ops
from audio_flamingo_amd._lib import AfkError


# ------------------------------------------------------------------------------------------------ the reference and the cases
def test_reference_is_softmax_over_the_union_of_both_key_sets():
    """against a direct fp64 softmax written out here: the visible prompt keys of r // n and the visible tail keys of r in ONE softmax"""
    g = torch.Generator().manual_seed(3)
    B0, n, Hq, Hkv, D, Sp, T = 2, 2, 4, 2, 8, 6, 3
    R = B0 * n
    q = torch.randn(R, Hq * D, generator=g)
    Kp, Vp = torch.randn(B0, Sp, Hkv * D, generator=g), torch.randn(B0, Hkv, D, Sp, generator=g)
    Kt, Vt = torch.randn(R, T, Hkv * D, generator=g), torch.randn(R, Hkv, D, T, generator=g)
    pr = torch.tensor([[1, 5], [0, 6]], dtype=torch.int32)
    tr = torch.tensor([[0, 2], [0, 0], [1, 3], [0, 1]], dtype=torch.int32)
    got = S.reference(q, Kp, Vp, Kt, Vt, pr, tr, n, Hq, Hkv, D, D ** -0.5)
    for r in range(R):
        for h in range(Hq):
            hk, b0 = h // (Hq // Hkv), r // n
            ks = torch.cat([Kp[b0, pr[b0, 0]:pr[b0, 1], hk * D:(hk + 1) * D], Kt[r, tr[r, 0]:tr[r, 1], hk * D:(hk + 1) * D]]).double()
            vs = torch.cat([Vp[b0, hk, :, pr[b0, 0]:pr[b0, 1]], Vt[r, hk, :, tr[r, 0]:tr[r, 1]]], -1).double()
            p = torch.softmax(ks @ q[r, h * D:(h + 1) * D].double() * D ** -0.5, 0)
            assert torch.allclose(got[r, h, 0], vs @ p, rtol=1e-12, atol=1e-12), (r, h)


def test_a_continuation_that_sees_no_key_is_a_zero_row():
    q = torch.ones(2, 8)
    z = torch.zeros((2, 2), dtype=torch.int32)
    out = S.reference(q, torch.ones(1, 4, 8), torch.ones(1, 1, 8, 64), torch.ones(2, 3, 8), torch.ones(2, 1, 8, 64), z[:1], z, 2, 1, 1, 8, 1.0)
    assert out.shape == (2, 1, 1, 8) and not out.any()


@pytest.mark.parametrize("case", S.CASES, ids=str)
def test_cases_are_finite_where_visible_and_nan_everywhere_else_but_the_decoys(case):
    c = S.shared_case(*case)
    B0, n, Hq, Hkv, D, Sp, T, ns = case
    assert c.q.stride(0) == (Hq + 2 * Hkv) * D and c.q.shape == (B0 * n, Hq * D)   # a strided view inside the fused q | k | v rows
    decoy_p = {(b, j) for b, _, j, seen in c.planted["prompt"] if not seen}
    decoy_t = {(r, j) for r, _, j, seen in c.planted["tail"] if not seen}
    for b0 in range(B0):
        lo, hi = c.prange[b0].tolist()
        for j in range(Sp):
            fin = bool(torch.isfinite(c.Kp[b0, j].float()).any())
            assert fin == (lo <= j < hi or (b0, j) in decoy_p), (b0, j)
        assert torch.isnan(c.Vtp[b0, :, :, Sp:].float()).all()
    for r in range(B0 * n):
        t0, t1 = c.trange[r].tolist()
        for j in range(T):
            fin = bool(torch.isfinite(c.Kt[r, j].float()).any())
            assert fin == (t0 <= j < t1 or (r, j) in decoy_t), (r, j)
        assert torch.isnan(c.Vtt[r, :, :, T:].float()).all()
    assert torch.isfinite(c.reference()).all()
    if Sp == 0 or T == 0:   # the empty side really is empty
        assert (c.prange[:, 1] == c.prange[:, 0]).all() if Sp == 0 else (c.trange[:, 1] == c.trange[:, 0]).all()


@pytest.mark.parametrize("case", [S.CASES[1], S.CASES[2]], ids=str)
def test_the_planted_keys_have_teeth(case):
    """one key more at either interval end (the decoys) moves a probed slice by at least SEP x the bar"""
    c = S.shared_case(*case)
    ref = c.reference()
    for kw in (dict(dp=1), dict(dt=1)):
        worst = P.slice_errors(c.reference(**kw), ref, c.slots(), c.D)[0][0]
        assert worst >= P.SEP, (kw, worst)


# ------------------------------------------------------------------------------------------------ the split rule
@pytest.mark.parametrize("Hq,Hkv", [(4, 4), (4, 2), (16, 4), (28, 4), (16, 2)])
def test_nsplit_rule(Hq, Hkv):
    for B0 in (1, 2, 8):
        for n in (1, 2, 4, 5, 8, 16):
            for keys in (0, 1, 127, 128, 255, 256, 1000, 7774, 15274, 1 << 20):
                ns = ops.attn_shared_nsplit(B0, n, Hq, Hkv, keys)
                assert 1 <= ns <= ops.ATTN_SHARED_RULE_SPLITS <= ops.ATTN_SHARED_MAX_SPLITS, (B0, n, keys, ns)
                assert ns == 1 or keys // ns >= ops.ATTN_SHARED_MIN_CHUNK, (B0, n, keys, ns)
                tiles = B0 * Hkv * -(-n // (32 // (Hq // Hkv)))
                assert ns == 1 or (ns - 1) * tiles < ops.ATTN_SHARED_TARGET_BLOCKS, (B0, n, keys, ns)
                if keys < 2 * ops.ATTN_SHARED_MIN_CHUNK:
                    assert ns == 1   # a prompt shorter than two chunks is not split


def test_nsplit_rule_at_the_flagship_geometry():
    assert ops.attn_shared_nsplit(1, 8, 28, 4, 7774) == 16     # 4 KV heads x 2 tiles of 4 copies = 8 tiles: the rule's cap
    assert ops.attn_shared_nsplit(1, 16, 28, 4, 1000) == 7     # 128-key chunks at the least
    assert ops.attn_shared_nsplit(8, 16, 28, 4, 15274) == 2    # 128 tiles x 2
    assert ops.attn_shared_nsplit(1, 2, 28, 4, 100) == 1
    assert ops.attn_shared_supported(28, 4, 128, 16) and not ops.attn_shared_supported(28, 4, 128, 17) and not ops.attn_shared_supported(12, 4, 128, 2)
    assert not ops.attn_shared_supported(28, 4, 96, 2)


# ------------------------------------------------------------------------------------------------ the two caches as one
def test_materialize_lays_the_prompt_rows_repeated_and_the_tails_behind_them():
    g = torch.Generator().manual_seed(5)
    L, B0, n, Hkv, D, S0, T = 2, 2, 3, 2, 4, 5, 3
    R, nk = B0 * n, Hkv * D
    Kp, Vtp = torch.randn(L, B0, S0, nk, generator=g), torch.randn(L, B0, Hkv, D, 64, generator=g)
    Kt, Vtt = torch.randn(L, R, T, nk, generator=g), torch.randn(L, R, Hkv, D, 64, generator=g)
    lo = torch.tensor([0, 2], dtype=torch.int32)
    kv = decode_share.materialize(Kp, Vtp, lo, S0, Kt, Vtt, n, S0 + 2)
    assert kv.K.shape == (L, R, S0 + T, nk) and kv.Vt.shape == (L, R, Hkv, D, 64) and kv.length == S0 + 2 == kv.get_seq_length()
    assert kv.lo.tolist() == [0, 0, 0, 2, 2, 2]
    for r in range(R):
        assert torch.equal(kv.K[:, r, :S0], Kp[:, r // n]) and torch.equal(kv.Vt[:, r, :, :, :S0], Vtp[:, r // n, :, :, :S0])
        assert torch.equal(kv.K[:, r, S0:], Kt[:, r]) and torch.equal(kv.Vt[:, r, :, :, S0:S0 + T], Vtt[:, r, :, :, :T])
    assert not kv.Vt[..., S0 + T:].any()   # the pad columns are zero, as AfkKVCache.allocate leaves them
    # a prompt cache with more slots than the prompt (headroom) gives only its first S0
    kv2 = decode_share.materialize(torch.cat([Kp, Kp], 2), Vtp, lo, S0, Kt, Vtt, n, S0)
    assert torch.equal(kv2.K, kv.K) and torch.equal(kv2.Vt, kv.Vt) and kv2.length == S0


# ------------------------------------------------------------------------------------------------ resolve
OK = dict(copies=3, num_beams=1)
REFUSALS = [(dict(use_cache=False), "use_cache=False"), (dict(exact_fp32=True), "AFK_EXACT_FP32=1"), (dict(past=True), "past_key_values="),
            (dict(hooks=True), "logits_processor= / stopping_criteria= / streamer="), (dict(lookup=True), "prompt_lookup_num_tokens="),
            (dict(num_beams=4, beam_device=False), "the host beam loop"), (dict(geometry=False), "outside the batched decode chain")]


@pytest.mark.parametrize("default", [False, True])
def test_resolve_keyword_against_the_class_attribute(default):
    r = decode_share.resolve
    assert r(None, default, **OK) == (decode_share.ShareSpec(n=3, beams=False) if default else None)
    assert r(False, default, **OK) is None
    assert r(True, default, **OK) == decode_share.ShareSpec(n=3, beams=False)
    assert r(True, default, copies=1, num_beams=4) == decode_share.ShareSpec(n=4, beams=True)
    assert r(True, default, copies=3, num_beams=4) == decode_share.ShareSpec(n=4, beams=True)   # the beams are the continuations
    assert r(True, default, copies=1, num_beams=1) is None   # nothing to share: today's route, whatever else is set
    assert r(True, default, copies=1, num_beams=1, use_cache=False, hooks=True) is None
    with pytest.raises(ValueError, match="share_prompt"):
        r(1, default, **OK)


@pytest.mark.parametrize("kw,what", REFUSALS, ids=[w for _, w in REFUSALS])
def test_resolve_refusals(kw, what):
    args = {**OK, **kw}
    with pytest.raises(AfkError) as e:
        decode_share.resolve(True, False, **args)
    assert "share_prompt=True" in str(e.value) and what in str(e.value)
    assert decode_share.resolve(None, True, **args) is None    # the class attribute falls back to today's route silently
    assert decode_share.resolve(False, True, **args) is None
    assert decode_share.resolve(None, False, **args) is None


def test_resolve_names_every_refused_item_of_a_combination():
    with pytest.raises(AfkError) as e:
        decode_share.resolve(True, False, copies=2, use_cache=False, past=True)
    assert "use_cache=False" in str(e.value) and "past_key_values=" in str(e.value)


def test_stats_count_what_is_stored():
    L, B0, n, Hkv, D, S0, T = 2, 1, 4, 2, 64, 100, 8
    z = lambda *s: torch.zeros(s, dtype=torch.bfloat16)
    sh = decode_share.SharedPrompt(cache=(z(L, B0, S0, Hkv * D), z(L, B0, Hkv, D, 128)), prange=None, S0=S0, n=n, pos0=None, trange=None, nsplit=1, ws=None)
    st = decode_share.stats(sh, (z(L, B0 * n, T, Hkv * D), z(L, B0 * n, Hkv, D, 64)), T)
    assert st["prompt_rows"] == 1 and st["copies"] == 4 and st["prompt_slots"] == 100 and st["tail_slots"] == 8
    assert st["cache_bytes"] == 2 * L * Hkv * D * ((100 + 128) + 4 * (8 + 64))
    assert st["unshared_cache_bytes"] == 2 * L * 4 * Hkv * D * (108 + 128) and st["cache_bytes"] < st["unshared_cache_bytes"]
    assert math.isclose(st["unshared_cache_bytes"] / st["cache_bytes"], 4 * 236 / (228 + 288))

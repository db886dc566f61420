"""CPU: the host rules of the append attention and of generate(past_key_values=...) - the split count chosen from the shape, the chunks the kernel cuts a
key hull into (ops.attn_append_chunks restates csrc/attention_append.hip), the attention-mask validation of a continuation and the length check."""
import pytest
import torch

from audio_flamingo_amd import ops
from audio_flamingo_amd._lib import AfkError
from audio_flamingo_amd.generation import continuation_lengths, continuation_mask_check

HEADS = [(4, 4), (4, 2), (16, 4), (28, 4), (16, 2)]   # G = 1, 2, 4, 7, 8


@pytest.mark.parametrize("Hq,Hkv", HEADS)
def test_nsplit_rule_on_edge_shapes(Hq, Hkv):
    for B in (1, 2, 8):
        for n in (1, 2, 31, 32, 33, 64, 768, 5000):
            for keys in (0, 1, 31, 255, 256, 257, 1024, 15000, 1 << 20):
                ns = ops.attn_append_nsplit(B, Hq, Hkv, n, keys)
                assert 1 <= ns <= ops.ATTN_APPEND_RULE_SPLITS <= ops.ATTN_APPEND_MAX_SPLITS, (B, n, keys, ns)
                assert ns == 1 or keys // ns >= ops.ATTN_APPEND_MIN_CHUNK, (B, n, keys, ns)   # no split shorter than the minimum chunk
                tiles = B * Hkv * -(-n // (32 // (Hq // Hkv)))
                assert ns == 1 or (ns - 1) * tiles < ops.ATTN_APPEND_TARGET_BLOCKS, (B, n, keys, ns)   # never more splits than the block target asks for


def test_nsplit_rule_at_the_flagship_geometry():
    """the measured optima of profiles/attn_append.md (AF3 geometry, B = 1): one block per CU"""
    assert ops.attn_append_nsplit(1, 28, 4, 8, 15008) == 16                                 # 8 tiles: the rule's cap
    assert ops.attn_append_nsplit(1, 28, 4, 64, 15064) == 4                                 # 64 tiles x 4
    assert ops.attn_append_nsplit(1, 28, 4, 768, 15768) == 1                                # 768 tiles already
    assert ops.attn_append_nsplit(1, 28, 4, 8, 1032) == 8                                   # 128-key chunks at the least
    assert ops.attn_append_nsplit(1, 28, 4, 8, 100) == 1
    assert ops.attn_append_nsplit(1, 4, 4, 1, 1 << 20) == ops.ATTN_APPEND_RULE_SPLITS == 16  # 4 tiles: the rule's cap, below the kernel's
    assert ops.attn_append_nsplit(2, 28, 4, 64, 15064) == 2 and ops.attn_append_nsplit(8, 28, 4, 64, 1088) == 1   # batches bring their own tiles


@pytest.mark.parametrize("ns", [1, 2, 3, 8, 13, 64])
def test_chunks_cover_the_hull_once_and_are_never_zero_wide_for_a_non_empty_range(ns):
    for lo, hi in [(0, 1), (0, 31), (0, 32), (0, 33), (5, 9), (37, 801), (31, 33), (0, 1000), (901, 7777), (7, 15064), (63, 64)]:
        ch = ops.attn_append_chunks(lo, hi, ns)
        assert len(ch) == ns
        live = [(a, b) for a, b in ch if b > a]
        assert live and live[0][0] == lo and live[-1][1] == hi, (lo, hi, ns, ch)
        assert all(live[i][1] == live[i + 1][0] for i in range(len(live) - 1)), (lo, hi, ns, ch)      # contiguous, no overlap
        assert ch[: len(live)] == live, (lo, hi, ns, ch)                                            # the empty splits are the trailing ones
        assert all(a % 32 == 0 for a, _ in live[1:]), (lo, hi, ns, ch)                              # 32-key boundaries (8-byte value loads)
    assert ops.attn_append_chunks(9, 9, ns) == [(9, 9)] * ns                                        # an empty hull: every split empty


def test_supported_geometries():
    for Hq, Hkv in HEADS:
        assert ops.attn_append_supported(Hq, Hkv, 64) and ops.attn_append_supported(Hq, Hkv, 128)
        assert not ops.attn_append_supported(Hq, Hkv, 32)
    assert not ops.attn_append_supported(12, 4, 128) and not ops.attn_append_supported(5, 2, 64)


def _mask(lo, S):
    return (torch.arange(S)[None, :] >= torch.tensor(lo)[:, None]).long()


def test_continuation_mask_accepts_the_left_padding_of_the_cache():
    continuation_mask_check(_mask([0], 12), torch.tensor([0], dtype=torch.int32), 7, 12)
    continuation_mask_check(_mask([3, 0], 12), torch.tensor([3, 0], dtype=torch.int32), 7, 12)
    continuation_mask_check(_mask([3, 3], 12).bool(), torch.tensor([3, 3], dtype=torch.int32), 7, 12)


@pytest.mark.parametrize("edit", ["hole in the past", "hole in the suffix", "padding moved", "padding dropped", "right padding"])
def test_continuation_mask_refuses_holes(edit):
    lo = torch.tensor([3, 0], dtype=torch.int32)
    am = _mask([3, 0], 12)
    if edit == "hole in the past":
        am[1, 5] = 0
    elif edit == "hole in the suffix":
        am[0, 9] = 0
    elif edit == "padding moved":
        am[0, 3] = 0
    elif edit == "padding dropped":
        am[0, :3] = 1
    else:
        am[1, 11] = 0
    with pytest.raises(AfkError, match="attention masks with holes"):
        continuation_mask_check(am, lo, 7, 12)


def test_continuation_mask_must_cover_the_whole_conversation():
    with pytest.raises(AfkError, match="whole conversation"):
        continuation_mask_check(torch.ones(1, 5, dtype=torch.long), torch.tensor([0], dtype=torch.int32), 7, 12)   # the suffix alone
    with pytest.raises(AfkError, match="whole conversation"):
        continuation_mask_check(torch.ones(2, 12, dtype=torch.long), torch.tensor([0], dtype=torch.int32), 7, 12)


def test_the_cache_must_be_shorter_than_the_conversation():
    assert continuation_lengths(7, 8) == 7
    for P, S in [(8, 8), (9, 8)]:
        with pytest.raises(ValueError, match=rf"{P} positions.*{S}"):
            continuation_lengths(P, S)


def test_routing_stays_inside_the_measured_envelope():
    """_decode_layers(append=True) launches the new kernel only where profiles/attn_append.md measured it to win; everything else - a short past, another
    geometry, a larger batch, a suffix beyond the kernel's grid - keeps the interval kernel instead of raising"""
    from types import SimpleNamespace

    from audio_flamingo_amd.modeling import AudioFlamingo3ForConditionalGeneration as M

    def routed(Hq, Hkv, D, B, n, keys, floor=0):
        me = SimpleNamespace(Hq=Hq, Hkv=Hkv, D=D, append_envelope=M.append_envelope, append_min_keys=floor)
        return M._append_routed(me, B, n, keys)

    assert routed(28, 4, 128, 1, 64, 15064) and routed(28, 4, 128, 8, 8, 264) and routed(4, 2, 64, 1, 8, 780) and routed(16, 2, 128, 1, 64, 8256)
    assert not routed(28, 4, 128, 1, 8, 263) and not routed(28, 4, 128, 9, 64, 15064) and not routed(16, 2, 128, 2, 64, 8256)
    assert not routed(4, 2, 64, 2, 8, 780) and not routed(4, 2, 64, 1, 8, 320)
    assert not routed(28, 4, 64, 1, 64, 15064) and not routed(12, 4, 128, 1, 64, 15064) and not routed(4, 2, 32, 1, 64, 15064)
    assert routed(28, 4, 128, 1, 65535 // 4 * 4, 1 << 20) and not routed(28, 4, 128, 1, 65535 // 4 * 4 + 4, 1 << 20)   # ceil(n / 4) * Hkv <= 65 535
    assert not routed(28, 4, 128, 1, 64, 15064, floor=1 << 30)

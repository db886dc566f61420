"""CPU: the FP8 decode-weight rule as tests/_w8_ref.py restates it (the GPU tests hold afk_quantize_rows_fp8 to that restatement bit for bit), and
decode_w8.resolve - the keyword, the class attribute and every refusal - which is pure host code."""
import pytest
import torch

from tests import _w8_ref as R

BF = torch.bfloat16


def _bf16_neighbour(x, up):
    """the next bf16 above / below a positive bf16 value"""
    b = torch.tensor([x], dtype=BF).view(torch.int16)
    return float((b + (1 if up else -1)).view(BF))


def _smallest_scale_exponent(a):
    """the definition, by search in fp64: the smallest e with a / 2^e <= 448"""
    e = 140
    while e > R.E_MIN and a / 2.0 ** (e - 1) <= R.FP8_MAX:
        e -= 1
    return e


def test_codes_equal_torchs_cast_at_the_defined_scale():
    g = torch.Generator().manual_seed(0)
    for std in (0.02, 1.0, 300.0, 1e-6):
        w = (torch.randn((16, 272), generator=g) * std).to(BF)
        codes, scale = R.quantize(w)
        assert codes.dtype == torch.uint8 and scale.dtype == torch.float32 and codes.shape == w.shape and scale.shape == (16,)
        for r in range(16):
            e = _smallest_scale_exponent(float(w[r].float().abs().max()))
            assert float(scale[r]) == 2.0 ** e
            v = (w[r].double() / 2.0 ** e).float()
            assert float(v.abs().max()) <= R.FP8_MAX
            assert torch.equal(codes[r], v.to(torch.float8_e4m3fn).view(torch.uint8)), f"row {r} at std {std}"
        assert 224.0 < float((w.float().abs().amax(1) / scale).min()) and float((w.float().abs().amax(1) / scale).max()) <= 448.0


@pytest.mark.parametrize("k", [-20, -7, 0, 3, 30])
def test_scale_rule_at_its_corners(k):
    s = 2.0 ** k
    # (row max, expected e): 448 * 2^k sits exactly on the largest code; one bf16 above it needs the next scale; 224 * 2^k is where the scale halves
    cases = [(448.0 * s, k), (_bf16_neighbour(448.0 * s, True), k + 1), (_bf16_neighbour(448.0 * s, False), k),
             (224.0 * s, k - 1), (_bf16_neighbour(224.0 * s, True), k), (_bf16_neighbour(224.0 * s, False), k - 1)]
    for a, e in cases:
        w = torch.zeros((1, 32), dtype=BF)
        w[0, 5], w[0, 9] = -a, a / 4
        codes, scale = R.quantize(w)
        assert float(scale[0]) == 2.0 ** e, (a, e)
        assert e == _smallest_scale_exponent(a)
        assert torch.equal(R.dequantize(codes, scale).float() == 0, w.float() == 0)
    codes, scale = R.quantize(torch.tensor([[448.0 * s, -448.0 * s]], dtype=BF))
    assert codes.tolist() == [[0x7E, 0xFE]]   # the largest finite code, never the NaN pattern 0x7F


def test_zero_rows_and_underflow():
    w = torch.zeros((3, 16), dtype=BF)
    w[1, 0] = 1.0                    # e = -8: the grid's smallest step is 2^-9 * 2^-8 = 2^-17
    w[1, 1], w[1, 2], w[1, 3], w[1, 4] = 2.0 ** -17, 2.0 ** -18, -(2.0 ** -19), 1.5 * 2.0 ** -18
    w[2, 0] = -0.0
    codes, scale = R.quantize(w)
    assert scale.tolist() == [1.0, 2.0 ** -8, 1.0]
    assert int(codes[0].sum()) == 0 and codes[2].tolist() == [0x80] + [0] * 15
    # 2^-17: the smallest subnormal; 2^-18: a tie, to even = 0; -2^-19: (signed) zero; 1.5 * 2^-18: above the tie, rounds up
    assert codes[1, :5].tolist() == [0x78, 0x01, 0x00, 0x80, 0x01]
    with pytest.raises(ValueError):
        R.quantize(torch.tensor([[1.0, float("nan")]], dtype=BF))


def test_dequantize_quantize_is_idempotent_on_values():
    g = torch.Generator().manual_seed(1)
    w = (torch.randn((32, 512), generator=g) * 0.05).to(BF)
    w[3] = 0
    w[4].clamp_(-0.25, 0.25)
    w[4, 7] = 225.0 * 2.0 ** -9      # the corner: the row max rounds DOWN to 224 * 2^e, so the second pass picks e - 1 and doubles every code - the values stay
    w[5, 0] = 50.0                   # an outlier: the rest of the row falls into the subnormals or to zero
    once = R.snap(w)
    c1, s1 = R.quantize(w)
    assert torch.equal(once.float(), c1.view(torch.float8_e4m3fn).float() * s1[:, None]), "code * scale is exact in bf16"
    c2, s2 = R.quantize(once)
    assert torch.equal(R.dequantize(c2, s2).float(), once.float())
    assert torch.equal(R.snap(once), once)
    assert float(once[4, 7]) == 224.0 * 2.0 ** -9 and float(s2[4]) * 2 == float(s1[4]) and not torch.equal(c1[4], c2[4])


def test_resolve_values_refusals_and_the_silent_default():
    from audio_flamingo_amd import decode_w8
    from audio_flamingo_amd._lib import AfkError

    assert decode_w8.resolve(None) is False and decode_w8.resolve("bf16") is False and decode_w8.resolve("bf16", "fp8") is False
    assert decode_w8.resolve("fp8") is True and decode_w8.resolve(None, "fp8") is True
    for bad in ("int8", "FP8", 8, True):
        with pytest.raises(ValueError, match="decode_weights"):
            decode_w8.resolve(bad)
    with pytest.raises(ValueError, match="decode_weight_dtype"):
        decode_w8.resolve(None, "e4m3")
    refusals = [(dict(rows=2), "more than one row"), (dict(num_beams=3), "num_beams > 1"), (dict(copies=2), "num_return_sequences > 1"),
                (dict(guidance=True), "guidance_scale"), (dict(lookup=True), "prompt_lookup_num_tokens"), (dict(share_prompt=True), "share_prompt=True"),
                (dict(use_cache=False), "use_cache=False"), (dict(exact_fp32=True), "AFK_EXACT_FP32=1"), (dict(chain_ok=False), "single-sequence decode chain"),
                (dict(widths_ok=False), "multiple of 16"), (dict(head_ok=False), "multiple of 8")]
    for kw, word in refusals:
        with pytest.raises(AfkError, match=word):
            decode_w8.resolve("fp8", **kw)
        assert decode_w8.resolve(None, "fp8", **kw) is False   # the class attribute on: today's route, silently
        assert decode_w8.resolve("bf16", "fp8", **kw) is False
    with pytest.raises(AfkError, match="num_beams > 1 / use_cache=False"):
        decode_w8.resolve("fp8", num_beams=2, use_cache=False)
    assert decode_w8.resolve("fp8", share_prompt=False) is True and decode_w8.resolve("fp8", share_prompt=None) is True

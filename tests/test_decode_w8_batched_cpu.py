"""CPU: decode_w8.resolve with the batched switch (decode_weights_batched= / AFK_DECODE_WEIGHTS_BATCHED) - pure host code.

Off (the default), every call of tests/test_decode_w8_cpu.py keeps its result and its message; on, a decode step of 2 - 8 rows takes the FP8 copy for a batch of
prompts, sampled copies, beams, guidance, prompt-lookup decoding and a shared prompt, and what stays refused is named under the keyword and silently bf16 under the
class default."""
import pytest

REFUSALS_ONE_ROW = [(dict(rows=2), "more than one row"), (dict(num_beams=3), "num_beams > 1"), (dict(copies=2), "num_return_sequences > 1"),
                    (dict(guidance=True), "guidance_scale"), (dict(lookup=True), "prompt_lookup_num_tokens"), (dict(share_prompt=True), "share_prompt=True"),
                    (dict(use_cache=False), "use_cache=False"), (dict(exact_fp32=True), "AFK_EXACT_FP32=1"), (dict(chain_ok=False), "single-sequence decode chain"),
                    (dict(widths_ok=False), "multiple of 16"), (dict(head_ok=False), "multiple of 8")]

# (what the call is, resolve's keywords): every combination the batched switch admits, with the rows of its decode step
ALLOWED = [("a batch of two prompts", dict(rows=2)), ("a batch of eight prompts", dict(rows=8)),
           ("two sampled copies", dict(rows=2, copies=2)), ("two prompts x three copies", dict(rows=6, copies=3)),
           ("two beams", dict(num_beams=2)), ("two prompts x four beams", dict(rows=2, num_beams=4)), ("beams with two returned", dict(num_beams=3, copies=2)),
           ("guidance, one prompt", dict(guidance=True)), ("guidance, four prompts", dict(rows=4, guidance=True)),
           ("prompt lookup, k = 3", dict(lookup=True, step_rows=4)), ("prompt lookup, k = 7", dict(lookup=True, step_rows=8)),
           ("two copies on a shared prompt", dict(rows=2, copies=2, share_prompt=True)), ("shared beams", dict(num_beams=4, share_prompt=True))]


def _resolve():
    from audio_flamingo_amd import decode_w8

    return decode_w8.resolve


def test_off_every_existing_result_and_message_is_unchanged():
    from audio_flamingo_amd._lib import AfkError

    resolve = _resolve()
    for extra in (dict(), dict(batched=False), dict(batched=False, batched_ok=False)):
        assert resolve(None, **extra) is False and resolve("bf16", **extra) is False and resolve("bf16", "fp8", **extra) is False
        assert resolve("fp8", **extra) is True and resolve(None, "fp8", **extra) is True
        for bad in ("int8", "FP8", 8, True):
            with pytest.raises(ValueError, match="decode_weights"):
                resolve(bad, **extra)
        with pytest.raises(ValueError, match="decode_weight_dtype"):
            resolve(None, "e4m3", **extra)
        for kw, word in REFUSALS_ONE_ROW:
            with pytest.raises(AfkError, match=word) as e:
                resolve("fp8", **kw, **extra)
            assert "single-sequence decode chain only" in str(e.value) and "decode_weights_batched" not in str(e.value)
            assert resolve(None, "fp8", **kw, **extra) is False
            assert resolve("bf16", "fp8", **kw, **extra) is False
        with pytest.raises(AfkError, match="num_beams > 1 / use_cache=False"):
            resolve("fp8", num_beams=2, use_cache=False, **extra)
        assert resolve("fp8", share_prompt=False, **extra) is True and resolve("fp8", share_prompt=None, **extra) is True


def test_the_switch_is_keyword_only():
    with pytest.raises(TypeError):
        _resolve()("fp8", "bf16", True)


@pytest.mark.parametrize("what,kw", ALLOWED, ids=[a[0] for a in ALLOWED])
def test_on_each_allowed_combination_takes_the_fp8_copy(what, kw):
    from audio_flamingo_amd._lib import AfkError

    resolve = _resolve()
    assert resolve("fp8", batched=True, **kw) is True, what
    assert resolve(None, "fp8", batched=True, **kw) is True, what
    assert resolve("bf16", "fp8", batched=True, **kw) is False and resolve(None, "bf16", batched=True, **kw) is False   # the switch alone turns nothing on
    # the same call without the switch is refused as before
    with pytest.raises(AfkError, match="single-sequence decode chain only"):
        resolve("fp8", **kw)
    # ... and what stays refused with it: by name under the keyword, today's route under the class default
    for extra, word in ((dict(assist=True), "assistant_model="), (dict(use_cache=False), "use_cache=False"), (dict(exact_fp32=True), "AFK_EXACT_FP32=1"),
                        (dict(batched_ok=False), "norm-in-prologue")):
        with pytest.raises(AfkError, match=word) as e:
            resolve("fp8", batched=True, **kw, **extra)
        assert "decode_weights_batched=True" in str(e.value)
        assert resolve(None, "fp8", batched=True, **kw, **extra) is False


def test_on_more_than_eight_rows_are_named():
    from audio_flamingo_amd._lib import AfkError

    resolve = _resolve()
    for kw, n in ((dict(rows=9), 9), (dict(rows=3, num_beams=3), 9), (dict(rows=5, guidance=True), 10), (dict(lookup=True, step_rows=9), 9),
                  (dict(rows=12, copies=4, share_prompt=True), 12)):
        with pytest.raises(AfkError, match=f"{n} rows in a decode step") as e:
            resolve("fp8", batched=True, **kw)
        assert "norm-in-prologue" not in str(e.value)   # the row count is the reason, whatever batched_ok would have said
        with pytest.raises(AfkError, match=f"{n} rows in a decode step"):
            resolve("fp8", batched=True, batched_ok=False, **kw)
        assert resolve(None, "fp8", batched=True, **kw) is False
    with pytest.raises(AfkError, match="9 rows in a decode step .* / assistant_model= / use_cache=False"):
        resolve("fp8", batched=True, rows=9, assist=True, use_cache=False)


def test_on_one_row_keeps_the_single_sequence_rules():
    from audio_flamingo_amd._lib import AfkError

    resolve = _resolve()
    assert resolve("fp8", batched=True) is True and resolve(None, "fp8", batched=True) is True
    assert resolve("fp8", batched=True, batched_ok=False) is True   # batched_ok speaks about steps of 2 - 8 rows only
    for kw, word in ((dict(use_cache=False), "use_cache=False"), (dict(exact_fp32=True), "AFK_EXACT_FP32=1"), (dict(chain_ok=False), "single-sequence decode chain"),
                     (dict(widths_ok=False), "multiple of 16"), (dict(head_ok=False), "multiple of 8"), (dict(assist=True), "assistant_model="),
                     (dict(share_prompt=True), "share_prompt=True")):
        with pytest.raises(AfkError, match=word) as e:
            resolve("fp8", batched=True, **kw)
        assert "single-sequence decode chain only" in str(e.value)
        assert resolve(None, "fp8", batched=True, **kw) is False

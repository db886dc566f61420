"""CPU: the yardsticks of the device sampler (tests/_sampler_ref.py) against known answers and against the torch restatement of the reference's logits
warpers (modeling._select_token), and the host side of afk_decode_sample: declared, exported, refusing bad arguments before any GPU work."""
import numpy as np
import pytest
import torch

from tests import _sampler_ref as R

CASES = [(1.0, 50, 1.0), (0.7, 50, 0.9), (1.3, 0, 0.9), (1.0, 0, 0.5), (1.5, 20, 0.95), (1.0, None, 0.999)]   # (T, k, p); None: k = V


def test_philox4x32_10_known_answers():
    """Random123's kat_vectors for philox4x32-10"""
    kat = [((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
           ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
           ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), "d16cfe09 94fdcceb 5001e420 24126ea1")]
    for ctr, key, want in kat:
        assert " ".join(f"{w:08x}" for w in R.philox4x32_10(ctr, key)) == want
    u = R.uniform(0x1234_5678_9ABC, 5, 3)
    assert 0.0 <= u < 1.0 and u * 2 ** 24 == int(u * 2 ** 24)
    assert R.uniform(0x1234_5678_9ABC, 5, 3) != R.uniform(0x0000_5678_9ABC, 5, 3), "the high seed word is part of the key"


def _torch_kept(monkeypatch, logits, T, k, p):
    """the support of the distribution modeling._select_token hands to torch.multinomial"""
    from audio_flamingo_amd.modeling import AudioFlamingo3ForConditionalGeneration as Mine

    seen = []
    monkeypatch.setattr(torch, "multinomial", lambda probs, n, generator=None: (seen.append(probs), probs.argmax(-1, keepdim=True))[1])
    Mine._select_token(logits[None], dict(temperature=T, top_k=k, top_p=p, generator=None))
    return (seen[0][0] > 0).numpy()


@pytest.mark.parametrize("V", [37, 1000, 152064])
def test_reference_kept_set_equals_the_torch_chain_on_tie_free_logits(monkeypatch, V):
    torch.manual_seed(0)
    for scale in (1.0, 4.0):
        x = torch.randn(V) * scale
        assert torch.unique(x).numel() >= 0.99 * V      # fp32 randn: a few dozen repeated values among 152 064, none of them at a threshold below
        for T, k, p in CASES:
            k = V if k is None else k
            ref = R.reference(x, T, k, p)
            assert np.array_equal(ref["keep"], _torch_kept(monkeypatch, x, T, k, p)), (V, scale, T, k, p)
            assert abs(ref["r"].sum() - 1.0) < 1e-12 and ref["keep"][int(x.argmax())]


@pytest.mark.parametrize("V", [1000, 152064])
def test_reference_kept_set_on_bf16_valued_logits_differs_from_the_torch_chain_only_inside_the_threshold_class(monkeypatch, V):
    """ties are the rule on lm_head outputs: top-p keeps or drops a class of equal values as a whole where the reference's sort splits it"""
    for scale in (1.0, 4.0):
        x = R.bf16_logits(V, scale, seed=V + int(scale))
        for T, k, p in CASES:
            k = V if k is None else k
            row = R.Row(x, T)
            if p < 1.0:
                p, half = row.snap_top_p(k, p)
                assert half > 1e-6     # the torch chain sums in fp32
            ref = row.result(k, p)
            tk = _torch_kept(monkeypatch, x, T, k, p)
            assert not (tk & ~ref["keep"]).any(), (V, scale, T, k, p)
            extra = ref["keep"] & ~tk
            assert not extra.any() or bool((row.z[extra] == row.z[ref["keep"]].min()).all()), (V, scale, T, k, p)


def test_reference_draw_and_degenerate_rows():
    x = torch.tensor([0.0, 1.0, float("-inf"), 1.0, float("nan"), 2.0])
    ref = R.reference(x, 1.0, 3, 1.0)
    assert ref["keep"].tolist() == [False, True, False, True, False, True]
    assert R.draw(ref, 0.0) == 1 and R.draw(ref, 1.0 - 2.0 ** -24) == 5 and R.draw(ref, float(ref["cdf"][1]) + 1e-9) == 3
    half = R.reference(x, 1.0, 0, 0.6)          # the two 1.0 stay or go together: cumulative class masses 0.072 / 0.466 / 1
    assert half["keep"].tolist() == [False, True, False, True, False, True]
    assert R.reference(x, 1.0, 0, 0.4)["keep"].tolist() == [False, False, False, False, False, True]
    inf = R.reference(torch.tensor([1.0, float("inf"), 3.0, float("inf")]), 0.7, 2, 0.9)
    assert inf["keep"].tolist() == [False, True, False, False] and R.draw(inf, 0.99) == 1
    none = R.reference(torch.tensor([float("-inf"), float("nan")]), 1.0, 0, 0.9)
    assert not none["keep"].any() and R.draw(none, 0.3) == 0


def test_decode_sample_is_declared_exported_and_validates_without_a_device():
    from audio_flamingo_amd import _lib, ops

    protos = _lib.prototypes()
    assert "afk_decode_sample" in protos and hasattr(_lib.load(), "afk_decode_sample")
    names = protos["afk_decode_sample"][2]
    assert names[:4] == ["logits", "ld_logits", "B", "V"] and "seed" in names and "step_base" in names and names[-1] == "stream"
    buf = torch.zeros(64, dtype=torch.float32)     # host memory: never touched - validation fails first
    p = buf.data_ptr()

    def call(logits=p, ld=64, B=1, V=64, T=1.0, k=0, top_p=1.0, nxt=p, ld_probs=0, tokens_out=None, state=None, emb=None, H=0, x_out=None):
        _lib.call("afk_decode_sample", logits, ld, B, V, T, k, top_p, None, 0, None, 0, nxt, None, ld_probs, None, tokens_out, 0, state, emb, 0, H, x_out, 0)

    with pytest.raises(_lib.AfkError, match="null"):
        call(logits=None)
    with pytest.raises(_lib.AfkError, match="null"):
        call(nxt=None)
    with pytest.raises(_lib.AfkError, match="V <= 8388608"):
        call(V=0)
    with pytest.raises(_lib.AfkError, match="B >= 1"):
        call(B=0)
    with pytest.raises(_lib.AfkError, match="row strides >= V"):
        call(ld=32)
    with pytest.raises(_lib.AfkError, match="temperature > 0"):
        call(T=0.0)
    with pytest.raises(_lib.AfkError, match="temperature > 0"):
        call(T=float("nan"))
    with pytest.raises(_lib.AfkError, match="top_p > 0"):
        call(top_p=0.0)
    with pytest.raises(_lib.AfkError, match="B == 1"):
        call(B=2, state=p, emb=p, x_out=p, H=8)
    with pytest.raises(_lib.AfkError, match="H %% 4|H % 4"):
        call(state=p, emb=p, x_out=p, H=6)
    with pytest.raises(_lib.AfkError, match="state"):
        call(tokens_out=p)
    with pytest.raises(_lib.AfkError, match="HIP device tensor"):
        ops.decode_sample(torch.zeros(2, 64), top_k=5)

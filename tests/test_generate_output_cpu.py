"""CPU: the output object of generate(return_dict_in_generate=True) against the reference's GenerateDecoderOnlyOutput built from the same fields, and the
resolution of the output flags (generation_output.resolve_output_flags) against a GenerationConfig.  No GPU, no library load."""
import pytest
import torch

from audio_flamingo_amd._lib import AfkError
from audio_flamingo_amd.generation_output import AfkGenerateOutput, OutputFlags, resolve_output_flags, step_buffer_view


def _fields(with_logits=True, with_scores=True):
    buf = torch.arange(3 * 2 * 5, dtype=torch.float32).view(3, 2, 5)
    return dict(sequences=torch.arange(14).view(2, 7), scores=tuple(buf[i] + 0.5 for i in range(3)) if with_scores else None,
                logits=tuple(buf[i] for i in range(3)) if with_logits else None, past_key_values=object())


@pytest.mark.parametrize("with_logits,with_scores", [(True, True), (True, False), (False, True), (False, False)])
def test_output_object_has_the_access_surface_of_the_reference_class(with_logits, with_scores):
    from transformers.generation.utils import GenerateDecoderOnlyOutput

    f = _fields(with_logits, with_scores)
    ours, ref = AfkGenerateOutput(**f), GenerateDecoderOnlyOutput(**f)
    assert list(ours.keys()) == list(ref.keys()) == [k for k in ("sequences", "scores", "logits", "past_key_values") if f[k] is not None]
    assert list(ours) == list(ref) and len(ours) == len(ref)
    assert ours.attentions is None and ours.hidden_states is None and "attentions" not in ours.keys()
    same = lambda a, b: a is b or (isinstance(a, tuple) and len(a) == len(b) and all(x is y for x, y in zip(a, b)))
    for k in ref.keys():
        assert same(ours[k], ref[k]) and same(getattr(ours, k), getattr(ref, k)) and k in ours
    rt, ot = ref.to_tuple(), ours.to_tuple()
    assert len(rt) == len(ot) and all(same(a, b) for a, b in zip(ot, rt))
    for i in range(len(rt)):
        assert same(ours[i], ref[i])
    assert all(same(a, b) for a, b in zip(ours[:2], ref[:2])) and len(ours[1:]) == len(ref[1:])
    assert [k for k, _ in ours.items()] == [k for k, _ in ref.items()]
    for missing in [k for k in ("scores", "logits", "attentions") if f.get(k) is None]:
        with pytest.raises(KeyError):
            ref[missing]
        with pytest.raises(KeyError):
            ours[missing]
    with pytest.raises(KeyError):
        ours["no_such_field"]
    with pytest.raises(IndexError):
        ours[len(rt)]


def test_flags_a_keyword_beats_the_generation_config():
    from transformers import GenerationConfig

    gc = GenerationConfig(return_dict_in_generate=True, output_scores=True, output_logits=False)
    assert resolve_output_flags(generation_config=gc) == OutputFlags(True, True, False)
    assert resolve_output_flags(output_logits=True, generation_config=gc) == OutputFlags(True, True, True)
    assert resolve_output_flags(output_scores=False, generation_config=gc) == OutputFlags(True, False, False)
    assert resolve_output_flags(return_dict_in_generate=False, generation_config=gc) == OutputFlags(False, False, False)
    assert resolve_output_flags(return_dict_in_generate=True, output_logits=True, generation_config=GenerationConfig()) == OutputFlags(True, False, True)
    assert resolve_output_flags(return_dict_in_generate=True) == OutputFlags(True, False, False) and not resolve_output_flags(return_dict_in_generate=True).collect
    assert resolve_output_flags() == OutputFlags(False, False, False)


def test_flags_scores_without_the_dict_collect_nothing():
    from transformers import GenerationConfig

    for kw in (dict(output_scores=True), dict(output_logits=True), dict(output_scores=True, output_logits=True),
               dict(generation_config=GenerationConfig(output_scores=True, output_logits=True))):
        fl = resolve_output_flags(**kw)
        assert fl == OutputFlags(False, False, False) and not fl.collect and not fl.return_dict
    # ... and such a call is the plain call: nothing about it is refused
    assert resolve_output_flags(output_scores=True, num_beams=4, use_cache=False, exact_fp32=True) == OutputFlags()


@pytest.mark.parametrize("how,word", [(dict(num_beams=2), "num_beams"), (dict(use_cache=False), "use_cache=False"), (dict(exact_fp32=True), "AFK_EXACT_FP32")])
def test_flags_refused_combinations_name_themselves(how, word):
    from transformers import GenerationConfig

    with pytest.raises(AfkError, match=word):
        resolve_output_flags(return_dict_in_generate=True, output_scores=True, **how)
    with pytest.raises(AfkError, match=word):
        resolve_output_flags(generation_config=GenerationConfig(return_dict_in_generate=True), **how)


@pytest.mark.parametrize("name", ["output_attentions", "output_hidden_states"])
def test_flags_attentions_and_hidden_states_are_refused(name):
    from types import SimpleNamespace

    with pytest.raises(AfkError, match=name):
        resolve_output_flags(**{name: True})
    with pytest.raises(AfkError, match=name):
        resolve_output_flags(return_dict_in_generate=True, generation_config=SimpleNamespace(**{name: True}))
    assert resolve_output_flags(**{name: False}, generation_config=SimpleNamespace(**{name: True})) == OutputFlags()


def test_step_buffer_view_finds_the_buffer_behind_consecutive_views():
    buf = torch.arange(4 * 3 * 5, dtype=torch.float32).view(4, 3, 5)
    rows = tuple(buf[i] for i in range(1, 4))
    v = step_buffer_view(rows)
    assert v is not None and v.data_ptr() == buf[1].data_ptr() and torch.equal(v, buf[1:])
    wide = torch.zeros(4, 3, 8)[:, :, :5]                              # rows with a pitch
    v = step_buffer_view(tuple(wide[i] for i in range(4)))
    assert v is not None and v.stride() == (24, 8, 1) and v.shape == (4, 3, 5)
    assert step_buffer_view((buf[0],)).shape == (1, 3, 5)
    assert step_buffer_view((buf[0], buf[2], buf[3])) is None          # no constant stride
    assert step_buffer_view((buf[1], buf[0])) is None                  # descending
    assert step_buffer_view((buf[0], buf[1].clone())) is None          # another storage
    assert step_buffer_view((buf[0], buf[1].double())) is None

"""GPU: what generate() enqueues and returns, mode by mode, against a recording (tests/golden/generate_trace.json): the ordered names of the library entry
points one call goes through (a spy on _lib.call; a captured step is seen once, while it is captured) and the ids it returns behind the prompt.  The recording pins the
host side of generate() - which launches, in which order, on which route - so that moving that code cannot move a launch unnoticed; the arithmetic is
pinned elsewhere (test_sampler_gpu, test_decode_process_gpu, test_decode_stop_gpu, test_generate_output_gpu, test_beam_gpu, test_model_gpu).

AFK_GENERATE_TRACE_RECORD=<path of a json file>: record instead of compare (every case adds its entry to that file).  A difference after a change that
was meant to leave generate() alone is a failure of that change, not a reason to record again."""
import json
import os

import pytest
import torch

from tests import _stop_ref as R
from tests.test_sampler_gpu import SAMPLED, _case_a, _Collect

pytestmark = pytest.mark.gpu

NEW = 12
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "generate_trace.json")
RECORD = os.environ.get("AFK_GENERATE_TRACE_RECORD")
FLAGS = dict(return_dict_in_generate=True, output_scores=True, output_logits=True)
_CTX = {}


def _ctx(dev):
    """the tiny golden model, its prompt and audio, and the 12 plain greedy ids the eos / stop-string cases are built from (that call also warms every
    per-model cache, so a case's trace does not depend on which case ran first)"""
    if dev not in _CTX:
        m, p, audio = _case_a(dev)
        plain = m.generate(p, max_new_tokens=NEW, **audio)
        _CTX[dev] = (m, p, audio, plain[0, p.shape[1]:].tolist())
    return _CTX[dev]


def _padded_batch(dev):
    g = torch.Generator().manual_seed(3)
    ids, att = torch.zeros((3, 40), dtype=torch.long), torch.zeros((3, 40), dtype=torch.long)
    for i, n in enumerate((40, 23, 31)):
        ids[i, 40 - n:] = torch.randint(0, 256, (n,), generator=g)
        att[i, 40 - n:] = 1
    return ids.to(dev), att.to(dev)


def _unused(p, new):
    used = set(p.flatten().tolist()) | set(new)
    return next(i for i in range(1, 1023) if i not in used)


def _greedy(m, p, audio, new, **kw):
    return m.generate(p, max_new_tokens=NEW, **audio, **kw)


def _sampled(m, p, audio, new, **kw):
    return m.generate(p, **audio, **SAMPLED, **kw)


def _eos_list(m, p, audio, new):
    assert new[6] not in new[:6]
    return m.generate(p, eos_token_id=[_unused(p, new), new[6]], max_new_tokens=NEW, **audio)


def _stop_string(m, p, audio, new):
    assert len(set(new[3:6])) == 3
    tok = R.tiny_tokenizer({new[3]: "Hel", new[4]: "lo", new[5]: " world"})
    return m.generate(p, stop_strings=["lo w"], tokenizer=tok, max_new_tokens=NEW, **audio)


def _padded(m, p, audio, new):
    ids, att = _padded_batch(p.device)
    return m.generate(ids, attention_mask=att, max_new_tokens=NEW)


def _beams_host(m, p, audio, new):
    m.beam_on_device = False
    try:
        return m.generate(p, num_beams=3, max_new_tokens=NEW, **audio)
    finally:
        del m.beam_on_device


MODES = {
    "greedy": _greedy,
    "greedy_repetition_penalty": lambda *a: _greedy(*a, repetition_penalty=1.3),
    "sampled": _sampled,
    "sampled_processors_dict": lambda *a: _sampled(*a, repetition_penalty=1.3, no_repeat_ngram_size=2, **FLAGS).sequences,
    "eos_list": _eos_list,
    "stop_string": _stop_string,
    "padded_batch_of_three": _padded,
    "beams_device": lambda *a: _greedy(*a, num_beams=3),
    "beams_host": _beams_host,
    "greedy_streamer": lambda *a: _greedy(*a, streamer=_Collect()),
    "greedy_eager": lambda *a: _greedy(*a, use_graph=False),
    "greedy_graph": lambda *a: _greedy(*a, use_graph=True),
    "greedy_repetition_penalty_eager": lambda *a: _greedy(*a, repetition_penalty=1.3, use_graph=False),
    "greedy_repetition_penalty_graph": lambda *a: _greedy(*a, repetition_penalty=1.3, use_graph=True),
    "sampled_eager": lambda *a: _sampled(*a, use_graph=False),
    "sampled_graph": lambda *a: _sampled(*a, use_graph=True),
}


@pytest.mark.parametrize("mode", list(MODES))
def test_generate_enqueues_and_returns_what_was_recorded(dev, mode, monkeypatch):
    from audio_flamingo_amd import _lib

    m, p, audio, new = _ctx(dev)
    assert type(m).beam_on_device, "the device route is the default"
    names = []
    real = _lib.call
    monkeypatch.setattr(_lib, "call", lambda name, *a: (names.append(name), real(name, *a))[1])
    out = MODES[mode](m, p, audio, new)
    monkeypatch.undo()
    inp = _padded_batch(dev)[0] if mode == "padded_batch_of_three" else p
    S0 = inp.shape[1]
    assert torch.equal(out[:, :S0], inp), mode   # the prompt comes back in front: the recording holds the generated columns only
    got = {"calls": names, "ids": out[:, S0:].tolist()}
    assert all(isinstance(n, str) for n in names) and all(isinstance(i, int) for row in got["ids"] for i in row)
    if RECORD:   # the file: {"names": the entry points seen so far, "modes": {mode: {"calls": indices into names, "ids": the generated columns}}}
        book = {"names": [], "modes": {}}
        if os.path.exists(RECORD):
            with open(RECORD) as f:
                book = json.load(f)
        book["names"] += sorted(set(names) - set(book["names"]))
        index = {n: i for i, n in enumerate(book["names"])}
        book["modes"][mode] = {"calls": [index[n] for n in names], "ids": got["ids"]}
        os.makedirs(os.path.dirname(os.path.abspath(RECORD)), exist_ok=True)
        with open(RECORD, "w") as f:
            json.dump(book, f, separators=(",", ":"), sort_keys=True)
        return
    with open(FIXTURE) as f:
        book = json.load(f)
    want = {"calls": [book["names"][i] for i in book["modes"][mode]["calls"]], "ids": book["modes"][mode]["ids"]}
    assert got["ids"] == want["ids"], (mode, got["ids"], want["ids"])
    diff = next((i for i, (a, b) in enumerate(zip(names, want["calls"])) if a != b), min(len(names), len(want["calls"])))
    assert names == want["calls"], (mode, f"{len(names)} calls against {len(want['calls'])} recorded; first difference at {diff}",
                                   names[max(diff - 3, 0): diff + 3], want["calls"][max(diff - 3, 0): diff + 3])

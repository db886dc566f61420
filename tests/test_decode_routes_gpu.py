"""GPU: the routes of the cached decoder forward that generate()'s recording (test_generate_trace_gpu) does not reach, each against a recording
(tests/golden/decode_routes.json): ONE call of _decode_logits, _lookup_forward, _forward_cached or _decode_layers(append=True) on a freshly prefilled cache
of the tiny golden model -> the ordered names of the library entry points the prefill and the call go through (a spy on _lib.call), a SHA-256 over the raw bytes of what it
returns and, where the call writes or grows the cache, a SHA-256 over K[:, :, :length] and Vt[..., :length].  The names pin the routing; the hashes pin every
integer a launch is given - a wrong cache pitch or a wrong copy on growth leaves the names alone and moves the bits.  No tolerance: the kernels are
bit-stable from launch to launch (checked while recording: every route runs twice and must repeat itself exactly), so the comparison is equality.

AFK_DECODE_ROUTES_RECORD=<path of a json file>: record instead of compare (every case adds its entry to that file).  A difference after a change that was
meant to leave the cached forward alone is a failure of that change, not a reason to record again."""
import hashlib
import json
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

S0 = 40
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "decode_routes.json")
RECORD = os.environ.get("AFK_DECODE_ROUTES_RECORD")
_CTX = {}


def _model(dev):
    """the tiny golden model (hidden 256, 4:2 heads of 64, 2 layers: the geometry that takes the norm-in-prologue launches and a chain cap of 32), warmed by
    one prefill and one decode step so that no route's names depend on which case ran first"""
    if dev not in _CTX:
        from tests.test_sampler_gpu import _case_a

        m = _case_a(dev)[0]
        _decode(m, 1)
        _CTX[dev] = m
    return _CTX[dev]


def _batch(dev, B, n=S0):
    """B left-padded rows of n positions (row 0 full; B = 1: no mask), token ids below the <sound> id"""
    g = torch.Generator().manual_seed(100 + B)
    ids, att = torch.zeros((B, n), dtype=torch.long), torch.zeros((B, n), dtype=torch.long)
    for i in range(B):
        k = n - (i * 7) % 18
        ids[i, n - k:] = torch.randint(0, 256, (k,), generator=g)
        att[i, n - k:] = 1
    return ids.to(dev), (att.to(dev) if B > 1 else None)


def _prefill(m, B):
    """forward(use_cache=True) on the batch -> (the AfkKVCache, the argmax token of every row)"""
    ids, att = _batch(m.device_, B)
    out = m(input_ids=ids, attention_mask=att, use_cache=True, logits_to_keep=1)
    return out.past_key_values, out.logits[:, -1].float().argmax(-1)


def _decode(m, B):
    """one _decode_logits on a fresh cache -> (logits, None)"""
    c, nxt = _prefill(m, B)
    return m._decode_logits(m._new_state((c.K, c.Vt), c.lo, c.length, nxt)), None


def _lookup(m, M):
    """one _lookup_forward: M consecutive new positions of one sequence behind the prompt -> (logits, None)"""
    dev = m.device_
    c, nxt = _prefill(m, 1)
    head, emb = m.arena["lm_head.weight"].data, m.arena[m._lm + "embed_tokens.weight"].data
    ar = torch.arange(M, device=dev, dtype=torch.int32)
    rows = (nxt + 37 * ar.long()) % 256
    x = emb.index_select(0, rows).contiguous()
    pos = (c.length + ar).contiguous()
    krange = torch.stack([torch.zeros_like(ar), c.length + 1 + ar], -1).contiguous()
    start = torch.full((1,), c.length, device=dev, dtype=torch.int32)
    aws = m._decode_attn_workspace(dev, c.Vt.shape[4], M) if m._lookup_chain_ok(M, head) else None
    return m._lookup_forward(x, (c.K, c.Vt), pos, krange, start, aws, head), None


def _forward_fresh(m):
    ids, att = _batch(m.device_, 3)
    out = m(input_ids=ids, attention_mask=att, use_cache=True)
    return out.logits, out.past_key_values


def _forward_continue(m, n):
    c, nxt = _prefill(m, 3)
    new = (nxt[:, None] + 11 * torch.arange(n, device=m.device_)[None]) % 256
    out = m(input_ids=new, past_key_values=c)
    return out.logits, out.past_key_values


def _append(m, headroom):
    """a turn of 6 rows behind the cached prompt as generate(past_key_values=...) runs it: _continue_setup, then _decode_layers(append=True) -> (the hidden
    rows, the cache)"""
    from audio_flamingo_amd.modeling import AfkKVCache

    c, nxt = _prefill(m, 1)
    P, n = c.length, 6
    new = (nxt[:, None] + 11 * torch.arange(n, device=m.device_)[None]) % 256
    lo, Kc, Vt, pos_rows, krange = m._continue_setup(c, None, 1, P + n, headroom, "test")
    x = m._merged_embeddings(new.contiguous(), None, None)
    y = m._decode_layers(x, 1, n, P, (Kc, Vt), pos_rows, krange, False, append=True)
    return y, AfkKVCache(Kc, Vt, lo, P + n)


_TINY_GROUP = (2, 64)   # (Hq // Hkv, head_dim) of the tiny model: inside the append envelope only from 321 keys on
# route -> (the attributes set on the model for the case, the call)
ROUTES = {
    "chain_single": ({}, lambda m: _decode(m, 1)),
    "fused_glue": (dict(decode_chain=False), lambda m: _decode(m, 1)),
    "plain_decode_layers": (dict(decode_chain=False, decode_fused_glue=False), lambda m: _decode(m, 1)),
    "interval_kernel": (dict(decode_splits=0), lambda m: _decode(m, 1)),
    "batched_3_prologue": (dict(decode_norm_mode="prologue"), lambda m: _decode(m, 3)),
    "batched_3_producer": (dict(decode_norm_mode="producer"), lambda m: _decode(m, 3)),
    "batched_3_launch": (dict(decode_norm_mode="launch"), lambda m: _decode(m, 3)),
    "batched_9": ({}, lambda m: _decode(m, 9)),
    "batched_17": ({}, lambda m: _decode(m, 17)),
    "above_chain_cap": (dict(decode_chain_batch=0), lambda m: _decode(m, 3)),
    "lookup_4": ({}, lambda m: _lookup(m, 4)),
    "lookup_4_above_cap": (dict(decode_chain_batch=2), lambda m: _lookup(m, 4)),
    "forward_prefill_padded_3": ({}, _forward_fresh),
    "forward_continue_1": ({}, lambda m: _forward_continue(m, 1)),
    "forward_continue_5": ({}, lambda m: _forward_continue(m, 5)),
    "forward_continue_grow": (dict(cache_headroom=2), lambda m: _forward_continue(m, 5)),
    "append_grow": (dict(append_min_keys=0, append_envelope={_TINY_GROUP: (1, 1)}), lambda m: _append(m, 300)),
    "append_below_floor": (dict(append_min_keys=1 << 20, append_envelope={_TINY_GROUP: (1, 1)}), lambda m: _append(m, 8)),
}
# what a route must launch (and must not), whatever the recording says
EXPECT = {
    "chain_single": ("afk_decode_chain_qkv", "afk_decode_chain_qkv_batched"),
    "fused_glue": ("afk_decode_qkv_finish", "afk_decode_chain_qkv"),
    "plain_decode_layers": ("afk_attn_decode", "afk_decode_qkv_finish"),
    "interval_kernel": ("afk_xattn_fwd", "afk_attn_decode"),
    "batched_3_prologue": ("afk_decode_chain_qkv_norm_batched", "afk_decode_chain_qkv_batched"),
    "batched_3_producer": ("afk_decode_chain_linear_residual_norm_batched", "afk_decode_chain_qkv_norm_batched"),
    "batched_3_launch": ("afk_decode_chain_qkv_batched", "afk_decode_chain_qkv_norm_batched"),
    "batched_9": ("afk_decode_chain_qkv_batched", "afk_decode_chain_qkv_norm_batched"),
    "batched_17": ("afk_decode_chain_qkv_batched", "afk_decode_chain_qkv_norm_batched"),
    "above_chain_cap": ("afk_attn_decode", "afk_attn_decode_fused"),
    "lookup_4": ("afk_attn_decode_fused", "afk_xattn_fwd"),
    "lookup_4_above_cap": ("afk_xattn_fwd", "afk_attn_decode_fused"),
    "append_grow": ("afk_attn_append", "afk_xattn_fwd"),
    "append_below_floor": ("afk_xattn_fwd", "afk_attn_append"),
}


def _sha(*tensors):
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.detach().contiguous().cpu().view(torch.uint8).numpy().tobytes())
    return h.hexdigest()


def _run(m, route, monkeypatch):
    """the route under the spy -> (names, the returned tensor, the cache or None); the model's attributes are put back"""
    from audio_flamingo_amd import _lib

    attrs, call = ROUTES[route]
    names = []
    real = _lib.call
    with monkeypatch.context() as mp:
        for k, v in attrs.items():
            mp.setattr(m, k, {**m.append_envelope, **v} if k == "append_envelope" else v)   # the envelope gains an entry, it loses none
        mp.setattr(_lib, "call", lambda name, *a: (names.append(name), real(name, *a))[1])
        out, cache = call(m)
    return names, out, cache


@pytest.mark.parametrize("route", list(ROUTES))
def test_route_enqueues_and_returns_what_was_recorded(dev, route, monkeypatch):
    m = _model(dev)
    names, out, cache = _run(m, route, monkeypatch)
    assert all(isinstance(n, str) for n in names) and names
    if route in EXPECT:
        assert EXPECT[route][0] in names and EXPECT[route][1] not in names, (route, sorted(set(names)))
    got = {"out": _sha(out)}
    if cache is not None:
        n = cache.length
        assert cache.K.shape[2] >= n and cache.Vt.shape[4] == -(-cache.K.shape[2] // 64) * 64
        got["cache"] = _sha(cache.K[:, :, :n], cache.Vt[..., :n])
    if RECORD:   # the file: {"names": the entry points seen so far, "routes": {route: {"calls": indices into names, "out": sha256, "cache": sha256}}}
        names2, out2, cache2 = _run(m, route, monkeypatch)
        assert names2 == names and torch.equal(out, out2), f"{route} does not repeat itself: names and argmax ids only"
        if cache is not None:
            assert torch.equal(cache.K[:, :, :n], cache2.K[:, :, :n]) and torch.equal(cache.Vt[..., :n], cache2.Vt[..., :n]), route
        book = {"names": [], "routes": {}}
        if os.path.exists(RECORD):
            with open(RECORD) as f:
                book = json.load(f)
        book["names"] += sorted(set(names) - set(book["names"]))
        index = {n: i for i, n in enumerate(book["names"])}
        book["routes"][route] = {"calls": [index[n] for n in names], **got}
        os.makedirs(os.path.dirname(os.path.abspath(RECORD)), exist_ok=True)
        with open(RECORD, "w") as f:
            json.dump(book, f, separators=(",", ":"), sort_keys=True)
        return
    with open(FIXTURE) as f:
        book = json.load(f)
    want = book["routes"][route]
    calls = [book["names"][i] for i in want["calls"]]
    diff = next((i for i, (a, b) in enumerate(zip(names, calls)) if a != b), min(len(names), len(calls)))
    assert names == calls, (route, f"{len(names)} calls against {len(calls)} recorded; first difference at {diff}",
                            names[max(diff - 3, 0): diff + 3], calls[max(diff - 3, 0): diff + 3])
    assert got["out"] == want["out"], (route, "the returned bits are not the recorded ones")
    assert got.get("cache") == want.get("cache"), (route, "the cache bits are not the recorded ones")


@pytest.mark.skipif(bool(RECORD), reason="recording")
def test_recording_holds_every_route():
    with open(FIXTURE) as f:
        book = json.load(f)
    assert set(book["routes"]) == set(ROUTES)
    assert all(("cache" in book["routes"][r]) == (r.startswith(("forward_", "append_"))) for r in ROUTES)

"""generate()'s shared prompt cache: share_prompt= / AFK_SHARE_PROMPT.  The n continuations of one prompt row - sampled copies (do_sample with
num_return_sequences = n) or the beams of a device beam search - keep ONE copy of the prompt's keys and values (the prefill's own cache, run once per prompt
row) and a short tail cache of their own generated positions; a decode step attends to both through afk_attn_decode_shared (csrc/attention_shared.hip; the
contract is in include/afk.h).  docs/generate.md, "Sharing the prompt".

  resolve(...)      pure, CPU-runnable: the keyword against the class attribute, with the refusals -> ShareSpec | None
  SharedPrompt      the record DecodeState.shared holds: the prompt cache, its key interval per row, the prompt length, n, the step's static buffers
  build(...)        the device state of one call: the tail cache, the intervals, the rotary offsets, the attention workspace
  materialize(...)  pure torch (CPU or device): the two caches laid out as the plain AfkKVCache of B0 * n rows a caller continues on
  stats(...)        what the call stored against what the expanded call would have"""
from __future__ import annotations

from dataclasses import dataclass
from typing import NamedTuple


class ShareSpec(NamedTuple):
    n: int        # continuations per prompt row
    beams: bool   # the continuations are beams (False: sampled copies)


def resolve(share_prompt=None, default=False, *, copies=1, num_beams=1, use_cache=True, exact_fp32=False, past=False, hooks=False, lookup=False,
            beam_device=True, geometry=True, assist=False):
    """share_prompt (None: `default`, the model's share_prompt_cache) -> ShareSpec, or None for today's route: the switch off, or nothing to share
    (one continuation per prompt row).  copies: num_return_sequences of a sampled call; num_beams > 1: the beams are the continuations.
    The combinations sharing does not run with - share_prompt=True: an AfkError naming them; None with the default on: None, silently:
      use_cache=False; AFK_EXACT_FP32=1 (exact_fp32); past_key_values= (past); logits_processor= / stopping_criteria= / streamer= (hooks); prompt-lookup
      decoding (lookup); assisted decoding (assist: assistant_model=); beams on the host loop (beam_device False: beam_on_device off or outside
      afk_beam_step's caps); a geometry or row count outside the batched decode chain or afk_attn_decode_shared's envelope (geometry False).
    Through generate() two of these never fire today, because an older refusal comes first and names the combination itself: a passed cache refuses
    num_return_sequences > 1 and num_beams > 1 ("generate(past_key_values=...) with ..."), and decode_lookup.resolve refuses do_sample and beams
    ("generate(prompt_lookup_num_tokens=...) with ..."), so no call with something to share reaches this function with past or lookup set.  They are kept so
    that the rule stands in one place if either older refusal is ever lifted."""
    from ._lib import AfkError

    if share_prompt is not None and not isinstance(share_prompt, bool):
        raise ValueError(f"`share_prompt` has to be None, True or False, but is {share_prompt!r}")
    if not (bool(default) if share_prompt is None else share_prompt):
        return None
    beams = int(num_beams) > 1
    n = int(num_beams) if beams else int(copies)
    if n <= 1:
        return None
    bad = [what for on, what in ((not use_cache, "use_cache=False"), (bool(exact_fp32), "AFK_EXACT_FP32=1"), (bool(past), "past_key_values="),
                                 (bool(hooks), "logits_processor= / stopping_criteria= / streamer="), (bool(lookup), "prompt_lookup_num_tokens="),
                                 (bool(assist), "assistant_model="),
                                 (beams and not beam_device, "the host beam loop (beam_on_device off or outside afk_beam_step's caps)"),
                                 (not geometry, "a geometry or row count outside the batched decode chain or afk_attn_decode_shared's envelope")) if on]
    if bad:
        if share_prompt is None:
            return None
        raise AfkError(f"generate(share_prompt=True) with {' / '.join(bad)}: the prompt cache is shared between the sampled copies or device beams of a "
                       f"row on the KV cache and the batched decode chain only")
    return ShareSpec(n=n, beams=beams)


@dataclass
class SharedPrompt:
    """what a decode step on two caches reads besides DecodeState.cache (the TAIL cache, one row per continuation).  A record: no behaviour."""
    cache: tuple    # the prompt cache (Kp [L, B0, S0, nk], Vtp [L, B0, Hkv, D, pad64(S0)]): the prefill's own
    prange: object  # int32 [B0, 2] = [lo, S0): the prompt keys a row's continuations see
    S0: int         # prompt positions
    n: int          # continuations per prompt row
    pos0: object    # int32 [B0 * n] = S0 - lo: the rotary position of tail slot 0
    trange: object  # int32 [B0 * n, 2] = [0, cur + 1), written by every step (static memory)
    nsplit: int     # prompt key splits (ops.attn_shared_nsplit)
    ws: object      # the attention workspace


def build(spec, prompt_cache, lo, S0, max_new, Hq, Hkv, D):
    """the state of one call behind the prefill of B0 prompt rows into prompt_cache (no headroom): -> (SharedPrompt, the zeroed tail cache (Kt, Vtt) of
    B0 * n rows x max_new positions, lo repeated per continuation, rep [B0 * n]: each continuation's prompt row).  One-time setup in torch ops."""
    import torch

    from . import _lib, ops
    from ._lib import AfkError
    from .decode_forward import AfkKVCache

    Kp, Vtp = prompt_cache
    L, B0, dev, n = Kp.shape[0], Kp.shape[1], Kp.device, spec.n
    rep = torch.arange(B0, device=dev).repeat_interleave(n)
    lo_rep = lo.index_select(0, rep).contiguous()
    tail = AfkKVCache.allocate(L, B0 * n, int(max_new), Hkv, D, dev)
    ns = ops.attn_shared_nsplit(B0, n, Hq, Hkv, S0)
    ws = torch.empty(int(_lib.load().afk_attn_decode_shared_workspace_floats(B0, n, Hq, D, ns)), device=dev, dtype=torch.float32)
    prange = torch.stack([lo, torch.full_like(lo, int(S0))], -1).to(torch.int32).contiguous()
    shared = SharedPrompt(cache=prompt_cache, prange=prange, S0=int(S0), n=n, pos0=(int(S0) - lo_rep).to(torch.int32).contiguous(),
                          trange=torch.zeros((B0 * n, 2), device=dev, dtype=torch.int32), nsplit=ns, ws=ws)
    # checked ONCE: the decode loop hands these tensors' pointers and pitches to afk_attn_decode_shared itself, every layer of every step
    if not (Kp.is_contiguous() and Vtp.is_contiguous() and Kp.shape[2] == int(S0)):
        raise AfkError(f"decode_share.build: the prompt cache must be contiguous and hold exactly the {int(S0)} prompt positions, got K {tuple(Kp.shape)}")
    ops.attn_shared_check(Kp[0], Vtp[0], tail[0][0], tail[1][0], shared.prange, shared.trange, B0, n, Hkv, D)
    return shared, tail, lo_rep, rep


def materialize(Kp, Vtp, lo, S0, Kt, Vtt, n, length):
    """the two caches as ONE plain cache of B0 * n rows (torch copies; CPU or device tensors): row b0 * n + c holds the prompt positions [0, S0) of prompt row
    b0, then the tail positions of continuation b0 * n + c at S0 .. S0 + T - 1; lo repeated per continuation; `length` filled positions.
    Kp [L, B0, >= S0, nk], Vtp [L, B0, Hkv, D, >= S0], Kt [L, B0 * n, T, nk], Vtt [L, B0 * n, Hkv, D, >= T] -> AfkKVCache(K [L, B0 * n, S0 + T, nk],
    Vt [L, B0 * n, Hkv, D, pad64(S0 + T)], lo [B0 * n], length)"""
    import torch

    from .decode_forward import AfkKVCache
    from .ops import pad64

    S0, n, T = int(S0), int(n), Kt.shape[2]
    L, R, _, nk = Kt.shape
    K = torch.zeros((L, R, S0 + T, nk), device=Kt.device, dtype=Kt.dtype)
    Vt = torch.zeros(tuple(Vtt.shape[:4]) + (pad64(S0 + T),), device=Vtt.device, dtype=Vtt.dtype)
    K[:, :, :S0].copy_(Kp[:, :, :S0].repeat_interleave(n, dim=1))
    K[:, :, S0:].copy_(Kt)
    Vt[..., :S0].copy_(Vtp[..., :S0].repeat_interleave(n, dim=1))
    Vt[..., S0:S0 + T].copy_(Vtt[..., :T])
    return AfkKVCache(K, Vt, lo.repeat_interleave(n, dim=0), int(length))


def stats(shared, tail, max_new):
    """last_share_stats of a call: the rows and slots it stored, its cache bytes and those of the expanded call (B0 * n rows of S0 + max_new positions)"""
    from .ops import pad64

    Kp, Vtp = shared.cache
    Kt, Vtt = tail
    L, R, T, nk = Kt.shape
    nbytes = lambda *ts: sum(t.numel() * t.element_size() for t in ts)
    full = shared.S0 + int(max_new)
    return dict(prompt_rows=int(Kp.shape[1]), copies=int(shared.n), prompt_slots=int(shared.S0), tail_slots=int(T), cache_bytes=nbytes(Kp, Vtp, Kt, Vtt),
                unshared_cache_bytes=L * R * nk * (full + pad64(full)) * Kt.element_size())

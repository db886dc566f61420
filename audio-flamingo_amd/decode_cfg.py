"""generate()'s classifier-free guidance: guidance_scale= / negative_prompt_ids= / negative_prompt_attention_mask=
(UnbatchedClassifierFreeGuidanceLogitsProcessor, transformers/generation/logits_process.py:2224-2339; GenerationMixin._get_logits_processor builds it first,
utils.py:1132-1152).  Every prompt row gets a second, unconditional row - its own prompt (the negative prompt, text only), its own cache rows, the same
selected tokens - in the SAME decode step: one cache of 2 * B rows, one pass over the weights, and afk_decode_cfg (csrc/decode_cfg.hip; the contract is in
include/afk.h) folds the two logits rows of a pair in front of the processors.  docs/generate.md, "Classifier-free guidance".

  resolve(...)   pure, CPU-runnable: keyword against generation config, validation, every refusal -> CfgSpec | None
  layout(...)    pure: where the two prompts lie in the combined cache -> CfgLayout
  CfgState       the record DecodeState.cfg holds: the scale, the pair count, the kernel's workspace
  build(...)     the device state of one call behind the two prefills: the combined cache, lo per row, the CfgState
  materialize(...)  pure torch: the conditional rows as the plain AfkKVCache a caller continues on
  stats(...)     the numbers of last_cfg_stats"""
from __future__ import annotations

from dataclasses import dataclass
from typing import NamedTuple


class CfgSpec(NamedTuple):
    scale: float
    negative_ids: object    # int64 [B, Sn], or None: the last id of every prompt row
    negative_mask: object   # [B, Sn] (LEFT padding), or None


def resolve(guidance_scale=None, negative_prompt_ids=None, negative_prompt_attention_mask=None, generation_config=None, *, batch_size, audio_token_id=None,
            num_beams=1, use_cache=True, exact_fp32=False, lookup=False, past=False, share_prompt=None, assist=False):
    """guidance_scale (keyword; None: the generation config's, by the rule generate() picks its other arguments with) -> CfgSpec, or None where guidance is
    inactive: no scale, or a scale of 1 (the reference's gate, utils.py:1132) - negative_prompt_* are then ignored, silently, as the reference ignores them.
    Any other float is taken (0, below 1, negative: the reference builds the processor for them).
    ValueError: a scale that is no number; negative_prompt_ids that are not [batch_size, Sn >= 1] (both batch sizes named: the reference fails later, in a
    broadcast); a mask whose shape differs from the ids'.
    AfkError: a mask that is not LEFT padding; a negative prompt that holds the audio placeholder id (the unconditional branch has no audio: the reference
    calls model(input_ids, attention_mask) only); and the combinations guidance does not run with, each named: num_beams > 1, use_cache=False,
    AFK_EXACT_FP32=1, prompt-lookup decoding (lookup), assisted decoding (assist: assistant_model=), past_key_values= (past: the unconditional cache of
    the previous turn is not carried), share_prompt=True (None takes the unshared route)."""
    import torch

    from ._lib import AfkError

    gc = generation_config
    if guidance_scale is None and gc is not None:
        guidance_scale = getattr(gc, "guidance_scale", None)
    if guidance_scale is None:
        return None
    if isinstance(guidance_scale, bool) or not isinstance(guidance_scale, (int, float)):
        raise ValueError(f"`guidance_scale` has to be a number, but is {guidance_scale!r}")
    scale = float(guidance_scale)
    if scale == 1.0:
        return None
    bad = [what for on, what in ((int(num_beams) > 1, "num_beams > 1"), (not use_cache, "use_cache=False"), (bool(exact_fp32), "AFK_EXACT_FP32=1"),
                                 (bool(lookup), "prompt_lookup_num_tokens="), (bool(assist), "assistant_model="), (bool(past), "past_key_values="),
                                 (share_prompt is True, "share_prompt=True")) if on]
    if bad:
        raise AfkError(f"generate(guidance_scale={guidance_scale!r}) with {' / '.join(bad)}: classifier-free guidance runs with greedy or sampled decoding on a "
                       f"fresh KV cache of its own only (the unconditional rows are prefilled by this call)")
    ids, mask = negative_prompt_ids, negative_prompt_attention_mask
    if ids is None:
        return CfgSpec(scale, None, None)   # the reference ignores a mask without ids as well: its first pass builds ones_like(input_ids[:, -1:])
    if not torch.is_tensor(ids) or ids.dim() != 2 or ids.shape[1] < 1 or ids.is_floating_point():
        raise ValueError(f"`negative_prompt_ids` has to be an integer tensor [batch, length >= 1], but is "
                         f"{tuple(ids.shape) if torch.is_tensor(ids) else type(ids).__name__}")
    if ids.shape[0] != int(batch_size):
        raise ValueError(f"`negative_prompt_ids` holds {ids.shape[0]} rows, but `input_ids` holds {int(batch_size)}: one negative prompt per prompt row")
    if audio_token_id is not None and bool((ids == int(audio_token_id)).any()):
        raise AfkError(f"generate(negative_prompt_ids=...) holds the audio placeholder id {int(audio_token_id)}: the unconditional branch runs without audio (the "
                       f"reference calls model(input_ids, attention_mask) only) - pass the text of the prompt without its audio ids")
    if mask is not None:
        if not torch.is_tensor(mask) or tuple(mask.shape) != tuple(ids.shape):
            raise ValueError(f"`negative_prompt_attention_mask` {tuple(mask.shape) if torch.is_tensor(mask) else type(mask).__name__} has to have the shape of "
                             f"`negative_prompt_ids` {tuple(ids.shape)}")
        m = mask.bool()
        lens = m.sum(-1)
        if not bool((m == (torch.arange(ids.shape[1], device=m.device)[None] >= (ids.shape[1] - lens)[:, None])).all()) or not bool((lens > 0).all()):
            raise AfkError("generate(negative_prompt_attention_mask=...): attention masks with holes are not supported - only LEFT padding in front of at least one "
                           "real id per row (pad the negative prompt on the left)")
    return CfgSpec(scale, ids, mask)


class CfgLayout(NamedTuple):
    Smax: int          # the slot both prompts end in front of: max(S0, Sn); the first decode step appends there
    off_c: int         # slot of conditional position 0: Smax - S0
    off_u: int         # slot of unconditional position 0: Smax - Sn
    lo: object         # [2 * B]: first real slot of every cache row (rows [0, B) conditional, [B, 2B) unconditional)


def layout(S0, lo_c, Sn, lo_u):
    """the combined cache of a call: both prompts are aligned to the RIGHT at slot Smax = max(S0, Sn), so every row of a step writes the same slot `cur` (the
    batched decode chain appends all its rows at one slot) and a row's rotary position is cur - lo.  lo_c [B] / lo_u [B]: the first real position of every row
    inside its own prompt (left padding; tensors or sequences of ints) -> CfgLayout, lo = concat(lo_c + off_c, lo_u + off_u) of the inputs' kind (int32 for
    sequences)"""
    import torch

    S0, Sn = int(S0), int(Sn)
    Smax = max(S0, Sn)
    as_t = lambda v: v if torch.is_tensor(v) else torch.tensor(list(v), dtype=torch.int32)
    lo_c, lo_u = as_t(lo_c), as_t(lo_u)
    if lo_c.shape != lo_u.shape:
        raise ValueError(f"decode_cfg.layout: {lo_c.numel()} conditional rows against {lo_u.numel()} unconditional ones")
    return CfgLayout(Smax=Smax, off_c=Smax - S0, off_u=Smax - Sn, lo=torch.cat([lo_c + (Smax - S0), lo_u.to(lo_c.device) + (Smax - Sn)]).contiguous())


@dataclass
class CfgState:
    """what a guided decode step reads besides the DecodeState it hangs on (whose cache, lo and nxt have 2 * B rows).  A record: no behaviour."""
    scale: float
    B: int                  # pairs: the selection, the processors, the stop rule and the recorded rows are those of rows [0, B)
    ws: object              # afk_decode_cfg's workspace
    Smax: int = 0
    S0: int = 0
    Sn: int = 0


def build(scale, cond_cache, lo_c, S0, uncond_cache, lo_u, Sn, max_new, V):
    """behind the two prefills (B rows x S0 with the audio into cond_cache, B rows x Sn text only into uncond_cache, both with no headroom: the short negative
    prompt is never padded to the audio prompt's length inside the prefill GEMMs): -> (CfgState, the combined cache (K, Vt) of 2 * B rows x Smax + max_new
    positions, lo [2 * B]).  One-time setup in torch copies."""
    from . import ops
    from .decode_forward import AfkKVCache

    (Kc, Vc), (Ku, Vu) = cond_cache, uncond_cache
    L, B, nk = Kc.shape[0], Kc.shape[1], Kc.shape[3]
    Hkv, D = Vc.shape[2], Vc.shape[3]
    lay = layout(S0, lo_c, Sn, lo_u)
    K, Vt = AfkKVCache.allocate(L, 2 * B, lay.Smax + int(max_new), Hkv, D, Kc.device)
    K[:, :B, lay.off_c:lay.Smax].copy_(Kc[:, :, :S0])
    K[:, B:, lay.off_u:lay.Smax].copy_(Ku[:, :, :Sn])
    Vt[:, :B, :, :, lay.off_c:lay.Smax].copy_(Vc[..., :S0])
    Vt[:, B:, :, :, lay.off_u:lay.Smax].copy_(Vu[..., :Sn])
    st = CfgState(scale=float(scale), B=B, ws=ops.decode_cfg_workspace(B, V, Kc.device), Smax=lay.Smax, S0=int(S0), Sn=int(Sn))
    return st, (K, Vt), lay.lo.to(Kc.device, lo_c.dtype).contiguous()


def materialize(K, Vt, lo, cfg, length):
    """the B conditional rows of the combined cache (K [L, 2B, T, nk], Vt [L, 2B, Hkv, D, >= T], lo [2B]) as a plain cache of their own: slot Smax - S0 becomes
    slot 0, so the cache is the one the unguided call returns - lo as the prompt's mask says, `length` = S0 + generated - 1 filled positions.  Torch copies (CPU or
    device tensors), made only where the output object is asked for."""
    from .decode_forward import AfkKVCache
    from .ops import pad64

    B, off, T = cfg.B, cfg.Smax - cfg.S0, K.shape[2] - (cfg.Smax - cfg.S0)
    Kc = K[:, :B, off:].contiguous()
    Vc = Vt.new_zeros(tuple(Vt.shape[:1]) + (B,) + tuple(Vt.shape[2:4]) + (pad64(T),))
    Vc[..., :T].copy_(Vt[:, :B, :, :, off:off + T])
    return AfkKVCache(Kc, Vc, (lo[:B] - off).contiguous(), int(length))


def stats(cfg, cache):
    """last_cfg_stats of a call: the cache rows, the slots of the two prompts and the bytes of the combined cache (the unconditional rows own Smax + max_new
    slots although they use Sn + max_new: memory only, the decode attention reads [lo, cur])"""
    K, Vt = cache
    return dict(rows=int(K.shape[1]), prompt_slots=int(cfg.S0), negative_slots=int(cfg.Sn), cache_bytes=sum(t.numel() * t.element_size() for t in (K, Vt)))

"""generate()'s FP8 decode weights: decode_weights= / AFK_DECODE_WEIGHTS.  The single-sequence decode chain (decode_forward._chain_layers / _chain_lm_head:
one launch per Linear, csrc/decode_chain.hip) spends most of a token streaming bf16 weights it reads exactly once; with decode_weights="fp8" it streams a copy
of them in OCP e4m3fn with one power-of-two fp32 scale per output row - half the bytes.  Weights only: activations, accumulation, the rounding points, the KV
cache, the prefill and forward() stay what they are.  The copy is extra memory (the prefill GEMMs keep reading the bf16 weights), built on first use and rebuilt
whenever arena.version() has moved.  The quantisation rule is in csrc/decode_w8.hip (contract: include/afk.h; torch restatement: tests/_w8_ref.py).
docs/generate.md, "FP8 decode weights".  decode_weights_batched= / AFK_DECODE_WEIGHTS_BATCHED (default off) lets decode steps of 2 - 8 rows - the matrix-pipe
launches of decode_forward._decode_layers_chain_batched - read the same copy; "FP8 decode weights, 2 - 8 rows" there.

  resolve(...)        pure, CPU-runnable: the keyword against the class attribute, with the refusals -> True (the FP8 route) | False (today's route)
  Q8                  one quantised tensor: codes uint8 [N, K], scale fp32 [N]
  DecodeW8            the record DecodeState.w8 and the model hold: the decoder layers' four Linears, the lm_head, the arena version they were taken at
  quantize_rows(...)  one tensor through afk_quantize_rows_fp8 (raises on a NaN / infinite weight, naming the tensor)
  build(model)        the copy of a model's decoder Linears and lm_head
  stats(...)          the numbers of last_w8_stats"""
from __future__ import annotations

from dataclasses import dataclass
from typing import NamedTuple

VALUES = ("bf16", "fp8")
LAYER_KEYS = ("self_attn.qkv.weight", "self_attn.o_proj.weight", "mlp.gate_up.weight", "mlp.down_proj.weight")   # as the arena lays them out


def resolve(decode_weights=None, default="bf16", *, rows=1, num_beams=1, copies=1, guidance=False, lookup=False, share_prompt=None, use_cache=True,
            exact_fp32=False, chain_ok=True, widths_ok=True, head_ok=True, assist=False, batched=False, step_rows=None, batched_ok=True):
    """decode_weights (None: `default`, the model's decode_weight_dtype) -> True where the call decodes on the FP8 copy, False for today's route ("bf16").
    Anything but None, "bf16" or "fp8" (keyword or default) is a ValueError.  FP8 runs on the single-sequence chain only; the calls that do not run it -
    decode_weights="fp8": an AfkError naming the combination; None with the default on: False, silently (the share_prompt convention):
      more than one row after input expansion (rows); num_beams > 1; num_return_sequences > 1 (copies); active guidance_scale (guidance); prompt-lookup
      decoding (lookup); assisted decoding (assist: assistant_model=); share_prompt=True; use_cache=False; AFK_EXACT_FP32=1 (exact_fp32); a geometry
      outside the single-sequence chain (chain_ok False); hidden size, Hq * head_dim or intermediate size not a multiple of 16 (widths_ok False); lm_head
      rows not a multiple of 8 (head_ok False).
    batched (decode_weights_batched= / the class attribute / AFK_DECODE_WEIGHTS_BATCHED; off: nothing above changes): a call whose decode step has 2 - 8 rows -
    a batch of prompts, num_return_sequences copies, beams, an active guidance_scale, prompt-lookup decoding, share_prompt=True - decodes on the FP8 copy through
    the matrix-pipe launches of the batched chain (afk_decode_chain_*_batched_w8) -> True.  step_rows: the rows of a decode step (None: rows * num_beams, twice
    that under guidance; prompt-lookup decoding: k + 1).  Refused there, by name under the keyword and silently under the default: more than 8 rows in a step,
    assistant_model=, use_cache=False, AFK_EXACT_FP32=1, a step that does not run the norm-in-prologue launches (batched_ok False: decode_norm_mode, the row
    bounds decode_mfma_from .. decode_prologue_max, the geometry).  A call of one row keeps the rules above whatever `batched` says."""
    from ._lib import AfkError

    for what, v in (("decode_weights", decode_weights), ("decode_weight_dtype", default)):
        if v is not None and v not in VALUES:
            raise ValueError(f"`{what}` has to be None, 'bf16' or 'fp8', but is {v!r}")
    if (default if decode_weights is None else decode_weights) != "fp8":
        return False
    n = int(step_rows) if step_rows is not None else int(rows) * max(int(num_beams), 1) * (2 if guidance else 1)
    if batched and n >= 2:
        bad = [what for on, what in ((n > 8, f"{n} rows in a decode step (more than 8)"), (bool(assist), "assistant_model="), (not use_cache, "use_cache=False"),
                                     (bool(exact_fp32), "AFK_EXACT_FP32=1"),
                                     (not batched_ok and n <= 8, "a decode step outside the norm-in-prologue launches of the batched decode chain")) if on]
        if bad:
            if decode_weights is None:
                return False
            raise AfkError(f"generate(decode_weights='fp8', decode_weights_batched=True) with {' / '.join(bad)}: the batched FP8 launches take 2 - 8 rows "
                           f"of the matrix-pipe decode chain, on the KV cache")
        return True
    bad = [what for on, what in ((int(rows) > 1, "more than one row"), (int(num_beams) > 1, "num_beams > 1"), (int(copies) > 1, "num_return_sequences > 1"),
                                 (bool(guidance), "guidance_scale="), (bool(lookup), "prompt_lookup_num_tokens="), (bool(assist), "assistant_model="),
                                 (share_prompt is True, "share_prompt=True"), (not use_cache, "use_cache=False"), (bool(exact_fp32), "AFK_EXACT_FP32=1"),
                                 (not chain_ok, "a geometry outside the single-sequence decode chain"),
                                 (not widths_ok, "a hidden size, Hq * head_dim or intermediate size that is not a multiple of 16"),
                                 (not head_ok, "lm_head rows that are not a multiple of 8")) if on]
    if bad:
        if decode_weights is None:
            return False
        raise AfkError(f"generate(decode_weights='fp8') with {' / '.join(bad)}: the FP8 weights are read by the single-sequence decode chain only (one row, "
                       f"greedy or sampled, on the KV cache)")
    return True


class Q8(NamedTuple):
    codes: object   # uint8 [N, K]: OCP e4m3fn
    scale: object   # fp32 [N]


@dataclass
class DecodeW8:
    """the FP8 copy of a model's decode weights.  A record: no behaviour."""
    layers: list    # per decoder layer: {key of LAYER_KEYS: Q8}
    head: Q8        # lm_head.weight
    version: int    # arena.version() the copy was taken at
    bytes_fp8: int  # codes and scales
    bytes_bf16: int  # the bf16 tensors they restate


def quantize_rows(w, name="weight"):
    """bf16 [N, K] (row stride >= K) on the device -> Q8, by afk_quantize_rows_fp8: one launch and one host read of its NaN / infinity flag (one-time work)"""
    import torch

    from . import _lib, ops
    from ._lib import AfkError

    if w.dim() != 2 or w.dtype != torch.bfloat16 or w.stride(1) != 1 or not w.is_cuda:
        raise AfkError(f"decode_w8.quantize_rows({name}): a bf16 matrix with contiguous rows on the device, got {tuple(w.shape)} {w.dtype} strides {w.stride()}")
    N, K = w.shape
    codes = torch.empty((N, K), device=w.device, dtype=torch.uint8)
    scale = torch.empty((N,), device=w.device, dtype=torch.float32)
    bad = torch.zeros(1, device=w.device, dtype=torch.int32)
    _lib.call("afk_quantize_rows_fp8", w.data_ptr(), w.stride(0), N, K, codes.data_ptr(), codes.stride(0), scale.data_ptr(), bad.data_ptr(), ops._stream())
    if int(bad.item()):
        raise AfkError(f"decode_w8: {name} holds a NaN or infinite weight; it cannot be quantised to FP8")
    return Q8(codes, scale)


def build(model):
    """the FP8 copy of every decoder layer's qkv / o_proj / gate_up / down_proj weight and of lm_head.weight, as the arena holds them -> DecodeW8"""
    arena, nbytes = model.arena, lambda t: t.numel() * t.element_size()
    version, b8, b16 = arena.version(), 0, 0

    def one(key):
        nonlocal b8, b16
        w = arena[key].data
        q = quantize_rows(w, key)
        b8, b16 = b8 + nbytes(q.codes) + nbytes(q.scale), b16 + nbytes(w)
        return q

    layers = [{k: one(f"{model._lm}layers.{i}.{k}") for k in LAYER_KEYS} for i in range(model.dec_layers)]
    return DecodeW8(layers=layers, head=one("lm_head.weight"), version=version, bytes_fp8=b8, bytes_bf16=b16)


def stats(w8, rebuilt):
    """last_w8_stats of a call: the tensors of the copy, its bytes against the bf16 bytes it restates, and whether this call (re)built it"""
    return dict(tensors=len(w8.layers) * len(LAYER_KEYS) + 1, bytes_fp8=int(w8.bytes_fp8), bytes_bf16=int(w8.bytes_bf16), rebuilt=bool(rebuilt))

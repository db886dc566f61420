"""The cached decoder forward of the MI355X-native Audio Flamingo 3 model (generation.py drives it step by step; docs/generate.md tells the routes).

  AfkKVCache            the cache object: layout, allocation, growth, interop with the reference's DynamicCache
  CacheGeometry         the cache's layout as the kernels are told it: every pitch stated once, built once per forward
  AfkDecodeForwardMixin the decode knobs, the cache set-up, the four per-layer loops on the C ABI and the routing between them, inherited by
                        AudioFlamingo3ForConditionalGeneration"""
import os
from typing import NamedTuple

import torch

from . import _lib, ops
from . import decode_w8 as _w8mod
from ._lib import AfkError
from .generation import continuation_lengths, continuation_mask_check


class AfkKVCache:
    """KV cache handed between forward(use_cache=True) calls (the role of transformers' DynamicCache): per-layer post-RoPE keys
    K [L, B, Smax, Hkv*D], values stored transposed Vt [L, B, Hkv, D, pad64(Smax)] (the layout the decode attention kernels read), the
    number of filled positions and, for left-padded prompts, the first real position of every sample."""

    def __init__(self, K, Vt, lo, length):
        self.K, self.Vt, self.lo, self.length = K, Vt, lo, int(length)

    def get_seq_length(self, layer_idx: int = 0) -> int:
        return self.length

    @staticmethod
    def allocate(L, B, Smax, Hkv, D, device):
        """-> zeroed K [L, B, Smax, Hkv * D], Vt [L, B, Hkv, D, pad64(Smax)]"""
        return (torch.zeros((L, B, Smax, Hkv * D), device=device, dtype=torch.bfloat16),
                torch.zeros((L, B, Hkv, D, ops.pad64(Smax)), device=device, dtype=torch.bfloat16))

    def grown(self, Smax, P):
        """-> K, Vt reallocated to Smax positions, the first P kept (torch copies); this object keeps its own tensors - the caller decides who sees the new ones"""
        L, B = self.K.shape[:2]
        K, Vt = self.allocate(L, B, Smax, self.Vt.shape[2], self.Vt.shape[3], self.K.device)
        K[:, :, :P].copy_(self.K[:, :, :P])
        Vt[..., :P].copy_(self.Vt[..., :P])
        return K, Vt

    # ---- interop with the reference's cache object (TF/cache_utils.py DynamicCache; generation/utils.py:519-640 hands one to every forward)
    @staticmethod
    def is_reference_cache(obj) -> bool:
        return obj is not None and not isinstance(obj, AfkKVCache) and hasattr(obj, "layers") and hasattr(obj, "update") and hasattr(obj, "get_seq_length")

    @classmethod
    def adopt(cls, ref_cache, n_layers: int, Hkv: int, D: int, n_new: int, headroom: int, device, attention_mask=None):
        """the tensors of a reference DynamicCache (per layer: keys / values [B, Hkv, S, D], keys post-RoPE - Qwen2Attention.forward
        modeling_qwen2.py:213-214) re-laid into this cache: K [L, B, Smax, Hkv * D], values transposed Vt [L, B, Hkv, D, pad64(Smax)].  Left padding is
        read off the attention_mask of the call (which covers past + new positions, as the reference requires)."""
        start = int(ref_cache.get_seq_length())
        if start == 0:
            return None   # an EMPTY reference cache on the prefill call (`past_key_values=DynamicCache()`): nothing to adopt
        if len(ref_cache.layers) != n_layers:
            raise AfkError(f"forward(past_key_values=<reference cache>): it holds {len(ref_cache.layers)} layers, the decoder has {n_layers}")
        k0 = ref_cache.layers[0].keys
        B = k0.shape[0]
        if tuple(k0.shape[1:]) != (Hkv, start, D):
            raise AfkError(f"forward(past_key_values=<reference cache>): layer 0 keys are {tuple(k0.shape)}, expected [B, {Hkv}, {start}, {D}]")
        K, Vt = cls.allocate(n_layers, B, start + n_new + headroom, Hkv, D, device)
        for i, layer in enumerate(ref_cache.layers):
            K[i, :, :start].copy_(layer.keys.to(device, torch.bfloat16).permute(0, 2, 1, 3).reshape(B, start, Hkv * D))
            Vt[i, :, :, :, :start].copy_(layer.values.to(device, torch.bfloat16).permute(0, 1, 3, 2))
        lo = torch.zeros(B, device=device, dtype=torch.int32)
        if attention_mask is not None:
            am = attention_mask.to(device)
            if am.shape[1] >= start and not bool(am[:, :start].all()):
                lo = (start - am[:, :start].sum(-1)).to(torch.int32)   # left padding: leading zeros of the past part
        return cls(K, Vt, lo, start)

    def write_back(self, ref_cache, first: int, n: int, Hkv: int, D: int):
        """append positions [first, first + n) of every layer to the reference cache the caller handed in (DynamicCache.update), so that it stays the
        caller's single source of truth: the next call - to this model or to the reference - finds past + new in it"""
        L, B = self.K.shape[0], self.K.shape[1]
        for i in range(L):
            k = self.K[i, :, first: first + n].reshape(B, n, Hkv, D).permute(0, 2, 1, 3).contiguous()
            v = self.Vt[i, :, :, :, first: first + n].permute(0, 1, 3, 2).contiguous()
            ref_cache.update(k, v, i)
        return ref_cache


class CacheGeometry(NamedTuple):
    """What a per-layer loop tells the kernels about the cache and the model around it, built once per forward (CacheGeometry.of).  All pitches count bf16
    elements.  A wrong pitch is a silent read of the wrong cache: this is the one place that spells them.  An immutable record; a NamedTuple because an eager
    decode step builds one and a frozen dataclass costs three times as much to construct (profiles/decode_forward_move.md)."""
    K: torch.Tensor; Vt: torch.Tensor            # the cache: post-RoPE keys [L, B, Smax, nk], transposed values [L, B, Hkv, D, Spad]
    Hq: int; Hkv: int; D: int; H: int; L: int    # query heads, key heads, head size, hidden size, decoder layers
    nq: int; nk: int                             # Hq * D, Hkv * D: a query row, a key row
    Smax: int; Spad: int                         # positions K holds, positions Vt holds (pad64(Smax))
    cos: torch.Tensor; sin: torch.Tensor; stream: int; eps: float
    k_sample: int    # K sample pitch: from one sample's keys to the next sample's
    k_row: int       # K row pitch: from one position's key to the next position's
    vt_sample: int   # Vt sample pitch: from one sample's values to the next sample's
    vt_row: int      # Vt row pitch: from one value channel's positions to the next channel's
    # the batched chain's per-row pitches: rows are samples, so the sample pitches - or, one_sequence, consecutive positions of ONE sample:
    k_write: int     # row m's key is WRITTEN k_write behind row m - 1's (one_sequence: the next cache slot, k_row)
    vt_write: int    # the same for its values (one_sequence: the next cache slot, 1)
    k_read: int      # row m READS the keys k_read behind row m - 1's (one_sequence: 0 - the same cache, up to its own key-range end)
    vt_read: int     # the same for the values

    @classmethod
    def of(cls, model, cache, one_sequence=False):
        (K, Vt), Hq, Hkv, D = cache, model.Hq, model.Hkv, model.D
        Smax, Spad, nk = K.shape[2], Vt.shape[4], Hkv * D
        cos, sin = model._rope_tables(int(model.config.text_config.max_position_embeddings))
        k_sample, vt_sample = Smax * nk, Hkv * D * Spad
        wr, rd = ((nk, 1), (0, 0)) if one_sequence else ((k_sample, vt_sample), (k_sample, vt_sample))
        return cls(K=K, Vt=Vt, Hq=Hq, Hkv=Hkv, D=D, H=model.H, L=model.dec_layers, nq=Hq * D, nk=nk, Smax=Smax, Spad=Spad, eps=float(model.rms_eps), cos=cos, sin=sin,
                   stream=ops._stream(), k_sample=k_sample, k_row=nk, vt_sample=vt_sample, vt_row=Spad, k_write=wr[0], vt_write=wr[1], k_read=rd[0], vt_read=rd[1])

    def k(self, i):
        return self.K[i].data_ptr()

    def vt(self, i):
        return self.Vt[i].data_ptr()


class AfkDecodeForwardMixin:
    # ------------------------------------------------------------------ the decode knobs
    decode_chain = os.environ.get("AFK_DECODE_CHAIN", "1") == "1"   # single sequence: one launch per Linear (csrc/decode_chain.hip), five per layer
    decode_mfma_from = int(os.environ.get("AFK_DECODE_MFMA_FROM", "2"))   # batched decode: sequences per step from which the norm-in-prologue matrix-pipe launches run
    decode_chain_batch_max = int(os.environ.get("AFK_DECODE_CHAIN_BATCH_MAX", "32"))   # 9 .. 32 sequences: two / four groups of eight through the same launches (8 = the split-K tile path of rounds 3-5 above eight)
    decode_prologue_max = int(os.environ.get("AFK_DECODE_PROLOGUE_MAX", "8"))   # largest batch that takes the RMSNorm in the consumer's prologue (above: a norm launch + plain launches)
    decode_norm_mode = os.environ.get("AFK_DECODE_NORM", "prologue")   # batched decode, four sequences and more: "prologue" | "producer" | "launch" (_decode_layers_chain_batched)
    decode_chain_batch = int(os.environ.get("AFK_DECODE_CHAIN_BATCH", "8"))   # largest batch the one-launch-per-Linear kernels take (0: single sequence only)
    decode_weight_dtype = os.environ.get("AFK_DECODE_WEIGHTS", "bf16")   # generate(decode_weights=None): "bf16" | "fp8" - the single-sequence chain on the FP8 copy of its weights (decode_w8.py)
    decode_weights_batched = os.environ.get("AFK_DECODE_WEIGHTS_BATCHED", "0") == "1"   # generate(decode_weights_batched=None): with "fp8", steps of 2 - 8 rows (batches, copies, beams, guidance, lookup verification, a shared prompt) read the FP8 copy too (afk_decode_chain_*_batched_w8)
    _w8 = None   # the FP8 copy (decode_w8.DecodeW8): built by quantize_decode_weights() / the first fp8 call, None until then and after drop_decode_weights()
    last_w8_stats = None   # the last generate() call that decoded on the FP8 copy: decode_w8.stats; None after every other call
    decode_splits = 8  # key-range splits of the Q = 1 attention (0: use the interval MFMA kernel instead)
    decode_fused_glue = True  # B <= 4: one glue kernel per Linear (csrc/decode_glue.hip) instead of reduce / bias / rope / append / norm / SwiGLU launches
    cache_headroom = 256  # forward(use_cache=True): positions reserved beyond the prompt; the cache grows by doubling when they run out
    left_pad_on_lds_kernels = True  # left-padded batches on the LDS-staged causal kernels (kv_lo); False: interval kernels (A/B, tests)
    # _decode_layers(append=True) launches the append kernel only inside the envelope profiles/attn_append.md measured it to win in (by more than the spread):
    # (Hq / Hkv, head_dim) -> (fewest visible keys, most samples).  Below 264 keys the interval kernel wins at every geometry (32 .. 136 keys: 7 - 12 us against 15)
    append_envelope = {(7, 128): (264, 8), (1, 128): (264, 1), (2, 128): (264, 1), (4, 128): (264, 1), (8, 128): (264, 1), (2, 64): (321, 1)}
    append_min_keys = 0     # a floor on top of the envelope (A/B: tools/bench_attn_append.py sets it above every length)
    DECODE_CHUNK_KEYS = 4096   # keys one split of the Q = 1 attention holds (csrc/attention_decode.hip MAXCHUNK): it refuses spad > nsplit * 4096

    # ------------------------------------------------------------------ cache set-up
    @staticmethod
    def _pos_and_key_range(lo, start, n):
        """n new positions per row at cache offset `start`, rows whose first real position is lo [B]: the rotary positions [B * n] (position_ids =
        cumsum(mask) - 1) and the key range [lo, i + 1) of every query row [B, n, 2]"""
        B = lo.shape[0]
        ar = torch.arange(start, start + n, device=lo.device, dtype=torch.int32)
        pos_rows = (ar[None, :] - lo[:, None]).clamp_min(0).reshape(-1).contiguous()
        krange = torch.stack([lo[:, None].expand(B, n), torch.maximum(ar[None, :] + 1, lo[:, None])], -1).contiguous()
        return pos_rows, krange

    def _prefill_setup(self, attention_mask, B, n, headroom, who):
        """what a prefill of n prompt positions per row into a FRESH cache needs (`who` names the caller in the error): lo [B] (the first real position of
        every row: attention_mask may pad on the LEFT) and whether any row is padded, the zeroed cache Kc / Vt with `headroom` positions behind the prompt,
        the rotary positions, the key ranges, and whether the LDS-staged causal kernels take the prompt"""
        dev = self.device_
        lo, padded = torch.zeros(B, device=dev, dtype=torch.int32), False
        if attention_mask is not None:
            am = attention_mask.to(dev)
            if not bool(am.all()):
                lens = am.sum(-1)
                if not bool((am.flip(-1).cumsum(-1) == torch.minimum(torch.arange(1, n + 1, device=dev)[None], lens[:, None])).all()):
                    raise AfkError(f"{who}: only LEFT-padded attention_mask is supported (pad the prompt on the left)")
                lo, padded = (n - lens).to(torch.int32), True
        Kc, Vt = AfkKVCache.allocate(self.dec_layers, B, n + headroom, self.Hkv, self.D, dev)
        pos_rows, krange = self._pos_and_key_range(lo, 0, n)
        fast = self.D in (64, 128) and ops.ATTN_IMPL == "lds" and (self.left_pad_on_lds_kernels or not padded)
        return lo, padded, Kc, Vt, pos_rows, krange, fast

    def _continue_setup(self, cache, attention_mask, B, S_total, headroom, who):
        """what a prefill of the suffix [P, S_total) on an EXISTING cache needs (P = cache.length; `who` names the caller in the error): the cache grown by
        reallocation when S_total + headroom positions do not fit (once per turn: torch copies, as _forward_cached grows it) - `cache` is updated in place,
        K / Vt replaced - the attention_mask held against the left padding the cache records (generation.continuation_mask_check), the rotary positions and
        the key ranges of the suffix rows.  -> (lo, Kc, Vt, pos_rows, krange)"""
        dev = self.device_
        P = continuation_lengths(cache.length, S_total, who)
        if cache.K.shape[1] != B or cache.K.shape[0] != self.dec_layers or cache.K.shape[3] != self.Hkv * self.D:
            raise AfkError(f"{who}: past_key_values holds {cache.K.shape[0]} layers of {cache.K.shape[1]} rows x {cache.K.shape[3]} key columns; this call needs "
                           f"{self.dec_layers} layers of {B} rows x {self.Hkv * self.D}")
        lo = cache.lo.to(dev, torch.int32)
        if attention_mask is not None:
            continuation_mask_check(attention_mask.to(dev), lo, P, S_total, who)
        if S_total + headroom > cache.K.shape[2] or ops.pad64(S_total + headroom) > cache.Vt.shape[4]:
            cache.K, cache.Vt = cache.grown(S_total + headroom, P)
        cache.lo = lo
        pos_rows, krange = self._pos_and_key_range(lo, P, S_total - P)
        return lo, cache.K, cache.Vt, pos_rows, krange

    @torch.no_grad()
    def _forward_cached(self, input_ids, inputs_embeds, input_features, input_features_mask, attention_mask, past, logits_to_keep, position_ids=None):
        from .modeling import AF3Output   # modeling imports this module

        dev = self.device_
        if inputs_embeds is not None:
            B, n = inputs_embeds.shape[:2]
            x = inputs_embeds.to(dev, torch.bfloat16).reshape(B * n, self.H).contiguous()
            ids = None
        else:
            ids = input_ids.to(dev)
            B, n = ids.shape
        ref_cache = None
        if AfkKVCache.is_reference_cache(past):
            # the reference's cache object (GenerationMixin hands a DynamicCache to every forward, generation/utils.py:519-640): its tensors are adopted
            # into this implementation's layout for the call and the new positions are appended to it afterwards - the caller keeps ONE cache object
            ref_cache = past
            past = AfkKVCache.adopt(ref_cache, self.dec_layers, self.Hkv, self.D, n, self.cache_headroom, dev, attention_mask)
            if past is not None and attention_mask is not None:
                attention_mask = None    # consumed: the left padding is in past.lo, the new positions are all real
        if past is None:
            lo, padded, Kc, Vt, pos_rows, krange, fast = self._prefill_setup(attention_mask, B, n, self.cache_headroom, "forward(use_cache=True)")
            if ids is not None:
                x = self._merged_embeddings(ids, input_features, input_features_mask)
            start = 0
            kv_lo = lo if padded else None
        else:
            if not isinstance(past, AfkKVCache):
                raise AfkError("forward(past_key_values=...): pass the AfkKVCache a previous forward(use_cache=True) returned, or the reference's DynamicCache")
            if input_features is not None:
                raise AfkError("forward(past_key_values=...): audio belongs to the prefill call (the reference merges it there too)")
            Kc, Vt, lo, start = past.K, past.Vt, past.lo, past.length
            if start + n > Kc.shape[2]:   # out of reserved positions: double the cache
                Kc, Vt = past.grown(max(2 * Kc.shape[2], start + n + self.cache_headroom), start)
            if ids is not None:
                x = ops.embed_scatter_fwd(ids.reshape(-1).contiguous(), None, self.arena[self._lm + "embed_tokens.weight"].data, None)
            fast, kv_lo = False, None
            pos_rows, krange = self._pos_and_key_range(lo, start, n)
        if position_ids is not None:
            # the rotary positions the caller computed (GenerationMixin: cumsum(attention_mask) - 1 of the whole sequence, sliced to the new tokens)
            pos_rows = position_ids.to(dev).expand(B, n).to(torch.int32).clamp_min(0).reshape(-1).contiguous()
        elif ref_cache is not None:
            # a reference cache and no position_ids: the reference rotates by cache_position = arange(past, past + n) whatever the mask says
            # (Qwen2Model.forward modeling_qwen2.py:361-364) - the keys already in the cache (or the reference's next call on it) follow that convention
            pos_rows = torch.arange(start, start + n, device=dev, dtype=torch.int32)[None, :].expand(B, n).reshape(-1).contiguous()
        y = self._decode_layers(x, B, n, start, (Kc, Vt), pos_rows, krange, fast, kv_lo=kv_lo)
        keep = n if not logits_to_keep else min(int(logits_to_keep), n)
        rows = y.reshape(B, n, -1)[:, n - keep:, :].reshape(B * keep, -1).contiguous()
        logits = ops.gemm_nt(rows, self.arena["lm_head.weight"].data).reshape(B, keep, -1)
        new_cache = AfkKVCache(Kc, Vt, lo, start + n)
        if ref_cache is not None:
            return AF3Output(logits=logits, past_key_values=new_cache.write_back(ref_cache, start, n, self.Hkv, self.D))
        return AF3Output(logits=logits, past_key_values=new_cache)

    def _w(self, i, key):
        """a parameter of decoder layer i"""
        return self.arena[f"{self._lm}layers.{i}.{key}"].data

    def _next_norm_weight(self, i):
        """the norm behind layer i's down projection: the next layer's input norm, or the model's final norm"""
        return self._w(i + 1, "input_layernorm.weight") if i + 1 < self.dec_layers else self.arena[self._lm + "norm.weight"].data

    def _decode_nsplit(self, spad):
        """key splits of the Q = 1 attention over a cache of pitch spad: decode_splits, or more when decode_splits chunks of 4 096 keys do not cover the
        cache (the kernel refuses that - it used to drop the keys behind them).  The one-launch form merges the splits' partials in LDS: nsplit * (D + 2)
        <= 4096; a longer cache is refused here rather than read in part."""
        ns = max(self.decode_splits, -(-int(spad) // self.DECODE_CHUNK_KEYS))
        if ns * (self.D + 2) > 4096:
            raise AfkError(f"decode attention: a KV cache of {spad} positions needs {ns} key splits of at most {self.DECODE_CHUNK_KEYS}; the split merge holds "
                           f"at most {4096 // (self.D + 2)} at head_dim {self.D} (cache limit {4096 // (self.D + 2) * self.DECODE_CHUNK_KEYS} positions)")
        return ns

    def _decode_attn_workspace(self, dev, spad, B=1, counters=True):
        """partials + arrival counters of afk_attn_decode_fused for B sequences over a cache of pitch spad (as many splits as _decode_nsplit(spad)); the
        counters start at zero and every launch leaves them at zero.  counters=False: afk_attn_decode reads no counter - the same size, uninitialised"""
        n = _lib.load().afk_attn_decode_workspace_floats(B, self.Hq, self.D, self._decode_nsplit(spad))
        return (torch.zeros if counters else torch.empty)(n, device=dev, dtype=torch.float32)

    def _decode_attn_ws_check(self, aws, B, spad):
        """-> the split count of a decode step whose workspace was allocated earlier (a captured graph replays it): the workspace must hold that many"""
        ns = self._decode_nsplit(spad)
        need = _lib.load().afk_attn_decode_workspace_floats(B, self.Hq, self.D, ns)
        if aws.numel() < need:
            raise AfkError(f"decode attention: workspace of {aws.numel()} floats for {ns} splits over spad {spad} (needs {need}): allocate it for this cache")
        return ns

    def _decode_layers(self, x, B, n, start, cache, pos_rows, krange, fast_prefill, start_dev=None, kv_lo=None, append=False):
        """all decoder layers on n new positions per sample (rows [B*n, H]) at cache offset `start` (or *start_dev: graph replay).
        cache = (K [L, B, Smax, Hkv*D] post-RoPE keys, Vt [L, B, Hkv, D, Smaxpad] values stored transposed: the layout the interval
        attention kernels read directly).  Attention: prefill on the LDS-staged causal kernel (left-padded prompts: kv_lo); everything else
        (decode steps, other head sizes) on the interval kernel: query row i of sample b sees keys [krange[b,i,0], krange[b,i,1]);
        with start_dev the kernel is given the whole cache length and the interval alone bounds what is visible.
        append (generate(past_key_values=...): a turn's rows behind a long past): the last branch launches the split-KV append kernel (afk_attn_append)
        in place of the interval kernel where _append_routed says it wins; off (the default), every launch is what it was."""
        Hq, Hkv, D = self.Hq, self.Hkv, self.D
        append_ns, append_ws = 0, None
        if append and not fast_prefill and self._append_routed(B, n, start + n):
            append_ns = ops.attn_append_nsplit(B, Hq, Hkv, n, start + n)
            append_ws = torch.empty(int(_lib.load().afk_attn_append_workspace_floats(B, Hq, n, D, append_ns)), device=x.device, dtype=torch.float32)
        g, w = CacheGeometry.of(self, cache), self._w
        nq, Sk = g.nq, (g.Smax if start_dev is not None else start + n)
        for i in range(g.L):
            h, _ = ops.rmsnorm_fwd(x, w(i, "input_layernorm.weight"), g.eps)
            qkv = ops.gemm_nt(h, w(i, "self_attn.qkv.weight"), bias=w(i, "self_attn.qkv.bias"))
            ops.rope_(qkv, g.cos, g.sin, S=n, nheads=Hq + Hkv, D=D, pos=pos_rows)
            ld = qkv.stride(0)
            _lib.call("afk_kv_cache_append", qkv.data_ptr(), ld, nq, g.k(i), g.k_sample, g.vt(i), g.vt_sample, g.vt_row, ops._p(start_dev), int(start or 0), B, n, Hkv, D, g.stream)
            if fast_prefill:
                o, _ = ops.attn_fwd(qkv, B, n, Hq, Hkv, D, scale=D ** -0.5, causal=True, kv_lo=kv_lo)
            elif n == 1 and D in (64, 128) and self.decode_splits > 0:
                # one query row per sample: split-KV kernel (the cache is read once, nsplit blocks per head)
                o = torch.empty((B, nq), device=x.device, dtype=torch.bfloat16)
                ws = self._decode_attn_workspace(x.device, g.Spad, B, counters=False)
                _lib.call("afk_attn_decode", qkv.data_ptr(), qkv.stride(0), D, g.k(i), g.k_sample, g.k_row, D, g.vt(i), g.vt_sample, g.vt_row,
                          o.data_ptr(), nq, D, krange.data_ptr(), B, Hq, Hkv, D, float(D ** -0.5), self._decode_nsplit(g.Spad), ws.data_ptr(), g.stream)
            elif append_ns:
                o = ops.attn_append(qkv, g.K[i], g.Vt[i], krange, B, n, Hq, Hkv, D, D ** -0.5, nsplit=append_ns, ws=append_ws)
            else:
                o = torch.empty((B * n, nq), device=x.device, dtype=torch.bfloat16)
                lse = torch.empty((B, Hq, n), device=x.device, dtype=torch.float32)
                _lib.call("afk_xattn_fwd", qkv.data_ptr(), n * ld, D, ld, g.k(i), g.k_sample, D, g.k_row, g.vt(i), o.data_ptr(), n * nq, D, nq, lse.data_ptr(), 0,
                          krange.data_ptr(), B, Hq, Hkv, n, Sk, ops.pad64(n), g.Spad, D, float(D ** -0.5), g.stream)
            x2 = ops.gemm_nt(o, w(i, "self_attn.o_proj.weight"), residual=x)
            h2, _ = ops.rmsnorm_fwd(x2, w(i, "post_attention_layernorm.weight"), g.eps)
            gu = ops.gemm_nt(h2, w(i, "mlp.gate_up.weight"))
            x = ops.gemm_nt(ops.silu_mul_fwd(gu), w(i, "mlp.down_proj.weight"), residual=x2)
        y, _ = ops.rmsnorm_fwd(x, self.arena[self._lm + "norm.weight"].data, g.eps)
        return y

    def _append_routed(self, B, n, keys):
        """does a continuation of n rows per sample that sees up to `keys` keys go to afk_attn_append?  Only a geometry the kernel takes, a launch its
        grid holds (ceil(n / rows per tile) * Hkv <= 65 535) and a shape inside the measured envelope; everything else stays on afk_xattn_fwd."""
        if not ops.attn_append_supported(self.Hq, self.Hkv, self.D):
            return False
        G = self.Hq // self.Hkv
        if -(-n // (32 // G)) * self.Hkv > 65535 or B > 65535:
            return False
        min_keys, max_batch = self.append_envelope.get((G, self.D), (1 << 62, 0))
        return B <= max_batch and keys >= max(min_keys, self.append_min_keys)

    def _decode_layers_fused(self, x, B, cache, pos_rows, krange, start_dev):
        """one new position per sample, B <= ops.GEMV_MAX_M rows: every Linear = weight-streaming GEMV partials + ONE glue kernel"""
        g, w = CacheGeometry.of(self, cache), self._w
        Hq, Hkv, D, H, nq, eps, st, dev = g.Hq, g.Hkv, g.D, g.H, g.nq, g.eps, g.stream, x.device
        ns, aws = self._decode_nsplit(g.Spad), self._decode_attn_workspace(dev, g.Spad, B, counters=False)

        def gemv(inp, wt):
            N, K = wt.shape
            sp = ops.splitk_plan(B, N, K)
            ws = torch.empty(sp * B * N, device=dev, dtype=torch.float32)
            _lib.call("afk_gemv_partials", inp.data_ptr(), inp.stride(0), wt.data_ptr(), wt.stride(0), B, N, K, sp, ws.data_ptr(), st)
            return ws, sp

        h, _ = ops.rmsnorm_fwd(x, w(0, "input_layernorm.weight"), self.rms_eps)
        for i in range(g.L):
            ws, sp = gemv(h, w(i, "self_attn.qkv.weight"))
            q = torch.empty((B, nq), device=dev, dtype=torch.bfloat16)
            _lib.call("afk_decode_qkv_finish", ws.data_ptr(), sp, B, w(i, "self_attn.qkv.bias").data_ptr(), g.cos.data_ptr(), g.sin.data_ptr(),
                      pos_rows.data_ptr(), q.data_ptr(), g.k(i), g.k_sample, g.vt(i), g.vt_sample, g.vt_row, start_dev.data_ptr(), Hq, Hkv, D, st)
            o = torch.empty((B, nq), device=dev, dtype=torch.bfloat16)
            _lib.call("afk_attn_decode", q.data_ptr(), nq, D, g.k(i), g.k_sample, g.k_row, D, g.vt(i), g.vt_sample, g.vt_row,
                      o.data_ptr(), nq, D, krange.data_ptr(), B, Hq, Hkv, D, float(D ** -0.5), ns, aws.data_ptr(), st)
            ws, sp = gemv(o, w(i, "self_attn.o_proj.weight"))
            x2, h2 = torch.empty_like(x), torch.empty_like(x)
            _lib.call("afk_decode_residual_rmsnorm", ws.data_ptr(), sp, B, H, x.data_ptr(), w(i, "post_attention_layernorm.weight").data_ptr(), eps,
                      x2.data_ptr(), h2.data_ptr(), st)
            wgu = w(i, "mlp.gate_up.weight")
            ws, sp = gemv(h2, wgu)
            act = torch.empty((B, wgu.shape[0] // 2), device=dev, dtype=torch.bfloat16)
            _lib.call("afk_decode_swiglu", ws.data_ptr(), sp, B, wgu.shape[0] // 2, act.data_ptr(), st)
            ws, sp = gemv(act, w(i, "mlp.down_proj.weight"))
            x, h = torch.empty_like(x2), torch.empty_like(x2)
            _lib.call("afk_decode_residual_rmsnorm", ws.data_ptr(), sp, B, H, x2.data_ptr(), self._next_norm_weight(i).data_ptr(), eps, x.data_ptr(), h.data_ptr(), st)
        return h  # already through the final norm

    # ------------------------------------------------------------------ FP8 decode weights (decode_w8.py)
    def quantize_decode_weights(self):
        """build (or rebuild) the FP8 copy of the decoder Linears and the lm_head that generate(decode_weights="fp8") decodes on -> the decode_w8.DecodeW8 record
        (per layer a uint8 code tensor and an fp32 scale vector for qkv / o_proj / gate_up / down_proj, the same for lm_head.weight, and the arena.version() they
        were taken at).  Extra memory: the bf16 weights stay (the prefill and forward() read them)."""
        self._require_hip()
        self._w8 = _w8mod.build(self)
        return self._w8

    def drop_decode_weights(self):
        """free the FP8 copy (the next fp8 call builds it again)"""
        self._w8 = None

    def _w8_current(self):
        """the FP8 copy of the weights AS THEY ARE: built on first use, rebuilt whenever arena.version() has moved (load_state_dict, in-place torch writes, the
        optimizer's raw-pointer steps - the rule of the W^T shadows); leaves the call's last_w8_stats"""
        rebuilt = self._w8 is None or self._w8.version != self.arena.version()
        if rebuilt:
            self.quantize_decode_weights()
        self.last_w8_stats = _w8mod.stats(self._w8, rebuilt)
        return self._w8

    def _w8_resolve(self, decode_weights, rows, num_beams, copies, guidance, lookup, share_prompt, use_cache, exact_fp32, assist=False, batched=None, lookup_rows=None):
        """decode_w8.resolve with what only the model knows: the geometry, and (batched: the keyword, None: the class attribute decode_weights_batched) whether a
        step of that many rows runs the norm-in-prologue launches.  lookup_rows: the k + 1 rows of a prompt-lookup verify forward"""
        on = (self.decode_weight_dtype if decode_weights is None else decode_weights) == "fp8"
        chain_ok = widths_ok = head_ok = batched_ok = True
        step_rows = None
        if on:   # asked only where the answer is read: with the switch off the call reads no attribute it did not read before
            chain_ok = self._chain_ok(1)
            widths_ok = self.H % 16 == 0 and (self.Hq * self.D) % 16 == 0 and self.I % 16 == 0
            head = self.arena["lm_head.weight"].data
            head_ok = head.shape[0] % 8 == 0
            batched = bool(self.decode_weights_batched if batched is None else batched)
            if batched:
                step_rows = int(lookup_rows) if lookup else int(rows) * max(int(num_beams), 1) * (2 if guidance else 1)
                batched_ok = (self.decode_norm_mode == "prologue" and self.decode_mfma_from <= step_rows <= self.decode_prologue_max
                              and self._prologue_shapes_ok(head) and self._chain_batched_ok(step_rows, head))
        return _w8mod.resolve(decode_weights, self.decode_weight_dtype, rows=rows, num_beams=num_beams, copies=copies, guidance=guidance, lookup=lookup,
                              share_prompt=share_prompt, use_cache=use_cache, exact_fp32=exact_fp32, chain_ok=chain_ok, widths_ok=widths_ok, head_ok=head_ok, assist=assist,
                              batched=bool(on and batched), step_rows=step_rows, batched_ok=batched_ok)

    def _chain_layers(self, x, cache, pos_rows, krange, start_dev, aws=None, w8=None):
        """one new position of ONE sequence: five launches per decoder layer (round 4; ten on the split-K + glue path above).  Every Linear is one
        weight-streaming launch in which a group of waves owns eight complete output rows: the qkv launch normalises the residual stream in its prologue
        and applies bias / RoPE / cache append in its epilogue, o_proj and down_proj add the residual, gate|up normalises in its prologue and multiplies
        silu(gate) * up in its epilogue; the Q = 1 attention merges its key chunks in the last block to finish (afk_attn_decode_fused).  -> the residual row
        behind the last layer, NOT through the final RMSNorm (_chain_lm_head takes it in its prologue).
        w8 (a decode_w8.DecodeW8): the four Linears stream its FP8 codes and row scales (afk_decode_chain_*_w8) in place of the bf16 weights; nothing else differs"""
        g, w = CacheGeometry.of(self, cache), self._w
        if w8 is not None:
            return self._chain_layers_w8(g, x, pos_rows, krange, start_dev, aws, w8)
        Hq, Hkv, D, H, nq, eps, st, dev = g.Hq, g.Hkv, g.D, g.H, g.nq, g.eps, g.stream, x.device
        if aws is None:
            aws = self._decode_attn_workspace(dev, g.Spad)
        ns = self._decode_attn_ws_check(aws, 1, g.Spad)
        q = torch.empty((1, nq), device=dev, dtype=torch.bfloat16)
        o = torch.empty((1, nq), device=dev, dtype=torch.bfloat16)
        for i in range(g.L):
            wqkv = w(i, "self_attn.qkv.weight")
            _lib.call("afk_decode_chain_qkv", x.data_ptr(), w(i, "input_layernorm.weight").data_ptr(), eps, wqkv.data_ptr(), wqkv.stride(0), H,
                      w(i, "self_attn.qkv.bias").data_ptr(), g.cos.data_ptr(), g.sin.data_ptr(), pos_rows.data_ptr(), q.data_ptr(), g.k(i), g.vt(i), g.vt_row, start_dev.data_ptr(), Hq, Hkv, D, st)
            _lib.call("afk_attn_decode_fused", q.data_ptr(), nq, D, g.k(i), g.k_sample, g.k_row, D, g.vt(i), g.vt_sample, g.vt_row,
                      o.data_ptr(), nq, D, krange.data_ptr(), 1, Hq, Hkv, D, float(D ** -0.5), ns, aws.data_ptr(), st)
            wo = w(i, "self_attn.o_proj.weight")
            x2 = torch.empty_like(x)
            _lib.call("afk_decode_chain_linear_residual", o.data_ptr(), wo.data_ptr(), wo.stride(0), H, nq, x.data_ptr(), x2.data_ptr(), st)
            wgu = w(i, "mlp.gate_up.weight")
            I = wgu.shape[0] // 2
            act = torch.empty((1, I), device=dev, dtype=torch.bfloat16)
            _lib.call("afk_decode_chain_gate_up", x2.data_ptr(), w(i, "post_attention_layernorm.weight").data_ptr(), eps, wgu.data_ptr(), wgu.stride(0), I, H, act.data_ptr(), st)
            wd = w(i, "mlp.down_proj.weight")
            x = torch.empty_like(x2)
            _lib.call("afk_decode_chain_linear_residual", act.data_ptr(), wd.data_ptr(), wd.stride(0), H, I, x2.data_ptr(), x.data_ptr(), st)
        return x

    def _chain_layers_w8(self, g, x, pos_rows, krange, start_dev, aws, w8):
        """_chain_layers on the FP8 copy: the same five launches per layer, the Linears' weight pointer and pitch replaced by codes, pitch and row scales"""
        w = self._w
        Hq, Hkv, D, H, nq, eps, st, dev = g.Hq, g.Hkv, g.D, g.H, g.nq, g.eps, g.stream, x.device
        if aws is None:
            aws = self._decode_attn_workspace(dev, g.Spad)
        ns = self._decode_attn_ws_check(aws, 1, g.Spad)
        q = torch.empty((1, nq), device=dev, dtype=torch.bfloat16)
        o = torch.empty((1, nq), device=dev, dtype=torch.bfloat16)
        q8 = lambda t: (t.codes.data_ptr(), t.codes.stride(0), t.scale.data_ptr())
        for i in range(g.L):
            lw = w8.layers[i]
            _lib.call("afk_decode_chain_qkv_w8", x.data_ptr(), w(i, "input_layernorm.weight").data_ptr(), eps, *q8(lw["self_attn.qkv.weight"]), H,
                      w(i, "self_attn.qkv.bias").data_ptr(), g.cos.data_ptr(), g.sin.data_ptr(), pos_rows.data_ptr(), q.data_ptr(), g.k(i), g.vt(i), g.vt_row, start_dev.data_ptr(), Hq, Hkv, D, st)
            _lib.call("afk_attn_decode_fused", q.data_ptr(), nq, D, g.k(i), g.k_sample, g.k_row, D, g.vt(i), g.vt_sample, g.vt_row,
                      o.data_ptr(), nq, D, krange.data_ptr(), 1, Hq, Hkv, D, float(D ** -0.5), ns, aws.data_ptr(), st)
            x2 = torch.empty_like(x)
            _lib.call("afk_decode_chain_linear_residual_w8", o.data_ptr(), *q8(lw["self_attn.o_proj.weight"]), H, nq, x.data_ptr(), x2.data_ptr(), st)
            gu = lw["mlp.gate_up.weight"]
            I = gu.codes.shape[0] // 2
            act = torch.empty((1, I), device=dev, dtype=torch.bfloat16)
            _lib.call("afk_decode_chain_gate_up_w8", x2.data_ptr(), w(i, "post_attention_layernorm.weight").data_ptr(), eps, *q8(gu), I, H, act.data_ptr(), st)
            x = torch.empty_like(x2)
            _lib.call("afk_decode_chain_linear_residual_w8", act.data_ptr(), *q8(lw["mlp.down_proj.weight"]), H, I, x2.data_ptr(), x.data_ptr(), st)
        return x

    def _chain_lm_head(self, x, head, logits=None, part_val=None, part_idx=None, w8=None):
        """the final RMSNorm + lm_head (rows % 8 == 0) on the residual row of _chain_layers, one more launch of the same kind: it leaves the fp32 logits [1, V]
        and / or (max, argmax) per eight rows, whichever buffers are given.  w8: on the FP8 copy of the lm_head (afk_decode_chain_lm_head_w8)"""
        if w8 is not None:
            h8 = w8.head
            _lib.call("afk_decode_chain_lm_head_w8", x.data_ptr(), self.arena[self._lm + "norm.weight"].data.data_ptr(), float(self.rms_eps), h8.codes.data_ptr(),
                      h8.codes.stride(0), h8.scale.data_ptr(), h8.codes.shape[0], x.shape[1], ops._p(logits), ops._p(part_val), ops._p(part_idx), ops._stream())
            return
        _lib.call("afk_decode_chain_lm_head", x.data_ptr(), self.arena[self._lm + "norm.weight"].data.data_ptr(), float(self.rms_eps), head.data_ptr(), head.stride(0),
                  head.shape[0], x.shape[1], ops._p(logits), ops._p(part_val), ops._p(part_idx), ops._stream())

    def _decode_layers_chain(self, x, cache, pos_rows, krange, start_dev, aws=None, head=None, w8=None):
        """_chain_layers, then with `head` (lm_head weight, rows % 8 == 0) the fp32 logits [1, V] of _chain_lm_head; otherwise the normalised hidden row.
        w8: both on the FP8 copy (generate() resolved that the head has its rows % 8 == 0)"""
        x = self._chain_layers(x, cache, pos_rows, krange, start_dev, aws=aws, w8=w8)
        if head is not None:
            logits = torch.empty((1, head.shape[0]), device=x.device, dtype=torch.float32)
            self._chain_lm_head(x, head, logits=logits, w8=w8)
            return logits
        return ops.rmsnorm_fwd(x, self.arena[self._lm + "norm.weight"].data, self.rms_eps)[0]

    def _decode_layers_chain_batched(self, x, B, cache, pos_rows, krange, start_dev, aws, head, one_sequence=False, shared=None, w8=None):
        """one new position of 2 .. 32 sequences: the single-sequence chain with M input rows per launch (`afk_decode_chain_*_batched`: the weights are still
        read once per step).  Round 6: 2 .. 8 sequences take the RMSNorm in the prologue of the Linear that consumes it (5 launches per layer), 9 .. 32 run as
        groups of eight behind one norm launch per norm (7 per layer); geometries the matrix-pipe launches do not take keep rounds 4-5's form (7 launches per
        layer against ~12 on the split-K + glue path).  one_sequence: the B rows are CONSECUTIVE positions of the one sequence in the cache (the verify forward of
        prompt-lookup decoding): row m lands in slot *start_dev + m and every row reads the same cache (CacheGeometry's k_write .. vt_read).
        shared (a decode_share.SharedPrompt): `cache` is the TAIL cache of the B = B0 * n continuations - the qkv launch appends to it as it is told to - and
        the attention launch is afk_attn_decode_shared over the prompt cache (prompt keys shared.prange) and the tail (krange = [B, 2]: the tail keys);
        aws is its workspace.  Nothing else in the loop differs.
        w8 (a decode_w8.DecodeW8; generate() resolved 2 - 8 rows on the norm-in-prologue launches): the four Linears and the lm_head stream its FP8 codes and
        row scales (afk_decode_chain_*_batched_w8); the attention launch, the ss buffers and everything else are the same.  -> fp32 logits [B, V]"""
        g, w = CacheGeometry.of(self, cache, one_sequence=one_sequence), self._w
        if w8 is not None:
            return self._decode_layers_chain_batched_w8(g, x, B, pos_rows, krange, start_dev, aws, head, shared, w8)
        Hq, Hkv, D, H, nq, eps, st, dev = g.Hq, g.Hkv, g.D, g.H, g.nq, g.eps, g.stream, x.device
        ns = self._decode_attn_ws_check(aws, B, g.Spad) if shared is None else shared.nsplit
        cos, sin, pos, start = g.cos.data_ptr(), g.sin.data_ptr(), pos_rows.data_ptr(), start_dev.data_ptr()
        q = torch.empty((B, nq), device=dev, dtype=torch.bfloat16)
        o = torch.empty((B, nq), device=dev, dtype=torch.bfloat16)
        # round 6: from two sequences on (the matrix-pipe regime of the batched launches) up to eight, no RMSNorm is a launch of its own.  "prologue" (default): the norm in
        # front of qkv / gate|up / lm_head is taken in that Linear's own prologue (afk_decode_chain_*_norm_batched: every block derives the row statistic and
        # normalises the rows it consumes) - 5 launches per layer; "producer": the norm rides behind o_proj / down (afk_decode_chain_linear_residual_norm_batched:
        # the last block to arrive normalises; measured 8 / 5 us of hand-over per launch); "launch": afk_rmsnorm_fwd as in rounds 4-5 (7 launches per layer)
        shapes_ok = B >= self.decode_mfma_from and self._prologue_shapes_ok(head)
        mode = self.decode_norm_mode if shapes_ok else "launch"
        if mode == "prologue" and B > self.decode_prologue_max:
            mode = "launch"   # 9 .. 32 sequences: normalising 16 - 32 rows in EVERY block costs more VALU time than one norm launch (B = 12: 4.20 ms in the prologue, 3.99 with the launch; gate|up at 17 rows: 82 us)
        if mode == "producer":
            cnt = getattr(self, "_chain_norm_counter", None)
            if cnt is None or cnt.device != dev:
                cnt = self._chain_norm_counter = torch.zeros(1, device=dev, dtype=torch.int32)
        h = ssx = None
        ngrp = 1 if B <= 8 else 2 if B <= 16 else 4   # groups of eight sequences the norm-in-prologue launches run (include/afk.h)
        _p = lambda t: None if t is None else t.data_ptr()
        for i in range(g.L):
            wqkv, bias = w(i, "self_attn.qkv.weight"), w(i, "self_attn.qkv.bias").data_ptr()
            if mode == "prologue":   # ssx: the partial sums of squares the previous layer's down launch left for these rows (None: the first layer takes the statistic itself)
                _lib.call("afk_decode_chain_qkv_norm_batched", x.data_ptr(), x.stride(0), B, w(i, "input_layernorm.weight").data_ptr(), eps, wqkv.data_ptr(), wqkv.stride(0), H,
                          bias, cos, sin, pos, q.data_ptr(), nq, g.k(i), g.k_write, g.vt(i), g.vt_write, g.vt_row, start, Hq, Hkv, D, _p(ssx), H // 16, st)
            else:
                if h is None:
                    h, _ = ops.rmsnorm_fwd(x, w(i, "input_layernorm.weight"), eps)
                _lib.call("afk_decode_chain_qkv_batched", h.data_ptr(), h.stride(0), B, wqkv.data_ptr(), wqkv.stride(0), H, bias,
                          cos, sin, pos, q.data_ptr(), nq, g.k(i), g.k_write, g.vt(i), g.vt_write, g.vt_row, start, Hq, Hkv, D, st)
            if shared is None:
                _lib.call("afk_attn_decode_fused", q.data_ptr(), nq, D, g.k(i), g.k_read, g.k_row, D, g.vt(i), g.vt_read, g.vt_row,
                          o.data_ptr(), nq, D, krange.data_ptr(), B, Hq, Hkv, D, float(D ** -0.5), ns, aws.data_ptr(), st)
            else:
                # the caches and intervals were checked once (decode_share.build -> ops.attn_shared_check); the prompt cache is contiguous: its pitches are spelled here
                Kp, Vtp = shared.cache
                _lib.call("afk_attn_decode_shared", q.data_ptr(), nq, D, Kp[i].data_ptr(), shared.S0 * g.nk, g.nk, D, Vtp[i].data_ptr(), Hkv * D * Vtp.shape[4],
                          Vtp.shape[4], shared.S0, g.k(i), g.k_sample, g.k_row, D, g.vt(i), g.vt_sample, g.vt_row, g.Smax, o.data_ptr(), nq, D,
                          shared.prange.data_ptr(), krange.data_ptr(), B // shared.n, shared.n, Hq, Hkv, D, float(D ** -0.5), ns, aws.data_ptr(), aws.numel(), st)
            wo, norm2 = w(i, "self_attn.o_proj.weight"), w(i, "post_attention_layernorm.weight")
            x2, h2 = torch.empty_like(x), None
            if mode == "producer":
                h2 = torch.empty_like(x)
                _lib.call("afk_decode_chain_linear_residual_norm_batched", o.data_ptr(), nq, B, wo.data_ptr(), wo.stride(0), H, nq, x.data_ptr(), x.stride(0), x2.data_ptr(), H, norm2.data_ptr(), eps,
                          h2.data_ptr(), H, cnt.data_ptr(), st)
            elif mode == "prologue":
                ss2 = torch.empty((ngrp, 8, H // 16), device=dev, dtype=torch.float32)   # [groups of eight sequences the launch runs: 1, 2 or 4][8][blocks of the launch]
                _lib.call("afk_decode_chain_linear_residual_ss_batched", o.data_ptr(), nq, B, wo.data_ptr(), wo.stride(0), H, nq, x.data_ptr(), x.stride(0), x2.data_ptr(), H, ss2.data_ptr(), st)
            else:
                _lib.call("afk_decode_chain_linear_residual_batched", o.data_ptr(), nq, B, wo.data_ptr(), wo.stride(0), H, nq, x.data_ptr(), x.stride(0), x2.data_ptr(), H, st)
                h2, _ = ops.rmsnorm_fwd(x2, norm2, eps)
            wgu = w(i, "mlp.gate_up.weight")
            I = wgu.shape[0] // 2
            act = torch.empty((B, I), device=dev, dtype=torch.bfloat16)
            if mode == "prologue":
                _lib.call("afk_decode_chain_gate_up_norm_batched", x2.data_ptr(), x2.stride(0), B, norm2.data_ptr(), eps, wgu.data_ptr(), wgu.stride(0), I, H, act.data_ptr(), I,
                          ss2.data_ptr(), H // 16, st)
            else:
                _lib.call("afk_decode_chain_gate_up_batched", h2.data_ptr(), h2.stride(0), B, wgu.data_ptr(), wgu.stride(0), I, H, act.data_ptr(), I, st)
            wd = w(i, "mlp.down_proj.weight")
            x = torch.empty_like(x2)
            if mode == "producer":
                h = torch.empty_like(x2)
                _lib.call("afk_decode_chain_linear_residual_norm_batched", act.data_ptr(), I, B, wd.data_ptr(), wd.stride(0), H, I, x2.data_ptr(), H, x.data_ptr(), H,
                          self._next_norm_weight(i).data_ptr(), eps, h.data_ptr(), H, cnt.data_ptr(), st)
            elif mode == "prologue":
                ssx = torch.empty((ngrp, 8, H // 16), device=dev, dtype=torch.float32)
                _lib.call("afk_decode_chain_linear_residual_ss_batched", act.data_ptr(), I, B, wd.data_ptr(), wd.stride(0), H, I, x2.data_ptr(), H, x.data_ptr(), H, ssx.data_ptr(), st)
            else:
                _lib.call("afk_decode_chain_linear_residual_batched", act.data_ptr(), I, B, wd.data_ptr(), wd.stride(0), H, I, x2.data_ptr(), H, x.data_ptr(), H, st)
                h = None
        final = self.arena[self._lm + "norm.weight"].data
        logits = torch.empty((B, head.shape[0]), device=dev, dtype=torch.float32)
        if mode == "prologue":
            _lib.call("afk_decode_chain_lm_head_norm_batched", x.data_ptr(), x.stride(0), B, final.data_ptr(), eps, head.data_ptr(), head.stride(0), head.shape[0], H,
                      logits.data_ptr(), head.shape[0], _p(ssx), H // 16, st)
            return logits
        y = h if mode == "producer" else ops.rmsnorm_fwd(x, final, eps)[0]
        _lib.call("afk_decode_chain_lm_head_batched", y.data_ptr(), y.stride(0), B, head.data_ptr(), head.stride(0), head.shape[0], H, logits.data_ptr(), head.shape[0], st)
        return logits

    def _decode_layers_chain_batched_w8(self, g, x, B, pos_rows, krange, start_dev, aws, head, shared, w8):
        """the "prologue" form of _decode_layers_chain_batched on the FP8 copy: the same five launches per layer and the lm_head launch, the Linears' weight
        pointer and pitch replaced by codes, pitch and row scales"""
        w = self._w
        Hq, Hkv, D, H, nq, eps, st, dev = g.Hq, g.Hkv, g.D, g.H, g.nq, g.eps, g.stream, x.device
        if not (self.decode_norm_mode == "prologue" and self.decode_mfma_from <= B <= min(self.decode_prologue_max, 8) and self._prologue_shapes_ok(head)):
            raise AfkError(f"the FP8 batched decode chain takes the norm-in-prologue launches only (2 - 8 rows), not a step of {B} rows in mode {self.decode_norm_mode!r}")
        ns = self._decode_attn_ws_check(aws, B, g.Spad) if shared is None else shared.nsplit
        cos, sin, pos, start = g.cos.data_ptr(), g.sin.data_ptr(), pos_rows.data_ptr(), start_dev.data_ptr()
        q = torch.empty((B, nq), device=dev, dtype=torch.bfloat16)
        o = torch.empty((B, nq), device=dev, dtype=torch.bfloat16)
        q8 = lambda t: (t.codes.data_ptr(), t.codes.stride(0), t.scale.data_ptr())
        _p = lambda t: None if t is None else t.data_ptr()
        ssx = None
        for i in range(g.L):
            lw = w8.layers[i]
            _lib.call("afk_decode_chain_qkv_norm_batched_w8", x.data_ptr(), x.stride(0), B, w(i, "input_layernorm.weight").data_ptr(), eps, *q8(lw["self_attn.qkv.weight"]), H,
                      w(i, "self_attn.qkv.bias").data_ptr(), cos, sin, pos, q.data_ptr(), nq, g.k(i), g.k_write, g.vt(i), g.vt_write, g.vt_row, start, Hq, Hkv, D, _p(ssx), H // 16, st)
            if shared is None:
                _lib.call("afk_attn_decode_fused", q.data_ptr(), nq, D, g.k(i), g.k_read, g.k_row, D, g.vt(i), g.vt_read, g.vt_row,
                          o.data_ptr(), nq, D, krange.data_ptr(), B, Hq, Hkv, D, float(D ** -0.5), ns, aws.data_ptr(), st)
            else:
                Kp, Vtp = shared.cache
                _lib.call("afk_attn_decode_shared", q.data_ptr(), nq, D, Kp[i].data_ptr(), shared.S0 * g.nk, g.nk, D, Vtp[i].data_ptr(), Hkv * D * Vtp.shape[4],
                          Vtp.shape[4], shared.S0, g.k(i), g.k_sample, g.k_row, D, g.vt(i), g.vt_sample, g.vt_row, g.Smax, o.data_ptr(), nq, D,
                          shared.prange.data_ptr(), krange.data_ptr(), B // shared.n, shared.n, Hq, Hkv, D, float(D ** -0.5), ns, aws.data_ptr(), aws.numel(), st)
            x2 = torch.empty_like(x)
            ss2 = torch.empty((1, 8, H // 16), device=dev, dtype=torch.float32)
            _lib.call("afk_decode_chain_linear_residual_ss_batched_w8", o.data_ptr(), nq, B, *q8(lw["self_attn.o_proj.weight"]), H, nq, x.data_ptr(), x.stride(0), x2.data_ptr(), H,
                      ss2.data_ptr(), st)
            gu = lw["mlp.gate_up.weight"]
            I = gu.codes.shape[0] // 2
            act = torch.empty((B, I), device=dev, dtype=torch.bfloat16)
            _lib.call("afk_decode_chain_gate_up_norm_batched_w8", x2.data_ptr(), x2.stride(0), B, w(i, "post_attention_layernorm.weight").data_ptr(), eps, *q8(gu), I, H,
                      act.data_ptr(), I, ss2.data_ptr(), H // 16, st)
            x = torch.empty_like(x2)
            ssx = torch.empty((1, 8, H // 16), device=dev, dtype=torch.float32)
            _lib.call("afk_decode_chain_linear_residual_ss_batched_w8", act.data_ptr(), I, B, *q8(lw["mlp.down_proj.weight"]), H, I, x2.data_ptr(), H, x.data_ptr(), H,
                      ssx.data_ptr(), st)
        h8 = w8.head
        logits = torch.empty((B, h8.codes.shape[0]), device=dev, dtype=torch.float32)
        _lib.call("afk_decode_chain_lm_head_norm_batched_w8", x.data_ptr(), x.stride(0), B, self.arena[self._lm + "norm.weight"].data.data_ptr(), eps, *q8(h8),
                  h8.codes.shape[0], H, logits.data_ptr(), h8.codes.shape[0], _p(ssx), H // 16, st)
        return logits

    # ------------------------------------------------------------------ which loop takes a step
    def _prologue_shapes_ok(self, head):
        """the norm-in-prologue matrix-pipe launches (afk_decode_chain_*_norm_batched / _linear_residual_ss_batched) take this geometry"""
        H, nq, nk = self.H, self.Hq * self.D, self.Hkv * self.D
        return (H % 64 == 0 and H <= 4096 and nq % 64 == 0 and self.I % 64 == 0 and (self.D // 2) % 16 == 0 and nk % 32 == 0 and head.shape[0] % 32 == 0)

    def _chain_batch_cap(self, head):
        """largest batch of the one-launch-per-Linear decode step: 8 sequences, or (round 6) 32 = four groups of eight where the norm-in-prologue launches apply"""
        cap = min(self.decode_chain_batch, 8)
        if cap == 8 and self.decode_norm_mode == "prologue" and self.decode_chain_batch_max > 8 and self._prologue_shapes_ok(head):
            cap = min(self.decode_chain_batch_max, 32)
        return cap

    def _chain_ok(self, B):
        """single-sequence decode on csrc/decode_chain.hip: one launch per Linear (head sizes of the decode attention kernel, 16-byte rows)"""
        return (self.decode_chain and B == 1 and self.D in (64, 128) and self.decode_splits > 0 and self.H % 8 == 0
                and self.decode_splits * (self.D + 2) <= 4096)

    def _chain_batched_ok(self, B, head):
        """B rows - sequences of a decode step, or the positions of a prompt-lookup verify forward - take the one-launch-per-Linear batched chain"""
        return self._chain_ok(1) and 2 <= B <= self._chain_batch_cap(head) and head.shape[0] % 8 == 0 and self.I % 4 == 0

    _lookup_chain_ok = _chain_batched_ok   # (M, head): the name generate()'s prompt-lookup route asks by

    def _decode_logits(self, st):
        """logits [B, V] (fp32) of the position after st.nxt (a generation.DecodeState): one pass over the decoder weights, cache append at st.cur (not advanced here)"""
        B = st.nxt.shape[0]
        x = st.emb.index_select(0, st.nxt)
        if st.shared is not None:
            # a shared prompt cache (decode_share.py): st.cache is the tail cache and st.cur its slot, from 0 - the new position is S0 - lo + cur, the visible
            # tail keys are [0, cur + 1).  Only the batched chain has the route (generate() resolved that before the prefill)
            sh = st.shared
            sh.trange[:, 1:].copy_((st.cur + 1).expand(B, 1))
            return self._decode_layers_chain_batched(x.contiguous(), B, st.cache, sh.pos0 + st.cur, sh.trange, st.cur, sh.ws, st.head, shared=sh, w8=st.w8)
        if st.single is not None:   # single sequence (generate()): views of the step-state tensor, advanced by ONE add per step
            pos1, kr1 = st.single.pos1, st.single.kr1
        else:
            pos1 = (st.cur - st.lo).contiguous()
            kr1 = torch.stack([st.lo, (st.cur + 1).expand(B)], -1).reshape(B, 1, 2).contiguous()
        if self._chain_batched_ok(B, st.head):
            if st.aws is None:
                st.aws = self._decode_attn_workspace(x.device, st.cache[1].shape[4], B)
            return self._decode_layers_chain_batched(x.contiguous(), B, st.cache, pos1, kr1, st.cur, st.aws, st.head, w8=st.w8)
        if self._chain_ok(B):
            if st.aws is None:
                st.aws = self._decode_attn_workspace(x.device, st.cache[1].shape[4])
            head = st.head if st.head.shape[0] % 8 == 0 else None
            y = self._decode_layers_chain(x.contiguous(), st.cache, pos1, kr1, st.cur, aws=st.aws, head=head, w8=st.w8)
            if head is not None:
                return y
        elif self.decode_fused_glue and B <= ops.GEMV_MAX_M and self.D in (64, 128) and self.decode_splits > 0 and ops.SPLITK:
            y = self._decode_layers_fused(x.contiguous(), B, st.cache, pos1, kr1, st.cur)
        else:
            y = self._decode_layers(x, B, 1, None, st.cache, pos1, kr1, False, start_dev=st.cur)
        return ops.gemm_nt(y, st.head).float()

    def _lookup_forward(self, x, cache, pos_rows, krange, start_dev, aws, head, w8=None):
        """the verify forward of prompt-lookup decoding: M = x.shape[0] consecutive new positions of ONE sequence (embedding rows x [M, H], rotary positions
        pos_rows [M], key ranges krange [M, 2] = [lo, end + j), cache slots *start_dev + j) in one pass over the decoder weights -> fp32 logits [M, V].  Up to
        _chain_batch_cap rows: the batched decode chain with its cache strides aliased onto the one sequence; above (or where the chain does not apply):
        _decode_layers on the interval kernel, then the lm_head GEMM.  w8: the chain on the FP8 copy (generate() resolved that the k + 1 rows take it)."""
        M = x.shape[0]
        if self._lookup_chain_ok(M, head):
            return self._decode_layers_chain_batched(x, M, cache, pos_rows, krange, start_dev, aws, head, one_sequence=True, w8=w8)
        y = self._decode_layers(x, 1, M, None, cache, pos_rows, krange.view(1, M, 2), False, start_dev=start_dev)
        return ops.gemm_nt(y, head).float()

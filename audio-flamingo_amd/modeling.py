"""MI355X-native Audio Flamingo 3 model with the surface of transformers' AudioFlamingo3ForConditionalGeneration.

Mirrors (same constructor config classes, same ``forward`` argument names, same ``state_dict`` keys, ``generate``):
    transformers/models/audioflamingo3/modeling_audioflamingo3.py:570-642 (ForConditionalGeneration)
    :448-562 (Model), :302-416 (Encoder), :419-439 (projector); transformers/models/qwen2/modeling_qwen2.py:321-402.
The arithmetic is entirely the hand-written gfx950 kernels of libafk.so (functional.py); this module only owns
the parameter layout (arena.py) and the order of the stages.  Parameters named as in the oracle are views into
fused arena blocks (q|k|v and gate|up are stored contiguously so that each is one GEMM), so
``load_state_dict`` from an oracle checkpoint and ``state_dict`` round-trip unchanged.

Deviations from the oracle surface (documented, not silent):
  * training forward with ``labels`` fuses lm_head + loss; ``output.logits`` is still there, as in the reference, but LAZY: the [B, S, V]
    tensor is built on first access from the DETACHED final hidden states under ``no_grad`` - it carries NO gradient (the reference's is in
    the graph: an auxiliary loss built on ``outputs.logits`` must use ``forward(return_logits=True)``, which builds the logits eagerly inside
    the step's autograd graph) and reading it after an optimizer step raises (the weights are no longer the ones of ``output.loss``); lm_head
    and the loss run only on the rows whose shifted label is not -100 (identical loss and gradients);
  * ``gradient_checkpointing_enable()`` = every layer recomputed, as in the reference; ``gradient_checkpointing_kwargs={"policy": "budget"}``
    opts into recomputing only what a memory budget requires;
  * greedy token selection on the device (``afk_decode_select_greedy``) ignores NaN logits (picks the largest finite one) where ``torch.argmax``
    returns the NaN's index: a model that produces NaNs decodes differently - by design, it keeps the graph-replayed step free of host checks;
  * ``AFK_EXACT_FP32=1`` routes the inference forward / greedy ``generate`` through the exact fp32 verification kernels (exact.py);
  * ``forward(use_cache=True)`` / ``forward(past_key_values=cache)``: the reference's cache protocol for inference (prefill returns an
    ``AfkKVCache``, later calls append one or several tokens); same kernels and cache layout as ``generate`` (decode_forward.py, inherited as
    ``AfkDecodeForwardMixin``: the cache, its layout, the per-layer decode loops and their routing);
  * ``generate`` (generation.py, inherited as ``AfkGenerationMixin``): prefill fills a KV cache, each new token is one HIP-graph replay; greedy, sampled
    or beam search, with the logits processors, the stopping rules and the output object decided by launches inside the replayed step - docs/generate.md
    tells every route and what is not built (constrained / assisted decoding);
  * ``attention_mask`` rows must be one contiguous run of ones (left padding - the reference processor's default -, right padding, or
    both); masks with holes raise.  Hidden states of padded positions are zeros-attended garbage in both implementations and are
    never compared.
"""
from __future__ import annotations

import os
from typing import Optional

import torch
from torch import nn

from . import _lib, ops
from ._lib import AfkError
from .arena import Arena
from .decode_forward import AfkDecodeForwardMixin, AfkKVCache  # noqa: F401  (AfkKVCache: importable from here, as before)
from . import functional as F_
from .generation import AfkGenerationMixin


class AF3Output:
    """The reference's ModelOutput surface (AudioFlamingo3CausalLMOutputWithPast, modeling_audioflamingo3.py:635-642): attribute, key, index and
    slice access, ``to_tuple()``, ``keys()`` / ``items()``.

    ``logits`` is ALWAYS available, as in the reference (which returns it whenever it returns a loss, :625-642) - but when ``labels`` were
    given the fused lm_head + loss path never built the [B, S, V] tensor, so it is materialised on FIRST ACCESS (one lm_head GEMM on the
    final hidden states the output keeps): a training loop that only reads ``out.loss`` / ``out[0]`` never pays for it, ``Trainer.evaluate``
    / ``compute_metrics`` (which read ``outputs[1:]``) get what they expect."""

    _FIELDS = ("loss", "logits", "past_key_values", "hidden_states", "attentions", "audio_hidden_states", "token_logprobs", "token_entropy")

    def __init__(self, loss=None, logits=None, past_key_values=None, hidden_states=None, attentions=None, audio_hidden_states=None, logits_fn=None,
                 token_logprobs=None, token_entropy=None):
        self.loss, self._logits, self._logits_fn = loss, logits, logits_fn
        # forward(labels=, return_token_logprobs=True): fp32 [B, S] aligned with labels (docs/token_logprobs.md); None when not asked for
        self.token_logprobs, self.token_entropy = token_logprobs, token_entropy
        self.past_key_values, self.hidden_states, self.attentions, self.audio_hidden_states = past_key_values, hidden_states, attentions, audio_hidden_states

    @property
    def logits(self):
        if self._logits is None and self._logits_fn is not None:
            self._logits, self._logits_fn = self._logits_fn(), None
        return self._logits

    @logits.setter
    def logits(self, v):
        self._logits, self._logits_fn = v, None

    @property
    def logits_materialized(self) -> bool:
        return self._logits is not None

    def _present(self, name):
        return (self._logits is not None or self._logits_fn is not None) if name == "logits" else getattr(self, name) is not None

    def keys(self):
        return [f for f in self._FIELDS if self._present(f)]

    def items(self):
        return [(f, getattr(self, f)) for f in self.keys()]

    def to_tuple(self):
        return tuple(getattr(self, f) for f in self.keys())

    def get(self, k, default=None):
        return getattr(self, k) if k in self._FIELDS and self._present(k) else default

    def __contains__(self, k):
        return k in self._FIELDS and self._present(k)

    def __getitem__(self, k):
        if isinstance(k, str):
            if k not in self._FIELDS:
                raise KeyError(k)
            return getattr(self, k)
        if isinstance(k, int):
            return getattr(self, self.keys()[k])   # out[0] is the loss: nothing else is touched (no logits materialisation)
        return self.to_tuple()[k]

    def __iter__(self):
        return iter(self.keys())

    def __len__(self):
        return len(self.keys())


class _Holder(nn.Module):
    """parameter container that reproduces the oracle's module tree (and therefore its state_dict keys)"""


def _attach(root: nn.Module, name: str, param: nn.Parameter):
    parts = name.split(".")
    m = root
    for p in parts[:-1]:
        if p not in m._modules:
            m.add_module(p, _Holder())
        m = m._modules[p]
    m.register_parameter(parts[-1], param)


class AudioFlamingo3ForConditionalGeneration(AfkGenerationMixin, AfkDecodeForwardMixin, nn.Module):
    """Drop-in for the oracle class of the same name (config = transformers.AudioFlamingo3Config or a duck-typed object)."""

    def __init__(self, config, device="cuda", init_seed: Optional[int] = 0):
        super().__init__()
        self.config = config
        ac, tc = config.audio_config, config.text_config
        self.device_ = torch.device(device)
        # NOTE: construction on "cpu" is allowed for host-side logic (layout, state_dict, DP bucketing tests);
        # every compute entry point raises AfkError for non-HIP tensors - there is no CPU arithmetic path.
        self.E, self.enc_heads, self.enc_ffn = ac.hidden_size, ac.num_attention_heads, ac.intermediate_size
        self.enc_layers, self.n_mels, self.max_pos = ac.num_hidden_layers, ac.num_mel_bins, ac.max_source_positions
        self.H, self.I, self.V = tc.hidden_size, tc.intermediate_size, tc.vocab_size
        self.Hq, self.Hkv = tc.num_attention_heads, tc.num_key_value_heads
        self.D = getattr(tc, "head_dim", None) or self.H // self.Hq
        self.dec_layers, self.rms_eps = tc.num_hidden_layers, tc.rms_norm_eps
        rp = getattr(tc, "rope_parameters", None) or {}
        self.rope_theta = float(rp.get("rope_theta", getattr(tc, "rope_theta", 10000.0)) if isinstance(rp, dict) else getattr(tc, "rope_theta", 10000.0))
        self.audio_token_id = config.audio_token_id
        self.check_placeholders = True
        for name, v in (("audio hidden", self.E), ("encoder ffn", self.enc_ffn), ("text hidden", self.H), ("intermediate", self.I),
                        ("vocab", self.V), ("3*n_mels", 3 * self.n_mels)):
            if v % 64:
                raise AfkError(f"{name} size {v} must be a multiple of 64 for the MFMA GEMM")
        if (self.E // self.enc_heads) not in (32, 64, 128) or self.D not in (32, 64, 128):
            raise AfkError("head_dim must be 32, 64 or 128")

        # ---------------- arena layout (forward order; one bucket per layer)
        a = Arena(self.device_)
        self.arena = a
        E, Fd, H, I, V = self.E, self.enc_ffn, self.H, self.I, self.V
        at, pj, lm = "model.audio_tower.", "model.multi_modal_projector.", "model.language_model."
        b = a.new_bucket("stem")
        a.add(at + "conv1.weight", (E, self.n_mels, 3), b, shadow="conv")
        a.add(at + "conv1.bias", (E,), b, decay=False)
        a.add(at + "conv2.weight", (E, E, 3), b, shadow="conv")
        a.add(at + "conv2.bias", (E,), b, decay=False)
        for i in range(self.enc_layers):
            p = f"{at}layers.{i}."
            b = a.new_bucket(f"enc{i}")
            a.add(p + "self_attn_layer_norm.weight", (E,), b, decay=False)
            a.add(p + "self_attn_layer_norm.bias", (E,), b, decay=False)
            a.add(p + "self_attn.qkv.weight", (3 * E, E), b, shadow="T")
            a.add(p + "self_attn.qkv.bias", (3 * E,), b, decay=False)
            a.add(p + "self_attn.out_proj.weight", (E, E), b, shadow="T")
            a.add(p + "self_attn.out_proj.bias", (E,), b, decay=False)
            a.add(p + "final_layer_norm.weight", (E,), b, decay=False)
            a.add(p + "final_layer_norm.bias", (E,), b, decay=False)
            a.add(p + "fc1.weight", (Fd, E), b, shadow="T")
            a.add(p + "fc1.bias", (Fd,), b, decay=False)
            a.add(p + "fc2.weight", (E, Fd), b, shadow="T")
            a.add(p + "fc2.bias", (E,), b, decay=False)
        b = a.new_bucket("enc_out")
        a.add(at + "layer_norm.weight", (E,), b, decay=False)
        a.add(at + "layer_norm.bias", (E,), b, decay=False)
        a.add(pj + "linear_1.weight", (H, E), b, shadow="T")
        a.add(pj + "linear_1.bias", (H,), b, decay=False)
        a.add(pj + "linear_2.weight", (H, H), b, shadow="T")
        a.add(pj + "linear_2.bias", (H,), b, decay=False)
        b = a.new_bucket("embed")
        a.add(lm + "embed_tokens.weight", (V, H), b)
        nq, nkv = self.Hq * self.D, self.Hkv * self.D
        for i in range(self.dec_layers):
            p = f"{lm}layers.{i}."
            b = a.new_bucket(f"dec{i}")
            a.add(p + "input_layernorm.weight", (H,), b, decay=False)
            a.add(p + "self_attn.qkv.weight", (nq + 2 * nkv, H), b, shadow="T")
            a.add(p + "self_attn.qkv.bias", (nq + 2 * nkv,), b, decay=False)
            a.add(p + "self_attn.o_proj.weight", (H, nq), b, shadow="T")
            a.add(p + "post_attention_layernorm.weight", (H,), b, decay=False)
            a.add(p + "mlp.gate_up.weight", (2 * I, H), b, shadow="T")
            a.add(p + "mlp.down_proj.weight", (H, I), b, shadow="T")
        b = a.new_bucket("head")
        a.add(lm + "norm.weight", (H,), b, decay=False)
        a.add("lm_head.weight", (V, H), b, shadow="T")
        a.finalize()
        # weights whose dgrad reads W itself (functional.NN_DGRAD_SUFFIXES: the NN kernel) never need an eager W^T shadow: not allocated, not refreshed
        for blk in a.order:
            if blk.shadow_kind == "T" and F_.NN_DGRAD_SUFFIXES and blk.key.endswith(F_.NN_DGRAD_SUFFIXES):
                blk.shadow_lazy = True

        # ---------------- oracle-named parameters = views into the arena
        self._prm = {}
        def P(name, blk_key, rows=None):
            blk = a[blk_key]
            d, g = (blk.data, blk.grad) if rows is None else (blk.data[rows[0]: rows[1]], blk.grad[rows[0]: rows[1]])
            prm = nn.Parameter(d)
            prm.grad = g
            self._prm[name] = prm
            _attach(self, name, prm)

        for k in ("conv1.weight", "conv1.bias", "conv2.weight", "conv2.bias", "layer_norm.weight", "layer_norm.bias"):
            P(at + k, at + k)
        # frozen sinusoid table (requires_grad False in the oracle, :332) lives outside the arena
        pos_prm = nn.Parameter(torch.zeros((self.max_pos, E), device=self.device_, dtype=torch.bfloat16), requires_grad=False)
        _attach(self, at + "embed_positions.weight", pos_prm)
        self._prm[at + "embed_positions.weight"] = pos_prm
        a.extra_state.append(pos_prm.data)
        for i in range(self.enc_layers):
            p = f"{at}layers.{i}."
            P(p + "self_attn.q_proj.weight", p + "self_attn.qkv.weight", (0, E))
            P(p + "self_attn.k_proj.weight", p + "self_attn.qkv.weight", (E, 2 * E))
            P(p + "self_attn.v_proj.weight", p + "self_attn.qkv.weight", (2 * E, 3 * E))
            P(p + "self_attn.q_proj.bias", p + "self_attn.qkv.bias", (0, E))
            P(p + "self_attn.v_proj.bias", p + "self_attn.qkv.bias", (2 * E, 3 * E))
            for k in ("self_attn.out_proj.weight", "self_attn.out_proj.bias", "self_attn_layer_norm.weight", "self_attn_layer_norm.bias",
                      "fc1.weight", "fc1.bias", "fc2.weight", "fc2.bias", "final_layer_norm.weight", "final_layer_norm.bias"):
                P(p + k, p + k)
        for k in ("linear_1.weight", "linear_1.bias", "linear_2.weight", "linear_2.bias"):
            P(pj + k, pj + k)
        P(lm + "embed_tokens.weight", lm + "embed_tokens.weight")
        for i in range(self.dec_layers):
            p = f"{lm}layers.{i}."
            for nm, (s, e) in (("q_proj", (0, nq)), ("k_proj", (nq, nq + nkv)), ("v_proj", (nq + nkv, nq + 2 * nkv))):
                P(p + f"self_attn.{nm}.weight", p + "self_attn.qkv.weight", (s, e))
                P(p + f"self_attn.{nm}.bias", p + "self_attn.qkv.bias", (s, e))
            P(p + "self_attn.o_proj.weight", p + "self_attn.o_proj.weight")
            P(p + "mlp.gate_proj.weight", p + "mlp.gate_up.weight", (0, I))
            P(p + "mlp.up_proj.weight", p + "mlp.gate_up.weight", (I, 2 * I))
            P(p + "mlp.down_proj.weight", p + "mlp.down_proj.weight")
            P(p + "input_layernorm.weight", p + "input_layernorm.weight")
            P(p + "post_attention_layernorm.weight", p + "post_attention_layernorm.weight")
        P(lm + "norm.weight", lm + "norm.weight")
        P("lm_head.weight", "lm_head.weight")

        self._at, self._pj, self._lm = at, pj, lm
        self._rope_cache = {}
        self.gradient_checkpointing = False
        if init_seed is not None:
            self.init_weights(init_seed)
        self.training = True

    # ------------------------------------------------------------------ init (oracle _init_weights: N(0, initializer_range), norms 1/0, biases 0)
    @torch.no_grad()
    def init_weights(self, seed: int = 0):
        a = self.arena
        std = float(getattr(self.config.audio_config, "initializer_range", 0.02))
        a.init_normal_(std, seed)
        for blk in a.order:
            if blk.key.endswith("norm.weight"):
                blk.data.fill_(1.0)
            elif blk.key.endswith(".bias"):
                blk.data.zero_()
        g = torch.Generator(device=self.device_)
        g.manual_seed(seed + 1)
        self.embed_positions.data.copy_((torch.randn(self.embed_positions.shape, device=self.device_, generator=g) * std).to(torch.bfloat16))
        a.step_counter += 1

    def load_state_dict(self, sd, strict=True, assign=False):
        r = super().load_state_dict({k: v.to(torch.bfloat16) for k, v in sd.items()}, strict=strict)
        # the k-third of the fused encoder bias is not a parameter (k_proj has no bias): keep it zero
        E = self.E
        for i in range(self.enc_layers):
            self.arena[f"{self._at}layers.{i}.self_attn.qkv.bias"].data[E: 2 * E].zero_()
        self.arena.step_counter += 1  # invalidate W^T shadows
        return r

    def trainable_numel(self):
        return sum(b.numel for b in self.arena.order)

    # ------------------------------------------------------------------ small PreTrainedModel conveniences scripts rely on
    @property
    def device(self):
        return self.device_

    @property
    def dtype(self):
        return torch.bfloat16

    def num_parameters(self, only_trainable: bool = False, exclude_embeddings: bool = False) -> int:
        """PreTrainedModel.num_parameters (the HF Trainer calls it with exclude_embeddings=True for its FLOPs estimate)"""
        skip = {id(self._prm[self._lm + "embed_tokens.weight"]), id(self.embed_positions)} if exclude_embeddings else set()
        return sum(p.numel() for p in self.parameters() if (p.requires_grad or not only_trainable) and id(p) not in skip)

    def get_input_embeddings(self):
        """holder module whose `.weight` is the arena view of embed_tokens (the reference returns its nn.Embedding)"""
        return self.model.language_model.embed_tokens

    def get_output_embeddings(self):
        return self.lm_head

    # ------------------------------------------------------------------ checkpoints (PreTrainedModel.from_pretrained / save_pretrained surface)
    @classmethod
    def from_pretrained(cls, path, device="cuda", **kwargs):
        """Load a reference checkpoint directory (what AudioFlamingo3ForConditionalGeneration.save_pretrained writes / what
        `nvidia/audio-flamingo-3-hf` unpacks to): config.json + *.safetensors (single file or sharded with model.safetensors.index.json).
        The parameter names are the reference's, so the tensors drop straight into the arena views."""
        import json
        import os

        from safetensors import safe_open
        from transformers import AutoConfig

        config = AutoConfig.from_pretrained(path)
        model = cls(config, device=device, init_seed=None, **kwargs)
        idx = os.path.join(path, "model.safetensors.index.json")
        files = sorted(set(json.load(open(idx))["weight_map"].values())) if os.path.exists(idx) else ["model.safetensors"]
        sd = {}
        for fn in files:
            with safe_open(os.path.join(path, fn), framework="pt", device="cpu") as f:
                for k in f.keys():
                    sd[cls._runtime_key(k)] = f.get_tensor(k)
        model.load_state_dict(sd, strict=True)
        return model

    # checkpoint files use the hub layout; the reference renames on load (transformers/conversion_mapping.py "qwen2_audio":
    # ^language_model.model -> model.language_model, ^language_model.lm_head -> lm_head, ^audio_tower -> model.audio_tower,
    # ^multi_modal_projector -> model.multi_modal_projector) and reverses it on save
    _HUB_PREFIXES = (("language_model.model.model.", "model.language_model."), ("language_model.model.", "model.language_model."),
                     ("language_model.lm_head.", "lm_head."), ("audio_tower.", "model.audio_tower."),
                     ("multi_modal_projector.", "model.multi_modal_projector."))

    @classmethod
    def _runtime_key(cls, k: str) -> str:
        for src, dst in cls._HUB_PREFIXES:
            if k.startswith(src):
                return dst + k[len(src):]
        return k

    @classmethod
    def _hub_key(cls, k: str) -> str:
        for src, dst in cls._HUB_PREFIXES[1:]:
            if k.startswith(dst):
                return src + k[len(dst):]
        return k

    def save_pretrained(self, path, max_shard_size: int = 5 << 30):
        """config.json + safetensors shards with the reference's parameter names (loadable by the reference's from_pretrained)"""
        import json
        import os

        from safetensors.torch import save_file

        os.makedirs(path, exist_ok=True)
        self.config.save_pretrained(path)
        shards, cur, size = [], {}, 0
        for k, v in self.state_dict().items():
            t = v.detach().to("cpu").contiguous().clone()
            nb = t.numel() * t.element_size()
            if cur and size + nb > max_shard_size:
                shards.append(cur)
                cur, size = {}, 0
            cur[self._hub_key(k)] = t
            size += nb
        shards.append(cur)
        if len(shards) == 1:
            save_file(shards[0], os.path.join(path, "model.safetensors"), metadata={"format": "pt"})
            return
        wm = {}
        for i, sh in enumerate(shards):
            fn = f"model-{i + 1:05d}-of-{len(shards):05d}.safetensors"
            save_file(sh, os.path.join(path, fn), metadata={"format": "pt"})
            wm.update({k: fn for k in sh})
        json.dump({"metadata": {"total_size": sum(t.numel() * t.element_size() for sh in shards for t in sh.values())}, "weight_map": wm},
                  open(os.path.join(path, "model.safetensors.index.json"), "w"))

    # ------------------------------------------------------------------ helpers
    def _rope_tables(self, S: int):
        """Qwen2RotaryEmbedding.forward (modeling_qwen2.py:91-102): fp32 angles, cos/sin rounded to bf16"""
        if S not in self._rope_cache:
            D = self.D
            inv = 1.0 / (self.rope_theta ** (torch.arange(0, D, 2, device=self.device_, dtype=torch.float32) / D))
            fr = torch.arange(S, device=self.device_, dtype=torch.float32)[:, None] * inv[None, :]
            emb = torch.cat([fr, fr], dim=-1)
            self._rope_cache[S] = (emb.cos().to(torch.bfloat16).contiguous(), emb.sin().to(torch.bfloat16).contiguous())
        return self._rope_cache[S]

    # Activation checkpointing (oracle: GradientCheckpointingLayer.__call__, transformers/modeling_layers.py:79-114, switched on by
    # gradient_checkpointing_enable, modeling_utils.py:3187: EVERY transformer layer re-runs its forward in backward - the answer for 80 GB
    # parts).  gradient_checkpointing_enable() with no arguments means exactly that here too (policy "full", round 5 / ADVICE r04: a caller that
    # switches checkpointing on to FIT must get the reference's memory behaviour).  Opt-in (gradient_checkpointing_kwargs / env):
    #     policy = "budget" (env AFK_CKPT_POLICY)  recompute only what a memory budget requires: 288 GB of HBM3E hold the activations of a 5-minute clip
    #                                              outright (185 GiB), and a recomputed layer costs a third of its forward + backward time again
    #     memory_budget_gib = None                 -> CKPT_BUDGET_FRACTION of the device's memory (0.85 x 288 GiB = 245 GiB on MI355X); env AFK_CKPT_BUDGET_GIB
    # The budget plan - how many of the FIRST layers of each tower are recomputed (their recompute runs last in backward, when the later layers'
    # activations are already gone) - is made per forward from the batch geometry, what this process has allocated, what the DEVICE still has free
    # (hipMemGetInfo: other processes count) plus this process's own cached blocks, and the W^T shadows that will still be allocated lazily; gradients
    # are bit-identical whatever the plan (tests/test_model_gpu.py::test_gradient_checkpointing_matches).  Every new plan is logged.
    CKPT_BUDGET_FRACTION = 0.85

    def gradient_checkpointing_enable(self, gradient_checkpointing_kwargs=None):
        kw = dict(gradient_checkpointing_kwargs or {})
        self.gradient_checkpointing = True
        self.ckpt_policy = kw.get("policy", os.environ.get("AFK_CKPT_POLICY", "full"))
        b = kw.get("memory_budget_gib", os.environ.get("AFK_CKPT_BUDGET_GIB"))
        self.ckpt_budget_bytes = None if b is None else int(float(b) * 2 ** 30)
        if self.ckpt_policy not in ("budget", "full"):
            raise ValueError(f"gradient_checkpointing policy {self.ckpt_policy!r}: 'budget' or 'full'")

    def gradient_checkpointing_disable(self):
        self.gradient_checkpointing = False

    ckpt_policy, ckpt_budget_bytes, ckpt_plan, _ckpt_logged = "full", None, None, None

    def activation_bytes_per_layer(self, windows: int, dec_rows: int):
        """bytes one encoder layer / one decoder layer keeps for backward (functional.EncoderLayerFn / DecoderLayerFn.save_for_backward):
        encoder, per row of W x 1500: x, h, o, x2, h2 (E each), qkv (3E), fc1 pre-activation and GELU output (F each) + fp32 statistics;
        decoder, per token: x, h, o, x2, h2 (H), qkv ((Hq + 2 Hkv) D), gate|up (2 I), SwiGLU output (I) + fp32 lse per head and statistics"""
        ac, tc = self.config.audio_config, self.config.text_config
        E, Fi = ac.hidden_size, ac.intermediate_size
        enc = windows * self.max_pos * (2 * (8 * E + 2 * Fi) + 4 * (4 + self.enc_heads))
        H, I = tc.hidden_size, tc.intermediate_size
        dec = dec_rows * (2 * (5 * H + (self.Hq + 2 * self.Hkv) * self.D + 3 * I) + 4 * (2 + self.Hq))
        return enc, dec

    def plan_checkpointing(self, windows: int, dec_rows: int, allocated_bytes: int, total_bytes: int, usable_bytes: Optional[int] = None,
                           pending_bytes: int = 0):
        """-> {"enc": n, "dec": n, ...}: how many of the first layers of each tower are recomputed.  Pure host arithmetic (tested on the CPU).
        usable_bytes: what this process can still obtain (device-free memory + its own cached-but-unallocated blocks; None = unknown, trust the budget);
        pending_bytes: allocations that will happen later in the step outside the activations (W^T shadows created lazily by the first backward)."""
        enc_b, dec_b = self.activation_bytes_per_layer(windows, dec_rows)
        if self.ckpt_policy == "full":
            return {"enc": self.enc_layers if windows else 0, "dec": self.dec_layers, "policy": "full"}
        budget = self.ckpt_budget_bytes if self.ckpt_budget_bytes is not None else int(self.CKPT_BUDGET_FRACTION * total_bytes)
        # what backward needs on top of the kept activations: one layer being recomputed + one layer's worth of gradient temporaries in each tower
        # in flight (three streams), the lm_head logits chunk and its fp32 split-K partials, allocator slack
        V = self.config.text_config.vocab_size
        headroom = 2 * dec_b + 2 * enc_b + 3 * F_.LMHeadLossFn.CHUNK * V * 2 + (6 << 30)
        avail = budget - allocated_bytes
        if usable_bytes is not None:
            avail = min(avail, int(usable_bytes))
        avail -= headroom + int(pending_bytes)
        need = self.enc_layers * enc_b + self.dec_layers * dec_b
        n_dec = n_enc = 0
        if need > avail:
            n_dec = min(self.dec_layers, -(-(need - avail) // max(dec_b, 1))) if dec_b else 0
            need -= n_dec * dec_b
            if need > avail and enc_b:
                n_enc = min(self.enc_layers, -(-(need - avail) // enc_b))
        return {"enc": int(n_enc), "dec": int(n_dec), "policy": "budget", "budget_gib": round(budget / 2 ** 30, 1),
                "allocated_gib": round(allocated_bytes / 2 ** 30, 1), "usable_gib": None if usable_bytes is None else round(usable_bytes / 2 ** 30, 1),
                "pending_gib": round(pending_bytes / 2 ** 30, 2), "enc_layer_gib": round(enc_b / 2 ** 30, 3), "dec_layer_gib": round(dec_b / 2 ** 30, 3)}

    def _pending_shadow_bytes(self) -> int:
        """W^T / conv shadows that do not exist yet and will be allocated by the first backward that needs them"""
        return sum(2 * b.numel * (2 if b.shadow_kind == "conv" else 1) for b in self.arena.order if b.shadow_kind is not None and b.shadow is None)

    def _make_ckpt_plan(self, windows, dec_rows):
        if not (self.gradient_checkpointing and torch.is_grad_enabled()):
            self.ckpt_plan = None
            return
        free, total = torch.cuda.mem_get_info(self.device_)
        alloc, reserved = torch.cuda.memory_allocated(self.device_), torch.cuda.memory_reserved(self.device_)
        self.ckpt_plan = self.plan_checkpointing(windows, dec_rows, alloc, total, usable_bytes=free + max(reserved - alloc, 0),
                                                 pending_bytes=self._pending_shadow_bytes())
        key = (windows, dec_rows, self.ckpt_plan["enc"], self.ckpt_plan["dec"], self.ckpt_plan["policy"])
        if key != self._ckpt_logged:
            self._ckpt_logged = key
            import logging

            logging.getLogger("audio_flamingo_amd").info("activation checkpointing plan for %d windows / %d decoder rows: %s", windows, dec_rows, self.ckpt_plan)

    def _layer(self, fn, *args, ckpt=True):
        if ckpt and self.gradient_checkpointing and torch.is_grad_enabled():
            import contextlib

            from torch.utils.checkpoint import checkpoint

            # the second context manager wraps the RE-RUN of the layer inside backward: functional.py skips what only produces the (discarded) output there
            return checkpoint(fn, *args, use_reentrant=False, context_fn=lambda: (contextlib.nullcontext(), F_.recomputing()))
        return fn(*args)

    def _require_hip(self):
        if self.device_.type != "cuda" or not torch.cuda.is_available():
            raise AfkError("audio_flamingo_amd: forward needs a HIP device (MI355X); this package has no CPU arithmetic path")

    @property
    def embed_positions(self):
        return self._prm[self._at + "embed_positions.weight"]

    def _anchor(self, key):
        """a real nn.Parameter of the stage: makes the Function's output require grad (its own grad slot stays None)"""
        return self._prm[key]

    # ------------------------------------------------------------------ audio tower + projector (a2-a9)
    def _post_encoder(self, x, W, T3, n_tok, input_ids):
        """hook between the audio tower and the projector (identity for AF3; Music Flamingo rotates by time here)"""
        return x

    def get_audio_features(self, input_features, input_features_mask=None, input_ids=None):
        """-> (audio_rows [W*T3, H] (all rows, padded windows included), tokens_per_window int64[W] or None)"""
        self._require_hip()
        a, at = self.arena, self._at
        feats = input_features.contiguous()
        if not feats.is_cuda:
            raise AfkError("input_features must be on the HIP device")
        if feats.dtype not in (torch.float32, torch.bfloat16):
            feats = feats.float()
        W, C, T = feats.shape
        T2 = (T - 1) // 2 + 1
        if T2 != self.max_pos:
            raise AfkError(f"input_features must have {2 * self.max_pos} frames (got {T}); embed_positions add requires it (:385)")
        kv_len, n_tok = None, None
        if input_features_mask is not None:
            L0 = input_features_mask.to(self.device_).sum(-1).to(torch.int64)
            L1 = (L0 - 1) // 2 + 1
            n_tok = (L1 - 2) // 2 + 1
            kv_len = L1.to(torch.int32).contiguous()
        x = F_.ConvStemFn.apply(feats, self._anchor(at + "conv1.weight"), a,
                                (at + "conv1.weight", at + "conv1.bias", at + "conv2.weight", at + "conv2.bias"),
                                self.embed_positions.data, W, T, C)
        if self.ckpt_plan is None or self.ckpt_plan.get("_windows") != W:   # stand-alone call (forward() plans both towers before it gets here)
            self._make_ckpt_plan(W, 0)
        n_ck = self.enc_layers if self.ckpt_plan is None else self.ckpt_plan["enc"]
        for i in range(self.enc_layers):
            p = f"{at}layers.{i}."
            x = self._layer(F_.EncoderLayerFn.apply, x, self._anchor(p + "fc1.weight"), a, p, W, T2, self.enc_heads, kv_len, ckpt=i < n_ck)
        T3 = T2 // 2
        x = F_.PoolNormFn.apply(x, self._anchor(at + "layer_norm.weight"), a, at + "layer_norm.weight", at + "layer_norm.bias", W * T3)
        x = self._post_encoder(x, W, T3, n_tok, input_ids)
        x = F_.ProjectorFn.apply(x, self._anchor(self._pj + "linear_1.weight"), a, self._pj)
        return x, n_tok

    # ------------------------------------------------------------------ forward (a10-a18)
    @staticmethod
    def _mask_intervals(attention_mask):
        """attention_mask [B, S] of 0/1 -> (lo [B], hi [B]) of the single run of ones per row, or None when nothing is padded.
        Computed on the mask's own device: a CPU mask (what a collator hands over) costs no device sync."""
        am = attention_mask != 0
        if bool(am.all()):
            return None
        S = am.shape[1]
        n = am.sum(-1)
        lo = am.to(torch.uint8).argmax(-1)
        lo = torch.where(n > 0, lo, torch.zeros_like(lo))
        hi = lo + n
        ar = torch.arange(S, device=am.device)[None]
        if not bool((am == ((ar >= lo[:, None]) & (ar < hi[:, None]))).all()):
            raise AfkError("attention_mask rows must each be ONE contiguous run of ones (left and/or right padding); got a mask with holes")
        return lo, hi

    _rows_cache = None  # (weakref(labels tensor), version, rows) - see _valid_rows
    # True: the POSITIONS of the labelled rows never change for a given labels tensor object, only the token values written into it do
    # (a static input buffer refilled in place every step: bench.py's rotating synthetic batches, a HIP-graph-replayed step).  The row
    # indices are then remembered per tensor object regardless of its version - no device scan, no host sync per step.
    label_rows_static = False
    label_rows_check = True   # with label_rows_static: device-side check (no sync) that the labelled-row COUNT still matches; a mismatch turns the loss into NaN
    _rows_poison = None

    def _valid_rows(self, labels):
        """-> (shift_labels [B*S] on the device, rows) with rows = int64 indices (device) of the positions whose SHIFTED label is not -100,
        or None when the lm_head should run on every row (all valid, or none).  The row count must be known on the host (it sizes the
        GEMMs): labels that arrive on the CPU (a collator's output) are scanned there - no device sync; device labels are scanned on
        the device (one sync) and the result is remembered for as long as the SAME tensor object (same version) comes back."""
        import weakref

        dev = self.device_
        sh = torch.nn.functional.pad(labels, (0, 1), value=-100)[:, 1:].reshape(-1)
        if not labels.is_cuda:
            rows = (sh != -100).nonzero().reshape(-1)
            shift = sh.to(dev).contiguous()
            rows = rows.to(dev) if 0 < rows.numel() < sh.numel() else None
            return shift, rows
        c = self._rows_cache
        if c is not None and c[0]() is labels and (c[1] == labels._version or self.label_rows_static):
            if self.label_rows_static and c[1] != labels._version and self.label_rows_check:
                # the promise is checked without a host sync: the number of labelled positions is compared ON THE DEVICE with the remembered
                # count and a mismatch poisons the loss (NaN), so a batch whose labelled positions moved cannot train on stale rows silently
                n_now = (sh != -100).sum()
                self._rows_poison = torch.where(n_now == c[3], 0.0, float("nan")).to(torch.float32)
            return sh.contiguous(), c[2]
        rows = (sh != -100).nonzero().reshape(-1)  # host sync: the count sizes the GEMMs
        rows = rows if 0 < rows.numel() < sh.numel() else None
        # the REAL labelled count is always remembered (rows is None both for "no row" and "every row"; label_rows_static may be switched on after this call,
        # and a remembered -1 would poison the next in-place label update - ADVICE r04)
        self._rows_cache = (weakref.ref(labels), labels._version, rows, int(rows.numel()) if rows is not None else int((sh != -100).sum()))
        return sh.contiguous(), rows

    def forward(self, input_ids=None, input_features=None, input_features_mask=None, attention_mask=None, position_ids=None,
                past_key_values=None, inputs_embeds=None, labels=None, use_cache=None, logits_to_keep=0, return_logits=None,
                num_items_in_batch=None, return_token_logprobs=False, return_token_entropy=False, **kwargs):
        if (input_ids is None) == (inputs_embeds is None):
            raise ValueError("You must specify exactly one of input_ids or inputs_embeds")
        if return_token_logprobs and labels is None:
            raise ValueError("return_token_logprobs=True needs labels: the log-probabilities are those of the label tokens")
        if return_token_entropy and not return_token_logprobs:
            raise ValueError("return_token_entropy=True needs return_token_logprobs=True: the entropy comes out of the same sweep over the logits")
        self._require_hip()
        from . import exact as _exact

        if return_token_logprobs:
            if past_key_values is not None or use_cache:
                raise AfkError("forward(return_token_logprobs=True, use_cache=True / past_key_values=...): the KV-cache path is inference only and has no "
                               "loss head; score the tokens with a plain labelled forward")
            if self._graphed_step or torch.cuda.is_current_stream_capturing():
                raise AfkError("forward(return_token_logprobs=True) inside GraphedTrainStep / a HIP-graph capture: the replayed step keeps the mean-CE "
                               "loss route only; run the step with a loss on out.token_logprobs eagerly")
            if _exact.ENABLED:
                raise AfkError("forward(return_token_logprobs=True) under AFK_EXACT_FP32=1: the exact-fp32 verification forward has no loss head; "
                               "unset AFK_EXACT_FP32")

        if _exact.ENABLED and labels is None and inputs_embeds is None and past_key_values is None and not torch.is_grad_enabled():
            # AFK_EXACT_FP32=1 (verification mode, exact.py): the inference forward in exact fp32 on the afk_x32_* kernels - fp32 logits, no KV cache.
            # What the mode does not implement is refused, never silently dropped
            if position_ids is not None or use_cache or logits_to_keep not in (0, None):
                raise AfkError("AFK_EXACT_FP32=1: the exact-fp32 verification forward takes no position_ids / use_cache / logits_to_keep "
                               "(positions are cumsum(attention_mask) - 1, every row's logits are returned, there is no KV cache); unset AFK_EXACT_FP32 for those")
            return AF3Output(logits=_exact.logits(self, input_ids, input_features, input_features_mask, attention_mask))
        if past_key_values is not None or use_cache:
            # inference with the reference's cache protocol (modeling_qwen2.py:213-214, 360-364): prefill returns a cache, later calls
            # append their tokens to it.  Same kernels and cache layout as generate(); no autograd graph.
            if labels is not None:
                raise AfkError("forward(labels=..., use_cache=True): the KV-cache path is inference only")
            return self._forward_cached(input_ids, inputs_embeds, input_features, input_features_mask, attention_mask, past_key_values,
                                        logits_to_keep, position_ids)
        a, lm = self.arena, self._lm
        if inputs_embeds is not None:
            # the reference merges audio only when input_ids are given (modeling_audioflamingo3.py:532-545): precomputed embeddings pass through
            B, S = inputs_embeds.shape[:2]
            ids = ids_flat = None
            input_features = None
        else:
            ids = input_ids.to(self.device_)
            B, S = ids.shape
            ids_flat = ids.reshape(-1).contiguous()
        audio, src = None, None
        # checkpoint plan of BOTH towers from the batch geometry, before the first layer allocates anything (memory-budgeted recompute)
        self._make_ckpt_plan(0 if input_features is None else int(input_features.shape[0]), B * S)
        if self.ckpt_plan is not None:
            self.ckpt_plan["_windows"] = 0 if input_features is None else int(input_features.shape[0])
        if input_features is not None:
            audio, n_tok = self.get_audio_features(input_features.to(self.device_), input_features_mask, input_ids=ids)
            src, cnt = ops.placeholder_scan(ids_flat, self.audio_token_id)
            T3 = audio.shape[0] // input_features.shape[0]
            if n_tok is not None:
                # rank r among placeholders -> row (window, t) of the padded audio buffer  (:483-486 boolean index)
                csum = torch.cumsum(n_tok, 0)
                r = src.clamp_min(0).to(torch.int64)
                win = torch.searchsorted(csum, r, right=True).clamp_max(n_tok.numel() - 1)
                row = win * T3 + (r - (csum - n_tok)[win])
                src = torch.where(src >= 0, row.to(torch.int32), src).contiguous()
                expected = csum[-1]
            else:
                expected = audio.shape[0]
            if self.check_placeholders:
                n = int(cnt.item())
                e = int(expected)
                if n != e:
                    raise ValueError(f"Audio features and audio tokens do not match, tokens: {n}, features: {e}")
        kv_len, krange, kv_lo = None, None, None
        if attention_mask is not None:
            iv = self._mask_intervals(attention_mask)
            if iv is not None:
                lo, hi = iv
                if bool((lo == 0).all()):   # right padding only: the LDS-staged causal kernels take the key count per sample
                    kv_len = hi.to(self.device_, torch.int32).contiguous()
                elif ops._use_lds(self.D) and self.left_pad_on_lds_kernels:
                    # left padding (processing_audioflamingo3.py:46) on the same kernels: keys [lo_b, hi_b) per sample, causal
                    kv_len = hi.to(self.device_, torch.int32).contiguous()
                    kv_lo = lo.to(self.device_, torch.int32).contiguous()
                else:                        # other head sizes: causal AND key in [lo_b, hi_b) per query row on the interval kernels
                    lo, hi = lo.to(self.device_, torch.int32), hi.to(self.device_, torch.int32)
                    i1 = torch.arange(1, S + 1, device=self.device_, dtype=torch.int32)[None]
                    end = torch.minimum(i1, hi[:, None])
                    krange = torch.stack([lo[:, None].expand(B, S), torch.maximum(end, lo[:, None])], -1).contiguous()
        pos = None
        if position_ids is not None:
            pos = position_ids.to(self.device_).expand(B, S).reshape(-1).to(torch.int32).contiguous()
        cos, sin = self._rope_tables(S if pos is None else int(self.config.text_config.max_position_embeddings))
        if inputs_embeds is not None:
            x = inputs_embeds.to(self.device_, torch.bfloat16).reshape(B * S, self.H).contiguous()
        else:
            x = F_.EmbedScatterFn.apply(audio, self._anchor(lm + "embed_tokens.weight"), a, lm + "embed_tokens.weight", ids_flat, src)
        audio_hidden = audio
        if kwargs.get("output_attentions"):
            raise AfkError("output_attentions=True: the attention kernels never materialise the probabilities (the reference's default sdpa path returns none either)")
        want_hidden = bool(kwargs.get("output_hidden_states", getattr(self.config, "output_hidden_states", False)))
        hidden = [x.reshape(B, S, -1)] if want_hidden else None      # the reference's tuple: merged embeddings, every layer's output, ...
        # the positions the loss reads, known before the decoder runs: behind its attention, the LAST decoder layer (and the final norm) run on those rows alone
        # (round 6, DecoderLayerFn rows=...: a quarter of the rows on the 256-answer-token batches of the benchmark) whenever nobody asks for the hidden states or
        # the logits of the other positions inside this call; the lazy `output.logits` of a labelled call re-runs the last layer on every row when it is read
        shift = rows = None
        if labels is not None:
            shift, rows = self._valid_rows(labels) if self.loss_on_valid_rows_only else (
                torch.nn.functional.pad(labels.to(self.device_), (0, 1), value=-100)[:, 1:].reshape(-1).contiguous(), None)
        last_rows = rows if (rows is not None and self.last_layer_rows_only and torch.is_grad_enabled() and not want_hidden and not return_logits
                             and self.dec_layers > 0) else None
        x_before_last, last_args = None, None
        for i in range(self.dec_layers):
            p = f"{lm}layers.{i}."
            la = (self._anchor(p + "mlp.down_proj.weight"), a, p, B, S, self.Hq, self.Hkv, self.D, self.rms_eps, cos, sin, pos, kv_len, krange, kv_lo)
            if i + 1 == self.dec_layers and last_rows is not None:
                x_before_last, last_args = x, la
                x = self._layer(F_.DecoderLayerFn.apply, x, *la, last_rows, ckpt=self.ckpt_plan is None or i < self.ckpt_plan["dec"])
            else:
                x = self._layer(F_.DecoderLayerFn.apply, x, *la, ckpt=self.ckpt_plan is None or i < self.ckpt_plan["dec"])
            if want_hidden and i + 1 < self.dec_layers:
                hidden.append(x.reshape(B, S, -1))
        x = F_.RMSNormFn.apply(x, self._anchor(lm + "norm.weight"), a, lm + "norm.weight", self.rms_eps)
        if want_hidden:
            hidden.append(x.reshape(B, S, -1))                            # ... with the LAST entry taken after the final norm (lm_head(hidden[-1]) == logits)
            hidden = tuple(hidden)
        loss, logits, token_logprobs, token_entropy = None, None, None, None
        if labels is not None:
            if last_rows is not None:   # x already holds the labelled rows only, in order
                shift, rows = shift.index_select(0, last_rows), None
            if num_items_in_batch is not None:
                denom = torch.as_tensor(num_items_in_batch, device=self.device_, dtype=torch.float32).reshape(1)
            else:
                denom = ops.count_valid(shift)
            if return_token_logprobs:
                # the per-token stage (F_.LMHeadLogprobFn): log p(label) per labelled row, with a gradient per row; the mean-CE stage does not run -
                # out.loss is built from the same tensor by torch ops
                at = last_rows if last_rows is not None else rows        # the flat positions (of the SHIFTED labels) x / rows stand for; None = every row
                lp = F_.LMHeadLogprobFn.apply(x, self._anchor("lm_head.weight"), a, "lm_head.weight", shift, bool(return_token_entropy), rows)
                lp, ent = (lp[0], lp[1].detach()) if return_token_entropy else (lp, None)

                def _place(v):
                    # row i = b * S + t - 1 of the shifted labels scores labels[b, t]: one step to the right; [b, 0] and every ignored position stay 0
                    flat = v if at is None else torch.zeros(B * S, device=v.device, dtype=v.dtype).index_copy(0, at, v)
                    return torch.nn.functional.pad(flat.reshape(B, S)[:, :-1], (1, 0))

                token_logprobs = _place(lp)
                token_entropy = None if ent is None else _place(ent)
                loss = -(token_logprobs.sum() / denom.reshape(()).clamp_min(1.0))
            else:
                loss = F_.LMHeadLossFn.apply(x, self._anchor("lm_head.weight"), a, "lm_head.weight", shift, denom, rows)
            if self._rows_poison is not None:   # label_rows_static promise broken -> NaN loss (see _valid_rows); 0.0 otherwise
                loss, self._rows_poison = loss + self._rows_poison, None
        def _logits(xh=x):
            xs = xh
            if isinstance(logits_to_keep, int) and logits_to_keep > 0:
                xs = xh.reshape(B, S, -1)[:, -logits_to_keep:, :].reshape(-1, xh.shape[-1]).contiguous()
            return F_.LMHeadFn.apply(xs, self._anchor("lm_head.weight"), a, "lm_head.weight").reshape(B, -1, self.V)

        if labels is None or return_logits:
            return AF3Output(loss=loss, logits=_logits(), hidden_states=hidden, audio_hidden_states=audio_hidden, token_logprobs=token_logprobs,
                             token_entropy=token_entropy)
        # labels given: the reference returns logits beside the loss (modeling_audioflamingo3.py:625-642); here they are built on first access -
        # from the DETACHED final hidden states (no second autograd branch, the step's graph is not kept alive by the output object) and only while
        # the weights are still the ones the loss was computed with: after an optimizer step the lm_head has moved, the logits would no longer
        # belong to `loss`, and the access raises instead (forward(return_logits=True) is the in-graph, forward-time path)
        x_keep, weights_at = (x if last_rows is None else x_before_last).detach(), a.version()

        def _lazy_logits():
            if a.version() != weights_at:
                raise AfkError("output.logits was first read after the parameters changed (optimizer step / load_state_dict): lazy logits would be "
                               "computed with other weights than output.loss; read them before the step or call forward(return_logits=True)")
            with torch.no_grad():
                if last_rows is None:
                    return _logits(x_keep)
                # the step ran its last layer on the labelled rows only: every position's logits need that layer (and the final norm) on every row
                xf = F_.DecoderLayerFn.apply(x_keep, *last_args)
                return _logits(F_.RMSNormFn.apply(xf, self._anchor(lm + "norm.weight"), a, lm + "norm.weight", self.rms_eps))

        return AF3Output(loss=loss, logits_fn=_lazy_logits, hidden_states=hidden, audio_hidden_states=audio_hidden, token_logprobs=token_logprobs,
                         token_entropy=token_entropy)

    # ------------------------------------------------------------------ generate (greedy; KV cache - SURVEY.md 8(f)-4)
    def _merged_embeddings(self, ids, input_features, input_features_mask):
        """embed_tokens(ids) with the <sound> rows replaced by the projected audio rows (forward() stages a9-a10) -> [B*S, H]"""
        a, lm = self.arena, self._lm
        ids_flat = ids.reshape(-1).contiguous()
        audio, src = None, None
        if input_features is not None:
            audio, n_tok = self.get_audio_features(input_features.to(self.device_), input_features_mask, input_ids=ids)
            src, _ = ops.placeholder_scan(ids_flat, self.audio_token_id)
            if n_tok is not None:
                T3 = audio.shape[0] // input_features.shape[0]
                csum = torch.cumsum(n_tok, 0)
                r = src.clamp_min(0).to(torch.int64)
                win = torch.searchsorted(csum, r, right=True).clamp_max(n_tok.numel() - 1)
                row = win * T3 + (r - (csum - n_tok)[win])
                src = torch.where(src >= 0, row.to(torch.int32), src).contiguous()
        return ops.embed_scatter_fwd(ids_flat, src, a[lm + "embed_tokens.weight"].data, audio)

    _graphed_step = False   # set by graphs.GraphedTrainStep around its eager warm-up steps
    loss_on_valid_rows_only = True  # lm_head + CE (+ their backward GEMMs) on the rows with a label only (False: all B*S rows, as the reference)
    last_layer_rows_only = os.environ.get("AFK_LAST_LAYER_ROWS", "1") == "1"   # training forward with labels: the last decoder layer behind its attention on the labelled rows only

    # gradient bookkeeping -------------------------------------------------------------------------
    def zero_grad(self, set_to_none: bool = False):
        self.arena.zero_grad()

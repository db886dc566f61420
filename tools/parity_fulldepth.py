#!/usr/bin/env python
"""Full-depth parity record on the configuration the benchmark times (VERDICT r04 "missing" #2 / "next" #1).

BASELINE configs[1]: AF3-7B (32 encoder + 28 decoder layers), B = 8, S = 1024, one 30 s window per sample - ONE state_dict in
  (1) the live reference  transformers.AudioFlamingo3ForConditionalGeneration in fp32 on this GPU      = ground truth
      (modeling_audioflamingo3.py:584-642, modeling_qwen2.py:342-402; eager, sdpa, micro-batches of 2 with fp32 gradient accumulation),
  (2) the same reference in bf16 on this GPU (full batch, as bench.py's eager leg runs it)                = the noise floor of ANY bf16 implementation,
  (3) this repo's model (libafk.so)                                                                      = what is checked,
all three on the SAME synthetic batch (bench.synthetic_batch).  The reference gets its features from ITS OWN frontend
(WhisperFeatureExtractor on the host, feature_extraction_whisper.py:135-168); ours computes them with afk_logmel on the device - the comparison is end
to end from the waveform.

Compared: first-step loss; logits on the 2 048 labelled rows; argmax on the rows whose fp32 top-1/top-2 gap exceeds twice the logit bar; EVERY parameter
gradient (rel-L2 against fp32, beside the reference-bf16 figure for the same tensor); gradient norm per layer bucket; the first AdamW update (sign
agreement with the update the fp32 gradients imply, parameter-sum delta).  BASELINE configs[4] (one 5-minute clip: 10 windows, S = 7 774) is compared
forward-only (loss, labelled logits, argmax).

Bars (tests/_tol.py): |d loss| <= 1e-2; |d logit| <= 2^-6 * max(1, |ref|max) or 2 x the reference-bf16 figure; 0 argmax mismatches on confident rows;
per-tensor gradient rel-L2 <= max(6e-2, 2 x the reference-bf16 figure of that tensor) ("ours <= 2 x (oracle bf16 vs fp32)").

Used by bench.py (untimed leg -> `parity_fulldepth` in the JSON line) and tests/test_fullwidth_gpu.py.  Needs ~230 GiB of HBM at its peak (our replica
with fp32 optimizer state beside the kept fp32 reference gradients).  The reference is imported as the CHECKER only.
"""
import gc
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

LOGIT_RTOL, LOSS_ATOL, GRAD_REL_L2, FLOOR_FACTOR, NOISE_DOMINATED = 2.0 ** -6, 1e-2, 6e-2, 2.0, 0.5   # tests/_tol.py
BF = torch.bfloat16


def _rel(a, b):
    a, b = a.float(), b.float()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


def _sum64(t, chunk=1 << 28):
    """fp64 sum of a large tensor without a full-size temporary"""
    f = t.reshape(-1)
    return float(sum(f[i:i + chunk].double().sum() for i in range(0, f.numel(), chunk)))


def _free():
    gc.collect()
    torch.cuda.empty_cache()


def _group(key):
    """layer bucket of a reference parameter name (the arena's buckets: one per transformer layer + the stems and heads)"""
    p = key.split(".")
    if "layers" in p:
        i = p.index("layers")
        return ("enc" if "audio_tower" in key else "dec") + f".{int(p[i + 1]):02d}"
    if "audio_tower" in key:
        return "enc.stem+ln"
    if "multi_modal_projector" in key:
        return "projector"
    if key == "lm_head.weight":
        return "lm_head"
    return "dec.embed+norm"


def restore_rope_buffers(model):
    """`module.to(torch.bfloat16)` rounds EVERY floating buffer - including the rotary embedding's non-persistent `inv_freq` (modeling_qwen2.py:67-68),
    and a later `.float()` only upcasts the rounded values: at theta = 1e6 and position 1 000 the highest frequencies are then off by radians.  A
    checkpoint loaded with `from_pretrained(dtype=bf16)` never goes through `.to()` and keeps the fp32 buffer (`:87` computes it with an explicit fp32
    arange) - that is the behaviour this repo implements, so the harness puts the fp32 values back after every dtype change of the reference."""
    for mod in model.modules():
        if hasattr(mod, "inv_freq") and hasattr(mod, "compute_default_rope_parameters") and getattr(mod, "rope_type", "default") == "default":
            inv, _ = mod.compute_default_rope_parameters(mod.config, mod.inv_freq.device)
            mod.inv_freq = torch.nn.Buffer(inv.float(), persistent=False)
            mod.original_inv_freq = torch.nn.Buffer(inv.float().clone(), persistent=False)
            if hasattr(mod, "position_angles") and hasattr(mod, "_compute_position_angles"):   # Music Flamingo's rotary TIME embedding: its angle table and
                mod.position_angles = torch.nn.Buffer(mod._compute_position_angles(mod.inv_freq), persistent=False)   # every timestamp take inv_freq's dtype
    return model


def _reference_features(waves_np):
    """the reference's own frontend, on the host (feature_extraction_whisper.py:135-168; chunk length 30 s, 128 mel bins)"""
    from transformers import WhisperFeatureExtractor

    fe = WhisperFeatureExtractor(feature_size=128)
    out = fe([w for w in waves_np], sampling_rate=16000, return_tensors="pt", return_attention_mask=True, padding="max_length")
    return out["input_features"], out["attention_mask"]


def _labelled_rows(labels):
    """rows whose NEXT token carries a label (loss_utils.py:65-66 shift): [B, S] bool"""
    return torch.nn.functional.pad(labels, (0, 1), value=-100)[:, 1:] != -100


def _ref_forward(model, ids, feats, fmask, labels, dtype, micro, backward):
    """reference forward (+ backward with gradient accumulation in the parameter dtype's .grad) -> loss (python float), labelled-row logits [n, V] (dtype)"""
    B = ids.shape[0]
    wps = feats.shape[0] // B          # windows per sample (window-major inside a sample, bench.synthetic_batch)
    n_micro = (B + micro - 1) // micro
    sel_all = _labelled_rows(labels)
    losses, lg = [], []
    for i in range(0, B, micro):
        kw = dict(input_ids=ids[i:i + micro], input_features=feats[i * wps:(i + micro) * wps].to(dtype), input_features_mask=fmask[i * wps:(i + micro) * wps], labels=labels[i:i + micro])
        if backward:
            out = model(**kw)
            (out.loss / n_micro).backward()
        else:
            with torch.no_grad():
                out = model(**kw)
        losses.append(float(out.loss.detach()))
        lg.append(out.logits.detach()[sel_all[i:i + micro]].clone())
        del out
    # every sample carries the same number of labelled tokens (bench.synthetic_batch): the batch mean is the mean of the micro-batch means
    return float(np.mean(losses)), torch.cat(lg, 0)


def _logit_stats(got, ref32, noise=None):
    """noise: the reference-bf16 run's own max |d logit| on these rows (None while that run itself is being scored).  "Confident" rows (SURVEY.md §8c:
    "argmax equal wherever the fp32 top-1/top-2 gap exceeds the measured bf16 noise"): gap > 2 x max(logit bar, measured noise) - top-1 may fall and
    top-2 rise by the noise each.  The count under the bar alone (tests/_tol.py's rule at the tiny goldens' depth) is reported beside it."""
    d = (got.float() - ref32).abs()
    absmax = float(ref32.abs().max())
    tol = LOGIT_RTOL * max(1.0, absmax)
    top2 = ref32.topk(2, -1).values
    gap = top2[:, 0] - top2[:, 1]
    wrong = got.float().argmax(-1) != ref32.argmax(-1)
    conf_bar = gap > 2 * tol
    out = {"max_abs_err": float(d.max()), "rel_l2": _rel(got, ref32), "ref_absmax": absmax, "abs_bar": tol, "rows": int(ref32.shape[0]),
           "confident_rows_bar_only": int(conf_bar.sum()), "argmax_mismatches_bar_only": int((wrong & conf_bar).sum()),
           "argmax_agreement_all_rows": float((~wrong).float().mean())}
    if noise is not None:
        conf = gap > 2 * max(tol, noise)
        out.update({"confident_gap": 2 * max(tol, noise), "confident_rows": int(conf.sum()), "argmax_mismatches_on_confident_rows": int((wrong & conf).sum())})
    return out


# ---------------------------------------------------------------------------------------------------------------- weight sets
# "init":   the reference's own _init_weights (normal 0.02) with biases / norm weights moved off their trivial values.  Faithful to bench.py's weights, but a
#           random-init 7B model has FLAT logits (top-1/top-2 gap below the bf16 noise on 97 % of the rows) and near-UNIFORM attention (the q / k projections'
#           gradients are differences of nearly equal numbers: 93 of 829 tensors are noise in the reference's own bf16 run) - round 5's record had no teeth there.
# "peaked": the same init, then  (i) every q / k projection (weights and biases) of both towers scaled so that the attention
#           softmax concentrates (encoder x 6, decoder x 1.7; calibrated on the GPU in round 6 - encoder x 1.5 ... 4.5 left 50-93 of the 208 q / k
#           gradient tensors below the reference's own bf16 noise, x 8 saturates the softmax and loses them again, x 6: none), (ii) embed_tokens scaled x 200 so that the token identity survives the
#           28 random layers in the residual stream and lm_head = embed_tokens / 480 so that the logit of the CURRENT token stands ~ 20 sigma above
#           the rest: argmax is then decided on (nearly) every row and the q / k gradients carry signal.  Same code path, same shapes, same kernels.
PEAKED = dict(enc_qk=float(os.environ.get("AFK_PEAK_ENC_QK", "6")), dec_qk=float(os.environ.get("AFK_PEAK_DEC_QK", "1.7")),
              embed=float(os.environ.get("AFK_PEAK_EMBED", "200")), head=float(os.environ.get("AFK_PEAK_HEAD", str(1.0 / 480))),
              audio=float(os.environ.get("AFK_PEAK_AUDIO", "200")))


def _build_state(cfg, dev, variant):
    """-> (reference model in bf16, train mode; its state_dict copy).  One state_dict serves the fp32 truth, the bf16 floor and this repo's model."""
    from transformers import AudioFlamingo3ForConditionalGeneration as Ref

    torch.manual_seed(0)
    with torch.device(dev):
        ref = Ref(cfg)
    g = torch.Generator(device=dev).manual_seed(4)
    with torch.no_grad():
        for k, p in ref.named_parameters():   # biases (zero) and norm weights (one) off their trivial init so that every gradient path carries signal
            if k.endswith(".bias"):
                p.copy_(0.02 * torch.randn(p.shape, device=dev, generator=g))
            elif "norm" in k.split(".")[-2] and k.endswith(".weight"):
                p.copy_(1 + 0.05 * torch.randn(p.shape, device=dev, generator=g))
        if variant == "peaked":
            for k, p in ref.named_parameters():
                if ".self_attn.q_proj." in k or ".self_attn.k_proj." in k:
                    p.mul_(PEAKED["enc_qk"] if "audio_tower" in k else PEAKED["dec_qk"])
            emb = ref.get_input_embeddings().weight
            emb.mul_(PEAKED["embed"])
            ref.lm_head.weight.copy_(emb * PEAKED["head"])
            # the audio rows enter the decoder beside the (scaled) text embeddings: the projector's output layer is scaled alike, or the loss would barely
            # depend on the audio tower and EVERY encoder gradient would be bf16 noise (first calibration run: 461 of 829 tensors noise-dominated)
            for k, p in ref.named_parameters():
                if "multi_modal_projector.linear_2." in k:
                    p.mul_(PEAKED["audio"])
    ref.to(BF)
    sd = {k: v.detach().clone() for k, v in ref.state_dict().items()}
    ref.train()
    return ref, sd


def _attention_peak(ref, ids, feats, fmask):
    """how concentrated the attention of this weight set is: mean over (head, query) of the largest softmax probability in decoder layer 0 and encoder
    layer 0 of the fp32 reference on sample 0 (hooks on the two self_attn modules; scores rebuilt from their own q / k projections and rotary tables)"""
    from transformers.models.qwen2.modeling_qwen2 import apply_rotary_pos_emb

    cap = {}

    def pre(name):
        def hook(mod, args, kwargs):
            if name not in cap:
                cap[name] = (args[0] if args else kwargs["hidden_states"]).detach()[:1], kwargs.get("position_embeddings")
        return hook

    dec0, enc0 = ref.model.language_model.layers[0].self_attn, ref.model.audio_tower.layers[0].self_attn
    hs = [dec0.register_forward_pre_hook(pre("dec"), with_kwargs=True), enc0.register_forward_pre_hook(pre("enc"), with_kwargs=True)]
    try:
        with torch.no_grad():
            ref(input_ids=ids[:1], input_features=feats[:1].to(next(ref.parameters()).dtype), input_features_mask=fmask[:1])
    finally:
        for h in hs:
            h.remove()
    out = {}
    with torch.no_grad():
        x, pe = cap["dec"]
        S = x.shape[1]
        D = dec0.head_dim
        q = dec0.q_proj(x).view(1, S, -1, D).transpose(1, 2)
        k = dec0.k_proj(x).view(1, S, -1, D).transpose(1, 2)
        if pe is not None:
            q, k = apply_rotary_pos_emb(q, k, pe[0][:1], pe[1][:1])
        k = k.repeat_interleave(q.shape[1] // k.shape[1], 1)
        sc = (q.float() @ k.float().transpose(-1, -2)) * D ** -0.5
        sc = sc.masked_fill(torch.ones(S, S, device=sc.device, dtype=torch.bool).triu(1), float("-inf"))
        pm = sc.softmax(-1).amax(-1)
        out["decoder_layer0_mean_max_prob"] = float(pm[..., S // 2:].mean())     # queries with >= S / 2 visible keys
        x, _ = cap["enc"]
        T = x.shape[1]
        De = enc0.head_dim
        q = (enc0.q_proj(x) * De ** -0.5).view(1, T, -1, De).transpose(1, 2)
        k = enc0.k_proj(x).view(1, T, -1, De).transpose(1, 2)
        out["encoder_layer0_mean_max_prob"] = float((q.float() @ k.float().transpose(-1, -2)).softmax(-1).amax(-1).mean())
    return out


def _score_gradients(named_grads, g32, floor_g, floor_sign, gn16, enc_layers, dec_layers):
    """every parameter gradient of ours against the fp32 truth, beside the reference-bf16 figure of the same tensor -> (record, over-the-bar dict)"""
    grads, bad, noisy, gn, gn32 = {}, {}, {}, {}, {}
    sign_ok = sign_n = fsign_ok = fsign_n = 0
    for k, gr in g32.items():
        pg = named_grads.get(k)
        if pg is None:
            continue
        r = _rel(pg, gr)
        grads[k] = r
        if floor_g[k] > NOISE_DOMINATED:   # the reference's own bf16 run is off by more than half this tensor's fp32 norm: bf16 cannot resolve it on this
            noisy[k] = {"ours": r, "floor": floor_g[k], "fp32_norm": float(gr.norm())}   # batch (tests/_tol.py NOISE_DOMINATED) - reported, held to the floor itself
            if r > FLOOR_FACTOR * floor_g[k]:
                bad[k] = {"ours": r, "floor": floor_g[k]}
        elif r > max(GRAD_REL_L2, FLOOR_FACTOR * floor_g[k]):
            bad[k] = {"ours": r, "floor": floor_g[k]}
        gn[_group(k)] = gn.get(_group(k), 0.0) + float(pg.float().square().sum())
        gn32[_group(k)] = gn32.get(_group(k), 0.0) + float(gr.square().sum())
        sign_ok += int((torch.sign(pg.float()) == torch.sign(gr)).sum())
        sign_n += pg.numel()
        fsign_ok += floor_sign[k][0]
        fsign_n += floor_sign[k][1]
    resolved = {k: v for k, v in grads.items() if k not in noisy} or grads
    worst = max(resolved, key=resolved.get)
    # >= 10 tensors spread over depth, by name (the record lists every tensor's figure in `all_tensors`)
    el, dl = enc_layers - 1, dec_layers - 1
    spread = ["model.audio_tower.conv1.weight", "model.audio_tower.layers.0.self_attn.q_proj.weight", f"model.audio_tower.layers.{el // 2}.fc1.weight",
              f"model.audio_tower.layers.{el}.fc2.weight", "model.multi_modal_projector.linear_1.weight", "model.language_model.embed_tokens.weight",
              "model.language_model.layers.0.self_attn.q_proj.weight", "model.language_model.layers.0.mlp.gate_proj.weight",
              f"model.language_model.layers.{dl // 2}.self_attn.k_proj.bias", f"model.language_model.layers.{dl // 2}.mlp.down_proj.weight",
              f"model.language_model.layers.{dl}.mlp.up_proj.weight", f"model.language_model.layers.{dl}.post_attention_layernorm.weight",
              "model.language_model.norm.weight", "lm_head.weight"]
    ratios = sorted(grads[k] / max(floor_g[k], 1e-12) for k in grads)
    qk = [k for k in grads if ".self_attn.q_proj." in k or ".self_attn.k_proj." in k]
    rec = {"tensors": len(grads), "worst": {"name": worst, "ours": grads[worst], "floor": floor_g[worst]},
           "median_rel_l2": float(np.median(list(grads.values()))), "median_floor": float(np.median([floor_g[k] for k in grads])),
           "ours_over_floor": {"median": ratios[len(ratios) // 2], "p95": ratios[int(0.95 * len(ratios))], "max": ratios[-1]},
           "over_bar": bad, "noise_dominated_in_the_reference_bf16_run": noisy, "spread": {k: {"ours": grads[k], "floor": floor_g[k]} for k in spread if k in grads},
           "qk_projection_tensors": {"count": len(qk), "asserted_against_the_fixed_or_2x_floor_bar": sum(1 for k in qk if k not in noisy),
                                     "noise_dominated": sum(1 for k in qk if k in noisy), "worst_ours_over_floor": max((grads[k] / max(floor_g[k], 1e-12) for k in qk), default=None)},
           "sign_agreement_with_fp32": sign_ok / max(sign_n, 1), "sign_agreement_floor": fsign_ok / max(fsign_n, 1),
           "bucket_norms": {b: {"ours": gn[b] ** 0.5, "fp32": gn32[b] ** 0.5, "ref_bf16": gn16[b] ** 0.5} for b in sorted(gn)},
           "bucket_norm_rel_err_max": max(abs(gn[b] ** 0.5 - gn32[b] ** 0.5) / max(gn32[b] ** 0.5, 1e-30) for b in gn),
           "all_tensors": {k: [round(grads[k], 5), round(floor_g[k], 5)] for k in grads}}
    return rec, bad


def _reference_runs(ref, sd, ids, feats_ref, fmask, labels, micro_fp32, batch, ckpt, log, tag):
    """(1) fp32 truth and (2) the reference's own bf16 run on one batch -> dict(loss32, lg32, g32, loss16, lg16, floor_g, floor_sign, gn16).
    ckpt: run the reference with ITS activation checkpointing (gradient_checkpointing_enable, modeling_layers.py:79-114) - the long-audio leg."""
    if ckpt:
        ref.gradient_checkpointing_enable()
    restore_rope_buffers(ref.float())
    t0 = time.perf_counter()
    loss32, lg32 = _ref_forward(ref, ids, feats_ref, fmask, labels, torch.float32, micro_fp32, True)
    g32 = {k: p.grad.detach().clone() for k, p in ref.named_parameters() if p.grad is not None}
    ref.zero_grad(set_to_none=True)
    torch.cuda.synchronize()
    log(f"[parity:{tag}] fp32 reference: loss {loss32:.6f}, {len(g32)} gradient tensors, {time.perf_counter() - t0:.1f} s")
    out = {"loss32": loss32, "lg32": lg32, "g32": g32}
    return out


def _floor_run(ref, sd, ids, feats_ref, fmask, labels, batch, g32, log, tag):
    restore_rope_buffers(ref.to(BF))
    assert all(torch.equal(v, sd[k]) for k, v in list(ref.state_dict().items())[:8]), "bf16 -> fp32 -> bf16 must give the weights back"
    t0 = time.perf_counter()
    loss16, lg16 = _ref_forward(ref, ids, feats_ref, fmask, labels, BF, batch, True)
    floor_g = {k: _rel(p.grad, g32[k]) for k, p in ref.named_parameters() if p.grad is not None}
    floor_sign, gn16 = {}, {}
    for k, p in ref.named_parameters():
        if p.grad is not None:
            gn16[_group(k)] = gn16.get(_group(k), 0.0) + float(p.grad.float().square().sum())
            floor_sign[k] = (int((torch.sign(p.grad.float()) == torch.sign(g32[k])).sum()), p.numel())
    ref.zero_grad(set_to_none=True)
    torch.cuda.synchronize()
    log(f"[parity:{tag}] bf16 reference: loss {loss16:.6f}, worst gradient rel-L2 vs fp32 {max(floor_g.values()):.4f}, {time.perf_counter() - t0:.1f} s")
    return {"loss16": loss16, "lg16": lg16, "floor_g": floor_g, "floor_sign": floor_sign, "gn16": gn16}


def _leg(dev, cfg, variant, batch, micro_fp32, long_windows, lr, enc_layers, dec_layers, log, with_adamw=True):
    """one weight set on the BASELINE configs[1] batch: truth, floor, ours -> record (the round-5 record's layout) with res["checks"] / res["green"]"""
    import bench

    t_start = time.perf_counter()
    waves, ids, labels = bench.synthetic_batch(batch, 0, dev, 1)
    lwaves, lids, llabels = bench.synthetic_batch(1, 0, dev, long_windows) if long_windows else (None, None, None)
    feats_ref, fmask = (t.to(dev) for t in _reference_features(waves.cpu().numpy()))
    if long_windows:
        lfeats_ref, lfmask = (t.to(dev) for t in _reference_features(lwaves.cpu().numpy()))
    ref, sd = _build_state(cfg, dev, variant)
    wtxt = "reference _init_weights under torch.manual_seed(0), biases ~ N(0, 0.02), norm weights ~ 1 + N(0, 0.05)"
    if variant == "peaked":
        wtxt += (f"; then q / k projections x {PEAKED['enc_qk']} (encoder) / x {PEAKED['dec_qk']} (decoder), embed_tokens x {PEAKED['embed']:.0f}, "
                 f"projector linear_2 x {PEAKED['audio']:.0f}, lm_head = embed_tokens x {PEAKED['head']:.5f} (peaked attention, decided argmax)")
    res = {"config": ("BASELINE configs[1]: " if (enc_layers, dec_layers, batch) == (32, 28, 8) else "NOT the BASELINE config: ") +
                     "AF3-7B %d+%d layers, B=%d, S=%d, one 30 s window per sample, bf16" % (enc_layers, dec_layers, batch, ids.shape[1]),
           "weights": wtxt + ", rounded to bf16; the SAME state_dict in all three models", "weight_set": variant,
           "truth": f"reference in fp32 on this GPU (bf16-rounded weights upcast), micro-batches of {micro_fp32}, fp32 gradient accumulation",
           "floor": "reference in bf16 on this GPU (eager, sdpa), full batch", "bars": {"loss_abs": LOSS_ATOL, "logit_rtol": LOGIT_RTOL, "grad_rel_l2": GRAD_REL_L2,
                                                                                      "floor_factor": FLOOR_FACTOR}}
    T = _reference_runs(ref, sd, ids, feats_ref, fmask, labels, micro_fp32, batch, False, log, variant)
    loss32, lg32, g32 = T["loss32"], T["lg32"], T["g32"]
    try:
        res["attention_peak_fp32_reference"] = _attention_peak(ref, ids, feats_ref, fmask)
    except Exception as e:   # a diagnostic: never takes the record down
        res["attention_peak_fp32_reference"] = {"error": repr(e)[:200]}
    long32 = _ref_forward(ref, lids, lfeats_ref, lfmask, llabels, torch.float32, 1, False) if long_windows else None
    Fl = _floor_run(ref, sd, ids, feats_ref, fmask, labels, batch, g32, log, variant)
    loss16, lg16, floor_g, floor_sign, gn16 = Fl["loss16"], Fl["lg16"], Fl["floor_g"], Fl["floor_sign"], Fl["gn16"]
    long16 = _ref_forward(ref, lids, lfeats_ref, lfmask, llabels, BF, 1, False) if long_windows else None
    floor_logits = _logit_stats(lg16, lg32)
    del ref, lg16
    _free()

    # ---------------------------------------------------------------- (3) ours
    from audio_flamingo_amd.arena import FusedAdamW
    from audio_flamingo_amd.frontend import LogMelFrontend
    from audio_flamingo_amd.modeling import AudioFlamingo3ForConditionalGeneration as Mine

    t0 = time.perf_counter()
    m = Mine(cfg, device=dev, init_seed=0)
    m.load_state_dict(sd)
    del sd
    opt = FusedAdamW(m.arena, lr=lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, state_dtype="fp32") if with_adamw else None  # the check reads the fp32 master
    frontend = LogMelFrontend(dev)
    res["logmel_max_abs_diff_vs_reference_frontend"] = float((frontend(waves, out_dtype=torch.float32) - feats_ref).abs().max())
    if long_windows:   # forward only, BEFORE the optimizer moves the weights
        with torch.no_grad():
            lout = m(input_ids=lids, input_features=frontend(lwaves, out_dtype=BF), labels=llabels, return_logits=True)
        lsel = _labelled_rows(llabels)
        lloss, llg = float(lout.loss), lout.logits[lsel].clone()
        del lout
        lf = _logit_stats(long16[1], long32[1])
        ls = _logit_stats(llg, long32[1], lf["max_abs_err"])
        res["long5min_forward"] = {"config": f"BASELINE configs[4] shape: one 5-minute clip = {long_windows} windows, S = {lids.shape[1]}, forward only",
                                   "loss": lloss, "loss_ref_fp32": long32[0], "loss_ref_bf16": long16[0], "logits": ls, "logits_floor_ref_bf16": lf}
        del llg, long32, long16
        _free()
    m.zero_grad()
    out = m(input_ids=ids, input_features=frontend(waves, out_dtype=BF), labels=labels)
    out.loss.backward()
    m.arena.join_streams()
    torch.cuda.synchronize()
    loss = float(out.loss.detach())
    lg = out.logits[_labelled_rows(labels)].clone()
    del out
    res.update({"loss": loss, "loss_ref_fp32": loss32, "loss_ref_bf16": loss16, "loss_abs_err": abs(loss - loss32), "loss_abs_err_floor": abs(loss16 - loss32),
                "logits": _logit_stats(lg, lg32, floor_logits["max_abs_err"]), "logits_floor_ref_bf16": floor_logits})
    del lg, lg32
    params = dict(m.named_parameters())
    res["gradients"], bad = _score_gradients({k: p.grad for k, p in params.items() if p.requires_grad and p.grad is not None}, g32, floor_g, floor_sign, gn16,
                                             enc_layers, dec_layers)
    worst = res["gradients"]["worst"]

    if with_adamw:
        # ------------------------------------------------------------ first AdamW step: the update against what the fp32 gradients imply
        # step 1 of AdamW (bias-corrected m = g, v = g^2, no decay): delta = -lr * g / (|g| + eps)
        base = m.arena.params.storage_offset()
        before = opt.master.clone()
        sum_before = _sum64(m.arena.params)
        opt.step()
        torch.cuda.synchronize()
        upd_ok = upd_n = 0
        d_sum = d_sum_exp = 0.0
        rel_num = rel_den = 0.0
        for k, gr in g32.items():
            p = params[k]
            if not p.requires_grad or not p.is_contiguous():
                continue
            off = p.storage_offset() - base
            d = (opt.master[off: off + p.numel()] - before[off: off + p.numel()]).view(p.shape)
            exp = -lr * gr / (gr.abs() + 1e-8)
            upd_ok += int((torch.sign(d) == torch.sign(exp)).sum())
            upd_n += p.numel()
            d_sum += float(d.double().sum())
            d_sum_exp += float(exp.double().sum())
            rel_num += float((d - exp).double().square().sum())
            rel_den += float(exp.double().square().sum())
        res["adamw_first_step"] = {"lr": lr, "update_sign_agreement_with_fp32_gradients": upd_ok / max(upd_n, 1),
                                   "reference_bf16_gradient_sign_agreement_with_fp32": res["gradients"]["sign_agreement_floor"],
                                   "update_rel_l2_vs_fp32_implied": (rel_num / max(rel_den, 1e-300)) ** 0.5,
                                   "master_sum_delta": d_sum, "master_sum_delta_fp32_implied": d_sum_exp,
                                   "bf16_param_sum_before": sum_before, "bf16_param_sum_after": _sum64(m.arena.params),
                                   "note": "|delta| = lr for every element with |g| >> eps, so the update differs from the fp32-implied one exactly where a gradient "
                                           "SIGN differs (near-zero gradients): sign agreement is the meaningful figure, beside the reference-bf16 gradients' own"}
        del before
    log(f"[parity:{variant}] ours: loss {loss:.6f} (fp32 {loss32:.6f}, ref bf16 {loss16:.6f}); worst gradient {worst['name']} {worst['ours']:.4f} (floor {worst['floor']:.4f}); "
        f"{time.perf_counter() - t0:.1f} s")
    del m, opt, g32, params
    _free()

    lgs = res["logits"]
    ok = {"loss": res["loss_abs_err"] <= max(LOSS_ATOL, FLOOR_FACTOR * res["loss_abs_err_floor"]),
          "logits": lgs["max_abs_err"] <= max(lgs["abs_bar"], FLOOR_FACTOR * floor_logits["max_abs_err"]),
          "argmax": lgs["argmax_mismatches_on_confident_rows"] == 0,
          "gradients": not bad,
          "bucket_norms": res["gradients"]["bucket_norm_rel_err_max"] <= GRAD_REL_L2}
    if with_adamw:
        ok["adamw_update"] = res["adamw_first_step"]["update_sign_agreement_with_fp32_gradients"] >= res["adamw_first_step"]["reference_bf16_gradient_sign_agreement_with_fp32"] - 0.02
    if variant == "peaked":   # the teeth: the argmax must be DECIDED on >= 90 % of the rows (and equal on all of those), the q / k gradients ASSERTED
        ok["confident_rows_ge_90pct"] = lgs["confident_rows"] >= 0.9 * lgs["rows"]
        qk = res["gradients"]["qk_projection_tensors"]
        ok["qk_gradients_asserted"] = qk["noise_dominated"] <= 0.05 * max(qk["count"], 1)
    if long_windows:
        l5 = res["long5min_forward"]
        ok["long5min_loss"] = abs(l5["loss"] - l5["loss_ref_fp32"]) <= max(LOSS_ATOL, FLOOR_FACTOR * abs(l5["loss_ref_bf16"] - l5["loss_ref_fp32"]))
        ok["long5min_logits"] = l5["logits"]["max_abs_err"] <= max(l5["logits"]["abs_bar"], FLOOR_FACTOR * l5["logits_floor_ref_bf16"]["max_abs_err"])
        ok["long5min_argmax"] = l5["logits"]["argmax_mismatches_on_confident_rows"] == 0
    res["checks"] = ok
    res["green"] = all(ok.values())
    res["seconds"] = round(time.perf_counter() - t_start, 1)
    return res


def long_train_leg(dev, windows=10, variant="peaked", enc_layers=32, dec_layers=28, log=lambda s: print(s, file=sys.stderr, flush=True)):
    """BASELINE configs[4] shape WITH the backward (VERDICT r05 missing 4): one 5-minute clip (10 windows, S = 7 774), B = 1, forward + backward of
        the reference in fp32 with ITS activation checkpointing (gradient_checkpointing_enable: modeling_layers.py:79-114) = truth,
        the reference in bf16, same                                                                                    = floor,
        this repo's model under BOTH recompute plans ("full" = every layer, the reference's semantics; "budget" = only what does not fit 0.85 x HBM)
    -> loss, EVERY parameter gradient (rel-L2 vs fp32 beside the floor), every bucket norm, and that the two plans give bit-identical gradients."""
    import bench

    t_start = time.perf_counter()
    cfg = bench.af3_7b_config(enc_layers, dec_layers)
    waves, ids, labels = bench.synthetic_batch(1, 0, dev, windows)
    feats_ref, fmask = (t.to(dev) for t in _reference_features(waves.cpu().numpy()))
    ref, sd = _build_state(cfg, dev, variant)
    T = _reference_runs(ref, sd, ids, feats_ref, fmask, labels, 1, 1, True, log, f"long/{variant}")
    Fl = _floor_run(ref, sd, ids, feats_ref, fmask, labels, 1, T["g32"], log, f"long/{variant}")
    del ref
    _free()
    from audio_flamingo_amd.frontend import LogMelFrontend
    from audio_flamingo_amd.modeling import AudioFlamingo3ForConditionalGeneration as Mine

    m = Mine(cfg, device=dev, init_seed=0)
    m.load_state_dict(sd)
    del sd
    frontend = LogMelFrontend(dev)
    res = {"config": f"BASELINE configs[4] shape: one 5-minute clip = {windows} windows, S = {ids.shape[1]}, B = 1, forward + BACKWARD, activation checkpointing",
           "weight_set": variant, "loss_ref_fp32": T["loss32"], "loss_ref_bf16": Fl["loss16"], "plans": {}}
    keep = None
    bad_all = {}
    for pol in ("full", "budget"):
        m.gradient_checkpointing_enable(dict(policy=pol))
        m.zero_grad()
        out = m(input_ids=ids, input_features=frontend(waves, out_dtype=BF), labels=labels)
        out.loss.backward()
        m.arena.join_streams()
        torch.cuda.synchronize()
        loss = float(out.loss.detach())
        del out
        plan = {k: v for k, v in (m.ckpt_plan or {}).items() if not k.startswith("_")}
        named = {k: p.grad for k, p in m.named_parameters() if p.requires_grad and p.grad is not None}
        rec, bad = _score_gradients(named, T["g32"], Fl["floor_g"], Fl["floor_sign"], Fl["gn16"], enc_layers, dec_layers)
        same = None
        if keep is None:
            keep = m.arena.grads.clone()
        else:
            same = bool(torch.equal(keep, m.arena.grads))
        res["plans"][pol] = {"loss": loss, "loss_abs_err": abs(loss - T["loss32"]), "loss_abs_err_floor": abs(Fl["loss16"] - T["loss32"]), "layers_recomputed": plan,
                             "gradients": rec, "gradients_bit_identical_to_full_plan": same}
        bad_all.update({f"{pol}:{k}": v for k, v in bad.items()})
        m.gradient_checkpointing_disable()
        log(f"[parity:long/{variant}] ours ({pol}): loss {loss:.6f} (fp32 {T['loss32']:.6f}); worst {rec['worst']['name']} {rec['worst']['ours']:.4f} (floor {rec['worst']['floor']:.4f})")
    del m, keep, T, Fl
    _free()
    pl = res["plans"]
    ok = {"loss": all(p["loss_abs_err"] <= max(LOSS_ATOL, FLOOR_FACTOR * p["loss_abs_err_floor"]) for p in pl.values()),
          "gradients": not bad_all,
          "bucket_norms": all(p["gradients"]["bucket_norm_rel_err_max"] <= GRAD_REL_L2 for p in pl.values()),
          "tensors_ge_20": all(p["gradients"]["tensors"] >= 20 for p in pl.values()),
          "plans_bit_identical": pl["budget"]["gradients_bit_identical_to_full_plan"] is True}
    res["over_bar"] = bad_all
    res["checks"], res["green"] = ok, all(ok.values())
    res["seconds"] = round(time.perf_counter() - t_start, 1)
    return res


def run(dev, batch=8, micro_fp32=2, long_windows=10, lr=1e-5, enc_layers=32, dec_layers=28, log=lambda s: print(s, file=sys.stderr, flush=True),
        peaked=True, long_train=True):
    """the full record: the "init" weight set (round 5's record, unchanged layout, top level) + res["peaked_record"] (the second weight set, same checks plus
    >= 90 % decided rows and asserted q / k gradients) + res["long5min_train_record"] (configs[4] shape, forward + backward, both recompute plans)"""
    import bench

    cfg = bench.af3_7b_config(enc_layers, dec_layers)
    res = _leg(dev, cfg, "init", batch, micro_fp32, long_windows, lr, enc_layers, dec_layers, log)
    if peaked:
        try:
            res["peaked_record"] = _leg(dev, cfg, "peaked", batch, micro_fp32, 0, lr, enc_layers, dec_layers, log)
        except Exception as e:
            res["peaked_record"] = {"green": False, "error": repr(e)[:400], "checks": {"ran": False}}
        _free()
        res["checks"]["peaked_weight_set"] = bool(res["peaked_record"]["green"])
    if long_train and long_windows:
        try:
            res["long5min_train_record"] = long_train_leg(dev, long_windows, "peaked" if peaked else "init", enc_layers, dec_layers, log)
        except Exception as e:
            res["long5min_train_record"] = {"green": False, "error": repr(e)[:400], "checks": {"ran": False}}
        _free()
        res["checks"]["long5min_train"] = bool(res["long5min_train_record"]["green"])
    res["green"] = all(res["checks"].values())
    return res


def write_record(res, name="parity_fulldepth.json"):
    """the full record (every tensor) beside the bench line: gpurun_out/ (merged back by gpurun); best effort"""
    try:
        d = os.path.join(ROOT, "gpurun_out")
        os.makedirs(d, exist_ok=True)
        with open(os.path.join(d, name), "w") as f:
            json.dump(res, f, indent=1)
    except OSError:
        pass


def _brief_leg(r):
    """<= 300 bytes of a leg's record"""
    if "error" in r:
        return {"green": False, "error": r["error"][:120]}
    lg, g = r.get("logits", {}), r.get("gradients", {})
    out = {"green": r["green"], "failed_checks": [k for k, v in r["checks"].items() if not v]}
    if lg:
        out.update({"confident_rows": lg.get("confident_rows"), "rows": lg.get("rows"), "argmax_mismatches": lg.get("argmax_mismatches_on_confident_rows"),
                    "logits_rel_l2": round(lg.get("rel_l2", 0.0), 4)})
    if g:
        qk = g.get("qk_projection_tensors", {})
        out.update({"grad_ratio_max": round(g["ours_over_floor"]["max"], 3), "qk_asserted": f"{qk.get('asserted_against_the_fixed_or_2x_floor_bar')}/{qk.get('count')}"})
    ap = r.get("attention_peak_fp32_reference")
    if isinstance(ap, dict) and "decoder_layer0_mean_max_prob" in ap:
        out["attn_max_prob_dec_enc"] = [round(ap["decoder_layer0_mean_max_prob"], 3), round(ap["encoder_layer0_mean_max_prob"], 3)]
    return out


def summary(res):
    """the part of the record that rides in bench.py's detail file and (through bench.parity_brief) its JSON line; the full record - every tensor - goes to
    gpurun_out/ and profiles/"""
    g = res["gradients"]
    out = {k: res[k] for k in ("config", "weights", "truth", "floor", "bars", "loss", "loss_ref_fp32", "loss_ref_bf16", "loss_abs_err", "logits",
                               "logits_floor_ref_bf16", "logmel_max_abs_diff_vs_reference_frontend", "adamw_first_step", "attention_peak_fp32_reference",
                               "checks", "green", "seconds") if k in res}
    out["gradients"] = {k: g[k] for k in ("tensors", "worst", "median_rel_l2", "median_floor", "ours_over_floor", "over_bar", "spread", "qk_projection_tensors",
                                          "sign_agreement_with_fp32", "sign_agreement_floor", "bucket_norm_rel_err_max") if k in g}
    out["gradients"]["noise_dominated_count"] = len(g.get("noise_dominated_in_the_reference_bf16_run", {}))
    if "long5min_forward" in res:
        out["long5min_forward"] = res["long5min_forward"]
    if "peaked_record" in res:
        out["peaked"] = _brief_leg(res["peaked_record"])
    if "long5min_train_record" in res:
        r = res["long5min_train_record"]
        if "error" in r:
            out["long5min_train"] = {"green": False, "error": r["error"][:120]}
        else:
            out["long5min_train"] = {"green": r["green"], "failed_checks": [k for k, v in r["checks"].items() if not v],
                                     "loss_abs_err": {p: round(v["loss_abs_err"], 5) for p, v in r["plans"].items()},
                                     "grad_ratio_max": {p: round(v["gradients"]["ours_over_floor"]["max"], 3) for p, v in r["plans"].items()},
                                     "tensors": r["plans"]["full"]["gradients"]["tensors"], "plans_bit_identical": r["plans"]["budget"]["gradients_bit_identical_to_full_plan"]}
    return out


if __name__ == "__main__":
    import argparse

    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "gpurun_out", "parity_fulldepth.json"))
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--no-long", action="store_true")
    ap.add_argument("--enc-layers", type=int, default=32)
    ap.add_argument("--dec-layers", type=int, default=28)
    ap.add_argument("--no-peaked", action="store_true")
    ap.add_argument("--no-long-train", action="store_true")
    ap.add_argument("--only-peaked", action="store_true", help="calibration: the peaked weight set on the configs[1] batch only")
    a = ap.parse_args()
    if a.only_peaked:
        import bench

        r = _leg(torch.device("cuda", 0), bench.af3_7b_config(a.enc_layers, a.dec_layers), "peaked", a.batch, 2, 0, 1e-5, a.enc_layers, a.dec_layers,
                 lambda s_: print(s_, file=sys.stderr, flush=True))
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(r, f, indent=1)
        g_ = r["gradients"]
        print(json.dumps({"checks": r["checks"], "attention_peak": r["attention_peak_fp32_reference"], "logits": r["logits"], "ours_over_floor": g_["ours_over_floor"],
                          "qk": g_["qk_projection_tensors"], "noise_dominated": len(g_["noise_dominated_in_the_reference_bf16_run"]), "over_bar": g_["over_bar"]}))
        sys.exit(0)
    r = run(torch.device("cuda", 0), batch=a.batch, long_windows=0 if a.no_long else 10, enc_layers=a.enc_layers, dec_layers=a.dec_layers, peaked=not a.no_peaked,
            long_train=not a.no_long_train)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(r, f, indent=1)
    print(json.dumps(summary(r)))
    sys.exit(0 if r["green"] else 1)

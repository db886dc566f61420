"""What forward(labels=, return_token_logprobs=True) costs: a measurement, no assertion.

(1) The benchmark step of bench.py (AF3-7B, clip30: 8 samples x 1024 tokens, 256 answer tokens each -> 2 048 labelled rows; log-mel front end, forward,
    backward, AdamW bucket by bucket inside backward) through out.loss of the per-token route against the same step through the mean-CE loss route: same
    build, same process, same model and optimizer, the routes ALTERNATING step by step, median of --steps steps per route, spread = (max - min) / median.
    The per-token route recomputes the lm_head logits of the labelled rows in backward: 2 x 2048 x 152064 x 3584 = 2.2 TFLOP expected on top of the step.
(2) The two kernels of csrc/token_logprob.hip on a 4 096 x 152 064 bf16 chunk (HIP events, median of --kernel-reps launches) against the bytes they move -
    2 V per row read in the forward, 2 V read + 2 V written in the backward - with afk_ce_fwd_bwd on the same chunk as the yardstick.

    python tools/bench_token_logprobs.py [--steps 5] [--warmup 2] [--enc-layers 32] [--dec-layers 28] [--out result.json]
prints one JSON line and, with --out, also writes it to that file (profiles/token_logprobs.md is written from it).
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import bench  # noqa: E402  (the benchmark configuration and its synthetic batches; sets the hardware-queue count before HIP initialises)
import torch  # noqa: E402


def _summary(ms):
    med = statistics.median(ms)
    return {"median_ms": round(med, 3), "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3), "spread": round((max(ms) - min(ms)) / med, 4), "n": len(ms)}


def kernel_times(dev, rows=4096, V=152064, reps=9):
    from audio_flamingo_amd import ops

    g = torch.Generator(device=dev).manual_seed(0)
    src = (torch.randn((rows, V), device=dev, generator=g) * 3.0).to(torch.bfloat16)
    labels = torch.randint(0, V, (rows,), device=dev, generator=g)
    buf = torch.empty_like(src)
    logp, lse, ent, row_loss = (torch.empty(rows, device=dev) for _ in range(4))
    u = torch.randn(rows, device=dev, generator=g)
    denom = ops.count_valid(labels)
    ops.token_logprob(src, labels, logp, lse)   # the lse the backward launches read

    def timed(fn, restore):
        ms = []
        for _ in range(reps + 1):
            if restore:
                buf.copy_(src)
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            ms.append(a.elapsed_time(b))
        return ms[1:]   # the first launch loads the code object

    legs = {
        "token_logprob": (lambda: ops.token_logprob(buf, labels, logp, lse), 2 * V),
        "token_logprob_entropy": (lambda: ops.token_logprob(buf, labels, logp, lse, ent), 2 * V),
        "token_logprob_bwd": (lambda: ops.token_logprob_bwd_(buf, labels, lse, u), 4 * V),
        "ce_fwd_bwd_nograd": (lambda: ops.ce_fwd_bwd_(buf, labels, row_loss, denom, write_grad=False), 2 * V),
        "ce_fwd_bwd": (lambda: ops.ce_fwd_bwd_(buf, labels, row_loss, denom, write_grad=True), 4 * V),
    }
    out = {"rows": rows, "V": V}
    for name, (fn, bytes_per_row) in legs.items():
        s = _summary(timed(fn, True))
        s["bytes_moved"] = rows * bytes_per_row
        s["tb_per_s"] = round(rows * bytes_per_row / (s["median_ms"] * 1e-3) / 1e12, 3)
        out[name] = s
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--enc-layers", type=int, default=32)
    ap.add_argument("--dec-layers", type=int, default=28)
    ap.add_argument("--kernel-reps", type=int, default=9)
    ap.add_argument("--no-step", action="store_true", help="only the kernel times")
    ap.add_argument("--out", default="", help="also write the JSON record to this file")
    args = ap.parse_args()
    from audio_flamingo_amd import functional as F_
    from audio_flamingo_amd.arena import FusedAdamW
    from audio_flamingo_amd.dp import BackwardOverlap
    from audio_flamingo_amd.frontend import LogMelFrontend
    from audio_flamingo_amd.modeling import AudioFlamingo3ForConditionalGeneration

    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    res = {"tool": "bench_token_logprobs", "kernels": kernel_times(dev, reps=args.kernel_reps)}
    if not args.no_step:
        model = AudioFlamingo3ForConditionalGeneration(bench.af3_7b_config(args.enc_layers, args.dec_layers), device=dev, init_seed=0)
        model.check_placeholders = False
        model.label_rows_static = True
        opt = FusedAdamW(model.arena, lr=1e-5, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0)
        opt.sync_master()
        overlap = BackwardOverlap(model.arena, opt, None)
        model.arena.lazy_T_shadows = F_.BWD_FORM == "direct"
        model.arena.refresh_shadows(force=True)
        model.arena.enable_wgrad_stream(True)
        frontend = LogMelFrontend(dev)
        nb = 2 * (args.warmup + args.steps)
        pool = [bench.synthetic_batch(args.batch, k * args.batch, dev, 1) for k in range(nb)]
        waves, ids, labels = (t.clone() for t in pool[0])
        n = [0]

        def step(per_token):
            w_, i_, l_ = pool[n[0] % nb]
            waves.copy_(w_), ids.copy_(i_), labels.copy_(l_)
            n[0] += 1
            feats = frontend(waves, out_dtype=torch.bfloat16)
            model.arena.zero_grad()
            overlap.begin_step()
            out = model(input_ids=ids, input_features=feats, labels=labels, **(dict(return_token_logprobs=True) if per_token else {}))
            out.loss.backward()
            overlap.finish()
            return out.loss

        times, losses = {False: [], True: []}, {False: [], True: []}
        for k in range(args.warmup + args.steps):
            for per_token in (False, True):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                loss = step(per_token)
                torch.cuda.synchronize()
                if k >= args.warmup:
                    times[per_token].append((time.perf_counter() - t0) * 1e3)
                    losses[per_token].append(round(float(loss.detach()), 4))
        a, b = _summary(times[False]), _summary(times[True])
        rows = int((labels[:, 1:] != -100).sum())
        tflop = 2.0 * rows * model.V * model.H / 1e12
        extra = b["median_ms"] - a["median_ms"]
        res["step"] = {"config": f"AF3-7B enc {args.enc_layers} dec {args.dec_layers}, batch {args.batch} x {ids.shape[1]} tokens, {rows} labelled rows",
                       "loss_route": a, "token_logprob_route": b, "extra_ms": round(extra, 2), "recompute_tflop": round(tflop, 3),
                       "recompute_pflops_if_all_extra": round(tflop / max(extra, 1e-9), 3) if extra > 0 else None,
                       "losses_loss_route": losses[False], "losses_token_logprob_route": losses[True],
                       "peak_allocated_gib": round(torch.cuda.max_memory_allocated(dev) / 2 ** 30, 1)}
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()

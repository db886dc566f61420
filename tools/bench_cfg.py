"""Classifier-free guidance in the decode graph: afk_decode_cfg (csrc/decode_cfg.hip) alone, and generate(guidance_scale=...) against the plain steps and
against the hook route (the reference's UnbatchedClassifierFreeGuidanceLogitsProcessor around this model as a logits_processor).

  python tools/bench_cfg.py kernel [out.json]   V = 152 064 (the AF3 vocabulary), B = 1 and 8: ops.decode_cfg in place on the conditional rows - both launches -
        next to a plain device copy of the same three rows (cond, uncond, out: [3, B, V] fp32 -> another buffer, one torch copy), the bound the kernel is held
        against.  Each form is captured into a HIP graph of NSET calls that rotate over NSET distinct buffer sets, so the host's enqueue cost is in neither
        time; REPEATS alternating repeats, device events around ~0.2 s of replays each; median us per call, spread (max - min) / median, the ratio.
  python tools/bench_cfg.py generate7b [out.json]   the AF3-7B geometry of bench.py (random init) behind a 7 500-position audio prompt (9 + 7 500 <sound> + 9
        ids), B = 1, greedy, a 22-id negative prompt: the guided call (graph), the plain call, the plain call on two copies of the prompt (the batched B = 2
        step) and the hook route (eager by construction).  Per route: time to the first token (max_new_tokens = 1), ms per token ((time of NEW tokens - time
        of 1) / (NEW - 1)), wall clock around a synchronise, medians of REPEATS alternating repeats with the spread, and the peak of torch's allocator over the
        NEW-token call minus what was resident before it (weights, inputs)."""
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from audio_flamingo_amd import _lib, ops

dev = torch.device("cuda")
REPEATS, NSET = int(os.environ.get("REPEATS", "5")), int(os.environ.get("NSET", "28"))


def _graph_of(fn, calls):
    """fn(0) .. fn(calls - 1) captured into one HIP graph (every call warmed eagerly first)"""
    for i in range(calls):
        fn(i)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for i in range(calls):
            fn(i)
    g.replay()
    torch.cuda.synchronize()
    return g


def _timed(g, replays, calls):
    """us per call over `replays` replays of a graph of `calls` calls"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(replays):
        g.replay()
    e1.record()
    torch.cuda.synchronize()
    return 1e3 * e0.elapsed_time(e1) / (replays * calls)


def kernel_leg():
    V, rows = int(os.environ.get("V", "152064")), []
    gen = torch.Generator(device=dev).manual_seed(0)
    for B in [int(x) for x in os.environ.get("B_LIST", "1,8").split(",")]:
        src = [torch.randn((3, B, V), device=dev, generator=gen) * 8 for _ in range(NSET)]   # [cond, uncond, out] of one step
        dst = [torch.empty_like(s) for s in src]
        ws = ops.decode_cfg_workspace(B, V, dev)

        def cfg(i):
            ops.decode_cfg(src[i % NSET][0], src[i % NSET][1], 3.0, out=src[i % NSET][2], ws=ws)

        def copy(i):
            dst[i % NSET].copy_(src[i % NSET])

        variants = [("copy of the three rows", copy), ("afk_decode_cfg", cfg)]
        graphs = [(name, _graph_of(fn, NSET)) for name, fn in variants]
        replays = max(2, min(4000, int(2e5 / max(_timed(graphs[1][1], 2, NSET), 1.0) / NSET)))   # ~0.2 s of the kernel per repeat
        times = {name: [] for name, _ in variants}
        for _ in range(REPEATS):
            for name, g_ in graphs:   # alternating: every variant once per repeat
                times[name].append(_timed(g_, replays, NSET))
        row = {"B": B, "V": V, "iters": replays * NSET, "buffer_sets": NSET, "row_bytes": 4 * V, "kernel_bytes_read_written": [4 * B * V * 4, B * V * 4],
               "copy_bytes_read_written": [3 * B * V * 4, 3 * B * V * 4], "build": _lib.load().afk_build_id().decode()}
        for name, ts in times.items():
            med = statistics.median(ts)
            row[name] = {"us": round(med, 2), "spread": round((max(ts) - min(ts)) / med, 3)}
        row["kernel_over_copy"] = round(row["afk_decode_cfg"]["us"] / row["copy of the three rows"]["us"], 2)
        rows.append(row)
        print(json.dumps(row), flush=True)
        del src, dst, graphs
    return rows


def generate7b_leg():
    from transformers import LogitsProcessorList, UnbatchedClassifierFreeGuidanceLogitsProcessor

    import bench
    from audio_flamingo_amd.frontend import LogMelFrontend
    from audio_flamingo_amd.modeling import AudioFlamingo3ForConditionalGeneration as Model

    new, windows, scale = int(os.environ.get("NEW", "33")), int(os.environ.get("WINDOWS", "10")), 3.0
    model = Model(bench.af3_7b_config(), device=dev, init_seed=0)
    model.check_placeholders = False
    waves, ids, _ = bench.synthetic_batch(1, 0, dev, windows)
    ids = ids[:, : 9 + bench.N_AUDIO_TOK * windows + 9]
    feats = LogMelFrontend(dev)(waves, out_dtype=torch.bfloat16)
    del waves
    text = ids[:, ids[0] != model.audio_token_id]
    neg = torch.cat([text, (torch.arange(22 - text.shape[1], device=dev)[None] + 100).to(text.dtype)], 1) if text.shape[1] < 22 else text[:, :22]
    ids2, feats2 = ids.repeat(2, 1), feats.repeat(2, *([1] * (feats.dim() - 1)))
    hook = lambda: LogitsProcessorList([UnbatchedClassifierFreeGuidanceLogitsProcessor(scale, model, neg)])   # a fresh one per call: it keeps its cache
    routes = {"guided (graph)": lambda n: model.generate(ids, input_features=feats, max_new_tokens=n, guidance_scale=scale, negative_prompt_ids=neg),
              "plain B = 1": lambda n: model.generate(ids, input_features=feats, max_new_tokens=n),
              "plain batched B = 2": lambda n: model.generate(ids2, input_features=feats2, max_new_tokens=n),
              "hook route (eager)": lambda n: model.generate(ids, input_features=feats, max_new_tokens=n, logits_processor=hook())}
    res = {"model": "AF3-7B geometry, random init", "prompt_rows": int(ids.shape[1]), "negative_rows": int(neg.shape[1]), "new_tokens": new, "repeats": REPEATS,
           "scale": scale, "build": _lib.load().afk_build_id().decode(), "routes": {}}

    def run(fn, n_new, record=None):
        torch.cuda.empty_cache()   # the graph capture inside generate() empties the caching allocator: outside the timed window for every route
        torch.cuda.synchronize()
        if record is not None:
            torch.cuda.reset_peak_memory_stats()
            before = torch.cuda.memory_allocated()
        t0 = time.perf_counter()
        out = fn(n_new)
        torch.cuda.synchronize()
        dt = 1e3 * (time.perf_counter() - t0)
        if record is not None:
            record["peak_mib_over_resident"] = round((torch.cuda.max_memory_allocated() - before) / 2 ** 20, 1)
            record["full_length"] = int(out.shape[1]) == int(ids.shape[1]) + n_new
        return dt

    rows = {name: {} for name in routes}
    for name, fn in routes.items():   # warm both shapes, then one recorded call
        run(fn, 1), run(fn, new)
        run(fn, new, record=rows[name])
        if name.startswith("guided"):
            rows[name]["cfg_stats"] = model.last_cfg_stats
    first, step = {name: [] for name in routes}, {name: [] for name in routes}
    names = list(routes)
    for rep_ in range(REPEATS):
        for name in (names if rep_ % 2 else names[::-1]):
            t1, tn = run(routes[name], 1), run(routes[name], new)
            first[name].append(t1)
            step[name].append((tn - t1) / (new - 1))
    for name in routes:
        f, s_ = statistics.median(first[name]), statistics.median(step[name])
        rows[name].update(first_token_ms=round(f, 1), first_token_spread=round((max(first[name]) - min(first[name])) / f, 3),
                          ms_per_token=round(s_, 3), ms_per_token_spread=round((max(step[name]) - min(step[name])) / s_, 3))
        res["routes"][name] = rows[name]
        print(json.dumps({name: rows[name]}), flush=True)
    return res


if __name__ == "__main__":
    leg = sys.argv[1] if len(sys.argv) > 1 else "kernel"
    result = {"kernel": kernel_leg, "generate7b": generate7b_leg}[leg]()
    if len(sys.argv) > 2:
        os.makedirs(os.path.dirname(os.path.abspath(sys.argv[2])), exist_ok=True)
        with open(sys.argv[2], "w") as f:
            json.dump(result, f, indent=1)

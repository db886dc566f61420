"""FP8 decode weights (generate(decode_weights="fp8"), decode_w8.py) against the bf16 route of the same build, in one process.

  python tools/bench_decode_w8.py speed [out.json]     the AF3-7B geometry of bench.py (random init), one sequence, greedy, graph replay, text-only prompts of
        CONTEXTS (default 256,15000) ids: per context and route the time to the first token (max_new_tokens = 1) and ms per token ((time of NEW tokens - time
        of 1) / (NEW - 1)), wall clock around a synchronise, medians of REPEATS alternating repeats with the spread (max - min) / median, and fp8 / bf16.
        The FP8 copy is built before the timed calls (last_w8_stats is reported).
  python tools/bench_decode_w8.py profile               one bf16 and one fp8 call of NEW tokens behind a 256-id prompt - the program a
        `rocprofv3 --kernel-trace --stats` run wraps (tools/prof_decode_w8.sh)
  python tools/bench_decode_w8.py table <trace.db> [out.md]   the per-launch table of the five Linears from that trace: calls, average us, the bytes the launch
        must stream (weights as stored + the row scales), achieved TB/s, and fp8 / bf16 per Linear
  python tools/bench_decode_w8.py quant_error [out.json]   the UNSNAPPED trained tiny golden (tests/golden, case A): the fp8 route against the bf16 route over the
        golden's greedy run - max |delta logit| in units of tests/_tol.py's logit bar, and the steps whose argmax differs (reported, not asserted)
  python tools/bench_decode_w8.py batched [out.json]   decode_weights_batched: the same geometry, graph replay, both routes alternating in one process - batches of
        B = 2, 4, 8 prompts of 256 ids (ms per step, the method of `speed`) and prompt-lookup decoding with k = 3 and 7 (ms per verify step: the time of NEW
        tokens minus the time of 1, over the steps the call enqueued)
  python tools/bench_decode_w8.py batched_profile       one bf16 and one fp8 call of NEW tokens at B = 8 - the program of a `rocprofv3 --kernel-trace --stats` run
  python tools/bench_decode_w8.py batched_table <trace.db> [out.md]   the per-launch table of the four matrix-pipe Linears (five per layer: o_proj and down share a
        kernel) from that trace
  python tools/bench_decode_w8.py batched_quant_error [out.json]   quant_error for a batch of the golden prompt twice"""
import json
import os
import re
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

REPEATS, NEW = int(os.environ.get("REPEATS", "5")), int(os.environ.get("NEW", "65"))
# the five Linears of the AF3-7B decode step: (N, K), and how gemv_chain_kernel<PRO, EPI, S, R, W8> names them at the default knobs
H, NQ, NK, I, V = 3584, 3584, 512, 18944, 152064
LINEARS = {"qkv": (NQ + 2 * NK, H, (1, 0)), "o_proj": (H, NQ, (0, 1)), "gate_up": (2 * I, H, (1, 2)), "down_proj": (H, I, (0, 1)), "lm_head": (V, H, (1, 3))}
PER_TOKEN = {"qkv": 28, "o_proj": 28, "gate_up": 28, "down_proj": 28, "lm_head": 1}


def linear_bytes(name, fp8):
    N, K, _ = LINEARS[name]
    return N * K + 4 * N if fp8 else 2 * N * K


def _model7b():
    import torch

    import bench
    from audio_flamingo_amd.modeling import AudioFlamingo3ForConditionalGeneration as Model

    model = Model(bench.af3_7b_config(), device=torch.device("cuda"), init_seed=0)
    model.check_placeholders = False
    return model


def _prompt(n, dev):
    import torch

    return torch.randint(0, 1000, (1, n), generator=torch.Generator().manual_seed(n)).to(dev)


def speed_leg():
    import torch

    from audio_flamingo_amd import _lib

    model = _model7b()
    dev = model.device_
    contexts = [int(x) for x in os.environ.get("CONTEXTS", "256,15000").split(",")]
    res = {"model": "AF3-7B geometry, random init", "new_tokens": NEW, "repeats": REPEATS, "build": _lib.load().afk_build_id().decode(),
           "chain_knobs": {k: os.environ.get(k) for k in ("AFK_CHAIN_S", "AFK_CHAIN_R")}, "contexts": {}}
    t0 = time.perf_counter()
    model.quantize_decode_weights()
    torch.cuda.synchronize()
    res["quantize_s"] = round(time.perf_counter() - t0, 2)

    def run(ids, n_new, **kw):
        torch.cuda.empty_cache()   # the graph capture inside generate() empties the caching allocator: outside the timed window for every route
        torch.cuda.synchronize()
        t = time.perf_counter()
        out = model.generate(ids, max_new_tokens=n_new, **kw)
        torch.cuda.synchronize()
        assert out.shape[1] == ids.shape[1] + n_new
        return 1e3 * (time.perf_counter() - t)

    routes = {"bf16": {}, "fp8": dict(decode_weights="fp8")}
    for n in contexts:
        ids = _prompt(n, dev)
        for kw in routes.values():   # warm both shapes of both routes
            run(ids, 1, **kw), run(ids, NEW, **kw)
        assert model.last_w8_stats is not None and model.last_w8_stats["rebuilt"] is False   # the fp8 route ran last, on the copy built above
        res["w8_stats"] = model.last_w8_stats
        first, step = {r: [] for r in routes}, {r: [] for r in routes}
        names = list(routes)
        for rep in range(REPEATS):
            for r in (names if rep % 2 else names[::-1]):   # alternating
                t1, tn = run(ids, 1, **routes[r]), run(ids, NEW, **routes[r])
                first[r].append(t1)
                step[r].append((tn - t1) / (NEW - 1))
        row = {}
        for r in routes:
            f, s = statistics.median(first[r]), statistics.median(step[r])
            row[r] = dict(first_token_ms=round(f, 1), ms_per_token=round(s, 4), ms_per_token_spread=round((max(step[r]) - min(step[r])) / s, 4),
                          ms_per_token_all=[round(x, 4) for x in step[r]])
        row["fp8_over_bf16"] = round(row["fp8"]["ms_per_token"] / row["bf16"]["ms_per_token"], 4)
        res["contexts"][str(n)] = row
        print(json.dumps({n: row}), flush=True)
    res["weight_bytes_per_token"] = {r: sum(PER_TOKEN[k] * linear_bytes(k, r == "fp8") for k in LINEARS) for r in routes}
    return res


def batched_leg():
    import torch

    from audio_flamingo_amd import _lib

    model = _model7b()
    dev = model.device_
    res = {"model": "AF3-7B geometry, random init", "new_tokens": NEW, "repeats": REPEATS, "build": _lib.load().afk_build_id().decode(), "context": 256, "settings": {}}
    model.quantize_decode_weights()
    torch.cuda.synchronize()
    routes = {"bf16": {}, "fp8": dict(decode_weights="fp8", decode_weights_batched=True)}

    def run(ids, n_new, **kw):   # -> (ms, decode steps the call enqueued)
        torch.cuda.empty_cache()
        torch.cuda.synchronize()
        t = time.perf_counter()
        model.generate(ids, max_new_tokens=n_new, **kw)
        torch.cuda.synchronize()
        ms = 1e3 * (time.perf_counter() - t)
        return ms, (model.last_lookup_stats["launched"] if "prompt_lookup_num_tokens" in kw else n_new - 1)

    settings = [(f"B={B}", _prompt(256, dev).repeat(B, 1), {}) for B in (2, 4, 8)]
    settings += [(f"lookup k={k}", _prompt(256, dev), dict(prompt_lookup_num_tokens=k)) for k in (3, 7)]
    for tag, ids, extra in settings:
        for kw in routes.values():   # warm both shapes of both routes
            run(ids, 1, **kw, **extra), run(ids, NEW, **kw, **extra)
        assert model.last_w8_stats is not None and model.last_w8_stats["rebuilt"] is False
        step = {r: [] for r in routes}
        names = list(routes)
        for rep in range(REPEATS):
            for r in (names if rep % 2 else names[::-1]):   # alternating
                (t1, _), (tn, steps) = run(ids, 1, **routes[r], **extra), run(ids, NEW, **routes[r], **extra)
                step[r].append((tn - t1) / max(steps, 1))
        row = {}
        for r in routes:
            s = statistics.median(step[r])
            row[r] = dict(ms_per_step=round(s, 4), spread=round((max(step[r]) - min(step[r])) / s, 4), all=[round(x, 4) for x in step[r]])
        row["fp8_over_bf16"] = round(row["fp8"]["ms_per_step"] / row["bf16"]["ms_per_step"], 4)
        res["settings"][tag] = row
        print(json.dumps({tag: row}), flush=True)
    res["weight_bytes_per_step"] = {r: sum(PER_TOKEN[k] * linear_bytes(k, r == "fp8") for k in LINEARS) for r in routes}
    return res


def batched_profile_leg():
    import torch

    model = _model7b()
    ids = _prompt(256, model.device_).repeat(8, 1)
    for kw in ({}, dict(decode_weights="fp8", decode_weights_batched=True)):
        model.generate(ids, max_new_tokens=NEW, **kw)
        torch.cuda.synchronize()
    return {}


def batched_table_leg(db_path, out_path=None):
    """gemv_chain_mfma_kernel<EPI, S, RG, PRO(, W8)>: qkv <0, 8, 32, 1>, o_proj and down <1, 8, 16, 2> (told apart by their time: down streams 5.3 x the bytes),
    gate|up <2, 4, 32, 1>, lm_head <3, 4, 32, 1>"""
    import sqlite3

    con = sqlite3.connect(db_path)
    tabs = [r[0] for r in con.execute("select name from sqlite_master where type in ('table', 'view')")]
    view = "kernels" if "kernels" in tabs else next(t for t in tabs if t.startswith("kernels"))
    rows = con.execute(f"select name, start, end from {view}").fetchall()
    agg = {}
    for name, s, e in rows:
        m = re.search(r"gemv_chain_mfma_kernel<(\d+), (\d+), (\d+), (\d+)(?:, (true|false|0|1))?>", name)
        if not m:
            continue
        epi, fp8 = int(m.group(1)), m.group(5) in ("true", "1")
        agg.setdefault(({0: "qkv", 1: "resid", 2: "gate_up", 3: "lm_head"}[epi], fp8), []).append((e - s) / 1e3)
    for fp8 in (False, True):   # the two Linear + residual launches of a layer alternate o_proj, down: split the sorted times in the middle
        d = sorted(agg.pop(("resid", fp8), []))
        if d:
            agg[("o_proj", fp8)], agg[("down_proj", fp8)] = d[:len(d) // 2], d[len(d) // 2:]
    lines = ["| Linear | N x K | route | launches | avg us | median us | bytes streamed | TB/s (avg) | fp8 / bf16 (avg us) |", "|---|---|---|---|---|---|---|---|---|"]
    per_step = {False: 0.0, True: 0.0}
    for which in LINEARS:
        N, K, _ = LINEARS[which]
        avg = {}
        for fp8 in (False, True):
            d = agg.get((which, fp8))
            if not d:
                continue
            avg[fp8] = sum(d) / len(d)
            per_step[fp8] += PER_TOKEN[which] * avg[fp8]
            b = linear_bytes(which, fp8)
            ratio = f"{avg[True] / avg[False]:.3f}" if fp8 and False in avg else ""
            lines.append(f"| {which} | {N} x {K} | {'fp8' if fp8 else 'bf16'} | {len(d)} | {avg[fp8]:.2f} | {statistics.median(d):.2f} | {b} | {b / avg[fp8] / 1e6:.2f} | {ratio} |")
    lines.append("")
    lines.append(f"the five Linears per step (28 layers + lm_head, serial sum of average kernel times): bf16 {per_step[False] / 1e3:.3f} ms, fp8 {per_step[True] / 1e3:.3f} ms")
    out = "\n".join(lines)
    print(out)
    if out_path:
        open(out_path, "w").write(out + "\n")
    return {}


def batched_quant_error_leg():
    import torch

    from tests._tol import logit_tol
    from tests.test_model_gpu import N_GEN
    from tests.test_sampler_gpu import _case_a

    m, p, audio = _case_a(torch.device("cuda:0"))
    p2, audio2 = p.repeat(2, 1), {k: v.repeat(2, *([1] * (v.dim() - 1))) for k, v in audio.items()}
    kw = dict(audio2, max_new_tokens=N_GEN, return_dict_in_generate=True, output_logits=True)
    ref, got = m.generate(p2, **kw), m.generate(p2, decode_weights="fp8", decode_weights_batched=True, **kw)
    S0 = p.shape[1]
    differ = (ref.sequences[:, S0:] != got.sequences[:, S0:]).any(0).nonzero().flatten().tolist()
    parted = differ[0] if differ else None
    steps = N_GEN if parted is None else parted + 1
    worst, argmax_differs = 0.0, 0
    for t in range(steps):
        r, g = ref.logits[t].float(), got.logits[t].float()
        worst = max(worst, float((g - r).abs().max()) / logit_tol(float(r.abs().max())))
        argmax_differs += int((r.argmax(-1) != g.argmax(-1)).any())
    res = dict(model="trained tiny golden, case A twice, unsnapped", rows=2, steps_compared=steps, ids_part_at=parted,
               max_abs_dlogit_over_logit_tol=round(worst, 3), steps_whose_argmax_differs=argmax_differs, w8_stats=m.last_w8_stats)
    print(json.dumps(res))
    return res


def profile_leg():
    import torch

    model = _model7b()
    ids = _prompt(256, model.device_)
    for kw in ({}, dict(decode_weights="fp8")):
        model.generate(ids, max_new_tokens=NEW, **kw)
        torch.cuda.synchronize()
    return {}


def table_leg(db_path, out_path=None):
    import sqlite3

    rows = sqlite3.connect(db_path).cursor().execute("select name, start, end from kernels").fetchall()
    agg = {}
    for name, s, e in rows:
        m = re.search(r"gemv_chain_kernel<(\d+), (\d+), (\d+), (\d+)(?:, (true|false|0|1))?>", name)
        if not m:
            continue
        pro, epi, S = int(m.group(1)), int(m.group(2)), int(m.group(3))
        fp8 = m.group(5) in ("true", "1")
        which = {(1, 0): "qkv", (1, 2): "gate_up", (1, 3): "lm_head"}.get((pro, epi)) or ("down_proj" if S == 8 else "o_proj")   # K > 4096 runs eight waves per group
        agg.setdefault((which, fp8), []).append((e - s) / 1e3)
    lines = ["| Linear | N x K | route | launches | avg us | median us | bytes streamed | TB/s (avg) | fp8 / bf16 (avg us) |", "|---|---|---|---|---|---|---|---|---|"]
    per_token = {False: 0.0, True: 0.0}
    for which in LINEARS:
        N, K, _ = LINEARS[which]
        avg = {}
        for fp8 in (False, True):
            d = agg.get((which, fp8))
            if not d:
                continue
            avg[fp8] = sum(d) / len(d)
            per_token[fp8] += PER_TOKEN[which] * avg[fp8]
            b = linear_bytes(which, fp8)
            ratio = f"{avg[True] / avg[False]:.3f}" if fp8 and False in avg else ""
            lines.append(f"| {which} | {N} x {K} | {'fp8' if fp8 else 'bf16'} | {len(d)} | {avg[fp8]:.2f} | {statistics.median(d):.2f} | {b} | {b / avg[fp8] / 1e6:.2f} | {ratio} |")
    lines.append("")
    lines.append(f"the five Linears per token (28 layers + lm_head, serial sum of average kernel times): bf16 {per_token[False] / 1e3:.3f} ms, fp8 {per_token[True] / 1e3:.3f} ms")
    out = "\n".join(lines)
    print(out)
    if out_path:
        open(out_path, "w").write(out + "\n")
    return {}


def quant_error_leg():
    import torch

    from tests._tol import logit_tol
    from tests.test_model_gpu import G, N_GEN
    from tests.test_sampler_gpu import _case_a

    m, p, audio = _case_a(torch.device("cuda:0"))
    gold = torch.load(os.path.join(G, "tiny64_caseA.pt"))["generate"][0, -N_GEN:]
    kw = dict(audio, max_new_tokens=N_GEN, return_dict_in_generate=True, output_logits=True)
    ref, got = m.generate(p, **kw), m.generate(p, decode_weights="fp8", **kw)
    a, b = ref.sequences[0, p.shape[1]:].tolist(), got.sequences[0, p.shape[1]:].tolist()
    parted = next((t for t in range(N_GEN) if a[t] != b[t]), None)
    steps = N_GEN if parted is None else parted + 1   # behind a step at which the ids part the two calls condition on different ids
    worst, argmax_differs = 0.0, 0
    for t in range(steps):
        r, g = ref.logits[t].float(), got.logits[t].float()
        worst = max(worst, float((g - r).abs().max()) / logit_tol(float(r.abs().max())))
        argmax_differs += int(r.argmax()) != int(g.argmax())
    res = dict(model="trained tiny golden, case A, unsnapped", steps_compared=steps, ids_part_at=parted, bf16_ids_equal_golden=a == gold.tolist(),
               max_abs_dlogit_over_logit_tol=round(worst, 3), steps_whose_argmax_differs=argmax_differs, w8_stats=m.last_w8_stats)
    print(json.dumps(res))
    return res


if __name__ == "__main__":
    leg = sys.argv[1] if len(sys.argv) > 1 else "speed"
    if leg == "table":
        table_leg(*sys.argv[2:4])
    elif leg == "batched_table":
        batched_table_leg(*sys.argv[2:4])
    else:
        result = {"speed": speed_leg, "profile": profile_leg, "quant_error": quant_error_leg, "batched": batched_leg, "batched_profile": batched_profile_leg,
                  "batched_quant_error": batched_quant_error_leg}[leg]()
        if len(sys.argv) > 2:
            os.makedirs(os.path.dirname(os.path.abspath(sys.argv[2])), exist_ok=True)
            with open(sys.argv[2], "w") as f:
                json.dump(result, f, indent=1)

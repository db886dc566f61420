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
        golden's greedy run - max |delta logit| in units of tests/_tol.py's logit bar, and the steps whose argmax differs (reported, not asserted)"""
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
    else:
        result = {"speed": speed_leg, "profile": profile_leg, "quant_error": quant_error_leg}[leg]()
        if len(sys.argv) > 2:
            os.makedirs(os.path.dirname(os.path.abspath(sys.argv[2])), exist_ok=True)
            with open(sys.argv[2], "w") as f:
                json.dump(result, f, indent=1)

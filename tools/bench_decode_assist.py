"""Assisted decoding (generate(assistant_model=, num_assistant_tokens=), decode_assist.py) against the plain greedy route of the same build, in one process.

  python tools/bench_decode_assist.py speed [out.json]   the AF3-7B geometry of bench.py (random init), one sequence, greedy, graph replay, text-only prompts of
        CONTEXTS (default 256,15000) ids.  Routes, alternating inside every repeat:
          plain          ms per token = (time of NEW tokens - time of 1) / (NEW - 1): the baseline, whose launches are the parent's
          assist k       for k in KS (default 3,5,7), with an assistant of Qwen2.5-0.5B geometry (24 layers, hidden 896, intermediate 4 864, 14 / 2 heads of 64,
                         the target's vocabulary; random init): ms per STEP = (time of NEW tokens - time of 1) / steps enqueued (last_assist_stats["launched"]:
                         a step costs the same whatever it accepts - its launches and their shapes do not depend on the drafts; the divisor therefore
                         counts the up to seven replays behind `done` too, which run the same launches).  The call of 1 token holds both prefills, so they
                         cancel; behind 15 000 keys they are the larger part of both terms, so read the spread column and raise NEW if it is large.
          self k         the target as its own assistant (SELF_K, default 3): every draft that the target's batched verify rows confirm is accepted, so the
                         measured ms per token of this row checks the arithmetic of the derived columns
        wall clock around a synchronise, medians of REPEATS (default 5) with the spread (max - min) / median.
        Random weights accept almost nothing, so next to each step cost stand ms per token at per-draft acceptance rates 0, 0.5, 0.8 and 1 DERIVED from it:
        a step emits (1 - a^(k + 1)) / (1 - a) tokens in expectation (k + 1 at a = 1) when every draft is accepted independently with probability a.
  python tools/bench_decode_assist.py table <speed.json> [out.md]   the tables of profiles/assist_decode.md from that file"""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

REPEATS, NEW = int(os.environ.get("REPEATS", "5")), int(os.environ.get("NEW", "65"))
RATES = (0.0, 0.5, 0.8, 1.0)


def tokens_per_step(a, k):
    """expected tokens a step emits when each of its k drafts is accepted independently with probability a: the accepted prefix plus one"""
    return float(k + 1) if a >= 1.0 else (1.0 - a ** (k + 1)) / (1.0 - a)


def _models():
    import torch
    from transformers import AudioFlamingo3Config

    import bench
    from audio_flamingo_amd.modeling import AudioFlamingo3ForConditionalGeneration as Model

    cfg = bench.af3_7b_config()
    target = Model(cfg, device=torch.device("cuda"), init_seed=0)
    tc = dict(vocab_size=cfg.text_config.vocab_size, hidden_size=896, intermediate_size=4864, num_hidden_layers=24, num_attention_heads=14, num_key_value_heads=2,
              max_position_embeddings=32768, rms_norm_eps=1e-6, rope_parameters=dict(rope_theta=1000000.0, rope_type="default"))
    small = AudioFlamingo3Config(audio_config=cfg.audio_config.to_dict(), text_config=tc, audio_token_id=cfg.audio_token_id)
    draft = Model(small, device=torch.device("cuda"), init_seed=1)
    for m in (target, draft):
        m.check_placeholders = False
    return target, draft


def _prompt(n, dev):
    import torch

    return torch.randint(0, 1000, (1, n), generator=torch.Generator().manual_seed(n)).to(dev)


def speed_leg():
    import torch

    from audio_flamingo_amd import _lib

    target, draft = _models()
    dev = target.device_
    contexts = [int(x) for x in os.environ.get("CONTEXTS", "256,15000").split(",")]
    ks = [int(x) for x in os.environ.get("KS", "3,5,7").split(",")]
    self_k = int(os.environ.get("SELF_K", "3"))
    res = {"model": "AF3-7B geometry, random init", "assistant": "Qwen2.5-0.5B geometry (24 layers, hidden 896, intermediate 4864, 14 / 2 heads of 64), random init",
           "new_tokens": NEW, "repeats": REPEATS, "build": _lib.load().afk_build_id().decode(), "contexts": {}}

    def run(ids, n_new, **kw):
        torch.cuda.empty_cache()   # the graph capture inside generate() empties the caching allocator: outside the timed window for every route
        torch.cuda.synchronize()
        t = time.perf_counter()
        out = target.generate(ids, max_new_tokens=n_new, **kw)
        torch.cuda.synchronize()
        assert out.shape[1] == ids.shape[1] + n_new
        return 1e3 * (time.perf_counter() - t), target.last_assist_stats

    routes = {"plain": {}}
    routes.update({f"assist k={k}": dict(assistant_model=draft, num_assistant_tokens=k) for k in ks})
    routes[f"self k={self_k}"] = dict(assistant_model=target, num_assistant_tokens=self_k)
    for n in contexts:
        ids = _prompt(n, dev)
        for kw in routes.values():   # warm both shapes of every route
            run(ids, 1, **kw), run(ids, NEW, **kw)
        per = {r: dict(token=[], step=[], stats=None) for r in routes}
        names = list(routes)
        for rep in range(REPEATS):
            for r in (names if rep % 2 else names[::-1]):   # alternating
                (t1, _), (tn, s) = run(ids, 1, **routes[r]), run(ids, NEW, **routes[r])
                per[r]["token"].append((tn - t1) / (NEW - 1))
                if s is not None:
                    per[r]["step"].append((tn - t1) / s["launched"])
                    per[r]["stats"] = s
        row = {}
        for r in routes:
            tok = statistics.median(per[r]["token"])
            row[r] = dict(ms_per_token=round(tok, 4), ms_per_token_spread=round((max(per[r]["token"]) - min(per[r]["token"])) / tok, 4),
                          ms_per_token_all=[round(x, 4) for x in per[r]["token"]])
            if per[r]["step"]:
                st, k = statistics.median(per[r]["step"]), routes[r]["num_assistant_tokens"]
                row[r].update(k=k, ms_per_step=round(st, 4), ms_per_step_spread=round((max(per[r]["step"]) - min(per[r]["step"])) / st, 4),
                              ms_per_step_all=[round(x, 4) for x in per[r]["step"]], stats=per[r]["stats"],
                              derived_ms_per_token={str(a): round(st / tokens_per_step(a, k), 4) for a in RATES})
        res["contexts"][str(n)] = row
        print(json.dumps({n: row}), flush=True)
    return res


def table_leg(src, out_path=None):
    with open(src) as f:
        res = json.load(f)
    lines = [f"build {res['build']}; {res['model']}; assistant: {res['assistant']}; {res['new_tokens']} new tokens per call, medians of {res['repeats']} "
             f"alternating repeats, spread = (max - min) / median.  ms per step = (t({res['new_tokens']} tokens) - t(1 token)) / steps enqueued; the steps "
             f"enqueued include the up to seven replays behind the end of the call, which run the same launches.  The four a = columns are DERIVED from the step "
             f"cost: ms per step / ((1 - a^(k + 1)) / (1 - a)) tokens per step (k + 1 at a = 1); only `ms per token measured` is a measurement.", ""]
    for n, row in res["contexts"].items():
        plain = row["plain"]
        lines += [f"### {n} cached keys", "",
                  f"plain greedy: {plain['ms_per_token']:.3f} ms per token (spread {100 * plain['ms_per_token_spread']:.1f} %; repeats "
                  f"{' / '.join(f'{x:.3f}' for x in plain['ms_per_token_all'])})", "",
                  "| route | ms per step (median of the repeats) | spread | steps enqueued / open, tokens, accepted | ms per token measured | derived: a = 0 | a = 0.5 | a = 0.8 | a = 1 | "
                  "break-even tokens per step |", "|---|---|---|---|---|---|---|---|---|---|"]
        for r, v in row.items():
            if r == "plain":
                continue
            s, d = v["stats"], v["derived_ms_per_token"]
            lines.append(f"| {r} | {v['ms_per_step']:.3f} | {100 * v['ms_per_step_spread']:.1f} % | {s['launched']} / {s['steps']}, {s['emitted']}, {s['accepted']} | "
                         f"{v['ms_per_token']:.3f} | {d['0.0']:.3f} | {d['0.5']:.3f} | {d['0.8']:.3f} | {d['1.0']:.3f} | {v['ms_per_step'] / plain['ms_per_token']:.2f} |")
        lines.append("")
    out = "\n".join(lines)
    print(out)
    if out_path:
        with open(out_path, "w") as f:
            f.write(out + "\n")
    return {}


if __name__ == "__main__":
    leg = sys.argv[1] if len(sys.argv) > 1 else "speed"
    if leg == "table":
        table_leg(*sys.argv[2:4])
    else:
        result = speed_leg()
        if len(sys.argv) > 2:
            os.makedirs(os.path.dirname(os.path.abspath(sys.argv[2])), exist_ok=True)
            with open(sys.argv[2], "w") as f:
                json.dump(result, f, indent=1)

"""Cost of a prompt-lookup decoding step against a plain greedy step (results: profiles/lookup_decode.md).

  python tools/bench_lookup.py [--ks 1,3,7,15] [--new N] [--repeats R]
      generate() on the AF3-7B geometry of tools/bench_decode.py, random weights, one sequence, the benchmark's prompt:
        plain    ms per step of plain greedy decoding = (t(N new tokens) - t(1 new token)) / (N - 1)
        k = ...  ms per verify step of generate(prompt_lookup_num_tokens=k) = (t(N) - t(1)) / steps enqueued (last_lookup_stats["launched"]); a step costs the
                 same whatever it accepts - the launches and their shapes do not depend on it
      ratio = verify step / plain step: the number of tokens a step has to emit on average to break even.
      The legs alternate inside a repeat.  tokens_per_step only shows what the run did: a random-weight model soon repeats itself, so its drafts get accepted,
      which says nothing about a trained model on real prompts - an acceptance rate is a property of a workload, and none is measured here.  same_ids: random
      weights leave near-ties that the batched and the single-row launches break differently; the id equality is tested on the trained tiny model.
One JSON line."""
import argparse
import json
import os
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--ks", default="1,3,7,15")
ap.add_argument("--new", type=int, default=65)
ap.add_argument("--repeats", type=int, default=3)
args = ap.parse_args()
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

if not torch.cuda.is_available():
    sys.exit("bench_lookup: needs a GPU (no CPU fallback, nothing is measured without one)")
dev = torch.device("cuda")


def main():
    import bench
    from audio_flamingo_amd.frontend import LogMelFrontend
    from audio_flamingo_amd.modeling import AudioFlamingo3ForConditionalGeneration as Model

    model = Model(bench.af3_7b_config(), device=dev, init_seed=0)
    model.check_placeholders = False
    waves, ids, _ = bench.synthetic_batch(1, 0, dev)
    ids = ids[:, : 9 + 750 + 9]
    feats = LogMelFrontend(dev)(waves, out_dtype=torch.bfloat16)
    ks = [int(k) for k in args.ks.split(",")]
    legs = ["plain"] + [f"k={k}" for k in ks]
    kw = {"plain": {}, **{f"k={k}": dict(prompt_lookup_num_tokens=k) for k in ks}}

    def run(leg, new):
        """-> (seconds, steps enqueued, the ids)"""
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = model.generate(ids, input_features=feats, max_new_tokens=new, **kw[leg])
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        return dt, (new - 1 if leg == "plain" else model.last_lookup_stats["launched"]), out

    res = dict(new=args.new, prompt=ids.shape[1], ms_per_step={leg: [] for leg in legs}, same_ids={}, steps={}, tokens_per_step={})
    plain = None
    for leg in legs:   # warm both shapes of every leg
        run(leg, 1)
        _, steps, out = run(leg, args.new)
        plain = out if leg == "plain" else plain
        res["same_ids"][leg] = bool(out.shape == plain.shape and torch.equal(out, plain))
        res["steps"][leg] = steps
        res["tokens_per_step"][leg] = round((args.new - 1) / max(steps if leg == "plain" else model.last_lookup_stats["steps"], 1), 3)
    for _ in range(args.repeats):
        for leg in legs:
            t1, _, _ = run(leg, 1)
            tn, steps, _ = run(leg, args.new)
            res["ms_per_step"][leg].append(round(1e3 * (tn - t1) / max(steps, 1), 4))
    med = {leg: sorted(v)[len(v) // 2] for leg, v in res["ms_per_step"].items()}
    res["median_ms_per_step"] = med
    res["break_even_tokens_per_step"] = {leg: round(med[leg] / med["plain"], 3) for leg in legs if leg != "plain"}
    print(json.dumps(res))


main()

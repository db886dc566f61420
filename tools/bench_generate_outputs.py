"""Cost of generate(return_dict_in_generate=True, output_scores / output_logits) per decode step (results: profiles/generate_outputs.md).

  python tools/bench_generate_outputs.py [--batches 1,8] [--legs greedy,sampled] [--new N] [--repeats R] [--configs off,logits,scores,both,hook]

generate() ms per decode step on the AF3-7B geometry of tools/bench_decode.py: (t(N new tokens) - t(1 new token)) / (N - 1), host clock around work that
ends in a device synchronise.  Configurations:
  off      the plain call (no flag): the captured step of the parent commit
  logits   return_dict_in_generate + output_logits: one afk_decode_record launch per step
  scores   return_dict_in_generate + output_scores: greedy one record launch, sampled none (the sampler's own launch writes the row)
  both     all three flags
  hook     the only route to the same rows without the flags: a recording logits_processor, which forces the eager hook loop
Every (batch, leg, configuration) is warmed at both lengths; inside a repeat the configurations alternate, so a drift of the machine hits all of them; the
repeats show the run-to-run spread.  The clocks are whatever the device's power management gives an unprivileged process (nothing is pinned).
One JSON line per invocation."""
import argparse
import json
import os
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--batches", default="1,8")
ap.add_argument("--legs", default="greedy,sampled")
ap.add_argument("--configs", default="off,logits,scores,both,hook")
ap.add_argument("--new", type=int, default=65)
ap.add_argument("--repeats", type=int, default=5)
args = ap.parse_args()
sys.path.insert(0, os.path.abspath(args.tree))
import torch  # noqa: E402

if not torch.cuda.is_available():
    sys.exit("bench_generate_outputs: needs a GPU (no CPU fallback, nothing is measured without one)")
dev = torch.device("cuda")


class Recorder:
    """what a user had to write before the flags existed: clone the row every step"""

    def __init__(self):
        self.rows = []

    def __call__(self, input_ids, scores):
        self.rows.append(scores.clone())
        return scores


def main():
    import bench
    from transformers import LogitsProcessorList

    from audio_flamingo_amd.frontend import LogMelFrontend
    from audio_flamingo_amd.modeling import AudioFlamingo3ForConditionalGeneration as Model

    model = Model(bench.af3_7b_config(), device=dev, init_seed=0)
    model.check_placeholders = False
    legs = {"greedy": {}, "sampled": dict(do_sample=True, temperature=0.7, top_k=50, top_p=0.9, seed=1)}
    on = dict(return_dict_in_generate=True)
    configs = {"off": lambda: {}, "logits": lambda: dict(on, output_logits=True), "scores": lambda: dict(on, output_scores=True),
               "both": lambda: dict(on, output_logits=True, output_scores=True), "hook": lambda: dict(logits_processor=LogitsProcessorList([Recorder()]))}
    res = dict(tree=os.path.abspath(args.tree), new=args.new, repeats=args.repeats, vocab=int(model.V), ms_per_step={})
    for B in (int(b) for b in args.batches.split(",")):
        waves, ids, _ = bench.synthetic_batch(B, 0, dev)
        ids = ids[:, : 9 + 750 + 9]
        feats = LogMelFrontend(dev)(waves, out_dtype=torch.bfloat16)

        def run(leg, cfg, new):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = model.generate(ids, input_features=feats, max_new_tokens=new, **legs[leg], **configs[cfg]())
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            del out
            return dt

        for leg in args.legs.split(","):
            names = args.configs.split(",")
            for cfg in names:
                run(leg, cfg, 1), run(leg, cfg, args.new)      # warm both lengths of every configuration
            t = {cfg: [] for cfg in names}
            for _ in range(args.repeats):                     # the configurations alternate inside a repeat
                for cfg in names:
                    t[cfg].append(round(1e3 * (run(leg, cfg, args.new) - run(leg, cfg, 1)) / (args.new - 1), 4))
            res["ms_per_step"][f"B{B}/{leg}"] = t
    print(json.dumps(res))


main()

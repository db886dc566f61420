"""Beam search in the decode graph against the host loop it replaces (results: profiles/beam_decode.md).

  python tools/bench_beam_decode.py [--batches 1,8] [--beams 4] [--new 33] [--repeats 3]
      generate(num_beams=4) ms per generated token on the AF3-7B geometry of bench.py's decode leg (random init, prompt of 9 + 750 <sound> + 9 ids, no eos id:
      every call runs its full length): (t(N new tokens) - t(1 new token)) / (N - 1), host clock around a device synchronise, both shapes warmed first.
        device   the step's decisions and the cache move as launches of the captured step (afk_beam_step / afk_beam_reorder_cache)
        host     the loop of torch ops: log_softmax / topk / gather over [B, nb * V], one host synchronisation and one index_select copy of the whole
                 cache per token - the code of the commit before this route existed, selected with beam_on_device = False
      Same process, same model, the two routes alternating inside a repeat.  Peak memory of a route: torch's max_memory_allocated over one N-token call minus
      what was allocated before it (weights, inputs).
One JSON line."""
import argparse
import json
import os
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--batches", default="1,8")
ap.add_argument("--beams", type=int, default=4)
ap.add_argument("--new", type=int, default=33)
ap.add_argument("--repeats", type=int, default=3)
args = ap.parse_args()
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

if not torch.cuda.is_available():
    sys.exit("bench_beam_decode: needs a GPU (no CPU fallback, nothing is measured without one)")
dev = torch.device("cuda")

import bench  # noqa: E402
from audio_flamingo_amd.frontend import LogMelFrontend  # noqa: E402
from audio_flamingo_amd.modeling import AudioFlamingo3ForConditionalGeneration as Model  # noqa: E402

model = Model(bench.af3_7b_config(), device=dev, init_seed=0)
model.check_placeholders = False
res = dict(beams=args.beams, new=args.new, rows=[])
for B in [int(b) for b in args.batches.split(",")]:
    waves, ids, _ = bench.synthetic_batch(B, 0, dev)
    ids = ids[:, : 9 + 750 + 9]
    feats = LogMelFrontend(dev)(waves, out_dtype=torch.bfloat16)
    outs, peak = {}, {}

    def run(route, new, record=False):
        model.beam_on_device = route == "device"
        torch.cuda.synchronize()
        if record:
            torch.cuda.reset_peak_memory_stats()
            before = torch.cuda.memory_allocated()
        t0 = time.perf_counter()
        out = model.generate(ids, input_features=feats, max_new_tokens=new, num_beams=args.beams)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        if record:
            peak[route] = round((torch.cuda.max_memory_allocated() - before) / 2 ** 20, 1)
            outs[route] = out
        return dt

    row = dict(B=B, cache_rows=B * args.beams, prompt=int(ids.shape[1]), ms_per_token={"device": [], "host": []})
    for route in ("device", "host"):
        run(route, 1), run(route, args.new)      # warm both shapes
        run(route, args.new, record=True)
    for _ in range(args.repeats):                  # the routes alternate inside a repeat
        for route in ("device", "host"):
            row["ms_per_token"][route].append(round(1e3 * (run(route, args.new) - run(route, 1)) / (args.new - 1), 4))
    row["peak_mib_over_resident"] = peak
    row["full_length"] = {r: int(o.shape[1]) == int(ids.shape[1]) + args.new for r, o in outs.items()}
    row["same_ids"] = bool(outs["device"].shape == outs["host"].shape and torch.equal(outs["device"], outs["host"]))
    res["rows"].append(row)
    del waves, feats
    torch.cuda.empty_cache()
print(json.dumps(res))

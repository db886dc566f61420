"""Cost of sampled token selection (results: profiles/decode_sampling.md).

  python tools/bench_decode_sample.py kernel
      per-launch time of afk_decode_sample by device events at V = 152 064, B in {1, 8, 32}, (top_k, top_p) in {(50, 1), (50, 0.9), (0, 0.9)},
      against the torch chain of modeling._select_token on the same logits, alternating in this process; three rounds -> the spread.
  python tools/bench_decode_sample.py generate [--tree DIR] [--batch B] [--legs greedy,sampled] [--new N] [--repeats R]
      generate() ms/token on the AF3-7B geometry of tools/bench_decode.py: (t(N new tokens) - t(1 new token)) / (N - 1).  --tree: the checkout whose package
      is measured (default: this one) - run one process per checkout, alternating, to compare two builds (e.g. the commit before device sampling, whose
      do_sample steps are eager with selection in torch).
  python tools/bench_decode_sample.py warpers [--lib PATH] [--rounds R]
      per-launch time of the sampler at V = 152 064, B = 1, temperature 0.7, top-k 50 + top-p 0.9: afk_decode_sample as it is, then - where the library
      exports afk_decode_sample_filtered - that entry with the four filters off, with min_p / typical_p / epsilon_cutoff / eta_cutoff added one at a time, and
      with all four.  The library is loaded by path through ctypes (--lib: another build of the same header's afk_decode_sample, e.g. the parent commit's), so
      one process measures one build: run the processes alternating to compare two.  Each round is the median of --launches single launches between device
      events; the rounds show the spread (results: profiles/decode_sampling_warpers.md).
  generate --legs sampled,min_p adds min_p = 0.05 to the sampled leg.
One JSON line per invocation."""
import argparse
import json
import os
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("mode", choices=["kernel", "generate", "warpers"])
ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--batch", type=int, default=1)
ap.add_argument("--legs", default="greedy,sampled")
ap.add_argument("--new", type=int, default=65)
ap.add_argument("--repeats", type=int, default=3)
ap.add_argument("--window", type=float, default=0.5, help="kernel mode: seconds per timed window")
ap.add_argument("--lib", default=None, help="warpers mode: the libafk.so to measure (default: this tree's)")
ap.add_argument("--rounds", type=int, default=5, help="warpers mode: medians per case")
ap.add_argument("--launches", type=int, default=400, help="warpers mode: launches per median")
args = ap.parse_args()
sys.path.insert(0, os.path.abspath(args.tree))
import torch  # noqa: E402

if not torch.cuda.is_available():
    sys.exit("bench_decode_sample: needs a GPU (no CPU fallback, nothing is measured without one)")
dev = torch.device("cuda")


def timed(fn, n):
    """-> microseconds per call over n calls between two device events"""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    b.synchronize()
    return 1e3 * a.elapsed_time(b) / n


def kernel_mode():
    from audio_flamingo_amd import ops
    from audio_flamingo_amd.modeling import AudioFlamingo3ForConditionalGeneration as Model

    V, rows = 152064, []
    for B in (1, 8, 32):
        g = torch.Generator().manual_seed(B)
        x = (torch.randn(B, V, generator=g) * 4.0).to(torch.bfloat16).float().to(dev)      # bf16-valued, as the lm_head writes them
        out = torch.empty(B, device=dev, dtype=torch.int64)
        step = torch.zeros(1, device=dev, dtype=torch.int32)
        gen = torch.Generator(device=dev)
        gen.manual_seed(1)
        for k, p in ((50, 1.0), (50, 0.9), (0, 0.9)):
            ours = lambda: ops.decode_sample(x, temperature=0.7, top_k=k, top_p=p, seed=1, step_base=step, out=out)
            chain = lambda: Model._select_token(x, dict(temperature=0.7, top_k=k, top_p=p, generator=gen))
            n = {}
            for name, fn in (("ours", ours), ("torch", chain)):       # warm the shape, then size the window
                timed(fn, 5)
                n[name] = max(20, int(args.window * 1e6 / timed(fn, 20)))
            t = {"ours": [], "torch": []}
            for _ in range(3):
                for name, fn in (("ours", ours), ("torch", chain)):
                    t[name].append(round(timed(fn, n[name]), 2))
            rows.append(dict(B=B, top_k=k, top_p=p, iters=n, ours_us=t["ours"], torch_us=t["torch"]))
    print(json.dumps(dict(mode="kernel", V=V, temperature=0.7, rows=rows)))


def generate_mode():
    import bench
    from audio_flamingo_amd.frontend import LogMelFrontend
    from audio_flamingo_amd.modeling import AudioFlamingo3ForConditionalGeneration as Model

    B = args.batch
    model = Model(bench.af3_7b_config(), device=dev, init_seed=0)
    model.check_placeholders = False
    waves, ids, _ = bench.synthetic_batch(B, 0, dev)
    ids = ids[:, : 9 + 750 + 9]
    feats = LogMelFrontend(dev)(waves, out_dtype=torch.bfloat16)
    kw = {"greedy": {}, "sampled": dict(do_sample=True, temperature=0.7, top_k=50, top_p=0.9, seed=1)}
    kw["min_p"] = dict(kw["sampled"], min_p=0.05)
    res = dict(mode="generate", tree=os.path.abspath(args.tree), batch=B, new=args.new, legs={})

    def run(leg, new):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        model.generate(ids, input_features=feats, max_new_tokens=new, **kw[leg])
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    legs = args.legs.split(",")
    for leg in legs:
        run(leg, 1), run(leg, args.new)      # warm both shapes
    for leg in legs:
        res["legs"][leg] = []
    for _ in range(args.repeats):            # legs alternate inside a repeat
        for leg in legs:
            res["legs"][leg].append(round(1e3 * (run(leg, args.new) - run(leg, 1)) / (args.new - 1), 4))
    print(json.dumps(res))


def warpers_mode():
    import ctypes
    import statistics

    from audio_flamingo_amd import _lib

    path = os.path.abspath(args.lib or _lib.LIB_PATH)
    lib, protos = ctypes.CDLL(path), _lib.parse_header()
    V = 152064
    x = (torch.randn(1, V, generator=torch.Generator().manual_seed(1)) * 4.0).to(torch.bfloat16).float().to(dev)      # bf16-valued, as the lm_head writes them
    out = torch.empty(1, device=dev, dtype=torch.int64)
    step = torch.zeros(1, device=dev, dtype=torch.int32)
    stream = torch.cuda.current_stream().cuda_stream
    head = (x.data_ptr(), x.stride(0), 1, V, 0.7, 50, 0.9)
    tail = (None, 1, step.data_ptr(), 0, out.data_ptr(), None, 0, None, None, 0, None, None, 0, 0, None, stream)
    off = dict(min_p=0.0, typical_p=1.0, epsilon_cutoff=0.0, eta_cutoff=0.0)
    on = dict(min_p=0.05, typical_p=0.9, epsilon_cutoff=3e-4, eta_cutoff=3e-4)
    cases = [("afk_decode_sample", None)]
    if hasattr(lib, "afk_decode_sample_filtered"):
        cases += [("filtered, all off", off)] + [("+ " + k, dict(off, **{k: v})) for k, v in on.items()] + [("+ all four", on)]
    for name in ("afk_decode_sample", "afk_decode_sample_filtered"):
        if hasattr(lib, name):
            getattr(lib, name).restype, getattr(lib, name).argtypes = protos[name][0], protos[name][1]

    def launch(f):
        rc = lib.afk_decode_sample(*head, *tail) if f is None else lib.afk_decode_sample_filtered(*head, *(f[k] for k in off), *tail)
        if rc != 0:
            sys.exit(f"bench_decode_sample: launch failed ({rc})")

    def median_us(f):
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(args.launches)]
        for a, b in ev:
            a.record()
            launch(f)
            b.record()
        torch.cuda.synchronize()
        return round(1e3 * statistics.median(a.elapsed_time(b) for a, b in ev), 2)

    t = {name: [] for name, _ in cases}
    for _, f in cases:
        for _ in range(20):
            launch(f)
    for _ in range(args.rounds):             # the cases alternate inside a round
        for name, f in cases:
            t[name].append(median_us(f))
    print(json.dumps(dict(mode="warpers", lib=path, V=V, B=1, temperature=0.7, top_k=50, top_p=0.9, filters=on, launches=args.launches, median_us=t)))


{"kernel": kernel_mode, "generate": generate_mode, "warpers": warpers_mode}[args.mode]()

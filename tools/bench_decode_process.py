"""Cost of the logits processors in the decode graph (results: profiles/decode_processors.md).

  python tools/bench_decode_process.py kernel
      per-launch time of afk_decode_process by device events at V = 152 064, history 768 + 64 ids: B in {1, 8}, penalty alone / with a 3-gram ban, and
      B = 1 with the greedy selection block; the time of restoring the inputs in front of every launch is measured alone and
      subtracted; three rounds -> the spread.
  python tools/bench_decode_process.py generate [--tree DIR] [--legs greedy,penalty,hooks] [--new N] [--repeats R]
      generate() ms/token on the AF3-7B geometry of tools/bench_decode.py, one sequence: (t(N new tokens) - t(1 new token)) / (N - 1).
        greedy   plain greedy decoding
        penalty  generate(repetition_penalty=1.05): the device path inside the captured step
        hooks    generate(logits_processor=[RepetitionPenaltyLogitsProcessor(1.05)]): the same ids through eager steps with host code between them
      --tree: the checkout whose package is measured (default: this one) - one process per checkout, alternating, to compare two builds (the commit before
      this feature has no `penalty` leg).
One JSON line per invocation."""
import argparse
import json
import os
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("mode", choices=["kernel", "generate"])
ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--legs", default="greedy,penalty,hooks")
ap.add_argument("--new", type=int, default=129)
ap.add_argument("--repeats", type=int, default=3)
ap.add_argument("--window", type=float, default=0.5, help="kernel mode: seconds per timed window")
args = ap.parse_args()
sys.path.insert(0, os.path.abspath(args.tree))
import torch  # noqa: E402

if not torch.cuda.is_available():
    sys.exit("bench_decode_process: needs a GPU (no CPU fallback, nothing is measured without one)")
dev = torch.device("cuda")
PENALTY = 1.05


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
    from audio_flamingo_amd import decode_process as P

    V, S0, H, rows = 152064, 768, 3584, []
    emb = torch.zeros((V, H), device=dev, dtype=torch.bfloat16)
    for B, g, select in ((1, 0, False), (1, 3, False), (1, 0, True), (8, 0, False), (8, 3, False)):
        gen = torch.Generator().manual_seed(B)
        x = (torch.randn(B, V, generator=gen) * 4.0).to(torch.bfloat16).float().to(dev)      # bf16-valued, as the lm_head writes them
        ids = torch.randint(0, V, (B, S0), generator=gen).to(dev)
        ids[:, 9:759] = 151669                                                                # the <sound> run of an AF3 prompt
        ps = P.build_state(P.ProcessSpec(penalty=PENALTY, ngram=g), ids, 64, V)
        nxt = torch.randint(0, V, (B,), generator=gen).to(dev)
        kw = {}
        if select:   # the state is advanced by every launch: a private copy whose slot the timed launches never read (step_base stays fixed)
            kw = dict(select=True, state=torch.tensor([0, S0 + 1, S0, S0], device=dev, dtype=torch.int32), emb=emb, x_out=torch.empty(H, device=dev, dtype=torch.bfloat16))
            nxt = nxt.clone()
        step = torch.full((1,), 63, device=dev, dtype=torch.int32)
        x0, nxt0 = x.clone(), nxt.clone()

        def restore():   # the launch edits the row in place (and, selecting, the token it appends next): every timed launch sees the same inputs
            x.copy_(x0), nxt.copy_(nxt0)

        def fn():
            restore()
            P.apply(ps, x, next_token=nxt, step_base=step, **kw)

        timed(fn, 5)
        n = max(20, int(args.window * 1e6 / timed(fn, 20)))
        both, alone = [timed(fn, n) for _ in range(3)], [timed(restore, n) for _ in range(3)]
        rows.append(dict(B=B, ngram=g, select=select, iters=n, restore_us=[round(v, 2) for v in alone], us=[round(u - v, 2) for u, v in zip(both, alone)]))
    print(json.dumps(dict(mode="kernel", V=V, history=S0 + 63, penalty=PENALTY, rows=rows)))


def generate_mode():
    import bench
    from audio_flamingo_amd.frontend import LogMelFrontend
    from audio_flamingo_amd.modeling import AudioFlamingo3ForConditionalGeneration as Model
    from transformers import LogitsProcessorList, RepetitionPenaltyLogitsProcessor

    model = Model(bench.af3_7b_config(), device=dev, init_seed=0)
    model.check_placeholders = False
    waves, ids, _ = bench.synthetic_batch(1, 0, dev)
    ids = ids[:, : 9 + 750 + 9]
    feats = LogMelFrontend(dev)(waves, out_dtype=torch.bfloat16)
    kw = {"greedy": {}, "penalty": dict(repetition_penalty=PENALTY),
          "hooks": dict(logits_processor=LogitsProcessorList([RepetitionPenaltyLogitsProcessor(PENALTY)]))}
    res = dict(mode="generate", tree=os.path.abspath(args.tree), new=args.new, legs={}, same_ids={})

    def run(leg, new, keep=None):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = model.generate(ids, input_features=feats, max_new_tokens=new, **kw[leg])
        torch.cuda.synchronize()
        if keep is not None:
            keep[leg] = out
        return time.perf_counter() - t0

    legs, outs = args.legs.split(","), {}
    for leg in legs:
        run(leg, 1), run(leg, args.new, outs)      # warm both shapes
    if "penalty" in outs and "hooks" in outs:      # the two ways to the same result
        res["same_ids"]["penalty_vs_hooks"] = bool(outs["penalty"].shape == outs["hooks"].shape and torch.equal(outs["penalty"], outs["hooks"]))
    if "greedy" in outs and "hooks" in outs:
        res["same_ids"]["hooks_differs_from_greedy"] = not (outs["greedy"].shape == outs["hooks"].shape and torch.equal(outs["greedy"], outs["hooks"]))
    for leg in legs:
        res["legs"][leg] = []
    for _ in range(args.repeats):                  # legs alternate inside a repeat
        for leg in legs:
            res["legs"][leg].append(round(1e3 * (run(leg, args.new) - run(leg, 1)) / (args.new - 1), 4))
    print(json.dumps(res))


kernel_mode() if args.mode == "kernel" else generate_mode()

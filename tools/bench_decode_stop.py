"""Cost of the stopping rule in the decode graph (results: profiles/decode_stop.md).

  python tools/bench_decode_stop.py kernel
      per-launch time of afk_decode_stop by device events, prompt of 768 ids + 64 emitted: B in {1, 8}, two eos ids alone / with three stop strings (ids that
      touch no string, and rows that end in the last four of the five ids of a match), on rows that never finish (every launch judges every row; nothing it
      writes changes, so no input has to be restored); three rounds -> the spread.
  python tools/bench_decode_stop.py generate [--tree DIR] [--legs greedy,eos_list,stop_strings] [--new N] [--repeats R]
      generate() ms/token on the AF3-7B geometry of tools/bench_decode.py, one sequence: (t(N new tokens) - t(1 new token)) / (N - 1).
        greedy        plain greedy decoding (no eos id: nothing of the stopping rule is enqueued)
        eos_list      generate(eos_token_id=[a, b]): the device route, eos ids the run never emits
        stop_strings  the same plus stop_strings=["\\n\\n", "</s>", "User:"] and an in-memory byte-level tokenizer (256 byte tokens and the whole strings as tokens;
                      the model's other ids take the table's dummy row, as ids of a real vocabulary that touch no stop string do)
      Every leg has to run its full N tokens (reported as full_length) or its figure is not comparable.
      --tree: the checkout whose package is measured (default: this one) - one process per checkout, alternating, to compare two builds (the commit before
      this feature has only the `greedy` leg).
One JSON line per invocation."""
import argparse
import json
import os
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("mode", choices=["kernel", "generate"])
ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--legs", default="greedy,eos_list,stop_strings")
ap.add_argument("--new", type=int, default=129)
ap.add_argument("--repeats", type=int, default=3)
ap.add_argument("--window", type=float, default=0.5, help="kernel mode: seconds per timed window")
args = ap.parse_args()
sys.path.insert(0, os.path.abspath(args.tree))
import torch  # noqa: E402

if not torch.cuda.is_available():
    sys.exit("bench_decode_stop: needs a GPU (no CPU fallback, nothing is measured without one)")
dev = torch.device("cuda")
STRINGS = ["\n\n", "</s>", "User:"]
V = 152064


def byte_tokenizer():
    """256 byte tokens at ids 0 .. 255, then the stop strings themselves and two fragments as tokens"""
    from tokenizers import Tokenizer, decoders, models, pre_tokenizers
    from transformers import PreTrainedTokenizerFast
    from transformers.convert_slow_tokenizer import bytes_to_unicode

    m = bytes_to_unicode()
    vocab = {m[b]: b for b in range(256)}
    for piece in STRINGS + ["User", "er:", "</"]:
        vocab["".join(m[b] for b in piece.encode())] = len(vocab)
    tok = Tokenizer(models.BPE(vocab=vocab, merges=[]))
    tok.pre_tokenizer = pre_tokenizers.ByteLevel(add_prefix_space=False, use_regex=False)
    tok.decoder = decoders.ByteLevel()
    return PreTrainedTokenizerFast(tokenizer_object=tok)


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
    from audio_flamingo_amd import decode_stop as D

    S0, rows = 768, []
    table = D.build_table(byte_tokenizer(), STRINGS)
    for B, strings, partial in ((1, False, False), (1, True, False), (1, True, True), (8, False, False), (8, True, False), (8, True, True)):
        gen = torch.Generator().manual_seed(B)
        ids = torch.randint(300, V - 2, (B, S0), generator=gen).to(dev)     # ids that touch no stop string, and neither eos id
        spec = D.StopSpec(eos=(V - 1, V - 2), pad=V - 1, stop_strings=tuple(STRINGS) if strings else ())
        ss = D.build_state(spec, ids, 64, table if strings else None)
        nxt = torch.randint(300, V - 2, (B,), generator=gen).to(dev)
        step = torch.full((1,), 63, device=dev, dtype=torch.int32)
        ss["ids"][:, S0:] = torch.randint(300, V - 2, (B, 64), generator=gen).to(dev)
        if partial:   # the byte tokens s, e, r in front of ":" and no U in front of them: every row walks the "User:" recurrence four ids deep and does not finish
            ss["ids"][:, S0 + 60:S0 + 63] = torch.tensor([ord(c) for c in "ser"], device=dev, dtype=torch.int32)
            nxt.fill_(ord(":"))

        def fn():
            D.apply(ss, nxt, step_base=step, feed_pad=B > 1)

        timed(fn, 5)
        n = max(20, int(args.window * 1e6 / timed(fn, 20)))
        us = [timed(fn, n) for _ in range(3)]
        assert ss["status"].tolist() == [63, B] and int(ss["stop_at"].min()) == D.INT_MAX
        rows.append(dict(B=B, stop_strings=len(STRINGS) if strings else 0, partial_match=partial, iters=n, us=[round(u, 2) for u in us]))
    print(json.dumps(dict(mode="kernel", history=S0 + 64, eos_ids=2, W=table["W"], P=table["P"], E=table["E"], rows=rows)))


def generate_mode():
    import bench
    from audio_flamingo_amd.frontend import LogMelFrontend
    from audio_flamingo_amd.modeling import AudioFlamingo3ForConditionalGeneration as Model

    model = Model(bench.af3_7b_config(), device=dev, init_seed=0)
    model.check_placeholders = False
    waves, ids, _ = bench.synthetic_batch(1, 0, dev)
    ids = ids[:, : 9 + 750 + 9]
    feats = LogMelFrontend(dev)(waves, out_dtype=torch.bfloat16)
    legs = args.legs.split(",")
    kw = {"greedy": {}}
    res = dict(mode="generate", tree=os.path.abspath(args.tree), new=args.new, legs={}, full_length={}, same_ids={})

    def run(leg, new, keep=None):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = model.generate(ids, input_features=feats, max_new_tokens=new, **kw[leg])
        torch.cuda.synchronize()
        if keep is not None:
            keep[leg] = out
        return time.perf_counter() - t0

    outs = {}
    run("greedy", 1), run("greedy", args.new, outs)
    used = set(outs["greedy"][0].tolist())
    eos = [i for i in range(V - 1, 0, -1) if i not in used][:2]      # two ids the greedy run never emits: every leg decodes the same N tokens
    kw["eos_list"] = dict(eos_token_id=eos)
    if "stop_strings" in legs:
        kw["stop_strings"] = dict(eos_token_id=eos, stop_strings=STRINGS, tokenizer=byte_tokenizer())
    for leg in legs:
        run(leg, 1), run(leg, args.new, outs)      # warm both shapes
        res["full_length"][leg] = outs[leg].shape[1] == ids.shape[1] + args.new
        res["same_ids"][leg] = bool(outs[leg].shape == outs["greedy"].shape and torch.equal(outs[leg], outs["greedy"]))
        res["legs"][leg] = []
    for _ in range(args.repeats):                  # legs alternate inside a repeat
        for leg in legs:
            res["legs"][leg].append(round(1e3 * (run(leg, args.new) - run(leg, 1)) / (args.new - 1), 4))
    print(json.dumps(res))


kernel_mode() if args.mode == "kernel" else generate_mode()

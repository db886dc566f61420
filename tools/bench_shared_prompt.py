"""afk_attn_decode_shared (csrc/attention_shared.hip) against the launch it replaces in a decode step, afk_attn_decode_fused on the expanded cache, and
generate(num_return_sequences=8) with the prompt cache shared and not.

  python tools/bench_shared_prompt.py kernel [out.json]   AF3-7B attention geometry (Hq 28, Hkv 4, D 128), one prompt row: n continuations behind Sp prompt
        positions, each with TAIL_FILL of T = 64 tail slots filled.  The shared launch pair (nsplit from ops.attn_shared_nsplit) against afk_attn_decode_fused over
        n cache rows of Sp + T positions (nsplit as the decode loop picks it: max(8, ceil(spad / 4096))).  Each form is captured into a HIP graph of NSET calls,
        one per cache set - as a decode step replays them, and so that the host's enqueue cost (Python checks, two launches against one) is in neither time -
        and REPEATS alternating repeats of `iters` calls each are timed with device events, `iters` sized so that a repeat of the slower form is about 0.2 s.
        The caches rotate over NSET distinct sets as the 28 layers of a model rotate them (the expanded sets are capped by EXPANDED_BYTES).
        Per shape: median us per call and the spread (max - min) / median, the bytes of K and Vt each form has to read, and both as fractions of streaming
        those bytes at 8 TB/s (the HBM rate DESIGN.md uses), and the two forms' outputs on one common set of keys against the kernels' test bar.
  python tools/bench_shared_prompt.py generate7b [out.json]   the AF3-7B geometry of bench.py (32 + 28 layers, 28:4 heads of 128, random init) behind the
        5-minute clip's prompt (9 + 7 500 <sound> + 9 ids = 7 518 positions): do_sample with num_return_sequences = 8, and num_beams = 4, each with share_prompt
        on and off alternating inside a repeat: time to the first token (max_new_tokens = 1), ms per step ((time of NEW tokens - time of 1) / (NEW - 1)), wall
        clock around a synchronise, and the peak of torch's allocator over the NEW-token call minus what was resident before it (weights, inputs).
  python tools/bench_shared_prompt.py generate [out.json]   the trained tiny golden model (2 layers, 4:2 heads of 64) behind its 772-row audio prompt,
        do_sample with num_return_sequences = 8: time to the first token (max_new_tokens = 1) and ms per step ((time of 65 tokens - time of 1) / 64), wall
        clock around a synchronise, and the peak of torch's allocator over the 65-token call; share_prompt on and off in alternating order.
  SP_LIST=...  N_LIST=...  select other kernel-leg shapes."""
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from audio_flamingo_amd import _lib, ops

dev = torch.device("cuda")
BF = torch.bfloat16
HBM = 8e12
REPEATS, NSET = int(os.environ.get("REPEATS", "5")), int(os.environ.get("NSET", "28"))
EXPANDED_BYTES = int(os.environ.get("EXPANDED_BYTES", str(6 << 30)))
T, TAIL_FILL = 64, 32


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
    Hq, Hkv, D = 28, 4, 128
    nq, nk = Hq * D, Hkv * D
    g = torch.Generator(device=dev).manual_seed(0)
    rnd = lambda *s, sc=1.0: (torch.randn(*s, device=dev, generator=g) * sc).to(BF)
    rows = []
    for Sp in [int(x) for x in os.environ.get("SP_LIST", "1000,7774,15274").split(",")]:
        Kp = [rnd(1, Sp, nk, sc=0.3) for _ in range(NSET)]
        Vtp = [rnd(1, Hkv, D, ops.pad64(Sp)) for _ in range(NSET)]
        for n in [int(x) for x in os.environ.get("N_LIST", "2,4,8,16").split(",")]:
            Smax = Sp + T
            spad = ops.pad64(Smax)
            per_set = n * (Smax * nk + Hkv * D * spad) * 2
            nset_x = max(2, min(NSET, EXPANDED_BYTES // per_set))
            Kx, Vx = [rnd(n, Smax, nk, sc=0.3) for _ in range(nset_x)], [rnd(n, Hkv, D, spad) for _ in range(nset_x)]
            Kt, Vtt = [rnd(n, T, nk, sc=0.3) for _ in range(NSET)], [rnd(n, Hkv, D, ops.pad64(T)) for _ in range(NSET)]
            # expanded set 0 holds the keys of shared set 0 (the prompt repeated, each tail behind it): the two forms' outputs are compared on it once
            Kx[0][:, :Sp], Kx[0][:, Sp:] = Kp[0], Kt[0]
            Vx[0][..., :Sp], Vx[0][..., Sp:Smax] = Vtp[0][..., :Sp], Vtt[0][..., :T]
            qkv = rnd(n, nq + 2 * nk, sc=0.3)
            q = qkv[:, :nq]
            qc = q.contiguous()
            o = torch.empty((n, nq), device=dev, dtype=BF)
            prange = torch.tensor([[0, Sp]], device=dev, dtype=torch.int32)
            trange = torch.tensor([[0, TAIL_FILL]] * n, device=dev, dtype=torch.int32)
            krange = torch.tensor([[0, Sp + TAIL_FILL]] * n, device=dev, dtype=torch.int32)
            ns_s = ops.attn_shared_nsplit(1, n, Hq, Hkv, Sp)
            ns_f = max(8, -(-spad // 4096))
            ws_s = torch.empty(int(_lib.load().afk_attn_decode_shared_workspace_floats(1, n, Hq, D, ns_s)), device=dev, dtype=torch.float32)
            ws_f = torch.zeros(int(_lib.load().afk_attn_decode_workspace_floats(n, Hq, D, ns_f)), device=dev, dtype=torch.float32)

            def shared(i):
                ops.attn_decode_shared(q, Kp[i % NSET], Vtp[i % NSET], Kt[i % NSET], Vtt[i % NSET], prange, trange, 1, n, Hq, Hkv, D, D ** -0.5, nsplit=ns_s, ws=ws_s, out=o)

            def fused(i):
                _lib.call("afk_attn_decode_fused", qc.data_ptr(), nq, D, Kx[i % nset_x].data_ptr(), Smax * nk, nk, D, Vx[i % nset_x].data_ptr(), Hkv * D * spad, spad,
                          o.data_ptr(), nq, D, krange.data_ptr(), n, Hq, Hkv, D, float(D ** -0.5), ns_f, ws_f.data_ptr(), ops._stream())

            variants = [("decode_fused, expanded cache", fused), ("decode_shared", shared)]
            fused(0)
            of = o.float().view(n, Hq, D).clone()
            shared(0)
            torch.cuda.synchronize()
            # the project's bar for these kernels per (continuation, head) slice, with the expanded launch as the reference (tests/_attn_probe.py)
            err, ref = (o.float().view(n, Hq, D) - of).norm(dim=-1), of.norm(dim=-1)
            worst = float((err / (2.0 ** -6 * ref + 2.0 ** -8 * D ** 0.5)).max())
            graphs = [(name, _graph_of(fn, NSET)) for name, fn in variants]   # every variant warmed on every cache set, then captured
            replays = max(2, min(2000, int(2e5 / max(_timed(graphs[0][1], 2, NSET), 1.0) / NSET)))   # ~0.2 s of the slow variant per repeat
            iters = replays * NSET
            times = {name: [] for name, _ in variants}
            for _ in range(REPEATS):
                for name, g_ in graphs:   # alternating: every variant once per repeat
                    times[name].append(_timed(g_, replays, NSET))
            bytes_x = 2 * 2 * n * (Sp + TAIL_FILL) * nk                    # K + Vt of the visible keys, bf16, every continuation its own
            bytes_s = 2 * 2 * (Sp + n * TAIL_FILL) * nk                    # the prompt once, the tails per continuation
            row = {"Sp": Sp, "n": n, "T": T, "tail_keys": TAIL_FILL, "iters": iters, "cache_sets": [nset_x, NSET], "nsplit": [ns_f, ns_s],
                   "bytes": [bytes_x, bytes_s], "outputs_worst_err_over_bar": round(worst, 3)}
            for (name, ts), nbytes in zip(times.items(), (bytes_x, bytes_s)):
                med = statistics.median(ts)
                row[name] = {"us": round(med, 1), "spread": round((max(ts) - min(ts)) / med, 3), "of_bound": round(1e6 * nbytes / HBM / med, 3)}
            row["speedup"] = round(row["decode_fused, expanded cache"]["us"] / row["decode_shared"]["us"], 2)
            rows.append(row)
            print(json.dumps(row), flush=True)
            del Kx, Vx, graphs
    return rows


def generate_leg():
    from tests.test_sampler_gpu import _case_a

    m, p, audio = _case_a(dev)
    n, steps = 8, 64
    kw = dict(audio, do_sample=True, temperature=1.5, top_k=0, seed=2, num_return_sequences=n)

    def run(share, new):
        torch.cuda.empty_cache()   # the graph capture inside generate() empties the caching allocator: outside the timed window for both variants
        torch.cuda.reset_peak_memory_stats()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        m.generate(p, max_new_tokens=new, share_prompt=share, **kw)
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0), torch.cuda.max_memory_allocated()

    res = {"prompt_rows": int(p.shape[1]), "copies": n, "steps": steps, "model": "tiny golden (2 decoder layers, hidden 256, 4:2 heads of 64)"}
    t = {(s, new): [] for s in (True, False) for new in (1, steps + 1)}
    peak = {}
    for rep in range(2 * REPEATS + 1):   # repeat 0 warms; the order alternates
        for share in ((True, False) if rep % 2 else (False, True)):
            for new in (1, steps + 1):
                ms, pk = run(share, new)
                if rep:
                    t[(share, new)].append(ms)
                    peak[(share, new)] = pk
    for share in (True, False):
        first, full = statistics.median(t[(share, 1)]), statistics.median(t[(share, steps + 1)])
        res["shared" if share else "expanded"] = {
            "first_token_ms": round(first, 2), "first_token_spread": round((max(t[(share, 1)]) - min(t[(share, 1)])) / first, 3),
            "ms_per_step": round((full - first) / steps, 4), "call_spread": round((max(t[(share, steps + 1)]) - min(t[(share, steps + 1)])) / full, 3),
            "peak_allocated_mib": round(peak[(share, steps + 1)] / 2 ** 20, 1)}
    m.generate(p, max_new_tokens=steps + 1, share_prompt=True, **kw)
    res["share_stats"] = m.last_share_stats
    print(json.dumps(res), flush=True)
    return res


def generate7b_leg():
    import bench
    from audio_flamingo_amd.frontend import LogMelFrontend
    from audio_flamingo_amd.modeling import AudioFlamingo3ForConditionalGeneration as Model

    new, windows = int(os.environ.get("NEW", "33")), int(os.environ.get("WINDOWS", "10"))
    model = Model(bench.af3_7b_config(), device=dev, init_seed=0)
    model.check_placeholders = False
    waves, ids, _ = bench.synthetic_batch(1, 0, dev, windows)
    ids = ids[:, : 9 + bench.N_AUDIO_TOK * windows + 9]
    feats = LogMelFrontend(dev)(waves, out_dtype=BF)
    del waves
    res = {"model": "AF3-7B geometry, random init", "prompt_rows": int(ids.shape[1]), "new_tokens": new, "repeats": REPEATS, "routes": {}}
    routes = {"sampled, num_return_sequences=8": dict(do_sample=True, temperature=1.5, top_k=0, seed=2, num_return_sequences=8),
              "beams, num_beams=4": dict(num_beams=4)}
    for route, kw in routes.items():
        def run(share, n_new, record=None):
            torch.cuda.empty_cache()   # the graph capture inside generate() empties the caching allocator: outside the timed window for both variants
            torch.cuda.synchronize()
            if record is not None:
                torch.cuda.reset_peak_memory_stats()
                before = torch.cuda.memory_allocated()
            t0 = time.perf_counter()
            out = model.generate(ids, input_features=feats, max_new_tokens=n_new, share_prompt=share, **kw)
            torch.cuda.synchronize()
            dt = 1e3 * (time.perf_counter() - t0)
            if record is not None:
                record["peak_mib_over_resident"] = round((torch.cuda.max_memory_allocated() - before) / 2 ** 20, 1)
                record["full_length"] = int(out.shape[1]) == int(ids.shape[1]) + n_new
            return dt

        rows = {True: {}, False: {}}
        for share in (True, False):   # warm both shapes, then one recorded call
            run(share, 1), run(share, new)
            run(share, new, record=rows[share])
            if share:
                rows[share]["share_stats"] = model.last_share_stats
        first, step = {True: [], False: []}, {True: [], False: []}
        for rep_ in range(REPEATS):
            for share in ((True, False) if rep_ % 2 else (False, True)):
                t1, tn = run(share, 1), run(share, new)
                first[share].append(t1)
                step[share].append((tn - t1) / (new - 1))
        for share in (True, False):
            f, s_ = statistics.median(first[share]), statistics.median(step[share])
            rows[share].update(first_token_ms=round(f, 1), first_token_spread=round((max(first[share]) - min(first[share])) / f, 3),
                               ms_per_step=round(s_, 3), ms_per_step_spread=round((max(step[share]) - min(step[share])) / s_, 3))
        res["routes"][route] = {"shared": rows[True], "expanded": rows[False]}
        print(json.dumps({route: res["routes"][route]}), flush=True)
    return res


if __name__ == "__main__":
    leg = sys.argv[1] if len(sys.argv) > 1 else "kernel"
    result = {"kernel": kernel_leg, "generate": generate_leg, "generate7b": generate7b_leg}[leg]()
    if len(sys.argv) > 2:
        os.makedirs(os.path.dirname(os.path.abspath(sys.argv[2])), exist_ok=True)
        with open(sys.argv[2], "w") as f:
            json.dump(result, f, indent=1)

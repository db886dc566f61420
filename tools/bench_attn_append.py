"""afk_attn_append (csrc/attention_append.hip) against the interval kernel it replaces in a continued generate() turn (afk_xattn_fwd), and the turn itself.

  python tools/bench_attn_append.py kernel [out.json]   AF3-7B geometry (Hq 28, Hkv 4, D 128), B = 1: n new rows behind P cached positions, the causal
        staircase; afk_xattn_fwd and afk_attn_append at a sweep of nsplit, REPEATS alternating repeats of ITERS launches each (device events), the cache
        rotated over NSET distinct sets as the layers of a model rotate it.  Per shape: median us per launch and the spread (max - min) / median over the
        repeats, the fraction of the cache-streaming bound (K + Vt of the visible keys read once at 8 TB/s, the HBM rate DESIGN.md uses), and what
        ops.attn_append_nsplit picks.
  python tools/bench_attn_append.py turn [out.json]     the trained tiny golden model: turn 2 (a 64-token question behind the 772-row audio prompt and an
        8-token answer), max_new_tokens 32, wall time with a synchronise: from scratch / continued on the cache with the append kernel / continued with the
        interval kernel (append_min_keys above every length); 2 * REPEATS repeats in rotating order.
  GEOM=Hq,Hkv,D  B=...  P_LIST=...  N_LIST=...  select other kernel-leg shapes (GEOM=4,2,64 P_LIST=780 N_LIST=65: the tiny model's turn)."""
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
REPEATS, NSET = int(os.environ.get("REPEATS", "3")), int(os.environ.get("NSET", "6"))


def _timed(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(iters):
        fn(i)
    e1.record()
    torch.cuda.synchronize()
    return 1e3 * e0.elapsed_time(e1) / iters


def kernel_leg():
    Hq, Hkv, D = (int(x) for x in os.environ.get("GEOM", "28,4,128").split(","))   # GEOM=4,2,64: the tiny golden model of the turn leg
    nq, nk = Hq * D, Hkv * D
    g = torch.Generator(device=dev).manual_seed(0)
    rnd = lambda *s, sc=1.0: (torch.randn(*s, device=dev, generator=g) * sc).to(BF)
    B = int(os.environ.get("B", "1"))
    rows = []
    for P in [int(x) for x in os.environ.get("P_LIST", "1024,8192,15000").split(",")]:
        Smax = P + 768 + 64
        spad = ops.pad64(Smax)
        Kc = [rnd(B, Smax, nk, sc=0.3) for _ in range(NSET)]
        Vt = [rnd(B, Hkv, D, spad) for _ in range(NSET)]
        for n in [int(x) for x in os.environ.get("N_LIST", "8,64,768").split(",")]:
            qkv = rnd(B * n, nq + 2 * nk, sc=0.3)
            q = qkv[:, :nq]
            ar = torch.arange(P, P + n, device=dev, dtype=torch.int32)
            kr = torch.stack([torch.zeros_like(ar), ar + 1], -1)[None].expand(B, n, 2).contiguous()
            o = torch.empty((B * n, nq), device=dev, dtype=BF)
            lse = torch.empty((B, Hq, n), device=dev, dtype=torch.float32)
            st = ops._stream()
            tiles = B * Hkv * -(-n // (32 // (Hq // Hkv)))
            sweep = [s for s in (1, 2, 4, 8, 16, 32, 64) if s == 1 or ((P + n) // s >= 128 and s * tiles <= 8192)]
            ws = torch.empty(int(_lib.load().afk_attn_append_workspace_floats(B, Hq, n, D, max(sweep))), device=dev, dtype=torch.float32)

            def xattn(i):
                _lib.call("afk_xattn_fwd", q.data_ptr(), n * q.stride(0), D, q.stride(0), Kc[i % NSET].data_ptr(), Smax * nk, D, nk, Vt[i % NSET].data_ptr(),
                          o.data_ptr(), n * nq, D, nq, lse.data_ptr(), 0, kr.data_ptr(), B, Hq, Hkv, n, P + n, ops.pad64(n), spad, D, float(D ** -0.5), st)

            def append(ns):
                return lambda i: ops.attn_append(q, Kc[i % NSET], Vt[i % NSET], kr, B, n, Hq, Hkv, D, D ** -0.5, nsplit=ns, ws=ws, out=o)

            variants = [("xattn", xattn)] + [(f"append ns={s}", append(s)) for s in sweep]
            xattn(0)
            torch.cuda.synchronize()
            iters = max(6, min(60, int(2e5 / max(_timed(xattn, 3), 1.0))))   # ~0.2 s of the slow variant per repeat
            for _, fn in variants:
                _timed(fn, NSET)   # warm every variant on every cache set
            times = {name: [] for name, _ in variants}
            for _ in range(REPEATS):
                for name, fn in variants:   # alternating: every variant once per repeat
                    times[name].append(_timed(fn, iters))
            bound_us = 1e6 * 2.0 * 2 * (P + n) * nk * B / HBM
            row = {"geom": [Hq, Hkv, D], "B": B, "P": P, "n": n, "iters": iters, "bound_us": round(bound_us, 2), "rule_nsplit": ops.attn_append_nsplit(B, Hq, Hkv, n, P + n)}
            for name, ts in times.items():
                med = statistics.median(ts)
                row[name] = {"us": round(med, 1), "spread": round((max(ts) - min(ts)) / med, 3), "of_bound": round(bound_us / med, 3)}
            rows.append(row)
            print(json.dumps(row), flush=True)
    return rows


def turn_leg():
    from tests.test_sampler_gpu import _case_a

    m, p, audio = _case_a(dev)
    g = torch.Generator().manual_seed(1)
    out1 = m.generate(p, max_new_tokens=8, return_dict_in_generate=True, **audio)
    full = torch.cat([out1.sequences, torch.randint(0, 256, (1, 64), generator=g).to(dev)], 1)

    def clone(c):
        from audio_flamingo_amd.modeling import AfkKVCache

        return AfkKVCache(c.K.clone(), c.Vt.clone(), c.lo.clone(), c.length)

    def scratch():
        return m.generate(full, max_new_tokens=32, **audio)

    def cont(min_keys):
        def run():
            m.append_min_keys = min_keys
            try:
                return m.generate(full, past_key_values=run.cache, max_new_tokens=32)
            finally:
                del m.append_min_keys
        return run

    variants = [("from scratch", scratch), ("continued, append kernel", cont(0)), ("continued, interval kernel", cont(1 << 30))]
    times = {name: [] for name, _ in variants}
    ids = {}
    for rep in range(2 * REPEATS + 1):   # repeat 0 warms; the order rotates, so that what a call leaves in the allocator favours nobody
        for name, fn in variants[rep % 3:] + variants[:rep % 3]:
            fn.cache = clone(out1.past_key_values)   # outside the timed window: a chat loop holds its cache
            # the graph capture inside generate() empties the caching allocator first: without this the variant that runs behind the from-scratch call pays
            # for freeing that call's encoder activations (measured: 1.1 ms on whichever continued variant came second)
            torch.cuda.empty_cache()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ids[name] = fn()
            torch.cuda.synchronize()
            if rep:
                times[name].append(1e3 * (time.perf_counter() - t0))
    res = {"prompt_rows": int(p.shape[1]), "turn_rows": int(full.shape[1] - out1.past_key_values.length), "max_new_tokens": 32,
           "same_ids": bool(all(torch.equal(ids["from scratch"], v) for v in ids.values()))}
    for name, ts in times.items():
        med = statistics.median(ts)
        res[name] = {"ms": round(med, 2), "spread": round((max(ts) - min(ts)) / med, 3)}
    print(json.dumps(res), flush=True)
    return res


if __name__ == "__main__":
    leg = sys.argv[1] if len(sys.argv) > 1 else "kernel"
    result = kernel_leg() if leg == "kernel" else turn_leg()
    if len(sys.argv) > 2:
        os.makedirs(os.path.dirname(os.path.abspath(sys.argv[2])), exist_ok=True)
        with open(sys.argv[2], "w") as f:
            json.dump(result, f, indent=1)

"""The two flat AdamW launches alone on the chip, same process, same box: adamw_kernel (fp32 master / m / v, 28 B/param) against adamw16_kernel
(bf16 m / v, no master, 14 B/param).  n = 2^30 elements by default (AF3-7B has 8.27e9 parameters: a launch of this size is an eighth of its step),
HIP events around every single launch, the two kernels alternating, warm-up first; median, min and max per kernel, GB/s on the algorithmic bytes,
share of the 6.29 TB/s achievable HBM rate and the ratio of the medians.  --out writes the markdown record (profiles/adamw16_bench.md).

    python tools/bench_adamw.py [--n 1073741824] [--iters 25] [--warmup 5] [--out FILE.md]"""
import argparse, json, os, statistics, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from audio_flamingo_amd import ops

ACHIEVABLE_TBS = 6.29

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=1 << 30)
ap.add_argument("--iters", type=int, default=25)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--out", default=None)
a = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("bench_adamw.py needs the GPU: a timing taken elsewhere says nothing")
dev, n = torch.device("cuda"), a.n
hp = dict(lr=1e-4, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.01)


def fill(dtype, scale):
    t = torch.empty(n, device=dev, dtype=dtype)
    for s in range(0, n, 1 << 27):
        t[s: s + (1 << 27)] = (torch.randn(min(1 << 27, n - s), device=dev) * scale).to(dtype)
    return t


grad = fill(torch.bfloat16, 1e-3)
p32, p16 = fill(torch.bfloat16, 0.02), fill(torch.bfloat16, 0.02)
master = p32.float()
m32, v32 = torch.zeros(n, device=dev), torch.zeros(n, device=dev)
m16, v16 = torch.zeros(n, device=dev, dtype=torch.bfloat16), torch.zeros(n, device=dev, dtype=torch.bfloat16)
step = [0, 0]


def run32():
    step[0] += 1
    ops.adamw_step(master, m32, v32, grad, p32, step=step[0], **hp)


def run16():
    step[1] += 1
    ops.adamw16_step(m16, v16, grad, p16, step=step[1], **hp)


kernels = (("adamw_kernel (fp32 master / m / v)", run32, 28), ("adamw16_kernel (bf16 m / v)", run16, 14))
for _ in range(a.warmup):
    for _, fn, _ in kernels:
        fn()
torch.cuda.synchronize()
times = [[], []]
for _ in range(a.iters):
    for i, (_, fn, _) in enumerate(kernels):   # alternating: both see the same box at the same moment
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        times[i].append(e0.elapsed_time(e1))
rows = []
for (name, _, bpe), t in zip(kernels, times):
    med = statistics.median(t)
    rows.append(dict(kernel=name, bytes_per_param=bpe, launches=len(t), ms_median=round(med, 4), ms_min=round(min(t), 4), ms_max=round(max(t), 4),
                     GBps_median=round(n * bpe / med / 1e6, 1), share_of_achievable_hbm=round(n * bpe / med / 1e9 / ACHIEVABLE_TBS, 3)))
ratio = rows[1]["ms_median"] / rows[0]["ms_median"]
res = dict(n=n, warmup=a.warmup, device=torch.cuda.get_device_name(0), kernels=rows, ratio_bf16_over_fp32=round(ratio, 4),
           af3_7b_ms={r["kernel"]: round(r["ms_median"] * 8.27e9 / n, 2) for r in rows})
print(json.dumps(res))
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(f"## flat AdamW launches alone, n = {n} elements, {a.iters} timed launches each (alternating, {a.warmup} warm-up), HIP events, {res['device']}\n\n")
        f.write("| kernel | B/param | median ms | min ms | max ms | GB/s (median) | share of 6.29 TB/s | AF3-7B (8.27e9 params) ms |\n|---|---|---|---|---|---|---|---|\n")
        for r in rows:
            f.write(f"| {r['kernel']} | {r['bytes_per_param']} | {r['ms_median']} | {r['ms_min']} | {r['ms_max']} | {r['GBps_median']} | "
                    f"{r['share_of_achievable_hbm']} | {res['af3_7b_ms'][r['kernel']]} |\n")
        f.write(f"\nratio of the medians, bf16 state / fp32 state: **{ratio:.3f}** (the byte ratio is 0.5)\n")

"""GEMM microbenchmark on the AF3-7B shapes (random data, guide rule 25): the two 256x256 NT kernels (v2 = 8-wave ping-pong, v3 = 4-wave
128x128 per wave), HIP-event timed through afk_prof_*.   python tools/bench_gemm.py [zeros]   (zeros: zero-filled operands = DVFS probe)
    python tools/bench_gemm.py mfma [out.json]    the step's NT / NN / TN shapes on each MFMA shape the library carries (ops.gemm_set_mfma 1 = 32x32x16,
    2 = 16x16x32), alternating shape by shape: 5 warm + 25 timed launches each, HIP events per launch -> median / min / max per row
    python tools/bench_gemm.py libs OTHER_LIBAFK_SO [out.json]   the same rows on two builds of the library in one process - the loaded one ("this") and
    OTHER ("other", e.g. the parent commit's build) - alternating launch by launch; each on its own dispatch rule, 256x256 kernels forced"""
import sys, os, json
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from audio_flamingo_amd import ops

SHAPES = [  # (name, M, N, K)
    ("dec gate_up fwd", 8192, 37888, 3584), ("dec down fwd", 8192, 3584, 18944), ("dec qkv fwd", 8192, 4608, 3584), ("dec o fwd", 8192, 3584, 3584),
    ("dec gate_up wgrad", 37888, 3584, 8192), ("dec down wgrad", 3584, 18944, 8192), ("dec gate_up dgrad", 8192, 3584, 37888),
    ("lm_head chunk", 2048, 152064, 3584), ("lm_head dgrad", 2048, 3584, 152064), ("lm_head wgrad", 152064, 3584, 2048),
    ("enc qkv fwd", 12000, 3840, 1280), ("enc fc1 fwd", 12000, 5120, 1280), ("enc fc2 fwd", 12000, 1280, 5120), ("enc out fwd", 12000, 1280, 1280),
    ("enc fc1 wgrad", 5120, 1280, 12032), ("enc qkv wgrad", 3840, 1280, 12032), ("enc out wgrad", 1280, 1280, 12032),
    ("square 4096", 4096, 4096, 4096), ("square 8192", 8192, 8192, 8192),
]
dev = torch.device("cuda")


def step_rows():
    """the step's NT / NN / TN shapes (table (c) of profiles/gemm_mfma_shape_ab.md)"""
    rows = [("nt", n, M, N, K) for n, M, N, K in SHAPES[:4] + SHAPES[7:8] + SHAPES[10:14]]
    rows += [("nn", "dec gate_up dgrad", 8192, 3584, 37888), ("nn", "dec down dgrad", 8192, 18944, 3584), ("nn", "dec qkv dgrad", 8192, 3584, 4608),
             ("nn", "dec o dgrad", 8192, 3584, 3584), ("nn", "lm_head dgrad", 2048, 3584, 152064), ("nn", "enc fc1 dgrad", 12000, 1280, 5120), ("nn", "enc qkv dgrad", 12000, 1280, 3840),
             ("tn", "dec gate_up wgrad", 37888, 3584, 8192), ("tn", "dec down wgrad", 3584, 18944, 8192), ("tn", "dec qkv wgrad", 4608, 3584, 8192),
             ("tn", "dec o wgrad", 3584, 3584, 8192), ("tn", "lm_head wgrad", 152064, 3584, 2048), ("tn", "enc fc1 wgrad", 5120, 1280, 12000),
             ("tn", "enc qkv wgrad", 3840, 1280, 12000), ("tn", "enc out wgrad", 1280, 1280, 12000)]
    return rows


def libs_ab(other_path, out_path):
    """per-shape A/B of two builds of libafk.so (profiles/gemm_tail.md table (b)): faster / slower only if the medians differ by more than twice the
    larger (max - min) of the two arms, else a tie"""
    import ctypes
    import statistics
    from audio_flamingo_amd import _lib
    this = _lib.load()
    other = ctypes.CDLL(other_path)
    for name, (ret, argtypes, _) in _lib.prototypes().items():
        fn = getattr(other, name)
        fn.restype, fn.argtypes = ret, argtypes
    arms = {"this": this, "other": other}
    res = []
    try:
        for lib in arms.values():
            _lib._lib = lib
            ops.gemm_set_variant(2)
        for form, name, M, N, K in step_rows():
            a = torch.randn((K, M) if form == "tn" else (M, K), device=dev).to(torch.bfloat16)
            b = torch.randn((N, K) if form == "nt" else (K, N), device=dev).to(torch.bfloat16)
            c = torch.empty((M, N), device=dev, dtype=torch.bfloat16)
            run = (lambda: ops.gemm_nt(a, b, out=c)) if form == "nt" else (lambda: ops.gemm(a, b, out=c, trans_a=form == "tn", trans_b=True))
            ev = {k: [] for k in arms}
            for it in range(30):          # 5 warm + 25 timed, the builds alternating launch by launch
                for k, lib in arms.items():
                    _lib._lib = lib
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record(); run(); e1.record()
                    if it >= 5:
                        ev[k].append((e0, e1))
            torch.cuda.synchronize()
            row = {"form": form, "name": name, "M": M, "N": N, "K": K}
            for k in arms:
                us = sorted(1e3 * x.elapsed_time(y) for x, y in ev[k])
                row[f"{k}_us"] = {"median": round(statistics.median(us), 1), "min": round(us[0], 1), "max": round(us[-1], 1)}
            d = row["other_us"]["median"] - row["this_us"]["median"]
            noise = 2 * max(row[f"{k}_us"]["max"] - row[f"{k}_us"]["min"] for k in arms)
            row["this_vs_other_pct"] = round(100.0 * d / row["other_us"]["median"], 2)
            row["verdict"] = "faster" if d > noise else "slower" if -d > noise else "tie"
            res.append(row)
            print(json.dumps(row), flush=True)
            del a, b, c
    finally:
        for lib in arms.values():
            _lib._lib = lib
            ops.gemm_set_variant(0)
        _lib._lib = this
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        json.dump({"device": torch.cuda.get_device_name(0), "this": _lib.LIB_PATH, "other": other_path, "rows": res}, open(out_path, "w"), indent=1)


def mfma_ab(out_path):
    """per-shape A/B of the MFMA shapes (profiles/gemm_mfma_shape_ab.md table (c))"""
    import statistics
    rows = step_rows()
    res = []
    ops.gemm_set_variant(2)
    try:
        for form, name, M, N, K in rows:
            a = torch.randn((K, M) if form == "tn" else (M, K), device=dev).to(torch.bfloat16)
            b = torch.randn((N, K) if form == "nt" else (K, N), device=dev).to(torch.bfloat16)
            c = torch.empty((M, N), device=dev, dtype=torch.bfloat16)
            run = (lambda: ops.gemm_nt(a, b, out=c)) if form == "nt" else (lambda: ops.gemm(a, b, out=c, trans_a=form == "tn", trans_b=True))
            shapes = ops.gemm_mfma_shapes(form)
            ev = {v: [] for v in shapes}
            for it in range(30):          # 5 warm + 25 timed, the shapes alternating launch by launch
                for v in shapes:
                    ops.gemm_set_mfma(v)
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record(); run(); e1.record()
                    if it >= 5:
                        ev[v].append((e0, e1))
            torch.cuda.synchronize()
            row = {"form": form, "name": name, "M": M, "N": N, "K": K}
            for v in shapes:
                us = sorted(1e3 * x.elapsed_time(y) for x, y in ev[v])
                row[f"mfma{v}_us"] = {"median": round(statistics.median(us), 1), "min": round(us[0], 1), "max": round(us[-1], 1)}
                row[f"mfma{v}_tflops"] = round(2.0 * M * N * K / statistics.median(us) / 1e6, 1)
            if len(shapes) == 2:
                row["speedup_2_over_1"] = round(row["mfma1_us"]["median"] / row["mfma2_us"]["median"], 4)
            res.append(row)
            print(json.dumps(row), flush=True)
            del a, b, c
    finally:
        ops.gemm_set_mfma(0)
        ops.gemm_set_variant(0)
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        json.dump({"device": torch.cuda.get_device_name(0), "rows": res}, open(out_path, "w"), indent=1)


if len(sys.argv) > 2 and sys.argv[1] == "libs":
    libs_ab(sys.argv[2], sys.argv[3] if len(sys.argv) > 3 else None)
    sys.exit(0)
if len(sys.argv) > 1 and sys.argv[1] == "mfma":
    mfma_ab(sys.argv[2] if len(sys.argv) > 2 else None)
    sys.exit(0)
ZEROS = len(sys.argv) > 1 and sys.argv[1] == "zeros"
if len(sys.argv) > 1 and sys.argv[1] == "nt":
    SHAPES = SHAPES[:12] + SHAPES[-2:]
if len(sys.argv) > 2 and sys.argv[2] == "few":
    SHAPES = [SHAPES[0], SHAPES[1], SHAPES[3], SHAPES[11], SHAPES[-1]]
res = []
if len(sys.argv) > 1 and sys.argv[1] in ("bw", "bwzeros"):
    SHAPES = []
for name, M, N, K in SHAPES:
    a = (torch.rand((M, K), device=dev) * 2 - 1).to(torch.bfloat16)
    b = (torch.rand((N, K), device=dev) * 2 - 1).to(torch.bfloat16)
    if ZEROS:
        a.zero_(); b.zero_()
    c = torch.empty((M, N), device=dev, dtype=torch.bfloat16)
    row = {"name": name, "M": M, "N": N, "K": K}
    for v in [int(x) for x in os.environ.get("AFK_BENCH_VARIANTS", "2,3").split(",")]:
        ops.gemm_set_variant(v)
        for _ in range(2):
            ops.gemm_nt(a, b, out=c)
        torch.cuda.synchronize()
        ops.prof_reset(); ops.prof_enable(True)
        for _ in range(5):
            ops.gemm_nt(a, b, out=c)
        ops.prof_enable(False)
        ms, fl, n = ops.prof_collect()
        row[f"v{v}_tflops"] = round(fl / ms / 1e9, 1)
        row[f"v{v}_us"] = round(1e3 * ms / n, 1)
    ops.gemm_set_variant(0)
    res.append(row)
    print(json.dumps(row), flush=True)

if len(sys.argv) > 1 and sys.argv[1] not in ("bw", "bwzeros"):
    sys.exit(0)
ZEROS = ZEROS or (len(sys.argv) > 1 and sys.argv[1] == "bwzeros")
# ---- backward forms: NN (dgrad) and TN (wgrad) against the NT kernel fed with pre-transposed operands
print("--- NN / TN forms (v2 = 256 kernels); nt_* = same contraction on the NT kernel incl. nothing else", flush=True)
BW = [("dec gate_up dgrad NN", "NN", 8192, 3584, 37888), ("dec down dgrad NN", "NN", 8192, 18944, 3584), ("dec qkv dgrad NN", "NN", 8192, 3584, 4608),
      ("lm_head dgrad NN", "NN", 2048, 3584, 152064), ("enc fc1 dgrad NN", "NN", 12000, 1280, 5120), ("enc qkv dgrad NN", "NN", 12000, 1280, 3840),
      ("dec gate_up wgrad TN", "TN", 37888, 3584, 8192), ("dec down wgrad TN", "TN", 3584, 18944, 8192), ("dec qkv wgrad TN", "TN", 4608, 3584, 8192),
      ("lm_head wgrad TN", "TN", 152064, 3584, 2048), ("enc fc1 wgrad TN", "TN", 5120, 1280, 12000), ("enc qkv wgrad TN", "TN", 3840, 1280, 12000),
      ("enc out wgrad TN", "TN", 1280, 1280, 12000), ("proj l2 wgrad TN", "TN", 3584, 3584, 6000)]
for name, form, M, N, K in BW:
    if form == "NN":
        a = (torch.rand((M, K), device=dev) * 2 - 1).to(torch.bfloat16)
        b = (torch.rand((K, N), device=dev) * 2 - 1).to(torch.bfloat16)
        kw = dict(trans_b=True)
    else:
        a = (torch.rand((K, M), device=dev) * 2 - 1).to(torch.bfloat16)
        b = (torch.rand((K, N), device=dev) * 2 - 1).to(torch.bfloat16)
        kw = dict(trans_a=True, trans_b=True)
    if ZEROS:
        a.zero_(); b.zero_()
    c = torch.empty((M, N), device=dev, dtype=torch.bfloat16)
    for _ in range(2):
        ops.gemm(a, b, out=c, **kw)
    torch.cuda.synchronize()
    ops.prof_reset(); ops.prof_enable(True)
    for _ in range(5):
        ops.gemm(a, b, out=c, **kw)
    ops.prof_enable(False)
    ms, fl, n = ops.prof_collect()
    print(json.dumps({"name": name, "M": M, "N": N, "K": K, "tflops": round(fl / ms / 1e9, 1), "us": round(1e3 * ms / n, 1)}), flush=True)

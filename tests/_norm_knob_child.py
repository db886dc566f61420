"""Child process of tests/test_norm_edges_gpu.py's knob tests: AFK_NORM_BWD / AFK_NORM_BWD_R are read once per process when the library first
dispatches a norm backward, so each knob needs a fresh process.  usage: python _norm_knob_child.py cases.pt out.pt
cases.pt: a list of dicts (kind, x, w, dy, mean, rstd, dx_add or None, dw_old or None) of CPU tensors; out.pt: per case dict(dx, dw, db) or dict(error)."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main(src, dst):
    import torch

    from audio_flamingo_amd import ops
    from audio_flamingo_amd._lib import AfkError

    dev = torch.device("cuda:0")
    out = []
    for c in torch.load(src):
        t = {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in c.items()}
        D = t["x"].shape[-1]
        acc = t["dw_old"] is not None
        dw = t["dw_old"].clone() if acc else torch.full((D,), float("nan"), device=dev, dtype=torch.bfloat16)
        db = dw.clone()
        try:
            if t["kind"] == "ln":
                dx = ops.layernorm_bwd(t["x"], t["w"], t["dy"], t["mean"], t["rstd"], dw, db, dx_add=t["dx_add"], accumulate=acc)
            else:
                dx = ops.rmsnorm_bwd(t["x"], t["w"], t["dy"], t["rstd"], dw, dx_add=t["dx_add"], accumulate=acc)
            torch.cuda.synchronize()
            out.append(dict(dx=dx.cpu(), dw=dw.cpu(), db=db.cpu()))
        except AfkError as e:
            out.append(dict(error=str(e)))
    torch.save(out, dst)


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2])

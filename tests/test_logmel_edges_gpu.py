"""csrc/logmel.hip on an MI355X at its edges, held to the float64 pipeline of tests/_frontend_ref.py within the DERIVED forward-error bound of its fp32
arithmetic (logmel_bound; tests/test_frontend_ref_cpu.py shows that four real mistakes exceed it on 7 % - 100 % of the outputs): T = 3 (fewer frames than
one 32-frame block), 33 (one block and one frame), 64 (no ragged block), 200 at n_mels = 64 (the fstep = 4 mapping of the mel stage) and 5 x 1650 frames
(logmel_finish_kernel past its 4096-block cap), on noise, a tone in noise and a half-silent window.  The bound is a worst case and loose, so the kernel's
median and 99.9th-percentile error are also held to 4x those of a torch fp32 restatement of the same steps (the factor test_ops_gpu.py::test_logmel
allows between independent fp32 evaluations of this pipeline).  Beside that: an all-zero window is exactly -1.5 whatever its neighbour, a window's
output does not depend on the batch it is in, two calls are bit-equal, and the bf16 output is the fp32 output rounded once.

Measured on an MI355X (the module prints them), per case: max error / bound; share left out (bound > 1e-2); share near the floor; median error, kernel
(fp32 restatement); 99.9th-percentile error, kernel (restatement):
  W1 T3    mels128   0.0057   0        0        4.48e-8 (4.00e-8)   2.13e-7 (2.39e-7)
  W3 T33   mels128   0.0298   2.45e-3  2.37e-4  4.91e-8 (3.30e-8)   8.47e-6 (1.07e-5)
  W3 T64   mels128   0.0290   1.99e-3  0        4.83e-8 (3.22e-8)   8.33e-6 (1.15e-5)
  W3 T200  mels64    0.0222   2.60e-5  0        4.01e-8 (2.64e-8)   2.85e-6 (4.48e-6)
  W5 T1650 mels128   0.0359   2.69e-3  1.66e-4  5.24e-8 (3.73e-8)   9.15e-6 (1.33e-5)
so the kernel's median is 1.1 - 1.5x the restatement's and its 99.9th percentile 0.6 - 0.9x (allowed: 4x).  The all-zero window came out -1.5000002 in
fp32 before log10(max(mel, 1e-10)) took its floored value as -10 exactly (log10f(1e-10f) is one ulp below -10 on the device); it is -1.5 now.
Module wall time 2.9 s for 10 cases; the slowest are the first call (1.6 s) and the 5 x 1650-frame case (0.6 s, its float64 reference and bound).
"""
import functools

import numpy as np
import pytest
import torch

from tests import _frontend_ref as R

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
CASE_IDS = [f"W{w}_T{n // R.HOP}_mels{m}" for w, n, m in R.LOGMEL_CASES]
STAT_FACTOR = 4.0


@functools.lru_cache(maxsize=None)
def _frontend(dev, n_mels):
    from audio_flamingo_amd.frontend import LogMelFrontend

    return LogMelFrontend(dev, n_mels)


@pytest.mark.parametrize("W,nsamp,n_mels", R.LOGMEL_CASES, ids=CASE_IDS)
def test_logmel_within_the_derived_bound(dev, W, nsamp, n_mels):
    fe = _frontend(dev, n_mels)
    wav = R.logmel_wave(W, nsamp)
    b = R.logmel_bound(wav, n_mels)
    wd = torch.from_numpy(wav.copy()).to(dev)
    out = fe(wd)
    assert out.shape == (W, n_mels, nsamp // R.HOP) and out.dtype == torch.float32
    got = out.cpu().numpy()
    assert np.isfinite(got).all()
    assert b.left_out <= R.SHARE_CAP and b.near_floor <= R.SHARE_CAP
    r = R.logmel_ratio(got, b)
    k_med, k_top = R.error_percentiles(got, b.ref)
    r_med, r_top = R.error_percentiles(R.logmel_fp32_restatement(wav, n_mels).numpy(), b.ref)
    print(f"logmel W={W} T={nsamp // R.HOP} n_mels={n_mels}: {r:.4f} of the bound (left out {b.left_out:.2e}, near the floor {b.near_floor:.2e}); "
          f"median error {k_med:.3g} (fp32 restatement {r_med:.3g}), 99.9th percentile {k_top:.3g} (restatement {r_top:.3g})")
    assert r <= 1.0, r
    assert k_med <= STAT_FACTOR * r_med and k_top <= STAT_FACTOR * r_top, (k_med, r_med, k_top, r_top)
    assert torch.equal(R.bits(fe(wd)), R.bits(out)), "two calls differ"


def test_bf16_output_is_the_fp32_output_rounded_once(dev):
    W, nsamp, n_mels = R.LOGMEL_CASES[1]
    fe = _frontend(dev, n_mels)
    wd = torch.from_numpy(R.logmel_wave(W, nsamp).copy()).to(dev)
    out, outb = fe(wd), fe(wd, out_dtype=BF)
    assert outb.dtype == BF and torch.equal(R.bits(outb), R.bits(out.to(BF)))
    assert torch.equal(R.bits(fe(wd, out_dtype=BF)), R.bits(outb)), "two calls differ"


@pytest.mark.parametrize("nsamp", [480, 160 * 33])
def test_all_zero_window_beside_a_loud_one(dev, nsamp):
    """mel = 0 -> log10(1e-10) = -10 in every bin, the window's own maximum too, so nothing is floored: (-10 + 4) / 4 = -1.5 exactly"""
    fe = _frontend(dev, 128)
    wav = np.zeros((3, nsamp), np.float32)
    wav[0] = np.random.default_rng(1).standard_normal(nsamp)
    wav[2] = 10.0 * R.logmel_wave(2, nsamp)[1]
    wd = torch.from_numpy(wav).to(dev)
    for dtype in (torch.float32, BF):
        out = fe(wd, out_dtype=dtype).cpu().float()
        assert bool((out[1] == -1.5).all()), (dtype, out[1].min().item(), out[1].max().item())
        assert bool((out[0].max() > 0.5)) and bool(torch.isfinite(out).all())


@pytest.mark.parametrize("nsamp", [160 * 33, 160 * 64])
def test_a_window_does_not_depend_on_its_batch(dev, nsamp):
    """a shared or leaked per-window maximum would floor the quiet window at the loud one's maximum - 8"""
    fe = _frontend(dev, 128)
    base = R.logmel_wave(3, nsamp)
    quiet = (1e-3 * base[0] / 0.1).astype(np.float32)
    loud = (1e4 * quiet[::-1]).astype(np.float32)
    both = torch.from_numpy(np.stack([loud, quiet])).to(dev)
    alone = fe(torch.from_numpy(quiet[None].copy()).to(dev))
    for order in ([0, 1], [1, 0]):
        out = fe(both[order].contiguous())
        assert torch.equal(R.bits(out[order.index(1)]), R.bits(alone[0])), ("the quiet window changed with its batch", order)
    ref = R.logmel_ref(np.stack([loud, quiet]), 128)
    assert np.abs(ref[1] - R.logmel_ref(quiet[None], 128)[0]).max() == 0 and ref[0].mean() - ref[1].mean() > 1.5, "the two windows are 80 dB apart"

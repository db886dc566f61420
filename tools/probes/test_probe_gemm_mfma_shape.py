"""The MFMA-shape tests of the product suite (tests/test_gemm_mfma_shape_gpu.py) on a probe build of libafk.so (`make -C audio-flamingo_amd/csrc PROBES=1`),
which carries BOTH shapes of every 256x256 kernel: the shape a kernel does not ship in the default library is covered here.  Run explicitly:

    python -m pytest tools/probes/test_probe_gemm_mfma_shape.py -q        (on a GPU box)
"""
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from test_gemm_mfma_shape_gpu import *  # noqa: E402,F401,F403  (the tests loop over ops.gemm_mfma_shapes(form): all of them on this build)
from test_gemm_mfma_shape_gpu import _ops  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="session")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def test_probe_build_carries_both_shapes(dev):
    from audio_flamingo_amd import _lib
    if not _lib.has_probes():
        pytest.skip("needs a -DAFK_PROBES build (make -C audio-flamingo_amd/csrc PROBES=1)")
    for form in ("nt", "nn", "tn"):
        assert _ops().gemm_mfma_shapes(form) == (1, 2)

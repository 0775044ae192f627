"""FillMedian across ranks: shells out to `torch.distributed.run`, so it collects last like the
other rehearsals (test_zz_rehearsals.py)."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.timeout(400)
def test_two_ranks_on_one_gpu_fit_the_median_of_the_union():
    """Two torchrun ranks share this GPU (gloo, collectives staged through the host); each fits
    its own 3 000-row frame.  tests/multirank_median_check.py asserts on every rank that the
    medians are bit-equal to pandas on the union: the per-pass histograms were summed over the
    ranks, so both stepped to the same prefix."""
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    port = 29300 + os.getpid() % 200
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
           "--master-addr", "127.0.0.1", "--master-port", str(port),
           os.path.join(ROOT, "tests", "multirank_median_check.py")]
    res = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=350)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-4000:]
    for r in (0, 1):
        assert f"rank {r}: FillMedian medians == pandas on the union" in res.stdout

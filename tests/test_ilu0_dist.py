# SPDX-License-Identifier: Apache-2.0
"""Multi-process ILU(0) (block-Jacobi): world sizes 2 and 3 over gloo on
CPU."""
import itertools
import os
import subprocess
import sys

import pytest

# own base port, 1200 above test_lobpcg_dist.py's: all counters add the
# same pid offset, so within one pytest process they never hand out the
# same port (the ranges over all pids do overlap)
_PORTS = itertools.count(35500 + (os.getpid() % 50) * 37)


def _run(nproc, timeout=300):
    env = dict(os.environ)
    env.setdefault("MASTER_ADDR", "127.0.0.1")
    # gloo on CPU also where a GPU is present: several ranks cannot share
    # one device under RCCL, so the workers see no device at all
    for var in ("HIP_VISIBLE_DEVICES", "CUDA_VISIBLE_DEVICES"):
        env[var] = ""
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    worker = os.path.join(repo, "tests", "dist_ilu0_worker.py")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1",
           f"--nproc-per-node={nproc}", "--master-addr", "127.0.0.1",
           "--master-port", str(next(_PORTS)), worker]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=timeout,
                       env=env, cwd=repo)
    assert r.returncode == 0, f"stdout:\n{r.stdout}\nstderr:\n{r.stderr}"
    assert "DIST_ILU0_OK" in r.stdout


@pytest.mark.parametrize("world", [2, 3])
def test_ilu0_distributed_cpu(world):
    _run(world)

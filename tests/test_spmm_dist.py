# SPDX-License-Identifier: Apache-2.0
"""Multi-process SpMM correctness: world sizes 2 and 3 over gloo on CPU
(the same exchange runs RCCL on GPU)."""
import itertools
import os
import subprocess
import sys

import pytest

# own port range, clear of test_distributed.py's counter
_PORTS = itertools.count(31900 + (os.getpid() % 50) * 37)


def _run(nproc, env_extra=None, timeout=300):
    env = dict(os.environ)
    env.setdefault("MASTER_ADDR", "127.0.0.1")
    env.update(env_extra or {})
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    worker = os.path.join(repo, "tests", "dist_spmm_worker.py")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1",
           f"--nproc-per-node={nproc}", "--master-addr", "127.0.0.1",
           "--master-port", str(next(_PORTS)), worker]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=timeout,
                       env=env, cwd=repo)
    assert r.returncode == 0, f"stdout:\n{r.stdout}\nstderr:\n{r.stderr}"
    assert "DIST_SPMM_OK" in r.stdout


@pytest.mark.parametrize("world", [2, 3])
def test_spmm_distributed_cpu(world):
    _run(world)


def test_spmm_distributed_coarse_images():
    _run(2, {"LS_PRECISE_IMAGES": "0"})

# SPDX-License-Identifier: Apache-2.0
"""Multi-process FSAI: world sizes 2 and 3 over gloo on CPU."""
import functools
import itertools
import os
import subprocess
import sys

import pytest

# own base port, 1200 above test_ilu0_dist.py's: all counters add the same
# pid offset, so within one pytest process they never hand out the same
# port (the ranges over all pids do overlap)
_PORTS = itertools.count(36700 + (os.getpid() % 50) * 37)

_REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_WORKER = os.path.join(_REPO, "tests", "dist_fsai_worker.py")


def _env():
    env = dict(os.environ)
    env.setdefault("MASTER_ADDR", "127.0.0.1")
    # gloo on CPU also where a GPU is present: several ranks cannot share
    # one device under RCCL, so the workers see no device at all
    for var in ("HIP_VISIBLE_DEVICES", "CUDA_VISIBLE_DEVICES"):
        env[var] = ""
    return env


@functools.lru_cache(maxsize=None)
def _world1_iters(timeout=300):
    """CG iterations on jump-48^2 with M = fsai(A) in ONE process on the
    CPU: what the distributed counts are compared against."""
    r = subprocess.run([sys.executable, _WORKER, "--iters"],
                       capture_output=True, text=True, timeout=timeout,
                       env=_env(), cwd=_REPO)
    assert r.returncode == 0, f"stdout:\n{r.stdout}\nstderr:\n{r.stderr}"
    line = [ln for ln in r.stdout.splitlines()
            if ln.startswith("FSAI_W1_ITERS")]
    assert line, r.stdout
    return int(line[0].split()[1])


def _run(nproc, timeout=300):
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1",
           f"--nproc-per-node={nproc}", "--master-addr", "127.0.0.1",
           "--master-port", str(next(_PORTS)), _WORKER, "--w1-iters",
           str(_world1_iters())]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=timeout,
                       env=_env(), cwd=_REPO)
    assert r.returncode == 0, f"stdout:\n{r.stdout}\nstderr:\n{r.stderr}"
    assert "DIST_FSAI_OK" in r.stdout


@pytest.mark.parametrize("world", [2, 3])
def test_fsai_distributed_cpu(world):
    _run(world)

# SPDX-License-Identifier: Apache-2.0
"""Drop-in fidelity: the reference's example programs run UNMODIFIED.

``examples/upstream/`` holds byte-identical copies of the reference's
user programs (pde.py, gmg.py, common.py, spmv/spgemm microbenchmarks).
These tests execute them with ``--package legate`` — the mode that, in
the reference, selects cupynumeric + legate_sparse — against this
framework's shims (cupynumeric/, legate/, legate_sparse.utils store
helpers), at world size 1 and under torchrun world size 2 (gloo on CPU),
and assert the programs' own convergence/residual gates.

Known reference-inherent non-convergent configurations (verified against
a pure-scipy oracle of the same algorithm, which stalls identically):
gmg ``-g linear`` (reference's linear_operator uses fine_dim where it
means fine_shape[1] in its bounds tests) and large-grid/deep-level
combinations where the 1-step power-iteration omega underestimates —
tests below use configurations that the algorithm itself converges on.
"""
import os
import subprocess
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UPSTREAM = os.path.join(REPO, "examples", "upstream")


def _run(args, world=1, timeout=600):
    env = dict(os.environ)
    env["PYTHONPATH"] = REPO + os.pathsep + env.get("PYTHONPATH", "")
    if world == 1:
        cmd = [sys.executable] + args
    else:
        port = str(28900 + abs(hash(tuple(args))) % 500)
        cmd = [sys.executable, "-m", "torch.distributed.run",
               "--nnodes=1", f"--nproc-per-node={world}",
               "--master-addr", "127.0.0.1", "--master-port", port] + args
    proc = subprocess.run(cmd, cwd=UPSTREAM, env=env, timeout=timeout,
                          capture_output=True, text=True)
    out = proc.stdout + proc.stderr
    assert proc.returncode == 0, out[-4000:]
    return out


@pytest.mark.parametrize("world", [1, 2])
def test_upstream_pde_unmodified(world):
    out = _run(["pde.py", "--package", "legate", "-n", "64", "-m", "64"],
               world=world)
    assert "CG converged" in out, out[-2000:]


@pytest.mark.parametrize("world", [1, 2])
def test_upstream_pde_throughput(world):
    out = _run(["pde.py", "--package", "legate", "-n", "64", "-m", "64",
                "-t", "-i", "30", "-w", "5"], world=world)
    assert "ms / iter" in out, out[-2000:]


@pytest.mark.parametrize("world", [1, 2])
def test_upstream_gmg_unmodified(world):
    # default problem (n=16, levels=2) — converges in the reference
    # algorithm; the program prints its own residual-gated verdict
    out = _run(["gmg.py", "--package", "legate"], world=world, timeout=900)
    assert "Converged in" in out, out[-2000:]


def test_upstream_gmg_n32():
    out = _run(["gmg.py", "--package", "legate", "-n", "32", "-l", "2",
                "-w"], timeout=900)
    assert "Converged in" in out, out[-2000:]


def test_upstream_gmg_diffusion():
    out = _run(["gmg.py", "--package", "legate", "-n", "32", "-l", "2",
                "-d", "diffusion"], timeout=900)
    assert "Converged in" in out, out[-2000:]


@pytest.mark.parametrize("world", [1, 2])
def test_upstream_spmv_microbenchmark(world):
    out = _run(["spmv_microbenchmark.py", "--package", "legate",
                "--nmin", "1k", "--nmax", "1k", "-i", "10"], world=world)
    assert "ms / iter" in out, out[-2000:]


def test_upstream_spmv_microbenchmark_repartition():
    out = _run(["spmv_microbenchmark.py", "--package", "legate",
                "--nmin", "1k", "--nmax", "1k", "-i", "10",
                "--repartition"])
    assert "ms / iter" in out, out[-2000:]


@pytest.mark.parametrize("world", [1, 2])
def test_upstream_spgemm_microbenchmark(world):
    out = _run(["spgemm_microbenchmark.py", "--package", "legate",
                "-n", "1k", "-i", "3"], world=world)
    assert "ms /" in out and "SPGEMM" in out, out[-2000:]


def test_upstream_files_byte_identical():
    """The harness only counts if the examples are truly unmodified:
    compare against the sha256 digests recorded from the reference's
    v24.11.01 examples (tests/golden/upstream_examples.sha256)."""
    import hashlib
    golden = os.path.join(REPO, "tests", "golden",
                          "upstream_examples.sha256")
    recorded = dict(reversed(line.split()) for line in open(golden))
    assert sorted(recorded) == ["common.py", "gmg.py", "pde.py",
                                "spgemm_microbenchmark.py",
                                "spmv_microbenchmark.py"]
    for name, a in recorded.items():
        b = hashlib.sha256(
            open(os.path.join(UPSTREAM, name), "rb").read()).hexdigest()
        assert a == b, f"{name} differs from the reference copy"


# ---------------------------------------------------------------------------
# GPU: the same unmodified programs on a real MI355X
# ---------------------------------------------------------------------------
@pytest.mark.gpu
def test_upstream_pde_gpu():
    out = _run(["pde.py", "--package", "legate", "-n", "256", "-m", "256"])
    assert "CG converged" in out, out[-2000:]


@pytest.mark.gpu
def test_upstream_pde_throughput_gpu():
    out = _run(["pde.py", "--package", "legate", "-n", "1024", "-m",
                "1024", "-t", "-i", "200", "-w", "50"])
    assert "ms / iter" in out, out[-2000:]


@pytest.mark.gpu
def test_upstream_gmg_gpu():
    out = _run(["gmg.py", "--package", "legate", "-n", "32", "-l", "2",
                "-w"], timeout=900)
    assert "Converged in" in out, out[-2000:]


@pytest.mark.gpu
def test_upstream_spmv_microbenchmark_gpu():
    out = _run(["spmv_microbenchmark.py", "--package", "legate",
                "--nmin", "64k", "--nmax", "64k", "-i", "50"])
    assert "ms / iter" in out, out[-2000:]

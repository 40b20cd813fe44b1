# SPDX-License-Identifier: Apache-2.0
"""The example drivers (the reference's headline workloads) run end-to-end
and pass their own residual checks."""
import os
import itertools
import subprocess
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


_PORTS = itertools.count(27900 + (os.getpid() % 50) * 37)


def _next_port() -> str:
    """Unique master port per torchrun invocation: back-to-back jobs on
    one port can cross-connect through lingering sockets (observed as a
    flaky gloo SIGABRT when the dist tests run consecutively)."""
    return str(next(_PORTS))


def _run(script, *args, timeout=300):
    r = subprocess.run([sys.executable, os.path.join(REPO, "examples",
                                                     script), *args],
                       capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, f"stdout:\n{r.stdout}\nstderr:\n{r.stderr}"
    return r.stdout


def test_pde_runs():
    out = _run("pde.py", "-n", "64")
    assert "PASS" in out


def test_pde_throughput_mode():
    out = _run("pde.py", "-n", "64", "--throughput", "-i", "20", "-w", "2")
    assert "ms/iter" in out


def test_gmg_runs():
    out = _run("gmg.py", "-k", "5")
    assert "PASS" in out


def test_gmg_diffusion():
    """-d diffusion instance (reference gmg.py:430-438 parity)."""
    out = _run("gmg.py", "-k", "5", "-d", "diffusion")
    assert "PASS" in out


def test_gmg_injection_gridop():
    """--gridop injection (reference gmg.py:448-456 parity)."""
    out = _run("gmg.py", "-k", "5", "-g", "injection", "--maxiter", "400")
    assert "PASS" in out


def test_spmv_microbenchmark():
    out = _run("spmv_microbenchmark.py", "--nmin", "4096", "--nmax", "8192",
               "-i", "3", "-w", "1")
    assert "ms/iter" in out or "GFLOP" in out


def test_spgemm_microbenchmark():
    out = _run("spgemm_microbenchmark.py", "-n", "4096", "-i", "2", "-w",
               "1")
    assert "ms/iter" in out


def test_bench_contract():
    """bench.py prints exactly one valid JSON line with required keys."""
    import json
    r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"),
                        "--nx", "128", "--steps", "5", "--warmup", "1",
                        "--spgemm-iters", "1"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    line = [l for l in r.stdout.splitlines() if l.startswith("{")][-1]
    d = json.loads(line)
    for key in ("metric", "value", "unit", "n_gpus", "steps", "warmup",
                "ms_per_step", "higher_is_better", "scaling",
                "vs_baseline", "dtype", "data", "config"):
        assert key in d, key
    assert d["n_gpus"] == 1
    assert d["scaling"] == "weak"


def _bench(*args):
    import json
    r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"),
                        "--nx", "96", "--steps", "3", "--warmup", "1",
                        "--inner", "2", *args],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


_SECONDARY_KEYS = ("spgemm_nnz_per_s", "spgemm_ms_per_iter",
                   "spgemm_out_nnz", "cg_ms_per_iter", "cg_gflops")


def test_bench_dump_outputs(tmp_path):
    """A plain run reports only the headline; --dump-outputs writes the
    last step's y, identical from run to run and equal to A @ x."""
    import numpy as np
    import scipy.sparse as sp
    dirs = [tmp_path / "a", tmp_path / "b"]
    for d in dirs:
        res = _bench("--dump-outputs", str(d))
        assert res["steps"] == 3 and res["ms_per_step"] > 0
        for key in _SECONDARY_KEYS:
            assert key not in res["config"], key
        assert sorted(p.name for p in d.iterdir()) == ["y.npy"]
    ya, yb = (np.load(d / "y.npy") for d in dirs)
    assert ya.dtype == np.float64 and ya.shape == (96 * 96,)
    assert np.array_equal(ya, yb)
    # y = A @ x with x in [0, 1): the 5-pt operator bounds |y| by 8 and
    # a random x cannot give the zero vector
    assert np.all(np.isfinite(ya)) and np.abs(ya).max() <= 8.0
    assert np.abs(ya).max() > 0
    T = sp.diags([-1.0, 2.0, -1.0], [-1, 0, 1], shape=(96, 96))
    L = sp.kronsum(T, T).tocsr()
    # A is symmetric positive definite, so x is recoverable from y: the
    # dump really is the product of the operator with some x in [0, 1)
    from scipy.sparse.linalg import spsolve
    x = spsolve(L.tocsc(), ya)
    assert x.min() > -1e-9 and x.max() < 1 + 1e-9


def test_bench_full_reports_secondary_sections():
    res = _bench("--full", "--spgemm-iters", "1")
    for key in _SECONDARY_KEYS:
        assert key in res["config"], key
    assert res["config"]["spgemm_out_nnz"] > res["config"]["nnz"]


@pytest.mark.gpu
def test_pde_gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    out = _run("pde.py", "-n", "256")
    assert "PASS" in out


@pytest.mark.gpu
def test_gmg_gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    out = _run("gmg.py", "-k", "7")
    assert "PASS" in out


@pytest.mark.gpu
def test_gmg_diffusion_gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    out = _run("gmg.py", "-k", "7", "-d", "diffusion")
    assert "PASS" in out


def test_pde_exact_mode():
    out = _run("pde.py", "-n", "48", "--exact")
    assert "PASS" in out

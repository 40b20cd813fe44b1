# SPDX-License-Identifier: Apache-2.0
"""Worker for the multi-process SpMM checks (launched by test_spmm_dist.py
through torch.distributed.run, world_size >= 2, gloo on CPU).

Every rank builds the same global operands, the library shards them, and
each case compares the all-gathered (M, k) result with scipy on EVERY
rank.  Exits nonzero on any mismatch; prints DIST_SPMM_OK at the end.
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np
import scipy.sparse as sp
import torch
import torch.distributed as dist

import legate_sparse as lsp
from legate_sparse import comm
from legate_sparse.runtime import runtime
from testutils import banded_matrix, to_np

K = 3


def check(name, cond):
    if not cond:
        print(f"[rank {runtime.rank}] FAIL: {name}", flush=True)
        sys.exit(1)
    if runtime.rank == 0:
        print(f"[rank 0] ok: {name}", flush=True)


def gathered(Y, M):
    """All-gather the local (rows, K) blocks into the global (M, K)."""
    counts = [c * K for c in runtime.partition(M).counts()]
    flat = comm.allgatherv(Y.as_subclass(torch.Tensor).reshape(-1), counts)
    return to_np(flat).reshape(M, K)


def run_case(name, S):
    M, N = S.shape
    X = np.random.default_rng(11).standard_normal((N, K))
    want = S @ X
    A = lsp.csr_array(S)
    lo, hi = runtime.local_range(N)
    for label, op in (("shard", X[lo:hi]), ("replicated", X)):
        Y = A.matmat(np.ascontiguousarray(op))
        rlo, rhi = A.row_range
        check(f"{name} {label} local shape",
              tuple(Y.shape) == (rhi - rlo, K))
        check(f"{name} {label}",
              np.allclose(gathered(Y, M), want, rtol=1e-10, atol=1e-12))
    return A, X, want


def block_diagonal(n, ws):
    """Diagonal blocks aligned with the equal partition: no rank reads a
    remote column (the any_halo == False branch on every rank)."""
    part = runtime.partition(n)
    rng = np.random.default_rng(5)
    blocks = [rng.standard_normal((part.count(r), part.count(r)))
              for r in range(ws)]
    return sp.csr_array(sp.block_diag(blocks, format="csr"))


def restriction(m, n):
    """2:1 full-weighting-like restriction: row i reads columns
    2i, 2i+1, 2i+2 — low ranks' windows stay inside their own shard of x
    while higher ranks reach into remote shards (asymmetric halos)."""
    rows = np.repeat(np.arange(m), 3)
    cols = (2 * np.arange(m)[:, None] + np.arange(3)[None, :]).reshape(-1)
    vals = np.tile([0.25, 0.5, 0.25], m)
    return sp.csr_array((vals, (rows, cols)), shape=(m, n))


def main():
    ws = runtime.world_size
    assert ws >= 2, "needs torchrun world_size >= 2"
    coarse = os.environ.get("LS_PRECISE_IMAGES") == "0"

    # banded 41x41: halos on both sides, unequal tail shard at world 3
    A, X, want = run_case("banded", sp.csr_array(banded_matrix(41, 7)))
    if not coarse:
        check("banded has halo", A._halo_plan()["any_halo"])

    # out= rules at world_size > 1
    M = 41
    rlo, rhi = A.row_range
    lo, hi = runtime.local_range(M)
    out_n = np.full((M, K), np.nan)
    r = A.matmat(np.ascontiguousarray(X[lo:hi]), out=out_n)
    check("numpy out global filled",
          r is out_n and np.allclose(out_n, want, rtol=1e-10, atol=1e-12))
    try:
        A.matmat(X, out=np.empty((rhi - rlo, K)))
        ok = False
    except ValueError:
        ok = True
    check("numpy out of local shape raises", ok)
    out_t = torch.full((rhi - rlo, K), float("nan"), dtype=torch.float64)
    A.matmat(X, out=out_t)
    check("torch out local filled",
          np.allclose(gathered(out_t, M), want, rtol=1e-10, atol=1e-12))
    try:
        A.matmat(X[:hi - lo + 1] if hi - lo + 1 != M else X[:1])
        ok = False
    except ValueError:
        ok = True
    check("bad X row count raises", ok)

    if not coarse:
        Ab, _, _ = run_case("block-diagonal", block_diagonal(41, ws))
        check("block-diagonal has no halo",
              not Ab._halo_plan()["any_halo"])
        Ar, _, _ = run_case("restriction", restriction(20, 41))
        check("restriction has halo", Ar._halo_plan()["any_halo"])
        mine = Ar._split_for_overlap()[1][1].numel() > 0
        flags = comm.allgather_scalars(int(mine)).tolist()
        check("restriction halo is asymmetric",
              0 < sum(flags) < ws)

    dist.barrier()
    if runtime.rank == 0:
        print("DIST_SPMM_OK", flush=True)


if __name__ == "__main__":
    main()

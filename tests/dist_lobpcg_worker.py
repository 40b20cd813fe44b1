# SPDX-License-Identifier: Apache-2.0
"""Worker for the multi-process LOBPCG checks (launched by
test_lobpcg_dist.py through torch.distributed.run, world_size >= 2).

Every rank builds the same global matrix, the library shards it, and each
rank checks the eigenvalues and the all-gathered eigenvectors against the
replicated scipy matrix.  All ranks must take the same number of
iterations.  Exits nonzero on any mismatch; prints DIST_LOBPCG_OK at the
end.
"""
import os
import sys
import warnings

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np
import torch
import torch.distributed as dist

import legate_sparse as lsp
from legate_sparse import comm
from legate_sparse.runtime import runtime
from testutils import to_np
import lobpcg_cases as lc

TOL = 1e-6


def check(name, cond):
    if not cond:
        print(f"[rank {runtime.rank}] FAIL: {name}", flush=True)
        sys.exit(1)
    if runtime.rank == 0:
        print(f"[rank 0] ok: {name}", flush=True)


def run(case, k, largest, shard_x):
    S, _, exact = lc.matrix(case)
    n = S.shape[0]
    name = f"{case} k={k} largest={largest} shard_x={shard_x}"
    X = lc.start_block(n, k, np.float64, seed=1)
    lo, hi = runtime.local_range(n)
    budget = 2 * lc.scipy_iterations(case, k, largest, "float64", TOL, 1) + 10
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        w, V, hist = lsp.linalg.lobpcg(
            lsp.csr_array(S), X[lo:hi] if shard_x else X, tol=TOL,
            maxiter=budget, largest=largest, retResidualNormsHistory=True)
    its = comm.allgather_scalars(lc.iterations(hist)).tolist()
    check(f"{name}: same iteration count on all ranks {its}",
          len(set(its)) == 1)
    check(f"{name}: local rows returned", tuple(V.shape) == (hi - lo, k))
    Vl = torch.as_tensor(to_np(V)).contiguous()
    counts = [c * k for c in runtime.partition(n).counts()]
    Vf = to_np(comm.allgatherv(Vl.reshape(-1), counts)).reshape(n, k)
    err = np.abs(w - lc.extremal(exact, k, largest))
    check(f"{name}: eigenvalues {err.max():.2e}", np.all(err <= TOL))
    res = np.linalg.norm(S @ Vf - Vf * w[None, :], axis=0)
    check(f"{name}: residuals {res.max():.2e}", np.all(res <= TOL))


def main():
    ws = runtime.world_size
    assert ws >= 2, "needs torchrun world_size >= 2"
    # n = 256 is ragged at world size 3, n = 225 at world size 2
    for case in ("poisson", "poisson15"):
        run(case, 4, False, shard_x=False)
        run(case, 4, False, shard_x=True)
    run("poisson", 5, True, shard_x=True)
    dist.barrier()
    if runtime.rank == 0:
        print("DIST_LOBPCG_OK", flush=True)


if __name__ == "__main__":
    main()

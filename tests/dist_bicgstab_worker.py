# SPDX-License-Identifier: Apache-2.0
"""Worker for the multi-process BiCGSTAB checks (launched by
test_bicgstab_dist.py through torch.distributed.run, world_size >= 2).

Every rank builds the same global system, the library shards it, and each
rank checks the all-gathered solution against the replicated scipy matrix.
All ranks must leave the solver with the same ``info``.  Exits nonzero on
any mismatch; prints DIST_BICGSTAB_OK at the end.
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np
import scipy.sparse as sp
import torch.distributed as dist

import legate_sparse as lsp
from legate_sparse import comm
from legate_sparse import utils as lsu
from legate_sparse.runtime import runtime
from testutils import to_np
import bicgstab_cases as bc


def check(name, cond):
    if not cond:
        print(f"[rank {runtime.rank}] FAIL: {name}", flush=True)
        sys.exit(1)
    if runtime.rank == 0:
        print(f"[rank 0] ok: {name}", flush=True)


def solve(name, A, S, b, rtol, want_info=0, **kw):
    n = S.shape[0]
    calls = []
    x, info = lsp.linalg.bicgstab(A, b, rtol=rtol,
                                  callback=lambda xk: calls.append(1), **kw)
    infos = comm.allgather_scalars(int(info)).tolist()
    check(f"{name}: same info on all ranks {infos}",
          all(i == want_info for i in infos))
    lo, hi = runtime.local_range(n)
    check(f"{name}: local shard returned", x.numel() == hi - lo)
    iters = comm.allgather_scalars(len(calls)).tolist()
    check(f"{name}: same iteration count on all ranks {iters}",
          len(set(iters)) == 1)
    xf = to_np(lsu.full_vector(x, n))
    check(f"{name}: finite", np.isfinite(xf).all())
    return xf


def main():
    ws = runtime.world_size
    assert ws >= 2, "needs torchrun world_size >= 2"

    # convection-diffusion 24x24, scipy-built and stencil-built
    S = bc.convdiff(24, 24)
    b = bc.rhs(576, np.float64)
    for label, A in (("csr", lsp.csr_array(S)),
                     ("stencil", bc.convdiff_lsp(24, 24))):
        xf = solve(f"convdiff {label}", A, S, b, 1e-10)
        check(f"convdiff {label}: residual",
              bc.rel_residual(S, xf, b) <= 1e-9)

    # local-shard right-hand side and x0
    xf = solve("convdiff shard rhs", lsp.csr_array(S), S,
               lsu.local_vector(b, 576), 1e-10,
               x0=lsu.local_vector(bc.rhs(576, np.float64, seed=8), 576))
    check("convdiff shard rhs: residual", bc.rel_residual(S, xf, b) <= 1e-9)

    # 3x3: converges within three iterations and then runs frozen up to
    # the first convergence test (one-row shards at world size 3)
    D = np.array([[4.0, 1, 0], [2, 5, 1], [0, 1, 3]])
    b3 = np.array([1.0, 2.0, 3.0])
    xf = solve("3x3", lsp.csr_array(sp.csr_array(D)), sp.csr_array(D), b3,
               1e-12, conv_test_iters=25)
    check("3x3: residual",
          np.linalg.norm(b3 - D @ xf) <= 1e-12 * np.linalg.norm(b3))

    # 5-step replay: the three all-reduces feed the same recurrence
    xf = solve("replay", lsp.csr_array(S), S, b, 0, want_info=5, maxiter=5,
               conv_test_iters=5)
    want = bc.np_replay(S, b, 5)
    check("replay: matches numpy",
          np.linalg.norm(xf - want) <= 1e-10 * np.linalg.norm(want))

    dist.barrier()
    if runtime.rank == 0:
        print("DIST_BICGSTAB_OK", flush=True)


if __name__ == "__main__":
    main()

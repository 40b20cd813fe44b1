# SPDX-License-Identifier: Apache-2.0
"""Worker for the multi-process ILU(0) checks (launched by
test_ilu0_dist.py through torch.distributed.run, world_size >= 2).

Every rank builds the same global system and the library shards it.  The
preconditioner is block-Jacobi: each rank's factor must equal the reference
ILU(0) of its own diagonal block, the apply touches only the rank's shard,
and every raise-or-not decision is the same on all ranks.  Exits nonzero on
any mismatch; prints DIST_ILU0_OK at the end.
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
import ilu0_cases as ic


def check(name, cond):
    if not cond:
        print(f"[rank {runtime.rank}] FAIL: {name}", flush=True)
        sys.exit(1)
    if runtime.rank == 0:
        print(f"[rank 0] ok: {name}", flush=True)


def all_true(flag):
    return all(int(v) == 1 for v in
               comm.allgather_scalars(1 if flag else 0).tolist())


def raises(exc, fn):
    try:
        fn()
    except exc as e:
        return str(e)
    return None


def solve(A, b, M):
    calls = []
    x, info = lsp.linalg.bicgstab(A, b, rtol=1e-8, M=M, conv_test_iters=1,
                                  callback=lambda xk: calls.append(1))
    infos = comm.allgather_scalars(int(info)).tolist()
    check(f"bicgstab info 0 on all ranks {infos}", all(i == 0 for i in infos))
    return to_np(lsu.full_vector(x, b.size)), len(calls)


def main():
    ws = runtime.world_size
    assert ws >= 2, "needs torchrun world_size >= 2"

    # convection-diffusion 24x24: per-rank factor == ILU(0) of the block
    S = bc.convdiff(24, 24)
    n = S.shape[0]
    A = lsp.csr_array(S)
    M = lsp.linalg.ilu0(A)
    lo, hi = runtime.local_range(n)
    block = sp.csr_matrix(S[lo:hi, lo:hi])
    block.sort_indices()
    ref = ic.ilu0_reference(block)
    ip, ix, fv = M.factor_local()
    check("factor pattern is the diagonal block",
          np.array_equal(to_np(ip), ref.indptr)
          and np.array_equal(to_np(ix), ref.indices))
    check("factor values equal the block's reference ILU(0)",
          np.allclose(to_np(fv), ref.data, **ic.tol(np.float64)))

    # the apply works on this rank's shard only
    r = ic.rhs(n, None, np.float64)
    want = ic.ilu_apply_reference(ref, r[lo:hi])
    got = to_np(M.matvec(r))               # global vector in, shard out
    check("matvec: shard of the block solve",
          got.shape == (hi - lo,) and np.allclose(got, want,
                                                  **ic.tol(np.float64)))
    got = to_np(M.matvec(lsu.local_vector(r, n)))
    check("matvec: local shard in",
          np.allclose(got, want, **ic.tol(np.float64)))
    R = ic.rhs(n, 5, np.float64)
    blk = to_np(M.matmat(R))
    cols = np.stack([ic.ilu_apply_reference(ref, R[lo:hi, j].copy())
                     for j in range(5)], axis=1)
    check("matmat: shard of the block solves",
          blk.shape == (hi - lo, 5) and np.allclose(blk, cols,
                                                    **ic.tol(np.float64)))

    # block-Jacobi ILU(0) still more than halves the BiCGSTAB iterations
    b = ic.rhs(n, None, np.float64, seed=9)
    x0, plain = solve(A, b, None)
    x1, pre = solve(A, b, M)
    if runtime.rank == 0:
        print(f"[rank 0] bicgstab iterations: M=None {plain}, "
              f"M=ilu0 {pre}", flush=True)
    check("preconditioned residual", bc.rel_residual(S, x1, b) <= 1e-7)
    check("fewer than half the unpreconditioned iterations",
          2 * pre < plain)

    # refactor on the same pattern, refused on another one (on all ranks)
    S2 = sp.csr_array(S * 2.0 + sp.identity(n))
    S2.sort_indices()
    M.refactor(lsp.csr_array(S2))
    ref2 = ic.ilu0_reference(sp.csr_matrix(S2[lo:hi, lo:hi]))
    check("refactor values",
          np.allclose(to_np(M.factor_local()[2]), ref2.data,
                      **ic.tol(np.float64)))
    other = sp.lil_matrix(S)
    other[0, 5] = 1.0                      # one more entry in rank 0's rows
    msg = raises(ValueError,
                 lambda: M.refactor(lsp.csr_array(sp.csr_array(
                     other.tocsr()))))
    check("refactor with another pattern raises on all ranks",
          all_true(msg is not None))

    # a zero pivot in the LAST rank's block raises on all ranks, naming
    # the global row
    lo_last = runtime.partition(n).lo(ws - 1)
    Z = sp.lil_matrix(S)
    for i in (lo_last, lo_last + 1):
        Z[i, :] = 0
        Z[:, i] = 0
    Z[lo_last, lo_last] = Z[lo_last + 1, lo_last + 1] = 1.0
    Z[lo_last, lo_last + 1] = Z[lo_last + 1, lo_last] = 1.0
    Z = sp.csr_array(Z.tocsr())
    Z.eliminate_zeros()
    msg = raises(RuntimeError, lambda: lsp.linalg.ilu0(lsp.csr_array(Z)))
    check("zero pivot raises on all ranks", all_true(msg is not None))
    check("zero pivot names the global row",
          all_true(msg is not None and f"row {lo_last + 1}" in msg))

    # a missing diagonal entry on one rank: ValueError everywhere
    D = sp.lil_matrix(S)
    D[lo_last + 2, lo_last + 2] = 0
    D = sp.csr_array(D.tocsr())
    D.eliminate_zeros()
    msg = raises(ValueError, lambda: lsp.linalg.ilu0(lsp.csr_array(D)))
    check("missing diagonal raises on all ranks", all_true(msg is not None))

    # no distributed triangular solve
    T = lsp.csr_array(ic.tri_matrix("rand300", True, np.float64))
    msg = raises(NotImplementedError,
                 lambda: lsp.linalg.spsolve_triangular(
                     T, ic.rhs(300, None, np.float64)))
    check("spsolve_triangular raises NotImplementedError on all ranks",
          all_true(msg is not None and "pipeline" in msg))

    dist.barrier()
    if runtime.rank == 0:
        print("DIST_ILU0_OK", flush=True)


if __name__ == "__main__":
    main()

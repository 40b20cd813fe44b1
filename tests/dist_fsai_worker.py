# SPDX-License-Identifier: Apache-2.0
"""Worker for the multi-process FSAI checks (launched by test_fsai_dist.py
through torch.distributed.run, world_size >= 2).

Every rank builds the same global system and the library shards it.  The
rows of G a rank owns need rows of A that earlier ranks own (the window
gather); the result must be the world-size-1 factor, row for row, the apply
must be exact, and every raise-or-not decision must be the same on all
ranks.  Exits nonzero on any mismatch; prints DIST_FSAI_OK at the end.

Run directly with ``--iters`` (one process) it prints the world-size-1 CG
iteration count the distributed run is compared against.
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np
import scipy.sparse as sp

import legate_sparse as lsp
from legate_sparse import comm
from legate_sparse import utils as lsu
from legate_sparse.runtime import runtime
from testutils import to_np
import fsai_cases as fc


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


def jump_cg(M_of):
    S = fc.matrix("jump48")
    A = lsp.csr_array(S)
    b = fc.rhs(S.shape[0], None, np.float64, seed=9)
    x, it = lsp.linalg.cg(A, b, rtol=1e-8, M=M_of(A), maxiter=5000)
    x = to_np(lsu.full_vector(x, b.size))
    return it, np.linalg.norm(b - S @ x) / np.linalg.norm(b)


def main():
    if "--iters" in sys.argv:
        it, _ = jump_cg(lambda A: lsp.linalg.fsai(A))
        print(f"FSAI_W1_ITERS {it}", flush=True)
        return
    import torch.distributed as dist

    ws = runtime.world_size
    assert ws >= 2, "needs torchrun world_size >= 2"
    w1_iters = int(sys.argv[sys.argv.index("--w1-iters") + 1])

    # band9: n = 41, the last rank's shard is short at world sizes 2 and 3
    cases = (("band9", "given", np.float64), ("grid33x17", 3, np.float64),
             ("grid9x8x7", 2, np.float32), ("herm300", 1, np.complex128))
    for name, p, dtype in cases:
        S = fc.matrix(name, dtype)
        P, want = fc.reference(name, p, dtype)
        n = S.shape[0]
        lo, hi = runtime.local_range(n)
        if name == "band9":
            counts = runtime.partition(n).counts()
            check(f"band9: short last shard {counts}",
                  counts[-1] < counts[0])
        A = lsp.csr_array(S)
        pat = lsp.csr_array(P) if p == "given" else p
        M = lsp.linalg.fsai(A, pat)
        s, e = P.indptr[lo], P.indptr[hi]
        tag = f"{name} p={p} {np.dtype(dtype).name}"
        check(f"{tag}: G's pattern is the reference's rows [{lo}, {hi})",
              all_true(np.array_equal(to_np(M.G.indptr), P.indptr[lo:hi + 1]
                                      - s)
                       and np.array_equal(to_np(M.G.indices), P.indices[s:e])))
        check(f"{tag}: G's values equal the world-1 reference",
              all_true(np.allclose(to_np(M.G.data), want[s:e],
                                   **fc.tol(dtype))))
        GHref = sp.csr_array(sp.csr_array(
            (want, P.indices, P.indptr), shape=P.shape).conj().T)
        GHref.sort_indices()
        s2, e2 = GHref.indptr[lo], GHref.indptr[hi]
        check(f"{tag}: GH is the conjugate transpose",
              all_true(np.array_equal(to_np(M.GH.indices),
                                      GHref.indices[s2:e2])
                       and np.allclose(to_np(M.GH.data), GHref.data[s2:e2],
                                       **fc.tol(dtype))))

        r = fc.rhs(n, None, dtype)
        full = fc.apply_reference(P, want, r)
        got = to_np(M.matvec(r))           # global vector in, shard out
        check(f"{tag}: matvec, global vector in",
              all_true(got.shape == (hi - lo,)
                       and np.allclose(got, full[lo:hi], **fc.tol(dtype))))
        got = to_np(M.matvec(lsu.local_vector(r, n)))
        check(f"{tag}: matvec, local shard in",
              all_true(np.allclose(got, full[lo:hi], **fc.tol(dtype))))
        R = fc.rhs(n, 5, dtype)
        blk = to_np(M.matmat(R))
        check(f"{tag}: matmat",
              all_true(blk.shape == (hi - lo, 5) and np.allclose(
                  blk, fc.apply_reference(P, want, R)[lo:hi],
                  **fc.tol(dtype))))

    # refactor on the same pattern; another pattern raises on all ranks
    S = fc.matrix("grid33x17")
    n = S.shape[0]
    lo, hi = runtime.local_range(n)
    M = lsp.linalg.fsai(lsp.csr_array(S), 2)
    r = fc.rhs(n, None, np.float64)
    S2 = sp.csr_array(S * 2.5 + sp.identity(n))
    S2.sort_indices()
    M.refactor(lsp.csr_array(S2))
    P = fc.pattern("grid33x17", 2)
    want2 = fc.reference_rows(S2, P)
    check("refactor values", all_true(np.allclose(
        to_np(M.G.data), want2[P.indptr[lo]:P.indptr[hi]],
        **fc.tol(np.float64))))
    fresh = lsp.linalg.fsai(lsp.csr_array(S2), 2)
    check("refactor: GH through the stored permutation equals a fresh one",
          all_true(bool((M.GH.data == fresh.GH.data).all())
                   and bool((M.GH.indices == fresh.GH.indices).all())))
    full = to_np(lsu.full_vector(fresh.matvec(r), n))
    got = to_np(lsu.full_vector(M.matvec(r), n))
    check("refactor: the apply equals a fresh operator's",
          all_true(np.array_equal(got, full)))
    M.refactor(lsp.csr_array(S))            # second use of the permutation
    back = lsp.linalg.fsai(lsp.csr_array(S), 2)
    check("refactor back: G and GH equal a fresh build",
          all_true(bool((M.G.data == back.G.data).all())
                   and bool((M.GH.data == back.GH.data).all())))
    other = sp.lil_matrix(S)
    other[0, 5] = other[5, 0] = -0.5       # one more entry in rank 0's rows
    msg = raises(ValueError, lambda: M.refactor(lsp.csr_array(sp.csr_array(
        other.tocsr()))))
    check("refactor with another pattern raises on all ranks",
          all_true(msg is not None))

    # CG on jump-48^2: the apply is exact, so the count is the world-1 one
    it, res = jump_cg(lambda A: lsp.linalg.fsai(A))
    if runtime.rank == 0:
        print(f"[rank 0] cg on jump48 with fsai: {it} iterations (world 1: "
              f"{w1_iters}), true relative residual {res:.2e}", flush=True)
    check("cg converged", all_true(res <= 1e-7))
    check("cg iterations <= world-1 iterations + 2",
          all_true(it <= w1_iters + 2))

    # the row limit: the long row lives on the last rank, all ranks raise
    D = lsp.csr_array(fc.matrix("dense33"))
    msg = raises(ValueError, lambda: lsp.linalg.fsai(
        D, lsp.csr_array(fc.pattern("dense33", "given"))))
    check("row limit raises on all ranks, naming the global row",
          all_true(msg is not None and "row 32 " in msg
                   and "FSAI_MAX_ROW = 32" in msg))

    # not positive definite in the LAST rank's rows: all ranks raise,
    # naming the global row
    n = 30
    bad_row = runtime.partition(n).lo(ws - 1) + 2
    msg = raises(RuntimeError, lambda: lsp.linalg.fsai(
        lsp.csr_array(fc.indefinite_block(bad_row))))
    check("indefinite matrix raises on all ranks",
          all_true(msg is not None))
    check("indefinite matrix names the global row",
          all_true(msg is not None and msg.endswith(f"row {bad_row}")))

    # a missing diagonal entry in the pattern on one rank
    P = sp.lil_matrix(fc.pattern("grid33x17", 1))
    P[3, 3] = 0
    P = sp.csr_array(P.tocsr())
    P.eliminate_zeros()
    msg = raises(ValueError, lambda: lsp.linalg.fsai(
        lsp.csr_array(fc.matrix("grid33x17")), lsp.csr_array(P)))
    check("missing diagonal raises on all ranks", all_true(msg is not None))

    dist.barrier()
    if runtime.rank == 0:
        print("DIST_FSAI_OK", flush=True)


if __name__ == "__main__":
    main()

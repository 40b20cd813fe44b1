# SPDX-License-Identifier: Apache-2.0
"""linalg.ilu0 on the CPU path: factor values against the pure-Python IKJ
reference, the apply against scipy's two triangular solves, refactor, the
error paths and the solvers that take it as M (docs/DESIGN.md §17)."""
import numpy as np
import pytest
import scipy.sparse as sp

import legate_sparse as lsp
from legate_sparse import linalg
from testutils import to_np
import ilu0_cases as ic

torch = pytest.importorskip("torch")

_DT = {"grid33x17": ic.DTYPES[:2], "grid9x8x7": ic.DTYPES[:2],
       "rand300sym": ic.DTYPES, "complex": ic.DTYPES[2:]}
CASES = [(n, d) for n in ic.ILU_NAMES for d in _DT[n]]


def _abs_tol(dtype, scale):
    t = ic.tol(dtype)
    return max(t["rtol"], t["atol"]) * scale


@pytest.mark.parametrize("name,dtype", CASES)
def test_factor_and_apply(name, dtype):
    A = ic.ilu_matrix(name, dtype)
    n = A.shape[0]
    F = ic.ilu0_reference(A)
    M = linalg.ilu0(lsp.csr_array(A))
    assert isinstance(M, linalg.LinearOperator) and M.shape == A.shape
    assert M.dtype == A.dtype
    ip, ix, fv = M.factor_local()
    assert np.array_equal(to_np(ip), F.indptr)
    assert np.array_equal(to_np(ix), F.indices)
    np.testing.assert_allclose(to_np(fv), F.data, **ic.tol(dtype))

    # L, U: unit diagonal stored; (L U - A) vanishes on A's pattern
    L = sp.csr_matrix((to_np(M.L.data), to_np(M.L.indices),
                       to_np(M.L.indptr)), shape=A.shape)
    U = sp.csr_matrix((to_np(M.U.data), to_np(M.U.indices),
                       to_np(M.U.indptr)), shape=A.shape)
    assert np.all(L.diagonal() == 1) and sp.triu(L, 1).nnz == 0
    assert sp.tril(U, -1).nnz == 0
    w = ic.wide(dtype)
    R = (L.astype(w) @ U.astype(w) - A.astype(w)).tocsr()
    coo = A.tocoo()
    on_pattern = np.abs(np.asarray(R[coo.row, coo.col]).reshape(-1))
    print(f"{name} {np.dtype(dtype).name}: max |LU - A| on pattern "
          f"{on_pattern.max():.3e}")
    assert on_pattern.max() <= _abs_tol(dtype, np.abs(A.data).max())

    r = ic.rhs(n, None, A.dtype)
    want = ic.ilu_apply_reference(F, r)
    np.testing.assert_allclose(to_np(M.matvec(r)), want, **ic.tol(dtype))
    np.testing.assert_allclose(to_np(M.solve(r)), want, **ic.tol(dtype))
    out = torch.empty(n, dtype=torch.from_numpy(r).dtype)
    assert M.matvec(torch.from_numpy(r), out=out) is out
    np.testing.assert_allclose(out.numpy(), want, **ic.tol(dtype))

    for k in (5, 40):
        Rb = ic.rhs(n, k, A.dtype, seed=k)
        got = to_np(M.matmat(Rb))
        assert got.shape == (n, k)
        for j in range(k):
            col = to_np(M.matvec(np.ascontiguousarray(Rb[:, j])))
            assert np.array_equal(got[:, j], col) or np.allclose(
                got[:, j], col, **ic.tol(dtype))
    with pytest.raises(NotImplementedError):
        M.rmatvec(r)
    with pytest.raises(NotImplementedError):
        M.rmatmat(Rb)


@pytest.mark.parametrize("name", ["grid33x17", "rand300sym", "arrow600sym"])
def test_torch_arm_factor(name):
    A = ic.ilu_matrix(name, np.float64)
    F = ic.ilu0_reference(A)
    M = linalg.ILU0(lsp.csr_array(A), _impl="torch")
    np.testing.assert_allclose(to_np(M.factor_local()[2]), F.data,
                               **ic.tol(np.float64))
    r = ic.rhs(A.shape[0], None, np.float64)
    np.testing.assert_allclose(to_np(M.matvec(r)),
                               ic.ilu_apply_reference(F, r),
                               **ic.tol(np.float64))


def test_symmetric_operator_for_spd():
    """SPD A, symmetric pattern: U = D L^T, so U^-1 L^-1 is symmetric."""
    A = ic.poisson2d(9, 7)
    M = linalg.ilu0(lsp.csr_array(A))
    n = A.shape[0]
    Minv = to_np(M.matmat(np.eye(n)))
    np.testing.assert_allclose(Minv, Minv.T, rtol=1e-10, atol=1e-12)
    assert np.linalg.eigvalsh((Minv + Minv.T) / 2).min() > 0


def test_refactor():
    A = ic.ilu_matrix("grid33x17", np.float64)
    La = lsp.csr_array(A)
    M = linalg.ilu0(La)
    sched = M._sched_l
    A2 = sp.csr_array(A * 2.5 + sp.identity(A.shape[0]))
    A2.sort_indices()
    assert M.refactor(lsp.csr_array(A2)) is M
    assert M._sched_l is sched                      # analysis reused
    fresh = linalg.ilu0(lsp.csr_array(A2))
    assert np.array_equal(to_np(M.factor_local()[2]),
                          to_np(fresh.factor_local()[2]))
    with pytest.raises(ValueError):
        M.refactor(lsp.csr_array(ic.ilu_matrix("grid9x8x7", np.float64)))
    other = sp.lil_matrix(A)
    other[0, 5] = 1.0                               # same shape, new entry
    with pytest.raises(ValueError):
        M.refactor(lsp.csr_array(sp.csr_array(other.tocsr())))


def test_errors():
    A = sp.lil_matrix(ic.ilu_matrix("grid33x17", np.float64))
    A[3, 3] = 0
    A = sp.csr_array(A.tocsr())
    A.eliminate_zeros()
    with pytest.raises(ValueError, match="diagonal"):
        linalg.ilu0(lsp.csr_array(A))
    with pytest.raises(ValueError):
        linalg.ilu0(lsp.csr_array(
            ic.ilu_matrix("grid33x17", np.float64)[:, :500]))
    with pytest.raises(RuntimeError, match=r"row 1\b"):
        linalg.ilu0(lsp.csr_array(ic.zero_pivot_matrix()))
    with pytest.raises(RuntimeError, match=r"row 1\b"):
        linalg.ILU0(lsp.csr_array(ic.zero_pivot_matrix()), _impl="torch")
    N = ic.ilu_matrix("grid33x17", np.float64).copy()
    N.data[N.indptr[40]] = np.nan
    with pytest.raises(RuntimeError, match="pivot"):
        linalg.ilu0(lsp.csr_array(N))


# ---- solver integration (fp64, rtol 1e-8, random b) ----------------------
def _bicgstab_iters(La, b, M):
    calls = []
    x, info = linalg.bicgstab(La, b, rtol=1e-8, M=M, conv_test_iters=1,
                              callback=lambda xk: calls.append(1))
    assert info == 0
    return to_np(x), len(calls)


def test_bicgstab_with_ilu0():
    A = ic.ilu_matrix("grid33x17", np.float64)
    La = lsp.csr_array(A)
    b = ic.rhs(A.shape[0], None, np.float64)
    _, plain = _bicgstab_iters(La, b, None)
    x, pre = _bicgstab_iters(La, b, linalg.ilu0(La))
    print(f"bicgstab iterations: M=None {plain}, M=ilu0 {pre}")
    assert 2 * pre < plain
    assert np.linalg.norm(b - A @ x) <= 1e-7 * np.linalg.norm(b)


def test_cg_with_ilu0():
    A = ic.poisson2d(24, 24)
    La = lsp.csr_array(A)
    b = ic.rhs(576, None, np.float64)
    _, plain = linalg.cg(La, b, rtol=1e-8, conv_test_iters=1)
    x, pre = linalg.cg(La, b, rtol=1e-8, M=linalg.ilu0(La),
                       conv_test_iters=1)
    print(f"cg iterations: M=None {plain}, M=ilu0 {pre}")
    assert 2 * pre < plain
    x = to_np(x)
    assert np.linalg.norm(b - A @ x) <= 1e-7 * np.linalg.norm(b)


def test_lobpcg_with_ilu0():
    """The README's matrix: same eigenvalues with M = ilu0(H) as with the
    Jacobi M."""
    import lobpcg_cases as lc
    n, k = 1000, 4
    d = np.linspace(1.0, 100.0, n)
    off = -0.3 * np.ones(n - 1)
    H = sp.diags([d, off, off], [0, -1, 1], format="csr")
    Lh = lsp.csr_array(H)
    X0 = lc.start_block(n, k, np.float64, 0)
    wj, _ = linalg.lobpcg(Lh, X0, M=lsp.diags([1.0 / d], [0], format="csr"),
                          tol=1e-8, maxiter=100, largest=False)
    wi, _ = linalg.lobpcg(Lh, X0, M=linalg.ilu0(Lh), tol=1e-8, maxiter=100,
                          largest=False)
    # both converged to residual 1e-8: eigenvalue errors are far below it
    np.testing.assert_allclose(wi, wj, rtol=0, atol=1e-8)
    np.testing.assert_allclose(wi, np.linalg.eigvalsh(H.toarray())[:k],
                               rtol=0, atol=1e-8)

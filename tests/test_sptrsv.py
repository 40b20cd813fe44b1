# SPDX-License-Identifier: Apache-2.0
"""linalg.spsolve_triangular on the CPU path against scipy, the level
schedule and the launch plan (docs/DESIGN.md §17)."""
import numpy as np
import pytest
import scipy.sparse as sp

import legate_sparse as lsp
from legate_sparse import linalg, ops
from testutils import to_np
import ilu0_cases as ic

torch = pytest.importorskip("torch")


def _solve_all(name, lower, dtype):
    for unit in (False, True):
        A = ic.tri_matrix(name, lower, dtype, unit)
        La = lsp.csr_array(A)
        n = A.shape[0]
        for k in (None, 1, 3, 40):
            b = ic.rhs(n, k, dtype, seed=5 if k is None else k)
            want = ic.tri_reference(A, b, lower, unit)
            got = to_np(linalg.spsolve_triangular(La, b, lower=lower,
                                                  unit_diagonal=unit))
            assert got.shape == b.shape and got.dtype == np.dtype(dtype)
            err = np.abs(got - want).max()
            print(f"{name} lower={lower} unit={unit} k={k} "
                  f"{np.dtype(dtype).name}: |err| {err:.3e}")
            np.testing.assert_allclose(got, want, **ic.tol(dtype))


@pytest.mark.parametrize("dtype", ic.DTYPES)
@pytest.mark.parametrize("lower", [True, False])
@pytest.mark.parametrize("name", ic.TRI_NAMES)
def test_spsolve_triangular_matches_scipy(name, lower, dtype):
    _solve_all(name, lower, dtype)


def test_torch_tensor_rhs_and_scipy_matrix():
    A = ic.tri_matrix("rand300", True, np.float64)
    b = ic.rhs(300, 3, np.float64)
    want = ic.tri_reference(A, b, True, False)
    got = linalg.spsolve_triangular(A, torch.from_numpy(b))  # scipy input
    np.testing.assert_allclose(to_np(got), want, **ic.tol(np.float64))


def test_common_dtype():
    A = ic.tri_matrix("rand300", True, np.float32)
    b = ic.rhs(300, None, np.complex128)
    got = to_np(linalg.spsolve_triangular(lsp.csr_array(A), b))
    assert got.dtype == np.complex128
    np.testing.assert_allclose(got, ic.tri_reference(A, b, True, False),
                               **ic.tol(np.complex128))
    ib = np.arange(300)
    got = to_np(linalg.spsolve_triangular(lsp.csr_array(A), ib))
    assert got.dtype == np.float64


@pytest.mark.parametrize("k", [None, 3, 40])
def test_overwrite_b(k):
    A = ic.tri_matrix("grid33x17", True, np.float64)
    La = lsp.csr_array(A)
    b = ic.rhs(A.shape[0], k, np.float64)
    want = ic.tri_reference(A, b, True, False)
    bt = torch.from_numpy(b.copy())
    got = linalg.spsolve_triangular(La, bt, overwrite_b=True)
    assert got.data_ptr() == bt.data_ptr()
    np.testing.assert_allclose(bt.numpy(), want, **ic.tol(np.float64))
    # without overwrite_b the right-hand side is left alone
    bt = torch.from_numpy(b.copy())
    linalg.spsolve_triangular(La, bt)
    assert np.array_equal(bt.numpy(), b)
    # a numpy b cannot be overwritten: solved on a copy
    b2 = b.copy()
    got = linalg.spsolve_triangular(La, b2, overwrite_b=True)
    assert np.array_equal(b2, b)
    np.testing.assert_allclose(to_np(got), want, **ic.tol(np.float64))


def test_errors():
    A = ic.tri_matrix("rand300", True, np.float64)
    La = lsp.csr_array(A)
    b = ic.rhs(300, None, np.float64)
    with pytest.raises(ValueError):
        linalg.spsolve_triangular(lsp.csr_array(A[:, :299]), b)
    with pytest.raises(ValueError):
        linalg.spsolve_triangular(La, b[:299])
    with pytest.raises(ValueError):
        linalg.spsolve_triangular(La, np.zeros((300, 2, 2)))
    with pytest.raises(ValueError):      # lower matrix given as upper
        linalg.spsolve_triangular(La, b, lower=False)
    with pytest.raises(ValueError):
        linalg.spsolve_triangular(
            lsp.csr_array(ic.tri_matrix("rand300", False, np.float64)), b)
    # the structural verdict is cached per structure version
    assert La._tri_cache[(La._struct_version, False, False)]["wrong_side"]

    # missing diagonal entry
    M = sp.lil_matrix(A)
    M[7, 7] = 0
    M = sp.csr_array(M.tocsr())
    M.eliminate_zeros()
    with pytest.raises(np.linalg.LinAlgError):
        linalg.spsolve_triangular(lsp.csr_array(M), b)
    # ... which unit_diagonal does not need
    want = ic.tri_reference(M, b, True, True)
    got = linalg.spsolve_triangular(lsp.csr_array(M), b, unit_diagonal=True)
    np.testing.assert_allclose(to_np(got), want, **ic.tol(np.float64))
    # stored zero on the diagonal
    Z = A.copy()
    Z.data[Z.indptr[8 + 1] - 1] = 0.0     # last entry of a lower row
    with pytest.raises(np.linalg.LinAlgError):
        linalg.spsolve_triangular(lsp.csr_array(Z), b)


@pytest.mark.parametrize("lower", [True, False])
@pytest.mark.parametrize("name", ic.TRI_NAMES)
def test_level_schedule(name, lower):
    A = ic.tri_matrix(name, lower, np.float64)
    La = lsp.csr_array(A)
    s = ops.level_schedule(La._indptr, La._indices, A.shape[0], lower)
    order, lptr = s.order_host.numpy(), s.level_ptr_host.numpy()
    ic.check_levels(A, lower, order, lptr)
    if name == "grid33x17":
        assert s.n_levels == 49
        assert np.diff(lptr).max() <= 17
    if name == "grid9x8x7":
        assert s.n_levels == 9 + 8 + 7 - 2
    if name == "bidiag1000":
        assert s.n_levels == 1000
    if name == "dense65":
        assert s.n_levels == 65


def test_level_schedule_row_offset():
    """Columns outside [row_offset, row_offset + n) are no dependencies."""
    A = ic.tri_matrix("bidiag1000", True, np.float64)
    blk = sp.csr_array(A[400:700])
    ip = torch.from_numpy(blk.indptr.astype(np.int64))
    ix = torch.from_numpy(blk.indices.astype(np.int64))
    s = ops.level_schedule(ip, ix, 300, True, row_offset=400)
    assert s.n_levels == 300
    assert s.order_host.tolist() == list(range(300))


def test_plans():
    def sched(name):
        A = ic.tri_matrix(name, True, np.float64)
        La = lsp.csr_array(A)
        return ops.level_schedule(La._indptr, La._indices, A.shape[0], True)

    s = sched("bidiag1000")
    assert s.plan().tolist() == [[1, 0, 1000]]      # ONE chain launch
    s2 = sched("twotier5000")
    kinds = s2.plan()[:, 0].tolist()
    assert 0 in kinds                                # at least one wide
    for s in (s, s2, sched("rand300"), sched("grid33x17")):
        for c in (1, 16, None):
            p = s.plan(c).numpy()
            assert p.shape[0] <= s.n_levels          # chaining never adds
            assert p[0, 1] == 0 and p[-1, 2] == s.n_levels
            assert np.array_equal(p[1:, 1], p[:-1, 2])
            w = np.diff(s.level_ptr_host.numpy())
            lim = ops.SPTRSV_CHAIN_ROWS if c is None else c
            for kind, lo, hi in p:
                if kind == 0:
                    assert hi == lo + 1 and w[lo] > lim
                else:
                    assert np.all(w[lo:hi] <= lim)
            # maximal runs: two chains never touch
            assert not np.any((p[1:, 0] == 1) & (p[:-1, 0] == 1))


def test_plan_function_direct():
    p = ops.sptrsv_plan([0, 1, 2, 10, 11, 30, 31], chain_rows=4)
    assert p.tolist() == [[1, 0, 2], [0, 2, 3], [1, 3, 4], [0, 4, 5],
                          [1, 5, 6]]
    assert ops.sptrsv_plan([0], 4).shape == (0, 3)


def test_constants_exported():
    from legate_sparse import _cext
    assert ops.SPTRSV_KMAX == 32 == ops.BLOCK_KMAX
    assert ops.SPTRSV_CHAIN_ROWS > 0 and ops.SPTRSV_GRID_CAP > 0
    if _cext.has_hip():
        ext = _cext.require_hip()
        assert ext.SPTRSV_KMAX == ops.SPTRSV_KMAX
        assert ext.SPTRSV_CHAIN_ROWS == ops.SPTRSV_CHAIN_ROWS
        assert ext.SPTRSV_GRID_CAP == ops.SPTRSV_GRID_CAP


@pytest.mark.parametrize("lower", [True, False])
@pytest.mark.parametrize("name", ["rand300", "grid33x17", "dense65"])
def test_torch_arm_matches(name, lower):
    for unit in (False, True):
        A = ic.tri_matrix(name, lower, np.float64, unit)
        La = lsp.csr_array(A)
        info = linalg._tri_analysis(La, lower, unit)
        b = ic.rhs(A.shape[0], 5, np.float64)
        X = torch.from_numpy(b.copy())
        ops.sptrsv(La._indptr, La._indices, La._data, info["dpos"],
                   info["sched"], X, lower=lower, unit_diagonal=unit,
                   _impl="torch")
        np.testing.assert_allclose(X.numpy(),
                                   ic.tri_reference(A, b, lower, unit),
                                   **ic.tol(np.float64))


def test_ops_argument_checks():
    A = ic.tri_matrix("rand300", True, np.float64)
    La = lsp.csr_array(A)
    info = linalg._tri_analysis(La, True, False)
    args = (La._indptr, La._indices, La._data, info["dpos"], info["sched"])
    with pytest.raises(ValueError):
        ops.sptrsv(*args, torch.zeros(300, 33, dtype=torch.float64))
    with pytest.raises(ValueError):
        ops.sptrsv(*args, torch.zeros(299, 2, dtype=torch.float64))
    with pytest.raises(ValueError):
        ops.sptrsv(*args, torch.zeros(300, 2, dtype=torch.float32))
    with pytest.raises(ValueError):
        ops.sptrsv(*args, torch.zeros(2, 300, dtype=torch.float64).T)
    with pytest.raises(ValueError):
        ops.sptrsv(*args, torch.zeros(300, 2, dtype=torch.float64),
                   lower=False)
    with pytest.raises(ValueError):
        ops.sptrsv(*args, torch.zeros(300, 2, dtype=torch.float64),
                   _impl="eager")

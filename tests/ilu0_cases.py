# SPDX-License-Identifier: Apache-2.0
"""Matrices and references shared by the triangular-solve and ILU(0) tests
(CPU, GPU and the multi-process worker).

Triangular matrices are built to be well conditioned: off-diagonal values
uniform in [-1, 1] (both parts for complex), each diagonal entry
+-(2 * (row abs-sum) + 1).  References: scipy's ``spsolve_triangular`` and a
dictionary-based pure-Python IKJ ILU(0), both in fp64 / complex128.
"""
import functools

import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

DTYPES = [np.float32, np.float64, np.complex64, np.complex128]

TRI_NAMES = ["n1", "diag", "bidiag1000", "dense65", "arrow600",
             "twotier5000", "rand300", "grid33x17", "grid9x8x7"]


def tol(dtype):
    """The project's tolerances (test_gpu_spmm._tol)."""
    if np.dtype(dtype) in (np.dtype(np.float32), np.dtype(np.complex64)):
        return dict(rtol=1e-4, atol=1e-4)
    return dict(rtol=1e-10, atol=1e-12)


def wide(dtype):
    return np.complex128 if np.dtype(dtype).kind == "c" else np.float64


def _values(rng, m, dtype):
    v = rng.uniform(-1, 1, m)
    if np.dtype(dtype).kind == "c":
        v = v + 1j * rng.uniform(-1, 1, m)
    return v


def _with_diagonal(rows, cols, n, dtype, rng):
    """CSR from the off-diagonal pattern (rows, cols) plus the dominant
    diagonal of the module docstring."""
    rows = np.asarray(rows, dtype=np.int64)
    cols = np.asarray(cols, dtype=np.int64)
    vals = _values(rng, rows.size, dtype)
    off = sp.csr_array((vals, (rows, cols)), shape=(n, n))
    rowsum = np.asarray(abs(off).sum(axis=1)).reshape(-1)
    d = (2 * rowsum + 1) * rng.choice([-1.0, 1.0], n)
    A = sp.csr_array(off + sp.diags(d, format="csr")).astype(dtype)
    A.sort_indices()
    return A


def grid_pattern(dims):
    """(rows, cols) of the off-diagonal entries of the 5-/7-point stencil
    on a grid, natural ordering, first dimension fastest."""
    n = int(np.prod(dims))
    idx = np.arange(n)
    rows, cols = [], []
    stride = 1
    for d in dims:
        c = (idx // stride) % d
        up = idx[c + 1 < d]
        rows += [up, up + stride]
        cols += [up + stride, up]
        stride *= d
    return np.concatenate(rows), np.concatenate(cols)


def _lower_pattern(name, rng):
    if name == "n1":
        return [], [], 1
    if name == "diag":
        return [], [], 300
    if name == "bidiag1000":
        r = np.arange(1, 1000)
        return r, r - 1, 1000
    if name == "dense65":
        r, c = np.tril_indices(65, -1)
        return r, c, 65
    if name == "arrow600":
        return np.full(599, 599), np.arange(599), 600
    if name == "twotier5000":
        rows, cols = [], []
        for i in range(64, 5000):
            c = rng.choice(64, size=rng.integers(0, 9), replace=False)
            rows += [i] * c.size
            cols += list(c)
        return rows, cols, 5000
    if name == "rand300":
        rows, cols = [], []
        for i in range(1, 300):
            c = rng.choice(i, size=min(i, rng.integers(0, 12)), replace=False)
            rows += [i] * c.size
            cols += list(c)
        return rows, cols, 300
    dims = {"grid33x17": (33, 17), "grid9x8x7": (9, 8, 7)}[name]
    r, c = grid_pattern(dims)
    keep = c < r
    return r[keep], c[keep], int(np.prod(dims))


@functools.lru_cache(maxsize=None)
def tri_matrix(name, lower=True, dtype=np.float64, unit=False):
    """The named triangular test matrix (scipy CSR, sorted); upper cases
    are the transposes of the lower ones.

    ``unit``: the matrix for ``unit_diagonal=True`` solves.  Dropping the
    dominant diagonal would leave an ill-conditioned unit triangle (dense65
    grows its solution to 1e4), so the rows are first divided by their
    diagonal entry (off-diagonal row abs-sums below 1/2) and the stored
    diagonal, which the solve must ignore, is then set to 3."""
    rng = np.random.default_rng(TRI_NAMES.index(name) + 11)
    r, c, n = _lower_pattern(name, rng)
    A = _with_diagonal(r, c, n, wide(dtype) if unit else dtype, rng)
    if not lower:
        A = sp.csr_array(A.T)
    if unit:
        A = sp.csr_array(sp.diags(1.0 / A.diagonal()) @ A)
        A.setdiag(3.0)
        A = sp.csr_array(A.astype(dtype))
    A.sort_indices()
    return A


def rhs(n, k, dtype, seed=3):
    """(n,) for k = None, else (n, k)."""
    rng = np.random.default_rng(seed)
    shape = (n,) if k is None else (n, k)
    b = rng.standard_normal(shape)
    if np.dtype(dtype).kind == "c":
        b = b + 1j * rng.standard_normal(shape)
    return b.astype(dtype)


def tri_reference(A, b, lower, unit_diagonal):
    """scipy's solve in fp64 / complex128 from the same (already rounded)
    inputs."""
    w = wide(np.result_type(A.dtype, np.asarray(b).dtype))
    return spla.spsolve_triangular(sp.csr_matrix(A.astype(w)), b.astype(w),
                                   lower=lower, unit_diagonal=unit_diagonal)


def check_levels(A, lower, order, level_ptr):
    """Every row appears once and its dependencies lie in strictly earlier
    levels; rows ascend within a level."""
    n = A.shape[0]
    order = np.asarray(order)
    level_ptr = np.asarray(level_ptr)
    assert sorted(order.tolist()) == list(range(n))
    level = np.empty(n, dtype=np.int64)
    for lv in range(level_ptr.size - 1):
        rows = order[level_ptr[lv]:level_ptr[lv + 1]]
        assert rows.size > 0 and np.all(np.diff(rows) > 0)
        level[rows] = lv
    coo = A.tocoo()
    dep = coo.col < coo.row if lower else coo.col > coo.row
    assert np.all(level[coo.col[dep]] < level[coo.row[dep]])
    # tight: a row above level 0 has a dependency one level below it
    best = np.full(n, -1, dtype=np.int64)
    np.maximum.at(best, coo.row[dep], level[coo.col[dep]])
    assert np.array_equal(level, best + 1)


# ---- ILU(0) inputs -------------------------------------------------------
def convdiff(nx, ny, cx=3.0, dtype=np.float64):
    """5-point diffusion plus x-convection: row stencil
    [-1, (-1 - cx), 4 + cx, -1, -1] (first-order upwind, coefficient cx);
    nonsymmetric values, symmetric pattern.  The complex variant adds
    0.2j I."""
    Tx = sp.diags([-1 - cx, 2 + cx, -1], [-1, 0, 1], shape=(nx, nx))
    Ty = sp.diags([-1, 2, -1], [-1, 0, 1], shape=(ny, ny))
    A = sp.kron(sp.identity(ny), Tx) + sp.kron(Ty, sp.identity(nx))
    if np.dtype(dtype).kind == "c":
        A = A + 0.2j * sp.identity(nx * ny)
    A = sp.csr_array(A.astype(dtype))
    A.sort_indices()
    return A


def poisson3d(dims, dtype=np.float64):
    r, c = grid_pattern(dims)
    n = int(np.prod(dims))
    A = sp.csr_array((-np.ones(r.size), (r, c)), shape=(n, n)) \
        + 6 * sp.identity(n, format="csr")
    A = sp.csr_array(A.astype(dtype))
    A.sort_indices()
    return A


def symmetrised(name, dtype=np.float64):
    """A triangular case's pattern made symmetric, fresh values, dominant
    diagonal."""
    rng = np.random.default_rng(TRI_NAMES.index(name) + 101)
    r, c, n = _lower_pattern(name, np.random.default_rng(
        TRI_NAMES.index(name) + 11))
    r, c = np.asarray(r, dtype=np.int64), np.asarray(c, dtype=np.int64)
    return _with_diagonal(np.concatenate([r, c]), np.concatenate([c, r]), n,
                          dtype, rng)


ILU_NAMES = ["grid33x17", "grid9x8x7", "rand300sym", "complex"]


@functools.lru_cache(maxsize=None)
def ilu_matrix(name, dtype=np.float64):
    if name == "grid33x17":
        return convdiff(33, 17, dtype=dtype)
    if name == "grid9x8x7":
        return poisson3d((9, 8, 7), dtype=dtype)
    if name == "rand300sym":
        return symmetrised("rand300", dtype)
    if name == "arrow600sym":
        return symmetrised("arrow600", dtype)
    if name == "complex":
        dt = np.complex64 if np.dtype(dtype) in (
            np.dtype(np.float32), np.dtype(np.complex64)) else np.complex128
        return convdiff(12, 9, cx=1.0, dtype=dt)
    raise KeyError(name)


def ilu0_reference(A):
    """Dictionary-based IKJ ILU(0) in fp64 / complex128: the combined
    factor (strict lower part L, the rest U) as scipy CSR on A's
    pattern."""
    A = sp.csr_matrix(A.astype(wide(A.dtype)))
    A.sort_indices()
    n = A.shape[0]
    rows = [dict(zip(A.indices[A.indptr[i]:A.indptr[i + 1]].tolist(),
                     A.data[A.indptr[i]:A.indptr[i + 1]].tolist()))
            for i in range(n)]
    for i in range(n):
        ri = rows[i]
        for k in sorted(c for c in ri if c < i):
            ri[k] = ri[k] / rows[k][k]
            f = ri[k]
            for j, v in rows[k].items():
                if j > k and j in ri:
                    ri[j] -= f * v
    data = np.array([rows[i][j] for i in range(n)
                     for j in A.indices[A.indptr[i]:A.indptr[i + 1]]],
                    dtype=A.dtype)
    return sp.csr_matrix((data, A.indices.copy(), A.indptr.copy()),
                         shape=A.shape)


def split_factor(F):
    """(L with unit diagonal, U) from the combined factor."""
    L = sp.tril(F, -1, format="csr") + sp.identity(F.shape[0],
                                                   dtype=F.dtype,
                                                   format="csr")
    return sp.csr_matrix(L), sp.csr_matrix(sp.triu(F, 0, format="csr"))


def ilu_apply_reference(F, r):
    """U^-1 L^-1 r through scipy's two triangular solves."""
    L, U = split_factor(F)
    w = wide(F.dtype)
    y = spla.spsolve_triangular(L, r.astype(w), lower=True,
                                unit_diagonal=True)
    return spla.spsolve_triangular(U, y, lower=False)


def zero_pivot_matrix(n=6, dtype=np.float64):
    """Tridiagonal whose second pivot cancels exactly: a11 - a10 a01 / a00
    = 1 - 1 = 0."""
    A = sp.diags([np.ones(n - 1), np.full(n, 4.0), np.ones(n - 1)],
                 [-1, 0, 1], format="lil")
    A[0, 0] = 1.0
    A[1, 1] = 1.0
    A = sp.csr_array(A.tocsr().astype(dtype))
    A.sort_indices()
    return A


def poisson2d(nx, ny, dtype=np.float64):
    Tx = sp.diags([-1, 2, -1], [-1, 0, 1], shape=(nx, nx))
    Ty = sp.diags([-1, 2, -1], [-1, 0, 1], shape=(ny, ny))
    A = sp.csr_array((sp.kron(sp.identity(ny), Tx)
                      + sp.kron(Ty, sp.identity(nx))).astype(dtype))
    A.sort_indices()
    return A

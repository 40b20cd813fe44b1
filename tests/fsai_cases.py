# SPDX-License-Identifier: Apache-2.0
"""Matrices, patterns and the reference shared by the FSAI tests (CPU, GPU
and the multi-process worker), docs/DESIGN.md §18.

Reference: row i of G on its sorted pattern P (last entry i) is ``conj(w)``
with ``S = A[P, P]``, ``S = C C^H``, ``C^H w = e_m``, evaluated per row in
numpy in float64 / complex128 from the (already rounded) test matrix.

Every block S of every case whose VALUES are compared has ``cond(S) <=
100`` (asserted in ``reference``): the relative error of a Cholesky solve
is a small multiple of ``cond(S) * eps``, i.e. below 1e-13 in double and
1e-4 / 8 in single for blocks of at most 32 rows, inside ``tol``.  The
jump-coefficient matrix is used for iteration counts only; its blocks mix
coefficients over three decades and are not held to that bound.
"""
import functools

import numpy as np
import scipy.sparse as sp

from ilu0_cases import DTYPES, grid_pattern, rhs, tol, wide  # noqa: F401

MAX_ROW = 32
COND_MAX = 100.0

# name -> (value dtypes, patterns); a pattern is an int power or "given"
CASES = {
    "grid33x17": (DTYPES[:2], (1, 3)),
    "grid9x8x7": (DTYPES[:2], (1, 2, 3)),
    "rand300": (DTYPES[:2], (1,)),
    "herm300": (DTYPES[2:], (1,)),
    "dense32": (DTYPES, ("given",)),
    "diag": (DTYPES, (1,)),
    "n1": (DTYPES, (1,)),
    "band8": (DTYPES[:2], ("given",)),
    "band9": (DTYPES[:2], ("given",)),
}
# the longest pattern row of each (case, pattern): asserted, so the tests
# know which sub-wave width they exercise
LONGEST = {("grid33x17", 1): 3, ("grid33x17", 3): 13, ("grid9x8x7", 1): 4,
           ("grid9x8x7", 2): 13, ("grid9x8x7", 3): 32, ("dense32", "given"): 32,
           ("diag", 1): 1, ("n1", 1): 1, ("band8", "given"): 8,
           ("band9", "given"): 9}
VALUE_CASES = [(n, p, d) for n, (dts, pats) in CASES.items()
               for p in pats for d in dts]


def _csr(A, dtype):
    A = sp.csr_array(A).astype(dtype)
    A.sort_indices()
    return A


def _laplacian(dims):
    r, c = grid_pattern(dims)
    n = int(np.prod(dims))
    return sp.csr_array((-np.ones(r.size), (r, c)), shape=(n, n)) \
        + 2 * len(dims) * sp.identity(n, format="csr")


def _random_hpd(n, density, complex_, seed):
    """Random Hermitian pattern, values uniform in [-1, 1] (both parts for
    complex), diagonal = 1.5 * (row abs-sum) + 1: strictly diagonally
    dominant, hence positive definite."""
    rng = np.random.default_rng(seed)
    low = sp.tril(sp.random(n, n, density=density, format="csr",
                            random_state=np.random.RandomState(seed)), -1)
    low = sp.csr_array(low)
    v = rng.uniform(-1, 1, low.nnz)
    if complex_:
        v = v + 1j * rng.uniform(-1, 1, low.nnz)
    low.data = v
    off = low + low.conj().T
    d = 1.5 * np.asarray(abs(off).sum(axis=1)).reshape(-1) + 1
    return off + sp.diags(d, format="csr")


def _dense_hpd(n, complex_, seed):
    rng = np.random.default_rng(seed)
    R = rng.uniform(-1, 1, (n, n))
    if complex_:
        R = R + 1j * rng.uniform(-1, 1, (n, n))
    return R @ R.conj().T / n + np.eye(n)


def _band(n, half, seed):
    rng = np.random.default_rng(seed)
    offs = list(range(1, half + 1))
    low = sp.diags([rng.uniform(-1, 1, n - o) for o in offs],
                   [-o for o in offs], shape=(n, n), format="csr")
    off = low + low.T
    d = 1.5 * np.asarray(abs(off).sum(axis=1)).reshape(-1) + 1
    return off + sp.diags(d, format="csr")


def jump(nx, ny=None, dtype=np.float64, seed=5):
    """5-point diffusion with cell coefficients k in {1, 10, 100, 1000},
    harmonic-mean couplings between neighbours and 1e-3 * k added to the
    diagonal (natural boundary: a row sums to 1e-3 * k)."""
    ny = nx if ny is None else ny
    rng = np.random.default_rng(seed)
    n = nx * ny
    k = 10.0 ** rng.integers(0, 4, n)
    r, c = grid_pattern((nx, ny))
    w = 2 * k[r] * k[c] / (k[r] + k[c])
    off = sp.csr_array((-w, (r, c)), shape=(n, n))
    d = -np.asarray(off.sum(axis=1)).reshape(-1) + 1e-3 * k
    return _csr(off + sp.diags(d, format="csr"), dtype)


@functools.lru_cache(maxsize=None)
def matrix(name, dtype=np.float64):
    """The named Hermitian positive definite test matrix (scipy CSR)."""
    cplx = np.dtype(dtype).kind == "c"
    if name == "grid33x17":
        A = _laplacian((33, 17))
    elif name == "grid9x8x7":
        A = _laplacian((9, 8, 7))
    elif name == "rand300":
        A = _random_hpd(300, 0.02, False, 21)
    elif name == "herm300":
        A = _random_hpd(300, 0.02, True, 22)
    elif name in ("dense32", "dense33"):
        A = sp.csr_array(_dense_hpd(int(name[5:]), cplx, 23))
    elif name == "diag":
        A = sp.diags(np.random.default_rng(24).uniform(0.5, 4, 300),
                     format="csr")
    elif name == "n1":
        A = sp.csr_array(np.array([[2.5]]))
    elif name in ("band8", "band9"):
        A = _band(41, 9, 25)
    elif name == "jump48":
        return jump(48, dtype=dtype)
    else:
        raise KeyError(name)
    return _csr(A, dtype)


@functools.lru_cache(maxsize=None)
def pattern(name, p):
    """Lower-triangular pattern (scipy CSR of ones, sorted): the lower
    triangle of the pattern of |A|^p for an int p, else the case's own."""
    if p == "given":
        n = matrix(name).shape[0]
        if name.startswith("dense"):
            P = sp.csr_array(np.tril(np.ones((n, n))))
        else:
            half = int(name[4:]) - 1
            P = sp.diags([np.ones(n - o) for o in range(half + 1)],
                         [-o for o in range(half + 1)], shape=(n, n))
    else:
        B = abs(sp.csr_array(matrix(
            name, np.complex128 if name == "herm300" else np.float64)))
        B.data[:] = 1.0
        P = B
        for _ in range(p - 1):
            P = P @ B
        P = sp.tril(P, 0)
    P = sp.csr_array(P).astype(np.float64)
    P.sort_indices()
    P.data[:] = 1.0
    return P


def reference_rows(A, P, cond_max=None):
    """G's values in P's layout, float64 / complex128; with ``cond_max``
    every block's condition number is asserted to stay below it."""
    w = wide(A.dtype)
    L = sp.tril(sp.csr_array(A).astype(w), 0).tocsr()
    H = (L + sp.tril(L, -1).conj().T).toarray() if A.shape[0] <= 4096 \
        else None
    Hs = None if H is not None else (L + sp.tril(L, -1).conj().T).tocsr()
    out = np.empty(P.nnz, dtype=w)
    worst = 0.0
    for i in range(P.shape[0]):
        s, e = P.indptr[i], P.indptr[i + 1]
        cols = P.indices[s:e]
        assert e > s and cols[-1] == i and np.all(np.diff(cols) > 0)
        S = H[np.ix_(cols, cols)] if H is not None \
            else Hs[cols][:, cols].toarray()
        if cond_max is not None:
            worst = max(worst, np.linalg.cond(S))
        C = np.linalg.cholesky(S)
        em = np.zeros(e - s, dtype=w)
        em[-1] = 1
        out[s:e] = np.linalg.solve(C.conj().T, em).conj()
    if cond_max is not None:
        assert worst <= cond_max, f"cond(S) {worst:.3g} > {cond_max}"
    return out


@functools.lru_cache(maxsize=None)
def reference(name, p, dtype):
    """(pattern, G values) for a value case; asserts the block condition
    bound and the documented longest row."""
    P = pattern(name, p)
    longest = int(np.diff(P.indptr).max())
    assert longest <= MAX_ROW
    if (name, p) in LONGEST:
        assert longest == LONGEST[(name, p)], (name, p, longest)
    vals = reference_rows(matrix(name, dtype), P, cond_max=COND_MAX)
    vals.setflags(write=False)
    return P, vals


def as_scipy(G):
    """A (world size 1) csr_array as scipy CSR."""
    from testutils import to_np
    return sp.csr_array((to_np(G.data), to_np(G.indices).astype(np.int64),
                         to_np(G.indptr)), shape=G.shape)


def apply_reference(P, gvals, r):
    """G^H (G r) in float64 / complex128."""
    G = sp.csr_array((gvals, P.indices, P.indptr), shape=P.shape)
    return G.conj().T @ (G @ r.astype(gvals.dtype))


def indefinite_diag(row=7):
    """33x17 Laplacian with a negative diagonal entry in ``row``: it is
    the last pivot of that row's own block, and every other pattern row
    that holds ``row`` has a larger number, so ``row`` is the smallest bad
    row."""
    A = sp.lil_matrix(matrix("grid33x17"))
    A[row, row] = -4.0
    return _csr(A.tocsr(), np.float64)


def indefinite_block(row=11):
    """Identity-dominant tridiagonal whose rows (row - 1, row) carry the
    block [[1, 2], [2, 1]]: row ``row``'s block breaks at its second
    pivot (1 - 4 < 0); row ``row + 1`` does not contain row - 1."""
    n = 30
    A = sp.lil_matrix(sp.identity(n) * 1.0)
    A[row, row - 1] = A[row - 1, row] = 2.0
    return _csr(A.tocsr(), np.float64)

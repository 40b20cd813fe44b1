# SPDX-License-Identifier: Apache-2.0
"""Matrices, oracles and checks shared by the LOBPCG tests (CPU, GPU and
the multi-process worker).

The oracle is dense ``numpy.linalg.eigvalsh`` in fp64/complex128, plus
``scipy.sparse.linalg.lobpcg`` on the same initial block for the iteration
budget."""
import functools
import warnings

import numpy as np
import scipy.sparse as sp

SEEDS = [0, 1, 2, 3, 4]

# case -> (block sizes, which ends, {dtype: tol})
CASES = {
    "poisson": ((1, 4, 5), ("smallest", "largest"),
                {np.float64: 1e-6, np.float32: 5e-3}),
    "diagdom_jacobi": ((3, 5), ("smallest",),
                       {np.float64: 1e-6, np.float32: 5e-2}),
    "hermitian": ((4,), ("smallest", "largest"),
                  {np.complex128: 1e-6, np.complex64: 2e-2}),
}


def poisson2d(m):
    """5-point Laplacian on an m x m grid (degenerate eigenvalue pairs)."""
    T = sp.diags([-1.0, 2.0, -1.0], [-1, 0, 1], shape=(m, m))
    A = sp.csr_array(sp.kron(sp.identity(m), T) + sp.kron(T, sp.identity(m)))
    A.sort_indices()
    return A


def diagdom(n=300):
    A = sp.csr_array(sp.diags(np.linspace(1, 1000, n))
                     + 0.5 * sp.diags([-1.0, -1.0], [-1, 1], shape=(n, n)))
    A.sort_indices()
    return A


def hermitian(n=200):
    rng = np.random.default_rng(11)
    off = 0.3 * (rng.standard_normal(n - 1) + 1j * rng.standard_normal(n - 1))
    A = sp.csr_array(sp.diags(np.linspace(1, 50, n)).astype(np.complex128)
                     + sp.diags(off, 1) + sp.diags(off.conj(), -1))
    A.sort_indices()
    return A


@functools.lru_cache(maxsize=None)
def matrix(case):
    """(scipy matrix in double precision, scipy Jacobi preconditioner or
    None, ascending exact eigenvalues)."""
    if case == "poisson":
        A = poisson2d(16)
    elif case == "poisson15":
        A = poisson2d(15)
    elif case in ("diagdom_jacobi", "diagdom"):
        A = diagdom()
    elif case == "hermitian":
        A = hermitian()
    else:
        raise KeyError(case)
    M = None
    if case == "diagdom_jacobi":
        M = sp.csr_array(sp.diags(1.0 / A.diagonal()))
    exact = np.linalg.eigvalsh(A.toarray())
    return A, M, exact


def start_block(n, k, dtype, seed):
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((n, k))
    if np.dtype(dtype).kind == "c":
        X = X + 1j * rng.standard_normal((n, k))
    return X.astype(dtype)


def extremal(exact, k, largest):
    return exact[::-1][:k] if largest else exact[:k]


@functools.lru_cache(maxsize=None)
def scipy_iterations(case, k, largest, dtype_name, tol, seed):
    """Iterations scipy's lobpcg takes on the same X; it must converge
    without a warning."""
    from scipy.sparse.linalg import lobpcg
    dtype = np.dtype(dtype_name)
    A, M, _ = matrix(case)
    X = start_block(A.shape[0], k, dtype, seed)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        out = lobpcg(A.astype(dtype), X, M=None if M is None else
                     M.astype(dtype), tol=tol, maxiter=500, largest=largest,
                     retResidualNormsHistory=True)
    return len(out[2]) - 2


def iterations(hist):
    """Iterations from a history list: entry 0 is the initial block, the
    last entry the post-processed result (as in scipy)."""
    return len(hist) - 2


def check_pairs(A, exact, w, V, k, largest, tol):
    """Checks (b)-(d): residuals recomputed in double precision, the k
    extremal eigenvalues, orthonormality."""
    cdt = np.complex128 if (np.iscomplexobj(V) or A.dtype.kind == "c") \
        else np.float64
    V = np.asarray(V).astype(cdt)
    w = np.asarray(w, dtype=np.float64)
    assert w.shape == (k,) and V.shape == (A.shape[0], k)
    res = np.linalg.norm(A.astype(cdt) @ V - V * w[None, :], axis=0)
    err = np.abs(w - extremal(exact, k, largest))
    orth = np.linalg.norm(V.conj().T @ V - np.eye(k))
    print(f"residuals {res} eigenvalue errors {err} orthonormality {orth}")
    assert np.all(res <= tol), (res, tol)
    assert np.all(err <= tol), (err, tol)
    assert orth <= np.sqrt(k) * tol, (orth, tol)

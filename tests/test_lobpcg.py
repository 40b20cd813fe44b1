# SPDX-License-Identifier: Apache-2.0
"""LOBPCG on the CPU path: convergence against dense eigenvalues and
scipy's iteration counts, the call contract, and the three block ops
against numpy."""
import warnings

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import legate_sparse as lsp
from legate_sparse import ops
from legate_sparse.linalg import LinearOperator
from testutils import to_np
import lobpcg_cases as lc


def _params():
    for case, (ks, whichs, tols) in lc.CASES.items():
        for dtype, tol in tols.items():
            for k in ks:
                for which in whichs:
                    yield pytest.param(
                        case, np.dtype(dtype), tol, k, which == "largest",
                        id=f"{case}-{np.dtype(dtype).name}-k{k}-{which}")


def _lsp_pair(case, dtype):
    S, M, exact = lc.matrix(case)
    A = lsp.csr_array(sp.csr_array(S.astype(dtype)))
    Ml = None if M is None else lsp.csr_array(sp.csr_array(M.astype(dtype)))
    return S, A, Ml, exact


@pytest.mark.parametrize("case,dtype,tol,k,largest", list(_params()))
def test_converges(case, dtype, tol, k, largest):
    S, A, M, exact = _lsp_pair(case, dtype)
    for seed in lc.SEEDS:
        X = lc.start_block(S.shape[0], k, dtype, seed)
        ref_its = lc.scipy_iterations(case, k, largest, dtype.name, tol, seed)
        with warnings.catch_warnings():
            warnings.simplefilter("error")          # (a), and (e) through it
            w, V, hist = lsp.linalg.lobpcg(
                A, X, M=M, tol=tol, maxiter=2 * ref_its + 10,
                largest=largest, retResidualNormsHistory=True)
        print(f"seed {seed}: scipy {ref_its} iterations, "
              f"here {lc.iterations(hist)}")
        assert isinstance(w, np.ndarray)
        lc.check_pairs(S, exact, w, to_np(V), k, largest, tol)


def test_jacobi_takes_fewer_iterations():
    S, A, M, _ = _lsp_pair("diagdom_jacobi", np.float64)
    X = lc.start_block(300, 3, np.float64, 0)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        _, _, h_pre = lsp.linalg.lobpcg(A, X, M=M, tol=1e-6, maxiter=400,
                                        largest=False,
                                        retResidualNormsHistory=True)
        _, _, h_plain = lsp.linalg.lobpcg(A, X, tol=1e-6, maxiter=400,
                                          largest=False,
                                          retResidualNormsHistory=True)
    print(lc.iterations(h_pre), lc.iterations(h_plain))
    assert lc.iterations(h_pre) < lc.iterations(h_plain)


def test_order_and_history_shapes():
    S, A, _, exact = _lsp_pair("poisson", np.float64)
    X = lc.start_block(256, 4, np.float64, 2)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        w, V, lh, rh = lsp.linalg.lobpcg(
            A, X, tol=1e-6, maxiter=300, retLambdaHistory=True,
            retResidualNormsHistory=True)            # largest=True default
        ws, _ = lsp.linalg.lobpcg(A, X, tol=1e-6, maxiter=300, largest=False)
    assert np.all(np.diff(w) <= 0) and np.all(np.diff(ws) >= 0)
    np.testing.assert_allclose(w, exact[::-1][:4], atol=1e-6)
    # scipy's shapes: lists of (k,) arrays, iterations + 2 entries each
    assert isinstance(lh, list) and isinstance(rh, list)
    assert len(lh) == len(rh) and len(rh) >= 3
    assert all(np.shape(a) == (4,) for a in lh + rh)
    np.testing.assert_array_equal(lh[-1], w)
    # only one of the two histories
    out = lsp.linalg.lobpcg(A, X, tol=1e-6, maxiter=300,
                            retLambdaHistory=True)
    assert len(out) == 3 and len(out[2]) == len(lh)


def test_exact_invariant_subspace_takes_zero_iterations():
    S, A, _, exact = _lsp_pair("diagdom", np.float64)
    lam, vec = np.linalg.eigh(S.toarray())
    X = vec[:, :3] @ np.array([[1.0, 2, 0], [0, 1, 1], [1, 0, 3]])
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        w, V, rh = lsp.linalg.lobpcg(A, X, tol=1e-8, largest=False,
                                     retResidualNormsHistory=True)
    assert lc.iterations(rh) == 0
    lc.check_pairs(S, exact, w, to_np(V), 3, False, 1e-8)


def test_argument_errors():
    _, A, _, _ = _lsp_pair("poisson", np.float64)
    X = lc.start_block(256, 2, np.float64, 0)
    with pytest.raises(NotImplementedError):
        lsp.linalg.lobpcg(A, X, B=A)
    with pytest.raises(NotImplementedError):
        lsp.linalg.lobpcg(A, X, Y=X)
    with pytest.raises(ValueError, match="k = 33"):
        lsp.linalg.lobpcg(A, lc.start_block(256, 33, np.float64, 0))
    small = lsp.csr_array(sp.csr_array(lc.poisson2d(3)))      # n = 9
    with pytest.raises(ValueError, match="3k"):
        lsp.linalg.lobpcg(small, lc.start_block(9, 4, np.float64, 0))
    with pytest.raises(ValueError):
        lsp.linalg.lobpcg(A, X[:100])


def test_tiny_maxiter_warns_and_returns_finite():
    S, A, _, _ = _lsp_pair("poisson", np.float64)
    X = lc.start_block(256, 4, np.float64, 0)
    with pytest.warns(UserWarning, match="tolerance"):
        w, V = lsp.linalg.lobpcg(A, X, tol=1e-10, maxiter=2, largest=False)
    V = to_np(V)
    assert np.isfinite(w).all() and np.isfinite(V).all()
    assert V.shape == (256, 4)
    np.testing.assert_allclose(V.T @ V, np.eye(4), atol=1e-10)


def test_python_matvec_operator():
    S, _, _, exact = _lsp_pair("diagdom", np.float64)
    D = torch.from_numpy(S.toarray())
    Aop = LinearOperator((300, 300), matvec=lambda x: D @ torch.as_tensor(x),
                         dtype=np.float64)
    d = torch.from_numpy(1.0 / S.diagonal())
    Mop = LinearOperator((300, 300), matvec=lambda x: d * torch.as_tensor(x),
                         dtype=np.float64)
    X = lc.start_block(300, 3, np.float64, 1)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        w, V = lsp.linalg.lobpcg(Aop, X, M=Mop, tol=1e-6, maxiter=60,
                                 largest=False)
    lc.check_pairs(S, exact, w, to_np(V), 3, False, 1e-6)


# ---- the block ops off the GPU: the torch path against numpy ------------
def _blk(rng, n, c, dtype):
    a = rng.standard_normal((n, c))
    if np.dtype(dtype).kind == "c":
        a = a + 1j * rng.standard_normal((n, c))
    return torch.from_numpy(a.astype(dtype))


@pytest.mark.parametrize("dtype", [np.float32, np.float64, np.complex64,
                                   np.complex128])
def test_block_ops_match_numpy(dtype):
    rng = np.random.default_rng(5)
    rtol = 1e-4 if np.dtype(dtype).itemsize <= 8 and \
        np.dtype(dtype) != np.float64 else 1e-12
    n = 77
    wide = _blk(rng, n, 12, dtype)
    X, Y = wide[:, 1:4], _blk(rng, n, 5, dtype)        # X: a strided panel
    G = ops.block_gram(X, Y)
    np.testing.assert_allclose(to_np(G), to_np(X).conj().T @ to_np(Y),
                               rtol=rtol, atol=rtol * n)
    Gt = ops.block_gram(X, Y, conj=False)
    np.testing.assert_allclose(to_np(Gt), to_np(X).T @ to_np(Y),
                               rtol=rtol, atol=rtol * n)
    C1, C2 = _blk(rng, 3, 5, dtype), _blk(rng, 5, 5, dtype)
    Z = _blk(rng, n, 5, dtype)
    want = to_np(X) @ to_np(C1) + to_np(Y) @ to_np(C2) + to_np(Z)
    ops.block_update(Z, [(X, C1), (Y, C2)], accumulate=True)
    np.testing.assert_allclose(to_np(Z), want, rtol=rtol, atol=rtol * 10)
    want = to_np(Y) @ to_np(C2)
    ops.block_update(Y, [(Y, C2)])                     # Z is X_0: allowed
    np.testing.assert_allclose(to_np(Y), want, rtol=rtol, atol=rtol * 10)
    rdt = np.zeros(0, dtype=dtype).real.dtype
    theta = torch.from_numpy(rng.standard_normal(5).astype(rdt))
    R = torch.empty_like(Y)
    nrm = ops.block_residual(R, Z, Y, theta)
    want = to_np(Z) - to_np(Y) * to_np(theta)[None, :]
    np.testing.assert_allclose(to_np(R), want, rtol=rtol, atol=rtol * 10)
    assert nrm.dtype == theta.dtype
    np.testing.assert_allclose(to_np(nrm), (np.abs(want) ** 2).sum(axis=0),
                               rtol=rtol)


def test_block_ops_refuse_bad_operands():
    X = torch.zeros(10, 4, dtype=torch.float64)
    with pytest.raises(ValueError):
        ops.block_gram(X, torch.zeros(9, 4, dtype=torch.float64))
    with pytest.raises(ValueError):
        ops.block_gram(X, torch.zeros(10, 4, dtype=torch.float32))
    with pytest.raises(ValueError):
        ops.block_gram(X, torch.zeros(10, 33, dtype=torch.float64))
    with pytest.raises(ValueError):                    # column-major view
        ops.block_gram(X, torch.zeros(4, 10, dtype=torch.float64).T)
    C = torch.zeros(4, 4, dtype=torch.float64)
    wide = torch.zeros(10, 8, dtype=torch.float64)
    with pytest.raises(ValueError, match="overlaps"):  # shifted by a column
        ops.block_update(wide[:, 0:4], [(wide[:, 1:5], C)])
    ops.block_update(wide[:, 0:4], [(wide[:, 4:8], C)])   # disjoint panels
    with pytest.raises(ValueError):                    # C of the wrong shape
        ops.block_update(X, [(X, torch.zeros(3, 4, dtype=torch.float64))])
    with pytest.raises(ValueError):
        ops.block_update(X, [])
    with pytest.raises(ValueError):                    # complex theta
        ops.block_residual(X.clone(), X, X,
                           torch.zeros(4, dtype=torch.complex128))
    assert ops.BLOCK_KMAX == 32

# SPDX-License-Identifier: Apache-2.0
"""CSR x dense block (SpMM): csr_array.matmat, spmm, ops.spmm and the
LinearOperator block products on CPU, against scipy.sparse products."""
import warnings

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import legate_sparse as lsp
from legate_sparse import _cext, linalg, ops
from testutils import sample_csr, to_np

DTYPES = [np.float32, np.float64, np.complex64, np.complex128]


def _tol(dtype):
    if np.dtype(dtype) in (np.dtype(np.float32), np.dtype(np.complex64)):
        return dict(rtol=1e-4, atol=1e-4)
    return dict(rtol=1e-10, atol=1e-12)


def _block(n, k, dtype, seed=7):
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((n, k))
    if np.dtype(dtype).kind == "c":
        X = X + 1j * rng.standard_normal((n, k))
    return np.ascontiguousarray(X.astype(dtype))


@pytest.mark.parametrize("k", [1, 2, 3, 5, 8, 17])
@pytest.mark.parametrize("dtype", DTYPES)
def test_matmat_dtypes_k(dtype, k):
    S = sample_csr(60, 47, 0.1, seed=1, dtype=dtype)
    X = _block(47, k, dtype)
    Y = lsp.csr_array(S).matmat(X)
    assert tuple(Y.shape) == (60, k)
    assert Y.is_contiguous()
    assert to_np(Y).dtype == np.dtype(dtype)
    np.testing.assert_allclose(to_np(Y), S @ X, **_tol(dtype))


def test_matmat_rectangular():
    S = sample_csr(37, 23, 0.2, seed=2)
    X = _block(23, 4, np.float64)
    np.testing.assert_allclose(to_np(lsp.csr_array(S).matmat(X)), S @ X,
                               rtol=1e-10, atol=1e-12)


def test_matmat_empty_rows():
    D = sample_csr(40, 31, 0.2, seed=3).toarray()
    D[[0, 5, 6, 39], :] = 0.0
    S = sp.csr_array(D)
    X = _block(31, 3, np.float64)
    Y = to_np(lsp.csr_array(S).matmat(X))
    np.testing.assert_allclose(Y, S @ X, rtol=1e-10, atol=1e-12)
    assert not Y[[0, 5, 6, 39]].any()


def test_matmat_all_empty_matrix():
    S = sp.csr_array((12, 9), dtype=np.float64)
    Y = to_np(lsp.csr_array(S).matmat(_block(9, 3, np.float64)))
    assert Y.shape == (12, 3) and not Y.any()


def test_matmat_k0():
    S = sample_csr(60, 47, 0.1, seed=1)
    Y = lsp.csr_array(S).matmat(np.zeros((47, 0)))
    assert tuple(Y.shape) == (60, 0)
    assert Y.dtype == torch.float64


def test_matmat_numpy_and_torch_operands():
    S = sample_csr(60, 47, 0.1, seed=1)
    X = _block(47, 3, np.float64)
    A = lsp.csr_array(S)
    Yn = A.matmat(X)
    Yt = A.matmat(torch.from_numpy(X))
    assert isinstance(Yn, torch.Tensor) and isinstance(Yt, torch.Tensor)
    assert Yn.global_length == 60
    np.testing.assert_array_equal(to_np(Yn), to_np(Yt))
    np.testing.assert_allclose(to_np(Yt), S @ X, rtol=1e-10, atol=1e-12)


def test_matmat_promotes_f32_matrix_f64_block():
    S = sample_csr(60, 47, 0.1, seed=1, dtype=np.float32)
    X = _block(47, 3, np.float64)
    Y = lsp.csr_array(S).matmat(X)
    assert Y.dtype == torch.float64
    np.testing.assert_allclose(to_np(Y), S.astype(np.float64) @ X,
                               rtol=1e-10, atol=1e-12)


def test_matmat_rejects_non_float_and_non_2d():
    A = lsp.csr_array(sample_csr(10, 8, 0.3, seed=1))
    with pytest.raises(NotImplementedError):
        A.matmat(np.ones((8, 2), dtype=np.int64))
    with pytest.raises(ValueError):
        A.matmat(np.ones(8))
    with pytest.raises(ValueError):
        A.matmat(np.ones((7, 2)))  # neither global nor shard row count


@pytest.mark.parametrize("kind", ["numpy", "torch"])
def test_matmat_column_major_warns(kind):
    S = sample_csr(60, 47, 0.1, seed=1)
    X = _block(47, 3, np.float64)
    Xf = np.asfortranarray(X)
    op = Xf if kind == "numpy" else torch.from_numpy(X.T.copy()).t()
    assert tuple(op.shape) == (47, 3)
    with pytest.warns(RuntimeWarning, match="implicit copy"):
        Y = lsp.csr_array(S).matmat(op)
    np.testing.assert_allclose(to_np(Y), S @ X, rtol=1e-10, atol=1e-12)
    # a row-major operand stays silent
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        lsp.csr_array(S).matmat(X)


def test_matmat_bad_out_raises():
    S = sample_csr(60, 47, 0.1, seed=1)
    A = lsp.csr_array(S)
    X = _block(47, 3, np.float64)
    bad = [
        torch.empty((60, 3), dtype=torch.float32),         # wrong dtype
        torch.empty((60, 4), dtype=torch.float64),         # wrong shape
        torch.empty((3, 60), dtype=torch.float64),         # transposed shape
        torch.empty(180, dtype=torch.float64),             # 1-D
        torch.empty((60, 6), dtype=torch.float64)[:, ::2],  # non-contiguous
        torch.empty((3, 60), dtype=torch.float64).t(),     # column-major
        np.empty((60, 3), dtype=np.float32),               # numpy, wrong dtype
        np.empty((59, 3), dtype=np.float64),               # numpy, wrong rows
        np.empty((60, 2), dtype=np.float64),               # numpy, wrong k
        np.empty(180, dtype=np.float64),                   # numpy, 1-D
    ]
    for out in bad:
        with pytest.raises(ValueError):
            A.matmat(X, out=out)


def test_matmat_good_out_filled():
    S = sample_csr(60, 47, 0.1, seed=1)
    A = lsp.csr_array(S)
    X = _block(47, 3, np.float64)
    out_t = torch.full((60, 3), np.nan, dtype=torch.float64)
    r = A.matmat(X, out=out_t)
    assert r.data_ptr() == out_t.data_ptr()
    np.testing.assert_allclose(out_t.numpy(), S @ X, rtol=1e-10, atol=1e-12)
    out_n = np.full((60, 3), np.nan)
    r = A.matmat(X, out=out_n)
    assert r is out_n
    np.testing.assert_allclose(out_n, S @ X, rtol=1e-10, atol=1e-12)


def test_spmm_free_function_writes_into_y():
    S = sample_csr(60, 47, 0.1, seed=1)
    X = _block(47, 5, np.float64)
    Y = torch.full((60, 5), np.nan, dtype=torch.float64)
    lsp.spmm(lsp.csr_array(S), torch.from_numpy(X), Y)
    np.testing.assert_allclose(Y.numpy(), S @ X, rtol=1e-10, atol=1e-12)


def _torch_reference(indptr, indices, vals, X, col_offset):
    n = indptr.numel() - 1
    ref = torch.zeros((n, X.shape[1]), dtype=vals.dtype)
    for i in range(n):
        for jp in range(int(indptr[i]), int(indptr[i + 1])):
            ref[i] += vals[jp] * X[int(indices[jp]) - col_offset]
    return ref


def _window_case(k=3, off=13):
    S = sample_csr(30, 21, 0.2, seed=4)
    indptr = torch.from_numpy(S.indptr.astype(np.int64))
    indices = torch.from_numpy(S.indices.astype(np.int32)) + off
    vals = torch.from_numpy(S.data)
    X = torch.from_numpy(_block(21, k, np.float64))
    return indptr, indices, vals, X


def test_ops_spmm_col_offset_accumulate():
    indptr, indices, vals, X = _window_case()
    ref = _torch_reference(indptr, indices, vals, X, 13)
    Y0 = torch.from_numpy(_block(30, 3, np.float64, seed=9))
    Y = Y0.clone()
    r = ops.spmm(indptr, indices, vals, X, Y, accumulate=True,
                 col_offset=13)
    assert r.data_ptr() == Y.data_ptr()
    np.testing.assert_allclose(Y.numpy(), (Y0 + ref).numpy(), rtol=1e-10,
                               atol=1e-12)
    Y = Y0.clone()
    ops.spmm(indptr, indices, vals, X, Y, col_offset=13)
    np.testing.assert_allclose(Y.numpy(), ref.numpy(), rtol=1e-10,
                               atol=1e-12)


def test_ops_spmm_path_validation():
    indptr, indices, vals, X = _window_case(k=ops.SPMM_NARROW_KMAX + 1)
    with pytest.raises(ValueError):
        ops.spmm(indptr, indices, vals, X, col_offset=13, path="fast")
    with pytest.raises(ValueError):
        ops.spmm(indptr, indices, vals, X, col_offset=13, path="narrow")
    ops.spmm(indptr, indices, vals, X, col_offset=13, path="wide")
    assert 1 <= ops.SPMM_NARROW_MAX <= ops.SPMM_NARROW_KMAX


@pytest.mark.parametrize("dtype", [np.float64, np.complex64])
def test_ops_spmm_torch_path_matches_native(monkeypatch, dtype):
    assert _cext.has_cpu()
    S = sample_csr(60, 47, 0.1, seed=1, dtype=dtype)
    indptr = torch.from_numpy(S.indptr.astype(np.int64))
    indices = torch.from_numpy(S.indices.astype(np.int64)) + 13
    vals = torch.from_numpy(S.data)
    X = torch.from_numpy(_block(47, 5, dtype))
    Y0 = torch.from_numpy(_block(60, 5, dtype, seed=9))
    for acc in (False, True):
        native = ops.spmm(indptr, indices, vals, X, Y0.clone(),
                          accumulate=acc, col_offset=13)
        with monkeypatch.context() as m:
            # the extension-less route: the same torch index_add_ code that
            # LS_FORCE_FALLBACK=1 selects for GPU tensors
            m.setattr(_cext, "has_cpu", lambda: False)
            eager = ops.spmm(indptr, indices, vals, X, Y0.clone(),
                             accumulate=acc, col_offset=13)
        np.testing.assert_allclose(eager.numpy(), native.numpy(),
                                   **_tol(dtype))
        want = S @ X.numpy() + (Y0.numpy() if acc else 0)
        np.testing.assert_allclose(native.numpy(), want, **_tol(dtype))


def test_matmul_2d_dense_still_rejected():
    A = lsp.csr_array(sample_csr(4, 4, 0.5, seed=1))
    with pytest.raises(NotImplementedError):
        A @ np.ones((4, 2))


# ---------------------------------------------------------------------------
# LinearOperator block products
# ---------------------------------------------------------------------------
def test_linear_operator_sparse_matmat_rmatmat():
    S = sample_csr(37, 23, 0.2, seed=2, dtype=np.complex128)
    op = linalg.aslinearoperator(lsp.csr_array(S))
    X = _block(23, 3, np.complex128)
    Z = _block(37, 4, np.complex128, seed=8)
    np.testing.assert_allclose(to_np(op.matmat(X)), S @ X, rtol=1e-10,
                               atol=1e-12)
    np.testing.assert_allclose(to_np(op.rmatmat(Z)), S.conj().T @ Z,
                               rtol=1e-10, atol=1e-12)
    AH = op._AH
    op.rmatmat(Z)
    assert op._AH is AH  # the adjoint is cached


def test_linear_operator_user_matvec_matmat():
    S = sample_csr(37, 23, 0.2, seed=2)
    St = sp.csr_array(S.T)
    op = linalg.LinearOperator(
        (37, 23), matvec=lambda v: torch.from_numpy(S @ to_np(v)),
        rmatvec=lambda v: torch.from_numpy(St @ to_np(v)),
        dtype=np.float64)
    X = torch.from_numpy(_block(23, 3, np.float64))
    Z = torch.from_numpy(_block(37, 2, np.float64, seed=8))
    Y = op.matmat(X)
    assert tuple(Y.shape) == (37, 3)
    np.testing.assert_allclose(to_np(Y), S @ X.numpy(), rtol=1e-10,
                               atol=1e-12)
    np.testing.assert_allclose(to_np(op.rmatmat(Z)), S.T @ Z.numpy(),
                               rtol=1e-10, atol=1e-12)
    # numpy in, numpy-returning matvec: stacked as numpy
    op_n = linalg.LinearOperator((37, 23), matvec=lambda v: S @ v,
                                 dtype=np.float64)
    Yn = op_n.matmat(X.numpy())
    assert isinstance(Yn, np.ndarray)
    np.testing.assert_allclose(Yn, S @ X.numpy(), rtol=1e-10, atol=1e-12)
    assert tuple(op.matmat(X[:, :0]).shape) == (37, 0)


def test_identity_operator_matmat_copies():
    op = linalg.IdentityOperator((9, 9), dtype=np.float64)
    X = torch.from_numpy(_block(9, 3, np.float64))
    Y = op.matmat(X)
    assert torch.equal(Y, X) and Y.data_ptr() != X.data_ptr()
    Z = op.rmatmat(X.numpy())
    assert isinstance(Z, np.ndarray) and not np.shares_memory(Z, X.numpy())
    np.testing.assert_array_equal(Z, X.numpy())

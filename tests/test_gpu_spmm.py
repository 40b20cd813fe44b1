# SPDX-License-Identifier: Apache-2.0
"""GPU numerics of the SpMM HIP kernels (src/hip/spmm.hip): both lane
mappings, every tile edge, misaligned operands, windows and accumulate —
against scipy.sparse products (pytest -m gpu on an MI355X)."""
import numpy as np
import pytest
import scipy.sparse as sp

import legate_sparse as lsp
from legate_sparse import ops
from testutils import sample_csr, banded_matrix, to_np

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

DTYPES = [np.float32, np.float64, np.complex64, np.complex128]


@pytest.fixture(scope="module", autouse=True)
def _check_native():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from legate_sparse import _cext
    # GPU runs MUST use the gfx950 extension — no silent fallback
    ext = _cext.require_hip()
    assert ops.SPMM_NARROW_MAX <= ops.SPMM_NARROW_KMAX
    assert ops.SPMM_NARROW_KMAX == ext.SPMM_NARROW_KMAX
    yield


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


def _dev_csr(S, idx_dtype=np.int32, col_offset=0):
    return (torch.from_numpy(S.indptr.astype(np.int64)).cuda(),
            torch.from_numpy(S.indices.astype(idx_dtype) + col_offset).cuda(),
            torch.from_numpy(S.data).cuda())


def _run_ops(S, X, path, **kw):
    indptr, indices, vals = _dev_csr(S)
    Y = ops.spmm(indptr, indices, vals, torch.from_numpy(X).cuda(),
                 path=path, **kw)
    assert Y.is_cuda and tuple(Y.shape) == (S.shape[0], X.shape[1])
    return to_np(Y)


_S500 = {}


def _sample500(dtype):
    key = np.dtype(dtype).name
    if key not in _S500:
        _S500[key] = sample_csr(500, 431, 0.05, seed=1, dtype=dtype)
    return _S500[key]


@pytest.mark.parametrize("k", [1, 2, 3, 4])
@pytest.mark.parametrize("path", ["narrow", "wide"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_gpu_spmm_dtypes_paths_small_k(dtype, path, k):
    S = _sample500(dtype)
    X = _block(431, k, dtype)
    np.testing.assert_allclose(_run_ops(S, X, path), S @ X, **_tol(dtype))


_S300 = {}


@pytest.mark.parametrize("k", [5, 7, 8, 9, 16, 17, 31, 32, 33, 63, 64, 65,
                               127, 128, 129, 257])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_gpu_spmm_wide_tile_edges(dtype, k):
    key = np.dtype(dtype).name
    if key not in _S300:
        _S300[key] = sample_csr(300, 211, 0.05, seed=2, dtype=dtype)
    S = _S300[key]
    X = _block(211, k, dtype)
    np.testing.assert_allclose(_run_ops(S, X, "wide"), S @ X, **_tol(dtype))


@pytest.mark.parametrize("k", [2, 8])
@pytest.mark.parametrize("nnz_per_row", [1, 7, 33, 101])
def test_gpu_spmm_row_lengths_auto(nnz_per_row, k):
    # sweeps the W (narrow) and G (wide) selections
    n = 2000
    S = banded_matrix(n, nnz_per_row=nnz_per_row)
    X = _block(n, k, np.float64)
    Y = lsp.csr_array(S).matmat(torch.from_numpy(X).cuda())
    assert Y.is_cuda
    np.testing.assert_allclose(to_np(Y), S @ X, rtol=1e-10, atol=1e-12)


@pytest.mark.parametrize("path", ["narrow", "wide"])
def test_gpu_spmm_long_single_row(path):
    # one dense row among 999 diagonal rows
    n = 1000
    D = np.zeros((n, n))
    D[0, :] = np.random.default_rng(4).standard_normal(n)
    D[np.arange(1, n), np.arange(1, n)] = 2.0
    S = sp.csr_array(D)
    X = _block(n, 5, np.float64)
    np.testing.assert_allclose(_run_ops(S, X, path), S @ X, rtol=1e-10,
                               atol=1e-12)


@pytest.mark.parametrize("k", [5, 6, 7, 8])
@pytest.mark.parametrize("dtype", DTYPES)
def test_gpu_spmm_narrow_upper_k(dtype, k):
    # the narrow kernel is instantiated past the auto crossover
    S = _sample500(dtype)
    X = _block(431, k, dtype)
    np.testing.assert_allclose(_run_ops(S, X, "narrow"), S @ X,
                               **_tol(dtype))


def test_gpu_spmm_narrow_past_limit_raises():
    S = _sample500(np.float64)
    X = _block(431, ops.SPMM_NARROW_KMAX + 1, np.float64)
    with pytest.raises(ValueError):
        _run_ops(S, X, "narrow")


@pytest.mark.parametrize("path", ["narrow", "wide"])
def test_gpu_spmm_empty_rows(path):
    D = sample_csr(200, 150, 0.05, seed=3).toarray()
    D[[0, 5, 6, 64, 199], :] = 0.0
    S = sp.csr_array(D)
    X = _block(150, 3, np.float64)
    got = _run_ops(S, X, path)
    np.testing.assert_allclose(got, S @ X, rtol=1e-10, atol=1e-12)
    assert not got[[0, 5, 6, 64, 199]].any()
    # under accumulate an empty row leaves Y untouched
    Y0 = _block(200, 3, np.float64, seed=9)
    got = _run_ops(S, X, path, Y=torch.from_numpy(Y0).cuda(),
                   accumulate=True)
    np.testing.assert_array_equal(got[[0, 5, 6, 64, 199]],
                                  Y0[[0, 5, 6, 64, 199]])
    np.testing.assert_allclose(got, Y0 + S @ X, rtol=1e-10, atol=1e-12)


@pytest.mark.parametrize("k", [3, 8])
def test_gpu_spmm_int64_indices(k):
    S = _sample500(np.float64)
    indptr, indices, vals = _dev_csr(S, idx_dtype=np.int64)
    assert indices.dtype == torch.int64
    X = _block(431, k, np.float64)
    Y = ops.spmm(indptr, indices, vals, torch.from_numpy(X).cuda())
    np.testing.assert_allclose(to_np(Y), S @ X, rtol=1e-10, atol=1e-12)


@pytest.mark.parametrize("path", ["narrow", "wide"])
@pytest.mark.parametrize("k", [4, 3])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_gpu_spmm_misaligned_views(dtype, k, path):
    # X and Y start one element into a larger buffer: k = 4 keeps the row
    # stride 16-byte aligned with a misaligned base, k = 3 misaligns the
    # stride as well — both must take the element-wise path
    S = _sample500(dtype)
    indptr, indices, vals = _dev_csr(S)
    X = _block(431, k, dtype)
    xbuf = torch.zeros(431 * k + 1, dtype=vals.dtype, device="cuda")
    xbuf[1:] = torch.from_numpy(X).cuda().reshape(-1)
    ybuf = torch.full((500 * k + 2,), 7.0, dtype=vals.dtype, device="cuda")
    Xv = xbuf[1:].view(431, k)
    Yv = ybuf[1:-1].view(500, k)
    assert Xv.data_ptr() % 16 != 0 and Yv.data_ptr() % 16 != 0
    ops.spmm(indptr, indices, vals, Xv, Yv, path=path)
    np.testing.assert_allclose(to_np(Yv), S @ X, **_tol(dtype))
    # nothing written outside the view
    assert float(ybuf[0]) == 7.0 and float(ybuf[-1]) == 7.0


@pytest.mark.parametrize("accumulate", [False, True])
@pytest.mark.parametrize("path", ["narrow", "wide"])
@pytest.mark.parametrize("k", [3, 4])
def test_gpu_spmm_col_offset(k, path, accumulate):
    S = sample_csr(300, 211, 0.05, seed=2)
    indptr, indices, vals = _dev_csr(S, col_offset=13)
    X = _block(211, k, np.float64)
    Y0 = _block(300, k, np.float64, seed=9)
    Y = torch.from_numpy(Y0).cuda()
    ops.spmm(indptr, indices, vals, torch.from_numpy(X).cuda(), Y,
             accumulate=accumulate, col_offset=13, path=path)
    want = S @ X + (Y0 if accumulate else 0.0)
    np.testing.assert_allclose(to_np(Y), want, rtol=1e-10, atol=1e-12)


@pytest.mark.parametrize("k", [4, 32, 33])
def test_gpu_spmm_bit_identical_runs(k):
    S = _sample500(np.float64)
    A = lsp.csr_array(S)
    X = torch.from_numpy(_block(431, k, np.float64)).cuda()
    a = A.matmat(X)
    b = A.matmat(X)
    assert torch.equal(a, b)


@pytest.mark.parametrize("dtype", DTYPES)
def test_gpu_matmat_matches_stacked_spmv(dtype):
    S = _sample500(dtype)
    A = lsp.csr_array(S)
    X = torch.from_numpy(_block(431, 6, dtype)).cuda()
    Y = A.matmat(X)
    cols = torch.stack([(A @ X[:, j].contiguous()).reshape(-1)
                        for j in range(6)], dim=1)
    np.testing.assert_allclose(to_np(Y), to_np(cols), **_tol(dtype))
    np.testing.assert_allclose(to_np(Y), S @ to_np(X), **_tol(dtype))


def test_gpu_matmat_out_on_wrong_device_raises():
    S = _sample500(np.float64)
    A = lsp.csr_array(S)
    X = torch.from_numpy(_block(431, 3, np.float64)).cuda()
    with pytest.raises(ValueError):
        A.matmat(X, out=torch.empty((500, 3), dtype=torch.float64))
    out = torch.empty((500, 3), dtype=torch.float64, device="cuda")
    A.matmat(X, out=out)
    np.testing.assert_allclose(to_np(out), S @ to_np(X), rtol=1e-10,
                               atol=1e-12)

# SPDX-License-Identifier: Apache-2.0
"""GPU numerics: every HIP kernel vs a plain fp32/fp64 torch/scipy
reference (run on the MI355X box via gpurun; pytest -m gpu)."""
import numpy as np
import pytest
import scipy.sparse as sp

import legate_sparse as lsp
from testutils import sample_csr, banded_matrix, to_np

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(),
                                  reason="no GPU")


@pytest.fixture(scope="module", autouse=True)
def _check_native():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from legate_sparse import _cext
    # GPU runs MUST use the gfx950 extension — no silent fallback
    _cext.require_hip()
    yield


@pytest.mark.parametrize("dtype",
                         [np.float32, np.float64, np.complex64,
                          np.complex128])
def test_gpu_spmv_dtypes(dtype):
    S = sample_csr(500, 431, 0.05, seed=1, dtype=dtype)
    rng = np.random.default_rng(2)
    x = rng.standard_normal(431).astype(dtype)
    if np.dtype(dtype).kind == "c":
        x = x + 1j * rng.standard_normal(431).astype(dtype)
    A = lsp.csr_array(S)
    assert A.data.is_cuda
    y = A @ torch.from_numpy(x).cuda()
    tol = 1e-4 if np.dtype(dtype).itemsize <= 8 else 1e-12
    np.testing.assert_allclose(to_np(y), S @ x, rtol=tol, atol=tol)


@pytest.mark.parametrize("nnz_per_row",
                         [1, 3, 5, 7, 9, 11, 15, 17, 31, 33, 101])
def test_gpu_spmv_row_lengths(nnz_per_row):
    # banded rows: up to 15 per row the affine plan accepts the matrix and
    # the product runs spmv_affine*; only 17 and 31 (pairu W=4), 33 (pair
    # W=8) and 101 (pair W=16) reach the general launcher.  Its kernels and
    # W selection are swept in test_gpu_spmv.py.
    n = 2000
    S = banded_matrix(n, nnz_per_row=min(nnz_per_row, n // 2) | 1)
    x = np.random.default_rng(3).standard_normal(n)
    y = lsp.csr_array(S) @ torch.from_numpy(x).cuda()
    np.testing.assert_allclose(to_np(y), S @ x, rtol=1e-10, atol=1e-12)


def test_gpu_spmv_long_single_row():
    # one dense row among short rows (wave-loop path)
    n = 1000
    D = np.zeros((n, n))
    D[0, :] = np.random.default_rng(4).standard_normal(n)
    D[np.arange(1, n), np.arange(1, n)] = 2.0
    S = sp.csr_array(D)
    x = np.random.default_rng(5).standard_normal(n)
    y = lsp.csr_array(S) @ torch.from_numpy(x).cuda()
    np.testing.assert_allclose(to_np(y), S @ x, rtol=1e-10, atol=1e-12)


@pytest.mark.parametrize("dtype", [np.float32, np.float64, np.complex128])
def test_gpu_spgemm_small_bin(dtype):
    # 5 per row on both sides: the affine product takes every interior
    # row; only the boundary rows reach the general path (merge W = 8)
    A = banded_matrix(300, nnz_per_row=5).astype(dtype)
    C = lsp.csr_array(A) @ lsp.csr_array(A)
    tol = 1e-4 if np.dtype(dtype).itemsize <= 8 else 1e-12
    np.testing.assert_allclose(to_np(C.todense()), (A @ A).toarray(),
                               rtol=tol, atol=tol)


def test_gpu_spgemm_mid_bin():
    # ~30 nnz/row squared: ub in (128, 1024] with a_len <= 32, so every
    # row runs the merge kernel W = 32, none an LDS-hash bin (those need
    # a_len > 64; test_gpu_spgemm.py covers them)
    A = banded_matrix(400, nnz_per_row=31)
    C = lsp.csr_array(A) @ lsp.csr_array(A)
    np.testing.assert_allclose(to_np(C.todense()), (A @ A).toarray(),
                               rtol=1e-10, atol=1e-11)


def test_gpu_spgemm_large_bin():
    # ub in (1024, 4096] with a_len <= 64: merge kernels W = 32 and W = 64
    A = banded_matrix(600, nnz_per_row=57)
    C = lsp.csr_array(A) @ lsp.csr_array(A)
    np.testing.assert_allclose(to_np(C.todense()), (A @ A).toarray(),
                               rtol=1e-10, atol=1e-11)


def test_gpu_spgemm_global_bin():
    # a fully dense row drives ub ~ n*avg > 4096 -> HBM hash fallback
    n = 700
    D = (np.random.default_rng(6).random((n, n)) > 0.98).astype(float)
    D[0, :] = 1.0
    D[:, 0] = 1.0
    S = sp.csr_array(D)
    C = lsp.csr_array(S) @ lsp.csr_array(S)
    np.testing.assert_allclose(to_np(C.todense()), (S @ S).toarray(),
                               rtol=1e-10, atol=1e-11)


def test_gpu_spgemm_mixed_bins():
    # matrix whose rows span all four bins in one call
    n = 800
    rng = np.random.default_rng(7)
    rows, cols, vals = [], [], []
    for i in range(n):
        if i < 4:
            nnz = n  # dense row -> global bin
        elif i < 40:
            nnz = 60
        elif i < 400:
            nnz = 12
        else:
            nnz = 3
        c = rng.choice(n, size=min(nnz, n), replace=False)
        rows.extend([i] * len(c))
        cols.extend(c.tolist())
        vals.extend(rng.standard_normal(len(c)).tolist())
    S = sp.csr_array((vals, (rows, cols)), shape=(n, n))
    C = lsp.csr_array(S) @ lsp.csr_array(S)
    np.testing.assert_allclose(to_np(C.todense()), (S @ S).toarray(),
                               rtol=1e-10, atol=1e-10)


@pytest.mark.parametrize("isalpha", [True, False])
@pytest.mark.parametrize("negate", [True, False])
@pytest.mark.parametrize("dtype", [np.float64, np.complex128])
def test_gpu_axpby(isalpha, negate, dtype):
    from legate_sparse.linalg import cg_axpby
    rng = np.random.default_rng(8)
    n = 10000

    def mk(seed):
        v = rng.standard_normal(n)
        if np.dtype(dtype).kind == "c":
            v = v + 1j * rng.standard_normal(n)
        return v.astype(dtype)

    y0, x0 = mk(1), mk(2)
    a = np.array([1.7], dtype=dtype)
    b = np.array([-0.4], dtype=dtype)
    y = torch.from_numpy(y0.copy()).cuda()
    x = torch.from_numpy(x0.copy()).cuda()
    cg_axpby(y, x, torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda(),
             isalpha=isalpha, negate=negate)
    val = (-1 if negate else 1) * a[0] / b[0]
    want = val * x0 + y0 if isalpha else x0 + val * y0
    np.testing.assert_allclose(to_np(y), want, rtol=1e-12)


@pytest.mark.parametrize("dtype", [np.float32, np.float64, np.complex128])
def test_gpu_vdot(dtype):
    from legate_sparse import ops
    rng = np.random.default_rng(9)
    n = 100003
    x = rng.standard_normal(n)
    y = rng.standard_normal(n)
    if np.dtype(dtype).kind == "c":
        x = x + 1j * rng.standard_normal(n)
        y = y + 1j * rng.standard_normal(n)
    x = x.astype(dtype)
    y = y.astype(dtype)
    got = ops.vdot(torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda())
    want = np.vdot(x, y)
    tol = 1e-3 if np.dtype(dtype).itemsize <= 8 else 1e-10
    np.testing.assert_allclose(to_np(got)[0], want, rtol=tol)


def test_gpu_dense_csr_roundtrip():
    rng = np.random.default_rng(10)
    D = rng.standard_normal((123, 77))
    D[rng.random((123, 77)) < 0.6] = 0.0
    A = lsp.csr_array(torch.from_numpy(D).cuda())
    S = sp.csr_array(D)
    assert A.nnz == S.nnz
    np.testing.assert_array_equal(to_np(A.indptr), S.indptr)
    np.testing.assert_array_equal(to_np(A.indices), S.indices)
    np.testing.assert_allclose(to_np(A.todense()), D)


def test_gpu_diagonal():
    S = sample_csr(211, 211, 0.05, seed=11)
    A = lsp.csr_array(S)
    np.testing.assert_allclose(to_np(A.diagonal()), S.diagonal())


def test_gpu_transpose():
    S = sample_csr(150, 90, 0.1, seed=12)
    A = lsp.csr_array(S)
    np.testing.assert_allclose(to_np(A.T.todense()), S.T.toarray())


def test_gpu_cg_poisson():
    from legate_sparse.gallery import poisson_2d
    A = poisson_2d(64, 64)
    assert A.data.is_cuda
    b = torch.ones(A.shape[0], dtype=torch.float64, device="cuda")
    x, iters = lsp.linalg.cg(A, b, rtol=1e-10, maxiter=2000)
    assert 0 < iters < 2000
    r = to_np(b - A @ x)
    assert np.linalg.norm(r) <= 1e-8 * np.linalg.norm(to_np(b))


def test_gpu_gmres_poisson():
    from legate_sparse.gallery import poisson_2d
    A = poisson_2d(32, 32)
    b = torch.ones(A.shape[0], dtype=torch.float64, device="cuda")
    x, info = lsp.linalg.gmres(A, b, rtol=1e-8, restart=50, maxiter=3000)
    assert info == 0


def test_gpu_ufuncs_and_scalars():
    S = sample_csr(100, 100, 0.05, seed=13)
    A = lsp.csr_array(S)
    got = (A * 2.0).tanh()
    want = S.copy()
    want.data = np.tanh(2.0 * S.data)
    np.testing.assert_allclose(to_np(got.todense()), want.toarray(),
                               rtol=1e-12)


def test_gpu_spgemm_fast_mode(monkeypatch):
    """LS_FAST_SPGEMM (ALG1-style: allocate by upper bound, skip
    symbolic) must give identical results to the exact 2-phase path."""
    monkeypatch.setenv("LS_FAST_SPGEMM", "1")
    n = 800
    rng = np.random.default_rng(21)
    rows, cols, vals = [], [], []
    for i in range(n):
        nnz = n if i < 3 else (60 if i < 30 else (12 if i < 300 else 3))
        c = rng.choice(n, size=min(nnz, n), replace=False)
        rows.extend([i] * len(c))
        cols.extend(c.tolist())
        vals.extend(rng.standard_normal(len(c)).tolist())
    S = sp.csr_array((vals, (rows, cols)), shape=(n, n))
    C = lsp.csr_array(S) @ lsp.csr_array(S)
    np.testing.assert_allclose(to_np(C.todense()), (S @ S).toarray(),
                               rtol=1e-10, atol=1e-10)


def test_gpu_rmat_spgemm():
    """R-MAT adjacency squared (power-law rows span every bin)."""
    from legate_sparse.gallery import rmat
    A = rmat(12, edge_factor=8, seed=3)
    r, c, v = A.tocoo()
    S = sp.csr_array((to_np(v), (to_np(r), to_np(c))), shape=A.shape)
    C = A @ A
    np.testing.assert_allclose(to_np(C.todense()), (S @ S).toarray(),
                               rtol=1e-9, atol=1e-9)


@pytest.mark.parametrize("nnz_per_row", [31, 57])
def test_gpu_spgemm_complex_big_bins(nnz_per_row):
    """complex128 through the merge kernels (a_len <= 64, ub <= 4096: no
    row reaches an LDS-hash bin; the reduced complex128 geometries are
    checked in test_gpu_spgemm.py)."""
    A = banded_matrix(500, nnz_per_row=nnz_per_row).astype(np.complex128)
    A = A + 1j * banded_matrix(500, nnz_per_row=nnz_per_row, seed=9)
    A = A.tocsr()
    C = lsp.csr_array(A) @ lsp.csr_array(A)
    np.testing.assert_allclose(to_np(C.todense()), (A @ A).toarray(),
                               rtol=1e-10, atol=1e-10)


def test_gpu_spgemm_fast_vs_exact_identical():
    import os
    A = banded_matrix(3000, nnz_per_row=9)
    La = lsp.csr_array(A)
    C1 = La @ La
    os.environ["LS_FAST_SPGEMM"] = "1"
    try:
        C2 = La @ La
    finally:
        del os.environ["LS_FAST_SPGEMM"]
    np.testing.assert_array_equal(to_np(C1.indptr), to_np(C2.indptr))
    np.testing.assert_array_equal(to_np(C1.indices), to_np(C2.indices))
    np.testing.assert_allclose(to_np(C1.data), to_np(C2.data), rtol=1e-14)


def test_gpu_jacobi_update():
    from legate_sparse import ops
    rng = np.random.default_rng(30)
    n = 50000
    x0 = rng.standard_normal(n)
    b = rng.standard_normal(n)
    y = rng.standard_normal(n)
    dinv = rng.random(n) + 0.5
    x = torch.from_numpy(x0.copy()).cuda()
    ops.jacobi_update(x, torch.from_numpy(b).cuda(),
                      torch.from_numpy(y).cuda(),
                      torch.from_numpy(dinv).cuda(), 0.8)
    want = x0 + 0.8 * dinv * (b - y)
    np.testing.assert_allclose(to_np(x), want, rtol=1e-12, atol=1e-13)


def test_gpu_spgemm_deterministic():
    """The affine product and the merge bins (the boundary rows here) must
    give bit-identical results across runs (binning order is
    nondeterministic but per-row outputs are not).  No row reaches a hash
    bin, which accumulates with atomics and promises no such thing."""
    A = banded_matrix(2000, nnz_per_row=9, seed=31)
    La = lsp.csr_array(A)
    C1 = La @ La
    C2 = La @ La
    assert torch.equal(C1._indptr, C2._indptr)
    assert torch.equal(C1._indices, C2._indices)
    assert torch.equal(C1._data, C2._data)


@pytest.mark.gpu
def test_spgemm_structure_cache_repeated_products():
    """Repeated A@B on unchanged structure hits the binning/symbolic
    cache; results must be identical, values-only changes must flow
    through, structure changes must invalidate."""
    S = sample_csr(300, 300, 0.05, seed=50)
    T = sample_csr(300, 300, 0.05, seed=51)
    A = lsp.csr_array(S)
    B = lsp.csr_array(T)
    C1 = A @ B
    C2 = A @ B  # cache hit
    want = (S @ T).toarray()
    np.testing.assert_allclose(to_np(C1.todense()), want, rtol=1e-12)
    np.testing.assert_allclose(to_np(C2.todense()), want, rtol=1e-12)
    assert C1.indptr.data_ptr() != C2.indptr.data_ptr()  # no aliasing
    # values-only change: cache stays valid, numeric recomputes
    A.data = A.data * 2.0
    C3 = A @ B
    np.testing.assert_allclose(to_np(C3.todense()), 2.0 * want,
                               rtol=1e-12)
    # structure change invalidates
    A.eliminate_zeros()
    C4 = A @ B
    np.testing.assert_allclose(to_np(C4.todense()), 2.0 * want,
                               rtol=1e-12)


@pytest.mark.gpu
def test_spmv_affine_poisson_gpu():
    """Affine kernel (no index stream) vs torch fallback on Poisson."""
    import legate_sparse.gallery as gal
    from legate_sparse import ops as lops
    A = gal.poisson_2d(257, 131)  # non-square grid, odd sizes
    plan = A._affine_plan()
    assert plan is not None
    x = torch.rand(A.shape[1], dtype=torch.float64, device="cuda")
    y_aff = lops.spmv(A._indptr, A._indices, A._data, x, affine=plan)
    import os as _os
    _os.environ["LS_SPMV_AFFINE_V"] = "2"
    y_aff2 = lops.spmv(A._indptr, A._indices, A._data, x, affine=plan)
    del _os.environ["LS_SPMV_AFFINE_V"]
    y_gen = lops.spmv(A._indptr, A._indices, A._data, x, affine=None)
    prod = A._data * x[A._indices.long()]
    rid = torch.repeat_interleave(
        torch.arange(A.shape[0], device="cuda"),
        A._indptr[1:] - A._indptr[:-1])
    y_ref = torch.zeros_like(y_aff).index_add_(0, rid, prod)
    assert torch.allclose(y_aff, y_ref, rtol=1e-13, atol=1e-13)
    assert torch.allclose(y_aff2, y_ref, rtol=1e-13, atol=1e-13)
    assert torch.allclose(y_gen, y_ref, rtol=1e-13, atol=1e-13)
    # accumulate path
    y0 = torch.rand_like(y_aff)
    y_acc = y0.clone()
    lops.spmv(A._indptr, A._indices, A._data, x, y_acc, accumulate=True,
              affine=plan)
    assert torch.allclose(y_acc, y0 + y_ref, rtol=1e-13, atol=1e-13)


@pytest.mark.gpu
def test_spmv_affine_banded_gpu():
    import scipy.sparse as sp2
    from legate_sparse import ops as lops
    n = 20001
    rng = np.random.default_rng(61)
    S = sp2.diags([rng.random(n - abs(o)) for o in range(-5, 6)],
                  list(range(-5, 6)), shape=(n, n), format="csr")
    A = lsp.csr_array(S)
    plan = A._affine_plan()
    assert plan is not None and plan[0] == 11
    x = np.random.default_rng(62).random(n)
    y = A @ x
    np.testing.assert_allclose(to_np(y), S @ x, rtol=1e-12)


@pytest.mark.gpu
def test_spmv_affine_through_cg():
    """The whole solver pipeline on an affine-detected operator."""
    import legate_sparse.gallery as gal
    A = gal.poisson_2d(128, 128)
    b = np.ones(A.shape[0])
    x, iters = lsp.linalg.cg(A, b, rtol=1e-10, maxiter=2000)
    r = to_np(b - A @ x)
    assert np.linalg.norm(r) <= 1e-8 * np.linalg.norm(b)


@pytest.mark.gpu
def test_spmv_fused_dot_gpu():
    """q = A p with the p.(Ap) reduction fused into the affine kernel."""
    import legate_sparse.gallery as gal
    from legate_sparse import ops as lops
    A = gal.poisson_2d(301, 211)
    # make square for the pq path
    A = gal.poisson_2d(256, 256)
    p = torch.rand(A.shape[0], dtype=torch.float64, device="cuda")
    q = torch.empty_like(p)
    pq = torch.zeros(1, dtype=torch.float64, device="cuda")
    assert A._matvec_pq(p, q, pq)
    q_ref = lops.spmv(A._indptr, A._indices, A._data, p)
    assert torch.allclose(q, q_ref, rtol=1e-13, atol=1e-13)
    want = float(torch.dot(p, q_ref))
    assert abs(float(pq) - want) <= 1e-10 * abs(want)


@pytest.mark.gpu
def test_spmv_affine_interior_piece_with_offset():
    """The distributed interior split piece: affine plan built on the
    piece tensors, kernel reading through an offset x base pointer —
    exactly the 8-GPU _matvec_dist path, validated on one GPU."""
    import legate_sparse.gallery as gal
    from legate_sparse import ops as lops
    from legate_sparse.csr import _build_affine_plan
    A = gal.poisson_2d(128, 128)
    N = A.shape[0]
    # emulate rank 0 of a 2-rank split: local rows [0, cut), interior
    # columns [0, cut) — the piece csr built exactly like
    # _split_for_overlap does on the LOCAL row block
    cut = N // 2
    dev = A._data.device
    row_ids = torch.repeat_interleave(
        torch.arange(N, device=dev), A._indptr[1:] - A._indptr[:-1])
    m = (row_ids < cut) & (A._indices.long() < cut)
    cnt = torch.bincount(row_ids[m], minlength=cut)
    ip = torch.zeros(cut + 1, dtype=torch.int64, device=dev)
    torch.cumsum(cnt, dim=0, out=ip[1:])
    ix = A._indices[m].contiguous()
    dv = A._data[m].contiguous()
    plan = _build_affine_plan(ip, ix, max(A.shape))
    # rows away from the shard edge keep all 5 entries -> plan exists
    assert plan is not None and plan[0] == 5
    x = torch.rand(N, dtype=torch.float64, device="cuda")
    y_aff = lops.spmv(ip, ix, dv, x, affine=plan)
    y_gen = lops.spmv(ip, ix, dv, x, affine=None)
    assert torch.allclose(y_aff, y_gen, rtol=1e-14, atol=1e-14)
    # the x-window semantics the dist path uses: kernel reads through
    # an offset base pointer (here offset 0 with the window [0, cut))
    y_off = lops.spmv(ip, ix, dv, x[:cut].contiguous(),
                      col_offset=0, affine=plan)
    assert torch.allclose(y_off, y_gen, rtol=1e-14, atol=1e-14)


@pytest.mark.gpu
def test_spgemm_affine_stencil_product():
    """A@B via the stencil-convolution kernel vs scipy, incl. boundary
    exception rows and repeated-product cache."""
    import legate_sparse.gallery as gal
    import scipy.sparse as sp2
    A = gal.poisson_2d(64, 48)
    S = sp2.csr_matrix(
        (to_np(A.data), to_np(A.indices), to_np(A.indptr)), shape=A.shape)
    C = A @ A
    want = (S @ S).toarray()
    np.testing.assert_allclose(to_np(C.todense()), want, rtol=1e-13)
    assert C.has_sorted_indices
    # repeated (cache hit) + values-only change
    A.data = A.data * 3.0
    C2 = A @ A
    np.testing.assert_allclose(to_np(C2.todense()), 9.0 * want,
                               rtol=1e-13)
    # banded x banded (different offsets)
    n = 5000
    d1 = sp2.diags([np.full(n - abs(o), float(o + 10))
                    for o in (-2, 0, 3)], [-2, 0, 3], format="csr")
    d2 = sp2.diags([np.full(n - abs(o), float(o + 5))
                    for o in (-1, 0, 1, 4)], [-1, 0, 1, 4], format="csr")
    L1, L2 = lsp.csr_array(d1), lsp.csr_array(d2)
    C3 = L1 @ L2
    np.testing.assert_allclose(
        to_np(C3.todense()), (d1 @ d2).toarray(), rtol=1e-13)
    # disabled path agrees
    import os as _os
    _os.environ["LS_SPGEMM_AFFINE"] = "0"
    try:
        C4 = lsp.csr_array(d1) @ lsp.csr_array(d2)
        np.testing.assert_allclose(to_np(C4.todense()),
                                   (d1 @ d2).toarray(), rtol=1e-13)
    finally:
        del _os.environ["LS_SPGEMM_AFFINE"]


@pytest.mark.gpu
def test_affine_diagonal_matrix_paths():
    """nd=1 affine: diagonal matrices hit the index-free kernels for
    SpMV and the stencil-product kernel for A @ D (the reference gmg's
    weighted-Jacobi spectral estimate pattern)."""
    import legate_sparse.gallery as gal
    import scipy.sparse as sp2
    n = 4000
    dvals = np.random.default_rng(70).random(n) + 0.5
    D = lsp.csr_array(sp2.diags([dvals], [0], format="csr"))
    assert D._affine_plan() is not None and D._affine_plan()[0] == 1
    x = np.random.default_rng(71).random(n)
    np.testing.assert_allclose(to_np(D @ x), dvals * x, rtol=1e-13)
    S = sp2.diags([np.ones(n - 1), 2 * np.ones(n), np.ones(n - 1)],
                  [-1, 0, 1], format="csr")
    A = lsp.csr_array(S)
    C = A @ D
    np.testing.assert_allclose(to_np(C.todense()),
                               (S @ sp2.diags([dvals], [0])).toarray(),
                               rtol=1e-13)


@pytest.mark.gpu
def test_spgemm_affine_windowed_B():
    """Distributed-path emulation on one GPU: B arrives as a row WINDOW
    [b_off, b_off+win) with an offset indptr — exactly what
    _gather_B_window hands the stencil-product at world_size > 1."""
    import scipy.sparse as sp2
    from legate_sparse import ops as lops
    from legate_sparse.csr import _build_affine_plan, _index_dtype_for
    n = 6000
    S = sp2.diags([np.full(n - abs(o), float(o + 4))
                   for o in (-2, -1, 0, 1, 2)],
                  [-2, -1, 0, 1, 2], format="csr")
    A = lsp.csr_array(S)
    # emulate "rank" rows = all, B window = rows [b_off, n)
    b_off = 0  # A columns span [0, n): window must cover them all
    Bw_ip = A._indptr.clone()
    Bw_ix = A._indices.clone()
    Bw_dv = A._data.clone()
    planA = A._affine_plan()
    planB = _build_affine_plan(Bw_ip, Bw_ix, n)
    assert planA is not None and planB is not None

    def general_rows(rows):
        ip = A._indptr
        cnts = ip[rows + 1] - ip[rows]
        sub_ip = torch.zeros(rows.numel() + 1, dtype=torch.int64,
                             device=ip.device)
        torch.cumsum(cnts, dim=0, out=sub_ip[1:])
        tot = int(sub_ip[-1])
        ent = (torch.repeat_interleave(ip[rows], cnts)
               + torch.arange(tot, device=ip.device)
               - torch.repeat_interleave(sub_ip[:-1], cnts))
        return lops.spgemm_local(
            sub_ip, A._indices[ent].contiguous(),
            A._data[ent].contiguous(), Bw_ip, Bw_ix, Bw_dv, n,
            b_row_offset=b_off)

    res = lops.spgemm_affine_try(
        A._indptr, A._data, planA, Bw_ip, Bw_dv, planB,
        Bw_ip.numel() - 1, n, general_rows,
        _index_dtype_for((n, n)), cache={}, b_row_off=b_off)
    assert res is not None
    C_ip, C_ix, C_dv = res
    want = (S @ S).tocsr()
    want.sort_indices()
    np.testing.assert_array_equal(to_np(C_ip), want.indptr)
    np.testing.assert_array_equal(to_np(C_ix), want.indices)
    np.testing.assert_allclose(to_np(C_dv), want.data, rtol=1e-13)

    # nonzero b_off: A sub-rows [2000, 4000) only need B rows
    # [1998, 4002) — hand it that window with the offset
    r0, r1 = 2000, 4000
    ipA = (A._indptr[r0:r1 + 1] - A._indptr[r0]).contiguous()
    s_el, e_el = int(A._indptr[r0]), int(A._indptr[r1])
    ixA = A._indices[s_el:e_el].contiguous()
    dvA = A._data[s_el:e_el].contiguous()
    boff = r0 - 2
    wip = (A._indptr[boff:r1 + 2 + 1] - A._indptr[boff]).contiguous()
    ws_el, we_el = int(A._indptr[boff]), int(A._indptr[r1 + 2])
    wix = A._indices[ws_el:we_el].contiguous()
    wdv = A._data[ws_el:we_el].contiguous()
    pA2 = _build_affine_plan(ipA, ixA, n)
    pB2 = _build_affine_plan(wip, wix, n)
    assert pA2 is not None and pB2 is not None

    def general_rows2(rows):
        cnts = ipA[rows + 1] - ipA[rows]
        sub_ip = torch.zeros(rows.numel() + 1, dtype=torch.int64,
                             device=ipA.device)
        torch.cumsum(cnts, dim=0, out=sub_ip[1:])
        tot = int(sub_ip[-1])
        ent = (torch.repeat_interleave(ipA[rows], cnts)
               + torch.arange(tot, device=ipA.device)
               - torch.repeat_interleave(sub_ip[:-1], cnts))
        return lops.spgemm_local(sub_ip, ixA[ent].contiguous(),
                                 dvA[ent].contiguous(), wip, wix, wdv,
                                 n, b_row_offset=boff)

    res2 = lops.spgemm_affine_try(
        ipA, dvA, pA2, wip, wdv, pB2, wip.numel() - 1, n,
        general_rows2, _index_dtype_for((n, n)), cache={},
        b_row_off=boff)
    assert res2 is not None
    C2_ip, C2_ix, C2_dv = res2
    sub_want = want[r0:r1]
    np.testing.assert_array_equal(to_np(C2_ip), sub_want.indptr)
    np.testing.assert_array_equal(to_np(C2_ix), sub_want.indices)
    np.testing.assert_allclose(to_np(C2_dv), sub_want.data, rtol=1e-13)


@pytest.mark.gpu
def test_affine_paths_fp32():
    """fp32 through the affine SpMV and stencil SpGEMM paths."""
    import scipy.sparse as sp2
    n = 3000
    S = sp2.diags([np.ones(n - abs(o), dtype=np.float32) * (o + 3)
                   for o in (-1, 0, 2)], [-1, 0, 2], format="csr")
    A = lsp.csr_array(S, dtype=np.float32)
    assert A.dtype == np.float32
    x = np.random.default_rng(80).random(n).astype(np.float32)
    np.testing.assert_allclose(to_np(A @ x), S @ x, rtol=1e-5)
    C = A @ A
    np.testing.assert_allclose(to_np(C.todense()), (S @ S).toarray(),
                               rtol=1e-5)


@pytest.mark.gpu
def test_spgemm_affine_complex():
    """Complex stencil products through the convolution kernel."""
    import scipy.sparse as sp2
    n = 2000
    rng = np.random.default_rng(95)
    diags = [rng.random(n - abs(o)) + 1j * rng.random(n - abs(o))
             for o in (-1, 0, 1)]
    S = sp2.diags(diags, [-1, 0, 1], format="csr")
    A = lsp.csr_array(S)
    assert A.dtype == np.complex128
    C = A @ A
    np.testing.assert_allclose(to_np(C.todense()), (S @ S).toarray(),
                               rtol=1e-12)


@pytest.mark.gpu
def test_spgemm_segsort_parity():
    """rocPRIM segmented postsort vs the torch composite on a power-law
    product.  With n_cols = 8192 every hub row gets an identity table, so
    neither run sorts anything here; the two post-sorts are compared on
    probed rows in test_gpu_spgemm.py."""
    import os as _os
    from legate_sparse.gallery import rmat
    A = rmat(13, edge_factor=24, seed=3)
    C1 = A @ A
    _os.environ["LS_SPGEMM_SEGSORT"] = "0"
    try:
        # fresh A (cache keyed per matrix pair; avoid cache hits mixing)
        B = rmat(13, edge_factor=24, seed=3)
        C2 = B @ B
    finally:
        del _os.environ["LS_SPGEMM_SEGSORT"]
    assert C1._data.numel() == C2._data.numel()
    assert torch.equal(C1._indptr, C2._indptr)
    assert torch.equal(C1._indices, C2._indices)
    assert torch.allclose(C1._data, C2._data, rtol=1e-12)
    # rows are canonically sorted
    rid = torch.repeat_interleave(
        torch.arange(C1.shape[0], device=C1._data.device),
        C1._indptr[1:] - C1._indptr[:-1])
    key = rid * C1.shape[1] + C1._indices.long()
    assert bool((key[1:] > key[:-1]).all())


@pytest.mark.gpu
def test_io_roundtrip_on_gpu():
    """mmread/mmwrite/save_npz on the GPU box (device-resident csr)."""
    import tempfile, os as _os
    import scipy.io as sio
    import scipy.sparse as sp2
    S = sp2.random(60, 45, 0.2, format="csr", random_state=7)
    d = tempfile.mkdtemp()
    p = _os.path.join(d, "m.mtx")
    sio.mmwrite(p, S)
    A = lsp.mmread(p)
    assert A.data.is_cuda
    np.testing.assert_allclose(to_np(A.todense()), S.toarray())
    p2 = _os.path.join(d, "w.mtx")
    lsp.mmwrite(p2, A)
    back = sio.mmread(p2).tocsr()
    np.testing.assert_allclose(back.toarray(), S.toarray())
    p3 = _os.path.join(d, "c")
    lsp.save_npz(p3, A)
    B = lsp.load_npz(p3)
    assert B.data.is_cuda
    np.testing.assert_allclose(to_np(B.todense()), S.toarray())

# SPDX-License-Identifier: Apache-2.0
"""Tiled affine SpMV: full tiles (no indptr/mask loads), mixed tiles and
exception rows, against the general kernel and scipy on the host.

Every structural case asserts from the plan's tile table that it holds
the tile kinds it claims to exercise."""
import numpy as np
import pytest
import scipy.sparse as sp

import legate_sparse as lsp
from testutils import to_np

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

TOL64 = dict(rtol=1e-13, atol=1e-13)   # the existing fp64 affine tests'
TOL32 = dict(rtol=1e-5)                # test_affine_paths_fp32's


@pytest.fixture(scope="module", autouse=True)
def _check_native():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from legate_sparse import _cext
    _cext.require_hip()
    yield


def _tile():
    from legate_sparse import _cext
    return _cext.require_hip().AFFINE_TILE


def _banded(n, offs, seed, dtype=np.float64):
    rng = np.random.default_rng(seed)
    diags = []
    for o in offs:
        d = rng.random(n - abs(o)) + 0.5
        if np.dtype(dtype).kind == "c":
            d = d + 1j * rng.random(n - abs(o))
        diags.append(d.astype(dtype))
    return sp.diags(diags, list(offs), shape=(n, n), format="csr")


def _rand_x(n, dtype, seed):
    rng = np.random.default_rng(seed)
    x = rng.random(n)
    if np.dtype(dtype).kind == "c":
        x = x + 1j * rng.random(n)
    return x.astype(dtype)


def _tiles(plan):
    """(tile table as a list, indices of full tiles, of mixed tiles)."""
    tb = plan.tile_base.tolist()
    full = [t for t, b in enumerate(tb) if b >= 0]
    mixed = [t for t, b in enumerate(tb) if b < 0]
    return tb, full, mixed


def _check_table(A, plan):
    """The table against its definition, recomputed on the host."""
    T = _tile()
    ip = to_np(A._indptr)
    mask = to_np(plan[2])
    n = mask.size
    want = []
    for t in range((n + T - 1) // T):
        rows = mask[t * T:(t + 1) * T]
        want.append(int(ip[t * T]) if rows.size == T and rows.all() else -1)
    assert plan.tile_base.dtype == torch.int64
    assert plan.tile_base.tolist() == want


def _check_spmv(A, S, seed=7, tol=TOL64, idx64=False):
    """Affine path vs general path vs scipy; returns the plan."""
    from legate_sparse import ops as lops
    plan = A._affine_plan()
    assert plan is not None
    _check_table(A, plan)
    xh = _rand_x(S.shape[1], S.dtype, seed)
    x = torch.from_numpy(xh).cuda()
    ix = A._indices.long() if idx64 else A._indices
    y_aff = lops.spmv(A._indptr, ix, A._data, x, affine=plan)
    y_gen = lops.spmv(A._indptr, ix, A._data, x, affine=None)
    np.testing.assert_allclose(to_np(y_aff), to_np(y_gen), **tol)
    np.testing.assert_allclose(to_np(y_aff), S @ xh, **tol)
    return plan


def _poisson(nx, ny, seed):
    """Poisson structure with random values, so a wrong vals index shows
    (the gallery's coefficients are the same in every row)."""
    import legate_sparse.gallery as gal
    A = gal.poisson_2d(nx, ny)
    g = torch.Generator().manual_seed(seed)
    A._data.copy_((torch.rand(A._data.numel(), generator=g,
                              dtype=torch.float64) + 0.5).cuda())
    S = sp.csr_matrix((to_np(A._data), to_np(A._indices),
                       to_np(A._indptr)), shape=A.shape)
    return A, S


def test_tile_constant_is_one_wave():
    assert _tile() == 64


def test_tridiagonal_and_pentadiagonal_192_both_base_parities():
    bases = []
    # (-2..2) gives base 317 like the tridiagonal's odd 191; the wide
    # five-diagonal one gives the even base
    for offs in ((-1, 0, 1), (-2, -1, 0, 1, 2), (-3, -1, 0, 1, 3)):
        S = _banded(192, offs, seed=len(offs) + offs[0])
        A = lsp.csr_array(S)
        plan = _check_spmv(A, S)
        assert plan[0] == len(offs)
        tb, full, mixed = _tiles(plan)
        assert full == [1] and mixed == [0, 2]
        assert tb[1] == int(A._indptr[64])
        bases.append(tb[1])
    assert bases[0] == 191
    assert {b % 2 for b in bases} == {0, 1}


@pytest.mark.parametrize("n,full,mixed", [
    (64, [], [0]),                       # single tile, mixed
    (65, [], [0, 1]),                    # partial last tile of one row
    (1000, list(range(1, 15)), [0, 15]),  # 15*64 + 40: partial last tile
    (256, [1, 2], [0, 3]),               # exact multiple
])
def test_tile_edges(n, full, mixed):
    S = _banded(n, (-1, 0, 1), seed=n)
    A = lsp.csr_array(S)
    plan = _check_spmv(A, S)
    _, got_full, got_mixed = _tiles(plan)
    assert got_full == full and got_mixed == mixed


def test_poisson_long_fast_axis_has_full_and_mixed_tiles():
    A, S = _poisson(200, 9, seed=1)
    plan = _check_spmv(A, S)
    assert plan[0] == 5
    _, full, mixed = _tiles(plan)
    assert full and mixed


def test_poisson_short_fast_axis_has_no_full_tile():
    A, S = _poisson(9, 200, seed=2)
    plan = _check_spmv(A, S)
    assert plan[0] == 5
    _, full, mixed = _tiles(plan)
    assert not full and mixed


def test_exception_rows_inside_full_tiles():
    n = 640
    C = _banded(n, range(-5, 6), seed=11).tocoo()
    row, col, val = C.row.copy(), C.col.copy(), C.data.copy()
    # row 100 loses an entry: short row
    keep = ~((row == 100) & (col == 102))
    row, col, val = row[keep], col[keep], val[keep]
    # row 300 keeps 11 entries but one column moves: only the mask tells
    col[(row == 300) & (col == 305)] = 310
    S = sp.csr_matrix((val, (row, col)), shape=(n, n))
    S.sort_indices()
    A = lsp.csr_array(S)
    plan = _check_spmv(A, S)
    nd, _, mask, rest, _ = plan
    assert nd == 11
    cnt = (A._indptr[1:] - A._indptr[:-1]).tolist()
    assert cnt[100] == 10 and cnt[300] == 11
    assert int(mask[100]) == 0 and int(mask[300]) == 0
    assert {100, 300} <= set(rest.tolist())
    _, full, mixed = _tiles(plan)
    assert mixed == [0, 1, 4, 9]          # 100 // 64 == 1, 300 // 64 == 4
    assert full == [2, 3, 5, 6, 7, 8]
    # same with a 64-bit index stream under the exception rows
    _check_spmv(A, S, idx64=True)


def test_nd1_diagonal():
    S = _banded(128, (0,), seed=21)
    A = lsp.csr_array(S)
    plan = _check_spmv(A, S)
    assert plan[0] == 1
    tb, full, mixed = _tiles(plan)
    assert tb == [0, 64] and not mixed


def test_nd16():
    S = _banded(640, range(-8, 8), seed=22)
    A = lsp.csr_array(S)
    plan = _check_spmv(A, S)
    assert plan[0] == 16
    _, full, mixed = _tiles(plan)
    assert mixed == [0, 9] and full == list(range(1, 9))


@pytest.mark.parametrize("dtype,tol", [(np.float32, TOL32),
                                       (np.complex128, TOL64)])
def test_value_dtypes(dtype, tol):
    S = _banded(1000, (-2, -1, 0, 1, 2), seed=31, dtype=dtype)
    A = lsp.csr_array(S, dtype=dtype)
    assert A.dtype == dtype
    plan = _check_spmv(A, S, tol=tol)
    _, full, mixed = _tiles(plan)
    assert full and mixed


def test_accumulate():
    from legate_sparse import ops as lops
    A, S = _poisson(200, 9, seed=3)
    plan = A._affine_plan()
    _, full, mixed = _tiles(plan)
    assert full and mixed
    xh = _rand_x(S.shape[1], np.float64, 41)
    y0 = _rand_x(S.shape[0], np.float64, 42)
    y = torch.from_numpy(y0).cuda()
    lops.spmv(A._indptr, A._indices, A._data, torch.from_numpy(xh).cuda(),
              y, accumulate=True, affine=plan)
    np.testing.assert_allclose(to_np(y), y0 + S @ xh, **TOL64)


def test_interior_piece_with_nonzero_col_offset():
    """Rank 1 of a 2-rank split: local rows [cut, N), interior columns
    [cut, N) with GLOBAL ids, x the rank's own shard read through a
    base pointer shifted by cut."""
    from legate_sparse import ops as lops
    from legate_sparse.csr import _build_affine_plan
    A, S = _poisson(200, 20, seed=4)
    N = A.shape[0]
    cut = N // 2
    dev = A._data.device
    row_ids = torch.repeat_interleave(
        torch.arange(N, device=dev), A._indptr[1:] - A._indptr[:-1])
    m = (row_ids >= cut) & (A._indices.long() >= cut)
    cnt = torch.bincount(row_ids[m] - cut, minlength=N - cut)
    ip = torch.zeros(N - cut + 1, dtype=torch.int64, device=dev)
    torch.cumsum(cnt, dim=0, out=ip[1:])
    ix = A._indices[m].contiguous()
    dv = A._data[m].contiguous()
    plan = _build_affine_plan(ip, ix, max(A.shape))
    assert plan is not None and plan[0] == 5
    _, full, mixed = _tiles(plan)
    assert full and mixed
    xh = _rand_x(N, np.float64, 43)
    x_shard = torch.from_numpy(xh[cut:]).cuda()
    y_aff = lops.spmv(ip, ix, dv, x_shard, col_offset=cut, affine=plan)
    y_gen = lops.spmv(ip, ix, dv, x_shard, col_offset=cut, affine=None)
    np.testing.assert_allclose(to_np(y_aff), to_np(y_gen), **TOL64)
    np.testing.assert_allclose(to_np(y_aff), S[cut:, cut:] @ xh[cut:],
                               **TOL64)


@pytest.mark.parametrize("nx,any_full", [(64, False), (200, True)])
def test_fused_dot(nx, any_full):
    from legate_sparse import ops as lops
    A, S = _poisson(nx, nx, seed=5)
    _, full, mixed = _tiles(A._affine_plan())
    assert mixed and bool(full) == any_full
    p = torch.rand(A.shape[0], dtype=torch.float64, device="cuda")
    q = torch.empty_like(p)
    pq = torch.zeros(1, dtype=torch.float64, device="cuda")
    assert A._matvec_pq(p, q, pq)
    q_ref = lops.spmv(A._indptr, A._indices, A._data, p)
    assert torch.allclose(q, q_ref, **TOL64)
    np.testing.assert_allclose(to_np(q), S @ to_np(p), **TOL64)
    want = float(torch.dot(p, q_ref))
    assert abs(float(pq) - want) <= 1e-10 * abs(want)


def test_null_tile_table_switch_is_bit_identical(monkeypatch):
    from legate_sparse import ops as lops
    A, S = _poisson(200, 40, seed=6)
    plan = A._affine_plan()
    _, full, mixed = _tiles(plan)
    assert full and mixed
    x = torch.rand(A.shape[1], dtype=torch.float64, device="cuda")
    y_tiles = lops.spmv(A._indptr, A._indices, A._data, x, affine=plan)
    monkeypatch.setenv("LS_SPMV_AFFINE_TILES", "0")
    y_rows = lops.spmv(A._indptr, A._indices, A._data, x, affine=plan)
    assert torch.equal(y_tiles, y_rows)
    np.testing.assert_allclose(to_np(y_rows), S @ to_np(x), **TOL64)


def test_grid_stride_loop_is_bit_identical(monkeypatch):
    """A 2-block grid (8 waves) walks the 16 tiles of n = 1000 in two
    steps of the grid-stride loop; the default grid takes one."""
    from legate_sparse import ops as lops
    S = _banded(1000, (-2, -1, 0, 1, 2), seed=51)
    A = lsp.csr_array(S)
    plan = A._affine_plan()
    x = torch.rand(A.shape[1], dtype=torch.float64, device="cuda")
    y_one = lops.spmv(A._indptr, A._indices, A._data, x, affine=plan)
    monkeypatch.setenv("LS_SPMV_AFFINE_GRID", "2")
    y_loop = lops.spmv(A._indptr, A._indices, A._data, x, affine=plan)
    assert torch.equal(y_one, y_loop)
    np.testing.assert_allclose(to_np(y_loop), S @ to_np(x), **TOL64)

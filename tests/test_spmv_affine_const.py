# SPDX-License-Identifier: Apache-2.0
"""Constant-coefficient tiles of the affine SpMV: full tiles whose rows
all hold the same values (-2 in the value-bound table) read no value
stream.  Checked against scipy on the host, the general kernel, the same
call with LS_SPMV_AFFINE_CONST=0 (bit for bit) and the table's definition
recomputed on the host.

Every case asserts from the table that it holds the tile kinds it claims
to exercise: -2 (constant), >= 0 (full, values vary), -1 (mixed)."""
import numpy as np
import pytest
import scipy.sparse as sp

import legate_sparse as lsp
from testutils import to_np

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

TOL64 = dict(rtol=1e-13, atol=1e-13)   # the existing fp64 affine tests'
TOL32 = dict(rtol=1e-5)                # test_affine_paths_fp32's

CONST, FULL, MIXED = "const", "full", "mixed"


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


def _const_banded(n, offs, coeffs, dtype=np.float64):
    """Banded CSR whose diagonal at offs[k] holds coeffs[k] in every row
    (explicit zeros kept)."""
    offs = list(offs)
    S = sp.diags([np.ones(n - abs(o)) for o in offs], offs, shape=(n, n),
                 format="csr").astype(dtype)
    S.sort_indices()
    row = np.repeat(np.arange(n), np.diff(S.indptr))
    k = np.searchsorted(np.asarray(offs), S.indices - row)
    S.data[:] = np.asarray(coeffs, dtype=dtype)[k]
    return S


def _set(S, row, col, value):
    """Overwrite one stored entry of a scipy CSR (structure untouched)."""
    lo, hi = S.indptr[row], S.indptr[row + 1]
    j = lo + int(np.nonzero(S.indices[lo:hi] == col)[0][0])
    S.data[j] = value


def _scipy_of(A):
    return sp.csr_matrix((to_np(A._data), to_np(A._indices),
                          to_np(A._indptr)), shape=A.shape)


def _rand_x(n, dtype, seed):
    rng = np.random.default_rng(seed)
    x = rng.random(n)
    if np.dtype(dtype).kind == "c":
        x = x + 1j * rng.random(n)
    return x.astype(dtype)


def _host_table(plan, vals):
    """tile_cbase from its definition, bitwise: (table, C) or None when
    the plan has no full tile."""
    T, nd = _tile(), int(plan[0])
    tb = to_np(plan.tile_base)
    v = to_np(vals)
    vi = v.view({4: np.uint32, 8: np.uint64}[v.dtype.itemsize])
    full = np.nonzero(tb >= 0)[0]
    if not full.size:
        return None
    C = vi[tb[full[0]]:tb[full[0]] + nd]
    want = tb.copy()
    for t in full:
        rows = vi[tb[t]:tb[t] + T * nd].reshape(T, nd)
        if (rows == C).all():
            want[t] = -2
    return want, C


def _kinds(table):
    out = set()
    for b in table:
        out.add(CONST if b == -2 else FULL if b >= 0 else MIXED)
    return out


def _table_checked(plan, vals):
    """The native table of ``vals`` against the host's; returns it as a
    list (the plan's own table when there is no full tile) together with
    the _AffineConst a caller gets (None without a -2 tile)."""
    from legate_sparse.csr import _affine_const_table, _build_affine_const
    want = _host_table(plan, vals)
    got = _affine_const_table(plan, vals)
    cst = _build_affine_const(plan, vals)
    if want is None:
        assert got is None and cst is None
        return plan.tile_base.tolist(), None
    cb, C = got
    assert cb.dtype == torch.int64 and C.dtype == vals.dtype
    assert cb.tolist() == want[0].tolist()
    assert to_np(C).view(want[1].dtype).tolist() == want[1].tolist()
    if -2 in want[0]:
        assert cst is not None
        assert cst.tile_cbase.tolist() == want[0].tolist()
        assert cst.data_ptr == vals.data_ptr() and cst.plan is plan
    else:
        assert cst is None
    return cb.tolist(), cst


def _spmv3(monkeypatch, ip, ix, dv, x, plan, cst, **kw):
    """(constant-table run, LS_SPMV_AFFINE_CONST=0 run, general kernel)."""
    from legate_sparse import ops as lops

    def run(**more):
        args = dict(kw)
        if "y" in args:
            args["y"] = args["y"].clone()
        return lops.spmv(ip, ix, dv, x, **args, **more)

    y_c = run(affine=plan, affine_const=cst)
    monkeypatch.setenv("LS_SPMV_AFFINE_CONST", "0")
    y_0 = run(affine=plan, affine_const=cst)
    monkeypatch.delenv("LS_SPMV_AFFINE_CONST")
    y_gen = run(affine=None)
    return y_c, y_0, y_gen


def _check(monkeypatch, A, S, kinds, tol=TOL64, seed=7):
    """Table, tile kinds and the three result comparisons for a matrix
    through its cached accessor; returns (table list, _AffineConst)."""
    plan = A._affine_plan()
    assert plan is not None
    table, cst = _table_checked(plan, A._data)
    assert _kinds(table) == set(kinds)
    got = A._affine_const()
    assert (got is None) == (cst is None)
    if got is not None:
        assert got.tile_cbase.tolist() == table
        assert A._affine_const() is got          # cached
    xh = _rand_x(S.shape[1], S.dtype, seed)
    x = torch.from_numpy(xh).cuda()
    y_c, y_0, y_gen = _spmv3(monkeypatch, A._indptr, A._indices, A._data,
                             x, plan, got)
    assert torch.equal(y_c, y_0)
    np.testing.assert_allclose(to_np(y_c), to_np(y_gen), **tol)
    np.testing.assert_allclose(to_np(y_c), S @ xh, **tol)
    # the public entry point takes the same path
    y_pub = torch.empty_like(y_c)
    lsp.spmv(A, x, y_pub)
    assert torch.equal(y_pub, y_c)
    return table, got


TRI = ((-1, 0, 1), (-1.25, 2.5, -0.75))
# all positive: the fp32 case has no absolute tolerance to absorb
# cancellation
PENTA = ((-2, -1, 0, 1, 2), (0.5, 1.25, 3.0, 0.75, 0.25))


def test_constant_tridiagonal_192(monkeypatch):
    S = _const_banded(192, *TRI)
    table, cst = _check(monkeypatch, lsp.csr_array(S), S, {CONST, MIXED})
    assert table[1] == -2 and table[0] == -1 and table[2] == -1
    assert to_np(cst.C).tolist() == list(TRI[1])


def test_one_changed_value_leaves_no_constant_tile(monkeypatch):
    S = _const_banded(192, *TRI)
    _set(S, 100, 101, 9.0)
    A = lsp.csr_array(S)
    table, cst = _check(monkeypatch, A, S, {FULL, MIXED})
    assert table[1] == int(A._indptr[64]) and cst is None


def test_all_three_tile_kinds_in_one_launch(monkeypatch):
    S = _const_banded(320, *TRI)
    _set(S, 150, 150, 9.0)
    A = lsp.csr_array(S)
    table, cst = _check(monkeypatch, A, S, {CONST, FULL, MIXED})
    assert table == [-1, -2, int(A._indptr[128]), -2, -1]
    assert cst is not None


def test_sign_of_zero_is_a_different_value(monkeypatch):
    S = _const_banded(256, (-1, 0, 1), (1.0, 0.0, 1.0))
    _set(S, 150, 150, -0.0)
    A = lsp.csr_array(S)
    assert A._data.numel() == S.nnz      # explicit zeros kept
    d = to_np(A._data)[int(A._indptr[150]) + 1]
    assert d == 0.0 and np.signbit(d)
    table, _ = _check(monkeypatch, A, S, {CONST, FULL, MIXED})
    assert table == [-1, -2, int(A._indptr[128]), -1]


def test_poisson_gallery_values(monkeypatch):
    import legate_sparse.gallery as gal
    A = gal.poisson_2d(200, 9)
    table, cst = _check(monkeypatch, A, _scipy_of(A), {CONST, MIXED})
    assert to_np(cst.C).tolist() == [-1.0, -1.0, 4.0, -1.0, -1.0]


def test_poisson_short_fast_axis_has_no_table(monkeypatch):
    import legate_sparse.gallery as gal
    A = gal.poisson_2d(9, 200)
    _, cst = _check(monkeypatch, A, _scipy_of(A), {MIXED})
    assert cst is None


@pytest.mark.parametrize("n,kinds,n_const", [
    (1000, {CONST, MIXED}, 14),   # 15 * 64 + 40: partial last tile
    (256, {CONST, MIXED}, 2),     # exact multiple
    (64, {MIXED}, 0),             # single mixed tile: no table
])
def test_tile_edges(monkeypatch, n, kinds, n_const):
    S = _const_banded(n, *TRI)
    table, cst = _check(monkeypatch, lsp.csr_array(S), S, kinds)
    assert table.count(-2) == n_const
    assert table[0] == -1 and table[-1] == -1
    assert (cst is None) == (n_const == 0)


def test_nd1_diagonal(monkeypatch):
    S = _const_banded(128, (0,), (1.75,))
    table, _ = _check(monkeypatch, lsp.csr_array(S), S, {CONST})
    assert table == [-2, -2]


def test_nd16(monkeypatch):
    coeffs = [0.25 * (k - 7) + 0.125 for k in range(16)]
    S = _const_banded(640, range(-8, 8), coeffs)
    A = lsp.csr_array(S)
    table, _ = _check(monkeypatch, A, S, {CONST, MIXED})
    assert A._affine_plan()[0] == 16
    assert table == [-1] + [-2] * 8 + [-1]


def test_fp32(monkeypatch):
    S = _const_banded(1000, *PENTA, dtype=np.float32)
    A = lsp.csr_array(S, dtype=np.float32)
    assert A.dtype == np.float32
    table, cst = _check(monkeypatch, A, S, {CONST, MIXED}, tol=TOL32)
    assert cst.C.dtype == torch.float32 and table.count(-2) == 14


@pytest.mark.parametrize("nd", [1, 2, 3, 4, 8, 13])
def test_fp32_same_bits_across_nd(monkeypatch, nd):
    """The fp32 row sum is where the two kernels could part (see the
    kernel's header comment): every ND parity, and the last ND offered."""
    lo = -(nd // 2)
    coeffs = [0.5 + 0.37 * k for k in range(nd)]   # inexact products
    S = _const_banded(320, range(lo, lo + nd), coeffs, dtype=np.float32)
    A = lsp.csr_array(S, dtype=np.float32)
    assert A._affine_plan()[0] == nd
    kinds = {CONST} if nd == 1 else {CONST, MIXED}
    _check(monkeypatch, A, S, kinds, tol=TOL32)


def test_fp32_wide_stencil_gets_no_table(monkeypatch):
    from legate_sparse import _cext
    from legate_sparse.csr import _affine_const_table
    nd = _cext.require_hip().AFFINE_CONST_F32_ND + 1
    S = _const_banded(320, range(-7, nd - 7), [1.0 + k for k in range(nd)],
                      dtype=np.float32)
    A = lsp.csr_array(S, dtype=np.float32)
    plan = A._affine_plan()
    assert plan[0] == nd and int((plan.tile_base >= 0).sum()) == 3
    assert _affine_const_table(plan, A._data) is None
    assert A._affine_const() is None
    S64 = S.astype(np.float64)                     # fp64 has no such cap
    assert lsp.csr_array(S64)._affine_const() is not None


def test_complex128_gets_no_table(monkeypatch):
    """The constant-tile kernels are instantiated for real dtypes only:
    a complex matrix builds no table and runs what it ran before."""
    from legate_sparse import ops as lops
    from legate_sparse.csr import _affine_const_table
    S = _const_banded(1000, *PENTA, dtype=np.complex128)
    S.data[:] = S.data * (1.0 + 0.5j)
    A = lsp.csr_array(S, dtype=np.complex128)
    plan = A._affine_plan()
    assert plan is not None and int((plan.tile_base >= 0).sum()) == 14
    assert _affine_const_table(plan, A._data) is None
    assert A._affine_const() is None
    xh = _rand_x(1000, np.complex128, 8)
    x = torch.from_numpy(xh).cuda()
    y = torch.empty_like(x)
    lsp.spmv(A, x, y)
    y_aff = lops.spmv(A._indptr, A._indices, A._data, x, affine=plan)
    y_gen = lops.spmv(A._indptr, A._indices, A._data, x, affine=None)
    assert torch.equal(y, y_aff)
    np.testing.assert_allclose(to_np(y), to_np(y_gen), **TOL64)
    np.testing.assert_allclose(to_np(y), S @ xh, **TOL64)


def test_accumulate(monkeypatch):
    import legate_sparse.gallery as gal
    A = gal.poisson_2d(200, 9)
    S = _scipy_of(A)
    plan = A._affine_plan()
    table, cst = _table_checked(plan, A._data)
    assert _kinds(table) == {CONST, MIXED}
    xh = _rand_x(S.shape[1], np.float64, 41)
    y0 = _rand_x(S.shape[0], np.float64, 42)
    y_c, y_0, y_gen = _spmv3(
        monkeypatch, A._indptr, A._indices, A._data,
        torch.from_numpy(xh).cuda(), plan, cst,
        y=torch.from_numpy(y0).cuda(), accumulate=True)
    assert torch.equal(y_c, y_0)
    np.testing.assert_allclose(to_np(y_c), to_np(y_gen), **TOL64)
    np.testing.assert_allclose(to_np(y_c), y0 + S @ xh, **TOL64)


@pytest.mark.parametrize("nx,kinds", [(64, {MIXED}),
                                      (200, {CONST, MIXED})])
def test_fused_dot(monkeypatch, nx, kinds):
    import legate_sparse.gallery as gal
    from legate_sparse import ops as lops
    A = gal.poisson_2d(nx, nx)
    S = _scipy_of(A)
    table, _ = _table_checked(A._affine_plan(), A._data)
    assert _kinds(table) == kinds
    assert (A._affine_const() is not None) == (CONST in kinds)
    p = torch.rand(A.shape[0], dtype=torch.float64, device="cuda")

    def run():
        q = torch.empty_like(p)
        pq = torch.zeros(1, dtype=torch.float64, device="cuda")
        assert A._matvec_pq(p, q, pq)
        return q, float(pq)

    q, pq = run()
    monkeypatch.setenv("LS_SPMV_AFFINE_CONST", "0")
    q_0, pq_0 = run()
    monkeypatch.delenv("LS_SPMV_AFFINE_CONST")
    assert torch.equal(q, q_0)
    q_ref = lops.spmv(A._indptr, A._indices, A._data, p)
    np.testing.assert_allclose(to_np(q), to_np(q_ref), **TOL64)
    np.testing.assert_allclose(to_np(q), S @ to_np(p), **TOL64)
    want = float(torch.dot(p, q_ref))
    assert abs(pq - want) <= 1e-10 * abs(want)
    assert abs(pq_0 - want) <= 1e-10 * abs(want)


def test_grid_stride_loop_is_bit_identical(monkeypatch):
    """A 2-block grid (8 waves) walks the 16 tiles of n = 1000 in two
    steps of the grid-stride loop; the default grid takes one."""
    from legate_sparse import ops as lops
    S = _const_banded(1000, *PENTA)
    A = lsp.csr_array(S)
    plan = A._affine_plan()
    table, cst = _table_checked(plan, A._data)
    assert _kinds(table) == {CONST, MIXED} and table.count(-2) == 14
    x = torch.rand(A.shape[1], dtype=torch.float64, device="cuda")
    y_one = lops.spmv(A._indptr, A._indices, A._data, x, affine=plan,
                      affine_const=cst)
    monkeypatch.setenv("LS_SPMV_AFFINE_GRID", "2")
    y_loop = lops.spmv(A._indptr, A._indices, A._data, x, affine=plan,
                       affine_const=cst)
    assert torch.equal(y_one, y_loop)
    np.testing.assert_allclose(to_np(y_loop), S @ to_np(x), **TOL64)


def test_interior_piece_with_nonzero_col_offset(monkeypatch):
    """Rank 1 of a 2-rank split: local rows [cut, N), interior columns
    [cut, N) with GLOBAL ids, x the rank's own shard read through a
    base pointer shifted by cut; the table is keyed to the piece's own
    values, as _split_for_overlap builds it."""
    import legate_sparse.gallery as gal
    from legate_sparse.csr import _build_affine_plan
    A = gal.poisson_2d(200, 20)
    S = _scipy_of(A)
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
    table, cst = _table_checked(plan, dv)
    assert _kinds(table) == {CONST, MIXED}
    xh = _rand_x(N, np.float64, 43)
    x_shard = torch.from_numpy(xh[cut:]).cuda()
    y_c, y_0, y_gen = _spmv3(monkeypatch, ip, ix, dv, x_shard, plan, cst,
                             col_offset=cut)
    assert torch.equal(y_c, y_0)
    np.testing.assert_allclose(to_np(y_c), to_np(y_gen), **TOL64)
    np.testing.assert_allclose(to_np(y_c), S[cut:, cut:] @ xh[cut:],
                               **TOL64)


def _poisson_with_table():
    import legate_sparse.gallery as gal
    A = gal.poisson_2d(200, 9)
    cst = A._affine_const()
    assert cst is not None and -2 in cst.tile_cbase.tolist()
    xh = _rand_x(A.shape[1], np.float64, 61)
    x = torch.from_numpy(xh).cuda()
    y = torch.empty_like(x)
    lsp.spmv(A, x, y)
    np.testing.assert_allclose(to_np(y), _scipy_of(A) @ xh, **TOL64)
    return A, cst, xh, x, y


def _spmv_vs_scipy(A, xh, x):
    y = torch.empty_like(x)
    lsp.spmv(A, x, y)
    np.testing.assert_allclose(to_np(y), _scipy_of(A) @ xh, **TOL64)
    return y


def test_invalidation_inplace_scale():
    A, cst, xh, x, y = _poisson_with_table()
    A.data.mul_(2.0)
    y2 = _spmv_vs_scipy(A, xh, x)
    assert torch.equal(y2, 2.0 * y)              # exact in fp64
    new = A._affine_const()
    assert new is not None and new is not cst
    assert to_np(new.C).tolist() == [-2.0, -2.0, 8.0, -2.0, -2.0]
    assert new.tile_cbase.tolist() == cst.tile_cbase.tolist()
    assert new.version == A.data._version != cst.version


def test_invalidation_single_entry():
    """Row 300, not row 100: the first 200 rows of poisson_2d(200, 9)
    are the y = 0 grid line, four entries each, so tile 100 // 64 is
    mixed from the start.  Row 300 (x = 100 of the second line) lies in
    a constant tile."""
    A, cst, xh, x, _ = _poisson_with_table()
    row = 300
    t = row // _tile()
    assert cst.tile_cbase[t] == -2
    A.data[A.indptr[row] + 2] = 7.0
    _spmv_vs_scipy(A, xh, x)
    new = A._affine_const()
    assert new is not None and new is not cst
    want = _host_table(A._affine_plan(), A._data)[0]
    assert new.tile_cbase.tolist() == want.tolist()
    assert new.tile_cbase[t] >= 0 and -2 in new.tile_cbase.tolist()


def test_invalidation_data_setter():
    A, _, xh, x, _ = _poisson_with_table()
    g = torch.Generator().manual_seed(9)
    A.data = (torch.rand(A.nnz, generator=g, dtype=torch.float64)
              + 0.5).cuda()
    _spmv_vs_scipy(A, xh, x)
    assert A._affine_const() is None


def test_invalidation_copy_into_data():
    A, cst, xh, x, _ = _poisson_with_table()
    g = torch.Generator().manual_seed(10)
    A._data.copy_((torch.rand(A.nnz, generator=g, dtype=torch.float64)
                   + 0.5).cuda())
    _spmv_vs_scipy(A, xh, x)
    assert A._affine_const() is None
    assert A._affine_plan() is cst.plan          # structure untouched


def test_second_invalidation_stops_detection():
    from legate_sparse.csr import _CONST_MAX_INVALIDATIONS
    assert _CONST_MAX_INVALIDATIONS == 2
    A, cst, xh, x, y = _poisson_with_table()
    A.data.mul_(2.0)
    assert A._affine_const() is not None         # first: rebuilt
    A.data.mul_(0.5)                             # constant again, but
    y2 = _spmv_vs_scipy(A, xh, x)                # second: stop scanning
    assert A._affine_const() is None
    assert torch.equal(y2, y)
    A.data.mul_(3.0)
    _spmv_vs_scipy(A, xh, x)
    assert A._affine_const() is None


def test_table_of_other_values_is_ignored():
    from legate_sparse import ops as lops
    A, cst, xh, x, _ = _poisson_with_table()
    g = torch.Generator().manual_seed(11)
    other = (torch.rand(A.nnz, generator=g, dtype=torch.float64)
             + 0.5).cuda()
    assert other.data_ptr() != cst.data_ptr
    y = lops.spmv(A._indptr, A._indices, other, x,
                  affine=A._affine_plan(), affine_const=cst)
    S = sp.csr_matrix((to_np(other), to_np(A._indices), to_np(A._indptr)),
                      shape=A.shape)
    np.testing.assert_allclose(to_np(y), S @ xh, **TOL64)


def test_stale_version_is_ignored_by_ops():
    """A direct caller who writes into vals and hands the old table on
    gets the new values, not the recorded pattern."""
    from legate_sparse import ops as lops
    A, cst, xh, x, _ = _poisson_with_table()
    A._data.mul_(3.0)
    assert cst.data_ptr == A._data.data_ptr()
    assert cst.version != A._data._version
    y = lops.spmv(A._indptr, A._indices, A._data, x,
                  affine=A._affine_plan(), affine_const=cst)
    np.testing.assert_allclose(to_np(y), _scipy_of(A) @ xh, **TOL64)


def test_new_plans_do_not_count_as_invalidations():
    from legate_sparse.csr import _CONST_MAX_INVALIDATIONS
    A, cst, xh, x, y = _poisson_with_table()
    for _ in range(_CONST_MAX_INVALIDATIONS + 1):
        A.indices = A.indices.clone()            # same structure, new plan
        new = A._affine_const()
        assert new is not None and new.plan is A._affine_plan()
        assert new.plan is not cst.plan
        assert new.tile_cbase.tolist() == cst.tile_cbase.tolist()
    assert torch.equal(_spmv_vs_scipy(A, xh, x), y)

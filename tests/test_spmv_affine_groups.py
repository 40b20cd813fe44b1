# SPDX-License-Identifier: Apache-2.0
"""Tile groups of the constant-tile affine SpMV: a wave takes
G = affine_group(nd, dtype) consecutive tiles and issues the x loads of
all its -2 tiles before the first sum; the exception rows ride in the
same launch.

Every case runs the default path against LS_SPMV_AFFINE_GROUP=1 (the
one-tile-per-wave kernel) and LS_SPMV_AFFINE_CONST=0 (no table) bit for bit, and against
scipy on the host at the tolerances of the existing affine tests, and
asserts from the table that it holds the tile kinds it claims."""
import numpy as np
import pytest
import scipy.sparse as sp

import legate_sparse as lsp
from testutils import to_np

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

TOL64 = dict(rtol=1e-13, atol=1e-13)   # the existing fp64 affine tests'
TOL32 = dict(rtol=1e-5)                # test_affine_paths_fp32's

TRI = ((-1, 0, 1), (-1.25, 2.5, -0.75))
# all positive: the fp32 cases have no absolute tolerance to absorb
# cancellation
PENTA = ((-2, -1, 0, 1, 2), (0.5, 1.25, 3.0, 0.75, 0.25))


@pytest.fixture(scope="module", autouse=True)
def _check_native():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from legate_sparse import _cext
    _cext.require_hip()
    yield


def _ext():
    from legate_sparse import _cext
    return _cext.require_hip()


def _tile():
    return _ext().AFFINE_TILE


def _group(nd, dtype=np.float64):
    g = _ext().affine_group(int(nd), 0 if np.dtype(dtype) == np.float32
                            else 1)
    assert g >= 1 and g & (g - 1) == 0
    return g


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


def _rand(n, dtype, seed):
    return np.random.default_rng(seed).random(n).astype(dtype)


def _table(A):
    """(table as a list, _AffineConst or None): the value-bound table, or
    the plan's own where no tile is constant."""
    plan = A._affine_plan()
    assert plan is not None
    cst = A._affine_const()
    if cst is None:
        return plan.tile_base.tolist(), None
    assert cst.plan is plan
    return cst.tile_cbase.tolist(), cst


def _ends_mixed_rest_const(table):
    return (table[0] == -1 and table[-1] == -1
            and all(b == -2 for b in table[1:-1]))


def _with_env(monkeypatch, name, value, fn):
    monkeypatch.setenv(name, value)
    try:
        return fn()
    finally:
        monkeypatch.delenv(name)


def _three(monkeypatch, run):
    """run() by default, with one tile per wave and without the table:
    the last two must match the first bit for bit."""
    y = run()
    y_g1 = _with_env(monkeypatch, "LS_SPMV_AFFINE_GROUP", "1", run)
    y_c0 = _with_env(monkeypatch, "LS_SPMV_AFFINE_CONST", "0", run)
    assert torch.equal(y, y_g1)
    assert torch.equal(y, y_c0)
    return y


def _spmv_checked(monkeypatch, A, S, xh, tol=TOL64, y0=None, **kw):
    """The three runs of ops.spmv on A with its plan and table, then
    scipy; y0 given: accumulate into a copy of it."""
    from legate_sparse import ops as lops
    plan = A._affine_plan()
    cst = A._affine_const()
    x = torch.from_numpy(xh).cuda()

    def run():
        if y0 is None:
            return lops.spmv(A._indptr, A._indices, A._data, x,
                             affine=plan, affine_const=cst, **kw)
        return lops.spmv(A._indptr, A._indices, A._data, x,
                         y=torch.from_numpy(y0).cuda(), accumulate=True,
                         affine=plan, affine_const=cst, **kw)

    y = _three(monkeypatch, run)
    want = S @ xh if y0 is None else y0 + S @ xh
    np.testing.assert_allclose(to_np(y), want, **tol)
    return y


# 1. constant groups and tails ------------------------------------------
@pytest.mark.parametrize("band", [TRI, PENTA], ids=["tri", "penta"])
@pytest.mark.parametrize("which", range(4))
def test_constant_groups_and_tails(monkeypatch, band, which):
    """Whole constant groups, a first and a last group with one mixed
    tile each, a partial last group, a partial last tile, and fewer
    tiles than a group holds."""
    T, G = _tile(), _group(len(band[0]))
    n = [T * (3 * G + 2), T * (3 * G + 2) + 40, T * G - 1, T * 2][which]
    S = _const_banded(n, *band)
    A = lsp.csr_array(S)
    table, cst = _table(A)
    assert len(table) == -(-n // T)
    if len(table) > 2:
        assert _ends_mixed_rest_const(table) and cst is not None
    else:
        assert table == [-1, -1] and cst is None
    _spmv_checked(monkeypatch, A, S, _rand(n, np.float64, 70 + which))


def test_fewer_tiles_than_a_group(monkeypatch):
    """An nd = 1 diagonal is constant in every whole tile, so two or three
    tiles make one partial group inside the group kernel; 40 rows less
    leave a partial, mixed last tile in it."""
    T, G = _tile(), _group(1)
    assert G > 3
    for i, n in enumerate([T * 2, T * 3, T * 3 - 40]):
        S = _const_banded(n, (0,), (1.75,))
        A = lsp.csr_array(S)
        table, cst = _table(A)
        assert cst is not None
        assert table == [-2] * (n // T) + [-1] * (1 if n % T else 0)
        _spmv_checked(monkeypatch, A, S, _rand(n, np.float64, 75 + i))
        _spmv_checked(monkeypatch, A, S, _rand(n, np.float64, 75 + i),
                      y0=_rand(n, np.float64, 78 + i))


# 2. one varying tile per position of the group -------------------------
def test_one_varying_tile_per_position(monkeypatch):
    """Tile G + k turns full-varying for each position k of a group while
    its group neighbours stay constant."""
    T, G = _tile(), _group(5)
    n = T * (3 * G + 2)
    for k in range(G):
        S = _const_banded(n, *PENTA)
        row = (G + k) * T + 5
        _set(S, row, row, 9.0)
        A = lsp.csr_array(S)
        table, cst = _table(A)
        want = [-1] + [-2] * (3 * G) + [-1]
        want[G + k] = int(A._indptr[(G + k) * T])
        assert table == want and cst is not None
        _spmv_checked(monkeypatch, A, S, _rand(n, np.float64, 80 + k))


# 3. Poisson seam --------------------------------------------------------
@pytest.mark.parametrize("nx", ["TG", 200])
@pytest.mark.parametrize("accumulate", [False, True])
def test_poisson_seam(monkeypatch, nx, accumulate):
    """Two adjacent mixed tiles at every grid-line seam, inside groups
    that also hold constant tiles."""
    import legate_sparse.gallery as gal
    T, G = _tile(), _group(5)
    nx = T * G if nx == "TG" else nx
    A = gal.poisson_2d(nx, 9)
    S = _scipy_of(A)
    table, cst = _table(A)
    assert cst is not None and set(table) == {-1, -2}
    seams = [t for t in range(len(table) - 1)
             if table[t] == -1 and table[t + 1] == -1]
    assert seams
    groups = [table[g:g + G] for g in range(0, len(table), G)]
    assert any(-1 in g and -2 in g for g in groups)
    n = A.shape[0]
    _spmv_checked(monkeypatch, A, S, _rand(n, np.float64, 90),
                  y0=_rand(n, np.float64, 91) if accumulate else None)


# 4. grid-stride loop over groups -----------------------------------------
def test_grid_stride_loop_over_groups(monkeypatch):
    """A 2-block grid (8 waves) takes 8 groups a step: more than two
    steps here, and the same bits as the default grid's single step."""
    T, G = _tile(), _group(5)
    n = T * G * 8 * 3 + 40
    S = _const_banded(n, *PENTA)
    A = lsp.csr_array(S)
    table, cst = _table(A)
    assert _ends_mixed_rest_const(table) and len(table) > 2 * 8 * G
    xh = _rand(n, np.float64, 100)
    y_one = _spmv_checked(monkeypatch, A, S, xh)
    monkeypatch.setenv("LS_SPMV_AFFINE_GRID", "2")
    y_loop = _spmv_checked(monkeypatch, A, S, xh)
    assert torch.equal(y_one, y_loop)


# 5. fp32 ------------------------------------------------------------------
@pytest.mark.parametrize("nd", [1, 2, 3, 4, 8, 13])
def test_fp32_same_bits_across_nd(monkeypatch, nd):
    """The same-bits contract of the constant-tile fp32 kernels, now
    across the group path."""
    T, G = _tile(), _group(nd, np.float32)
    n = T * (2 * G + 2)
    lo = -(nd // 2)
    coeffs = [0.5 + 0.37 * k for k in range(nd)]   # inexact products
    S = _const_banded(n, range(lo, lo + nd), coeffs, dtype=np.float32)
    A = lsp.csr_array(S, dtype=np.float32)
    assert A._affine_plan()[0] == nd
    table, cst = _table(A)
    assert cst is not None
    if nd == 1:
        assert table == [-2] * (2 * G + 2)
    else:
        # nd = 2 has no upper diagonal: its last tile is constant too
        assert table[0] == -1 and set(table[1:-1]) == {-2}
        assert table[-1] == (-2 if nd == 2 else -1)
    _spmv_checked(monkeypatch, A, S, _rand(n, np.float32, 110 + nd),
                  tol=TOL32)


# 6. wide stencil ------------------------------------------------------------
def test_nd16_fp64(monkeypatch):
    T, G = _tile(), _group(16)
    n = T * (2 * G + 2)
    coeffs = [0.25 * (k - 7) + 0.125 for k in range(16)]
    S = _const_banded(n, range(-8, 8), coeffs)
    A = lsp.csr_array(S)
    assert A._affine_plan()[0] == 16
    table, cst = _table(A)
    assert _ends_mixed_rest_const(table) and cst is not None
    _spmv_checked(monkeypatch, A, S, _rand(n, np.float64, 120))


# 7. shifted x pointer, y off the 16-B grid ------------------------------------
@pytest.mark.parametrize("odd", [0, 1], ids=["even_cut", "odd_cut"])
def test_interior_piece_shifted_x_and_y(monkeypatch, odd):
    """Rank 1 of a 2-rank split (see test_spmv_affine_const): x is read
    through a base pointer shifted by an even and by an odd number of
    entries, and y starts 8 bytes off a 16-byte boundary."""
    import legate_sparse.gallery as gal
    from legate_sparse import ops as lops
    from legate_sparse.csr import _build_affine_plan, _build_affine_const
    A = gal.poisson_2d(200, 20)
    S = _scipy_of(A)
    N = A.shape[0]
    cut = N // 2 + odd
    assert cut % 2 == odd
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
    cst = _build_affine_const(plan, dv)
    assert cst is not None and set(cst.tile_cbase.tolist()) == {-1, -2}
    xh = _rand(N, np.float64, 130 + odd)
    x_shard = torch.from_numpy(xh[cut:]).cuda()
    assert x_shard.data_ptr() % 16 == 0

    def run():
        y = torch.empty(N - cut + 1, dtype=torch.float64, device=dev)[1:]
        assert y.data_ptr() % 16 == 8
        return lops.spmv(ip, ix, dv, x_shard, y=y, affine=plan,
                         affine_const=cst, col_offset=cut)

    y = _three(monkeypatch, run)
    np.testing.assert_allclose(to_np(y), S[cut:, cut:] @ xh[cut:], **TOL64)


# 8. fused dot ---------------------------------------------------------------------
def test_fused_dot(monkeypatch):
    """The fused dot keeps the one-tile kernel: q keeps its bits and pq
    stays within the existing 1e-10."""
    import legate_sparse.gallery as gal
    from legate_sparse import ops as lops
    A = gal.poisson_2d(200, 200)
    S = _scipy_of(A)
    table, cst = _table(A)
    assert cst is not None and set(table) == {-1, -2}
    p = torch.rand(A.shape[0], dtype=torch.float64, device="cuda")
    pqs = []

    def run():
        q = torch.empty_like(p)
        pq = torch.zeros(1, dtype=torch.float64, device="cuda")
        assert A._matvec_pq(p, q, pq)
        pqs.append(float(pq))
        return q

    q = _three(monkeypatch, run)
    q_ref = lops.spmv(A._indptr, A._indices, A._data, p)
    np.testing.assert_allclose(to_np(q), to_np(q_ref), **TOL64)
    np.testing.assert_allclose(to_np(q), S @ to_np(p), **TOL64)
    want = float(torch.dot(p, q_ref))
    assert len(pqs) == 3
    for pq in pqs:
        assert abs(pq - want) <= 1e-10 * abs(want)


# 9. exception rows inside the launch --------------------------------------------------
@pytest.mark.parametrize("case", ["diagonal", "banded", "poisson"])
@pytest.mark.parametrize("accumulate", [False, True])
def test_fold_is_bit_identical(monkeypatch, case, accumulate):
    """LS_SPMV_AFFINE_FOLD=0 (exception rows in a launch of their own)
    against the default: no exception rows, exception rows at both ends
    only, exception rows throughout."""
    import legate_sparse.gallery as gal
    T = _tile()
    if case == "diagonal":
        n = T * 2 * _group(1)
        S = _const_banded(n, (0,), (1.75,))
        A = lsp.csr_array(S)
        n_rest = 0
    elif case == "banded":
        n = T * (3 * _group(5) + 2) + 40
        S = _const_banded(n, *PENTA)
        A = lsp.csr_array(S)
        n_rest = 4
    else:
        A = gal.poisson_2d(200, 9)
        S = _scipy_of(A)
        n_rest = None
    table, cst = _table(A)
    assert cst is not None and -2 in table
    rest = A._affine_plan()[3]
    if n_rest is None:
        # both ends of every grid line and the whole first and last line
        assert rest.numel() >= 2 * 9 + 2 * 200 - 4
        r = to_np(rest)
        assert r.min() == 0 and r.max() == A.shape[0] - 1
        assert ((r > 400) & (r < A.shape[0] - 400)).any()
    else:
        assert rest.numel() == n_rest
        if n_rest:
            assert sorted(to_np(rest).tolist()) == [0, 1, n - 2, n - 1]
    assert int((to_np(A._affine_plan()[2]) == 0).sum()) == rest.numel()
    n = A.shape[0]
    xh = _rand(n, np.float64, 140)
    y0 = _rand(n, np.float64, 141) if accumulate else None
    y = _spmv_checked(monkeypatch, A, S, xh, y0=y0)
    monkeypatch.setenv("LS_SPMV_AFFINE_FOLD", "0")
    y_sep = _spmv_checked(monkeypatch, A, S, xh, y0=y0)
    assert torch.equal(y, y_sep)

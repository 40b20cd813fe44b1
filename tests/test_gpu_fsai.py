# SPDX-License-Identifier: Apache-2.0
"""GPU numerics of the FSAI setup kernel (src/hip/fsai.hip) and of
linalg.fsai on top of it: values against the per-row numpy reference on
both sub-wave widths and both index dtypes, a sliced window, launch-shape
overrides, run-to-run identity, the pivot flag, the apply and a
preconditioned solve (pytest -m gpu on an MI355X)."""
import numpy as np
import pytest
import scipy.sparse as sp

import legate_sparse as lsp
from legate_sparse import linalg, ops
from testutils import to_np
import fsai_cases as fc

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

I32_MAX = 2 ** 31 - 1


@pytest.fixture(scope="module", autouse=True)
def _check_native():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from legate_sparse import _cext
    # GPU runs MUST use the gfx950 extension — no silent fallback
    ext = _cext.require_hip()
    assert ext.FSAI_MAX_ROW == ops.FSAI_MAX_ROW == fc.MAX_ROW
    assert ext.FSAI_NARROW == ops.FSAI_NARROW == 8
    assert ext.FSAI_GRID_CAP == ops.FSAI_GRID_CAP
    yield


def _raw(A, P, idx_dtype=torch.int32, max_row=None, **kw):
    """ops.fsai_rows straight on device arrays -> (values, flag)."""
    cv = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a)).to(dt).cuda()
    flag = torch.empty(1, dtype=torch.int32, device="cuda")
    if max_row is None:
        max_row = int(np.diff(P.indptr).max())
    vals = ops.fsai_rows(
        cv(P.indptr, torch.int64), cv(P.indices, idx_dtype),
        cv(A.indptr, torch.int64), cv(A.indices, idx_dtype),
        torch.from_numpy(A.data.copy()).cuda(), 0, 0, flag, max_row, **kw)
    return vals, flag


def _build(name, p, dtype):
    A = lsp.csr_array(fc.matrix(name, dtype))
    pat = lsp.csr_array(fc.pattern(name, p)) if p == "given" else p
    return linalg.fsai(A, pat)


@pytest.mark.parametrize("name,p,dtype", fc.VALUE_CASES)
def test_gpu_fsai_values(name, p, dtype):
    P, want = fc.reference(name, p, dtype)
    M = _build(name, p, dtype)
    assert M.G.data.is_cuda and M.GH.data.is_cuda
    assert np.array_equal(to_np(M.G.indptr), P.indptr)
    assert np.array_equal(to_np(M.G.indices), P.indices)
    got = to_np(M.G.data)
    print(f"{name} p={p} {np.dtype(dtype).name}: longest row "
          f"{np.diff(P.indptr).max()}, max |G - ref| "
          f"{np.abs(got - want).max():.3e}")
    np.testing.assert_allclose(got, want, **fc.tol(dtype))
    d = fc.as_scipy(M.G).diagonal()
    assert np.all(d.real > 0) and np.all(d.imag == 0)
    for idt in (torch.int32, torch.int64):
        vals, flag = _raw(fc.matrix(name, dtype), P, idt)
        np.testing.assert_allclose(to_np(vals), want, **fc.tol(dtype))
        assert int(flag.item()) == I32_MAX


@pytest.mark.parametrize("idt", [torch.int32, torch.int64])
def test_gpu_fsai_sliced_window(idt):
    """Local rows [lo, hi) against a window of A that starts at the
    smallest pattern column (row_offset != 0): the distributed call shape
    at world size 1."""
    name, p = "grid9x8x7", 2
    A = fc.matrix(name)
    P, want = fc.reference(name, p, np.float64)
    lo, hi = 200, 330
    w0 = int(P.indices[P.indptr[lo]:P.indptr[hi]].min())
    assert 0 < w0 < lo
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a)).to(dt).cuda()
    flag = torch.empty(1, dtype=torch.int32, device="cuda")
    vals = ops.fsai_rows(
        t(P.indptr[lo:hi + 1] - P.indptr[lo], torch.int64),
        t(P.indices[P.indptr[lo]:P.indptr[hi]], idt),
        t(A.indptr[w0:hi + 1] - A.indptr[w0], torch.int64),
        t(A.indices[A.indptr[w0]:A.indptr[hi]], idt),
        t(A.data[A.indptr[w0]:A.indptr[hi]], torch.float64), w0, lo, flag,
        13)
    np.testing.assert_allclose(to_np(vals),
                               want[P.indptr[lo]:P.indptr[hi]],
                               **fc.tol(np.float64))
    assert int(flag.item()) == I32_MAX


@pytest.mark.parametrize("name,p", [("grid33x17", 1), ("band8", "given"),
                                    ("grid9x8x7", 1)])
def test_gpu_fsai_launch_shapes(name, p):
    """An 8-lane case through the 32-lane kernel, the torch arm and a
    one-workgroup grid."""
    A = fc.matrix(name)
    P, want = fc.reference(name, p, np.float64)
    assert np.diff(P.indptr).max() <= ops.FSAI_NARROW
    base, _ = _raw(A, P)
    np.testing.assert_allclose(to_np(base), want, **fc.tol(np.float64))
    for kw in (dict(max_row=32), dict(_impl="torch"), dict(_grid_cap=1),
               dict(max_row=9, _grid_cap=1)):
        vals, flag = _raw(A, P, **kw)
        print(f"{name} {kw}: bit-equal to the default launch: "
              f"{torch.equal(vals, base)}")
        np.testing.assert_allclose(to_np(vals), want, **fc.tol(np.float64))
        if "_impl" not in kw:
            # a row's arithmetic and its order depend neither on the
            # sub-wave width nor on the grid
            assert torch.equal(vals, base)
        assert int(flag.item()) == I32_MAX
    with pytest.raises(ValueError):
        _raw(A, P, _grid_cap=ops.FSAI_GRID_CAP + 1)


def test_gpu_fsai_bit_identical():
    for name, p in (("rand300", 1), ("grid9x8x7", 3), ("grid33x17", 1)):
        A, P = fc.matrix(name, np.float32), fc.pattern(name, p)
        assert torch.equal(_raw(A, P)[0], _raw(A, P)[0])
    a = _build("herm300", 1, np.complex128)
    b = _build("herm300", 1, np.complex128)
    assert torch.equal(a.G.data, b.G.data)
    assert torch.equal(a.GH.data, b.GH.data)


def test_gpu_fsai_pivot_flag_and_errors():
    """Indefinite input is an error return, not a trap: the flag names the
    smallest bad row and the device stays usable."""
    for S, row in ((fc.indefinite_diag(7), 7), (fc.indefinite_block(11), 11)):
        _, flag = _raw(S, sp.csr_array(sp.tril(S, 0)))
        assert int(flag.item()) == row
        with pytest.raises(RuntimeError,
                           match=rf"not positive definite at row {row}\b"):
            linalg.fsai(lsp.csr_array(S))
    # still usable
    P, want = fc.reference("grid33x17", 1, np.float64)
    vals, flag = _raw(fc.matrix("grid33x17"), P)
    np.testing.assert_allclose(to_np(vals), want, **fc.tol(np.float64))
    assert int(flag.item()) == I32_MAX
    # the 33-entry row raises before any launch: the flag is never preset
    D = lsp.csr_array(fc.matrix("dense33"))
    with pytest.raises(ValueError, match=r"row 32 .*FSAI_MAX_ROW = 32"):
        linalg.fsai(D, lsp.csr_array(fc.pattern("dense33", "given")))
    sentinel = torch.full((1,), 123, dtype=torch.int32, device="cuda")
    A33, P33 = fc.matrix("dense33"), fc.pattern("dense33", "given")
    cv = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a)).to(dt).cuda()
    for mr in (32, 33):
        with pytest.raises(ValueError):
            ops.fsai_rows(cv(P33.indptr, torch.int64),
                          cv(P33.indices, torch.int32),
                          cv(A33.indptr, torch.int64),
                          cv(A33.indices, torch.int32),
                          cv(A33.data, torch.float64), 0, 0, sentinel, mr)
    assert int(sentinel.item()) == 123


@pytest.mark.parametrize("name,p,dtype", [
    ("grid33x17", 3, np.float64), ("grid9x8x7", 1, np.float32),
    ("herm300", 1, np.complex128)])
def test_gpu_fsai_apply(name, p, dtype):
    P, gv = fc.reference(name, p, dtype)
    n = P.shape[0]
    M = _build(name, p, dtype)
    r = fc.rhs(n, None, dtype)
    rt = torch.from_numpy(r).cuda()
    want = fc.apply_reference(P, gv, r)
    got = M.matvec(rt)
    assert got.is_cuda
    np.testing.assert_allclose(to_np(got), want, **fc.tol(dtype))
    out = torch.empty_like(rt)
    assert M.matvec(rt, out=out) is out and torch.equal(out, got)
    for k in (5, 40):
        R = fc.rhs(n, k, dtype, seed=k)
        blk = M.matmat(torch.from_numpy(R).cuda())
        assert blk.is_cuda and tuple(blk.shape) == (n, k)
        np.testing.assert_allclose(to_np(blk), fc.apply_reference(P, gv, R),
                                   **fc.tol(dtype))


def test_gpu_fsai_refactor():
    S = fc.matrix("grid33x17")
    M = linalg.fsai(lsp.csr_array(S), 2)
    G, GH = M.G, M.GH
    r = torch.from_numpy(fc.rhs(S.shape[0], None, np.float64)).cuda()
    M.matvec(r)                              # plans and value caches built
    S2 = sp.csr_array(S * 2.5 + sp.identity(S.shape[0]))
    S2.sort_indices()
    A2 = lsp.csr_array(S2)
    assert M.refactor(A2) is M and M.G is G and M.GH is GH
    fresh = linalg.fsai(A2, 2)
    assert torch.equal(M.G.data, fresh.G.data)
    assert torch.equal(M.GH.data, fresh.GH.data)
    assert torch.equal(M.matvec(r), fresh.matvec(r))


def test_gpu_cg_with_fsai():
    """jump-48^2, fp64, rtol 1e-8, true residual checked."""
    S = fc.matrix("jump48")
    A = lsp.csr_array(S)
    b = fc.rhs(S.shape[0], None, np.float64, seed=9)
    bt = torch.from_numpy(b).cuda()
    it = {}
    for label, M in (("none", None), ("p1", linalg.fsai(A)),
                     ("p2", linalg.fsai(A, 2))):
        x, n_it = linalg.cg(A, bt, rtol=1e-8, M=M, maxiter=5000)
        assert x.is_cuda
        res = np.linalg.norm(b - S @ to_np(x)) / np.linalg.norm(b)
        print(f"cg on jump48, M={label}: {n_it} iterations, true relative "
              f"residual {res:.2e}")
        assert res <= 1e-7
        it[label] = n_it
    assert 2 * it["p1"] <= it["none"]
    assert it["p2"] <= it["p1"]

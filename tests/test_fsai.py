# SPDX-License-Identifier: Apache-2.0
"""linalg.fsai on the CPU path: the factor's values against the per-row
numpy reference, its defining properties, patterns, the apply, refactor,
the error paths and the solvers that take it as M (docs/DESIGN.md §18)."""
import numpy as np
import pytest
import scipy.sparse as sp

import legate_sparse as lsp
from legate_sparse import linalg, ops
from testutils import to_np
import fsai_cases as fc

torch = pytest.importorskip("torch")


def _build(name, p, dtype, **kw):
    A = lsp.csr_array(fc.matrix(name, dtype))
    pat = lsp.csr_array(fc.pattern(name, p)) if p == "given" else p
    return linalg.FSAI(A, pat, **kw)


def _raw(A, P, idx_dtype, device="cpu", max_row=None, **kw):
    """ops.fsai_rows straight on arrays -> (values, flag)."""
    cv = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a)).to(dt) \
        .to(device)
    flag = torch.empty(1, dtype=torch.int32, device=device)
    if max_row is None:
        max_row = int(np.diff(P.indptr).max())
    vals = ops.fsai_rows(
        cv(P.indptr, torch.int64), cv(P.indices, idx_dtype),
        cv(A.indptr, torch.int64), cv(A.indices, idx_dtype),
        torch.from_numpy(A.data.copy()).to(device), 0, 0, flag, max_row,
        **kw)
    return vals, flag


@pytest.mark.parametrize("name,p,dtype", fc.VALUE_CASES)
def test_values(name, p, dtype):
    P, want = fc.reference(name, p, dtype)
    M = _build(name, p, dtype)
    assert isinstance(M, linalg.LinearOperator)
    assert M.shape == P.shape and M.dtype == np.dtype(dtype)
    G = fc.as_scipy(M.G)
    assert np.array_equal(G.indptr, P.indptr)
    assert np.array_equal(G.indices, P.indices)
    err = np.abs(G.data - want).max()
    print(f"{name} p={p} {np.dtype(dtype).name}: longest row "
          f"{np.diff(P.indptr).max()}, max |G - ref| {err:.3e}")
    np.testing.assert_allclose(G.data, want, **fc.tol(dtype))
    # GH is G's conjugate transpose
    GH = fc.as_scipy(M.GH)
    assert abs(GH - G.conj().T).max() == 0
    # the diagonal is real and positive, diag(G A G^H) = 1
    d = G.diagonal()
    assert np.all(d.real > 0) and np.all(d.imag == 0)
    w = fc.wide(dtype)
    Gw, Aw = G.astype(w), fc.matrix(name, dtype).astype(w)
    one = (Gw @ Aw @ Gw.conj().T).diagonal()
    np.testing.assert_allclose(one, np.ones(P.shape[0]), **fc.tol(dtype))
    # both index dtypes through the raw op
    for idt in (torch.int32, torch.int64):
        vals, flag = _raw(fc.matrix(name, dtype), P, idt)
        np.testing.assert_allclose(to_np(vals), want, **fc.tol(dtype))
        assert int(flag) == 2 ** 31 - 1


@pytest.mark.parametrize("dtype", fc.DTYPES)
def test_dense_is_inverse_cholesky(dtype):
    A = fc.matrix("dense32", dtype)
    G = fc.as_scipy(_build("dense32", "given", dtype).G).toarray()
    want = np.linalg.inv(np.linalg.cholesky(
        A.toarray().astype(fc.wide(dtype))))
    np.testing.assert_allclose(G, want, **fc.tol(dtype))


def test_upper_triangle_is_never_read():
    A = fc.matrix("grid33x17")
    want = fc.as_scipy(linalg.fsai(lsp.csr_array(A)).G)
    junk = sp.csr_array(sp.tril(A, 0) + 7.5 * sp.triu(A, 1))
    got = fc.as_scipy(linalg.fsai(lsp.csr_array(junk)).G)
    assert np.array_equal(got.data, want.data)


def test_pattern_forms():
    A = lsp.csr_array(fc.matrix("grid9x8x7"))
    base = fc.as_scipy(linalg.fsai(A, 2).G)
    # None is 1; an explicit pattern equals the int pattern, and only its
    # lower triangle counts
    assert np.array_equal(fc.as_scipy(linalg.fsai(A).G).data,
                          fc.as_scipy(linalg.fsai(A, 1).G).data)
    P = fc.pattern("grid9x8x7", 2)
    for pat in (P, sp.csr_array(P + sp.triu(P.T, 1))):
        G = fc.as_scipy(linalg.fsai(A, lsp.csr_array(pat)).G)
        assert np.array_equal(G.indices, base.indices)
        assert np.array_equal(G.data, base.data)
    with pytest.raises(ValueError):
        linalg.fsai(A, 0)
    with pytest.raises(TypeError):
        linalg.fsai(A, 1.5)
    with pytest.raises(ValueError, match="shape"):
        linalg.fsai(A, lsp.csr_array(fc.pattern("grid33x17", 1)))


def _halved(S):
    """S with every entry stored as two halves (duplicates installed
    through the indices setter)."""
    rep = np.repeat(np.arange(S.nnz), 2)
    dup = lsp.csr_array.__new__(lsp.csr_array)
    dev = lsp.csr_array(S).data.device
    dup._init_local(torch.from_numpy(2 * S.indptr.astype(np.int64)).to(dev),
                    torch.from_numpy(S.indices[rep].astype(np.int64)).to(dev),
                    torch.from_numpy(S.data[rep] / 2).to(dev), S.shape)
    dup.indices = dup.indices.clone()
    assert not dup.has_canonical_format
    return dup


def test_non_canonical_input():
    """Duplicates are summed on a copy, the input is left alone; refactor
    takes the same non-canonical matrix, and a canonical one."""
    S = fc.matrix("rand300")
    want = fc.as_scipy(linalg.fsai(lsp.csr_array(S)).G)
    dup = _halved(S)
    before = dup.data.clone()
    M = linalg.fsai(dup)
    got = fc.as_scipy(M.G)
    assert torch.equal(dup.data, before) and dup.nnz_local == 2 * S.nnz
    assert np.array_equal(got.indices, want.indices)
    np.testing.assert_allclose(got.data, want.data, **fc.tol(np.float64))
    first = M.G.data.clone()
    M.refactor(dup)
    assert torch.equal(M.G.data, first)
    S2 = sp.csr_array(S * 2.0 + sp.identity(S.shape[0]))
    S2.sort_indices()
    fresh = linalg.fsai(lsp.csr_array(S2))
    for A2 in (_halved(S2), lsp.csr_array(S2)):
        M.refactor(A2)
        np.testing.assert_allclose(to_np(M.G.data), to_np(fresh.G.data),
                                   **fc.tol(np.float64))
        np.testing.assert_allclose(to_np(M.GH.data), to_np(fresh.GH.data),
                                   **fc.tol(np.float64))


@pytest.mark.parametrize("name,p,dtype", [
    ("grid33x17", 3, np.float64), ("grid9x8x7", 1, np.float32),
    ("herm300", 1, np.complex128), ("herm300", 1, np.complex64)])
def test_apply(name, p, dtype):
    P, gv = fc.reference(name, p, dtype)
    n = P.shape[0]
    M = _build(name, p, dtype)
    r = fc.rhs(n, None, dtype)
    want = fc.apply_reference(P, gv, r)
    got = M.matvec(r)
    np.testing.assert_allclose(to_np(got), want, **fc.tol(dtype))
    np.testing.assert_allclose(to_np(M.rmatvec(r)), want, **fc.tol(dtype))
    dev = M.G.data.device           # the runtime's device: cpu or a GPU
    rt = torch.from_numpy(r).to(dev)
    out = torch.empty_like(rt)
    assert M.matvec(rt, out=out) is out
    np.testing.assert_allclose(to_np(out), want, **fc.tol(dtype))
    for k in (5, 40):
        R = fc.rhs(n, k, dtype, seed=k)
        for blk in (M.matmat(torch.from_numpy(R).to(dev)), M.rmatmat(R)):
            assert tuple(blk.shape) == (n, k)
            np.testing.assert_allclose(
                to_np(blk), fc.apply_reference(P, gv, R), **fc.tol(dtype))
    with pytest.raises(ValueError):
        M.matmat(r)


def test_refactor():
    S = fc.matrix("grid33x17")
    A = lsp.csr_array(S)
    M = linalg.fsai(A, 2)
    G, GH = M.G, M.GH
    r = fc.rhs(S.shape[0], None, np.float64)
    M.matvec(r)
    S2 = sp.csr_array(S * 2.5 + sp.identity(S.shape[0]))
    S2.sort_indices()
    A2 = lsp.csr_array(S2)
    assert M.refactor(A2) is M and M.G is G and M.GH is GH
    fresh = linalg.fsai(A2, 2)
    assert torch.equal(M.G.data, fresh.G.data)
    assert torch.equal(M.GH.data, fresh.GH.data)
    assert torch.equal(M.matvec(r), fresh.matvec(r))
    with pytest.raises(ValueError, match="pattern"):
        M.refactor(lsp.csr_array(fc.matrix("grid9x8x7")))
    other = sp.lil_matrix(S)
    other[0, 5] = other[5, 0] = -0.5
    with pytest.raises(ValueError, match="pattern"):
        M.refactor(lsp.csr_array(sp.csr_array(other.tocsr())))


def test_errors():
    with pytest.raises(ValueError, match="square"):
        linalg.fsai(lsp.csr_array(sp.csr_array(np.ones((3, 4)))))
    # a pattern row without its diagonal
    A = lsp.csr_array(fc.matrix("grid33x17"))
    P = sp.lil_matrix(fc.pattern("grid33x17", 1))
    P[9, 9] = 0
    P = sp.csr_array(P.tocsr())
    P.eliminate_zeros()
    with pytest.raises(ValueError, match="diagonal"):
        linalg.fsai(A, lsp.csr_array(P))
    # a row of 33 entries: the limit and the global row are named
    D = lsp.csr_array(fc.matrix("dense33"))
    with pytest.raises(ValueError, match=r"row 32 .*FSAI_MAX_ROW = 32"):
        linalg.fsai(D, lsp.csr_array(fc.pattern("dense33", "given")))
    assert ops.FSAI_MAX_ROW == 32
    from legate_sparse import _cext
    assert _cext.require_cpu().FSAI_MAX_ROW == ops.FSAI_MAX_ROW
    # not positive definite: the smallest bad row is named
    with pytest.raises(RuntimeError, match=r"not positive definite at row "
                                           r"7\b"):
        linalg.fsai(lsp.csr_array(fc.indefinite_diag(7)))
    with pytest.raises(RuntimeError, match=r"not positive definite at row "
                                           r"11\b"):
        linalg.fsai(lsp.csr_array(fc.indefinite_block(11)))
    N = fc.matrix("grid33x17").copy()
    N.data[N.indptr[40]] = np.nan
    with pytest.raises(RuntimeError, match="not positive definite"):
        linalg.fsai(lsp.csr_array(N))


def test_raw_op_checks_its_arguments():
    A, P = fc.matrix("grid33x17"), fc.pattern("grid33x17", 1)
    _raw(A, P, torch.int32)
    with pytest.raises(ValueError, match="max_row|longest row"):
        _raw(A, P, torch.int32, max_row=2)
    with pytest.raises(ValueError, match="FSAI_MAX_ROW"):
        _raw(A, P, torch.int32, max_row=33)
    bad = P.copy()
    s = bad.indptr[50]
    bad.indices[s], bad.indices[s + 1] = bad.indices[s + 1], bad.indices[s]
    with pytest.raises(ValueError, match="sorted|diagonal"):
        _raw(A, bad, torch.int32)
    # a window that does not cover the pattern's columns
    flag = torch.empty(1, dtype=torch.int32)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    with pytest.raises(ValueError, match="cover"):
        ops.fsai_rows(t(P.indptr).long(), t(P.indices).int(),
                      t(A.indptr[:101]).long(), t(A.indices).int(),
                      t(A.data), 0, 0, flag, 3)
    with pytest.raises(ValueError, match="dtype|contiguous"):
        ops.fsai_rows(t(P.indptr).long(), t(P.indices).long(),
                      t(A.indptr).long(), t(A.indices).int(), t(A.data), 0,
                      0, flag, 3)


def test_raw_op_window_and_torch_arm():
    """A sliced window (row_offset != 0) and the torch arm give the
    reference values."""
    name, p = "grid9x8x7", 2
    A = fc.matrix(name)
    P, want = fc.reference(name, p, np.float64)
    lo, hi = 200, 330
    w0 = int(P.indices[P.indptr[lo]:P.indptr[hi]].min())
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a)).to(dt)
    flag = torch.empty(1, dtype=torch.int32)
    args = (t(P.indptr[lo:hi + 1] - P.indptr[lo], torch.int64),
            t(P.indices[P.indptr[lo]:P.indptr[hi]], torch.int32),
            t(A.indptr[w0:hi + 1] - A.indptr[w0], torch.int64),
            t(A.indices[A.indptr[w0]:A.indptr[hi]], torch.int32),
            t(A.data[A.indptr[w0]:A.indptr[hi]], torch.float64), w0, lo,
            flag, 13)
    assert w0 > 0
    ref = want[P.indptr[lo]:P.indptr[hi]]
    for impl in ("native", "torch"):
        vals = ops.fsai_rows(*args, _impl=impl)
        np.testing.assert_allclose(to_np(vals), ref, **fc.tol(np.float64))
        assert int(flag) == 2 ** 31 - 1
    B = fc.indefinite_block(11)
    _, flag = _raw(B, sp.csr_array(sp.tril(B, 0)), torch.int32,
                   _impl="torch")
    assert int(flag) == 11


def test_solvers_accept_fsai():
    S = fc.matrix("grid33x17")
    A = lsp.csr_array(S)
    M = linalg.fsai(A, 2)
    b = fc.rhs(S.shape[0], None, np.float64)
    for solver, kw in ((linalg.cg, {}), (linalg.bicgstab, {}),
                       (linalg.gmres, {"restart": 40})):
        x = solver(A, b, rtol=1e-8, M=M, **kw)[0]
        res = np.linalg.norm(b - S @ to_np(x)) / np.linalg.norm(b)
        print(f"{solver.__name__}: true relative residual {res:.2e}")
        assert res <= 1e-7


def test_lobpcg_with_fsai():
    import lobpcg_cases as lc
    n, k = 1000, 4
    d = np.linspace(1.0, 100.0, n)
    off = -0.3 * np.ones(n - 1)
    H = sp.diags([d, off, off], [0, -1, 1], format="csr")
    Lh = lsp.csr_array(H)
    X0 = lc.start_block(n, k, np.float64, 0)
    w, _ = linalg.lobpcg(Lh, X0, M=linalg.fsai(Lh, 2), tol=1e-8, maxiter=100,
                         largest=False)
    np.testing.assert_allclose(w, np.linalg.eigvalsh(H.toarray())[:k],
                               rtol=0, atol=1e-8)


def test_cg_iteration_condition():
    """jump-48^2, fp64, rtol 1e-8: FSAI at least halves the iterations and
    a richer pattern does not need more."""
    S = fc.matrix("jump48")
    A = lsp.csr_array(S)
    b = fc.rhs(S.shape[0], None, np.float64, seed=9)
    it = {}
    for label, M in (("none", None), ("p1", linalg.fsai(A)),
                     ("p2", linalg.fsai(A, 2))):
        x, n_it = linalg.cg(A, b, rtol=1e-8, M=M, maxiter=5000)
        res = np.linalg.norm(b - S @ to_np(x)) / np.linalg.norm(b)
        print(f"cg on jump48, M={label}: {n_it} iterations, true relative "
              f"residual {res:.2e}")
        assert res <= 1e-7
        it[label] = n_it
    assert 2 * it["p1"] <= it["none"]
    assert it["p2"] <= it["p1"]

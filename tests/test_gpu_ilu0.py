# SPDX-License-Identifier: Apache-2.0
"""GPU numerics of the ILU(0) factor kernels (src/hip/sptrsv.hip) and of
linalg.ilu0 on top of them: factor values against the pure-Python IKJ
reference on both working-row paths, launch-plan edges, run-to-run
identity, the pivot flag, the apply, and end-to-end preconditioned solves
(pytest -m gpu on an MI355X)."""
import numpy as np
import pytest
import scipy.sparse as sp

import legate_sparse as lsp
from legate_sparse import linalg, ops
from testutils import to_np
import ilu0_cases as ic

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

_DT = {"grid33x17": ic.DTYPES[:2], "grid9x8x7": ic.DTYPES[:2],
       "rand300sym": ic.DTYPES, "complex": ic.DTYPES[2:],
       "arrow600sym": ic.DTYPES}
CASES = [(n, d) for n in _DT for d in _DT[n]]


@pytest.fixture(scope="module", autouse=True)
def _check_native():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from legate_sparse import _cext
    # GPU runs MUST use the gfx950 extension — no silent fallback
    _cext.require_hip()
    yield


def _raw_factor(A, idx_dtype=torch.int32, **kw):
    """ops.ilu0_factor straight on device arrays -> (values, flag)."""
    n = A.shape[0]
    indptr = torch.from_numpy(A.indptr.astype(np.int64)).cuda()
    indices = torch.from_numpy(A.indices.astype(np.int64)).cuda() \
        .to(idx_dtype)
    F = torch.from_numpy(A.data.copy()).cuda()
    dpos, has = ops.diag_positions(indptr, indices, n)
    assert bool(has.all())
    sched = ops.level_schedule(indptr, indices, n, True)
    flag = torch.empty(1, dtype=torch.int32, device="cuda")
    ops.ilu0_factor(indptr, indices, F, dpos, sched, flag,
                    int(np.diff(A.indptr).max()), **kw)
    return F, flag, sched


@pytest.mark.parametrize("name,dtype", CASES)
def test_gpu_ilu0_factor_and_apply(name, dtype):
    A = ic.ilu_matrix(name, dtype)
    n = A.shape[0]
    Fref = ic.ilu0_reference(A)
    M = linalg.ilu0(lsp.csr_array(A))
    fv = M.factor_local()[2]
    assert fv.is_cuda
    err = np.abs(to_np(fv) - Fref.data).max()
    print(f"{name} {np.dtype(dtype).name}: factor |err| {err:.3e}, "
          f"longest row {np.diff(A.indptr).max()}, levels {M.levels}, "
          f"launches per apply {M.launches_per_apply}")
    np.testing.assert_allclose(to_np(fv), Fref.data, **ic.tol(dtype))
    assert M.launches_per_apply <= sum(M.levels)
    for idt in (torch.int32, torch.int64):
        F, flag, _ = _raw_factor(A, idt)
        np.testing.assert_allclose(to_np(F), Fref.data, **ic.tol(dtype))
        assert int(flag.item()) == 2 ** 31 - 1

    r = ic.rhs(n, None, A.dtype)
    want = ic.ilu_apply_reference(Fref, r)
    rt = torch.from_numpy(r).cuda()
    got = M.matvec(rt)
    np.testing.assert_allclose(to_np(got), want, **ic.tol(dtype))
    out = torch.empty_like(rt)
    assert M.matvec(rt, out=out) is out and torch.equal(out, got)
    for k in (5, 8, 40):
        Rb = ic.rhs(n, k, A.dtype, seed=k)
        blk = M.matmat(torch.from_numpy(Rb).cuda())
        assert tuple(blk.shape) == (n, k)
        for j in (0, k // 2, k - 1):
            wj = ic.ilu_apply_reference(Fref, np.ascontiguousarray(Rb[:, j]))
            np.testing.assert_allclose(to_np(blk[:, j]), wj, **ic.tol(dtype))


@pytest.mark.parametrize("name", ["grid33x17", "rand300sym", "arrow600sym"])
def test_gpu_ilu0_plan_edges(name):
    """All-wide, all-chain and mixed plans and a capped grid give the same
    factor: each row's arithmetic does not depend on the plan."""
    A = ic.ilu_matrix(name, np.float64)
    Fref = ic.ilu0_reference(A)
    base, _, sched = _raw_factor(A)
    np.testing.assert_allclose(to_np(base), Fref.data, **ic.tol(np.float64))
    for chain_rows in (1, 16, None, 10 ** 6):
        for cap in (1, 2, None):
            F, flag, _ = _raw_factor(A, _chain_rows=chain_rows,
                                     _grid_cap=cap)
            print(f"{name} chain_rows={chain_rows} cap={cap}: launches "
                  f"{sched.n_launches(chain_rows)}, bit-equal to the "
                  f"default plan: {torch.equal(F, base)}")
            np.testing.assert_allclose(to_np(F), Fref.data,
                                       **ic.tol(np.float64))
            np.testing.assert_allclose(to_np(F), to_np(base),
                                       **ic.tol(np.float64))
            assert int(flag.item()) == 2 ** 31 - 1


def test_gpu_ilu0_bit_identical():
    for name in ("rand300sym", "arrow600sym", "grid9x8x7"):
        A = ic.ilu_matrix(name, np.float32)
        assert torch.equal(_raw_factor(A)[0], _raw_factor(A)[0])


def test_gpu_ilu0_torch_arm():
    A = ic.ilu_matrix("grid33x17", np.float64)
    F, flag, _ = _raw_factor(A, _impl="torch")
    np.testing.assert_allclose(to_np(F), ic.ilu0_reference(A).data,
                               **ic.tol(np.float64))
    assert int(flag.item()) == 2 ** 31 - 1


def test_gpu_ilu0_pivot_flag():
    with pytest.raises(RuntimeError, match=r"row 1\b"):
        linalg.ilu0(lsp.csr_array(ic.zero_pivot_matrix()))
    # the flag holds the SMALLEST offending row: every row after row 1
    # divides by the zero pivot and turns non-finite as well
    for n in (8, 700):
        _, flag, _ = _raw_factor(ic.zero_pivot_matrix(n))
        assert int(flag.item()) == 1
    # a NaN planted in A
    N = ic.ilu_matrix("grid33x17", np.float64).copy()
    N.data[N.indptr[40]] = np.nan
    with pytest.raises(RuntimeError, match="pivot"):
        linalg.ilu0(lsp.csr_array(N))
    # missing diagonal: ValueError before any kernel
    D = sp.lil_matrix(ic.ilu_matrix("grid33x17", np.float64))
    D[3, 3] = 0
    D = sp.csr_array(D.tocsr())
    D.eliminate_zeros()
    with pytest.raises(ValueError, match="diagonal"):
        linalg.ilu0(lsp.csr_array(D))


def test_gpu_ilu0_refactor():
    A = ic.ilu_matrix("grid33x17", np.float64)
    M = linalg.ilu0(lsp.csr_array(A))
    A2 = sp.csr_array(A * 2.5 + sp.identity(A.shape[0]))
    A2.sort_indices()
    M.refactor(lsp.csr_array(A2))
    np.testing.assert_allclose(to_np(M.factor_local()[2]),
                               ic.ilu0_reference(A2).data,
                               **ic.tol(np.float64))
    with pytest.raises(ValueError):
        M.refactor(lsp.csr_array(ic.ilu_matrix("grid9x8x7", np.float64)))


def test_gpu_bicgstab_with_ilu0():
    A = ic.ilu_matrix("grid33x17", np.float64)
    La = lsp.csr_array(A)
    b = ic.rhs(A.shape[0], None, np.float64)
    iters = {}
    for label, M in (("none", None), ("ilu0", linalg.ilu0(La))):
        calls = []
        x, info = linalg.bicgstab(La, torch.from_numpy(b).cuda(), rtol=1e-8,
                                  M=M, conv_test_iters=1,
                                  callback=lambda xk: calls.append(1))
        assert info == 0 and x.is_cuda
        assert np.linalg.norm(b - A @ to_np(x)) <= 1e-7 * np.linalg.norm(b)
        iters[label] = len(calls)
    print(f"bicgstab iterations {iters}")
    assert 2 * iters["ilu0"] < iters["none"]


def test_gpu_cg_with_ilu0():
    A = ic.poisson2d(24, 24)
    La = lsp.csr_array(A)
    b = ic.rhs(576, None, np.float64)
    bt = torch.from_numpy(b).cuda()
    _, plain = linalg.cg(La, bt, rtol=1e-8, conv_test_iters=1)
    x, pre = linalg.cg(La, bt, rtol=1e-8, M=linalg.ilu0(La),
                       conv_test_iters=1)
    print(f"cg iterations: M=None {plain}, M=ilu0 {pre}")
    assert 2 * pre < plain
    assert np.linalg.norm(b - A @ to_np(x)) <= 1e-7 * np.linalg.norm(b)

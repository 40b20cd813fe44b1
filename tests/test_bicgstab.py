# SPDX-License-Identifier: Apache-2.0
"""BiCGSTAB on the CPU path: convergence on nonsymmetric operators, the
call contract, the guarded (frozen) iteration, breakdown reporting, a
5-step replay against a numpy transcription, and the four fused ops
against their numpy formulas."""
import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spla
import torch

import legate_sparse as lsp
from legate_sparse import ops
from legate_sparse.linalg import LinearOperator
from legate_sparse.runtime import runtime
from testutils import to_np
import bicgstab_cases as bc

DTYPES = bc.DTYPES


def _solve_and_check(S, b, **kw):
    dtype = S.dtype
    rtol = bc.solve_rtol(dtype)
    x, info = lsp.linalg.bicgstab(lsp.csr_array(S), b, rtol=rtol, **kw)
    res = bc.rel_residual(S, to_np(x), b)
    print(f"{np.dtype(dtype).name}: info={info} true residual={res:.3e}")
    assert info == 0
    assert res <= 10 * rtol
    return x


# ---- convergence ---------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_converges_convdiff(dtype):
    S = bc.convdiff(24, 24, dtype=dtype)
    _solve_and_check(S, bc.rhs(S.shape[0], dtype))


@pytest.mark.parametrize("dtype", DTYPES)
def test_converges_nonaffine(dtype):
    S = bc.nonaffine(dtype)
    _solve_and_check(S, bc.rhs(300, dtype), conv_test_iters=5)


def test_stencil_grid_is_convdiff():
    # sanity check of the test helper only (passes without the solver):
    # the stencil_grid operator the GPU and multi-process tests solve with
    # is the scipy matrix their residuals are measured against
    for dtype, shape in ((np.float64, (33, 17)), (np.complex128, (24, 24))):
        A = bc.convdiff_lsp(*shape, dtype=dtype)
        S = bc.convdiff(*shape, dtype=dtype)
        assert abs(sp.csr_array(to_np(A.todense())) - S).max() == 0


# ---- x0 and b = 0 --------------------------------------------------------
def test_x0_at_solution():
    S = bc.convdiff(24, 24)
    b = bc.rhs(576, np.float64)
    x0 = spla.spsolve(S.tocsc(), b)
    x, info = lsp.linalg.bicgstab(lsp.csr_array(S), b, x0=x0, rtol=1e-10)
    assert info == 0
    assert bc.rel_residual(S, to_np(x), b) <= 1e-9


def test_x0_rough_guess():
    S = bc.convdiff(24, 24)
    b = bc.rhs(576, np.float64)
    _solve_and_check(S, b, x0=bc.rhs(576, np.float64, seed=8))


def test_zero_rhs():
    S = bc.convdiff(24, 24)
    x, info = lsp.linalg.bicgstab(lsp.csr_array(S), np.zeros(576))
    assert info == 0
    assert not to_np(x).any()


# ---- preconditioner ------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kind", ["csr", "operator"])
def test_jacobi_preconditioner(kind, dtype):
    S = bc.nonaffine(dtype)
    dinv = (1.0 / S.diagonal()).astype(dtype)
    if kind == "csr":
        M = lsp.csr_array(sp.csr_array(sp.diags(dinv).tocsr()))
    else:
        dinv_t = torch.from_numpy(dinv).to(runtime.device)
        M = LinearOperator(S.shape, matvec=lambda z: z * dinv_t, dtype=dtype)
    _solve_and_check(S, bc.rhs(300, dtype), M=M, conv_test_iters=5)


# ---- maxiter exhaustion --------------------------------------------------
def test_maxiter_exhausted():
    S = bc.convdiff(24, 24)
    x, info = lsp.linalg.bicgstab(lsp.csr_array(S), bc.rhs(576, np.float64),
                                  maxiter=3, rtol=1e-12)
    assert info == 3
    assert np.isfinite(to_np(x)).all()


# ---- frozen iteration: r reaches zero between two convergence tests ------
@pytest.mark.parametrize("name", ["3x3", "2I"])
def test_frozen_iteration_stays_finite(name):
    if name == "3x3":
        D = np.array([[4.0, 1, 0], [2, 5, 1], [0, 1, 3]])
        b = np.array([1.0, 2.0, 3.0])
    else:
        D = 2.0 * np.eye(7)
        b = np.arange(1.0, 8.0)
    x, info = lsp.linalg.bicgstab(lsp.csr_array(sp.csr_array(D)), b,
                                  conv_test_iters=25, rtol=1e-12)
    x = to_np(x)
    assert info == 0
    assert np.isfinite(x).all()
    assert np.linalg.norm(b - D @ x) <= 1e-12 * np.linalg.norm(b)


# ---- breakdown -----------------------------------------------------------
def test_breakdown_reports_negative_info():
    D = np.array([[0.0, 1.0], [-1.0, 0.0]])
    x, info = lsp.linalg.bicgstab(lsp.csr_array(sp.csr_array(D)),
                                  np.array([1.0, 0.0]), maxiter=50)
    assert info < 0
    assert np.isfinite(to_np(x)).all()


# ---- call contract -------------------------------------------------------
def test_column_rhs_accepted_and_block_rejected():
    S = bc.convdiff(24, 24)
    A = lsp.csr_array(S)
    b = bc.rhs(576, np.float64)
    x, info = lsp.linalg.bicgstab(A, b.reshape(-1, 1), rtol=1e-10)
    assert info == 0
    assert bc.rel_residual(S, to_np(x), b) <= 1e-9
    with pytest.raises(ValueError):
        lsp.linalg.bicgstab(A, np.ones((576, 2)))


def test_non_square_raises():
    S = bc.convdiff(24, 24)[:500]
    with pytest.raises(ValueError):
        lsp.linalg.bicgstab(lsp.csr_array(sp.csr_array(S)), np.ones(500))


def _count_iters(S, b, **kw):
    calls = []
    x, info = lsp.linalg.bicgstab(lsp.csr_array(S), b, conv_test_iters=1,
                                  callback=lambda xk: calls.append(1), **kw)
    return x, info, len(calls)


def test_callback_once_per_iteration():
    S = bc.convdiff(24, 24)
    _, info, calls = _count_iters(S, bc.rhs(576, np.float64), maxiter=3,
                                  rtol=1e-12)
    assert info == 3 and calls == 3


def test_tol_is_alias_of_rtol():
    S = bc.convdiff(24, 24)
    b = bc.rhs(576, np.float64)
    x_t, info_t, n_t = _count_iters(S, b, tol=1e-10)
    x_r, info_r, n_r = _count_iters(S, b, rtol=1e-10)
    _, _, n_default = _count_iters(S, b)
    assert info_t == 0 and info_r == 0
    assert n_t == n_r and n_t > n_default
    assert np.array_equal(to_np(x_t), to_np(x_r))
    assert bc.rel_residual(S, to_np(x_t), b) <= 1e-9


def test_atol_dominates_when_larger():
    S = bc.convdiff(24, 24)
    b = bc.rhs(576, np.float64)
    atol = 1e-2 * np.linalg.norm(b)
    x, info, n_loose = _count_iters(S, b, rtol=1e-12, atol=atol)
    _, _, n_tight = _count_iters(S, b, rtol=1e-12)
    assert info == 0 and n_loose < n_tight
    assert np.linalg.norm(b - S @ to_np(x)) <= 10 * atol


# ---- 5-step replay: pins the order of the updates and the scalars --------
@pytest.mark.parametrize("dtype", [np.float64, np.complex128])
def test_five_step_replay(dtype):
    S = bc.convdiff(24, 24, dtype=dtype)
    b = bc.rhs(576, dtype)
    x, info = lsp.linalg.bicgstab(lsp.csr_array(S), b, maxiter=5,
                                  conv_test_iters=5, rtol=0)
    want = bc.np_replay(S, b, 5)
    assert info == 5
    err = np.linalg.norm(to_np(x) - want) / np.linalg.norm(want)
    print(f"{np.dtype(dtype).name}: replay error {err:.3e}")
    assert err <= 1e-10


# ---- the four fused ops against numpy ------------------------------------
N = 1000


def _tol(dtype):
    if np.dtype(dtype) in (np.dtype(np.float32), np.dtype(np.complex64)):
        return dict(rtol=1e-4, atol=1e-4)
    return dict(rtol=1e-10, atol=1e-12)


def _vecs(dtype, count):
    return [bc.rhs(N, dtype, seed=20 + i) for i in range(count)]


def _scalars(dtype, zero=None):
    """rho, rhv, ts, tt as numpy scalars of ``dtype``; ``zero`` names the
    one set to exactly zero."""
    vals = dict(zip(("rho", "rhv", "ts", "tt"),
                    bc.rhs(4, dtype, seed=31) + np.dtype(dtype).type(2)))
    if zero is not None:
        vals[zero] = np.dtype(dtype).type(0)
    return vals


def _t(a):
    return torch.from_numpy(np.atleast_1d(np.asarray(a)).copy())


@pytest.mark.parametrize("zero", [None, "rhv", "ts", "tt"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_op_bicgstab_p(dtype, zero):
    p, r, v = _vecs(dtype, 3)
    sc = _scalars(dtype, zero)
    want = bc.np_bicgstab_p(p, r, v, **sc)
    pt = _t(p)
    out = ops.bicgstab_p(pt, _t(r), _t(v), *(_t(sc[k]) for k in
                                              ("rho", "rhv", "ts", "tt")))
    assert out is pt
    assert np.isfinite(to_np(pt)).all()
    np.testing.assert_allclose(to_np(pt), want, **_tol(dtype))
    if zero:
        # any zero denominator freezes beta to zero: a restart, p = r
        np.testing.assert_array_equal(to_np(pt), r)


@pytest.mark.parametrize("zero", [None, "rhv"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_op_bicgstab_s(dtype, zero):
    r, v = _vecs(dtype, 2)
    sc = _scalars(dtype, zero)
    s = torch.full((N,), 7, dtype=_t(r).dtype)
    ops.bicgstab_s(s, _t(r), _t(v), _t(sc["rho"]), _t(sc["rhv"]))
    assert np.isfinite(to_np(s)).all()
    np.testing.assert_allclose(
        to_np(s), bc.np_bicgstab_s(r, v, sc["rho"], sc["rhv"]),
        **_tol(dtype))
    if zero:
        np.testing.assert_array_equal(to_np(s), r)


@pytest.mark.parametrize("dtype", DTYPES)
def test_op_vdot2(dtype):
    t, s = _vecs(dtype, 2)
    out2 = torch.full((2,), 5, dtype=_t(t).dtype)
    ops.vdot2(_t(t), _t(s), out2)
    np.testing.assert_allclose(to_np(out2), bc.np_vdot2(t, s),
                               **_tol(dtype))


def test_ops_refuse_mismatched_operands():
    # the HIP path would reinterpret these silently
    r, v = (_t(a) for a in _vecs(np.float64, 2))
    one = torch.ones(1, dtype=torch.float64)
    s = torch.empty(N, dtype=torch.float64)
    with pytest.raises(ValueError):
        ops.bicgstab_s(s, r.float(), v, one, one)       # vector dtype
    with pytest.raises(ValueError):
        ops.bicgstab_s(s, r[:-1], v, one, one)          # vector length
    with pytest.raises(ValueError):
        ops.bicgstab_s(s, r, v, one.float(), one)       # scalar dtype
    with pytest.raises(ValueError):
        ops.bicgstab_s(s, r, v, torch.ones(2, dtype=torch.float64), one)
    with pytest.raises(ValueError):
        ops.vdot2(r, v, torch.zeros(3, dtype=torch.float64))


@pytest.mark.parametrize("alias", [False, True])
@pytest.mark.parametrize("zero", [None, "rhv", "tt"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_op_bicgstab_xr(dtype, zero, alias):
    x, phat, shat, s, t, rhat = _vecs(dtype, 6)
    if alias:
        shat = s
    sc = _scalars(dtype, zero)
    xw, rw, ow = bc.np_bicgstab_xr(x, phat, shat, s, t, rhat, **sc)
    xt, rt = _t(x), torch.full((N,), 7, dtype=_t(x).dtype)
    st = _t(s)
    out2 = torch.full((2,), 5, dtype=xt.dtype)
    ops.bicgstab_xr(xt, rt, _t(phat), st if alias else _t(shat), st, _t(t),
                    _t(rhat), *(_t(sc[k]) for k in
                                ("rho", "rhv", "ts", "tt")), out2)
    for got in (xt, rt, out2):
        assert np.isfinite(to_np(got)).all()
    np.testing.assert_allclose(to_np(xt), xw, **_tol(dtype))
    np.testing.assert_allclose(to_np(rt), rw, **_tol(dtype))
    np.testing.assert_allclose(to_np(out2), ow, **_tol(dtype))
    if zero == "tt":
        np.testing.assert_array_equal(to_np(rt), s)

# SPDX-License-Identifier: Apache-2.0
"""GPU numerics of the BiCGSTAB HIP kernels (src/hip/solver_ops.hip) and
the solver on top of them: every size around the wave and block edges,
misaligned operands (the element-wise instantiation), zero denominators,
the grid-stride loop past the grid cap, end-to-end solves and the 5-step
replay (pytest -m gpu on an MI355X)."""
import numpy as np
import pytest
import scipy.sparse as sp

import legate_sparse as lsp
from legate_sparse import ops
from testutils import to_np
import bicgstab_cases as bc

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

DTYPES = bc.DTYPES
SIZES = [1, 63, 64, 65, 255, 256, 257, 1000]
SCALARS = ("rho", "rhv", "ts", "tt")
EXT = None


@pytest.fixture(scope="module", autouse=True)
def _check_native():
    global EXT
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from legate_sparse import _cext
    # GPU runs MUST use the gfx950 extension — no silent fallback
    EXT = _cext.require_hip()
    for k in ("BICGSTAB_P", "BICGSTAB_S", "VDOT2", "BICGSTAB_XR"):
        assert getattr(EXT, k + "_GRID_CAP") > 0
        assert getattr(EXT, k + "_PER_BLOCK") > 0
    yield


def _tol(dtype):
    # tolerances of test_gpu_spmm._tol
    if np.dtype(dtype) in (np.dtype(np.float32), np.dtype(np.complex64)):
        return dict(rtol=1e-4, atol=1e-4)
    return dict(rtol=1e-10, atol=1e-12)


def _wide(a):
    """float64 / complex128 copy: the reduced outputs are compared with a
    reference that carries no single-precision summation error of its own."""
    a = np.asarray(a)
    return a.astype(np.complex128 if a.dtype.kind == "c" else np.float64)


def _check_dots(name, got, want, dtype):
    err = np.abs(got - want)
    print(f"{name} {np.dtype(dtype).name}: |err| {err.max():.3e}, "
          f"smallest |want| {np.abs(want).min():.3e}")
    np.testing.assert_allclose(got, want, **_tol(dtype))


def _vecs(n, dtype, count):
    return [bc.rhs(n, dtype, seed=20 + i) for i in range(count)]


def _scalars(dtype, zero=None):
    vals = dict(zip(SCALARS,
                    bc.rhs(4, dtype, seed=31) + np.dtype(dtype).type(2)))
    if zero is not None:
        vals[zero] = np.dtype(dtype).type(0)
    return vals


def _dev(a, misalign=False):
    """Device copy; ``misalign`` returns a [1:] view of a longer buffer."""
    a = np.atleast_1d(np.asarray(a))
    if not misalign:
        return torch.from_numpy(a.copy()).cuda()
    buf = torch.zeros(a.size + 1, dtype=torch.from_numpy(a).dtype,
                      device="cuda")
    buf[1:] = torch.from_numpy(a.copy()).cuda()
    view = buf[1:]
    # off the 16-byte grid for every dtype narrower than 16 bytes
    # (complex128 has a single, element-wise instantiation anyway)
    assert view.data_ptr() % 16 == a.itemsize % 16
    return view


def _dev_scalars(sc):
    return [_dev(sc[k]) for k in SCALARS]


def _run_p(n, dtype, zero=None, misalign=False):
    p, r, v = _vecs(n, dtype, 3)
    sc = _scalars(dtype, zero)
    pt = _dev(p, misalign)
    ops.bicgstab_p(pt, _dev(r, misalign), _dev(v, misalign),
                   *_dev_scalars(sc))
    got = to_np(pt)
    assert np.isfinite(got).all()
    np.testing.assert_allclose(got, bc.np_bicgstab_p(p, r, v, **sc),
                               **_tol(dtype))
    if zero:
        np.testing.assert_array_equal(got, r)


def _run_s(n, dtype, zero=None, misalign=False):
    r, v = _vecs(n, dtype, 2)
    sc = _scalars(dtype, zero)
    st = _dev(np.full(n, 7, dtype=dtype), misalign)
    ops.bicgstab_s(st, _dev(r, misalign), _dev(v, misalign),
                   _dev(sc["rho"]), _dev(sc["rhv"]))
    got = to_np(st)
    assert np.isfinite(got).all()
    np.testing.assert_allclose(
        got, bc.np_bicgstab_s(r, v, sc["rho"], sc["rhv"]), **_tol(dtype))
    if zero:
        np.testing.assert_array_equal(got, r)


def _run_vdot2(n, dtype, misalign=False):
    t, s = _vecs(n, dtype, 2)
    out2 = _dev(np.full(2, 5, dtype=dtype))
    ops.vdot2(_dev(t, misalign), _dev(s, misalign), out2)
    _check_dots("vdot2", to_np(out2), bc.np_vdot2(_wide(t), _wide(s)),
                dtype)


def _run_xr(n, dtype, zero=None, misalign=False, alias=False):
    x, phat, shat, s, t, rhat = _vecs(n, dtype, 6)
    if alias:
        shat = s
    sc = _scalars(dtype, zero)
    xw, rw, _ = bc.np_bicgstab_xr(x, phat, shat, s, t, rhat, **sc)
    xt = _dev(x, misalign)
    rt = _dev(np.full(n, 7, dtype=dtype), misalign)
    st = _dev(s, misalign)
    out2 = _dev(np.full(2, 5, dtype=dtype))
    ops.bicgstab_xr(xt, rt, _dev(phat, misalign),
                    st if alias else _dev(shat, misalign), st,
                    _dev(t, misalign), _dev(rhat, misalign),
                    *_dev_scalars(sc), out2)
    for got in (xt, rt, out2):
        assert np.isfinite(to_np(got)).all()
    np.testing.assert_allclose(to_np(xt), xw, **_tol(dtype))
    np.testing.assert_allclose(to_np(rt), rw, **_tol(dtype))
    wide = {k: _wide(val) for k, val in sc.items()}
    _, _, ow = bc.np_bicgstab_xr(*(_wide(a) for a in
                                   (x, phat, shat, s, t, rhat)), **wide)
    _check_dots("bicgstab_xr", to_np(out2), ow, dtype)
    if zero == "tt":
        np.testing.assert_array_equal(to_np(rt), s)
    # the inputs were only read
    np.testing.assert_array_equal(to_np(st), s)


# ---- kernels against numpy ----------------------------------------------
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("dtype", DTYPES)
def test_gpu_kernels_sizes(dtype, n):
    _run_p(n, dtype)
    _run_s(n, dtype)
    _run_vdot2(n, dtype)
    _run_xr(n, dtype)
    _run_xr(n, dtype, alias=True)


@pytest.mark.parametrize("dtype", DTYPES)
def test_gpu_kernels_misaligned(dtype):
    _run_p(1000, dtype, misalign=True)
    _run_s(1000, dtype, misalign=True)
    _run_vdot2(1000, dtype, misalign=True)
    _run_xr(1000, dtype, misalign=True)


def test_gpu_misaligned_writes_stay_inside_view():
    n = 1000
    x, phat, shat, s, t, rhat = _vecs(n, np.float64, 6)
    sc = _scalars(np.float64)
    bufs = [torch.full((n + 2,), 9.0, dtype=torch.float64, device="cuda")
            for _ in range(2)]
    xt, rt = bufs[0][1:-1], bufs[1][1:-1]
    xt.copy_(torch.from_numpy(x))
    ops.bicgstab_xr(xt, rt, _dev(phat), _dev(shat), _dev(s), _dev(t),
                    _dev(rhat), *_dev_scalars(sc), _dev(np.zeros(2)))
    ops.bicgstab_p(xt, _dev(s), _dev(t), *_dev_scalars(sc))
    ops.bicgstab_s(rt, _dev(s), _dev(t), _dev(sc["rho"]), _dev(sc["rhv"]))
    for b in bufs:
        assert float(b[0]) == 9.0 and float(b[-1]) == 9.0


@pytest.mark.parametrize("dtype", DTYPES)
def test_gpu_zero_denominators(dtype):
    for zero in ("rhv", "ts", "tt"):
        _run_p(1000, dtype, zero=zero)
    _run_s(1000, dtype, zero="rhv")
    for zero in ("rhv", "tt"):
        _run_xr(1000, dtype, zero=zero)


@pytest.mark.parametrize("kernel", ["BICGSTAB_P", "BICGSTAB_S", "VDOT2",
                                    "BICGSTAB_XR"])
@pytest.mark.parametrize("dtype", [np.float64, np.complex64])
def test_gpu_grid_stride_loop(dtype, kernel):
    # past cap * per_block the capped grid has to stride a second time
    n = (getattr(EXT, kernel + "_GRID_CAP")
         * getattr(EXT, kernel + "_PER_BLOCK") + 77)
    {"BICGSTAB_P": _run_p, "BICGSTAB_S": _run_s, "VDOT2": _run_vdot2,
     "BICGSTAB_XR": _run_xr}[kernel](n, dtype)


# ---- the solver ----------------------------------------------------------
def _solve_and_check(A, S, b, **kw):
    rtol = bc.solve_rtol(S.dtype)
    x, info = lsp.linalg.bicgstab(A, b, rtol=rtol, **kw)
    assert x.is_cuda
    res = bc.rel_residual(S, to_np(x), b)
    print(f"{np.dtype(S.dtype).name}: info={info} true residual={res:.3e}")
    assert info == 0
    assert res <= 10 * rtol


@pytest.mark.parametrize("dtype", DTYPES)
def test_gpu_solve_convdiff(dtype):
    A = bc.convdiff_lsp(24, 24, dtype=dtype)
    assert A.data.is_cuda
    S = bc.convdiff(24, 24, dtype=dtype)
    _solve_and_check(A, S, bc.rhs(576, dtype))


@pytest.mark.parametrize("dtype", DTYPES)
def test_gpu_solve_nonaffine(dtype):
    S = bc.nonaffine(dtype)
    _solve_and_check(lsp.csr_array(S), S, bc.rhs(300, dtype),
                     conv_test_iters=5)


def test_gpu_five_step_replay():
    S = bc.convdiff(24, 24)
    b = bc.rhs(576, np.float64)
    x, info = lsp.linalg.bicgstab(bc.convdiff_lsp(24, 24), b, maxiter=5,
                                  conv_test_iters=5, rtol=0)
    want = bc.np_replay(S, b, 5)
    assert info == 5 and x.is_cuda
    err = np.linalg.norm(to_np(x) - want) / np.linalg.norm(want)
    print(f"replay error {err:.3e}")
    assert err <= 1e-10


@pytest.mark.parametrize("dtype", DTYPES)
def test_gpu_solve_jacobi_preconditioner(dtype):
    S = bc.nonaffine(dtype)
    dinv = (1.0 / S.diagonal()).astype(dtype)
    M = lsp.csr_array(sp.csr_array(sp.diags(dinv).tocsr()))
    _solve_and_check(lsp.csr_array(S), S, bc.rhs(300, dtype), M=M,
                     conv_test_iters=5)

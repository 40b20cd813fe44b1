# SPDX-License-Identifier: Apache-2.0
"""GPU numerics of the level-scheduled triangular-solve kernels
(src/hip/sptrsv.hip): every test matrix, both triangles, unit and stored
diagonal, four dtypes, both index types, the narrow and wide lane mappings,
all-wide / all-chain / mixed launch plans and the grid-stride loop
(pytest -m gpu on an MI355X)."""
import functools

import numpy as np
import pytest

import legate_sparse as lsp
from legate_sparse import linalg, ops
from testutils import to_np
import ilu0_cases as ic

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

KS = [1, 2, 4, 5, 8, 32]
EXT = None


@pytest.fixture(scope="module", autouse=True)
def _check_native():
    global EXT
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from legate_sparse import _cext
    # GPU runs MUST use the gfx950 extension — no silent fallback
    EXT = _cext.require_hip()
    assert EXT.SPTRSV_KMAX == ops.SPTRSV_KMAX == 32
    assert EXT.SPTRSV_CHAIN_ROWS == ops.SPTRSV_CHAIN_ROWS
    assert EXT.SPTRSV_GRID_CAP == ops.SPTRSV_GRID_CAP
    yield


@functools.lru_cache(maxsize=None)
def _reference(name, lower, unit, dtype, k):
    A = ic.tri_matrix(name, lower, dtype, unit)
    b = ic.rhs(A.shape[0], k, dtype, seed=k)
    return b, ic.tri_reference(A, b, lower, unit)


def _device_csr(A, idx_dtype):
    """(indptr, indices, vals, diag_pos, schedule) on the GPU."""
    indptr = torch.from_numpy(A.indptr.astype(np.int64)).cuda()
    indices = torch.from_numpy(A.indices.astype(np.int64)).cuda() \
        .to(idx_dtype)
    vals = torch.from_numpy(A.data.copy()).cuda()
    dpos, _ = ops.diag_positions(indptr, indices, A.shape[0])
    return indptr, indices, vals, dpos


def _solve(csr, sched, b, lower, unit, **kw):
    X = torch.from_numpy(b.copy()).cuda()
    ops.sptrsv(*csr, sched, X, lower=lower, unit_diagonal=unit, **kw)
    return X


@pytest.mark.parametrize("dtype", ic.DTYPES)
@pytest.mark.parametrize("lower", [True, False])
@pytest.mark.parametrize("name", ic.TRI_NAMES)
def test_gpu_sptrsv(name, lower, dtype):
    for unit in (False, True):
        A = ic.tri_matrix(name, lower, dtype, unit)
        for idt in (torch.int32, torch.int64):
            csr = _device_csr(A, idt)
            sched = ops.level_schedule(csr[0], csr[1], A.shape[0], lower)
            for k in KS:
                b, want = _reference(name, lower, unit, dtype, k)
                got = to_np(_solve(csr, sched, b, lower, unit))
                err = np.abs(got - want).max()
                print(f"{name} lower={lower} unit={unit} {idt} k={k} "
                      f"{np.dtype(dtype).name}: |err| {err:.3e}")
                np.testing.assert_allclose(got, want, **ic.tol(dtype))


@pytest.mark.parametrize("dtype", [np.float32, np.complex128])
@pytest.mark.parametrize("lower", [True, False])
@pytest.mark.parametrize("name", ["bidiag1000", "twotier5000", "rand300",
                                  "grid33x17", "arrow600"])
def test_gpu_sptrsv_plan_edges(name, lower, dtype):
    """The same solve all-wide (_chain_rows=1 where levels are wider),
    all-chain and mixed, with the grid capped so that a level takes the
    grid-stride loop."""
    A = ic.tri_matrix(name, lower, dtype)
    csr = _device_csr(A, torch.int32)
    sched = ops.level_schedule(csr[0], csr[1], A.shape[0], lower)
    for k in (1, 4, 8):
        b, want = _reference(name, lower, False, dtype, k)
        base = _solve(csr, sched, b, lower, False)
        np.testing.assert_allclose(to_np(base), want, **ic.tol(dtype))
        for chain_rows in (1, 16, None, 10 ** 6):
            for cap in (1, 2, None):
                got = _solve(csr, sched, b, lower, False,
                             _chain_rows=chain_rows, _grid_cap=cap)
                same = torch.equal(got, base)
                print(f"{name} k={k} chain_rows={chain_rows} cap={cap}: "
                      f"launches {sched.n_launches(chain_rows)}, "
                      f"bit-equal to default plan: {same}")
                np.testing.assert_allclose(to_np(got), want, **ic.tol(dtype))
                np.testing.assert_allclose(to_np(got), to_np(base),
                                           **ic.tol(dtype))
    if name == "bidiag1000":
        assert sched.n_launches() == 1
    if name == "twotier5000":
        assert 0 in sched.plan()[:, 0].tolist()
        # several thousand rows in one level, two workgroups: grid-stride
        assert np.diff(sched.level_ptr_host.numpy()).max() > 2 * 256


@pytest.mark.parametrize("k", [1, 4, 32])
def test_gpu_sptrsv_bit_identical(k):
    for name in ("rand300", "dense65", "twotier5000"):
        A = ic.tri_matrix(name, True, np.float64)
        csr = _device_csr(A, torch.int32)
        sched = ops.level_schedule(csr[0], csr[1], A.shape[0], True)
        b, _ = _reference(name, True, False, np.float64, k)
        assert torch.equal(_solve(csr, sched, b, True, False),
                           _solve(csr, sched, b, True, False))


@pytest.mark.parametrize("k", [1, 3, 5, 8])
def test_gpu_sptrsv_column_panel(k):
    """A block that is a column panel of a wider buffer (ld > k): solved in
    place, the other columns untouched."""
    A = ic.tri_matrix("grid33x17", False, np.float64)
    n = A.shape[0]
    csr = _device_csr(A, torch.int32)
    sched = ops.level_schedule(csr[0], csr[1], n, False)
    b = ic.rhs(n, k, np.float64, seed=k)
    want = ic.tri_reference(A, b, False, False)
    buf = torch.full((n, 13), 7.0, dtype=torch.float64, device="cuda")
    buf[:, 3:3 + k] = torch.from_numpy(b).cuda()
    ops.sptrsv(*csr, sched, buf[:, 3:3 + k], lower=False)
    np.testing.assert_allclose(to_np(buf[:, 3:3 + k]), want,
                               **ic.tol(np.float64))
    rest = torch.cat([buf[:, :3], buf[:, 3 + k:]], dim=1)
    assert bool((rest == 7.0).all())


@pytest.mark.parametrize("dtype", ic.DTYPES)
def test_gpu_spsolve_triangular(dtype):
    """The public function on the device: 1-D b, a 40-column block (two
    panels), overwrite_b, the errors."""
    for lower in (True, False):
        A = ic.tri_matrix("rand300", lower, dtype)
        La = lsp.csr_array(A)
        assert La.data.is_cuda
        for k in (None, 40):
            b = ic.rhs(300, k, dtype)
            want = ic.tri_reference(A, b, lower, False)
            got = linalg.spsolve_triangular(La, torch.from_numpy(b).cuda(),
                                            lower=lower)
            assert got.is_cuda and tuple(got.shape) == b.shape
            np.testing.assert_allclose(to_np(got), want, **ic.tol(dtype))
            got = linalg.spsolve_triangular(La, b, lower=lower)  # numpy b
            np.testing.assert_allclose(to_np(got), want, **ic.tol(dtype))
            bt = torch.from_numpy(b.copy()).cuda()
            got = linalg.spsolve_triangular(La, bt, lower=lower,
                                            overwrite_b=True)
            assert got.data_ptr() == bt.data_ptr()
            np.testing.assert_allclose(to_np(bt), want, **ic.tol(dtype))
        with pytest.raises(ValueError):
            linalg.spsolve_triangular(La, b, lower=not lower)
    Z = ic.tri_matrix("rand300", True, dtype).copy()
    Z.data[Z.indptr[9] - 1] = 0
    with pytest.raises(np.linalg.LinAlgError):
        linalg.spsolve_triangular(lsp.csr_array(Z), ic.rhs(300, None, dtype))


def test_gpu_torch_arm():
    """The _impl="torch" arm (the A/B benchmark's arm B) on the device."""
    for lower in (True, False):
        A = ic.tri_matrix("grid33x17", lower, np.float64)
        csr = _device_csr(A, torch.int32)
        sched = ops.level_schedule(csr[0], csr[1], A.shape[0], lower)
        b, want = _reference("grid33x17", lower, False, np.float64, 8)
        got = _solve(csr, sched, b, lower, False, _impl="torch")
        np.testing.assert_allclose(to_np(got), want, **ic.tol(np.float64))

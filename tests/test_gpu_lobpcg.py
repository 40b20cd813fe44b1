# SPDX-License-Identifier: Apache-2.0
"""GPU numerics of the LOBPCG block kernels (src/hip/block_ops.hip) — every
dtype, tile edge, layout and instantiation against numpy — and the solver
end to end on the device (pytest -m gpu on an MI355X)."""
import functools
import warnings

import numpy as np
import pytest
import scipy.sparse as sp

import legate_sparse as lsp
from legate_sparse import ops
from testutils import to_np
import lobpcg_cases as lc
from test_gpu_spmm import _tol

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

DTYPES = [np.float32, np.float64, np.complex64, np.complex128]
NS = [1, 63, 64, 65, 255, 256, 257, 1000]
PQ = [(1, 1), (1, 5), (3, 3), (4, 7), (8, 8), (5, 17), (32, 32)]
# packed: contiguous, 16-byte aligned (the pack instantiation when the row
#   length allows it)
# panel: columns 16.. of a buffer 16 columns wider (ld > cols, rows still
#   aligned: the pack instantiation on a strided panel)
# ragged: columns 1.. of a buffer 3 columns wider (ld > cols, unaligned)
# offset1: contiguous, base pointer one element past the 16-byte grid
LAYOUTS = ["packed", "panel", "ragged", "offset1"]
FILLS = ["exact", "normal"]

_EXT = {}


@pytest.fixture(scope="module", autouse=True)
def _check_native():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from legate_sparse import _cext
    # GPU runs MUST use the gfx950 extension — no silent fallback
    ext = _cext.require_hip()
    for kern in ("GRAM", "UPDATE", "RESIDUAL"):
        assert getattr(ext, f"BLOCK_{kern}_GRID_CAP") > 0
        assert getattr(ext, f"BLOCK_{kern}_PER_BLOCK") > 0
    assert ext.BLOCK_KMAX == ops.BLOCK_KMAX == 32
    _EXT["ext"] = ext
    yield


@functools.lru_cache(maxsize=None)
def _host(n, cols, dtype_name, fill, seed):
    """Host block, computed once and never modified.  'exact': entries in
    {-1, 0, 1} (both parts), so every sum of the tests stays an integer
    below 2^24.  'normal': N(0, 1)."""
    dtype = np.dtype(dtype_name)
    rng = np.random.default_rng(1000 * seed + 31 * cols + n % 997)
    draw = (lambda: rng.integers(-1, 2, size=(n, cols)).astype(np.float64)) \
        if fill == "exact" else (lambda: rng.standard_normal((n, cols)))
    a = draw()
    if dtype.kind == "c":
        a = a + 1j * draw()
    a = a.astype(dtype)
    a.setflags(write=False)
    return a


def _coef(p, q, dtype, fill, seed):
    rng = np.random.default_rng(77 * seed + 5 * p + q)
    if fill == "exact":
        c = rng.integers(-2, 3, size=(p, q)).astype(np.float64)
        if np.dtype(dtype).kind == "c":
            c = c + 1j * rng.integers(-2, 3, size=(p, q))
    else:
        c = rng.standard_normal((p, q))
        if np.dtype(dtype).kind == "c":
            c = c + 1j * rng.standard_normal((p, q))
    return c.astype(dtype)


def _dev(a, layout):
    """Device view holding ``a`` in the given layout."""
    n, cols = a.shape
    t = torch.from_numpy(np.array(a)).cuda()
    if layout == "packed":
        return t
    if layout in ("panel", "ragged"):
        off, extra = (16, 16) if layout == "panel" else (1, 3)
        wide = torch.full((n, cols + extra), 7, dtype=t.dtype, device="cuda")
        view = wide[:, off:off + cols]
        view.copy_(t)
        return view
    flat = torch.empty(n * cols + 1, dtype=t.dtype, device="cuda")
    view = flat[1:].view(n, cols)
    view.copy_(t)
    return view


def _compare(got, want, dtype, fill):
    if fill == "exact":
        np.testing.assert_array_equal(got, want.astype(got.dtype))
    else:
        np.testing.assert_allclose(got, want, **_tol(dtype))


def _wide(a):
    return a.astype(np.complex128 if a.dtype.kind == "c" else np.float64)


@pytest.mark.parametrize("fill", FILLS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_gpu_block_gram(dtype, fill):
    name = np.dtype(dtype).name
    for n in NS:
        for p, q in PQ:
            X, Y = _host(n, p, name, fill, 1), _host(n, q, name, fill, 2)
            want = _wide(X).conj().T @ _wide(Y)
            want_t = _wide(X).T @ _wide(Y)
            for layout in LAYOUTS:
                Xd, Yd = _dev(X, layout), _dev(Y, layout)
                G = ops.block_gram(Xd, Yd)
                assert G.is_cuda and tuple(G.shape) == (p, q)
                _compare(to_np(G), want, dtype, fill)
            _compare(to_np(ops.block_gram(_dev(X, "packed"),
                                          _dev(Y, "ragged"), conj=False)),
                     want_t, dtype, fill)
    # X^H X with one operand passed twice, and n = 0
    Xd = _dev(_host(257, 8, name, fill, 1), "packed")
    _compare(to_np(ops.block_gram(Xd, Xd)),
             _wide(to_np(Xd)).conj().T @ _wide(to_np(Xd)), dtype, fill)
    E = torch.empty((0, 3), dtype=Xd.dtype, device="cuda")
    assert not to_np(ops.block_gram(E, E)).any()


@pytest.mark.parametrize("fill", FILLS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_gpu_block_update(dtype, fill):
    name = np.dtype(dtype).name
    for n in NS:
        for p, q in PQ:
            # three terms of widths p, q and q (all whole packs when p and
            # q are); one term of width p
            widths = [p, q, q]
            Xs = [_host(n, w, name, fill, 3 + i) for i, w in enumerate(widths)]
            Cs = [_coef(w, q, dtype, fill, i) for i, w in enumerate(widths)]
            Z0 = _host(n, q, name, fill, 9)
            for nterms in (3, 1):
                prod = sum(_wide(x) @ _wide(c)
                           for x, c in zip(Xs[:nterms], Cs[:nterms]))
                for layout in LAYOUTS:
                    for acc in (False, True):
                        Zd = _dev(Z0, layout)
                        terms = [(_dev(x, layout), torch.from_numpy(c).cuda())
                                 for x, c in zip(Xs[:nterms], Cs[:nterms])]
                        out = ops.block_update(Zd, terms, accumulate=acc)
                        assert out is Zd
                        _compare(to_np(Zd),
                                 prod + _wide(Z0) if acc else prod,
                                 dtype, fill)
    # Z is X_0 itself (square coefficient), with and without accumulate,
    # and a panel layout whose untouched columns must stay untouched
    for acc in (False, True):
        X = _host(257, 8, name, fill, 3)
        C = _coef(8, 8, dtype, fill, 4)
        Xd = _dev(X, "panel")
        ops.block_update(Xd, [(Xd, torch.from_numpy(C).cuda())],
                         accumulate=acc)
        want = _wide(X) @ _wide(C) + (_wide(X) if acc else 0)
        _compare(to_np(Xd), want, dtype, fill)
        wide = Xd._base if Xd._base is not None else Xd
        assert (to_np(wide)[:, :16] == 7).all()
    Z = torch.empty((0, 3), dtype=Xd.dtype, device="cuda")
    ops.block_update(Z, [(Z, torch.zeros((3, 3), dtype=Z.dtype,
                                         device="cuda"))])


@pytest.mark.parametrize("fill", FILLS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_gpu_block_residual(dtype, fill):
    name = np.dtype(dtype).name
    rdt = np.zeros(0, dtype=dtype).real.dtype
    for n in NS:
        for k in sorted({p for p, _ in PQ} | {q for _, q in PQ}):
            AX, X = _host(n, k, name, fill, 5), _host(n, k, name, fill, 6)
            th = _coef(1, k, rdt, fill, 8).reshape(k)
            want = _wide(AX) - _wide(X) * th.astype(np.float64)[None, :]
            # re^2 + im^2, not abs()^2: hypot rounds, the integers do not
            want_n = (want.real ** 2 + want.imag ** 2).sum(axis=0)
            for layout in LAYOUTS:
                R = _dev(np.zeros((n, k), dtype=dtype), layout)
                nrm = ops.block_residual(R, _dev(AX, layout), _dev(X, layout),
                                         torch.from_numpy(th).cuda())
                assert nrm.is_cuda and nrm.dtype == getattr(torch, rdt.name)
                _compare(to_np(R), want, dtype, fill)
                if fill == "exact":
                    np.testing.assert_array_equal(to_np(nrm),
                                                  want_n.astype(rdt))
                else:
                    np.testing.assert_allclose(to_np(nrm), want_n,
                                               rtol=_tol(dtype)["rtol"])
    E = torch.empty((0, 3), dtype=getattr(torch, np.dtype(dtype).name),
                    device="cuda")
    nrm = ops.block_residual(E.clone(), E, E,
                             torch.zeros(3, dtype=getattr(torch, rdt.name),
                                         device="cuda"))
    assert not to_np(nrm).any()


# ---- one more row than GRID_CAP * PER_BLOCK: the grid-stride loop --------
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_gpu_block_gram_grid_stride(dtype):
    ext = _EXT["ext"]
    n = ext.BLOCK_GRAM_GRID_CAP * ext.BLOCK_GRAM_PER_BLOCK + 1
    name = np.dtype(dtype).name
    X, Y = _host(n, 2, name, "exact", 1), _host(n, 2, name, "exact", 2)
    G = ops.block_gram(_dev(X, "packed"), _dev(Y, "packed"))
    np.testing.assert_array_equal(to_np(G),
                                  (_wide(X).T @ _wide(Y)).astype(dtype))


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_gpu_block_update_grid_stride(dtype):
    ext = _EXT["ext"]
    n = ext.BLOCK_UPDATE_GRID_CAP * ext.BLOCK_UPDATE_PER_BLOCK + 1
    name = np.dtype(dtype).name
    X, Y = _host(n, 2, name, "exact", 1), _host(n, 1, name, "exact", 2)
    C, D = _coef(2, 2, dtype, "exact", 1), _coef(1, 2, dtype, "exact", 2)
    Z = _dev(np.zeros((n, 2), dtype=dtype), "packed")
    ops.block_update(Z, [(_dev(X, "packed"), torch.from_numpy(C).cuda()),
                         (_dev(Y, "packed"), torch.from_numpy(D).cuda())])
    np.testing.assert_array_equal(
        to_np(Z), (_wide(X) @ _wide(C) + _wide(Y) @ _wide(D)).astype(dtype))


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_gpu_block_residual_grid_stride(dtype):
    ext = _EXT["ext"]
    n = ext.BLOCK_RESIDUAL_GRID_CAP * ext.BLOCK_RESIDUAL_PER_BLOCK + 1
    name = np.dtype(dtype).name
    AX, X = _host(n, 2, name, "exact", 5), _host(n, 2, name, "exact", 6)
    th = np.array([1, -1], dtype=dtype)
    R = _dev(np.zeros((n, 2), dtype=dtype), "packed")
    nrm = ops.block_residual(R, _dev(AX, "packed"), _dev(X, "packed"),
                             torch.from_numpy(th).cuda())
    want = _wide(AX) - _wide(X) * th[None, :]
    np.testing.assert_array_equal(to_np(R), want.astype(dtype))
    np.testing.assert_array_equal(to_np(nrm),
                                  (want ** 2).sum(axis=0).astype(dtype))


# ---- reproducibility: same input, same bits -------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_gpu_block_reductions_bit_identical(dtype):
    name = np.dtype(dtype).name
    rdt = np.zeros(0, dtype=dtype).real.dtype
    n = 300_001
    X = _dev(_host(n, 8, name, "normal", 1), "packed")
    Y = _dev(_host(n, 5, name, "normal", 2), "packed")
    g1, g2 = to_np(ops.block_gram(X, Y)), to_np(ops.block_gram(X, Y))
    np.testing.assert_array_equal(g1, g2)
    AX = _dev(_host(n, 8, name, "normal", 3), "packed")
    th = torch.from_numpy(np.linspace(-1, 2, 8).astype(rdt)).cuda()
    R = torch.empty_like(X)
    n1 = to_np(ops.block_residual(R, AX, X, th))
    n2 = to_np(ops.block_residual(R, AX, X, th))
    np.testing.assert_array_equal(n1, n2)


# ---- the solver on the device ----------------------------------------------
def _solver_params():
    for case in ("poisson", "hermitian", "diagdom_jacobi"):
        ks, whichs, tols = lc.CASES[case]
        for dtype, tol in tols.items():
            if case == "diagdom_jacobi" and dtype != np.float64:
                continue
            for k in ks:
                for which in whichs:
                    yield pytest.param(
                        case, np.dtype(dtype), tol, k, which == "largest",
                        id=f"{case}-{np.dtype(dtype).name}-k{k}-{which}")


@pytest.mark.parametrize("case,dtype,tol,k,largest", list(_solver_params()))
def test_gpu_lobpcg(case, dtype, tol, k, largest):
    S, M, exact = lc.matrix(case)
    A = lsp.csr_array(sp.csr_array(S.astype(dtype)))
    Ml = None if M is None else lsp.csr_array(sp.csr_array(M.astype(dtype)))
    X = lc.start_block(S.shape[0], k, dtype, 0)
    budget = 2 * lc.scipy_iterations(case, k, largest, dtype.name, tol, 0) + 10
    with warnings.catch_warnings():
        warnings.simplefilter("error")                  # (a)
        w, V, hist = lsp.linalg.lobpcg(
            A, torch.from_numpy(X).cuda(), M=Ml, tol=tol, maxiter=budget,
            largest=largest, retResidualNormsHistory=True)
    assert V.is_cuda and isinstance(w, np.ndarray)
    print(f"{lc.iterations(hist)} iterations (budget {budget})")
    lc.check_pairs(S, exact, w, to_np(V), k, largest, tol)   # (b)-(d)

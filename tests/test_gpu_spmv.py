# SPDX-License-Identifier: Apache-2.0
"""GPU numerics of the general CSR SpMV kernels (src/hip/spmv.hip: vector,
pair, pair2, sten, pairu, stream and the launcher that picks among them)
against the exact and high-precision oracles of spmv_cases.py
(pytest -m gpu on an MI355X).

Every call states which kernel it expects and checks it against the
extension's ``spmv_select``, so a test cannot drift onto another kernel
without failing."""
import os
import subprocess
import sys

import numpy as np
import pytest
import scipy.sparse as sp

import legate_sparse as lsp
import spmv_cases as sc
from legate_sparse import ops
from testutils import to_np

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

CODE = {"float32": 0, "float64": 1, "complex64": 2, "complex128": 3}
OFF = sc.COL_OFFSET


@pytest.fixture(scope="module", autouse=True)
def _check_native():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from legate_sparse import _cext
    # GPU runs MUST use the gfx950 extension — no silent fallback
    _cext.require_hip()
    yield


def _ext():
    from legate_sparse import _cext
    return _cext.require_hip()


# ---------------------------------------------------------------------------
# device operands and host references, each made once and left unchanged
# ---------------------------------------------------------------------------
_DEV = {}
_REF = {}


def _dev(key, make):
    if key not in _DEV:
        _DEV[key] = torch.from_numpy(np.array(make())).cuda()
    return _DEV[key]


def _structure(case, idx):
    ip = _dev((case.name, "indptr"), lambda: case.S.indptr.astype(np.int64))
    ix = _dev((case.name, "indices", np.dtype(idx).name),
              lambda: case.S.indices.astype(idx))
    return ip, ix


def _values(case, f, dtype):
    k = (case.name, f.kind, np.dtype(dtype).name)
    return (_dev(k + ("vals",), lambda: f.vals),
            _dev(k + ("x",), lambda: f.x),
            _dev(k + ("y0",), lambda: f.y0))


def _want(case, kind, dtype, acc):
    key = (case.name, kind, np.dtype(dtype).name, acc)
    if key not in _REF:
        f = sc.fill(case, kind, dtype)
        if kind == "exact":
            _REF[key] = sc.exact_oracle(case, f.vals, f.x, f.y0, acc)
        else:
            _REF[key] = sc.reference(case, f.vals, f.x, f.y0, acc)
    return _REF[key]


def _launch(ip, ix, vals, x, y0, acc, cfg, max_nnz=-1, col_offset=0):
    """One ops.spmv call into a fresh copy of y0 (so a kernel that fails to
    overwrite shows)."""
    y = y0.clone()
    out = ops.spmv(ip, ix, vals, x, y, accumulate=acc,
                   w_override=cfg.w_override, nt=cfg.nt, pair=cfg.pair,
                   swz=cfg.swz, col_offset=col_offset, max_nnz=max_nnz)
    assert out is y
    return y


AUTO = sc.Config("auto", -1, 0, False, 0, None, False)


def _selected(case, dtype, acc, cfg, max_nnz=-1):
    return _ext().spmv_select(case.lens.size, case.S.nnz,
                              CODE[np.dtype(dtype).name], acc,
                              cfg.w_override, cfg.nt, cfg.pair, cfg.swz,
                              max_nnz)


def _check_case(case, cfg, dtype, idx, acc, expect, max_nnz=-1):
    """Exact fill, normal fill and run-to-run equality of one launch
    configuration on one matrix."""
    what = (f"{case.name} {cfg.name} {np.dtype(dtype).name} "
            f"{np.dtype(idx).name} acc={acc} max_nnz={max_nnz}")
    assert _selected(case, dtype, acc, cfg, max_nnz) == expect, what
    ip, ix = _structure(case, idx)
    fe = sc.fill(case, "exact", dtype)
    y = _launch(ip, ix, *_values(case, fe, dtype), acc, cfg, max_nnz)
    sc.check_exact(to_np(y), _want(case, "exact", dtype, acc), what)
    fn = sc.fill(case, "normal", dtype)
    ops_n = _values(case, fn, dtype)
    y1 = _launch(ip, ix, *ops_n, acc, cfg, max_nnz)
    ref, scale = _want(case, "normal", dtype, acc)
    sc.check_bound(case, to_np(y1), ref, scale, what)
    if expect[0] != "stream":
        # stream adds the pieces of a row that spans element blocks with
        # atomics, in whatever order the blocks arrive: exempt.  Every other
        # kernel has one fixed summation order per row.
        y2 = _launch(ip, ix, *ops_n, acc, cfg, max_nnz)
        assert torch.equal(y1, y2), what + ": two runs differ"


def _dtypes_of(cfg):
    return sc.REAL_DTYPES if cfg.real_only else sc.DTYPES


# ---------------------------------------------------------------------------
# explicit variants
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("cfg_name", [c.name for c in sc.CONFIGS])
def test_gpu_spmv_explicit_variant(cfg_name):
    cfg = sc.CONFIG_BY_NAME[cfg_name]
    n = 0
    for name in sc.case_names():
        case = sc.get_case(name)
        if not sc.fits(cfg, case):
            continue
        for dtype in _dtypes_of(cfg):
            real = np.dtype(dtype).kind == "f"
            for acc in (False, True):
                expect = sc.expected_kernel(cfg, case, real, acc)
                for idx in sc.IDX_DTYPES:
                    _check_case(case, cfg, dtype, idx, acc, expect)
                    n += 1
    assert n >= 8 * 8  # at least eight matrices per configuration


POISON_CASES = ["uniform1even", "uniform2odd", "uniform7odd", "uniform8even",
                "uniform15odd", "uniform16even", "uniform31odd",
                "uniform64even", "ragged", "long_row", "sparse_tail"]


@pytest.mark.parametrize("cfg_name", [c.name for c in sc.CONFIGS] + ["auto"])
def test_gpu_spmv_nan_containment(cfg_name):
    """NaN in a stored value next to a row boundary and in one x entry:
    exactly the owning rows become NaN.  A kernel that masks by multiplying
    with zero instead of the ``pp >= s`` / ``pp + 1 < e`` guards spreads it
    to the neighbouring row."""
    cfg = AUTO if cfg_name == "auto" else sc.CONFIG_BY_NAME[cfg_name]
    n = 0
    for name in POISON_CASES:
        case = sc.get_case(name)
        if not sc.fits(cfg, case):
            continue
        mx = sc.max_len(case) if cfg is AUTO else -1
        for dtype in _dtypes_of(cfg):
            f = sc.fill(case, "exact", dtype)
            p = sc.poison(case, f.vals, f.x)
            assert p is not None
            pv = torch.from_numpy(p.vals).cuda()
            px = torch.from_numpy(p.x).cuda()
            _, _, y0 = _values(case, f, dtype)
            for idx in sc.IDX_DTYPES:
                ip, ix = _structure(case, idx)
                for acc in (False, True):
                    y = _launch(ip, ix, pv, px, y0, acc, cfg, mx)
                    sc.check_poison(
                        case, to_np(y), p, _want(case, "exact", dtype, acc),
                        f"{name} {cfg.name} {np.dtype(dtype).name} "
                        f"{np.dtype(idx).name} acc={acc}")
                    n += 1
    assert n >= 3 * 8


# ---------------------------------------------------------------------------
# operand placement: column window, storage offset, odd-offset views
# ---------------------------------------------------------------------------
def _odd_view(t):
    """The same elements as a contiguous view that starts one element into
    a larger buffer, as ``tensor[1:]`` produces: pair loads then sit on
    8-byte (fp64, int64), 4-byte (fp32, int32) boundaries instead of 16 / 8.
    gfx950 global loads permit that, and the pair kernels rely on it for
    any CSR piece cut out of a larger one."""
    v = torch.cat([t.new_zeros(1), t])[1:]
    assert v.is_contiguous() and v.storage_offset() == 1
    assert v.data_ptr() % (2 * v.element_size()) == v.element_size()
    return v


@pytest.mark.parametrize("cfg_name", [c.name for c in sc.CONFIGS])
def test_gpu_spmv_windows_and_views(cfg_name):
    cfg = sc.CONFIG_BY_NAME[cfg_name]
    for name in ("uniform7odd", "uniform7even", "ragged"):
        case = sc.get_case(name)
        if not sc.fits(cfg, case):
            continue
        for dtype in _dtypes_of(cfg):
            f = sc.fill(case, "exact", dtype)
            vals, x, y0 = _values(case, f, dtype)
            junk = x.new_full((40,), 7)
            x_mid = torch.cat([junk, x, junk[:7]])[40:40 + x.numel()]
            assert x_mid.storage_offset() == 40 and x_mid.is_contiguous()
            for idx in sc.IDX_DTYPES:
                ip, ix = _structure(case, idx)
                ix_off = ix + OFF
                for acc in (False, True):
                    want = _want(case, "exact", dtype, acc)
                    what = (f"{name} {cfg.name} {np.dtype(dtype).name} "
                            f"{np.dtype(idx).name} acc={acc} ")
                    # global columns c in [13, 13 + n_cols), x holds the
                    # window: the kernel reads x[c - 13]
                    y = _launch(ip, ix_off, vals, x, y0, acc, cfg,
                                col_offset=OFF)
                    sc.check_exact(to_np(y), want, what + "col_offset")
                    # the same window cut from the middle of a longer x
                    y = _launch(ip, ix_off, vals, x_mid, y0, acc, cfg,
                                col_offset=OFF)
                    sc.check_exact(to_np(y), want, what + "x window")
                    y = _launch(ip, _odd_view(ix), _odd_view(vals),
                                _odd_view(x), y0, acc, cfg)
                    sc.check_exact(to_np(y), want, what + "odd views")


# ---------------------------------------------------------------------------
# XCD swizzle where the block count is no multiple of 8
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("nb", [1, 7, 8, 9, 13])
def test_gpu_spmv_swizzle_block_counts(nb):
    for w in (4, 64):
        rpb = 256 // w
        n_rows = nb * rpb - (1 if rpb == 4 else 5)
        assert (n_rows + rpb - 1) // rpb == nb  # the grid of the launch
        lens = np.random.default_rng(500 + nb + w).integers(0, 21, n_rows)
        case = sc.from_lens(f"swz_nb{nb}_w{w}", lens, sc.N_COLS,
                            seed=600 + nb + w)
        for cfg_name in (f"vector_swz_w{w}", f"pair_swz_w{w}"):
            cfg = sc.CONFIG_BY_NAME[cfg_name]
            for dtype in _dtypes_of(cfg):
                real = np.dtype(dtype).kind == "f"
                for acc in (False, True):
                    expect = sc.expected_kernel(cfg, case, real, acc)
                    assert expect == (cfg_name[:-len(f"_w{w}")], w)
                    for idx in sc.IDX_DTYPES:
                        _check_case(case, cfg, dtype, idx, acc, expect)


# ---------------------------------------------------------------------------
# automatic dispatch, with and without the row-length hint
# ---------------------------------------------------------------------------
_SEEN = set()       # (kernel, W, value dtype, index dtype) run by auto
_AUTO_DONE = set()


def _auto_case(name):
    if name in _AUTO_DONE:
        return
    case = sc.get_case(name)
    for dtype in sc.DTYPES:
        real = np.dtype(dtype).kind == "f"
        # the true maximum (csr_array passes it) and -1 (direct ops.spmv
        # callers and the distributed pieces without a hint)
        for mx in (sc.max_len(case), -1):
            expect = sc.expected_auto(case, real, mx)
            for idx in sc.IDX_DTYPES:
                for acc in (False, True):
                    _check_case(case, AUTO, dtype, idx, acc, expect, mx)
                _SEEN.add(expect + (np.dtype(dtype).name,
                                    np.dtype(idx).name))
    _AUTO_DONE.add(name)


@pytest.mark.parametrize("name", sc.case_names())
def test_gpu_spmv_auto_dispatch(name):
    _auto_case(name)


# ---------------------------------------------------------------------------
# the public route: csr_array @ x and lsp.spmv
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("L", sc.UNIFORM_L)
def test_gpu_spmv_public_route(L):
    """_max_row_nnz -> max_nnz -> kernel, end to end: the matrices are not
    affine, so the product must run the general kernel that the launcher
    picks for max_nnz = L."""
    for parity in ("odd", "even"):
        case = sc.get_case(f"uniform{L}{parity}")
        for dtype in sc.DTYPES:
            real = np.dtype(dtype).kind == "f"
            for kind in ("exact", "normal"):
                f = sc.fill(case, kind, dtype)
                S = sp.csr_array(
                    (f.vals.copy(), case.S.indices, case.S.indptr),
                    shape=case.S.shape)
                A = lsp.csr_array(S)
                assert A.data.is_cuda
                assert to_np(A.data).dtype == np.dtype(dtype)
                assert A._affine_plan() is None
                assert A._max_row_nnz() == L
                expect = sc.expected_auto(case, real, L)
                assert _selected(case, dtype, False, AUTO, L) == expect
                idx = to_np(A._indices).dtype
                _SEEN.add(expect + (np.dtype(dtype).name, idx.name))
                x = torch.from_numpy(f.x.copy()).cuda()
                y_mat = to_np(A @ x)
                y_pre = torch.from_numpy(f.y0.copy()).cuda()
                out = lsp.spmv(A, x, y_pre)
                assert out.data_ptr() == y_pre.data_ptr()
                what = f"{case.name} {np.dtype(dtype).name} {kind}"
                for got in (y_mat, to_np(y_pre)):
                    if kind == "exact":
                        sc.check_exact(got, _want(case, kind, dtype, False),
                                       what)
                    else:
                        ref, scale = _want(case, kind, dtype, False)
                        sc.check_bound(case, got, ref, scale, what)


def test_gpu_sum_axis1_into_host_out():
    """sum(axis=1) is a ones-matvec through ops.spmv, which writes through
    a raw pointer: a host ``out`` for a GPU matrix must be filled by a copy,
    never handed to the kernel."""
    case = sc.get_case("uniform7odd")
    f = sc.fill(case, "exact", np.float64)
    A = lsp.csr_array(sp.csr_array(
        (f.vals.copy(), case.S.indices, case.S.indptr), shape=case.S.shape))
    assert A.data.is_cuda
    want = sc.seg_sum(f.vals, case.S.indptr)
    out_host = torch.zeros(sc.N_ROWS, dtype=torch.float64)
    assert A.sum(axis=1, out=out_host) is out_host
    np.testing.assert_array_equal(out_host.numpy(), want)
    out_dev = torch.zeros(sc.N_ROWS, dtype=torch.float64, device="cuda")
    assert A.sum(axis=1, out=out_dev) is out_dev
    np.testing.assert_array_equal(to_np(out_dev), want)


# ---------------------------------------------------------------------------
# grid-stride loops
# ---------------------------------------------------------------------------
def test_gpu_spmv_grid_stride_loops():
    """LS_SPMV_GRID is read once per process, so a fresh child runs the
    explicit table under a cap of 3 blocks: at 777 rows every kernel's row
    loop then takes many steps.  One child, no retry."""
    worker = os.path.join(os.path.dirname(os.path.abspath(__file__)),
                          "spmv_gridcap_worker.py")
    env = dict(os.environ, LS_SPMV_GRID="3")
    # start-up of torch and the GPU dominates; the launches take a second
    res = subprocess.run([sys.executable, worker], env=env, timeout=180,
                         capture_output=True, text=True)
    assert res.returncode == 0, res.stdout[-4000:] + res.stderr[-4000:]
    ok = [ln for ln in res.stdout.splitlines() if ln.startswith("OK ")]
    want = sum(len([c for c in sc.CONFIGS if sc.fits(c, case)])
               for case in (sc.get_case("ragged"),
                            sc.uniform(5, "odd"), sc.uniform(5, "even")))
    assert len(ok) == want, res.stdout[-4000:]
    assert "GRIDCAP_DONE" in res.stdout


# ---------------------------------------------------------------------------
# coverage of the launcher's defaults (kept last in the file)
# ---------------------------------------------------------------------------
def test_gpu_spmv_auto_reaches_every_default_instantiation():
    """Every (kernel, W) that pair=-1, w_override=0 can select, for every
    value and index dtype, was run and checked above.  Listed explicitly: a
    launcher change that adds, drops or renames a default shows here."""
    for name in sc.case_names():
        _auto_case(name)  # no-op for what already ran in this session
    real = [("sten", 4), ("pairu", 2), ("pairu", 4), ("vector", 1),
            ("pair", 1), ("pair", 2), ("pair", 4), ("pair", 8),
            ("pair", 16), ("pair", 32), ("pair", 64)]
    cplx = [("vector", 1), ("vector", 2), ("vector", 4), ("vector", 8),
            ("vector", 16), ("vector", 32), ("vector", 64)]
    want = set()
    for idx in ("int32", "int64"):
        want |= {k + (d, idx) for k in real for d in ("float32", "float64")}
        want |= {k + (d, idx) for k in cplx
                 for d in ("complex64", "complex128")}
    assert len(want) == 72
    assert want - _SEEN == set()
    assert _SEEN - want == set()

# SPDX-License-Identifier: Apache-2.0
"""The general-SpMV cases, fills, oracles and configuration table of
spmv_cases.py, proven on the host: every matrix goes through ops.spmv on
CPU tensors (the C++ extension and the torch route) and is held to the
same exact / bounded / NaN-containment checks that test_gpu_spmv.py
applies to the HIP kernels."""
import numpy as np
import pytest

import spmv_cases as sc
from legate_sparse import _cext, ops
from legate_sparse.csr import _build_affine_plan

torch = pytest.importorskip("torch")

OFF = sc.COL_OFFSET


def _tensors(case, f, idx_dtype, col_offset):
    S = case.S
    return (torch.from_numpy(S.indptr.astype(np.int64)),
            torch.from_numpy(S.indices.astype(idx_dtype) + col_offset),
            torch.from_numpy(f.vals.copy()), torch.from_numpy(f.x.copy()))


def _run(indptr, indices, vals, x, y0, accumulate, col_offset):
    y = torch.from_numpy(y0.copy())
    out = ops.spmv(indptr, indices, vals, x, y, accumulate=accumulate,
                   col_offset=col_offset)
    assert out is y
    return y.numpy()


def _routes(monkeypatch):
    """The CPU extension, then the torch route (CPU tensors reach it only
    without the extension; LS_FORCE_FALLBACK selects the same code for GPU
    tensors)."""
    assert _cext.has_cpu()
    yield "ext"
    with monkeypatch.context() as m:
        m.setattr(_cext, "has_cpu", lambda: False)
        yield "torch"


@pytest.mark.parametrize("name", sc.case_names())
def test_case_is_not_affine(name):
    case = sc.get_case(name)
    S = case.S
    assert S.has_sorted_indices and S.shape[0] == case.lens.size
    np.testing.assert_array_equal(np.diff(S.indptr), case.lens)
    for i in range(S.shape[0]):
        row = S.indices[S.indptr[i]:S.indptr[i + 1]]
        assert np.all(np.diff(row) > 0)
    if case.lone_col is not None:
        assert np.count_nonzero(S.indices == case.lone_col) == 1
    for idx in sc.IDX_DTYPES:
        plan = _build_affine_plan(
            torch.from_numpy(S.indptr.astype(np.int64)),
            torch.from_numpy(S.indices.astype(idx)), max(S.shape))
        assert plan is None


def test_case_shapes_hold_what_they_claim():
    for L in sc.UNIFORM_L:
        odd, even = (sc.get_case(f"uniform{L}{p}") for p in ("odd", "even"))
        assert odd.S.nnz % 2 == 1 and even.S.nnz % 2 == 0
        for c in (odd, even):
            assert c.S.shape == (sc.N_ROWS, sc.N_COLS)
            assert sc.max_len(c) == L == c.L
            # row starts of both parities
            assert {int(s) % 2 for s in c.S.indptr[:-1]} == {0, 1}
    r = sc.get_case("ragged")
    for i in (0, sc.N_ROWS - 1, 100, 101, 102, 103, 63, 64, 255, 256):
        assert r.lens[i] == 0
    assert r.lens.max() == 300 and np.count_nonzero(r.lens > 64) >= 3
    lr = sc.get_case("long_row")
    s, e = int(lr.S.indptr[300]), int(lr.S.indptr[301])
    assert e - s == 5000 and s // 2048 + 2 <= (e - 1) // 2048
    st = sc.get_case("sparse_tail")
    assert st.S.nnz / sc.N_ROWS < 3 and sc.max_len(st) > 31
    assert sc.get_case("rows0").S.shape[0] == 0
    assert sc.get_case("empty300").S.nnz == 0
    assert sc.get_case("one_by_one").S.nnz == 1


def test_table_respects_capacities():
    assert sc.PAIR_CAPACITY == {5: 7, 6: 15, 7: 15, 8: 31}
    assert len({c.name for c in sc.CONFIGS}) == len(sc.CONFIGS)
    for cfg in sc.CONFIGS:
        assert cfg.cap == sc.PAIR_CAPACITY.get(cfg.pair)
        assert cfg.real_only == (cfg.pair != 0)
    for name in sc.case_names():
        case = sc.get_case(name)
        for cfg in sc.configs_for(case):
            assert cfg.cap is None or sc.max_len(case) <= cfg.cap
    # every bounded kernel meets rows of exactly its capacity
    assert sc.CONFIG_BY_NAME["sten_np4"] in sc.configs_for(
        sc.get_case("uniform7odd"))
    assert sc.CONFIG_BY_NAME["pairu_w4"] in sc.configs_for(
        sc.get_case("uniform31even"))
    assert sc.CONFIG_BY_NAME["pairu_w4"] not in sc.configs_for(
        sc.get_case("uniform32odd"))


def test_select_agrees_with_table():
    """The launcher's selection, exported by the HIP extension (a host
    function: no GPU involved), against the table's statement of it."""
    if not _cext.has_hip():
        pytest.skip("HIP extension not built")
    ext = _cext.require_hip()
    for name in sc.case_names():
        case = sc.get_case(name)
        n, nnz = case.lens.size, case.S.nnz
        for code in range(4):
            real = code < 2
            for acc in (False, True):
                for cfg in sc.configs_for(case):
                    got = ext.spmv_select(n, nnz, code, acc, cfg.w_override,
                                          cfg.nt, cfg.pair, cfg.swz, -1)
                    assert got == sc.expected_kernel(cfg, case, real, acc), \
                        (name, code, acc, cfg.name)
                for mx in (-1, sc.max_len(case)):
                    got = ext.spmv_select(n, nnz, code, acc, 0, False, -1,
                                          0, mx)
                    assert got == sc.expected_auto(case, real, mx), \
                        (name, code, acc, mx)
    # a width that is no power of two <= 64 runs as 64
    for w in (3, 48, 65, 128):
        assert ext.spmv_select(777, 7770, 1, False, w, False, 0, 0, -1) == \
            ("vector", 64)


@pytest.mark.parametrize("name", sc.case_names())
def test_cpu_spmv_exact_and_bounded(monkeypatch, name):
    case = sc.get_case(name)
    for route in _routes(monkeypatch):
        for dtype in sc.DTYPES:
            fe = sc.fill(case, "exact", dtype)
            fn = sc.fill(case, "normal", dtype)
            for acc in (False, True):
                want = sc.exact_oracle(case, fe.vals, fe.x, fe.y0, acc)
                ref, scale = sc.reference(case, fn.vals, fn.x, fn.y0, acc)
                for idx in sc.IDX_DTYPES:
                    for off in (0, OFF):
                        what = (f"{name} {route} {np.dtype(dtype).name} "
                                f"{np.dtype(idx).name} acc={acc} off={off}")
                        t = _tensors(case, fe, idx, off)
                        sc.check_exact(_run(*t, fe.y0, acc, off), want, what)
                        t = _tensors(case, fn, idx, off)
                        sc.check_bound(case, _run(*t, fn.y0, acc, off), ref,
                                       scale, what)


@pytest.mark.parametrize("name", ["uniform1even", "uniform2odd",
                                  "uniform7odd", "uniform16even", "ragged",
                                  "long_row", "sparse_tail"])
def test_cpu_spmv_nan_containment(monkeypatch, name):
    case = sc.get_case(name)
    for route in _routes(monkeypatch):
        for dtype in sc.DTYPES:
            f = sc.fill(case, "exact", dtype)
            p = sc.poison(case, f.vals, f.x)
            assert p is not None
            assert not set(p.nan_rows) & set(p.clean_rows)
            want = sc.exact_oracle(case, f.vals, f.x, f.y0, True)
            indptr, indices, _, _ = _tensors(case, f, np.int32, 0)
            got = _run(indptr, indices, torch.from_numpy(p.vals),
                       torch.from_numpy(p.x), f.y0, True, 0)
            sc.check_poison(case, got, p, want,
                            f"{name} {route} {np.dtype(dtype).name}")


def test_every_testable_case_can_be_poisoned():
    for name in sc.case_names():
        case = sc.get_case(name)
        f = sc.fill(case, "exact", np.float32)
        p = sc.poison(case, f.vals, f.x)
        if case.lens.size >= 300 and case.S.nnz:
            assert p is not None, name


def test_checks_notice_one_wrong_element():
    """The oracles against deliberate damage: dropping, doubling or
    misattributing one element of one row must fail the exact check, and a
    dropped element must leave the bound of the normal fill."""
    case = sc.get_case("uniform15odd")
    r = 300
    s = int(case.S.indptr[r])
    for dtype in sc.DTYPES:
        f = sc.fill(case, "exact", dtype)
        want = sc.exact_oracle(case, f.vals, f.x, f.y0, False)
        good = (want[0] if want[1] is None
                else want[0] + 1j * want[1]).astype(dtype)
        sc.check_exact(good, want)
        one = f.vals[s] * f.x[case.S.indices[s]]
        for delta, row in ((-one, r), (one, r), (one, r - 1)):
            bad = good.copy()
            bad[row] += delta
            with pytest.raises(AssertionError):
                sc.check_exact(bad, want)
        g = sc.fill(case, "normal", dtype)
        ref, scale = sc.reference(case, g.vals, g.x, g.y0, False)
        got = ref.astype(dtype)
        sc.check_bound(case, got, ref, scale)
        got[r] -= g.vals[s] * g.x[case.S.indices[s]]
        with pytest.raises(AssertionError):
            sc.check_bound(case, got, ref, scale)


def test_reference_is_wider_than_the_bound_needs():
    assert sc._wide(np.float32) == np.float64
    assert sc._wide(np.complex64) == np.complex128
    for d in (np.float64, np.complex128):
        w = sc._wide(d)
        assert np.finfo(w).eps * 2 ** 11 <= np.finfo(d).eps
    assert np.finfo(np.float64).eps * 2 ** 11 <= np.finfo(np.float32).eps

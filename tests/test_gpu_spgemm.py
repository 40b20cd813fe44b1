# SPDX-License-Identifier: Apache-2.0
"""GPU checks of every SpGEMM kernel of src/hip/spgemm.hip and of the
segmented post-sort of src/hip/segsort.hip against the oracle of
spgemm_cases.py (pytest -m gpu on an MI355X).

Every comparison is on the triple (indptr, indices, data): indptr and
indices equal to the oracle's (so sorted, duplicate-free, of the input
index type, with entries that cancel to zero kept), exact-fill values
equal, normal-fill values within spgemm_cases.entry_bound.

Part a calls each kernel by its own entry point on row lists chosen here,
whatever bin ``row_bin`` would give those rows; the only condition is
spgemm_cases.assert_fits, checked on the host before every launch, because
an over-full hash table never terminates.  Output arrays are pre-filled
with sentinels (-1, NaN); what the oracle does not place must still be a
sentinel afterwards.  Parts b-f run the pipeline (ops.spgemm_local, A @ B)
and assert the device's bin counts against the numpy replica first, so a
case cannot drift onto another kernel unnoticed.

LS_SPGEMM_ABLATE makes the LDS kernels skip phases and produce wrong
results on purpose (timing probes); it is not tested."""
import os
import subprocess
import sys

import numpy as np
import pytest
import scipy.sparse as sp

import legate_sparse as lsp
import spgemm_cases as g
from legate_sparse import ops
from testutils import to_np

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

CODE = {"float32": 0, "float64": 1, "complex64": 2, "complex128": 3}
ICODE = {"int32": 0, "int64": 1}
TYPES = [(d, i) for d in g.DTYPES for i in g.IDX_DTYPES]
TYPE_IDS = [f"{np.dtype(d).name}-{np.dtype(i).name}" for d, i in TYPES]
IDX_IDS = [np.dtype(i).name for i in g.IDX_DTYPES]
KINDS = ("exact", "normal")
TAIL = 64   # sentinel elements behind the last row of every output


@pytest.fixture(scope="module", autouse=True)
def _check_native():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from legate_sparse import _cext
    # GPU runs MUST use the gfx950 extension — no silent fallback
    ext = _cext.require_hip()
    assert tuple(ext.spgemm_lds_bins) == g.LDS_BINS
    assert int(ext.spgemm_global_chunk) == g.GLOBAL_CHUNK
    yield


def _ext():
    from legate_sparse import _cext
    return _cext.require_hip()


def _st():
    return torch.cuda.current_stream().cuda_stream


def _dn(a):
    return torch.from_numpy(np.array(a)).cuda()


# ---------------------------------------------------------------------------
# device operands, each made once and left unchanged
# ---------------------------------------------------------------------------
_DEV = {}


def _dev(key, make):
    if key not in _DEV:
        _DEV[key] = _dn(make())
    return _DEV[key]


class Operands:
    """Device tensors of one case for one fill and one pair of types."""

    def __init__(self, case, kind, dtype, idx):
        f = g.fill(case, kind, dtype)
        dn, xn = np.dtype(dtype).name, np.dtype(idx).name
        self.case, self.kind, self.dtype, self.idx = case, kind, dtype, idx
        A, B = case.A, case.B
        self.ip = _dev((case.name, "Aip"), lambda: A.indptr.astype(np.int64))
        self.bp = _dev((case.name, "Bip"), lambda: B.indptr.astype(np.int64))
        self.ix = _dev((case.name, "Aix", xn), lambda: A.indices.astype(idx))
        self.bx = _dev((case.name, "Bix", xn), lambda: B.indices.astype(idx))
        self.a = _dev((case.name, "a", kind, dn), lambda: f.a)
        self.b = _dev((case.name, "b", kind, dn), lambda: f.b)
        self.code, self.icode = CODE[dn], ICODE[xn]
        self.n_rows = case.a_len.size

    def structure_args(self):
        return (self.ip.data_ptr(), self.ix.data_ptr(), self.bp.data_ptr(),
                self.bx.data_ptr())

    def numeric_args(self):
        return (self.ip.data_ptr(), self.ix.data_ptr(), self.a.data_ptr(),
                self.bp.data_ptr(), self.bx.data_ptr(), self.b.data_ptr())

    def local(self, cache=None):
        return ops.spgemm_local(self.ip, self.ix, self.a, self.bp, self.bx,
                                self.b, self.case.n_cols, cache=cache)


def _shuffled(rows, seed=5):
    rows = np.asarray(rows, dtype=np.int64)
    return rows[np.random.default_rng(seed).permutation(rows.size)]


def _nan(dtype):
    return np.nan + 1j * np.nan if np.dtype(dtype).kind == "c" else np.nan


def _is_sentinel(v):
    return np.isnan(v.real) & np.isnan(v.imag) if np.iscomplexobj(v) \
        else np.isnan(v)


def _device_bins(o):
    """(ub, counts) of the fused phase-0 kernel."""
    ub = torch.full((o.n_rows,), -1, dtype=torch.int64, device="cuda")
    cnt = torch.zeros(8, dtype=torch.int64, device="cuda")
    _ext().spgemm_row_ub_bins(o.ip.data_ptr(), o.ix.data_ptr(),
                              o.bp.data_ptr(), ub.data_ptr(), o.n_rows,
                              cnt.data_ptr(), o.icode, _st())
    return to_np(ub), to_np(cnt)


def _assert_bins(o):
    ub, cnt = _device_bins(o)
    np.testing.assert_array_equal(ub, o.case.ub)
    np.testing.assert_array_equal(cnt, g.bin_counts(o.case))
    return cnt


# ---------------------------------------------------------------------------
# a. each kernel by its own entry point
# ---------------------------------------------------------------------------
def _layout(case, st, rows, count):
    """Row offsets of the output: the oracle's indptr (exact layout), or
    for COUNT runs a capacity layout of ub + 1 slots per listed row (slack
    and one guard element), nothing for the others."""
    if not count:
        return st.indptr.copy()
    cap = np.zeros(case.a_len.size, dtype=np.int64)
    cap[rows] = case.ub[rows] + 1
    off = np.zeros(cap.size + 1, dtype=np.int64)
    np.cumsum(cap, out=off[1:])
    return off


def _check_rows(o, rows, off, Ci, Cv, rn, count, what):
    """Listed rows hold the oracle's entries from off[row] on; everything
    else in the output, in row_nnz too, is still the sentinel."""
    case, st = o.case, g.structure(o.case)
    rows = np.sort(np.asarray(rows, dtype=np.int64))
    Ci, Cv = to_np(Ci), to_np(Cv)
    want_i = np.full(Ci.size, -1, dtype=Ci.dtype)
    for r in rows:
        seg = st.indices[st.indptr[r]:st.indptr[r + 1]]
        want_i[off[r]:off[r] + seg.size] = seg
    assert Ci.dtype == np.dtype(o.idx)
    np.testing.assert_array_equal(Ci, want_i, err_msg=what + " indices")
    written = want_i >= 0
    assert np.all(_is_sentinel(Cv[~written])), what + ": wrote outside"
    g.check_values(o.kind, o.dtype, Cv[written],
                   g.want(case, o.kind, o.dtype), st.n_ij,
                   g.entry_sel(st, rows), what)
    if count:
        want_n = np.full(o.n_rows, -7, dtype=np.int64)
        want_n[rows] = case.distinct[rows]
        np.testing.assert_array_equal(to_np(rn), want_n,
                                      err_msg=what + " row_nnz")


def _numeric(o, rows, count, launch, what):
    case, st = o.case, g.structure(o.case)
    off = _layout(case, st, rows, count)
    total = int(off[-1]) + TAIL
    Ci = torch.full((total,), -1, dtype=o.ix.dtype, device="cuda")
    Cv = torch.full((total,), _nan(o.dtype), dtype=o.a.dtype, device="cuda")
    rn = torch.full((o.n_rows,), -7, dtype=torch.int64, device="cuda")
    rl = _dn(_shuffled(rows))
    off_d = _dn(off)
    launch(rl.data_ptr(), rl.numel(), off_d.data_ptr(), Ci.data_ptr(),
           Cv.data_ptr(), rn.data_ptr() if count else 0)
    torch.cuda.synchronize()
    _check_rows(o, rows, off, Ci, Cv, rn, count, what)


def _symbolic(o, rows, launch, what):
    rn = torch.full((o.n_rows,), -7, dtype=torch.int64, device="cuda")
    rl = _dn(_shuffled(rows, 6))
    launch(rl.data_ptr(), rl.numel(), rn.data_ptr())
    torch.cuda.synchronize()
    want_n = np.full(o.n_rows, -7, dtype=np.int64)
    want_n[rows] = o.case.distinct[rows]
    np.testing.assert_array_equal(to_np(rn), want_n, err_msg=what)


@pytest.mark.parametrize("idx", g.IDX_DTYPES, ids=IDX_IDS)
def test_row_ub_and_bin_scatter(idx):
    """row_ub, row_ub_bins and bin_scatter against the replica: counts per
    bin, and every row exactly once, in its bin's group."""
    ext = _ext()
    for n_cols in g.WIDTHS:
        o = Operands(g.get_case(n_cols), "exact", np.float64, idx)
        cnt = _assert_bins(o)
        ub = torch.full((o.n_rows,), -1, dtype=torch.int64, device="cuda")
        ext.spgemm_row_ub(o.ip.data_ptr(), o.ix.data_ptr(), o.bp.data_ptr(),
                          ub.data_ptr(), o.n_rows, o.icode, _st())
        np.testing.assert_array_equal(to_np(ub), o.case.ub)
        cnt2 = torch.zeros(8, dtype=torch.int64, device="cuda")
        ext.spgemm_bin_count(o.ip.data_ptr(), ub.data_ptr(), o.n_rows,
                             cnt2.data_ptr(), _st())
        np.testing.assert_array_equal(to_np(cnt2), cnt)
        bases = np.concatenate([[0], np.cumsum(cnt)[:-1]]).astype(np.int64)
        cursors = _dn(bases)
        rows_out = torch.full((o.n_rows,), -1, dtype=torch.int64,
                              device="cuda")
        ext.spgemm_bin_scatter(o.ip.data_ptr(), ub.data_ptr(), o.n_rows,
                               cursors.data_ptr(), rows_out.data_ptr(), _st())
        rows_out = to_np(rows_out)
        np.testing.assert_array_equal(np.sort(rows_out),
                                      np.arange(o.n_rows))
        np.testing.assert_array_equal(to_np(cursors), bases + cnt)
        for b in range(8):
            grp = rows_out[bases[b]:bases[b] + cnt[b]]
            np.testing.assert_array_equal(
                np.sort(grp), np.nonzero(o.case.bins == b)[0])


@pytest.mark.parametrize("wcfg", [0, 1, 2], ids=["W8", "W32", "W64"])
@pytest.mark.parametrize("idx", g.IDX_DTYPES, ids=IDX_IDS)
def test_merge_symbolic(wcfg, idx):
    ext = _ext()
    case = g.get_case(g.N_MID)
    o = Operands(case, "exact", np.float64, idx)
    rows = g.eligible_rows(case, "merge", wcfg)
    assert {0, 1, g.MERGE_W[wcfg]} <= set(case.a_len[rows].tolist())
    g.assert_fits(case, "merge", wcfg, rows)
    _symbolic(o, rows, lambda rl, n, rn: ext.spgemm_merge_symbolic(
        wcfg, rl, n, *o.structure_args(), rn, o.icode, _st()),
        f"merge symbolic W{g.MERGE_W[wcfg]}")


@pytest.mark.parametrize("wcfg", [0, 1, 2], ids=["W8", "W32", "W64"])
@pytest.mark.parametrize("dtype,idx", TYPES, ids=TYPE_IDS)
def test_merge_numeric(wcfg, dtype, idx):
    """Every row with a_len <= W (a_len 0, below W, equal to W; ub up to
    4096), exact layout and COUNT into a capacity layout."""
    ext = _ext()
    case = g.get_case(g.N_MID)
    rows = g.eligible_rows(case, "merge", wcfg)
    assert np.any(case.ub[rows] == g.MERGE_UB)
    g.assert_fits(case, "merge", wcfg, rows)
    for kind in KINDS:
        o = Operands(case, kind, dtype, idx)
        for count in (False, True):
            _numeric(o, rows, count,
                     lambda rl, n, off, ci, cv, rn: ext.spgemm_merge_numeric(
                         wcfg, rl, n, *o.numeric_args(), off, ci, cv,
                         o.code, o.icode, rn, _st()),
                     f"merge W{g.MERGE_W[wcfg]} {kind} count={count}")


@pytest.mark.parametrize("cfg", [0, 1, 2, 3])
@pytest.mark.parametrize("idx", g.IDX_DTYPES, ids=IDX_IDS)
def test_lds_symbolic(cfg, idx):
    """All rows with ub within the bin's limit, a 5-entry row and the
    colliding rows included."""
    ext = _ext()
    case = g.get_case(g.N_MID)
    o = Operands(case, "exact", np.float64, idx)
    rows = g.eligible_rows(case, "lds_symbolic", cfg)
    assert case.rows["last_m8"] in rows and case.rows["m8_empty"] in rows
    assert case.rows[f"coll_c{cfg}"] in rows
    assert np.any(case.distinct[rows] == g.LDS_BINS[cfg])
    g.assert_fits(case, "lds_symbolic", cfg, rows)
    _symbolic(o, rows, lambda rl, n, rn: ext.spgemm_symbolic_lds(
        cfg, rl, n, *o.structure_args(), rn, o.icode, _st()),
        f"lds symbolic cfg{cfg}")


@pytest.mark.parametrize("cfg", [0, 1, 2, 3])
@pytest.mark.parametrize("dtype,idx", TYPES, ids=TYPE_IDS)
def test_lds_numeric(cfg, dtype, idx):
    """cfg0-2: compact-then-sort kernel, packed and unpacked keys; cfg3:
    full-table sort, for complex128 on the 4096-slot table that row
    c3_4096d fills exactly.  a_len from 0 to 200: below, at and above the
    group width of every geometry but cfg3's 256."""
    ext = _ext()
    case = g.get_case(g.N_MID)
    size = np.dtype(dtype).itemsize
    rows = g.eligible_rows(case, "lds", cfg, size)
    assert case.rows[f"coll_c{cfg}"] in rows and case.rows["m8_1"] in rows
    assert np.any(case.distinct[rows] == g.LDS_BINS[cfg])
    if cfg == 3:
        assert case.distinct[case.rows["c3_4096d"]] == 4096
        assert case.rows["c3_4096d"] in rows
        assert g.lds_table(3, 16) == 4096
    g.assert_fits(case, "lds", cfg, rows, size)
    for kind in KINDS:
        o = Operands(case, kind, dtype, idx)
        for count in (False, True):
            for pack in (0, 1):
                _numeric(o, rows, count,
                         lambda rl, n, off, ci, cv, rn:
                         ext.spgemm_numeric_lds(
                             cfg, rl, n, *o.numeric_args(), off, ci, cv,
                             o.code, o.icode, rn, pack, _st()),
                         f"lds cfg{cfg} {kind} count={count} pack={pack}")


@pytest.mark.parametrize("n_cols", [g.N_CUT_LO, g.N_CUT_HI])
def test_lds_numeric_last_column_at_the_pack_cut(n_cols):
    """The largest column on both sides of the pack cut, straight through
    the packing geometries: at N = 2^24 - 2 the packed key of column N - 1
    is the largest there is and must still sort below EMPTY."""
    ext = _ext()
    case = g.get_case(n_cols)
    for dtype, idx in ((np.float32, np.int32), (np.complex128, np.int64)):
        o = Operands(case, "exact", dtype, idx)
        for cfg in (0, 1):
            rows = g.eligible_rows(case, "lds", cfg, np.dtype(dtype).itemsize)
            assert case.rows["last_c0"] in rows
            assert case.rows["last_m8"] in rows
            for count in (False, True):
                _numeric(o, rows, count,
                         lambda rl, n, off, ci, cv, rn:
                         ext.spgemm_numeric_lds(
                             cfg, rl, n, *o.numeric_args(), off, ci, cv,
                             o.code, o.icode, rn, case.pack, _st()),
                         f"lds cfg{cfg} N={n_cols} count={count}")


@pytest.mark.parametrize("dtype,idx", TYPES, ids=TYPE_IDS)
def test_compact_rows(dtype, idx):
    """Capacity layout -> exact layout for a subset of the rows."""
    ext = _ext()
    case = g.get_case(g.N_MID)
    st = g.structure(case)
    o = Operands(case, "exact", dtype, idx)
    rows = np.sort(np.concatenate([np.nonzero(case.bins == 0)[0],
                                   [case.rows["c3_4096d"],
                                    case.rows["m64_64"]]]))
    src_off = _layout(case, st, rows, True)
    src_i = np.full(int(src_off[-1]), -3, dtype=idx)
    re, im = g.want(case, "exact", dtype)
    full = (re + (1j * im if im is not None else 0)).astype(dtype)
    src_v = np.full(src_i.size, _nan(dtype), dtype=dtype)
    for r in rows:
        s, e = st.indptr[r], st.indptr[r + 1]
        src_i[src_off[r]:src_off[r] + e - s] = st.indices[s:e]
        src_v[src_off[r]:src_off[r] + e - s] = full[s:e]
    Ci = torch.full((st.indices.size + TAIL,), -1, dtype=o.ix.dtype,
                    device="cuda")
    Cv = torch.full((st.indices.size + TAIL,), _nan(dtype), dtype=o.a.dtype,
                    device="cuda")
    rl, so, di = _dn(_shuffled(rows)), _dn(src_off), _dn(st.indptr)
    si, sv = _dn(src_i), _dn(src_v)
    ext.spgemm_compact_rows(rl.data_ptr(), rl.numel(), so.data_ptr(),
                            di.data_ptr(), si.data_ptr(), sv.data_ptr(),
                            Ci.data_ptr(), Cv.data_ptr(), o.code, o.icode,
                            _st())
    torch.cuda.synchronize()
    _check_rows(o, rows, st.indptr, Ci, Cv, None, False, "compact_rows")


def _global_rows(case):
    names = ["m8_empty", "m8_e8", "m8_1", "c1_128s", "coll_c3", "c3_4096d",
             "c3_4096s", "last_c0", "last_g", "coll_g", "g_4097_65",
             "g_4097_129", "g_8192_5", "g_16400", "g_24576"]
    return np.sort(np.array([case.rows[n] for n in names], dtype=np.int64))


@pytest.mark.parametrize("identity", [0, 1], ids=["probed", "identity"])
@pytest.mark.parametrize("dtype,idx", TYPES, ids=TYPE_IDS)
def test_global_kernels(identity, dtype, idx):
    """spgemm_symbolic_global, spgemm_numeric_global_fill and the two
    compaction kernels on hand-built batch descriptors.  Probed tables are
    the smallest power of two above ``distinct`` (fuller than the pipeline's
    2 * ub, never full); identity tables span p2n.  Rows with a_len 0, with
    ub 0, with an empty B row between long ones, with 1 to 12 chunks."""
    ext = _ext()
    case = g.get_case(g.N_MID)
    st = g.structure(case)
    rows = _global_rows(case)
    if identity:
        sizes = np.full(rows.size, g.p2n_of(case.n_cols), dtype=np.int64)
    else:
        sizes = g._pow2ceil(case.distinct[rows] + 1)
    g.assert_fits(case, "global", bool(identity), rows, tbl_size=sizes)
    bt = g.global_batch(case, rows, sizes)
    assert bt.chunk_ord.max() == 11 and bt.a_len.min() == 0
    d = {k: _dn(getattr(bt, k)) for k in
         ("rows", "tbl_off", "tbl_size", "chunk_rowidx", "chunk_ord",
          "blen_prefix", "pref_base", "a_len")}
    desc = (d["blen_prefix"].data_ptr(), d["pref_base"].data_ptr(),
            d["a_len"].data_ptr())
    n_ch = int(bt.chunk_ord.size)
    keys = torch.full((bt.total,), -1, dtype=torch.int32, device="cuda")
    o = Operands(case, "exact", dtype, idx)
    rn = torch.zeros(o.n_rows, dtype=torch.int64, device="cuda")
    ext.spgemm_symbolic_global(
        d["rows"].data_ptr(), d["chunk_rowidx"].data_ptr(),
        d["chunk_ord"].data_ptr(), n_ch, *o.structure_args(),
        keys.data_ptr(), d["tbl_off"].data_ptr(), d["tbl_size"].data_ptr(),
        rn.data_ptr(), o.icode, identity, *desc, _st())
    torch.cuda.synchronize()
    want_n = np.zeros(o.n_rows, dtype=np.int64)
    want_n[rows] = case.distinct[rows]
    np.testing.assert_array_equal(to_np(rn), want_n, err_msg="symbolic")
    compact = ext.spgemm_global_compact_sorted if identity \
        else ext.spgemm_global_compact
    for kind in KINDS:
        o = Operands(case, kind, dtype, idx)
        for count in (False, True):
            what = f"global identity={identity} {kind} count={count}"
            keys.fill_(-1)
            vals = torch.zeros(bt.total, dtype=o.a.dtype, device="cuda")
            ext.spgemm_numeric_global_fill(
                d["rows"].data_ptr(), d["chunk_rowidx"].data_ptr(),
                d["chunk_ord"].data_ptr(), n_ch, *o.numeric_args(),
                keys.data_ptr(), vals.data_ptr(), d["tbl_off"].data_ptr(),
                d["tbl_size"].data_ptr(), o.code, o.icode, identity, *desc,
                _st())
            off = _layout(case, st, rows, count)
            total = int(off[-1]) + TAIL
            Ci = torch.full((total,), -1, dtype=o.ix.dtype, device="cuda")
            Cv = torch.full((total,), _nan(dtype), dtype=o.a.dtype,
                            device="cuda")
            rn = torch.full((o.n_rows,), -7, dtype=torch.int64,
                            device="cuda")
            off_d = _dn(off)
            compact(d["rows"].data_ptr(), rows.size, keys.data_ptr(),
                    vals.data_ptr(), d["tbl_off"].data_ptr(),
                    d["tbl_size"].data_ptr(), off_d.data_ptr(),
                    Ci.data_ptr(), Cv.data_ptr(),
                    rn.data_ptr() if count else 0, o.code, o.icode, _st())
            torch.cuda.synchronize()
            if not identity:
                # spgemm_global_compact emits table order: sort each row
                # on the host (the device post-sort is checked on its own
                # and through the pipeline)
                ci, cv = to_np(Ci), to_np(Cv)
                for r in rows:
                    s, e = off[r], off[r] + case.distinct[r]
                    perm = np.argsort(ci[s:e], kind="stable")
                    ci[s:e], cv[s:e] = ci[s:e][perm], cv[s:e][perm]
                Ci, Cv = torch.from_numpy(ci), torch.from_numpy(cv)
            _check_rows(o, rows, off, Ci, Cv, rn, count, what)


# ---------------------------------------------------------------------------
# b. the pipeline
# ---------------------------------------------------------------------------
def _check_local(o, out, what):
    ip, ix, v = out
    g.check_product(o.case, o.kind, o.dtype, o.idx, to_np(ip), to_np(ix),
                    to_np(v), what)


def _check_cache(case, cache):
    """The row groups and global batches ops._spgemm_hip built against the
    replica and the host-built descriptors."""
    for b in range(8):
        np.testing.assert_array_equal(
            np.sort(to_np(cache["groups"][b])), np.nonzero(case.bins == b)[0])
    seen = []
    for (rows_b, off_b, sizes_b, total_b, ch_ri, ch_ord, tot_ch, ident,
         bpre, pbase, albat) in cache["g_batches"]:
        rows_b = to_np(rows_b)
        seen.append(rows_b)
        np.testing.assert_array_equal(to_np(sizes_b), case.tbl_size[rows_b])
        assert np.all(case.tbl_ident[rows_b] == bool(ident))
        bt = g.global_batch(case, rows_b, case.tbl_size[rows_b])
        g.assert_fits(case, "global", bool(ident), rows_b,
                      tbl_size=bt.tbl_size)
        np.testing.assert_array_equal(to_np(off_b), bt.tbl_off)
        assert total_b == bt.total and tot_ch == bt.chunk_ord.size
        np.testing.assert_array_equal(to_np(ch_ri), bt.chunk_rowidx)
        np.testing.assert_array_equal(to_np(ch_ord), bt.chunk_ord)
        np.testing.assert_array_equal(to_np(albat), bt.a_len)
        bpre, pbase = to_np(bpre), to_np(pbase)
        for i in range(rows_b.size):
            np.testing.assert_array_equal(
                bpre[pbase[i]:pbase[i] + bt.a_len[i]],
                bt.blen_prefix[bt.pref_base[i]:bt.pref_base[i] + bt.a_len[i]])
    np.testing.assert_array_equal(np.sort(np.concatenate(seen)),
                                  np.nonzero(case.bins == 7)[0])
    return sum(1 for bt in cache["g_batches"] if bt[7]), \
        sum(1 for bt in cache["g_batches"] if not bt[7])


@pytest.mark.parametrize("n_cols", g.ALL_WIDTHS)
@pytest.mark.parametrize("dtype,idx", TYPES, ids=TYPE_IDS)
def test_pipeline(n_cols, dtype, idx):
    """First call (hybrid merge + symbolic), second call on the same cache
    (plain numeric into the cached indptr), a values-only change on the
    cached structure, and a first call with the normal fill."""
    case = g.get_case(n_cols)
    o = Operands(case, "exact", dtype, idx)
    on = Operands(case, "normal", dtype, idx)
    _assert_bins(o)
    cache = {}
    c1 = o.local(cache)
    _check_local(o, c1, f"N={n_cols} first call")
    n_ident, n_probed = _check_cache(case, cache)
    gl = case.bins == 7
    assert (n_ident > 0) == bool(case.tbl_ident[gl].any())
    assert (n_probed > 0) == bool((~case.tbl_ident[gl]).any())
    assert (n_ident > 0, n_probed > 0) == {
        g.N_SMALL: (True, False), g.N_MID: (True, True)}.get(
            n_cols, (False, True))
    c2 = o.local(cache)
    _check_local(o, c2, f"N={n_cols} cached call")
    assert c2[0].data_ptr() != cache["C_indptr"].data_ptr()
    assert c2[0].data_ptr() != c1[0].data_ptr()
    _check_local(on, on.local(cache), f"N={n_cols} values-only change")
    _check_local(on, on.local(), f"N={n_cols} normal fill, no cache")


@pytest.mark.parametrize("n_cols", g.WIDTHS)
@pytest.mark.parametrize("dtype,idx", TYPES, ids=TYPE_IDS)
def test_pipeline_fast_mode(n_cols, dtype, idx, monkeypatch):
    """LS_FAST_SPGEMM=1: every numeric kernel counts into a capacity layout
    (COUNT = true) and the result is compacted afterwards."""
    monkeypatch.setenv("LS_FAST_SPGEMM", "1")
    case = g.get_case(n_cols)
    for kind in KINDS:
        o = Operands(case, kind, dtype, idx)
        _assert_bins(o)
        cache = {}
        _check_local(o, o.local(cache), f"fast N={n_cols} {kind}")
        assert "C_indptr" not in cache


@pytest.mark.parametrize("dtype,idx", TYPES, ids=TYPE_IDS)
def test_pipeline_ident_div(dtype, idx, monkeypatch):
    """LS_SPGEMM_IDENT_DIV=1 against the default at N = 2^17 + 3: the two
    rows with ub > 16384 move from identity to probed tables."""
    case = g.get_case(g.N_MID)
    o = Operands(case, "exact", dtype, idx)
    _assert_bins(o)
    cache = {}
    c_def = o.local(cache)
    ident_def = np.sort(np.concatenate(
        [to_np(b[0]) for b in cache["g_batches"] if b[7]]))
    np.testing.assert_array_equal(
        ident_def, np.sort([case.rows["g_16400"], case.rows["g_24576"]]))
    monkeypatch.setenv("LS_SPGEMM_IDENT_DIV", "1")
    cache1 = {}
    c_one = o.local(cache1)
    assert all(b[7] == 0 for b in cache1["g_batches"])
    sizes, ident = g.table_rule(case.ub, case.n_cols, ident_div=1)
    for b in cache1["g_batches"]:
        np.testing.assert_array_equal(to_np(b[2]), sizes[to_np(b[0])])
    _check_local(o, c_def, "IDENT_DIV default")
    _check_local(o, c_one, "IDENT_DIV=1")
    on = Operands(case, "normal", dtype, idx)
    _check_local(on, on.local(), "IDENT_DIV=1 normal")


@pytest.mark.parametrize("n_cols", [g.N_MID, g.N_BIG])
@pytest.mark.parametrize("dtype,idx", TYPES, ids=TYPE_IDS)
def test_pipeline_segsort_against_torch_composite(n_cols, dtype, idx,
                                                  monkeypatch):
    """LS_SPGEMM_SEGSORT=0 against 1 where the replica says rows get probed
    tables, so both post-sorts have rows to sort (exact and fast mode)."""
    case = g.get_case(n_cols)
    assert (~case.tbl_ident[case.bins == 7]).sum() >= 5
    o = Operands(case, "exact", dtype, idx)
    on = Operands(case, "normal", dtype, idx)
    _assert_bins(o)
    outs = {}
    for seg in ("1", "0"):
        monkeypatch.setenv("LS_SPGEMM_SEGSORT", seg)
        cache = {}
        outs[seg] = o.local(cache)
        assert any(b[7] == 0 for b in cache["g_batches"])
        _check_local(o, outs[seg], f"SEGSORT={seg} N={n_cols}")
        _check_local(on, on.local(), f"SEGSORT={seg} N={n_cols} normal")
        monkeypatch.setenv("LS_FAST_SPGEMM", "1")
        _check_local(o, o.local(), f"SEGSORT={seg} fast N={n_cols}")
        monkeypatch.delenv("LS_FAST_SPGEMM")
    for x, y in zip(outs["0"], outs["1"]):
        assert torch.equal(x, y)


@pytest.mark.parametrize("dtype,idx", TYPES, ids=TYPE_IDS)
def test_pipeline_windowed_B(dtype, idx):
    """A's columns confined to [off, off + K) and B handed over as that row
    window with b_row_offset = off: rows in every merge, LDS and global
    bin, probed and identity tables, first and cached call."""
    case = g.get_case(g.N_MID)
    off = 40961
    for kind in KINDS:
        o = Operands(case, kind, dtype, idx)
        _assert_bins(o)
        ix = _dev((case.name, "Aix+off", np.dtype(idx).name),
                  lambda: (case.A.indices + off).astype(idx))
        cache = {}
        for call in ("first", "cached"):
            out = ops.spgemm_local(o.ip, ix, o.a, o.bp, o.bx, o.b,
                                   case.n_cols, b_row_offset=off,
                                   cache=cache)
            _check_local(o, out, f"windowed {kind} {call}")
        _check_cache(case, cache)


@pytest.mark.parametrize("dtype", [np.float32, np.float64, np.complex64,
                                   np.complex128],
                         ids=lambda d: np.dtype(d).name)
def test_matmul_operator(dtype):
    """A @ B through csr_array, twice (the second product hits the
    structure cache of the pair)."""
    case = g.get_case(g.N_MID)
    f = g.fill(case, "exact", dtype)
    A = lsp.csr_array(sp.csr_array((f.a.copy(), case.A.indices,
                                    case.A.indptr), shape=case.A.shape),
                      dtype=dtype)
    B = lsp.csr_array(sp.csr_array((f.b.copy(), case.B.indices,
                                    case.B.indptr), shape=case.B.shape),
                      dtype=dtype)
    assert A.data.is_cuda and A.nnz == case.A.nnz and B.nnz == case.B.nnz
    for call in ("first", "cached"):
        C = A @ B
        assert C.shape == (case.A.shape[0], case.n_cols)
        g.check_product(case, "exact", dtype, None, to_np(C._indptr),
                        to_np(C._indices), to_np(C._data), f"A @ B {call}")
    assert "C_indptr" in A._spgemm_cache_for(B)


# ---------------------------------------------------------------------------
# c. bit-for-bit repeatability
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.complex128],
                         ids=lambda d: np.dtype(d).name)
def test_repeatable_rows(dtype):
    """Two runs on the normal fill are bit-identical in the rows of the
    merge bins (register merge, fixed order) and in the rows compacted from
    identity tables.  At N = 2^17 + 3 the identity rows are g_16400 and
    g_24576, whose B rows are disjoint, so every slot takes one product.
    The hash bins (LDS and probed or shared identity slots) accumulate with
    atomics in arrival order and are exempt, as the stream kernel is in the
    SpMV tests; the exact fill pins them.  The structure is identical
    everywhere."""
    case = g.get_case(g.N_MID)
    st = g.structure(case)
    o = Operands(case, "normal", dtype, np.int32)
    _assert_bins(o)
    r1, r2 = o.local(), o.local()
    assert torch.equal(r1[0], r2[0]) and torch.equal(r1[1], r2[1])
    ident = (case.bins == 7) & case.tbl_ident
    assert ident.sum() == 2
    assert np.all(case.distinct[ident] == case.ub[ident])
    rows = np.nonzero((case.bins <= 2) | ident)[0]
    sel = g.entry_sel(st, rows)
    assert sel.size > 40000
    v1, v2 = to_np(r1[2])[sel], to_np(r2[2])[sel]
    assert v1.tobytes() == v2.tobytes()


# ---------------------------------------------------------------------------
# d. segsort_pairs alone
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,idx", TYPES, ids=TYPE_IDS)
def test_segsort_pairs(dtype, idx):
    """Per-segment numpy sort; keys distinct within a segment, the largest
    column present, end_bit from n_cols as the pipeline computes it; a gap
    between segments must stay untouched."""
    ext = _ext()
    code, icode = CODE[np.dtype(dtype).name], ICODE[np.dtype(idx).name]
    rng = np.random.default_rng(99)
    for n_cols in (1, 2, 2 ** 16, 2 ** 16 + 1):
        want_sizes = [0, 1, 255, 256, 257, 2047, 2048, 2049, 20000]
        sizes = sorted({min(s, n_cols) for s in want_sizes})
        gap = 5
        seg_b, seg_e, pos = [], [], gap
        for s in sizes:
            seg_b.append(pos)
            seg_e.append(pos + s)
            pos += s + gap
        total = pos
        keys = np.full(total, -1, dtype=idx)
        vals = np.full(total, _nan(dtype), dtype=dtype)
        want_k, want_v = keys.copy(), vals.copy()
        for si, (b, e) in enumerate(zip(seg_b, seg_e)):
            if e == b:
                continue
            k = rng.choice(n_cols - 1, size=e - b - 1, replace=False) \
                if e - b > 1 else np.zeros(0, dtype=np.int64)
            k = rng.permutation(np.append(k, n_cols - 1))
            v = (k * 0.5 + si).astype(dtype)
            if np.dtype(dtype).kind == "c":
                v = v - 1j * k.astype(dtype)
            keys[b:e], vals[b:e] = k, v
            perm = np.argsort(k, kind="stable")
            want_k[b:e], want_v[b:e] = k[perm], v[perm]
        end_bit = max(1, int(n_cols - 1).bit_length())
        kin, vin = _dn(keys), _dn(vals)
        kout = torch.full((total,), -1, dtype=kin.dtype, device="cuda")
        vout = torch.full((total,), _nan(dtype), dtype=vin.dtype,
                          device="cuda")
        sb = _dn(np.array(seg_b, dtype=np.int64))
        se = _dn(np.array(seg_e, dtype=np.int64))
        tb = int(ext.segsort_temp_bytes(total, len(sizes), sb.data_ptr(),
                                        se.data_ptr(), end_bit, code, icode,
                                        _st()))
        temp = torch.empty(max(tb, 16), dtype=torch.uint8, device="cuda")
        ext.segsort_pairs(temp.data_ptr(), tb, kin.data_ptr(),
                          kout.data_ptr(), vin.data_ptr(), vout.data_ptr(),
                          total, len(sizes), sb.data_ptr(), se.data_ptr(),
                          end_bit, code, icode, _st())
        torch.cuda.synchronize()
        np.testing.assert_array_equal(to_np(kout), want_k,
                                      err_msg=f"keys n_cols={n_cols}")
        got_v = to_np(vout)
        live = want_k >= 0
        np.testing.assert_array_equal(got_v[live], want_v[live],
                                      err_msg=f"values n_cols={n_cols}")
        assert np.all(_is_sentinel(got_v[~live]))
        np.testing.assert_array_equal(to_np(kin), keys)  # inputs unchanged


# ---------------------------------------------------------------------------
# e. affine product
# ---------------------------------------------------------------------------
def _banded(n, offsets):
    S = sp.diags([np.ones(n - abs(o)) for o in offsets], offsets,
                 format="csr")
    S.sort_indices()
    return S


def _poisson(nx, ny):
    def T(m):
        return sp.diags([np.ones(m - 1), np.ones(m), np.ones(m - 1)],
                        [-1, 0, 1])
    S = (sp.kron(sp.eye(ny), T(nx)) + sp.kron(T(ny), sp.eye(nx))).tocsr()
    S.sort_indices()
    S.data[:] = 1.0
    return S


def _affine_product(SA, SB, dtype, accepted):
    """A @ B with both affine kernels against each other and the oracle,
    for both fills; ``accepted`` says whether the plan takes the pair."""
    st = g.expand(SA.indptr, SA.indices, SB.indptr, SB.indices, SB.shape[1])
    rng = np.random.default_rng(SA.nnz + SB.nnz)
    cplx = np.dtype(dtype).kind == "c"
    for kind in KINDS:
        def draw(n):
            if kind == "exact":
                ch = np.array([-3, -2, -1, 1, 2, 3])
                v = rng.choice(ch, n).astype(np.float64)
                return (v + 1j * rng.choice(ch, n) if cplx else v
                        ).astype(dtype)
            v = rng.standard_normal(n)
            return (v + 1j * rng.standard_normal(n) if cplx else v
                    ).astype(dtype)
        a, b = draw(SA.nnz), draw(SB.nnz)
        wanted = (g.exact_values(st, a, b) if kind == "exact"
                  else g.wide_values(st, a, b))
        outs = {}
        for k in ("lds", "out"):
            os.environ["LS_SPGEMM_AFFINE_K"] = k
            try:
                A = lsp.csr_array(sp.csr_array((a, SA.indices, SA.indptr),
                                               shape=SA.shape), dtype=dtype)
                B = lsp.csr_array(sp.csr_array((b, SB.indices, SB.indptr),
                                               shape=SB.shape), dtype=dtype)
                assert A._affine_plan() is not None
                assert B._affine_plan() is not None
                for call in ("first", "cached"):
                    C = A @ B
                    what = f"affine {k} {kind} {call}"
                    g.check_structure(st, to_np(C._indptr),
                                      to_np(C._indices), None, what)
                    g.check_values(kind, dtype, to_np(C._data), wanted,
                                   st.n_ij, what=what)
                aff = A._spgemm_cache_for(B).get("aff", "unset")
                assert aff != "unset"
                assert (aff is not None) == accepted, what
                if accepted:
                    # valid rows exist and so do exception rows
                    valid = to_np(aff[2])
                    assert 0 < valid.sum() < valid.size
                outs[k] = C
            finally:
                del os.environ["LS_SPGEMM_AFFINE_K"]
        assert torch.equal(outs["lds"]._indices, outs["out"]._indices)
        if accepted:
            # repeatable bit for bit: fixed summation order, and the
            # exception rows of these operands run the merge kernels
            for k in ("lds", "out"):
                os.environ["LS_SPGEMM_AFFINE_K"] = k
                try:
                    C2 = A @ B
                finally:
                    del os.environ["LS_SPGEMM_AFFINE_K"]
                assert torch.equal(C2._data, outs[k]._data), (kind, k)


@pytest.mark.parametrize("dtype", g.DTYPES, ids=lambda d: np.dtype(d).name)
def test_affine_banded_3x4(dtype):
    n = 701
    _affine_product(_banded(n, (-2, 0, 3)), _banded(n, (-1, 0, 1, 4)),
                    dtype, True)


@pytest.mark.parametrize("dtype", g.DTYPES, ids=lambda d: np.dtype(d).name)
def test_affine_poisson(dtype):
    S = _poisson(40, 24)
    # 13 offset sums: one more than the budget takes at 16 bytes a value
    _affine_product(S, S, dtype, np.dtype(dtype) != np.complex128)


@pytest.mark.parametrize("dtype,offs_a,offs_b,n_e,accepted", [
    (np.float64, (0, 5, 10, 15, 20), (0, 1, 2, 3, 4), 25, True),
    (np.float64, (0, 13), tuple(range(13)), 26, False),
    (np.complex128, (0, 4, 8), (0, 1, 2, 3), 12, True),
    (np.complex128, (0, 1), tuple(range(12)), 13, False),
    (np.float32, (0, 8, 16, 24, 32), tuple(range(8)), 40, True),
    (np.float32, (0, 13, 26, 39), tuple(range(13)), 52, False),
], ids=["f64-25", "f64-26", "c128-12", "c128-13", "f32-40", "f32-52"])
def test_affine_accumulator_budget(dtype, offs_a, offs_b, n_e, accepted):
    """The sum-set sizes on both sides of the accumulator budget: the
    largest accepted, and one beyond, which falls to the general path.  The
    float32 pair has more than 32 distinct offset sums (the budget allows
    51 there)."""
    assert len({a + b for a in offs_a for b in offs_b}) == n_e
    n = 601
    _affine_product(_banded(n, offs_a), _banded(n, offs_b), dtype, accepted)


# ---------------------------------------------------------------------------
# f. scalar merge
# ---------------------------------------------------------------------------
def test_scalar_merge_in_a_fresh_process():
    """LS_SPGEMM_SCALAR is read once per process, so a fresh child runs the
    W = 8 cases of parts a and b under LS_SPGEMM_SCALAR=1.  One child, no
    retry."""
    worker = os.path.join(os.path.dirname(os.path.abspath(__file__)),
                          "spgemm_scalar_worker.py")
    env = dict(os.environ, LS_SPGEMM_SCALAR="1")
    res = subprocess.run([sys.executable, worker], env=env, timeout=180,
                         capture_output=True, text=True)
    assert res.returncode == 0, res.stdout[-4000:] + res.stderr[-4000:]
    ok = [ln for ln in res.stdout.splitlines() if ln.startswith("OK ")]
    # direct: 8 type pairs x 2 fills x COUNT on/off; pipeline: 8 x 3 widths
    assert len(ok) == 8 * 2 * 2 + 8 * 3, res.stdout[-4000:]
    assert "SCALAR_DONE" in res.stdout

# SPDX-License-Identifier: Apache-2.0
"""CPU checks of what the GPU SpGEMM tests rest on (spgemm_cases.py): the
generated operands land in the bins and table classes they claim, the
oracle is right where a dense integer product can tell, it keeps cancelled
entries that scipy drops, and the CPU paths of ops.spgemm_local reproduce
it triple for triple on every case."""
import numpy as np
import pytest
import scipy.sparse as sp

import spgemm_cases as g

torch = pytest.importorskip("torch")

from legate_sparse import _cext, ops  # noqa: E402


@pytest.mark.parametrize("n_cols", g.ALL_WIDTHS)
def test_cases_land_where_they_claim(n_cols):
    c = g.get_case(n_cols)
    assert c.B.shape[0] > 1000 and 40000 < c.B.nnz < 50000
    assert c.B.has_sorted_indices and c.A.has_sorted_indices
    assert c.B.indices.max() == n_cols - 1
    for nm, b in g.EXPECT_BIN.items():
        assert c.bins[c.rows[nm]] == b, nm
    for nm, (a_len, ub) in g.EXPECT_SHAPE.items():
        r = c.rows[nm]
        assert (c.a_len[r], c.ub[r]) == (a_len, ub), nm
    # a_len, ub and distinct from the operands themselves
    np.testing.assert_array_equal(c.a_len, np.diff(c.A.indptr))
    ones = sp.csr_array((np.ones(c.A.nnz), c.A.indices, c.A.indptr),
                        shape=c.A.shape)
    np.testing.assert_array_equal(
        c.ub, np.rint(ones @ np.diff(c.B.indptr).astype(float)))
    st = g.structure(c)
    np.testing.assert_array_equal(c.distinct, np.diff(st.indptr))
    assert np.all(c.distinct <= c.ub)
    if n_cols > g.N_SMALL:
        for nm in ("m8_ub4096", "m64_64", "c0_ub48", "c1_128", "c2_1024",
                   "c3_4096d", "g_24576"):
            assert c.distinct[c.rows[nm]] == c.ub[c.rows[nm]], nm
    assert c.distinct[c.rows["c3_4096s"]] == 32
    assert c.distinct[c.rows["c1_128s"]] == 1
    # no bin's row count fills whole blocks, for either value size
    cnt = g.bin_counts(c)
    for w in range(3):
        assert cnt[w] % g.merge_rows_per_block(w) != 0
    for cfg in range(3):
        for size in (8, 16):
            rpb = g.lds_rows_per_block(cfg, size)
            assert rpb == 1 or cnt[3 + cfg] % rpb != 0
    assert cnt.sum() == c.a_len.size and np.all(cnt > 1)
    # every row fits the kernel its bin runs, for every value size
    for b in range(3):
        g.assert_fits(c, "merge", b, np.nonzero(c.bins == b)[0])
    for cfg in range(4):
        rows = np.nonzero(c.bins == 3 + cfg)[0]
        g.assert_fits(c, "lds_symbolic", cfg, rows)
        for size in (4, 8, 16):
            g.assert_fits(c, "lds", cfg, rows, size)


def test_colliding_columns_share_one_wrapping_chain():
    for n_cols in g.ALL_WIDTHS:
        c = g.get_case(n_cols)
        r = c.rows["coll_c3"]
        st = g.structure(c)
        cols = st.indices[st.indptr[r]:st.indptr[r + 1]]
        assert cols.size == 16
        for tbl in (64, 256, 2048, 4096, 8192):
            if tbl > c.coll_stride:
                continue
            h = (cols * g.HASH_MULT % 2 ** 32) & (tbl - 1)
            # one chain of 16 from slot TBL - 3: it wraps past the end
            assert np.all(h == tbl - 3), (n_cols, tbl)


def test_table_classes():
    """N = 5003: all identity.  2^17 + 3: ub <= 16384 probed (16384 or
    32768 slots), beyond identity, so one product runs both batch classes;
    with LS_SPGEMM_IDENT_DIV=1 all probed.  >= 2^24 - 2: all probed."""
    c = g.get_case(g.N_SMALL)
    gl = c.bins == 7
    assert gl.sum() == 7 and np.all(c.tbl_ident[gl])
    assert np.all(c.tbl_size[gl] == 8192)
    c = g.get_case(g.N_MID)
    gl = np.nonzero(c.bins == 7)[0]
    for r in gl:
        if c.ub[r] <= 8192:
            assert (c.tbl_size[r], c.tbl_ident[r]) == (16384, False)
        else:
            assert c.ub[r] > 16384
            assert (c.tbl_size[r], c.tbl_ident[r]) == (2 ** 18, True)
    assert c.tbl_ident[gl].sum() == 2 and (~c.tbl_ident[gl]).sum() == 5
    size, ident = g.table_rule(c.ub[gl], c.n_cols, ident_div=1)
    assert not ident.any() and size.max() == 65536
    # the rule between the two classes, from the rule itself
    size, ident = g.table_rule(np.array([4097, 8192, 8193, 16384, 16385]),
                               g.N_MID)
    assert size.tolist() == [16384, 16384, 32768, 32768, 2 ** 18]
    assert ident.tolist() == [False] * 4 + [True]
    for n_cols in (g.N_BIG, g.N_CUT_LO, g.N_CUT_HI):
        c = g.get_case(n_cols)
        gl = c.bins == 7
        assert not c.tbl_ident[gl].any()
        assert np.all(c.tbl_size[gl] >= 2 * c.ub[gl])
        assert np.all(c.tbl_size[gl] < 4 * c.ub[gl])
    assert [g.pack_flag(n) for n in g.ALL_WIDTHS] == [1, 1, 0, 1, 0]
    # the largest packed key stays below EMPTY
    assert ((g.N_CUT_LO - 1) << 8 | 255) < 0xFFFFFFFF


def test_row_bin_thresholds():
    a = np.array([0, 8, 9, 32, 33, 64, 65, 64, 65, 65, 65, 65, 65, 65, 65, 1])
    u = np.array([0, 4096, 1, 1, 1, 4096, 0, 4097, 48, 49, 128, 129, 1024,
                  1025, 4096, 4097])
    assert g.row_bin(a, u).tolist() == [0, 0, 1, 1, 2, 2, 3, 7, 3, 4, 4, 5,
                                        5, 6, 6, 7]


def _small(seed, m=9, k=11, n=13, complex_=False):
    rng = np.random.default_rng(seed)
    A = sp.random(m, k, 0.4, random_state=rng, format="csr")
    B = sp.random(k, n, 0.4, random_state=rng, format="csr")
    for M in (A, B):
        M.sort_indices()
        d = rng.integers(1, 4, M.nnz) * rng.choice([-1, 1], M.nnz)
        M.data = (d + 1j * rng.integers(1, 4, M.nnz) if complex_
                  else d.astype(float))
    return A, B


@pytest.mark.parametrize("complex_", [False, True])
def test_oracle_matches_dense_integer_product(complex_):
    for seed in range(5):
        A, B = _small(seed, complex_=complex_)
        st = g.expand(A.indptr, A.indices, B.indptr, B.indices, B.shape[1])
        re, im = g.exact_values(st, A.data, B.data)
        Ad, Bd = A.toarray(), B.toarray()
        D = Ad @ Bd
        pattern = ((Ad != 0).astype(int) @ (Bd != 0).astype(int))
        rows = np.repeat(np.arange(A.shape[0]), np.diff(st.indptr))
        got = np.zeros(D.shape, dtype=D.dtype)
        got[rows, st.indices] = re + (1j * im if complex_ else 0)
        np.testing.assert_array_equal(got, D)
        cnt = np.zeros(D.shape, dtype=int)
        cnt[rows, st.indices] = st.n_ij
        np.testing.assert_array_equal(cnt, pattern)
        for r in range(A.shape[0]):
            assert np.all(np.diff(st.indices[st.indptr[r]:st.indptr[r + 1]])
                          > 0)
        ref, scale = g.wide_values(st, A.data, B.data)
        np.testing.assert_array_equal(ref, (re + 1j * im) if complex_ else re)
        assert np.all(scale * (1 + 1e-12) >= np.abs(ref))


def test_oracle_keeps_cancelled_entry_and_scipy_drops_it():
    """[[1, 1]] @ [[1, 2], [-1, 3]]: entry (0, 0) is 1 - 1.  This project
    stores it (structure does not depend on values); scipy's product does
    not, which is why scipy is not the structural reference."""
    A = sp.csr_array(np.array([[1.0, 1.0]]))
    B = sp.csr_array(np.array([[1.0, 2.0], [-1.0, 3.0]]))
    st = g.expand(A.indptr, A.indices, B.indptr, B.indices, 2)
    re, _ = g.exact_values(st, A.data, B.data)
    assert st.indptr.tolist() == [0, 2] and st.indices.tolist() == [0, 1]
    assert re.tolist() == [0, 5] and st.n_ij.tolist() == [2, 2]
    S = A @ B
    assert S.nnz == 1 and S.indices.tolist() == [1]
    ip, ix, v = ops.spgemm_local(
        *(torch.from_numpy(np.asarray(x)) for x in (
            A.indptr.astype(np.int64), A.indices.astype(np.int64), A.data,
            B.indptr.astype(np.int64), B.indices.astype(np.int64), B.data)),
        2)
    assert ip.tolist() == [0, 2] and ix.tolist() == [0, 1]
    assert v.tolist() == [0.0, 5.0]


def _operands(c, kind, dtype, idx):
    f = g.fill(c, kind, dtype)
    t = torch.from_numpy
    return (t(c.A.indptr.astype(np.int64)), t(c.A.indices.astype(idx)),
            t(f.a.copy()), t(c.B.indptr.astype(np.int64)),
            t(c.B.indices.astype(idx)), t(f.b.copy()))


@pytest.mark.parametrize("n_cols", g.ALL_WIDTHS)
def test_cpu_extension_reproduces_the_oracle(n_cols):
    assert _cext.has_cpu()
    c = g.get_case(n_cols)
    combos = [(np.float64, np.int32), (np.complex64, np.int64),
              (np.float32, np.int64), (np.complex128, np.int32)]
    if n_cols > g.N_MID:    # the CPU kernel's dense accumulator spans N
        combos = combos[:2]
    for dtype, idx in combos:
        for kind in ("exact", "normal"):
            ip, ix, v = ops.spgemm_local(*_operands(c, kind, dtype, idx),
                                         n_cols)
            g.check_product(c, kind, dtype, idx, ip.numpy(), ix.numpy(),
                            v.numpy(), f"cpu {n_cols} {kind}")


@pytest.mark.parametrize("n_cols", g.WIDTHS)
def test_torch_composite_reproduces_the_oracle(n_cols):
    """_spgemm_esc, the device-independent fallback (it returns int64
    indices whatever the input index type)."""
    c = g.get_case(n_cols)
    for dtype, idx in ((np.float64, np.int64), (np.complex128, np.int32)):
        for kind in ("exact", "normal"):
            ip, ix, v = ops._spgemm_esc(*_operands(c, kind, dtype, idx),
                                        n_cols)
            g.check_product(c, kind, dtype, None, ip.numpy(), ix.numpy(),
                            v.numpy(), f"esc {n_cols} {kind}")


def test_windowed_B_on_cpu():
    """A's columns shifted by off and B handed over as the row window that
    starts at off: the same product."""
    c = g.get_case(g.N_MID)
    off = 12345
    ip, ix, a, bp, bx, b = _operands(c, "exact", np.float64, np.int64)
    for fn in (ops.spgemm_local, ops._spgemm_esc):
        out = fn(ip, ix + off, a, bp, bx, b, c.n_cols, off)
        g.check_product(c, "exact", np.float64, np.int64,
                        *(x.numpy() for x in out), what="windowed")


def test_global_batch_descriptors():
    c = g.get_case(g.N_MID)
    rows = np.nonzero(c.bins == 7)[0]
    bt = g.global_batch(c, rows, c.tbl_size[rows])
    assert bt.chunk_rowidx.size == bt.chunk_ord.size
    assert bt.chunk_rowidx.size == sum(
        max(1, -(-int(u) // g.GLOBAL_CHUNK)) for u in c.ub[rows])
    for i, r in enumerate(rows):
        pre = bt.blen_prefix[bt.pref_base[i]:bt.pref_base[i] + bt.a_len[i]]
        assert pre[-1] == c.ub[r] and np.all(np.diff(pre) >= 0)
    i = rows.tolist().index(c.rows["g_8192_5"])
    pre = bt.blen_prefix[bt.pref_base[i]:bt.pref_base[i] + 5]
    assert pre.tolist() == [2048, 4096, 4096, 6144, 8192]  # tie in the middle
    with pytest.raises(AssertionError):
        g.assert_fits(c, "global", False, rows, tbl_size=c.distinct[rows] // 2
                      * 0 + 4096)
    with pytest.raises(AssertionError):
        g.assert_fits(c, "merge", 0, [c.rows["m32_9"]])
    with pytest.raises(AssertionError):
        g.assert_fits(c, "lds", 0, [c.rows["c1_49"]])
    with pytest.raises(AssertionError):
        g.assert_fits(c, "lds", 3, [c.rows["g_4097_65"]], 16)

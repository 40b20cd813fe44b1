# SPDX-License-Identifier: Apache-2.0
"""Operands, value fills, the oracle and numpy replicas of the row binning
shared by the SpGEMM tests (CPU: test_spgemm_cases.py, GPU:
test_gpu_spgemm.py and spgemm_scalar_worker.py).  Imports without a GPU.

One case per width N of B.  B has about 1100 rows in blocks of fixed length
(0, 1, 2, 8, 16, 32, 64, 512, 2048); a row of A is a list of B-row ids, so
its length ``a_len``, its expansion bound ``ub`` (the sum of the picked
B-row lengths) and its number of distinct output columns are known before
anything is multiplied.  Column modes of the B blocks:

disjoint   all rows of the block (and of every other disjoint block) have
           different columns while N has room for them: distinct == ub,
           the fullest table a bin can see.
identical  all rows of the block share their columns: distinct is the
           B-row length and every slot takes a_len contributions.
colliding  16 columns c0 + S*j with S a multiple of every LDS table size
           that fits N (S = 8192 for N > 2^17, else 256) and c0 chosen so
           that hash1 = col * 2654435761 & (TBL - 1) is TBL - 3 for every
           TBL <= S: one probe chain of 16 that wraps past the table end.

The named rows of A sit on every threshold of ``row_bin``
(src/hip/spgemm.hip); fillers keep each bin's row count off the multiples
of its rows per block.  Every case records, per row, the bin and the
global-table class the numpy replicas of ``row_bin`` and of the sizing rule
of ``ops._spgemm_hip`` give.

Two fills, as in spmv_cases: ``exact`` (integers in +-{1,2,3}, both parts
for complex; at most 4096 contributions of magnitude <= 18 per entry, so
every sum is an integer below 2^24, exact in fp32 in any order) and
``normal``.  The oracle is an expand-sort-reduce over (row, col) keys that
keeps entries whose value cancels to zero; scipy's product drops those, so
it cannot serve as the reference for the structure.
"""
from collections import namedtuple

import numpy as np
import scipy.sparse as sp

from spmv_cases import DTYPES, IDX_DTYPES, _wide  # noqa: F401

# thresholds of row_bin and the LDS geometries, from the header comment of
# src/hip/spgemm.hip and its launch helpers; the GPU tests compare the first
# two with ext.spgemm_lds_bins and ext.spgemm_global_chunk
LDS_BINS = (48, 128, 1024, 4096)
GLOBAL_CHUNK = 2048
MERGE_W = (8, 32, 64)
MERGE_UB = 4096
N_BINS = 8
HASH_MULT = 2654435761

N_SMALL = 5003             # pack; every global table identity
N_MID = 2 ** 17 + 3        # pack; probed and identity global tables
N_BIG = 2 ** 24 + 5        # no pack; every global table probed
N_CUT_LO = 2 ** 24 - 2     # the last width that packs
N_CUT_HI = 2 ** 24 - 1     # the first that does not
WIDTHS = (N_SMALL, N_MID, N_BIG)
ALL_WIDTHS = WIDTHS + (N_CUT_LO, N_CUT_HI)


def pack_flag(n_cols):
    """ops._spgemm_hip: (col << 8 | slot) keys need col < 2^24 - 1."""
    return 1 if n_cols < (1 << 24) - 1 else 0


def merge_rows_per_block(wcfg):
    return 256 // MERGE_W[wcfg]


def lds_table(cfg, itemsize, symbolic=False):
    """Slots of the LDS table compiled for (cfg, value size)."""
    if cfg == 3 and itemsize > 8 and not symbolic:
        return 4096
    return (64, 256, 2048, 8192)[cfg]


def lds_rows_per_block(cfg, itemsize, symbolic=False):
    if symbolic or itemsize <= 8:
        return (32, 16, 2, 1)[cfg]
    return (32, 8, 1, 1)[cfg]


# ---------------------------------------------------------------------------
# replicas
# ---------------------------------------------------------------------------
def row_bin(a_len, ub, lds_bins=LDS_BINS):
    """numpy replica of row_bin(): 0-2 merge W = 8/32/64, 3-6 LDS hash
    cfg0-3, 7 global."""
    a_len = np.asarray(a_len, dtype=np.int64)
    ub = np.asarray(ub, dtype=np.int64)
    merge = (ub <= MERGE_UB) & (a_len <= MERGE_W[2])
    mb = np.where(a_len <= MERGE_W[0], 0, np.where(a_len <= MERGE_W[1], 1, 2))
    hb = 3 + np.searchsorted(np.asarray(lds_bins, dtype=np.int64), ub,
                             side="left")
    return np.where(merge, mb, hb).astype(np.int64)


def _pow2ceil(x):
    x = np.maximum(np.asarray(x, dtype=np.int64), 1)
    return (1 << np.ceil(np.log2(x.astype(np.float64))).astype(np.int64))


def p2n_of(n_cols):
    p = 1
    while p < int(n_cols):
        p *= 2
    return p


def table_rule(ub, n_cols, ident_div=4):
    """(slots, identity) of the global-bin tables: 2 * ub clamped to the
    power of two above N and rounded up to a power of two; identity (slot =
    col, N-spanning table) where that reaches p2n / ident_div while p2n is
    at most 2^19, else only where it reaches p2n."""
    p2n = p2n_of(n_cols)
    size = _pow2ceil(np.minimum(2 * np.asarray(ub, dtype=np.int64), p2n))
    if ident_div > 1 and p2n * 4 <= (1 << 21):
        ident = size * ident_div >= p2n
        size = np.where(ident, p2n, size)
    else:
        ident = size >= p2n
    return size.astype(np.int64), ident


# ---------------------------------------------------------------------------
# operands
# ---------------------------------------------------------------------------
# name, rows, length, mode; the order is the order of B's rows.  The two
# halves of the 2048 block lie on both sides of the empty rows, so a sorted
# A row can have an empty B row between long ones.
_BLOCKS = [
    ("L2048a", 6, 2048, "disjoint"),
    ("L1d", 200, 1, "disjoint"),
    ("L1s", 130, 1, "identical"),
    ("E", 160, 0, "empty"),
    ("L2d", 64, 2, "disjoint"),
    ("L8d", 64, 8, "disjoint"),
    ("L16d", 64, 16, "disjoint"),
    ("L32d", 128, 32, "disjoint"),
    ("L32s", 130, 32, "identical"),
    ("L64d", 64, 64, "disjoint"),
    ("L64s", 64, 64, "identical"),
    ("L512d", 8, 512, "disjoint"),
    ("C16", 70, 16, "colliding"),
    ("C1", 16, 1, "colliding"),
    ("T", 3, 2, "last"),
    ("L2048b", 6, 2048, "disjoint"),
]
# logical columns are handed out in this order, so that at N = 5003 the
# blocks named first are still disjoint
_COL_ORDER = ["L32d", "L1d", "L1s", "L32s", "L64s", "L2d", "L8d", "L16d",
              "L64d", "L512d", "L2048a", "L2048b"]

Case = namedtuple(
    "Case", "name n_cols A B a_len ub distinct bins tbl_size tbl_ident "
            "rows claim coll_stride pack")


def _stride(n_cols, span):
    s = max(1, (n_cols - 1) // span)
    while np.gcd(s, n_cols) != 1:
        s -= 1
    return s


def collide_base(stride):
    """c0 < stride with hash1(c0, stride - 1) == stride - 3."""
    return ((stride - 3) * pow(HASH_MULT, -1, stride)) % stride


def _build_B(n_cols):
    info = {name: (rows, length, mode) for name, rows, length, mode in _BLOCKS}
    span = sum(info[b][0] * info[b][1] if info[b][2] == "disjoint"
               else info[b][1] for b in _COL_ORDER)
    stride = _stride(n_cols, span)
    cols_of = {}
    cur = 0
    for name in _COL_ORDER:
        rows, length, mode = info[name]
        out = []
        for r in range(rows):
            first = cur + (r * length if mode == "disjoint" else 0)
            c = (np.arange(first, first + length, dtype=np.int64)
                 * stride) % n_cols
            out.append(np.sort(c))
        cols_of[name] = out
        cur += rows * length if mode == "disjoint" else length
    S = 8192 if n_cols > 2 ** 17 else 256
    c0 = collide_base(S)
    coll = c0 + S * np.arange(16, dtype=np.int64)
    assert coll[-1] < n_cols
    cols_of["C16"] = [coll] * info["C16"][0]
    cols_of["C1"] = [coll[j:j + 1] for j in range(16)]
    cols_of["E"] = [np.zeros(0, dtype=np.int64)] * info["E"][0]
    cols_of["T"] = [np.array([0, n_cols - 1]), np.array([1, n_cols - 1]),
                    np.array([n_cols - 2, n_cols - 1])]
    first_row = {}
    lens, cols = [], []
    for name, rows, length, mode in _BLOCKS:
        first_row[name] = len(lens)
        for c in cols_of[name]:
            assert c.size == length and np.all(np.diff(c) > 0)
            lens.append(length)
            cols.append(c)
    indptr = np.zeros(len(lens) + 1, dtype=np.int64)
    np.cumsum(lens, out=indptr[1:])
    indices = np.concatenate(cols).astype(np.int64)
    B = sp.csr_array((np.ones(indices.size), indices, indptr),
                     shape=(len(lens), n_cols))
    return B, first_row, info, span, S


def _named_rows(pick):
    """name -> (B-row ids, what the construction promises for distinct:
    'disjoint' (== ub), an integer, or None)."""
    E, r = "E", {}
    r["m8_empty"] = ([], 0)
    r["m8_e1"] = (pick(E, 1), 0)
    r["m8_e8"] = (pick(E, 8, 3), 0)
    r["m8_1"] = (pick("L8d", 1), "disjoint")
    r["m8_7"] = (pick("L8d", 7, 1), "disjoint")
    r["m8_ub4096"] = (pick("L512d", 8), "disjoint")
    r["m32_9"] = (pick("L16d", 9), "disjoint")
    r["m32_32"] = (pick("L32d", 32), "disjoint")
    r["m64_33"] = (pick("L8d", 33, 8), "disjoint")
    r["m64_64"] = (pick("L64d", 64), "disjoint")
    r["m64_64s"] = (pick("L64s", 64), 64)
    r["c0_ub0"] = (pick(E, 65, 20), 0)
    r["c0_ub48"] = (pick("L1d", 48) + pick(E, 17, 1), "disjoint")
    r["c0_200"] = (pick("L1d", 48, 50) + pick(E, 152), "disjoint")
    r["c1_49"] = (pick("L1d", 49, 100) + pick(E, 16, 90), "disjoint")
    r["c1_128"] = (pick("L1d", 128, 30), "disjoint")
    r["c1_128s"] = (pick("L1s", 128), 1)
    r["c2_129"] = (pick("L1d", 129, 70), "disjoint")
    r["c2_1024"] = (pick("L16d", 64) + pick(E, 1, 159), "disjoint")
    r["c3_1025"] = (pick("L16d", 64) + pick("L1d", 1, 199), "disjoint")
    r["c3_4096d"] = (pick("L32d", 128), "disjoint")
    r["c3_4096s"] = (pick("L32s", 128, 2), 32)
    r["g_4097_65"] = (pick("L64d", 64) + pick("L1d", 1, 5), "disjoint")
    r["g_4097_129"] = (pick("L32d", 128) + pick("L1d", 1, 6), "disjoint")
    r["g_8192_5"] = (pick("L2048a", 2, 1) + pick(E, 1, 77)
                     + pick("L2048b", 2, 3), "disjoint")
    r["g_16400"] = (pick("L2048a", 6) + pick("L2048b", 2)
                    + pick("L16d", 1, 63), "disjoint")
    r["g_24576"] = (pick("L2048a", 6) + pick("L2048b", 6), "disjoint")
    # colliding rows, one per LDS geometry and one in a probed global table
    r["coll_m8"] = (pick("C1", 5, 2) + pick("C16", 3), 16)
    r["coll_c0"] = (pick("C16", 2) + pick("C1", 16) + pick(E, 47, 30), 16)
    r["coll_c1"] = (pick("C16", 7, 3) + pick(E, 58, 100), 16)
    r["coll_c2"] = (pick("C16", 40) + pick(E, 25, 10), 16)
    r["coll_c3"] = (pick("C16", 70), 16)
    r["coll_g"] = (pick("C16", 70) + pick("L2048b", 2), None)
    # the last column of B in every kind of bin
    r["last_m8"] = (pick("T", 3), 4)
    r["last_c0"] = (pick("T", 3) + pick(E, 62, 40), 4)
    r["last_c1"] = (pick("T", 3) + pick("L1d", 100, 10), None)
    r["last_c2"] = (pick("T", 3) + pick("L1d", 150, 20) + pick("L2d", 30),
                    None)
    r["last_c3"] = (pick("T", 3) + pick("L32d", 70, 9), None)
    r["last_g"] = (pick("T", 3) + pick("L2048a", 3), None)
    return r


def _fillers(pick, rng):
    out = {}
    for i in range(45):       # merge W = 8
        n = 1 + i % 8
        out[f"f0_{i}"] = pick("L8d", n, int(rng.integers(0, 56))) \
            if i % 3 else pick("L2d", n, int(rng.integers(0, 56)))
    for i in range(5):        # merge W = 32
        out[f"f1_{i}"] = pick("L8d", 9 + 5 * i, i)
    for i in range(3):        # merge W = 64
        out[f"f2_{i}"] = pick("L2d", 33 + 15 * i, min(i, 1))
    for i in range(33):       # cfg0: a_len >= 65, ub <= 48
        k = i % 49
        out[f"f3_{i}"] = pick("L1d", k, 3 * i) + pick(E_, 65 + i - k, i)
    for i in range(14):       # cfg1: 49 <= ub <= 128
        k = 49 + 6 * i
        out[f"f4_{i}"] = pick("L1d", k, i) + pick(E_, max(0, 70 - k), 2 * i)
    for i in range(5):        # cfg2: 129 <= ub <= 1024
        out[f"f5_{i}"] = (pick("L1d", 100 + 20 * i, i)
                          + pick("L2d", 15 + 10 * i))
    for i in range(2):        # cfg3
        out[f"f6_{i}"] = pick("L16d", 64) + pick("L1d", 7 + 30 * i, 11)
    return out


E_ = "E"
_CASES = {}


def get_case(n_cols):
    """The case of width n_cols, built once per process, never modified."""
    if n_cols in _CASES:
        return _CASES[n_cols]
    B, first_row, info, span, S = _build_B(n_cols)

    def pick(block, n, start=0):
        assert 0 <= start and start + n <= info[block][0], (block, n, start)
        f = first_row[block] + start
        return list(range(f, f + n))

    named = _named_rows(pick)
    rows = {k: v[0] for k, v in named.items()}
    rows.update(_fillers(pick, np.random.default_rng(4242)))
    names = sorted(rows)
    order = np.random.default_rng(77).permutation(len(names))
    names = [names[i] for i in order]
    blen = np.diff(B.indptr)
    a_lists = []
    for nm in names:
        ids = np.array(sorted(rows[nm]), dtype=np.int64)
        assert np.all(np.diff(ids) > 0), nm
        a_lists.append(ids)
    a_len = np.array([a.size for a in a_lists], dtype=np.int64)
    indptr = np.zeros(len(names) + 1, dtype=np.int64)
    np.cumsum(a_len, out=indptr[1:])
    indices = (np.concatenate(a_lists) if a_lists
               else np.zeros(0, dtype=np.int64))
    A = sp.csr_array((np.ones(indices.size), indices, indptr),
                     shape=(len(names), B.shape[0]))
    ub = np.array([int(blen[a].sum()) for a in a_lists], dtype=np.int64)
    distinct = np.array(
        [np.unique(np.concatenate(
            [B.indices[B.indptr[k]:B.indptr[k + 1]] for k in a]
            + [np.zeros(0, dtype=np.int64)])).size for a in a_lists],
        dtype=np.int64)
    bins = row_bin(a_len, ub)
    size, ident = table_rule(ub, n_cols)
    row_of = {nm: i for i, nm in enumerate(names)}
    claim = {}
    for nm, (_, promise) in named.items():
        i = row_of[nm]
        if promise == "disjoint":
            if span <= n_cols:      # the columns wrap at N = 5003
                assert distinct[i] == ub[i], (nm, distinct[i], ub[i])
                claim[nm] = int(ub[i])
        elif promise is not None:
            assert distinct[i] == promise, (nm, distinct[i], promise)
            claim[nm] = promise
    case = Case(f"N{n_cols}", n_cols, A, B, a_len, ub, distinct, bins, size,
                ident, row_of, claim, S, pack_flag(n_cols))
    for a in (a_len, ub, distinct, bins, size, ident):
        a.setflags(write=False)
    _CASES[n_cols] = case
    return case


# the bin every named row must land in, at every width
EXPECT_BIN = {
    "m8_empty": 0, "m8_e1": 0, "m8_e8": 0, "m8_1": 0, "m8_7": 0,
    "m8_ub4096": 0, "m32_9": 1, "m32_32": 1, "m64_33": 2, "m64_64": 2,
    "m64_64s": 2, "c0_ub0": 3, "c0_ub48": 3, "c0_200": 3, "c1_49": 4,
    "c1_128": 4, "c1_128s": 4, "c2_129": 5, "c2_1024": 5, "c3_1025": 6,
    "c3_4096d": 6, "c3_4096s": 6, "g_4097_65": 7, "g_4097_129": 7,
    "g_8192_5": 7, "g_16400": 7, "g_24576": 7, "coll_m8": 0, "coll_c0": 3,
    "coll_c1": 4, "coll_c2": 5, "coll_c3": 6, "coll_g": 7, "last_m8": 0,
    "last_c0": 3, "last_c1": 4, "last_c2": 5, "last_c3": 6, "last_g": 7,
}
# (a_len, ub) of the rows the issue names
EXPECT_SHAPE = {
    "m8_empty": (0, 0), "m8_e1": (1, 0), "m8_e8": (8, 0), "m8_1": (1, 8),
    "m8_7": (7, 56), "m8_ub4096": (8, 4096), "m32_9": (9, 144),
    "m32_32": (32, 1024), "m64_33": (33, 264), "m64_64": (64, 4096),
    "c0_ub0": (65, 0), "c0_ub48": (65, 48), "c0_200": (200, 48),
    "c1_49": (65, 49), "c1_128": (128, 128), "c2_129": (129, 129),
    "c2_1024": (65, 1024), "c3_1025": (65, 1025), "c3_4096d": (128, 4096),
    "g_4097_65": (65, 4097), "g_4097_129": (129, 4097),
    "g_8192_5": (5, 8192), "g_16400": (9, 16400), "g_24576": (12, 24576),
}


def bin_counts(case, rows=None):
    b = case.bins if rows is None else case.bins[np.asarray(rows)]
    return np.bincount(b, minlength=N_BINS)


# ---------------------------------------------------------------------------
# preconditions of the kernels
# ---------------------------------------------------------------------------
def eligible_rows(case, kernel, arg, itemsize=8):
    """Rows of the case that ``kernel`` may be handed: ("merge", wcfg),
    ("lds", cfg) or ("lds_symbolic", cfg)."""
    if kernel == "merge":
        ok = (case.a_len <= MERGE_W[arg]) & (case.ub <= MERGE_UB)
    else:
        tbl = lds_table(arg, itemsize, kernel == "lds_symbolic")
        ok = (case.ub <= LDS_BINS[arg]) & (case.distinct <= tbl)
    return np.nonzero(ok)[0]


def assert_fits(case, kernel, arg, rows, itemsize=8, tbl_size=None):
    """Raise before anything is launched if a row is beyond the kernel's
    capacity: an over-full hash table makes the probe loop spin forever."""
    rows = np.asarray(rows, dtype=np.int64)
    assert rows.size == 0 or (rows.min() >= 0
                              and rows.max() < case.a_len.size)
    if kernel == "merge":
        assert np.all(case.a_len[rows] <= MERGE_W[arg]), "a_len > W"
        assert np.all(case.ub[rows] <= MERGE_UB), "ub beyond the merge bins"
    elif kernel in ("lds", "lds_symbolic"):
        tbl = lds_table(arg, itemsize, kernel == "lds_symbolic")
        assert np.all(case.ub[rows] <= LDS_BINS[arg]), "ub beyond the bin"
        assert np.all(case.distinct[rows] <= tbl), "table over-full"
    elif kernel == "global":
        tbl_size = np.asarray(tbl_size, dtype=np.int64)
        identity = arg
        assert np.all(tbl_size & (tbl_size - 1) == 0) and np.all(tbl_size > 0)
        if identity:
            assert np.all(tbl_size >= case.n_cols), "identity table < N"
        else:
            assert np.all(case.distinct[rows] <= tbl_size), "table over-full"
    else:
        raise ValueError(kernel)


# ---------------------------------------------------------------------------
# fills
# ---------------------------------------------------------------------------
Fill = namedtuple("Fill", "kind a b")
_FILLS = {}


def fill(case, kind, dtype):
    """(A values, B values) of ``dtype``; cached, read-only, no zeros."""
    dtype = np.dtype(dtype)
    key = (case.name, kind, dtype.name)
    if key in _FILLS:
        return _FILLS[key]
    assert kind in ("exact", "normal")
    rng = np.random.default_rng(case.n_cols % 9973 + (kind == "normal"))
    cplx = dtype.kind == "c"

    def draw(n):
        if kind == "exact":
            ch = np.array([-3, -2, -1, 1, 2, 3], dtype=np.int64)
            v = rng.choice(ch, size=n).astype(np.float64)
            if cplx:
                v = v + 1j * rng.choice(ch, size=n)
        else:
            v = rng.standard_normal(n)
            if cplx:
                v = v + 1j * rng.standard_normal(n)
        return v.astype(dtype)

    a, b = draw(case.A.nnz), draw(case.B.nnz)
    assert np.all(a != 0) and np.all(b != 0)
    a.setflags(write=False)
    b.setflags(write=False)
    _FILLS[key] = Fill(kind, a, b)
    return _FILLS[key]


# ---------------------------------------------------------------------------
# oracle: expand, sort by (row, col), reduce
# ---------------------------------------------------------------------------
Structure = namedtuple("Structure",
                       "indptr indices n_ij a_pos b_pos starts")


def expand(A_indptr, A_indices, B_indptr, B_indices, n_cols):
    """Structure of A @ B with every structurally present entry kept.
    a_pos/b_pos are the operand positions of the contributions in sorted
    (row, col) order, starts the first contribution of every entry."""
    A_indptr = np.asarray(A_indptr, dtype=np.int64)
    A_indices = np.asarray(A_indices, dtype=np.int64)
    B_indptr = np.asarray(B_indptr, dtype=np.int64)
    B_indices = np.asarray(B_indices, dtype=np.int64)
    n_rows = A_indptr.size - 1
    a_row = np.repeat(np.arange(n_rows, dtype=np.int64), np.diff(A_indptr))
    blen = (B_indptr[1:] - B_indptr[:-1])[A_indices]
    total = int(blen.sum())
    a_pos = np.repeat(np.arange(A_indices.size, dtype=np.int64), blen)
    seg = np.cumsum(blen) - blen
    b_pos = (np.repeat(B_indptr[A_indices], blen)
             + np.arange(total, dtype=np.int64) - np.repeat(seg, blen))
    key = a_row[a_pos] * np.int64(n_cols) + B_indices[b_pos]
    order = np.argsort(key, kind="stable")
    key = key[order]
    first = np.ones(total, dtype=bool)
    first[1:] = key[1:] != key[:-1]
    starts = np.nonzero(first)[0]
    ukey = key[starts]
    n_ij = np.diff(np.append(starts, total))
    rows = ukey // np.int64(n_cols)
    indptr = np.zeros(n_rows + 1, dtype=np.int64)
    np.cumsum(np.bincount(rows, minlength=n_rows), out=indptr[1:])
    return Structure(indptr, ukey - rows * np.int64(n_cols), n_ij,
                     a_pos[order], b_pos[order], starts)


def _reduce(x, starts):
    return np.add.reduceat(x, starts) if starts.size else x[:0]


def _as_int(v):
    r = np.rint(v).astype(np.int64)
    assert np.array_equal(r, v)
    return r


def exact_values(st, a, b):
    """int64 real and imaginary parts (None for real inputs) of the entries
    of ``st`` for integer-valued a, b."""
    ea, eb = a[st.a_pos], b[st.b_pos]
    if np.iscomplexobj(a):
        ar, ai = _as_int(ea.real), _as_int(ea.imag)
        br, bi = _as_int(eb.real), _as_int(eb.imag)
        return (_reduce(ar * br - ai * bi, st.starts),
                _reduce(ar * bi + ai * br, st.starts))
    return _reduce(_as_int(ea) * _as_int(eb), st.starts), None


def wide_values(st, a, b):
    """(ref, scale) in the wide type of spmv_cases._wide: ref_ij = sum_k
    a_ik b_kj and scale_ij = sum_k |a_ik| |b_kj| from the rounded inputs."""
    w = _wide(a.dtype)
    ea, eb = a[st.a_pos].astype(w), b[st.b_pos].astype(w)
    return (_reduce(ea * eb, st.starts),
            _reduce(np.abs(ea) * np.abs(eb), st.starts))


def entry_bound(dtype, n_ij, scale):
    """|got - ref| <= f (n_ij + 2) eps scale_ij, f = 4 for complex: twice
    the gamma_n bound of a sum of n_ij products (see spmv_cases.row_bound);
    valid for any summation order, atomics included."""
    dtype = np.dtype(dtype)
    f = 4.0 if dtype.kind == "c" else 1.0
    return f * (n_ij + 2) * np.finfo(dtype).eps * scale


_ST = {}
_WANT = {}


def structure(case):
    if case.name not in _ST:
        _ST[case.name] = expand(case.A.indptr, case.A.indices, case.B.indptr,
                                case.B.indices, case.n_cols)
    return _ST[case.name]


def want(case, kind, dtype):
    """Cached oracle values of the whole product for one fill."""
    key = (case.name, kind, np.dtype(dtype).name)
    if key not in _WANT:
        f = fill(case, kind, dtype)
        st = structure(case)
        _WANT[key] = (exact_values(st, f.a, f.b) if kind == "exact"
                      else wide_values(st, f.a, f.b))
    return _WANT[key]


def check_structure(st, indptr, indices, idx_dtype=None, what=""):
    indptr = np.asarray(indptr)
    indices = np.asarray(indices)
    np.testing.assert_array_equal(indptr, st.indptr, err_msg=what + " indptr")
    if idx_dtype is not None:
        assert indices.dtype == np.dtype(idx_dtype), (what, indices.dtype)
    np.testing.assert_array_equal(indices, st.indices,
                                  err_msg=what + " indices")


def check_values(kind, dtype, got, wanted, n_ij, sel=None, what=""):
    """``got`` against the oracle's values (entries ``sel`` of them)."""
    got = np.asarray(got)
    assert got.dtype == np.dtype(dtype), (what, got.dtype)
    if sel is None:
        sel = slice(None)
    if kind == "exact":
        re, im = wanted
        if im is None:
            np.testing.assert_array_equal(got, re[sel].astype(got.dtype),
                                          err_msg=what)
        else:
            np.testing.assert_array_equal(
                got.real, re[sel].astype(got.real.dtype),
                err_msg=what + " (real part)")
            np.testing.assert_array_equal(
                got.imag, im[sel].astype(got.imag.dtype),
                err_msg=what + " (imaginary part)")
        return
    ref, scale = wanted
    ref, scale, n = ref[sel], scale[sel], n_ij[sel]
    err = np.abs(got.astype(ref.dtype) - ref)
    bound = entry_bound(got.dtype, n, scale)
    bad = np.nonzero(~(err <= bound))[0]
    if bad.size:
        i = int(bad[np.argmax((err - bound)[bad])])
        raise AssertionError(
            f"{what}: {bad.size} entries outside the bound; worst entry {i} "
            f"({int(n[i])} contributions): |got - ref| = {float(err[i]):.3e}"
            f" > {float(bound[i]):.3e}, got {got[i]!r}, ref {ref[i]!r}")


def check_product(case, kind, dtype, idx_dtype, indptr, indices, vals,
                  what=""):
    """A whole product (indptr, indices, vals) against the oracle."""
    st = structure(case)
    check_structure(st, indptr, indices, idx_dtype, what)
    check_values(kind, dtype, vals, want(case, kind, dtype), st.n_ij,
                 what=what)


def entry_sel(st, rows):
    """Positions in the oracle's entry arrays of the entries of ``rows``,
    row after row."""
    rows = np.asarray(rows, dtype=np.int64)
    if rows.size == 0:
        return np.zeros(0, dtype=np.int64)
    return np.concatenate([np.arange(st.indptr[r], st.indptr[r + 1])
                           for r in rows] + [np.zeros(0, dtype=np.int64)])


# ---------------------------------------------------------------------------
# batch descriptors of the global kernels (host replica of what
# ops._spgemm_hip builds for one batch)
# ---------------------------------------------------------------------------
Batch = namedtuple("Batch", "rows tbl_off tbl_size total chunk_rowidx "
                            "chunk_ord blen_prefix pref_base a_len")


def global_batch(case, rows, tbl_size):
    rows = np.asarray(rows, dtype=np.int64)
    tbl_size = np.asarray(tbl_size, dtype=np.int64)
    blen = np.diff(case.B.indptr)
    ip, ix = case.A.indptr, case.A.indices
    pre, base, alen = [], [], []
    for r in rows:
        base.append(sum(alen))
        k = ix[ip[r]:ip[r + 1]]
        pre.append(np.cumsum(blen[k]))
        alen.append(k.size)
    nch = np.maximum((case.ub[rows] + GLOBAL_CHUNK - 1) // GLOBAL_CHUNK, 1)
    ch_row = np.repeat(np.arange(rows.size, dtype=np.int64), nch)
    ch_ord = (np.arange(int(nch.sum()), dtype=np.int64)
              - np.repeat(np.cumsum(nch) - nch, nch))
    off = np.cumsum(tbl_size) - tbl_size
    prefix = (np.concatenate(pre) if pre else np.zeros(0)).astype(np.int64)
    # the kernels read blen_prefix[pref_base + i] for i < a_len only; one
    # spare element keeps the pointer of an all-empty batch valid
    prefix = np.append(prefix, 0)
    return Batch(rows, off.astype(np.int64), tbl_size, int(tbl_size.sum()),
                 ch_row, ch_ord, prefix, np.array(base, dtype=np.int64),
                 np.array(alen, dtype=np.int64))

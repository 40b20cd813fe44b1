# SPDX-License-Identifier: Apache-2.0
"""Matrices, value fills, oracles and the launch-configuration table shared
by the general CSR SpMV tests (CPU: test_spmv_cases.py, GPU:
test_gpu_spmv.py and spmv_gridcap_worker.py).  Imports without a GPU.

Every matrix has random distinct sorted columns per row, so no affine plan
accepts it and a product through the public API runs the general kernels
of src/hip/spmv.hip.

Two fills:

exact   vals in {+-1, +-2, +-3}, x and y0 small non-zero integers (complex:
        both components).  Every partial sum is an integer far below 2^24,
        so it is exact in fp32 in any order, fused or not, atomics or not.
        The oracle is int64 arithmetic and the comparison is equality: one
        lost, duplicated or misattributed element changes an integer.
normal  standard normals.  The reference is the same (rounded) inputs
        summed in longdouble (8/16-byte types) or float64 (4/8-byte types)
        and the comparison is the per-row bound of ``row_bound``.
"""
from collections import namedtuple

import numpy as np
import scipy.sparse as sp

DTYPES = [np.float32, np.float64, np.complex64, np.complex128]
REAL_DTYPES = [np.float32, np.float64]
IDX_DTYPES = [np.int32, np.int64]

N_ROWS = 777   # odd; no multiple of 4, 64, 128 or 256
N_COLS = 531
UNIFORM_L = [1, 2, 3, 4, 7, 8, 15, 16, 31, 32, 63, 64, 127, 128, 255, 256,
             257]
COL_OFFSET = 13

# name, structure (scipy CSR of ones, int64 indptr/indices), row lengths,
# the column that exactly one row references and that row, and for the
# uniform matrices their L
Case = namedtuple("Case", "name S lens lone_col lone_row L")


# ---------------------------------------------------------------------------
# matrix builders
# ---------------------------------------------------------------------------
def from_lens(name, lens, n_cols, seed, L=None):
    """Random distinct sorted columns out of [0, n_cols - 1) for every row;
    column n_cols - 1 then replaces the largest column of one row in the
    middle, so exactly that row references it."""
    lens = np.asarray(lens, dtype=np.int64)
    n = lens.size
    rng = np.random.default_rng(seed)
    indptr = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(lens, out=indptr[1:])
    indices = np.empty(int(indptr[-1]), dtype=np.int64)
    assert lens.max(initial=0) <= n_cols - 1
    for i in range(n):
        if lens[i]:
            cols = rng.choice(n_cols - 1, size=int(lens[i]), replace=False)
            cols.sort()
            indices[indptr[i]:indptr[i + 1]] = cols
    lone_col = lone_row = None
    nonempty = np.nonzero(lens > 0)[0]
    if nonempty.size:
        lone_row = int(nonempty[nonempty.size // 2])
        lone_col = n_cols - 1
        indices[indptr[lone_row + 1] - 1] = lone_col
    S = sp.csr_array((np.ones(indices.size), indices, indptr),
                     shape=(n, n_cols))
    assert S.has_sorted_indices
    return Case(name, S, lens, lone_col, lone_row, L)


def uniform(L, parity, n_rows=N_ROWS, n_cols=N_COLS):
    """Every row of length L.  For even L, row 0 has length 1 so that row
    starts take both parities (odd L alternates by itself).  The total nnz
    is then odd for odd n_rows; parity "even" takes one element off the last
    row.  In the odd version the last pair of the value stream is the
    kernels' scalar tail (``pp + 2 > nnz``).  The maximum row length is L in
    both."""
    assert parity in ("odd", "even") and n_rows % 2 == 1 and n_rows >= 3
    lens = np.full(n_rows, L, dtype=np.int64)
    if L % 2 == 0:
        lens[0] = 1
    assert lens.sum() % 2 == 1
    if parity == "even":
        lens[-1] -= 1
    return from_lens(f"uniform{L}{parity}", lens, n_cols,
                     seed=1000 + 2 * L + (parity == "even"), L=L)


def ragged(n_rows=N_ROWS, n_cols=N_COLS):
    """Heavy-tailed lengths on 0..300 with empty rows first, last, in a run
    of four and on both sides of the wave (63/64) and block (255/256)
    edges."""
    rng = np.random.default_rng(77)
    lens = np.minimum(300, np.floor(4.0 * rng.pareto(1.1, n_rows))
                      ).astype(np.int64)
    lens[400] = 300
    for r in (0, n_rows - 1, 100, 101, 102, 103, 63, 64, 255, 256):
        lens[r] = 0
    return from_lens("ragged", lens, n_cols, seed=78)


def long_row(n_rows=N_ROWS, n_cols=6007):
    """One row of 5000 among rows of length 2: W = 64 loops 40 steps, and in
    the stream kernel the row (elements 599..5598) spans three element
    blocks at PE = 8 (2048 elements each).  Rows 0 and 400 have odd lengths
    so that row starts take both parities."""
    lens = np.full(n_rows, 2, dtype=np.int64)
    lens[0] = 1
    lens[300] = 5000
    lens[400] = 3
    return from_lens("long_row", lens, n_cols, seed=79)


def sparse_tail(n_rows=N_ROWS, n_cols=N_COLS):
    """Mean below 3 with a maximum above 31: with or without the row-length
    hint the launcher's default is the plain vector kernel at W = 1."""
    lens = np.ones(n_rows, dtype=np.int64)
    lens[::9] = 2
    lens[500] = 40
    lens[10:13] = 0
    return from_lens("sparse_tail", lens, n_cols, seed=80)


def degenerate():
    return [
        from_lens("rows0", np.zeros(0, dtype=np.int64), 5, seed=90),
        from_lens("rows1", np.array([3]), 9, seed=91),
        from_lens("empty300", np.zeros(300, dtype=np.int64), 17, seed=92),
        from_lens("one_by_one", np.array([1]), 2, seed=93),
    ]


_CASES = {}


def all_cases():
    """name -> Case, built once per process and never modified."""
    if not _CASES:
        cs = [uniform(L, p) for L in UNIFORM_L for p in ("odd", "even")]
        cs += [ragged(), long_row(), sparse_tail()] + degenerate()
        for c in cs:
            _CASES[c.name] = c
    return _CASES


def case_names():
    names = [f"uniform{L}{p}" for L in UNIFORM_L for p in ("odd", "even")]
    return names + ["ragged", "long_row", "sparse_tail", "rows0", "rows1",
                    "empty300", "one_by_one"]


def get_case(name):
    return all_cases()[name]


def max_len(case):
    return int(case.lens.max(initial=0))


# ---------------------------------------------------------------------------
# fills
# ---------------------------------------------------------------------------
Fill = namedtuple("Fill", "kind vals x y0")


def _ints(rng, n, choices):
    return rng.choice(np.asarray(choices, dtype=np.int64), size=n)


_FILLS = {}


def fill(case, kind, dtype):
    """(vals, x, y0) of ``dtype`` for ``case``; cached, read-only.  Every x
    entry is non-zero: the element before an odd row start and the one after
    a row end always contribute if a kernel wrongly takes them in."""
    dtype = np.dtype(dtype)
    key = (case.name, kind, dtype.name)
    if key in _FILLS:
        return _FILLS[key]
    nnz = case.S.nnz
    n_rows, n_cols = case.S.shape
    seed = sum(ord(ch) for ch in case.name) * 7 + (kind == "normal")
    rng = np.random.default_rng(seed)
    cplx = dtype.kind == "c"

    def draw(n, exact_choices):
        if kind == "exact":
            a = _ints(rng, n, exact_choices).astype(np.float64)
            if cplx:
                a = a + 1j * _ints(rng, n, exact_choices)
        else:
            a = rng.standard_normal(n)
            if cplx:
                a = a + 1j * rng.standard_normal(n)
        return a.astype(dtype)

    assert kind in ("exact", "normal")
    vals = draw(nnz, [-3, -2, -1, 1, 2, 3])
    x = draw(n_cols, [-3, -2, -1, 1, 2, 3])
    y0 = draw(n_rows, [-4, -3, -2, -1, 0, 1, 2, 3, 4])
    assert np.all(x != 0) and np.all(vals != 0)
    for a in (vals, x, y0):
        a.setflags(write=False)
    _FILLS[key] = Fill(kind, vals, x, y0)
    return _FILLS[key]


# ---------------------------------------------------------------------------
# oracles
# ---------------------------------------------------------------------------
def seg_sum(a, indptr):
    """Per-row sums of ``a`` in a's own dtype (empty rows give 0)."""
    indptr = np.asarray(indptr)
    out = np.zeros(indptr.size - 1, dtype=a.dtype)
    ne = np.diff(indptr) > 0
    if a.size:
        out[ne] = np.add.reduceat(a, indptr[:-1][ne])
    return out


def exact_oracle(case, vals, x, y0, accumulate):
    """Integer arithmetic on the integer-valued inputs.  Returns the real
    and the imaginary part as int64 (imaginary None for real inputs)."""
    ip, ix = case.S.indptr, case.S.indices

    def as_int(a):
        r = np.rint(a).astype(np.int64)
        assert np.array_equal(r, a)
        return r

    xg = x[ix]
    if np.iscomplexobj(vals):
        ar, ai = as_int(vals.real), as_int(vals.imag)
        br, bi = as_int(xg.real), as_int(xg.imag)
        re = seg_sum(ar * br - ai * bi, ip)
        im = seg_sum(ar * bi + ai * br, ip)
        if accumulate:
            re = re + as_int(y0.real)
            im = im + as_int(y0.imag)
        return re, im
    re = seg_sum(as_int(vals) * as_int(xg), ip)
    if accumulate:
        re = re + as_int(y0)
    return re, None


def check_exact(got, want, what=""):
    re, im = want
    got = np.asarray(got)
    if im is None:
        np.testing.assert_array_equal(got, re.astype(got.dtype),
                                      err_msg=what)
    else:
        np.testing.assert_array_equal(got.real, re.astype(got.real.dtype),
                                      err_msg=what + " (real part)")
        np.testing.assert_array_equal(got.imag, im.astype(got.imag.dtype),
                                      err_msg=what + " (imaginary part)")


def _wide(dtype):
    """The reference precision of ``dtype``: longdouble for 8-byte reals and
    16-byte complex, float64 for 4-byte reals and 8-byte complex."""
    dtype = np.dtype(dtype)
    if dtype == np.float32:
        return np.dtype(np.float64)
    if dtype == np.complex64:
        return np.dtype(np.complex128)
    if np.finfo(np.longdouble).eps > 2.0 ** -63:
        raise RuntimeError("the fp64 reference needs an extended-precision "
                           "numpy longdouble")
    return np.dtype(np.clongdouble if dtype.kind == "c" else np.longdouble)


def reference(case, vals, x, y0, accumulate):
    """(ref, scale) in the wide type: ref_i = sum_j a_ij x_j (+ y0_i) and
    scale_i = sum_j |a_ij| |x_j| (+ |y0_i|), both from the rounded inputs.
    Its own rounding error is below n_i * eps(wide) * scale_i, at least
    2^11 times less than the bound it is used in."""
    ip, ix = case.S.indptr, case.S.indices
    w = _wide(vals.dtype)
    a = vals.astype(w)
    b = x.astype(w)[ix]
    ref = seg_sum(a * b, ip)
    scale = seg_sum(np.abs(a) * np.abs(b), ip)
    if accumulate:
        ref = ref + y0.astype(w)
        scale = scale + np.abs(y0.astype(w))
    return ref, scale


def row_bound(case, dtype, scale):
    """|got_i - ref_i| <= (n_i + 2) * eps(dtype) * scale_i: twice the
    gamma_n bound of a length-n_i sum of products (n_i multiplications,
    n_i - 1 additions and the addition to y0, each within eps / 2), valid
    for any summation order, with or without contraction.  Complex types
    take a further factor 4 for the component-wise product."""
    dtype = np.dtype(dtype)
    eps = np.finfo(dtype).eps
    factor = 4.0 if dtype.kind == "c" else 1.0
    return factor * (case.lens + 2) * eps * scale


def check_bound(case, got, ref, scale, what=""):
    got = np.asarray(got)
    err = np.abs(got.astype(ref.dtype) - ref)
    bound = row_bound(case, got.dtype, scale)
    bad = np.nonzero(~(err <= bound))[0]
    if bad.size:
        i = int(bad[np.argmax((err - bound)[bad])])
        raise AssertionError(
            f"{what}: {bad.size} rows outside the bound; worst row {i} "
            f"(length {int(case.lens[i])}): |got - ref| = {float(err[i]):.3e}"
            f" > {float(bound[i]):.3e}, got {got[i]!r}, ref {ref[i]!r}")


# ---------------------------------------------------------------------------
# NaN containment
# ---------------------------------------------------------------------------
Poison = namedtuple("Poison", "vals x nan_rows clean_rows")


def poison(case, vals, x):
    """NaN in three places, or None where the matrix has no room for them:

    - the stored value just BEFORE an odd row start s (the pair kernels of
      the row starting at s load it as the first half of their first pair
      and must drop it by ``pp >= s``),
    - the stored value AT another odd row start (the row before loads it as
      the second half of its last pair and must drop it by ``pp + 1 < e``),
    - the x entry that exactly one row references.

    Exactly the rows that own these become NaN; ``clean_rows`` are the
    neighbours that a wrong guard would contaminate."""
    ip, lens = case.S.indptr, case.lens
    n = lens.size
    if case.lone_row is None or n < 8:
        return None
    cand = [r for r in range(1, n)
            if ip[r] % 2 == 1 and lens[r] > 0 and lens[r - 1] > 0
            and case.lone_row not in (r - 1, r)]
    if len(cand) < 2:
        return None
    ra = cand[0]
    later = [r for r in cand if r >= ra + 3]
    if not later:
        return None
    rb = later[len(later) // 2]
    v = vals.copy()
    xx = x.copy()
    v[ip[ra] - 1] = np.nan       # owned by row ra - 1
    v[ip[rb]] = np.nan           # owned by row rb
    xx[case.lone_col] = np.nan   # read by lone_row only
    return Poison(v, xx, sorted({ra - 1, rb, case.lone_row}),
                  sorted({ra, rb - 1}))


def check_poison(case, got, p, want_exact, what=""):
    got = np.asarray(got)
    isnan = np.isnan(got)
    np.testing.assert_array_equal(
        np.nonzero(isnan)[0], np.asarray(p.nan_rows),
        err_msg=what + ": NaN rows")
    keep = ~isnan
    re, im = want_exact
    if im is None:
        np.testing.assert_array_equal(got[keep], re[keep].astype(got.dtype),
                                      err_msg=what)
    else:
        np.testing.assert_array_equal(got.real[keep], re[keep], err_msg=what)
        np.testing.assert_array_equal(got.imag[keep], im[keep], err_msg=what)


# ---------------------------------------------------------------------------
# launch configurations (ops.spmv: pair, w_override, nt, swz)
# ---------------------------------------------------------------------------
# cap: the longest row the kernel handles (None: any); a hint beyond it is
# outside the kernel's contract, so configs_for never offers it.
# real_only: complex dtypes fall through to the vector kernel.
Config = namedtuple("Config", "name pair w_override nt swz cap real_only")

WIDTHS = [1, 2, 4, 8, 16, 32, 64]
PAIR_CAPACITY = {5: 7, 6: 15, 7: 15, 8: 31}


def _table():
    t = []
    for w in WIDTHS:
        t.append(Config(f"vector_w{w}", 0, w, False, 0, None, False))
        t.append(Config(f"vector_nt_w{w}", 0, w, True, 0, None, False))
        t.append(Config(f"vector_swz_w{w}", 0, w, False, 1, None, False))
        t.append(Config(f"pair_w{w}", 1, w, False, 0, None, True))
        t.append(Config(f"pair_swz_w{w}", 1, w, False, 1, None, True))
        t.append(Config(f"pair2_w{w}", 4, w, False, 0, None, True))
    t.append(Config("sten_np4", 5, 0, False, 0, PAIR_CAPACITY[5], True))
    t.append(Config("sten_np8", 6, 0, False, 0, PAIR_CAPACITY[6], True))
    t.append(Config("pairu_w2", 7, 0, False, 0, PAIR_CAPACITY[7], True))
    t.append(Config("pairu_w4", 8, 0, False, 0, PAIR_CAPACITY[8], True))
    t.append(Config("stream_pe8", 2, 0, False, 0, None, True))
    t.append(Config("stream_pe16", 3, 0, False, 0, None, True))
    return t


CONFIGS = _table()
CONFIG_BY_NAME = {c.name: c for c in CONFIGS}


def fits(cfg, case):
    return cfg.cap is None or max_len(case) <= cfg.cap


def configs_for(case):
    return [c for c in CONFIGS if fits(c, case)]


def auto_width(case):
    """The launcher's default W: the largest power of two <= 64 with
    4 W <= mean row length, 1 at the least."""
    n = case.lens.size
    mean = case.S.nnz / n if n else 0.0
    w = 1
    while w < 64 and 4 * w <= mean:
        w *= 2
    return w


def expected_kernel(cfg, case, is_real, accumulate):
    """(kernel, W) that the launcher must pick for an explicit table
    configuration, stated independently of the C++ selection."""
    w = cfg.w_override if cfg.w_override else auto_width(case)
    vec = ("vector_nt" if cfg.nt else
           "vector_swz" if cfg.swz == 1 else "vector")
    if not is_real:
        return vec, w
    if cfg.pair in (2, 3):
        # stream needs a zeroed y and at least one row
        if accumulate or case.lens.size == 0:
            return vec, w
        return "stream", 8 if cfg.pair == 2 else 16
    if cfg.pair == 5:
        return "sten", 4
    if cfg.pair == 6:
        return "sten", 8
    if cfg.pair == 7:
        return "pairu", 2
    if cfg.pair == 8:
        return "pairu", 4
    if cfg.pair == 4:
        return "pair2", w
    if cfg.pair == 1:
        return ("pair_swz" if cfg.swz == 1 else "pair"), w
    return vec, w


def expected_auto(case, is_real, max_nnz):
    """(kernel, W) of pair=-1, w_override=0, nt=False, swz=0."""
    n = case.lens.size
    mean = case.S.nnz / n if n else 0.0
    w = auto_width(case)
    if not is_real:
        return "vector", w
    if 0 <= max_nnz <= 7:
        return "sten", 4
    if 0 <= max_nnz <= 15:
        return "pairu", 2
    if 0 <= max_nnz <= 31:
        return "pairu", 4
    return ("pair" if mean >= 3.0 else "vector"), w

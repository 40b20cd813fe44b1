# SPDX-License-Identifier: Apache-2.0
"""Internal op dispatch: HIP kernels on GPU, C++/OpenMP or torch on CPU.

Each op here corresponds to one task class of the reference's C++ layer
(SURVEY §2.2/§2.3): CSRSpMVRowSplit → ``spmv``; SpGEMMCSRxCSRxCSR{NNZ,} →
``spgemm_local``; CSRToDense/DenseToCSR → conversions; GetCSRDiagonal →
``diagonal``; AXPBY → ``axpby``; plus the dot/norm block-reductions feeding
RCCL all-reduce.

GPU tensors REQUIRE the in-tree HIP extension — there is no silent eager
fallback (set LS_FORCE_FALLBACK=1 explicitly to debug against torch).
"""
from __future__ import annotations

from typing import Optional, Tuple

import torch

from . import _cext
from .settings import settings

_DTYPE_CODE = {
    torch.float32: 0,
    torch.float64: 1,
    torch.complex64: 2,
    torch.complex128: 3,
}

_IDX_CODE = {torch.int32: 0, torch.int64: 1}


def _code(t: torch.Tensor) -> int:
    return _DTYPE_CODE[t.dtype]


def _icode(t: torch.Tensor) -> int:
    return _IDX_CODE[t.dtype]


def _use_hip(t: torch.Tensor) -> bool:
    return t.is_cuda and not settings.force_cpu_fallback


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


# ---------------------------------------------------------------------------
# SpMV: y[i] (+)= sum_j vals[jp] * x[indices[jp]]   (rows local, x gathered)
# ---------------------------------------------------------------------------
def spmv(indptr: torch.Tensor, indices: torch.Tensor, vals: torch.Tensor,
         x: torch.Tensor, y: Optional[torch.Tensor] = None,
         accumulate: bool = False, w_override: int = 0,
         nt: bool = False, pair: int = -1, swz: int = 0,
         col_offset: int = 0, max_nnz: int = -1,
         affine=None, dot_out: Optional[torch.Tensor] = None,
         affine_const=None) -> torch.Tensor:
    """col_offset: kernels read x[c - col_offset] for global column c —
    realized as an adjusted base pointer, the same "fake offset dense
    pointer" trick the reference plays on cuSPARSE (spmv.cu:75-90).

    General kernels (GPU, no ``affine``; ``ext.spmv_select`` with the same
    arguments returns the (kernel, W) a call runs).  ``pair`` selects:

    ====  ==========================================  ==================
    pair  kernel                                      longest row
    ====  ==========================================  ==================
     -1   launcher's choice (below)                   any
      0   vector, sub-wave of W lanes per row         any
      1   pair, W lanes x 2 elements per step         any
      2   stream, 2048 elements per block (PE = 8)    any
      3   stream, 4096 elements per block (PE = 16)   any
      4   pair2, a sub-wave serves two rows           any
      5   sten, one lane per row, 4 pairs             7
      6   sten, one lane per row, 8 pairs             15
      7   pairu, 2 lanes per row, 4 pairs each        15
      8   pairu, 4 lanes per row, 4 pairs each        31
    ====  ==========================================  ==================

    Codes 1..8 are for real dtypes; complex values run the vector kernel
    whatever ``pair`` says.  Stream writes boundary rows with atomics into
    a zeroed y, so with ``accumulate`` codes 2 and 3 run the vector kernel
    too.  Codes 5..8 read a fixed number of pairs per row and DROP THE
    ELEMENTS of any longer row without a diagnostic: pass them only for a
    matrix whose longest row fits.

    ``pair=-1``: W is the largest power of two <= 64 with 4 W <= mean row
    length; real dtypes take pair (mean >= 3) or vector at that W, unless
    ``max_nnz >= 0`` says that the longest row has at most 7 / 15 / 31
    elements, which selects code 5 / 7 / 8.  ``max_nnz`` is trusted, not
    checked: a value smaller than the true maximum drops elements silently
    (-1: unknown, never selects 5..8).

    ``w_override`` > 0 replaces W for vector, pair and pair2; a value that
    is not a power of two <= 64 runs as 64.  ``nt`` (non-temporal loads)
    and ``swz=1`` (XCD block remap) apply to the vector kernel, ``swz=1``
    also to pair; ``nt`` wins over ``swz``.  LS_SPMV_GRID caps the grid
    (default 8192 blocks; read once per process).

    ``affine``: stencil plan (csr._affine_plan) — rows with columns ==
    row + D[j] skip the index stream entirely (8 B/nnz instead of
    12 B/nnz), and whole tiles of such rows skip indptr and the mask as
    well (plan.tile_base); exception rows run from a row list.

    ``affine_const``: constant-tile table of ``vals`` under ``affine``
    (csr._AffineConst) -- full tiles whose rows all hold the same values
    read no value stream.  It is used only if it was built from this
    plan and from a tensor at ``vals.data_ptr()`` whose torch ``_version``
    is still the recorded one; anything else is
    ignored and the call runs as without it.  LS_SPMV_AFFINE_CONST=0
    ignores it always (in-build A/B), and so does LS_SPMV_AFFINE_TILES=0.
    With the table and without dot fusion a wave takes
    ``ext.affine_group(nd, dtype)`` tiles at a time (where that is > 1)
    and the exception rows run inside the same launch;
    LS_SPMV_AFFINE_GROUP=1 runs the one-tile kernel and its separate
    row-list launch, LS_SPMV_AFFINE_FOLD=0 only the latter.
    """
    n_rows = indptr.numel() - 1
    if y is None:
        y = torch.empty(n_rows, dtype=vals.dtype, device=vals.device)
        accumulate = False
    x_ptr = x.data_ptr() - int(col_offset) * x.element_size()
    if _use_hip(vals):
        ext = _cext.require_hip()
        if affine is not None and pair < 0 and w_override == 0:
            nd, D, mask, rest, xconsec = affine[:5]
            import os as _os
            v2 = _os.environ.get("LS_SPMV_AFFINE_V", "1") == "2" and \
                not vals.is_complex()
            # LS_SPMV_AFFINE_TILES=0: null tile table, every tile takes
            # the per-row (mixed) path — in-build A/B of the tile table
            tiles = (getattr(affine, "tile_base", None)
                     if _os.environ.get("LS_SPMV_AFFINE_TILES", "1") != "0"
                     else None)
            cst = affine_const
            if cst is not None and (
                    tiles is None or v2 or vals.is_complex()
                    or cst.plan is not affine
                    or cst.data_ptr != vals.data_ptr()
                    or cst.version != vals._version
                    or _os.environ.get("LS_SPMV_AFFINE_CONST", "1") == "0"):
                cst = None
            fuse_dot = (dot_out is not None and not accumulate
                        and not v2 and not vals.is_complex())
            # LS_SPMV_AFFINE_GROUP=1: the one-tile-per-wave kernel instead
            # of the tile-group kernel (in-build A/B)
            group = 1 if _os.environ.get("LS_SPMV_AFFINE_GROUP") == "1" else 0
            # the exception rows ride in the tile-group launch
            # (LS_SPMV_AFFINE_FOLD=0: own launch); the fused dot needs
            # them first and has no tile groups
            fold = (cst is not None and not fuse_dot and not group
                    and rest.numel() > 0
                    and ext.affine_group(int(nd), _code(vals)) > 1
                    and _os.environ.get("LS_SPMV_AFFINE_FOLD", "1") != "0")
            if fuse_dot and rest.numel():
                # exception rows FIRST so the fused x.y reduction over
                # non-mask rows reads final y values
                ext.spmv_rows(rest.data_ptr(), rest.numel(),
                              indptr.data_ptr(), indices.data_ptr(),
                              vals.data_ptr(), x_ptr, y.data_ptr(),
                              _code(vals), _icode(indices), accumulate,
                              _stream())
            if v2:
                x_hi = int(col_offset) + x.numel()
                ext.spmv_affine2(indptr.data_ptr(), vals.data_ptr(),
                                 x_ptr, y.data_ptr(), D.data_ptr(),
                                 mask.data_ptr(), n_rows, vals.numel(),
                                 x_hi, int(nd), bool(xconsec),
                                 _code(vals), accumulate, _stream())
            else:
                if fuse_dot:
                    dot_out.zero_()
                ext.spmv_affine(indptr.data_ptr(), vals.data_ptr(), x_ptr,
                                y.data_ptr(), D.data_ptr(),
                                mask.data_ptr(),
                                cst.tile_cbase.data_ptr() if cst is not None
                                else tiles.data_ptr() if tiles is not None
                                else 0,
                                n_rows, int(nd), _code(vals), accumulate,
                                dot_out.data_ptr() if fuse_dot else 0,
                                cst.C.data_ptr() if cst is not None else 0,
                                rest.data_ptr() if fold else 0,
                                rest.numel() if fold else 0,
                                indices.data_ptr() if fold else 0,
                                _icode(indices), group, _stream())
            if rest.numel() and not fuse_dot and not fold:
                ext.spmv_rows(rest.data_ptr(), rest.numel(),
                              indptr.data_ptr(), indices.data_ptr(),
                              vals.data_ptr(), x_ptr, y.data_ptr(),
                              _code(vals), _icode(indices), accumulate,
                              _stream())
            if dot_out is not None and not fuse_dot:
                vdot(x, y, conj=False, out=dot_out)
            return y
        ext.spmv(indptr.data_ptr(), indices.data_ptr(), vals.data_ptr(),
                 x_ptr, y.data_ptr(), n_rows, vals.numel(),
                 _code(vals), _icode(indices), accumulate, _stream(),
                 int(w_override), bool(nt), int(pair), int(swz),
                 int(max_nnz))
        if dot_out is not None:
            vdot(x, y, conj=False, out=dot_out)
        return y
    if not vals.is_cuda and _cext.has_cpu():
        _cext.require_cpu().spmv(indptr.data_ptr(), indices.data_ptr(),
                                 vals.data_ptr(), x_ptr, y.data_ptr(),
                                 n_rows, _code(vals), _icode(indices),
                                 accumulate)
        return y
    # torch fallback (debug / extension-less CPU)
    prod = vals * x[(indices.long() - col_offset)]
    row_ids = torch.repeat_interleave(
        torch.arange(n_rows, device=vals.device),
        (indptr[1:] - indptr[:-1]),
    )
    if not accumulate:
        y.zero_()
    y.index_add_(0, row_ids, prod)
    return y


# ---------------------------------------------------------------------------
# SpMM: Y[i, :] (+)= sum_j vals[jp] * X[indices[jp], :]   (X, Y row-major)
# ---------------------------------------------------------------------------
# the narrow/wide crossover of path="auto": k <= this takes the narrow
# kernel (row split over a sub-wave, K accumulators per lane), larger k the
# wide one (lanes over columns)
SPMM_NARROW_MAX = 4
# largest k that path="narrow" accepts: the K values the narrow kernel is
# instantiated for (the extension exports the same number and refuses more)
SPMM_NARROW_KMAX = 8

_SPMM_PATHS = ("auto", "narrow", "wide")


def spmm(indptr: torch.Tensor, indices: torch.Tensor, vals: torch.Tensor,
         X: torch.Tensor, Y: Optional[torch.Tensor] = None,
         accumulate: bool = False, col_offset: int = 0,
         path: str = "auto") -> torch.Tensor:
    """CSR x dense block.  ``X`` is a row-major window whose row
    ``c - col_offset`` holds global column ``c`` — an adjusted base pointer
    as in ``spmv``, shifted by ``col_offset * k`` elements.

    ``path`` forces the HIP kernel ("narrow" | "wide"); "auto" picks narrow
    for k <= SPMM_NARROW_MAX.  It is validated on every route so a typo
    never passes silently on CPU."""
    if path not in _SPMM_PATHS:
        raise ValueError(f"spmm path must be one of {_SPMM_PATHS}, "
                         f"got {path!r}")
    if X.ndim != 2 or not X.is_contiguous():
        raise ValueError("spmm needs a contiguous row-major 2-D X")
    n_rows = indptr.numel() - 1
    k = int(X.shape[1])
    if path == "narrow" and k > SPMM_NARROW_KMAX:
        raise ValueError(f"spmm path 'narrow' supports k <= "
                         f"{SPMM_NARROW_KMAX}, got k = {k}")
    if Y is None:
        Y = torch.empty((n_rows, k), dtype=vals.dtype, device=vals.device)
        accumulate = False
    elif (Y.ndim != 2 or tuple(Y.shape) != (n_rows, k)
          or not Y.is_contiguous()):
        raise ValueError(f"spmm needs a contiguous ({n_rows}, {k}) Y")
    if n_rows == 0 or k == 0:
        return Y
    if vals.numel() == 0:
        # nothing to gather (and X may be an empty window with no storage)
        if not accumulate:
            Y.zero_()
        return Y
    x_ptr = X.data_ptr() - int(col_offset) * k * X.element_size()
    if _use_hip(vals):
        ext = _cext.require_hip()
        narrow = path == "narrow" or (path == "auto"
                                      and k <= SPMM_NARROW_MAX)
        ext.spmm(indptr.data_ptr(), indices.data_ptr(), vals.data_ptr(),
                 x_ptr, Y.data_ptr(), n_rows, vals.numel(), k,
                 int(col_offset), int(X.shape[0]), _code(vals),
                 _icode(indices), accumulate, 0 if narrow else 1, _stream())
        return Y
    if not vals.is_cuda and _cext.has_cpu():
        _cext.require_cpu().spmm(indptr.data_ptr(), indices.data_ptr(),
                                 vals.data_ptr(), x_ptr, Y.data_ptr(),
                                 n_rows, k, _code(vals), _icode(indices),
                                 accumulate)
        return Y
    # torch fallback (debug / extension-less CPU)
    prod = vals.unsqueeze(1) * X[(indices.long() - col_offset)]
    row_ids = torch.repeat_interleave(
        torch.arange(n_rows, device=vals.device),
        (indptr[1:] - indptr[:-1]),
    )
    if not accumulate:
        Y.zero_()
    Y.index_add_(0, row_ids, prod)
    return Y


# ---------------------------------------------------------------------------
# SpGEMM (local rows of A) x (gathered rows of B) -> local rows of C
# ---------------------------------------------------------------------------
def spgemm_local(
    A_indptr: torch.Tensor, A_indices: torch.Tensor, A_vals: torch.Tensor,
    B_indptr: torch.Tensor, B_indices: torch.Tensor, B_vals: torch.Tensor,
    n_colsB: int, b_row_offset: int = 0, cache=None,
) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """Gustavson 2-phase.  B rows are indexed by A's GLOBAL column ids;
    when only the window [b_row_offset, ...) of B's rows was gathered,
    the kernels see an offset indptr base pointer (windowed B-row image,
    reference csr.py:656-666)."""
    n_rows = A_indptr.numel() - 1
    dev = A_vals.device
    bp_ptr = B_indptr.data_ptr() - int(b_row_offset) * 8
    if _use_hip(A_vals):
        return _spgemm_hip(A_indptr, A_indices, A_vals, B_indptr, B_indices,
                           B_vals, n_colsB, bp_ptr, b_row_offset,
                           cache=cache)
    if not A_vals.is_cuda and _cext.has_cpu():
        ext = _cext.require_cpu()
        row_nnz = torch.empty(n_rows, dtype=torch.int64)
        ext.spgemm_symbolic(A_indptr.data_ptr(), A_indices.data_ptr(),
                            n_rows, bp_ptr,
                            B_indices.data_ptr(), int(n_colsB),
                            row_nnz.data_ptr(), _icode(A_indices))
        C_indptr = torch.zeros(n_rows + 1, dtype=torch.int64)
        torch.cumsum(row_nnz, dim=0, out=C_indptr[1:])
        nnz = int(C_indptr[-1])
        C_indices = torch.empty(nnz, dtype=A_indices.dtype)
        C_vals = torch.empty(nnz, dtype=A_vals.dtype)
        ext.spgemm_numeric(A_indptr.data_ptr(), A_indices.data_ptr(),
                           A_vals.data_ptr(), n_rows, bp_ptr,
                           B_indices.data_ptr(), B_vals.data_ptr(),
                           int(n_colsB), C_indptr.data_ptr(),
                           C_indices.data_ptr(), C_vals.data_ptr(),
                           _code(A_vals), _icode(A_indices))
        return C_indptr, C_indices, C_vals
    # torch fallback: ESC (expand - sort - compress), works on any device.
    return _spgemm_esc(A_indptr, A_indices, A_vals, B_indptr, B_indices,
                       B_vals, n_colsB, b_row_offset)


def spgemm_affine_try(A_indptr, A_vals, planA, B_indptr, B_vals, planB,
                      n_rowsB, n_colsB,
                      general_rows_fn, idx_dtype, cache=None,
                      b_row_off=0):
    """C = A @ B via the stencil-convolution kernel when BOTH operands
    are affine: C's columns per valid row are the sorted offset sum-set
    E = unique(DA + DB); the numeric phase is ndA*ndB FMAs into nE LDS
    accumulators per row — no hash tables, no index-stream reads, sorted
    output by construction.  Exception rows (A/B boundary rows,
    edge-of-matrix columns) are computed by ``general_rows_fn(rows) ->
    (ip, idx, vals)`` over an A-submatrix and merged in.  Returns
    (C_ip, C_idx, C_vals) or None when the plan does not apply.

    The structure prefix (sum-set, validity, C indptr) is cached per
    (A,B) structure like the general path's binning cache."""
    import os as _os
    if _os.environ.get("LS_SPGEMM_AFFINE", "1") in ("0", "false"):
        return None
    if planA is None or planB is None:
        return None
    if not _use_hip(A_vals):
        return None
    dev = A_vals.device
    n_rows = A_indptr.numel() - 1
    ndA, DA, maskA, _, _ = planA
    ndB, DB, maskB, _, _ = planB
    hit = cache is not None and "aff" in cache
    if hit:
        st_c = cache["aff"]
        if st_c is None:
            return None  # plan previously rejected (nE too large)
        (E_dev, ps_dev, validC, C_ip_c, nnz, rows_g, src_off,
         DA_dev, slot_a, slot_b, soff) = st_c
    else:
        # planB was detected on the (possibly windowed) B tensors where
        # row ids are window-local: D_win = col - (k - b_row_off), so
        # the GLOBAL offset is D_win - b_row_off
        E_all = DA.long().reshape(-1, 1) + (
            DB.long() - int(b_row_off)).reshape(1, -1)
        E = torch.unique(E_all.reshape(-1))          # sorted unique
        nE = E.numel()
        # LDS accumulator budget: nE * LS_THREADS * elsize <= 51 KB
        # (fp64: nE <= 25; complex128: nE <= 12)
        if nE * 256 * A_vals.element_size() > 51 * 1024:
            if cache is not None:
                cache["aff"] = None
            return None
        ps_dev = torch.searchsorted(E, E_all.reshape(-1)).to(
            torch.int16).to(dev).contiguous()
        E_dev = E.to(torch.int32).to(dev).contiguous()
        # validity: A row affine; every touched B row in-range and
        # affine; every output column in [0, n_colsB)
        # B rows may be a gathered WINDOW starting at global row
        # b_row_off: mask indices are window-local, k stays global
        idx = torch.arange(n_rows, device=dev)
        valid = maskA.bool().clone()
        mB = maskB.bool()
        for a in DA.tolist():
            k = idx + int(a)                       # global B row id
            kw = k - int(b_row_off)                # window-local
            okk = (kw >= 0) & (kw < n_rowsB)
            kb = torch.where(okk, kw, torch.zeros_like(kw))
            valid &= okk & mB[kb]
        e_lo, e_hi = int(E[0]), int(E[-1])
        valid &= (idx + e_lo >= 0) & (idx + e_hi < n_colsB)
        validC = valid.to(torch.uint8).contiguous()
        rows_g = torch.nonzero(~valid).reshape(-1).contiguous()
        DA_dev = DA.to(torch.int32).to(dev).contiguous()
        # slot-CSR for the output-centric kernel: pairs grouped by slot
        order = torch.argsort(ps_dev.int(), stable=True)
        slot_a = (order // ndB).to(torch.int16).contiguous()
        slot_b = (order % ndB).to(torch.int16).contiguous()
        soff = torch.zeros(int(E.numel()) + 1, dtype=torch.int32,
                           device=dev)
        cnts = torch.bincount(ps_dev.long(), minlength=int(E.numel()))
        soff[1:] = torch.cumsum(cnts, dim=0).to(torch.int32)
    # exception rows always recompute numerically (values change);
    # their STRUCTURE is deterministic so C_ip/src_off cache cleanly
    sub = general_rows_fn(rows_g) if rows_g.numel() else None
    if sub is not None:
        sub_ip, sub_idx, sub_vals = sub
        if sub_idx.dtype != idx_dtype:
            sub_idx = sub_idx.to(idx_dtype)
    if not hit:
        nE_t = torch.full((n_rows,), E_dev.numel(), dtype=torch.int64,
                          device=dev)
        cnt = torch.where(validC.bool(), nE_t, torch.zeros_like(nE_t))
        if sub is not None:
            cnt[rows_g] = sub_ip[1:] - sub_ip[:-1]
        C_ip_c = torch.zeros(n_rows + 1, dtype=torch.int64, device=dev)
        torch.cumsum(cnt, dim=0, out=C_ip_c[1:])
        nnz = int(C_ip_c[-1].item())
        src_off = None
        if sub is not None:
            src_off = torch.zeros(n_rows, dtype=torch.int64, device=dev)
            src_off[rows_g] = sub_ip[:-1]
        if cache is not None:
            cache["aff"] = (E_dev, ps_dev, validC, C_ip_c, nnz, rows_g,
                            src_off, DA_dev, slot_a, slot_b, soff)
    ext = _cext.require_hip()
    st = _stream()
    C_ip = C_ip_c.clone()  # never alias the cached structure
    C_idx = torch.empty(nnz, dtype=idx_dtype, device=dev)
    C_vals = torch.empty(nnz, dtype=A_vals.dtype, device=dev)
    bp_ptr = B_indptr.data_ptr() - int(b_row_off) * 8
    if _os.environ.get("LS_SPGEMM_AFFINE_K", "lds") == "out":
        ext.spgemm_affine_out(A_indptr.data_ptr(), A_vals.data_ptr(),
                              bp_ptr, B_vals.data_ptr(),
                              DA_dev.data_ptr(), soff.data_ptr(),
                              slot_a.data_ptr(), slot_b.data_ptr(),
                              int(E_dev.numel()), E_dev.data_ptr(),
                              validC.data_ptr(), C_ip.data_ptr(),
                              C_idx.data_ptr(), C_vals.data_ptr(),
                              n_rows, _code(A_vals),
                              _IDX_CODE[idx_dtype], st)
    else:
        ext.spgemm_affine(A_indptr.data_ptr(), A_vals.data_ptr(),
                          bp_ptr, B_vals.data_ptr(),
                          DA_dev.data_ptr(), int(ndA), int(ndB),
                          ps_dev.data_ptr(), int(E_dev.numel()),
                          E_dev.data_ptr(), validC.data_ptr(),
                          C_ip.data_ptr(), C_idx.data_ptr(),
                          C_vals.data_ptr(), n_rows, _code(A_vals),
                          _IDX_CODE[idx_dtype], st)
    if sub is not None:
        ext.spgemm_compact_rows(
            rows_g.data_ptr(), rows_g.numel(), src_off.data_ptr(),
            C_ip.data_ptr(), sub_idx.data_ptr(), sub_vals.data_ptr(),
            C_idx.data_ptr(), C_vals.data_ptr(), _code(A_vals),
            _IDX_CODE[idx_dtype], st)
    return C_ip, C_idx, C_vals


def _spgemm_hip(A_indptr, A_indices, A_vals, B_indptr, B_indices, B_vals,
                n_colsB, bp_ptr=None, b_row_offset=0, cache=None):
    """Binned hash-table Gustavson on gfx950 (src/hip/spgemm.hip).

    Rows are binned by their expansion upper bound so the per-row hash
    table fits LDS (sorted output via in-LDS bitonic); oversize rows fall
    back to an HBM workspace table and are canonically sorted afterwards.

    Two modes (the analogue of the reference's cuSPARSE ALG1/ALG3 switch,
    spgemm_csr_csr_csr.cu:196-216, selected by LS_FAST_SPGEMM):
      exact (default): symbolic pass -> exact allocation -> numeric
      fast:            allocate by upper bound (memory-hungry), numeric
                       counts exact nnz, compact afterwards — skips the
                       whole symbolic pass."""
    import os as _os
    import time as _time
    _timing = _os.environ.get("LS_SPGEMM_TIMING") == "1"

    def _tick(label, _last=[None]):
        if not _timing:
            return
        torch.cuda.synchronize()
        now = _time.perf_counter()
        if _last[0] is not None:
            print(f"  [spgemm] {label}: {(now - _last[0])*1e3:.1f} ms",
                  flush=True)
        _last[0] = now

    ext = _cext.require_hip()
    dev = A_vals.device
    st = _stream()
    n_rows = A_indptr.numel() - 1
    code = _code(A_vals)
    icode = _icode(A_indices)
    _tick(None)
    assert A_indices.dtype == B_indices.dtype
    if n_colsB >= 2 ** 32:
        raise NotImplementedError("SpGEMM requires B.shape[1] < 2^32")
    if bp_ptr is None:
        bp_ptr = B_indptr.data_ptr()
    fast = settings.fast_spgemm
    pack = 1 if n_colsB < (1 << 24) - 1 else 0

    # structure cache (repeated products on unchanged sparsity — the
    # analogue of the reference's Legion partition caching that its
    # --stable microbenchmark mode exploits): binning, batches and the
    # symbolic result depend only on A/B STRUCTURE, so a cache hit skips
    # row_ub, binning and the whole symbolic phase.
    hit = (not fast) and cache is not None and "C_indptr" in cache
    if hit:
        ub = cache["ub"]
        groups = cache["groups"]
        g_batches = cache["g_batches"]
        g_keys = cache["g_keys"]
        _tick("cache_hit")
    else:
        # fused phase 0: ub + bin histogram in ONE kernel pass over A
        ub = torch.empty(n_rows, dtype=torch.int64, device=dev)
        counts_d = torch.zeros(8, dtype=torch.int64, device=dev)
        ext.spgemm_row_ub_bins(A_indptr.data_ptr(), A_indices.data_ptr(),
                               bp_ptr, ub.data_ptr(), n_rows,
                               counts_d.data_ptr(), icode, st)
        _tick("row_ub+count")
        counts = counts_d.cpu().tolist()
        bases = [0]
        for c in counts[:-1]:
            bases.append(bases[-1] + int(c))
        cursors = torch.tensor(bases, dtype=torch.int64, device=dev)
        rows_out = torch.empty(n_rows, dtype=torch.int64, device=dev)
        ext.spgemm_bin_scatter(A_indptr.data_ptr(), ub.data_ptr(), n_rows,
                               cursors.data_ptr(), rows_out.data_ptr(), st)
        groups = [rows_out[bases[i]:bases[i] + int(counts[i])]
                  for i in range(8)]
    mbins = groups[:3]          # merge W=8/32/64
    bins = groups[3:7]          # LDS-hash cfg0..3
    rows_g = groups[7].contiguous()

    row_nnz = torch.zeros(n_rows, dtype=torch.int64, device=dev)
    if not hit:
        g_batches = []
        g_keys = None
    if (not hit) and rows_g.numel():
        # table size per row: a row has at most min(ub, n_colsB) distinct
        # columns; clamp, then split into batches whose total workspace
        # stays bounded (power-law matrices would otherwise demand
        # sum-of-flops-sized tables — the R-MAT OOM)
        p2n = 1
        while p2n < int(n_colsB):
            p2n *= 2
        need = torch.clamp(2 * ub[rows_g], max=p2n).double()
        sizes_all = torch.pow(2.0, torch.ceil(torch.log2(need))).to(
            torch.int64)
        # rows whose table spans all columns use IDENTITY hashing
        # (slot = col): no probe walks, sequential-ish access, sorted
        # compaction for free (skips the batched post-sort).  The
        # threshold trades per-row table traffic (O(p2n) init+sweep)
        # against probe walks + post-sort: LS_SPGEMM_IDENT_DIV=k makes
        # rows with table >= p2n/k identity (1 = exact-span only).
        _idiv = int(_os.environ.get("LS_SPGEMM_IDENT_DIV", "4"))
        # extra conversions (beyond exact-span) only while the identity
        # table stays small in ABSOLUTE terms: measured +15% at
        # scale-18 (p2n = 1 MB tables) but -20% at scale-20 (4 MB
        # tables dominate) — profiles/spgemm_r02.md sweep
        if _idiv > 1 and p2n * 4 <= (1 << 21):
            ident_all = sizes_all * _idiv >= p2n
            sizes_all = torch.where(ident_all,
                                    torch.full_like(sizes_all, p2n),
                                    sizes_all)
        else:
            ident_all = sizes_all >= p2n
        budget = max(int(sizes_all.max().item()), 1 << 27)  # >= 512 MB keys
        CH = int(ext.spgemm_global_chunk)
        a_len_g2 = A_indptr[rows_g + 1] - A_indptr[rows_g]
        a_lo_g = A_indptr[rows_g]
        max_total = 0
        # vectorized batch construction; chunks cover EXPANSION positions
        # (per-thread binary search over the per-row B-length prefix in
        # the kernel), so hub rows with few A-entries still parallelize
        for ident in (False, True):
            sel = torch.nonzero(ident_all == ident).reshape(-1)
            if not sel.numel():
                continue
            sizes_s = sizes_all[sel]
            csum = torch.cumsum(sizes_s, dim=0)
            batch_id = torch.div(csum - sizes_s, budget,
                                 rounding_mode="floor")
            off_global = csum - sizes_s
            rows_s = rows_g[sel]
            a_len_s = a_len_g2[sel]
            ub_s = ub[rows_s]
            # per-row inclusive B-length prefix over this class's entries
            tot_e = int(a_len_s.sum())
            base_ent = torch.cumsum(a_len_s, 0) - a_len_s
            row_of = torch.repeat_interleave(
                torch.arange(sel.numel(), device=dev), a_len_s)
            ent_off = (torch.arange(tot_e, device=dev)
                       - torch.repeat_interleave(base_ent, a_len_s))
            a_pos = a_lo_g[sel][row_of] + ent_off
            k_loc = A_indices[a_pos].long() - b_row_offset
            blen = B_indptr[k_loc + 1] - B_indptr[k_loc]
            g = torch.cumsum(blen, 0)
            rowpre = torch.where(
                base_ent > 0,
                g[torch.clamp(base_ent - 1, min=0)],
                torch.zeros_like(base_ent))
            blen_prefix = (g - torch.repeat_interleave(rowpre, a_len_s)
                           ).contiguous()
            # chunks per row by expansion size
            nch = torch.div(ub_s + (CH - 1), CH,
                            rounding_mode="floor").clamp(min=1)
            ch_start = torch.cumsum(nch, 0) - nch
            tot_ch_all = int(nch.sum())
            ch_rowidx_all = torch.repeat_interleave(
                torch.arange(sel.numel(), device=dev), nch)
            ch_ord_all = (torch.arange(tot_ch_all, device=dev)
                          - torch.repeat_interleave(ch_start, nch))
            n_b = int(batch_id[-1]) + 1
            bt = torch.arange(n_b, device=dev)
            row_lo = torch.searchsorted(batch_id, bt, right=False)
            row_hi = torch.searchsorted(batch_id, bt, right=True)
            ch_lo = ch_start[row_lo]
            ch_hi = torch.where(
                row_hi < sel.numel(), ch_start.take(
                    torch.clamp(row_hi, max=sel.numel() - 1)),
                torch.full_like(row_hi, tot_ch_all))
            ch_hi = torch.where(row_hi < sel.numel(), ch_hi,
                                torch.full_like(row_hi, tot_ch_all))
            base = off_global[row_lo]
            tot = csum[torch.clamp(row_hi - 1, min=0)] - base
            host = torch.stack([row_lo, row_hi, ch_lo, ch_hi, tot]).cpu()
            rl, rh, cl, chh, tt = host.tolist()
            for b in range(n_b):
                r0, r1 = int(rl[b]), int(rh[b])
                c0, c1 = int(cl[b]), int(chh[b])
                rows_b = rows_s[r0:r1]
                sizes_b = sizes_s[r0:r1].contiguous()
                off_b = (off_global[r0:r1] - off_global[r0]).contiguous()
                total_b = int(tt[b]) if r1 > r0 else 0
                max_total = max(max_total, total_b)
                ch_rowidx = (ch_rowidx_all[c0:c1] - r0).contiguous()
                ch_ord = ch_ord_all[c0:c1].contiguous()
                pref_base_b = base_ent[r0:r1].contiguous()
                a_len_b = a_len_s[r0:r1].contiguous()
                g_batches.append((rows_b, off_b, sizes_b, total_b,
                                  ch_rowidx, ch_ord, c1 - c0,
                                  1 if ident else 0, blen_prefix,
                                  pref_base_b, a_len_b))
        g_keys = torch.empty(max_total, dtype=torch.int32, device=dev)
    _tick("binning")

    # hybrid: merge-bin rows skip their symbolic pass — merge numeric
    # runs ONCE into a capacity layout (cap = ub, bounded by the 4096
    # merge cutoff) counting exact nnz, then one gather compacts into C.
    # Saves the whole merge symbolic (measured ~2 ms of 8 ms on Poisson)
    # for ~cap-sized temporary storage.
    n_merge = 0 if hit else sum(r.numel() for r in mbins)
    cap_total = int(ub[torch.cat([r for r in mbins])].sum().item()) \
        if n_merge else 0
    # cache hit: C_indptr is known — run plain exact numeric directly
    # into C (no hybrid capacity layout, no symbolic)
    hybrid = (not fast) and (not hit) and n_merge > 0 \
        and cap_total <= (1 << 29)
    if hybrid:
        cap_off = torch.zeros(n_rows + 1, dtype=torch.int64, device=dev)
        mrows = torch.cat([r for r in mbins])
        ub_m = torch.zeros(n_rows, dtype=torch.int64, device=dev)
        ub_m[mrows] = ub[mrows]
        torch.cumsum(ub_m, dim=0, out=cap_off[1:])
        Ci_cap = torch.empty(cap_total, dtype=A_indices.dtype, device=dev)
        Cv_cap = torch.empty(cap_total, dtype=A_vals.dtype, device=dev)
        for wcfg, rows in enumerate(mbins):
            if rows.numel():
                ext.spgemm_merge_numeric(
                    wcfg, rows.data_ptr(), rows.numel(),
                    A_indptr.data_ptr(), A_indices.data_ptr(),
                    A_vals.data_ptr(), bp_ptr, B_indices.data_ptr(),
                    B_vals.data_ptr(), cap_off.data_ptr(),
                    Ci_cap.data_ptr(), Cv_cap.data_ptr(), code, icode,
                    row_nnz.data_ptr(), st)

    if not fast:
        # ---- exact 2-phase: symbolic then numeric --------------------
        if (not hybrid) and (not hit):
            for wcfg, rows in enumerate(mbins):
                if rows.numel():
                    ext.spgemm_merge_symbolic(
                        wcfg, rows.data_ptr(), rows.numel(),
                        A_indptr.data_ptr(), A_indices.data_ptr(), bp_ptr,
                        B_indices.data_ptr(), row_nnz.data_ptr(), icode,
                        st)
        if not hit:
            for cfg, rows in enumerate(bins):
                if rows.numel():
                    ext.spgemm_symbolic_lds(
                        cfg, rows.data_ptr(), rows.numel(),
                        A_indptr.data_ptr(),
                        A_indices.data_ptr(), bp_ptr,
                        B_indices.data_ptr(), row_nnz.data_ptr(), icode,
                        st)
            for (rows_b, off_b, sizes_b, total_b, ch_ri, ch_ord,
                 tot_ch, ident, bpre, pbase, albat) in g_batches:
                g_keys[:total_b].fill_(-1)
                ext.spgemm_symbolic_global(
                    rows_b.data_ptr(), ch_ri.data_ptr(), ch_ord.data_ptr(),
                    tot_ch, A_indptr.data_ptr(), A_indices.data_ptr(),
                    bp_ptr,
                    B_indices.data_ptr(), g_keys.data_ptr(),
                    off_b.data_ptr(),
                    sizes_b.data_ptr(), row_nnz.data_ptr(), icode, ident,
                    bpre.data_ptr(), pbase.data_ptr(), albat.data_ptr(),
                    st)
            _tick("symbolic")
        if hit:
            # clone: cached structure must not alias the returned matrix
            C_indptr = cache["C_indptr"].clone()
            nnz = cache["nnz"]
        else:
            C_indptr = torch.zeros(n_rows + 1, dtype=torch.int64,
                                   device=dev)
            torch.cumsum(row_nnz, dim=0, out=C_indptr[1:])
            nnz = int(C_indptr[-1].item())
        C_indices = torch.empty(nnz, dtype=A_indices.dtype, device=dev)
        C_vals = torch.empty(nnz, dtype=A_vals.dtype, device=dev)
        out_indptr = C_indptr
        nnz_ptr = 0
        _tick("alloc")
    else:
        # ---- fast: allocate by upper bound, numeric counts -----------
        # (clamped: a row has at most n_colsB distinct columns)
        out_indptr = torch.zeros(n_rows + 1, dtype=torch.int64, device=dev)
        torch.cumsum(torch.clamp(ub, max=int(n_colsB)), dim=0,
                     out=out_indptr[1:])
        cap = int(out_indptr[-1].item())
        C_indices = torch.empty(cap, dtype=A_indices.dtype, device=dev)
        C_vals = torch.empty(cap, dtype=A_vals.dtype, device=dev)
        nnz_ptr = row_nnz.data_ptr()

    if hybrid:
        # compact merged rows from the capacity layout into C (kernel:
        # the torch index-assembly version of this copy cost ~16 ms)
        ext.spgemm_compact_rows(
            mrows.data_ptr(), mrows.numel(), cap_off.data_ptr(),
            C_indptr.data_ptr(), Ci_cap.data_ptr(), Cv_cap.data_ptr(),
            C_indices.data_ptr(), C_vals.data_ptr(), code, icode, st)
        del Ci_cap, Cv_cap
    else:
        for wcfg, rows in enumerate(mbins):
            if rows.numel():
                ext.spgemm_merge_numeric(
                    wcfg, rows.data_ptr(), rows.numel(),
                    A_indptr.data_ptr(), A_indices.data_ptr(),
                    A_vals.data_ptr(), bp_ptr, B_indices.data_ptr(),
                    B_vals.data_ptr(), out_indptr.data_ptr(),
                    C_indices.data_ptr(), C_vals.data_ptr(), code, icode,
                    nnz_ptr, st)
    for cfg, rows in enumerate(bins):
        if rows.numel():
            ext.spgemm_numeric_lds(
                cfg, rows.data_ptr(), rows.numel(), A_indptr.data_ptr(),
                A_indices.data_ptr(), A_vals.data_ptr(),
                bp_ptr, B_indices.data_ptr(),
                B_vals.data_ptr(), out_indptr.data_ptr(),
                C_indices.data_ptr(), C_vals.data_ptr(), code, icode,
                nnz_ptr, pack, st)
    rows_unsorted = []
    if g_batches:
        g_vals = torch.empty(g_keys.numel(), dtype=A_vals.dtype, device=dev)
        for (rows_b, off_b, sizes_b, total_b, ch_ri, ch_ord,
             tot_ch, ident, bpre, pbase, albat) in g_batches:
            g_keys[:total_b].fill_(-1)
            g_vals[:total_b].zero_()
            ext.spgemm_numeric_global_fill(
                rows_b.data_ptr(), ch_ri.data_ptr(), ch_ord.data_ptr(),
                tot_ch, A_indptr.data_ptr(), A_indices.data_ptr(),
                A_vals.data_ptr(), bp_ptr, B_indices.data_ptr(),
                B_vals.data_ptr(), g_keys.data_ptr(), g_vals.data_ptr(),
                off_b.data_ptr(), sizes_b.data_ptr(), code, icode, ident,
                bpre.data_ptr(), pbase.data_ptr(), albat.data_ptr(), st)
            if ident:
                # identity tables (slot == col): ordered compaction emits
                # sorted rows directly
                ext.spgemm_global_compact_sorted(
                    rows_b.data_ptr(), rows_b.numel(), g_keys.data_ptr(),
                    g_vals.data_ptr(), off_b.data_ptr(),
                    sizes_b.data_ptr(), out_indptr.data_ptr(),
                    C_indices.data_ptr(), C_vals.data_ptr(), nnz_ptr,
                    code, icode, st)
            else:
                ext.spgemm_global_compact(
                    rows_b.data_ptr(), rows_b.numel(), g_keys.data_ptr(),
                    g_vals.data_ptr(), off_b.data_ptr(),
                    sizes_b.data_ptr(), out_indptr.data_ptr(),
                    C_indices.data_ptr(), C_vals.data_ptr(), nnz_ptr,
                    code, icode, st)
                rows_unsorted.append(rows_b)

    _tick("numeric")
    if fast:
        # compact the capacity layout to exact CSR
        C_indptr = torch.zeros(n_rows + 1, dtype=torch.int64, device=dev)
        torch.cumsum(row_nnz, dim=0, out=C_indptr[1:])
        total_nnz = int(C_indptr[-1].item())
        src = (torch.repeat_interleave(out_indptr[:-1], row_nnz)
               + torch.arange(total_nnz, device=dev)
               - torch.repeat_interleave(C_indptr[:-1], row_nnz))
        C_indices = C_indices[src]
        C_vals = C_vals[src]

    if rows_unsorted:
        # canonical per-row sort for NON-identity global-bin rows, in
        # entry-bounded batches (an unbatched sort materialized ~3x
        # total-entries int64 tensors — OOM at R-MAT scale 20)
        rows_u = torch.cat(rows_unsorted)
        cnts_all = (C_indptr[rows_u + 1] - C_indptr[rows_u])
        csum_u = torch.cumsum(cnts_all, 0)
        budget_e = 1 << 28
        n_u = rows_u.numel()
        start_row = 0
        while start_row < n_u:
            base_e = int(csum_u[start_row - 1]) if start_row else 0
            end_row = int(torch.searchsorted(
                csum_u, torch.tensor(base_e + budget_e, device=dev),
                right=True))
            end_row = max(end_row, start_row + 1)
            end_row = min(end_row, n_u)
            rg = rows_u[start_row:end_row]
            cnts = cnts_all[start_row:end_row]
            total_e = int(cnts.sum())
            if total_e:
                starts = C_indptr[rg]
                seg_start = torch.cumsum(cnts, 0) - cnts
                pos = (torch.arange(total_e, device=dev)
                       - torch.repeat_interleave(seg_start, cnts))
                ent = torch.repeat_interleave(starts, cnts) + pos
                if _os.environ.get("LS_SPGEMM_SEGSORT", "1") == "1":
                    # rocPRIM segmented radix sort over the packed
                    # segments, only the column bits (torch composite
                    # measured 1.02 s of R-MAT scale-20's 3.44 s)
                    keys_in = C_indices[ent].contiguous()
                    vals_in = C_vals[ent].contiguous()
                    keys_out = torch.empty_like(keys_in)
                    vals_out = torch.empty_like(vals_in)
                    seg_b = seg_start.contiguous()
                    seg_e = (seg_start + cnts).contiguous()
                    end_bit = max(1, int(n_colsB - 1).bit_length())
                    tb = ext.segsort_temp_bytes(
                        total_e, rg.numel(), seg_b.data_ptr(),
                        seg_e.data_ptr(), end_bit, code,
                        _icode(keys_in), st)
                    temp = torch.empty(max(int(tb), 16),
                                       dtype=torch.uint8, device=dev)
                    ext.segsort_pairs(
                        temp.data_ptr(), int(tb), keys_in.data_ptr(),
                        keys_out.data_ptr(), vals_in.data_ptr(),
                        vals_out.data_ptr(), total_e, rg.numel(),
                        seg_b.data_ptr(), seg_e.data_ptr(), end_bit,
                        code, _icode(keys_in), st)
                    C_indices[ent] = keys_out
                    C_vals[ent] = vals_out
                    del keys_in, vals_in, keys_out, vals_out, temp
                else:
                    seg = torch.repeat_interleave(
                        torch.arange(rg.numel(), device=dev), cnts)
                    keys = seg * int(n_colsB) + C_indices[ent].long()
                    order = torch.argsort(keys)
                    C_indices[ent] = C_indices[ent][order]
                    C_vals[ent] = C_vals[ent][order]
                    del seg, keys, order
                del seg_start, pos, ent
            start_row = end_row
    _tick("postsort")
    if cache is not None and not fast and not hit:
        cache.update({"ub": ub, "groups": groups, "g_batches": g_batches,
                      "g_keys": g_keys, "C_indptr": C_indptr, "nnz": nnz})
    return C_indptr, C_indices, C_vals


def _spgemm_esc(A_indptr, A_indices, A_vals, B_indptr, B_indices, B_vals,
                n_colsB, b_row_offset: int = 0):
    dev = A_vals.device
    n_rows = A_indptr.numel() - 1
    a_rows = torch.repeat_interleave(
        torch.arange(n_rows, device=dev), A_indptr[1:] - A_indptr[:-1])
    k = A_indices.long() - b_row_offset
    blen = (B_indptr[1:] - B_indptr[:-1])[k.long()]
    e_rows = torch.repeat_interleave(a_rows, blen)
    e_avals = torch.repeat_interleave(A_vals, blen)
    total = int(blen.sum())
    # position within each expanded B-row segment
    seg_starts = torch.cumsum(blen, 0) - blen
    pos = torch.arange(total, device=dev) - torch.repeat_interleave(
        seg_starts, blen)
    b_off = torch.repeat_interleave(B_indptr[k.long()], blen) + pos
    e_cols = B_indices[b_off]
    e_vals = e_avals * B_vals[b_off]
    key = e_rows * int(n_colsB) + e_cols.long()
    key_sorted, order = torch.sort(key, stable=True)
    vals_sorted = e_vals[order]
    uniq, inverse = torch.unique_consecutive(key_sorted, return_inverse=True)
    C_vals = torch.zeros(uniq.numel(), dtype=A_vals.dtype, device=dev)
    C_vals.index_add_(0, inverse, vals_sorted)
    C_rows = torch.div(uniq, n_colsB, rounding_mode="floor")
    C_indices = uniq - C_rows * n_colsB
    row_nnz = torch.bincount(C_rows, minlength=n_rows)
    C_indptr = torch.zeros(n_rows + 1, dtype=torch.int64, device=dev)
    torch.cumsum(row_nnz, dim=0, out=C_indptr[1:])
    return C_indptr, C_indices, C_vals


# ---------------------------------------------------------------------------
# Conversions
# ---------------------------------------------------------------------------
def csr_to_dense(indptr, indices, vals, n_rows, n_cols) -> torch.Tensor:
    out = torch.zeros(n_rows, n_cols, dtype=vals.dtype, device=vals.device)
    if _use_hip(vals):
        ext = _cext.require_hip()
        ext.csr_to_dense(indptr.data_ptr(), indices.data_ptr(),
                         vals.data_ptr(), out.data_ptr(), n_rows, n_cols,
                         _code(vals), _icode(indices), _stream())
        return out
    row_ids = torch.repeat_interleave(
        torch.arange(n_rows, device=vals.device), indptr[1:] - indptr[:-1])
    out[row_ids, indices.long()] = vals
    return out


def dense_to_csr(dense: torch.Tensor, idx_dtype=torch.int64):
    n_rows, n_cols = dense.shape
    dense = dense.contiguous()
    if _use_hip(dense):
        ext = _cext.require_hip()
        row_nnz = torch.empty(n_rows, dtype=torch.int64, device=dense.device)
        ext.dense_to_csr_nnz(dense.data_ptr(), row_nnz.data_ptr(), n_rows,
                             n_cols, _code(dense), _stream())
        indptr = torch.zeros(n_rows + 1, dtype=torch.int64,
                             device=dense.device)
        torch.cumsum(row_nnz, dim=0, out=indptr[1:])
        nnz = int(indptr[-1].item())
        indices = torch.empty(nnz, dtype=idx_dtype, device=dense.device)
        vals = torch.empty(nnz, dtype=dense.dtype, device=dense.device)
        ext.dense_to_csr_fill(dense.data_ptr(), indptr.data_ptr(),
                              indices.data_ptr(), vals.data_ptr(), n_rows,
                              n_cols, _code(dense), _IDX_CODE[idx_dtype],
                              _stream())
        return indptr, indices, vals
    mask = dense != 0
    row_nnz = mask.sum(dim=1)
    indptr = torch.zeros(n_rows + 1, dtype=torch.int64, device=dense.device)
    torch.cumsum(row_nnz, dim=0, out=indptr[1:])
    nz = mask.nonzero(as_tuple=True)
    return indptr, nz[1].to(idx_dtype), dense[nz]


def diagonal(indptr, indices, vals, n_rows, row_offset: int) -> torch.Tensor:
    """diag[i] = vals[jp] where indices[jp] == row_offset + i, else 0
    (reference get_diagonal.cu:26-44; row_offset makes it partition-aware)."""
    out = torch.zeros(n_rows, dtype=vals.dtype, device=vals.device)
    if _use_hip(vals):
        ext = _cext.require_hip()
        ext.diagonal(indptr.data_ptr(), indices.data_ptr(), vals.data_ptr(),
                     out.data_ptr(), n_rows, int(row_offset), _code(vals),
                     _icode(indices), _stream())
        return out
    row_ids = torch.repeat_interleave(
        torch.arange(n_rows, device=vals.device), indptr[1:] - indptr[:-1])
    hit = indices.long() == (row_ids + row_offset)
    out[row_ids[hit]] = vals[hit]
    return out


# ---------------------------------------------------------------------------
# Solver primitives
# ---------------------------------------------------------------------------
def axpby(y: torch.Tensor, x: torch.Tensor, a: torch.Tensor,
          b: torch.Tensor, isalpha: bool, negate: bool) -> torch.Tensor:
    """Fused CG update with DEVICE-scalar a, b (1-element tensors):
        val = (negate ? -1 : 1) * a/b
        isalpha: y = val*x + y      else: y = x + val*y
    The division happens inside the kernel — no host sync (reference
    axpby.cu:25-47, launched from linalg.py:433-451)."""
    if _use_hip(y):
        ext = _cext.require_hip()
        ext.axpby(y.data_ptr(), x.data_ptr(), a.data_ptr(), b.data_ptr(),
                  y.numel(), bool(isalpha), bool(negate), _code(y), _stream())
        return y
    val = a / b
    if negate:
        val = -val
    if isalpha:
        y.add_(x * val)
    else:
        y.mul_(val).add_(x)
    return y


def jacobi_update(x: torch.Tensor, b: torch.Tensor, y: torch.Tensor,
                  dinv: torch.Tensor, omega: float) -> torch.Tensor:
    """Fused weighted-Jacobi update  x += omega * dinv * (b - y)
    (one pass instead of three; the GMG smoother hot op)."""
    if _use_hip(x):
        ext = _cext.require_hip()
        ext.jacobi(x.data_ptr(), b.data_ptr(), y.data_ptr(),
                   dinv.data_ptr(), float(omega), x.numel(), _code(x),
                   _stream())
        return x
    x.add_(omega * dinv * (b - y))
    return x


def cg_fused(x: torch.Tensor, r: torch.Tensor, p: torch.Tensor,
             q: torch.Tensor, rho: torch.Tensor, pq: torch.Tensor,
             rho_out: torch.Tensor) -> torch.Tensor:
    """Fused unpreconditioned-CG update (real dtypes): alpha = rho/pq
    computed in-kernel from device scalars; x += alpha*p; r -= alpha*q;
    rho_out = local ||r||^2 — one pass over p,q,x,r replacing two axpby
    launches plus the separate r-dot (z = r in unpreconditioned CG).
    Caller all-reduces rho_out across ranks."""
    if _use_hip(x) and not x.is_complex():
        rho_out.zero_()
        _cext.require_hip().cg_fused(
            x.data_ptr(), r.data_ptr(), p.data_ptr(), q.data_ptr(),
            rho.data_ptr(), pq.data_ptr(), rho_out.data_ptr(),
            x.numel(), _code(x), _stream())
        return rho_out
    alpha = (rho / pq).reshape(())
    x += alpha * p
    r -= alpha * q
    rho_out.copy_((r * r).sum().reshape(rho_out.shape))
    return rho_out


def gs_dots(V: torch.Tensor, K: int, w: torch.Tensor,
            out: torch.Tensor = None, conj: bool = True) -> torch.Tensor:
    """out[k] = <V[k, :], w> for k < K — the batched Gram-Schmidt dots
    in one pass over the basis block (LDS-staged w).  V must be a
    contiguous (>=K, n) matrix.  Falls back to a fused torch path off
    GPU."""
    n = w.numel()
    if out is None:
        out = torch.zeros(K, dtype=w.dtype, device=w.device)
    else:
        out.zero_()
    if _use_hip(w) and V.stride(1) == 1:
        _cext.require_hip().gs_dots(V.data_ptr(),
                                    V.stride(0), int(K), w.data_ptr(),
                                    out.data_ptr(), n, bool(conj),
                                    _code(w), _stream())
        return out
    basis = V[:K].conj() if (conj and w.is_complex()) else V[:K]
    out.copy_(basis @ w.reshape(-1))
    return out


def vdot(x: torch.Tensor, y: torch.Tensor, conj: bool = True,
         out: torch.Tensor = None) -> torch.Tensor:
    """Local <x, y> as a 1-element device tensor (block-reduce kernel on
    GPU).  Caller all-reduces across ranks; never .item() in solver
    loops.  ``out`` (zeroed here) enables stable buffers for hipGraph
    capture."""
    if _use_hip(x):
        ext = _cext.require_hip()
        if out is None:
            out = torch.zeros(1, dtype=x.dtype, device=x.device)
        else:
            out.zero_()
        ext.vdot(x.data_ptr(), y.data_ptr(), out.data_ptr(), x.numel(),
                 bool(conj), _code(x), _stream())
        return out
    if conj and x.is_complex():
        res = (x.conj() * y).sum().reshape(1)
    else:
        res = (x * y).sum().reshape(1)
    if out is not None:
        out.copy_(res)
        return out
    return res


# ---------------------------------------------------------------------------
# BiCGSTAB primitives (docs/DESIGN.md §15).  Every scalar is a 1-element
# device tensor; quotients use the GUARDED division  a (/) b  = a / b, but
# exactly 0 when b is exactly 0 — formed in-kernel, never on the host.
# ---------------------------------------------------------------------------
def _gdiv(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """Guarded a/b of 1-element tensors (torch path; no host sync)."""
    zero = b == 0
    q = a / torch.where(zero, torch.ones_like(b), b)
    return torch.where(zero, torch.zeros_like(q), q)


def _bicg_check(vecs, scalars=(), out2=None) -> None:
    """The kernels take raw pointers: a wrong dtype, device or length would
    be reinterpreted silently, so it is refused here."""
    ref = vecs[0]
    for t in vecs:
        if (t.numel() != ref.numel() or not t.is_contiguous()
                or t.dtype != ref.dtype or t.device != ref.device):
            raise ValueError("BiCGSTAB ops need contiguous vectors of one "
                             "length, dtype and device")
    for t, want in [(a, 1) for a in scalars] + (
            [(out2, 2)] if out2 is not None else []):
        if (t.numel() != want or not t.is_contiguous()
                or t.dtype != ref.dtype or t.device != ref.device):
            raise ValueError(f"BiCGSTAB scalar buffers need {want} "
                             "element(s) of the vectors' dtype and device")


def bicgstab_p(p: torch.Tensor, r: torch.Tensor, v: torch.Tensor,
               rho: torch.Tensor, rhv: torch.Tensor, ts: torch.Tensor,
               tt: torch.Tensor) -> torch.Tensor:
    """p <- r + beta (p - omega v) with omega = ts (/) tt and
    beta = (rho (/) rhv) * (tt (/) ts), in place."""
    _bicg_check((p, r, v), (rho, rhv, ts, tt))
    if _use_hip(p):
        _cext.require_hip().bicgstab_p(
            p.data_ptr(), r.data_ptr(), v.data_ptr(), rho.data_ptr(),
            rhv.data_ptr(), ts.data_ptr(), tt.data_ptr(), p.numel(),
            _code(p), _stream())
        return p
    omega = _gdiv(ts, tt).reshape(())
    beta = (_gdiv(rho, rhv) * _gdiv(tt, ts)).reshape(())
    p.sub_(omega * v).mul_(beta).add_(r)
    return p


def bicgstab_s(s: torch.Tensor, r: torch.Tensor, v: torch.Tensor,
               rho: torch.Tensor, rhv: torch.Tensor) -> torch.Tensor:
    """s <- r - (rho (/) rhv) v."""
    _bicg_check((s, r, v), (rho, rhv))
    if _use_hip(s):
        _cext.require_hip().bicgstab_s(
            s.data_ptr(), r.data_ptr(), v.data_ptr(), rho.data_ptr(),
            rhv.data_ptr(), s.numel(), _code(s), _stream())
        return s
    alpha = _gdiv(rho, rhv).reshape(())
    torch.sub(r, alpha * v, out=s)
    return s


def vdot2(t: torch.Tensor, s: torch.Tensor,
          out2: torch.Tensor) -> torch.Tensor:
    """out2 <- [<t, s>, <t, t>] (conjugating t) in one pass over t and s.
    ``out2`` is a 2-element tensor, zeroed here; caller all-reduces it."""
    _bicg_check((t, s), out2=out2)
    if _use_hip(t):
        out2.zero_()
        _cext.require_hip().vdot2(t.data_ptr(), s.data_ptr(),
                                  out2.data_ptr(), t.numel(), _code(t),
                                  _stream())
        return out2
    tc = t.conj() if t.is_complex() else t
    out2[0] = (tc * s).sum()
    out2[1] = (tc * t).sum()
    return out2


def bicgstab_xr(x: torch.Tensor, r: torch.Tensor, phat: torch.Tensor,
                shat: torch.Tensor, s: torch.Tensor, t: torch.Tensor,
                rhat: torch.Tensor, rho: torch.Tensor, rhv: torch.Tensor,
                ts: torch.Tensor, tt: torch.Tensor,
                out2: torch.Tensor) -> torch.Tensor:
    """With alpha = rho (/) rhv and omega = ts (/) tt:
    x <- x + alpha phat + omega shat;  r <- s - omega t;
    out2 <- [<rhat, r_new>, <r_new, r_new>] in the same pass.
    ``phat`` may alias p and ``shat`` may alias ``s``; x, r and out2 alias
    nothing, and out2 must not alias an input scalar."""
    _bicg_check((x, r, phat, shat, s, t, rhat), (rho, rhv, ts, tt), out2)
    if _use_hip(x):
        out2.zero_()
        _cext.require_hip().bicgstab_xr(
            x.data_ptr(), r.data_ptr(), phat.data_ptr(), shat.data_ptr(),
            s.data_ptr(), t.data_ptr(), rhat.data_ptr(), rho.data_ptr(),
            rhv.data_ptr(), ts.data_ptr(), tt.data_ptr(), out2.data_ptr(),
            x.numel(), _code(x), _stream())
        return out2
    alpha = _gdiv(rho, rhv).reshape(())
    omega = _gdiv(ts, tt).reshape(())
    x.add_(alpha * phat).add_(omega * shat)
    torch.sub(s, omega * t, out=r)
    rc = r.conj() if r.is_complex() else r
    hc = rhat.conj() if rhat.is_complex() else rhat
    out2[0] = (hc * r).sum()
    out2[1] = (rc * r).sum()
    return out2


# ---------------------------------------------------------------------------
# Tall-skinny block algebra for LOBPCG (docs/DESIGN.md §16).  Operands are
# row-major (n, cols) blocks with unit column stride and any row stride
# >= cols (a column panel of a wider buffer is fine), 1 <= cols <=
# BLOCK_KMAX.  Reductions are bit-reproducible: partial slab + fixed-order
# reduce, no float atomics.
# ---------------------------------------------------------------------------
BLOCK_KMAX = 32

def _real_dtype(dt: torch.dtype) -> torch.dtype:
    return {torch.complex64: torch.float32,
            torch.complex128: torch.float64}.get(dt, dt)


def _block_check(blocks, smalls=()) -> None:
    """The kernels take raw pointers: dtype, device, shape and strides are
    checked here.  ``smalls`` are (tensor, shape, dtype) device matrices or
    vectors that must be contiguous."""
    ref = blocks[0]
    if ref.dtype not in _DTYPE_CODE:
        raise ValueError(f"block ops: unsupported dtype {ref.dtype}")
    for t in blocks:
        if t.ndim != 2:
            raise ValueError("block ops need 2-D blocks")
        cols = int(t.shape[1])
        if not 1 <= cols <= BLOCK_KMAX:
            raise ValueError(
                f"block ops take 1 to {BLOCK_KMAX} columns, got {cols}")
        if (t.shape[0] != ref.shape[0] or t.dtype != ref.dtype
                or t.device != ref.device):
            raise ValueError("block ops need blocks of one row count, "
                             "dtype and device")
        if t.shape[0] > 0 and (t.stride(1) != 1 or t.stride(0) < cols):
            raise ValueError("block ops need row-major blocks: unit column "
                             "stride and a row stride >= the column count")
    for t, shape, dt in smalls:
        if (tuple(t.shape) != tuple(shape) or t.dtype != dt
                or t.device != ref.device or not t.is_contiguous()):
            raise ValueError(
                f"block ops: need a contiguous {tuple(shape)} {dt} tensor "
                f"on {ref.device}, got {tuple(t.shape)} {t.dtype} on "
                f"{t.device}")


def _ld(t: torch.Tensor) -> int:
    # a 0- or 1-row view may report any stride; the kernel never uses it
    return max(int(t.stride(0)), int(t.shape[1])) if t.shape[0] > 1 \
        else int(t.shape[1])


def _block_grid(ext, kind: str, n: int) -> int:
    """Workgroups the kernel launches for n rows (sizes its slab)."""
    per = getattr(ext, f"BLOCK_{kind}_PER_BLOCK")
    cap = getattr(ext, f"BLOCK_{kind}_GRID_CAP")
    return min(cap, max(1, -(-n // per)))


def _overlap(a: torch.Tensor, b: torch.Tensor) -> str:
    """'none', 'same' (identical view) or 'partial' for two blocks."""
    if a.numel() == 0 or b.numel() == 0 or \
            a.untyped_storage().data_ptr() != b.untyped_storage().data_ptr():
        return "none"
    if (a.data_ptr() == b.data_ptr() and a.shape == b.shape
            and a.stride() == b.stride()):
        return "same"
    es = a.element_size()

    def span(t):
        lo = t.data_ptr()
        return lo, lo + ((t.shape[0] - 1) * t.stride(0) + t.shape[1]) * es
    (alo, ahi), (blo, bhi) = span(a), span(b)
    if ahi <= blo or bhi <= alo:
        return "none"
    ld = a.stride(0)
    if a.shape[0] > 1 and b.shape[0] > 1 and b.stride(0) == ld:
        # column panels of one wider buffer: disjoint column ranges
        base = min(alo, blo)
        ca, cb = (alo - base) // es, (blo - base) // es
        if max(ca + a.shape[1], cb + b.shape[1]) <= ld and (
                ca + a.shape[1] <= cb or cb + b.shape[1] <= ca):
            return "none"
    return "partial"


def block_gram(X: torch.Tensor, Y: torch.Tensor, conj: bool = True,
               out: torch.Tensor = None) -> torch.Tensor:
    """``G = X^H Y`` (``X^T Y`` with ``conj=False``): X is (n, p), Y is
    (n, q), the result a (p, q) device tensor holding this rank's partial
    sum (the caller all-reduces).  X and Y may alias.  Bit-identical from
    run to run for the same input."""
    p, q = int(X.shape[1]), int(Y.shape[1])
    if out is None:
        out = torch.empty((p, q), dtype=X.dtype, device=X.device)
    _block_check((X, Y), [(out, (p, q), X.dtype)])
    n = int(X.shape[0])
    if _use_hip(X):
        ext = _cext.require_hip()
        slab = torch.empty(_block_grid(ext, "GRAM", n) * p * q, dtype=X.dtype,
                           device=X.device)
        ext.block_gram(X.data_ptr(), _ld(X), p, Y.data_ptr(), _ld(Y), q,
                       out.data_ptr(), slab.data_ptr(), slab.numel(), n,
                       bool(conj), _code(X), _stream())
        return out
    return _block_gram_torch(X, Y, conj, out)


_GRAM_TORCH_CHUNK = 1024


def _block_gram_torch(X, Y, conj, out):
    """torch formulation.  A tall block goes through a split-K batched
    product (chunks of 1024 rows, partial Grams summed): the plain
    ``X^H @ Y`` puts the whole n-long contraction on one tile — measured
    450 ms against 0.12 ms for the kernel at n = 4.2M, k = 8, fp64
    (profiles/lobpcg_r05.md)."""
    Xt = X.conj() if (conj and X.is_complex()) else X
    n, c = int(X.shape[0]), _GRAM_TORCH_CHUNK
    nb = n // c
    if nb < 64:
        out.copy_(Xt.transpose(0, 1) @ Y)
        return out
    p, q = int(X.shape[1]), int(Y.shape[1])
    head = torch.bmm(Xt[:nb * c].reshape(nb, c, p).transpose(1, 2),
                     Y[:nb * c].reshape(nb, c, q)).sum(dim=0)
    if nb * c < n:
        head = head + Xt[nb * c:].transpose(0, 1) @ Y[nb * c:]
    out.copy_(head)
    return out


def block_update(Z: torch.Tensor, terms, accumulate: bool = False
                 ) -> torch.Tensor:
    """``Z = sum_i X_i @ C_i (+ Z)`` in one pass.  ``terms`` is a sequence
    of one to three ``(X_i, C_i)`` pairs: X_i an (n, p_i) block, C_i a
    contiguous (p_i, q) device matrix, Z an (n, q) block.

    Aliasing: Z may BE one of the X_i (the identical view: same pointer,
    shape and strides) and may be a column panel of the same wider buffer
    as an X_i when their column ranges are disjoint.  Any other overlap of
    Z with an X_i, and any overlap of Z with a C_i, is refused.  The X_i
    may alias each other freely."""
    terms = list(terms)
    if not 1 <= len(terms) <= 3:
        raise ValueError("block_update takes one to three (X, C) terms")
    q = int(Z.shape[1])
    _block_check([Z] + [x for x, _ in terms],
                 [(c, (int(x.shape[1]), q), Z.dtype) for x, c in terms])
    for x, c in terms:
        if _overlap(Z, x) == "partial":
            raise ValueError("block_update: Z overlaps an input block "
                             "without being that block")
        if Z.numel() and c.numel() and Z.untyped_storage().data_ptr() == \
                c.untyped_storage().data_ptr():
            raise ValueError("block_update: Z shares storage with a "
                             "coefficient matrix")
    n = int(Z.shape[0])
    if _use_hip(Z):
        ext = _cext.require_hip()
        flat = []
        for i in range(3):
            x, c = terms[i] if i < len(terms) else terms[0]
            flat += [x.data_ptr(), _ld(x), int(x.shape[1]), c.data_ptr()]
        ext.block_update(Z.data_ptr(), _ld(Z), q, len(terms), *flat,
                         bool(accumulate), n, _code(Z), _stream())
        return Z
    return _block_update_torch(Z, terms, accumulate)


def _block_update_torch(Z, terms, accumulate):
    acc = terms[0][0] @ terms[0][1]
    for x, c in terms[1:]:
        acc = acc + x @ c
    if accumulate:
        acc = acc + Z
    Z.copy_(acc)
    return Z


def block_residual(R: torch.Tensor, AX: torch.Tensor, X: torch.Tensor,
                   theta: torch.Tensor, norms: torch.Tensor = None
                   ) -> torch.Tensor:
    """``R = AX - X diag(theta)`` and, from the same pass, the k squared
    column 2-norms of R (this rank's partial sums; the caller all-reduces).
    ``theta`` and ``norms`` are k-element device vectors of the REAL dtype
    of the blocks.  R may be AX or X itself; any other overlap is refused.
    The norms are bit-identical from run to run.  Returns ``norms``."""
    k = int(X.shape[1])
    rdt = _real_dtype(X.dtype)
    if norms is None:
        norms = torch.empty(k, dtype=rdt, device=X.device)
    _block_check((R, AX, X), [(theta, (k,), rdt), (norms, (k,), rdt)])
    if _overlap(R, AX) == "partial" or _overlap(R, X) == "partial":
        raise ValueError("block_residual: R overlaps an input block "
                         "without being that block")
    n = int(X.shape[0])
    if _use_hip(X):
        ext = _cext.require_hip()
        slab = torch.empty(_block_grid(ext, "RESIDUAL", n) * k, dtype=rdt,
                           device=X.device)
        ext.block_residual(R.data_ptr(), _ld(R), AX.data_ptr(), _ld(AX),
                           X.data_ptr(), _ld(X), theta.data_ptr(),
                           norms.data_ptr(), slab.data_ptr(), slab.numel(),
                           k, n, _code(X), _stream())
        return norms
    return _block_residual_torch(R, AX, X, theta, norms)


def _block_residual_torch(R, AX, X, theta, norms):
    res = AX - X * theta.to(X.dtype).reshape(1, -1)
    R.copy_(res)
    norms.copy_((R.real ** 2 + R.imag ** 2).sum(dim=0) if R.is_complex()
                else (R * R).sum(dim=0))
    return norms


# ---------------------------------------------------------------------------
# Level-scheduled sparse triangular solve and ILU(0) (docs/DESIGN.md §17).
# The matrix is a LOCAL square CSR (columns are local row numbers, sorted
# within a row).  Rows are grouped into dependency levels on the host once
# per structure; the levels become a launch plan of "wide" launches (one
# level, many workgroups) and "chain" launches (a run of narrow levels, one
# workgroup, a barrier between levels).  No kernel waits on another
# workgroup.
# ---------------------------------------------------------------------------
SPTRSV_KMAX = 32
# a level with at most this many rows joins a chain (the extension exports
# the same numbers; tests compare them)
SPTRSV_CHAIN_ROWS = 256
SPTRSV_GRID_CAP = 4096
_I32_MAX = 2 ** 31 - 1
_SPTRSV_IMPLS = ("native", "torch")


def diag_positions(indptr: torch.Tensor, indices: torch.Tensor, n: int,
                   row_offset: int = 0):
    """``(diag_pos, has_diag)``: the position of the diagonal in every row
    of a CSR with sorted rows, or the insertion point where it is not
    stored, and a mask of the rows that store it.  Index arithmetic on the
    matrix's device."""
    dev = indptr.device
    rows = torch.arange(n, device=dev)
    row_of = torch.repeat_interleave(rows, indptr[1:] - indptr[:-1])
    col = indices.long() - int(row_offset)
    cnt = torch.bincount(row_of[col < row_of], minlength=n)
    dpos = (indptr[:-1] + cnt).contiguous()
    if col.numel():
        at = col[dpos.clamp(max=col.numel() - 1)]
        has = (dpos < indptr[1:]) & (at == rows)
    else:
        has = torch.zeros(n, dtype=torch.bool, device=dev)
    return dpos, has


def sptrsv_plan(level_ptr, chain_rows: int):
    """Launch plan for the levels ``level_ptr`` describes: an (m, 3) int64
    numpy array of ``(kind, lv_lo, lv_hi)``, kind 0 = wide (one level with
    more than ``chain_rows`` rows), 1 = chain (a maximal run of levels of
    at most ``chain_rows`` rows each)."""
    import numpy as np
    w = np.diff(np.asarray(level_ptr, dtype=np.int64))
    if w.size == 0:
        return np.zeros((0, 3), dtype=np.int64)
    narrow = w <= int(chain_rows)
    prev_narrow = np.concatenate([[False], narrow[:-1]])
    lo = np.flatnonzero(~narrow | ~prev_narrow)
    hi = np.concatenate([lo[1:], [w.size]])
    return np.ascontiguousarray(
        np.stack([narrow[lo].astype(np.int64), lo, hi], axis=1))


class LevelSchedule:
    """Rows sorted by dependency level (``order``, stable within a level)
    and the level boundaries (``level_ptr``), on the host and on the
    matrix's device, with the launch plans built from them."""

    def __init__(self, order: torch.Tensor, level_ptr: torch.Tensor, device,
                 lower: bool):
        self.lower = bool(lower)
        self.order_host = order
        self.level_ptr_host = level_ptr.contiguous()
        self.n_levels = int(level_ptr.numel()) - 1
        self.order = order.to(device)
        self.level_ptr = self.level_ptr_host.to(device)
        self._plans = {}
        self._torch_levels = None

    def plan(self, chain_rows=None) -> torch.Tensor:
        c = SPTRSV_CHAIN_ROWS if chain_rows is None else int(chain_rows)
        if c < 1:
            raise ValueError("_chain_rows must be at least 1")
        if c not in self._plans:
            self._plans[c] = torch.from_numpy(
                sptrsv_plan(self.level_ptr_host.numpy(), c))
        return self._plans[c]

    def n_launches(self, chain_rows=None) -> int:
        return int(self.plan(chain_rows).shape[0])

    def torch_levels(self, indptr, indices, dpos):
        """Per-level index tensors of the ``_impl="torch"`` arm:
        ``(rows, entries, columns, segment ids, diagonal positions)``."""
        if self._torch_levels is not None:
            return self._torch_levels
        dev = indptr.device
        rows = self.order
        n = int(rows.numel())
        if self.lower:
            s, e = indptr[rows], dpos[rows]
        else:
            nnz = int(indices.numel())
            e = indptr[rows + 1]
            d = dpos[rows]
            if nnz:
                has = (d < e) & (indices[d.clamp(max=nnz - 1)].long() == rows)
            else:
                has = torch.zeros(n, dtype=torch.bool, device=dev)
            s = d + has.long()
        cnt = e - s
        off = torch.cumsum(cnt, 0) - cnt
        seg = torch.repeat_interleave(torch.arange(n, device=dev), cnt)
        ent = s[seg] + (torch.arange(seg.numel(), device=dev) - off[seg])
        cols = indices[ent].long()
        ends = torch.cat([off, cnt.sum().reshape(1)])
        lp = self.level_ptr_host.tolist()
        eb = ends[self.level_ptr].cpu().tolist()
        out = []
        for lv in range(self.n_levels):
            a, b = lp[lv], lp[lv + 1]
            out.append((rows[a:b], ent[eb[lv]:eb[lv + 1]],
                        cols[eb[lv]:eb[lv + 1]],
                        seg[eb[lv]:eb[lv + 1]] - a, dpos[rows[a:b]]))
        self._torch_levels = out
        return out


def level_schedule(indptr: torch.Tensor, indices: torch.Tensor, n: int,
                   lower: bool, row_offset: int = 0) -> LevelSchedule:
    """Level analysis of the lower or upper triangle: one sequential
    O(nnz) pass on the host (``indptr`` / ``indices`` of a GPU matrix are
    copied there once).  Entries whose column falls outside
    ``[row_offset, row_offset + n)`` are not dependencies."""
    cpu = _cext.require_cpu()
    ip = indptr.to("cpu", torch.int64).contiguous()
    ix = indices.to("cpu").contiguous()
    order = torch.empty(n, dtype=torch.int64)
    lptr = torch.zeros(n + 1, dtype=torch.int64)
    nl = cpu.level_schedule(ip.data_ptr(), ix.data_ptr(), int(n), bool(lower),
                            int(row_offset), order.data_ptr(),
                            lptr.data_ptr(), _icode(ix)) if n else 0
    return LevelSchedule(order, lptr[:nl + 1].clone(), indptr.device, lower)


def _tri_check(indptr, indices, vals, diag_pos, sched, what):
    n = int(indptr.numel()) - 1
    if vals.dtype not in _DTYPE_CODE or indices.dtype not in _IDX_CODE:
        raise ValueError(f"{what}: unsupported value or index dtype")
    for t, dt, ne in ((indptr, torch.int64, n + 1),
                      (diag_pos, torch.int64, n),
                      (sched.order, torch.int64, n),
                      (indices, indices.dtype, vals.numel()),
                      (vals, vals.dtype, vals.numel())):
        if (t.dtype != dt or t.numel() != ne or t.device != vals.device
                or not t.is_contiguous()):
            raise ValueError(f"{what}: needs contiguous CSR arrays, diag_pos "
                             f"and schedule of one matrix on one device")
    return n


def _cap_arg(grid_cap) -> int:
    if grid_cap is None:
        return 0
    if not 1 <= int(grid_cap) <= SPTRSV_GRID_CAP:
        raise ValueError(f"_grid_cap outside [1, {SPTRSV_GRID_CAP}]")
    return int(grid_cap)


def sptrsv(indptr: torch.Tensor, indices: torch.Tensor, vals: torch.Tensor,
           diag_pos: torch.Tensor, sched: LevelSchedule, X: torch.Tensor,
           lower: bool = True, unit_diagonal: bool = False,
           _impl: str = "native", _grid_cap=None, _chain_rows=None
           ) -> torch.Tensor:
    """Solve ``T X = X`` IN PLACE, T the lower (upper) triangle of the
    square local CSR: row i uses the entries ``[indptr[i], diag_pos[i])``
    (``(diag_pos[i], indptr[i+1])``) and divides by the stored diagonal
    unless ``unit_diagonal``.  X is an (n, k) row-major block, 1 <= k <=
    SPTRSV_KMAX, with unit column stride and any row stride >= k.
    ``sched`` is ``level_schedule(...)`` of the same triangle.  Without
    ``unit_diagonal`` every row must store its diagonal (the caller checks:
    ``diag_positions`` returns the mask).  Bit-identical from run to run.  ``_grid_cap`` / ``_chain_rows`` override the launch
    shape for tests."""
    if _impl not in _SPTRSV_IMPLS:
        raise ValueError(f"_impl must be one of {_SPTRSV_IMPLS}")
    n = _tri_check(indptr, indices, vals, diag_pos, sched, "sptrsv")
    if sched.lower != bool(lower):
        raise ValueError("sptrsv: the schedule is of the other triangle")
    if X.ndim != 2 or int(X.shape[0]) != n:
        raise ValueError(f"sptrsv needs an ({n}, k) block")
    k = int(X.shape[1])
    if not 1 <= k <= SPTRSV_KMAX:
        raise ValueError(f"sptrsv takes 1 to {SPTRSV_KMAX} columns, got {k}")
    if X.dtype != vals.dtype or X.device != vals.device:
        raise ValueError("sptrsv: X must have the matrix's dtype and device")
    if n > 1 and (X.stride(1) != 1 or X.stride(0) < k):
        raise ValueError("sptrsv needs a row-major block: unit column "
                         "stride and a row stride >= the column count")
    if n == 1 and k > 1 and X.stride(1) != 1:
        raise ValueError("sptrsv needs unit column stride")
    cap = _cap_arg(_grid_cap)
    plan = sched.plan(_chain_rows)
    if n == 0:
        return X
    if _impl == "torch" or (X.is_cuda and settings.force_cpu_fallback):
        return _sptrsv_torch(indptr, indices, vals, diag_pos, sched, X,
                             unit_diagonal)
    if X.is_cuda:
        ext = _cext.require_hip()
        ext.sptrsv(indptr.data_ptr(), indices.data_ptr(), vals.data_ptr(),
                   diag_pos.data_ptr(), sched.order.data_ptr(),
                   sched.level_ptr.data_ptr(), X.data_ptr(), _ld(X), k, n,
                   vals.numel(), sched.level_ptr_host.data_ptr(),
                   sched.n_levels, plan.data_ptr(), int(plan.shape[0]),
                   bool(lower), bool(unit_diagonal), cap, _code(vals),
                   _icode(indices), _stream())
        return X
    _cext.require_cpu().sptrsv(
        indptr.data_ptr(), indices.data_ptr(), vals.data_ptr(),
        diag_pos.data_ptr(), X.data_ptr(), _ld(X), k, n, bool(lower),
        bool(unit_diagonal), _code(vals), _icode(indices))
    return X


def _sptrsv_torch(indptr, indices, vals, dpos, sched, X, unit):
    """Per-level index ops in torch (debug arm and the A/B benchmark)."""
    for rows, ent, cols, seg, drows in sched.torch_levels(indptr, indices,
                                                          dpos):
        xi = X[rows]
        if ent.numel():
            xi = xi.index_add(0, seg, vals[ent].unsqueeze(1) * X[cols],
                              alpha=-1)
        if not unit:
            xi = xi / vals[drows].unsqueeze(1)
        X[rows] = xi
    return X


def ilu0_factor(indptr: torch.Tensor, indices: torch.Tensor, F: torch.Tensor,
                diag_pos: torch.Tensor, sched: LevelSchedule,
                flag: torch.Tensor, max_row_nnz: int,
                _impl: str = "native", _grid_cap=None, _chain_rows=None
                ) -> torch.Tensor:
    """IKJ ILU(0) IN PLACE on ``F`` (the values of a square local CSR whose
    every diagonal entry is stored, ``diag_pos`` pointing at them): on
    return the strict lower part holds L (unit diagonal implied) and the
    rest U.  ``sched`` is the LOWER schedule.  ``flag`` (one int32 on the
    matrix's device) receives the smallest row whose pivot is zero or not
    finite, or 2**31 - 1; nothing is read back here.  ``max_row_nnz`` is
    the longest row (picks the sub-wave width)."""
    if _impl not in _SPTRSV_IMPLS:
        raise ValueError(f"_impl must be one of {_SPTRSV_IMPLS}")
    n = _tri_check(indptr, indices, F, diag_pos, sched, "ilu0_factor")
    if not sched.lower:
        raise ValueError("ilu0_factor needs the lower schedule")
    if (flag.dtype != torch.int32 or flag.numel() != 1
            or flag.device != F.device):
        raise ValueError("ilu0_factor: flag is one int32 on the matrix's "
                         "device")
    if n > _I32_MAX:
        raise ValueError("ilu0_factor: too many local rows")
    cap = _cap_arg(_grid_cap)
    plan = sched.plan(_chain_rows)
    flag.fill_(_I32_MAX)
    if n == 0:
        return F
    if _impl == "torch" or (F.is_cuda and settings.force_cpu_fallback):
        return _ilu0_factor_torch(indptr, indices, F, diag_pos, sched, flag)
    if F.is_cuda:
        ext = _cext.require_hip()
        ext.ilu0_factor(indptr.data_ptr(), indices.data_ptr(), F.data_ptr(),
                        diag_pos.data_ptr(), sched.order.data_ptr(),
                        sched.level_ptr.data_ptr(), flag.data_ptr(), n,
                        F.numel(), sched.level_ptr_host.data_ptr(),
                        sched.n_levels, plan.data_ptr(), int(plan.shape[0]),
                        int(max_row_nnz) > 32, cap, _code(F),
                        _icode(indices), _stream())
        return F
    bad = _cext.require_cpu().ilu0_factor(
        indptr.data_ptr(), indices.data_ptr(), F.data_ptr(),
        diag_pos.data_ptr(), n, _code(F), _icode(indices))
    if bad < n:
        flag.fill_(int(bad))
    return F


def _ilu0_factor_torch(indptr, indices, F, dpos, sched, flag):
    """Per-level torch formulation: within a level, step p handles the p-th
    lower entry of every row that has one; the (row, column) targets of the
    updates are found by searchsorted in the row-major keys."""
    dev = F.device
    n = int(indptr.numel()) - 1
    nnz = int(F.numel())
    row_of = torch.repeat_interleave(torch.arange(n, device=dev),
                                     indptr[1:] - indptr[:-1])
    idx = indices.long()
    keys = row_of * n + idx
    nlow = dpos - indptr[:-1]
    lp = sched.level_ptr_host.tolist()
    for lv in range(1, sched.n_levels):
        rows = sched.order[lp[lv]:lp[lv + 1]]
        low = nlow[rows]
        for p in range(int(low.max())):
            act = rows[low > p]
            pos = indptr[act] + p
            kr = idx[pos]
            aik = F[pos] / F[dpos[kr]]
            F[pos] = aik
            us = dpos[kr] + 1
            cnt = indptr[kr + 1] - us
            off = torch.cumsum(cnt, 0) - cnt
            seg = torch.repeat_interleave(
                torch.arange(act.numel(), device=dev), cnt)
            q = us[seg] + (torch.arange(seg.numel(), device=dev) - off[seg])
            tgt = act[seg] * n + idx[q]
            loc = torch.searchsorted(keys, tgt).clamp(max=nnz - 1)
            hit = keys[loc] == tgt
            loc, seg, q = loc[hit], seg[hit], q[hit]
            F[loc] = F[loc] - aik[seg] * F[q]      # distinct positions
    piv = F[dpos]
    bad = (piv == 0) | ~torch.isfinite(piv)
    first = torch.where(bad, torch.arange(n, device=dev),
                        torch.full((), _I32_MAX, device=dev)).min()
    flag.copy_(first.to(torch.int32).reshape(1))
    return F


# ---------------------------------------------------------------------------
# FSAI setup (docs/DESIGN.md §18): row i of G on its sorted pattern P_i
# (last entry i) is the last row of C^{-1}, A[P_i, P_i] = C C^H.  Rows are
# independent: one launch, one sub-wave per row.
# ---------------------------------------------------------------------------
FSAI_MAX_ROW = 32
# longest pattern row the 8-lane mapping takes (the extension exports the
# same numbers; tests compare them)
FSAI_NARROW = 8
FSAI_GRID_CAP = 4096
# blocks the torch arm factors at a time: chunk * max_row**2 entries
_FSAI_TORCH_CHUNK_ENTRIES = 1 << 24


def _fsai_check(p_indptr, p_indices, w_indptr, w_indices, w_vals,
                row_offset, row_lo, flag, max_row, out, validate):
    if w_vals.dtype not in _DTYPE_CODE or w_indices.dtype not in _IDX_CODE:
        raise ValueError("fsai_rows: unsupported value or index dtype")
    dev = w_vals.device
    n = int(p_indptr.numel()) - 1
    n_win = int(w_indptr.numel()) - 1
    if n < 0 or n_win < 0:
        raise ValueError("fsai_rows: indptr arrays need at least one entry")
    for t, dt in ((p_indptr, torch.int64), (w_indptr, torch.int64),
                  (p_indices, w_indices.dtype), (w_indices, w_indices.dtype),
                  (w_vals, w_vals.dtype), (out, w_vals.dtype)):
        if (t.dtype != dt or t.ndim != 1 or t.device != dev
                or not t.is_contiguous()):
            raise ValueError("fsai_rows: needs contiguous 1-D arrays on one "
                             "device, int64 indptr, one index dtype and one "
                             "value dtype")
    if w_vals.numel() != w_indices.numel() \
            or out.numel() != p_indices.numel():
        raise ValueError("fsai_rows: values do not match their indices")
    if (flag.dtype != torch.int32 or flag.numel() != 1
            or flag.device != dev):
        raise ValueError("fsai_rows: flag is one int32 on the matrix's "
                         "device")
    if not 1 <= int(max_row) <= FSAI_MAX_ROW:
        raise ValueError(f"fsai_rows: longest row {max_row} outside "
                         f"[1, FSAI_MAX_ROW = {FSAI_MAX_ROW}]")
    if n > _I32_MAX:
        raise ValueError("fsai_rows: too many local rows")
    if not validate or n == 0:
        return n, n_win
    # the kernels take raw pointers: everything they index is checked here
    # (index arithmetic on the device, two host reads: the indptr arrays
    # first, because the index checks below rely on them)
    plen = p_indptr[1:] - p_indptr[:-1]
    wlen = w_indptr[1:] - w_indptr[:-1]
    pnnz, wnnz = int(p_indices.numel()), int(w_indices.numel())
    bad = [p_indptr[0] != 0, p_indptr[-1] != pnnz, (plen < 1).any(),
           (plen > int(max_row)).any(), w_indptr[0] < 0,
           w_indptr[-1] > wnnz, (wlen < 0).any()]
    shape_bad = torch.stack([b.reshape(()) for b in bad]).cpu().tolist()
    if any(shape_bad[:4]):
        raise ValueError("fsai_rows: the pattern's indptr is inconsistent, a "
                         "row is empty or a row is longer than max_row")
    if any(shape_bad[4:]):
        raise ValueError("fsai_rows: the window's indptr is inconsistent")
    col = p_indices.long()
    row_of = torch.repeat_interleave(torch.arange(n, device=dev), plen)
    inc = torch.ones(pnnz, dtype=torch.bool, device=dev)
    inc[1:] = (col[1:] > col[:-1]) | (row_of[1:] != row_of[:-1])
    last = col[p_indptr[1:] - 1]
    lo, hi = int(row_offset), int(row_offset) + n_win
    wcol_bad = (w_indices < 0).any() if wnnz else inc.new_zeros(())
    checks = torch.stack([
        (~inc).any(),
        (last != torch.arange(n, device=dev) + int(row_lo)).any(),
        ((col < lo) | (col >= hi)).any(), wcol_bad]).cpu().tolist()
    if checks[0]:
        raise ValueError("fsai_rows: pattern rows must be sorted and free "
                         "of duplicates")
    if checks[1]:
        raise ValueError("fsai_rows: every pattern row must end with its "
                         "diagonal entry")
    if checks[2]:
        raise ValueError(f"fsai_rows: the window rows [{lo}, {hi}) do not "
                         f"cover the pattern's columns")
    if checks[3]:
        raise ValueError("fsai_rows: negative window column")
    return n, n_win


def fsai_rows(p_indptr: torch.Tensor, p_indices: torch.Tensor,
              w_indptr: torch.Tensor, w_indices: torch.Tensor,
              w_vals: torch.Tensor, row_offset: int, row_lo: int,
              flag: torch.Tensor, max_row: int,
              out: Optional[torch.Tensor] = None, _impl: str = "native",
              _grid_cap=None, _validate: bool = True) -> torch.Tensor:
    """Values of the FSAI factor G in the pattern's layout.

    ``p_indptr`` / ``p_indices``: the pattern of this rank's rows, GLOBAL
    sorted columns, the last entry of local row r being its diagonal
    ``row_lo + r``.  ``w_*``: a CSR window of the Hermitian positive
    definite matrix holding its rows ``[row_offset, row_offset + n_win)``
    with global sorted columns; it must cover every pattern column.  Only
    window entries with ``col <= row`` are read.  ``max_row`` bounds the
    longest pattern row (<= FSAI_MAX_ROW) and picks the sub-wave width: 8
    lanes up to FSAI_NARROW, else 32.  ``flag`` (one int32 on the device)
    receives the smallest local row with a pivot that is not positive and
    finite, or 2**31 - 1; nothing is read back from the kernel here.
    ``_validate=False`` skips the argument checks that read the index
    arrays (the caller vouches for arrays that passed them before).
    Bit-identical from run to run."""
    if _impl not in _SPTRSV_IMPLS:
        raise ValueError(f"_impl must be one of {_SPTRSV_IMPLS}")
    if out is None:
        out = torch.empty(p_indices.numel(), dtype=w_vals.dtype,
                          device=w_vals.device)
    n, n_win = _fsai_check(p_indptr, p_indices, w_indptr, w_indices, w_vals,
                           row_offset, row_lo, flag, max_row, out, _validate)
    if _grid_cap is not None and not 1 <= int(_grid_cap) <= FSAI_GRID_CAP:
        raise ValueError(f"_grid_cap outside [1, {FSAI_GRID_CAP}]")
    cap = 0 if _grid_cap is None else int(_grid_cap)
    flag.fill_(_I32_MAX)
    if n == 0:
        return out
    if _impl == "torch" or (out.is_cuda and settings.force_cpu_fallback):
        return _fsai_rows_torch(p_indptr, p_indices, w_indptr, w_indices,
                                w_vals, int(row_offset), flag, int(max_row),
                                out)
    if out.is_cuda:
        ext = _cext.require_hip()
        ext.fsai_rows(p_indptr.data_ptr(), p_indices.data_ptr(),
                      p_indices.numel(), w_indptr.data_ptr(),
                      w_indices.data_ptr(), w_vals.data_ptr(), n_win,
                      w_indices.numel(), int(row_offset), int(row_lo), n,
                      out.data_ptr(), flag.data_ptr(), int(max_row), cap,
                      _code(w_vals), _icode(w_indices), _stream())
        return out
    bad = _cext.require_cpu().fsai_rows(
        p_indptr.data_ptr(), p_indices.data_ptr(), w_indptr.data_ptr(),
        w_indices.data_ptr(), w_vals.data_ptr(), n_win, int(row_offset),
        int(row_lo), n, out.data_ptr(), _code(w_vals), _icode(w_indices))
    if bad < n:
        flag.fill_(int(bad))
    return out


def _fsai_rows_torch(p_indptr, p_indices, w_indptr, w_indices, w_vals,
                     row_offset, flag, max_row, out):
    """Batched dense formulation: every row's block padded to ``max_row``
    with identity, S looked up by searchsorted on row * K + col keys of the
    window, batched Cholesky and one triangular solve per block."""
    dev = out.device
    n = int(p_indptr.numel()) - 1
    n_win = int(w_indptr.numel()) - 1
    pnnz, wnnz = int(p_indices.numel()), int(w_indices.numel())
    Mx = int(max_row)
    pcol = p_indices.long()
    wcol = w_indices.long()
    K = int(max(int(pcol.max()), int(wcol.max()) if wnnz else 0)) + 1
    wrow = torch.repeat_interleave(
        torch.arange(n_win, device=dev) + row_offset,
        w_indptr[1:] - w_indptr[:-1])
    wkeys = wrow * K + wcol
    plen = p_indptr[1:] - p_indptr[:-1]
    ar = torch.arange(Mx, device=dev)
    tril = ar[:, None] >= ar[None, :]
    eye = torch.eye(Mx, dtype=out.dtype, device=dev)
    first = torch.full((), _I32_MAX, dtype=torch.int64, device=dev)
    chunk = max(1, _FSAI_TORCH_CHUNK_ENTRIES // (Mx * Mx))
    for r0 in range(0, n, chunk):
        r1 = min(n, r0 + chunk)
        ln = plen[r0:r1]
        valid = ar[None, :] < ln[:, None]
        pos = (p_indptr[r0:r1, None] + ar[None, :]).clamp(max=pnnz - 1)
        cols = torch.where(valid, pcol[pos], torch.zeros_like(pos))
        both = valid[:, :, None] & valid[:, None, :] & tril[None]
        tk = cols[:, :, None] * K + cols[:, None, :]
        if wnnz:
            loc = torch.searchsorted(wkeys, tk.reshape(-1)).reshape(
                tk.shape).clamp(max=wnnz - 1)
            hit = both & (wkeys[loc] == tk)
            S = torch.where(hit, w_vals[loc], torch.zeros_like(w_vals[:1]))
        else:
            S = torch.zeros(tk.shape, dtype=out.dtype, device=dev)
        dg = torch.diagonal(S, dim1=1, dim2=2)
        S = S + S.mH - torch.diag_embed(dg)
        S = S + eye[None] * (~valid)[:, :, None].to(out.dtype)
        L, info = torch.linalg.cholesky_ex(S)
        E = (ar[None, :] == (ln[:, None] - 1)).to(out.dtype).unsqueeze(-1)
        w = torch.linalg.solve_triangular(L.mH, E, upper=True)[:, :, 0]
        out[p_indptr[r0]:p_indptr[r1]] = w.conj()[valid]
        wr = torch.view_as_real(w) if w.is_complex() else w.unsqueeze(-1)
        bad = (info != 0) | ~torch.isfinite(wr).all(dim=-1).all(dim=-1)
        rows = torch.arange(r0, r1, device=dev)
        first = torch.minimum(first, torch.where(
            bad, rows, torch.full_like(rows, _I32_MAX)).min())
    flag.copy_(first.to(torch.int32).reshape(1))
    return out

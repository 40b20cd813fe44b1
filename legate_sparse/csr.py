# SPDX-License-Identifier: Apache-2.0
"""CSR array: the core distributed sparse type.

MI355X-native re-design of the reference's ``legate_sparse/csr.py``
(csr_array, csr.py:89-748).  Differences by design:

- Legion stores → torch tensors; pos Rect<1> arrays → plain ``indptr``.
- Legion auto-partitioning → explicit equal 1-D row partition: rank r owns
  global rows [lo, hi) of every matrix (reference csr.py:587 align).
- Legion image constraints → explicit RCCL collectives: x all-gather for the
  SpMV halo (reference csr.py:591 MIN_MAX image), B-row all-gather for
  SpGEMM (csr.py:656-666 images), all-to-allv for transpose
  (csr.py:512-544 semantics).
- cuSPARSE → hand-written gfx950 HIP kernels (src/hip/).

SPMD conventions (world_size > 1):
- Constructors take GLOBAL (replicated) inputs and keep only local rows.
- Dense vectors passed to ``dot``/``__matmul__`` may be either global
  (length N, replicated) or local shards (length = partition(N) count);
  results are LOCAL shards of partition(M).
"""
from __future__ import annotations

from typing import Optional, Tuple

import numpy as np
import torch

import warnings

from . import _cext, comm, ops
from .base import CompressedBase, as_torch_1d
from .lsarray import lsarray
from .runtime import runtime
from .types import to_numpy_dtype, to_torch_dtype

_INDEX_DTYPE = torch.int64
_UID = 0


def _index_dtype_for(shape) -> torch.dtype:
    """int32 column indices whenever the matrix allows — halves the
    streamed index bytes of the memory-bound SpMV/SpGEMM kernels."""
    return torch.int32 if max(int(shape[0]), int(shape[1])) < 2**31 - 1 \
        else torch.int64


def _default_device() -> torch.device:
    return runtime.device


def _coerce_2d(x) -> torch.Tensor:
    if isinstance(x, torch.Tensor):
        t = x
    else:
        t = torch.from_numpy(np.ascontiguousarray(x))
    if t.ndim != 2:
        raise ValueError("expected a 2-D array")
    return t


def _check_value_dtype(tdt: torch.dtype):
    if tdt not in (torch.float32, torch.float64, torch.complex64,
                   torch.complex128):
        raise NotImplementedError(
            f"unsupported dtype {tdt}; supported: float32, float64, "
            "complex64, complex128")


def _common_dtype(*tensors) -> torch.dtype:
    dt = tensors[0].dtype
    for t in tensors[1:]:
        dt = torch.promote_types(dt, t.dtype)
    _check_value_dtype(dt)
    return dt


def _route_to_row_owners(row, col, val, part):
    """All-to-allv COO entries to the ranks owning their rows (the
    explicit analogue of Legion moving data to match the row partition).
    ``row`` carries GLOBAL row ids; every rank may hold an arbitrary
    subset.  Returns the entries this rank owns (rows still global)."""
    ws = runtime.world_size
    if ws == 1:
        return row, col, val
    owner = torch.clamp(
        torch.div(row, max(part.chunk, 1), rounding_mode="floor"),
        max=ws - 1)
    order = torch.argsort(owner, stable=True)
    row, col, val, owner = row[order], col[order], val[order], owner[order]
    counts = torch.bincount(owner.cpu().long(), minlength=ws).tolist()
    row = torch.cat(comm.alltoallv(list(torch.split(row, counts))))
    col = torch.cat(comm.alltoallv(list(torch.split(col, counts))))
    val = torch.cat(comm.alltoallv(list(torch.split(val, counts))))
    return row, col, val


def _assemble_local_rows(row_local, col, val, lr, N, dedup=True):
    """Sort (row, col), optionally sum duplicates, build local indptr.
    Shared by the COO constructor, transpose, and gallery.rmat."""
    dev = val.device
    if row_local.numel():
        key = row_local * N + col
        order = torch.argsort(key)
        row_local, col, val, key = (row_local[order], col[order],
                                    val[order], key[order])
        if dedup:
            uniq, inverse = torch.unique_consecutive(key,
                                                     return_inverse=True)
            if uniq.numel() != key.numel():
                newval = torch.zeros(uniq.numel(), dtype=val.dtype,
                                     device=dev)
                newval.index_add_(0, inverse, val)
                val = newval
                row_local = torch.div(uniq, N, rounding_mode="floor")
                col = uniq - row_local * N
    cnt = torch.bincount(row_local, minlength=lr)
    indptr = torch.zeros(lr + 1, dtype=torch.int64, device=dev)
    torch.cumsum(cnt, dim=0, out=indptr[1:])
    return indptr, col, val


class _AffinePlan(tuple):
    """(nd, D int32, mask uint8, rest rows, xconsec), plus the per-tile
    table ``tile_base`` carried as an attribute so the 5-field shape the
    callers unpack stays what it was."""
    tile_base = None


def _affine_tile_table(indptr: torch.Tensor, mask: torch.Tensor,
                       tile: int) -> torch.Tensor:
    """int64[ceil(n / tile)]: indptr[t*tile] where all ``tile`` rows of
    tile t exist and conform (mask == 1), else -1.  Inside such a tile
    row r starts at tile_base[t] + (r - t*tile) * nd, so the kernel
    reads neither indptr nor mask there."""
    n = mask.numel()
    n_full = n // tile
    tb = torch.full(((n + tile - 1) // tile,), -1, dtype=torch.int64,
                    device=mask.device)
    if n_full:
        full = mask[:n_full * tile].view(n_full, tile).min(dim=1).values
        tb[:n_full] = torch.where(full != 0,
                                  indptr[0:n_full * tile:tile],
                                  tb[:n_full])
    return tb


def _build_affine_plan(indptr: torch.Tensor, indices: torch.Tensor,
                       max_extent: int):
    """Detect the affine-stencil structure of a LOCAL CSR block: rows
    whose columns are exactly ``row + D[j]`` (5-pt Poisson, banded
    operators, gallery stencils — and their interior/halo split pieces
    in the distributed path).  Such rows never read the index stream in
    SpMV — 8 B/nnz instead of 12 B/nnz on the memory-bound path (the
    DIA-style structural specialization the CSR format hides).  Returns
    (nd, D int32, mask uint8, rest rows, xconsec) or None, with the
    per-tile table ``.tile_base`` (see _affine_tile_table) attached for
    device tensors; exception rows (grid boundaries) go through the
    general gather kernel from the ``rest`` list."""
    ip, ix = indptr, indices
    n = ip.numel() - 1
    dev = ix.device
    # int32 offsets only; detection needs a real population
    if not (n >= 64 and ix.numel() >= n
            and max_extent < 2 ** 31 - 1):
        return None
    cnt = ip[1:] - ip[:-1]
    bc = torch.bincount(torch.clamp(cnt, max=17))
    nd = int(bc.argmax())
    if not (1 <= nd <= 16 and int(bc[nd]) >= 0.75 * n):
        return None
    rows_c = torch.nonzero(cnt == nd).reshape(-1)
    starts = ip[:-1][rows_c]
    first = int(rows_c[0])
    s0 = int(ip[first])
    D = ix[s0:s0 + nd].long() - first
    offs = torch.arange(nd, device=dev)
    mask = torch.zeros(n, dtype=torch.uint8, device=dev)
    CH = 1 << 22  # bound the (rows, nd) gather temporaries
    for c0 in range(0, rows_c.numel(), CH):
        rc = rows_c[c0:c0 + CH]
        st = starts[c0:c0 + CH]
        cols = ix[st.unsqueeze(1) + offs].long()
        ok = (cols == rc.unsqueeze(1) + D).all(dim=1)
        mask[rc[ok]] = 1
    good = int(mask.sum())
    if good < 0.75 * n:
        return None
    rest = torch.nonzero(mask == 0).reshape(-1)
    xconsec = bool((D == (torch.arange(nd, device=dev) + D[0])).all())
    plan = _AffinePlan((nd, D.to(torch.int32).contiguous(), mask,
                        rest.contiguous(), xconsec))
    if mask.is_cuda and _cext.has_hip():
        # the tile size is the kernel's: read it from the extension
        plan.tile_base = _affine_tile_table(
            ip, mask, _cext.hip_kernels.AFFINE_TILE)
    return plan


# a matrix whose constant-tile table went stale this many times stops
# being scanned: an application that rewrites its coefficients every step
# must not pay the detection pass (one read of vals) every step
_CONST_MAX_INVALIDATIONS = 2


class _AffineConst:
    """Value-bound companion of an affine plan: ``tile_cbase`` marks the
    full tiles whose every row holds the values ``C`` bit for bit with
    -2 (the SpMV kernel then reads no value stream there).  Valid only
    for the plan object, the values buffer and the version of its
    contents it was built from."""
    __slots__ = ("tile_cbase", "C", "plan", "data_ptr", "version")

    def __init__(self, tile_cbase, C, plan, vals):
        self.tile_cbase = tile_cbase
        self.C = C
        self.plan = plan
        self.data_ptr = vals.data_ptr()
        self.version = vals._version

    def matches(self, plan, vals) -> bool:
        return (self.plan is plan and self.data_ptr == vals.data_ptr()
                and self.version == vals._version)


def _affine_const_table(plan, vals: torch.Tensor):
    """(tile_cbase, C) of ``vals`` under ``plan``, or None when there is
    nothing to scan: no tile table, no full tile, a complex dtype (the
    constant-tile kernels are instantiated for real values only) or an
    fp32 stencil wider than the extension's AFFINE_CONST_F32_ND (past it
    the kernel pair would not give the same bits, see spmv.hip).  C is
    the first row of the first full tile; the scan is one native pass
    over ``vals`` (ls_affine_const_tiles)."""
    tb = getattr(plan, "tile_base", None) if plan is not None else None
    if tb is None or not vals.is_cuda or vals.is_complex() \
            or not _cext.has_hip():
        return None
    if vals.dtype == torch.float32 and \
            int(plan[0]) > _cext.hip_kernels.AFFINE_CONST_F32_ND:
        return None
    full = torch.nonzero(tb >= 0)
    if not full.numel():
        return None
    nd = int(plan[0])
    s0 = int(tb[int(full[0])])
    C = vals[s0:s0 + nd].clone()
    cb = torch.empty_like(tb)
    _cext.require_hip().affine_const_tiles(
        vals.data_ptr(), tb.data_ptr(), C.data_ptr(), cb.data_ptr(),
        tb.numel(), nd, ops._code(vals),
        torch.cuda.current_stream().cuda_stream)
    return cb, C


def _build_affine_const(plan, vals: torch.Tensor):
    """The constant-tile table of ``vals`` under ``plan`` as an
    _AffineConst, or None when no tile comes out constant."""
    res = _affine_const_table(plan, vals)
    if res is None or not bool((res[0] == -2).any()):
        return None
    return _AffineConst(res[0], res[1], plan, vals)


import scipy.sparse as _scipy_sparse

from .coverage import clone_scipy_arr_kind


@clone_scipy_arr_kind(_scipy_sparse.csr_array)
class csr_array(CompressedBase):
    """scipy.sparse.csr_array-compatible distributed CSR matrix."""

    format = "csr"

    # ------------------------------------------------------------------
    # Constructors (reference csr.py:89-286)
    # ------------------------------------------------------------------
    def __init__(self, arg, shape=None, dtype=None, copy: bool = False,
                 local: bool = False, _local=None):
        """``local=True`` declares PRE-SHARDED input (VERDICT r01 item 5 —
        the replicated-global ctor contract breaks at 288 GB-scale):

        - COO ``(data, (row, col))``: this rank holds an arbitrary subset
          of the GLOBAL entries (row ids global); entries are routed to
          their row owners with one all-to-allv, nothing replicated.
        - CSR triple ``(data, indices, indptr)``: the triple describes
          exactly this rank's row block of the equal row partition.
        """
        if _local is not None:
            # internal fast path: (indptr, indices, data) already LOCAL
            indptr, indices, data = _local
            self._init_local(indptr, indices, data, shape)
            return
        if local:
            self._from_sharded(arg, shape, dtype)
            return

        device = _default_device()
        tdt = to_torch_dtype(dtype) if dtype is not None else None

        if isinstance(arg, csr_array):
            self._init_local(
                arg._indptr.clone(), arg._indices.clone(),
                arg._data.clone() if tdt is None else arg._data.to(tdt),
                arg.shape)
            return

        # scipy sparse input
        if hasattr(arg, "tocsr") and hasattr(arg, "shape") and not isinstance(
                arg, (tuple, list)):
            sp = arg.tocsr()
            sp.sort_indices()
            self._from_global_csr(
                torch.from_numpy(np.asarray(sp.indptr, dtype=np.int64)),
                torch.from_numpy(np.asarray(sp.indices, dtype=np.int64)),
                torch.from_numpy(np.ascontiguousarray(sp.data)),
                sp.shape, tdt, device)
            return

        if isinstance(arg, (tuple, list)) and len(arg) == 2 and all(
                isinstance(v, (int, np.integer)) for v in arg):
            # empty (M, N)  (reference csr.py:161-181)
            M, N = int(arg[0]), int(arg[1])
            tdt = tdt or torch.float64
            _check_value_dtype(tdt)
            part = runtime.partition(M)
            lr = part.count(runtime.rank)
            self._init_local(
                torch.zeros(lr + 1, dtype=_INDEX_DTYPE, device=device),
                torch.empty(0, dtype=_INDEX_DTYPE, device=device),
                torch.empty(0, dtype=tdt, device=device),
                (M, N))
            return

        if isinstance(arg, (tuple, list)) and len(arg) == 2:
            # COO: (data, (row, col))  (reference csr.py:183-219)
            data, (row, col) = arg
            self._from_global_coo(
                as_torch_1d(data), as_torch_1d(row, dtype=np.int64),
                as_torch_1d(col, dtype=np.int64), shape, tdt, device)
            return

        if isinstance(arg, (tuple, list)) and len(arg) == 3:
            # CSR triple: (data, indices, indptr) GLOBAL
            # (reference csr.py:221-265)
            data, indices, indptr = arg
            self._from_global_csr(
                as_torch_1d(indptr, dtype=np.int64),
                as_torch_1d(indices, dtype=np.int64),
                as_torch_1d(data), shape, tdt, device)
            return

        # dense input (reference csr.py:109-148)
        dense = _coerce_2d(arg)
        if tdt is not None:
            dense = dense.to(tdt)
        _check_value_dtype(dense.dtype)
        M, N = dense.shape
        part = runtime.partition(M)
        lo, hi = part.lo(runtime.rank), part.hi(runtime.rank)
        local = dense[lo:hi].to(device)
        indptr, indices, vals = ops.dense_to_csr(
            local, idx_dtype=_index_dtype_for((M, N)))
        self._init_local(indptr, indices, vals, (M, N))

    def _from_sharded(self, arg, shape, dtype):
        device = _default_device()
        tdt = to_torch_dtype(dtype) if dtype is not None else None
        if shape is None:
            raise ValueError("local=True requires an explicit shape "
                             "(global extents are not discoverable from "
                             "one rank's shard)")
        M, N = int(shape[0]), int(shape[1])
        if isinstance(arg, (tuple, list)) and len(arg) == 2:
            data, (row, col) = arg
            val = as_torch_1d(data, device=device)
            if tdt is not None:
                val = val.to(tdt)
            _check_value_dtype(val.dtype)
            row = as_torch_1d(row, dtype=np.int64, device=device)
            col = as_torch_1d(col, dtype=np.int64, device=device)
            part = runtime.partition(M)
            row, col, val = _route_to_row_owners(row, col, val, part)
            lo, hi = part.lo(runtime.rank), part.hi(runtime.rank)
            indptr, col, val = _assemble_local_rows(row - lo, col, val,
                                                    hi - lo, N, dedup=True)
            self._init_local(indptr, col.to(_INDEX_DTYPE),
                             val.contiguous(), (M, N))
            return
        if isinstance(arg, (tuple, list)) and len(arg) == 3:
            data, indices, indptr = arg
            val = as_torch_1d(data, device=device)
            if tdt is not None:
                val = val.to(tdt)
            _check_value_dtype(val.dtype)
            indices = as_torch_1d(indices, dtype=np.int64, device=device)
            indptr = as_torch_1d(indptr, dtype=np.int64, device=device)
            part = runtime.partition(M)
            lr = part.count(runtime.rank)
            if indptr.numel() != lr + 1:
                raise ValueError(
                    f"local CSR triple: indptr length {indptr.numel()} "
                    f"does not match this rank's row block ({lr} rows)")
            # same canonicalization as the global-triple path
            if indices.numel() > 1:
                row_of = torch.repeat_interleave(
                    torch.arange(lr, device=device),
                    indptr[1:] - indptr[:-1])
                key = row_of * N + indices
                if bool((key[1:] <= key[:-1]).any()):
                    indptr, indices, val = _assemble_local_rows(
                        row_of, indices, val, lr, N, dedup=True)
            self._init_local(indptr, indices.to(_INDEX_DTYPE),
                             val.contiguous(), (M, N))
            return
        raise ValueError(
            "local=True supports (data, (row, col)) or "
            "(data, indices, indptr) inputs")

    def _init_local(self, indptr, indices, data, shape):
        if shape is None:
            raise ValueError("shape required")
        _check_value_dtype(data.dtype)
        self._shape = (int(shape[0]), int(shape[1]))
        self._part = runtime.partition(self._shape[0])
        self._row_lo = self._part.lo(runtime.rank)
        self._row_hi = self._part.hi(runtime.rank)
        assert indptr.numel() == (self._row_hi - self._row_lo) + 1, (
            indptr.numel(), self._row_lo, self._row_hi)
        self._indptr = indptr.contiguous()
        idt = _index_dtype_for(self._shape)
        self._indices = indices.to(idt).contiguous()
        self._data = data.contiguous()
        self._global_nnz: Optional[int] = None
        global _UID
        _UID += 1
        self._uid = _UID          # forever-unique structure identity
        self._struct_version = 0

    def _from_global_csr(self, indptr, indices, data, shape, tdt, device):
        if shape is None:
            M = indptr.numel() - 1
            N = int(indices.max().item()) + 1 if indices.numel() else 0
            shape = (M, N)
        M, N = int(shape[0]), int(shape[1])
        if indptr.numel() - 1 != M:
            raise ValueError("indptr length does not match shape")
        if tdt is not None:
            data = data.to(tdt)
        _check_value_dtype(data.dtype)
        part = runtime.partition(M)
        lo, hi = part.lo(runtime.rank), part.hi(runtime.rank)
        s, e = int(indptr[lo]), int(indptr[hi])
        l_indptr = (indptr[lo:hi + 1] - indptr[lo]).to(device=device,
                                                       dtype=_INDEX_DTYPE)
        l_indices = indices[s:e].to(device=device, dtype=_INDEX_DTYPE)
        l_data = data[s:e].to(device)
        # every kernel (and has_sorted_indices) assumes canonical rows;
        # scipy leaves raw triples unsorted until sort_indices() — here
        # canonical form is established at construction.  Detection is
        # one vectorized pass; the sort runs only when needed.
        if l_indices.numel() > 1:
            lr = hi - lo
            row_of = torch.repeat_interleave(
                torch.arange(lr, device=device),
                l_indptr[1:] - l_indptr[:-1])
            key = row_of * N + l_indices
            # strict increase == sorted AND duplicate-free; equal keys
            # are duplicates to sum (canonical form)
            if bool((key[1:] <= key[:-1]).any()):
                l_indptr, l_indices, l_data = _assemble_local_rows(
                    row_of, l_indices, l_data, lr, N, dedup=True)
        self._init_local(l_indptr, l_indices, l_data, (M, N))

    def _from_global_coo(self, data, row, col, shape, tdt, device):
        if shape is None:
            M = int(row.max().item()) + 1 if row.numel() else 0
            N = int(col.max().item()) + 1 if col.numel() else 0
            shape = (M, N)
        M, N = int(shape[0]), int(shape[1])
        if tdt is not None:
            data = data.to(tdt)
        _check_value_dtype(data.dtype)
        part = runtime.partition(M)
        lo, hi = part.lo(runtime.rank), part.hi(runtime.rank)
        keep = (row >= lo) & (row < hi)
        row, col, data = row[keep] - lo, col[keep], data[keep]
        row, col, data = row.to(device), col.to(device), data.to(device)
        lr = hi - lo
        indptr, col, data = _assemble_local_rows(row, col, data, lr, N,
                                                 dedup=True)
        self._init_local(indptr, col.to(_INDEX_DTYPE),
                         data.contiguous(), (M, N))

    # ------------------------------------------------------------------
    # Properties (reference csr.py:289-336)
    # ------------------------------------------------------------------
    @property
    def shape(self) -> Tuple[int, int]:
        return self._shape

    @property
    def dim(self) -> int:
        return 2

    @property
    def nnz(self) -> int:
        """GLOBAL nnz.  First access is a collective (all-gather of local
        counts) — in SPMD code call it on every rank, never inside a
        rank-guarded branch."""
        if self._global_nnz is None:
            local = self._data.numel()
            if runtime.world_size > 1:
                t = comm.allgather_scalars(local)
                self._global_nnz = int(t.sum().item())
            else:
                self._global_nnz = local
        return self._global_nnz

    @property
    def nnz_local(self) -> int:
        """This rank's stored-entry count — NO collective, safe inside
        rank-guarded code (unlike ``nnz``, whose first access
        all-gathers and must therefore run on every rank)."""
        return self._data.numel()

    @property
    def data(self) -> torch.Tensor:
        return self._data

    @data.setter
    def data(self, new):
        t = as_torch_1d(new, device=self._data.device)
        if t.numel() != self._data.numel():
            raise ValueError("data size mismatch")
        _check_value_dtype(t.dtype)
        self._data = t.contiguous()
        self._ov_cache = None  # halo/interior split caches values
        # the constant-tile table too; a new tensor can reuse the old
        # one's address and version, so mark the entry stale by hand
        if getattr(self, "_const_cache", None) is not None:
            self._const_cache.version = -1

    @property
    def vals(self) -> torch.Tensor:
        """Alias of ``data`` (reference API exposes ``.vals``)."""
        return self._data

    @property
    def indices(self) -> torch.Tensor:
        return self._indices

    @indices.setter
    def indices(self, new):
        """Install new column indices.  Kernels (merge-path SpGEMM,
        stencil SpMV pair loads) assume canonical rows, so arbitrary user
        indices are validated and re-canonicalized here: out-of-bounds
        raises, unsorted rows are sorted (permuting data in step), and
        remaining duplicates are tracked so ``has_canonical_format``
        reports honestly (the reference flips indices_sorted /
        canonical_format flags instead — set_indices semantics)."""
        t = as_torch_1d(new, device=self._data.device)
        if t.numel() != self._indices.numel():
            raise ValueError("indices size mismatch")
        t = t.to(torch.int64)
        N = self._shape[1]
        if t.numel() and (bool((t < 0).any()) or bool((t >= N).any())):
            raise ValueError(f"column index out of bounds [0, {N})")
        if t.numel() > 1:
            lr = self._row_hi - self._row_lo
            row_of = torch.repeat_interleave(
                torch.arange(lr, device=t.device),
                self._indptr[1:] - self._indptr[:-1])
            key = row_of * N + t
            if bool((key[1:] < key[:-1]).any()):     # unsorted: sort rows
                order = torch.argsort(key, stable=True)
                t = t[order]
                self._data = self._data[order].contiguous()
                key = key[order]
            self._canonical = not bool((key[1:] == key[:-1]).any())
        else:
            self._canonical = True
        self._indices = t.to(_index_dtype_for(self._shape)).contiguous()
        self._halo_cache = None
        self._ov_cache = None
        self._max_nnz_cache = None
        self._struct_version += 1
        self._spgemm_cache = None
        self._affine_cache = "unset"

    @property
    def has_sorted_indices(self) -> bool:
        """Column indices are kept sorted within every row: ctors sort,
        SpGEMM sorts in-kernel, and the indices setter re-sorts."""
        return True

    @property
    def has_canonical_format(self) -> bool:
        """Sorted AND duplicate-free rows.  False only after the user
        installs duplicate indices via the setter."""
        return getattr(self, "_canonical", True)

    @property
    def indptr(self) -> torch.Tensor:
        return self._indptr

    @property
    def row_range(self) -> Tuple[int, int]:
        """This rank's global row block [lo, hi)."""
        return self._row_lo, self._row_hi

    def _data_tensor(self) -> torch.Tensor:
        return self._data

    def _with_data(self, data: torch.Tensor) -> "csr_array":
        out = csr_array.__new__(csr_array)
        out._init_local(self._indptr.clone(), self._indices.clone(), data,
                        self._shape)
        return out

    # ------------------------------------------------------------------
    # Core ops
    # ------------------------------------------------------------------
    def _max_row_nnz(self) -> int:
        """Cached max row length (drives the stencil SpMV variant)."""
        if getattr(self, "_max_nnz_cache", None) is None:
            if self._indptr.numel() > 1:
                self._max_nnz_cache = int(
                    (self._indptr[1:] - self._indptr[:-1]).max())
            else:
                self._max_nnz_cache = 0
        return self._max_nnz_cache

    def _affine_plan(self):
        """Cached affine plan over THIS matrix's local tensors —
        see _build_affine_plan."""
        import os as _os
        if _os.environ.get("LS_SPMV_AFFINE", "1") in ("0", "false"):
            return None
        cached = getattr(self, "_affine_cache", "unset")
        if cached != "unset":
            return cached
        plan = _build_affine_plan(self._indptr, self._indices,
                                  max(self._shape))
        self._affine_cache = plan
        return plan

    def _affine_const(self, plan=None):
        """Cached constant-tile table (_AffineConst) of this matrix's
        values under its affine plan, or None.  The cached table is
        returned only while the plan object, ``data.data_ptr()`` and the
        torch ``_version`` of ``data`` are the ones it was built from;
        otherwise it is rebuilt.  The _CONST_MAX_INVALIDATIONS-th time a
        change of VALUES (in-place write or ``data`` assignment under an
        unchanged plan) makes it stale, the matrix stops being scanned;
        a new plan (indices setter, eliminate_zeros) rebuilds without
        counting.  LS_SPMV_AFFINE_CONST=0 (or LS_SPMV_AFFINE_TILES=0)
        returns None."""
        import os as _os
        if not self._data.is_cuda or \
                _os.environ.get("LS_SPMV_AFFINE_CONST", "1") == "0" or \
                _os.environ.get("LS_SPMV_AFFINE_TILES", "1") == "0":
            return None
        if plan is None:
            plan = self._affine_plan()
        if plan is None:
            return None
        d = self._data
        c = getattr(self, "_const_cache", None)
        if c is not None:
            # an _AffineConst; tile_cbase None records "no constant tile"
            if c.matches(plan, d):
                return c if c.tile_cbase is not None else None
            if c.plan is plan:  # same structure: the values changed
                self._const_invalidations = getattr(
                    self, "_const_invalidations", 0) + 1
        if getattr(self, "_const_invalidations", 0) \
                >= _CONST_MAX_INVALIDATIONS:
            self._const_cache = None
            return None
        table = _build_affine_const(plan, d)
        self._const_cache = table if table is not None else \
            _AffineConst(None, None, plan, d)
        return table

    def _spgemm_cache_for(self, B: "csr_array") -> dict:
        """Per-(A,B)-structure cache for repeated products (binning +
        symbolic skip; the analogue of the reference's cached Legion
        partitions that --stable microbenchmark mode exploits)."""
        tok = (B._uid, B._struct_version, self._struct_version)
        c = getattr(self, "_spgemm_cache", None)
        if c is None or c[0] != tok:
            c = (tok, {})
            self._spgemm_cache = c
        return c[1]

    def _halo_plan(self):
        """MIN_MAX column-window halo plan (the explicit replacement of
        the reference's image(crd, x, MIN_MAX) constraint, csr.py:591).

        Each rank needs only x[min_col : max_col+1] of its local matrix;
        the plan (cached — structure is immutable) records that window and
        the per-rank slice exchange realizing it via all-to-allv over
        xGMI, instead of a full x all-gather."""
        if getattr(self, "_halo_cache", None) is not None:
            return self._halo_cache
        N = self._shape[1]
        part = runtime.partition(N)
        ws = runtime.world_size
        if self._indices.numel():
            mn = int(self._indices.min())
            mx = int(self._indices.max()) + 1
        else:
            mn = part.lo(runtime.rank)
            mx = mn
        wins = comm.allgather_scalars(mn).tolist(), \
            comm.allgather_scalars(mx).tolist()
        mns, mxs = wins
        lo, hi = part.lo(runtime.rank), part.hi(runtime.rank)
        send = []
        for r in range(ws):
            a = max(lo, int(mns[r]))
            b = min(hi, int(mxs[r]))
            send.append((a - lo, max(0, b - a)))
        recv_counts = []
        for r in range(ws):
            a = max(part.lo(r), mn)
            b = min(part.hi(r), mx)
            recv_counts.append(max(0, b - a))
        # GLOBAL halo participation flag: rank r has halo work iff its
        # column window leaves its own x shard.  The exchange is a
        # collective, so EVERY rank must take the same branch even when
        # its own halo is empty (asymmetric structure — e.g. restriction
        # operators — would otherwise deadlock/mismatch the collective).
        any_halo = any(
            int(mns[r]) < part.lo(r) or int(mxs[r]) > part.hi(r)
            for r in range(ws))
        self._halo_cache = {
            "min_col": mn, "win": mx - mn, "send": send,
            "recv_counts": recv_counts, "any_halo": any_halo,
        }
        return self._halo_cache

    def _gather_x(self, x: torch.Tensor):
        """Produce the x window needed by local SpMV; returns
        (x_window, col_offset) where the kernel reads x_window[c - off]."""
        N = self._shape[1]
        if x.numel() == N:
            return x, 0  # replicated input: nothing to move
        part = runtime.partition(N)
        if x.numel() != part.count(runtime.rank):
            raise ValueError(
                f"x length {x.numel()} is neither global ({N}) nor the "
                f"local shard ({part.count(runtime.rank)})")
        if runtime.world_size == 1:
            return x, 0
        plan = self._halo_plan()
        chunks = [x[s:s + c] for (s, c) in plan["send"]]
        recv = comm.alltoallv(chunks)
        x_win = torch.cat(recv) if len(recv) > 1 else recv[0]
        assert x_win.numel() == plan["win"], (x_win.numel(), plan)
        return x_win, plan["min_col"]

    def _split_for_overlap(self):
        """Cached interior/halo split of the local rows: interior columns
        fall in this rank's own x shard (no comm), halo columns don't.
        Enables overlapping the halo all-to-all with the interior SpMV
        (the overlap Legion gave the reference for free — SURVEY §2.4)."""
        if getattr(self, "_ov_cache", None) is not None:
            return self._ov_cache
        N = self._shape[1]
        part = runtime.partition(N)
        lo, hi = part.lo(runtime.rank), part.hi(runtime.rank)
        lr = self._row_hi - self._row_lo
        dev = self._data.device
        idx = self._indices.long()
        mask = (idx >= lo) & (idx < hi)
        row_ids = torch.repeat_interleave(
            torch.arange(lr, device=dev), self._indptr[1:] - self._indptr[:-1])

        def build(m):
            cnt = torch.bincount(row_ids[m], minlength=lr)
            ip = torch.zeros(lr + 1, dtype=torch.int64, device=dev)
            torch.cumsum(cnt, dim=0, out=ip[1:])
            mx = int(cnt.max()) if cnt.numel() else 0
            return (ip, self._indices[m].contiguous(),
                    self._data[m].contiguous(), mx)

        interior = build(mask)
        halo = build(~mask)
        # the interior piece of a stencil operator is itself affine
        # (minus shard-boundary rows): the distributed SpMV's dominant
        # kernel gets the index-stream-free path too
        import os as _os
        plan_i = None
        if self._data.is_cuda and _os.environ.get(
                "LS_SPMV_AFFINE", "1") not in ("0", "false"):
            plan_i = _build_affine_plan(interior[0], interior[1],
                                        max(self._shape))
        # dv_i is private to this cache and rebuilt with it, so its
        # constant-tile table is built once here, keyed to dv_i
        const_i = None
        if plan_i is not None and \
                _os.environ.get("LS_SPMV_AFFINE_CONST", "1") != "0" and \
                _os.environ.get("LS_SPMV_AFFINE_TILES", "1") != "0":
            const_i = _build_affine_const(plan_i, interior[2])
        self._ov_cache = (interior, halo, plan_i, const_i)
        return self._ov_cache

    def _matvec_dist(self, x: torch.Tensor,
                     y: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Distributed matvec with comm/compute overlap: the halo
        all-to-all runs async (RCCL stream) while the interior SpMV
        computes on the compute stream; the halo part then accumulates.

        LS_PRECISE_IMAGES=0 falls back to a full x all-gather with no
        window/overlap (the coarse-image escape hatch; the reference's
        LEGATE_SPARSE_PRECISE_IMAGES analogue)."""
        from .settings import settings as _settings
        if not _settings.precise_images:
            part_x = runtime.partition(self._shape[1])
            x_full = comm.allgatherv(x, part_x.counts())
            return ops.spmv(self._indptr, self._indices, self._data,
                            x_full, y)
        N = self._shape[1]
        part = runtime.partition(N)
        lo = part.lo(runtime.rank)
        # the plan is collective on first build — every rank must reach it
        # BEFORE any rank-local early-out (asymmetric halos otherwise
        # mismatch the collective ordering)
        plan = self._halo_plan()
        if not plan["any_halo"]:
            # no rank needs remote columns: pure local SpMV everywhere
            aff = self._affine_plan() if self._data.is_cuda else None
            return ops.spmv(self._indptr, self._indices, self._data, x, y,
                            col_offset=lo, max_nnz=self._max_row_nnz(),
                            affine=aff,
                            affine_const=self._affine_const(aff))
        ((ip_i, ix_i, dv_i, mx_i),
         (ip_h, ix_h, dv_h, mx_h), aff_i, const_i) = \
            self._split_for_overlap()
        pieces = [x[s:s + c] for (s, c) in plan["send"] if c > 0]
        send = torch.cat(pieces) if pieces else x[:0]
        x_win, work = comm.alltoallv_single_async(
            send, [c for (_, c) in plan["send"]], plan["recv_counts"])
        y = ops.spmv(ip_i, ix_i, dv_i, x, y, col_offset=lo, max_nnz=mx_i,
                     affine=aff_i, affine_const=const_i)
        if work is not None:
            work.wait()
        if ix_h.numel():
            ops.spmv(ip_h, ix_h, dv_h, x_win, y, accumulate=True,
                     col_offset=plan["min_col"], max_nnz=mx_h)
        return y

    def _matvec_pq(self, p: torch.Tensor, q: torch.Tensor,
                   pq_out: torch.Tensor) -> bool:
        """q = A p AND pq_out = <p, q> in one fused kernel (local part;
        the CG pipeline's dot costs no extra memory pass).  Only for the
        single-device square real path with an affine plan; returns
        False when the caller must fall back to matvec + vdot."""
        if (runtime.world_size > 1 or not self._data.is_cuda
                or self._data.is_complex()
                or self._shape[0] != self._shape[1]
                or p.numel() != self._shape[1]):
            return False
        plan = self._affine_plan()
        if plan is None:
            return False
        ops.spmv(self._indptr, self._indices, self._data, p,
                 q.reshape(-1), affine=plan, dot_out=pq_out,
                 affine_const=self._affine_const(plan))
        return True

    def _coerce_vec(self, other) -> torch.Tensor:
        t = other if isinstance(other, torch.Tensor) else as_torch_1d(other)
        if isinstance(t, torch.Tensor) and t.ndim == 1 \
                and not t.is_contiguous():
            # reference csr.py:446-452: transformed operand stores force an
            # implicit copy and warn; a non-contiguous tensor is the torch
            # analogue (kernels need a flat contiguous window)
            warnings.warn(
                "implicit copy of a non-contiguous operand vector; pass a "
                "contiguous tensor to avoid the copy", RuntimeWarning)
        return t.to(self._data.device).reshape(-1).contiguous()

    def dot(self, other, out: Optional[torch.Tensor] = None):
        # scalar
        if np.isscalar(other) or (isinstance(other, torch.Tensor)
                                  and other.ndim == 0):
            return self.multiply(other)
        if isinstance(other, csr_array):
            if out is not None:
                raise ValueError("out= not supported for SpGEMM")
            return spgemm_csr_csr_csr(self, other)
        t = other if isinstance(other, torch.Tensor) else torch.from_numpy(
            np.ascontiguousarray(other))
        squeezed = False
        if t.ndim == 2 and t.shape[1] == 1:
            t = t.reshape(-1)
            squeezed = True
        if t.ndim != 1:
            raise NotImplementedError(
                "only matrix-vector and matrix-matrix products supported")
        if not (t.dtype.is_floating_point or t.dtype.is_complex):
            raise NotImplementedError(
                f"unsupported operand dtype {t.dtype} "
                "(float32/float64/complex64/complex128 only)")
        dt = _common_dtype(self._data, t)
        x = self._coerce_vec(t).to(dt)
        A = self if self._data.dtype == dt else self.astype(
            to_numpy_dtype(dt))
        lr = self._row_hi - self._row_lo
        np_out = None
        if isinstance(out, np.ndarray):
            # reference examples pass cupynumeric arrays as out=
            # (spmv_microbenchmark.py:21-27); accept a host array of the
            # GLOBAL length and write the gathered result back into it so
            # chained A.dot(y, out=x) keeps working at any world size
            if out.shape[0] != self._shape[0] or \
                    to_torch_dtype(out.dtype) != dt:
                raise ValueError("bad out= vector")
            np_out = out
            out = None
        if out is not None:
            if out.shape[0] != lr or out.dtype != dt:
                raise ValueError("bad out= vector")
            y = out.reshape(-1)
        else:
            y = None
        N = self._shape[1]
        if runtime.world_size > 1 and x.numel() != N:
            y = A._matvec_dist(x, y)
        else:
            x_win, col_off = A._gather_x(x)
            aff = A._affine_plan() if A._data.is_cuda else None
            y = ops.spmv(A._indptr, A._indices, A._data, x_win, y,
                         col_offset=col_off, max_nnz=A._max_row_nnz(),
                         affine=aff, affine_const=A._affine_const(aff))
        if np_out is not None:
            full = y if runtime.world_size == 1 else comm.allgatherv(
                y, self._part.counts())
            flat = np_out.reshape(-1)
            flat[:] = full.detach().cpu().numpy()
            return np_out
        y = lsarray.wrap(y.reshape(-1, 1) if squeezed else y, self._shape[0])
        return y

    def _coerce_mat(self, other) -> torch.Tensor:
        """2-D operand -> row-major tensor on the data's device."""
        copied = False
        if isinstance(other, torch.Tensor):
            t = other
        else:
            a = np.asarray(other)
            if a.ndim == 2 and any(s < 0 for s in a.strides):
                # torch cannot view negative strides: numpy makes the copy
                a = np.ascontiguousarray(a)
                copied = True
            t = torch.from_numpy(a)
        if t.ndim != 2:
            raise ValueError(
                f"matmat expects a 2-D operand, got {t.ndim}-D")
        if copied or not t.is_contiguous():
            warnings.warn(
                "implicit copy of a non-contiguous operand block; pass a "
                "row-major contiguous tensor to avoid the copy",
                RuntimeWarning)
        return t.to(self._data.device).contiguous()

    def _matmat_dist(self, X: torch.Tensor,
                     Y: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Distributed SpMM on a local (shard_rows, k) block of X: the
        block analogue of ``_matvec_dist``.  Row-major row ranges are
        contiguous, so the vector exchange carries over with every count
        multiplied by k; the cached halo plan and interior/halo split are
        reused as they are."""
        from .settings import settings as _settings
        k = int(X.shape[1])
        N = self._shape[1]
        part = runtime.partition(N)
        if not _settings.precise_images:
            x_full = comm.allgatherv(X.reshape(-1),
                                     [c * k for c in part.counts()])
            return ops.spmm(self._indptr, self._indices, self._data,
                            x_full.reshape(N, k), Y)
        lo = part.lo(runtime.rank)
        # collective on first build: reached by every rank before any
        # rank-local early-out, and all ranks branch on the GLOBAL
        # any_halo flag (see _matvec_dist)
        plan = self._halo_plan()
        if not plan["any_halo"]:
            return ops.spmm(self._indptr, self._indices, self._data, X, Y,
                            col_offset=lo)
        ((ip_i, ix_i, dv_i, _),
         (ip_h, ix_h, dv_h, _), _, _) = self._split_for_overlap()
        pieces = [X[s:s + c].reshape(-1) for (s, c) in plan["send"]
                  if c > 0]
        send = torch.cat(pieces) if pieces else X.reshape(-1)[:0]
        x_win, work = comm.alltoallv_single_async(
            send, [c * k for (_, c) in plan["send"]],
            [c * k for c in plan["recv_counts"]])
        Y = ops.spmm(ip_i, ix_i, dv_i, X, Y, col_offset=lo)
        if work is not None:
            work.wait()
        if ix_h.numel():
            ops.spmm(ip_h, ix_h, dv_h, x_win.reshape(plan["win"], k), Y,
                     accumulate=True, col_offset=plan["min_col"])
        return Y

    def matmat(self, X, out=None):
        """``Y = A @ X`` for a dense block ``X`` of shape (N, k) or this
        rank's (shard_rows, k) block of it; returns this rank's
        (local_rows, k) block, row-major.  One pass over the matrix for
        all k columns.  (``dot``/``@`` still reject 2-D dense operands;
        routing them here is a follow-up.)"""
        t = X if isinstance(X, torch.Tensor) else np.asarray(X)
        if t.ndim != 2:
            raise ValueError(f"matmat expects a 2-D operand, got {t.ndim}-D")
        if isinstance(t, torch.Tensor):
            tdt = t.dtype
        elif t.dtype.kind in "fc":
            tdt = torch.from_numpy(np.empty(0, dtype=t.dtype)).dtype
        else:
            tdt = None
        if tdt is None or not (tdt.is_floating_point or tdt.is_complex):
            raise NotImplementedError(
                f"unsupported operand dtype {t.dtype} "
                "(float32/float64/complex64/complex128 only)")
        dt = torch.promote_types(self._data.dtype, tdt)
        _check_value_dtype(dt)
        Xc = self._coerce_mat(t).to(dt)
        A = self if self._data.dtype == dt else self.astype(
            to_numpy_dtype(dt))
        M, N = self._shape
        lr = self._row_hi - self._row_lo
        k = int(Xc.shape[1])
        shard = runtime.partition(N).count(runtime.rank)
        if Xc.shape[0] != N and Xc.shape[0] != shard:
            raise ValueError(
                f"X row count {Xc.shape[0]} is neither global ({N}) nor "
                f"the local shard ({shard})")
        np_out = None
        Y = None
        if isinstance(out, np.ndarray):
            # host array of the GLOBAL shape, filled with the gathered
            # result (as dot does for vectors)
            if out.shape != (M, k) or out.dtype != to_numpy_dtype(dt):
                raise ValueError(
                    f"bad out= block: numpy out must be the global "
                    f"({M}, {k}) of dtype {dt}")
            np_out = out
        elif out is not None:
            if not isinstance(out, torch.Tensor) \
                    or out.device != self._data.device \
                    or tuple(out.shape) != (lr, k) or out.dtype != dt \
                    or not out.is_contiguous():
                raise ValueError(
                    f"bad out= block: need a contiguous ({lr}, {k}) "
                    f"{dt} tensor on {self._data.device}")
            Y = out
        if k == 0:
            if np_out is not None:
                return np_out
            if Y is None:
                Y = torch.empty((lr, 0), dtype=dt, device=self._data.device)
            return lsarray.wrap(Y, M)
        if runtime.world_size > 1 and Xc.shape[0] != N:
            Y = A._matmat_dist(Xc, Y)
        else:
            # replicated X (or a single rank): global columns index X
            # directly, no communication at any world size
            Y = ops.spmm(A._indptr, A._indices, A._data, Xc, Y)
        if np_out is not None:
            full = Y if runtime.world_size == 1 else comm.allgatherv(
                Y.reshape(-1),
                [c * k for c in self._part.counts()]).reshape(M, k)
            np_out[...] = full.detach().cpu().numpy()
            return np_out
        return lsarray.wrap(Y, M)

    def __matmul__(self, other):
        return self.dot(other)

    def __rmatmul__(self, other):
        """x @ A == (A.T @ x) for 1-D x (reference csr.py:412-414)."""
        t = other if isinstance(other, torch.Tensor) else torch.from_numpy(
            np.ascontiguousarray(other))
        if t.ndim == 1:
            return self.transpose().dot(t)
        raise NotImplementedError("left-multiplication only for vectors")

    def matvec(self, x, out=None):
        return self.dot(x, out=out)

    def rmatvec(self, x):
        return self.T.dot(x)

    def multiply(self, other):
        """Scalar multiply only (reference csr.py:392-409)."""
        if isinstance(other, torch.Tensor) and other.ndim == 0:
            other = other.item()
        if not np.isscalar(other):
            raise NotImplementedError(
                "multiply supports scalars only (as in the reference)")
        return self._with_data(self._data * other)

    def __mul__(self, other):
        return self.multiply(other)

    __rmul__ = __mul__

    def _add_sparse(self, other: "csr_array", alpha=1.0) -> "csr_array":
        """C = self + alpha*other (same shape; partitions match by
        construction).  Local concat -> sort -> duplicate sum."""
        if self.shape != other.shape:
            raise ValueError(f"shape mismatch {self.shape} vs {other.shape}")
        dt = _common_dtype(self._data, other._data)
        dev = self._data.device
        lr = self._row_hi - self._row_lo
        r1 = torch.repeat_interleave(
            torch.arange(lr, device=dev),
            self._indptr[1:] - self._indptr[:-1])
        r2 = torch.repeat_interleave(
            torch.arange(lr, device=dev),
            other._indptr[1:] - other._indptr[:-1])
        row = torch.cat([r1, r2])
        col = torch.cat([self._indices.long(), other._indices.long()])
        val = torch.cat([self._data.to(dt), alpha * other._data.to(dt)])
        key = row * self._shape[1] + col
        key, order = torch.sort(key, stable=True)
        val = val[order]
        uniq, inverse = torch.unique_consecutive(key, return_inverse=True)
        out_val = torch.zeros(uniq.numel(), dtype=dt, device=dev)
        out_val.index_add_(0, inverse, val)
        out_row = torch.div(uniq, self._shape[1], rounding_mode="floor")
        out_col = uniq - out_row * self._shape[1]
        cnt = torch.bincount(out_row, minlength=lr)
        indptr = torch.zeros(lr + 1, dtype=torch.int64, device=dev)
        torch.cumsum(cnt, dim=0, out=indptr[1:])
        out = csr_array.__new__(csr_array)
        out._init_local(indptr, out_col, out_val.contiguous(), self._shape)
        return out

    def __add__(self, other):
        if isinstance(other, csr_array):
            return self._add_sparse(other, 1.0)
        if hasattr(other, "tocsr"):
            return self._add_sparse(csr_array(other), 1.0)
        if np.isscalar(other) and other == 0:
            return self.copy()
        return NotImplemented

    __radd__ = __add__

    def __sub__(self, other):
        if isinstance(other, csr_array):
            return self._add_sparse(other, -1.0)
        if hasattr(other, "tocsr"):
            return self._add_sparse(csr_array(other), -1.0)
        return NotImplemented

    def eliminate_zeros(self):
        """Drop explicitly stored zeros in place (scipy API)."""
        keep = self._data != 0
        dev = self._data.device
        lr = self._row_hi - self._row_lo
        row = torch.repeat_interleave(
            torch.arange(lr, device=dev),
            self._indptr[1:] - self._indptr[:-1])[keep]
        self._indices = self._indices[keep].contiguous()
        self._data = self._data[keep].contiguous()
        cnt = torch.bincount(row, minlength=lr)
        indptr = torch.zeros(lr + 1, dtype=torch.int64, device=dev)
        torch.cumsum(cnt, dim=0, out=indptr[1:])
        self._indptr = indptr
        self._global_nnz = None
        self._halo_cache = None
        self._ov_cache = None
        # row lengths shrank: stale cache would be a (safe) over-estimate
        # that can pin a less-unrolled SpMV tier
        self._max_nnz_cache = None
        self._struct_version += 1
        self._spgemm_cache = None
        self._affine_cache = "unset"
        return self

    def sum_duplicates(self):
        """No-op: construction keeps canonical form (scipy API)."""
        return self

    def diagonal(self, k: int = 0):
        """Main diagonal (k=0 only, reference csr.py:345-368); returns the
        LOCAL shard of the diagonal under partition(M)."""
        if k != 0:
            raise NotImplementedError("only the main diagonal (k=0)")
        d = ops.diagonal(self._indptr, self._indices, self._data,
                         self._row_hi - self._row_lo, self._row_lo)
        # scipy: the main diagonal has length min(M, N) — drop the rows
        # below the last diagonal entry (rectangular matrices)
        dmin = min(self._shape)
        keep = max(0, min(dmin, self._row_hi) - self._row_lo)
        if keep != d.numel():
            d = d[:keep].contiguous()
        if runtime.world_size > 1 and self._shape[0] != self._shape[1]:
            # vector convention: results are partition(len) shards.  The
            # row partition clipped to dmin is NOT partition(dmin) for
            # rectangular matrices — redistribute (diag is small; one
            # allgatherv of the clipped counts, then slice own shard)
            part_rows = self._part
            counts = [max(0, min(dmin, part_rows.hi(r))
                          - part_rows.lo(r))
                      for r in range(runtime.world_size)]
            full = comm.allgatherv(d, counts)
            lo, hi = runtime.local_range(dmin)
            d = full[lo:hi].contiguous()
        return lsarray.wrap(d, dmin)

    def todense(self, order=None, out: Optional[torch.Tensor] = None):
        """Dense LOCAL row block (full matrix at world_size == 1);
        reference csr.py:370-390 (same ``order``/``out`` contract:
        only C order, ``out`` is filled in place when given)."""
        if order is not None and str(order).upper() != "C":
            raise ValueError("order must be None or 'C'")
        dense = ops.csr_to_dense(self._indptr, self._indices, self._data,
                                 self._row_hi - self._row_lo, self._shape[1])
        if out is not None:
            if tuple(out.shape) != tuple(dense.shape):
                raise ValueError(
                    f"out shape {tuple(out.shape)} != {tuple(dense.shape)}")
            if isinstance(out, torch.Tensor):
                out.copy_(dense)
            else:
                out[...] = dense.cpu().numpy()
            return out
        return dense

    toarray = todense

    def sum(self, axis=None, dtype=None, out=None):
        """Reference base.py:111-171 contract: axis=None global scalar,
        axis=0/1 marginals (axis-1 via ones-matvec); ``dtype`` casts the
        accumulator, ``out`` receives the result in place."""
        tdt = to_torch_dtype(dtype) if dtype is not None else None
        if axis is None:
            if out is not None:
                raise ValueError("out= not supported for scalar sum")
            d = self._data.to(tdt) if tdt is not None else self._data
            s = d.sum().reshape(1)
            if runtime.world_size > 1:
                comm.allreduce_(s)
            return s[0]
        if axis in (1, -1):
            A = self if tdt is None or tdt == self._data.dtype else \
                self.astype(to_numpy_dtype(tdt))
            ones = torch.ones(A._shape[1], dtype=A._data.dtype,
                              device=A._data.device)
            y = out.reshape(-1) if isinstance(out, torch.Tensor) else None
            if y is not None and y.device != A._data.device:
                # the kernel writes through a raw pointer: an out on another
                # device (a host tensor for a GPU matrix) gets a copy
                y.copy_(ops.spmv(A._indptr, A._indices, A._data, ones))
                return out
            res = ops.spmv(A._indptr, A._indices, A._data, ones, y)
            return out if out is not None else res
        if axis == 0:
            d = self._data.to(tdt) if tdt is not None else self._data
            res = torch.zeros(self._shape[1], dtype=d.dtype,
                              device=d.device)
            res.scatter_add_(0, self._indices.long(), d)
            if runtime.world_size > 1:
                comm.allreduce_(res)
            if out is not None:
                out.copy_(res)
                return out
            return res
        raise ValueError("axis must be None, 0, or 1")

    def power(self, n, dtype=None):
        """Elementwise power of stored values (scipy csr.power; n > 0
        keeps the zero-preserving contract)."""
        if not np.isscalar(n):
            raise NotImplementedError("power expects a scalar exponent")
        d = self._data.to(to_torch_dtype(dtype)) if dtype is not None \
            else self._data
        return self._with_data(torch.pow(d, n))

    def trace(self, offset: int = 0):
        """Sum of the main diagonal (scipy API; offset 0 only, like
        ``diagonal``)."""
        d = self.diagonal(offset).as_subclass(torch.Tensor)
        s = d.sum().reshape(1)
        if runtime.world_size > 1:
            comm.allreduce_(s)
        return s[0]

    def mean(self, axis=None, dtype=None, out=None):
        """Mean over all entries or along an axis (zeros included,
        scipy semantics)."""
        M, N = self._shape
        if axis is None:
            return self.sum(dtype=dtype) / float(M * N)
        denom = float(N if axis in (1, -1) else M)
        res = self.sum(axis=axis, dtype=dtype, out=out)
        if out is not None:
            out /= denom
            return out
        return res / denom

    def __truediv__(self, other):
        if isinstance(other, torch.Tensor) and other.ndim == 0:
            other = other.item()
        if not np.isscalar(other):
            raise NotImplementedError("division by scalars only")
        return self._with_data(self._data / other)

    def transpose(self, axes=None, copy: bool = False) -> "csr_array":
        """Distributed transpose (reference csr.py:512-544 semantics):
        expand local rows to COO, all-to-allv entries to the new row owner
        (new row = old column), sort, assemble."""
        if axes is not None:
            raise ValueError("axes argument not supported")
        M, N = self._shape
        dev = self._data.device
        lr = self._row_hi - self._row_lo
        grow = torch.repeat_interleave(
            torch.arange(self._row_lo, self._row_hi, device=dev),
            self._indptr[1:] - self._indptr[:-1])
        col = self._indices.long()
        val = self._data
        newpart = runtime.partition(N)
        if runtime.world_size > 1:
            # route by COLUMN (the transposed row): reuse the row-owner
            # router with (col, grow) swapped
            col, grow, val = _route_to_row_owners(col, grow, val, newpart)
        # local assembly: new rows = col - new_lo
        new_lo = newpart.lo(runtime.rank)
        lrn = newpart.count(runtime.rank)
        indptr, ncol, val = _assemble_local_rows(
            col - new_lo, grow, val, lrn, M, dedup=False)
        out = csr_array.__new__(csr_array)
        out._init_local(indptr, ncol.to(_INDEX_DTYPE), val.contiguous(),
                        (N, M))
        return out

    @property
    def T(self) -> "csr_array":
        return self.transpose()

    def tocsr(self, copy: bool = False) -> "csr_array":
        return self.copy() if copy else self

    def getnnz(self, axis=None):
        if axis is None:
            return self.nnz
        if axis in (1, -1):
            return self._indptr[1:] - self._indptr[:-1]
        if axis == 0:
            out = torch.zeros(self._shape[1], dtype=torch.int64,
                              device=self._data.device)
            out.scatter_add_(0, self._indices.long(),
                             torch.ones_like(self._indices, dtype=torch.int64))
            if runtime.world_size > 1:
                comm.allreduce_(out)
            return out
        raise ValueError("axis must be None, 0, or 1")

    def count_nonzero(self) -> int:
        local = int((self._data != 0).sum())
        if runtime.world_size > 1:
            return int(comm.allgather_scalars(local).sum())
        return local

    def get_shape(self):
        return self._shape

    def tocoo(self):
        """Local COO triple (rows are GLOBAL row ids)."""
        dev = self._data.device
        grow = torch.repeat_interleave(
            torch.arange(self._row_lo, self._row_hi, device=dev),
            self._indptr[1:] - self._indptr[:-1])
        return grow, self._indices, self._data

    # -- misc -----------------------------------------------------------
    def __repr__(self):
        return (f"<legate_sparse.csr_array shape={self._shape} "
                f"nnz={self.nnz} dtype={self.dtype} "
                f"rows[{self._row_lo}:{self._row_hi}]>")

    def __str__(self):
        return self.__repr__()


csr_matrix = csr_array


# ---------------------------------------------------------------------------
# Free functions (reference csr.py:562-748)
# ---------------------------------------------------------------------------
def spmv(A: csr_array, x: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
    """y = A @ x into a preallocated local y (reference csr.py:562-593)."""
    xv = A._coerce_vec(x)
    if runtime.world_size > 1 and xv.numel() != A.shape[1]:
        return A._matvec_dist(xv, y.reshape(-1))
    x_win, col_off = A._gather_x(xv)
    aff = A._affine_plan() if A._data.is_cuda else None
    return ops.spmv(A._indptr, A._indices, A._data, x_win, y.reshape(-1),
                    col_offset=col_off, max_nnz=A._max_row_nnz(),
                    affine=aff, affine_const=A._affine_const(aff))


def spmm(A: csr_array, X, Y: torch.Tensor) -> torch.Tensor:
    """Y = A @ X into a preallocated local (local_rows, k) block Y."""
    return A.matmat(X, out=Y)


def _col_windows(A: csr_array):
    """All ranks' needed B-row windows [mn_r, mx_r) — the explicit
    analogue of the reference's FAST_IMAGE_RANGE pre-task
    (csr.py:606-617).  Collective (one int64 allgather each way)."""
    if A._indices.numel():
        mn = int(A._indices.min())
        mx = int(A._indices.max()) + 1
    else:
        mn = mx = 0
    mns = comm.allgather_scalars(mn).tolist()
    mxs = comm.allgather_scalars(mx).tolist()
    return mns, mxs


def _round_bounds(mns, mxs, k, K):
    """Round-k B-row range per destination rank: window split into K
    equal sub-windows, deterministic from the allgathered metadata (so
    every rank derives every pair's exchange without negotiation)."""
    out = []
    for d in range(len(mns)):
        W = mxs[d] - mns[d]
        out.append((mns[d] + (W * k) // K, mns[d] + (W * (k + 1)) // K))
    return out


def _issue_B_exchange(B: csr_array, bounds):
    """Post one round of the B-row exchange: every rank sends the slices
    of ITS OWN rows that each destination's round-range covers, async on
    the RCCL stream (reference semantics: MIN_MAX B-row images,
    csr.py:656-666).  Returns handles for _finish_B_exchange."""
    ws = runtime.world_size
    dev = B._data.device
    lo, hi = B._part.lo(runtime.rank), B._part.hi(runtime.rank)
    rank = runtime.rank
    clipped = []
    for (a, b) in bounds:
        a2, b2 = max(lo, int(a)), min(hi, int(b))
        if b2 < a2:
            a2 = b2 = lo
        clipped.append((a2, b2))
    # element offsets for all send ranges in one host transfer
    probe = torch.tensor([v - lo for ab in clipped for v in ab],
                         dtype=torch.int64, device=dev)
    el = B._indptr[probe].cpu().tolist()
    row_nnz_local = B._indptr[1:] - B._indptr[:-1]
    send_rn, send_ix, send_dv = [], [], []
    el_send = []
    for r, (a, b) in enumerate(clipped):
        s_el, e_el = el[2 * r], el[2 * r + 1]
        send_rn.append(row_nnz_local[a - lo:b - lo])
        send_ix.append(B._indices[s_el:e_el])
        send_dv.append(B._data[s_el:e_el])
        el_send.append(e_el - s_el)
    # deterministic row-count splits; element splits need one tiny
    # alltoall (the receiver cannot know senders' nnz structure)
    a_k, b_k = bounds[rank]
    rn_out = [max(0, min(B._part.hi(s), b_k) - max(B._part.lo(s), a_k))
              for s in range(ws)]
    el_t = torch.tensor(el_send, dtype=torch.int64, device=dev)
    el_recv = torch.empty_like(el_t)
    import torch.distributed as dist
    dist.all_to_all_single(el_recv, el_t)
    el_out = [int(x) for x in el_recv.cpu()]
    rn_buf, w1 = comm.alltoallv_single_async(
        torch.cat(send_rn) if send_rn else B._indptr[:0],
        [t.numel() for t in send_rn], rn_out)
    ix_buf, w2 = comm.alltoallv_single_async(
        torch.cat(send_ix) if send_ix else B._indices[:0],
        el_send, el_out)
    dv_buf, w3 = comm.alltoallv_single_async(
        torch.cat(send_dv) if send_dv else B._data[:0],
        el_send, el_out)
    return {"rn": rn_buf, "ix": ix_buf, "dv": dv_buf,
            "works": (w1, w2, w3), "range": (a_k, b_k), "dev": dev}


def _finish_B_exchange(h):
    """Wait for a posted round and assemble the received window CSR."""
    for w in h["works"]:
        if w is not None:
            w.wait()
    a_k, b_k = h["range"]
    n_win = b_k - a_k
    Bw_indptr = torch.zeros(n_win + 1, dtype=torch.int64, device=h["dev"])
    if n_win:
        assert h["rn"].numel() == n_win, (h["rn"].numel(), a_k, b_k)
        torch.cumsum(h["rn"], dim=0, out=Bw_indptr[1:])
    return Bw_indptr, h["ix"], h["dv"], a_k


def _gather_B_window(A: csr_array, B: csr_array, windows=None):
    """Single-shot gather of the whole B-row window each rank needs.
    Returns (Bw_indptr, Bw_indices, Bw_vals, row_offset): kernels index
    the windowed indptr through an offset base pointer."""
    if runtime.world_size == 1:
        return B._indptr, B._indices, B._data, 0
    mns, mxs = windows if windows is not None else _col_windows(A)
    h = _issue_B_exchange(B, list(zip(mns, mxs)))
    return _finish_B_exchange(h)


def _split_A_by_col(A: csr_array, edges):
    """Split A's local rows into len(edges)-1 column-range pieces
    (indptr/indices/vals per piece) for the chunked SpGEMM: piece k holds
    the entries whose column falls in [edges[k], edges[k+1])."""
    dev = A._data.device
    lr = A._indptr.numel() - 1
    row_of = torch.repeat_interleave(
        torch.arange(lr, device=dev), A._indptr[1:] - A._indptr[:-1])
    col = A._indices.long()
    pieces = []
    for k in range(len(edges) - 1):
        m = (col >= edges[k]) & (col < edges[k + 1])
        cnt = torch.bincount(row_of[m], minlength=lr)
        ip = torch.zeros(lr + 1, dtype=torch.int64, device=dev)
        torch.cumsum(cnt, dim=0, out=ip[1:])
        pieces.append((ip, A._indices[m].contiguous(),
                       A._data[m].contiguous()))
    return pieces


def _merge_partial_C(partials, lr, N, dev, dt, idt):
    """Sum K partial products C = sum_k A_k @ B_k (sparse COO concat +
    sort + duplicate-sum)."""
    if len(partials) == 1:
        return partials[0]
    rows, cols, vals = [], [], []
    for (ip, ix, dv) in partials:
        if ix.numel() == 0:
            continue
        rows.append(torch.repeat_interleave(
            torch.arange(lr, device=dev), ip[1:] - ip[:-1]))
        cols.append(ix.long())
        vals.append(dv)
    if not rows:
        return (torch.zeros(lr + 1, dtype=torch.int64, device=dev),
                torch.empty(0, dtype=idt, device=dev),
                torch.empty(0, dtype=dt, device=dev))
    row = torch.cat(rows)
    col = torch.cat(cols)
    val = torch.cat(vals)
    ip, col, val = _assemble_local_rows(row, col, val, lr, N, dedup=True)
    return ip, col.to(idt), val.contiguous()


def spgemm_csr_csr_csr(A: csr_array, B: csr_array) -> csr_array:
    """C = A @ B, distributed (reference csr.py:598-748).

    Local Gustavson (hash-table HIP kernel on GPU, OpenMP on CPU) over
    this rank's A rows; B rows arrive by collective, windowed to
    [min_col(A), max_col(A)) per rank (the reference's FAST_IMAGE_RANGE +
    MIN_MAX images).  When the window payload exceeds
    LS_SPGEMM_CHUNK_MB, the gather runs in K bounded ROUNDS and round
    k+1's all-to-allv is posted before round k's local Gustavson runs —
    comm/compute overlap with bounded peak memory (window chunk + partial
    outputs), instead of materializing a window that approaches the whole
    of B at R-MAT scale.  No global pos assembly is needed — C's indptr
    stays local by construction, which replaces the reference's NCCL nnz
    all-gather + exclusive scan (spgemm_csr_csr_csr.cu:43-62)."""
    if A.shape[1] != B.shape[0]:
        raise ValueError(
            f"dimension mismatch {A.shape} @ {B.shape}")
    from .settings import settings as _settings

    dt = _common_dtype(A._data, B._data)
    if A._data.dtype != dt:
        A = A.astype(to_numpy_dtype(dt))
    if B._data.dtype != dt:
        B = B.astype(to_numpy_dtype(dt))
    ws = runtime.world_size
    M, N = A.shape[0], B.shape[1]

    def _single_shot(windows=None):
        B_indptr, B_indices, B_data, b_off = _gather_B_window(A, B, windows)
        cache = A._spgemm_cache_for(B)
        if A._data.is_cuda:
            # stencil-convolution path on the gathered window: the
            # window plan is structure-only, so it rides the cache
            planB = cache.get("aff_planB", "unset")
            if planB == "unset":
                planB = (B._affine_plan() if runtime.world_size == 1
                         else _build_affine_plan(B_indptr, B_indices,
                                                 max(B.shape) + b_off))
                cache["aff_planB"] = planB

            def _general_rows(rows):
                ip = A._indptr
                cnts = ip[rows + 1] - ip[rows]
                sub_ip = torch.zeros(rows.numel() + 1, dtype=torch.int64,
                                     device=ip.device)
                torch.cumsum(cnts, dim=0, out=sub_ip[1:])
                tot = int(sub_ip[-1])
                ent = (torch.repeat_interleave(ip[rows], cnts)
                       + torch.arange(tot, device=ip.device)
                       - torch.repeat_interleave(sub_ip[:-1], cnts))
                return ops.spgemm_local(
                    sub_ip, A._indices[ent].contiguous(),
                    A._data[ent].contiguous(), B_indptr, B_indices,
                    B_data, N, b_row_offset=b_off)
            res = ops.spgemm_affine_try(
                A._indptr, A._data, A._affine_plan(),
                B_indptr, B_data, planB,
                B_indptr.numel() - 1, N, _general_rows,
                _index_dtype_for((M, N)), cache=cache,
                b_row_off=b_off)
            if res is not None:
                return res
        A_indices = A._indices
        if A_indices.dtype != B_indices.dtype:
            A_indices = A_indices.to(torch.int64)
            B_indices = B_indices.to(torch.int64)
        return ops.spgemm_local(
            A._indptr, A_indices, A._data, B_indptr, B_indices, B_data,
            N, b_row_offset=b_off, cache=cache)

    if ws == 1:
        C_indptr, C_indices, C_vals = _single_shot()
    else:
        mns, mxs = _col_windows(A)
        # decide the round count K from the LARGEST rank window so every
        # rank derives the same K from the same allgathered metadata
        force_rows = _settings.spgemm_chunk_rows
        chunk_mb = _settings.spgemm_chunk_mb
        max_win = max((mx - mn) for mn, mx in zip(mns, mxs))
        if force_rows > 0:
            K = max(1, -(-max_win // force_rows))
        elif chunk_mb > 0 and max_win > 0:
            bnnz_local = B._data.numel()
            total_bnnz = int(comm.allgather_scalars(bnnz_local).sum())
            bytes_per_row = (total_bnnz / max(B.shape[0], 1)) * (
                B._data.element_size() + B._indices.element_size()) + 8
            K = max(1, int(max_win * bytes_per_row //
                           (chunk_mb * 1024 * 1024)))
        else:
            K = 1
        if K <= 1:
            C_indptr, C_indices, C_vals = _single_shot((mns, mxs))
        else:
            rank = runtime.rank
            my_edges = [mns[rank] + ((mxs[rank] - mns[rank]) * k) // K
                        for k in range(K + 1)]
            A_pieces = _split_A_by_col(A, my_edges)
            lr = A._indptr.numel() - 1
            partials = []
            pending = _issue_B_exchange(B, _round_bounds(mns, mxs, 0, K))
            for k in range(K):
                nxt = None
                if k + 1 < K:
                    # post round k+1 BEFORE computing round k: the RCCL
                    # exchange proceeds on the comm stream while the
                    # Gustavson kernels run
                    nxt = _issue_B_exchange(
                        B, _round_bounds(mns, mxs, k + 1, K))
                Bw_ip, Bw_ix, Bw_dv, b_off = _finish_B_exchange(pending)
                ipA, ixA, dvA = A_pieces[k]
                if ixA.numel():
                    if ixA.dtype != Bw_ix.dtype:
                        ixA = ixA.to(torch.int64)
                        Bw_ix = Bw_ix.to(torch.int64)
                    partials.append(ops.spgemm_local(
                        ipA, ixA, dvA, Bw_ip, Bw_ix, Bw_dv, N,
                        b_row_offset=b_off))
                pending = nxt
            C_indptr, C_indices, C_vals = _merge_partial_C(
                partials, lr, N, A._data.device, dt,
                _index_dtype_for((M, N)))
    out = csr_array.__new__(csr_array)
    out._init_local(C_indptr, C_indices, C_vals, (M, N))
    return out

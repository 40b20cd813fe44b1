# SPDX-License-Identifier: Apache-2.0
"""Iterative solvers: CG, GMRES, BiCGSTAB, LOBPCG, LinearOperator; the
sparse triangular solve and the ILU(0) preconditioner; the
FSAI preconditioner.

Counterpart of the reference's ``legate_sparse/linalg.py`` (linalg.py:85-668).
The key property preserved is the *async solver pipeline* (SURVEY §3.4):

- ``cg_axpby`` consumes its scalars as 1-element DEVICE tensors; the
  division a/b happens inside the fused HIP kernel (reference axpby.cu:25-47)
  so no ``.item()`` ever occurs in the iteration body.
- Scalar reductions (rho, pq) are local block-reduce + RCCL all-reduce of a
  single element, left on device.
- Convergence is tested only every ``conv_test_iters`` iterations
  (reference linalg.py:529-533) — the only host syncs in the loop.

All vectors are LOCAL shards of partition(n) in SPMD mode.
"""
from __future__ import annotations

from typing import Callable, Optional

import numpy as np
import torch

from . import comm, ops
from .base import as_torch_1d
from .lsarray import lsarray
from .runtime import runtime
from .types import to_numpy_dtype, to_torch_dtype


def _wrap_result(t: torch.Tensor, n_global: int):
    """Tag a solver result with its global length so user code can mix it
    with replicated global arrays (see lsarray.py)."""
    return lsarray.wrap(t, n_global)


def _check_rhs_shape(b, n: int):
    """Reference contract (linalg.py:479, 593): b must be (n,) or (n, 1)."""
    shp = getattr(b, "shape", None)
    if shp is not None and len(shp) not in (1, 2):
        raise ValueError(f"b must be 1-D or a column vector, got shape {shp}")
    if shp is not None and len(shp) == 2 and shp[1] != 1:
        raise ValueError(f"b must be (n,) or (n, 1), got shape {shp}")


def _get_atol_rtol(b_norm: float, tol=None, atol=0.0, rtol=1e-5):
    """Legacy-tol resolution (reference linalg.py:454-462): ``tol``
    overrides ``rtol``; ``atol=None`` means "use rtol"; the effective
    absolute tolerance is ``max(atol, rtol*||b||)``."""
    rtol = float(tol) if tol is not None else rtol
    if atol is None:
        atol = rtol
    atol = max(float(atol), float(rtol) * float(b_norm))
    return atol, rtol


def _to_local_vec(v, n_global: int, dtype, device) -> torch.Tensor:
    """Accept a global (replicated) or local-shard vector; return the
    local shard."""
    t = as_torch_1d(v, device=device).to(to_torch_dtype(dtype))
    if isinstance(t, torch.Tensor) and type(t) is not torch.Tensor:
        t = t.as_subclass(torch.Tensor)  # strip lsarray wrapper inside solvers
    part = runtime.partition(n_global)
    lo, hi = part.lo(runtime.rank), part.hi(runtime.rank)
    if t.numel() == n_global and n_global != (hi - lo):
        return t[lo:hi].contiguous()
    if t.numel() == (hi - lo):
        return t.contiguous()
    if t.numel() == n_global:
        return t.contiguous()
    raise ValueError(
        f"vector length {t.numel()} matches neither global {n_global} nor "
        f"local shard {hi - lo}")


def _gdot(x: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
    """Global <x, y> as a 1-element device tensor."""
    s = ops.vdot(x, y, conj=True)
    if runtime.world_size > 1:
        comm.allreduce_(s)
    return s


def _gnorm(x: torch.Tensor) -> torch.Tensor:
    s = _gdot(x, x)
    return torch.sqrt(torch.abs(s))


# ---------------------------------------------------------------------------
# LinearOperator family (reference linalg.py:85-414)
# ---------------------------------------------------------------------------
class LinearOperator:
    def __init__(self, shape, matvec=None, rmatvec=None, dtype=None):
        if matvec is not None:
            # scipy-style factory usage
            self.shape = tuple(int(s) for s in shape)
            self.dtype = np.dtype(dtype) if dtype is not None else None
            self._matvec_fn = matvec
            self._rmatvec_fn = rmatvec
        else:
            self.shape = tuple(int(s) for s in shape)
            self.dtype = np.dtype(dtype) if dtype is not None else None
            self._matvec_fn = None
            self._rmatvec_fn = None

    def matvec(self, x, out=None):
        if self._matvec_fn is None:
            raise NotImplementedError
        y = self._matvec_fn(x)
        if out is not None:
            out.copy_(y if isinstance(y, torch.Tensor) else torch.as_tensor(y))
            return out
        return y

    def rmatvec(self, x, out=None):
        if self._rmatvec_fn is None:
            raise NotImplementedError
        y = self._rmatvec_fn(x)
        if out is not None:
            out.copy_(y if isinstance(y, torch.Tensor) else torch.as_tensor(y))
            return out
        return y

    def _apply_columns(self, fn, X, n_out):
        """Generic block product: ``fn`` column by column, stacked."""
        if getattr(X, "ndim", None) != 2:
            raise ValueError("expected a 2-D block of column vectors")
        is_t = isinstance(X, torch.Tensor)
        k = int(X.shape[1])
        if k == 0:
            return (X.new_empty((n_out, 0)) if is_t
                    else np.empty((n_out, 0), dtype=X.dtype))
        cols = []
        for j in range(k):
            xj = X[:, j].contiguous() if is_t \
                else np.ascontiguousarray(X[:, j])
            cols.append(fn(xj))
        if all(isinstance(c, torch.Tensor) for c in cols):
            return torch.stack([c.reshape(-1) for c in cols], dim=1)
        return np.stack([np.asarray(c).reshape(-1) for c in cols], axis=1)

    def matmat(self, X):
        """``A @ X`` for a 2-D block X (scipy's LinearOperator.matmat);
        subclasses with a native block product override this."""
        return self._apply_columns(self.matvec, X, self.shape[0])

    def rmatmat(self, X):
        """``A^H @ X`` for a 2-D block X."""
        return self._apply_columns(self.rmatvec, X, self.shape[1])

    def __matmul__(self, x):
        return self.matvec(x)

    def dot(self, x):
        return self.matvec(x)


class IdentityOperator(LinearOperator):
    def __init__(self, shape, dtype=None):
        super().__init__(shape, dtype=dtype)

    def matvec(self, x, out=None):
        if out is not None:
            out.copy_(x)
            return out
        return x.clone() if isinstance(x, torch.Tensor) else x

    rmatvec = matvec

    def matmat(self, X):
        if getattr(X, "ndim", None) != 2:
            raise ValueError("expected a 2-D block of column vectors")
        return X.clone() if isinstance(X, torch.Tensor) \
            else np.array(X, copy=True)

    rmatmat = matmat


class _SparseMatrixLinearOperator(LinearOperator):
    """Wraps a csr_array; caches A.conj().T for rmatvec
    (reference linalg.py:375-387)."""

    def __init__(self, A):
        self.A = A
        self._AH = None
        super().__init__(A.shape, dtype=A.dtype)

    def matvec(self, x, out=None):
        return self.A.dot(x, out=out)

    def rmatvec(self, x, out=None):
        if self._AH is None:
            self._AH = self.A.conj().transpose()
        return self._AH.dot(x, out=out)

    def matmat(self, X):
        return self.A.matmat(X)

    def rmatmat(self, X):
        if self._AH is None:
            self._AH = self.A.conj().transpose()
        return self._AH.matmat(X)


def aslinearoperator(A):
    if isinstance(A, LinearOperator):
        return A
    if hasattr(A, "format"):
        return _SparseMatrixLinearOperator(A if A.format == "csr"
                                           else A.tocsr())
    raise TypeError(f"cannot wrap {type(A)} as LinearOperator")


# reference linalg.py:417-431 exposes make_linear_operator; scipy calls
# the same thing aslinearoperator — provide both names.
make_linear_operator = aslinearoperator


def norm(A, ord="fro"):
    """Matrix norm of a sparse array: 'fro', 1 (max column abs sum), or
    inf (max row abs sum) — scipy.sparse.linalg.norm-compatible subset."""
    import math as _math

    if not hasattr(A, "indptr"):
        raise TypeError("norm expects a sparse array")
    data = A.data
    absd = data.abs()
    if ord in ("fro", None):
        s = (absd * absd).sum().reshape(1)
        if runtime.world_size > 1:
            comm.allreduce_(s)
        return float(torch.sqrt(s))
    if ord == 1:
        col = torch.zeros(A.shape[1], dtype=absd.dtype, device=absd.device)
        col.scatter_add_(0, A.indices.long(), absd)
        if runtime.world_size > 1:
            comm.allreduce_(col)
        return float(col.max()) if col.numel() else 0.0
    if ord in (np.inf, float("inf"), "inf"):
        row = torch.zeros(A.indptr.numel() - 1, dtype=absd.dtype,
                          device=absd.device)
        ids = torch.repeat_interleave(
            torch.arange(row.numel(), device=absd.device),
            A.indptr[1:] - A.indptr[:-1])
        row.scatter_add_(0, ids, absd)
        m = row.max().reshape(1) if row.numel() else torch.zeros(
            1, dtype=absd.dtype, device=absd.device)
        if runtime.world_size > 1:
            comm.allreduce_(m, op="max")
        return float(m)
    raise NotImplementedError(f"norm ord={ord!r} not supported")


# ---------------------------------------------------------------------------
# Fused CG update (reference linalg.py:433-451 + axpby.cu)
# ---------------------------------------------------------------------------
def cg_axpby(y: torch.Tensor, x: torch.Tensor, a: torch.Tensor,
             b: torch.Tensor, isalpha: bool, negate: bool = False):
    """y = (±a/b)·x + y  (isalpha) or y = x + (±a/b)·y  — a, b are
    1-element device tensors consumed inside the kernel."""
    return ops.axpby(y, x, a, b, isalpha, negate)


# ---------------------------------------------------------------------------
# CG (reference linalg.py:465-535, CuPy-derived)
# ---------------------------------------------------------------------------
from .coverage import track_provenance


@track_provenance
def cg(A, b, x0=None, tol=None, maxiter: Optional[int] = None, M=None,
       callback: Optional[Callable] = None, atol: float = 0.0,
       rtol: float = 1e-5, conv_test_iters: int = 25):
    """Conjugate gradient.  Returns ``(x, iters)`` — the solution (local
    shard in SPMD mode) and the iteration count, matching the reference
    contract (reference linalg.py:465-535 returns (x, iters); legacy
    ``tol=`` is accepted as an alias for ``rtol`` via _get_atol_rtol)."""
    Aop = aslinearoperator(A)
    n = Aop.shape[0]
    _check_rhs_shape(b, n)
    dtype = Aop.dtype if Aop.dtype is not None else np.float64
    device = runtime.device
    b = _to_local_vec(b, n, dtype, device)
    if maxiter is None:
        maxiter = n * 10
    Mop = aslinearoperator(M) if M is not None and not isinstance(
        M, LinearOperator) else (M or IdentityOperator(Aop.shape,
                                                       dtype=dtype))

    bnrm2 = _gnorm(b)
    # b = 0: the exact solution is x = 0; entering the loop would divide
    # 0/0 in the fused axpby (scipy returns immediately too).  One host
    # sync before the loop, not inside it.
    if float(bnrm2.item()) == 0.0:
        return _wrap_result(torch.zeros_like(b), n), 0
    rtol_eff = float(tol) if tol is not None else float(rtol)
    atol_eff = rtol_eff if atol is None else float(atol)
    # atol_t = max(atol, rtol*||b||) as a device scalar (_get_atol_rtol
    # semantics without forcing a host sync on bnrm2)
    atol_t = torch.clamp(bnrm2 * rtol_eff, min=atol_eff)

    if x0 is None:
        x = torch.zeros_like(b)
        r = b.clone()
    else:
        x = _to_local_vec(x0, n, dtype, device).clone()
        r = b - Aop.matvec(x)

    # Unpreconditioned CG aliases z = r (saves two full vector passes
    # per iteration vs copying through an identity preconditioner).
    ident_M = isinstance(Mop, IdentityOperator)
    if ident_M:
        z = r
    else:
        z = Mop.matvec(r)
        if not isinstance(z, torch.Tensor):
            z = torch.as_tensor(z, device=device)
        if z.data_ptr() == r.data_ptr():
            z = z.clone()
    p = z.clone()
    q = torch.empty_like(b)
    rho = _gdot(r, z)
    iters = 0

    import os as _os
    # ---- fused unpreconditioned iteration (real dtypes) --------------
    # 4 launches per iteration: SpMV, p·q dot, cg_fused
    # (alpha in-kernel; x += alpha p; r -= alpha q; rho' = ||r||^2 in the
    # SAME pass — z = r so the next rho IS the residual norm), and the
    # beta axpby.  Zero host syncs except the amortized convergence test.
    use_fused = ident_M and not b.is_complex()
    graph = None
    if use_fused:
        rho_buf = rho.clone()
        pq_buf = torch.zeros_like(rho_buf)
        rho_new = torch.zeros_like(rho_buf)
        atol_sq = (atol_t * atol_t).to(rho_buf.dtype)
        ws = runtime.world_size
        # matvec+dot fusion: when A is our CSR with an affine plan, the
        # p.(A p) reduction rides inside the SpMV kernel (no extra pass)
        A_csr = Aop.A if hasattr(Aop, "A") and hasattr(
            getattr(Aop, "A"), "_matvec_pq") else None

        def _one_iter():
            if A_csr is None or not A_csr._matvec_pq(p, q, pq_buf):
                Aop.matvec(p, out=q)
                ops.vdot(p, q, out=pq_buf)
            if ws > 1:
                comm.allreduce_(pq_buf)
            ops.cg_fused(x, r, p, q, rho_buf, pq_buf, rho_new)
            if ws > 1:
                comm.allreduce_(rho_new)
            # beta = rho_new / rho ; p = r + beta p
            cg_axpby(p, r, rho_new, rho_buf, isalpha=False, negate=False)
            rho_buf.copy_(rho_new)

        # hipGraph capture: fixed 5-kernel sequence on stable buffers —
        # removes per-iteration launch/Python overhead.  Measured: clear
        # win below ~2M rows (launch-bound); at 16.7M rows kernels
        # dominate and the one-time capture cost (~15 ms) is pure
        # overhead for short solves — gate by size (LS_CG_GRAPH=1
        # forces, 0 disables; benchmarks/cg_fused_ab.py evidence).
        _graph_env = _os.environ.get("LS_CG_GRAPH", "auto")
        _graph_on = (_graph_env == "1"
                     or (_graph_env == "auto" and b.numel() <= 2 ** 21))
        if (callback is None and runtime.world_size == 1
                and device.type == "cuda" and maxiter > 8 and _graph_on):
            try:
                # warmup replays are REAL iterations (side-stream per
                # torch graph-capture protocol)
                side = torch.cuda.Stream()
                side.wait_stream(torch.cuda.current_stream())
                with torch.cuda.stream(side):
                    for _ in range(3):
                        _one_iter()
                        iters += 1
                torch.cuda.current_stream().wait_stream(side)
                graph = torch.cuda.CUDAGraph()
                with torch.cuda.graph(graph):
                    _one_iter()  # recorded, NOT executed (stream capture)
            except Exception:
                graph = None  # fall back to the eager loop

        step = conv_test_iters if conv_test_iters > 0 else maxiter
        while iters < maxiter:
            if graph is not None:
                n_rep = min(step - (iters % step) if iters % step else
                            step, maxiter - iters)
                for _ in range(n_rep):
                    graph.replay()
                iters += n_rep
            else:
                _one_iter()
                iters += 1
                if callback is not None:
                    callback(x)
                if conv_test_iters <= 0 or not (
                        iters % conv_test_iters == 0 or iters == maxiter):
                    continue
            # amortized host sync: rho_new IS ||r||^2 — no extra pass
            if bool((rho_new <= atol_sq).item()):
                break
        return _wrap_result(x, n), iters

    while iters < maxiter:
        Aop.matvec(p, out=q)
        pq = _gdot(p, q)
        # alpha = rho / pq ; x += alpha p ; r -= alpha q — all in-kernel
        cg_axpby(x, p, rho, pq, isalpha=True, negate=False)
        cg_axpby(r, q, rho, pq, isalpha=True, negate=True)
        iters += 1
        if callback is not None:
            callback(x)
        if conv_test_iters > 0 and (iters % conv_test_iters == 0
                                    or iters == maxiter):
            rnorm = _gnorm(r)  # host sync point (deliberate, amortized)
            if bool((rnorm <= atol_t).item()):
                break
        if not ident_M:
            z = Mop.matvec(r, out=z if isinstance(z, torch.Tensor)
                           else None)
            if not isinstance(z, torch.Tensor):
                z = torch.as_tensor(z, device=device)
        rho1 = rho
        rho = _gdot(r, z)
        # beta = rho / rho1 ; p = z + beta p
        cg_axpby(p, z, rho, rho1, isalpha=False, negate=False)

    return _wrap_result(x, n), iters


# ---------------------------------------------------------------------------
# GMRES (reference linalg.py:540-668, restarted, host lstsq)
# ---------------------------------------------------------------------------
@track_provenance
def gmres(A, b, x0=None, tol=None, restart: Optional[int] = None,
          maxiter: Optional[int] = None, M=None,
          callback: Optional[Callable] = None, restrt: Optional[int] = None,
          atol: float = 0.0, callback_type: Optional[str] = None,
          rtol: float = 1e-5, reorthogonalize: bool = False):
    """Restarted GMRES, right-preconditioned (reference linalg.py:540-668,
    CuPy-derived): solves A·M y = b and returns x = M y.

    Async-pipeline design (the CG analogue of SURVEY §3.4): the Arnoldi
    inner loop performs ZERO host syncs — the Hessenberg matrix H is built
    column-by-column ON DEVICE (batched Gram-Schmidt dot + one allreduce
    per column), the new basis vector is normalized by a device scalar,
    and H is transferred to the host once per restart for the small lstsq
    (the reference also solves lstsq on host, linalg.py:658-661).

    ``reorthogonalize=True`` adds a second Gram-Schmidt pass per column
    (classical GS twice) for ill-conditioned systems — still sync-free.

    Returns (x, info): info=0 converged, else the iteration count.
    """
    Aop = aslinearoperator(A)
    n = Aop.shape[0]
    _check_rhs_shape(b, n)
    if restrt is not None:
        if restart is not None:
            raise ValueError("cannot specify both restart and restrt")
        restart = restrt
    if callback_type is None:
        callback_type = "pr_norm"
    if callback_type not in ("x", "pr_norm"):
        raise ValueError(f"Unknown callback_type: {callback_type}")
    dtype = Aop.dtype if Aop.dtype is not None else np.float64
    device = runtime.device
    b = _to_local_vec(b, n, dtype, device)
    if maxiter is None:
        maxiter = min(n, 1000)
    if restart is None:
        restart = min(20, n)
    restart = min(restart, maxiter)
    Mop = M if isinstance(M, LinearOperator) else (
        aslinearoperator(M) if M is not None
        else IdentityOperator(Aop.shape, dtype=dtype))
    ident_M = isinstance(Mop, IdentityOperator)

    bnrm2 = float(_gnorm(b).item())
    eff_atol, _ = _get_atol_rtol(bnrm2, tol, atol, rtol)
    if bnrm2 == 0.0:
        return _wrap_result(b.clone(), n), 0

    if x0 is None:
        x = torch.zeros_like(b)
    else:
        x = _to_local_vec(x0, n, dtype, device).clone()

    cdtype = to_torch_dtype(dtype)
    tiny = torch.tensor(
        np.finfo(np.dtype(dtype).char.lower() if np.dtype(dtype).kind == "c"
                 else np.dtype(dtype)).tiny,
        dtype=to_torch_dtype(np.float64), device=device)

    def _apply_M(v):
        out = Mop.matvec(v)
        if not isinstance(out, torch.Tensor):
            out = torch.as_tensor(out, device=device)
        return out.reshape(-1).to(cdtype)

    iters = 0
    while True:
        # right preconditioning: residual of the TRUE system at M(y)
        mx = x if ident_M else _apply_M(x)
        r = b - Aop.matvec(mx).reshape(-1)
        beta_t = _gnorm(r)                      # device scalar
        beta = float(beta_t.item())             # 1 sync per restart
        if callback is not None:
            if callback_type == "x":
                callback(mx)
            elif callback_type == "pr_norm" and iters > 0:
                callback(beta / bnrm2)
        if beta <= eff_atol or iters >= maxiter:
            break
        m = min(restart, maxiter - iters)
        V = torch.zeros(m + 1, r.numel(), dtype=cdtype, device=device)
        H = torch.zeros(m + 1, m, dtype=cdtype, device=device)
        V[0] = r / beta_t
        for j in range(m):
            z = V[j] if ident_M else _apply_M(V[j])
            w = Aop.matvec(z)
            if not isinstance(w, torch.Tensor):
                w = torch.as_tensor(w, device=device)
            w = w.reshape(-1).to(cdtype)
            # classical Gram-Schmidt: one batched dot + one allreduce.
            # Shapes matter on GPU: a (j+1, n) @ (n, 1) GEMM with huge k
            # and tiny m parallelizes terribly in BLAS (single tile);
            # vecdot reduces each basis row with a proper two-stage
            # reduction, and the projection update uses the (n, j+1)
            # orientation that GEMV handles at bandwidth.
            basis = V[:j + 1]
            hcol = ops.gs_dots(V, j + 1, w)
            if runtime.world_size > 1:
                comm.allreduce_(hcol)
            # u -= V h (reference compute_hu: no conjugation on h here;
            # the conj lives in the dot, vecdot(V, w) = conj(V).w)
            w = w - (hcol.reshape(1, -1) @ basis).reshape(-1)
            if reorthogonalize:
                h2 = ops.gs_dots(V, j + 1, w)
                if runtime.world_size > 1:
                    comm.allreduce_(h2)
                w = w - (h2.reshape(1, -1) @ basis).reshape(-1)
                hcol = hcol + h2
            hnorm = _gnorm(w)                   # device scalar, no sync
            H[: j + 1, j] = hcol
            H[j + 1, j] = hnorm.to(cdtype)
            # guarded normalize: breakdown (hnorm ~ 0) yields a zero
            # vector and a zero H column instead of inf/nan — lstsq
            # handles the rank deficiency; still no host sync.
            safe = torch.where(hnorm > tiny.to(hnorm.dtype), hnorm,
                               torch.ones_like(hnorm))
            V[j + 1] = torch.where(hnorm > tiny.to(hnorm.dtype),
                                   w / safe.to(cdtype),
                                   torch.zeros_like(w))
            iters += 1
        # one H transfer per restart (not per column)
        Hh = H[: m + 1, : m].cpu().numpy()
        e1 = np.zeros(m + 1, dtype=Hh.dtype)
        e1[0] = beta
        ym, *_ = np.linalg.lstsq(Hh, e1, rcond=None)
        yt = torch.from_numpy(np.ascontiguousarray(ym)).to(
            device=device, dtype=cdtype)
        x = x + (yt.reshape(1, -1) @ V[:m]).reshape(-1)
    info = 0 if beta <= eff_atol else iters
    return _wrap_result(mx, n), info


# ---------------------------------------------------------------------------
# BiCGSTAB (docs/DESIGN.md §15): short recurrence for nonsymmetric systems
# ---------------------------------------------------------------------------
@track_provenance
def bicgstab(A, b, x0=None, tol=None, maxiter: Optional[int] = None, M=None,
             callback: Optional[Callable] = None, atol: float = 0.0,
             rtol: float = 1e-5, conv_test_iters: int = 25):
    """BiCGSTAB for general square systems (scipy.sparse.linalg.bicgstab
    contract).  Seven vectors, two operator applications per iteration, no
    restart.  ``M`` approximates the inverse of A and is applied as scipy
    applies it: ``phat = M p``, ``shat = M s``.

    The iteration never reads the host: alpha, omega and beta are formed
    inside the fused kernels from 1-element device tensors with a guarded
    division (x/0 := 0), so an iteration that runs on after r reached zero
    between two convergence tests is a no-op.  At world size > 1 there are
    exactly three all-reduces per iteration (rhv, [ts, tt], [rho, rr]) and
    every loop-ending decision is taken from all-reduced values.

    Returns ``(x, info)``: 0 converged; -10 rho or <rhat, v> broke down;
    -11 omega broke down or a scalar is not finite; ``maxiter`` when the
    iteration limit was reached.  Convergence and breakdown are tested
    every ``conv_test_iters`` iterations and at ``maxiter``.
    """
    Aop = aslinearoperator(A)
    if Aop.shape[0] != Aop.shape[1]:
        raise ValueError(f"expected a square operator, got {Aop.shape}")
    n = Aop.shape[0]
    _check_rhs_shape(b, n)
    dtype = Aop.dtype if Aop.dtype is not None else np.float64
    device = runtime.device
    b = _to_local_vec(b, n, dtype, device)
    if maxiter is None:
        maxiter = n * 10
    Mop = M if isinstance(M, LinearOperator) else (
        aslinearoperator(M) if M is not None
        else IdentityOperator(Aop.shape, dtype=dtype))
    ident_M = isinstance(Mop, IdentityOperator)

    bnrm2 = float(_gnorm(b).item())
    if bnrm2 == 0.0:
        return _wrap_result(torch.zeros_like(b), n), 0
    eff_atol, _ = _get_atol_rtol(bnrm2, tol, atol, rtol)

    if x0 is None:
        x = torch.zeros_like(b)
        r = b.clone()
    else:
        x = _to_local_vec(x0, n, dtype, device).clone()
        r = b - Aop.matvec(x).reshape(-1)

    # ---- all buffers before the loop ---------------------------------
    rhat = r.clone()
    p = r.clone()
    v = torch.empty_like(b)
    s = torch.empty_like(b)
    t = torch.empty_like(b)
    # unpreconditioned: phat IS p and shat IS s (no copies)
    phat = p if ident_M else torch.empty_like(b)
    shat = s if ident_M else torch.empty_like(b)
    rr0 = _gdot(r, r)                      # rho_0 = <rhat, r0> = ||r0||^2
    # two [rho, ||r||^2] pairs that swap roles every iteration, each kept
    # with the 1-element view of its rho
    pair = torch.cat([rr0, rr0])
    cur = (pair, pair[0:1])
    pair = torch.zeros_like(pair)
    nxt = (pair, pair[0:1])
    rhv = torch.zeros_like(rr0)            # <rhat, v>
    tst = torch.zeros_like(pair)           # [<t, s>, <t, t>]
    ts, tt = tst[0:1], tst[1:2]
    ws = runtime.world_size

    def _status():
        """One host read of the (all-reduced) scalars -> info or None."""
        h = torch.cat([cur[0], rhv, tst]).cpu().numpy()
        rho_h, rr_h, rhv_h, ts_h = h[0], h[1], h[2], h[3]
        if np.sqrt(np.abs(rr_h)) <= eff_atol:
            return 0
        if rho_h == 0 or rhv_h == 0:
            return -10
        if ts_h == 0 or not np.all(np.isfinite(h)):
            return -11
        return None

    if float(torch.sqrt(torch.abs(rr0)).item()) <= eff_atol:
        return _wrap_result(x, n), 0

    step = conv_test_iters if conv_test_iters > 0 else maxiter
    iters = 0
    info = maxiter
    while iters < maxiter:
        rho, out2 = cur[1], nxt[0]
        if iters > 0:
            ops.bicgstab_p(p, r, v, rho, rhv, ts, tt)
        if not ident_M:
            Mop.matvec(p, out=phat)
        Aop.matvec(phat, out=v)
        ops.vdot(rhat, v, out=rhv)
        if ws > 1:
            comm.allreduce_(rhv)
        ops.bicgstab_s(s, r, v, rho, rhv)
        if not ident_M:
            Mop.matvec(s, out=shat)
        Aop.matvec(shat, out=t)
        ops.vdot2(t, s, tst)
        if ws > 1:
            comm.allreduce_(tst)
        ops.bicgstab_xr(x, r, phat, shat, s, t, rhat, rho, rhv, ts, tt, out2)
        if ws > 1:
            comm.allreduce_(out2)
        cur, nxt = nxt, cur
        iters += 1
        if callback is not None:
            callback(x)
        if iters % step == 0 or iters == maxiter:
            st = _status()
            if st is not None:
                info = st
                break
    return _wrap_result(x, n), info


# ---------------------------------------------------------------------------
# LOBPCG (docs/DESIGN.md §16): block eigensolver on SpMM + block kernels
# ---------------------------------------------------------------------------
def _plain_block(y, device, dt) -> torch.Tensor:
    """Result of a user or library ``matmat`` -> plain 2-D device tensor."""
    if not isinstance(y, torch.Tensor):
        y = torch.from_numpy(np.ascontiguousarray(np.asarray(y)))
    if type(y) is not torch.Tensor:
        y = y.as_subclass(torch.Tensor)
    return y.to(device=device, dtype=dt)


def _chol_inv(G: np.ndarray):
    """Inverse upper Cholesky factor of a Hermitian Gram matrix, after
    scaling it to unit diagonal: ``G = R^H R`` -> ``R^{-1}``, so that
    ``V R^{-1}`` is orthonormal.  None when G is not numerically positive
    definite."""
    import scipy.linalg as sla
    G = (G + G.conj().T) / 2
    d = np.real(np.diag(G))
    if not np.all(np.isfinite(G)) or np.any(d <= 0):
        return None
    s = 1.0 / np.sqrt(d)
    try:
        Rf = np.linalg.cholesky(G * s[:, None] * s[None, :]).conj().T
        Ri = sla.solve_triangular(Rf, np.eye(G.shape[0], dtype=G.dtype))
    except (np.linalg.LinAlgError, sla.LinAlgError):
        return None
    Ri = s[:, None] * Ri
    return Ri if np.all(np.isfinite(Ri)) else None


@track_provenance
def lobpcg(A, X, B=None, M=None, Y=None, tol=None, maxiter=None,
           largest=True, verbosityLevel=0, retLambdaHistory=False,
           retResidualNormsHistory=False, restartControl=20,
           _block_impl="hip"):
    """Locally optimal block preconditioned conjugate gradient
    (scipy.sparse.linalg.lobpcg signature) for the k extremal eigenpairs of
    a symmetric/Hermitian ``A``.

    ``A`` (a csr_array or LinearOperator) and the optional preconditioner
    ``M`` are applied only through ``aslinearoperator(.).matmat``; with a
    csr_array the one operator application per iteration is one SpMM on the
    active columns.  ``X`` is the (n, k) initial block, global or this
    rank's (shard, k) rows.  ``B`` and ``Y`` are not implemented.  Unlike
    scipy there is no dense fallback for small problems: ``n < 3k`` raises.

    All passes over (n, k) blocks run in the block kernels
    (``ops.block_gram / block_update / block_residual``); the small dense
    algebra (Cholesky factors, the <= 3k x 3k Rayleigh-Ritz problem) runs
    on the host in double precision.  That costs three small device-to-host
    reads per iteration (k norms; the Cholesky Grams; the Gram panels) and
    the coefficient matrices going back.  Every decision (convergence,
    active set, restart, breakdown) is taken from all-reduced values, so
    all ranks branch alike.

    Returns ``(w, V)`` — w a host numpy array of k eigenvalues ordered as
    scipy orders them (descending for ``largest=True``, ascending
    otherwise), V this rank's (local_rows, k) block — followed by the
    eigenvalue and residual-norm histories when requested.  Exhausting
    ``maxiter`` (default 20) warns and returns the best block seen.
    """
    import warnings
    import scipy.linalg as sla

    if B is not None:
        raise NotImplementedError("lobpcg: generalized problems (B) are "
                                  "not implemented")
    if Y is not None:
        raise NotImplementedError("lobpcg: constraints (Y) are not "
                                  "implemented")
    if _block_impl not in ("hip", "torch"):
        raise ValueError("_block_impl is 'hip' or 'torch'")
    Aop = aslinearoperator(A)
    if Aop.shape[0] != Aop.shape[1]:
        raise ValueError(f"expected a square operator, got {Aop.shape}")
    n = Aop.shape[0]
    device = runtime.device
    Xin = X if isinstance(X, torch.Tensor) else torch.from_numpy(
        np.ascontiguousarray(np.asarray(X)))
    if type(Xin) is not torch.Tensor:
        Xin = Xin.as_subclass(torch.Tensor)
    if Xin.ndim != 2:
        raise ValueError("lobpcg: X must be a 2-D (n, k) block")
    k = int(Xin.shape[1])
    if k < 1 or k > ops.BLOCK_KMAX:
        raise ValueError(f"lobpcg: block size k = {k} is outside "
                         f"[1, {ops.BLOCK_KMAX}]")
    if n < 3 * k:
        raise ValueError(f"lobpcg: n = {n} is below 3k = {3 * k}; use a "
                         "dense eigensolver for a problem this small")
    xdt = Xin.dtype if (Xin.dtype.is_floating_point
                        or Xin.dtype.is_complex) else torch.float64
    dt = xdt if Aop.dtype is None else torch.promote_types(
        to_torch_dtype(Aop.dtype), xdt)
    if dt not in (torch.float32, torch.float64, torch.complex64,
                  torch.complex128):
        raise NotImplementedError(f"lobpcg: unsupported dtype {dt}")
    rdt = ops._real_dtype(dt)
    hdt = np.complex128 if dt.is_complex else np.float64
    part = runtime.partition(n)
    lo, hi = part.lo(runtime.rank), part.hi(runtime.rank)
    ln = hi - lo
    if Xin.shape[0] == n and ln != n:
        Xin = Xin[lo:hi]
    elif Xin.shape[0] != ln:
        raise ValueError(f"X row count {Xin.shape[0]} is neither global "
                         f"({n}) nor the local shard ({ln})")
    Mop = None if M is None else aslinearoperator(M)
    if tol is None:
        tol = float(np.sqrt(np.finfo(to_numpy_dtype(rdt)).eps)) * n
    tol = float(tol)
    if maxiter is None:
        maxiter = 20
    ws = runtime.world_size

    if _block_impl == "hip":
        gram_fn, update_fn, resid_fn = (ops.block_gram, ops.block_update,
                                        ops.block_residual)
    else:
        def gram_fn(Xb, Yb, out=None):
            return ops._block_gram_torch(Xb, Yb, True, out)
        update_fn = ops._block_update_torch
        resid_fn = ops._block_residual_torch

    def new_block():
        return torch.empty((ln, k), dtype=dt, device=device)

    def panel(buf, m):
        """The first m columns' worth of a (ln, k) buffer as a CONTIGUOUS
        (ln, m) block (matmat wants contiguous operands)."""
        return buf if m == k else buf.reshape(-1)[:ln * m].view(ln, m)

    def to_dev(Ch):
        return torch.from_numpy(np.ascontiguousarray(Ch)).to(
            device=device, dtype=dt)

    # one flat device buffer takes every small Gram of an iteration, so
    # they are all-reduced and read with one call each
    gbuf = torch.empty(12 * k * k, dtype=dt, device=device)

    def grams(pairs):
        """Host (double) copies of Xb^H Yb for each pair: one all-reduce,
        one device-to-host read."""
        off = 0
        views = []
        for Xb, Yb in pairs:
            p, q = int(Xb.shape[1]), int(Yb.shape[1])
            g = gbuf[off:off + p * q].view(p, q)
            gram_fn(Xb, Yb, out=g)
            views.append((off, p, q))
            off += p * q
        if ws > 1:
            comm.allreduce_(gbuf[:off])
        h = gbuf[:off].cpu().numpy().astype(hdt)
        return [h[o:o + p * q].reshape(p, q) for o, p, q in views]

    def apply_A(Wb, out):
        if isinstance(Aop, _SparseMatrixLinearOperator) \
                and np.dtype(Aop.A.dtype) == to_numpy_dtype(dt):
            Aop.A.matmat(Wb, out=out)      # SpMM straight into our buffer
            return out
        y = _plain_block(Aop.matmat(Wb), device, dt)
        if tuple(y.shape) != tuple(Wb.shape):
            raise ValueError(f"A.matmat changed the block shape "
                             f"{tuple(Wb.shape)} to {tuple(y.shape)}")
        out.copy_(y)
        return out

    def pick(lam):
        order = np.argsort(lam)
        return order[::-1][:k] if largest else order[:k]

    # ---- buffers: everything (n, k) is allocated here ------------------
    Xs = [new_block(), new_block(), new_block()]   # current / best / spare
    AXs = [new_block(), new_block(), new_block()]
    Rb, Wbuf, AWbuf = new_block(), new_block(), new_block()
    Pb, APb, Pa_buf, APa_buf = (new_block(), new_block(), new_block(),
                                new_block())
    theta = torch.empty(k, dtype=rdt, device=device)
    nrm = torch.empty(k, dtype=rdt, device=device)
    cur = 0
    Xs[0].copy_(Xin.to(device=device, dtype=dt))

    # ---- orthonormalize X, initial Rayleigh-Ritz -----------------------
    (G,) = grams([(Xs[0], Xs[0])])
    Ri = _chol_inv(G)
    if Ri is None:
        raise ValueError("lobpcg: the initial block X is rank deficient")
    update_fn(Xs[0], [(Xs[0], to_dev(Ri))], False)
    apply_A(Xs[0], AXs[0])
    (H,) = grams([(Xs[0], AXs[0])])
    lam, Q = np.linalg.eigh((H + H.conj().T) / 2)
    ii = pick(lam)
    lam = lam[ii]
    Qd = to_dev(Q[:, ii])
    update_fn(Xs[0], [(Xs[0], Qd)], False)
    update_fn(AXs[0], [(AXs[0], Qd)], False)

    lam_hist = [lam.copy()]
    res_hist = []
    active = np.ones(k, dtype=bool)
    have_P = False
    best = 0
    smallest = np.inf
    it = 0
    failed = False
    while True:
        Xc, AXc = Xs[cur], AXs[cur]
        theta.copy_(torch.from_numpy(lam.astype(np.float64)))
        resid_fn(Rb, AXc, Xc, theta, nrm)
        if ws > 1:
            comm.allreduce_(nrm)
        norms = np.sqrt(np.abs(nrm.cpu().numpy().astype(np.float64)))
        res_hist.append(norms.copy())
        mean_norm = float(norms.sum()) / k
        forced = False
        if mean_norm < smallest:
            smallest = mean_norm
            best = cur
        elif mean_norm > 2.0 ** restartControl * smallest:
            forced = True
            apply_A(Xc, AXc)
        active &= norms > tol
        na = int(active.sum())
        if verbosityLevel:
            print(f"iteration {it}: block size {na}, eigenvalues {lam}, "
                  f"residual norms {norms}")
        if na == 0 or it >= maxiter:
            break
        act = np.nonzero(active)[0]

        # ---- W = M R[:, active], projected against X, orthonormalized --
        if na == k:
            Wa = Rb
        else:
            Sel = np.zeros((k, na), dtype=hdt)
            Sel[act, np.arange(na)] = 1
            Wa = update_fn(panel(Wbuf, na), [(Rb, to_dev(Sel))], False)
        if Mop is not None:
            Wm = _plain_block(Mop.matmat(Wa), device, dt)
            Wa = panel(Wbuf, na)
            Wa.copy_(Wm)
        gxw = gbuf[:k * na].view(k, na)
        gram_fn(Xc, Wa, out=gxw)
        if ws > 1:
            comm.allreduce_(gxw)
        update_fn(Wa, [(Xc, -gxw)], True)           # no host read
        restart = forced or not have_P
        pairs = [(Wa, Wa)] + ([] if restart else [(Pb, Pb)])
        gs = grams(pairs)
        Ri = _chol_inv(gs[0])
        if Ri is None:
            failed = True
            break
        update_fn(Wa, [(Wa, to_dev(Ri))], False)
        AWa = apply_A(Wa, panel(AWbuf, na))
        if not restart:
            Rp = _chol_inv(gs[1][np.ix_(act, act)])
            if Rp is None:
                restart = True
            else:
                # P[:, active] R^{-1} without a gather: the factor sits in
                # the active rows of a (k, na) matrix
                E = np.zeros((k, na), dtype=hdt)
                E[act, :] = Rp
                Ed = to_dev(E)
                Pa = update_fn(panel(Pa_buf, na) if na < k else Pb,
                               [(Pb, Ed)], False)
                APa = update_fn(panel(APa_buf, na) if na < k else APb,
                                [(APb, Ed)], False)

        # ---- Rayleigh-Ritz on [X W P] ----------------------------------
        C = None
        while C is None:
            S = [Xc, Wa] + ([] if restart else [Pa])
            AS = [AXc, AWa] + ([] if restart else [APa])
            nb = len(S)
            idx = [(i, j) for i in range(nb) for j in range(i, nb)]
            gs = grams([(S[i], AS[j]) for i, j in idx]
                       + [(S[i], S[j]) for i, j in idx])
            sizes = [int(b.shape[1]) for b in S]
            offs = np.concatenate([[0], np.cumsum(sizes)])
            m = int(offs[-1])
            gA = np.zeros((m, m), dtype=hdt)
            gB = np.zeros((m, m), dtype=hdt)
            for t, (i, j) in enumerate(idx):
                for gM, blk in ((gA, gs[t]), (gB, gs[len(idx) + t])):
                    gM[offs[i]:offs[i + 1], offs[j]:offs[j + 1]] = blk
                    if i != j:
                        gM[offs[j]:offs[j + 1], offs[i]:offs[i + 1]] = \
                            blk.conj().T
            gA = (gA + gA.conj().T) / 2
            gB = (gB + gB.conj().T) / 2
            try:
                if not (np.all(np.isfinite(gA)) and np.all(np.isfinite(gB))):
                    raise np.linalg.LinAlgError("non-finite Gram matrix")
                lam_all, vec = sla.eigh(gA, gB, check_finite=False)
                ii = pick(lam_all)
                C = vec[:, ii]
                new_lam = lam_all[ii]
                if not np.all(np.isfinite(C)):
                    raise np.linalg.LinAlgError("non-finite Ritz vectors")
            except (np.linalg.LinAlgError, sla.LinAlgError):
                C = None
                if restart:
                    failed = True
                    break
                restart = True       # drop P for this iteration
        if failed:
            break
        lam = new_lam
        Cx, Cw = to_dev(C[:k]), to_dev(C[k:k + na])
        # the next X goes to the buffer that is neither current nor best
        nxt = next(i for i in range(3) if i != cur and i != best)
        if restart:
            update_fn(Xs[nxt], [(Xc, Cx), (Wa, Cw)], False)
            update_fn(AXs[nxt], [(AXc, Cx), (AWa, Cw)], False)
            update_fn(Pb, [(Wa, Cw)], False)
            update_fn(APb, [(AWa, Cw)], False)
        else:
            Cp = to_dev(C[k + na:])
            update_fn(Xs[nxt], [(Xc, Cx), (Wa, Cw), (Pa, Cp)], False)
            update_fn(AXs[nxt], [(AXc, Cx), (AWa, Cw), (APa, Cp)], False)
            update_fn(Pb, [(Wa, Cw), (Pa, Cp)], False)
            update_fn(APb, [(AWa, Cw), (APa, Cp)], False)
        have_P = True
        cur = nxt
        it += 1
        lam_hist.append(lam.copy())

    # ---- post-processing: exact A X and a final Rayleigh-Ritz ----------
    # (the loop leaves through its convergence test, so the last residual
    # entry belongs to Xs[cur]; the best block is the one returned)
    Xf, AXf = Xs[best], AXs[best]
    apply_A(Xf, AXf)
    gs = grams([(Xf, AXf), (Xf, Xf)])
    try:
        lam, Q = sla.eigh((gs[0] + gs[0].conj().T) / 2,
                          (gs[1] + gs[1].conj().T) / 2, check_finite=False)
    except (np.linalg.LinAlgError, sla.LinAlgError) as e:
        raise ValueError("lobpcg: the final Rayleigh-Ritz failed") from e
    ii = pick(lam)
    lam = lam[ii]
    Qd = to_dev(Q[:, ii])
    update_fn(Xf, [(Xf, Qd)], False)
    update_fn(AXf, [(AXf, Qd)], False)
    theta.copy_(torch.from_numpy(lam.astype(np.float64)))
    resid_fn(Rb, AXf, Xf, theta, nrm)
    if ws > 1:
        comm.allreduce_(nrm)
    norms = np.sqrt(np.abs(nrm.cpu().numpy().astype(np.float64)))
    lam_hist.append(lam.copy())
    res_hist.append(norms.copy())
    if failed or norms.max() > tol:
        warnings.warn(
            f"lobpcg exited at iteration {it} with residual norms {norms} "
            f"not reaching the requested tolerance {tol}"
            + (" (the Rayleigh-Ritz problem broke down)" if failed else ""),
            UserWarning, stacklevel=2)
    if verbosityLevel:
        print(f"final eigenvalues {lam}, residual norms {norms}")

    out = [lam.astype(np.float64), lsarray.wrap(Xf, n)]
    if retLambdaHistory:
        out.append(lam_hist)
    if retResidualNormsHistory:
        out.append(res_hist)
    return tuple(out)


# ---------------------------------------------------------------------------
# Sparse triangular solve and ILU(0) (docs/DESIGN.md §17)
# ---------------------------------------------------------------------------
def _plain(t: torch.Tensor) -> torch.Tensor:
    return t if type(t) is torch.Tensor else t.as_subclass(torch.Tensor)


def _tri_analysis(A, lower: bool, unit_diagonal: bool) -> dict:
    """Per-structure analysis for ``spsolve_triangular``, cached on the
    matrix by (structure version, lower, unit_diagonal): diagonal
    positions, the wrong-side and missing-diagonal checks (index
    arithmetic, one host read) and the level schedule."""
    key = (A._struct_version, bool(lower), bool(unit_diagonal))
    cache = getattr(A, "_tri_cache", None)
    if cache is None or cache.get("version") != A._struct_version:
        cache = {"version": A._struct_version}
        A._tri_cache = cache
    if key not in cache:
        n = A.shape[0]
        indptr, indices = A._indptr, A._indices
        dpos, has = ops.diag_positions(indptr, indices, n)
        if lower:
            wrong = indptr[1:] - dpos - has.long()
        else:
            wrong = dpos - indptr[:-1]
        checks = torch.stack([(wrong > 0).any(), (~has).any()]).cpu().tolist()
        entry = {"dpos": dpos, "wrong_side": bool(checks[0]),
                 "missing_diag": bool(checks[1]), "sched": None}
        if not entry["wrong_side"]:
            entry["sched"] = ops.level_schedule(indptr, indices, n, lower)
        cache[key] = entry
    return cache[key]


def spsolve_triangular(A, b, lower: bool = True, overwrite_A: bool = False,
                       overwrite_b: bool = False,
                       unit_diagonal: bool = False):
    """Solve ``A x = b`` for a sparse triangular ``A``
    (scipy.sparse.linalg.spsolve_triangular's signature and semantics).

    ``A`` is a square csr_array (or anything ``csr_array(...)`` accepts),
    ``b`` is ``(n,)`` or ``(n, k)``, numpy or a torch tensor.  The result
    has ``b``'s shape and the common dtype.  With ``unit_diagonal`` the
    stored diagonal entries are ignored.  ``overwrite_b`` solves in place
    when ``b`` is a row-major tensor of the result's dtype on the runtime
    device; ``overwrite_A`` is accepted and has no effect (A is never
    modified).  Any k: the level-scheduled kernels take up to 32 columns a
    pass and wider blocks go in panels.

    Raises ``ValueError`` for a non-square A, a shape mismatch or stored
    entries on the wrong side of the diagonal, ``numpy.linalg.LinAlgError``
    when ``unit_diagonal`` is false and a diagonal entry is missing or
    zero, and ``NotImplementedError`` at world size above 1.
    """
    from .csr import csr_array

    if runtime.world_size > 1:
        raise NotImplementedError(
            "spsolve_triangular runs at world size 1 only: a distributed "
            "triangular solve is a pipeline across ranks (every rank waits "
            "for the rows of the ranks before it), which is not implemented")
    if not isinstance(A, csr_array):
        A = csr_array(A)
    n = A.shape[0]
    if A.shape[0] != A.shape[1]:
        raise ValueError(f"A must be square, got shape {A.shape}")
    is_t = isinstance(b, torch.Tensor)
    bt = _plain(b) if is_t else torch.from_numpy(np.asarray(b))
    if bt.ndim not in (1, 2) or int(bt.shape[0]) != n:
        raise ValueError(f"b has shape {tuple(bt.shape)}, incompatible with "
                         f"A of shape {A.shape}")
    device = A._data.device
    bdt = bt.dtype if (bt.dtype.is_floating_point or bt.dtype.is_complex) \
        else torch.float64
    dt = torch.promote_types(A._data.dtype, bdt)
    if dt not in (torch.float32, torch.float64, torch.complex64,
                  torch.complex128):
        raise NotImplementedError(f"spsolve_triangular: dtype {dt}")
    info = _tri_analysis(A, lower, unit_diagonal)
    if info["wrong_side"]:
        raise ValueError(
            f"A is not {'lower' if lower else 'upper'} triangular: it stores "
            f"entries {'above' if lower else 'below'} the diagonal")
    vals = A._data if A._data.dtype == dt else A._data.to(dt)
    if not unit_diagonal:
        if info["missing_diag"] or (n and bool(
                (vals[info["dpos"]] == 0).any())):
            raise np.linalg.LinAlgError(
                "A is singular: a diagonal entry is missing or zero")
    B2 = bt.reshape(n, 1) if bt.ndim == 1 else bt
    k = int(B2.shape[1])
    reuse = (overwrite_b and is_t and bt.dtype == dt and bt.device == device
             and (bt.ndim == 1 and bt.is_contiguous()
                  or bt.ndim == 2 and (n <= 1 or k == 0 or (
                      B2.stride(1) == 1 and B2.stride(0) >= k))))
    if reuse:
        X = B2
    else:
        X = torch.empty((n, k), dtype=dt, device=device)
        X.copy_(B2)
    for c0 in range(0, k, ops.SPTRSV_KMAX):
        ops.sptrsv(A._indptr, A._indices, vals, info["dpos"], info["sched"],
                   X[:, c0:c0 + ops.SPTRSV_KMAX], lower=lower,
                   unit_diagonal=unit_diagonal)
    out = X.reshape(n) if bt.ndim == 1 else X
    return _wrap_result(out, n)


class ILU0(LinearOperator):
    """Incomplete LU factorisation on A's own sparsity pattern, as a
    preconditioner: ``matvec(r)`` applies ``U^-1 L^-1`` with two
    level-scheduled sweeps over ONE combined factor (strict lower part L
    with an implied unit diagonal, the rest U).

    ``(L U - A)`` is zero on the pattern of A.  For a symmetric positive
    definite A with a symmetric pattern the factors satisfy ``U = D L^T``,
    so the operator ``U^-1 L^-1`` is symmetric (and positive definite where
    the pivots stay positive): it is a valid ``M`` for ``cg`` and
    ``lobpcg`` as well as for ``gmres`` and ``bicgstab``.

    At world size W the preconditioner is block-Jacobi: every rank factors
    the diagonal block of its own rows (entries whose column belongs to
    another rank are dropped for the factorisation only) and applies it to
    its own shard with no communication.

    After construction ``matvec`` and ``matmat`` read nothing back from the
    device and allocate only their output: the sweeps run in place on it.
    """

    def __init__(self, A, _impl: str = "native"):
        from .csr import csr_array

        if not isinstance(A, csr_array):
            A = csr_array(A)
        if A.shape[0] != A.shape[1]:
            raise ValueError(f"ilu0 needs a square matrix, got {A.shape}")
        super().__init__(A.shape, dtype=A.dtype)
        self._impl = _impl
        n = A.shape[0]
        self._lo, self._hi = A._row_lo, A._row_hi
        ln = self._hi - self._lo
        indptr, indices = A._indptr, A._indices
        dev = indptr.device
        self._src = (indptr, indices)
        if runtime.world_size > 1:
            col = indices.long()
            keep = (col >= self._lo) & (col < self._hi)
            row_of = torch.repeat_interleave(
                torch.arange(ln, device=dev), indptr[1:] - indptr[:-1])
            cnt = torch.bincount(row_of[keep], minlength=ln)
            indptr = torch.cat([torch.zeros(1, dtype=torch.int64, device=dev),
                                torch.cumsum(cnt, 0)])
            indices = (col[keep] - self._lo).to(indices.dtype).contiguous()
            self._sel = torch.nonzero(keep).reshape(-1)
        else:
            self._sel = None
        self._indptr, self._indices = indptr, indices
        dpos, has = ops.diag_positions(indptr, indices, ln)
        missing = (~has).any().to(torch.int64).reshape(1)
        if runtime.world_size > 1:
            comm.allreduce_(missing, op="max")
        if bool(missing.item()):
            raise ValueError("ilu0 needs every diagonal entry of A stored")
        self._dpos = dpos
        self._sched_l = ops.level_schedule(indptr, indices, ln, True)
        self._sched_u = ops.level_schedule(indptr, indices, ln, False)
        self._max_row = int((indptr[1:] - indptr[:-1]).max()) if ln else 0
        self._flag = torch.empty(1, dtype=torch.int32, device=dev)
        self._F = None
        self._factor(A._data)

    # -- factorisation ----------------------------------------------------
    def _factor(self, data: torch.Tensor) -> None:
        F = data.clone() if self._sel is None else data[self._sel]
        ops.ilu0_factor(self._indptr, self._indices, F, self._dpos,
                        self._sched_l, self._flag, self._max_row,
                        _impl=self._impl)
        # the one host read: smallest local row with a bad pivot
        bad = int(self._flag.item())
        n = self.shape[0]
        row = torch.tensor([self._lo + bad if bad < self._hi - self._lo
                            else n], dtype=torch.int64,
                           device=runtime.device)
        if runtime.world_size > 1:
            comm.allreduce_(row, op="min")
        row = int(row.item())
        if row < n:
            raise RuntimeError(f"ilu0: zero or non-finite pivot in row {row}")
        self._F = F

    def refactor(self, A2) -> "ILU0":
        """New values on the SAME sparsity pattern: the level analysis and
        every index array are reused.  ``ValueError`` for another
        pattern."""
        same = (tuple(A2.shape) == self.shape
                and getattr(A2, "format", None) == "csr"
                and hasattr(A2, "_indptr"))
        if same:
            ip, ix = self._src
            same = (A2._indptr is ip and A2._indices is ix) or (
                A2._indptr.shape == ip.shape and A2._indices.shape == ix.shape
                and torch.equal(A2._indptr, ip)
                and torch.equal(A2._indices.long(), ix.long()))
        if runtime.world_size > 1:
            flag = torch.tensor([0 if same else 1], dtype=torch.int64,
                                device=runtime.device)
            comm.allreduce_(flag, op="max")
            same = not bool(flag.item())
        if not same:
            raise ValueError("refactor needs a csr_array with the sparsity "
                             "pattern of the factored matrix")
        data = A2._data
        want = to_torch_dtype(self.dtype)
        self._factor(data if data.dtype == want else data.to(want))
        return self

    # -- apply --------------------------------------------------------------
    @property
    def levels(self):
        """(levels of the L sweep, levels of the U sweep)."""
        return self._sched_l.n_levels, self._sched_u.n_levels

    @property
    def launches_per_apply(self) -> int:
        """Kernel launches of one ``matvec`` after chaining."""
        return self._sched_l.n_launches() + self._sched_u.n_launches()

    def _sweeps(self, X: torch.Tensor) -> None:
        for sched, lower in ((self._sched_l, True), (self._sched_u, False)):
            ops.sptrsv(self._indptr, self._indices, self._F, self._dpos,
                       sched, X, lower=lower, unit_diagonal=lower,
                       _impl=self._impl)

    def matvec(self, r, out=None):
        x = _to_local_vec(r, self.shape[0], self.dtype, self._F.device)
        if out is None:
            out = torch.empty_like(x)
        else:
            out = _plain(out)
            if out.shape != x.shape or out.dtype != x.dtype \
                    or not out.is_contiguous():
                raise ValueError("ilu0.matvec: out must be a contiguous "
                                 "vector of the operator's dtype")
        if out.data_ptr() != x.data_ptr():
            out.copy_(x)
        self._sweeps(out.view(-1, 1))
        return out

    def solve(self, r):
        """``U^-1 L^-1 r`` (scipy's ``spilu(...).solve``)."""
        return _wrap_result(self.matvec(r), self.shape[0])

    def matmat(self, R):
        """``U^-1 L^-1 R`` for an (n, k) block, the factor streamed once
        per panel of at most 32 columns."""
        if getattr(R, "ndim", None) != 2:
            raise ValueError("expected a 2-D block of column vectors")
        Rt = _plain(R) if isinstance(R, torch.Tensor) else torch.from_numpy(
            np.ascontiguousarray(np.asarray(R)))
        n, ln = self.shape[0], self._hi - self._lo
        if Rt.shape[0] == n and ln != n:
            Rt = Rt[self._lo:self._hi]
        elif Rt.shape[0] != ln:
            raise ValueError(f"block row count {Rt.shape[0]} is neither "
                             f"global ({n}) nor the local shard ({ln})")
        k = int(Rt.shape[1])
        out = torch.empty((ln, k), dtype=self._F.dtype, device=self._F.device)
        out.copy_(Rt)
        for c0 in range(0, k, ops.SPTRSV_KMAX):
            self._sweeps(out[:, c0:c0 + ops.SPTRSV_KMAX])
        return out

    def rmatvec(self, x, out=None):
        raise NotImplementedError("ilu0: rmatvec is not implemented")

    def rmatmat(self, X):
        raise NotImplementedError("ilu0: rmatmat is not implemented")

    # -- inspection ---------------------------------------------------------
    def factor_local(self):
        """This rank's combined factor as ``(indptr, indices, values)`` of
        its diagonal block (local column numbers)."""
        return self._indptr, self._indices, self._F

    def _split(self):
        import scipy.sparse as sp
        from .csr import csr_array

        if runtime.world_size > 1:
            raise NotImplementedError(
                "L and U are per-rank diagonal blocks at world size above "
                "1; read them with factor_local()")
        S = sp.csr_matrix((self._F.cpu().numpy(), self._indices.cpu().numpy(),
                           self._indptr.cpu().numpy()), shape=self.shape)
        L = sp.tril(S, -1, format="csr") + sp.identity(
            self.shape[0], dtype=S.dtype, format="csr")
        return csr_array(L.tocsr()), csr_array(sp.triu(S, 0, format="csr"))

    @property
    def L(self):
        """Unit lower factor with its ones stored (built on the host: for
        inspection and tests, not on the apply path)."""
        return self._split()[0]

    @property
    def U(self):
        """Upper factor with its diagonal."""
        return self._split()[1]


def ilu0(A) -> ILU0:
    """ILU(0) of a square csr_array whose every diagonal entry is stored,
    as a ``LinearOperator`` any solver here takes as ``M=``::

        M = linalg.ilu0(A); x, info = linalg.bicgstab(A, b, M=M)

    ``ValueError`` for a missing diagonal entry (before any kernel runs),
    ``RuntimeError`` naming the global row for a zero or non-finite pivot.
    See :class:`ILU0`."""
    return ILU0(A)


# ---------------------------------------------------------------------------
# Factorised sparse approximate inverse (docs/DESIGN.md §18)
# ---------------------------------------------------------------------------
def _row_ids(indptr: torch.Tensor, lo: int) -> torch.Tensor:
    """Global row number of every stored entry of a local CSR."""
    n = int(indptr.numel()) - 1
    return torch.repeat_interleave(
        torch.arange(lo, lo + n, device=indptr.device),
        indptr[1:] - indptr[:-1])


def _lower_triangle(indptr, indices, lo):
    """(indptr, indices) of the entries with ``col <= row``."""
    n = int(indptr.numel()) - 1
    row = _row_ids(indptr, lo)
    keep = indices.long() <= row
    cnt = torch.bincount(row[keep] - lo, minlength=n)
    ip = torch.zeros(n + 1, dtype=torch.int64, device=indptr.device)
    torch.cumsum(cnt, 0, out=ip[1:])
    return ip, indices[keep].contiguous()


def _canonical_csr(A):
    """``A`` itself when its rows are sorted and duplicate-free, else a copy
    with the duplicates summed."""
    from .csr import _assemble_local_rows, csr_array

    if A.has_canonical_format:
        return A
    ip, ix, dv = _assemble_local_rows(
        _row_ids(A._indptr, 0), A._indices.long(), A._data,
        A._row_hi - A._row_lo, A.shape[1], dedup=True)
    Ac = csr_array.__new__(csr_array)
    Ac._init_local(ip, ix, dv.contiguous(), A.shape)
    return Ac


class FSAI(LinearOperator):
    """Factorised sparse approximate inverse preconditioner
    (Kolotilina-Yeremin) of a Hermitian positive definite ``A = L L^H``: a
    sparse lower-triangular ``G ~ L^-1`` on a prescribed pattern, applied as
    ``M = G^H G`` with two sparse matrix-vector products.

    Row i of G on its pattern ``P_i`` (sorted, last entry i) is the last
    row of ``C^-1`` where ``A[P_i, P_i] = C C^H``: ``diag(G A G^H) = 1``,
    G's diagonal is real and positive, and with the full lower-triangular
    pattern ``G = inv(cholesky(A))``.  Only the entries of A with
    ``col <= row`` are read; the upper triangle is never touched.

    ``G`` and ``GH`` are ordinary distributed csr_arrays, so the apply is
    exact at every world size.  After construction ``matvec`` and ``matmat``
    read nothing back from the device.  A pattern row holds at most
    ``FSAI_MAX_ROW`` = 32 entries.
    """

    def __init__(self, A, pattern=None, _impl: str = "native"):
        from .csr import csr_array

        if not isinstance(A, csr_array):
            A = csr_array(A)
        n = A.shape[0]
        if A.shape[0] != A.shape[1]:
            raise ValueError(f"fsai needs a square matrix, got {A.shape}")
        super().__init__(A.shape, dtype=A.dtype)
        self._impl = _impl
        lo, hi = A._row_lo, A._row_hi
        self._lo, self._hi = lo, hi
        ln = hi - lo
        dev = A._data.device
        A = _canonical_csr(A)
        self._src = (A._indptr, A._indices)

        # -- pattern ------------------------------------------------------
        if pattern is None:
            pattern = 1
        if isinstance(pattern, csr_array):
            if tuple(pattern.shape) != tuple(A.shape):
                raise ValueError(f"pattern has shape {pattern.shape}, A has "
                                 f"{A.shape}")
            src_ip, src_ix = pattern._indptr, pattern._indices
        elif isinstance(pattern, (int, np.integer)) \
                and not isinstance(pattern, bool):
            if pattern < 1:
                raise ValueError("pattern power must be at least 1")
            # unit values on |A|'s pattern: every product entry is a
            # positive count, nothing cancels or overflows
            rdt = torch.float32 if A._data.dtype in (
                torch.float32, torch.complex64) else torch.float64
            B = A._with_data(torch.ones(A._data.numel(), dtype=rdt,
                                        device=dev))
            Q = B
            for _ in range(int(pattern) - 1):
                Q = Q.dot(B)
            src_ip, src_ix = Q._indptr, Q._indices
        else:
            raise TypeError("pattern must be None, an int power or a "
                            "csr_array")
        p_ip, p_ix = _lower_triangle(src_ip, src_ix, lo)

        # -- checks, the same decision on every rank (§13.4) ----------------
        plen = p_ip[1:] - p_ip[:-1]
        rows = torch.arange(lo, hi, device=dev)
        if p_ix.numel():
            last = p_ix[(p_ip[1:] - 1).clamp(min=0)].long()
            nodiag = (plen < 1) | (last != rows)
        else:
            nodiag = torch.ones(ln, dtype=torch.bool, device=dev)
        long_row = torch.where(plen > ops.FSAI_MAX_ROW, rows,
                               torch.full_like(rows, n))
        verdict = torch.stack([
            nodiag.any().to(torch.int64) if ln else rows.new_zeros(()),
            n - (long_row.min() if ln else rows.new_full((), n)),
            plen.max() if ln else rows.new_zeros(())]).to(runtime.device)
        if runtime.world_size > 1:
            comm.allreduce_(verdict, op="max")
        missing, long_at, max_row = verdict.cpu().tolist()
        if missing:
            raise ValueError("fsai: every pattern row needs its diagonal "
                             "entry")
        if long_at:
            raise ValueError(
                f"fsai: pattern row {n - long_at} has more than "
                f"FSAI_MAX_ROW = {ops.FSAI_MAX_ROW} entries")
        # the global longest row picks the kernel on every rank alike
        self._max_row = max(int(max_row), 1)

        self._flag = torch.empty(1, dtype=torch.int32, device=dev)
        self.G = csr_array.__new__(csr_array)
        self.G._init_local(p_ip, p_ix, torch.zeros(
            p_ix.numel(), dtype=A._data.dtype, device=dev), A.shape)
        self.G.data = self._rows(A, validate=True)
        self.GH = self.G.conj().transpose()
        self._gh_plan = None
        self._tmp = torch.empty(ln, dtype=A._data.dtype, device=dev)

    # -- setup ----------------------------------------------------------------
    def _rows(self, A, validate: bool) -> torch.Tensor:
        """G's values from A's: gather the window of A's rows this rank's
        pattern names (a collective above world size 1), one kernel launch,
        one host read of the pivot flag."""
        from .csr import _gather_B_window

        w_ip, w_ix, w_dv, w_off = _gather_B_window(self.G, A)
        vals = ops.fsai_rows(self.G._indptr, self.G._indices, w_ip, w_ix,
                             w_dv, w_off, self._lo, self._flag,
                             self._max_row, _impl=self._impl,
                             _validate=validate)
        bad = int(self._flag.item())
        n = self.shape[0]
        row = torch.tensor([self._lo + bad if bad < self._hi - self._lo
                            else n], dtype=torch.int64,
                           device=runtime.device)
        if runtime.world_size > 1:
            comm.allreduce_(row, op="min")
        row = int(row.item())
        if row < n:
            raise RuntimeError(
                f"fsai: A is not positive definite at row {row}")
        return vals

    def _gh_values(self, gvals: torch.Tensor) -> torch.Tensor:
        """GH's values from G's through a stored permutation, built at the
        first ``refactor`` and reused, so later ones move values only.

        The permutation is read off ``csr_array.transpose`` itself: a copy
        of G whose values are its own local entry numbers is transposed
        once, which tells every entry of GH the entry of G it came from;
        the rank that holds it is the owner of GH's column (G's row) under
        the row partition.  Nothing here depends on HOW transpose orders
        its output.  Above world size 1 each rank then asks the owners for
        the entries it needs (one all-to-allv of index lists, once), and
        every call answers with one all-to-allv of values."""
        ws = runtime.world_size
        if self._gh_plan is None:
            nnz = int(self.G._data.numel())
            # entry numbers are exact in float64 (nnz < 2**53)
            ids = self.G._with_data(torch.arange(
                nnz, dtype=torch.float64, device=self.G._data.device))
            T = ids.transpose()
            if not (T._indptr.shape == self.GH._indptr.shape
                    and torch.equal(T._indptr, self.GH._indptr)
                    and torch.equal(T._indices, self.GH._indices)):
                raise RuntimeError("fsai: transpose gave GH another layout")
            src_idx = T._data.long()
            if ws == 1:
                self._gh_plan = (src_idx, None, None, None)
            else:
                part = runtime.partition(self.shape[0])
                src = torch.clamp(torch.div(
                    T._indices.long(), max(part.chunk, 1),
                    rounding_mode="floor"), max=ws - 1)
                # received values arrive grouped by source rank, each group
                # in the order of the request sent to that rank
                order = torch.argsort(src, stable=True)
                want = torch.bincount(src.cpu(), minlength=ws).tolist()
                asked = comm.alltoallv(
                    list(torch.split(src_idx[order], want)))
                give = [int(t.numel()) for t in asked]
                self._gh_plan = (None, torch.cat(asked), give, order)
        perm, send_idx, give, order = self._gh_plan
        if perm is not None:
            v = gvals[perm]
        else:
            got = torch.cat(comm.alltoallv(
                list(torch.split(gvals[send_idx], give))))
            v = torch.empty_like(got)
            v[order] = got
        return torch.conj(v).resolve_conj().contiguous()

    def refactor(self, A2) -> "FSAI":
        """New values on the SAME sparsity pattern: the pattern
        construction and the argument checks are skipped, and ``G`` and
        ``GH`` stay the same objects, so their cached SpMV plans survive;
        GH's values follow G's through a stored permutation.  A
        non-canonical ``A2`` is summed on a copy first, as in ``fsai``.
        ``ValueError`` for another pattern."""
        same = (tuple(A2.shape) == self.shape
                and getattr(A2, "format", None) == "csr"
                and hasattr(A2, "_indptr"))
        if same:
            A2 = _canonical_csr(A2)
            ip, ix = self._src
            same = (A2._indptr is ip and A2._indices is ix) or (
                A2._indptr.shape == ip.shape and A2._indices.shape == ix.shape
                and torch.equal(A2._indptr, ip)
                and torch.equal(A2._indices.long(), ix.long()))
        if runtime.world_size > 1:
            flag = torch.tensor([0 if same else 1], dtype=torch.int64,
                                device=runtime.device)
            comm.allreduce_(flag, op="max")
            same = not bool(flag.item())
        if not same:
            raise ValueError("refactor needs a csr_array with the sparsity "
                             "pattern of the matrix fsai was built from")
        want = to_torch_dtype(self.dtype)
        if A2._data.dtype != want:
            A2 = A2.astype(self.dtype)
        vals = self._rows(A2, validate=False)
        # through the data setter: it marks value-bound caches stale
        self.G.data = vals
        self.GH.data = self._gh_values(vals)
        return self

    # -- apply ------------------------------------------------------------------
    def matvec(self, r, out=None):
        """``G^H (G r)``: two SpMVs, the intermediate in a buffer allocated
        at construction."""
        x = _to_local_vec(r, self.shape[0], self.dtype, self._tmp.device)
        if out is not None:
            out = _plain(out)
        self.G.dot(x, out=self._tmp)
        y = self.GH.dot(self._tmp, out=out)
        return out if out is not None else _plain(y)

    def matmat(self, R):
        """``G^H (G R)`` for an (n, k) block through the SpMM kernels."""
        if getattr(R, "ndim", None) != 2:
            raise ValueError("expected a 2-D block of column vectors")
        return _plain(self.GH.matmat(_plain(self.G.matmat(R))))

    # the operator is Hermitian
    rmatvec = matvec
    rmatmat = matmat


def fsai(A, pattern=None) -> FSAI:
    """FSAI preconditioner of a square Hermitian positive definite
    csr_array in canonical format (duplicates are summed on a copy first),
    as a ``LinearOperator`` any solver here takes as ``M=``::

        M = linalg.fsai(A); x, it = linalg.cg(A, b, M=M)

    ``pattern``: ``None`` or an int ``p >= 1`` for the lower triangle of
    the pattern of ``|A|^p`` (``p - 1`` SpGEMMs), or a csr_array of A's
    shape whose lower triangle is taken.  Only the entries of A with
    ``col <= row`` are read.  ``ValueError`` for a pattern row without its
    diagonal or with more than ``FSAI_MAX_ROW`` = 32 entries (before any
    kernel runs), ``RuntimeError`` naming the global row where A is not
    positive definite.  See :class:`FSAI`."""
    return FSAI(A, pattern)

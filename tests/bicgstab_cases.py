# SPDX-License-Identifier: Apache-2.0
"""Operators, numpy formulas and the numpy replay shared by the BiCGSTAB
tests (CPU, GPU and the multi-process worker)."""
import numpy as np
import scipy.sparse as sp

from testutils import sample_csr

DTYPES = [np.float32, np.float64, np.complex64, np.complex128]


def solve_rtol(dtype):
    """Solver rtol per dtype; the tests assert the TRUE residual at 10x."""
    single = np.dtype(dtype) in (np.dtype(np.float32), np.dtype(np.complex64))
    return 1e-5 if single else 1e-10


def convdiff_stencil(cx=0.6, cy=0.3):
    return [[0, -1 - cy, 0], [-1 - cx, 4, -1 + cx], [0, -1 + cy, 0]]


def convdiff(nx, ny, cx=0.6, cy=0.3, dtype=np.float64):
    """5-point diffusion plus central convection (scipy); the complex
    variant adds 0.2j I."""
    Tx = sp.diags([-1 - cx, 2, -1 + cx], [-1, 0, 1], shape=(nx, nx))
    Ty = sp.diags([-1 - cy, 2, -1 + cy], [-1, 0, 1], shape=(ny, ny))
    A = sp.kron(sp.identity(ny), Tx) + sp.kron(Ty, sp.identity(nx))
    if np.dtype(dtype).kind == "c":
        A = A + 0.2j * sp.identity(nx * ny)
    A = sp.csr_array(A.astype(dtype))
    A.sort_indices()
    return A


def convdiff_lsp(nx, ny, dtype=np.float64, cx=0.6, cy=0.3):
    """The same operator from gallery.stencil_grid (affine on the GPU)."""
    from legate_sparse import gallery
    S = np.array(convdiff_stencil(cx, cy), dtype=dtype)
    if np.dtype(dtype).kind == "c":
        S[1, 1] += 0.2j
    return gallery.stencil_grid(S, (ny, nx), dtype=dtype)


def nonaffine(dtype=np.float64):
    """Random sparse 300x300 made diagonally dominant by an irregular
    diagonal rowsum(|S|) + 1 + (i mod 7)."""
    S = sample_csr(300, 300, 0.05, seed=5, dtype=dtype)
    d = np.asarray(abs(S).sum(axis=1)).reshape(-1) + 1 + np.arange(300) % 7
    A = sp.csr_array((S + sp.diags(d.astype(dtype))).astype(dtype))
    A.sort_indices()
    return A


def rhs(n, dtype, seed=3):
    rng = np.random.default_rng(seed)
    b = rng.standard_normal(n)
    if np.dtype(dtype).kind == "c":
        b = b + 1j * rng.standard_normal(n)
    return b.astype(dtype)


def rel_residual(A, x, b):
    A = A.astype(np.complex128 if np.iscomplexobj(b) else np.float64)
    x = np.asarray(x, dtype=A.dtype).reshape(-1)
    b = np.asarray(b, dtype=A.dtype).reshape(-1)
    return np.linalg.norm(b - A @ x) / np.linalg.norm(b)


# ---- numpy formulas of the four fused ops (guarded division) -------------
def gdiv(a, b):
    return a / b if b != 0 else a * 0


def np_bicgstab_p(p, r, v, rho, rhv, ts, tt):
    omega = gdiv(ts, tt)
    beta = gdiv(rho, rhv) * gdiv(tt, ts)
    return r + beta * (p - omega * v)


def np_bicgstab_s(r, v, rho, rhv):
    return r - gdiv(rho, rhv) * v


def np_vdot2(t, s):
    return np.array([np.vdot(t, s), np.vdot(t, t)])


def np_bicgstab_xr(x, phat, shat, s, t, rhat, rho, rhv, ts, tt):
    alpha = gdiv(rho, rhv)
    omega = gdiv(ts, tt)
    xn = x + alpha * phat + omega * shat
    rn = s - omega * t
    return xn, rn, np.array([np.vdot(rhat, rn), np.vdot(rn, rn)])


def np_replay(A, b, steps, M=None):
    """The solver's recurrence, transcribed step by step (x0 = 0)."""
    apply_M = (lambda z: z) if M is None else (lambda z: M @ z)
    x = np.zeros_like(b)
    r = b.copy()
    rhat = r.copy()
    p = r.copy()
    rho = np.vdot(rhat, r)
    v = rhv = ts = tt = None
    for k in range(steps):
        if k > 0:
            p = np_bicgstab_p(p, r, v, rho, rhv, ts, tt)
        phat = apply_M(p)
        v = A @ phat
        rhv = np.vdot(rhat, v)
        s = np_bicgstab_s(r, v, rho, rhv)
        shat = apply_M(s)
        t = A @ shat
        ts, tt = np_vdot2(t, s)
        x, r, (rho, _) = np_bicgstab_xr(x, phat, shat, s, t, rhat, rho, rhv,
                                        ts, tt)
    return x

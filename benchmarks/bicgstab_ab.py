#!/usr/bin/env python3
# A/B: lsp.linalg.bicgstab (fused kernels, device scalars) against the same
# recurrence written with A.dot and plain torch ops — what a user could
# write without the solver.  fp64 convection-diffusion operator on an NxN
# grid (gallery.stencil_grid, the affine SpMV carries both arms), a fixed
# number of iterations (rtol = atol = 0, one convergence test at the end).
#
# Arm B is written to be as cheap as torch allows: scalars stay 0-dim
# device tensors (no host read in the loop), the divisions are plain (no
# zero guard, so fewer small kernels than the solver's semantics need),
# v and t are written through out=.
#
# The arms alternate in one process after a warm-up of each; every clock
# read follows a device synchronise.  A timed call is a whole solve, so
# ms/iter includes each arm's set-up (buffers, the norm of b) spread over
# the iterations.
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import legate_sparse as lsp
from legate_sparse import gallery

CX, CY = 0.6, 0.3
STENCIL = [[0, -1 - CY, 0], [-1 - CX, 4, -1 + CX], [0, -1 + CY, 0]]


def torch_bicgstab(A, b, iters):
    """BiCGSTAB with A.dot and torch ops (x0 = 0, unpreconditioned)."""
    x = torch.zeros_like(b)
    r = b.clone()
    rhat = r.clone()
    p = r.clone()
    v = torch.empty_like(b)
    t = torch.empty_like(b)
    rho = torch.vdot(rhat, r)
    alpha = omega = rho_old = None
    for k in range(iters):
        if k > 0:
            beta = (rho / rho_old) * (alpha / omega)
            p = r + beta * (p - omega * v)
        A.dot(p, out=v)
        alpha = rho / torch.vdot(rhat, v)
        s = r - alpha * v
        A.dot(s, out=t)
        omega = torch.vdot(t, s) / torch.vdot(t, t)
        x += alpha * p
        x += omega * s
        r = s - omega * t
        rho_old = rho
        rho = torch.vdot(rhat, r)
    return x, torch.sqrt(torch.vdot(r, r))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", type=int, default=2048)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=7)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bicgstab_ab.py measures on the GPU; no device found")
    sync = torch.cuda.synchronize

    N = args.grid
    A = gallery.stencil_grid(STENCIL, (N, N), dtype=np.float64)
    n = A.shape[0]
    dev = A.data.device
    gen = torch.Generator(device=dev).manual_seed(0)
    b = torch.rand(n, dtype=torch.float64, device=dev, generator=gen)
    bn = float(torch.linalg.norm(b))

    def arm_a(iters=args.iters):
        x, info = lsp.linalg.bicgstab(A, b, rtol=0.0, atol=0.0,
                                      maxiter=iters, conv_test_iters=iters)
        return x.as_subclass(torch.Tensor), info

    def arm_b(iters=args.iters):
        return torch_bicgstab(A, b, iters)

    # the arms must agree before any time is worth reading: few steps
    # (the iteration amplifies rounding differences as it goes on)
    xa, _ = arm_a(5)
    xb, _ = arm_b(5)
    rel5 = float(torch.linalg.norm(xa - xb) / torch.linalg.norm(xb))
    assert rel5 < 1e-10, rel5
    # warm-up at the timed size; residuals of both arms after all steps
    xa, info = arm_a()
    xb, _ = arm_b()
    res_a = float(torch.linalg.norm(b - A.dot(xa))) / bn
    res_b = float(torch.linalg.norm(b - A.dot(xb))) / bn

    def timed(fn):
        sync()
        t0 = time.perf_counter()
        fn()
        sync()
        return (time.perf_counter() - t0) / args.iters * 1e3

    ta, tb = [], []
    for _ in range(args.rounds):
        ta.append(timed(arm_a))
        tb.append(timed(arm_b))

    def stats(ts):
        s = sorted(ts)
        return {"median": s[len(s) // 2], "min": s[0], "max": s[-1]}

    sa, sb = stats(ta), stats(tb)
    print(f"device: {torch.cuda.get_device_name(0)}; grid {N}x{N}, "
          f"n = {n}, fp64; {args.iters} iterations per solve; "
          f"{args.rounds} alternating rounds")
    print(f"agreement after 5 steps: rel diff {rel5:.1e}; true relative "
          f"residual after {args.iters}: A {res_a:.3e} (info {info}), "
          f"B {res_b:.3e}")
    print("| arm | ms/iter median | min | max |")
    print("|---|---|---|---|")
    print(f"| A lsp.linalg.bicgstab | {sa['median']:.4f} | {sa['min']:.4f} "
          f"| {sa['max']:.4f} |")
    print(f"| B A.dot + torch ops | {sb['median']:.4f} | {sb['min']:.4f} "
          f"| {sb['max']:.4f} |")
    print(f"B / A (medians): {sb['median'] / sa['median']:.2f}")


if __name__ == "__main__":
    main()

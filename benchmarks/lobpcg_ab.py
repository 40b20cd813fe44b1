#!/usr/bin/env python3
# A/B: lsp.linalg.lobpcg with the gfx950 block kernels (arm A) against the
# SAME driver with block_gram / block_update / block_residual routed through
# their torch formulations (arm B, the private _block_impl="torch" switch;
# as cheap as torch allows: the Gram is a split-K batched product, because
# the plain X^H @ Y runs on a single tile and takes ~0.45 s a call here).
# 5-point Poisson on an NxN grid (gallery.stencil_grid), k = 8, fp64,
# smallest eigenvalues, a fixed number of iterations (tol = 0, so the solver
# never converges and warns at maxiter; the warning is silenced here).
#
# The arms alternate in one process after a warm-up of each; every clock
# read follows a device synchronise.  A timed call is a whole solve, so
# ms/iter includes set-up (buffers, the initial and the final Rayleigh-Ritz)
# spread over the iterations.  Before that, a first table times each block
# op alone at the solver's shapes, HIP against torch, with device events.
import argparse
import os
import sys
import time
import warnings

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import legate_sparse as lsp
from legate_sparse import gallery, ops

STENCIL = [[0, -1, 0], [-1, 4, -1], [0, -1, 0]]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", type=int, default=2048)
    ap.add_argument("--k", type=int, default=8)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("lobpcg_ab.py measures on the GPU; no device found")
    sync = torch.cuda.synchronize

    N, k = args.grid, args.k
    A = gallery.stencil_grid(STENCIL, (N, N), dtype=np.float64)
    n = A.shape[0]
    dev = A.data.device
    gen = torch.Generator(device=dev).manual_seed(0)
    X0 = torch.randn(n, k, dtype=torch.float64, device=dev, generator=gen)

    # ---- each op alone, at the solver's shapes --------------------------
    Xb = X0.clone()
    Yb = torch.randn(n, k, dtype=torch.float64, device=dev, generator=gen)
    Pb = torch.randn(n, k, dtype=torch.float64, device=dev, generator=gen)
    Zb = torch.empty_like(Xb)
    C = [torch.randn(k, k, dtype=torch.float64, device=dev, generator=gen)
         for _ in range(3)]
    th = torch.linspace(0, 1, k, dtype=torch.float64, device=dev)
    nr = torch.empty(k, dtype=torch.float64, device=dev)
    G = torch.empty(k, k, dtype=torch.float64, device=dev)
    t3 = [(Xb, C[0]), (Yb, C[1]), (Pb, C[2])]
    es = 8
    cases = [
        ("block_gram (torch: split-K bmm)", 2 * n * k * es,
         lambda: ops.block_gram(Xb, Yb, out=G),
         lambda: ops._block_gram_torch(Xb, Yb, True, G)),
        ("block_gram (torch: plain X^T @ Y)", 2 * n * k * es,
         lambda: ops.block_gram(Xb, Yb, out=G),
         lambda: G.copy_(Xb.transpose(0, 1) @ Yb)),
        ("block_update, 3 terms", 4 * n * k * es,
         lambda: ops.block_update(Zb, t3),
         lambda: ops._block_update_torch(Zb, t3, False)),
        ("block_update, 1 term", 2 * n * k * es,
         lambda: ops.block_update(Zb, t3[:1]),
         lambda: ops._block_update_torch(Zb, t3[:1], False)),
        ("block_residual", 3 * n * k * es,
         lambda: ops.block_residual(Zb, Yb, Xb, th, nr),
         lambda: ops._block_residual_torch(Zb, Yb, Xb, th, nr)),
    ]

    def ev_time(fn, reps=10):
        # the plain skinny GEMM takes ~0.5 s a call: two repetitions do
        fn()
        sync()
        e0 = torch.cuda.Event(enable_timing=True)
        e1 = torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        sync()
        return e0.elapsed_time(e1) / reps

    print(f"device: {torch.cuda.get_device_name(0)}; grid {N}x{N}, n = {n}, "
          f"k = {k}, fp64")
    print("| op (n x k fp64) | minimal bytes | HIP ms | HIP GB/s | torch ms "
          "| torch / HIP |")
    print("|---|---|---|---|---|---|")
    for name, nbytes, f_hip, f_torch in cases:
        # alternate twice, keep the better of each
        th_ = min(ev_time(f_hip), ev_time(f_hip))
        rt = 2 if "plain" in name else 10
        tt_ = min(ev_time(f_torch, rt), ev_time(f_torch, rt))
        print(f"| {name} | {nbytes / 1e6:.0f} MB | {th_:.4f} | "
              f"{nbytes / th_ / 1e6:.0f} | {tt_:.4f} | {tt_ / th_:.2f} |",
              flush=True)

    def arm(impl, iters=args.iters):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", UserWarning)
            w, V, hist = lsp.linalg.lobpcg(
                A, X0, tol=0.0, maxiter=iters, largest=False,
                retResidualNormsHistory=True, _block_impl=impl)
        return w, V, hist

    # the arms must agree before any time is worth reading
    t0 = time.perf_counter()
    wa, _, _ = arm("hip", 5)
    sync()
    t1 = time.perf_counter()
    wb, _, _ = arm("torch", 5)
    sync()
    print(f"first solves (5 iterations, cold): A {t1 - t0:.2f} s, "
          f"B {time.perf_counter() - t1:.2f} s", flush=True)
    rel5 = float(np.abs(wa - wb).max() / np.abs(wb).max())
    assert rel5 < 1e-8, rel5
    wa, _, ha = arm("hip")
    wb, _, hb = arm("torch")

    def timed(impl):
        sync()
        t0 = time.perf_counter()
        arm(impl)
        sync()
        return (time.perf_counter() - t0) / args.iters * 1e3

    ta, tb = [], []
    for _ in range(args.rounds):
        ta.append(timed("hip"))
        tb.append(timed("torch"))
        print(f"round: A {ta[-1]:.3f} ms/iter, B {tb[-1]:.3f} ms/iter",
              flush=True)

    def stats(ts):
        s = sorted(ts)
        return {"median": s[len(s) // 2], "min": s[0], "max": s[-1]}

    sa, sb = stats(ta), stats(tb)
    print()
    print(f"smallest eigenvalues; {args.iters} iterations per solve; "
          f"{args.rounds} alternating rounds")
    print(f"eigenvalue agreement after 5 iterations: rel diff {rel5:.1e}; "
          f"largest residual norm after {args.iters}: "
          f"A {ha[-1].max():.3e}, B {hb[-1].max():.3e}")
    print("| arm | ms/iter median | min | max |")
    print("|---|---|---|---|")
    print(f"| A HIP block kernels | {sa['median']:.4f} | {sa['min']:.4f} "
          f"| {sa['max']:.4f} |")
    print(f"| B torch block ops | {sb['median']:.4f} | {sb['min']:.4f} "
          f"| {sb['max']:.4f} |")
    print(f"B / A (medians): {sb['median'] / sa['median']:.2f}")


if __name__ == "__main__":
    main()

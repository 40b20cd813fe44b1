#!/usr/bin/env python3
# A/B: the ILU(0) apply (linalg.ilu0(A).matvec / .matmat, two level-scheduled
# triangular sweeps) on the gfx950 kernels of src/hip/sptrsv.hip (arm A)
# against the SAME operator with both sweeps routed through per-level torch
# index ops (arm B, the private _impl="torch" switch), fp64, on
#   - a 3-D 7-point grid of about 4M rows (160^3), and
#   - the 2-D 5-point grid 2048^2,
# both in natural ordering.  Reported per matrix: levels, launches per apply
# after chaining (the one performance condition: launches <= levels), the
# factorisation time of each arm, matvec and matmat (k = 8) per call, and one
# A.dot on the same matrix for scale.
#
# Then end to end: bicgstab on a 3-D convection-diffusion problem (upwind
# x-convection) with M=None against M=ilu0(A), to the same rtol: iterations
# and wall time, the factorisation counted separately.
#
# The arms alternate in one process after a warm-up of each; every clock
# read follows a device synchronise.
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import scipy.sparse as sp
import torch

import legate_sparse as lsp
from legate_sparse import linalg


def grid_matrix(dims, cx=0.0):
    """5-/7-point diffusion on a grid, natural ordering (first dimension
    fastest), plus first-order upwind convection of strength cx along the
    first dimension.  No explicit zeros are stored."""
    n = int(np.prod(dims))
    idx = np.arange(n, dtype=np.int64)
    rows, cols, vals = [idx], [idx], [np.full(n, 2.0 * len(dims) + cx)]
    stride = 1
    for ax, d in enumerate(dims):
        c = (idx // stride) % d
        up = idx[c + 1 < d]
        west = -1.0 - (cx if ax == 0 else 0.0)
        rows += [up, up + stride]
        cols += [up + stride, up]
        vals += [np.full(up.size, -1.0), np.full(up.size, west)]
        stride *= d
    A = sp.csr_matrix((np.concatenate(vals),
                       (np.concatenate(rows), np.concatenate(cols))),
                      shape=(n, n))
    A.sort_indices()
    return A


def timed(fn, reps, sync):
    sync()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    sync()
    return (time.perf_counter() - t0) / reps * 1e3


def median(ts):
    return sorted(ts)[len(ts) // 2]


def apply_ab(label, dims, args, sync):
    S = grid_matrix(dims)
    A = lsp.csr_array(S)
    n = A.shape[0]
    dev = A.data.device
    sync()
    t0 = time.perf_counter()
    M = linalg.ilu0(A)
    sync()
    t_first = (time.perf_counter() - t0) * 1e3      # analysis + factor
    t_fa = timed(lambda: M.refactor(A), 3, sync)    # numeric factor only
    Fa = M.factor_local()[2].clone()
    M._impl = "torch"
    M.refactor(A)
    t_fb = timed(lambda: M.refactor(A), 1, sync)
    Fb = M.factor_local()[2]
    fdiff = float((Fa - Fb).abs().max())
    lv = M.levels
    launches = M.launches_per_apply
    assert launches <= sum(lv), (launches, lv)

    gen = torch.Generator(device=dev).manual_seed(0)
    r = torch.randn(n, dtype=torch.float64, device=dev, generator=gen)
    R = torch.randn(n, args.k, dtype=torch.float64, device=dev,
                    generator=gen)
    out = torch.empty_like(r)

    def arm(impl, fn):
        M._impl = "native" if impl == "A" else "torch"
        return fn()

    # the arms must agree before any time is worth reading (also warm-up)
    ya = arm("A", lambda: M.matvec(r).clone())
    yb = arm("B", lambda: M.matvec(r).clone())
    rel = float((ya - yb).abs().max() / yb.abs().max())
    assert rel < 1e-10, rel
    Ya = arm("A", lambda: M.matmat(R))
    Yb = arm("B", lambda: M.matmat(R))
    relm = float((Ya - Yb).abs().max() / Yb.abs().max())
    assert relm < 1e-10, relm
    del Ya, Yb

    res = {"A": {"mv": [], "mm": []}, "B": {"mv": [], "mm": []}}
    for _ in range(args.rounds):
        for impl, reps in (("A", args.reps), ("B", 1)):
            res[impl]["mv"].append(arm(impl, lambda: timed(
                lambda: M.matvec(r, out=out), reps, sync)))
            res[impl]["mm"].append(arm(impl, lambda: timed(
                lambda: M.matmat(R), reps, sync)))
    M._impl = "native"
    t_dot = timed(lambda: A.dot(r), 20, sync)

    print(f"\n### {label}: n = {n}, nnz = {S.nnz}, fp64")
    print(f"levels: L sweep {lv[0]}, U sweep {lv[1]}; launches per apply "
          f"after chaining: {launches} (levels: {sum(lv)})")
    print(f"first ilu0(A) (host level analysis of both sweeps + factor): "
          f"{t_first:.1f} ms; refactor: HIP {t_fa:.2f} ms, torch "
          f"{t_fb:.1f} ms; factors agree to {fdiff:.1e}")
    print(f"arms agree: matvec rel diff {rel:.1e}, matmat {relm:.1e}; "
          f"one A.dot: {t_dot:.4f} ms")
    print("| call | A HIP ms (median, min, max) | B torch ms (median, min, "
          "max) | B / A |")
    print("|---|---|---|---|")
    for key, name in (("mv", "matvec"), ("mm", f"matmat k = {args.k}")):
        a, b = res["A"][key], res["B"][key]
        print(f"| {name} | {median(a):.3f}, {min(a):.3f}, {max(a):.3f} | "
              f"{median(b):.2f}, {min(b):.2f}, {max(b):.2f} | "
              f"{median(b) / median(a):.1f} |", flush=True)


def end_to_end(args, sync):
    m = args.cd_grid
    S = grid_matrix((m, m, m), cx=args.cx)
    A = lsp.csr_array(S)
    n = A.shape[0]
    dev = A.data.device
    gen = torch.Generator(device=dev).manual_seed(1)
    b = torch.randn(n, dtype=torch.float64, device=dev, generator=gen)
    sync()
    t0 = time.perf_counter()
    M = linalg.ilu0(A)
    sync()
    t_setup = (time.perf_counter() - t0) * 1e3

    def solve(Mop):
        calls = []
        sync()
        t0 = time.perf_counter()
        x, info = linalg.bicgstab(A, b, rtol=args.rtol, M=Mop,
                                  conv_test_iters=args.conv_test_iters,
                                  callback=lambda xk: calls.append(1))
        sync()
        dt = (time.perf_counter() - t0) * 1e3
        rn = float(torch.linalg.norm(b - A.dot(x)) / torch.linalg.norm(b))
        return dt, len(calls), int(info), rn

    solve(None), solve(M)                            # warm-up
    rows = {"M=None": [], "M=ilu0(A)": []}
    for _ in range(args.rounds):
        rows["M=None"].append(solve(None))
        rows["M=ilu0(A)"].append(solve(M))
    print(f"\n### bicgstab, 3-D convection-diffusion {m}^3 (upwind "
          f"x-convection {args.cx}), n = {n}, rtol {args.rtol}, convergence "
          f"tested every {args.conv_test_iters} iterations")
    print(f"ilu0(A) set-up (level analysis + factor): {t_setup:.1f} ms; "
          f"levels {M.levels}, launches per apply {M.launches_per_apply}")
    print("| M | iterations | info | true rel. residual | wall ms (median, "
          "min, max) | ms / iteration |")
    print("|---|---|---|---|---|---|")
    for name, rs in rows.items():
        ts = [r[0] for r in rs]
        print(f"| {name} | {rs[0][1]} | {rs[0][2]} | {rs[0][3]:.2e} | "
              f"{median(ts):.1f}, {min(ts):.1f}, {max(ts):.1f} | "
              f"{median(ts) / max(rs[0][1], 1):.3f} |", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid3", type=int, default=160)
    ap.add_argument("--grid2", type=int, default=2048)
    ap.add_argument("--cd-grid", type=int, default=96)
    ap.add_argument("--cx", type=float, default=3.0)
    ap.add_argument("--k", type=int, default=8)
    ap.add_argument("--rtol", type=float, default=1e-8)
    ap.add_argument("--conv-test-iters", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("ilu0_ab.py measures on the GPU; no device found")
    sync = torch.cuda.synchronize
    print(f"device: {torch.cuda.get_device_name(0)}")
    g3, g2 = args.grid3, args.grid2
    apply_ab(f"3-D 7-point {g3}^3", (g3, g3, g3), args, sync)
    apply_ab(f"2-D 5-point {g2}^2", (g2, g2), args, sync)
    end_to_end(args, sync)

    # the bidiagonal test matrix: one launch per sweep
    nb = 1000
    B = sp.diags([np.full(nb - 1, -0.5), np.full(nb, 2.0)], [-1, 0],
                 format="csr")
    La = lsp.csr_array(B)
    info = linalg._tri_analysis(La, True, False)
    print(f"\nbidiagonal {nb}: levels {info['sched'].n_levels}, launches "
          f"{info['sched'].n_launches()}")
    assert info["sched"].n_launches() == 1


if __name__ == "__main__":
    main()

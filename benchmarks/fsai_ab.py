#!/usr/bin/env python3
# FSAI (linalg.fsai, docs/DESIGN.md §18) measured in fp64 on
#   - the 3-D 7-point grid 160^3 and the 2-D 5-point grid 2048^2,
#   - each with constant coefficients and with jump coefficients (cell
#     values 10^{0..3}, harmonic-mean couplings, 1e-3 k on the diagonal).
#
# Per matrix and pattern power p = 1, 2, 3:
#   set-up   the whole fsai(A, p) call (pattern SpGEMMs, checks, kernel,
#            transpose), refactor (same pattern), and the row kernel alone:
#            arm A = src/hip/fsai.hip, arm B = the batched torch
#            formulation (ops.fsai_rows(_impl="torch")); B runs on the
#            constant-coefficient matrices only (its cost does not depend
#            on the values);
#   apply    M.matvec against one A.dot and against ilu0(A).matvec;
#   solve    cg to one rtol with M=None, M=ilu0(A) and M=fsai(A, p):
#            iterations, true residual and wall time, set-up apart.
#
# Everything timed is warmed up first (every p's constructor, both row
# kernel arms, every solve arm).  Arms that are compared alternate inside
# each round, in one process: the row kernel as A, B, A, B, ..., the solves
# as None, ilu0, fsai(1), fsai(2), fsai(3), None, ...  A solve arm whose
# warm-up takes longer than --slow-ms joins the first round only.  Every
# clock read follows a device synchronise; medians over --rounds rounds.
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import scipy.sparse as sp
import torch

import legate_sparse as lsp
from legate_sparse import linalg, ops


def grid_matrix(dims, jump=False, seed=5):
    """5-/7-point diffusion, natural ordering, first dimension fastest.
    Constant: 2 * ndim on the diagonal, -1 off it.  Jump: cell coefficients
    k in {1, 10, 100, 1000}, coupling 2 k_i k_j / (k_i + k_j), diagonal =
    sum of the row's couplings + 1e-3 k_i."""
    n = int(np.prod(dims))
    idx = np.arange(n, dtype=np.int64)
    k = 10.0 ** np.random.default_rng(seed).integers(0, 4, n) if jump \
        else None
    rows, cols, vals = [], [], []
    diag = np.full(n, 1e-3) * k if jump else np.full(n, 2.0 * len(dims))
    stride = 1
    for d in dims:
        c = (idx // stride) % d
        up = idx[c + 1 < d]
        w = 2 * k[up] * k[up + stride] / (k[up] + k[up + stride]) if jump \
            else np.ones(up.size)
        rows += [up, up + stride]
        cols += [up + stride, up]
        vals += [-w, -w]
        if jump:
            np.add.at(diag, up, w)
            np.add.at(diag, up + stride, w)
        stride *= d
    A = sp.csr_matrix((np.concatenate(vals + [diag]),
                       (np.concatenate(rows + [idx]),
                        np.concatenate(cols + [idx]))), shape=(n, n))
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


def kernel_fn(M, A, impl):
    """The row kernel alone on M's pattern -> (callable, its output)."""
    flag = torch.empty(1, dtype=torch.int32, device=A.data.device)
    out = torch.empty_like(M.G.data)
    return (lambda: ops.fsai_rows(
        M.G.indptr, M.G.indices, A.indptr, A.indices, A.data, 0, 0, flag,
        M._max_row, out=out, _impl=impl, _validate=False)), out


def solve(A, b, Mop, args, sync):
    sync()
    t0 = time.perf_counter()
    x, it = linalg.cg(A, b, rtol=args.rtol, M=Mop, maxiter=args.maxiter,
                      conv_test_iters=args.conv_test_iters)
    sync()
    dt = (time.perf_counter() - t0) * 1e3
    rn = float(torch.linalg.norm(b - A.dot(x)) / torch.linalg.norm(b))
    return dt, int(it), rn


def one_matrix(label, dims, jump, args, sync):
    S = grid_matrix(dims, jump)
    A = lsp.csr_array(S)
    n = A.shape[0]
    dev = A.data.device
    gen = torch.Generator(device=dev).manual_seed(0)
    r = torch.randn(n, dtype=torch.float64, device=dev, generator=gen)
    b = torch.randn(n, dtype=torch.float64, device=dev, generator=gen)
    out = torch.empty_like(r)
    print(f"\n### {label}: n = {n}, nnz = {S.nnz}, fp64", flush=True)
    A.dot(r)
    t_dot = median([timed(lambda: A.dot(r, out=out), 20, sync)
                    for _ in range(args.rounds)])

    ilu = None
    if not args.no_ilu0:
        sync()
        t0 = time.perf_counter()
        ilu = linalg.ilu0(A)
        sync()
        t_ilu_setup = (time.perf_counter() - t0) * 1e3
        ilu.matvec(r, out=out)
        t_ilu = median([timed(lambda: ilu.matvec(r, out=out), 2, sync)
                        for _ in range(args.rounds)])
        print(f"one A.dot: {t_dot:.4f} ms; ilu0(A): set-up "
              f"{t_ilu_setup:.1f} ms, matvec {t_ilu:.3f} ms "
              f"({ilu.launches_per_apply} launches)", flush=True)
    else:
        print(f"one A.dot: {t_dot:.4f} ms", flush=True)

    Ms = {}
    print("| p | longest row | nnz(G) | fsai(A, p) ms | refactor ms | row "
          "kernel A HIP ms | row kernel B torch ms | B / A | matvec ms | "
          "/ A.dot" + ("" if ilu is None else " | / ilu0 matvec") + " |")
    print("|---|---|---|---|---|---|---|---|---|---|"
          + ("" if ilu is None else "---|"))
    for p in args.powers:
        linalg.fsai(A, p)                                    # warm-up
        fulls = []
        for _ in range(args.rounds):
            M = None
            sync()
            t0 = time.perf_counter()
            M = linalg.fsai(A, p)
            sync()
            fulls.append((time.perf_counter() - t0) * 1e3)
        t_full = median(fulls)
        M.refactor(A)                                        # warm-up
        t_re = median([timed(lambda: M.refactor(A), 1, sync)
                       for _ in range(args.rounds)])
        fa, va = kernel_fn(M, A, "native")
        fa()                                                 # warm-up
        assert torch.equal(va, M.G.data)
        with_b = args.torch_arm and not jump
        if with_b:
            fb, vb = kernel_fn(M, A, "torch")
            fb()                                             # warm-up
            rel = float((va - vb).abs().max() / vb.abs().max())
            assert rel < 1e-10, rel
        tas, tbs = [], []
        for _ in range(args.rounds):                         # A, B, A, B, ...
            tas.append(timed(fa, 3, sync))
            if with_b:
                tbs.append(timed(fb, 1, sync))
        t_ka = median(tas)
        if with_b:
            t_kb = median(tbs)
            kb, ratio = f"{t_kb:.1f}", f"{t_kb / t_ka:.1f}"
            del fb, vb
        else:
            kb = ratio = "-"
        del fa, va
        M.matvec(r, out=out)
        t_mv = median([timed(lambda: M.matvec(r, out=out), 10, sync)
                       for _ in range(args.rounds)])
        print(f"| {p} | {M._max_row} | {M.G.nnz} | {t_full:.1f} | {t_re:.1f} "
              f"| {t_ka:.2f} | {kb} | {ratio} | {t_mv:.4f} | "
              f"{t_mv / t_dot:.2f}"
              + ("" if ilu is None else f" | {t_mv / t_ilu:.3f}") + " |",
              flush=True)
        Ms[p] = M

    print(f"\ncg to rtol {args.rtol} (maxiter {args.maxiter}, convergence "
          f"tested every {args.conv_test_iters} iterations), random b:")
    print("| M | iterations | true rel. residual | wall ms (median, min, "
          "max) | ms / iteration |")
    print("|---|---|---|---|---|")
    arms = [("None", None)]
    if ilu is not None:
        arms.append(("ilu0(A)", ilu))
    arms += [(f"fsai(A, {p})", Ms[p]) for p in args.powers]
    warm = {name: solve(A, b, Mop, args, sync) for name, Mop in arms}
    res = {name: [] for name, _ in arms}
    for rnd in range(args.rounds):                # the arms alternate
        for name, Mop in arms:
            if rnd == 0 or warm[name][0] <= args.slow_ms:
                res[name].append(solve(A, b, Mop, args, sync))
    for name, _ in arms:
        rs = res[name]
        ts = [x[0] for x in rs]
        note = "" if len(ts) == args.rounds else f" ({len(ts)} timed solve)"
        print(f"| {name} | {rs[0][1]} | {rs[0][2]:.2e} | {median(ts):.1f}, "
              f"{min(ts):.1f}, {max(ts):.1f}{note} | "
              f"{median(ts) / max(rs[0][1], 1):.4f} |", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid3", type=int, default=160)
    ap.add_argument("--grid2", type=int, default=2048)
    ap.add_argument("--powers", type=int, nargs="+", default=[1, 2, 3])
    ap.add_argument("--rtol", type=float, default=1e-8)
    ap.add_argument("--maxiter", type=int, default=30000)
    ap.add_argument("--conv-test-iters", type=int, default=25)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--slow-ms", type=float, default=5000.0,
                    help="a solve arm whose warm-up is slower than this "
                         "joins the first round only")
    ap.add_argument("--no-ilu0", action="store_true")
    ap.add_argument("--no-torch-arm", dest="torch_arm", action="store_false")
    ap.add_argument("--only", choices=["3d", "2d"], default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("fsai_ab.py measures on the GPU; no device found")
    sync = torch.cuda.synchronize
    print(f"device: {torch.cuda.get_device_name(0)}")
    g3, g2 = args.grid3, args.grid2
    for jump in (False, True):
        kind = "jump coefficients" if jump else "constant coefficients"
        if args.only != "2d":
            one_matrix(f"3-D 7-point {g3}^3, {kind}", (g3, g3, g3), jump,
                       args, sync)
        if args.only != "3d":
            one_matrix(f"2-D 5-point {g2}^2, {kind}", (g2, g2), jump, args,
                       sync)


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
# A/B: one SpMM (A.matmat(X)) vs the k SpMV calls it replaces
# (A @ X[:, j].contiguous(), which takes the affine SpMV on these
# operators).  fp64; 5-point Poisson on an NxN grid and the banded 11/row
# operator at the same row count; k in {2, 4, 8, 16, 32}.  The two variants
# alternate in one process, every shape is warmed, the clock is read after
# a device synchronise and each variant is timed for >= 1 s in total.
#
# Byte model (fp64, int32 indices, general non-affine SpMV as the model
# baseline): k SpMVs move k*(12*nnz + 16*n); one SpMM that reads A once
# moves 12*nnz + 16*k*n.  "GB/s" below is that model over measured time.
#
# A second table times the narrow and the wide kernel against each other
# on every k both accept (the crossover of path="auto").
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import scipy.sparse as sp
import torch

import legate_sparse as lsp
from legate_sparse import ops
from legate_sparse.gallery import poisson_2d

ROUNDS = 5


def _sync_time(fn, iters):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters


def alternate(fns, min_seconds):
    """Per-call seconds of each fn: ROUNDS rounds, variants alternating
    within a round, each variant timed >= min_seconds over all rounds."""
    iters = []
    for fn in fns:
        for _ in range(3):
            fn()
        t = _sync_time(fn, 3)
        iters.append(max(3, int(min_seconds / ROUNDS / max(t, 1e-7)) + 1))
    res = [[] for _ in fns]
    for _ in range(ROUNDS):
        for i, fn in enumerate(fns):
            res[i].append(_sync_time(fn, iters[i]))
    return res


def stats(ts):
    s = sorted(ts)
    return s[len(s) // 2], s[0], s[-1]


def bench(name, A, ks, min_seconds, out):
    n, N = A.shape
    nnz = A.nnz
    gen = torch.Generator(device="cuda").manual_seed(0)
    print(f"## {name}: n = {n}, nnz = {nnz}", flush=True)
    print("| k | matmat ms (min..max) | k x SpMV ms (min..max) | speedup |"
          " model MB spmm / spmv | GB/s spmm / spmv | max rel diff |")
    print("|---|---|---|---|---|---|---|", flush=True)
    for k in ks:
        X = torch.rand((N, k), dtype=torch.float64, device="cuda",
                       generator=gen)
        Y = torch.empty((n, k), dtype=torch.float64, device="cuda")

        def f_spmm():
            A.matmat(X, out=Y)

        def f_loop():
            for j in range(k):
                A @ X[:, j].contiguous()

        # results must agree before any time is worth reading
        ref = torch.stack([(A @ X[:, j].contiguous()).reshape(-1)
                           for j in range(k)], dim=1)
        f_spmm()
        rel = float((Y - ref).abs().max() / ref.abs().max())
        assert rel < 1e-12, (name, k, rel)
        del ref
        t_mm, t_lp = alternate([f_spmm, f_loop], min_seconds)
        m_mm, lo_mm, hi_mm = stats(t_mm)
        m_lp, lo_lp, hi_lp = stats(t_lp)
        b_mm = 12 * nnz + 16 * k * n
        b_lp = k * (12 * nnz + 16 * n)
        print(f"| {k} | {m_mm * 1e3:.3f} ({lo_mm * 1e3:.3f}.."
              f"{hi_mm * 1e3:.3f}) | {m_lp * 1e3:.3f} ({lo_lp * 1e3:.3f}.."
              f"{hi_lp * 1e3:.3f}) | {m_lp / m_mm:.2f}x | "
              f"{b_mm / 1e6:.0f} / {b_lp / 1e6:.0f} | "
              f"{b_mm / m_mm / 1e9:.0f} / {b_lp / m_lp / 1e9:.0f} | "
              f"{rel:.1e} |", flush=True)
        out.append({"op": name, "k": k, "spmm_ms": m_mm * 1e3,
                    "spmm_ms_min": lo_mm * 1e3, "spmm_ms_max": hi_mm * 1e3,
                    "spmv_loop_ms": m_lp * 1e3,
                    "spmv_loop_ms_min": lo_lp * 1e3,
                    "spmv_loop_ms_max": hi_lp * 1e3,
                    "speedup": m_lp / m_mm, "model_bytes_spmm": b_mm,
                    "model_bytes_spmv_loop": b_lp, "max_rel_diff": rel})
        del X, Y


def bench_paths(name, A, min_seconds, out):
    n, N = A.shape
    print(f"## {name}: narrow vs wide kernel", flush=True)
    print("| k | narrow ms (min..max) | wide ms (min..max) | wide/narrow |")
    print("|---|---|---|---|", flush=True)
    for k in range(1, ops.SPMM_NARROW_KMAX + 1):
        X = torch.rand((N, k), dtype=torch.float64, device="cuda")
        Y = torch.empty((n, k), dtype=torch.float64, device="cuda")
        fns = [lambda p=p: ops.spmm(A._indptr, A._indices, A._data, X, Y,
                                    path=p) for p in ("narrow", "wide")]
        t_n, t_w = alternate(fns, min_seconds)
        m_n, lo_n, hi_n = stats(t_n)
        m_w, lo_w, hi_w = stats(t_w)
        print(f"| {k} | {m_n * 1e3:.3f} ({lo_n * 1e3:.3f}..{hi_n * 1e3:.3f})"
              f" | {m_w * 1e3:.3f} ({lo_w * 1e3:.3f}..{hi_w * 1e3:.3f}) | "
              f"{m_w / m_n:.2f} |", flush=True)
        out.append({"op": name, "k": k, "narrow_ms": m_n * 1e3,
                    "wide_ms": m_w * 1e3})
        del X, Y


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", type=int, default=2048,
                    help="Poisson grid side; both operators get grid^2 rows")
    ap.add_argument("--ks", type=int, nargs="+", default=[2, 4, 8, 16, 32])
    ap.add_argument("--seconds", type=float, default=1.0,
                    help="least total timed seconds per variant and shape")
    ap.add_argument("--no-paths", action="store_true",
                    help="skip the narrow-vs-wide table")
    ap.add_argument("--json", default=None, help="also dump rows as JSON")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("spmm_ab.py measures on the GPU; no device found")
    print(f"device: {torch.cuda.get_device_name(0)}; rounds = {ROUNDS}; "
          f">= {args.seconds} s per variant; narrow/wide crossover "
          f"k <= {ops.SPMM_NARROW_MAX}", flush=True)
    rows, paths = [], []
    n = args.grid * args.grid
    mats = [(f"poisson{args.grid}", lambda: poisson_2d(args.grid, args.grid))]

    def banded():
        offs = list(range(-5, 6))
        rng = np.random.default_rng(0)
        S = sp.diags([rng.random(n - abs(o)) + 1.0 for o in offs], offs,
                     shape=(n, n), format="csr")
        return lsp.csr_array(S)

    mats.append((f"banded11_{n}", banded))
    for name, make in mats:
        A = make()
        bench(name, A, args.ks, args.seconds, rows)
        if not args.no_paths:
            bench_paths(name, A, args.seconds / 2, paths)
        del A
        torch.cuda.empty_cache()
    if args.json:
        with open(args.json, "w") as f:
            json.dump({"ab": rows, "paths": paths}, f, indent=1)


if __name__ == "__main__":
    main()

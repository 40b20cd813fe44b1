#!/usr/bin/env python3
# SPDX-License-Identifier: Apache-2.0
"""Flagship benchmark: SpMV GFLOP/s (+ SpGEMM nnz/s) on 5-pt Poisson CSR.

Driver contract: ``python bench.py --gpus N --steps K --warmup W``
(multi-GPU via torch.distributed.run, one rank per GPU over RCCL).
One timed step = ``--inner`` distributed SpMVs  y = A @ x  (fp64),
including the x-halo all-gather.  Weak scaling: each GPU owns an nx*nx
block of rows (global grid nx x (N*nx)).

A plain run does only what the headline figure needs: set up, warm up,
time the steps, print the result line.  ``--full`` adds the secondary
timed sections (SpGEMM A @ A reported as nnz(C)/s, and the CG solver
pipeline) and their ``config`` entries.  ``--dump-outputs DIR`` writes
the y of the last timed SpMV to ``DIR/y.npy`` (a fixed, seeded sample
of its entries when y is large), so that two builds can be compared
output for output; x is seeded, so the inputs repeat from run to run.

Metric/config match BASELINE.json: "SpMV GFLOP/s + SpGEMM nnz/s on 5-pt
Poisson CSR", synthetic operator, fp64 (the reference's solvers run fp64).
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

# --dump-outputs budget: 2**20 float64 entries per rank (8 MiB), so that
# even an 8-rank run stays at the 64 MB ceiling for a dump
DUMP_MAX_ELEMS = 1 << 20
INPUT_SEED = 20240917


def dump_outputs(out_dir, y, rank, ws):
    """Write y (this rank's rows of the last timed SpMV) as float64 .npy.

    Up to DUMP_MAX_ELEMS entries the whole vector is written; beyond
    that, the entries at a fixed, seeded, sorted set of row indices.
    """
    import numpy as np

    os.makedirs(out_dir, exist_ok=True)
    n = y.numel()
    if n > DUMP_MAX_ELEMS:
        idx = np.sort(np.random.default_rng(INPUT_SEED).choice(
            n, size=DUMP_MAX_ELEMS, replace=False))
        y = y[torch.from_numpy(idx).to(y.device)]
    name = "y.npy" if ws <= 1 else f"y_rank{rank}.npy"
    np.save(os.path.join(out_dir, name),
            y.detach().cpu().numpy().astype(np.float64, copy=False))


def time_secondary(args, lsp, runtime, A, x, sync):
    """--full only: SpGEMM and CG timed sections -> their config entries."""
    ws = runtime.world_size
    on_gpu = torch.cuda.is_available()
    M = A.shape[0]
    nnz = A.nnz

    # ---- SpGEMM (secondary metric) ----
    sg_iters = max(args.spgemm_iters, 1)
    C = A @ A  # warmup + nnz discovery
    c_nnz = C.nnz
    del C
    sync()
    t0 = time.perf_counter()
    for _ in range(sg_iters):
        C = A @ A
        del C
    sync()
    t1 = time.perf_counter()
    sg_elapsed = t1 - t0
    if ws > 1:
        t = torch.tensor([sg_elapsed], dtype=torch.float64,
                         device=runtime.device if on_gpu else "cpu")
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        sg_elapsed = float(t.item())
    spgemm_nnz_per_s = c_nnz * sg_iters / sg_elapsed

    # ---- CG (solver pipeline: SpMV + dots + fused axpby) ----
    cg_iters = 50
    lsp.linalg.cg(A, x, rtol=0.0, maxiter=10, conv_test_iters=0)  # warmup
    sync()
    t0 = time.perf_counter()
    lsp.linalg.cg(A, x, rtol=0.0, maxiter=cg_iters, conv_test_iters=0)
    sync()
    cg_elapsed = time.perf_counter() - t0
    if ws > 1:
        t = torch.tensor([cg_elapsed], dtype=torch.float64,
                         device=runtime.device if on_gpu else "cpu")
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        cg_elapsed = float(t.item())
    cg_ms = cg_elapsed / cg_iters * 1e3

    return {
        "spgemm_nnz_per_s": round(spgemm_nnz_per_s, 1),
        "spgemm_ms_per_iter": round(sg_elapsed / sg_iters * 1e3, 3),
        "spgemm_out_nnz": c_nnz,
        "cg_ms_per_iter": round(cg_ms, 4),
        "cg_gflops": round((2 * nnz + 10 * M) / (cg_elapsed /
                                                 cg_iters) / 1e9, 1),
    }


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--gpus", type=int, default=1)
    p.add_argument("--steps", type=int, default=100)
    p.add_argument("--warmup", type=int, default=10)
    p.add_argument("--nx", type=int, default=4096,
                   help="per-GPU grid edge (rows per GPU = nx*nx)")
    p.add_argument("--spgemm-iters", type=int, default=5,
                   help="timed SpGEMM iterations (--full only)")
    p.add_argument("--inner", type=int, default=100,
                   help="SpMV iterations per timed step (a step must be "
                        "big enough that the driver's wall clock, not "
                        "launch noise, dominates)")
    p.add_argument("--full", action="store_true",
                   help="also time the secondary sections (SpGEMM, CG) "
                        "and report them under config")
    p.add_argument("--dump-outputs", metavar="DIR", default=None,
                   help="write the last timed step's y to DIR/y.npy "
                        "(float64; a seeded sample of at most "
                        f"{DUMP_MAX_ELEMS} entries per rank)")
    args = p.parse_args()

    import legate_sparse as lsp
    from legate_sparse.gallery import poisson_2d
    from legate_sparse.runtime import runtime

    rank = runtime.rank
    ws = runtime.world_size
    n_gpus = max(ws, 1)
    on_gpu = torch.cuda.is_available()
    nx = args.nx
    ny = nx * n_gpus  # weak scaling: fixed nx*nx rows per GPU

    A = poisson_2d(nx, ny)
    M = A.shape[0]
    nnz = A.nnz
    lo, hi = A.row_range
    # seeded per rank: the same arguments give the same x in every run
    torch.manual_seed(INPUT_SEED + rank)
    x = torch.rand(hi - lo, dtype=torch.float64, device=runtime.device)
    y = torch.empty_like(x)

    def sync():
        if ws > 1:
            dist.barrier()
        if on_gpu:
            torch.cuda.synchronize()

    # ---- SpMV ----
    # one bench "step" = args.inner SpMV iterations, so the timed region
    # is seconds even when the driver asks for few steps (a 20-step run
    # times 2000 SpMVs ~ 0.6 s instead of 5.8 ms)
    inner = max(args.inner, 1)
    for _ in range(min(args.warmup * inner, 2 * inner)):
        lsp.spmv(A, x, y)
    sync()
    t0 = time.perf_counter()
    for _ in range(args.steps * inner):
        lsp.spmv(A, x, y)
    sync()
    t1 = time.perf_counter()
    elapsed = t1 - t0

    # MAX over ranks of elapsed time
    if ws > 1:
        t = torch.tensor([elapsed], dtype=torch.float64,
                         device=runtime.device if on_gpu else "cpu")
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())

    ms_per_step = elapsed / args.steps * 1e3
    gflops = 2.0 * nnz * args.steps * inner / elapsed / 1e9

    if args.dump_outputs:
        dump_outputs(args.dump_outputs, y, rank, ws)

    secondary = (time_secondary(args, lsp, runtime, A, x, sync)
                 if args.full else {})

    if rank == 0:
        out = {
            "metric": "SpMV GFLOP/s on 5-pt Poisson CSR (fp64)",
            "value": round(gflops, 3),
            "unit": "GFLOP/s",
            "n_gpus": n_gpus,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": round(ms_per_step, 6),
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": None,
            "dtype": "fp64",
            "data": "synthetic 5-pt Poisson operator, random x",
            "config": {
                "model": "5-pt 2-D Poisson CSR",
                "spmv_iters_per_step": inner,
                "spmv_ms": round(ms_per_step / inner, 6),
                "grid": f"{nx}x{ny}",
                "rows": M,
                "nnz": nnz,
                "parallelism": f"row-split dp{n_gpus}, windowed halo "
                               "all-to-all + interior/halo overlap",
                **secondary,
                "device": "cuda" if on_gpu else "cpu",
            },
        }
        print(json.dumps(out))


if __name__ == "__main__":
    main()

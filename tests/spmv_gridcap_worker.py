# SPDX-License-Identifier: Apache-2.0
"""Worker of test_gpu_spmv.py::test_gpu_spmv_grid_stride_loops.

The general SpMV launcher reads LS_SPMV_GRID once per process, so the
grid-stride loops of its kernels are checked in a process of their own,
started with LS_SPMV_GRID=3: three blocks for 777 rows.  Runs every table
configuration on the ragged and the uniform L = 5 matrices (exact fill,
integer oracle), prints one ``OK <matrix> <configuration>`` line per pair
and GRIDCAP_DONE at the end; exits nonzero at the first mismatch."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np
import torch

import spmv_cases as sc
from legate_sparse import _cext, ops


def main():
    if os.environ.get("LS_SPMV_GRID") != "3":
        print("FAIL: start me with LS_SPMV_GRID=3", flush=True)
        return 1
    if not torch.cuda.is_available():
        print("FAIL: no GPU", flush=True)
        return 1
    _cext.require_hip()
    cases = [sc.get_case("ragged"), sc.uniform(5, "odd"),
             sc.uniform(5, "even")]
    for case in cases:
        ip = torch.from_numpy(case.S.indptr.astype(np.int64)).cuda()
        for cfg in sc.configs_for(case):
            for dtype in sc.REAL_DTYPES if cfg.real_only else sc.DTYPES:
                f = sc.fill(case, "exact", dtype)
                vals = torch.from_numpy(f.vals.copy()).cuda()
                x = torch.from_numpy(f.x.copy()).cuda()
                y0 = torch.from_numpy(f.y0.copy()).cuda()
                for idx in sc.IDX_DTYPES:
                    ix = torch.from_numpy(case.S.indices.astype(idx)).cuda()
                    for acc in (False, True):
                        y = y0.clone()
                        ops.spmv(ip, ix, vals, x, y, accumulate=acc,
                                 w_override=cfg.w_override, nt=cfg.nt,
                                 pair=cfg.pair, swz=cfg.swz)
                        want = sc.exact_oracle(case, f.vals, f.x, f.y0, acc)
                        try:
                            sc.check_exact(y.cpu().numpy(), want)
                        except AssertionError as e:
                            print(f"FAIL {case.name} {cfg.name} "
                                  f"{np.dtype(dtype).name} "
                                  f"{np.dtype(idx).name} acc={acc}\n{e}",
                                  flush=True)
                            return 1
            print(f"OK {case.name} {cfg.name}", flush=True)
    print("GRIDCAP_DONE", flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())

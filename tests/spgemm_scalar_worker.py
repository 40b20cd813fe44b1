# SPDX-License-Identifier: Apache-2.0
"""Worker of test_gpu_spgemm.py::test_scalar_merge_in_a_fresh_process.

The merge launcher reads LS_SPGEMM_SCALAR once per process, so the
lane-per-row scalar merge (spgemm_merge_scalar_kernel, a_len <= 8) is
checked in a process of its own, started with LS_SPGEMM_SCALAR=1.  Runs the
W = 8 entry point on every row it may take (both fills, exact layout and
COUNT into a capacity layout) and the pipeline at the three widths, for
every pair of value and index types; prints one ``OK ...`` line per check
and SCALAR_DONE at the end; exits nonzero at the first mismatch."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np
import torch

import spgemm_cases as g
import test_gpu_spgemm as t
from legate_sparse import _cext


def main():
    if os.environ.get("LS_SPGEMM_SCALAR") != "1":
        print("FAIL: start me with LS_SPGEMM_SCALAR=1", flush=True)
        return 1
    if not torch.cuda.is_available():
        print("FAIL: no GPU", flush=True)
        return 1
    ext = _cext.require_hip()
    case = g.get_case(g.N_MID)
    rows = g.eligible_rows(case, "merge", 0)
    g.assert_fits(case, "merge", 0, rows)
    for dtype, idx in t.TYPES:
        tn = f"{np.dtype(dtype).name} {np.dtype(idx).name}"
        try:
            for kind in t.KINDS:
                o = t.Operands(case, kind, dtype, idx)
                for count in (False, True):
                    t._numeric(
                        o, rows, count,
                        lambda rl, n, off, ci, cv, rn:
                        ext.spgemm_merge_numeric(
                            0, rl, n, *o.numeric_args(), off, ci, cv,
                            o.code, o.icode, rn, t._st()),
                        f"scalar merge {kind} count={count}")
                    print(f"OK direct {tn} {kind} count={count}", flush=True)
            for n_cols in g.WIDTHS:
                c = g.get_case(n_cols)
                o = t.Operands(c, "exact", dtype, idx)
                cnt = t._assert_bins(o)
                assert cnt[0] > 32
                cache = {}
                t._check_local(o, o.local(cache), "scalar first call")
                t._check_local(o, o.local(cache), "scalar cached call")
                on = t.Operands(c, "normal", dtype, idx)
                t._check_local(on, on.local(), "scalar normal fill")
                print(f"OK pipeline {tn} N={n_cols}", flush=True)
        except AssertionError as e:
            print(f"FAIL {tn}\n{e}", flush=True)
            return 1
    print("SCALAR_DONE", flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())

# SPDX-License-Identifier: Apache-2.0
"""Public namespace re-exports (reference legate_sparse/module.py:49-70)."""
from __future__ import annotations

from .coverage import track_provenance
from .csr import csr_array, csr_matrix  # noqa
from .csr import spmv as _spmv, spgemm_csr_csr_csr as _spgemm
from .csr import spmm as _spmm
from .dia import dia_array, dia_matrix  # noqa
from .gallery import diags as _diags, eye as _eye, identity as _identity
from .io import mmread as _mmread, mmwrite as _mmwrite
from .io import save_npz, load_npz  # noqa
from .types import coord_ty, nnz_ty  # noqa

# provenance labels: rocprof traces attribute kernels to these API entry
# points (the reference wraps every public name with Legate's
# track_provenance, coverage.py:87-107; enable ranges with
# utils.enable_profiler_ranges())
spmv = track_provenance(_spmv, "spmv")
spmm = track_provenance(_spmm, "spmm")
spgemm_csr_csr_csr = track_provenance(_spgemm, "spgemm_csr_csr_csr")
diags = track_provenance(_diags, "diags")
eye = track_provenance(_eye, "eye")
identity = track_provenance(_identity, "identity")
mmread = track_provenance(_mmread, "mmread")
mmwrite = track_provenance(_mmwrite, "mmwrite")


def is_sparse_matrix(o) -> bool:
    return isinstance(o, (csr_array, dia_array))


def issparse(o) -> bool:
    return is_sparse_matrix(o)


def isspmatrix(o) -> bool:
    return is_sparse_matrix(o)


def isspmatrix_csr(o) -> bool:
    return isinstance(o, csr_array)


def isspmatrix_dia(o) -> bool:
    return isinstance(o, dia_array)

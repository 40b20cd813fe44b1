// SPDX-License-Identifier: Apache-2.0
// CPU/OpenMP kernels for legate_sparse (MI355X-native framework).
//
// These are the CPU counterparts of the reference's cpu/omp task variants:
//   - CSR SpMV row loop        (reference src/sparse/array/csr/spmv.cc:36-43,
//                               spmv_omp.cc:36-45)
//   - Gustavson SpGEMM 2-phase (reference spgemm_csr_csr_csr.cc:38-160,
//                               spgemm_csr_csr_csr_omp.cc:53-167)
// re-designed: plain indptr instead of Legion pos rects, int32/int64
// indices, dense per-thread accumulators, OpenMP dynamic row scheduling.
//
// All pointers arrive as uintptr_t from torch tensors (contiguous,
// host-resident). value dtype codes: 0=f32, 1=f64, 2=c64, 3=c128;
// index dtype codes: 0=int32, 1=int64.

#include <pybind11/pybind11.h>
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <limits>
#include <complex>
#include <vector>
#include <stdexcept>

#ifdef _OPENMP
#include <omp.h>
#endif

namespace py = pybind11;

using i64 = int64_t;

template <typename T, typename I>
static void spmv_impl(const i64* indptr, const I* indices, const T* vals,
                      const T* x, T* y, i64 n_rows, bool accumulate) {
  // `if` clause: a parallel region on a tiny matrix costs more than the
  // work itself (and spins cgroup CPU quota in containers)
#pragma omp parallel for schedule(static) if (n_rows > 16384)
  for (i64 i = 0; i < n_rows; ++i) {
    T acc = accumulate ? y[i] : T(0);
    for (i64 jp = indptr[i]; jp < indptr[i + 1]; ++jp) {
      acc += vals[jp] * x[indices[jp]];
    }
    y[i] = acc;
  }
}

// CSR x dense block: Y[i, :] (+)= sum_jp vals[jp] * X[indices[jp], :],
// X and Y row-major with k columns.  Row-parallel, inner loop over k.
template <typename T, typename I>
static void spmm_impl(const i64* indptr, const I* indices, const T* vals,
                      const T* x, T* y, i64 n_rows, i64 k, bool accumulate) {
#pragma omp parallel for schedule(static) if (n_rows * k > 16384)
  for (i64 i = 0; i < n_rows; ++i) {
    T* yr = y + i * k;
    if (!accumulate) std::fill(yr, yr + k, T(0));
    for (i64 jp = indptr[i]; jp < indptr[i + 1]; ++jp) {
      const T v = vals[jp];
      const T* xr = x + (i64)indices[jp] * k;
      for (i64 q = 0; q < k; ++q) yr[q] += v * xr[q];
    }
  }
}

// Gustavson symbolic: row_nnz[i] = |union of B-row col sets over A's row i|.
template <typename I>
static void spgemm_symbolic_impl(const i64* A_indptr, const I* A_indices,
                                 i64 n_rowsA, const i64* B_indptr,
                                 const I* B_indices, i64 n_colsB,
                                 i64* row_nnz) {
#pragma omp parallel if (n_rowsA > 4096)
  {
    std::vector<i64> marker(n_colsB, -1);
#pragma omp for schedule(dynamic, 64)
    for (i64 i = 0; i < n_rowsA; ++i) {
      i64 count = 0;
      for (i64 jp = A_indptr[i]; jp < A_indptr[i + 1]; ++jp) {
        const i64 k = (i64)A_indices[jp];
        for (i64 kp = B_indptr[k]; kp < B_indptr[k + 1]; ++kp) {
          const i64 col = (i64)B_indices[kp];
          if (marker[col] != i) {
            marker[col] = i;
            ++count;
          }
        }
      }
      row_nnz[i] = count;
    }
  }
}

// Gustavson numeric: emits columns in sorted order (unlike the reference,
// which emits insertion order — spgemm_csr_csr_csr.cc:92-160; sorted output
// keeps scipy compatibility bit-clean).
template <typename T, typename I>
static void spgemm_numeric_impl(const i64* A_indptr, const I* A_indices,
                                const T* A_vals, i64 n_rowsA,
                                const i64* B_indptr, const I* B_indices,
                                const T* B_vals, i64 n_colsB,
                                const i64* C_indptr, I* C_indices,
                                T* C_vals) {
#pragma omp parallel if (n_rowsA > 4096)
  {
    std::vector<T> workspace(n_colsB, T(0));
    std::vector<i64> marker(n_colsB, -1);
    std::vector<i64> cols;
#pragma omp for schedule(dynamic, 64)
    for (i64 i = 0; i < n_rowsA; ++i) {
      cols.clear();
      for (i64 jp = A_indptr[i]; jp < A_indptr[i + 1]; ++jp) {
        const i64 k = (i64)A_indices[jp];
        const T a = A_vals[jp];
        for (i64 kp = B_indptr[k]; kp < B_indptr[k + 1]; ++kp) {
          const i64 col = (i64)B_indices[kp];
          if (marker[col] != i) {
            marker[col] = i;
            workspace[col] = a * B_vals[kp];
            cols.push_back(col);
          } else {
            workspace[col] += a * B_vals[kp];
          }
        }
      }
      std::sort(cols.begin(), cols.end());
      i64 out = C_indptr[i];
      for (i64 col : cols) {
        C_indices[out] = (I)col;
        C_vals[out] = workspace[col];
        ++out;
      }
    }
  }
}

enum DtypeCode { F32 = 0, F64 = 1, C64 = 2, C128 = 3 };

#define DISPATCH_VAL(code, CALL)                         \
  switch (code) {                                        \
    case F32: { using scalar_t = float;  CALL; break; }  \
    case F64: { using scalar_t = double; CALL; break; }  \
    case C64: { using scalar_t = std::complex<float>;  CALL; break; } \
    case C128:{ using scalar_t = std::complex<double>; CALL; break; } \
    default: throw std::runtime_error("bad dtype code");             \
  }

#define DISPATCH_IDX(code, CALL)                         \
  switch (code) {                                        \
    case 0: { using index_t = int32_t; CALL; break; }    \
    case 1: { using index_t = int64_t; CALL; break; }    \
    default: throw std::runtime_error("bad index dtype code"); \
  }

static void spmv(uintptr_t indptr, uintptr_t indices, uintptr_t vals,
                 uintptr_t x, uintptr_t y, i64 n_rows, int dtype,
                 int idx_dtype, bool accumulate) {
  DISPATCH_VAL(dtype, DISPATCH_IDX(idx_dtype, (spmv_impl<scalar_t, index_t>(
      reinterpret_cast<const i64*>(indptr),
      reinterpret_cast<const index_t*>(indices),
      reinterpret_cast<const scalar_t*>(vals),
      reinterpret_cast<const scalar_t*>(x),
      reinterpret_cast<scalar_t*>(y), n_rows, accumulate))));
}

static void spmm(uintptr_t indptr, uintptr_t indices, uintptr_t vals,
                 uintptr_t x, uintptr_t y, i64 n_rows, i64 k, int dtype,
                 int idx_dtype, bool accumulate) {
  DISPATCH_VAL(dtype, DISPATCH_IDX(idx_dtype, (spmm_impl<scalar_t, index_t>(
      reinterpret_cast<const i64*>(indptr),
      reinterpret_cast<const index_t*>(indices),
      reinterpret_cast<const scalar_t*>(vals),
      reinterpret_cast<const scalar_t*>(x),
      reinterpret_cast<scalar_t*>(y), n_rows, k, accumulate))));
}

static void spgemm_symbolic(uintptr_t A_indptr, uintptr_t A_indices,
                            i64 n_rowsA, uintptr_t B_indptr,
                            uintptr_t B_indices, i64 n_colsB,
                            uintptr_t row_nnz, int idx_dtype) {
  DISPATCH_IDX(idx_dtype, (spgemm_symbolic_impl<index_t>(
      reinterpret_cast<const i64*>(A_indptr),
      reinterpret_cast<const index_t*>(A_indices), n_rowsA,
      reinterpret_cast<const i64*>(B_indptr),
      reinterpret_cast<const index_t*>(B_indices), n_colsB,
      reinterpret_cast<i64*>(row_nnz))));
}

static void spgemm_numeric(uintptr_t A_indptr, uintptr_t A_indices,
                           uintptr_t A_vals, i64 n_rowsA, uintptr_t B_indptr,
                           uintptr_t B_indices, uintptr_t B_vals, i64 n_colsB,
                           uintptr_t C_indptr, uintptr_t C_indices,
                           uintptr_t C_vals, int dtype, int idx_dtype) {
  DISPATCH_VAL(dtype, DISPATCH_IDX(idx_dtype, (
      spgemm_numeric_impl<scalar_t, index_t>(
          reinterpret_cast<const i64*>(A_indptr),
          reinterpret_cast<const index_t*>(A_indices),
          reinterpret_cast<const scalar_t*>(A_vals), n_rowsA,
          reinterpret_cast<const i64*>(B_indptr),
          reinterpret_cast<const index_t*>(B_indices),
          reinterpret_cast<const scalar_t*>(B_vals), n_colsB,
          reinterpret_cast<const i64*>(C_indptr),
          reinterpret_cast<index_t*>(C_indices),
          reinterpret_cast<scalar_t*>(C_vals)))));
}

// ---------------------------------------------------------------------------
// Level-scheduled triangular solve / ILU(0) (docs/DESIGN.md §17)
// ---------------------------------------------------------------------------
// One sequential O(nnz) pass: level[i] = 1 + max(level[j]) over the
// off-diagonal entries of row i on the solve's side (columns below i for
// lower, above i for upper), 0 when there are none.  Columns are global:
// local column = indices - row_offset, and entries outside [0, n) are not
// dependencies.  The upper sweep walks the rows from the bottom.  Writes
// `order` (n rows sorted by level, ascending row number within a level) and
// `level_ptr` (room for n + 1 entries); returns the number of levels.
template <typename I>
static i64 level_schedule_impl(const i64* indptr, const I* indices, i64 n,
                               bool lower, i64 row_offset, i64* order,
                               i64* level_ptr) {
  std::vector<i64> level(n, 0);
  i64 n_levels = 0;
  for (i64 t = 0; t < n; ++t) {
    const i64 i = lower ? t : n - 1 - t;
    i64 lv = 0;
    for (i64 jp = indptr[i]; jp < indptr[i + 1]; ++jp) {
      const i64 j = (i64)indices[jp] - row_offset;
      if (j < 0 || j >= n) continue;
      if (lower ? j < i : j > i) lv = std::max(lv, level[j] + 1);
    }
    level[i] = lv;
    n_levels = std::max(n_levels, lv + 1);
  }
  std::fill(level_ptr, level_ptr + n_levels + 1, i64(0));
  for (i64 i = 0; i < n; ++i) ++level_ptr[level[i] + 1];
  for (i64 l = 0; l < n_levels; ++l) level_ptr[l + 1] += level_ptr[l];
  std::vector<i64> fill(level_ptr, level_ptr + n_levels);
  for (i64 i = 0; i < n; ++i) order[fill[level[i]]++] = i;
  return n_levels;
}

static i64 level_schedule(uintptr_t indptr, uintptr_t indices, i64 n,
                          bool lower, i64 row_offset, uintptr_t order,
                          uintptr_t level_ptr, int idx_dtype) {
  i64 r = 0;
  DISPATCH_IDX(idx_dtype, (r = level_schedule_impl<index_t>(
      reinterpret_cast<const i64*>(indptr),
      reinterpret_cast<const index_t*>(indices), n, lower, row_offset,
      reinterpret_cast<i64*>(order), reinterpret_cast<i64*>(level_ptr))));
  return r;
}

// In-place sweep X <- T^{-1} X over a square local CSR; X is (n, k) with
// row stride ld.  dpos[i] is the diagonal's position in row i or its
// insertion point.
template <typename T, typename I>
static void sptrsv_impl(const i64* indptr, const I* indices, const T* vals,
                        const i64* dpos, T* x, i64 ld, i64 k, i64 n,
                        bool lower, bool unit) {
  for (i64 t = 0; t < n; ++t) {
    const i64 i = lower ? t : n - 1 - t;
    const i64 d = dpos[i];
    i64 s, e;
    if (lower) {
      s = indptr[i];
      e = d;
    } else {
      e = indptr[i + 1];
      s = (d < e && (i64)indices[d] == i) ? d + 1 : d;
    }
    T* xi = x + i * ld;
    for (i64 jp = s; jp < e; ++jp) {
      const T v = vals[jp];
      const T* xr = x + (i64)indices[jp] * ld;
      for (i64 q = 0; q < k; ++q) xi[q] -= v * xr[q];
    }
    if (!unit) {
      const T dv = vals[d];
      for (i64 q = 0; q < k; ++q) xi[q] /= dv;
    }
  }
}

static void sptrsv(uintptr_t indptr, uintptr_t indices, uintptr_t vals,
                   uintptr_t dpos, uintptr_t x, i64 ld, i64 k, i64 n,
                   bool lower, bool unit, int dtype, int idx_dtype) {
  DISPATCH_VAL(dtype, DISPATCH_IDX(idx_dtype, (sptrsv_impl<scalar_t, index_t>(
      reinterpret_cast<const i64*>(indptr),
      reinterpret_cast<const index_t*>(indices),
      reinterpret_cast<const scalar_t*>(vals),
      reinterpret_cast<const i64*>(dpos), reinterpret_cast<scalar_t*>(x), ld,
      k, n, lower, unit))));
}

template <typename T>
static bool bad_pivot(const T& v) {
  return v == T(0) || !(std::abs(v) <= std::numeric_limits<double>::max());
}

// IKJ ILU(0) in place on f (A's values on entry); every diagonal is stored.
// Returns the first row whose pivot is zero or not finite, or n.
template <typename T, typename I>
static i64 ilu0_factor_impl(const i64* indptr, const I* indices, T* f,
                            const i64* dpos, i64 n) {
  i64 bad = n;
  for (i64 i = 0; i < n; ++i) {
    const i64 e = indptr[i + 1], d = dpos[i];
    for (i64 p = indptr[i]; p < d; ++p) {
      const i64 kr = (i64)indices[p];
      const T aik = f[p] / f[dpos[kr]];
      f[p] = aik;
      // merge the upper part of row kr into the rest of row i
      i64 l = p + 1;
      for (i64 q = dpos[kr] + 1; q < indptr[kr + 1] && l < e; ++q) {
        const I j = indices[q];
        while (l < e && indices[l] < j) ++l;
        if (l < e && indices[l] == j) f[l] -= aik * f[q];
      }
    }
    if (bad == n && bad_pivot(f[d])) bad = i;
  }
  return bad;
}

static i64 ilu0_factor(uintptr_t indptr, uintptr_t indices, uintptr_t f,
                       uintptr_t dpos, i64 n, int dtype, int idx_dtype) {
  i64 r = n;
  DISPATCH_VAL(dtype, DISPATCH_IDX(idx_dtype, (
      r = ilu0_factor_impl<scalar_t, index_t>(
          reinterpret_cast<const i64*>(indptr),
          reinterpret_cast<const index_t*>(indices),
          reinterpret_cast<scalar_t*>(f),
          reinterpret_cast<const i64*>(dpos), n))));
  return r;
}

// ---------------------------------------------------------------------------
// FSAI setup (docs/DESIGN.md §18)
// ---------------------------------------------------------------------------
#define LS_FSAI_MAX_ROW 32

template <typename T> struct fsai_real { using type = T; };
template <typename T> struct fsai_real<std::complex<T>> { using type = T; };
static inline float fs_conj(float v) { return v; }
static inline double fs_conj(double v) { return v; }
template <typename T>
static inline std::complex<T> fs_conj(std::complex<T> v) { return std::conj(v); }
static inline float fs_re(float v) { return v; }
static inline double fs_re(double v) { return v; }
template <typename T>
static inline T fs_re(std::complex<T> v) { return v.real(); }

// Row r of G on its sorted pattern P (m entries, the last one the diagonal
// row_lo + r): S = A[P, P] from the entries of A with col <= row (window
// rows [row_offset, row_offset + n_win)), S = C C^H, C^H w = e_m, row =
// conj(w).  The same per-row arithmetic and order as fsai.hip.  A pivot
// that is not positive and finite is replaced by 1; returns the smallest
// such local row (also for a pattern row the kernel cannot take), or
// n_local.
template <typename T, typename I>
static i64 fsai_rows_impl(const i64* p_indptr, const I* p_indices,
                          const i64* w_indptr, const I* w_indices,
                          const T* w_vals, i64 n_win, i64 row_offset,
                          i64 row_lo, i64 n_local, T* G) {
  using R = typename fsai_real<T>::type;
  constexpr int W = LS_FSAI_MAX_ROW;
  i64 first_bad = n_local;
#pragma omp parallel for schedule(dynamic, 256) reduction(min : first_bad) \
    if (n_local > 2048)
  for (i64 r = 0; r < n_local; ++r) {
    const i64 ps = p_indptr[r];
    const i64 m64 = p_indptr[r + 1] - ps;
    if (m64 < 1 || m64 > W) {
      first_bad = std::min(first_bad, r);
      continue;
    }
    const int m = (int)m64;
    T S[W * (W + 1) / 2];
    i64 P[W];
    bool bad = false;
    std::fill(S, S + m * (m + 1) / 2, T(0));
    for (int a = 0; a < m; ++a) P[a] = (i64)p_indices[ps + a];
    if (P[m - 1] != row_lo + r) bad = true;
    for (int a = 0; a < m; ++a) {
      const i64 pa = P[a], wr = pa - row_offset;
      if (wr < 0 || wr >= n_win) {
        bad = true;
        continue;
      }
      for (i64 q = w_indptr[wr]; q < w_indptr[wr + 1]; ++q) {
        const i64 c = (i64)w_indices[q];
        if (c > pa) continue;  // the upper triangle is never read
        const i64* hit = std::lower_bound(P, P + a + 1, c);
        if (hit != P + a + 1 && *hit == c)
          S[a * (a + 1) / 2 + (hit - P)] = w_vals[q];
      }
    }
    for (int k = 0; k < m; ++k) {
      const int rk = k * (k + 1) / 2;
      T skk = S[rk + k];
      for (int j = 0; j < k; ++j) skk = skk - S[rk + j] * fs_conj(S[rk + j]);
      R piv = fs_re(skk);
      if (!(piv > R(0)) || piv - piv != R(0)) {
        bad = true;
        piv = R(1);
      }
      const R d = std::sqrt(piv);
      for (int a = k + 1; a < m; ++a) {
        const int ra = a * (a + 1) / 2;
        T s = S[ra + k];
        for (int j = 0; j < k; ++j) s = s - S[ra + j] * fs_conj(S[rk + j]);
        S[ra + k] = s / d;
      }
      S[rk + k] = T(d);
    }
    T acc[W];
    std::fill(acc, acc + m, T(0));
    for (int b = m - 1; b >= 0; --b) {
      const int rb = b * (b + 1) / 2;
      const T rhs = b == m - 1 ? T(1) : T(0);
      const T wb = (rhs - acc[b]) / fs_re(S[rb + b]);
      for (int a = 0; a < b; ++a) acc[a] += fs_conj(S[rb + a]) * wb;
      G[ps + b] = fs_conj(wb);
    }
    if (bad) first_bad = std::min(first_bad, r);
  }
  return first_bad;
}

static i64 fsai_rows(uintptr_t p_indptr, uintptr_t p_indices,
                     uintptr_t w_indptr, uintptr_t w_indices,
                     uintptr_t w_vals, i64 n_win, i64 row_offset, i64 row_lo,
                     i64 n_local, uintptr_t G, int dtype, int idx_dtype) {
  i64 r = n_local;
  DISPATCH_VAL(dtype, DISPATCH_IDX(idx_dtype, (
      r = fsai_rows_impl<scalar_t, index_t>(
          reinterpret_cast<const i64*>(p_indptr),
          reinterpret_cast<const index_t*>(p_indices),
          reinterpret_cast<const i64*>(w_indptr),
          reinterpret_cast<const index_t*>(w_indices),
          reinterpret_cast<const scalar_t*>(w_vals), n_win, row_offset,
          row_lo, n_local, reinterpret_cast<scalar_t*>(G)))));
  return r;
}

PYBIND11_MODULE(_cpu_kernels, m) {
  m.def("fsai_rows", &fsai_rows);
  m.attr("FSAI_MAX_ROW") = LS_FSAI_MAX_ROW;
  m.def("level_schedule", &level_schedule);
  m.def("sptrsv", &sptrsv);
  m.def("ilu0_factor", &ilu0_factor);
  m.doc() = "legate_sparse CPU/OpenMP kernels";
  m.def("spmv", &spmv, py::arg("indptr"), py::arg("indices"), py::arg("vals"),
        py::arg("x"), py::arg("y"), py::arg("n_rows"), py::arg("dtype"),
        py::arg("idx_dtype"), py::arg("accumulate") = false);
  m.def("spmm", &spmm, py::arg("indptr"), py::arg("indices"), py::arg("vals"),
        py::arg("x"), py::arg("y"), py::arg("n_rows"), py::arg("k"),
        py::arg("dtype"), py::arg("idx_dtype"), py::arg("accumulate") = false);
  m.def("spgemm_symbolic", &spgemm_symbolic);
  m.def("spgemm_numeric", &spgemm_numeric);
#ifdef _OPENMP
  m.attr("has_openmp") = true;
#else
  m.attr("has_openmp") = false;
#endif
}

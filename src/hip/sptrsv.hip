// SPDX-License-Identifier: Apache-2.0
// Level-scheduled sparse triangular solve and ILU(0) factorisation for
// gfx950 (docs/DESIGN.md §17).
//
//   sptrsv_level / sptrsv_chain          X <- T^{-1} X, in place, T the lower
//                                        or upper triangle of a CSR matrix
//   ilu0_factor_level / ilu0_factor_chain  IKJ ILU(0) on the matrix's pattern
//
// The host sorts the rows by dependency level (`order`, `level_ptr`) and
// turns the levels into a launch plan of two kinds:
//   wide   one level, one grid-stride launch over its slice of `order`;
//   chain  a run of consecutive narrow levels, ONE workgroup that walks the
//          run with a __syncthreads() between levels.
// NO kernel here waits on another workgroup: dependencies between
// workgroups are carried only by kernel boundaries on one stream, and the
// chain loop is bounded by the level count it is given.
//
// X is a row-major (n, k) block with unit column stride and row stride
// ld >= k, 1 <= k <= LS_SPTRSV_KMAX; every offset is formed in 64 bits.
// Row i reads X[j, :] for the off-diagonal entries on the solve's side:
// [indptr[i], diag_pos[i]) for lower, (diag_pos[i], indptr[i+1]) for upper
// (diag_pos is the insertion point when the diagonal is not stored).  One
// entry point therefore serves L (unit) and U of a combined ILU(0) factor.
//
// No float atomics and a fixed summation order per row: results are
// bit-identical from run to run.

#include "common.h"
#include <climits>
#include <stdexcept>
#include <string>
#include <type_traits>

#define LS_SPTRSV_KMAX 32
// a level with at most this many rows joins a chain
#define LS_SPTRSV_CHAIN_ROWS 256
#define LS_SPTRSV_GRID_CAP 4096
// largest k of the narrow (row split over a sub-wave) mapping
#define LS_SPTRSV_NARROW_KMAX 4
// nonzeros whose loads the wide mapping issues before the first FMA
#define LS_SPTRSV_WIDE_UNROLL 4
// working-row entries an ILU(0) sub-wave of W lanes keeps in LDS: W * this
#define LS_ILU0_LDS_PER_LANE 4

namespace {

template <typename T>
__device__ inline bool ls_finite(T v) { return v - v == T(0); }
template <typename T>
__device__ inline bool ls_finite(Cplx<T> v) {
  return v.re - v.re == T(0) && v.im - v.im == T(0);
}

template <typename T, typename I>
struct TriArgs {
  const i64* indptr;
  const I* indices;
  const T* vals;
  const i64* dpos;
  const i64* order;
  T* X;  // read AND written by the same launch: never __restrict__/const
  i64 ld;
  i64 n;
  i64 nnz;
  int k;
  int lower;
  int unit;
};

// off-diagonal range [s, e) of `row` on the solve's side and the position
// d of its diagonal
template <typename T, typename I>
__device__ inline void tri_range(const TriArgs<T, I>& a, i64 row, i64& s,
                                 i64& e, i64& d) {
  LS_ASSERT_RANGE(row, a.n);
  d = a.dpos[row];
  if (a.lower) {
    s = a.indptr[row];
    e = d;
  } else {
    e = a.indptr[row + 1];
    s = d;
    if (d < e) {
      LS_ASSERT_RANGE(d, a.nnz);
      if ((i64)a.indices[d] == row) s = d + 1;
    }
  }
}

// ---------------------------------------------------------------------------
// narrow: W lanes split the row's nonzeros (rows longer than W loop), KT
// accumulators per lane, one shuffle reduction per accumulator; lane 0 of
// the sub-wave finishes the row.  k <= KT.
// ---------------------------------------------------------------------------
template <typename T, typename I, int W, int KT>
__device__ inline void tri_rows_narrow(const TriArgs<T, I>& a, i64 lo, i64 hi,
                                       i64 first, i64 stride) {
  const int lane = threadIdx.x % W;
  for (i64 idx = lo + first; idx < hi; idx += stride) {
    const i64 row = a.order[idx];
    i64 s, e, d;
    tri_range(a, row, s, e, d);
    T acc[KT];
#pragma unroll
    for (int q = 0; q < KT; ++q) acc[q] = ls_zero<T>();
    for (i64 jp = s + lane; jp < e; jp += W) {
      LS_ASSERT_RANGE(jp, a.nnz);
      const i64 c = (i64)a.indices[jp];
      LS_ASSERT_RANGE(c, a.n);
      const T v = a.vals[jp];
      const T* xr = a.X + c * a.ld;
#pragma unroll
      for (int q = 0; q < KT; ++q)
        if (q < a.k) acc[q] += v * xr[q];
    }
#pragma unroll
    for (int q = 0; q < KT; ++q) acc[q] = group_reduce_sum<T, W>(acc[q]);
    if (lane == 0) {
      T* xi = a.X + row * a.ld;
      T dv = ls_zero<T>();
      if (!a.unit) {
        LS_ASSERT_RANGE(d, a.nnz);
        dv = a.vals[d];
      }
#pragma unroll
      for (int q = 0; q < KT; ++q) {
        if (q < a.k) {
          T x = xi[q] - acc[q];
          if (!a.unit) x = x / dv;
          xi[q] = x;
        }
      }
    }
  }
}

// ---------------------------------------------------------------------------
// wide: G lanes own one row, lane = column; the group walks the row's
// nonzeros serially (index/value loads are broadcasts, X[c, :] is one
// coalesced segment) with U nonzeros' loads in flight; no reduction.
// ---------------------------------------------------------------------------
template <typename T, typename I, int G>
__device__ inline void tri_rows_wide(const TriArgs<T, I>& a, i64 lo, i64 hi,
                                     i64 first, i64 stride) {
  constexpr int U = LS_SPTRSV_WIDE_UNROLL;
  const int col = threadIdx.x % G;
  const bool on = col < a.k;
  for (i64 idx = lo + first; idx < hi; idx += stride) {
    const i64 row = a.order[idx];
    i64 s, e, d;
    tri_range(a, row, s, e, d);
    T acc = ls_zero<T>();
    i64 jp = s;
    for (; jp + U <= e; jp += U) {
      i64 c[U];
      T v[U], x[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        LS_ASSERT_RANGE(jp + u, a.nnz);
        c[u] = (i64)a.indices[jp + u];
        LS_ASSERT_RANGE(c[u], a.n);
        v[u] = a.vals[jp + u];
      }
#pragma unroll
      for (int u = 0; u < U; ++u)
        x[u] = on ? a.X[c[u] * a.ld + col] : ls_zero<T>();
#pragma unroll
      for (int u = 0; u < U; ++u) acc += v[u] * x[u];
    }
    for (; jp < e; ++jp) {
      LS_ASSERT_RANGE(jp, a.nnz);
      const i64 c = (i64)a.indices[jp];
      LS_ASSERT_RANGE(c, a.n);
      const T v = a.vals[jp];
      if (on) acc += v * a.X[c * a.ld + col];
    }
    if (on) {
      T x = a.X[row * a.ld + col] - acc;
      if (!a.unit) {
        LS_ASSERT_RANGE(d, a.nnz);
        x = x / a.vals[d];
      }
      a.X[row * a.ld + col] = x;
    }
  }
}

// NARROW: W = sub-wave width, P = KT; otherwise W = G, P unused
template <typename T, typename I, bool NARROW, int W, int P>
__device__ inline void tri_rows(const TriArgs<T, I>& a, i64 lo, i64 hi,
                                i64 first, i64 stride) {
  if constexpr (NARROW)
    tri_rows_narrow<T, I, W, P>(a, lo, hi, first, stride);
  else
    tri_rows_wide<T, I, W>(a, lo, hi, first, stride);
}

// one level: rows order[lo:hi), grid-stride over sub-wave slots
template <typename T, typename I, bool NARROW, int W, int P>
__global__ __launch_bounds__(LS_THREADS) void sptrsv_level(
    TriArgs<T, I> a, i64 lo, i64 hi) {
  constexpr int RPB = LS_THREADS / W;
  tri_rows<T, I, NARROW, W, P>(a, lo, hi,
                               (i64)blockIdx.x * RPB + threadIdx.x / W,
                               (i64)gridDim.x * RPB);
}

// levels [lv_lo, lv_hi) by ONE workgroup.  Rows of level l read X rows that
// earlier levels of this same launch stored: __syncthreads() is a
// workgroup-scope release/acquire fence around the barrier (the stores of
// every wave have left for the CU's write-through vector L1, which all
// waves of the workgroup share, before any wave passes it), and X is only
// ever accessed through plain vector loads and stores.
template <typename T, typename I, bool NARROW, int W, int P>
__global__ __launch_bounds__(LS_THREADS) void sptrsv_chain(
    TriArgs<T, I> a, const i64* __restrict__ level_ptr, i64 lv_lo,
    i64 lv_hi) {
  constexpr int RPB = LS_THREADS / W;
  for (i64 lv = lv_lo; lv < lv_hi; ++lv) {
    tri_rows<T, I, NARROW, W, P>(a, level_ptr[lv], level_ptr[lv + 1],
                                 threadIdx.x / W, RPB);
    __syncthreads();
  }
}

// ---------------------------------------------------------------------------
// ILU(0), IKJ.  One sub-wave of W lanes per row i.  For each lower entry
// (i, k) in ascending k, sequentially: a_ik /= a_kk; then the lanes run over
// the upper entries (k, j) of the FINISHED row k, find j among row i's
// later entries by binary search and subtract a_ik * a_kj.  Lanes update
// distinct positions: no atomics.
//
// The working row lives in LDS when it has at most W * LS_ILU0_LDS_PER_LANE
// entries (written back once), in global memory otherwise.  Either way a
// value one lane writes in step p is read by other lanes of the sub-wave in
// step p + 1: __threadfence_block() (workgroup-scope fence: the wave's
// outstanding LDS and global stores are waited for, and the compiler keeps
// no copy across it) sits between the steps.  The wave runs in lockstep, so
// every lane's step-p store is issued before the fence.
// ---------------------------------------------------------------------------
template <typename T, typename I>
struct IluArgs {
  const i64* indptr;
  const I* indices;
  T* F;  // factor values, A's values on entry
  const i64* dpos;
  const i64* order;
  int* flag;  // smallest row with a zero / non-finite pivot
  i64 n;
  i64 nnz;
};

template <typename T, typename I, int W>
__device__ inline void ilu0_rows(const IluArgs<T, I>& a, T* lds,
                                 i64 lo, i64 hi, i64 first, i64 stride) {
  constexpr int CAP = W * LS_ILU0_LDS_PER_LANE;
  const int lane = threadIdx.x % W;
  T* w = lds + (threadIdx.x / W) * CAP;
  for (i64 idx = lo + first; idx < hi; idx += stride) {
    const i64 row = a.order[idx];
    LS_ASSERT_RANGE(row, a.n);
    const i64 s = a.indptr[row], e = a.indptr[row + 1], d = a.dpos[row];
    LS_ASSERT_RANGE(d, a.nnz);
    const bool fits = e - s <= CAP;
    // the working row: LDS copy or the row's own slice of F
    T* wr = fits ? w : a.F + s;
    if (fits) {
      for (i64 t = lane; t < e - s; t += W) w[t] = a.F[s + t];
      __threadfence_block();
    }
    for (i64 p = s; p < d; ++p) {
      const i64 kr = (i64)a.indices[p];
      LS_ASSERT_RANGE(kr, a.n);
      const i64 kd = a.dpos[kr], ke = a.indptr[kr + 1];
      LS_ASSERT_RANGE(kd, a.nnz);
      const T aik = wr[p - s] / a.F[kd];
      if (lane == 0) wr[p - s] = aik;
      for (i64 q = kd + 1 + lane; q < ke; q += W) {
        const i64 j = (i64)a.indices[q];
        // first position in (p, e) whose column is >= j
        i64 l = p + 1, r = e;
        while (l < r) {
          const i64 m = (l + r) >> 1;
          if ((i64)a.indices[m] < j) l = m + 1; else r = m;
        }
        if (l < e && (i64)a.indices[l] == j)
          wr[l - s] = wr[l - s] - aik * a.F[q];
      }
      __threadfence_block();
    }
    const T piv = wr[d - s];
    if (fits)
      for (i64 t = lane; t < e - s; t += W) a.F[s + t] = w[t];
    if (lane == 0 && (ls_is_zero(piv) || !ls_finite(piv)))
      atomicMin(a.flag, (int)row);
    // the next row reuses w: its fill must not pass this row's reads
    __threadfence_block();
  }
}

template <typename T, typename I, int W>
__global__ __launch_bounds__(LS_THREADS) void ilu0_factor_level(
    IluArgs<T, I> a, i64 lo, i64 hi) {
  constexpr int RPB = LS_THREADS / W;
  __shared__ T lds[LS_THREADS * LS_ILU0_LDS_PER_LANE];
  ilu0_rows<T, I, W>(a, lds, lo, hi, (i64)blockIdx.x * RPB + threadIdx.x / W,
                     (i64)gridDim.x * RPB);
}

// levels [lv_lo, lv_hi) by one workgroup; F rows finished in one level are
// read by the next: the same __syncthreads() fence as in sptrsv_chain
template <typename T, typename I, int W>
__global__ __launch_bounds__(LS_THREADS) void ilu0_factor_chain(
    IluArgs<T, I> a, const i64* __restrict__ level_ptr, i64 lv_lo,
    i64 lv_hi) {
  constexpr int RPB = LS_THREADS / W;
  __shared__ T lds[LS_THREADS * LS_ILU0_LDS_PER_LANE];
  for (i64 lv = lv_lo; lv < lv_hi; ++lv) {
    ilu0_rows<T, I, W>(a, lds, level_ptr[lv], level_ptr[lv + 1],
                       threadIdx.x / W, RPB);
    __syncthreads();
  }
}

// ---------------------------------------------------------------------------
// host side: walk the launch plan.  plan holds n_launch triples
// (kind, lv_lo, lv_hi), kind 0 = wide (lv_hi == lv_lo + 1), 1 = chain;
// level_ptr_host is the host copy of level_ptr (n_levels + 1 entries).
// ---------------------------------------------------------------------------
template <typename F>
void walk_plan(const i64* level_ptr_host, i64 n_levels, const i64* plan,
               i64 n_launch, i64 n, F&& launch) {
  i64 next = 0;
  for (i64 t = 0; t < n_launch; ++t) {
    const i64 kind = plan[3 * t], l0 = plan[3 * t + 1], l1 = plan[3 * t + 2];
    if (l0 != next || l1 <= l0 || l1 > n_levels || (kind != 0 && kind != 1) ||
        (kind == 0 && l1 != l0 + 1))
      throw std::runtime_error("sptrsv: malformed launch plan");
    const i64 lo = level_ptr_host[l0], hi = level_ptr_host[l1];
    if (lo < 0 || hi < lo || hi > n)
      throw std::runtime_error("sptrsv: level_ptr out of range");
    launch(kind == 1, l0, l1, lo, hi);
    next = l1;
  }
  if (next != n_levels)
    throw std::runtime_error("sptrsv: launch plan does not cover the levels");
}

template <typename T, typename I, bool NARROW, int W, int P>
void sptrsv_run(const TriArgs<T, I>& a, const i64* level_ptr_dev,
                const i64* level_ptr_host, i64 n_levels, const i64* plan,
                i64 n_launch, int grid_cap, hipStream_t stream) {
  constexpr int RPB = LS_THREADS / W;
  walk_plan(level_ptr_host, n_levels, plan, n_launch, a.n,
            [&](bool chain, i64 l0, i64 l1, i64 lo, i64 hi) {
    if (chain) {
      hipLaunchKernelGGL((sptrsv_chain<T, I, NARROW, W, P>), dim3(1),
                         dim3(LS_THREADS), 0, stream, a, level_ptr_dev, l0,
                         l1);
    } else {
      hipLaunchKernelGGL((sptrsv_level<T, I, NARROW, W, P>),
                         dim3(grid_1d(hi - lo, RPB, grid_cap)),
                         dim3(LS_THREADS), 0, stream, a, lo, hi);
    }
  });
}

template <typename T, typename I>
void sptrsv_launch(TriArgs<T, I> a, const i64* level_ptr_dev,
                   const i64* level_ptr_host, i64 n_levels, const i64* plan,
                   i64 n_launch, int grid_cap, hipStream_t stream) {
  if (a.n <= 0) return;
#define LS_TRI_GO(NARROW, W, P)                                            \
  sptrsv_run<T, I, NARROW, W, P>(a, level_ptr_dev, level_ptr_host,         \
                                 n_levels, plan, n_launch, grid_cap, stream)
  if (a.k <= LS_SPTRSV_NARROW_KMAX) {
    // sub-wave width from the mean row length, as in spmm_launch; the
    // triangle holds about half of the row
    const double mean = 0.5 * (double)a.nnz / (double)a.n;
    const int W = mean <= 8 ? 4 : (mean <= 32 ? 16 : 64);
    if (a.k == 1) {
      if (W == 4) LS_TRI_GO(true, 4, 1);
      else if (W == 16) LS_TRI_GO(true, 16, 1);
      else LS_TRI_GO(true, 64, 1);
    } else {
      if (W == 4) LS_TRI_GO(true, 4, LS_SPTRSV_NARROW_KMAX);
      else if (W == 16) LS_TRI_GO(true, 16, LS_SPTRSV_NARROW_KMAX);
      else LS_TRI_GO(true, 64, LS_SPTRSV_NARROW_KMAX);
    }
  } else if (a.k <= 8) {
    LS_TRI_GO(false, 8, 0);
  } else if (a.k <= 16) {
    LS_TRI_GO(false, 16, 0);
  } else {
    LS_TRI_GO(false, 32, 0);
  }
#undef LS_TRI_GO
  ls_check(hipGetLastError(), "sptrsv");
}

template <typename T, typename I, int W>
void ilu0_run(const IluArgs<T, I>& a, const i64* level_ptr_dev,
              const i64* level_ptr_host, i64 n_levels, const i64* plan,
              i64 n_launch, int grid_cap, hipStream_t stream) {
  constexpr int RPB = LS_THREADS / W;
  walk_plan(level_ptr_host, n_levels, plan, n_launch, a.n,
            [&](bool chain, i64 l0, i64 l1, i64 lo, i64 hi) {
    if (chain) {
      hipLaunchKernelGGL((ilu0_factor_chain<T, I, W>), dim3(1),
                         dim3(LS_THREADS), 0, stream, a, level_ptr_dev, l0,
                         l1);
    } else {
      hipLaunchKernelGGL((ilu0_factor_level<T, I, W>),
                         dim3(grid_1d(hi - lo, RPB, grid_cap)),
                         dim3(LS_THREADS), 0, stream, a, lo, hi);
    }
  });
}

int check_cap(int grid_cap) {
  if (grid_cap == 0) return LS_SPTRSV_GRID_CAP;
  if (grid_cap < 1 || grid_cap > LS_SPTRSV_GRID_CAP)
    throw std::runtime_error("sptrsv: grid cap outside [1, " +
                             std::to_string(LS_SPTRSV_GRID_CAP) + "]");
  return grid_cap;
}

}  // namespace

int ls_sptrsv_kmax() { return LS_SPTRSV_KMAX; }
int ls_sptrsv_chain_rows() { return LS_SPTRSV_CHAIN_ROWS; }
int ls_sptrsv_grid_cap() { return LS_SPTRSV_GRID_CAP; }

// level_ptr_host and plan are HOST pointers (read before this returns);
// everything else is device memory.  grid_cap 0 means the default.
void ls_sptrsv(uintptr_t indptr, uintptr_t indices, uintptr_t vals,
               uintptr_t dpos, uintptr_t order, uintptr_t level_ptr_dev,
               uintptr_t X, i64 ld, int k, i64 n, i64 nnz,
               uintptr_t level_ptr_host, i64 n_levels, uintptr_t plan,
               i64 n_launch, bool lower, bool unit, int grid_cap, int dtype,
               int idx_dtype, uintptr_t stream) {
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  if (k < 1 || k > LS_SPTRSV_KMAX)
    throw std::runtime_error("sptrsv: column count " + std::to_string(k) +
                             " outside [1, " +
                             std::to_string(LS_SPTRSV_KMAX) + "]");
  if (ld < k || n < 0 || nnz < 0)
    throw std::runtime_error("sptrsv: bad row stride or size");
  const int cap = check_cap(grid_cap);
  DISPATCH_VAL_T(dtype, DISPATCH_IDX_T(idx_dtype, ({
    TriArgs<val_t, idx_t> a;
    a.indptr = reinterpret_cast<const i64*>(indptr);
    a.indices = reinterpret_cast<const idx_t*>(indices);
    a.vals = reinterpret_cast<const val_t*>(vals);
    a.dpos = reinterpret_cast<const i64*>(dpos);
    a.order = reinterpret_cast<const i64*>(order);
    a.X = reinterpret_cast<val_t*>(X);
    a.ld = ld;
    a.n = n;
    a.nnz = nnz;
    a.k = k;
    a.lower = lower ? 1 : 0;
    a.unit = unit ? 1 : 0;
    sptrsv_launch<val_t, idx_t>(
        a, reinterpret_cast<const i64*>(level_ptr_dev),
        reinterpret_cast<const i64*>(level_ptr_host), n_levels,
        reinterpret_cast<const i64*>(plan), n_launch, cap, s);
  })));
}

// F holds A's values on entry and the combined factor on return (strict
// lower part L without its unit diagonal, upper part U); flag is one int,
// preset by the caller to a value >= n.  wide_rows: take the 64-lane
// sub-wave (some row has more than 32 entries).
void ls_ilu0_factor(uintptr_t indptr, uintptr_t indices, uintptr_t F,
                    uintptr_t dpos, uintptr_t order, uintptr_t level_ptr_dev,
                    uintptr_t flag, i64 n, i64 nnz, uintptr_t level_ptr_host,
                    i64 n_levels, uintptr_t plan, i64 n_launch,
                    bool wide_rows, int grid_cap, int dtype, int idx_dtype,
                    uintptr_t stream) {
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  if (n < 0 || n > (i64)INT_MAX || nnz < 0)
    throw std::runtime_error("ilu0_factor: bad size");
  if (n == 0) return;
  const int cap = check_cap(grid_cap);
  DISPATCH_VAL_T(dtype, DISPATCH_IDX_T(idx_dtype, ({
    IluArgs<val_t, idx_t> a;
    a.indptr = reinterpret_cast<const i64*>(indptr);
    a.indices = reinterpret_cast<const idx_t*>(indices);
    a.F = reinterpret_cast<val_t*>(F);
    a.dpos = reinterpret_cast<const i64*>(dpos);
    a.order = reinterpret_cast<const i64*>(order);
    a.flag = reinterpret_cast<int*>(flag);
    a.n = n;
    a.nnz = nnz;
    auto lpd = reinterpret_cast<const i64*>(level_ptr_dev);
    auto lph = reinterpret_cast<const i64*>(level_ptr_host);
    auto pl = reinterpret_cast<const i64*>(plan);
    if (wide_rows)
      ilu0_run<val_t, idx_t, 64>(a, lpd, lph, n_levels, pl, n_launch, cap, s);
    else
      ilu0_run<val_t, idx_t, 8>(a, lpd, lph, n_levels, pl, n_launch, cap, s);
  })));
  ls_check(hipGetLastError(), "ilu0_factor");
}

// SPDX-License-Identifier: Apache-2.0
// Factorised sparse approximate inverse (FSAI) setup for gfx950
// (docs/DESIGN.md §18).
//
//   fsai_rows   row i of G on the sorted pattern P_i (m entries, the last
//               one i itself): S = A[P_i, P_i], S = C C^H, C^H w = e_m,
//               G[i, P_i] = conj(w), i.e. the last row of C^{-1}.
//
// One sub-wave of W lanes (8 or 32, chosen on the host from the longest
// pattern row) owns a row; rows are independent, so the grid strides over
// them and NO kernel waits on anything.  Per row:
//   1. the packed lower triangle of S (m (m + 1) / 2 entries) is zeroed in
//      LDS and P_i is staged next to it;
//   2. groups of 8 lanes walk the window rows P_i[a] of A, keep the entries
//      with column <= P_i[a], find the column in P_i[0..a] by binary search
//      and store the value at (a, slot): distinct slots, no atomics;
//   3. left-looking Cholesky in LDS, lane a owns row a of C: m steps, the
//      pivot travels by shuffle inside the sub-wave;
//   4. column-oriented back substitution, an accumulator per lane, w[b]
//      broadcast by shuffle; LDS is only read.
// Only entries of A on or below the diagonal are read.
//
// A value one lane stores in step k is read by other lanes of the sub-wave
// in step k + 1.  As in ilu0_factor_* (sptrsv.hip) the wave runs in
// lockstep and __threadfence_block() sits between the steps.  There is NO
// __syncthreads() here: rows of one workgroup have different m.  Every loop
// is bounded by m <= W or by a row length of A.  Summation order per row is
// fixed: results are bit-identical from run to run.
//
// A pivot that is not positive and finite is replaced by 1 so the row's
// control flow stays uniform, and the local row goes to `flag` through an
// integer atomicMin; so does a row whose pattern the kernel cannot take
// (length outside [1, W], last entry not the diagonal, a column outside the
// window), which the Python layer rules out before the launch.

#include "common.h"
#include <climits>
#include <stdexcept>
#include <string>
#include <type_traits>

#define LS_FSAI_MAX_ROW 32
#define LS_FSAI_NARROW 8
#define LS_FSAI_GRID_CAP 4096
// lanes that share one window row of A during the gather
#define LS_FSAI_GATHER_LANES 8

namespace {

template <typename T> struct fsai_real { using type = T; };
template <typename T> struct fsai_real<Cplx<T>> { using type = T; };

template <typename T>
__device__ inline T fs_re(T v) { return v; }
template <typename T>
__device__ inline T fs_re(Cplx<T> v) { return v.re; }

template <typename T>
__device__ inline T fs_div(T v, T d) { return v / d; }
template <typename T>
__device__ inline Cplx<T> fs_div(Cplx<T> v, T d) { return {v.re / d, v.im / d}; }

template <typename T>
__device__ inline void fs_set_real(T& v, T r) { v = r; }
template <typename T>
__device__ inline void fs_set_real(Cplx<T>& v, T r) { v.re = r; v.im = T(0); }

template <typename T, int W>
__device__ inline T fs_shfl(T v, int src) { return __shfl(v, src, W); }
template <typename T, int W>
__device__ inline Cplx<T> fs_shfl_c(Cplx<T> v, int src) {
  return {__shfl(v.re, src, W), __shfl(v.im, src, W)};
}
template <typename T, int W>
__device__ inline T fs_bcast(T v, int src) {
  if constexpr (is_cplx<T>::value)
    return fs_shfl_c<typename fsai_real<T>::type, W>(v, src);
  else
    return fs_shfl<T, W>(v, src);
}

// threads per workgroup: 16-byte values on the wide mapping take half a
// workgroup so the static LDS stays near 35 KB for every instantiation
template <typename T, int W>
struct FsaiCfg {
  static constexpr int THREADS =
      (sizeof(T) == 16 && W == LS_FSAI_MAX_ROW) ? LS_THREADS / 2 : LS_THREADS;
  static constexpr int RPB = THREADS / W;
  static constexpr int TRI = W * (W + 1) / 2;
};

template <typename T, typename I>
struct FsaiArgs {
  const i64* p_indptr;   // pattern, local rows
  const I* p_indices;    // global sorted columns, diagonal last
  const i64* w_indptr;   // window of A: rows [row_offset, row_offset + n_win)
  const I* w_indices;
  const T* w_vals;
  T* G;                  // out, pattern layout
  int* flag;
  i64 p_nnz;
  i64 n_win;
  i64 w_nnz;
  i64 row_offset;
  i64 row_lo;
  i64 n_local;
};

template <typename T, typename I, int W>
__global__ __launch_bounds__((FsaiCfg<T, W>::THREADS)) void fsai_rows_kernel(
    FsaiArgs<T, I> a) {
  using R = typename fsai_real<T>::type;
  using Cfg = FsaiCfg<T, W>;
  constexpr int SUB = LS_FSAI_GATHER_LANES;
  constexpr int NS = W / SUB;
  __shared__ T lds_s[Cfg::RPB * Cfg::TRI];
  __shared__ i64 lds_p[Cfg::RPB * W];
  const int lane = threadIdx.x % W;
  const int slot = threadIdx.x / W;
  T* S = lds_s + slot * Cfg::TRI;
  i64* P = lds_p + slot * W;
  const int ra = lane * (lane + 1) / 2;

  for (i64 r = (i64)blockIdx.x * Cfg::RPB + slot; r < a.n_local;
       r += (i64)gridDim.x * Cfg::RPB) {
    const i64 ps = a.p_indptr[r];
    const i64 m64 = a.p_indptr[r + 1] - ps;
    if (m64 < 1 || m64 > W) {  // nothing in LDS was touched
      if (lane == 0) atomicMin(a.flag, (int)r);
      continue;
    }
    const int m = (int)m64;
    bool bad = false;

    // 1. zero S, stage P
    for (int t = lane; t < m * (m + 1) / 2; t += W) S[t] = ls_zero<T>();
    if (lane < m) {
      LS_ASSERT_RANGE(ps + lane, a.p_nnz);
      P[lane] = (i64)a.p_indices[ps + lane];
    }
    __threadfence_block();
    if (P[m - 1] != a.row_lo + r) bad = true;

    // 2. gather S = A[P, P], lower triangle
    for (int aa = lane / SUB; aa < m; aa += NS) {
      const i64 pa = P[aa];
      const i64 wr = pa - a.row_offset;
      if (wr < 0 || wr >= a.n_win) {  // leaves a zero row: bad pivot
        bad = true;
        continue;
      }
      const i64 s = a.w_indptr[wr], e = a.w_indptr[wr + 1];
      for (i64 q = s + lane % SUB; q < e; q += SUB) {
        LS_ASSERT_RANGE(q, a.w_nnz);
        const i64 c = (i64)a.w_indices[q];
        if (c > pa) continue;  // the upper triangle is never read
        int l = 0, h = aa + 1;
        while (l < h) {
          const int mid = (l + h) >> 1;
          if (P[mid] < c) l = mid + 1; else h = mid;
        }
        if (l <= aa && P[l] == c) S[aa * (aa + 1) / 2 + l] = a.w_vals[q];
      }
    }
    __threadfence_block();

    // 3. S = C C^H, left-looking; lane a owns row a
    for (int k = 0; k < m; ++k) {
      const int rk = k * (k + 1) / 2;
      T s = ls_zero<T>();
      if (lane >= k && lane < m) {
        s = S[ra + k];
        for (int j = 0; j < k; ++j) s = s - S[ra + j] * ls_conj(S[rk + j]);
      }
      R piv = fs_shfl<R, W>(fs_re(s), k);
      if (!(piv > R(0)) || piv - piv != R(0)) {
        bad = true;
        piv = R(1);
      }
      const R d = sqrt(piv);
      if (lane == k) {
        fs_set_real(S[ra + k], d);
      } else if (lane > k && lane < m) {
        S[ra + k] = fs_div(s, d);
      }
      __threadfence_block();
    }

    // 4. C^H w = e_m: w[b] = (e_m[b] - sum_{c > b} conj(C[c, b]) w[c]) / C[b, b]
    T acc = ls_zero<T>();
    T wl = ls_zero<T>();
    for (int b = m - 1; b >= 0; --b) {
      const int rb = b * (b + 1) / 2;
      T wb = ls_zero<T>();
      if (lane == b) {
        T rhs = ls_zero<T>();
        if (b == m - 1) fs_set_real(rhs, R(1));
        wb = fs_div(rhs - acc, fs_re(S[rb + b]));
        wl = wb;
      }
      wb = fs_bcast<T, W>(wb, b);
      if (lane < b) acc += ls_conj(S[rb + lane]) * wb;
    }
    if (lane < m) a.G[ps + lane] = ls_conj(wl);
    // any lane may have seen a bad column; the pivot test is uniform
    if (bad) atomicMin(a.flag, (int)r);
    // the next row reuses S and P: its fill must not pass this row's reads
    __threadfence_block();
  }
}

template <typename T, typename I, int W>
void fsai_launch(const FsaiArgs<T, I>& a, int grid_cap, hipStream_t stream) {
  using Cfg = FsaiCfg<T, W>;
  hipLaunchKernelGGL((fsai_rows_kernel<T, I, W>),
                     dim3(grid_1d(a.n_local, Cfg::RPB, grid_cap)),
                     dim3(Cfg::THREADS), 0, stream, a);
}

}  // namespace

int ls_fsai_max_row() { return LS_FSAI_MAX_ROW; }
int ls_fsai_narrow() { return LS_FSAI_NARROW; }
int ls_fsai_grid_cap() { return LS_FSAI_GRID_CAP; }

// All pointers are device memory.  flag is one int, preset by the caller to
// a value >= n_local.  max_row is the longest pattern row (picks the
// sub-wave width); grid_cap 0 means the default.
void ls_fsai_rows(uintptr_t p_indptr, uintptr_t p_indices, i64 p_nnz,
                  uintptr_t w_indptr, uintptr_t w_indices, uintptr_t w_vals,
                  i64 n_win, i64 w_nnz, i64 row_offset, i64 row_lo,
                  i64 n_local, uintptr_t G, uintptr_t flag, int max_row,
                  int grid_cap, int dtype, int idx_dtype, uintptr_t stream) {
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  if (n_local < 0 || n_local > (i64)INT_MAX || p_nnz < 0 || n_win < 0 ||
      w_nnz < 0)
    throw std::runtime_error("fsai_rows: bad size");
  if (max_row < 1 || max_row > LS_FSAI_MAX_ROW)
    throw std::runtime_error("fsai_rows: longest row " +
                             std::to_string(max_row) + " outside [1, " +
                             std::to_string(LS_FSAI_MAX_ROW) + "]");
  if (grid_cap == 0) grid_cap = LS_FSAI_GRID_CAP;
  if (grid_cap < 1 || grid_cap > LS_FSAI_GRID_CAP)
    throw std::runtime_error("fsai_rows: grid cap outside [1, " +
                             std::to_string(LS_FSAI_GRID_CAP) + "]");
  if (n_local == 0) return;
  DISPATCH_VAL_T(dtype, DISPATCH_IDX_T(idx_dtype, ({
    FsaiArgs<val_t, idx_t> a;
    a.p_indptr = reinterpret_cast<const i64*>(p_indptr);
    a.p_indices = reinterpret_cast<const idx_t*>(p_indices);
    a.w_indptr = reinterpret_cast<const i64*>(w_indptr);
    a.w_indices = reinterpret_cast<const idx_t*>(w_indices);
    a.w_vals = reinterpret_cast<const val_t*>(w_vals);
    a.G = reinterpret_cast<val_t*>(G);
    a.flag = reinterpret_cast<int*>(flag);
    a.p_nnz = p_nnz;
    a.n_win = n_win;
    a.w_nnz = w_nnz;
    a.row_offset = row_offset;
    a.row_lo = row_lo;
    a.n_local = n_local;
    if (max_row <= LS_FSAI_NARROW)
      fsai_launch<val_t, idx_t, LS_FSAI_NARROW>(a, grid_cap, s);
    else
      fsai_launch<val_t, idx_t, LS_FSAI_MAX_ROW>(a, grid_cap, s);
  })));
  ls_check(hipGetLastError(), "fsai_rows");
}

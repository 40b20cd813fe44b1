// SPDX-License-Identifier: Apache-2.0
// CSR x dense multi-vector product (SpMM) for gfx950.
//
// Semantics: Y[i, :] (+)= sum_jp vals[jp] * X[indices[jp], :] over local
// rows, X and Y row-major with k columns.  The matrix is streamed ONCE for
// all k right-hand sides (k SpMV calls stream it k times).
//
// Two lane mappings, because the two ends of k want opposite ones:
//   narrow (k <= LS_SPMM_NARROW_KMAX, K a template parameter): the row's
//     nonzeros are split over a sub-wave of W lanes exactly like
//     spmv_vector_kernel; each lane keeps K accumulators and reads the K
//     contiguous entries of X[c, :]; one sub-wave reduction per accumulator.
//   wide (any k): G lanes own one row x one column tile, each lane V
//     adjacent columns (V * sizeof(T) = 16 B).  The group walks the row's
//     nonzeros serially: vals/indices are broadcast loads, X[c, tile] is
//     one coalesced segment, and there is no reduction at all.
//
// 16-byte accesses are legal only when the X and Y base pointers (X after
// the col_offset adjustment) and the row stride k*sizeof(T) are 16-byte
// multiples; the host decides that once (template parameter VEC) and the
// element-wise instantiation runs otherwise.
//
// No atomics, no cross-wave reductions: results are bit-identical from run
// to run.  Every X/Y offset (c*k, row*k) is formed in 64 bits.

#include "common.h"
#include <stdexcept>
#include <string>
#include <type_traits>

// largest k the narrow kernel is instantiated for
#define LS_SPMM_NARROW_KMAX 8
// nonzeros whose loads the wide kernel issues before the first FMA
#define LS_SPMM_WIDE_UNROLL 4

namespace {

template <typename T> struct real_of { using type = T; };
template <typename T> struct real_of<Cplx<T>> { using type = T; };

// 16-byte vector of the value type's underlying real
template <typename T>
using vec16_t = __attribute__((ext_vector_type(
    16 / sizeof(typename real_of<T>::type)))) typename real_of<T>::type;

// N contiguous elements; VEC: p is 16-B aligned and N*sizeof(T) % 16 == 0
template <typename T, int N, bool VEC>
__device__ inline void load_elems(const T* __restrict__ p, T (&out)[N]) {
  if constexpr (VEC) {
    static_assert((N * sizeof(T)) % 16 == 0, "row is not a 16-B multiple");
    constexpr int NV = N * sizeof(T) / 16;
    vec16_t<T> tmp[NV];
#pragma unroll
    for (int i = 0; i < NV; ++i)
      tmp[i] = reinterpret_cast<const vec16_t<T>*>(p)[i];
    __builtin_memcpy(out, tmp, sizeof(tmp));
  } else {
#pragma unroll
    for (int q = 0; q < N; ++q) out[q] = p[q];
  }
}

template <typename T, int N, bool VEC>
__device__ inline void store_elems(T* __restrict__ p, const T (&in)[N]) {
  if constexpr (VEC) {
    constexpr int NV = N * sizeof(T) / 16;
    vec16_t<T> tmp[NV];
    __builtin_memcpy(tmp, in, sizeof(tmp));
#pragma unroll
    for (int i = 0; i < NV; ++i)
      reinterpret_cast<vec16_t<T>*>(p)[i] = tmp[i];
  } else {
#pragma unroll
    for (int q = 0; q < N; ++q) p[q] = in[q];
  }
}

// ---------------------------------------------------------------------------
// narrow: W lanes split the row's nonzeros, K accumulators per lane
// ---------------------------------------------------------------------------
template <typename T, typename I, int W, int K, bool VEC>
__global__ __launch_bounds__(LS_THREADS) void spmm_narrow_kernel(
    const i64* __restrict__ indptr, const I* __restrict__ indices,
    const T* __restrict__ vals, const T* __restrict__ X, T* __restrict__ Y,
    i64 n_rows, i64 c_lo, i64 c_n, int accumulate) {
  constexpr int ROWS_PER_BLOCK = LS_THREADS / W;
  const int group = threadIdx.x / W;
  const int lane = threadIdx.x % W;
  const i64 stride = (i64)gridDim.x * ROWS_PER_BLOCK;
  for (i64 row = (i64)blockIdx.x * ROWS_PER_BLOCK + group; row < n_rows;
       row += stride) {
    const i64 s = indptr[row];
    const i64 e = indptr[row + 1];
    T acc[K];
#pragma unroll
    for (int q = 0; q < K; ++q) acc[q] = ls_zero<T>();
    for (i64 jp = s + lane; jp < e; jp += W) {
      const i64 c = (i64)indices[jp];
      LS_ASSERT_RANGE(c - c_lo, c_n);
      const T v = vals[jp];
      T xr[K];
      load_elems<T, K, VEC>(X + c * (i64)K, xr);
#pragma unroll
      for (int q = 0; q < K; ++q) acc[q] += v * xr[q];
    }
#pragma unroll
    for (int q = 0; q < K; ++q) acc[q] = group_reduce_sum<T, W>(acc[q]);
    if (lane == 0) {
      T* yr = Y + row * (i64)K;
      if (accumulate) {
        T old[K];
        load_elems<T, K, VEC>(yr, old);
#pragma unroll
        for (int q = 0; q < K; ++q) acc[q] += old[q];
      }
      store_elems<T, K, VEC>(yr, acc);
    }
  }
}

// ---------------------------------------------------------------------------
// wide: G lanes own (row, column tile); lane owns V adjacent columns
// ---------------------------------------------------------------------------
template <typename T, typename I, int G, bool VEC>
__global__ __launch_bounds__(LS_THREADS) void spmm_wide_kernel(
    const i64* __restrict__ indptr, const I* __restrict__ indices,
    const T* __restrict__ vals, const T* __restrict__ X, T* __restrict__ Y,
    i64 n_rows, i64 k, i64 n_tiles, i64 c_lo, i64 c_n, int accumulate) {
  constexpr int V = 16 / sizeof(T);
  constexpr int U = LS_SPMM_WIDE_UNROLL;
  constexpr int ROWS_PER_BLOCK = LS_THREADS / G;
  const int group = threadIdx.x / G;
  const int lane = threadIdx.x % G;
  const i64 stride = (i64)gridDim.x * ROWS_PER_BLOCK;
  for (i64 tile = blockIdx.y; tile < n_tiles; tile += gridDim.y) {
    const i64 col0 = (tile * G + lane) * V;
    // VEC implies k % V == 0: a lane's V columns are all in or all out;
    // the element-wise path guards every tail column by itself
    if (col0 >= k) continue;
    int nv = V;
    if constexpr (!VEC) nv = (k - col0 < V) ? (int)(k - col0) : V;
    for (i64 row = (i64)blockIdx.x * ROWS_PER_BLOCK + group; row < n_rows;
         row += stride) {
      const i64 s = indptr[row];
      const i64 e = indptr[row + 1];
      T acc[V];
#pragma unroll
      for (int q = 0; q < V; ++q) acc[q] = ls_zero<T>();
      i64 jp = s;
      for (; jp + U <= e; jp += U) {
        // all index/value loads, then all X-row loads, then the FMAs
        i64 c[U];
        T v[U];
        T xr[U][V];
#pragma unroll
        for (int u = 0; u < U; ++u) {
          c[u] = (i64)indices[jp + u];
          LS_ASSERT_RANGE(c[u] - c_lo, c_n);
          v[u] = vals[jp + u];
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
          const T* xp = X + c[u] * k + col0;
          if constexpr (VEC) {
            load_elems<T, V, true>(xp, xr[u]);
          } else {
#pragma unroll
            for (int q = 0; q < V; ++q)
              xr[u][q] = q < nv ? xp[q] : ls_zero<T>();
          }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
#pragma unroll
          for (int q = 0; q < V; ++q) acc[q] += v[u] * xr[u][q];
        }
      }
      for (; jp < e; ++jp) {
        const i64 c = (i64)indices[jp];
        LS_ASSERT_RANGE(c - c_lo, c_n);
        const T v = vals[jp];
        const T* xp = X + c * k + col0;
        T xr[V];
        if constexpr (VEC) {
          load_elems<T, V, true>(xp, xr);
        } else {
#pragma unroll
          for (int q = 0; q < V; ++q) xr[q] = q < nv ? xp[q] : ls_zero<T>();
        }
#pragma unroll
        for (int q = 0; q < V; ++q) acc[q] += v * xr[q];
      }
      T* yp = Y + row * k + col0;
      if constexpr (VEC) {
        if (accumulate) {
          T old[V];
          load_elems<T, V, true>(yp, old);
#pragma unroll
          for (int q = 0; q < V; ++q) acc[q] += old[q];
        }
        store_elems<T, V, true>(yp, acc);
      } else {
#pragma unroll
        for (int q = 0; q < V; ++q) {
          if (q < nv) {
            if (accumulate)
              yp[q] += acc[q];
            else
              yp[q] = acc[q];
          }
        }
      }
    }
  }
}

template <int N>
using int_c = std::integral_constant<int, N>;

template <typename F>
void dispatch_pow2(int w, F&& f) {
  switch (w) {
    case 1: f(int_c<1>{}); break;
    case 2: f(int_c<2>{}); break;
    case 4: f(int_c<4>{}); break;
    case 8: f(int_c<8>{}); break;
    case 16: f(int_c<16>{}); break;
    case 32: f(int_c<32>{}); break;
    case 64: f(int_c<64>{}); break;
    default: throw std::runtime_error("spmm: bad sub-wave width");
  }
}

template <typename T, typename I>
void spmm_launch(const i64* indptr, const I* indices, const T* vals,
                 const T* X, T* Y, i64 n_rows, i64 nnz, i64 k, i64 c_lo,
                 i64 c_n, bool accumulate, int path, hipStream_t stream) {
  if (n_rows <= 0 || k <= 0) return;
  // the 16-byte path needs both (adjusted) bases and the row stride
  // 16-byte aligned; decided here once, never per element
  const bool vec =
      ((reinterpret_cast<uintptr_t>(X) | reinterpret_cast<uintptr_t>(Y)) %
           16 == 0) &&
      ((k * (i64)sizeof(T)) % 16 == 0);
  const int acc = accumulate ? 1 : 0;
  constexpr int GRID_CAP = 8192;
  if (path == 0) {
    if (k > LS_SPMM_NARROW_KMAX)
      throw std::runtime_error("spmm: k exceeds the narrow kernel's limit");
    // W as in spmv_launch: largest power of two <= mean/2
    const double mean = (double)nnz / (double)n_rows;
    int W = 1;
    while (W < 64 && (double)(W * 4) <= mean) W *= 2;
    dispatch_pow2(W, [&](auto wtag) {
      constexpr int WS = decltype(wtag)::value;
      const int grid = grid_1d(n_rows, LS_THREADS / WS, GRID_CAP);
      auto go = [&](auto ktag) {
        constexpr int K = decltype(ktag)::value;
        if constexpr ((K * sizeof(T)) % 16 == 0) {
          if (vec) {
            hipLaunchKernelGGL((spmm_narrow_kernel<T, I, WS, K, true>),
                               dim3(grid), dim3(LS_THREADS), 0, stream,
                               indptr, indices, vals, X, Y, n_rows, c_lo,
                               c_n, acc);
            return;
          }
        }
        hipLaunchKernelGGL((spmm_narrow_kernel<T, I, WS, K, false>),
                           dim3(grid), dim3(LS_THREADS), 0, stream, indptr,
                           indices, vals, X, Y, n_rows, c_lo, c_n, acc);
      };
      static_assert(LS_SPMM_NARROW_KMAX == 8, "extend the K switch");
      switch ((int)k) {
        case 1: go(int_c<1>{}); break;
        case 2: go(int_c<2>{}); break;
        case 3: go(int_c<3>{}); break;
        case 4: go(int_c<4>{}); break;
        case 5: go(int_c<5>{}); break;
        case 6: go(int_c<6>{}); break;
        case 7: go(int_c<7>{}); break;
        default: go(int_c<8>{}); break;
      }
    });
    ls_check(hipGetLastError(), "spmm_narrow");
    return;
  }
  if (path != 1) throw std::runtime_error("spmm: bad path code");
  // G = smallest power of two whose tile (G*V columns) covers k, so a
  // short k does not idle most of a wave; k beyond 64*V takes more tiles
  constexpr int V = 16 / sizeof(T);
  int G = 1;
  while (G < 64 && (i64)G * V < k) G *= 2;
  const i64 n_tiles = (k + (i64)G * V - 1) / ((i64)G * V);
  const unsigned grid_y = (unsigned)(n_tiles < 65535 ? n_tiles : 65535);
  dispatch_pow2(G, [&](auto gtag) {
    constexpr int GS = decltype(gtag)::value;
    const int grid = grid_1d(n_rows, LS_THREADS / GS, GRID_CAP);
    if (vec)
      hipLaunchKernelGGL((spmm_wide_kernel<T, I, GS, true>),
                         dim3(grid, grid_y), dim3(LS_THREADS), 0, stream,
                         indptr, indices, vals, X, Y, n_rows, k, n_tiles,
                         c_lo, c_n, acc);
    else
      hipLaunchKernelGGL((spmm_wide_kernel<T, I, GS, false>),
                         dim3(grid, grid_y), dim3(LS_THREADS), 0, stream,
                         indptr, indices, vals, X, Y, n_rows, k, n_tiles,
                         c_lo, c_n, acc);
  });
  ls_check(hipGetLastError(), "spmm_wide");
}

}  // namespace

int ls_spmm_narrow_kmax() { return LS_SPMM_NARROW_KMAX; }

// X is the base pointer ALREADY adjusted by -col_offset*k elements; valid
// gathered columns are [c_lo, c_lo + c_n) (checked in LS_DEBUG builds).
// path: 0 = narrow, 1 = wide.
void ls_spmm(uintptr_t indptr, uintptr_t indices, uintptr_t vals,
             uintptr_t X, uintptr_t Y, i64 n_rows, i64 nnz, i64 k, i64 c_lo,
             i64 c_n, int dtype, int idx_dtype, bool accumulate, int path,
             uintptr_t stream) {
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  DISPATCH_VAL_T(dtype, DISPATCH_IDX_T(idx_dtype, (
      spmm_launch<val_t, idx_t>(
          reinterpret_cast<const i64*>(indptr),
          reinterpret_cast<const idx_t*>(indices),
          reinterpret_cast<const val_t*>(vals),
          reinterpret_cast<const val_t*>(X), reinterpret_cast<val_t*>(Y),
          n_rows, nnz, k, c_lo, c_n, accumulate, path, s))));
}

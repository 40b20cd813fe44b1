// SPDX-License-Identifier: Apache-2.0
// CSR SpMV for gfx950 — the hot kernel of the framework.
//
// Semantics: y[i] (+)= sum_jp vals[jp] * x[indices[jp]] over local rows
// (the reference computes this through cuSPARSE on a localized CSR,
// spmv.cu:62-157; here it is a hand-written CDNA4 kernel).
//
// Strategy: "vector CSR" — a power-of-two sub-wave of W lanes per row.
// fp64 CSR SpMV streams 12-16 B/nnz and issues 3 loads per element
// (val, idx, x-gather), so it can be VMEM-ISSUE-bound before it is
// bandwidth-bound.  Design choices, each measured
// (profiles/spmv_sweep_r01.txt and successors):
//   - int32 column indices when the matrix allows (DISPATCH_IDX_T)
//   - PAIR variant: each lane owns 2 consecutive elements loaded as one
//     16-B val vector + one 8-B idx vector from an even-aligned base —
//     4 VMEM instructions per 2 elements instead of 6
//   - plain (cached) loads: nt measured 25-40% slower here
//   - W = largest pow2 <= mean/2 (2 elements per lane)
//   - optional XCD-aware bijective block remap: contiguous row chunks
//     per XCD L2 (x reuse between neighboring rows)

#include "common.h"
#include <cstdlib>
#include <stdexcept>
#include <string>

namespace {

template <typename T>
__device__ inline T nt_load(const T* p) {
  return __builtin_nontemporal_load(p);
}
template <typename T>
__device__ inline Cplx<T> nt_load(const Cplx<T>* p) {
  return {__builtin_nontemporal_load(&p->re),
          __builtin_nontemporal_load(&p->im)};
}

__device__ inline void dot_atomic_add(float* p, float v) {
  atomicAdd(p, v);
}
__device__ inline void dot_atomic_add(double* p, double v) {
  atomicAdd(p, v);
}
template <typename T>
__device__ inline void dot_atomic_add(Cplx<T>* p, Cplx<T> v) {
  atomicAdd(&p->re, v.re);
  atomicAdd(&p->im, v.im);
}

__device__ inline int xcd_swizzle(int b, int nwg) {
  // bijective remap: XCD (= b % 8 by observed dispatch) gets a contiguous
  // chunk of the grid (cdna_hip_programming.md T1, bijective variant)
  const int q = nwg >> 3, r = nwg & 7;
  const int xcd = b & 7, pos = b >> 3;
  return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + pos;
}

template <typename T, typename I, int W, bool NT, bool SWZ>
__global__ __launch_bounds__(LS_THREADS) void spmv_vector_kernel(
    const i64* __restrict__ indptr, const I* __restrict__ indices,
    const T* __restrict__ vals, const T* __restrict__ x, T* __restrict__ y,
    i64 n_rows, int accumulate) {
  constexpr int ROWS_PER_BLOCK = LS_THREADS / W;
  const int group = threadIdx.x / W;
  const int lane = threadIdx.x % W;
  const int blk = SWZ ? xcd_swizzle(blockIdx.x, gridDim.x) : blockIdx.x;
  const i64 stride = (i64)gridDim.x * ROWS_PER_BLOCK;
  for (i64 row = (i64)blk * ROWS_PER_BLOCK + group; row < n_rows;
       row += stride) {
    const i64 s = indptr[row];
    const i64 e = indptr[row + 1];
    T acc = ls_zero<T>();
    for (i64 jp = s + lane; jp < e; jp += W) {
      LS_ASSERT_RANGE(indices[jp], (i64)1 << 62);
      if constexpr (NT)
        acc += nt_load(vals + jp) * x[nt_load(indices + jp)];
      else
        acc += vals[jp] * x[indices[jp]];
    }
    acc = group_reduce_sum<T, W>(acc);
    if (lane == 0) {
      if (accumulate)
        y[row] += acc;
      else
        y[row] = acc;
    }
  }
}

// PAIR variant (real dtypes): 2 consecutive elements per lane per step,
// loaded as vectors from an even (16-B for f64) aligned base — halves the
// VMEM instruction count on the vals/indices streams.
template <typename T, typename I, int W, bool SWZ>
__global__ __launch_bounds__(LS_THREADS) void spmv_pair_kernel(
    const i64* __restrict__ indptr, const I* __restrict__ indices,
    const T* __restrict__ vals, const T* __restrict__ x, T* __restrict__ y,
    i64 n_rows, i64 nnz, int accumulate) {
  using T2 = __attribute__((ext_vector_type(2))) T;
  using I2 = __attribute__((ext_vector_type(2))) I;
  constexpr int ROWS_PER_BLOCK = LS_THREADS / W;
  const int group = threadIdx.x / W;
  const int lane = threadIdx.x % W;
  const int blk = SWZ ? xcd_swizzle(blockIdx.x, gridDim.x) : blockIdx.x;
  const i64 stride = (i64)gridDim.x * ROWS_PER_BLOCK;
  for (i64 row = (i64)blk * ROWS_PER_BLOCK + group; row < n_rows;
       row += stride) {
    const i64 s = indptr[row];
    const i64 e = indptr[row + 1];
    const i64 s2 = s & ~(i64)1;  // aligned pair base (never < 0)
    T acc = ls_zero<T>();
    for (i64 pp = s2 + 2 * lane; pp < e; pp += 2 * W) {
      T2 v;
      I2 c;
      if (pp + 2 <= nnz) {  // odd global tail: vector load would read past
        v = *reinterpret_cast<const T2*>(vals + pp);
        c = *reinterpret_cast<const I2*>(indices + pp);
      } else {
        v.x = vals[pp];
        c.x = indices[pp];
      }
      if (pp >= s) acc += v.x * x[c.x];
      if (pp + 1 < e) acc += v.y * x[c.y];
    }
    acc = group_reduce_sum<T, W>(acc);
    if (lane == 0) {
      if (accumulate)
        y[row] += acc;
      else
        y[row] = acc;
    }
  }
}

// STENCIL variant for uniformly short rows (max nnz/row <= 2*NP-1):
// one lane per row, ALL pair loads issued unrolled before any use —
// maximum per-lane memory-level parallelism, no sub-wave reduce.
template <typename T, typename I, int NP>
__global__ __launch_bounds__(LS_THREADS) void spmv_sten_kernel(
    const i64* __restrict__ indptr, const I* __restrict__ indices,
    const T* __restrict__ vals, const T* __restrict__ x, T* __restrict__ y,
    i64 n_rows, i64 nnz, int accumulate) {
  using T2 = __attribute__((ext_vector_type(2))) T;
  using I2 = __attribute__((ext_vector_type(2))) I;
  const i64 stride = (i64)gridDim.x * blockDim.x;
  for (i64 row = (i64)blockIdx.x * blockDim.x + threadIdx.x; row < n_rows;
       row += stride) {
    const i64 s = indptr[row];
    const i64 e = indptr[row + 1];
    const i64 s2 = s & ~(i64)1;
    T2 v[NP];
    I2 c[NP];
#pragma unroll
    for (int p = 0; p < NP; ++p) {
      const i64 pp = s2 + 2 * p;
      if (pp < e) {
        if (pp + 2 <= nnz) {
          v[p] = *reinterpret_cast<const T2*>(vals + pp);
          c[p] = *reinterpret_cast<const I2*>(indices + pp);
        } else {  // odd global tail: scalar load, .y unused
          v[p].x = vals[pp];
          c[p].x = indices[pp];
        }
      }
    }
    T acc = ls_zero<T>();
#pragma unroll
    for (int p = 0; p < NP; ++p) {
      const i64 pp = s2 + 2 * p;
      if (pp >= s && pp < e) acc += v[p].x * x[c[p].x];
      if (pp + 1 >= s && pp + 1 < e) acc += v[p].y * x[c[p].y];
    }
    if (accumulate)
      y[row] += acc;
    else
      y[row] = acc;
  }
}

// PAIRU variant: W lanes per row, each lane's PPL pairs fully unrolled
// (coverage: max nnz + 1 <= 2*W*PPL).  Generalizes the stencil kernel
// to wider rows while keeping every load issued before any use.
template <typename T, typename I, int W, int PPL>
__global__ __launch_bounds__(LS_THREADS) void spmv_pairu_kernel(
    const i64* __restrict__ indptr, const I* __restrict__ indices,
    const T* __restrict__ vals, const T* __restrict__ x, T* __restrict__ y,
    i64 n_rows, i64 nnz, int accumulate) {
  using T2 = __attribute__((ext_vector_type(2))) T;
  using I2 = __attribute__((ext_vector_type(2))) I;
  constexpr int RPB = LS_THREADS / W;
  const int group = threadIdx.x / W;
  const int lane = threadIdx.x % W;
  const i64 stride = (i64)gridDim.x * RPB;
  for (i64 row = (i64)blockIdx.x * RPB + group; row < n_rows;
       row += stride) {
    const i64 s = indptr[row];
    const i64 e = indptr[row + 1];
    const i64 s2 = s & ~(i64)1;
    T2 v[PPL];
    I2 c[PPL];
#pragma unroll
    for (int k = 0; k < PPL; ++k) {
      const i64 pp = s2 + 2 * (lane + k * W);
      if (pp < e) {
        if (pp + 2 <= nnz) {
          v[k] = *reinterpret_cast<const T2*>(vals + pp);
          c[k] = *reinterpret_cast<const I2*>(indices + pp);
        } else {  // odd global tail
          v[k].x = vals[pp];
          c[k].x = indices[pp];
        }
      }
    }
    T acc = ls_zero<T>();
#pragma unroll
    for (int k = 0; k < PPL; ++k) {
      const i64 pp = s2 + 2 * (lane + k * W);
      if (pp >= s && pp < e) acc += v[k].x * x[c[k].x];
      if (pp + 1 >= s && pp + 1 < e) acc += v[k].y * x[c[k].y];
    }
    acc = group_reduce_sum<T, W>(acc);
    if (lane == 0) {
      if (accumulate)
        y[row] += acc;
      else
        y[row] = acc;
    }
  }
}

// PAIR2 variant: each W-lane group serves TWO ADJACENT rows per step,
// interleaving their pair loads — 94.5% of the PAIR kernel's wave
// cycles are parked on memory waits (SQ_WAIT_ANY), so doubling the
// independent load chains per lane raises memory-level parallelism.
template <typename T, typename I, int W, bool SWZ>
__global__ __launch_bounds__(LS_THREADS) void spmv_pair2_kernel(
    const i64* __restrict__ indptr, const I* __restrict__ indices,
    const T* __restrict__ vals, const T* __restrict__ x, T* __restrict__ y,
    i64 n_rows, i64 nnz, int accumulate) {
  using T2 = __attribute__((ext_vector_type(2))) T;
  using I2 = __attribute__((ext_vector_type(2))) I;
  constexpr int GROUPS = LS_THREADS / W;
  const int group = threadIdx.x / W;
  const int lane = threadIdx.x % W;
  const int blk = SWZ ? xcd_swizzle(blockIdx.x, gridDim.x) : blockIdx.x;
  const i64 stride = (i64)gridDim.x * GROUPS * 2;
  for (i64 row = ((i64)blk * GROUPS + group) * 2; row < n_rows;
       row += stride) {
    const bool has2 = row + 1 < n_rows;
    const i64 s1 = indptr[row];
    const i64 e1 = indptr[row + 1];
    const i64 s2 = has2 ? e1 : 0;
    const i64 e2 = has2 ? indptr[row + 2] : 0;
    const i64 b1 = s1 & ~(i64)1;
    const i64 b2 = s2 & ~(i64)1;
    T acc1 = ls_zero<T>();
    T acc2 = ls_zero<T>();
    i64 p1 = b1 + 2 * lane;
    i64 p2 = b2 + 2 * lane;
    while (p1 < e1 || p2 < e2) {
      // issue both rows' loads before either use
      T2 v1, v2;
      I2 c1, c2;
      const bool g1 = p1 < e1;
      const bool g2 = p2 < e2;
      if (g1) {
        if (p1 + 2 <= nnz) {
          v1 = *reinterpret_cast<const T2*>(vals + p1);
          c1 = *reinterpret_cast<const I2*>(indices + p1);
        } else {  // odd global tail
          v1.x = vals[p1];
          c1.x = indices[p1];
        }
      }
      if (g2) {
        if (p2 + 2 <= nnz) {
          v2 = *reinterpret_cast<const T2*>(vals + p2);
          c2 = *reinterpret_cast<const I2*>(indices + p2);
        } else {
          v2.x = vals[p2];
          c2.x = indices[p2];
        }
      }
      if (g1) {
        if (p1 >= s1) acc1 += v1.x * x[c1.x];
        if (p1 + 1 < e1) acc1 += v1.y * x[c1.y];
        p1 += 2 * W;
      }
      if (g2) {
        if (p2 >= s2) acc2 += v2.x * x[c2.x];
        if (p2 + 1 < e2) acc2 += v2.y * x[c2.y];
        p2 += 2 * W;
      }
    }
    acc1 = group_reduce_sum<T, W>(acc1);
    acc2 = group_reduce_sum<T, W>(acc2);
    if (lane == 0) {
      if (accumulate) {
        y[row] += acc1;
        if (has2) y[row + 1] += acc2;
      } else {
        y[row] = acc1;
        if (has2) y[row + 1] = acc2;
      }
    }
  }
}

// STREAM variant (CSR-stream): each block owns a fixed ELEMENT range
// [base, base+NB), loads val/idx pairs coalesced, gathers x, stages the
// products in LDS, then reduces its rows from LDS (binary search for the
// row range).  Rows fully inside the block store directly; block-boundary
// rows atomicAdd into a pre-zeroed y.  Short-row matrices only (long rows
// would serialize one thread's reduce) — selection in spmv_launch.
__device__ inline i64 last_row_leq(const i64* __restrict__ indptr,
                                   i64 n_rows, i64 v) {
  // max r in [0, n_rows) with indptr[r] <= v
  i64 lo = 0, hi = n_rows - 1;
  while (lo < hi) {
    const i64 mid = (lo + hi + 1) >> 1;
    if (indptr[mid] <= v)
      lo = mid;
    else
      hi = mid - 1;
  }
  return lo;
}

template <typename T, typename I, int PE>
__global__ __launch_bounds__(LS_THREADS) void spmv_stream_kernel(
    const i64* __restrict__ indptr, const I* __restrict__ indices,
    const T* __restrict__ vals, const T* __restrict__ x, T* __restrict__ y,
    i64 n_rows, i64 nnz) {
  using T2 = __attribute__((ext_vector_type(2))) T;
  using I2 = __attribute__((ext_vector_type(2))) I;
  constexpr int NB = LS_THREADS * PE;
  __shared__ T prods[NB];
  const i64 base = (i64)blockIdx.x * NB;
  if (base >= nnz) return;
  const i64 end = (base + NB < nnz) ? base + NB : nnz;
  // load + multiply, pairs (base is NB-aligned, NB even => 16-B aligned)
  for (int t = threadIdx.x * 2; t < NB; t += LS_THREADS * 2) {
    const i64 j = base + t;
    if (j + 1 < end) {
      const T2 v = *reinterpret_cast<const T2*>(vals + j);
      const I2 c = *reinterpret_cast<const I2*>(indices + j);
      const T2 p = {v.x * x[c.x], v.y * x[c.y]};
      *reinterpret_cast<T2*>(&prods[t]) = p;
    } else if (j < end) {
      prods[t] = vals[j] * x[indices[j]];
    }
  }
  __syncthreads();
  const i64 r0 = last_row_leq(indptr, n_rows, base);
  const i64 r1 = last_row_leq(indptr, n_rows, end - 1);
  for (i64 r = r0 + threadIdx.x; r <= r1; r += LS_THREADS) {
    const i64 rs = indptr[r], re = indptr[r + 1];
    const i64 s = rs > base ? rs : base;
    const i64 e = re < end ? re : end;
    T acc = ls_zero<T>();
    for (i64 j = s; j < e; ++j) acc += prods[j - base];
    if (rs >= base && re <= end) {
      y[r] = acc;  // interior row: exactly one owner
    } else if (e > s) {
      atomicAdd(&y[r], acc);  // boundary row: y pre-zeroed by host
    }
  }
}

// AFFINE variant: rows whose columns are exactly row + D[j] (detected
// and cached host-side — 5-pt stencils, banded operators) never load
// the index stream at all: 8 B/nnz instead of 12 B/nnz on the
// memory-bound path.  Non-conforming rows (grid boundaries, ~0.1%) are
// masked out here and computed by spmv_rows_kernel from a row list:
// run inline, one lane's serial indptr/indices/x chain holds its whole
// wave for ~10 memory latencies (measured +30 us on Poisson 4096^2,
// profiles/spmv_affine_tiles.md).
//
// Each wave walks tiles of LS_AFFINE_TILE rows.  tile_base[t] >= 0 says
// every row of tile t conforms, so row r of it starts at
// tile_base[t] + (r - t*TILE) * ND: neither indptr nor mask is read
// (one uniform 8-B load per wave instead of 9 B per row).  A tile with
// tile_base[t] < 0 (or a null table) is mixed: its conforming rows read
// mask + indptr per row.
//
// CONST (real dtypes): the table is the value-bound tile_cbase written by
// affine_const_tiles_kernel below, which adds a third tile kind:
//   -2   full AND every row of the tile holds the values cpat[0..ND)
//        bit for bit (constant-coefficient stencils): no vals, indptr or
//        mask load at all, the row is sum_j cpat[j] * x[row + D[j]] with
//        cpat in sgprs -- about 10 B/row read instead of 50
//   >= 0 full, values vary: as above
//   -1   mixed: as above
// cpat is a runtime argument and the sum keeps the order and shape of
// the loaded-values path, so y has the same bits either way.  The table
// belongs to one vals tensor at one version of its contents: the host
// side (csr_array._affine_const) hands it out only while the plan object,
// the tensor's data_ptr() and its torch _version are the ones it was
// built from, rebuilds it otherwise, and stops scanning a matrix whose
// table went stale twice; ops.spmv ignores a table of another data_ptr().
// LS_SPMV_AFFINE_CONST=0 runs without the table, LS_SPMV_AFFINE_TILES=0
// without either table (in-build A/B).  CONST = false never touches cpat
// and compiles to what it did without the parameter.
//
// Tile groups (narrow stencils with a table, no dot fusion): a -2 tile is
// 64 rows x 17 B of traffic behind the whole chain kernarg -> D, cpat,
// table -> x -> store, so one tile per wave leaves the memory system
// short of requests (profiles/spmv_affine_const.md: 53 % of the copy
// rate).  Where affine_group(ND, sizeof(T)) > 1 such a launch goes to
// spmv_affine_groups_kernel instead of spmv_affine_kernel: a wave
// owns that many consecutive tiles, reads their table entries with one
// scalar load issued together with D and cpat, and issues the x loads of
// all its -2 tiles before the first sum; its other tiles then run the
// per-row body.  The grid counts groups, and the exception rows (the row
// list of spmv_rows_kernel) run in the first blocks of the same launch.
// Sums keep their order and shape, so y keeps its bits.
// LS_SPMV_AFFINE_GROUP=1 launches this kernel and the row list as before,
// LS_SPMV_AFFINE_FOLD=0 only moves the row list back into its own launch
// (in-build A/B).  This kernel itself, with and without DOT, is what it
// was before groups existed (profiles/spmv_affine_groups.md).
//
// Same bits as the CONST = false kernel of the same matrix takes one more
// step in fp32.  The fp64 sum compiles to one fma chain in every
// instantiation.  The fp32 sum of the CONST = false kernels does not:
// the vectoriser turns it into v_pk_mul_f32 plus adds, i.e. every
// product is rounded before it is added, for ND <= LS_AFFINE_CONST_F32_ND
// (beyond that it leaves a fused tail).  CONST = true fp32 kernels
// therefore switch contraction off for the row sum, which is that same
// arithmetic whatever the vectoriser then does, and are not offered past
// that ND.  tests/test_spmv_affine_const.py compares the two kernels bit
// for bit across ND, so a compiler that decides otherwise shows there.
#define LS_AFFINE_CONST_F32_ND 13
template <typename T, int ND>
__device__ __forceinline__ T affine_row_sum_unfused(const T (&a)[ND],
                                                    const T (&xv)[ND]) {
#pragma clang fp contract(off)
  T acc = ls_zero<T>();
#pragma unroll
  for (int j = 0; j < ND; ++j) acc += a[j] * xv[j];
  return acc;
}

// Tile groups: a wave of spmv_affine_groups_kernel owns
// affine_group(ND, sizeof(T)) consecutive tiles.  The x values of all of
// them take 320 B of registers per lane at the most (eight tiles of the
// 5-point fp64 stencil: measured against two and four,
// profiles/spmv_affine_groups.md); a stencil wider than 80 B per row gets
// no groups and stays on spmv_affine_kernel, which is short of sgprs as
// it is.
__host__ __device__ constexpr int affine_group(int nd, int elem_bytes) {
  if (elem_bytes == 4 && nd > LS_AFFINE_CONST_F32_ND) return 1;  // no table
  if (nd * elem_bytes > 80) return 1;
  int g = 1;
  while (2 * g <= 8 && 2 * g * nd * elem_bytes <= 320) g *= 2;
  return g;
}

// The constant-tile kernel of narrow stencils (real dtypes, no dot
// fusion, affine_group(ND, sizeof(T)) > 1).  tile_base is the value-bound
// table.  The first rest_blocks blocks do the exception rows rest[0 ..
// n_rest) (spmv_rows_kernel's loop, same sum order; their y rows have
// mask == 0 and lie in no full tile, so the groups never touch them), the
// others do the groups.  Tiles that are not -2 run the per-row body of
// spmv_affine_kernel, repeated here so that kernel stays as it is.
template <typename T, int ND>
__global__ __launch_bounds__(LS_THREADS) void spmv_affine_groups_kernel(
    const i64* __restrict__ indptr, const T* __restrict__ vals,
    const T* __restrict__ x, T* __restrict__ y,
    const int* __restrict__ D, const unsigned char* __restrict__ mask,
    const i64* __restrict__ tile_base, i64 n_rows, int accumulate,
    const T* __restrict__ cpat, const i64* __restrict__ rest,
    const void* __restrict__ indices, i64 n_rest, int rest_blocks,
    int idx64) {
  static_assert(!is_cplx<T>::value, "constant tiles: real dtypes only");
  constexpr bool UNFUSED = sizeof(T) == 4;
  constexpr int G = affine_group(ND, (int)sizeof(T));
  static_assert(G > 1, "one tile per wave is spmv_affine_kernel");
  unsigned blk = blockIdx.x, n_blk = gridDim.x;
  if (n_rest > 0) {
    if (blk < (unsigned)rest_blocks) {
      const i64 i = (i64)blk * LS_THREADS + threadIdx.x;
      if (i >= n_rest) return;
      const i64 row = rest[i];
      const i64 s = indptr[row];
      const i64 e = indptr[row + 1];
      T acc = ls_zero<T>();
      if (idx64) {
        const i64* ix = static_cast<const i64*>(indices);
        for (i64 jp = s; jp < e; ++jp) acc += vals[jp] * x[ix[jp]];
      } else {
        const int* ix = static_cast<const int*>(indices);
        for (i64 jp = s; jp < e; ++jp) acc += vals[jp] * x[ix[jp]];
      }
      if (accumulate)
        y[row] += acc;
      else
        y[row] = acc;
      return;
    }
    blk -= rest_blocks;
    n_blk -= rest_blocks;
  }
  const int lane = threadIdx.x % WAVE_SIZE;
  // wave-uniform group index, kept scalar so the table load is scalar.
  // The launch has LS_THREADS per block: reading blockDim.x here would
  // put a vector load of the dispatch packet in front of everything.
  const i64 wave0 = __builtin_amdgcn_readfirstlane(
      (int)((blk * LS_THREADS + threadIdx.x) / WAVE_SIZE));
  const i64 n_waves = (i64)n_blk * (LS_THREADS / WAVE_SIZE);
  const i64 n_tiles = (n_rows + LS_AFFINE_TILE - 1) / LS_AFFINE_TILE;
  const i64 n_groups = (n_tiles + G - 1) / G;
  // a group's table entries: contiguous, one scalar load; the last group
  // may be partial and reads no entry past n_tiles
  auto load_entries = [&](const i64 t0, i64 (&b)[G])
                          __attribute__((always_inline)) {
    if (t0 + G <= n_tiles) {
#pragma unroll
      for (int k = 0; k < G; ++k) b[k] = tile_base[t0 + k];
    } else {
#pragma unroll
      for (int k = 0; k < G; ++k)
        b[k] = t0 + k < n_tiles ? tile_base[t0 + k] : (i64)-1;
    }
  };
  // the first group's entries go out together with D and cpat, the next
  // group's at the end of each step: the wave's life is a chain of
  // dependent latencies, and this takes one link out of it
  i64 b[G];
  if (wave0 < n_groups) load_entries(wave0 * G, b);
  int d[ND];
#pragma unroll
  for (int j = 0; j < ND; ++j) d[j] = D[j];  // uniform: lands in sgprs
  T c[ND];
#pragma unroll
  for (int j = 0; j < ND; ++j) c[j] = cpat[j];  // uniform, like d
  // a full tile whose values vary (base >= 0) or a mixed one (base == -1):
  // spmv_affine_kernel's rows, sum in the same order and shape
  auto other_tile = [&](const i64 tile, const i64 base)
                        __attribute__((always_inline)) {
    const i64 row = tile * LS_AFFINE_TILE + lane;
    i64 s;
    if (base >= 0) {
      s = base + (i64)lane * ND;
    } else {
      if (row >= n_rows) return;
      if (!mask[row]) return;
      s = indptr[row];
    }
    T v[ND], xv[ND];
#pragma unroll
    for (int j = 0; j < ND; ++j) v[j] = vals[s + j];
#pragma unroll
    for (int j = 0; j < ND; ++j) xv[j] = x[row + d[j]];
    T acc = ls_zero<T>();
    if constexpr (UNFUSED) {
      acc = affine_row_sum_unfused<T, ND>(v, xv);
    } else {
#pragma unroll
      for (int j = 0; j < ND; ++j) acc += v[j] * xv[j];
    }
    if (accumulate)
      y[row] += acc;
    else
      y[row] = acc;
  };
  // the grid-stride loop advances by groups of G tiles, group-aligned
  for (i64 grp = wave0; grp < n_groups;) {
    const i64 t0 = grp * G;
    unsigned consts = 0;  // the group's -2 tiles (wave-uniform masks)
    unsigned others = 0;  // its tiles that exist and are not -2
#pragma unroll
    for (int k = 0; k < G; ++k) {
      if (b[k] == -2)
        consts |= 1u << k;
      else if (t0 + k < n_tiles)
        others |= 1u << k;
    }
    if (consts) {
      // every x load of every -2 tile of the group goes out before the
      // first sum: G * ND loads in flight per lane, not ND.  Loads and
      // sums are straight-line code, so each sum waits for its own
      // tile's loads only; the scalar branches guard the stores.  Slot k
      // of a group that holds other tiles re-reads the x of the group's
      // first -2 tile (rows the wave loads anyway, never a row >=
      // n_rows) and drops the sum.
      const int k_first = __builtin_ctz(consts);
      T xv[G][ND];
#pragma unroll
      for (int k = 0; k < G; ++k) {
        const int ks = ((consts >> k) & 1u) ? k : k_first;
        const T* xrow = x + ((t0 + ks) * LS_AFFINE_TILE + lane);
#pragma unroll
        for (int j = 0; j < ND; ++j) xv[k][j] = xrow[d[j]];
      }
      // no sum is scheduled in among the loads
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int k = 0; k < G; ++k) {
        const i64 row = (t0 + k) * LS_AFFINE_TILE + lane;
        T acc = ls_zero<T>();
        if constexpr (UNFUSED) {
          acc = affine_row_sum_unfused<T, ND>(c, xv[k]);
        } else {
#pragma unroll
          for (int j = 0; j < ND; ++j) acc += c[j] * xv[k][j];
        }
        // pins the sum here: without it the compiler sinks a tile's
        // loads and sum behind the branch, after the other tiles'
        asm volatile("" : "+v"(acc));
        if ((consts >> k) & 1u) {
          if (accumulate)
            y[row] += acc;
          else
            y[row] = acc;
        }
      }
    }
    // full-varying and mixed tiles of the group, one after another
    // (rare: 3 % of the tiles on Poisson 4096^2)
    while (others) {
      const int k = __builtin_ctz(others);
      others &= others - 1;
      other_tile(t0 + k, tile_base[t0 + k]);
    }
    grp += n_waves;
    if (grp < n_groups) load_entries(grp * G, b);
  }
}

template <typename T, int ND, bool DOT, bool CONST>
__global__ __launch_bounds__(LS_THREADS) void spmv_affine_kernel(
    const i64* __restrict__ indptr, const T* __restrict__ vals,
    const T* __restrict__ x, T* __restrict__ y,
    const int* __restrict__ D, const unsigned char* __restrict__ mask,
    const i64* __restrict__ tile_base, i64 n_rows, int accumulate,
    T* __restrict__ dot_out, const T* __restrict__ cpat) {
  // DOT: additionally reduce sum_i x[i]*y[i] into dot_out (the CG
  // pipeline's p.(A p), fused so the dot costs no extra pass)
  static_assert(LS_AFFINE_TILE == WAVE_SIZE, "one tile per wave step");
  static_assert(!CONST || !is_cplx<T>::value, "CONST: real dtypes only");
  constexpr bool UNFUSED = CONST && sizeof(T) == 4;
  int d[ND];
#pragma unroll
  for (int j = 0; j < ND; ++j) d[j] = D[j];  // uniform: lands in sgprs
  [[maybe_unused]] T c[ND];
  if constexpr (CONST) {
#pragma unroll
    for (int j = 0; j < ND; ++j) c[j] = cpat[j];  // uniform, like d
  }
  const int lane = threadIdx.x % WAVE_SIZE;
  // wave-uniform tile index, kept scalar so the table load is scalar
  const i64 wave0 = __builtin_amdgcn_readfirstlane(
      (int)((blockIdx.x * blockDim.x + threadIdx.x) / WAVE_SIZE));
  const i64 n_waves = (i64)gridDim.x * (LS_THREADS / WAVE_SIZE);
  const i64 n_tiles = (n_rows + LS_AFFINE_TILE - 1) / LS_AFFINE_TILE;
  T dacc = ls_zero<T>();
  for (i64 tile = wave0; tile < n_tiles; tile += n_waves) {
    const i64 row = tile * LS_AFFINE_TILE + lane;
    const i64 base = tile_base ? tile_base[tile] : (i64)-1;
    if constexpr (CONST) {
      if (base == -2) {  // wave-uniform; the tile is whole, so row < n_rows
        T xv[ND];
#pragma unroll
        for (int j = 0; j < ND; ++j) xv[j] = x[row + d[j]];
        T acc = ls_zero<T>();
        if constexpr (UNFUSED) {
          acc = affine_row_sum_unfused<T, ND>(c, xv);
        } else {
#pragma unroll
          for (int j = 0; j < ND; ++j) acc += c[j] * xv[j];
        }
        if (accumulate)
          y[row] += acc;
        else
          y[row] = acc;
        if constexpr (DOT) dacc += x[row] * acc;
        continue;
      }
    }
    i64 s;
    if (base >= 0) {
      s = base + (i64)lane * ND;
    } else {
      if (row >= n_rows) continue;
      if (!mask[row]) {
        if constexpr (DOT) dacc += x[row] * y[row];
        continue;
      }
      s = indptr[row];
    }
    T v[ND], xv[ND];
#pragma unroll
    for (int j = 0; j < ND; ++j) v[j] = vals[s + j];
#pragma unroll
    for (int j = 0; j < ND; ++j) xv[j] = x[row + d[j]];
    T acc = ls_zero<T>();
    if constexpr (UNFUSED) {
      acc = affine_row_sum_unfused<T, ND>(v, xv);
    } else {
#pragma unroll
      for (int j = 0; j < ND; ++j) acc += v[j] * xv[j];
    }
    if (accumulate)
      y[row] += acc;
    else
      y[row] = acc;
    if constexpr (DOT) dacc += x[row] * acc;
  }
  if constexpr (DOT) {
    __shared__ T partials[LS_THREADS / WAVE_SIZE];
    dacc = group_reduce_sum<T, WAVE_SIZE>(dacc);
    const int wave = threadIdx.x / WAVE_SIZE;
    const int lane = threadIdx.x % WAVE_SIZE;
    if (lane == 0) partials[wave] = dacc;
    __syncthreads();
    if (threadIdx.x == 0) {
      T total = partials[0];
      for (int w = 1; w < LS_THREADS / WAVE_SIZE; ++w)
        total += partials[w];
      dot_atomic_add(dot_out, total);
    }
  }
}

// Constant-tile detection for spmv_affine_kernel<.., CONST = true>: one
// wave per tile, one read of vals.  tile_cbase[t] = -2 when tile t is
// full (tile_base[t] >= 0) and each of its rows holds cpat[0..nd) bit
// for bit, else tile_base[t].  U is the unsigned integer of the value's
// width: an integer compare keeps -0.0 apart from 0.0 and NaN payloads
// apart from each other, so a -2 tile cannot change a result bit.
template <typename U>
__global__ __launch_bounds__(LS_THREADS) void affine_const_tiles_kernel(
    const U* __restrict__ vals, const i64* __restrict__ tile_base,
    const U* __restrict__ cpat, i64* __restrict__ tile_cbase, i64 n_tiles,
    int nd) {
  const int lane = threadIdx.x % WAVE_SIZE;
  const i64 wave0 = __builtin_amdgcn_readfirstlane(
      (int)((blockIdx.x * blockDim.x + threadIdx.x) / WAVE_SIZE));
  const i64 n_waves = (i64)gridDim.x * (LS_THREADS / WAVE_SIZE);
  for (i64 tile = wave0; tile < n_tiles; tile += n_waves) {
    const i64 base = tile_base[tile];
    bool same = base >= 0;
    if (same) {
      const U* row = vals + base + (i64)lane * nd;
      for (int j = 0; j < nd; ++j) same &= row[j] == cpat[j];
    }
    const bool all = __ballot(same) == ~0ull;
    if (lane == 0) tile_cbase[tile] = all ? (i64)-2 : base;
  }
}

// AFFINE2: pair-loaded variant of the affine kernel — vals stream loaded
// as 16-B T2 vectors from an even-aligned base (halves the vals VMEM
// count); when the stencil offsets are CONSECUTIVE (banded operators:
// D = d0, d0+1, ..., d0+ND-1) the x window [row+d0, row+d0+ND) is also
// pair-loaded.  x_hi guards the final x pair at the array tail.
template <typename T, int ND, bool XCONSEC>
__global__ __launch_bounds__(LS_THREADS) void spmv_affine2_kernel(
    const i64* __restrict__ indptr, const T* __restrict__ vals,
    const T* __restrict__ x, T* __restrict__ y,
    const int* __restrict__ D, const unsigned char* __restrict__ mask,
    i64 n_rows, i64 nnz, i64 x_hi, int accumulate) {
  using T2 = __attribute__((ext_vector_type(2))) T;
  int d[ND];
#pragma unroll
  for (int j = 0; j < ND; ++j) d[j] = D[j];
  constexpr int NP = (ND + 2) / 2;   // pairs covering [s2, s2+ND+1)
  constexpr int NX = (ND + 1) / 2;   // pairs covering [base, base+ND)
  const i64 stride = (i64)gridDim.x * blockDim.x;
  for (i64 row = (i64)blockIdx.x * blockDim.x + threadIdx.x; row < n_rows;
       row += stride) {
    if (!mask[row]) continue;
    const i64 s = indptr[row];
    const i64 s2 = s & ~(i64)1;
    T2 vp[NP];
#pragma unroll
    for (int k = 0; k < NP; ++k) {
      const i64 pp = s2 + 2 * k;
      if (pp < s + ND) {
        if (pp + 2 <= nnz) {
          vp[k] = *reinterpret_cast<const T2*>(vals + pp);
        } else {
          vp[k].x = vals[pp];
        }
      }
    }
    T xv[ND];
    if constexpr (XCONSEC) {
      const i64 base = row + d[0];
      T2 xp[NX + 1];
#pragma unroll
      for (int k = 0; k <= NX; ++k) {
        const i64 bb = base + 2 * k;
        if (2 * k < ND) {
          if (bb + 2 <= x_hi) {
            xp[k] = *reinterpret_cast<const T2*>(x + bb);
          } else {
            xp[k].x = x[bb];
          }
        }
      }
#pragma unroll
      for (int j = 0; j < ND; ++j)
        xv[j] = (j & 1) ? xp[j / 2].y : xp[j / 2].x;
    } else {
#pragma unroll
      for (int j = 0; j < ND; ++j) xv[j] = x[row + d[j]];
    }
    T acc = ls_zero<T>();
    if (s == s2) {
#pragma unroll
      for (int j = 0; j < ND; ++j)
        acc += ((j & 1) ? vp[j / 2].y : vp[j / 2].x) * xv[j];
    } else {
#pragma unroll
      for (int j = 0; j < ND; ++j)
        acc += (((j + 1) & 1) ? vp[(j + 1) / 2].y
                              : vp[(j + 1) / 2].x) * xv[j];
    }
    if (accumulate)
      y[row] += acc;
    else
      y[row] = acc;
  }
}

// general gather over an explicit row list (the affine variant's
// exception rows; also reusable for any scattered-row update)
template <typename T, typename I>
__global__ __launch_bounds__(LS_THREADS) void spmv_rows_kernel(
    const i64* __restrict__ rows_list, i64 n_list,
    const i64* __restrict__ indptr, const I* __restrict__ indices,
    const T* __restrict__ vals, const T* __restrict__ x,
    T* __restrict__ y, int accumulate) {
  const i64 stride = (i64)gridDim.x * blockDim.x;
  for (i64 i = (i64)blockIdx.x * blockDim.x + threadIdx.x; i < n_list;
       i += stride) {
    const i64 row = rows_list[i];
    const i64 s = indptr[row];
    const i64 e = indptr[row + 1];
    T acc = ls_zero<T>();
    for (i64 jp = s; jp < e; ++jp) acc += vals[jp] * x[indices[jp]];
    if (accumulate)
      y[row] += acc;
    else
      y[row] = acc;
  }
}

// Which general kernel a call runs.  The selection lives in one host
// function so that the launcher and the tests (module.cpp: spmv_select)
// cannot disagree about it.
enum SpmvKind {
  SPMV_VECTOR = 0,  // spmv_vector_kernel<W, NT=false, SWZ=false>
  SPMV_VECTOR_NT,   // spmv_vector_kernel<W, NT=true,  SWZ=false>
  SPMV_VECTOR_SWZ,  // spmv_vector_kernel<W, NT=false, SWZ=true>
  SPMV_PAIR,        // spmv_pair_kernel<W, SWZ=false>
  SPMV_PAIR_SWZ,    // spmv_pair_kernel<W, SWZ=true>
  SPMV_PAIR2,       // spmv_pair2_kernel<W, SWZ=false>
  SPMV_STEN,        // spmv_sten_kernel<NP = W>       (W is 4 or 8)
  SPMV_PAIRU,       // spmv_pairu_kernel<W, PPL = 4>  (W is 2 or 4)
  SPMV_STREAM,      // spmv_stream_kernel<PE = W>     (W is 8 or 16)
};
struct SpmvChoice {
  int kind;
  int W;
};

SpmvChoice spmv_select(i64 n_rows, i64 nnz, bool is_real, bool accumulate,
                       int w_override, bool nt, int pair_mode, int swz_mode,
                       i64 max_nnz) {
  const double mean = n_rows > 0 ? (double)nnz / (double)n_rows : 0.0;
  // W = largest power of two <= mean/2 (measured: ~2 elements per lane,
  // profiles/spmv_sweep_r01.txt)
  int W = 1;
  while (W < 64 && (double)(W * 4) <= mean) W *= 2;
  if (w_override > 0) W = w_override;
  // the kernels exist for W = 1, 2, 4, ..., 64: anything else runs as 64
  if (W < 1 || W > 64 || (W & (W - 1))) W = 64;
  // uniformly short rows: fully unrolled kernels (every load issued
  // before any use) measured 592 vs 525 GF/s on 5-pt Poisson
  // (profiles/spmv_pmc_r01.md)
  if (is_real && pair_mode < 0 && max_nnz >= 0) {
    if (max_nnz <= 7)
      pair_mode = 5;        // stencil W=1, PPL=4
    else if (max_nnz <= 15)
      pair_mode = 7;        // pairu W=2, PPL=4
    else if (max_nnz <= 31)
      pair_mode = 8;        // pairu W=4, PPL=4
  }
  const bool pair = (pair_mode < 0) ? (is_real && mean >= 3.0)
                                    : (pair_mode == 1 && is_real);
  const bool swz = swz_mode == 1;
  if (is_real) {
    // STREAM variant: pair_mode 2 (PE=8) / 3 (PE=16); real dtypes,
    // non-accumulating only (boundary rows atomicAdd into zeroed y)
    if ((pair_mode == 2 || pair_mode == 3) && !accumulate && n_rows > 0)
      return {SPMV_STREAM, pair_mode == 2 ? 8 : 16};
    if (pair_mode == 7) return {SPMV_PAIRU, 2};
    if (pair_mode == 8) return {SPMV_PAIRU, 4};
    if (pair_mode == 5) return {SPMV_STEN, 4};
    if (pair_mode == 6) return {SPMV_STEN, 8};
    if (pair_mode == 4) return {SPMV_PAIR2, W};
    if (pair) return {swz ? SPMV_PAIR_SWZ : SPMV_PAIR, W};
  }
  if (nt) return {SPMV_VECTOR_NT, W};
  if (swz) return {SPMV_VECTOR_SWZ, W};
  return {SPMV_VECTOR, W};
}

const char* spmv_kind_name(int kind) {
  static const char* const names[] = {"vector", "vector_nt", "vector_swz",
                                      "pair",   "pair_swz",  "pair2",
                                      "sten",   "pairu",     "stream"};
  return names[kind];
}

template <typename T, typename I>
void spmv_launch(const i64* indptr, const I* indices, const T* vals,
                 const T* x, T* y, i64 n_rows, i64 nnz, bool accumulate,
                 int w_override, bool nt, int pair_mode, int swz_mode,
                 i64 max_nnz, hipStream_t stream) {
  const SpmvChoice ch =
      spmv_select(n_rows, nnz, !is_cplx<T>::value, accumulate, w_override,
                  nt, pair_mode, swz_mode, max_nnz);
  if constexpr (!is_cplx<T>::value) {
    if (ch.kind == SPMV_STREAM) {
      ls_check(hipMemsetAsync(y, 0, n_rows * sizeof(T), stream),
               "spmv memset");
      if (nnz == 0) return;  // no element block: y = 0 is the product
      if (ch.W == 8) {
        constexpr int NB = LS_THREADS * 8;
        const i64 grid = (nnz + NB - 1) / NB;
        hipLaunchKernelGGL((spmv_stream_kernel<T, I, 8>), dim3(grid),
                           dim3(LS_THREADS), 0, stream, indptr, indices,
                           vals, x, y, n_rows, nnz);
      } else {
        constexpr int NB = LS_THREADS * 16;
        const i64 grid = (nnz + NB - 1) / NB;
        hipLaunchKernelGGL((spmv_stream_kernel<T, I, 16>), dim3(grid),
                           dim3(LS_THREADS), 0, stream, indptr, indices,
                           vals, x, y, n_rows, nnz);
      }
      ls_check(hipGetLastError(), "spmv_stream");
      return;
    }
  }
  static const char* gcap_env = std::getenv("LS_SPMV_GRID");
  const int gcap = gcap_env ? atoi(gcap_env) : 8192;
  const int acc = accumulate ? 1 : 0;
  if constexpr (!is_cplx<T>::value) {
    if (ch.kind == SPMV_PAIRU) {
      if (ch.W == 2)
        hipLaunchKernelGGL((spmv_pairu_kernel<T, I, 2, 4>),
                           dim3(grid_1d(n_rows, LS_THREADS / 2, gcap)),
                           dim3(LS_THREADS), 0, stream, indptr, indices,
                           vals, x, y, n_rows, nnz, acc);
      else
        hipLaunchKernelGGL((spmv_pairu_kernel<T, I, 4, 4>),
                           dim3(grid_1d(n_rows, LS_THREADS / 4, gcap)),
                           dim3(LS_THREADS), 0, stream, indptr, indices,
                           vals, x, y, n_rows, nnz, acc);
      ls_check(hipGetLastError(), "spmv");
      return;
    }
    if (ch.kind == SPMV_STEN) {
      const int grid3 = grid_1d(n_rows, LS_THREADS, gcap);
      if (ch.W == 4)
        hipLaunchKernelGGL((spmv_sten_kernel<T, I, 4>), dim3(grid3),
                           dim3(LS_THREADS), 0, stream, indptr, indices,
                           vals, x, y, n_rows, nnz, acc);
      else
        hipLaunchKernelGGL((spmv_sten_kernel<T, I, 8>), dim3(grid3),
                           dim3(LS_THREADS), 0, stream, indptr, indices,
                           vals, x, y, n_rows, nnz, acc);
      ls_check(hipGetLastError(), "spmv");
      return;
    }
  }
  auto launch = [&](auto wtag) {
    constexpr int WS = decltype(wtag)::value;
    constexpr int RPB = LS_THREADS / WS;
    const int grid = grid_1d(n_rows, RPB, gcap);
    switch (ch.kind) {
      case SPMV_PAIR2:
        if constexpr (!is_cplx<T>::value)
          hipLaunchKernelGGL((spmv_pair2_kernel<T, I, WS, false>),
                             dim3(grid_1d(n_rows, RPB * 2, gcap)),
                             dim3(LS_THREADS), 0, stream, indptr, indices,
                             vals, x, y, n_rows, nnz, acc);
        break;
      case SPMV_PAIR_SWZ:
        if constexpr (!is_cplx<T>::value)
          hipLaunchKernelGGL((spmv_pair_kernel<T, I, WS, true>),
                             dim3(grid), dim3(LS_THREADS), 0, stream,
                             indptr, indices, vals, x, y, n_rows, nnz, acc);
        break;
      case SPMV_PAIR:
        if constexpr (!is_cplx<T>::value)
          hipLaunchKernelGGL((spmv_pair_kernel<T, I, WS, false>),
                             dim3(grid), dim3(LS_THREADS), 0, stream,
                             indptr, indices, vals, x, y, n_rows, nnz, acc);
        break;
      case SPMV_VECTOR_NT:
        hipLaunchKernelGGL((spmv_vector_kernel<T, I, WS, true, false>),
                           dim3(grid), dim3(LS_THREADS), 0, stream, indptr,
                           indices, vals, x, y, n_rows, acc);
        break;
      case SPMV_VECTOR_SWZ:
        hipLaunchKernelGGL((spmv_vector_kernel<T, I, WS, false, true>),
                           dim3(grid), dim3(LS_THREADS), 0, stream, indptr,
                           indices, vals, x, y, n_rows, acc);
        break;
      default:
        hipLaunchKernelGGL((spmv_vector_kernel<T, I, WS, false, false>),
                           dim3(grid), dim3(LS_THREADS), 0, stream, indptr,
                           indices, vals, x, y, n_rows, acc);
        break;
    }
  };
  switch (ch.W) {
    case 1: launch(std::integral_constant<int, 1>{}); break;
    case 2: launch(std::integral_constant<int, 2>{}); break;
    case 4: launch(std::integral_constant<int, 4>{}); break;
    case 8: launch(std::integral_constant<int, 8>{}); break;
    case 16: launch(std::integral_constant<int, 16>{}); break;
    case 32: launch(std::integral_constant<int, 32>{}); break;
    default: launch(std::integral_constant<int, 64>{}); break;
  }
  ls_check(hipGetLastError(), "spmv");
}

}  // namespace

namespace {
template <typename T>
void spmv_affine_dispatch_nd(const i64* indptr, const T* vals, const T* x,
                             T* y, const int* D,
                             const unsigned char* mask,
                             const i64* tile_base, i64 n_rows, int nd,
                             int accumulate, T* dot_out, const T* cpat,
                             const i64* rest, i64 n_rest,
                             const void* indices, int idx64, bool group1,
                             hipStream_t s) {
  // cpat != null: tile_base is the value-bound tile_cbase (-2 tiles)
  if (cpat && (is_cplx<T>::value || !tile_base ||
               (sizeof(T) == 4 && nd > LS_AFFINE_CONST_F32_ND)))
    throw std::runtime_error(
        "spmv_affine: constant tiles need a real dtype, a tile table and, "
        "in fp32, nd <= " + std::to_string(LS_AFFINE_CONST_F32_ND));
  // the constant-tile launch of a narrow stencil takes tile groups, and
  // the exception rows with them (LS_SPMV_AFFINE_GROUP=1: group1)
  const bool groups = cpat && !dot_out && !group1 && !is_cplx<T>::value &&
                      nd >= 1 && nd <= 16 &&
                      affine_group(nd, (int)sizeof(T)) > 1;
  if (n_rest > 0 && !groups)
    throw std::runtime_error(
        "spmv_affine: a row list rides in a launch with tile groups only");
  // one tile per wave, blocks dispatched in row order: measured 162.6 us
  // uncapped vs 168.6 / 174.6 / 182.9 us at caps 32768 / 16384 / 8192
  // (Poisson 4096^2, profiles/spmv_affine_tiles.md); the grid-stride
  // loop only runs past 2^30 rows.  The DOT variant keeps the 8192 cap:
  // every block ends in one atomic on dot_out.
  const char* gcap_env = std::getenv("LS_SPMV_AFFINE_GRID");
  int gcap = gcap_env ? atoi(gcap_env) : 0;
  if (gcap < 1) gcap = dot_out ? 8192 : 1 << 22;
  const int grid = grid_1d(n_rows, LS_THREADS, gcap);
  // groups: the grid counts groups, the row list's blocks come on top
  const i64 n_tiles = (n_rows + LS_AFFINE_TILE - 1) / LS_AFFINE_TILE;
  const int rest_blocks =
      n_rest > 0 ? (int)((n_rest + LS_THREADS - 1) / LS_THREADS) : 0;
  switch (nd) {
#define LS_AFF_GROUPS(N)                                                   \
  if constexpr (!is_cplx<T>::value &&                                      \
                affine_group(N, (int)sizeof(T)) > 1) {                     \
    if (groups) {                                                          \
      constexpr int g = affine_group(N, (int)sizeof(T));                   \
      const int ggrid =                                                    \
          grid_1d((n_tiles + g - 1) / g, LS_THREADS / WAVE_SIZE, gcap) +   \
          rest_blocks;                                                     \
      hipLaunchKernelGGL((spmv_affine_groups_kernel<T, N>), dim3(ggrid),   \
                         dim3(LS_THREADS), 0, s, indptr, vals, x, y, D,    \
                         mask, tile_base, n_rows, accumulate, cpat, rest,  \
                         indices, n_rest, rest_blocks, idx64);             \
      break;                                                               \
    }                                                                      \
  }
#define LS_AFF_LAUNCH(N, DOT, CONST)                                       \
  hipLaunchKernelGGL((spmv_affine_kernel<T, N, DOT, CONST>), dim3(grid),   \
                     dim3(LS_THREADS), 0, s, indptr, vals, x, y, D, mask,  \
                     tile_base, n_rows, accumulate, dot_out, cpat)
#define LS_AFF_CASE(N)                                                     \
  case N:                                                                  \
    LS_AFF_GROUPS(N)                                                       \
    if constexpr (!is_cplx<T>::value) {                                    \
      if (cpat) {                                                          \
        if (dot_out)                                                       \
          LS_AFF_LAUNCH(N, true, true);                                    \
        else                                                               \
          LS_AFF_LAUNCH(N, false, true);                                   \
        break;                                                             \
      }                                                                    \
    }                                                                      \
    if (dot_out)                                                           \
      LS_AFF_LAUNCH(N, true, false);                                       \
    else                                                                   \
      LS_AFF_LAUNCH(N, false, false);                                      \
    break;
    LS_AFF_CASE(1)
    LS_AFF_CASE(2) LS_AFF_CASE(3) LS_AFF_CASE(4) LS_AFF_CASE(5)
    LS_AFF_CASE(6) LS_AFF_CASE(7) LS_AFF_CASE(8) LS_AFF_CASE(9)
    LS_AFF_CASE(10) LS_AFF_CASE(11) LS_AFF_CASE(12) LS_AFF_CASE(13)
    LS_AFF_CASE(14) LS_AFF_CASE(15) LS_AFF_CASE(16)
#undef LS_AFF_CASE
#undef LS_AFF_GROUPS
#undef LS_AFF_LAUNCH
    default:
      throw std::runtime_error("spmv_affine: nd out of range (1..16)");
  }
  ls_check(hipGetLastError(), "spmv_affine");
}
}  // namespace

namespace {
template <typename T>
void spmv_affine2_dispatch_nd(const i64* indptr, const T* vals, const T* x,
                              T* y, const int* D,
                              const unsigned char* mask, i64 n_rows,
                              i64 nnz, i64 x_hi, int nd, bool xconsec,
                              int accumulate, hipStream_t s) {
  const int grid = grid_1d(n_rows, LS_THREADS, 8192);
  switch (nd * 2 + (xconsec ? 1 : 0)) {
#define LS_AFF2_CASE(N)                                                    \
  case 2 * N:                                                              \
    hipLaunchKernelGGL((spmv_affine2_kernel<T, N, false>), dim3(grid),     \
                       dim3(LS_THREADS), 0, s, indptr, vals, x, y, D,      \
                       mask, n_rows, nnz, x_hi, accumulate);               \
    break;                                                                 \
  case 2 * N + 1:                                                          \
    hipLaunchKernelGGL((spmv_affine2_kernel<T, N, true>), dim3(grid),      \
                       dim3(LS_THREADS), 0, s, indptr, vals, x, y, D,      \
                       mask, n_rows, nnz, x_hi, accumulate);               \
    break;
    LS_AFF2_CASE(1)
    LS_AFF2_CASE(2) LS_AFF2_CASE(3) LS_AFF2_CASE(4) LS_AFF2_CASE(5)
    LS_AFF2_CASE(6) LS_AFF2_CASE(7) LS_AFF2_CASE(8) LS_AFF2_CASE(9)
    LS_AFF2_CASE(10) LS_AFF2_CASE(11) LS_AFF2_CASE(12) LS_AFF2_CASE(13)
    LS_AFF2_CASE(14) LS_AFF2_CASE(15) LS_AFF2_CASE(16)
#undef LS_AFF2_CASE
    default:
      throw std::runtime_error("spmv_affine2: nd out of range (1..16)");
  }
  ls_check(hipGetLastError(), "spmv_affine2");
}
}  // namespace

void ls_spmv_affine2(uintptr_t indptr, uintptr_t vals, uintptr_t x,
                     uintptr_t y, uintptr_t D, uintptr_t mask, i64 n_rows,
                     i64 nnz, i64 x_hi, int nd, bool xconsec, int dtype,
                     bool accumulate, uintptr_t stream) {
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  if (dtype == 0)
    spmv_affine2_dispatch_nd<float>(
        reinterpret_cast<const i64*>(indptr),
        reinterpret_cast<const float*>(vals),
        reinterpret_cast<const float*>(x), reinterpret_cast<float*>(y),
        reinterpret_cast<const int*>(D),
        reinterpret_cast<const unsigned char*>(mask), n_rows, nnz, x_hi,
        nd, xconsec, accumulate ? 1 : 0, s);
  else if (dtype == 1)
    spmv_affine2_dispatch_nd<double>(
        reinterpret_cast<const i64*>(indptr),
        reinterpret_cast<const double*>(vals),
        reinterpret_cast<const double*>(x), reinterpret_cast<double*>(y),
        reinterpret_cast<const int*>(D),
        reinterpret_cast<const unsigned char*>(mask), n_rows, nnz, x_hi,
        nd, xconsec, accumulate ? 1 : 0, s);
  else
    throw std::runtime_error("spmv_affine2: real dtypes only");
}

void ls_spmv_affine(uintptr_t indptr, uintptr_t vals, uintptr_t x,
                    uintptr_t y, uintptr_t D, uintptr_t mask,
                    uintptr_t tile_base, i64 n_rows, int nd, int dtype,
                    bool accumulate, uintptr_t dot_out, uintptr_t cpat,
                    uintptr_t rest, i64 n_rest, uintptr_t indices,
                    int idx_dtype, int group, uintptr_t stream) {
  // cpat != 0: tile_base is a tile_cbase from ls_affine_const_tiles and
  // cpat its nd-value pattern (device, the value dtype).  n_rest > 0:
  // the exception rows rest[0..n_rest) run in the same launch (indices
  // of idx_dtype, as in ls_spmv_rows).  group == 1: one tile per wave.
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  if (dot_out && dtype > 1)
    throw std::runtime_error("spmv_affine dot fusion: real dtypes only");
  if (n_rest > 0 && (idx_dtype < 0 || idx_dtype > 1 || !rest || !indices))
    throw std::runtime_error("spmv_affine: bad folded row list");
  DISPATCH_VAL_T(dtype, spmv_affine_dispatch_nd<val_t>(
      reinterpret_cast<const i64*>(indptr),
      reinterpret_cast<const val_t*>(vals),
      reinterpret_cast<const val_t*>(x), reinterpret_cast<val_t*>(y),
      reinterpret_cast<const int*>(D),
      reinterpret_cast<const unsigned char*>(mask),
      reinterpret_cast<const i64*>(tile_base), n_rows, nd,
      accumulate ? 1 : 0, reinterpret_cast<val_t*>(dot_out),
      reinterpret_cast<const val_t*>(cpat),
      reinterpret_cast<const i64*>(rest), n_rest > 0 ? n_rest : 0,
      reinterpret_cast<const void*>(indices), idx_dtype == 1 ? 1 : 0,
      group == 1, s));
}

void ls_affine_const_tiles(uintptr_t vals, uintptr_t tile_base,
                           uintptr_t cpat, uintptr_t tile_cbase,
                           i64 n_tiles, int nd, int dtype,
                           uintptr_t stream) {
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  if (nd < 1 || nd > 16)
    throw std::runtime_error("affine_const_tiles: nd out of range (1..16)");
  if (n_tiles <= 0) return;
  const int grid = grid_1d(n_tiles, LS_THREADS / WAVE_SIZE, 1 << 22);
  const i64* tb = reinterpret_cast<const i64*>(tile_base);
  i64* cb = reinterpret_cast<i64*>(tile_cbase);
  if (dtype == 0)
    hipLaunchKernelGGL((affine_const_tiles_kernel<uint32_t>), dim3(grid),
                       dim3(LS_THREADS), 0, s,
                       reinterpret_cast<const uint32_t*>(vals), tb,
                       reinterpret_cast<const uint32_t*>(cpat), cb,
                       n_tiles, nd);
  else if (dtype == 1)
    hipLaunchKernelGGL((affine_const_tiles_kernel<uint64_t>), dim3(grid),
                       dim3(LS_THREADS), 0, s,
                       reinterpret_cast<const uint64_t*>(vals), tb,
                       reinterpret_cast<const uint64_t*>(cpat), cb,
                       n_tiles, nd);
  else
    throw std::runtime_error("affine_const_tiles: real dtypes only");
  ls_check(hipGetLastError(), "affine_const_tiles");
}

int ls_affine_tile() { return LS_AFFINE_TILE; }
int ls_affine_group(int nd, int dtype) {
  // tiles per wave of the CONST kernels: dtype 0 = f32, 1 = f64
  if (nd < 1 || nd > 16 || dtype < 0 || dtype > 1)
    throw std::runtime_error("affine_group: nd 1..16, real dtypes only");
  return affine_group(nd, dtype == 0 ? 4 : 8);
}
int ls_affine_const_f32_nd() { return LS_AFFINE_CONST_F32_ND; }

void ls_spmv_rows(uintptr_t rows_list, i64 n_list, uintptr_t indptr,
                  uintptr_t indices, uintptr_t vals, uintptr_t x,
                  uintptr_t y, int dtype, int idx_dtype, bool accumulate,
                  uintptr_t stream) {
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const int grid = grid_1d(n_list, LS_THREADS, 4096);
  DISPATCH_VAL_T(dtype, DISPATCH_IDX_T(idx_dtype, hipLaunchKernelGGL(
      (spmv_rows_kernel<val_t, idx_t>), dim3(grid), dim3(LS_THREADS), 0,
      s, reinterpret_cast<const i64*>(rows_list), n_list,
      reinterpret_cast<const i64*>(indptr),
      reinterpret_cast<const idx_t*>(indices),
      reinterpret_cast<const val_t*>(vals),
      reinterpret_cast<const val_t*>(x), reinterpret_cast<val_t*>(y),
      accumulate ? 1 : 0)));
  ls_check(hipGetLastError(), "spmv_rows");
}

void ls_spmv(uintptr_t indptr, uintptr_t indices, uintptr_t vals,
             uintptr_t x, uintptr_t y, i64 n_rows, i64 nnz, int dtype,
             int idx_dtype, bool accumulate, uintptr_t stream,
             int w_override, bool nt, int pair_mode, int swz_mode,
             i64 max_nnz) {
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  DISPATCH_VAL_T(dtype, DISPATCH_IDX_T(idx_dtype, (
      spmv_launch<val_t, idx_t>(
          reinterpret_cast<const i64*>(indptr),
          reinterpret_cast<const idx_t*>(indices),
          reinterpret_cast<const val_t*>(vals),
          reinterpret_cast<const val_t*>(x), reinterpret_cast<val_t*>(y),
          n_rows, nnz, accumulate, w_override, nt, pair_mode, swz_mode,
          max_nnz, s))));
}

// (kernel name, W) that ls_spmv would run for these arguments
// (module.cpp: spmv_select); no launch
void ls_spmv_select(i64 n_rows, i64 nnz, int dtype, bool accumulate,
                    int w_override, bool nt, int pair_mode, int swz_mode,
                    i64 max_nnz, const char** name, int* W) {
  if (dtype < 0 || dtype > 3) throw std::runtime_error("bad dtype code");
  const SpmvChoice ch = spmv_select(n_rows, nnz, dtype <= 1, accumulate,
                                    w_override, nt, pair_mode, swz_mode,
                                    max_nnz);
  *name = spmv_kind_name(ch.kind);
  *W = ch.W;
}

// SPDX-License-Identifier: Apache-2.0
// Hash-based Gustavson SpGEMM for gfx950.
//
// Replaces the reference's cuSPARSE 3-phase path
// (spgemm_csr_csr_csr.cu:196-332) with a 2-phase LDS-hash design:
//
//   phase 0  row_upper_bound: ub[i] = sum of B-row lengths over A's row i
//   phase 1  symbolic: per C-row distinct-column count via LDS hash insert
//   phase 2  numeric:  hash insert + accumulate, in-LDS bitonic sort,
//            coalesced sorted write-out (no global sort pass — profiling
//            showed a rocprim canonical sort costing more than the numeric
//            phase itself)
//
// Rows are binned by ub so the hash table fits LDS (160 KiB/CU):
//   cfg0: ub <=   48 —  8 lanes/row, 32 rows/block,   64-slot table
//   cfg1: ub <=  128 — 16 lanes/row, 16 rows/block,  256-slot table
//   cfg2: ub <= 1024 —  1 wave/row,   2 rows/block, 2048-slot table
//   cfg3: ub <= 4096 —  1 block/row,               8192-slot table
//   global bin (ub > 4096): per-row power-of-two table in HBM workspace,
//     compacted unsorted (host sorts those rows; they are rare).
//
// Column ids hash as uint32 (B.cols < 2^32, asserted in Python); tables
// are linear-probed, empty slot = 0xFFFFFFFF (sorts to the end, so the
// bitonic pass needs no size specialization).

#include "common.h"

#include <cstdlib>

namespace {

constexpr uint32_t EMPTY = 0xFFFFFFFFu;

__device__ inline uint32_t hash1(uint32_t col, uint32_t mask) {
  return (col * 2654435761u) & mask;
}

// Insert col; returns true if newly inserted (symbolic counting).
__device__ inline bool tbl_insert(uint32_t* tbl, uint32_t mask,
                                  uint32_t col) {
  uint32_t h = hash1(col, mask);
  while (true) {
    uint32_t cur = tbl[h];
    if (cur == col) return false;
    if (cur == EMPTY) {
      uint32_t prev = atomicCAS(&tbl[h], EMPTY, col);
      if (prev == EMPTY) return true;
      if (prev == col) return false;
    }
    h = (h + 1) & mask;
  }
}

// Find or claim the slot of col (numeric accumulate path).
__device__ inline uint32_t tbl_find_or_insert(uint32_t* tbl, uint32_t mask,
                                              uint32_t col) {
  uint32_t h = hash1(col, mask);
  while (true) {
    uint32_t cur = tbl[h];
    if (cur == col) return h;
    if (cur == EMPTY) {
      uint32_t prev = atomicCAS(&tbl[h], EMPTY, col);
      if (prev == EMPTY || prev == col) return h;
    }
    h = (h + 1) & mask;
  }
}

__device__ inline void atomic_add_val(float* p, float v) { atomicAdd(p, v); }
__device__ inline void atomic_add_val(double* p, double v) { atomicAdd(p, v); }
template <typename T>
__device__ inline void atomic_add_val(Cplx<T>* p, Cplx<T> v) {
  atomicAdd(&p->re, v.re);
  atomicAdd(&p->im, v.im);
}

// ---------------------------------------------------------------------------
// phase 0: upper bound per row
// ---------------------------------------------------------------------------
template <typename I>
__global__ __launch_bounds__(LS_THREADS) void row_ub_kernel(
    const i64* __restrict__ A_indptr, const I* __restrict__ A_indices,
    const i64* __restrict__ B_indptr, i64* __restrict__ ub, i64 n_rows) {
  constexpr int W = 4;
  constexpr int RPB = LS_THREADS / W;
  const int group = threadIdx.x / W;
  const int lane = threadIdx.x % W;
  const i64 stride = (i64)gridDim.x * RPB;
  for (i64 row = (i64)blockIdx.x * RPB + group; row < n_rows; row += stride) {
    i64 acc = 0;
    for (i64 jp = A_indptr[row] + lane; jp < A_indptr[row + 1]; jp += W) {
      const i64 k = (i64)A_indices[jp];
      acc += B_indptr[k + 1] - B_indptr[k];
    }
    acc = group_reduce_sum<i64, W>(acc);
    if (lane == 0) ub[row] = acc;
  }
}

// ---------------------------------------------------------------------------
// LDS-hash symbolic/numeric, parameterized on (BLOCK, ROWS_PER_BLOCK, TBL).
// One row per thread-group (W = BLOCK/ROWS threads); exactly one row per
// group per launch index (no grid-stride) and compile-time loop bounds, so
// every __syncthreads() is uniform across the block.
// ---------------------------------------------------------------------------
template <typename I, int BLOCK, int ROWS, int TBL>
__global__ __launch_bounds__(BLOCK) void spgemm_symbolic_lds_kernel(
    const i64* __restrict__ rows_list, i64 n_bin_rows,
    const i64* __restrict__ A_indptr, const I* __restrict__ A_indices,
    const i64* __restrict__ B_indptr, const I* __restrict__ B_indices,
    i64* __restrict__ row_nnz) {
  constexpr int W = BLOCK / ROWS;
  __shared__ uint32_t tbl[ROWS][TBL];
  __shared__ int cnt[ROWS];
  const int group = threadIdx.x / W;
  const int lane = threadIdx.x % W;
  const i64 idx = (i64)blockIdx.x * ROWS + group;
  for (int t = lane; t < TBL; t += W) tbl[group][t] = EMPTY;
  if (lane == 0) cnt[group] = 0;
  __syncthreads();
  if (idx < n_bin_rows) {
    const i64 row = rows_list[idx];
    int local = 0;
    for (i64 jp = A_indptr[row] + lane; jp < A_indptr[row + 1]; jp += W) {
      const i64 k = (i64)A_indices[jp];
      for (i64 kp = B_indptr[k]; kp < B_indptr[k + 1]; ++kp) {
        if (tbl_insert(tbl[group], TBL - 1, (uint32_t)B_indices[kp]))
          ++local;
      }
    }
    atomicAdd(&cnt[group], local);
  }
  __syncthreads();
  if (idx < n_bin_rows && lane == 0) row_nnz[rows_list[idx]] = cnt[group];
}

template <typename T, typename I, int BLOCK, int ROWS, int TBL,
          bool COUNT, int ABL = 0>
__global__ __launch_bounds__(BLOCK) void spgemm_numeric_lds_kernel(
    const i64* __restrict__ rows_list, i64 n_bin_rows,
    const i64* __restrict__ A_indptr, const I* __restrict__ A_indices,
    const T* __restrict__ A_vals, const i64* __restrict__ B_indptr,
    const I* __restrict__ B_indices, const T* __restrict__ B_vals,
    const i64* __restrict__ C_indptr, I* __restrict__ C_indices,
    T* __restrict__ C_vals, i64* __restrict__ row_nnz_out) {
  constexpr int W = BLOCK / ROWS;
  __shared__ uint32_t keys[ROWS][TBL];
  __shared__ T vals[ROWS][TBL];
  __shared__ int cnt[ROWS];
  const int group = threadIdx.x / W;
  const int lane = threadIdx.x % W;
  const i64 idx = (i64)blockIdx.x * ROWS + group;
  // pre-zero both tables: any lane may then atomicAdd into a slot another
  // lane just claimed, with no init race
  for (int t = lane; t < TBL; t += W) {
    keys[group][t] = EMPTY;
    vals[group][t] = ls_zero<T>();
  }
  if (COUNT && lane == 0) cnt[group] = 0;
  __syncthreads();
  if (idx < n_bin_rows) {
    const i64 row = rows_list[idx];
    int fresh_cnt = 0;
    for (i64 jp = A_indptr[row] + lane; jp < A_indptr[row + 1]; jp += W) {
      const i64 k = (i64)A_indices[jp];
      const T a = A_vals[jp];
      for (i64 kp = B_indptr[k]; kp < B_indptr[k + 1]; ++kp) {
        const uint32_t col = (uint32_t)B_indices[kp];
        if constexpr (COUNT) {
          uint32_t h = hash1(col, TBL - 1);
          uint32_t slot;
          while (true) {
            uint32_t cur = keys[group][h];
            if (cur == col) { slot = h; break; }
            if (cur == EMPTY) {
              uint32_t prev = atomicCAS(&keys[group][h], EMPTY, col);
              if (prev == EMPTY) { slot = h; ++fresh_cnt; break; }
              if (prev == col) { slot = h; break; }
            }
            h = (h + 1) & (TBL - 1);
          }
          if constexpr (ABL == 2)
            vals[group][slot] = a * B_vals[kp];
          else
            atomic_add_val(&vals[group][slot], a * B_vals[kp]);
        } else {
          const uint32_t slot = tbl_find_or_insert(
              keys[group], TBL - 1, col);
          if constexpr (ABL == 2)
            vals[group][slot] = a * B_vals[kp];
          else
            atomic_add_val(&vals[group][slot], a * B_vals[kp]);
        }
      }
    }
    if constexpr (COUNT) atomicAdd(&cnt[group], fresh_cnt);
  }
  __syncthreads();
  // in-place bitonic sort of (keys, vals) over the whole table; EMPTY
  // (0xFFFFFFFF) sorts to the end, so the live entries end up as a sorted
  // prefix.  Compile-time bounds -> uniform barriers.
#pragma unroll 1
  for (int k = 2; ABL == 0 && k <= TBL; k <<= 1) {
#pragma unroll 1
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int t = threadIdx.x % W; t < TBL; t += W) {
        const int tj = t ^ j;
        if (tj > t) {
          const bool up = ((t & k) == 0);
          const uint32_t a = keys[group][t];
          const uint32_t b = keys[group][tj];
          if ((a > b) == up) {
            keys[group][t] = b;
            keys[group][tj] = a;
            const T tv = vals[group][t];
            vals[group][t] = vals[group][tj];
            vals[group][tj] = tv;
          }
        }
      }
      // each group's table is touched only by its own W lanes; when the
      // group fits one wave (W <= 64: cfg0-2) lockstep + in-order LDS
      // makes a block barrier unnecessary — a compiler fence suffices.
      // Measured: the block barriers were 20.7 of 24.3 ms of the Poisson
      // numeric phase (LS_SPGEMM_ABLATE).
      if constexpr (W <= 64)
        __builtin_amdgcn_wave_barrier();
      else
        __syncthreads();
    }
  }
  if (idx < n_bin_rows) {
    const i64 row = rows_list[idx];
    const i64 base = C_indptr[row];
    const i64 n_out = COUNT ? (i64)cnt[group] : C_indptr[row + 1] - base;
    for (i64 t = lane; t < n_out; t += W) {
      C_indices[base + t] = (I)keys[group][t];
      C_vals[base + t] = vals[group][t];
    }
    if (COUNT && lane == 0) row_nnz_out[row] = n_out;
  }
}

// ---------------------------------------------------------------------------
// Global-memory hash bin (ub > LDS capacity): one 256-thread block per row,
// per-row power-of-two table region in workspace (keys pre-filled 0xFF,
// vals pre-zeroed by the host).  Output UNSORTED; host post-sorts these
// rare rows.
// ---------------------------------------------------------------------------
// One-pass row binning: bin id from (a_len, ub) thresholds, per-bin
// counts, then scatter compaction — replaces a bucketize+argsort+
// bincount chain of ~15 small torch launches + a host sync.
// Bins: 0-2 merge (a_len <= 8/32/64 and ub <= 4096), 3-6 LDS hash by ub
// (<=48/128/1024/4096), 7 global.  Order within a bin is arbitrary
// (rows are independent).
// ---------------------------------------------------------------------------
constexpr int N_BINS = 8;

__device__ inline int row_bin(i64 alen, i64 ubv) {
  if (ubv <= 4096 && alen <= 64) {
    if (alen <= 8) return 0;
    if (alen <= 32) return 1;
    return 2;
  }
  if (ubv <= 48) return 3;
  if (ubv <= 128) return 4;
  if (ubv <= 1024) return 5;
  if (ubv <= 4096) return 6;
  return 7;
}

// ---------------------------------------------------------------------------
// AFFINE x AFFINE product: when A rows are {row + DA[a]} and B rows are
// {row + DB[b]} (stencil/banded operators), C's columns are the sorted
// sum-set E = unique(DA + DB) and the numeric phase is a register/LDS
// convolution — no hash tables, no index-stream reads, sorted output by
// construction.  Valid rows are precomputed host-side (validC: A row
// affine, every touched B row affine, output columns in range);
// exception rows run through the general Gustavson path and are merged.
// Accumulators live in LDS (dynamic slot indexing would spill registers);
// layout acc[slot * LS_THREADS + tid] is bank-conflict-free.
// ---------------------------------------------------------------------------
template <typename T, typename I>
__global__ __launch_bounds__(LS_THREADS) void spgemm_affine_kernel(
    const i64* __restrict__ A_ip, const T* __restrict__ A_vals,
    const i64* __restrict__ B_ip, const T* __restrict__ B_vals,
    const int* __restrict__ DA, int ndA, int ndB,
    const short* __restrict__ pair_slot, int nE,
    const int* __restrict__ E,
    const unsigned char* __restrict__ validC,
    const i64* __restrict__ C_ip, I* __restrict__ C_idx,
    T* __restrict__ C_vals, i64 n_rows) {
  extern __shared__ char smem_raw[];
  T* acc = reinterpret_cast<T*>(smem_raw);
  // nE is bounded by the accumulator budget of spgemm_affine_try (51 KB /
  // (LS_THREADS * sizeof(T))): 51 for 4-byte values
  __shared__ int E_s[64];
  __shared__ short ps_s[16 * 16];
  if (threadIdx.x < nE) E_s[threadIdx.x] = E[threadIdx.x];
  if (threadIdx.x < ndA * ndB) ps_s[threadIdx.x] = pair_slot[threadIdx.x];
  __syncthreads();
  const int tid = threadIdx.x;
  const int lane = tid % WAVE_SIZE;
  const i64 stride = (i64)gridDim.x * blockDim.x;
  // uniform outer loop (every thread iterates the same count so the
  // wave-cooperative writeback can synchronize safely)
  for (i64 base_it = (i64)blockIdx.x * blockDim.x; base_it < n_rows;
       base_it += stride) {
    const i64 row = base_it + tid;
    const bool ok = row < n_rows && validC[row];
    if (ok) {
      for (int t = 0; t < nE; ++t)
        acc[t * LS_THREADS + tid] = ls_zero<T>();
      const i64 sA = A_ip[row];
      for (int a = 0; a < ndA; ++a) {
        const i64 k = row + DA[a];
        const i64 sB = B_ip[k];
        const T va = A_vals[sA + a];
        const short* ps = ps_s + a * ndB;
        for (int b = 0; b < ndB; ++b)
          acc[(int)ps[b] * LS_THREADS + tid] += va * B_vals[sB + b];
      }
    }
    // writeback: when a whole wave's 64 consecutive rows are valid,
    // the wave's C region [C_ip[w0], C_ip[w0+64]) is one contiguous
    // span of 64*nE elements — copy it coalesced (element e -> row
    // e/nE, slot e%nE from the LDS accumulators) instead of each lane
    // scattering nE-strided stores across 64 cache lines
    __builtin_amdgcn_wave_barrier();  // LDS acc: cross-lane reads below
    const unsigned long long ball =
        __ballot(static_cast<int>(ok));
    if (ball == ~0ull) {
      const i64 w0 = row - lane;
      const int wbase = tid - lane;
      const i64 span0 = C_ip[w0];
      const int total = WAVE_SIZE * nE;
      for (int e = lane; e < total; e += WAVE_SIZE) {
        const int rr = e / nE;
        const int ss = e - rr * nE;
        C_idx[span0 + e] = (I)(w0 + rr + E_s[ss]);
        C_vals[span0 + e] = acc[ss * LS_THREADS + wbase + rr];
      }
    } else if (ok) {
      const i64 cb = C_ip[row];
      for (int t = 0; t < nE; ++t) {
        C_idx[cb + t] = (I)(row + E_s[t]);
        C_vals[cb + t] = acc[t * LS_THREADS + tid];
      }
    }
  }
}

// fused phase 0: ub + bin histogram in ONE pass over A (saves the
// separate bin_count kernel's full re-read of indptr+ub and a launch)
template <typename I>
__global__ __launch_bounds__(LS_THREADS) void row_ub_bins_kernel(
    const i64* __restrict__ A_indptr, const I* __restrict__ A_indices,
    const i64* __restrict__ B_indptr, i64* __restrict__ ub, i64 n_rows,
    i64* __restrict__ counts) {
  constexpr int W = 4;
  constexpr int RPB = LS_THREADS / W;
  __shared__ i64 loc[N_BINS];
  if (threadIdx.x < N_BINS) loc[threadIdx.x] = 0;
  __syncthreads();
  const int group = threadIdx.x / W;
  const int lane = threadIdx.x % W;
  const i64 stride = (i64)gridDim.x * RPB;
  for (i64 row = (i64)blockIdx.x * RPB + group; row < n_rows;
       row += stride) {
    const i64 s = A_indptr[row];
    const i64 e = A_indptr[row + 1];
    i64 acc = 0;
    for (i64 jp = s + lane; jp < e; jp += W) {
      const i64 k = (i64)A_indices[jp];
      acc += B_indptr[k + 1] - B_indptr[k];
    }
    acc = group_reduce_sum<i64, W>(acc);
    if (lane == 0) {
      ub[row] = acc;
      atomicAdd(reinterpret_cast<unsigned long long*>(
                    &loc[row_bin(e - s, acc)]), 1ull);
    }
  }
  __syncthreads();
  if (threadIdx.x < N_BINS && loc[threadIdx.x])
    atomicAdd(reinterpret_cast<unsigned long long*>(&counts[threadIdx.x]),
              (unsigned long long)loc[threadIdx.x]);
}

__global__ __launch_bounds__(LS_THREADS) void spgemm_bin_count_kernel(
    const i64* __restrict__ A_indptr, const i64* __restrict__ ub,
    i64 n_rows, i64* __restrict__ counts) {
  __shared__ i64 loc[N_BINS];
  if (threadIdx.x < N_BINS) loc[threadIdx.x] = 0;
  __syncthreads();
  const i64 stride = (i64)gridDim.x * blockDim.x;
  for (i64 r = (i64)blockIdx.x * blockDim.x + threadIdx.x; r < n_rows;
       r += stride) {
    const int b = row_bin(A_indptr[r + 1] - A_indptr[r], ub[r]);
    atomicAdd(reinterpret_cast<unsigned long long*>(&loc[b]), 1ull);
  }
  __syncthreads();
  if (threadIdx.x < N_BINS && loc[threadIdx.x])
    atomicAdd(reinterpret_cast<unsigned long long*>(&counts[threadIdx.x]),
              (unsigned long long)loc[threadIdx.x]);
}

__global__ __launch_bounds__(LS_THREADS) void spgemm_bin_scatter_kernel(
    const i64* __restrict__ A_indptr, const i64* __restrict__ ub,
    i64 n_rows, i64* __restrict__ cursors, i64* __restrict__ rows_out) {
  // two-pass per-block aggregation: ONE global atomicAdd per bin per
  // block (a naive per-row atomic on 8 shared cursors serializes at
  // ~88 ops/us — 0.2 s for 16.7M rows)
  __shared__ i64 cnt[N_BINS];
  __shared__ i64 base[N_BINS];
  const i64 chunk = (n_rows + gridDim.x - 1) / gridDim.x;
  const i64 r0 = (i64)blockIdx.x * chunk;
  const i64 r1 = min(r0 + chunk, n_rows);
  if (threadIdx.x < N_BINS) cnt[threadIdx.x] = 0;
  __syncthreads();
  for (i64 r = r0 + threadIdx.x; r < r1; r += blockDim.x) {
    const int b = row_bin(A_indptr[r + 1] - A_indptr[r], ub[r]);
    atomicAdd(reinterpret_cast<unsigned long long*>(&cnt[b]), 1ull);
  }
  __syncthreads();
  if (threadIdx.x < N_BINS) {
    base[threadIdx.x] = (i64)atomicAdd(
        reinterpret_cast<unsigned long long*>(&cursors[threadIdx.x]),
        (unsigned long long)cnt[threadIdx.x]);
    cnt[threadIdx.x] = 0;
  }
  __syncthreads();
  for (i64 r = r0 + threadIdx.x; r < r1; r += blockDim.x) {
    const int b = row_bin(A_indptr[r + 1] - A_indptr[r], ub[r]);
    const i64 pos = (i64)atomicAdd(
        reinterpret_cast<unsigned long long*>(&cnt[b]), 1ull);
    rows_out[base[b] + pos] = r;
  }
}

// Copy per-row segments from a capacity layout into the final CSR
// arrays (hybrid merge-fast compaction): one W-lane group per row,
// coalesced, 2x row bytes of traffic.
template <typename T, typename I>
__global__ __launch_bounds__(LS_THREADS) void spgemm_compact_rows_kernel(
    const i64* __restrict__ rows_list, i64 n_bin_rows,
    const i64* __restrict__ src_off, const i64* __restrict__ dst_indptr,
    const I* __restrict__ src_idx, const T* __restrict__ src_val,
    I* __restrict__ dst_idx, T* __restrict__ dst_val) {
  constexpr int W = 8;
  constexpr int RPB = LS_THREADS / W;
  const int group = threadIdx.x / W;
  const int lane = threadIdx.x % W;
  const i64 stride = (i64)gridDim.x * RPB;
  for (i64 i = (i64)blockIdx.x * RPB + group; i < n_bin_rows; i += stride) {
    const i64 row = rows_list[i];
    const i64 s = src_off[row];
    const i64 d = dst_indptr[row];
    const i64 m = dst_indptr[row + 1] - d;
    for (i64 t = lane; t < m; t += W) {
      dst_idx[d + t] = src_idx[s + t];
      dst_val[d + t] = src_val[s + t];
    }
  }
}

// ---------------------------------------------------------------------------
// Register k-way MERGE path for rows with few A-entries (a_len <= W) and
// bounded expansion: lane l owns A-entry l and walks its (sorted) B row;
// each output element is a wave-min over the lanes' cursors plus a masked
// contribution sum — no LDS, no atomics, no hash, sorted output for free.
// This covers every row of stencil-type operators (5-pt Poisson: a_len 5).
// ---------------------------------------------------------------------------
template <typename I, int W>
__device__ inline uint32_t grp_min_u32(uint32_t v) {
#pragma unroll
  for (int off = W / 2; off > 0; off >>= 1) {
    const uint32_t o = __shfl_xor(v, off, WAVE_SIZE);
    v = o < v ? o : v;
  }
  return v;
}

template <typename T, int W>
__device__ inline T grp_sum(T v) {
#pragma unroll
  for (int off = W / 2; off > 0; off >>= 1) {
    v += ls_shfl_down(v, off);
  }
  return v;  // valid in lane 0 of the group
}

template <typename I, int W>
__global__ __launch_bounds__(LS_THREADS) void spgemm_merge_symbolic_kernel(
    const i64* __restrict__ rows_list, i64 n_bin_rows,
    const i64* __restrict__ A_indptr, const I* __restrict__ A_indices,
    const i64* __restrict__ B_indptr, const I* __restrict__ B_indices,
    i64* __restrict__ row_nnz) {
  constexpr int ROWS = LS_THREADS / W;
  const int group = threadIdx.x / W;
  const int lane = threadIdx.x % W;
  const i64 idx = (i64)blockIdx.x * ROWS + group;
  if (idx >= n_bin_rows) return;
  const i64 row = rows_list[idx];
  const i64 s = A_indptr[row];
  const int alen = (int)(A_indptr[row + 1] - s);
  i64 kp = 0, kend = 0;
  if (lane < alen) {
    const i64 k = (i64)A_indices[s + lane];
    kp = B_indptr[k];
    kend = B_indptr[k + 1];
  }
  uint32_t mycol = (lane < alen && kp < kend) ? (uint32_t)B_indices[kp]
                                              : EMPTY;
  i64 cnt = 0;
  while (true) {
    const uint32_t mn = grp_min_u32<I, W>(mycol);
    if (mn == EMPTY) break;
    ++cnt;
    if (mycol == mn) {
      ++kp;
      mycol = (kp < kend) ? (uint32_t)B_indices[kp] : EMPTY;
    }
  }
  if (lane == 0) row_nnz[row] = cnt;
}

template <typename T, typename I, int W, bool COUNT>
__global__ __launch_bounds__(LS_THREADS) void spgemm_merge_numeric_kernel(
    const i64* __restrict__ rows_list, i64 n_bin_rows,
    const i64* __restrict__ A_indptr, const I* __restrict__ A_indices,
    const T* __restrict__ A_vals, const i64* __restrict__ B_indptr,
    const I* __restrict__ B_indices, const T* __restrict__ B_vals,
    const i64* __restrict__ C_indptr, I* __restrict__ C_indices,
    T* __restrict__ C_vals, i64* __restrict__ row_nnz_out) {
  constexpr int ROWS = LS_THREADS / W;
  const int group = threadIdx.x / W;
  const int lane = threadIdx.x % W;
  const i64 idx = (i64)blockIdx.x * ROWS + group;
  if (idx >= n_bin_rows) return;
  const i64 row = rows_list[idx];
  const i64 s = A_indptr[row];
  const int alen = (int)(A_indptr[row + 1] - s);
  i64 kp = 0, kend = 0;
  T a = ls_zero<T>();
  if (lane < alen) {
    const i64 k = (i64)A_indices[s + lane];
    a = A_vals[s + lane];
    kp = B_indptr[k];
    kend = B_indptr[k + 1];
  }
  uint32_t mycol = (lane < alen && kp < kend) ? (uint32_t)B_indices[kp]
                                              : EMPTY;
  T myval = (mycol != EMPTY) ? B_vals[kp] : ls_zero<T>();
  const i64 base = C_indptr[row];
  i64 out = 0;
  while (true) {
    const uint32_t mn = grp_min_u32<I, W>(mycol);
    if (mn == EMPTY) break;
    T contrib = (mycol == mn) ? a * myval : ls_zero<T>();
    contrib = grp_sum<T, W>(contrib);
    if (lane == 0) {
      C_indices[base + out] = (I)mn;
      C_vals[base + out] = contrib;
    }
    ++out;
    if (mycol == mn) {
      ++kp;
      if (kp < kend) {
        mycol = (uint32_t)B_indices[kp];
        myval = B_vals[kp];
      } else {
        mycol = EMPTY;
      }
    }
  }
  if (COUNT && lane == 0) row_nnz_out[row] = out;
}

// Lane-per-row SCALAR merge for the shortest-A bin (a_len <= 8): all 8
// merge heads live in registers and the k-way min / accumulate runs as
// straight-line per-lane code — no shuffles, no cross-lane dependency
// chains, 64 rows per wave.  The wave-merge kernel spends ~10 wave ops
// per OUTPUT element on a grp_min→grp_sum latency chain; here the same
// output costs unrolled VALU with 8-deep ILP.  Memory stays friendly on
// banded/stencil matrices: adjacent lanes hold adjacent rows, whose
// k-th B rows are adjacent in memory.  Selected by LS_SPGEMM_SCALAR.
template <typename T, typename I, bool COUNT>
__global__ __launch_bounds__(LS_THREADS) void spgemm_merge_scalar_kernel(
    const i64* __restrict__ rows_list, i64 n_bin_rows,
    const i64* __restrict__ A_indptr, const I* __restrict__ A_indices,
    const T* __restrict__ A_vals, const i64* __restrict__ B_indptr,
    const I* __restrict__ B_indices, const T* __restrict__ B_vals,
    const i64* __restrict__ C_indptr, I* __restrict__ C_indices,
    T* __restrict__ C_vals, i64* __restrict__ row_nnz_out) {
  constexpr int MAXA = 8;
  const i64 idx = (i64)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= n_bin_rows) return;
  const i64 row = rows_list[idx];
  const i64 s = A_indptr[row];
  const int alen = (int)(A_indptr[row + 1] - s);
  i64 kp[MAXA], kend[MAXA];
  T a[MAXA], hval[MAXA];
  uint32_t hcol[MAXA];
#pragma unroll
  for (int h = 0; h < MAXA; ++h) {
    kp[h] = 0;
    kend[h] = 0;
    a[h] = ls_zero<T>();
    hval[h] = ls_zero<T>();
    hcol[h] = EMPTY;
    if (h < alen) {
      const i64 k = (i64)A_indices[s + h];
      a[h] = A_vals[s + h];
      kp[h] = B_indptr[k];
      kend[h] = B_indptr[k + 1];
      if (kp[h] < kend[h]) {
        hcol[h] = (uint32_t)B_indices[kp[h]];
        hval[h] = B_vals[kp[h]];
      }
    }
  }
  const i64 base = C_indptr[row];
  i64 out = 0;
  while (true) {
    uint32_t mn = hcol[0];
#pragma unroll
    for (int h = 1; h < MAXA; ++h) mn = hcol[h] < mn ? hcol[h] : mn;
    if (mn == EMPTY) break;
    T acc = ls_zero<T>();
#pragma unroll
    for (int h = 0; h < MAXA; ++h) {
      if (hcol[h] == mn) {
        acc += a[h] * hval[h];
        ++kp[h];
        if (kp[h] < kend[h]) {
          hcol[h] = (uint32_t)B_indices[kp[h]];
          hval[h] = B_vals[kp[h]];
        } else {
          hcol[h] = EMPTY;
        }
      }
    }
    C_indices[base + out] = (I)mn;
    C_vals[base + out] = acc;
    ++out;
  }
  if (COUNT) row_nnz_out[row] = out;
}

// Compact-then-sort numeric kernel for wave-contained groups (W <= 64):
// hash-accumulate into the table, compact live entries to a second LDS
// region, then bitonic-sort only pow2ceil(cnt) elements (full-table
// sorting measured 20.7 of 24.3 ms on Poisson — LS_SPGEMM_ABLATE).
template <typename T, typename I, int BLOCK, int ROWS, int TBL, bool COUNT,
          int ABL = 0, bool PACK = false>
__global__ __launch_bounds__(BLOCK) void spgemm_numeric_lds_csort_kernel(
    const i64* __restrict__ rows_list, i64 n_bin_rows,
    const i64* __restrict__ A_indptr, const I* __restrict__ A_indices,
    const T* __restrict__ A_vals, const i64* __restrict__ B_indptr,
    const I* __restrict__ B_indices, const T* __restrict__ B_vals,
    const i64* __restrict__ C_indptr, I* __restrict__ C_indices,
    T* __restrict__ C_vals, i64* __restrict__ row_nnz_out) {
  constexpr int W = BLOCK / ROWS;
  static_assert(W <= 64, "groups must be wave-contained");
  constexpr int PACK_BITS = 8;  // slot index bits; requires TBL <= 256
  static_assert(!PACK || TBL <= (1 << PACK_BITS), "PACK needs small TBL");
  __shared__ uint32_t keys[ROWS][TBL];
  __shared__ T vals[ROWS][TBL];
  __shared__ uint32_t okeys[ROWS][TBL];
  // PACK keeps the TABLE slot in the key's low bits, so no second value
  // buffer is needed (smaller LDS -> more blocks per CU)
  __shared__ T ovals[ROWS][PACK ? 1 : TBL];
  __shared__ int cur[ROWS];
  const int group = threadIdx.x / W;
  const int lane = threadIdx.x % W;
  const i64 idx = (i64)blockIdx.x * ROWS + group;
  for (int t = lane; t < TBL; t += W) {
    keys[group][t] = EMPTY;
    vals[group][t] = ls_zero<T>();
  }
  if (lane == 0) cur[group] = 0;
  __builtin_amdgcn_wave_barrier();
  if (idx < n_bin_rows) {
    const i64 row = rows_list[idx];
    for (i64 jp = A_indptr[row] + lane; jp < A_indptr[row + 1]; jp += W) {
      const i64 k = (i64)A_indices[jp];
      const T a = A_vals[jp];
      for (i64 kp = B_indptr[k]; kp < B_indptr[k + 1]; ++kp) {
        const uint32_t slot = tbl_find_or_insert(
            keys[group], TBL - 1, (uint32_t)B_indices[kp]);
        atomic_add_val(&vals[group][slot], a * B_vals[kp]);
      }
    }
  }
  __builtin_amdgcn_wave_barrier();
  if constexpr (ABL == 3) {  // ablation: keep table live, skip the rest
    if (lane == 0 && keys[group][0] == 1234567u) C_vals[0] = vals[group][0];
    return;
  }
  // compact live entries to the front of okeys (+ovals without PACK).
  // PACK keeps the TABLE slot in the key's low bits so the sort permutes
  // one u32 array and values never move.
  for (int t = lane; t < TBL; t += W) {
    const uint32_t c = keys[group][t];
    if (c != EMPTY) {
      const int at = atomicAdd(&cur[group], 1);
      if constexpr (PACK) {
        okeys[group][at] = (c << PACK_BITS) | (uint32_t)t;
      } else {
        okeys[group][at] = c;
        ovals[group][at] = vals[group][t];
      }
    }
  }
  __builtin_amdgcn_wave_barrier();
  if constexpr (ABL == 4) {
    if (lane == 0 && okeys[group][0] == 1234567u) C_vals[0] = ovals[group][0];
    return;
  }
  const int m = cur[group];
  int P = 1;
  while (P < m) P <<= 1;
  // wave-uniform sort bound: divergent per-group loop bounds churn the
  // exec mask; sorting every group to the wave's max P is cheaper
  P = (int)wave_reduce_max_u32((uint32_t)P);
  for (int t = lane + m; t < P; t += W) okeys[group][t] = EMPTY;
  __builtin_amdgcn_wave_barrier();
#pragma unroll 1
  for (int k = 2; k <= P; k <<= 1) {
#pragma unroll 1
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int t = lane; t < P; t += W) {
        const int tj = t ^ j;
        if (tj > t) {
          const bool up = ((t & k) == 0);
          const uint32_t a = okeys[group][t];
          const uint32_t b = okeys[group][tj];
          if ((a > b) == up) {
            okeys[group][t] = b;
            okeys[group][tj] = a;
            if constexpr (!PACK) {
              const T tv = ovals[group][t];
              ovals[group][t] = ovals[group][tj];
              ovals[group][tj] = tv;
            }
          }
        }
      }
      __builtin_amdgcn_wave_barrier();
    }
  }
  if constexpr (ABL == 5) {
    if (lane == 0 && okeys[group][0] == 1234567u) C_vals[0] = ovals[group][0];
    return;
  }
  if (idx < n_bin_rows) {
    const i64 row = rows_list[idx];
    const i64 base = C_indptr[row];
    for (int t = lane; t < m; t += W) {
      if constexpr (PACK) {
        const uint32_t kk = okeys[group][t];
        C_indices[base + t] = (I)(kk >> PACK_BITS);
        C_vals[base + t] = vals[group][kk & (TBL - 1)];
      } else {
        C_indices[base + t] = (I)okeys[group][t];
        C_vals[base + t] = ovals[group][t];
      }
    }
    if (COUNT && lane == 0) row_nnz_out[row] = m;
  }
}

// ---------------------------------------------------------------------------
// Hub rows are CHUNKED over many workgroups (one workgroup per
// GLOBAL_CHUNK A-elements of a row) so a power-law row parallelizes
// across the chip; a separate compact kernel then walks each row's table.
constexpr int GLOBAL_CHUNK = 2048;

template <typename I>
__global__ __launch_bounds__(LS_THREADS) void spgemm_symbolic_global_kernel(
    const i64* __restrict__ rows_list,
    const i64* __restrict__ chunk_rowidx, const i64* __restrict__ chunk_ord,
    i64 n_chunks, const i64* __restrict__ A_indptr,
    const I* __restrict__ A_indices, const i64* __restrict__ B_indptr,
    const I* __restrict__ B_indices, uint32_t* __restrict__ tbl_ws,
    const i64* __restrict__ tbl_off, const i64* __restrict__ tbl_size,
    i64* __restrict__ row_nnz, int identity,
    const i64* __restrict__ blen_prefix, const i64* __restrict__ pref_base,
    const i64* __restrict__ a_len_g) {
  // Work is chunked by EXPANSION POSITION (not A-entry): thread e finds
  // its (A-entry, B-offset) by binary search in the row's B-length
  // prefix — hub rows with few A-entries but huge B-rows parallelize
  // fully instead of serializing a per-lane B walk.
  const i64 ch = blockIdx.x;
  if (ch >= n_chunks) return;
  const i64 idx = chunk_rowidx[ch];
  const i64 row = rows_list[idx];
  uint32_t* tbl = tbl_ws + tbl_off[idx];
  const uint32_t mask = (uint32_t)tbl_size[idx] - 1;
  const i64 pb = pref_base[idx];
  const i64 alen = a_len_g[idx];
  const i64 ub_row = alen ? blen_prefix[pb + alen - 1] : 0;
  const i64 e0 = chunk_ord[ch] * GLOBAL_CHUNK;
  const i64 e1 = min(e0 + GLOBAL_CHUNK, ub_row);
  const i64 a_base = A_indptr[row];
  __shared__ int cnt;
  if (threadIdx.x == 0) cnt = 0;
  __syncthreads();
  int local = 0;
  for (i64 e = e0 + threadIdx.x; e < e1; e += blockDim.x) {
    // smallest i with blen_prefix[pb+i] > e
    i64 lo = 0, hi = alen - 1;
    while (lo < hi) {
      const i64 mid = (lo + hi) >> 1;
      if (blen_prefix[pb + mid] > e)
        hi = mid;
      else
        lo = mid + 1;
    }
    const i64 b_off = e - (lo ? blen_prefix[pb + lo - 1] : 0);
    const i64 k = (i64)A_indices[a_base + lo];
    const uint32_t col = (uint32_t)B_indices[B_indptr[k] + b_off];
    if (identity) {
      if (tbl[col] != col && atomicCAS(&tbl[col], EMPTY, col) == EMPTY)
        ++local;
    } else if (tbl_insert(tbl, mask, col)) {
      ++local;
    }
  }
  atomicAdd(&cnt, local);
  __syncthreads();
  if (threadIdx.x == 0 && cnt)
    atomicAdd(reinterpret_cast<unsigned long long*>(&row_nnz[row]),
              (unsigned long long)cnt);
}

template <typename T, typename I>
__global__ __launch_bounds__(LS_THREADS) void spgemm_numeric_global_fill(
    const i64* __restrict__ rows_list,
    const i64* __restrict__ chunk_rowidx, const i64* __restrict__ chunk_ord,
    i64 n_chunks, const i64* __restrict__ A_indptr,
    const I* __restrict__ A_indices, const T* __restrict__ A_vals,
    const i64* __restrict__ B_indptr, const I* __restrict__ B_indices,
    const T* __restrict__ B_vals, uint32_t* __restrict__ key_ws,
    T* __restrict__ val_ws, const i64* __restrict__ tbl_off,
    const i64* __restrict__ tbl_size, int identity,
    const i64* __restrict__ blen_prefix, const i64* __restrict__ pref_base,
    const i64* __restrict__ a_len_g) {
  const i64 ch = blockIdx.x;
  if (ch >= n_chunks) return;
  const i64 idx = chunk_rowidx[ch];
  const i64 row = rows_list[idx];
  uint32_t* keys = key_ws + tbl_off[idx];
  T* vals = val_ws + tbl_off[idx];
  const uint32_t mask = (uint32_t)tbl_size[idx] - 1;
  const i64 pb = pref_base[idx];
  const i64 alen = a_len_g[idx];
  const i64 ub_row = alen ? blen_prefix[pb + alen - 1] : 0;
  const i64 e0 = chunk_ord[ch] * GLOBAL_CHUNK;
  const i64 e1 = min(e0 + GLOBAL_CHUNK, ub_row);
  const i64 a_base = A_indptr[row];
  for (i64 e = e0 + threadIdx.x; e < e1; e += blockDim.x) {
    i64 lo = 0, hi = alen - 1;
    while (lo < hi) {
      const i64 mid = (lo + hi) >> 1;
      if (blen_prefix[pb + mid] > e)
        hi = mid;
      else
        lo = mid + 1;
    }
    const i64 b_off = e - (lo ? blen_prefix[pb + lo - 1] : 0);
    const i64 k = (i64)A_indices[a_base + lo];
    const T a = A_vals[a_base + lo];
    const i64 bp0 = B_indptr[k] + b_off;
    const uint32_t col = (uint32_t)B_indices[bp0];
    uint32_t slot;
    if (identity) {
      slot = col;
      if (keys[col] != col) keys[col] = col;  // idempotent mark
    } else {
      slot = tbl_find_or_insert(keys, mask, col);
    }
    atomic_add_val(&vals[slot], a * B_vals[bp0]);
  }
}

template <typename T, typename I>
__global__ __launch_bounds__(LS_THREADS) void spgemm_global_compact(
    const i64* __restrict__ rows_list, i64 n_bin_rows,
    const uint32_t* __restrict__ key_ws, const T* __restrict__ val_ws,
    const i64* __restrict__ tbl_off, const i64* __restrict__ tbl_size,
    const i64* __restrict__ C_indptr, I* __restrict__ C_indices,
    T* __restrict__ C_vals, i64* __restrict__ row_nnz_out) {
  const i64 idx = blockIdx.x;
  if (idx >= n_bin_rows) return;
  const i64 row = rows_list[idx];
  const uint32_t* keys = key_ws + tbl_off[idx];
  const T* vals = val_ws + tbl_off[idx];
  const i64 sz = tbl_size[idx];
  __shared__ int cursor;
  if (threadIdx.x == 0) cursor = 0;
  __syncthreads();
  const i64 base = C_indptr[row];
  for (i64 t = threadIdx.x; t < sz; t += blockDim.x) {
    const uint32_t c = keys[t];
    if (c != EMPTY) {
      const int at = atomicAdd(&cursor, 1);
      C_indices[base + at] = (I)c;
      C_vals[base + at] = vals[t];
    }
  }
  __syncthreads();
  if (threadIdx.x == 0 && row_nnz_out != nullptr) row_nnz_out[row] = cursor;
}

// ---------------------------------------------------------------------------
// Launch helpers
// ---------------------------------------------------------------------------
template <typename I>
void symbolic_lds_dispatch(int cfg, const i64* rl, i64 n, const i64* ap,
                           const I* ai, const i64* bp, const I* bi,
                           i64* rn, hipStream_t s) {
  switch (cfg) {
    case 0:
      hipLaunchKernelGGL((spgemm_symbolic_lds_kernel<I, 256, 32, 64>),
                         dim3((n + 31) / 32), dim3(256), 0, s, rl, n, ap,
                         ai, bp, bi, rn);
      break;
    case 1:
      hipLaunchKernelGGL((spgemm_symbolic_lds_kernel<I, 256, 16, 256>),
                         dim3((n + 15) / 16), dim3(256), 0, s, rl, n, ap,
                         ai, bp, bi, rn);
      break;
    case 2:
      hipLaunchKernelGGL((spgemm_symbolic_lds_kernel<I, 128, 2, 2048>),
                         dim3((n + 1) / 2), dim3(128), 0, s, rl, n, ap, ai,
                         bp, bi, rn);
      break;
    default:
      hipLaunchKernelGGL((spgemm_symbolic_lds_kernel<I, 256, 1, 8192>),
                         dim3(n), dim3(256), 0, s, rl, n, ap, ai, bp, bi,
                         rn);
  }
}

template <typename T, typename I, bool COUNT>
void numeric_lds_dispatch(int cfg, const i64* rl, i64 n, const i64* ap,
                          const I* ai, const T* av, const i64* bp,
                          const I* bi, const T* bv, const i64* cp, I* ci,
                          T* cv, i64* rn, bool pack, hipStream_t s) {
  // cfg0-2 use the compact-then-sort kernel (double LDS buffers: 16-byte
  // value types shrink ROWS to stay under 160 KiB).  pack: sort a single
  // (col<<8|slot) u32 array instead of moving values (n_cols < 2^24-1).
  constexpr bool big = sizeof(T) > 8;
  switch (cfg) {
    case 0:
      if (pack)
        hipLaunchKernelGGL(
            (spgemm_numeric_lds_csort_kernel<T, I, 256, 32, 64, COUNT, 0,
                                             true>),
            dim3((n + 31) / 32), dim3(256), 0, s, rl, n, ap, ai, av, bp,
            bi, bv, cp, ci, cv, rn);
      else
        hipLaunchKernelGGL(
            (spgemm_numeric_lds_csort_kernel<T, I, 256, 32, 64, COUNT>),
            dim3((n + 31) / 32), dim3(256), 0, s, rl, n, ap, ai, av, bp,
            bi, bv, cp, ci, cv, rn);
      break;
    case 1:
      if constexpr (big) {
        if (pack)
          hipLaunchKernelGGL(
              (spgemm_numeric_lds_csort_kernel<T, I, 128, 8, 256, COUNT,
                                               0, true>),
              dim3((n + 7) / 8), dim3(128), 0, s, rl, n, ap, ai, av, bp,
              bi, bv, cp, ci, cv, rn);
        else
          hipLaunchKernelGGL(
              (spgemm_numeric_lds_csort_kernel<T, I, 128, 8, 256, COUNT>),
              dim3((n + 7) / 8), dim3(128), 0, s, rl, n, ap, ai, av, bp,
              bi, bv, cp, ci, cv, rn);
      } else {
        if (pack)
          hipLaunchKernelGGL(
              (spgemm_numeric_lds_csort_kernel<T, I, 256, 16, 256, COUNT,
                                               0, true>),
              dim3((n + 15) / 16), dim3(256), 0, s, rl, n, ap, ai, av,
              bp, bi, bv, cp, ci, cv, rn);
        else
          hipLaunchKernelGGL(
              (spgemm_numeric_lds_csort_kernel<T, I, 256, 16, 256,
                                               COUNT>),
              dim3((n + 15) / 16), dim3(256), 0, s, rl, n, ap, ai, av,
              bp, bi, bv, cp, ci, cv, rn);
      }
      break;
    case 2:
      if constexpr (big)
        hipLaunchKernelGGL(
            (spgemm_numeric_lds_csort_kernel<T, I, 64, 1, 2048, COUNT>),
            dim3(n), dim3(64), 0, s, rl, n, ap, ai, av, bp, bi, bv, cp,
            ci, cv, rn);
      else
        hipLaunchKernelGGL(
            (spgemm_numeric_lds_csort_kernel<T, I, 128, 2, 2048, COUNT>),
            dim3((n + 1) / 2), dim3(128), 0, s, rl, n, ap, ai, av, bp, bi,
            bv, cp, ci, cv, rn);
      break;
    default: {
      // 16-byte values (c128) at TBL=8192 exceed 160 KiB LDS; use 4096
      // slots there (bin cutoff is ub <= 4096: the table can be exactly
      // full — linear probing still terminates).
      constexpr int TBL3 = big ? 4096 : 8192;
      hipLaunchKernelGGL(
          (spgemm_numeric_lds_kernel<T, I, 256, 1, TBL3, COUNT>),
          dim3(n), dim3(256), 0, s, rl, n, ap, ai, av, bp, bi, bv, cp, ci,
          cv, rn);
    }
  }
}

template <typename T, typename I, int ABL>
void numeric_lds_dispatch_abl(int cfg, const i64* rl, i64 n, const i64* ap,
                              const I* ai, const T* av, const i64* bp,
                              const I* bi, const T* bv, const i64* cp,
                              I* ci, T* cv, i64* rn, hipStream_t s) {
  if constexpr (ABL >= 3) {
    // csort-kernel phase ablation (cfg0 geometry only; timing probes)
    hipLaunchKernelGGL(
        (spgemm_numeric_lds_csort_kernel<T, I, 256, 32, 64, false, ABL>),
        dim3((n + 31) / 32), dim3(256), 0, s, rl, n, ap, ai, av, bp, bi,
        bv, cp, ci, cv, rn);
    return;
  }
  switch (cfg) {
    case 0:
      hipLaunchKernelGGL(
          (spgemm_numeric_lds_kernel<T, I, 256, 32, 64, false, ABL>),
          dim3((n + 31) / 32), dim3(256), 0, s, rl, n, ap, ai, av, bp, bi,
          bv, cp, ci, cv, rn);
      break;
    case 1:
      hipLaunchKernelGGL(
          (spgemm_numeric_lds_kernel<T, I, 256, 16, 256, false, ABL>),
          dim3((n + 15) / 16), dim3(256), 0, s, rl, n, ap, ai, av, bp, bi,
          bv, cp, ci, cv, rn);
      break;
    case 2:
      hipLaunchKernelGGL(
          (spgemm_numeric_lds_kernel<T, I, 128, 2, 2048, false, ABL>),
          dim3((n + 1) / 2), dim3(128), 0, s, rl, n, ap, ai, av, bp, bi,
          bv, cp, ci, cv, rn);
      break;
    default: {
      constexpr int TBL3 = (sizeof(T) > 8) ? 4096 : 8192;
      hipLaunchKernelGGL(
          (spgemm_numeric_lds_kernel<T, I, 256, 1, TBL3, false, ABL>),
          dim3(n), dim3(256), 0, s, rl, n, ap, ai, av, bp, bi, bv, cp, ci,
          cv, rn);
    }
  }
}

template <typename T, typename I>
__global__ __launch_bounds__(LS_THREADS) void spgemm_global_compact_sorted(
    const i64* __restrict__ rows_list, i64 n_bin_rows,
    const uint32_t* __restrict__ key_ws, const T* __restrict__ val_ws,
    const i64* __restrict__ tbl_off, const i64* __restrict__ tbl_size,
    const i64* __restrict__ C_indptr, I* __restrict__ C_indices,
    T* __restrict__ C_vals, i64* __restrict__ row_nnz_out) {
  // ORDERED stream compaction for identity-hash rows (slot == col):
  // scanning slots in order emits ascending columns, so these rows never
  // need a host-side canonical sort (which at R-MAT scale 20 would
  // materialize ~70 GB index tensors).
  const i64 idx = blockIdx.x;
  if (idx >= n_bin_rows) return;
  const i64 row = rows_list[idx];
  const uint32_t* keys = key_ws + tbl_off[idx];
  const T* vals = val_ws + tbl_off[idx];
  const i64 sz = tbl_size[idx];
  constexpr int NW = LS_THREADS / WAVE_SIZE;
  __shared__ i64 running;
  __shared__ unsigned wave_tot[NW];
  if (threadIdx.x == 0) running = 0;
  __syncthreads();
  const int wave = threadIdx.x / WAVE_SIZE;
  const int lane = threadIdx.x % WAVE_SIZE;
  const i64 base = C_indptr[row];
  for (i64 tile = 0; tile < sz; tile += LS_THREADS) {
    const i64 t = tile + threadIdx.x;
    const bool live = (t < sz) && (keys[t] != EMPTY);
    const unsigned long long mask = __ballot(live);
    const unsigned prefix = (unsigned)__popcll(
        mask & ((1ull << lane) - 1ull));
    if (lane == 0) wave_tot[wave] = (unsigned)__popcll(mask);
    __syncthreads();
    unsigned wave_base = 0;
    for (int w = 0; w < wave; ++w) wave_base += wave_tot[w];
    if (live) {
      const i64 at = running + wave_base + prefix;
      C_indices[base + at] = (I)t;
      C_vals[base + at] = vals[t];
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      unsigned tot = 0;
      for (int w = 0; w < NW; ++w) tot += wave_tot[w];
      running += tot;
    }
    __syncthreads();
  }
  if (threadIdx.x == 0 && row_nnz_out != nullptr) row_nnz_out[row] = running;
}

}  // namespace

// ---------------------------------------------------------------------------
// Host entry points
// ---------------------------------------------------------------------------
namespace {
template <typename I>
void merge_symbolic_dispatch(int wcfg, const i64* rl, i64 n, const i64* ap,
                             const I* ai, const i64* bp, const I* bi,
                             i64* rn, hipStream_t s) {
  auto L = [&](auto wt) {
    constexpr int W = decltype(wt)::value;
    constexpr int ROWS = LS_THREADS / W;
    hipLaunchKernelGGL((spgemm_merge_symbolic_kernel<I, W>),
                       dim3((n + ROWS - 1) / ROWS), dim3(LS_THREADS), 0, s,
                       rl, n, ap, ai, bp, bi, rn);
  };
  if (wcfg == 0) L(std::integral_constant<int, 8>{});
  else if (wcfg == 1) L(std::integral_constant<int, 32>{});
  else L(std::integral_constant<int, 64>{});
}

inline bool scalar_merge_enabled() {
  static const bool on = [] {
    const char* e = std::getenv("LS_SPGEMM_SCALAR");
    return e && e[0] == '1';
  }();
  return on;
}

template <typename T, typename I, bool COUNT>
void merge_numeric_dispatch(int wcfg, const i64* rl, i64 n, const i64* ap,
                            const I* ai, const T* av, const i64* bp,
                            const I* bi, const T* bv, const i64* cp, I* ci,
                            T* cv, i64* rn, hipStream_t s) {
  if (wcfg == 0 && scalar_merge_enabled()) {
    hipLaunchKernelGGL((spgemm_merge_scalar_kernel<T, I, COUNT>),
                       dim3((n + LS_THREADS - 1) / LS_THREADS),
                       dim3(LS_THREADS), 0, s, rl, n, ap, ai, av, bp, bi,
                       bv, cp, ci, cv, rn);
    return;
  }
  auto L = [&](auto wt) {
    constexpr int W = decltype(wt)::value;
    constexpr int ROWS = LS_THREADS / W;
    hipLaunchKernelGGL((spgemm_merge_numeric_kernel<T, I, W, COUNT>),
                       dim3((n + ROWS - 1) / ROWS), dim3(LS_THREADS), 0, s,
                       rl, n, ap, ai, av, bp, bi, bv, cp, ci, cv, rn);
  };
  if (wcfg == 0) L(std::integral_constant<int, 8>{});
  else if (wcfg == 1) L(std::integral_constant<int, 32>{});
  else L(std::integral_constant<int, 64>{});
}
}  // namespace

void ls_spgemm_compact_rows(uintptr_t rows_list, i64 n,
                            uintptr_t src_off, uintptr_t dst_indptr,
                            uintptr_t src_idx, uintptr_t src_val,
                            uintptr_t dst_idx, uintptr_t dst_val,
                            int dtype, int idx_dtype, uintptr_t stream) {
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  DISPATCH_VAL_T(dtype, DISPATCH_IDX_T(idx_dtype, hipLaunchKernelGGL(
      (spgemm_compact_rows_kernel<val_t, idx_t>),
      dim3(grid_1d(n, LS_THREADS / 8, 8192)), dim3(LS_THREADS), 0, s,
      reinterpret_cast<const i64*>(rows_list), n,
      reinterpret_cast<const i64*>(src_off),
      reinterpret_cast<const i64*>(dst_indptr),
      reinterpret_cast<const idx_t*>(src_idx),
      reinterpret_cast<const val_t*>(src_val),
      reinterpret_cast<idx_t*>(dst_idx),
      reinterpret_cast<val_t*>(dst_val))));
  ls_check(hipGetLastError(), "spgemm_compact_rows");
}

// Output-centric variant: one lane per C ELEMENT.  Lane (row, ss)
// computes C[row, row+E[ss]] = sum over the (a,b) pairs whose offset
// sum lands on slot ss (host-precomputed CSR over slots).  No LDS
// accumulators (the lane's products sum in registers), naturally
// coalesced writes, 2-3 independent loads per lane — latency-bound
// where the LDS variant serialized on accumulator RMW chains.
template <typename T, typename I>
__global__ __launch_bounds__(LS_THREADS) void spgemm_affine_out_kernel(
    const i64* __restrict__ A_ip, const T* __restrict__ A_vals,
    const i64* __restrict__ B_ip, const T* __restrict__ B_vals,
    const int* __restrict__ DA,
    const int* __restrict__ slot_off, const short* __restrict__ slot_a,
    const short* __restrict__ slot_b, int nE, const int* __restrict__ E,
    const unsigned char* __restrict__ validC,
    const i64* __restrict__ C_ip, I* __restrict__ C_idx,
    T* __restrict__ C_vals, i64 n_rows) {
  __shared__ int E_s[64];  // nE <= 51, as in spgemm_affine_kernel
  __shared__ int soff_s[65];
  __shared__ short sa_s[16 * 16];
  __shared__ short sb_s[16 * 16];
  const int npairs = slot_off[nE];
  if (threadIdx.x < nE) E_s[threadIdx.x] = E[threadIdx.x];
  if (threadIdx.x <= nE) soff_s[threadIdx.x] = slot_off[threadIdx.x];
  if (threadIdx.x < npairs) {
    sa_s[threadIdx.x] = slot_a[threadIdx.x];
    sb_s[threadIdx.x] = slot_b[threadIdx.x];
  }
  __syncthreads();
  const i64 total = n_rows * (i64)nE;
  const i64 stride = (i64)gridDim.x * blockDim.x;
  for (i64 e = (i64)blockIdx.x * blockDim.x + threadIdx.x; e < total;
       e += stride) {
    const i64 row = e / nE;
    const int ss = (int)(e - row * nE);
    if (!validC[row]) continue;
    const i64 sA = A_ip[row];
    T acc = ls_zero<T>();
    const int p0 = soff_s[ss], p1 = soff_s[ss + 1];
    for (int p = p0; p < p1; ++p) {
      const int a = sa_s[p];
      const i64 k = row + DA[a];
      acc += A_vals[sA + a] * B_vals[B_ip[k] + sb_s[p]];
    }
    const i64 o = C_ip[row] + ss;
    C_idx[o] = (I)(row + E_s[ss]);
    C_vals[o] = acc;
  }
}

void ls_spgemm_affine(uintptr_t A_ip, uintptr_t A_vals, uintptr_t B_ip,
                      uintptr_t B_vals, uintptr_t DA, int ndA, int ndB,
                      uintptr_t pair_slot, int nE, uintptr_t E,
                      uintptr_t validC, uintptr_t C_ip, uintptr_t C_idx,
                      uintptr_t C_vals, i64 n_rows, int dtype,
                      int idx_dtype, uintptr_t stream) {
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const int grid = grid_1d(n_rows, LS_THREADS, 8192);
  DISPATCH_VAL_T(dtype, DISPATCH_IDX_T(idx_dtype, ({
    const size_t smem = (size_t)nE * LS_THREADS * sizeof(val_t);
    hipLaunchKernelGGL((spgemm_affine_kernel<val_t, idx_t>), dim3(grid),
                       dim3(LS_THREADS), smem, s,
                       reinterpret_cast<const i64*>(A_ip),
                       reinterpret_cast<const val_t*>(A_vals),
                       reinterpret_cast<const i64*>(B_ip),
                       reinterpret_cast<const val_t*>(B_vals),
                       reinterpret_cast<const int*>(DA), ndA, ndB,
                       reinterpret_cast<const short*>(pair_slot), nE,
                       reinterpret_cast<const int*>(E),
                       reinterpret_cast<const unsigned char*>(validC),
                       reinterpret_cast<const i64*>(C_ip),
                       reinterpret_cast<idx_t*>(C_idx),
                       reinterpret_cast<val_t*>(C_vals), n_rows);
  })));
  ls_check(hipGetLastError(), "spgemm_affine");
}

void ls_spgemm_affine_out(uintptr_t A_ip, uintptr_t A_vals, uintptr_t B_ip,
                          uintptr_t B_vals, uintptr_t DA,
                          uintptr_t slot_off, uintptr_t slot_a,
                          uintptr_t slot_b, int nE, uintptr_t E,
                          uintptr_t validC, uintptr_t C_ip,
                          uintptr_t C_idx, uintptr_t C_vals, i64 n_rows,
                          int dtype, int idx_dtype, uintptr_t stream) {
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const i64 total = n_rows * (i64)nE;
  const int grid = grid_1d(total, LS_THREADS, 16384);
  DISPATCH_VAL_T(dtype, DISPATCH_IDX_T(idx_dtype, hipLaunchKernelGGL(
      (spgemm_affine_out_kernel<val_t, idx_t>), dim3(grid),
      dim3(LS_THREADS), 0, s,
      reinterpret_cast<const i64*>(A_ip),
      reinterpret_cast<const val_t*>(A_vals),
      reinterpret_cast<const i64*>(B_ip),
      reinterpret_cast<const val_t*>(B_vals),
      reinterpret_cast<const int*>(DA),
      reinterpret_cast<const int*>(slot_off),
      reinterpret_cast<const short*>(slot_a),
      reinterpret_cast<const short*>(slot_b), nE,
      reinterpret_cast<const int*>(E),
      reinterpret_cast<const unsigned char*>(validC),
      reinterpret_cast<const i64*>(C_ip),
      reinterpret_cast<idx_t*>(C_idx),
      reinterpret_cast<val_t*>(C_vals), n_rows)));
  ls_check(hipGetLastError(), "spgemm_affine_out");
}

void ls_spgemm_row_ub_bins(uintptr_t A_indptr, uintptr_t A_indices,
                           uintptr_t B_indptr, uintptr_t ub, i64 n_rows,
                           uintptr_t counts, int idx_dtype,
                           uintptr_t stream) {
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  int grid = grid_1d(n_rows, LS_THREADS / 4, 8192);
  DISPATCH_IDX_T(idx_dtype, hipLaunchKernelGGL(
      (row_ub_bins_kernel<idx_t>), dim3(grid), dim3(LS_THREADS), 0, s,
      reinterpret_cast<const i64*>(A_indptr),
      reinterpret_cast<const idx_t*>(A_indices),
      reinterpret_cast<const i64*>(B_indptr),
      reinterpret_cast<i64*>(ub), n_rows,
      reinterpret_cast<i64*>(counts)));
  ls_check(hipGetLastError(), "spgemm_row_ub_bins");
}

void ls_spgemm_bin_count(uintptr_t A_indptr, uintptr_t ub, i64 n_rows,
                         uintptr_t counts, uintptr_t stream) {
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(spgemm_bin_count_kernel,
                     dim3(grid_1d(n_rows, LS_THREADS, 4096)),
                     dim3(LS_THREADS), 0, s,
                     reinterpret_cast<const i64*>(A_indptr),
                     reinterpret_cast<const i64*>(ub), n_rows,
                     reinterpret_cast<i64*>(counts));
  ls_check(hipGetLastError(), "spgemm_bin_count");
}

void ls_spgemm_bin_scatter(uintptr_t A_indptr, uintptr_t ub, i64 n_rows,
                           uintptr_t cursors, uintptr_t rows_out,
                           uintptr_t stream) {
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(spgemm_bin_scatter_kernel,
                     dim3(grid_1d(n_rows, LS_THREADS, 1024)),
                     dim3(LS_THREADS), 0, s,
                     reinterpret_cast<const i64*>(A_indptr),
                     reinterpret_cast<const i64*>(ub), n_rows,
                     reinterpret_cast<i64*>(cursors),
                     reinterpret_cast<i64*>(rows_out));
  ls_check(hipGetLastError(), "spgemm_bin_scatter");
}

void ls_spgemm_merge_symbolic(int wcfg, uintptr_t rows_list, i64 n,
                              uintptr_t A_indptr, uintptr_t A_indices,
                              uintptr_t B_indptr, uintptr_t B_indices,
                              uintptr_t row_nnz, int idx_dtype,
                              uintptr_t stream) {
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  DISPATCH_IDX_T(idx_dtype, (merge_symbolic_dispatch<idx_t>(
      wcfg, reinterpret_cast<const i64*>(rows_list), n,
      reinterpret_cast<const i64*>(A_indptr),
      reinterpret_cast<const idx_t*>(A_indices),
      reinterpret_cast<const i64*>(B_indptr),
      reinterpret_cast<const idx_t*>(B_indices),
      reinterpret_cast<i64*>(row_nnz), s)));
  ls_check(hipGetLastError(), "spgemm_merge_symbolic");
}

void ls_spgemm_merge_numeric(int wcfg, uintptr_t rows_list, i64 n,
                             uintptr_t A_indptr, uintptr_t A_indices,
                             uintptr_t A_vals, uintptr_t B_indptr,
                             uintptr_t B_indices, uintptr_t B_vals,
                             uintptr_t C_indptr, uintptr_t C_indices,
                             uintptr_t C_vals, int dtype, int idx_dtype,
                             uintptr_t row_nnz_out, uintptr_t stream) {
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  if (row_nnz_out) {
    DISPATCH_VAL_T(dtype, DISPATCH_IDX_T(idx_dtype, (
        merge_numeric_dispatch<val_t, idx_t, true>(
            wcfg, reinterpret_cast<const i64*>(rows_list), n,
            reinterpret_cast<const i64*>(A_indptr),
            reinterpret_cast<const idx_t*>(A_indices),
            reinterpret_cast<const val_t*>(A_vals),
            reinterpret_cast<const i64*>(B_indptr),
            reinterpret_cast<const idx_t*>(B_indices),
            reinterpret_cast<const val_t*>(B_vals),
            reinterpret_cast<const i64*>(C_indptr),
            reinterpret_cast<idx_t*>(C_indices),
            reinterpret_cast<val_t*>(C_vals),
            reinterpret_cast<i64*>(row_nnz_out), s))));
  } else {
    DISPATCH_VAL_T(dtype, DISPATCH_IDX_T(idx_dtype, (
        merge_numeric_dispatch<val_t, idx_t, false>(
            wcfg, reinterpret_cast<const i64*>(rows_list), n,
            reinterpret_cast<const i64*>(A_indptr),
            reinterpret_cast<const idx_t*>(A_indices),
            reinterpret_cast<const val_t*>(A_vals),
            reinterpret_cast<const i64*>(B_indptr),
            reinterpret_cast<const idx_t*>(B_indices),
            reinterpret_cast<const val_t*>(B_vals),
            reinterpret_cast<const i64*>(C_indptr),
            reinterpret_cast<idx_t*>(C_indices),
            reinterpret_cast<val_t*>(C_vals), nullptr, s))));
  }
  ls_check(hipGetLastError(), "spgemm_merge_numeric");
}

void ls_spgemm_row_ub(uintptr_t A_indptr, uintptr_t A_indices,
                      uintptr_t B_indptr, uintptr_t ub, i64 n_rows,
                      int idx_dtype, uintptr_t stream) {
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  int grid = grid_1d(n_rows, LS_THREADS / 4, 8192);
  DISPATCH_IDX_T(idx_dtype, hipLaunchKernelGGL(
      (row_ub_kernel<idx_t>), dim3(grid), dim3(LS_THREADS), 0, s,
      reinterpret_cast<const i64*>(A_indptr),
      reinterpret_cast<const idx_t*>(A_indices),
      reinterpret_cast<const i64*>(B_indptr),
      reinterpret_cast<i64*>(ub), n_rows));
  ls_check(hipGetLastError(), "spgemm_row_ub");
}

void ls_spgemm_symbolic_lds(int cfg, uintptr_t rows_list, i64 n_bin_rows,
                            uintptr_t A_indptr, uintptr_t A_indices,
                            uintptr_t B_indptr, uintptr_t B_indices,
                            uintptr_t row_nnz, int idx_dtype,
                            uintptr_t stream) {
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  DISPATCH_IDX_T(idx_dtype, symbolic_lds_dispatch<idx_t>(
      cfg, reinterpret_cast<const i64*>(rows_list), n_bin_rows,
      reinterpret_cast<const i64*>(A_indptr),
      reinterpret_cast<const idx_t*>(A_indices),
      reinterpret_cast<const i64*>(B_indptr),
      reinterpret_cast<const idx_t*>(B_indices),
      reinterpret_cast<i64*>(row_nnz), s));
  ls_check(hipGetLastError(), "spgemm_symbolic_lds");
}

#include <cstdlib>

void ls_spgemm_numeric_lds(int cfg, uintptr_t rows_list, i64 n_bin_rows,
                           uintptr_t A_indptr, uintptr_t A_indices,
                           uintptr_t A_vals, uintptr_t B_indptr,
                           uintptr_t B_indices, uintptr_t B_vals,
                           uintptr_t C_indptr, uintptr_t C_indices,
                           uintptr_t C_vals, int dtype, int idx_dtype,
                           uintptr_t row_nnz_out, int pack,
                           uintptr_t stream) {
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  static const char* abl_env = std::getenv("LS_SPGEMM_ABLATE");
  const int abl = abl_env ? atoi(abl_env) : 0;
  if (abl >= 3 && !row_nnz_out) {
    auto run = [&](auto tag) {
      constexpr int A = decltype(tag)::value;
      DISPATCH_VAL_T(dtype, DISPATCH_IDX_T(idx_dtype, (
          numeric_lds_dispatch_abl<val_t, idx_t, A>(
              cfg, reinterpret_cast<const i64*>(rows_list), n_bin_rows,
              reinterpret_cast<const i64*>(A_indptr),
              reinterpret_cast<const idx_t*>(A_indices),
              reinterpret_cast<const val_t*>(A_vals),
              reinterpret_cast<const i64*>(B_indptr),
              reinterpret_cast<const idx_t*>(B_indices),
              reinterpret_cast<const val_t*>(B_vals),
              reinterpret_cast<const i64*>(C_indptr),
              reinterpret_cast<idx_t*>(C_indices),
              reinterpret_cast<val_t*>(C_vals), nullptr, s))));
    };
    if (abl == 3) run(std::integral_constant<int, 3>{});
    else if (abl == 4) run(std::integral_constant<int, 4>{});
    else run(std::integral_constant<int, 5>{});
    ls_check(hipGetLastError(), "spgemm_numeric_lds");
    return;
  }
  if (abl == 1 && !row_nnz_out) {
    DISPATCH_VAL_T(dtype, DISPATCH_IDX_T(idx_dtype, (
        numeric_lds_dispatch_abl<val_t, idx_t, 1>(
            cfg, reinterpret_cast<const i64*>(rows_list), n_bin_rows,
            reinterpret_cast<const i64*>(A_indptr),
            reinterpret_cast<const idx_t*>(A_indices),
            reinterpret_cast<const val_t*>(A_vals),
            reinterpret_cast<const i64*>(B_indptr),
            reinterpret_cast<const idx_t*>(B_indices),
            reinterpret_cast<const val_t*>(B_vals),
            reinterpret_cast<const i64*>(C_indptr),
            reinterpret_cast<idx_t*>(C_indices),
            reinterpret_cast<val_t*>(C_vals), nullptr, s))));
    ls_check(hipGetLastError(), "spgemm_numeric_lds");
    return;
  }
  if (abl == 2 && !row_nnz_out) {
    DISPATCH_VAL_T(dtype, DISPATCH_IDX_T(idx_dtype, (
        numeric_lds_dispatch_abl<val_t, idx_t, 2>(
            cfg, reinterpret_cast<const i64*>(rows_list), n_bin_rows,
            reinterpret_cast<const i64*>(A_indptr),
            reinterpret_cast<const idx_t*>(A_indices),
            reinterpret_cast<const val_t*>(A_vals),
            reinterpret_cast<const i64*>(B_indptr),
            reinterpret_cast<const idx_t*>(B_indices),
            reinterpret_cast<const val_t*>(B_vals),
            reinterpret_cast<const i64*>(C_indptr),
            reinterpret_cast<idx_t*>(C_indices),
            reinterpret_cast<val_t*>(C_vals), nullptr, s))));
    ls_check(hipGetLastError(), "spgemm_numeric_lds");
    return;
  }
  if (row_nnz_out) {
    DISPATCH_VAL_T(dtype, DISPATCH_IDX_T(idx_dtype, (
        numeric_lds_dispatch<val_t, idx_t, true>(
            cfg, reinterpret_cast<const i64*>(rows_list), n_bin_rows,
            reinterpret_cast<const i64*>(A_indptr),
            reinterpret_cast<const idx_t*>(A_indices),
            reinterpret_cast<const val_t*>(A_vals),
            reinterpret_cast<const i64*>(B_indptr),
            reinterpret_cast<const idx_t*>(B_indices),
            reinterpret_cast<const val_t*>(B_vals),
            reinterpret_cast<const i64*>(C_indptr),
            reinterpret_cast<idx_t*>(C_indices),
            reinterpret_cast<val_t*>(C_vals),
            reinterpret_cast<i64*>(row_nnz_out), pack != 0, s))));
  } else {
    DISPATCH_VAL_T(dtype, DISPATCH_IDX_T(idx_dtype, (
        numeric_lds_dispatch<val_t, idx_t, false>(
            cfg, reinterpret_cast<const i64*>(rows_list), n_bin_rows,
            reinterpret_cast<const i64*>(A_indptr),
            reinterpret_cast<const idx_t*>(A_indices),
            reinterpret_cast<const val_t*>(A_vals),
            reinterpret_cast<const i64*>(B_indptr),
            reinterpret_cast<const idx_t*>(B_indices),
            reinterpret_cast<const val_t*>(B_vals),
            reinterpret_cast<const i64*>(C_indptr),
            reinterpret_cast<idx_t*>(C_indices),
            reinterpret_cast<val_t*>(C_vals), nullptr, pack != 0, s))));
  }
  ls_check(hipGetLastError(), "spgemm_numeric_lds");
}

void ls_spgemm_symbolic_global(uintptr_t rows_list, uintptr_t chunk_rowidx,
                               uintptr_t chunk_ord, i64 n_chunks,
                               uintptr_t A_indptr, uintptr_t A_indices,
                               uintptr_t B_indptr, uintptr_t B_indices,
                               uintptr_t tbl_ws, uintptr_t tbl_off,
                               uintptr_t tbl_size, uintptr_t row_nnz,
                               int idx_dtype, int identity,
                               uintptr_t blen_prefix, uintptr_t pref_base,
                               uintptr_t a_len_g, uintptr_t stream) {
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  DISPATCH_IDX_T(idx_dtype, hipLaunchKernelGGL(
      (spgemm_symbolic_global_kernel<idx_t>), dim3(n_chunks),
      dim3(LS_THREADS), 0, s, reinterpret_cast<const i64*>(rows_list),
      reinterpret_cast<const i64*>(chunk_rowidx),
      reinterpret_cast<const i64*>(chunk_ord), n_chunks,
      reinterpret_cast<const i64*>(A_indptr),
      reinterpret_cast<const idx_t*>(A_indices),
      reinterpret_cast<const i64*>(B_indptr),
      reinterpret_cast<const idx_t*>(B_indices),
      reinterpret_cast<uint32_t*>(tbl_ws),
      reinterpret_cast<const i64*>(tbl_off),
      reinterpret_cast<const i64*>(tbl_size),
      reinterpret_cast<i64*>(row_nnz), identity,
      reinterpret_cast<const i64*>(blen_prefix),
      reinterpret_cast<const i64*>(pref_base),
      reinterpret_cast<const i64*>(a_len_g)));
  ls_check(hipGetLastError(), "spgemm_symbolic_global");
}

void ls_spgemm_numeric_global_fill(uintptr_t rows_list,
                                   uintptr_t chunk_rowidx,
                                   uintptr_t chunk_ord, i64 n_chunks,
                                   uintptr_t A_indptr, uintptr_t A_indices,
                                   uintptr_t A_vals, uintptr_t B_indptr,
                                   uintptr_t B_indices, uintptr_t B_vals,
                                   uintptr_t key_ws, uintptr_t val_ws,
                                   uintptr_t tbl_off, uintptr_t tbl_size,
                                   int dtype, int idx_dtype, int identity,
                                   uintptr_t blen_prefix,
                                   uintptr_t pref_base, uintptr_t a_len_g,
                                   uintptr_t stream) {
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  DISPATCH_VAL_T(dtype, DISPATCH_IDX_T(idx_dtype, hipLaunchKernelGGL(
      (spgemm_numeric_global_fill<val_t, idx_t>), dim3(n_chunks),
      dim3(LS_THREADS), 0, s, reinterpret_cast<const i64*>(rows_list),
      reinterpret_cast<const i64*>(chunk_rowidx),
      reinterpret_cast<const i64*>(chunk_ord), n_chunks,
      reinterpret_cast<const i64*>(A_indptr),
      reinterpret_cast<const idx_t*>(A_indices),
      reinterpret_cast<const val_t*>(A_vals),
      reinterpret_cast<const i64*>(B_indptr),
      reinterpret_cast<const idx_t*>(B_indices),
      reinterpret_cast<const val_t*>(B_vals),
      reinterpret_cast<uint32_t*>(key_ws),
      reinterpret_cast<val_t*>(val_ws),
      reinterpret_cast<const i64*>(tbl_off),
      reinterpret_cast<const i64*>(tbl_size), identity,
      reinterpret_cast<const i64*>(blen_prefix),
      reinterpret_cast<const i64*>(pref_base),
      reinterpret_cast<const i64*>(a_len_g))));
  ls_check(hipGetLastError(), "spgemm_numeric_global_fill");
}

void ls_spgemm_global_compact_sorted(
    uintptr_t rows_list, i64 n_bin_rows, uintptr_t key_ws,
    uintptr_t val_ws, uintptr_t tbl_off, uintptr_t tbl_size,
    uintptr_t C_indptr, uintptr_t C_indices, uintptr_t C_vals,
    uintptr_t row_nnz_out, int dtype, int idx_dtype, uintptr_t stream) {
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  DISPATCH_VAL_T(dtype, DISPATCH_IDX_T(idx_dtype, hipLaunchKernelGGL(
      (spgemm_global_compact_sorted<val_t, idx_t>), dim3(n_bin_rows),
      dim3(LS_THREADS), 0, s, reinterpret_cast<const i64*>(rows_list),
      n_bin_rows, reinterpret_cast<const uint32_t*>(key_ws),
      reinterpret_cast<const val_t*>(val_ws),
      reinterpret_cast<const i64*>(tbl_off),
      reinterpret_cast<const i64*>(tbl_size),
      reinterpret_cast<const i64*>(C_indptr),
      reinterpret_cast<idx_t*>(C_indices),
      reinterpret_cast<val_t*>(C_vals),
      reinterpret_cast<i64*>(row_nnz_out))));
  ls_check(hipGetLastError(), "spgemm_global_compact_sorted");
}

void ls_spgemm_global_compact(uintptr_t rows_list, i64 n_bin_rows,
                              uintptr_t key_ws, uintptr_t val_ws,
                              uintptr_t tbl_off, uintptr_t tbl_size,
                              uintptr_t C_indptr, uintptr_t C_indices,
                              uintptr_t C_vals, uintptr_t row_nnz_out,
                              int dtype, int idx_dtype, uintptr_t stream) {
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  DISPATCH_VAL_T(dtype, DISPATCH_IDX_T(idx_dtype, hipLaunchKernelGGL(
      (spgemm_global_compact<val_t, idx_t>), dim3(n_bin_rows),
      dim3(LS_THREADS), 0, s, reinterpret_cast<const i64*>(rows_list),
      n_bin_rows, reinterpret_cast<const uint32_t*>(key_ws),
      reinterpret_cast<const val_t*>(val_ws),
      reinterpret_cast<const i64*>(tbl_off),
      reinterpret_cast<const i64*>(tbl_size),
      reinterpret_cast<const i64*>(C_indptr),
      reinterpret_cast<idx_t*>(C_indices),
      reinterpret_cast<val_t*>(C_vals),
      reinterpret_cast<i64*>(row_nnz_out))));
  ls_check(hipGetLastError(), "spgemm_global_compact");
}

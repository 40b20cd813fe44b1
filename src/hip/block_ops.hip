// SPDX-License-Identifier: Apache-2.0
// Tall-skinny dense block algebra for gfx950 (docs/DESIGN.md §16): the
// streaming passes LOBPCG makes over its (n, k) blocks around the SpMM.
//
//   block_gram      G = X^H Y            X (n, p), Y (n, q)  ->  (p, q)
//   block_update    Z = sum_i X_i C_i (+ Z)   up to three terms, one pass
//   block_residual  R = AX - X diag(theta), and the k column sums |R|^2
//
// Every operand is a row-major block with unit column stride and an
// explicit row stride ld >= cols, so a column panel of a wider buffer is
// passed without a copy.  Column counts are runtime values in
// [1, LS_BLOCK_KMAX]; every offset is formed in 64 bits; n = 0 is legal.
//
// All three follow the §15 streaming conventions: a capped grid-stride loop
// over row chunks, a 16-byte pack instantiation chosen once on the host (base
// pointers, row strides and row lengths all 16-byte multiples) and an
// element-wise one otherwise, guarded tails, no padding.
//
// Reductions are REPRODUCIBLE: no float atomics.  Each workgroup sums its
// rows in a fixed order and writes one slab row; slab_reduce_kernel then sums
// the slab rows in a fixed order (Guideline 12, partial slab + reduce pass).
// The grid depends on n alone, so the same input gives the same bits.

#include "common.h"
#include <stdexcept>
#include <string>

#define LS_BLOCK_KMAX 32

namespace {

constexpr int GRAM_PER_BLOCK = 256;    // rows per workgroup chunk
constexpr int GRAM_GRID_CAP = 1024;
constexpr int UPDATE_PER_BLOCK = 128;
constexpr int UPDATE_GRID_CAP = 2048;
constexpr int RESID_PER_BLOCK = 256;
constexpr int RESID_GRID_CAP = 1024;
// dynamic LDS budgets (bytes); <= 64 KiB needs no opt-in
constexpr int GRAM_LDS_BYTES = 32 * 1024;
constexpr int UPDATE_LDS_BYTES = 64 * 1024;
// the gram kernel's cross-slice reduction reuses the staging area
constexpr int GRAM_RED_ELEMS = LS_THREADS * 4;

template <typename T> struct real_of { using type = T; };
template <typename T> struct real_of<Cplx<T>> { using type = T; };

template <typename T>
__device__ inline T abs2(T v) { return v * v; }
template <typename T>
__device__ inline T abs2(Cplx<T> v) { return v.re * v.re + v.im * v.im; }

template <typename T>
__device__ inline T scale_real(T v, T s) { return v * s; }
template <typename T>
__device__ inline Cplx<T> scale_real(Cplx<T> v, T s) {
  return {v.re * s, v.im * s};
}

template <typename T, int V>
struct alignas(V == 1 ? alignof(T) : sizeof(T) * V) Pack {
  T e[V];
};

// Stage `rows` rows of a (., cols) block, starting at row r0, into LDS with
// row stride cols.  A row takes 1 << shift lanes of V elements each (lanes
// past the row's end idle); V > 1 requires cols % V == 0 and 16-byte
// aligned rows, which the host has checked.
template <typename T, int V>
__device__ inline void stage_rows(T* __restrict__ dst, const T* src, i64 ld,
                                  int cols, int shift, i64 r0, int rows) {
  const int items = rows << shift;
  const int mask = (1 << shift) - 1;
  for (int it = threadIdx.x; it < items; it += LS_THREADS) {
    const int r = it >> shift;
    const int c = (it & mask) * V;
    if (c < cols) {
      const Pack<T, V> k =
          *reinterpret_cast<const Pack<T, V>*>(src + (r0 + r) * ld + c);
#pragma unroll
      for (int j = 0; j < V; ++j) dst[r * cols + c + j] = k.e[j];
    }
  }
}

// ---------------------------------------------------------------------------
// block_gram.  A workgroup stages R rows of X and Y in LDS; thread
// (tile, slice) keeps a 2 x 2 tile of G in registers and walks the rows
// slice, slice + S, ... of the staged rows, S = 256 / tiles.  After the last
// chunk the S slices are summed through LDS in slice order and the
// workgroup's (p, q) partial goes to its slab row.
// ---------------------------------------------------------------------------
template <typename T, int V, bool CONJ>
__global__ __launch_bounds__(LS_THREADS) void block_gram_kernel(
    const T* X, i64 ldx, int p, int xshift, const T* Y, i64 ldy, int q,
    int yshift, T* __restrict__ slab, i64 n, int R) {
  extern __shared__ __align__(16) unsigned char ls_block_smem[];
  T* xs = reinterpret_cast<T*>(ls_block_smem);
  T* ys = xs + R * p;
  const int tq = (q + 1) / 2;
  const int ntile = ((p + 1) / 2) * tq;   // <= 256
  const int nslice = LS_THREADS / ntile;  // >= 1
  const int tile = threadIdx.x % ntile;
  const int slice = threadIdx.x / ntile;
  const bool active = slice < nslice;
  // an odd p or q leaves a half-empty tile: its second index is clamped
  // (reads stay in range) and that part of the tile is never written out
  const int i0 = 2 * (tile / tq), j0 = 2 * (tile % tq);
  const int i1 = i0 + 1 < p ? i0 + 1 : i0;
  const int j1 = j0 + 1 < q ? j0 + 1 : j0;
  T a00 = ls_zero<T>(), a01 = ls_zero<T>(), a10 = ls_zero<T>(),
    a11 = ls_zero<T>();
  for (i64 base = (i64)blockIdx.x * GRAM_PER_BLOCK; base < n;
       base += (i64)gridDim.x * GRAM_PER_BLOCK) {
    const i64 cend = base + GRAM_PER_BLOCK < n ? base + GRAM_PER_BLOCK : n;
    for (i64 r0 = base; r0 < cend; r0 += R) {
      const int rows = r0 + R < cend ? R : (int)(cend - r0);
      stage_rows<T, V>(xs, X, ldx, p, xshift, r0, rows);
      stage_rows<T, V>(ys, Y, ldy, q, yshift, r0, rows);
      __syncthreads();
      if (active) {
        for (int r = slice; r < rows; r += nslice) {
          T x0 = xs[r * p + i0], x1 = xs[r * p + i1];
          const T y0 = ys[r * q + j0], y1 = ys[r * q + j1];
          if constexpr (CONJ) {
            x0 = ls_conj(x0);
            x1 = ls_conj(x1);
          }
          a00 += x0 * y0;
          a01 += x0 * y1;
          a10 += x1 * y0;
          a11 += x1 * y1;
        }
      }
      __syncthreads();
    }
  }
  T* red = xs;  // >= GRAM_RED_ELEMS elements, free after the last barrier
  if (active) {
    T* dst = red + (slice * ntile + tile) * 4;
    dst[0] = a00;
    dst[1] = a01;
    dst[2] = a10;
    dst[3] = a11;
  }
  __syncthreads();
  const int E = p * q;
  for (int e = threadIdx.x; e < E; e += LS_THREADS) {
    const int i = e / q, j = e % q;
    const int src = ((i / 2) * tq + j / 2) * 4 + (i & 1) * 2 + (j & 1);
    T s = red[src];
    for (int sl = 1; sl < nslice; ++sl) s += red[sl * ntile * 4 + src];
    slab[(i64)blockIdx.x * E + e] = s;
  }
}

// out[e] = sum_b slab[b, e], one wave per entry: lane l sums rows l, l + 64,
// ... in order, then a fixed shuffle tree.
template <typename T>
__global__ __launch_bounds__(LS_THREADS) void slab_reduce_kernel(
    const T* __restrict__ slab, int nb, int E, T* __restrict__ out) {
  const int e = blockIdx.x * (LS_THREADS / WAVE_SIZE) +
                threadIdx.x / WAVE_SIZE;
  if (e >= E) return;
  const int lane = threadIdx.x % WAVE_SIZE;
  T acc = ls_zero<T>();
  for (int b = lane; b < nb; b += WAVE_SIZE) acc += slab[(i64)b * E + e];
  acc = group_reduce_sum<T, WAVE_SIZE>(acc);
  if (lane == 0) out[e] = acc;
}

// ---------------------------------------------------------------------------
// block_update.  A workgroup keeps every C_i in LDS (rows padded with zeros
// to a multiple of 4 columns), stages R rows of every X_i, and each thread
// produces 4 adjacent columns of one row of Z.  Rows are private to one
// workgroup and Z is written only after the barrier that follows staging,
// so Z may be one of the X_i.
// ---------------------------------------------------------------------------
template <typename T>
struct UpdateArgs {
  const T* X[3];
  const T* C[3];
  i64 ld[3];
  int p[3];
  int shift[3];
};

template <typename T, int V>
__global__ __launch_bounds__(LS_THREADS) void block_update_kernel(
    T* Z, i64 ldz, int q, int zshift, UpdateArgs<T> a, int nterms,
    int accumulate, i64 n, int R) {
  extern __shared__ __align__(16) unsigned char ls_block_smem[];
  const int qs = (q + 3) & ~3;
  const int qg = qs / 4;
  T* cs[3];
  T* xs[3];
  {
    // constant trip counts, fully unrolled: cs/xs stay in registers
    T* cur = reinterpret_cast<T*>(ls_block_smem);
#pragma unroll
    for (int t = 0; t < 3; ++t) {
      cs[t] = cur;
      if (t < nterms) cur += a.p[t] * qs;
    }
#pragma unroll
    for (int t = 0; t < 3; ++t) {
      xs[t] = cur;
      if (t < nterms) cur += R * a.p[t];
    }
  }
#pragma unroll
  for (int t = 0; t < 3; ++t) {
    if (t >= nterms) continue;
    const int cnt = a.p[t] * qs;
    for (int e = threadIdx.x; e < cnt; e += LS_THREADS) {
      const int l = e / qs, j = e % qs;
      cs[t][e] = j < q ? a.C[t][l * q + j] : ls_zero<T>();
    }
  }
  const int zmask = (1 << zshift) - 1;
  for (i64 base = (i64)blockIdx.x * UPDATE_PER_BLOCK; base < n;
       base += (i64)gridDim.x * UPDATE_PER_BLOCK) {
    const i64 cend =
        base + UPDATE_PER_BLOCK < n ? base + UPDATE_PER_BLOCK : n;
    for (i64 r0 = base; r0 < cend; r0 += R) {
      const int rows = r0 + R < cend ? R : (int)(cend - r0);
      __syncthreads();  // previous tile's reads (and the C fill) are done
#pragma unroll
      for (int t = 0; t < 3; ++t)
        if (t < nterms)
          stage_rows<T, V>(xs[t], a.X[t], a.ld[t], a.p[t], a.shift[t], r0,
                           rows);
      __syncthreads();
      const int items = rows << zshift;
      for (int it = threadIdx.x; it < items; it += LS_THREADS) {
        const int r = it >> zshift;
        const int g = it & zmask;
        if (g >= qg) continue;
        T acc[4];
#pragma unroll
        for (int m = 0; m < 4; ++m) acc[m] = ls_zero<T>();
#pragma unroll
        for (int t = 0; t < 3; ++t) {
          if (t >= nterms) continue;
          const int pt = a.p[t];
          const T* xr = xs[t] + r * pt;
          const T* c = cs[t] + 4 * g;
          for (int l = 0; l < pt; ++l) {
            const T xv = xr[l];
#pragma unroll
            for (int m = 0; m < 4; ++m) acc[m] += xv * c[l * qs + m];
          }
        }
        T* zr = Z + (r0 + r) * ldz + 4 * g;
        if constexpr (V > 1) {
          // q % V == 0 and V divides 4: whole packs, all inside the row
#pragma unroll
          for (int m = 0; m < 4; m += V) {
            if (4 * g + m < q) {
              Pack<T, V> k;
              if (accumulate) {
                k = *reinterpret_cast<const Pack<T, V>*>(zr + m);
#pragma unroll
                for (int j = 0; j < V; ++j) k.e[j] = acc[m + j] + k.e[j];
              } else {
#pragma unroll
                for (int j = 0; j < V; ++j) k.e[j] = acc[m + j];
              }
              *reinterpret_cast<Pack<T, V>*>(zr + m) = k;
            }
          }
        } else {
#pragma unroll
          for (int m = 0; m < 4; ++m) {
            if (4 * g + m < q) zr[m] = accumulate ? acc[m] + zr[m] : acc[m];
          }
        }
      }
    }
  }
}

// ---------------------------------------------------------------------------
// block_residual.  Element-wise; a row takes 1 << shift lanes of V columns,
// so a thread keeps the same columns for the whole grid-stride loop and
// carries their V partial sums of |R|^2.  The workgroup sums them per
// column in thread order into its slab row.
// ---------------------------------------------------------------------------
template <typename T, int V>
__global__ __launch_bounds__(LS_THREADS) void block_residual_kernel(
    T* Rb, i64 ldr, const T* AX, i64 lda, const T* X, i64 ldx,
    const typename real_of<T>::type* __restrict__ theta,
    typename real_of<T>::type* __restrict__ slab, int k, int shift, i64 n) {
  using Rt = typename real_of<T>::type;
  __shared__ Rt red[LS_THREADS][V];
  const int lanes = 1 << shift;
  const int c = (threadIdx.x & (lanes - 1)) * V;
  const int rows_per_pass = LS_THREADS >> shift;
  Rt acc[V], th[V];
#pragma unroll
  for (int j = 0; j < V; ++j) {
    acc[j] = Rt(0);
    th[j] = c + j < k ? theta[c + j] : Rt(0);
  }
  if (c < k) {
    for (i64 row = (i64)blockIdx.x * rows_per_pass + (threadIdx.x >> shift);
         row < n; row += (i64)gridDim.x * rows_per_pass) {
      const Pack<T, V> ak =
          *reinterpret_cast<const Pack<T, V>*>(AX + row * lda + c);
      const Pack<T, V> xk =
          *reinterpret_cast<const Pack<T, V>*>(X + row * ldx + c);
      Pack<T, V> rk;
#pragma unroll
      for (int j = 0; j < V; ++j) {
        rk.e[j] = ak.e[j] - scale_real(xk.e[j], th[j]);
        acc[j] += abs2(rk.e[j]);
      }
      *reinterpret_cast<Pack<T, V>*>(Rb + row * ldr + c) = rk;
    }
  }
#pragma unroll
  for (int j = 0; j < V; ++j) red[threadIdx.x][j] = acc[j];
  __syncthreads();
  if ((int)threadIdx.x < k) {
    const int j = threadIdx.x;
    Rt s = Rt(0);
    for (int t = j / V; t < LS_THREADS; t += lanes) s += red[t][j % V];
    slab[(i64)blockIdx.x * k + j] = s;
  }
}

inline int pow2_shift(int lanes) {
  int s = 0;
  while ((1 << s) < lanes) ++s;
  return s;
}

inline void check_cols(int c, const char* what) {
  if (c < 1 || c > LS_BLOCK_KMAX)
    throw std::runtime_error(std::string(what) + ": column count " +
                             std::to_string(c) + " outside [1, " +
                             std::to_string(LS_BLOCK_KMAX) + "]");
}

// 16-byte packs are legal for a block when its base and its row stride in
// bytes are 16-byte multiples and its rows hold whole packs
inline bool pack_ok(uintptr_t base, i64 ld, int cols, int esize) {
  const int v = 16 / esize;
  return base % 16 == 0 && (ld * esize) % 16 == 0 && cols % v == 0;
}

template <typename T>
void launch_gram(bool vec, bool conj, int grid, size_t lds, hipStream_t s,
                 const T* xp, i64 ldx, int p, int xs, const T* yp, i64 ldy,
                 int q, int ys, T* sp, i64 n, int R) {
  constexpr int VW = 16 / (int)sizeof(T);
  const dim3 g(grid), b(LS_THREADS);
  if (vec && conj)
    hipLaunchKernelGGL((block_gram_kernel<T, VW, true>), g, b, lds, s, xp,
                       ldx, p, xs, yp, ldy, q, ys, sp, n, R);
  else if (vec)
    hipLaunchKernelGGL((block_gram_kernel<T, VW, false>), g, b, lds, s, xp,
                       ldx, p, xs, yp, ldy, q, ys, sp, n, R);
  else if (conj)
    hipLaunchKernelGGL((block_gram_kernel<T, 1, true>), g, b, lds, s, xp,
                       ldx, p, xs, yp, ldy, q, ys, sp, n, R);
  else
    hipLaunchKernelGGL((block_gram_kernel<T, 1, false>), g, b, lds, s, xp,
                       ldx, p, xs, yp, ldy, q, ys, sp, n, R);
}

template <typename T>
void launch_slab_reduce(const T* slab, int nb, int E, T* out,
                        hipStream_t s) {
  const int per = LS_THREADS / WAVE_SIZE;
  hipLaunchKernelGGL((slab_reduce_kernel<T>), dim3((E + per - 1) / per),
                     dim3(LS_THREADS), 0, s, slab, nb, E, out);
}

}  // namespace

int ls_block_kmax() { return LS_BLOCK_KMAX; }
int ls_block_gram_grid_cap() { return GRAM_GRID_CAP; }
int ls_block_gram_per_block() { return GRAM_PER_BLOCK; }
int ls_block_update_grid_cap() { return UPDATE_GRID_CAP; }
int ls_block_update_per_block() { return UPDATE_PER_BLOCK; }
int ls_block_residual_grid_cap() { return RESID_GRID_CAP; }
int ls_block_residual_per_block() { return RESID_PER_BLOCK; }

// slab: workspace of >= grid * p * q elements, grid = grid_1d(n, PER_BLOCK,
// GRID_CAP); slab_elems is its size, checked here
void ls_block_gram(uintptr_t X, i64 ldx, int p, uintptr_t Y, i64 ldy, int q,
                   uintptr_t out, uintptr_t slab, i64 slab_elems, i64 n,
                   bool conj, int dtype, uintptr_t stream) {
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  check_cols(p, "block_gram");
  check_cols(q, "block_gram");
  if (ldx < p || ldy < q || n < 0)
    throw std::runtime_error("block_gram: bad row stride or row count");
  const int grid = grid_1d(n, GRAM_PER_BLOCK, GRAM_GRID_CAP);
  if (slab_elems < (i64)grid * p * q)
    throw std::runtime_error("block_gram: workspace too small");
  DISPATCH_VAL_T(dtype, ({
    constexpr int ES = (int)sizeof(val_t);
    constexpr int VW = 16 / ES;
    int R = GRAM_LDS_BYTES / ES / (p + q);
    if (R > GRAM_PER_BLOCK) R = GRAM_PER_BLOCK;
    i64 elems = (i64)R * (p + q);
    if (elems < GRAM_RED_ELEMS) elems = GRAM_RED_ELEMS;
    const size_t lds = (size_t)elems * ES;
    const bool vec = VW > 1 && pack_ok(X, ldx, p, ES) &&
                     pack_ok(Y, ldy, q, ES);
    const int v = vec ? VW : 1;
    const int xs = pow2_shift(p / v), ys = pow2_shift(q / v);
    auto xp = reinterpret_cast<const val_t*>(X);
    auto yp = reinterpret_cast<const val_t*>(Y);
    auto sp = reinterpret_cast<val_t*>(slab);
    launch_gram<val_t>(vec, conj, grid, lds, s, xp, ldx, p, xs, yp, ldy, q,
                       ys, sp, n, R);
    launch_slab_reduce<val_t>(sp, grid, p * q,
                              reinterpret_cast<val_t*>(out), s);
  }));
  ls_check(hipGetLastError(), "block_gram");
}

void ls_block_update(uintptr_t Z, i64 ldz, int q, int nterms, uintptr_t X0,
                     i64 ld0, int p0, uintptr_t C0, uintptr_t X1, i64 ld1,
                     int p1, uintptr_t C1, uintptr_t X2, i64 ld2, int p2,
                     uintptr_t C2, bool accumulate, i64 n, int dtype,
                     uintptr_t stream) {
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  if (nterms < 1 || nterms > 3)
    throw std::runtime_error("block_update: 1 to 3 terms");
  check_cols(q, "block_update");
  const uintptr_t Xs[3] = {X0, X1, X2}, Cs[3] = {C0, C1, C2};
  const i64 lds_[3] = {ld0, ld1, ld2};
  const int ps[3] = {p0, p1, p2};
  int psum = 0;
  for (int t = 0; t < nterms; ++t) {
    check_cols(ps[t], "block_update");
    if (lds_[t] < ps[t])
      throw std::runtime_error("block_update: row stride below columns");
    psum += ps[t];
  }
  if (ldz < q || n < 0)
    throw std::runtime_error("block_update: bad row stride or row count");
  const int grid = grid_1d(n, UPDATE_PER_BLOCK, UPDATE_GRID_CAP);
  const int qs = (q + 3) & ~3;
  DISPATCH_VAL_T(dtype, ({
    constexpr int ES = (int)sizeof(val_t);
    constexpr int VW = 16 / ES;
    // aim for four workgroups per CU; the C matrices come first
    int budget = 32 * 1024 / ES;
    if (budget < psum * qs + 8 * psum) budget = UPDATE_LDS_BYTES / ES;
    int R = (budget - psum * qs) / psum;
    if (R > UPDATE_PER_BLOCK) R = UPDATE_PER_BLOCK;
    if (R < 1) throw std::runtime_error("block_update: LDS budget");
    const size_t lds = (size_t)(psum * qs + R * psum) * ES;
    bool vec = VW > 1 && pack_ok(Z, ldz, q, ES);
    for (int t = 0; t < nterms; ++t)
      vec = vec && pack_ok(Xs[t], lds_[t], ps[t], ES);
    const int v = vec ? VW : 1;
    UpdateArgs<val_t> a;
    for (int t = 0; t < 3; ++t) {
      const int u = t < nterms ? t : 0;
      a.X[t] = reinterpret_cast<const val_t*>(Xs[u]);
      a.C[t] = reinterpret_cast<const val_t*>(Cs[u]);
      a.ld[t] = lds_[u];
      a.p[t] = ps[u];
      a.shift[t] = pow2_shift(ps[u] / v);
    }
    const int zshift = pow2_shift(qs / 4);
    auto zp = reinterpret_cast<val_t*>(Z);
    if (vec)
      hipLaunchKernelGGL((block_update_kernel<val_t, VW>), dim3(grid),
                         dim3(LS_THREADS), lds, s, zp, ldz, q, zshift, a,
                         nterms, (int)accumulate, n, R);
    else
      hipLaunchKernelGGL((block_update_kernel<val_t, 1>), dim3(grid),
                         dim3(LS_THREADS), lds, s, zp, ldz, q, zshift, a,
                         nterms, (int)accumulate, n, R);
  }));
  ls_check(hipGetLastError(), "block_update");
}

// theta, norms and slab hold the REAL type of dtype; slab has
// >= grid * k elements, grid = grid_1d(n, PER_BLOCK, GRID_CAP)
void ls_block_residual(uintptr_t R, i64 ldr, uintptr_t AX, i64 lda,
                       uintptr_t X, i64 ldx, uintptr_t theta, uintptr_t norms,
                       uintptr_t slab, i64 slab_elems, int k, i64 n,
                       int dtype, uintptr_t stream) {
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  check_cols(k, "block_residual");
  if (ldr < k || lda < k || ldx < k || n < 0)
    throw std::runtime_error("block_residual: bad row stride or row count");
  const int grid = grid_1d(n, RESID_PER_BLOCK, RESID_GRID_CAP);
  if (slab_elems < (i64)grid * k)
    throw std::runtime_error("block_residual: workspace too small");
  DISPATCH_VAL_T(dtype, ({
    using real_t = typename real_of<val_t>::type;
    constexpr int ES = (int)sizeof(val_t);
    constexpr int VW = 16 / ES;
    const bool vec = VW > 1 && pack_ok(R, ldr, k, ES) &&
                     pack_ok(AX, lda, k, ES) && pack_ok(X, ldx, k, ES);
    const int shift = pow2_shift(k / (vec ? VW : 1));
    auto rp = reinterpret_cast<val_t*>(R);
    auto ap = reinterpret_cast<const val_t*>(AX);
    auto xp = reinterpret_cast<const val_t*>(X);
    auto tp = reinterpret_cast<const real_t*>(theta);
    auto sp = reinterpret_cast<real_t*>(slab);
    if (vec)
      hipLaunchKernelGGL((block_residual_kernel<val_t, VW>), dim3(grid),
                         dim3(LS_THREADS), 0, s, rp, ldr, ap, lda, xp, ldx,
                         tp, sp, k, shift, n);
    else
      hipLaunchKernelGGL((block_residual_kernel<val_t, 1>), dim3(grid),
                         dim3(LS_THREADS), 0, s, rp, ldr, ap, lda, xp, ldx,
                         tp, sp, k, shift, n);
    launch_slab_reduce<real_t>(sp, grid, k,
                               reinterpret_cast<real_t*>(norms), s);
  }));
  ls_check(hipGetLastError(), "block_residual");
}

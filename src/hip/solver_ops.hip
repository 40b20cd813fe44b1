// SPDX-License-Identifier: Apache-2.0
// Solver primitives for gfx950: fused AXPBY with device scalars, and
// block-reduced dot products.
//
// AXPBY (reference axpby.cu:25-47): the scalar quotient a/b is computed
// INSIDE the kernel from 1-element device tensors, so the CG loop never
// synchronizes with the host.  Memory-bound: vectorized grid-stride.
//
// VDOT: grid-stride partial sums -> wave shuffle reduce -> LDS across
// waves -> one device-scope atomicAdd per block into the 1-element output
// (Guideline 12).  The output feeds a 1-element RCCL all-reduce.
//
// BiCGSTAB: four streaming kernels with in-kernel guarded quotients of
// device scalars (see the section further down).

#include "common.h"
#include <cstdlib>
#include <stdexcept>

namespace {

template <typename T, bool IS_ALPHA, bool NEGATE>
__global__ __launch_bounds__(LS_THREADS) void axpby_kernel(
    T* __restrict__ y, const T* __restrict__ x, const T* __restrict__ a,
    const T* __restrict__ b, i64 n) {
  T val = (*a) / (*b);
  if constexpr (NEGATE) {
    if constexpr (is_cplx<T>::value)
      val = ls_zero<T>() - val;
    else
      val = -val;
  }
  const i64 stride = (i64)gridDim.x * blockDim.x;
  for (i64 i = (i64)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += stride) {
    if constexpr (IS_ALPHA)
      y[i] = val * x[i] + y[i];
    else
      y[i] = x[i] + val * y[i];
  }
}

template <typename T>
__global__ __launch_bounds__(LS_THREADS) void jacobi_kernel(
    T* __restrict__ x, const T* __restrict__ b, const T* __restrict__ y,
    const T* __restrict__ dinv, double omega, i64 n) {
  const i64 stride = (i64)gridDim.x * blockDim.x;
  for (i64 i = (i64)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += stride) {
    if constexpr (is_cplx<T>::value) {
      T r = b[i] - y[i];
      T upd = dinv[i] * r;
      x[i] += T{(decltype(upd.re))(omega) * upd.re,
                (decltype(upd.re))(omega) * upd.im};
    } else {
      x[i] += (T)omega * dinv[i] * (b[i] - y[i]);
    }
  }
}

__device__ inline void atomic_add_out(float* p, float v) { atomicAdd(p, v); }
__device__ inline void atomic_add_out(double* p, double v) {
  atomicAdd(p, v);
}
template <typename T>
__device__ inline void atomic_add_out(Cplx<T>* p, Cplx<T> v) {
  atomicAdd(&p->re, v.re);
  atomicAdd(&p->im, v.im);
}

template <typename T, bool CONJ>
__global__ __launch_bounds__(LS_THREADS) void vdot_kernel(
    const T* __restrict__ x, const T* __restrict__ y, T* __restrict__ out,
    i64 n) {
  __shared__ T partials[LS_THREADS / WAVE_SIZE];
  T acc = ls_zero<T>();
  const i64 stride = (i64)gridDim.x * blockDim.x;
  for (i64 i = (i64)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += stride) {
    if constexpr (CONJ)
      acc += ls_conj(x[i]) * y[i];
    else
      acc += x[i] * y[i];
  }
  acc = group_reduce_sum<T, WAVE_SIZE>(acc);
  const int wave = threadIdx.x / WAVE_SIZE;
  const int lane = threadIdx.x % WAVE_SIZE;
  if (lane == 0) partials[wave] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    T total = partials[0];
    for (int w = 1; w < LS_THREADS / WAVE_SIZE; ++w) total += partials[w];
    atomic_add_out(out, total);
  }
}

// Fused CG update (real dtypes): alpha = rho/pq in-kernel;
//   x += alpha*p;  r -= alpha*q;  rho_out += sum r^2
// — one pass over p,q,x,r replaces two axpby launches plus a separate
// r-dot pass (unpreconditioned CG has z = r, so the next rho IS ||r||^2).
template <typename T>
__global__ __launch_bounds__(LS_THREADS) void cg_fused_kernel(
    T* __restrict__ x, T* __restrict__ r, const T* __restrict__ p,
    const T* __restrict__ q, const T* __restrict__ rho,
    const T* __restrict__ pq, T* __restrict__ rho_out, i64 n) {
  __shared__ T partials[LS_THREADS / WAVE_SIZE];
  const T alpha = (*rho) / (*pq);
  T acc = T(0);
  const i64 stride = (i64)gridDim.x * blockDim.x;
  for (i64 i = (i64)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += stride) {
    const T xv = x[i] + alpha * p[i];
    const T rv = r[i] - alpha * q[i];
    x[i] = xv;
    r[i] = rv;
    acc += rv * rv;
  }
  acc = group_reduce_sum<T, WAVE_SIZE>(acc);
  const int wave = threadIdx.x / WAVE_SIZE;
  const int lane = threadIdx.x % WAVE_SIZE;
  if (lane == 0) partials[wave] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    T total = partials[0];
    for (int w = 1; w < LS_THREADS / WAVE_SIZE; ++w) total += partials[w];
    atomic_add_out(rho_out, total);
  }
}

// Batched Gram-Schmidt dots: out[k] += <V[k, :], w> for k < K in ONE
// pass over V (the K x n basis block) with w staged through LDS per
// block chunk.  torch's vecdot/matmul formulations either materialize
// the (K, n) product or single-tile the skinny GEMM — measured 1.2 ms
// per GMRES inner iteration at n = 4.2M; this kernel is the plain
// BW-bound pass (profiles/gmres_r02.md).
template <typename T, bool CONJ>
__global__ __launch_bounds__(LS_THREADS) void gs_dots_kernel(
    const T* __restrict__ V, i64 ld, int K, const T* __restrict__ w,
    T* __restrict__ out, i64 n) {
  constexpr int PE = 8;
  constexpr i64 CH = (i64)LS_THREADS * PE;
  __shared__ T wsh[LS_THREADS * PE];
  __shared__ T partials[LS_THREADS / WAVE_SIZE];
  const int wave = threadIdx.x / WAVE_SIZE;
  const int lane = threadIdx.x % WAVE_SIZE;
  for (i64 base = (i64)blockIdx.x * CH; base < n;
       base += (i64)gridDim.x * CH) {
    const i64 end = (base + CH < n) ? base + CH : n;
    for (i64 i = base + threadIdx.x; i < end; i += LS_THREADS)
      wsh[i - base] = w[i];
    __syncthreads();
    for (int k = 0; k < K; ++k) {
      const T* vk = V + (i64)k * ld;
      T acc = ls_zero<T>();
      for (i64 i = base + threadIdx.x; i < end; i += LS_THREADS) {
        if constexpr (CONJ)
          acc += ls_conj(vk[i]) * wsh[i - base];
        else
          acc += vk[i] * wsh[i - base];
      }
      acc = group_reduce_sum<T, WAVE_SIZE>(acc);
      if (lane == 0) partials[wave] = acc;
      __syncthreads();
      if (threadIdx.x == 0) {
        T total = partials[0];
        for (int v = 1; v < LS_THREADS / WAVE_SIZE; ++v)
          total += partials[v];
        atomic_add_out(out + k, total);
      }
      __syncthreads();
    }
    __syncthreads();
  }
}

// ---------------------------------------------------------------------------
// BiCGSTAB (docs/DESIGN.md §15).  Every scalar is one device element; the
// quotients are formed in-kernel with a GUARDED division: a (/) b is
// exactly zero when b is exactly zero, so an iteration that runs on after
// r hit zero between two convergence tests is a no-op instead of 0/0.
//
// All four kernels stream V-element packs (16 bytes when every vector
// pointer is 16-byte aligned — decided once on the host — else V = 1) in
// a capped grid-stride loop; the n % V tail is done by the first threads
// of block 0 through the V = 1 chunk.
// ---------------------------------------------------------------------------
constexpr int BICG_PER_BLOCK = LS_THREADS * 4;  // elements per block
constexpr int BICG_GRID_CAP = 2048;

template <typename T>
__device__ inline T ls_gdiv(T a, T b) {
  return ls_is_zero(b) ? T(0) : a / b;
}
// complex: Smith's division — Cplx::operator/ squares the denominator,
// which under/overflows fp32 for the tiny <t,t> of a nearly converged solve
template <typename T>
__device__ inline Cplx<T> ls_gdiv(Cplx<T> a, Cplx<T> b) {
  if (ls_is_zero(b)) return {T(0), T(0)};
  if (fabs(b.re) >= fabs(b.im)) {
    const T q = b.im / b.re;
    const T d = b.re + b.im * q;
    return {(a.re + a.im * q) / d, (a.im - a.re * q) / d};
  }
  const T q = b.re / b.im;
  const T d = b.re * q + b.im;
  return {(a.re * q + a.im) / d, (a.im * q - a.re) / d};
}

template <typename T, int V>
struct alignas(V == 1 ? alignof(T) : sizeof(T) * V) Pack {
  T e[V];
};
template <typename T, int V>
__device__ inline Pack<T, V> ld_pack(const T* p) {
  return *reinterpret_cast<const Pack<T, V>*>(p);
}
template <typename T, int V>
__device__ inline void st_pack(T* p, const Pack<T, V>& k) {
  *reinterpret_cast<Pack<T, V>*>(p) = k;
}

// block-reduce two accumulators, one atomic per block per output
template <typename T>
__device__ inline void block_reduce2_out(T a0, T a1, T* out2) {
  __shared__ T partials[2][LS_THREADS / WAVE_SIZE];
  a0 = group_reduce_sum<T, WAVE_SIZE>(a0);
  a1 = group_reduce_sum<T, WAVE_SIZE>(a1);
  const int wave = threadIdx.x / WAVE_SIZE;
  const int lane = threadIdx.x % WAVE_SIZE;
  if (lane == 0) {
    partials[0][wave] = a0;
    partials[1][wave] = a1;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    T t0 = partials[0][0], t1 = partials[1][0];
    for (int w = 1; w < LS_THREADS / WAVE_SIZE; ++w) {
      t0 += partials[0][w];
      t1 += partials[1][w];
    }
    atomic_add_out(out2, t0);
    atomic_add_out(out2 + 1, t1);
  }
}

// p <- r + beta (p - omega v)
template <typename T, int V>
__device__ inline void bicg_p_chunk(T* p, const T* r, const T* v, T beta,
                                    T omega, i64 i) {
  Pack<T, V> pk = ld_pack<T, V>(p + i);
  const Pack<T, V> rk = ld_pack<T, V>(r + i), vk = ld_pack<T, V>(v + i);
#pragma unroll
  for (int j = 0; j < V; ++j)
    pk.e[j] = rk.e[j] + beta * (pk.e[j] - omega * vk.e[j]);
  st_pack<T, V>(p + i, pk);
}

template <typename T, int V>
__global__ __launch_bounds__(LS_THREADS) void bicgstab_p_kernel(
    T* __restrict__ p, const T* __restrict__ r, const T* __restrict__ v,
    const T* __restrict__ rho, const T* __restrict__ rhv,
    const T* __restrict__ ts, const T* __restrict__ tt, i64 n) {
  const T omega = ls_gdiv(*ts, *tt);
  // two benign quotients, not rho*tt / (rhv*ts): no fp32 overflow
  const T beta = ls_gdiv(*rho, *rhv) * ls_gdiv(*tt, *ts);
  const i64 tid = (i64)blockIdx.x * blockDim.x + threadIdx.x;
  const i64 stride = (i64)gridDim.x * blockDim.x;
  const i64 nv = n / V;
  for (i64 k = tid; k < nv; k += stride)
    bicg_p_chunk<T, V>(p, r, v, beta, omega, k * V);
  if constexpr (V > 1) {
    const i64 i = nv * V + tid;
    if (i < n) bicg_p_chunk<T, 1>(p, r, v, beta, omega, i);
  }
}

// s <- r - alpha v
template <typename T, int V>
__device__ inline void bicg_s_chunk(T* s, const T* r, const T* v, T alpha,
                                    i64 i) {
  const Pack<T, V> rk = ld_pack<T, V>(r + i), vk = ld_pack<T, V>(v + i);
  Pack<T, V> sk;
#pragma unroll
  for (int j = 0; j < V; ++j) sk.e[j] = rk.e[j] - alpha * vk.e[j];
  st_pack<T, V>(s + i, sk);
}

template <typename T, int V>
__global__ __launch_bounds__(LS_THREADS) void bicgstab_s_kernel(
    T* __restrict__ s, const T* __restrict__ r, const T* __restrict__ v,
    const T* __restrict__ rho, const T* __restrict__ rhv, i64 n) {
  const T alpha = ls_gdiv(*rho, *rhv);
  const i64 tid = (i64)blockIdx.x * blockDim.x + threadIdx.x;
  const i64 stride = (i64)gridDim.x * blockDim.x;
  const i64 nv = n / V;
  for (i64 k = tid; k < nv; k += stride)
    bicg_s_chunk<T, V>(s, r, v, alpha, k * V);
  if constexpr (V > 1) {
    const i64 i = nv * V + tid;
    if (i < n) bicg_s_chunk<T, 1>(s, r, v, alpha, i);
  }
}

// a0 += conj(t) s ; a1 += conj(t) t
template <typename T, int V>
__device__ inline void vdot2_chunk(const T* t, const T* s, T& a0, T& a1,
                                   i64 i) {
  const Pack<T, V> tk = ld_pack<T, V>(t + i), sk = ld_pack<T, V>(s + i);
#pragma unroll
  for (int j = 0; j < V; ++j) {
    const T tc = ls_conj(tk.e[j]);
    a0 += tc * sk.e[j];
    a1 += tc * tk.e[j];
  }
}

template <typename T, int V>
__global__ __launch_bounds__(LS_THREADS) void vdot2_kernel(
    const T* __restrict__ t, const T* __restrict__ s, T* __restrict__ out2,
    i64 n) {
  T a0 = ls_zero<T>(), a1 = ls_zero<T>();
  const i64 tid = (i64)blockIdx.x * blockDim.x + threadIdx.x;
  const i64 stride = (i64)gridDim.x * blockDim.x;
  const i64 nv = n / V;
  for (i64 k = tid; k < nv; k += stride)
    vdot2_chunk<T, V>(t, s, a0, a1, k * V);
  if constexpr (V > 1) {
    const i64 i = nv * V + tid;
    if (i < n) vdot2_chunk<T, 1>(t, s, a0, a1, i);
  }
  block_reduce2_out(a0, a1, out2);
}

// x <- x + alpha phat + omega shat ; r <- s - omega t ;
// a0 += conj(rhat) r ; a1 += conj(r) r
template <typename T, int V>
__device__ inline void bicg_xr_chunk(T* x, T* r, const T* phat,
                                     const T* shat, const T* s, const T* t,
                                     const T* rhat, T alpha, T omega, T& a0,
                                     T& a1, i64 i) {
  Pack<T, V> xk = ld_pack<T, V>(x + i);
  const Pack<T, V> pk = ld_pack<T, V>(phat + i),
                   hk = ld_pack<T, V>(shat + i), sk = ld_pack<T, V>(s + i),
                   tk = ld_pack<T, V>(t + i), qk = ld_pack<T, V>(rhat + i);
  Pack<T, V> rk;
#pragma unroll
  for (int j = 0; j < V; ++j) {
    xk.e[j] = xk.e[j] + alpha * pk.e[j] + omega * hk.e[j];
    const T rn = sk.e[j] - omega * tk.e[j];
    rk.e[j] = rn;
    a0 += ls_conj(qk.e[j]) * rn;
    a1 += ls_conj(rn) * rn;
  }
  st_pack<T, V>(x + i, xk);
  st_pack<T, V>(r + i, rk);
}

// phat/shat may alias each other's sources (phat == p, shat == s when
// unpreconditioned): read-only here, so only x and r carry __restrict__
template <typename T, int V>
__global__ __launch_bounds__(LS_THREADS) void bicgstab_xr_kernel(
    T* __restrict__ x, T* __restrict__ r, const T* phat, const T* shat,
    const T* s, const T* t, const T* rhat, const T* rho, const T* rhv,
    const T* ts, const T* tt, T* out2, i64 n) {
  const T alpha = ls_gdiv(*rho, *rhv);
  const T omega = ls_gdiv(*ts, *tt);
  T a0 = ls_zero<T>(), a1 = ls_zero<T>();
  const i64 tid = (i64)blockIdx.x * blockDim.x + threadIdx.x;
  const i64 stride = (i64)gridDim.x * blockDim.x;
  const i64 nv = n / V;
  for (i64 k = tid; k < nv; k += stride)
    bicg_xr_chunk<T, V>(x, r, phat, shat, s, t, rhat, alpha, omega, a0, a1,
                        k * V);
  if constexpr (V > 1) {
    const i64 i = nv * V + tid;
    if (i < n)
      bicg_xr_chunk<T, 1>(x, r, phat, shat, s, t, rhat, alpha, omega, a0,
                          a1, i);
  }
  block_reduce2_out(a0, a1, out2);
}

// all vector pointers 16-byte aligned -> 16-byte packs, else element-wise
template <typename... P>
inline bool bicg_aligned16(P... ptrs) {
  return (((ptrs) % 16 == 0) && ...);
}

}  // namespace

int ls_bicgstab_grid_cap() { return BICG_GRID_CAP; }
int ls_bicgstab_per_block() { return BICG_PER_BLOCK; }

// V = 16 / sizeof(val_t) when aligned (1 for complex128 either way)
#define BICG_LAUNCH(kernel, aligned, ...)                                  \
  do {                                                                     \
    constexpr int VW = 16 / (int)sizeof(val_t);                            \
    if constexpr (VW > 1) {                                                \
      if (aligned) {                                                       \
        hipLaunchKernelGGL((kernel<val_t, VW>), dim3(grid),                \
                           dim3(LS_THREADS), 0, s, __VA_ARGS__);           \
        break;                                                             \
      }                                                                    \
    }                                                                      \
    hipLaunchKernelGGL((kernel<val_t, 1>), dim3(grid), dim3(LS_THREADS),   \
                       0, s, __VA_ARGS__);                                 \
  } while (0)

void ls_bicgstab_p(uintptr_t p, uintptr_t r, uintptr_t v, uintptr_t rho,
                   uintptr_t rhv, uintptr_t ts, uintptr_t tt, i64 n,
                   int dtype, uintptr_t stream) {
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const int grid = grid_1d(n, BICG_PER_BLOCK, BICG_GRID_CAP);
  const bool al = bicg_aligned16(p, r, v);
  DISPATCH_VAL_T(dtype, ({
    BICG_LAUNCH(bicgstab_p_kernel, al, reinterpret_cast<val_t*>(p),
                reinterpret_cast<const val_t*>(r),
                reinterpret_cast<const val_t*>(v),
                reinterpret_cast<const val_t*>(rho),
                reinterpret_cast<const val_t*>(rhv),
                reinterpret_cast<const val_t*>(ts),
                reinterpret_cast<const val_t*>(tt), n);
  }));
  ls_check(hipGetLastError(), "bicgstab_p");
}

void ls_bicgstab_s(uintptr_t sv, uintptr_t r, uintptr_t v, uintptr_t rho,
                   uintptr_t rhv, i64 n, int dtype, uintptr_t stream) {
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const int grid = grid_1d(n, BICG_PER_BLOCK, BICG_GRID_CAP);
  const bool al = bicg_aligned16(sv, r, v);
  DISPATCH_VAL_T(dtype, ({
    BICG_LAUNCH(bicgstab_s_kernel, al, reinterpret_cast<val_t*>(sv),
                reinterpret_cast<const val_t*>(r),
                reinterpret_cast<const val_t*>(v),
                reinterpret_cast<const val_t*>(rho),
                reinterpret_cast<const val_t*>(rhv), n);
  }));
  ls_check(hipGetLastError(), "bicgstab_s");
}

void ls_vdot2(uintptr_t t, uintptr_t sv, uintptr_t out2, i64 n, int dtype,
              uintptr_t stream) {
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const int grid = grid_1d(n, BICG_PER_BLOCK, BICG_GRID_CAP);
  const bool al = bicg_aligned16(t, sv);
  DISPATCH_VAL_T(dtype, ({
    BICG_LAUNCH(vdot2_kernel, al, reinterpret_cast<const val_t*>(t),
                reinterpret_cast<const val_t*>(sv),
                reinterpret_cast<val_t*>(out2), n);
  }));
  ls_check(hipGetLastError(), "vdot2");
}

void ls_bicgstab_xr(uintptr_t x, uintptr_t r, uintptr_t phat, uintptr_t shat,
                    uintptr_t sv, uintptr_t t, uintptr_t rhat, uintptr_t rho,
                    uintptr_t rhv, uintptr_t ts, uintptr_t tt, uintptr_t out2,
                    i64 n, int dtype, uintptr_t stream) {
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const int grid = grid_1d(n, BICG_PER_BLOCK, BICG_GRID_CAP);
  const bool al = bicg_aligned16(x, r, phat, shat, sv, t, rhat);
  DISPATCH_VAL_T(dtype, ({
    BICG_LAUNCH(bicgstab_xr_kernel, al, reinterpret_cast<val_t*>(x),
                reinterpret_cast<val_t*>(r),
                reinterpret_cast<const val_t*>(phat),
                reinterpret_cast<const val_t*>(shat),
                reinterpret_cast<const val_t*>(sv),
                reinterpret_cast<const val_t*>(t),
                reinterpret_cast<const val_t*>(rhat),
                reinterpret_cast<const val_t*>(rho),
                reinterpret_cast<const val_t*>(rhv),
                reinterpret_cast<const val_t*>(ts),
                reinterpret_cast<const val_t*>(tt),
                reinterpret_cast<val_t*>(out2), n);
  }));
  ls_check(hipGetLastError(), "bicgstab_xr");
}

void ls_gs_dots(uintptr_t V, i64 ld, int K, uintptr_t w, uintptr_t out,
                i64 n, bool conj, int dtype, uintptr_t stream) {
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  int grid = grid_1d(n, LS_THREADS * 8, 4096);
  DISPATCH_VAL_T(dtype, ({
    auto vp = reinterpret_cast<const val_t*>(V);
    auto wp = reinterpret_cast<const val_t*>(w);
    auto op = reinterpret_cast<val_t*>(out);
    if (conj)
      hipLaunchKernelGGL((gs_dots_kernel<val_t, true>), dim3(grid),
                         dim3(LS_THREADS), 0, s, vp, ld, K, wp, op, n);
    else
      hipLaunchKernelGGL((gs_dots_kernel<val_t, false>), dim3(grid),
                         dim3(LS_THREADS), 0, s, vp, ld, K, wp, op, n);
  }));
  ls_check(hipGetLastError(), "gs_dots");
}

void ls_cg_fused(uintptr_t x, uintptr_t r, uintptr_t p, uintptr_t q,
                 uintptr_t rho, uintptr_t pq, uintptr_t rho_out, i64 n,
                 int dtype, uintptr_t stream) {
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  static const int pe = [] {
    const char* e = std::getenv("LS_CGF_PE");
    return e ? atoi(e) : 4;
  }();
  static const int cap = [] {
    const char* e = std::getenv("LS_CGF_CAP");
    return e ? atoi(e) : 4096;
  }();
  int grid = grid_1d(n, LS_THREADS * pe, cap);
  if (dtype == 0)
    hipLaunchKernelGGL((cg_fused_kernel<float>), dim3(grid),
                       dim3(LS_THREADS), 0, s,
                       reinterpret_cast<float*>(x),
                       reinterpret_cast<float*>(r),
                       reinterpret_cast<const float*>(p),
                       reinterpret_cast<const float*>(q),
                       reinterpret_cast<const float*>(rho),
                       reinterpret_cast<const float*>(pq),
                       reinterpret_cast<float*>(rho_out), n);
  else if (dtype == 1)
    hipLaunchKernelGGL((cg_fused_kernel<double>), dim3(grid),
                       dim3(LS_THREADS), 0, s,
                       reinterpret_cast<double*>(x),
                       reinterpret_cast<double*>(r),
                       reinterpret_cast<const double*>(p),
                       reinterpret_cast<const double*>(q),
                       reinterpret_cast<const double*>(rho),
                       reinterpret_cast<const double*>(pq),
                       reinterpret_cast<double*>(rho_out), n);
  else
    throw std::runtime_error("cg_fused: real dtypes only");
  ls_check(hipGetLastError(), "cg_fused");
}

void ls_axpby(uintptr_t y, uintptr_t x, uintptr_t a, uintptr_t b, i64 n,
              bool isalpha, bool negate, int dtype, uintptr_t stream) {
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  int grid = grid_1d(n, LS_THREADS, 4096);
  DISPATCH_VAL_T(dtype, ({
    auto yp = reinterpret_cast<val_t*>(y);
    auto xp = reinterpret_cast<const val_t*>(x);
    auto ap = reinterpret_cast<const val_t*>(a);
    auto bp = reinterpret_cast<const val_t*>(b);
    if (isalpha) {
      if (negate)
        hipLaunchKernelGGL((axpby_kernel<val_t, true, true>), dim3(grid),
                           dim3(LS_THREADS), 0, s, yp, xp, ap, bp, n);
      else
        hipLaunchKernelGGL((axpby_kernel<val_t, true, false>), dim3(grid),
                           dim3(LS_THREADS), 0, s, yp, xp, ap, bp, n);
    } else {
      if (negate)
        hipLaunchKernelGGL((axpby_kernel<val_t, false, true>), dim3(grid),
                           dim3(LS_THREADS), 0, s, yp, xp, ap, bp, n);
      else
        hipLaunchKernelGGL((axpby_kernel<val_t, false, false>), dim3(grid),
                           dim3(LS_THREADS), 0, s, yp, xp, ap, bp, n);
    }
  }));
  ls_check(hipGetLastError(), "axpby");
}

void ls_jacobi(uintptr_t x, uintptr_t b, uintptr_t y, uintptr_t dinv,
               double omega, i64 n, int dtype, uintptr_t stream) {
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  int grid = grid_1d(n, LS_THREADS, 4096);
  DISPATCH_VAL_T(dtype, hipLaunchKernelGGL(
      (jacobi_kernel<val_t>), dim3(grid), dim3(LS_THREADS), 0, s,
      reinterpret_cast<val_t*>(x), reinterpret_cast<const val_t*>(b),
      reinterpret_cast<const val_t*>(y),
      reinterpret_cast<const val_t*>(dinv), omega, n));
  ls_check(hipGetLastError(), "jacobi");
}

void ls_vdot(uintptr_t x, uintptr_t y, uintptr_t out, i64 n, bool conj,
             int dtype, uintptr_t stream) {
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  int grid = grid_1d(n, LS_THREADS * 8, 2048);
  DISPATCH_VAL_T(dtype, ({
    auto xp = reinterpret_cast<const val_t*>(x);
    auto yp = reinterpret_cast<const val_t*>(y);
    auto op = reinterpret_cast<val_t*>(out);
    if (conj)
      hipLaunchKernelGGL((vdot_kernel<val_t, true>), dim3(grid),
                         dim3(LS_THREADS), 0, s, xp, yp, op, n);
    else
      hipLaunchKernelGGL((vdot_kernel<val_t, false>), dim3(grid),
                         dim3(LS_THREADS), 0, s, xp, yp, op, n);
  }));
  ls_check(hipGetLastError(), "vdot");
}

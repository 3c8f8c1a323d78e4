// Periods.project over a batch, the all-p sweep, Periods.periodic_norm and the dictionary projection of
// RamanujanPeriods.  Reference citations are file:line into /root/reference/pyPeriod/.
#pragma once

#include <type_traits>

#include "ph_device.h"

namespace ph {

// ======================================================================================
// K1  Periods.project over a batch  (Periods.py:142-219)
//   grid.x = W * chunks; each workgroup projects its window onto p_list[k0 .. k1).
//   Non-orth: means stay in registers and rows stream straight to HBM (write-bound).
//   Orth: projection is materialised in a second LDS buffer, sub-projections removed there.
// ======================================================================================
template <typename T>
struct ProjectLds {
  T* xs;
  T* buf;  // orth: the whole projection is materialised here; otherwise only one period of means
  size_t bytes;
};
template <typename T, class C>
__host__ __device__ __forceinline__ ProjectLds<T> project_carve(C cv, int N, int scratch_len, bool lw, bool buf_lds) {
  ProjectLds<T> L;
  L.xs = lw ? cv.template take<T>(N) : nullptr;
  L.buf = buf_lds ? cv.template take<T>(scratch_len) : nullptr;
  L.bytes = cv.off;
  return L;
}

template <typename T, bool LW>
__global__ __launch_bounds__(kBlock) void k_project_batch(const T* __restrict__ x, int N,
                                                          const int* __restrict__ p_list, int n_p, int chunks,
                                                          unsigned flags, Tables tb, int scratch_len,
                                                          T* __restrict__ gbuf, T* gwin, T* __restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  // gbuf != nullptr: the window is too long for two LDS buffers, the second one lives in HBM.
  const ProjectLds<T> L = project_carve<T>(Carve(smem), N, scratch_len, LW, !gbuf);
  T* xs = window_buf<T, LW>(L.xs, gwin, N);
  T* buf = second_buf(L.buf, gbuf, scratch_len);

  const int64_t w = blockIdx.x / chunks;
  const int c = blockIdx.x % chunks;
  const int per = (n_p + chunks - 1) / chunks;
  const int k0 = c * per;
  const int k1 = min(n_p, k0 + per);
  load_window(x + w * (int64_t)N, xs, N);
  __syncthreads();

  const bool trunc = flags & kTrunc;
  const bool single = flags & kSingle;
  constexpr int V = 16 / sizeof(T);
  for (int k = k0; k < k1; ++k) {
    const int p = p_list[k];
    T* orow = out + (w * n_p + k) * (int64_t)N;
    const int lim = single ? min(p, N) : N;
    if (!(flags & kOrth)) {
      // means in row order (bit-identical to the reference), one per residue that exists
      const Fold f(N, p);
      const int np = min(p, N);
      for (int j = threadIdx.x; j < np; j += blockDim.x) buf[j] = residue_mean(xs, f, j, trunc);
      __syncthreads();
      // tile (Periods.py:196-198): coalesced 16-byte stores, n mod p kept incrementally
      if ((N % V) == 0 && (lim % V) == 0) {
        using vec_t = typename std::conditional<sizeof(T) == 8, double2, float4>::type;
        const int stride = blockDim.x * V;
        int j = (threadIdx.x * V) % p;
        const int step = stride % p;
        for (int n = threadIdx.x * V; n < lim; n += stride) {
          T v[V];
          int jj = j;
#pragma unroll
          for (int e = 0; e < V; ++e) {
            v[e] = buf[jj];
            jj = (jj + 1 == p) ? 0 : jj + 1;
          }
          *reinterpret_cast<vec_t*>(orow + n) = *reinterpret_cast<const vec_t*>(v);
          j += step;
          if (j >= p) j -= p;
        }
      } else {
        int j = threadIdx.x % p;
        const int step = blockDim.x % p;
        for (int n = threadIdx.x; n < lim; n += blockDim.x) {
          orow[n] = buf[j];
          j += step;
          if (j >= p) j -= p;
        }
      }
      __syncthreads();  // buf is rewritten by the next period
    } else {
      project_lds(xs, buf, N, p, flags, tb);
      for (int n = threadIdx.x; n < lim; n += blockDim.x) orow[n] = buf[n];
      __syncthreads();
    }
  }
}

// ======================================================================================
// K2  fused all-p sweep  (inner loops Periods.py:501-510, :324-331)
//   grid.x = W * chunks.  Fast path (no flags): wave-per-period, no workgroup barrier after
//   the window load.  Flagged path: workgroup-cooperative full projection per period.
// ======================================================================================
// LDS bytes of k_sweep for the host.  The kernel spells its takes out itself (see there) and this is their count, kept
// in step by hand: a piece added to one is added to the other.
template <typename T>
__host__ __device__ inline size_t sweep_lds_bytes(int N, bool lw, bool buf_lds) {
  CarveCount cv;
  if (lw) cv.take<T>(N + kPad);         // xs
  if (buf_lds) cv.take<T>(N);           // buf: the projection of the norm modes with trunc / orth
  cv.take<double>(kRedDoubles);         // red
  cv.take<int>(4);                      // qctr
  return cv.off;
}

template <typename T, bool LW>
__global__ __launch_bounds__(1024) __attribute__((amdgpu_waves_per_eu(PH_STEP1_WAVES, 8))) void k_sweep(const T* __restrict__ x, int N, int p_lo, int p_hi, int mode,
                                                      int chunks, unsigned flags, Tables tb,
                                                      const PGeom* __restrict__ geom,
                                                      const PassPlan* __restrict__ plan, int n_pass,
                                                      T* __restrict__ gbuf, T* gwin,
                                                      double* __restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  // The takes are spelled out here, not run through a carve function as in the other kernels: with one, this kernel's
  // trunc / orth path measured 6.6 % slower (profiles/lds_layout).  The host counts them in sweep_lds_bytes above.
  Carve cv(smem);
  T* xs = window_buf<T, LW>(LW ? cv.take<T>(N + kPad) : nullptr, gwin, N + kPad);
  const bool general = (flags & (kTrunc | kOrth)) && mode != 2;
  T* buf = !general ? nullptr : gbuf ? gbuf + (int64_t)blockIdx.x * N : cv.take<T>(N);
  double* red = cv.take<double>(kRedDoubles);
  int* qctr = cv.take<int>(4);  // pass queue of the norm modes

  const int64_t w = blockIdx.x / chunks;
  const int c = blockIdx.x % chunks;
  const int P = p_hi - p_lo + 1;
  const int per = (P + chunks - 1) / chunks;
  const int pa = p_lo + c * per;
  const int pb = min(p_hi, pa + per - 1);
  load_window(x + w * (int64_t)N, xs, N);
  zero_pad(xs, N);
  if (threadIdx.x == 0) qctr[0] = c * ((n_pass + chunks - 1) / chunks) + (int)(blockDim.x >> 6);
  __syncthreads();
  double* orow = out + w * (int64_t)P;

  if (!general) {
    const int lane = threadIdx.x & (kWave - 1);
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int nw = blockDim.x >> 6;
    if (mode == 2) {
      wave_sweep<T, true, LW>(xs, N, geom, pa + wv, pb, nw, lane, [&](double v, int p) {
        if ((lane & 7) == 0) orow[p - p_lo] = v;
      });
    } else {
      // norm modes: the workgroups of a window split the pass plan, not the period range
      const int pper = (n_pass + chunks - 1) / chunks;
      const int i0 = c * pper, i1 = min(n_pass, i0 + pper);
      wave_sweep_plan<T, LW>(
          xs, N, geom, plan, i0 + wv, i1, nw, lane,
          [&](double v, int p) {
            if ((lane & 7) == 0) orow[p - p_lo] = periodic_norm_from_sq(v, N, mode == 1 ? p : 0);
          },
          qctr);
    }
  } else {
    for (int p = pa; p <= pb; ++p) {
      const double v = block_sweep_value(xs, buf, N, p, mode == 1 ? p : 0, flags, tb, red);
      if (threadIdx.x == 0) orow[p - p_lo] = v;
    }
  }
}

// ======================================================================================
// Periods.periodic_norm over a batch (Periods.py:221-241); streams from HBM, any N.
// ======================================================================================
template <typename T>
__global__ __launch_bounds__(kBlock) void k_periodic_norm(const T* __restrict__ x, int N, int p_div,
                                                          double* __restrict__ out) {
  __shared__ double red[kRedDoubles];
  const int64_t w = blockIdx.x;
  const T* row = x + w * (int64_t)N;
  double acc = 0.0;
  for (int n = threadIdx.x; n < N; n += blockDim.x) {
    const double t = (double)row[n];
    acc += t * t;
  }
  const double ss = block_sum(acc, red);
  if (threadIdx.x == 0) out[w] = periodic_norm_from_sq(ss, N, p_div);
}

// ======================================================================================
// RamanujanPeriods.project(x, basis) (RamanujanPeriods.py:124-131) for an arbitrary
// dictionary: row <- row / max(row); out[i] = float32(dot(x, row) * row).  One workgroup
// per dictionary row, rows streamed from HBM twice (max, then dot+scale from L2).
// ======================================================================================
__global__ __launch_bounds__(kBlock) void k_dict_project(const double* __restrict__ x,
                                                         const double* __restrict__ basis, int N,
                                                         float* __restrict__ out) {
  __shared__ double red[kRedDoubles];
  const int64_t i = blockIdx.x;
  const double* row = basis + i * (int64_t)N;
  double m = -INFINITY;
  for (int n = threadIdx.x; n < N; n += blockDim.x) m = fmax(m, row[n]);
  m = wave_max(m);
  if ((threadIdx.x & (kWave - 1)) == 0) red[threadIdx.x >> 6] = m;
  __syncthreads();
  m = red[0];
  for (int k = 1; k < (int)(blockDim.x >> 6); ++k) m = fmax(m, red[k]);
  __syncthreads();
  double acc = 0.0;
  for (int n = threadIdx.x; n < N; n += blockDim.x) acc += x[n] * (row[n] / m);
  const double dot = block_sum(acc, red);
  for (int n = threadIdx.x; n < N; n += blockDim.x) out[i * (int64_t)N + n] = (float)(dot * (row[n] / m));
}

}  // namespace ph

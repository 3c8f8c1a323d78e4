// Periods.best_frequency: direct spectrum, FFT, chirp-z and the residual update.
#pragma once

#include "ph_device.h"

namespace ph {

// ======================================================================================
// Periods.best_frequency  (Periods.py:351-398).  Two launches per round:
//   k_bf_spectrum: grid (bin chunks, W).  The residual is staged in LDS; thread per rfft bin k,
//     X[k] = sum_n x[n] (cos - i sin)(2 pi k n / L) with the phase index k n mod L kept
//     incrementally and the twiddles read from a float64 table (L2-resident); every workgroup
//     leaves its best (|X|^2, k), first maximum.  A single window still fills the chip.
//   The bins are ranked on |2^-e X[k]|^2 with e = floor(log2 max |x|) over the samples the transform reads
//   (bf_scale_exp): |X|^2 itself is inf in every bin for a window scaled by 2^520 and 0 in every bin near 2^-560,
//   where numpy's np.abs (hypot) still ranks.  The factor is a power of two, so a window whose |X|^2 stays in range
//   ranks exactly as before.
//   k_bf_update: one workgroup per window: argmax over the chunks, p = rint(2 L / k), project
//     (all flag combinations), store, subtract, residual back to the HBM workspace.
// ======================================================================================
constexpr int kBfBlock = 256;

// floor(log2 max_n |x[n]|) from every thread's share `m` of the maximum (0 for an all-zero window or one without a
// finite maximum; fmax skips NaN samples, which poison every bin anyway).  `red` holds >= kMaxWaves doubles; ends with
// a barrier.
__device__ __forceinline__ int bf_scale_exp(double m, double* red) {
  m = block_max(m, red);
  return (m > 0.0 && m <= 1.7976931348623157e308) ? ilogb(m) : 0;
}
// re^2 + im^2 of 2^-e (re + i im)
__device__ __forceinline__ double bf_mag2(double re, double im, int e) {
  const double r = ldexp(re, -e), i = ldexp(im, -e);
  return r * r + i * i;
}

// LDS of the three spectrum kernels: the staged window (k_bf_spectrum, when it is in LDS) or the complex work array of
// n points (k_bf_fft: n = L, k_bf_chirp: n = M), then the slots of the peak reduction.
template <typename T>
struct BfSpectrumLds {
  T* stage;
  double* re;
  double* im;
  double* wbest;
  int* wbestp;
  size_t bytes;
};
template <typename T, class C>
__host__ __device__ __forceinline__ BfSpectrumLds<T> bf_spectrum_carve(C cv, size_t stage_len, size_t n) {
  BfSpectrumLds<T> L;
  L.stage = stage_len ? cv.template take<T>(stage_len) : nullptr;
  L.re = n ? cv.template take<double>(n) : nullptr;
  L.im = n ? cv.template take<double>(n) : nullptr;
  L.wbest = cv.template take<double>(kMaxWaves);
  L.wbestp = cv.template take<int>(kMaxWaves);
  L.bytes = cv.off;
  return L;
}

template <typename T, bool LW>
__global__ __launch_bounds__(kBfBlock) void k_bf_spectrum(const T* __restrict__ res, int N, int L,
                                                          const double2* __restrict__ tw,
                                                          const int* __restrict__ status,
                                                          double* __restrict__ part_m2, int* __restrict__ part_k) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const BfSpectrumLds<T> lds = bf_spectrum_carve<T>(Carve(smem), LW ? N : 0, 0);
  const int64_t w = blockIdx.y;
  const T* xs = res + w * (int64_t)N;  // LW == false: every thread walks the residual in HBM / L2 (broadcast reads)
  T* stage = lds.stage;
  double* wbest = lds.wbest;
  int* wbestp = lds.wbestp;
  const int chunk = blockIdx.x, nchunk = gridDim.x;
  if (status[w] != 0) return;  // the reference has raised for this window already
  const int tid = threadIdx.x, lane = tid & (kWave - 1);
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6), nw = blockDim.x >> 6;
  const int M = N < L ? N : L;  // rfft(data, L) truncates or zero-pads to L samples
  if constexpr (LW) {
    load_window(xs, stage, N);
    __syncthreads();
    xs = stage;
  }
  double xmax = 0.0;
  for (int n = tid; n < M; n += blockDim.x) xmax = fmax(xmax, fabs((double)xs[n]));
  const int e = bf_scale_exp(xmax, wbest);
  double best = -1.0;
  int bestk = 0;  // bin + 1; 0 = none
  const int k = chunk * (int)blockDim.x + tid;
  if (k <= L / 2) {
    double re = 0.0, im = 0.0;
    int idx = 0;
    for (int n = 0; n < M; ++n) {
      const double xv = (double)xs[n];
      const double2 cs = tw[idx];
      re = fma(xv, cs.x, re);
      im = fma(xv, cs.y, im);
      idx += k;
      if (idx >= L) idx -= L;
    }
    const double m2 = bf_mag2(re, im, e);
    if (m2 > best) {  // false for NaN
      best = m2;
      bestk = k + 1;
    }
  }
  wave_argmax(best, bestk);
  if (lane == 0) {
    wbest[wv] = best;
    wbestp[wv] = bestk;
  }
  __syncthreads();
  if (tid == 0) {
    best = -1.0;
    bestk = 0;
    for (int i = 0; i < nw; ++i)
      if (wbestp[i] != 0 && (bestk == 0 || wbest[i] > best || (wbest[i] == best && wbestp[i] < bestk))) {
        best = wbest[i];
        bestk = wbestp[i];
      }
    part_m2[w * nchunk + chunk] = best;
    part_k[w * nchunk + chunk] = bestk;
  }
}

// In-LDS radix-2 FFT stages (decimation in time; the data is already in bit-reversed order):
// log2 L stages of L / 2 butterflies, twiddles exp(-2 pi i j / 2^s) from a float64 (cos, sin) table
// of the L-th roots.  Ends with a barrier.
__device__ __forceinline__ void lds_fft_stages(double* __restrict__ re, double* __restrict__ im, int L, int logL,
                                               const double2* __restrict__ tw) {
  for (int s = 1; s <= logL; ++s) {
    const int half = 1 << (s - 1);
    const int tstep = L >> s;
    for (int b = threadIdx.x; b < (L >> 1); b += blockDim.x) {
      const int j = b & (half - 1);
      const int a0 = ((b >> (s - 1)) << s) + j, a1 = a0 + half;
      const double2 cs = tw[j * tstep];  // (cos, sin) of +angle; the forward transform uses cos - i sin
      const double xr = re[a1], xi = im[a1];
      const double tr = fma(xr, cs.x, xi * cs.y), ti = fma(xi, cs.x, -xr * cs.y);
      const double ur = re[a0], ui = im[a0];
      re[a0] = ur + tr;
      im[a0] = ui + ti;
      re[a1] = ur - tr;
      im[a1] = ui - ti;
    }
    __syncthreads();
  }
}

// First maximum of |2^-e (re[k] + i im[k])|^2 over k <= kmax -> the (|X|^2, bin + 1) record of window w, slot 0.
__device__ __forceinline__ void bf_store_peak(const double* __restrict__ re, const double* __restrict__ im, int kmax, int e,
                                              double* wbest, int* wbestp, int64_t w, double* __restrict__ part_m2,
                                              int* __restrict__ part_k) {
  const int tid = threadIdx.x, lane = tid & (kWave - 1);
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6), nw = blockDim.x >> 6;
  double best = -1.0;
  int bestk = 0;  // bin + 1; 0 = none
  for (int k = tid; k <= kmax; k += blockDim.x) {
    const double m2 = bf_mag2(re[k], im[k], e);
    if (m2 > best) {  // false for NaN; ascending k per thread keeps the first maximum
      best = m2;
      bestk = k + 1;
    }
  }
  wave_argmax(best, bestk);
  if (lane == 0) {
    wbest[wv] = best;
    wbestp[wv] = bestk;
  }
  __syncthreads();
  if (tid == 0) {
    best = -1.0;
    bestk = 0;
    for (int i = 0; i < nw; ++i)
      if (wbestp[i] != 0 && (bestk == 0 || wbest[i] > best || (wbest[i] == best && wbestp[i] < bestk))) {
        best = wbest[i];
        bestk = wbestp[i];
      }
    part_m2[w] = best;
    part_k[w] = bestk;
  }
}

// Power-of-two win_size that fits the LDS: the spectrum is an in-LDS radix-2 FFT, one workgroup per
// window -- O(L log L) instead of the O(N L) of the direct DFT above.  Leaves the same
// (|X|^2, bin + 1) record, first maximum, in chunk slot 0.
template <typename T>
__global__ __launch_bounds__(kBlockWide) void k_bf_fft(const T* __restrict__ res, int N, int L, int logL,
                                                       const double2* __restrict__ tw,
                                                       const int* __restrict__ status,
                                                       double* __restrict__ part_m2, int* __restrict__ part_k) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const BfSpectrumLds<T> lds = bf_spectrum_carve<T>(Carve(smem), 0, L);
  double *re = lds.re, *im = lds.im, *wbest = lds.wbest;
  int* wbestp = lds.wbestp;
  const int64_t w = blockIdx.x;
  if (status[w] != 0) return;  // the reference has raised for this window already
  const int M0 = N < L ? N : L;  // rfft(data, L) truncates or zero-pads to L samples
  const T* xs = res + w * (int64_t)N;
  double xmax = 0.0;
  for (int n = threadIdx.x; n < L; n += blockDim.x) {
    const int r = (int)(__brev((unsigned)n) >> (32 - logL));
    const double xv = n < M0 ? (double)xs[n] : 0.0;
    xmax = fmax(xmax, fabs(xv));
    re[r] = xv;
    im[r] = 0.0;
  }
  const int e = bf_scale_exp(xmax, wbest);  // (its barrier completes re, im)
  lds_fft_stages(re, im, L, logL, tw);
  bf_store_peak(re, im, L >> 1, e, wbest, wbestp, w, part_m2, part_k);
}

// Any other win_size whose chirp convolution fits the LDS: Bluestein.  With w[n] = exp(-i pi n^2 / L),
//   X[k] = w[k] sum_n (x[n] w[n]) conj(w[k - n]),
// a convolution evaluated with two radix-2 FFTs of size M >= min(N, L) + L/2 + 1 (only the bins k <= L/2
// are needed, so M is about 1.5 L instead of 2 L): a = x w (zero-padded) -> FFT -> times B = FFT(conj(w),
// wrapped; built once per (L, N) on the host) -> inverse FFT.  |X[k]| = |c[k]|, the final chirp is skipped.
template <typename T>
__global__ __launch_bounds__(kBlockWide) void k_bf_chirp(const T* __restrict__ res, int N, int L, int M, int logM,
                                                         const double2* __restrict__ twm,
                                                         const double2* __restrict__ chirp,
                                                         const double2* __restrict__ bfft,
                                                         const int* __restrict__ status,
                                                         double* __restrict__ part_m2, int* __restrict__ part_k) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const BfSpectrumLds<T> lds = bf_spectrum_carve<T>(Carve(smem), 0, M);
  double *re = lds.re, *im = lds.im, *wbest = lds.wbest;
  int* wbestp = lds.wbestp;
  const int64_t w = blockIdx.x;
  if (status[w] != 0) return;
  const int M0 = N < L ? N : L;
  const T* xs = res + w * (int64_t)N;
  double xmax = 0.0;
  for (int n = threadIdx.x; n < M; n += blockDim.x) {
    const int r = (int)(__brev((unsigned)n) >> (32 - logM));
    double ar = 0.0, ai = 0.0;
    if (n < M0) {
      const double xv = (double)xs[n];
      xmax = fmax(xmax, fabs(xv));
      const double2 cs = chirp[n];  // (cos, sin)(pi n^2 / L); w[n] = cos - i sin
      ar = xv * cs.x;
      ai = -xv * cs.y;
    }
    re[r] = ar;
    im[r] = ai;
  }
  const int e = bf_scale_exp(xmax, wbest);  // (its barrier completes re, im)
  lds_fft_stages(re, im, M, logM, twm);
  // pointwise product with B, conjugated for the inverse transform (ifft(z) = conj(fft(conj(z))) / M), and
  // moved to bit-reversed order: element n and its mirror are handled by the thread that owns min(n, brev(n))
  for (int n = threadIdx.x; n < M; n += blockDim.x) {
    const int r = (int)(__brev((unsigned)n) >> (32 - logM));
    if (n > r) continue;
    const double2 b0 = bfft[n];
    const double p0r = re[n] * b0.x - im[n] * b0.y, p0i = re[n] * b0.y + im[n] * b0.x;
    if (r == n) {
      re[n] = p0r;
      im[n] = -p0i;
    } else {
      const double2 b1 = bfft[r];
      const double p1r = re[r] * b1.x - im[r] * b1.y, p1i = re[r] * b1.y + im[r] * b1.x;
      re[r] = p0r;
      im[r] = -p0i;
      re[n] = p1r;
      im[n] = -p1i;
    }
  }
  __syncthreads();
  lds_fft_stages(re, im, M, logM, twm);
  // c[k] = conj(result[k]) / M: the magnitudes only differ by the common factor 1 / M (kept out: the record is
  // only compared with the other bins of the same window)
  bf_store_peak(re, im, L >> 1, e, wbest, wbestp, w, part_m2, part_k);
}

template <typename T>
struct BfUpdateLds {
  T* work;
  T* buf;
  double* red;
  size_t bytes;
};
template <typename T, class C>
__host__ __device__ __forceinline__ BfUpdateLds<T> bf_update_carve(C cv, int N, bool lw, bool buf_lds) {
  BfUpdateLds<T> L;
  L.work = lw ? cv.template take<T>(N) : nullptr;
  L.buf = buf_lds ? cv.template take<T>(N) : nullptr;
  L.red = cv.template take<double>(kRedDoubles);
  L.bytes = cv.off;
  return L;
}

template <typename T, bool LW>
__global__ __launch_bounds__(kBlockWide) void k_bf_update(T* __restrict__ res, int N, int L, int num, int it,
                                                          unsigned flags, Tables tb, T* __restrict__ gbuf, int nchunk,
                                                          const double* __restrict__ part_m2,
                                                          const int* __restrict__ part_k, double* __restrict__ dnorm,
                                                          uint32_t* __restrict__ periods_out,
                                                          double* __restrict__ powers_out, T* __restrict__ bases_out,
                                                          int* __restrict__ status) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const BfUpdateLds<T> lds = bf_update_carve<T>(Carve(smem), N, LW, !gbuf);
  const int64_t w = blockIdx.x;
  // LW == false: the residual is projected where it lives (the HBM workspace `res`)
  T* work = LW ? lds.work : res + w * (int64_t)N;
  T* buf = second_buf(lds.buf, gbuf, N);
  double* red = lds.red;
  const int tid = threadIdx.x;
  T* brow = bases_out + (w * num + it) * (int64_t)N;
  bool dead = status[w] != 0;
  int p = 0;
  if (!dead) {
    double best = -1.0;
    int bestk = 0;
    for (int c = 0; c < nchunk; ++c) {  // chunks in ascending bin order: strict '>' keeps the first maximum
      const double v = part_m2[w * nchunk + c];
      const int kk = part_k[w * nchunk + c];
      if (kk != 0 && (bestk == 0 || v > best)) {
        best = v;
        bestk = kk;
      }
    }
    if (bestk <= 1) {  // bin 0 (or nothing comparable): 2 L / 0 in the reference
      dead = true;
      __syncthreads();  // every thread has read status[w]
      if (tid == 0) status[w] = 1;
    } else {
      p = (int)rint(2.0 * (double)L / (double)(bestk - 1));
    }
  }
  if (dead) {  // rows from the failing round on stay zero
    for (int n = tid; n < N; n += blockDim.x) brow[n] = T(0);
    if (tid == 0) {
      periods_out[w * num + it] = 0u;
      powers_out[w * num + it] = 0.0;
    }
    return;
  }
  if constexpr (LW) {
    load_window(res + w * (int64_t)N, work, N);
    __syncthreads();
  }
  double dn;
  if (it == 0) {
    dn = periodic_norm_from_sq(block_sumsq(work, N, red), N, 0);
    if (tid == 0) dnorm[w] = dn;
  } else {
    dn = dnorm[w];
  }
  project_lds(work, buf, N, p, flags, tb);
  const double nrm = periodic_norm_from_sq(block_sumsq(buf, N, red), N, 0);
  for (int n = tid; n < N; n += blockDim.x) {
    const T b = buf[n];
    brow[n] = b;
    res[w * (int64_t)N + n] = work[n] - b;
  }
  if (tid == 0) {
    periods_out[w * num + it] = (uint32_t)p;
    powers_out[w * num + it] = nrm / dn;
  }
}

}  // namespace ph

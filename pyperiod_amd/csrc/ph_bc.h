// Periods.best_correlation: one window per workgroup, and the window-pair screen.
#pragma once

#include "ph_device.h"
#include "ph_pair.h"

namespace ph {

// ======================================================================================
// Periods.best_correlation  (Periods.py:289-349).  One workgroup per window.
// ======================================================================================
constexpr int kCandCap = 256;  // screened candidates per sweep kept for exact evaluation

struct CandCtl {
  unsigned long long lbits;  // running lower bound on the best value (bits of a non-negative double)
  int ncand;
  int nsurv;
};

template <typename T>
struct BcLds {
  T* work;
  T* buf;
  double* red;
  double* wbest;
  int* wbestp;
  int* cand_q;
  double* cand_hi;
  CandCtl* ctl;
  size_t bytes;
};
template <typename T, class C>
__host__ __device__ __forceinline__ BcLds<T> bc_carve(C cv, int N, bool lw, bool buf_lds) {
  BcLds<T> L;
  L.work = lw ? cv.template take<T>(N + kPad) : nullptr;
  L.buf = buf_lds ? cv.template take<T>(N) : nullptr;
  L.red = cv.template take<double>(kRedDoubles);
  L.wbest = cv.template take<double>(kMaxWaves);
  L.wbestp = cv.template take<int>(kMaxWaves);
  L.cand_q = cv.template take<int>(kCandCap);
  L.cand_hi = cv.template take<double>(kCandCap);
  L.ctl = cv.template take<CandCtl>(1);
  L.bytes = cv.off;
  return L;
}

template <typename T, bool LW>
__global__ __launch_bounds__(kBlockWide) __attribute__((amdgpu_waves_per_eu(PH_STEP1_WAVES, 8))) void k_best_correlation(const T* __restrict__ x, int N, int num,
                                                             int max_length, double ratio, unsigned flags,
                                                             Tables tb, const PGeom* __restrict__ geom,
                                                             const PassPlan* __restrict__ plan, int n_pass,
                                                             T* __restrict__ gbuf, T* gwin,
                                                             uint32_t* __restrict__ periods_out,
                                                             double* __restrict__ norms_out,
                                                             T* __restrict__ bases_out,
                                                             int* __restrict__ status_out) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const bool general = flags & (kTrunc | kOrth);
  const BcLds<T> L = bc_carve<T>(Carve(smem), N, LW, general && !gbuf);
  T* work = window_buf<T, LW>(L.work, gwin, N + kPad);
  T* buf = !general ? nullptr : second_buf(L.buf, gbuf, N);
  double *red = L.red, *wbest = L.wbest, *cand_hi = L.cand_hi;
  int *wbestp = L.wbestp, *cand_q = L.cand_q;
  CandCtl* ctl = L.ctl;

  const int64_t w = blockIdx.x;
  const int tid = threadIdx.x;
  const int lane = tid & (kWave - 1);
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int nw = blockDim.x >> 6;
  T* bases = bases_out + w * (int64_t)num * N;
  load_window(x + w * (int64_t)N, work, N);
  zero_pad(work, N);
  __syncthreads();
  const double sqrtN = sqrt((double)N);
  const double og = sqrt(block_sumsq(work, N, red)) / sqrtN;  // :316
  double old_norm = og;
  int status = 0;

  for (int i = 0; i < num; ++i) {
    T* brow = bases + (int64_t)i * N;
    uint32_t keep_p = 0u;
    double keep_n = 0.0;
    bool zero_row = true;
    if (status == 0) {
      // argmax over (p, s) of |sum(x[s::p])|, strict '>' in p-major order (:324-331).
      // Screen: the multi-period passes of the pass plan give max_s |S_p[s]| for up to three periods
      // per fold, but from class sums, i.e. not in the reference's row order.  |S~ - S| <= R 2^-53
      // sum|x| bounds the difference, so every period whose screened value is within that radius
      // of the best is re-evaluated with the row-order pass and the exact values are compared.
      double asum = 0.0;
      for (int n = tid; n < N; n += blockDim.x) asum += fabs((double)work[n]);
      asum = block_sum(asum, red);
      if (tid == 0) {
        ctl->lbits = 0ull;
        ctl->ncand = 0;
        ctl->nsurv = 0;
      }
      __syncthreads();
      // A NaN or Inf sample leaves no bound to screen with: every period exactly, as after a list overflow.  The
      // reference's strict '>' passes over a NaN sum and takes the first infinite one (:329).
      const bool screen = asum <= 1.7976931348623157e308;
      if (screen) {
        const double radius = 4.0 * 1.1102230246251565e-16 * asum;  // 4 * 2^-53 * sum|x| per row
        double lrun = 0.0;
        wave_sweep_plan<T, LW, true>(work, N, geom, plan, wv, n_pass, nw, lane, [&](double v, int q) {
          const double e = radius * (double)(geom[q].rows + 4);
          const double hi = v + e, lo = v - e;
          lrun = fmax(lrun, __longlong_as_double((long long)*(volatile unsigned long long*)&ctl->lbits));
          if ((lane & 7) == 0 && hi > 0.0 && hi >= lrun) {
            const int idx = atomicAdd(&ctl->ncand, 1);
            if (idx < kCandCap) {
              cand_q[idx] = q;
              cand_hi[idx] = hi;
            }
          }
          if (lo > lrun) {
            lrun = lo;
            if ((lane & 7) == 0) atomicMax(&ctl->lbits, (unsigned long long)__double_as_longlong(lo));
          }
        });
      }
      __syncthreads();
      const int ncand = screen ? ctl->ncand : kCandCap + 1;
      double best = 0.0;
      int bestp = 0;
      auto exact = [&](int q) {  // row-order sums, bit-identical to the reference's sum(x[s::q])
        const double v = wave_max(wave_partial<T, true, LW>(work, N, q, geom[q], lane));
        if (v > best || (v == best && bestp != 0 && q < bestp)) {
          best = v;
          bestp = q;
        }
      };
      if (ncand <= kCandCap) {
        if (wv == 0) {  // survivors: upper bound reaches the final lower bound (compacted in place)
          const double lfin = __longlong_as_double((long long)ctl->lbits);
          int ns = 0;
          for (int b = 0; b < ncand; b += kWave) {
            const int k = b + lane;
            const bool keep = k < ncand && cand_hi[k] >= lfin;
            const int q = k < ncand ? cand_q[k] : 0;
            const unsigned long long m = __ballot(keep);
            const int pos = ns + __popcll(m & ((1ull << lane) - 1ull));
            if (keep) cand_q[pos] = q;
            ns += __popcll(m);
          }
          if (lane == 0) ctl->nsurv = ns;
        }
        __syncthreads();
        const int ns = ctl->nsurv;
        for (int k = wv; k < ns; k += nw) exact(cand_q[k]);
      } else {  // list overflow (many near-ties) or no screen: every period exactly
        for (int q = 2 + wv; q <= max_length - 1; q += nw) exact(q);
      }
      if (!(best > 0.0)) bestp = 0;
      if (lane == 0) {
        wbest[wv] = best;
        wbestp[wv] = bestp;
      }
      __syncthreads();
      red_argmax(wbest, wbestp, nw, best, bestp);
      __syncthreads();
      if (bestp == 0) {
        status = 1;  // reference: project(data, None) raises
      } else {
        // project, subtract unconditionally (:334-340)
        if (!general) {
          const Fold f(N, bestp);
          for (int j = tid; j < bestp; j += blockDim.x) {
            const T m = residue_mean(work, f, j, false);
            const int cnt = f.count(j);
            for (int r = 0; r < cnt; ++r) {
              const int n = r * bestp + j;
              brow[n] = m;
              work[n] -= m;
            }
          }
        } else {
          project_lds(work, buf, N, bestp, flags, tb);
          for (int n = tid; n < N; n += blockDim.x) {
            const T m = buf[n];
            brow[n] = m;
            work[n] -= m;
          }
        }
        __syncthreads();
        const double this_norm = sqrt(block_sumsq(work, N, red)) / sqrtN;
        const double gain = (old_norm - this_norm) / og;
        if (gain > ratio) {  // :343
          keep_p = (uint32_t)bestp;
          keep_n = gain;
          old_norm = this_norm;
          zero_row = false;
        }
      }
    }
    if (zero_row)
      for (int n = tid; n < N; n += blockDim.x) brow[n] = T(0);
    if (tid == 0) {
      periods_out[w * num + i] = keep_p;
      norms_out[w * num + i] = keep_n;
    }
  }
  if (tid == 0) status_out[w] = status;
}

// ======================================================================================
// Periods.best_correlation, window-pair screen (plain projection, fp64 windows that fit the LDS twice).
//   Same layout as k_mbest_step1_pair: two windows per workgroup, pair window + one fp64 staging buffer in LDS, fp64
//   residuals in the HBM workspace.  Per outer iteration (Periods.py:320-347) the multi-period passes run over the
//   float images with "largest square" in place of "sum of squares" (max_s |S_p[s]|, :327-331); |sqrt(screen) - max|S||
//   <= 1.25 (R + 2) 2^-24 sum|r| (any summation order of R float-rounded terms), so the periods whose upper bound
//   reaches the best lower bound contain the exact argmax; they are re-evaluated with the row-order fp64 pass of
//   k_best_correlation and compared exactly as there (strict '>', lowest period among equals).  Both windows of a pair
//   always run the same number of iterations, so they never fall out of step.
// ======================================================================================
// control words and state of k_best_correlation_pair in LDS; window w of the pair has word NAME + w
enum { BP_LISTED = 0 /* survivors listed */, BP_STATUS = 2, BP_EXISTS = 4, BP_QUEUE = 6 /* pass queue of the screen (one word) */, BP_WORDS = 8 };
enum {
  BP_ABSSUM = 0,  // sum |r| of the scaled residual
  BP_SCALE = 2,
  BP_OG = 4,        // og and old_norm of Periods.py:316-317
  BP_OLD_NORM = 6,
  BP_USABLE = 8,    // 1 / 0: the float image can be screened
  BP_DOUBLES = 10
};

struct BcPairLds {
  f2* pw;
  double* stg;
  double* red;
  double* wbest;
  int* wbestp;
  int* list;
  int* ctl;
  double* st;
  size_t bytes;
};
template <class C>
__host__ __device__ __forceinline__ BcPairLds bc_pair_carve(C cv, int N) {
  BcPairLds L;
  L.pw = cv.template take<f2>(N + kPad);
  L.stg = cv.template take<double>(N + kPad);
  L.red = cv.template take<double>(kRedDoubles);
  L.wbest = cv.template take<double>(kMaxWaves);
  L.wbestp = cv.template take<int>(kMaxWaves);
  L.list = cv.template take<int>(2 * kPairListCap);
  L.ctl = cv.template take<int>(BP_WORDS);
  L.st = cv.template take<double>(BP_DOUBLES);
  L.bytes = cv.off;
  return L;
}

__global__ __launch_bounds__(1024) __attribute__((amdgpu_waves_per_eu(PH_STEP1_WAVES, 8))) void k_best_correlation_pair(
    const double* __restrict__ x, int W, int N, int num, int max_length, double ratio, const PGeom* __restrict__ geom,
    const PGeomF* __restrict__ geomf, const PassPlan* __restrict__ plan, int n_pass, double* __restrict__ gres,
    uint32_t* __restrict__ periods_out, double* __restrict__ norms_out, double* __restrict__ bases_out,
    int* __restrict__ status_out) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const BcPairLds L = bc_pair_carve(Carve(smem), N);
  f2* pw = L.pw;
  double *stg = L.stg, *red = L.red, *wbest = L.wbest, *st = L.st;
  int *wbestp = L.wbestp, *list = L.list, *ctl = L.ctl;

  const int tid = threadIdx.x;
  const int lane = tid & (kWave - 1);
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  constexpr int NW = kPairWaves, nw = NW;  // always 64 kPairWaves threads (plan_best_correlation): see k_mbest_step1_pair
  const size_t gstride = win_stride((size_t)N);
  float* pwf = reinterpret_cast<float*>(pw);
  const double sqrtN = uniform_f64(sqrt((double)N));
  const int p_lo = 2, p_hi = max_length - 1, P = p_hi - p_lo + 1;

  zero_pad(stg, N);
  for (int i = tid; i < kPad; i += blockDim.x) pw[N + i] = f2_zero();
  for (int w = 0; w < 2; ++w) {
    const int64_t gw = 2 * (int64_t)blockIdx.x + w;
    const bool exists = gw < W;
    __syncthreads();
    if (exists) {
      load_window(x + gw * (int64_t)N, stg, N);
    } else {
      for (int n = tid; n < N; n += blockDim.x) stg[n] = 0.0;
    }
    __syncthreads();
    double a2 = 0.0, a1 = 0.0;
    for (int n = tid; n < N; n += blockDim.x) {
      const double v = stg[n];
      a2 = fma(v, v, a2);
      a1 += fabs(v);
    }
    block_sum2<NW>(a2, a1, red);
    const double sc = uniform_f64(pair_pick_scale(a2, N));
    for (int n = tid; n < N; n += blockDim.x) pwf[2 * n + w] = (float)(stg[n] * sc);
    if (tid == 0) {
      st[BP_ABSSUM + w] = a1 * sc * (1.0 + 1e-9);
      st[BP_SCALE + w] = sc;
      st[BP_OG + w] = st[BP_OLD_NORM + w] = sqrt(a2) / sqrtN;
      st[BP_USABLE + w] = pair_usable(a2) ? 1.0 : 0.0;
      ctl[BP_STATUS + w] = 0;
      ctl[BP_EXISTS + w] = exists ? 1 : 0;
      ctl[BP_QUEUE] = nw;
    }
  }
  __syncthreads();

  for (int it = 0; it < num; ++it) {
    const bool run0 = ctl[BP_EXISTS] && ctl[BP_STATUS] == 0, run1 = ctl[BP_EXISTS + 1] && ctl[BP_STATUS + 1] == 0;
    __syncthreads();
    if (tid == 0) ctl[BP_LISTED] = ctl[BP_LISTED + 1] = 0;
    prio_by_progress(it);
    if ((run0 || run1) && P > 0) {
      // ---- screen: largest square of a residue sum per period, both windows (Periods.py:324-331 in float)
      f2* vals = reinterpret_cast<f2*>(stg);
      pair_sweep_plan<true>(
          pw, N, geomf, plan, wv, n_pass, nw, [&](float z, int q) { pair_store1(vals, z, q, p_lo); },
          [&](float z, int q_a, int q_b) { pair_store2(vals, z, q_a, q_b, p_lo); },
          PH_PAIR_QUEUE ? &ctl[BP_QUEUE] : nullptr);
      prio_short_phase();
      __syncthreads();
      if (tid == 0) ctl[BP_QUEUE] = nw;  // for the next screen (barriers in between)
      const bool scr0 = run0 && st[BP_USABLE] != 0.0, scr1 = run1 && st[BP_USABLE + 1] != 0.0;
      if (scr0 || scr1) {
        const double u0 = 1.25 * 5.9604644775390625e-08 * st[BP_ABSSUM], u1 = 1.25 * 5.9604644775390625e-08 * st[BP_ABSSUM + 1];
        const float fn = (float)N;
        double lo0 = -1.0 / 0.0, lo1 = -1.0 / 0.0;
        for (int idx = tid; idx < P; idx += blockDim.x) {
          const f2 v = vals[idx];
          const double rr = (double)(pair_rows_upper(fn, p_lo + idx) + 2);
          lo0 = fmax(lo0, sqrt((double)v.x) - rr * u0);
          lo1 = fmax(lo1, sqrt((double)v.y) - rr * u1);
        }
        lo0 = wave_max(lo0);
        lo1 = wave_max(lo1);
        if (lane == 0) {
          red[wv] = lo0;
          red[kMaxWaves + wv] = lo1;
        }
        __syncthreads();
        lo0 = red_combine<true, NW>(red, nw);  // (fmax in slot order: the value of the loop this replaces)
        lo1 = red_combine<true, NW>(red + kMaxWaves, nw);
        for (int idx = tid; idx < P; idx += blockDim.x) {
          const f2 v = vals[idx];
          const double rr = (double)(pair_rows_upper(fn, p_lo + idx) + 2);
          const double h0 = sqrt((double)v.x) + rr * u0, h1 = sqrt((double)v.y) + rr * u1;
          if (scr0 && h0 > 0.0 && h0 >= lo0) {
            const int k = atomicAdd(&ctl[BP_LISTED], 1);
            if (k < kPairListCap) list[k] = p_lo + idx;
          }
          if (scr1 && h1 > 0.0 && h1 >= lo1) {
            const int k = atomicAdd(&ctl[BP_LISTED + 1], 1);
            if (k < kPairListCap) list[kPairListCap + k] = p_lo + idx;
          }
        }
      }
    }
    __syncthreads();
    for (int w = 0; w < 2; ++w) {
      const int64_t gw = 2 * (int64_t)blockIdx.x + w;
      if (!ctl[BP_EXISTS + w]) continue;
      double* brow = bases_out + (gw * num + it) * (int64_t)N;
      int status = ctl[BP_STATUS + w];
      uint32_t keep_p = 0u;
      double keep_n = 0.0;
      bool zero_row = true;
      const double og = st[BP_OG + w], old_norm = st[BP_OLD_NORM + w], sc = st[BP_SCALE + w];
      const bool exact_all = st[BP_USABLE + w] == 0.0 || ctl[BP_LISTED + w] > kPairListCap;
      const int ncand = exact_all ? P : ctl[BP_LISTED + w];
      __syncthreads();
      if (status == 0) {
        const double* src = it == 0 ? x + gw * (int64_t)N : gres + gw * gstride;
        load_window(src, stg, N);
        __syncthreads();
        double best = 0.0;
        int bestp = 0;
        for (int k = wv; k < ncand; k += nw) {  // row-order sums, bit-identical to the reference's sum(x[s::q])
          const int q = exact_all ? p_lo + k : list[w * kPairListCap + k];
          const double v = wave_max(wave_partial<double, true, true>(stg, N, q, geom[q], lane));
          if (v > best || (v == best && bestp != 0 && q < bestp)) {
            best = v;
            bestp = q;
          }
        }
        if (!(best > 0.0)) bestp = 0;
        if (lane == 0) {
          wbest[wv] = best;
          wbestp[wv] = bestp;
        }
        __syncthreads();
        red_argmax<NW>(wbest, wbestp, nw, best, bestp);
        __syncthreads();
        if (bestp == 0) {
          status = 1;  // reference: project(data, None) raises
        } else {
          // project, subtract unconditionally (:334-340); the new residual goes to the workspace and, as floats, into pw
          double* dst = gres + gw * gstride;
          double a2 = 0.0, a1 = 0.0;
          const Fold f(N, bestp);
          for (int j = tid; j < bestp; j += blockDim.x) {
            const double m = residue_mean(stg, f, j, false);
            const int cnt = f.count(j);
            for (int r = 0; r < cnt; ++r) {
              const int n = r * bestp + j;
              const double v = stg[n] - m;
              brow[n] = m;
              dst[n] = v;
              pwf[2 * n + w] = (float)(v * sc);
              a2 = fma(v, v, a2);
              a1 += fabs(v);
            }
          }
          block_sum2<NW>(a2, a1, red);
          const double this_norm = sqrt(a2) / sqrtN;
          const double gain = (old_norm - this_norm) / og;
          zero_row = !(gain > ratio);  // :343
          if (!zero_row) {
            keep_p = (uint32_t)bestp;
            keep_n = gain;
          }
          double sc2 = sc;
          const bool ok = pair_usable(a2);
          if (pair_image_stale(a2, sc, N)) {
            sc2 = uniform_f64(pair_pick_scale(a2, N));
            __syncthreads();
            pair_rescale(pwf, w, N, (float)(sc2 / sc), tid);
          }
          if (tid == 0) {
            st[BP_ABSSUM + w] = a1 * sc2 * (1.0 + 1e-9);
            st[BP_SCALE + w] = sc2;
            if (!zero_row) st[BP_OLD_NORM + w] = this_norm;
            st[BP_USABLE + w] = ok ? 1.0 : 0.0;
          }
        }
      }
      if (zero_row) {
        __syncthreads();  // (brow may hold this round's projection)
        for (int n = tid; n < N; n += blockDim.x) brow[n] = 0.0;
      }
      if (tid == 0) {
        periods_out[gw * num + it] = keep_p;
        norms_out[gw * num + it] = keep_n;
        ctl[BP_STATUS + w] = status;
      }
      __syncthreads();
    }
  }
  __syncthreads();
  if (tid < 2) {
    const int64_t gw = 2 * (int64_t)blockIdx.x + tid;
    if (gw < W) status_out[gw] = ctl[BP_STATUS + tid];
  }
}

}  // namespace ph

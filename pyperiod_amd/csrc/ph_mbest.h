// Periods.m_best: step 1 (one window per workgroup, and the window-pair screen) and step 2.
#pragma once

#include "ph_device.h"
#include "ph_pair.h"

namespace ph {

// ======================================================================================
// m_best step 1  (Periods.py:494-537): repeat { all-p sweep, argmax, subtract } until `num`
// distinct periods are found.  One workgroup per window, one launch per window batch.
// ======================================================================================
// skip bits of step 1: bit i = period p_lo + i has been chosen ten times over and is left out of the sweeps
__device__ __forceinline__ bool skip_test(const uint32_t* skip, int i) { return (skip[i >> 5] >> (i & 31)) & 1u; }
__device__ __forceinline__ void skip_set(uint32_t* skip, int i) { skip[i >> 5] |= 1u << (i & 31); }

// Does (ss, p) beat the best candidate so far (best_ss, bestp; bestp == 0: none yet)?  The reference compares the
// rounded norms sqrt(ss)/sqrt(N)[/sqrt(p)] and keeps the lowest period among equal ones (Periods.py:512); the norm is
// monotone in ss (ss / p in gamma mode), so the sums of squares are compared directly and the square roots and
// divisions -- norm(ss, divisor), the caller's form of periodic_norm_from_sq -- are evaluated only when two candidates
// are within rounding distance of each other.
template <typename Norm>
__device__ __forceinline__ bool mbest_prefers(double ss, int p, double best_ss, int bestp, int gamma, Norm&& norm) {
  bool take = bestp == 0;
  if (!take) {
    const double lhs = gamma ? ss * (double)bestp : ss;
    const double rhs = gamma ? best_ss * (double)p : best_ss;
    if (lhs > rhs * (1.0 + 1e-14)) {
      take = true;
    } else if (lhs >= rhs * (1.0 - 1e-14)) {
      const double vn = norm(ss, gamma ? p : 0);
      const double vb = norm(best_ss, gamma ? bestp : 0);
      take = vn > vb || (vn == vb && p < bestp);
    }
  }
  return take;
}

// Bookkeeping of a sweep's winner (Periods.py:518-535), identical in every thread; thread 0 writes the LDS tables.
// `best` is read by thread 0 alone: k_mbest_step1_pair hands over the norm in wavefront 0 only on its fold-once path.
// `row` is the row that holds bestp already, or -1.  Returns the action -- 0 = subtract only, 1 = store new row,
// 2 = accumulate into existing row -- and leaves the row it applies to in `row`.  Ten repeats are accumulated; the
// next one sets the period's skip bit instead.
__device__ __forceinline__ int mbest_book(int& row, int bestp, double best, int p_lo, int tid, int& filled, int& repeats,
                                          double* norms, uint32_t* periods, uint32_t* skip) {
  int action;
  __syncthreads();  // every thread has looked for the row
  if (row >= 0 && repeats < 10) {
    action = 2;
    if (tid == 0) norms[row] += best;
    repeats += 1;
  } else if (row >= 0) {
    action = 0;
    if (tid == 0) skip_set(skip, bestp - p_lo);
    repeats = 0;
  } else {
    action = 1;
    row = filled;
    if (tid == 0) {
      periods[row] = (uint32_t)bestp;
      norms[row] = best;
    }
    filled += 1;
    repeats = 0;
  }
  return action;
}

// LDS bytes of k_mbest_step1 for the host.  The kernel spells its takes out itself (see there) and this is their count,
// kept in step by hand: a piece added to one is added to the other.
template <typename T>
__host__ __device__ inline size_t step1_lds_bytes(int N, int num, int P, bool lw, bool buf_lds, bool small_means) {
  CarveCount cv;
  if (lw) cv.take<T>(N + kPad);         // work
  if (buf_lds) cv.take<T>(N);           // buf
  cv.take<double>(kRedDoubles);         // red
  cv.take<double>(kMaxWaves);           // wbest
  cv.take<int>(kMaxWaves);              // wbestp
  cv.take<double>(num);                 // norms
  cv.take<uint32_t>(num);               // periods
  cv.take<uint32_t>((P + 31) / 32);     // skip
  if (small_means) {
    cv.take<T>(kPairSmallP);            // msm
    cv.take<T>(kPairSplitW);            // prt
  }
  return cv.off;
}

template <typename T, bool LW>
__global__ __launch_bounds__(1024) __attribute__((amdgpu_waves_per_eu(PH_STEP1_WAVES, 8))) void k_mbest_step1(const T* __restrict__ x, int N, int num, int p_lo,
                                                        int p_hi, int gamma, unsigned flags, Tables tb,
                                                        const PGeom* __restrict__ geom,
                                                        const PassPlan* __restrict__ plan, int n_pass,
                                                        T* __restrict__ gbuf, T* gwin,
                                                        int max_iters, uint32_t* __restrict__ periods_out,
                                                        double* __restrict__ norms_out, T* __restrict__ rows_out,
                                                        int row_stride, double* __restrict__ dnorm_out,
                                                        int* __restrict__ status_out,
                                                        int* __restrict__ sweeps_out, int small_means) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  // The takes are spelled out here, not run through a carve function as in the other kernels: with one, this kernel
  // measured 1 % (long windows) to 5 % (trunc) slower (profiles/lds_layout).  The host counts them in step1_lds_bytes.
  Carve cv(smem);
  T* work = window_buf<T, LW>(LW ? cv.take<T>(N + kPad) : nullptr, gwin, N + kPad);
  const bool general = flags & (kTrunc | kOrth);
  T* buf = !general ? nullptr : gbuf ? gbuf + (int64_t)blockIdx.x * N : cv.take<T>(N);
  double* red = cv.take<double>(kRedDoubles);
  double* wbest = cv.take<double>(kMaxWaves);
  int* wbestp = cv.take<int>(kMaxWaves);
  double* norms = cv.take<double>(num);
  uint32_t* periods = cv.take<uint32_t>(num);
  const int P = p_hi - p_lo + 1;
  uint32_t* skip = cv.take<uint32_t>((P + 31) / 32);
  // means / partial sums of a short winning period (split_row_means); absent when the LDS has no room for them
  T* msm = small_means ? cv.take<T>(kPairSmallP) : nullptr;
  T* prt = small_means ? cv.take<T>(kPairSplitW) : nullptr;

  const int64_t w = blockIdx.x;
  const int tid = threadIdx.x;
  const int lane = tid & (kWave - 1);
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int nw = blockDim.x >> 6;
  // Basis rows leave step 1 in COMPACT form: row k of the window is the mean vector of its period (the first
  // p elements of the tiled projection; the projection is p-periodic in every flag mode), row_stride elements
  // apart.  Step 2 refines them and writes the (num, N) matrix once, in final order.
  T* rows = rows_out + w * (int64_t)num * row_stride;

  load_window(x + w * (int64_t)N, work, N);
  zero_pad(work, N);
  for (int k = tid; k < num; k += blockDim.x) {
    norms[k] = 0.0;
    periods[k] = 0u;
  }
  for (int k = tid; k < (P + 31) / 32; k += blockDim.x) skip[k] = 0u;
  __syncthreads();
  const double data_norm = uniform_f64(periodic_norm_from_sq(block_sumsq(work, N, red), N, 0));

  int filled = 0;   // `i` of Periods.py:494
  int repeats = 0;  // `iters`
  int status = 0;
  int iters = 0;
  while (filled < num) {
    if (++iters > max_iters) {
      status = 2;
      break;
    }
    // ---- sweep (Periods.py:501-515): strict '>' keeps the lowest p among equal norms
    double best = 0.0;
    int bestp = 0;
    if (!general) {
      // Periods arrive out of order from the pass plan: sums of squares are compared, the rounded norm of the winner
      // is taken once per lane at the end.  The comparison is mbest_prefers, written out: as a call it costs this
      // kernel scalar spills (2 more at fp64, 8 bytes of scratch at fp32 / HBM windows).
      double best_ss = 0.0;
      wave_sweep_plan<T, LW>(work, N, geom, plan, wv, n_pass, nw, lane, [&](double ss, int p) {
        if (skip_test(skip, p - p_lo) || !(ss > 0.0)) return;
        bool take = bestp == 0;
        if (!take) {
          const double lhs = gamma ? ss * (double)bestp : ss;
          const double rhs = gamma ? best_ss * (double)p : best_ss;
          if (lhs > rhs * (1.0 + 1e-14)) {
            take = true;
          } else if (lhs >= rhs * (1.0 - 1e-14)) {
            const double vn = periodic_norm_from_sq(ss, N, gamma ? p : 0);
            const double vb = periodic_norm_from_sq(best_ss, N, gamma ? bestp : 0);
            take = vn > vb || (vn == vb && p < bestp);
          }
        }
        if (take) {
          best_ss = ss;
          bestp = p;
        }
      });
      best = bestp != 0 ? periodic_norm_from_sq(best_ss, N, gamma ? bestp : 0) : 0.0;
      if (!(best > 0.0)) bestp = 0;  // the reference needs p_norm > 0 (Periods.py:497,512)
      wave_argmax(best, bestp);
      if (lane == 0) {
        wbest[wv] = best;
        wbestp[wv] = bestp;
      }
      __syncthreads();
      red_argmax(wbest, wbestp, nw, best, bestp);
      __syncthreads();
    } else {
      for (int p = p_lo; p <= p_hi; ++p) {
        const double v = block_sweep_value(work, buf, N, p, gamma ? p : 0, flags, tb, red);
        if (v > best && !skip_test(skip, p - p_lo)) {
          best = v;
          bestp = p;
        }
      }
    }
    if (bestp == 0) {  // reference: max_base is None -> TypeError at Periods.py:520/537
      status = 1;
      break;
    }
    // ---- bookkeeping: mbest_book, written out (as a call it costs the fp64 / HBM-window form a scalar spill)
    int row = -1;
    for (int k = 0; k < num; ++k)
      if (periods[k] == (uint32_t)bestp) row = k;
    int action;
    __syncthreads();
    if (row >= 0 && repeats < 10) {
      action = 2;
      if (tid == 0) norms[row] += best;
      repeats += 1;
    } else if (row >= 0) {
      action = 0;
      if (tid == 0) skip_set(skip, bestp - p_lo);
      repeats = 0;
    } else {
      action = 1;
      row = filled;
      if (tid == 0) {
        periods[row] = (uint32_t)bestp;
        norms[row] = best;
      }
      filled += 1;
      repeats = 0;
    }
    // ---- project the winner, update bases row, subtract from the residual (:531-537)
    T* brow = rows + (int64_t)(row < 0 ? 0 : row) * row_stride;
    if (!general && msm && bestp <= kPairSmallP) {
      // a short period: its few residues have hundreds of rows each -- means through LDS (split_row_means, as
      // k_mbest_step1_pair), the subtraction is spread over the workgroup
      split_row_means(work, msm, prt, N, bestp, tid, min((int)blockDim.x, kPairSplitW));
      if (tid < bestp) {
        const T m = msm[tid];
        if (action == 1)
          brow[tid] = m;
        else if (action == 2)
          brow[tid] += m;
      }
      int idx = tid % bestp;
      const int step = blockDim.x % bestp;
      for (int n = tid; n < N; n += blockDim.x) {
        work[n] -= msm[idx];
        idx += step;
        idx = idx >= bestp ? idx - bestp : idx;
      }
    } else if (!general) {
      const Fold f(N, bestp);
      for (int j = tid; j < bestp; j += blockDim.x) {
        const T m = residue_mean(work, f, j, false);
        const int cnt = f.count(j);
        if (action == 1)
          brow[j] = m;
        else if (action == 2)
          brow[j] += m;  // every element of the tiled row would get the same sum (Periods.py:519)
        for (int r = 0; r < cnt; ++r) work[r * bestp + j] -= m;
      }
    } else {
      project_lds(work, buf, N, bestp, flags, tb);
      for (int n = tid; n < N; n += blockDim.x) {
        const T m = buf[n];
        if (n < bestp) {
          if (action == 1)
            brow[n] = m;
          else if (action == 2)
            brow[n] += m;
        }
        work[n] -= m;
      }
    }
    __syncthreads();
  }
  __syncthreads();
  // rows the algorithm never filled keep period 0: step 2 writes them as zeros (np.zeros((num, N)), Periods.py:490)
  for (int k = tid; k < num; k += blockDim.x) {
    periods_out[w * num + k] = periods[k];
    norms_out[w * num + k] = norms[k];
  }
  if (tid == 0) {
    dnorm_out[w] = data_norm;
    status_out[w] = status;
    if (sweeps_out) sweeps_out[w] = status == 2 ? iters - 1 : iters;  // all-p sweeps performed
  }
}

// ======================================================================================
// m_best step 1, window-pair screen (plain projection, fp64 windows that fit the LDS twice).
//   One workgroup owns TWO windows.  LDS holds the pair window pw (element n = {fl32(a[n] sa), fl32(b[n] sb)},
//   ph_pair.h) and ONE fp64 staging buffer; the fp64 residuals live in an HBM workspace (gres; the input itself
//   before the first subtraction).  An iteration of Periods.py:496-537 is
//     1. screen: the pass plan over pw -- every ds_read_b64 / v_pk_add_f32 / address instruction serves both
//        windows; the 1364 x 2 float values land in the (idle) staging buffer;
//     2. per window: best lower bound L = max_q (v_q - rad_q), survivors { q : v_q + rad_q >= L } (pair_radius is a
//        rigorous bound on |screen - exact|, so the exact argmax -- and every period that ties with it in the
//        rounded norm -- is among them; ~1 survivor per sweep);
//     3. per window: residual -> staging, survivors re-evaluated in fp64 and compared exactly as k_mbest_step1
//        does (lazy rounded norms, lowest period among equals), bookkeeping, row-order projection of the winner,
//        and ONE fused pass that subtracts, sums the squares of the new residual, writes it back to the
//        workspace and writes its float image into pw.
//   A window that is not finite / all zero, or whose survivor list overflows, takes every period through the
//   exact evaluation instead (same decisions as k_mbest_step1, slower).
//   Cover rule (plain m_best, p_scr > p_lo): the plan holds only the periods [p_scr, p_hi], p_scr = p_hi / 2 + 1, each
//   of which bounds its divisors (E_d <= E_m for d | m, ph_pair.h).  Step 2 scans those, and every period m whose
//   upper bound (+ pair_cover_slack) reaches L -- skipped or not -- puts itself (unless skipped) and its unskipped
//   proper divisors >= p_lo (fac_off / fac_q, and 1) on the list; step 3 first thins the list with one fp64 value
//   per candidate, a wavefront each, to those within 1e-9 of the largest.  p_scr == p_lo: no cover logic, every
//   period is screened (m_best_gamma, whose E_q / q the rule does not order, and PH_PAIR_COVER=0).
// ======================================================================================
constexpr int kPairCoop = 6;  // up to this many survivors are evaluated by the whole workgroup, one after the other

// control words of k_mbest_step1_pair in LDS; window w of the pair has word NAME + w
enum {
  MP_LISTED = 0,      // survivors listed
  MP_FILLED = 2,      // rows filled (`i` of Periods.py:494)
  MP_REPEATS = 4,     // `iters` of Periods.py:494
  MP_STATUS = 6,      // status in the low byte; above it the window-sweeps that took the fold-once path
  MP_SWEEPS = 8,      // sweeps done
  MP_RUNNING = 10,    // still running
  MP_EXACT_ALL = 12,  // every period goes through the exact evaluation
  MP_QUEUE = 14,      // pass queue of the screen (one word)
  MP_WORDS = 16
};
enum { MP_UNIT = 0, MP_SCALE = 2, MP_DOUBLES = 4 };  // sum of squares of the scaled residual (unit of the radius); its scale

// block_sum<NW> with the combine done once: every wavefront adding the same NW partial sums is NW loads and NW additions in
// each of them for one value.  Wavefront 0 adds them -- the same additions in the same order -- between the two barriers
// block_sum has anyway, and the others read the total behind the second.  The total lies in red[kMaxWaves], a slot no block
// sum writes its partial values to; it is written again only behind the first barrier of a later call, which no wavefront
// reaches before it has the value.  What a caller must keep (as block_sum_once has its own condition, ph_device.h): red holds
// more than kMaxWaves doubles (kRedDoubles = 2 kMaxWaves), and a barrier lies between the read of the total here and anything
// else that writes the upper half of red -- block_sum2, the survivor scan's second maximum.  In k_mbest_step1_pair every such
// write is a phase and at least one barrier away.
template <int NW>
__device__ __forceinline__ double block_sum_lead(double v, double* red, int wv, int lane) {
  static_assert(kRedDoubles > kMaxWaves, "the total lies behind the partial sums");
  double* total = red + kMaxWaves;
  v = wave_sum(v);
  if (lane == 0) red[wv] = v;
  __syncthreads();
  if (wv == 0) {
    const double t = red_combine<false, NW>(red, NW);
    if (lane == 0) *total = t;
  }
  __syncthreads();
  return uniform_f64(*total);
}

// sum_j S_p[j]^2 / cnt_p[j] of the fp64 window `xs` (LDS), residues j = first, first + stride, ... (p >= 64 path)
__device__ __forceinline__ double pair_exact_part(const double* __restrict__ xs, int p, const PGeom& g, int first, int stride) {
  double part = 0.0;
  for (int j = first; j < p; j += stride) {
    const bool full = j < g.nfull;
    const double s = column_sum(xs, j, p, full ? g.rows : g.rows - 1);
    part = fma(s * s, full ? g.w_full : g.w_short, part);
  }
  return part;
}

// LDS of k_mbest_step1_pair: the pair window, one fp64 staging buffer, bookkeeping of two windows.
struct Step1PairLds {
  f2* pw;
  double* stg;
  double* red;
  double* wbest;
  int* wbestp;
  double* norms;
  uint32_t* periods;
  uint32_t* skip;
  int* list;
  int* ctl;
  double* dst2;
  double* msm;  // means of a short winning period
  double* prt;  // partial sums of split_row_means
  size_t bytes;
};
template <class C>
__host__ __device__ __forceinline__ Step1PairLds step1_pair_carve(C cv, int N, int num, int P) {
  Step1PairLds L;
  // (the control words first: their addresses -- the pass queue's among them, which every pass of the screen takes a
  // ticket from -- are constants of the instruction, not values derived from the shape and kept in registers)
  L.ctl = cv.template take<int>(MP_WORDS);
  L.dst2 = cv.template take<double>(MP_DOUBLES);
  L.pw = cv.template take<f2>(N + kPad);
  L.stg = cv.template take<double>(N + kPad);
  L.red = cv.template take<double>(kRedDoubles);
  L.wbest = cv.template take<double>(kMaxWaves);
  L.wbestp = cv.template take<int>(kMaxWaves);
  L.norms = cv.template take<double>(2 * num);
  L.periods = cv.template take<uint32_t>(2 * num);
  L.skip = cv.template take<uint32_t>(2 * ((P + 31) / 32));
  L.list = cv.template take<int>(2 * kPairListCap);
  L.msm = cv.template take<double>(kPairSmallP);
  L.prt = cv.template take<double>(kPairSplitW);
  L.bytes = cv.off;
  return L;
}

// The arguments of k_mbest_step1_pair: one block passed by value, i.e. the kernarg segment itself.  The kernel sits at
// its scalar-register budget, and 26 arguments loaded in the entry block were parked in lanes of vector registers
// (v_writelane) and brought back by v_readlane at every use, four of them in front of every pass of the screen.  Only
// what a pass needs stays in scalar registers across the screen -- N, p_lo, plan, geomf, n_pass --; everything else is
// fetched from the block by a scalar load at the head of the phase that uses it (pair_args_at_use), which costs no
// vector instruction.
struct Step1PairArgs {
  const double* x;
  int W, N, num, p_lo, p_hi, p_scr, gamma;
  int n_pass;
  const int* fac_off;
  const int* fac_q;
  const PGeom* geom;
  const PGeomF* geomf;
  const double* radq;
  const PassPlan* plan;
  double* gres;
  uint32_t* periods_out;
  double* norms_out;
  double* rows_out;
  double* dnorm_out;
  int* status_out;
  int* sweeps_out;
  // thin_band: pair_thin_band(N) from the host (computed here it is a loop invariant in vector registers, spilled around the
  // screen), or a negative number: no fold-once path (PH_PAIR_FOLD_ONCE=0)
  double thin_band;
  int max_iters, row_stride, fold_report;
};
typedef const __attribute__((address_space(4))) Step1PairArgs* step1_pair_args_ptr;

// The block for the phase that begins here: its address through a scalar register pair, the way const_at_use passes a
// constant, so that the loads of the fields stay behind this point (loads from the kernarg segment are invariant and
// would otherwise all move to the kernel's entry block).
__device__ __forceinline__ step1_pair_args_ptr pair_args_at_use() {
  step1_pair_args_ptr p = (step1_pair_args_ptr)__builtin_amdgcn_kernarg_segment_ptr();
  asm volatile("" : "+s"(p));
  return p;
}
// the kernel's LDS layout from the block (scalar arithmetic; a phase computes the pieces it uses)
__device__ __forceinline__ Step1PairLds pair_lds_at_use(step1_pair_args_ptr A, unsigned char* smem) {
  return step1_pair_carve(Carve(smem), A->N, A->num, A->p_hi - A->p_lo + 1);
}
// a pointer fetched that way, known to point to global memory (a pointer loaded from memory is a flat one to the compiler)
template <typename T>
__device__ __forceinline__ T* pair_arg_global(T* p) {
  return (T*)(__attribute__((address_space(1))) T*)p;
}
// ... and a table the kernel only reads (ConstTable, ph_device.h)
template <typename T>
__device__ __forceinline__ ConstTable<T> pair_arg_table(const T* p) {
  return ConstTable<T>(p);
}

__global__ __launch_bounds__(1024) __attribute__((amdgpu_waves_per_eu(PH_STEP1_WAVES, 8))) void k_mbest_step1_pair(const Step1PairArgs) {
  // (the block is read through the segment pointer only: named and read as a parameter, it was copied to scratch)
  const step1_pair_args_ptr a = (step1_pair_args_ptr)__builtin_amdgcn_kernarg_segment_ptr();
  // What the screen works with, in scalar registers for the whole kernel: the scr_ names.  Only the round loop's head, the
  // screen and the debug prints use them.  Every phase behind the screen declares its own N, p_lo, stg, ctl, wv, ... from
  // the block (below): a phase that read a scr_ value instead would make the compiler keep what it derives from it across
  // the passes again -- in lanes.
  const int scr_N = a->N, scr_p_lo = a->p_lo, scr_n_pass = a->n_pass;
  const ConstTable<PGeomF> scr_geomf = pair_arg_table(a->geomf);
  const ConstTable<PassPlan> scr_plan = pair_arg_table(a->plan);
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const Step1PairLds scr_L = pair_lds_at_use(a, smem);
  f2* scr_pw = scr_L.pw;
  double* scr_stg = scr_L.stg;
  int* scr_ctl = scr_L.ctl;

  const int tid = threadIdx.x;
  const int scr_wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  // The host launches this kernel with 64 kPairWaves threads and nothing else (plan_m_best): the wavefront count is a
  // constant and the workgroup reductions test no slot (ph_device.h, red_combine), and so is the stride of the thread
  // loops (read from the dispatch packet it was a load through the vector memory pipe at every use, its address in a
  // vector register pair for the whole kernel).
  constexpr int NW = kPairWaves, nw = NW;
  constexpr int kThreads = NW * kWave;
  const double sqrtN = uniform_f64(sqrt((double)scr_N));

  {  // the windows' images and the bookkeeping of both (in front of the round loop: the screen's own values serve)
  const int N = scr_N, p_lo = scr_p_lo;
  const Step1PairLds& L = scr_L;
  f2* pw = scr_pw;
  double* stg = scr_stg;
  int* ctl = scr_ctl;
  const int SK = (a->p_hi - p_lo + 1 + 31) / 32;
  double *red = L.red, *norms = L.norms, *dst2 = L.dst2;
  uint32_t *periods = L.periods, *skip = L.skip;
  float* pwf = reinterpret_cast<float*>(pw);
  for (int k = tid; k < 2 * a->num; k += kThreads) {
    norms[k] = 0.0;
    periods[k] = 0u;
  }
  for (int k = tid; k < 2 * SK; k += kThreads) skip[k] = 0u;
  if (tid < MP_WORDS) ctl[tid] = tid == MP_QUEUE ? nw : 0;
  zero_pad<NW>(stg, N);
  for (int i = tid; i < kPad; i += kThreads) pw[N + i] = f2_zero();
  for (int w = 0; w < 2; ++w) {
    const int64_t gw = 2 * (int64_t)blockIdx.x + w;
    const bool exists = gw < a->W;
    __syncthreads();
    if (exists) {
      load_window<NW>(pair_arg_global(a->x) + gw * (int64_t)N, stg, N);
    } else {
      for (int n = tid; n < N; n += kThreads) stg[n] = 0.0;
    }
    __syncthreads();
    const double rsq = block_sumsq<NW>(stg, N, red);
    const double sc = uniform_f64(pair_pick_scale(rsq, N));
    for (int n = tid; n < N; n += kThreads) pwf[2 * n + w] = (float)(stg[n] * sc);
    if (tid == 0) {
      dst2[MP_UNIT + w] = rsq * sc * sc * (1.0 + 1e-9);
      dst2[MP_SCALE + w] = sc;
      ctl[MP_RUNNING + w] = exists ? 1 : 0;
      ctl[MP_EXACT_ALL + w] = pair_usable(rsq) ? 0 : 1;
      if (exists) pair_arg_global(a->dnorm_out)[gw] = periodic_norm_from_sq_n(rsq, sqrtN, 0);
    }
  }
  }
  StageClock<kPairTimers, 6, 3> clk;  // stages: screen, scan, load, thin, exact, update; counters: candidates, exact_all, folded
  WgStamp<kClocks> stamp;
  for (;;) {
    __syncthreads();
    // (values that are identical in all lanes go to scalar registers as they are read: as vector registers they were
    // spilled around the screen, and every reload is a scratch access through L2 on the critical path of the exact phases)
    const bool act0 = __builtin_amdgcn_readfirstlane(scr_ctl[MP_RUNNING]) != 0, act1 = __builtin_amdgcn_readfirstlane(scr_ctl[MP_RUNNING + 1]) != 0;
    if (!act0 && !act1) break;
    prio_by_progress(__builtin_amdgcn_readfirstlane(max(scr_ctl[MP_SWEEPS], scr_ctl[MP_SWEEPS + 1])));  // sweeps done: keeps the two workgroups of a CU in step (ph_device.h)
    if (scr_wv == 0 && pair_lane() == 0) scr_ctl[MP_LISTED] = scr_ctl[MP_LISTED + 1] = 0;  // (read as `ncand` before the last barrier of the previous round)
    // ---- 1. screen of both windows (Periods.py:501-515 in float); values into the idle staging buffer
    f2* vals = reinterpret_cast<f2*>(scr_stg);
    pair_sweep_plan<false, true>(
        scr_pw, scr_N, scr_geomf, scr_plan, scr_wv, scr_n_pass, nw, [&](float z, int q) { pair_store1(vals, z, q, scr_p_lo); },
        [&](float z, int q_a, int q_b) { pair_store2(vals, z, q_a, q_b, scr_p_lo); },
        PH_PAIR_QUEUE ? &scr_ctl[MP_QUEUE] : nullptr);
    __syncthreads();
    clk.mark(0);
    prio_short_phase();
    {  // phases 2 and 3 of this round
    // The thread and lane indices are RECOMPUTED here (wave number in a scalar register + v_mbcnt): kept live across the
    // screen they were spilled, and the exact phases reloaded them from scratch -- through L2 -- fifteen times per round.
    // (the wave number through its scalar register, as const_at_use: what the phases derive from it -- LDS addresses of a
    // thread's slots -- is then made here, by the scalar unit, and not kept in lanes across the screen)
    const int wv = const_at_use(scr_wv);
    const int tid = (wv << 6) + pair_lane();
    const int lane = tid & (kWave - 1);
    if (tid == 0) scr_ctl[MP_QUEUE] = nw;  // the pass queue of the next screen (barriers in between)
    // ---- 2. survivors of both windows: two passes over the screened values
    {
      const bool scr0 = act0 && !__builtin_amdgcn_readfirstlane(scr_ctl[MP_EXACT_ALL]), scr1 = act1 && !__builtin_amdgcn_readfirstlane(scr_ctl[MP_EXACT_ALL + 1]);
      if (scr0 || scr1) {
        // (everything the scan works with is fetched or derived here, behind the screen: nothing of it is live across the passes)
        const step1_pair_args_ptr A = pair_args_at_use();
        const int N = A->N, p_lo = A->p_lo, P = A->p_hi - p_lo + 1, SK = (P + 31) / 32, p_scr = A->p_scr, gamma = A->gamma;
        const Step1PairLds L = pair_lds_at_use(A, smem);
        double *stg = L.stg, *red = L.red, *dst2 = L.dst2;
        int *list = L.list, *ctl = L.ctl;
        const uint32_t* skip = L.skip;
        const f2* vals = reinterpret_cast<const f2*>(stg);
        const ConstTable<double> radq = pair_arg_table(A->radq);
        const ConstTable<int> fac_off = pair_arg_table(A->fac_off);
        const ConstTable<int> fac_q = pair_arg_table(A->fac_q);
        const double unit0 = uniform_f64(dst2[MP_UNIT]), unit1 = uniform_f64(dst2[MP_UNIT + 1]);
        // cover rule: the screened periods bound their divisors below p_scr.  `seen` (a bit per such divisor and
        // window, so that a divisor of two covering periods is listed once) lies in front of the first screened
        // value: 2 SD words <= 8 (p_scr - p_lo) bytes.
        const int i0 = p_scr - p_lo;
        const bool cover = i0 > 0;
        const int SD = (i0 + 31) >> 5;
        uint32_t* seen = reinterpret_cast<uint32_t*>(stg);
        for (int k = tid; k < 2 * SD; k += kThreads) seen[k] = 0u;
        const double slack = cover ? pair_cover_slack(N) : 0.0;
        // One screened entry as both passes need it: the two values, the radius -- radq[q] = pair_radius(ceil(N / q), q)
        // from the host table next to geomf, the bound the proof in ph_pair.h states -- 1 / q in gamma mode and the skip
        // bits.  At most kThreads entries (683 of 1024 threads at N = 4096) means one entry per thread: it is read
        // once and stays in registers across the barrier.
        struct Entry {
          f2 v;
          double rad, rq;
          bool skip0, skip1;
        };
        auto entry = [&](int idx) {
          Entry e;
          const int q = p_lo + idx;
          const uint32_t bit = 1u << (idx & 31);
          e.v = vals[idx];
          e.rad = radq[q];
          e.rq = gamma ? 1.0 / (double)q : 1.0;
          e.skip0 = (skip[idx >> 5] & bit) != 0;
          e.skip1 = (skip[SK + (idx >> 5)] & bit) != 0;
          return e;
        };
        const int idx_own = i0 + tid;
        Entry own = {f2_zero(), 0.0, 1.0, true, true};
        if (idx_own < P) own = entry(idx_own);
        const double ninf = const_at_use(-1.0 / 0.0);  // (as a vector-register invariant it was spilled around the screen)
        double lo0 = ninf, lo1 = ninf;
        for (int idx = idx_own; idx < P; idx += kThreads) {
          const Entry e = idx == idx_own ? own : entry(idx);
          double a = (double)e.v.x - e.rad * unit0, b = (double)e.v.y - e.rad * unit1;
          if (gamma) {
            a *= e.rq;
            b *= e.rq;
          }
          if (!e.skip0 && a > lo0) lo0 = a;
          if (!e.skip1 && b > lo1) lo1 = b;
        }
        lo0 = wave_max(lo0);
        lo1 = wave_max(lo1);
        if (lane == 0) {
          red[wv] = lo0;
          red[kMaxWaves + wv] = lo1;
        }
        __syncthreads();
        // (every wavefront combines the two maxima itself.  Combined by wavefront 0 alone and read back behind one more
        // barrier, the counter of a launch fell by 0.7e6 of the 4.8e6 its 2 x 31 v_max_f64 predict: with that form in the
        // kernel the plan pointer of the screen is parked in lanes and read back in front of every pass.  Not kept.)
        lo0 = uniform_f64(red_combine<true, NW>(red, nw));
        lo1 = uniform_f64(red_combine<true, NW>(red + kMaxWaves, nw));
        // every screened period skipped: nothing bounds the winner from below, every period goes through the exact phase
        const bool none0 = cover && scr0 && !(lo0 > ninf), none1 = cover && scr1 && !(lo1 > ninf);
        if (tid == 0 && none0) ctl[MP_LISTED] = kPairListCap + 1;
        if (tid == 0 && none1) ctl[MP_LISTED + 1] = kPairListCap + 1;
        // periods that tie with the winner in the ROUNDED norm survive too
        const double thr0 = lo0 - fabs(lo0) * 1e-9, thr1 = lo1 - fabs(lo1) * 1e-9;
        for (int idx = idx_own; idx < P; idx += kThreads) {
          const Entry e = idx == idx_own ? own : entry(idx);
          const int q = p_lo + idx;
          const double rad = e.rad + slack;
          double a = (double)e.v.x + rad * unit0, b = (double)e.v.y + rad * unit1;
          if (gamma) {
            a *= e.rq;
            b *= e.rq;
          }
          const bool hit0 = scr0 && !none0 && a >= thr0, hit1 = scr1 && !none1 && b >= thr1;
          if (hit0 && !e.skip0) {
            const int k = atomicAdd(&ctl[MP_LISTED], 1);
            if (k < kPairListCap) list[k] = q;
          }
          if (hit1 && !e.skip1) {
            const int k = atomicAdd(&ctl[MP_LISTED + 1], 1);
            if (k < kPairListCap) list[kPairListCap + k] = q;
          }
          if (cover && (hit0 || hit1)) {
            // q covers (skipped or not): its proper divisors in [p_lo, p_scr) may hold the maximum
            const int f1 = fac_off[q + 1];
            for (int f = fac_off[q] - (p_lo == 1 ? 1 : 0); f < f1; ++f) {
              const int d = f < fac_off[q] ? 1 : fac_q[f];  // the table leaves out 1
              if (d < p_lo || d >= p_scr) continue;
              const int di = d - p_lo;
              const uint32_t dbit = 1u << (di & 31);
              for (int w = 0; w < 2; ++w) {
                if (!(w ? hit1 : hit0) || (skip[w * SK + (di >> 5)] & dbit)) continue;
                if (atomicOr(&seen[w * SD + (di >> 5)], dbit) & dbit) continue;
                const int k = atomicAdd(&ctl[MP_LISTED + w], 1);
                if (k < kPairListCap) list[w * kPairListCap + k] = d;
              }
            }
          }
        }
      }
    }
    __syncthreads();
    clk.mark(1);
    // ---- 3. exact phase, one window at a time through the staging buffer
    for (int w = 0; w < 2; ++w) {
      if (!(w ? act1 : act0)) continue;
      // (as in the scan: the arguments and the LDS layout of this window-sweep, fetched and derived behind the screen)
      const step1_pair_args_ptr A = pair_args_at_use();
      const int N = A->N, p_lo = A->p_lo, P = A->p_hi - p_lo + 1, SK = (P + 31) / 32;
      const int num = A->num, p_scr = A->p_scr, gamma = A->gamma, max_iters = A->max_iters, row_stride = A->row_stride;
      const Step1PairLds L = pair_lds_at_use(A, smem);
      double *stg = L.stg, *red = L.red, *wbest = L.wbest, *norms = L.norms, *dst2 = L.dst2, *msm = L.msm, *prt = L.prt;
      int *wbestp = L.wbestp, *list = L.list, *ctl = L.ctl;
      uint32_t *periods = L.periods, *skip = L.skip;
      float* pwf = reinterpret_cast<float*>(L.pw);
      const size_t gstride = win_stride((size_t)N);
      const bool fold_once = __double2hiint(A->thin_band) >= 0;  // (the sign bit, on the scalar unit)
      const double* __restrict__ x = pair_arg_global(A->x);
      double* __restrict__ gres = pair_arg_global(A->gres);
      double* __restrict__ rows_out = pair_arg_global(A->rows_out);
      const ConstTable<PGeom> geom = pair_arg_table(A->geom);
      const int64_t gw = 2 * (int64_t)blockIdx.x + w;
      int filled = __builtin_amdgcn_readfirstlane(ctl[MP_FILLED + w]), repeats = __builtin_amdgcn_readfirstlane(ctl[MP_REPEATS + w]), status = 0,
          iters = __builtin_amdgcn_readfirstlane(ctl[MP_SWEEPS + w]);
      const int nlisted = __builtin_amdgcn_readfirstlane(ctl[MP_LISTED + w]);
      const bool exact_all = __builtin_amdgcn_readfirstlane(ctl[MP_EXACT_ALL + w]) != 0 || nlisted > kPairListCap;
      int ncand = exact_all ? P : nlisted;
      double* nrm = norms + w * num;
      uint32_t* per = periods + w * num;
      uint32_t* sk = skip + w * SK;
      const int* lst = list + w * kPairListCap;
      __syncthreads();
      bool folded = false;  // this window-sweep took the fold-once path
      if (iters + 1 > max_iters) {
        status = 2;
      } else {
        const double* src = iters == 0 ? x + gw * (int64_t)N : gres + gw * gstride;
        iters += 1;
        // ---- fold-once path (ph_pair.h, pair_thin_band): the list is one top period m > kPairSmallP and divisors of it.
        // The residual is folded once, at m, straight from the workspace (the input before the first subtraction): the
        // column sums S_m go to the idle staging buffer and give the cooperative value of m -- thread <-> residue and
        // order of pair_exact_part --, the value of every listed divisor and the means of the update.  A divisor within
        // the band of m (a window that is d-periodic), or any other list, takes the phases below from the staging load on.
        int fold_m = 0;
        double fold_ss = 0.0;
        if (fold_once && !exact_all) {
          const int k0 = lane, k1 = kWave + lane;
          const int q0 = k0 < ncand ? lst[k0] : 0, q1 = k1 < ncand ? lst[k1] : 0;
          const unsigned long long t0 = __ballot(q0 >= p_scr), t1 = __ballot(q1 >= p_scr);
          if (__popcll(t0) + __popcll(t1) == 1) {
            const int m = t0 ? __builtin_amdgcn_readlane(q0, __builtin_amdgcn_readfirstlane(__ffsll((long long)t0) - 1))
                             : __builtin_amdgcn_readlane(q1, __builtin_amdgcn_readfirstlane(__ffsll((long long)t1) - 1));
            // every other entry must divide m (a skipped top period lists its divisors too): m = k d with k the rounded
            // float quotient, exact for m < 2^22
            const float fm = (float)m;
            const int c0 = (int)(fm * __builtin_amdgcn_rcpf((float)max(q0, 1)) + 0.5f), c1 = (int)(fm * __builtin_amdgcn_rcpf((float)max(q1, 1)) + 0.5f);
            const bool odd = (k0 < ncand && c0 * q0 != m) || (k1 < ncand && c1 * q1 != m);
            if (m > kPairSmallP && __ballot(odd) == 0ull) fold_m = m;
          }
        }
        if (fold_m != 0) {
          const PGeom gm = geom[fold_m];
          double part = 0.0;
          if (tid == 0) wbestp[0] = 0;  // the tie flag of the thinning below
          for (int j = tid; j < fold_m; j += kThreads) {
            const bool full = j < gm.nfull;
            const double s = pair_column_sum_global(src, j, fold_m, full ? gm.rows : gm.rows - 1);
            part = fma(s * s, full ? gm.w_full : gm.w_short, part);
            stg[j] = s;
          }
          fold_ss = block_sum_lead<NW>(part, red, wv, lane);
          clk.mark(2);
          if (ncand > 1) {
            // a wavefront per listed divisor: its value from S_m (pair_thin_part) against the threshold; one that reaches it
            // raises the flag (wbestp is idle on this path; cleared in front of the barriers of the block sum above)
            // the band in the units of the values: MP_UNIT without its scale, a power of two
            const int se = __builtin_amdgcn_frexp_exp(dst2[MP_SCALE + w]) - 1;
            const double band = A->thin_band * ldexp(dst2[MP_UNIT + w], -2 * se);
            // (1e-9 through a scalar register pair at its use: as a loop invariant in vector registers it is spilled around
            // the screen)
            double tie = 1e-9;
            asm volatile("" : "+s"(tie));
            const double thr = fold_ss - fabs(fold_ss) * tie - band;
            for (int k = wv; k < ncand; k += nw) {
              const int d = __builtin_amdgcn_readfirstlane(lst[k]);
              if (d == fold_m) continue;
              const double t = wave_sum(pair_thin_part(stg, fold_m, d, geom[d], lane));
              if (lane == 0 && !(t < thr)) wbestp[0] = 1;
            }
            __syncthreads();
            // (a window that falls back rewrites the staging buffer at once; wbestp only behind further barriers)
            if (__builtin_amdgcn_readfirstlane(wbestp[0]) != 0) fold_m = 0;
          }
          clk.mark(3);
        }
        if (fold_m == 0) {
        load_window<NW>(src, stg, N);
        __syncthreads();
        clk.mark(2);
        if (p_scr > p_lo && !exact_all && ncand > 1) {
          // cover rule: the list holds the surviving screened periods AND their divisors, which no screen value has
          // thinned out.  A wavefront per candidate evaluates them in fp64; only those within 1e-9 (relative) of the
          // largest value -- the winner and whatever may tie with it in the rounded norm -- stay for the decision
          // below.  (msm is idle until a winner is projected; kPairListCap <= kPairSmallP.)
          for (int k = wv; k < ncand; k += nw) {
            const int p = lst[k];
            const PGeom g = geom[p];
            const double part = p < 64 ? wave_partial_small(stg, N, p, g, lane) : pair_exact_part(stg, p, g, lane, kWave);
            const double ss = wave_sum(part);
            if (lane == 0) msm[k] = ss;
          }
          __syncthreads();
          if (wv == 0) {
            const int k0 = lane, k1 = kWave + lane;
            const double v0 = k0 < ncand ? msm[k0] : -1.0, v1 = k1 < ncand ? msm[k1] : -1.0;
            const int q0 = lst[k0], q1 = k1 < kPairListCap ? lst[k1] : 0;
            const double top = wave_max(fmax(v0, v1));
            const bool keep0 = k0 < ncand && v0 >= top - fabs(top) * 1e-9, keep1 = k1 < ncand && v1 >= top - fabs(top) * 1e-9;
            const unsigned long long m0 = __ballot(keep0), m1 = __ballot(keep1);
            const int n0 = __popcll(m0);
            int* out = list + w * kPairListCap;
            // (set bits below the lane with v_mbcnt: the mask (1 << lane) - 1 was built in front of the exact phase
            // of every round and spilled, 16 bytes per lane)
            const auto below = [](unsigned long long m) {
              return (int)__builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
            };
            if (keep0) out[below(m0)] = q0;
            if (keep1) out[n0 + below(m1)] = q1;
            if (lane == 0) ctl[MP_LISTED + w] = n0 + __popcll(m1);
          }
          __syncthreads();
          ncand = __builtin_amdgcn_readfirstlane(ctl[MP_LISTED + w]);
        }
        clk.mark(3);
        }  // staging load and thinning of a window-sweep that does not fold once
        folded = fold_m != 0;
        if (kPairTimers) {  // (spelled out: an unused look at exact_all changes the branches the compiler builds from it)
          clk.count(0, exact_all ? P : nlisted);  // (candidates in front of the thinning)
          clk.count(1, exact_all ? 1 : 0);
          clk.count(2, fold_m != 0 ? 1 : 0);
        }
        double best_ss = 0.0;
        int bestp = 0;
        // (the norm with sqrt(N) from a scalar register)
        const auto norm = [&](double s, int div) { return periodic_norm_from_sq_n(s, sqrtN, div); };
        auto consider = [&](double ss, int p) {
          if (!(ss > 0.0)) return;
          if (mbest_prefers(ss, p, best_ss, bestp, gamma, norm)) {
            best_ss = ss;
            bestp = p;
          }
        };
        double best = 0.0;  // NOT identical in every thread on the fold-once path: the norm in wavefront 0, 0.0 elsewhere (thread 0 books it)
        if (fold_m != 0) {
          consider(fold_ss, fold_m);
          // The rounded norm of the winner is booked by thread 0 alone (mbest_book): wavefront 0 takes the square root and
          // the divisions, the others do not.  Nobody needs the test `best > 0` here: consider() took m only with
          // fold_ss > 0, and the root of a positive double is at least 2^-537, which divided by sqrt(N) sqrt(m) < 2^32
          // stays positive -- so the norm is positive exactly when bestp is set.
          if (wv == 0) best = bestp != 0 ? periodic_norm_from_sq_n(best_ss, sqrtN, gamma ? bestp : 0) : 0.0;
        } else if (ncand <= kPairCoop) {
          // few survivors (the normal case): the whole workgroup folds one candidate at a time, a wavefront per
          // 64 residues; partial sums are combined in wave order, so every thread holds the same value
          for (int k = 0; k < ncand; ++k) {
            const int p = exact_all ? p_lo + k : lst[k];
            if (skip_test(sk, p - p_lo)) continue;
            const PGeom g = geom[p];
            double part = 0.0;
            if (p < 64) {
              if (wv == 0) part = wave_partial_small(stg, N, p, g, lane);
            } else {
              part = pair_exact_part(stg, p, g, tid, kThreads);
            }
            consider(block_sum<NW>(part, red), p);
          }
          best = bestp != 0 ? periodic_norm_from_sq_n(best_ss, sqrtN, gamma ? bestp : 0) : 0.0;
          if (!(best > 0.0)) bestp = 0;  // the reference needs p_norm > 0 (Periods.py:497,512)
        } else {
          for (int k = wv; k < ncand; k += nw) {
            const int p = exact_all ? p_lo + k : lst[k];
            if (skip_test(sk, p - p_lo)) continue;
            const PGeom g = geom[p];
            const double part = p < 64 ? wave_partial_small(stg, N, p, g, lane) : pair_exact_part(stg, p, g, lane, kWave);
            consider(wave_sum(part), p);
          }
          best = bestp != 0 ? periodic_norm_from_sq_n(best_ss, sqrtN, gamma ? bestp : 0) : 0.0;
          if (!(best > 0.0)) bestp = 0;
          if (lane == 0) {
            wbest[wv] = best;
            wbestp[wv] = bestp;
          }
          __syncthreads();
          red_argmax<NW>(wbest, wbestp, nw, best, bestp);
          __syncthreads();
        }
        clk.mark(4);
        if (bestp == 0) {  // reference: max_base is None -> TypeError at Periods.py:520/537
          status = 1;
        } else {
          // bookkeeping (mbest_book)
          // (the row that holds the winner already: 64 rows per ballot instead of `num` LDS reads in every thread)
          int row = -1;
          for (int k0 = 0; k0 < num; k0 += kWave) {
            const unsigned long long hit = __ballot(k0 + lane < num && per[k0 + lane] == (uint32_t)bestp);
            if (hit) row = k0 + 63 - __clzll(hit);
          }
          const int action = mbest_book(row, bestp, best, p_lo, tid, filled, repeats, nrm, per, sk);
          // project the winner (row order), update the compact basis row, subtract (:531-537).  The new residual is
          // not needed in LDS again: it goes straight to the workspace and, as floats, into pw.  The scale of the
          // float image only has to keep the RMS near 1; it is renewed when the residual has shrunk by 2^16.
          double* brow = rows_out + (gw * (int64_t)num + (row < 0 ? 0 : row)) * row_stride;
          const bool more = filled < num;
          const double sc = uniform_f64(dst2[MP_SCALE + w]);
          double* dst = gres + gw * gstride;
          double acc = 0.0;
          const PGeom gb = geom[__builtin_amdgcn_readfirstlane(bestp)];  // (a scalar load; Fold(N, p) divides in every thread)
          const Fold f(bestp, gb.rows, gb.nfull);
          if (fold_m != 0) {
            // the means from the column sums in the staging buffer (S / cnt: residue_mean's expression); every thread
            // subtracts them from its own columns, read again from the source and written to the workspace -- in place
            // after the first sweep, a thread touches only its own columns
            for (int j = tid; j < bestp; j += kThreads) {
              const int cnt = f.count(j);
              const double m = stg[j] / (double)cnt;
              if (action == 1)
                brow[j] = m;
              else if (action == 2)
                brow[j] += m;
              if (more) {
                // (four rows are read before the first is written: source and workspace may be the same memory, and a
                // load behind a store would wait for it)
                for (int r0 = 0; r0 < cnt; r0 += 4) {
                  const unsigned at = (unsigned)(r0 * bestp + j);
                  double v[4];
#pragma unroll
                  for (int u = 0; u < 4; ++u) v[u] = src[r0 + u < cnt ? at + (unsigned)(u * bestp) : at];
#pragma unroll
                  for (int u = 0; u < 4; ++u) {
                    if (r0 + u < cnt) {
                      const unsigned n = at + (unsigned)(u * bestp);
                      const double t = v[u] - m;
                      dst[n] = t;
                      pwf[2 * n + w] = (float)(t * sc);
                      acc = fma(t, t, acc);
                    }
                  }
                }
              }
            }
          } else if (bestp <= kPairSmallP) {
            // a short period: its few residues have hundreds of rows each -- means through LDS, the subtraction is spread
            // over the workgroup
            // (the usual winner of m_best_gamma); split_row_means deals the rows of a residue to several threads
            split_row_means(stg, msm, prt, N, bestp, tid, kPairSplitW);
            if (tid < bestp) {
              const double m = msm[tid];
              if (action == 1)
                brow[tid] = m;
              else if (action == 2)
                brow[tid] += m;
            }
            if (more) {
              int idx = tid % bestp;
              const int step = kThreads % bestp;
              for (int n = tid; n < N; n += kThreads) {
                const double v = stg[n] - msm[idx];
                dst[n] = v;
                pwf[2 * n + w] = (float)(v * sc);
                acc = fma(v, v, acc);
                idx += step;
                idx = idx >= bestp ? idx - bestp : idx;
              }
            }
          } else {
            for (int j = tid; j < bestp; j += kThreads) {
              const double m = residue_mean(stg, f, j, false);
              const int cnt = f.count(j);
              if (action == 1)
                brow[j] = m;
              else if (action == 2)
                brow[j] += m;
              if (more) {
                for (int r = 0; r < cnt; ++r) {
                  const int n = r * bestp + j;
                  const double v = stg[n] - m;
                  dst[n] = v;
                  pwf[2 * n + w] = (float)(v * sc);
                  acc = fma(v, v, acc);
                }
              }
            }
          }
          if (more) {
            const double rsq = block_sum_lead<NW>(acc, red, wv, lane);
            const double unit = rsq * sc * sc;
            // (pair_usable and pair_image_stale written out, their constants through scalar registers at this use: as
            // loop invariants in vector registers 1.79e308 and 9e-13 N were spilled around the round loop, and both
            // came back from scratch right behind the block sum of every window-sweep)
            const bool ok = rsq > 0.0 && rsq < const_at_use(1.79e308);
            if (ok && unit < const_at_use(kPairStaleMeanSq) * (double)const_at_use(N)) {
              const double sc2 = uniform_f64(pair_pick_scale(rsq, N));
              __syncthreads();
              pair_rescale<NW>(pwf, w, N, (float)(sc2 / sc), tid);
              if (tid == 0) {
                dst2[MP_UNIT + w] = rsq * sc2 * sc2 * (1.0 + 1e-9);
                dst2[MP_SCALE + w] = sc2;
              }
            } else if (tid == 0) {
              dst2[MP_UNIT + w] = unit * (1.0 + 1e-9);
            }
            if (tid == 0) ctl[MP_EXACT_ALL + w] = ok ? 0 : 1;
          }
        }
      }
      __syncthreads();
      if (tid == 0) {
        ctl[MP_FILLED + w] = filled;
        ctl[MP_REPEATS + w] = repeats;
        ctl[MP_STATUS + w] = status | (((ctl[MP_STATUS + w] >> 8) + (folded ? 1 : 0)) << 8);
        ctl[MP_SWEEPS + w] = iters;
        ctl[MP_RUNNING + w] = (status == 0 && filled < num) ? 1 : 0;
      }
      clk.mark(5);
    }
    }  // phases 2 and 3
  }
  if (kClocks && (blockIdx.x % 16) == 7 && tid == 0) {
    stamp.finish();
    printf("PAIRWG %d start %lld end %lld cycles %lld MHz %.0f hwid %x xcc %x\n", (int)blockIdx.x, stamp.wk0, stamp.wk1, stamp.ck1 - stamp.ck0,
           100.0 * (double)(stamp.ck1 - stamp.ck0) / (double)(stamp.wk1 - stamp.wk0), stamp.hwid, stamp.xcc);
  }
  if (kPairTimers && blockIdx.x < PH_PAIR_TIMERS_WGS && tid == 0)
    printf("pair timers (100 MHz ticks) screen %lld scan %lld load %lld thin %lld exact %lld update %lld  candidates %d exact_all %d folded %d sweeps %d %d\n",
           clk.ticks(0), clk.ticks(1), clk.ticks(2), clk.ticks(3), clk.ticks(4), clk.ticks(5), clk.counted(0), clk.counted(1), clk.counted(2), scr_ctl[MP_SWEEPS],
           scr_ctl[MP_SWEEPS + 1]);
  __syncthreads();
  {  // the outputs
    const step1_pair_args_ptr A = pair_args_at_use();
    const int num = A->num, fold_report = A->fold_report;
    const Step1PairLds L = pair_lds_at_use(A, smem);
    const double* norms = L.norms;
    const uint32_t* periods = L.periods;
    const int* ctl = L.ctl;
    uint32_t* __restrict__ periods_out = pair_arg_global(A->periods_out);
    double* __restrict__ norms_out = pair_arg_global(A->norms_out);
    int* __restrict__ status_out = pair_arg_global(A->status_out);
    int* __restrict__ sweeps_out = pair_arg_global(A->sweeps_out);
    // rows the algorithm never filled keep period 0: step 2 writes them as zeros (np.zeros((num, N)), Periods.py:490)
    for (int w = 0; w < 2; ++w) {
      const int64_t gw = 2 * (int64_t)blockIdx.x + w;
      if (gw >= A->W) continue;
      for (int k = tid; k < num; k += kThreads) {
        periods_out[gw * num + k] = periods[w * num + k];
        norms_out[gw * num + k] = norms[w * num + k];
      }
      if (tid == 0) {
        status_out[gw] = ctl[MP_STATUS + w] & 255;
        // fold_report (PH_PAIR_FOLD_REPORT=1, tests): the fold-once count of the window above bit 16 of its sweep count
        if (sweeps_out) sweeps_out[gw] = ctl[MP_SWEEPS + w] | (fold_report ? (ctl[MP_STATUS + w] >> 8) << 16 : 0);
      }
    }
  }
}

// ======================================================================================
// m_best step 2  (Periods.py:540-598): factor refinement, including the reference's
// quirks: stale `p` in gamma mode (:559,572), `nq` = norm of the LAST factor's projection
// (:569-572), no advance of i after a split (:581-594).  One workgroup per window.
// norms_io holds raw norms on entry and powers (norms / ||data||, :600) on exit.
//   Compact rows.  Basis row i is the tiled mean vector m of its period p (step 1 writes nothing else, a
//   split keeps it so: the factor's projection is f-periodic, f | p), so step 1 hands over only the first
//   p elements of every row and np.insert (:585-594) becomes a permutation of row slots: a split writes
//   two compact rows (the projection into the slot of the row that falls off the end, the remainder in
//   place) and moves no data.  The (num, N) matrix is written exactly once, in final order, each row as
//   soon as the loop has passed it.
//   For a divisor f of p
//     S_f[j] = sum_{n < N, n = j (mod f)} row[n] = sum_{k < p, k = j (mod f)} cnt_p[k] m[k],
//   so the factor norms (plain projection, fp64) fold the count-scaled p-vector -- a "window" of length p
//   whose every residue mod f has p/f rows -- instead of the N-element row.  The count weights 1/cnt_f[j]
//   are those of the real window: the fold runs on geom[f] with rows := p/f + 1, whose one extra row for
//   the residues j < nfull_f reads zeros stored behind the vector.
// ======================================================================================
// geom[p] computed in registers (same expressions as prepare_geom on the host; IEEE divisions)
__device__ __forceinline__ PGeom make_geom(int N, int p) {
  const int rows = (N + p - 1) / p;
  PGeom g;
  g.rows = rows;
  g.nfull = p - (rows * p - N);
  g.w_full = 1.0 / (double)rows;
  g.w_short = rows > 1 ? 1.0 / (double)(rows - 1) : 0.0;
  return g;
}

constexpr int kStep2Pre = 3;  // a staged row has at most 3 elements per thread (p <= 3 * blockDim)
// bit of k_mbest_step2's `flags` beside kTrunc / kOrth: a factor's fold geometry is read from the host's table
// (PH_STEP2_GEOM=0 clears it: lane 0 rebuilds it per factor and hands it over through LDS)
constexpr unsigned kStep2Geom = 0x100u;
typedef __attribute__((address_space(3))) void* lds_void_ptr;
typedef const __attribute__((address_space(1))) void* global_void_ptr;

// rowbuf[n] = row[n mod p], n < N: the tiled row of a compact vector
template <typename T>
__device__ __forceinline__ void expand_row(const T* __restrict__ src, int p, T* __restrict__ dst, int N) {
  const int step = blockDim.x % p;
  int idx = threadIdx.x % p;
  for (int n = threadIdx.x; n < N; n += blockDim.x) {
    dst[n] = src[idx];
    idx += step;
    if (idx >= p) idx -= p;
  }
}

template <typename T>
struct Step2Lds {
  T* rowbuf;
  T* buf;
  double* red;
  double* norms;
  uint32_t* periods;
  double* fvals;
  int* ffac;
  PGeom* fgeom;    // per wavefront: geometry of the fold of a periodic row
  int* fa;         // divisor list of row k's period: tb.fac_q[fa[k] .. fb[k])
  int* fb;
  int* slot;       // compact row of logical row k: rows + slot[k] * row_stride
  int* ffac_next;  // divisor list of the staged row
  size_t bytes;
};
// max_fac = most proper divisors any candidate period has (PGeom / divisor slots of step 2)
template <typename T, class C>
__host__ __device__ __forceinline__ Step2Lds<T> step2_carve(C cv, int N, int num, int max_fac, bool lw, bool buf_lds) {
  Step2Lds<T> L;
  L.rowbuf = lw ? cv.template take<T>(N + kPad) : nullptr;
  L.buf = buf_lds ? cv.template take<T>(N) : nullptr;
  L.red = cv.template take<double>(kRedDoubles);
  L.norms = cv.template take<double>(num);
  L.periods = cv.template take<uint32_t>(num);
  L.fvals = cv.template take<double>(max_fac > 0 ? max_fac : 1);
  L.ffac = cv.template take<int>(max_fac > 0 ? max_fac : 1);
  L.fgeom = cv.template take<PGeom>(kMaxWaves);
  L.fa = cv.template take<int>(num);
  L.fb = cv.template take<int>(num);
  L.slot = cv.template take<int>(num);
  L.ffac_next = cv.template take<int>(max_fac > 64 ? max_fac : 64);
  L.bytes = cv.off;
  return L;
}

template <typename T, bool LW>
__global__ __launch_bounds__(kBlockWide) __attribute__((amdgpu_waves_per_eu(PH_STEP1_WAVES, 8))) void k_mbest_step2(int N, int num, int gamma, int stale_p, unsigned flags,
                                                        Tables tb, const PGeom* __restrict__ geom, int max_fac,
                                                        T* __restrict__ gbuf, T* gwin,
                                                        uint32_t* __restrict__ periods_io,
                                                        double* __restrict__ norms_io, T* __restrict__ bases_out,
                                                        const double* __restrict__ dnorm,
                                                        const int* __restrict__ status, T* __restrict__ rows_io,
                                                        int row_stride) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const Step2Lds<T> L = step2_carve<T>(Carve(smem), N, num, max_fac, LW, !gbuf);
  T* rowbuf = window_buf<T, LW>(L.rowbuf, gwin, N + kPad);
  T* buf = second_buf(L.buf, gbuf, N);
  double *red = L.red, *norms = L.norms, *fvals = L.fvals;
  uint32_t* periods = L.periods;
  PGeom* fgeom = L.fgeom;
  int *ffac = L.ffac, *fa = L.fa, *fb = L.fb, *slot = L.slot, *ffac_next = L.ffac_next;

  const int64_t w = blockIdx.x;
  const int tid = threadIdx.x;
  const int lane = tid & (kWave - 1);
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int nw = blockDim.x >> 6;
  const bool general = flags & (kTrunc | kOrth);
  const bool periodic_rows = sizeof(T) == 8 && !general;
  T* rows = rows_io + w * (int64_t)num * row_stride;
  for (int k = tid; k < num; k += blockDim.x) {
    norms[k] = norms_io[w * num + k];
    const uint32_t per = periods_io[w * num + k];
    periods[k] = per;
    fa[k] = tb.fac_off[per];
    fb[k] = tb.fac_off[per + 1];
    slot[k] = k;
  }
  zero_pad(rowbuf, N);
  __syncthreads();

  StageClock<kStep2Timers, 7, 2> clk;  // stages: as printed below; counters: rows, splits
  const int gdiv = gamma ? stale_p : 0;
  int i = (status[w] == 0) ? 0 : num;  // a window whose step 1 failed is passed through
  // a row whose period has no proper divisor (a prime) has nothing to test and is not even read
  auto next_row = [&](int r) {  // (the same in every lane: scalar, and the row loop's branches with it)
    while (r < num && fa[r] == fb[r]) ++r;
    return __builtin_amdgcn_readfirstlane(r);
  };
  // The rows are short and known one row ahead: the next row's elements and divisor list are copied
  // HBM -> LDS by LDS-DMA (global_load_lds: no registers, the 64-VGPR fold code has none to spare) into the
  // unused upper part of rowbuf while the current row is folded -- the loop is otherwise a chain of dependent
  // HBM round trips (row, divisor list, geometry) per row.  The explicit s_waitcnt vmcnt(0) in front of the barrier
  // behind the folds drains the DMA: hipcc puts only lgkmcnt(0) in front of a __syncthreads of this kernel (its
  // other barriers do not wait for the tile-out stores).  On gfx950 vmcnt counts loads and stores alike, and the
  // compiler's wait for a load behind stores is vmcnt(0): it waits for the stores in flight as well.
  int stage_row = -1, stage_at = 0;  // the staged row and its offset in rowbuf
  // The (num, N) matrix is written exactly once, in final order: logical rows below the loop position can
  // no longer change (a split inserts at i and moves rows >= i only), so they are tiled out as the loop
  // passes them -- the stores drain while the next rows are folded.  Rows step 1 never filled (period 0)
  // are zeros (np.zeros((num, N)), Periods.py:490).
  T* out = bases_out + w * (int64_t)num * N;
  int done = 0;
  auto flush_rows = [&](int upto) {
    for (; done < upto; ++done) {
      const int pr = (int)periods[done];
      T* dst = out + (int64_t)done * N;
      if (pr == 0) {
        for (int n = tid; n < N; n += blockDim.x) dst[n] = T(0);
      } else {
        expand_row(rows + (int64_t)slot[done] * row_stride, pr, dst, N);
      }
    }
  };
  i = next_row(i);
  clk.mark(0);
  while (i < num) {
    // The thread's LDS and table addresses below are loop invariants, which the compiler computes once in front of
    // the loop and -- at the 64-VGPR cap of the fold code -- spills: every use then waits for a reload from scratch,
    // a memory round trip behind vmcnt(0) (the tile-out stores in flight included), a dozen per row.  Through an
    // opaque copy of the thread index per iteration each address is one or two vector instructions instead.
    int t = tid, ln = lane;
    asm volatile("" : "+v"(t), "+v"(ln));
    const int per = __builtin_amdgcn_readfirstlane((int)periods[i]);  // (uniform: what follows from it stays scalar)
    const int a = fa[i], b = fb[i];
    const T* src = rows + (int64_t)slot[i] * row_stride;
    // v[k] = cnt_p[k] m[k] for k < per, then zeros for the extra row and the tail reads of the last group
    const int zend = per + (per >> 1) + 256;
    const bool short_row = periodic_rows && zend <= N + kPad;
    if (short_row) {
      const PGeom gp = make_geom(N, per);
      const double cf = (double)gp.rows, cs = (double)(gp.rows - 1);
      if (stage_row == i) {  // the staging area may overlap [0, zend): read, barrier, write
        double el[kStep2Pre];
#pragma unroll
        for (int u = 0; u < kStep2Pre; ++u) {
          const int k = t + u * blockDim.x;
          el[u] = k < per ? (double)rowbuf[stage_at + k] : 0.0;
        }
        __syncthreads();
#pragma unroll
        for (int u = 0; u < kStep2Pre; ++u) {
          const int k = t + u * blockDim.x;
          if (k < zend) rowbuf[k] = (T)(el[u] * (k < gp.nfull ? cf : cs));
        }
        for (int k = t + kStep2Pre * blockDim.x; k < zend; k += blockDim.x) rowbuf[k] = T(0);
        if (t < b - a) ffac[t] = ffac_next[t];
      } else {
        for (int k = t; k < zend; k += blockDim.x)
          rowbuf[k] = (T)(k < per ? (double)src[k] * (k < gp.nfull ? cf : cs) : 0.0);
        if (t < b - a) ffac[t] = tb.fac_q[a + t];
      }
    } else {  // fp32 rows, trunc / orth modes, periods beyond 2N/3: the tiled row itself
      expand_row(src, per, rowbuf, N);
      if (!general && t < b - a) ffac[t] = tb.fac_q[a + t];
    }
    __syncthreads();
    clk.mark(1);
    const int inext = next_row(i + 1);
    stage_row = -1;
    if (LW && short_row && inext < num) {  // LW == false: rowbuf is an HBM workspace, nothing to stage into
      const int pn = __builtin_amdgcn_readfirstlane((int)periods[inext]);
      const int so = (zend + 1) & ~1;          // 16-byte aligned, behind everything the folds of row i read
      const int npieces = (pn + 127) >> 7;     // 64 lanes x 16 B = 128 doubles per wave instruction
      if (pn <= kStep2Pre * (int)blockDim.x && pn + (pn >> 1) + 256 <= N + kPad && so + 128 * npieces <= N &&
          128 * npieces <= row_stride && fb[inext] - fa[inext] <= 64) {
        const T* srcn = rows + (int64_t)slot[inext] * row_stride;  // 128 * npieces <= row_stride: stays inside the row
        for (int j = wv; j < npieces; j += nw)
          __builtin_amdgcn_global_load_lds((global_void_ptr)(srcn + 128 * j + 2 * ln),
                                           (lds_void_ptr)(rowbuf + so + 128 * j), 16, 0, 0);
        if (wv == nw - 1)  // reads up to 63 words behind the list: the device table has that slack
          __builtin_amdgcn_global_load_lds((global_void_ptr)(tb.fac_q + fa[inext] + ln), (lds_void_ptr)ffac_next, 4, 0, 0);
        stage_at = __builtin_amdgcn_readfirstlane(so);
        stage_row = inext;
      }
    }
    double top = 0.0, last = 0.0;
    int topf = -1;
    if (!general) {
      // one wavefront per factor: ||P_f row||^2 = sum_j S_f[j]^2 / cnt_f[j]
      for (int k = wv; k < b - a; k += nw) {
        // one call site for both row forms (a second inlined copy of the fold costs spills).  Compact row: a
        // "window" of length per with per / f rows per residue, weights by the real counts of f (rows + 1: see
        // the header; the f < 64 path ignores `rows`).
        PGeom g;
        int f;
        if (flags & kStep2Geom) {  // geom[f] holds make_geom(N, f) bit for bit (prepare_geom: the same expressions): scalar loads
          f = __builtin_amdgcn_readfirstlane(ffac[k]);
          g = geom[f];
          if (short_row) g.rows = per / f + 1;
        } else {  // lane 0 builds the geometry and hands it over in this wavefront's LDS slot
          f = ffac[k];
          if (lane == 0) {
            PGeom g0;
            if (short_row) {
              g0 = make_geom(N, f);
              g0.rows = per / f + 1;
            } else {
              g0 = geom[f];
            }
            fgeom[wv] = g0;
          }
          ram_wave_sync();
          const PGeom gl = fgeom[wv];  // (into scalar registers, where the table's copy arrives too)
          g.rows = __builtin_amdgcn_readfirstlane(gl.rows);
          g.nfull = __builtin_amdgcn_readfirstlane(gl.nfull);
          g.w_full = uniform_f64(gl.w_full);
          g.w_short = uniform_f64(gl.w_short);
          f = __builtin_amdgcn_readfirstlane(f);
          ram_wave_sync();  // the slot is rewritten for this wavefront's next factor
        }
        const double ss = wave_sum(wave_partial<T, false, LW>(rowbuf, short_row ? per : N, f, g, lane));
        if (lane == 0) fvals[k] = periodic_norm_from_sq(ss, N, gdiv);
      }
      clk.mark(2);
      __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0): the LDS-DMA of the next row has landed
      __syncthreads();
      clk.mark(3);
      // rows below i are final: their stores drain behind the scan below and the next row's folds (issued
      // here, after the wait above, so that the DMA is not held up behind them)
      flush_rows(i);
      for (int k = 0; k < b - a; ++k) {  // the reference's scan order (Periods.py:549-563)
        const double v = fvals[k];
        if (v > top) {
          top = v;
          topf = ffac[k];
        }
        last = v;
      }
    } else {
      flush_rows(i);
      for (int k = a; k < b; ++k) {
        const int f = tb.fac_q[k];
        const double v = block_sweep_value(rowbuf, buf, N, f, gdiv, flags, tb, red);
        if (v > top) {
          top = v;
          topf = f;
        }
        last = v;
      }
    }
    bool split = false;
    if (topf >= 0) {
      bool present = false;
      for (int k = 0; k < num; ++k) present |= (periods[k] == (uint32_t)topf);
      if (!present) {
        double floor_q = norms[0];
        for (int k = 1; k < num; ++k) floor_q = fmin(floor_q, norms[k]);
        split = (last + top) > (norms[num - 1] + norms[i]) && last > floor_q && top > floor_q;
      }
    }
    const int s_here = slot[i], s_last = slot[num - 1];
    __syncthreads();
    clk.mark(4);
    clk.count(0);
    clk.count(1, split ? 1 : 0);
    if (!split) {
      i = inext;
      continue;
    }
    // ---- split (:581-594): materialise the winning factor's projection exactly;
    //   logical rows i+2.. <- rows i+1.. ; row i+1 <- row i - proj ; row i <- proj ; the last row falls off.
    //   In compact form: proj (topf elements) goes into the slot of the row that falls off, row i - proj
    //   (per elements) replaces row i in place, and the slots are renumbered -- no row moves.
    stage_row = -1;
    if (short_row) {  // the projection wants the tiled row
      expand_row(src, per, rowbuf, N);
      __syncthreads();
    }
    project_lds(rowbuf, buf, N, topf, flags, tb);
    {
      T* dst = rows + (int64_t)s_last * row_stride;  // i == num - 1: the split row itself falls off
      if (i + 1 < num) {
        T* rem = rows + (int64_t)s_here * row_stride;
        for (int k = t; k < per; k += blockDim.x) rem[k] = rowbuf[k] - buf[k];
      }
      for (int k = t; k < topf; k += blockDim.x) dst[k] = buf[k];
    }
    if (tid == 0) {
      for (int r = num - 1; r >= i + 2; --r) {
        norms[r] = norms[r - 1];
        periods[r] = periods[r - 1];
        fa[r] = fa[r - 1];
        fb[r] = fb[r - 1];
        slot[r] = slot[r - 1];
      }
      if (i + 1 < num) {
        norms[i + 1] = last;  // the old row keeps its period, weakened (:582-584)
        periods[i + 1] = (uint32_t)per;
        fa[i + 1] = a;
        fb[i + 1] = b;
        slot[i + 1] = s_here;
      }
      norms[i] = top;
      periods[i] = (uint32_t)topf;
      fa[i] = tb.fac_off[topf];
      fb[i] = tb.fac_off[topf + 1];
      slot[i] = s_last;
    }
    __threadfence_block();
    __syncthreads();
    i = next_row(i);  // the new row i is examined next: i is not advanced (:581-594)
    clk.mark(5);
  }
  __syncthreads();
  flush_rows(num);
  clk.mark(6);
  if (kStep2Timers && (blockIdx.x % PH_STEP2_TIMERS_EVERY) == 5 % PH_STEP2_TIMERS_EVERY && tid == 0)
    printf("step2 wg %d (100 MHz ticks): init %lld stage %lld folds %lld dma+barrier %lld flush+scan %lld split %lld final flush %lld total %lld rows %d splits %d\n",
           (int)blockIdx.x, clk.ticks(0), clk.ticks(1), clk.ticks(2), clk.ticks(3), clk.ticks(4), clk.ticks(5), clk.ticks(6), clk.total(), clk.counted(0), clk.counted(1));
  const double dn = dnorm[w];
  for (int k = tid; k < num; k += blockDim.x) {
    periods_io[w * num + k] = periods[k];
    norms_io[w * num + k] = norms[k] / dn;
  }
}

}  // namespace ph

// QOPeriods: fold sums, tiled sums, the find_periods loops and the orthogonal powers.
#pragma once

#include "ph_device.h"

namespace ph {

// ======================================================================================
// QOPeriods building blocks (QOPeriods.py:779-795): W = A x and A^T w for natural-basis A.
// ======================================================================================
// LDS of k_fold_sums (the staged window) and of k_tile_sum (one window's weights): a single array.
template <typename U>
struct StageLds {
  U* stage;
  size_t bytes;
};
template <typename U, class C>
__host__ __device__ __forceinline__ StageLds<U> stage_carve(C cv, size_t n) {
  StageLds<U> L;
  L.stage = cv.template take<U>(n);
  L.bytes = cv.off;
  return L;
}

template <typename T, bool LW>
__global__ __launch_bounds__(kBlock) void k_fold_sums(const T* __restrict__ x, int N,
                                                      const int* __restrict__ p_list,
                                                      const int* __restrict__ keep,
                                                      const int* __restrict__ row_off, int n_p, int stride,
                                                      double* __restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int64_t w = blockIdx.x;
  const T* xs = x + w * (int64_t)N;  // LW == false: a window longer than the LDS is folded straight from HBM / L2
  if constexpr (LW) {
    T* stage = stage_carve<T>(Carve(smem), N).stage;
    load_window(xs, stage, N);
    __syncthreads();
    xs = stage;
  }
  double* orow = out + w * (int64_t)stride;
  for (int k = 0; k < n_p; ++k) {
    const int p = p_list[k];
    const Fold f(N, p);
    for (int j = threadIdx.x; j < keep[k]; j += blockDim.x)
      orow[row_off[k] + j] = (double)column_sum(xs, j, p, f.count(j));
  }
}

template <typename T>
__global__ __launch_bounds__(kBlock) void k_tile_sum(const double* __restrict__ wts, int N,
                                                     const int* __restrict__ p_list,
                                                     const int* __restrict__ keep,
                                                     const int* __restrict__ row_off, int n_p, int stride,
                                                     T* __restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  double* ws = stage_carve<double>(Carve(smem), stride).stage;
  const int64_t w = blockIdx.x;
  for (int i = threadIdx.x; i < stride; i += blockDim.x) ws[i] = wts[w * (int64_t)stride + i];
  __syncthreads();
  for (int n = threadIdx.x; n < N; n += blockDim.x) {
    double acc = 0.0;
    for (int k = 0; k < n_p; ++k) {  // row order of A, like np.matmul(A.T, w) sums over rows
      const int j = n % p_list[k];
      if (j < keep[k]) acc += ws[row_off[k] + j];
    }
    out[w * (int64_t)N + n] = (T)acc;
  }
}

// ======================================================================================
// QOPeriods.find_periods, non-orthogonal / update_weights=True branch (QOPeriods.py:373-596
// with :468-478, :510-522, :560-594; get_subspaces :830-840; solve_quadratic :779-796), the
// whole greedy loop on the device.  One workgroup per window.  Per iteration:
//   gamma-normalised all-p sweep of the residual (pass plan)  -> strongest period
//   rows kept for it = Euler-phi mass its divisors add to the running divisor set
//   right-hand side A x extended by the fold of the data over the new rows
//   A A^T w = A x by preconditioned conjugate gradients in LDS -- the Gram matrix (integer co-occurrence
//   counts of the indicator rows) is never formed, its rows are regenerated inside the product (qo_offdiag)
//   reconstruction A^T w, residual
// The reference stops when rms(reconstruction) <= rms(data) * thresh (default test_function)
// or when numpy.linalg.solve raises LinAlgError (here: non-positive curvature or a non-finite residual of
// the solve, a period that adds no new rows, or a repeated period -- the cases that make the reference's
// matrix singular).  A solve that has not converged after its iteration bound (an ill-conditioned but
// regular dictionary) ends the window with PH_ST_ITER_CAP: the host loop, which solves as the reference
// does, takes it.  counts[w] = {periods reported, blocks in the dictionary}.
// ======================================================================================
#ifndef PH_QO_OCC
#define PH_QO_OCC __attribute__((amdgpu_waves_per_eu(8, 8)))  // two 16-wave workgroups per CU need <= 64 VGPRs
#endif
constexpr int kQoMaxBlocks = 64;
constexpr int kQoGreedyMaxRows = 1 << 20;  // k_qo_greedy: dictionary rows per window (weights live in HBM only)
constexpr int kQoPairTab = 16;  // dictionaries of up to this many blocks keep their pair constants in LDS

__device__ __forceinline__ int qo_gcd(int a, int b) {
  while (b != 0) {
    const int t = a % b;
    a = b;
    b = t;
  }
  return a;
}

// Off-diagonal part of one row of the Gram matrix A A^T times a vector, WITHOUT the matrix.  Row (a, i) is the
// indicator of n = i (mod p_a); its entry against row (b, j) counts the n < N with n = i (p_a) and n = j (p_b)
// (QOPeriods.py:781).  Along n = i, i + p_a, ... the residue mod p_b advances by p_a mod p_b and returns after
// cycle = p_b / gcd steps, so
//   sum_j G[(a,i),(b,j)] v_b[j] = sum_{t < min(cycle, terms)} count(t) v_b[idx_t],   count(t) = (terms-1-t) / cycle + 1,
// with terms = samples of residue i.  For N < lcm(p_a, p_b) every count is 1 and the loop is the fold of the tiled
// v_b.  The steps t = t0, t0 + ts, ... are summed (a group of `ts` lanes shares a long row).
__device__ __forceinline__ int qo_wrap(int idx, int pb) {  // idx in [0, 2 pb) -> idx mod pb
  return (int)min((unsigned)idx, (unsigned)(idx - pb));
}

// `vb` points at block b's entries inside a vector in the solver's layout: k_b entries followed by one zero, so an
// index past the kept rows is clamped onto the zero instead of being masked.
__device__ __forceinline__ double qo_offdiag(const double* __restrict__ vb, int kb, int pb, int cycle, int step, int i,
                                             int terms, int t0, int ts) {
  const int lim = cycle < terms ? cycle : terms;
  if (t0 >= lim) return 0.0;
  int idx = (int)(((unsigned)i + (unsigned)t0 * (unsigned)step) % (unsigned)pb);  // i < 2^20, t0 < 16, step < p_b < 2^20
  const int sstep = ts == 1 ? step : (int)(((unsigned)ts * (unsigned)step) % (unsigned)pb);
  if (cycle >= terms) {  // all counts are 1
    double s0 = 0.0, s1 = 0.0;
    int t = t0;
    for (; t + 3 * ts < lim; t += 4 * ts) {
      const int i1 = qo_wrap(idx + sstep, pb), i2 = qo_wrap(i1 + sstep, pb), i3 = qo_wrap(i2 + sstep, pb);
      const double v0 = vb[min(idx, kb)], v1 = vb[min(i1, kb)], v2 = vb[min(i2, kb)], v3 = vb[min(i3, kb)];
      s0 += v0;
      s1 += v1;
      s0 += v2;
      s1 += v3;
      idx = qo_wrap(i3 + sstep, pb);
    }
    for (; t < lim; t += ts) {
      s0 += vb[min(idx, kb)];
      idx = qo_wrap(idx + sstep, pb);
    }
    return s0 + s1;
  }
  const int chi = (terms - 1) / cycle + 1, tsw = (terms - 1) % cycle;
  double shi = 0.0, slo = 0.0;
  for (int t = t0; t < lim; t += ts) {
    const double v = vb[min(idx, kb)];
    if (t <= tsw)
      shi += v;
    else
      slo += v;
    idx = qo_wrap(idx + sstep, pb);
  }
  // (the fused form spelled out: left to the compiler's contraction, which of the two products is rounded on its own
  // depends on the code around the call, and the callers would not agree to the last bit)
  return fma((double)chi, shi, (double)(chi - 1) * slo);
}

// ======================================================================================
// The solver of the normal equations A A^T w = A x, stated once.  k_qo_find, k_qo_fit (ph_fit.h) and k_qo_fit_win call
// it: the first two around the matrix-free product below, k_qo_fit_win around its staged product.
// A dictionary as the product sees it.  Solver layout of a vector: block b's k_b entries start at slot boff[b] + b and
// are followed by one zero (qo_offdiag clamps indices past the kept rows onto it).
// ======================================================================================
struct QoDict {
  const int* bper;   // period of dictionary block b
  const int* bkeep;  // rows kept for it
  const int* boff;   // first row of block b
  const int* ioff;   // first work item of block b
  const int* blg;    // log2 of the lanes that share a row of block b
  const int* ptab;   // (a, b): {p_b / gcd(p_a, p_b), p_a mod p_b}, filled for dictionaries of up to kQoPairTab blocks
  const int* trm;    // per slot: samples of the row's residue
  int nblk;
};

// Work split of the product: a row of block a costs sum_b min(cycle_ab, samples) steps -- the rows of short periods are
// the long ones.  -> the steps of one row of block a.
__device__ __forceinline__ int qo_row_steps(const int* bper, int nblk, int a, int N) {
  const int pa = bper[a], terms = (N - 1) / pa + 1;
  int st = 0;
  for (int b = 0; b < nblk; ++b) {
    if (b == a) continue;
    const int cyc = bper[b] / qo_gcd(pa, bper[b]);
    st += cyc < terms ? cyc : terms;
  }
  return st;
}

// Block a gets L_a = 1, 2, ..., 16 lanes per row (blg = log2 L_a) so that no lane walks more than ~1/1024 of all steps;
// the lanes of a row are neighbours and combine with DPP.  Greedy: give the block with the longest walk twice the lanes
// while all items still fit one round of the workgroup (blocks of periods below 64 always get 16 lanes: their rows have
// up to N / 2 samples).  One thread; `steps` from qo_row_steps.
__device__ __forceinline__ void qo_lane_split(const int* bper, const int* bkeep, const int* steps, int nblk, int* blg,
                                              int* ioff) {
  int items = 0;
  for (int a = 0; a < nblk; ++a) {
    blg[a] = bper[a] < 64 ? 4 : 0;
    items += ((bkeep[a] << blg[a]) + 15) & ~15;
  }
  for (int round = 0; round < 4 * kQoMaxBlocks; ++round) {  // (every round adds one to some blg[a] <= 4)
    int worst = -1, wst = 24;
    for (int a = 0; a < nblk; ++a)
      if (blg[a] < 4 && (steps[a] >> blg[a]) > wst) {
        wst = steps[a] >> blg[a];
        worst = a;
      }
    if (worst < 0) break;
    const int grown = items - (((bkeep[worst] << blg[worst]) + 15) & ~15) + (((bkeep[worst] << (blg[worst] + 1)) + 15) & ~15);
    if (grown > (int)blockDim.x) break;
    items = grown;
    blg[worst] += 1;
  }
  int off = 0;
  for (int a = 0; a < nblk; ++a) {
    ioff[a] = off;
    off += ((bkeep[a] << blg[a]) + 15) & ~15;  // groups never straddle a 16-lane DPP row
  }
  ioff[nblk] = off;
}

// out = A A^T vv.  The Gram matrix (integer co-occurrence counts, QOPeriods.py:781) is never formed: its rows are
// regenerated from the CRT structure inside the product (qo_offdiag), so the solve touches LDS only.  With `dots`, the
// lane that finishes a row also accumulates that row's terms of gamma = (r, z), delta = (w, z) and |r|^2 (vv is z
// then, `rv` the residual), so the three sums need no pass of their own.
__device__ __forceinline__ void qo_gram_apply(const QoDict& D, const double* __restrict__ vv, double* __restrict__ out,
                                              const double* rv, bool dots, double& dg, double& dd, double& dr) {
  const int tid = threadIdx.x, nblk = D.nblk;
  const int nitems = D.ioff[nblk];
  for (int v = tid; v < nitems; v += blockDim.x) {
    int a = 0;
    while (a + 1 < nblk && D.ioff[a + 1] <= v) ++a;
    const int lg = D.blg[a], L = 1 << lg;
    const int e = v - D.ioff[a];
    const int i = e >> lg, gl = e & (L - 1);
    const int ka = D.bkeep[a];
    double acc = 0.0;
    int terms = 1;
    const int sl = D.boff[a] + a + (i < ka ? i : 0);
    if (i < ka) {  // (the padding items of the last row group only take part in the DPP steps)
      const int pa = D.bper[a];
      terms = D.trm[sl];
      for (int b = 0; b < nblk; ++b) {
        if (b == a) continue;
        const int pb = D.bper[b];
        int cycle, step;
        if (nblk <= kQoPairTab) {
          cycle = D.ptab[2 * (a * kQoPairTab + b)];
          step = D.ptab[2 * (a * kQoPairTab + b) + 1];
        } else {
          cycle = pb / qo_gcd(pa, pb);
          step = pa % pb;
        }
        acc += qo_offdiag(vv + D.boff[b] + b, D.bkeep[b], pb, cycle, step, i, terms, gl, L);
      }
    }
    if (lg >= 4) acc += dpp_f64<kDppRor8>(acc);
    if (lg >= 3) acc += dpp_f64<kDppHalfMirror>(acc);
    if (lg >= 2) acc += dpp_f64<kDppXor2>(acc);
    if (lg >= 1) acc += dpp_f64<kDppXor1>(acc);
    if (gl == 0 && i < ka) {
      const double z = vv[sl], wrow = fma((double)terms, z, acc);
      out[sl] = wrow;
      if (dots) {
        const double t = rv[sl];
        dg = fma(t, z, dg);
        dd = fma(wrow, z, dd);
        dr = fma(t, t, dr);
      }
    }
  }
}

// The seven vectors of a solve, kv doubles each in the solver layout.
struct QoCgVectors {
  double* xv;   // weights
  double* rv;   // residual of the normal equations (on entry: the right-hand side)
  double* pv;   // search direction
  double* qv;   // G pv (WARM, on entry: G xv)
  double* zv;   // preconditioned residual
  double* wv_;  // G zv
  double* dv;   // 1 / diagonal (Jacobi preconditioner)
};
struct QoCgResult {
  int iter;        // iterations taken (updates of the weights)
  double rr;       // |r|^2 at the exit
  bool curvature;  // not positive definite: numpy.linalg.solve would raise or return garbage
  bool converged;  // rr <= (tol |A x|)^2; false also when rr is not finite
};

// Jacobi-preconditioned conjugate gradients in the single-reduction form (Chronopoulos / Gear): z = D^-1 r, w = G z, and
// gamma = (r, z), delta = (w, z), |r|^2 come out of ONE workgroup reduction per iteration; p and q = G p follow by
// recurrence.  product(vv, out, dg, dd, dr) writes out = G vv and adds the calling thread's terms of the three sums (vv
// is z then); it may hold barriers of its own, and the rows it does not write (the pad slots) must be zero in qv and
// wv_.  WARM: xv holds earlier weights and qv = G xv, the residual starts as rv - qv; otherwise xv = 0.
// ||r|| <= tol ||A x||: with the condition numbers seen (kappa ~ 3000) the weights are then good to 3e-10 (fp64
// windows, tol 1e-13, bar 1e-8) and 3e-6 (float windows, whose residual is stored as float; tol 1e-9, bar 1e-4).  The
// diagonal blocks are diagonal; with that as preconditioner the spectrum is a cluster at 1 plus a few small
// eigenvalues from the mean / common-divisor directions the blocks share: 20-70 iterations to 1e-13, 4 K + 100 at most.
// The caller classifies what comes back (k_qo_find tells a finite rr at the bound from a singular dictionary).
template <typename T, bool WARM, typename Product>
__device__ __forceinline__ QoCgResult qo_cg(const QoCgVectors& V, int KS, int K, double* red, double* red3,
                                            Product&& product) {
  const int tid = threadIdx.x, lane = tid & (kWave - 1), nw = blockDim.x >> 6;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  double* const xv = V.xv;
  double* const rv = V.rv;
  double* const pv = V.pv;
  double* const qv = V.qv;
  double* const zv = V.zv;
  double* const wv_ = V.wv_;
  const double* const dv = V.dv;
  double bb = 0.0;
  for (int r = tid; r < KS; r += blockDim.x) {
    const double bval = rv[r];
    double t = bval;
    if constexpr (WARM) {
      t = bval - qv[r];
      rv[r] = t;
    }
    zv[r] = t * dv[r];
    bb = fma(bval, bval, bb);
  }
  bb = block_sum(bb, red);  // (its barriers also publish zv)
  const double tol = sizeof(T) == 4 ? 1e-9 : 1e-13;
  const double tol2 = tol * tol * bb;
  const int itmax = 4 * K + 100;
  double gamma_old = 0.0, alpha = 0.0, rr = 1.0 / 0.0;
  bool curvature = false;
  int iter = 0;
  for (;; ++iter) {
    double dg = 0.0, dd = 0.0, dr = 0.0;
    product(zv, wv_, dg, dd, dr);
    // one reduction for the three sums; the partials of odd and even iterations use different slots, so the only
    // barriers of an iteration are the one here and the one behind the vector updates
    double* part = red3 + (iter & 1) * 3 * kMaxWaves;
    const double sg = wave_sum(dg), sd = wave_sum(dd), sr = wave_sum(dr);
    if (lane == 0) {
      part[wv] = sg;
      part[kMaxWaves + wv] = sd;
      part[2 * kMaxWaves + wv] = sr;
    }
    __syncthreads();
    // (all reads in flight before the first addition: the loop over the run-time wave count was 3 x 16 dependent LDS
    // round trips per iteration)
    const double g = uniform_f64(red_combine(part, nw)), d = uniform_f64(red_combine(part + kMaxWaves, nw));
    rr = uniform_f64(red_combine(part + 2 * kMaxWaves, nw));
    if (rr <= tol2 || iter >= itmax) break;
    const double beta = iter == 0 ? 0.0 : g / gamma_old;
    const double denom = iter == 0 ? d : d - beta * g / alpha;
    if (!(denom > 0.0) || !(g > 0.0)) {
      curvature = true;
      break;
    }
    alpha = g / denom;
    gamma_old = g;
    for (int r = tid; r < KS; r += blockDim.x) {
      const double pn = fma(beta, iter == 0 ? 0.0 : pv[r], zv[r]);
      const double qn = fma(beta, iter == 0 ? 0.0 : qv[r], wv_[r]);
      pv[r] = pn;
      qv[r] = qn;
      xv[r] = fma(alpha, pn, xv[r]);
      const double t = fma(-alpha, qn, rv[r]);
      rv[r] = t;
      zv[r] = t * dv[r];
    }
    __syncthreads();
  }
  return {iter, rr, curvature, rr <= tol2};
}

// TRUNC (trunc_to_integer_multiple): only the selection changes -- the gamma norm of the trunc projection
// (wave_sweep_trunc); the solve ignores trunc like the reference's _update_weights.  The plain instantiations compile
// to the code they had before the parameter existed (everything TRUNC touches is `if constexpr`).
// LDS of k_qo_find: the residual window (when it lives in LDS), bookkeeping, the pair table, the weights, and the six
// work vectors + sample counts of the conjugate-gradient solve (one slot per dictionary row and one per block: block
// b's k_b entries start at slot boff[b] + b and are followed by one zero, qo_offdiag clamps indices past the kept rows
// onto it).  The work vectors only live during a solve, when the residual window is dead (it is rebuilt from the data
// and the reconstruction afterwards): with `overlay` they lie over the window buffer, which leaves room for a second
// workgroup on the CU; otherwise they sit behind the weights.
template <typename T>
struct QoFindLds {
  T* work;
  double* red;
  double* wbest;
  int* wbestp;
  int* bper;       // period of dictionary block b
  int* bkeep;      // rows kept for it
  int* boff;       // first row of block b
  double* bnorm;
  uint32_t* seen;  // running divisor set R (QOPeriods.py:832-835)
  int* ptab;       // (a, b): {p_b / gcd(p_a, p_b), p_a mod p_b}
  double* red3;    // wave partials of the solver's fused reduction (two parities)
  int* blg;        // log2 of the lanes that share a row of block b in the product
  int* ioff;       // first work item of block b
  QoCgVectors v;   // xv persists: earlier rows start from their last values; dv = 1 / samples of the row's residue
  int* trm;        // samples of the row's residue
  size_t window;   // bytes of the window piece (0: it lives in HBM) and of the work vectors: the host's overlay rule
  size_t solver;
  size_t bytes;
};
template <typename T, class C>
__host__ __device__ __forceinline__ QoFindLds<T> qo_find_carve(C cv, int N, int p_hi, int kcap, bool lw, bool overlay) {
  QoFindLds<T> L;
  L.work = lw ? cv.template take<T>(N + kPad) : nullptr;
  L.window = cv.off;
  L.red = cv.template take<double>(kRedDoubles);
  L.wbest = cv.template take<double>(kMaxWaves);
  L.wbestp = cv.template take<int>(kMaxWaves);
  L.bper = cv.template take<int>(kQoMaxBlocks);
  L.bkeep = cv.template take<int>(kQoMaxBlocks);
  L.boff = cv.template take<int>(kQoMaxBlocks + 1);
  L.bnorm = cv.template take<double>(kQoMaxBlocks);
  L.seen = cv.template take<uint32_t>((p_hi + 32) / 32);
  L.ptab = cv.template take<int>(2 * kQoPairTab * kQoPairTab);
  L.red3 = cv.template take<double>(6 * kMaxWaves);
  L.blg = cv.template take<int>(kQoMaxBlocks);
  L.ioff = cv.template take<int>(kQoMaxBlocks + 1);
  const int kv = kcap + kQoMaxBlocks;
  L.v.xv = cv.template take<double>(kv);
  C sv = cv.at(overlay ? 0 : cv.off);
  const size_t sv0 = sv.off;
  L.v.rv = sv.template take<double>(kv);
  L.v.pv = sv.template take<double>(kv);
  L.v.qv = sv.template take<double>(kv);
  L.v.zv = sv.template take<double>(kv);
  L.v.wv_ = sv.template take<double>(kv);
  L.v.dv = sv.template take<double>(kv);
  L.trm = sv.template take<int>(kv);
  L.solver = sv.off - sv0;
  L.bytes = cv.off > sv.off ? cv.off : sv.off;
  return L;
}

template <typename T, bool LW, bool TRUNC = false>
__global__ __launch_bounds__(1024) PH_QO_OCC void k_qo_find(const T* __restrict__ x, int N, int num, double thresh,
                                                        int p_lo, int p_hi, const PGeom* __restrict__ geom,
                                                        const PassPlan* __restrict__ plan, int n_pass,
                                                        const int* __restrict__ phi, const int* __restrict__ div_off,
                                                        const int* __restrict__ div_q, int kcap, int overlay, T* gwin,
                                                        double* __restrict__ ws_all, uint32_t* __restrict__ periods_out,
                                                        double* __restrict__ norms_out, int* __restrict__ keeps_out,
                                                        int* __restrict__ counts_out, double* __restrict__ weights_out,
                                                        T* __restrict__ resid_out, int* __restrict__ status_out) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const QoFindLds<T> L = qo_find_carve<T>(Carve(smem), N, p_hi, kcap, LW, LW && overlay);
  // the residual: LDS, or (LW == false: windows that leave no room for the solver's vectors) the HBM workspace
  T* work = window_buf<T, LW>(L.work, gwin, N + kPad);
  double *red = L.red, *wbest = L.wbest, *bnorm = L.bnorm, *red3 = L.red3;
  int *wbestp = L.wbestp, *bper = L.bper, *bkeep = L.bkeep, *boff = L.boff, *ptab = L.ptab, *blg = L.blg;
  int* ioff = L.ioff;
  uint32_t* seen = L.seen;
  double *xv = L.v.xv, *rv = L.v.rv, *pv = L.v.pv, *qv = L.v.qv, *zv = L.v.zv, *wv_ = L.v.wv_, *dv = L.v.dv;
  int* trm = L.trm;

  const int64_t w = blockIdx.x;
  const int tid = threadIdx.x;
  const int lane = tid & (kWave - 1);
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int nw = blockDim.x >> 6;
  const T* data = x + w * (int64_t)N;
  double* wts = ws_all + w * 2 * (int64_t)kcap;  // last good weights (row order)
  double* rhs = wts + kcap;                      // A x of the rows found so far

  load_window(data, work, N);
  zero_pad(work, N);
  for (int k = tid; k < (p_hi + 32) / 32; k += blockDim.x) seen[k] = 0u;
  if (tid == 0) boff[0] = 0;
  __syncthreads();
  const double data_sq = block_sumsq(work, N, red);
  double recon_sq = 0.0;
  int nb = 0;        // blocks in the dictionary
  int status = 0;
  bool stopped_by_test = false;

  StageClock<kQoTimers, 4> clk;  // stages: sweep, rhs, cg, recon; counter: cg iterations
  for (int it = 0; it < num; ++it) {
    if (it > 0 && !(sqrt(recon_sq / N) > sqrt(data_sq / N) * thresh)) {  // QOPeriods.py:391,418
      stopped_by_test = true;
      break;
    }
    if (nb >= kQoMaxBlocks) {
      status = 3;
      break;
    }
    // ---- strongest gamma-normalised projection of the residual (QOPeriods.py:470-478)
    double best = 0.0;
    int bestp = 0;
    double best_ss = 0.0;  // same lazy comparison as in k_mbest_step1 (gamma norm: ss / p)
    auto consider = [&](double ss, int p) {
      if (!(ss > 0.0)) return;
      bool take = bestp == 0;
      if (!take) {
        const double lhs = ss * (double)bestp, rhs = best_ss * (double)p;
        if (lhs > rhs * (1.0 + 1e-14)) {
          take = true;
        } else if (lhs >= rhs * (1.0 - 1e-14)) {
          const double vn = periodic_norm_from_sq(ss, N, p), vb = periodic_norm_from_sq(best_ss, N, bestp);
          take = vn > vb || (vn == vb && p < bestp);
        }
      }
      if (take) {
        best_ss = ss;
        bestp = p;
      }
    };
    if constexpr (TRUNC)
      wave_sweep_trunc(work, N, p_lo, p_hi, wv, nw, lane, consider);
    else
      wave_sweep_plan<T, LW>(work, N, geom, plan, wv, n_pass, nw, lane, consider);
    best = bestp != 0 ? periodic_norm_from_sq(best_ss, N, bestp) : 0.0;
    if (!(best > 0.0)) bestp = 0;
    wave_argmax(best, bestp);
    if (lane == 0) {
      wbest[wv] = best;
      wbestp[wv] = bestp;
    }
    __syncthreads();
    red_argmax(wbest, wbestp, nw, best, bestp);
    __syncthreads();
    clk.mark(0);
    if (bestp == 0) {  // nothing left to explain; the reference keeps looping on zeros
      if constexpr (TRUNC) status = 1;  // (PH_ST_NO_PERIOD: not mirrored for trunc, the host loop takes the window)
      break;
    }
    // ---- rows this period contributes (QOPeriods.py:833-840); a repeated period or one whose
    //      divisors are all present adds none and makes the reference's matrix singular
    int keep = 0;
    for (int k = div_off[bestp]; k < div_off[bestp + 1]; ++k) {
      const int r = div_q[k];
      if (!((seen[r >> 5] >> (r & 31)) & 1u)) keep += phi[r];
    }
    bool repeated = false;
    for (int b = 0; b < nb; ++b) repeated |= (bper[b] == bestp);
    __syncthreads();
    const int row0 = boff[nb];
    if (keep == 0 || repeated) break;  // LinAlgError path (QOPeriods.py:552-559)
    if (row0 + keep > kcap) {
      status = 3;
      break;
    }
    if (tid == 0) {
      for (int k = div_off[bestp]; k < div_off[bestp + 1]; ++k) seen[div_q[k] >> 5] |= 1u << (div_q[k] & 31);
      bper[nb] = bestp;
      bkeep[nb] = keep;
      boff[nb + 1] = row0 + keep;
      bnorm[nb] = best;
    }
    // pair constants of the new block against every block (and itself: unused)
    if (nb < kQoPairTab) {
      for (int e = tid; e < nb; e += blockDim.x) {
        const int pe = bper[e], g = qo_gcd(pe, bestp);
        ptab[2 * (e * kQoPairTab + nb)] = bestp / g;  // row in block e against block nb
        ptab[2 * (e * kQoPairTab + nb) + 1] = pe % bestp;
        ptab[2 * (nb * kQoPairTab + e)] = pe / g;
        ptab[2 * (nb * kQoPairTab + e) + 1] = bestp % pe;
      }
    }
    // right-hand side rows of the new block: fold of the data (QOPeriods.py:782), one wavefront per residue (a
    // small period has few residues with many samples each)
    for (int j = wv; j < keep; j += nw) {
      const int terms = (N - 1 - j) / bestp + 1;
      double sj = 0.0;
      for (int r = lane; r < terms; r += kWave) sj += (double)data[j + (int64_t)r * bestp];
      sj = wave_sum(sj);
      if (lane == 0) rhs[row0 + j] = sj;
    }
    __threadfence_block();
    __syncthreads();
    clk.mark(1);
    const int K = row0 + keep;
    const int nblk = nb + 1;
    const int KS = K + nblk;  // slots
    // the window buffer is dead from here to the reconstruction: set the solver's vectors up in it
    for (int sl = tid; sl < KS; sl += blockDim.x) {
      int a = 0;
      while (a + 1 < nblk && boff[a + 1] + a + 1 <= sl) ++a;
      const int i = sl - boff[a] - a;
      const bool pad = i >= bkeep[a];  // the zero behind block a
      const int r = boff[a] + i;
      const int terms = pad ? 1 : (N - 1 - i) / bper[a] + 1;
      trm[sl] = terms;
      dv[sl] = pad ? 0.0 : 1.0 / (double)terms;
      rv[sl] = pad ? 0.0 : rhs[r];  // the right-hand side, until the first product turns it into the residual
      wv_[sl] = 0.0;  // (the product never writes the pad slots)
      qv[sl] = 0.0;
      if (pad || r >= row0) xv[sl] = 0.0;  // the rows of earlier steps start from their last weights
    }
    // work split of the product (qo_row_steps, qo_lane_split)
    if (tid == 0) {
      int steps[kQoMaxBlocks];
      for (int a = 0; a < nblk; ++a) steps[a] = qo_row_steps(bper, nblk, a, N);
      qo_lane_split(bper, bkeep, steps, nblk, blg, ioff);
    }
    __syncthreads();
    // ---- A A^T w = A x by preconditioned conjugate gradients (qo_cg around qo_gram_apply), in LDS only -- a dense
    //      factorisation of the K x K matrix (K up to ~900, 5 MB) streamed it through HBM K / 32 times.  The rows of
    //      earlier steps start from their last weights, so the residual starts as A x - G xv.
    const QoDict dict{bper, bkeep, boff, ioff, blg, ptab, trm, nblk};
    bool singular = false;
    {
      double none = 0.0;
      qo_gram_apply(dict, xv, qv, rv, false, none, none, none);
      __syncthreads();
      const QoCgResult cg = qo_cg<T, true>(QoCgVectors{xv, rv, pv, qv, zv, wv_, dv}, KS, K, red, red3,
                                           [&](const double* __restrict__ vv, double* __restrict__ out, double& dg,
                                               double& dd, double& dr) { qo_gram_apply(dict, vv, out, rv, true, dg, dd, dr); });
      singular = cg.curvature;
      if (!cg.converged) {
        // no convergence: a residual that is not finite means a singular dictionary; a finite one after the bound of
        // positive-curvature steps is an ill-conditioned but regular one, which numpy.linalg.solve still solves --
        // PH_ST_ITER_CAP hands the window to the host loop
        singular = true;
        if (cg.rr < 1.0 / 0.0 && status == 0) status = 2;
      }
      clk.count(0, cg.iter);
    }
    clk.mark(2);
    __syncthreads();
    if (singular) {
      // go back one iteration and stop (QOPeriods.py:552-559): the weights return to the last good solve, and the
      // residual -- the solver's vectors may have overwritten the window -- is rebuilt from them below
      for (int r = tid; r < row0; r += blockDim.x) {
        int a = 0;
        while (a + 1 < nb && boff[a + 1] <= r) ++a;
        xv[r + a] = wts[r];
      }
    } else {
      nb += 1;
      for (int r = tid; r < K; r += blockDim.x) {
        int a = 0;
        while (a + 1 < nb && boff[a + 1] <= r) ++a;
        wts[r] = xv[r + a];
      }
    }
    __syncthreads();
    // ---- reconstruction A^T w (QOPeriods.py:795) and the new residual
    double rs = 0.0;
    for (int n = tid; n < N; n += blockDim.x) {
      double rec = 0.0;
      for (int b = 0; b < nb; ++b) {
        const int i = n % bper[b];
        if (i < bkeep[b]) rec += xv[boff[b] + b + i];
      }
      rs += rec * rec;
      work[n] = (T)((double)data[n] - rec);
    }
    if (LW) zero_pad(work, N);
    recon_sq = block_sum(rs, red);
    __syncthreads();
    clk.mark(3);
    if (singular) break;
  }
  __syncthreads();
  if (kQoTimers && w < 12 && tid == 0)
    printf("qo timers (100 MHz ticks) sweep %lld rhs %lld cg %lld recon %lld  cg iterations %d K=%d nb=%d\n", clk.ticks(0), clk.ticks(1),
           clk.ticks(2), clk.ticks(3), clk.counted(0), boff[nb], nb);
  // outputs.  When the loop stopped on the test function the reference reports all periods
  // but the last one, yet keeps the weights / dictionary of all of them (QOPeriods.py:584-592).
  const int n_report = stopped_by_test ? nb - 1 : nb;
  for (int b = tid; b < num; b += blockDim.x) {
    const bool in = b < nb;
    periods_out[w * num + b] = in ? (uint32_t)bper[b] : 0u;
    norms_out[w * num + b] = in ? bnorm[b] : 0.0;
    keeps_out[w * num + b] = in ? bkeep[b] : 0;
  }
  const int Kf = boff[nb];
  for (int r = tid; r < kcap; r += blockDim.x) weights_out[w * (int64_t)kcap + r] = r < Kf ? wts[r] : 0.0;
  for (int n = tid; n < N; n += blockDim.x) resid_out[w * (int64_t)N + n] = work[n];
  if (tid == 0) {
    counts_out[2 * w] = n_report < 0 ? 0 : n_report;
    counts_out[2 * w + 1] = nb;
    status_out[w] = status;
  }
}

// ======================================================================================
// QOPeriods.find_periods with update_weights=False (QOPeriods.py:645-714 as the host loop of
// pyperiod_amd/QOPeriods.py runs it), the whole greedy loop on the device.  One workgroup per window.
// Each new block is fitted ALONE to the running residual; its rows are disjoint residue classes, so
// A A^T is diagonal and the fit is a set of residue means -- no solve, no Gram table.  Per step:
//   gamma sweep of the residual (plain pass plan, or the trunc sweep)    -> strongest period p
//   keep = phi mass of the divisors of p that divide no earlier period (_dont_update_weights)
//   rows = keep, or all p rows when keep == 0 (`matrix[:keep] if keep else matrix`: a period that
//     repeats or divides earlier ones)
//   weights = residue means of the residual over those rows; residual -= tiled means
//   stop test rms(block reconstruction) > rms(data) * thresh from sum_j count_j w_j^2
// When the test fails the last period's block is fitted once more to the current residual and
// appended (the residual is left as it was) and one period fewer is reported (QOPeriods.py:163-169).
// A selection without a positive norm ends with PH_ST_NO_PERIOD (the host loop re-selects the last
// period there), more rows than kcap with PH_ST_CAP: the caller re-runs such windows on the host.
//
// WIN: the fit under one analysis window `win` of N doubles (solve_quadratic(res, A, window=win), QOPeriods.py:779-796,
// as _dont_update_weights calls it).  A diag(win) A^T of one natural-basis block is diag(den), so
//   w_j = num_j / den_j,  num_j = sum win[n] res[n],  den_j = sum win[n]  over n = j (mod p),
// both sums in double from one traversal of the class in the order of the unwindowed fit.  The reconstruction A^T w
// is not windowed: the stop test and the residual update are those of WIN = false.  A class with den_j == 0 (the
// reference's matrix is singular there) or a sum that is not finite ends the window with PH_ST_ITER_CAP.  The window
// is read through L2 (once per round; the sweep reads the residual hundreds of times) and takes no LDS.
// ======================================================================================
// num / den of residue j over `n` rows, row order, eight loads of each array ahead of their adds (column_sum's shape).
template <typename T>
__device__ __forceinline__ void window_class_sums(const T* __restrict__ xs, const double* __restrict__ win, int j, int p,
                                                  int n, double& num, double& den) {
  double sn = 0.0, sd = 0.0;
  int64_t i = j;
  int r = 0;
  for (; r + 8 <= n; r += 8) {
    double v[8], g[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      g[u] = win[i + (int64_t)u * p];
      v[u] = (double)xs[i + (int64_t)u * p];
    }
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      sn += g[u] * v[u];
      sd += g[u];
    }
    i += 8 * (int64_t)p;
  }
  for (; r < n; ++r) {
    const double g = win[i];
    sn += g * (double)xs[i];
    sd += g;
    i += p;
  }
  num = sn;
  den = sd;
}

// A windowed class that cannot be fitted: den == 0, or a sum that is NaN or infinite.
__device__ __forceinline__ bool window_class_bad(double num, double den) {
  return den == 0.0 || !(fabs(den) <= 1.7976931348623157e308) || !(fabs(num) <= 1.7976931348623157e308);
}

template <typename T>
struct QoGreedyLds {
  T* work;
  double* red;
  double* wbest;
  int* wbestp;
  size_t bytes;
};
template <typename T, class C>
__host__ __device__ __forceinline__ QoGreedyLds<T> qo_greedy_carve(C cv, int N, bool lw) {
  QoGreedyLds<T> L;
  L.work = lw ? cv.template take<T>(N + kPad) : nullptr;
  L.red = cv.template take<double>(kRedDoubles);
  L.wbest = cv.template take<double>(kMaxWaves);
  L.wbestp = cv.template take<int>(kMaxWaves);
  L.bytes = cv.off;
  return L;
}

template <typename T, bool LW, bool TRUNC, bool WIN = false>
__global__ __launch_bounds__(1024) void k_qo_greedy(const T* __restrict__ x, int N, int num, double thresh, int p_lo,
                                                    int p_hi, const PGeom* __restrict__ geom,
                                                    const PassPlan* __restrict__ plan, int n_pass,
                                                    const int* __restrict__ phi, const int* __restrict__ div_off,
                                                    const int* __restrict__ div_q, int kcap, T* gwin,
                                                    uint32_t* __restrict__ seen_ws, uint32_t* __restrict__ periods_out, double* __restrict__ norms_out,
                                                    int* __restrict__ keeps_out, int* __restrict__ counts_out,
                                                    double* __restrict__ weights_out, T* __restrict__ resid_out,
                                                    int* __restrict__ status_out, const double* __restrict__ win) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const QoGreedyLds<T> L = qo_greedy_carve<T>(Carve(smem), N, LW);
  T* work = window_buf<T, LW>(L.work, gwin, N + kPad);  // the running residual
  double *red = L.red, *wbest = L.wbest;
  int* wbestp = L.wbestp;
  // Nothing else lives in LDS, so no N or max_length is too large: the divisors of the periods found so far are a
  // bitset in the HBM workspace, the weights of the block being fitted go straight to the output row.

  const int64_t w = blockIdx.x;
  const int tid = threadIdx.x;
  const int lane = tid & (kWave - 1);
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int nw = blockDim.x >> 6;
  double* wout = weights_out + w * (int64_t)kcap;
  uint32_t* seen = seen_ws + w * (int64_t)((p_hi + 32) / 32);

  load_window(x + w * (int64_t)N, work, N);
  zero_pad(work, N);
  for (int k = tid; k < (p_hi + 32) / 32; k += blockDim.x) seen[k] = 0u;
  __syncthreads();
  const double data_sq = block_sumsq(work, N, red);
  double recon_sq = 0.0;
  int nb = 0, row0 = 0, status = 0;
  int lastp = 0, lastkeep = 0;
  double lastnorm = 0.0;
  bool stopped_by_test = false;
  for (int it = 0; it < num; ++it) {
    int p, keep;
    double nrm;
    if (it > 0 && !(sqrt(recon_sq / N) > sqrt(data_sq / N) * thresh)) {  // QOPeriods.py:391,418
      stopped_by_test = true;  // re-fit of the last period's block (its keep is unchanged: same earlier periods)
      p = lastp;
      keep = lastkeep;
      nrm = lastnorm;
    } else {
      // ---- strongest gamma-normalised projection of the residual, first maximum (QOPeriods.py:470-478)
      double best_ss = 0.0;
      int bestp = 0;
      auto consider = [&](double ss, int q) {
        if (!(ss > 0.0)) return;
        bool take = bestp == 0;
        if (!take) {
          const double lhs = ss * (double)bestp, rhs = best_ss * (double)q;
          if (lhs > rhs * (1.0 + 1e-14)) {
            take = true;
          } else if (lhs >= rhs * (1.0 - 1e-14)) {
            const double vn = periodic_norm_from_sq(ss, N, q), vb = periodic_norm_from_sq(best_ss, N, bestp);
            take = vn > vb || (vn == vb && q < bestp);
          }
        }
        if (take) {
          best_ss = ss;
          bestp = q;
        }
      };
      if constexpr (TRUNC)
        wave_sweep_trunc(work, N, p_lo, p_hi, wv, nw, lane, consider);
      else
        wave_sweep_plan<T, LW>(work, N, geom, plan, wv, n_pass, nw, lane, consider);
      double best = bestp != 0 ? periodic_norm_from_sq(best_ss, N, bestp) : 0.0;
      if (!(best > 0.0)) bestp = 0;
      wave_argmax(best, bestp);
      if (lane == 0) {
        wbest[wv] = best;
        wbestp[wv] = bestp;
      }
      __syncthreads();
      red_argmax(wbest, wbestp, nw, best, bestp);
      if (bestp == 0 || bestp > N) {  // no positive norm (or residues without samples): not mirrored here
        status = 1;
        break;
      }
      // ---- rows of the new block: phi mass of its divisors that divide no earlier period (QOPeriods.py:244-260)
      keep = 0;
      for (int k = div_off[bestp]; k < div_off[bestp + 1]; ++k) {
        const int r = div_q[k];
        if (!((seen[r >> 5] >> (r & 31)) & 1u)) keep += phi[r];
      }
      __syncthreads();  // every thread has read `seen` and the wave winners
      if (tid == 0)
        for (int k = div_off[bestp]; k < div_off[bestp + 1]; ++k) seen[div_q[k] >> 5] |= 1u << (div_q[k] & 31);
      p = bestp;
      nrm = best;
    }
    const int rows = keep ? keep : p;  // `matrix[:keep] if keep else matrix` (QOPeriods.py Pp)
    if (row0 + rows > kcap) {
      status = 3;
      break;
    }
    // ---- weights: residue means of the residual (A A^T is diagonal: the samples of each residue)
    const int R = (N + p - 1) / p, nfull = p - (R * p - N);
    if constexpr (WIN) {  // windowed residue means num_j / den_j, same two traversals
      int bad = 0;
      if (R >= 4 * kWave) {
        for (int j = wv; j < rows; j += nw) {
          const int cnt = j < nfull ? R : R - 1;
          double sn = 0.0, sd = 0.0;
          for (int r = lane; r < cnt; r += kWave) {
            const int64_t n = j + (int64_t)r * p;
            const double g = win[n];
            sn += g * (double)work[n];
            sd += g;
          }
          sn = wave_sum(sn);
          sd = wave_sum(sd);
          bad |= window_class_bad(sn, sd);
          if (lane == 0) wout[row0 + j] = sn / sd;
        }
      } else {
        for (int j = tid; j < rows; j += blockDim.x) {
          double sn, sd;
          window_class_sums(work, win, j, p, j < nfull ? R : R - 1, sn, sd);
          bad |= window_class_bad(sn, sd);
          wout[row0 + j] = sn / sd;
        }
      }
      // uniform over the workgroup: every thread leaves together (the rows written above are zeroed at the end)
      if (block_sum((double)bad, red) != 0.0) {
        status = 2;
        break;
      }
    } else if (R >= 4 * kWave) {  // few residues with many samples: one wavefront per residue
      for (int j = wv; j < rows; j += nw) {
        const int cnt = j < nfull ? R : R - 1;
        double sj = 0.0;
        for (int r = lane; r < cnt; r += kWave) sj += (double)work[j + (int64_t)r * p];
        sj = wave_sum(sj);
        if (lane == 0) wout[row0 + j] = sj / (double)cnt;
      }
    } else {  // one thread per residue, rows in order (the fold of ph_fold_sums)
      for (int j = tid; j < rows; j += blockDim.x) {
        const int cnt = j < nfull ? R : R - 1;
        double sj;
        if constexpr (sizeof(T) == 8) {
          sj = column_sum(work, j, p, cnt);
        } else {
          sj = 0.0;
          for (int r = 0; r < cnt; ++r) sj += (double)work[j + r * p];
        }
        wout[row0 + j] = sj / (double)cnt;
      }
    }
    __syncthreads();
    const double* mw = wout + row0;  // (read back through L2 by the other threads of the workgroup)
    double rs = 0.0;
    for (int j = tid; j < rows; j += blockDim.x) {
      const double m = mw[j];
      rs = fma((double)(j < nfull ? R : R - 1) * m, m, rs);
    }
    recon_sq = block_sum(rs, red);
    if (tid == 0) {
      periods_out[w * num + nb] = (uint32_t)p;
      norms_out[w * num + nb] = nrm;
      keeps_out[w * num + nb] = keep;
    }
    nb += 1;
    row0 += rows;
    if (stopped_by_test) break;  // the residual stays the one the test saw
    // ---- residual -= A^T w
    for (int n = tid; n < N; n += blockDim.x) {
      const int j = n % p;
      if (j < rows) work[n] = (T)((double)work[n] - mw[j]);
    }
    __syncthreads();
    lastp = p;
    lastkeep = keep;
    lastnorm = nrm;
  }
  __syncthreads();
  for (int b = nb + tid; b < num; b += blockDim.x) {
    periods_out[w * num + b] = 0u;
    norms_out[w * num + b] = 0.0;
    keeps_out[w * num + b] = 0;
  }
  for (int r = row0 + tid; r < kcap; r += blockDim.x) wout[r] = 0.0;
  for (int n = tid; n < N; n += blockDim.x) resid_out[w * (int64_t)N + n] = work[n];
  if (tid == 0) {
    counts_out[2 * w] = stopped_by_test ? nb - 2 : nb;  // (nb counts the re-fitted block too)
    counts_out[2 * w + 1] = nb;
    status_out[w] = status;
  }
}

// ======================================================================================
// QOPeriods.get_best_period_orthogonal / eq_3 / auto_corr  (QOPeriods.py:1122-1232), the
// Muresan-Parks orthogonal period powers.  One workgroup per window, window and its full
// autocorrelation resident in LDS:
//   r[k]   = sum_{n < N-k} x[n] x[n+k]                                   (auto_corr, :1151-1173)
//   e3[q]  = (q/N) (r[0] + 2 sum_{l=1}^{N//q - 1} r[l q])                 (eq_3, :1122-1149)
//   pows[q] = max(e3[q], 0) - sum_{f | q, f < q} pows[f]                  (:1210-1217)
//           = sum_{d | q} mu(q/d) max(e3[d], 0)   (Moebius inversion of the same recursion),
//   negatives clipped to 0 afterwards, optionally divided by q (:1218-1223).
// ======================================================================================
// The powers of ONE window for the calling workgroup: `xs` is the window (LDS or HBM / L2), `r` (N doubles) and `m`
// (max_p doubles) are its work arrays.  r_out / e3_out are this window's output rows or nullptr; emit(q, pows[q]) is
// called once per q < max_p by the thread that owns q (q = tid, tid + blockDim.x, ...: ascending per thread).  Shared
// by k_orth_powers and k_qo_orth_select (ph_fit.h): same loops, same summation order, same bits.  No barrier at the
// end: `r` is dead on return (its last read lies before the second barrier), `m` is read until the caller's next one.
template <typename T, typename Emit>
__device__ __forceinline__ void orth_powers_row(const T* xs, double* r, double* m, int N, int max_p, int normalize,
                                                const int* __restrict__ mob_off, const int* __restrict__ mob_d,
                                                const int* __restrict__ mob_mu, double* __restrict__ r_out,
                                                double* __restrict__ e3_out, Emit&& emit) {
  const int tid = threadIdx.x;
  // autocorrelation: lags k and N-1-k are paired on one thread (N-k plus k+1 products = N+1)
  for (int k = tid; k < (N + 1) / 2; k += blockDim.x) {
    const int k2 = N - 1 - k;
    double a = 0.0, b = 0.0;
    for (int n = 0; n + k < N; ++n) a += (double)xs[n] * (double)xs[n + k];
    if (k2 != k)
      for (int n = 0; n + k2 < N; ++n) b += (double)xs[n] * (double)xs[n + k2];
    r[k] = a;
    if (k2 != k) r[k2] = b;
  }
  __threadfence_block();
  __syncthreads();
  if (r_out)
    for (int k = tid; k < N; k += blockDim.x) r_out[k] = r[k];
  for (int q = tid; q < max_p; q += blockDim.x) {
    double v = 0.0;
    if (q >= 1) {
      const int M = N / q;
      double second = 0.0;
      for (int l = 1; l < M; ++l) second += r[l * q];
      v = ((double)q / (double)N) * (r[0] + 2.0 * second);
    }
    if (e3_out) e3_out[q] = v;
    m[q] = fmax(v, 0.0);
  }
  __threadfence_block();
  __syncthreads();
  for (int q = tid; q < max_p; q += blockDim.x) {
    double v = 0.0;
    for (int k = mob_off[q]; k < mob_off[q + 1]; ++k) v += (double)mob_mu[k] * m[mob_d[k]];
    v = v < 0.0 ? 0.0 : v;
    if (normalize && q >= 1) v = v / (double)q;
    emit(q, q >= 1 ? v : 0.0);
  }
}

// LDS of k_orth_powers and k_qo_orth_select (ph_fit.h): window, autocorrelation and clipped eq. 3 values when they live
// in LDS (`lw`), then k_qo_orth_select's reduction slots (`select`).
template <typename T>
struct OrthLds {
  T* stage;
  double* r;
  double* m;
  double* red;
  double* wbest;
  int* wbestp;
  size_t bytes;
};
template <typename T, class C>
__host__ __device__ __forceinline__ OrthLds<T> orth_carve(C cv, int N, int max_p, bool lw, bool select) {
  OrthLds<T> L;
  L.stage = lw ? cv.template take<T>(N) : nullptr;
  L.r = lw ? cv.template take<double>(N) : nullptr;
  L.m = lw ? cv.template take<double>(max_p) : nullptr;
  L.red = select ? cv.template take<double>(kRedDoubles) : nullptr;
  L.wbest = select ? cv.template take<double>(kMaxWaves) : nullptr;
  L.wbestp = select ? cv.template take<int>(kMaxWaves) : nullptr;
  L.bytes = cv.off;
  return L;
}

template <typename T, bool LW>
__global__ __launch_bounds__(kBlockWide) void k_orth_powers(const T* __restrict__ x, int N, int max_p, int normalize,
                                                            const int* __restrict__ mob_off,
                                                            const int* __restrict__ mob_d,
                                                            const int* __restrict__ mob_mu,
                                                            double* __restrict__ gws,
                                                            double* __restrict__ r_out, double* __restrict__ e3_out,
                                                            double* __restrict__ pows_out) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int64_t w = blockIdx.x;
  // LW: window, autocorrelation and clipped eq. 3 values live in LDS.  Otherwise (long windows) the
  // window is read straight from HBM / L2 and the two work arrays sit in the HBM workspace `gws`.
  const T* xs = x + w * (int64_t)N;
  double *r, *m;
  if constexpr (LW) {
    const OrthLds<T> L = orth_carve<T>(Carve(smem), N, max_p, true, false);
    r = L.r;
    m = L.m;
    load_window(xs, L.stage, N);
    __syncthreads();
    xs = L.stage;
  } else {
    r = gws + w * ((int64_t)N + max_p);
    m = r + N;
  }
  double* prow = pows_out + w * (int64_t)max_p;
  orth_powers_row(xs, r, m, N, max_p, normalize, mob_off, mob_d, mob_mu, r_out ? r_out + w * (int64_t)N : nullptr,
                  e3_out ? e3_out + w * (int64_t)max_p : nullptr, [&](int q, double v) { prow[q] = v; });
}

}  // namespace ph

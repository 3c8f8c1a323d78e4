// Fit of a GIVEN period list (QOPeriods.compute_reconstruction, RamanujanPeriods.find_periods_with_weights) on the
// device.  k_qo_fit runs get_subspaces' row bookkeeping, the right-hand side by folds and the solver of k_qo_find
// (qo_cg around qo_gram_apply, ph_qo.h) for a list it is handed instead of one it selects greedily.  k_qo_fit_win is
// the same fit under an analysis window: the same carve, prologue, bookkeeping, solver and epilogue around a product
// that goes through a staged sample-length vector.  k_ram_select turns Ramanujan norms into that list; k_ram_select_ref
// does so against a choosable reference level and keeps at most pcap periods.  Then the orthogonal selection step
// (k_qo_orth_select) and QOPeriods.get_periods (k_qo_extract).
// Included by period_hip.hip behind ph_kernels.h.  Reference citations are file:line into /root/reference/pyPeriod/.
#pragma once

#include "ph_kernels.h"

namespace ph {

constexpr int kFitMaxPeriod = 1 << 20;  // qo_offdiag's index arithmetic holds for periods below 2^20
constexpr int kFitCtl = 4;              // control words: status, rows, -, k_qo_fit_win's zero-diagonal flag

// Threads per workgroup: small dictionaries take small workgroups, so that several share a CU.
__host__ __device__ inline int qo_fit_block(int kcap) { return kcap > 512 ? 1024 : kcap > 128 ? 512 : 256; }

// sum over the 16 lanes of a DPP row (every lane of the row gets it)
__device__ __forceinline__ double row16_sum(double v) {
  v += dpp_f64<kDppRor8>(v);
  v += dpp_f64<kDppHalfMirror>(v);
  v += dpp_f64<kDppXor2>(v);
  v += dpp_f64<kDppXor1>(v);
  return v;
}

// ---- What k_qo_fit and k_qo_fit_win share besides the solver: the carve, the prologue, the row bookkeeping, the
//      epilogue.  (k_qo_fit_win leaves blg, bsteps, ptab and trm unused.)
struct QoFitLds {
  double* red;
  double* red3;    // wave partials of the solver's fused reduction (two parities)
  int* bper;       // period of dictionary block b
  int* bkeep;      // rows kept for it
  int* boff;       // first row of block b
  int* ioff;       // first work item of block b (k_qo_fit: of the product; k_qo_fit_win: of the fold)
  int* blg;        // log2 of the lanes that share a row of block b in the product
  int* bsteps;     // steps one row of block b walks in the product
  int* ptab;       // (a, b): {p_b / gcd(p_a, p_b), p_a mod p_b}
  int* ctl;
  uint32_t* seen;  // the divisor bitset (bookkeeping only); the solver's vectors take its place
  QoCgVectors v;   // solver layout; rv starts as the right-hand side (QOPeriods.py:782), dv = 1 / diagonal
  int* trm;        // samples of the row's residue
  double* u;       // k_qo_fit_win: the staging vector of u_len doubles when it lives in LDS
  size_t bytes;
};
// Dynamic LDS of k_qo_fit and k_qo_fit_win, the one statement of its layout (the kernels carve with it, the host counts
// with it).  Bookkeeping, then the solver's seven vectors + the sample counts, one slot per dictionary row and one per
// block.  The divisor bitset over 1 .. max_period is only alive during the row bookkeeping and lies over the vectors,
// so the size depends on kcap alone unless the bitset is the larger of the two.  The window never enters LDS;
// k_qo_fit_win's u sits behind the larger of the two when the host places it in LDS (u_len = N, otherwise 0).
template <class C>
__host__ __device__ __forceinline__ QoFitLds qo_fit_carve(C cv, int kcap, int max_period, size_t u_len = 0) {
  QoFitLds L;
  L.red = cv.template take<double>(kRedDoubles);
  L.red3 = cv.template take<double>(6 * kMaxWaves);
  L.bper = cv.template take<int>(kQoMaxBlocks + 1);
  L.bkeep = cv.template take<int>(kQoMaxBlocks + 1);
  L.boff = cv.template take<int>(kQoMaxBlocks + 1);
  L.ioff = cv.template take<int>(kQoMaxBlocks + 1);
  L.blg = cv.template take<int>(kQoMaxBlocks);
  L.bsteps = cv.template take<int>(kQoMaxBlocks);
  L.ptab = cv.template take<int>(2 * kQoPairTab * kQoPairTab);
  L.ctl = cv.template take<int>(kFitCtl);
  C sn = cv.at(cv.off);
  L.seen = sn.template take<uint32_t>((size_t)(max_period + 32) / 32);
  const int kv = kcap + kQoMaxBlocks;
  L.v.xv = cv.template take<double>(kv);
  L.v.rv = cv.template take<double>(kv);
  L.v.pv = cv.template take<double>(kv);
  L.v.qv = cv.template take<double>(kv);
  L.v.zv = cv.template take<double>(kv);
  L.v.wv_ = cv.template take<double>(kv);
  L.v.dv = cv.template take<double>(kv);
  L.trm = cv.template take<int>(kv);
  C uc = cv.at(cv.off > sn.off ? cv.off : sn.off);
  L.u = u_len ? uc.template take<double>(u_len) : nullptr;
  L.bytes = uc.off;
  return L;
}
__host__ __device__ inline size_t qo_fit_lds_bytes(int kcap, int max_period) {
  return qo_fit_carve(CarveCount(), kcap, max_period).bytes;
}

// The calling workgroup's window: its slices of the arguments.
template <typename T>
struct QoFitWindow {
  const T* data;
  const int* list;  // its period list
  int n_list;
  int* keeps_row;
  double* wout;
  T* resid;
  int* status;
};

// Prologue: the window's slices, zero keeps and weights.  -> status 0, 1 (empty list) or 3 (more entries than pcap or
// kQoMaxBlocks), uniform over the workgroup.
template <typename T>
__device__ __forceinline__ int qo_fit_begin(QoFitWindow<T>& W, const T* __restrict__ x, int N,
                                            const int* __restrict__ periods, const int* __restrict__ n_periods, int pcap,
                                            int per_stride, int kcap, int* __restrict__ keeps_out,
                                            double* __restrict__ weights_out, T* __restrict__ resid_out,
                                            int* __restrict__ status_out) {
  const int64_t w = blockIdx.x;
  const int tid = threadIdx.x;
  W.data = x + w * (int64_t)N;
  W.list = periods + (per_stride ? w * (int64_t)per_stride : 0);
  W.n_list = n_periods[per_stride ? w : 0];
  W.keeps_row = keeps_out + w * (int64_t)pcap;
  W.wout = weights_out + w * (int64_t)kcap;
  W.resid = resid_out + w * (int64_t)N;
  W.status = status_out + w;
  for (int k = tid; k < pcap; k += blockDim.x) W.keeps_row[k] = 0;
  for (int r = tid; r < kcap; r += blockDim.x) W.wout[r] = 0.0;
  int status = 0;
  if (W.n_list <= 0) status = 1;
  if (W.n_list > pcap || W.n_list > kQoMaxBlocks) status = 3;
  return status;
}

// Rows each period contributes (get_subspaces, QOPeriods.py:830-840): one wavefront, the lanes over the divisors.
// Fills bper, bkeep, boff and the window's keeps; ioff becomes the prefix of block_items(p, keep) (k_qo_fit_win's fold
// work items; k_qo_fit's lane split writes ioff afterwards).  -> status 0, 2 or 3 (see k_qo_fit), uniform; K = rows.
// The bitset is dead on return: the vectors may take its place.
template <typename Items>
__device__ __forceinline__ int qo_fit_rows(const QoFitLds& L, const int* __restrict__ list, int n_list, int N,
                                           int max_period, const int* __restrict__ phi, const int* __restrict__ div_off,
                                           const int* __restrict__ div_q, int kcap, int* __restrict__ keeps_row, int& K,
                                           Items&& block_items) {
  const int tid = threadIdx.x, lane = tid & (kWave - 1);
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  uint32_t* const seen = L.seen;
  for (int k = tid; k < (max_period + 32) / 32; k += blockDim.x) seen[k] = 0u;
  __syncthreads();
  if (wv == 0) {
    int st = 0, rows = 0, items = 0;
    for (int b = 0; b < n_list; ++b) {
      const int p = list[b];
      if (p < 1 || p > max_period) {  // (uniform)
        st = 2;
        break;
      }
      const int d0 = div_off[p], d1 = div_off[p + 1];
      double mass = 0.0;
      for (int k = d0 + lane; k < d1; k += kWave) {
        const int r = div_q[k];
        if (!((seen[r >> 5] >> (r & 31)) & 1u)) mass += (double)phi[r];
      }
      const int keep = (int)wave_sum(mass);  // (exact: the mass of all divisors of p is p)
      ram_wave_sync();
      for (int k = d0 + lane; k < d1; k += kWave) {
        const int r = div_q[k];
        atomicOr(&seen[r >> 5], 1u << (r & 31));
      }
      ram_wave_sync();
      if (lane == 0) {
        L.bper[b] = p;
        L.bkeep[b] = keep;
        L.boff[b] = rows;
        L.ioff[b] = items;
        keeps_row[b] = keep;
      }
      if (keep == 0 || keep > N) st = 2;
      rows += keep;  // (<= 64 * 2^20: no overflow)
      items += block_items(p, keep);
    }
    if (st == 0 && rows > N) st = 2;  // more rows than samples: rank of the matrix <= N, singular whatever the blocks are
    if (st == 0 && rows > kcap) st = 3;
    if (lane == 0) {
      L.boff[n_list] = rows;
      L.ioff[n_list] = items;
      L.ctl[0] = st;
      L.ctl[1] = rows;
      L.ctl[3] = 0;
    }
  }
  __syncthreads();
  const int status = L.ctl[0];
  K = L.ctl[1];
  __syncthreads();
  return status;
}

// Epilogue (after the solve; holds the barrier that ends it): a failed solve is status 2 with the zero weights of the
// prologue and no residual; otherwise the weights in row order, the reconstruction A^T w (QOPeriods.py:795, never
// windowed) in row order and the residual x - A^T w in the dtype of x.
template <typename T>
__device__ __forceinline__ void qo_fit_finish(const QoFitLds& L, const QoFitWindow<T>& W, int N, int K, bool failed) {
  const int tid = threadIdx.x, nblk = W.n_list;
  const double* const xv = L.v.xv;
  __syncthreads();
  if (failed) {
    if (tid == 0) *W.status = 2;
    return;
  }
  for (int r = tid; r < K; r += blockDim.x) {
    int a = 0;
    while (a + 1 < nblk && L.boff[a + 1] <= r) ++a;
    W.wout[r] = xv[r + a];
  }
  for (int n = tid; n < N; n += blockDim.x) {
    double rec = 0.0;
    for (int b = 0; b < nblk; ++b) {
      const int i = n % L.bper[b];
      if (i < L.bkeep[b]) rec += xv[L.boff[b] + b + i];
    }
    W.resid[n] = (T)((double)W.data[n] - rec);
  }
  if (tid == 0) *W.status = 0;
}

// ======================================================================================
// QOPeriods.compute_reconstruction / get_subspaces + solve_quadratic for a given period list (QOPeriods.py:807-852,
// :779-796, :1054-1116), natural basis, no analysis window.  One workgroup per window; all solver arithmetic in fp64.
//   rows of block b = Euler-phi mass the divisors of p_b add to the running divisor set (get_subspaces :830-840)
//   right-hand side A x by folds of the window, read from HBM / L2 (the window is read twice: here and for the residual)
//   A A^T w = A x by the solver k_qo_find uses (ph_qo.h: qo_cg around qo_gram_apply with qo_lane_split's work split),
//     started from zero
//   weights in row order, residual x - A^T w
// status: 0 ok; 1 empty list; 3 more entries than pcap or kQoMaxBlocks, or more rows than kcap; 2 a period outside
// 1 .. max_period, a block without rows (repeated period / all divisors present: the reference's Pp(.., keep=0) hands
// back all p rows and its matrix is singular) or with more rows than samples (zero diagonal), a dictionary with more
// rows than samples altogether (rank deficient: conjugate gradients would still converge on it), non-positive curvature, a
// non-finite residual of the solve, or no convergence within 4 K + 100 iterations (the host path solves those as the
// reference does).  Windows that are not ok get zero weights; their residual is not written.  Every loop is bounded;
// nothing waits on anything outside the workgroup.
// ======================================================================================
template <typename T>
__global__ __launch_bounds__(1024) void k_qo_fit(const T* __restrict__ x, int N, const int* __restrict__ periods,
                                                 const int* __restrict__ n_periods, int pcap, int per_stride,
                                                 int max_period, const int* __restrict__ phi,
                                                 const int* __restrict__ div_off, const int* __restrict__ div_q, int kcap,
                                                 int* __restrict__ keeps_out, double* __restrict__ weights_out,
                                                 T* __restrict__ resid_out, int* __restrict__ status_out) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const QoFitLds L = qo_fit_carve(Carve(smem), kcap, max_period);
  int *const bper = L.bper, *const bkeep = L.bkeep, *const boff = L.boff, *const ptab = L.ptab, *const trm = L.trm;
  double* const rv = L.v.rv;
  const int tid = threadIdx.x;
  const int lane = tid & (kWave - 1);
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int nw = blockDim.x >> 6;
  QoFitWindow<T> W;
  int K = 0;
  int status = qo_fit_begin(W, x, N, periods, n_periods, pcap, per_stride, kcap, keeps_out, weights_out, resid_out, status_out);
  if (status == 0)
    status = qo_fit_rows(L, W.list, W.n_list, N, max_period, phi, div_off, div_q, kcap, W.keeps_row, K,
                         [](int, int) { return 0; });
  if (status != 0) {  // (uniform over the workgroup)
    if (tid == 0) *W.status = status;
    return;
  }
  const T* data = W.data;
  const int nblk = W.n_list;
  const int KS = K + nblk;  // slots
  // pair constants of every block against every block (the diagonal is unused)
  if (nblk <= kQoPairTab) {
    for (int e = tid; e < nblk * nblk; e += blockDim.x) {
      const int a = e / nblk, b = e - a * nblk;
      const int pa = bper[a], pb = bper[b];
      ptab[2 * (a * kQoPairTab + b)] = pb / qo_gcd(pa, pb);
      ptab[2 * (a * kQoPairTab + b) + 1] = pa % pb;
    }
  }
  // per slot: samples of the row's residue, the preconditioner, zeros
  for (int sl = tid; sl < KS; sl += blockDim.x) {
    int a = 0;
    while (a + 1 < nblk && boff[a + 1] + a + 1 <= sl) ++a;
    const int i = sl - boff[a] - a;
    const bool pad = i >= bkeep[a];  // the zero behind block a
    const int terms = pad ? 1 : (N - 1 - i) / bper[a] + 1;
    trm[sl] = terms;
    L.v.dv[sl] = pad ? 0.0 : 1.0 / (double)terms;
    L.v.xv[sl] = 0.0;
    rv[sl] = 0.0;
    L.v.zv[sl] = 0.0;  // (the product never writes the pad slots)
    L.v.wv_[sl] = 0.0;
    L.v.qv[sl] = 0.0;
    L.v.pv[sl] = 0.0;
  }
  __syncthreads();
  // ---- right-hand side A x (QOPeriods.py:782): folds of the window.  One wavefront per residue; blocks whose residues
  //      have at most 16 samples take four residues per wavefront, one per DPP row.
  for (int a = 0; a < nblk; ++a) {
    const int p = bper[a], keep = bkeep[a], s0 = boff[a] + a;
    if ((N - 1) / p + 1 > 16) {
      for (int j = wv; j < keep; j += nw) {
        const int terms = (N - 1 - j) / p + 1;
        double sj = 0.0;
        for (int r = lane; r < terms; r += kWave) sj += (double)data[j + (int64_t)r * p];
        sj = wave_sum(sj);
        if (lane == 0) rv[s0 + j] = sj;
      }
    } else {
      const int sub = lane >> 4, l = lane & 15;
      for (int j0 = 4 * wv; j0 < keep; j0 += 4 * nw) {
        const int j = j0 + sub;
        const int64_t n = j + (int64_t)l * p;
        double sj = (j < keep && n < N) ? (double)data[n] : 0.0;
        sj = row16_sum(sj);
        if (l == 0 && j < keep) rv[s0 + j] = sj;
      }
    }
  }
  // work split of the product, the steps across the threads
  for (int a = tid; a < nblk; a += blockDim.x) L.bsteps[a] = qo_row_steps(bper, nblk, a, N);
  __syncthreads();
  if (tid == 0) qo_lane_split(bper, bkeep, L.bsteps, nblk, L.blg, L.ioff);
  __syncthreads();
  // ---- A A^T w = A x from zero
  const QoDict dict{bper, bkeep, boff, L.ioff, L.blg, ptab, trm, nblk};
  const QoCgResult cg = qo_cg<T, false>(L.v, KS, K, L.red, L.red3,
                                        [&](const double* __restrict__ vv, double* __restrict__ out, double& dg, double& dd,
                                            double& dr) { qo_gram_apply(dict, vv, out, rv, true, dg, dd, dr); });
  const bool failed = cg.curvature || !cg.converged;  // (not converged: not finite, or the bound was hit)
  if (kFitTimers && blockIdx.x < 64 && tid == 0) printf("qo_fit window %d: blocks %d rows %d cg iterations %d %s\n", (int)blockIdx.x, nblk, K, cg.iter, failed ? "FAILED" : "ok");
  qo_fit_finish(L, W, N, K, failed);
}

// ======================================================================================
// k_qo_fit_win: k_qo_fit under an analysis window (solve_quadratic(x, A, window=win), QOPeriods.py:779-796):
//   (A diag(win)) A^T w = (A diag(win)) x, reconstruction A^T w and residual x - A^T w unwindowed.
// Dynamic LDS, the one statement of its layout: k_qo_fit's (qo_fit_lds_bytes: bookkeeping, the solver's vectors with the
// divisor bitset overlaying them), then the staging vector u of N doubles when it lives in LDS.  The host places u in
// LDS when that still fits the workgroup's limit and otherwise in an HBM workspace of N doubles per workgroup; win is
// shared by the whole grid and is always read from HBM / L2.
// ======================================================================================
__host__ __device__ inline size_t qo_fit_win_lds_bytes(int N, int kcap, int max_period, bool u_in_lds) {
  return qo_fit_carve(CarveCount(), kcap, max_period, u_in_lds ? N : 0).bytes;
}
// Threads per workgroup: the staging pass is one element of u per thread and step, so long windows take wide workgroups.
__host__ __device__ inline int qo_fit_win_block(int kcap, int N) {
  const int solver = qo_fit_block(kcap), stage = N > 4096 ? 1024 : N > 1024 ? 512 : 256;
  return solver > stage ? solver : stage;
}

// A diag(win) A^T has no closed-form sample counts, so the product goes through u (sample length), matrix-free:
//   stage:  u[n] = win[n] * sum_b v[b, n mod p_b] over the blocks with n mod p_b < keep_b   (win . A^T v)
//   fold:   out[a, i] = sum_r u[i + r p_a]                                                  (A u)
// Both passes put the lanes of a wavefront on consecutive n.  The stage takes four elements of u per thread, a workgroup
// width apart, so that a thread divides once per block and steps the residue from there.  The fold is row r of the
// fold with the lanes over the residues: a block of period >= 64 is cut into 64-residue work items, one fold row per
// step; a block of period p < 64 is one work item that folds 64 / P rows per step (P = p rounded up to a power of two,
// lane = row * P + residue, all p residues folded and keep stored), the rows' lanes then combine by butterfly.  The
// active lanes of either 32-lane half read distinct, adjacent doubles: no LDS bank is hit twice.  The right-hand side
// A (win . x) and the Jacobi diagonal sum_r win[i + r p_a] are the same fold of u = win . x and u = win.
// Status as k_qo_fit; a row whose diagonal is not > 0 ends the window with status 2 (the reference's matrix is then
// singular or indefinite).  ULDS: u is the LDS behind the solver, else ws + blockIdx.x * N.  Every loop is bounded;
// nothing waits on anything outside the workgroup.
template <typename T, bool ULDS>
__global__ __launch_bounds__(1024) void k_qo_fit_win(const T* __restrict__ x, int N, const double* __restrict__ win,
                                                     const int* __restrict__ periods, const int* __restrict__ n_periods,
                                                     int pcap, int per_stride, int max_period,
                                                     const int* __restrict__ phi, const int* __restrict__ div_off,
                                                     const int* __restrict__ div_q, int kcap, double* __restrict__ ws,
                                                     int* __restrict__ keeps_out, double* __restrict__ weights_out,
                                                     T* __restrict__ resid_out, int* __restrict__ status_out) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const QoFitLds L = qo_fit_carve(Carve(smem), kcap, max_period, ULDS ? N : 0);
  int *const bper = L.bper, *const bkeep = L.bkeep, *const boff = L.boff, *const ioff = L.ioff, *const ctl = L.ctl;
  double *const rv = L.v.rv, *const dv = L.v.dv;
  const int tid = threadIdx.x;
  const int lane = tid & (kWave - 1);
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int nw = blockDim.x >> 6;
  double* u;
  if constexpr (ULDS) {
    u = L.u;
  } else {
    u = ws + blockIdx.x * (int64_t)N;
  }
  QoFitWindow<T> W;
  int K = 0;
  int status = qo_fit_begin(W, x, N, periods, n_periods, pcap, per_stride, kcap, keeps_out, weights_out, resid_out, status_out);
  if (status == 0)  // a block's fold work items: one for a period below 64, else one per 64 kept rows
    status = qo_fit_rows(L, W.list, W.n_list, N, max_period, phi, div_off, div_q, kcap, W.keeps_row, K,
                         [](int p, int keep) { return p < kWave ? 1 : (keep + kWave - 1) / kWave; });
  if (status != 0) {  // (uniform over the workgroup)
    if (tid == 0) *W.status = status;
    return;
  }
  const T* data = W.data;
  const int nblk = W.n_list;
  const int KS = K + nblk;  // slots
  for (int sl = tid; sl < KS; sl += blockDim.x) {
    L.v.xv[sl] = 0.0;
    rv[sl] = 0.0;
    L.v.zv[sl] = 0.0;  // (the fold never writes the pad slots)
    L.v.wv_[sl] = 0.0;
    L.v.qv[sl] = 0.0;
    L.v.pv[sl] = 0.0;
    dv[sl] = 0.0;
  }
  // A u: consume(slot, sum_r u[i + r p_a]) for every row; the caller's barrier has published u
  auto fold_u = [&](auto&& consume) {
    const int nitems = ioff[nblk];
    for (int it = wv; it < nitems; it += nw) {
      int a = 0;
      while (a + 1 < nblk && ioff[a + 1] <= it) ++a;
      const int p = bper[a], keep = bkeep[a], s0 = boff[a] + a;
      int lg = 6;  // log2 of the lanes one fold row takes
      if (p < kWave) {
        lg = 0;
        while ((1 << lg) < p) ++lg;
      }
      const int i = p < kWave ? (lane & ((1 << lg) - 1)) : (it - ioff[a]) * kWave + lane;
      const int64_t stride = (int64_t)p << (6 - lg);
      double acc = 0.0;
      if (i < (p < kWave ? p : keep))
        for (int64_t n = i + (int64_t)(lane >> lg) * p; n < N; n += stride) acc += u[n];
      for (int off = 1 << lg; off < kWave; off <<= 1) acc += __shfl_xor(acc, off, kWave);  // (uniform trip count)
      if ((lane >> lg) == 0 && i < keep) consume(s0 + i, acc);
    }
  };
  // ---- Jacobi diagonal: the fold of the window itself
  for (int n = tid; n < N; n += blockDim.x) u[n] = win[n];
  __syncthreads();
  fold_u([&](int sl, double s) {
    if (s > 0.0)
      dv[sl] = 1.0 / s;
    else
      ctl[3] = 1;  // (every writer stores the same value)
  });
  __syncthreads();
  if (ctl[3] != 0) {
    if (tid == 0) *W.status = 2;
    return;
  }
  // ---- right-hand side A (win . x) (QOPeriods.py:781-782)
  for (int n = tid; n < N; n += blockDim.x) u[n] = win[n] * (double)data[n];
  __syncthreads();
  fold_u([&](int sl, double s) { rv[sl] = s; });
  __syncthreads();
  // ---- A diag(win) A^T w = A (win . x) from zero: the shared recurrence around the staged product
  const QoCgResult cg = qo_cg<T, false>(
      L.v, KS, K, L.red, L.red3,
      [&](const double* __restrict__ vv, double* __restrict__ out, double& dg, double& dd, double& dr) {
        for (int base = 0; base < N; base += 4 * (int)blockDim.x) {
          double acc[4] = {0.0, 0.0, 0.0, 0.0};
          for (int b = 0; b < nblk; ++b) {
            const int p = bper[b], keep = bkeep[b], step = (int)blockDim.x % p;
            const double* vb = vv + boff[b] + b;
            int r = (base + tid) % p;
#pragma unroll
            for (int c = 0; c < 4; ++c) {
              if (r < keep) acc[c] += vb[r];
              r += step;
              r -= r >= p ? p : 0;
            }
          }
#pragma unroll
          for (int c = 0; c < 4; ++c) {
            const int n = base + tid + c * (int)blockDim.x;
            if (n < N) u[n] = win[n] * acc[c];
          }
        }
        __syncthreads();
        fold_u([&](int sl, double wrow) {
          const double z = vv[sl];
          out[sl] = wrow;
          const double t = rv[sl];
          dg = fma(t, z, dg);
          dd = fma(wrow, z, dd);
          dr = fma(t, t, dr);
        });
      });
  const bool failed = cg.curvature || !cg.converged;  // (not converged: not finite, or the bound was hit)
  if (kFitTimers && blockIdx.x < 64 && tid == 0) printf("qo_fit_win window %d: blocks %d rows %d cg iterations %d %s\n", (int)blockIdx.x, nblk, K, cg.iter, failed ? "FAILED" : "ok");
  qo_fit_finish(L, W, N, K, failed);
}

// The two passes k_ram_select and k_ram_select_ref share, one wavefront per row.
// The level of a row as numpy.max sees it: |max_q row[q]| over q in 0 .. q_hi, NaN when any entry is NaN.
__device__ __forceinline__ double ram_row_level(const double* __restrict__ row, int q_hi, int lane) {
  double m = -INFINITY;
  int bad = 0;
  for (int q = lane; q <= q_hi; q += kWave) {
    const double v = row[q];
    bad |= v != v;
    m = fmax(m, v);
  }
  m = wave_max(m);
  if (__ballot(bad) != 0ull) m = NAN;
  return fabs(m);
}

// The candidates of a row -- the q in 0 .. q_hi with row[q] / m > thresh -- compacted in ascending q by ballot and
// popcount: prow[pos] = q for the candidates at positions pos < pcap.  -> how many there are (also beyond pcap), the
// same number in every lane.
__device__ __forceinline__ int ram_compact_candidates(const double* __restrict__ row, int q_hi, double m, double thresh,
                                                      int pcap, int lane, int* __restrict__ prow) {
  int count = 0;
  for (int q0 = 0; q0 <= q_hi; q0 += kWave) {
    const int q = q0 + lane;
    const bool sel = q <= q_hi && row[q <= q_hi ? q : 0] / m > thresh;
    const unsigned long long mask = __ballot(sel);
    const int pos = count + __popcll(mask & ((1ull << lane) - 1ull));
    if (sel && pos < pcap) prow[pos] = q;
    count += __popcll(mask);
  }
  return count;
}

// ======================================================================================
// The threshold of RamanujanPeriods.find_periods_with_weights (RamanujanPeriods.py:95-99): one wavefront per window.
// m = |max_q norms[w, q]| over the whole row as numpy.max sees it (a NaN anywhere makes it NaN: ram_row_level), then the
// ascending list of the q with norms[w, q] / m > thresh -- that IEEE double division and strict comparison, so NaN is
// never selected (ram_compact_candidates).  counts[w] = how many there are (also beyond pcap), periods[w, :] the first
// pcap of them.
// ======================================================================================
__global__ __launch_bounds__(kWave) void k_ram_select(const double* __restrict__ norms, int q_hi, double thresh, int pcap,
                                                     int* __restrict__ periods, int* __restrict__ counts) {
  const int64_t w = blockIdx.x;
  const int lane = threadIdx.x;
  const double* row = norms + w * (int64_t)(q_hi + 1);
  const double m = ram_row_level(row, q_hi, lane);
  int* prow = periods + w * (int64_t)pcap;
  const int count = ram_compact_candidates(row, q_hi, m, thresh, pcap, lane, prow);
  for (int k = count + lane; k < pcap; k += kWave) prow[k] = 0;
  if (lane == 0) counts[w] = count;
}

// A double as a 64-bit key with the order of the doubles (NaN aside): a < b <=> ram_key(a) < ram_key(b), and equal keys
// <=> equal bits.  Candidates of k_ram_select_ref are never zero, so equal values have equal keys.
__device__ __forceinline__ unsigned long long ram_key(double v) {
  const unsigned long long b = (unsigned long long)__double_as_longlong(v);
  return b ^ ((b >> 63) ? ~0ull : 0x8000000000000000ull);
}

// ======================================================================================
// k_ram_select against a choosable reference level and with a capped list: one wavefront per window.
//   m          ref[w] when `ref` is given, otherwise k_ram_select's |max| of the row (a NaN anywhere makes it NaN)
//   candidates the q in 0 .. q_hi with norms[w, q] / m > thresh -- k_ram_select's IEEE double division and strict
//              comparison: a NaN entry or quotient is never a candidate, and with thresh > 0 neither is a zero
//   over[w]    how many candidates there are
//   kept       all of them when over[w] <= pcap; otherwise q is kept iff fewer than pcap candidates q' have
//              norms[q'] > norms[q], or norms[q'] == norms[q] and q' < q: the pcap largest, ties to the smaller period
//   counts[w]  min(over[w], pcap); periods[w, :counts[w]] the kept q ascending, zeros behind them
// With ref == nullptr and over[w] <= pcap the lists are k_ram_select's bit for bit: both kernels call ram_row_level and
// ram_compact_candidates.
// A row over the cap finds c, the pcap-th largest candidate, by bisection on the 64 bits of ram_key, most significant
// first -- one strided pass over the row per bit, the row read from global memory / L2 -- and compacts once more:
// everything > c and the first pcap - #{> c} of the entries == c in ascending q.
// ======================================================================================
__global__ __launch_bounds__(kWave) void k_ram_select_ref(const double* __restrict__ norms, int q_hi, double thresh,
                                                         const double* __restrict__ ref, int pcap,
                                                         int* __restrict__ periods, int* __restrict__ counts,
                                                         int* __restrict__ over) {
  const int64_t w = blockIdx.x;
  const int lane = threadIdx.x;
  const double* row = norms + w * (int64_t)(q_hi + 1);
  const double m = ref ? ref[w] : ram_row_level(row, q_hi, lane);
  int* prow = periods + w * (int64_t)pcap;
  const unsigned long long below = (1ull << lane) - 1ull;
  const int count = ram_compact_candidates(row, q_hi, m, thresh, pcap, lane, prow);
  if (lane == 0) {
    over[w] = count;
    counts[w] = count < pcap ? count : pcap;
  }
  if (count <= pcap) {  // (uniform over the wavefront)
    for (int k = count + lane; k < pcap; k += kWave) prow[k] = 0;
    return;
  }
  // ---- over the cap: c = the largest key that at least pcap candidates reach
  unsigned long long c = 0ull;
  for (int bit = 63; bit >= 0; --bit) {
    const unsigned long long trial = c | (1ull << bit);
    int n = 0;
    for (int q0 = 0; q0 <= q_hi; q0 += kWave) {
      const int q = q0 + lane;
      const double v = row[q <= q_hi ? q : 0];
      n += __popcll(__ballot(q <= q_hi && v / m > thresh && ram_key(v) >= trial));
    }
    if (n >= pcap) c = trial;
  }
  int above = 0;
  for (int q0 = 0; q0 <= q_hi; q0 += kWave) {
    const int q = q0 + lane;
    const double v = row[q <= q_hi ? q : 0];
    above += __popcll(__ballot(q <= q_hi && v / m > thresh && ram_key(v) > c));
  }
  const int ties = pcap - above;  // (>= 1: fewer than pcap candidates lie above c)
  __syncthreads();                // the first pass wrote prow from other lanes
  int kept = 0, eq = 0;
  for (int q0 = 0; q0 <= q_hi; q0 += kWave) {
    const int q = q0 + lane;
    const double v = row[q <= q_hi ? q : 0];
    const bool cand = q <= q_hi && v / m > thresh;
    const unsigned long long key = ram_key(v);
    const unsigned long long eqm = __ballot(cand && key == c);
    const bool sel = cand && (key > c || (key == c && eq + __popcll(eqm & below) < ties));
    const unsigned long long mask = __ballot(sel);
    const int pos = kept + __popcll(mask & below);
    if (sel && pos < pcap) prow[pos] = q;
    kept += __popcll(mask);
    eq += __popcll(eqm);
  }
}

// ======================================================================================
// The selection step of QOPeriods.find_periods under orthogonal (Muresan-Parks) selection for a batch of residuals
// (QOPeriods.py:435-448): one workgroup per window does what get_best_period_orthogonal(res, max_p, normalize=True)
// (:1175-1232), Periods.project(res, p, trunc, orthogonalize=True) (Periods.py:142-219) and periodic_norm(base, p)
// (:221-241) do in three calls.
//   powers   orth_powers_row, the body of k_orth_powers: the same bits as ph_orth_powers(normalize = 1) in the same
//            placement, so the argmax is the 1-D path's on every input
//   winner   first maximum over q < max_p; 0 (all powers zero) becomes 1 (:1227-1232); a non-finite power -- or, below,
//            a non-finite norm: a NaN sample clips to zero powers -- ends the window with status 1 (PH_ST_NO_PERIOD),
//            period 0 and norm 0
//   norm     fold -> mean (truncated mean under kTrunc) -> tile into the N doubles that held the autocorrelation (dead
//            once the powers are final), then base -= project(base, p / f) for the sub-periods of the orth tables in
//            their order, then ||base|| / sqrt(N) / sqrt(p)
// All arithmetic is in double whatever T is; the window is only read.  LW: window, work arrays and reductions in LDS
// (orth_carve: k_orth_powers' layout + the reduction slots); otherwise the window is read from HBM / L2
// and the work arrays are N + max_p doubles per workgroup of the workspace `gws`.
// ======================================================================================

// Row-order sum of residue j over n rows of a window of T, in double: column_sum's order for either element type.
template <typename T>
__device__ __forceinline__ double column_sum_f64(const T* __restrict__ xs, int j, int p, int n) {
  if (n <= 0) return 0.0;
  const T* ptr = xs + j;
  double s = (double)ptr[0];
  ptr += p;
  int r = 1;
  for (; r + 8 <= n; r += 8) {
    double v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) v[u] = (double)ptr[u * p];
#pragma unroll
    for (int u = 0; u < 8; ++u) s += v[u];
    ptr += 8 * p;
  }
  for (; r < n; ++r) {
    s += (double)ptr[0];
    ptr += p;
  }
  return s;
}

// dst[n] = mean[n mod p] in double from a window of T (fold_mean_tile with residue_mean's two means).  No barrier.
template <typename T>
__device__ __forceinline__ void fold_mean_tile_f64(const T* __restrict__ src, double* __restrict__ dst, int N, int p,
                                                   bool trunc) {
  const Fold f(N, p);
  for (int j = threadIdx.x; j < p; j += blockDim.x) {
    const int cnt = f.count(j);
    const int n = trunc ? (f.trows < cnt ? f.trows : cnt) : cnt;
    const double m = column_sum_f64(src, j, p, n) / (double)(trunc ? f.trows : cnt);
    for (int r = 0; r < cnt; ++r) dst[r * p + j] = m;
  }
}

template <typename T, bool LW>
__global__ __launch_bounds__(kBlockWide) void k_qo_orth_select(const T* __restrict__ x, int N, int max_p, unsigned flags,
                                                               Tables tb, const int* __restrict__ mob_off,
                                                               const int* __restrict__ mob_d,
                                                               const int* __restrict__ mob_mu, double* __restrict__ gws,
                                                               int* __restrict__ period_out, double* __restrict__ norm_out,
                                                               double* __restrict__ pows_out, int* __restrict__ status_out) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int64_t w = blockIdx.x;
  const int tid = threadIdx.x;
  const int nw = (blockDim.x + kWave - 1) / kWave;
  const OrthLds<T> L = orth_carve<T>(Carve(smem), N, max_p, LW, true);
  const T* xs = x + w * (int64_t)N;
  double *r, *m;
  if constexpr (LW) {
    r = L.r;
    m = L.m;
    load_window(xs, L.stage, N);
    __syncthreads();
    xs = L.stage;
  } else {
    r = gws + w * ((int64_t)N + max_p);
    m = r + N;
  }
  double *red = L.red, *wbest = L.wbest;
  int* wbestp = L.wbestp;

  // ---- powers; each thread keeps the first maximum of its own q (ascending), keyed q + 1 (0 = none)
  double bv = -1.0;
  int bkey = 0, bad = 0;
  double* prow = pows_out ? pows_out + w * (int64_t)max_p : nullptr;
  orth_powers_row(xs, r, m, N, max_p, 1, mob_off, mob_d, mob_mu, nullptr, nullptr, [&](int q, double v) {
    if (prow) prow[q] = v;
    bad |= !(fabs(v) <= 1.7976931348623157e308);  // NaN or infinite
    if (v > bv) {
      bv = v;
      bkey = q + 1;
    }
  });
  wave_argmax(bv, bkey);
  if ((tid & (kWave - 1)) == 0) {
    wbest[tid >> 6] = bv;
    wbestp[tid >> 6] = bkey;
  }
  const double nbad = block_sum((double)bad, red);  // (its barriers also publish the wave winners and retire `m`)
  if (nbad != 0.0) {
    if (tid == 0) {
      period_out[w] = 0;
      norm_out[w] = 0.0;
      status_out[w] = 1;
    }
    return;
  }
  double best;
  int key;
  red_argmax(wbest, wbestp, nw, best, key);  // takes positive values only: all powers zero -> key 0
  const int p = key > 1 ? key - 1 : 1;       // (QOPeriods.py:1227-1232)

  // ---- base = project(row, p, trunc, orthogonalize=True) in the autocorrelation's N doubles, then its norm
  const bool trunc = flags & kTrunc;
  fold_mean_tile_f64(xs, r, N, p, trunc);
  __threadfence_block();
  __syncthreads();
  for (int k = tb.orth_off[p]; k < tb.orth_off[p + 1]; ++k) {
    subtract_projection_inplace(r, N, tb.orth_q[k], trunc);
    __threadfence_block();
    __syncthreads();
  }
  const double ss = block_sumsq(r, N, red);
  const bool finite = ss <= 1.7976931348623157e308;  // (a NaN sample clips to a zero power -- fmax -- and shows here)
  if (tid == 0) {
    period_out[w] = finite ? p : 0;
    norm_out[w] = finite ? periodic_norm_from_sq(ss, N, p) : 0.0;
    status_out[w] = finite ? 0 : 1;
  }
}

// ======================================================================================
// QOPeriods.get_periods (QOPeriods.py:719-741 with concatenate_periods :854-887 and stack_pairwise_gcd_subspaces
// :889-938) for a batch of fitted dictionaries: one workgroup per window, float64 throughout.
//   c       the concatenated segments: segment a holds rows_a weights and p_a - rows_a zeros
//   actual  c - P c, P the orthogonal projector onto the span of the pairwise gcd rows -- what every decomp_type of the
//           reference computes through a different factorisation.  Closed form, nothing is factorised: with M_e(x) the
//           fold-mean of a segment to period e and u_a^d = sum_{e | d} mu(d / e) tile_d(M_e(c_a)) (the part of c_a that is
//           d-periodic and not periodic with a proper divisor of d), for every d that divides at least two periods
//             v = sum_{a : d | p_a} u_a^d / sum_{a : d | p_a} (d / p_a),   actual_a += tile((d / p_a) v - u_a^d).
//           One period alone: the reference's matrix is ones((1, p)), actual = c - mean(c).
// Order of every sum, the same in both placements (equal bits): d ascending; a in list order; e ascending over the
// divisors with mu(d / e) != 0 (the tables of prepare_mobius); a fold of `rows` rows is split over L = 2^k lanes (L depends
// on e, rows and the workgroup width only), lane l adds rows l, l + L, ... in order and the lanes combine by butterfly.
// Working storage, the one statement of its layout (the kernel carves in this order; the host plans with it): c and
// actual, ccap doubles each; u and the running sum, dcap doubles each; the list of shared d, dcap int32 --
// dcap = min(max_period, ccap / 2) bounds the second largest period, hence every shared d and their number.  WL: in LDS
// behind the control words; otherwise one slice per workgroup of the HBM workspace `gws`.  The segment and weight
// offsets (2 (pcap + 1) int32 per window) always live in the HBM workspace `gidx`, so the placement depends on ccap
// and max_period alone.
// status: 0 ok; 1 K <= 0; 3 K > pcap, sum(p) > ccap or sum(rows) > kcap; 2 a period outside 1 .. max_period, rows
// outside 0 .. period, or a period listed twice (2 before 3).  Rows that are not ok are zero.  Every loop is bounded;
// nothing waits on anything outside the workgroup.
// ======================================================================================
constexpr int kExtCtl = 4;  // control words: status, shared d's, second largest period (then: a repeated period), sum of the periods
__host__ __device__ inline int qo_extract_dcap(int ccap, int max_period) {
  const int d = ccap / 2 < max_period ? ccap / 2 : max_period;
  return d < 1 ? 1 : d;
}
struct QoExtractWork {
  double* cin;  // the concatenated input segments
  double* acc;  // the output accumulators
  double* uv;   // u_a^d of the current (d, a)
  double* sv;   // sum_a u_a^d, then v
  int* dl;      // the d shared by at least two periods, ascending
  size_t bytes;
};
template <class C>
__host__ __device__ __forceinline__ QoExtractWork qo_extract_work_carve(C wk, int ccap, int max_period) {
  const int dcap = qo_extract_dcap(ccap, max_period);
  const size_t wk0 = wk.off;
  QoExtractWork L;
  L.cin = wk.template take<double>(ccap);
  L.acc = wk.template take<double>(ccap);
  L.uv = wk.template take<double>(dcap);
  L.sv = wk.template take<double>(dcap);
  L.dl = wk.template take<int>(dcap);
  L.bytes = wk.off - wk0;
  return L;
}
__host__ __device__ inline size_t qo_extract_work_bytes(int ccap, int max_period) {
  return qo_extract_work_carve(CarveCount(), ccap, max_period).bytes;
}
// LDS of k_qo_extract: the control words, then the working storage when it lives there
struct QoExtractLds {
  int* ctl;
  QoExtractWork work;
  size_t bytes;
};
template <class C>
__host__ __device__ __forceinline__ QoExtractLds qo_extract_carve(C cv, int ccap, int max_period, bool work_in_lds) {
  QoExtractLds L;
  L.ctl = cv.template take<int>(kExtCtl);
  L.work = work_in_lds ? qo_extract_work_carve(cv, ccap, max_period) : QoExtractWork{};
  L.bytes = cv.off + L.work.bytes;
  return L;
}
__host__ __device__ inline size_t qo_extract_lds_bytes(int ccap, int max_period, bool work_in_lds) {
  return qo_extract_carve(CarveCount(), ccap, max_period, work_in_lds).bytes;
}

template <bool WL>
__global__ __launch_bounds__(kBlock) void k_qo_extract(const int* __restrict__ periods, const int* __restrict__ rows,
                                                       const int* __restrict__ counts, int pcap,
                                                       const double* __restrict__ weights, int kcap, int max_period, int ccap,
                                                       const int* __restrict__ mob_off, const int* __restrict__ mob_d,
                                                       const int* __restrict__ mob_mu, int* __restrict__ gidx,
                                                       double* __restrict__ gws, double* __restrict__ out,
                                                       int* __restrict__ status_out) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int64_t w = blockIdx.x;
  const int tid = threadIdx.x;
  const int lane = tid & (kWave - 1);
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int nthr = blockDim.x;
  const QoExtractLds L = qo_extract_carve(Carve(smem), ccap, max_period, WL);
  int* ctl = L.ctl;
  // WL == false: the working storage is this workgroup's slice of the HBM workspace, carved the same way
  const QoExtractWork wk = WL ? L.work
                              : qo_extract_work_carve(Carve(reinterpret_cast<unsigned char*>(gws) +
                                                            w * (int64_t)qo_extract_work_bytes(ccap, max_period)),
                                                      ccap, max_period);
  double *cin = wk.cin, *acc = wk.acc, *uv = wk.uv, *sv = wk.sv;
  int* dl = wk.dl;
  int* soff = gidx + w * 2 * ((int64_t)pcap + 1);  // first element of segment a
  int* woff = soff + pcap + 1;                     // first weight of block a
  const int* per = periods + w * (int64_t)pcap;
  const int* rws = rows + w * (int64_t)pcap;
  const double* wrow = weights + w * (int64_t)kcap;
  double* orow = out + w * (int64_t)ccap;
  auto sync = [] {
    __threadfence_block();
    __syncthreads();
  };
  auto leave = [&](int st) {  // (uniform over the workgroup)
    for (int n = tid; n < ccap; n += nthr) orow[n] = 0.0;
    if (tid == 0) status_out[w] = st;
  };

  const int K = counts[w];
  if (K <= 0 || K > pcap) {
    leave(K <= 0 ? 1 : 3);
    return;
  }
  // ---- the lists: ranges, capacities, offsets, the second largest period
  if (tid == 0) {
    int64_t sp = 0, sr = 0;
    int bad = 0, cap = 0, m1 = 0, m2 = 0;
    for (int a = 0; a < K; ++a) {
      const int p = per[a], r = rws[a];
      if (p < 1 || p > max_period || r < 0 || r > p) {
        bad = 1;
        continue;
      }
      if (!cap) {
        soff[a] = (int)sp;
        woff[a] = (int)sr;
      }
      sp += p;  // (<= 2^20 entries of <= 2^20: no overflow)
      sr += r;
      if (sp > ccap || sr > kcap) cap = 1;
      if (p > m1) {
        m2 = m1;
        m1 = p;
      } else if (p > m2) {
        m2 = p;
      }
    }
    ctl[0] = bad ? 2 : cap ? 3 : 0;
    ctl[1] = 0;
    ctl[2] = m2;
    ctl[3] = cap ? 0 : (int)sp;
  }
  sync();
  if (ctl[0] != 0) {
    leave(ctl[0]);
    return;
  }
  const int total = ctl[3];
  // ---- the d that divide at least two periods (all <= the second largest period), repeated periods: one wavefront
  if (K >= 2 && wv == 0) {
    const int dmax = ctl[2];
    int cnt = 0, dup = 0;
    for (int d0 = 1; d0 <= dmax; d0 += kWave) {
      const int d = d0 + lane;
      int nd = 0, ne = 0;
      if (d <= dmax)
        for (int a = 0; a < K; ++a) {
          const int p = per[a];
          nd += p % d == 0;
          ne += p == d;
        }
      dup |= ne >= 2;
      const bool sel = nd >= 2;
      const unsigned long long mask = __ballot(sel);
      if (sel) dl[cnt + __popcll(mask & ((1ull << lane) - 1ull))] = d;  // (fewer than dmax <= dcap entries)
      cnt += __popcll(mask);
    }
    const bool any_dup = __ballot(dup) != 0ull;
    if (lane == 0) {
      ctl[1] = cnt;
      ctl[2] = any_dup ? 1 : 0;  // (only this wavefront read the second largest period there)
    }
  }
  sync();
  if (K >= 2 && ctl[2] != 0) {
    leave(2);
    return;
  }
  // ---- concatenate (QOPeriods.py:879-887)
  for (int a = 0; a < K; ++a) {
    const int p = per[a], r = rws[a], so = soff[a], wo = woff[a];
    for (int j = tid; j < p; j += nthr) {
      const double v = j < r ? wrow[wo + j] : 0.0;
      cin[so + j] = v;
      acc[so + j] = v;
    }
  }
  sync();
  // fold-means of a segment of p doubles to period e: consume(i, mean of ca[i::e]) from one thread per residue
  auto fold_means = [&](const double* __restrict__ ca, int p, int e, auto&& consume) {
    const int nrows = p / e;
    int lg = 0;
    while (lg < 6 && (2 << lg) * e <= nthr && (2 << lg) <= nrows) ++lg;
    const int L = 1 << lg, l = tid & (L - 1), per_pass = nthr >> lg;
    for (int base = 0; base < e; base += per_pass) {  // (uniform trip count)
      const int i = base + (tid >> lg);
      double s = 0.0;
      if (i < e) {
        const double* ptr = ca + i + (int64_t)l * e;
        const int64_t stride = (int64_t)e << lg;
        for (int r = l; r < nrows; r += L) {
          s += *ptr;
          ptr += stride;
        }
      }
      for (int off = 1; off < L; off <<= 1) s += __shfl_xor(s, off, kWave);
      if (i < e && l == 0) consume(i, s / (double)nrows);
    }
  };
  // dst[n] += scale * src[n mod d] for n < p
  auto tile_add = [&](double* __restrict__ dst, const double* __restrict__ src, int p, int d, double scale) {
    int r = tid % d;
    const int step = nthr % d;
    for (int n = tid; n < p; n += nthr) {
      dst[n] = fma(scale, src[r], dst[n]);
      r += step;
      r -= r >= d ? d : 0;
    }
  };
  if (K == 1) {  // ones((1, p)): actual = c - mean(c)
    fold_means(cin, per[0], 1, [&](int, double m) { uv[0] = m; });
    sync();
    tile_add(acc, uv, per[0], 1, -1.0);
  }
  const int nshared = K >= 2 ? ctl[1] : 0;
  for (int s = 0; s < nshared; ++s) {
    const int d = dl[s];
    const int k0 = mob_off[d], k1 = mob_off[d + 1];
    double den = 0.0;
    for (int a = 0; a < K; ++a) {
      const int p = per[a];
      if (p % d == 0) den += (double)d / (double)p;
    }
    for (int j = tid; j < d; j += nthr) sv[j] = 0.0;
    for (int a = 0; a < K; ++a) {
      const int p = per[a];
      if (p % d != 0) continue;  // (uniform)
      for (int j = tid; j < d; j += nthr) uv[j] = 0.0;
      sync();
      for (int k = k0; k < k1; ++k) {
        const int e = mob_d[k];
        const double mu = (double)mob_mu[k];
        fold_means(cin + soff[a], p, e, [&](int i, double m) {
          const double val = mu * m;
          for (int n = i; n < d; n += e) uv[n] += val;
        });
        sync();
      }
      for (int j = tid; j < d; j += nthr) sv[j] += uv[j];
      tile_add(acc + soff[a], uv, p, d, -1.0);
      sync();
    }
    for (int j = tid; j < d; j += nthr) sv[j] = sv[j] / den;
    sync();
    for (int a = 0; a < K; ++a) {
      const int p = per[a];
      if (p % d == 0) tile_add(acc + soff[a], sv, p, d, (double)d / (double)p);
    }
    sync();
  }
  sync();
  for (int n = tid; n < ccap; n += nthr) orow[n] = n < total ? acc[n] : 0.0;
  if (tid == 0) status_out[w] = 0;
}

}  // namespace ph

// RamanujanPeriods.find_periods: hierarchical folds and the Ramanujan-subspace filter.
#pragma once

#include "ph_device.h"

namespace ph {

// ======================================================================================
// RamanujanPeriods.find_periods  (RamanujanPeriods.py:67-86, :124-169), folded form.
//   Rows of the reference dictionary are shifts of c_q / phi(q) (the row / max(row) at :129
//   cancels the L2 normalisation of :168).  With S = fold of x to period q:
//     a = S (star) c_q / phi,  out = a (*) c_q / phi  ==  (q/phi)^2 * E_q S,
//   where E_q = sum_{d | q} mu(q/d) P_d = prod_{prime r | q} (I - P_{q/r}) is the projector onto
//   the Ramanujan subspace (P_d = mean over the q/d cosets mod d), and
//   norms[q] = sum_j cnt_q[j] * out_j^2.
//
//   Hierarchical folds.  Only the periods of the upper half of the range, Q in (q_hi/2, q_hi]
//   ("roots"), are folded from the window (N reads each, chunked wave fold into the wave's LDS
//   strip A).  Every smaller period q has a multiple Q among the roots and S_q[i] = sum_t
//   S_Q[i + t q] is a fold of the STRIP (Q reads instead of N): the host hands every q <= q_hi/2
//   to one root ("children").  Children are folded from A into the scratch strip B and filtered
//   there; the root itself is filtered in place last.
//
//   The projector is applied one prime factor at a time, in place.  A step with d = q/r cosets
//   uses lane-per-coset when d >= 64 and a row-split mapping (64/d groups of d lanes, shuffle
//   tree) when d < 64, so that a large prime factor never serialises a coset in one lane.
//   One wavefront works on one root at a time; the wavefronts of a workgroup share the window.
// ======================================================================================
constexpr int kRamMaxWaves = 16;

// Everything the kernel needs to know about one period, in ONE 128-byte record (two s_load_dwordx16): the strip
// steps of a wavefront are chains of dependent LDS round trips with 3-4 wavefronts per SIMD to hide them, and the
// round-2 tables (root -> child list -> step offsets -> steps -> row-split geometry, geometry, scale) put five
// dependent scalar loads from memory in front of every period.
struct RamStep {  // one factor (I - P_d) of E_q: d = q / r cosets of r elements
  int dr;         // d | r << 16
  int sm;         // row-split geometry of d < 64: G | inv16 << 8, G = 64 / d row groups, inv16 = ceil(65536 / d)
  double inv_r;   // (lane / d == (lane * inv16) >> 16 for lane < 64)
};
constexpr int kRamMaxSteps = 5;  // distinct primes of q < 30030
struct RamJob {
  int q, k, nfull, rows;  // period; k = Q / q rows of a child in its root's strip; geometry of the fold of the window
  int c0, c1, flags, sm;  // root: its children are jobs [c0, c1); flags = emit | nsteps << 8; sm: geometry of q < 64
  double scale2, pad;     // (q / phi(q))^2
  RamStep st[kRamMaxSteps];
};
static_assert(sizeof(RamJob) == 128, "RamJob is uploaded as 32 words");

// Root fold without remainder rows.  The fold it replaced took the rows of a residue in blocks of 4 and then drained
// after every single leftover row and after the partial last row: at config 3 (22 rows of 6 chunks per root) a group
// issued 5 full batches and up to 4 one-row batches, each a full LDS round trip with 4 wavefronts per SIMD to hide it
// -- the folds ran at 0.55 of the streaming LDS rate although the bare 16-loads / drain / 16-adds pattern reaches 0.85
// at that occupancy (tools/micro/lds_pipe_bench 1024 163840; the A/B is profiles/r4_study/ram_ab_root_fold_v2.txt).
// Here the `rows` rows of a root are
// cut into k = ceil(rows / 8) batches of U or U + 1 rows (U = rows / k, compile time), every batch fully in flight
// before its one wait, and the partial last row is the last row of the last batch (lanes without it read element 0
// and add nothing).  The order of the additions per residue is unchanged (row 0, 1, ..., rows - 1).
template <typename T, int C, int NR, bool LAST, bool LW>
__device__ __forceinline__ void ram_fold_batch(typename Win<T, LW>::ptr ptr, typename Win<T, LW>::ptr x0, int p, const bool (&has)[C],
                                               double (&s)[C]) {
  T v[NR][C];
#pragma unroll
  for (int u = 0; u < NR; ++u)
#pragma unroll
    for (int c = 0; c < C; ++c) {
      if (LAST && u == NR - 1)
        v[u][c] = has[c] ? ptr[u * p + 64 * c] : x0[0];
      else
        v[u][c] = ptr[u * p + 64 * c];
    }
  __builtin_amdgcn_s_waitcnt(0xC07F);  // lgkmcnt(0)
  __builtin_amdgcn_sched_barrier(0);
#pragma unroll
  for (int u = 0; u < NR; ++u)
#pragma unroll
    for (int c = 0; c < C; ++c) s[c] += (LAST && u == NR - 1) ? (has[c] ? (double)v[u][c] : 0.0) : (double)v[u][c];
}

template <typename T, int C, int U, bool LW>
__device__ __forceinline__ void ram_fold_group(const T* __restrict__ xs, int p, int nfull, int k, int rem, int c0, int lane,
                                               double* __restrict__ sbuf) {
  typedef typename Win<T, LW>::ptr wptr;
  double s[C];
  bool has[C];
#pragma unroll
  for (int c = 0; c < C; ++c) {
    s[c] = 0.0;
    has[c] = 64 * (c0 + c) + lane < nfull;
  }
  const wptr x0 = Win<T, LW>::cast(xs);
  wptr ptr = x0 + lane + 64 * c0;
  int b = 0;
  for (; b < rem; ++b) {  // rem < k batches of U + 1 rows
    ram_fold_batch<T, C, U + 1, false, LW>(ptr, x0, p, has, s);
    ptr += (U + 1) * p;
  }
  for (; b + 1 < k; ++b) {
    ram_fold_batch<T, C, U, false, LW>(ptr, x0, p, has, s);
    ptr += U * p;
  }
  ram_fold_batch<T, C, U, true, LW>(ptr, x0, p, has, s);  // ends with the partial row
#pragma unroll
  for (int c = 0; c < C; ++c) {
    const int j = 64 * (c0 + c) + lane;
    if (j < p) sbuf[j] = s[c];
  }
}

template <typename T, int U, bool LW>
__device__ __forceinline__ void ram_root_fold_u(const T* __restrict__ xs, int Q, int nfull, int k, int rem, int lane,
                                                double* __restrict__ sbuf) {
  const int nchunks = (Q + 63) >> 6;
  int k0 = 0;
  for (; k0 + 4 <= nchunks; k0 += 4) ram_fold_group<T, 4, U, LW>(xs, Q, nfull, k, rem, k0, lane, sbuf);
  switch (nchunks - k0) {
    case 3: ram_fold_group<T, 3, U, LW>(xs, Q, nfull, k, rem, k0, lane, sbuf); break;
    case 2: ram_fold_group<T, 2, U, LW>(xs, Q, nfull, k, rem, k0, lane, sbuf); break;
    case 1: ram_fold_group<T, 1, U, LW>(xs, Q, nfull, k, rem, k0, lane, sbuf); break;
    default: break;
  }
}

// S_Q of the window into the strip, Q >= 64 (rows = ceil(N / Q) >= 1)
template <typename T, bool LW>
__device__ __forceinline__ void ram_root_fold(const T* __restrict__ xs, int Q, int rows, int nfull, int lane,
                                              double* __restrict__ sbuf) {
  const int k = (rows + 7) >> 3;  // batches
  int U = 1;                      // rows / k without a division (k <= rows, the quotient is in 1 .. 8)
  while ((U + 1) * k <= rows) ++U;
  const int rem = rows - U * k;
  switch (U) {
    case 1: ram_root_fold_u<T, 1, LW>(xs, Q, nfull, k, rem, lane, sbuf); break;
    case 2: ram_root_fold_u<T, 2, LW>(xs, Q, nfull, k, rem, lane, sbuf); break;
    case 3: ram_root_fold_u<T, 3, LW>(xs, Q, nfull, k, rem, lane, sbuf); break;
    case 4: ram_root_fold_u<T, 4, LW>(xs, Q, nfull, k, rem, lane, sbuf); break;
    case 5: ram_root_fold_u<T, 5, LW>(xs, Q, nfull, k, rem, lane, sbuf); break;
    case 6: ram_root_fold_u<T, 6, LW>(xs, Q, nfull, k, rem, lane, sbuf); break;
    case 7: ram_root_fold_u<T, 7, LW>(xs, Q, nfull, k, rem, lane, sbuf); break;
    default: ram_root_fold_u<T, 8, LW>(xs, Q, nfull, k, rem, lane, sbuf); break;
  }
}

// Row-split coset sums of s[0 .. len) modulo d < 64 (d | len): lane = g d + i (g < G = 64 / d) adds
// s[lane + k G d]; the G partial sums of a coset are combined with a shuffle tree.  Returns the coset
// total in EVERY lane of the coset's column (lane mod d), 0 in the idle lanes >= G d.
__device__ __forceinline__ double strip_cosets_small(const double* __restrict__ s, int len, int d, int sm, int lane) {
  const int G = sm & 255, inv16 = sm >> 8, L = G * d;
  double part = 0.0;
  if (lane < L) {
    int idx = lane;
    for (; idx + 3 * L < len; idx += 4 * L) {  // four loads in flight; the sum keeps its order
      const double a = s[idx], b = s[idx + L], c = s[idx + 2 * L], e = s[idx + 3 * L];
      part += a;
      part += b;
      part += c;
      part += e;
    }
    for (; idx < len; idx += L) part += s[idx];
  }
  int sft = 1;
  while (sft < G) sft <<= 1;
  for (sft >>= 1; sft >= 1; sft >>= 1) {
    const int src = lane + sft * d;
    const double o = __shfl(part, src & (kWave - 1), kWave);
    part += (src < L) ? o : 0.0;
  }
  const int g = (lane * inv16) >> 16;                     // lane / d
  const double tot = __shfl(part, lane - g * d, kWave);  // the column's total sits in its first row group
  return lane < L ? tot : 0.0;
}

// The strip loops below run with compile-time trip counts where the counts are small (a coset of r = 2, 3, 5, 7
// elements when d >= 64 and q <= 512; a child with k = Q / q <= 8 rows) and take two lane chunks per trip: the
// kernel is paced by the dependent LDS round trips of each wavefront, so all loads of a trip are in flight
// together.  Lanes past the end read element 0 and write nothing.  Sums keep the order of the generic loops.
template <int K>
__device__ __forceinline__ void strip_fold_fixed(const double* __restrict__ src, int q, double* __restrict__ dst,
                                                 int lane) {
  for (int c0 = 0; c0 < q; c0 += 2 * kWave) {
    const int i0 = c0 + lane, i1 = i0 + kWave;
    const bool ok0 = i0 < q, ok1 = i1 < q;
    const double* p0 = src + (ok0 ? i0 : 0);
    const double* p1 = src + (ok1 ? i1 : 0);
    double v0[K], v1[K];
#pragma unroll
    for (int t = 0; t < K; ++t) {
      v0[t] = p0[t * q];
      v1[t] = p1[t * q];
    }
    double e0 = 0.0, o0 = 0.0, e1 = 0.0, o1 = 0.0;
#pragma unroll
    for (int t = 0; t < K; ++t) {
      if (t & 1) {
        o0 += v0[t];
        o1 += v1[t];
      } else {
        e0 += v0[t];
        e1 += v1[t];
      }
    }
    if (ok0) dst[i0] = e0 + o0;
    if (ok1) dst[i1] = e1 + o1;
  }
}

// dst[i] = sum_t src[i + t q], i < q  (len = k q): the fold of a folded strip.
__device__ __forceinline__ void strip_fold(const double* __restrict__ src, int len, int q, int k, int sm,
                                           double* __restrict__ dst, int lane) {
  if (q < 64) {
    const double tot = strip_cosets_small(src, len, q, sm, lane);
    if (lane < q) dst[lane] = tot;
    return;
  }
  switch (k) {
    case 2: strip_fold_fixed<2>(src, q, dst, lane); return;
    case 3: strip_fold_fixed<3>(src, q, dst, lane); return;
    case 4: strip_fold_fixed<4>(src, q, dst, lane); return;
    case 5: strip_fold_fixed<5>(src, q, dst, lane); return;
    case 6: strip_fold_fixed<6>(src, q, dst, lane); return;
    case 7: strip_fold_fixed<7>(src, q, dst, lane); return;
    case 8: strip_fold_fixed<8>(src, q, dst, lane); return;
    default: break;
  }
  for (int i = lane; i < q; i += kWave) {
    double a0 = 0.0, a1 = 0.0;
    int t = 0;
    for (; t + 2 <= k; t += 2) {
      a0 += src[i + t * q];
      a1 += src[i + (t + 1) * q];
    }
    if (t < k) a0 += src[i + t * q];
    dst[i] = a0 + a1;
  }
}

// Sum of squares of the filtered strip, split by the count of the residue: norms[q] = (q / phi)^4 (cs all + full) with
// cs = rows - 1 (every residue has at least rows - 1 samples, the residues below nfull one more).
struct RamAcc {
  double all = 0.0, full = 0.0;
  __device__ __forceinline__ void add(double o, int j, int nfull) {
    const double t = o * o;
    all += t;
    full += j < nfull ? t : 0.0;
  }
};

// One factor (I - P_d) of the projector: every element of s[0 .. q) loses the mean of its coset modulo d (r = q / d
// elements per coset); each lane reads and writes only its own elements.  LAST: the last factor of a period writes
// nothing back -- the filtered values go straight into the sum of squares (one pass over the strip, its stores and
// one wavefront sync less per period).
template <int R, bool LAST>
__device__ __forceinline__ void strip_step_fixed(double* __restrict__ s, int d, double inv_r, int lane, int nfull,
                                                 RamAcc& acc) {
  for (int c0 = 0; c0 < d; c0 += 2 * kWave) {
    const int i0 = c0 + lane, i1 = i0 + kWave;
    const bool ok0 = i0 < d, ok1 = i1 < d;
    double* p0 = s + (ok0 ? i0 : 0);
    double* p1 = s + (ok1 ? i1 : 0);
    double v0[R], v1[R];
#pragma unroll
    for (int t = 0; t < R; ++t) {
      v0[t] = p0[t * d];
      v1[t] = p1[t * d];
    }
    double m0 = 0.0, m1 = 0.0;
#pragma unroll
    for (int t = 0; t < R; ++t) {
      m0 += v0[t];
      m1 += v1[t];
    }
    m0 *= inv_r;
    m1 *= inv_r;
    if (ok0) {
#pragma unroll
      for (int t = 0; t < R; ++t) {
        if (LAST)
          acc.add(v0[t] - m0, i0 + t * d, nfull);
        else
          p0[t * d] = v0[t] - m0;
      }
    }
    if (ok1) {
#pragma unroll
      for (int t = 0; t < R; ++t) {
        if (LAST)
          acc.add(v1[t] - m1, i1 + t * d, nfull);
        else
          p1[t * d] = v1[t] - m1;
      }
    }
  }
}

template <bool LAST>
__device__ __forceinline__ void strip_step(double* __restrict__ s, int q, const RamStep& st, int lane, int nfull,
                                           RamAcc& acc) {
  const int d = st.dr & 0xffff, r = st.dr >> 16;
  const double inv_r = st.inv_r;
  if (d < 64) {
    const int L = (st.sm & 255) * d;
    const double m = strip_cosets_small(s, q, d, st.sm, lane) * inv_r;
    if (lane < L) {
      int idx = lane;
      for (; idx + 3 * L < q; idx += 4 * L) {
        const double a = s[idx], b = s[idx + L], c = s[idx + 2 * L], e = s[idx + 3 * L];
        if (LAST) {
          acc.add(a - m, idx, nfull);
          acc.add(b - m, idx + L, nfull);
          acc.add(c - m, idx + 2 * L, nfull);
          acc.add(e - m, idx + 3 * L, nfull);
        } else {
          s[idx] = a - m;
          s[idx + L] = b - m;
          s[idx + 2 * L] = c - m;
          s[idx + 3 * L] = e - m;
        }
      }
      for (; idx < q; idx += L) {
        if (LAST)
          acc.add(s[idx] - m, idx, nfull);
        else
          s[idx] -= m;
      }
    }
    return;
  }
  switch (r) {  // r is prime; d >= 64 and q <= 512 leave 2, 3, 5, 7
    case 2: strip_step_fixed<2, LAST>(s, d, inv_r, lane, nfull, acc); return;
    case 3: strip_step_fixed<3, LAST>(s, d, inv_r, lane, nfull, acc); return;
    case 5: strip_step_fixed<5, LAST>(s, d, inv_r, lane, nfull, acc); return;
    case 7: strip_step_fixed<7, LAST>(s, d, inv_r, lane, nfull, acc); return;
    default: break;
  }
  for (int i = lane; i < d; i += kWave) {
    double m = 0.0;
    for (int t = 0; t < r; ++t) m += s[i + t * d];
    m *= inv_r;
    for (int t = 0; t < r; ++t) {
      if (LAST)
        acc.add(s[i + t * d] - m, i + t * d, nfull);
      else
        s[i + t * d] -= m;
    }
  }
}

// s holds S_q: apply E_q (in place, but for the last factor) and reduce to norms[q] (all lanes get it).  `steps` is
// the record's step list in memory: the next step is fetched (scalar load) while the current one runs.
__device__ __forceinline__ double ram_emit(double* __restrict__ s, const RamJob& J, const RamStep* __restrict__ steps,
                                           int lane) {
  const int q = J.q, nsteps = J.flags >> 8, nfull = J.nfull;
  RamAcc acc;
  RamStep cur = steps[0];
#pragma unroll 1
  for (int k = 0; k + 1 < nsteps; ++k) {
    const RamStep nxt = steps[k + 1];
    strip_step<false>(s, q, cur, lane, nfull, acc);
    ram_wave_sync();
    cur = nxt;
  }
  if (nsteps > 0) {
    strip_step<true>(s, q, cur, lane, nfull, acc);
  } else {  // q == 1: E_1 is the identity
    for (int j = lane; j < q; j += kWave) acc.add(s[j], j, nfull);
  }
  const double cs = (double)(J.rows - 1);
  return wave_sum(cs * acc.all + acc.full) * (J.scale2 * J.scale2);  // out = (q / phi)^2 E_q S, norms = sum cnt out^2
}

// LDS of k_ramanujan: the window, then per wavefront strip A (q_hi doubles, the root fold) and strip B (q_hi / 2, one
// child).  pad == 0 (the host drops the zeroed pad when that makes room for one more wavefront; roots >= 64 only): the
// reads of a fold past the end of the window land in the strips -- they belong to lanes whose sums are discarded.
template <typename T>
struct RamLds {
  T* xs;
  double* sA;  // nw strips of lenA
  double* sB;  // nw strips of lenB
  int lenA, lenB;
  size_t bytes;
};
template <typename T, class C>
__host__ __device__ __forceinline__ RamLds<T> ram_carve(C cv, int N, int q_hi, int nw, int pad, bool lw) {
  RamLds<T> L;
  L.xs = lw ? cv.template take<T>(N + pad) : nullptr;
  L.lenA = q_hi;
  L.lenB = q_hi / 2 > 0 ? q_hi / 2 : 1;
  L.sA = cv.template take<double>((size_t)nw * L.lenA);
  L.sB = cv.template take<double>((size_t)nw * L.lenB);
  L.bytes = cv.off;
  return L;
}

template <typename T, bool LW>
__global__ __launch_bounds__(kRamMaxWaves * 64) void k_ramanujan(const T* __restrict__ x, int N, int q_hi,
                                                                const RamJob* __restrict__ roots, int n_root,
                                                                const RamJob* __restrict__ children, T* gwin, int pad,
                                                                double* __restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int nw = blockDim.x >> 6;
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int lane = threadIdx.x & (kWave - 1);
  const RamLds<T> L = ram_carve<T>(Carve(smem), N, q_hi, nw, pad, LW);
  T* xs = window_buf<T, LW>(L.xs, gwin, N + pad);
  double* sA = L.sA + (size_t)wv * L.lenA;  // this wave's root fold S_Q
  double* sB = L.sB + (size_t)wv * L.lenB;  // scratch for one child

  const int64_t w = blockIdx.x;
  const WgStamp<kClocks> t0;
  load_window(x + w * (int64_t)N, xs, N);
  if (pad) zero_pad(xs, N);
  double* orow = out + w * (int64_t)(q_hi + 1);
  // the root queue: orow[0] (0 is never a period) is zero on entry and is put back to zero at the end -- an LDS
  // counter would cost the 16 bytes that decide between 15 and 16 wavefronts at config 3
  int* next_root = reinterpret_cast<int*>(orow);
  __syncthreads();
  const WgStamp<kClocks> t1;  // the window is loaded

  // A workgroup holds its CU alone (window + strips fill the LDS) and ends with its slowest wavefront: the roots are
  // taken from a queue, not dealt round-robin -- no wavefront idles while another still has whole roots to do.
  for (int i = wv; i < n_root;) {
    int nxt = 0;
    if (lane == 0) nxt = atomicAdd(next_root, 1);  // asked for now, needed after this root: the HBM round trip hides
    const RamJob R = roots[i];
    const int Q = R.q;
    // ---- S_Q from the window
    if (Q < 64) {
      const double tot = wave_fold_small(xs, N, Q, lane);  // row-split path, S_Q[lane] in the lanes below Q
      if (lane < Q) sA[lane] = tot;
    } else {
      // LDS capacity (window + strips) caps this kernel at 3-4 wavefronts per SIMD, so registers are plentiful:
      // batches of up to 9 rows x 4 chunks of loads in flight per wait, no leftover rows (ram_root_fold)
      ram_root_fold<T, LW>(xs, Q, R.rows, R.nfull, lane, sA);
    }
    ram_wave_sync();
#ifdef PH_RAM_FOLDS_ONLY  // profiling aid (results incomplete): the root folds alone, one strip element kept alive
    if (lane == 0) orow[Q] = sA[Q >> 1];
    ram_wave_sync();
    i = nw + __builtin_amdgcn_readfirstlane(nxt);
    continue;
#endif
    // ---- children: fold of the strip, filtered in the scratch strip
    for (int c = R.c0; c < R.c1; ++c) {
      const RamJob C = children[c];
      strip_fold(sA, Q, C.q, C.k, C.sm, sB, lane);
      ram_wave_sync();
      const double v = ram_emit(sB, C, children[c].st, lane);
      if (lane == 0) orow[C.q] = v;
      ram_wave_sync();  // sB is rewritten by the next child
    }
    if (R.flags & 1) {
      const double v = ram_emit(sA, R, roots[i].st, lane);
      if (lane == 0) orow[Q] = v;
    }
    ram_wave_sync();  // sA is rewritten by the next root
    i = nw + __builtin_amdgcn_readfirstlane(nxt);
  }
  __syncthreads();
  if (threadIdx.x == 0) orow[0] = 0.0;
  if (kClocks && (blockIdx.x == 7 || blockIdx.x == 2000) && threadIdx.x == 0) {
    const WgStamp<kClocks> t2;
    printf("k_ramanujan window %d: load %lld cycles / %lld ticks(100MHz), work %lld cycles / %lld ticks -> %.0f MHz\n", (int)w,
           t1.ck0 - t0.ck0, t1.wk0 - t0.wk0, t2.ck0 - t1.ck0, t2.wk0 - t1.wk0, 100.0 * (double)(t2.ck0 - t1.ck0) / (double)(t2.wk0 - t1.wk0));
  }
}

}  // namespace ph

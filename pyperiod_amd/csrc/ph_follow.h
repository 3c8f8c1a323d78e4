// Extraction along a period track: k_follow peels, frame by frame, the periodic component at the periods a caller names
// for that frame -- its own contour, an edited one, one from another tool -- and leaves ONE period of every component in
// the segment layout k_qo_extract writes and k_overlap_add_periodic reads.  Reference citations are file:line into
// the reference's pyPeriod/.
//
//   x_f[i]     = (double)(Tf)((double)signal[f hop + i] * window[i]) for f hop + i < L, else 0   (window == nullptr: no
//                product) -- exactly the frame k_frames would write, widened to double; no (W, N) array exists
//   C_f        = counts[f] clipped to [0, pcap];  r_0 = x_f, off = 0
//   for a = 0 .. C_f - 1:  p = periods[f, a];  stop at the first block with p < 1, p > N or off + p > ccap
//     s        = project(r_a, p, trunc, False, return_single_period=True)        (Periods.py:171-198, :216-217)
//     seg[f, off + j] = s[j] for j < p;   r_{a+1}[i] = r_a[i] - s[i mod p]       (Periods.py:277)
//     powers[f, a] = (pn(r_a) - pn(r_{a+1})) / pn(x_f), exactly 0.0 when pn(x_f) == 0      (Periods.py:238-241, :278-280)
//     off += p
//   done[f] = the blocks written; powers[f, a >= done[f]] = 0.0; seg behind the last block is never written.
//
// The means are residue_mean's (follow_mean: column_sum, plus numpy's +0.0 identity): one thread per residue, rows added in order with one division, the bits of
// the reference's np.sum(cp, 0) / divs (trunc: np.mean over the complete rows).  p <= N gives every residue a sample
// and trunc a complete row.  (p = 1 alone is no row-order sum in the reference: see numpy_contiguous_sum below.)  The
// subtraction is one rounded operation per sample.  Only the sums of squares behind
// `powers` go through the block reduction, whose order is not numpy's (the 1e-10 bar of the small_to_large powers).
//
// One workgroup handles one frame at a time and the workgroups walk the frames grid-stride, so whatever the kernel
// needs besides its arguments is sized per workgroup, never per frame.  Two states of N doubles move together: the
// residual frame and one period of means live in LDS while both fit the workgroup's limit (LW), otherwise in the
// workgroup's slice of an HBM workspace (2 * win_stride(N) doubles; the signal and the window are then read from HBM /
// L2 as in the LDS placement, and the residual goes through L2).  A barrier orders either placement: the states are
// written and read by the same workgroup only.
// Per frame and block the workgroup makes three passes over the residual: the column sums (p threads, each a chain of
// N / p dependent adds with eight reads in flight -- the latency-bound phase for short periods, and the one that may not
// be re-associated), the subtraction fused with the sum of squares (all threads, i mod p kept incrementally), and the
// block reduction.  No atomics; index arithmetic that involves W, L or ccap is int64 (W * ccap passes 2^31).
//
// Included by period_hip.hip behind ph_frames.h.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "ph_device.h"

namespace ph {

constexpr int kFollowMaxBlocks = 64;  // blocks per frame: what a 64-bit routing mask of k_overlap_add_periodic can name
constexpr int kFollowMaxSeg = 1 << 24;  // ccap, the limit k_overlap_add_periodic puts on the same array

// threads per workgroup: a quarter of the frame in whole wavefronts, 64 .. 1024.  A thread then owns four samples of the
// load and subtraction passes, and frames of a thousand samples leave room for eight workgroups per CU -- the column sums
// of a short period keep only p threads busy, and other workgroups are what hides their latency.
__host__ __device__ inline int follow_block(int N) {
  const int b = ((N + 3) / 4 + kWave - 1) & ~(kWave - 1);
  return b < kWave ? kWave : b > 1024 ? 1024 : b;
}

// LDS of k_follow: the reduction scratch, and with `in_lds` the residual frame and one period of means (p <= N)
struct FollowLds {
  double* red;
  double* r;
  double* m;
  size_t bytes;
};
template <class C>
__host__ __device__ __forceinline__ FollowLds follow_carve(C cv, int N, bool in_lds) {
  FollowLds L;
  L.red = cv.template take<double>(kRedDoubles);
  L.r = in_lds ? cv.template take<double>((size_t)N) : nullptr;
  L.m = in_lds ? cv.template take<double>((size_t)N) : nullptr;
  L.bytes = cv.off;
  return L;
}
// doubles of one workgroup's slice of the HBM workspace (the same two states)
__host__ __device__ inline size_t follow_work_doubles(int N) { return 2 * win_stride((size_t)N); }

// ---- p = 1: the one period whose reference sum is not a row-order sum.  np.sum(cp, 0) on the (N, 1) rectangle reduces
// along the contiguous axis, where numpy adds pairwise: the elements in chunks of 8192 (its buffer), the chunk sums added
// up in order from 0.0, and inside a chunk the tree below -- halves cut at a multiple of 8 down to leaves of at most 128
// elements, a leaf summed in eight strided accumulators that are combined as ((0+1)+(2+3))+((4+5)+(6+7)), the tail and
// leaves under 8 elements one by one.  The kernels that hold the 1e-10 bar take the row order there; this one holds the
// reference's bits at every period, so it walks that very tree: one thread, depth first, the left sums of the open nodes
// in `stk` (LDS, one double per level: 8 levels at most below 8192 elements).
constexpr int kNumpyChunk = 8192, kNumpyLeaf = 128;

__device__ __forceinline__ double numpy_leaf_sum(const double* a, int n) {
  if (n < 8) {
    double res = 0.0;
    for (int i = 0; i < n; ++i) res += a[i];
    return res;
  }
  double r[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) r[j] = a[j];
  int i = 8;
  for (; i < n - (n % 8); i += 8) {
#pragma unroll
    for (int j = 0; j < 8; ++j) r[j] += a[i + j];
  }
  double res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
  for (; i < n; ++i) res += a[i];
  return res;
}

__device__ inline double numpy_pairwise_sum(const double* a, int n, double* stk) {
  unsigned right = 0;  // bit d: the node on the way down at depth d + 1 is a right child
  int depth = 0;
  for (;;) {
    int start = 0, len = n;
    for (int d = 0; d < depth; ++d) {
      int n2 = len / 2;
      n2 -= n2 % 8;
      if ((right >> d) & 1u) {
        start += n2;
        len -= n2;
      } else {
        len = n2;
      }
    }
    if (len > kNumpyLeaf) {  // an inner node: its left child first
      right &= ~(1u << depth);
      ++depth;
      continue;
    }
    double ret = numpy_leaf_sum(a + start, len);
    for (;;) {  // back up: a left child hands over to its sibling, a right child closes the node
      if (depth == 0) return ret;
      --depth;
      if (!((right >> depth) & 1u)) {
        stk[depth] = ret;
        right |= 1u << depth;
        ++depth;
        break;
      }
      ret = stk[depth] + ret;
    }
  }
}

// the sum of a[0 .. n) in the order of np.add.reduce over a contiguous axis
__device__ inline double numpy_contiguous_sum(const double* a, int n, double* stk) {
  double acc = 0.0;
  for (int at = 0; at < n; at += kNumpyChunk) acc += numpy_pairwise_sum(a + at, n - at < kNumpyChunk ? n - at : kNumpyChunk, stk);
  return acc;
}

// residue_mean with the reference's sign of zero: np.sum starts from its identity +0.0, so a residue whose samples are
// all -0.0 (a sample under a window weight of exactly zero) sums to +0.0 there and to -0.0 in column_sum alone.  Adding
// the identity once changes no other sum by a bit (x + 0.0 == x for every x but -0.0); the rows and the divisor are
// those of residue_mean.
__device__ __forceinline__ double follow_mean(const double* __restrict__ xs, const Fold& f, int j, bool trunc) {
  const int n = trunc ? (f.trows < f.count(j) ? f.trows : f.count(j)) : f.count(j);
  const int div = trunc ? f.trows : f.count(j);
  return (0.0 + column_sum(xs, j, f.p, n)) / (double)div;
}

template <typename Tin, typename Tf, bool LW>
__global__ __launch_bounds__(1024) void k_follow(const Tin* __restrict__ s, int64_t L, int N, int hop, int64_t W,
                                                 const double* __restrict__ win, const int* __restrict__ periods,
                                                 const int* __restrict__ counts, int pcap, int ccap, unsigned flags,
                                                 double* gws, double* __restrict__ seg, double* __restrict__ powers,
                                                 int* __restrict__ done) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const FollowLds Ld = follow_carve(Carve(smem), N, LW);
  double* r = LW ? Ld.r : gws + (size_t)blockIdx.x * follow_work_doubles(N);
  double* m = LW ? Ld.m : r + win_stride((size_t)N);
  double* red = Ld.red;
  const int tid = threadIdx.x, nt = blockDim.x;
  const bool trunc = flags & kTrunc;

  for (int64_t f = blockIdx.x; f < W; f += gridDim.x) {
    // ---- the frame, as k_frames rounds it, and its sum of squares
    const int64_t at = f * hop;
    double acc = 0.0;
    for (int i = tid; i < N; i += nt) {
      double v = 0.0;
      if (at + i < L) {
        const double t = win ? (double)s[at + i] * win[i] : (double)s[at + i];
        v = (double)(Tf)t;
      }
      r[i] = v;
      acc += v * v;
    }
    // (the barriers of block_sum also make r whole for every thread; the ones of the last frame's final block_sum stand
    // between that frame's reads of r and these writes)
    const double pn0 = periodic_norm_from_sq(block_sum(acc, red), N, 0);
    double pn_prev = pn0;

    const int cf = counts[f] < 0 ? 0 : counts[f] > pcap ? pcap : counts[f];
    const int* prow = periods + f * (int64_t)pcap;
    double* srow = seg + f * (int64_t)ccap;
    double* wrow = powers + f * (int64_t)pcap;
    int64_t off = 0;
    int a = 0;
    for (; a < cf; ++a) {
      const int p = prow[a];  // (the same value in every thread: the stop is uniform)
      if (p < 1 || p > N || off + p > ccap) break;
      // ---- one period of means, in row order: kept for the subtraction and written out as the block's segment
      if (p == 1) {  // the mean: numpy's own order (above); trunc or not, the sum over all N samples by N
        if (tid == 0) {
          const double mj = numpy_contiguous_sum(r, N, red) / (double)N;
          m[0] = mj;
          srow[off] = mj;
        }
      } else {
        const Fold fo(N, p);
        for (int j = tid; j < p; j += nt) {
          const double mj = follow_mean(r, fo, j, trunc);
          m[j] = mj;
          srow[off + j] = mj;
        }
      }
      __syncthreads();
      // ---- r <- r - tile(means), one rounded subtraction per sample; i mod p kept incrementally
      acc = 0.0;
      int j = tid % p;
      const int step = nt % p;
      for (int i = tid; i < N; i += nt) {
        const double v = r[i] - m[j];
        r[i] = v;
        acc += v * v;
        j += step;
        if (j >= p) j -= p;
      }
      // (block_sum's barriers: r is whole before the next block's column sums, m is read before it is rewritten)
      const double pn = periodic_norm_from_sq(block_sum(acc, red), N, 0);
      if (tid == 0) wrow[a] = pn0 == 0.0 ? 0.0 : (pn_prev - pn) / pn0;
      pn_prev = pn;
      off += p;
    }
    if (tid == 0) done[f] = a;
    for (int k = a + tid; k < pcap; k += nt) wrow[k] = 0.0;
  }
}

}  // namespace ph

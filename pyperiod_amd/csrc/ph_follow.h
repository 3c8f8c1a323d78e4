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
// k_follow_residual is the same body on the frames f0 .. f0 + Wb of the recording, and keeps what k_follow throws away:
//   x_f as above with f0 + f for f;  the walk stops at the first p < 1 or p > N (no ccap);  out[f, i] = r_{C}[i], the
//   residual after the last block peeled, every sample of every row (no blocks: x_f itself, the frame k_frames writes
//   as double).  It writes no seg, powers or done, so it sums no squares and reduces nothing.  The statements of both
//   kernels are ph_follow_body.h, included into each: the residual has k_follow's bits by construction.
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
  constexpr bool RES = false;  // (one body for both kernels: ph_follow_body.h says what RES selects and why it is text)
  constexpr int64_t f0 = 0;
  double* const out = nullptr;
#include "ph_follow_body.h"
}

// The frames f0 .. f0 + W of the recording less the tracks named for them: periods (W, pcap) and counts (W) are
// block-local, out is (W, N).  pcap == 0: no tracks, periods and counts are not read.
template <typename Tin, typename Tf, bool LW>
__global__ __launch_bounds__(1024) void k_follow_residual(const Tin* __restrict__ s, int64_t L, int N, int hop,
                                                          int64_t f0, int64_t W, const double* __restrict__ win,
                                                          const int* __restrict__ periods,
                                                          const int* __restrict__ counts, int pcap, unsigned flags,
                                                          double* gws, double* __restrict__ out) {
  constexpr bool RES = true;
  constexpr int ccap = 0;
  double* const seg = nullptr;
  double* const powers = nullptr;
  int* const done = nullptr;
#include "ph_follow_body.h"
}

}  // namespace ph

// Short-time framing and overlap-add on the device: k_frames cuts a signal of L samples into the (W, N) batch every
// other entry point takes, k_overlap_add folds a (W, K, N) result back onto the L samples of the signal, and
// k_overlap_add_tracks folds it onto several tracks of L samples, the rows of each chosen by a mask;
// k_overlap_add_periodic does the same from one period per row (the segments of k_qo_extract), tiled on the fly;
// k_overlap_add_block / k_overlap_add_finish do the work of the first two for a recording that comes in blocks of
// frames.  All are
// memory-bound element-wise kernels without LDS; all index arithmetic is int64 (f * hop and f * N pass 2^31 for real
// recordings).  Included by period_hip.hip behind ph_fit.h.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace ph {

constexpr int kFramesBlock = 256;

template <typename T, int V>
struct alignas(sizeof(T) * V) FrameVec {
  T v[V];
};

// ======================================================================================
// frames[f, i] = Tout((double)s[f * hop + i] * win[i]) if f * hop + i < L else 0          (win == nullptr: no product,
// a same-dtype copy is exact).  frames is (W, N) row-major contiguous = one flat array of W * N elements, and the kernel
// walks it flat: a lane owns V consecutive elements, V * sizeof(Tout) = 16 bytes, and stores them with one 16-byte
// access.  A flat vector is 16-byte aligned whenever the base pointer is, whatever N is (an odd N only makes it straddle
// two rows, which costs a wrap of (f, i) and nothing else), so the host picks V > 1 exactly when `frames` is 16-byte
// aligned and V = 1 -- every access scalar, correct for every N, hop and alignment -- otherwise.  The elements behind the
// last whole vector (W * N mod V of them) are stored one by one.
// The source address s + f * hop + i has no alignment to speak of (odd hop, float32): the V samples are read with one
// vector load only when they lie in one row, inside the signal, and the real address is aligned to the vector;
// otherwise one by one.  Overlapping frames re-read the signal from L2 (the signal is hop / N of the output's size).
// Grid: flat over the vectors with a grid-stride loop, so W never sits in a 16-bit grid dimension; (f, i) of a lane's
// first vector costs one 64-bit division, every further step adds the precomputed quotient and remainder of the stride.
// ======================================================================================
template <typename Tin, typename Tout, int V>
__global__ __launch_bounds__(kFramesBlock) void k_frames(const Tin* __restrict__ s, int64_t L, int N, int hop, int64_t W,
                                                        const double* __restrict__ win, Tout* __restrict__ frames) {
  const int64_t total = W * (int64_t)N;
  const int64_t n_vec = total / V;
  const int64_t stride = (int64_t)gridDim.x * kFramesBlock;  // in vectors
  const int64_t step = stride * V;                           // in elements
  const int64_t step_f = step / N;
  const int step_i = (int)(step % N);
  int64_t vec = (int64_t)blockIdx.x * kFramesBlock + threadIdx.x;
  int64_t f = 0;
  int i = 0;
  if (vec < n_vec) {
    const int64_t e0 = vec * V;
    f = e0 / N;
    i = (int)(e0 - f * N);
  }
  for (; vec < n_vec; vec += stride) {
    FrameVec<Tout, V> o;
    const int64_t src = f * hop + i;
    bool done = false;
    if constexpr (V > 1) {
      // one row, inside the signal, and the real source address aligned to the vector
      if (i + V <= N && src + V <= L && (reinterpret_cast<uintptr_t>(s + src) % (sizeof(Tin) * V)) == 0) {
        const FrameVec<Tin, V> in = *reinterpret_cast<const FrameVec<Tin, V>*>(s + src);
#pragma unroll
        for (int j = 0; j < V; ++j) o.v[j] = win ? (Tout)((double)in.v[j] * win[i + j]) : (Tout)(double)in.v[j];
        done = true;
      }
    }
    if (!done) {
      int64_t ff = f;
      int ii = i;
#pragma unroll
      for (int j = 0; j < V; ++j) {
        const int64_t a = ff * hop + ii;
        Tout r = (Tout)0;
        if (a < L) r = win ? (Tout)((double)s[a] * win[ii]) : (Tout)(double)s[a];
        o.v[j] = r;
        if (++ii == N) {
          ii = 0;
          ++ff;
        }
      }
    }
    *reinterpret_cast<FrameVec<Tout, V>*>(frames + vec * V) = o;
    f += step_f;
    i += step_i;
    if (i >= N) {
      i -= N;
      ++f;
    }
  }
  // the elements behind the last whole vector
  if constexpr (V > 1) {
    const int64_t e = n_vec * V + (int64_t)blockIdx.x * kFramesBlock + threadIdx.x;
    if (e < total) {
      const int64_t ff = e / N;
      const int ii = (int)(e - ff * N);
      const int64_t a = ff * hop + ii;
      Tout r = (Tout)0;
      if (a < L) r = win ? (Tout)((double)s[a] * win[ii]) : (Tout)(double)s[a];
      frames[e] = r;
    }
  }
}

// ---- the pieces of the walk every overlap-add kernel below makes for its sample n
// the frames f < W with 0 <= n - f hop < N: f_lo .. f_hi (none when f_lo > f_hi)
__device__ __forceinline__ void ola_frame_span(int64_t n, int64_t N, int64_t hop, int64_t W, int64_t& f_lo, int64_t& f_hi) {
  f_lo = n < N ? 0 : (n - N) / hop + 1;
  f_hi = n / hop;
  if (f_hi > W - 1) f_hi = W - 1;
}
// a count as the caller left it, clipped to [0, cap]
__device__ __forceinline__ int ola_clip(int count, int cap) { return count < 0 ? 0 : count > cap ? cap : count; }
// the synthesis weight of offset i (nullptr: all ones); its product with the analysis weight is added to den
template <typename I>
__device__ __forceinline__ double ola_window(I i, const double* __restrict__ wa, const double* __restrict__ ws, double& den) {
  const double s = ws ? ws[i] : 1.0;
  den += (wa ? wa[i] : 1.0) * s;
  return s;
}
// the lowest kf bits of a mask word: unsigned throughout, and no shift by 64 (kf = 0: no bit at all)
__device__ __forceinline__ unsigned long long ola_cut(unsigned long long m, int kf) {
  if (kf < 64) m &= (1ull << kf) - 1ull;
  return m;
}
// num, or with `norm` num / den where den > 0 and exactly 0.0 elsewhere
__device__ __forceinline__ double ola_result(double num, double den, int norm) {
  return norm ? (den > 0.0 ? num / den : 0.0) : num;
}
// The two row walks over row[k * N], the sample of one frame's rows.  The one-launch kernels and the blocked kernel add
// their terms with these, so a block continues a sample's sum with the very expression of the one-launch kernels:
// num += s * (double)row[...], four loads in flight, added in ascending k.
// the rows k < kf
template <typename T>
__device__ __forceinline__ void ola_add_rows(const T* __restrict__ row, int N, int kf, double s, double& num) {
  int k = 0;
  for (; k + 4 <= kf; k += 4) {
    const double a0 = (double)row[(int64_t)(k + 0) * N], a1 = (double)row[(int64_t)(k + 1) * N];
    const double a2 = (double)row[(int64_t)(k + 2) * N], a3 = (double)row[(int64_t)(k + 3) * N];
    num += s * a0;
    num += s * a1;
    num += s * a2;
    num += s * a3;
  }
  for (; k < kf; ++k) num += s * (double)row[(int64_t)k * N];
}
// the rows a mask word names, already cut to the rows in use (ola_cut): lowest set bit first
template <typename T>
__device__ __forceinline__ void ola_add_masked(const T* __restrict__ row, int N, unsigned long long m, double s, double& num) {
  int left = __builtin_popcountll(m);
  for (; left >= 4; left -= 4) {
    const int k0 = __builtin_ctzll(m);
    m &= m - 1ull;
    const int k1 = __builtin_ctzll(m);
    m &= m - 1ull;
    const int k2 = __builtin_ctzll(m);
    m &= m - 1ull;
    const int k3 = __builtin_ctzll(m);
    m &= m - 1ull;
    const double a0 = (double)row[(int64_t)k0 * N], a1 = (double)row[(int64_t)k1 * N];
    const double a2 = (double)row[(int64_t)k2 * N], a3 = (double)row[(int64_t)k3 * N];
    num += s * a0;
    num += s * a1;
    num += s * a2;
    num += s * a3;
  }
  for (; left > 0; --left) {
    const int k = __builtin_ctzll(m);
    m &= m - 1ull;
    num += s * (double)row[(int64_t)k * N];
  }
}

// ======================================================================================
// Overlap-add in the gather form: y (W, K, N) of T -> out (L) float64.
//   num[n] = sum_f sum_{k < K_f} ws[n - f hop] * y[f, k, n - f hop]     over the frames f < W with 0 <= n - f hop < N
//   den[n] = sum_f wa[n - f hop] * ws[n - f hop]                        over the same frames
//   out[n] = ola_result(num[n], den[n], norm)
// K_f = counts[f] clipped to [0, K] (counts == nullptr: K); rows k >= K_f are never read.
// Every output sample is owned by one lane, which walks its at most ceil(N / hop) frames in ascending f and their rows in
// ascending k, accumulating in float64: one fixed order per sample, no atomics, so the result is the same bits on every
// run.  Lanes of a wavefront take consecutive n, so for one (f, k) they read consecutive elements of one row: every load
// is coalesced, and the grid as a whole reads each element of y with f hop + i < L exactly once.  den comes from the
// same walk.  Flat grid with a grid-stride loop over n.
// ======================================================================================
template <typename T>
__global__ __launch_bounds__(kFramesBlock) void k_overlap_add(const T* __restrict__ y, int64_t W, int K, int N, int hop,
                                                             int64_t L, const int* __restrict__ counts,
                                                             const double* __restrict__ wa, const double* __restrict__ ws,
                                                             int norm, double* __restrict__ out) {
  const int64_t stride = (int64_t)gridDim.x * kFramesBlock;
  for (int64_t n = (int64_t)blockIdx.x * kFramesBlock + threadIdx.x; n < L; n += stride) {
    int64_t f_lo, f_hi;
    ola_frame_span(n, N, hop, W, f_lo, f_hi);
    double num = 0.0, den = 0.0;
    for (int64_t f = f_lo; f <= f_hi; ++f) {
      const int i = (int)(n - f * hop);
      const int kf = counts ? ola_clip(counts[f], K) : K;
      const double s = ola_window(i, wa, ws, den);
      const T* row = y + (f * K) * (int64_t)N + i;
      ola_add_rows(row, N, kf, s, num);
    }
    out[n] = ola_result(num, den, norm);
  }
}

// ======================================================================================
// Routed overlap-add: the same y (W, K, N), folded onto NT tracks of L samples each -> out (NT, L) float64.
//   num[t, n] = sum_f ws[n - f hop] * sum_{k < K_f, bit k of masks[t, f] set} y[f, k, n - f hop]
//   A track with no term at n gives num = 0.0 and so exactly 0.0.
// masks (NT, W) 64-bit words: bit k of masks[t, f] routes row k of frame f to track t (K <= 64, checked on the host).  A
// mask instead of a (W, K) label array: with labels a lane would compare all K labels of a frame for the ~K / NT rows it
// loads; with a mask it is one 8-byte load per frame -- the same address for every lane of a wavefront unless the
// wavefront straddles two frames' worth of n or two tracks -- and then a walk over the set bits.  Bits at or above K_f
// are cut off (ola_cut), the walk (ola_add_masked) takes the lowest set bit with ctz and clears it with m & (m - 1), so
// bit 63 is a row like any other.  Masks may overlap (the row is added to every track that names it); rows behind K_f
// or in no mask are never read.
// One lane owns one (t, n) and walks frames in ascending f, rows in ascending k, accumulating in float64: one fixed
// order, no atomics, the same bits on every run.  Items are flat over NT * L, so the lanes of a wavefront may lie in two
// tracks (L not a multiple of 64): every lane derives its own (t, n) and loads its own mask word.  Grid-stride loop.
// ======================================================================================
template <typename T>
__global__ __launch_bounds__(kFramesBlock) void k_overlap_add_tracks(const T* __restrict__ y, int64_t W, int K, int N, int hop,
                                                                    int64_t L, const int* __restrict__ counts,
                                                                    const unsigned long long* __restrict__ masks,
                                                                    int64_t NT, const double* __restrict__ wa,
                                                                    const double* __restrict__ ws, int norm,
                                                                    double* __restrict__ out) {
  const int64_t total = NT * L;
  const int64_t stride = (int64_t)gridDim.x * kFramesBlock;
  for (int64_t item = (int64_t)blockIdx.x * kFramesBlock + threadIdx.x; item < total; item += stride) {
    const int64_t t = item / L;
    const int64_t n = item - t * L;
    int64_t f_lo, f_hi;
    ola_frame_span(n, N, hop, W, f_lo, f_hi);
    const unsigned long long* mrow = masks + t * W;
    double num = 0.0, den = 0.0;
    for (int64_t f = f_lo; f <= f_hi; ++f) {
      const int i = (int)(n - f * hop);
      const int kf = counts ? ola_clip(counts[f], K) : K;
      const double s = ola_window(i, wa, ws, den);
      const T* row = y + (f * K) * (int64_t)N + i;
      ola_add_masked(row, N, ola_cut(mrow[f], kf), s, num);
    }
    out[item] = ola_result(num, den, norm);
  }
}

// ======================================================================================
// Routed overlap-add of periodic segments: seg (W, ccap) float64 holds ONE period of every block -- the layout
// k_qo_extract writes: block a of frame f is p(f, a) = periods[f, a] doubles at off(f, a) = sum_{b < a} p(f, b) -- and is
// tiled on the fly onto NT tracks of L samples -> out (NT, L) float64.  With i = n - f hop:
//   num[t, n] = sum_f ws[i] * sum_{a < C_f, bit a of masks[t, f] set} seg[f, off(f, a) + (i mod p(f, a))]
//   C_f = counts[f] clipped to [0, min(pcap, 64)].  The dense (W, K, N) rows k_overlap_add_tracks reads never exist: a
//   frame costs sum p doubles, not K N.
// One lane owns one (t, n) and walks frames in ascending f, blocks in ascending a, accumulating in float64: the order
// of k_overlap_add_tracks, no atomics, the same bits on every run.  Flat grid-stride loop over NT * L, int64 addressing.
// The offsets are the running sum of the periods the walk has passed, so a lane reads periods[f, a] for every a up to
// the highest bit of its (cut) mask word -- the same address for every lane of a wavefront that lies in one frame and
// track, one cache line per 16 blocks -- and seg only for the blocks its mask names.
// Stop rule: the device arrays are whatever the caller left there, so the walk of a frame ends at the first block with
// p < 1 or off + p > ccap; that block and the ones behind it contribute nothing.  Every read of seg is therefore at
// off + r with 0 <= r < p and off + p <= ccap: inside the frame's row.  Elements behind sum p, blocks behind C_f and
// blocks in no mask of the lane's track are never read.
// i mod p: 0 <= i < N < 2^31 and, by the stop rule, 1 <= p <= ccap <= 2^24, so the unsigned 32-bit remainder is exact
// (p > N gives i).  It is the compiler's expansion (a float reciprocal and two corrections, ~20 VALU instructions per
// term): measured against the gathers in tools/short_time_qo_bench.py, DESIGN.md 4.2h.
// ======================================================================================
__global__ __launch_bounds__(kFramesBlock) void k_overlap_add_periodic(const double* __restrict__ seg, const int* __restrict__ periods,
                                                                      const int* __restrict__ counts,
                                                                      const unsigned long long* __restrict__ masks, int64_t W,
                                                                      int pcap, int ccap, int64_t NT, int N, int hop, int64_t L,
                                                                      const double* __restrict__ wa, const double* __restrict__ ws,
                                                                      int norm, double* __restrict__ out) {
  const int64_t total = NT * L;
  const int64_t stride = (int64_t)gridDim.x * kFramesBlock;
  const int cmax = pcap < 64 ? pcap : 64;
  for (int64_t item = (int64_t)blockIdx.x * kFramesBlock + threadIdx.x; item < total; item += stride) {
    const int64_t t = item / L;
    const int64_t n = item - t * L;
    int64_t f_lo, f_hi;
    ola_frame_span(n, N, hop, W, f_lo, f_hi);
    const unsigned long long* mrow = masks + t * W;
    double num = 0.0, den = 0.0;
    for (int64_t f = f_lo; f <= f_hi; ++f) {
      const unsigned i = (unsigned)(n - f * hop);
      const int cf = ola_clip(counts[f], cmax);
      const double s = ola_window(i, wa, ws, den);
      const unsigned long long m = ola_cut(mrow[f], cf);
      if (m == 0ull) continue;
      const int last = 63 - __builtin_clzll(m);  // < cf <= pcap
      const int* prow = periods + f * (int64_t)pcap;
      const double* srow = seg + f * (int64_t)ccap;
      int64_t off = 0;
      for (int a = 0; a <= last; ++a) {
        const int p = prow[a];
        if (p < 1 || off + p > ccap) break;  // the stop rule
        if ((m >> a) & 1ull) num += s * srow[off + (int64_t)(i % (unsigned)p)];
        off += p;
      }
    }
    out[item] = ola_result(num, den, norm);
  }
}

// ======================================================================================
// Overlap-add in frame blocks: k_overlap_add_block adds the frames f0 .. f0 + Wb - 1 of a recording into a running sum
// acc (NT, L) float64, k_overlap_add_finish turns the running sum into the result.  Everything about the block is
// block-local: y (Wb, K, N) of T, counts (Wb), masks (NT, Wb); only f0 places it in the recording.
//   Routed = false (NT = 1): acc[0, n] += the terms k_overlap_add adds for the frames of the block (ola_add_rows); K
//     may exceed 64.
//   Routed = true: acc[t, n] += the terms k_overlap_add_tracks adds for them (ola_cut, ola_add_masked).
// The work items are the NT * (n1 - n0) samples of the block's span, n0 = f0 hop, n1 = min(L, (f0 + Wb - 1) hop + N);
// a sample outside the span is neither read nor written.  A lane loads num = acc[t, n], walks the frames
// max(f_lo(n), f0) .. min(f_hi(n), f0 + Wb - 1) in ascending f -- f_lo / f_hi are those of the whole recording; its last
// frame can only cut f_hi where the block's last frame does already -- with the row walk of the one-launch kernels, and
// stores num back.  den is not touched here: it depends on n, W, hop and the windows alone, and k_overlap_add_finish
// recomputes it by the walk of the one-launch kernels over all W frames (ola_window only) and writes
// out[t, n] = ola_result(acc[t, n], den[n], norm); out may be acc itself, each lane reads its own element before it
// writes it.
// Contract (nothing here can check it): acc is zeroed before the first block, the blocks are applied on one stream in
// ascending f0, and every frame belongs to exactly one block.  A lane of a later block then continues the walk of its
// sample where the lane of the block before left it: the same additions in the same order as one launch over the whole
// (W, K, N) array, whose `num = 0.0` is the zeroed acc.  After finish the result is, bit for bit, that of k_overlap_add
// (Routed = false) or of k_overlap_add_tracks (Routed = true).
// No LDS, int64 index arithmetic, flat grid-stride loops.  A block moves 2 * 8 * NT * (n1 - n0) bytes of acc on top of
// the rows it reads.
// ======================================================================================
template <typename T, bool Routed>
__global__ __launch_bounds__(kFramesBlock) void k_overlap_add_block(const T* __restrict__ y, int64_t Wb, int K, int N, int hop,
                                                                   int64_t L, int64_t f0, const int* __restrict__ counts,
                                                                   const unsigned long long* __restrict__ masks, int64_t NT,
                                                                   const double* __restrict__ ws, double* __restrict__ acc) {
  const int64_t n0 = f0 * hop;
  const int64_t end = (f0 + Wb - 1) * hop + N;
  const int64_t span = (end < L ? end : L) - n0;
  const int64_t total = NT * span;
  const int64_t stride = (int64_t)gridDim.x * kFramesBlock;
  for (int64_t item = (int64_t)blockIdx.x * kFramesBlock + threadIdx.x; item < total; item += stride) {
    const int64_t t = item / span;
    const int64_t n = n0 + (item - t * span);
    int64_t f_lo, f_hi;
    ola_frame_span(n, N, hop, f0 + Wb, f_lo, f_hi);
    if (f_lo < f0) f_lo = f0;
    double num = acc[t * L + n], den = 0.0;  // (den: what ola_window wants; dead here)
    for (int64_t f = f_lo; f <= f_hi; ++f) {
      const int64_t fb = f - f0;
      const int i = (int)(n - f * hop);
      const int kf = counts ? ola_clip(counts[fb], K) : K;
      const double s = ola_window(i, nullptr, ws, den);
      const T* row = y + (fb * K) * (int64_t)N + i;
      if constexpr (Routed)
        ola_add_masked(row, N, ola_cut(masks[t * Wb + fb], kf), s, num);
      else
        ola_add_rows(row, N, kf, s, num);
    }
    acc[t * L + n] = num;
  }
}

// (acc and out may be one array: no __restrict__ on either)
__global__ __launch_bounds__(kFramesBlock) void k_overlap_add_finish(const double* acc, int64_t NT, int N, int hop, int64_t L,
                                                                    int64_t W, const double* __restrict__ wa,
                                                                    const double* __restrict__ ws, int norm, double* out) {
  const int64_t total = NT * L;
  const int64_t stride = (int64_t)gridDim.x * kFramesBlock;
  for (int64_t item = (int64_t)blockIdx.x * kFramesBlock + threadIdx.x; item < total; item += stride) {
    const int64_t n = item % L;
    int64_t f_lo, f_hi;
    ola_frame_span(n, N, hop, W, f_lo, f_hi);
    double den = 0.0;
    for (int64_t f = f_lo; f <= f_hi; ++f) ola_window((int)(n - f * hop), wa, ws, den);
    out[item] = ola_result(acc[item], den, norm);
  }
}

}  // namespace ph

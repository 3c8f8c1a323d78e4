// Best path through a time-period map: k_period_path runs the dynamic programme that links one frame's period to the
// next -- maximal summed salience minus a penalty on jumps -- over a cost table c (W frames, P periods), and traces the
// path back, in one launch.  One workgroup owns one map; the grid is the batch of R maps.
//
//   c'[f][j]   = isfinite(c[f][j]) ? c[f][j] : -inf                 (NaN, +inf and -inf are all "forbidden")
//   D[0][j]    = c'[0][j]
//   best[f][j] = max over o of D[f-1][j+o] - pen[|o|], 0 <= j+o < P, pen[o] = jump * o for o = 0 .. band;
//                offsets tried in the order 0, -1, +1, -2, +2, ... -band, +band, a candidate replaces the current one
//                only if strictly greater; bp[f][j] = the offset kept
//   D[f][j]    = c'[f][j] + best[f][j]
//   end        = the first (lowest j) maximum of D[W-1];  score = D[W-1][end]
//   path[W-1]  = end;  path[f-1] = path[f] + bp[f][path[f]];  value[f] = c[f][path[f]]
//   score == -inf (some frame had no reachable state): status PH_ST_NO_PERIOD, path all -1, values 0.
//
// Every product, difference and sum above is one fp64 operation rounded once: pen is a table filled once (a product
// that feeds a store cannot be contracted with anything), the kernel body is compiled with contraction off, and max and
// the comparisons are exact.  The result therefore does not depend on how the states are spread over the threads: path,
// score and values are, bit for bit, those of a plain loop over the lines above.
//
// Forward pass.  The states of a frame are spread over the workgroup, state j = threadIdx.x + s * blockDim.x for
// s < NS = path_states(P), in a workgroup of path_block(P) threads -- cut so that every thread holds NS states --
// so for one offset the lanes of a wavefront read consecutive doubles of D[f-1]: ds_read_b64 at a stride of
// 8 bytes, conflict-free in each 32-lane half whatever the offset.  D[f-1] and D[f] are two LDS rows of P + 2 * 64
// doubles whose 64 cells on either side hold -inf for the whole launch: the inner loop has no bounds test, and a halo
// candidate (-inf) never replaces anything (nothing compares strictly below it), so a kept offset always stays inside
// the row.  One __syncthreads per frame: frame f reads row (f-1) & 1 and writes row f & 1.  The cost row of frame
// f + 1 is requested from HBM before the barrier of frame f and first used at the end of frame f + 1, so it lands
// behind that frame's work.
// Back-pointers are int8.  A frame's P of them are written as bytes into one of two LDS staging rows and go to the
// (R, W, Pb) workspace one frame later -- after the barrier that made the staging row whole -- as one dword per lane,
// consecutive lanes consecutive dwords; Pb = P rounded up to 16, so every workspace row starts 16-byte aligned.
// Row 0 of a map's workspace is never written or read (frame 0 has no back-pointer).
//
// Backtrace.  A dependent HBM load per frame would cost about a microsecond each.  Instead the workgroup copies a tile
// of `tile` whole workspace rows (16-byte vectors) into the LDS the D rows no longer need, one lane walks the tile there
// (one dependent LDS byte read per frame) and leaves the path of the tile in LDS, and the workgroup stores that piece of
// path and gathers its values from the cost table.  Two barriers per tile.  The tile height is path_carve's `tile`.
//
// Included by ph_kernels.h.  Index arithmetic that involves R, W or ld is int64.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "ph_device.h"

namespace ph {

#ifndef PH_PATH_UNROLL
#define PH_PATH_UNROLL 1
#endif

constexpr int kPathHalo = 64;            // forbidden cells on either side of a D row = the largest band
constexpr int kPathMaxP = 8192;          // two D rows of kPathMaxP + 2 * kPathHalo doubles are 133 KB of the 160 KB
constexpr int kPathMaxStates = 8;        // states of a frame per thread: kPathMaxP / 1024
constexpr size_t kPathMinRegion = 64 * 1024;  // the backtrace tile gets at least this (two workgroups still share a CU)

// bytes of one back-pointer row, in LDS and in the workspace
__host__ __device__ inline int path_row_bytes(int P) { return (P + 15) & ~15; }

// states of a frame per thread: as few as 1024 threads allow, 1 .. kPathMaxStates
__host__ __device__ inline int path_states(int P) { return (P + 1023) / 1024; }

// threads per workgroup: what gives every thread path_states(P) states, in whole wavefronts -- P = 1365 is 704 threads
// with two states each, not 1024 of which a third has two.  The offset loop has no branch, so a thread without a state
// would do a state's work for nothing.
__host__ __device__ inline int path_block(int P) {
  const int ns = path_states(P);
  return ((P + ns - 1) / ns + kWave - 1) & ~(kWave - 1);
}

// LDS of k_period_path.  The penalties and the reduction scratch live for the whole launch; behind them one region
// holds the forward pass (two D rows with their halos, two staging rows of back-pointers) and then, over the same
// bytes, the backtrace (a tile of `tile` workspace rows and the path of the tile).  The region is as large as the
// forward pass needs, at least kPathMinRegion; `tile` is what fits it -- the one place that number is derived -- or
// `tile_cap` when that is smaller (tile_cap < 1: no cap; a cap of 1 is the untiled walk the benchmark compares with).
struct PathLds {
  double* pen;    // band + 1 penalties (room for kPathHalo + 1)
  double* red_v;  // one maximum per wavefront
  int* red_i;     // and its state
  double* d[2];   // D rows, each P + 2 * kPathHalo doubles; state j is d[k][kPathHalo + j]
  signed char* stage[2];  // back-pointers of one frame, Pb bytes
  signed char* rows;      // backtrace: tile * Pb bytes
  int* piece;             // backtrace: path[lo - 1 + k] of the tile's row k
  int tile;
  size_t bytes;
};
template <class C>
__host__ __device__ __forceinline__ PathLds path_carve(C cv, int P, int tile_cap) {
  PathLds L;
  const size_t Pb = (size_t)path_row_bytes(P);
  L.pen = cv.template take<double>(kPathHalo + 1);
  L.red_v = cv.template take<double>(kMaxWaves);
  L.red_i = cv.template take<int>(kMaxWaves);
  const size_t region_at = cv.off;
  C fw = cv.at(region_at);
  L.d[0] = fw.template take<double>((size_t)P + 2 * kPathHalo);
  L.d[1] = fw.template take<double>((size_t)P + 2 * kPathHalo);
  L.stage[0] = fw.template take<signed char>(Pb);
  L.stage[1] = fw.template take<signed char>(Pb);
  const size_t forward = fw.off - region_at;
  const size_t region = forward > kPathMinRegion ? forward : kPathMinRegion;
  // tile rows of Pb bytes and one int each, the ints rounded up to the 16 bytes of a piece
  int tile = (int)((region - 16) / (Pb + sizeof(int)));
  if (tile_cap >= 1 && tile > tile_cap) tile = tile_cap;
  L.tile = tile;
  C bt = cv.at(region_at);
  L.rows = bt.template take<signed char>((size_t)tile * Pb);
  L.piece = bt.template take<int>((size_t)tile);
  L.bytes = region_at + region;
  return L;
}

__device__ __forceinline__ double path_finite_or_forbidden(double v) {
  const unsigned long long b = (unsigned long long)__double_as_longlong(v);
  return ((b >> 52) & 0x7ffull) == 0x7ffull ? -INFINITY : v;
}

// (v, i) <- the larger of (v, i) and (ov, oi); equal values keep the lower state
__device__ __forceinline__ void path_take_max(double& v, int& i, double ov, int oi) {
  if (ov > v || (ov == v && oi < i)) {
    v = ov;
    i = oi;
  }
}

template <int NS>
__global__ __launch_bounds__(1024) void k_period_path(const double* __restrict__ cost, int64_t W, int P, int64_t ld, int band,
                                                      double jump, int tile_cap, signed char* __restrict__ ws,
                                                      int* __restrict__ path, double* __restrict__ value,
                                                      double* __restrict__ score, int* __restrict__ status) {
#pragma clang fp contract(off)
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const PathLds L = path_carve(Carve(smem), P, tile_cap);
  const int tid = threadIdx.x, nt = blockDim.x;
  const int lane = tid & (kWave - 1), wv = tid >> 6, nw = nt >> 6;
  const int Pb = path_row_bytes(P);
  const int64_t r = blockIdx.x;
  const double* c = cost + r * W * ld;      // the map: row f at c + f * ld
  signed char* wsr = ws + r * W * (int64_t)Pb;  // its back-pointers: row f at wsr + f * Pb
  int* prow = path + r * W;
  double* vrow = value ? value + r * W : nullptr;

  // ---- once: the penalties, the halos of both rows, the staging rows' bytes behind P
  for (int o = tid; o <= band; o += nt) L.pen[o] = jump * (double)o;
  for (int i = tid; i < 2 * kPathHalo; i += nt) {
    const int at = i < kPathHalo ? i : P + i;  // kPathHalo cells before state 0, kPathHalo behind state P - 1
    L.d[0][at] = -INFINITY;
    L.d[1][at] = -INFINITY;
  }
  for (int i = P + tid; i < Pb; i += nt) L.stage[0][i] = L.stage[1][i] = 0;

  // ---- frame 0, and the cost row of frame 1 on its way
  double cur[NS];
#pragma unroll
  for (int s = 0; s < NS; ++s) {
    const int j = tid + s * nt;
    if (j < P) L.d[0][kPathHalo + j] = path_finite_or_forbidden(c[j]);
    cur[s] = (W > 1 && j < P) ? c[ld + j] : 0.0;
  }
  __syncthreads();

  // ---- forward pass: one barrier per frame
  // (the rows by arithmetic, not by an index into L.d / L.stage: a runtime index would put the struct into scratch)
  const size_t drow = (size_t)(L.d[1] - L.d[0]), srow = (size_t)(L.stage[1] - L.stage[0]);
  for (int64_t f = 1; f < W; ++f) {
    const int par = (int)(f & 1);
    const double* dp = L.d[0] + (par ? 0 : drow) + kPathHalo;
    double* dc = L.d[0] + (par ? drow : 0) + kPathHalo;
    signed char* st = L.stage[0] + (par ? srow : 0);
    // the staging row the last frame filled goes out, a dword per lane (frame 0 has none)
    if (f > 1) {
      const uint32_t* from = reinterpret_cast<const uint32_t*>(L.stage[0] + (par ? 0 : srow));
      uint32_t* to = reinterpret_cast<uint32_t*>(wsr + (f - 1) * (int64_t)Pb);
      for (int i = tid; i < Pb / 4; i += nt) to[i] = from[i];
    }
    // (a thread's states behind P - 1 work on state P - 1 and store nothing: no branch inside the offset loop, so the
    // reads of several offsets are in flight together)
    double best[NS];
    int off[NS];
    const double* at[NS];
    const double pen0 = L.pen[0];
#pragma unroll
    for (int s = 0; s < NS; ++s) {
      const int j = tid + s * nt;
      at[s] = dp + (j < P ? j : P - 1);
      best[s] = at[s][0] - pen0;
      off[s] = 0;
    }
    // (not unrolled: hipcc merges the reads of the offsets o and o + 1 of an unrolled body into ds_read2_b64 pairs, which
    // take more LDS cycles than two ds_read_b64, and needs twice the registers at NS = 8; -DPH_PATH_UNROLL=n builds that
    // loop -- it measured the same, profiles/period_path/README.md)
#pragma unroll PH_PATH_UNROLL
    for (int o = 1; o <= band; ++o) {
      const double pn = L.pen[o];
#pragma unroll
      for (int s = 0; s < NS; ++s) {
        const double lo = at[s][-o] - pn, hi = at[s][o] - pn;
        if (lo > best[s]) {
          best[s] = lo;
          off[s] = -o;
        }
        if (hi > best[s]) {
          best[s] = hi;
          off[s] = o;
        }
      }
    }
#pragma unroll
    for (int s = 0; s < NS; ++s) {
      const int j = tid + s * nt;
      if (j < P) {
        dc[j] = path_finite_or_forbidden(cur[s]) + best[s];
        st[j] = (signed char)off[s];
      }
      // the next cost row: asked for before this frame's barrier, used at the end of the next frame
      cur[s] = (f + 1 < W && j < P) ? c[(f + 1) * ld + j] : 0.0;
    }
    __syncthreads();
  }
  if (W > 1) {  // the last frame's staging row
    const uint32_t* from = reinterpret_cast<const uint32_t*>(((W - 1) & 1) ? L.stage[1] : L.stage[0]);
    uint32_t* to = reinterpret_cast<uint32_t*>(wsr + (W - 1) * (int64_t)Pb);
    for (int i = tid; i < Pb / 4; i += nt) to[i] = from[i];
  }

  // ---- end = the first maximum of D[W - 1]
  const double* dl = (((W - 1) & 1) ? L.d[1] : L.d[0]) + kPathHalo;
  double bv = -INFINITY;
  int bi = 0x7fffffff;
#pragma unroll
  for (int s = 0; s < NS; ++s) {
    const int j = tid + s * nt;
    if (j < P) path_take_max(bv, bi, dl[j], j);
  }
  for (int d = kWave / 2; d >= 1; d >>= 1) {
    const double ov = __shfl_xor(bv, d, kWave);
    const int oi = __shfl_xor(bi, d, kWave);
    path_take_max(bv, bi, ov, oi);
  }
  if (lane == 0) {
    L.red_v[wv] = bv;
    L.red_i[wv] = bi;
  }
  __syncthreads();  // (also: every back-pointer row is stored, the D rows are dead)
  bv = L.red_v[0];
  bi = L.red_i[0];
  for (int k = 1; k < nw; ++k) path_take_max(bv, bi, L.red_v[k], L.red_i[k]);
  const bool reachable = bv > -INFINITY;  // (every thread holds the same bv, bi)
  if (tid == 0) {
    score[r] = bv;
    status[r] = reachable ? PH_ST_OK : PH_ST_NO_PERIOD;
  }
  if (!reachable) {
    for (int64_t f = tid; f < W; f += nt) {
      prow[f] = -1;
      if (vrow) vrow[f] = 0.0;
    }
    return;
  }
  if (tid == 0) {
    prow[W - 1] = bi;
    if (vrow) vrow[W - 1] = c[(W - 1) * ld + bi];
  }

  // ---- backtrace, a tile of workspace rows at a time: rows lo .. hi give path[lo - 1 .. hi - 1]
  int j = bi;  // path[hi]; only thread 0's copy is carried on
  for (int64_t hi = W - 1; hi >= 1;) {
    const int n = hi < L.tile ? (int)hi : L.tile;
    const int64_t lo = hi - n + 1;
    // (no barrier here: the rows are read by thread 0 alone, before the barrier that ends the walk below, and the piece
    // is written again only behind the next barrier, which every thread reaches with its stores of this piece issued)
    {
      const uint4* from = reinterpret_cast<const uint4*>(wsr + lo * (int64_t)Pb);
      uint4* to = reinterpret_cast<uint4*>(L.rows);
      const int nv = n * (Pb / 16);
      for (int i = tid; i < nv; i += nt) to[i] = from[i];
    }
    __syncthreads();
    if (tid == 0) {
      for (int k = n - 1; k >= 0; --k) {
        j += L.rows[(size_t)k * Pb + j];
        j = j < 0 ? 0 : j >= P ? P - 1 : j;  // (a kept offset stays inside the row; this holds whatever the workspace holds)
        L.piece[k] = j;
      }
    }
    __syncthreads();
    for (int k = tid; k < n; k += nt) {
      const int64_t f = lo - 1 + k;
      const int pj = L.piece[k];
      prow[f] = pj;
      if (vrow) vrow[f] = c[f * ld + pj];
    }
    hi = lo - 1;
  }
}

}  // namespace ph

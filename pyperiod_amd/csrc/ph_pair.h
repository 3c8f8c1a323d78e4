// Window-pair screen of the all-p sweep (gfx950 / CDNA4 only).
//
// The norm sweeps of ph_device.h are VALU-issue bound: per ds_read_b64 the fold spends one v_add_f64 plus
// 2-3 instructions of addressing, masking and reduction.  Here TWO windows share a workgroup and every LDS
// element is the pair {fl32(a[n] * sa), fl32(b[n] * sb)} of their float-rounded (power-of-two scaled) samples:
// one ds_read_b64 brings a sample of both windows, v_pk_add_f32 / v_pk_fma_f32 fold both, and every address,
// mask, weight and cross-lane instruction of a pass is shared between them -- the instruction stream of one
// fp64 pass now serves two windows.  Always 8-byte aligned, no shifted copies, same register footprint as the
// fp64 fold (a float pair is as wide as a double).  The window is followed by kPad ZEROED pairs: the chunk that holds
// the cut of a period reads the missing last sample of its short residues from there (pair_rows_group, STR).
//
// The float values only SCREEN the candidates of an m_best iteration (Periods.py:501-515): a rigorous radius
// (pair_radius) bounds |screen - exact|, and the periods whose upper bound reaches the best lower bound are
// re-evaluated in fp64 by the kernel (k_mbest_step1_pair in ph_mbest.h), which decides on those values.
//
// Plain m_best screens only the periods in (p_hi / 2, p_hi]: the projection onto the d-periodic vectors is never
// longer than the one onto the m-periodic vectors when d | m, so a period with a multiple in range needs a look (in
// fp64) only when that multiple survives -- the cover rule, derived at pair_cover_slack below.  At p = 2 ... 1365,
// N = 4096 that is 683 few-row single passes (R = 4, 5, 6) per sweep instead of 800 mixed ones.
#pragma once

#include "ph_device.h"

namespace ph {

typedef float f2 __attribute__((ext_vector_type(2)));
typedef const volatile __attribute__((address_space(3))) f2* pair_ptr;

// float geometry of a period for the screen (host table next to PGeom)
struct PGeomF {
  int rows;       // R = ceil(N / p)
  int nfull;      // residues j < nfull own R samples, the others R-1
  float w_full;   // fl32(1 / R)
  float w_short;  // fl32(1 / (R-1))  (0 when R == 1)
};

__device__ __forceinline__ f2 f2_make(float a, float b) {
  f2 r;
  r.x = a;
  r.y = b;
  return r;
}
__device__ __forceinline__ f2 f2_zero() { return f2_make(0.0f, 0.0f); }
// zero written into its registers at this point (the compiler's own zero may be one pair made in front of the kernel's
// main loop and -- at the register cap -- brought back from a spill at every use)
__device__ __forceinline__ f2 f2_zero_at_use() {
  f2 r;
  asm volatile("v_mov_b64 %0, 0" : "=v"(r));
  return r;
}
__device__ __forceinline__ f2 f2_fma(f2 a, f2 b, f2 c) { return __builtin_elementwise_fma(a, b, c); }
__device__ __forceinline__ f2 f2_max(f2 a, f2 b) { return __builtin_elementwise_max(a, b); }
// accumulate one residue sum t: sum of squares (norm screens) or largest square (MX: the max |S| screen of
// best_correlation, Periods.py:327-331)
template <bool MX>
__device__ __forceinline__ f2 f2_acc(f2 part, f2 t) {
  return MX ? f2_max(part, t * t) : f2_fma(t, t, part);
}

template <int CTRL>
__device__ __forceinline__ f2 dpp_f2(f2 v) {
  const int a = __builtin_amdgcn_update_dpp(0, __float_as_int(v.x), CTRL, 0xF, 0xF, false);
  const int b = __builtin_amdgcn_update_dpp(0, __float_as_int(v.y), CTRL, 0xF, 0xF, false);
  return f2_make(__int_as_float(a), __int_as_float(b));
}

// Lane index, recomputed where it is needed (two VALU) instead of kept live across the folds: as a long-lived
// value it was spilled, and every segment of every pass started with a scratch reload in front of its first LDS
// address.  The volatile asm keeps the compiler from hoisting it back into one register.
__device__ __forceinline__ int pair_lane() {
  int l;
  asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(l));
  return l;
}

// ---------------------------------------------------------------- few-row single passes (R <= 6)
// STR (with MASK): the last chunk STRADDLES the cut of the period -- its lanes below `nvalid` are residues with NR
// samples, the lanes from there up to `nvalid2` residues with NR - 1 whose last-row load falls into the zeroed pad
// behind the window (index (NR-1) p + j >= N exactly for those j, and < N + 64): one chunk serves both count classes,
// and the part with the short residues starts on a chunk boundary.  Their squares go to `part2`.
template <int NR, int C, bool MASK, bool MX, bool STR = false>
__device__ __forceinline__ void pair_rows_group(pair_ptr ptr, int p, int nvalid, int nvalid2, int lane, f2& part, f2& part2) {
  f2 v[NR][C];
#pragma unroll
  for (int r = 0; r < NR; ++r)
#pragma unroll
    for (int c = 0; c < C; ++c) v[r][c] = ptr[r * p + 64 * c];
  __builtin_amdgcn_s_waitcnt(0xC07F);  // lgkmcnt(0)
  __builtin_amdgcn_sched_barrier(0);
#pragma unroll
  for (int c = 0; c < C; ++c) {
    f2 t = v[0][c];
#pragma unroll
    for (int r = 1; r < NR; ++r) t += v[r][c];
    if (MASK && c == C - 1) {  // a masked group is cut in its LAST chunk only
      const int col = 64 * c + lane;
      if (STR) {
        const f2 t2 = (col >= nvalid && col < nvalid2) ? t : f2_zero();
        part2 = f2_acc<MX>(part2, t2);
      }
      t = (col < nvalid) ? t : f2_zero();
    }
    part = f2_acc<MX>(part, t);
  }
}
template <int NR, int C, bool MASK, bool MX>
__device__ __forceinline__ void pair_rows_group(pair_ptr ptr, int p, int nvalid, int lane, f2& part) {
  pair_rows_group<NR, C, MASK, MX, false>(ptr, p, nvalid, nvalid, lane, part, part);
}

// ---------------------------------------------------------------- general segmented group (see seg_group)
// STR: as in pair_rows_group -- the lanes of the last chunk from `nvalid` up to `nvalid2` are residues with one sample
// fewer (their last row reads the zeroed pad); their squares take the weights `wgt2` and go to `part2`.
template <int M, int U, int C, bool MASK, bool MX, bool STR = false>
__device__ __forceinline__ void pair_seg_group(pair_ptr ptr, int p, int nrows, int nvalid, int nvalid2, int lane,
                                               const float (&wgt)[7], const float (&wgt2)[7], f2 (&part)[3], f2 (&part2)[3]) {
  static_assert(U % M == 0, "a row block must cover whole class cycles");
  f2 a[M][C];
  int r = 0;
  if (nrows >= U) {  // the first row block initialises the class sums (no zeroing, no adds)
    f2 v[U][C];
#pragma unroll
    for (int u = 0; u < U; ++u)
#pragma unroll
      for (int c = 0; c < C; ++c) v[u][c] = ptr[u * p + 64 * c];
    __builtin_amdgcn_s_waitcnt(0xC07F);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int u = 0; u < M; ++u)
#pragma unroll
      for (int c = 0; c < C; ++c) {
        a[u][c] = v[u][c];
#pragma unroll
        for (int w = u + M; w < U; w += M) a[u][c] += v[w][c];
      }
    ptr += U * p;
    r = U;
  } else {
#pragma unroll
    for (int u = 0; u < M; ++u)
#pragma unroll
      for (int c = 0; c < C; ++c) a[u][c] = f2_zero();
  }
  for (; r + U <= nrows; r += U) {
    f2 v[U][C];
#pragma unroll
    for (int u = 0; u < U; ++u)
#pragma unroll
      for (int c = 0; c < C; ++c) v[u][c] = ptr[u * p + 64 * c];
    __builtin_amdgcn_s_waitcnt(0xC07F);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int u = 0; u < U; ++u)
#pragma unroll
      for (int c = 0; c < C; ++c) a[u % M][c] += v[u][c];
    ptr += U * p;
  }
  if (U > 1) {
    const int rem = nrows - r;
#pragma unroll
    for (int u = 0; u < U - 1; ++u) {
      if (u < rem) {
        asm volatile("" ::: "memory");  // keep the wave-uniform branch (see seg_group)
        f2 v[C];
#pragma unroll
        for (int c = 0; c < C; ++c) v[c] = ptr[u * p + 64 * c];
        __builtin_amdgcn_s_waitcnt(0xC07F);
#pragma unroll
        for (int c = 0; c < C; ++c) a[u % M][c] += v[c];
      }
    }
  }
  // squares of the class sums of chunk c into `pt` with the weights `w`
  auto fin = [&](int c, const float (&w)[7], f2 (&pt)[3]) {
    if (M == 1) {
      pt[0] = f2_acc<MX>(pt[0], a[0][c]);
    } else if (MX) {  // max |S| of p, 2p and (M == 4) 4p from the class sums; no count weights
      const f2 e = M == 4 ? a[0][c] + a[2 % M][c] : a[0][c], o = M == 4 ? a[1 % M][c] + a[3 % M][c] : a[1 % M][c];
      pt[0] = f2_acc<true>(pt[0], e + o);
      pt[1] = f2_acc<true>(f2_acc<true>(pt[1], e), o);
      if (M == 4) {
#pragma unroll
        for (int u = 0; u < M; ++u) pt[2] = f2_acc<true>(pt[2], a[u][c]);
      }
    } else if (M == 2) {
      const f2 e = a[0][c], o = a[1 % M][c], t = e + o;
      pt[0] = f2_fma(t, t, pt[0]);
      pt[1] = f2_fma(e, e, pt[1]);
      pt[2] = f2_fma(o, o, pt[2]);
    } else {
      const f2 e = a[0][c] + a[2 % M][c], o = a[1 % M][c] + a[3 % M][c], t = e + o;
      pt[0] = f2_fma(t, t * w[0], pt[0]);
      pt[1] = f2_fma(e, e * w[1], pt[1]);
      pt[1] = f2_fma(o, o * w[2], pt[1]);
#pragma unroll
      for (int u = 0; u < M; ++u) pt[2] = f2_fma(a[u][c], a[u][c] * w[3 + u], pt[2]);
    }
  };
#pragma unroll
  for (int c = 0; c < C; ++c) {
    if (MASK && c == C - 1) {
      // a masked group holds exactly the chunks that are left: only the last one is cut -- one class without a straddle
      // by zeroing its sum, otherwise by running the squares under the lane masks (two scalar instructions, no selects)
      const int col = 64 * c + lane;
      if (M == 1) {  // (selects, not branches: the compiler turns the choice between the two arrays into a scratch pointer)
        part[0] = f2_acc<MX>(part[0], (col < nvalid) ? a[0][c] : f2_zero());
        if (STR) part2[0] = f2_acc<MX>(part2[0], (col >= nvalid && col < nvalid2) ? a[0][c] : f2_zero());
      } else if (col < nvalid) {
        fin(c, wgt, part);
      } else if (STR && col < nvalid2) {
        fin(c, wgt2, part2);
      }
    } else {
      fin(c, wgt, part);
    }
  }
}
template <int M, int U, int C, bool MASK, bool MX>
__device__ __forceinline__ void pair_seg_group(pair_ptr ptr, int p, int nrows, int nvalid, int lane,
                                               const float (&wgt)[7], f2 (&part)[3]) {
  pair_seg_group<M, U, C, MASK, MX, false>(ptr, p, nrows, nvalid, nvalid, lane, wgt, wgt, part, part);
}

// Per-lane partials of sum_j S_q[j]^2 / cnt_q[j] of BOTH windows, base period p >= 64; segment logic of seg_group.
// The pass is dispatched once, on the row count of the period, to straight-line code for both segments (see "passes
// with one dispatch" in ph_device.h: one CU has one scalar unit, and the screens kept it ~90 % busy; measured with
// tools/micro/pair_pass_bench.hip: 129 -> 71 scalar instructions per few-row pass, 100 -> 85 ns per pass and CU).
// columns [0, len) from `base` (lane included), NR samples each; STR: `len` is the cut of the period, and the chunk
// that holds it also takes the residues behind it (up to column `cols`) into `part2`
template <int NR, bool MX, bool STR = false>
__device__ __forceinline__ void pair_single_rows(pair_ptr base, int p, int len, int cols, int lane, f2& part, f2& part2) {
  constexpr int CG = NR <= 4 ? 4 : 2;
  const int whole = len >> 6;
  int c = 0;
  for (; c + CG <= whole; c += CG) pair_rows_group<NR, CG, false, MX>(base + 64 * c, p, 0, lane, part);
  for (; c < whole; ++c) {
    asm volatile("" ::: "memory");
    pair_rows_group<NR, 1, false, MX>(base + 64 * c, p, 0, lane, part);
  }
  const int rem = len & 63;
  if (rem) {
    asm volatile("" ::: "memory");
    pair_rows_group<NR, 1, true, MX, STR>(base + 64 * whole, p, rem, cols - 64 * whole, lane, part, part2);
  }
}

#ifndef PH_PAIR_U1
#define PH_PAIR_U1 2  // rows per load block of the many-row single passes
#endif
// one part of a pass: columns [0, len) from `base` (lane included), nrows samples each, squares into `part` with the
// weights `wgt`.  STR: `len` is the cut of the period; the chunk that holds it also takes the residues behind it, up to
// column `cols`, with the weights `wgt2` into `part2`.
template <int M, int U, bool MX, bool STR = false>
__device__ __forceinline__ void pair_multi_segment(pair_ptr base, int p, int len, int cols, int nrows, int lane,
                                                   const float (&wgt)[7], const float (&wgt2)[7], f2 (&part)[3], f2 (&part2)[3]) {
  constexpr int CM = (M == 4) ? 2 : 4;
  const int whole = len >> 6;
  int c = 0;
  for (; c + CM <= whole; c += CM) pair_seg_group<M, U, CM, false, MX>(base + 64 * c, p, nrows, 64 * CM, lane, wgt, part);
  const int left = len - 64 * c;  // < 64 CM columns
  const int left2 = cols - 64 * c;
  const pair_ptr at = base + 64 * c;
  if (CM == 4 && left > 128) {
    if (left > 192) pair_seg_group<M, U, (CM == 4 ? 4 : 1), true, MX, STR>(at, p, nrows, left, left2, lane, wgt, wgt2, part, part2);
    else pair_seg_group<M, U, (CM == 4 ? 3 : 1), true, MX, STR>(at, p, nrows, left, left2, lane, wgt, wgt2, part, part2);
  } else if (left > 64) {
    pair_seg_group<M, U, 2, true, MX, STR>(at, p, nrows, left, left2, lane, wgt, wgt2, part, part2);
  } else if (left > 0) {
    pair_seg_group<M, U, 1, true, MX, STR>(at, p, nrows, left, left2, lane, wgt, wgt2, part, part2);
  }
}

// Per-lane partials of sum_j S_p[j]^2 / cnt_p[j] (MX: max_j S_p[j]^2) of both windows, p >= 64.  The residues below
// the cut c = nfull own `rows` samples, the others one fewer; part A is every chunk up to and including the one that
// holds c - 1 (its lanes behind the cut ride along: STR), part B starts on the next chunk boundary -- ceil(p / 64)
// chunk columns per pass instead of ceil(c / 64) + ceil((p - c) / 64).
template <bool MX = false>
__device__ __forceinline__ f2 pair_pass_single(const f2* __restrict__ xs, int p, const PGeomF g) {
  const int lane = pair_lane();
  const int cut = g.nfull;
  const int acols = min(p, (cut + 63) & ~63), rest = p - acols;
  const pair_ptr a = (pair_ptr)xs + lane, b = a + acols;
  f2 sa = f2_zero(), sb = f2_zero();
  switch (g.rows) {
#define PH_SINGLE_CASE(R)                                              \
  case R:                                                              \
    pair_single_rows<R, MX, true>(a, p, cut, acols, lane, sa, sb);     \
    pair_single_rows<R - 1, MX>(b, p, rest, rest, lane, sb, sb);       \
    break;
    PH_SINGLE_CASE(2)
    PH_SINGLE_CASE(3)
    PH_SINGLE_CASE(4)
    PH_SINGLE_CASE(5)
    PH_SINGLE_CASE(6)
#undef PH_SINGLE_CASE
    default: {
      const float wgt[7] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
      f2 pa[3] = {f2_zero(), f2_zero(), f2_zero()}, pb[3] = {f2_zero(), f2_zero(), f2_zero()};
      pair_multi_segment<1, PH_PAIR_U1, MX, true>(a, p, cut, acols, g.rows, lane, wgt, wgt, pa, pb);
      if (rest > 0) pair_multi_segment<1, PH_PAIR_U1, MX>(b, p, rest, rest, g.rows - 1, lane, wgt, wgt, pb, pb);
      sa = pa[0];
      sb = pb[0];
      break;
    }
  }
  if (MX) return f2_max(sa, sb);
  return f2_fma(sa, f2_make(g.w_full, g.w_full), sb * g.w_short);
}

// (x < y) ? a : b of wave-uniform values on the scalar unit (the compiler's version of a float select under a scalar
// condition is two v_mov and a v_cndmask)
__device__ __forceinline__ float scalar_select_lt(int x, int y, float a, float b) {
  float r;
  asm("s_cmp_lt_i32 %1, %2\n\ts_cselect_b32 %0, %3, %4" : "=s"(r) : "s"(x), "s"(y), "s"(a), "s"(b) : "scc");
  return r;
}

// ---------------------------------------------------------------- shared-load pass: q and q + 64 from one set of reads
// A wavefront that folds period q holds a[r][c] = x[64 c + lane + r q] (row r, chunk column c).  Because
// (64 c + lane) + r (q + 64) = 64 (c + r) + lane + r q,
//   S_q   [64 c + lane] = sum_r a[r][c]        S_{q+64}[64 c + lane] = sum_r a[r][c + r]:
// the fold of q + 64 takes the same registers in the same lanes, one column further per row -- no cross-lane traffic,
// no second set of loads, packed adds.  The host pairs q with q + 64 only when ceil(N / q) = ceil(N / (q + 64)) = R,
// 3 <= R <= 6, and q has at least R + 1 chunk columns (build_plan, PassPlan m = 3), which keeps the bookkeeping regular:
//   weights  both periods take 1 / R below their cut and 1 / (R - 1) behind it;
//   cut      nfull(q + 64) = nfull(q) - 64 (R - 1): chunk c of q + 64 is complete when column c + R - 1 arrives, so
//            both periods cross their cut in the SAME column at the same lane -- the columns in front of it feed the
//            1 / R sums of both, the columns behind it the 1 / (R - 1) sums of both;
//   loads    row r, column c is read only while 64 c + r q < N, and only up to column ceil(q / 64) + r, the last one
//            q + 64 needs of it (rows up to R - 2 reach that column inside the window: pair_duo_tail).  Every sample
//            either period owns is read, what lies behind the window is a zero of the pad, and no read goes past
//            index N + 62.
// The wavefront streams over the columns and carries the R - 1 unfinished sums of q + 64 in `pend` (pend[k]: rows
// 0 ... k of chunk c - k), rotated by unrolling.  Everything is straight-line code in the manner of pair_rows_group (U
// columns of loads, one lgkmcnt(0), then the adds): R rows per column in front of the cut, R - 1 behind it; what a side
// has besides its full groups is one group of 1 ... U - 1 columns -- behind the cut it comes last, in front of the cut
// FIRST, at column 0.  In the first R - 1 columns no chunk of q + 64 is complete yet: with the odd group in front, every
// group that holds one of them stands at a compile-time position and leaves the square out there (pair_duo_front; the
// columns keep their order, so every sum is the one of the other order bit for bit).  The column that holds the cut and the last column
// of q classify their lanes -- wave-uniform intervals, so the squares run under lane masks from the scalar unit
// (pair_duo_edge) instead of per-lane selects.  The R - 1 columns behind the last one of q bring the rows that q + 64
// still lacks (pair_duo_tail).  Adds and squares per period are those of two single passes, in the same order in
// every variant; the reads are ~0.63 x (45 281 -> 28 669 wavefront loads per sweep at N = 4096, p = 683 ... 1365).
// (the window address of the lane is recomputed in front of every loop, as pair_lane() is: kept live across the pass it
// is spilled around the groups)
__device__ __forceinline__ pair_ptr pair_at(const f2* __restrict__ xs) { return (pair_ptr)xs + pair_lane(); }

// acc += v * v in the lanes of `lanes` (a wave-uniform bit mask) only: the packed FMA runs under EXEC & lanes, the
// other lanes keep their sum.  The lane sets of a pass are intervals the scalar unit knows (pair_lanes_below); a select
// per lane and operand in front of an unconditional FMA cost 30 vector instructions per classified column.  EXEC is
// back in place at the end of the statement, in front of any LDS or cross-lane instruction.
__device__ __forceinline__ unsigned long pair_lanes_below(int n) { return ~0ul >> (64 - n); }  // lanes 0 ... n - 1, 1 <= n <= 64
__device__ __forceinline__ void f2_sq_acc_lanes(f2& acc, f2 v, unsigned long lanes) {
  unsigned long keep;
  asm volatile(
      "s_and_saveexec_b64 %[keep], %[m]\n\t"
      "v_pk_fma_f32 %[acc], %[v], %[v], %[acc]\n\t"
      "s_mov_b64 exec, %[keep]"
      : [acc] "+v"(acc), [keep] "=&s"(keep)
      : [v] "v"(v), [m] "s"(lanes)
      : "scc");
}
// the column that holds the cut: lanes of `below` are residues in front of it (sums sa, pa), the others lie behind it
// (pb), and those of them in `inq` are residues of q as well (sb)
__device__ __forceinline__ void f2_sq_acc_cut(f2& sa, f2& pa, f2& sb, f2& pb, f2 t, f2 d, unsigned long below, unsigned long inq) {
  unsigned long keep;
  asm volatile(
      "s_and_saveexec_b64 %[keep], %[below]\n\t"
      "v_pk_fma_f32 %[sa], %[t], %[t], %[sa]\n\t"
      "v_pk_fma_f32 %[pa], %[d], %[d], %[pa]\n\t"
      "s_andn2_b64 exec, %[keep], %[below]\n\t"
      "v_pk_fma_f32 %[pb], %[d], %[d], %[pb]\n\t"
      "s_and_b64 exec, exec, %[inq]\n\t"
      "v_pk_fma_f32 %[sb], %[t], %[t], %[sb]\n\t"
      "s_mov_b64 exec, %[keep]"
      : [sa] "+v"(sa), [pa] "+v"(pa), [sb] "+v"(sb), [pb] "+v"(pb), [keep] "=&s"(keep)
      : [t] "v"(t), [d] "v"(d), [below] "s"(below), [inq] "s"(inq)
      : "scc");
}

// U columns, NR rows each.  PRO says what becomes of the sums of q + 64 that complete here -- in the first R - 1
// columns of a pass none is complete.  Every group in front of column R - 1 stands at a position known at compile time
// (pair_duo_front), so the count is static:
//   0       every column is at R - 1 or behind it: all of them are squared;
//   k > 0   the first k columns of the group are in front of R - 1: they simply have no square.
template <int R, int NR, int U, int PRO>
__device__ __forceinline__ void pair_duo_group(pair_ptr ptr, int q, f2 (&pend)[R - 1], f2& sa, f2& pa, f2& sb, f2& pb) {
  static_assert(NR == R || NR == R - 1, "all rows (in front of the cut), or all but the last (behind it)");
  static_assert(PRO >= 0 && PRO <= U, "columns without a square are columns of the group");
  f2 v[NR][U];
#pragma unroll
  for (int r = 0; r < NR; ++r)
#pragma unroll
    for (int u = 0; u < U; ++u) v[r][u] = ptr[r * q + 64 * u];
  __builtin_amdgcn_s_waitcnt(0xC07F);  // lgkmcnt(0)
  __builtin_amdgcn_sched_barrier(0);
#pragma unroll
  for (int u = 0; u < U; ++u) {
    f2 t = v[0][u];
#pragma unroll
    for (int r = 1; r < NR; ++r) t += v[r][u];
    if (NR == R) sa = f2_fma(t, t, sa);
    else sb = f2_fma(t, t, sb);
    if (u >= PRO) {
      f2 d = pend[R - 2];  // the chunk of q + 64 that lies R - 1 columns back
      if (NR == R) d += v[NR - 1][u];
      if (NR == R) pa = f2_fma(d, d, pa);
      else pb = f2_fma(d, d, pb);
    }
#pragma unroll
    for (int k = R - 2; k >= 1; --k) pend[k] = pend[k - 1] + v[k][u];
    pend[0] = v[0][u];
  }
}

// A column whose lanes are classified: the one that holds the cut (NR = R; `below` = its lanes in front of the cut), and
// the last column of q (`inq` = its lanes that are residues of q; the others belong to q + 64 alone).  Both lie at
// column R - 1 or behind it (pair_duo_rows), so the sum of q + 64 that completes here is always squared.
template <int R, int NR>
__device__ __forceinline__ void pair_duo_edge(pair_ptr ptr, int q, unsigned long below, unsigned long inq, f2 (&pend)[R - 1],
                                              f2& sa, f2& pa, f2& sb, f2& pb) {
  static_assert(NR == R || NR == R - 1, "all rows (in front of the cut), or all but the last (behind it)");
  f2 v[NR];
#pragma unroll
  for (int r = 0; r < NR; ++r) v[r] = ptr[r * q];
  __builtin_amdgcn_s_waitcnt(0xC07F);  // lgkmcnt(0)
  __builtin_amdgcn_sched_barrier(0);
  f2 t = v[0];
#pragma unroll
  for (int r = 1; r < NR; ++r) t += v[r];
  f2 d = pend[R - 2];
  if (NR == R) d += v[NR - 1];
  if (NR == R) {
    f2_sq_acc_cut(sa, pa, sb, pb, t, d, below, inq);
  } else {
    f2_sq_acc_lanes(sb, t, inq);
    pb = f2_fma(d, d, pb);
  }
#pragma unroll
  for (int k = R - 2; k >= 1; --k) pend[k] = pend[k - 1] + v[k];
  pend[0] = v[0];
}

// The columns ncb + t, t = T0 ... T1 - 1 of 0 ... R - 2, behind the last column of q (ncb = ceil(q / 64)): q + 64 needs
// the rows t ... R - 2 of them.  All of them lie inside the window: row R - 2 of column ncb + t starts at index
// 64 (ncb + t) + (R - 2) q, which is below N because 64 ncb - q + 64 t <= 63 + 64 (R - 2) < cut = N - (R - 1) q (the
// partner has R rows: cut > 64 (R - 1), see pair_duo_rows), and its lanes end below N + 63.  Every chunk of q + 64 that
// completes here lies behind its cut; the last one, chunk ncb, is cut at q + 64 (after column R - 2).  Six rows take the
// columns in two batches (15 loads would cost the registers).
template <int R, int T0, int T1>
__device__ __forceinline__ void pair_duo_tail(const f2* __restrict__ xs, int q, int ncb, f2 (&pend)[R - 1], f2& pb) {
  const pair_ptr at = pair_at(xs) + 64 * ncb;
  f2 v[R - 1][R - 1];  // [row][t]
#pragma unroll
  for (int t = T0; t < T1; ++t)
#pragma unroll
    for (int r = t; r < R - 1; ++r) v[r][t] = at[r * q + 64 * t];
  __builtin_amdgcn_s_waitcnt(0xC07F);  // lgkmcnt(0)
  __builtin_amdgcn_sched_barrier(0);
#pragma unroll
  for (int t = T0; t < T1; ++t) {
    pb = f2_fma(pend[R - 2], pend[R - 2], pb);  // chunk ncb + t - (R - 1)
#pragma unroll
    for (int k = R - 2; k >= 1; --k) pend[k] = k >= t ? pend[k - 1] + v[k][t] : pend[k - 1];
    if (t == 0) pend[0] = v[0][0];
  }
  if (T1 == R - 1) f2_sq_acc_lanes(pb, pend[R - 2], pair_lanes_below(q - 64 * (ncb - 1)));  // chunk ncb: residues q ... q + 63
}

// The columns in front of the cut, up to the first group boundary at or behind column R - 1.  The pairing rule gives
// whole >= R - 1 (pair_duo_rows), and the first group has F = whole mod UA columns (UA when that is 0), so whole - F is a
// multiple of UA: a full group that starts at S = F + k UA < R - 1 <= whole ends at S + UA <= whole.  The groups peeled
// here therefore always exist, and each knows at compile time how many of its columns lie in front of R - 1.
template <int R, int UA, int S>
__device__ __forceinline__ void pair_duo_peel(pair_ptr at, int q, f2 (&pend)[R - 1], f2& sa, f2& pa, f2& sb, f2& pb) {
  if constexpr (S < R - 1) {
    pair_duo_group<R, R, UA, (R - 1 - S < UA ? R - 1 - S : UA)>(at + 64 * S, q, pend, sa, pa, sb, pb);
    pair_duo_peel<R, UA, S + UA>(at, q, pend, sa, pa, sb, pb);
  }
}
// returns the column the main loop starts at
template <int R, int UA, int F>
__device__ __forceinline__ int pair_duo_front(pair_ptr at, int q, f2 (&pend)[R - 1], f2& sa, f2& pa, f2& sb, f2& pb) {
  static_assert(F >= 1 && F <= UA, "the first group is the remainder, or a full group");
  pair_duo_group<R, R, F, (R - 1 < F ? R - 1 : F)>(at, q, pend, sa, pa, sb, pb);
  pair_duo_peel<R, UA, F>(at, q, pend, sa, pa, sb, pb);
  return F >= R - 1 ? F : F + (R - 1 - F + UA - 1) / UA * UA;
}

template <int R>
__device__ __forceinline__ void pair_duo_rows(const f2* __restrict__ xs, int N, int q, const PGeomF g, f2& base, f2& partner) {
  // loads in flight: 12 / 16 / 10 / 12 in front of the cut (R = 3 ... 6), 8 / 12 / 12 / 10 behind it
  constexpr int UA = R <= 4 ? 4 : 2, UB = R <= 4 ? 4 : R == 5 ? 3 : 2;
  constexpr int B3 = UB < 4 ? 1 : 3, B2 = UB < 3 ? 1 : 2;  // widths of the remainder groups behind the cut
  const int cut = g.nfull, ncb = (q + 63) >> 6, last = ncb - 1;  // the last column of q is cut at q
  f2 pend[R - 1];
#pragma unroll
  for (int k = 0; k < R - 1; ++k) pend[k] = f2_zero();
  f2 sa = f2_zero(), pa = f2_zero(), sb, pb;
  int c;
  {
    // In front of the cut the group of odd size comes FIRST, at column 0, and full groups follow: every group that holds
    // one of the first R - 1 columns then stands at a compile-time position, and the main loop ends exactly at `whole`.
    const int whole = min(cut >> 6, last);
    const pair_ptr at = pair_at(xs);
    const int rem = whole & (UA - 1);
    if (UA > 3 && rem == 3) c = pair_duo_front<R, UA, (UA > 3 ? 3 : 1)>(at, q, pend, sa, pa, sb, pb);
    else if (UA > 2 && rem == 2) c = pair_duo_front<R, UA, (UA > 2 ? 2 : 1)>(at, q, pend, sa, pa, sb, pb);
    else if (rem == 1) c = pair_duo_front<R, UA, 1>(at, q, pend, sa, pa, sb, pb);
    else c = pair_duo_front<R, UA, UA>(at, q, pend, sa, pa, sb, pb);
    // Two groups per trip: the second takes its loads from the row addresses of the first (512 UA bytes further on, an
    // offset in the instruction), which halves the address arithmetic of the loop.  In front of the cut only up to four
    // rows: at five and six the addresses kept across both groups cost the kernel one more spilled register.
    if constexpr (R <= 4) {
      for (; c + 2 * UA <= whole; c += 2 * UA) {
        pair_duo_group<R, R, UA, 0>(at + 64 * c, q, pend, sa, pa, sb, pb);
        pair_duo_group<R, R, UA, 0>(at + 64 * c + 64 * UA, q, pend, sa, pa, sb, pb);
      }
    }
    for (; c + UA <= whole; c += UA) pair_duo_group<R, R, UA, 0>(at + 64 * c, q, pend, sa, pa, sb, pb);
  }
  sb = f2_zero_at_use();  // (not live in front of the cut)
  pb = f2_zero_at_use();
  // From here on every column lies at R - 1 or behind it: the partner has R rows as well, (R - 1) (q + 64) < N, so
  // cut = N - (R - 1) q > 64 (R - 1) -- `whole` >= R - 1, and q has more than R chunk columns.
  const unsigned long inq = pair_lanes_below(q - 64 * last);  // lanes of the last column that are residues of q
  if (c < last && 64 * c < cut) {  // the column that holds the cut
    asm volatile("" ::: "memory");
    pair_duo_edge<R, R>(pair_at(xs) + 64 * c, q, pair_lanes_below(cut - 64 * c), ~0ul, pend, sa, pa, sb, pb);
    c += 1;
  }
  {
    const pair_ptr at = pair_at(xs);
    for (; c + 2 * UB <= last; c += 2 * UB) {  // (two groups per trip, as in front of the cut)
      pair_duo_group<R, R - 1, UB, 0>(at + 64 * c, q, pend, sa, pa, sb, pb);
      pair_duo_group<R, R - 1, UB, 0>(at + 64 * c + 64 * UB, q, pend, sa, pa, sb, pb);
    }
    for (; c + UB <= last; c += UB) pair_duo_group<R, R - 1, UB, 0>(at + 64 * c, q, pend, sa, pa, sb, pb);
    const int rem = last - c;
    if (rem > 0) {  // fewer than UB columns: one group, one drain
      asm volatile("" ::: "memory");
      if (UB > 3 && rem == 3) pair_duo_group<R, R - 1, B3, 0>(at + 64 * c, q, pend, sa, pa, sb, pb);
      else if (UB > 2 && rem == 2) pair_duo_group<R, R - 1, B2, 0>(at + 64 * c, q, pend, sa, pa, sb, pb);
      else pair_duo_group<R, R - 1, 1, 0>(at + 64 * c, q, pend, sa, pa, sb, pb);
    }
  }
  asm volatile("" ::: "memory");
  if (64 * last < cut) pair_duo_edge<R, R>(pair_at(xs) + 64 * last, q, pair_lanes_below(cut - 64 * last), inq, pend, sa, pa, sb, pb);
  else pair_duo_edge<R, R - 1>(pair_at(xs) + 64 * last, q, 0ul, inq, pend, sa, pa, sb, pb);
  const f2 wf = f2_make(g.w_full, g.w_full);
  base = f2_fma(sa, wf, sb * g.w_short);  // (complete: two registers fewer across the tail)
  if (R == 6) {
    pair_duo_tail<R, 0, 2>(xs, q, ncb, pend, pb);
    pair_duo_tail<R, 2, R - 1>(xs, q, ncb, pend, pb);
  } else {
    pair_duo_tail<R, 0, R - 1>(xs, q, ncb, pend, pb);
  }
  partner = f2_fma(pa, wf, pb * g.w_short);
}

// Per-lane partials of both windows for the periods q (`base`) and q + 64 (`partner`); g = geometry of q, and the host
// guarantees that q + 64 has the same row count R, 3 <= R <= 6, and that q > 64 R.
__device__ __forceinline__ void pair_pass_duo(const f2* __restrict__ xs, int N, int q, const PGeomF g, f2& base, f2& partner) {
  base = partner = f2_zero();
  switch (g.rows) {
#define PH_DUO_CASE(R)                                \
  case R:                                             \
    pair_duo_rows<R>(xs, N, q, g, base, partner);     \
    break;
    PH_DUO_CASE(3)
    PH_DUO_CASE(4)
    PH_DUO_CASE(5)
    PH_DUO_CASE(6)
#undef PH_DUO_CASE
    default: break;
  }
}

// ---------------------------------------------------------------- multi-class pass, straight-line segments
// Period p, 2p (and 4p) from the class sums of one fold: the weights of a part are compile-time indexed and chosen on
// the scalar unit, the tail of a part is picked by two compares, and no flag survives a branch.
template <int M, bool MX = false, typename GT>
__device__ __forceinline__ void pair_pass_multi(const f2* __restrict__ xs, int p, GT geom,
                                                f2 (&total)[3]) {
  static_assert(M == 2 || M == 4, "two or four classes");
  const PGeomF g1 = geom[p], g2 = geom[2 * p], g4 = geom[(M == 4 ? 4 : 2) * p];
  const int lane = pair_lane();
  const int cut = g1.nfull;
  const int acols = min(p, (cut + 63) & ~63), rest = p - acols;  // part A: the chunks up to the one that holds the cut
  const pair_ptr a = (pair_ptr)xs + lane;
  // class u of period 2p / 4p at column j is the residue u p + j: the columns below the cut lie on one side of
  // nfull(2p), nfull(4p), the columns behind it on one side as well (weights wa / wb)
  float wa[7], wb[7];
  wa[0] = g1.w_full;
  wb[0] = g1.w_short;
  wa[1] = g2.w_full;  // residue 0 is never short
  wa[3] = g4.w_full;
  if (!MX) {
    wa[2] = scalar_select_lt(p, g2.nfull, g2.w_full, g2.w_short);
#pragma unroll
    for (int u = 0; u < 2; ++u) wb[1 + u] = scalar_select_lt(cut + u * p, g2.nfull, g2.w_full, g2.w_short);
#pragma unroll
    for (int u = 1; u < 4; ++u) wa[3 + u] = M == 4 ? scalar_select_lt(u * p, g4.nfull, g4.w_full, g4.w_short) : 0.0f;
#pragma unroll
    for (int u = 0; u < 4; ++u) wb[3 + u] = M == 4 ? scalar_select_lt(cut + u * p, g4.nfull, g4.w_full, g4.w_short) : 0.0f;
  }
  if (M == 4) {  // the weights are applied per chunk, straight into the totals
    total[0] = total[1] = total[2] = f2_zero();
    pair_multi_segment<M, M, MX, true>(a, p, cut, acols, g1.rows, lane, wa, wb, total, total);
    if (rest > 0) pair_multi_segment<M, M, MX>(a + acols, p, rest, rest, g1.rows - 1, lane, wb, wb, total, total);
    return;
  }
  f2 sa[3] = {f2_zero(), f2_zero(), f2_zero()}, sb[3] = {f2_zero(), f2_zero(), f2_zero()};
  pair_multi_segment<M, M, MX, true>(a, p, cut, acols, g1.rows, lane, wa, wb, sa, sb);
  if (rest > 0) pair_multi_segment<M, M, MX>(a + acols, p, rest, rest, g1.rows - 1, lane, wb, wb, sb, sb);
  if (MX) {
    total[0] = f2_max(sa[0], sb[0]);
    total[1] = f2_max(sa[1], sb[1]);
  } else {
    total[0] = f2_fma(sa[0], f2_make(wa[0], wa[0]), sb[0] * wb[0]);
    total[1] = f2_fma(sa[1], f2_make(wa[1], wa[1]), f2_fma(sa[2], f2_make(wa[2], wa[2]), f2_fma(sb[1], f2_make(wb[1], wb[1]), sb[2] * wb[2])));
  }
  total[2] = f2_zero();
}

// p < 64: row-split path of wave_fold_small / wave_partial_small for pairs.
template <bool MX = false>
__device__ __forceinline__ f2 pair_partial_small(const f2* __restrict__ xs, int N, int p, const PGeomF& g) {
  const int lane = pair_lane();
  const int G = 64 / p;
  const int L = G * p;
  const int full = N / L;
  const bool on = lane < L;
  const f2* ptr = xs + (on ? lane : 0);
  f2 s0 = f2_zero(), s1 = f2_zero();
  int r = 0;
  for (; r + 4 <= full; r += 4) {
    const f2 a = ptr[0], b = ptr[L], c = ptr[2 * L], d = ptr[3 * L];
    s0 += a;
    s1 += b;
    s0 += c;
    s1 += d;
    ptr += 4 * L;
  }
  for (; r < full; ++r) {
    s0 += ptr[0];
    ptr += L;
  }
  const bool tail = on && (full * L + lane < N);
  const f2 tv = xs[tail ? full * L + lane : 0];
  f2 tot = s0 + s1 + (tail ? tv : f2_zero());
  tot = on ? tot : f2_zero();
  int s = 1;
  while (s < G) s <<= 1;
  for (s >>= 1; s >= 1; s >>= 1) {
    const int src = lane + s * p;
    const float ox = __shfl(tot.x, src & (kWave - 1), kWave);
    const float oy = __shfl(tot.y, src & (kWave - 1), kWave);
    tot += (src < L) ? f2_make(ox, oy) : f2_zero();
  }
  const float w = MX ? 1.0f : (lane < g.nfull) ? g.w_full : g.w_short;
  return (lane < p) ? tot * tot * w : f2_zero();
}

// Wavefront totals of the per-lane pairs, PACKED: the consumers of a screen store the totals or test them in one lane,
// nobody needs them in all 64.  v_permlane32_swap puts the two windows of a period side by side in one register (lanes
// 0-31 window a, 32-63 window b: half the data per level from there on), v_permlane16_swap does the same with two
// periods (rows of 16 lanes), and the rest of the tree runs inside the rows with the DPP operand folded into the add
// (ror 8, half mirror, xor 2, xor 1 -- nothing goes through the LDS pipe).  9 instructions for one period, 10 for two
// (the all-lanes versions of round 3: 20 and 22).
template <int CTRL>
__device__ __forceinline__ float dpp_f32(float v) {
  return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xF, 0xF, false));
}

template <bool MX>
__device__ __forceinline__ float pair_row_reduce(float z) {
  auto op = [](float u, float v) { return MX ? fmaxf(u, v) : u + v; };
  z = op(z, dpp_f32<kDppRor8>(z));
  z = op(z, dpp_f32<kDppHalfMirror>(z));
  z = op(z, dpp_f32<kDppXor2>(z));
  z = op(z, dpp_f32<kDppXor1>(z));
  return z;
}

// one period: afterwards lanes 0-31 hold the wavefront total (MX: maximum) of v.x, lanes 32-63 that of v.y
template <bool MX>
__device__ __forceinline__ float pair_reduce1(f2 v) {
  auto op = [](float u, float w) { return MX ? fmaxf(u, w) : u + w; };
  const auto r0 = __builtin_amdgcn_permlane32_swap((unsigned)__float_as_int(v.x), (unsigned)__float_as_int(v.y), false, false);
  const float z = op(__int_as_float((int)r0[0]), __int_as_float((int)r0[1]));  // rows: x, x, y, y (two partials each)
  const unsigned zi = (unsigned)__float_as_int(z);
  const auto r1 = __builtin_amdgcn_permlane16_swap(zi, zi, false, false);
  return pair_row_reduce<MX>(op(__int_as_float((int)r1[0]), __int_as_float((int)r1[1])));
}

// two periods: afterwards the rows of 16 lanes hold the totals of a.x, a.y, b.x, b.y (lanes 0-15, 16-31, 32-47, 48-63)
template <bool MX>
__device__ __forceinline__ float pair_reduce2(f2 a, f2 b) {
  auto op = [](float u, float w) { return MX ? fmaxf(u, w) : u + w; };
  const auto r0 = __builtin_amdgcn_permlane32_swap((unsigned)__float_as_int(a.x), (unsigned)__float_as_int(b.x), false, false);
  const auto r1 = __builtin_amdgcn_permlane32_swap((unsigned)__float_as_int(a.y), (unsigned)__float_as_int(b.y), false, false);
  const float x = op(__int_as_float((int)r0[0]), __int_as_float((int)r0[1]));  // rows: a.x, a.x, b.x, b.x
  const float y = op(__int_as_float((int)r1[0]), __int_as_float((int)r1[1]));  // rows: a.y, a.y, b.y, b.y
  const auto r2 = __builtin_amdgcn_permlane16_swap((unsigned)__float_as_int(x), (unsigned)__float_as_int(y), false, false);
  return pair_row_reduce<MX>(op(__int_as_float((int)r2[0]), __int_as_float((int)r2[1])));  // rows: a.x, a.y, b.x, b.y
}

// where the packed totals go in an array of pairs `vals` (entry q - q0 = {window a, window b} of period q)
__device__ __forceinline__ void pair_store1(f2* vals, float z, int q, int q0) {
  const int l = pair_lane();
  if ((l & 31) == 0) reinterpret_cast<float*>(vals)[2 * (q - q0) + (l >> 5)] = z;
}
__device__ __forceinline__ void pair_store2(f2* vals, float z, int qa, int qb, int q0) {
  const int l = pair_lane();
  if ((l & 15) == 0) reinterpret_cast<float*>(vals)[2 * ((l < 32 ? qa : qb) - q0) + ((l >> 4) & 1)] = z;
}

// ---------------------------------------------------------------- chains of periods up to 64
// The row-split pass at L <= 64 (lane l < L adds x[l + n L]: the fold to period L, contiguous reads) is the fold of
// every divisor of L as well: S_{L/2}[l] = S_L[l] + S_L[l + L/2], and so on down the powers of two.  One pass of
// N / L loads yields L, L/2, ..., L / 2^(nlev-1) -- the host plans 32 chains for the 63 periods up to 64 (PassPlan
// m = 8 + nlev).  Two levels share one wavefront reduction (pair_reduce2).  Any summation order is covered by
// pair_radius.
__device__ __forceinline__ f2 pair_shift_down(f2 v, int lane, int by) {  // v of lane + by (lanes that matter: < 64 - by)
  const int addr = ((lane + by) & (kWave - 1)) << 2;
  return f2_make(__int_as_float(__builtin_amdgcn_ds_bpermute(addr, __float_as_int(v.x))),
                 __int_as_float(__builtin_amdgcn_ds_bpermute(addr, __float_as_int(v.y))));
}

template <bool MX>
__device__ __forceinline__ f2 pair_chain_term(f2 tot, int lane, int q, const PGeomF& g) {
  const float w = MX ? 1.0f : (lane < g.nfull) ? g.w_full : g.w_short;
  return (lane < q) ? tot * tot * w : f2_zero();
}

template <bool MX, typename GT, typename F, typename F2>
__device__ __forceinline__ void pair_chain_small(const f2* __restrict__ xs, int N, int L, int nlev,
                                                 GT geom, F&& consume, F2&& consume2) {
  const int lane = pair_lane();
  PGeomF g = geom[L];
  const int full = g.nfull == L ? g.rows : g.rows - 1;  // floor(N / L)
  const bool on = lane < L;
  const f2* ptr = xs + (on ? lane : 0);
  f2 s0 = f2_zero(), s1 = f2_zero();
  int r = 0;
  for (; r + 4 <= full; r += 4) {
    const f2 a = ptr[0], b = ptr[L], c = ptr[2 * L], d = ptr[3 * L];
    s0 += a;
    s1 += b;
    s0 += c;
    s1 += d;
    ptr += 4 * L;
  }
  for (; r < full; ++r) {
    s0 += ptr[0];
    ptr += L;
  }
  const bool tail = on && (full * L + lane < N);
  const f2 tv = xs[tail ? full * L + lane : 0];
  f2 tot = s0 + s1 + (tail ? tv : f2_zero());
  tot = on ? tot : f2_zero();
  int q = L;
  for (int lev = 0; lev < nlev; lev += 2) {
    const f2 va = pair_chain_term<MX>(tot, lane, q, g);
    if (lev + 1 < nlev) {
      const int q2 = q >> 1;
      const PGeomF g2 = geom[q2];
      tot += pair_shift_down(tot, lane, q2);
      const f2 vb = pair_chain_term<MX>(tot, lane, q2, g2);
      consume2(pair_reduce2<MX>(va, vb), q, q2);
      if (lev + 2 < nlev) {
        q = q2 >> 1;
        g = geom[q];
        tot += pair_shift_down(tot, lane, q);
      }
    } else {
      consume(pair_reduce1<MX>(va), q);
    }
  }
}

// Screen sweep driven by the pass plan.  consume(z, q) gets the packed totals of one period (pair_reduce1: lanes 0-31
// window a, 32-63 window b), consume2(z, q_a, q_b) those of two periods of a multi-class pass or two levels of a chain
// (pair_reduce2: rows of 16 lanes = q_a window a, q_a window b, q_b window a, q_b window b); pair_store1 / pair_store2
// put them into an array.  Every period is reduced on its own: nothing is live across the folds (the online 8-period
// butterfly of the fp64 sweeps kept pending partials that were spilled in every pass: 3.03 -> 2.82 ms in round 3).
// DUO: the plan may hold shared-load entries (m = 3, pair_pass_duo); the other kernels never get such a plan.
template <bool MX = false, bool DUO = false, typename GT, typename PT, typename F, typename F2>
__device__ __forceinline__ void pair_sweep_plan(const f2* __restrict__ xs, int N, GT geom,
                                                PT plan, int i_first, int i_end, int stride,
                                                F&& consume, F2&& consume2, int* __restrict__ queue = nullptr) {
  auto red = [](f2 v) { return pair_reduce1<MX>(v); };
  // `queue` (an LDS counter the caller has set to `stride`, the number of wavefronts): the passes are taken in plan
  // order by whichever wavefront is free -- the passes differ in cost and the sweep ends at a barrier.
  for (int i = i_first; i < i_end;) {
    int ticket = 0;
    if (queue && pair_lane() == 0) ticket = lds_ticket(queue);  // the next pass: claimed now, looked at after this one
    const int p = plan[i].p, m = plan[i].m;
    if (m >= 8) {
      pair_chain_small<MX>(xs, N, p, m - 8, geom, consume, consume2);
    } else if (m == 0) {
      consume(red(pair_partial_small<MX>(xs, N, p, geom[p])), p);
    } else if (m == 1) {
      consume(red(pair_pass_single<MX>(xs, p, geom[p])), p);
    } else if (DUO && m == 3) {  // p and p + 64 from one set of reads (k_mbest_step1_pair only)
      f2 va, vb;
      pair_pass_duo(xs, N, p, geom[p], va, vb);
      consume2(pair_reduce2<MX>(va, vb), p, p + 64);
    } else if (m == 2) {
      f2 part[3];
      pair_pass_multi<2, MX>(xs, p, geom, part);
      consume2(pair_reduce2<MX>(part[0], part[1]), p, 2 * p);
    } else {
      f2 part[3];
      pair_pass_multi<4, MX>(xs, p, geom, part);
      consume2(pair_reduce2<MX>(part[0], part[1]), p, 2 * p);
      consume(red(part[2]), 4 * p);
    }
    i = queue ? lds_ticket_value(ticket) : i + stride;
  }
}

// Rigorous radius of the screen, in units of the (scaled) sum of squares ssq of the fp64 residual r:
//   |screen(q) - sum_j S_q[j]^2 / cnt_q[j]| <= pair_radius(q) * ssq.
// With u = 2^-24, rf = fl32(r s) (s a power of two, |rf - r s| <= u |r s|), n_j <= R terms per residue and
// A_j = sum |r s| over the coset: any summation order gives |S^_j - S_j| <= (u + gamma_{R-1}) A_j <= R u' A_j, so
// |S^_j^2 - S_j^2| / cnt_j <= (2 |S_j| + R u' A_j) R u' A_j / cnt_j <= 2 R u' (1 + R u') Q_j by Cauchy-Schwarz
// (A_j^2 <= cnt_j Q_j, Q_j = sum (r s)^2 over the coset, sum_j Q_j = ssq).  Squaring, weighting with fl32(1/cnt)
// and the class sums add <= 6 u per term; the positive sum over q/64 chunks, two segments and the butterfly adds
// gamma_{q/64 + 10}.  First order: (2 R + q/64 + 16) u; the factor 1.5 and the +32 cover the second-order terms
// (R u <= 2^-13 for R <= 2048), the error of the fp64 value itself (<= (2R + q/64 + 16) 2^-53) and the error of ssq.
// Underflow: the windows are scaled to RMS ~ 1, so denormal roundings (<= 2^-149 each) are far below the radius.
__host__ __device__ __forceinline__ double pair_radius(int rows, int q) {
  return 1.5 * (2.0 * (double)rows + (double)(q >> 6) + 32.0) * 5.9604644775390625e-08;
}

// Cover rule of k_mbest_step1_pair (plain m_best): V_d, the d-periodic vectors of length N, lie in V_m when d | m, so
// the exact values obey E_d <= E_m, and every d <= floor(p_hi / 2) has a multiple in (floor(p_hi / 2), p_hi].  Only
// those "top" periods are screened; a divisor is evaluated (in fp64) only when a multiple m may still hold the maximum:
//   E^_d <= E_d + e_d ssq <= E_m + e_d ssq <= screen(m) + (pair_radius(m) + e_d) ssq,
// E^_d being the fp64 value the exact phase computes for d and e_d <= (2 R_d + d/64 + 16) 2^-53 its rounding error (the
// fp64 analogue of the first-order term above: u = 2^-53, no input rounding).  R_d <= N and d <= N give
// e_d <= (2 N + N/64 + 16) 2^-53 < (2 N + 32) 2^-52, the factor 2 covering the second-order terms.  The slack is
// ABSOLUTE, in units of ssq: after a period has been removed E_d and E_m are both rounding noise of order 1e-33 ssq in
// either order, which no bound relative to E_m would cover.  Never less than 2^-40.
__host__ __device__ __forceinline__ double pair_cover_slack(int N) {
  return fmax(9.094947017729282e-13, (2.0 * (double)N + 32.0) * 2.220446049250313e-16);
}

// Fold-once path of k_mbest_step1_pair: the residual is folded ONCE at the surviving top period m (column sums S_m in
// row order), and a listed divisor d | m is valued from those sums, T_d = sum_j (sum_{k = j (mod d)} S_m[k])^2 / cnt_d[j],
// instead of by a fold of its own over the window (v_d, the value of the staged thinning in k_mbest_step1_pair).  Both
// are fp64 evaluations of the same E_d, and they differ only in the ORDER in which a residue's R_d samples are added: v_d
// adds them row by row, T_d adds the rows of each of the m / d columns of m first, then those column sums, for d < 64
// finished by shuffles.  The bound e_d behind pair_cover_slack holds for any order: its first-order term is
// gamma_{n-1} A_j with n <= R_d the number of terms of the residue, whatever the tree (the sum over the residues likewise:
// d / 64 + 10 terms at most in either form).  So |T_d - E_d| and |v_d - E_d| are at most e_d ssq <= slack ssq, and
// |T_d - v_d| <= 2 slack ssq.  The same holds for m itself:
// the cooperative value E^_m (whole workgroup) and the thinning's wavefront value v_m differ by at most 2 slack ssq.
// The path is taken only when every listed divisor has
//   T_d < E^_m - |E^_m| 1e-9 - band ssq,   band = 5 slack.
// Then v_d <= T_d + 2 slack ssq < v_m + 4 slack ssq - (|v_m| - 2 slack ssq) 1e-9 - 5 slack ssq < v_m - |v_m| 1e-9 (the
// spare (1 - 2e-9) slack ssq >= 9e-13 ssq is far above the rounding of these few operations, ~1e-16 E): the staged
// thinning keeps m alone, and the staged phases then decide on the cooperative value of m alone -- the value this path has.
// Units as for pair_cover_slack: the sum of squares of the (scaled) residual, MP_UNIT of the kernel.
// (the kernel gets the number from the host)
__host__ __device__ __forceinline__ double pair_thin_band(int N) { return 5.0 * pair_cover_slack(N); }

// Row-order sum of column j of period m over `n` >= 1 rows of a window in GLOBAL memory (the first row is read
// unconditionally: the pair kernel runs only with max_length < N, pair_eligible, so every column of a candidate period
// has at least one row and a full one at least two): ((x[j] + x[m + j]) + x[2 m + j]) + ...,
// the additions of column_sum in the same order, so the same bits.  Groups of four loads behind the first (a top period
// has 3 ... 6 rows) on 32-bit offsets from the wave-uniform base: the kernel sits at its register cap.
__device__ __forceinline__ double pair_column_sum_global(const double* __restrict__ src, int j, int m, int n) {
  unsigned at = (unsigned)j;
  double s = src[at];
  at += (unsigned)m;
  // (a row past the end re-reads the group's first sample and is not added: no tail loop of dependent round trips, and
  // no "+ 0.0" that would turn a sum of -0.0 into +0.0)
  for (int r = 1; r < n; r += 4) {
    const bool k1 = r + 1 < n, k2 = r + 2 < n, k3 = r + 3 < n;
    const double a = src[at], b = src[k1 ? at + (unsigned)m : at], c = src[k2 ? at + 2u * (unsigned)m : at],
                 d = src[k3 ? at + 3u * (unsigned)m : at];
    s += a;
    s = k1 ? s + b : s;
    s = k2 ? s + c : s;
    s = k3 ? s + d : s;
    at += 4u * (unsigned)m;
  }
  return s;
}

// T_d of the fold-once path for one wavefront: S = the column sums of period m in LDS, d | m, g = geometry of d in the
// window (the counts cnt_d[j]).  d >= 64: lane j, j + 64, ... adds its m / d sums.  d < 64: G = 64 / d lanes share a
// residue (lane l adds S[l], S[l + G d], ...), and the G partial sums are added by shuffles.  Per-lane partials; the
// caller sums them over the wavefront.
__device__ __forceinline__ double pair_thin_part(const double* __restrict__ S, int m, int d, const PGeom& g, int lane) {
  double part = 0.0;
  if (d >= kWave) {
    // four residues per trip, their reads in flight together (a residue has only m / d sums, a chain of that many LDS
    // round trips each); a residue past the end re-reads the trip's first one and is left out
    const int n = m / d;
    for (int j0 = lane; j0 < d; j0 += 4 * kWave) {
      double s[4];
      const double* at = S + j0;
#pragma unroll
      for (int u = 0; u < 4; ++u) s[u] = at[j0 + u * kWave < d ? u * kWave : 0];
      for (int r = 1; r < n; ++r) {
        at += d;
#pragma unroll
        for (int u = 0; u < 4; ++u) s[u] += at[j0 + u * kWave < d ? u * kWave : 0];
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int j = j0 + u * kWave;
        if (j < d) part = fma(s[u] * s[u], j < g.nfull ? g.w_full : g.w_short, part);
      }
    }
  } else {
    const int G = kWave / d, L = G * d;
    const int q = m / L, rem = m - q * L;
    double tot = lane < L ? column_sum(S, lane, L, q + (lane < rem ? 1 : 0)) : 0.0;
    const double own = tot;
    for (int k = 1; k < G; ++k) {
      const double o = __shfl(own, (lane + k * d) & (kWave - 1), kWave);  // (lanes below d read lanes below L)
      tot += o;
    }
    part = lane < d ? tot * tot * (lane < g.nfull ? g.w_full : g.w_short) : 0.0;
  }
  return part;
}

// ---------------------------------------------------------------- shared by the window-pair kernels
// (k_mbest_step1_pair, k_best_correlation_pair, k_small_to_large_pair)
#ifndef PH_PAIR_QUEUE
#define PH_PAIR_QUEUE 1
#endif
constexpr int kPairListCap = 96;
constexpr int kPairSmallP = 256;  // winners up to this period: means through LDS, subtraction by all threads
constexpr int kPairSplitW = 512;  // threads that share the rows of a short winner's residues (split_row_means)

__device__ __forceinline__ bool pair_usable(double rsq) { return rsq > 0.0 && rsq < 1.79e308; }

// power of two that brings the RMS of a window into [0.7, 1.5)
__device__ __forceinline__ double pair_pick_scale(double rsq, int N) {
  if (!pair_usable(rsq)) return 1.0;
  int e;
  (void)frexp(rsq / (double)N, &e);
  return ldexp(1.0, -(e >> 1));
}

// The scale of a float image only has to keep its RMS near 1: it is renewed (pair_pick_scale, then pair_rescale) when
// the residual, sum of squares rsq at scale sc, has shrunk to an RMS below 2^-20.
constexpr double kPairStaleMeanSq = 9.0e-13;  // (2^-20)^2, rounded down
__device__ __forceinline__ bool pair_image_stale(double rsq, double sc, int N) {
  return pair_usable(rsq) && rsq * sc * sc < kPairStaleMeanSq * (double)N;
}

// float image of window w of a pair times a power of two: the rescaled image is the image at the new scale
// (tid: for a kernel that recomputes its thread index to keep it out of long-lived registers)
template <int NW = 0>
__device__ __forceinline__ void pair_rescale(float* __restrict__ pwf, int w, int N, float up, int tid = threadIdx.x) {
  for (int n = tid; n < N; n += block_threads<NW>()) pwf[2 * n + w] *= up;
}

// upper bound of ceil(N / q) without an integer division (the radius only has to be an upper bound)
__device__ __forceinline__ int pair_rows_upper(float fn, int q) {
  return (int)(fn * __builtin_amdgcn_rcpf((float)q) * 1.000001f) + 1;
}

}  // namespace ph

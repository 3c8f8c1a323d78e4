// The body of k_follow and of k_follow_residual (ph_follow.h): the statements of a kernel, included into both, with no
// include guard.  RES == false is k_follow as ph_follow.h states it (f0 == 0, `out` unused).  RES == true is
// k_follow_residual: the same cut, means and subtractions on the frames f0 .. f0 + W of the recording, whose final
// residual r_C goes to out[f, 0 .. N) -- no seg, powers or done, so no sums of squares and no block reductions (a plain
// barrier stands where each reduction's barriers stood), and no ccap to end the walk.
// The including kernel supplies, as parameters or as constants: RES, s, L, N, hop, f0, W, win, periods, counts, pcap,
// ccap, flags, gws, seg, powers, done, out, and the types Tin, Tf and the placement LW.
// Text and not a __forceinline__ function: behind a function the compiler keeps the hidden-argument select of
// blockDim.x that it folds away in a kernel's own statements (k_follow then took 2 .. 5 more VGPRs and 2 % longer at
// frames of 4096); included, k_follow compiles to the instructions it had before there was a second kernel.
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const FollowLds Ld = follow_carve(Carve(smem), N, LW);
  double* r = LW ? Ld.r : gws + (size_t)blockIdx.x * follow_work_doubles(N);
  double* m = LW ? Ld.m : r + win_stride((size_t)N);
  double* red = Ld.red;
  const int tid = threadIdx.x, nt = blockDim.x;
  const bool trunc = flags & kTrunc;

  for (int64_t f = blockIdx.x; f < W; f += gridDim.x) {
    // ---- the frame, as k_frames rounds it, and its sum of squares
    const int64_t at = (f0 + f) * hop;
    double acc = 0.0;
    for (int i = tid; i < N; i += nt) {
      double v = 0.0;
      if (at + i < L) {
        const double t = win ? (double)s[at + i] * win[i] : (double)s[at + i];
        v = (double)(Tf)t;
      }
      r[i] = v;
      if constexpr (!RES) acc += v * v;
    }
    // (the barriers of block_sum also make r whole for every thread; the ones of the last frame's final block_sum stand
    // between that frame's reads of r and these writes.  RES: one barrier makes r whole; the last frame's row of `out`
    // was read by the threads that write the same elements here)
    double pn0 = 0.0, pn_prev = 0.0;
    if constexpr (RES) {
      __syncthreads();
    } else {
      pn0 = periodic_norm_from_sq(block_sum(acc, red), N, 0);
      pn_prev = pn0;
    }

    const int cf = RES && pcap == 0 ? 0 : counts[f] < 0 ? 0 : counts[f] > pcap ? pcap : counts[f];
    const int* prow = periods + f * (int64_t)pcap;
    double* srow = RES ? nullptr : seg + f * (int64_t)ccap;
    double* wrow = RES ? nullptr : powers + f * (int64_t)pcap;
    int64_t off = 0;
    int a = 0;
    for (; a < cf; ++a) {
      const int p = prow[a];  // (the same value in every thread: the stop is uniform)
      if (p < 1 || p > N || (!RES && off + p > ccap)) break;
      // ---- one period of means, in row order: kept for the subtraction and written out as the block's segment
      if (p == 1) {  // the mean: numpy's own order (above); trunc or not, the sum over all N samples by N
        if (tid == 0) {
          const double mj = numpy_contiguous_sum(r, N, red) / (double)N;
          m[0] = mj;
          if constexpr (!RES) srow[off] = mj;
        }
      } else {
        const Fold fo(N, p);
        for (int j = tid; j < p; j += nt) {
          const double mj = follow_mean(r, fo, j, trunc);
          m[j] = mj;
          if constexpr (!RES) srow[off + j] = mj;
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
        if constexpr (!RES) acc += v * v;
        j += step;
        if (j >= p) j -= p;
      }
      // (block_sum's barriers: r is whole before the next block's column sums, m is read before it is rewritten)
      if constexpr (RES) {
        __syncthreads();
      } else {
        const double pn = periodic_norm_from_sq(block_sum(acc, red), N, 0);
        if (tid == 0) wrow[a] = pn0 == 0.0 ? 0.0 : (pn_prev - pn) / pn0;
        pn_prev = pn;
      }
      off += p;
    }
    if constexpr (RES) {
      // ---- the residual after the last block: every sample of the row, each by the thread that wrote it last
      double* orow = out + f * (int64_t)N;
      for (int i = tid; i < N; i += nt) orow[i] = r[i];
    } else {
      if (tid == 0) done[f] = a;
      for (int k = a + tid; k < pcap; k += nt) wrow[k] = 0.0;
    }
  }

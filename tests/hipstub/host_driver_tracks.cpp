// Drives ph_overlap_add_tracks through the HOST half of the library (hip_stub.cpp stands in for the runtime; kernels do
// not run, outputs are not looked at).  Built with -fsanitize=address,undefined by tests/test_host_sanitizers.py:
// every refusal, K = 64 against K = 65, the host-pointer staging of y, masks, counts and both windows with exact-size
// vectors, NULL optional pointers, and the size arithmetic with T * L and W * K * N beyond 2^31 (sizes only: those calls
// pass PH_FLAG_DEVICE, so nothing of that size is allocated or touched) must touch no byte out of bounds and overflow no
// integer; every accepted call is one launch of kFramesBlock threads without LDS, named k_overlap_add_tracks.
#include "driver_common.h"

int main() {
  ph_ctx* c = nullptr;
  EXPECT(ph_create(0, &c), PH_OK);
  EXPECT(ph_profile_enable(c, 1), PH_OK);
  stub_reset_launches();

  // ---- host-pointer staging: {L, N, hop, W, K, T}; exact-size vectors, so ASan sees any byte read or written past them
  const int shapes[][6] = {{1000, 64, 16, 60, 3, 2}, {997, 63, 3, 312, 1, 1}, {50, 64, 7, 1, 2, 5}, {8, 8, 1, 1, 1, 1},
                           {1000, 64, 80, 13, 64, 3}, {7, 1, 1, 7, 1, 9}, {333, 65, 64, 6, 5, 4}};
  for (const auto& sh : shapes) {
    const int L = sh[0], N = sh[1], hop = sh[2], W = sh[3], K = sh[4], T = sh[5];
    std::vector<double> win(N, 0.5), out((size_t)T * L);
    std::vector<int32_t> cnt(W, K);
    std::vector<uint64_t> masks((size_t)T * W, ~0ull);
    for (int dt : {PH_F64, PH_F32}) {
      std::vector<char> y((size_t)W * K * N * (dt == PH_F64 ? 8 : 4));
      // NULL optional pointers
      EXPECT(ph_overlap_add_tracks(c, y.data(), dt, W, K, N, hop, L, nullptr, masks.data(), T, nullptr, nullptr, 0, out.data()),
             PH_OK);
      one_launch("k_overlap_add_tracks", __LINE__);
      EXPECT(ph_overlap_add_tracks(c, y.data(), dt, W, K, N, hop, L, cnt.data(), masks.data(), T, win.data(), win.data(),
                                   PH_FLAG_OLA_NORM, out.data()), PH_OK);
      one_launch("k_overlap_add_tracks", __LINE__);
      EXPECT(ph_overlap_add_tracks(c, y.data(), dt, W, K, N, hop, L, cnt.data(), masks.data(), T, nullptr, win.data(),
                                   PH_FLAG_DEVICE | PH_FLAG_OLA_NORM, out.data()), PH_OK);
      one_launch("k_overlap_add_tracks", __LINE__);
    }
  }

  // ---- sizes beyond 2^31, device form: the pointers are never dereferenced on the host
  {
    double tiny[2] = {0, 0};
    const uint64_t* tm = reinterpret_cast<const uint64_t*>(tiny);
    const int64_t W = (int64_t)1 << 21;  // W * K * N = 5 * 2^33
    const int N = 4096, hop = 512, K = 5;
    const int64_t L = (W - 1) * hop + N;  // > 2^30: T * L > 2^31 from T = 3 on
    EXPECT(ph_overlap_add_tracks(c, tiny, PH_F64, W, K, N, hop, L, nullptr, tm, 9, nullptr, nullptr, PH_FLAG_DEVICE, tiny), PH_OK);
    one_launch("k_overlap_add_tracks", __LINE__);
    EXPECT(ph_overlap_add_tracks(c, tiny, PH_F32, W, 64, N, hop, L, nullptr, tm, 3, nullptr, nullptr,
                                 PH_FLAG_DEVICE | PH_FLAG_OLA_NORM, tiny), PH_OK);
    one_launch("k_overlap_add_tracks", __LINE__);
    // T * W beyond 2^31 with a small L
    EXPECT(ph_overlap_add_tracks(c, tiny, PH_F64, 70000, 1, 8, 1, 70007, nullptr, tm, 40000, nullptr, nullptr, PH_FLAG_DEVICE,
                                 tiny), PH_OK);
    one_launch("k_overlap_add_tracks", __LINE__);
    // f * hop beyond 2^31 as well: hop of 2^20 over 2^12 frames
    const int64_t W2 = 4096, L2 = (W2 - 1) * ((int64_t)1 << 20) + 1;
    EXPECT(ph_overlap_add_tracks(c, tiny, PH_F32, W2, 1, 8, 1 << 20, L2, nullptr, tm, 2, nullptr, nullptr, PH_FLAG_DEVICE, tiny),
           PH_OK);
    one_launch("k_overlap_add_tracks", __LINE__);
    // byte counts that do not fit 64 bits are refused, not wrapped: W * K * N, T * L, T * W
    EXPECT(ph_overlap_add_tracks(c, tiny, PH_F64, INT64_MAX / 2, 64, INT32_MAX, 1, INT64_MAX, nullptr, tm, 1, nullptr, nullptr,
                                 PH_FLAG_DEVICE, tiny), PH_E_ARG);
    EXPECT(ph_overlap_add_tracks(c, tiny, PH_F64, 4, 2, 16, 8, INT64_MAX / 16, nullptr, tm, 3, nullptr, nullptr, PH_FLAG_DEVICE,
                                 tiny), PH_E_ARG);
    said("T * L", __LINE__);
    EXPECT(ph_overlap_add_tracks(c, tiny, PH_F64, (int64_t)1 << 40, 1, 1, 1, (int64_t)1 << 40, nullptr, tm, (int64_t)1 << 21,
                                 nullptr, nullptr, PH_FLAG_DEVICE, tiny), PH_E_ARG);
    EXPECT(ph_overlap_add_tracks(c, tiny, PH_F64, 4, 2, 16, 8, 100, nullptr, tm, INT64_MAX, nullptr, nullptr, PH_FLAG_DEVICE,
                                 tiny), PH_E_ARG);
    // the largest counts that pass
    EXPECT(ph_overlap_add_tracks(c, tiny, PH_F64, 4, 2, 16, 8, INT64_MAX / 64, nullptr, tm, 8, nullptr, nullptr, PH_FLAG_DEVICE,
                                 tiny), PH_OK);
    one_launch("k_overlap_add_tracks", __LINE__);
    no_launch(__LINE__);
  }

  // ---- refused, not read
  {
    std::vector<double> y(4 * 2 * 16), out(3 * 100);
    std::vector<uint64_t> masks(3 * 4, 1);
    for (unsigned dev : {0u, (unsigned)PH_FLAG_DEVICE}) {
#define OT(ctx, yy, dt, W, K, N, hop, L, mm, T, o) \
  ph_overlap_add_tracks(ctx, yy, dt, W, K, N, hop, L, nullptr, mm, T, nullptr, nullptr, dev, o)
      EXPECT(OT(nullptr, y.data(), PH_F64, 4, 2, 16, 8, 100, masks.data(), 3, out.data()), PH_E_ARG);
      said("ctx", __LINE__);
      EXPECT(OT(c, nullptr, PH_F64, 4, 2, 16, 8, 100, masks.data(), 3, out.data()), PH_E_ARG);
      EXPECT(OT(c, y.data(), PH_F64, 4, 2, 16, 8, 100, nullptr, 3, out.data()), PH_E_ARG);
      said("masks", __LINE__);
      EXPECT(OT(c, y.data(), PH_F64, 4, 2, 16, 8, 100, masks.data(), 3, nullptr), PH_E_ARG);
      EXPECT(OT(c, y.data(), 7, 4, 2, 16, 8, 100, masks.data(), 3, out.data()), PH_E_ARG);
      said("dtype", __LINE__);
      EXPECT(OT(c, y.data(), -1, 4, 2, 16, 8, 100, masks.data(), 3, out.data()), PH_E_ARG);
      EXPECT(OT(c, y.data(), PH_F64, 0, 2, 16, 8, 100, masks.data(), 3, out.data()), PH_E_ARG);
      EXPECT(OT(c, y.data(), PH_F64, 4, 0, 16, 8, 100, masks.data(), 3, out.data()), PH_E_ARG);
      EXPECT(OT(c, y.data(), PH_F64, 4, 2, 0, 8, 100, masks.data(), 3, out.data()), PH_E_ARG);
      EXPECT(OT(c, y.data(), PH_F64, 4, 2, 16, 0, 100, masks.data(), 3, out.data()), PH_E_ARG);
      EXPECT(OT(c, y.data(), PH_F64, 4, 2, 16, -3, 100, masks.data(), 3, out.data()), PH_E_ARG);
      EXPECT(OT(c, y.data(), PH_F64, 4, 2, 16, 8, 0, masks.data(), 3, out.data()), PH_E_ARG);
      EXPECT(OT(c, y.data(), PH_F64, 4, 2, 16, 8, 24, masks.data(), 3, out.data()), PH_E_ARG);  // (W - 1) hop == L
      said("behind", __LINE__);
      EXPECT(OT(c, y.data(), PH_F64, 4, 2, 16, 8, 100, masks.data(), 0, out.data()), PH_E_ARG);
      said("T=0", __LINE__);
      EXPECT(OT(c, y.data(), PH_F64, 4, 2, 16, 8, 100, masks.data(), -1, out.data()), PH_E_ARG);
      EXPECT(OT(c, y.data(), PH_F64, 4, 65, 16, 8, 100, masks.data(), 3, out.data()), PH_E_ARG);  // one row too many
      said("K=65", __LINE__);
      EXPECT(OT(c, y.data(), PH_F64, 4, INT32_MAX, 16, 8, 100, masks.data(), 3, out.data()), PH_E_ARG);
#undef OT
      no_launch(__LINE__);
    }
    // K = 64 is the last admissible row count, and the last admissible length has frame W - 1 start on the last sample
    std::vector<double> y64(4 * 64 * 16);
    EXPECT(ph_overlap_add_tracks(c, y64.data(), PH_F64, 4, 64, 16, 8, 100, nullptr, masks.data(), 3, nullptr, nullptr, 0,
                                 out.data()), PH_OK);
    one_launch("k_overlap_add_tracks", __LINE__);
    EXPECT(ph_overlap_add_tracks(c, y.data(), PH_F64, 4, 2, 16, 8, 25, nullptr, masks.data(), 3, nullptr, nullptr, 0, out.data()),
           PH_OK);
    one_launch("k_overlap_add_tracks", __LINE__);
  }

  // ---- the profile name of every launch (the profile keeps the first 256)
  float ms[300];
  int cntp = 0;
  EXPECT(ph_profile_read(c, ms, 300, &cntp), PH_OK);
  check_profile(c, cntp);
  EXPECT(ph_sync(c), PH_OK);
  EXPECT(ph_destroy(c), PH_OK);
  return finish("tracks");
}

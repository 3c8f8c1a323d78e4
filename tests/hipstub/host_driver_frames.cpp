// Drives ph_frames and ph_overlap_add through the HOST half of the library (hip_stub.cpp stands in for the runtime; kernels
// do not run, outputs are not looked at).  Built with -fsanitize=address,undefined by tests/test_host_sanitizers.py:
// argument validation, the host-pointer staging (the signal once, L elements), the size arithmetic with W * N and
// W * K * N beyond 2^31 (sizes only: those calls pass PH_FLAG_DEVICE, so nothing of that size is allocated or touched) and
// W == 1 must touch no byte out of bounds and overflow no integer; every call is one launch of kFramesBlock threads
// without LDS, named k_frames / k_overlap_add in the profile.
#include "driver_common.h"

int main() {
  ph_ctx* c = nullptr;
  EXPECT(ph_create(0, &c), PH_OK);
  EXPECT(ph_profile_enable(c, 1), PH_OK);
  stub_reset_launches();

  // ---- host-pointer staging: {L, N, hop, W, K}; exact-size vectors, so ASan sees any byte read or written past them
  const int shapes[][5] = {{1000, 64, 16, 60, 3}, {997, 63, 3, 312, 1}, {50, 64, 7, 1, 2}, {8, 8, 1, 1, 1},
                           {1000, 64, 80, 13, 2}, {7, 1, 1, 7, 1}, {333, 65, 64, 6, 3}};
  for (const auto& sh : shapes) {
    const int L = sh[0], N = sh[1], hop = sh[2], W = sh[3], K = sh[4];
    std::vector<double> win(N, 0.5), out(L);
    std::vector<int32_t> cnt(W, K);
    for (int in_dt : {PH_F64, PH_F32})
      for (int out_dt : {PH_F64, PH_F32}) {
        std::vector<char> sig((size_t)L * (in_dt == PH_F64 ? 8 : 4)), fr((size_t)W * N * (out_dt == PH_F64 ? 8 : 4));
        for (const double* w : {(const double*)nullptr, (const double*)win.data()}) {
          EXPECT(ph_frames(c, sig.data(), in_dt, L, N, hop, W, w, out_dt, 0, fr.data()), PH_OK);
          one_launch("k_frames", __LINE__);
        }
        // an output that is not 16-byte aligned (device form; the scalar variant is chosen on the host)
        std::vector<char> odd((size_t)W * N * 8 + 16);
        EXPECT(ph_frames(c, sig.data(), in_dt, L, N, hop, W, nullptr, out_dt, PH_FLAG_DEVICE, odd.data() + 8), PH_OK);
        one_launch("k_frames", __LINE__);
      }
    for (int dt : {PH_F64, PH_F32}) {
      std::vector<char> y((size_t)W * K * N * (dt == PH_F64 ? 8 : 4));
      EXPECT(ph_overlap_add(c, y.data(), dt, W, K, N, hop, L, nullptr, nullptr, nullptr, 0, out.data()), PH_OK);
      one_launch("k_overlap_add", __LINE__);
      EXPECT(ph_overlap_add(c, y.data(), dt, W, K, N, hop, L, cnt.data(), win.data(), win.data(), PH_FLAG_OLA_NORM, out.data()),
             PH_OK);
      one_launch("k_overlap_add", __LINE__);
      EXPECT(ph_overlap_add(c, y.data(), dt, W, K, N, hop, L, cnt.data(), nullptr, win.data(),
                            PH_FLAG_DEVICE | PH_FLAG_OLA_NORM, out.data()), PH_OK);
      one_launch("k_overlap_add", __LINE__);
    }
  }

  // ---- sizes beyond 2^31 elements, device form: the pointers are never dereferenced on the host
  {
    double tiny[2] = {0, 0};
    const int64_t W = (int64_t)1 << 21;           // W * N = 2^33, W * K * N = 5 * 2^33
    const int N = 4096, hop = 512, K = 5;
    const int64_t L = (W - 1) * hop + N;          // > 2^30
    EXPECT(ph_frames(c, tiny, PH_F32, L, N, hop, W, nullptr, PH_F64, PH_FLAG_DEVICE, tiny), PH_OK);
    one_launch("k_frames", __LINE__);
    EXPECT(ph_overlap_add(c, tiny, PH_F64, W, K, N, hop, L, nullptr, nullptr, nullptr, PH_FLAG_DEVICE, tiny), PH_OK);
    one_launch("k_overlap_add", __LINE__);
    // f * hop beyond 2^31 as well: hop of 2^20 over 2^12 frames
    const int64_t W2 = 4096, L2 = (W2 - 1) * ((int64_t)1 << 20) + 1;
    EXPECT(ph_frames(c, tiny, PH_F64, L2, 8, 1 << 20, W2, nullptr, PH_F64, PH_FLAG_DEVICE, tiny), PH_OK);
    one_launch("k_frames", __LINE__);
    EXPECT(ph_overlap_add(c, tiny, PH_F32, W2, 1, 8, 1 << 20, L2, nullptr, nullptr, nullptr, PH_FLAG_DEVICE, tiny), PH_OK);
    one_launch("k_overlap_add", __LINE__);
    // an element count that does not fit 64 bits is refused, not wrapped
    EXPECT(ph_frames(c, tiny, PH_F64, INT64_MAX, INT32_MAX, 1, INT64_MAX / 2, nullptr, PH_F64, PH_FLAG_DEVICE, tiny), PH_E_ARG);
    EXPECT(ph_overlap_add(c, tiny, PH_F64, INT64_MAX / 2, INT32_MAX, INT32_MAX, 1, INT64_MAX, nullptr, nullptr, nullptr,
                          PH_FLAG_DEVICE, tiny), PH_E_ARG);
    no_launch(__LINE__);
  }

  // ---- refused, not read
  {
    std::vector<double> sig(100), fr(4 * 16), y(4 * 2 * 16), out(100);
    for (unsigned dev : {0u, (unsigned)PH_FLAG_DEVICE}) {
#define FR(ctx, s, idt, L, N, hop, W, odt, o) ph_frames(ctx, s, idt, L, N, hop, W, nullptr, odt, dev, o)
      EXPECT(FR(nullptr, sig.data(), PH_F64, 100, 16, 8, 4, PH_F64, fr.data()), PH_E_ARG);
      EXPECT(FR(c, nullptr, PH_F64, 100, 16, 8, 4, PH_F64, fr.data()), PH_E_ARG);
      EXPECT(FR(c, sig.data(), PH_F64, 100, 16, 8, 4, PH_F64, nullptr), PH_E_ARG);
      EXPECT(FR(c, sig.data(), 2, 100, 16, 8, 4, PH_F64, fr.data()), PH_E_ARG);
      EXPECT(FR(c, sig.data(), PH_F64, 100, 16, 8, 4, -1, fr.data()), PH_E_ARG);
      EXPECT(FR(c, sig.data(), PH_F64, 0, 16, 8, 4, PH_F64, fr.data()), PH_E_ARG);
      EXPECT(FR(c, sig.data(), PH_F64, 100, 0, 8, 4, PH_F64, fr.data()), PH_E_ARG);
      EXPECT(FR(c, sig.data(), PH_F64, 100, 16, 0, 4, PH_F64, fr.data()), PH_E_ARG);
      EXPECT(FR(c, sig.data(), PH_F64, 100, 16, -3, 4, PH_F64, fr.data()), PH_E_ARG);
      EXPECT(FR(c, sig.data(), PH_F64, 100, 16, 8, 0, PH_F64, fr.data()), PH_E_ARG);
      EXPECT(FR(c, sig.data(), PH_F64, 24, 16, 8, 4, PH_F64, fr.data()), PH_E_ARG);  // (W - 1) hop == L
      EXPECT(FR(c, sig.data(), PH_F64, 23, 16, 8, 4, PH_F64, fr.data()), PH_E_ARG);  // (W - 1) hop > L
#undef FR
#define OA(ctx, yy, dt, W, K, N, hop, L, o) ph_overlap_add(ctx, yy, dt, W, K, N, hop, L, nullptr, nullptr, nullptr, dev, o)
      EXPECT(OA(nullptr, y.data(), PH_F64, 4, 2, 16, 8, 100, out.data()), PH_E_ARG);
      EXPECT(OA(c, nullptr, PH_F64, 4, 2, 16, 8, 100, out.data()), PH_E_ARG);
      EXPECT(OA(c, y.data(), PH_F64, 4, 2, 16, 8, 100, nullptr), PH_E_ARG);
      EXPECT(OA(c, y.data(), 7, 4, 2, 16, 8, 100, out.data()), PH_E_ARG);
      EXPECT(OA(c, y.data(), PH_F64, 0, 2, 16, 8, 100, out.data()), PH_E_ARG);
      EXPECT(OA(c, y.data(), PH_F64, 4, 0, 16, 8, 100, out.data()), PH_E_ARG);
      EXPECT(OA(c, y.data(), PH_F64, 4, 2, 0, 8, 100, out.data()), PH_E_ARG);
      EXPECT(OA(c, y.data(), PH_F64, 4, 2, 16, 0, 100, out.data()), PH_E_ARG);
      EXPECT(OA(c, y.data(), PH_F64, 4, 2, 16, 8, 0, out.data()), PH_E_ARG);
      EXPECT(OA(c, y.data(), PH_F64, 4, 2, 16, 8, 24, out.data()), PH_E_ARG);  // (W - 1) hop == L
#undef OA
      no_launch(__LINE__);
    }
    // the last admissible length: frame W - 1 starts on the last sample
    EXPECT(ph_frames(c, sig.data(), PH_F64, 25, 16, 8, 4, nullptr, PH_F64, 0, fr.data()), PH_OK);
    one_launch("k_frames", __LINE__);
    EXPECT(ph_overlap_add(c, y.data(), PH_F64, 4, 2, 16, 8, 25, nullptr, nullptr, nullptr, 0, out.data()), PH_OK);
    one_launch("k_overlap_add", __LINE__);
  }

  // ---- the profile name of every launch (the profile keeps the first 256)
  float ms[300];
  int cntp = 0;
  EXPECT(ph_profile_read(c, ms, 300, &cntp), PH_OK);
  check_profile(c, cntp);
  EXPECT(ph_sync(c), PH_OK);
  EXPECT(ph_destroy(c), PH_OK);
  return finish("frames");
}

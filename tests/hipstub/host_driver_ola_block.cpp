// Drives ph_overlap_add_block and ph_overlap_add_finish through the HOST half of the library (hip_stub.cpp stands in for the
// runtime; kernels do not run, outputs are not looked at).  Built with -fsanitize=address,undefined by
// tests/test_host_sanitizers_blocks.py: every refusal, the host-pointer staging of y, counts, masks, the window and of acc
// BOTH ways with exact-size vectors (finish with out == acc too), NULL optional pointers, and the size arithmetic with
// f0 * hop, Wb * K * N and T * L beyond 2^31 (sizes only: those calls pass PH_FLAG_DEVICE, so nothing of that size is
// allocated or touched) must touch no byte out of bounds and overflow no integer; every accepted call is one launch of
// kFramesBlock threads without LDS, named after its kernel.
#include "driver_common.h"

int main() {
  ph_ctx* c = nullptr;
  EXPECT(ph_create(0, &c), PH_OK);
  EXPECT(ph_profile_enable(c, 1), PH_OK);
  stub_reset_launches();

  // ---- host-pointer staging: {L, N, hop, W, K, T, B}; a recording of W frames in blocks of B
  const int shapes[][7] = {{1000, 64, 16, 60, 3, 2, 7}, {997, 63, 3, 312, 1, 1, 100}, {50, 64, 7, 1, 2, 5, 1}, {8, 8, 1, 1, 1, 1, 4},
                           {1000, 64, 80, 13, 64, 3, 12}, {7, 1, 1, 7, 1, 9, 2}, {333, 65, 64, 6, 70, 1, 5}};
  for (const auto& sh : shapes) {
    const int L = sh[0], N = sh[1], hop = sh[2], W = sh[3], K = sh[4], T = sh[5], B = sh[6];
    std::vector<double> win(N, 0.5), acc1(L), accT((size_t)T * L), out((size_t)T * L);
    for (int dt : {PH_F64, PH_F32}) {
      for (int f0 = 0; f0 < W; f0 += B) {
        const int Wb = f0 + B <= W ? B : W - f0;
        std::vector<char> y((size_t)Wb * K * N * (dt == PH_F64 ? 8 : 4));
        std::vector<int32_t> cnt(Wb, K);
        std::vector<uint64_t> masks((size_t)T * Wb, ~0ull);
        // no masks: one track, any K; NULL optional pointers
        EXPECT(ph_overlap_add_block(c, y.data(), dt, Wb, K, N, hop, L, f0, nullptr, nullptr, 1, nullptr, 0, acc1.data()), PH_OK);
        one_launch("k_overlap_add_block", __LINE__);
        EXPECT(ph_overlap_add_block(c, y.data(), dt, Wb, K, N, hop, L, f0, cnt.data(), nullptr, 1, win.data(), 0, acc1.data()),
               PH_OK);
        one_launch("k_overlap_add_block", __LINE__);
        if (K <= 64) {
          EXPECT(ph_overlap_add_block(c, y.data(), dt, Wb, K, N, hop, L, f0, cnt.data(), masks.data(), T, win.data(), 0,
                                      accT.data()), PH_OK);
          one_launch("k_overlap_add_block", __LINE__);
          EXPECT(ph_overlap_add_block(c, y.data(), dt, Wb, K, N, hop, L, f0, nullptr, masks.data(), T, nullptr, PH_FLAG_DEVICE,
                                      accT.data()), PH_OK);
          one_launch("k_overlap_add_block", __LINE__);
        }
      }
    }
    EXPECT(ph_overlap_add_finish(c, accT.data(), T, N, hop, L, W, nullptr, nullptr, 0, out.data()), PH_OK);
    one_launch("k_overlap_add_finish", __LINE__);
    EXPECT(ph_overlap_add_finish(c, accT.data(), T, N, hop, L, W, win.data(), win.data(), PH_FLAG_OLA_NORM, accT.data()), PH_OK);
    one_launch("k_overlap_add_finish", __LINE__);  // in place
    EXPECT(ph_overlap_add_finish(c, acc1.data(), 1, N, hop, L, W, nullptr, win.data(), PH_FLAG_DEVICE | PH_FLAG_OLA_NORM,
                                 acc1.data()), PH_OK);
    one_launch("k_overlap_add_finish", __LINE__);
  }

  // ---- acc really travels both ways: the stub's kernels do nothing, so the values must come back as they went up
  {
    const int L = 100, N = 16, hop = 8, Wb = 4, T = 3;
    std::vector<double> y((size_t)Wb * 2 * N), acc((size_t)T * L);
    std::vector<uint64_t> masks((size_t)T * Wb, 1);
    for (size_t i = 0; i < acc.size(); ++i) acc[i] = (double)i + 0.25;
    EXPECT(ph_overlap_add_block(c, y.data(), PH_F64, Wb, 2, N, hop, L, 5, nullptr, masks.data(), T, nullptr, 0, acc.data()), PH_OK);
    one_launch("k_overlap_add_block", __LINE__);
    for (size_t i = 0; i < acc.size(); ++i)
      if (acc[i] != (double)i + 0.25) {
        std::printf("FAIL acc[%zu] came back as %g\n", i, acc[i]);
        ++fails;
        break;
      }
  }

  // ---- sizes beyond 2^31, device form: the pointers are never dereferenced on the host
  {
    double tiny[2] = {0, 0};
    const uint64_t* tm = reinterpret_cast<const uint64_t*>(tiny);
    const int64_t W = (int64_t)1 << 22, Wb = (int64_t)1 << 21;  // Wb * K * N = 5 * 2^33, f0 * hop = 2^30 .. 2^31
    const int N = 4096, hop = 512, K = 5;
    const int64_t L = (W - 1) * hop + N;  // > 2^31
    for (int64_t f0 : {(int64_t)0, Wb}) {
      EXPECT(ph_overlap_add_block(c, tiny, PH_F64, Wb, K, N, hop, L, f0, nullptr, nullptr, 1, nullptr, PH_FLAG_DEVICE, tiny), PH_OK);
      one_launch("k_overlap_add_block", __LINE__);
      EXPECT(ph_overlap_add_block(c, tiny, PH_F32, Wb, 64, N, hop, L, f0, nullptr, tm, 9, nullptr, PH_FLAG_DEVICE, tiny), PH_OK);
      one_launch("k_overlap_add_block", __LINE__);
    }
    EXPECT(ph_overlap_add_finish(c, tiny, 9, N, hop, L, W, nullptr, nullptr, PH_FLAG_DEVICE | PH_FLAG_OLA_NORM, tiny), PH_OK);
    one_launch("k_overlap_add_finish", __LINE__);
    // f0 * hop far beyond 2^31: hop of 2^20, a one-frame block at frame 2^22
    const int64_t f1 = (int64_t)1 << 22, L1 = f1 * ((int64_t)1 << 20) + 1;
    EXPECT(ph_overlap_add_block(c, tiny, PH_F32, 1, 1, 8, 1 << 20, L1, f1, nullptr, tm, 2, nullptr, PH_FLAG_DEVICE, tiny), PH_OK);
    one_launch("k_overlap_add_block", __LINE__);
    EXPECT(ph_overlap_add_block(c, tiny, PH_F32, 1, 1, 8, 1 << 20, L1, f1 + 1, nullptr, tm, 2, nullptr, PH_FLAG_DEVICE, tiny),
           PH_E_ARG);
    said("behind", __LINE__);
    // the last frame the signal admits, from the largest f0 and from the largest Wb
    EXPECT(ph_overlap_add_block(c, tiny, PH_F64, 1, 1, 8, 1, INT64_MAX / 8, INT64_MAX / 8 - 1, nullptr, nullptr, 1, nullptr,
                                PH_FLAG_DEVICE, tiny), PH_OK);
    one_launch("k_overlap_add_block", __LINE__);
    EXPECT(ph_overlap_add_block(c, tiny, PH_F64, 1, 1, 8, 1, INT64_MAX / 8, INT64_MAX / 8, nullptr, nullptr, 1, nullptr,
                                PH_FLAG_DEVICE, tiny), PH_E_ARG);
    EXPECT(ph_overlap_add_block(c, tiny, PH_F64, 2, 1, 8, 1, INT64_MAX / 8, INT64_MAX / 8 - 1, nullptr, nullptr, 1, nullptr,
                                PH_FLAG_DEVICE, tiny), PH_E_ARG);
    EXPECT(ph_overlap_add_block(c, tiny, PH_F64, INT64_MAX, 1, 8, 1, INT64_MAX / 8, INT64_MAX, nullptr, nullptr, 1, nullptr,
                                PH_FLAG_DEVICE, tiny), PH_E_ARG);  // f0 + Wb would overflow
    // byte counts that do not fit 64 bits are refused, not wrapped: Wb * K * N, T * L, T * Wb
    EXPECT(ph_overlap_add_block(c, tiny, PH_F64, INT64_MAX / 2, 64, INT32_MAX, 1, INT64_MAX, 0, nullptr, nullptr, 1, nullptr,
                                PH_FLAG_DEVICE, tiny), PH_E_ARG);
    said("W * K * N", __LINE__);
    EXPECT(ph_overlap_add_block(c, tiny, PH_F64, 4, 2, 16, 8, INT64_MAX / 16, 3, nullptr, tm, 3, nullptr, PH_FLAG_DEVICE, tiny),
           PH_E_ARG);
    said("T * L", __LINE__);
    EXPECT(ph_overlap_add_block(c, tiny, PH_F64, 4, 2, 16, 8, INT64_MAX / 4, 3, nullptr, nullptr, 1, nullptr, PH_FLAG_DEVICE, tiny),
           PH_E_ARG);  // L * 8 alone
    EXPECT(ph_overlap_add_block(c, tiny, PH_F64, (int64_t)1 << 40, 1, 1, 1, (int64_t)1 << 41, 7, nullptr, tm, (int64_t)1 << 21,
                                nullptr, PH_FLAG_DEVICE, tiny), PH_E_ARG);
    EXPECT(ph_overlap_add_block(c, tiny, PH_F64, 4, 2, 16, 8, 100, 3, nullptr, tm, INT64_MAX, nullptr, PH_FLAG_DEVICE, tiny),
           PH_E_ARG);
    EXPECT(ph_overlap_add_finish(c, tiny, 3, 16, 8, INT64_MAX / 16, 12, nullptr, nullptr, PH_FLAG_DEVICE, tiny), PH_E_ARG);
    said("T * L", __LINE__);
    EXPECT(ph_overlap_add_finish(c, tiny, (int64_t)1 << 21, 1, 1, (int64_t)1 << 40, (int64_t)1 << 40, nullptr, nullptr,
                                 PH_FLAG_DEVICE, tiny), PH_E_ARG);
    EXPECT(ph_overlap_add_finish(c, tiny, INT64_MAX, 16, 8, 100, 12, nullptr, nullptr, PH_FLAG_DEVICE, tiny), PH_E_ARG);
    // the largest counts that pass
    EXPECT(ph_overlap_add_block(c, tiny, PH_F64, 4, 2, 16, 8, INT64_MAX / 64, 3, nullptr, tm, 8, nullptr, PH_FLAG_DEVICE, tiny),
           PH_OK);
    one_launch("k_overlap_add_block", __LINE__);
    EXPECT(ph_overlap_add_finish(c, tiny, 8, 16, 8, INT64_MAX / 64, 12, nullptr, nullptr, PH_FLAG_DEVICE, tiny), PH_OK);
    one_launch("k_overlap_add_finish", __LINE__);
    no_launch(__LINE__);
  }

  // ---- refused, not read
  {
    std::vector<double> y(4 * 2 * 16), acc(3 * 100);
    std::vector<uint64_t> masks(3 * 4, 1);
    for (unsigned dev : {0u, (unsigned)PH_FLAG_DEVICE}) {
#define OB(ctx, yy, dt, Wb, K, N, hop, L, f0, mm, T, a) \
  ph_overlap_add_block(ctx, yy, dt, Wb, K, N, hop, L, f0, nullptr, mm, T, nullptr, dev, a)
      EXPECT(OB(nullptr, y.data(), PH_F64, 4, 2, 16, 8, 100, 3, masks.data(), 3, acc.data()), PH_E_ARG);
      said("ctx", __LINE__);
      EXPECT(OB(c, nullptr, PH_F64, 4, 2, 16, 8, 100, 3, masks.data(), 3, acc.data()), PH_E_ARG);
      EXPECT(OB(c, y.data(), PH_F64, 4, 2, 16, 8, 100, 3, masks.data(), 3, nullptr), PH_E_ARG);
      said("acc", __LINE__);
      EXPECT(OB(c, y.data(), 7, 4, 2, 16, 8, 100, 3, masks.data(), 3, acc.data()), PH_E_ARG);
      said("dtype", __LINE__);
      EXPECT(OB(c, y.data(), -1, 4, 2, 16, 8, 100, 3, masks.data(), 3, acc.data()), PH_E_ARG);
      EXPECT(OB(c, y.data(), PH_F64, 0, 2, 16, 8, 100, 3, masks.data(), 3, acc.data()), PH_E_ARG);
      EXPECT(OB(c, y.data(), PH_F64, -2, 2, 16, 8, 100, 3, masks.data(), 3, acc.data()), PH_E_ARG);
      EXPECT(OB(c, y.data(), PH_F64, 4, 0, 16, 8, 100, 3, masks.data(), 3, acc.data()), PH_E_ARG);
      EXPECT(OB(c, y.data(), PH_F64, 4, 2, 0, 8, 100, 3, masks.data(), 3, acc.data()), PH_E_ARG);
      EXPECT(OB(c, y.data(), PH_F64, 4, 2, 16, 0, 100, 3, masks.data(), 3, acc.data()), PH_E_ARG);
      EXPECT(OB(c, y.data(), PH_F64, 4, 2, 16, -3, 100, 3, masks.data(), 3, acc.data()), PH_E_ARG);
      EXPECT(OB(c, y.data(), PH_F64, 4, 2, 16, 8, 0, 0, masks.data(), 3, acc.data()), PH_E_ARG);
      EXPECT(OB(c, y.data(), PH_F64, 4, 2, 16, 8, 100, -1, masks.data(), 3, acc.data()), PH_E_ARG);
      said("f0", __LINE__);
      EXPECT(OB(c, y.data(), PH_F64, 4, 2, 16, 8, 100, INT64_MIN, masks.data(), 3, acc.data()), PH_E_ARG);
      EXPECT(OB(c, y.data(), PH_F64, 4, 2, 16, 8, 100, 10, masks.data(), 3, acc.data()), PH_E_ARG);  // frame 13 at 104
      said("behind", __LINE__);
      EXPECT(OB(c, y.data(), PH_F64, 4, 2, 16, 8, 96, 9, masks.data(), 3, acc.data()), PH_E_ARG);  // (f0 + Wb - 1) hop == L
      said("behind", __LINE__);
      EXPECT(OB(c, y.data(), PH_F64, 4, 2, 16, 8, 24, 0, masks.data(), 3, acc.data()), PH_E_ARG);
      said("behind", __LINE__);
      EXPECT(OB(c, y.data(), PH_F64, 4, 2, 16, 8, 100, INT64_MAX, masks.data(), 3, acc.data()), PH_E_ARG);
      EXPECT(OB(c, y.data(), PH_F64, 4, 2, 16, 8, 100, 3, nullptr, 3, acc.data()), PH_E_ARG);  // no masks: T must be 1
      said("T=3", __LINE__);
      EXPECT(OB(c, y.data(), PH_F64, 4, 2, 16, 8, 100, 3, nullptr, 0, acc.data()), PH_E_ARG);
      EXPECT(OB(c, y.data(), PH_F64, 4, 2, 16, 8, 100, 3, masks.data(), 0, acc.data()), PH_E_ARG);
      said("T=0", __LINE__);
      EXPECT(OB(c, y.data(), PH_F64, 4, 2, 16, 8, 100, 3, masks.data(), -1, acc.data()), PH_E_ARG);
      EXPECT(OB(c, y.data(), PH_F64, 4, 65, 16, 8, 100, 3, masks.data(), 3, acc.data()), PH_E_ARG);  // one row too many
      said("K=65", __LINE__);
      EXPECT(OB(c, y.data(), PH_F64, 4, INT32_MAX, 16, 8, 100, 3, masks.data(), 3, acc.data()), PH_E_ARG);
#undef OB
#define OF(ctx, a, T, N, hop, L, W, o) ph_overlap_add_finish(ctx, a, T, N, hop, L, W, nullptr, nullptr, dev | PH_FLAG_OLA_NORM, o)
      EXPECT(OF(nullptr, acc.data(), 3, 16, 8, 100, 12, acc.data()), PH_E_ARG);
      said("ctx", __LINE__);
      EXPECT(OF(c, nullptr, 3, 16, 8, 100, 12, acc.data()), PH_E_ARG);
      said("acc", __LINE__);
      EXPECT(OF(c, acc.data(), 3, 16, 8, 100, 12, nullptr), PH_E_ARG);
      EXPECT(OF(c, acc.data(), 0, 16, 8, 100, 12, acc.data()), PH_E_ARG);
      said("T=0", __LINE__);
      EXPECT(OF(c, acc.data(), -1, 16, 8, 100, 12, acc.data()), PH_E_ARG);
      EXPECT(OF(c, acc.data(), 3, 0, 8, 100, 12, acc.data()), PH_E_ARG);
      EXPECT(OF(c, acc.data(), 3, 16, 0, 100, 12, acc.data()), PH_E_ARG);
      EXPECT(OF(c, acc.data(), 3, 16, -8, 100, 12, acc.data()), PH_E_ARG);
      EXPECT(OF(c, acc.data(), 3, 16, 8, 0, 12, acc.data()), PH_E_ARG);
      EXPECT(OF(c, acc.data(), 3, 16, 8, 100, 0, acc.data()), PH_E_ARG);
      EXPECT(OF(c, acc.data(), 3, 16, 8, 100, -5, acc.data()), PH_E_ARG);
      EXPECT(OF(c, acc.data(), 3, 16, 8, 100, 14, acc.data()), PH_E_ARG);  // (W - 1) hop = 104 >= L
      said("behind", __LINE__);
#undef OF
      no_launch(__LINE__);
    }
    // the last admissible block, K = 65 without masks, K = 64 with them
    EXPECT(ph_overlap_add_block(c, y.data(), PH_F64, 4, 2, 16, 8, 100, 9, nullptr, masks.data(), 3, nullptr, 0, acc.data()), PH_OK);
    one_launch("k_overlap_add_block", __LINE__);
    std::vector<double> y65(4 * 65 * 16);
    EXPECT(ph_overlap_add_block(c, y65.data(), PH_F64, 4, 65, 16, 8, 100, 3, nullptr, nullptr, 1, nullptr, 0, acc.data()), PH_OK);
    one_launch("k_overlap_add_block", __LINE__);
    EXPECT(ph_overlap_add_block(c, y65.data(), PH_F64, 4, 64, 16, 8, 100, 3, nullptr, masks.data(), 3, nullptr, 0, acc.data()), PH_OK);
    one_launch("k_overlap_add_block", __LINE__);
    EXPECT(ph_overlap_add_finish(c, acc.data(), 3, 16, 8, 100, 13, nullptr, nullptr, 0, acc.data()), PH_OK);
    one_launch("k_overlap_add_finish", __LINE__);
  }

  // ---- the profile name of every launch (the profile keeps the first 256)
  float ms[300];
  int cntp = 0;
  EXPECT(ph_profile_read(c, ms, 300, &cntp), PH_OK);
  check_profile(c, cntp);
  EXPECT(ph_sync(c), PH_OK);
  EXPECT(ph_destroy(c), PH_OK);
  return finish("ola_block");
}

// Drives ph_follow_residual through the HOST half of the library (hip_stub.cpp stands in for the runtime; kernels do not
// run, outputs are not looked at).  Built with -fsanitize=address,undefined by
// tests/test_host_sanitizers_follow_residual.py: every refusal, pcap == 0 with NULL periods and counts, the host-pointer
// staging with exact-size vectors (the signal goes up once, L elements of its dtype; periods and counts are the block's),
// and the size arithmetic with f0 * hop and Wb * N beyond 2^31 must touch no byte out of bounds and overflow no integer;
// every accepted call is one launch with the block and the LDS bytes of ph_follow_plan_info, named k_follow_residual.
#include "driver_common.h"

// one launch since the last reset, with the plan query's block and LDS for frames of N samples
static void residual_launch(ph_ctx* c, int N, int line) {
  int block[4];
  long long l[4];
  int pb = 0, pl = 0, pw = 0;
  EXPECT(ph_follow_plan_info(c, N, &pb, &pl, &pw), PH_OK);
  const int n = stub_launches(block, l, 4);
  if (n != 1 || block[0] != pb || l[0] != pl) {
    std::printf("FAIL line %d: %d launches, block %d (plan %d), lds %lld (plan %d)\n", line, n, n ? block[0] : -1, pb,
                n ? l[0] : -1LL, pl);
    ++fails;
  }
  launched("k_follow_residual");
  stub_reset_launches();
}

int main() {
  ph_ctx* c = nullptr;
  EXPECT(ph_create(0, &c), PH_OK);
  EXPECT(ph_profile_enable(c, 1), PH_OK);
  stub_reset_launches();

  // ---- host-pointer staging: {L, N, hop, f0, Wb, pcap}; N = 20000 does not fit the LDS twice (workspace placement)
  const int shapes[][6] = {{1, 1, 1, 0, 1, 1},        {40, 16, 8, 0, 4, 3},         {40, 16, 8, 3, 2, 3},   {33, 16, 8, 4, 1, 1},
                           {100, 37, 5, 7, 13, 64},   {5000, 4096, 512, 1, 2, 4},   {300, 64, 64, 2, 3, 2}, {200, 48, 61, 1, 3, 3},
                           {50000, 20000, 10000, 2, 3, 2}};
  for (const auto& sh : shapes) {
    const int L = sh[0], N = sh[1], hop = sh[2], f0 = sh[3], Wb = sh[4], pcap = sh[5];
    std::vector<double> s64(L, 0.5), win(N, 1.0), out((size_t)Wb * N);  // exact sizes
    std::vector<float> s32(L, 0.5f);
    std::vector<int32_t> periods((size_t)Wb * pcap, 1), counts(Wb, pcap);
    EXPECT(ph_follow_residual(c, s64.data(), PH_F64, L, N, hop, f0, Wb, win.data(), PH_F64, periods.data(), counts.data(),
                              pcap, 0, out.data()), PH_OK);
    residual_launch(c, N, __LINE__);
    EXPECT(ph_follow_residual(c, s32.data(), PH_F32, L, N, hop, f0, Wb, nullptr, PH_F32, periods.data(), counts.data(), pcap,
                              PH_FLAG_TRUNC, out.data()), PH_OK);
    residual_launch(c, N, __LINE__);
    EXPECT(ph_follow_residual(c, s32.data(), PH_F32, L, N, hop, f0, Wb, win.data(), PH_F64, periods.data(), counts.data(),
                              pcap, PH_FLAG_DEVICE | PH_FLAG_TRUNC, out.data()), PH_OK);
    residual_launch(c, N, __LINE__);
    // no tracks: periods and counts may be NULL, or present and not read
    EXPECT(ph_follow_residual(c, s64.data(), PH_F64, L, N, hop, f0, Wb, win.data(), PH_F32, nullptr, nullptr, 0, 0,
                              out.data()), PH_OK);
    residual_launch(c, N, __LINE__);
    EXPECT(ph_follow_residual(c, s32.data(), PH_F32, L, N, hop, f0, Wb, nullptr, PH_F64, periods.data(), nullptr, 0,
                              PH_FLAG_DEVICE, out.data()), PH_OK);
    residual_launch(c, N, __LINE__);
  }

  // ---- sizes beyond 2^31, device form: the pointers are never dereferenced on the host
  {
    double tiny[2] = {0, 0};
    int32_t* ti = reinterpret_cast<int32_t*>(tiny);
    const int64_t M = (int64_t)1 << 20;
    // f0 * hop = 2^40 samples in front of the block, Wb * N = 2^32 doubles
    EXPECT(ph_follow_residual(c, tiny, PH_F32, (M + M - 1) * M + 1, 4096, 1 << 20, M, M, tiny, PH_F64, ti, ti, 64,
                              PH_FLAG_DEVICE, tiny), PH_OK);
    residual_launch(c, 4096, __LINE__);
    // hop at the top of int, the block at the far end of the recording
    EXPECT(ph_follow_residual(c, tiny, PH_F64, (int64_t)1 << 58, 1000, INT32_MAX, ((int64_t)1 << 27) - 5, 5, nullptr, PH_F32,
                              nullptr, nullptr, 0, PH_FLAG_DEVICE, tiny), PH_OK);
    residual_launch(c, 1000, __LINE__);
    // f0 at the top of int64: f0 + Wb is never formed
    EXPECT(ph_follow_residual(c, tiny, PH_F64, 100, 16, 8, INT64_MAX, 4, nullptr, PH_F64, ti, ti, 1, PH_FLAG_DEVICE, tiny),
           PH_E_ARG);
    said(">= L", __LINE__);
    EXPECT(ph_follow_residual(c, tiny, PH_F64, 100, 16, 8, INT64_MAX - 2, 4, nullptr, PH_F64, ti, ti, 1, PH_FLAG_DEVICE, tiny),
           PH_E_ARG);
    said(">= L", __LINE__);
    // byte counts that do not fit 64 bits are refused, not wrapped (nothing is allocated for them)
    EXPECT(ph_follow_residual(c, tiny, PH_F64, INT64_MAX, 16, 8, 0, 4, nullptr, PH_F64, ti, ti, 1, PH_FLAG_DEVICE, tiny),
           PH_E_ARG);
    said("64 bits", __LINE__);
    EXPECT(ph_follow_residual(c, tiny, PH_F64, INT64_MAX / 8 + 1, 16, 8, 0, 4, nullptr, PH_F64, ti, ti, 1, PH_FLAG_DEVICE,
                              tiny), PH_E_ARG);
    said("64 bits", __LINE__);
    // Wb * N * 8 = 2^64
    EXPECT(ph_follow_residual(c, tiny, PH_F64, (int64_t)1 << 59, 16, 1, 0, (int64_t)1 << 57, nullptr, PH_F64, ti, ti, 1,
                              PH_FLAG_DEVICE, tiny), PH_E_ARG);
    said("64 bits", __LINE__);
    // Wb * pcap * 4 = 2^65 while Wb * N * 8 = 2^60 fits
    EXPECT(ph_follow_residual(c, tiny, PH_F64, (int64_t)1 << 58, 1, 1, 0, (int64_t)1 << 57, nullptr, PH_F64, ti, ti, 64,
                              PH_FLAG_DEVICE, tiny), PH_E_ARG);
    said("Wb * pcap", __LINE__);
    no_launch(__LINE__);
  }

  // ---- refused, not read
  {
    std::vector<double> s(40), win(16), out(4 * 16);
    std::vector<int32_t> periods(4 * 3, 2), counts(4, 3);
    for (unsigned dev : {0u, (unsigned)PH_FLAG_DEVICE}) {
#define FR(ctx, sig, idt, L, N, hop, f0, Wb, fdt, per, cnt, pcap, o) \
  ph_follow_residual(ctx, sig, idt, L, N, hop, f0, Wb, win.data(), fdt, per, cnt, pcap, dev, o)
      EXPECT(FR(nullptr, s.data(), PH_F64, 40, 16, 8, 0, 4, PH_F64, periods.data(), counts.data(), 3, out.data()), PH_E_ARG);
      said("ctx", __LINE__);
      EXPECT(FR(c, nullptr, PH_F64, 40, 16, 8, 0, 4, PH_F64, periods.data(), counts.data(), 3, out.data()), PH_E_ARG);
      said("NULL", __LINE__);
      EXPECT(FR(c, s.data(), PH_F64, 40, 16, 8, 0, 4, PH_F64, periods.data(), counts.data(), 3, nullptr), PH_E_ARG);
      said("NULL", __LINE__);
      EXPECT(FR(c, s.data(), PH_F64, 40, 16, 8, 0, 4, PH_F64, nullptr, counts.data(), 3, out.data()), PH_E_ARG);
      said("pcap", __LINE__);
      EXPECT(FR(c, s.data(), PH_F64, 40, 16, 8, 0, 4, PH_F64, periods.data(), nullptr, 3, out.data()), PH_E_ARG);
      said("pcap", __LINE__);
      EXPECT(FR(c, s.data(), PH_F64, 40, 16, 8, 0, 4, PH_F64, nullptr, nullptr, 1, out.data()), PH_E_ARG);
      said("NULL", __LINE__);
      for (int bad : {2, -1, 99}) {
        EXPECT(FR(c, s.data(), bad, 40, 16, 8, 0, 4, PH_F64, periods.data(), counts.data(), 3, out.data()), PH_E_ARG);
        said("dtype", __LINE__);
        EXPECT(FR(c, s.data(), PH_F64, 40, 16, 8, 0, 4, bad, periods.data(), counts.data(), 3, out.data()), PH_E_ARG);
        said("dtype", __LINE__);
      }
      for (int64_t bad : {(int64_t)0, (int64_t)-1, INT64_MIN}) {
        EXPECT(FR(c, s.data(), PH_F64, bad, 16, 8, 0, 4, PH_F64, periods.data(), counts.data(), 3, out.data()), PH_E_ARG);
        said(">= 1", __LINE__);
        EXPECT(FR(c, s.data(), PH_F64, 40, 16, 8, 0, bad, PH_F64, periods.data(), counts.data(), 3, out.data()), PH_E_ARG);
        said(">= 1", __LINE__);
      }
      for (int bad : {0, -1, INT32_MIN}) {
        EXPECT(FR(c, s.data(), PH_F64, 40, bad, 8, 0, 4, PH_F64, periods.data(), counts.data(), 3, out.data()), PH_E_ARG);
        said(">= 1", __LINE__);
        EXPECT(FR(c, s.data(), PH_F64, 40, 16, bad, 0, 4, PH_F64, periods.data(), counts.data(), 3, out.data()), PH_E_ARG);
        said(">= 1", __LINE__);
      }
      for (int64_t bad : {(int64_t)-1, INT64_MIN}) {
        EXPECT(FR(c, s.data(), PH_F64, 40, 16, 8, bad, 4, PH_F64, periods.data(), counts.data(), 3, out.data()), PH_E_ARG);
        said("f0", __LINE__);
      }
      // a frame that starts at or behind the end of the signal: (f0 + Wb - 1) * hop = 40 >= L
      EXPECT(FR(c, s.data(), PH_F64, 40, 16, 8, 0, 6, PH_F64, periods.data(), counts.data(), 3, out.data()), PH_E_ARG);
      said(">= L", __LINE__);
      EXPECT(FR(c, s.data(), PH_F64, 40, 16, 8, 2, 4, PH_F64, periods.data(), counts.data(), 3, out.data()), PH_E_ARG);
      said(">= L", __LINE__);
      EXPECT(FR(c, s.data(), PH_F64, 40, 16, 8, 5, 1, PH_F64, periods.data(), counts.data(), 3, out.data()), PH_E_ARG);
      said(">= L", __LINE__);
      EXPECT(FR(c, s.data(), PH_F64, 40, 16, INT32_MAX, 1, 1, PH_F64, periods.data(), counts.data(), 3, out.data()), PH_E_ARG);
      EXPECT(FR(c, s.data(), PH_F64, 40, 16, 8, 0, INT64_MAX, PH_F64, periods.data(), counts.data(), 3, out.data()), PH_E_ARG);
      for (int bad : {-1, 65, INT32_MIN, INT32_MAX}) {
        EXPECT(FR(c, s.data(), PH_F64, 40, 16, 8, 0, 4, PH_F64, periods.data(), counts.data(), bad, out.data()), PH_E_ARG);
        said("pcap", __LINE__);
      }
      no_launch(__LINE__);
#undef FR
    }
    // the limits themselves: the block's last frame starts on the last sample; pcap = 64
    std::vector<int32_t> p64(3 * 64, 1), c3(3, 64);
    out.assign(3 * 16, 0.0);
    s.assign(33, 0.0);
    EXPECT(ph_follow_residual(c, s.data(), PH_F64, 33, 16, 8, 2, 3, win.data(), PH_F64, p64.data(), c3.data(), 64, 0,
                              out.data()), PH_OK);
    residual_launch(c, 16, __LINE__);
  }

  // ---- the profile name of every launch
  float ms[300];
  int cntp = 0;
  EXPECT(ph_profile_read(c, ms, 300, &cntp), PH_OK);
  check_profile(c, cntp);
  EXPECT(ph_sync(c), PH_OK);
  EXPECT(ph_destroy(c), PH_OK);
  return finish("follow_residual");
}

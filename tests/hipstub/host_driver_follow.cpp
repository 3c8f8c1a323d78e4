// Drives ph_follow and ph_follow_plan_info through the HOST half of the library (hip_stub.cpp stands in for the runtime;
// kernels do not run, outputs are not looked at).  Built with -fsanitize=address,undefined by
// tests/test_host_sanitizers_follow.py: every refusal, the host-pointer staging with exact-size vectors (the signal goes
// up once, L elements of its dtype; seg travels both ways), and the size arithmetic with W * ccap and W * hop beyond 2^31
// must touch no byte out of bounds and overflow no integer; every accepted call is one launch with the block and the LDS
// bytes of the plan query, named k_follow.
#include "driver_common.h"

// one launch since the last reset, with the plan query's block and LDS for frames of N samples
static void follow_launch(ph_ctx* c, int N, int line) {
  int block[4];
  long long l[4];
  int pb = 0, pl = 0, pw = 0;
  EXPECT(ph_follow_plan_info(c, N, &pb, &pl, &pw), PH_OK);
  int want_block = ((N + 3) / 4 + 63) / 64 * 64;  // a quarter of the frame in whole wavefronts, 64 .. 1024
  want_block = want_block < 64 ? 64 : want_block > 1024 ? 1024 : want_block;
  const int n = stub_launches(block, l, 4);
  if (n != 1 || block[0] != pb || l[0] != pl || pb != want_block || (pw != PH_PLAN_LDS && pw != PH_PLAN_HBM) ||
      (pw == PH_PLAN_LDS && pl < 16 * N) || (pw == PH_PLAN_HBM && pl >= 16 * N)) {
    std::printf("FAIL line %d: %d launches, block %d (plan %d, want %d), lds %lld (plan %d), placement %d\n", line, n,
                n ? block[0] : -1, pb, want_block, n ? l[0] : -1LL, pl, pw);
    ++fails;
  }
  launched("k_follow");
  stub_reset_launches();
}

int main() {
  ph_ctx* c = nullptr;
  EXPECT(ph_create(0, &c), PH_OK);
  EXPECT(ph_profile_enable(c, 1), PH_OK);
  stub_reset_launches();

  // ---- host-pointer staging: {L, N, hop, W, pcap, ccap}; N = 20000 does not fit the LDS twice (workspace placement)
  const int shapes[][6] = {{1, 1, 1, 1, 1, 1},      {40, 16, 8, 4, 3, 20},   {33, 16, 8, 5, 1, 1},   {100, 37, 5, 13, 64, 74},
                           {5000, 4096, 512, 3, 4, 9000}, {300, 64, 64, 5, 2, 128}, {200, 48, 61, 4, 3, 70},
                           {50000, 20000, 10000, 4, 2, 40000}};
  for (const auto& sh : shapes) {
    const int L = sh[0], N = sh[1], hop = sh[2], W = sh[3], pcap = sh[4], ccap = sh[5];
    std::vector<double> s64(L, 0.5), win(N, 1.0), seg((size_t)W * ccap), powers((size_t)W * pcap);  // exact sizes
    std::vector<float> s32(L, 0.5f);
    std::vector<int32_t> periods((size_t)W * pcap, 1), counts(W, pcap), done(W);
    EXPECT(ph_follow(c, s64.data(), PH_F64, L, N, hop, W, win.data(), PH_F64, periods.data(), counts.data(), pcap, ccap, 0,
                     seg.data(), powers.data(), done.data()), PH_OK);
    follow_launch(c, N, __LINE__);
    EXPECT(ph_follow(c, s32.data(), PH_F32, L, N, hop, W, nullptr, PH_F32, periods.data(), counts.data(), pcap, ccap,
                     PH_FLAG_TRUNC, seg.data(), powers.data(), done.data()), PH_OK);
    follow_launch(c, N, __LINE__);
    EXPECT(ph_follow(c, s32.data(), PH_F32, L, N, hop, W, win.data(), PH_F64, periods.data(), counts.data(), pcap, ccap,
                     PH_FLAG_DEVICE | PH_FLAG_TRUNC, seg.data(), powers.data(), done.data()), PH_OK);
    follow_launch(c, N, __LINE__);
  }

  // ---- the plan query
  {
    int last_lds = 0;
    for (int N : {1, 2, 63, 64, 65, 255, 256, 257, 1024, 4096, 4097, 9000}) {
      int block = 0, lds = 0, where = 0;
      EXPECT(ph_follow_plan_info(c, N, &block, &lds, &where), PH_OK);
      if (block < 64 || block > 1024 || block % 64 || lds > 160 * 1024 || lds < last_lds || where != PH_PLAN_LDS ||
          (long long)block * 4 < (N < 4096 ? N : 4096)) {
        std::printf("FAIL plan N=%d: block %d, lds %d, placement %d\n", N, block, lds, where);
        ++fails;
      }
      last_lds = lds;
    }
    int block = 0, lds = 0, where = 0;
    EXPECT(ph_follow_plan_info(c, 1 << 20, &block, &lds, &where), PH_OK);  // far beyond the LDS: the workspace
    if (where != PH_PLAN_HBM || block != 1024 || lds > 1024) {
      std::printf("FAIL plan N=2^20: block %d, lds %d, placement %d\n", block, lds, where);
      ++fails;
    }
    int x = 0;
    EXPECT(ph_follow_plan_info(nullptr, 64, &x, &x, &x), PH_E_ARG);
    EXPECT(ph_follow_plan_info(c, 64, nullptr, &x, &x), PH_E_ARG);
    EXPECT(ph_follow_plan_info(c, 64, &x, nullptr, &x), PH_E_ARG);
    EXPECT(ph_follow_plan_info(c, 64, &x, &x, nullptr), PH_E_ARG);
    EXPECT(ph_follow_plan_info(c, 0, &x, &x, &x), PH_E_ARG);
    said("N=", __LINE__);
    EXPECT(ph_follow_plan_info(c, -7, &x, &x, &x), PH_E_ARG);
    no_launch(__LINE__);
  }

  // ---- sizes beyond 2^31, device form: the pointers are never dereferenced on the host
  {
    double tiny[2] = {0, 0};
    int32_t* ti = reinterpret_cast<int32_t*>(tiny);
    // W * ccap = 2^18 * 2^24 = 2^42 doubles, W * hop = 2^18 * 2^20 = 2^38 samples
    const int64_t W = (int64_t)1 << 18;
    EXPECT(ph_follow(c, tiny, PH_F32, (W - 1) * ((int64_t)1 << 20) + 1, 4096, 1 << 20, W, tiny, PH_F64, ti, ti, 64, 1 << 24,
                     PH_FLAG_DEVICE, tiny, tiny, ti), PH_OK);
    follow_launch(c, 4096, __LINE__);
    // hop at the top of int, W * hop beyond 2^31 many times over
    EXPECT(ph_follow(c, tiny, PH_F64, ((int64_t)1 << 58), 1000, INT32_MAX, (int64_t)1 << 26, nullptr, PH_F32, ti, ti, 1, 1,
                     PH_FLAG_DEVICE, tiny, tiny, ti), PH_OK);
    follow_launch(c, 1000, __LINE__);
    // byte counts that do not fit 64 bits are refused, not wrapped (nothing is allocated for them)
    EXPECT(ph_follow(c, tiny, PH_F64, INT64_MAX, 16, 8, 4, nullptr, PH_F64, ti, ti, 1, 1, PH_FLAG_DEVICE, tiny, tiny, ti), PH_E_ARG);
    said("64 bits", __LINE__);
    EXPECT(ph_follow(c, tiny, PH_F64, INT64_MAX / 8 + 1, 16, 8, 4, nullptr, PH_F64, ti, ti, 1, 1, PH_FLAG_DEVICE, tiny, tiny, ti),
           PH_E_ARG);
    said("64 bits", __LINE__);
    EXPECT(ph_follow(c, tiny, PH_F64, (int64_t)1 << 50, 16, 1, (int64_t)1 << 40, nullptr, PH_F64, ti, ti, 1, 1 << 24,
                     PH_FLAG_DEVICE, tiny, tiny, ti), PH_E_ARG);
    said("64 bits", __LINE__);
    EXPECT(ph_follow(c, tiny, PH_F64, INT64_MAX / 8, 16, 2, (int64_t)1 << 57, nullptr, PH_F64, ti, ti, 64, 1, PH_FLAG_DEVICE, tiny,
                     tiny, ti), PH_E_ARG);
    said("64 bits", __LINE__);
    no_launch(__LINE__);
  }

  // ---- refused, not read
  {
    std::vector<double> s(40), win(16), seg(4 * 20), powers(4 * 3);
    std::vector<int32_t> periods(4 * 3, 2), counts(4, 3), done(4);
    for (unsigned dev : {0u, (unsigned)PH_FLAG_DEVICE}) {
#define FO(ctx, sig, idt, L, N, hop, W, fdt, per, cnt, pcap, ccap, sg, pw, dn) \
  ph_follow(ctx, sig, idt, L, N, hop, W, win.data(), fdt, per, cnt, pcap, ccap, dev, sg, pw, dn)
      EXPECT(FO(nullptr, s.data(), PH_F64, 40, 16, 8, 4, PH_F64, periods.data(), counts.data(), 3, 20, seg.data(), powers.data(),
                done.data()), PH_E_ARG);
      said("ctx", __LINE__);
      EXPECT(FO(c, nullptr, PH_F64, 40, 16, 8, 4, PH_F64, periods.data(), counts.data(), 3, 20, seg.data(), powers.data(),
                done.data()), PH_E_ARG);
      said("NULL", __LINE__);
      EXPECT(FO(c, s.data(), PH_F64, 40, 16, 8, 4, PH_F64, nullptr, counts.data(), 3, 20, seg.data(), powers.data(), done.data()),
             PH_E_ARG);
      EXPECT(FO(c, s.data(), PH_F64, 40, 16, 8, 4, PH_F64, periods.data(), nullptr, 3, 20, seg.data(), powers.data(), done.data()),
             PH_E_ARG);
      EXPECT(FO(c, s.data(), PH_F64, 40, 16, 8, 4, PH_F64, periods.data(), counts.data(), 3, 20, nullptr, powers.data(),
                done.data()), PH_E_ARG);
      EXPECT(FO(c, s.data(), PH_F64, 40, 16, 8, 4, PH_F64, periods.data(), counts.data(), 3, 20, seg.data(), nullptr, done.data()),
             PH_E_ARG);
      EXPECT(FO(c, s.data(), PH_F64, 40, 16, 8, 4, PH_F64, periods.data(), counts.data(), 3, 20, seg.data(), powers.data(),
                nullptr), PH_E_ARG);
      said("NULL", __LINE__);
      for (int bad : {2, -1, 99}) {
        EXPECT(FO(c, s.data(), bad, 40, 16, 8, 4, PH_F64, periods.data(), counts.data(), 3, 20, seg.data(), powers.data(),
                  done.data()), PH_E_ARG);
        said("dtype", __LINE__);
        EXPECT(FO(c, s.data(), PH_F64, 40, 16, 8, 4, bad, periods.data(), counts.data(), 3, 20, seg.data(), powers.data(),
                  done.data()), PH_E_ARG);
        said("dtype", __LINE__);
      }
      for (int64_t bad : {(int64_t)0, (int64_t)-1, INT64_MIN}) {
        EXPECT(FO(c, s.data(), PH_F64, bad, 16, 8, 4, PH_F64, periods.data(), counts.data(), 3, 20, seg.data(), powers.data(),
                  done.data()), PH_E_ARG);
        said(">= 1", __LINE__);
        EXPECT(FO(c, s.data(), PH_F64, 40, 16, 8, bad, PH_F64, periods.data(), counts.data(), 3, 20, seg.data(), powers.data(),
                  done.data()), PH_E_ARG);
        said(">= 1", __LINE__);
      }
      for (int bad : {0, -1, INT32_MIN}) {
        EXPECT(FO(c, s.data(), PH_F64, 40, bad, 8, 4, PH_F64, periods.data(), counts.data(), 3, 20, seg.data(), powers.data(),
                  done.data()), PH_E_ARG);
        said(">= 1", __LINE__);
        EXPECT(FO(c, s.data(), PH_F64, 40, 16, bad, 4, PH_F64, periods.data(), counts.data(), 3, 20, seg.data(), powers.data(),
                  done.data()), PH_E_ARG);
        said(">= 1", __LINE__);
        EXPECT(FO(c, s.data(), PH_F64, 40, 16, 8, 4, PH_F64, periods.data(), counts.data(), bad, 20, seg.data(), powers.data(),
                  done.data()), PH_E_ARG);
        said("pcap", __LINE__);
        EXPECT(FO(c, s.data(), PH_F64, 40, 16, 8, 4, PH_F64, periods.data(), counts.data(), 3, bad, seg.data(), powers.data(),
                  done.data()), PH_E_ARG);
        said("ccap", __LINE__);
      }
      // a frame that starts at or behind the end of the signal: (W - 1) * hop = 40 >= L
      EXPECT(FO(c, s.data(), PH_F64, 40, 16, 8, 6, PH_F64, periods.data(), counts.data(), 3, 20, seg.data(), powers.data(),
                done.data()), PH_E_ARG);
      said(">= L", __LINE__);
      EXPECT(FO(c, s.data(), PH_F64, 40, 16, INT32_MAX, 2, PH_F64, periods.data(), counts.data(), 3, 20, seg.data(), powers.data(),
                done.data()), PH_E_ARG);
      EXPECT(FO(c, s.data(), PH_F64, 40, 16, 8, INT64_MAX, PH_F64, periods.data(), counts.data(), 3, 20, seg.data(), powers.data(),
                done.data()), PH_E_ARG);
      EXPECT(FO(c, s.data(), PH_F64, 40, 16, 8, 4, PH_F64, periods.data(), counts.data(), 65, 20, seg.data(), powers.data(),
                done.data()), PH_E_ARG);
      said("pcap", __LINE__);
      EXPECT(FO(c, s.data(), PH_F64, 40, 16, 8, 4, PH_F64, periods.data(), counts.data(), 3, (1 << 24) + 1, seg.data(),
                powers.data(), done.data()), PH_E_ARG);
      said("ccap", __LINE__);
      EXPECT(FO(c, s.data(), PH_F64, 40, 16, 8, 4, PH_F64, periods.data(), counts.data(), 3, INT32_MAX, seg.data(), powers.data(),
                done.data()), PH_E_ARG);
      no_launch(__LINE__);
#undef FO
    }
    // the limits themselves: the last frame starts on the last sample; pcap = 64
    std::vector<int32_t> p64(5 * 64, 1), c5(5, 64), d5(5);
    std::vector<double> pw64(5 * 64);
    seg.assign(5 * 20, 0.0);
    s.assign(33, 0.0);
    EXPECT(ph_follow(c, s.data(), PH_F64, 33, 16, 8, 5, win.data(), PH_F64, p64.data(), c5.data(), 64, 20, 0, seg.data(),
                     pw64.data(), d5.data()), PH_OK);
    follow_launch(c, 16, __LINE__);
  }

  // ---- the profile name of every launch
  float ms[300];
  int cntp = 0;
  EXPECT(ph_profile_read(c, ms, 300, &cntp), PH_OK);
  check_profile(c, cntp);
  EXPECT(ph_sync(c), PH_OK);
  EXPECT(ph_destroy(c), PH_OK);
  return finish("follow");
}

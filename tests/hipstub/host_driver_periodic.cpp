// Drives ph_overlap_add_periodic through the HOST half of the library (hip_stub.cpp stands in for the runtime; kernels do
// not run, outputs are not looked at).  Built with -fsanitize=address,undefined by tests/test_host_sanitizers.py:
// every refusal, the limits of pcap and ccap, the host-pointer staging of seg, periods, counts, masks and both windows
// with exact-size vectors, NULL optional pointers, and the size arithmetic with T * L, T * W, W * ccap and W * pcap beyond
// 2^31 and at 2^63 (sizes only: those calls pass PH_FLAG_DEVICE, so nothing of that size is allocated or touched) must
// touch no byte out of bounds and overflow no integer; every accepted call is one launch of kFramesBlock threads without
// LDS, named k_overlap_add_periodic.
#include "driver_common.h"

int main() {
  ph_ctx* c = nullptr;
  EXPECT(ph_create(0, &c), PH_OK);
  EXPECT(ph_profile_enable(c, 1), PH_OK);
  stub_reset_launches();

  // ---- host-pointer staging: {L, N, hop, W, pcap, ccap, T}; exact-size vectors, so ASan sees any byte read or written
  // past them
  const int shapes[][7] = {{1000, 64, 16, 60, 3, 40, 2}, {997, 63, 3, 312, 1, 1, 1},  {50, 64, 7, 1, 2, 200, 5},
                           {8, 8, 1, 1, 1, 8, 1},        {1000, 64, 80, 13, 64, 999, 3}, {7, 1, 1, 7, 1, 1, 9},
                           {333, 65, 64, 6, 5, 17, 4},   {100, 16, 8, 12, 100, 3, 2}};
  for (const auto& sh : shapes) {
    const int L = sh[0], N = sh[1], hop = sh[2], W = sh[3], pcap = sh[4], ccap = sh[5], T = sh[6];
    std::vector<double> win(N, 0.5), out((size_t)T * L), seg((size_t)W * ccap, 1.0);
    std::vector<int32_t> cnt(W, pcap), per((size_t)W * pcap, 1);
    std::vector<uint64_t> masks((size_t)T * W, ~0ull);
    // NULL optional pointers
    EXPECT(ph_overlap_add_periodic(c, seg.data(), per.data(), cnt.data(), masks.data(), W, pcap, ccap, T, N, hop, L, nullptr,
                                   nullptr, 0, out.data()), PH_OK);
    one_launch("k_overlap_add_periodic", __LINE__);
    EXPECT(ph_overlap_add_periodic(c, seg.data(), per.data(), cnt.data(), masks.data(), W, pcap, ccap, T, N, hop, L, win.data(),
                                   win.data(), PH_FLAG_OLA_NORM, out.data()), PH_OK);
    one_launch("k_overlap_add_periodic", __LINE__);
    EXPECT(ph_overlap_add_periodic(c, seg.data(), per.data(), cnt.data(), masks.data(), W, pcap, ccap, T, N, hop, L, nullptr,
                                   win.data(), PH_FLAG_DEVICE | PH_FLAG_OLA_NORM, out.data()), PH_OK);
    one_launch("k_overlap_add_periodic", __LINE__);
  }

  // ---- sizes beyond 2^31 and at 2^63, device form: the pointers are never dereferenced on the host
  {
    double tiny[2] = {0, 0};
    const uint64_t* tm = reinterpret_cast<const uint64_t*>(tiny);
    const int32_t* ti = reinterpret_cast<const int32_t*>(tiny);
    const unsigned D = PH_FLAG_DEVICE;
    const int64_t W = (int64_t)1 << 21;
    const int N = 4096, hop = 512;
    const int64_t L = (W - 1) * hop + N;  // > 2^30: T * L > 2^31 from T = 3 on
    EXPECT(ph_overlap_add_periodic(c, tiny, ti, ti, tm, W, 8, 1 << 14, 9, N, hop, L, nullptr, nullptr, D, tiny), PH_OK);  // W * ccap = 2^35
    one_launch("k_overlap_add_periodic", __LINE__);
    EXPECT(ph_overlap_add_periodic(c, tiny, ti, ti, tm, W, 1 << 20, 1 << 24, 3, N, hop, L, nullptr, nullptr, D | PH_FLAG_OLA_NORM,
                                   tiny), PH_OK);  // both limits: W * pcap = 2^41, W * ccap = 2^45
    one_launch("k_overlap_add_periodic", __LINE__);
    // T * W beyond 2^31 with a small L
    EXPECT(ph_overlap_add_periodic(c, tiny, ti, ti, tm, 70000, 1, 8, 40000, 8, 1, 70007, nullptr, nullptr, D, tiny), PH_OK);
    one_launch("k_overlap_add_periodic", __LINE__);
    // f * hop beyond 2^31 as well: hop of 2^20 over 2^12 frames
    const int64_t W2 = 4096, L2 = (W2 - 1) * ((int64_t)1 << 20) + 1;
    EXPECT(ph_overlap_add_periodic(c, tiny, ti, ti, tm, W2, 1, 8, 2, 8, 1 << 20, L2, nullptr, nullptr, D, tiny), PH_OK);
    one_launch("k_overlap_add_periodic", __LINE__);
    // the largest N a frame can have
    EXPECT(ph_overlap_add_periodic(c, tiny, ti, ti, tm, 2, 3, 1 << 24, 2, INT32_MAX, INT32_MAX, (int64_t)1 << 32, nullptr, nullptr, D,
                                   tiny), PH_OK);
    one_launch("k_overlap_add_periodic", __LINE__);
    // byte counts that do not fit 64 bits are refused, not wrapped: T * L, T * W, W * ccap, W * pcap
    EXPECT(ph_overlap_add_periodic(c, tiny, ti, ti, tm, 4, 2, 16, 3, 16, 8, INT64_MAX / 16, nullptr, nullptr, D, tiny), PH_E_ARG);
    said("T * L", __LINE__);
    EXPECT(ph_overlap_add_periodic(c, tiny, ti, ti, tm, 4, 2, 16, INT64_MAX, 16, 8, 100, nullptr, nullptr, D, tiny), PH_E_ARG);
    EXPECT(ph_overlap_add_periodic(c, tiny, ti, ti, tm, (int64_t)1 << 40, 1, 1, (int64_t)1 << 21, 1, 1, (int64_t)1 << 40, nullptr,
                                   nullptr, D, tiny), PH_E_ARG);
    EXPECT(ph_overlap_add_periodic(c, tiny, ti, ti, tm, (int64_t)1 << 40, 1, 1 << 24, 1, 1, 1, (int64_t)1 << 40, nullptr, nullptr, D,
                                   tiny), PH_E_ARG);
    said("W * ccap", __LINE__);
    EXPECT(ph_overlap_add_periodic(c, tiny, ti, ti, tm, (int64_t)1 << 42, 1 << 20, 1, 1, 1, 1, (int64_t)1 << 42, nullptr, nullptr, D,
                                   tiny), PH_E_ARG);
    EXPECT(ph_overlap_add_periodic(c, tiny, ti, ti, tm, INT64_MAX, 1 << 20, 1 << 24, INT64_MAX, INT32_MAX, 1, INT64_MAX, nullptr,
                                   nullptr, D, tiny), PH_E_ARG);
    no_launch(__LINE__);
    // the largest counts that pass: T * L * 8 and W * ccap * 8 just inside 2^63
    EXPECT(ph_overlap_add_periodic(c, tiny, ti, ti, tm, 4, 2, 16, 8, 16, 8, INT64_MAX / 64, nullptr, nullptr, D, tiny), PH_OK);
    one_launch("k_overlap_add_periodic", __LINE__);
    EXPECT(ph_overlap_add_periodic(c, tiny, ti, ti, tm, ((int64_t)1 << 36) - 1, 1, 1 << 24, 1, 1, 1, (int64_t)1 << 36, nullptr, nullptr,
                                   D, tiny), PH_OK);
    one_launch("k_overlap_add_periodic", __LINE__);
  }

  // ---- refused, not read
  {
    std::vector<double> seg(4 * 16), out(3 * 100);
    std::vector<int32_t> per(4 * 2, 3), cnt(4, 2);
    std::vector<uint64_t> masks(3 * 4, 1);
    for (unsigned dev : {0u, (unsigned)PH_FLAG_DEVICE}) {
#define OP(ctx, sg, pr, cn, mm, W, pcap, ccap, T, N, hop, L, o) \
  ph_overlap_add_periodic(ctx, sg, pr, cn, mm, W, pcap, ccap, T, N, hop, L, nullptr, nullptr, dev, o)
      EXPECT(OP(nullptr, seg.data(), per.data(), cnt.data(), masks.data(), 4, 2, 16, 3, 16, 8, 100, out.data()), PH_E_ARG);
      said("ctx", __LINE__);
      EXPECT(OP(c, nullptr, per.data(), cnt.data(), masks.data(), 4, 2, 16, 3, 16, 8, 100, out.data()), PH_E_ARG);
      said("seg", __LINE__);
      EXPECT(OP(c, seg.data(), nullptr, cnt.data(), masks.data(), 4, 2, 16, 3, 16, 8, 100, out.data()), PH_E_ARG);
      EXPECT(OP(c, seg.data(), per.data(), nullptr, masks.data(), 4, 2, 16, 3, 16, 8, 100, out.data()), PH_E_ARG);
      EXPECT(OP(c, seg.data(), per.data(), cnt.data(), nullptr, 4, 2, 16, 3, 16, 8, 100, out.data()), PH_E_ARG);
      said("masks", __LINE__);
      EXPECT(OP(c, seg.data(), per.data(), cnt.data(), masks.data(), 4, 2, 16, 3, 16, 8, 100, nullptr), PH_E_ARG);
      EXPECT(OP(c, seg.data(), per.data(), cnt.data(), masks.data(), 0, 2, 16, 3, 16, 8, 100, out.data()), PH_E_ARG);
      EXPECT(OP(c, seg.data(), per.data(), cnt.data(), masks.data(), -4, 2, 16, 3, 16, 8, 100, out.data()), PH_E_ARG);
      EXPECT(OP(c, seg.data(), per.data(), cnt.data(), masks.data(), 4, 0, 16, 3, 16, 8, 100, out.data()), PH_E_ARG);
      said("pcap", __LINE__);
      EXPECT(OP(c, seg.data(), per.data(), cnt.data(), masks.data(), 4, (1 << 20) + 1, 16, 3, 16, 8, 100, out.data()), PH_E_ARG);
      said("pcap", __LINE__);
      EXPECT(OP(c, seg.data(), per.data(), cnt.data(), masks.data(), 4, INT32_MAX, 16, 3, 16, 8, 100, out.data()), PH_E_ARG);
      EXPECT(OP(c, seg.data(), per.data(), cnt.data(), masks.data(), 4, 2, 0, 3, 16, 8, 100, out.data()), PH_E_ARG);
      said("ccap", __LINE__);
      EXPECT(OP(c, seg.data(), per.data(), cnt.data(), masks.data(), 4, 2, (1 << 24) + 1, 3, 16, 8, 100, out.data()), PH_E_ARG);
      said("ccap", __LINE__);
      EXPECT(OP(c, seg.data(), per.data(), cnt.data(), masks.data(), 4, 2, INT32_MIN, 3, 16, 8, 100, out.data()), PH_E_ARG);
      EXPECT(OP(c, seg.data(), per.data(), cnt.data(), masks.data(), 4, 2, 16, 0, 16, 8, 100, out.data()), PH_E_ARG);
      said("T=0", __LINE__);
      EXPECT(OP(c, seg.data(), per.data(), cnt.data(), masks.data(), 4, 2, 16, -1, 16, 8, 100, out.data()), PH_E_ARG);
      EXPECT(OP(c, seg.data(), per.data(), cnt.data(), masks.data(), 4, 2, 16, 3, 0, 8, 100, out.data()), PH_E_ARG);
      EXPECT(OP(c, seg.data(), per.data(), cnt.data(), masks.data(), 4, 2, 16, 3, 16, 0, 100, out.data()), PH_E_ARG);
      EXPECT(OP(c, seg.data(), per.data(), cnt.data(), masks.data(), 4, 2, 16, 3, 16, -3, 100, out.data()), PH_E_ARG);
      EXPECT(OP(c, seg.data(), per.data(), cnt.data(), masks.data(), 4, 2, 16, 3, 16, 8, 0, out.data()), PH_E_ARG);
      EXPECT(OP(c, seg.data(), per.data(), cnt.data(), masks.data(), 4, 2, 16, 3, 16, 8, 24, out.data()), PH_E_ARG);  // (W - 1) hop == L
      said("behind", __LINE__);
#undef OP
      no_launch(__LINE__);
    }
    // the last admissible length has frame W - 1 start on the last sample
    EXPECT(ph_overlap_add_periodic(c, seg.data(), per.data(), cnt.data(), masks.data(), 4, 2, 16, 3, 16, 8, 25, nullptr, nullptr, 0,
                                   out.data()), PH_OK);
    one_launch("k_overlap_add_periodic", __LINE__);
  }

  // ---- the profile name of every launch (the profile keeps the first 256)
  float ms[300];
  int cntp = 0;
  EXPECT(ph_profile_read(c, ms, 300, &cntp), PH_OK);
  check_profile(c, cntp);
  EXPECT(ph_sync(c), PH_OK);
  EXPECT(ph_destroy(c), PH_OK);
  return finish("periodic");
}

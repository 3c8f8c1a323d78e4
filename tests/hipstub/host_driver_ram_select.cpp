// Drives ph_ramanujan_select through the HOST half of the library (hip_stub.cpp stands in for the runtime; kernels do not
// run, outputs are not looked at).  Built with -fsanitize=address,undefined by tests/test_host_sanitizers.py:
// argument validation, the staging of the norms and the optional reference levels and of the three int32 outputs must
// touch no byte out of bounds -- at pcap = 2^20 too, and the size arithmetic with W * (q_hi + 1) * 8 beyond 2^31 --,
// every refusal comes before a launch, and an accepted call launches k_ram_select_ref once: one wavefront per row, no
// LDS.
#include <cmath>
#include <cstdint>

#include "driver_common.h"

// one launch of 64 threads without LDS since the last reset
static void one_wave_launch(int line) {
  int block[4];
  long long l[4];
  const int n = stub_launches(block, l, 4);
  if (n != 1 || block[0] != 64 || l[0] != 0) {
    std::printf("FAIL line %d: %d launches, block %d, lds %lld\n", line, n, n ? block[0] : -1, n ? l[0] : -1LL);
    ++fails;
  }
  launched("k_ram_select_ref");
  stub_reset_launches();
}

int main() {
  ph_ctx* c = nullptr;
  EXPECT(ph_create(0, &c), PH_OK);
  EXPECT(ph_profile_enable(c, 1), PH_OK);
  // {W, q_hi, pcap}: the smallest call, rows at and around one and two wavefronts, the record format's limit, pcap = 2^20
  const int sizes[][3] = {{1, 1, 1}, {3, 63, 2}, {5, 64, 7}, {32, 128, 64}, {2, 200, 300}, {2, 30029, 64}, {3, 7, 1 << 20}};
  for (const auto& sz : sizes) {
    const int W = sz[0], q_hi = sz[1], pcap = sz[2];
    std::vector<double> norms((size_t)W * (q_hi + 1), 0.5), ref(W, 1.0);
    std::vector<int32_t> per((size_t)W * pcap), cnt(W), over(W);
    for (unsigned dev : {0u, (unsigned)PH_FLAG_DEVICE}) {
      for (const double* r : {(const double*)nullptr, (const double*)ref.data()}) {
        stub_reset_launches();
        EXPECT(ph_ramanujan_select(c, norms.data(), W, q_hi, 0.2, r, pcap, dev, per.data(), cnt.data(), over.data()), PH_OK);
        one_wave_launch(__LINE__);
      }
      // refused, not read and not launched
#define SEL(ctx, nn, ww, qq, tt, pc, pp, cc, oo) ph_ramanujan_select(ctx, nn, ww, qq, tt, ref.data(), pc, dev, pp, cc, oo)
      EXPECT(SEL(nullptr, norms.data(), W, q_hi, 0.2, pcap, per.data(), cnt.data(), over.data()), PH_E_ARG);
      said("ctx", __LINE__);
      EXPECT(SEL(c, nullptr, W, q_hi, 0.2, pcap, per.data(), cnt.data(), over.data()), PH_E_ARG);
      said("norms", __LINE__);
      EXPECT(SEL(c, norms.data(), W, q_hi, 0.2, pcap, nullptr, cnt.data(), over.data()), PH_E_ARG);
      EXPECT(SEL(c, norms.data(), W, q_hi, 0.2, pcap, per.data(), nullptr, over.data()), PH_E_ARG);
      EXPECT(SEL(c, norms.data(), W, q_hi, 0.2, pcap, per.data(), cnt.data(), nullptr), PH_E_ARG);
      said("NULL", __LINE__);
      EXPECT(SEL(c, norms.data(), 0, q_hi, 0.2, pcap, per.data(), cnt.data(), over.data()), PH_E_ARG);
      EXPECT(SEL(c, norms.data(), -1, q_hi, 0.2, pcap, per.data(), cnt.data(), over.data()), PH_E_ARG);
      EXPECT(SEL(c, norms.data(), (int64_t)1 << 40, q_hi, 0.2, pcap, per.data(), cnt.data(), over.data()), PH_E_ARG);
      EXPECT(SEL(c, norms.data(), INT64_MAX, q_hi, 0.2, pcap, per.data(), cnt.data(), over.data()), PH_E_ARG);
      said("W=", __LINE__);
      EXPECT(SEL(c, norms.data(), W, 0, 0.2, pcap, per.data(), cnt.data(), over.data()), PH_E_ARG);
      EXPECT(SEL(c, norms.data(), W, -1, 0.2, pcap, per.data(), cnt.data(), over.data()), PH_E_ARG);
      EXPECT(SEL(c, norms.data(), W, 30030, 0.2, pcap, per.data(), cnt.data(), over.data()), PH_E_ARG);
      EXPECT(SEL(c, norms.data(), W, 0x7fffffff, 0.2, pcap, per.data(), cnt.data(), over.data()), PH_E_ARG);
      said("q_hi", __LINE__);
      EXPECT(SEL(c, norms.data(), W, q_hi, 0.2, 0, per.data(), cnt.data(), over.data()), PH_E_ARG);
      EXPECT(SEL(c, norms.data(), W, q_hi, 0.2, -1, per.data(), cnt.data(), over.data()), PH_E_ARG);
      EXPECT(SEL(c, norms.data(), W, q_hi, 0.2, (1 << 20) + 1, per.data(), cnt.data(), over.data()), PH_E_ARG);
      said("pcap", __LINE__);
      EXPECT(SEL(c, norms.data(), W, q_hi, 0.0, pcap, per.data(), cnt.data(), over.data()), PH_E_ARG);
      EXPECT(SEL(c, norms.data(), W, q_hi, -0.2, pcap, per.data(), cnt.data(), over.data()), PH_E_ARG);
      EXPECT(SEL(c, norms.data(), W, q_hi, std::nan(""), pcap, per.data(), cnt.data(), over.data()), PH_E_ARG);
      said("thresh", __LINE__);
#undef SEL
      no_launch(__LINE__);
    }
  }
  {
    // ---- W * (q_hi + 1) * 8 beyond 2^31 (and W * pcap * 4 beyond 2^40), device form: sizes only, the pointers are
    // never dereferenced on the host and nothing of that size is allocated
    const int64_t W = 9000;
    const int q_hi = 30029;
    static_assert(W * (q_hi + 1) * 8 > (1LL << 31), "the case this is about");
    std::vector<double> norms(16);
    std::vector<int32_t> out(16);
    for (const int64_t w : {W, (int64_t)0x7fffffffLL / 64}) {
      for (const int pcap : {3, 1 << 20}) {
        stub_reset_launches();
        EXPECT(ph_ramanujan_select(c, norms.data(), w, q_hi, 0.2, norms.data(), pcap, PH_FLAG_DEVICE, out.data(), out.data(),
                                   out.data()), PH_OK);
        one_wave_launch(__LINE__);
      }
    }
  }
  float ms[300];
  int cntp = 0;
  EXPECT(ph_profile_read(c, ms, 300, &cntp), PH_OK);
  check_profile(c, cntp);
  EXPECT(ph_sync(c), PH_OK);
  EXPECT(ph_destroy(c), PH_OK);
  return finish("ram_select");
}

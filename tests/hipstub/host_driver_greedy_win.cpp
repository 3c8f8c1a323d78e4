// Drives ph_qo_greedy_win through the HOST half of the library (hip_stub.cpp stands in for the runtime; kernels do not
// run, outputs are not looked at).  Built with -fsanitize=address,undefined by tests/test_host_sanitizers.py:
// argument validation, the staging of the analysis window beside the batch, the divisor tables and the LDS layout must
// touch no byte out of bounds, and the one launch must ask for the LDS that ph_qo_plan_info(PH_FLAG_KEEP_WEIGHTS) names.
#include <cmath>

#include "driver_common.h"

int main() {
  ph_ctx* c = nullptr;
  EXPECT(ph_create(0, &c), PH_OK);
  EXPECT(ph_profile_enable(c, 1), PH_OK);
  const int sizes[][2] = {{1, 7}, {3, 100}, {5, 1000}, {2, 4096}, {1, 20000}, {1, 50000}};
  for (const auto& sz : sizes) {
    const int W = sz[0], N = sz[1], num = 5;
    std::vector<double> x((size_t)W * N), win((size_t)N);
    for (size_t i = 0; i < x.size(); ++i) x[i] = std::sin(0.37 * (double)i) + 0.01 * (double)(i % 7);
    for (int i = 0; i < N; ++i) win[i] = 0.5 - 0.5 * std::cos(6.283185307179586 * i / (N > 1 ? N - 1 : 1));
    std::vector<float> xf(x.begin(), x.end());
    const int p_hi = N / 3 > 2 ? N / 3 : 2;
    for (int dtype : {PH_F64, PH_F32}) {
      const void* px = dtype == PH_F64 ? (const void*)x.data() : (const void*)xf.data();
      const size_t es = dtype == PH_F64 ? 8 : 4;
      std::vector<uint32_t> per((size_t)W * num);
      std::vector<double> nr((size_t)W * num);
      std::vector<int32_t> kp((size_t)W * num), cnt((size_t)2 * W), st(W);
      std::vector<char> resid((size_t)W * N * es);
      for (unsigned dev : {0u, (unsigned)PH_FLAG_DEVICE}) {
        for (unsigned fl : {0u, (unsigned)PH_FLAG_TRUNC, (unsigned)PH_FLAG_KEEP_WEIGHTS, (unsigned)(PH_FLAG_TRUNC | PH_FLAG_KEEP_WEIGHTS)}) {
          for (int kcap : {1, 64, 4096, 1 << 20}) {
            if ((size_t)W * kcap > ((size_t)1 << 22)) continue;
            std::vector<double> w((size_t)W * kcap);
            int lds = 0, where = 0;
            EXPECT(ph_qo_plan_info(c, dtype, N, p_hi, kcap, fl | PH_FLAG_KEEP_WEIGHTS, &lds, &where), PH_OK);
            stub_reset_launches();
            EXPECT(ph_qo_greedy_win(c, px, dtype, W, N, win.data(), num, 0.1, 2, p_hi, kcap, fl | dev, per.data(), nr.data(),
                                    kp.data(), cnt.data(), w.data(), resid.data(), st.data()), PH_OK);
            int block[4];
            long long l[4];
            const int n = stub_launches(block, l, 4);
            if (n != 1 || l[0] != lds) {
              std::printf("FAIL N %d dtype %d flags %u kcap %d: %d launches, lds %lld, plan %d (placement %d)\n", N, dtype, fl | dev,
                          kcap, n, n ? l[0] : -1LL, lds, where);
              ++fails;
            }
          }
          // max_length < 0 is N / 3
          std::vector<double> w((size_t)W * 64);
          EXPECT(ph_qo_greedy_win(c, px, dtype, W, N, win.data(), num, 0.1, 1, -1, 64, fl | dev, per.data(), nr.data(), kp.data(),
                                  cnt.data(), w.data(), resid.data(), st.data()), N >= 3 ? PH_OK : PH_E_ARG);
        }
        // refused, not read
        std::vector<double> w((size_t)W * 64);
#define GREEDY(ctx, xx, dt, ww, nn, wn, nm, lo, hi, kc, flg, out0, stat)                                                       \
  ph_qo_greedy_win(ctx, xx, dt, ww, nn, wn, nm, 0.1, lo, hi, kc, flg, out0, nr.data(), kp.data(), cnt.data(), w.data(), \
                   resid.data(), stat)
        EXPECT(GREEDY(nullptr, px, dtype, W, N, win.data(), num, 2, p_hi, 64, dev, per.data(), st.data()), PH_E_ARG);
        EXPECT(GREEDY(c, nullptr, dtype, W, N, win.data(), num, 2, p_hi, 64, dev, per.data(), st.data()), PH_E_ARG);
        EXPECT(GREEDY(c, px, dtype, W, N, nullptr, num, 2, p_hi, 64, dev, per.data(), st.data()), PH_E_ARG);
        EXPECT(GREEDY(c, px, 7, W, N, win.data(), num, 2, p_hi, 64, dev, per.data(), st.data()), PH_E_ARG);
        EXPECT(GREEDY(c, px, dtype, 0, N, win.data(), num, 2, p_hi, 64, dev, per.data(), st.data()), PH_E_ARG);
        EXPECT(GREEDY(c, px, dtype, W, 0, win.data(), num, 2, p_hi, 64, dev, per.data(), st.data()), PH_E_ARG);
        EXPECT(GREEDY(c, px, dtype, W, N, win.data(), 0, 2, p_hi, 64, dev, per.data(), st.data()), PH_E_ARG);
        EXPECT(GREEDY(c, px, dtype, W, N, win.data(), num, 0, p_hi, 64, dev, per.data(), st.data()), PH_E_ARG);
        EXPECT(GREEDY(c, px, dtype, W, N, win.data(), num, p_hi + 1, p_hi, 64, dev, per.data(), st.data()), PH_E_ARG);
        EXPECT(GREEDY(c, px, dtype, W, N, win.data(), num, 2, p_hi, 0, dev, per.data(), st.data()), PH_E_ARG);
        EXPECT(GREEDY(c, px, dtype, W, N, win.data(), num, 2, p_hi, (1 << 20) + 1, dev, per.data(), st.data()), PH_E_ARG);
        EXPECT(GREEDY(c, px, dtype, W, N, win.data(), num, 2, p_hi, 64, dev, nullptr, st.data()), PH_E_ARG);
        EXPECT(GREEDY(c, px, dtype, W, N, win.data(), num, 2, p_hi, 64, dev, per.data(), nullptr), PH_E_ARG);
        EXPECT(GREEDY(c, px, dtype, W, N, win.data(), num, 2, p_hi, 64, dev | PH_FLAG_ORTH, per.data(), st.data()), PH_E_UNSUPPORTED);
#undef GREEDY
      }
    }
  }
  // the profile name of the launch
  float ms[300];
  int cntp = 0;
  EXPECT(ph_profile_read(c, ms, 300, &cntp), PH_OK);
  check_profile(c, cntp, "k_qo_greedy_win");
  EXPECT(ph_sync(c), PH_OK);
  EXPECT(ph_destroy(c), PH_OK);
  return finish("greedy_win");
}

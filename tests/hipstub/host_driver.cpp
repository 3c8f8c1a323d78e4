// Drives every entry point of include/periodhip.h through the HOST half of the library (hip_stub.cpp stands in for
// the runtime; kernels do not run, outputs are not looked at).  Built with -fsanitize=address,undefined by
// tests/test_host_sanitizers.py: what is checked is that argument validation, pass plans, geometry / CSR / Bluestein
// tables, staging copies and LDS layout arithmetic touch no byte out of bounds and hit no undefined behaviour.
#include <cmath>

#include "driver_common.h"

struct Csr {
  std::vector<int32_t> off, q;
};

// proper divisors d of p with 1 < d < p (any fixed order will do here)
static Csr factor_tables(int max_p) {
  Csr t;
  t.off.assign(max_p + 2, 0);
  for (int p = 0; p <= max_p; ++p) {
    t.off[p] = (int32_t)t.q.size();
    for (int d = 2; p > 0 && d < p; ++d)
      if (p % d == 0) t.q.push_back(d);
  }
  t.off[max_p + 1] = (int32_t)t.q.size();
  if (t.q.empty()) t.q.push_back(1);
  return t;
}

// sub-periods p / f for the prime proper divisors f of p (Periods.py:209-214)
static Csr orth_tables(int max_p) {
  Csr t;
  t.off.assign(max_p + 2, 0);
  for (int p = 0; p <= max_p; ++p) {
    t.off[p] = (int32_t)t.q.size();
    for (int f = 2; p > 0 && f < p; ++f) {
      bool prime = true;
      for (int d = 2; d * d <= f; ++d) prime &= (f % d != 0);
      if (prime && p % f == 0) t.q.push_back(p / f);
    }
  }
  t.off[max_p + 1] = (int32_t)t.q.size();
  if (t.q.empty()) t.q.push_back(1);
  return t;
}

// ph_plan_info for `op`, then the entry point itself (run): the launches the stub records must be the plan's kernels,
// with the plan's block size and dynamic LDS.
template <typename F>
static void expect_plan(ph_ctx* c, int op, int dtype, int N, std::vector<int32_t> prm, unsigned fl, int line, F run) {
  int32_t rec[PH_PLAN_LEN];
  const int rc = ph_plan_info(c, op, dtype, N, prm.data(), (int)prm.size(), fl, rec);
  if (rc != PH_OK) {
    std::printf("FAIL line %d: ph_plan_info(op %d, N %d) -> %d (%s)\n", line, op, N, rc, ph_last_error());
    ++fails;
    return;
  }
  stub_reset_launches();
  const int rr = run();
  int block[16];
  long long lds[16];
  const int n = stub_launches(block, lds, 16);
  bool ok = rr == PH_OK && n == rec[PH_PLAN_KERNELS];
  for (int k = 0; ok && k < n; ++k) {
    const int32_t* r = rec + PH_PLAN_K0 + k * PH_PLAN_STRIDE;
    ok = block[k] == r[PH_PLAN_BLOCK] && lds[k] == r[PH_PLAN_LDS_BYTES];
  }
  if (!ok) {
    std::printf("FAIL line %d: op %d dtype %d N %d flags %u: run -> %d, %d launches, plan %d kernels", line, op, dtype, N, fl,
                rr, n, rec[PH_PLAN_KERNELS]);
    for (int k = 0; k < n && k < 2; ++k)
      std::printf(" | launch %d: block %d lds %lld, plan block %d lds %d", k, block[k], lds[k],
                  rec[PH_PLAN_K0 + k * PH_PLAN_STRIDE + PH_PLAN_BLOCK], rec[PH_PLAN_K0 + k * PH_PLAN_STRIDE + PH_PLAN_LDS_BYTES]);
    std::printf("\n");
    ++fails;
  }
}

static void plan_checks(ph_ctx* c) {
  int32_t rec[PH_PLAN_LEN];
  const int32_t prm[4] = {2, 300, 0, 0};
  // bad arguments
  EXPECT(ph_plan_info(c, 99, PH_F64, 4096, nullptr, 0, 0, rec), PH_E_ARG);
  EXPECT(ph_plan_info(c, PH_OP_SWEEP, 7, 4096, nullptr, 0, 0, rec), PH_E_ARG);
  EXPECT(ph_plan_info(c, PH_OP_SWEEP, PH_F64, 0, nullptr, 0, 0, rec), PH_E_ARG);
  EXPECT(ph_plan_info(c, PH_OP_SWEEP, PH_F64, 4096, nullptr, 2, 0, rec), PH_E_ARG);
  EXPECT(ph_plan_info(c, PH_OP_SWEEP, PH_F64, 4096, prm, -1, 0, rec), PH_E_ARG);
  EXPECT(ph_plan_info(c, PH_OP_SWEEP, PH_F64, 4096, prm, 2, 0, nullptr), PH_E_ARG);
  EXPECT(ph_plan_info(nullptr, PH_OP_SWEEP, PH_F64, 4096, prm, 2, 0, rec), PH_E_ARG);
  const int32_t bad_sweep[3] = {5, 4, 0}, bad_mode[3] = {2, 40, 3}, bad_num[3] = {0, 2, 40}, bad_len[3] = {5, 9, 3};
  EXPECT(ph_plan_info(c, PH_OP_SWEEP, PH_F64, 4096, bad_sweep, 3, 0, rec), PH_E_ARG);
  EXPECT(ph_plan_info(c, PH_OP_SWEEP, PH_F64, 4096, bad_mode, 3, 0, rec), PH_E_ARG);
  EXPECT(ph_plan_info(c, PH_OP_M_BEST, PH_F64, 4096, bad_num, 3, 0, rec), PH_E_ARG);
  EXPECT(ph_plan_info(c, PH_OP_M_BEST, PH_F64, 4096, bad_len, 3, 0, rec), PH_E_ARG);
  const int32_t ram_wide[2] = {2, 20000}, ram_format[2] = {2, 30030}, orth_small[1] = {1}, bf_bad[1] = {1};
  EXPECT(ph_plan_info(c, PH_OP_RAMANUJAN, PH_F64, 60000, ram_wide, 2, 0, rec), PH_E_ARG);  // one wave's strips > LDS
  EXPECT(ph_plan_info(c, PH_OP_RAMANUJAN, PH_F64, 100000, ram_format, 2, 0, rec), PH_E_ARG);
  EXPECT(ph_plan_info(c, PH_OP_ORTH_POWERS, PH_F64, 4096, orth_small, 1, 0, rec), PH_E_ARG);
  EXPECT(ph_plan_info(c, PH_OP_BEST_FREQUENCY, PH_F64, 1, bf_bad, 1, 0, rec), PH_E_ARG);
  {
    std::vector<double> x(60000, 0.5), out((size_t)20001);
    EXPECT(ph_ramanujan_norms(c, x.data(), PH_F64, 1, 60000, 2, 20000, 0, out.data()), PH_E_ARG);
  }
  // both sides of the pair, step-1 block, small_means, second-buffer, window and FFT / chirp switches
  const int max_len = 300;
  const Csr fac = factor_tables(max_len), orth = orth_tables(2 * 8192);
  for (int N : {1000, 3071, 3072, 5400, 6500, 9400, 9800, 10100, 19400, 20200, 21000, 40500, 41000}) {
    std::vector<double> x((size_t)N);
    for (int i = 0; i < N; ++i) x[i] = std::sin(0.37 * i) + 0.25 * std::sin(0.05 * i);
    std::vector<float> xf(x.begin(), x.end());
    for (int dtype : {PH_F64, PH_F32}) {
      const void* px = dtype == PH_F64 ? (const void*)x.data() : (const void*)xf.data();
      for (unsigned fl : {0u, (unsigned)PH_FLAG_TRUNC}) {
        const int num = 3;
        std::vector<uint32_t> per(num);
        std::vector<double> pw(num), bases((size_t)num * N), sw(max_len + 1), proj((size_t)2 * N);
        std::vector<int32_t> st(1), cnt(1), ip(16);
        std::vector<int32_t> pl = {7, max_len};
        expect_plan(c, PH_OP_PROJECT, dtype, N, {max_len}, fl, __LINE__, [&] {
          return ph_project_batch(c, px, dtype, 1, N, pl.data(), 2, nullptr, nullptr, 0, fl, proj.data());
        });
        expect_plan(c, PH_OP_SWEEP, dtype, N, {2, max_len, PH_SWEEP_NORM}, fl, __LINE__, [&] {
          return ph_sweep(c, px, dtype, 1, N, 2, max_len, PH_SWEEP_NORM, nullptr, nullptr, 0, fl, sw.data());
        });
        expect_plan(c, PH_OP_M_BEST, dtype, N, {num, 2, max_len}, fl, __LINE__, [&] {
          return ph_m_best(c, px, dtype, 1, N, num, 2, max_len, 0, nullptr, nullptr, fac.off.data(), fac.q.data(), max_len, fl,
                           per.data(), pw.data(), bases.data(), st.data(), nullptr);
        });
        std::vector<double> sb((size_t)16 * N), spw(16);
        expect_plan(c, PH_OP_SMALL_TO_LARGE, dtype, N, {max_len}, fl, __LINE__, [&] {
          return ph_small_to_large(c, px, dtype, 1, N, 0.05, max_len, nullptr, nullptr, 0, fl, 16, cnt.data(), ip.data(),
                                   spw.data(), sb.data(), st.data());
        });
        expect_plan(c, PH_OP_BEST_CORRELATION, dtype, N, {max_len}, fl, __LINE__, [&] {
          return ph_best_correlation(c, px, dtype, 1, N, num, max_len, 0.01, nullptr, nullptr, 0, fl, per.data(), pw.data(),
                                     bases.data(), st.data());
        });
        for (int win : {256, 300, 4096, 5400, 5500, 8192, 16384}) {
          std::vector<uint32_t> bp(1);
          std::vector<double> bpw(1), bb((size_t)N);
          expect_plan(c, PH_OP_BEST_FREQUENCY, dtype, N, {win}, fl, __LINE__, [&] {
            return ph_best_frequency(c, px, dtype, 1, N, win, 1, orth.off.data(), orth.q.data(), 2 * 8192, fl, bp.data(),
                                     bpw.data(), bb.data(), st.data());
          });
        }
        if (fl) continue;  // the remaining ops take no flags
        for (int qh : {64, 128, 512, N / 3}) {
          if (12 * (size_t)qh + 32 > 160 * 1024) continue;  // one wave's strips exceed the LDS: refused above
          std::vector<double> rn((size_t)qh + 1);
          expect_plan(c, PH_OP_RAMANUJAN, dtype, N, {2, qh}, 0, __LINE__, [&] {
            return ph_ramanujan_norms(c, px, dtype, 1, N, 2, qh, 0, rn.data());
          });
        }
        std::vector<double> op((size_t)max_len);
        expect_plan(c, PH_OP_ORTH_POWERS, dtype, N, {max_len}, 0, __LINE__, [&] {
          return ph_orth_powers(c, px, dtype, 1, N, max_len, 0, 0, nullptr, nullptr, op.data());
        });
        std::vector<int32_t> fp = {3, 8}, fk = {3, 7};
        std::vector<double> fs(10);
        expect_plan(c, PH_OP_FOLD_SUMS, dtype, N, {}, 0, __LINE__, [&] {
          return ph_fold_sums(c, px, dtype, 1, N, fp.data(), fk.data(), 2, 0, fs.data());
        });
      }
    }
  }
}

static void expect_eq(long long got, long long want, const char* what, int line) {
  if (got != want) {
    std::printf("FAIL line %d: %s is %lld, want %lld\n", line, what, got, want);
    ++fails;
  }
}

// A context created under PH_HBM_WINDOW=1 keeps every window in HBM, so its m_best runs the one-window step 1 where a
// default context runs the window pair: the plan record, the ph_m_best_*_info queries and the launch all have to say so.
// The screen of that kernel is the one a context under PH_STEP1_PAIR=0 reports.
static void hbm_window_checks() {
  ph_ctx *hbm = nullptr, *one = nullptr;
  setenv("PH_HBM_WINDOW", "1", 1);
  EXPECT(ph_create(0, &hbm), PH_OK);
  unsetenv("PH_HBM_WINDOW");
  setenv("PH_STEP1_PAIR", "0", 1);
  EXPECT(ph_create(0, &one), PH_OK);
  unsetenv("PH_STEP1_PAIR");
  const int N = 4096, num = 10, max_len = N / 3;
  int32_t rec[PH_PLAN_LEN];
  const int32_t prm[3] = {num, 2, -1};
  EXPECT(ph_plan_info(hbm, PH_OP_M_BEST, PH_F64, N, prm, 3, 0, rec), PH_OK);
  expect_eq(rec[PH_PLAN_K0 + PH_PLAN_VARIANT], PH_PLAN_ONE, "step-1 variant under PH_HBM_WINDOW", __LINE__);
  expect_eq(rec[PH_PLAN_K0 + PH_PLAN_WINDOW], PH_PLAN_HBM, "step-1 window under PH_HBM_WINDOW", __LINE__);
  int wpw = 0, bps = 0;
  EXPECT(ph_m_best_info(hbm, PH_F64, N, num, 2, -1, 0, &wpw, &bps), PH_OK);
  expect_eq(wpw, 1, "windows per workgroup under PH_HBM_WINDOW", __LINE__);
  expect_eq(bps, 8, "LDS bytes per sample under PH_HBM_WINDOW", __LINE__);
  for (int gamma : {0, 1}) {
    int ent[2] = {0, 0}, scr[2] = {0, 0};
    long long el[2] = {0, 0};
    EXPECT(ph_m_best_screen_info(hbm, PH_F64, N, num, 2, -1, 0, gamma, &ent[0], &scr[0], &el[0]), PH_OK);
    EXPECT(ph_m_best_screen_info(one, PH_F64, N, num, 2, -1, 0, gamma, &ent[1], &scr[1], &el[1]), PH_OK);
    expect_eq(ent[0], ent[1], "screen entries under PH_HBM_WINDOW", __LINE__);
    expect_eq(scr[0], scr[1], "screened periods under PH_HBM_WINDOW", __LINE__);
    expect_eq(el[0], el[1], "screen LDS elements under PH_HBM_WINDOW", __LINE__);
    expect_eq(scr[0], max_len - 1, "screened periods of the one-window kernel", __LINE__);
  }
  int np[2] = {0, 0}, nq[2] = {0, 0};
  EXPECT(ph_m_best_plan_info(hbm, PH_F64, N, num, 2, -1, 0, &np[0], &nq[0]), PH_OK);
  EXPECT(ph_m_best_plan_info(one, PH_F64, N, num, 2, -1, 0, &np[1], &nq[1]), PH_OK);
  expect_eq(np[0], np[1], "plan passes under PH_HBM_WINDOW", __LINE__);
  const Csr fac = factor_tables(max_len);
  std::vector<double> x((size_t)N), pw(num), bases((size_t)num * N);
  for (int i = 0; i < N; ++i) x[i] = std::sin(0.37 * i) + 0.25 * std::sin(0.05 * i);
  std::vector<uint32_t> per(num);
  std::vector<int32_t> st(1);
  expect_plan(hbm, PH_OP_M_BEST, PH_F64, N, {num, 2, -1}, 0, __LINE__, [&] {
    return ph_m_best(hbm, x.data(), PH_F64, 1, N, num, 2, -1, 0, nullptr, nullptr, fac.off.data(), fac.q.data(), max_len, 0,
                     per.data(), pw.data(), bases.data(), st.data(), nullptr);
  });
  // the query refuses the lengths its siblings and the launch refuse, and says which
  EXPECT(ph_m_best_info(one, PH_F64, N, num, 5, 4, 0, &wpw, &bps), PH_E_ARG);
  said("min_length", __LINE__);
  said("max_length", __LINE__);
  said("5, 4", __LINE__);
  EXPECT(ph_m_best_info(one, PH_F64, N, num, 0, 4, 0, &wpw, &bps), PH_E_ARG);
  EXPECT(ph_destroy(hbm), PH_OK);
  EXPECT(ph_destroy(one), PH_OK);
}

int main() {
  ph_ctx* c = nullptr;
  int n = 0;
  EXPECT(ph_device_count(&n), PH_OK);
  EXPECT(ph_create(0, &c), PH_OK);
  EXPECT(ph_create(0, nullptr), PH_E_ARG);
  int cu = 0, lds = 0, a = 0, b = 0;
  EXPECT(ph_device_info(c, &cu, &lds), PH_OK);
  EXPECT(ph_max_window(c, PH_F64, 0, &a), PH_OK);
  EXPECT(ph_max_window(c, PH_F32, PH_FLAG_TRUNC | PH_FLAG_ORTH, &a), PH_OK);
  for (int lo : {1, 2, 63, 64, 65, 700}) {
    for (int hi : {lo, lo + 1, 3 * lo + 77, 5000}) EXPECT(ph_sweep_plan_info(c, lo, hi, &a, &b), PH_OK);
  }
  EXPECT(ph_sweep_plan_info(c, 0, 5, &a, &b), PH_E_ARG);
  EXPECT(ph_m_best_info(c, PH_F64, 4096, 10, 2, -1, 0, &a, &b), PH_OK);
  EXPECT(ph_m_best_info(c, PH_F32, 4096, 10, 2, 1365, PH_FLAG_TRUNC, &a, &b), PH_OK);
  EXPECT(ph_m_best_plan_info(c, PH_F64, 4096, 10, 2, -1, 0, &a, &b), PH_OK);
  EXPECT(ph_m_best_plan_info(c, PH_F64, 4096, 10, 9, 3, 0, &a, &b), PH_E_ARG);
  EXPECT(ph_profile_enable(c, 1), PH_OK);

  const int sizes[][2] = {{1, 7}, {3, 100}, {5, 1000}, {2, 4096}, {1, 9000}, {1, 20000}};
  for (const auto& sz : sizes) {
    const int W = sz[0], N = sz[1];
    std::vector<double> x((size_t)W * N);
    for (size_t i = 0; i < x.size(); ++i) x[i] = std::sin(0.37 * (double)i) + 0.01 * (double)(i % 7);
    std::vector<float> xf(x.begin(), x.end());
    const int maxp = N;  // tables up to N
    const Csr fac = factor_tables(maxp), orth = orth_tables(maxp);
    for (int dtype : {PH_F64, PH_F32}) {
      const void* px = dtype == PH_F64 ? (const void*)x.data() : (const void*)xf.data();
      const size_t es = dtype == PH_F64 ? 8 : 4;
      for (unsigned dev : {0u, (unsigned)PH_FLAG_DEVICE}) {
        std::vector<double> out((size_t)W * 8 * N + 16);
        std::vector<int32_t> pl = {1, 2, 3, N / 2 > 0 ? N / 2 : 1, N, N + 3, 64, 65};
        EXPECT(ph_periodic_norm(c, px, dtype, W, N, 0, dev, out.data()), PH_OK);
        EXPECT(ph_periodic_norm(c, px, dtype, W, N, 5, dev, out.data()), PH_OK);
        for (unsigned fl : {0u, (unsigned)PH_FLAG_TRUNC, (unsigned)PH_FLAG_ORTH, (unsigned)(PH_FLAG_TRUNC | PH_FLAG_ORTH | PH_FLAG_SINGLE)}) {
          std::vector<int32_t> pl2(pl);
          if (fl & PH_FLAG_ORTH)
            for (auto& p : pl2) p = p > maxp ? maxp : p;
          EXPECT(ph_project_batch(c, px, dtype, W, N, pl2.data(), (int)pl2.size(), orth.off.data(), orth.q.data(), maxp, fl | dev,
                                  out.data()), PH_OK);
        }
        const int p_hi = N / 3 > 2 ? N / 3 : 2;
        std::vector<double> sw((size_t)W * (p_hi + 2));
        for (int mode : {PH_SWEEP_NORM, PH_SWEEP_NORM_GAMMA, PH_SWEEP_MAXABS}) {
          EXPECT(ph_sweep(c, px, dtype, W, N, 2, p_hi, mode, nullptr, nullptr, 0, dev, sw.data()), PH_OK);
          EXPECT(ph_sweep(c, px, dtype, W, N, 1, p_hi, mode, orth.off.data(), orth.q.data(), maxp, dev | PH_FLAG_ORTH, sw.data()),
                 PH_OK);
        }
        const int num = 5;
        std::vector<uint32_t> per((size_t)W * num);
        std::vector<double> pw((size_t)W * num), bases((size_t)W * num * N);
        std::vector<int32_t> st(W), nsw(W), cnt((size_t)2 * W), ips((size_t)W * 64);
        for (int gamma : {0, 1})
          for (unsigned fl : {0u, (unsigned)(PH_FLAG_TRUNC | PH_FLAG_ORTH)}) {
            EXPECT(ph_m_best(c, px, dtype, W, N, num, 2, p_hi, gamma, orth.off.data(), orth.q.data(), fac.off.data(), fac.q.data(),
                             maxp, fl | dev, per.data(), pw.data(), bases.data(), st.data(), nsw.data()), PH_OK);
          }
        EXPECT(ph_m_best(c, px, dtype, W, N, num, 2, -1, 0, nullptr, nullptr, fac.off.data(), fac.q.data(), maxp, dev, per.data(),
                         pw.data(), bases.data(), st.data(), nullptr), PH_OK);
        EXPECT(ph_m_best(c, px, dtype, W, N, num, 2, p_hi, 0, nullptr, nullptr, nullptr, nullptr, maxp, dev, per.data(), pw.data(),
                         bases.data(), st.data(), nullptr), PH_E_ARG);
        std::vector<double> spw((size_t)W * 16), sb((size_t)W * 16 * N);
        EXPECT(ph_small_to_large(c, px, dtype, W, N, 0.05, -1, nullptr, nullptr, 0, dev, 16, cnt.data(), ips.data(), spw.data(),
                                 sb.data(), st.data()), PH_OK);
        EXPECT(ph_small_to_large(c, px, dtype, W, N, 0.05, p_hi, orth.off.data(), orth.q.data(), maxp, dev | PH_FLAG_ORTH | PH_FLAG_NOSYNC,
                                 16, cnt.data(), ips.data(), spw.data(), nullptr, st.data()), PH_OK);
        EXPECT(ph_best_correlation(c, px, dtype, W, N, num, -1, 0.01, nullptr, nullptr, 0, dev, per.data(), pw.data(), bases.data(),
                                   st.data()), N >= 9 ? PH_OK : PH_OK);
        for (int win : {N, 64, 100, 4097})
          EXPECT(ph_best_frequency(c, px, dtype, W, N, win, num, orth.off.data(), orth.q.data(), maxp, dev, per.data(), pw.data(),
                                   bases.data(), st.data()), 2 * win <= maxp || true ? PH_OK : PH_OK);
        if (N >= 16) {
          const int qh = N / 3 < 700 ? N / 3 : 700;
          std::vector<double> rn((size_t)W * (qh + 1));
          EXPECT(ph_ramanujan_norms(c, px, dtype, W, N, 2, qh, dev, rn.data()), PH_OK);
          EXPECT(ph_ramanujan_norms(c, px, dtype, W, N, 5, 9, dev, rn.data()), PH_OK);
        }
        std::vector<int32_t> fp = {3, 8, N / 4 > 0 ? N / 4 : 1}, fk = {3, 7, N / 4 > 1 ? N / 4 - 1 : 1};
        const int rows = fk[0] + fk[1] + fk[2];
        std::vector<double> fs((size_t)W * rows), ts((size_t)W * N);
        EXPECT(ph_fold_sums(c, px, dtype, W, N, fp.data(), fk.data(), 3, dev, fs.data()), PH_OK);
        EXPECT(ph_tile_sum(c, fs.data(), W, N, fp.data(), fk.data(), 3, dtype, dev, ts.data()), PH_OK);
        for (int kcap : {64, 512, 1024}) {
          int ok = 0;
          EXPECT(ph_qo_feasible(c, dtype, N, p_hi, kcap, &ok), PH_OK);
          if (!ok) continue;
          std::vector<double> w((size_t)W * kcap), nr((size_t)W * num);
          std::vector<int32_t> kp((size_t)W * num);
          std::vector<char> resid((size_t)W * N * es);
          EXPECT(ph_qo_find_periods(c, px, dtype, W, N, num, 0.1, 2, p_hi, kcap, dev, per.data(), nr.data(), kp.data(), cnt.data(),
                                    w.data(), resid.data(), st.data()), PH_OK);
        }
        const int mp = N / 2 > 2 ? N / 2 : 2;
        std::vector<double> ac((size_t)W * N), e3((size_t)W * mp), op((size_t)W * mp);
        EXPECT(ph_orth_powers(c, px, dtype, W, N, mp, 1, dev, ac.data(), e3.data(), op.data()), PH_OK);
        EXPECT(ph_orth_powers(c, px, dtype, W, N, -1, 0, dev, nullptr, nullptr, op.data()), PH_OK);
      }
    }
    // a dictionary for ph_dict_project
    if (N <= 1000) {
      std::vector<double> basis((size_t)6 * N, 0.5);
      std::vector<float> proj((size_t)6 * N);
      EXPECT(ph_dict_project(c, x.data(), basis.data(), 6, N, 0, proj.data()), PH_OK);
    }
    // malformed tables and arguments must be refused, not read
    Csr bad = orth;
    bad.off[3] = bad.off[2] - 1 < 0 ? 5 : bad.off[2] - 1;
    bad.off[4] = 0;
    std::vector<double> out((size_t)W * N);
    std::vector<int32_t> one = {2};
    EXPECT(ph_project_batch(c, x.data(), PH_F64, W, N, one.data(), 1, bad.off.data(), bad.q.data(), maxp, PH_FLAG_ORTH, out.data()),
           PH_E_ARG);
    EXPECT(ph_project_batch(c, x.data(), PH_F64, W, N, one.data(), 1, orth.off.data(), orth.q.data(), 1, PH_FLAG_ORTH, out.data()),
           PH_E_ARG);
    EXPECT(ph_project_batch(c, x.data(), 7, W, N, one.data(), 1, nullptr, nullptr, 0, 0, out.data()), PH_E_ARG);
    EXPECT(ph_project_batch(c, nullptr, PH_F64, W, N, one.data(), 1, nullptr, nullptr, 0, 0, out.data()), PH_E_ARG);
    EXPECT(ph_sweep(c, x.data(), PH_F64, 0, N, 2, 3, 0, nullptr, nullptr, 0, 0, out.data()), PH_E_ARG);
  }
  plan_checks(c);
  hbm_window_checks();
  float ms[300];
  int cntp = 0;
  EXPECT(ph_profile_read(c, ms, 300, &cntp), PH_OK);
  for (int i = 0; i < cntp && i < 256; ++i) (void)ph_profile_name(c, i);
  EXPECT(ph_sync(c), PH_OK);
  EXPECT(ph_destroy(c), PH_OK);
  return finish("");
}

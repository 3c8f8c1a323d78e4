// Drives ph_qo_get_periods through the HOST half of the library (hip_stub.cpp stands in for the runtime; kernels do not
// run, outputs are not looked at).  Built with -fsanitize=address,undefined by tests/test_host_sanitizers.py:
// argument validation, the plan query, the Moebius tables, the staging of the three int32 lists beside the weights and
// the workspaces must touch no byte out of bounds, and the one launch must ask for the LDS and the workgroup width that
// ph_plan_info(PH_OP_QO_GET_PERIODS) names.
#include "driver_common.h"

int main() {
  ph_ctx* c = nullptr;
  EXPECT(ph_create(0, &c), PH_OK);
  EXPECT(ph_profile_enable(c, 1), PH_OK);
  // {W, pcap, largest period}: sum(p) from a few doubles (LDS) to far beyond the LDS (HBM workspace)
  const int sizes[][3] = {{1, 1, 1}, {3, 2, 18}, {5, 5, 100}, {2, 3, 5461}, {1, 4, 20000}, {2, 64, 1 << 20}};
  for (const auto& sz : sizes) {
    const int W = sz[0], pcap = sz[1], pmax = sz[2];
    std::vector<int32_t> per((size_t)W * pcap), rws((size_t)W * pcap), cnt(W), st(W);
    int64_t ccap64 = 0, kcap64 = 0;
    for (int w = 0; w < W; ++w) {
      int64_t sp = 0, sr = 0;
      cnt[w] = pcap - (w % 2 && pcap > 1 ? 1 : 0);
      for (int a = 0; a < pcap; ++a) {
        const int p = pmax - 7 * a > 0 ? pmax - 7 * a : 1;
        per[(size_t)w * pcap + a] = p;
        rws[(size_t)w * pcap + a] = p - (a > 0 && p > 1 ? 1 : 0);
        if (a < cnt[w]) {
          sp += p;
          sr += rws[(size_t)w * pcap + a];
        }
      }
      ccap64 = sp > ccap64 ? sp : ccap64;
      kcap64 = sr > kcap64 ? sr : kcap64;
    }
    if (ccap64 > (1 << 24)) ccap64 = 1 << 24;  // (the kernel would answer PH_ST_CAP; the host half does not care)
    if (kcap64 > (1 << 24)) kcap64 = 1 << 24;
    const int ccap = (int)ccap64, kcap = (int)kcap64;
    std::vector<double> wts((size_t)W * kcap, 0.25), out((size_t)W * ccap);
    for (unsigned dev : {0u, (unsigned)PH_FLAG_DEVICE}) {
      int32_t plan[PH_PLAN_LEN];
      const int32_t prm[2] = {ccap, pmax};
      EXPECT(ph_plan_info(c, PH_OP_QO_GET_PERIODS, PH_F64, ccap, prm, 2, 0, plan), PH_OK);
      stub_reset_launches();
      EXPECT(ph_qo_get_periods(c, per.data(), rws.data(), cnt.data(), W, pcap, wts.data(), kcap, pmax, ccap, dev, out.data(),
                               st.data()), PH_OK);
      int block[4];
      long long l[4];
      const int n = stub_launches(block, l, 4);
      if (n != 1 || l[0] != plan[PH_PLAN_K0 + PH_PLAN_LDS_BYTES] || block[0] != plan[PH_PLAN_K0 + PH_PLAN_BLOCK] ||
          plan[PH_PLAN_KERNELS] != 1 || plan[PH_PLAN_K0 + PH_PLAN_WINDOW] != plan[PH_PLAN_K0 + PH_PLAN_SECOND]) {
        std::printf("FAIL W %d pcap %d pmax %d flags %u: %d launches, lds %lld block %d, plan lds %d block %d\n", W, pcap, pmax, dev,
                    n, n ? l[0] : -1LL, n ? block[0] : -1, plan[PH_PLAN_K0 + PH_PLAN_LDS_BYTES], plan[PH_PLAN_K0 + PH_PLAN_BLOCK]);
        ++fails;
      }
      launched("k_qo_extract");
      // a few doubles fit the LDS, a sum of periods beyond it does not
      const int where = plan[PH_PLAN_K0 + PH_PLAN_WINDOW];
      if ((ccap <= 1000 && where != PH_PLAN_LDS) || (ccap >= 20000 && where != PH_PLAN_HBM)) {
        std::printf("FAIL ccap %d placed %d\n", ccap, where);
        ++fails;
      }
      // refused, not read
#define GETP(ctx, pp, rr, cc, ww, pc, wt, kc, mp, cp, oo, ss) \
  ph_qo_get_periods(ctx, pp, rr, cc, ww, pc, wt, kc, mp, cp, dev, oo, ss)
      EXPECT(GETP(nullptr, per.data(), rws.data(), cnt.data(), W, pcap, wts.data(), kcap, pmax, ccap, out.data(), st.data()), PH_E_ARG);
      EXPECT(GETP(c, nullptr, rws.data(), cnt.data(), W, pcap, wts.data(), kcap, pmax, ccap, out.data(), st.data()), PH_E_ARG);
      EXPECT(GETP(c, per.data(), nullptr, cnt.data(), W, pcap, wts.data(), kcap, pmax, ccap, out.data(), st.data()), PH_E_ARG);
      EXPECT(GETP(c, per.data(), rws.data(), nullptr, W, pcap, wts.data(), kcap, pmax, ccap, out.data(), st.data()), PH_E_ARG);
      EXPECT(GETP(c, per.data(), rws.data(), cnt.data(), W, pcap, nullptr, kcap, pmax, ccap, out.data(), st.data()), PH_E_ARG);
      EXPECT(GETP(c, per.data(), rws.data(), cnt.data(), W, pcap, wts.data(), kcap, pmax, ccap, nullptr, st.data()), PH_E_ARG);
      EXPECT(GETP(c, per.data(), rws.data(), cnt.data(), W, pcap, wts.data(), kcap, pmax, ccap, out.data(), nullptr), PH_E_ARG);
      EXPECT(GETP(c, per.data(), rws.data(), cnt.data(), 0, pcap, wts.data(), kcap, pmax, ccap, out.data(), st.data()), PH_E_ARG);
      EXPECT(GETP(c, per.data(), rws.data(), cnt.data(), W, 0, wts.data(), kcap, pmax, ccap, out.data(), st.data()), PH_E_ARG);
      EXPECT(GETP(c, per.data(), rws.data(), cnt.data(), W, (1 << 20) + 1, wts.data(), kcap, pmax, ccap, out.data(), st.data()), PH_E_ARG);
      EXPECT(GETP(c, per.data(), rws.data(), cnt.data(), W, pcap, wts.data(), 0, pmax, ccap, out.data(), st.data()), PH_E_ARG);
      EXPECT(GETP(c, per.data(), rws.data(), cnt.data(), W, pcap, wts.data(), (1 << 24) + 1, pmax, ccap, out.data(), st.data()), PH_E_ARG);
      EXPECT(GETP(c, per.data(), rws.data(), cnt.data(), W, pcap, wts.data(), kcap, 0, ccap, out.data(), st.data()), PH_E_ARG);
      EXPECT(GETP(c, per.data(), rws.data(), cnt.data(), W, pcap, wts.data(), kcap, (1 << 20) + 1, ccap, out.data(), st.data()), PH_E_ARG);
      EXPECT(GETP(c, per.data(), rws.data(), cnt.data(), W, pcap, wts.data(), kcap, pmax, 0, out.data(), st.data()), PH_E_ARG);
      EXPECT(GETP(c, per.data(), rws.data(), cnt.data(), W, pcap, wts.data(), kcap, pmax, (1 << 24) + 1, out.data(), st.data()), PH_E_ARG);
#undef GETP
    }
  }
  // the plan query: defaults, a NULL context, a NULL record, bad parameters
  int32_t plan[PH_PLAN_LEN];
  EXPECT(ph_plan_info(c, PH_OP_QO_GET_PERIODS, PH_F64, 600, nullptr, 0, 0, plan), PH_OK);
  EXPECT(ph_plan_info(nullptr, PH_OP_QO_GET_PERIODS, PH_F64, 600, nullptr, 0, 0, plan), PH_E_ARG);
  EXPECT(ph_plan_info(c, PH_OP_QO_GET_PERIODS, PH_F64, 600, nullptr, 0, 0, nullptr), PH_E_ARG);
  const int32_t bad0[2] = {0, 10}, bad1[2] = {100, 0}, bad2[2] = {100, (1 << 20) + 1};
  EXPECT(ph_plan_info(c, PH_OP_QO_GET_PERIODS, PH_F64, 600, bad0, 2, 0, plan), PH_E_ARG);
  EXPECT(ph_plan_info(c, PH_OP_QO_GET_PERIODS, PH_F64, 600, bad1, 2, 0, plan), PH_E_ARG);
  EXPECT(ph_plan_info(c, PH_OP_QO_GET_PERIODS, PH_F64, 600, bad2, 2, 0, plan), PH_E_ARG);
  EXPECT(ph_plan_info(c, PH_OP_QO_GET_PERIODS + 1, PH_F64, 600, nullptr, 0, 0, plan), PH_E_ARG);
  // the profile name of every launch
  float ms[300];
  int cntp = 0;
  EXPECT(ph_profile_read(c, ms, 300, &cntp), PH_OK);
  check_profile(c, cntp);
  EXPECT(ph_sync(c), PH_OK);
  EXPECT(ph_destroy(c), PH_OK);
  return finish("get_periods");
}

// Drives ph_period_path and ph_period_path_plan_info through the HOST half of the library (hip_stub.cpp stands in for the
// runtime; kernels do not run, outputs are not looked at).  Built with -fsanitize=address,undefined by
// tests/test_host_sanitizers_path.py: every refusal, the host-pointer staging of dense and of strided cost tables with
// exact-size vectors (the table goes up as it lies: (R * W - 1) * ld + P doubles), a NULL value array, R = 0, and the
// size arithmetic with R * W * P and R * W * ld beyond 2^31 must touch no byte out of bounds and overflow no integer;
// every accepted call is one launch with the block and the LDS bytes of the plan query, named k_period_path.
#include <cmath>
#include <limits>

#include "driver_common.h"

// one launch since the last reset, with the plan query's block and LDS for P columns
static void path_launch(ph_ctx* c, int P, int line) {
  int block[4];
  long long l[4];
  int pb = 0, pl = 0, pt = 0;
  EXPECT(ph_period_path_plan_info(c, P, &pb, &pl, &pt), PH_OK);
  const int ns = (P + 1023) / 1024, want_block = ((P + ns - 1) / ns + 63) / 64 * 64;  // equal states per thread
  const int n = stub_launches(block, l, 4);
  if (n != 1 || block[0] != pb || l[0] != pl || pb != want_block || pt < 1) {
    std::printf("FAIL line %d: %d launches, block %d (plan %d, want %d), lds %lld (plan %d), tile %d\n", line, n,
                n ? block[0] : -1, pb, want_block, n ? l[0] : -1LL, pl, pt);
    ++fails;
  }
  launched("k_period_path");
  stub_reset_launches();
}

int main() {
  ph_ctx* c = nullptr;
  EXPECT(ph_create(0, &c), PH_OK);
  EXPECT(ph_profile_enable(c, 1), PH_OK);
  stub_reset_launches();

  // ---- host-pointer staging: {R, W, P, ld, band}
  const int shapes[][5] = {{1, 1, 1, 1, 0},     {1, 7, 5, 5, 2},      {3, 4, 63, 63, 8},     {2, 5, 64, 80, 64},
                           {1, 3, 1025, 1030, 1}, {4, 2, 1365, 1366, 8}, {1, 2, 8192, 8192, 64}, {2, 1, 8192, 8200, 0},
                           {5, 9, 2, 1000, 1}};
  for (const auto& sh : shapes) {
    const int R = sh[0], W = sh[1], P = sh[2], ld = sh[3], band = sh[4];
    const size_t rows = (size_t)R * W;
    std::vector<double> cost((rows - 1) * ld + P, 1.0), value(rows), score(R);  // exact: not a double behind the last row
    std::vector<int32_t> path(rows), status(R);
    EXPECT(ph_period_path(c, cost.data(), R, W, P, ld, band, 0.25, 0, path.data(), value.data(), score.data(), status.data()),
           PH_OK);
    path_launch(c, P, __LINE__);
    EXPECT(ph_period_path(c, cost.data(), R, W, P, ld, band, 0.0, 0, path.data(), nullptr, score.data(), status.data()), PH_OK);
    path_launch(c, P, __LINE__);
    EXPECT(ph_period_path(c, cost.data(), R, W, P, ld, band, 1e300, PH_FLAG_DEVICE, path.data(), value.data(), score.data(),
                          status.data()), PH_OK);
    path_launch(c, P, __LINE__);
  }

  // ---- the plan query: the tile height falls as the rows grow, and what it reports fits the device
  {
    int last_tile = 1 << 30;
    for (int P : {1, 2, 63, 64, 65, 1023, 1024, 1025, 1365, 4096, 8191, 8192}) {
      int block = 0, lds = 0, tile = 0;
      EXPECT(ph_period_path_plan_info(c, P, &block, &lds, &tile), PH_OK);
      const int row = (P + 15) / 16 * 16;
      if (block < 64 || block > 1024 || block % 64 || lds > 160 * 1024 || tile < 1 || tile > last_tile ||
          (long long)tile * (row + 4) > lds || (long long)block * 8 < P) {
        std::printf("FAIL plan P=%d: block %d, lds %d, tile %d\n", P, block, lds, tile);
        ++fails;
      }
      last_tile = tile;
    }
    int x = 0;
    EXPECT(ph_period_path_plan_info(nullptr, 64, &x, &x, &x), PH_E_ARG);
    EXPECT(ph_period_path_plan_info(c, 64, nullptr, &x, &x), PH_E_ARG);
    EXPECT(ph_period_path_plan_info(c, 64, &x, nullptr, &x), PH_E_ARG);
    EXPECT(ph_period_path_plan_info(c, 64, &x, &x, nullptr), PH_E_ARG);
    EXPECT(ph_period_path_plan_info(c, 0, &x, &x, &x), PH_E_ARG);
    EXPECT(ph_period_path_plan_info(c, 8193, &x, &x, &x), PH_E_ARG);
    said("P=", __LINE__);
    no_launch(__LINE__);
  }

  // ---- sizes beyond 2^31, device form: the pointers are never dereferenced on the host.  The back-pointer workspace is
  // real (R * W * P bytes: 2^31 + 2^14 here, never touched), so a machine that cannot give it answers PH_E_NOMEM
  {
    double tiny[2] = {0, 0};
    int32_t* ti = reinterpret_cast<int32_t*>(tiny);
    const int64_t W = ((int64_t)1 << 17) + 1;  // R * W * P = 2^31 + 2^14, R * W * ld = 2^38 + 2^21
    const int rc = ph_period_path(c, tiny, 2, W, 8192, (int64_t)1 << 20, 64, 0.0, PH_FLAG_DEVICE, ti, tiny, tiny, ti);
    if (rc == PH_OK) {
      path_launch(c, 8192, __LINE__);
    } else if (rc != PH_E_NOMEM) {
      std::printf("FAIL line %d: -> %d (%s)\n", __LINE__, rc, ph_last_error());
      ++fails;
    }
    stub_reset_launches();
    // byte counts that do not fit 64 bits are refused, not wrapped (nothing is allocated for them)
    EXPECT(ph_period_path(c, tiny, 1, INT64_MAX / 16, 1, 2, 0, 0.0, PH_FLAG_DEVICE, ti, tiny, tiny, ti), PH_E_ARG);
    said("64 bits", __LINE__);
    EXPECT(ph_period_path(c, tiny, 2, INT64_MAX / 32 + 1, 1, 1, 0, 0.0, PH_FLAG_DEVICE, ti, tiny, tiny, ti), PH_E_ARG);
    said("64 bits", __LINE__);
    EXPECT(ph_period_path(c, tiny, 1, 2, 1, INT64_MAX, 0, 0.0, PH_FLAG_DEVICE, ti, tiny, tiny, ti), PH_E_ARG);
    said("64 bits", __LINE__);
    EXPECT(ph_period_path(c, tiny, 0x7fffffffLL, (int64_t)1 << 40, 8192, 8192, 0, 0.0, PH_FLAG_DEVICE, ti, tiny, tiny, ti),
           PH_E_ARG);
    said("64 bits", __LINE__);
    no_launch(__LINE__);
  }

  // ---- refused, not read; R = 0 is accepted and launches nothing
  {
    std::vector<double> cost(2 * 3 * 5), value(6), score(2);
    std::vector<int32_t> path(6), status(2);
    const double inf = std::numeric_limits<double>::infinity();
    for (unsigned dev : {0u, (unsigned)PH_FLAG_DEVICE}) {
#define PP(ctx, cc, R, W, P, ld, band, jump, pa, sc, st) \
  ph_period_path(ctx, cc, R, W, P, ld, band, jump, dev, pa, value.data(), sc, st)
      EXPECT(PP(nullptr, cost.data(), 2, 3, 5, 5, 2, 0.5, path.data(), score.data(), status.data()), PH_E_ARG);
      said("ctx", __LINE__);
      EXPECT(PP(c, nullptr, 2, 3, 5, 5, 2, 0.5, path.data(), score.data(), status.data()), PH_E_ARG);
      said("NULL", __LINE__);
      EXPECT(PP(c, cost.data(), 2, 3, 5, 5, 2, 0.5, nullptr, score.data(), status.data()), PH_E_ARG);
      EXPECT(PP(c, cost.data(), 2, 3, 5, 5, 2, 0.5, path.data(), nullptr, status.data()), PH_E_ARG);
      EXPECT(PP(c, cost.data(), 2, 3, 5, 5, 2, 0.5, path.data(), score.data(), nullptr), PH_E_ARG);
      EXPECT(PP(c, cost.data(), 2, 3, 0, 5, 2, 0.5, path.data(), score.data(), status.data()), PH_E_ARG);
      said("P=", __LINE__);
      EXPECT(PP(c, cost.data(), 2, 3, -1, 5, 2, 0.5, path.data(), score.data(), status.data()), PH_E_ARG);
      EXPECT(PP(c, cost.data(), 2, 3, 8193, 8193, 2, 0.5, path.data(), score.data(), status.data()), PH_E_ARG);
      said("P=", __LINE__);
      EXPECT(PP(c, cost.data(), 2, 3, INT32_MAX, INT32_MAX, 2, 0.5, path.data(), score.data(), status.data()), PH_E_ARG);
      EXPECT(PP(c, cost.data(), 2, 3, 5, 5, -1, 0.5, path.data(), score.data(), status.data()), PH_E_ARG);
      said("band", __LINE__);
      EXPECT(PP(c, cost.data(), 2, 3, 5, 5, 65, 0.5, path.data(), score.data(), status.data()), PH_E_ARG);
      said("band", __LINE__);
      EXPECT(PP(c, cost.data(), 2, 3, 5, 5, 2, -0.5, path.data(), score.data(), status.data()), PH_E_ARG);
      said("jump", __LINE__);
      EXPECT(PP(c, cost.data(), 2, 3, 5, 5, 2, inf, path.data(), score.data(), status.data()), PH_E_ARG);
      EXPECT(PP(c, cost.data(), 2, 3, 5, 5, 2, -inf, path.data(), score.data(), status.data()), PH_E_ARG);
      EXPECT(PP(c, cost.data(), 2, 3, 5, 5, 2, std::nan(""), path.data(), score.data(), status.data()), PH_E_ARG);
      said("jump", __LINE__);
      EXPECT(PP(c, cost.data(), 2, 0, 5, 5, 2, 0.5, path.data(), score.data(), status.data()), PH_E_ARG);
      said("W=", __LINE__);
      EXPECT(PP(c, cost.data(), 2, -4, 5, 5, 2, 0.5, path.data(), score.data(), status.data()), PH_E_ARG);
      EXPECT(PP(c, cost.data(), 2, INT64_MIN, 5, 5, 2, 0.5, path.data(), score.data(), status.data()), PH_E_ARG);
      EXPECT(PP(c, cost.data(), -1, 3, 5, 5, 2, 0.5, path.data(), score.data(), status.data()), PH_E_ARG);
      said("R=", __LINE__);
      EXPECT(PP(c, cost.data(), (int64_t)1 << 31, 3, 5, 5, 2, 0.5, path.data(), score.data(), status.data()), PH_E_ARG);
      EXPECT(PP(c, cost.data(), INT64_MIN, 3, 5, 5, 2, 0.5, path.data(), score.data(), status.data()), PH_E_ARG);
      EXPECT(PP(c, cost.data(), 2, 3, 5, 4, 2, 0.5, path.data(), score.data(), status.data()), PH_E_ARG);
      said("ld=", __LINE__);
      EXPECT(PP(c, cost.data(), 2, 3, 5, 0, 2, 0.5, path.data(), score.data(), status.data()), PH_E_ARG);
      EXPECT(PP(c, cost.data(), 2, 3, 5, INT64_MIN, 2, 0.5, path.data(), score.data(), status.data()), PH_E_ARG);
      no_launch(__LINE__);
      EXPECT(PP(c, cost.data(), 0, 3, 5, 5, 2, 0.5, path.data(), score.data(), status.data()), PH_OK);
      no_launch(__LINE__);
#undef PP
    }
    // the limits themselves
    EXPECT(ph_period_path(c, cost.data(), 2, 3, 5, 5, 64, 0.0, 0, path.data(), value.data(), score.data(), status.data()), PH_OK);
    path_launch(c, 5, __LINE__);
    EXPECT(ph_period_path(c, cost.data(), 2, 3, 5, 5, 0, 1.7976931348623157e308, 0, path.data(), value.data(), score.data(),
                          status.data()), PH_OK);
    path_launch(c, 5, __LINE__);
  }

  // ---- the profile name of every launch
  float ms[300];
  int cntp = 0;
  EXPECT(ph_profile_read(c, ms, 300, &cntp), PH_OK);
  check_profile(c, cntp);
  EXPECT(ph_sync(c), PH_OK);
  EXPECT(ph_destroy(c), PH_OK);
  return finish("path");
}

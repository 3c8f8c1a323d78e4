// Walks a grid of arguments through ph_plan_info, ph_qo_plan_info and ph_qo_feasible on three contexts (default,
// PH_HBM_WINDOW=1, pair kernels off) and writes every answer as one line of text: the table of LDS sizes and placements
// the host derives from the kernels' carve functions.  With a path as first argument the table goes to that file (to be
// compared between two builds of the library); without, only its line count and a hash are printed.  For a sample of the
// grid the entry point itself runs through the stub and the launches it records must carry the plan's block and LDS
// bytes.  Built with -fsanitize=address,undefined by tests/test_host_sanitizers.py like its siblings.
#include <cmath>
#include <cstdarg>
#include <cstdint>
#include <string>

#include "driver_common.h"

static FILE* table = nullptr;
static uint64_t table_hash = 1469598103934665603ull;
static long table_lines = 0;

static void emit(const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  const int n = std::vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  for (int i = 0; i < n && i < (int)sizeof buf - 1; ++i) table_hash = (table_hash ^ (unsigned char)buf[i]) * 1099511628211ull;
  ++table_lines;
  if (table) std::fprintf(table, "%s\n", buf);
}

static void plan_line(ph_ctx* c, const char* ctx, int op, int dtype, int N, std::vector<int32_t> prm, unsigned fl) {
  int32_t rec[PH_PLAN_LEN] = {};
  const int rc = ph_plan_info(c, op, dtype, N, prm.data(), (int)prm.size(), fl, rec);
  std::string p, r;
  for (int32_t v : prm) p += " " + std::to_string(v);
  if (rc == PH_OK)
    for (int32_t v : rec) r += " " + std::to_string(v);
  else
    r = std::string(" ") + ph_last_error();
  emit("%s op %d dtype %d N %d flags %u prm%s -> %d:%s", ctx, op, dtype, N, fl, p.c_str(), rc, r.c_str());
}

static void walk(ph_ctx* c, const char* ctx) {
  const unsigned modes[3] = {0u, (unsigned)PH_FLAG_TRUNC, (unsigned)PH_FLAG_ORTH};
  for (int N = 4; N <= 45000; N += (N < 200 ? 1 : 61)) {
    for (int dtype : {PH_F64, PH_F32}) {
      for (int ml : {2, 300, N / 3}) {
        for (unsigned fl : modes) {
          plan_line(c, ctx, PH_OP_PROJECT, dtype, N, {ml}, fl);
          for (int mode : {PH_SWEEP_NORM, PH_SWEEP_MAXABS}) plan_line(c, ctx, PH_OP_SWEEP, dtype, N, {2, ml, mode}, fl);
          for (int num : {1, 3, 10}) plan_line(c, ctx, PH_OP_M_BEST, dtype, N, {num, 2, ml}, fl);
          plan_line(c, ctx, PH_OP_SMALL_TO_LARGE, dtype, N, {ml}, fl);
          plan_line(c, ctx, PH_OP_BEST_CORRELATION, dtype, N, {ml}, fl);
          plan_line(c, ctx, PH_OP_QO_ORTH_SELECT, dtype, N, {ml}, fl);
        }
        plan_line(c, ctx, PH_OP_ORTH_POWERS, dtype, N, {ml}, 0);
        for (int kcap : {1, 64, 512, 1024, 2048}) {
          plan_line(c, ctx, PH_OP_QO_FIT, dtype, N, {kcap, ml}, 0);
          plan_line(c, ctx, PH_OP_QO_FIT_WIN, dtype, N, {kcap, ml}, 0);
          for (unsigned fl : {0u, (unsigned)PH_FLAG_TRUNC, (unsigned)PH_FLAG_KEEP_WEIGHTS}) {
            int lds = -1, place = -1;
            const int rc = ph_qo_plan_info(c, dtype, N, ml, kcap, fl, &lds, &place);
            emit("%s qo_plan dtype %d N %d ml %d kcap %d flags %u -> %d: %d %d%s%s", ctx, dtype, N, ml, kcap, fl, rc, lds, place,
                 rc == PH_OK ? "" : " ", rc == PH_OK ? "" : ph_last_error());
          }
          int ok = -1;
          const int rc = ph_qo_feasible(c, dtype, N, ml, kcap, &ok);
          emit("%s qo_feasible dtype %d N %d ml %d kcap %d -> %d: %d", ctx, dtype, N, ml, kcap, rc, ok);
        }
        for (int ccap : {N, 2048, 16 * N}) plan_line(c, ctx, PH_OP_QO_GET_PERIODS, dtype, N, {ccap, ml}, 0);
      }
      for (unsigned fl : modes)
        for (int win : {N, 300, 4096, 16384}) plan_line(c, ctx, PH_OP_BEST_FREQUENCY, dtype, N, {win}, fl);
      for (int qh : {64, 128, 512, N / 3}) plan_line(c, ctx, PH_OP_RAMANUJAN, dtype, N, {2, qh}, 0);
      plan_line(c, ctx, PH_OP_FOLD_SUMS, dtype, N, {}, 0);
    }
  }
}

// proper divisors d of p with 1 < d < p
static void factor_tables(int max_p, std::vector<int32_t>* off, std::vector<int32_t>* q) {
  off->assign(max_p + 2, 0);
  for (int p = 0; p <= max_p; ++p) {
    (*off)[p] = (int32_t)q->size();
    for (int d = 2; p > 0 && d < p; ++d)
      if (p % d == 0) q->push_back(d);
  }
  (*off)[max_p + 1] = (int32_t)q->size();
  if (q->empty()) q->push_back(1);
}

// ph_plan_info for `op`, then the entry point itself: the launches the stub records are the plan's kernels, with the
// plan's block size and dynamic LDS.
template <typename F>
static void expect_plan(ph_ctx* c, int op, int dtype, int N, std::vector<int32_t> prm, unsigned fl, int line, F run) {
  int32_t rec[PH_PLAN_LEN];
  EXPECT(ph_plan_info(c, op, dtype, N, prm.data(), (int)prm.size(), fl, rec), PH_OK);
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
    std::printf("FAIL line %d: op %d dtype %d N %d flags %u: run -> %d (%s), %d launches, plan %d kernels\n", line, op, dtype, N,
                fl, rr, ph_last_error(), n, rec[PH_PLAN_KERNELS]);
    ++fails;
  }
}

static void sample_launches(ph_ctx* c) {
  const int max_len = 300, num = 3;
  std::vector<int32_t> fac_off, fac_q;
  factor_tables(max_len, &fac_off, &fac_q);
  for (int N : {700, 4096, 9705, 12000, 30000}) {
    std::vector<double> x((size_t)N);
    for (int i = 0; i < N; ++i) x[i] = std::sin(0.37 * i) + 0.25 * std::sin(0.05 * i);
    std::vector<float> xf(x.begin(), x.end());
    for (int dtype : {PH_F64, PH_F32}) {
      const void* px = dtype == PH_F64 ? (const void*)x.data() : (const void*)xf.data();
      for (unsigned fl : {0u, (unsigned)PH_FLAG_TRUNC}) {
        std::vector<uint32_t> per(num);
        std::vector<double> pw(num), bases((size_t)num * N), sw(max_len + 1), proj((size_t)2 * N), sb((size_t)16 * N), spw(16);
        std::vector<int32_t> st(1), cnt(1), ip(16), pl = {7, max_len};
        expect_plan(c, PH_OP_PROJECT, dtype, N, {max_len}, fl, __LINE__, [&] {
          return ph_project_batch(c, px, dtype, 1, N, pl.data(), 2, nullptr, nullptr, 0, fl, proj.data());
        });
        expect_plan(c, PH_OP_SWEEP, dtype, N, {2, max_len, PH_SWEEP_NORM}, fl, __LINE__, [&] {
          return ph_sweep(c, px, dtype, 1, N, 2, max_len, PH_SWEEP_NORM, nullptr, nullptr, 0, fl, sw.data());
        });
        expect_plan(c, PH_OP_M_BEST, dtype, N, {num, 2, max_len}, fl, __LINE__, [&] {
          return ph_m_best(c, px, dtype, 1, N, num, 2, max_len, 0, nullptr, nullptr, fac_off.data(), fac_q.data(), max_len, fl,
                           per.data(), pw.data(), bases.data(), st.data(), nullptr);
        });
        expect_plan(c, PH_OP_SMALL_TO_LARGE, dtype, N, {max_len}, fl, __LINE__, [&] {
          return ph_small_to_large(c, px, dtype, 1, N, 0.05, max_len, nullptr, nullptr, 0, fl, 16, cnt.data(), ip.data(),
                                   spw.data(), sb.data(), st.data());
        });
        expect_plan(c, PH_OP_BEST_CORRELATION, dtype, N, {max_len}, fl, __LINE__, [&] {
          return ph_best_correlation(c, px, dtype, 1, N, num, max_len, 0.01, nullptr, nullptr, 0, fl, per.data(), pw.data(),
                                     bases.data(), st.data());
        });
      }
      for (int qh : {64, 512}) {
        std::vector<double> rn((size_t)qh + 1);
        expect_plan(c, PH_OP_RAMANUJAN, dtype, N, {2, qh}, 0, __LINE__, [&] {
          return ph_ramanujan_norms(c, px, dtype, 1, N, 2, qh, 0, rn.data());
        });
      }
      std::vector<double> op((size_t)max_len), fs(10);
      std::vector<int32_t> fp = {3, 8}, fk = {3, 7};
      expect_plan(c, PH_OP_ORTH_POWERS, dtype, N, {max_len}, 0, __LINE__, [&] {
        return ph_orth_powers(c, px, dtype, 1, N, max_len, 0, 0, nullptr, nullptr, op.data());
      });
      expect_plan(c, PH_OP_FOLD_SUMS, dtype, N, {}, 0, __LINE__, [&] {
        return ph_fold_sums(c, px, dtype, 1, N, fp.data(), fk.data(), 2, 0, fs.data());
      });
    }
  }
}

int main(int argc, char** argv) {
  if (argc > 1 && !(table = std::fopen(argv[1], "w"))) {
    std::printf("cannot write %s\n", argv[1]);
    return 2;
  }
  ph_ctx *def = nullptr, *hbm = nullptr, *one = nullptr;
  EXPECT(ph_create(0, &def), PH_OK);
  setenv("PH_HBM_WINDOW", "1", 1);
  EXPECT(ph_create(0, &hbm), PH_OK);
  unsetenv("PH_HBM_WINDOW");
  for (const char* v : {"PH_STEP1_PAIR", "PH_S2L_PAIR", "PH_BC_PAIR"}) setenv(v, "0", 1);
  EXPECT(ph_create(0, &one), PH_OK);
  for (const char* v : {"PH_STEP1_PAIR", "PH_S2L_PAIR", "PH_BC_PAIR"}) unsetenv(v);
  walk(def, "default");
  walk(hbm, "hbm_window");
  walk(one, "no_pair");
  if (table) std::fclose(table);
  std::printf("plan table: %ld lines, fnv1a %016llx\n", table_lines, (unsigned long long)table_hash);
  sample_launches(def);
  sample_launches(hbm);
  sample_launches(one);
  EXPECT(ph_destroy(def), PH_OK);
  EXPECT(ph_destroy(hbm), PH_OK);
  EXPECT(ph_destroy(one), PH_OK);
  return finish("plans");
}

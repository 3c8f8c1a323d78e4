// libperiod_hip.so -- C ABI (include/periodhip.h) over the gfx950 kernels (ph_kernels.h: one header per algorithm).
// Host side only: argument checks, device staging for host-pointer calls, small integer
// tables, launch geometry.  No compute happens on the host.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/periodhip.h"
#include "ph_kernels.h"
#include "ph_fit.h"
#include "ph_frames.h"
#include "ph_follow.h"

namespace {

thread_local std::string g_err;

int fail(int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  g_err = buf;
  return code;
}

#define PH_HIP(call)                                                                         \
  do {                                                                                       \
    hipError_t e_ = (call);                                                                  \
    if (e_ != hipSuccess)                                                                    \
      return fail(e_ == hipErrorOutOfMemory ? PH_E_NOMEM : PH_E_HIP, "%s failed: %s", #call, \
                  hipGetErrorString(e_));                                                    \
  } while (0)

#define PH_TRY(expr)          \
  do {                        \
    int rc_ = (expr);         \
    if (rc_ != PH_OK) return rc_; \
  } while (0)

struct DevBuf {
  void* p = nullptr;
  size_t cap = 0;
};

struct TableSlot {
  DevBuf dev;
  std::vector<int32_t> host;  // last uploaded content (skip identical re-uploads)
  bool valid = false;
};

enum { T_PLIST, T_ORTH_OFF, T_ORTH_Q, T_FAC_OFF, T_FAC_Q, T_AUX0, T_AUX1, T_AUX2, T_AUX3, T_FIT_PHI, T_FIT_OFF, T_FIT_DQ, T_COUNT };
enum { B_IN, B_OUT0, B_OUT1, B_OUT2, B_OUT3, B_OUT4, B_WS0, B_WS1, B_GEN0, B_GBUF, B_GWIN, B_COUNT };

}  // namespace

struct ph_ctx {
  int device = 0;
  hipStream_t own_stream = nullptr;
  hipStream_t stream = nullptr;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  int num_cu = 0;
  int lds_limit = 0;
  DevBuf buf[B_COUNT];
  TableSlot tab[T_COUNT];
  // per-period fold geometry for the tuned sweeps, cached for the last (N, max_p)
  DevBuf geom;
  DevBuf geomf;  // the same table in float (ph::PGeomF), for the window-pair screen
  DevBuf radq;   // radius of that screen per period: ph::pair_radius(ceil(N / q), q) (pair_radius_table)
  DevBuf kapf;   // kappa_q of k_small_to_large_pair's flag test (ph::s2l_kappa, rounded up to float)
  int geom_n = -1, geom_max_p = -1;
  bool step1_pair = true;  // PH_STEP1_PAIR=0: always the one-window fp64 kernel for m_best step 1
  bool s2l_pair = true;    // PH_S2L_PAIR=0: always the one-window kernel for small_to_large
  bool bc_pair = true;     // PH_BC_PAIR=0: always the one-window kernel for best_correlation
  bool pair_chain = true;  // PH_PAIR_CHAIN=0: the window-pair kernels take the periods below 64 one pass each
  bool pair_cover = true;  // PH_PAIR_COVER=0: plain m_best screens every period instead of the top half (pair_screen_lo)
  bool pair_duo = true;    // PH_PAIR_DUO=0: the window-pair m_best screen folds every period in a pass of its own
  bool pair_fold_once = true;  // PH_PAIR_FOLD_ONCE=0: k_mbest_step1_pair stages, thins and evaluates every window-sweep as before the fold-once path
  bool pair_fold_report = false;  // PH_PAIR_FOLD_REPORT=1 (tests): n_sweeps carries the window's fold-once count above bit 16
  bool step2_geom = true;  // PH_STEP2_GEOM=0: k_mbest_step2 rebuilds each factor's fold geometry instead of reading the table's
  DevBuf twid;  // cos/sin(2 pi k / L), k < L, of the last best_frequency win_size
  int twid_len = -1;
  DevBuf bs_tab;  // Bluestein tables of the last (win_size, min(N, win_size)): M twiddles, chirp, FFT of the wrapped chirp
  int bs_L = -1, bs_M0 = -1;
  DevBuf plan;  // pass plan of the norm sweeps, cached for the last (p_lo, p_hi)
  int plan_lo = -1, plan_hi = -1, plan_n = 0, plan_m = -1, plan_duo_n = 0;
  int plan_max_m = 4;  // largest row-class count a pass may use (PH_PLAN_MAX_M overrides: 1, 2 or 4)
  int sweep_block = ph::kBlockWide;  // threads per workgroup of the sweep kernels (PH_SWEEP_BLOCK overrides)
  int step1_block = 0;               // k_mbest_step1 only: 0 = automatic (PH_STEP1_BLOCK overrides, <= 1024)
  int qo_block = 1024;               // k_qo_find threads per workgroup (PH_QO_BLOCK overrides)
  int s2l_block = 1024;              // k_small_to_large_pair threads per workgroup (PH_S2L_BLOCK overrides, >= 512)
  bool qo_hbm_window = false;        // PH_QO_HBM_WINDOW=1: keep the residual of k_qo_find in HBM even when it fits LDS
  bool hbm_window = false;           // PH_HBM_WINDOW=1: every window and second window-sized buffer in HBM
  int path_tile_cap = 0;             // PH_PATH_TILE_ROWS=n: k_period_path's backtrace tile holds at most n rows (0: what fits)
  // Moebius tables of the orthogonal powers for the last max_p (prepare_mobius)
  int mob_max_p = -1;
  std::vector<int32_t> mob_off, mob_d, mob_mu;
  // optional per-kernel HIP-event timing (ph_profile_*)
  bool prof_on = false;
  int prof_n = 0;
  std::vector<hipEvent_t> prof_ev;  // 2 events per recorded launch
  std::vector<const char*> prof_name;
};

namespace {

int ensure(ph_ctx* c, DevBuf& b, size_t bytes) {
  if (bytes <= b.cap && b.p) return PH_OK;
  if (b.p) {
    PH_HIP(hipStreamSynchronize(c->stream));
    PH_HIP(hipFree(b.p));
    b.p = nullptr;
    b.cap = 0;
  }
  const size_t want = std::max<size_t>(bytes, 256);
  PH_HIP(hipMalloc(&b.p, want));
  b.cap = want;
  return PH_OK;
}

// Upload a small int table (host pointer) into a cached device slot.
int upload_table(ph_ctx* c, int slot, const int32_t* src, size_t n, const int** dev_out) {
  TableSlot& t = c->tab[slot];
  if (n == 0) {
    PH_TRY(ensure(c, t.dev, 16));
    *dev_out = static_cast<const int*>(t.dev.p);
    return PH_OK;
  }
  if (t.valid && t.host.size() == n && std::memcmp(t.host.data(), src, n * sizeof(int32_t)) == 0) {
    *dev_out = static_cast<const int*>(t.dev.p);
    return PH_OK;
  }
  t.valid = false;
  // the previous content may still be in use by queued kernels
  PH_HIP(hipStreamSynchronize(c->stream));
  PH_TRY(ensure(c, t.dev, n * sizeof(int32_t) + 256));  // 64 readable words behind the table (wave-wide list reads)
  t.host.assign(src, src + n);
  PH_HIP(hipMemcpyAsync(t.dev.p, t.host.data(), n * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
  PH_HIP(hipStreamSynchronize(c->stream));
  t.valid = true;
  *dev_out = static_cast<const int*>(t.dev.p);
  return PH_OK;
}

size_t elem_size(int dtype) { return dtype == PH_F64 ? 8 : 4; }

// Pass plan of a norm sweep over [p_lo, p_hi]: every period is produced exactly once, either
// by its own pass or as 2p / 4p of a smaller base period (see PassPlan in ph_device.h).
// Periods below 64 use the row-split path one at a time (m = 0).
// `chains` (window-pair kernels): the periods up to 64 are taken in chains L, L/2, L/4, ... -- one row-split pass at
// L yields them all (m = 8 + number of periods, see pair_chain_small in ph_pair.h) -- instead of one pass each.
// `duo_n` (k_mbest_step1_pair only; the window length, 0 = off): a single pass at p with R = 3 ... 6 rows and more than R
// chunk columns (p > 64 R) also takes p + 64 when that period has the same row count and no pass of its own yet (m = 3,
// pair_pass_duo in ph_pair.h) -- greedy in ascending order, so the pairing stays inside one row class; what finds no
// partner stays m = 1.
std::vector<ph::PassPlan> build_plan(int p_lo, int p_hi, int max_m, bool mixed = true, bool chains = false, int duo_n = 0) {
  std::vector<ph::PassPlan> host;
  std::vector<char> covered((size_t)p_hi + 1, 0);
  if (chains) {
    for (int L = std::min(p_hi, 64); L >= p_lo; --L) {
      if (covered[L]) continue;
      int n = 0;
      for (int q = L; q >= p_lo && q >= 1 && !covered[q]; q >>= 1) {
        covered[q] = 1;
        n += 1;
        if (q & 1) break;
      }
      host.push_back(ph::PassPlan{L, 8 + n});
    }
    std::reverse(host.begin(), host.end());
  }
  for (int p = p_lo; p <= p_hi; ++p) {
    if (p < 64 && !chains) {
      host.push_back(ph::PassPlan{p, 0});
      continue;
    }
    if (covered[p]) continue;
    int m = (4LL * p <= p_hi) ? 4 : (2LL * p <= p_hi) ? 2 : 1;
    m = std::min(m, max_m);
    for (int d = 1; d <= m; d *= 2) covered[(size_t)d * p] = 1;
    if (duo_n > 0 && m == 1 && p >= 64 && p + 64 <= p_hi && !covered[p + 64]) {
      const int rows = (duo_n + p - 1) / p;
      if (rows >= 3 && rows <= 6 && (p + 63) / 64 > rows && (duo_n + p + 63) / (p + 64) == rows) {
        covered[p + 64] = 1;
        m = 3;
      }
    }
    host.push_back(ph::PassPlan{p, m});
  }
  // Interleave the pass types evenly (entry i of a type with n entries gets the key (i + 0.5) / n):
  // the waves of a CU walk the plan in step, and a mix of LDS-heavy single passes and VALU-heavy
  // multi-class passes overlaps better than a phase of each.
  if (mixed && !std::getenv("PH_PLAN_SORTED")) {
    int count[5] = {0, 0, 0, 0, 0}, seen[5] = {0, 0, 0, 0, 0};
    for (const auto& e : host) count[e.m >= 8 ? 0 : e.m] += 1;
    std::vector<std::pair<double, size_t>> key(host.size());
    for (size_t i = 0; i < host.size(); ++i) {
      const int m = host[i].m >= 8 ? 0 : host[i].m;
      key[i] = {(seen[m] + 0.5) / count[m], i};
      seen[m] += 1;
    }
    std::stable_sort(key.begin(), key.end());
    std::vector<ph::PassPlan> mixed(host.size());
    for (size_t i = 0; i < host.size(); ++i) mixed[i] = host[key[i].second];
    host.swap(mixed);
  }
  if (const char* only = std::getenv("PH_PLAN_ONLY_M")) {  // profiling aid: keep one pass type (results incomplete)
    const int want = std::atoi(only);
    std::vector<ph::PassPlan> kept;
    for (const auto& e : host)
      if (e.m == want) kept.push_back(e);
    host.swap(kept);
  }
  return host;
}

// `mixed`: interleave the pass types (kernels whose workgroups split the plan in chunks: a mix of LDS-heavy
// and VALU-heavy passes overlaps better); otherwise ascending base period, i.e. the expensive multi-class
// passes first and the cheap few-row singles last -- what a workgroup that walks the WHOLE plan between two
// barriers wants (k_mbest_step1: shorter tail before the argmax barrier, -3 %).
int prepare_plan(ph_ctx* c, int p_lo, int p_hi, const ph::PassPlan** out, int* n_pass, int max_m = 4, bool mixed = true,
                 bool chains = false, int duo_n = 0) {
  max_m = std::min(max_m, c->plan_max_m);
  chains = chains && c->pair_chain;
  if (!c->pair_duo) duo_n = 0;
  if (!mixed) max_m += 8;  // cache key
  if (chains) max_m += 16;
  if (c->plan.p && c->plan_lo == p_lo && c->plan_hi == p_hi && c->plan_m == max_m && c->plan_duo_n == duo_n) {
    *out = static_cast<const ph::PassPlan*>(c->plan.p);
    *n_pass = c->plan_n;
    return PH_OK;
  }
  const std::vector<ph::PassPlan> host = build_plan(p_lo, p_hi, max_m & 7, mixed, chains, duo_n);
  PH_HIP(hipStreamSynchronize(c->stream));
  PH_TRY(ensure(c, c->plan, std::max<size_t>(1, host.size()) * sizeof(ph::PassPlan)));
  if (!host.empty())
    PH_HIP(hipMemcpyAsync(c->plan.p, host.data(), host.size() * sizeof(ph::PassPlan), hipMemcpyHostToDevice,
                          c->stream));
  PH_HIP(hipStreamSynchronize(c->stream));
  c->plan_lo = p_lo;
  c->plan_hi = p_hi;
  c->plan_m = max_m;
  c->plan_duo_n = duo_n;
  c->plan_n = (int)host.size();
  *out = static_cast<const ph::PassPlan*>(c->plan.p);
  *n_pass = c->plan_n;
  return PH_OK;
}

// Radius of the window-pair screen per period, in units of the sum of squares: radq[q] = pair_radius(ceil(N / q), q),
// the bound ph_pair.h proves (k_mbest_step1_pair reads it in its survivor scan instead of estimating the row count).
std::vector<double> pair_radius_table(int N, int max_p) {
  std::vector<double> host((size_t)max_p + 1, 0.0);
  for (int q = 1; q <= max_p; ++q) host[q] = ph::pair_radius((N + q - 1) / q, q);
  return host;
}

// Dense table geom[p], p in [0, max_p]: rows, nfull and the reciprocal counts of period p.
int prepare_geom(ph_ctx* c, int N, int max_p, const ph::PGeom** out) {
  if (c->geom.p && c->geom_n == N && c->geom_max_p >= max_p) {
    *out = static_cast<const ph::PGeom*>(c->geom.p);
    return PH_OK;
  }
  std::vector<ph::PGeom> host((size_t)max_p + 1);
  host[0] = ph::PGeom{0, 0, 0.0, 0.0};
  for (int p = 1; p <= max_p; ++p) {
    const int rows = (N + p - 1) / p;
    const int shortn = rows * p - N;
    host[p] = ph::PGeom{rows, p - shortn, 1.0 / rows, rows > 1 ? 1.0 / (rows - 1) : 0.0};
  }
  PH_HIP(hipStreamSynchronize(c->stream));
  PH_TRY(ensure(c, c->geom, host.size() * sizeof(ph::PGeom)));
  PH_HIP(hipMemcpyAsync(c->geom.p, host.data(), host.size() * sizeof(ph::PGeom), hipMemcpyHostToDevice, c->stream));
  std::vector<ph::PGeomF> hostf(host.size());
  for (size_t p = 0; p < host.size(); ++p)
    hostf[p] = ph::PGeomF{host[p].rows, host[p].nfull, (float)host[p].w_full, (float)host[p].w_short};
  PH_TRY(ensure(c, c->geomf, hostf.size() * sizeof(ph::PGeomF)));
  PH_HIP(hipMemcpyAsync(c->geomf.p, hostf.data(), hostf.size() * sizeof(ph::PGeomF), hipMemcpyHostToDevice, c->stream));
  const std::vector<double> hostr = pair_radius_table(N, max_p);
  PH_TRY(ensure(c, c->radq, hostr.size() * sizeof(double)));
  PH_HIP(hipMemcpyAsync(c->radq.p, hostr.data(), hostr.size() * sizeof(double), hipMemcpyHostToDevice, c->stream));
  std::vector<float> hostk(host.size(), 0.0f);
  for (size_t p = 1; p < host.size(); ++p) {
    const double k = ph::s2l_kappa(N, host[p].rows, (int)p);
    float f = (float)k;
    if ((double)f < k) f = std::nextafterf(f, INFINITY);
    hostk[p] = f;
  }
  PH_TRY(ensure(c, c->kapf, hostk.size() * sizeof(float)));
  PH_HIP(hipMemcpyAsync(c->kapf.p, hostk.data(), hostk.size() * sizeof(float), hipMemcpyHostToDevice, c->stream));
  PH_HIP(hipStreamSynchronize(c->stream));
  c->geom_n = N;
  c->geom_max_p = max_p;
  *out = static_cast<const ph::PGeom*>(c->geom.p);
  return PH_OK;
}

int check_common(ph_ctx* c, const void* x, int dtype, int64_t W, int N) {
  if (!c) return fail(PH_E_ARG, "ctx is NULL");
  if (!x) return fail(PH_E_ARG, "x is NULL");
  if (dtype != PH_F64 && dtype != PH_F32) return fail(PH_E_ARG, "dtype must be PH_F64 or PH_F32");
  if (W < 1 || W > 0x7fffffffLL / 64) return fail(PH_E_ARG, "W=%lld out of range", (long long)W);
  if (N < 1) return fail(PH_E_ARG, "N=%d must be >= 1", N);
  return PH_OK;
}

int check_lds(const ph_ctx* c, size_t bytes, int N, const char* what) {
  if (bytes > (size_t)c->lds_limit)
    return fail(PH_E_ARG, "%s: window of N=%d needs %zu B of LDS, device limit is %d B", what, N, bytes,
                c->lds_limit);
  return PH_OK;
}

// f(T{}) for the runtime element type.
template <typename F>
int dispatch(int dtype, F&& f) {
  return dtype == PH_F64 ? f(double{}) : f(float{});
}

// f(T{}, std::bool_constant<window in LDS>{}) for the runtime element type / window placement.
template <typename F>
int dispatch(int dtype, bool lds_window, F&& f) {
  if (dtype == PH_F64) return lds_window ? f(double{}, std::true_type{}) : f(double{}, std::false_type{});
  return lds_window ? f(float{}, std::true_type{}) : f(float{}, std::false_type{});
}

template <typename K>
int allow_lds(K kernel, size_t bytes) {
  if (bytes > 48 * 1024) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
    if (e != hipSuccess) return fail(PH_E_HIP, "hipFuncSetAttribute(LDS=%zu): %s", bytes, hipGetErrorString(e));
  }
  return PH_OK;
}

constexpr int kProfCap = 256;

// Brackets one kernel launch with HIP events on the context's stream when profiling is on.
struct ProfScope {
  ph_ctx* c;
  bool live;
  ProfScope(ph_ctx* ctx, const char* name) : c(ctx), live(ctx->prof_on && ctx->prof_n < kProfCap) {
    if (!live) return;
    if ((int)c->prof_ev.size() < 2 * (c->prof_n + 1)) {
      hipEvent_t a = nullptr, b = nullptr;
      if (hipEventCreate(&a) != hipSuccess || hipEventCreate(&b) != hipSuccess) {
        live = false;
        return;
      }
      c->prof_ev.push_back(a);
      c->prof_ev.push_back(b);
      c->prof_name.push_back(name);
    }
    c->prof_name[c->prof_n] = name;
    (void)hipEventRecord(c->prof_ev[2 * c->prof_n], c->stream);
  }
  ~ProfScope() {
    if (!live) return;
    (void)hipEventRecord(c->prof_ev[2 * c->prof_n + 1], c->stream);
    c->prof_n += 1;
  }
};

int launch_check(const char* what) {
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(PH_E_HIP, "launch of %s failed: %s", what, hipGetErrorString(e));
  return PH_OK;
}

// One kernel launch on the context's stream, its profile bracket around the launch alone; a failure is reported under
// `name`, the kernel that was launched.  The kernel's LDS limit must already allow `lds` (launch does both).
template <typename K, typename... A>
int enqueue(ph_ctx* c, const char* name, K kernel, dim3 grid, int block, size_t lds, A... args) {
  {
    ProfScope ps_(c, name);
    hipLaunchKernelGGL(kernel, grid, dim3(block), lds, c->stream, args...);
  }
  return launch_check(name);
}

// The launch sequence of every kernel: raise its LDS limit to `lds`, then enqueue.  (ph_best_frequency raises the
// limits of its kernels once and enqueues them `num` times.)
template <typename K, typename... A>
int launch(ph_ctx* c, const char* name, K kernel, dim3 grid, int block, size_t lds, A... args) {
  PH_TRY(allow_lds(kernel, lds));
  return enqueue(c, name, kernel, grid, block, lds, args...);
}

// Orth tables (only when PH_FLAG_ORTH) and validation of their content.
int prepare_orth(ph_ctx* c, unsigned flags, const int32_t* off, const int32_t* q, int table_max_p, int need_p,
                 ph::Tables* tb) {
  tb->orth_off = tb->orth_q = nullptr;
  if (!(flags & PH_FLAG_ORTH)) return PH_OK;
  if (!off || !q) return fail(PH_E_ARG, "PH_FLAG_ORTH needs orth_off/orth_q tables");
  if (table_max_p < need_p) return fail(PH_E_ARG, "orth tables cover p <= %d, need %d", table_max_p, need_p);
  const size_t n_off = (size_t)table_max_p + 2;
  if (off[0] != 0) return fail(PH_E_ARG, "orth_off[0] must be 0");
  for (size_t i = 0; i + 1 < n_off; ++i)
    if (off[i + 1] < off[i]) return fail(PH_E_ARG, "orth_off not monotone at %zu", i);
  const size_t n_q = (size_t)off[n_off - 1];
  for (size_t i = 0; i < n_q; ++i)
    if (q[i] < 1) return fail(PH_E_ARG, "orth_q[%zu]=%d must be >= 1", i, q[i]);
  PH_TRY(upload_table(c, T_ORTH_OFF, off, n_off, &tb->orth_off));
  PH_TRY(upload_table(c, T_ORTH_Q, q, n_q, &tb->orth_q));
  return PH_OK;
}

int prepare_fac(ph_ctx* c, const int32_t* off, const int32_t* q, int table_max_p, int need_p, ph::Tables* tb) {
  if (!off || !q) return fail(PH_E_ARG, "fac_off/fac_q tables are required");
  if (table_max_p < need_p) return fail(PH_E_ARG, "factor tables cover p <= %d, need %d", table_max_p, need_p);
  const size_t n_off = (size_t)table_max_p + 2;
  if (off[0] != 0) return fail(PH_E_ARG, "fac_off[0] must be 0");
  for (size_t i = 0; i + 1 < n_off; ++i)
    if (off[i + 1] < off[i]) return fail(PH_E_ARG, "fac_off not monotone at %zu", i);
  const size_t n_q = (size_t)off[n_off - 1];
  for (size_t i = 0; i < n_q; ++i)
    if (q[i] < 1 || q[i] > table_max_p) return fail(PH_E_ARG, "fac_q[%zu]=%d out of range", i, q[i]);
  PH_TRY(upload_table(c, T_FAC_OFF, off, n_off, &tb->fac_off));
  PH_TRY(upload_table(c, T_FAC_Q, q, n_q, &tb->fac_q));
  return PH_OK;
}

// Host-pointer staging: `Stage` maps each user array to the pointer the kernel uses.
struct Stage {
  ph_ctx* c;
  bool device;
  struct Out {
    void* user;
    void* dev;
    size_t bytes;
  };
  std::vector<Out> outs;
  Stage(ph_ctx* ctx, unsigned flags) : c(ctx), device(flags & PH_FLAG_DEVICE) {}
  int in(const void* user, size_t bytes, const void** dev, int slot = B_IN) {
    if (device) {
      *dev = user;
      return PH_OK;
    }
    PH_TRY(ensure(c, c->buf[slot], bytes));
    PH_HIP(hipMemcpyAsync(c->buf[slot].p, user, bytes, hipMemcpyHostToDevice, c->stream));
    *dev = c->buf[slot].p;
    return PH_OK;
  }
  int out(int slot, void* user, size_t bytes, void** dev) {
    if (!user) {
      *dev = nullptr;
      return PH_OK;
    }
    if (device) {
      *dev = user;
      return PH_OK;
    }
    PH_TRY(ensure(c, c->buf[slot], bytes));
    *dev = c->buf[slot].p;
    outs.push_back({user, *dev, bytes});
    return PH_OK;
  }
  int finish() {
    if (device) return PH_OK;
    for (const Out& o : outs)
      PH_HIP(hipMemcpyAsync(o.user, o.dev, o.bytes, hipMemcpyDeviceToHost, c->stream));
    PH_HIP(hipStreamSynchronize(c->stream));
    return PH_OK;
  }
};

int pick_chunks(ph_ctx* c, int64_t W, int items, int min_items_per_chunk) {
  const int64_t target = (int64_t)c->num_cu * 8;  // >= 8 workgroups per CU in flight/queued
  int64_t chunks = (target + W - 1) / W;
  const int64_t max_chunks = std::max(1, items / std::max(1, min_items_per_chunk));
  chunks = std::max<int64_t>(1, std::min(chunks, max_chunks));
  return (int)chunks;
}

using ph::carve_bytes;
using ph::CarveCount;
using ph::kBlock;
using ph::kBlockWide;
using ph::kPad;
using ph::kMaxWaves;
using ph::kRedDoubles;

// LDS bytes of a kernel whose carve depends on the element type: `carve(T())` runs the kernel's x_carve<T> on a
// CarveCount.
template <class F>
size_t lds_of(int dtype, F carve) {
  return dtype == PH_F64 ? carve(double()).bytes : carve(float()).bytes;
}

// LDS layout of k_qo_find: bookkeeping, the pair table, the weights, and the six work vectors + sample counts of the
// conjugate-gradient solve (one slot per dictionary row and one per block).  The residual window stays in LDS when
// it fits; the work vectors then OVERLAY it if it is large enough (the window is dead during a solve) -- 79 KB per
// workgroup for N = 16384 fp32 with kcap = 1024, two workgroups per CU -- and sit behind it otherwise.  Windows
// that do not fit (long fp64 windows) move to the HBM workspace and the sweeps read them through L2.
// *placement_out = PH_QO_LDS_OVERLAY, PH_QO_LDS_BEHIND or PH_QO_HBM.
int qo_lds_layout(ph_ctx* c, int dtype, int N, int max_length, int kcap, size_t* lds_out, int* placement_out) {
  struct Count {
    size_t bytes, window, solver;  // the layout, its window piece, its work vectors
  };
  const auto count = [&](bool lw, bool overlay) {
    const auto of = [&](auto t) {
      const auto L = ph::qo_find_carve<decltype(t)>(CarveCount(), N, max_length, kcap, lw, overlay);
      return Count{L.bytes, L.window, L.solver};
    };
    return dtype == PH_F64 ? of(double()) : of(float());
  };
  const size_t bare = count(false, false).bytes, limit = (size_t)c->lds_limit;
  if (bare > limit)
    return fail(PH_E_ARG, "ph_qo_find_periods: kcap=%d needs %zu B of LDS for the solver (limit %d B)", kcap, bare,
                c->lds_limit);
  const Count behind = count(true, false);
  const bool overlay = behind.window >= behind.solver;  // the vectors fit over the window
  const size_t with_window = overlay ? count(true, true).bytes : behind.bytes;
  const bool lds_window = !c->qo_hbm_window && with_window <= limit;
  *lds_out = lds_window ? with_window : bare;
  *placement_out = !lds_window ? PH_QO_HBM : overlay ? PH_QO_LDS_OVERLAY : PH_QO_LDS_BEHIND;
  return PH_OK;
}

// LDS layout of k_qo_greedy: the residual window (or nothing: the HBM workspace holds it) and the reductions.  The
// divisor bitset lives in the HBM workspace and the block's weights in the output row, so the LDS need does not depend
// on max_length or kcap, and every N and max_length is feasible.  A window in LDS counts as PH_QO_LDS_BEHIND (there
// are no work vectors to overlay it).
void qo_greedy_layout(const ph_ctx* c, int dtype, int N, size_t* lds_out, int* placement_out) {
  const auto lds = [&](bool lw) {
    return lds_of(dtype, [&](auto t) { return ph::qo_greedy_carve<decltype(t)>(CarveCount(), N, lw); });
  };
  const bool lds_window = !c->qo_hbm_window && lds(true) <= (size_t)c->lds_limit;
  *lds_out = lds(lds_window);
  *placement_out = lds_window ? PH_QO_LDS_BEHIND : PH_QO_HBM;
}

// Argument checks and layout of ph_qo_find_periods, shared by the launch and ph_qo_plan_info.  max_length < 0 means
// N / 3 (QOPeriods.py:374-375); *max_length_io receives the value used.
int qo_plan(ph_ctx* c, int dtype, int N, int* max_length_io, int kcap, unsigned flags, size_t* lds_out,
            int* placement_out) {
  if (flags & PH_FLAG_ORTH)
    return fail(PH_E_UNSUPPORTED, "ph_qo_find_periods: orthogonal selection is not implemented on the device");
  const bool keep_weights = flags & PH_FLAG_KEEP_WEIGHTS;
  if (*max_length_io < 0) *max_length_io = N / 3;
  if (!keep_weights && (kcap < 1 || kcap > 2048)) return fail(PH_E_ARG, "kcap=%d must be in [1, 2048]", kcap);
  if (keep_weights && (kcap < 1 || kcap > ph::kQoGreedyMaxRows))
    return fail(PH_E_ARG, "kcap=%d must be in [1, %d] with PH_FLAG_KEEP_WEIGHTS", kcap, ph::kQoGreedyMaxRows);
  if (keep_weights) {
    qo_greedy_layout(c, dtype, N, lds_out, placement_out);
    return PH_OK;
  }
  return qo_lds_layout(c, dtype, N, *max_length_io, kcap, lds_out, placement_out);
}

size_t pair_lds_bytes(int N, int num, int P) { return ph::step1_pair_carve(CarveCount(), N, num, P).bytes; }

// The window-pair screen serves fp64 windows, plain projection, candidate periods below N, when the pair window
// and the staging buffer fit the LDS; everything else runs k_mbest_step1.
bool pair_eligible(const ph_ctx* c, int dtype, int N, int num, int min_length, int max_length, unsigned flags) {
  const bool general = flags & (PH_FLAG_TRUNC | PH_FLAG_ORTH);
  return c->step1_pair && dtype == PH_F64 && !general && max_length < N && min_length <= max_length &&
         pair_lds_bytes(N, num, max_length - min_length + 1) <= (size_t)c->lds_limit;
}

// First period the window-pair screen of m_best evaluates.  Plain m_best (gamma == 0): a period with a multiple in range
// cannot beat that multiple (cover rule, ph_pair.h), so the screen starts behind max_length / 2 and the kernel looks at
// a smaller period only when one of its multiples survives.  m_best_gamma compares E_q / q, which the rule does not
// order: it screens every period, and so does PH_PAIR_COVER=0.  A result equal to min_length means "no cover logic".
int pair_screen_lo(const ph_ctx* c, int min_length, int max_length, int gamma) {
  return (c->pair_cover && !gamma) ? std::max(min_length, max_length / 2 + 1) : min_length;
}

// ----------------------------------------------------------------------------- launch plans
// One planning function per entry point: the variant, the placement of the window and of the second window-sized
// buffer, the block size and the LDS of every kernel it launches, from the arguments alone (nothing is allocated or
// launched).  The launcher and ph_plan_info both call it; the launcher only allocates the workspaces the plan names.
struct KernelPlan {
  int variant = PH_PLAN_ONE;
  int window = PH_PLAN_LDS;
  int second = PH_PLAN_NONE;
  int block = 0;
  size_t lds = 0;
  int small_means = 0;
  int waves = 0;
  int pad = 0;
};

struct Plan {
  int n_kernels = 1;
  KernelPlan k[2];
};

// Placement of the window buffer and of the second window-sized buffer (materialised projections) of one kernel.
// `lds(window_in_lds, second_in_lds)` counts the kernel's carve.  Everything in LDS when it fits; otherwise the second
// buffer moves to an HBM workspace, and then the window (the kernels' <T, false> instantiations fold it through L2).
template <class F>
void plan_buffers(const ph_ctx* c, KernelPlan* k, bool second_needed, F lds) {
  const auto fits = [&](bool lw, bool second) { return !c->hbm_window && lds(lw, second) <= (size_t)c->lds_limit; };
  k->second = !second_needed ? PH_PLAN_NONE : fits(true, true) ? PH_PLAN_LDS : PH_PLAN_HBM;
  k->window = fits(true, k->second == PH_PLAN_LDS) ? PH_PLAN_LDS : PH_PLAN_HBM;
  k->lds = lds(k->window == PH_PLAN_LDS, k->second == PH_PLAN_LDS);
}

// The HBM workspace (slot, `bytes`) of a buffer the plan put there; nullptr when it stays in LDS or is not needed.
int place(ph_ctx* c, int where, int slot, size_t bytes, void** p) {
  *p = nullptr;
  if (where != PH_PLAN_HBM) return PH_OK;
  PH_TRY(ensure(c, c->buf[slot], bytes));
  *p = c->buf[slot].p;
  return PH_OK;
}

// k_project_batch: window + projection scratch (min(p_max, N), N with PH_FLAG_ORTH).
int plan_project(const ph_ctx* c, int dtype, int N, int pmax, unsigned flags, Plan* pl, int* scratch_len) {
  KernelPlan& k = pl->k[0];
  *scratch_len = (flags & PH_FLAG_ORTH) ? N : std::min(pmax, N);
  plan_buffers(c, &k, true, [&](bool lw, bool second) {
    return lds_of(dtype,
                  [&](auto t) { return ph::project_carve<decltype(t)>(CarveCount(), N, *scratch_len, lw, second); });
  });
  k.block = kBlock;
  return check_lds(c, k.lds, N, "ph_project_batch");
}

// k_sweep: the norm modes with trunc / orth materialise the projection in a second buffer.
int plan_sweep(const ph_ctx* c, int dtype, int N, int mode, unsigned flags, Plan* pl) {
  KernelPlan& k = pl->k[0];
  const bool general = (flags & (PH_FLAG_TRUNC | PH_FLAG_ORTH)) && mode != PH_SWEEP_MAXABS;
  const auto lds = [&](bool lw, bool second) {
    return dtype == PH_F64 ? ph::sweep_lds_bytes<double>(N, lw, general && second)
                           : ph::sweep_lds_bytes<float>(N, lw, general && second);
  };
  // long windows (at most two workgroups per CU): 16 wavefronts per workgroup
  k.block = (3 * lds(true, true) > (size_t)c->lds_limit && c->sweep_block == ph::kBlockWide) ? 1024 : c->sweep_block;
  plan_buffers(c, &k, general, lds);
  return check_lds(c, k.lds, N, "ph_sweep");
}

// m_best: k[0] = step 1 (k_mbest_step1 or the window-pair screen k_mbest_step1_pair), k[1] = step 2.  max_fac = most
// proper divisors any candidate period has (PGeom / divisor slots of step 2).
int plan_m_best(const ph_ctx* c, int dtype, int N, int num, int min_length, int max_length, int max_fac, unsigned flags,
                Plan* pl) {
  const bool general = flags & (PH_FLAG_TRUNC | PH_FLAG_ORTH);
  const int P = max_length - min_length + 1;
  KernelPlan& s1 = pl->k[0];
  KernelPlan& s2 = pl->k[1];
  pl->n_kernels = 2;
  const auto lds1 = [&](bool lw, bool second, bool small_means) {
    return dtype == PH_F64 ? ph::step1_lds_bytes<double>(N, num, P, lw, general && second, small_means)
                           : ph::step1_lds_bytes<float>(N, num, P, lw, general && second, small_means);
  };
  const auto lds2 = [&](bool lw, bool second) {
    return lds_of(dtype,
                  [&](auto t) { return ph::step2_carve<decltype(t)>(CarveCount(), N, num, max_fac, lw, second); });
  };
  // LDS for the means of a short winning period (split_row_means): only when the window stays in LDS beside it
  s1.small_means = (!general && !c->hbm_window && lds1(true, false, true) <= (size_t)c->lds_limit) ? 1 : 0;
  plan_buffers(c, &s1, general, [&](bool lw, bool second) { return lds1(lw, second, s1.small_means); });
  // step 2 materialises a projection only when a row is split (rare) or in the trunc/orth modes:
  // in plain mode that buffer always lives in the HBM workspace, which lets four workgroups of
  // eight wavefronts share a CU instead of two of four
  if (general) {
    plan_buffers(c, &s2, true, lds2);
  } else {
    plan_buffers(c, &s2, false, lds2);
    s2.second = PH_PLAN_HBM;
  }
  PH_TRY(check_lds(c, std::max(s1.lds, s2.lds), N, "ph_m_best"));
  // Window-pair screen (k_mbest_step1_pair): fp64 windows, plain projection, candidate periods below N, and room for
  // the pair window plus one fp64 staging buffer in LDS.
  const bool pair = pair_eligible(c, dtype, N, num, min_length, max_length, flags) && s1.window == PH_PLAN_LDS &&
                    s2.window == PH_PLAN_LDS;
  if (pair) {
    s1.variant = PH_PLAN_PAIR;
    s1.lds = pair_lds_bytes(N, num, P);
    s1.block = ph::kPairWaves * ph::kWave;  // the kernel is compiled for this block and no other
    s1.small_means = 0;  // the pair kernel keeps its own short-period means (kPairSmallP)
  } else {
    // 16 wavefronts per window: two workgroups per CU at N = 4096 (-2.4 % against four of 8 waves),
    // and long windows, which leave room for one or two workgroups per CU, still fill the SIMDs
    // (N = 8192: -15 %, N = 16384: -23 %)
    // (short windows, N < 3072, keep 8: four workgroups per CU there)
    s1.block = c->step1_block ? c->step1_block : (c->sweep_block == ph::kBlockWide && N >= 3072) ? 1024 : c->sweep_block;
  }
  s2.block = general ? kBlock : c->sweep_block;
  return PH_OK;
}

// small_to_large: k_small_to_large or the persistent window-pair screen k_small_to_large_pair.
int plan_small_to_large(const ph_ctx* c, int dtype, int N, int n_periods, unsigned flags, Plan* pl) {
  const bool general = flags & (PH_FLAG_TRUNC | PH_FLAG_ORTH);
  KernelPlan& k = pl->k[0];
  plan_buffers(c, &k, general, [&](bool lw, bool second) {
    return lds_of(dtype,
                  [&](auto t) { return ph::s2l_carve<decltype(t)>(CarveCount(), N, general, lw, general && second); });
  });
  PH_TRY(check_lds(c, k.lds, N, "ph_small_to_large"));
  // Window-pair screen (ph_s2l.h): fp64 windows, plain projection, candidate periods below N.  LDS: the pair window and
  // one fp64 staging buffer, two 16-wave workgroups per CU; the fp64 residuals live in an HBM workspace.
  const size_t lds_pair = ph::s2l_pair_lds_bytes(N);
  const bool pair = c->s2l_pair && dtype == PH_F64 && !general && k.window == PH_PLAN_LDS && n_periods < N &&
                    n_periods >= 2 && c->sweep_block >= 512 && lds_pair <= (size_t)c->lds_limit;
  k.variant = pair ? PH_PLAN_PAIR : PH_PLAN_ONE;
  k.block = pair ? c->s2l_block : c->sweep_block;
  if (pair) k.lds = lds_pair;
  return PH_OK;
}

// best_correlation: k_best_correlation or the window-pair screen k_best_correlation_pair.
int plan_best_correlation(const ph_ctx* c, int dtype, int N, int max_length, unsigned flags, Plan* pl) {
  const bool general = flags & (PH_FLAG_TRUNC | PH_FLAG_ORTH);
  KernelPlan& k = pl->k[0];
  plan_buffers(c, &k, general, [&](bool lw, bool second) {
    return lds_of(dtype, [&](auto t) { return ph::bc_carve<decltype(t)>(CarveCount(), N, lw, general && second); });
  });
  PH_TRY(check_lds(c, k.lds, N, "ph_best_correlation"));
  // Window-pair screen (k_best_correlation_pair): fp64 windows, plain projection, pair window + staging buffer in LDS
  const size_t lds_pair = ph::bc_pair_carve(CarveCount(), N).bytes;
  const bool pair = c->bc_pair && dtype == PH_F64 && !general && k.window == PH_PLAN_LDS && max_length <= N &&
                    max_length - 1 >= 2 && lds_pair <= (size_t)c->lds_limit;
  k.variant = pair ? PH_PLAN_PAIR : PH_PLAN_ONE;
  k.block = pair ? ph::kPairWaves * ph::kWave : c->sweep_block;  // (the pair kernel is compiled for this block and no other)
  if (pair) k.lds = lds_pair;
  return PH_OK;
}

// best_frequency: k[0] = the spectrum (in-LDS FFT, Bluestein chirp or direct DFT), k[1] = k_bf_update.
struct BfShape {
  size_t lds_spec, lds_fft, lds_chirp;
  int logL, M0, M, logM, nchunk, wlen;
};

int plan_best_frequency(const ph_ctx* c, int dtype, int N, int L, Plan* pl, BfShape* g) {
  KernelPlan& s = pl->k[0];
  KernelPlan& u = pl->k[1];
  pl->n_kernels = 2;
  // windows longer than the LDS: both kernels work on the residual where it lives (HBM workspace)
  plan_buffers(c, &u, true, [&](bool lw, bool second) {
    return lds_of(dtype, [&](auto t) { return ph::bf_update_carve<decltype(t)>(CarveCount(), N, lw, second); });
  });
  PH_TRY(check_lds(c, u.lds, N, "ph_best_frequency"));
  u.block = kBlockWide;
  const auto lds_spectrum = [&](size_t stage_len, size_t n) {
    return lds_of(dtype, [&](auto t) { return ph::bf_spectrum_carve<decltype(t)>(CarveCount(), stage_len, n); });
  };
  g->lds_spec = lds_spectrum(u.window == PH_PLAN_LDS ? N : 0, 0);
  PH_TRY(check_lds(c, g->lds_spec, N, "ph_best_frequency"));
  // power-of-two win_size whose complex work array fits the LDS: in-LDS FFT, one record per window
  g->lds_fft = lds_spectrum(0, L);
  const bool use_fft = (L & (L - 1)) == 0 && L >= 4 && g->lds_fft <= (size_t)c->lds_limit && !std::getenv("PH_BF_DIRECT");
  g->logL = 0;
  while ((1 << g->logL) < L) ++g->logL;
  // any other win_size: Bluestein's chirp convolution on two FFTs of size M >= min(N, L) + L / 2 + 1, if that fits
  g->M0 = std::min(N, L);
  g->logM = 0;
  while ((1LL << g->logM) < (long long)g->M0 + L / 2 + 1) ++g->logM;
  g->M = 1 << g->logM;
  g->lds_chirp = lds_spectrum(0, g->M);
  const bool use_chirp =
      !use_fft && L >= 4 && g->logM <= 20 && g->lds_chirp <= (size_t)c->lds_limit && !std::getenv("PH_BF_DIRECT");
  g->nchunk = (use_fft || use_chirp) ? 1 : (L / 2 + 1 + ph::kBfBlock - 1) / ph::kBfBlock;
  g->wlen = std::max(g->M0, L / 2 + 1);  // chirp entries the kernel and the wrapped filter need
  s.variant = use_fft ? PH_PLAN_FFT : use_chirp ? PH_PLAN_CHIRP : PH_PLAN_DIRECT;
  s.window = (use_fft || use_chirp) ? PH_PLAN_HBM : u.window;
  s.lds = use_fft ? g->lds_fft : use_chirp ? g->lds_chirp : g->lds_spec;
  s.block = (use_fft || use_chirp) ? kBlockWide : ph::kBfBlock;
  return PH_OK;
}

// k_ramanujan: per wavefront strip A (q_hi doubles, the root fold) and strip B (q_hi / 2, one child).  As many
// wavefronts as the LDS left by the window allows, at most 16; when fewer than four fit beside an LDS-resident window
// (the reference's default range q_hi = N / 3 on a long window) the window moves to the HBM workspace and the strips
// get the whole LDS.
int plan_ramanujan(const ph_ctx* c, int dtype, int N, int q_hi, Plan* pl) {
  const size_t sz = elem_size(dtype);
  KernelPlan& k = pl->k[0];
  const auto lds = [&](int nw, int pad, bool lw) {
    return lds_of(dtype, [&](auto t) { return ph::ram_carve<decltype(t)>(CarveCount(), N, q_hi, nw, pad, lw); });
  };
  const size_t strip = lds(1, 0, false);  // strips A and B of one wavefront
  const size_t win_bytes = carve_bytes(N + kPad, sz);
  auto waves_for = [&](size_t room) { return (int)std::min<size_t>(ph::kRamMaxWaves, room / strip); };
  const size_t limit = (size_t)c->lds_limit;
  int nw = 0, pad = kPad;
  bool hbm = c->hbm_window;
  if (hbm) {
    nw = waves_for(limit);
  } else {
    nw = win_bytes < limit ? waves_for(limit - win_bytes) : 0;
    // The zeroed pad behind the window serves the row-split fold of roots below 64 (q_hi < 128) only; a fold of a root
    // >= 64 merely reads up to 255 elements past the window for lanes whose sums it discards.  Without the pad those
    // reads land in the strips -- and at config 3 window + 16 x 6 KB of strips are exactly the 160 KB of the CU.
    const size_t win_bare = carve_bytes(N, sz);
    if (q_hi >= 128 && nw >= 2 && nw < ph::kRamMaxWaves && waves_for(limit - win_bare) > nw) {
      nw = waves_for(limit - win_bare);
      pad = 0;
    }
    if (nw < 4) {
      const int nw_hbm = waves_for(limit);
      if (nw_hbm > nw) {
        nw = nw_hbm;
        pad = kPad;
        hbm = true;
      }
    }
  }
  if (nw < 1)
    return fail(PH_E_ARG, "ph_ramanujan_norms: q_hi=%d needs %zu B of LDS per wavefront, device limit is %d B", q_hi, strip,
                c->lds_limit);
  k.lds = lds(nw, pad, !hbm);
  PH_TRY(check_lds(c, k.lds, N, "ph_ramanujan_norms"));
  if (q_hi >= 30030 || q_hi > 0xffff) return fail(PH_E_ARG, "ph_ramanujan_norms: q_hi=%d is beyond the record format", q_hi);
  k.window = hbm ? PH_PLAN_HBM : PH_PLAN_LDS;
  k.waves = nw;
  k.pad = pad;
  k.block = nw * 64;
  return PH_OK;
}

// k_orth_powers: window + autocorrelation + clipped eq. 3 values in LDS when they fit, otherwise the window is read
// from HBM / L2 and the two work arrays live in an HBM workspace.
void plan_orth_powers(const ph_ctx* c, int dtype, int N, int max_p, Plan* pl) {
  KernelPlan& k = pl->k[0];
  const auto lds = [&](bool lw) {
    return lds_of(dtype, [&](auto t) { return ph::orth_carve<decltype(t)>(CarveCount(), N, max_p, lw, false); });
  };
  const bool lds_window = !c->hbm_window && lds(true) <= (size_t)c->lds_limit;
  k.lds = lds(lds_window);
  k.window = k.second = lds_window ? PH_PLAN_LDS : PH_PLAN_HBM;
  k.block = kBlockWide;
}

// k_qo_orth_select: k_orth_powers' placement rule on its own layout (the same three arrays + the reduction slots; the
// projection reuses the autocorrelation's N doubles, so nothing is added for it).
int plan_qo_orth_select(const ph_ctx* c, int dtype, int N, int max_p, Plan* pl) {
  if (max_p < 2) return fail(PH_E_ARG, "ph_qo_orth_select: max_p=%d must be >= 2", max_p);
  KernelPlan& k = pl->k[0];
  const auto lds = [&](bool lw) {
    return lds_of(dtype, [&](auto t) { return ph::orth_carve<decltype(t)>(CarveCount(), N, max_p, lw, true); });
  };
  const bool lds_window = !c->hbm_window && lds(true) <= (size_t)c->lds_limit;
  k.lds = lds(lds_window);
  k.window = k.second = lds_window ? PH_PLAN_LDS : PH_PLAN_HBM;
  k.block = kBlockWide;
  return PH_OK;
}

// Divisors d of q with mu(q / d) != 0 in ascending order, CSR by q < max_p, and mu(q / d): the Moebius sum of the
// orthogonal powers (QOPeriods.py:1210-1217).  Kept for the last max_p; upload_table skips the copy of unchanged content.
int prepare_mobius(ph_ctx* c, int max_p, const int** d_off, const int** d_d, const int** d_mu) {
  if (c->mob_max_p != max_p) {
    std::vector<int32_t> mu(max_p, 1), &off = c->mob_off, &dd = c->mob_d, &dm = c->mob_mu;
    c->mob_max_p = -1;
    std::vector<char> comp(max_p, 0);
    for (int i = 2; i < max_p; ++i) {
      if (comp[i]) continue;
      for (int j = i; j < max_p; j += i) {
        comp[j] = j > i;
        mu[j] = -mu[j];
      }
      for (int64_t j = (int64_t)i * i; j < max_p; j += (int64_t)i * i) mu[j] = 0;
    }
    off.assign((size_t)max_p + 1, 0);
    for (int d = 1; d < max_p; ++d)
      for (int q = d; q < max_p; q += d)
        if (mu[q / d] != 0) ++off[q + 1];
    for (int q = 0; q < max_p; ++q) off[q + 1] += off[q];
    dd.assign((size_t)off[max_p], 0);
    dm.assign((size_t)off[max_p], 0);
    std::vector<int32_t> fill(off.begin(), off.end() - 1);
    for (int d = 1; d < max_p; ++d)
      for (int q = d; q < max_p; q += d)
        if (mu[q / d] != 0) {
          dd[fill[q]] = d;
          dm[fill[q]++] = mu[q / d];
        }
    c->mob_max_p = max_p;
  }
  PH_TRY(upload_table(c, T_AUX0, c->mob_off.data(), c->mob_off.size(), d_off));
  PH_TRY(upload_table(c, T_AUX1, c->mob_d.data(), c->mob_d.size(), d_d));
  PH_TRY(upload_table(c, T_AUX2, c->mob_mu.data(), c->mob_mu.size(), d_mu));
  return PH_OK;
}

// k_fold_sums: longer windows are folded from HBM / L2.
void plan_fold_sums(const ph_ctx* c, int dtype, int N, Plan* pl) {
  KernelPlan& k = pl->k[0];
  const size_t staged = lds_of(dtype, [&](auto t) { return ph::stage_carve<decltype(t)>(CarveCount(), N); });
  const bool lds_window = !c->hbm_window && staged <= (size_t)c->lds_limit;
  k.lds = lds_window ? staged : 0;
  k.window = lds_window ? PH_PLAN_LDS : PH_PLAN_HBM;
  k.block = kBlock;
}

// Euler phi of every q <= max_p and all divisors of q in ascending order, CSR by q (QOPeriods.py:834-838), by sieve:
// O(max_p log max_p).
void divisor_tables(int max_p, std::vector<int32_t>* phi_out, std::vector<int32_t>* off_out, std::vector<int32_t>* dq_out) {
  std::vector<int32_t>&phi = *phi_out, &off = *off_out, &dq = *dq_out;
  phi.assign((size_t)max_p + 1, 0);
  off.assign((size_t)max_p + 2, 0);
  for (int i = 0; i <= max_p; ++i) phi[i] = i;
  for (int i = 2; i <= max_p; ++i)
    if (phi[i] == i)
      for (int j = i; j <= max_p; j += i) phi[j] -= phi[j] / i;
  for (int d = 1; d <= max_p; ++d)
    for (int q = d; q <= max_p; q += d) ++off[q + 1];
  for (int q = 0; q <= max_p; ++q) off[q + 1] += off[q];
  dq.assign((size_t)off[max_p + 1], 0);
  {
    std::vector<int32_t> fill(off.begin(), off.end() - 1);
    for (int d = 1; d <= max_p; ++d)
      for (int q = d; q <= max_p; q += d) dq[fill[q]++] = d;
  }
  if (dq.empty()) dq.push_back(1);
}

// k_qo_fit: the LDS holds the solver's vectors only (ph::qo_fit_lds_bytes, the layout the kernel carves); the window is
// read from HBM / L2.  The largest feasible kcap is the last one this accepts.
int plan_qo_fit(const ph_ctx* c, int kcap, int max_period, Plan* pl) {
  if (max_period < 1 || max_period > ph::kFitMaxPeriod)
    return fail(PH_E_ARG, "ph_qo_fit: max_period=%d must be in [1, %d]", max_period, ph::kFitMaxPeriod);
  if (kcap < 1 || kcap > ph::kQoGreedyMaxRows) return fail(PH_E_ARG, "ph_qo_fit: kcap=%d must be in [1, %d]", kcap, ph::kQoGreedyMaxRows);
  KernelPlan& k = pl->k[0];
  k.lds = ph::qo_fit_lds_bytes(kcap, max_period);
  if (k.lds > (size_t)c->lds_limit)
    return fail(PH_E_ARG, "ph_qo_fit: kcap=%d, max_period=%d need %zu B of LDS (limit %d B)", kcap, max_period, k.lds,
                c->lds_limit);
  k.window = PH_PLAN_HBM;
  k.block = ph::qo_fit_block(kcap);
  return PH_OK;
}

// k_qo_fit_win: k_qo_fit's LDS plus the staging vector u of N doubles (ph::qo_fit_win_lds_bytes, the layout the kernel
// carves).  u stays in LDS behind the solver while both fit the workgroup's limit and PH_HBM_WINDOW is not set; otherwise
// it takes N doubles per workgroup of an HBM workspace (`second`).  The analysis window is shared by the grid and is
// always read from HBM / L2, as x is (`window`).
int plan_qo_fit_win(const ph_ctx* c, int N, int kcap, int max_period, Plan* pl) {
  PH_TRY(plan_qo_fit(c, kcap, max_period, pl));
  KernelPlan& k = pl->k[0];
  const bool u_lds = !c->hbm_window && ph::qo_fit_win_lds_bytes(N, kcap, max_period, true) <= (size_t)c->lds_limit;
  k.lds = ph::qo_fit_win_lds_bytes(N, kcap, max_period, u_lds);
  k.second = u_lds ? PH_PLAN_LDS : PH_PLAN_HBM;
  k.block = ph::qo_fit_win_block(kcap, N);
  return PH_OK;
}

// k_qo_extract: the concatenated input, the accumulators, the two d-length vectors and the list of shared d
// (ph::qo_extract_work_bytes, the layout the kernel carves) live in LDS behind the control words while they fit the
// workgroup's limit and PH_HBM_WINDOW is not set; otherwise in one slice per workgroup of an HBM workspace.  Both move
// together (`window` = the input, `second` = the accumulators).
int plan_qo_extract(const ph_ctx* c, int ccap, int max_period, Plan* pl) {
  if (max_period < 1 || max_period > ph::kFitMaxPeriod)
    return fail(PH_E_ARG, "ph_qo_get_periods: max_period=%d must be in [1, %d]", max_period, ph::kFitMaxPeriod);
  if (ccap < 1 || ccap > (1 << 24)) return fail(PH_E_ARG, "ph_qo_get_periods: ccap=%d must be in [1, 2^24]", ccap);
  KernelPlan& k = pl->k[0];
  const bool in_lds = !c->hbm_window && ph::qo_extract_lds_bytes(ccap, max_period, true) <= (size_t)c->lds_limit;
  k.lds = ph::qo_extract_lds_bytes(ccap, max_period, in_lds);
  k.window = k.second = in_lds ? PH_PLAN_LDS : PH_PLAN_HBM;
  k.block = kBlock;
  return PH_OK;
}

// ----------------------------------------------------------------------------- argument resolvers
// One per entry point, as qo_plan and fit_prepare are for theirs: the defaults and refusals of the entry point's own
// arguments, then its plan_* function.  The entry point and its ph_plan_info case both call it and state no argument rule
// themselves; what only a launch can check (NULL outputs, the content of tables, W) stays with the launch.
int resolve_project(const ph_ctx* c, int dtype, int N, int pmax, unsigned flags, Plan* pl, int* scratch_len) {
  if (pmax < 1) return fail(PH_E_ARG, "p_list max %d must be >= 1", pmax);
  return plan_project(c, dtype, N, pmax, flags, pl, scratch_len);
}

int check_sweep_range(int p_lo, int p_hi) {
  if (p_lo < 1 || p_hi < p_lo) return fail(PH_E_ARG, "need 1 <= p_lo <= p_hi (got %d, %d)", p_lo, p_hi);
  return PH_OK;
}

int resolve_sweep(const ph_ctx* c, int dtype, int N, int p_lo, int p_hi, int mode, unsigned flags, Plan* pl) {
  PH_TRY(check_sweep_range(p_lo, p_hi));
  if (mode < 0 || mode > 2) return fail(PH_E_ARG, "mode %d unknown", mode);
  return plan_sweep(c, dtype, N, mode, flags, pl);
}

// Most proper divisors (1 and p removed) any period up to max_length has: the longest row of the caller's factor table
// (CSR offsets, covering max_length), or without one the same count by sieve, as _factors.factor_tables makes the rows.
int max_proper_divisors(const int32_t* fac_off, int max_length) {
  int max_fac = 1;
  if (fac_off) {
    for (int q = 0; q <= max_length; ++q) max_fac = std::max(max_fac, fac_off[q + 1] - fac_off[q]);
    return max_fac;
  }
  std::vector<int32_t> nd((size_t)max_length + 1, 0);
  for (int d = 2; d <= max_length; ++d)
    for (int q = 2 * d; q <= max_length; q += d) ++nd[q];
  return std::max(max_fac, *std::max_element(nd.begin(), nd.end()));
}

// m_best: max_length < 0 means N / 3 (Periods.py:485-486); max_fac < 0 means "count them" (max_proper_divisors over
// fac_off, which may be NULL).  `pair` is the plan's step-1 variant and p_scr the first period that kernel screens, so
// the launch and the ph_m_best_*_info queries cannot disagree on either.
struct MBestArgs {
  int max_length, max_fac, p_scr;
  bool pair;
  Plan pl;
};

int resolve_m_best(const ph_ctx* c, int dtype, int N, int num, int min_length, int max_length, int gamma,
                   const int32_t* fac_off, int table_max_p, int max_fac, unsigned flags, MBestArgs* a) {
  if (num < 1 || num > 4096) return fail(PH_E_ARG, "num=%d must be in [1, 4096]", num);
  if (max_length < 0) max_length = N / 3;
  if (min_length < 1 || max_length < min_length)
    return fail(PH_E_ARG, "need 1 <= min_length <= max_length (got %d, %d)", min_length, max_length);
  if (fac_off && table_max_p < max_length)
    return fail(PH_E_ARG, "factor tables cover p <= %d, need %d", table_max_p, max_length);
  a->max_length = max_length;
  a->max_fac = max_fac < 0 ? max_proper_divisors(fac_off, max_length) : max_fac;
  PH_TRY(plan_m_best(c, dtype, N, num, min_length, max_length, a->max_fac, flags, &a->pl));
  a->pair = a->pl.k[0].variant == PH_PLAN_PAIR;
  a->p_scr = a->pair ? pair_screen_lo(c, min_length, max_length, gamma) : min_length;
  return PH_OK;
}

// what the ph_m_best_*_info queries ask: ph_m_best's resolver without a factor table (the divisor count by sieve)
int m_best_query(const ph_ctx* c, int dtype, int N, int num, int min_length, int max_length, int gamma, unsigned flags,
                 MBestArgs* a) {
  if (dtype != PH_F64 && dtype != PH_F32) return fail(PH_E_ARG, "dtype must be PH_F64 or PH_F32");
  if (N < 1) return fail(PH_E_ARG, "N=%d must be >= 1", N);
  return resolve_m_best(c, dtype, N, num, min_length, max_length, gamma, nullptr, 0, -1, flags, a);
}

// n_periods < 0 means N / 2 (Periods.py:271-272)
int resolve_small_to_large(const ph_ctx* c, int dtype, int N, int* n_periods_io, unsigned flags, Plan* pl) {
  if (*n_periods_io < 0) *n_periods_io = N / 2;
  return plan_small_to_large(c, dtype, N, *n_periods_io, flags, pl);
}

// max_length < 0 means N / 3 (Periods.py:311-312)
int resolve_best_correlation(const ph_ctx* c, int dtype, int N, int* max_length_io, unsigned flags, Plan* pl) {
  if (*max_length_io < 0) *max_length_io = N / 3;
  return plan_best_correlation(c, dtype, N, *max_length_io, flags, pl);
}

// win_size < 1 means N (Periods.py:381-382); *L receives the value used
int resolve_best_frequency(const ph_ctx* c, int dtype, int N, int win_size, int* L, Plan* pl, BfShape* g) {
  *L = win_size < 1 ? N : win_size;
  if (*L < 2 || *L > (1 << 24)) return fail(PH_E_ARG, "win_size=%d out of range", *L);
  return plan_best_frequency(c, dtype, N, *L, pl, g);
}

int resolve_ramanujan(const ph_ctx* c, int dtype, int N, int q_lo, int q_hi, Plan* pl) {
  if (q_lo < 1 || q_hi < 1) return fail(PH_E_ARG, "need q_lo, q_hi >= 1 (got %d, %d)", q_lo, q_hi);
  return plan_ramanujan(c, dtype, N, q_hi, pl);
}

// max_p < 0 means N / 2 (QOPeriods.py:1204-1207)
int resolve_orth_powers(const ph_ctx* c, int dtype, int N, int* max_p_io, Plan* pl) {
  if (*max_p_io < 0) *max_p_io = N / 2;
  if (*max_p_io < 2) return fail(PH_E_ARG, "max_p=%d must be >= 2", *max_p_io);
  plan_orth_powers(c, dtype, N, *max_p_io, pl);
  return PH_OK;
}

// ph_period_path: the limits of k_period_path (ph_path.h) and its launch shape -- threads, states per thread, the carve's
// LDS bytes and backtrace tile height, the bytes of one back-pointer row.  R, W and ld are a launch's own; the plan query
// asks with R = W = 1, ld = P.
struct PathPlan {
  int block, states, tile, row_bytes;
  size_t lds;
};

int resolve_period_path(const ph_ctx* c, int64_t R, int64_t W, int P, int64_t ld, int band, double jump, PathPlan* pp) {
  if (P < 1 || P > ph::kPathMaxP) return fail(PH_E_ARG, "ph_period_path: P=%d must be in [1, %d]", P, ph::kPathMaxP);
  if (band < 0 || band > ph::kPathHalo)
    return fail(PH_E_ARG, "ph_period_path: band=%d must be in [0, %d]", band, ph::kPathHalo);
  if (!(jump >= 0.0) || !(jump <= 1.7976931348623157e308))
    return fail(PH_E_ARG, "ph_period_path: jump=%g must be finite and >= 0", jump);
  if (W < 1) return fail(PH_E_ARG, "ph_period_path: W=%lld must be >= 1", (long long)W);
  if (R < 0 || R > 0x7fffffffLL) return fail(PH_E_ARG, "ph_period_path: R=%lld must be in [0, 2^31)", (long long)R);
  if (ld < P) return fail(PH_E_ARG, "ph_period_path: ld=%lld must be >= P=%d", (long long)ld, P);
  // R * W * ld doubles of cost, R * W * row_bytes of back-pointers (row_bytes <= 16 ld): both inside int64
  if (W > (INT64_MAX / 16) / ld || (R > 0 && W * ld > (INT64_MAX / 16) / R))
    return fail(PH_E_ARG, "ph_period_path: R * W * ld does not fit 64 bits");
  const auto L = ph::path_carve(CarveCount(), P, c->path_tile_cap);
  *pp = PathPlan{ph::path_block(P), ph::path_states(P), L.tile, ph::path_row_bytes(P), L.bytes};
  if (pp->lds > (size_t)c->lds_limit)
    return fail(PH_E_ARG, "ph_period_path: P=%d needs %zu B of LDS, device limit is %d B", P, pp->lds, c->lds_limit);
  return PH_OK;
}

// ph_follow: the sizes k_follow (ph_follow.h) takes and its launch shape -- threads, the carve's LDS bytes, and where the
// two per-workgroup states (the residual frame, one period of means) live: in LDS while both fit the workgroup's limit
// and PH_HBM_WINDOW is not set, otherwise in one slice per workgroup of an HBM workspace.  Both move together.
struct FollowPlan {
  int block, placement;
  size_t lds;
};
int resolve_follow(const ph_ctx* c, int N, FollowPlan* fp) {
  if (N < 1) return fail(PH_E_ARG, "ph_follow: N=%d must be >= 1", N);
  const bool in_lds = !c->hbm_window && ph::follow_carve(ph::CarveCount(), N, true).bytes <= (size_t)c->lds_limit;
  *fp = FollowPlan{ph::follow_block(N), in_lds ? PH_PLAN_LDS : PH_PLAN_HBM, ph::follow_carve(ph::CarveCount(), N, in_lds).bytes};
  return PH_OK;
}

// (ph_qo_orth_select has no default or refusal beside plan_qo_orth_select's own max_p >= 2: that function is its resolver)

// What the window-pair kernels take beside the one-window arguments: one fp64 row of win_stride(N) per window in the
// B_GWIN workspace, and the float tables prepare_geom keeps next to geom.
struct PairWs {
  double* gwin;
  const ph::PGeomF* geomf;
  const double* radq;
  const float* kapf;
};

int pair_workspace(ph_ctx* c, int64_t W, int N, PairWs* ws) {
  PH_TRY(ensure(c, c->buf[B_GWIN], (size_t)W * ph::win_stride((size_t)N) * sizeof(double)));
  *ws = PairWs{static_cast<double*>(c->buf[B_GWIN].p), static_cast<const ph::PGeomF*>(c->geomf.p),
               static_cast<const double*>(c->radq.p), static_cast<const float*>(c->kapf.p)};
  return PH_OK;
}

}  // namespace


// =========================================================================================
extern "C" {

int ph_version(void) { return PH_VERSION; }

#ifdef PH_CLOCKS
// diagnostic builds only (not part of the C ABI): workgroup stamps of the last k_small_to_large_pair launch
int ph_debug_stamps(long long* dst, int n_wg) {
  PH_HIP(hipDeviceSynchronize());
  PH_HIP(hipMemcpyFromSymbol(dst, HIP_SYMBOL(ph::g_ph_stamps), sizeof(long long) * 4 * (size_t)n_wg));
  return PH_OK;
}
#endif

const char* ph_last_error(void) { return g_err.c_str(); }

int ph_device_count(int* count) {
  if (!count) return fail(PH_E_ARG, "count is NULL");
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess) {
    *count = 0;
    return fail(PH_E_HIP, "hipGetDeviceCount: %s", hipGetErrorString(e));
  }
  *count = n;
  return PH_OK;
}

int ph_create(int device, ph_ctx** out) {
  if (!out) return fail(PH_E_ARG, "out is NULL");
  *out = nullptr;
  int n = 0;
  PH_HIP(hipGetDeviceCount(&n));
  if (device < 0 || device >= n) return fail(PH_E_ARG, "device %d not in [0, %d)", device, n);
  PH_HIP(hipSetDevice(device));
  ph_ctx* c = new (std::nothrow) ph_ctx();
  if (!c) return fail(PH_E_NOMEM, "out of host memory");
  c->device = device;
  hipDeviceProp_t prop;
  hipError_t e = hipGetDeviceProperties(&prop, device);
  if (e != hipSuccess) {
    delete c;
    return fail(PH_E_HIP, "hipGetDeviceProperties: %s", hipGetErrorString(e));
  }
  c->num_cu = prop.multiProcessorCount;
  // gfx950 has 160 KiB of LDS per CU and one workgroup may use all of it; take the largest
  // figure the runtime reports (an oversize launch fails cleanly with a launch error).
  size_t lds = prop.sharedMemPerBlock;
  lds = std::max(lds, prop.sharedMemPerBlockOptin);
  lds = std::max(lds, prop.maxSharedMemoryPerMultiProcessor);
  c->lds_limit = (int)std::min<size_t>(lds, 160 * 1024);
  if ((e = hipStreamCreateWithFlags(&c->own_stream, hipStreamNonBlocking)) != hipSuccess ||
      (e = hipEventCreate(&c->ev0)) != hipSuccess || (e = hipEventCreate(&c->ev1)) != hipSuccess) {
    delete c;
    return fail(PH_E_HIP, "stream/event creation: %s", hipGetErrorString(e));
  }
  c->stream = c->own_stream;
  if (const char* e = std::getenv("PH_PLAN_MAX_M")) {
    const int v = std::atoi(e);
    if (v == 1 || v == 2 || v == 4) c->plan_max_m = v;
  }
  if (const char* e = std::getenv("PH_STEP1_PAIR")) c->step1_pair = std::atoi(e) != 0;
  if (const char* e = std::getenv("PH_S2L_PAIR")) c->s2l_pair = std::atoi(e) != 0;
  if (const char* e = std::getenv("PH_BC_PAIR")) c->bc_pair = std::atoi(e) != 0;
  if (const char* e = std::getenv("PH_PAIR_CHAIN")) c->pair_chain = std::atoi(e) != 0;
  if (const char* e = std::getenv("PH_PAIR_COVER")) c->pair_cover = std::atoi(e) != 0;
  if (const char* e = std::getenv("PH_PAIR_DUO")) c->pair_duo = std::atoi(e) != 0;
  if (const char* e = std::getenv("PH_PAIR_FOLD_ONCE")) c->pair_fold_once = std::atoi(e) != 0;
  if (const char* e = std::getenv("PH_PAIR_FOLD_REPORT")) c->pair_fold_report = std::atoi(e) != 0;
  if (const char* e = std::getenv("PH_STEP2_GEOM")) c->step2_geom = std::atoi(e) != 0;
  if (const char* e = std::getenv("PH_STEP1_BLOCK")) {
    const int v = std::atoi(e);
    if (v >= 64 && v <= 1024 && v % 64 == 0) c->step1_block = v;
  }
  if (const char* e = std::getenv("PH_S2L_BLOCK")) {
    const int v = std::atoi(e);
    if (v >= 512 && v <= 1024 && v % 64 == 0) c->s2l_block = v;
  }
  if (const char* e = std::getenv("PH_QO_BLOCK")) {
    const int v = std::atoi(e);
    if (v >= 64 && v <= 1024 && v % 64 == 0) c->qo_block = v;
  }
  if (std::getenv("PH_QO_HBM_WINDOW")) c->qo_hbm_window = true;
  if (const char* e = std::getenv("PH_HBM_WINDOW"))
    if (std::atoi(e) != 0) c->hbm_window = c->qo_hbm_window = true;
  if (const char* e = std::getenv("PH_SWEEP_BLOCK")) {
    const int v = std::atoi(e);
    if (v >= 64 && v <= 512 && v % 64 == 0) c->sweep_block = v;
  }
  if (const char* e = std::getenv("PH_PATH_TILE_ROWS")) c->path_tile_cap = std::max(0, std::atoi(e));
  *out = c;
  return PH_OK;
}

int ph_destroy(ph_ctx* c) {
  if (!c) return PH_OK;
  (void)hipSetDevice(c->device);
  (void)hipStreamSynchronize(c->stream);
  for (DevBuf& b : c->buf)
    if (b.p) (void)hipFree(b.p);
  for (TableSlot& t : c->tab)
    if (t.dev.p) (void)hipFree(t.dev.p);
  if (c->geom.p) (void)hipFree(c->geom.p);
  if (c->geomf.p) (void)hipFree(c->geomf.p);
  if (c->radq.p) (void)hipFree(c->radq.p);
  if (c->kapf.p) (void)hipFree(c->kapf.p);
  if (c->plan.p) (void)hipFree(c->plan.p);
  if (c->twid.p) (void)hipFree(c->twid.p);
  if (c->bs_tab.p) (void)hipFree(c->bs_tab.p);
  for (hipEvent_t e : c->prof_ev) (void)hipEventDestroy(e);
  if (c->ev0) (void)hipEventDestroy(c->ev0);
  if (c->ev1) (void)hipEventDestroy(c->ev1);
  if (c->own_stream) (void)hipStreamDestroy(c->own_stream);
  delete c;
  return PH_OK;
}

int ph_set_stream(ph_ctx* c, void* hip_stream) {
  if (!c) return fail(PH_E_ARG, "ctx is NULL");
  // drain the old stream, but rebind even if that fails (a borrowed stream may have been destroyed:
  // the context must not stay stuck on it); the error is reported after the switch
  const hipError_t e = hipStreamSynchronize(c->stream);
  if (hip_stream == PH_STREAM_DEFAULT)
    c->stream = nullptr;  // the legacy default stream
  else
    c->stream = hip_stream ? static_cast<hipStream_t>(hip_stream) : c->own_stream;
  if (e != hipSuccess) {
    (void)hipGetLastError();
    return fail(PH_E_HIP, "ph_set_stream: draining the previous stream failed (%s); the new stream is bound",
                hipGetErrorString(e));
  }
  return PH_OK;
}

int ph_sweep_plan_info(ph_ctx* c, int p_lo, int p_hi, int* n_pass, int* n_periods) {
  if (!c || !n_pass || !n_periods) return fail(PH_E_ARG, "NULL argument");
  PH_TRY(check_sweep_range(p_lo, p_hi));
  *n_pass = (int)build_plan(p_lo, p_hi, c->plan_max_m, true, c->pair_chain).size();  // the plan ph_sweep's norm modes run
  *n_periods = p_hi - p_lo + 1;
  return PH_OK;
}

int ph_pair_radius_table(int N, int max_p, double* out) {
  if (!out) return fail(PH_E_ARG, "NULL argument");
  if (N < 1 || max_p < 1 || max_p > N) return fail(PH_E_ARG, "need 1 <= max_p <= N (got %d, %d)", max_p, N);
  const std::vector<double> host = pair_radius_table(N, max_p);
  std::copy(host.begin(), host.end(), out);
  return PH_OK;
}

int ph_m_best_info(ph_ctx* c, int dtype, int N, int num, int min_length, int max_length, unsigned flags,
                   int* windows_per_workgroup, int* lds_bytes_per_sample) {
  if (!c || !windows_per_workgroup || !lds_bytes_per_sample) return fail(PH_E_ARG, "NULL argument");
  MBestArgs a;
  PH_TRY(m_best_query(c, dtype, N, num, min_length, max_length, 0, flags, &a));
  *windows_per_workgroup = a.pair ? 2 : 1;
  *lds_bytes_per_sample = a.pair ? 8 : (int)elem_size(dtype);
  return PH_OK;
}

int ph_m_best_plan_info(ph_ctx* c, int dtype, int N, int num, int min_length, int max_length, unsigned flags, int* n_pass,
                        int* n_periods) {
  if (!c || !n_pass || !n_periods) return fail(PH_E_ARG, "NULL argument");
  // the passes plain m_best runs: the pair kernel screens [pair_screen_lo, max_length] only (m_best_gamma: every period)
  MBestArgs a;
  PH_TRY(m_best_query(c, dtype, N, num, min_length, max_length, 0, flags, &a));
  *n_pass = (int)build_plan(a.p_scr, a.max_length, c->plan_max_m, false, a.pair && c->pair_chain).size();
  *n_periods = a.max_length - min_length + 1;
  return PH_OK;
}

namespace {

// LDS elements (64 per wavefront load) one entry of a window-pair plan reads: the loads of pair_pass_single /
// pair_pass_multi (every chunk of the part up to the cut with all rows, the chunks behind it with one row fewer),
// of pair_pass_duo (its load rule, column by column) and of the row-split passes below 64.
long long plan_entry_elements(const ph::PassPlan& e, int N) {
  const int p = e.p;
  if (e.m == 0 || e.m >= 8) {
    const int L = (64 / p) * p;
    return 64LL * ((N + L - 1) / L);
  }
  const int rows = (N + p - 1) / p, cut = N - (rows - 1) * p;
  if (e.m != 3) {
    const int acols = std::min(p, (cut + 63) & ~63), rest = p - acols;
    return 64LL * ((long long)((cut + 63) / 64) * rows + (long long)((rest + 63) / 64) * (rows - 1));
  }
  const int ncb = (p + 63) / 64;
  long long loads = 0;
  for (int col = 0; col < ncb + rows; ++col)
    for (int r = 0; r < rows; ++r)
      if (r >= col - ncb && 64 * col + r * p < N) loads += 1;
  return 64 * loads;
}

}  // namespace

int ph_m_best_screen_info(ph_ctx* c, int dtype, int N, int num, int min_length, int max_length, unsigned flags, int gamma,
                          int* n_entries, int* n_screened, long long* lds_elements) {
  if (!c || !n_entries || !n_screened || !lds_elements) return fail(PH_E_ARG, "NULL argument");
  // (the one-window kernel folds every period of [min_length, max_length] in its own precision: same accounting)
  MBestArgs a;
  PH_TRY(m_best_query(c, dtype, N, num, min_length, max_length, gamma, flags, &a));
  const std::vector<ph::PassPlan> plan =
      build_plan(a.p_scr, a.max_length, c->plan_max_m, false, a.pair && c->pair_chain, a.pair && c->pair_duo ? N : 0);
  *n_entries = (int)plan.size();
  *n_screened = a.max_length - a.p_scr + 1;
  *lds_elements = 0;
  for (const ph::PassPlan& e : plan) *lds_elements += plan_entry_elements(e, N);
  return PH_OK;
}

int ph_sync(ph_ctx* c) {
  if (!c) return fail(PH_E_ARG, "ctx is NULL");
  PH_HIP(hipStreamSynchronize(c->stream));
  return PH_OK;
}

int ph_timer_begin(ph_ctx* c) {
  if (!c) return fail(PH_E_ARG, "ctx is NULL");
  PH_HIP(hipEventRecord(c->ev0, c->stream));
  return PH_OK;
}

int ph_timer_end(ph_ctx* c, float* ms) {
  if (!c || !ms) return fail(PH_E_ARG, "NULL argument");
  PH_HIP(hipEventRecord(c->ev1, c->stream));
  PH_HIP(hipEventSynchronize(c->ev1));
  PH_HIP(hipEventElapsedTime(ms, c->ev0, c->ev1));
  return PH_OK;
}

int ph_profile_enable(ph_ctx* c, int on) {
  if (!c) return fail(PH_E_ARG, "ctx is NULL");
  c->prof_on = on != 0;
  c->prof_n = 0;
  return PH_OK;
}

int ph_profile_read(ph_ctx* c, float* ms, int cap, int* count) {
  if (!c || !count) return fail(PH_E_ARG, "NULL argument");
  PH_HIP(hipStreamSynchronize(c->stream));
  *count = c->prof_n;
  for (int i = 0; i < c->prof_n && i < cap && ms; ++i)
    PH_HIP(hipEventElapsedTime(&ms[i], c->prof_ev[2 * i], c->prof_ev[2 * i + 1]));
  return PH_OK;
}

const char* ph_profile_name(ph_ctx* c, int i) {
  if (!c || i < 0 || i >= c->prof_n) return "";
  return c->prof_name[i];
}

int ph_device_info(ph_ctx* c, int* num_cu, int* lds_bytes) {
  if (!c) return fail(PH_E_ARG, "ctx is NULL");
  if (num_cu) *num_cu = c->num_cu;
  if (lds_bytes) *lds_bytes = c->lds_limit;
  return PH_OK;
}

int ph_max_window(ph_ctx* c, int dtype, unsigned flags, int* max_n) {
  if (!c || !max_n) return fail(PH_E_ARG, "NULL argument");
  if (dtype != PH_F64 && dtype != PH_F32) return fail(PH_E_ARG, "dtype must be PH_F64 or PH_F32");
  (void)flags;  // a second (projection) buffer moves to an HBM workspace before the window does
  // the last N whose sweep window stays in LDS (the placement is monotone in N): sweep_lds(lo), !sweep_lds(hi)
  auto sweep_lds = [&](int n) {
    Plan pl;
    return n < 1 || (plan_sweep(c, dtype, n, PH_SWEEP_NORM, 0u, &pl) == PH_OK && pl.k[0].window == PH_PLAN_LDS);
  };
  int lo = 0, hi = (int)((size_t)c->lds_limit / elem_size(dtype)) + 1;
  while (hi - lo > 1) {
    const int mid = lo + (hi - lo) / 2;
    (sweep_lds(mid) ? lo : hi) = mid;
  }
  *max_n = lo;
  return PH_OK;
}

int ph_plan_info(ph_ctx* c, int op, int dtype, int N, const int32_t* params, int n_params, unsigned flags,
                 int32_t* out) {
  if (!c || !out) return fail(PH_E_ARG, "NULL argument");
  if (n_params < 0 || (n_params > 0 && !params)) return fail(PH_E_ARG, "params NULL or n_params=%d < 0", n_params);
  if (dtype != PH_F64 && dtype != PH_F32) return fail(PH_E_ARG, "dtype must be PH_F64 or PH_F32");
  if (N < 1) return fail(PH_E_ARG, "N=%d must be >= 1", N);
  static_assert(PH_PLAN_K1 == PH_PLAN_K0 + PH_PLAN_STRIDE && PH_PLAN_LEN == PH_PLAN_K0 + 2 * PH_PLAN_STRIDE,
                "periodhip.h plan record layout");
  auto prm = [&](int i, int def) { return i < n_params ? (int)params[i] : def; };
  Plan pl;
  switch (op) {
    case PH_OP_PROJECT: {
      int scratch_len;
      PH_TRY(resolve_project(c, dtype, N, prm(0, N), flags, &pl, &scratch_len));
      break;
    }
    case PH_OP_SWEEP:
      PH_TRY(resolve_sweep(c, dtype, N, prm(0, 1), prm(1, N / 3), prm(2, PH_SWEEP_NORM), flags, &pl));
      break;
    case PH_OP_M_BEST: {
      MBestArgs a;
      PH_TRY(resolve_m_best(c, dtype, N, prm(0, 5), prm(1, 2), prm(2, -1), 0, nullptr, 0, prm(3, -1), flags, &a));
      pl = a.pl;
      break;
    }
    case PH_OP_SMALL_TO_LARGE: {
      int n_periods = prm(0, -1);
      PH_TRY(resolve_small_to_large(c, dtype, N, &n_periods, flags, &pl));
      break;
    }
    case PH_OP_BEST_CORRELATION: {
      int max_length = prm(0, -1);
      PH_TRY(resolve_best_correlation(c, dtype, N, &max_length, flags, &pl));
      break;
    }
    case PH_OP_BEST_FREQUENCY: {
      int L;
      BfShape g;
      PH_TRY(resolve_best_frequency(c, dtype, N, prm(0, -1), &L, &pl, &g));
      break;
    }
    case PH_OP_RAMANUJAN:
      PH_TRY(resolve_ramanujan(c, dtype, N, prm(0, 2), prm(1, N / 3), &pl));
      break;
    case PH_OP_ORTH_POWERS: {
      int max_p = prm(0, -1);
      PH_TRY(resolve_orth_powers(c, dtype, N, &max_p, &pl));
      break;
    }
    case PH_OP_FOLD_SUMS:
      plan_fold_sums(c, dtype, N, &pl);
      break;
    case PH_OP_QO_FIT:
      PH_TRY(plan_qo_fit(c, prm(0, 512), prm(1, N), &pl));
      break;
    case PH_OP_QO_FIT_WIN:
      PH_TRY(plan_qo_fit_win(c, N, prm(0, 512), prm(1, N), &pl));
      break;
    case PH_OP_QO_ORTH_SELECT: {
      int max_p = prm(0, -1);
      if (max_p < 0) max_p = N / 3;  // find_periods' max_length default (QOPeriods.py:374-375)
      PH_TRY(plan_qo_orth_select(c, dtype, N, max_p, &pl));
      break;
    }
    case PH_OP_QO_GET_PERIODS:
      PH_TRY(plan_qo_extract(c, prm(0, N), prm(1, N), &pl));
      break;
    default:
      return fail(PH_E_ARG, "op %d unknown", op);
  }
  std::memset(out, 0, PH_PLAN_LEN * sizeof(int32_t));
  out[PH_PLAN_KERNELS] = pl.n_kernels;
  for (int i = 0; i < pl.n_kernels; ++i) {
    const KernelPlan& k = pl.k[i];
    int32_t* r = out + PH_PLAN_K0 + i * PH_PLAN_STRIDE;
    r[PH_PLAN_VARIANT] = k.variant;
    r[PH_PLAN_WINDOW] = k.window;
    r[PH_PLAN_SECOND] = k.second;
    r[PH_PLAN_BLOCK] = k.block;
    r[PH_PLAN_LDS_BYTES] = (int32_t)k.lds;
    r[PH_PLAN_SMALL_MEANS] = k.small_means;
    r[PH_PLAN_WAVES] = k.waves;
    r[PH_PLAN_PAD] = k.pad;
  }
  return PH_OK;
}

// ----------------------------------------------------------------------------- K1
int ph_project_batch(ph_ctx* c, const void* x, int dtype, int64_t W, int N, const int32_t* p_list, int n_p,
                     const int32_t* orth_off, const int32_t* orth_q, int table_max_p, unsigned flags,
                     void* out) {
  PH_TRY(check_common(c, x, dtype, W, N));
  if (!p_list || n_p < 1 || !out) return fail(PH_E_ARG, "p_list/out NULL or n_p < 1");
  int pmax = 1;
  for (int k = 0; k < n_p; ++k) {
    if (p_list[k] < 1) return fail(PH_E_ARG, "p_list[%d]=%d must be >= 1", k, p_list[k]);
    pmax = std::max(pmax, p_list[k]);
  }
  PH_HIP(hipSetDevice(c->device));
  const size_t sz = elem_size(dtype);
  Plan pl;
  int scratch_len;
  PH_TRY(resolve_project(c, dtype, N, pmax, flags, &pl, &scratch_len));
  const size_t lds = pl.k[0].lds;
  const int chunks = pick_chunks(c, W, n_p, 1);
  void *gbuf, *gwin;
  PH_TRY(place(c, pl.k[0].second, B_GBUF, (size_t)W * chunks * scratch_len * sz, &gbuf));
  PH_TRY(place(c, pl.k[0].window, B_GWIN, (size_t)W * chunks * ph::win_stride(N) * sz, &gwin));
  ph::Tables tb{};
  PH_TRY(prepare_orth(c, flags, orth_off, orth_q, table_max_p, pmax, &tb));
  const int* d_plist;
  PH_TRY(upload_table(c, T_PLIST, p_list, n_p, &d_plist));
  Stage st(c, flags);
  const void* dx;
  void* dout;
  PH_TRY(st.in(x, (size_t)W * N * sz, &dx));
  PH_TRY(st.out(B_OUT0, out, (size_t)W * n_p * N * sz, &dout));
  const unsigned kflags = flags & (PH_FLAG_TRUNC | PH_FLAG_ORTH | PH_FLAG_SINGLE);
  if (flags & PH_FLAG_SINGLE) PH_HIP(hipMemsetAsync(dout, 0, (size_t)W * n_p * N * sz, c->stream));
  const dim3 grid((unsigned)(W * chunks));
  PH_TRY(dispatch(dtype, !gwin, [&](auto t, auto lw) {
    using T = decltype(t);
    return launch(c, "k_project_batch", ph::k_project_batch<T, decltype(lw)::value>, grid, kBlock, lds, (const T*)dx, N,
                  d_plist, n_p, chunks, kflags, tb, scratch_len, (T*)gbuf, (T*)gwin, (T*)dout);
  }));
  return st.finish();
}

// ----------------------------------------------------------------------------- K2
int ph_sweep(ph_ctx* c, const void* x, int dtype, int64_t W, int N, int p_lo, int p_hi, int mode,
             const int32_t* orth_off, const int32_t* orth_q, int table_max_p, unsigned flags, double* out) {
  PH_TRY(check_common(c, x, dtype, W, N));
  if (!out) return fail(PH_E_ARG, "out is NULL");
  Plan pl;
  PH_TRY(resolve_sweep(c, dtype, N, p_lo, p_hi, mode, flags, &pl));
  PH_HIP(hipSetDevice(c->device));
  const size_t sz = elem_size(dtype);
  const bool general = pl.k[0].second != PH_PLAN_NONE;
  const size_t lds = pl.k[0].lds;
  const int P = p_hi - p_lo + 1;
  const int sweep_block = pl.k[0].block;
  const int chunks = pick_chunks(c, W, P, 8 * (sweep_block / 64));
  void *gbuf, *gwin;
  PH_TRY(place(c, pl.k[0].second, B_GBUF, (size_t)W * chunks * N * sz, &gbuf));
  PH_TRY(place(c, pl.k[0].window, B_GWIN, (size_t)W * chunks * ph::win_stride(N + kPad) * sz, &gwin));
  const ph::PGeom* geom;
  PH_TRY(prepare_geom(c, N, p_hi, &geom));
  const ph::PassPlan* plan;
  int n_pass;
  // norm modes: the periods up to 64 in chains (one row-split pass yields L, L/2, ...: wave_chain_small)
  PH_TRY(prepare_plan(c, p_lo, p_hi, &plan, &n_pass, 4, true, true));
  ph::Tables tb{};
  PH_TRY(prepare_orth(c, general ? flags : 0u, orth_off, orth_q, table_max_p, p_hi, &tb));
  Stage st(c, flags);
  const void* dx;
  void* dout;
  PH_TRY(st.in(x, (size_t)W * N * sz, &dx));
  PH_TRY(st.out(B_OUT0, out, (size_t)W * P * sizeof(double), &dout));
  const unsigned kflags = flags & (PH_FLAG_TRUNC | PH_FLAG_ORTH);
  const dim3 grid((unsigned)(W * chunks));
  PH_TRY(dispatch(dtype, !gwin, [&](auto t, auto lw) {
    using T = decltype(t);
    return launch(c, "k_sweep", ph::k_sweep<T, decltype(lw)::value>, grid, sweep_block, lds, (const T*)dx, N, p_lo, p_hi,
                  mode, chunks, kflags, tb, geom, plan, n_pass, (T*)gbuf, (T*)gwin, (double*)dout);
  }));
  return st.finish();
}

// ----------------------------------------------------------------------------- m_best
int ph_m_best(ph_ctx* c, const void* x, int dtype, int64_t W, int N, int num, int min_length, int max_length,
              int gamma, const int32_t* orth_off, const int32_t* orth_q, const int32_t* fac_off,
              const int32_t* fac_q, int table_max_p, unsigned flags, uint32_t* periods, double* powers,
              void* bases, int32_t* status, int32_t* n_sweeps) {
  PH_TRY(check_common(c, x, dtype, W, N));
  if (!periods || !powers || !bases || !status) return fail(PH_E_ARG, "output pointer is NULL");
  if (!fac_off || !fac_q) return fail(PH_E_ARG, "fac_off/fac_q tables are required");
  MBestArgs a;
  PH_TRY(resolve_m_best(c, dtype, N, num, min_length, max_length, gamma, fac_off, table_max_p, -1, flags, &a));
  max_length = a.max_length;
  const int max_fac = a.max_fac, p_scr = a.p_scr;
  const bool pair = a.pair;
  const KernelPlan &s1 = a.pl.k[0], &s2 = a.pl.k[1];
  PH_HIP(hipSetDevice(c->device));
  const size_t sz = elem_size(dtype);
  const int P = max_length - min_length + 1;
  // the two kernels run back to back on one stream and may share the workspaces
  void *gbuf1, *gbuf2, *gwin1, *gwin2;
  PH_TRY(place(c, s1.second, B_GBUF, (size_t)W * N * sz, &gbuf1));
  PH_TRY(place(c, s2.second, B_GBUF, (size_t)W * N * sz, &gbuf2));
  PH_TRY(place(c, s1.window, B_GWIN, (size_t)W * ph::win_stride(N + kPad) * sz, &gwin1));
  PH_TRY(place(c, s2.window, B_GWIN, (size_t)W * ph::win_stride(N + kPad) * sz, &gwin2));
  ph::Tables tb{};
  PH_TRY(prepare_orth(c, flags, orth_off, orth_q, table_max_p, max_length, &tb));
  PH_TRY(prepare_fac(c, fac_off, fac_q, table_max_p, max_length, &tb));
  const ph::PGeom* geom;
  PH_TRY(prepare_geom(c, N, max_length, &geom));
  const ph::PassPlan* plan;
  int n_pass;
  // (the cached plan is keyed by its first period: the top-half plan of m_best and the full plan of m_best_gamma differ there)
  PH_TRY(prepare_plan(c, p_scr, max_length, &plan, &n_pass, 4, false, pair, pair ? N : 0));
  Stage st(c, flags);
  const void* dx;
  void *dper, *dpow, *dbases, *dstat;
  PH_TRY(st.in(x, (size_t)W * N * sz, &dx));
  PH_TRY(st.out(B_OUT0, periods, (size_t)W * num * sizeof(uint32_t), &dper));
  PH_TRY(st.out(B_OUT1, powers, (size_t)W * num * sizeof(double), &dpow));
  PH_TRY(st.out(B_OUT2, bases, (size_t)W * num * N * sz, &dbases));
  PH_TRY(st.out(B_OUT3, status, (size_t)W * sizeof(int32_t), &dstat));
  void* dsweeps;
  PH_TRY(st.out(B_OUT4, n_sweeps, (size_t)W * sizeof(int32_t), &dsweeps));
  PH_TRY(ensure(c, c->buf[B_WS0], (size_t)W * sizeof(double)));
  double* dnorm = static_cast<double*>(c->buf[B_WS0].p);
  // compact basis rows between the two kernels: the first p elements of every row (ph_mbest.h, step 2);
  // 16-byte aligned rows of a whole number of 128-element LDS-DMA pieces
  const int row_stride = (max_length + 127) & ~127;
  PH_TRY(ensure(c, c->buf[B_WS1], (size_t)W * num * row_stride * sz));
  void* drows = c->buf[B_WS1].p;
  const unsigned kflags = flags & (PH_FLAG_TRUNC | PH_FLAG_ORTH);
  const int max_iters = 12 * (P + num) + 64;
  const dim3 grid((unsigned)W);
  if (pair) {
    PairWs ws;
    PH_TRY(pair_workspace(c, W, N, &ws));
    ph::Step1PairArgs a;
    a.x = (const double*)dx;
    a.W = (int)W;
    a.N = N;
    a.num = num;
    a.p_lo = min_length;
    a.p_hi = max_length;
    a.p_scr = p_scr;
    a.gamma = gamma;
    a.n_pass = n_pass;
    a.fac_off = tb.fac_off;
    a.fac_q = tb.fac_q;
    a.geom = geom;
    a.geomf = ws.geomf;
    a.radq = ws.radq;
    a.plan = plan;
    a.gres = ws.gwin;
    a.periods_out = (uint32_t*)dper;
    a.norms_out = (double*)dpow;
    a.rows_out = (double*)drows;
    a.dnorm_out = dnorm;
    a.status_out = (int*)dstat;
    a.sweeps_out = (int*)dsweeps;
    a.thin_band = c->pair_fold_once ? ph::pair_thin_band(N) : -1.0;
    a.max_iters = max_iters;
    a.row_stride = row_stride;
    a.fold_report = c->pair_fold_report ? 1 : 0;
    PH_TRY(launch(c, "k_mbest_step1", ph::k_mbest_step1_pair, dim3((unsigned)((W + 1) / 2)), s1.block, s1.lds, a));
  } else {
    PH_TRY(dispatch(dtype, !gwin1, [&](auto t, auto lw) {
      using T = decltype(t);
      return launch(c, "k_mbest_step1", ph::k_mbest_step1<T, decltype(lw)::value>, grid, s1.block, s1.lds, (const T*)dx, N,
                    num, min_length, max_length, gamma, kflags, tb, geom, plan, n_pass, (T*)gbuf1, (T*)gwin1, max_iters,
                    (uint32_t*)dper, (double*)dpow, (T*)drows, row_stride, dnorm, (int*)dstat, (int*)dsweeps,
                    s1.small_means);
    }));
  }
  PH_TRY(dispatch(dtype, !gwin2, [&](auto t, auto lw) {
    using T = decltype(t);
    return launch(c, "k_mbest_step2", ph::k_mbest_step2<T, decltype(lw)::value>, grid, s2.block, s2.lds, N, num, gamma,
                  max_length, kflags | (c->step2_geom ? ph::kStep2Geom : 0u), tb, geom, max_fac, (T*)gbuf2, (T*)gwin2, (uint32_t*)dper, (double*)dpow, (T*)dbases,
                  dnorm, (const int*)dstat, (T*)drows, row_stride);
  }));
  return st.finish();
}

// ----------------------------------------------------------------------------- small_to_large
int ph_small_to_large(ph_ctx* c, const void* x, int dtype, int64_t W, int N, double thresh, int n_periods,
                      const int32_t* orth_off, const int32_t* orth_q, int table_max_p, unsigned flags, int cap,
                      int32_t* counts, int32_t* periods, double* powers, void* bases, int32_t* status) {
  PH_TRY(check_common(c, x, dtype, W, N));
  if (!counts || !periods || !powers || !status) return fail(PH_E_ARG, "output pointer is NULL");
  if (cap < 1) return fail(PH_E_ARG, "cap=%d must be >= 1", cap);
  Plan pl;
  PH_TRY(resolve_small_to_large(c, dtype, N, &n_periods, flags, &pl));
  PH_HIP(hipSetDevice(c->device));
  const size_t sz = elem_size(dtype);
  const KernelPlan& k = pl.k[0];
  void *gbuf, *gwin;
  PH_TRY(place(c, k.second, B_GBUF, (size_t)W * N * sz, &gbuf));
  PH_TRY(place(c, k.window, B_GWIN, (size_t)W * ph::win_stride(N + kPad) * sz, &gwin));
  const ph::PGeom* geom;
  PH_TRY(prepare_geom(c, N, std::max(n_periods, 2), &geom));
  ph::Tables tb{};
  PH_TRY(prepare_orth(c, flags, orth_off, orth_q, table_max_p, std::max(n_periods, 1), &tb));
  Stage st(c, flags);
  const void* dx;
  void *dcnt, *dper, *dpow, *dbases, *dstat;
  PH_TRY(st.in(x, (size_t)W * N * sz, &dx));
  PH_TRY(st.out(B_OUT0, counts, (size_t)W * sizeof(int32_t), &dcnt));
  PH_TRY(st.out(B_OUT1, periods, (size_t)W * cap * sizeof(int32_t), &dper));
  PH_TRY(st.out(B_OUT2, powers, (size_t)W * cap * sizeof(double), &dpow));
  PH_TRY(st.out(B_OUT3, bases, (size_t)W * cap * N * sz, &dbases));
  PH_TRY(st.out(B_OUT4, status, (size_t)W * sizeof(int32_t), &dstat));
  PH_HIP(hipMemsetAsync(dper, 0, (size_t)W * cap * sizeof(int32_t), c->stream));
  PH_HIP(hipMemsetAsync(dpow, 0, (size_t)W * cap * sizeof(double), c->stream));
  PH_TRY(ensure(c, c->buf[B_GEN0], 256));
  int* dmax = static_cast<int*>(c->buf[B_GEN0].p);  // largest count of the batch (device word)
  PH_HIP(hipMemsetAsync(dmax, 0, 2 * sizeof(int), c->stream));  // [1]: pair counter of the persistent pair kernel
  const unsigned kflags = flags & (PH_FLAG_TRUNC | PH_FLAG_ORTH);
  const dim3 grid((unsigned)W);
  if (k.variant == PH_PLAN_PAIR) {
    PairWs ws;
    PH_TRY(pair_workspace(c, W, N, &ws));
    // persistent workgroups: as many as are resident at once (LDS and the 32 wavefronts of a CU), pairs from a counter
    const int64_t npairs = (W + 1) / 2;
    const int per_cu = (int)std::max<size_t>(1, std::min<size_t>((size_t)c->lds_limit / k.lds, 2048 / (size_t)k.block));
    const unsigned grid_pairs = (unsigned)std::min<int64_t>(npairs, (int64_t)c->num_cu * per_cu);
    // the instantiation follows the block: the fixed-count one is never launched with another block size
    const auto kern = k.block == ph::kPairWaves * ph::kWave ? ph::k_small_to_large_pair<ph::kPairWaves> : ph::k_small_to_large_pair<0>;
    PH_TRY(launch(c, "k_small_to_large", kern, dim3(grid_pairs), k.block, k.lds, (const double*)dx,
                  (int)W, N, thresh, n_periods, ws.geomf, ws.kapf, ws.gwin, cap, (int*)dcnt, (int*)dper, (double*)dpow,
                  (double*)dbases, (int*)dstat, dmax, dmax + 1));
  } else {
    PH_TRY(dispatch(dtype, !gwin, [&](auto t, auto lw) {
      using T = decltype(t);
      return launch(c, "k_small_to_large", ph::k_small_to_large<T, decltype(lw)::value>, grid, k.block, k.lds, (const T*)dx,
                    N, thresh, n_periods, kflags, tb, geom, (T*)gbuf, (T*)gwin, cap, (int*)dcnt, (int*)dper, (double*)dpow,
                    (T*)dbases, (int*)dstat, dmax);
    }));
  }
  PH_TRY(st.finish());
  // Capacity overflow must be impossible to miss: host-pointer calls are synchronous anyway; a
  // device-pointer call reads the batch maximum back (one word, one stream synchronisation) unless
  // the caller opted out with PH_FLAG_NOSYNC and checks `status` / `counts` itself.
  if (!(flags & PH_FLAG_DEVICE) || !(flags & PH_FLAG_NOSYNC)) {
    int worst = 0;
    PH_HIP(hipMemcpyAsync(&worst, dmax, sizeof(int), hipMemcpyDeviceToHost, c->stream));
    PH_HIP(hipStreamSynchronize(c->stream));
    if (worst > cap) return fail(PH_E_CAP, "a window accepted %d periods, cap is %d", worst, cap);
  }
  return PH_OK;
}

// ----------------------------------------------------------------------------- best_correlation
int ph_best_correlation(ph_ctx* c, const void* x, int dtype, int64_t W, int N, int num, int max_length,
                        double ratio, const int32_t* orth_off, const int32_t* orth_q, int table_max_p,
                        unsigned flags, uint32_t* periods, double* norms, void* bases, int32_t* status) {
  PH_TRY(check_common(c, x, dtype, W, N));
  if (!periods || !norms || !bases || !status) return fail(PH_E_ARG, "output pointer is NULL");
  if (num < 1) return fail(PH_E_ARG, "num=%d must be >= 1", num);
  Plan pl;
  PH_TRY(resolve_best_correlation(c, dtype, N, &max_length, flags, &pl));
  PH_HIP(hipSetDevice(c->device));
  const size_t sz = elem_size(dtype);
  const KernelPlan& k = pl.k[0];
  const bool pair = k.variant == PH_PLAN_PAIR;
  void *gbuf, *gwin;
  PH_TRY(place(c, k.second, B_GBUF, (size_t)W * N * sz, &gbuf));
  PH_TRY(place(c, k.window, B_GWIN, (size_t)W * ph::win_stride(N + kPad) * sz, &gwin));
  const ph::PassPlan* plan = nullptr;
  int n_pass = 0;
  if (max_length - 1 >= 2) PH_TRY(prepare_plan(c, 2, max_length - 1, &plan, &n_pass, 4, true, pair));
  const ph::PGeom* geom;
  PH_TRY(prepare_geom(c, N, std::max(max_length, 2), &geom));
  ph::Tables tb{};
  PH_TRY(prepare_orth(c, flags, orth_off, orth_q, table_max_p, std::max(max_length, 1), &tb));
  Stage st(c, flags);
  const void* dx;
  void *dper, *dnrm, *dbases, *dstat;
  PH_TRY(st.in(x, (size_t)W * N * sz, &dx));
  PH_TRY(st.out(B_OUT0, periods, (size_t)W * num * sizeof(uint32_t), &dper));
  PH_TRY(st.out(B_OUT1, norms, (size_t)W * num * sizeof(double), &dnrm));
  PH_TRY(st.out(B_OUT2, bases, (size_t)W * num * N * sz, &dbases));
  PH_TRY(st.out(B_OUT3, status, (size_t)W * sizeof(int32_t), &dstat));
  const unsigned kflags = flags & (PH_FLAG_TRUNC | PH_FLAG_ORTH);
  const dim3 grid((unsigned)W);
  if (pair) {
    PairWs ws;
    PH_TRY(pair_workspace(c, W, N, &ws));
    PH_TRY(launch(c, "k_best_correlation", ph::k_best_correlation_pair, dim3((unsigned)((W + 1) / 2)), k.block, k.lds,
                  (const double*)dx, (int)W, N, num, max_length, ratio, geom, ws.geomf, plan, n_pass, ws.gwin, (uint32_t*)dper,
                  (double*)dnrm, (double*)dbases, (int*)dstat));
  } else {
    PH_TRY(dispatch(dtype, !gwin, [&](auto t, auto lw) {
      using T = decltype(t);
      return launch(c, "k_best_correlation", ph::k_best_correlation<T, decltype(lw)::value>, grid, k.block, k.lds,
                    (const T*)dx, N, num, max_length, ratio, kflags, tb, geom, plan, n_pass, (T*)gbuf, (T*)gwin,
                    (uint32_t*)dper, (double*)dnrm, (T*)dbases, (int*)dstat);
    }));
  }
  return st.finish();
}

// ----------------------------------------------------------------------------- best_frequency
int ph_best_frequency(ph_ctx* c, const void* x, int dtype, int64_t W, int N, int win_size, int num,
                      const int32_t* orth_off, const int32_t* orth_q, int table_max_p, unsigned flags,
                      uint32_t* periods, double* powers, void* bases, int32_t* status) {
  PH_TRY(check_common(c, x, dtype, W, N));
  if (!periods || !powers || !bases || !status) return fail(PH_E_ARG, "output pointer is NULL");
  if (num < 1) return fail(PH_E_ARG, "num=%d must be >= 1", num);
  if (W > 65535) return fail(PH_E_ARG, "ph_best_frequency: W=%lld exceeds 65535 windows per call", (long long)W);
  int L;
  Plan pl;
  BfShape g;
  PH_TRY(resolve_best_frequency(c, dtype, N, win_size, &L, &pl, &g));
  PH_HIP(hipSetDevice(c->device));
  const size_t sz = elem_size(dtype);
  const bool use_fft = pl.k[0].variant == PH_PLAN_FFT, use_chirp = pl.k[0].variant == PH_PLAN_CHIRP;
  const bool lds_window = pl.k[1].window == PH_PLAN_LDS;
  const size_t lds = pl.k[1].lds, lds_spec = g.lds_spec, lds_fft = g.lds_fft, lds_chirp = g.lds_chirp;
  const int logL = g.logL, M0 = g.M0, M = g.M, logM = g.logM, nchunk = g.nchunk, wlen = g.wlen;
  void* gbuf;
  PH_TRY(place(c, pl.k[1].second, B_GBUF, (size_t)W * N * sz, &gbuf));
  if (use_chirp && (c->bs_L != L || c->bs_M0 != M0)) {
    const long double pi = 3.141592653589793238462643383279L;
    std::vector<double> tab(2 * ((size_t)M + wlen + M));  // [twiddles M | chirp wlen | B M] as (re, im) pairs
    double* twm = tab.data();
    double* chp = twm + 2 * (size_t)M;
    double* bf = chp + 2 * (size_t)wlen;
    for (int k = 0; k < M; ++k) {
      const long double a = 2.0L * pi * (long double)k / (long double)M;
      twm[2 * (size_t)k] = (double)std::cos(a);
      twm[2 * (size_t)k + 1] = (double)std::sin(a);
    }
    for (int n = 0; n < wlen; ++n) {  // n^2 mod 2L keeps the angle exact and small
      const long double a = pi * (long double)(((long long)n * n) % (2LL * L)) / (long double)L;
      chp[2 * (size_t)n] = (double)std::cos(a);
      chp[2 * (size_t)n + 1] = (double)std::sin(a);
    }
    // B = FFT_M of the wrapped conj(w): b[m] = exp(+i pi m^2 / L) for m in [0, L/2] and at M - m for m in [1, M0)
    std::vector<long double> br((size_t)M, 0.0L), bi((size_t)M, 0.0L);
    for (int m = 0; m <= L / 2; ++m) {
      br[m] = chp[2 * (size_t)m];
      bi[m] = chp[2 * (size_t)m + 1];
    }
    for (int m = 1; m < M0; ++m) {
      br[M - m] = chp[2 * (size_t)m];
      bi[M - m] = chp[2 * (size_t)m + 1];
    }
    for (int i = 1, j = 0; i < M; ++i) {  // bit reversal, then iterative radix-2 (host, long double)
      int bit = M >> 1;
      for (; j & bit; bit >>= 1) j ^= bit;
      j ^= bit;
      if (i < j) {
        std::swap(br[i], br[j]);
        std::swap(bi[i], bi[j]);
      }
    }
    for (int len = 2; len <= M; len <<= 1) {
      const int half = len >> 1;
      for (int j = 0; j < half; ++j) {
        const long double a = -2.0L * pi * (long double)j / (long double)len;
        const long double wr = std::cos(a), wi = std::sin(a);
        for (int i = j; i < M; i += len) {
          const long double xr = br[i + half] * wr - bi[i + half] * wi, xi = br[i + half] * wi + bi[i + half] * wr;
          br[i + half] = br[i] - xr;
          bi[i + half] = bi[i] - xi;
          br[i] += xr;
          bi[i] += xi;
        }
      }
    }
    for (int k = 0; k < M; ++k) {
      bf[2 * (size_t)k] = (double)br[k];
      bf[2 * (size_t)k + 1] = (double)bi[k];
    }
    PH_HIP(hipStreamSynchronize(c->stream));
    PH_TRY(ensure(c, c->bs_tab, tab.size() * sizeof(double)));
    PH_HIP(hipMemcpyAsync(c->bs_tab.p, tab.data(), tab.size() * sizeof(double), hipMemcpyHostToDevice, c->stream));
    PH_HIP(hipStreamSynchronize(c->stream));
    c->bs_L = L;
    c->bs_M0 = M0;
  }
  ph::Tables tb{};
  PH_TRY(prepare_orth(c, flags, orth_off, orth_q, table_max_p, 2 * L, &tb));
  if (c->twid_len != L) {  // twiddles in float64; k / L is an exact fraction of a turn
    std::vector<double> tw(2 * (size_t)L);
    const long double two_pi = 6.283185307179586476925286766559L;
    for (int k = 0; k < L; ++k) {
      const long double a = two_pi * (long double)k / (long double)L;
      tw[2 * (size_t)k] = (double)std::cos(a);
      tw[2 * (size_t)k + 1] = (double)std::sin(a);
    }
    PH_HIP(hipStreamSynchronize(c->stream));
    PH_TRY(ensure(c, c->twid, tw.size() * sizeof(double)));
    PH_HIP(hipMemcpyAsync(c->twid.p, tw.data(), tw.size() * sizeof(double), hipMemcpyHostToDevice, c->stream));
    PH_HIP(hipStreamSynchronize(c->stream));
    c->twid_len = L;
  }
  Stage st(c, flags);
  const void* dx;
  void *dper, *dpow, *dbases, *dstat;
  PH_TRY(st.in(x, (size_t)W * N * sz, &dx));
  PH_TRY(st.out(B_OUT0, periods, (size_t)W * num * sizeof(uint32_t), &dper));
  PH_TRY(st.out(B_OUT1, powers, (size_t)W * num * sizeof(double), &dpow));
  PH_TRY(st.out(B_OUT2, bases, (size_t)W * num * N * sz, &dbases));
  PH_TRY(st.out(B_OUT3, status, (size_t)W * sizeof(int32_t), &dstat));
  // workspace: the residual, per-chunk spectral maxima, ||data||
  PH_TRY(ensure(c, c->buf[B_GWIN], (size_t)W * N * sz));
  PH_TRY(ensure(c, c->buf[B_WS0], (size_t)W * nchunk * sizeof(double) + (size_t)W * sizeof(double)));
  PH_TRY(ensure(c, c->buf[B_WS1], (size_t)W * nchunk * sizeof(int)));
  void* dres = c->buf[B_GWIN].p;
  double* dpart = static_cast<double*>(c->buf[B_WS0].p);
  double* dnrm = dpart + (size_t)W * nchunk;
  int* dpartk = static_cast<int*>(c->buf[B_WS1].p);
  PH_HIP(hipMemcpyAsync(dres, dx, (size_t)W * N * sz, hipMemcpyDeviceToDevice, c->stream));
  PH_HIP(hipMemsetAsync(dstat, 0, (size_t)W * sizeof(int32_t), c->stream));
  const unsigned kflags = flags & (PH_FLAG_TRUNC | PH_FLAG_ORTH);
  const dim3 grid_s((unsigned)nchunk, (unsigned)W), grid_u((unsigned)W);
  PH_TRY(dispatch(dtype, lds_window, [&](auto t, auto lw) {
    using T = decltype(t);
    constexpr bool LW = decltype(lw)::value;
    PH_TRY(allow_lds(ph::k_bf_spectrum<T, LW>, lds_spec));
    if (use_fft) PH_TRY(allow_lds(ph::k_bf_fft<T>, lds_fft));
    if (use_chirp) PH_TRY(allow_lds(ph::k_bf_chirp<T>, lds_chirp));
    PH_TRY(allow_lds(ph::k_bf_update<T, LW>, lds));
    // (the limits are raised once, above: the num iterations enqueue only)
    const double2 *twid = (const double2*)c->twid.p, *twm = (const double2*)c->bs_tab.p;
    for (int it = 0; it < num; ++it) {
      if (use_fft) {
        PH_TRY(enqueue(c, "k_bf_fft", ph::k_bf_fft<T>, grid_u, pl.k[0].block, lds_fft, (const T*)dres, N, L, logL, twid,
                       (const int*)dstat, dpart, dpartk));
      } else if (use_chirp) {
        PH_TRY(enqueue(c, "k_bf_chirp", ph::k_bf_chirp<T>, grid_u, pl.k[0].block, lds_chirp, (const T*)dres, N, L, M, logM,
                       twm, twm + M, twm + M + wlen, (const int*)dstat, dpart, dpartk));
      } else {
        PH_TRY(enqueue(c, "k_bf_spectrum", ph::k_bf_spectrum<T, LW>, grid_s, pl.k[0].block, lds_spec, (const T*)dres, N, L,
                       twid, (const int*)dstat, dpart, dpartk));
      }
      PH_TRY(enqueue(c, "k_bf_update", ph::k_bf_update<T, LW>, grid_u, pl.k[1].block, lds, (T*)dres, N, L, num, it, kflags,
                     tb, (T*)gbuf, nchunk, (const double*)dpart, (const int*)dpartk, dnrm, (uint32_t*)dper, (double*)dpow,
                     (T*)dbases, (int*)dstat));
    }
    return (int)PH_OK;
  }));
  return st.finish();
}

// ----------------------------------------------------------------------------- Ramanujan
// What a launch of k_ramanujan needs besides the data: the plan, the HBM window workspace (or nullptr) and the job
// table on the device.  ph_ramanujan_norms and ph_ramanujan_fit both prepare it here and launch through ram_enqueue.
struct RamLaunch {
  Plan pl;
  void* gwin = nullptr;
  const int* d_tab = nullptr;
  int n_root = 0;
};

static int ram_prepare(ph_ctx* c, int dtype, int64_t W, int N, int q_lo, int q_hi, RamLaunch* rl) {
  const size_t sz = elem_size(dtype);
  Plan& pl = rl->pl;
  PH_TRY(resolve_ramanujan(c, dtype, N, q_lo, q_hi, &pl));
  const KernelPlan& k = pl.k[0];
  void*& gwin = rl->gwin;
  PH_TRY(place(c, k.window, B_GWIN, (size_t)W * ph::win_stride(N + kPad) * sz, &gwin));
  // One 128-byte record per period (ph::RamJob): the factors (I - P_d) of its projector (d = q / r for each prime
  // r | q, with 1 / r and the row-split geometry of a coset count below 64), the scale (q / phi(q))^2 and the
  // geometry of its fold of the window.
  auto small_geom = [](int d) { return d >= 1 && d < 64 ? (64 / d) | (((65536 + d - 1) / d) << 8) : 0; };
  std::vector<ph::RamJob> job((size_t)q_hi + 1);
  {
    std::vector<int32_t> phi(q_hi + 1);
    for (int i = 0; i <= q_hi; ++i) phi[i] = i;
    std::vector<std::vector<int32_t>> primes_of(q_hi + 1);
    std::vector<char> comp(q_hi + 1, 0);
    for (int i = 2; i <= q_hi; ++i) {
      if (comp[i]) continue;
      for (int j = i; j <= q_hi; j += i) {
        comp[j] = j > i;
        phi[j] -= phi[j] / i;
        primes_of[j].push_back(i);
      }
    }
    for (int q = 1; q <= q_hi; ++q) {
      ph::RamJob& J = job[q];
      std::memset(&J, 0, sizeof(J));
      J.q = q;
      J.k = 1;
      J.rows = (N + q - 1) / q;            // as PGeom: residues j < nfull own `rows` samples, the others rows - 1
      J.nfull = N - (J.rows - 1) * q;
      J.sm = small_geom(q);
      const double sc = (double)q / (double)phi[q];
      J.scale2 = sc * sc;
      int ns = 0;
      for (int r : primes_of[q]) {
        J.st[ns].dr = (q / r) | (r << 16);
        J.st[ns].sm = small_geom(q / r);
        J.st[ns].inv_r = 1.0 / (double)r;
        ++ns;
      }
      J.flags = ns << 8;
    }
  }
  // Root plan: roots are the periods of (q_hi/2, q_hi]; every wanted q <= q_hi/2 becomes the child of one
  // of its multiples there (the least loaded one; children cost a strip fold and a filter, O(Q + q)).
  // Roots are dealt to the wavefronts in order of decreasing work.
  std::vector<ph::RamJob> tab;  // root records, then the children
  int& n_root = rl->n_root;
  n_root = 0;
  if (q_lo <= q_hi) {
    const int half = q_hi / 2;
    std::vector<std::vector<int32_t>> kids((size_t)q_hi + 1);
    std::vector<int64_t> load((size_t)q_hi + 1, 0);
    for (int Q = half + 1; Q <= q_hi; ++Q) load[Q] = (int64_t)N + Q;
    for (int q = std::min(half, q_hi); q >= q_lo; --q) {
      int best = 0;
      for (int Q = ((half / q) + 1) * q; Q <= q_hi; Q += q)
        if (!best || load[Q] < load[best]) best = Q;
      kids[best].push_back(q);
      load[best] += 2 * (int64_t)best + 4 * q;
    }
    std::vector<int> order;
    for (int Q = half + 1; Q <= q_hi; ++Q)
      if (Q >= q_lo || !kids[Q].empty()) order.push_back(Q);
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return load[a] > load[b]; });
    n_root = (int)order.size();
    tab.resize((size_t)n_root);
    for (int i = 0; i < n_root; ++i) {
      const int Q = order[i];
      ph::RamJob R = job[Q];
      R.c0 = (int32_t)(tab.size() - (size_t)n_root);
      for (int q : kids[Q]) {
        ph::RamJob C = job[q];
        C.k = Q / q;
        tab.push_back(C);
      }
      R.c1 = (int32_t)(tab.size() - (size_t)n_root);
      R.flags |= Q >= q_lo ? 1 : 0;
      tab[i] = R;
    }
  }
  if (tab.empty()) tab.push_back(ph::RamJob{});
  // the records travel as raw int32 words through a cached table slot
  PH_TRY(upload_table(c, T_AUX2, reinterpret_cast<const int32_t*>(tab.data()), tab.size() * (sizeof(ph::RamJob) / 4), &rl->d_tab));
  return PH_OK;
}

// zero the norms, then one k_ramanujan launch on the context's stream
static int ram_enqueue(ph_ctx* c, const RamLaunch& rl, int dtype, int64_t W, int N, int q_hi, const void* dx, void* dout) {
  const KernelPlan& k = rl.pl.k[0];
  void* gwin = rl.gwin;
  const int n_root = rl.n_root;
  PH_HIP(hipMemsetAsync(dout, 0, (size_t)W * (q_hi + 1) * sizeof(double), c->stream));
  const dim3 grid((unsigned)W);
  if (n_root > 0) {
    const ph::RamJob* d_roots = reinterpret_cast<const ph::RamJob*>(rl.d_tab);
    PH_TRY(dispatch(dtype, !gwin, [&](auto t, auto lw) {
      using T = decltype(t);
      return launch(c, "k_ramanujan", ph::k_ramanujan<T, decltype(lw)::value>, grid, k.block, k.lds, (const T*)dx, N, q_hi,
                    d_roots, n_root, d_roots + n_root, (T*)gwin, k.pad, (double*)dout);
    }));
  }
  return PH_OK;
}

int ph_ramanujan_norms(ph_ctx* c, const void* x, int dtype, int64_t W, int N, int q_lo, int q_hi,
                       unsigned flags, double* out) {
  PH_TRY(check_common(c, x, dtype, W, N));
  if (!out) return fail(PH_E_ARG, "out is NULL");
  PH_HIP(hipSetDevice(c->device));
  const size_t sz = elem_size(dtype);
  RamLaunch rl;
  PH_TRY(ram_prepare(c, dtype, W, N, q_lo, q_hi, &rl));
  Stage st(c, flags);
  const void* dx;
  void* dout;
  PH_TRY(st.in(x, (size_t)W * N * sz, &dx));
  PH_TRY(st.out(B_OUT0, out, (size_t)W * (q_hi + 1) * sizeof(double), &dout));
  PH_TRY(ram_enqueue(c, rl, dtype, W, N, q_hi, dx, dout));
  return st.finish();
}

// ----------------------------------------------------------------------------- QOPeriods blocks
static int qo_tables(ph_ctx* c, const int32_t* p_list, const int32_t* keep, int n_p, const int** d_p,
                     const int** d_keep, const int** d_off, int* stride) {
  if (!p_list || !keep || n_p < 1) return fail(PH_E_ARG, "p_list/keep NULL or n_p < 1");
  std::vector<int32_t> off(n_p + 1, 0);
  for (int k = 0; k < n_p; ++k) {
    if (p_list[k] < 1 || keep[k] < 0 || keep[k] > p_list[k])
      return fail(PH_E_ARG, "need p >= 1 and 0 <= keep <= p at entry %d", k);
    off[k + 1] = off[k] + keep[k];
  }
  *stride = off[n_p];
  if (*stride < 1) return fail(PH_E_ARG, "sum(keep) must be >= 1");
  PH_TRY(upload_table(c, T_PLIST, p_list, n_p, d_p));
  PH_TRY(upload_table(c, T_AUX0, keep, n_p, d_keep));
  PH_TRY(upload_table(c, T_AUX1, off.data(), off.size(), d_off));
  return PH_OK;
}

int ph_fold_sums(ph_ctx* c, const void* x, int dtype, int64_t W, int N, const int32_t* p_list,
                 const int32_t* keep, int n_p, unsigned flags, double* out) {
  PH_TRY(check_common(c, x, dtype, W, N));
  if (!out) return fail(PH_E_ARG, "out is NULL");
  PH_HIP(hipSetDevice(c->device));
  const size_t sz = elem_size(dtype);
  Plan pl;
  plan_fold_sums(c, dtype, N, &pl);
  const bool lds_window = pl.k[0].window == PH_PLAN_LDS;
  const size_t lds = pl.k[0].lds;
  const int *d_p, *d_keep, *d_off;
  int stride;
  PH_TRY(qo_tables(c, p_list, keep, n_p, &d_p, &d_keep, &d_off, &stride));
  Stage st(c, flags);
  const void* dx;
  void* dout;
  PH_TRY(st.in(x, (size_t)W * N * sz, &dx));
  PH_TRY(st.out(B_OUT0, out, (size_t)W * stride * sizeof(double), &dout));
  const dim3 grid((unsigned)W);
  PH_TRY(dispatch(dtype, lds_window, [&](auto t, auto lw) {
    using T = decltype(t);
    return launch(c, "k_fold_sums", ph::k_fold_sums<T, decltype(lw)::value>, grid, pl.k[0].block, lds, (const T*)dx, N, d_p,
                  d_keep, d_off, n_p, stride, (double*)dout);
  }));
  return st.finish();
}

int ph_tile_sum(ph_ctx* c, const double* wts, int64_t W, int N, const int32_t* p_list, const int32_t* keep,
                int n_p, int dtype, unsigned flags, void* out) {
  PH_TRY(check_common(c, wts, dtype, W, N));
  if (!out) return fail(PH_E_ARG, "out is NULL");
  PH_HIP(hipSetDevice(c->device));
  const size_t sz = elem_size(dtype);
  const int *d_p, *d_keep, *d_off;
  int stride;
  PH_TRY(qo_tables(c, p_list, keep, n_p, &d_p, &d_keep, &d_off, &stride));
  const size_t lds = ph::stage_carve<double>(CarveCount(), stride).bytes;
  PH_TRY(check_lds(c, lds, N, "ph_tile_sum"));
  Stage st(c, flags);
  const void* dw;
  void* dout;
  PH_TRY(st.in(wts, (size_t)W * stride * sizeof(double), &dw));
  PH_TRY(st.out(B_OUT0, out, (size_t)W * N * sz, &dout));
  const dim3 grid((unsigned)W);
  PH_TRY(dispatch(dtype, [&](auto t) {
    using T = decltype(t);
    return launch(c, "k_tile_sum", ph::k_tile_sum<T>, grid, kBlock, lds, (const double*)dw, N, d_p, d_keep, d_off, n_p, stride,
                  (T*)dout);
  }));
  return st.finish();
}

// ----------------------------------------------------------------------------- periodic_norm
int ph_periodic_norm(ph_ctx* c, const void* x, int dtype, int64_t W, int N, int p, unsigned flags,
                     double* out) {
  PH_TRY(check_common(c, x, dtype, W, N));
  if (!out) return fail(PH_E_ARG, "out is NULL");
  if (p < 0) return fail(PH_E_ARG, "p=%d must be >= 0 (0 = no period normalisation)", p);
  PH_HIP(hipSetDevice(c->device));
  const size_t sz = elem_size(dtype);
  Stage st(c, flags);
  const void* dx;
  void* dout;
  PH_TRY(st.in(x, (size_t)W * N * sz, &dx));
  PH_TRY(st.out(B_OUT0, out, (size_t)W * sizeof(double), &dout));
  const dim3 grid((unsigned)W);
  PH_TRY(dispatch(dtype, [&](auto t) {
    using T = decltype(t);
    return launch(c, "k_periodic_norm", ph::k_periodic_norm<T>, grid, kBlock, 0, (const T*)dx, N, p, (double*)dout);
  }));
  return st.finish();
}

// ----------------------------------------------------------------------------- dictionary project
int ph_dict_project(ph_ctx* c, const double* x, const double* basis, int rows, int N, unsigned flags,
                    float* out) {
  if (!c || !x || !basis || !out) return fail(PH_E_ARG, "NULL argument");
  if (rows < 1 || N < 1) return fail(PH_E_ARG, "rows=%d, N=%d must be >= 1", rows, N);
  PH_HIP(hipSetDevice(c->device));
  const bool device = flags & PH_FLAG_DEVICE;
  const double *dx = x, *db = basis;
  float* dout = out;
  if (!device) {
    PH_TRY(ensure(c, c->buf[B_IN], (size_t)N * 8));
    PH_TRY(ensure(c, c->buf[B_WS1], (size_t)rows * N * 8));
    PH_TRY(ensure(c, c->buf[B_OUT0], (size_t)rows * N * 4));
    PH_HIP(hipMemcpyAsync(c->buf[B_IN].p, x, (size_t)N * 8, hipMemcpyHostToDevice, c->stream));
    PH_HIP(hipMemcpyAsync(c->buf[B_WS1].p, basis, (size_t)rows * N * 8, hipMemcpyHostToDevice, c->stream));
    dx = (const double*)c->buf[B_IN].p;
    db = (const double*)c->buf[B_WS1].p;
    dout = (float*)c->buf[B_OUT0].p;
  }
  PH_TRY(launch(c, "k_dict_project", ph::k_dict_project, dim3((unsigned)rows), kBlock, 0, dx, db, N, dout));
  if (!device) {
    PH_HIP(hipMemcpyAsync(out, dout, (size_t)rows * N * 4, hipMemcpyDeviceToHost, c->stream));
    PH_HIP(hipStreamSynchronize(c->stream));
  }
  return PH_OK;
}

// ----------------------------------------------------------------------------- QOPeriods.find_periods
// ph_qo_find_periods (window == nullptr) and ph_qo_greedy_win (the fixed-weight loop under `window`): one set of
// argument checks, tables and staging
static int qo_find_run(ph_ctx* c, const void* x, int dtype, int64_t W, int N, const double* window, int num, double thresh,
                       int min_length, int max_length, int kcap, unsigned flags, uint32_t* periods,
                       double* norms, int32_t* keeps, int32_t* counts, double* weights, void* residual,
                       int32_t* status) {
  PH_TRY(check_common(c, x, dtype, W, N));
  if (!periods || !norms || !keeps || !counts || !weights || !residual || !status)
    return fail(PH_E_ARG, "output pointer is NULL");
  const bool trunc = flags & PH_FLAG_TRUNC;
  const bool keep_weights = flags & PH_FLAG_KEEP_WEIGHTS;
  if (num < 1) return fail(PH_E_ARG, "num=%d must be >= 1", num);
  size_t lds;
  int placement;
  PH_TRY(qo_plan(c, dtype, N, &max_length, kcap, flags, &lds, &placement));
  if (min_length < 1 || max_length < min_length)
    return fail(PH_E_ARG, "need 1 <= min_length <= max_length (got %d, %d)", min_length, max_length);
  PH_HIP(hipSetDevice(c->device));
  const size_t sz = elem_size(dtype);
  const bool lds_window = placement != PH_QO_HBM, overlay = placement == PH_QO_LDS_OVERLAY;
  void* gwin = nullptr;
  if (!lds_window) {
    PH_TRY(ensure(c, c->buf[B_GWIN], (size_t)W * ph::win_stride(N + kPad) * sz));
    gwin = c->buf[B_GWIN].p;
  }
  const ph::PGeom* geom;
  PH_TRY(prepare_geom(c, N, max_length, &geom));
  const ph::PassPlan* plan;
  int n_pass;
  PH_TRY(prepare_plan(c, min_length, max_length, &plan, &n_pass));
  // Euler phi and all divisors of every candidate period (QOPeriods.py:834-838)
  std::vector<int32_t> phi, off, dq;
  divisor_tables(max_length, &phi, &off, &dq);
  const int *d_phi, *d_off, *d_dq;
  PH_TRY(upload_table(c, T_AUX0, phi.data(), phi.size(), &d_phi));
  PH_TRY(upload_table(c, T_AUX1, off.data(), off.size(), &d_off));
  PH_TRY(upload_table(c, T_AUX2, dq.data(), dq.size(), &d_dq));
  if (!keep_weights)  // last good weights + rhs of every window
    PH_TRY(ensure(c, c->buf[B_WS1], (size_t)W * 2 * kcap * sizeof(double)));
  else  // divisor bitset of every window
    PH_TRY(ensure(c, c->buf[B_WS1], (size_t)W * ((max_length + 32) / 32) * sizeof(uint32_t)));
  Stage st(c, flags);
  const void* dx;
  void *dper, *dnrm, *dkeep, *dcnt, *dwts, *dres, *dstat;
  const void* dwin = nullptr;
  PH_TRY(st.in(x, (size_t)W * N * sz, &dx));
  if (window) PH_TRY(st.in(window, (size_t)N * sizeof(double), &dwin, B_GBUF));
  PH_TRY(st.out(B_OUT0, periods, (size_t)W * num * sizeof(uint32_t), &dper));
  PH_TRY(st.out(B_OUT1, norms, (size_t)W * num * sizeof(double), &dnrm));
  PH_TRY(st.out(B_OUT2, keeps, (size_t)W * num * sizeof(int32_t), &dkeep));
  PH_TRY(st.out(B_OUT3, counts, (size_t)W * 2 * sizeof(int32_t), &dcnt));
  PH_TRY(st.out(B_OUT4, weights, (size_t)W * kcap * sizeof(double), &dwts));
  PH_TRY(st.out(B_WS0, residual, (size_t)W * N * sz, &dres));
  PH_TRY(st.out(B_GEN0, status, (size_t)W * sizeof(int32_t), &dstat));
  const dim3 grid((unsigned)W);
  const char* name = window ? "k_qo_greedy_win" : keep_weights ? "k_qo_greedy" : "k_qo_find";
  PH_TRY(dispatch(dtype, lds_window, [&](auto t, auto lw) {
    using T = decltype(t);
    constexpr bool LW = decltype(lw)::value;
    if (keep_weights) {
      auto kernel = window ? (trunc ? ph::k_qo_greedy<T, LW, true, true> : ph::k_qo_greedy<T, LW, false, true>)
                           : (trunc ? ph::k_qo_greedy<T, LW, true> : ph::k_qo_greedy<T, LW, false>);
      return launch(c, name, kernel, grid, c->qo_block, lds, (const T*)dx, N, num, thresh, min_length, max_length, geom, plan,
                    n_pass, d_phi, d_off, d_dq, kcap, (T*)gwin, (uint32_t*)c->buf[B_WS1].p, (uint32_t*)dper, (double*)dnrm,
                    (int*)dkeep, (int*)dcnt, (double*)dwts, (T*)dres, (int*)dstat, (const double*)dwin);
    }
    auto kernel = trunc ? ph::k_qo_find<T, LW, true> : ph::k_qo_find<T, LW>;
    return launch(c, name, kernel, grid, c->qo_block, lds, (const T*)dx, N, num, thresh, min_length, max_length, geom, plan,
                  n_pass, d_phi, d_off, d_dq, kcap, overlay ? 1 : 0, (T*)gwin, (double*)c->buf[B_WS1].p, (uint32_t*)dper,
                  (double*)dnrm, (int*)dkeep, (int*)dcnt, (double*)dwts, (T*)dres, (int*)dstat);
  }));
  return st.finish();
}

int ph_qo_find_periods(ph_ctx* c, const void* x, int dtype, int64_t W, int N, int num, double thresh,
                       int min_length, int max_length, int kcap, unsigned flags, uint32_t* periods,
                       double* norms, int32_t* keeps, int32_t* counts, double* weights, void* residual,
                       int32_t* status) {
  return qo_find_run(c, x, dtype, W, N, nullptr, num, thresh, min_length, max_length, kcap, flags, periods, norms, keeps,
                     counts, weights, residual, status);
}

int ph_qo_greedy_win(ph_ctx* c, const void* x, int dtype, int64_t W, int N, const double* window, int num, double thresh,
                     int min_length, int max_length, int kcap, unsigned flags, uint32_t* periods, double* norms,
                     int32_t* keeps, int32_t* counts, double* weights, void* residual, int32_t* status) {
  PH_TRY(check_common(c, x, dtype, W, N));
  if (!window) return fail(PH_E_ARG, "ph_qo_greedy_win: window is NULL (ph_qo_find_periods fits without a window)");
  return qo_find_run(c, x, dtype, W, N, window, num, thresh, min_length, max_length, kcap, flags | PH_FLAG_KEEP_WEIGHTS,
                     periods, norms, keeps, counts, weights, residual, status);
}

int ph_qo_feasible(ph_ctx* c, int dtype, int N, int max_length, int kcap, int* ok) {
  if (!c || !ok) return fail(PH_E_ARG, "NULL argument");
  *ok = 0;
  if (N < 1 || kcap < 1 || kcap > 2048) return PH_OK;
  if (max_length < 0) max_length = N / 3;
  size_t lds;
  int placement;
  if (qo_lds_layout(c, dtype, N, max_length, kcap, &lds, &placement) == PH_OK) *ok = 1;
  return PH_OK;
}

int ph_qo_plan_info(ph_ctx* c, int dtype, int N, int max_length, int kcap, unsigned flags, int* lds_bytes,
                    int* placement) {
  if (!c || !lds_bytes || !placement) return fail(PH_E_ARG, "NULL argument");
  if (dtype != PH_F64 && dtype != PH_F32) return fail(PH_E_ARG, "dtype must be PH_F64 or PH_F32");
  if (N < 1) return fail(PH_E_ARG, "N=%d must be >= 1", N);
  size_t lds;
  PH_TRY(qo_plan(c, dtype, N, &max_length, kcap, flags, &lds, placement));
  *lds_bytes = (int)lds;
  return PH_OK;
}

// ----------------------------------------------------------------------------- fit of a given period list
// Checks shared by ph_qo_fit and ph_ramanujan_fit, the plan, and the phi / divisor tables of 1 .. max_period on the
// device (slots of their own: the Ramanujan job table stays where it is while both kernels are queued).
struct FitLaunch {
  Plan pl;
  const int *d_phi = nullptr, *d_off = nullptr, *d_dq = nullptr;
};

static int fit_prepare(ph_ctx* c, int N, bool windowed, int pcap, int max_period, int kcap, FitLaunch* fl) {
  if (pcap < 1 || pcap > (1 << 20)) return fail(PH_E_ARG, "pcap=%d must be in [1, 2^20]", pcap);
  if (windowed)
    PH_TRY(plan_qo_fit_win(c, N, kcap, max_period, &fl->pl));
  else
    PH_TRY(plan_qo_fit(c, kcap, max_period, &fl->pl));
  std::vector<int32_t> phi, off, dq;
  divisor_tables(max_period, &phi, &off, &dq);
  PH_TRY(upload_table(c, T_FIT_PHI, phi.data(), phi.size(), &fl->d_phi));
  PH_TRY(upload_table(c, T_FIT_OFF, off.data(), off.size(), &fl->d_off));
  PH_TRY(upload_table(c, T_FIT_DQ, dq.data(), dq.size(), &fl->d_dq));
  return PH_OK;
}

static int fit_enqueue(ph_ctx* c, const FitLaunch& fl, int dtype, int64_t W, int N, const void* dx, const int* dper,
                       const int* dnper, int pcap, int per_stride, int max_period, int kcap, void* dkeep, void* dwts,
                       void* dres, void* dstat) {
  const KernelPlan& k = fl.pl.k[0];
  const dim3 grid((unsigned)W);
  return dispatch(dtype, [&](auto t) {
    using T = decltype(t);
    return launch(c, "k_qo_fit", ph::k_qo_fit<T>, grid, k.block, k.lds, (const T*)dx, N, dper, dnper, pcap, per_stride,
                  max_period, fl.d_phi, fl.d_off, fl.d_dq, kcap, (int*)dkeep, (double*)dwts, (T*)dres, (int*)dstat);
  });
}

// k_qo_fit_win: `dwin` the analysis window on the device, `dws` the HBM workspace of u (nullptr when the plan keeps u in LDS)
static int fit_win_enqueue(ph_ctx* c, const FitLaunch& fl, int dtype, int64_t W, int N, const void* dx, const double* dwin,
                           const int* dper, const int* dnper, int pcap, int per_stride, int max_period, int kcap,
                           double* dws, void* dkeep, void* dwts, void* dres, void* dstat) {
  const KernelPlan& k = fl.pl.k[0];
  const dim3 grid((unsigned)W);
  return dispatch(dtype, k.second == PH_PLAN_LDS, [&](auto t, auto ul) {
    using T = decltype(t);
    return launch(c, "k_qo_fit_win", ph::k_qo_fit_win<T, decltype(ul)::value>, grid, k.block, k.lds, (const T*)dx, N, dwin,
                  dper, dnper, pcap, per_stride, max_period, fl.d_phi, fl.d_off, fl.d_dq, kcap, dws, (int*)dkeep,
                  (double*)dwts, (T*)dres, (int*)dstat);
  });
}

// ph_qo_fit (window == nullptr) and ph_qo_fit_win: one set of argument checks, tables and staging
static int qo_fit_run(ph_ctx* c, const void* x, int dtype, int64_t W, int N, const double* window, const int32_t* periods,
                      const int32_t* n_periods, int pcap, int per_stride, int max_period, int kcap, unsigned flags,
                      int32_t* keeps, double* weights, void* residual, int32_t* status) {
  PH_TRY(check_common(c, x, dtype, W, N));
  if (!periods || !n_periods) return fail(PH_E_ARG, "periods / n_periods is NULL");
  if (!keeps || !weights || !residual || !status) return fail(PH_E_ARG, "output pointer is NULL");
  if (per_stride != 0 && per_stride < pcap) return fail(PH_E_ARG, "per_stride=%d must be 0 (one shared list) or >= pcap=%d", per_stride, pcap);
  PH_HIP(hipSetDevice(c->device));
  FitLaunch fl;
  PH_TRY(fit_prepare(c, N, window != nullptr, pcap, max_period, kcap, &fl));
  const size_t sz = elem_size(dtype);
  const size_t lists = per_stride ? (size_t)W : 1;
  Stage st(c, flags);
  const void *dx, *dper, *dnper, *dwin = nullptr;
  void *dkeep, *dwts, *dres, *dstat, *dws = nullptr;
  PH_TRY(st.in(x, (size_t)W * N * sz, &dx));
  PH_TRY(st.in(periods, ((lists - 1) * (size_t)per_stride + pcap) * sizeof(int32_t), &dper, B_GBUF));
  PH_TRY(st.in(n_periods, lists * sizeof(int32_t), &dnper, B_WS1));
  if (window) {
    PH_TRY(st.in(window, (size_t)N * sizeof(double), &dwin, B_GWIN));
    PH_TRY(place(c, fl.pl.k[0].second, B_OUT0, (size_t)W * N * sizeof(double), &dws));
  }
  PH_TRY(st.out(B_OUT3, keeps, (size_t)W * pcap * sizeof(int32_t), &dkeep));
  PH_TRY(st.out(B_OUT4, weights, (size_t)W * kcap * sizeof(double), &dwts));
  PH_TRY(st.out(B_WS0, residual, (size_t)W * N * sz, &dres));
  PH_TRY(st.out(B_GEN0, status, (size_t)W * sizeof(int32_t), &dstat));
  if (window)
    PH_TRY(fit_win_enqueue(c, fl, dtype, W, N, dx, (const double*)dwin, (const int*)dper, (const int*)dnper, pcap, per_stride,
                           max_period, kcap, (double*)dws, dkeep, dwts, dres, dstat));
  else
    PH_TRY(fit_enqueue(c, fl, dtype, W, N, dx, (const int*)dper, (const int*)dnper, pcap, per_stride, max_period, kcap, dkeep,
                       dwts, dres, dstat));
  return st.finish();
}

int ph_qo_fit(ph_ctx* c, const void* x, int dtype, int64_t W, int N, const int32_t* periods, const int32_t* n_periods,
              int pcap, int per_stride, int max_period, int kcap, unsigned flags, int32_t* keeps, double* weights,
              void* residual, int32_t* status) {
  return qo_fit_run(c, x, dtype, W, N, nullptr, periods, n_periods, pcap, per_stride, max_period, kcap, flags, keeps, weights,
                    residual, status);
}

int ph_qo_fit_win(ph_ctx* c, const void* x, int dtype, int64_t W, int N, const double* window, const int32_t* periods,
                  const int32_t* n_periods, int pcap, int per_stride, int max_period, int kcap, unsigned flags,
                  int32_t* keeps, double* weights, void* residual, int32_t* status) {
  if (!window) return fail(PH_E_ARG, "ph_qo_fit_win: window is NULL (ph_qo_fit fits without a window)");
  return qo_fit_run(c, x, dtype, W, N, window, periods, n_periods, pcap, per_stride, max_period, kcap, flags, keeps, weights,
                    residual, status);
}

int ph_ramanujan_fit(ph_ctx* c, const void* x, int dtype, int64_t W, int N, int q_lo, int q_hi, double thresh, int pcap,
                     int kcap, unsigned flags, double* norms, int32_t* periods, int32_t* counts, int32_t* keeps,
                     double* weights, void* residual, int32_t* status) {
  if (!(thresh > 0.0)) return fail(PH_E_ARG, "thresh=%g must be > 0 (index 0 would be selected)", thresh);
  PH_TRY(check_common(c, x, dtype, W, N));
  if (!norms || !periods || !counts || !keeps || !weights || !residual || !status)
    return fail(PH_E_ARG, "output pointer is NULL");
  PH_HIP(hipSetDevice(c->device));
  RamLaunch rl;
  PH_TRY(ram_prepare(c, dtype, W, N, q_lo, q_hi, &rl));
  FitLaunch fl;
  PH_TRY(fit_prepare(c, N, false, pcap, q_hi, kcap, &fl));
  const size_t sz = elem_size(dtype);
  Stage st(c, flags);
  const void* dx;
  void *dnrm, *dper, *dcnt, *dkeep, *dwts, *dres, *dstat;
  PH_TRY(st.in(x, (size_t)W * N * sz, &dx));
  PH_TRY(st.out(B_OUT0, norms, (size_t)W * (q_hi + 1) * sizeof(double), &dnrm));
  PH_TRY(st.out(B_OUT1, periods, (size_t)W * pcap * sizeof(int32_t), &dper));
  PH_TRY(st.out(B_OUT2, counts, (size_t)W * sizeof(int32_t), &dcnt));
  PH_TRY(st.out(B_OUT3, keeps, (size_t)W * pcap * sizeof(int32_t), &dkeep));
  PH_TRY(st.out(B_OUT4, weights, (size_t)W * kcap * sizeof(double), &dwts));
  PH_TRY(st.out(B_WS0, residual, (size_t)W * N * sz, &dres));
  PH_TRY(st.out(B_GEN0, status, (size_t)W * sizeof(int32_t), &dstat));
  // three launches on the context's stream, no host round trip between them
  PH_TRY(ram_enqueue(c, rl, dtype, W, N, q_hi, dx, dnrm));
  PH_TRY(launch(c, "k_ram_select", ph::k_ram_select, dim3((unsigned)W), ph::kWave, 0, (const double*)dnrm, q_hi, thresh, pcap,
                (int*)dper, (int*)dcnt));
  PH_TRY(fit_enqueue(c, fl, dtype, W, N, dx, (const int*)dper, (const int*)dcnt, pcap, pcap, q_hi, kcap, dkeep, dwts, dres,
                     dstat));
  return st.finish();
}

// ----------------------------------------------------------------------------- capped selection from given norms
int ph_ramanujan_select(ph_ctx* c, const double* norms, int64_t W, int q_hi, double thresh, const double* ref, int pcap,
                        unsigned flags, int32_t* periods, int32_t* counts, int32_t* over) {
  if (!c) return fail(PH_E_ARG, "ctx is NULL");
  if (!norms) return fail(PH_E_ARG, "norms is NULL");
  if (!periods || !counts || !over) return fail(PH_E_ARG, "output pointer is NULL");
  if (W < 1 || W > 0x7fffffffLL / 64) return fail(PH_E_ARG, "W=%lld out of range", (long long)W);
  if (q_hi < 1) return fail(PH_E_ARG, "need q_hi >= 1 (got %d)", q_hi);
  if (q_hi >= 30030 || q_hi > 0xffff)
    return fail(PH_E_ARG, "ph_ramanujan_select: q_hi=%d is beyond the record format of ph_ramanujan_norms", q_hi);
  if (pcap < 1 || pcap > (1 << 20)) return fail(PH_E_ARG, "pcap=%d must be in [1, 2^20]", pcap);
  if (!(thresh > 0.0)) return fail(PH_E_ARG, "thresh=%g must be > 0 (index 0 would be selected)", thresh);
  // W < 2^25, q_hi + 1 <= 30030 and pcap <= 2^20: every byte count below stays under 2^48
  static_assert(sizeof(size_t) >= 8, "byte counts are 64-bit");
  PH_HIP(hipSetDevice(c->device));
  Stage st(c, flags);
  const void *dnrm, *dref = nullptr;
  void *dper, *dcnt, *dover;
  PH_TRY(st.in(norms, (size_t)W * ((size_t)q_hi + 1) * sizeof(double), &dnrm));
  if (ref) PH_TRY(st.in(ref, (size_t)W * sizeof(double), &dref, B_GWIN));
  PH_TRY(st.out(B_OUT1, periods, (size_t)W * (size_t)pcap * sizeof(int32_t), &dper));
  PH_TRY(st.out(B_OUT2, counts, (size_t)W * sizeof(int32_t), &dcnt));
  PH_TRY(st.out(B_OUT3, over, (size_t)W * sizeof(int32_t), &dover));
  PH_TRY(launch(c, "k_ram_select_ref", ph::k_ram_select_ref, dim3((unsigned)W), ph::kWave, 0, (const double*)dnrm, q_hi,
                thresh, (const double*)dref, pcap, (int*)dper, (int*)dcnt, (int*)dover));
  return st.finish();
}

// ----------------------------------------------------------------------------- orthogonal period powers
int ph_orth_powers(ph_ctx* c, const void* x, int dtype, int64_t W, int N, int max_p, int normalize,
                   unsigned flags, double* autocorr, double* eq3, double* powers) {
  PH_TRY(check_common(c, x, dtype, W, N));
  if (!powers) return fail(PH_E_ARG, "powers is NULL");
  Plan pl;
  PH_TRY(resolve_orth_powers(c, dtype, N, &max_p, &pl));
  PH_HIP(hipSetDevice(c->device));
  const size_t sz = elem_size(dtype);
  const bool lds_window = pl.k[0].window == PH_PLAN_LDS;
  const size_t lds = pl.k[0].lds;
  void* gws;
  PH_TRY(place(c, pl.k[0].second, B_WS1, (size_t)W * ((size_t)N + max_p) * sizeof(double), &gws));
  const int *d_off, *d_d, *d_mu;
  PH_TRY(prepare_mobius(c, max_p, &d_off, &d_d, &d_mu));
  Stage st(c, flags);
  const void* dx;
  void *dr, *de, *dp;
  PH_TRY(st.in(x, (size_t)W * N * sz, &dx));
  PH_TRY(st.out(B_OUT0, autocorr, (size_t)W * N * sizeof(double), &dr));
  PH_TRY(st.out(B_OUT1, eq3, (size_t)W * max_p * sizeof(double), &de));
  PH_TRY(st.out(B_OUT2, powers, (size_t)W * max_p * sizeof(double), &dp));
  const dim3 grid((unsigned)W);
  PH_TRY(dispatch(dtype, lds_window, [&](auto t, auto lw) {
    using T = decltype(t);
    return launch(c, "k_orth_powers", ph::k_orth_powers<T, decltype(lw)::value>, grid, pl.k[0].block, lds, (const T*)dx, N,
                  max_p, normalize, d_off, d_d, d_mu, (double*)gws, (double*)dr, (double*)de, (double*)dp);
  }));
  return st.finish();
}

// ----------------------------------------------------------------------------- orthogonal selection step
int ph_qo_orth_select(ph_ctx* c, const void* x, int dtype, int64_t W, int N, int max_p, const int32_t* orth_off,
                      const int32_t* orth_q, int table_max_p, unsigned flags, int32_t* period, double* norm,
                      double* powers, int32_t* status) {
  PH_TRY(check_common(c, x, dtype, W, N));
  if (!period || !norm || !status) return fail(PH_E_ARG, "period/norm/status is NULL");
  Plan pl;
  PH_TRY(plan_qo_orth_select(c, dtype, N, max_p, &pl));
  if (table_max_p < max_p - 1)
    return fail(PH_E_ARG, "ph_qo_orth_select: orth tables cover p <= %d, need %d", table_max_p, max_p - 1);
  PH_HIP(hipSetDevice(c->device));
  const size_t sz = elem_size(dtype);
  const bool lds_window = pl.k[0].window == PH_PLAN_LDS;
  const size_t lds = pl.k[0].lds;
  void* gws;
  PH_TRY(place(c, pl.k[0].second, B_WS1, (size_t)W * ((size_t)N + max_p) * sizeof(double), &gws));
  ph::Tables tb{};
  PH_TRY(prepare_orth(c, PH_FLAG_ORTH, orth_off, orth_q, table_max_p, max_p - 1, &tb));
  const int *d_off, *d_d, *d_mu;
  PH_TRY(prepare_mobius(c, max_p, &d_off, &d_d, &d_mu));
  Stage st(c, flags);
  const void* dx;
  void *dper, *dnrm, *dpow, *dstat;
  PH_TRY(st.in(x, (size_t)W * N * sz, &dx));
  PH_TRY(st.out(B_OUT0, period, (size_t)W * sizeof(int32_t), &dper));
  PH_TRY(st.out(B_OUT1, norm, (size_t)W * sizeof(double), &dnrm));
  PH_TRY(st.out(B_OUT2, powers, (size_t)W * max_p * sizeof(double), &dpow));
  PH_TRY(st.out(B_OUT3, status, (size_t)W * sizeof(int32_t), &dstat));
  const unsigned kflags = flags & PH_FLAG_TRUNC;
  const dim3 grid((unsigned)W);
  PH_TRY(dispatch(dtype, lds_window, [&](auto t, auto lw) {
    using T = decltype(t);
    return launch(c, "k_qo_orth_select", ph::k_qo_orth_select<T, decltype(lw)::value>, grid, pl.k[0].block, lds,
                  (const T*)dx, N, max_p, kflags, tb, d_off, d_d, d_mu, (double*)gws, (int*)dper, (double*)dnrm, (double*)dpow,
                  (int*)dstat);
  }));
  return st.finish();
}

// ----------------------------------------------------------------------------- QOPeriods.get_periods
int ph_qo_get_periods(ph_ctx* c, const int32_t* periods, const int32_t* rows, const int32_t* counts, int64_t W, int pcap,
                      const double* weights, int kcap, int max_period, int ccap, unsigned flags, double* out,
                      int32_t* status) {
  if (!c) return fail(PH_E_ARG, "ctx is NULL");
  if (!periods || !rows || !counts || !weights) return fail(PH_E_ARG, "periods / rows / counts / weights is NULL");
  if (!out || !status) return fail(PH_E_ARG, "output pointer is NULL");
  if (W < 1 || W > 0x7fffffffLL / 64) return fail(PH_E_ARG, "W=%lld out of range", (long long)W);
  if (pcap < 1 || pcap > (1 << 20)) return fail(PH_E_ARG, "pcap=%d must be in [1, 2^20]", pcap);
  if (kcap < 1 || kcap > (1 << 24)) return fail(PH_E_ARG, "kcap=%d must be in [1, 2^24]", kcap);
  Plan pl;
  PH_TRY(plan_qo_extract(c, ccap, max_period, &pl));
  PH_HIP(hipSetDevice(c->device));
  const KernelPlan& k = pl.k[0];
  const int *d_off, *d_d, *d_mu;
  PH_TRY(prepare_mobius(c, max_period + 1, &d_off, &d_d, &d_mu));  // (the tables cover q < their bound)
  void *gws, *gidx;
  PH_TRY(place(c, k.second, B_WS0, (size_t)W * ph::qo_extract_work_bytes(ccap, max_period), &gws));
  PH_TRY(place(c, PH_PLAN_HBM, B_OUT1, (size_t)W * 2 * ((size_t)pcap + 1) * sizeof(int32_t), &gidx));
  Stage st(c, flags);
  const void *dper, *drow, *dcnt, *dwts;
  void *dout, *dstat;
  PH_TRY(st.in(periods, (size_t)W * pcap * sizeof(int32_t), &dper, B_GBUF));
  PH_TRY(st.in(rows, (size_t)W * pcap * sizeof(int32_t), &drow, B_WS1));
  PH_TRY(st.in(counts, (size_t)W * sizeof(int32_t), &dcnt, B_GWIN));
  PH_TRY(st.in(weights, (size_t)W * kcap * sizeof(double), &dwts, B_IN));
  PH_TRY(st.out(B_OUT0, out, (size_t)W * ccap * sizeof(double), &dout));
  PH_TRY(st.out(B_GEN0, status, (size_t)W * sizeof(int32_t), &dstat));
  const dim3 grid((unsigned)W);
  auto extract = [&](auto wl) {
    return launch(c, "k_qo_extract", ph::k_qo_extract<decltype(wl)::value>, grid, k.block, k.lds, (const int*)dper,
                  (const int*)drow, (const int*)dcnt, pcap, (const double*)dwts, kcap, max_period, ccap, d_off, d_d, d_mu,
                  (int*)gidx, (double*)gws, (double*)dout, (int*)dstat);
  };
  PH_TRY(k.second == PH_PLAN_LDS ? extract(std::true_type{}) : extract(std::false_type{}));
  return st.finish();
}


}  // extern "C"

// ----------------------------------------------------------------------------- short-time framing / overlap-add
namespace {

// the frame walk every short-time entry point makes: positive sizes, and every frame starts inside the signal.  `rows`
// points at K where the entry point has rows per frame (K is then checked and named with the rest), nullptr where not
int check_frame_walk(const char* what, int64_t W, const int* rows, int N, int hop, int64_t L) {
  if (rows && (W < 1 || *rows < 1 || N < 1 || hop < 1 || L < 1))
    return fail(PH_E_ARG, "%s: W=%lld, K=%d, N=%d, hop=%d, L=%lld must all be >= 1", what, (long long)W, *rows, N, hop,
                (long long)L);
  if (W < 1 || N < 1 || hop < 1 || L < 1)
    return fail(PH_E_ARG, "%s: W=%lld, N=%d, hop=%d, L=%lld must all be >= 1", what, (long long)W, N, hop, (long long)L);
  if (W - 1 > (L - 1) / hop)
    return fail(PH_E_ARG, "%s: frame %lld starts at or behind the end of the signal ((W - 1) * hop >= L = %lld)", what,
                (long long)(W - 1), (long long)L);
  return PH_OK;
}

// the element count W * rows * N (times 8 bytes) stays inside int64 -- it may well pass 2^31
int check_framed_size(const char* what, int64_t W, int rows, int N) {
  if (W > (INT64_MAX / 8) / ((int64_t)rows * N)) return fail(PH_E_ARG, "%s: W * K * N does not fit 64 bits", what);
  return PH_OK;
}

// T tracks: at least one, and the (T, L) result and the (T, W) masks (times 8 bytes) stay inside int64.  Two calls,
// because each routed entry point has limits of its own that it has always named between the two
int check_tracks(const char* what, int64_t T) {
  return T < 1 ? fail(PH_E_ARG, "%s: T=%lld must be >= 1", what, (long long)T) : (int)PH_OK;
}
int check_tracks_size(const char* what, int64_t T, int64_t W, int64_t L) {
  if (T > (INT64_MAX / 8) / L || T > (INT64_MAX / 8) / W)
    return fail(PH_E_ARG, "%s: T * L or T * W does not fit 64 bits", what);
  return PH_OK;
}

// What the three overlap-add kernels take besides their rows: the optional counts and windows, the masks of the routed
// ones (T = 0: none), and the `norm` flag -- staged into the same slots for all three.
struct OlaSides {
  const int* counts = nullptr;
  const unsigned long long* masks = nullptr;
  const double *wa = nullptr, *ws = nullptr;
  int norm = 0;
  int stage(Stage& st, unsigned flags, int64_t W, int N, const int32_t* h_counts, const uint64_t* h_masks, int64_t T,
            const double* win_a, const double* win_s) {
    const void *dc = nullptr, *dm = nullptr, *da = nullptr, *ds = nullptr;
    if (h_counts) PH_TRY(st.in(h_counts, (size_t)W * sizeof(int32_t), &dc, B_GBUF));
    if (h_masks) PH_TRY(st.in(h_masks, (size_t)T * W * sizeof(uint64_t), &dm, B_WS0));
    if (win_a) PH_TRY(st.in(win_a, (size_t)N * sizeof(double), &da, B_GWIN));
    if (win_s) PH_TRY(st.in(win_s, (size_t)N * sizeof(double), &ds, B_WS1));
    counts = (const int*)dc, masks = (const unsigned long long*)dm, wa = (const double*)da, ws = (const double*)ds;
    norm = (flags & PH_FLAG_OLA_NORM) ? 1 : 0;
    return PH_OK;
  }
};

// workgroups of a flat grid-stride kernel over `items` lanes' worth of work
unsigned flat_grid(const ph_ctx* c, int64_t items) {
  const int64_t want = (items + ph::kFramesBlock - 1) / ph::kFramesBlock;
  const int64_t cap = (int64_t)std::max(1, c->num_cu) * 64;
  return (unsigned)std::max<int64_t>(1, std::min(want, cap));
}

template <typename Tin, typename Tout>
int launch_frames(ph_ctx* c, const void* ds, int64_t L, int N, int hop, int64_t W, const double* dwin, void* dout) {
  constexpr int V = 16 / (int)sizeof(Tout);
  const int64_t total = W * (int64_t)N;
  if (reinterpret_cast<uintptr_t>(dout) % 16 == 0)
    return launch(c, "k_frames", ph::k_frames<Tin, Tout, V>, dim3(flat_grid(c, total / V)), ph::kFramesBlock, 0,
                  (const Tin*)ds, L, N, hop, W, dwin, (Tout*)dout);
  return launch(c, "k_frames", ph::k_frames<Tin, Tout, 1>, dim3(flat_grid(c, total)), ph::kFramesBlock, 0, (const Tin*)ds, L,
                N, hop, W, dwin, (Tout*)dout);
}

}  // namespace

extern "C" {

int ph_frames(ph_ctx* c, const void* signal, int in_dtype, int64_t L, int N, int hop, int64_t W, const double* window,
              int out_dtype, unsigned flags, void* frames) {
  if (!c) return fail(PH_E_ARG, "ctx is NULL");
  if (!signal || !frames) return fail(PH_E_ARG, "signal / frames is NULL");
  if ((in_dtype != PH_F64 && in_dtype != PH_F32) || (out_dtype != PH_F64 && out_dtype != PH_F32))
    return fail(PH_E_ARG, "in_dtype and out_dtype must be PH_F64 or PH_F32");
  const int one = 1;
  PH_TRY(check_frame_walk("ph_frames", W, &one, N, hop, L));
  PH_TRY(check_framed_size("ph_frames", W, 1, N));
  PH_HIP(hipSetDevice(c->device));
  Stage st(c, flags);
  const void *ds, *dwin = nullptr;
  void* dout;
  PH_TRY(st.in(signal, (size_t)L * elem_size(in_dtype), &ds));  // the signal once: L elements, not W * N
  if (window) PH_TRY(st.in(window, (size_t)N * sizeof(double), &dwin, B_GWIN));
  PH_TRY(st.out(B_OUT0, frames, (size_t)W * N * elem_size(out_dtype), &dout));
  PH_TRY(dispatch(in_dtype, [&](auto ti) {
    return dispatch(out_dtype, [&](auto to) {
      return launch_frames<decltype(ti), decltype(to)>(c, ds, L, N, hop, W, (const double*)dwin, dout);
    });
  }));
  return st.finish();
}

int ph_overlap_add(ph_ctx* c, const void* y, int dtype, int64_t W, int K, int N, int hop, int64_t L,
                   const int32_t* counts, const double* win_a, const double* win_s, unsigned flags, double* out) {
  if (!c) return fail(PH_E_ARG, "ctx is NULL");
  if (!y || !out) return fail(PH_E_ARG, "y / out is NULL");
  if (dtype != PH_F64 && dtype != PH_F32) return fail(PH_E_ARG, "dtype must be PH_F64 or PH_F32");
  PH_TRY(check_frame_walk("ph_overlap_add", W, &K, N, hop, L));
  PH_TRY(check_framed_size("ph_overlap_add", W, K, N));
  PH_HIP(hipSetDevice(c->device));
  Stage st(c, flags);
  OlaSides sd;
  const void* dy;
  void* dout;
  PH_TRY(st.in(y, (size_t)W * K * N * elem_size(dtype), &dy));
  PH_TRY(sd.stage(st, flags, W, N, counts, nullptr, 0, win_a, win_s));
  PH_TRY(st.out(B_OUT0, out, (size_t)L * sizeof(double), &dout));
  const dim3 grid(flat_grid(c, L));
  PH_TRY(dispatch(dtype, [&](auto t) {
    using T = decltype(t);
    return launch(c, "k_overlap_add", ph::k_overlap_add<T>, grid, ph::kFramesBlock, 0, (const T*)dy, W, K, N, hop, L, sd.counts,
                  sd.wa, sd.ws, sd.norm, (double*)dout);
  }));
  return st.finish();
}

int ph_overlap_add_tracks(ph_ctx* c, const void* y, int dtype, int64_t W, int K, int N, int hop, int64_t L,
                          const int32_t* counts, const uint64_t* masks, int64_t T, const double* win_a,
                          const double* win_s, unsigned flags, double* out) {
  if (!c) return fail(PH_E_ARG, "ctx is NULL");
  if (!y || !masks || !out) return fail(PH_E_ARG, "y / masks / out is NULL");
  if (dtype != PH_F64 && dtype != PH_F32) return fail(PH_E_ARG, "dtype must be PH_F64 or PH_F32");
  PH_TRY(check_frame_walk("ph_overlap_add_tracks", W, &K, N, hop, L));
  PH_TRY(check_framed_size("ph_overlap_add_tracks", W, K, N));
  PH_TRY(check_tracks("ph_overlap_add_tracks", T));
  if (K > 64) return fail(PH_E_ARG, "ph_overlap_add_tracks: K=%d rows per frame do not fit a 64-bit mask", K);
  PH_TRY(check_tracks_size("ph_overlap_add_tracks", T, W, L));
  PH_HIP(hipSetDevice(c->device));
  Stage st(c, flags);
  OlaSides sd;
  const void* dy;
  void* dout;
  PH_TRY(st.in(y, (size_t)W * K * N * elem_size(dtype), &dy));
  PH_TRY(sd.stage(st, flags, W, N, counts, masks, T, win_a, win_s));
  PH_TRY(st.out(B_OUT0, out, (size_t)T * L * sizeof(double), &dout));
  const dim3 grid(flat_grid(c, T * L));
  PH_TRY(dispatch(dtype, [&](auto t) {
    using E = decltype(t);
    return launch(c, "k_overlap_add_tracks", ph::k_overlap_add_tracks<E>, grid, ph::kFramesBlock, 0, (const E*)dy, W, K, N,
                  hop, L, sd.counts, sd.masks, T, sd.wa, sd.ws, sd.norm, (double*)dout);
  }));
  return st.finish();
}

int ph_overlap_add_periodic(ph_ctx* c, const double* seg, const int32_t* periods, const int32_t* counts,
                            const uint64_t* masks, int64_t W, int pcap, int ccap, int64_t T, int N, int hop, int64_t L,
                            const double* win_a, const double* win_s, unsigned flags, double* out) {
  if (!c) return fail(PH_E_ARG, "ctx is NULL");
  if (!seg || !periods || !counts || !masks || !out)
    return fail(PH_E_ARG, "ph_overlap_add_periodic: seg / periods / counts / masks / out is NULL");
  // (there is no W * K * N array here, so no product of that size to refuse)
  PH_TRY(check_frame_walk("ph_overlap_add_periodic", W, nullptr, N, hop, L));
  PH_TRY(check_tracks("ph_overlap_add_periodic", T));
  if (pcap < 1 || pcap > (1 << 20)) return fail(PH_E_ARG, "ph_overlap_add_periodic: pcap=%d must be in [1, 2^20]", pcap);
  if (ccap < 1 || ccap > (1 << 24)) return fail(PH_E_ARG, "ph_overlap_add_periodic: ccap=%d must be in [1, 2^24]", ccap);
  PH_TRY(check_tracks_size("ph_overlap_add_periodic", T, W, L));
  if (W > (INT64_MAX / 8) / ccap || W > (INT64_MAX / 4) / pcap)
    return fail(PH_E_ARG, "ph_overlap_add_periodic: W * ccap or W * pcap does not fit 64 bits");
  PH_HIP(hipSetDevice(c->device));
  Stage st(c, flags);
  OlaSides sd;
  const void *dseg, *dper;
  void* dout;
  PH_TRY(st.in(seg, (size_t)W * ccap * sizeof(double), &dseg));
  PH_TRY(st.in(periods, (size_t)W * pcap * sizeof(int32_t), &dper, B_GEN0));
  PH_TRY(sd.stage(st, flags, W, N, counts, masks, T, win_a, win_s));
  PH_TRY(st.out(B_OUT0, out, (size_t)T * L * sizeof(double), &dout));
  const dim3 grid(flat_grid(c, T * L));
  PH_TRY(launch(c, "k_overlap_add_periodic", ph::k_overlap_add_periodic, grid, ph::kFramesBlock, 0, (const double*)dseg,
                (const int*)dper, sd.counts, sd.masks, W, pcap, ccap, T, N, hop, L, sd.wa, sd.ws, sd.norm, (double*)dout));
  return st.finish();
}

int ph_overlap_add_block(ph_ctx* c, const void* y, int dtype, int64_t Wb, int K, int N, int hop, int64_t L, int64_t f0,
                         const int32_t* counts, const uint64_t* masks, int64_t T, const double* win_s, unsigned flags,
                         double* acc) {
  if (!c) return fail(PH_E_ARG, "ctx is NULL");
  if (!y || !acc) return fail(PH_E_ARG, "y / acc is NULL");
  if (dtype != PH_F64 && dtype != PH_F32) return fail(PH_E_ARG, "dtype must be PH_F64 or PH_F32");
  PH_TRY(check_frame_walk("ph_overlap_add_block", Wb, &K, N, hop, L));  // (the sizes, and the block as if f0 were 0)
  if (f0 < 0) return fail(PH_E_ARG, "ph_overlap_add_block: f0=%lld must be >= 0", (long long)f0);
  if (f0 > (L - 1) / hop - (Wb - 1))  // (no f0 + Wb, which may overflow)
    return fail(PH_E_ARG, "ph_overlap_add_block: the block's last frame starts at or behind the end of the signal "
                "((f0 + Wb - 1) * hop >= L = %lld with f0 = %lld, Wb = %lld)", (long long)L, (long long)f0, (long long)Wb);
  PH_TRY(check_framed_size("ph_overlap_add_block", Wb, K, N));
  if (!masks && T != 1) return fail(PH_E_ARG, "ph_overlap_add_block: T=%lld without masks (one track: T = 1)", (long long)T);
  PH_TRY(check_tracks("ph_overlap_add_block", T));
  if (masks && K > 64) return fail(PH_E_ARG, "ph_overlap_add_block: K=%d rows per frame do not fit a 64-bit mask", K);
  PH_TRY(check_tracks_size("ph_overlap_add_block", T, Wb, L));
  PH_HIP(hipSetDevice(c->device));
  Stage st(c, flags);
  OlaSides sd;
  const void *dy, *dold;
  void* dacc;
  PH_TRY(st.in(y, (size_t)Wb * K * N * elem_size(dtype), &dy));
  PH_TRY(sd.stage(st, flags, Wb, N, counts, masks, T, nullptr, win_s));
  // acc travels both ways, whole: up into the slot it comes down from
  PH_TRY(st.in(acc, (size_t)T * L * sizeof(double), &dold, B_OUT0));
  PH_TRY(st.out(B_OUT0, acc, (size_t)T * L * sizeof(double), &dacc));
  const int64_t end = (f0 + Wb - 1) * hop + N;  // <= L - 1 + N
  const dim3 grid(flat_grid(c, T * (std::min(end, L) - f0 * hop)));
  PH_TRY(dispatch(dtype, [&](auto t) {
    using E = decltype(t);
    auto block = [&](auto routed) {
      return launch(c, "k_overlap_add_block", ph::k_overlap_add_block<E, decltype(routed)::value>, grid, ph::kFramesBlock, 0,
                    (const E*)dy, Wb, K, N, hop, L, f0, sd.counts, sd.masks, T, sd.ws, (double*)dacc);
    };
    return sd.masks ? block(std::true_type{}) : block(std::false_type{});
  }));
  return st.finish();
}

int ph_overlap_add_finish(ph_ctx* c, const double* acc, int64_t T, int N, int hop, int64_t L, int64_t W,
                          const double* win_a, const double* win_s, unsigned flags, double* out) {
  if (!c) return fail(PH_E_ARG, "ctx is NULL");
  if (!acc || !out) return fail(PH_E_ARG, "acc / out is NULL");
  PH_TRY(check_frame_walk("ph_overlap_add_finish", W, nullptr, N, hop, L));
  PH_TRY(check_tracks("ph_overlap_add_finish", T));
  PH_TRY(check_tracks_size("ph_overlap_add_finish", T, W, L));
  PH_HIP(hipSetDevice(c->device));
  Stage st(c, flags);
  OlaSides sd;
  const void* dacc;
  void* dout;
  PH_TRY(st.in(acc, (size_t)T * L * sizeof(double), &dacc));
  PH_TRY(sd.stage(st, flags, W, N, nullptr, nullptr, 0, win_a, win_s));
  PH_TRY(st.out(B_OUT0, out, (size_t)T * L * sizeof(double), &dout));
  PH_TRY(launch(c, "k_overlap_add_finish", ph::k_overlap_add_finish, dim3(flat_grid(c, T * L)), ph::kFramesBlock, 0,
                (const double*)dacc, T, N, hop, L, W, sd.wa, sd.ws, sd.norm, (double*)dout));
  return st.finish();
}

// ----------------------------------------------------------------------------- best path through a time-period map
int ph_period_path_plan_info(ph_ctx* c, int P, int* block, int* lds_bytes, int* tile_rows) {
  if (!c || !block || !lds_bytes || !tile_rows) return fail(PH_E_ARG, "NULL argument");
  PathPlan pp;
  PH_TRY(resolve_period_path(c, 1, 1, P, P, 0, 0.0, &pp));
  *block = pp.block;
  *lds_bytes = (int)pp.lds;
  *tile_rows = pp.tile;
  return PH_OK;
}

int ph_period_path(ph_ctx* c, const double* cost, int64_t R, int64_t W, int P, int64_t ld, int band, double jump,
                   unsigned flags, int32_t* path, double* value, double* score, int32_t* status) {
  if (!c) return fail(PH_E_ARG, "ctx is NULL");
  if (!cost || !path || !score || !status) return fail(PH_E_ARG, "ph_period_path: cost / path / score / status is NULL");
  PathPlan pp;
  PH_TRY(resolve_period_path(c, R, W, P, ld, band, jump, &pp));
  if (R == 0) return PH_OK;
  PH_HIP(hipSetDevice(c->device));
  const size_t rows = (size_t)R * (size_t)W;
  PH_TRY(ensure(c, c->buf[B_WS0], rows * (size_t)pp.row_bytes));  // the back-pointers, (R, W, row_bytes) int8
  Stage st(c, flags);
  const void* dcost;
  void *dpath, *dval, *dscore, *dstat;
  // a strided host table goes up as it lies, gaps included, and the kernel walks it with the same ld
  PH_TRY(st.in(cost, ((rows - 1) * (size_t)ld + (size_t)P) * sizeof(double), &dcost));
  PH_TRY(st.out(B_OUT0, path, rows * sizeof(int32_t), &dpath));
  PH_TRY(st.out(B_OUT1, value, rows * sizeof(double), &dval));
  PH_TRY(st.out(B_OUT2, score, (size_t)R * sizeof(double), &dscore));
  PH_TRY(st.out(B_GEN0, status, (size_t)R * sizeof(int32_t), &dstat));
  const auto go = [&](auto ns) {
    return launch(c, "k_period_path", ph::k_period_path<decltype(ns)::value>, dim3((unsigned)R), pp.block, pp.lds,
                  (const double*)dcost, W, P, ld, band, jump, c->path_tile_cap, (signed char*)c->buf[B_WS0].p, (int*)dpath,
                  (double*)dval, (double*)dscore, (int*)dstat);
  };
  int rc = PH_E_ARG;
  switch (pp.states) {  // 1 .. kPathMaxStates, by the limit on P
    case 1: rc = go(std::integral_constant<int, 1>{}); break;
    case 2: rc = go(std::integral_constant<int, 2>{}); break;
    case 3: rc = go(std::integral_constant<int, 3>{}); break;
    case 4: rc = go(std::integral_constant<int, 4>{}); break;
    case 5: rc = go(std::integral_constant<int, 5>{}); break;
    case 6: rc = go(std::integral_constant<int, 6>{}); break;
    case 7: rc = go(std::integral_constant<int, 7>{}); break;
    case 8: rc = go(std::integral_constant<int, 8>{}); break;
  }
  PH_TRY(rc);
  return st.finish();
}

// ----------------------------------------------------------------------------- extraction along a period track
int ph_follow_plan_info(ph_ctx* c, int N, int* block, int* lds_bytes, int* placement) {
  if (!c || !block || !lds_bytes || !placement) return fail(PH_E_ARG, "NULL argument");
  FollowPlan fp;
  PH_TRY(resolve_follow(c, N, &fp));
  *block = fp.block;
  *lds_bytes = (int)fp.lds;
  *placement = fp.placement;
  return PH_OK;
}

int ph_follow(ph_ctx* c, const void* signal, int in_dtype, int64_t L, int N, int hop, int64_t W, const double* window,
              int frame_dtype, const int32_t* periods, const int32_t* counts, int pcap, int ccap, unsigned flags,
              double* seg, double* powers, int32_t* done) {
  if (!c) return fail(PH_E_ARG, "ctx is NULL");
  if (!signal || !periods || !counts || !seg || !powers || !done)
    return fail(PH_E_ARG, "ph_follow: signal / periods / counts / seg / powers / done is NULL");
  if ((in_dtype != PH_F64 && in_dtype != PH_F32) || (frame_dtype != PH_F64 && frame_dtype != PH_F32))
    return fail(PH_E_ARG, "ph_follow: in_dtype and frame_dtype must be PH_F64 or PH_F32");
  PH_TRY(check_frame_walk("ph_follow", W, nullptr, N, hop, L));
  if (pcap < 1 || pcap > ph::kFollowMaxBlocks)
    return fail(PH_E_ARG, "ph_follow: pcap=%d must be in [1, %d] (blocks per frame a 64-bit mask can name)", pcap,
                ph::kFollowMaxBlocks);
  if (ccap < 1 || ccap > ph::kFollowMaxSeg) return fail(PH_E_ARG, "ph_follow: ccap=%d must be in [1, 2^24]", ccap);
  // (W * pcap * 8 follows from W * 2^9 <= INT64_MAX / 8 < W * ccap's bound only for ccap >= 64: both are checked)
  if (L > INT64_MAX / 8 || W > (INT64_MAX / 8) / ccap || W > (INT64_MAX / 8) / pcap)
    return fail(PH_E_ARG, "ph_follow: L, W * ccap or W * pcap does not fit 64 bits");
  FollowPlan fp;
  PH_TRY(resolve_follow(c, N, &fp));
  PH_HIP(hipSetDevice(c->device));
  // workgroups walk the frames grid-stride: at most eight per CU (four when each brings a workspace slice of 16 N
  // bytes), and the workspace is theirs, not the frames'
  const unsigned grid =
      (unsigned)std::min<int64_t>(W, (int64_t)std::max(1, c->num_cu) * (fp.placement == PH_PLAN_LDS ? 8 : 4));
  void* gws;
  PH_TRY(place(c, fp.placement, B_WS0, (size_t)grid * ph::follow_work_doubles(N) * sizeof(double), &gws));
  Stage st(c, flags);
  const void *ds, *dwin = nullptr, *dper, *dcnt, *dold;
  void *dseg, *dpow, *ddone;
  PH_TRY(st.in(signal, (size_t)L * elem_size(in_dtype), &ds));  // the signal once: L elements, no frames
  if (window) PH_TRY(st.in(window, (size_t)N * sizeof(double), &dwin, B_GWIN));
  PH_TRY(st.in(periods, (size_t)W * pcap * sizeof(int32_t), &dper, B_GEN0));
  PH_TRY(st.in(counts, (size_t)W * sizeof(int32_t), &dcnt, B_GBUF));
  // seg travels both ways, whole: the elements the kernel never writes come back as they went up
  PH_TRY(st.in(seg, (size_t)W * ccap * sizeof(double), &dold, B_OUT0));
  PH_TRY(st.out(B_OUT0, seg, (size_t)W * ccap * sizeof(double), &dseg));
  PH_TRY(st.out(B_OUT1, powers, (size_t)W * pcap * sizeof(double), &dpow));
  PH_TRY(st.out(B_OUT2, done, (size_t)W * sizeof(int32_t), &ddone));
  const unsigned kflags = flags & PH_FLAG_TRUNC;
  PH_TRY(dispatch(in_dtype, [&](auto ti) {
    return dispatch(frame_dtype, fp.placement == PH_PLAN_LDS, [&](auto tf, auto lw) {
      return launch(c, "k_follow", ph::k_follow<decltype(ti), decltype(tf), decltype(lw)::value>, dim3(grid), fp.block,
                    fp.lds, (const decltype(ti)*)ds, L, N, hop, W, (const double*)dwin, (const int*)dper, (const int*)dcnt,
                    pcap, ccap, kflags, (double*)gws, (double*)dseg, (double*)dpow, (int*)ddone);
    });
  }));
  return st.finish();
}

int ph_follow_residual(ph_ctx* c, const void* signal, int in_dtype, int64_t L, int N, int hop, int64_t f0, int64_t Wb,
                       const double* window, int frame_dtype, const int32_t* periods, const int32_t* counts, int pcap,
                       unsigned flags, double* out) {
  if (!c) return fail(PH_E_ARG, "ctx is NULL");
  if (!signal || !out) return fail(PH_E_ARG, "ph_follow_residual: signal / out is NULL");
  if (pcap > 0 && (!periods || !counts))
    return fail(PH_E_ARG, "ph_follow_residual: periods / counts is NULL with pcap=%d (no tracks: pcap = 0)", pcap);
  if ((in_dtype != PH_F64 && in_dtype != PH_F32) || (frame_dtype != PH_F64 && frame_dtype != PH_F32))
    return fail(PH_E_ARG, "ph_follow_residual: in_dtype and frame_dtype must be PH_F64 or PH_F32");
  PH_TRY(check_frame_walk("ph_follow_residual", Wb, nullptr, N, hop, L));  // (the sizes, and the block as if f0 were 0)
  if (f0 < 0) return fail(PH_E_ARG, "ph_follow_residual: f0=%lld must be >= 0", (long long)f0);
  if (f0 > (L - 1) / hop - (Wb - 1))  // (no f0 + Wb, which may overflow)
    return fail(PH_E_ARG, "ph_follow_residual: the block's last frame starts at or behind the end of the signal "
                "((f0 + Wb - 1) * hop >= L = %lld with f0 = %lld, Wb = %lld)", (long long)L, (long long)f0, (long long)Wb);
  if (pcap < 0 || pcap > ph::kFollowMaxBlocks)
    return fail(PH_E_ARG, "ph_follow_residual: pcap=%d must be in [0, %d]", pcap, ph::kFollowMaxBlocks);
  PH_TRY(check_framed_size("ph_follow_residual", Wb, 1, N));
  if (L > INT64_MAX / 8 || (pcap > 0 && Wb > (INT64_MAX / 4) / pcap))
    return fail(PH_E_ARG, "ph_follow_residual: L or Wb * pcap does not fit 64 bits");
  FollowPlan fp;
  PH_TRY(resolve_follow(c, N, &fp));
  PH_HIP(hipSetDevice(c->device));
  // (the grid and the workspace of ph_follow)
  const unsigned grid =
      (unsigned)std::min<int64_t>(Wb, (int64_t)std::max(1, c->num_cu) * (fp.placement == PH_PLAN_LDS ? 8 : 4));
  void* gws;
  PH_TRY(place(c, fp.placement, B_WS0, (size_t)grid * ph::follow_work_doubles(N) * sizeof(double), &gws));
  Stage st(c, flags);
  const void *ds, *dwin = nullptr, *dper = nullptr, *dcnt = nullptr;
  void* dout;
  PH_TRY(st.in(signal, (size_t)L * elem_size(in_dtype), &ds));  // the signal once, whole: f0 indexes into it
  if (window) PH_TRY(st.in(window, (size_t)N * sizeof(double), &dwin, B_GWIN));
  if (pcap > 0) {
    PH_TRY(st.in(periods, (size_t)Wb * pcap * sizeof(int32_t), &dper, B_GEN0));
    PH_TRY(st.in(counts, (size_t)Wb * sizeof(int32_t), &dcnt, B_GBUF));
  }
  PH_TRY(st.out(B_OUT0, out, (size_t)Wb * N * sizeof(double), &dout));
  const unsigned kflags = flags & PH_FLAG_TRUNC;
  PH_TRY(dispatch(in_dtype, [&](auto ti) {
    return dispatch(frame_dtype, fp.placement == PH_PLAN_LDS, [&](auto tf, auto lw) {
      return launch(c, "k_follow_residual", ph::k_follow_residual<decltype(ti), decltype(tf), decltype(lw)::value>,
                    dim3(grid), fp.block, fp.lds, (const decltype(ti)*)ds, L, N, hop, f0, Wb, (const double*)dwin,
                    (const int*)dper, (const int*)dcnt, pcap, kflags, (double*)gws, (double*)dout);
    });
  }));
  return st.finish();
}

}  // extern "C"

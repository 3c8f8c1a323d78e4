/*
 * periodhip.h -- C ABI of libperiod_hip.so: the MI355X (gfx950) implementation of the
 * pyPeriod projection hot path.
 *
 * The reference (woolgathering/pyPeriod v1) has no FFI; its boundary for this path is the
 * Python class surface exported at pyPeriod/__init__.py:1-3.  Each entry point below is what
 * a binding for that surface needs; the reference code it replaces is cited per function
 * (file:line into /root/reference/pyPeriod/).  INTEGRATION.md shows the ctypes stub a
 * reference maintainer would add.
 *
 * Conventions
 *   - extern "C", plain pointers and sizes, no torch / numpy types.
 *   - every function returns an int status: PH_OK (0) or a negative PH_E_* code; the text of
 *     the last failure on the calling thread is returned by ph_last_error().
 *   - windows are row-major (W, N) contiguous, dtype PH_F64 or PH_F32 (W = number of
 *     independent signal windows, N = samples per window).  One window == one call of the
 *     reference.
 *   - array arguments are HOST pointers by default: the library stages them through device
 *     buffers owned by the context and the call is synchronous.  With PH_FLAG_DEVICE in
 *     `flags` all *array* arguments (x and every output) are DEVICE pointers on the
 *     context's device, nothing is copied, and the call only enqueues work on the context's
 *     stream (use ph_sync / ph_timer_*).  The small integer tables (p_list, orth_*, fac_*)
 *     are always host pointers.
 *   - the caller owns every buffer it passes; the library never frees or retains them.
 *   - a ph_ctx is bound to one device and is not re-entrant; use one context per thread/GPU.
 *   - set-order tables: two places of the reference iterate a CPython `set` of divisors
 *     (Periods.py:209 and Periods.py:549) and the result depends on that order.  The caller
 *     supplies the order as dense CSR tables indexed by period: entries for period p are
 *     q[off[p]] .. q[off[p+1]-1], off has (table_max_p + 2) entries.  The Python host builds
 *     them from real CPython sets (pyperiod_amd/_factors.py).
 */
#ifndef PERIODHIP_H
#define PERIODHIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PH_VERSION 100 /* 0.1.0 */

/* status codes */
#define PH_OK 0
#define PH_E_ARG (-1)         /* bad argument (shape, range, NULL, unsupported N) */
#define PH_E_HIP (-2)         /* a HIP runtime call failed */
#define PH_E_NOMEM (-3)       /* device or host allocation failed */
#define PH_E_CAP (-4)         /* output capacity too small; see the function's doc */
#define PH_E_UNSUPPORTED (-5) /* valid request this build does not implement */

/* dtype of the window data */
#define PH_F64 0
#define PH_F32 1

/* flags */
#define PH_FLAG_TRUNC 1u  /* trunc_to_integer_multiple (Periods.py:178-184) */
#define PH_FLAG_ORTH 2u   /* orthogonalize (Periods.py:208-214); needs orth tables */
#define PH_FLAG_SINGLE 4u /* return_single_period (Periods.py:216-217): only out[..., :p] written */
#define PH_FLAG_DEVICE 8u /* array arguments are device pointers, call is asynchronous */
#define PH_FLAG_NOSYNC 16u /* with PH_FLAG_DEVICE: never synchronise, not even to report PH_E_CAP */
#define PH_FLAG_KEEP_WEIGHTS 32u /* ph_qo_find_periods: update_weights=False (QOPeriods.py:645-714) */
#define PH_FLAG_OLA_NORM 64u /* ph_overlap_add: divide by the overlap-added window product */

/* sweep modes */
#define PH_SWEEP_NORM 0       /* periodic_norm(project(x,p))        Periods.py:507-508 */
#define PH_SWEEP_NORM_GAMMA 1 /* periodic_norm(project(x,p), p)     Periods.py:509-510 */
#define PH_SWEEP_MAXABS 2     /* max_s |sum(x[s::p])|               Periods.py:327-331 */

/* per-window status words written by the algorithm kernels */
#define PH_ST_OK 0
#define PH_ST_NO_PERIOD 1 /* no candidate period had a positive norm (reference raises) */
#define PH_ST_ITER_CAP 2  /* iteration bound hit before `num` periods were found (qo_find_periods: of the solve) */
#define PH_ST_CAP 3       /* more accepted periods than `cap` (small_to_large) */

typedef struct ph_ctx ph_ctx;

/* ---- library / context ---------------------------------------------------------------- */
int ph_version(void);
const char* ph_last_error(void);
int ph_device_count(int* count);
/* Create a context on HIP device `device` with its own non-blocking stream.  PH_HBM_WINDOW=1 in the environment
 * (read here) makes the context keep every window and every second window-sized buffer in its HBM workspaces, as
 * if the LDS could not hold them: an independent same-precision reference for the LDS paths. */
int ph_create(int device, ph_ctx** out);
int ph_destroy(ph_ctx* ctx);
/* Borrow an existing hipStream_t (e.g. torch.cuda.current_stream().cuda_stream); NULL
 * restores the context's own (non-blocking) stream.  The device's default stream has the
 * handle 0, which cannot be told from NULL: pass PH_STREAM_DEFAULT for it -- work the caller
 * enqueued on the default stream (torch's current stream unless changed) is then ordered with
 * the library's kernels. */
#define PH_STREAM_DEFAULT ((void*)1)
int ph_set_stream(ph_ctx* ctx, void* hip_stream);
int ph_sync(ph_ctx* ctx);
/* HIP-event timer on the context's stream (the stream the kernels run on). */
int ph_timer_begin(ph_ctx* ctx);
int ph_timer_end(ph_ctx* ctx, float* elapsed_ms);
/* Per-kernel timing: while enabled, every kernel the library launches on this context is
 * bracketed with HIP events on the context's stream (up to 256 launches since the last
 * ph_profile_enable).  ph_profile_read synchronises the stream and returns the elapsed
 * milliseconds of launch i in ms[i]; ph_profile_name gives the kernel's name. */
int ph_profile_enable(ph_ctx* ctx, int on);
int ph_profile_read(ph_ctx* ctx, float* ms, int cap, int* count);
const char* ph_profile_name(ph_ctx* ctx, int i);
/* Multiprocessor count and per-workgroup LDS limit of the context's device. */
int ph_device_info(ph_ctx* ctx, int* num_cu, int* lds_bytes);
/* Largest N for which ph_sweep keeps a window of `dtype` in LDS (the fast path): exactly the last N at which
 * ph_plan_info(PH_OP_SWEEP) reports PH_PLAN_LDS for the window (the same N in every mode: a second buffer leaves
 * the LDS first).  Every other entry point switches at an N of its own, which ph_plan_info reports.  Longer
 * windows are accepted by every entry point: the window then lives in (or is read straight from) HBM / L2 --
 * project, sweep, m_best, small_to_large, best_correlation, ramanujan_norms, best_frequency,
 * qo_find_periods, fold_sums and orth_powers alike.  `flags` is ignored.  0 under PH_HBM_WINDOW. */
int ph_max_window(ph_ctx* ctx, int dtype, unsigned flags, int* max_n);

/* Pass plan of the norm sweeps (ph_sweep norm modes, ph_m_best, ph_qo_find_periods) over the
 * candidate periods [p_lo, p_hi]: n_periods = p_hi - p_lo + 1 periods are produced by n_pass
 * passes over the LDS-resident window (a pass at base period p also yields the folds of 2p
 * and 4p).  n_pass * N * sizeof(T) is the number of bytes one sweep reads from LDS. */
int ph_sweep_plan_info(ph_ctx* ctx, int p_lo, int p_hi, int* n_pass, int* n_periods);

/* The radius table of the window-pair screen of ph_m_best, as the host uploads it for windows of N samples: out[q],
 * q = 1 ... max_p <= N (out[0] = 0; max_p + 1 doubles), bounds |float screen value - fp64 value| of period q in units
 * of the window's sum of squares.  Host arithmetic only: needs no context and no device. */
int ph_pair_radius_table(int N, int max_p, double* out);

/* Measurement helper: which step-1 kernel ph_m_best runs for these arguments.  fp64 windows in plain mode
 * that fit the LDS twice are screened two windows per workgroup in packed float (windows_per_workgroup = 2,
 * one 8-byte LDS element carries a sample of both windows, lds_bytes_per_sample = 8 per PAIR) and only the
 * survivors of the screen are re-evaluated in fp64; otherwise one window per workgroup is folded in its
 * own precision (1, sizeof(T)).  A fold pass reads N * lds_bytes_per_sample bytes from LDS per workgroup. */
int ph_m_best_info(ph_ctx* ctx, int dtype, int N, int num, int min_length, int max_length, unsigned flags,
                   int* windows_per_workgroup, int* lds_bytes_per_sample);

/* Measurement helper: the pass plan that step-1 kernel walks per sweep over [min_length, max_length] (max_length < 0:
 * N / 3, Periods.py:486): n_pass passes over the window for n_periods candidate periods.  The window-pair kernel
 * takes the periods up to 64 in chains (one row-split pass at L yields L, L/2, L/4, ...), so its plan is shorter
 * than ph_sweep_plan_info's.  Reported is the plan plain m_best (gamma = 0) runs: there the window-pair kernel
 * screens only the periods in (max_length / 2, max_length] -- a period with a multiple in range cannot beat that
 * multiple, and is evaluated in fp64 only when a multiple survives the screen -- so n_pass counts the passes over
 * that range while n_periods stays max_length - min_length + 1.  m_best_gamma (gamma = 1) runs the full plan over
 * [min_length, max_length], and so does every context created with PH_PAIR_COVER=0 in the environment.
 * n_pass = periods the screen folds, each counted as one read of the window: the window-pair kernel folds some of
 * them two to a pass (ph_m_best_screen_info), so n_pass * N * 8 is the LDS traffic of the equivalent plan of single
 * passes, not the bytes the kernel reads. */
int ph_m_best_plan_info(ph_ctx* ctx, int dtype, int N, int num, int min_length, int max_length, unsigned flags,
                        int* n_pass, int* n_periods);

/* Measurement helper: the plan as the step-1 kernel walks it (gamma = 0: m_best, 1: m_best_gamma).  n_entries = plan
 * entries per sweep; n_screened = periods they fold; lds_elements = LDS elements (of lds_bytes_per_sample bytes,
 * ph_m_best_info) one sweep reads per workgroup, 64 per wavefront load.  The window-pair kernel folds a period
 * p >= 64 with at most 6 rows together with p + 64 from one set of loads when both have the same row count, so it has
 * fewer entries than periods and reads less than n_screened windows; a context created with PH_PAIR_DUO=0 in the
 * environment plans one pass per period. */
int ph_m_best_screen_info(ph_ctx* ctx, int dtype, int N, int num, int min_length, int max_length, unsigned flags,
                          int gamma, int* n_entries, int* n_screened, long long* lds_elements);

/* ---- Periods.periodic_norm over a batch (Periods.py:221-241) ---------------------------
 * out[w] = ||x[w]||_2 / sqrt(N), additionally / sqrt(p) when p > 0.  Any N. */
int ph_periodic_norm(ph_ctx* ctx, const void* x, int dtype, int64_t W, int N, int p,
                     unsigned flags, double* out);

/* ---- K1: Periods.project over a batch (Periods.py:142-219) ------------------------------
 * out[w, k, :] = project(x[w], p_list[k], trunc, orth)      shape (W, n_p, N), dtype of x.
 * Non-orth results are bit-identical to the reference (row-order accumulation, one
 * division).  p_list[k] >= 1.  orth_off/orth_q: for period p the ordered list of sub-periods
 * p/f (f prime, proper) to project out (Periods.py:209-214); ignored without PH_FLAG_ORTH. */
int ph_project_batch(ph_ctx* ctx, const void* x, int dtype, int64_t W, int N,
                     const int32_t* p_list, int n_p,
                     const int32_t* orth_off, const int32_t* orth_q, int table_max_p,
                     unsigned flags, void* out);

/* ---- K2: fused all-p sweep (inner loops Periods.py:501-510 and :324-331) ----------------
 * out[w, p - p_lo] for p in [p_lo, p_hi] (inclusive), float64, shape (W, p_hi - p_lo + 1).
 * One launch per window batch; each window is read from HBM once and stays in LDS. */
int ph_sweep(ph_ctx* ctx, const void* x, int dtype, int64_t W, int N, int p_lo, int p_hi,
             int mode, const int32_t* orth_off, const int32_t* orth_q, int table_max_p,
             unsigned flags, double* out);

/* ---- Periods._m_best_meta (Periods.py:456-601; m_best :408-430, m_best_gamma :432-454) --
 * periods (W, num) uint32, powers (W, num) float64, bases (W, num, N) dtype of x,
 * status (W) int32 (PH_ST_*).  Step 1 (the repeated all-p sweep, argmax, subtract) and
 * step 2 (factor refinement) both run on the device.  fac_off/fac_q: ordered proper
 * divisors (1 and p removed) of every p <= max_length, i.e. the iteration order of
 * get_factors(p, remove_1_and_n=True) at Periods.py:548-549.  Pass max_length < 0 for the
 * reference default floor(N/3).  With gamma = 0 step 1 of fp64 windows reads the same table to find the divisors
 * of the periods that survive its screen (ph_m_best_plan_info), so it must list EVERY proper divisor; with
 * gamma = 1 (m_best_gamma) the screen runs the full plan over every period and step 1 does not read it.
 * min_length = 1 offers period 1, whose row of fac_off is empty: a window that keeps it is returned PH_ST_OK with
 * its numbers, while the reference dies there (get_factors(1, remove_1_and_n=True), KeyError at Periods.py:548).
 * A caller that wants the reference's behaviour treats a PH_ST_OK row whose periods hold a 1 as failed; the Python
 * engine does so (PeriodEngine.m_best sets such rows to PH_ST_NO_PERIOD, Periods raises KeyError). */
int ph_m_best(ph_ctx* ctx, const void* x, int dtype, int64_t W, int N, int num,
              int min_length, int max_length, int gamma,
              const int32_t* orth_off, const int32_t* orth_q,
              const int32_t* fac_off, const int32_t* fac_q, int table_max_p,
              unsigned flags, uint32_t* periods, double* powers, void* bases, int32_t* status,
              int32_t* n_sweeps /* (W) all-p sweeps each window needed in step 1, or NULL */);

/* ---- Periods.small_to_large (Periods.py:246-287) ----------------------------------------
 * counts (W) int32 = number of accepted periods; periods (W, cap) int32; powers (W, cap)
 * float64; bases (W, cap, N) dtype of x or NULL.  Windows that accept more than `cap`
 * periods get status PH_ST_CAP, counts[w] holds the true count, and the call returns
 * PH_E_CAP so that the host can retry with a larger cap -- also with PH_FLAG_DEVICE: the
 * library then reads the batch's largest count back (one word; the call synchronises the
 * stream).  PH_FLAG_DEVICE | PH_FLAG_NOSYNC keeps the call asynchronous and returns PH_OK;
 * the caller must then inspect `status`.  n_periods < 0 = floor(N/2). */
int ph_small_to_large(ph_ctx* ctx, const void* x, int dtype, int64_t W, int N, double thresh,
                      int n_periods, const int32_t* orth_off, const int32_t* orth_q,
                      int table_max_p, unsigned flags, int cap, int32_t* counts,
                      int32_t* periods, double* powers, void* bases, int32_t* status);

/* ---- Periods.best_correlation (Periods.py:289-349) --------------------------------------
 * periods (W, num) uint32, norms (W, num) float64, bases (W, num, N).  max_length < 0 =
 * floor(N/3); candidate periods are 2 .. max_length-1 (exclusive bound, Periods.py:324). */
int ph_best_correlation(ph_ctx* ctx, const void* x, int dtype, int64_t W, int N, int num,
                        int max_length, double ratio,
                        const int32_t* orth_off, const int32_t* orth_q, int table_max_p,
                        unsigned flags, uint32_t* periods, double* norms, void* bases,
                        int32_t* status);

/* ---- Periods.best_frequency (Periods.py:351-398) ----------------------------------------
 * num times: k = argmax |rfft(residual, win_size)| (first maximum, Periods.py:386-389),
 * p = round(2 win_size / k) (:390-391, round-half-even), project, store, subtract (:392-397).
 * The spectrum is an in-LDS radix-2 FFT when win_size is a power of two whose complex work array
 * fits the LDS (win_size <= 8192), Bluestein's chirp convolution on two such FFTs for any other
 * win_size up to about 5400, otherwise a direct real DFT over the first min(N, win_size) samples
 * (no FFT library; bins spread over the whole GPU); twiddles from float64 tables in every case; the projection honours PH_FLAG_TRUNC / PH_FLAG_ORTH (orth tables must cover
 * p <= 2 win_size).  win_size < 1 = N (:381-382).  Two launches per round; W <= 65535.
 * periods (W, num) uint32; powers (W, num) float64 = norm / ||data|| (:397-399); bases
 * (W, num, N).  status PH_ST_NO_PERIOD: the spectral peak was bin 0 (or the spectrum NaN) at
 * some iteration -- the reference divides by zero there and raises OverflowError; rows from that
 * iteration on are zero. */
int ph_best_frequency(ph_ctx* ctx, const void* x, int dtype, int64_t W, int N, int win_size,
                      int num, const int32_t* orth_off, const int32_t* orth_q, int table_max_p,
                      unsigned flags, uint32_t* periods, double* powers, void* bases,
                      int32_t* status);

/* ---- RamanujanPeriods.find_periods (RamanujanPeriods.py:67-86 with :124-169) ------------
 * out (W, q_hi + 1) float64; entries below q_lo are zero (RamanujanPeriods.py:71).
 * Evaluated in float64 through the folded form (fold to S_q, Moebius-filter with the
 * integer Ramanujan sum c_q); the reference accumulates in float32, parity is 1e-5.
 * Any range: q_hi = N / 3 (the reference default, RamanujanPeriods.py:68-69) works for
 * N = 4096 .. 16384 and beyond, as long as one wavefront's strips (12 q_hi bytes) fit the LDS. */
int ph_ramanujan_norms(ph_ctx* ctx, const void* x, int dtype, int64_t W, int N, int q_lo,
                       int q_hi, unsigned flags, double* out);

/* ---- RamanujanPeriods.project(x, basis) (RamanujanPeriods.py:124-131) ------------------
 * Arbitrary dictionary: x (N) float64, basis (rows, N) float64 -> out (rows, N) float32 with
 * out[i] = dot(x, basis[i]/max(basis[i])) * basis[i]/max(basis[i]). */
int ph_dict_project(ph_ctx* ctx, const double* x, const double* basis, int rows, int N,
                    unsigned flags, float* out);

/* ---- QOPeriods.find_periods, non-orthogonal branch --------------------------------------
 * (QOPeriods.py:373-596, get_subspaces :830-840, solve_quadratic :779-796) with the default
 * test function rms(reconstruction) > rms(data) * thresh.  The whole greedy loop runs on the
 * device, one workgroup per window: gamma sweep, phi-mass row bookkeeping, Gram matrix (closed-form
 * counts, never formed: regenerated inside the product) and right-hand side by folds, matrix-free preconditioned
 * conjugate-gradient solve of A A^T w = A x, reconstruction, residual.
 * Any N (the residual moves to an HBM workspace when it does not fit the LDS beside the solver).
 * periods/norms/keeps (W, num): dictionary blocks in the order found (period, gamma norm, rows
 * kept); counts (W, 2) = {periods the reference reports, blocks in the dictionary} (they differ
 * by one when the test function stopped the loop, QOPeriods.py:584-592); weights (W, kcap)
 * float64, rows of block b start at sum(keeps[:b]); residual (W, N) dtype of x.
 * kcap = capacity in dictionary rows per window (status PH_ST_CAP when exceeded).
 * A conjugate-gradient solve that does not converge within its iteration bound (an ill-conditioned dictionary that
 * numpy.linalg.solve still solves) ends the window with PH_ST_ITER_CAP; callers re-run such windows on the host.
 * PH_FLAG_TRUNC: the period is chosen by the gamma norm of the trunc projection (Periods.py:178-184); the solve
 * is unchanged.  A selection without a positive norm then ends the window with PH_ST_NO_PERIOD.
 * PH_FLAG_KEEP_WEIGHTS (update_weights=False, QOPeriods.py:645-714): each new block is fitted alone to the running
 * residual (residue means, no solve); kcap may then go up to 2^20, and every N and max_length fits (nothing of
 * the dictionary lives in LDS).  Output layout:
 *   periods / norms / keeps describe the blocks in the order fitted, duplicates included;
 *   counts = {periods reported, blocks}: when the test function stops the loop, the last period's block is
 *     fitted once more to the current residual and appended (the residual is not updated), and one period
 *     fewer is reported;
 *   block b holds keeps[b] rows, or periods[b] rows when keeps[b] == 0 (`matrix[:keep] if keep else matrix`);
 *   weights is the concatenation of the blocks' rows.
 *   A selection without a positive norm ends the window with PH_ST_NO_PERIOD.
 * PH_FLAG_ORTH returns PH_E_UNSUPPORTED. */
int ph_qo_find_periods(ph_ctx* ctx, const void* x, int dtype, int64_t W, int N, int num,
                       double thresh, int min_length, int max_length, int kcap, unsigned flags,
                       uint32_t* periods, double* norms, int32_t* keeps, int32_t* counts,
                       double* weights, void* residual, int32_t* status);

/* ---- QOPeriods.find_periods with update_weights=False under an analysis window ----------
 * ph_qo_find_periods with PH_FLAG_KEEP_WEIGHTS, each block fitted under `window` (N float64 samples, one window for
 * the whole batch; a device pointer with PH_FLAG_DEVICE like every array; NULL returns PH_E_ARG): the weights of a
 * block are solve_quadratic(residual, block, window=window) (QOPeriods.py:779-796 as _dont_update_weights calls it,
 * :707-709), i.e. w_j = sum(window[n] residual[n]) / sum(window[n]) over n = j (mod period) -- the windowed Gram matrix
 * of one natural-basis block is diagonal.  Selection, the stop test and the residual update are not windowed.  One
 * launch per batch (k_qo_greedy_win).
 * Outputs, counts, the keeps[b] == 0 rule and kcap in [1, 2^20]: the PH_FLAG_KEEP_WEIGHTS section above.
 * flags: PH_FLAG_TRUNC selects the trunc sweep; PH_FLAG_KEEP_WEIGHTS is accepted and implied; PH_FLAG_ORTH returns
 * PH_E_UNSUPPORTED.
 * status: PH_ST_OK, PH_ST_NO_PERIOD, PH_ST_CAP as above; PH_ST_ITER_CAP when a fitted residue class has a window sum
 * of exactly zero (the reference's matrix is singular and its loop ends on LinAlgError) or a sum that is not finite.
 * Callers re-run windows that are not PH_ST_OK on the host. */
int ph_qo_greedy_win(ph_ctx* ctx, const void* x, int dtype, int64_t W, int N, const double* window, int num,
                     double thresh, int min_length, int max_length, int kcap, unsigned flags, uint32_t* periods,
                     double* norms, int32_t* keeps, int32_t* counts, double* weights, void* residual,
                     int32_t* status);

/* *ok = 1 when ph_qo_find_periods can run windows of N samples of `dtype` with `kcap` dictionary
 * rows on this device (bookkeeping and the six work vectors of the conjugate-gradient solve fit the
 * workgroup's LDS; the window joins them there or moves to the HBM workspace), else 0 -- callers fall back to a host-driven loop instead of catching PH_E_ARG. */
int ph_qo_feasible(ph_ctx* ctx, int dtype, int N, int max_length, int kcap, int* ok);

/* Where ph_qo_find_periods would put the residual window of one workgroup for these arguments, and the LDS it
 * would ask for (*lds_bytes), without running anything: PH_QO_LDS_OVERLAY = window in LDS, the solver's work
 * vectors overlay it; PH_QO_LDS_BEHIND = window in LDS, the work vectors (k_qo_find) or nothing (PH_FLAG_KEEP_WEIGHTS)
 * behind it; PH_QO_HBM = window in the HBM workspace.  The answer is computed by the code the launch uses and honours
 * PH_QO_HBM_WINDOW; max_length < 0 means N / 3.  Arguments the launch refuses return its error code.
 * With PH_FLAG_KEEP_WEIGHTS this is also the plan of ph_qo_greedy_win (its analysis window takes no LDS). */
#define PH_QO_LDS_OVERLAY 0
#define PH_QO_LDS_BEHIND 1
#define PH_QO_HBM 2
int ph_qo_plan_info(ph_ctx* ctx, int dtype, int N, int max_length, int kcap, unsigned flags, int* lds_bytes,
                    int* placement);

/* ---- launch plan of an entry point ------------------------------------------------------
 * What entry point `op` would launch for windows of N samples of `dtype` with these parameters and `flags`, without
 * running anything.  The answer comes from the planning function the launch itself uses (it honours PH_HBM_WINDOW
 * and the PH_*_PAIR / block overrides of the context); arguments the launch refuses return its error code.
 * params[0 .. n_params-1], by op (a missing entry takes the default shown; -1 = the reference's default):
 *   PH_OP_PROJECT           {max period in p_list}
 *   PH_OP_SWEEP             {p_lo, p_hi, mode}                       p_hi default N / 3
 *   PH_OP_M_BEST            {num, min_length, max_length, max_fac}  max_fac: most entries of one fac_off row
 *                                                                   (default: proper divisors, 1 and p removed)
 *   PH_OP_SMALL_TO_LARGE    {n_periods}                              default N / 2
 *   PH_OP_BEST_CORRELATION  {max_length}                             default N / 3
 *   PH_OP_BEST_FREQUENCY    {win_size}                               default N
 *   PH_OP_RAMANUJAN         {q_lo, q_hi}                             default 2, N / 3
 *   PH_OP_ORTH_POWERS       {max_p}                                  default N / 2
 *   PH_OP_FOLD_SUMS         {}
 *   PH_OP_QO_FIT            {kcap, max period}                       default 512, N   (ph_qo_fit; ph_ramanujan_fit's
 *                                                                   third kernel with max period = q_hi).  N and dtype
 *                                                                   do not enter: the window is read from HBM / L2
 *                                                                   (PH_PLAN_HBM) and the LDS holds the solver only.
 *                                                                   A kcap whose vectors do not fit the LDS returns
 *                                                                   PH_E_ARG here as at the launch, so the largest
 *                                                                   feasible kcap is found without launching.
 *   PH_OP_QO_FIT_WIN        {kcap, max period}                       default 512, N   (ph_qo_fit_win).  N enters:
 *                                                                   PH_PLAN_SECOND says where the staging vector u
 *                                                                   of N doubles lives -- PH_PLAN_LDS behind the
 *                                                                   solver's vectors while both fit the workgroup's
 *                                                                   limit, else PH_PLAN_HBM (always under
 *                                                                   PH_HBM_WINDOW=1); x and the analysis window are
 *                                                                   read from HBM / L2 (PH_PLAN_WINDOW =
 *                                                                   PH_PLAN_HBM).  kcap as PH_OP_QO_FIT.
 *   PH_OP_QO_ORTH_SELECT    {max_p}                                  default N / 3   (ph_qo_orth_select: PH_PLAN_WINDOW
 *                                                                   and PH_PLAN_SECOND move together -- window, the N
 *                                                                   doubles shared by the autocorrelation and the
 *                                                                   projection, and max_p doubles in LDS, or the
 *                                                                   window read from HBM / L2 and the work arrays in
 *                                                                   an HBM workspace)
 *   PH_OP_QO_GET_PERIODS    {ccap, max period}                       default N, N   (ph_qo_get_periods; N and dtype do not
 *                                                                   enter otherwise).  PH_PLAN_WINDOW (the concatenated
 *                                                                   input) and PH_PLAN_SECOND (the accumulators) move
 *                                                                   together: both, two vectors of
 *                                                                   min(max period, ccap / 2) doubles and as many
 *                                                                   int32 in LDS while that fits the workgroup's
 *                                                                   limit, else in an HBM workspace (always under
 *                                                                   PH_HBM_WINDOW=1)
 * ph_tile_sum and ph_dict_project do not depend on N (LDS of sum(keep) doubles / none) and have no op.
 * out[PH_PLAN_LEN] int32: out[PH_PLAN_KERNELS] kernels launched per call (per round for best_frequency), then one
 * record of PH_PLAN_STRIDE words per kernel at out[PH_PLAN_K0] (m_best step 1, best_frequency spectrum) and
 * out[PH_PLAN_K1] (m_best step 2, best_frequency update); slot i of kernel k is out[PH_PLAN_K0 + k * PH_PLAN_STRIDE + i]:
 *   PH_PLAN_VARIANT      PH_PLAN_ONE (one window per workgroup), PH_PLAN_PAIR (two windows, float screen),
 *                        PH_PLAN_FFT / PH_PLAN_CHIRP / PH_PLAN_DIRECT (best_frequency spectrum)
 *   PH_PLAN_WINDOW       PH_PLAN_LDS or PH_PLAN_HBM: where the kernel reads the window (the k_bf_fft / k_bf_chirp
 *                        spectra always read the residual from HBM into their LDS work array)
 *   PH_PLAN_SECOND       PH_PLAN_NONE, PH_PLAN_LDS or PH_PLAN_HBM: the second window-sized buffer (materialised
 *                        projection; ph_orth_powers: its autocorrelation work arrays)
 *   PH_PLAN_BLOCK        threads per workgroup
 *   PH_PLAN_LDS_BYTES    dynamic LDS per workgroup
 *   PH_PLAN_SMALL_MEANS  m_best step 1: 1 when the means of a short winner go through LDS (split_row_means), else 0
 *   PH_PLAN_WAVES        Ramanujan: wavefronts per workgroup (one strip pair each), else 0
 *   PH_PLAN_PAD          Ramanujan: zeroed elements behind the LDS window (0 or 256), else 0 */
#define PH_OP_PROJECT 0
#define PH_OP_SWEEP 1
#define PH_OP_M_BEST 2
#define PH_OP_SMALL_TO_LARGE 3
#define PH_OP_BEST_CORRELATION 4
#define PH_OP_BEST_FREQUENCY 5
#define PH_OP_RAMANUJAN 6
#define PH_OP_ORTH_POWERS 7
#define PH_OP_FOLD_SUMS 8
#define PH_OP_QO_FIT 9
#define PH_OP_QO_FIT_WIN 10
#define PH_OP_QO_ORTH_SELECT 11
#define PH_OP_QO_GET_PERIODS 12
#define PH_PLAN_KERNELS 0
#define PH_PLAN_K0 1
#define PH_PLAN_K1 9
#define PH_PLAN_STRIDE 8
#define PH_PLAN_LEN 17
#define PH_PLAN_VARIANT 0
#define PH_PLAN_WINDOW 1
#define PH_PLAN_SECOND 2
#define PH_PLAN_BLOCK 3
#define PH_PLAN_LDS_BYTES 4
#define PH_PLAN_SMALL_MEANS 5
#define PH_PLAN_WAVES 6
#define PH_PLAN_PAD 7
#define PH_PLAN_ONE 0
#define PH_PLAN_PAIR 1
#define PH_PLAN_FFT 2
#define PH_PLAN_CHIRP 3
#define PH_PLAN_DIRECT 4
#define PH_PLAN_NONE 0
#define PH_PLAN_LDS 1
#define PH_PLAN_HBM 2
int ph_plan_info(ph_ctx* ctx, int op, int dtype, int N, const int32_t* params, int n_params, unsigned flags,
                 int32_t* out);

/* ---- fit of a GIVEN period list: QOPeriods.compute_reconstruction / get_subspaces + solve_quadratic ------------
 * (QOPeriods.py:807-852, :779-796, :1054-1116), natural basis, no analysis window.  One workgroup per window runs the
 * phi-mass row bookkeeping, the right-hand side by folds, the matrix-free preconditioned conjugate gradients of
 * ph_qo_find_periods (same product, tolerances and iteration bound 4 K + 100, started from zero) and the residual.
 * periods (W, pcap) int32 with n_periods (W) int32 entries used per window, rows per_stride >= pcap apart;
 * per_stride == 0: one list periods[0 .. pcap) with n_periods[0] shared by all windows.  Both follow PH_FLAG_DEVICE
 * like every array, so the host may not be able to read the lists: max_period (<= 2^20) bounds the phi / divisor
 * tables and the divisor bitset, and a window whose list holds an entry < 1 or > max_period gets PH_ST_ITER_CAP.
 * keeps (W, pcap) int32 (0 behind the list); weights (W, kcap) float64, rows of block b start at sum(keeps[:b]);
 * residual (W, N) dtype of x; status (W) int32:
 *   PH_ST_OK
 *   PH_ST_NO_PERIOD  empty list
 *   PH_ST_CAP        more than pcap or 64 entries, or sum(keeps) > kcap
 *   PH_ST_ITER_CAP   a period outside 1 .. max_period; a block without rows (a repeated period, or one whose
 *                    divisors are all present: the reference's matrix is singular) or with more rows than samples;
 *                    sum(keeps) > N (rank deficient);
 *                    non-positive curvature or a non-finite residual of the solve; no convergence within the bound
 * Windows that are not PH_ST_OK have zero weights and an unspecified residual; callers re-run them on the host. */
int ph_qo_fit(ph_ctx* ctx, const void* x, int dtype, int64_t W, int N,
              const int32_t* periods, const int32_t* n_periods, int pcap, int per_stride, int max_period,
              int kcap, unsigned flags,
              int32_t* keeps, double* weights, void* residual, int32_t* status);

/* ---- the same fit under an analysis window: solve_quadratic(x, A, window=win) (QOPeriods.py:779-796) ------------
 * (A diag(win)) A^T w = (A diag(win)) x; the reconstruction A^T w and the residual x - A^T w are unwindowed.
 * window (N) float64, one for the whole batch, follows PH_FLAG_DEVICE like every array; NULL returns PH_E_ARG
 * (ph_qo_fit is the fit without a window).  Every other argument, the outputs and the status codes are ph_qo_fit's,
 * with the same conjugate gradients (tolerances, bound 4 K + 100, started from zero) around a product that goes through
 * a staging vector of N doubles per workgroup: u = win . (A^T v), then the folds A u.  ph_plan_info(PH_OP_QO_FIT_WIN)
 * says whether u is in LDS or in an HBM workspace of the context.  The Jacobi diagonal is the fold of the window; a row
 * whose diagonal is not > 0 (window zero or negative over a whole residue class: the reference's matrix is singular
 * or indefinite) gives PH_ST_ITER_CAP, as does non-positive curvature met by the solve under a window with negative
 * samples.  Windows that are not PH_ST_OK have zero weights and an unspecified residual. */
int ph_qo_fit_win(ph_ctx* ctx, const void* x, int dtype, int64_t W, int N, const double* window,
                  const int32_t* periods, const int32_t* n_periods, int pcap, int per_stride, int max_period,
                  int kcap, unsigned flags,
                  int32_t* keeps, double* weights, void* residual, int32_t* status);

/* ---- RamanujanPeriods.find_periods_with_weights (RamanujanPeriods.py:88-122), default test function ----------
 * ph_ramanujan_norms, the threshold (periods = the q with norms[q] / |max(norms)| > thresh, that IEEE division and
 * strict comparison, NaN never selected) and ph_qo_fit's kernel, enqueued on the context's stream with no host round
 * trip between them.  norms (W, q_hi + 1) float64 as ph_ramanujan_norms writes them; periods (W, pcap) int32
 * ascending (0 behind the list); counts (W) int32 = periods selected (may exceed pcap: PH_ST_CAP); keeps, weights,
 * residual, status as ph_qo_fit with max_period = q_hi.  thresh must be > 0 (PH_E_ARG otherwise: index 0 would be
 * selected and the reference dies on period 0). */
int ph_ramanujan_fit(ph_ctx* ctx, const void* x, int dtype, int64_t W, int N, int q_lo, int q_hi, double thresh,
                     int pcap, int kcap, unsigned flags,
                     double* norms, int32_t* periods, int32_t* counts, int32_t* keeps,
                     double* weights, void* residual, int32_t* status);

/* ---- the threshold of ph_ramanujan_fit on given norms, against a choosable level and with a capped list ----------
 * One launch (k_ram_select_ref, one wavefront per row) on norms (W, q_hi + 1) float64 as ph_ramanujan_norms writes them.
 *   m_w        = ref[w] when ref is given (W doubles); with ref == NULL what ph_ramanujan_fit uses: |max| of the row
 *                as numpy.max sees it, so a NaN anywhere makes it NaN
 *   candidates = the q in 0 .. q_hi with norms[w, q] / m_w > thresh -- that IEEE double division and strict
 *                comparison: a NaN entry or a NaN / zero-over-zero quotient is never a candidate, and with thresh > 0
 *                and m_w >= 0 every candidate is strictly positive
 *   over[w]    = number of candidates
 *   kept       = all of them when over[w] <= pcap; otherwise q is kept iff fewer than pcap candidates q' have
 *                norms[q'] > norms[q], or norms[q'] == norms[q] and q' < q: the pcap largest, ties to the smaller period
 *   counts[w]  = min(over[w], pcap); periods[w, :counts[w]] = the kept periods ascending, zeros behind them
 * With ref == NULL and over[w] <= pcap the lists are those of ph_ramanujan_fit, bit for bit.  periods (W, pcap),
 * counts (W) and over (W) are int32; every array follows PH_FLAG_DEVICE.  PH_E_ARG before anything is launched: a NULL
 * ctx / norms / output, W < 1, q_hi < 1 or beyond the record format of ph_ramanujan_norms, pcap outside [1, 2^20],
 * !(thresh > 0). */
int ph_ramanujan_select(ph_ctx* ctx, const double* norms, int64_t W, int q_hi, double thresh,
                        const double* ref /* W or NULL */, int pcap, unsigned flags,
                        int32_t* periods, int32_t* counts, int32_t* over);

/* ---- QOPeriods.get_best_period_orthogonal / eq_3 / auto_corr (QOPeriods.py:1122-1232) -----
 * powers (W, max_p) float64: the Muresan-Parks orthogonal period powers `pows` for q < max_p
 * (entry 0 is 0), divided by q when normalize != 0; autocorr (W, N) = auto_corr(x, k) for every
 * lag k, eq3 (W, max_p) = eq_3(x, q) -- both optional (NULL).  max_p < 0 = floor(N/2). */
int ph_orth_powers(ph_ctx* ctx, const void* x, int dtype, int64_t W, int N, int max_p,
                   int normalize, unsigned flags, double* autocorr, double* eq3, double* powers);

/* ---- selection step of QOPeriods.find_periods under orthogonal (Muresan-Parks) selection (QOPeriods.py:435-448) ----
 * For every window of a batch of residuals, in one launch (one workgroup per window):
 *   powers = get_best_period_orthogonal(x[w], max_p, normalize=True, return_powers=True)   (QOPeriods.py:1175-1232)
 *            -- the bits ph_orth_powers(normalize = 1) gives for the same window placement;
 *   period[w] = first maximum of powers over q in [0, max_p); 0 (all powers zero) becomes 1  (:1227-1232)
 *   norm[w]   = periodic_norm(project(x[w], period, trunc, orthogonalize=True), period)
 *               (Periods.py:142-219, the sub-periods p / f of :208-214 in the order of orth_off / orth_q; :221-241).
 * All arithmetic is in float64 for either dtype: a PH_F32 call gives the bits of the PH_F64 call on the upcast windows.
 * period (W) int32, norm (W) float64, powers (W, max_p) float64 or NULL, status (W) int32: PH_ST_OK, or
 * PH_ST_NO_PERIOD when a power or the norm is not finite -- overflow, or a NaN sample, which the clip of eq. 3 turns into
 * zero powers and the projection into a NaN norm -- (period 0, norm 0; callers re-run such windows on the host).
 * flags: PH_FLAG_TRUNC (the projection's truncated mean, Periods.py:178-184) and PH_FLAG_DEVICE; the orth tables
 * are always needed (host pointers) and must cover p <= max_p - 1.  max_p < 2 or table_max_p < max_p - 1: PH_E_ARG.
 * ph_plan_info(PH_OP_QO_ORTH_SELECT) says where the window and the work arrays live. */
int ph_qo_orth_select(ph_ctx* ctx, const void* x, int dtype, int64_t W, int N, int max_p,
                      const int32_t* orth_off, const int32_t* orth_q, int table_max_p, unsigned flags,
                      int32_t* period, double* norm, double* powers /* (W, max_p) or NULL */, int32_t* status);

/* ---- QOPeriods.get_periods (QOPeriods.py:719-741; concatenate_periods :854-887, stack_pairwise_gcd_subspaces :889-938,
 * reduce_rows :86-94) for a batch of fitted dictionaries, one launch (k_qo_extract, one workgroup per window), float64.
 * Window w has counts[w] dictionary blocks: periods[w, a] and rows[w, a] (row stride pcap) in dictionary order, and the
 * weights row weights[w, :] (stride kcap) is the concatenation of the blocks' weights -- block a starts at
 * sum(rows[w, :a]).  These are the (periods, keeps, counts[:, 1], weights) ph_qo_find_periods and ph_qo_fit write (with
 * PH_FLAG_KEEP_WEIGHTS a keeps entry of 0 stands for `period` rows and must be replaced first).  All five arrays
 * follow PH_FLAG_DEVICE, the int32 lists included, as ph_qo_fit's do.
 * The result is  actual = c - P c:  c the concatenated segments (segment a = rows[a] weights, then zeros up to
 * periods[a]) and P the orthogonal projector onto the span of the pairwise gcd rows -- for every pair a < b and shift
 * i < g = gcd(p_a, p_b): -1 on segment a at j = i (mod g), +1 on segment b at j = i (mod g).  It is evaluated in closed
 * form by fold-means and Moebius sums, no matrix is built.  out (W, ccap) float64: segment a of window w
 * starts at sum(periods[w, :a]); the row is zero behind sum(periods[w, :]).
 * Deliberate deviations from the (repaired) reference -- v1 cannot run the method at all, it passes `self._k` into the
 * positional `type` of solve_quadratic and dies with TypeError; with that call repaired:
 *   - every decomp_type ('row reduction', 'lu', 'qr', least squares) is a factorisation of the same projector, and this
 *     entry point returns the projector's result for all of them.  The reference raises LinAlgError for 'row reduction'
 *     on a rank-1 matrix (one period, or two coprime periods: reduce_rows hands back a 1-D row) and for 'lu' with three
 *     or more periods (singular U); those accidents of the factorisation are NOT mirrored.
 *   - `self._k` is ignored (the reference's regularisation line is commented out).
 * Mirrored: one period alone gives c - mean(c) (the reference's matrix is ones((1, p))); an empty dictionary is
 * PH_ST_NO_PERIOD (the reference ends in ValueError).
 * max_period (<= 2^20) bounds the Moebius tables; ccap in [1, 2^24], kcap in [1, 2^24], pcap in [1, 2^20].  NULL pointers
 * and range errors return PH_E_ARG before any HIP call.  status (W) int32:
 *   PH_ST_OK
 *   PH_ST_NO_PERIOD  counts[w] <= 0
 *   PH_ST_CAP        counts[w] > pcap, sum(periods) > ccap or sum(rows) > kcap
 *   PH_ST_ITER_CAP   a period < 1 or > max_period; rows < 0 or rows > period; a period listed twice
 * Rows that are not PH_ST_OK are zero.  ph_plan_info(PH_OP_QO_GET_PERIODS) says where the work arrays live; both
 * placements give the same bits (one fixed summation order). */
int ph_qo_get_periods(ph_ctx* ctx, const int32_t* periods, const int32_t* rows, const int32_t* counts,
                      int64_t W, int pcap, const double* weights, int kcap, int max_period,
                      int ccap, unsigned flags, double* out, int32_t* status);

/* ---- QOPeriods building blocks (QOPeriods.py:779-795) -----------------------------------
 * ph_fold_sums: W = A x for natural-basis rows -- out[w, off_k + j] = sum_{n = j (mod p_k)}
 * x[w, n], j < keep_k; row stride = sum(keep).  ph_tile_sum: reconstruction A^T w --
 * out[w, n] = sum_k wts[w, off_k + (n mod p_k)] (0 where n mod p_k >= keep_k). */
int ph_fold_sums(ph_ctx* ctx, const void* x, int dtype, int64_t W, int N,
                 const int32_t* p_list, const int32_t* keep, int n_p, unsigned flags,
                 double* out);
int ph_tile_sum(ph_ctx* ctx, const double* wts, int64_t W, int N, const int32_t* p_list,
                const int32_t* keep, int n_p, int dtype, unsigned flags, void* out);

/* ---- short-time analysis: frame a long signal, overlap-add a framed result (no counterpart in the reference, which
 * takes one window per call) ----------------------------------------------------------------------
 * ph_frames: frames (W, N) row-major contiguous of out_dtype from a signal of L samples of in_dtype:
 *   frames[f, i] = (out_dtype)((double)signal[f * hop + i] * window[i])   if f * hop + i < L, else 0
 * window (N) float64 or NULL (no product: a same-dtype call copies exactly).  hop >= 1, hop > N is allowed; W >= 1 and
 * (W - 1) * hop < L, so every frame starts inside the signal.  W * N may exceed 2^31.  The host-pointer form uploads
 * the signal once (L elements, not W * N).  One launch (k_frames): 16-byte stores whenever `frames` is 16-byte aligned,
 * for every N; scalar accesses otherwise.
 * ph_overlap_add: y (W, K, N) of dtype -> out (L) float64,
 *   num[n] = sum_f sum_{k < K_f} win_s[n - f * hop] * y[f, k, n - f * hop]
 *   den[n] = sum_f win_a[n - f * hop] * win_s[n - f * hop]          both over the frames f < W with 0 <= n - f * hop < N
 *   out[n] = num[n], or with PH_FLAG_OLA_NORM num[n] / den[n] where den[n] > 0 and exactly 0.0 elsewhere (samples no frame
 *   covers, or a zero window product).
 * K_f = counts[f] clipped to [0, K] (counts (W) int32 or NULL = K); rows k >= K_f are never read.  win_a / win_s (N) float64
 * or NULL = all ones.  One launch (k_overlap_add): one lane per output sample, float64 accumulation in one fixed order,
 * no atomics -- the same bits on every run.
 * Both: every array follows PH_FLAG_DEVICE (window, counts included); PH_E_ARG for a NULL ctx / signal / frames / y / out,
 * an unknown dtype, a size < 1, or (W - 1) * hop >= L, before any HIP call. */
int ph_frames(ph_ctx* ctx, const void* signal, int in_dtype, int64_t L, int N, int hop, int64_t W,
              const double* window /* N or NULL */, int out_dtype, unsigned flags, void* frames);
int ph_overlap_add(ph_ctx* ctx, const void* y, int dtype, int64_t W, int K, int N, int hop, int64_t L,
                   const int32_t* counts /* W or NULL */, const double* win_a, const double* win_s,
                   unsigned flags /* PH_FLAG_DEVICE | PH_FLAG_OLA_NORM */, double* out);

/* ph_overlap_add_tracks: the routed overlap-add -- y (W, K, N) of dtype -> out (T, L) float64,
 *   num[t, n] = sum_f win_s[n - f * hop] * sum_{k < K_f, bit k of masks[t, f] set} y[f, k, n - f * hop]
 *   den[n], K_f, the frames of a sample, win_a / win_s and PH_FLAG_OLA_NORM as in ph_overlap_add; a track without a term
 *   at n is exactly 0.0 there.
 * masks (T, W) 64-bit words: bit k of masks[t, f] routes row k of frame f to track t, so K <= 64.  Bits at or above K_f
 * are ignored; rows behind K_f or in no mask are never read; masks may overlap (the row is added to every track that names
 * it).  One launch (k_overlap_add_tracks): one lane per (t, n), float64 accumulation in ascending f, then ascending k, no
 * atomics -- the same bits on every run.  T * L and W * K * N may exceed 2^31.
 * Every array follows PH_FLAG_DEVICE.  PH_E_ARG for a NULL ctx / y / masks / out, an unknown dtype, what ph_overlap_add
 * refuses, T < 1, K > 64, or T * L * 8 / T * W * 8 beyond 64 bits, before any HIP call. */
int ph_overlap_add_tracks(ph_ctx* ctx, const void* y, int dtype, int64_t W, int K, int N, int hop, int64_t L,
                          const int32_t* counts /* W or NULL */, const uint64_t* masks /* (T, W) */, int64_t T,
                          const double* win_a, const double* win_s,
                          unsigned flags /* PH_FLAG_DEVICE | PH_FLAG_OLA_NORM */, double* out /* (T, L) */);

/* ph_overlap_add_periodic: the routed overlap-add of periodic segments -- seg (W, ccap) float64 in the
 * layout ph_qo_get_periods writes (block a of frame f is p(f, a) = periods[f, a] doubles at off(f, a) = sum of periods[f, :a])
 * -> out (T, L) float64, every block tiled to the frame on the fly.  With i = n - f * hop over the frames f < W, 0 <= i < N:
 *   num[t, n] = sum_f win_s[i] * sum_{a < C_f, bit a of masks[t, f] set} seg[f, off(f, a) + (i mod p(f, a))]
 *   C_f = counts[f] clipped to [0, min(pcap, 64)]; den[n], win_a / win_s, PH_FLAG_OLA_NORM and the exact 0.0 of a track
 *   without a term as in ph_overlap_add_tracks.
 * periods (W, pcap) int32, counts (W) int32, masks (T, W) 64-bit words: bit a of masks[t, f] routes block a of frame f to
 * track t (blocks at or above 64 cannot be routed); masks may overlap.  The offsets are derived in the kernel from
 * `periods`.  The walk of a frame stops at the first block with p < 1 or off + p > ccap: that block and the ones behind it
 * contribute nothing, so no read leaves the frame's row of seg whatever the arrays hold; elements behind sum(p), blocks
 * behind C_f and blocks in no mask of the track are never read.  i mod p is exact for N < 2^31 and p <= ccap <= 2^24
 * (p > N, p = N and p = 1 included).  One launch (k_overlap_add_periodic): one lane per (t, n), float64 accumulation in
 * ascending f, then ascending a, no atomics -- the same bits on every run.  T * L may exceed 2^31.
 * Every array follows PH_FLAG_DEVICE.  PH_E_ARG for a NULL ctx / seg / periods / counts / masks / out, W, N, hop, T, pcap,
 * ccap or L < 1, pcap > 2^20, ccap > 2^24, (W - 1) * hop >= L, or T * L * 8 / T * W * 8 / W * ccap * 8 / W * pcap * 4 beyond
 * 64 bits, before any HIP call. */
int ph_overlap_add_periodic(ph_ctx* ctx, const double* seg /* (W, ccap) */, const int32_t* periods /* (W, pcap) */,
                            const int32_t* counts /* W */, const uint64_t* masks /* (T, W) */, int64_t W, int pcap,
                            int ccap, int64_t T, int N, int hop, int64_t L, const double* win_a, const double* win_s,
                            unsigned flags /* PH_FLAG_DEVICE | PH_FLAG_OLA_NORM */, double* out /* (T, L) */);

/* ph_overlap_add_block / ph_overlap_add_finish: ph_overlap_add and ph_overlap_add_tracks for a recording whose frames come
 * in blocks, so that the (W, K, N) array never exists as a whole.
 * ph_overlap_add_block adds the frames f0 .. f0 + Wb - 1 of the recording into acc (T, L) float64, read and written:
 *   acc[t, n] += sum_{f0 <= f < f0 + Wb} win_s[n - f * hop] * sum_{k < K_f [, bit k of masks[t, f - f0] set]} y[f - f0, k, n - f * hop]
 * y (Wb, K, N) of dtype, counts (Wb) and masks (T, Wb) are block-local; K_f, win_s and the frames of a sample as in
 * ph_overlap_add.  masks == NULL: T must be 1, every row k < K_f is added (ph_overlap_add's walk; K may exceed 64).
 * With masks: ph_overlap_add_tracks's walk, K <= 64.  Only the samples f0 * hop .. min(L, (f0 + Wb - 1) * hop + N) - 1 of
 * each row of acc are read and written.  One launch (k_overlap_add_block).  The host-pointer form moves all of acc up and
 * down again; a long recording keeps acc on the device (PH_FLAG_DEVICE).
 * ph_overlap_add_finish: out[t, n] = acc[t, n], or with PH_FLAG_OLA_NORM acc[t, n] / den[n] where den[n] > 0 and exactly
 * 0.0 elsewhere; den[n] is that of ph_overlap_add for the W frames of the whole recording, recomputed here.  out may be
 * acc.  One launch (k_overlap_add_finish).
 * Contract, which neither call can check: acc is zeroed before the first block; the blocks are applied on one stream in
 * ascending f0; every frame f < W belongs to exactly one block.  After ph_overlap_add_finish, out is then bit for bit what
 * ph_overlap_add (masks == NULL) or ph_overlap_add_tracks gives for the whole (W, K, N) array: every sample's terms are
 * added in the same order, a later block continuing the sum where the block before left it.
 * Every array follows PH_FLAG_DEVICE.  PH_E_ARG, before any HIP call, for a NULL ctx / y / acc / out, an unknown dtype, a
 * size < 1, f0 < 0, (f0 + Wb - 1) * hop >= L (a frame that starts behind the signal; for finish (W - 1) * hop >= L),
 * masks == NULL with T != 1, masks with K > 64, or Wb * K * N * 8 / T * L * 8 / T * Wb * 8 beyond 64 bits. */
int ph_overlap_add_block(ph_ctx* ctx, const void* y, int dtype, int64_t Wb, int K, int N, int hop, int64_t L, int64_t f0,
                         const int32_t* counts /* Wb or NULL */, const uint64_t* masks /* (T, Wb) or NULL */, int64_t T,
                         const double* win_s, unsigned flags, double* acc /* (T, L), read and written */);
int ph_overlap_add_finish(ph_ctx* ctx, const double* acc, int64_t T, int N, int hop, int64_t L, int64_t W,
                          const double* win_a, const double* win_s, unsigned flags /* PH_FLAG_DEVICE | PH_FLAG_OLA_NORM */,
                          double* out /* (T, L) */);

/* ph_period_path: the best path through a time-period map -- R cost tables cost (R, W, ld) float64, of
 * which the first P columns of every row are used, -> the state of every frame.  With band B and pen[o] = jump * o:
 *   c'[f][j]   = cost[f][j] if finite, else -inf                  (NaN, +inf and -inf all mean "forbidden")
 *   D[0][j]    = c'[0][j];   D[f][j] = c'[f][j] + max_o (D[f-1][j+o] - pen[|o|])   over |o| <= B, 0 <= j + o < P
 *                offsets tried in the order 0, -1, +1, -2, +2, ..., a later one kept only if strictly greater
 *   score      = max_j D[W-1][j]; path[W-1] = the lowest such j; path[f-1] = path[f] + the offset kept at (f, path[f])
 *   value[f]   = cost[f][path[f]]
 * Every product, difference and sum is one float64 operation rounded once and max is exact, so path, value and score are
 * bit for bit those of a plain loop over these lines.  status[r] = PH_ST_OK, or PH_ST_NO_PERIOD when score is -inf (some
 * frame has no reachable state): then path[r] is all -1 and value[r] all 0.  path (R, W) int32, value (R, W) float64 or
 * NULL, score (R) float64, status (R) int32.  The columns P .. ld - 1 of cost are never read by the kernel.
 * One launch (k_period_path), one workgroup per map; the int8 back-pointers live in an (R, W, P rounded up to 16) workspace
 * of the context (PH_E_NOMEM when it cannot be allocated) and the backtrace walks them in LDS, a tile of whole rows at a
 * time.  R * W * P and R * W * ld may exceed 2^31.  The host-pointer form uploads the table as it lies, gaps included.
 * Every array follows PH_FLAG_DEVICE.  PH_E_ARG, before any HIP call, for a NULL ctx / cost / path / score / status, P not in
 * [1, 8192], band not in [0, 64], jump negative or not finite, W < 1, R < 0 or >= 2^31, ld < P, or R * W * ld * 16 beyond 64
 * bits.  R == 0 is PH_OK and launches nothing.
 * ph_period_path_plan_info: the launch shape for P columns -- threads per workgroup, LDS bytes, and the rows of one
 * backtrace tile (what fits the LDS the forward pass leaves behind; PH_PATH_TILE_ROWS=n in the environment of ph_create
 * caps it, for measurements).  Nothing runs on the device. */
int ph_period_path(ph_ctx* ctx, const double* cost /* (R, W, ld) */, int64_t R, int64_t W, int P, int64_t ld, int band,
                   double jump, unsigned flags /* PH_FLAG_DEVICE */, int32_t* path /* (R, W) */,
                   double* value /* (R, W) or NULL */, double* score /* (R) */, int32_t* status /* (R) */);
int ph_period_path_plan_info(ph_ctx* ctx, int P, int* block, int* lds_bytes, int* tile_rows);

/* ph_follow: extraction along a period track -- the periodic component of every frame of a recording at
 * the periods the caller names for that frame, peeled one after the other.  The kernel cuts its frames from the signal
 * itself (L samples of in_dtype); no (W, N) array exists.  Frame f is what ph_frames would write, widened to double:
 *   x_f[i] = (double)(frame_dtype)((double)signal[f * hop + i] * window[i]) for f * hop + i < L, else 0
 * (window == NULL: no product; frame_dtype PH_F32 rounds each sample to float once, PH_F64 does not round).
 *   C_f = counts[f] clipped to [0, pcap];  r_0 = x_f, off = 0
 *   for a = 0 .. C_f - 1, p = periods[f, a]; the walk of the frame stops at the first block with p < 1, p > N or
 *   off + p > ccap, otherwise
 *     s = project(r_a, p, trunc, False, return_single_period=True)   residues added in row order, one division
 *     seg[f, off + j] = s[j] for j < p
 *     r_{a+1}[i] = r_a[i] - s[i mod p]                                one rounded subtraction per sample
 *     powers[f, a] = (pn(r_a) - pn(r_{a+1})) / pn(x_f)                pn = periodic_norm; exactly 0.0 when pn(x_f) == 0
 *     off += p
 * done[f] = the blocks written, powers[f, a >= done[f]] = 0.0, and the elements of seg behind the last block are never
 * written (the host-pointer form moves seg up and down again, so they come back as they were).  seg and done are those
 * of a plain loop over these lines bit for bit; the sum of squares inside pn is a workgroup reduction, so powers is
 * within 1e-10 * pn(r_a) / pn(x_f) of that loop.  Non-finite samples propagate; there is no status word.
 * seg (W, ccap) float64, periods (W, pcap) int32 and counts (W) int32 are the layout ph_qo_get_periods writes and
 * ph_overlap_add_periodic reads.  The first two stop rules are that kernel's; a frame that stops only on p > N does not
 * stop in its walk, so such a frame must not be handed on as it stands.
 * One launch (k_follow): a workgroup handles one frame at a time and the workgroups walk the frames grid-stride; the
 * residual frame and one period of means (N doubles each) live in LDS while both fit the workgroup's limit, otherwise --
 * always under PH_HBM_WINDOW=1 -- in a per-workgroup slice of a workspace of the context.  W * ccap may exceed 2^31.
 * flags: PH_FLAG_DEVICE | PH_FLAG_TRUNC.  Every array follows PH_FLAG_DEVICE.  PH_E_ARG, before any HIP call, for a
 * NULL ctx / signal / periods / counts / seg / powers / done, an unknown dtype, a size < 1, (W - 1) * hop >= L,
 * pcap > 64, ccap > 2^24, or L * 8 / W * ccap * 8 / W * pcap * 8 beyond 64 bits.
 * ph_follow_plan_info: the launch shape for frames of N samples -- threads per workgroup, LDS bytes and the placement
 * of the two states (PH_PLAN_LDS or PH_PLAN_HBM).  Nothing runs on the device. */
int ph_follow(ph_ctx* ctx, const void* signal, int in_dtype, int64_t L, int N, int hop, int64_t W,
              const double* window /* N or NULL */, int frame_dtype, const int32_t* periods /* (W, pcap) */,
              const int32_t* counts /* W */, int pcap, int ccap, unsigned flags /* PH_FLAG_DEVICE | PH_FLAG_TRUNC */,
              double* seg /* (W, ccap) */, double* powers /* (W, pcap) */, int32_t* done /* W */);
int ph_follow_plan_info(ph_ctx* ctx, int N, int* block, int* lds_bytes, int* placement);

/* ph_follow_residual: the frames of a recording less the tracks named for them -- what ph_follow
 * leaves of each frame after its peels, which ph_follow itself throws away.  Row i of `out` belongs to frame f0 + i:
 *   x[j] = (double)(frame_dtype)((double)signal[(f0 + i) * hop + j] * window[j]) for (f0 + i) * hop + j < L, else 0
 *   C_i = counts[i] clipped to [0, pcap];  r_0 = x
 *   for a = 0 .. C_i - 1, p = periods[i, a]; the walk of the frame stops at the first block with p < 1 or p > N
 *   (there is no ccap), otherwise
 *     s = project(r_a, p, trunc, False, return_single_period=True)   residues added in row order, one division
 *     r_{a+1}[j] = r_a[j] - s[j mod p]                                one rounded subtraction per sample
 *   out[i, j] = r_C[j] for every j < N, C the blocks peeled (none: x itself, the row ph_frames writes, as double).
 * One launch (k_follow_residual): the body, launch shape and placement of k_follow (ph_follow_plan_info reports them),
 * compiled without the segment, powers and done outputs and hence without their sums of squares and reductions; the
 * cut, the means and the subtractions are the same statements, so `out` is ph_follow's residual bit for bit.
 * periods (Wb, pcap) and counts (Wb) are local to the block; pcap == 0: both may be NULL and the call is a float64
 * ph_frames of the block.  Wb * N and f0 * hop may exceed 2^31.  Non-finite samples propagate; no status word.
 * flags: PH_FLAG_DEVICE | PH_FLAG_TRUNC.  Every array follows PH_FLAG_DEVICE; the host-pointer form uploads the whole
 * signal.  PH_E_ARG, before any HIP call, for a NULL ctx / signal / out, NULL periods / counts with pcap > 0, an unknown
 * dtype, N, hop, L or Wb < 1, f0 < 0, (f0 + Wb - 1) * hop >= L, pcap outside 0 .. 64, or Wb * N * 8 / L * 8 /
 * Wb * pcap * 4 beyond 64 bits. */
int ph_follow_residual(ph_ctx* ctx, const void* signal, int in_dtype, int64_t L, int N, int hop, int64_t f0, int64_t Wb,
                       const double* window /* N or NULL */, int frame_dtype,
                       const int32_t* periods /* (Wb, pcap), block-local */, const int32_t* counts /* Wb */, int pcap,
                       unsigned flags /* PH_FLAG_DEVICE | PH_FLAG_TRUNC */, double* out /* (Wb, N) */);

#ifdef __cplusplus
}
#endif
#endif /* PERIODHIP_H */

/*
 * ibo_abi.h -- C ABI of libibo_hip.so, the MI355X (gfx950) implementation of the
 * GP-posterior + acquisition hot path of misterwindupbird/IBO.
 *
 * Two groups of entry points:
 *
 *  (A) LEGACY symbols -- byte-for-byte the signatures the reference's Python
 *      binds with ctypes today, so the .so is a drop-in for cpp/libs/libego:
 *        acqmaxGP   replaces  cpp/optimizeGP.cpp:262-283
 *        logCDFs    replaces  cpp/helpers.cpp:30-56
 *                   bound at  ego/acquisition/__init__.py:343-364
 *        direct     replaces  cpp/direct.cpp:329 (cpp/direct.h:76)
 *                   bound at  ego/utils/optimize.py:320-333
 *
 *  (B) HANDLE-BASED symbols (ibo_*) -- re-entrant, explicit status codes,
 *      batch/candidate-array aware (the legacy ABI has no notion of a
 *      candidate array).  These are what ibo_amd's Python host code calls and
 *      what a maintainer would bind to move GaussianProcess.addData /
 *      posterior(s) / maximize* / fastUCBGallery onto the GPU.
 *
 * Conventions: all matrices row-major fp64; "host" pointers are ordinary
 * process memory borrowed for the duration of the call; "dev" pointers are HIP
 * device memory on the handle's device (from ibo_dev_alloc or any hipMalloc).
 * Every ibo_* function returns an IBO_* status; ibo_last_error() describes the
 * last failure on the calling thread.  No torch / C++ types cross this line.
 */
#ifndef IBO_ABI_H
#define IBO_ABI_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define IBO_ABI_VERSION 8   /* 2: + ibo_gp_extend, ibo_comm_count; 3: + ibo_pref_*; 4: + ibo_dev_generation; 5: + ibo_sweep_state_info; 6: + ibo_sweep_state_levels;
                             * 7: + ibo_gpu_time_ms, ibo_acq_sweep_exchange, ibo_direct_server_info, ibo_acq_grad_batch, ibo_posterior_cov, ibo_posterior_sample (added later, without a new version); options "super_min_nb", "direct_resident", "direct_idle_ms", "arena_mb" -- ibo_set_option knows the keys listed below and nothing else: the experiment switches of rounds 2-4
                             * (nlml_groups, cov_fast, chol_fused, small_local, zero_copy, gallery_lazy, pipe_fit, .. -- about 35 keys) were removed in
                             * round 5 and now return IBO_ERR_ARG "unknown option", as does a NULL key; ibo_nlml_grid's covariance pass is the fast one;
                             * 8: - ibo_direct_server_info and the options "direct_resident", "direct_idle_ms" (ibo_direct_max's resident evaluation server, measured
                             * slower than the launches and removed: both keys are unknown options now); + ibo_gp_loo, ibo_loo_grad (leave-one-out predictions and the LOO-CV
                             * objective with its gradient: additions within 8, nothing else changed); + ibo_gp_remove (observations taken out of a fitted model in
                             * O(N^2): added within 8, nothing else changed); within 8 as well: the ibo_pref_* entries refuse a workspace begun on another
                             * model (IBO_ERR_STATE where a call used to compute from stale data -- no symbol, signature or valid call order changed);
                             * + ibo_cacq_sweep, ibo_cacq_batch, ibo_cacq_grad_batch, ibo_cacq_direct_max (EI / PI weighted by the probability of feasibility
                             * under up to eight constraint models: added within 8, nothing else changed);
                             * + ibo_kg_sweep, ibo_kg_batch, ibo_kg_direct_max, ibo_kg_stage_ms (the knowledge gradient against a reference set) and the
                             * options "kg_chunk", "kg_timing": added within 8, nothing else changed;
                             * + the option "cacq_chunk" (within 8: no symbol changed);
                             * + ibo_paths_create, ibo_paths_destroy, ibo_paths_info, ibo_paths_coef, ibo_paths_sweep, ibo_paths_batch, ibo_paths_direct_max
                             * (pathwise posterior draws: Thompson sampling over whole candidate arrays) and the option "paths_chunk": added within 8,
                             * nothing else changed;
                             * + ibo_qei_sweep, ibo_qei_batch, ibo_qei_direct_max, ibo_qei_stage_ms (Monte-Carlo parallel expected improvement with pending
                             * points) and the options "qei_chunk", "qei_timing": added within 8, nothing else changed;
                             * + ibo_ehvi_sweep, ibo_ehvi_batch, ibo_ehvi_grad_batch, ibo_ehvi_direct_max (the expected hypervolume improvement of two
                             * objectives over a Pareto front), ibo_ehvi_scan_ms and the options "ehvi_chunk", "ehvi_timing": added within 8, nothing else changed;
                             * + ibo_paths_grad_batch (values and gradients of the pathwise draws with respect to x; "paths_chunk" bounds its pieces too):
                             * added within 8, nothing else changed;
                             * + ibo_ggp_create, ibo_ggp_destroy, ibo_ggp_info, ibo_ggp_fit, ibo_ggp_get_R, ibo_ggp_get_L, ibo_ggp_acq_batch, ibo_ggp_acq_sweep,
                             * ibo_ggp_direct_max, ibo_ggp_stage_ms (a GP observed with gradients, on a handle type of its own) and the options "ggp_chunk",
                             * "ggp_timing": added within 8, nothing else changed;
                             * + ibo_mes_sweep, ibo_mes_batch, ibo_mes_grad_batch, ibo_mes_direct_max, ibo_mes_maxcdf, ibo_mes_scan_ms (max-value entropy
                             * search against samples of the maximum, and the max-value cdf over a candidate set that the Gumbel approximation of those
                             * samples is fitted to) and the options "mes_chunk", "mes_timing": added within 8, nothing else changed;
                             * + ibo_sgp_create, ibo_sgp_destroy, ibo_sgp_fit, ibo_sgp_add, ibo_sgp_acq_batch, ibo_sgp_acq_sweep, ibo_sgp_direct_max,
                             * ibo_sgp_nlml, ibo_sgp_get, ibo_sgp_stage_ms (a sparse GP on inducing points, DTC / FITC, on a handle type of its own) and the
                             * options "sgp_chunk", "sgp_timing": added within 8, nothing else changed;
                             * + ibo_sgp_nlml_grad, ibo_sgp_grad_stage_ms (the sparse marginal likelihood's gradient with respect to the log
                             * hyper-parameters, the log noise and the inducing points, for fitc / dtc / vfe): added within 8, nothing else changed;
                             * + ibo_ggp_nlml_grad, ibo_ggp_grad_stage_ms (the marginal likelihood of a GP observed with gradients and its gradient with
                             * respect to the log hyper-parameters, the log noise and the log gradient noises): added within 8, nothing else changed */

/* status codes */
#define IBO_OK              0
#define IBO_ERR_ARG         1   /* bad argument (null pointer, size, enum)            */
#define IBO_ERR_HIP         2   /* HIP runtime error (see ibo_last_error)              */
#define IBO_ERR_NOT_PD      3   /* matrix not positive definite (numpy LinAlgError)    */
#define IBO_ERR_STATE       4   /* call order (e.g. sweep before fit)                  */
#define IBO_ERR_NO_DEVICE   5   /* no gfx950 device visible -- there is NO CPU fallback */
#define IBO_ERR_COMM        6   /* RCCL error                                          */

/* kernel type codes == the reference's (ego/acquisition/__init__.py:323-333) */
#define IBO_K_SE_ARD   0        /* hyper = D length scales                             */
#define IBO_K_SE_ISO   1        /* hyper = [theta]                                     */
#define IBO_K_MATERN3  2        /* hyper = [theta]  (magnitude goes in sf2)            */
#define IBO_K_MATERN5  3        /* hyper = [theta]  (magnitude goes in sf2)            */

/* acquisition codes == the reference's (ego/acquisition/__init__.py:309-321) */
#define IBO_ACQ_EI   0
#define IBO_ACQ_PI   1
#define IBO_ACQ_UCB  2
#define IBO_ACQ_NONE 3          /* posterior only                                      */

/* erf flavour: libm as cpp/optimizeGP.cpp:200-204, or the
 * Numerical-Recipes fit with truncated constants of
 * ego/gaussianprocess/__init__.py:55-77 */
#define IBO_ERF_LIBM 0
#define IBO_ERF_NR   1

/* diagonal rule for the covariance matrix */
#define IBO_DIAG_UNIT_PLUS_NOISE 0   /* 1+noise : GaussianProcess._computeCorrelations,
                                        ego/gaussianprocess/__init__.py:138            */
#define IBO_DIAG_KERNEL_PLUS_NOISE 1 /* k(x,x)+noise : marginalLikelihood,
                                        ego/gaussianprocess/trainhyper.py:55           */

typedef struct ibo_gp ibo_gp_t;       /* a fitted GP resident on one GPU */
typedef struct ibo_comm ibo_comm_t;   /* an RCCL communicator (one rank per GPU) */

/* ---------------------------------------------------------------- library */
int         ibo_abi_version(void);
const char *ibo_last_error(void);
int         ibo_device_count(int *count);
/* name/arch string of a device ("gfx950...") into buf */
int         ibo_device_name(int device, char *buf, size_t buflen);
/* self-test of the fp64 MFMA fragment layout on the device (returns IBO_OK or
 * IBO_ERR_HIP with a message); cheap, used by smoke() */
int         ibo_selftest_mfma(int device, double *max_abs_err);
/* milliseconds of device time this process has measured with HIP events on `device` so far: fits and block extensions, candidate
 * sweeps (the dominant kernel's span, as ibo_last_sweep_kernel_ms), likelihood grids (a batch's longest sub-batch span) and
 * gradients.  DIRECT's small batches and the copies are not event-timed and not in it.  bench.py reports it as gpu_kernel_s_total
 * so that a line can be related to an outside observer's busy-GPU samples. */
int         ibo_gpu_time_ms(int device, double *ms);
/* The twenty-seven option keys (everything else is decided by the data: sizes, dimensions, what the caller asks for).
 * Functional:  "legacy_exact" 1/0 -- acqmaxGP in libego's operation order (default) or on the MFMA sweep kernels (see acqmaxGP);
 *   "nlml_batch" B -- matrices per batched factorisation in ibo_nlml_grid (0: as many as 12 GB hold; the values do not depend on it);
 *   "pool_limit_mb" n -- the per-device free list of recycled buffers (ibo_trim);
 *   "arena_mb" n -- MiB per slab of the buffer arena (1024; 0: none): device buffers of up to half a slab are sub-allocated from slabs
 *   taken from the device once, the first when the library first allocates there, so a new model finds warm memory (ibo_trim keeps the first);
 *   "super_min_nb" nb -- block columns from which a single-level factorisation runs in super-panels of 16 (64; linalg.hip launch_cholesky_super:
 *   the columns beyond a super-panel take its steps as one deep update from packed operands -- the same bits, a matter of speed only);
 *   "fused2_min_nb" nb -- block columns (of 64 rows) from which a single matrix is factored in the two-level order (104; the order fixes the
 *   last bits of L and W -- one rule for ibo_gp_fit, the preference GP and ibo_nlml_grad).
 * Comparators kept for the tests (a second route to the same numbers):  "sweep_path" 0 auto (small2.hip's three kernels up to 4096
 *   candidates, sweep2_kernel above; GEMV / panel-split / first-generation tile kernels where the dot form is not admissible) / 1 GEMV /
 *   2 MFMA tile / 3 panel-split;  "dot_form" -1 auto / 0 / 1 (k* by differences or by the exponent GEMM);  "gallery_prune" 0/1/2 and
 *   "part_levels" 2..4 (see ibo_acq_sweep_incremental);  "host_pipeline" 1/0 (large host batches in overlapped chunks or in one shot);
 *   "chol_left" 1/0 (ibo_nlml_grid's left-looking order or the right-looking one: identical bits);  "kg_chunk" m (candidates per chunk of
 *   the ibo_kg_* entries, 0: by bytes -- identical bits);  "cacq_chunk" m (candidates per chunk of ibo_cacq_sweep, rounded up to 256,
 *   0: by bytes, 2^30 / (16 (ncon + 1)) -- identical bits);  "paths_chunk" m (candidates per launch of the ibo_paths_* entries, rounded up to
 *   256, 0: 2^21 -- identical bits);  "qei_chunk" m (candidates per chunk of the ibo_qei_* entries, rounded up to 256, 0: by bytes --
 *   identical bits);  "ehvi_chunk" m (candidates per chunk of the ibo_ehvi_* entries, rounded up to 256, 0: by bytes, 2^25 -- identical bits
 *   among chunks of up to 4096 and among larger ones, see the ibo_ehvi_* entries);  "mes_chunk" m (candidates per chunk of the ibo_mes_* entries, rounded up to 256, 0: by bytes, 2^26 -- the same
 *   statement as "ehvi_chunk", see the ibo_mes_* entries);  "ggp_chunk" m (candidates per chunk of the ibo_ggp_* entries,
 *   rounded up to 256, 0: by bytes -- identical bits);  "sgp_chunk" n (observations and candidates per chunk of the ibo_sgp_* entries,
 *   rounded up to 256, 0: by bytes -- see those entries for what stays bit-identical).
 * Diagnostic:  "sgp_timing" 1/0 (see ibo_sgp_stage_ms);  "ggp_timing" 1/0 (see ibo_ggp_stage_ms);  "kg_timing" 1/0 (see ibo_kg_stage_ms);  "qei_timing" 1/0 (see ibo_qei_stage_ms);  "ehvi_timing" 1/0 (see ibo_ehvi_scan_ms);  "mes_timing" 1/0 (see ibo_mes_scan_ms).
 * Test hook:  "alloc_fill" -1 (off, the default) / 0 .. 255 (anything else: IBO_ERR_ARG) -- while it is on, every device buffer the library
 *   newly obtains (from its arena, its free list or the device; a buffer that already has the capacity is live and left alone) and every
 *   array of ibo_dev_alloc is filled with that byte and the device synchronised before it is handed out; the pinned staging of a handle is
 *   filled on the host when the handle takes it over and when it grows.  A new buffer's content is undefined, and no result, status or info
 *   word may depend on it: 0xFF makes every unwritten double a NaN and every int -1, 0x7F a finite 1.4e306 and 0x7F7F7F7F
 *   (tests/test_gpu_alloc_fill.py).  Off, it costs one relaxed atomic load per allocation and changes no kernel, launch or allocation order.
 * Env: IBO_SWEEP_IMPL=gemv|mfma, IBO_DOT_FORM, IBO_POOL_LIMIT_MB, IBO_HOST_THREADS (the legacy symbol's host crew), IBO_DEVICE (legacy symbols),
 *   IBO_NLML_GROUPS=1..4 (sub-batches of an ibo_nlml_grid batch, each on its own stream; 2; the values do not depend on it).
 * Threading (the reference's library keeps its whole model in process-wide statics, cpp/optimizeGP.cpp:36-55,240-259, and is not
 * re-entrant; this one is): handles are independent of each other -- each has its own stream, events, staging and buffers --
 * so several threads may drive several handles on one device at the same time (one handle belongs to one thread at a time);
 * the buffer pool and the allocation table are mutexed; the per-device workspaces behind ibo_nlml_grid / ibo_nlml_grad and
 * ibo_trim are serialised by a per-device mutex (concurrent grids on one device take turns; a sweep on another handle never waits for them); the last
 * error is thread-local.  The option switches are process-wide CONFIGURATION held in atomics: changing one while another
 * thread computes is defined but takes effect at an unspecified call boundary -- set them before the threads start.
 * (tests/test_gpu_gallery_oracle.py::test_two_threads_two_handles_one_device.) */
int         ibo_set_option(const char *key, int value);

/* ---------------------------------------------------------------- device memory */
int ibo_dev_alloc(int device, size_t bytes, void **dev_ptr);
int ibo_dev_free(int device, void *dev_ptr);
int ibo_memcpy_h2d(int device, void *dev_dst, const void *host_src, size_t bytes);
int ibo_memcpy_d2h(int device, void *host_dst, const void *dev_src, size_t bytes);
int ibo_device_synchronize(int device);
/* Every ibo_dev_alloc allocation carries a generation: a process-wide counter value taken at allocation and again by each
 * ibo_memcpy_h2d into it (0 for memory this library did not allocate).  State kept per candidate array
 * (ibo_acq_sweep_incremental) is keyed on it, never on the address, which hipFree / hipMalloc recycle. */
int ibo_dev_generation(int device, const void *dev_ptr, uint64_t *generation);

/* ---------------------------------------------------------------- model (fit) */
int ibo_gp_create(int device, ibo_gp_t **out);
int ibo_gp_destroy(ibo_gp_t *gp);

/*
 * Fit: replaces GaussianProcess._computeCorrelations + linalg.cholesky
 * (ego/gaussianprocess/__init__.py:134-149,294-299) and the per-call
 * linalg.inv(R) of cdirectGP (ego/acquisition/__init__.py:385-388).
 *   R = K(X,X) with diagonal 1+noise;  L = chol(R);  W = L^-1 (explicit,
 *   kept in an MFMA-fragment layout);  alphaY = R^-1 Y, alpha1 = R^-1 1.
 * hyper: nhyper doubles per kernel type (see IBO_K_*); sf2 multiplies the
 * kernel (1 for SE kernels, magnitude^2 for SV / Matern in the Python model).
 * On IBO_ERR_NOT_PD *info (optional) receives the 1-based failing pivot.
 * 1 <= D <= 64 (IBO_ERR_ARG otherwise; the reference has no limit, its tests and demos stay below 7).  Up to 32 dimensions
 * the exponent-GEMM kernels take the sweeps; 33 .. 64 run through the difference-form kernels only (and without the kept
 * state of ibo_acq_sweep_incremental: every call is a full sweep).
 */
int ibo_gp_fit(ibo_gp_t *gp, int ktype, int N, int D,
               const double *X_host, const double *Y_host,
               const double *hyper_host, int nhyper, double sf2, double noise,
               int *info);

/*
 * Same, but factor a caller-supplied symmetric matrix A (N x N, host) in place
 * of R: PrefGaussianProcess uses A = R + C^-1
 * (ego/gaussianprocess/__init__.py:487-498, ego/acquisition/__init__.py:385-386).
 * R itself stays available (ibo_gp_get_R) because callers read GP.R.
 */
int ibo_gp_fit_with_matrix(ibo_gp_t *gp, int ktype, int N, int D,
                           const double *X_host, const double *Y_host,
                           const double *hyper_host, int nhyper, double sf2, double noise,
                           const double *A_host, int *info);

/*
 * Append n observations (Xnew_host: n x D) to a fitted model WITHOUT refactoring: the block extension of
 * GaussianProcess.addData (ego/gaussianprocess/__init__.py:301-308: z = solve(L, m), d = chol(r - z^T z)),
 * one point at a time, O(N^2) per point.  Y_all_host holds all N + n targets.  R, L, W and both alpha vectors
 * are updated in place on the device.  Returns IBO_ERR_STATE -- and changes nothing -- when the handle cannot
 * be extended (never fitted, fitted from a caller-supplied matrix or from an inverse, or N + n exceeds the
 * row padding, a multiple of 64): the caller then calls ibo_gp_fit with all the data.  IBO_ERR_NOT_PD as
 * ibo_gp_fit, and any other error, leave the handle UNFITTED (every later call returns IBO_ERR_STATE until a refit).
 */
int ibo_gp_extend(ibo_gp_t *gp, int n, const double *Xnew_host, const double *Y_all_host, int *info);
/* head-room: later fits of this handle pad the matrices to a multiple of 64 that leaves at least `rows` free rows, so
 * that many observations can be appended by ibo_gp_extend before a refit is due (a gallery of n points on a model
 * whose size is a multiple of 64 would otherwise refit, and sweep in full, in its very first round) */
int ibo_gp_reserve(ibo_gp_t *gp, int rows);

/*
 * Take n observations out of a fitted model WITHOUT refactoring: per removed row the rank-one update of the trailing factor and of its
 * inverse from the L and W = L^-1 the handle holds (two scans, O(N^2), no factorisation), one row at a time in descending index order.
 * rows_host: n distinct 0-based indices in [0, N), in any order (the same set gives the same bits in any order).  Y_rest_host: the N - n
 * remaining targets in their new order (the caller owns Y, as in ibo_gp_extend).  L, W, both alpha vectors and the points are rewritten on
 * the device; R is formed again on request; a kept sweep state is dropped; the row padding stays, so every removed row is head-room for
 * ibo_gp_extend.  IBO_ERR_ARG -- and nothing changed -- for a NULL argument, n < 1, n >= N, an index out of range or given twice.
 * IBO_ERR_STATE -- and nothing changed -- when the handle's factor is not that of its own kernel matrix (never fitted, fitted from a
 * caller-supplied matrix or from an inverse): the caller then calls ibo_gp_fit with the remaining data.  IBO_ERR_NOT_PD (info: the 1-based
 * row whose step was refused -- W[i][i] not finite and positive, or a sum not finite), and any other error, leave the handle UNFITTED.
 * Fixed-order sums: the same call on the same model gives the same bits.  Any fitted size (up to 23168 rows).
 */
int ibo_gp_remove(ibo_gp_t *gp, int n, const int *rows_host, const double *Y_rest_host, int *info);

/*
 * Preference GP on the device (PrefGaussianProcess.addPreferences, ego/gaussianprocess/__init__.py:347-498: the MAP of
 *     S(y) = -sum_pairs (d+1) log Phi((y_v - y_u)/sqrt 2) + y^T R^-1 y / 2     (:351-385)
 * and then L = chol(R + C^-1), :459-498).  The host keeps what is O(pairs) -- Phi, its derivatives, the line search --
 * and the device everything that is N x N: only vectors and the distinct entries of the pair sums cross the bus
 * (round 1 shipped an N x N Hessian per Newton step through ibo_spd_solve, and C and C^-1 through ibo_spd_inverse).
 *   ibo_pref_begin        after a plain ibo_gp_fit of the points: R^-1 = W^T W is formed on the handle.  The workspace belongs to the
 *                         model as it is at this call -- this fit, this number of rows, this padding.  After ibo_gp_extend,
 *                         ibo_gp_remove or another fit of the handle (one that failed included) the three entries below return
 *                         IBO_ERR_STATE, with handle and outputs untouched, until ibo_pref_begin is called again.  ibo_gp_set_y,
 *                         ibo_gp_set_prior and ibo_gp_set_kstar_sf2 leave it valid: R does not depend on them.
 *   ibo_pref_rinv_mul     out = R^-1 y
 *   ibo_pref_newton_step  H = R^-1 + sum of the sparse term (lin[e] = row * N + col, distinct entries: the host sums
 *                         the per-pair contributions rho (e_v - e_u)(e_v - e_u)^T); delta = -H^-1 grad; rdelta = R^-1 delta
 *   ibo_pref_finish       C = diag I + sparse term; the handle is refactored from R + C^-1 exactly as
 *                         ibo_gp_fit_with_matrix would (Y as set by ibo_gp_set_y).  IBO_ERR_NOT_PD: call again with a
 *                         larger diag (the reference's regulariser loop, :489-497) or refit: the workspace survives that failure,
 *                         and a successful call (the same points, the same R: it may be repeated with another C).  After a success
 *                         the model is no plain fit any more, so ibo_pref_rinv_mul and ibo_pref_newton_step return IBO_ERR_STATE.
 */
int ibo_pref_begin(ibo_gp_t *gp);
int ibo_pref_rinv_mul(ibo_gp_t *gp, const double *y_host, double *out_host);
int ibo_pref_newton_step(ibo_gp_t *gp, int nnz, const int64_t *lin_host, const double *val_host,
                         const double *grad_host, double *delta_host, double *rdelta_host, int *info);
int ibo_pref_finish(ibo_gp_t *gp, int nnz, const int64_t *lin_host, const double *val_host, double diag, int *info);

/* replace Y (and the alpha vectors) without refactoring: the preference GP's
 * C-matrix loop re-reads mu with L fixed (ego/gaussianprocess/__init__.py:476) */
int ibo_gp_set_y(ibo_gp_t *gp, const double *Y_host);

/* signal variance used for the CROSS-covariances k(x_i, c) of later sweeps only.
 * libego evaluates k* with sf2 = 1 for kernel types 0-2 whatever the Python
 * kernel's magnitude (cpp/optimizeGP.cpp:303-310) while R was built with it; a
 * drop-in maximize* sets this to reproduce that, then restores it. */
int ibo_gp_set_kstar_sf2(ibo_gp_t *gp, double sf2);

/* RBF-network mean prior m(x) = sum_i beta_i exp(-theta |(x-lowerb)/width - mean_i|^2)
 * (ego/gaussianprocess/prior.py:60-66, cpp/optimizeGP.cpp:116-133); nb = 0 clears it */
int ibo_gp_set_prior(ibo_gp_t *gp, int nb, const double *means_host, const double *beta_host,
                     double theta, const double *lowerb_host, const double *width_host);

/* copy the public attributes back (N x N row-major each).  R = K(X, X) with the reference's diagonal 1 + noise is formed on the
 * first request after a fit (a fit itself only needs its factor; ibo_gp_extend keeps a formed R up to date) */
int ibo_gp_get_R(ibo_gp_t *gp, double *R_host);
int ibo_gp_get_L(ibo_gp_t *gp, double *L_host);
/* W = L^-1 (N x N, lower triangular), and R^-1 = W^T W if wanted by a caller */
int ibo_gp_get_W(ibo_gp_t *gp, double *W_host);
/*
 * Leave-one-out predictions of the fitted model at its own points, from the factor the handle holds (O(N^2), one pass over W): with A the
 * matrix the handle factored (R with diagonal 1 + noise, or what ibo_gp_fit_with_matrix was given), d_i = (A^-1)_ii = |column i of W|^2 and
 * c = aY - m(x_i) a1 (m: the mean prior, if any; the reference subtracts the query's prior from every target):
 *     mu_host[i] = Y_i - c_i / d_i        s2_host[i] = 1 / d_i        *nloo_host = sum_i [-log(d_i) / 2 + c_i^2 / (2 d_i)] + N log(2 pi) / 2
 * i.e. the posterior at x_i of the model fitted WITHOUT observation i (the variance includes the noise, as ibo_posterior_batch's does) and the
 * negative leave-one-out log predictive probability.  UNCLIPPED: ibo_posterior_batch clips its variance to [clamp_lo, 10] (Python: [1e-7, 10]),
 * this does not.  Any output may be NULL, not all of them (IBO_ERR_ARG); IBO_ERR_STATE before a successful fit.  Works after ibo_gp_extend.
 * Fixed-order sums: the same call gives the same bits.
 */
int ibo_gp_loo(ibo_gp_t *gp, double *mu_host, double *s2_host, double *nloo_host);
int ibo_gp_info(ibo_gp_t *gp, int *N, int *D, int *device, double *max_y);
/* milliseconds of the last fit, device-side (hipEvent) */
int ibo_gp_last_fit_ms(ibo_gp_t *gp, float *ms);

/* covariance matrix only (no factorisation): Kernel.covMatrix / _computeCorrelations.
 * A2 may be NULL (square K(A1,A1) with the chosen diagonal rule) or a second
 * point set (cross-covariance K(A1,A2), n1 x n2, no diagonal rule).  n1 >= 1, and n2 >= 1 when A2 is given
 * (IBO_ERR_ARG otherwise). */
int ibo_cov_matrix(int device, int ktype, int D, const double *hyper_host, int nhyper, double sf2,
                   int n1, const double *A1_host, int n2, const double *A2_host,
                   int diag_rule, double noise, double *K_host);

/* X = A^-1 B for a symmetric positive-definite A (N x N) and nrhs right-hand sides (B, X:
 * nrhs x N row-major), all host buffers: blocked Cholesky + explicit L^-1 on the GPU.  The
 * preference GP's MAP (ego/gaussianprocess/__init__.py:442) runs Newton steps through this:
 * the Hessian of its functional is R^-1 plus the preference terms.  IBO_ERR_NOT_PD / *info
 * as ibo_gp_fit. */
int ibo_spd_solve(int device, int N, const double *A_host, int nrhs, const double *B_host,
                  double *X_host, int *info);

/* A^-1 of a symmetric positive-definite A (N x N, host in / host out) = W^T W with W = chol(A)^-1.
 * Replaces linalg.inv(self.C) of the preference GP (ego/gaussianprocess/__init__.py:488,514). */
int ibo_spd_inverse(int device, int N, const double *A_host, double *Ainv_host, int *info);

/* ---------------------------------------------------------------- posterior / sweep */
/*
 * Batched posterior: replaces GaussianProcess.posterior / posteriors / mu
 * (ego/gaussianprocess/__init__.py:169-254).  clamp_lo = 1e-7 reproduces the
 * Python clip(.., 10e-8, 10), 1e-8 the native clamp (cpp/optimizeGP.cpp:150-157).
 * Host buffers in and out (PCIe-inclusive).  s2_host may be NULL.
 */
int ibo_posterior_batch(ibo_gp_t *gp, int64_t M, const double *Q_host, double clamp_lo,
                        double *mu_host, double *s2_host);

/*
 * The same evaluation for points that live on the HOST (Q_host: M x D), results into host arrays (any of mu_host,
 * s2_host, acq_host may be NULL): EI / PI / UCB.negf(x) and their vectorised forms (ego/acquisition/__init__.py:47-166).
 * ymax NaN = max(Y).  Small batches cost no allocation and no copy launch; from 2^18 points on upload, sweep and download
 * are pipelined in chunks.  ibo_posterior_batch is this with acq = IBO_ACQ_NONE.
 */
int ibo_acq_batch(ibo_gp_t *gp, int64_t M, const double *Q_host, int acq, double parm, int erf_mode,
                  double clamp_lo, double ymax, double *mu_host, double *s2_host, double *acq_host);

/*
 * ibo_acq_batch plus the gradients with respect to the query point: dmu_host, ds2_host, dacq_host are M x D row-major,
 * d/dx_d of mu, of the clipped sigma^2 and of the acquisition at each point.  Any output may be NULL, not all of them.
 * mu / s2 / acq are ibo_acq_batch's numbers bit for bit.  With acq = IBO_ACQ_NONE only posterior gradients are formed
 * and dacq_host must be NULL.  Conventions as the sweep: k* with the handle's k* signal variance (ibo_gp_set_kstar_sf2);
 * mu = m + k*.aY - m k*.a1 (m: the mean prior, if any); sigma^2 = 1 + noise - |W k*|^2 clipped to [clamp_lo, 10].
 *   dmu   = dm (1 - k*.a1) + sum_i dk*_i (aY_i - m a1_i)
 *   ds2   = -2 sum_i dk*_i u_i with u = W^T (W k*) = R^-1 k*, and exactly 0 where the clip is active (raw sigma^2 outside
 *           the open interval (clamp_lo, 10))
 *   EI    = Phi(z) dmu + phi(z) dsigma;  PI = phi(z) (dmu - z dsigma) / sigma;  UCB = dmu + parm dsigma
 *           (z = (mu - ymax - parm) / sigma, dsigma = ds2 / (2 sigma); Phi, phi of the erf flavour.  This is the analytic
 *           gradient: with IBO_ERF_NR, whose constants 0.707106 and 0.398942 are truncated, it differs from the derivative
 *           of the returned values by about 1e-6 relative.)
 * Cost per point: 2 N^2 flops (two triangular products) + O(N D).  Sums run in a fixed order: the same call gives the
 * same bits.  Works for every model the handle can be fitted with (1 <= D <= 64, any N); the scratch is bounded by one
 * chunk of candidates (192 MiB, or one tile of 64 candidates where that alone is larger: about 290 MiB at 20480 rows).
 * IBO_ERR_STATE before a fit; IBO_ERR_ARG for M < 1, NULL Q_host, a bad acq or erf_mode, or every output NULL.
 */
int ibo_acq_grad_batch(ibo_gp_t *gp, int64_t M, const double *Q_host, int acq, double parm, int erf_mode,
                       double clamp_lo, double ymax, double *mu_host, double *s2_host, double *acq_host,
                       double *dmu_host, double *ds2_host, double *dacq_host);

/*
 * The joint posterior of M query points Q (M x D row-major): S_host (M x M row-major) receives
 *   S_ab = k(q_a, q_b) - v_a.v_b  (a != b),   S_aa = 1 + noise - |v_a|^2 (with_noise = 1) or 1 - |v_a|^2 (with_noise = 0),
 * v_a = W k*(q_a), W = L^-1 as the handle holds it (a preference GP: its own factor of R + C^-1), k and k* with the handle's
 * k* signal variance (ibo_gp_set_kstar_sf2).  That is the Schur complement of the fitted matrix extended by the query rows:
 * diag(S) with with_noise = 1 is ibo_posterior_batch's s2 before its clip, and observing q_b turns the variance at q_a into
 * S_aa - S_ab^2 / S_bb.  S is unclipped and exactly symmetric (the lower 64 x 64 tiles are formed and mirrored).
 * mu_host (M, may be NULL) receives ibo_posterior_batch's mean, bit for bit (its launches run first).
 * Cost: N^2 M flops for V = W K* (W's blocks above the diagonal skipped) + N M^2 for the lower half of V^T V, on the fp64 MFMA
 * pipe, in a fixed order: the same call gives the same bits.  Device scratch: M^2 + M Npad doubles + one chunk of K* (256 MiB
 * at most), returned to the pool before the call returns.
 * 1 <= M <= IBO_COV_MAX_M (S is 2^31 bytes there).  IBO_ERR_NO_DEVICE without a device (checked first); IBO_ERR_ARG for M
 * outside the limit or a NULL gp, Q_host or S_host; IBO_ERR_STATE before a fit.
 */
#define IBO_COV_MAX_M 16384
int ibo_posterior_cov(ibo_gp_t *gp, int64_t M, const double *Q_host, int with_noise,
                      double *mu_host, double *S_host);

/*
 * nsamp zero-mean draws from the joint posterior of ibo_posterior_cov: S + jitter I is formed on the device (with the identity
 * padding of the in-place factorisation) and factored there, S + jitter I = L_S L_S^T (the route of ibo_spd_*: panel 1 up to
 * 2048 rows, panels of four beyond), and F_host (nsamp x M row-major) receives F[s] = L_S Z[s] for the rows Z[s] of Z_host
 * (nsamp x M row-major).  S never reaches the host; the mean is not added (mu_host, M and optional, receives it as
 * ibo_posterior_cov does), so a caller may take it from another handle.  Cost: ibo_posterior_cov's + M^3 / 3 for the
 * factorisation + M^2 nsamp for the product.  Device scratch: Mp^2 + 2 nsamp_p Mp doubles (Mp, nsamp_p: rounded up to 64) on
 * top of ibo_posterior_cov's, without its M^2.
 * IBO_ERR_NOT_PD when the factorisation fails: *info (optional) the 1-based failing pivot, as dpotrf's info (0 otherwise).
 * 1 <= M <= IBO_SAMPLE_MAX_M, 1 <= nsamp <= IBO_SAMPLE_MAX_DRAWS, jitter finite and >= 0: IBO_ERR_ARG otherwise, and for a
 * NULL gp, Q_host, Z_host or F_host.  IBO_ERR_NO_DEVICE without a device (checked first); IBO_ERR_STATE before a fit.
 */
#define IBO_SAMPLE_MAX_M 16384
#define IBO_SAMPLE_MAX_DRAWS 4096
int ibo_posterior_sample(ibo_gp_t *gp, int64_t M, const double *Q_host, int with_noise, double jitter,
                         int nsamp, const double *Z_host, double *F_host, double *mu_host, int *info);

/*
 * Fused candidate sweep: the batched equivalent of M calls of
 * GP_Maximizer::negei/negpi/negucb (cpp/optimizeGP.cpp:57-236), i.e. what
 * maximizeEI/PI/UCB evaluate inside DIRECT and what fastUCBGallery's
 * latin-hypercube step evaluates (ego/acquisition/gallery.py:111-116).
 *
 *   cand_dev     M x D candidates, DEVICE memory, row-major
 *   acq          IBO_ACQ_*;  parm = xi (EI/PI) or the sigma multiplier (UCB)
 *   ymax         incumbent; pass NAN to use max(Y) as acqmaxGP does (:316-321)
 *   excl_host    n_excl x D points (host) -- candidates with
 *                min_j |c - excl_j|_2 <= excl_radius are left out of the argmax
 *                (the gallery's 0.5-distance rule, gallery.py:102,113); n_excl=0: none
 *   index_base   added to the local row index to form the reported index
 *                (global index of this rank's shard)
 *   mu_dev, s2_dev, acq_dev   optional DEVICE outputs (M doubles each) or NULL
 *   best_val, best_idx        HOST outputs: maximum of the (positive) acquisition
 *                and the FIRST index attaining it (numpy.argmax order, and the
 *                strict '<' of cpp/direct.cpp:124).  NaN values never win; a candidate
 *                with a NaN coordinate has NaN outputs (and so never wins either).
 *                When nothing is admissible -- every candidate excluded or NaN --
 *                best_idx = -1 (index_base is NOT added) and best_val = -INFINITY,
 *                on every route and in every entry that reports an arg-max
 *                (ibo_acq_sweep_incremental, ibo_acq_sweep_exchange, ibo_cacq_sweep,
 *                ibo_kg_sweep).  tests/test_gpu_argmax_contract.py holds every
 *                kernel to this rule at its reduction boundaries.
 * Blocking.  The posterior part costs N^2 + 3ND + 4N flops per candidate.
 */
int ibo_acq_sweep(ibo_gp_t *gp, int64_t M, const double *cand_dev,
                  int acq, double parm, int erf_mode, double clamp_lo, double ymax,
                  int n_excl, const double *excl_host, double excl_radius,
                  int64_t index_base,
                  double *mu_dev, double *s2_dev, double *acq_dev,
                  double *best_val, int64_t *best_idx);

/*
 * ibo_acq_sweep for a caller that sweeps the SAME device candidate array again and again while the model grows by
 * ibo_gp_extend -- fastUCBGallery's rounds (ego/acquisition/gallery.py:92-134: one hallucinated observation per
 * round, the same sample set).  The first call is a full sweep and leaves q = |W k*|^2 (and the two mean terms) per
 * candidate on the handle, 24 bytes each.  A later call with the same array, after at most 8 rows were appended and
 * nothing else changed, folds the new rows of W into q -- (w_new . k*)^2, O(N) per candidate instead of O(N^2) --
 * re-forms the means from the current alpha vectors and evaluates the acquisition as usual.  Anything else (other
 * array or size, a refit, ibo_gp_set_y, another k* variance, batches small enough for the other kernels) is a full sweep.
 * "The same array" means the same ibo_dev_alloc allocation at the same GENERATION (ibo_dev_generation) and offset: an
 * array that was freed and reallocated at the same address, or overwritten through ibo_memcpy_h2d, is a different one,
 * and memory the library did not allocate is swept in full every time.  Contents changed behind the library's back (the
 * caller's own kernels or hipMemcpy) are the one thing it cannot see.
 *
 * When only the arg-max is asked for (mu_dev, s2_dev and acq_dev all NULL) and the acquisition grows with the variance
 * (IBO_ACQ_EI, IBO_ACQ_UCB with parm >= 0), the state is formed in LEVELS of W's rows, split at about N/8, N/4 and N/2 (multiples
 * of 128): level 0, rows [0, N/8) -- 1/64 of the work: W is triangular -- for every candidate, together with the means; each later
 * level only for the 32-candidate tiles whose BOUND -- the acquisition at the variance 1 + noise - q(rows so far), which can only
 * shrink as rows are added -- reaches a value that a complete candidate attains (the top 3 % of the level-0 ranking are completed
 * first to supply it).  The returned (best_val, best_idx) are those of the full sweep: a tile left incomplete cannot hold the
 * maximum.  ibo_set_option("part_levels", 2 | 3 | 4) caps the levels of states formed afterwards (2: one split at N/2, rounds 2-3).
 * Later calls are lazy too: the complete tiles fold in the rows appended since, the best value they reach is the threshold,
 * and only tiles whose bound -- from their stale state, the means widened by nu_max sum |(W y)_i| over the appended rows (nu_max =
 * sf2_k / sqrt(sf2_fit) bounds |W k*|; no lazy mode where the fitted matrix admits no such bound):
 * nothing for observations on the posterior mean (the gallery's), everything for real ones -- reaches it are refreshed and
 * completed.  A call that wants per-candidate outputs (or IBO_ACQ_PI / IBO_ACQ_NONE), or a model with a mean prior, refreshes
 * and completes every tile first.
 * 512 <= padded rows <= 4096; 40 bytes of state per candidate.  ibo_set_option("gallery_prune", 0) restores the one-kernel
 * first sweep, 2 runs the same launches with every tile completed (what the pruned run is tested against, bit for bit).
 */
int ibo_acq_sweep_incremental(ibo_gp_t *gp, int64_t M, const double *cand_dev,
                              int acq, double parm, int erf_mode, double clamp_lo, double ymax,
                              int n_excl, const double *excl_host, double excl_radius,
                              int64_t index_base,
                              double *mu_dev, double *s2_dev, double *acq_dev,
                              double *best_val, int64_t *best_idx);

/* the kept state of ibo_acq_sweep_incremental: its 32-candidate tiles and how many of them carry their full variance
 * (equal unless the state was formed in two parts); both 0 when the handle keeps no state */
int ibo_sweep_state_info(ibo_gp_t *gp, int64_t *tiles, int64_t *complete);
/* the same in detail: the state's number of levels (1: formed by the one-kernel sweep or none), splits[3] = the rows where
 * levels 1, 2, 3 begin (0 beyond nlev - 1), tiles_at_level[4] = how many tiles stand at each level (a tile at level
 * nlev - 1 is complete) */
int ibo_sweep_state_levels(ibo_gp_t *gp, int *nlev, int *splits, int64_t *tiles_at_level);

/* device-side duration (hipEvent, ms) of the dominant kernel of the last
 * ibo_acq_sweep / ibo_posterior_batch on this handle, and its name */
int ibo_last_sweep_kernel_ms(ibo_gp_t *gp, float *ms, const char **kernel_name);

/* ---------------------------------------------------------------- DIRECT on the GPU objective */
/*
 * maximise an acquisition over a box with the reference's DIRECT
 * (cpp/direct.cpp:329-581) -- tree logic on the host, every batch of new
 * sample points evaluated by the sweep kernel.  compat != 0 reproduces the
 * reference's trajectory quirks incl. the dimension-0 stall;
 * compat == 0 applies the fixed-dimension test to dimension 0 as well.
 * opt = maximum of the acquisition, optx[D] its location, nsamples optional.
 */
int ibo_direct_max(ibo_gp_t *gp, int D, const double *lb, const double *ub,
                   int acq, double parm, int erf_mode, double clamp_lo,
                   int maxiter, int maxtime, int maxsample, int compat,
                   double *opt, double *optx, int64_t *nsamples);

/* ---------------------------------------------------------------- constrained acquisition over several handles */
/*
 * EI / PI of an objective model weighted by the probability that up to IBO_CACQ_MAX_CON constraint models are feasible (Schonlau
 * 1998; Gardner et al. 2014; Gelbart et al. 2014).  Every handle has its own X, N, kernel, noise, prior and k* signal variance;
 * they share D and the device.  With (mu_j, sigma_j^2) what ibo_acq_batch returns for constraint handle con[j] at x (variance
 * clipped to [clamp_lo, 10]):
 *   z_j  = sense_j (thresh_j - mu_j) / sigma_j     sense_j = +1: feasible where c_j(x) <= thresh_j;  -1: where c_j(x) >= thresh_j
 *   P(x) = prod_j Phi(z_j)                          (ncon = 0: 1)
 *   A(x) = the objective's IBO_ACQ_EI / IBO_ACQ_PI with the call's parm, ymax, erf_mode;  IBO_ACQ_NONE: A = 1, the pure
 *          probability of feasibility (what one maximises while no feasible point is known);  IBO_ACQ_UCB: IBO_ERR_ARG (a signed
 *          value times a probability orders nothing)
 *   val(x) = A(x) P(x), multiplied in the order A, Phi(z_0), Phi(z_1), ...
 * Phi and phi are those of the call's erf_mode for the constraints as for the objective (IBO_ERF_NR: the truncated constants too).
 * ymax NaN = max(Y) of the objective handle, as in ibo_acq_sweep; callers normally pass the best FEASIBLE observation.  A handle
 * may appear more than once (objective and constraint, or two constraints for a band): the handles are evaluated one after the
 * other.  A call leaves each handle as a plain ibo_acq_sweep / ibo_acq_batch on it would (k* variance, prior, kept sweep state).
 *
 * Errors, all four entries: IBO_ERR_NO_DEVICE without a device (checked first); IBO_ERR_ARG for a NULL obj, ncon outside
 * [0, IBO_CACQ_MAX_CON], NULL con / thresh / sense or a NULL con[j] with ncon > 0, a sense other than +1 / -1, a non-finite
 * threshold, handles on different devices or with different D, M < 1, a NULL point array, IBO_ACQ_UCB or an unknown acq / erf_mode,
 * every output NULL; IBO_ERR_STATE if any handle is not fitted.
 */
#define IBO_CACQ_MAX_CON 8

/*
 * The sweep: cand_dev (M x D, DEVICE) and the exclusion balls, index_base and arg-max rule of ibo_acq_sweep -- NaN values and
 * excluded candidates never win, the largest val wins, the lowest index wins ties (every val 0.0: the first candidate that is not
 * excluded), best_idx = -1 when everything is excluded.  acq_dev, pof_dev, val_dev: optional DEVICE outputs (M doubles each): A, P,
 * val.  With ncon = 0, best_val, best_idx and acq_dev are ibo_acq_sweep's, bit for bit.
 * Cost: one plain sweep per model (the objective's is skipped for IBO_ACQ_NONE) plus one streaming pass of 16 (ncon + 1) bytes per
 * candidate; that many bytes of device scratch, at most about 1 GiB (more candidates run in chunks), returned before the call
 * returns.  Blocking.
 */
int ibo_cacq_sweep(ibo_gp_t *obj, int ncon, ibo_gp_t *const *con, const double *thresh, const int *sense,
                   int64_t M, const double *cand_dev, int acq, double parm, int erf_mode, double clamp_lo, double ymax,
                   int n_excl, const double *excl_host, double excl_radius, int64_t index_base,
                   double *acq_dev, double *pof_dev, double *val_dev,
                   double *best_val, int64_t *best_idx);

/*
 * The same values for points on the HOST (Q_host: M x D), into host arrays (any of acq_host, pof_host, val_host may be NULL, not
 * all): one ibo_acq_batch per handle, combined on the host.  acq_host is ibo_acq_batch's acquisition of the objective, bit for bit.
 */
int ibo_cacq_batch(ibo_gp_t *obj, int ncon, ibo_gp_t *const *con, const double *thresh, const int *sense,
                   int64_t M, const double *Q_host, int acq, double parm, int erf_mode, double clamp_lo, double ymax,
                   double *acq_host, double *pof_host, double *val_host);

/*
 * ibo_cacq_batch's val (val_host, bit for bit) and its gradient with respect to the query point (dval_host: M x D row-major),
 * composed on the host from ibo_acq_grad_batch per handle, in a fixed order and without dividing by Phi (finite where a factor
 * underflows):
 *   dsigma_j = dsigma^2_j / (2 sigma_j)            (0 where handle j's clip is active, as ibo_acq_grad_batch defines it)
 *   dz_j     = -(sense_j dmu_j + z_j dsigma_j) / sigma_j
 *   dP       = sum_j phi(z_j) dz_j prod_{i != j} Phi(z_i)
 *   dval     = dA P + A dP                          (dA = ibo_acq_grad_batch's dacq; 0 for IBO_ACQ_NONE)
 * Either output may be NULL, not both.  Cost: ibo_acq_grad_batch's per handle.  The analytic gradient: with IBO_ERF_NR it differs
 * from the derivative of the returned values by about 1e-6 relative (see ibo_acq_grad_batch).
 */
int ibo_cacq_grad_batch(ibo_gp_t *obj, int ncon, ibo_gp_t *const *con, const double *thresh, const int *sense,
                        int64_t M, const double *Q_host, int acq, double parm, int erf_mode, double clamp_lo, double ymax,
                        double *val_host, double *dval_host);

/*
 * ibo_direct_max on val: the same DIRECT, options and batched schedule, every batch of sample points evaluated as
 * ibo_cacq_batch does.  opt = the maximum of val, optx[D] its location, nsamples optional (not all three NULL).  IBO_ERR_ARG
 * also for NULL bounds or D other than the models'.
 */
int ibo_cacq_direct_max(ibo_gp_t *obj, int ncon, ibo_gp_t *const *con, const double *thresh, const int *sense,
                        int D, const double *lb, const double *ub, int acq, double parm, int erf_mode, double clamp_lo, double ymax,
                        int maxiter, int maxtime, int maxsample, int compat,
                        double *opt, double *optx, int64_t *nsamples);

/* ---------------------------------------------------------------- expected hypervolume improvement (two objectives) */
/*
 * Two objectives, each known through its own fitted handle obj[0], obj[1] (a handle may be both; a preference GP may be either), both to
 * be MAXIMISED, assumed independent; a reference point ref = (r1, r2); a front: nfront points (front_host, nfront x 2 row-major, host
 * memory) in objective space.  The acquisition is the expected growth of the hypervolume the front dominates above ref after one
 * observation of both objectives at x (Emmerich et al. 2006; Yang et al. 2019) -- in closed form.  The reference has no counterpart: its
 * acquisitions (ego/acquisition/__init__.py) rank candidates for one objective only.
 *
 * The front's canonical form (made on the host by every entry): points not strictly above ref in BOTH coordinates go, then dominated
 * points and duplicates; the rest sorted ascending in the first coordinate, (a_1, b_1) .. (a_n, b_n) -- b is then strictly descending --
 * with a_0 = r1, a_{n+1} = +inf, b_{n+1} = r2.  n <= IBO_EHVI_MAX_FRONT after that (nfront itself is not limited).
 * With (mu_k, s2_k) what ibo_acq_sweep returns for obj[k] with IBO_ACQ_NONE at the call's clamp_lo, sigma_k = sqrt(s2_k):
 *   psi_k(t) = sigma_k phi(u) + (mu_k - t) Phi(u),  u = (mu_k - t) / sigma_k        (EI over t with parm 0; psi_1(+inf) = 0, never evaluated)
 *   d_i      = psi_1(a_i) - psi_1(a_{i+1}), and 0 where that is negative              i = 0 .. n
 *   EHVI(x)  = sum_i d_i psi_2(b_{i+1})                                              i ascending, plain fp64, no fused multiply-add
 * (the improvement split into the n + 1 vertical strips between neighbouring a's; an empty front: EI_1(r1) EI_2(r2)).  Phi and phi in the
 * call's erf_mode.  A NaN (a NaN candidate coordinate) stays a NaN and never wins the arg-max.
 * Every entry computes a candidate's value the same way: the two plain sweeps into device scratch, then one kernel (ehvi.hip) with one
 * candidate per lane that walks the strips in order.  The kernel adds nothing of its own to the bits: they are a function of the
 * candidate's (mu_k, s2_k) and the canonical front.  ibo_acq_sweep picks its kernels by the size of the launch, and its routes agree with
 * each other to rounding only; so a short launch is padded here (candidates at the origin, nobody reads their results) to the size class of
 * the call's chunk -- min(M, the chunk): up to 4096 the small-batch kernels (launches of up to 128 candidates run as 160), above that the
 * large-batch kernel (a tail of up to 4096 runs as 4097).  Within a class the sweep, a host batch, the gradient entry's value and the value
 * DIRECT reports agree bit for bit, whatever M, the candidate's place and "ehvi_chunk" are; between the classes, and for a model whose
 * inputs keep it off the dot form, to rounding.
 *
 * Errors, all four entries, in this order: IBO_ERR_NO_DEVICE without a device; IBO_ERR_ARG for a NULL obj, obj[0] or obj[1], handles on
 * different devices, nfront < 0, a NULL front_host with nfront > 0, a NULL ref, M < 1, a NULL point array, an unknown erf_mode, every
 * output NULL, a non-finite ref, a NaN or an infinity in front_host, more than IBO_EHVI_MAX_FRONT points left after canonicalisation;
 * IBO_ERR_STATE if a handle is not fitted; IBO_ERR_ARG if the handles differ in D.
 */
#define IBO_EHVI_MAX_FRONT 1024

/*
 * The sweep: cand_dev (M x D, DEVICE) and the exclusion balls, index_base and arg-max rule of ibo_acq_sweep -- NaN values and excluded
 * candidates never win, the largest value wins, the lowest index wins ties, best_idx = -1 and best_val = -inf when nothing is admissible.
 * val_dev: optional DEVICE output, M doubles.  Cost: the two plain sweeps plus 2 (n + 1) Gaussian cdf / pdf pairs per candidate; 32 bytes
 * of device scratch per candidate, at most 1 GiB (more candidates run in chunks), returned before the call returns.  Blocking.
 */
int ibo_ehvi_sweep(ibo_gp_t *const *obj, int nfront, const double *front_host, const double *ref,
                   int64_t M, const double *cand_dev, int erf_mode, double clamp_lo,
                   int n_excl, const double *excl_host, double excl_radius, int64_t index_base,
                   double *val_dev, double *best_val, int64_t *best_idx);

/* The same values for points on the HOST (Q_host: M x D) into val_host: the points are uploaded and go through the sweep's route. */
int ibo_ehvi_batch(ibo_gp_t *const *obj, int nfront, const double *front_host, const double *ref,
                   int64_t M, const double *Q_host, int erf_mode, double clamp_lo, double *val_host);

/*
 * ibo_ehvi_batch's value (val_host, bit for bit) and its gradient with respect to the query point (grad_host: M x D row-major).  The
 * kernel's second variant also sums, over the strips in the same order,
 *   G_mu1 = sum (Phi(u_1,i) - Phi(u_1,i+1)) psi_2(b_{i+1})      G_sigma1 = sum (phi(u_1,i) - phi(u_1,i+1)) psi_2(b_{i+1})     (0 where d_i was clamped)
 *   G_mu2 = sum d_i Phi(u_2,i+1)                                G_sigma2 = sum d_i phi(u_2,i+1)
 * and the host applies the chain rule to ibo_acq_grad_batch's (dmu_k, ds2_k) per handle, k = 0 then 1:
 *   grad EHVI = sum_k G_mu_k dmu_k + G_sigma_k ds2_k / (2 sigma_k)                  (ds2_k is 0 where handle k's clip is active)
 * Either output may be NULL, not both.  The analytic gradient: with IBO_ERF_NR it differs from the derivative of the returned values by
 * about 1e-6 relative (see ibo_acq_grad_batch).
 */
int ibo_ehvi_grad_batch(ibo_gp_t *const *obj, int nfront, const double *front_host, const double *ref,
                        int64_t M, const double *Q_host, int erf_mode, double clamp_lo, double *val_host, double *grad_host);

/*
 * ibo_direct_max on EHVI: the same DIRECT, options and batched schedule, every batch of sample points evaluated as ibo_ehvi_batch does.
 * opt = the maximum, optx[D] its location, nsamples optional (not all three NULL).  IBO_ERR_ARG also for NULL bounds or D other than
 * the models'.
 */
int ibo_ehvi_direct_max(ibo_gp_t *const *obj, int nfront, const double *front_host, const double *ref,
                        int D, const double *lb, const double *ub, int erf_mode, double clamp_lo,
                        int maxiter, int maxtime, int maxsample, int compat,
                        double *opt, double *optx, int64_t *nsamples);

/* With ibo_set_option("ehvi_timing", 1) every ibo_ehvi_* call of this thread waits after each launch of the scan kernel and adds its
 * device time (HIP events around that launch alone, not the per-model sweeps) to *ms.  reset != 0 clears the sum after it is read; ms may
 * be NULL.  A diagnostic: the option is process-wide, the sum is per thread. */
int ibo_ehvi_scan_ms(double *ms, int reset);

/* ---------------------------------------------------------------- max-value entropy search */
/*
 * Max-value entropy search (MES; Wang & Jegelka 2017): how much one observation at x tells about the VALUE of the maximum, y*.  One fitted
 * handle gp (a preference GP passes), K samples of y* (ystar_host, host memory, 1 <= K <= IBO_MES_MAX_SAMPLES -- PosteriorPaths.maxima's
 * exact draws, or draws from ibo_mes_maxcdf's Gumbel fit), clamp_lo and s2_offset >= 0.  The reference has no counterpart.
 *
 * Every entry sorts y* ascending on the host, so a value's bits do not depend on the caller's order.
 * With (mu, s2) what ibo_acq_sweep returns for gp with IBO_ACQ_NONE at the call's clamp_lo:
 *   v       = max(s2 - s2_offset, clamp_lo),  sigma = sqrt(v),  gamma_k = (y*_k - mu) / sigma
 *             (s2 is the predictive variance 1 + noise - |W k*|^2; the latent one is sf2 - |W k*|^2, so s2_offset = 1 + noise - sf2 asks for MES
 *             of the latent function and 0 for MES of an observation; a latent variance clipped away is floored at clamp_lo)
 *   MES(x)  = (1/K) sum_k h(gamma_k)                                                 k ascending, plain fp64, no fused multiply-add
 *   h(g)    = g lambda(g) / 2 - log Phi(g),  lambda = phi / Phi
 * -- h is the entropy of N(0, 1) minus the entropy of N(0, 1) truncated above at g.  0.5 (1 + erf) loses log Phi below g = -8 and above
 * g = 8, so h is evaluated in a tail-safe form, the same on every route (there is no erf_mode: nothing of the reference is mirrored):
 *   g >= 0:  q = erfc(g / sqrt 2) / 2,   lambda = phi(g) / (1 - q),       h = g lambda / 2 + (-log1p(-q))
 *   g <  0:  e = erfcx(-g / sqrt 2),     lambda = sqrt(2 / pi) / e,       h = g lambda / 2 + (g^2 / 2 - log(e / 2))
 *   phi(g) = exp(-(g^2 / 2)) / sqrt(2 pi)
 * A NaN (a NaN candidate coordinate) stays a NaN and never wins the arg-max.
 * Every entry computes a candidate's value the same way: per chunk one plain sweep into device scratch (16 bytes a candidate), then one
 * kernel (mes.hip) with one candidate per lane that sums its K terms in order; ystar is uploaded once per call.  Short launches are
 * padded to the two size classes exactly as the ibo_ehvi_* entries pad theirs, and the statement is the same: within a class the
 * sweep, a host batch, the gradient entry's value and the value DIRECT reports agree bit for bit, whatever M, the candidate's place and
 * "mes_chunk" are; between the classes, and for a model whose inputs keep it off the dot form, to rounding.
 *
 * Errors, the four value entries, in this order: IBO_ERR_ARG for what the samples alone decide, with or without a device -- K < 1 or
 * K > IBO_MES_MAX_SAMPLES, a NULL ystar_host, a NaN or an infinity in it, a negative or non-finite s2_offset; IBO_ERR_NO_DEVICE without
 * a device; IBO_ERR_ARG for a NULL gp, M < 1, a NULL point array, every output NULL; IBO_ERR_STATE if the handle is not fitted.
 */
#define IBO_MES_MAX_SAMPLES 1024
#define IBO_MES_MAX_LEVELS 64

/*
 * The sweep: cand_dev (M x D, DEVICE) and the exclusion balls, index_base and arg-max rule of ibo_acq_sweep -- NaN values and excluded
 * candidates never win, the largest value wins, the lowest index wins ties, best_idx = -1 and best_val = -inf when nothing is admissible.
 * val_dev: optional DEVICE output, M doubles.  Cost: the plain sweep plus K terms per candidate (an erfc or erfcx, an exp or a log each);
 * 16 bytes of device scratch per candidate, at most 1 GiB (more candidates run in chunks), returned before the call returns.  Blocking.
 */
int ibo_mes_sweep(ibo_gp_t *gp, int K, const double *ystar_host, double s2_offset,
                  int64_t M, const double *cand_dev, double clamp_lo,
                  int n_excl, const double *excl_host, double excl_radius, int64_t index_base,
                  double *val_dev, double *best_val, int64_t *best_idx);

/* The same values for points on the HOST (Q_host: M x D) into val_host: the points are uploaded and go through the sweep's route. */
int ibo_mes_batch(ibo_gp_t *gp, int K, const double *ystar_host, double s2_offset,
                  int64_t M, const double *Q_host, double clamp_lo, double *val_host);

/*
 * ibo_mes_batch's value (val_host, bit for bit) and its gradient with respect to the query point (grad_host: M x D row-major).  The
 * kernel's second variant also sums, over the samples in the same order, with h'(g) = -(lambda / 2) (1 + g^2 + g lambda),
 *   G_mu = (1/K) sum_k h'(gamma_k) (-1 / sigma)          G_sigma = (1/K) sum_k h'(gamma_k) (-gamma_k / sigma)
 * and the host applies the chain rule to ibo_acq_grad_batch's (dmu, ds2):
 *   grad MES = G_mu dmu + G_sigma ds2 / (2 sigma)         (ds2 is 0 where either clamp is active: the sweep's, or the floor of v)
 * Either output may be NULL, not both.
 */
int ibo_mes_grad_batch(ibo_gp_t *gp, int K, const double *ystar_host, double s2_offset,
                       int64_t M, const double *Q_host, double clamp_lo, double *val_host, double *grad_host);

/*
 * ibo_direct_max on MES: the same DIRECT, options and batched schedule, every batch of sample points evaluated as ibo_mes_batch does.
 * opt = the maximum, optx[D] its location, nsamples optional (not all three NULL).  IBO_ERR_ARG also for NULL bounds or D other than
 * the model's.
 */
int ibo_mes_direct_max(ibo_gp_t *gp, int K, const double *ystar_host, double s2_offset,
                       int D, const double *lb, const double *ub, double clamp_lo,
                       int maxiter, int maxtime, int maxsample, int compat,
                       double *opt, double *optx, int64_t *nsamples);

/*
 * What the Gumbel approximation of the max-value distribution is fitted to (Wang & Jegelka 2017, section 3.1): over the candidates
 * cand_dev (M x D, DEVICE), with (mu_i, sigma_i) as above (s2_offset, clamp_lo), for each of nlev levels t_k (lev_host, host memory,
 * 0 <= nlev <= IBO_MES_MAX_LEVELS)
 *   logcdf_host[k] = sum_i log Phi((t_k - mu_i) / sigma_i)          -- log P(max_i f(x_i) <= t_k) were the candidates independent
 * (log Phi in the tail-safe form above), and the bracket stats_host[0] = max_i mu_i, stats_host[1] = max_i (mu_i + 5 sigma_i).  nlev = 0
 * returns only the bracket (lev_host and logcdf_host may be NULL).  Candidates with a NaN posterior are skipped (in the sums and in the
 * bracket; with none left the bracket is -inf).  One kernel sums each block of 256 candidates in a fixed tree, a second launch adds the
 * block sums in ascending block order: the result's bits do not depend on "mes_chunk" (beyond the size classes of the plain sweep).
 * IBO_ERR_ARG, with or without a device, for nlev out of range, a NULL lev_host or logcdf_host with nlev > 0, a NaN level (+-inf
 * passes), a negative or non-finite s2_offset; IBO_ERR_NO_DEVICE without a device; IBO_ERR_ARG for a NULL gp, M < 1, a NULL cand_dev,
 * a NULL stats_host; IBO_ERR_STATE if the handle is not fitted.
 */
int ibo_mes_maxcdf(ibo_gp_t *gp, int64_t M, const double *cand_dev, int nlev, const double *lev_host, double s2_offset, double clamp_lo,
                   double *logcdf_host, double *stats_host);

/* With ibo_set_option("mes_timing", 1) every ibo_mes_* call of this thread waits after each launch of the scan kernel (the value
 * kernel, or ibo_mes_maxcdf's reduction) and adds its device time (HIP events around that launch alone, not the sweep) to *ms.
 * reset != 0 clears the sum after it is read; ms may be NULL.  A diagnostic: the option is process-wide, the sum is per thread. */
int ibo_mes_scan_ms(double *ms, int reset);

/* ---------------------------------------------------------------- knowledge gradient */
/*
 * The knowledge gradient of a candidate x against a reference set A = {a_1 .. a_n} (ref_host, nref x D row-major, host memory,
 * 1 <= nref <= IBO_KG_MAX_REF): the expected rise of the best posterior mean over the set after one more observation at x.
 * Conventions of ibo_posterior_cov: k and k* with the handle's k* signal variance, v = W k*, unclipped covariances.
 *   mu_a     the posterior mean at a, the mean prior included: m + k*.aY - m k*.a1 (ibo_acq_grad_batch's formula)
 *   s2_x     1 + noise - |v_x|^2 clipped to [clamp_lo, 10] (ibo_posterior_batch's rule), sigma_x = sqrt(s2_x)
 *   b_a(x)   (k(a, x) - v_a.v_x) / sigma_x: the change of mu_a per standard deviation of the new observation
 *   lines    with_self = 1: line 0 is the candidate's own, mu_0 = mu_x, b_0 = max(1 - |v_x|^2, 0) / sigma_x, and the reference
 *            lines follow as 1 .. n; with_self = 0: the n reference lines alone
 *   KG(x)    max(E_Z[max_i (mu_i + b_i Z)] - max_i mu_i, 0), Z standard normal, Phi from libm's erf
 *            (a NaN -- a NaN candidate coordinate, say -- stays a NaN: it is returned as such and never wins the arg-max)
 * The evaluation order is part of the definition.  mu* = max_i mu_i is taken off every mu_i first.  Line i owns z in (lo_i, hi_i),
 * c_ij = (mu_j - mu_i) / (b_i - b_j), lo_i = max of c_ij over {j : b_j < b_i}, hi_i = min of c_ij over {j : b_j > b_i}; a line j with
 * b_j = b_i puts line i out when mu_j > mu_i, or when mu_j = mu_i and j < i.  Both differences of c_ij are formed as written, so
 * c_ij and c_ji are the same bits and two nearly identical lines split the axis at one point.  A line with lo_i < hi_i contributes
 * (mu_i - mu*) (Phi(hi_i) - Phi(lo_i)) + b_i (phi(lo_i) - phi(hi_i)); a wavefront sums the contributions of one candidate, lane l
 * those of the lines l, l + 64, .. in ascending order, then over the lanes in a fixed butterfly.
 * The means are dot products over the k* rows (lane l of a wavefront over the rows l, l + 64, .., then the same butterfly), NOT
 * ibo_posterior_batch's launches, whose route depends on the batch size: they agree with them to rounding, not bit for bit.
 * A candidate's KG bits depend on the model, the reference set, with_self and clamp_lo and on nothing else: not on M, on its place in
 * the array, on the chunking, nor on the entry (sweep, host batch, DIRECT) it came through.
 * Cost: N^2 (nref + M) flops for V = W K* and 2 N nref M for the cross-covariance on the fp64 MFMA pipe; (nref + with_self)^2 M pair
 * steps with one fp64 division each on the vector ALU -- the larger part from a few hundred reference points on.
 * Device scratch, from the pool and returned before the call returns: the reference state (2 np Npad doubles while it is built,
 * np Npad after; np = nref rounded up to 64) and per chunk of candidates K* and V^T (mc Npad doubles each) and the slopes (mc np),
 * each at most 256 MiB or 256 candidates where that alone is more, mc <= 65280 (ibo_set_option("kg_chunk", m) sets mc, rounded up to 256).
 * IBO_ERR_NO_DEVICE without a device (checked first); IBO_ERR_ARG for a NULL gp, reference set or candidate array, nref outside
 * [1, IBO_KG_MAX_REF], M < 1, every output NULL or a non-finite reference coordinate; IBO_ERR_STATE before a fit.
 * There are no exclusion balls and no gradients with respect to x.
 */
#define IBO_KG_MAX_REF 1024

/* M candidates on the device (cand_dev, M x D): kg_dev (device, M, optional) receives the values; best_val / best_idx the maximum
 * and the first index that attains it, index_base added (-1 if no value is a number). */
int ibo_kg_sweep(ibo_gp_t *gp, int nref, const double *ref_host, int64_t M, const double *cand_dev, int with_self,
                 double clamp_lo, int64_t index_base, double *kg_dev, double *best_val, int64_t *best_idx);

/* M host points: kg_host (M) and, all optional, what the values were made of: mu_ref_host (nref), mu_host and s2_host (M, s2
 * clipped), b_host (M x nref row-major, b_host[x][a] = b_a(q_x)). */
int ibo_kg_batch(ibo_gp_t *gp, int nref, const double *ref_host, int64_t M, const double *Q_host, int with_self,
                 double clamp_lo, double *kg_host, double *mu_ref_host, double *mu_host, double *s2_host, double *b_host);

/* ibo_direct_max on KG: the same DIRECT, options and batched schedule; the reference state is built once and stays on the device
 * across the batches.  opt = the maximum, optx[D] its location, nsamples optional (not all three NULL).  IBO_ERR_ARG also for NULL
 * bounds or D other than the model's. */
int ibo_kg_direct_max(ibo_gp_t *gp, int nref, const double *ref_host, int D, const double *lb, const double *ub,
                      int with_self, double clamp_lo, int maxiter, int maxtime, int maxsample, int compat,
                      double *opt, double *optx, int64_t *nsamples);

/* With ibo_set_option("kg_timing", 1) every ibo_kg_* call of this thread waits after each chunk and adds the device time of its
 * stages (HIP events) to ms[IBO_KG_STAGES]: the reference state, K*, V^T = K* W^T, the row kernel, the cross-covariance, the
 * expected maximum.  reset != 0 clears the sums after they are read; ms may be NULL.  A diagnostic: the option is process-wide
 * (every thread's ibo_kg_* calls wait after each chunk while it is set), the sums are per thread. */
#define IBO_KG_STAGES 6
int ibo_kg_stage_ms(double *ms, int reset);

/* ---------------------------------------------------------------- parallel expected improvement (Monte-Carlo q-EI) */
/*
 * The expected improvement of a candidate x evaluated TOGETHER with a pending set P = {p_1 .. p_p} (pend_host, npend x D row-major, host
 * memory, 0 <= npend <= IBO_QEI_MAX_PENDING; NULL allowed when npend = 0) over the joint predictive distribution,
 *   qEI(x | P) = E[max(max(y(x), max_j y(p_j)) - t, 0)],   t = ymax + xi (ymax NaN: the model's largest observation, as ibo_acq_batch),
 * estimated with the CALLER's base samples Z_host (nsamp x (npend + 1) row-major, 1 <= nsamp <= IBO_QEI_MAX_SAMPLES; column j belongs to
 * pending point j, the last column to the candidate).  The library draws nothing.
 * Conventions of ibo_posterior_cov with with_noise = 1: k and k* with the handle's k* signal variance, v = W k*.  Means are the row
 * kernel's of the knowledge gradient, m + k*.aY - m k*.a1 as dot products over the k* rows (NOT ibo_posterior_batch's launches).
 * The pending state, once per call:
 *   mu_P     the means at the pending points
 *   S_PP     S_ab = k(p_a, p_b) - v_a.v_b (the entry a > b as the device forms it, mirrored), S_aa = ((1 + noise) - |v_a|^2) + jitter
 *   L_P      the Cholesky factor of S_PP, on the host in plain double, row by row: L_ji = (S_ji - sum_{k<i} L_jk L_ik) / L_ii for i < j, then
 *            L_jj = sqrt(S_jj - sum_{k<j} L_jk^2); every sum starts from the S entry and takes its terms in ascending k, each by one fused
 *            multiply-add acc = fma(-a, b, acc).  A pivot that is not a positive finite number returns IBO_ERR_NOT_PD with the 1-based
 *            pivot in *info (0 otherwise; info may be NULL).
 *   g_s      max_j y_sj,  y_sj = mu_P,j + sum_{i<=j} L_ji z_si taken as y = mu_P,j; y = fma(L_ji, z_si, y) in ascending i; -inf when npend = 0
 *   base     (1/S) sum_s max(g_s - t, 0), the value of the pending set alone (0 when npend = 0), summed in the order given below
 * Per candidate x:
 *   mu_x, s2_x = clip(1 + noise - |v_x|^2, clamp_lo, 10)              (the knowledge gradient's row kernel)
 *   c_j      k(p_j, x) - v_pj.v_x: the tile product of the knowledge gradient's cross kernel WITHOUT its division by sigma_x
 *   l        L_P^-1 c by forward substitution: l_j = (c_j - sum_{i<j} L_ji l_i) / L_jj, acc = c_j; acc = fma(-L_ji, l_i, acc) in ascending i
 *   d        r = s2_x; r = fma(-l_j, l_j, r) in ascending j;  d = sqrt(r) if r > 0, else 0
 *   f_s      f = mu_x; f = fma(l_j, z_sj, f) in ascending j; f = fma(d, z_sp, f)
 *   qEI      (1/S) sum_s max(max(f_s, g_s) - t, 0): the term of sample s is h - t with h = f_s if f_s > g_s, else g_s, and is added only if
 *            it is > 0.  A wavefront sums one candidate: lane l the samples l, l + 64, .. in ascending order, then over the lanes in a fixed
 *            butterfly (offsets 32, 16, .. 1), then one division by S.  base is summed the same way, which is why
 *            qEI(x | P) >= base holds EXACTLY for every candidate: termwise max(f, g) >= g, and every rounding on the way is monotone.
 * (l, d) is the last row of the Cholesky factor of the bordered (p + 1) x (p + 1) joint covariance, applied to the same z; for npend = 0
 * and S -> infinity the value is ibo_acq_batch's EI with libm erf.  The evaluation order above is part of the definition.  A candidate's
 * bits depend on the model, P, Z, t, clamp_lo and jitter and on nothing else: not on M, on its place in the array, on the chunking, nor on
 * the entry (sweep, host batch, DIRECT) it came through.  A NaN candidate coordinate gives a NaN value, which never wins the arg-max.
 * Cost: N^2 (npend + M) flops for V = W K* and 2 N 64 M for the cross-covariance (the pending set fills one 64-wide tile column) on the
 * fp64 MFMA pipe; nsamp (npend + 1) M fused multiply-adds on the vector ALU in the finish.
 * Device scratch, from the pool and returned before the call returns: the pending state (3 x 64 Npad doubles while it is built, 64 Npad
 * after, and (npend + 2) nsamp' doubles of samples, nsamp' = nsamp rounded up to 256) and per chunk of candidates K* and V^T (mc Npad
 * doubles each) and the covariances (64 mc), each at most 256 MiB or 256 candidates where that alone is more, mc <= 65280
 * (ibo_set_option("qei_chunk", m) sets mc, rounded up to 256).
 * IBO_ERR_NO_DEVICE without a device (checked first); IBO_ERR_ARG for a NULL gp, Z_host, candidate array (or pend_host with npend > 0),
 * npend or nsamp outside their limits, M < 1, every output NULL, a non-finite pending coordinate, base sample, xi or jitter, jitter < 0;
 * IBO_ERR_STATE before a fit (checked before the values are looked at).  There are no exclusion balls and no gradients with respect to x.
 */
#define IBO_QEI_MAX_PENDING 15
#define IBO_QEI_MAX_SAMPLES 4096

/* M candidates on the device (cand_dev, M x D): qei_dev (device, M, optional) receives the values; base (optional) the pending set's own
 * value; best_val / best_idx the maximum and the first index that attains it, index_base added (-inf and -1 if no value is a number). */
int ibo_qei_sweep(ibo_gp_t *gp, int npend, const double *pend_host, int nsamp, const double *Z_host, double ymax, double xi,
                  double clamp_lo, double jitter, int64_t M, const double *cand_dev, int64_t index_base, double *qei_dev,
                  double *base, double *best_val, int64_t *best_idx, int *info);

/* M host points: qei_host (M) and, all optional (but not all NULL), what the values were made of: base, mu_pend_host (npend), S_pend_host
 * (npend x npend row-major, jitter included), mu_host and s2_host (M, s2 clipped), c_host (M x npend row-major, c_host[x][j] = c_j(q_x)). */
int ibo_qei_batch(ibo_gp_t *gp, int npend, const double *pend_host, int nsamp, const double *Z_host, double ymax, double xi,
                  double clamp_lo, double jitter, int64_t M, const double *Q_host, double *qei_host, double *base,
                  double *mu_pend_host, double *S_pend_host, double *mu_host, double *s2_host, double *c_host, int *info);

/* ibo_direct_max on qEI(. | P): the same DIRECT, options and batched schedule; the pending state and the samples are built once and stay
 * on the device across the batches.  opt = the maximum, optx[D] its location, nsamples optional (not all three NULL).  IBO_ERR_ARG also
 * for NULL bounds or D other than the model's. */
int ibo_qei_direct_max(ibo_gp_t *gp, int npend, const double *pend_host, int nsamp, const double *Z_host, double ymax, double xi,
                       double clamp_lo, double jitter, int D, const double *lb, const double *ub, int maxiter, int maxtime,
                       int maxsample, int compat, double *opt, double *optx, int64_t *nsamples, int *info);

/* ibo_kg_stage_ms for the ibo_qei_* entries, under ibo_set_option("qei_timing", 1): the pending state (its device part), K*,
 * V^T = K* W^T, the row kernel, the cross-covariance, the Monte-Carlo finish. */
#define IBO_QEI_STAGES 6
int ibo_qei_stage_ms(double *ms, int reset);

/* ---------------------------------------------------------------- pathwise posterior draws */
/*
 * A posterior draw as a FUNCTION (Matheron's rule with a random-Fourier-feature prior; Wilson et al. 2020), S of them in one object:
 *   path_s(x) = m(x) + sum_j phi_j(x) w_sj + sum_i k(x, X_i) c_si - m(x) sum_i k(x, X_i) a1_i        (the last term only with a mean prior)
 *   phi_j(x)  = sqrt(2 sf2 / F) cos(omega_j . x + b_j),   c_s = aY - A^-1 (Phi(X) w_s + eps_s),   A^-1 = W^T W with the handle's W
 * so that path_s = mu + g_s with mu the posterior mean of ibo_posterior_batch (m + k*.aY - m k*.a1) and
 * g_s(x) = phi(x).w_s - k*(x)^T A^-1 (Phi(X) w_s + eps_s).  k and k* carry the handle's k* signal variance sf2 as it is when the object
 * is created.  For a plainly fitted model (A = R = K(X, X; sf2) with 1 + noise on the diagonal), w_s ~ N(0, I_F),
 * eps_s ~ N(0, (1 + noise - sf2) I_N) and omega drawn from the kernel's spectral density, g_s is a draw of the latent posterior:
 * Cov g = k(a, b) - v_a.v_b (ibo_posterior_cov's Sigma off the diagonal, sf2 - |v_a|^2 on it) up to the feature error, which falls as
 * 1 / sqrt(F).  The arrays are the CALLER's: omega_host (F x D), phase_host (F, best reduced into [0, 2 pi)), w_host (S x F),
 * eps_host (S x N); nothing here judges them (ibo_amd.acquisition.pathwise.spectralDraws makes them).
 * The evaluation order is part of the definition: per (candidate, path) ONE accumulator takes the F feature terms in ascending j, then
 * the N kernel terms in ascending i, in k-steps of four on v_mfma_f64_16x16x4_f64 (zero terms pad F and N to multiples of 32); the
 * mean prior comes last, as m + acc - m acc1.  omega_j . x + b_j is formed in double-double and reduced by pi / 2 in fixed cost
 * (accurate to 2e-16 for |omega . x + b| < 2^30); k(x, X_i) by differences.  A value's bits depend on the object and the candidate's
 * coordinates and on nothing else: not on M, the candidate's place, the chunking, nor the entry (sweep, host batch, DIRECT).
 * A NaN coordinate gives NaN in every path of that candidate, and NaN never wins.
 * The object is a self-contained SNAPSHOT on the device (rows, kernel parameters, prior arrays, draws, coefficients, its own stream):
 * it stays valid after ibo_gp_extend / ibo_gp_remove / a refit / ibo_gp_destroy of the model -- a draw of the posterior as it was.
 * One object belongs to one thread at a time.
 * Cost: creation N^2 S + 2 N F S; evaluation 2 (Fp + Np32) Sp flops per candidate on the fp64 MFMA pipe plus about 10 D + 45 vector
 * instructions per (candidate, feature) and 3 D + 40 per (candidate, model row), generated once per tile of 64 (63 with a mean prior)
 * paths.  Device memory: (Fp + Np32) x Sp doubles of coefficients (Fp, Np32: F, N rounded up to 32; Sp: 64 per tile of paths).
 * Gradients (ibo_paths_grad_batch): d path_s / dx_d = sum_j -amp sin(omega_j . x + b_j) omega_jd w_sj + sum_i h_i w_d (x_d - X_id) c_si
 * (h_i as ibo_acq_grad_batch's: -k, -3 sf2 e^-r, -(5/3) sf2 (1 + r) e^-r; finite at r = 0), with a mean prior dm_d (1 - k*.a1) + g_sd -
 * m d(k*.a1)/dx_d.  The derivative of the generated piece is generated the same way and contracted with the same coefficients, one
 * accumulator per (point, path, d) in the values' k order: a gradient's bits depend on the object and the point alone, not on M, the
 * point's place, the pieces a call is cut into, nor on path_of.  A NaN coordinate gives NaN gradients for that point only.  Cost per
 * point: the factor (sine or h_i) once per k, then per dimension one multiplication per k and the values' 2 (Fp + Np32) Sp flops.
 * Not provided: exclusion balls, preference / augmented models (A - K is not diagonal there), the RCCL
 * exchange.
 * IBO_ERR_NO_DEVICE without a device (checked first); IBO_ERR_ARG for NULLs, sizes outside the limits, M < 1, every output NULL,
 * `path` out of range or D other than the object's; IBO_ERR_STATE for an unfitted handle (or one fitted from libego's inverse).
 */
typedef struct ibo_paths ibo_paths_t;
#define IBO_PATHS_MAX_PATHS    256
#define IBO_PATHS_MAX_FEATURES 16384
int ibo_paths_create(ibo_gp_t *gp, int nfeat, const double *omega_host /* F x D */, const double *phase_host /* F */,
                     int npaths, const double *w_host /* S x F */, const double *eps_host /* S x N */, ibo_paths_t **out);
int ibo_paths_destroy(ibo_paths_t *p);
/* any of the outputs may be NULL */
int ibo_paths_info(ibo_paths_t *p, int *npaths, int *nfeat, int *N, int *D, int *device);
/* the coefficients as the device holds them, S x (F + N): w_s, then c_s */
int ibo_paths_coef(ibo_paths_t *p, double *coef_host);
/* M candidates on the device (cand_dev, M x D): values_dev (device, S x M path-major, optional) receives the values; per path
 * best_val / best_idx (host, S each, optional) the maximum and the first index that attains it, index_base added -- or -inf and -1
 * (no base added) when no value of that path is a number. */
int ibo_paths_sweep(ibo_paths_t *p, int64_t M, const double *cand_dev, int64_t index_base,
                    double *values_dev, double *best_val, int64_t *best_idx);
/* M host points: values_host (S x M path-major) */
int ibo_paths_batch(ibo_paths_t *p, int64_t M, const double *Q_host, double *values_host);
/* M host points: values (optional) and gradients with respect to x.  path_of optional (M ints, each in [0, S)):
 *   path_of == NULL: values_host S x M path-major,     grads_host S x M x D
 *   path_of != NULL: values_host M (path path_of[i] at point i), grads_host M x D
 * The values are ibo_paths_batch's, bit for bit.  IBO_ERR_ARG for M < 1, a NULL Q_host or grads_host, or a path index out of range. */
int ibo_paths_grad_batch(ibo_paths_t *p, int64_t M, const double *Q_host, const int *path_of, double *values_host, double *grads_host);
/* ibo_direct_max on ONE path: the same DIRECT, options and batched schedule; every batch evaluated as ibo_paths_batch evaluates that
 * path.  opt = the maximum, optx[D] its location, nsamples optional (not all three NULL). */
int ibo_paths_direct_max(ibo_paths_t *p, int path, int D, const double *lb, const double *ub, int maxiter, int maxtime,
                         int maxsample, int compat, double *opt, double *optx, int64_t *nsamples);

/* ---------------------------------------------------------------- gradient observations */
/*
 * A GP observed with gradients: at each of N points the value Y_i AND the D partial derivatives G_i (what the reference's constructor
 * advertises as G= and never finished: ego/gaussianprocess/__init__.py:198-206 calls a covWithGradients that does not exist).  The model
 * has P = N (D + 1) rows in POINT-MAJOR order, as the reference interleaves them: row i (D + 1) is the value at x_i, rows i (D + 1) + d
 * (d = 1 .. D) are df/dx_d at x_i.  With u = x - x' (x the row's point, x' the column's) the (D + 1) x (D + 1) block of a pair is
 *     [ k           dk/dx'_e        ]          dk/dx'_e = -dk/dx_e
 *     [ dk/dx_d     d2k/dx_d dx'_e  ]
 *   SE (w_d = 1/theta_d^2)          k = sf2 exp(-sum w_d u_d^2 / 2);  dk/dx_d = -w_d u_d k;  d2k = (w_d delta_de - w_d u_d w_e u_e) k
 *   Matern-3/2 (z = sqrt 3 r/theta) k = sf2 (1 + z) e^-z;  dk/dx_d = -sf2 c u_d e^-z, c = 3/theta^2;  d2k = sf2 c e^-z (delta_de - sqrt 3 u_d u_e / (theta r)),
 *                                   the second term 0 at r = 0
 *   Matern-5/2 (s = sqrt 5 r/theta) k = sf2 e^-s (1 + s + s^2/3);  dk/dx_d = -sf2 c (1 + s) e^-s u_d, c = 5/(3 theta^2);
 *                                   d2k = sf2 c e^-s ((1 + s) delta_de - (5/theta^2) u_d u_e)
 * Diagonal: a value row keeps ibo_gp_fit's rule, 1 + noise; derivative row d gets d2k/dx_d dx'_d (0) + gnoise[d - 1].
 * Posterior at q: k*(q) has the entries k(q, x_i) and dk(q, x_i)/dx_i,d; mu = k*^T A^-1 [Y; G] (interleaved), s2 = (1 + noise) - |W k*|^2
 * clipped to [clamp_lo, 10], W = L^-1; EI / PI / UCB from (mu, s2) by the formula of every sweep, in both erf flavours.  ymax NaN: max(Y),
 * over the values only.  ONE signal variance throughout (no ibo_gp_set_kstar_sf2: libego has no gradient models); no mean prior.
 * The handle is its own type: no ibo_gp_* / ibo_acq_* entry accepts it.  One handle belongs to one thread at a time.
 * The means are dot products over the k* rows (the row kernel of the knowledge gradient: lane l over the rows l, l + 64, .., then a fixed
 * butterfly).  A candidate's bits depend on the model and its coordinates and on nothing else: not on M, its place, the chunking
 * (ibo_set_option("ggp_chunk", m): candidates per chunk, rounded up to 256; 0: by bytes, 256 MiB of K*), nor on the entry.
 * Cost: the fit is one P-row factorisation on the route of a plain fit of P rows; a candidate costs P^2 flops for V^T = K* W^T on the fp64
 * MFMA pipe plus one exp per data point.  Device scratch per chunk: K* and V^T, mc Ppad doubles each, returned before the call returns.
 * Errors: IBO_ERR_NO_DEVICE without a device (checked first); IBO_ERR_ARG for NULLs, M < 1, an unknown acq / erf_mode, every output NULL;
 * IBO_ERR_STATE before a successful fit.
 */
typedef struct ibo_ggp ibo_ggp_t;
#define IBO_GGP_MAX_ROWS 8192        /* P = N (D + 1) at most: the largest frame this unit's scratch (one 512 MiB frame for ibo_ggp_get_R) and
                                      * all three fit routes -- pipelined, super-panels from 4096 rows, two-level from 6656 -- are sized for */
int ibo_ggp_create(int device, ibo_ggp_t **out);
int ibo_ggp_destroy(ibo_ggp_t *h);
/* any of the outputs may be NULL; P = N (D + 1); max_y: the largest observed value */
int ibo_ggp_info(ibo_ggp_t *h, int *N, int *D, int *P, int *device, double *max_y);
/* X: N x D, Y: N, G: N x D (G[i][d] = df/dx_d at x_i), gnoise: D, all host.  hyper / nhyper / sf2 / noise as ibo_gp_fit.  IBO_ERR_NOT_PD
 * with the 1-based failing pivot in *info (optional), as ibo_gp_fit: the handle is then UNFITTED.  IBO_ERR_ARG for N (D + 1) >
 * IBO_GGP_MAX_ROWS, N < 1, D outside 1 .. 64. */
int ibo_ggp_fit(ibo_ggp_t *h, int ktype, int N, int D, const double *X_host, const double *Y_host, const double *G_host /* N x D */,
                const double *hyper_host, int nhyper, double sf2, double noise, const double *gnoise_host /* D */, int *info);
/* P x P row-major, point-major rows.  R is A as factored (assembled again by the fit's kernel: the same bits); L its Cholesky factor */
int ibo_ggp_get_R(ibo_ggp_t *h, double *R_host);
int ibo_ggp_get_L(ibo_ggp_t *h, double *L_host);
/* ibo_acq_batch's arguments: host points in (Q_host: M x D), any of mu / s2 / acq out (not all NULL) */
int ibo_ggp_acq_batch(ibo_ggp_t *h, int64_t M, const double *Q_host, int acq, double parm, int erf_mode,
                      double clamp_lo, double ymax, double *mu_host, double *s2_host, double *acq_host);
/* Device candidates (cand_dev: M x D); optional DEVICE outputs (M doubles each); best_val / best_idx (host, optional) under the arg-max rule
 * of ibo_acq_sweep: the largest value wins, the lowest index wins ties, NaN never wins, index_base is added; -inf and -1 when no value is
 * a number.  No exclusion balls, no kept state, no exchange. */
int ibo_ggp_acq_sweep(ibo_ggp_t *h, int64_t M, const double *cand_dev, int acq, double parm, int erf_mode,
                      double clamp_lo, double ymax, int64_t index_base,
                      double *mu_dev, double *s2_dev, double *acq_dev, double *best_val, int64_t *best_idx);
/* ibo_direct_max on the gradient model: the same DIRECT, options and batched schedule, every batch evaluated as ibo_ggp_acq_batch does
 * (ymax = max(Y)).  IBO_ERR_ARG also for IBO_ACQ_NONE, NULL bounds or D other than the model's. */
int ibo_ggp_direct_max(ibo_ggp_t *h, int D, const double *lb, const double *ub, int acq, double parm, int erf_mode,
                       double clamp_lo, int maxiter, int maxtime, int maxsample, int compat,
                       double *opt, double *optx, int64_t *nsamples);
/* ibo_kg_stage_ms for the ibo_ggp_* entries, under ibo_set_option("ggp_timing", 1): [0] the assembly of A, [1] K*, [2] V^T = K* W^T,
 * [3] the row kernel, [4] unused (0), [5] the acquisition, [6] factor-and-invert, [7] the alpha vectors. */
#define IBO_GGP_STAGES 8
int ibo_ggp_stage_ms(double *ms, int reset);
/*
 * The negative log marginal likelihood of the gradient-observation model and its gradient for ONE theta, stateless like ibo_nlml_grad (and on
 * the same per-device workspace, under the same mutex; X and the interleaved targets stay resident while their content is unchanged, in
 * buffers of their own: ibo_nlml_grad / ibo_loo_grad called before and after return the same bits).
 *   t = [Y; G] interleaved point-major, P = N (D + 1);  A_nl = C + diag(noise, gnoise_1 .. gnoise_D) per point, C the derivative covariance
 *   of the blocks above with ITS OWN diagonal: sf2 on a value row (ibo_nlml_grad's convention, covMatrix + noise I -- ibo_ggp_fit puts
 *   1 + noise there whatever sf2 is; for sf2 = 1 A_nl is ibo_ggp_fit's matrix bit for bit), g1(0) w_d on derivative row d.
 *   NL = t^T A^-1 t / 2 + sum_i log L_ii + (P / 2) log 2 pi;   dNL/dlog theta_h = sum_ab (A^-1 - alpha alpha^T)_ab (dA/dlog theta_h)_ab / 2,
 *   the exact derivative of NL.
 * modes / dims are numbered as ibo_nlml_grad's -- 0: the SE-ARD length scale of dimension dims[h]; 1, 3, 4: the one length scale of an
 * SE-iso, Matern-3/2, Matern-5/2 kernel; 2: the signal magnitude (dA = 2 C, diagonal included) -- but every mode here is the derivative of A
 * itself.  Modes 3 and 4 are NOT the reference's Kernel.derivative matrices that ibo_nlml_grad reproduces (quirks of value-only kernels,
 * an unscaled r in mode 3): with z = sum_d w_d u_d^2, t_d = w_d u_d, d = d/dlog theta,
 *   mode 0     dz = -2 w_h u_h^2, dt_d = -2 t_d [d = h], dw_d = -2 w_d [d = h], dk = -(g1/2) dz, dg1 = -(g2/2) dz, dg2 = -(k/2) dz
 *   1, 3, 4    dz = -2 z, dt_d = -2 t_d, dw_d = -2 w_d, dk = g1 z, dg1 = g2 z, dg2 (always times t_d t_e, 0 at r = 0) = k z (SE),
 *              9 sf2 e^-r (1 + r) / r (Matern-3/2), 25/3 sf2 e^-r r (Matern-5/2)
 *   d(value, d/dx'_e) = dg1 t_e + g1 dt_e, its mirror image the negative; d(d, e) = (dg1 w_d + g1 dw_d) [d = e] - dg2 t_d t_e - g2 (dt_d t_e + t_d dt_e)
 * grad_noise_host (1 + D, optional): dNL/dlog noise = noise sum_{value rows} d / 2 and dNL/dlog gnoise_e = gnoise_e sum_{rows of d/dx_e} d / 2,
 * d = diag(A^-1) - alpha o alpha.  grad_host (ngrad) may be NULL: value only, when grad_noise_host is NULL too nothing but the factorisation runs
 * and *nlml_host has the same bits.
 * Launches: the assembly of A_nl into the frame of the fit's route for P rows, factor-and-invert, alpha, the two scalars, K^-1 = W^T W as
 * ibo_nlml_grad forms it (64 x 64 tiles below 1792 rows, the packed-operand product from there), one contraction kernel -- a workgroup per
 * tile of 16 x 16 point pairs, O(D^2) per pair once and O(1) per derivative -- and a fixed-order sum of the per-tile partial sums; one pinned
 * read-back behind one synchronisation.  No atomics: two calls give the same bits, and a component has the same bits alone, in a full list
 * and in a permuted one.
 * Limits: N (D + 1) <= IBO_GGP_MAX_ROWS, D in 1 .. 64, 1 <= ngrad <= 65 when grad_host is given.
 * Errors: IBO_ERR_NO_DEVICE first; IBO_ERR_ARG for NULLs, sizes and a bad derivative spec; IBO_ERR_NOT_PD leaves the outputs untouched.
 */
int ibo_ggp_nlml_grad(int device, int ktype, int N, int D, const double *X_host, const double *Y_host, const double *G_host,
                      const double *hyper_host, int nhyper, double sf2, double noise, const double *gnoise_host /* D */,
                      int ngrad, const int *modes, const int *dims,
                      double *nlml_host, double *grad_host /* ngrad, or NULL: value only */, double *grad_noise_host /* 1 + D, or NULL */);
/* under ibo_set_option("ggp_timing", 1), accumulated per thread: [0] the assembly of A_nl, [1] factor-and-invert with alpha and the two
 * scalars, [2] K^-1 = W^T W, [3] the contraction and its sum. */
#define IBO_GGP_GRAD_STAGES 4
int ibo_ggp_grad_stage_ms(double *ms, int reset);

/* ---------------------------------------------------------------- sparse (inducing-point) GP */
/*
 * A GP on m inducing points Z that stands for N >> m noisy observations (DTC / FITC): the fit is O(N m^2), and after it the data are
 * gone -- the model is m rows whatever N was.  k carries sf2; every diagonal counts k(x, x) as 1 (ibo_gp_fit's rule); noise = sigma^2.
 *   K~uu = K(Z, Z) with diagonal 1 + jitter = L_u L_u^T, W_u = L_u^-1;  q_i = |W_u k_u(x_i)|^2
 *   lambda_i = noise + max(1 - q_i, 0) (IBO_SGP_FITC) or noise (IBO_SGP_DTC)
 *   F[a][i] = k(z_a, x_i) / sqrt(lambda_i), y~_i = y_i / sqrt(lambda_i);  G = F F^T, b = F y~, yy = y~.y~, ll = sum log lambda_i,
 *   tt = sum max(1 - q_i, 0);  A = K~uu + G = L_A L_A^T, W_A = L_A^-1, alpha = W_A^T W_A b
 *   mu(x) = k_u(x)^T alpha;  s2(x) = noise + (1 - |W_u k_u(x)|^2) + |W_A k_u(x)|^2, summed in that order and THEN clipped to [clamp_lo, 10]
 *   (it includes the noise, as the plain model's does);  EI / PI / UCB from (mu, s2) by the formula of every sweep, both erf flavours;
 *   ymax NaN: the largest target among all data seen.
 *   NLML = (ll + 2 sum log L_A,ii - 2 sum log L_u,ii + yy - |W_A b|^2 + N log 2 pi) / 2;  IBO_SGP_NLML_VFE (a DTC model only): + tt / (2 noise),
 *   Titsias' bound.  Values only.
 * The handle is its own type: no ibo_gp_* / ibo_acq_* entry accepts it.  It wraps two m-row frames on the points Z -- U (a plain fit with
 * noise = jitter) and A (the factorisation of a matrix it is handed, noise field 0) -- and keeps G+, the (mp + 64)^2 lower tiles of
 * [F; y~] [F; y~]^T (mp: m rounded up to 64).  Observations travel in chunks through pinned staging and are not kept: per chunk the U
 * frame's plain sweep (the q_i), the generation of Ft and G+ += Ft Ft^T on the fp64 MFMA unit, the accumulators loaded from G+ and
 * continued in ascending observation order.  So the bits of G, b and yy do not depend on the chunking (ibo_set_option("sgp_chunk", n):
 * observations -- and candidates -- per chunk, rounded up to 256; 0: by bytes, 256 MiB of Ft): exactly for DTC; for FITC among chunks of one
 * size class of the plain sweep that supplies q_i (up to 4096 rows and beyond, see "mes_chunk").  ll and tt are added per 256 observations
 * in a fixed order.  ibo_sgp_add accumulates into the kept sums and refactors A: O(n m^2 + m^3).
 * Candidates: per chunk the two frames' plain sweeps into scratch, then one streaming kernel; host batches and DIRECT are uploaded and take
 * the same route, so a candidate's value is the same bits from batch, sweep and DIRECT within a size class (the statement of ibo_mes_*).
 * Limits: 1 <= m <= IBO_SGP_MAX_M, D <= 64, N >= 1 (N < m is allowed).
 * Errors: IBO_ERR_NO_DEVICE first; IBO_ERR_ARG for NULLs, sizes, non-finite X / Y / Z, noise <= 0, jitter < 0, an unknown method / kind /
 * acq / erf_mode, every output NULL; IBO_ERR_NOT_PD with the 1-based pivot in *info and the matrix that failed (K~uu or A) in the message:
 * the handle is then UNFITTED (also after a failed ibo_sgp_add); IBO_ERR_STATE before a successful fit.
 */
typedef struct ibo_sgp ibo_sgp_t;
#define IBO_SGP_MAX_M 8192
#define IBO_SGP_FITC 0
#define IBO_SGP_DTC  1
#define IBO_SGP_NLML_MODEL 0         /* the marginal likelihood of the model as fitted (FITC or DTC) */
#define IBO_SGP_NLML_VFE   1         /* the DTC value + tt / (2 noise); IBO_ERR_ARG on a FITC model  */
int ibo_sgp_create(int device, ibo_sgp_t **out);
int ibo_sgp_destroy(ibo_sgp_t *h);
/* Z: m x D, X: N x D, Y: N, all host; hyper / nhyper / sf2 as ibo_gp_fit.  lambda_host (optional): receives the N lambda_i. */
int ibo_sgp_fit(ibo_sgp_t *h, int ktype, int D, const double *hyper_host, int nhyper, double sf2, double noise, double jitter, int method,
                int m, const double *Z_host, int64_t N, const double *X_host, const double *Y_host, double *lambda_host, int *info);
/* n more observations into the kept sums, then A is factored again.  The model needs no stored data. */
int ibo_sgp_add(ibo_sgp_t *h, int64_t n, const double *X_host, const double *Y_host, double *lambda_host, int *info);
/* ibo_acq_batch's arguments: host points in (Q_host: M x D), any of mu / s2 / acq out (not all NULL) */
int ibo_sgp_acq_batch(ibo_sgp_t *h, int64_t M, const double *Q_host, int acq, double parm, int erf_mode,
                      double clamp_lo, double ymax, double *mu_host, double *s2_host, double *acq_host);
/* ibo_acq_sweep's arguments and arg-max rule: device candidates, optional DEVICE outputs, exclusion balls, index_base; best_val /
 * best_idx on the host (optional): -inf and -1 when nothing is admissible. */
int ibo_sgp_acq_sweep(ibo_sgp_t *h, int64_t M, const double *cand_dev, int acq, double parm, int erf_mode, double clamp_lo, double ymax,
                      int n_excl, const double *excl_host, double excl_radius, int64_t index_base,
                      double *mu_dev, double *s2_dev, double *acq_dev, double *best_val, int64_t *best_idx);
/* ibo_direct_max on the sparse model: the same DIRECT, every batch evaluated as ibo_sgp_acq_batch does (ymax = the largest target).
 * IBO_ERR_ARG also for IBO_ACQ_NONE, NULL bounds or D other than the model's. */
int ibo_sgp_direct_max(ibo_sgp_t *h, int D, const double *lb, const double *ub, int acq, double parm, int erf_mode,
                       double clamp_lo, int maxiter, int maxtime, int maxsample, int compat,
                       double *opt, double *optx, int64_t *nsamples);
int ibo_sgp_nlml(ibo_sgp_t *h, int kind, double *value);
/* What the model is made of, for the tests.  m x m row-major: K~uu, G, A, L_u, L_A; m doubles: b, alpha; one double: yy, ll, tt, N. */
#define IBO_SGP_GET_KUU   0
#define IBO_SGP_GET_G     1
#define IBO_SGP_GET_A     2
#define IBO_SGP_GET_LU    3
#define IBO_SGP_GET_LA    4
#define IBO_SGP_GET_B     5
#define IBO_SGP_GET_ALPHA 6
#define IBO_SGP_GET_YY    7
#define IBO_SGP_GET_LL    8
#define IBO_SGP_GET_TT    9
#define IBO_SGP_GET_N     10
int ibo_sgp_get(ibo_sgp_t *h, int what, double *out_host);
/* under ibo_set_option("sgp_timing", 1), accumulated per thread: [0] the q sweeps of the observations, [1] the generation of Ft, [2] the
 * Gram product, [3] the assembly of A, [4] factor-and-invert with the alpha vectors, [5] the candidates' two sweeps, [6] the finish kernel. */
#define IBO_SGP_STAGES 8
int ibo_sgp_stage_ms(double *ms, int reset);
/*
 * The sparse negative log marginal likelihood and its gradient for ONE theta / noise / Z, stateless like ibo_nlml_grad: a fit (ibo_sgp_fit on a
 * private per-device handle that ibo_trim gives back) and one more pass over the data, O(N m^2) on the fp64 MFMA unit.
 *   kind   IBO_SGP_FITC / IBO_SGP_DTC: the model's own objective (IBO_SGP_NLML_MODEL of that fit);  IBO_SGP_VFE: Titsias' bound
 *          (IBO_SGP_NLML_VFE of a DTC fit).  *value is ibo_sgp_nlml's value for the same arguments, bit for bit.
 *   per observation  mu_i = alpha.k_i, a_i = k_i^T A^-1 k_i, c_i = [1 / lambda_i - ((y_i - mu_i)^2 + a_i) / lambda_i^2] / 2 = dNL/dlambda_i,
 *          e_i = c_i [1 - q_i > 0] (fitc), 0 (dtc), [1 - q_i > 0] / (2 noise) (vfe): the clamp max(1 - q, 0) is differentiated as that indicator,
 *          taken from the device's own q_i
 *   dNL/dK, column i   g_i = (A^-1 k_i + alpha (mu_i - y_i)) / lambda_i - 2 e_i K~uu^-1 k_i          (never stored)
 *   dNL/dK~uu          S = (A^-1 + alpha alpha^T - K~uu^-1) / 2 + K~uu^-1 (K E K^T) K~uu^-1, off the diagonal (the diagonal is the constant 1 + jitter)
 *   with z = sum_d w_d Delta_d^2, rho = dk/dz:
 *   grad_Z[a][d]       2 w_d [sum_i g_ai rho_ai (Z_ad - X_id) + 2 sum_{b != a} S_ab rho_ab (Z_ad - Z_bd)]
 *   grad_hyper[h]      modes / dims as ibo_nlml_grad's: mode 0 (the length scale of dimension dims[h]) -2 w_d [sum_ai g rho Delta_d^2 + sum_{a != b} S rho Delta_d^2];
 *                      modes 1, 3, 4 (one length scale for every dimension) the sum of that over d, with the rho of the kernel's own family;
 *                      mode 2 (the signal magnitude) 2 [sum g_ai k_ai + sum_{a != b} S_ab K~uu,ab].  All with respect to the LOG of the parameter.
 *   grad_lognoise      noise (sum_i c_i - [vfe] tt / (2 noise^2))
 * The data stream in the fit's chunks ("sgp_chunk"); per chunk the two frames' plain sweeps (q_i, mu_i, a_i), a per-observation kernel, the
 * generation of the operands and one fused kernel: 64 x 64 tiles of g from [A^-1 | K~uu^-1] against [k_i / lambda_i | -2 e_i k_i] with the
 * derivative epilogue applied in LDS; the signed Gram matrix K E K^T is accumulated beside it (not for dtc).  No atomics: two calls with the
 * same arguments give the same bits; another chunking may differ within rounding.  A component's bits do not depend on which other outputs
 * are asked for, nor on where it stands in modes / dims.
 * 0 <= ngrad <= 65 (modes / dims may be NULL when 0); grad_hyper (ngrad), grad_lognoise (1), grad_Z (m x D row-major) are optional (NULL).
 * Limits and errors: ibo_sgp_fit's, IBO_ERR_ARG also for an unknown kind or derivative spec.  Every error, IBO_ERR_NOT_PD (pivot in *info)
 * among them, leaves all outputs untouched.
 */
#define IBO_SGP_VFE  2               /* a kind of ibo_sgp_nlml_grad only: ibo_sgp_fit does not take it */
int ibo_sgp_nlml_grad(int device, int ktype, int D, const double *hyper_host, int nhyper, double sf2, double noise, double jitter, int kind,
                      int m, const double *Z_host, int64_t N, const double *X_host, const double *Y_host,
                      int ngrad, const int *modes, const int *dims,
                      double *value, double *grad_hyper, double *grad_lognoise, double *grad_Z, int *info);
/* under ibo_set_option("sgp_timing", 1), accumulated per thread: [0] the fit, [1] the two inverses, [2] the observations' two sweeps, [3] the
 * per-observation kernel and the generation of the operands, [4] the fused contraction, [5] the signed Gram product, [6] S and the K~uu
 * contraction, [7] the sums over the strips. */
#define IBO_SGP_GRAD_STAGES 8
int ibo_sgp_grad_stage_ms(double *ms, int reset);

/* DIRECT minimisation of a HOST callback with the reference's semantics
 * (cpp/direct.cpp:329; what ego.utils.optimize.cdirect wraps), plus the sample
 * counter and the compat switch (bit 0).  Bit 1 of `compat` selects the batched schedule ibo_direct_max runs the GPU
 * objective under -- one evaluation batch per iteration: every potentially-optimal rectangle's probes plus its child
 * centres, guessed before the probe values are known and verified bit for bit afterwards -- with the same
 * (fmin, xmin, nsamples) as the sequential call order.  Host-side only: no GPU is touched. */
int ibo_direct_host(double (*objective)(int, double *), int ndim, const double *lb, const double *ub,
                    int maxiter, int maxtime, int maxsample, int compat,
                    double *fmin, double *xmin, int64_t *nsamples);

/* ---------------------------------------------------------------- marginal likelihood grid */
/*
 * nlml[t] for n_theta hyper-parameter rows (each nhyper doubles):
 * marginalLikelihood(..., computeGradient=False) of
 * ego/gaussianprocess/trainhyper.py:47-75 (K = covMatrix + noise I).
 * A non-positive-definite K yields NAN in that slot (the reference's nlml()
 * wrapper maps the LinAlgError to 100, trainhyper.py:111-114 -- done host side).
 */
int ibo_nlml_grid(int device, int ktype, int N, int D,
                  const double *X_host, const double *Y_host,
                  int n_theta, const double *thetas_host, int nhyper,
                  const double *sf2_host /* n_theta or NULL (=1) */, double noise,
                  double *nlml_host);
/* Device memory is recycled: ibo_nlml_grid and ibo_nlml_grad keep their workspaces (the batch of factor
 * matrices; the N x N buffers of the gradient) between calls, and the buffers of destroyed handles go to a
 * per-device free list (at most 2 GiB; ibo_set_option("pool_limit_mb", n) or env IBO_POOL_LIMIT_MB) for the next handle; buffers of up
 * to half a slab live in the arena (see "arena_mb").  This releases all of it EXCEPT the library's standing reservation on the device: the
 * arena's first slab and four stream / event / staging sets, which the next model would otherwise pay milliseconds to make again. */
int ibo_trim(int device);

/*
 * NLML and its gradient w.r.t. each LOG hyper-parameter for one theta: marginalLikelihood(...,
 * computeGradient=True), ego/gaussianprocess/trainhyper.py:47-75, with dK/dtheta_h as
 * Kernel.derivative(X, h) builds it (ego/gaussianprocess/kernel.py).  modes[h]: 0 SE-ARD length
 * scale of dimension dims[h]; 1 SE-iso length scale; 2 signal magnitude (2K); 3 Matern-3/2 and
 * 4 Matern-5/2 length scale.  grad_host receives ngrad values (1 <= ngrad <= 65; 17 per pass of the gradient kernel).
 * A learning loop calls this dozens of times with one data set and another theta: X and Y stay on the device between calls and go up again
 * only when their CONTENT differs from the last call's (compared on the host; ibo_trim forgets them).
 */
int ibo_nlml_grad(int device, int ktype, int N, int D, const double *X_host, const double *Y_host,
                  const double *hyper_host, int nhyper, double sf2, double noise,
                  int ngrad, const int *modes, const int *dims, double *nlml_host, double *grad_host);

/*
 * The leave-one-out objective of K = covMatrix + noise I for one theta, to be minimised like the NLML (Rasmussen & Williams 5.4.2): with
 * B = K^-1, d_i = B_ii, alpha = B y
 *     nloo = sum_i [-log(d_i) / 2 + alpha_i^2 / (2 d_i)] + N log(2 pi) / 2        mu_host[i] = y_i - alpha_i / d_i        s2_host[i] = 1 / d_i
 * and, when grad_host is given, d nloo / d log theta_h = -sum_i [alpha_i r_i - (1 + alpha_i^2 / d_i) s_i / 2] / d_i for h < ngrad, where
 * T = B dK_h, r = T alpha, s_i = sum_b T_ib B_ib and dK_h = Kernel.derivative(X, h) as modes / dims describe it (ibo_nlml_grad's).  Contract,
 * limits and error codes are ibo_nlml_grad's (up to 23168 rows; IBO_ERR_NOT_PD leaves the outputs untouched), except that grad_host may be
 * NULL (value only: ngrad, modes, dims ignored) and 1 <= ngrad <= 65 otherwise; mu_host / s2_host are optional.  It runs ibo_nlml_grad's
 * sequence up to K^-1 on that entry's workspace and resident X / Y (calls of the two may interleave freely; neither changes the other's
 * bits), then 2 ngrad N^3 flops on the fp64 MFMA unit, four derivatives per pass, dK_h generated on the fly.  Fixed-order sums, no atomics.
 */
int ibo_loo_grad(int device, int ktype, int N, int D, const double *X_host, const double *Y_host,
                 const double *hyper_host, int nhyper, double sf2, double noise,
                 int ngrad, const int *modes, const int *dims,
                 double *nloo_host, double *grad_host /* ngrad, or NULL: value only */,
                 double *mu_host /* N or NULL */, double *s2_host /* N or NULL */);

/* ---------------------------------------------------------------- multi-GPU arg-max exchange (RCCL) */
#define IBO_COMM_ID_BYTES 128
int ibo_comm_get_unique_id(unsigned char id[IBO_COMM_ID_BYTES]);
int ibo_comm_init(int device, int world_size, int rank,
                  const unsigned char id[IBO_COMM_ID_BYTES], ibo_comm_t **out);
int ibo_comm_destroy(ibo_comm_t *comm);
/* ranks in the communicator as RCCL reports them (ncclCommCount) */
int ibo_comm_count(ibo_comm_t *comm, int *nranks);
/*
 * One all-reduce(sum) over a world_size x (3+npayload) slot buffer (value,
 * index, valid flag, payload) in which each rank fills only its own slot (RCCL has no MAXLOC), followed by the same
 * deterministic local reduction on every rank: maximum value, ties to the
 * lowest global index.  payload (npayload doubles, e.g. the winner's
 * coordinates) travels in the same buffer.  All outputs are identical on
 * every rank.
 */
int ibo_comm_argmax(ibo_comm_t *comm, double val, int64_t idx,
                    const double *payload, int npayload,
                    double *best_val, int64_t *best_idx, double *best_payload, int *best_rank);
/*
 * The sharded sweep's step in ONE call: ibo_acq_sweep (incremental != 0: ibo_acq_sweep_incremental) over this rank's block of the
 * candidate array (rows index_base ..), then the exchange above with the winner's D coordinates as payload -- the sweep's (value,
 * index) never visit the host on the way: a kernel writes them and the coordinates into the rank's slot of the all-reduce buffer,
 * ncclAllReduce runs on the sweep's stream, one copy into pinned memory brings back every rank's slot, one synchronisation.
 * local_val / local_idx: this rank's own maximum (index -1 and -inf without an admissible candidate); best_* as ibo_comm_argmax,
 * best_x: D doubles.  Replaces, per round, the candidate loop of ego/acquisition/gallery.py:93-134 cut over the ranks.
 */
int ibo_acq_sweep_exchange(ibo_gp_t *gp, ibo_comm_t *comm, int incremental, int64_t M, const double *cand_dev,
                           int acq, double parm, int erf_mode, double clamp_lo, double ymax,
                           int n_excl, const double *excl_host, double excl_radius, int64_t index_base,
                           double *local_val, int64_t *local_idx,
                           double *best_val, int64_t *best_idx, double *best_x, int *best_rank);
/* in-place ncclAllReduce(sum) of a host buffer: gathers the sharded NLML grid (each rank fills
 * its own theta slots of a zero buffer) */
int ibo_comm_allreduce_sum(ibo_comm_t *comm, double *host_buf, int64_t n);
int ibo_comm_barrier(ibo_comm_t *comm);

/* ---------------------------------------------------------------- (A) legacy libego symbols */
typedef double (*objective_t)(int, double *);

/* cpp/optimizeGP.cpp:262-283.  Returns malloc'd [fmin, xmin[0..ndim)] with
 * fmin = minimum of the NEGATED acquisition; caller frees with free(). NULL on
 * unknown acqfunc (as the reference) or on any failure (message on stderr).
 * The objective is evaluated in the reference's own operation order (cpp/optimizeGP.cpp:57-236: k*, prior mean and the
 * acquisition with the host's libm; aMb's two sequential sums per contraction on the device, products and sums rounded
 * separately), so fmin and xmin equal libego's BIT FOR BIT, whatever the conditioning of invR (csrc/legacy.hip).
 * Differences kept on purpose: kerneltype 3 takes its magnitude from hyperparams[1] (the reference reads hyperparams[ndim],
 * out of bounds for ndim > 1) and prints nothing; a kerneltype outside 0..3 (the reference's switch leaves k* uninitialised) returns NULL.
 * The host half (k*, prior mean, acquisition: O(N D) per sample point) runs on a crew of host threads over the batch's points
 * (IBO_HOST_THREADS, default min(16, the cores the process may use)).  ibo_set_option("legacy_exact", 0): the fast route (invR factored on the
 * device, MFMA sweep kernels; within 1e-6 of libego on well-conditioned data only).  Re-entrant: own handle per call. */
const double *acqmaxGP(int ndim, double *lb, double *ub, double *invR, double *X, double *Y,
                       int nx, int acqfunc, int kerneltype, double *hyperparams,
                       int npbases, double *pbasismeans, double *pbasisbeta, double pbasistheta,
                       double *pbasislowerb, double *pbasiswidth, double parm, double noise,
                       int maxiter, int maxtime, int maxsample);

/* cpp/direct.cpp:329: DIRECT minimisation of a host callback (host-side only;
 * kept so ego.utils.optimize.cdirect keeps working against this library). */
const double *direct(objective_t objective, int ndim, double *lb, double *ub,
                     int maxiter, int maxtime, int maxsample);

/* cpp/helpers.cpp:30-56: sum of log(Phi((x[p[i]] - x[p[i+1]]) / sqrt 2) / sqrt 2) over i = 0, 2, 4, ... < n
 * (terms whose argument of log is exactly 0 are skipped).  Host-side only.  The reference's only caller
 * (ego/gaussianprocess/__init__.py:362-371, off by default) passes flattened (v, u, degree) triples with
 * n = 3 P and so also reads one int past the end for odd P; this entry point keeps the pair-stride loop
 * but never reads p[n]. */
double logCDFs(int nprefinds, int *prefinds, double *x);

#ifdef __cplusplus
}
#endif
#endif /* IBO_ABI_H */

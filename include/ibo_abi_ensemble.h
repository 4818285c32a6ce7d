/* ibo_abi_ensemble.h -- acquisitions integrated over an ensemble of fitted models: the ibo_iacq_* entries of libibo_hip.
 *
 * A header of its own beside ibo_abi.h (which it includes, and which does not include it): the five entries were added within
 * IBO_ABI_VERSION 8 and no symbol of ibo_abi.h changed.  A later version may fold the two headers together.  Plain C99.
 *
 * Hyper-parameter marginalisation (Snoek, Larochelle & Adams 2012): S fitted handles gp[0 .. S-1] -- the same data under S samples of
 * the kernel's hyper-parameters -- and S weights w_s.  With (mu_s, s2_s) what ibo_acq_sweep returns for gp[s] with IBO_ACQ_NONE at the
 * call's clamp_lo, and a(mu, sigma) the call's acquisition (IBO_ACQ_EI / _PI / _UCB with parm, ymax, erf_mode as ibo_acq_sweep
 * defines them; IBO_ACQ_NONE: a = mu):
 *
 *   val  = sum_s w_s a(mu_s, sqrt(s2_s))                                  the weights as given, NOT normalised
 *   mean = (sum_s w_s mu_s) / (sum_s w_s)                                 the mixture's mean
 *   var  = (sum_s w_s (s2_s + (mu_s - mean)^2)) / (sum_s w_s)             the mixture's variance: deviations from the mean in a second
 *                                                                         pass, not E[x^2] - mean^2, which cancels
 *
 * Every sum runs over s ascending, in plain fp64 with products and sums rounded separately (no fused multiply-add), and starts from -0.0.
 * A member with w_s == 0 is neither swept nor read: whatever its posterior holds (NaN included) changes no bit.  So S = 1 with w = 1 is
 * ibo_acq_sweep's acq / best_val / best_idx bit for bit where no launch is padded (see below), and one handle listed twice with
 * weights 1/2, 1/2 is that too.  ymax NaN: gp[0]'s largest observation, for every member.
 *
 * Rules of every entry: 1 <= S <= IBO_IACQ_MAX; every weight finite and >= 0, at least one > 0; every handle non-NULL, fitted, on one
 * device, of one D (a handle may be listed more than once).  IBO_ERR_ARG otherwise (IBO_ERR_STATE for a handle that is not fitted), and
 * for M < 1, a NULL point array, an unknown acq / erf_mode, every output NULL; IBO_ERR_NO_DEVICE without a device.  The checks run
 * in this order: the device, S, the arrays, then per member its handle, its weight and its device, the weights' sum, M, the points, acq,
 * erf_mode, the outputs, every member's fit, every member's D.  A failing call leaves its outputs untouched.
 *
 * Cost: one plain sweep per member with w_s > 0, one after the other on the member's own stream, plus one streaming pass of 16 S bytes
 * per candidate (32 S with var) on gp[0]'s stream; 16 S bytes of pooled scratch per candidate, at most about 1 GiB (more candidates go in
 * chunks of "iacq_chunk", an ibo_set_option key: candidates per chunk rounded up to 256, 0: by bytes).  A short launch is padded to the
 * size class of the call's chunk as ibo_mes_sweep's is (up to 128 candidates run as 160 when the chunk is at most 4096, up to 4096 as
 * 4097 beyond), so a candidate's val / mean / var are the same bits from ibo_iacq_sweep, ibo_iacq_batch, ibo_iacq_grad_batch's
 * val_host and ibo_iacq_direct_max within a size class, whatever "iacq_chunk" is; between the classes they agree to rounding.
 */
#ifndef IBO_ABI_ENSEMBLE_H
#define IBO_ABI_ENSEMBLE_H

#include "ibo_abi.h"

#ifdef __cplusplus
extern "C" {
#endif

#define IBO_IACQ_MAX 32

/* Device candidates (cand_dev: M x D row-major on the handles' device).  val_dev / mean_dev / var_dev: M doubles each on the device, any
 * may be NULL.  The arg-max of val as ibo_acq_sweep's: candidates within excl_radius of one of the n_excl points excl_host (host,
 * n_excl x D) and NaN values never win, the lowest index wins ties, index_base is added to best_idx, and (-inf, -1) when nothing may
 * win.  best_val / best_idx may be NULL; not all five outputs. */
int ibo_iacq_sweep(ibo_gp_t *const *gp, int S, const double *w, int64_t M, const double *cand_dev,
                   int acq, double parm, int erf_mode, double clamp_lo, double ymax,
                   int n_excl, const double *excl_host, double excl_radius, int64_t index_base,
                   double *val_dev, double *mean_dev, double *var_dev, double *best_val, int64_t *best_idx);

/* Host points (Q_host: M x D) through the sweep's own route; val_host / mean_host / var_host: M doubles each, any may be NULL, not all. */
int ibo_iacq_batch(ibo_gp_t *const *gp, int S, const double *w, int64_t M, const double *Q_host,
                   int acq, double parm, int erf_mode, double clamp_lo, double ymax,
                   double *val_host, double *mean_host, double *var_host);

/* ibo_iacq_batch's val (val_host, bit for bit) and its gradient with respect to the query point (dval_host: M x D row-major):
 *   dval = sum_s w_s dacq_s        dacq_s = ibo_acq_grad_batch's dacq of gp[s] (IBO_ACQ_NONE: its dmu), s ascending on the host,
 *                                  members with w_s == 0 left out
 * Either output may be NULL, not both.  Cost: ibo_acq_grad_batch's per member. */
int ibo_iacq_grad_batch(ibo_gp_t *const *gp, int S, const double *w, int64_t M, const double *Q_host,
                        int acq, double parm, int erf_mode, double clamp_lo, double ymax,
                        double *val_host, double *dval_host);

/* ibo_direct_max on val: the same DIRECT, options and batched schedule, every batch of sample points evaluated as ibo_iacq_batch does.
 * opt = the maximum of val, optx[D] its location, nsamples optional (not all three NULL).  IBO_ERR_ARG also for NULL bounds or D other
 * than the models'. */
int ibo_iacq_direct_max(ibo_gp_t *const *gp, int S, const double *w, int D, const double *lb, const double *ub,
                        int acq, double parm, int erf_mode, double clamp_lo, double ymax,
                        int maxiter, int maxtime, int maxsample, int compat, double *opt, double *optx, int64_t *nsamples);

/* With ibo_set_option("iacq_timing", 1) every ibo_iacq_* call of this thread waits after each chunk's sweeps and after its finish kernel
 * and adds their device times (HIP events) to ms[0] (the sweeps, first member's stream to gp[0]'s) and ms[1] (the finish).  reset != 0
 * zeroes the sums after reading; ms may be NULL. */
int ibo_iacq_stage_ms(double *ms, int reset);

#ifdef __cplusplus
}
#endif
#endif /* IBO_ABI_ENSEMBLE_H */

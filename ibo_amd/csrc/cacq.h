// cacq.h -- the constrained acquisition's combine (cacq.hip): the streaming pass over the per-model (mu, s2) a call's sweeps left in
// device scratch, and the host twin of its Gaussian cdf / pdf for host batches and their gradients (abi_cacq.hip: ibo_cacq_*).
#pragma once
#include "ibo_common.h"

// One chunk of candidates.  ms: the scratch, 2 (ncon + 1) arrays `stride` doubles apart -- mu and s2 of the objective, then of each
// constraint model in order (the objective's pair is not read when spec.acq == 3).
struct CacqArgs {
    CacqSpec spec;
    int64_t stride;
    const double *ms;
    FinishTail t;                        // the chunk (t.M <= stride), the exclusion balls, the partials
    double *out_acq, *out_pof, *out_val; // the chunk's part of the optional outputs
};
int launch_cacq_finish(const CacqArgs &a, hipStream_t s);

// ---- host twin of gauss_cdf_pdf_dev (ibo_common.h), both erf flavours
static inline double erf_nr_host(double z)
{
    const double t = 1.0 / (1.0 + 0.5 * fabs(z));
    double p = 0.17087277;
    p = -0.82215223 + t * p;
    p = 1.48851587 + t * p;
    p = -1.13520398 + t * p;
    p = 0.27886807 + t * p;
    p = -0.18628806 + t * p;
    p = 0.09678418 + t * p;
    p = 0.37409196 + t * p;
    p = 1.00002368 + t * p;
    const double ans = 1.0 - t * exp(-z * z - 1.26551223 + t * p);
    return z >= 0.0 ? ans : -ans;
}
static inline void gauss_cdf_pdf_host(int erf_mode, double z, double *cdf, double *pdf)
{
    if (erf_mode == 0) {
        *cdf = 0.5 * (1.0 + erf(z / sqrt(2.0)));
        *pdf = exp(-(z * z / 2.0)) / sqrt(2.0 * M_PI);
    } else {
        *cdf = 0.5 * (1.0 + erf_nr_host(z * 0.707106));
        *pdf = exp(-(z * z / 2.0)) * 0.398942;
    }
}

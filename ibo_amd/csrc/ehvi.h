// ehvi.h -- the strip scan of the two-objective expected hypervolume improvement (ehvi.hip): EHVI per candidate from the (mu, s2) pairs
// the two per-model sweeps left in device scratch, walked over the canonical front (abi_ehvi.hip: ibo_ehvi_*).
#pragma once
#include "ibo_common.h"

#define IBO_EHVI_MAX_PAIRS 1024          // IBO_EHVI_MAX_FRONT of ibo_abi.h: the front in LDS, 16 bytes a point

// One chunk of candidates.  ms: the scratch, four arrays `stride` doubles apart -- mu and s2 of objective 1, then of objective 2.
struct EhviArgs {
    int n;                               // points of the canonical front (<= IBO_EHVI_MAX_PAIRS)
    int erf_mode;
    double r1, r2;                       // the reference point: a_0 = r1, b_{n+1} = r2
    const double *front;                 // device, n interleaved (a_i, b_i), a ascending, b descending
    int64_t stride;                      // (>= t.M: a short launch is padded for the sweeps, see abi_eval.h: class_padded)
    const double *ms;
    FinishTail t;                        // the chunk, the exclusion balls, the partials
    double *out_val;                     // the chunk's part of the optional output
    double *out_sums; int64_t sums_stride;      // the gradient's variant: the chunk's part of six arrays `sums_stride` apart -- G_mu1, G_sigma1, G_mu2, G_sigma2, sigma_1, sigma_2
};
// sums: the variant that also stores out_sums (the same value, bit for bit)
int launch_ehvi_finish(const EhviArgs &a, bool sums, hipStream_t s);

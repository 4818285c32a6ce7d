// marg.h -- the combine of an acquisition integrated over an ensemble of models (marg.hip): the streaming pass over the per-member
// (mu, s2) a call's sweeps left in device scratch (abi_marg.hip: ibo_iacq_*).
#pragma once
#include "ibo_common.h"

// One chunk of candidates.  ms: the scratch, 2 S arrays `stride` doubles apart -- mu and s2 of member 0, then of member 1, .. ; the pair of
// a member whose weight is 0 keeps its places and is never read.  w: the weights as the caller gave them (not normalised), by value.
struct MargArgs {
    int S, acq, erf_mode;
    double ymax, parm;
    int64_t stride;                      // (>= t.M: a short launch is padded for the sweeps, see abi_eval.h: class_padded)
    const double *ms;
    FinishTail t;                        // the chunk, the exclusion balls, the partials
    double *out_val, *out_mean, *out_var;        // the chunk's part of the optional outputs
    double w[IBO_MARG_MAX];
};
int launch_marg_finish(const MargArgs &a, hipStream_t s);

// mes.h -- max-value entropy search (mes.hip): MES per candidate from the (mu, s2) pair one plain sweep left in device scratch, summed over
// the sorted samples of the maximum; and the max-value cdf over a candidate set that the Gumbel fit of such samples starts from
// (abi_mes.hip: ibo_mes_*).
#pragma once
#include "ibo_common.h"

#define IBO_MES_MAX_K 1024               // IBO_MES_MAX_SAMPLES of ibo_abi.h: the samples in LDS, 8 bytes each
#define IBO_MES_MAX_LEV 64               // IBO_MES_MAX_LEVELS of ibo_abi.h

// One chunk of candidates.  ms: the scratch, two arrays `stride` doubles apart -- mu, then s2.
struct MesArgs {
    int K;                               // samples of the maximum (1 .. IBO_MES_MAX_K)
    const double *ystar;                 // device, K doubles, ascending
    double s2_offset, clamp_lo;          // v = max(s2 - s2_offset, clamp_lo), sigma = sqrt(v)
    int64_t stride;                      // (>= t.M: a short launch is padded for the sweep, see abi_eval.h: class_padded)
    const double *ms;
    FinishTail t;                        // the chunk, the exclusion balls, the partials
    double *out_val;                     // the chunk's part of the optional output
    double *out_sums; int64_t sums_stride;      // the gradient's variant: the chunk's part of four arrays `sums_stride` apart -- G_mu, G_sigma, sigma, and 1 where v follows s2 (0 where its floor is active)
};
// sums: the variant that also stores out_sums (the same value, bit for bit)
int launch_mes_finish(const MesArgs &a, bool sums, hipStream_t s);

// One chunk of the max-value cdf: per block of 256 candidates sum_i log Phi((t_k - mu_i) / sigma_i) for each level, max mu_i and max (mu_i + 5 sigma_i)
struct MesCdfArgs {
    int nlev;                            // levels (0 .. IBO_MES_MAX_LEV)
    const double *lev;                   // device, nlev doubles
    double s2_offset, clamp_lo;
    int64_t M, stride;                   // as MesArgs
    const double *ms;
    double *part_sum;                    // the chunk's part of nblk x nlev block sums (block-major)
    double *part_mu, *part_ub;           // the chunk's part of nblk block maxima each
};
int launch_mes_maxcdf(const MesCdfArgs &a, hipStream_t s);
// the block partials of a whole call, added in ascending block order: out[0 .. nlev) the sums, out[nlev] max mu, out[nlev + 1] max (mu + 5 sigma)
int launch_mes_maxcdf_final(const double *part_sum, const double *part_mu, const double *part_ub, int64_t nblk, int nlev, double *out, hipStream_t s);

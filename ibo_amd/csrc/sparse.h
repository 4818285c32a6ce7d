// sparse.h -- the inducing-point GP's own kernels (sparse.hip): a chunk of observations into the scaled cross-covariance Ft, Ft Ft^T
// accumulated into the kept Gram matrix on the fp64 MFMA unit, A = K~uu + G, and the streaming finish of a candidate sweep over the
// model's two m-row frames (abi_sparse.hip: ibo_sgp_*).
#pragma once
#include "ibo_common.h"

#define SGP_ROWS 16              // inducing rows per workgroup of sgp_scaled_kuf_kernel

// One chunk of n observations.  Ft: (mp + 64) rows of ld doubles, contraction-major (the observation index is contiguous):
//   rows a < m     F[a][i] = k(z_a, x_i) / sqrt(lambda_i)
//   row  mp        y_i / sqrt(lambda_i)          (mp: m rounded up to 64 -- the targets start a tile of their own)
//   everything else (pad rows, columns i >= n) zero.
// lambda_i = noise + max(s2u_i - jitter, 0) (fitc: s2u is the U frame's unclipped variance 1 + jitter - q_i) or noise (dtc).
// part: per 256 observations the sums of log lambda_i and of max(s2u_i - jitter, 0), each added in one fixed tree order
// (nblk = ceil(n / 256) apart); lam (optional): lambda_i.
struct SgpKufArgs {
    KParams kp;
    int m, mp;
    const double *Z; int ldz;        // the inducing points, m rows ldz apart (a frame's Xp)
    const double *X; int n;          // the chunk, n x D
    const double *Y;                 // n
    const double *s2u;               // n
    int fitc;
    double noise, jitter;
    int ld;                          // n rounded up to 32
    double *Ft;
    double *lam;
    double *part;
};
int launch_sgp_scaled_kuf(const SgpKufArgs &a, hipStream_t s);

// G+ (the lower 64 x 64 tiles of an (mp + 64)^2 matrix, rows ldg apart) += Ft Ft^T over the chunk's ld columns: the accumulators are
// loaded from G+ and continued in ascending observation order.  Row mp of G+ then holds b = F y~, its diagonal entry y~.y~.
int launch_sgp_gram(const double *Ft, int ld, int mp, double *G, hipStream_t s);

// A = Kuu + G, m x m with rows m apart, both triangles from one sum (Kuu: rows ldk apart, its lower triangle is read); Y (Np): b, then zeros
int launch_sgp_assemble(const double *Kuu, int ldk, const double *G, int ldg, int m, int mp, int Np, double *A, double *Y, hipStream_t s);

// One chunk of candidates from the two frames' plain sweeps: s2 = noise + (s2u - jitter) + (1 - s2a), clipped to [clamp_lo, 10];
// mu = mua; then the acquisition, the exclusion balls and one (max, lowest index) partial per 256 candidates.
struct SgpFinishArgs {
    FinishTail t;                        // the chunk, the exclusion balls, the partials
    const double *s2u, *mua, *s2a;
    double noise, jitter, clamp_lo, ymax, parm;
    int acq, erf_mode;
    double *out_mu, *out_s2, *out_acq;   // the chunk's part of the optional outputs
};
int launch_sgp_finish(const SgpFinishArgs &a, hipStream_t s);

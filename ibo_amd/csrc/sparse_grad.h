// sparse_grad.h -- the kernels of the sparse GP's marginal-likelihood gradient (sparse_grad.hip; abi_sparse.hip: ibo_sgp_nlml_grad).
//
// With K = K_uf (m x N, columns k_i), mu_i = alpha.k_i, a_i = k_i^T A^-1 k_i, c_i = dNL/dlambda_i and e_i the weight on d max(1 - q_i, 0):
//   g_i = (A^-1 k_i + alpha (mu_i - y_i)) / lambda_i - 2 e_i K~uu^-1 k_i                     dNL/dK, never stored
//   S   = (A^-1 + alpha alpha^T - K~uu^-1) / 2 + K~uu^-1 (K E K^T) K~uu^-1, diagonal 0        dNL/dK~uu
// and with rho = dk/dz (z = sum_d w_d Delta_d^2), Delta = Z_ad - X_id (or Z_ad - Z_bd), h = g rho:
//   sumZ[a][d] = sum_i h_ai Delta_d     sumL[a][d] = sum_i h_ai Delta_d^2     sumS = sum_ai g_ai k_ai
// which the host turns into the gradient (abi_sparse.hip).
#pragma once
#include "ibo_common.h"

#define SGP_GRAD_FITC 0
#define SGP_GRAD_DTC  1
#define SGP_GRAD_VFE  2

// Per observation of a chunk (n live of ld, ld a multiple of 64): lambda_i, e_i, r_i = (mu_i - y_i) / lambda_i; the pad gets (1, 0, 0).
// s2u: the U frame's unclipped variance 1 + jitter - q_i; mua, s2a: the A frame's mean and variance 1 - a_i.  part: sum of c_i per 256
// observations in one fixed tree order.
struct SgpGradObsArgs {
    int n, ld, kind;
    double noise, jitter;
    const double *s2u, *mua, *s2a, *Y;
    double *lam, *ev, *rv, *part;
};
int launch_sgp_grad_obs(const SgpGradObsArgs &a, hipStream_t s);

// The chunk's operands from k_ai = k(z_a, x_i) (the difference form and cov_from_z_fast of sgp_scaled_kuf_kernel: the fit's bits):
//   Bo   observation-major, ld rows of ldb doubles: [k_ai / lambda_i | -2 e_i k_ai]  (the second half only when two)
//   Kt, KEt (optional) contraction-major, mp rows of ld doubles: k_ai and e_i k_ai
// zero for a >= m and i >= n.
struct SgpGradGenArgs {
    KParams kp;
    int m, mp;
    const double *Z; int ldz;
    const double *X; int n, ld;
    const double *lam, *ev;
    int two;
    double *Bo; int ldb;
    double *Kt, *KEt;
};
int launch_sgp_grad_gen(const SgpGradGenArgs &a, hipStream_t s);

// The fused contraction.  A workgroup owns 64 inducing rows and walks its strip of 64-observation tiles in ascending order:
//   from_S = 0: the tile of g on v_mfma_f64_16x16x4_f64 (cv_tile): [A^-1 | K~uu^-1] (rows ldi apart) against Bo, plus alpha_a r_i
//   from_S = 1: the tile is read from S (rows lds apart) and the "observations" are the inducing points themselves (X = Z, n = m)
// then the derivative epilogue through LDS.  partZ, partL: nstrips x mp x D (zeroed by the caller; a workgroup adds to its own rows only);
// partS: nstrips x (mp / 64).  No atomics: the same bits from call to call.
struct SgpGradArgs {
    KParams kp;
    int m, mp;
    const double *Z; int ldz;
    const double *Ainv, *Uinv; int ldi;
    int two;
    const double *Bo; int ldb;
    const double *alpha, *rv;
    const double *X; int ldx, n;
    int ntiles, tiles_per_strip, nstrips;
    const double *S; int lds;
    double *partZ, *partL, *partS;
};
int launch_sgp_grad_contract(const SgpGradArgs &a, int from_S, hipStream_t s);

// tot += the partials, strips in ascending order: totZ, totL (m x D), totS (one double; the row blocks in ascending order within a strip)
int launch_sgp_grad_reduce(const double *partZ, const double *partL, const double *partS, int nstrips, int m, int mp, int D,
                           double *totZ, double *totL, double *totS, hipStream_t s);

// C (64 x 64 tiles, rows ldc apart) = or += A B^T over kend (a multiple of 32) through cv_tile; rows: a multiple of 64.
// lower_only: the tiles on and below the diagonal.
int launch_sgp_abt(const double *A, int lda, const double *B, int ldb, double *C, int ldc, int rows, int kend, int accumulate, int lower_only, hipStream_t s);
// the upper triangle from the lower one
int launch_sgp_mirror(double *H, int ld, int rows, hipStream_t s);
// S = (A^-1 + alpha alpha^T - K~uu^-1) / 2 + (M + M^T) / 2 off the diagonal of the leading m x m block (M optional), 0 elsewhere in mp x mp
int launch_sgp_grad_S(const double *Ainv, const double *Uinv, int ldi, const double *alpha, const double *M, int ldm, int m, int mp, double *S, hipStream_t s);

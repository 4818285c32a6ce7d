// loo.h -- the leave-one-out kernels (loo.hip) behind ibo_gp_loo (abi_fit.hip) and ibo_loo_grad (abi_nlml.hip).  With B = A^-1, d_i = B_ii
// and alpha = B y:  mu_-i = y_i - alpha_i / d_i,  s2_-i = 1 / d_i,  nloo = sum_i [-log(d_i) / 2 + alpha_i^2 / (2 d_i)] + N log(2 pi) / 2.
// Every matrix is row-major with 64-bit offsets.
#pragma once
#include "ibo_common.h"

#define IBO_LOO_HP 4             // derivatives one pass of loo_contract_kernel takes off one panel of B

// d_i = sum_{i <= k < N} W[k][i]^2 for the lower triangular W = L^-1 (ld ldw); whatever lies above W's diagonal is never read
int launch_loo_diag(const double *W, size_t ldw, int N, double *d, hipStream_t s);
// on a fitted handle: c_i = aY_i - m(x_i) a1_i (m: the mean prior, 0 without one), mu_i = Y_i - c_i / d_i, s2_i = 1 / d_i (unclipped) and
// out[0] = sum_i [-log(d_i) / 2 + c_i^2 / (2 d_i)] in a fixed order.  mu / s2 / out: device, each optional.
int launch_loo_handle(const PriorDev &prior, const double *Xp, int DP, int D, int N, const double *Y, const double *aY, const double *a1,
                      const double *d, double *mu, double *s2, double *out, hipStream_t s);
// the value side of ibo_loo_grad from B (ldb; only the diagonal is read) and alpha: out[0] = the sum above; mu / s2 optional
int launch_loo_value(const double *B, size_t ldb, int N, const double *Y, const double *alpha, double *mu, double *s2, double *out,
                     hipStream_t s);
// doubles of scratch launch_loo_contract needs for an Np-row problem (one pass' partial sums)
size_t loo_contract_scratch(int Np);
// grad[h] = d nloo / d log theta_h for h < gs.nh, from B (Np x Np, ld Np: the 64 x 64 blocks on and below the diagonal, the others taken as
// their mirror images; rows and columns >= N never used), alpha, X (N x D, ld ldx) and the kernel: T = B dA_h on the MFMA unit, dA_h made
// from X on the fly, IBO_LOO_HP derivatives per pass.  grad: device, gs.nh doubles.  Fixed-order sums, no atomics.
int launch_loo_contract(const KParams &kp, const GradSpec &gs, int N, int Np, const double *X, int ldx, const double *B, const double *alpha,
                        double *part, double *grad, hipStream_t s);

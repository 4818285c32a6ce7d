// gradobs.h -- the derivative covariance of a GP observed with gradients (gradobs.hip) and what the ABI unit (abi_gradobs.hip) hands it.
// Row-major everywhere, 64-bit offsets.
//
// Rows are POINT-MAJOR: row i (D + 1) is the value at x_i, rows i (D + 1) + d (d = 1 .. D) are df/dx_d at x_i; P = N (D + 1).
// With u = x - x' (x the row's point, x' the column's), t_d = w_d u_d and three factors per point pair,
//   SE          k = sf2 exp(-z / 2)               g1 = k                       g2 = k
//   Matern-3/2  k = sf2 (1 + r) exp(-r)           g1 = 3 sf2 exp(-r)           g2 = 3 g1 / r   (0 at r = 0)
//   Matern-5/2  k = sf2 (1 + r + r^2/3) exp(-r)   g1 = 5/3 sf2 (1 + r) exp(-r) g2 = 25/3 sf2 exp(-r)
// (z = sum_d w_d u_d^2; r = sqrt(3 z), sqrt(5 z)), the (D + 1) x (D + 1) block of the pair is
//   [ k           g1 t_e                          ]        (value, d/dx'_e)
//   [ -g1 t_d     g1 w_d delta_de - g2 (t_d t_e)  ]        (d/dx_d, d2/dx_d dx'_e)
// t_d t_e is formed first, so the entry (a, b) of the pair (i, j) and the entry (b, a) of the pair (j, i) are the same bits.
#pragma once
#include "ibo_common.h"

// A in the identity-padded frame factor_invert takes: Np x Np (ld Np), A[r][c] for r, c < P = N (D + 1) from the blocks above with the
// diagonal rule -- vdiag on a value row, g1(0) w_d + gnoise[d - 1] on derivative row d -- and the identity on the rows and columns
// [P, Np).  vdiag is the caller's: 1 + noise for the fit (whatever sf2 is), sf2 + noise for the marginal likelihood (the same bits at
// sf2 = 1).  X: N x D (device), gnoise: D (device).  Every element of the frame is written, both triangles.
int launch_gradobs_assemble(const KParams &kp, const double *X, int N, double vdiag, const double *gnoise, double *A, int Np,
                            hipStream_t s);
// The gradient of the marginal likelihood (ibo_ggp_nlml_grad): sum_ab (Kinv - alpha alpha^T)_ab (dA/dlog theta_h)_ab / 2 for the ngrad
// derivatives of gs, then the 1 + D noise terms noise_e sum_{rows of kind e} (diag Kinv - alpha o alpha) / 2, into out (ngrad + 1 + D).
// Kinv: Np x Np (ld Np), valid in its lower 64 x 64 blocks (read at (max, min) on a point's own block); alpha: P.  One workgroup per tile
// of 16 x 16 point pairs on and below the diagonal; pairs below it count twice.  Per pair, with M = Kinv - alpha alpha^T split into its
// scalar m00, its vectors a_e = M_0e, b_d = M_d0 and its D x D block C, the block's sum is
//   F = k m00 + g1 ((a - b).t + sum_d w_d C_dd) - g2 t^T C t
// and every derivative follows from m00, S1 = (a - b).t + sum_d w_d C_dd, q = t^T C t and, per dimension, V_d = -2 g1 ((a - b)_d t_d +
// w_d C_dd) + 2 g2 t_d ((C t)_d + (C^T t)_d):  signal 2 F;  one shared length scale g1 z m00 + (g2 z - 2 g1) S1 - (dg2 - 4 g2) q;  the
// length scale of dimension d  w_d u_d^2 (g1 m00 + g2 S1 - (dg2 / z) q) + V_d  (dg2: the finite form of gradobs.hip, 0 at r = 0).
// A tile's partial sums (D dimensions, shared, signal; the diagonal tiles' 1 + D noise sums) go to `part`, gradobs_contract_scratch(N, D)
// doubles, and are added in a fixed order: no atomics, and a component's bits do not depend on gs.
size_t gradobs_contract_scratch(int N, int D);
int launch_gradobs_contract(const KParams &kp, const GradSpec &gs, const double *X, int N, const double *Kinv, int Np, const double *alpha,
                            double noise, const double *gnoise, double *part, double *out, hipStream_t s);
// Kt[c][j (D + 1)] = k(q_c, x_j), Kt[c][j (D + 1) + d] = dk(q_c, x_j) / dx_j,d = g1 t_d (u = q_c - x_j) for c < m, j < N; 0 elsewhere in
// the mp x Pp block (ld Pp): the layout launch_cov_tri reads.  Q: m x D (device).  mp <= 65535.
int launch_gradobs_kstar(const KParams &kp, const double *X, int N, int Pp, const double *Q, int m, int mp, double *Kt, hipStream_t s);
// acq[i] = the acquisition (acq_value_dev: EI / PI / UCB in either erf flavour; IBO_ACQ_NONE: mu) from mu[i] and s2[i], i < m; mu_out /
// s2_out (optional) receive copies of mu / s2
int launch_gradobs_acq(int acq, int erf_mode, double ymax, double parm, const double *mu, const double *s2, int m, double *out,
                       double *mu_out, double *s2_out, hipStream_t s);

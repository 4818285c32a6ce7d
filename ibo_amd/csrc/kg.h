// kg.h -- the knowledge-gradient kernels (kg.hip) and what the ABI unit (abi_kg.hip) hands them.  Row-major everywhere, 64-bit offsets.
//
// One chunk of candidates goes through cov.hip's two launchers (Kt = K(X, data), Vt = Kt W^T) and then
//   kg_rows     per row of Kt / Vt: the posterior mean, |v|^2, the clipped variance
//   kg_cross    B[x][a] = (k(a, x) - v_a.v_x) / sigma_x against the resident reference rows, candidate-major (MFMA, cov_dev.h's tile)
//   kg_epigraph KG(x) = E max_i (mu_i + b_i Z) - max_i mu_i by the pair scan of ibo_abi.h
//   kg_argmax   one (max, lowest index) partial per 256 candidates for launch_argmax_final
// Nothing a candidate's value is made of depends on the chunk, on the candidate's place in it or on how many there are.
#pragma once
#include "ibo_common.h"

#define IBO_KG_LINES 1025        // IBO_KG_MAX_REF reference lines + the candidate's own

// One row r < m of Kt (ldk) and Vt (ldv), both at least Npad wide: muY = Kt[r].aY and mu1 = Kt[r].a1 over k < N and q = |Vt[r]|^2 over
// k < K, each lane over k = lane, lane + 64, .. in ascending order, then one butterfly over the wavefront; mu = m + muY - m mu1 with the
// mean prior m at Q[r] (muY without one); s2 = 1 + noise - q clipped to [clamp_lo, 10].  q_out, s2_out may be NULL.
struct KgRowsArgs {
    const double *Kt; size_t ldk;
    const double *Vt; size_t ldv;
    const double *alphaY, *alpha1;
    const double *Q; int D;             // m x D
    PriorDev prior;
    int N, K, m;
    double noise, clamp_lo;
    double *mu, *q, *s2;
};
int launch_kg_rows(const KgRowsArgs &a, hipStream_t s);

// B[x][a] for x < m, a < n from the 64 x 64 tiles of VtX VtA^T (VtX: mp x >= K, VtA: np x >= K, mp, np multiples of 64, K of 32);
// sigma_x = sqrt(s2[x]).  B: mp x ldb, ldb >= np; entries beyond (m, n) are written as 0.  unscaled != 0: B[x][a] = k(a, x) - v_a.v_x, the
// covariance itself (s2 is not read) -- the same tile body and the same difference, without the division.
struct KgCrossArgs {
    KParams kp;
    const double *VtX; size_t ldx; int m, mp;
    const double *VtA; size_t lda; int n, np;
    int K;
    const double *X, *A;                // m x D, n x D
    const double *s2;                   // m
    double *B; size_t ldb;
    int unscaled;
};
int launch_kg_cross(const KgCrossArgs &a, hipStream_t s);

// kg[x], x < m.  Lines: with_self the candidate's own (mu[x], max(1 - q[x], 0) / sqrt(s2[x])) first, then (muA[a], B[x][a]), a < n.
struct KgEpiArgs {
    int m, n, with_self;
    const double *muA; double maxA;     // max_a muA[a]
    const double *mu, *q, *s2;          // m
    const double *B; size_t ldb;
    double *kg;
};
int launch_kg_epigraph(const KgEpiArgs &a, hipStream_t s);

// part_val / part_idx[b] = (max, lowest index) over the candidates 256 b <= i < min(256 b + 256, m); the index is index_base + first + position.  NaN never wins.
int launch_kg_argmax(const double *kg, int64_t m, int64_t first, int64_t index_base, double *part_val, int64_t *part_idx, hipStream_t s);

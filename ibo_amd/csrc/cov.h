// cov.h -- the joint-posterior kernels of ibo_posterior_cov / ibo_posterior_sample (cov.hip) and what the ABI units (abi_batch.hip, abi_kg.hip)
// hands them.  Every matrix is row-major with 64-bit offsets: Sigma reaches 2^31 bytes at M = 16384, K* and V 2.1 GB at N = 16400.
#pragma once
#include "ibo_common.h"

#define IBO_COV_TILE 64          // rows and columns of every padded operand are multiples of this

// Kt[c][j] = k(q_c, X_j) for c < m, j < N (k with kp.sf2, the handle's k* signal variance); 0 elsewhere in the mp x Npad block
int launch_cov_kstar(const KParams &kp, const double *Xp, int N, int Npad, int DP, const double *Q, int m, int mp, double *Kt,
                     hipStream_t s);
// C[r][n] = sum_{k <= n} A[r][k] B[n][k] over n < nvalid (B's other entries, whatever they hold, are never used): rows x ncols
// (both multiples of 64; A: rows x >= ncols, lda; B: ncols x >= ncols, ldb).  V^T = K*^T W^T and F = Z L^T.
int launch_cov_tri(const double *A, size_t lda, const double *B, size_t ldb, int nvalid, int rows, int ncols, double *C, size_t ldc,
                   hipStream_t s);
// S[a][b] = S[b][a] = k(q_a, q_b) - v_a.v_b (a != b), S[a][a] = diag - |v_a|^2, for a, b < M, from the lower 64 x 64 tiles of
// Vt Vt^T (Vt: Mp x >= K, ld ldv; K a multiple of 16).  pad: the rows and columns [M, Mp) are identity (the in-place Cholesky's pad).
int launch_cov_syrk(const KParams &kp, const double *Q, const double *Vt, size_t ldv, int K, int M, int Mp, double diag, int pad,
                    double *S, size_t lds, hipStream_t s);

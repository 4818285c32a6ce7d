// downdate.h -- the kernels (downdate.hip) behind ibo_gp_remove (abi_fit.hip): one observation taken out of a fitted model in O(N^2), from
// the L and the W = L^-1 the handle holds.  With row / column i removed, m = N - 1 - i rows below it and L33 the trailing block:
//     p = -W[i+1:, i] / W[i, i] (= L33^-1 l32),   t_0 = 1, t_{k+1} = t_k + p_k^2,   d_k = sqrt(t_{k+1} / t_k),   q_k = p_k / sqrt(t_k t_{k+1})
//     L33' = L33 (diag(d) + strict-lower(p q^T))                    a suffix scan along every row
//     W'   = (diag(1 / d) - strict-lower(q p^T)) (W[i+1:, :] + p (x) W[i, :]), column i dropped      a prefix scan down every column
// Every matrix is Npad x Npad row-major, out of place (the shift by one row and one column makes an in-place rewrite a race between
// workgroups), 64-bit addresses throughout.  Fixed-order sums, no atomics on data: the same call gives the same bits.
#pragma once
#include "ibo_common.h"

// doubles of scratch a removal needs: p, d, q, 1 / d (Npad each) and the W kernel's partial sums ((Npad / 64) x Npad)
size_t downdate_scratch(int Npad);
// p, d, q, 1 / d of removing row i of the N-row model (ws as above).  info (device int, not cleared here) receives i + 1 when W[i][i] is not
// finite and positive or a t is not finite; the kernels after it then write nothing that is used.
int launch_downdate_scalars(const double *W, int N, int Npad, int i, double *ws, int *info, hipStream_t s);
// Lout = the factor without row i in the padding invariants of a fit: lower triangle of the N - 1 rows, zeros above the diagonal inside the
// diagonal blocks, identity on rows >= N - 1.  The 64 x 64 blocks right of the diagonal blocks are not written (as a fit leaves them: scratch
// until launch_zero_upper).  Only L's lower triangle is read.
int launch_downdate_L(const double *L, int N, int Npad, int i, const double *ws, double *Lout, hipStream_t s);
// Wout = W' on and below the diagonal blocks: zeros above the diagonal inside them, on rows >= N - 1 and on columns >= N - 1; the blocks right
// of the diagonal blocks are not written (launch_pack_w, which every removal ends with, takes the lower triangle only).  Only W's lower
// triangle is read.
int launch_downdate_W(const double *W, int N, int Npad, int i, double *ws, double *Wout, hipStream_t s);
// Xout = Xp without row i (rows >= N - 1 zero); Npad x DP each, Xout another buffer than Xp
int launch_downdate_X(const double *Xp, int N, int Npad, int DP, int i, double *Xout, hipStream_t s);

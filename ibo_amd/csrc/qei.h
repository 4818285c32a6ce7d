// qei.h -- the Monte-Carlo finish of the parallel expected improvement (qei.hip) and what the ABI unit (abi_qei.hip) hands it.
//
// One chunk of candidates goes through cov.hip's two launchers (Kt = K(X, data), Vt = Kt W^T), kg.hip's row kernel (mu, |v|^2, the clipped
// s2) and kg.hip's cross kernel without its division (C[x][j] = k(p_j, x) - v_pj.v_x against the resident pending rows), and then
//   qei_finish   qEI(x | P) = (1/S) sum_s max(max(f_s, g_s) - t, 0),  f_s = mu_x + sum_j l_j z_sj + d z_sp,  l = L_P^-1 c,  d = sqrt(max(s2 - |l|^2, 0))
// Nothing a candidate's value is made of depends on the chunk, on the candidate's place in it or on how many there are.
#pragma once
#include "ibo_common.h"

#define QEI_MAX_P 15             // IBO_QEI_MAX_PENDING
#define QEI_SB 256               // samples per LDS stage
#define QEI_CW 4                 // candidates per wavefront: 16 per workgroup share a stage of samples

// The samples as the device holds them, transposed and padded: ZG[j Sp + s] = z_sj for j <= p, ZG[(p + 1) Sp + s] = g_s; Sp = S rounded
// up to QEI_SB (the padding is never added to a sum).  L: L_P packed by rows, L[j (j + 1) / 2 + i] = L_ji for i <= j < p -- in the kernel's
// arguments, so that the forward substitution reads it through the scalar cache.
struct QeiFinishArgs {
    int m, p, S, Sp;
    double t;                            // ymax + xi
    const double *ZG;
    const double *mu, *s2;               // m
    const double *C; size_t ldc;         // m x ldc, ldc >= p (not read when p == 0)
    double *qei;                         // m
    double L[QEI_MAX_P * (QEI_MAX_P + 1) / 2];
};
int launch_qei_finish(const QeiFinishArgs &a, hipStream_t s);

// grad.h -- the gradient kernels of ibo_acq_grad_batch (grad.hip) and what the ABI unit (abi_batch.hip) hands them.
#pragma once
#include "ibo_common.h"

struct GradArgs {
    KParams kp;                  // kp.sf2: the k* signal variance (ibo_gp_set_kstar_sf2)
    int N, Npad, DP;
    const double *Xp;            // Npad x DP, zero padded
    const double *W;             // Npad x Npad row-major, lower triangular (W = L^-1)
    const double *alphaY, *alpha1;
    PriorDev prior;
    double noise, clamp_lo, ymax, parm;
    int acq, erf_mode;
    // the chunk's plan (grad_plan) and its scratch
    int TM, KC, nsplit, nparts;
    double *K, *H;               // mc x Npad each
    double *Pt, *Pu;             // nsplit x mc x Npad each
    double *E;                   // mc x nparts x (3 + 2 DP)
};

struct GradPlan {
    int TM;                      // candidates per tile of the triangular products (16 or 64)
    int mc;                      // candidates per chunk
    int KC, nsplit;              // split-K: ranges of KC rows of W (a multiple of 64), nsplit of them cover the model's rows
    int nparts;                  // row parts of the epilogue
    size_t ws_doubles;           // scratch of one chunk
};

GradPlan grad_plan(int N, int Npad, int DP, int64_t M);
// cand: mc x D (device memory or pinned host memory); dmu / ds2 / dacq: mc x D each, optional
int launch_grad(const GradArgs &a, const double *cand, int mc, double *dmu, double *ds2, double *dacq, hipStream_t s);

// paths.h -- the pathwise posterior draws' kernels (paths.hip) and what the ABI unit (abi_paths.hip) hands them.  Row-major, 64-bit offsets.
//
//   paths_tile    values of 64 candidates x 64 coefficient columns: sum_k A[x][k] coef[k][c] over the unified k axis
//                   k in [0, Fp)            A = amp cos(omega_k . x + b_k)   (0 for F <= k < Fp)
//                   k in [Fp, Fp + Np32)    A = k(x, X_{k - Fp})             (0 beyond the model's N rows)
//                 with A generated into LDS a k-step of 32 at a time (never written to memory), on v_mfma_f64_16x16x4_f64; the epilogue
//                 adds the mean prior, writes the values path-major and one (max, first index) partial per path and 64 candidates
//   paths_grad    d/dx_d of the same sums for PG_DC dimensions per workgroup: the derivative of the generated piece -- -amp sin(.) omega_kd,
//                 h_i w_d (x_d - X_id) -- is generated the same way, one 64 x 32 piece and one accumulator set per dimension; the epilogue applies
//                 dm (1 - s1) + g - m gs1 with a mean prior (s1, gs1 from column 63) and writes [s][x][d], or [x][d] for the path path_of[x]
//   paths_solve   coef[Fp + j][col(s)] = aY[j] - sum_{i >= j} W[i][j] Y[s][i], i ascending (z = W^T y: the second half of A^-1 = W^T W)
//   paths_final   per path the winner among its partials (the rule of ibo_common.h: larger value, then lower index; INT64_MAX when none)
// A value depends on the path object and the candidate's coordinates alone: the k order is fixed, and no sum crosses a candidate row.
#pragma once
#include "ibo_common.h"

#define PT_KB 32                 // k-step staged in LDS
#define PT_LDA (PT_KB + 1)       // LDS row stride of the generated operand (odd: a fragment's 16 rows fall on distinct banks)
#define PG_DC 4                  // dimensions per workgroup of the gradient kernel (one accumulator set each; one wave per SIMD)
#define PT_LDB 80                // LDS row stride of the coefficient rows (two consecutive k rows fall on the two halves of the banks)

// Coefficient columns: a tile of 64 columns carries `pt` paths -- 64, or 63 with a mean prior, whose column 63 holds alpha_1 on the
// kernel rows (0 on the feature rows): k*.a1 of the candidate, which the prior's mean needs, comes out of the same contraction.
// Path s is column 64 (s / pt) + s % pt.
static inline int paths_col(int s, int pt) { return 64 * (s / pt) + s % pt; }

struct PathsArgs {
    KParams kp;                         // family, D, w; sf2: the k* signal variance
    const double *X; int ldx, N;        // the model's rows, N x ldx
    const double *omega, *phase;        // Fp x D and Fp, zero beyond F
    int F, Fp; double amp;              // amp = sqrt(2 sf2 / F)
    const double *coef; int Sp;         // (Fp + Np32) x Sp
    int kend;                           // Fp: the feature part alone (ibo_paths_create's Phi(X) w); Fp + Np32: the whole path
    PriorDev prior;                     // nb > 0: value = m + acc - m acc_63 (needs pt == 63)
    int pt, S;
    int only;                           // >= 0: this path alone, from its own column tile, into values[voff + x] (DIRECT's evaluator)
    const double *cand; int ldc, m;     // this launch's candidates, m x ldc
    int64_t first, index_base;          // the first candidate's place in the whole array (a multiple of 64); added to the winner's index
    double *values; size_t ldv; int64_t voff;       // values[s ldv + voff + x] (+= what is there already, if accumulate), or NULL
    int accumulate;
    double *part_val; int64_t *part_idx; int64_t nblk;      // [s nblk + first / 64 + tile], or NULL
};
int launch_paths_tile(const PathsArgs &a, hipStream_t s);

// The gradient of a launch's m points: a.cand / ldc / m and the object's fields of a (values, partials and `only` are not read).
struct PathsGradArgs {
    PathsArgs a;
    const int *path_of;                 // device, m entries in [0, S): grads[(goff + x) D + d] of path path_of[x] alone; NULL: every path,
    double *grads; size_t ldg;          //   grads[((s ldg) + goff + x) D + d]
    int64_t goff;
};
int launch_paths_grad_tile(const PathsGradArgs &ga, hipStream_t s);
int launch_paths_pick(const double *vals, size_t ldv, const int *path_of, int m, double *out, hipStream_t s);     // out[i] = vals[path_of[i] ldv + i]

// Y: rows of paths (ldy apart), W: Np x Np lower triangular row-major; writes the kernel rows of coef for s < S, and alpha_1 into
// column 63 of every tile when pt == 63
int launch_paths_solve(const double *W, int Np, int N, const double *Y, size_t ldy, int S, int pt, const double *aY, const double *a1,
                       double *coef, int Sp, int Fp, hipStream_t s);

int launch_paths_final(const double *part_val, const int64_t *part_idx, int64_t nblk, int S, double *out_val, int64_t *out_idx,
                       hipStream_t s);

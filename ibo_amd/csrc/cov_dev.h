// cov_dev.h -- the 64 x 64 tile product on v_mfma_f64_16x16x4_f64 that cov.hip's kernels and kg.hip's cross kernel share: one body, so that
// every product formed from V^T rows sums its k terms in the same order wherever it is used.
#pragma once
#include "ibo_common.h"

#define CV_KB 32                 // k-step staged in LDS
#define CV_LD (CV_KB + 1)        // LDS row stride in doubles (odd: the 16 rows of a fragment fall on distinct banks)

typedef double cv_d2 __attribute__((ext_vector_type(2)));

// acc += the 64 x 64 tile at (r0, n0) of A B^T over k in [0, kend) (kend a multiple of CV_KB).  TRI: B[n][k] is taken as 0 unless
// k <= n < nvalid.  Wave w holds rows 32 (w >> 1) + {0, 16}, columns 32 (w & 1) + {0, 16}: acc[i][j].
template <bool TRI>
__device__ __forceinline__ void cv_tile(const double *__restrict__ A, size_t lda, const double *__restrict__ B, size_t ldb, int r0, int n0,
                                        int kend, int nvalid, d4_t (&acc)[2][2], double *As, double *Bs)
{
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6, wr = wv >> 1, wc = wv & 1;
    const int lr = t >> 4, lk = (t & 15) * 2;             // this thread's rows lr + 16 u and k pair lk of a stage
    cv_d2 va[4], vb[4];
    auto fetch = [&](int kb) {
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const int row = lr + 16 * u;
            va[u] = *(const cv_d2 *)(A + (size_t)(r0 + row) * lda + kb + lk);
            cv_d2 b = *(const cv_d2 *)(B + (size_t)(n0 + row) * ldb + kb + lk);
            if (TRI) {
                const int n = n0 + row, k = kb + lk;
                const bool live = n < nvalid;
                b.x = (live && k <= n) ? b.x : 0.0;
                b.y = (live && k + 1 <= n) ? b.y : 0.0;
            }
            vb[u] = b;
        }
    };
    fetch(0);
    for (int kb = 0; kb < kend; kb += CV_KB) {
#pragma unroll
        for (int u = 0; u < 4; u++) {
            double *a = As + (lr + 16 * u) * CV_LD + lk, *b = Bs + (lr + 16 * u) * CV_LD + lk;
            a[0] = va[u].x; a[1] = va[u].y;
            b[0] = vb[u].x; b[1] = vb[u].y;
        }
        __syncthreads();
        if (kb + CV_KB < kend) fetch(kb + CV_KB);
#pragma unroll
        for (int kk = 0; kk < CV_KB; kk += 4) {
            const int ko = kk + (lane >> 4), ro = lane & 15;
            const double a0 = As[(32 * wr + ro) * CV_LD + ko], a1 = As[(32 * wr + 16 + ro) * CV_LD + ko];
            const double b0 = Bs[(32 * wc + ro) * CV_LD + ko], b1 = Bs[(32 * wc + 16 + ro) * CV_LD + ko];
            acc[0][0] = mfma_f64(a0, b0, acc[0][0]);
            acc[0][1] = mfma_f64(a0, b1, acc[0][1]);
            acc[1][0] = mfma_f64(a1, b0, acc[1][0]);
            acc[1][1] = mfma_f64(a1, b1, acc[1][1]);
        }
        __syncthreads();
    }
}

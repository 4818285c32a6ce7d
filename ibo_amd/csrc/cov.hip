// cov.hip -- the joint posterior of M query points (ibo_posterior_cov) and draws from it (ibo_posterior_sample).
//
//   cov_kstar_kernel   Kt = K(Q, X): mp x Npad, query-major, zero beyond the model's rows and the chunk's points
//   cov_tri_kernel     Vt = Kt W^T (V = W K*, W = L^-1 lower triangular: the blocks above its diagonal are skipped) and, for the
//                      draws, F = Z L_S^T -- one kernel: C[r][n] = sum_{k <= n} A[r][k] B[n][k]
//   cov_syrk_kernel    Sigma = K(Q, Q) - V^T V on the lower 64 x 64 tiles; the epilogue forms k(q_a, q_b) and the diagonal rule and
//                      mirrors every element into the upper triangle (exactly symmetric)
// Both products run on v_mfma_f64_16x16x4_f64: 64 x 64 output tiles, four waves of 32 x 32, k-steps of 32 staged in LDS with the next
// step's operands in registers while the current one is on the MFMAs.  Every output element sums its k terms in ascending order in one
// workgroup: the same call gives the same bits.  Operands are read with 64-bit addresses (no buffer descriptors): Sigma is 2^31 bytes
// at M = 16384, Kt and V 2.1 GB at N = 16400, M = 16384.
#include "cov.h"
#include "cov_dev.h"

__global__ void __launch_bounds__(256) cov_kstar_kernel(KParams kp, const double *__restrict__ Xp, int N, int Npad, int DP,
                                                        const double *__restrict__ Q, int m, double *__restrict__ Kt)
{
    __shared__ double xs[IBO_DMAX];
    const int c = blockIdx.y, D = kp.D;
    if ((int)threadIdx.x < D) xs[threadIdx.x] = c < m ? Q[(size_t)c * D + threadIdx.x] : 0.0;
    __syncthreads();
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= Npad) return;
    double k = 0.0;
    if (c < m && j < N) {
        k = cov_from_z_rt(kp.family, wsqdist_dev(kp.w, xs, Xp + (size_t)j * DP, D), kp.sf2);
    }
    Kt[(size_t)c * Npad + j] = k;
}

// one 64 x 64 tile of C per workgroup; column blocks in descending order (the longest k ranges start first)
__global__ void __launch_bounds__(256) cov_tri_kernel(const double *__restrict__ A, size_t lda, const double *__restrict__ B, size_t ldb,
                                                      int nvalid, int nbn, double *__restrict__ C, size_t ldc)
{
    __shared__ double As[64 * CV_LD], Bs[64 * CV_LD];
    const int n0 = (nbn - 1 - (int)blockIdx.x) * 64, r0 = blockIdx.y * 64;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, wr = wv >> 1, wc = wv & 1;
    d4_t acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; i++)
#pragma unroll
        for (int j = 0; j < 2; j++) acc[i][j] = d4_t{0.0, 0.0, 0.0, 0.0};
    const int kv = (nvalid + CV_KB - 1) / CV_KB * CV_KB;
    const int kend = n0 + 64 < kv ? n0 + 64 : kv;
    if (n0 < nvalid) cv_tile<true>(A, lda, B, ldb, r0, n0, kend, nvalid, acc, As, Bs);
#pragma unroll
    for (int i = 0; i < 2; i++)
#pragma unroll
        for (int j = 0; j < 2; j++)
#pragma unroll
            for (int e = 0; e < 4; e++) {
                const int r = r0 + 32 * wr + 16 * i + (lane >> 4) + 4 * e, n = n0 + 32 * wc + 16 * j + (lane & 15);
                C[(size_t)r * ldc + n] = acc[i][j][e];
            }
}

// one lower 64 x 64 tile (bm >= bn) per workgroup, blockIdx.x = bm (bm + 1) / 2 + bn
__global__ void __launch_bounds__(256) cov_syrk_kernel(KParams kp, const double *__restrict__ Q, const double *__restrict__ Vt, size_t ldv,
                                                       int K, int M, int Mp, double diag, int pad, double *__restrict__ S, size_t lds)
{
    __shared__ double As[64 * CV_LD], Bs[64 * CV_LD];
    const int t = blockIdx.x;
    int bm = (int)((sqrt(8.0 * t + 1.0) - 1.0) * 0.5);
    while ((bm + 1) * (bm + 2) / 2 <= t) bm++;
    while (bm * (bm + 1) / 2 > t) bm--;
    const int bn = t - bm * (bm + 1) / 2;
    const int r0 = bm * 64, n0 = bn * 64;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, wr = wv >> 1, wc = wv & 1, D = kp.D;
    d4_t acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; i++)
#pragma unroll
        for (int j = 0; j < 2; j++) acc[i][j] = d4_t{0.0, 0.0, 0.0, 0.0};
    cv_tile<false>(Vt, ldv, Vt, ldv, r0, n0, K, 0, acc, As, Bs);
#pragma unroll
    for (int i = 0; i < 2; i++)
#pragma unroll
        for (int j = 0; j < 2; j++)
#pragma unroll
            for (int e = 0; e < 4; e++) {
                const int a = r0 + 32 * wr + 16 * i + (lane >> 4) + 4 * e, b = n0 + 32 * wc + 16 * j + (lane & 15);
                if (a < b) continue;                          // (diagonal tiles) the upper element is the mirror of the lower one
                double v;
                if (a >= M || b >= M) {
                    if (!pad) continue;
                    v = a == b ? 1.0 : 0.0;
                } else if (a == b) {
                    v = diag - acc[i][j][e];
                } else {
                    v = cov_from_z_rt(kp.family, wsqdist_dev(kp.w, Q + (size_t)a * D, Q + (size_t)b * D, D), kp.sf2) - acc[i][j][e];
                }
                S[(size_t)a * lds + b] = v;
                if (a != b) S[(size_t)b * lds + a] = v;
            }
}

int launch_cov_kstar(const KParams &kp, const double *Xp, int N, int Npad, int DP, const double *Q, int m, int mp, double *Kt,
                     hipStream_t s)
{
    hipLaunchKernelGGL(cov_kstar_kernel, dim3((Npad + 255) / 256, mp), dim3(256), 0, s, kp, Xp, N, Npad, DP, Q, m, Kt);
    return (int)hipGetLastError();
}

int launch_cov_tri(const double *A, size_t lda, const double *B, size_t ldb, int nvalid, int rows, int ncols, double *C, size_t ldc,
                   hipStream_t s)
{
    const int nbn = ncols / 64;
    hipLaunchKernelGGL(cov_tri_kernel, dim3(nbn, rows / 64), dim3(256), 0, s, A, lda, B, ldb, nvalid, nbn, C, ldc);
    return (int)hipGetLastError();
}

int launch_cov_syrk(const KParams &kp, const double *Q, const double *Vt, size_t ldv, int K, int M, int Mp, double diag, int pad,
                    double *S, size_t lds, hipStream_t s)
{
    const int nt = Mp / 64;
    hipLaunchKernelGGL(cov_syrk_kernel, dim3(nt * (nt + 1) / 2), dim3(256), 0, s, kp, Q, Vt, ldv, K, M, Mp, diag, pad, S, lds);
    return (int)hipGetLastError();
}

void ibo_touch_cov() { hipFuncAttributes a; (void)hipFuncGetAttributes(&a, (const void *)cov_syrk_kernel); }     // (see small2.hip: ibo_touch_small2)

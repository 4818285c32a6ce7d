// sparse.hip -- the inducing-point GP's kernels (ibo_sgp_*): N observations into the m x m Gram matrix of their scaled cross-covariance.
//
//   sgp_scaled_kuf_kernel  a chunk of observations -> Ft = [F ; 0 ; y~ ; 0], contraction-major.  One lane per observation, SGP_ROWS inducing
//                          rows per workgroup: the observation's coordinates are read once per workgroup and dimension, the inducing rows
//                          come from LDS (a broadcast), the exponent is the difference form of cov_matrix_kernel (subtract, then scale) and
//                          k* goes through cov_from_z_fast -- one exp_fast, and one sqrt_fast for the Matern families, per entry.  Nothing is
//                          summed over the observations here: a column's bits depend on its own point alone.  The workgroups of the targets'
//                          row also leave lambda and the chunk's two sums, per 256 observations in one fixed tree order.
//   sgp_gram_kernel        G+ += Ft Ft^T on v_mfma_f64_16x16x4_f64 through cv_tile<false> (cov_dev.h): one lower 64 x 64 tile per workgroup,
//                          the accumulators loaded from G+ and continued in ascending observation order -- the bits of G, b and y~.y~ do not
//                          depend on how the data were cut into chunks (a short last chunk's zero columns add +0).
//   sgp_assemble_kernel    A = K~uu + G, both triangles from one sum; b into the frame's targets.
//   sgp_finish_kernel      one candidate per lane (as cacq_finish_kernel): the composed variance, the clip, acq_value_dev, the exclusion
//                          balls, one arg-max partial per workgroup.
// Vector stores and plain C++ only.
#include "sparse.h"
#include "cov_dev.h"

template <int FAM>
__global__ __launch_bounds__(256) void sgp_scaled_kuf_kernel(SgpKufArgs a)
{
    __shared__ double zs[SGP_ROWS][IBO_DMAX];
    __shared__ double red[2][256];
    const int t = threadIdx.x, D = a.kp.D;
    const int a0 = blockIdx.y * SGP_ROWS;
    const int i = blockIdx.x * 256 + t;
    const bool frow = a0 < a.mp;                              // rows of F (or its pad); otherwise the targets' tile
    if (frow)
        for (int e = t; e < SGP_ROWS * D; e += 256) {
            const int r = e / D, d = e - r * D;
            zs[r][d] = (a0 + r < a.m) ? a.Z[(size_t)(a0 + r) * a.ldz + d] : 0.0;
        }
    __syncthreads();
    const bool live = i < a.n;
    double excess = 0.0, lam = 1.0;
    if (live) {
        if (a.s2u) { excess = a.s2u[i] - a.jitter; excess = excess > 0.0 ? excess : 0.0; }
        lam = a.fitc ? a.noise + excess : a.noise;
    }
    const double rs = 1.0 / sqrt(lam);
    if (frow) {
        if (i >= a.ld) return;
        double z[SGP_ROWS];
#pragma unroll
        for (int r = 0; r < SGP_ROWS; r++) z[r] = 0.0;
        if (live)
            for (int d = 0; d < D; d++) {
                const double xd = a.X[(size_t)i * D + d], w = a.kp.w[d];
#pragma unroll
                for (int r = 0; r < SGP_ROWS; r++) { const double u = zs[r][d] - xd; z[r] = fma(w * u, u, z[r]); }
            }
        const double log_sf2 = log(a.kp.sf2);
#pragma unroll
        for (int r = 0; r < SGP_ROWS; r++) {
            const double k = (live && a0 + r < a.m) ? cov_from_z_fast<FAM>(z[r], log_sf2, a.kp.sf2) * rs : 0.0;
            a.Ft[(size_t)(a0 + r) * a.ld + i] = k;
        }
        return;
    }
    // the targets' tile: row mp holds y~, the 63 rows below it are zero
    if (i < a.ld) {
#pragma unroll
        for (int r = 0; r < SGP_ROWS; r++) a.Ft[(size_t)(a0 + r) * a.ld + i] = (a0 == a.mp && r == 0 && live) ? a.Y[i] * rs : 0.0;
    }
    if (a0 != a.mp) return;                                    // (block-uniform)
    if (live && a.lam) a.lam[i] = lam;
    red[0][t] = live ? log(lam) : 0.0;
    red[1][t] = live ? excess : 0.0;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {                        // one fixed tree: the sums do not depend on the launch
        if (t < o) { red[0][t] += red[0][t + o]; red[1][t] += red[1][t + o]; }
        __syncthreads();
    }
    if (t == 0) { a.part[blockIdx.x] = red[0][0]; a.part[gridDim.x + blockIdx.x] = red[1][0]; }
}

int launch_sgp_scaled_kuf(const SgpKufArgs &a, hipStream_t s)
{
    if (a.n < 1 || a.ld < a.n || (a.ld & 31) || (a.mp & 63) || a.m < 1 || a.m > a.mp || a.kp.D < 1 || a.kp.D > IBO_DMAX) return (int)hipErrorInvalidValue;
    const dim3 grid((unsigned)((a.n + 255) / 256), (unsigned)((a.mp + 64) / SGP_ROWS));
    if (a.kp.family == FAM_SE) hipLaunchKernelGGL(sgp_scaled_kuf_kernel<FAM_SE>, grid, dim3(256), 0, s, a);
    else if (a.kp.family == FAM_M3) hipLaunchKernelGGL(sgp_scaled_kuf_kernel<FAM_M3>, grid, dim3(256), 0, s, a);
    else hipLaunchKernelGGL(sgp_scaled_kuf_kernel<FAM_M5>, grid, dim3(256), 0, s, a);
    return (int)hipGetLastError();
}

// one lower 64 x 64 tile (bm >= bn) per workgroup, blockIdx.x = bm (bm + 1) / 2 + bn (cov_syrk_kernel's order)
__global__ __launch_bounds__(256) void sgp_gram_kernel(const double *__restrict__ Ft, size_t ld, int kend, double *__restrict__ G, size_t ldg)
{
    __shared__ double As[64 * CV_LD], Bs[64 * CV_LD];
    const int t = blockIdx.x;
    int bm = (int)((sqrt(8.0 * t + 1.0) - 1.0) * 0.5);
    while ((bm + 1) * (bm + 2) / 2 <= t) bm++;
    while (bm * (bm + 1) / 2 > t) bm--;
    const int bn = t - bm * (bm + 1) / 2;
    const int r0 = bm * 64, n0 = bn * 64;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, wr = wv >> 1, wc = wv & 1;
    d4_t acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; i++)
#pragma unroll
        for (int j = 0; j < 2; j++)
#pragma unroll
            for (int e = 0; e < 4; e++) {
                const int r = r0 + 32 * wr + 16 * i + (lane >> 4) + 4 * e, n = n0 + 32 * wc + 16 * j + (lane & 15);
                acc[i][j][e] = G[(size_t)r * ldg + n];
            }
    cv_tile<false>(Ft, ld, Ft, ld, r0, n0, kend, 0, acc, As, Bs);
#pragma unroll
    for (int i = 0; i < 2; i++)
#pragma unroll
        for (int j = 0; j < 2; j++)
#pragma unroll
            for (int e = 0; e < 4; e++) {
                const int r = r0 + 32 * wr + 16 * i + (lane >> 4) + 4 * e, n = n0 + 32 * wc + 16 * j + (lane & 15);
                G[(size_t)r * ldg + n] = acc[i][j][e];
            }
}

int launch_sgp_gram(const double *Ft, int ld, int mp, double *G, hipStream_t s)
{
    if (ld < 32 || (ld & 31) || mp < 64 || (mp & 63)) return (int)hipErrorInvalidValue;
    const int nt = (mp + 64) / 64;
    hipLaunchKernelGGL(sgp_gram_kernel, dim3(nt * (nt + 1) / 2), dim3(256), 0, s, Ft, (size_t)ld, ld, G, (size_t)(mp + 64));
    return (int)hipGetLastError();
}

__global__ __launch_bounds__(256) void sgp_assemble_kernel(const double *__restrict__ Kuu, int ldk, const double *__restrict__ G, int ldg, int m, int mp,
                                                           int Np, double *__restrict__ A, double *__restrict__ Y)
{
    const int b = blockIdx.x * 16 + (threadIdx.x & 15), r = blockIdx.y * 16 + (threadIdx.x >> 4);
    if (blockIdx.y == 0 && (threadIdx.x >> 4) == 0)
        for (int c = b; c < Np; c += gridDim.x * 16) Y[c] = c < m ? G[(size_t)mp * ldg + c] : 0.0;
    if (r >= m || b > r) return;
    const double v = Kuu[(size_t)r * ldk + b] + G[(size_t)r * ldg + b];
    A[(size_t)r * m + b] = v;
    if (b != r) A[(size_t)b * m + r] = v;
}

int launch_sgp_assemble(const double *Kuu, int ldk, const double *G, int ldg, int m, int mp, int Np, double *A, double *Y, hipStream_t s)
{
    if (m < 1 || m > mp || Np < m) return (int)hipErrorInvalidValue;
    const unsigned nb = (unsigned)((m + 15) / 16);
    hipLaunchKernelGGL(sgp_assemble_kernel, dim3(nb, nb), dim3(256), 0, s, Kuu, ldk, G, ldg, m, mp, Np, A, Y);
    return (int)hipGetLastError();
}

// NaN values and excluded candidates never win the arg-max (block256_argmax's rule)
__global__ __launch_bounds__(256) void sgp_finish_kernel(SgpFinishArgs a)
{
    const int64_t li = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const bool valid = li < a.t.M;
    const int64_t gi = valid ? li : a.t.M - 1;
    const double mu = a.mua[gi];
    // sigma^2 + (1 - q_U) + q_A in exactly this order; additions only, so there is nothing to contract
    const double du = a.s2u[gi] - a.jitter, da = 1.0 - a.s2a[gi];
    double s2 = (a.noise + du) + da;
    if (s2 < a.clamp_lo) s2 = a.clamp_lo;                     // (a NaN passes both clamps)
    else if (s2 > 10.0) s2 = 10.0;
    double val = (a.acq == 3) ? mu : acq_value_dev(a.acq, a.erf_mode, mu, sqrt(s2), a.ymax, a.parm);
    finish_tail<true>(a.t, li, val, [&] {
        if (a.out_mu) a.out_mu[li] = mu;
        if (a.out_s2) a.out_s2[li] = s2;
        if (a.out_acq) a.out_acq[li] = val;
    });
}

int launch_sgp_finish(const SgpFinishArgs &a, hipStream_t s)
{
    if (!finish_tail_ok(a.t)) return (int)hipErrorInvalidValue;
    const int64_t nblk = (a.t.M + 255) / 256;
    hipLaunchKernelGGL(sgp_finish_kernel, dim3((unsigned)nblk), dim3(256), 0, s, a);
    return (int)hipGetLastError();
}

void ibo_touch_sparse() { hipFuncAttributes a; (void)hipFuncGetAttributes(&a, (const void *)sgp_finish_kernel); }     // (see small2.hip: ibo_touch_small2)

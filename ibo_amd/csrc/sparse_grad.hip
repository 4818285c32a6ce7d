// sparse_grad.hip -- the sparse GP's marginal-likelihood gradient (ibo_sgp_nlml_grad): one more pass over the observations after the fit.
//
//   sgp_grad_obs_kernel       one lane per observation: lambda_i, c_i = dNL/dlambda_i, e_i, r_i from the two frames' plain sweeps; sum c_i per
//                             256 observations in the fixed tree of sgp_scaled_kuf_kernel.
//   sgp_grad_gen_kernel       the chunk's operands from k_ai (the fit's generation: difference form, cov_from_z_fast): the observation-major
//                             column operand [k_i / lambda_i | -2 e_i k_i] and, for the signed Gram product, contraction-major k and e k.
//   sgp_grad_contract_kernel  a 64 x 64 tile of g = dNL/dK on v_mfma_f64_16x16x4_f64 through cv_tile -- [A^-1 | K~uu^-1] against the column
//                             operand, a contraction of length 2 mp (mp for DTC) -- and the derivative epilogue WITHOUT storing g: the tile goes
//                             to LDS (over the product's staging), every thread takes one inducing row and 16 observations, forms z, k and
//                             rho = dk/dz (one exp_fast, one sqrt_fast for the Matern families), keeps h = g rho in registers and loops over the
//                             dimensions: sum h Delta_d and sum h Delta_d^2, added across the row's four threads in one order and into the
//                             workgroup's own partial rows.  A workgroup owns 64 inducing rows and a strip of tiles in ascending order.  The
//                             same kernel contracts S = dNL/dK~uu with Z in the role of the observations (FROM_S).
//   sgp_grad_reduce_kernel    the strips' partials in ascending order.
//   sgp_abt_kernel            C (+)= A B^T, one 64 x 64 tile per workgroup (cv_tile): the signed Gram matrix H = (K E) K^T over the chunks and
//                             the two m^3 products of K~uu^-1 H K~uu^-1.  sgp_gram_kernel is untouched.
//   sgp_grad_S_kernel         S from A^-1, K~uu^-1, alpha and that product.
// No atomics anywhere: every sum has one order.  Vector stores and plain C++ only.
#include "sparse_grad.h"
#include "sparse.h"
#include "cov_dev.h"

__global__ __launch_bounds__(256) void sgp_grad_obs_kernel(SgpGradObsArgs a)
{
    __shared__ double red[256];
    const int t = threadIdx.x, i = blockIdx.x * 256 + t;
    const bool live = i < a.n;
    double lam = 1.0, e = 0.0, r = 0.0, c = 0.0;
    if (live) {
        double excess = a.s2u[i] - a.jitter;
        excess = excess > 0.0 ? excess : 0.0;                 // (the fit's lambda, bit for bit)
        const bool pos = excess > 0.0;
        lam = a.kind == SGP_GRAD_FITC ? a.noise + excess : a.noise;
        const double mu = a.mua[i], ai = 1.0 - a.s2a[i], y = a.Y[i], il = 1.0 / lam, d = y - mu;
        c = 0.5 * (il - fma(d, d, ai) * il * il);
        if (a.kind == SGP_GRAD_FITC) e = pos ? c : 0.0;
        else if (a.kind == SGP_GRAD_VFE) e = pos ? 0.5 / a.noise : 0.0;
        r = (mu - y) * il;
    }
    if (i < a.ld) { a.lam[i] = lam; a.ev[i] = e; a.rv[i] = r; }
    red[t] = c;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (t < o) red[t] += red[t + o];
        __syncthreads();
    }
    if (t == 0) a.part[blockIdx.x] = red[0];
}

int launch_sgp_grad_obs(const SgpGradObsArgs &a, hipStream_t s)
{
    if (a.n < 1 || a.ld < a.n || (a.ld & 63)) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(sgp_grad_obs_kernel, dim3((unsigned)((a.ld + 255) / 256)), dim3(256), 0, s, a);
    return (int)hipGetLastError();
}

template <int FAM>
__global__ __launch_bounds__(256) void sgp_grad_gen_kernel(SgpGradGenArgs a)
{
    __shared__ double zs[SGP_ROWS][IBO_DMAX];
    const int t = threadIdx.x, D = a.kp.D;
    const int a0 = blockIdx.y * SGP_ROWS;
    const int i = blockIdx.x * 256 + t;
    for (int e = t; e < SGP_ROWS * D; e += 256) {
        const int r = e / D, d = e - r * D;
        zs[r][d] = (a0 + r < a.m) ? a.Z[(size_t)(a0 + r) * a.ldz + d] : 0.0;
    }
    __syncthreads();
    if (i >= a.ld) return;
    const bool live = i < a.n;
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
    const double il = 1.0 / a.lam[i], ei = a.ev[i];
    double *bo = a.Bo + (size_t)i * a.ldb + a0;
#pragma unroll
    for (int r = 0; r < SGP_ROWS; r++) {
        const double k = (live && a0 + r < a.m) ? cov_from_z_fast<FAM>(z[r], log_sf2, a.kp.sf2) : 0.0;
        bo[r] = k * il;
        if (a.two) bo[a.mp + r] = -2.0 * ei * k;
        if (a.Kt) { a.Kt[(size_t)(a0 + r) * a.ld + i] = k; a.KEt[(size_t)(a0 + r) * a.ld + i] = ei * k; }
    }
}

int launch_sgp_grad_gen(const SgpGradGenArgs &a, hipStream_t s)
{
    if (a.n < 1 || a.ld < a.n || (a.ld & 63) || (a.mp & 63) || a.m < 1 || a.m > a.mp || a.kp.D < 1 || a.kp.D > IBO_DMAX || a.ldb < (a.two ? 2 : 1) * a.mp || (a.ldb & 1)
        || (!a.Kt) != (!a.KEt))
        return (int)hipErrorInvalidValue;
    const dim3 grid((unsigned)((a.ld + 255) / 256), (unsigned)(a.mp / SGP_ROWS));
    if (a.kp.family == FAM_SE) hipLaunchKernelGGL(sgp_grad_gen_kernel<FAM_SE>, grid, dim3(256), 0, s, a);
    else if (a.kp.family == FAM_M3) hipLaunchKernelGGL(sgp_grad_gen_kernel<FAM_M3>, grid, dim3(256), 0, s, a);
    else hipLaunchKernelGGL(sgp_grad_gen_kernel<FAM_M5>, grid, dim3(256), 0, s, a);
    return (int)hipGetLastError();
}

// rho = dk/dz from k and z: finite at z = 0 (gradobs.hip's forms)
template <int FAM>
__device__ __forceinline__ double sgp_rho(double z, double k)
{
    if (FAM == FAM_SE) return -0.5 * k;
    if (FAM == FAM_M3) { const double r = sqrt_fast(3.0 * z); return -1.5 * k / (1.0 + r); }
    const double r = sqrt_fast(5.0 * z);
    return -(5.0 / 6.0) * k * (1.0 + r) / fma(r, fma(r, 1.0 / 3.0, 1.0), 1.0);
}

#define SGP_GT_LD 65             // the g tile's row stride in LDS

template <int FAM, bool FROM_S>
__global__ __launch_bounds__(256) void sgp_grad_contract_kernel(SgpGradArgs a)
{
    __shared__ double AB[2 * 64 * CV_LD];                     // cv_tile's two stages; afterwards the g tile (64 x SGP_GT_LD fits)
    __shared__ double Xs[64 * IBO_DMAX];                      // the tile's observations, 64 x D
    double *As = AB, *Bs = AB + 64 * CV_LD, *gt = AB;
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6, wr = wv >> 1, wc = wv & 1;
    const int D = a.kp.D, r0 = blockIdx.x * 64, strip = blockIdx.y;
    const int row = t >> 2, sub = t & 3;                      // the epilogue: inducing row r0 + row, observations 16 sub .. 16 sub + 15 of the tile
    const bool rowlive = r0 + row < a.m;
    const double *zrow = a.Z + (size_t)(rowlive ? r0 + row : 0) * a.ldz;
    const double log_sf2 = log(a.kp.sf2);
    double *pZ = a.partZ + ((size_t)strip * a.mp + r0 + row) * D, *pL = a.partL + ((size_t)strip * a.mp + r0 + row) * D;
    double sgk = 0.0;
    const int t0 = strip * a.tiles_per_strip, t1 = min(a.ntiles, t0 + a.tiles_per_strip);
    for (int tile = t0; tile < t1; tile++) {
        const int n0 = tile * 64;
        if (!FROM_S) {
            d4_t acc[2][2];
#pragma unroll
            for (int i = 0; i < 2; i++)
#pragma unroll
                for (int j = 0; j < 2; j++) acc[i][j] = (d4_t){0.0, 0.0, 0.0, 0.0};
            cv_tile<false>(a.Ainv, (size_t)a.ldi, a.Bo, (size_t)a.ldb, r0, n0, a.mp, 0, acc, As, Bs);
            if (a.two) cv_tile<false>(a.Uinv, (size_t)a.ldi, a.Bo + a.mp, (size_t)a.ldb, r0, n0, a.mp, 0, acc, As, Bs);
            // (cv_tile ends behind a barrier: the stages are free)
#pragma unroll
            for (int i = 0; i < 2; i++)
#pragma unroll
                for (int j = 0; j < 2; j++)
#pragma unroll
                    for (int e = 0; e < 4; e++) {
                        const int r = 32 * wr + 16 * i + (lane >> 4) + 4 * e, n = 32 * wc + 16 * j + (lane & 15);
                        gt[r * SGP_GT_LD + n] = fma(a.alpha[r0 + r], a.rv[n0 + n], acc[i][j][e]);
                    }
        } else {
            for (int e = t; e < 4096; e += 256) {
                const int r = e >> 6, n = e & 63;
                gt[r * SGP_GT_LD + n] = a.S[(size_t)(r0 + r) * a.lds + n0 + n];
            }
        }
        for (int e = t; e < 64 * D; e += 256) {
            const int i = e / D, d = e - i * D;
            Xs[e] = (n0 + i < a.n) ? a.X[(size_t)(n0 + i) * a.ldx + d] : 0.0;
        }
        __syncthreads();
        double h[16];
        {
            double z[16];
#pragma unroll
            for (int j = 0; j < 16; j++) z[j] = 0.0;
            for (int d = 0; d < D; d++) {
                const double zd = zrow[d], w = a.kp.w[d];
#pragma unroll
                for (int j = 0; j < 16; j++) { const double u = zd - Xs[(16 * sub + j) * D + d]; z[j] = fma(w * u, u, z[j]); }
            }
#pragma unroll
            for (int j = 0; j < 16; j++) {
                const double g = rowlive ? gt[row * SGP_GT_LD + 16 * sub + j] : 0.0;
                const double k = cov_from_z_fast<FAM>(z[j], log_sf2, a.kp.sf2);
                h[j] = g * sgp_rho<FAM>(z[j], k);
                sgk = fma(g, k, sgk);
            }
        }
        for (int d = 0; d < D; d++) {
            const double zd = zrow[d];
            double s1 = 0.0, s2 = 0.0;
#pragma unroll
            for (int j = 0; j < 16; j++) {
                const double u = zd - Xs[(16 * sub + j) * D + d], hu = h[j] * u;
                s1 += hu;
                s2 = fma(hu, u, s2);
            }
            s1 += __shfl_xor(s1, 1); s1 += __shfl_xor(s1, 2);           // the row's four threads: (0 + 1) + (2 + 3) in every lane
            s2 += __shfl_xor(s2, 1); s2 += __shfl_xor(s2, 2);
            if (sub == 0 && rowlive) { pZ[d] += s1; pL[d] += s2; }     // this workgroup's own rows of its strip's partials
        }
        __syncthreads();                                      // the next tile's product stages over gt and Xs
    }
    AB[t] = sgk;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (t < o) AB[t] += AB[t + o];
        __syncthreads();
    }
    if (t == 0) a.partS[(size_t)strip * gridDim.x + blockIdx.x] = AB[0];
}

int launch_sgp_grad_contract(const SgpGradArgs &a, int from_S, hipStream_t s)
{
    if (a.m < 1 || a.m > a.mp || (a.mp & 63) || a.kp.D < 1 || a.kp.D > IBO_DMAX || a.ntiles < 1 || a.tiles_per_strip < 1
        || (int64_t)a.nstrips * a.tiles_per_strip < a.ntiles || a.nstrips < 1 || a.nstrips > 65535)
        return (int)hipErrorInvalidValue;
    if (from_S ? (!a.S || a.lds < a.ntiles * 64) : (!a.Ainv || !a.Bo || a.ldi < a.mp || a.ldb < (a.two ? 2 : 1) * a.mp || (a.ldb & 1) || (a.ldi & 1) || (a.two && !a.Uinv)))
        return (int)hipErrorInvalidValue;
    const dim3 grid((unsigned)(a.mp / 64), (unsigned)a.nstrips);
#define SGP_GRAD_LAUNCH(F) \
    do { if (from_S) hipLaunchKernelGGL((sgp_grad_contract_kernel<F, true>), grid, dim3(256), 0, s, a); \
         else hipLaunchKernelGGL((sgp_grad_contract_kernel<F, false>), grid, dim3(256), 0, s, a); } while (0)
    if (a.kp.family == FAM_SE) SGP_GRAD_LAUNCH(FAM_SE);
    else if (a.kp.family == FAM_M3) SGP_GRAD_LAUNCH(FAM_M3);
    else SGP_GRAD_LAUNCH(FAM_M5);
#undef SGP_GRAD_LAUNCH
    return (int)hipGetLastError();
}

__global__ __launch_bounds__(256) void sgp_grad_reduce_kernel(const double *__restrict__ partZ, const double *__restrict__ partL, const double *__restrict__ partS,
                                                              int nstrips, int m, int mp, int D, double *__restrict__ totZ, double *__restrict__ totL, double *__restrict__ totS)
{
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e < (int64_t)m * D) {
        double sz = 0.0, sl = 0.0;
        for (int s = 0; s < nstrips; s++) { sz += partZ[(size_t)s * mp * D + e]; sl += partL[(size_t)s * mp * D + e]; }
        totZ[e] += sz; totL[e] += sl;
    }
    if (e == 0) {
        double ss = 0.0;
        for (int s = 0; s < nstrips * (mp / 64); s++) ss += partS[s];
        totS[0] += ss;
    }
}

int launch_sgp_grad_reduce(const double *partZ, const double *partL, const double *partS, int nstrips, int m, int mp, int D,
                           double *totZ, double *totL, double *totS, hipStream_t s)
{
    if (nstrips < 1 || m < 1 || m > mp || D < 1) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(sgp_grad_reduce_kernel, dim3((unsigned)(((int64_t)m * D + 255) / 256)), dim3(256), 0, s, partZ, partL, partS, nstrips, m, mp, D, totZ, totL, totS);
    return (int)hipGetLastError();
}

// one 64 x 64 tile per workgroup; lower_only: blockIdx.x = bm (bm + 1) / 2 + bn (sgp_gram_kernel's order)
__global__ __launch_bounds__(256) void sgp_abt_kernel(const double *__restrict__ A, size_t lda, const double *__restrict__ B, size_t ldb,
                                                      double *__restrict__ C, size_t ldc, int nt, int kend, int accumulate, int lower_only)
{
    __shared__ double As[64 * CV_LD], Bs[64 * CV_LD];
    const int t = blockIdx.x;
    int bm, bn;
    if (lower_only) {
        bm = (int)((sqrt(8.0 * t + 1.0) - 1.0) * 0.5);
        while ((bm + 1) * (bm + 2) / 2 <= t) bm++;
        while (bm * (bm + 1) / 2 > t) bm--;
        bn = t - bm * (bm + 1) / 2;
    } else { bm = t / nt; bn = t - bm * nt; }
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
                acc[i][j][e] = accumulate ? C[(size_t)r * ldc + n] : 0.0;
            }
    cv_tile<false>(A, lda, B, ldb, r0, n0, kend, 0, acc, As, Bs);
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

int launch_sgp_abt(const double *A, int lda, const double *B, int ldb, double *C, int ldc, int rows, int kend, int accumulate, int lower_only, hipStream_t s)
{
    if (rows < 64 || (rows & 63) || kend < 32 || (kend & 31) || lda < kend || ldb < kend || ldc < rows || (lda & 1) || (ldb & 1)) return (int)hipErrorInvalidValue;
    const int nt = rows / 64;
    hipLaunchKernelGGL(sgp_abt_kernel, dim3((unsigned)(lower_only ? nt * (nt + 1) / 2 : nt * nt)), dim3(256), 0, s, A, (size_t)lda, B, (size_t)ldb, C, (size_t)ldc, nt, kend,
                       accumulate, lower_only);
    return (int)hipGetLastError();
}

__global__ __launch_bounds__(256) void sgp_mirror_kernel(double *__restrict__ H, int ld, int rows)
{
    const int b = blockIdx.x * 16 + (threadIdx.x & 15), r = blockIdx.y * 16 + (threadIdx.x >> 4);
    if (r >= rows || b >= r) return;
    H[(size_t)b * ld + r] = H[(size_t)r * ld + b];
}

int launch_sgp_mirror(double *H, int ld, int rows, hipStream_t s)
{
    if (rows < 1 || ld < rows) return (int)hipErrorInvalidValue;
    const unsigned nb = (unsigned)((rows + 15) / 16);
    hipLaunchKernelGGL(sgp_mirror_kernel, dim3(nb, nb), dim3(256), 0, s, H, ld, rows);
    return (int)hipGetLastError();
}

__global__ __launch_bounds__(256) void sgp_grad_S_kernel(const double *__restrict__ Ainv, const double *__restrict__ Uinv, int ldi, const double *__restrict__ alpha,
                                                         const double *__restrict__ M, int ldm, int m, int mp, double *__restrict__ S)
{
    const int b = blockIdx.x * 16 + (threadIdx.x & 15), r = blockIdx.y * 16 + (threadIdx.x >> 4);
    if (r >= mp || b >= mp) return;
    double v = 0.0;
    if (r < m && b < m && r != b) {
        v = 0.5 * ((Ainv[(size_t)r * ldi + b] + alpha[r] * alpha[b]) - Uinv[(size_t)r * ldi + b]);
        if (M) v += 0.5 * (M[(size_t)r * ldm + b] + M[(size_t)b * ldm + r]);
    }
    S[(size_t)r * mp + b] = v;
}

int launch_sgp_grad_S(const double *Ainv, const double *Uinv, int ldi, const double *alpha, const double *M, int ldm, int m, int mp, double *S, hipStream_t s)
{
    if (m < 1 || m > mp || ldi < mp || (M && ldm < mp)) return (int)hipErrorInvalidValue;
    const unsigned nb = (unsigned)((mp + 15) / 16);
    hipLaunchKernelGGL(sgp_grad_S_kernel, dim3(nb, nb), dim3(256), 0, s, Ainv, Uinv, ldi, alpha, M, ldm, m, mp, S);
    return (int)hipGetLastError();
}

void ibo_touch_sparse_grad() { hipFuncAttributes a; (void)hipFuncGetAttributes(&a, (const void *)sgp_grad_S_kernel); }     // (see small2.hip: ibo_touch_small2)

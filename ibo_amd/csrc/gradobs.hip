// gradobs.hip -- the derivative covariance of a GP observed with gradients (ibo_ggp_*): rows in point-major order, see gradobs.h.
//
//   gradobs_assemble_kernel  A = [K, dK/dx'; dK/dx, d2K/dx dx'] with its diagonal rule, in the identity-padded frame of the factorisation.
//                            One workgroup per tile of 16 x 16 point pairs: the pair's three factors (one exp, one sqrt for Matern) go to
//                            LDS once, then the tile's 16 (D + 1) x 16 (D + 1) entries are formed from them and stored row by row
//                            (consecutive lanes, consecutive columns)
//   gradobs_kstar_kernel     Kt = K*(Q, data) of a chunk of query points, query-major, zero in the pad: one workgroup per query point and
//                            256 data points -- two factors per (query, point) to LDS, then the 256 (D + 1) entries in column order
//   gradobs_acq_kernel       EI / PI / UCB from (mu, s2) by acq_value_dev, the sweeps' epilogue formula
// Both covariance kernels are exp- and store-bound; nothing here sums anything, so a row's bits depend on its own points alone.
#include "gradobs.h"

#define GO_TP 16                 // points per side of an assemble tile (256 pairs: one per thread)
#define GO_KP 256                // data points per workgroup of the k* kernel

// the three factors of one point pair from z = sum_d w_d u_d^2 (gradobs.h); k is cov_from_z's expression
__device__ __forceinline__ void go_factors(int fam, double z, double sf2, double *k, double *g1, double *g2)
{
    if (fam == FAM_SE) { const double e = sf2 * exp(-0.5 * z); *k = e; *g1 = e; *g2 = e; return; }
    if (fam == FAM_M3) {
        const double r = sqrt(3.0 * z), e = exp(-r);
        *k = sf2 * (1.0 + r) * e;
        *g1 = 3.0 * sf2 * e;
        *g2 = r > 0.0 ? 3.0 * *g1 / r : 0.0;          // (the second-derivative term vanishes at r = 0: t_d t_e / r -> 0)
        return;
    }
    const double r = sqrt(5.0 * z), e = exp(-r);
    *k = sf2 * (1.0 + r + r * r * (1.0 / 3.0)) * e;
    *g1 = (5.0 / 3.0) * sf2 * (1.0 + r) * e;
    *g2 = (25.0 / 3.0) * sf2 * e;
}

__global__ void __launch_bounds__(256) gradobs_assemble_kernel(KParams kp, const double *__restrict__ X, int N, double noise,
                                                               const double *__restrict__ gnoise, double *__restrict__ A, int Np)
{
    __shared__ double xr[GO_TP * IBO_DMAX], xc[GO_TP * IBO_DMAX], ws[IBO_DMAX], fk[256], f1[256], f2[256];
    const int D = kp.D, B = D + 1, tid = threadIdx.x;
    const int i0 = blockIdx.y * GO_TP, j0 = blockIdx.x * GO_TP;
    const size_t P = (size_t)N * B;
    for (int e = tid; e < GO_TP * D; e += 256) {
        const int p = e / D, d = e - p * D;
        xr[e] = i0 + p < N ? X[(size_t)(i0 + p) * D + d] : 0.0;
        xc[e] = j0 + p < N ? X[(size_t)(j0 + p) * D + d] : 0.0;
    }
    if (tid < D) ws[tid] = kp.w[tid];
    __syncthreads();
    {
        const int pi = tid >> 4, pj = tid & 15;
        go_factors(kp.family, wsqdist_dev(ws, xr + pi * D, xc + pj * D, D), kp.sf2, &fk[tid], &f1[tid], &f2[tid]);
    }
    __syncthreads();
    const int R = GO_TP * B;                            // the tile is R x R entries
    for (int e = tid; e < R * R; e += 256) {
        const int r = e / R, c = e - r * R;
        const size_t gr = (size_t)i0 * B + r, gc = (size_t)j0 * B + c;
        if (gr >= (size_t)Np || gc >= (size_t)Np) continue;
        double v = gr == gc ? 1.0 : 0.0;                // the pad: identity
        if (gr < P && gc < P) {
            const int pi = r / B, a = r - pi * B, pj = c / B, b = c - pj * B, f = pi * GO_TP + pj;
            const double ta = a ? ws[a - 1] * (xr[pi * D + a - 1] - xc[pj * D + a - 1]) : 0.0;
            const double tb = b ? ws[b - 1] * (xr[pi * D + b - 1] - xc[pj * D + b - 1]) : 0.0;
            if (a == 0) v = b == 0 ? fk[f] : f1[f] * tb;
            else if (b == 0) v = -(f1[f] * ta);
            else {
                const double tt = ta * tb;              // first: (a, b) here and (b, a) of the mirrored pair are the same bits
                v = fma(-f2[f], tt, a == b ? f1[f] * ws[a - 1] : 0.0);
            }
            if (gr == gc) v = a == 0 ? 1.0 + noise : v + gnoise[a - 1];
        }
        A[gr * (size_t)Np + gc] = v;
    }
}

__global__ void __launch_bounds__(256) gradobs_kstar_kernel(KParams kp, const double *__restrict__ X, int N, int Pp,
                                                            const double *__restrict__ Q, int m, double *__restrict__ Kt)
{
    __shared__ double qs[IBO_DMAX], ws[IBO_DMAX], fk[GO_KP], f1[GO_KP];
    const int c = blockIdx.y, D = kp.D, B = D + 1, tid = threadIdx.x, j0 = blockIdx.x * GO_KP;
    if (tid < D) { qs[tid] = c < m ? Q[(size_t)c * D + tid] : 0.0; ws[tid] = kp.w[tid]; }
    __syncthreads();
    double k = 0.0, g1 = 0.0, g2;
    if (c < m && j0 + tid < N) go_factors(kp.family, wsqdist_dev(ws, qs, X + (size_t)(j0 + tid) * D, D), kp.sf2, &k, &g1, &g2);
    fk[tid] = k; f1[tid] = g1;
    __syncthreads();
    const size_t col0 = (size_t)j0 * B;
    double *row = Kt + (size_t)c * Pp;
    for (int e = tid; e < GO_KP * B; e += 256) {
        if (col0 + e >= (size_t)Pp) break;
        const int p = e / B, d = e - p * B, j = j0 + p;
        double v = 0.0;
        if (c < m && j < N) v = d == 0 ? fk[p] : f1[p] * (ws[d - 1] * (qs[d - 1] - X[(size_t)j * D + d - 1]));
        row[col0 + e] = v;
    }
}

__global__ void __launch_bounds__(256) gradobs_acq_kernel(int acq, int erf_mode, double ymax, double parm, const double *__restrict__ mu,
                                                          const double *__restrict__ s2, int m, double *__restrict__ out,
                                                          double *__restrict__ mu_out, double *__restrict__ s2_out)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= m) return;
    const double u = mu[i], v = s2[i];
    if (out) out[i] = acq == 3 ? u : acq_value_dev(acq, erf_mode, u, sqrt(v), ymax, parm);
    if (mu_out) mu_out[i] = u;
    if (s2_out) s2_out[i] = v;
}

int launch_gradobs_assemble(const KParams &kp, const double *X, int N, double noise, const double *gnoise, double *A, int Np, hipStream_t s)
{
    const int B = kp.D + 1;
    if (N < 1 || kp.D < 1 || kp.D > IBO_DMAX || (Np & 63) || (size_t)N * B > (size_t)Np) return (int)hipErrorInvalidValue;
    const int nt = ((Np + B - 1) / B + GO_TP - 1) / GO_TP;          // tiles of 16 points that cover the frame's Np rows
    hipLaunchKernelGGL(gradobs_assemble_kernel, dim3(nt, nt), dim3(256), 0, s, kp, X, N, noise, gnoise, A, Np);
    return (int)hipGetLastError();
}

int launch_gradobs_kstar(const KParams &kp, const double *X, int N, int Pp, const double *Q, int m, int mp, double *Kt, hipStream_t s)
{
    const int B = kp.D + 1;
    if (N < 1 || m < 1 || m > mp || mp > 65535 || kp.D < 1 || kp.D > IBO_DMAX || (size_t)N * B > (size_t)Pp) return (int)hipErrorInvalidValue;
    const int nbx = (Pp + GO_KP * B - 1) / (GO_KP * B);
    hipLaunchKernelGGL(gradobs_kstar_kernel, dim3(nbx, mp), dim3(256), 0, s, kp, X, N, Pp, Q, m, Kt);
    return (int)hipGetLastError();
}

int launch_gradobs_acq(int acq, int erf_mode, double ymax, double parm, const double *mu, const double *s2, int m, double *out,
                       double *mu_out, double *s2_out, hipStream_t s)
{
    if (m < 1) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(gradobs_acq_kernel, dim3((m + 255) / 256), dim3(256), 0, s, acq, erf_mode, ymax, parm, mu, s2, m, out, mu_out, s2_out);
    return (int)hipGetLastError();
}

void ibo_touch_gradobs() { hipFuncAttributes a; (void)hipFuncGetAttributes(&a, (const void *)gradobs_kstar_kernel); }     // (see small2.hip: ibo_touch_small2)

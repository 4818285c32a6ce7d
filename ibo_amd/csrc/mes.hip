// mes.hip -- max-value entropy search (ibo_mes_*): per candidate
//     MES = (1/K) sum_k h(gamma_k),   h(g) = g lambda(g) / 2 - log Phi(g),  lambda = phi / Phi,   gamma_k = (y*_k - mu) / sigma
// over the K sorted samples y*_k of the maximum, from the (mu, s2) pair the plain sweep left in device scratch (sigma^2 = max(s2 - s2_offset,
// clamp_lo)); then the exclusion balls, the optional per-candidate output and one (max, lowest index) partial per 256 candidates for
// launch_argmax_final.  And mes_maxcdf_kernel: sum_i log Phi((t - mu_i) / sigma_i) over a candidate set at up to 64 levels t, with the bracket
// [max mu, max (mu + 5 sigma)] -- what the Gumbel approximation of the maximum's distribution is fitted to.
//
// One candidate per lane, as ehvi.hip and for its reasons.  The work is K terms per candidate -- an erfc and an exp, or an erfcx and a log, in
// fp64 each: VALU and transcendental issue, nothing for the matrix unit -- against 16 bytes in and 8 out, so the only traffic that matters is
// the samples': they are staged once per workgroup into LDS (8 KiB at the limit of 1024), and in step k every lane reads the SAME double, which
// the LDS serves as a broadcast.  Each lane sums its own terms in ascending order: no cross-lane sum, and a candidate's bits depend on its
// (mu, s2) and the samples alone -- not on its lane, its chunk or the launch's size.
//
// 0.5 (1 + erf) (gauss_cdf_pdf_dev) holds Phi to an ABSOLUTE 1e-16, which loses log Phi below gamma = -8 (Phi itself underflows at -38) and
// above 8 (1 - Phi is rounded away); mes_terms takes Phi from its own tail on either side.
#include "mes.h"

#pragma clang fp contract(off)     // the sums below as written, in both variants: no fused multiply-add decides a bit of the value

// lambda = phi / Phi and nll = -log Phi at g, tail-safe on both sides (a NaN g takes the second branch and stays a NaN)
__device__ __forceinline__ void mes_terms(double g, double *lambda, double *nll)
{
    if (g >= 0.0) {
        const double q = 0.5 * erfc(g / sqrt(2.0));                  // 1 - Phi
        *lambda = (exp(-(g * g / 2.0)) / sqrt(2.0 * M_PI)) / (1.0 - q);
        *nll = -log1p(-q);
    } else {
        const double e = erfcx(-g / sqrt(2.0));                      // 2 Phi exp(g^2 / 2)
        *lambda = sqrt(2.0 / M_PI) / e;
        *nll = g * g / 2.0 - log(e / 2.0);
    }
}

// SUMS: also G_mu, G_sigma, sigma and the floor's flag (out_sums); the value's operations are the same ones.
template <bool SUMS>
__global__ __launch_bounds__(256) void mes_finish_kernel(MesArgs a)
{
    __shared__ double ys[IBO_MES_MAX_K];
    for (int k = threadIdx.x; k < a.K; k += 256) ys[k] = a.ystar[k];
    __syncthreads();
    const int64_t li = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const bool valid = li < a.t.M;
    const int64_t gi = valid ? li : a.t.M - 1;
    const double mu = a.ms[gi];
    double v = a.ms[(size_t)a.stride + gi] - a.s2_offset;
    const bool floored = v < a.clamp_lo;                             // (a NaN is not: it goes through)
    if (floored) v = a.clamp_lo;
    const double sigma = sqrt(v);
    double sum = 0.0, sd = 0.0, sdg = 0.0;
    for (int k = 0; k < a.K; k++) {
        const double g = (ys[k] - mu) / sigma;
        double lam, nll;
        mes_terms(g, &lam, &nll);
        sum = sum + (g * lam / 2.0 + nll);
        if (SUMS) {
            const double dh = -(lam / 2.0) * (1.0 + g * g + g * lam);
            sd = sd + dh;
            sdg = sdg + dh * g;
        }
    }
    double val = sum / (double)a.K;
    finish_tail<false>(a.t, li, val, [&] {
        if (a.out_val) a.out_val[li] = val;
        if (SUMS) {
            const size_t st = (size_t)a.sums_stride;
            a.out_sums[li] = -(sd / (double)a.K) / sigma; a.out_sums[st + li] = -(sdg / (double)a.K) / sigma;
            a.out_sums[2 * st + li] = sigma; a.out_sums[3 * st + li] = floored ? 0.0 : 1.0;
        }
    });
}

int launch_mes_finish(const MesArgs &a, bool sums, hipStream_t s)
{
    if (!finish_tail_ok(a.t) || a.t.M > a.stride || a.K < 1 || a.K > IBO_MES_MAX_K || !a.ystar || !a.ms || (sums && (!a.out_sums || a.sums_stride < a.t.M)))
        return (int)hipErrorInvalidValue;
    const int64_t nblk = (a.t.M + 255) / 256;
    hipLaunchKernelGGL(sums ? mes_finish_kernel<true> : mes_finish_kernel<false>, dim3((unsigned)nblk), dim3(256), 0, s, a);
    return (int)hipGetLastError();
}

// the sum of v over the workgroup's 256 lanes in a fixed tree (the wave's butterfly, then (w0 + w1) + (w2 + w3)); every lane returns it.
// MAX: the maximum instead.  buf: four doubles of LDS, free again when the call returns.
template <bool MAX>
__device__ __forceinline__ double mes_block256(double v, double *buf)
{
    for (int o = 32; o > 0; o >>= 1) {
        const double w = __shfl_xor(v, o);
        v = MAX ? (w > v ? w : v) : v + w;
    }
    if ((threadIdx.x & 63) == 0) buf[threadIdx.x >> 6] = v;
    __syncthreads();
    const double a = buf[0], b = buf[1], c = buf[2], d = buf[3];
    __syncthreads();
    if (MAX) { const double x = b > a ? b : a, y = d > c ? d : c; return y > x ? y : x; }
    return (a + b) + (c + d);
}

// One workgroup per 256 candidates; a candidate with a NaN posterior adds 0 to every sum and -inf to both maxima.
__global__ __launch_bounds__(256) void mes_maxcdf_kernel(MesCdfArgs a)
{
    __shared__ double lev[IBO_MES_MAX_LEV];
    __shared__ double buf[4];
    if ((int)threadIdx.x < a.nlev) lev[threadIdx.x] = a.lev[threadIdx.x];
    __syncthreads();
    const int64_t li = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t gi = li < a.M ? li : a.M - 1;
    const double mu = a.ms[gi];
    double v = a.ms[(size_t)a.stride + gi] - a.s2_offset;
    if (v < a.clamp_lo) v = a.clamp_lo;
    const double sigma = sqrt(v);
    const bool live = li < a.M && mu == mu && sigma == sigma;
    const double top = mes_block256<true>(live ? mu : -INFINITY, buf);
    const double ub = mes_block256<true>(live ? mu + 5.0 * sigma : -INFINITY, buf);
    if (threadIdx.x == 0) { a.part_mu[blockIdx.x] = top; a.part_ub[blockIdx.x] = ub; }
    for (int k = 0; k < a.nlev; k++) {
        double lam, nll = 0.0;
        if (live) mes_terms((lev[k] - mu) / sigma, &lam, &nll);
        const double sum = mes_block256<false>(-nll, buf);
        if (threadIdx.x == 0) a.part_sum[(size_t)blockIdx.x * a.nlev + k] = sum;
    }
}

int launch_mes_maxcdf(const MesCdfArgs &a, hipStream_t s)
{
    if (a.M < 1 || a.M > a.stride || a.nlev < 0 || a.nlev > IBO_MES_MAX_LEV || (a.nlev > 0 && (!a.lev || !a.part_sum)) || !a.ms || !a.part_mu || !a.part_ub)
        return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(mes_maxcdf_kernel, dim3((unsigned)((a.M + 255) / 256)), dim3(256), 0, s, a);
    return (int)hipGetLastError();
}

// thread k < nlev: level k's block sums added in ascending block order; threads nlev and nlev + 1: the two maxima
__global__ __launch_bounds__(128) void mes_maxcdf_final_kernel(const double *part_sum, const double *part_mu, const double *part_ub, int64_t nblk, int nlev,
                                                               double *out)
{
    const int k = threadIdx.x;
    if (k < nlev) {
        double s = 0.0;
        for (int64_t b = 0; b < nblk; b++) s = s + part_sum[(size_t)b * nlev + k];
        out[k] = s;
    } else if (k < nlev + 2) {
        const double *p = k == nlev ? part_mu : part_ub;
        double m = -INFINITY;
        for (int64_t b = 0; b < nblk; b++) m = p[b] > m ? p[b] : m;
        out[k] = m;
    }
}

int launch_mes_maxcdf_final(const double *part_sum, const double *part_mu, const double *part_ub, int64_t nblk, int nlev, double *out, hipStream_t s)
{
    if (nblk < 1 || nlev < 0 || nlev > IBO_MES_MAX_LEV || (nlev > 0 && !part_sum) || !part_mu || !part_ub || !out) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(mes_maxcdf_final_kernel, dim3(1), dim3(128), 0, s, part_sum, part_mu, part_ub, nblk, nlev, out);
    return (int)hipGetLastError();
}

void ibo_touch_mes() { hipFuncAttributes a; (void)hipFuncGetAttributes(&a, (const void *)mes_finish_kernel<false>); }     // (see small2.hip: ibo_touch_small2)

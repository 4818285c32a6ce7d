// ehvi.hip -- the strip scan of the two-objective expected hypervolume improvement (ibo_ehvi_*): per candidate
//     EHVI = sum_{i=0..n} max(psi_1(a_i) - psi_1(a_{i+1}), 0) psi_2(b_{i+1}),      psi(t) = sigma phi(u) + (mu - t) Phi(u),  u = (mu - t) / sigma
// over the canonical front (a_1, b_1) .. (a_n, b_n), a_0 = r1, psi_1(a_{n+1} = +inf) = 0, b_{n+1} = r2, from the (mu, s2) pairs the two
// per-model sweeps left in device scratch; then the exclusion balls, the optional per-candidate output and one (max, lowest index)
// partial per 256 candidates for launch_argmax_final.
//
// One candidate per lane.  The work is 2 (n + 1) cdf / pdf pairs per candidate -- an erf and an exp in fp64 each, VALU and transcendental
// issue, nothing for the matrix unit -- against 32 bytes in and 8 out, so the only traffic that matters is the front's: it is staged once
// per workgroup into LDS (16 bytes a point, 16 KiB at the limit of 1024), and in step i every lane reads the SAME pair, which the LDS
// serves as a broadcast (16 bytes per strip and wave -- the compiler reads them as one b128 or as two b64 -- no bank conflict).  A lane keeps psi_1(a_i) from the step before, so a
// strip costs one psi_1 and one psi_2; the sentinel at +inf is never evaluated.  Each lane sums its own strips in ascending order: no
// cross-lane sum, and a candidate's bits depend on its (mu, s2) and the front alone -- not on its lane, its chunk or the launch's size.
// A wavefront per candidate would spread the strips over 64 lanes, but then the sum's order would be the butterfly's, a front of three
// points would leave 60 lanes idle, and psi_1(a_i) would be evaluated twice per strip.
#include "ehvi.h"

#pragma clang fp contract(off)     // the sums below as written, in both variants: no fused multiply-add decides a bit of the value

// psi at threshold t, with the Phi and phi it is made of
__device__ __forceinline__ double ehvi_psi(int erf_mode, double mu, double sigma, double t, double *cdf, double *pdf)
{
    const double dm = mu - t;
    gauss_cdf_pdf_dev(erf_mode, dm / sigma, cdf, pdf);
    return sigma * *pdf + dm * *cdf;
}

// SUMS: also the four partial sums of the gradient and the two sigmas (out_sums); the value's operations are the same ones.
// ERF: the call's erf flavour (one flavour's constants per instance: both together do not fit the scalar registers)
template <bool SUMS, int ERF>
__global__ __launch_bounds__(256) void ehvi_finish_kernel(EhviArgs a)
{
    __shared__ double fr[2 * IBO_EHVI_MAX_PAIRS];
    for (int k = threadIdx.x; k < 2 * a.n; k += 256) fr[k] = a.front[k];
    __syncthreads();
    const int64_t li = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const bool valid = li < a.t.M;
    const int64_t gi = valid ? li : a.t.M - 1;
    const double mu1 = a.ms[gi], sg1 = sqrt(a.ms[(size_t)a.stride + gi]);
    const double mu2 = a.ms[2 * (size_t)a.stride + gi], sg2 = sqrt(a.ms[3 * (size_t)a.stride + gi]);
    double c0, p0, c1, p1, c2, p2;
    double prev = ehvi_psi(ERF, mu1, sg1, a.r1, &c0, &p0);
    double val = 0.0, gm1 = 0.0, gs1 = 0.0, gm2 = 0.0, gs2 = 0.0;
    for (int i = 0; i <= a.n; i++) {
        const bool last = i == a.n;                                  // the strip beyond a_n: psi_1(+inf) = Phi = phi = 0, b = r2
        double next = 0.0;
        c1 = 0.0; p1 = 0.0;
        if (!last) next = ehvi_psi(ERF, mu1, sg1, fr[2 * i], &c1, &p1);
        const double w = ehvi_psi(ERF, mu2, sg2, last ? a.r2 : fr[2 * i + 1], &c2, &p2);
        double d = prev - next;
        const bool neg = d < 0.0;                                    // (a NaN is not: it goes through)
        if (neg) d = 0.0;
        val = val + d * w;
        if (SUMS) {
            gm1 = gm1 + (neg ? 0.0 : (c0 - c1) * w);
            gs1 = gs1 + (neg ? 0.0 : (p0 - p1) * w);
            gm2 = gm2 + d * c2;
            gs2 = gs2 + d * p2;
            c0 = c1; p0 = p1;
        }
        prev = next;
    }
    finish_tail<false>(a.t, li, val, [&] {
        if (a.out_val) a.out_val[li] = val;
        if (SUMS) {
            const size_t st = (size_t)a.sums_stride;
            a.out_sums[li] = gm1; a.out_sums[st + li] = gs1; a.out_sums[2 * st + li] = gm2; a.out_sums[3 * st + li] = gs2;
            a.out_sums[4 * st + li] = sg1; a.out_sums[5 * st + li] = sg2;
        }
    });
}

int launch_ehvi_finish(const EhviArgs &a, bool sums, hipStream_t s)
{
    if (!finish_tail_ok(a.t) || a.t.M > a.stride || a.n < 0 || a.n > IBO_EHVI_MAX_PAIRS || (a.n > 0 && !a.front) || (a.erf_mode != 0 && a.erf_mode != 1) || (sums && (!a.out_sums || a.sums_stride < a.t.M)))
        return (int)hipErrorInvalidValue;
    const int64_t nblk = (a.t.M + 255) / 256;
    void (*k)(EhviArgs) = sums ? (a.erf_mode ? ehvi_finish_kernel<true, 1> : ehvi_finish_kernel<true, 0>)
                               : (a.erf_mode ? ehvi_finish_kernel<false, 1> : ehvi_finish_kernel<false, 0>);
    hipLaunchKernelGGL(k, dim3((unsigned)nblk), dim3(256), 0, s, a);
    return (int)hipGetLastError();
}

void ibo_touch_ehvi() { hipFuncAttributes a; (void)hipFuncGetAttributes(&a, (const void *)ehvi_finish_kernel<false, 0>); }     // (see small2.hip: ibo_touch_small2)

// marg.hip -- the combine of an integrated acquisition sweep (ibo_iacq_sweep): val = sum_s w_s acq(mu_s, s2_s) per candidate from the
// (mu, s2) pairs the per-member sweeps left in device scratch, the mixture's mean and variance where asked for, the exclusion balls, the
// optional per-candidate outputs and one (max, lowest index) partial per 256 candidates for launch_argmax_final.
//
// A streaming pass: 16 bytes per member and candidate in (twice that with mean / var, whose second pass finds the first one's lines in L2),
// up to 24 out, one erf chain per member.  One thread per candidate, consecutive lanes on consecutive elements of every array (8-byte
// loads and stores, coalesced), no LDS beyond the four per-wave partials of the reduction, no atomics.  The weights are kernel arguments:
// the member loop reads them with scalar loads at a uniform index, nothing is indexed in registers.
#include "marg.h"

// Every sum runs over the members in ascending s, products and sums rounded separately (no fused multiply-add: the host restatement
// is plain fp64).  The sums start at -0.0, the one start that leaves a single term -- S = 1, w = 1 -- every bit it has, a -0.0 included.
// NaN values and excluded candidates never win the arg-max (block256_argmax's rule)
__global__ __launch_bounds__(256) void marg_finish_kernel(MargArgs a)
{
#pragma clang fp contract(off)
    const int64_t li = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const bool valid = li < a.t.M;
    const int64_t gi = valid ? li : a.t.M - 1;
    double val = -0.0, sm = -0.0, sw = 0.0;
    for (int s = 0; s < a.S; s++) {
        const double w = a.w[s];
        if (w == 0.0) continue;
        const double mu = a.ms[(size_t)(2 * s) * a.stride + gi];
        const double s2 = a.ms[(size_t)(2 * s + 1) * a.stride + gi];
        const double v = (a.acq == 3) ? mu : acq_value_dev(a.acq, a.erf_mode, mu, sqrt(s2), a.ymax, a.parm);
        val += w * v;
        sm += w * mu;
        sw += w;
    }
    const double mbar = sm / sw;
    double vbar = 0.0;
    if (a.out_var) {                     // the second pass: deviations from the mean, not E[x^2] - mbar^2
        double sv = 0.0;
        for (int s = 0; s < a.S; s++) {
            const double w = a.w[s];
            if (w == 0.0) continue;
            const double mu = a.ms[(size_t)(2 * s) * a.stride + gi];
            const double s2 = a.ms[(size_t)(2 * s + 1) * a.stride + gi];
            const double d = mu - mbar;
            sv += w * (s2 + d * d);
        }
        vbar = sv / sw;
    }
    finish_tail<true>(a.t, li, val, [&] {
        if (a.out_val) a.out_val[li] = val;
        if (a.out_mean) a.out_mean[li] = mbar;
        if (a.out_var) a.out_var[li] = vbar;
    });
}

int launch_marg_finish(const MargArgs &a, hipStream_t s)
{
    if (!finish_tail_ok(a.t) || a.t.M > a.stride || a.S < 1 || a.S > IBO_MARG_MAX || !a.ms) return (int)hipErrorInvalidValue;
    const int64_t nblk = (a.t.M + 255) / 256;
    hipLaunchKernelGGL(marg_finish_kernel, dim3((unsigned)nblk), dim3(256), 0, s, a);
    return (int)hipGetLastError();
}

void ibo_touch_marg() { hipFuncAttributes a; (void)hipFuncGetAttributes(&a, (const void *)marg_finish_kernel); }     // (see small2.hip: ibo_touch_small2)

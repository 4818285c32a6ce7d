// cacq.hip -- the combine of a constrained acquisition sweep (ibo_cacq_sweep): val = A P per candidate from the (mu, s2) pairs the
// per-model sweeps left in device scratch, the exclusion balls, the optional per-candidate outputs and one (max, lowest index) partial
// per 256 candidates for launch_argmax_final.
//
// A streaming pass: 16 bytes per model and candidate in, up to 24 out, one erf chain per model.  One thread per candidate, consecutive
// lanes on consecutive elements of every array (8-byte loads and stores, coalesced), no LDS beyond the four per-wave partials of the
// reduction.  At 2^20 candidates and two constraints that is 75 MB against three MFMA-bound sweeps of 16.5 ms.
#include "cacq.h"

// NaN values and excluded candidates never win the arg-max (block256_argmax's rule)
__global__ __launch_bounds__(256) void cacq_finish_kernel(CacqArgs a)
{
    const int64_t li = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const bool valid = li < a.t.M;
    const int64_t gi = valid ? li : a.t.M - 1;
    double A, P;
    double val = cacq_value_dev(a.spec, [&](int k, double *mu, double *s2) {
        *mu = a.ms[(size_t)(2 * k) * a.stride + gi];
        *s2 = a.ms[(size_t)(2 * k + 1) * a.stride + gi];
    }, &A, &P);
    finish_tail<true>(a.t, li, val, [&] {
        if (a.out_acq) a.out_acq[li] = A;
        if (a.out_pof) a.out_pof[li] = P;
        if (a.out_val) a.out_val[li] = val;
    });
}

int launch_cacq_finish(const CacqArgs &a, hipStream_t s)
{
    if (!finish_tail_ok(a.t) || a.t.M > a.stride) return (int)hipErrorInvalidValue;
    const int64_t nblk = (a.t.M + 255) / 256;
    hipLaunchKernelGGL(cacq_finish_kernel, dim3((unsigned)nblk), dim3(256), 0, s, a);
    return (int)hipGetLastError();
}

void ibo_touch_cacq() { hipFuncAttributes a; (void)hipFuncGetAttributes(&a, (const void *)cacq_finish_kernel); }     // (see small2.hip: ibo_touch_small2)

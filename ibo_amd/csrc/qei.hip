// qei.hip -- the Monte-Carlo finish of the parallel expected improvement (ibo_qei_sweep / ibo_qei_batch / ibo_qei_direct_max).
//
//   qei_finish_kernel<P>   P pending points.  One wavefront per QEI_CW candidates, lanes over the samples (kg_epigraph_kernel's layout); a
//                          workgroup's 16 candidates share every stage of QEI_SB samples, which its 256 threads copy from the transposed
//                          sample block into LDS (P + 2 rows: z_.0 .. z_.P and g).  Per candidate the forward substitution l = L_P^-1 c
//                          and d run once, wave-uniform, with L_P read from the kernel's arguments; per (candidate, sample) P + 1 fused
//                          multiply-adds, a max, a subtraction and an add.  P is a template parameter: every loop over the pending
//                          points is unrolled and l stays in registers -- no scratch.
// The order of every sum is ibo_abi.h's: it depends on nothing but the candidate, so its bits are the same in any chunk, at any place,
// in any call.
#include "qei.h"

__device__ __forceinline__ double qei_wave_sum(double v)
{
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);      // (a + b = b + a: every lane ends with the same bits)
    return v;
}

template <int P>
__global__ __launch_bounds__(256) void qei_finish_kernel(QeiFinishArgs a)
{
    __shared__ double zs[(P + 2) * QEI_SB];
    constexpr int PP = P > 0 ? P : 1;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int x0 = (blockIdx.x * 4 + wv) * QEI_CW;
    double mu[QEI_CW], d[QEI_CW], l[QEI_CW][PP], sum[QEI_CW];
    bool bad[QEI_CW];
#pragma unroll
    for (int c = 0; c < QEI_CW; c++) {
        const int x = x0 + c < a.m ? x0 + c : a.m - 1;
        mu[c] = a.mu[x];
        double r = a.s2[x];
        l[c][0] = 0.0;
#pragma unroll
        for (int j = 0; j < P; j++) {
            double t = a.C[(size_t)x * a.ldc + j];
#pragma unroll
            for (int i = 0; i < j; i++) t = fma(-a.L[j * (j + 1) / 2 + i], l[c][i], t);
            l[c][j] = t / a.L[j * (j + 1) / 2 + j];
            r = fma(-l[c][j], l[c][j], r);
        }
        d[c] = r > 0.0 ? sqrt(r) : 0.0;
        bad[c] = !(mu[c] == mu[c]) || !(r == r);                    // a NaN coordinate: the max below would pass it over
        sum[c] = 0.0;
    }
    for (int s0 = 0; s0 < a.Sp; s0 += QEI_SB) {
#pragma unroll
        for (int j = 0; j < P + 2; j++) zs[j * QEI_SB + threadIdx.x] = a.ZG[(size_t)j * a.Sp + s0 + threadIdx.x];
        __syncthreads();
#pragma unroll
        for (int k = 0; k < QEI_SB / 64; k++) {
            const int sl = k * 64 + lane;
            double z[P + 1];
#pragma unroll
            for (int j = 0; j <= P; j++) z[j] = zs[j * QEI_SB + sl];
            const double g = zs[(P + 1) * QEI_SB + sl];
            const bool live = s0 + sl < a.S;
#pragma unroll
            for (int c = 0; c < QEI_CW; c++) {
                double f = mu[c];
#pragma unroll
                for (int j = 0; j < P; j++) f = fma(l[c][j], z[j], f);
                f = fma(d[c], z[P], f);
                const double term = (f > g ? f : g) - a.t;
                if (live && term > 0.0) sum[c] += term;
            }
        }
        __syncthreads();
    }
#pragma unroll
    for (int c = 0; c < QEI_CW; c++) {
        const double v = qei_wave_sum(sum[c]) / (double)a.S;
        if (lane == 0 && x0 + c < a.m) a.qei[x0 + c] = bad[c] ? NAN : v;
    }
}

template <int P>
static void qei_launch(const QeiFinishArgs &a, hipStream_t s)
{
    const int per = 4 * QEI_CW;
    hipLaunchKernelGGL(qei_finish_kernel<P>, dim3((a.m + per - 1) / per), dim3(256), 0, s, a);
}

int launch_qei_finish(const QeiFinishArgs &a, hipStream_t s)
{
    if (a.m < 1 || a.p < 0 || a.p > QEI_MAX_P || a.S < 1 || a.Sp < a.S || (a.Sp % QEI_SB) || (a.p > 0 && a.ldc < (size_t)a.p)) return (int)hipErrorInvalidValue;
    typedef void (*launch_t)(const QeiFinishArgs &, hipStream_t);
    static const launch_t table[QEI_MAX_P + 1] = {qei_launch<0>, qei_launch<1>, qei_launch<2>, qei_launch<3>, qei_launch<4>, qei_launch<5>, qei_launch<6>,
                                                  qei_launch<7>, qei_launch<8>, qei_launch<9>, qei_launch<10>, qei_launch<11>, qei_launch<12>,
                                                  qei_launch<13>, qei_launch<14>, qei_launch<15>};
    table[a.p](a, s);
    return (int)hipGetLastError();
}

void ibo_touch_qei() { hipFuncAttributes a; (void)hipFuncGetAttributes(&a, (const void *)qei_finish_kernel<0>); }     // (see small2.hip: ibo_touch_small2)

// kg.hip -- the knowledge gradient of a candidate against a resident reference set (ibo_kg_sweep / ibo_kg_batch / ibo_kg_direct_max).
//
//   kg_rows_kernel      one wavefront per row of Kt / Vt: k*.aY, k*.a1, |v|^2 -> mu, the clipped s2
//   kg_cross_kernel     B = (K(X, A) - VtX VtA^T) / sigma_x on v_mfma_f64_16x16x4_f64 through cv_tile<false> (cov_dev.h): 64 x 64 tiles of
//                       (candidates x reference points), stored candidate-major; <false>: without the division (qei.hip's covariances)
//   kg_epigraph_kernel  the expected maximum of n (+ 1) lines per candidate: one wavefront per candidate, its slopes in LDS, the reference
//                       means in LDS once per workgroup; lane l owns the lines l, l + 64, .. and scans all the others (n^2 pair steps
//                       with one fp64 division each -- the cost of the whole acquisition from a few hundred lines on)
//   kg_argmax_kernel    cacq_finish_kernel's reduction over the values: one partial per 256 candidates
// Every sum runs in an order that depends on nothing but the row it belongs to: a candidate's bits are the same in any chunk, at any
// place, in any call.
#include "kg.h"
#include "cov_dev.h"

__device__ __forceinline__ double kg_wave_sum(double v)
{
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);      // (a + b = b + a: every lane ends with the same bits)
    return v;
}

__global__ __launch_bounds__(256) void kg_rows_kernel(KgRowsArgs a)
{
    const int lane = threadIdx.x & 63, r = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= a.m) return;
    const double *kt = a.Kt + (size_t)r * a.ldk, *vt = a.Vt + (size_t)r * a.ldv;
    const bool pr = a.prior.nb > 0;
    double sy = 0.0, s1 = 0.0, q = 0.0;
    for (int k = lane; k < a.N; k += 64) {
        const double kk = kt[k];
        sy = fma(kk, a.alphaY[k], sy);
        if (pr) s1 = fma(kk, a.alpha1[k], s1);
    }
    for (int k = lane; k < a.K; k += 64) { const double v = vt[k]; q = fma(v, v, q); }
    sy = kg_wave_sum(sy); s1 = kg_wave_sum(s1); q = kg_wave_sum(q);
    if (lane != 0) return;
    double mu = sy;
    if (pr) {
        const double *xp = a.Q + (size_t)r * a.D;
        const double m = prior_mean_dev(a.prior, a.D, [&](int j) { return xp[j]; });
        mu = m + sy - m * s1;
    }
    double s2 = 1.0 + a.noise - q;
    if (s2 < a.clamp_lo) s2 = a.clamp_lo;
    else if (s2 > 10.0) s2 = 10.0;
    a.mu[r] = mu;
    if (a.q) a.q[r] = q;
    if (a.s2) a.s2[r] = s2;
}

// one 64 x 64 tile per workgroup: blockIdx.y the candidates' tile, blockIdx.x the reference points'
template <bool SCALED>
__global__ void __launch_bounds__(256) kg_cross_kernel(KgCrossArgs a)
{
    __shared__ double As[64 * CV_LD], Bs[64 * CV_LD];
    const int r0 = blockIdx.y * 64, n0 = blockIdx.x * 64;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, wr = wv >> 1, wc = wv & 1, D = a.kp.D;
    d4_t acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; i++)
#pragma unroll
        for (int j = 0; j < 2; j++) acc[i][j] = d4_t{0.0, 0.0, 0.0, 0.0};
    cv_tile<false>(a.VtX, a.ldx, a.VtA, a.lda, r0, n0, a.K, 0, acc, As, Bs);
#pragma unroll
    for (int i = 0; i < 2; i++)
#pragma unroll
        for (int j = 0; j < 2; j++)
#pragma unroll
            for (int e = 0; e < 4; e++) {
                const int x = r0 + 32 * wr + 16 * i + (lane >> 4) + 4 * e, c = n0 + 32 * wc + 16 * j + (lane & 15);
                double v = 0.0;
                if (x < a.m && c < a.n) {
                    const double k = cov_from_z_rt(a.kp.family, wsqdist_dev(a.kp.w, a.A + (size_t)c * D, a.X + (size_t)x * D, D), a.kp.sf2);
                    v = k - acc[i][j][e];
                    if (SCALED) v = v / sqrt(a.s2[x]);
                }
                a.B[(size_t)x * a.ldb + c] = v;
            }
}

// Phi and phi at a crossing point, exact at the two ends of the axis
__device__ __forceinline__ void kg_cdf_pdf(double z, double *cdf, double *pdf)
{
    if (z == -INFINITY) { *cdf = 0.0; *pdf = 0.0; }
    else if (z == INFINITY) { *cdf = 1.0; *pdf = 0.0; }
    else gauss_cdf_pdf_dev(0, z, cdf, pdf);
}

// Dynamic LDS: the reference means (n doubles), then each wavefront's slope row (n doubles).  Line i of a candidate is its own line for
// i == 0 with with_self, reference point i - with_self otherwise; every mu has mu* = max_i mu_i taken off before it is used.
__global__ __launch_bounds__(256) void kg_epigraph_kernel(KgEpiArgs a)
{
    extern __shared__ double kg_lds[];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, n = a.n, ws = a.with_self, L = n + ws;
    double *ms = kg_lds, *bs = kg_lds + (size_t)n * (1 + wv);
    const int xr = blockIdx.x * 4 + wv;
    const bool valid = xr < a.m;
    const int x = valid ? xr : a.m - 1;
    const double *brow = a.B + (size_t)x * a.ldb;
    for (int j = threadIdx.x; j < n; j += 256) ms[j] = a.muA[j];
    for (int j = lane; j < n; j += 64) bs[j] = brow[j];
    __syncthreads();
    const double mux = a.mu[x];
    const double mstar = ws ? fmax(a.maxA, mux) : a.maxA;
    const double m0 = mux - mstar, b0 = fmax(1.0 - a.q[x], 0.0) / sqrt(a.s2[x]);
    double sum = 0.0;
    for (int i = lane; i < L; i += 64) {
        const bool self = ws && i == 0;
        const int ir = self ? 0 : i - ws;
        const double mi = self ? m0 : ms[ir] - mstar, bi = self ? b0 : bs[ir];
        double lo = -INFINITY, hi = INFINITY;
        bool out = false;
        // c_ij = (mu_j - mu_i) / (b_i - b_j): both differences as written, so that c_ji has the same bits.  before: j < i.
        auto step = [&](double mj, double bj, bool before) {
            const double c = (mj - mi) / (bi - bj);
            if (bj < bi) lo = fmax(lo, c);
            else if (bj > bi) hi = fmin(hi, c);
            else out = out || mj > mi || (mj == mi && before);
        };
        if (ws && !self) step(m0, b0, true);
        for (int j = 0; j < n; j++) step(ms[j] - mstar, bs[j], j + ws < i);      // (j + ws == i: equal in both, not before -- no effect)
        if (!out && lo < hi) {
            double Pl, pl, Ph, ph;
            kg_cdf_pdf(lo, &Pl, &pl);
            kg_cdf_pdf(hi, &Ph, &ph);
            sum += mi * (Ph - Pl) + bi * (pl - ph);
        }
    }
    sum = kg_wave_sum(sum);
    if (valid && lane == 0) a.kg[xr] = sum < 0.0 ? 0.0 : sum;            // (not fmax: a NaN stays a NaN, and the arg-max passes it over)
}

// A NaN never wins the arg-max (block256_argmax's rule)
__global__ __launch_bounds__(256) void kg_argmax_kernel(const double *__restrict__ kg, int64_t m, int64_t first, int64_t index_base,
                                                        double *__restrict__ part_val, int64_t *__restrict__ part_idx)
{
    const int64_t li = (int64_t)blockIdx.x * 256 + threadIdx.x;
    double val = li < m ? kg[li] : -INFINITY;
    int64_t idx = index_base + first + li;
    if (!(li < m) || !(val == val)) { val = -INFINITY; idx = INT64_MAX; }
    block256_argmax(val, idx, part_val, part_idx);
}

int launch_kg_rows(const KgRowsArgs &a, hipStream_t s)
{
    if (a.m < 1) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(kg_rows_kernel, dim3((a.m + 3) / 4), dim3(256), 0, s, a);
    return (int)hipGetLastError();
}

int launch_kg_cross(const KgCrossArgs &a, hipStream_t s)
{
    if (a.m < 1 || a.m > a.mp || a.n < 1 || a.n > a.np || (a.mp & 63) || (a.np & 63) || (a.K & (CV_KB - 1)) || a.ldb < (size_t)a.np)
        return (int)hipErrorInvalidValue;
    if (a.unscaled) hipLaunchKernelGGL(kg_cross_kernel<false>, dim3(a.np / 64, a.mp / 64), dim3(256), 0, s, a);
    else hipLaunchKernelGGL(kg_cross_kernel<true>, dim3(a.np / 64, a.mp / 64), dim3(256), 0, s, a);
    return (int)hipGetLastError();
}

int launch_kg_epigraph(const KgEpiArgs &a, hipStream_t s)
{
    if (a.m < 1 || a.n < 1 || a.n + (a.with_self ? 1 : 0) > IBO_KG_LINES || a.ldb < (size_t)a.n) return (int)hipErrorInvalidValue;
    const size_t lds = sizeof(double) * (size_t)a.n * 5;            // 40 KiB at 1024 reference points
    hipLaunchKernelGGL(kg_epigraph_kernel, dim3((a.m + 3) / 4), dim3(256), lds, s, a);
    return (int)hipGetLastError();
}

int launch_kg_argmax(const double *kg, int64_t m, int64_t first, int64_t index_base, double *part_val, int64_t *part_idx, hipStream_t s)
{
    if (m < 1 || (first & 255)) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(kg_argmax_kernel, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, s, kg, m, first, index_base, part_val, part_idx);
    return (int)hipGetLastError();
}

void ibo_touch_kg() { hipFuncAttributes a; (void)hipFuncGetAttributes(&a, (const void *)kg_epigraph_kernel); }     // (see small2.hip: ibo_touch_small2)

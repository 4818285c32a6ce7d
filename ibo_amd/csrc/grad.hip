// grad.hip -- gradients of the posterior and of EI / PI / UCB with respect to the query point (ibo_acq_grad_batch).
//
// Per chunk of Mc candidates, five launches, every sum in a fixed order (no atomics):
//   grad_kstar_kernel    k*_i and h_i = (dk/dx_d) / (w_d (x_d - X_id)) for every row: K, H (Mc x Npad, candidate-major)
//   grad_tri_kernel<0>   t = W k*   (split-K partials Pt[s][c][i] over the rows j <= i of W)
//   grad_tri_kernel<1>   u = W^T t  (split-K partials Pu[s][c][j] over the rows i >= j of W; t is summed from Pt as it is loaded)
//   grad_epi_part_kernel per (row part, candidate): sum_i h_i c_i (x_d - X_id) for c = aY - m a1 and c = u, plus a_Y.k*, a_1.k*, |t|^2
//   grad_finish_kernel   per candidate and dimension: the parts in order, the prior's gradient, the clip rule and the acquisition's chain rule
// u = W^T (W k*) = R^-1 k*: 2 N^2 flops per candidate whatever D, then O(N D) for the epilogue.  W is read row-major as the fit leaves it
// (Npad x Npad, lower triangular; only the triangle is used, whatever lies above it): 64-bit addresses, no buffer descriptors.
#include "grad.h"

#define GR_ROWS 64        // output rows per workgroup of grad_tri_kernel
#define GR_KB 16          // k-step staged in LDS

// k* of one candidate against every row, and h_i: dk/dx_d = h_i w_d (x_d - X_id) -- finite at r = 0 for all three families
__global__ void __launch_bounds__(256) grad_kstar_kernel(GradArgs a, const double *cand, int mc)
{
    __shared__ double xs[IBO_DMAX];
    const int c = blockIdx.y, D = a.kp.D;
    if (threadIdx.x < D) xs[threadIdx.x] = cand[(size_t)c * D + threadIdx.x];
    __syncthreads();
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= a.Npad) return;
    double k = 0.0, h = 0.0;
    if (i < a.N) {
        const double *xr = a.Xp + (size_t)i * a.DP;
        const double z = wsqdist_dev(a.kp.w, xs, xr, D);
        const double sf2 = a.kp.sf2;
        if (a.kp.family == FAM_SE) {
            k = sf2 * exp(-0.5 * z);
            h = -k;
        } else if (a.kp.family == FAM_M3) {
            const double r = sqrt(3.0 * z), e = exp(-r);
            k = sf2 * (1.0 + r) * e;
            h = -3.0 * sf2 * e;
        } else {
            const double r = sqrt(5.0 * z), e = exp(-r);
            k = sf2 * (1.0 + r + r * r * (1.0 / 3.0)) * e;
            h = -(5.0 / 3.0) * sf2 * (1.0 + r) * e;
        }
    }
    a.K[(size_t)c * a.Npad + i] = k;
    a.H[(size_t)c * a.Npad + i] = h;
}

// One 64-row block of t (UP = 0: t_r = sum_{j <= r} W[r][j] k_j) or u (UP = 1: u_r = sum_{i >= r} W[i][r] t_i) for TM = 16 CPT
// candidates, over the k range of split s: [s KC, (s + 1) KC) restricted to the triangle and to the model's N rows.  A workgroup whose
// range is empty writes nothing; the readers sum exactly the splits that can be non-empty for a row (grad_t_at / grad_u_at).
template <int UP, int CPT>
__global__ void __launch_bounds__(256) grad_tri_kernel(GradArgs a, int mc)
{
    constexpr int TM = 16 * CPT;
    __shared__ double ws[GR_KB][GR_ROWS + 1];
    __shared__ double bs[GR_KB][TM + 1];
    const int tid = threadIdx.x, r0 = blockIdx.x * GR_ROWS, s = blockIdx.y, c0 = blockIdx.z * TM;
    const int N = a.N, Np = a.Npad, KC = a.KC;
    if (r0 >= N) return;
    int kbeg = s * KC, kend = min((s + 1) * KC, N);
    if (UP) kbeg = max(kbeg, r0);
    else kend = min(kend, r0 + GR_ROWS);
    if (kbeg >= kend) return;
    const int tr = tid & 15, tc = tid >> 4;
    double acc[4][CPT];
#pragma unroll
    for (int x = 0; x < 4; x++)
#pragma unroll
        for (int y = 0; y < CPT; y++) acc[x][y] = 0.0;
    for (int kb = kbeg; kb < kend; kb += GR_KB) {
#pragma unroll
        for (int e = 0; e < GR_ROWS * GR_KB / 256; e++) {
            const int idx = tid + 256 * e;
            int rr, kk;
            if (UP) { rr = idx % GR_ROWS; kk = idx / GR_ROWS; }
            else { kk = idx % GR_KB; rr = idx / GR_KB; }
            const int r = r0 + rr, k = kb + kk;
            double v = 0.0;
            if (k < kend && r < N && (UP ? k >= r : k <= r))
                v = UP ? a.W[(size_t)k * Np + r] : a.W[(size_t)r * Np + k];
            ws[kk][rr] = v;
        }
        for (int idx = tid; idx < TM * GR_KB; idx += 256) {
            const int kk = idx % GR_KB, cc = idx / GR_KB;
            const int k = kb + kk, c = c0 + cc;
            double v = 0.0;
            if (k < kend && c < mc) {
                if (UP) {                                              // t_k: the splits 0 .. k / KC of Pt, in order
                    const int shi = k / KC;
                    for (int q = 0; q <= shi; q++) v += a.Pt[((size_t)q * mc + c) * Np + k];
                } else v = a.K[(size_t)c * Np + k];
            }
            bs[kk][cc] = v;
        }
        __syncthreads();
#pragma unroll
        for (int kk = 0; kk < GR_KB; kk++) {
            double wv[4], bv[CPT];
#pragma unroll
            for (int x = 0; x < 4; x++) wv[x] = ws[kk][tr + 16 * x];
#pragma unroll
            for (int y = 0; y < CPT; y++) bv[y] = bs[kk][tc * CPT + y];
#pragma unroll
            for (int x = 0; x < 4; x++)
#pragma unroll
                for (int y = 0; y < CPT; y++) acc[x][y] = fma(wv[x], bv[y], acc[x][y]);
        }
        __syncthreads();
    }
    double *P = UP ? a.Pu : a.Pt;
#pragma unroll
    for (int y = 0; y < CPT; y++) {
        const int c = c0 + tc * CPT + y;
        if (c >= mc) continue;
#pragma unroll
        for (int x = 0; x < 4; x++) P[((size_t)s * mc + c) * Np + r0 + tr + 16 * x] = acc[x][y];
    }
}

__device__ __forceinline__ double grad_t_at(const GradArgs &a, int mc, int c, int i)
{
    double v = 0.0;
    for (int q = 0; q <= i / a.KC; q++) v += a.Pt[((size_t)q * mc + c) * a.Npad + i];
    return v;
}
__device__ __forceinline__ double grad_u_at(const GradArgs &a, int mc, int c, int i)
{
    double v = 0.0;
    for (int q = i / a.KC; q < a.nsplit; q++) v += a.Pu[((size_t)q * mc + c) * a.Npad + i];
    return v;
}

// Partial sums of one row part [i0, i1) for one candidate.  Thread (g, d): d = tid % DP, g = tid / DP; rows i0 + g, i0 + g + G, ...
// Out: E[(c * nparts + p) * ES + ..] = [aY.k*, a1.k*, |t|^2, S_mu[DP], S_u[DP]], ES = 3 + 2 DP
__global__ void __launch_bounds__(256) grad_epi_part_kernel(GradArgs a, const double *cand, int mc)
{
    __shared__ double xs[IBO_DMAX];
    __shared__ double sm[256 * 2];
    __shared__ double ss[256 * 3];
    __shared__ double mprior;
    const int tid = threadIdx.x, p = blockIdx.x, c = blockIdx.y, D = a.kp.D, DP = a.DP, G = 256 / DP;
    if (tid < D) xs[tid] = cand[(size_t)c * D + tid];
    __syncthreads();
    if (tid == 0) mprior = prior_mean_dev(a.prior, D, [&](int j) { return xs[j]; });
    __syncthreads();
    const double m = mprior;
    const int d = tid % DP, g = tid / DP;
    const int rows = (a.N + a.nparts - 1) / a.nparts;
    const int i0 = p * rows, i1 = min(a.N, i0 + rows);
    const double xd = d < D ? xs[d] : 0.0;
    double smu = 0.0, su = 0.0, sY = 0.0, s1 = 0.0, sq = 0.0;
    const size_t cb = (size_t)c * a.Npad;
    for (int i = i0 + g; i < i1; i += G) {
        const double k = a.K[cb + i], h = a.H[cb + i];
        const double aY = a.alphaY[i], a1 = a.alpha1[i];
        const double u = grad_u_at(a, mc, c, i);
        const double dx = xd - a.Xp[(size_t)i * DP + d];
        smu = fma(h * fma(-m, a1, aY), dx, smu);
        su = fma(h * u, dx, su);
        if (d == 0) {
            const double t = grad_t_at(a, mc, c, i);
            sY = fma(k, aY, sY); s1 = fma(k, a1, s1); sq = fma(t, t, sq);
        }
    }
    sm[2 * tid] = smu; sm[2 * tid + 1] = su;
    if (d == 0) { ss[3 * g] = sY; ss[3 * g + 1] = s1; ss[3 * g + 2] = sq; }
    __syncthreads();
    double *E = a.E + ((size_t)c * a.nparts + p) * (3 + 2 * DP);
    if (tid < DP) {
        double r0 = 0.0, r1 = 0.0;
        for (int q = 0; q < G; q++) { r0 += sm[2 * (q * DP + tid)]; r1 += sm[2 * (q * DP + tid) + 1]; }
        E[3 + tid] = r0; E[3 + DP + tid] = r1;
    } else if (tid < DP + 3) {
        const int j = tid - DP;
        double r = 0.0;
        for (int q = 0; q < G; q++) r += ss[3 * q + j];
        E[j] = r;
    }
}

// one candidate per 64-lane workgroup, lane = dimension
__global__ void __launch_bounds__(64) grad_finish_kernel(GradArgs a, const double *cand, int mc, double *dmu, double *ds2, double *dacq)
{
    __shared__ double xs[IBO_DMAX];
    const int c = blockIdx.x, d = threadIdx.x, D = a.kp.D, DP = a.DP, ES = 3 + 2 * DP;
    if (d < D) xs[d] = cand[(size_t)c * D + d];
    __syncthreads();
    const double *E = a.E + (size_t)c * a.nparts * ES;
    double sY = 0.0, s1 = 0.0, q = 0.0, smu = 0.0, su = 0.0;
    for (int p = 0; p < a.nparts; p++) {
        const double *e = E + (size_t)p * ES;
        sY += e[0]; s1 += e[1]; q += e[2];
        if (d < DP) { smu += e[3 + d]; su += e[3 + DP + d]; }
    }
    if (d >= D) return;
    double dm = 0.0;
    const double m = prior_mean_dev(a.prior, D, [&](int e) { return xs[e]; }, d, &dm);
    const double w = a.kp.w[d];
    const double mu = a.prior.nb > 0 ? m + sY - m * s1 : sY;
    const double gmu = dm * (1.0 - s1) + w * smu;
    const double raw = 1.0 + a.noise - q;
    const bool clipped = !(raw > a.clamp_lo && raw < 10.0);
    const double s2 = raw < a.clamp_lo ? a.clamp_lo : (raw > 10.0 ? 10.0 : raw);
    const double gs2 = clipped ? 0.0 : -2.0 * w * su;
    const size_t o = (size_t)c * D + d;
    if (dmu) dmu[o] = gmu;
    if (ds2) ds2[o] = gs2;
    if (dacq) {
        const double sig = sqrt(s2), gsig = gs2 / (2.0 * sig);
        double g;
        if (a.acq == 2) g = gmu + a.parm * gsig;
        else {
            const double z = (mu - a.ymax - a.parm) / sig;
            double cdf, pdf;
            gauss_cdf_pdf_dev(a.erf_mode, z, &cdf, &pdf);
            g = a.acq == 1 ? pdf * (gmu - z * gsig) / sig : cdf * gmu + pdf * gsig;
        }
        dacq[o] = g;
    }
}

int launch_grad(const GradArgs &a, const double *cand, int mc, double *dmu, double *ds2, double *dacq, hipStream_t s)
{
    grad_kstar_kernel<<<dim3((a.Npad + 255) / 256, mc), 256, 0, s>>>(a, cand, mc);
    const int rb = a.Npad / GR_ROWS;
    if (a.TM == 16) {
        const dim3 grid(rb, a.nsplit, (mc + 15) / 16);
        grad_tri_kernel<0, 1><<<grid, 256, 0, s>>>(a, mc);
        grad_tri_kernel<1, 1><<<grid, 256, 0, s>>>(a, mc);
    } else {
        const dim3 grid(rb, a.nsplit, (mc + 63) / 64);
        grad_tri_kernel<0, 4><<<grid, 256, 0, s>>>(a, mc);
        grad_tri_kernel<1, 4><<<grid, 256, 0, s>>>(a, mc);
    }
    grad_epi_part_kernel<<<dim3(a.nparts, mc), 256, 0, s>>>(a, cand, mc);
    grad_finish_kernel<<<mc, 64, 0, s>>>(a, cand, mc, dmu, ds2, dacq);
    return (int)hipGetLastError();
}

// Chunking: candidates per chunk (mc), split-K count and row parts, all fixed by (N, Npad, M) alone -- the same call gives the same bits
GradPlan grad_plan(int N, int Npad, int DP, int64_t M)
{
    GradPlan pl;
    const int rb = Npad / GR_ROWS;
    pl.TM = M <= 16 ? 16 : 64;
    // scratch per candidate: K, H, and nsplit partials each of t and u (Npad doubles apiece), plus the epilogue's parts
    const size_t budget = (size_t)192 << 20;                          // bytes of scratch per chunk, at most (one chunk at a time)
    int64_t mc = M < 16384 ? M : 16384;                               // (grid dimension y of the per-candidate launches)
    int nsplit = 1;
    for (;;) {
        const int mt = (int)((mc + pl.TM - 1) / pl.TM);
        // enough workgroups to fill the chip: about 2048 non-empty (row block, split, candidate tile) triples; half the pairs are empty
        nsplit = (int)((4096 + (int64_t)rb * mt - 1) / ((int64_t)rb * mt));
        nsplit = nsplit < 1 ? 1 : (nsplit > rb ? rb : nsplit);
        const size_t per = (size_t)Npad * 8 * (2 + 2 * (size_t)nsplit);
        if ((size_t)mc * per <= budget || mc <= pl.TM) break;
        mc = (int64_t)(budget / per) / pl.TM * pl.TM;
        if (mc < pl.TM) mc = pl.TM;
    }
    pl.mc = (int)mc;
    pl.KC = (Npad / nsplit + GR_ROWS - 1) / GR_ROWS * GR_ROWS;        // a multiple of the row block: the triangle's edge falls on a block edge
    pl.nsplit = (N + pl.KC - 1) / pl.KC;
    // row parts of the epilogue: about 1024 workgroups, at least 256 rows each
    int np = (int)((1024 + mc - 1) / mc);
    const int maxp = (N + 255) / 256;
    pl.nparts = np < 1 ? 1 : (np > maxp ? maxp : np);
    pl.ws_doubles = (size_t)pl.mc * Npad * (2 + 2 * (size_t)pl.nsplit) + (size_t)pl.mc * pl.nparts * (3 + 2 * DP);
    return pl;
}

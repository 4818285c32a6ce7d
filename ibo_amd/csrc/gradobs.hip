// gradobs.hip -- the derivative covariance of a GP observed with gradients (ibo_ggp_*): rows in point-major order, see gradobs.h.
//
//   gradobs_assemble_kernel  A = [K, dK/dx'; dK/dx, d2K/dx dx'] with its diagonal rule, in the identity-padded frame of the factorisation.
//                            One workgroup per tile of 16 x 16 point pairs: the pair's three factors (one exp, one sqrt for Matern) go to
//                            LDS once, then the tile's 16 (D + 1) x 16 (D + 1) entries are formed from them and stored row by row
//                            (consecutive lanes, consecutive columns)
//   gradobs_kstar_kernel     Kt = K*(Q, data) of a chunk of query points, query-major, zero in the pad: one workgroup per query point and
//                            256 data points -- two factors per (query, point) to LDS, then the 256 (D + 1) entries in column order
//   gradobs_acq_kernel       EI / PI / UCB from (mu, s2) by acq_value_dev, the sweeps' epilogue formula
//   gradobs_contract_kernel  the marginal likelihood's gradient (ibo_ggp_nlml_grad): K^-1 - alpha alpha^T against dA/dlog theta, a workgroup per
//   gradobs_reduce_kernel    tile of 16 x 16 point pairs, per-tile partial sums added in a fixed order (see the kernels)
// Both covariance kernels are exp- and store-bound and sum nothing, so a row's bits depend on its own points alone.
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

__global__ void __launch_bounds__(256) gradobs_assemble_kernel(KParams kp, const double *__restrict__ X, int N, double vdiag,
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
            if (gr == gc) v = a == 0 ? vdiag : v + gnoise[a - 1];
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

// ---- the marginal likelihood's gradient (gradobs.h: launch_gradobs_contract).  The assembly kernel's shape: a workgroup per tile of 16 x 16
// point pairs, coordinates, weights and alpha's rows in LDS, one thread per pair.  The thread walks its pair's (D + 1) x (D + 1) block of
// Kinv once -- row d for (C t)_d and, when a per-dimension length scale is asked for, column d for (C^T t)_d; the lanes of a row of pairs
// sit D + 1 columns apart, so a wave's loads of one step share their cache lines with its next D steps -- and takes alpha alpha^T off in
// closed form (its block is an outer product: O(D) per pair).  A pair's own block (i = j) has t = 0: only its diagonal is read, so a block
// that straddles two of Kinv's 64-row blocks never touches the upper one.  Pairs above the diagonal and off the matrix weigh 0.
// Sums: a wave's by wave_sum_rows, the four waves' through LDS, first to last; per dimension V_d as soon as row d is done, then, once the
// pair's scalars are known, w_d u_d^2 times them.  Tiles above the diagonal leave at once.
__global__ void __launch_bounds__(256) gradobs_contract_kernel(KParams kp, const double *__restrict__ X, int N, const double *__restrict__ Kinv,
                                                               int ld, const double *__restrict__ alpha, int need_ard, double *__restrict__ part)
{
    __shared__ double xr[GO_TP * IBO_DMAX], xc[GO_TP * IBO_DMAX], ws[IBO_DMAX];
    __shared__ double ar[GO_TP * (IBO_DMAX + 1)], ac[GO_TP * (IBO_DMAX + 1)], dg[GO_TP * (IBO_DMAX + 1)], red[IBO_DMAX + 2][4];
    const int by = blockIdx.y, bx = blockIdx.x;
    if (bx > by) return;
    const int D = kp.D, B = D + 1, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int i0 = by * GO_TP, j0 = bx * GO_TP, nt = gridDim.y;
    const size_t nlow = (size_t)nt * (nt + 1) / 2, blk = (size_t)by * (by + 1) / 2 + bx;
    for (int e = tid; e < GO_TP * D; e += 256) {
        const int p = e / D, d = e - p * D;
        xr[e] = i0 + p < N ? X[(size_t)(i0 + p) * D + d] : 0.0;
        xc[e] = j0 + p < N ? X[(size_t)(j0 + p) * D + d] : 0.0;
    }
    for (int e = tid; e < GO_TP * B; e += 256) {
        const int p = e / B;
        ar[e] = i0 + p < N ? alpha[(size_t)i0 * B + e] : 0.0;
        ac[e] = j0 + p < N ? alpha[(size_t)j0 * B + e] : 0.0;
        dg[e] = 0.0;
    }
    if (tid < D) ws[tid] = kp.w[tid];
    __syncthreads();
    const int pi = tid >> 4, pj = tid & 15, i = i0 + pi, j = j0 + pj;
    const bool in = i < N && j < N && i >= j, off = in && i > j, on = in && i == j;
    const double wgt = off ? 2.0 : (on ? 1.0 : 0.0);
    const double *xi = xr + pi * D, *xj = xc + pj * D, *ai = ar + pi * B, *aj = ac + pj * B;
    const double z = wsqdist_dev(ws, xi, xj, D);
    double k, g1, g2, dg2;                              // dg2 = dg2/dlog(shared length scale), in its finite form
    go_factors(kp.family, z, kp.sf2, &k, &g1, &g2);
    if (kp.family == FAM_SE) dg2 = k * z;
    else if (kp.family == FAM_M3) { const double r = sqrt(3.0 * z); dg2 = r > 0.0 ? 9.0 * k / r : 0.0; }
    else dg2 = g2 * sqrt(5.0 * z);
    const double g3 = z > 0.0 ? dg2 / z : 0.0;          // dg2 = g3 w_h u_h^2 for one dimension's length scale
    const size_t r0 = (size_t)i * B, c0 = (size_t)j * B;
    const double *K0 = Kinv + r0 * (size_t)ld + c0;     // the pair's block (row >= column throughout when i > j)
    double m00 = 0.0, sab = 0.0, trw = 0.0, q = 0.0, pa = 0.0, pb = 0.0;
    if (in) m00 = K0[0] - ai[0] * aj[0];
    if (off)
        for (int e = 0; e < D; e++) {
            const double te = ws[e] * (xi[e] - xj[e]);
            pa = fma(ai[1 + e], te, pa); pb = fma(aj[1 + e], te, pb);
        }
    for (int d = 0; d < D; d++) {
        double vd = 0.0;
        if (in) {
            const double cdd = K0[(size_t)(1 + d) * ld + 1 + d] - ai[1 + d] * aj[1 + d], wc = ws[d] * cdd;
            trw += wc;
            vd = -2.0 * g1 * wc;
            if (on) dg[pi * B + 1 + d] = cdd;
            if (off) {
                const double td = ws[d] * (xi[d] - xj[d]);
                const double abt = ((K0[1 + d] - K0[(size_t)(1 + d) * ld]) - (ai[0] * aj[1 + d] - ai[1 + d] * aj[0])) * td;
                sab += abt;
                const double *row = K0 + (size_t)(1 + d) * ld + 1;
                double rd = 0.0;
                for (int e = 0; e < D; e++) rd = fma(row[e], ws[e] * (xi[e] - xj[e]), rd);
                rd = fma(-ai[1 + d], pb, rd);
                q = fma(td, rd, q);
                vd = -2.0 * g1 * (abt + wc);
                if (need_ard) {
                    const double *col = K0 + ld + 1 + d;
                    double cd = 0.0;
                    for (int e = 0; e < D; e++) cd = fma(col[(size_t)e * ld], ws[e] * (xi[e] - xj[e]), cd);
                    cd = fma(-aj[1 + d], pa, cd);
                    vd = fma(2.0 * g2 * td, rd + cd, vd);
                }
            }
        }
        if (need_ard) {
            const double s = wave_sum_rows(wgt * vd);
            if (lane == 0) red[d][wave] = s;
        }
    }
    if (on) dg[pi * B] = m00;
    const double s1 = sab + trw;
    {
        const double shared = g1 * z * m00 + (g2 * z - 2.0 * g1) * s1 - (dg2 - 4.0 * g2) * q;
        const double signal = 2.0 * (k * m00 + g1 * s1 - g2 * q);
        const double a = wave_sum_rows(wgt * shared), b = wave_sum_rows(wgt * signal);
        if (lane == 0) { red[D][wave] = a; red[D + 1][wave] = b; }
    }
    if (need_ard) {
        const double sard = wgt * (g1 * m00 + g2 * s1 - g3 * q);
        for (int d = 0; d < D; d++) {
            const double u = xi[d] - xj[d];
            const double s = wave_sum_rows(sard * (ws[d] * (u * u)));
            if (lane == 0) red[d][wave] += s;
        }
    }
    __syncthreads();
    for (int c = tid + (need_ard ? 0 : D); c < D + 2; c += 256)
        part[(size_t)c * nlow + blk] = ((red[c][0] + red[c][1]) + red[c][2]) + red[c][3];
    if (bx == by && tid < B) {                          // the noise terms: diag(Kinv) - alpha o alpha of the tile's points, row kind tid
        double s = 0.0;
        for (int p = 0; p < GO_TP; p++) s += dg[p * B + tid];
        part[(size_t)(D + 2) * nlow + (size_t)tid * nt + by] = s;
    }
}

// out[h] = 1/2 the sum of component h's partial sums in a fixed order (h < gs.nh: the derivative gs asks for; then the noise terms, times
// noise and gnoise[e - 1]).  A component is summed the same way whatever else gs holds.
__global__ void __launch_bounds__(256) gradobs_reduce_kernel(const double *__restrict__ part, int nlow, int nt, int D, GradSpec gs, double noise,
                                                             const double *__restrict__ gnoise, double *__restrict__ out)
{
    __shared__ double red[256];
    const int h = blockIdx.x, t = threadIdx.x;
    const double *p;
    int n;
    double scale = 0.5;
    if (h < gs.nh) {
        const int mode = gs.mode[h], c = mode == 0 ? gs.dim[h] : (mode == 2 ? D + 1 : D);
        p = part + (size_t)c * nlow; n = nlow;
    } else {
        const int e = h - gs.nh;
        p = part + (size_t)(D + 2) * nlow + (size_t)e * nt; n = nt;
        scale = 0.5 * (e == 0 ? noise : gnoise[e - 1]);
    }
    double s = 0.0;
    for (int i = t; i < n; i += 256) s += p[i];
    red[t] = s;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) { if (t < o) red[t] += red[t + o]; __syncthreads(); }
    if (t == 0) out[h] = scale * red[0];
}

int launch_gradobs_assemble(const KParams &kp, const double *X, int N, double vdiag, const double *gnoise, double *A, int Np, hipStream_t s)
{
    const int B = kp.D + 1;
    if (N < 1 || kp.D < 1 || kp.D > IBO_DMAX || (Np & 63) || (size_t)N * B > (size_t)Np) return (int)hipErrorInvalidValue;
    const int nt = ((Np + B - 1) / B + GO_TP - 1) / GO_TP;          // tiles of 16 points that cover the frame's Np rows
    hipLaunchKernelGGL(gradobs_assemble_kernel, dim3(nt, nt), dim3(256), 0, s, kp, X, N, vdiag, gnoise, A, Np);
    return (int)hipGetLastError();
}

size_t gradobs_contract_scratch(int N, int D)
{
    const size_t nt = (size_t)(N + GO_TP - 1) / GO_TP;
    return (size_t)(D + 2) * (nt * (nt + 1) / 2) + (size_t)(D + 1) * nt;
}

int launch_gradobs_contract(const KParams &kp, const GradSpec &gs, const double *X, int N, const double *Kinv, int Np, const double *alpha,
                            double noise, const double *gnoise, double *part, double *out, hipStream_t s)
{
    const int D = kp.D, B = D + 1;
    if (N < 1 || D < 1 || D > IBO_DMAX || gs.nh < 0 || gs.nh > IBO_GRAD_MAX || (size_t)N * B > (size_t)Np) return (int)hipErrorInvalidValue;
    int need_ard = 0;
    for (int h = 0; h < gs.nh; h++) need_ard |= gs.mode[h] == 0;
    const int nt = (N + GO_TP - 1) / GO_TP;
    hipLaunchKernelGGL(gradobs_contract_kernel, dim3(nt, nt), dim3(256), 0, s, kp, X, N, Kinv, Np, alpha, need_ard, part);
    hipLaunchKernelGGL(gradobs_reduce_kernel, dim3(gs.nh + B), dim3(256), 0, s, part, nt * (nt + 1) / 2, nt, D, gs, noise, gnoise, out);
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

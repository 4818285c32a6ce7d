// loo.hip -- leave-one-out predictions and the LOO-CV objective with its gradient (ibo_gp_loo, ibo_loo_grad).
//
//   loo_diag_kernel      d_i = sum_{k >= i} W[k][i]^2: the diagonal of A^-1 = W^T W from a handle's W = L^-1, one thread per column, rows in
//                        ascending order, a wave's 64 columns walking the rows together (coalesced along rows)
//   loo_point_kernel     mu_-i = y_i - c_i / d_i, s2_-i = 1 / d_i and sum_i [-log(d_i) / 2 + c_i^2 / (2 d_i)] (one workgroup, fixed order)
//   loo_contract_kernel  the hot path of the gradient: per 64 x 64 tile (rows i, columns b) of T = B dA_h (B = A^-1, dA_h = dK / d log theta_h)
//                        the partial sums r_i = sum_b T_ib alpha_b and s_i = sum_b T_ib B_ib, for up to IBO_LOO_HP derivatives off one panel of B
//   loo_finish_kernel    the partial sums in column-tile order, then d nloo / d log theta_h = -sum_i [alpha_i r_i - (1 + alpha_i^2 / d_i) s_i / 2] / d_i
// The product runs on v_mfma_f64_16x16x4_f64 like cov.hip's: 64 x 64 tiles, four waves of 32 x 32, k-steps of 32 through LDS with the next
// step's operands in registers.  The A operand is a 64-row panel of B, read from the 64 x 64 blocks on and below the diagonal (a block above it
// is the transpose of its mirror image: the routes that form K^-1 store only the lower blocks); the B operand is dA_h, generated from X and the
// kernel parameters into LDS (never stored): a pair's kernel value is computed once per pass and every derivative's factor derived from it.
// Rows and columns beyond N contribute exact zeros.  No atomics: the same call gives the same bits.  64-bit addresses throughout.
#include "loo.h"

#define LO_KB 32                 // k-step staged in LDS
#define LO_LD (LO_KB + 1)        // LDS row stride in doubles (odd: the 16 rows of a fragment fall on distinct banks)
#define LO_HP IBO_LOO_HP

typedef double lo_d2 __attribute__((ext_vector_type(2)));

struct LooPass { int nh; int mode[LO_HP]; int dim[LO_HP]; };      // one pass' derivatives (GradSpec's modes)

// the 256 threads' values summed in a fixed order; red: 256 doubles of LDS
__device__ __forceinline__ double lo_block_sum(double v, double *red)
{
    const int t = threadIdx.x;
    red[t] = v;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) { if (t < o) red[t] += red[t + o]; __syncthreads(); }
    return red[0];
}

__global__ void __launch_bounds__(64) loo_diag_kernel(const double *__restrict__ W, size_t ldw, int N, double *__restrict__ d)
{
    const int k0 = blockIdx.x * 64, i = k0 + threadIdx.x;
    if (i >= N) return;
    double s = 0.0;
    int k = k0;
    for (; k < k0 + 64 && k < N; k++)                      // the wave's diagonal block: column i starts at row i
        if (k >= i) { const double v = W[(size_t)k * ldw + i]; s = fma(v, v, s); }
    const double *p = W + (size_t)k * ldw + i;
    for (; k + 8 <= N; k += 8, p += 8 * ldw) {             // eight rows' loads in flight, the squares added in row order
        double v[8];
#pragma unroll
        for (int u = 0; u < 8; u++) v[u] = p[(size_t)u * ldw];
#pragma unroll
        for (int u = 0; u < 8; u++) s = fma(v[u], v[u], s);
    }
    for (; k < N; k++, p += ldw) { const double v = *p; s = fma(v, v, s); }
    d[i] = s;
}

// d_i = dsrc[i * dstride] (a vector, or the diagonal of B); c_i = aY_i - m(x_i) a1_i (prior.nb = 0: c = aY)
__global__ void __launch_bounds__(256) loo_point_kernel(PriorDev prior, const double *__restrict__ Xp, int DP, int D, int N,
                                                        const double *__restrict__ Y, const double *__restrict__ aY,
                                                        const double *__restrict__ a1, const double *__restrict__ dsrc, size_t dstride,
                                                        double *__restrict__ mu, double *__restrict__ s2, double *__restrict__ out)
{
    __shared__ double red[256];
    double acc = 0.0;
    for (int i = threadIdx.x; i < N; i += 256) {
        double c = aY[i];
        if (prior.nb > 0) c = fma(-prior_mean_dev(prior, D, [&](int j) { return Xp[(size_t)i * DP + j]; }), a1[i], c);
        const double di = dsrc[(size_t)i * dstride];
        if (mu) mu[i] = Y[i] - c / di;
        if (s2) s2[i] = 1.0 / di;
        acc += c * c / (2.0 * di) - 0.5 * log(di);
    }
    const double v = lo_block_sum(acc, red);
    if (threadIdx.x == 0 && out) out[0] = v;
}

// blockIdx.x: column tile (b), blockIdx.y: row tile (i).  part[((h * 2 + which) * nt + column tile) * Np + i], which = 0: r, 1: s.
// Dynamic LDS: As[64 x LO_LD] | Bs[LO_HP][64 x LO_LD] | xb[64 x (D | 1)] (the column tile's points, scaled by sqrt(w_d)) | xa[LO_KB x (D | 1)] (the points of the
// k-step being generated: fetched two steps ahead into registers, so the generation never waits on global memory).
__global__ void __launch_bounds__(256) loo_contract_kernel(KParams kp, LooPass gs, int N, int Np, const double *__restrict__ X, int ldx,
                                                           const double *__restrict__ B, const double *__restrict__ alpha,
                                                           double *__restrict__ part)
{
    extern __shared__ __attribute__((aligned(16))) double lo_lds[];
    double *As = lo_lds, *Bs = As + 64 * LO_LD, *xb = Bs + LO_HP * 64 * LO_LD;
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6, wr = wv >> 1, wc = wv & 1;
    const int bt = blockIdx.x, it = blockIdx.y, b0 = bt * 64, i0 = it * 64, D = kp.D, ldp = D | 1, nt = Np / 64, nh = gs.nh;
    double *xa = xb + 64 * ldp;
    const double inv_w0 = 1.0 / kp.w[0];                  // the Matern kernels have one length scale: |x_a - x_b|^2 = z / w
    const int lr = t >> 4, lk = (t & 15) * 2;             // direct order: this thread's rows lr + 16 u and k pair lk of a stage
    const int tk = t >> 3, tr = (t & 7) * 8;              // transposed order: its k and rows tr .. tr + 7
    for (int e = t; e < 64 * D; e += 256) {
        const int r = e / D, d = e - r * D;
        xb[r * ldp + d] = b0 + r < N ? kp.sw[d] * X[(size_t)(b0 + r) * ldx + d] : 0.0;
    }
    __syncthreads();
    d4_t acc[LO_HP][2][2];
#pragma unroll
    for (int h = 0; h < LO_HP; h++)
#pragma unroll
        for (int i = 0; i < 2; i++)
#pragma unroll
            for (int j = 0; j < 2; j++) acc[h][i][j] = d4_t{0.0, 0.0, 0.0, 0.0};
    lo_d2 va[4], vg[LO_HP][4];
    double xr[LO_KB * IBO_DMAX / 256];                    // a k-step's points: LO_KB x D values over the 256 threads
    auto fetch_x = [&](int kb) {
#pragma unroll
        for (int j = 0; j < LO_KB * IBO_DMAX / 256; j++) {
            const int e = t + 256 * j;
            if (e < LO_KB * D) { const int r = e / D, d = e - r * D; xr[j] = kb + r < N ? kp.sw[d] * X[(size_t)(kb + r) * ldx + d] : 0.0; }
        }
    };
    auto store_x = [&]() {
#pragma unroll
        for (int j = 0; j < LO_KB * IBO_DMAX / 256; j++) {
            const int e = t + 256 * j;
            if (e < LO_KB * D) { const int r = e / D, d = e - r * D; xa[r * ldp + d] = xr[j]; }
        }
    };
    // the panel of B: block (it, ab) as stored when ab < it, the transpose of (ab, it) when ab > it, element by element on the diagonal
    auto fetch = [&](int kb) {
        const int ab = kb >> 6;
        if (ab < it) {
#pragma unroll
            for (int u = 0; u < 4; u++) {
                const int i = i0 + lr + 16 * u, a = kb + lk;
                lo_d2 v = *(const lo_d2 *)(B + (size_t)i * Np + a);
                v.x = (i < N && a < N) ? v.x : 0.0;
                v.y = (i < N && a + 1 < N) ? v.y : 0.0;
                va[u] = v;
            }
        } else if (ab > it) {
            const int a = kb + tk;
#pragma unroll
            for (int u = 0; u < 4; u++) {
                const int i = i0 + tr + 2 * u;
                lo_d2 v = *(const lo_d2 *)(B + (size_t)a * Np + i);
                v.x = (a < N && i < N) ? v.x : 0.0;
                v.y = (a < N && i + 1 < N) ? v.y : 0.0;
                va[u] = v;
            }
        } else {
#pragma unroll
            for (int u = 0; u < 4; u++) {
                const int i = i0 + lr + 16 * u, a = kb + lk, a1 = a + 1;
                lo_d2 v;
                v.x = B[(size_t)(i > a ? i : a) * Np + (i > a ? a : i)];
                v.y = B[(size_t)(i > a1 ? i : a1) * Np + (i > a1 ? a1 : i)];
                v.x = (i < N && a < N) ? v.x : 0.0;
                v.y = (i < N && a1 < N) ? v.y : 0.0;
                va[u] = v;
            }
        }
    };
    // dA_h[b][a] for this thread's four b (rows lr + 16 u of the column tile) and two a (kb + lk, + 1)
    auto gen = [&](int kb) {
        const int a0 = kb + lk;
        const bool in0 = a0 < N, in1 = a0 + 1 < N;
        const double *xa0 = xa + lk * ldp, *xa1 = xa0 + ldp;
        double z[4][2];
#pragma unroll
        for (int u = 0; u < 4; u++) z[u][0] = z[u][1] = 0.0;
#pragma unroll 2
        for (int d = 0; d < D; d++) {
            const double p0 = xa0[d], p1 = xa1[d];
#pragma unroll
            for (int u = 0; u < 4; u++) {
                const double xv = xb[(lr + 16 * u) * ldp + d], t0 = p0 - xv, t1 = p1 - xv;
                z[u][0] = fma(t0, t0, z[u][0]);
                z[u][1] = fma(t1, t1, z[u][1]);
            }
        }
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const int bl = lr + 16 * u, b = b0 + bl;
            double k[2];
#pragma unroll
            for (int c = 0; c < 2; c++)
                k[c] = kp.family == FAM_SE ? kp.sf2 * exp_fast(-0.5 * z[u][c]) : cov_from_z_rt(kp.family, z[u][c], kp.sf2);
#pragma unroll
            for (int h = 0; h < LO_HP; h++) {
                if (h >= nh) continue;
                const int mode = gs.mode[h];
                double g[2];
#pragma unroll
                for (int c = 0; c < 2; c++) {
                    double dk;
                    if (mode == 0) {                           // SE-ARD length scale of dimension dim[h]: K w u^2
                        const int dd = gs.dim[h];
                        const double uu = (c ? xa1 : xa0)[dd] - xb[bl * ldp + dd];
                        dk = k[c] * (uu * uu);
                    } else if (mode == 1) dk = k[c] * z[u][c];  // SE-iso length scale: K z
                    else if (mode == 2) dk = 2.0 * k[c];        // signal magnitude: 2 K (diagonal 2 sf2: the noise is not part of it)
                    else if (mode == 3) {                       // Matern length scales as Kernel.derivative has them (the 3/2 one on the unscaled distance)
                        const double r3 = sqrt(z[u][c] * inv_w0);
                        dk = a0 + c == b ? 0.0 : kp.sf2 * r3 * r3 * exp(-r3);
                    } else {
                        const double zz = 5.0 * z[u][c], s = sqrt(zz);
                        dk = a0 + c == b ? 0.0 : kp.sf2 * (zz + s * s * s) * exp(-s) / 3.0;
                    }
                    g[c] = ((c ? in1 : in0) && b < N) ? dk : 0.0;
                }
                vg[h][u] = lo_d2{g[0], g[1]};
            }
        }
    };
    const int kend = (N + LO_KB - 1) / LO_KB * LO_KB;
    fetch_x(0);
    store_x();
    __syncthreads();
    fetch(0);
    gen(0);
    if (LO_KB < kend) fetch_x(LO_KB);
    __syncthreads();                                       // (everyone has read step 0's points)
    for (int kb = 0; kb < kend; kb += LO_KB) {
        if (kb + LO_KB < kend) store_x();
        if ((kb >> 6) > it) {
#pragma unroll
            for (int u = 0; u < 4; u++) { As[(tr + 2 * u) * LO_LD + tk] = va[u].x; As[(tr + 2 * u + 1) * LO_LD + tk] = va[u].y; }
        } else {
#pragma unroll
            for (int u = 0; u < 4; u++) { double *a = As + (lr + 16 * u) * LO_LD + lk; a[0] = va[u].x; a[1] = va[u].y; }
        }
#pragma unroll
        for (int h = 0; h < LO_HP; h++) {
            if (h >= nh) continue;
#pragma unroll
            for (int u = 0; u < 4; u++) { double *b = Bs + h * 64 * LO_LD + (lr + 16 * u) * LO_LD + lk; b[0] = vg[h][u].x; b[1] = vg[h][u].y; }
        }
        __syncthreads();
        if (kb + LO_KB < kend) {
            fetch(kb + LO_KB);
            gen(kb + LO_KB);
            if (kb + 2 * LO_KB < kend) fetch_x(kb + 2 * LO_KB);
        }
#pragma unroll
        for (int kk = 0; kk < LO_KB; kk += 4) {
            const int ko = kk + (lane >> 4), ro = lane & 15;
            const double a0 = As[(32 * wr + ro) * LO_LD + ko], a1 = As[(32 * wr + 16 + ro) * LO_LD + ko];
#pragma unroll
            for (int h = 0; h < LO_HP; h++) {
                if (h >= nh) continue;
                const double *bs = Bs + h * 64 * LO_LD;
                const double v0 = bs[(32 * wc + ro) * LO_LD + ko], v1 = bs[(32 * wc + 16 + ro) * LO_LD + ko];
                acc[h][0][0] = mfma_f64(a0, v0, acc[h][0][0]);
                acc[h][0][1] = mfma_f64(a0, v1, acc[h][0][1]);
                acc[h][1][0] = mfma_f64(a1, v0, acc[h][1][0]);
                acc[h][1][1] = mfma_f64(a1, v1, acc[h][1][1]);
            }
        }
        __syncthreads();
    }
    // epilogue: T_ib times alpha_b and times B_ib, summed along b: a thread's two column fragments, the 16 lanes of a row, the two waves
    // side by side -- always in that order.  C/D layout: col = lane & 15, row = (lane >> 4) + 4 e.
    double alb[2], bib[2][2][4];
#pragma unroll
    for (int j = 0; j < 2; j++) {
        const int b = b0 + 32 * wc + 16 * j + (lane & 15);
        alb[j] = b < N ? alpha[b] : 0.0;
#pragma unroll
        for (int i = 0; i < 2; i++)
#pragma unroll
            for (int e = 0; e < 4; e++) {
                const int r = i0 + 32 * wr + 16 * i + (lane >> 4) + 4 * e;
                bib[i][j][e] = (r < N && b < N) ? B[(size_t)(r > b ? r : b) * Np + (r > b ? b : r)] : 0.0;
            }
    }
    double *red = Bs;                                      // [h][which][wc][64 rows]: the loop's last barrier has passed
#pragma unroll
    for (int h = 0; h < LO_HP; h++) {
        if (h >= nh) continue;
#pragma unroll
        for (int i = 0; i < 2; i++)
#pragma unroll
            for (int e = 0; e < 4; e++) {
                double rr = acc[h][i][0][e] * alb[0], ss = acc[h][i][0][e] * bib[i][0][e];
                rr = fma(acc[h][i][1][e], alb[1], rr);
                ss = fma(acc[h][i][1][e], bib[i][1][e], ss);
#pragma unroll
                for (int o = 1; o < 16; o <<= 1) { rr += __shfl_xor(rr, o); ss += __shfl_xor(ss, o); }
                if ((lane & 15) == 0) {
                    const int row = 32 * wr + 16 * i + (lane >> 4) + 4 * e;
                    red[((h * 2 + 0) * 2 + wc) * 64 + row] = rr;
                    red[((h * 2 + 1) * 2 + wc) * 64 + row] = ss;
                }
            }
    }
    __syncthreads();
    for (int idx = t; idx < nh * 128; idx += 256) {
        const int hw = idx >> 6, row = idx & 63;           // hw = h * 2 + which
        part[((size_t)hw * nt + bt) * Np + i0 + row] = red[(hw * 2 + 0) * 64 + row] + red[(hw * 2 + 1) * 64 + row];
    }
}

// one workgroup per derivative of the pass
__global__ void __launch_bounds__(256) loo_finish_kernel(const double *__restrict__ part, int N, int Np, const double *__restrict__ B,
                                                         const double *__restrict__ alpha, double *__restrict__ grad)
{
    __shared__ double red[256];
    const int h = blockIdx.x, nt = Np / 64;
    const double *pr = part + (size_t)(h * 2) * nt * Np, *ps = part + (size_t)(h * 2 + 1) * nt * Np;
    double acc = 0.0;
    for (int i = threadIdx.x; i < N; i += 256) {
        double r = 0.0, s = 0.0;
        for (int b = 0; b < nt; b++) { r += pr[(size_t)b * Np + i]; s += ps[(size_t)b * Np + i]; }
        const double di = B[(size_t)i * Np + i], al = alpha[i];
        acc += (al * r - 0.5 * (1.0 + al * al / di) * s) / di;
    }
    const double v = lo_block_sum(acc, red);
    if (threadIdx.x == 0) grad[h] = -v;
}

int launch_loo_diag(const double *W, size_t ldw, int N, double *d, hipStream_t s)
{
    hipLaunchKernelGGL(loo_diag_kernel, dim3((N + 63) / 64), dim3(64), 0, s, W, ldw, N, d);
    return (int)hipGetLastError();
}

int launch_loo_handle(const PriorDev &prior, const double *Xp, int DP, int D, int N, const double *Y, const double *aY, const double *a1,
                      const double *d, double *mu, double *s2, double *out, hipStream_t s)
{
    hipLaunchKernelGGL(loo_point_kernel, dim3(1), dim3(256), 0, s, prior, Xp, DP, D, N, Y, aY, a1, d, (size_t)1, mu, s2, out);
    return (int)hipGetLastError();
}

int launch_loo_value(const double *B, size_t ldb, int N, const double *Y, const double *alpha, double *mu, double *s2, double *out,
                     hipStream_t s)
{
    PriorDev none;
    none.nb = 0; none.theta = 0.0; none.means = none.beta = none.lowerb = none.width = nullptr;
    hipLaunchKernelGGL(loo_point_kernel, dim3(1), dim3(256), 0, s, none, (const double *)nullptr, 0, 0, N, Y, alpha, alpha, B, ldb + 1, mu, s2,
                       out);
    return (int)hipGetLastError();
}

size_t loo_contract_scratch(int Np) { return (size_t)2 * LO_HP * (size_t)(Np / 64) * Np; }

int launch_loo_contract(const KParams &kp, const GradSpec &gs, int N, int Np, const double *X, int ldx, const double *B, const double *alpha,
                        double *part, double *grad, hipStream_t s)
{
    const int nt = Np / 64;
    const size_t lds = sizeof(double) * ((size_t)(1 + LO_HP) * 64 * LO_LD + (64 + LO_KB) * (size_t)(kp.D | 1));      // 84.5 KiB + the points (of 160 KiB)
    hipError_t e = hipFuncSetAttribute((const void *)loo_contract_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return (int)e;
    for (int h0 = 0; h0 < gs.nh; h0 += LO_HP) {
        LooPass p;
        p.nh = gs.nh - h0 < LO_HP ? gs.nh - h0 : LO_HP;
        for (int h = 0; h < LO_HP; h++) { p.mode[h] = h < p.nh ? gs.mode[h0 + h] : 2; p.dim[h] = h < p.nh ? gs.dim[h0 + h] : 0; }
        hipLaunchKernelGGL(loo_contract_kernel, dim3(nt, nt), dim3(256), lds, s, kp, p, N, Np, X, ldx, B, alpha, part);
        hipLaunchKernelGGL(loo_finish_kernel, dim3(p.nh), dim3(256), 0, s, (const double *)part, N, Np, B, alpha, grad + h0);
    }
    return (int)hipGetLastError();
}

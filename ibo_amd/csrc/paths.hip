// paths.hip -- pathwise posterior draws (ibo_paths_*): path_s(x) = m(x) + sum_j phi_j(x) w_sj + sum_i k(x, X_i) c_si for S paths at once.
//
//   paths_tile_kernel   one workgroup per 64 candidates x 64 coefficient columns.  The K loop runs over the Fp feature rows and then the
//                       Np32 kernel rows of the coefficient block in steps of 32.  Per step the 64 x 32 piece of [Phi | K*] is GENERATED
//                       into LDS (each thread: one k, eight candidates) and the 32 x 64 piece of the coefficients is staged beside it; four
//                       waves of 32 x 32 contract them on v_mfma_f64_16x16x4_f64.  Neither Phi nor K* exists in memory.
//                         feature  t = omega_k . x + b_k in double-double (two-product by FMA, two-sum), so that data far from the origin
//                                  lose nothing; n = rint(t 2/pi), r = t - n pi/2 by two FMAs (the first is exact), then the sine and the
//                                  cosine polynomials of fdlibm's kernels on |r| <= pi/4 and the quadrant.  Fixed cost, no slow path;
//                                  accurate to 2e-16 for |t| < 2^30.  A NaN coordinate gives NaN.
//                         kernel   z by differences in wsqdist_dev's arithmetic, cov_from_z_rt (the library's exp and sqrt: a NaN stays one)
//                       Epilogue: the tile goes through LDS transposed; a wave takes 16 columns, lane = candidate: the mean prior
//                       (m + acc - m acc_63, acc_63 = k*.a1 from the tile's own last column), the path-major values, and per path
//                       the wave's (max, first index) under wave_argmax -- one partial per path and 64 candidates.
//   paths_grad_tile_kernel  the gradient of the same tile with respect to x, PG_DC dimensions per workgroup (see the kernel)
//   paths_pick_kernel   a point's own path out of the path-major values (ibo_paths_grad_batch with path_of)
//   paths_solve_kernel  z = W^T y per path, one thread per row j and eight paths, i ascending; coef = aY - z
//   paths_final_kernel  argmax_final_kernel's loop over the partials and block256_argmax, one workgroup per path
#include "paths.h"

// r = (hi + lo) - n pi/2 with n = rint(hi 2/pi), |lo| << |hi|: s = sin r, c = cos r on |r| <= pi/4; returns the quadrant n mod 4
__device__ __forceinline__ int paths_reduce(double hi, double lo, double &s, double &c)
{
    const double n = rint(hi * 6.36619772367581382433e-01);
    double r = fma(-n, 1.57079632679489655800e+00, hi);          // exact: a multiple of 2^-52 below 1
    r = fma(-n, 6.12323399573676603587e-17, r);
    r += lo;
    const int q = (int)n & 3;
    const double z = r * r;
    s = 1.58969099521155010221e-10;
    s = fma(s, z, -2.50507602534068634195e-08);
    s = fma(s, z, 2.75573137070700676789e-06);
    s = fma(s, z, -1.98412698298579493134e-04);
    s = fma(s, z, 8.33333333332248946124e-03);
    s = fma(s, z, -1.66666666666666324348e-01);
    s = fma(r * z, s, r);
    c = -1.13596475577881948265e-11;
    c = fma(c, z, 2.08757232129817482790e-09);
    c = fma(c, z, -2.75573143513906633035e-07);
    c = fma(c, z, 2.48015872894767294178e-05);
    c = fma(c, z, -1.38888888888741095749e-03);
    c = fma(c, z, 4.16666666666666019037e-02);
    c = fma(z * z, c, fma(-0.5, z, 1.0));
    return q;
}

// cos(hi + lo), |lo| << |hi|
__device__ __forceinline__ double paths_cos(double hi, double lo)
{
    double s, c;
    const int q = paths_reduce(hi, lo, s, c);
    const double v = (q & 1) ? s : c;
    return (q == 1 || q == 2) ? -v : v;
}

// sin(hi + lo): the same reduction and polynomials, the other quadrant rule
__device__ __forceinline__ double paths_sin(double hi, double lo)
{
    double s, c;
    const int q = paths_reduce(hi, lo, s, c);
    const double v = (q & 1) ? c : s;
    return (q & 2) ? -v : v;
}

// (s, c) += om x without rounding the product or the sum away: c collects what s cannot hold
__device__ __forceinline__ void paths_dd_fma(double om, double x, double &s, double &c)
{
#pragma clang fp contract(off)
    const double p = om * x;
    const double e = fma(om, x, -p);
    const double sn = s + p;
    const double bb = sn - s;
    const double err = (s - (sn - bb)) + (p - bb);
    c = c + (err + e);
    s = sn;
}

__global__ void __launch_bounds__(256, 2) paths_tile_kernel(PathsArgs a)
{
    extern __shared__ double pt_lds[];
    __shared__ double ms[64];
    const int D = a.kp.D;
    double *Xs = pt_lds;                       // 64 x D: this tile's candidates (zeros beyond m)
    double *As = Xs + 64 * D;                  // 64 x PT_LDA
    double *Bs = As + 64 * PT_LDA;             // PT_KB x PT_LDB
    double *T = As;                            // the epilogue's 64 x 65 tile, column-major, over As and Bs
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6, wr = wv >> 1, wc = wv & 1;
    const int r0 = blockIdx.y * 64;
    const int ct = a.only >= 0 ? a.only / a.pt : (int)blockIdx.x, c0 = ct * 64;
    for (int e = t; e < 64 * D; e += 256) {
        const int r = e / D, d = e - r * D;
        Xs[e] = (r0 + r < a.m) ? a.cand[(size_t)(r0 + r) * a.ldc + d] : 0.0;
    }
    d4_t acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; i++)
#pragma unroll
        for (int j = 0; j < 2; j++) acc[i][j] = d4_t{0.0, 0.0, 0.0, 0.0};
    __syncthreads();
    const int kl = t & 31, rb = t >> 5;                    // generation: k = kb + kl, candidates rb + 8 u
    const int br = t >> 3, bc = (t & 7) * 8;               // coefficient staging: row kb + br, columns c0 + bc .. + 7
    for (int kb = 0; kb < a.kend; kb += PT_KB) {
        const double *bp = a.coef + (size_t)(kb + br) * a.Sp + c0 + bc;
        double bv[8];
#pragma unroll
        for (int u = 0; u < 8; u++) bv[u] = bp[u];
        double g[8];
        if (kb < a.Fp) {
            const int k = kb + kl;
            const double *om = a.omega + (size_t)k * D;
            const double ph = a.phase[k];
            double s[8], c[8];
#pragma unroll
            for (int u = 0; u < 8; u++) { s[u] = ph; c[u] = 0.0; }
            for (int d = 0; d < D; d++) {
                const double o = om[d];
#pragma unroll
                for (int u = 0; u < 8; u++) paths_dd_fma(o, Xs[(rb + 8 * u) * D + d], s[u], c[u]);
            }
#pragma unroll
            for (int u = 0; u < 8; u++) g[u] = k < a.F ? a.amp * paths_cos(s[u], c[u]) : 0.0;
        } else {
            const int i = kb - a.Fp + kl;
            const bool live = i < a.N;
            const double *xi = a.X + (size_t)(live ? i : 0) * a.ldx;
            double z[8];
#pragma unroll
            for (int u = 0; u < 8; u++) z[u] = 0.0;
            for (int d = 0; d < D; d++) {
                const double x = xi[d], w = a.kp.w[d];
#pragma unroll
                for (int u = 0; u < 8; u++) { const double df = x - Xs[(rb + 8 * u) * D + d]; z[u] = fma(w * df, df, z[u]); }
            }
#pragma unroll
            for (int u = 0; u < 8; u++) g[u] = live ? cov_from_z_rt(a.kp.family, z[u], a.kp.sf2) : 0.0;
        }
#pragma unroll
        for (int u = 0; u < 8; u++) { As[(rb + 8 * u) * PT_LDA + kl] = g[u]; Bs[br * PT_LDB + bc + u] = bv[u]; }
        __syncthreads();
#pragma unroll
        for (int kk = 0; kk < PT_KB; kk += 4) {
            const int ko = kk + (lane >> 4), ro = lane & 15;
            const double a0 = As[(32 * wr + ro) * PT_LDA + ko], a1 = As[(32 * wr + 16 + ro) * PT_LDA + ko];
            const double b0 = Bs[ko * PT_LDB + 32 * wc + ro], b1 = Bs[ko * PT_LDB + 32 * wc + 16 + ro];
            acc[0][0] = mfma_f64(a0, b0, acc[0][0]);
            acc[0][1] = mfma_f64(a0, b1, acc[0][1]);
            acc[1][0] = mfma_f64(a1, b0, acc[1][0]);
            acc[1][1] = mfma_f64(a1, b1, acc[1][1]);
        }
        __syncthreads();
    }
#pragma unroll
    for (int i = 0; i < 2; i++)
#pragma unroll
        for (int j = 0; j < 2; j++)
#pragma unroll
            for (int e = 0; e < 4; e++)
                T[(32 * wc + 16 * j + (lane & 15)) * 65 + 32 * wr + 16 * i + (lane >> 4) + 4 * e] = acc[i][j][e];
    const bool pr = a.prior.nb > 0;
    if (pr && t < 64) ms[t] = prior_mean_dev(a.prior, D, [&](int j) { return Xs[t * D + j]; });
    __syncthreads();
    const int64_t x = (int64_t)r0 + lane;
    const bool valid = x < a.m;
    for (int cc = 0; cc < 16; cc++) {
        const int col = wv * 16 + cc, s = ct * a.pt + col;
        if (col >= a.pt || s >= a.S || (a.only >= 0 && s != a.only)) continue;         // (the same for every lane of the wave)
        double v = T[col * 65 + lane];
        if (pr) { const double m = ms[lane], s1 = T[63 * 65 + lane]; v = m + v - m * s1; }
        const int row = a.only >= 0 ? 0 : s;
        if (a.values && valid) {
            double *o = a.values + (size_t)row * a.ldv + a.voff + x;
            *o = a.accumulate ? *o + v : v;
        }
        if (a.part_val) {
            double bv = v;
            int64_t bi = a.index_base + a.first + x;
            if (!valid || !(v == v)) { bv = -INFINITY; bi = INT64_MAX; }
            wave_argmax(bv, bi);
            if (lane == 0) {
                const size_t o = (size_t)row * a.nblk + a.first / 64 + blockIdx.y;
                a.part_val[o] = bv; a.part_idx[o] = bi;
            }
        }
    }
}

// The gradient of the same tile: one workgroup per 64 points x 64 coefficient columns x PG_DC dimensions, the K loop of the value kernel.
// Per (point, k) the expensive factor is generated ONCE -- a feature's -amp sin(t) (t in the value kernel's double-double, paths_reduce's
// reduction), a model row's h_i (grad_kstar_kernel's, from z by differences) -- and per dimension of the chunk multiplied by omega_kd or by
// w_d (x_d - X_id), staged into that dimension's own 64 x 32 piece and contracted into that dimension's own accumulators.  With a mean
// prior k* itself is staged too and contracted with the tile's last column alone (s1 = k*.a1, on the waves that hold it).  A sum's k order
// does not depend on the chunk, so neither do its bits.  One wave per SIMD: PG_DC accumulator sets of 32 registers each.
__global__ void __launch_bounds__(256) paths_grad_tile_kernel(PathsGradArgs ga)
{
    extern __shared__ double pt_lds[];
    __shared__ double ms[64], s1s[64], dms[PG_DC * 64];
    const PathsArgs &a = ga.a;
    const int D = a.kp.D;
    double *Xs = pt_lds;                       // 64 x D: this tile's points (zeros beyond m)
    double *As = Xs + 64 * D;                  // PG_DC pieces of 64 x PT_LDA, one per dimension of the chunk
    double *Ks = As + PG_DC * 64 * PT_LDA;     // 64 x PT_LDA: k* (read with a mean prior only)
    double *Bs = Ks + 64 * PT_LDA;             // PT_KB x PT_LDB
    double *T = As;                            // the epilogue's 64 x 65 tile, column-major, one dimension at a time
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6, wr = wv >> 1, wc = wv & 1;
    const int r0 = blockIdx.y * 64, ct = blockIdx.x, c0 = ct * 64, d0 = blockIdx.z * PG_DC, nd = min(PG_DC, D - d0);
    const bool pr = a.prior.nb > 0;
    for (int e = t; e < 64 * D; e += 256) {
        const int r = e / D, d = e - r * D;
        Xs[e] = (r0 + r < a.m) ? a.cand[(size_t)(r0 + r) * a.ldc + d] : 0.0;
    }
    d4_t acc[PG_DC][2][2], accv[2];
#pragma unroll
    for (int j = 0; j < PG_DC; j++)
#pragma unroll
        for (int i = 0; i < 2; i++) { acc[j][i][0] = d4_t{0.0, 0.0, 0.0, 0.0}; acc[j][i][1] = d4_t{0.0, 0.0, 0.0, 0.0}; }
    accv[0] = accv[1] = d4_t{0.0, 0.0, 0.0, 0.0};
    __syncthreads();
    const int kl = t & 31, rb = t >> 5;                    // generation: k = kb + kl, points rb + 8 u
    const int br = t >> 3, bc = (t & 7) * 8;               // coefficient staging: row kb + br, columns c0 + bc .. + 7
    for (int kb = 0; kb < a.kend; kb += PT_KB) {
        const bool feat = kb < a.Fp;
        const double *bp = a.coef + (size_t)(kb + br) * a.Sp + c0 + bc;
        double bv[8];
#pragma unroll
        for (int u = 0; u < 8; u++) bv[u] = bp[u];
        double f[8];
        if (feat) {
            const int k = kb + kl;
            const double *om = a.omega + (size_t)k * D;
            const double ph = a.phase[k];
            double s[8], c[8];
#pragma unroll
            for (int u = 0; u < 8; u++) { s[u] = ph; c[u] = 0.0; }
            for (int d = 0; d < D; d++) {
                const double o = om[d];
#pragma unroll
                for (int u = 0; u < 8; u++) paths_dd_fma(o, Xs[(rb + 8 * u) * D + d], s[u], c[u]);
            }
#pragma unroll
            for (int u = 0; u < 8; u++) f[u] = k < a.F ? -(a.amp * paths_sin(s[u], c[u])) : 0.0;
#pragma unroll
            for (int j = 0; j < PG_DC; j++)
                if (j < nd) {
                    const double o = om[d0 + j];
#pragma unroll
                    for (int u = 0; u < 8; u++) As[(j * 64 + rb + 8 * u) * PT_LDA + kl] = f[u] * o;
                }
        } else {
            const int i = kb - a.Fp + kl;
            const bool live = i < a.N;
            const double *xi = a.X + (size_t)(live ? i : 0) * a.ldx;
            double z[8];
#pragma unroll
            for (int u = 0; u < 8; u++) z[u] = 0.0;
            for (int d = 0; d < D; d++) {
                const double x = xi[d], w = a.kp.w[d];
#pragma unroll
                for (int u = 0; u < 8; u++) { const double df = x - Xs[(rb + 8 * u) * D + d]; z[u] = fma(w * df, df, z[u]); }
            }
            const double sf2 = a.kp.sf2;
#pragma unroll
            for (int u = 0; u < 8; u++) {
                double k, h;
                if (a.kp.family == FAM_SE) {
                    k = sf2 * exp(-0.5 * z[u]);
                    h = -k;
                } else if (a.kp.family == FAM_M3) {
                    const double r = sqrt(3.0 * z[u]), e = exp(-r);
                    k = sf2 * (1.0 + r) * e;
                    h = -3.0 * sf2 * e;
                } else {
                    const double r = sqrt(5.0 * z[u]), e = exp(-r);
                    k = sf2 * (1.0 + r + r * r * (1.0 / 3.0)) * e;
                    h = -(5.0 / 3.0) * sf2 * (1.0 + r) * e;
                }
                f[u] = live ? h : 0.0;
                if (pr) Ks[(rb + 8 * u) * PT_LDA + kl] = live ? k : 0.0;
            }
#pragma unroll
            for (int j = 0; j < PG_DC; j++)
                if (j < nd) {
                    const double x = xi[d0 + j], w = a.kp.w[d0 + j];
#pragma unroll
                    for (int u = 0; u < 8; u++) As[(j * 64 + rb + 8 * u) * PT_LDA + kl] = f[u] * (w * (Xs[(rb + 8 * u) * D + d0 + j] - x));
                }
        }
#pragma unroll
        for (int u = 0; u < 8; u++) Bs[br * PT_LDB + bc + u] = bv[u];
        __syncthreads();
        const bool s1 = pr && !feat && wc == 1;              // (the same for every lane of the wave)
#pragma unroll
        for (int kk = 0; kk < PT_KB; kk += 4) {
            const int ko = kk + (lane >> 4), ro = lane & 15;
            const double b0 = Bs[ko * PT_LDB + 32 * wc + ro], b1 = Bs[ko * PT_LDB + 32 * wc + 16 + ro];
#pragma unroll
            for (int j = 0; j < PG_DC; j++)
                if (j < nd) {
                    const double a0 = As[(j * 64 + 32 * wr + ro) * PT_LDA + ko], a1 = As[(j * 64 + 32 * wr + 16 + ro) * PT_LDA + ko];
                    acc[j][0][0] = mfma_f64(a0, b0, acc[j][0][0]);
                    acc[j][0][1] = mfma_f64(a0, b1, acc[j][0][1]);
                    acc[j][1][0] = mfma_f64(a1, b0, acc[j][1][0]);
                    acc[j][1][1] = mfma_f64(a1, b1, acc[j][1][1]);
                }
            if (s1) {
                accv[0] = mfma_f64(Ks[(32 * wr + ro) * PT_LDA + ko], b1, accv[0]);
                accv[1] = mfma_f64(Ks[(32 * wr + 16 + ro) * PT_LDA + ko], b1, accv[1]);
            }
        }
        __syncthreads();
    }
    if (pr) {
        for (int e = t; e < 64 * nd; e += 256) {
            const int x = e & 63, j = e >> 6;
            double dm;
            const double m = prior_mean_dev(a.prior, D, [&](int q) { return Xs[x * D + q]; }, d0 + j, &dm);
            dms[e] = dm;
            if (j == 0) ms[x] = m;
        }
        if (wc == 1 && (lane & 15) == 15)                   // column 63 of the tile: k*.a1 of the wave's 32 points
#pragma unroll
            for (int i = 0; i < 2; i++)
#pragma unroll
                for (int e = 0; e < 4; e++) s1s[32 * wr + 16 * i + (lane >> 4) + 4 * e] = accv[i][e];
    }
    const int64_t x = (int64_t)r0 + lane;
    const bool valid = x < a.m;
    const int po = (ga.path_of && valid) ? ga.path_of[x] : -1;
#pragma unroll
    for (int j = 0; j < PG_DC; j++) {
        if (j >= nd) continue;                               // (the same for the whole workgroup)
        __syncthreads();
#pragma unroll
        for (int i = 0; i < 2; i++)
#pragma unroll
            for (int jj = 0; jj < 2; jj++)
#pragma unroll
                for (int e = 0; e < 4; e++)
                    T[(32 * wc + 16 * jj + (lane & 15)) * 65 + 32 * wr + 16 * i + (lane >> 4) + 4 * e] = acc[j][i][jj][e];
        __syncthreads();
        for (int cc = 0; cc < 16; cc++) {
            const int col = wv * 16 + cc, s = ct * a.pt + col;
            if (col >= a.pt || s >= a.S) continue;           // (the same for every lane of the wave)
            double v = T[col * 65 + lane];
            if (pr) v = dms[j * 64 + lane] * (1.0 - s1s[lane]) + v - ms[lane] * T[63 * 65 + lane];
            if (!valid) continue;
            if (ga.path_of) {
                if (s == po) ga.grads[(size_t)(ga.goff + x) * D + d0 + j] = v;
            } else {
                ga.grads[((size_t)s * ga.ldg + ga.goff + x) * D + d0 + j] = v;
            }
        }
    }
}

// out[i] = vals[path_of[i]][i]: the value of a point's own path out of the path-major block
__global__ void __launch_bounds__(256) paths_pick_kernel(const double *__restrict__ vals, size_t ldv, const int *__restrict__ path_of, int m,
                                                         double *__restrict__ out)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < m) out[i] = vals[(size_t)path_of[i] * ldv + i];
}

__global__ void __launch_bounds__(256) paths_solve_kernel(const double *__restrict__ W, int Np, int N, const double *__restrict__ Y, size_t ldy,
                                                          int S, int pt, const double *__restrict__ aY, const double *__restrict__ a1,
                                                          double *__restrict__ coef, int Sp, int Fp)
{
    const int j = blockIdx.x * 256 + threadIdx.x, s0 = blockIdx.y * 8;
    double z[8];
#pragma unroll
    for (int u = 0; u < 8; u++) z[u] = 0.0;
    for (int i = blockIdx.x * 256; i < N; i++) {             // (a uniform loop: the rows above this thread's own add nothing)
        if (i < j || j >= N) continue;
        const double w = W[(size_t)i * Np + j];
#pragma unroll
        for (int u = 0; u < 8; u++) z[u] = fma(w, Y[(size_t)(s0 + u) * ldy + i], z[u]);
    }
    if (j >= N) return;
    double *row = coef + (size_t)(Fp + j) * Sp;
#pragma unroll
    for (int u = 0; u < 8; u++)
        if (s0 + u < S) row[64 * ((s0 + u) / pt) + (s0 + u) % pt] = aY[j] - z[u];
    if (pt == 63 && blockIdx.y == 0)
        for (int c = 63; c < Sp; c += 64) row[c] = a1[j];
}

// one workgroup per path: its partials in a 256-stride loop, then block256_argmax into out[path] (INT64_MAX where nothing is admissible)
__global__ __launch_bounds__(256) void paths_final_kernel(const double *__restrict__ pv, const int64_t *__restrict__ pi, int64_t n,
                                                          double *out_v, int64_t *out_i)
{
    pv += (size_t)blockIdx.x * n; pi += (size_t)blockIdx.x * n;
    double v = -INFINITY;
    int64_t i = INT64_MAX;
    for (int64_t e = threadIdx.x; e < n; e += 256) {
        const double ov = pv[e]; const int64_t oi = pi[e];
        if (ov > v || (ov == v && oi < i)) { v = ov; i = oi; }
    }
    block256_argmax(v, i, out_v, out_i);
}

int launch_paths_tile(const PathsArgs &a, hipStream_t s)
{
    const int D = a.kp.D;
    if (a.m < 1 || a.m > 64 * 65535 || D < 1 || D > IBO_DMAX || (a.Fp & (PT_KB - 1)) || (a.kend & (PT_KB - 1)) || (a.Sp & 63) || (a.first & 63) ||
        a.F < 1 || a.F > a.Fp || a.kend < a.Fp || a.S < 1 || (a.pt != 63 && a.pt != 64) || (a.prior.nb > 0 && a.pt != 63) ||
        (a.S + a.pt - 1) / a.pt * 64 > a.Sp || a.only >= a.S)
        return (int)hipErrorInvalidValue;
    const size_t lds = sizeof(double) * ((size_t)64 * D + 64 * PT_LDA + PT_KB * PT_LDB);
    if (lds > 48 * 1024) {
        hipError_t e = hipFuncSetAttribute((const void *)paths_tile_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return (int)e;
    }
    const int ntile = a.only >= 0 ? 1 : (a.S + a.pt - 1) / a.pt;
    hipLaunchKernelGGL(paths_tile_kernel, dim3(ntile, (a.m + 63) / 64), dim3(256), lds, s, a);
    return (int)hipGetLastError();
}

int launch_paths_grad_tile(const PathsGradArgs &ga, hipStream_t s)
{
    const PathsArgs &a = ga.a;
    const int D = a.kp.D;
    if (a.m < 1 || a.m > 64 * 65535 || D < 1 || D > IBO_DMAX || (a.Fp & (PT_KB - 1)) || (a.kend & (PT_KB - 1)) || (a.Sp & 63) || a.F < 1 ||
        a.F > a.Fp || a.kend < a.Fp || a.S < 1 || (a.pt != 63 && a.pt != 64) || (a.prior.nb > 0 && a.pt != 63) ||
        (a.S + a.pt - 1) / a.pt * 64 > a.Sp || !ga.grads || ga.goff < 0 || (!ga.path_of && (size_t)(ga.goff + a.m) > ga.ldg))
        return (int)hipErrorInvalidValue;
    const size_t lds = sizeof(double) * ((size_t)64 * D + (PG_DC + 1) * 64 * PT_LDA + PT_KB * PT_LDB);
    hipError_t e = hipFuncSetAttribute((const void *)paths_grad_tile_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(paths_grad_tile_kernel, dim3((a.S + a.pt - 1) / a.pt, (a.m + 63) / 64, (D + PG_DC - 1) / PG_DC), dim3(256), lds, s, ga);
    return (int)hipGetLastError();
}

int launch_paths_pick(const double *vals, size_t ldv, const int *path_of, int m, double *out, hipStream_t s)
{
    if (m < 1) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(paths_pick_kernel, dim3((m + 255) / 256), dim3(256), 0, s, vals, ldv, path_of, m, out);
    return (int)hipGetLastError();
}

int launch_paths_solve(const double *W, int Np, int N, const double *Y, size_t ldy, int S, int pt, const double *aY, const double *a1,
                       double *coef, int Sp, int Fp, hipStream_t s)
{
    if (N < 1 || S < 1) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(paths_solve_kernel, dim3((N + 255) / 256, (S + 7) / 8), dim3(256), 0, s, W, Np, N, Y, ldy, S, pt, aY, a1, coef, Sp, Fp);
    return (int)hipGetLastError();
}

int launch_paths_final(const double *part_val, const int64_t *part_idx, int64_t nblk, int S, double *out_val, int64_t *out_idx,
                       hipStream_t s)
{
    if (nblk < 1 || S < 1) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(paths_final_kernel, dim3(S), dim3(256), 0, s, part_val, part_idx, nblk, out_val, out_idx);
    return (int)hipGetLastError();
}

void ibo_touch_paths() { hipFuncAttributes a; (void)hipFuncGetAttributes(&a, (const void *)paths_tile_kernel); }     // (see small2.hip: ibo_touch_small2)

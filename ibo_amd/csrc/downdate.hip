// downdate.hip -- one observation taken out of a fitted model in O(N^2) (ibo_gp_remove): the rank-one update of the trailing factor and of
// its inverse as two scans over what the handle holds (downdate.h has the formulas).
//
//   downdate_scalars_kernel  p, d, q, 1 / d: one workgroup; t_{k+1} = t_k + p_k^2 is ONE sequential sum in index order (lane 0, the p's of a
//                            1024-chunk staged in LDS), everything else elementwise
//   downdate_L_kernel        a workgroup owns 64 consecutive rows of L' and walks the 64-column tiles from the diagonal tile leftwards to
//                            column 0.  A tile goes global -> registers (coalesced along rows, the next tile's loads in flight during the
//                            scan) -> LDS -> scan -> LDS -> global.  The scan: lane r of the first wave carries row r's running
//                            s = sum_{j > k} p_j L33[r][j], added right to left one column at a time (plain fma), and turns L33[r][k] into
//                            d_k L33[r][k] + q_k s.  Rows above i and columns left of i are copies.
//   downdate_W_*             a lane owns a column of W', a workgroup (one wave) a 64 x 64 tile on or below the diagonal, so the chip is filled
//                            by tiles rather than by N threads: the rows are split into the FIXED segments of 64 output rows (a function of
//                            Npad only).  _part: each tile's sum_k p_k W~[k][c] over its rows, top to bottom.  _prefix: per column the
//                            exclusive running sum of those partial sums in segment order, top to bottom.  _apply: S starts at that value
//                            and continues row by row: W'[j][c] = W~[j][c] / d_j - q_j S, S += p_j W~[j][c].
//                            So S of a row is ((segment sums added in segment order) + the rows of its own segment in row order): the
//                            same association for the same Npad and i, whatever the launch.
// No MFMA work here: both scans are bandwidth- and latency-bound.  No atomics except the info word.  64-bit addresses only.
#include "downdate.h"

#define DD_LD 65                 // LDS row stride of a 64 x 64 tile in doubles (odd: a column walk and a row walk are both conflict-free)

size_t downdate_scratch(int Npad) { return 4 * (size_t)Npad + (size_t)(Npad / 64) * Npad; }

__global__ void __launch_bounds__(1024) downdate_scalars_kernel(const double *__restrict__ W, int N, int Npad, int i, double *__restrict__ p,
                                                                double *__restrict__ d, double *__restrict__ q, double *__restrict__ rd,
                                                                int *info)
{
    __shared__ double ps[1024], ts[1025];
    const int t = threadIdx.x, m = N - 1 - i;
    const double wii = W[(size_t)i * Npad + i];
    if (!(isfinite(wii) && wii > 0.0)) { if (t == 0) atomicCAS(info, 0, i + 1); return; }
    if (t == 0) ts[0] = 1.0;
    bool bad = false;
    for (int base = 0; base < m; base += 1024) {
        const int n = m - base < 1024 ? m - base : 1024;
        double pk = 0.0;
        if (t < n) { pk = -W[(size_t)(i + 1 + base + t) * Npad + i] / wii; ps[t] = pk; }
        __syncthreads();
        if (t == 0) {                                   // the one sequential sum, in index order
            double tk = ts[0];
#pragma unroll 8
            for (int k = 0; k < n; k++) { tk = fma(ps[k], ps[k], tk); ts[k + 1] = tk; }
        }
        __syncthreads();
        if (t < n) {
            const double tk = ts[t], tn = ts[t + 1], dk = sqrt(tn / tk);
            bad |= !isfinite(tn);
            p[base + t] = pk; d[base + t] = dk; q[base + t] = pk / sqrt(tk * tn); rd[base + t] = 1.0 / dk;
        }
        __syncthreads();
        if (t == 0) ts[0] = ts[n];
    }
    if (bad) atomicCAS(info, 0, i + 1);
}

// blockIdx.x: the 64-row block of L' (output rows R0 .. R0 + 63).  Output (r', c') comes from source (r' + (r' >= i), c' + (c' >= i)).
__global__ void __launch_bounds__(256) downdate_L_kernel(const double *__restrict__ L, int N, int Npad, int i, const double *__restrict__ ws,
                                                         double *__restrict__ Lout)
{
    __shared__ double tile[64 * DD_LD];
    __shared__ double pdq[3 * 64];                       // p | d | q of the tile's columns
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
    const int R0 = blockIdx.x * 64, N1 = N - 1, m = N1 - i;
    double v[16], sc = 0.0;
    auto fetch = [&](int C0) {
        const int cp = C0 + lane, c = cp + (cp >= i ? 1 : 0);
#pragma unroll
        for (int u = 0; u < 16; u++) {
            const int rp = R0 + wv + 4 * u, r = rp + (rp >= i ? 1 : 0);
            if (rp < N1 && cp <= rp) v[u] = L[(size_t)r * Npad + c];             // r <= N - 1, c <= r
            else v[u] = (rp >= N1 && rp == cp) ? 1.0 : 0.0;                      // above the diagonal: zero; the pad: identity
        }
        if (wv < 3) { const int k = cp - i; sc = (k >= 0 && k < m) ? ws[(size_t)wv * Npad + k] : 0.0; }
    };
    const int rp = R0 + lane;                            // the scan's row (first wave)
    const bool trailing = rp >= i && rp < N1;
    double s = 0.0;
    fetch(R0);
    for (int C0 = R0; C0 >= 0; C0 -= 64) {
#pragma unroll
        for (int u = 0; u < 16; u++) tile[(wv + 4 * u) * DD_LD + lane] = v[u];
        if (wv < 3) pdq[wv * 64 + lane] = sc;
        __syncthreads();
        if (C0 > 0) fetch(C0 - 64);                      // in flight during the scan
        if (wv == 0 && R0 + 63 >= i && R0 < N1 && C0 + 63 >= i) {
            for (int cc = 63; cc >= 0; cc--) {
                const int cp = C0 + cc;
                if (cp < i || cp >= N1) continue;        // (uniform) a copied column, or the pad
                const double x = tile[lane * DD_LD + cc], pk = pdq[cc], dk = pdq[64 + cc], qk = pdq[128 + cc];
                if (trailing) tile[lane * DD_LD + cc] = fma(qk, s, dk * x);
                s = fma(pk, x, s);
            }
        }
        __syncthreads();
#pragma unroll
        for (int u = 0; u < 16; u++)
            Lout[(size_t)(R0 + wv + 4 * u) * Npad + C0 + lane] = tile[(wv + 4 * u) * DD_LD + lane];
        __syncthreads();
    }
}

// W~[r'][c'] of output row r' (i <= r' < N - 1) and output column c' (< N - 1) = W[r' + 1][c' + (c' >= i)] + p_{r' - i} wi with wi = W[i][c']
// for c' < i, else 0 (W[i][c] = 0 right of the diagonal: one formula for the columns left and right of i).  Zero above the diagonal.
// blockIdx.x: column tile, blockIdx.y: row segment (64 output rows).  part[seg * Npad + c'] = sum over the segment's rows of p_k W~[k][c'],
// top to bottom.  Segments above row i's and tiles above the diagonal have nothing to add and are never read.
__global__ void __launch_bounds__(64) downdate_W_part_kernel(const double *__restrict__ W, int N, int Npad, int i, const double *__restrict__ p,
                                                             double *__restrict__ part)
{
    __shared__ double pr[64];
    const int lane = threadIdx.x, CB = blockIdx.x, RB = blockIdx.y, R0 = RB * 64, N1 = N - 1;
    if (CB > RB || R0 + 63 < i || R0 >= N1) return;
    const int cp = CB * 64 + lane, c = cp + (cp >= i ? 1 : 0);
    { const int k = R0 + lane - i; pr[lane] = (k >= 0 && R0 + lane < N1) ? p[k] : 0.0; }
    __syncthreads();
    const bool live = cp < N1;
    const double wi = (live && cp < i) ? W[(size_t)i * Npad + cp] : 0.0;
    double S = 0.0;
#pragma unroll
    for (int r0 = 0; r0 < 64; r0 += 16) {                // sixteen rows' loads in flight, added in row order
        double w[16];
#pragma unroll
        for (int u = 0; u < 16; u++) {
            const int rp = R0 + r0 + u;
            w[u] = (live && rp >= i && rp < N1 && cp <= rp) ? W[(size_t)(rp + 1) * Npad + c] : 0.0;
        }
#pragma unroll
        for (int u = 0; u < 16; u++) {
            const double pk = pr[r0 + u];                // zero outside [i, N - 1): such a row adds an exact zero
            S = fma(pk, fma(pk, wi, w[u]), S);
        }
    }
    part[(size_t)RB * Npad + cp] = S;
}

// per column: part[seg][c'] becomes the sum of the segments before it, in segment order from the first one that holds a term
__global__ void __launch_bounds__(256) downdate_W_prefix_kernel(int N, int Npad, int i, double *__restrict__ part)
{
    const int cp = blockIdx.x * 256 + threadIdx.x, N1 = N - 1;
    if (cp >= Npad) return;
    const int first = (i >> 6) > (cp >> 6) ? (i >> 6) : (cp >> 6), nseg = (N1 + 63) / 64;
    double run = 0.0;
    for (int s0 = first; s0 < nseg; s0 += 8) {           // eight loads in flight, added in segment order
        double v[8];
#pragma unroll
        for (int u = 0; u < 8; u++) v[u] = s0 + u < nseg ? part[(size_t)(s0 + u) * Npad + cp] : 0.0;
#pragma unroll
        for (int u = 0; u < 8; u++)
            if (s0 + u < nseg) { part[(size_t)(s0 + u) * Npad + cp] = run; run += v[u]; }
    }
}

// blockIdx as in _part; writes the whole 64 x 64 tile of W' (tiles above the diagonal are left alone)
__global__ void __launch_bounds__(64) downdate_W_apply_kernel(const double *__restrict__ W, int N, int Npad, int i, const double *__restrict__ ws,
                                                              const double *__restrict__ part, double *__restrict__ Wout)
{
    __shared__ double pr[64], qr[64], rr[64];
    const int lane = threadIdx.x, CB = blockIdx.x, RB = blockIdx.y, R0 = RB * 64, N1 = N - 1;
    if (CB > RB) return;
    const int cp = CB * 64 + lane, c = cp + (cp >= i ? 1 : 0);
    const bool scan = R0 + 63 >= i && R0 < N1;           // the segment holds rows at or below i
    {
        const int k = R0 + lane - i;
        const bool in = k >= 0 && R0 + lane < N1;
        pr[lane] = in ? ws[k] : 0.0; qr[lane] = in ? ws[2 * (size_t)Npad + k] : 0.0; rr[lane] = in ? ws[3 * (size_t)Npad + k] : 0.0;
    }
    __syncthreads();
    const bool live = cp < N1;
    const double wi = (live && cp < i) ? W[(size_t)i * Npad + cp] : 0.0;
    double S = scan ? part[(size_t)RB * Npad + cp] : 0.0;
#pragma unroll
    for (int r0 = 0; r0 < 64; r0 += 16) {
        double w[16];
#pragma unroll
        for (int u = 0; u < 16; u++) {
            const int rp = R0 + r0 + u, r = rp + (rp >= i ? 1 : 0);
            w[u] = (live && rp < N1 && cp <= rp) ? W[(size_t)r * Npad + c] : 0.0;          // r <= N - 1, c <= r
        }
#pragma unroll
        for (int u = 0; u < 16; u++) {
            const int rp = R0 + r0 + u;
            double out = w[u];                           // rows above i: a copy; the pad: zero
            if (rp >= i && rp < N1) {                    // (uniform)
                const double pk = pr[r0 + u], wt = fma(pk, wi, w[u]);
                out = fma(-qr[r0 + u], S, wt * rr[r0 + u]);
                S = fma(pk, wt, S);
            }
            Wout[(size_t)rp * Npad + cp] = out;
        }
    }
}

__global__ void __launch_bounds__(256) downdate_X_kernel(const double *__restrict__ Xp, int N, int Npad, int DP, int i, double *__restrict__ Xout)
{
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= (size_t)Npad * DP) return;
    const int rp = (int)(e / DP), dd = (int)(e - (size_t)rp * DP);
    Xout[e] = rp < N - 1 ? Xp[(size_t)(rp + (rp >= i ? 1 : 0)) * DP + dd] : 0.0;
}

int launch_downdate_scalars(const double *W, int N, int Npad, int i, double *ws, int *info, hipStream_t s)
{
    hipLaunchKernelGGL(downdate_scalars_kernel, dim3(1), dim3(1024), 0, s, W, N, Npad, i, ws, ws + Npad, ws + 2 * (size_t)Npad, ws + 3 * (size_t)Npad,
                       info);
    return (int)hipGetLastError();
}

int launch_downdate_L(const double *L, int N, int Npad, int i, const double *ws, double *Lout, hipStream_t s)
{
    hipLaunchKernelGGL(downdate_L_kernel, dim3(Npad / 64), dim3(256), 0, s, L, N, Npad, i, ws, Lout);
    return (int)hipGetLastError();
}

int launch_downdate_W(const double *W, int N, int Npad, int i, double *ws, double *Wout, hipStream_t s)
{
    const int nb = Npad / 64;
    double *part = ws + 4 * (size_t)Npad;
    hipLaunchKernelGGL(downdate_W_part_kernel, dim3(nb, nb), dim3(64), 0, s, W, N, Npad, i, (const double *)ws, part);
    hipLaunchKernelGGL(downdate_W_prefix_kernel, dim3((Npad + 255) / 256), dim3(256), 0, s, N, Npad, i, part);
    hipLaunchKernelGGL(downdate_W_apply_kernel, dim3(nb, nb), dim3(64), 0, s, W, N, Npad, i, (const double *)ws, (const double *)part, Wout);
    return (int)hipGetLastError();
}

int launch_downdate_X(const double *Xp, int N, int Npad, int DP, int i, double *Xout, hipStream_t s)
{
    const size_t total = (size_t)Npad * DP;
    hipLaunchKernelGGL(downdate_X_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, Xp, N, Npad, DP, i, Xout);
    return (int)hipGetLastError();
}

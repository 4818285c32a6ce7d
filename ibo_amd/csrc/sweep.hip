// sweep.hip -- the fused candidate sweep on gfx950: for every candidate c
//   k*_i = k(x_i, c);  mu = m(c) + aY.k* - m(c) a1.k*;  q = |W k*|^2;
//   s2 = clamp(1+noise-q);  acq = EI/PI/UCB(mu, sqrt(s2));  arg-max over c.
// It is the batched form of GP_Maximizer::posterior + negei/negpi/negucb
// (cpp/optimizeGP.cpp:57-236) and of GaussianProcess.posterior
// (ego/gaussianprocess/__init__.py:169-228).  K(X, X*) never touches HBM.
//
// Main kernel (sweep_mfma_kernel): one workgroup (16 waves by default) per 64 candidates.
//   * the N x 64 block of k* is produced 32 rows at a time into LDS, already in
//     fp64-MFMA B-fragment order; observation rows are wave-uniform (scalar
//     loads), the candidate sits in registers, one lane per candidate;
//   * W = L^-1 is streamed from L2 in A-fragment order (pack_w_kernel), one
//     16-byte load per lane per two k4-steps, and never staged in LDS: each
//     wave owns distinct rows;
//   * V = W K* is accumulated 512 rows at a time (16 waves x 2 row-blocks of 16
//     x 4 candidate blocks of 16 = 64 accumulator VGPRs per lane); row blocks
//     are interleaved over the waves so the triangular part stays balanced and
//     the zero upper-triangular tiles are skipped;
//   * the epilogue squares and reduces V down the rows, finishes mu/s2/acq and
//     does a wave-level (max, lowest index) reduction -> one partial per tile.
// Small batches (M <= 16) go through a row-parallel GEMV kernel instead.
#include "ibo_common.h"
#include <atomic>
#include <type_traits>

#define TC 64          // candidates per workgroup

// Tile configuration of the main kernel.  NW waves per workgroup, each owning RBW
// row-blocks (16 rows) x 4 candidate-blocks (16 candidates) of the 512-row panel:
// NW * RBW = 32.  KCH = rows of K* per LDS stage.  fp64 MFMA issues at one per 64
// cycles per SIMD but a single wave only reaches ~46 % of that (tools/mfma_f64_peak),
// so the pipe needs >= 2 waves per SIMD in their MFMA phase at any time:
// <16, 2> (64 accumulator VGPRs, 4 waves/SIMD) is the default, <8, 4> the first version.
// (s_setprio around the MFMA block was tried: -9 %, it pins the compiler's schedule.  A persistent
// grid-stride tile loop saves the ~9 us dispatch of each 16-wave workgroup (+2.4 % at N=1024, +12 %
// at N=256) but wrapping the body in a loop, inline or as a noinline callee, costs hipcc 19-35 % in
// register allocation / scheduling of the body, so the one-workgroup-per-tile form stays.  Two 8-wave
// workgroups of 32 candidates per CU -- same work per wave, the idea being that one covers the other's
// dispatch/epilogue -- measured 66 % at N=1024 and no better at N=256: two k* rows per wave instruction
// need per-lane observation loads and the 128-VGPR budget then spills 60-200 registers.)
// DOT: the scaled squared distance as -2 (a_k + b_c + x~.c~) (D+1 FMAs) instead of the
// difference form (2D); for the squared exponential the exp() takes that sum directly -- fp64 VALU shares the MFMA pipe, instruction count is time.
// CBW: candidate-blocks per wave (4: a wave spans the whole tile; 2: waves come in pairs
// that share row-blocks, each wave owning RBW = 4 row-blocks spread over the panel, which
// keeps all 16 waves busy until the last stage of the triangular diagonal block).
// SPLIT: small batches (DIRECT's per-iteration batches, a few hundred points) cannot fill 256
// CUs with one workgroup per 64 candidates, so the row panels (PANEL rows each) are spread over
// blockIdx.y as well; every workgroup writes its panel's partial |V|^2 (and the last panel the
// mean) and sweep_gemv_finish_kernel sums the partials in a fixed order.
template <int FAM, int DP, int NW, int RBW, int CBW, int KCH, bool DOT, int PANEL = 512, bool SPLIT = false>
__global__ __launch_bounds__(NW * 64) void sweep_mfma_kernel(SweepArgs a)
{
    constexpr int CG = 4 / CBW;                    // candidate groups of waves
    constexpr int RG = NW / CG;                    // row groups of waves
    static_assert(RG * RBW * 16 == PANEL, "waves x row-blocks must tile the panel");
    constexpr int KPW = KCH / NW;                  // K* rows generated per wave per stage
    static_assert(KPW >= 1 && KPW <= 4 && (4 % KPW == 0), "wave generates 1, 2 or 4 rows of a k4-step");
    __shared__ double lds_k[2][KCH * TC];          // K* stage, B-fragment order
    __shared__ double lds_c[DP * TC];              // candidate coordinates, [d][candidate]
    __shared__ double lds_q[NW][TC];
    __shared__ double lds_m[2][NW][TC];

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int64_t tile0 = (int64_t)blockIdx.x * TC;
    const int D = a.kp.D;
#ifdef IBO_STAMPS   // diagnostic build (tools/stamp_sweep.py): where does a tile's time go?
    unsigned long long cyc[6] = {0, 0, 0, 0, 0, 0}; unsigned nst[2] = {0, 0};   // shader cycles: k* gen / MFMA / barrier, plain and diagonal stages
    unsigned long long st[8];
#define STAMP(i) st[i] = __builtin_amdgcn_s_memrealtime()
    STAMP(0);
#else
#define STAMP(i)
#endif

    for (int e = tid; e < TC * DP; e += NW * 64) {
        int d = e / TC, c = e - d * TC;
        int64_t gi = tile0 + c;
        if (gi > a.M - 1) gi = a.M - 1;
        lds_c[e] = (d < D) ? a.cand[gi * D + d] * a.kp.sw[d] : 0.0;     // pre-scaled: c~_d = c_d sqrt(w_d)
    }
    __syncthreads();
    constexpr bool CX_REG = (DP <= 8);             // keep the candidate in registers when it is small
    double cx[CX_REG ? DP : 1];
    double bc;                                      // log sf2 - |c~|^2 / 2   (dot form)
    {
        double n2 = 0.0;
#pragma unroll
        for (int d = 0; d < DP; d++) {
            double v = lds_c[d * TC + lane];
            n2 = fma(v, v, n2);
            if (CX_REG) cx[CX_REG ? d : 0] = v;
        }
        bc = fma(-0.5, n2, FAM == FAM_SE ? a.log_sf2 : 0.0);
    }
    STAMP(1);

    const int Npad = a.Npad;                        // multiple of 64 >= KCH: stages never run past it
    const int nk8 = Npad >> 3;
    const int nRB = Npad >> 4;
    const int npanel = (Npad + PANEL - 1) / PANEL;
    const double2 *Wp2 = (const double2 *)a.Wp;
    double muY = 0.0, mu1 = 0.0;
    double qacc[CBW];                               // lanes 0..15 hold sums for candidate block cg*CBW + cb
#pragma unroll
    for (int cb = 0; cb < CBW; cb++) qacc[cb] = 0.0;
    // this wave's slot in a stage: rows kl0 .. kl0+KPW-1, written in B-fragment order
    const int cg = wave % CG, rg = wave / CG;       // this wave's candidate group / row group
    const int kl0 = wave * KPW;
    const int wr_off = ((kl0 >> 2) * 4 + (lane >> 4)) * 64 + (kl0 & 3) * 16 + (lane & 15);

    // produce K* rows [k0, k0+KCH) into stage b (LAST: also accumulate the mean)
    auto gen = [&](int k0, int b, auto last_tag) {
        constexpr bool LAST = decltype(last_tag)::value;
        if constexpr (DP > 8) {
            // 9..32 dimensions: the candidate's coordinates come from LDS and the row's scaled observation coordinates
            // from SGPRs.  With the KPW rows unrolled side by side and all of a row's coordinates loaded at once (32 or
            // 64 SGPRs) hipcc spilled up to ~470 registers (SGPRs into VGPR lanes, then VGPRs to scratch): 40 % of the
            // MFMA rate for the Matern kernels at DP = 16.  Rows one at a time, coordinates eight at a time (16 SGPRs):
            // 36 B of scratch per lane, 67-69 % for every family at DP = 16, 58-61 % at DP = 32.
#pragma unroll 1
            for (int kk = 0; kk < KPW; kk++) {
                const int k = k0 + kl0 + kk;
                const double *xr = a.Xs + (size_t)k * DP;
                double kv;
                constexpr int DCH = 8;                     // coordinates in SGPRs at a time
                if (DOT) {
                    double y = a.ak[k] + bc;
#pragma unroll 1
                    for (int d0 = 0; d0 < DP; d0 += DCH) {
#pragma unroll
                        for (int d = d0; d < d0 + DCH; d++) y = fma(xr[d], lds_c[d * TC + lane], y);
                    }
                    if (FAM == FAM_SE) kv = exp_fast(y);
                    else kv = cov_from_z_fast<FAM>(fmax(-2.0 * y, 0.0), a.log_sf2, a.kp.sf2);
                } else {
                    double z = 0.0;
#pragma unroll 1
                    for (int d0 = 0; d0 < DP; d0 += DCH) {
#pragma unroll
                        for (int d = d0; d < d0 + DCH; d++) {
                            double t = xr[d] - lds_c[d * TC + lane];
                            z = fma(t, t, z);
                        }
                    }
                    kv = cov_from_z_fast<FAM>(z, a.log_sf2, a.kp.sf2);
                }
                if (LAST) {
                    muY = fma(a.alphaY[k], kv, muY);
                    mu1 = fma(a.alpha1[k], kv, mu1);
                }
                lds_k[b][wr_off + kk * 16] = kv;
            }
            return;
        }
#pragma unroll
        for (int kk = 0; kk < KPW; kk++) {
            const int k = k0 + kl0 + kk;
            const double *xr = a.Xs + (size_t)k * DP;
            double kv;
            if (DOT) {
                double y = a.ak[k] + bc;
#pragma unroll
                for (int d = 0; d < DP; d++) y = fma(xr[d], CX_REG ? cx[CX_REG ? d : 0] : lds_c[d * TC + lane], y);
                if (FAM == FAM_SE) kv = exp_fast(y);
                else kv = cov_from_z_fast<FAM>(fmax(-2.0 * y, 0.0), a.log_sf2, a.kp.sf2);   // z = |x~ - c~|^2 = -2y
            } else {
                double z = 0.0;
#pragma unroll
                for (int d = 0; d < DP; d++) {
                    double t = xr[d] - (CX_REG ? cx[CX_REG ? d : 0] : lds_c[d * TC + lane]);
                    z = fma(t, t, z);
                }
                kv = cov_from_z_fast<FAM>(z, a.log_sf2, a.kp.sf2);
            }
            if (LAST) {
                muY = fma(a.alphaY[k], kv, muY);
                mu1 = fma(a.alpha1[k], kv, mu1);
            }
            lds_k[b][wr_off + kk * 16] = kv;
        }
    };

    // Panel p covers rows [row0, row1) and needs k in [0, row1).  When Npad is not a multiple of
    // the panel, the short panel comes FIRST (rows [0, rem)): there it only costs its own few
    // stages, whereas as the last panel it would regenerate every k* row for a handful of rows.
    const int rem = Npad % PANEL;
    auto run_panel = [&](int p, auto last_tag, auto partial_tag) {
        constexpr bool PARTIAL = decltype(partial_tag)::value;
        const int row0 = (rem == 0) ? p * PANEL : (p == 0 ? 0 : rem + (p - 1) * PANEL);
        const int row1 = (rem == 0) ? row0 + PANEL : (p == 0 ? rem : row0 + PANEL);
        const int kend = row1;
        const int nchunk = kend / KCH;
        const int nfull = row0 / KCH;               // stages strictly left of the diagonal block
        int g[RBW];
        bool keep[RBW];
        const double2 *wrow[RBW];
#pragma unroll
        for (int i = 0; i < RBW; i++) {
            g[i] = (row0 >> 4) + rg + RG * i;
            keep[i] = 16 * g[i] < row1;             // row-block exists (the short panel has fewer)
            wrow[i] = Wp2 + ((size_t)min(g[i], nRB - 1) * nk8) * 64 + lane;
        }
        d4_t acc[RBW][CBW];
#pragma unroll
        for (int i = 0; i < RBW; i++)
#pragma unroll
            for (int cb = 0; cb < CBW; cb++) acc[i][cb] = (d4_t){0.0, 0.0, 0.0, 0.0};

        gen(0, 0, last_tag);
        __syncthreads();
        // One stage: A operands are loaded unconditionally (the tiles above the diagonal are
        // stored as zeros) and prefetched one k8-step ahead; with DIAG the MFMAs of all-zero
        // tiles are skipped (row-block g has non-zeros in columns <= 16 g + 15).
        auto stage = [&](int t, auto diag_tag) {
            constexpr bool DIAG = decltype(diag_tag)::value;
#ifdef IBO_STAMPS
            const unsigned long long c0 = __builtin_amdgcn_s_memtime();
#endif
            const int b = t & 1;
            const int j0 = (t * KCH) >> 3;
            double2 af[RBW];
#pragma unroll
            for (int i = 0; i < RBW; i++) af[i] = wrow[i][(size_t)j0 * 64];
            if (t + 1 < nchunk) gen((t + 1) * KCH, b ^ 1, last_tag);
#ifdef IBO_STAMPS
            const unsigned long long c1 = __builtin_amdgcn_s_memtime();
#endif
#pragma unroll
            for (int jj = 0; jj < KCH / 8; jj++) {
                double2 afn[RBW];
                if (jj + 1 < KCH / 8) {
#pragma unroll
                    for (int i = 0; i < RBW; i++) afn[i] = wrow[i][(size_t)(j0 + jj + 1) * 64];
                }
                bool act[RBW];
#pragma unroll
                for (int i = 0; i < RBW; i++)
                    act[i] = !DIAG || ((!PARTIAL || keep[i]) && 8 * (j0 + jj) <= 16 * g[i] + 15);
#pragma unroll
                for (int h = 0; h < 2; h++) {
                    double bf[CBW];
#pragma unroll
                    for (int cb = 0; cb < CBW; cb++)
                        bf[cb] = lds_k[b][((jj * 2 + h) * 4 + cg * CBW + cb) * 64 + lane];
#pragma unroll
                    for (int i = 0; i < RBW; i++) {
                        if (act[i]) {
                            const double av = h ? af[i].y : af[i].x;
#pragma unroll
                            for (int cb = 0; cb < CBW; cb++) acc[i][cb] = mfma_f64(av, bf[cb], acc[i][cb]);
                        }
                    }
                }
                if (jj + 1 < KCH / 8) {
#pragma unroll
                    for (int i = 0; i < RBW; i++) af[i] = afn[i];
                }
            }
#ifdef IBO_STAMPS
            const unsigned long long c2 = __builtin_amdgcn_s_memtime();
            __syncthreads();
            const unsigned long long c3 = __builtin_amdgcn_s_memtime();
            cyc[DIAG ? 3 : 0] += c1 - c0; cyc[DIAG ? 4 : 1] += c2 - c1; cyc[DIAG ? 5 : 2] += c3 - c2;
            nst[DIAG ? 1 : 0] += 1;
#else
            __syncthreads();
#endif
        };
        // a PARTIAL last panel (N not a multiple of the panel) has waves whose row-blocks do not
        // exist: it runs every stage through the predicated form so those MFMAs are skipped
        // (a separate instantiation, so the full-panel code is not perturbed)
        const int nplain = PARTIAL ? 0 : nfull;
        for (int t = 0; t < nplain; t++) stage(t, std::false_type{});
        for (int t = nplain; t < nchunk; t++) stage(t, std::true_type{});
        // |V|^2 down the rows of this panel: acc[i][cb][r] is row (lane>>4)+4r, column lane&15
#pragma unroll
        for (int cb = 0; cb < CBW; cb++) {
            double s = 0.0;
#pragma unroll
            for (int i = 0; i < RBW; i++) {
                double si = 0.0;
#pragma unroll
                for (int r = 0; r < 4; r++) si = fma(acc[i][cb][r], acc[i][cb][r], si);
                s += keep[i] ? si : 0.0;
            }
            s += __shfl_xor(s, 16);
            s += __shfl_xor(s, 32);
            qacc[cb] += s;
        }
    };

    // the last panel sees every k: it also forms the mean.  Only panel 0 can be short.
    if (SPLIT) {
        const int p = blockIdx.y;
        if (p == npanel - 1) {
            if (p == 0 && rem) run_panel(p, std::true_type{}, std::true_type{});
            else run_panel(p, std::true_type{}, std::false_type{});
        } else if (p == 0 && rem) run_panel(p, std::false_type{}, std::true_type{});
        else run_panel(p, std::false_type{}, std::false_type{});
    } else if (npanel == 1) {
        if (rem) run_panel(0, std::true_type{}, std::true_type{});
        else run_panel(0, std::true_type{}, std::false_type{});
    } else {
        if (rem) run_panel(0, std::false_type{}, std::true_type{});
        else run_panel(0, std::false_type{}, std::false_type{});
        for (int p = 1; p + 1 < npanel; p++) run_panel(p, std::false_type{}, std::false_type{});
        STAMP(2);
        run_panel(npanel - 1, std::true_type{}, std::false_type{});
        STAMP(3);
    }

    // every wave contributes to CBW candidate blocks only; the others get zeros
    lds_q[wave][lane] = 0.0;
    if (lane < 16) {
#pragma unroll
        for (int cb = 0; cb < CBW; cb++) lds_q[wave][(cg * CBW + cb) * 16 + lane] = qacc[cb];
    }
    lds_m[0][wave][lane] = muY;
    lds_m[1][wave][lane] = mu1;
    __syncthreads();
    STAMP(4);
    if (wave == 0) {
        double q = 0.0, my = 0.0, m1 = 0.0;
#pragma unroll
        for (int w = 0; w < NW; w++) { q += lds_q[w][lane]; my += lds_m[0][w][lane]; m1 += lds_m[1][w][lane]; }
        int64_t li = tile0 + lane;
        bool valid = li < a.M;
        if (SPLIT) {
            if (valid) {
                a.qpart[(size_t)blockIdx.y * a.M + li] = q;
                if ((int)blockIdx.y == npanel - 1) { a.mupart[li] = my; a.mupart[a.M + li] = m1; }
            }
            return;
        }
        bool excl;
        double val = finish_candidate(a, a.cand + (valid ? li : a.M - 1) * D, q, my, m1, li, valid, excl);
        int64_t idx = a.index_base + li;
        if (!valid || excl || !(val == val)) { val = -INFINITY; idx = INT64_MAX; }
        wave_argmax(val, idx);
        if (lane == 0) { a.part_val[blockIdx.x] = val; a.part_idx[blockIdx.x] = idx; }
#ifdef IBO_STAMPS
        STAMP(5);
        if (lane == 0 && !SPLIT && a.mupart) {
            unsigned hw = __builtin_amdgcn_s_getreg((4 << 0) | (0 << 6) | (31 << 11));     // HW_ID
            unsigned xcc = __builtin_amdgcn_s_getreg((20 << 0) | (0 << 6) | (3 << 11));    // XCC_ID
            unsigned long long *d = (unsigned long long *)a.mupart + (size_t)blockIdx.x * 16;
            for (int i = 0; i < 6; i++) d[i] = st[i];
            d[6] = hw; d[7] = xcc;
            for (int i = 0; i < 6; i++) d[8 + i] = cyc[i];
            d[14] = nst[0]; d[15] = nst[1];
        }
#endif
    }
}

// ------------------------------------------------------------------------
// small-batch path: grid (row chunks of 64, M).  Each workgroup rebuilds k*
// for its candidate in LDS and reduces 64 rows of W k*.
// ------------------------------------------------------------------------
__global__ __launch_bounds__(256) void sweep_gemv_kernel(SweepArgs a)
{
    extern __shared__ double ks[];      // Npad
    __shared__ double red[4][3];
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
    const int64_t c = blockIdx.y;
    const int rc = blockIdx.x;
    const int D = a.kp.D, Npad = a.Npad, DP = a.DP;
    const double *x = a.cand + c * D;
    const int kmax = min(Npad, rc * 64 + 64);       // rows of this chunk need k < kmax only
    const int kneed = (rc == 0) ? Npad : kmax;      // chunk 0 also forms the mean
    double py = 0.0, p1 = 0.0;
    for (int k = t; k < kneed; k += 256) {
        const double *xr = a.Xp + (size_t)k * DP;
        double z = 0.0;
        for (int d = 0; d < D; d++) { double u = xr[d] - x[d]; z += a.kp.w[d] * (u * u); }
        double kv = cov_from_z_rt(a.kp.family, z, a.kp.sf2);
        ks[k] = kv;
        if (rc == 0) { py += a.alphaY[k] * kv; p1 += a.alpha1[k] * kv; }
    }
    __syncthreads();
    double qs = 0.0;
    for (int rr = 0; rr < 16; rr++) {
        int row = rc * 64 + wv * 16 + rr;
        if (row >= Npad) break;
        const double *w = a.W + (size_t)row * Npad;
        double s = 0.0;
        for (int k = lane; k <= row; k += 64) s += w[k] * ks[k];
        for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
        qs += s * s;
    }
    for (int o = 32; o > 0; o >>= 1) { py += __shfl_xor(py, o); p1 += __shfl_xor(p1, o); }
    if (lane == 0) { red[wv][0] = qs; red[wv][1] = py; red[wv][2] = p1; }
    __syncthreads();
    if (t == 0) {
        a.qpart[(size_t)rc * a.M + c] = red[0][0] + red[1][0] + red[2][0] + red[3][0];
        if (rc == 0) {
            a.mupart[c] = red[0][1] + red[1][1] + red[2][1] + red[3][1];
            a.mupart[a.M + c] = red[0][2] + red[1][2] + red[2][2] + red[3][2];
        }
    }
}

__global__ __launch_bounds__(64) void sweep_gemv_finish_kernel(SweepArgs a, int nrc)
{
    const int lane = threadIdx.x;
    int64_t li = (int64_t)blockIdx.x * 64 + lane;
    bool valid = li < a.M;
    int64_t ci = valid ? li : a.M - 1;
    double q = 0.0;
    for (int r0 = 0; r0 < nrc; r0 += 8) {              // index order; eight loads in flight
        double v[8];
#pragma unroll
        for (int u = 0; u < 8; u++) v[u] = r0 + u < nrc ? a.qpart[(size_t)(r0 + u) * a.M + ci] : 0.0;
#pragma unroll
        for (int u = 0; u < 8; u++) if (r0 + u < nrc) q += v[u];
    }
    bool excl;
    double val = finish_candidate(a, a.cand + ci * a.kp.D, q, a.mupart[ci], a.mupart[a.M + ci], li, valid, excl);
    int64_t idx = a.index_base + li;
    if (!valid || excl || !(val == val)) { val = -INFINITY; idx = INT64_MAX; }
    wave_argmax(val, idx);
    if (lane == 0) { a.part_val[blockIdx.x] = val; a.part_idx[blockIdx.x] = idx; }
}

// final (max, lowest index) over the per-tile partials: one workgroup, fixed order
__global__ __launch_bounds__(256) void argmax_final_kernel(const double *__restrict__ pv,
                                                           const int64_t *__restrict__ pi, int64_t n,
                                                           double *out_v, int64_t *out_i)
{
    __shared__ double sv[4];
    __shared__ int64_t si[4];
    double v = -INFINITY;
    int64_t i = INT64_MAX;
    for (int64_t e = threadIdx.x; e < n; e += 256) {
        double ov = pv[e]; int64_t oi = pi[e];
        if (ov > v || (ov == v && oi < i)) { v = ov; i = oi; }
    }
    wave_argmax(v, i);
    if ((threadIdx.x & 63) == 0) { sv[threadIdx.x >> 6] = v; si[threadIdx.x >> 6] = i; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < 4; w++)
            if (sv[w] > v || (sv[w] == v && si[w] < i)) { v = sv[w]; i = si[w]; }
        out_v[0] = v;
        out_i[0] = (i == INT64_MAX) ? -1 : i;
    }
}


template <int FAM, int NW, int RBW, int CBW, int KCH, bool DOT>
static int launch_mfma_cfg(const SweepArgs &a, int64_t ntiles, hipStream_t s)
{
    dim3 grid((unsigned)ntiles), block(NW * 64);
    if (a.DP == 4) hipLaunchKernelGGL((sweep_mfma_kernel<FAM, 4, NW, RBW, CBW, KCH, DOT>), grid, block, 0, s, a);
    else if (a.DP == 8) hipLaunchKernelGGL((sweep_mfma_kernel<FAM, 8, NW, RBW, CBW, KCH, DOT>), grid, block, 0, s, a);
    else if (a.DP == 16) hipLaunchKernelGGL((sweep_mfma_kernel<FAM, 16, NW, RBW, CBW, KCH, DOT>), grid, block, 0, s, a);
    else if (a.DP == 32) hipLaunchKernelGGL((sweep_mfma_kernel<FAM, 32, NW, RBW, CBW, KCH, DOT>), grid, block, 0, s, a);
    else if (!DOT) hipLaunchKernelGGL((sweep_mfma_kernel<FAM, 64, NW, RBW, CBW, KCH, false>), grid, block, 0, s, a);     // 33 .. 64 dimensions: difference form only
    else return (int)hipErrorInvalidValue;
    return (int)hipGetLastError();
}

template <int FAM, bool DOT>
static int launch_mfma_var(const SweepArgs &a, int64_t ntiles, hipStream_t s)
{
    // <16 waves, 2 row-blocks x 4 candidate-blocks per wave, 64-row stages> (the tile shapes <16,2,4,32>, <8,4,4,32> and
    // <16,4,2,64> of round 1 measured 66-75 % against this one's 79 % and are gone)
    return launch_mfma_cfg<FAM, 16, 2, 4, 64, DOT>(a, ntiles, s);
}

template <int FAM, bool DOT>
static int launch_mfma_split(const SweepArgs &a, int64_t ntiles, hipStream_t s)
{
    // IBO_SPLIT_PANEL-row panels: 16 waves = 4 row-blocks x 4 candidate-blocks, one accumulator each
    static_assert(IBO_SPLIT_PANEL == 64, "the split configuration below tiles a 64-row panel");
    dim3 grid((unsigned)ntiles, (a.Npad + IBO_SPLIT_PANEL - 1) / IBO_SPLIT_PANEL), block(1024);
    if (a.DP == 4) hipLaunchKernelGGL((sweep_mfma_kernel<FAM, 4, 16, 1, 1, 64, DOT, IBO_SPLIT_PANEL, true>), grid, block, 0, s, a);
    else if (a.DP == 8) hipLaunchKernelGGL((sweep_mfma_kernel<FAM, 8, 16, 1, 1, 64, DOT, IBO_SPLIT_PANEL, true>), grid, block, 0, s, a);
    else if (a.DP == 16) hipLaunchKernelGGL((sweep_mfma_kernel<FAM, 16, 16, 1, 1, 64, DOT, IBO_SPLIT_PANEL, true>), grid, block, 0, s, a);
    else if (a.DP == 32) hipLaunchKernelGGL((sweep_mfma_kernel<FAM, 32, 16, 1, 1, 64, DOT, IBO_SPLIT_PANEL, true>), grid, block, 0, s, a);
    else if (!DOT) hipLaunchKernelGGL((sweep_mfma_kernel<FAM, 64, 16, 1, 1, 64, false, IBO_SPLIT_PANEL, true>), grid, block, 0, s, a);
    else return (int)hipErrorInvalidValue;
    return (int)hipGetLastError();
}

template <int FAM>
static int launch_mfma_fam(const SweepArgs &a, int64_t ntiles, hipStream_t s)
{
    if (a.qpart) {           // split mode requested by the caller (small batch)
        if (a.dot_form) return launch_mfma_split<FAM, true>(a, ntiles, s);
        return launch_mfma_split<FAM, false>(a, ntiles, s);
    }
    // large batches reach this kernel only in the difference form: data that admit the dot form go to sweep2.hip
    // (abi_sweep.hip: sweep_tile clears dot_form on this route, also when a test forces it)
    return launch_mfma_var<FAM, false>(a, ntiles, s);
}

int launch_sweep_mfma(const SweepArgs &a, hipStream_t s, hipEvent_t e0, hipEvent_t e1)
{
    int64_t ntiles = (a.M + TC - 1) / TC;
    int rc;
    if (e0) (void)hipEventRecord(e0, s);
    if (a.kp.family == FAM_SE) rc = launch_mfma_fam<FAM_SE>(a, ntiles, s);
    else if (a.kp.family == FAM_M3) rc = launch_mfma_fam<FAM_M3>(a, ntiles, s);
    else rc = launch_mfma_fam<FAM_M5>(a, ntiles, s);
    if (e1) (void)hipEventRecord(e1, s);
    if (rc) return rc;
    if (a.qpart) {
        hipLaunchKernelGGL(sweep_gemv_finish_kernel, dim3((unsigned)ntiles), dim3(64), 0, s, a,
                           (a.Npad + IBO_SPLIT_PANEL - 1) / IBO_SPLIT_PANEL);
        rc = (int)hipGetLastError();
        if (rc) return rc;
    }
    return launch_argmax_final(a, ntiles, s);
}

// k* of one candidate (8 Npad bytes, dynamic) and red[4][3] (96 bytes, static) in the 160 KiB of LDS a workgroup may hold on gfx950: 20416 rows
bool sweep_gemv_fits(int Npad) { return sizeof(double) * ((size_t)Npad + 12) <= 160 * 1024; }

int launch_sweep_gemv(const SweepArgs &a, hipStream_t s, hipEvent_t e0, hipEvent_t e1)
{
    if (!sweep_gemv_fits(a.Npad)) return (int)hipErrorInvalidConfiguration;     // (abi_sweep.hip: choose_route reports it before anything is launched)
    int nrc = a.Npad / 64;
    dim3 grid(nrc, (unsigned)a.M);
    if (sizeof(double) * a.Npad > 64 * 1024) {     // up to 160 KiB of LDS per workgroup on gfx950
        hipError_t e = hipFuncSetAttribute((const void *)sweep_gemv_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                           (int)(sizeof(double) * a.Npad));
        if (e != hipSuccess) return (int)e;
    }
    if (e0) (void)hipEventRecord(e0, s);
    hipLaunchKernelGGL(sweep_gemv_kernel, grid, dim3(256), sizeof(double) * a.Npad, s, a);
    if (e1) (void)hipEventRecord(e1, s);
    int64_t ntiles = (a.M + 63) / 64;
    hipLaunchKernelGGL(sweep_gemv_finish_kernel, dim3((unsigned)ntiles), dim3(64), 0, s, a, nrc);
    int rc = (int)hipGetLastError();
    if (rc) return rc;
    return launch_argmax_final(a, ntiles, s);
}

int launch_argmax_final(const SweepArgs &a, int64_t ntiles, hipStream_t s)
{
    if (!a.result_val) return 0;                     // per-point outputs only (DIRECT batches, posteriors): no arg-max wanted
    hipLaunchKernelGGL(argmax_final_kernel, dim3(1), dim3(256), 0, s, a.part_val, a.part_idx, ntiles,
                       a.result_val, a.result_idx);
    return (int)hipGetLastError();
}

void ibo_touch_sweep() { hipFuncAttributes a; (void)hipFuncGetAttributes(&a, (const void *)argmax_final_kernel); }     // (see small2.hip: ibo_touch_small2)

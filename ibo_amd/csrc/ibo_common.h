// ibo_common.h -- shared declarations for the gfx950 implementation of the
// GP-posterior + acquisition path (see include/ibo_abi.h for the boundary).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>
#include <vector>

#define IBO_DMAX 64            // largest input dimensionality handled on device (rows of X are padded to DP = 4, 8, 16, 32 or 64)
#define IBO_DDOT 32            // ... and the largest for which the dot-form kernels (sweep2.hip, small2.hip: exponent GEMM of up to
                               // nine k4-steps) are instantiated; beyond, the difference-form kernels of sweep.hip take every batch

// The dot form y = a_k + b_c + x~.c~ (x~ = x sqrt(w)) carries an ABSOLUTE error of about |x~|^2 2^-52 in the exponent, whatever the distance
// between the two points; a model whose scaled observations lie farther from the origin takes the difference-form kernels.
//   IBO_DOT_GUARD       max_k |x~_k|^2 of a model's observations that still admits the dot-form sweeps (dot_form_ok and ibo_gp_extend in
//                       abi_fit.hip).  The posterior mean is the sensitive output: its error is about (exponent error) x sum_i |k*_i alpha_i|,
//                       absolute and growing with the model.  At 1e5 -- the value until the suite left the unit cube -- a 1100-row model at
//                       the edge missed the 1e-9 absolute bar on the mean (1.2e-9 to 3e-9 on the device, 0.9 to 1.0 of the bar in the
//                       float64 restatement of tests/shift_reference.py); 2e4 leaves that model a factor of four, the variance and the
//                       acquisition values a factor of a hundred under their 1e-6.
//   IBO_DOT_GUARD_NLML  the same for ibo_nlml_grid's covariance pass, on the per-dimension bound sum_d w_d max_k x_kd^2 over every theta-point of
//                       the call (abi_nlml.hip).  At its edge the likelihood value moves by up to 2e-8 relative (1e-10 in the unit cube),
//                       which no optimiser notices: left where it was.
//   IBO_DOT_PULL_IN     |c~|^2 beyond which a CANDIDATE of a dot-form sweep is pulled in to that radius (s2_stage_candidates in sweep2_dev.h).
//                       775 length scales from the origin is at least 630 from any admitted observation (|x~| <= 142 under IBO_DOT_GUARD),
//                       where k* = 0 exactly for every family: the value does not change, and the exponent stays within what s2_exp's
//                       integer arithmetic covers (|y| < 7e5).
#define IBO_DOT_GUARD 2e4
#define IBO_DOT_GUARD_NLML 1e5
#define IBO_DOT_PULL_IN 6e5

// |x~|^2 of one point under a kernel's scaling (host side: the guards above)
static inline double ibo_scaled_norm2(const double *sw, const double *x, int D)
{
    double n2 = 0.0;
    for (int d = 0; d < D; d++) { const double v = x[d] * sw[d]; n2 += v * v; }
    return n2;
}

// covariance families after normalising the reference's four kernel types to
// "weighted squared distance z = sum_d w_d (x_d - c_d)^2, then a scalar map":
//   SE  (ARD: w_d = 1/theta_d^2, ISO: w_d = 1/theta^2)  k = sf2 exp(-z/2)
//   M3  (w_d = 1/theta^2)  r = sqrt(3 z)  k = sf2 (1 + r) exp(-r)
//   M5  (w_d = 1/theta^2)  r = sqrt(5 z)  k = sf2 (1 + r + r^2/3) exp(-r)
// (cpp/optimizeGP.cpp:67-113, ego/gaussianprocess/kernel.py:87-89,147-149,207-210,246-249)
enum { FAM_SE = 0, FAM_M3 = 1, FAM_M5 = 2 };

struct KParams {
    int family;
    int D;                      // true dimensionality (<= IBO_DMAX)
    double sf2;
    double w[IBO_DMAX];         // zero beyond D
    double sw[IBO_DMAX];        // sqrt(w): coordinates are pre-scaled for the sweep's k* generation
};

// z of two unscaled points: the difference first, then one FMA per dimension in ascending order (cov.hip, grad.hip).  The sweeps' k*
// generation scales first or takes the dot form -- other roundings, kept where they are.
__device__ __forceinline__ double wsqdist_dev(const double *w, const double *a, const double *b, int D)
{
    double z = 0.0;
    for (int d = 0; d < D; d++) { const double u = a[d] - b[d]; z = fma(w[d] * u, u, z); }
    return z;
}

template <int FAM>
__device__ __forceinline__ double cov_from_z(double z, double sf2)
{
    if (FAM == FAM_SE) return sf2 * exp(-0.5 * z);
    if (FAM == FAM_M3) { double r = sqrt(3.0 * z); return sf2 * (1.0 + r) * exp(-r); }
    double r = sqrt(5.0 * z);
    return sf2 * (1.0 + r + r * r * (1.0 / 3.0)) * exp(-r);
}

// exp(y) for the k* generation in 16 VALU instructions (the library's takes ~30).
// Next to a saturated fp64 MFMA pipe EVERY VALU instruction -- fp64, fp32 or integer --
// costs 7-13 pipe cycles (tools/mfma_f64_peak), so instruction count is sweep time.
//   t = y log2(e) + 1.5*2^52 puts n = rint(y log2 e) in the low mantissa bits of t;
//   r = y - n ln2 (two-term Cody-Waite);  degree-10 near-minimax polynomial on
//   |r| <= ln2/2 (max relative error 4.4e-16, fitted at Chebyshev nodes; 4.5e-16 with the
//   roundings of its evaluation: tests/kstar_reference.py restates it against mpmath);
//   2^n by an integer add into the exponent field.  Valid for -708 <= y <= 709;
//   smaller y is clamped (result 3e-308 instead of a denormal or 0).
__device__ __forceinline__ double exp_fast(double y)
{
    y = fmax(y, -708.0);
    const double magic = 6755399441055744.0;               // 1.5 * 2^52
    const double t = fma(y, 1.4426950408889634074, magic);
    const double n = t - magic;
    double r = fma(n, -6.93147180369123816490e-01, y);
    r = fma(n, -1.90821492927058770002e-10, r);
    double p = 2.76263763215172631873e-07;
    p = fma(p, r, 2.76401811512398433028e-06);
    p = fma(p, r, 2.48015043005816596198e-05);
    p = fma(p, r, 1.98411702694117908236e-04);
    p = fma(p, r, 1.38888889325245227201e-03);
    p = fma(p, r, 8.33333338566888577603e-03);
    p = fma(p, r, 4.16666666665730586749e-02);
    p = fma(p, r, 1.66666666665543999892e-01);
    p = fma(p, r, 5.00000000000000555112e-01);
    p = fma(p, r, 1.00000000000000666134e+00);
    p = fma(p, r, 1.0);
    const int hi = __double2hiint(p) + (__double2loint(t) << 20);
    return __hiloint2double(hi, __double2loint(p));
}

// sqrt(x), x >= 0, for the sweep's hot loop: v_rsq_f64 and one third-order correction (7 instructions; the
// library sqrt is a ~20-instruction sequence with scaling for denormals and exceptional inputs, and every VALU
// instruction costs MFMA issue slots here).  x is floored at 1e-300 so that x = 0 (a candidate on top of an
// observation) gives 1e-150 instead of 0 * inf; relative error < 2e-16 elsewhere.
__device__ __forceinline__ double sqrt_fast(double x)
{
    x = fmax(x, 1e-300);
    const double y = __builtin_amdgcn_rsq(x);
    const double r = x * y;
    const double e = fma(-r, y, 1.0);                 // 1 - x y^2
    return fma(r * e, fma(0.375, e, 0.5), r);
}

// k* from pre-scaled coordinates.  SE: y = log sf2 - z/2 fed to exp_fast.
template <int FAM>
__device__ __forceinline__ double cov_from_z_fast(double z, double log_sf2, double sf2)
{
    if (FAM == FAM_SE) return exp_fast(fma(-0.5, z, log_sf2));
    if (FAM == FAM_M3) { double r = sqrt_fast(3.0 * z); return sf2 * (1.0 + r) * exp_fast(-r); }
    double r = sqrt_fast(5.0 * z);
    return sf2 * fma(r, fma(r, 1.0 / 3.0, 1.0), 1.0) * exp_fast(-r);
}

__device__ __forceinline__ double cov_from_z_rt(int fam, double z, double sf2)
{
    if (fam == FAM_SE) return cov_from_z<FAM_SE>(z, sf2);
    if (fam == FAM_M3) return cov_from_z<FAM_M3>(z, sf2);
    return cov_from_z<FAM_M5>(z, sf2);
}

typedef double d4_t __attribute__((ext_vector_type(4)));

// which derivative each hyper-parameter index asks for (nlml_grad_kernel)
#define IBO_GRAD_MAX 65          // D length scales + the signal magnitude
struct GradSpec {
    int nh;
    int mode[IBO_GRAD_MAX];     // 0 SE-ARD length scale of dimension dim[h]; 1 SE-iso length scale; 2 signal
                                // magnitude (2K); 3 Matern-3/2 length scale; 4 Matern-5/2 length scale
    int dim[IBO_GRAD_MAX];
};

// fp64 MFMA 16x16x4: D(16x16) += A(16x4) * B(4x16).  Lane l supplies
// A[row = l&15][k = l>>4] and B[k = l>>4][col = l&15]; it receives
// D[row = (l>>4) + 4*r][col = l&15] in element r (cdna_hip_programming.md s3).
__device__ __forceinline__ d4_t mfma_f64(double a, double b, d4_t c)
{
    return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0);
}

// the wave's 64 values summed in a fixed order without a trip through the LDS crossbar: four DPP steps inside the rows of 16 lanes (xor 1, xor 2,
// half-row mirror, row mirror), then the four row sums, first to last (assemble.hip: nlml_grad_fast_kernel; gradobs.hip: gradobs_contract_kernel)
__device__ __forceinline__ double wave_sum_rows(double v)
{
#define WS_STEP(ctrl) { const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(v), ctrl, 0xf, 0xf, true), \
                                  hi = __builtin_amdgcn_update_dpp(0, __double2hiint(v), ctrl, 0xf, 0xf, true); v += __hiloint2double(hi, lo); }
    WS_STEP(0xB1) WS_STEP(0x4E) WS_STEP(0x141) WS_STEP(0x140)
#undef WS_STEP
    auto row = [&](int l) { return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), l), __builtin_amdgcn_readlane(__double2loint(v), l)); };
    return ((row(0) + row(16)) + row(32)) + row(48);
}

// RBF-network mean prior parameters (device pointers)
struct PriorDev {
    int nb;
    double theta;
    const double *means;    // nb x D
    const double *beta;     // nb
    const double *lowerb;   // D
    const double *width;    // D
};

// The RBF-network prior mean m(x) = sum_i beta_i exp(-theta |u - c_i|^2), u = (x - lowerb) / width, basis functions in ascending order: the
// ONE sum behind every mean the library returns (sweep epilogue, gradient, leave-one-out).  X(j): coordinate j of the point (a lambda, so
// that the system-scope loads of finish_candidate<true> go through the same body).  dm (grad_finish_kernel): also receives dm / dx_dd, every
// term formed from the very beta_i exp(..) that enters the mean.
template <typename XF>
__device__ __forceinline__ double prior_mean_dev(const PriorDev &p, int D, XF X, int dd = 0, double *dm = nullptr)
{
    double m = 0.0, g = 0.0;
    for (int i = 0; i < p.nb; i++) {
        double d = 0.0;
        for (int j = 0; j < D; j++) {
            const double t = (X(j) - p.lowerb[j]) / p.width[j] - p.means[(size_t)i * D + j];
            d += t * t;
        }
        const double be = p.beta[i] * exp(-p.theta * d);
        m += be;
        if (dm) g += be * (-2.0 * p.theta) * ((X(dd) - p.lowerb[dd]) / p.width[dd] - p.means[(size_t)i * D + dd]) / p.width[dd];
    }
    if (dm) *dm = g;
    return m;
}

// acquisition value (positive) from (mu, sigma); mirrors
// cpp/optimizeGP.cpp:194-236 (libm) and ego/acquisition/__init__.py:68-71,107-110,150-164
// with CDF/PDF of ego/gaussianprocess/__init__.py:55-77 (NR).
__device__ __forceinline__ double erf_nr_dev(double z)
{
    double t = 1.0 / (1.0 + 0.5 * fabs(z));
    double p = 0.17087277;
    p = -0.82215223 + t * p;
    p = 1.48851587 + t * p;
    p = -1.13520398 + t * p;
    p = 0.27886807 + t * p;
    p = -0.18628806 + t * p;
    p = 0.09678418 + t * p;
    p = 0.37409196 + t * p;
    p = 1.00002368 + t * p;
    double ans = 1.0 - t * exp(-z * z - 1.26551223 + t * p);
    return z >= 0.0 ? ans : -ans;
}

// Gaussian cdf and pdf at z in either erf flavour (NR: with the reference's truncated 1 / sqrt 2 and 1 / sqrt(2 pi))
__device__ __forceinline__ void gauss_cdf_pdf_dev(int erf_mode, double z, double *cdf, double *pdf)
{
    if (erf_mode == 0) {
        *cdf = 0.5 * (1.0 + erf(z / sqrt(2.0)));
        *pdf = exp(-(z * z / 2.0)) / sqrt(2.0 * M_PI);
    } else {
        *cdf = 0.5 * (1.0 + erf_nr_dev(z * 0.707106));
        *pdf = exp(-(z * z / 2.0)) * 0.398942;
    }
}

__device__ __forceinline__ double acq_value_dev(int acq, int erf_mode, double mu, double sigma,
                                                double ymax, double parm)
{
    if (acq == 2) return mu + parm * sigma;
    double ydiff = mu - ymax - parm;
    double Z = ydiff / sigma;
    double cdf, pdf;
    gauss_cdf_pdf_dev(erf_mode, Z, &cdf, &pdf);
    if (acq == 1) return cdf;
    return ydiff * cdf + sigma * pdf;
}

// What a constrained acquisition (ibo_cacq_*) is made of beside the models: the objective's acquisition and one (threshold, sense) per
// constraint model.  sense +1: feasible where c_j <= thresh_j; -1: where c_j >= thresh_j.
#define IBO_CACQ_MAX 8          // IBO_CACQ_MAX_CON of ibo_abi.h
struct CacqSpec {
    int ncon, acq, erf_mode;
    double ymax, parm;
    double thresh[IBO_CACQ_MAX];
    int sense[IBO_CACQ_MAX];
};

// The constrained acquisition of one candidate: val = A Phi(z_0) Phi(z_1) .., multiplied in that order; A = EI / PI of the objective
// (acq == 3: A = 1, the pure probability of feasibility), z_j = s_j (t_j - mu_j) / sigma_j, P = prod_j Phi(z_j) (empty product: 1).
// MS(k, &mu, &s2): the posterior of model k at the candidate, variance clipped -- k = 0 the objective (not asked for when acq == 3),
// k = 1 + j constraint j.  Phi in the call's erf flavour, as the objective's.
template <typename MS>
__device__ __forceinline__ double cacq_value_dev(const CacqSpec &c, MS ms, double *A, double *P)
{
    double mu, s2, a = 1.0;
    if (c.acq != 3) { ms(0, &mu, &s2); a = acq_value_dev(c.acq, c.erf_mode, mu, sqrt(s2), c.ymax, c.parm); }
    double p = 1.0, v = a;
    for (int j = 0; j < c.ncon; j++) {
        ms(1 + j, &mu, &s2);
        const double z = (double)c.sense[j] * (c.thresh[j] - mu) / sqrt(s2);
        double cdf, pdf;
        gauss_cdf_pdf_dev(c.erf_mode, z, &cdf, &pdf);
        p *= cdf; v *= cdf;
    }
    *A = a; *P = p;
    return v;
}

#define IBO_MARG_MAX 32         // IBO_IACQ_MAX of ibo_abi_ensemble.h: the members of an integrated acquisition (marg.h)

// ---- host-side launch API of the kernels (defined in linalg.hip / assemble.hip / update3.hip / sweep*.hip / small2.hip)
#define IBO_SPLIT_PANEL 64      // rows per workgroup of the small-batch (SPLIT) sweep
#define IBO_S2_TCAND 32         // candidates per workgroup of sweep2_kernel (sweep2.hip)

struct SweepArgs {
    KParams kp;
    int N, Npad, DP;
    int64_t M;
    const double *Xp;        // Npad x DP, zero padded
    const double *Xs;        // Npad x DP, coordinates scaled by sqrt(w_d)  (x~)
    const double *ak;        // Npad: -|x~_k|^2 / 2
    const double *XA;        // [x~ | a_k | 1] in MFMA A-fragment order (pack_xa_kernel), rows padded to a multiple of 128
    const double *exp_tab;   // 2^(j/2048), j < 2048 (device; sweep2's exp)
    double log_sf2;          // log of the k* signal variance
    int dot_form;            // y = ak + bc + x~.c~ (D+1 FMAs) instead of the difference form (2D)
    const double *W;         // Npad x Npad row-major lower-triangular, q = |W k*|^2
    const double *Wp;        // same matrix in MFMA fragment order (see pack_w_kernel)
    const double *alphaY;    // Npad
    const double *alpha1;    // Npad
    const double *cand;      // M x D
    PriorDev prior;
    double noise, clamp_lo, ymax, parm;
    int acq, erf_mode;
    int n_excl; const double *excl; double excl_radius;   // n_excl x D (device)
    int64_t index_base;
    double *out_mu, *out_s2, *out_acq;   // optional
    double *part_val; int64_t *part_idx; // one per 64-candidate tile
    double *qpart;                       // gemv path scratch: rowchunks x M
    double *mupart;                      // gemv path scratch: 2 x M
    double *result_val; int64_t *result_idx;   // device, single element each
    int rank1_row;                             // sweep2_rank1_kernel: the appended row of W being folded into the state (< 0: only the means are formed)
    // Kept state of ibo_acq_sweep_incremental (state5 != 0): qpart = [q_a, aY.k*, a1.k*, zsum, q_b][M]; q = (q_a + q_b) + zsum.
    // q_a: rows [0, h) of W; q_b: rows [h, Npad) -- 0 until the candidate's tile is complete; zsum: the squares the appended rows added.
    // With q_b missing the candidate's variance is an UPPER bound (q can only grow), so EI / UCB computed from it bound its value.
    int state5;
    int part_lo, part_hi;                      // sweep2_kernel<.., PART>: the rows of W this launch covers (part_lo > 0: the second part)
    int part_rows;                             // the model's rows when the state was formed: later rows never enter q_a / q_b (zsum has them)
    int *tile_done;                            // per 32-candidate tile: the last LEVEL of W's rows folded into (q_a, q_b): 0 after the first part,
                                               // part_nlev - 1 once the tile is complete (round 4: up to four levels, see sweep2_part_levels)
    double *tile_ub;                           // per tile: largest value (exact or bound) of its candidates (acq_bound_kernel)
    unsigned long long *part_thresh;           // order-preserving bits of the value a tile's bound must reach to be completed (0: any finite bound)
    int part_all;                              // complete every incomplete tile, whatever its bound
    int part_means;                            // the first part also forms aY.k* and a1.k* (its launch carries the alpha vectors in LDS)
    double part_slack;                         // absolute part of the slack a bound is given against the threshold (s2_part_limit)
    // lazy refresh of such a state: per tile the appended rows already folded into zsum (and the means' age), the selection flags of
    // the launch at hand, the model's rows now, W y (the drift margin's source), and whether tiles may be left stale at all
    int *tile_rows; int *tile_sel; const double *wy; int rank_hi; int part_lazy;
    int part_level, part_nlev;                 // this launch's level (>= 1: only tiles whose tile_done is part_level - 1 run), and how many levels there are
    double nu_max;                             // bound on |(W k*)_i| for any candidate: sf2_k / sqrt(sf2_fit) (abi_sweep.hip: sweep_sweep2_kept); the drift margin's factor
    unsigned long long *part_best;             // acq_bound_kernel: running maximum over the COMPLETE tiles, same encoding
    // small2.hip: when set, the last workgroup of the last kernel stores done_seq there (host-visible memory) after all
    // results are out -- the host spins on that word instead of going through an event
    unsigned long long *done_flag; unsigned long long done_seq; unsigned *done_count;
    const double *cand_host;                   // the same candidates where the HOST can read them (pinned staging), or NULL
};

// The acquisition epilogue of one candidate, for every sweep kernel: prior mean, variance clamp, EI / PI / UCB, exclusion balls, optional
// outputs; returns the value.  Coordinates are read from global memory where needed (prior, exclusion balls) so that no per-lane
// coordinate array exists (dynamic indexing would put it in scratch).
// SYS: the host spins on a completion flag instead of waiting for the launch to end (small2.hip: small_finish_kernel<true>):
// coordinates and results go through system-scope accesses, which leave no L2 line to be written back before the flag
// (a.kp.D where it is used and the prior behind its own test, not a local copy: sweep_mfma_kernel's register allocation is at its limit, and
// with a local D its 32- and 64-dimensional difference-form instances take 8 more bytes of scratch per lane)
template <bool SYS = false>
__device__ __forceinline__ double finish_candidate(const SweepArgs &a, const double *xp, double q, double muY, double mu1,
                                                   int64_t li, bool valid, bool &excluded)
{
    auto X = [&](int j) { return SYS ? __hip_atomic_load(xp + j, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) : xp[j]; };
    // A candidate with a NaN coordinate has a NaN posterior, and k* does not say so by itself: v_max_f64 returns its other operand, so
    // exp_fast's clamp, sqrt_fast's floor and s2_kstar's z = fmax(-2y, 0) turn the NaN exponent into a point infinitely far away (the
    // squared exponential by differences: k* = 3e-308, the prior variance -- a value that can win) or on top of every observation (Matern).
    // The coordinates are in L2 from the staging; the NaN goes into the sums themselves (no flag kept alive: see the note on a.kp.D above).
    // Not under SYS: those batches come from the host, have no arg-max, and a read of the pinned coordinates would put a bus round trip
    // into every DIRECT batch.
    if (!SYS)
        for (int j = 0; j < a.kp.D; j++)
            if (!(xp[j] == xp[j])) q = muY = NAN;
    const double m = (a.prior.nb > 0) ? prior_mean_dev(a.prior, a.kp.D, X) : 0.0;
    const double mu = (a.prior.nb > 0) ? (m + muY - m * mu1) : muY;
    double s2 = 1.0 + a.noise - q;                  // (a NaN passes both clamps)
    if (s2 < a.clamp_lo) s2 = a.clamp_lo;
    else if (s2 > 10.0) s2 = 10.0;
    const double val = (a.acq == 3) ? mu : acq_value_dev(a.acq, a.erf_mode, mu, sqrt(s2), a.ymax, a.parm);
    excluded = false;
    for (int e = 0; e < a.n_excl; e++) {
        double d2 = 0.0;
        for (int j = 0; j < a.kp.D; j++) { double t = X(j) - a.excl[(size_t)e * a.kp.D + j]; d2 += t * t; }
        if (!(sqrt(d2) > a.excl_radius)) excluded = true;
    }
    if (valid) {
        if (SYS) {                                      // (the flag may be seen before the launch ends: no launch boundary flushes these)
            if (a.out_mu) __hip_atomic_store(a.out_mu + li, mu, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            if (a.out_s2) __hip_atomic_store(a.out_s2 + li, s2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            if (a.out_acq) __hip_atomic_store(a.out_acq + li, val, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        } else {
            if (a.out_mu) a.out_mu[li] = mu;
            if (a.out_s2) a.out_s2[li] = s2;
            if (a.out_acq) a.out_acq[li] = val;
        }
    }
    return val;
}

// The arg-max rule, for every kernel that picks a winner: the larger value wins, the lower index wins ties.  A lane that must never win
// (out of range, excluded, NaN) comes in with (-inf, INT64_MAX) -- its kernel's own masking line, whose condition differs per kernel.
// wave_argmax: every lane of the wave ends with the wave's winner.
__device__ __forceinline__ void wave_argmax(double &v, int64_t &i)
{
    for (int o = 32; o > 0; o >>= 1) {
        double ov = __shfl_xor(v, o);
        int64_t oi = __shfl_xor(i, o);
        if (ov > v || (ov == v && oi < i)) { v = ov; i = oi; }
    }
}
// ... and of a workgroup of 256 threads: the four waves' winners through LDS; thread 0 stores the workgroup's partial for launch_argmax_final
__device__ __forceinline__ void block256_argmax(double val, int64_t idx, double *part_val, int64_t *part_idx)
{
    __shared__ double sv[4];
    __shared__ int64_t si[4];
    wave_argmax(val, idx);
    if ((threadIdx.x & 63) == 0) { sv[threadIdx.x >> 6] = val; si[threadIdx.x >> 6] = idx; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < 4; w++)
            if (sv[w] > val || (sv[w] == val && si[w] < idx)) { val = sv[w]; idx = si[w]; }
        part_val[blockIdx.x] = val; part_idx[blockIdx.x] = idx;
    }
}

// What the finish kernels of the moments pipeline (abi_moments.h: cacq.hip, ehvi.hip, mes.hip, sparse.hip) are told alike about one chunk
// of candidates; the pipeline fills it, the unit's own arguments stand beside it.  (The fields, and the struct's place after `ms` in the
// units' arguments, keep the order the kernel arguments have always had: ehvi.hip's libm-erf instances sit at the scalar register limit, and
// another order of the scalar loads costs them a dozen more spills.)
struct FinishTail {
    int64_t M;                           // candidates of this chunk
    int64_t first;                       // the chunk's first candidate in the call's array (a multiple of 256)
    const double *cand; int D;           // the chunk's candidates, M x D
    int n_excl; const double *excl; double excl_radius;     // n_excl x D (device)
    int64_t index_base;
    double *part_val; int64_t *part_idx; // the chunk's partials: one per 256 candidates
};
// the half of a finish launch's argument check that does not depend on the kernel
static inline bool finish_tail_ok(const FinishTail &t)
{
    return t.M >= 1 && !(t.first & 255) && t.cand && t.part_val && t.part_idx && (t.n_excl <= 0 || t.excl);
}
// ... and how such a kernel ends, with candidate li's value in hand: the exclusion balls (finish_candidate's rule, coordinates read from
// the candidate array), store() -- the kernel's own per-candidate outputs, for a lane in range; after the balls, whose centres stay scalar
// loads that way -- then a lane that is out of range, excluded or NaN never wins, the index in the call's numbering, block256_argmax.
// FMA: whether the squared distance is summed with fused multiply-adds -- written out, because the kernels differ and a ball's edge must
// not move with the compiler's mood: ehvi.hip and mes.hip are compiled with contraction off, cacq.hip and sparse.hip with it on.
template <bool FMA, typename Store>
__device__ __forceinline__ void finish_tail(const FinishTail &t, int64_t li, double val, Store store)
{
#pragma clang fp contract(off)
    const bool valid = li < t.M;
    const double *xp = t.cand + (valid ? li : t.M - 1) * t.D;
    bool excl = false;
    for (int e = 0; e < t.n_excl; e++) {
        double d2 = 0.0;
        for (int j = 0; j < t.D; j++) { double d = xp[j] - t.excl[(size_t)e * t.D + j]; d2 = FMA ? fma(d, d, d2) : d2 + d * d; }
        if (!(sqrt(d2) > t.excl_radius)) excl = true;
    }
    if (valid) store();
    int64_t idx = t.index_base + t.first + li;
    if (!valid || excl || !(val == val)) { val = -INFINITY; idx = INT64_MAX; }
    block256_argmax(val, idx, t.part_val, t.part_idx);
}

int launch_sweep_mfma(const SweepArgs &a, hipStream_t s, hipEvent_t e0, hipEvent_t e1);
int launch_sweep_gemv(const SweepArgs &a, hipStream_t s, hipEvent_t e0, hipEvent_t e1);
// large batches, dot form: 32-candidate tiles, 1024-row panels, exponent GEMM on the MFMA unit (sweep2.hip)
int launch_sweep2(const SweepArgs &a, hipStream_t s, hipEvent_t e0, hipEvent_t e1);
int launch_sweep2_refresh(const SweepArgs &a, int row_first, int row_last, hipStream_t s, hipEvent_t e0, hipEvent_t e1);
// first sweep of a kept state with the second part of W only where a tile's bound can still win (sweep2.hip); prune = false:
// every tile is completed (same launches, same arithmetic -- the reference the pruned run is held to)
int launch_sweep2_pruned(const SweepArgs &a, bool prune, hipStream_t s, hipEvent_t e0, hipEvent_t e1);
// after launch_sweep2_refresh's rank-1 launches on such a state: complete the tiles whose bound has risen to the best complete value
int launch_sweep2_complete(const SweepArgs &a, hipStream_t s);
int launch_sweep2_pruned_finish_all(const SweepArgs &a, hipStream_t s);
bool sweep2_part_fits(int Npad, int D);
int sweep2_part_nlev(int Npad);                   // levels a new kept state gets (<= ibo_set_option("part_levels"))
void set_part_levels(int v);
int sweep2_part_levels(int Npad, int *h);        // the row splits h[0] < h[1] < .. (multiples of 128, at most 3): level l covers rows [h[l-1], h[l]); returns the number of levels
bool sweep2_fits(int Npad);
bool sweep_gemv_fits(int Npad);      // sweep.hip: k* of one candidate in LDS, 8 Npad + 96 bytes <= 160 KiB (20416 rows)
bool sweep2_rank1_fits(int Npad, int D);
// small batches (16 < M <= 8192), dot form: k* to HBM, one workgroup per 16-row block of W, fixed-order sums (small2.hip)
int launch_sweep_small(const SweepArgs &a, double *ws, hipStream_t s, hipEvent_t e0, hipEvent_t e1);
size_t small_sweep_workspace(int Npad, int64_t M);
int launch_pack_xa(const double *Xs, const double *ak, int N, int Npad, int DP, int D, double *XA, hipStream_t s);
int launch_argmax_final(const SweepArgs &a, int64_t ntiles, hipStream_t s);

// K[i][j] = k(A1_i, A2_j) (A2 = NULL: the square matrix K(A1, A1) with the diagonal rule applied; lower_only: only its blocks on and below the diagonal)
int launch_cov_matrix(const KParams &kp, int n1, const double *A1, int n2, const double *A2,
                      int lda_pts, int diag_rule, double noise, double *K, int ldk, hipStream_t s, int lower_only = 0);
int launch_cov_fit(const KParams &kp, int n, const double *X, int ldp, int diag_rule, double noise, double *K2, int np2, double *Eye,
                   int *zero_word, hipStream_t s);          // the fit's own pass: working copy (lower blocks, identity pad), ride-along identity, info word
int launch_cov_matrix_batched(const KParams *kps_dev, int batch, int n1, const double *A1, int ldp, int diag_rule, double noise,
                              double *K, int ldk, size_t kstride, hipStream_t s, int dot_ok = 0);
// factor the Npad x Npad matrix in L (lower part, ld = Npad) in place; diag64 receives the
// inverses of the 64x64 diagonal blocks; info (device int) gets the 1-based failing pivot or 0
// ws (optional): Npad * Npad doubles per matrix (wstride apart), the packed store of the packed-operand trailing update
// (update3.hip: launch_chol_update2); without it the 64 x 64-tile update kernel runs.  Results are bit-identical either way.
int launch_cholesky(double *L, int Npad, double *diag64, int *info_dev, hipStream_t s, double *ws = nullptr);
int launch_cholesky_batched(double *L, int Npad, double *diag64, int *info_dev, int batch, size_t lstride,
                            int panel, hipStream_t s, double *ws = nullptr, size_t wstride = 0);
int launch_chol_update2(double *L, int Npad, int p0, int pend, int batch, size_t lstride, double *ws, size_t wstride,
                        hipStream_t s, const double *Lpanel = nullptr);
// left-looking outer order from one packed copy of the finished block columns (update3.hip); bit-identical to the above
// what a row workgroup of chol_panel_fused_kernel leaves in its matrix's info word when a flag wait runs out (not a pivot: the caller
// runs the batch again through the launches that have no waits)
static const int kPanelWaitTimeout = 0x7ffffff0;
struct CholGroup { double *L, *diag64, *Pk; int *info; int batch; hipStream_t stream; int *flags; };   // flags: 4 ints per matrix (the fused panel kernel's hand-overs) or null      // a sub-batch of matrices (lstride / pstride apart) on its stream
int launch_cholesky_batched_left(const CholGroup *groups, int ngroups, int Npad, size_t lstride, int panel, size_t pstride, int nlive,
                                 int nfactor = 0, int rm_from = 0);
int launch_chol_pack3(const double *L, int Npad, int r0, int c0, int K, int batch, size_t lstride, double *Pk, size_t pstride,
                      hipStream_t s);
int launch_chol_pack3e(const double *E, int Npad, int rend, int c0, int K, double *PkE, hipStream_t s);
int launch_chol_update3(double *L, int Npad, int c0, int width, int nlive, int batch, size_t lstride, const double *Pk,
                        size_t pstride, hipStream_t s);
// the same kernel on any region that starts on the diagonal (rows >= c0, columns [c0, c0 + width)) and any range [kbeg, kend) of packed columns
// C = P P^T (lower 128-tiles) of an upper triangular P on the packed-operand kernel, long K ranges in pieces (update3.hip)
void syrk3_plan(int Npad, int piece, std::vector<int> &tasks, std::vector<int> &sums, int *nslots);
int launch_syrk3(const double *P, double *Pk, double *C, int Npad, const int *tasks_dev, int ntasks, const int *sums_dev, int nsums, double *part,
                 hipStream_t s);
int launch_chol_update3_range(double *L, int Npad, int c0, int width, int kbeg, int kend, int nlive, int batch, size_t lstride,
                              const double *Pk, size_t pstride, hipStream_t s);
// out-of-place, one fused launch per block column (plain right-looking order; `work` is destroyed)
// Ework (identity on entry) / Eout, optional: W = L^-1 rides along -- Eout receives (L^-1)^T, blocks on and above the diagonal
int launch_cholesky_fused(double *work, double *out, int Npad, double *diag64, int *info_dev, hipStream_t s,
                          double *Ework = nullptr, double *Eout = nullptr, bool info_is_zero = false);
// the two-level order (panels of P block columns) out of place, one fused launch per block column inside a panel
int launch_cholesky_fused2(double *work, double *out, int Npad, double *diag64, int *info_dev, int P, hipStream_t s,
                           bool info_is_zero = false, double *ws = nullptr);
// the single-level order in SUPER-PANELS (linalg.hip): the pipelined launches keep their trailing tiles inside a super-panel of 16 block
// columns; the columns beyond take a finished super-panel's steps as ONE deep update from packed operands (update3.hip).  tall: [A ; E] in
// one buffer (2 Npad x Npad: the matrix being reduced, then the ride-along's identity); Pk: 2 Npad^2 doubles (the packed store of
// [out ; Eout]).  Same bits as launch_cholesky_fused.
static const int kSuperFrom = 64;       // block columns (4096 rows) from which it is the faster one (3840 rows: 1.85 against 1.77 ms; 4096: 2.04 / 2.10; 5000: 3.18 / 3.48)
static const int kSuperPanel = 16;
int launch_cholesky_super(double *tall, double *out, int Npad, double *diag64, int *info_dev, hipStream_t s, double *Eout, double *Pk,
                          bool info_is_zero = false);
// W = Et^T (lower, rows >= N zero) and, unless Wp is null, its MFMA-fragment-order copy Wp (another buffer than Et) in one pass
int launch_transpose_pack(const double *Et, int N, int Npad, double *W, double *Wp, hipStream_t s);
// W = L^-1 (row-major, ld = Npad; only the blocks on and below the diagonal are written) using diag64 from launch_cholesky and a scratch T (Npad x Npad)
int launch_trinv(const double *L, int Npad, const double *diag64, double *W, double *T, hipStream_t s);
// zero the strict upper triangle (ld = Npad)
int launch_zero_upper(double *A, int Npad, hipStream_t s);
// Wout/Wp from S; mode 0: W[i][j] = S[i][j]; mode 1: W[i][j] = S[N-1-j][N-1-i] (i,j < N);
// rows/cols >= N are zero.  Wout may be NULL or == S only for mode 0.
int launch_pack_w(const double *S, int N, int Npad, int mode, double *Wout, double *Wp, hipStream_t s);
// alpha = W^T (W y) for two right-hand sides at once (y and the all-ones vector)
int launch_alpha(const double *W, int N, int Npad, const double *y, double *tmp2, double *alphaY,
                 double *alpha1, hipStream_t s);
// Xs = Xp * sqrt(w), ak = -|Xs_k|^2/2; maxnorm2 (device double) receives max_k |Xs_k|^2
int launch_scale_x(const KParams &kp, const double *Xp, int Npad, int DP, double *Xs, double *ak, hipStream_t s);
// C = W^T W (Wt: scratch for the transpose), all Npad x Npad
int launch_wtw(const double *W, double *Wt, double *C, int Npad, hipStream_t s, int lower_only = 0, int wt_ready = 0);     // lower_only: blocks on and below the diagonal
int launch_nlml_grad(const KParams &kp, const GradSpec &gs, int N, const double *X, int ldx, const double *Kinv, int ldk,
                     const double *alpha, double *partial, double *out, hipStream_t s);
// one-point block extension (ibo_gp_extend): kvec[i] = k(x_i, x_N) for i < N (zero beyond) and row / column N of R
int launch_extend_kvec(const KParams &kp, const double *Xp, int ldp, int N, int Npad, double noise, double *R, double *kvec,
                       hipStream_t s);
// d = sqrt(1 + noise - |z|^2); L[N][:N] = z, L[N][N] = d; W[N][:N] = -u/d, W[N][N] = 1/d; row-block N/16 of Wp repacked
int launch_extend_rows(int N, int Npad, double noise, const double *z, const double *u, double *L, double *W, double *Wp,
                       int *info, hipStream_t s);
int launch_nlml_aug(double *L, int Npad, int N, const double *y, hipStream_t s, int batch = 1, size_t lstride = 0);
int launch_nlml_scalars(const double *L, int Npad, int N, const double *y, const double *alpha, double *out2, hipStream_t s);
int launch_nlml_reduce(const double *L, int Npad, int N, double *out2, hipStream_t s, int batch = 1, size_t lstride = 0);
int launch_pad_copy(const double *src, int N, int lds, double *dst, int Npad, double pad_diag, hipStream_t s);
// preference GP: out = base (or 0) + diag I + sparse entries (lin = row * N + col, distinct), identity pad;  A = R + Cinv
int launch_pref_build(const double *base, int N, int Npad, double diag, int nnz, const long long *lin, const double *val,
                      double *out, hipStream_t s);
int launch_pref_sum(const double *R, const double *Cinv, int N, int Npad, double *A, hipStream_t s);
int launch_mfma_selftest(double *out_err, hipStream_t s);
int streams_run_side_by_side(hipStream_t a, hipStream_t b, bool *yes);      // a timing probe: do the two streams sit on different hardware queues?

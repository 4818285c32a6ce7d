// abi_batch.hip -- host points behind the C ABI: batches of posteriors and acquisition values (eval_host_points, one sweep or pipelined
// chunks), query-point gradients, the joint posterior and draws from it, and DIRECT over a GPU objective (direct_maximize, the one driver).
#include "abi_eval.h"
#include "abi_factor.h"
#include "grad.h"
#include "cov.h"

// Host batches hand their results over as one block: (mu, s2, acq) restricted to the wanted ones, contiguous in that order, m values each.
struct Packed3 { double *p[3]; int n; };         // p[k]: where output k of such a block lies (NULL: not wanted); n: how many are
static Packed3 pack3(double *base, size_t m, const double *mu, const double *s2, const double *acq)
{
    Packed3 w = {{nullptr, nullptr, nullptr}, 0};
    const double *want[3] = {mu, s2, acq};
    for (int k = 0; k < 3; k++)
        if (want[k]) w.p[k] = base + m * w.n++;
    return w;
}
// a block in host memory -> the caller's arrays
static void unpack3(const double *base, size_t m, double *mu, double *s2, double *acq)
{
    const Packed3 w = pack3(const_cast<double *>(base), m, mu, s2, acq);
    double *dst[3] = {mu, s2, acq};
    for (int k = 0; k < 3; k++)
        if (dst[k]) memcpy(dst[k], w.p[k], sizeof(double) * m);
}
// the request of a host batch: per-candidate outputs into such a block at `base`, no arg-max
static SweepRequest batch_request(int64_t m, const double *cand_dev, int acq, double parm, int erf_mode, double clamp_lo, double ymax, const Packed3 &out)
{
    SweepRequest r;
    r.M = m; r.cand_dev = cand_dev; r.acq = acq; r.parm = parm; r.erf_mode = erf_mode; r.clamp_lo = clamp_lo; r.ymax = ymax;
    r.mu_dev = out.p[0]; r.s2_dev = out.p[1]; r.acq_dev = out.p[2];
    return r;
}

// Large host-in / host-out batches (GP.posteriors(X) on 10^5..10^7 NumPy rows): chunks of 2^17 points go through
// two sets of pinned + device buffers; the upload of chunk c+1 and the download of chunk c-1 run on their own
// streams while chunk c is in the sweep kernel, so the call costs about the kernel time, not kernel + PCIe +
// pageable staging.
static int eval_host_points_pipelined(ibo_gp *g, int64_t M, const double *Q_host, int acq, double parm, int erf_mode,
                                      double clamp_lo, double *mu_host, double *s2_host, double *acq_host, double ymax)
{
    const int64_t CH = (int64_t)1 << 17;
    const int D = g->D;
    if (!g->h2d_stream) {                             // copy streams and their events: created on first use
        HIP_TRY(hipStreamCreateWithFlags(&g->h2d_stream, hipStreamNonBlocking));
        HIP_TRY(hipStreamCreateWithFlags(&g->d2h_stream, hipStreamNonBlocking));
        for (int b = 0; b < 2; b++) {
            HIP_TRY(hipEventCreateWithFlags(&g->pe_in[b], hipEventDisableTiming));
            HIP_TRY(hipEventCreateWithFlags(&g->pe_k[b], hipEventDisableTiming));
            HIP_TRY(hipEventCreateWithFlags(&g->pe_out[b], hipEventDisableTiming));
        }
    }
    IBO_TRY(g->cand.ensure((size_t)(2 * CH) * D));
    IBO_TRY(g->outs.ensure((size_t)(2 * CH) * 3));
    IBO_TRY(ensure_pinned(g, (size_t)(2 * CH) * (D + 3)));
    double *pin_in[2] = {g->pin, g->pin + CH * D};
    double *pin_out[2] = {g->pin + 2 * CH * D, g->pin + 2 * CH * D + 3 * CH};
    double *dev_in[2] = {g->cand.p, g->cand.p + CH * D};
    double *dev_out[2] = {g->outs.p, g->outs.p + 3 * CH};
    const int64_t nch = (M + CH - 1) / CH;
    auto drain = [&](int64_t c) -> int {              // results of chunk c: pinned -> caller's arrays
        const int b = (int)(c & 1);
        const int64_t m = (c + 1 < nch) ? CH : M - c * CH;
        HIP_TRY(hipEventSynchronize(g->pe_out[b]));
        unpack3(pin_out[b], (size_t)m, mu_host ? mu_host + c * CH : nullptr, s2_host ? s2_host + c * CH : nullptr, acq_host ? acq_host + c * CH : nullptr);
        return IBO_OK;
    };
    for (int64_t c = 0; c < nch; c++) {
        const int b = (int)(c & 1);
        const int64_t m = (c + 1 < nch) ? CH : M - c * CH;
        if (c >= 2) IBO_TRY(drain(c - 2));           // frees buffer set b (its download has finished)
        memcpy(pin_in[b], Q_host + c * CH * D, sizeof(double) * m * D);
        HIP_TRY(hipMemcpyAsync(dev_in[b], pin_in[b], sizeof(double) * m * D, hipMemcpyHostToDevice, g->h2d_stream));
        HIP_TRY(hipEventRecord(g->pe_in[b], g->h2d_stream));
        HIP_TRY(hipStreamWaitEvent(g->stream, g->pe_in[b], 0));
        const Packed3 out = pack3(dev_out[b], (size_t)m, mu_host, s2_host, acq_host);
        IBO_TRY(run_sweep(g, batch_request(m, dev_in[b], acq, parm, erf_mode, clamp_lo, ymax, out)));
        HIP_TRY(hipEventRecord(g->pe_k[b], g->stream));
        HIP_TRY(hipStreamWaitEvent(g->d2h_stream, g->pe_k[b], 0));
        HIP_TRY(hipMemcpyAsync(pin_out[b], dev_out[b], sizeof(double) * m * out.n, hipMemcpyDeviceToHost, g->d2h_stream));
        HIP_TRY(hipEventRecord(g->pe_out[b], g->d2h_stream));
    }
    if (nch >= 2) IBO_TRY(drain(nch - 2));
    IBO_TRY(drain(nch - 1));
    return IBO_OK;
}

int eval_host_points(ibo_gp *g, int64_t M, const double *Q_host, int acq, double parm, int erf_mode,
                     double clamp_lo, double *mu_host, double *s2_host, double *acq_host, double ymax)
{
    if (M >= ((int64_t)1 << 18) && g_host_pipeline)
        return eval_host_points_pipelined(g, M, Q_host, acq, parm, erf_mode, clamp_lo, mu_host, s2_host, acq_host, ymax);
    IBO_TRY(g->cand.ensure((size_t)M * g->D));
    IBO_TRY(g->outs.ensure(3 * (size_t)M));
    // pinned staging (input points + up to 3 output arrays): pageable copies cost ~15 us each and
    // DIRECT issues ~100 small batches per maximisation
    IBO_TRY(ensure_pinned(g, (size_t)M * (g->D + 3)));
    hipStream_t s = g->stream;
    double *pin_in = g->pin, *pin_out = g->pin + (size_t)M * g->D;
    memcpy(pin_in, Q_host, sizeof(double) * M * g->D);
    // Batches of at most 8192 points skip the copy launches altogether: pinned host memory is device-visible, the
    // kernels read the few KB of candidates from it and store the results into it (two ~10 us launches per batch).
    const bool zero_copy = M <= 8192;
    if (!zero_copy) HIP_TRY(hipMemcpyAsync(g->cand.p, pin_in, sizeof(double) * M * g->D, hipMemcpyHostToDevice, s));
    const Packed3 out = pack3(zero_copy ? pin_out : g->outs.p, (size_t)M, mu_host, s2_host, acq_host);
    SweepRequest r = batch_request(M, zero_copy ? pin_in : g->cand.p, acq, parm, erf_mode, clamp_lo, ymax, out);
    if (zero_copy) { r.cand_host = pin_in; r.signal = true; r.timed = false; }      // small batches: no kernel-time events either
    g->signal_pending = false;
    IBO_TRY(run_sweep(g, r));
    if (!zero_copy) HIP_TRY(hipMemcpyAsync(pin_out, g->outs.p, sizeof(double) * M * out.n, hipMemcpyDeviceToHost, s));
    if (zero_copy) {
        // a batch of this size is back in tens of microseconds: spin for a moment before handing the thread to the runtime's
        // blocking wait (whose wake-up alone costs about as much as the batch) -- on the word small2.hip's last kernel stores
        // behind its results (no event to record, signal and query), or on a completion event for the other kernels
        const bool flag = g->signal_pending;
        if (!flag) HIP_TRY(hipEventRecord(g->fit1, s));
        struct timespec w0, w1;
        clock_gettime(CLOCK_MONOTONIC, &w0);
        for (int spin = 0;; spin++) {
            if (flag) {
                if (*(volatile unsigned long long *)g->done_flag == g->done_seq) break;
                if (spin & 63) continue;
            } else {
                hipError_t q = hipEventQuery(g->fit1);
                if (q == hipSuccess) break;
                if (q != hipErrorNotReady) HIP_TRY(q);
            }
            clock_gettime(CLOCK_MONOTONIC, &w1);
            if ((w1.tv_sec - w0.tv_sec) * 1e6 + (w1.tv_nsec - w0.tv_nsec) * 1e-3 > 300.0) { HIP_TRY(hipStreamSynchronize(s)); break; }
        }
    } else HIP_TRY(hipStreamSynchronize(s));
    unpack3(pin_out, (size_t)M, mu_host, s2_host, acq_host);
    return IBO_OK;
}

extern "C" int ibo_posterior_batch(ibo_gp_t *g, int64_t M, const double *Q_host, double clamp_lo,
                                   double *mu_host, double *s2_host)
{
    if (!g || !Q_host || !mu_host) return fail(IBO_ERR_ARG, "NULL argument");
    if (M < 1) return fail(IBO_ERR_ARG, "M=%lld", (long long)M);
    IBO_TRY(use_device(g->device));
    if (!g->fitted) return fail(IBO_ERR_STATE, "posterior before a successful fit");
    return eval_host_points(g, M, Q_host, IBO_ACQ_NONE, 0.0, IBO_ERF_LIBM, clamp_lo, mu_host, s2_host, nullptr);
}

// host points in, host arrays out (any of mu / s2 / acq may be NULL): what EI(GP).negf(x), PI, UCB and their vectorised
// forms ask for -- small batches cost no allocation and no copy launch (pinned staging read and written by the kernels)
extern "C" int ibo_acq_batch(ibo_gp_t *g, int64_t M, const double *Q_host, int acq, double parm, int erf_mode,
                             double clamp_lo, double ymax, double *mu_host, double *s2_host, double *acq_host)
{
    if (!g || !Q_host || (!mu_host && !s2_host && !acq_host)) return fail(IBO_ERR_ARG, "NULL argument");
    if (M < 1) return fail(IBO_ERR_ARG, "M=%lld", (long long)M);
    if (acq < 0 || acq > 3) return fail(IBO_ERR_ARG, "unknown acquisition %d", acq);
    IBO_TRY(use_device(g->device));
    if (!g->fitted) return fail(IBO_ERR_STATE, "evaluation before a successful fit");
    return eval_host_points(g, M, Q_host, acq, parm, erf_mode, clamp_lo, mu_host, s2_host, acq_host, ymax);
}

// ------------------------------------------------------------------------ gradients with respect to the query point (grad.hip)
// The values (mu, s2, acq) come from eval_host_points -- the very numbers ibo_acq_batch returns; the gradients from the chunks of
// grad.hip, which form their own mu and s2 for the clip rule and the chain rule.  Up to 64 points: the candidates are read from, and the
// gradients written to, the handle's pinned staging (no copy launches).
extern "C" int ibo_acq_grad_batch(ibo_gp_t *g, int64_t M, const double *Q_host, int acq, double parm, int erf_mode,
                                  double clamp_lo, double ymax, double *mu_host, double *s2_host, double *acq_host,
                                  double *dmu_host, double *ds2_host, double *dacq_host)
{
    if (!g || !Q_host) return fail(IBO_ERR_ARG, "NULL argument");
    if (!mu_host && !s2_host && !acq_host && !dmu_host && !ds2_host && !dacq_host) return fail(IBO_ERR_ARG, "every output is NULL");
    if (M < 1) return fail(IBO_ERR_ARG, "M=%lld", (long long)M);
    if (acq < 0 || acq > 3) return fail(IBO_ERR_ARG, "unknown acquisition %d", acq);
    if (erf_mode != IBO_ERF_LIBM && erf_mode != IBO_ERF_NR) return fail(IBO_ERR_ARG, "unknown erf mode %d", erf_mode);
    if (acq == IBO_ACQ_NONE && dacq_host) return fail(IBO_ERR_ARG, "dacq_host with IBO_ACQ_NONE");
    IBO_TRY(use_device(g->device));
    if (!g->fitted) return fail(IBO_ERR_STATE, "gradient before a successful fit");
    if (mu_host || s2_host || acq_host)
        IBO_TRY(eval_host_points(g, M, Q_host, acq, parm, erf_mode, clamp_lo, mu_host, s2_host, acq_host, ymax));
    if (!dmu_host && !ds2_host && !dacq_host) return IBO_OK;
    const int D = g->D;
    hipStream_t s = g->stream;
    const GradPlan pl = grad_plan(g->N, g->Npad, g->DP, M);
    IBO_TRY(g->grad_ws.ensure(pl.ws_doubles));
    GradArgs a;
    memset(&a, 0, sizeof(a));
    a.kp = g->kp; a.N = g->N; a.Npad = g->Npad; a.DP = g->DP;
    a.Xp = g->Xp.p; a.W = g->W.p; a.alphaY = g->alphaY.p; a.alpha1 = g->alpha1.p;
    a.prior = prior_of(g);
    a.noise = g->noise; a.clamp_lo = clamp_lo; a.ymax = (ymax == ymax) ? ymax : g->maxY; a.parm = parm;
    a.acq = acq; a.erf_mode = erf_mode;
    a.TM = pl.TM; a.KC = pl.KC; a.nsplit = pl.nsplit; a.nparts = pl.nparts;
    double *outs_host[3] = {dmu_host, ds2_host, dacq_host};
    const bool zero_copy = M <= 64;                 // (pl.mc >= 64: one chunk)
    if (zero_copy) {
        IBO_TRY(ensure_pinned(g, (size_t)M * D * 4));
        memcpy(g->pin, Q_host, sizeof(double) * M * D);
    } else {
        IBO_TRY(g->grad_cand.ensure((size_t)pl.mc * D));
        IBO_TRY(g->grad_out.ensure((size_t)pl.mc * D * 3));
    }
    for (int64_t c0 = 0; c0 < M; c0 += pl.mc) {
        const int m = (int)(M - c0 < pl.mc ? M - c0 : pl.mc);
        const size_t nk = (size_t)m * g->Npad, np = (size_t)pl.nsplit * nk;
        a.K = g->grad_ws.p; a.H = a.K + nk; a.Pt = a.H + nk; a.Pu = a.Pt + np; a.E = a.Pu + np;
        const double *cand;
        double *obase;
        if (zero_copy) {
            cand = g->pin; obase = g->pin + (size_t)M * D;
        } else {
            HIP_TRY(hipMemcpyAsync(g->grad_cand.p, Q_host + c0 * D, sizeof(double) * m * D, hipMemcpyHostToDevice, s));
            cand = g->grad_cand.p; obase = g->grad_out.p;
        }
        double *od[3];
        for (int k = 0; k < 3; k++) od[k] = outs_host[k] ? obase + (size_t)k * m * D : nullptr;
        KERNEL_TRY(launch_grad(a, cand, m, od[0], od[1], od[2], s));
        if (!zero_copy)
            for (int k = 0; k < 3; k++)
                if (outs_host[k]) HIP_TRY(hipMemcpyAsync(outs_host[k] + c0 * D, od[k], sizeof(double) * m * D, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        if (zero_copy)
            for (int k = 0; k < 3; k++)
                if (outs_host[k]) memcpy(outs_host[k], od[k], sizeof(double) * M * D);
    }
    return IBO_OK;
}

// ------------------------------------------------------------------------ joint posterior and draws from it (cov.hip)
// mu: the launch sequence of ibo_posterior_batch (the same numbers, bit for bit)
static int cov_mean(ibo_gp *g, int64_t M, const double *Q_host, double *mu_host)
{
    std::vector<double> s2((size_t)M);
    return eval_host_points(g, M, Q_host, IBO_ACQ_NONE, 0.0, IBO_ERF_LIBM, 1e-7, mu_host, s2.data(), nullptr);
}

int vt_rows(ibo_gp *g, const double *pts_dev, int m, int mp, double *kt, double *vt, hipStream_t s)
{
    KERNEL_TRY(launch_cov_kstar(g->kp, g->Xp.p, g->N, g->Npad, g->DP, pts_dev, m, mp, kt, s));
    KERNEL_TRY(launch_cov_tri(kt, (size_t)g->Npad, g->W.p, (size_t)g->Npad, g->N, mp, g->Npad, vt, (size_t)g->Npad, s));
    return IBO_OK;
}

// Sigma of the M points into S (device, ld lds), diagonal rule diag - |v_a|^2; pad: rows and columns [M, round_up(M, 64)) identity.
// Scratch: the points, V^T (Mp x Npad) and one chunk of K* (at most 256 MiB, at least 64 points); handed back on every exit path.
static int cov_sigma(ibo_gp *g, int64_t M, const double *Q_host, double diag, int pad, double *S, size_t lds)
{
    const int N = g->N, Np = g->Npad, D = g->D, Mp = round_up((int)M, IBO_COV_TILE);
    hipStream_t s = g->stream;
    int mc = (int)((((size_t)256 << 20) / ((size_t)Np * sizeof(double))) / IBO_COV_TILE * IBO_COV_TILE);
    mc = mc < IBO_COV_TILE ? IBO_COV_TILE : (mc > Mp ? Mp : mc);
    ScopedBuf<double> q, kt, vt;
    IBO_TRY(q.ensure((size_t)M * D)); IBO_TRY(kt.ensure((size_t)mc * Np)); IBO_TRY(vt.ensure((size_t)Mp * Np));
    HIP_TRY(hipMemcpyAsync(q.p, Q_host, sizeof(double) * (size_t)M * D, hipMemcpyHostToDevice, s));
    for (int c0 = 0; c0 < Mp; c0 += mc) {
        const int mp = Mp - c0 < mc ? Mp - c0 : mc;
        const int m = (int)(M - c0 < mp ? M - c0 : mp);           // >= 1: c0 <= Mp - 64 < M
        IBO_TRY(vt_rows(g, q.p + (size_t)c0 * D, m, mp, kt.p, vt.p + (size_t)c0 * Np, s));
    }
    KERNEL_TRY(launch_cov_syrk(g->kp, q.p, vt.p, (size_t)Np, round_up(N, 32), (int)M, Mp, diag, pad, S, lds, s));
    HIP_TRY(hipStreamSynchronize(s));
    return IBO_OK;
}

extern "C" int ibo_posterior_cov(ibo_gp_t *g, int64_t M, const double *Q_host, int with_noise, double *mu_host, double *S_host)
{
    IBO_TRY(use_device(g ? g->device : 0));
    if (!g || !Q_host || !S_host) return fail(IBO_ERR_ARG, "NULL argument");
    if (M < 1 || M > IBO_COV_MAX_M) return fail(IBO_ERR_ARG, "M=%lld outside [1, %d]", (long long)M, IBO_COV_MAX_M);
    if (!g->fitted) return fail(IBO_ERR_STATE, "posterior covariance before a successful fit");
    if (mu_host) IBO_TRY(cov_mean(g, M, Q_host, mu_host));
    hipStream_t s = g->stream;
    ScopedBuf<double> S;
    IBO_TRY(S.ensure((size_t)M * M));
    HIP_TRY(hipEventRecord(g->ev0, s));
    IBO_TRY(cov_sigma(g, M, Q_host, with_noise ? 1.0 + g->noise : 1.0, 0, S.p, (size_t)M));
    HIP_TRY(hipMemcpyAsync(S_host, S.p, sizeof(double) * (size_t)M * M, hipMemcpyDeviceToHost, s));
    return finish_span(g);
}

// Sigma + jitter I padded to Mp = round_up(M, 64) rows (identity pad), factored in place by ibo_spd_*'s route, then F = Z L^T on the
// MFMA pipe.  Sigma never leaves the device.
extern "C" int ibo_posterior_sample(ibo_gp_t *g, int64_t M, const double *Q_host, int with_noise, double jitter, int nsamp,
                                    const double *Z_host, double *F_host, double *mu_host, int *info)
{
    IBO_TRY(use_device(g ? g->device : 0));
    if (!g || !Q_host || !Z_host || !F_host) return fail(IBO_ERR_ARG, "NULL argument");
    if (M < 1 || M > IBO_SAMPLE_MAX_M) return fail(IBO_ERR_ARG, "M=%lld outside [1, %d]", (long long)M, IBO_SAMPLE_MAX_M);
    if (nsamp < 1 || nsamp > IBO_SAMPLE_MAX_DRAWS) return fail(IBO_ERR_ARG, "nsamp=%d outside [1, %d]", nsamp, IBO_SAMPLE_MAX_DRAWS);
    if (!(jitter >= 0.0 && jitter < HUGE_VAL)) return fail(IBO_ERR_ARG, "jitter=%g is not a finite value >= 0", jitter);
    if (!g->fitted) return fail(IBO_ERR_STATE, "posterior draws before a successful fit");
    if (info) *info = 0;
    if (mu_host) IBO_TRY(cov_mean(g, M, Q_host, mu_host));
    hipStream_t s = g->stream;
    const int Mp = round_up((int)M, IBO_COV_TILE), Sp = round_up(nsamp, IBO_COV_TILE);
    ScopedBuf<double> S, d64, Z, F;
    ScopedBuf<int> dinfo;
    IBO_TRY(S.ensure((size_t)Mp * Mp)); IBO_TRY(d64.ensure(diag64_size(Mp))); IBO_TRY(dinfo.ensure(1));
    IBO_TRY(Z.ensure((size_t)Sp * Mp)); IBO_TRY(F.ensure((size_t)Sp * Mp));
    HIP_TRY(hipEventRecord(g->ev0, s));
    IBO_TRY(cov_sigma(g, M, Q_host, (with_noise ? 1.0 + g->noise : 1.0) + jitter, 1, S.p, (size_t)Mp));
    KERNEL_TRY(launch_cholesky(S.p, Mp, d64.p, dinfo.p, s));                  // (FACTOR_IN_PLACE's route; only the factor is wanted)
    char noun[64];
    snprintf(noun, sizeof noun, "posterior covariance + %g I", jitter);
    IBO_TRY(factor_info(dinfo.p, s, noun, info));
    HIP_TRY(hipMemsetAsync(Z.p, 0, sizeof(double) * (size_t)Sp * Mp, s));
    HIP_TRY(hipMemcpy2DAsync(Z.p, sizeof(double) * Mp, Z_host, sizeof(double) * M, sizeof(double) * M, nsamp, hipMemcpyHostToDevice, s));
    KERNEL_TRY(launch_cov_tri(Z.p, (size_t)Mp, S.p, (size_t)Mp, (int)M, Sp, Mp, F.p, (size_t)Mp, s));
    HIP_TRY(hipMemcpy2DAsync(F_host, sizeof(double) * M, F.p, sizeof(double) * Mp, sizeof(double) * M, nsamp, hipMemcpyDeviceToHost, s));
    return finish_span(g);
}

// ------------------------------------------------------------------------ DIRECT on a GPU objective
int direct_maximize(const ibo::batch_eval_t &value, const char *label, int D, const double *lb, const double *ub,
                    int maxiter, int maxtime, int maxsample, int compat, double *opt, double *optx, int64_t *nsamples)
{
    const bool dbg = getenv("IBO_DEBUG") != nullptr;
    double t_eval = 0.0; int n_batches = 0; int64_t n_pts = 0;
    ibo::batch_eval_t ev = [&](const double *pts, int n, double *vals) -> int {
        struct timespec a0, a1;
        if (dbg) clock_gettime(CLOCK_MONOTONIC, &a0);
        const int rc = value(pts, n, vals);
        if (dbg) { clock_gettime(CLOCK_MONOTONIC, &a1); t_eval += (a1.tv_sec - a0.tv_sec) * 1e3 + (a1.tv_nsec - a0.tv_nsec) * 1e-6; n_batches++; n_pts += n; }
        if (rc) return rc;
        for (int i = 0; i < n; i++) vals[i] = -vals[i];     // DIRECT minimises the negated value
        return 0;
    };
    ibo::DirectOptions o;
    o.maxiter = maxiter; o.maxtime = maxtime; o.maxsample = maxsample; o.compat = compat != 0;
    o.per_rectangle = false;
    struct timespec w0, w1;
    clock_gettime(CLOCK_MONOTONIC, &w0);
    ibo::DirectResult r = ibo::direct_minimize(ev, D, lb, ub, o);
    clock_gettime(CLOCK_MONOTONIC, &w1);
    if (dbg) fprintf(stderr, "[libibo_hip] %s: %d iterations, %lld samples, %d batches (%lld points): %.2f ms total, %.2f ms in evaluation\n",
                     label, r.iterations, (long long)r.nsamples, n_batches, (long long)n_pts,
                     (w1.tv_sec - w0.tv_sec) * 1e3 + (w1.tv_nsec - w0.tv_nsec) * 1e-6, t_eval);
    if (r.status) return r.status;
    if (opt) *opt = -r.fmin;
    if (optx) for (int i = 0; i < D; i++) optx[i] = r.xmin[i];
    if (nsamples) *nsamples = r.nsamples;
    return IBO_OK;
}

int direct_on_gp(ibo_gp *g, int D, const double *lb, const double *ub, int acq, double parm, int erf_mode,
                 double clamp_lo, int maxiter, int maxtime, int maxsample, int compat,
                 double *opt, double *optx, int64_t *nsamples)
{
    if (D != g->D) return fail(IBO_ERR_ARG, "bounds have %d dimensions, model has %d", D, g->D);
    const ibo::batch_eval_t value = [&](const double *pts, int n, double *vals) -> int {
        return eval_host_points(g, n, pts, acq, parm, erf_mode, clamp_lo, nullptr, nullptr, vals);
    };
    return direct_maximize(value, "DIRECT", D, lb, ub, maxiter, maxtime, maxsample, compat, opt, optx, nsamples);
}

extern "C" int ibo_direct_max(ibo_gp_t *g, int D, const double *lb, const double *ub, int acq, double parm,
                              int erf_mode, double clamp_lo, int maxiter, int maxtime, int maxsample,
                              int compat, double *opt, double *optx, int64_t *nsamples)
{
    if (!g || !lb || !ub) return fail(IBO_ERR_ARG, "NULL argument");
    if (acq < 0 || acq > 2) return fail(IBO_ERR_ARG, "unknown acquisition %d", acq);
    IBO_TRY(use_device(g->device));
    if (!g->fitted) return fail(IBO_ERR_STATE, "direct before a successful fit");
    return direct_on_gp(g, D, lb, ub, acq, parm, erf_mode, clamp_lo, maxiter, maxtime, maxsample, compat,
                        opt, optx, nsamples);
}

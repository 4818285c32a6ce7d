// abi_sparse.hip -- a sparse GP on inducing points (DTC / FITC) behind the C ABI: ibo_sgp_* (kernels: sparse.hip; the per-frame work:
// fit_begin / fit_factor and run_sweep).
//
// The handle wraps two ibo_gp frames on the m inducing points Z that no other entry ever sees:
//   U  a plain fit with noise = jitter: L_u, W_u; its plain sweep gives s2_U = 1 + jitter - q
//   A  staged on the same points, then fit_factor(have_A = true) on A = K~uu + G with the noise field 0 and the targets b: its alpha
//      vector is the model's, its plain sweep gives mu = k_u^T alpha and s2_A = 1 - |W_A k_u|^2
// and keeps G+ = [F; y~] [F; y~]^T (lower 64 x 64 tiles), ll, tt, N and the largest target.  The observations pass through in chunks and
// are not kept.
//   chunk of data     upload (pinned staging) -> U sweep (s2_U, unclipped) -> sgp_scaled_kuf_kernel -> sgp_gram_kernel, on the A frame's stream
//   refactor          K~uu (the U frame's R) + G -> sgp_assemble_kernel -> fit_factor on the A frame
//   chunk of points   U sweep, A sweep into pool scratch -> sgp_finish_kernel; launch_argmax_final for the winner (abi_moments.h)
// Host batches and DIRECT are uploaded and take the route of the sweep: the same bits within a size class of the plain sweep (class_padded).
// ibo_sgp_nlml_grad (at the end; kernels: sparse_grad.hip) is stateless: ibo_sgp_fit on a private per-device handle, then
//   the inverses      A^-1 = W_A^T W_A, K~uu^-1 = W_u^T W_u (launch_wtw)
//   chunk of data     upload -> U sweep, A sweep (q, mu, a) -> sgp_grad_obs_kernel -> sgp_grad_gen_kernel -> sgp_grad_contract_kernel
//                     -> sgp_grad_reduce_kernel; not for dtc: H += (K E) K^T (sgp_abt_kernel)
//   after the chunks  S from A^-1, K~uu^-1, alpha and K~uu^-1 H K~uu^-1, then the contraction kernel again with Z as the observations
#include "abi_moments.h"
#include "abi_factor.h"
#include "sparse.h"
#include "sparse_grad.h"

std::atomic<int> g_sgp_chunk{0};      // ibo_set_option("sgp_chunk", n): observations / candidates per chunk (rounded up to 256); 0: by bytes
std::atomic<int> g_sgp_timing{0};     // ibo_set_option("sgp_timing", 1): HIP events around every stage, read with ibo_sgp_stage_ms
static thread_local double t_sgp_ms[IBO_SGP_STAGES];
static thread_local double t_sgp_grad_ms[IBO_SGP_GRAD_STAGES];
enum { SGP_GR_FIT = 0, SGP_GR_INVERSES, SGP_GR_SWEEPS, SGP_GR_GEN, SGP_GR_CONTRACT, SGP_GR_GRAM, SGP_GR_UU, SGP_GR_REDUCE };
enum { SGP_ST_Q = 0, SGP_ST_GEN, SGP_ST_GRAM, SGP_ST_ASSEMBLE, SGP_ST_FACTOR, SGP_ST_SWEEPS, SGP_ST_FINISH };

struct ibo_sgp {
    ibo_gp *gu = nullptr, *ga = nullptr;     // the two m-row frames
    int device = 0, m = 0, mp = 0, D = 0, method = IBO_SGP_FITC;
    bool fitted = false;
    int64_t N = 0;
    KParams kp;
    double noise = 0.0, jitter = 0.0, maxY = 0.0, ll = 0.0, tt = 0.0;
    double logdet_u = 0.0, logdet_a = 0.0, wb2 = 0.0;      // 2 sum log L_ii of both factors; |W_A b|^2
    DevBuf<double> Gp;                       // (mp + 64)^2
    void release() { Gp.release(); }
    double *pin = nullptr; size_t pin_cap = 0;
};

namespace {

int sgp_pinned(ibo_sgp *h, size_t need)
{
    if (need <= h->pin_cap) return IBO_OK;
    if (h->pin) (void)hipHostFree(h->pin);
    h->pin = nullptr; h->pin_cap = 0;
    HIP_TRY(hipHostMalloc((void **)&h->pin, sizeof(double) * need, hipHostMallocDefault));
    h->pin_cap = need;
    alloc_fill_host(h->pin, sizeof(double) * need);
    return IBO_OK;
}

bool all_finite(const double *p, size_t n)
{
    for (size_t i = 0; i < n; i++)
        if (!std::isfinite(p[i])) return false;
    return true;
}

// n observations into G+, ll, tt, N and the largest target; chunks in ascending order on the A frame's stream
int sgp_accumulate(ibo_sgp *h, int64_t n, const double *X, const double *Y, double *lambda_host)
{
    ibo_gp *gu = h->gu, *ga = h->ga;
    hipStream_t su = gu->stream, sa = ga->stream;
    const int D = h->D, m = h->m, mp = h->mp;
    const int64_t nc = moments_chunk_length(n, 8 * (int64_t)(mp + 64), g_sgp_chunk, (int64_t)256 << 20);
    const int64_t rows = class_padded(nc, nc), ldmax = (nc + 31) / 32 * 32, nblkmax = (nc + 255) / 256;
    ScopedBuf<double> xc, yc, s2, Ft, lam, part;
    IBO_TRY(xc.ensure((size_t)rows * D)); IBO_TRY(yc.ensure((size_t)nc)); IBO_TRY(s2.ensure((size_t)rows));
    IBO_TRY(Ft.ensure((size_t)(mp + 64) * ldmax)); IBO_TRY(lam.ensure((size_t)nc)); IBO_TRY(part.ensure(2 * (size_t)nblkmax));
    IBO_TRY(sgp_pinned(h, (size_t)rows * D + 2 * (size_t)nc + 2 * (size_t)nblkmax));
    SpanClock clock;
    IBO_TRY(clock.make(g_sgp_timing != 0));
    for (int64_t c0 = 0; c0 < n; c0 += nc) {
        const int64_t k = n - c0 < nc ? n - c0 : nc, kp = class_padded(k, nc), nblk = (k + 255) / 256;
        double *px = h->pin, *py = px + (size_t)rows * D, *pl = py + nc, *pp = pl + nc;
        memcpy(px, X + (size_t)c0 * D, sizeof(double) * (size_t)k * D);
        memset(px + (size_t)k * D, 0, sizeof(double) * (size_t)(kp - k) * D);       // the sweep's padding to its size class: points at the origin
        memcpy(py, Y + c0, sizeof(double) * (size_t)k);
        for (int64_t i = 0; i < k; i++)
            if (h->N + c0 + i == 0 || py[i] > h->maxY) h->maxY = py[i];
        HIP_TRY(hipMemcpyAsync(xc.p, px, sizeof(double) * (size_t)kp * D, hipMemcpyHostToDevice, su));
        HIP_TRY(hipMemcpyAsync(yc.p, py, sizeof(double) * (size_t)k, hipMemcpyHostToDevice, su));
        // q of the chunk: the U frame's plain sweep, nothing clipped from below (s2_U = 1 + jitter - q).  DTC's lambda does not read it;
        // the sum tt -- the VFE bound's trace term -- does.
        SweepRequest r;
        r.M = kp; r.cand_dev = xc.p; r.acq = IBO_ACQ_NONE; r.clamp_lo = -1.0; r.s2_dev = s2.p;
        IBO_TRY(clock.start(su));
        IBO_TRY(run_sweep(gu, r));
        IBO_TRY(clock.stop(su, &t_sgp_ms[SGP_ST_Q]));
        HIP_TRY(hipStreamSynchronize(su));                       // the generation runs on the A frame's stream
        SgpKufArgs a;
        memset(&a, 0, sizeof(a));
        a.kp = h->kp; a.m = m; a.mp = mp; a.Z = ga->Xp.p; a.ldz = ga->DP; a.X = xc.p; a.n = (int)k; a.Y = yc.p; a.s2u = s2.p;
        a.fitc = h->method == IBO_SGP_FITC; a.noise = h->noise; a.jitter = h->jitter; a.ld = (int)((k + 31) / 32 * 32);
        a.Ft = Ft.p; a.lam = lam.p; a.part = part.p;
        IBO_TRY(clock.start(sa));
        KERNEL_TRY(launch_sgp_scaled_kuf(a, sa));
        IBO_TRY(clock.stop(sa, &t_sgp_ms[SGP_ST_GEN]));
        IBO_TRY(clock.start(sa));
        KERNEL_TRY(launch_sgp_gram(Ft.p, a.ld, mp, h->Gp.p, sa));
        IBO_TRY(clock.stop(sa, &t_sgp_ms[SGP_ST_GRAM]));
        HIP_TRY(hipMemcpyAsync(pp, part.p, sizeof(double) * 2 * (size_t)nblk, hipMemcpyDeviceToHost, sa));
        if (lambda_host) HIP_TRY(hipMemcpyAsync(pl, lam.p, sizeof(double) * (size_t)k, hipMemcpyDeviceToHost, sa));
        HIP_TRY(hipStreamSynchronize(sa));                       // the staging and the scratch are the next chunk's
        for (int64_t b = 0; b < nblk; b++) { h->ll += pp[b]; h->tt += pp[nblk + b]; }     // ascending blocks of 256: the chunking does not show
        if (lambda_host) memcpy(lambda_host + c0, pl, sizeof(double) * (size_t)k);
    }
    h->N += n;
    return IBO_OK;
}

// 2 sum log L_ii of a frame's factor
int sgp_logdet(ibo_gp *g, double *out)
{
    std::vector<double> d((size_t)g->N);
    HIP_TRY(hipMemcpy2D(d.data(), sizeof(double), g->L.p, sizeof(double) * ((size_t)g->Npad + 1), sizeof(double), (size_t)g->N, hipMemcpyDeviceToHost));
    double s = 0.0;
    for (int i = 0; i < g->N; i++) s += log(d[i]);
    *out = 2.0 * s;
    return IBO_OK;
}

// A = K~uu + G and b into the A frame, then its factorisation
int sgp_refactor(ibo_sgp *h, int *info)
{
    ibo_gp *gu = h->gu, *ga = h->ga;
    hipStream_t sa = ga->stream;
    const int m = h->m, mp = h->mp;
    SpanClock clock;
    IBO_TRY(clock.make(g_sgp_timing != 0));
    IBO_TRY(ensure_R(gu));
    HIP_TRY(hipStreamSynchronize(gu->stream));
    IBO_TRY(ga->A.ensure((size_t)m * m));
    IBO_TRY(clock.start(sa));
    KERNEL_TRY(launch_sgp_assemble(gu->R.p, gu->Npad, h->Gp.p, mp + 64, m, mp, ga->Npad, ga->A.p, ga->Y.p, sa));
    IBO_TRY(clock.stop(sa, &t_sgp_ms[SGP_ST_ASSEMBLE]));
    ga->maxY = h->maxY;
    ga->st_gen = 0;
    IBO_TRY(clock.start(sa));
    const int rc = fit_factor(ga, h->kp, m, 0.0, true, info);        // synchronises
    if (rc == IBO_ERR_NOT_PD) return fail(IBO_ERR_NOT_PD, "A = K~uu + G is not positive definite (pivot %d)", info ? *info : -1);
    IBO_TRY(rc);
    IBO_TRY(clock.stop(sa, &t_sgp_ms[SGP_ST_FACTOR]));
    // |W_A b|^2 from launch_alpha's first product (fit_alpha left W_A b at the head of the frame's scratch)
    std::vector<double> wb((size_t)m);
    HIP_TRY(hipMemcpy(wb.data(), ga->tmp.p, sizeof(double) * (size_t)m, hipMemcpyDeviceToHost));
    double s = 0.0;
    for (int i = 0; i < m; i++) s += wb[i] * wb[i];
    h->wb2 = s;
    return sgp_logdet(ga, &h->logdet_a);
}

struct SgpCall { int acq, erf_mode; double parm, clamp_lo, ymax; };
enum { SGP_OUT_MU = 0, SGP_OUT_S2, SGP_OUT_ACQ };           // MomentsPipeline::out

// The one route of every evaluating entry: per chunk s2_U from the U frame, (mu, s2_A) from the A frame -- nothing is clipped before the
// composition -- then sgp_finish_kernel on the A frame's stream.
void sgp_pipeline(ibo_sgp *h, const SgpCall &c, MomentsPipeline *p)
{
    p->add(h->gu, false, true, -1.0, IBO_ERF_LIBM);
    p->add(h->ga, true, true, -1.0, IBO_ERF_LIBM);
    p->home = h->ga; p->chunk_opt = g_sgp_chunk; p->timing = g_sgp_timing != 0;
    p->sweeps_ms = &t_sgp_ms[SGP_ST_SWEEPS]; p->finish_ms = &t_sgp_ms[SGP_ST_FINISH];
    p->finish = [h, &c, p](const MomentChunk &k, hipStream_t s) -> int {
        SgpFinishArgs a;
        memset(&a, 0, sizeof(a));
        a.noise = h->noise; a.jitter = h->jitter; a.clamp_lo = c.clamp_lo; a.ymax = c.ymax == c.ymax ? c.ymax : h->maxY; a.parm = c.parm;
        a.acq = c.acq; a.erf_mode = c.erf_mode;
        a.t = k.tail; a.s2u = k.ms; a.mua = k.ms + k.stride; a.s2a = k.ms + 2 * k.stride;
        a.out_mu = k.at(p->out[SGP_OUT_MU]); a.out_s2 = k.at(p->out[SGP_OUT_S2]); a.out_acq = k.at(p->out[SGP_OUT_ACQ]);
        KERNEL_TRY(launch_sgp_finish(a, s));
        return IBO_OK;
    };
}

// Host points through the sweep's own route -- the device's values are the sweep's bits.
int sgp_eval_host(ibo_sgp *h, const SgpCall &c, int64_t M, const double *Q_host, double *mu, double *s2, double *acq)
{
    MomentsPipeline p;
    sgp_pipeline(h, c, &p);
    double *const host[3] = {mu, s2, acq};
    const size_t len[3] = {(size_t)M, (size_t)M, (size_t)M};
    return p.eval_host(M, Q_host, 3, host, len);
}

}  // namespace

extern "C" int ibo_sgp_create(int device, ibo_sgp_t **out)
{
    if (!out) return fail(IBO_ERR_ARG, "out is NULL");
    ibo_gp *gu = nullptr, *ga = nullptr;
    IBO_TRY(ibo_gp_create(device, &gu));
    const int rc = ibo_gp_create(device, &ga);
    if (rc != IBO_OK) { (void)ibo_gp_destroy(gu); return rc; }
    ibo_sgp *h = new ibo_sgp();
    h->gu = gu; h->ga = ga; h->device = device;
    memset(&h->kp, 0, sizeof(h->kp));
    *out = h;
    return IBO_OK;
}

extern "C" int ibo_sgp_destroy(ibo_sgp_t *h)
{
    if (!h) return IBO_OK;
    (void)hipSetDevice(h->device);
    (void)hipDeviceSynchronize();
    g_pool_quiet = true;
    h->release();
    g_pool_quiet = false;
    if (h->pin) (void)hipHostFree(h->pin);
    const int r1 = ibo_gp_destroy(h->gu), r2 = ibo_gp_destroy(h->ga);
    delete h;
    return r1 != IBO_OK ? r1 : r2;
}

extern "C" int ibo_sgp_fit(ibo_sgp_t *h, int ktype, int D, const double *hyper, int nhyper, double sf2, double noise, double jitter, int method,
                           int m, const double *Z, int64_t N, const double *X, const double *Y, double *lambda_host, int *info)
{
    if (!h) return fail(IBO_ERR_ARG, "handle is NULL");
    IBO_TRY(use_device(h->device));
    if (!Z || !X || !Y) return fail(IBO_ERR_ARG, "Z/X/Y is NULL");
    if (m < 1 || m > IBO_SGP_MAX_M) return fail(IBO_ERR_ARG, "m=%d inducing points, not 1 .. %d", m, IBO_SGP_MAX_M);
    if (N < 1) return fail(IBO_ERR_ARG, "N=%lld", (long long)N);
    if (method != IBO_SGP_FITC && method != IBO_SGP_DTC) return fail(IBO_ERR_ARG, "unknown method %d", method);
    if (!(noise > 0.0) || !std::isfinite(noise)) return fail(IBO_ERR_ARG, "noise=%g", noise);
    if (!(jitter >= 0.0) || !std::isfinite(jitter)) return fail(IBO_ERR_ARG, "jitter=%g", jitter);
    KParams kp;
    IBO_TRY(make_kparams(ktype, D, hyper, nhyper, sf2, &kp));
    if (!all_finite(Z, (size_t)m * D)) return fail(IBO_ERR_ARG, "Z holds a value that is not finite");
    if (!all_finite(X, (size_t)N * D)) return fail(IBO_ERR_ARG, "X holds a value that is not finite");
    if (!all_finite(Y, (size_t)N)) return fail(IBO_ERR_ARG, "Y holds a value that is not finite");
    if (info) *info = 0;
    h->fitted = false;
    h->m = m; h->mp = round_up(m, 64); h->D = D; h->method = method; h->kp = kp; h->noise = noise; h->jitter = jitter;
    h->N = 0; h->ll = 0.0; h->tt = 0.0; h->maxY = 0.0;
    const std::vector<double> zero((size_t)m, 0.0);
    // U: a plain fit on Z with noise = jitter
    int rc = ibo_gp_fit(h->gu, ktype, m, D, Z, zero.data(), hyper, nhyper, sf2, jitter, info);
    if (rc == IBO_ERR_NOT_PD) return fail(IBO_ERR_NOT_PD, "K~uu = K(Z, Z) + jitter is not positive definite (pivot %d)", info ? *info : -1);
    IBO_TRY(rc);
    IBO_TRY(sgp_logdet(h->gu, &h->logdet_u));
    // A: the same points staged (scaled copies, packed operands); its matrix and targets come from sgp_assemble_kernel
    IBO_TRY(fit_begin(h->ga, ktype, m, D, Z, zero.data(), hyper, nhyper, sf2, 0.0, false, &kp));
    const size_t gn = (size_t)(h->mp + 64) * (h->mp + 64);
    IBO_TRY(h->Gp.ensure(gn));
    HIP_TRY(hipMemsetAsync(h->Gp.p, 0, sizeof(double) * gn, h->ga->stream));
    HIP_TRY(hipStreamSynchronize(h->ga->stream));               // (the staging's pinned buffer is free again)
    IBO_TRY(sgp_accumulate(h, N, X, Y, lambda_host));
    IBO_TRY(sgp_refactor(h, info));
    h->fitted = true;
    return IBO_OK;
}

extern "C" int ibo_sgp_add(ibo_sgp_t *h, int64_t n, const double *X, const double *Y, double *lambda_host, int *info)
{
    if (!h) return fail(IBO_ERR_ARG, "handle is NULL");
    IBO_TRY(use_device(h->device));
    if (!X || !Y) return fail(IBO_ERR_ARG, "X/Y is NULL");
    if (n < 1) return fail(IBO_ERR_ARG, "n=%lld", (long long)n);
    if (!h->fitted) return fail(IBO_ERR_STATE, "ibo_sgp_add before a successful fit");
    if (!all_finite(X, (size_t)n * h->D)) return fail(IBO_ERR_ARG, "X holds a value that is not finite");
    if (!all_finite(Y, (size_t)n)) return fail(IBO_ERR_ARG, "Y holds a value that is not finite");
    if (info) *info = 0;
    h->fitted = false;                                           // the kept sums are being rewritten: a failure leaves the handle unfitted
    IBO_TRY(sgp_accumulate(h, n, X, Y, lambda_host));
    IBO_TRY(sgp_refactor(h, info));
    h->fitted = true;
    return IBO_OK;
}

extern "C" int ibo_sgp_acq_batch(ibo_sgp_t *h, int64_t M, const double *Q_host, int acq, double parm, int erf_mode,
                                 double clamp_lo, double ymax, double *mu_host, double *s2_host, double *acq_host)
{
    IBO_TRY(wrapped_check(h, "sparse", Q_host != nullptr, M, acq, erf_mode, true));
    if (!mu_host && !s2_host && !acq_host) return fail(IBO_ERR_ARG, "every output is NULL");
    const SgpCall c = {acq, erf_mode, parm, clamp_lo, ymax};
    return sgp_eval_host(h, c, M, Q_host, mu_host, s2_host, acq_host);
}

extern "C" int ibo_sgp_acq_sweep(ibo_sgp_t *h, int64_t M, const double *cand_dev, int acq, double parm, int erf_mode, double clamp_lo, double ymax,
                                 int n_excl, const double *excl_host, double excl_radius, int64_t index_base,
                                 double *mu_dev, double *s2_dev, double *acq_dev, double *best_val, int64_t *best_idx)
{
    IBO_TRY(wrapped_check(h, "sparse", cand_dev != nullptr, M, acq, erf_mode, true));
    if (!mu_dev && !s2_dev && !acq_dev && !best_val && !best_idx) return fail(IBO_ERR_ARG, "every output is NULL");
    const SgpCall c = {acq, erf_mode, parm, clamp_lo, ymax};
    MomentsPipeline p;
    sgp_pipeline(h, c, &p);
    p.out[SGP_OUT_MU] = mu_dev; p.out[SGP_OUT_S2] = s2_dev; p.out[SGP_OUT_ACQ] = acq_dev;
    return p.sweep(M, cand_dev, M, n_excl, excl_host, excl_radius, index_base, best_val, best_idx);
}

extern "C" int ibo_sgp_direct_max(ibo_sgp_t *h, int D, const double *lb, const double *ub, int acq, double parm, int erf_mode,
                                  double clamp_lo, int maxiter, int maxtime, int maxsample, int compat,
                                  double *opt, double *optx, int64_t *nsamples)
{
    IBO_TRY(wrapped_check(h, "sparse", lb && ub, 1, acq, erf_mode, false));
    if (!opt && !optx && !nsamples) return fail(IBO_ERR_ARG, "every output is NULL");
    if (D != h->D) return fail(IBO_ERR_ARG, "bounds have %d dimensions, the model has %d", D, h->D);
    const SgpCall c = {acq, erf_mode, parm, clamp_lo, NAN};
    const ibo::batch_eval_t value = [&](const double *pts, int n, double *vals) -> int {
        return sgp_eval_host(h, c, n, pts, nullptr, nullptr, vals);
    };
    return direct_maximize(value, "sparse-model DIRECT", D, lb, ub, maxiter, maxtime, maxsample, compat, opt, optx, nsamples);
}

static int sgp_yy(ibo_sgp *h, double *yy)
{
    const size_t ldg = (size_t)h->mp + 64;
    HIP_TRY(hipMemcpy(yy, h->Gp.p + (size_t)h->mp * ldg + h->mp, sizeof(double), hipMemcpyDeviceToHost));
    return IBO_OK;
}

extern "C" int ibo_sgp_nlml(ibo_sgp_t *h, int kind, double *value)
{
    IBO_TRY(use_device(h ? h->device : 0));
    if (!h || !value) return fail(IBO_ERR_ARG, "NULL argument");
    if (kind != IBO_SGP_NLML_MODEL && kind != IBO_SGP_NLML_VFE) return fail(IBO_ERR_ARG, "unknown kind %d", kind);
    if (!h->fitted) return fail(IBO_ERR_STATE, "marginal likelihood before a successful fit");
    if (kind == IBO_SGP_NLML_VFE && h->method != IBO_SGP_DTC)
        return fail(IBO_ERR_ARG, "the variational bound is the DTC value plus a trace term: the model was fitted as FITC");
    double yy = 0.0;
    IBO_TRY(sgp_yy(h, &yy));
    double v = 0.5 * (h->ll + h->logdet_a - h->logdet_u + yy - h->wb2 + (double)h->N * log(2.0 * M_PI));
    if (kind == IBO_SGP_NLML_VFE) v += h->tt / (2.0 * h->noise);
    *value = v;
    return IBO_OK;
}

extern "C" int ibo_sgp_get(ibo_sgp_t *h, int what, double *out)
{
    IBO_TRY(use_device(h ? h->device : 0));
    if (!h || !out) return fail(IBO_ERR_ARG, "NULL argument");
    if (!h->fitted) return fail(IBO_ERR_STATE, "ibo_sgp_get before a successful fit");
    const int m = h->m;
    const size_t ldg = (size_t)h->mp + 64;
    switch (what) {
    case IBO_SGP_GET_KUU: return ibo_gp_get_R(h->gu, out);
    case IBO_SGP_GET_G:
        HIP_TRY(hipMemcpy2D(out, sizeof(double) * m, h->Gp.p, sizeof(double) * ldg, sizeof(double) * m, (size_t)m, hipMemcpyDeviceToHost));
        for (int a = 0; a < m; a++)                              // (only the lower tiles are kept)
            for (int b = a + 1; b < m; b++) out[(size_t)a * m + b] = out[(size_t)b * m + a];
        return IBO_OK;
    case IBO_SGP_GET_A:
        HIP_TRY(hipMemcpy(out, h->ga->A.p, sizeof(double) * (size_t)m * m, hipMemcpyDeviceToHost));
        return IBO_OK;
    case IBO_SGP_GET_LU: return ibo_gp_get_L(h->gu, out);
    case IBO_SGP_GET_LA: return ibo_gp_get_L(h->ga, out);
    case IBO_SGP_GET_B:
        HIP_TRY(hipMemcpy(out, h->ga->Y.p, sizeof(double) * (size_t)m, hipMemcpyDeviceToHost));
        return IBO_OK;
    case IBO_SGP_GET_ALPHA:
        HIP_TRY(hipMemcpy(out, h->ga->alphaY.p, sizeof(double) * (size_t)m, hipMemcpyDeviceToHost));
        return IBO_OK;
    case IBO_SGP_GET_YY: return sgp_yy(h, out);
    case IBO_SGP_GET_LL: *out = h->ll; return IBO_OK;
    case IBO_SGP_GET_TT: *out = h->tt; return IBO_OK;
    case IBO_SGP_GET_N: *out = (double)h->N; return IBO_OK;
    }
    return fail(IBO_ERR_ARG, "unknown quantity %d", what);
}

extern "C" int ibo_sgp_stage_ms(double *ms, int reset)
{
    return read_stage_sums(t_sgp_ms, IBO_SGP_STAGES, ms, reset);
}

// ------------------------------------------------------------------------ the marginal likelihood's gradient
// One private handle per device, kept between calls (a learning loop calls with another theta / noise / Z dozens of times) and given back
// by ibo_trim; the caller holds g_dev_mu.
static ibo_sgp *g_sgp_grad_handle[16];

void sgp_grad_trim(int device)
{
    ibo_sgp *&h = g_sgp_grad_handle[device & 15];
    if (h) { (void)ibo_sgp_destroy(h); h = nullptr; }
}

namespace {

struct SgpGradTotals { std::vector<double> Z[2], L[2]; double S[2]; double csum; };

// After a successful fit of h: the pass over the observations and the K~uu contraction.  tot: [0] the data's sums, [1] K~uu's.
int sgp_grad_pass(ibo_sgp *h, int kind, int64_t N, const double *X, const double *Y, SgpGradTotals *tot)
{
    ibo_gp *gu = h->gu, *ga = h->ga;
    hipStream_t su = gu->stream, sa = ga->stream;
    const int D = h->D, m = h->m, mp = h->mp, ldi = ga->Npad;
    if (gu->Npad != ldi || ldi < mp) return fail(IBO_ERR_STATE, "the two frames are padded to %d and %d rows for mp=%d", gu->Npad, ldi, mp);
    const bool two = kind != SGP_GRAD_DTC;                      // a DTC objective has e = 0: no K~uu^-1 half, no signed Gram matrix
    const int ldb = (two ? 2 : 1) * mp;
    SpanClock clock;
    IBO_TRY(clock.make(g_sgp_timing != 0));
    // the inverses: A^-1 = W_A^T W_A, K~uu^-1 = W_u^T W_u (ibo_nlml_grad's product)
    const size_t nn = (size_t)ldi * ldi;
    ScopedBuf<double> Ainv, Uinv, wt;
    IBO_TRY(Ainv.ensure(nn)); IBO_TRY(Uinv.ensure(nn)); IBO_TRY(wt.ensure(nn));
    HIP_TRY(hipStreamSynchronize(su));
    IBO_TRY(clock.start(sa));
    KERNEL_TRY(launch_wtw(ga->W.p, wt.p, Ainv.p, ldi, sa));
    KERNEL_TRY(launch_wtw(gu->W.p, wt.p, Uinv.p, ldi, sa));
    IBO_TRY(clock.stop(sa, &t_sgp_grad_ms[SGP_GR_INVERSES]));
    // the chunks: the fit's chunking, so that the U sweep gives the fit's q_i bit for bit
    const int64_t nc = moments_chunk_length(N, 8 * (int64_t)(mp + 64), g_sgp_chunk, (int64_t)256 << 20);
    const int64_t rows = class_padded(nc, nc), ldmax = (nc + 63) / 64 * 64, nblkmax = (ldmax + 255) / 256;
    const int rb = mp / 64;
    // a workgroup per 64 inducing rows and strip of tiles: about 1024 workgroups, the strips as even as the tiles allow
    const int nsmax = 1024 / rb < 1 ? 1 : 1024 / rb;
    auto strips_for = [&](int ntiles, int *tps) { const int ns = nsmax < ntiles ? nsmax : ntiles; *tps = (ntiles + ns - 1) / ns; return (ntiles + *tps - 1) / *tps; };
    ScopedBuf<double> xc, yc, ms, per, Bo, Kt, H, part, pc, totd;
    IBO_TRY(xc.ensure((size_t)rows * D)); IBO_TRY(yc.ensure((size_t)nc)); IBO_TRY(ms.ensure(3 * (size_t)rows));
    IBO_TRY(per.ensure(3 * (size_t)ldmax)); IBO_TRY(Bo.ensure((size_t)ldmax * ldb)); IBO_TRY(pc.ensure((size_t)nblkmax));
    if (two) { IBO_TRY(Kt.ensure(2 * (size_t)mp * ldmax)); IBO_TRY(H.ensure(3 * (size_t)mp * mp)); }
    const size_t pzn = (size_t)nsmax * mp * D, psn = (size_t)nsmax * rb;
    IBO_TRY(part.ensure(2 * pzn + psn));
    const size_t tn = (size_t)m * D;
    IBO_TRY(totd.ensure(2 * (2 * tn + 1)));
    HIP_TRY(hipMemsetAsync(totd.p, 0, sizeof(double) * 2 * (2 * tn + 1), sa));
    if (two) HIP_TRY(hipMemsetAsync(H.p, 0, sizeof(double) * (size_t)mp * mp, sa));
    IBO_TRY(sgp_pinned(h, (size_t)rows * D + (size_t)nc + (size_t)nblkmax));
    double *lam = per.p, *ev = per.p + ldmax, *rv = per.p + 2 * ldmax;
    double *partZ = part.p, *partL = part.p + pzn, *partS = part.p + 2 * pzn;
    // the strips a launch uses, no more: its workgroups add to their own rows of partZ / partL (every entry of partS is written)
    auto zero_partials = [&](int nstrips) -> int {
        HIP_TRY(hipMemsetAsync(partZ, 0, sizeof(double) * (size_t)nstrips * mp * D, sa));
        HIP_TRY(hipMemsetAsync(partL, 0, sizeof(double) * (size_t)nstrips * mp * D, sa));
        return IBO_OK;
    };
    SgpGradArgs g;
    memset(&g, 0, sizeof(g));
    g.kp = h->kp; g.m = m; g.mp = mp; g.Z = ga->Xp.p; g.ldz = ga->DP; g.Ainv = Ainv.p; g.Uinv = Uinv.p; g.ldi = ldi; g.two = two ? 1 : 0;
    g.Bo = Bo.p; g.ldb = ldb; g.alpha = ga->alphaY.p; g.rv = rv; g.partZ = partZ; g.partL = partL; g.partS = partS;
    tot->csum = 0.0;
    for (int64_t c0 = 0; c0 < N; c0 += nc) {
        const int64_t k = N - c0 < nc ? N - c0 : nc, kp = class_padded(k, nc), nblk = (k + 255) / 256;
        const int ld = (int)((k + 63) / 64 * 64);
        double *px = h->pin, *py = px + (size_t)rows * D, *pp = py + nc;
        memcpy(px, X + (size_t)c0 * D, sizeof(double) * (size_t)k * D);
        memset(px + (size_t)k * D, 0, sizeof(double) * (size_t)(kp - k) * D);
        memcpy(py, Y + c0, sizeof(double) * (size_t)k);
        HIP_TRY(hipMemcpyAsync(xc.p, px, sizeof(double) * (size_t)kp * D, hipMemcpyHostToDevice, su));
        HIP_TRY(hipMemcpyAsync(yc.p, py, sizeof(double) * (size_t)k, hipMemcpyHostToDevice, su));
        // the two frames' plain sweeps, as the candidate route runs them: q_i, mu_i, a_i
        SweepRequest r;
        r.M = kp; r.cand_dev = xc.p; r.acq = IBO_ACQ_NONE; r.clamp_lo = -1.0; r.s2_dev = ms.p;
        IBO_TRY(clock.start(su));
        IBO_TRY(run_sweep(gu, r));
        HIP_TRY(hipStreamSynchronize(su));
        r.mu_dev = ms.p + rows; r.s2_dev = ms.p + 2 * rows;
        IBO_TRY(run_sweep(ga, r));
        if (clock.on) { HIP_TRY(hipStreamSynchronize(sa)); IBO_TRY(clock.stop(su, &t_sgp_grad_ms[SGP_GR_SWEEPS])); }
        SgpGradObsArgs o;
        memset(&o, 0, sizeof(o));
        o.n = (int)k; o.ld = ld; o.kind = kind; o.noise = h->noise; o.jitter = h->jitter; o.s2u = ms.p; o.mua = ms.p + rows; o.s2a = ms.p + 2 * rows;
        o.Y = yc.p; o.lam = lam; o.ev = ev; o.rv = rv; o.part = pc.p;
        SgpGradGenArgs ge;
        memset(&ge, 0, sizeof(ge));
        ge.kp = h->kp; ge.m = m; ge.mp = mp; ge.Z = ga->Xp.p; ge.ldz = ga->DP; ge.X = xc.p; ge.n = (int)k; ge.ld = ld; ge.lam = lam; ge.ev = ev;
        ge.two = two ? 1 : 0; ge.Bo = Bo.p; ge.ldb = ldb; ge.Kt = two ? Kt.p : nullptr; ge.KEt = two ? Kt.p + (size_t)mp * ld : nullptr;
        IBO_TRY(clock.start(sa));
        KERNEL_TRY(launch_sgp_grad_obs(o, sa));
        KERNEL_TRY(launch_sgp_grad_gen(ge, sa));
        IBO_TRY(clock.stop(sa, &t_sgp_grad_ms[SGP_GR_GEN]));
        g.X = xc.p; g.ldx = D; g.n = (int)k; g.ntiles = ld / 64;
        g.nstrips = strips_for(g.ntiles, &g.tiles_per_strip);
        if (g.nstrips > nsmax) return fail(IBO_ERR_STATE, "%d strips, room for %d", g.nstrips, nsmax);
        IBO_TRY(zero_partials(g.nstrips));
        IBO_TRY(clock.start(sa));
        KERNEL_TRY(launch_sgp_grad_contract(g, 0, sa));
        IBO_TRY(clock.stop(sa, &t_sgp_grad_ms[SGP_GR_CONTRACT]));
        IBO_TRY(clock.start(sa));
        KERNEL_TRY(launch_sgp_grad_reduce(partZ, partL, partS, g.nstrips, m, mp, D, totd.p, totd.p + tn, totd.p + 2 * tn, sa));
        IBO_TRY(clock.stop(sa, &t_sgp_grad_ms[SGP_GR_REDUCE]));
        if (two) {                                               // H += (K E) K^T, the lower tiles, continued in ascending observation order
            IBO_TRY(clock.start(sa));
            KERNEL_TRY(launch_sgp_abt(ge.KEt, ld, ge.Kt, ld, H.p, mp, mp, ld, 1, 1, sa));
            IBO_TRY(clock.stop(sa, &t_sgp_grad_ms[SGP_GR_GRAM]));
        }
        HIP_TRY(hipMemcpyAsync(pp, pc.p, sizeof(double) * (size_t)nblk, hipMemcpyDeviceToHost, sa));
        HIP_TRY(hipStreamSynchronize(sa));
        for (int64_t b = 0; b < nblk; b++) tot->csum += pp[b];  // ascending blocks of 256
    }
    // S = dNL/dK~uu, then the same contraction with Z in the role of the observations
    IBO_TRY(clock.start(sa));
    double *Hm = H.p, *T = two ? H.p + (size_t)mp * mp : nullptr, *M = two ? H.p + 2 * (size_t)mp * mp : nullptr;
    if (two) {
        KERNEL_TRY(launch_sgp_mirror(Hm, mp, mp, sa));
        KERNEL_TRY(launch_sgp_abt(Uinv.p, ldi, Hm, mp, T, mp, mp, mp, 0, 0, sa));          // T = K~uu^-1 H     (H symmetric)
        KERNEL_TRY(launch_sgp_abt(T, mp, Uinv.p, ldi, M, mp, mp, mp, 0, 0, sa));           // M = T K~uu^-1     (K~uu^-1 symmetric)
    }
    ScopedBuf<double> Sbuf;
    IBO_TRY(Sbuf.ensure((size_t)mp * mp));
    double *S = Sbuf.p;
    KERNEL_TRY(launch_sgp_grad_S(Ainv.p, Uinv.p, ldi, ga->alphaY.p, M, mp, m, mp, S, sa));
    g.X = ga->Xp.p; g.ldx = ga->DP; g.n = m; g.ntiles = rb; g.S = S; g.lds = mp;
    g.nstrips = strips_for(g.ntiles, &g.tiles_per_strip);
    if (g.nstrips > nsmax) return fail(IBO_ERR_STATE, "%d strips, room for %d", g.nstrips, nsmax);
    IBO_TRY(zero_partials(g.nstrips));
    KERNEL_TRY(launch_sgp_grad_contract(g, 1, sa));
    double *t1 = totd.p + 2 * tn + 1;
    KERNEL_TRY(launch_sgp_grad_reduce(partZ, partL, partS, g.nstrips, m, mp, D, t1, t1 + tn, t1 + 2 * tn, sa));
    IBO_TRY(clock.stop(sa, &t_sgp_grad_ms[SGP_GR_UU]));
    std::vector<double> host(2 * (2 * tn + 1));
    HIP_TRY(hipMemcpyAsync(host.data(), totd.p, sizeof(double) * host.size(), hipMemcpyDeviceToHost, sa));
    HIP_TRY(hipStreamSynchronize(sa));
    for (int w = 0; w < 2; w++) {
        const double *p = host.data() + (size_t)w * (2 * tn + 1);
        tot->Z[w].assign(p, p + tn); tot->L[w].assign(p + tn, p + 2 * tn); tot->S[w] = p[2 * tn];
    }
    return IBO_OK;
}

}  // namespace

extern "C" int ibo_sgp_nlml_grad(int device, int ktype, int D, const double *hyper, int nhyper, double sf2, double noise, double jitter, int kind,
                                 int m, const double *Z, int64_t N, const double *X, const double *Y, int ngrad, const int *modes, const int *dims,
                                 double *value, double *grad_hyper, double *grad_lognoise, double *grad_Z, int *info)
{
    IBO_TRY(use_device(device));
    if (!hyper || !Z || !X || !Y || !value) return fail(IBO_ERR_ARG, "NULL argument");
    if (kind != IBO_SGP_FITC && kind != IBO_SGP_DTC && kind != IBO_SGP_VFE) return fail(IBO_ERR_ARG, "unknown kind %d", kind);
    if (ngrad < 0 || ngrad > IBO_GRAD_MAX) return fail(IBO_ERR_ARG, "ngrad=%d unsupported (0..%d)", ngrad, IBO_GRAD_MAX);
    if (ngrad > 0 && (!modes || !dims)) return fail(IBO_ERR_ARG, "modes / dims is NULL");
    for (int i = 0; i < ngrad; i++)
        if (modes[i] < 0 || modes[i] > 4 || dims[i] < 0 || dims[i] >= D) return fail(IBO_ERR_ARG, "bad derivative spec");
    std::lock_guard<std::mutex> lk(g_dev_mu[device & 15]);      // (the private handle is per device)
    ibo_sgp *&h = g_sgp_grad_handle[device & 15];
    if (!h) IBO_TRY(ibo_sgp_create(device, &h));
    SpanClock clock;
    IBO_TRY(clock.make(g_sgp_timing != 0));
    IBO_TRY(clock.start(h->ga->stream));
    IBO_TRY(ibo_sgp_fit(h, ktype, D, hyper, nhyper, sf2, noise, jitter, kind == IBO_SGP_VFE ? IBO_SGP_DTC : kind, m, Z, N, X, Y, nullptr, info));
    IBO_TRY(clock.stop(h->ga->stream, &t_sgp_grad_ms[SGP_GR_FIT]));
    double v = 0.0;
    IBO_TRY(ibo_sgp_nlml(h, kind == IBO_SGP_VFE ? IBO_SGP_NLML_VFE : IBO_SGP_NLML_MODEL, &v));
    const bool want_hyper = ngrad > 0 && grad_hyper;
    if (want_hyper || grad_lognoise || grad_Z) {
        SgpGradTotals tot;
        IBO_TRY(sgp_grad_pass(h, kind, N, X, Y, &tot));
        const KParams &kp = h->kp;
        // dNL/dlog l_d = -2 w_d (sum_a L[a][d]), the rows in ascending order, the data's sum and then K~uu's
        std::vector<double> Ld((size_t)D, 0.0);
        for (int d = 0; d < D; d++) {
            double s0 = 0.0, s1 = 0.0;
            for (int a = 0; a < m; a++) { s0 += tot.L[0][(size_t)a * D + d]; s1 += tot.L[1][(size_t)a * D + d]; }
            Ld[d] = -2.0 * kp.w[d] * (s0 + s1);
        }
        if (want_hyper)
            for (int i = 0; i < ngrad; i++) {
                if (modes[i] == 0) grad_hyper[i] = Ld[dims[i]];
                else if (modes[i] == 2) grad_hyper[i] = 2.0 * (tot.S[0] + tot.S[1]);
                else { double s = 0.0; for (int d = 0; d < D; d++) s += Ld[d]; grad_hyper[i] = s; }      // one length scale for every dimension
            }
        if (grad_lognoise) *grad_lognoise = noise * (tot.csum - (kind == IBO_SGP_VFE ? h->tt / (2.0 * noise * noise) : 0.0));
        if (grad_Z)
            for (int a = 0; a < m; a++)
                for (int d = 0; d < D; d++)
                    grad_Z[(size_t)a * D + d] = 2.0 * kp.w[d] * (tot.Z[0][(size_t)a * D + d] + 2.0 * tot.Z[1][(size_t)a * D + d]);
    }
    *value = v;
    return IBO_OK;
}

extern "C" int ibo_sgp_grad_stage_ms(double *ms, int reset)
{
    return read_stage_sums(t_sgp_grad_ms, IBO_SGP_GRAD_STAGES, ms, reset);
}

// abi_mes.hip -- max-value entropy search behind the C ABI: ibo_mes_sweep, ibo_mes_batch, ibo_mes_grad_batch, ibo_mes_direct_max, and
// ibo_mes_maxcdf, the max-value cdf over a candidate set (kernels: mes.hip; the per-model work: run_sweep).
#include "abi_eval.h"
#include "mes.h"

#include <algorithm>

std::atomic<int> g_mes_chunk{0};      // ibo_set_option("mes_chunk", m): candidates per chunk of the ibo_mes_* entries (rounded up to 256); 0: by bytes
std::atomic<int> g_mes_timing{0};     // ibo_set_option("mes_timing", 1): HIP events around every launch of the scan kernels, read with ibo_mes_scan_ms
static thread_local double t_mes_ms = 0.0;

static_assert(IBO_MES_MAX_K == IBO_MES_MAX_SAMPLES && IBO_MES_MAX_LEV == IBO_MES_MAX_LEVELS, "the kernels' LDS arrays hold what the ABI admits");

// the leading arguments of the four value entries, and the sorted samples made of them
struct MesCall {
    ibo_gp *g; double s2_offset, clamp_lo;
    int K; std::vector<double> ys;                           // ascending
    ScopedBuf<double> ys_dev;                                // the same on the device: uploaded once per call (mes_begin), whatever it evaluates
};

static int mes_offset_ok(double s2_offset)
{
    if (!(s2_offset >= 0.0) || std::isinf(s2_offset)) return fail(IBO_ERR_ARG, "s2_offset=%g", s2_offset);
    return IBO_OK;
}

// What the four entries check alike: what the samples alone decide (no device needed), the device, the arguments, the handle's state.
static int mes_begin(ibo_gp *gp, int K, const double *ystar_host, double s2_offset, int64_t M, const void *points, double clamp_lo, bool any_out,
                     MesCall *c)
{
    if (K < 1 || K > IBO_MES_MAX_SAMPLES) return fail(IBO_ERR_ARG, "K=%d samples of the maximum, not 1 .. %d", K, IBO_MES_MAX_SAMPLES);
    if (!ystar_host) return fail(IBO_ERR_ARG, "ystar_host is NULL");
    for (int k = 0; k < K; k++)
        if (!std::isfinite(ystar_host[k])) return fail(IBO_ERR_ARG, "sample %d of the maximum is not finite", k);
    IBO_TRY(mes_offset_ok(s2_offset));
    IBO_TRY(use_device(gp ? gp->device : 0));
    if (!gp) return fail(IBO_ERR_ARG, "gp is NULL");
    if (M < 1) return fail(IBO_ERR_ARG, "M=%lld", (long long)M);
    if (!points) return fail(IBO_ERR_ARG, "NULL argument");
    if (!any_out) return fail(IBO_ERR_ARG, "every output is NULL");
    if (!gp->fitted) return fail(IBO_ERR_STATE, "max-value entropy search before the fit");
    c->g = gp; c->s2_offset = s2_offset; c->clamp_lo = clamp_lo; c->K = K;
    c->ys.assign(ystar_host, ystar_host + K);
    std::sort(c->ys.begin(), c->ys.end());
    IBO_TRY(c->ys_dev.ensure((size_t)K));
    HIP_TRY(hipMemcpyAsync(c->ys_dev.p, c->ys.data(), sizeof(double) * K, hipMemcpyHostToDevice, gp->stream));
    HIP_TRY(hipStreamSynchronize(gp->stream));
    return IBO_OK;
}

// the candidates of one chunk as run_sweep takes them: the caller's rows where the padded launch fits into them, else a padded copy
static int mes_chunk_rows(ibo_gp *g, const double *cand_dev, int64_t cand_rows, int64_t c0, int64_t m, int64_t mp, ScopedBuf<double> *pad, const double **rows)
{
    const int D = g->D;
    *rows = cand_dev + c0 * D;
    if (c0 + mp <= cand_rows) return IBO_OK;
    IBO_TRY(pad->ensure((size_t)mp * D));
    HIP_TRY(hipMemcpyAsync(pad->p, *rows, sizeof(double) * (size_t)m * D, hipMemcpyDeviceToDevice, g->stream));
    HIP_TRY(hipMemsetAsync(pad->p + (size_t)m * D, 0, sizeof(double) * (size_t)(mp - m) * D, g->stream));
    *rows = pad->p;
    return IBO_OK;
}

// candidates per chunk (a multiple of the kernels' workgroup) and the scratch's stride: 16 bytes of (mu, s2) a candidate, at most 1 GiB
static void mes_chunking(int64_t M, int64_t *mc, int64_t *stride)
{
    *mc = (((int64_t)1 << 30) / 16) / 256 * 256;
    if (g_mes_chunk > 0) *mc = ((int64_t)g_mes_chunk + 255) / 256 * 256;
    if (M <= *mc) *mc = M;
    *stride = class_padded(*mc, *mc);                          // (every launch of the call fits: a tail is padded to at most mc's own size class)
}

// the diagnostic's events: made and destroyed per call
struct MesEvents {
    hipEvent_t e0 = nullptr, e1 = nullptr;
    ~MesEvents() { if (e0) (void)hipEventDestroy(e0); if (e1) (void)hipEventDestroy(e1); }
    int make() { HIP_TRY(hipEventCreate(&e0)); HIP_TRY(hipEventCreate(&e1)); return IBO_OK; }
    int stop(hipStream_t s)
    {
        float ms1 = 0.f;
        HIP_TRY(hipEventRecord(e1, s)); HIP_TRY(hipEventSynchronize(e1)); HIP_TRY(hipEventElapsedTime(&ms1, e0, e1));
        t_mes_ms += ms1;
        return IBO_OK;
    }
};

// What a call may ask of the device pass beside the arg-max: the values, and the gradient's sums (four arrays M apart)
struct MesOut { double *val_dev = nullptr, *sums_dev = nullptr; double *best_val = nullptr; int64_t *best_idx = nullptr; };

// The one route of every value entry: per chunk the plain sweep -- (mu, s2) into pooled scratch, no arg-max, no read-back -- then
// mes_finish_kernel, all on the model's stream.
// cand_rows: the rows cand_dev has room for (>= M; rows from M on are the caller's padding, see class_padded).
static int mes_device(const MesCall &c, int64_t M, const double *cand_dev, int64_t cand_rows, int n_excl, const double *excl_host,
                      double excl_radius, int64_t index_base, const MesOut &o)
{
    ibo_gp *g = c.g;
    hipStream_t s = g->stream;
    MesArgs a;
    memset(&a, 0, sizeof(a));
    a.K = c.K; a.ystar = c.ys_dev.p; a.s2_offset = c.s2_offset; a.clamp_lo = c.clamp_lo;
    a.D = g->D; a.index_base = index_base; a.excl_radius = excl_radius;
    IBO_TRY(upload_exclusions(g, n_excl, excl_host, &a.n_excl, &a.excl));
    int64_t mc, stride;
    mes_chunking(M, &mc, &stride);
    const int64_t nblk = (M + 255) / 256;
    ScopedBuf<double> ms, pv, pad;
    ScopedBuf<int64_t> pi;
    IBO_TRY(ms.ensure(2 * (size_t)stride));
    IBO_TRY(pv.ensure((size_t)nblk)); IBO_TRY(pi.ensure((size_t)nblk));
    const bool timing = g_mes_timing != 0;
    MesEvents ev;
    if (timing) IBO_TRY(ev.make());
    a.ms = ms.p; a.stride = stride; a.sums_stride = M;
    for (int64_t c0 = 0; c0 < M; c0 += mc) {
        const int64_t m = M - c0 < mc ? M - c0 : mc, mp = class_padded(m, mc);
        SweepRequest r;
        r.M = mp; r.acq = IBO_ACQ_NONE; r.clamp_lo = c.clamp_lo;
        IBO_TRY(mes_chunk_rows(g, cand_dev, cand_rows, c0, m, mp, &pad, &r.cand_dev));
        r.mu_dev = ms.p; r.s2_dev = ms.p + stride;
        IBO_TRY(run_sweep(g, r));
        a.M = m; a.first = c0; a.cand = r.cand_dev;
        a.out_val = o.val_dev ? o.val_dev + c0 : nullptr;
        a.out_sums = o.sums_dev ? o.sums_dev + c0 : nullptr;
        a.part_val = pv.p + c0 / 256; a.part_idx = pi.p + c0 / 256;
        if (timing) HIP_TRY(hipEventRecord(ev.e0, s));
        KERNEL_TRY(launch_mes_finish(a, o.sums_dev != nullptr, s));
        if (timing) IBO_TRY(ev.stop(s));
    }
    if (o.best_val || o.best_idx) return argmax_readback(g, pv.p, pi.p, nblk, o.best_val, o.best_idx);
    HIP_TRY(hipStreamSynchronize(s));
    return IBO_OK;
}

extern "C" int ibo_mes_sweep(ibo_gp_t *gp, int K, const double *ystar_host, double s2_offset, int64_t M, const double *cand_dev, double clamp_lo,
                             int n_excl, const double *excl_host, double excl_radius, int64_t index_base,
                             double *val_dev, double *best_val, int64_t *best_idx)
{
    MesCall c;
    IBO_TRY(mes_begin(gp, K, ystar_host, s2_offset, M, cand_dev, clamp_lo, val_dev || best_val || best_idx, &c));
    MesOut o;
    o.val_dev = val_dev; o.best_val = best_val; o.best_idx = best_idx;
    return mes_device(c, M, cand_dev, M, n_excl, excl_host, excl_radius, index_base, o);
}

// Host points: uploaded, then the sweep's own sweep and kernel -- the device's values are the sweep's bits.
// val: M; sums (the gradient's): 4 M, see MesArgs.
static int mes_eval_host(const MesCall &c, int64_t M, const double *Q_host, double *val, double *sums)
{
    const size_t m = (size_t)M;
    hipStream_t s = c.g->stream;
    const size_t rows = (size_t)class_padded(M, M), D = (size_t)c.g->D;        // (a short batch carries its padding: no copy on the device)
    ScopedBuf<double> q, out;
    IBO_TRY(q.ensure(rows * D)); IBO_TRY(out.ensure(m * (sums ? 5 : 1)));
    HIP_TRY(hipMemcpyAsync(q.p, Q_host, sizeof(double) * m * D, hipMemcpyHostToDevice, s));
    if (rows > m) HIP_TRY(hipMemsetAsync(q.p + m * D, 0, sizeof(double) * (rows - m) * D, s));
    MesOut o;
    o.val_dev = out.p; o.sums_dev = sums ? out.p + m : nullptr;
    IBO_TRY(mes_device(c, M, q.p, (int64_t)rows, 0, nullptr, 0.0, 0, o));
    if (val) HIP_TRY(hipMemcpyAsync(val, out.p, sizeof(double) * m, hipMemcpyDeviceToHost, s));
    if (sums) HIP_TRY(hipMemcpyAsync(sums, out.p + m, sizeof(double) * 4 * m, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return IBO_OK;
}

extern "C" int ibo_mes_batch(ibo_gp_t *gp, int K, const double *ystar_host, double s2_offset, int64_t M, const double *Q_host, double clamp_lo,
                             double *val_host)
{
    MesCall c;
    IBO_TRY(mes_begin(gp, K, ystar_host, s2_offset, M, Q_host, clamp_lo, val_host != nullptr, &c));
    return mes_eval_host(c, M, Q_host, val_host, nullptr);
}

// grad MES = G_mu grad mu + G_sigma grad s2 / (2 sigma): the sums from the kernel's second variant, the posterior's gradients from
// ibo_acq_grad_batch (ds2 is 0 where the sweep's clip is active; where the floor of v is, the kernel's flag is 0).
extern "C" int ibo_mes_grad_batch(ibo_gp_t *gp, int K, const double *ystar_host, double s2_offset, int64_t M, const double *Q_host, double clamp_lo,
                                  double *val_host, double *grad_host)
{
    MesCall c;
    IBO_TRY(mes_begin(gp, K, ystar_host, s2_offset, M, Q_host, clamp_lo, val_host || grad_host, &c));
    if (!grad_host) return mes_eval_host(c, M, Q_host, val_host, nullptr);
    const size_t m = (size_t)M, D = (size_t)c.g->D;
    std::vector<double> sums(4 * m), dmu(m * D), ds2(m * D);
    IBO_TRY(mes_eval_host(c, M, Q_host, val_host, sums.data()));
    IBO_TRY(ibo_acq_grad_batch(c.g, M, Q_host, IBO_ACQ_NONE, 0.0, IBO_ERF_LIBM, clamp_lo, NAN, nullptr, nullptr, nullptr, dmu.data(), ds2.data(), nullptr));
    const double *gm = sums.data(), *gs = gm + m, *sig = gm + 2 * m, *follows = gm + 3 * m;
    for (size_t i = 0; i < m; i++)
        for (size_t d = 0; d < D; d++)
            grad_host[i * D + d] = gm[i] * dmu[i * D + d] + gs[i] * ((follows[i] != 0.0 ? ds2[i * D + d] : 0.0) / (2.0 * sig[i]));
    return IBO_OK;
}

// direct_maximize on the handle: the same driver, every batch through mes_eval_host
extern "C" int ibo_mes_direct_max(ibo_gp_t *gp, int K, const double *ystar_host, double s2_offset, int D, const double *lb, const double *ub,
                                  double clamp_lo, int maxiter, int maxtime, int maxsample, int compat, double *opt, double *optx, int64_t *nsamples)
{
    MesCall c;
    IBO_TRY(mes_begin(gp, K, ystar_host, s2_offset, 1, (lb && ub) ? lb : nullptr, clamp_lo, opt || optx || nsamples, &c));
    if (D != c.g->D) return fail(IBO_ERR_ARG, "bounds have %d dimensions, the model has %d", D, c.g->D);
    const ibo::batch_eval_t value = [&](const double *pts, int n, double *vals) -> int { return mes_eval_host(c, n, pts, vals, nullptr); };
    char label[64];
    snprintf(label, sizeof(label), "max-value entropy DIRECT (%d samples)", c.K);
    return direct_maximize(value, label, D, lb, ub, maxiter, maxtime, maxsample, compat, opt, optx, nsamples);
}

// Per chunk the plain sweep and mes_maxcdf_kernel's block partials; then one launch adds all of them in block order.
extern "C" int ibo_mes_maxcdf(ibo_gp_t *gp, int64_t M, const double *cand_dev, int nlev, const double *lev_host, double s2_offset, double clamp_lo,
                              double *logcdf_host, double *stats_host)
{
    if (nlev < 0 || nlev > IBO_MES_MAX_LEVELS) return fail(IBO_ERR_ARG, "nlev=%d levels, not 0 .. %d", nlev, IBO_MES_MAX_LEVELS);
    if (nlev > 0 && (!lev_host || !logcdf_host)) return fail(IBO_ERR_ARG, "NULL argument");
    for (int k = 0; k < nlev; k++)
        if (lev_host[k] != lev_host[k]) return fail(IBO_ERR_ARG, "level %d is a NaN", k);
    IBO_TRY(mes_offset_ok(s2_offset));
    IBO_TRY(use_device(gp ? gp->device : 0));
    if (!gp) return fail(IBO_ERR_ARG, "gp is NULL");
    if (M < 1) return fail(IBO_ERR_ARG, "M=%lld", (long long)M);
    if (!cand_dev || !stats_host) return fail(IBO_ERR_ARG, "NULL argument");
    if (!gp->fitted) return fail(IBO_ERR_STATE, "max-value cdf before the fit");
    ibo_gp *g = gp;
    hipStream_t s = g->stream;
    int64_t mc, stride;
    mes_chunking(M, &mc, &stride);
    const int64_t nblk = (M + 255) / 256;
    ScopedBuf<double> ms, part, pad, io;
    IBO_TRY(ms.ensure(2 * (size_t)stride));
    IBO_TRY(part.ensure((size_t)nblk * (nlev + 2)));           // the block sums (nblk x nlev), then the two block maxima
    IBO_TRY(io.ensure(2 * (size_t)nlev + 2));                   // the levels, then the results
    MesCdfArgs a;
    memset(&a, 0, sizeof(a));
    a.nlev = nlev; a.lev = io.p; a.s2_offset = s2_offset; a.clamp_lo = clamp_lo; a.ms = ms.p; a.stride = stride;
    double *pmu = part.p + (size_t)nblk * nlev, *pub = pmu + nblk, *res = io.p + nlev;
    if (nlev > 0) HIP_TRY(hipMemcpyAsync(io.p, lev_host, sizeof(double) * nlev, hipMemcpyHostToDevice, s));
    HIP_TRY(hipStreamSynchronize(s));                          // (lev_host is the caller's pageable memory)
    const bool timing = g_mes_timing != 0;
    MesEvents ev;
    if (timing) IBO_TRY(ev.make());
    for (int64_t c0 = 0; c0 < M; c0 += mc) {
        const int64_t m = M - c0 < mc ? M - c0 : mc, mp = class_padded(m, mc);
        SweepRequest r;
        r.M = mp; r.acq = IBO_ACQ_NONE; r.clamp_lo = clamp_lo;
        IBO_TRY(mes_chunk_rows(g, cand_dev, M, c0, m, mp, &pad, &r.cand_dev));
        r.mu_dev = ms.p; r.s2_dev = ms.p + stride;
        IBO_TRY(run_sweep(g, r));
        a.M = m;
        a.part_sum = part.p + (size_t)(c0 / 256) * nlev; a.part_mu = pmu + c0 / 256; a.part_ub = pub + c0 / 256;
        if (timing) HIP_TRY(hipEventRecord(ev.e0, s));
        KERNEL_TRY(launch_mes_maxcdf(a, s));
        if (timing) IBO_TRY(ev.stop(s));
    }
    KERNEL_TRY(launch_mes_maxcdf_final(part.p, pmu, pub, nblk, nlev, res, s));
    if (nlev > 0) HIP_TRY(hipMemcpyAsync(logcdf_host, res, sizeof(double) * nlev, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(stats_host, res + nlev, sizeof(double) * 2, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return IBO_OK;
}

extern "C" int ibo_mes_scan_ms(double *ms, int reset)
{
    if (ms) *ms = t_mes_ms;
    if (reset) t_mes_ms = 0.0;
    return IBO_OK;
}

// abi_mes.hip -- max-value entropy search behind the C ABI: ibo_mes_sweep, ibo_mes_batch, ibo_mes_grad_batch, ibo_mes_direct_max, and
// ibo_mes_maxcdf, the max-value cdf over a candidate set (kernels: mes.hip; the chunks and the per-model work: abi_moments.h).
#include "abi_moments.h"
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

// What a call may ask of the device pass beside the arg-max (MomentsPipeline::out): the values, and the gradient's sums (four arrays M apart)
enum { MES_OUT_VAL = 0, MES_OUT_SUMS };

// The one route of every value entry: one slot, so every launch is on the model's stream -- per chunk the plain sweep, then mes_finish_kernel.
static void mes_pipeline(const MesCall &c, int64_t M, MomentsPipeline *p)
{
    p->add(c.g, true, true, c.clamp_lo, IBO_ERF_LIBM);
    p->home = c.g; p->chunk_opt = g_mes_chunk; p->timing = g_mes_timing != 0; p->finish_ms = &t_mes_ms;
    p->finish = [&c, p, M](const MomentChunk &k, hipStream_t s) -> int {
        MesArgs a;
        memset(&a, 0, sizeof(a));
        a.K = c.K; a.ystar = c.ys_dev.p; a.s2_offset = c.s2_offset; a.clamp_lo = c.clamp_lo;
        a.t = k.tail; a.ms = k.ms; a.stride = k.stride; a.sums_stride = M;
        a.out_val = k.at(p->out[MES_OUT_VAL]); a.out_sums = k.at(p->out[MES_OUT_SUMS]);
        KERNEL_TRY(launch_mes_finish(a, a.out_sums != nullptr, s));
        return IBO_OK;
    };
}

extern "C" int ibo_mes_sweep(ibo_gp_t *gp, int K, const double *ystar_host, double s2_offset, int64_t M, const double *cand_dev, double clamp_lo,
                             int n_excl, const double *excl_host, double excl_radius, int64_t index_base,
                             double *val_dev, double *best_val, int64_t *best_idx)
{
    MesCall c;
    IBO_TRY(mes_begin(gp, K, ystar_host, s2_offset, M, cand_dev, clamp_lo, val_dev || best_val || best_idx, &c));
    MomentsPipeline p;
    mes_pipeline(c, M, &p);
    p.out[MES_OUT_VAL] = val_dev;
    return p.sweep(M, cand_dev, M, n_excl, excl_host, excl_radius, index_base, best_val, best_idx);
}

// Host points through the sweep's own route.  val: M; sums (the gradient's): 4 M, see MesArgs.
static int mes_eval_host(const MesCall &c, int64_t M, const double *Q_host, double *val, double *sums)
{
    MomentsPipeline p;
    mes_pipeline(c, M, &p);
    double *const host[2] = {val, sums};
    const size_t len[2] = {(size_t)M, 4 * (size_t)M};
    return p.eval_host(M, Q_host, sums ? 2 : 1, host, len);
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

// The pipeline's chunks with mes_maxcdf_kernel's block partials as their finish; then one launch adds all of them in block order.
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
    hipStream_t s = gp->stream;
    MomentsPipeline p;
    p.add(gp, true, true, clamp_lo, IBO_ERF_LIBM);
    p.home = gp; p.chunk_opt = g_mes_chunk; p.timing = g_mes_timing != 0; p.finish_ms = &t_mes_ms;
    IBO_TRY(p.begin(M));
    const int64_t nblk = (M + 255) / 256;
    ScopedBuf<double> part, io;
    IBO_TRY(part.ensure((size_t)nblk * (nlev + 2)));           // the block sums (nblk x nlev), then the two block maxima
    IBO_TRY(io.ensure(2 * (size_t)nlev + 2));                   // the levels, then the results
    double *pmu = part.p + (size_t)nblk * nlev, *pub = pmu + nblk, *res = io.p + nlev;
    if (nlev > 0) HIP_TRY(hipMemcpyAsync(io.p, lev_host, sizeof(double) * nlev, hipMemcpyHostToDevice, s));
    HIP_TRY(hipStreamSynchronize(s));                          // (lev_host is the caller's pageable memory)
    p.finish = [&](const MomentChunk &k, hipStream_t st) -> int {
        MesCdfArgs a;
        memset(&a, 0, sizeof(a));
        a.nlev = nlev; a.lev = io.p; a.s2_offset = s2_offset; a.clamp_lo = clamp_lo; a.ms = k.ms; a.stride = k.stride; a.M = k.m;
        a.part_sum = part.p + (size_t)(k.c0 / 256) * nlev; a.part_mu = pmu + k.c0 / 256; a.part_ub = pub + k.c0 / 256;
        KERNEL_TRY(launch_mes_maxcdf(a, st));
        return IBO_OK;
    };
    FinishTail none;                                           // (no exclusions, no arg-max: the block sums are this entry's partials)
    memset(&none, 0, sizeof(none));
    IBO_TRY(p.chunks(M, cand_dev, M, none, nullptr, nullptr));
    KERNEL_TRY(launch_mes_maxcdf_final(part.p, pmu, pub, nblk, nlev, res, s));
    if (nlev > 0) HIP_TRY(hipMemcpyAsync(logcdf_host, res, sizeof(double) * nlev, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(stats_host, res + nlev, sizeof(double) * 2, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return IBO_OK;
}

extern "C" int ibo_mes_scan_ms(double *ms, int reset)
{
    return read_stage_sums(&t_mes_ms, 1, ms, reset);
}

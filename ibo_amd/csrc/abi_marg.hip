// abi_marg.hip -- acquisitions integrated over an ensemble of models behind the C ABI (include/ibo_abi_ensemble.h): sum_s w_s acq_s over
// S handles -- ibo_iacq_sweep, ibo_iacq_batch, ibo_iacq_grad_batch, ibo_iacq_direct_max, ibo_iacq_stage_ms (kernel: marg.hip; the chunks
// and the per-member sweeps: abi_moments.h).
#include "abi_moments.h"
#include "marg.h"
#include "../../include/ibo_abi_ensemble.h"

std::atomic<int> g_iacq_chunk{0};     // ibo_set_option("iacq_chunk", m): candidates per chunk of the ibo_iacq_* entries (rounded up to 256); 0: by bytes
std::atomic<int> g_iacq_timing{0};    // ibo_set_option("iacq_timing", 1): HIP events around every chunk's sweeps and its finish, read with ibo_iacq_stage_ms
static thread_local double t_iacq_ms[2] = {0.0, 0.0};        // sweeps, finish

static_assert(IBO_MARG_MAX == IBO_IACQ_MAX, "the kernel's weight array holds every member the ABI admits");
static_assert(MOMENT_SLOTS >= IBO_IACQ_MAX, "the pipeline has a slot per member");

// the leading arguments of the four computing entries
struct IacqCall {
    ibo_gp *const *gp; int S; const double *w;
    int acq; double parm; int erf_mode; double clamp_lo, ymax;
};

// What the four entries check alike, in cacq_begin's order: the device first, then the arguments, then the handles' state -- and their
// dimensionality last, which only a fitted handle has.  points: the entry's candidate / query array; any_out: whether it was given an
// output at all.  Fills the kernel's view of the request but the chunk (ymax NaN: member 0's largest observation).
static int iacq_begin(const IacqCall &c, int64_t M, const void *points, bool any_out, MargArgs *a)
{
    ibo_gp *first = (c.gp && c.S >= 1) ? c.gp[0] : nullptr;
    IBO_TRY(use_device(first ? first->device : 0));
    if (c.S < 1 || c.S > IBO_IACQ_MAX) return fail(IBO_ERR_ARG, "S=%d members outside [1, %d]", c.S, IBO_IACQ_MAX);
    if (!c.gp || !c.w) return fail(IBO_ERR_ARG, "NULL ensemble argument");
    double sum = 0.0;
    for (int s = 0; s < c.S; s++) {
        if (!c.gp[s]) return fail(IBO_ERR_ARG, "member handle %d is NULL", s);
        if (!(c.w[s] >= 0.0) || !(c.w[s] < HUGE_VAL)) return fail(IBO_ERR_ARG, "w[%d]=%g is not a finite weight >= 0", s, c.w[s]);
        if (c.gp[s]->device != first->device)
            return fail(IBO_ERR_ARG, "member %d lives on device %d, member 0 on device %d", s, c.gp[s]->device, first->device);
        sum += c.w[s];
    }
    if (!(sum > 0.0)) return fail(IBO_ERR_ARG, "every weight is 0");
    if (M < 1) return fail(IBO_ERR_ARG, "M=%lld", (long long)M);
    if (!points) return fail(IBO_ERR_ARG, "NULL argument");
    if (c.acq != IBO_ACQ_EI && c.acq != IBO_ACQ_PI && c.acq != IBO_ACQ_UCB && c.acq != IBO_ACQ_NONE)
        return fail(IBO_ERR_ARG, "unknown acquisition %d", c.acq);
    if (c.erf_mode != IBO_ERF_LIBM && c.erf_mode != IBO_ERF_NR) return fail(IBO_ERR_ARG, "unknown erf mode %d", c.erf_mode);
    if (!any_out) return fail(IBO_ERR_ARG, "every output is NULL");
    for (int s = 0; s < c.S; s++)
        if (!c.gp[s]->fitted) return fail(IBO_ERR_STATE, "integrated acquisition before member %d's fit", s);
    for (int s = 0; s < c.S; s++)
        if (c.gp[s]->D != first->D) return fail(IBO_ERR_ARG, "member %d has %d dimensions, member 0 %d", s, c.gp[s]->D, first->D);
    memset(a, 0, sizeof(*a));
    a->S = c.S; a->acq = c.acq; a->erf_mode = c.erf_mode; a->parm = c.parm;
    a->ymax = (c.ymax == c.ymax) ? c.ymax : first->maxY;
    for (int s = 0; s < c.S; s++) a->w[s] = c.w[s];
    return IBO_OK;
}

// What a call may ask of the device pass beside the arg-max (MomentsPipeline::out)
enum { IACQ_OUT_VAL = 0, IACQ_OUT_MEAN, IACQ_OUT_VAR };

// The one route of every value entry: one plain sweep per member with a weight, one after the other on the member's stream (a handle may
// appear more than once; a member whose weight is 0 keeps its places in the scratch and is not swept), then marg_finish_kernel on member
// 0's stream -- the stream rule is the pipeline's (abi_moments.hip).  Every launch is padded to its size class.
static void iacq_pipeline(const IacqCall &c, const MargArgs &spec, MomentsPipeline *p)
{
    for (int s = 0; s < c.S; s++) p->add(c.gp[s], true, true, c.clamp_lo, c.erf_mode, c.w[s] != 0.0);
    p->home = c.gp[0]; p->padded = true; p->chunk_opt = g_iacq_chunk;
    p->timing = g_iacq_timing != 0;
    if (p->timing) { p->sweeps_ms = &t_iacq_ms[0]; p->finish_ms = &t_iacq_ms[1]; }
    p->finish = [spec, p](const MomentChunk &k, hipStream_t s) -> int {
        MargArgs a = spec;
        a.t = k.tail; a.ms = k.ms; a.stride = k.stride;
        a.out_val = k.at(p->out[IACQ_OUT_VAL]); a.out_mean = k.at(p->out[IACQ_OUT_MEAN]); a.out_var = k.at(p->out[IACQ_OUT_VAR]);
        KERNEL_TRY(launch_marg_finish(a, s));
        return IBO_OK;
    };
}

extern "C" int ibo_iacq_sweep(ibo_gp_t *const *gp, int S, const double *w, int64_t M, const double *cand_dev,
                              int acq, double parm, int erf_mode, double clamp_lo, double ymax,
                              int n_excl, const double *excl_host, double excl_radius, int64_t index_base,
                              double *val_dev, double *mean_dev, double *var_dev, double *best_val, int64_t *best_idx)
{
    const IacqCall c = {gp, S, w, acq, parm, erf_mode, clamp_lo, ymax};
    MargArgs spec;
    IBO_TRY(iacq_begin(c, M, cand_dev, val_dev || mean_dev || var_dev || best_val || best_idx, &spec));
    MomentsPipeline p;
    iacq_pipeline(c, spec, &p);
    p.out[IACQ_OUT_VAL] = val_dev; p.out[IACQ_OUT_MEAN] = mean_dev; p.out[IACQ_OUT_VAR] = var_dev;
    return p.sweep(M, cand_dev, M, n_excl, excl_host, excl_radius, index_base, best_val, best_idx);
}

// Host points through the sweep's own route.  val, mean, var: M each, any may be NULL.
static int iacq_eval_host(const IacqCall &c, const MargArgs &spec, int64_t M, const double *Q_host, double *val, double *mean, double *var)
{
    MomentsPipeline p;
    iacq_pipeline(c, spec, &p);
    double *const host[3] = {val, mean, var};
    const size_t len[3] = {(size_t)M, (size_t)M, (size_t)M};
    return p.eval_host(M, Q_host, 3, host, len);
}

extern "C" int ibo_iacq_batch(ibo_gp_t *const *gp, int S, const double *w, int64_t M, const double *Q_host,
                              int acq, double parm, int erf_mode, double clamp_lo, double ymax,
                              double *val_host, double *mean_host, double *var_host)
{
    const IacqCall c = {gp, S, w, acq, parm, erf_mode, clamp_lo, ymax};
    MargArgs spec;
    IBO_TRY(iacq_begin(c, M, Q_host, val_host || mean_host || var_host, &spec));
    return iacq_eval_host(c, spec, M, Q_host, val_host, mean_host, var_host);
}

// dval = sum_s w_s dacq_s, composed on the host from ibo_acq_grad_batch per member (its dacq; under IBO_ACQ_NONE its dmu) in ascending s,
// products and sums rounded separately; a member whose weight is 0 is not asked.  The value is the host batch's.
extern "C" int ibo_iacq_grad_batch(ibo_gp_t *const *gp, int S, const double *w, int64_t M, const double *Q_host,
                                   int acq, double parm, int erf_mode, double clamp_lo, double ymax,
                                   double *val_host, double *dval_host)
{
#pragma clang fp contract(off)
    const IacqCall c = {gp, S, w, acq, parm, erf_mode, clamp_lo, ymax};
    MargArgs spec;
    IBO_TRY(iacq_begin(c, M, Q_host, val_host || dval_host, &spec));
    if (val_host) IBO_TRY(iacq_eval_host(c, spec, M, Q_host, val_host, nullptr, nullptr));
    if (!dval_host) return IBO_OK;
    const size_t n = (size_t)M * (size_t)gp[0]->D;
    std::vector<double> g(n), sum(n, -0.0);
    for (int s = 0; s < S; s++) {
        if (w[s] == 0.0) continue;
        const bool none = acq == IBO_ACQ_NONE;
        IBO_TRY(ibo_acq_grad_batch(gp[s], M, Q_host, acq, parm, erf_mode, clamp_lo, spec.ymax, nullptr, nullptr, nullptr,
                                   none ? g.data() : nullptr, nullptr, none ? nullptr : g.data()));
        for (size_t i = 0; i < n; i++) sum[i] += w[s] * g[i];
    }
    memcpy(dval_host, sum.data(), sizeof(double) * n);
    return IBO_OK;
}

// direct_maximize over all the members: the same driver, every batch through iacq_eval_host
extern "C" int ibo_iacq_direct_max(ibo_gp_t *const *gp, int S, const double *w, int D, const double *lb, const double *ub,
                                   int acq, double parm, int erf_mode, double clamp_lo, double ymax,
                                   int maxiter, int maxtime, int maxsample, int compat, double *opt, double *optx, int64_t *nsamples)
{
    const IacqCall c = {gp, S, w, acq, parm, erf_mode, clamp_lo, ymax};
    MargArgs spec;
    IBO_TRY(iacq_begin(c, 1, (lb && ub) ? lb : nullptr, opt || optx || nsamples, &spec));
    if (D != gp[0]->D) return fail(IBO_ERR_ARG, "bounds have %d dimensions, the models have %d", D, gp[0]->D);
    const ibo::batch_eval_t value = [&](const double *pts, int n, double *vals) -> int {
        return iacq_eval_host(c, spec, n, pts, vals, nullptr, nullptr);
    };
    char label[64];
    snprintf(label, sizeof(label), "integrated DIRECT (%d members)", S);
    return direct_maximize(value, label, D, lb, ub, maxiter, maxtime, maxsample, compat, opt, optx, nsamples);
}

extern "C" int ibo_iacq_stage_ms(double *ms, int reset)
{
    return read_stage_sums(t_iacq_ms, 2, ms, reset);
}

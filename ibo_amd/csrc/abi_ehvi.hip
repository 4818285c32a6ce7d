// abi_ehvi.hip -- the two-objective expected hypervolume improvement behind the C ABI: ibo_ehvi_sweep, ibo_ehvi_batch, ibo_ehvi_grad_batch,
// ibo_ehvi_direct_max (kernel: ehvi.hip; the chunks and the per-model work: abi_moments.h; the front's canonical form: ehvi_front.h).
#include "abi_moments.h"
#include "ehvi.h"
#include "ehvi_front.h"

std::atomic<int> g_ehvi_chunk{0};     // ibo_set_option("ehvi_chunk", m): candidates per chunk of the ibo_ehvi_* entries (rounded up to 256); 0: by bytes
std::atomic<int> g_ehvi_timing{0};    // ibo_set_option("ehvi_timing", 1): HIP events around every launch of the scan kernel, read with ibo_ehvi_scan_ms
static thread_local double t_ehvi_ms = 0.0;

static_assert(IBO_EHVI_MAX_PAIRS == IBO_EHVI_MAX_FRONT, "the kernel's LDS array holds every front the ABI admits");

// the leading arguments of the four ibo_ehvi_* entries, and the canonical front made of them
struct EhviCall {
    ibo_gp *g1, *g2; int erf_mode; double clamp_lo;
    double r1, r2; int n; std::vector<double> pairs;         // n interleaved (a_i, b_i)
    ScopedBuf<double> front_dev;                             // the pairs on the device: uploaded once per call (ehvi_begin), whatever it evaluates
};

// What the four entries check alike, in cacq_begin's order: the device, the arguments, the handles' state, their dimensionality.
static int ehvi_begin(ibo_gp_t *const *obj, int nfront, const double *front_host, const double *ref, int64_t M, const void *points,
                      int erf_mode, double clamp_lo, bool any_out, EhviCall *c)
{
    IBO_TRY(use_device(obj && obj[0] ? obj[0]->device : 0));
    if (!obj || !obj[0] || !obj[1]) return fail(IBO_ERR_ARG, "an objective handle is NULL");
    if (obj[0]->device != obj[1]->device)
        return fail(IBO_ERR_ARG, "objective 1 lives on device %d, objective 0 on device %d", obj[1]->device, obj[0]->device);
    if (nfront < 0) return fail(IBO_ERR_ARG, "nfront=%d", nfront);
    if (nfront > 0 && !front_host) return fail(IBO_ERR_ARG, "front_host is NULL");
    if (!ref) return fail(IBO_ERR_ARG, "ref is NULL");
    if (M < 1) return fail(IBO_ERR_ARG, "M=%lld", (long long)M);
    if (!points) return fail(IBO_ERR_ARG, "NULL argument");
    if (erf_mode != IBO_ERF_LIBM && erf_mode != IBO_ERF_NR) return fail(IBO_ERR_ARG, "unknown erf mode %d", erf_mode);
    if (!any_out) return fail(IBO_ERR_ARG, "every output is NULL");
    long long where = 0;
    switch (ehvi_canonical_front(nfront, front_host, ref, IBO_EHVI_MAX_FRONT, &c->pairs, &where)) {
    case IBO_EHVI_FRONT_BAD_REF: return fail(IBO_ERR_ARG, "ref=(%g, %g) is not finite", ref[0], ref[1]);
    case IBO_EHVI_FRONT_BAD_POINT: return fail(IBO_ERR_ARG, "front point %lld is not finite", where);
    case IBO_EHVI_FRONT_TOO_MANY: return fail(IBO_ERR_ARG, "%lld front points are left after the dominated ones went, more than %d", where, IBO_EHVI_MAX_FRONT);
    default: break;
    }
    if (!obj[0]->fitted || !obj[1]->fitted) return fail(IBO_ERR_STATE, "hypervolume improvement before objective %d's fit", obj[0]->fitted ? 1 : 0);
    if (obj[0]->D != obj[1]->D) return fail(IBO_ERR_ARG, "objective 1 has %d dimensions, objective 0 %d", obj[1]->D, obj[0]->D);
    c->g1 = obj[0]; c->g2 = obj[1]; c->erf_mode = erf_mode; c->clamp_lo = clamp_lo;
    c->r1 = ref[0]; c->r2 = ref[1]; c->n = (int)(c->pairs.size() / 2);
    if (c->n > 0) {
        IBO_TRY(c->front_dev.ensure(2 * (size_t)c->n));
        HIP_TRY(hipMemcpyAsync(c->front_dev.p, c->pairs.data(), sizeof(double) * 2 * c->n, hipMemcpyHostToDevice, c->g1->stream));
        HIP_TRY(hipStreamSynchronize(c->g1->stream));
    }
    return IBO_OK;
}

// What a call may ask of the device pass beside the arg-max (MomentsPipeline::out): the values, and the gradient's sums (six arrays M apart)
enum { EHVI_OUT_VAL = 0, EHVI_OUT_SUMS };

// The one route of every entry: per chunk the two plain sweeps, 32 bytes of scratch per candidate (the same handle may be both), then
// ehvi_finish_kernel on the first model's stream.
static void ehvi_pipeline(const EhviCall &c, int64_t M, MomentsPipeline *p)
{
    p->add(c.g1, true, true, c.clamp_lo, c.erf_mode);
    p->add(c.g2, true, true, c.clamp_lo, c.erf_mode);
    p->home = c.g1; p->chunk_opt = g_ehvi_chunk; p->timing = g_ehvi_timing != 0; p->finish_ms = &t_ehvi_ms;
    p->finish = [&c, p, M](const MomentChunk &k, hipStream_t s) -> int {
        EhviArgs a;
        memset(&a, 0, sizeof(a));
        a.n = c.n; a.erf_mode = c.erf_mode; a.r1 = c.r1; a.r2 = c.r2; a.front = c.front_dev.p;
        a.t = k.tail; a.ms = k.ms; a.stride = k.stride; a.sums_stride = M;
        a.out_val = k.at(p->out[EHVI_OUT_VAL]); a.out_sums = k.at(p->out[EHVI_OUT_SUMS]);
        KERNEL_TRY(launch_ehvi_finish(a, a.out_sums != nullptr, s));
        return IBO_OK;
    };
}

extern "C" int ibo_ehvi_sweep(ibo_gp_t *const *obj, int nfront, const double *front_host, const double *ref,
                              int64_t M, const double *cand_dev, int erf_mode, double clamp_lo,
                              int n_excl, const double *excl_host, double excl_radius, int64_t index_base,
                              double *val_dev, double *best_val, int64_t *best_idx)
{
    EhviCall c;
    IBO_TRY(ehvi_begin(obj, nfront, front_host, ref, M, cand_dev, erf_mode, clamp_lo, val_dev || best_val || best_idx, &c));
    MomentsPipeline p;
    ehvi_pipeline(c, M, &p);
    p.out[EHVI_OUT_VAL] = val_dev;
    return p.sweep(M, cand_dev, M, n_excl, excl_host, excl_radius, index_base, best_val, best_idx);
}

// Host points through the sweep's own route -- a strip scan on the host would cost about 40 us a point at 1024 strips, and the device's
// values are the sweep's bits.  val: M; sums (the gradient's): 6 M, see EhviArgs.
static int ehvi_eval_host(const EhviCall &c, int64_t M, const double *Q_host, double *val, double *sums)
{
    MomentsPipeline p;
    ehvi_pipeline(c, M, &p);
    double *const host[2] = {val, sums};
    const size_t len[2] = {(size_t)M, 6 * (size_t)M};
    return p.eval_host(M, Q_host, sums ? 2 : 1, host, len);
}

extern "C" int ibo_ehvi_batch(ibo_gp_t *const *obj, int nfront, const double *front_host, const double *ref,
                              int64_t M, const double *Q_host, int erf_mode, double clamp_lo, double *val_host)
{
    EhviCall c;
    IBO_TRY(ehvi_begin(obj, nfront, front_host, ref, M, Q_host, erf_mode, clamp_lo, val_host != nullptr, &c));
    return ehvi_eval_host(c, M, Q_host, val_host, nullptr);
}

// grad EHVI = sum_k G_mu_k grad mu_k + G_sigma_k grad s2_k / (2 sigma_k), k = 1, 2 in this order: the sums from the kernel's second
// variant, the posteriors' gradients from ibo_acq_grad_batch per handle (ds2 is 0 where the clip is active).
extern "C" int ibo_ehvi_grad_batch(ibo_gp_t *const *obj, int nfront, const double *front_host, const double *ref,
                                   int64_t M, const double *Q_host, int erf_mode, double clamp_lo, double *val_host, double *grad_host)
{
    EhviCall c;
    IBO_TRY(ehvi_begin(obj, nfront, front_host, ref, M, Q_host, erf_mode, clamp_lo, val_host || grad_host, &c));
    if (!grad_host) return ehvi_eval_host(c, M, Q_host, val_host, nullptr);
    const size_t m = (size_t)M, D = (size_t)c.g1->D;
    std::vector<double> sums(6 * m), dmu(m * D), ds2(m * D);
    IBO_TRY(ehvi_eval_host(c, M, Q_host, val_host, sums.data()));
    ibo_gp *gp[2] = {c.g1, c.g2};
    for (int k = 0; k < 2; k++) {
        IBO_TRY(ibo_acq_grad_batch(gp[k], M, Q_host, IBO_ACQ_NONE, 0.0, erf_mode, clamp_lo, NAN, nullptr, nullptr, nullptr, dmu.data(), ds2.data(),
                                   nullptr));
        const double *gm = sums.data() + 2 * k * m, *gs = gm + m, *sig = sums.data() + (4 + k) * m;
        for (size_t i = 0; i < m; i++)
            for (size_t d = 0; d < D; d++) {
                const double t = gm[i] * dmu[i * D + d] + gs[i] * (ds2[i * D + d] / (2.0 * sig[i]));
                grad_host[i * D + d] = k ? grad_host[i * D + d] + t : t;
            }
    }
    return IBO_OK;
}

// direct_maximize over both handles: the same driver, every batch through ehvi_eval_host
extern "C" int ibo_ehvi_direct_max(ibo_gp_t *const *obj, int nfront, const double *front_host, const double *ref,
                                   int D, const double *lb, const double *ub, int erf_mode, double clamp_lo,
                                   int maxiter, int maxtime, int maxsample, int compat, double *opt, double *optx, int64_t *nsamples)
{
    EhviCall c;
    IBO_TRY(ehvi_begin(obj, nfront, front_host, ref, 1, (lb && ub) ? lb : nullptr, erf_mode, clamp_lo, opt || optx || nsamples, &c));
    if (D != c.g1->D) return fail(IBO_ERR_ARG, "bounds have %d dimensions, the models have %d", D, c.g1->D);
    const ibo::batch_eval_t value = [&](const double *pts, int n, double *vals) -> int { return ehvi_eval_host(c, n, pts, vals, nullptr); };
    char label[64];
    snprintf(label, sizeof(label), "hypervolume DIRECT (%d front points)", c.n);
    return direct_maximize(value, label, D, lb, ub, maxiter, maxtime, maxsample, compat, opt, optx, nsamples);
}

extern "C" int ibo_ehvi_scan_ms(double *ms, int reset)
{
    return read_stage_sums(&t_ehvi_ms, 1, ms, reset);
}

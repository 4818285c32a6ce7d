// abi_cacq.hip -- the constrained acquisition behind the C ABI: A(x) prod_j Phi(z_j) over several handles -- ibo_cacq_sweep, ibo_cacq_batch,
// ibo_cacq_grad_batch, ibo_cacq_direct_max (kernel: cacq.hip; the sweep's chunks: abi_moments.h; the host batches' per-model work: eval_host_points).
#include "abi_moments.h"
#include "cacq.h"

std::atomic<int> g_cacq_chunk{0};     // ibo_set_option("cacq_chunk", m): candidates per chunk of ibo_cacq_sweep (rounded up to 256); 0: by bytes

static_assert(IBO_CACQ_MAX == IBO_CACQ_MAX_CON, "the kernel argument arrays hold every constraint the ABI admits");

// the leading arguments of the four ibo_cacq_* entries
struct CacqCall {
    ibo_gp *obj; int ncon; ibo_gp *const *con; const double *thresh; const int *sense;
    int acq; double parm; int erf_mode; double clamp_lo, ymax;
};

// What the four entries check alike, in ibo_abi.h's order: the device first (as ibo_posterior_cov), then the arguments, then the handles'
// state -- and their dimensionality last, which only a fitted handle has.  points: the entry's candidate / query array; any_out: whether
// it was given an output at all.  Fills the kernel's view of the request (ymax NaN: the objective's largest observation).
static int cacq_begin(const CacqCall &c, int64_t M, const void *points, bool any_out, CacqSpec *sp)
{
    IBO_TRY(use_device(c.obj ? c.obj->device : 0));
    if (!c.obj) return fail(IBO_ERR_ARG, "the objective handle is NULL");
    if (c.ncon < 0 || c.ncon > IBO_CACQ_MAX_CON) return fail(IBO_ERR_ARG, "ncon=%d outside [0, %d]", c.ncon, IBO_CACQ_MAX_CON);
    if (c.ncon > 0 && (!c.con || !c.thresh || !c.sense)) return fail(IBO_ERR_ARG, "NULL constraint argument");
    for (int j = 0; j < c.ncon; j++) {
        if (!c.con[j]) return fail(IBO_ERR_ARG, "constraint handle %d is NULL", j);
        if (c.sense[j] != 1 && c.sense[j] != -1) return fail(IBO_ERR_ARG, "sense[%d]=%d is neither +1 nor -1", j, c.sense[j]);
        if (!(fabs(c.thresh[j]) < HUGE_VAL)) return fail(IBO_ERR_ARG, "thresh[%d]=%g is not finite", j, c.thresh[j]);
        if (c.con[j]->device != c.obj->device)
            return fail(IBO_ERR_ARG, "constraint %d lives on device %d, the objective on device %d", j, c.con[j]->device, c.obj->device);
    }
    if (M < 1) return fail(IBO_ERR_ARG, "M=%lld", (long long)M);
    if (!points) return fail(IBO_ERR_ARG, "NULL argument");
    if (c.acq == IBO_ACQ_UCB) return fail(IBO_ERR_ARG, "IBO_ACQ_UCB has no constrained form: a signed value times a probability orders nothing");
    if (c.acq != IBO_ACQ_EI && c.acq != IBO_ACQ_PI && c.acq != IBO_ACQ_NONE) return fail(IBO_ERR_ARG, "unknown acquisition %d", c.acq);
    if (c.erf_mode != IBO_ERF_LIBM && c.erf_mode != IBO_ERF_NR) return fail(IBO_ERR_ARG, "unknown erf mode %d", c.erf_mode);
    if (!any_out) return fail(IBO_ERR_ARG, "every output is NULL");
    if (!c.obj->fitted) return fail(IBO_ERR_STATE, "constrained acquisition before the objective's fit");
    for (int j = 0; j < c.ncon; j++)
        if (!c.con[j]->fitted) return fail(IBO_ERR_STATE, "constrained acquisition before constraint %d's fit", j);
    for (int j = 0; j < c.ncon; j++)
        if (c.con[j]->D != c.obj->D)
            return fail(IBO_ERR_ARG, "constraint %d has %d dimensions, the objective %d", j, c.con[j]->D, c.obj->D);
    memset(sp, 0, sizeof(*sp));
    sp->ncon = c.ncon; sp->acq = c.acq; sp->erf_mode = c.erf_mode;
    sp->ymax = (c.ymax == c.ymax) ? c.ymax : c.obj->maxY; sp->parm = c.parm;
    for (int j = 0; j < c.ncon; j++) { sp->thresh[j] = c.thresh[j]; sp->sense[j] = c.sense[j]; }
    return IBO_OK;
}

// One plain sweep per model, one after the other (a handle may appear more than once; the pure probability of feasibility does not look at
// the objective), then cacq_finish_kernel on the objective's stream.  Scratch: 16 (ncon + 1) bytes per candidate from the pool, at most
// about 1 GiB (more candidates go in chunks), handed back before the call returns.  No launch is padded: see MomentsPipeline::padded.
extern "C" int ibo_cacq_sweep(ibo_gp_t *obj, int ncon, ibo_gp_t *const *con, const double *thresh, const int *sense,
                              int64_t M, const double *cand_dev, int acq, double parm, int erf_mode, double clamp_lo, double ymax,
                              int n_excl, const double *excl_host, double excl_radius, int64_t index_base,
                              double *acq_dev, double *pof_dev, double *val_dev, double *best_val, int64_t *best_idx)
{
    const CacqCall c = {obj, ncon, con, thresh, sense, acq, parm, erf_mode, clamp_lo, ymax};
    CacqSpec spec;
    IBO_TRY(cacq_begin(c, M, cand_dev, acq_dev || pof_dev || val_dev || best_val || best_idx, &spec));
    MomentsPipeline p;
    p.add(obj, true, true, clamp_lo, erf_mode, acq != IBO_ACQ_NONE);
    for (int j = 0; j < ncon; j++) p.add(con[j], true, true, clamp_lo, erf_mode);
    p.home = obj; p.padded = false; p.chunk_opt = g_cacq_chunk;
    p.out[0] = acq_dev; p.out[1] = pof_dev; p.out[2] = val_dev;
    p.finish = [&](const MomentChunk &k, hipStream_t s) -> int {
        CacqArgs a;
        memset(&a, 0, sizeof(a));
        a.spec = spec; a.t = k.tail; a.ms = k.ms; a.stride = k.stride;
        a.out_acq = k.at(p.out[0]); a.out_pof = k.at(p.out[1]); a.out_val = k.at(p.out[2]);
        KERNEL_TRY(launch_cacq_finish(a, s));
        return IBO_OK;
    };
    return p.sweep(M, cand_dev, M, n_excl, excl_host, excl_radius, index_base, best_val, best_idx);
}

// Host batches (and with them every DIRECT batch): the ncon + 1 eval_host_points calls one after the other -- the objective's acquisition
// as ibo_acq_batch returns it, (mu, s2) of each constraint -- then the combine on the HOST (cacq.h's twin of gauss_cdf_pdf_dev): the
// per-model results are in host memory already, and one erf per constraint and point (about 20 ns) is less than another launch and wait.
// A, P, val: M each, any may be NULL.  keep (the gradient's): Phi, phi, z and sigma of every constraint, constraint-major.
struct CacqHostTerms { std::vector<double> cdf, pdf, z, sig; };
static int cacq_eval_host(const CacqCall &c, const CacqSpec &sp, int64_t M, const double *Q_host, double *A, double *P, double *val,
                          CacqHostTerms *keep)
{
    const size_t m = (size_t)M;
    std::vector<double> a(m, 1.0), p(m, 1.0), mu(c.ncon ? m : 0), s2(c.ncon ? m : 0);
    if (c.acq != IBO_ACQ_NONE)
        IBO_TRY(eval_host_points(c.obj, M, Q_host, c.acq, c.parm, c.erf_mode, c.clamp_lo, nullptr, nullptr, a.data(), sp.ymax));
    std::vector<double> v(a);
    if (keep) { keep->cdf.resize(m * c.ncon); keep->pdf.resize(m * c.ncon); keep->z.resize(m * c.ncon); keep->sig.resize(m * c.ncon); }
    for (int j = 0; j < c.ncon; j++) {
        IBO_TRY(eval_host_points(c.con[j], M, Q_host, IBO_ACQ_NONE, 0.0, c.erf_mode, c.clamp_lo, mu.data(), s2.data(), nullptr));
        for (size_t i = 0; i < m; i++) {
            const double sig = sqrt(s2[i]);
            const double z = (double)sp.sense[j] * (sp.thresh[j] - mu[i]) / sig;
            double cdf, pdf;
            gauss_cdf_pdf_host(c.erf_mode, z, &cdf, &pdf);
            p[i] *= cdf; v[i] *= cdf;
            if (keep) { keep->cdf[j * m + i] = cdf; keep->pdf[j * m + i] = pdf; keep->z[j * m + i] = z; keep->sig[j * m + i] = sig; }
        }
    }
    if (A) memcpy(A, a.data(), sizeof(double) * m);
    if (P) memcpy(P, p.data(), sizeof(double) * m);
    if (val) memcpy(val, v.data(), sizeof(double) * m);
    return IBO_OK;
}

extern "C" int ibo_cacq_batch(ibo_gp_t *obj, int ncon, ibo_gp_t *const *con, const double *thresh, const int *sense,
                              int64_t M, const double *Q_host, int acq, double parm, int erf_mode, double clamp_lo, double ymax,
                              double *acq_host, double *pof_host, double *val_host)
{
    const CacqCall c = {obj, ncon, con, thresh, sense, acq, parm, erf_mode, clamp_lo, ymax};
    CacqSpec sp;
    IBO_TRY(cacq_begin(c, M, Q_host, acq_host || pof_host || val_host, &sp));
    return cacq_eval_host(c, sp, M, Q_host, acq_host, pof_host, val_host, nullptr);
}

// grad val = grad A . P + A . grad P, composed on the host from ibo_acq_grad_batch per handle (dacq of the objective, dmu / ds2 of each
// constraint) in a fixed order; no division by Phi, so it stays finite where a factor underflows.
extern "C" int ibo_cacq_grad_batch(ibo_gp_t *obj, int ncon, ibo_gp_t *const *con, const double *thresh, const int *sense,
                                   int64_t M, const double *Q_host, int acq, double parm, int erf_mode, double clamp_lo, double ymax,
                                   double *val_host, double *dval_host)
{
    const CacqCall c = {obj, ncon, con, thresh, sense, acq, parm, erf_mode, clamp_lo, ymax};
    CacqSpec sp;
    IBO_TRY(cacq_begin(c, M, Q_host, val_host || dval_host, &sp));
    const size_t m = (size_t)M, D = (size_t)obj->D;
    CacqHostTerms t;
    std::vector<double> A(m), P(m);
    IBO_TRY(cacq_eval_host(c, sp, M, Q_host, A.data(), P.data(), val_host, dval_host ? &t : nullptr));
    if (!dval_host) return IBO_OK;
    std::vector<double> g1(m * D), g2(ncon ? m * D : 0), dP(m * D, 0.0);
    if (acq != IBO_ACQ_NONE)
        IBO_TRY(ibo_acq_grad_batch(obj, M, Q_host, acq, parm, erf_mode, clamp_lo, sp.ymax, nullptr, nullptr, nullptr, nullptr, nullptr, g1.data()));
    for (size_t i = 0; i < m; i++)
        for (size_t d = 0; d < D; d++) dval_host[i * D + d] = (acq != IBO_ACQ_NONE) ? g1[i * D + d] * P[i] : 0.0;
    for (int j = 0; j < ncon; j++) {
        IBO_TRY(ibo_acq_grad_batch(con[j], M, Q_host, IBO_ACQ_NONE, 0.0, erf_mode, clamp_lo, NAN, nullptr, nullptr, nullptr, g1.data(), g2.data(),
                                   nullptr));
        for (size_t i = 0; i < m; i++) {
            double w = t.pdf[j * m + i];                         // phi(z_j) prod_{k != j} Phi(z_k), k ascending
            for (int k = 0; k < ncon; k++)
                if (k != j) w *= t.cdf[k * m + i];
            const double sig = t.sig[j * m + i], z = t.z[j * m + i];
            for (size_t d = 0; d < D; d++) {
                const double dsig = g2[i * D + d] / (2.0 * sig);          // (ds2 is 0 where the clip is active)
                const double dz = -((double)sp.sense[j] * g1[i * D + d] + z * dsig) / sig;
                dP[i * D + d] += w * dz;
            }
        }
    }
    for (size_t i = 0; i < m; i++)
        for (size_t d = 0; d < D; d++) dval_host[i * D + d] += A[i] * dP[i * D + d];
    return IBO_OK;
}

// direct_on_gp over all the handles: the same driver, every batch through cacq_eval_host
extern "C" int ibo_cacq_direct_max(ibo_gp_t *obj, int ncon, ibo_gp_t *const *con, const double *thresh, const int *sense,
                                   int D, const double *lb, const double *ub, int acq, double parm, int erf_mode, double clamp_lo, double ymax,
                                   int maxiter, int maxtime, int maxsample, int compat, double *opt, double *optx, int64_t *nsamples)
{
    const CacqCall c = {obj, ncon, con, thresh, sense, acq, parm, erf_mode, clamp_lo, ymax};
    CacqSpec sp;
    IBO_TRY(cacq_begin(c, 1, (lb && ub) ? lb : nullptr, opt || optx || nsamples, &sp));
    if (D != obj->D) return fail(IBO_ERR_ARG, "bounds have %d dimensions, the models have %d", D, obj->D);
    const ibo::batch_eval_t value = [&](const double *pts, int n, double *vals) -> int {
        return cacq_eval_host(c, sp, n, pts, nullptr, nullptr, vals, nullptr);
    };
    char label[64];
    snprintf(label, sizeof(label), "constrained DIRECT (%d constraints)", ncon);
    return direct_maximize(value, label, D, lb, ub, maxiter, maxtime, maxsample, compat, opt, optx, nsamples);
}

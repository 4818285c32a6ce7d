// abi_ehvi.hip -- the two-objective expected hypervolume improvement behind the C ABI: ibo_ehvi_sweep, ibo_ehvi_batch, ibo_ehvi_grad_batch,
// ibo_ehvi_direct_max (kernel: ehvi.hip; the per-model work: run_sweep; the front's canonical form: ehvi_front.h).
#include "abi_eval.h"
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

// What a call may ask of the device pass beside the arg-max: the values, and the gradient's sums (six arrays M apart)
struct EhviOut { double *val_dev = nullptr, *sums_dev = nullptr; double *best_val = nullptr; int64_t *best_idx = nullptr; };

// The one route of every entry: per chunk the two plain sweeps -- (mu, s2) into pooled scratch, 32 bytes per candidate, no arg-max, no
// read-back, one after the other (the same handle may be both) -- then ehvi_finish_kernel on the first model's stream.
// cand_rows: the rows cand_dev has room for (>= M; rows from M on are the caller's padding, see class_padded).
static int ehvi_device(const EhviCall &c, int64_t M, const double *cand_dev, int64_t cand_rows, int n_excl, const double *excl_host,
                       double excl_radius, int64_t index_base, const EhviOut &o)
{
    ibo_gp *g = c.g1;
    hipStream_t s = g->stream;
    const int D = g->D;
    EhviArgs a;
    memset(&a, 0, sizeof(a));
    a.n = c.n; a.erf_mode = c.erf_mode; a.r1 = c.r1; a.r2 = c.r2;
    a.D = D; a.index_base = index_base; a.excl_radius = excl_radius;
    IBO_TRY(upload_exclusions(g, n_excl, excl_host, &a.n_excl, &a.excl));
    int64_t mc = (((int64_t)1 << 30) / 32) / 256 * 256;        // candidates per chunk: a multiple of the combine's workgroup
    if (g_ehvi_chunk > 0) mc = ((int64_t)g_ehvi_chunk + 255) / 256 * 256;
    if (M <= mc) mc = M;
    const int64_t nblk = (M + 255) / 256;
    const int64_t stride = class_padded(mc, mc);               // (every launch of the call fits: a tail is padded to at most mc's own size class)
    ScopedBuf<double> ms, pv, pad;
    ScopedBuf<int64_t> pi;
    IBO_TRY(ms.ensure(4 * (size_t)stride));
    IBO_TRY(pv.ensure((size_t)nblk)); IBO_TRY(pi.ensure((size_t)nblk));
    a.front = c.front_dev.p;
    const bool timing = g_ehvi_timing != 0;
    struct Events {                                             // (the diagnostic's: made and destroyed per call)
        hipEvent_t e0 = nullptr, e1 = nullptr;
        ~Events() { if (e0) (void)hipEventDestroy(e0); if (e1) (void)hipEventDestroy(e1); }
    } ev;
    if (timing) { HIP_TRY(hipEventCreate(&ev.e0)); HIP_TRY(hipEventCreate(&ev.e1)); }
    a.ms = ms.p; a.stride = stride; a.sums_stride = M;
    for (int64_t c0 = 0; c0 < M; c0 += mc) {
        const int64_t m = M - c0 < mc ? M - c0 : mc, mp = class_padded(m, mc);
        SweepRequest r;
        r.M = mp; r.cand_dev = cand_dev + c0 * D; r.acq = IBO_ACQ_NONE; r.erf_mode = c.erf_mode; r.clamp_lo = c.clamp_lo;
        if (c0 + mp > cand_rows) {                              // a short launch of the caller's array: its candidates, then the padding
            IBO_TRY(pad.ensure((size_t)mp * D));
            HIP_TRY(hipMemcpyAsync(pad.p, r.cand_dev, sizeof(double) * (size_t)m * D, hipMemcpyDeviceToDevice, s));
            HIP_TRY(hipMemsetAsync(pad.p + (size_t)m * D, 0, sizeof(double) * (size_t)(mp - m) * D, s));
            HIP_TRY(hipStreamSynchronize(s));                   // (the second model's sweep reads them on its own stream)
            r.cand_dev = pad.p;
        }
        r.mu_dev = ms.p; r.s2_dev = ms.p + stride;
        IBO_TRY(run_sweep(c.g1, r));
        r.mu_dev = ms.p + 2 * (size_t)stride; r.s2_dev = ms.p + 3 * (size_t)stride;
        IBO_TRY(run_sweep(c.g2, r));
        if (c.g2->stream != s) HIP_TRY(hipStreamSynchronize(c.g2->stream));     // the combine runs on the first model's stream
        a.M = m; a.first = c0; a.cand = r.cand_dev;
        a.out_val = o.val_dev ? o.val_dev + c0 : nullptr;
        a.out_sums = o.sums_dev ? o.sums_dev + c0 : nullptr;
        a.part_val = pv.p + c0 / 256; a.part_idx = pi.p + c0 / 256;
        if (timing) HIP_TRY(hipEventRecord(ev.e0, s));
        KERNEL_TRY(launch_ehvi_finish(a, o.sums_dev != nullptr, s));
        if (timing) {
            float ms1 = 0.f;
            HIP_TRY(hipEventRecord(ev.e1, s)); HIP_TRY(hipEventSynchronize(ev.e1)); HIP_TRY(hipEventElapsedTime(&ms1, ev.e0, ev.e1));
            t_ehvi_ms += ms1;
        }
        if (c0 + mc < M) HIP_TRY(hipStreamSynchronize(s));      // the next chunk's sweeps, on another stream, write the same scratch
    }
    if (o.best_val || o.best_idx) return argmax_readback(g, pv.p, pi.p, nblk, o.best_val, o.best_idx);
    HIP_TRY(hipStreamSynchronize(s));
    return IBO_OK;
}

extern "C" int ibo_ehvi_sweep(ibo_gp_t *const *obj, int nfront, const double *front_host, const double *ref,
                              int64_t M, const double *cand_dev, int erf_mode, double clamp_lo,
                              int n_excl, const double *excl_host, double excl_radius, int64_t index_base,
                              double *val_dev, double *best_val, int64_t *best_idx)
{
    EhviCall c;
    IBO_TRY(ehvi_begin(obj, nfront, front_host, ref, M, cand_dev, erf_mode, clamp_lo, val_dev || best_val || best_idx, &c));
    EhviOut o;
    o.val_dev = val_dev; o.best_val = best_val; o.best_idx = best_idx;
    return ehvi_device(c, M, cand_dev, M, n_excl, excl_host, excl_radius, index_base, o);
}

// Host points: uploaded, then the sweep's own two sweeps and kernel -- a strip scan on the host would cost about 40 us a point at 1024
// strips, and the device's values are the sweep's bits.  val: M; sums (the gradient's): 6 M, see EhviArgs.
static int ehvi_eval_host(const EhviCall &c, int64_t M, const double *Q_host, double *val, double *sums)
{
    const size_t m = (size_t)M;
    hipStream_t s = c.g1->stream;
    const size_t rows = (size_t)class_padded(M, M), D = (size_t)c.g1->D;      // (a short batch carries its padding: no copy on the device)
    ScopedBuf<double> q, out;
    IBO_TRY(q.ensure(rows * D)); IBO_TRY(out.ensure(m * (sums ? 7 : 1)));
    HIP_TRY(hipMemcpyAsync(q.p, Q_host, sizeof(double) * m * D, hipMemcpyHostToDevice, s));
    if (rows > m) HIP_TRY(hipMemsetAsync(q.p + m * D, 0, sizeof(double) * (rows - m) * D, s));
    HIP_TRY(hipStreamSynchronize(s));                          // (the second model's sweep reads them on its own stream)
    EhviOut o;
    o.val_dev = out.p; o.sums_dev = sums ? out.p + m : nullptr;
    IBO_TRY(ehvi_device(c, M, q.p, (int64_t)rows, 0, nullptr, 0.0, 0, o));
    if (val) HIP_TRY(hipMemcpyAsync(val, out.p, sizeof(double) * m, hipMemcpyDeviceToHost, s));
    if (sums) HIP_TRY(hipMemcpyAsync(sums, out.p + m, sizeof(double) * 6 * m, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return IBO_OK;
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
    if (ms) *ms = t_ehvi_ms;
    if (reset) t_ehvi_ms = 0.0;
    return IBO_OK;
}

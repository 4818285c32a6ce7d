// abi_gradobs.hip -- a GP observed with gradients behind the C ABI: ibo_ggp_* (kernels: gradobs.hip; the rest are existing launches).
//
// The model has P = N (D + 1) rows in point-major order (gradobs.h).  Its handle wraps an ibo_gp that no other entry ever sees and that
// serves as the P-row FRAME: stream, events, pinned staging, L, W = L^-1, alpha = A^-1 [Y; G], the arg-max result words.  The frame's own
// points, scaled copies and packed operands are never made: nothing of the plain sweeps runs on it.
//   fit     gradobs_assemble_kernel into the identity-padded frame, factor_invert on the route of a plain fit (FACTOR_FIT), launch_alpha
//   values  the row pipeline (abi_rows.h) with this unit's K* (gradobs_kstar_kernel) in place of launch_cov_kstar: V^T = K* W^T by
//           launch_cov_tri, the row kernel (K = N = P: mu = k*.alpha, s2 = 1 + noise - |v|^2 clipped), then acq_value_dev per candidate;
//           launch_kg_argmax / launch_argmax_final for the winner
// Every entry sends its points through RowPipeline::chunk, and nothing there lets a row depend on the rows beside it: a candidate's value
// is the same bits from the host batch, the sweep and DIRECT, whatever the chunk.
#include "abi_rows.h"
#include "abi_factor.h"
#include "gradobs.h"

std::atomic<int> g_ggp_chunk{0};      // ibo_set_option("ggp_chunk", m): candidates per chunk (rounded up to 256); 0: by bytes
std::atomic<int> g_ggp_timing{0};     // ibo_set_option("ggp_timing", 1): HIP events around every stage, read with ibo_ggp_stage_ms
static thread_local double t_ggp_ms[IBO_GGP_STAGES];
static_assert(IBO_GGP_STAGES == ROW_STAGES + 2, "the row pipeline's six slots, then the factorisation and the alpha vectors");
enum { GGP_ST_ASSEMBLE = ST_STATE, GGP_ST_FACTOR = ROW_STAGES, GGP_ST_ALPHA = ROW_STAGES + 1 };

struct ibo_ggp {
    ibo_gp *g = nullptr;              // the P-row frame
    int device = 0, N = 0, D = 0, P = 0;
    bool fitted = false;
    KParams kp;
    double noise = 0.0, maxY = 0.0;
    DevBuf<double> X, gnoise;         // N x D, D
    void release() { X.release(); gnoise.release(); }
};

namespace {

struct GgpRun {
    ibo_ggp *h = nullptr;
    int acq = IBO_ACQ_NONE, erf_mode = IBO_ERF_LIBM;
    double ymax = 0.0, parm = 0.0;
    const double *sweep_base = nullptr;              // a device sweep: where its candidates begin, and its per-candidate outputs
    double *mu_dev = nullptr, *s2_dev = nullptr;
    RowPipeline rows;
};

int ggp_begin(ibo_ggp *h, GgpRun &st, int acq, double parm, int erf_mode, double clamp_lo, double ymax)
{
    st.h = h; st.acq = acq; st.erf_mode = erf_mode; st.parm = parm;
    st.ymax = ymax == ymax ? ymax : h->maxY;          // NaN: the largest observed VALUE
    IBO_TRY(st.rows.begin(h->g, clamp_lo, g_ggp_chunk, 1, 0, false, g_ggp_timing != 0, t_ggp_ms));
    st.rows.kstar = [h](const double *pts, int m, int mp, double *kt, hipStream_t s) -> int {
        KERNEL_TRY(launch_gradobs_kstar(h->kp, h->X.p, h->N, h->g->Npad, pts, m, mp, kt, s));
        return IBO_OK;
    };
    st.rows.tail = [&st](int m, int, const double *cand, double *out) -> int {
        RowPipeline &p = st.rows;
        IBO_TRY(p.clock.mark(4));                     // (no cross stage)
        const size_t c0 = st.sweep_base ? (size_t)(cand - st.sweep_base) / (size_t)st.h->D : 0;
        KERNEL_TRY(launch_gradobs_acq(st.acq, st.erf_mode, st.ymax, st.parm, p.mu.p, p.s2.p, m, out, st.mu_dev ? st.mu_dev + c0 : nullptr,
                                      st.s2_dev ? st.s2_dev + c0 : nullptr, p.g->stream));
        return p.clock.mark(5);
    };
    return IBO_OK;
}

}  // namespace

extern "C" int ibo_ggp_create(int device, ibo_ggp_t **out)
{
    if (!out) return fail(IBO_ERR_ARG, "out is NULL");
    ibo_gp *g = nullptr;
    IBO_TRY(ibo_gp_create(device, &g));
    ibo_ggp *h = new ibo_ggp();
    h->g = g; h->device = device;
    memset(&h->kp, 0, sizeof(h->kp));
    *out = h;
    return IBO_OK;
}

extern "C" int ibo_ggp_destroy(ibo_ggp_t *h)
{
    if (!h) return IBO_OK;
    (void)hipSetDevice(h->device);
    (void)hipDeviceSynchronize();
    g_pool_quiet = true;
    h->release();
    g_pool_quiet = false;
    const int rc = ibo_gp_destroy(h->g);
    delete h;
    return rc;
}

extern "C" int ibo_ggp_info(ibo_ggp_t *h, int *N, int *D, int *P, int *device, double *max_y)
{
    if (!h) return fail(IBO_ERR_ARG, "handle is NULL");
    if (N) *N = h->N;
    if (D) *D = h->D;
    if (P) *P = h->P;
    if (device) *device = h->device;
    if (max_y) *max_y = h->maxY;
    return IBO_OK;
}

extern "C" int ibo_ggp_fit(ibo_ggp_t *h, int ktype, int N, int D, const double *X, const double *Y, const double *G,
                           const double *hyper, int nhyper, double sf2, double noise, const double *gnoise, int *info)
{
    if (!h) return fail(IBO_ERR_ARG, "handle is NULL");
    IBO_TRY(use_device(h->device));
    if (!X || !Y || !G || !gnoise) return fail(IBO_ERR_ARG, "X/Y/G/gnoise is NULL");
    if (N < 1) return fail(IBO_ERR_ARG, "N=%d", N);
    KParams kp;
    IBO_TRY(make_kparams(ktype, D, hyper, nhyper, sf2, &kp));
    if ((int64_t)N * (D + 1) > IBO_GGP_MAX_ROWS)
        return fail(IBO_ERR_ARG, "N (D + 1) = %lld rows, at most %d", (long long)N * (D + 1), IBO_GGP_MAX_ROWS);
    if (info) *info = 0;
    ibo_gp *g = h->g;
    hipStream_t s = g->stream;
    const int P = N * (D + 1), Np = round_up(P, 64);
    h->fitted = false; g->fitted = false;
    h->N = N; h->D = D; h->P = P; h->kp = kp; h->noise = noise;
    // the frame: P rows, no points of its own, no prior
    g->N = P; g->D = D; g->Npad = Np; g->DP = D; g->kp = kp; g->kp_fit = kp; g->noise = noise; g->nb = 0;
    g->reversed = false; g->R_valid = false; g->st_gen = 0; g->pw.ready = false;
    IBO_TRY(h->X.ensure((size_t)N * D)); IBO_TRY(h->gnoise.ensure((size_t)D));
    IBO_TRY(fit_buffers(g, Np));
    // [Y; G] interleaved point by point, through the frame's pinned buffer (see stage_data in abi_fit.hip)
    IBO_TRY(ensure_pinned(g, (size_t)N * D + D + Np));
    double *xp = g->pin, *gp = xp + (size_t)N * D, *yp = gp + D;
    memcpy(xp, X, sizeof(double) * (size_t)N * D);
    memcpy(gp, gnoise, sizeof(double) * D);
    memset(yp, 0, sizeof(double) * Np);
    double my = Y[0];
    for (int i = 0; i < N; i++) {
        yp[(size_t)i * (D + 1)] = Y[i];
        for (int d = 0; d < D; d++) yp[(size_t)i * (D + 1) + 1 + d] = G[(size_t)i * D + d];
        if (Y[i] > my) my = Y[i];
    }
    h->maxY = my; g->maxY = my;
    HIP_TRY(hipMemcpyAsync(h->X.p, xp, sizeof(double) * (size_t)N * D, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(h->gnoise.p, gp, sizeof(double) * D, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(g->Y.p, yp, sizeof(double) * Np, hipMemcpyHostToDevice, s));
    // the frame and the tail of a plain fit (abi_fit.hip), around this model's own assembly
    FactorRoute route;
    FactorBufs b;
    IBO_TRY(fit_operands(g, &route, &b));                        // (eye_ready false: the factorisation writes the identity)
    StageClock clock;
    IBO_TRY(clock.make(s, t_ggp_ms, g_ggp_timing != 0));
    HIP_TRY(hipMemsetAsync(g->info.p, 0, sizeof(int), s));
    HIP_TRY(hipEventRecord(g->fit0, s));
    IBO_TRY(clock.mark(0));
    KERNEL_TRY(launch_gradobs_assemble(kp, h->X.p, N, 1.0 + noise, h->gnoise.p, b.A, Np, s));
    IBO_TRY(clock.mark(1));
    IBO_TRY(fit_invert(g, route, b, P));
    IBO_TRY(clock.mark(2));
    IBO_TRY(fit_alpha(g, P));
    IBO_TRY(clock.mark(3));                                      // (on the stream before fit_end waits for anything)
    IBO_TRY(fit_end(g, false, "gradient-observation matrix", info));      // synchronises; a failed pivot leaves the handle unfitted
    const int stage[3] = {GGP_ST_ASSEMBLE, GGP_ST_FACTOR, GGP_ST_ALPHA};
    for (int k = 0; k < 3; k++)
        if (const int rc = clock.account(k, k + 1, stage[k])) { g->fitted = false; return rc; }      // (as before: neither handle counts as fitted)
    h->fitted = true;
    return IBO_OK;
}

// A as factored: assembled again by the fit's kernel from the fit's inputs (the factorisation consumed its copy) -- the same bits
extern "C" int ibo_ggp_get_R(ibo_ggp_t *h, double *R_host)
{
    IBO_TRY(use_device(h ? h->device : 0));
    if (!h || !R_host) return fail(IBO_ERR_ARG, "NULL argument");
    if (!h->fitted) return fail(IBO_ERR_STATE, "R before a successful fit");
    const int Np = h->g->Npad;
    hipStream_t s = h->g->stream;
    ScopedBuf<double> A;
    IBO_TRY(A.ensure((size_t)Np * Np));
    KERNEL_TRY(launch_gradobs_assemble(h->kp, h->X.p, h->N, 1.0 + h->noise, h->gnoise.p, A.p, Np, s));
    HIP_TRY(hipMemcpy2DAsync(R_host, sizeof(double) * h->P, A.p, sizeof(double) * Np, sizeof(double) * h->P, (size_t)h->P, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return IBO_OK;
}

extern "C" int ibo_ggp_get_L(ibo_ggp_t *h, double *L_host)
{
    IBO_TRY(use_device(h ? h->device : 0));
    if (!h || !L_host) return fail(IBO_ERR_ARG, "NULL argument");
    if (!h->fitted) return fail(IBO_ERR_STATE, "L before a successful fit");
    return ibo_gp_get_L(h->g, L_host);
}

extern "C" int ibo_ggp_acq_batch(ibo_ggp_t *h, int64_t M, const double *Q_host, int acq, double parm, int erf_mode,
                                 double clamp_lo, double ymax, double *mu_host, double *s2_host, double *acq_host)
{
    IBO_TRY(wrapped_check(h, "gradient", Q_host != nullptr, M, acq, erf_mode, true));
    if (!mu_host && !s2_host && !acq_host) return fail(IBO_ERR_ARG, "every output is NULL");
    HIP_TRY(hipEventRecord(h->g->ev0, h->g->stream));
    GgpRun st;
    IBO_TRY(ggp_begin(h, st, acq, parm, erf_mode, clamp_lo, ymax));
    IBO_TRY(st.rows.eval_host(M, Q_host, acq_host, mu_host, s2_host, nullptr, 0));
    return finish_span(h->g);
}

extern "C" int ibo_ggp_acq_sweep(ibo_ggp_t *h, int64_t M, const double *cand_dev, int acq, double parm, int erf_mode,
                                 double clamp_lo, double ymax, int64_t index_base,
                                 double *mu_dev, double *s2_dev, double *acq_dev, double *best_val, int64_t *best_idx)
{
    IBO_TRY(wrapped_check(h, "gradient", cand_dev != nullptr, M, acq, erf_mode, true));
    if (!mu_dev && !s2_dev && !acq_dev && !best_val && !best_idx) return fail(IBO_ERR_ARG, "every output is NULL");
    HIP_TRY(hipEventRecord(h->g->ev0, h->g->stream));
    GgpRun st;
    IBO_TRY(ggp_begin(h, st, acq, parm, erf_mode, clamp_lo, ymax));
    st.sweep_base = cand_dev; st.mu_dev = mu_dev; st.s2_dev = s2_dev;
    return st.rows.sweep(M, cand_dev, index_base, acq_dev, best_val, best_idx);
}

extern "C" int ibo_ggp_direct_max(ibo_ggp_t *h, int D, const double *lb, const double *ub, int acq, double parm, int erf_mode,
                                  double clamp_lo, int maxiter, int maxtime, int maxsample, int compat,
                                  double *opt, double *optx, int64_t *nsamples)
{
    IBO_TRY(wrapped_check(h, "gradient", lb && ub, 1, acq, erf_mode, false));
    if (!opt && !optx && !nsamples) return fail(IBO_ERR_ARG, "every output is NULL");
    if (D != h->D) return fail(IBO_ERR_ARG, "bounds have %d dimensions, the model has %d", D, h->D);
    GgpRun st;
    IBO_TRY(ggp_begin(h, st, acq, parm, erf_mode, clamp_lo, NAN));
    const ibo::batch_eval_t value = [&](const double *pts, int n, double *vals) -> int {
        return st.rows.eval_host(n, pts, vals, nullptr, nullptr, nullptr, 0);
    };
    return direct_maximize(value, "gradient-model DIRECT", D, lb, ub, maxiter, maxtime, maxsample, compat, opt, optx, nsamples);
}

extern "C" int ibo_ggp_stage_ms(double *ms, int reset)
{
    return read_stage_sums(t_ggp_ms, IBO_GGP_STAGES, ms, reset);
}

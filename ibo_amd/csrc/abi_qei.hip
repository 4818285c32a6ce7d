// abi_qei.hip -- the Monte-Carlo parallel expected improvement behind the C ABI: ibo_qei_sweep, ibo_qei_batch, ibo_qei_direct_max
// (kernels: qei.hip, kg.hip, cov.hip).
//
// ONE route for every entry: the pending state (the pending points, their V^T rows, mu_P, L_P on the host, the transposed samples with g
// beside them) is built once per call and stays on the device; candidates go through the row pipeline (abi_rows.h) in chunks of a multiple
// of 256 -- K* and V^T by cov.hip's launchers, kg.hip's row kernel, and this unit's tail: kg.hip's cross kernel without its division, the
// finish.  None of these lets a row's result depend on the rows beside it, so a candidate's bits are the same from a sweep, a host batch or
// a DIRECT batch, whatever the chunk.
//
// Scratch, all from the pool and handed back on every exit path: the pending state (3 x 64 Npad doubles while it is built, 64 Npad after,
// and (p + 2) Sp doubles of samples); per chunk K* and V^T (mc Npad doubles each) and the covariances (mc x 64), each at most 256 MiB -- or
// 256 candidates where that alone is more -- and never more than 65280 candidates.
#include "abi_rows.h"
#include "qei.h"

std::atomic<int> g_qei_chunk{0};      // ibo_set_option("qei_chunk", m): candidates per chunk (rounded up to 256); 0: by bytes
std::atomic<int> g_qei_timing{0};     // ibo_set_option("qei_timing", 1): HIP events around every stage, read with ibo_qei_stage_ms
static thread_local double t_qei_ms[IBO_QEI_STAGES];

namespace {

struct QeiState {
    int p = 0, S = 0, Sp = 0;
    double t = 0.0, base = 0.0;
    std::vector<double> muP_host, S_host, zg_host;
    double L[QEI_MAX_P * (QEI_MAX_P + 1) / 2];
    ScopedBuf<double> P, vtP, ZG;                    // the pending state
    RowPipeline rows;                                // the chunks: its cross block holds the covariances C, 64 wide (none when p = 0)
};

inline bool is_fin(double v) { return fabs(v) < HUGE_VAL; }

// What the three entries check alike, in ibo_abi.h's order: the device first, the arguments, the handle's state, the values.
int qei_check(ibo_gp *g, int npend, const double *pend_host, int nsamp, const double *Z_host, double xi, double jitter, bool ptrs_ok, int64_t M,
              int *info)
{
    if (info) *info = 0;
    IBO_TRY(use_device(g ? g->device : 0));
    if (!g || !Z_host || !ptrs_ok || (npend > 0 && !pend_host)) return fail(IBO_ERR_ARG, "NULL argument");
    if (npend < 0 || npend > IBO_QEI_MAX_PENDING) return fail(IBO_ERR_ARG, "npend=%d outside [0, %d]", npend, IBO_QEI_MAX_PENDING);
    if (nsamp < 1 || nsamp > IBO_QEI_MAX_SAMPLES) return fail(IBO_ERR_ARG, "nsamp=%d outside [1, %d]", nsamp, IBO_QEI_MAX_SAMPLES);
    if (M < 1) return fail(IBO_ERR_ARG, "M=%lld", (long long)M);
    if (!g->fitted) return fail(IBO_ERR_STATE, "parallel expected improvement before a successful fit");
    if (!is_fin(xi)) return fail(IBO_ERR_ARG, "xi is not finite");
    if (!is_fin(jitter) || jitter < 0.0) return fail(IBO_ERR_ARG, "jitter must be finite and >= 0");
    for (size_t i = 0; i < (size_t)npend * g->D; i++)
        if (!is_fin(pend_host[i])) return fail(IBO_ERR_ARG, "pending coordinate %zu is not finite", i);
    for (size_t i = 0; i < (size_t)nsamp * (npend + 1); i++)
        if (!is_fin(Z_host[i])) return fail(IBO_ERR_ARG, "base sample %zu is not finite", i);
    return IBO_OK;
}

KgCrossArgs cross_args(const QeiState &st, const double *VtX, int m, int mp, const double *X, double *B)
{
    const ibo_gp *g = st.rows.g;
    KgCrossArgs c;
    memset(&c, 0, sizeof(c));
    c.kp = g->kp; c.VtX = VtX; c.ldx = (size_t)g->Npad; c.m = m; c.mp = mp; c.VtA = st.vtP.p; c.lda = (size_t)g->Npad; c.n = st.p; c.np = IBO_COV_TILE;
    c.K = round_up(g->N, 32); c.X = X; c.A = st.P.p; c.s2 = nullptr; c.B = B; c.ldb = (size_t)IBO_COV_TILE; c.unscaled = 1;
    return c;
}

// 64 partial sums (sample s goes to s mod 64, in ascending s), then the wavefront's butterfly: the finish kernel's order, so that
// base <= every value holds exactly
double lane_order_mean(const std::vector<double> &term, int S)
{
    double v[64], w[64];
    for (int l = 0; l < 64; l++) v[l] = 0.0;
    for (int s = 0; s < S; s++)
        if (term[s] > 0.0) v[s & 63] += term[s];
    for (int o = 32; o > 0; o >>= 1) {
        for (int l = 0; l < 64; l++) w[l] = v[l] + v[l ^ o];
        for (int l = 0; l < 64; l++) v[l] = w[l];
    }
    return v[0] / (double)S;
}

// The pipeline's tail: the covariances with the pending points (if there are any), then the finish.
int qei_tail(QeiState &st, int m, int mp, const double *cand, double *out)
{
    RowPipeline &r = st.rows;
    hipStream_t s = r.g->stream;
    if (st.p > 0) KERNEL_TRY(launch_kg_cross(cross_args(st, r.vt.p, m, mp, cand, r.cross.p), s));
    IBO_TRY(r.clock.mark(4));
    QeiFinishArgs f;
    memset(&f, 0, sizeof(f));
    f.m = m; f.p = st.p; f.S = st.S; f.Sp = st.Sp; f.t = st.t; f.ZG = st.ZG.p; f.mu = r.mu.p; f.s2 = r.s2.p; f.C = r.cross.p; f.ldc = (size_t)IBO_COV_TILE;
    f.qei = out;
    memcpy(f.L, st.L, sizeof(f.L));
    KERNEL_TRY(launch_qei_finish(f, s));
    return r.clock.mark(5);
}

// The pending state; the device is idle when this returns.
int qei_begin(ibo_gp *g, QeiState &st, int npend, const double *pend_host, int nsamp, const double *Z_host, double ymax, double xi,
              double clamp_lo, double jitter, int *info)
{
    const int Np = g->Npad, D = g->D, p = npend, T = IBO_COV_TILE;
    hipStream_t s = g->stream;
    StageClock &clock = st.rows.clock;
    st.p = p; st.S = nsamp; st.Sp = round_up(nsamp, QEI_SB);
    st.t = ((ymax == ymax) ? ymax : g->maxY) + xi;
    IBO_TRY(st.rows.begin(g, clamp_lo, g_qei_chunk, (size_t)T, p > 0 ? (size_t)T : 0, false, g_qei_timing != 0, t_qei_ms));
    st.rows.tail = [&st](int m, int mp, const double *cand, double *out) { return qei_tail(st, m, mp, cand, out); };
    st.muP_host.assign((size_t)p, 0.0); st.S_host.assign((size_t)p * p, 0.0);
    memset(st.L, 0, sizeof(st.L));
    IBO_TRY(st.ZG.ensure((size_t)(p + 2) * st.Sp));
    if (p > 0) {
        ScopedBuf<double> ktP, muP, qP, Bpp;
        std::vector<double> q_host((size_t)p), B_host((size_t)p * T);
        IBO_TRY(st.P.ensure((size_t)p * D)); IBO_TRY(st.vtP.ensure((size_t)T * Np)); IBO_TRY(ktP.ensure((size_t)T * Np));
        IBO_TRY(muP.ensure((size_t)T)); IBO_TRY(qP.ensure((size_t)T)); IBO_TRY(Bpp.ensure((size_t)T * T));
        IBO_TRY(clock.mark(0));
        HIP_TRY(hipMemcpyAsync(st.P.p, pend_host, sizeof(double) * (size_t)p * D, hipMemcpyHostToDevice, s));
        IBO_TRY(vt_rows(g, st.P.p, p, T, ktP.p, st.vtP.p, s));
        KgRowsArgs r = rows_args(g, ktP.p, st.vtP.p, st.P.p, p, clamp_lo);
        r.mu = muP.p; r.q = qP.p;
        KERNEL_TRY(launch_kg_rows(r, s));
        KERNEL_TRY(launch_kg_cross(cross_args(st, st.vtP.p, p, T, st.P.p, Bpp.p), s));
        HIP_TRY(hipMemcpyAsync(st.muP_host.data(), muP.p, sizeof(double) * (size_t)p, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipMemcpyAsync(q_host.data(), qP.p, sizeof(double) * (size_t)p, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipMemcpyAsync(B_host.data(), Bpp.p, sizeof(double) * (size_t)p * T, hipMemcpyDeviceToHost, s));
        IBO_TRY(clock.mark(1));
        HIP_TRY(hipStreamSynchronize(s));
        IBO_TRY(clock.account(0, 1, ST_STATE));
        // S_PP: the lower triangle as the cross kernel formed it, mirrored; the diagonal from |v_a|^2
        for (int a = 0; a < p; a++) {
            for (int b = 0; b < a; b++) st.S_host[(size_t)a * p + b] = st.S_host[(size_t)b * p + a] = B_host[(size_t)a * T + b];
            const double raw = 1.0 + g->noise - q_host[a];
            st.S_host[(size_t)a * p + a] = raw + jitter;
        }
        // L_P by rows, every sum in ascending k through fma (ibo_abi.h)
        for (int j = 0; j < p; j++) {
            double *Lj = st.L + j * (j + 1) / 2;
            for (int i = 0; i < j; i++) {
                const double *Li = st.L + i * (i + 1) / 2;
                double acc = st.S_host[(size_t)j * p + i];
                for (int k = 0; k < i; k++) acc = fma(-Lj[k], Li[k], acc);
                Lj[i] = acc / Li[i];
            }
            double acc = st.S_host[(size_t)j * p + j];
            for (int k = 0; k < j; k++) acc = fma(-Lj[k], Lj[k], acc);
            if (!(acc > 0.0) || !is_fin(acc)) {
                if (info) *info = j + 1;
                return fail(IBO_ERR_NOT_PD, "the pending points' joint covariance is not positive definite at pivot %d (raise jitter)", j + 1);
            }
            Lj[j] = sqrt(acc);
        }
    }
    // the samples transposed, g beside them, base
    const int S = nsamp, Sp = st.Sp, w = p + 1;
    st.zg_host.assign((size_t)(p + 2) * Sp, 0.0);
    std::vector<double> term((size_t)S);
    for (int si = 0; si < S; si++) {
        const double *z = Z_host + (size_t)si * w;
        for (int j = 0; j <= p; j++) st.zg_host[(size_t)j * Sp + si] = z[j];
        double gs = -INFINITY;
        for (int j = 0; j < p; j++) {
            const double *Lj = st.L + j * (j + 1) / 2;
            double y = st.muP_host[j];
            for (int i = 0; i <= j; i++) y = fma(Lj[i], z[i], y);
            gs = y > gs ? y : gs;
        }
        st.zg_host[(size_t)(p + 1) * Sp + si] = gs;
        term[si] = gs - st.t;
    }
    for (int si = S; si < Sp; si++) st.zg_host[(size_t)(p + 1) * Sp + si] = -INFINITY;
    st.base = p > 0 ? lane_order_mean(term, S) : 0.0;
    HIP_TRY(hipMemcpyAsync(st.ZG.p, st.zg_host.data(), sizeof(double) * st.zg_host.size(), hipMemcpyHostToDevice, s));
    HIP_TRY(hipStreamSynchronize(s));
    return IBO_OK;
}

}  // namespace

extern "C" int ibo_qei_sweep(ibo_gp_t *g, int npend, const double *pend_host, int nsamp, const double *Z_host, double ymax, double xi,
                             double clamp_lo, double jitter, int64_t M, const double *cand_dev, int64_t index_base, double *qei_dev,
                             double *base, double *best_val, int64_t *best_idx, int *info)
{
    IBO_TRY(qei_check(g, npend, pend_host, nsamp, Z_host, xi, jitter, cand_dev != nullptr, M, info));
    if (!qei_dev && !base && !best_val && !best_idx) return fail(IBO_ERR_ARG, "every output is NULL");
    HIP_TRY(hipEventRecord(g->ev0, g->stream));
    QeiState st;
    IBO_TRY(qei_begin(g, st, npend, pend_host, nsamp, Z_host, ymax, xi, clamp_lo, jitter, info));
    if (base) *base = st.base;
    if (!qei_dev && !best_val && !best_idx) return finish_span(g);
    return st.rows.sweep(M, cand_dev, index_base, qei_dev, best_val, best_idx);
}

extern "C" int ibo_qei_batch(ibo_gp_t *g, int npend, const double *pend_host, int nsamp, const double *Z_host, double ymax, double xi,
                             double clamp_lo, double jitter, int64_t M, const double *Q_host, double *qei_host, double *base,
                             double *mu_pend_host, double *S_pend_host, double *mu_host, double *s2_host, double *c_host, int *info)
{
    IBO_TRY(qei_check(g, npend, pend_host, nsamp, Z_host, xi, jitter, Q_host != nullptr, M, info));
    if (!qei_host && !base && !mu_pend_host && !S_pend_host && !mu_host && !s2_host && !c_host) return fail(IBO_ERR_ARG, "every output is NULL");
    HIP_TRY(hipEventRecord(g->ev0, g->stream));
    QeiState st;
    IBO_TRY(qei_begin(g, st, npend, pend_host, nsamp, Z_host, ymax, xi, clamp_lo, jitter, info));
    if (base) *base = st.base;
    if (mu_pend_host && npend > 0) memcpy(mu_pend_host, st.muP_host.data(), sizeof(double) * (size_t)npend);
    if (S_pend_host && npend > 0) memcpy(S_pend_host, st.S_host.data(), sizeof(double) * (size_t)npend * npend);
    if (qei_host || mu_host || s2_host || (c_host && npend > 0)) IBO_TRY(st.rows.eval_host(M, Q_host, qei_host, mu_host, s2_host, c_host, (size_t)npend));
    return finish_span(g);
}

// direct_maximize with the pending state and the samples kept on the device across the batches
extern "C" int ibo_qei_direct_max(ibo_gp_t *g, int npend, const double *pend_host, int nsamp, const double *Z_host, double ymax, double xi,
                                  double clamp_lo, double jitter, int D, const double *lb, const double *ub, int maxiter, int maxtime,
                                  int maxsample, int compat, double *opt, double *optx, int64_t *nsamples, int *info)
{
    IBO_TRY(qei_check(g, npend, pend_host, nsamp, Z_host, xi, jitter, lb && ub, 1, info));
    if (!opt && !optx && !nsamples) return fail(IBO_ERR_ARG, "every output is NULL");
    if (D != g->D) return fail(IBO_ERR_ARG, "bounds have %d dimensions, the model has %d", D, g->D);
    QeiState st;
    IBO_TRY(qei_begin(g, st, npend, pend_host, nsamp, Z_host, ymax, xi, clamp_lo, jitter, info));
    const ibo::batch_eval_t value = [&](const double *pts, int n, double *vals) -> int {
        return st.rows.eval_host(n, pts, vals, nullptr, nullptr, nullptr, 0);
    };
    char label[64];
    snprintf(label, sizeof(label), "parallel-EI DIRECT (%d pending, %d samples)", npend, nsamp);
    return direct_maximize(value, label, D, lb, ub, maxiter, maxtime, maxsample, compat, opt, optx, nsamples);
}

extern "C" int ibo_qei_stage_ms(double *ms, int reset)
{
    return read_stage_sums(t_qei_ms, IBO_QEI_STAGES, ms, reset);
}

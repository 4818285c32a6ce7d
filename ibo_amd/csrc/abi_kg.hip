// abi_kg.hip -- the knowledge gradient behind the C ABI: ibo_kg_sweep, ibo_kg_batch, ibo_kg_direct_max (kernels: kg.hip, cov.hip).
//
// ONE route for every entry: the reference state (the reference points, their V^T rows and posterior means) is built once per call and
// stays on the device; candidates go through the row pipeline (abi_rows.h) in chunks of a multiple of 256 -- K* and V^T by cov.hip's
// launchers, the row kernel, and this unit's tail: the cross kernel, the epigraph kernel.  None of these lets a row's result depend on
// the rows beside it, so a candidate's bits are the same from a sweep, a host batch or a DIRECT batch, whatever the chunk.
//
// Scratch, all from the pool and handed back on every exit path: the reference state, 2 np Npad doubles while it is built and np Npad
// after (np = nref rounded up to 64: 168 MiB each at 20480 rows and 1024 points); per chunk K* and V^T (mc Npad doubles each) and the
// slopes (mc np doubles), each at most 256 MiB -- or 256 candidates where that alone is more -- and never more than 65280 candidates.
#include "abi_rows.h"

std::atomic<int> g_kg_chunk{0};       // ibo_set_option("kg_chunk", m): candidates per chunk (rounded up to 256); 0: by bytes
std::atomic<int> g_kg_timing{0};      // ibo_set_option("kg_timing", 1): HIP events around every stage, read with ibo_kg_stage_ms
static thread_local double t_kg_ms[IBO_KG_STAGES];

namespace {

struct KgState {
    int n = 0, np = 0, with_self = 0;
    double maxA = 0.0;
    std::vector<double> muA_host;
    ScopedBuf<double> A, vtA, muA;                   // the reference state
    RowPipeline rows;                                // the chunks: its cross block holds the slopes B, np wide
};

// What the three entries check alike, in ibo_abi.h's order: the device first (as ibo_posterior_cov), the arguments, the handle's state.
int kg_check(ibo_gp *g, int nref, const double *ref_host, bool ptrs_ok, int64_t M)
{
    IBO_TRY(use_device(g ? g->device : 0));
    if (!g || !ref_host || !ptrs_ok) return fail(IBO_ERR_ARG, "NULL argument");
    if (nref < 1 || nref > IBO_KG_MAX_REF) return fail(IBO_ERR_ARG, "nref=%d outside [1, %d]", nref, IBO_KG_MAX_REF);
    if (M < 1) return fail(IBO_ERR_ARG, "M=%lld", (long long)M);
    if (!g->fitted) return fail(IBO_ERR_STATE, "knowledge gradient before a successful fit");
    for (size_t i = 0; i < (size_t)nref * g->D; i++)
        if (!(fabs(ref_host[i]) < HUGE_VAL)) return fail(IBO_ERR_ARG, "reference coordinate %zu is not finite", i);
    return IBO_OK;
}

// The pipeline's tail: the slopes against the reference rows, then the epigraph.
int kg_tail(KgState &st, int m, int mp, const double *cand, double *kg_out)
{
    RowPipeline &p = st.rows;
    const ibo_gp *g = p.g;
    hipStream_t s = g->stream;
    KgCrossArgs c;
    memset(&c, 0, sizeof(c));
    c.kp = g->kp; c.VtX = p.vt.p; c.ldx = (size_t)g->Npad; c.m = m; c.mp = mp; c.VtA = st.vtA.p; c.lda = (size_t)g->Npad; c.n = st.n; c.np = st.np;
    c.K = round_up(g->N, 32); c.X = cand; c.A = st.A.p; c.s2 = p.s2.p; c.B = p.cross.p; c.ldb = (size_t)st.np;
    KERNEL_TRY(launch_kg_cross(c, s));
    IBO_TRY(p.clock.mark(4));
    KgEpiArgs e;
    memset(&e, 0, sizeof(e));
    e.m = m; e.n = st.n; e.with_self = st.with_self; e.muA = st.muA.p; e.maxA = st.maxA; e.mu = p.mu.p; e.q = p.q.p; e.s2 = p.s2.p;
    e.B = p.cross.p; e.ldb = (size_t)st.np; e.kg = kg_out;
    KERNEL_TRY(launch_kg_epigraph(e, s));
    return p.clock.mark(5);
}

// The reference state; the device is idle when this returns.
int kg_begin(ibo_gp *g, KgState &st, int nref, const double *ref_host, int with_self, double clamp_lo)
{
    const int Np = g->Npad, D = g->D;
    hipStream_t s = g->stream;
    StageClock &clock = st.rows.clock;
    st.n = nref; st.np = round_up(nref, IBO_COV_TILE); st.with_self = with_self ? 1 : 0;
    IBO_TRY(st.rows.begin(g, clamp_lo, g_kg_chunk, (size_t)st.np, (size_t)st.np, true, g_kg_timing != 0, t_kg_ms));
    st.rows.tail = [&st](int m, int mp, const double *cand, double *out) { return kg_tail(st, m, mp, cand, out); };
    ScopedBuf<double> ktA;
    IBO_TRY(st.A.ensure((size_t)nref * D)); IBO_TRY(st.vtA.ensure((size_t)st.np * Np)); IBO_TRY(st.muA.ensure((size_t)st.np));
    IBO_TRY(ktA.ensure((size_t)st.np * Np));
    st.muA_host.resize((size_t)nref);
    IBO_TRY(clock.mark(0));
    HIP_TRY(hipMemcpyAsync(st.A.p, ref_host, sizeof(double) * (size_t)nref * D, hipMemcpyHostToDevice, s));
    IBO_TRY(vt_rows(g, st.A.p, nref, st.np, ktA.p, st.vtA.p, s));
    KgRowsArgs r = rows_args(g, ktA.p, st.vtA.p, st.A.p, nref, clamp_lo);
    r.mu = st.muA.p;
    KERNEL_TRY(launch_kg_rows(r, s));
    HIP_TRY(hipMemcpyAsync(st.muA_host.data(), st.muA.p, sizeof(double) * (size_t)nref, hipMemcpyDeviceToHost, s));
    IBO_TRY(clock.mark(1));
    HIP_TRY(hipStreamSynchronize(s));
    IBO_TRY(clock.account(0, 1, ST_STATE));
    st.maxA = st.muA_host[0];
    for (int i = 1; i < nref; i++) st.maxA = st.muA_host[i] > st.maxA ? st.muA_host[i] : st.maxA;
    return IBO_OK;
}

}  // namespace

extern "C" int ibo_kg_sweep(ibo_gp_t *g, int nref, const double *ref_host, int64_t M, const double *cand_dev, int with_self,
                            double clamp_lo, int64_t index_base, double *kg_dev, double *best_val, int64_t *best_idx)
{
    IBO_TRY(kg_check(g, nref, ref_host, cand_dev != nullptr, M));
    if (!kg_dev && !best_val && !best_idx) return fail(IBO_ERR_ARG, "every output is NULL");
    HIP_TRY(hipEventRecord(g->ev0, g->stream));
    KgState st;
    IBO_TRY(kg_begin(g, st, nref, ref_host, with_self, clamp_lo));
    return st.rows.sweep(M, cand_dev, index_base, kg_dev, best_val, best_idx);
}

extern "C" int ibo_kg_batch(ibo_gp_t *g, int nref, const double *ref_host, int64_t M, const double *Q_host, int with_self,
                            double clamp_lo, double *kg_host, double *mu_ref_host, double *mu_host, double *s2_host, double *b_host)
{
    IBO_TRY(kg_check(g, nref, ref_host, Q_host != nullptr, M));
    if (!kg_host && !mu_ref_host && !mu_host && !s2_host && !b_host) return fail(IBO_ERR_ARG, "every output is NULL");
    HIP_TRY(hipEventRecord(g->ev0, g->stream));
    KgState st;
    IBO_TRY(kg_begin(g, st, nref, ref_host, with_self, clamp_lo));
    if (mu_ref_host) memcpy(mu_ref_host, st.muA_host.data(), sizeof(double) * (size_t)nref);
    if (kg_host || mu_host || s2_host || b_host) IBO_TRY(st.rows.eval_host(M, Q_host, kg_host, mu_host, s2_host, b_host, (size_t)nref));
    return finish_span(g);
}

// direct_on_gp with the reference state kept on the device across the batches
extern "C" int ibo_kg_direct_max(ibo_gp_t *g, int nref, const double *ref_host, int D, const double *lb, const double *ub,
                                 int with_self, double clamp_lo, int maxiter, int maxtime, int maxsample, int compat,
                                 double *opt, double *optx, int64_t *nsamples)
{
    IBO_TRY(kg_check(g, nref, ref_host, lb && ub, 1));
    if (!opt && !optx && !nsamples) return fail(IBO_ERR_ARG, "every output is NULL");
    if (D != g->D) return fail(IBO_ERR_ARG, "bounds have %d dimensions, the model has %d", D, g->D);
    KgState st;
    IBO_TRY(kg_begin(g, st, nref, ref_host, with_self, clamp_lo));
    const ibo::batch_eval_t value = [&](const double *pts, int n, double *vals) -> int {
        return st.rows.eval_host(n, pts, vals, nullptr, nullptr, nullptr, 0);
    };
    char label[64];
    snprintf(label, sizeof(label), "knowledge-gradient DIRECT (%d reference points)", nref);
    return direct_maximize(value, label, D, lb, ub, maxiter, maxtime, maxsample, compat, opt, optx, nsamples);
}

extern "C" int ibo_kg_stage_ms(double *ms, int reset)
{
    return read_stage_sums(t_kg_ms, IBO_KG_STAGES, ms, reset);
}

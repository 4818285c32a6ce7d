// abi_kg.hip -- the knowledge gradient behind the C ABI: ibo_kg_sweep, ibo_kg_batch, ibo_kg_direct_max (kernels: kg.hip, cov.hip).
//
// ONE route for every entry: the reference state (the reference points, their V^T rows and posterior means) is built once per call and
// stays on the device; candidates go through kg_chunk in chunks of a multiple of 256 -- K* and V^T by cov.hip's launchers, the row
// kernel, the cross kernel, the epigraph kernel.  None of these lets a row's result depend on the rows beside it, so a candidate's bits
// are the same from a sweep, a host batch or a DIRECT batch, whatever the chunk.
//
// Scratch, all from the pool and handed back on every exit path: the reference state, 2 np Npad doubles while it is built and np Npad
// after (np = nref rounded up to 64: 168 MiB each at 20480 rows and 1024 points); per chunk K* and V^T (mc Npad doubles each) and the
// slopes (mc np doubles), each at most 256 MiB -- or 256 candidates where that alone is more -- and never more than 65280 candidates.
#include "abi_eval.h"
#include "cov.h"
#include "kg.h"

std::atomic<int> g_kg_chunk{0};       // ibo_set_option("kg_chunk", m): candidates per chunk (rounded up to 256); 0: by bytes
std::atomic<int> g_kg_timing{0};      // ibo_set_option("kg_timing", 1): HIP events around every stage, read with ibo_kg_stage_ms
static thread_local double t_kg_ms[IBO_KG_STAGES];

namespace {

enum { ST_REF = 0, ST_KSTAR, ST_TRI, ST_ROWS, ST_CROSS, ST_EPI };

struct KgState {
    ibo_gp *g = nullptr;
    int n = 0, np = 0, with_self = 0;
    double clamp_lo = 0.0, maxA = 0.0;
    int64_t mc = 0;                                  // candidates per chunk
    std::vector<double> muA_host;
    ScopedBuf<double> A, vtA, muA;                   // the reference state
    ScopedBuf<double> cand, kt, vt, mu, q, s2, B, kg;     // one chunk
    hipEvent_t ev[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    bool timing = false;
    ~KgState() { for (hipEvent_t e : ev) if (e) (void)hipEventDestroy(e); }
};

int kg_mark(KgState &st, int k) { if (st.timing) HIP_TRY(hipEventRecord(st.ev[k], st.g->stream)); return IBO_OK; }
// after a synchronisation: the time between marks k0 and k1 goes to stage `stage`
int kg_account(KgState &st, int k0, int k1, int stage)
{
    if (!st.timing) return IBO_OK;
    float ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms, st.ev[k0], st.ev[k1]));
    t_kg_ms[stage] += ms;
    return IBO_OK;
}

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

KgRowsArgs rows_args(const ibo_gp *g, const double *Kt, const double *Vt, const double *Q, int m, double clamp_lo)
{
    KgRowsArgs r;
    memset(&r, 0, sizeof(r));
    r.Kt = Kt; r.ldk = (size_t)g->Npad; r.Vt = Vt; r.ldv = (size_t)g->Npad;
    r.alphaY = g->alphaY.p; r.alpha1 = g->alpha1.p; r.Q = Q; r.D = g->D; r.prior = prior_of(g);
    r.N = g->N; r.K = g->N; r.m = m; r.noise = g->noise; r.clamp_lo = clamp_lo;
    return r;
}

// The reference state; the device is idle when this returns.
int kg_begin(ibo_gp *g, KgState &st, int nref, const double *ref_host, int with_self, double clamp_lo)
{
    const int Np = g->Npad, D = g->D;
    hipStream_t s = g->stream;
    st.g = g; st.n = nref; st.np = round_up(nref, IBO_COV_TILE); st.with_self = with_self ? 1 : 0; st.clamp_lo = clamp_lo;
    st.timing = g_kg_timing != 0;
    if (st.timing)
        for (hipEvent_t &e : st.ev) HIP_TRY(hipEventCreate(&e));
    const size_t lim = (size_t)256 << 20;
    int64_t mc = g_kg_chunk > 0 ? (int64_t)g_kg_chunk : (int64_t)std::min(lim / ((size_t)Np * sizeof(double)), lim / ((size_t)st.np * sizeof(double)));
    st.mc = std::min<int64_t>(std::max<int64_t>((mc + (g_kg_chunk > 0 ? 255 : 0)) / 256 * 256, 256), 65280);      // (cov_kstar_kernel: one grid row per point, at most 65535)
    ScopedBuf<double> ktA;
    IBO_TRY(st.A.ensure((size_t)nref * D)); IBO_TRY(st.vtA.ensure((size_t)st.np * Np)); IBO_TRY(st.muA.ensure((size_t)st.np));
    IBO_TRY(ktA.ensure((size_t)st.np * Np));
    st.muA_host.resize((size_t)nref);
    IBO_TRY(kg_mark(st, 0));
    HIP_TRY(hipMemcpyAsync(st.A.p, ref_host, sizeof(double) * (size_t)nref * D, hipMemcpyHostToDevice, s));
    IBO_TRY(vt_rows(g, st.A.p, nref, st.np, ktA.p, st.vtA.p, s));
    KgRowsArgs r = rows_args(g, ktA.p, st.vtA.p, st.A.p, nref, clamp_lo);
    r.mu = st.muA.p;
    KERNEL_TRY(launch_kg_rows(r, s));
    HIP_TRY(hipMemcpyAsync(st.muA_host.data(), st.muA.p, sizeof(double) * (size_t)nref, hipMemcpyDeviceToHost, s));
    IBO_TRY(kg_mark(st, 1));
    HIP_TRY(hipStreamSynchronize(s));
    IBO_TRY(kg_account(st, 0, 1, ST_REF));
    st.maxA = st.muA_host[0];
    for (int i = 1; i < nref; i++) st.maxA = st.muA_host[i] > st.maxA ? st.muA_host[i] : st.maxA;
    return IBO_OK;
}

// room for chunks of up to m candidates (the device is idle: a larger buffer replaces a smaller one)
int kg_reserve(KgState &st, int64_t m, bool need_cand, bool need_kg)
{
    const size_t mp = (size_t)round_up((int)std::min(m, st.mc), IBO_COV_TILE), Np = (size_t)st.g->Npad;
    if (need_cand) IBO_TRY(st.cand.ensure(mp * st.g->D));
    if (need_kg) IBO_TRY(st.kg.ensure(mp));
    IBO_TRY(st.kt.ensure(mp * Np)); IBO_TRY(st.vt.ensure(mp * Np)); IBO_TRY(st.B.ensure(mp * st.np));
    IBO_TRY(st.mu.ensure(mp)); IBO_TRY(st.q.ensure(mp)); IBO_TRY(st.s2.ensure(mp));
    return IBO_OK;
}

// One chunk: m <= st.mc candidates at cand (device, m x D) -> kg_out (device, m); the per-candidate pieces stay in st.mu / s2 / q / B.
// Nothing is waited for unless the stages are being timed.
int kg_chunk(KgState &st, int m, const double *cand, double *kg_out)
{
    ibo_gp *g = st.g;
    const int N = g->N, Np = g->Npad, mp = round_up(m, IBO_COV_TILE);
    hipStream_t s = g->stream;
    IBO_TRY(kg_mark(st, 0));
    KERNEL_TRY(launch_cov_kstar(g->kp, g->Xp.p, N, Np, g->DP, cand, m, mp, st.kt.p, s));
    IBO_TRY(kg_mark(st, 1));
    KERNEL_TRY(launch_cov_tri(st.kt.p, (size_t)Np, g->W.p, (size_t)Np, N, mp, Np, st.vt.p, (size_t)Np, s));
    IBO_TRY(kg_mark(st, 2));
    KgRowsArgs r = rows_args(g, st.kt.p, st.vt.p, cand, m, st.clamp_lo);
    r.mu = st.mu.p; r.q = st.q.p; r.s2 = st.s2.p;
    KERNEL_TRY(launch_kg_rows(r, s));
    IBO_TRY(kg_mark(st, 3));
    KgCrossArgs c;
    memset(&c, 0, sizeof(c));
    c.kp = g->kp; c.VtX = st.vt.p; c.ldx = (size_t)Np; c.m = m; c.mp = mp; c.VtA = st.vtA.p; c.lda = (size_t)Np; c.n = st.n; c.np = st.np;
    c.K = round_up(N, 32); c.X = cand; c.A = st.A.p; c.s2 = st.s2.p; c.B = st.B.p; c.ldb = (size_t)st.np;
    KERNEL_TRY(launch_kg_cross(c, s));
    IBO_TRY(kg_mark(st, 4));
    KgEpiArgs e;
    memset(&e, 0, sizeof(e));
    e.m = m; e.n = st.n; e.with_self = st.with_self; e.muA = st.muA.p; e.maxA = st.maxA; e.mu = st.mu.p; e.q = st.q.p; e.s2 = st.s2.p;
    e.B = st.B.p; e.ldb = (size_t)st.np; e.kg = kg_out;
    KERNEL_TRY(launch_kg_epigraph(e, s));
    IBO_TRY(kg_mark(st, 5));
    if (st.timing) {
        HIP_TRY(hipStreamSynchronize(s));
        for (int k = 0; k < 5; k++) IBO_TRY(kg_account(st, k, k + 1, ST_KSTAR + k));
    }
    return IBO_OK;
}

// Host points in chunks: upload, kg_chunk, read back what is asked for (any of the outputs may be NULL).  The device is idle on return.
int kg_eval_host(KgState &st, int64_t M, const double *Q_host, double *kg_host, double *mu_host, double *s2_host, double *b_host)
{
    ibo_gp *g = st.g;
    const size_t D = (size_t)g->D, n = (size_t)st.n;
    hipStream_t s = g->stream;
    IBO_TRY(kg_reserve(st, M, true, true));
    for (int64_t c0 = 0; c0 < M; c0 += st.mc) {
        const int m = (int)std::min(M - c0, st.mc);
        HIP_TRY(hipMemcpyAsync(st.cand.p, Q_host + (size_t)c0 * D, sizeof(double) * m * D, hipMemcpyHostToDevice, s));
        IBO_TRY(kg_chunk(st, m, st.cand.p, st.kg.p));
        if (kg_host) HIP_TRY(hipMemcpyAsync(kg_host + c0, st.kg.p, sizeof(double) * m, hipMemcpyDeviceToHost, s));
        if (mu_host) HIP_TRY(hipMemcpyAsync(mu_host + c0, st.mu.p, sizeof(double) * m, hipMemcpyDeviceToHost, s));
        if (s2_host) HIP_TRY(hipMemcpyAsync(s2_host + c0, st.s2.p, sizeof(double) * m, hipMemcpyDeviceToHost, s));
        if (b_host) HIP_TRY(hipMemcpy2DAsync(b_host + (size_t)c0 * n, sizeof(double) * n, st.B.p, sizeof(double) * st.np, sizeof(double) * n,
                                             (size_t)m, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
    }
    return IBO_OK;
}

}  // namespace

extern "C" int ibo_kg_sweep(ibo_gp_t *g, int nref, const double *ref_host, int64_t M, const double *cand_dev, int with_self,
                            double clamp_lo, int64_t index_base, double *kg_dev, double *best_val, int64_t *best_idx)
{
    IBO_TRY(kg_check(g, nref, ref_host, cand_dev != nullptr, M));
    if (!kg_dev && !best_val && !best_idx) return fail(IBO_ERR_ARG, "every output is NULL");
    hipStream_t s = g->stream;
    const int D = g->D;
    HIP_TRY(hipEventRecord(g->ev0, s));
    KgState st;
    IBO_TRY(kg_begin(g, st, nref, ref_host, with_self, clamp_lo));
    IBO_TRY(kg_reserve(st, M, false, kg_dev == nullptr));
    const int64_t nblk = (M + 255) / 256;
    ScopedBuf<double> pv;
    ScopedBuf<int64_t> pi;
    const bool want_best = best_val || best_idx;
    if (want_best) { IBO_TRY(pv.ensure((size_t)nblk)); IBO_TRY(pi.ensure((size_t)nblk)); }
    for (int64_t c0 = 0; c0 < M; c0 += st.mc) {            // (one stream: a chunk's kernels start after the last chunk's have read the scratch)
        const int m = (int)std::min(M - c0, st.mc);
        double *out = kg_dev ? kg_dev + c0 : st.kg.p;
        IBO_TRY(kg_chunk(st, m, cand_dev + (size_t)c0 * D, out));
        if (want_best) KERNEL_TRY(launch_kg_argmax(out, m, c0, index_base, pv.p + c0 / 256, pi.p + c0 / 256, s));
    }
    if (want_best) IBO_TRY(argmax_readback(g, pv.p, pi.p, nblk, best_val, best_idx));
    return finish_span(g);                                      // (waits for the stream: the scratch goes back to the pool after it)
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
    if (kg_host || mu_host || s2_host || b_host) IBO_TRY(kg_eval_host(st, M, Q_host, kg_host, mu_host, s2_host, b_host));
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
        return kg_eval_host(st, n, pts, vals, nullptr, nullptr, nullptr);
    };
    char label[64];
    snprintf(label, sizeof(label), "knowledge-gradient DIRECT (%d reference points)", nref);
    return direct_maximize(value, label, D, lb, ub, maxiter, maxtime, maxsample, compat, opt, optx, nsamples);
}

extern "C" int ibo_kg_stage_ms(double *ms, int reset)
{
    if (ms) memcpy(ms, t_kg_ms, sizeof(t_kg_ms));
    if (reset) memset(t_kg_ms, 0, sizeof(t_kg_ms));
    return IBO_OK;
}

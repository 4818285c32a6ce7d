// abi_paths.hip -- pathwise posterior draws behind the C ABI: ibo_paths_create / destroy / info / coef / sweep / batch / grad_batch / direct_max
// (kernels: paths.hip; V = U W^T by cov.hip's triangular launcher).
//
// A path object is a SNAPSHOT on the device: the model's rows, kernel parameters, prior arrays, the spectral draws and the coefficient
// block, its own stream and scratch.  Nothing in it points back at the model it was drawn from.
// ONE route for every entry: paths_run launches paths_tile_kernel over chunks of a multiple of 256 candidates.  The kernel lets no
// candidate's value depend on the rows beside it, so the bits are the same from a sweep, a host batch or a DIRECT batch, in any chunk.
#include "abi_eval.h"
#include "cov.h"
#include "paths.h"

std::atomic<int> g_paths_chunk{0};    // ibo_set_option("paths_chunk", m): candidates per chunk (rounded up to 256); 0: 2^21

struct ibo_paths {
    int device = 0, N = 0, D = 0, ldx = 0, F = 0, Fp = 0, Np32 = 0, S = 0, Sp = 0, pt = 64, nb = 0;
    KParams kp;
    double amp = 0.0, ptheta = 0.0;
    hipStream_t stream = nullptr;
    DevBuf<double> X, omega, phase, coef, pmeans, pbeta, plowerb, pwidth;
    DevBuf<double> cand, vals, pv, resv;              // scratch of the evaluation entries, kept between calls (DIRECT's many batches)
    DevBuf<int64_t> pi, resi;
    DevBuf<double> grad, pick;                        // ibo_paths_grad_batch: a chunk's gradients, its values picked by path_of
    DevBuf<int> pof;
};

namespace {

void paths_free(ibo_paths *p)
{
    (void)hipSetDevice(p->device);
    (void)hipDeviceSynchronize();
    g_pool_quiet = true;
    p->X.release(); p->omega.release(); p->phase.release(); p->coef.release(); p->pmeans.release(); p->pbeta.release(); p->plowerb.release();
    p->pwidth.release(); p->cand.release(); p->vals.release(); p->pv.release(); p->resv.release(); p->pi.release(); p->resi.release();
    p->grad.release(); p->pick.release(); p->pof.release();
    g_pool_quiet = false;
    if (p->stream) (void)hipStreamDestroy(p->stream);
    delete p;
}

PathsArgs paths_args(const ibo_paths *p)
{
    PathsArgs a;
    memset(&a, 0, sizeof(a));
    a.kp = p->kp; a.X = p->X.p; a.ldx = p->ldx; a.N = p->N; a.omega = p->omega.p; a.phase = p->phase.p; a.F = p->F; a.Fp = p->Fp; a.amp = p->amp;
    a.coef = p->coef.p; a.Sp = p->Sp; a.kend = p->Fp + p->Np32; a.pt = p->pt; a.S = p->S; a.only = -1; a.ldc = p->D;
    a.prior.nb = p->nb; a.prior.theta = p->ptheta; a.prior.means = p->pmeans.p; a.prior.beta = p->pbeta.p; a.prior.lowerb = p->plowerb.p;
    a.prior.width = p->pwidth.p;
    return a;
}

int64_t paths_chunk_len()
{
    const int64_t c = g_paths_chunk > 0 ? ((int64_t)g_paths_chunk + 255) / 256 * 256 : (int64_t)1 << 21;
    return std::min<int64_t>(c, (int64_t)1 << 21);              // (one grid row per 64 candidates, at most 65535)
}

// M candidates on the device through the tile kernel in chunks; a carries the outputs (values / ldv / voff for candidate 0, the partials)
int paths_run(ibo_paths *p, PathsArgs a, int64_t M, const double *cand_dev)
{
    const int64_t mc = paths_chunk_len(), voff = a.voff;
    for (int64_t c0 = 0; c0 < M; c0 += mc) {
        a.m = (int)std::min(M - c0, mc); a.cand = cand_dev + (size_t)c0 * p->D; a.first = c0; a.voff = voff + c0;
        KERNEL_TRY(launch_paths_tile(a, p->stream));
    }
    return IBO_OK;
}

// host points -> host values (S x M, or M for one path): upload, run, read back, in pieces of at most mb points
int paths_eval_host(ibo_paths *p, int64_t M, const double *Q_host, int only, double *values_host)
{
    const int rows = only >= 0 ? 1 : p->S;
    const int64_t mb = std::min<int64_t>(M, std::max<int64_t>(256, ((int64_t)1 << 24) / rows));
    IBO_TRY(p->cand.ensure((size_t)mb * p->D)); IBO_TRY(p->vals.ensure((size_t)mb * rows));
    for (int64_t c0 = 0; c0 < M; c0 += mb) {
        const int64_t m = std::min(M - c0, mb);
        HIP_TRY(hipMemcpyAsync(p->cand.p, Q_host + (size_t)c0 * p->D, sizeof(double) * (size_t)m * p->D, hipMemcpyHostToDevice, p->stream));
        PathsArgs a = paths_args(p);
        a.only = only; a.values = p->vals.p; a.ldv = (size_t)mb;
        IBO_TRY(paths_run(p, a, m, p->cand.p));
        HIP_TRY(hipMemcpy2DAsync(values_host + c0, sizeof(double) * (size_t)M, p->vals.p, sizeof(double) * (size_t)mb, sizeof(double) * (size_t)m,
                                 (size_t)rows, hipMemcpyDeviceToHost, p->stream));
        HIP_TRY(hipStreamSynchronize(p->stream));
    }
    return IBO_OK;
}

}  // namespace

extern "C" int ibo_paths_create(ibo_gp_t *g, int nfeat, const double *omega_host, const double *phase_host, int npaths,
                                const double *w_host, const double *eps_host, ibo_paths_t **out)
{
    IBO_TRY(use_device(g ? g->device : 0));
    if (!g || !omega_host || !phase_host || !w_host || !eps_host || !out) return fail(IBO_ERR_ARG, "NULL argument");
    if (nfeat < 1 || nfeat > IBO_PATHS_MAX_FEATURES) return fail(IBO_ERR_ARG, "nfeat=%d outside [1, %d]", nfeat, IBO_PATHS_MAX_FEATURES);
    if (npaths < 1 || npaths > IBO_PATHS_MAX_PATHS) return fail(IBO_ERR_ARG, "npaths=%d outside [1, %d]", npaths, IBO_PATHS_MAX_PATHS);
    if (!g->fitted) return fail(IBO_ERR_STATE, "paths before a successful fit");
    if (g->reversed) return fail(IBO_ERR_STATE, "paths on a model fitted from libego's inverse");
    const int N = g->N, D = g->D, Np = g->Npad, F = nfeat, S = npaths;
    ibo_paths *p = new ibo_paths();
    struct Guard { ibo_paths *p; ~Guard() { if (p) paths_free(p); } } guard{p};
    p->device = g->device; p->N = N; p->D = D; p->ldx = g->DP; p->F = F; p->Fp = round_up(F, PT_KB); p->Np32 = round_up(N, PT_KB); p->S = S;
    p->nb = g->nb; p->ptheta = g->ptheta; p->pt = g->nb > 0 ? 63 : 64; p->Sp = (S + p->pt - 1) / p->pt * 64;
    p->kp = g->kp; p->amp = sqrt(2.0 * g->kp.sf2 / F);
    HIP_TRY(hipStreamCreate(&p->stream));
    const size_t K = (size_t)p->Fp + p->Np32, Sp = (size_t)p->Sp;
    IBO_TRY(p->X.ensure((size_t)N * g->DP)); IBO_TRY(p->omega.ensure((size_t)p->Fp * D)); IBO_TRY(p->phase.ensure((size_t)p->Fp));
    IBO_TRY(p->coef.ensure(K * Sp));
    hipStream_t s = g->stream;                        // (the model's stream: its fit and its prior upload are ordered before this)
    HIP_TRY(hipMemcpyAsync(p->X.p, g->Xp.p, sizeof(double) * (size_t)N * g->DP, hipMemcpyDeviceToDevice, s));
    if (g->nb > 0) {
        IBO_TRY(p->pmeans.ensure((size_t)g->nb * D)); IBO_TRY(p->pbeta.ensure((size_t)g->nb)); IBO_TRY(p->plowerb.ensure((size_t)D)); IBO_TRY(p->pwidth.ensure((size_t)D));
        HIP_TRY(hipMemcpyAsync(p->pmeans.p, g->pmeans.p, sizeof(double) * (size_t)g->nb * D, hipMemcpyDeviceToDevice, s));
        HIP_TRY(hipMemcpyAsync(p->pbeta.p, g->pbeta.p, sizeof(double) * (size_t)g->nb, hipMemcpyDeviceToDevice, s));
        HIP_TRY(hipMemcpyAsync(p->plowerb.p, g->plowerb.p, sizeof(double) * (size_t)D, hipMemcpyDeviceToDevice, s));
        HIP_TRY(hipMemcpyAsync(p->pwidth.p, g->pwidth.p, sizeof(double) * (size_t)D, hipMemcpyDeviceToDevice, s));
    }
    // the feature rows of the coefficient block (w transposed into the column layout), the padded spectral draws
    std::vector<double> hc((size_t)p->Fp * Sp, 0.0), ho((size_t)p->Fp * D, 0.0), hp((size_t)p->Fp, 0.0);
    for (int sI = 0; sI < S; sI++) {
        const int col = paths_col(sI, p->pt);
        for (int k = 0; k < F; k++) hc[(size_t)k * Sp + col] = w_host[(size_t)sI * F + k];
    }
    memcpy(ho.data(), omega_host, sizeof(double) * (size_t)F * D);
    memcpy(hp.data(), phase_host, sizeof(double) * (size_t)F);
    HIP_TRY(hipMemsetAsync(p->coef.p, 0, sizeof(double) * K * Sp, s));
    HIP_TRY(hipMemcpyAsync(p->coef.p, hc.data(), sizeof(double) * hc.size(), hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(p->omega.p, ho.data(), sizeof(double) * ho.size(), hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(p->phase.p, hp.data(), sizeof(double) * hp.size(), hipMemcpyHostToDevice, s));
    // U = eps + Phi(X) w (rows of paths, Npad wide, zero padded), Y = U W^T, coef = aY - W^T y
    const int S64 = round_up(S, IBO_COV_TILE);
    ScopedBuf<double> U, Y;
    IBO_TRY(U.ensure((size_t)S64 * Np)); IBO_TRY(Y.ensure((size_t)S64 * Np));
    HIP_TRY(hipMemsetAsync(U.p, 0, sizeof(double) * (size_t)S64 * Np, s));
    HIP_TRY(hipMemcpy2DAsync(U.p, sizeof(double) * (size_t)Np, eps_host, sizeof(double) * (size_t)N, sizeof(double) * (size_t)N, (size_t)S,
                             hipMemcpyHostToDevice, s));
    PathsArgs a = paths_args(p);
    a.kend = p->Fp; a.prior.nb = 0; a.cand = p->X.p; a.ldc = p->ldx; a.m = N; a.values = U.p; a.ldv = (size_t)Np; a.accumulate = 1;
    KERNEL_TRY(launch_paths_tile(a, s));
    KERNEL_TRY(launch_cov_tri(U.p, (size_t)Np, g->W.p, (size_t)Np, N, S64, Np, Y.p, (size_t)Np, s));
    KERNEL_TRY(launch_paths_solve(g->W.p, Np, N, Y.p, (size_t)Np, S, p->pt, g->alphaY.p, g->alpha1.p, p->coef.p, p->Sp, p->Fp, s));
    HIP_TRY(hipStreamSynchronize(s));
    guard.p = nullptr;
    *out = p;
    return IBO_OK;
}

extern "C" int ibo_paths_destroy(ibo_paths_t *p)
{
    IBO_TRY(use_device(p ? p->device : 0));
    if (p) paths_free(p);
    return IBO_OK;
}

extern "C" int ibo_paths_info(ibo_paths_t *p, int *npaths, int *nfeat, int *N, int *D, int *device)
{
    IBO_TRY(use_device(p ? p->device : 0));
    if (!p) return fail(IBO_ERR_ARG, "NULL argument");
    if (npaths) *npaths = p->S;
    if (nfeat) *nfeat = p->F;
    if (N) *N = p->N;
    if (D) *D = p->D;
    if (device) *device = p->device;
    return IBO_OK;
}

extern "C" int ibo_paths_coef(ibo_paths_t *p, double *coef_host)
{
    IBO_TRY(use_device(p ? p->device : 0));
    if (!p || !coef_host) return fail(IBO_ERR_ARG, "NULL argument");
    const size_t K = (size_t)p->Fp + p->Np32, Sp = (size_t)p->Sp, F = (size_t)p->F, N = (size_t)p->N;
    std::vector<double> h(K * Sp);
    HIP_TRY(hipMemcpyAsync(h.data(), p->coef.p, sizeof(double) * K * Sp, hipMemcpyDeviceToHost, p->stream));
    HIP_TRY(hipStreamSynchronize(p->stream));
    for (int s = 0; s < p->S; s++) {
        const int col = paths_col(s, p->pt);
        double *o = coef_host + (size_t)s * (F + N);
        for (size_t k = 0; k < F; k++) o[k] = h[k * Sp + col];
        for (size_t i = 0; i < N; i++) o[F + i] = h[((size_t)p->Fp + i) * Sp + col];
    }
    return IBO_OK;
}

extern "C" int ibo_paths_sweep(ibo_paths_t *p, int64_t M, const double *cand_dev, int64_t index_base, double *values_dev,
                               double *best_val, int64_t *best_idx)
{
    IBO_TRY(use_device(p ? p->device : 0));
    if (!p || !cand_dev) return fail(IBO_ERR_ARG, "NULL argument");
    if (M < 1) return fail(IBO_ERR_ARG, "M=%lld", (long long)M);
    if (!values_dev && !best_val && !best_idx) return fail(IBO_ERR_ARG, "every output is NULL");
    const bool want_best = best_val || best_idx;
    const int64_t nblk = (M + 63) / 64;
    PathsArgs a = paths_args(p);
    a.values = values_dev; a.ldv = (size_t)M; a.index_base = index_base;
    if (want_best) {
        IBO_TRY(p->pv.ensure((size_t)nblk * p->S)); IBO_TRY(p->pi.ensure((size_t)nblk * p->S));
        IBO_TRY(p->resv.ensure((size_t)p->S)); IBO_TRY(p->resi.ensure((size_t)p->S));
        a.part_val = p->pv.p; a.part_idx = p->pi.p; a.nblk = nblk;
    }
    IBO_TRY(paths_run(p, a, M, cand_dev));
    if (want_best) {
        KERNEL_TRY(launch_paths_final(p->pv.p, p->pi.p, nblk, p->S, p->resv.p, p->resi.p, p->stream));
        if (best_val) HIP_TRY(hipMemcpyAsync(best_val, p->resv.p, sizeof(double) * (size_t)p->S, hipMemcpyDeviceToHost, p->stream));
        if (best_idx) HIP_TRY(hipMemcpyAsync(best_idx, p->resi.p, sizeof(int64_t) * (size_t)p->S, hipMemcpyDeviceToHost, p->stream));
    }
    HIP_TRY(hipStreamSynchronize(p->stream));
    if (best_idx)
        for (int s = 0; s < p->S; s++) if (best_idx[s] == INT64_MAX) best_idx[s] = -1;        // (nothing admissible: no base added)
    return IBO_OK;
}

extern "C" int ibo_paths_batch(ibo_paths_t *p, int64_t M, const double *Q_host, double *values_host)
{
    IBO_TRY(use_device(p ? p->device : 0));
    if (!p || !Q_host || !values_host) return fail(IBO_ERR_ARG, "NULL argument");
    if (M < 1) return fail(IBO_ERR_ARG, "M=%lld", (long long)M);
    return paths_eval_host(p, M, Q_host, -1, values_host);
}

extern "C" int ibo_paths_grad_batch(ibo_paths_t *p, int64_t M, const double *Q_host, const int *path_of, double *values_host,
                                    double *grads_host)
{
    IBO_TRY(use_device(p ? p->device : 0));
    if (!p || !Q_host || !grads_host) return fail(IBO_ERR_ARG, "NULL argument");
    if (M < 1) return fail(IBO_ERR_ARG, "M=%lld", (long long)M);
    if (path_of)
        for (int64_t i = 0; i < M; i++)
            if (path_of[i] < 0 || path_of[i] >= p->S) return fail(IBO_ERR_ARG, "path_of[%lld]=%d outside [0, %d)", (long long)i, path_of[i], p->S);
    const size_t D = (size_t)p->D, S = (size_t)p->S, rows = path_of ? 1 : S;
    // pieces by bytes (2^24 doubles of values and gradients) and by "paths_chunk": a point's bits do not depend on its piece
    const int64_t mb = std::min<int64_t>(std::min(M, paths_chunk_len()), std::max<int64_t>(256, ((int64_t)1 << 24) / (int64_t)(S * (D + 1))));
    IBO_TRY(p->cand.ensure((size_t)mb * D)); IBO_TRY(p->grad.ensure(rows * (size_t)mb * D));
    if (values_host) IBO_TRY(p->vals.ensure(S * (size_t)mb));
    if (path_of) { IBO_TRY(p->pof.ensure((size_t)mb)); if (values_host) IBO_TRY(p->pick.ensure((size_t)mb)); }
    for (int64_t c0 = 0; c0 < M; c0 += mb) {
        const int64_t m = std::min(M - c0, mb);
        HIP_TRY(hipMemcpyAsync(p->cand.p, Q_host + (size_t)c0 * D, sizeof(double) * (size_t)m * D, hipMemcpyHostToDevice, p->stream));
        if (path_of) HIP_TRY(hipMemcpyAsync(p->pof.p, path_of + c0, sizeof(int) * (size_t)m, hipMemcpyHostToDevice, p->stream));
        PathsGradArgs ga;
        ga.a = paths_args(p);
        if (values_host) {                            // paths_tile_kernel itself: the bits of ibo_paths_batch
            PathsArgs a = ga.a;
            a.values = p->vals.p; a.ldv = (size_t)mb;
            IBO_TRY(paths_run(p, a, m, p->cand.p));
            if (path_of) {
                KERNEL_TRY(launch_paths_pick(p->vals.p, (size_t)mb, p->pof.p, (int)m, p->pick.p, p->stream));
                HIP_TRY(hipMemcpyAsync(values_host + c0, p->pick.p, sizeof(double) * (size_t)m, hipMemcpyDeviceToHost, p->stream));
            } else {
                HIP_TRY(hipMemcpy2DAsync(values_host + c0, sizeof(double) * (size_t)M, p->vals.p, sizeof(double) * (size_t)mb,
                                         sizeof(double) * (size_t)m, S, hipMemcpyDeviceToHost, p->stream));
            }
        }
        ga.a.cand = p->cand.p; ga.a.m = (int)m;
        ga.path_of = path_of ? p->pof.p : nullptr; ga.grads = p->grad.p; ga.ldg = (size_t)mb; ga.goff = 0;
        KERNEL_TRY(launch_paths_grad_tile(ga, p->stream));
        HIP_TRY(hipMemcpy2DAsync(grads_host + (size_t)c0 * D, sizeof(double) * (size_t)M * D, p->grad.p, sizeof(double) * (size_t)mb * D,
                                 sizeof(double) * (size_t)m * D, rows, hipMemcpyDeviceToHost, p->stream));
        HIP_TRY(hipStreamSynchronize(p->stream));
    }
    return IBO_OK;
}

extern "C" int ibo_paths_direct_max(ibo_paths_t *p, int path, int D, const double *lb, const double *ub, int maxiter, int maxtime,
                                    int maxsample, int compat, double *opt, double *optx, int64_t *nsamples)
{
    IBO_TRY(use_device(p ? p->device : 0));
    if (!p || !lb || !ub) return fail(IBO_ERR_ARG, "NULL argument");
    if (!opt && !optx && !nsamples) return fail(IBO_ERR_ARG, "every output is NULL");
    if (path < 0 || path >= p->S) return fail(IBO_ERR_ARG, "path=%d outside [0, %d)", path, p->S);
    if (D != p->D) return fail(IBO_ERR_ARG, "bounds have %d dimensions, the paths have %d", D, p->D);
    const ibo::batch_eval_t value = [&](const double *pts, int n, double *vals) -> int { return paths_eval_host(p, n, pts, path, vals); };
    char label[64];
    snprintf(label, sizeof(label), "posterior-path DIRECT (path %d of %d)", path, p->S);
    return direct_maximize(value, label, D, lb, ub, maxiter, maxtime, maxsample, compat, opt, optx, nsamples);
}

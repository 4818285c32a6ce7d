// abi_pref.hip -- the preference GP's device steps behind the C ABI (ibo_pref_*); the final model ends in the fit's own fit_factor (abi_fit.hip).
// PrefGaussianProcess.addPreferences (ego/gaussianprocess/__init__.py:347-498) minimises
//     S(y) = -sum_pairs (d + 1) log Phi((y_v - y_u)/sqrt 2) + y^T R^-1 y / 2
// and then factors R + C^-1.  The O(pairs) terms (Phi, its derivatives, the line search) stay with the host; every
// N x N object -- R^-1 = W^T W, the Hessian R^-1 + sum rho (e_v - e_u)(e_v - e_u)^T and its factorisation, C, C^-1,
// R + C^-1 -- lives on the device, and only vectors and the pairs' distinct matrix entries cross the bus.
#include "abi_factor.h"

static int pref_alloc(ibo_gp *g)
{
    const int Np = g->Npad;
    const size_t nn = (size_t)Np * Np;
    auto &pw = g->pw;
    IBO_TRY(pw.Rinv.ensure(nn)); IBO_TRY(pw.A.ensure(nn)); IBO_TRY(pw.Lh.ensure(nn)); IBO_TRY(pw.E.ensure(nn));
    IBO_TRY(pw.Et.ensure(nn)); IBO_TRY(pw.d64.ensure(diag64_size(Np))); IBO_TRY(pw.vec.ensure(4 * (size_t)Np));
    IBO_TRY(pw.tmp.ensure(alpha_scratch(Np))); IBO_TRY(pw.info.ensure(1));
    return IBO_OK;
}
// pw.A (N x N in an identity-padded Npad x Npad frame; destroyed) -> pw.E = the inverse of its Cholesky factor, pad rows zero.  Et is
// scratch afterwards (the callers' launch_wtw).  Synchronises.
static int pref_factor(ibo_gp *g, int *info)
{
    auto &pw = g->pw;
    FactorRoute route;
    IBO_TRY(factor_route(g->Npad, FACTOR_PREF, &route));
    FactorBufs b = {};
    b.A = pw.A.p; b.L = pw.Lh.p; b.Pk = pw.Lh.p;        // Lh: the factor on the ride-along, lent as the packed-update store in place
    b.eye = pw.E.p; b.Et = pw.Et.p; b.W = pw.E.p; b.d64 = pw.d64.p; b.info = pw.info.p;
    IBO_TRY(factor_invert(route, g->N, g->Npad, b, g->stream));
    return factor_info(pw.info.p, g->stream, "matrix", info);
}
static int pref_sparse(ibo_gp *g, int nnz, const int64_t *lin_host, const double *val_host)
{
    auto &pw = g->pw;
    if (nnz < 0 || (nnz > 0 && (!lin_host || !val_host))) return fail(IBO_ERR_ARG, "bad sparse term");
    for (int e = 0; e < nnz; e++)
        if (lin_host[e] < 0 || lin_host[e] >= (int64_t)g->N * g->N) return fail(IBO_ERR_ARG, "matrix entry %d out of range", e);
    if (nnz == 0) return IBO_OK;
    IBO_TRY(pw.lin.ensure(nnz)); IBO_TRY(pw.val.ensure(nnz));
    HIP_TRY(hipMemcpyAsync(pw.lin.p, lin_host, sizeof(int64_t) * nnz, hipMemcpyHostToDevice, g->stream));
    HIP_TRY(hipMemcpyAsync(pw.val.p, val_host, sizeof(double) * nnz, hipMemcpyHostToDevice, g->stream));
    return IBO_OK;
}

extern "C" int ibo_pref_begin(ibo_gp_t *g)
{
    if (!g) return fail(IBO_ERR_ARG, "gp is NULL");
    if (!g->fitted || !g->plain_fit || g->reversed) return fail(IBO_ERR_STATE, "ibo_pref_begin needs a plain fitted model (L = chol(R))");
    IBO_TRY(use_device(g->device));
    IBO_TRY(pref_alloc(g));
    KERNEL_TRY(launch_wtw(g->W.p, g->pw.Et.p, g->pw.Rinv.p, g->Npad, g->stream));       // R^-1 = W^T W (zero on the pad)
    g->pw.ready = true; g->pw.epoch = g->fit_epoch; g->pw.N = g->N; g->pw.Npad = g->Npad;
    return IBO_OK;
}

// The workspace belongs to the model ibo_pref_begin ran on: R^-1 = W^T W is that model's, and every buffer is sized by its Npad.  fit_epoch
// moves with every fit and every removal; an extension keeps it (a kept sweep state survives one) but changes N.  Both callers of stage_data,
// the only place that moves Npad, clear pw.ready before they restage (a fit that then FAILS leaves another N and Npad under the old epoch), so
// ready, epoch and N already decide; Npad is compared all the same, belt and braces, because it is what sizes every buffer written here and
// ibo_pref_finish cannot ask for `fitted` instead (its own IBO_ERR_NOT_PD leaves the handle unfitted, and the caller's retry with a larger
// diag must still be accepted).
static bool pref_owned(const ibo_gp *g)
{
    return g->pw.ready && g->pw.epoch == g->fit_epoch && g->pw.N == g->N && g->pw.Npad == g->Npad;
}

static int pref_check(ibo_gp *g)
{
    if (!g) return fail(IBO_ERR_ARG, "gp is NULL");
    if (!pref_owned(g) || !g->fitted || !g->plain_fit)
        return fail(IBO_ERR_STATE, "no ibo_pref_begin since this model was last fitted, extended or reduced");
    return use_device(g->device);
}

extern "C" int ibo_pref_rinv_mul(ibo_gp_t *g, const double *y_host, double *out_host)
{
    IBO_TRY(pref_check(g));
    if (!y_host || !out_host) return fail(IBO_ERR_ARG, "NULL argument");
    auto &pw = g->pw;
    const int N = g->N, Np = g->Npad;
    hipStream_t s = g->stream;
    std::vector<double> yp(Np, 0.0);
    for (int i = 0; i < N; i++) yp[i] = y_host[i];
    HIP_TRY(hipMemcpyAsync(pw.vec.p, yp.data(), sizeof(double) * Np, hipMemcpyHostToDevice, s));
    KERNEL_TRY(launch_alpha(g->W.p, N, Np, pw.vec.p, pw.tmp.p, pw.vec.p + Np, pw.vec.p + 2 * (size_t)Np, s));
    HIP_TRY(hipMemcpyAsync(out_host, pw.vec.p + Np, sizeof(double) * N, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return IBO_OK;
}

extern "C" int ibo_pref_newton_step(ibo_gp_t *g, int nnz, const int64_t *lin_host, const double *val_host,
                                    const double *grad_host, double *delta_host, double *rdelta_host, int *info)
{
    IBO_TRY(pref_check(g));
    if (!grad_host || !delta_host || !rdelta_host) return fail(IBO_ERR_ARG, "NULL argument");
    auto &pw = g->pw;
    const int N = g->N, Np = g->Npad;
    hipStream_t s = g->stream;
    IBO_TRY(pref_sparse(g, nnz, lin_host, val_host));
    std::vector<double> bp(Np, 0.0);
    for (int i = 0; i < N; i++) bp[i] = -grad_host[i];
    HIP_TRY(hipMemcpyAsync(pw.vec.p, bp.data(), sizeof(double) * Np, hipMemcpyHostToDevice, s));
    KERNEL_TRY(launch_pref_build(pw.Rinv.p, N, Np, 0.0, nnz, pw.lin.p, pw.val.p, pw.A.p, s));
    IBO_TRY(pref_factor(g, info));                      // synchronises: bp may go
    double *delta = pw.vec.p + Np, *rdelta = pw.vec.p + 2 * (size_t)Np, *junk = pw.vec.p + 3 * (size_t)Np;
    KERNEL_TRY(launch_alpha(pw.E.p, N, Np, pw.vec.p, pw.tmp.p, delta, junk, s));        // delta = H^-1 (-g)
    KERNEL_TRY(launch_alpha(g->W.p, N, Np, delta, pw.tmp.p, rdelta, junk, s));           // R^-1 delta, for the line search
    HIP_TRY(hipMemcpyAsync(delta_host, delta, sizeof(double) * N, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(rdelta_host, rdelta, sizeof(double) * N, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return IBO_OK;
}

// C = diag I + the pairs' entries; the handle's factor becomes chol(R + C^-1) (W, alpha vectors with it), as
// ibo_gp_fit_with_matrix(R + C^-1) would leave it.  IBO_ERR_NOT_PD (from C or from the sum): nothing usable is left
// but the data; the caller adds to `diag` and calls again, or refits.
extern "C" int ibo_pref_finish(ibo_gp_t *g, int nnz, const int64_t *lin_host, const double *val_host, double diag, int *info)
{
    if (!g) return fail(IBO_ERR_ARG, "gp is NULL");
    if (!pref_owned(g) || g->reversed || g->N < 1)
        return fail(IBO_ERR_STATE, "no ibo_pref_begin since this model was last fitted, extended or reduced");
    IBO_TRY(use_device(g->device));
    auto &pw = g->pw;
    const int N = g->N, Np = g->Npad;
    hipStream_t s = g->stream;
    IBO_TRY(pref_sparse(g, nnz, lin_host, val_host));
    KERNEL_TRY(launch_pref_build(nullptr, N, Np, diag, nnz, pw.lin.p, pw.val.p, pw.A.p, s));
    g->fitted = false;                                   // from here on the old factor is not to be trusted
    IBO_TRY(pref_factor(g, info));
    KERNEL_TRY(launch_wtw(pw.E.p, pw.Et.p, pw.A.p, Np, s));                              // C^-1
    IBO_TRY(g->A.ensure((size_t)N * N));
    IBO_TRY(ensure_R(g));
    KERNEL_TRY(launch_pref_sum(g->R.p, pw.A.p, N, Np, g->A.p, s));
    IBO_TRY(fit_factor(g, g->kp_fit, N, g->noise, true, info));
    pw.epoch = g->fit_epoch;                             // the same points and the same R: the workspace stays with the handle (another ibo_pref_finish is accepted)
    return IBO_OK;
}

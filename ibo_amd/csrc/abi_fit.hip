// abi_fit.hip -- the model side of the C ABI: fit (covariance, factor-and-invert through abi_factor.h, alpha vectors), the block extension,
// the removal of rows, set_y, the prior, accessors and ibo_cov_matrix.
#include "abi_factor.h"
#include "loo.h"
#include "downdate.h"

#include <algorithm>

int make_kparams(int ktype, int D, const double *hyper, int nhyper, double sf2, KParams *kp)
{
    if (D < 1 || D > IBO_DMAX) return fail(IBO_ERR_ARG, "D=%d unsupported (1..%d)", D, IBO_DMAX);
    if (!hyper) return fail(IBO_ERR_ARG, "hyper is NULL");
    memset(kp, 0, sizeof(*kp));
    kp->D = D; kp->sf2 = sf2;
    switch (ktype) {
    case IBO_K_SE_ARD:
        if (nhyper < D) return fail(IBO_ERR_ARG, "SE-ARD needs %d length scales, got %d", D, nhyper);
        kp->family = FAM_SE;
        for (int d = 0; d < D; d++) { kp->w[d] = 1.0 / (hyper[d] * hyper[d]); kp->sw[d] = 1.0 / fabs(hyper[d]); }
        break;
    case IBO_K_SE_ISO:
    case IBO_K_MATERN3:
    case IBO_K_MATERN5:
        if (nhyper < 1) return fail(IBO_ERR_ARG, "kernel needs a length scale");
        kp->family = ktype == IBO_K_SE_ISO ? FAM_SE : (ktype == IBO_K_MATERN3 ? FAM_M3 : FAM_M5);
        for (int d = 0; d < D; d++) { kp->w[d] = 1.0 / (hyper[0] * hyper[0]); kp->sw[d] = 1.0 / fabs(hyper[0]); }
        break;
    default:
        return fail(IBO_ERR_ARG, "unknown kernel type %d", ktype);
    }
    return IBO_OK;
}

// |x~|^2 bounds the absolute error of y = a_k + b_c + x~.c~ by ~|x~|^2 * 2^-52 (IBO_DOT_GUARD, ibo_common.h)
static int dot_form_ok(const KParams &kp, const double *X, int N, int D)
{
    if (D > IBO_DDOT) return 0;                      // 33 .. 64 dimensions: difference-form kernels only
    double mx = 0.0;
    for (int i = 0; i < N; i++) {
        const double n2 = ibo_scaled_norm2(kp.sw, X + (size_t)i * D, D);
        if (n2 > mx) mx = n2;
    }
    const char *e = getenv("IBO_DOT_FORM");
    if (e) return atoi(e);
    return mx <= IBO_DOT_GUARD;
}

// the factor-side buffers of a handle whose frame has Np rows: what a fit writes, from the targets on (the gradient-observation frame has no others)
int fit_buffers(ibo_gp *g, int Np)
{
    const size_t nn = (size_t)Np * Np;
    IBO_TRY(g->Y.ensure(Np)); IBO_TRY(g->L.ensure(nn)); IBO_TRY(g->W.ensure(nn));
    IBO_TRY(g->T.ensure(nn)); IBO_TRY(g->Wp.ensure(nn)); IBO_TRY(g->diag64.ensure(diag64_size(Np)));
    // sweep2's stages cover rows up to the next multiple of 128: the tail of both alpha vectors stays zero
    IBO_TRY(g->alphaY.ensure((size_t)Np + 128)); IBO_TRY(g->alpha1.ensure((size_t)Np + 128));
    if (g->alpha_tail_Y != g->alphaY.p || g->alpha_tail_1 != g->alpha1.p || g->alpha_tail_Np != Np) {     // (nothing writes there)
        HIP_TRY(hipMemsetAsync(g->alphaY.p + Np, 0, 128 * sizeof(double), g->stream));
        HIP_TRY(hipMemsetAsync(g->alpha1.p + Np, 0, 128 * sizeof(double), g->stream));
        g->alpha_tail_Y = g->alphaY.p; g->alpha_tail_1 = g->alpha1.p; g->alpha_tail_Np = Np;
    }
    IBO_TRY(g->tmp.ensure(alpha_scratch(Np) + (size_t)Np));     // launch_alpha's scratch, then one vector (ibo_gp_extend)
    return g->info.ensure(1);
}

// stage observations (optionally in reverse order) and size every buffer
static int stage_data(ibo_gp *g, int N, int D, const double *X, const double *Y, bool reverse)
{
    if (N < 1) return fail(IBO_ERR_ARG, "N=%d", N);
    if (!X || !Y) return fail(IBO_ERR_ARG, "X/Y is NULL");
    g->N = N; g->D = D; g->Npad = round_up(N + (reverse ? 0 : g->reserve), 64); g->DP = D <= 4 ? 4 : (D <= 8 ? 8 : (D <= 16 ? 16 : (D <= 32 ? 32 : 64)));
    g->reversed = reverse;
    g->R_valid = false;             // new points: R is formed again when someone asks (ensure_R)
    const int Np = g->Npad, DP = g->DP;
    IBO_TRY(g->Xp.ensure((size_t)Np * DP)); IBO_TRY(g->Xs.ensure((size_t)Np * DP)); IBO_TRY(g->ak.ensure(Np));
    IBO_TRY(g->XA.ensure((size_t)((Np + 127) / 128 * 8) * ((D + 5) / 4) * 64));
    IBO_TRY(fit_buffers(g, Np));
    // staged through the handle's pinned buffer: the copies are truly asynchronous and nothing has to be waited for before the fit's
    // kernels are queued (a pageable source is staged by the runtime and had to be kept alive by a stream synchronise: ~25 us of a 0.37 ms fit)
    IBO_TRY(ensure_pinned(g, (size_t)Np * DP + Np));
    double *xp = g->pin, *yp = g->pin + (size_t)Np * DP;
    memset(g->pin, 0, sizeof(double) * ((size_t)Np * DP + Np));
    g->Yhost.assign(N, 0.0);
    double my = Y[0];
    for (int i = 0; i < N; i++) {
        int s = reverse ? N - 1 - i : i;
        for (int d = 0; d < D; d++) xp[(size_t)i * DP + d] = X[(size_t)s * D + d];
        yp[i] = Y[s];
        g->Yhost[i] = Y[s];
        if (Y[i] > my) my = Y[i];      // acqmaxGP's maxY scan, cpp/optimizeGP.cpp:316-321
    }
    g->maxY = my;
    HIP_TRY(hipMemcpyAsync(g->Xp.p, xp, sizeof(double) * (size_t)Np * DP, hipMemcpyHostToDevice, g->stream));
    HIP_TRY(hipMemcpyAsync(g->Y.p, yp, sizeof(double) * Np, hipMemcpyHostToDevice, g->stream));
    return IBO_OK;                                  // (every caller ends with a stream synchronise before the pinned buffer is used again)
}

// synchronises; a failed pivot leaves the handle unfitted
static int check_info(ibo_gp *g, int *info, const char *noun = "matrix")
{
    const int rc = factor_info(g->info.p, g->stream, noun, info);
    if (rc != IBO_OK) g->fitted = false;
    return rc;
}

// after the stream has passed fit1: fit0 -> fit1 is the fit's time (ibo_gp_last_fit_ms) and goes to the device's GPU time
static int fit_span(ibo_gp *g)
{
    HIP_TRY(hipEventElapsedTime(&g->fit_ms, g->fit0, g->fit1));
    gpu_time_add(g->device, g->fit_ms);
    return IBO_OK;
}

// R = K(X, X) with the reference's hard-wired diagonal 1 + noise (ego/gaussianprocess/__init__.py:138), over the rows the
// model holds now, by the kernel and in the order of operations the fit's own covariance pass uses: what a fit, or a fit
// and its extensions, would have written had they kept R up to date.
int ensure_R(ibo_gp *g)
{
    if (g->R_valid) return IBO_OK;
    IBO_TRY(g->R.ensure((size_t)g->Npad * g->Npad));             // N x N with row stride Npad (room to extend)
    KERNEL_TRY(launch_cov_matrix(g->kp_fit, g->N, g->Xp.p, 0, nullptr, g->DP, IBO_DIAG_UNIT_PLUS_NOISE, g->noise, g->R.p, g->Npad, g->stream));
    g->R_valid = true;
    return IBO_OK;
}

// What every fit starts with: the kernel's parameters, the data staged (reverse: in reverse order) and scaled, the dot form's guard ...
int fit_begin(ibo_gp *g, int ktype, int N, int D, const double *X, const double *Y, const double *hyper, int nhyper, double sf2,
                     double noise, bool reverse, KParams *kp)
{
    IBO_TRY(use_device(g->device));
    IBO_TRY(make_kparams(ktype, D, hyper, nhyper, sf2, kp));
    g->fitted = false;
    g->pw.ready = false;                                 // other data from here on, whether or not they can be factored
    IBO_TRY(stage_data(g, N, D, X, Y, reverse));
    g->kp = *kp; g->noise = noise;
    if (!reverse) g->kp_fit = *kp;
    KERNEL_TRY(launch_scale_x(*kp, g->Xp.p, g->Npad, g->DP, g->Xs.p, g->ak.p, g->stream));
    KERNEL_TRY(launch_pack_xa(g->Xs.p, g->ak.p, N, g->Npad, g->DP, D, g->XA.p, g->stream));
    g->dot_form = dot_form_ok(*kp, X, N, D);
    return IBO_OK;
}
// ... and ends with, W in place, in two halves (a caller that times its stages marks the stream between them): both alpha vectors, queued ...
int fit_alpha(ibo_gp *g, int N)
{
    KERNEL_TRY(launch_alpha(g->W.p, N, g->Npad, g->Y.p, g->tmp.p, g->alphaY.p, g->alpha1.p, g->stream));
    return IBO_OK;
}
// ... then the info word (synchronises; noun: what the message calls the matrix) and the span fit0 -> fit1
int fit_end(ibo_gp *g, bool plain, const char *noun, int *info)
{
    HIP_TRY(hipEventRecord(g->fit1, g->stream));
    IBO_TRY(check_info(g, info, noun));
    IBO_TRY(fit_span(g));
    g->fitted = true;
    g->plain_fit = plain;
    g->fit_epoch++;
    return IBO_OK;
}

// A handle's frame for its Npad rows (fit_frame, abi_factor.h, which says why T and W are lent twice): the matrix goes to b->A ...
int fit_operands(ibo_gp *g, FactorRoute *route, FactorBufs *b)
{
    return fit_frame(g->Npad, g->T.p, g->L.p, g->W.p, g->Wp.p, g->T.p, g->W.p, g->diag64.p, g->info.p, g->tall, g->Pk2, route, b);
}
// ... and the factorisation and inversion of the matrix in it (N rows its own), queued: T and Wp then trade places
int fit_invert(ibo_gp *g, FactorRoute route, const FactorBufs &b, int N)
{
    IBO_TRY(factor_invert(route, N, g->Npad, b, g->stream));
    std::swap(g->T, g->Wp);
    g->L_upper_dirty = true;        // the strict upper blocks of L are scratch until someone asks for L
    return IBO_OK;
}

// Everything of a fit after the data are staged: R, L = chol(R) -- or chol(A) for a matrix already in g->A (N x N) --,
// W = L^-1 and its packed copy, both alpha vectors.
int fit_factor(ibo_gp *g, const KParams &kp, int N, double noise, bool have_A, int *info)
{
    const int Np = g->Npad;
    hipStream_t s = g->stream;
    FactorRoute route;
    FactorBufs b;
    HIP_TRY(hipEventRecord(g->fit0, s));
    IBO_TRY(fit_operands(g, &route, &b));
    // R's identity-padded working copy and in the same pass, on the ride-along, the identity it starts from; and the cleared info word
    // (GP.R itself is not written here: 33 MB of stores at N = 2048 that only ibo_gp_get_R and ibo_pref_finish read -- ensure_R;
    // stage_data marked it stale)
    b.eye_ready = !have_A && route != ROUTE_TWO_LEVEL;
    if (!have_A)
        KERNEL_TRY(launch_cov_fit(kp, N, g->Xp.p, g->DP, IBO_DIAG_UNIT_PLUS_NOISE, noise, b.A, Np, b.eye_ready ? b.eye : nullptr, g->info.p, s));
    else {
        HIP_TRY(hipMemsetAsync(g->info.p, 0, sizeof(int), s));
        KERNEL_TRY(launch_pad_copy(g->A.p, N, N, b.A, Np, 1.0, s));
    }
    IBO_TRY(fit_invert(g, route, b, N));
    IBO_TRY(fit_alpha(g, N));
    return fit_end(g, !have_A, "matrix", info);
}

static int fit_impl(ibo_gp *g, int ktype, int N, int D, const double *X, const double *Y,
                    const double *hyper, int nhyper, double sf2, double noise, const double *A_host, int *info)
{
    if (!g) return fail(IBO_ERR_ARG, "gp is NULL");
    KParams kp;
    IBO_TRY(fit_begin(g, ktype, N, D, X, Y, hyper, nhyper, sf2, noise, false, &kp));
    if (A_host) {
        IBO_TRY(g->A.ensure((size_t)N * N));
        HIP_TRY(hipMemcpyAsync(g->A.p, A_host, sizeof(double) * (size_t)N * N, hipMemcpyHostToDevice, g->stream));
    }
    return fit_factor(g, kp, N, noise, A_host != nullptr, info);
}

// Append observations to a fitted model without refactoring: the block extension of
// GaussianProcess.addData (ego/gaussianprocess/__init__.py:301-308), z = L^-1 m, d = chol(r - z^T z), one
// point at a time.  With W = L^-1 already on the device, z = W k and the new row of W is -(W^T z)/d: two
// triangular matrix-vector products (the same kernels that form alpha), O(N^2) instead of the O(N^3) refit.
extern "C" int ibo_gp_extend(ibo_gp_t *g, int n, const double *Xnew, const double *Yall, int *info)
{
    if (!g || !Xnew || !Yall || n < 1) return fail(IBO_ERR_ARG, "bad argument");
    if (!g->fitted || !g->plain_fit || g->reversed) return fail(IBO_ERR_STATE, "model cannot be extended in place");
    if (g->N + n > g->Npad) return fail(IBO_ERR_STATE, "no room in the current padding (%d + %d > %d)", g->N, n, g->Npad);
    IBO_TRY(use_device(g->device));
    hipStream_t s = g->stream;
    const int Np = g->Npad, DP = g->DP, D = g->D, N0 = g->N;
    if (info) *info = 0;
    // stage the new rows of X (padded to DP) behind the old ones; sizes do not change
    std::vector<double> xp((size_t)n * DP, 0.0);
    for (int i = 0; i < n; i++)
        for (int d = 0; d < D; d++) xp[(size_t)i * DP + d] = Xnew[(size_t)i * D + d];
    HIP_TRY(hipMemcpyAsync(g->Xp.p + (size_t)N0 * DP, xp.data(), xp.size() * sizeof(double), hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemsetAsync(g->info.p, 0, sizeof(int), s));
    HIP_TRY(hipEventRecord(g->fit0, s));
    // from here on the handle's rows are being rewritten: any early return (a HIP or launch error) must leave it marked
    // unfitted -- the caller then refits -- rather than "fitted" with rows N0.. of L / W / Wp half-written
    g->fitted = false;
    for (int i = 0; i < n; i++) {
        const int N = N0 + i;                       // rows present before this point
        // k = K(X, x_new) (also the new row / column of R), z = W k and u = W^T z, then the new rows of L and W
        double *kvec = g->tmp.p + alpha_scratch(Np);
        KERNEL_TRY(launch_extend_kvec(g->kp_fit, g->Xp.p, DP, N, Np, g->noise, g->R_valid ? g->R.p : nullptr, kvec, s));
        KERNEL_TRY(launch_alpha(g->W.p, N, Np, kvec, g->tmp.p, g->T.p, g->T.p + Np, s));      // t2[0..Np) = z, T[0..Np) = W^T z
        KERNEL_TRY(launch_extend_rows(N, Np, g->noise, g->tmp.p, g->T.p, g->L.p, g->W.p, g->Wp.p, g->info.p, s));
    }
    const int N1 = N0 + n;
    std::vector<double> yp(Np, 0.0);
    double my = Yall[0];
    for (int i = 0; i < N1; i++) { yp[i] = Yall[i]; if (Yall[i] > my) my = Yall[i]; }
    HIP_TRY(hipMemcpyAsync(g->Y.p, yp.data(), yp.size() * sizeof(double), hipMemcpyHostToDevice, s));
    KERNEL_TRY(launch_scale_x(g->kp_fit, g->Xp.p, Np, DP, g->Xs.p, g->ak.p, s));
    KERNEL_TRY(launch_pack_xa(g->Xs.p, g->ak.p, N1, Np, DP, D, g->XA.p, s));
    KERNEL_TRY(launch_alpha(g->W.p, N1, Np, g->Y.p, g->tmp.p, g->alphaY.p, g->alpha1.p, s));
    HIP_TRY(hipEventRecord(g->fit1, s));
    // (synchronises -- xp / yp go out of scope; a failed pivot: the rows written so far belong to a matrix that is not positive definite,
    // the handle stays unfitted and needs a refit)
    IBO_TRY(check_info(g, info));
    IBO_TRY(fit_span(g));
    if (g->dot_form) {                              // |x~|^2 of the new points still admits the dot form?
        for (int i = 0; i < n && g->dot_form; i++)
            if (ibo_scaled_norm2(g->kp_fit.sw, Xnew + (size_t)i * D, D) > IBO_DOT_GUARD) g->dot_form = 0;
    }
    // the kept sweep state's stale tiles carry means formed with the OLD alpha vectors, and the lazy refresh's drift margin only
    // covers the appended rows' (W y)_i: a caller that changed an earlier target along the way (GaussianProcess.Y is a public
    // attribute) gets a full sweep next time, as after ibo_gp_set_y
    for (int i = 0; i < N0; i++)
        if (!(Yall[i] == g->Yhost[i])) { g->st_gen = 0; break; }
    g->N = N1; g->maxY = my;
    g->Yhost.assign(Yall, Yall + N1);
    g->L_upper_dirty = true;
    g->fitted = true;
    return IBO_OK;
}

// Take observations out of a fitted model without refactoring: per row the rank-one update of the trailing factor and of its inverse
// (downdate.hip), O(N^2), in DESCENDING index order so the earlier indices stay valid.  Out of place: L' into T (scratch after a fit; the two
// then trade places, as fit_factor trades T and Wp), W' into one pool buffer that is handed back before the call returns.  Npad does not
// change: a removal gives a row of head-room back to ibo_gp_extend.
extern "C" int ibo_gp_remove(ibo_gp_t *g, int n, const int *rows_host, const double *Y_rest, int *info)
{
    if (!g || !rows_host || !Y_rest || n < 1) return fail(IBO_ERR_ARG, "bad argument");
    if (!g->fitted || !g->plain_fit || g->reversed) return fail(IBO_ERR_STATE, "rows cannot be removed from this model in place");
    if (n >= g->N) return fail(IBO_ERR_ARG, "cannot remove %d of %d rows", n, g->N);
    std::vector<int> rows(rows_host, rows_host + n);
    std::sort(rows.begin(), rows.end(), [](int a, int b) { return a > b; });
    for (int k = 0; k < n; k++) {
        if (rows[k] < 0 || rows[k] >= g->N) return fail(IBO_ERR_ARG, "row %d out of range (model: %d rows)", rows[k], g->N);
        if (k > 0 && rows[k] == rows[k - 1]) return fail(IBO_ERR_ARG, "row %d given twice", rows[k]);
    }
    IBO_TRY(use_device(g->device));
    hipStream_t s = g->stream;
    const int Np = g->Npad, DP = g->DP, D = g->D, N0 = g->N, N1 = N0 - n;
    if (info) *info = 0;
    ScopedBuf<double> wbuf;
    IBO_TRY(wbuf.ensure((size_t)Np * Np));
    IBO_TRY(g->tmp.ensure(downdate_scratch(Np)));       // (inside what stage_data sized for launch_alpha)
    std::vector<double> yp(Np, 0.0);
    double my = Y_rest[0];
    for (int i = 0; i < N1; i++) { yp[i] = Y_rest[i]; if (Y_rest[i] > my) my = Y_rest[i]; }      // stage_data's scan
    HIP_TRY(hipMemsetAsync(g->info.p, 0, sizeof(int), s));
    HIP_TRY(hipEventRecord(g->fit0, s));
    // from here on the handle's rows are being rewritten: any early return must leave it marked unfitted (the caller then refits)
    g->fitted = false;
    g->st_gen = 0;                                      // a kept sweep state never survives a removal
    g->R_valid = false;                                 // ensure_R re-forms R on request
    const double *Lsrc = g->L.p, *Wsrc = g->W.p;
    double *Ldst = g->T.p, *Wdst = wbuf.p;
    for (int k = 0; k < n; k++) {
        const int N = N0 - k, i = rows[k];
        KERNEL_TRY(launch_downdate_scalars(Wsrc, N, Np, i, g->tmp.p, g->info.p, s));
        KERNEL_TRY(launch_downdate_L(Lsrc, N, Np, i, g->tmp.p, Ldst, s));
        KERNEL_TRY(launch_downdate_W(Wsrc, N, Np, i, g->tmp.p, Wdst, s));
        KERNEL_TRY(launch_downdate_X(g->Xp.p, N, Np, DP, i, g->Xs.p, s));                         // Xs: rewritten by launch_scale_x below
        HIP_TRY(hipMemcpyAsync(g->Xp.p, g->Xs.p, sizeof(double) * (size_t)Np * DP, hipMemcpyDeviceToDevice, s));
        const double *l = Lsrc, *w = Wsrc;
        Lsrc = Ldst; Ldst = const_cast<double *>(l);
        Wsrc = Wdst; Wdst = const_cast<double *>(w);
    }
    if (Lsrc != g->L.p) std::swap(g->L, g->T);          // an odd number of steps: the factor is in what was T
    KERNEL_TRY(launch_pack_w(Wsrc, N1, Np, 0, g->W.p, g->Wp.p, s));                               // W (from the pool buffer, or in place) and its fragment copy
    HIP_TRY(hipMemcpyAsync(g->Y.p, yp.data(), yp.size() * sizeof(double), hipMemcpyHostToDevice, s));
    KERNEL_TRY(launch_scale_x(g->kp_fit, g->Xp.p, Np, DP, g->Xs.p, g->ak.p, s));
    KERNEL_TRY(launch_pack_xa(g->Xs.p, g->ak.p, N1, Np, DP, D, g->XA.p, s));
    KERNEL_TRY(launch_alpha(g->W.p, N1, Np, g->Y.p, g->tmp.p, g->alphaY.p, g->alpha1.p, s));
    HIP_TRY(hipEventRecord(g->fit1, s));
    g->N = N1;                                          // (what the device holds now, whatever the info word says)
    IBO_TRY(check_info(g, info));                       // synchronises: yp and the pool buffer may go
    IBO_TRY(fit_span(g));
    g->maxY = my;
    g->Yhost.assign(Y_rest, Y_rest + N1);
    g->L_upper_dirty = true;
    g->fit_epoch++;
    g->fitted = true;
    return IBO_OK;
}

extern "C" int ibo_gp_reserve(ibo_gp_t *g, int rows)
{
    if (!g || rows < 0) return fail(IBO_ERR_ARG, "bad argument");
    g->reserve = rows;
    return IBO_OK;
}

extern "C" int ibo_gp_fit(ibo_gp_t *g, int ktype, int N, int D, const double *X, const double *Y,
                          const double *hyper, int nhyper, double sf2, double noise, int *info)
{
    return fit_impl(g, ktype, N, D, X, Y, hyper, nhyper, sf2, noise, nullptr, info);
}

extern "C" int ibo_gp_fit_with_matrix(ibo_gp_t *g, int ktype, int N, int D, const double *X, const double *Y,
                                      const double *hyper, int nhyper, double sf2, double noise,
                                      const double *A_host, int *info)
{
    if (!A_host) return fail(IBO_ERR_ARG, "A_host is NULL");
    return fit_impl(g, ktype, N, D, X, Y, hyper, nhyper, sf2, noise, A_host, info);
}

// legacy entry: the caller hands over invR (ego/acquisition/__init__.py:385-388).
// invR = G G^T; q = |G^T k*|^2; reversing the index order makes G^T lower
// triangular so the same sweep kernel applies (see pack_w_kernel, mode 1).
int fit_from_inverse(ibo_gp *g, int ktype, int N, int D, const double *X, const double *Y,
                            const double *hyper, int nhyper, double sf2, double noise, const double *invR)
{
    KParams kp;
    IBO_TRY(fit_begin(g, ktype, N, D, X, Y, hyper, nhyper, sf2, noise, true, &kp));
    const int Np = g->Npad;
    hipStream_t s = g->stream;
    IBO_TRY(g->A.ensure((size_t)N * N));
    HIP_TRY(hipMemcpyAsync(g->A.p, invR, sizeof(double) * (size_t)N * N, hipMemcpyHostToDevice, s));
    HIP_TRY(hipEventRecord(g->fit0, s));
    KERNEL_TRY(launch_pad_copy(g->A.p, N, N, g->L.p, Np, 1.0, s));
    KERNEL_TRY(launch_cholesky(g->L.p, Np, g->diag64.p, g->info.p, s));          // (FACTOR_IN_PLACE's route; only the factor is wanted)
    KERNEL_TRY(launch_pack_w(g->L.p, N, Np, 1, g->W.p, g->Wp.p, s));
    IBO_TRY(fit_alpha(g, N));
    return fit_end(g, false, "matrix", nullptr);
}

extern "C" int ibo_gp_set_y(ibo_gp_t *g, const double *Y_host)
{
    if (!g || !Y_host) return fail(IBO_ERR_ARG, "NULL argument");
    if (!g->fitted) return fail(IBO_ERR_STATE, "set_y before fit");
    IBO_TRY(use_device(g->device));
    std::vector<double> yp(g->Npad, 0.0);
    double my = Y_host[0];
    for (int i = 0; i < g->N; i++) {
        yp[i] = Y_host[g->reversed ? g->N - 1 - i : i];
        g->Yhost[i] = yp[i];
        if (Y_host[i] > my) my = Y_host[i];
    }
    g->maxY = my;
    g->st_gen = 0;                                  // the kept per-candidate means were formed with the old alpha vectors
    HIP_TRY(hipMemcpyAsync(g->Y.p, yp.data(), yp.size() * sizeof(double), hipMemcpyHostToDevice, g->stream));
    KERNEL_TRY(launch_alpha(g->W.p, g->N, g->Npad, g->Y.p, g->tmp.p, g->alphaY.p, g->alpha1.p, g->stream));
    HIP_TRY(hipStreamSynchronize(g->stream));
    return IBO_OK;
}

extern "C" int ibo_gp_set_kstar_sf2(ibo_gp_t *g, double sf2)
{
    if (!g) return fail(IBO_ERR_ARG, "gp is NULL");
    g->kp.sf2 = sf2;
    return IBO_OK;
}

extern "C" int ibo_gp_set_prior(ibo_gp_t *g, int nb, const double *means, const double *beta, double theta,
                                const double *lowerb, const double *width)
{
    if (!g) return fail(IBO_ERR_ARG, "gp is NULL");
    if (nb <= 0) { g->nb = 0; return IBO_OK; }
    if (g->D <= 0) return fail(IBO_ERR_STATE, "set_prior before fit (dimension unknown)");
    if (!means || !beta || !lowerb || !width) return fail(IBO_ERR_ARG, "NULL prior array");
    IBO_TRY(use_device(g->device));
    const int D = g->D;
    IBO_TRY(g->pmeans.ensure((size_t)nb * D)); IBO_TRY(g->pbeta.ensure(nb));
    IBO_TRY(g->plowerb.ensure(D)); IBO_TRY(g->pwidth.ensure(D));
    HIP_TRY(hipMemcpy(g->pmeans.p, means, sizeof(double) * nb * D, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(g->pbeta.p, beta, sizeof(double) * nb, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(g->plowerb.p, lowerb, sizeof(double) * D, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(g->pwidth.p, width, sizeof(double) * D, hipMemcpyHostToDevice));
    g->nb = nb; g->ptheta = theta;
    return IBO_OK;
}

static int copy_square(ibo_gp *g, const double *src, int ld, double *dst_host)
{
    IBO_TRY(use_device(g->device));
    HIP_TRY(hipMemcpy2D(dst_host, sizeof(double) * g->N, src, sizeof(double) * ld, sizeof(double) * g->N, g->N,
                        hipMemcpyDeviceToHost));
    return IBO_OK;
}

extern "C" int ibo_gp_get_R(ibo_gp_t *g, double *R_host)
{
    if (!g || !R_host) return fail(IBO_ERR_ARG, "NULL argument");
    if (!g->fitted || g->reversed) return fail(IBO_ERR_STATE, "R not available");
    IBO_TRY(use_device(g->device));
    IBO_TRY(ensure_R(g));
    HIP_TRY(hipStreamSynchronize(g->stream));
    return copy_square(g, g->R.p, g->Npad, R_host);
}
extern "C" int ibo_gp_get_L(ibo_gp_t *g, double *L_host)
{
    if (!g || !L_host) return fail(IBO_ERR_ARG, "NULL argument");
    if (!g->fitted || g->reversed) return fail(IBO_ERR_STATE, "L not available");
    if (g->L_upper_dirty) {
        IBO_TRY(use_device(g->device));
        KERNEL_TRY(launch_zero_upper(g->L.p, g->Npad, g->stream));
        HIP_TRY(hipStreamSynchronize(g->stream));
        g->L_upper_dirty = false;
    }
    return copy_square(g, g->L.p, g->Npad, L_host);
}
extern "C" int ibo_gp_get_W(ibo_gp_t *g, double *W_host)
{
    if (!g || !W_host) return fail(IBO_ERR_ARG, "NULL argument");
    if (!g->fitted || g->reversed) return fail(IBO_ERR_STATE, "W not available");
    return copy_square(g, g->W.p, g->Npad, W_host);
}
// Leave-one-out predictions of a fitted model from what the handle holds: d_i = |column i of W|^2 = (A^-1)_ii, c = aY - m(x_i) a1.
extern "C" int ibo_gp_loo(ibo_gp_t *g, double *mu_host, double *s2_host, double *nloo_host)
{
    if (!g) return fail(IBO_ERR_ARG, "gp is NULL");
    if (!mu_host && !s2_host && !nloo_host) return fail(IBO_ERR_ARG, "every output is NULL");
    IBO_TRY(use_device(g->device));
    if (!g->fitted || g->reversed) return fail(IBO_ERR_STATE, "leave-one-out before a successful fit");
    const int N = g->N, Np = g->Npad;
    hipStream_t s = g->stream;
    ScopedBuf<double> buf;                              // d, mu, s2 (Np each) and the sum
    IBO_TRY(buf.ensure(3 * (size_t)Np + 1));
    double *d = buf.p, *mu = d + Np, *s2 = mu + Np, *out = s2 + Np;
    KERNEL_TRY(launch_loo_diag(g->W.p, (size_t)Np, N, d, s));
    KERNEL_TRY(launch_loo_handle(prior_of(g), g->Xp.p, g->DP, g->D, N, g->Y.p, g->alphaY.p, g->alpha1.p, d, mu_host ? mu : nullptr, s2_host ? s2 : nullptr,
                                 out, s));
    double v = 0.0;
    if (mu_host) HIP_TRY(hipMemcpyAsync(mu_host, mu, sizeof(double) * N, hipMemcpyDeviceToHost, s));
    if (s2_host) HIP_TRY(hipMemcpyAsync(s2_host, s2, sizeof(double) * N, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(&v, out, sizeof(double), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (nloo_host) *nloo_host = v + 0.5 * N * log(2.0 * M_PI);
    return IBO_OK;
}
extern "C" int ibo_gp_info(ibo_gp_t *g, int *N, int *D, int *device, double *max_y)
{
    if (!g) return fail(IBO_ERR_ARG, "gp is NULL");
    if (N) *N = g->N;
    if (D) *D = g->D;
    if (device) *device = g->device;
    if (max_y) *max_y = g->maxY;
    return IBO_OK;
}
extern "C" int ibo_gp_last_fit_ms(ibo_gp_t *g, float *ms)
{
    if (!g || !ms) return fail(IBO_ERR_ARG, "NULL argument");
    *ms = g->fit_ms;
    return IBO_OK;
}

extern "C" int ibo_cov_matrix(int device, int ktype, int D, const double *hyper, int nhyper, double sf2,
                              int n1, const double *A1, int n2, const double *A2, int diag_rule, double noise,
                              double *K_host)
{
    if (!A1 || !K_host || n1 < 1 || (A2 && n2 < 1)) return fail(IBO_ERR_ARG, "bad argument");
    IBO_TRY(use_device(device));
    KParams kp;
    IBO_TRY(make_kparams(ktype, D, hyper, nhyper, sf2, &kp));
    int m2 = A2 ? n2 : n1;
    ScopedBuf<double> a1, a2, k;
    IBO_TRY(a1.ensure((size_t)n1 * D)); IBO_TRY(k.ensure((size_t)n1 * m2));
    HIP_TRY(hipMemcpy(a1.p, A1, sizeof(double) * n1 * D, hipMemcpyHostToDevice));
    if (A2) {
        IBO_TRY(a2.ensure((size_t)n2 * D));
        HIP_TRY(hipMemcpy(a2.p, A2, sizeof(double) * n2 * D, hipMemcpyHostToDevice));
    }
    KERNEL_TRY(launch_cov_matrix(kp, n1, a1.p, n2, A2 ? a2.p : nullptr, D, diag_rule, noise, k.p, m2, nullptr, 0));
    HIP_TRY(hipMemcpy(K_host, k.p, sizeof(double) * (size_t)n1 * m2, hipMemcpyDeviceToHost));
    return IBO_OK;
}

// abi_factor.hip -- the one factor-and-invert routine behind the C ABI (abi_factor.h): the route choice, the factorisation with one of two
// inversion tails, the info word's read-back; and the two entries that are nothing but that routine, ibo_spd_solve and ibo_spd_inverse.
#include "abi_factor.h"

// The single-level order up to g_fused2_min_nb block columns
static inline bool single_level_order(int Np) { return Np / 64 < g_fused2_min_nb; }
// The super-panels address their tall store [A ; E] (2 Np^2 doubles) through a buffer descriptor with 32-bit offsets: only while it lies inside
// 2^31 - 1 bytes (11584 rows; an option that keeps a larger matrix in the single-level order takes the step-by-step launches instead)
static inline bool super_order(int Np) { return Np / 64 >= g_super_min_nb && 2 * (size_t)Np * Np * sizeof(double) <= 0x7fffffffu; }
// The packed stores of the left-looking updates (update3.hip) are addressed with 32-bit unsigned byte offsets: one matrix must lie inside
// 2^32 - 1 bytes (23168 rows)
static inline bool u3_fits(int Np) { return (size_t)Np * Np * sizeof(double) <= 0xffffffffu; }

int factor_route(int Np, FactorCaller who, FactorRoute *route)
{
    if (who == FACTOR_IN_PLACE) { *route = ROUTE_IN_PLACE; return IBO_OK; }      // (lends no packed store: no limit but memory)
    if (!u3_fits(Np)) return fail(IBO_ERR_ARG, "at most 23168 rows: the factorisation's packed store must lie inside 2^32 - 1 bytes (model: %d padded rows)", Np);
    if (single_level_order(Np)) *route = who == FACTOR_FIT && super_order(Np) ? ROUTE_RIDE_SUPER : ROUTE_RIDE;
    else *route = who == FACTOR_FIT ? ROUTE_TWO_LEVEL : ROUTE_IN_PLACE;
    return IBO_OK;
}

int factor_invert(FactorRoute route, int N, int Np, const FactorBufs &b, hipStream_t s)
{
    if (route == ROUTE_RIDE || route == ROUTE_RIDE_SUPER) {
        // E = I turns into (L^-1)^T in Et under the factorisation's own launches; one pass transposes it into W and packs it
        if (!b.eye_ready) KERNEL_TRY(launch_pad_copy(b.A, 0, 1, b.eye, Np, 1.0, s));            // identity (no source rows: nothing is read)
        if (route == ROUTE_RIDE_SUPER) KERNEL_TRY(launch_cholesky_super(b.A, b.L, Np, b.d64, b.info, s, b.Et, b.Pk, b.info_zero));
        else KERNEL_TRY(launch_cholesky_fused(b.A, b.L, Np, b.d64, b.info, s, b.eye, b.Et, b.info_zero));
        KERNEL_TRY(launch_transpose_pack(b.Et, N, Np, b.W, b.Wp, s));
        return IBO_OK;
    }
    const double *L = b.L;
    if (route == ROUTE_TWO_LEVEL) KERNEL_TRY(launch_cholesky_fused2(b.A, b.L, Np, b.d64, b.info, 4, s, b.info_zero, b.Pk));
    else {
        KERNEL_TRY(launch_cholesky(b.A, Np, b.d64, b.info, s, b.Pk));                            // (clears the info word itself)
        L = b.A;
    }
    // recursive doubling reads L's blocks strictly below the diagonal and d64, and writes W's blocks on and below it; pack_w_kernel then
    // rewrites EVERY element of W (zeros above the diagonal and in the pad rows): neither L's upper blocks nor W need clearing first
    KERNEL_TRY(launch_trinv(L, Np, b.d64, b.W, b.Et, s));
    KERNEL_TRY(launch_pack_w(b.W, N, Np, 0, b.W, b.Wp ? b.Wp : b.Et, s));
    return IBO_OK;
}

int fit_frame(int Np, double *T, double *L, double *W, double *Et, double *Wp, double *Pk, double *d64, int *info,
              DevBuf<double> &tall, DevBuf<double> &Pk2, FactorRoute *route, FactorBufs *b)
{
    const size_t nn = (size_t)Np * Np;
    IBO_TRY(factor_route(Np, FACTOR_FIT, route));
    *b = FactorBufs{};
    b->A = T; b->eye = W; b->Pk = Pk;
    if (*route == ROUTE_RIDE_SUPER) {
        IBO_TRY(tall.ensure(2 * nn)); IBO_TRY(Pk2.ensure(2 * nn));
        b->A = tall.p; b->eye = tall.p + nn; b->Pk = Pk2.p;
    }
    b->L = L; b->Et = Et; b->W = W; b->Wp = Wp; b->d64 = d64; b->info = info; b->info_zero = true;
    return IBO_OK;
}

int factor_info_word(int h, const char *noun, int *info_out)
{
    if (info_out) *info_out = h;
    if (h != 0) return fail(IBO_ERR_NOT_PD, "%s is not positive definite (pivot %d)", noun, h);
    return IBO_OK;
}

int factor_info(const int *info_dev, hipStream_t s, const char *noun, int *info_out)
{
    int h = 0;
    HIP_TRY(hipMemcpyAsync(&h, info_dev, sizeof(int), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return factor_info_word(h, noun, info_out);
}

// ------------------------------------------------------------------------ ibo_spd_*
// A (N x N, host) -> W = L^-1 of its Cholesky factor in an Np-row frame, pad rows zero, on the null stream; synchronises
struct SpdWork {
    ScopedBuf<double> A, L, W, T, d64;
    ScopedBuf<int> info;
};
static int spd_invert_factor(SpdWork &w, int N, int Np, const double *A_host, size_t a_size, int *info)
{
    const size_t nn = (size_t)Np * Np;
    IBO_TRY(w.A.ensure(a_size)); IBO_TRY(w.L.ensure(nn)); IBO_TRY(w.W.ensure(nn)); IBO_TRY(w.T.ensure(nn));
    IBO_TRY(w.d64.ensure(diag64_size(Np))); IBO_TRY(w.info.ensure(1));
    hipStream_t s = nullptr;
    FactorRoute route;
    IBO_TRY(factor_route(Np, FACTOR_IN_PLACE, &route));
    HIP_TRY(hipMemcpy(w.A.p, A_host, sizeof(double) * (size_t)N * N, hipMemcpyHostToDevice));
    KERNEL_TRY(launch_pad_copy(w.A.p, N, N, w.L.p, Np, 1.0, s));
    FactorBufs b = {};
    b.A = w.L.p; b.Et = w.T.p; b.W = w.W.p; b.d64 = w.d64.p; b.info = w.info.p;
    IBO_TRY(factor_invert(route, N, Np, b, s));
    return factor_info(w.info.p, s, "matrix", info);
}

// Solve A X = B for a symmetric positive-definite A (N x N, host) and nrhs right-hand sides
// (B, X: nrhs x N row-major, host) on the GPU: blocked Cholesky, explicit L^-1, X = L^-T (L^-1 B).
// Used by the preference GP's Newton iterations (the Hessian of the MAP functional).
extern "C" int ibo_spd_solve(int device, int N, const double *A_host, int nrhs, const double *B_host,
                             double *X_host, int *info)
{
    if (!A_host || !B_host || !X_host || N < 1 || nrhs < 1) return fail(IBO_ERR_ARG, "bad argument");
    IBO_TRY(use_device(device));
    const int Np = round_up(N, 64);
    SpdWork w;
    ScopedBuf<double> db, dx, d1, tmp;
    IBO_TRY(db.ensure(Np)); IBO_TRY(dx.ensure(Np)); IBO_TRY(d1.ensure(Np)); IBO_TRY(tmp.ensure(alpha_scratch(Np)));
    IBO_TRY(spd_invert_factor(w, N, Np, A_host, (size_t)N * N, info));
    hipStream_t s = nullptr;
    std::vector<double> bp(Np, 0.0);
    for (int r = 0; r < nrhs; r++) {
        for (int i = 0; i < N; i++) bp[i] = B_host[(size_t)r * N + i];
        HIP_TRY(hipMemcpy(db.p, bp.data(), sizeof(double) * Np, hipMemcpyHostToDevice));
        KERNEL_TRY(launch_alpha(w.W.p, N, Np, db.p, tmp.p, dx.p, d1.p, s));
        HIP_TRY(hipMemcpy(X_host + (size_t)r * N, dx.p, sizeof(double) * N, hipMemcpyDeviceToHost));
    }
    return IBO_OK;
}

// inverse of a symmetric positive-definite matrix (N x N host in / out): Cholesky, L^-1, W^T W.
// The preference GP needs C^-1 for L = chol(R + C^-1) (ego/gaussianprocess/__init__.py:488).
extern "C" int ibo_spd_inverse(int device, int N, const double *A_host, double *Ainv_host, int *info)
{
    if (!A_host || !Ainv_host || N < 1) return fail(IBO_ERR_ARG, "bad argument");
    IBO_TRY(use_device(device));
    const int Np = round_up(N, 64);
    SpdWork w;
    IBO_TRY(spd_invert_factor(w, N, Np, A_host, (size_t)Np * Np, info));      // (A's buffer receives the padded inverse)
    hipStream_t s = nullptr;
    KERNEL_TRY(launch_wtw(w.W.p, w.T.p, w.A.p, Np, s));
    HIP_TRY(hipMemcpy2D(Ainv_host, sizeof(double) * N, w.A.p, sizeof(double) * Np, sizeof(double) * N, N, hipMemcpyDeviceToHost));
    return IBO_OK;
}

// abi_rows.hip -- the row pipeline behind ibo_kg_* and ibo_qei_* (abi_rows.h): no entry of its own.  Nothing here lets a row's result
// depend on the rows beside it, and every entry of both units sends its candidates through RowPipeline::chunk: that is why a candidate's
// value is the same bits from a sweep, a host batch and a DIRECT batch, whatever the chunk.
#include "abi_rows.h"

KgRowsArgs rows_args(const ibo_gp *g, const double *Kt, const double *Vt, const double *Q, int m, double clamp_lo)
{
    KgRowsArgs r;
    memset(&r, 0, sizeof(r));
    r.Kt = Kt; r.ldk = (size_t)g->Npad; r.Vt = Vt; r.ldv = (size_t)g->Npad;
    r.alphaY = g->alphaY.p; r.alpha1 = g->alpha1.p; r.Q = Q; r.D = g->D; r.prior = prior_of(g);
    r.N = g->N; r.K = g->N; r.m = m; r.noise = g->noise; r.clamp_lo = clamp_lo;
    return r;
}

// Candidates per chunk: the option rounded up to 256, or what keeps K*, V^T and the cross block (cross_width doubles a candidate) at
// 256 MiB each, rounded down to 256; at least 256.
static int64_t chunk_length(int opt, int Npad, size_t cross_width)
{
    const size_t lim = (size_t)256 << 20;
    const int64_t mc = opt > 0 ? (int64_t)opt : (int64_t)std::min(lim / ((size_t)Npad * sizeof(double)), lim / (cross_width * sizeof(double)));
    return std::min<int64_t>(std::max<int64_t>((mc + (opt > 0 ? 255 : 0)) / 256 * 256, 256), 65280);      // (cov_kstar_kernel: one grid row per point, at most 65535)
}

int RowPipeline::begin(ibo_gp *gp, double clamp, int chunk_opt, size_t cross_width, size_t ld, bool q_kept, bool timing, double *ms)
{
    g = gp; clamp_lo = clamp; ldx = ld; keep_q = q_kept;
    IBO_TRY(clock.make(g->stream, ms, timing));
    mc = chunk_length(chunk_opt, g->Npad, cross_width);
    return IBO_OK;
}

int RowPipeline::reserve(int64_t m, bool need_cand, bool need_val)
{
    const size_t mp = (size_t)round_up((int)std::min(m, mc), IBO_COV_TILE), Np = (size_t)g->Npad;
    if (need_cand) IBO_TRY(cand.ensure(mp * g->D));
    if (need_val) IBO_TRY(val.ensure(mp));
    IBO_TRY(kt.ensure(mp * Np)); IBO_TRY(vt.ensure(mp * Np));
    if (ldx) IBO_TRY(cross.ensure(mp * ldx));
    IBO_TRY(mu.ensure(mp));
    if (keep_q) IBO_TRY(q.ensure(mp));
    return s2.ensure(mp);
}

int RowPipeline::chunk(int m, const double *pts, double *out)
{
    const int N = g->N, Np = g->Npad, mp = round_up(m, IBO_COV_TILE);
    hipStream_t s = g->stream;
    IBO_TRY(clock.mark(0));
    if (kstar) IBO_TRY(kstar(pts, m, mp, kt.p, s));
    else KERNEL_TRY(launch_cov_kstar(g->kp, g->Xp.p, N, Np, g->DP, pts, m, mp, kt.p, s));
    IBO_TRY(clock.mark(1));
    KERNEL_TRY(launch_cov_tri(kt.p, (size_t)Np, g->W.p, (size_t)Np, N, mp, Np, vt.p, (size_t)Np, s));
    IBO_TRY(clock.mark(2));
    KgRowsArgs r = rows_args(g, kt.p, vt.p, pts, m, clamp_lo);
    r.mu = mu.p; r.q = keep_q ? q.p : nullptr; r.s2 = s2.p;
    KERNEL_TRY(launch_kg_rows(r, s));
    IBO_TRY(clock.mark(3));
    IBO_TRY(tail(m, mp, pts, out));
    if (clock.on) {
        HIP_TRY(hipStreamSynchronize(s));
        for (int k = 0; k < 5; k++) {
            if (ST_KSTAR + k == ST_CROSS && !ldx) continue;      // no cross block, no cross launch: the gap between two marks is no stage (the slot stays 0)
            IBO_TRY(clock.account(k, k + 1, ST_KSTAR + k));
        }
    }
    return IBO_OK;
}

int RowPipeline::eval_host(int64_t M, const double *Q_host, double *val_host, double *mu_host, double *s2_host, double *x_host, size_t ncols)
{
    const size_t D = (size_t)g->D;
    hipStream_t s = g->stream;
    IBO_TRY(reserve(M, true, true));
    for (int64_t c0 = 0; c0 < M; c0 += mc) {
        const int m = (int)std::min(M - c0, mc);
        HIP_TRY(hipMemcpyAsync(cand.p, Q_host + (size_t)c0 * D, sizeof(double) * m * D, hipMemcpyHostToDevice, s));
        IBO_TRY(chunk(m, cand.p, val.p));
        if (val_host) HIP_TRY(hipMemcpyAsync(val_host + c0, val.p, sizeof(double) * m, hipMemcpyDeviceToHost, s));
        if (mu_host) HIP_TRY(hipMemcpyAsync(mu_host + c0, mu.p, sizeof(double) * m, hipMemcpyDeviceToHost, s));
        if (s2_host) HIP_TRY(hipMemcpyAsync(s2_host + c0, s2.p, sizeof(double) * m, hipMemcpyDeviceToHost, s));
        if (x_host && ncols > 0) HIP_TRY(hipMemcpy2DAsync(x_host + (size_t)c0 * ncols, sizeof(double) * ncols, cross.p, sizeof(double) * ldx,
                                                          sizeof(double) * ncols, (size_t)m, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
    }
    return IBO_OK;
}

int RowPipeline::sweep(int64_t M, const double *cand_dev, int64_t index_base, double *out_dev, double *best_val, int64_t *best_idx)
{
    hipStream_t s = g->stream;
    IBO_TRY(reserve(M, false, out_dev == nullptr));
    const int64_t nblk = (M + 255) / 256;
    ScopedBuf<double> pv;
    ScopedBuf<int64_t> pi;
    const bool want_best = best_val || best_idx;
    if (want_best) { IBO_TRY(pv.ensure((size_t)nblk)); IBO_TRY(pi.ensure((size_t)nblk)); }
    for (int64_t c0 = 0; c0 < M; c0 += mc) {                 // (one stream: a chunk's kernels start after the last chunk's have read the scratch)
        const int m = (int)std::min(M - c0, mc);
        double *out = out_dev ? out_dev + c0 : val.p;
        IBO_TRY(chunk(m, cand_dev + (size_t)c0 * g->D, out));
        if (want_best) KERNEL_TRY(launch_kg_argmax(out, m, c0, index_base, pv.p + c0 / 256, pi.p + c0 / 256, s));
    }
    if (want_best) IBO_TRY(argmax_readback(g, pv.p, pi.p, nblk, best_val, best_idx));
    return finish_span(g);                                   // (waits for the stream: the scratch goes back to the pool after it)
}

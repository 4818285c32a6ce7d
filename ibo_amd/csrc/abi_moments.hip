// abi_moments.hip -- the moments pipeline behind ibo_cacq_sweep, ibo_ehvi_*, ibo_mes_* and the evaluating ibo_sgp_* entries
// (abi_moments.h): no entry of its own.  Every entry of those units sends its candidates through MomentsPipeline::chunks, and a short
// launch runs in the size class of the call's chunk: that is why a candidate's value is the same bits from a sweep, a host batch, the
// gradient's value and a DIRECT batch, whatever the chunk.
//
// The stream rule.  The finish runs on the home stream, the sweeps on their handles' streams, and all of them share the scratch and, for
// a padded tail, the copy of the rows.  So a slot whose stream is not home's is waited for after its sweep; and if there is such a slot,
// home's stream is waited for after the padded copy (the foreign sweep reads it) and between chunks (the next chunk's foreign sweep
// writes the scratch the finish is reading).  With every slot on home's stream the stream's own order does all of this, and nothing waits.
#include "abi_moments.h"

int64_t moments_chunk_length(int64_t M, int64_t bytes_per_candidate, int chunk_opt, int64_t budget)
{
    int64_t mc = (budget / bytes_per_candidate) / 256 * 256;
    if (mc < 256) mc = 256;
    if (chunk_opt > 0) mc = ((int64_t)chunk_opt + 255) / 256 * 256;
    return M <= mc ? M : mc;
}

void MomentsPipeline::add(ibo_gp *g, bool mu, bool s2, double clamp_lo, int erf_mode, bool on)
{
    MomentSlot &sl = slot[nslots++];
    sl.g = g; sl.mu = mu; sl.s2 = s2; sl.clamp_lo = clamp_lo; sl.erf_mode = erf_mode; sl.on = on;
}

bool MomentsPipeline::foreign() const
{
    for (int i = 0; i < nslots; i++)
        if (slot[i].on && slot[i].g->stream != home->stream) return true;
    return false;
}

int MomentsPipeline::begin(int64_t M)
{
    int narrays = 0;
    for (int i = 0; i < nslots; i++) narrays += (slot[i].mu ? 1 : 0) + (slot[i].s2 ? 1 : 0);
    mc = moments_chunk_length(M, 8 * (int64_t)narrays, chunk_opt);
    stride = padded ? class_padded(mc, mc) : mc;               // (every launch of the call fits: a tail is padded to at most mc's own size class)
    IBO_TRY(ms.ensure((size_t)narrays * (size_t)stride));
    return clock.make(timing);
}

int MomentsPipeline::chunks(int64_t M, const double *cand_dev, int64_t cand_rows, FinishTail tail, double *pv, int64_t *pi)
{
    hipStream_t s = home->stream;
    const int D = home->D;
    const bool other = foreign();
    hipStream_t s_first = s;
    for (int i = nslots - 1; i >= 0; i--)
        if (slot[i].on) s_first = slot[i].g->stream;
    MomentChunk c;
    c.ms = ms.p; c.stride = stride;
    tail.D = D;
    for (int64_t c0 = 0; c0 < M; c0 += mc) {
        const int64_t m = M - c0 < mc ? M - c0 : mc, mp = padded ? class_padded(m, mc) : m;
        const double *rows = cand_dev + c0 * D;
        if (c0 + mp > cand_rows) {                               // a short launch of the caller's array: its candidates, then points at the origin
            IBO_TRY(pad.ensure((size_t)mp * D));
            HIP_TRY(hipMemcpyAsync(pad.p, rows, sizeof(double) * (size_t)m * D, hipMemcpyDeviceToDevice, s));
            HIP_TRY(hipMemsetAsync(pad.p + (size_t)m * D, 0, sizeof(double) * (size_t)(mp - m) * D, s));
            if (other) HIP_TRY(hipStreamSynchronize(s));
            rows = pad.p;
        }
        if (sweeps_ms) IBO_TRY(clock.start(s_first));
        double *next = ms.p;
        for (int i = 0; i < nslots; i++) {
            const MomentSlot &sl = slot[i];
            SweepRequest r;
            r.M = mp; r.cand_dev = rows; r.acq = IBO_ACQ_NONE; r.erf_mode = sl.erf_mode; r.clamp_lo = sl.clamp_lo;
            if (sl.mu) { r.mu_dev = next; next += stride; }
            if (sl.s2) { r.s2_dev = next; next += stride; }
            if (!sl.on) continue;
            IBO_TRY(run_sweep(sl.g, r));
            if (sl.g->stream != s) HIP_TRY(hipStreamSynchronize(sl.g->stream));
        }
        if (sweeps_ms && clock.on) { HIP_TRY(hipStreamSynchronize(s)); IBO_TRY(clock.stop(s_first, sweeps_ms)); }
        c.m = m; c.c0 = c0; c.rows = rows;
        tail.M = m; tail.first = c0; tail.cand = rows;
        tail.part_val = pv ? pv + c0 / 256 : nullptr; tail.part_idx = pi ? pi + c0 / 256 : nullptr;
        c.tail = tail;
        if (finish_ms) IBO_TRY(clock.start(s));
        IBO_TRY(finish(c, s));
        if (finish_ms) IBO_TRY(clock.stop(s, finish_ms));
        if (other && c0 + mc < M) HIP_TRY(hipStreamSynchronize(s));
    }
    return IBO_OK;
}

int MomentsPipeline::sweep(int64_t M, const double *cand_dev, int64_t cand_rows, int n_excl, const double *excl_host, double excl_radius,
                           int64_t index_base, double *best_val, int64_t *best_idx)
{
    FinishTail tail;
    memset(&tail, 0, sizeof(tail));
    tail.index_base = index_base; tail.excl_radius = excl_radius;
    IBO_TRY(upload_exclusions(home, n_excl, excl_host, &tail.n_excl, &tail.excl));
    IBO_TRY(begin(M));
    const int64_t nblk = (M + 255) / 256;
    ScopedBuf<double> pv;
    ScopedBuf<int64_t> pi;
    IBO_TRY(pv.ensure((size_t)nblk)); IBO_TRY(pi.ensure((size_t)nblk));
    IBO_TRY(chunks(M, cand_dev, cand_rows, tail, pv.p, pi.p));
    if (best_val || best_idx) return argmax_readback(home, pv.p, pi.p, nblk, best_val, best_idx);
    HIP_TRY(hipStreamSynchronize(home->stream));                 // (the scratch goes back to the pool after it)
    return IBO_OK;
}

int MomentsPipeline::eval_host(int64_t M, const double *Q_host, int k, double *const *host, const size_t *len)
{
    const size_t m = (size_t)M, D = (size_t)home->D;
    hipStream_t s = home->stream;
    const size_t rows = (size_t)class_padded(M, M);              // (a short batch carries its padding: no copy on the device)
    size_t total = 0;
    for (int i = 0; i < k; i++) total += len[i];
    ScopedBuf<double> q, res;
    IBO_TRY(q.ensure(rows * D)); IBO_TRY(res.ensure(total));
    HIP_TRY(hipMemcpyAsync(q.p, Q_host, sizeof(double) * m * D, hipMemcpyHostToDevice, s));
    if (rows > m) HIP_TRY(hipMemsetAsync(q.p + m * D, 0, sizeof(double) * (rows - m) * D, s));
    if (foreign()) HIP_TRY(hipStreamSynchronize(s));             // (a foreign sweep reads them on its own stream)
    double *at = res.p;
    for (int i = 0; i < k; at += len[i], i++) out[i] = host[i] ? at : nullptr;
    IBO_TRY(sweep(M, q.p, (int64_t)rows, 0, nullptr, 0.0, 0, nullptr, nullptr));
    for (int i = 0; i < k; i++)
        if (host[i]) HIP_TRY(hipMemcpyAsync(host[i], out[i], sizeof(double) * len[i], hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return IBO_OK;
}

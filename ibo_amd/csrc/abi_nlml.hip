// abi_nlml.hip -- the marginal-likelihood side of the C ABI: the batched theta-grid, one value + gradient (of the plain model, of leave-one-out
// and of the gradient-observation model) and ibo_trim (which owns their per-device workspaces).
#include "abi_factor.h"
#include "abi_eval.h"       // (the stage clock)
#include "loo.h"
#include "gradobs.h"

// ------------------------------------------------------------------------ marginal-likelihood grid
struct NlmlWorkspace {
    DevBuf<double> dX, dY, dout, dL, d64, dP;       // dP: packed store of the trailing updates (update3.hip)
    DevBuf<KParams> dkp;                            // the theta-points' kernel parameters (one covariance launch per sub-batch)
    DevBuf<int> dinfo, dflags;                      // dflags: four hand-over words per matrix (chol_panel_fused_kernel)
    const double *padded = nullptr;                 // dL as it was when its matrices got their identity pad,
    int pad_Np = 0, pad_N = 0, pad_B = 0;           // and for which geometry
    hipStream_t streams[4] = {nullptr, nullptr, nullptr, nullptr};     // sub-batches of a grid run side by side (created on first use, kept)
    hipEvent_t t0[4] = {nullptr, nullptr, nullptr, nullptr}, t1[4] = {nullptr, nullptr, nullptr, nullptr};     // a sub-batch's span on its stream (ibo_gpu_time_ms)
    void release()                                  // (ibo_trim; the streams and events are its own business)
    { for (DevBuf<double> *b : {&dX, &dY, &dout, &dL, &d64, &dP}) b->release(); dinfo.release(); dflags.release(); dkp.release(); padded = nullptr; }
};
static NlmlWorkspace g_nlml_ws[16];
static const int kSyrk3From = 1792;          // rows from which ibo_nlml_grad forms K^-1 = W^T W on the packed-operand kernel (launch_syrk3)
// data a learning loop sends dozens of times (the same X and Y with another theta): kept on the device with a host mirror, compared by content
struct Resident {
    DevBuf<double> d;
    std::vector<double> host;                       // what d holds (np doubles), or empty: nothing known
    // d = the n values at src, zeros behind them up to np; uploaded unless the mirror has np entries of which the first n are src's
    int put(const double *src, size_t n, size_t np)
    {
        IBO_TRY(d.ensure(np));
        if (host.size() == np && memcmp(host.data(), src, sizeof(double) * n) == 0) return IBO_OK;
        std::vector<double> v(np, 0.0);
        memcpy(v.data(), src, sizeof(double) * n);
        host.clear();                               // (not valid while the copy is in flight or if it fails)
        HIP_TRY(hipMemcpy(d.p, v.data(), sizeof(double) * np, hipMemcpyHostToDevice));
        host.swap(v);
        return IBO_OK;
    }
    void release() { d.release(); host.clear(); }   // (nothing of this data is on the device any more)
};
struct GradWorkspace {
    DevBuf<double> dL, dW, dT, dKi, d64, dal, da1, tmp, dpart, dout, dpiece, tall, Pk2;     // tall, Pk2: the super-panel order's (launch_cholesky_super)
    DevBuf<double> lpart, lout, lmu;                // ibo_loo_grad: one pass' partial sums, [gradient, value], [mu_-i, s2_-i]
    DevBuf<int> dinfo, dtasks, dsums;
    int plan_Np = 0, ntasks = 0, nsums = 0;         // launch_syrk3's lists on the device, for this Npad
    hipEvent_t t0 = nullptr, t1 = nullptr;          // the evaluation's span on the device (ibo_gpu_time_ms)
    Resident X, Y;                                  // the plain entries' data: N x D; the targets, padded to the frame
    double *pin = nullptr;                          // kGradPin doubles: the results come back through it, the info word at kGradPinInfo, behind ONE synchronisation
    // ibo_ggp_nlml_grad's data, in buffers of their own: the plain entries' resident X and Y are never touched
    Resident gX, gT, gN;                            // X, the interleaved targets (padded), gnoise
    DevBuf<double> gpart, gout;                     // the contraction's partial sums, the results
    void release()                                  // (ibo_trim; the events stay, the pinned block is its own business)
    {
        for (DevBuf<double> *b : {&dL, &dW, &dT, &dKi, &d64, &dal, &da1, &tmp, &dpart, &dout, &dpiece, &tall, &Pk2, &lpart, &lout, &lmu, &gpart, &gout}) b->release();
        for (DevBuf<int> *b : {&dinfo, &dtasks, &dsums}) b->release();
        for (Resident *r : {&X, &Y, &gX, &gT, &gN}) r->release();
        plan_Np = 0;                                // (launch_syrk3's lists went with dtasks / dsums)
    }
};
static const int kGradPin = 2 * IBO_GRAD_MAX + 8, kGradPinInfo = 2 * IBO_GRAD_MAX + 6;     // (ibo_ggp_nlml_grad: ngrad + 1 + D + 2 results)
static GradWorkspace g_grad_ws[16];

extern "C" int ibo_trim(int device)
{
    IBO_TRY(use_device(device));
    std::lock_guard<std::mutex> lk(g_dev_mu[device & 15]);
    NlmlWorkspace &ws = g_nlml_ws[device & 15];
    ws.release();
    for (int g = 0; g < 4; g++) if (ws.streams[g]) {
        (void)hipStreamDestroy(ws.streams[g]); ws.streams[g] = nullptr;
        if (ws.t0[g]) { (void)hipEventDestroy(ws.t0[g]); (void)hipEventDestroy(ws.t1[g]); ws.t0[g] = ws.t1[g] = nullptr; }
    }
    GradWorkspace &gw = g_grad_ws[device & 15];
    gw.release();
    if (gw.pin) { (void)hipHostFree(gw.pin); gw.pin = nullptr; }
    sgp_grad_trim(device);                           // (ibo_sgp_nlml_grad's private handle)
    pool_trim(device);
    return IBO_OK;
}

extern "C" int ibo_nlml_grid(int device, int ktype, int N, int D, const double *X, const double *Y,
                             int n_theta, const double *thetas, int nhyper, const double *sf2s, double noise,
                             double *nlml_host)
{
    if (!X || !Y || !thetas || !nlml_host || N < 1 || n_theta < 1) return fail(IBO_ERR_ARG, "bad argument");
    IBO_TRY(use_device(device));
    std::lock_guard<std::mutex> lk(g_dev_mu[device & 15]);      // the batch workspace is per device: concurrent grids take turns
    const int Np = round_up(N + 1, 64);            // room for the appended y row (see aug_row_kernel)
    // theta-points are independent and one factorisation is a latency-bound chain of small kernels:
    // B matrices sit side by side in HBM (B x 8 Np^2 bytes -- 4.4 GB for 32 x N=4096, nothing on a 288 GB
    // part) and every launch of the chain works on all of them (blockIdx.z), so the chain's latency is
    // paid once per batch and the update kernels fill the chip.
    const size_t nn = (size_t)Np * Np;
    int B;
    {
        const size_t budget = (size_t)12 << 30;    // bytes of factor storage per batch (of 288 GB)
        size_t fit = budget / (nn * sizeof(double));
        if (fit < 1) fit = 1;
        if (fit > 256) fit = 256;                   // N = 4096: 64 matrices side by side 0.617 ms per theta, 32: 0.655, 16: 0.72; N = 1024: 256: 45 us, 32: 69 us
        B = g_nlml_batch > 0 ? g_nlml_batch.load() : (int)fit;
        if (B > n_theta) B = n_theta;
    }
    // the workspace is kept between calls (hyper-parameter learning calls this in a loop and allocating and
    // freeing gigabytes costs more than the factorisations); ibo_trim() gives it back
    NlmlWorkspace &ws = g_nlml_ws[device & 15];
    DevBuf<double> &dX = ws.dX, &dY = ws.dY, &dout = ws.dout, &dL = ws.dL, &d64 = ws.d64;
    DevBuf<int> &dinfo = ws.dinfo;
    hipStream_t s = nullptr;
    IBO_TRY(dX.ensure((size_t)N * D)); IBO_TRY(dY.ensure(N));
    IBO_TRY(dout.ensure(2 * (size_t)n_theta)); IBO_TRY(dinfo.ensure(n_theta));
    IBO_TRY(dL.ensure(nn * B)); IBO_TRY(d64.ensure(diag64_size(Np) * B));
    // packed operands of the trailing updates, per matrix: the factor's finished columns in fragment order (update3.hip; the
    // right-looking A/B order writes and reads one panel of it at a time)
    const bool left = g_chol_left != 0;
    const size_t pws = nn;
    IBO_TRY(ws.dP.ensure(pws * B));
    IBO_TRY(ws.dflags.ensure((size_t)4 * B));
    HIP_TRY(hipMemcpy(dX.p, X, sizeof(double) * N * D, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(dY.p, Y, sizeof(double) * N, hipMemcpyHostToDevice));
    // identity pad once: the factorisation leaves the pad rows/columns as it found them, so the workspace of an
    // earlier call with the same geometry still has them (a learning loop calls this again and again)
    if (ws.padded != dL.p || ws.pad_Np != Np || ws.pad_N != N || ws.pad_B < B) {
        for (int k = 0; k < B; k++) KERNEL_TRY(launch_pad_copy(dX.p, 0, 1, dL.p + nn * k, Np, 1.0, s));
        ws.padded = dL.p; ws.pad_Np = Np; ws.pad_N = N; ws.pad_B = B;
    }
    // every theta-point's kernel parameters go up once; a sub-batch's covariance matrices are one launch
    std::vector<KParams> kps(n_theta);
    for (int t = 0; t < n_theta; t++)
        IBO_TRY(make_kparams(ktype, D, thetas + (size_t)t * nhyper, nhyper, sf2s ? sf2s[t] : 1.0, &kps[t]));
    // the covariance pass forms the exponent on the MFMA unit (cov_grid_mfma_kernel) where every scaled point of every theta-point stays
    // within the dot form's accuracy guard: |x~|^2 <= sum_d w_d max_k x_kd^2 <= IBO_DOT_GUARD_NLML (ibo_set_option("dot_form", 0) keeps the difference form)
    int dot_ok = g_dot_override.load() != 0 && D <= IBO_DDOT;
    if (dot_ok) {
        std::vector<double> xm(D, 0.0);
        for (int i = 0; i < N; i++)
            for (int d = 0; d < D; d++) { const double v = X[(size_t)i * D + d] * X[(size_t)i * D + d]; if (v > xm[d]) xm[d] = v; }
        for (int t = 0; t < n_theta && dot_ok; t++) {
            double b = 0.0;
            for (int d = 0; d < D; d++) b += kps[t].w[d] * xm[d];
            if (!(b <= IBO_DOT_GUARD_NLML)) dot_ok = 0;
        }
    }
    IBO_TRY(ws.dkp.ensure(n_theta));
    HIP_TRY(hipMemcpy(ws.dkp.p, kps.data(), sizeof(KParams) * n_theta, hipMemcpyHostToDevice));
    HIP_TRY(hipStreamSynchronize(s));               // the identity pad is in place before the sub-batches' streams start
    // Whatever way this function is left, nothing of it stays in flight on the sub-batch streams: they are non-blocking, so the next
    // call's blocking copies into dX / dY / dkp would not wait for them (an error return inside the batch loop used to leave them running).
    struct StreamDrain {
        NlmlWorkspace &w;
        ~StreamDrain() { for (int g = 0; g < 4; g++) if (w.streams[g]) (void)hipStreamSynchronize(w.streams[g]); }
    } drain{ws};
    std::vector<int> info(n_theta);
    for (int t0 = 0; t0 < n_theta; t0 += B) {
        const int nb = n_theta - t0 < B ? n_theta - t0 : B;
        // One batch.  with_flags: the panels' diagonal blocks and the rows below them in one launch whose row workgroups wait on flags the
        // diagonal workgroups raise (chol_panel_fused_kernel).  Such a wait is bounded; if one ever runs out (the launch's forward progress
        // rests on the dispatch order of its workgroups) the workgroup leaves the code kPanelWaitTimeout in the matrix's info word -- which
        // says nothing about the matrix: the batch is then run again through the two-launch form of the panels (no waits, the same bits).
        auto run_batch = [&](bool with_flags) -> int {
            // sub-batches of at least 8 matrices, each on its own stream: one's in-panel chain (64 workgroups at a time, latency)
            // and launch tails run beside the other's long-K updates
            int G = left ? g_nlml_groups.load() : 1;
            while (G > 1 && nb / G < 8) G--;
            CholGroup grp[4];
            for (int g = 0; g < G; g++) {
                if (!ws.streams[g]) {
                    // a sub-batch's stream must run BESIDE the others': a new stream may share a hardware queue with one of them
                    // (assemble.hip: streams_run_side_by_side) -- then another is made, the rejected ones given back afterwards
                    hipStream_t rejected[6];
                    int nrej = 0;
                    for (;;) {
                        hipStream_t cand = nullptr;
                        HIP_TRY(hipStreamCreateWithFlags(&cand, hipStreamNonBlocking));
                        bool ok = true;
                        for (int g2 = 0; g2 < g && ok; g2++) KERNEL_TRY(streams_run_side_by_side(ws.streams[g2], cand, &ok));
                        if (ok || nrej == 6) { ws.streams[g] = cand; break; }
                        rejected[nrej++] = cand;
                    }
                    if (getenv("IBO_DEBUG")) fprintf(stderr, "[libibo_hip] sub-batch stream %d: %d candidate(s) shared a hardware queue with an earlier one%s\n", g, nrej, nrej == 6 ? " -- none found that does not" : "");
                    for (int r = 0; r < nrej; r++) (void)hipStreamDestroy(rejected[r]);
                }
                if (!ws.t0[g]) { HIP_TRY(hipEventCreate(&ws.t0[g])); HIP_TRY(hipEventCreate(&ws.t1[g])); }
                hipStream_t sg = ws.streams[g];
                HIP_TRY(hipEventRecord(ws.t0[g], sg));
                const int k0 = (int)((long long)nb * g / G), k1 = (int)((long long)nb * (g + 1) / G), ng = k1 - k0;
                grp[g] = CholGroup{dL.p + nn * k0, d64.p + diag64_size(Np) * k0, ws.dP.p + pws * k0, dinfo.p + t0 + k0, ng, sg,
                                   with_flags ? ws.dflags.p + 4 * k0 : nullptr};
                KERNEL_TRY(launch_cov_matrix_batched(ws.dkp.p + t0 + k0, ng, N, dX.p, D, IBO_DIAG_KERNEL_PLUS_NOISE, noise, dL.p + nn * k0, Np, nn, sg, dot_ok));
                KERNEL_TRY(launch_nlml_aug(dL.p + nn * k0, Np, N, dY.p, sg, ng, nn));
            }
            // (N a multiple of 64: the y row sits alone in the last block column, whose factor nobody reads -- it is left out)
            if (left) KERNEL_TRY(launch_cholesky_batched_left(grp, G, Np, nn, 4, pws, N + 1, N % 64 == 0 ? Np / 64 - 1 : Np / 64, N / 64));
            else KERNEL_TRY(launch_cholesky_batched(grp[0].L, Np, grp[0].diag64, grp[0].info, grp[0].batch, nn, 4, grp[0].stream, grp[0].Pk, pws));      // (G = 1)
            for (int g = 0; g < G; g++) {
                KERNEL_TRY(launch_nlml_reduce(grp[g].L, Np, N, dout.p + 2 * (size_t)(grp[g].info - dinfo.p), grp[g].stream, grp[g].batch, nn));
                HIP_TRY(hipEventRecord(ws.t1[g], grp[g].stream));
            }
            float span = 0.f;
            for (int g = 0; g < G; g++) {
                HIP_TRY(hipStreamSynchronize(ws.streams[g]));      // the next batch reuses the matrix slots
                float ms = 0.f;
                if (hipEventElapsedTime(&ms, ws.t0[g], ws.t1[g]) == hipSuccess && ms > span) span = ms;
            }
            gpu_time_add(device, span);                            // (the sub-batches run side by side: the longest span, not the sum)
            HIP_TRY(hipMemcpy(info.data() + t0, dinfo.p + t0, sizeof(int) * nb, hipMemcpyDeviceToHost));
            return IBO_OK;
        };
        IBO_TRY(run_batch(true));
        bool timed_out = false;
        for (int k = 0; k < nb; k++) timed_out |= info[t0 + k] == kPanelWaitTimeout;
        if (timed_out) {
            // (the matrices were overwritten by the failed attempt: run_batch forms them again; the identity pad is untouched by a factorisation)
            IBO_TRY(run_batch(false));
            for (int k = 0; k < nb; k++)
                if (info[t0 + k] == kPanelWaitTimeout) return fail(IBO_ERR_HIP, "a panel launch reported a wait that ran out on the path that has no waits");
        }
    }
    HIP_TRY(hipStreamSynchronize(s));
    std::vector<double> out(2 * (size_t)n_theta);
    HIP_TRY(hipMemcpy(out.data(), dout.p, sizeof(double) * out.size(), hipMemcpyDeviceToHost));
    const double half_log_2pi_n = 0.5 * N * log(2.0 * M_PI);
    for (int t = 0; t < n_theta; t++)
        nlml_host[t] = info[t] ? NAN : 0.5 * out[2 * t] + out[2 * t + 1] + half_log_2pi_n;
    return IBO_OK;
}

// The frame of one evaluation on the device's GradWorkspace (the caller holds its mutex): the buffers of an Np-row factorisation, the pinned
// result block and the fit's frame for Np rows (fit_frame, abi_factor.h) -- the matrix in dT, the factor into dL, (L^-1)^T (or the doubling's
// scratch) in dKi, W into dW -- no packed copy: nothing sweeps here; the two-level order is lent no packed-update store.
static int grad_frame(GradWorkspace &ws, int Np, FactorRoute *route, FactorBufs *b)
{
    const size_t nn = (size_t)Np * Np;
    // workspace kept between calls (BFGS calls this dozens of times; five N^2 buffers allocated and freed per
    // call cost as much as the arithmetic); ibo_trim() releases it
    IBO_TRY(ws.dL.ensure(nn)); IBO_TRY(ws.dW.ensure(nn)); IBO_TRY(ws.dT.ensure(nn)); IBO_TRY(ws.dKi.ensure(nn)); IBO_TRY(ws.d64.ensure(diag64_size(Np)));
    IBO_TRY(ws.dal.ensure(Np)); IBO_TRY(ws.da1.ensure(Np)); IBO_TRY(ws.tmp.ensure(alpha_scratch(Np))); IBO_TRY(ws.dinfo.ensure(1));
    if (!ws.pin) {
        HIP_TRY(hipHostMalloc((void **)&ws.pin, sizeof(double) * kGradPin, hipHostMallocDefault));
        alloc_fill_host(ws.pin, sizeof(double) * kGradPin);
    }
    IBO_TRY(fit_frame(Np, ws.dT.p, ws.dL.p, ws.dW.p, ws.dKi.p, nullptr, nullptr, ws.d64.p, ws.dinfo.p, ws.tall, ws.Pk2, route, b));
    if (!ws.t0) { HIP_TRY(hipEventCreate(&ws.t0)); HIP_TRY(hipEventCreate(&ws.t1)); }
    return IBO_OK;
}

// Behind the matrix in b.A (its info word cleared): the factorisation with W riding along, alpha = A^-1 y, the two scalars (optional, device:
// (y . alpha, sum log L_ii)) and, if Kinv_out is given, K^-1 = W^T W on the route the size selects; *Kinv_out: where its lower 64 x 64 blocks
// are.  Queued on the null stream, nothing waited for.  mid (optional): recorded between alpha / the scalars and the product.
static int grad_factor(GradWorkspace &ws, FactorRoute route, const FactorBufs &b, int N, int Np, const double *y, double *scalars,
                       const double **Kinv_out, hipEvent_t mid = nullptr)
{
    hipStream_t s = nullptr;
    const bool fused = route != ROUTE_TWO_LEVEL;
    DevBuf<double> &dL = ws.dL, &dW = ws.dW, &dT = ws.dT, &dKi = ws.dKi;
    // no look at the info word until everything is queued: a failed factorisation only turns the rest into NaNs
    IBO_TRY(factor_invert(route, N, Np, b, s));
    KERNEL_TRY(launch_alpha(dW.p, N, Np, y, ws.tmp.p, ws.dal.p, ws.da1.p, s));
    if (scalars) KERNEL_TRY(launch_nlml_scalars(dL.p, Np, N, y, ws.dal.p, scalars, s));        // (y . alpha, sum log L_ii): L has been read for the last time
    if (mid) HIP_TRY(hipEventRecord(mid, s));
    if (!Kinv_out) return IBO_OK;
    // K^-1 = W^T W: with the ride-along, W^T is what the factorisation left in dKi -- no transpose; the result goes to dT, free by now
    if (fused && Np >= kSyrk3From) {
        // from 1792 rows the product runs on the packed-operand kernel (128 x 128 tiles, A fragments straight from L2), its long K ranges in pieces
        // of 256 columns below 2560 rows, 512 below 4096, 1024 from there (measured: 0.692 -> 0.668 ms per evaluation at N = 1792, 0.809 -> 0.766 at
        // 2048, 1.028 -> 1.002 at 2560, 1.436 -> 1.400 at 3072; below 1792 rows wtw_kernel's 64 x 64 tiles are as fast); the packed copy of W^T
        // goes where L was
        if (ws.plan_Np != Np) {
            std::vector<int> tasks, sums;
            int nslots = 0;
            syrk3_plan(Np, Np < 2560 ? 256 : (Np < 4096 ? 512 : 1024), tasks, sums, &nslots);
            IBO_TRY(ws.dtasks.ensure(tasks.size())); IBO_TRY(ws.dsums.ensure(sums.size() + 4)); IBO_TRY(ws.dpiece.ensure((size_t)(nslots + 1) * 16384));
            HIP_TRY(hipMemcpy(ws.dtasks.p, tasks.data(), sizeof(int) * tasks.size(), hipMemcpyHostToDevice));
            if (!sums.empty()) HIP_TRY(hipMemcpy(ws.dsums.p, sums.data(), sizeof(int) * sums.size(), hipMemcpyHostToDevice));
            ws.plan_Np = Np; ws.ntasks = (int)tasks.size() / 4; ws.nsums = (int)sums.size() / 4;
        }
        KERNEL_TRY(launch_syrk3(dKi.p, dL.p, dT.p, Np, ws.dtasks.p, ws.ntasks, ws.dsums.p, ws.nsums, ws.dpiece.p, s));
    } else if (fused) KERNEL_TRY(launch_wtw(dW.p, dKi.p, dT.p, Np, s, 1, 1));
    else KERNEL_TRY(launch_wtw(dW.p, dT.p, dKi.p, Np, s, 1));                      // (dT: scratch for W^T)
    *Kinv_out = fused ? dT.p : dKi.p;
    return IBO_OK;
}

// What the three gradient entries share, on the device's one GradWorkspace (the caller holds its mutex): the data resident, the frame of the
// N-row matrix with targets y, then -- queued on the null stream behind ws.t0, nothing waited for -- the caller's assembly into b.A and
// grad_factor.  one_pass: the assembly clears the info word and, where b.eye_ready, writes the identity to b.eye (launch_cov_fit); else the word
// is cleared here and the factorisation writes the identity.  clock: marks 0 .. 3 around assembly, factorisation with alpha, and the product.
struct ResidentPut { Resident &r; const double *src; size_t n, np; };
template <typename Assemble>
static int grad_prepare(GradWorkspace &ws, std::initializer_list<ResidentPut> data, int N, int Np, const Resident &y, bool one_pass,
                        const Assemble &assemble, StageClock &clock, double *scalars, const double **Kinv_out)
{
    for (const ResidentPut &p : data) IBO_TRY(p.r.put(p.src, p.n, p.np));
    FactorRoute route;
    FactorBufs b;
    IBO_TRY(grad_frame(ws, Np, &route, &b));
    hipStream_t s = nullptr;
    b.eye_ready = one_pass && route != ROUTE_TWO_LEVEL;
    if (!one_pass) HIP_TRY(hipMemsetAsync(ws.dinfo.p, 0, sizeof(int), s));
    HIP_TRY(hipEventRecord(ws.t0, s));
    IBO_TRY(clock.mark(0));
    IBO_TRY(assemble(b, s));
    IBO_TRY(clock.mark(1));
    IBO_TRY(grad_factor(ws, route, b, N, Np, y.d.p, scalars, Kinv_out, clock.ev[2]));
    return clock.mark(3);
}
// ibo_nlml_grad's and ibo_loo_grad's: X and Y resident, the covariance matrix by launch_cov_fit's one pass; untimed
static int plain_prepare(GradWorkspace &ws, const KParams &kp, int N, int D, const double *X, const double *Y, double noise, double *scalars,
                         const double **Kinv_out)
{
    const int Np = round_up(N, 64);
    StageClock off;                                  // (every mark a no-op)
    return grad_prepare(ws, {{ws.X, X, (size_t)N * D, (size_t)N * D}, {ws.Y, Y, (size_t)N, (size_t)Np}}, N, Np, ws.Y, true,
        [&](const FactorBufs &b, hipStream_t s) -> int {
            KERNEL_TRY(launch_cov_fit(kp, N, ws.X.d.p, D, IBO_DIAG_KERNEL_PLUS_NOISE, noise, b.A, Np, b.eye_ready ? b.eye : nullptr, ws.dinfo.p, s));
            return IBO_OK;
        }, off, scalars, Kinv_out);
}

// modes / dims -> the derivative spec the contraction kernels take (ngrad = 0: none)
static int grad_spec(int ngrad, const int *modes, const int *dims, int D, GradSpec *gs)
{
    gs->nh = ngrad;
    for (int h = 0; h < ngrad; h++) {
        if (modes[h] < 0 || modes[h] > 4 || dims[h] < 0 || dims[h] >= D) return fail(IBO_ERR_ARG, "bad derivative spec");
        gs->mode[h] = modes[h]; gs->dim[h] = dims[h];
    }
    return IBO_OK;
}

// The end of an evaluation queued behind grad_prepare: ws.t1, the `nres` result doubles and the info word through the pinned block behind ONE
// synchronisation, the span t0 -> t1 to the device's GPU time, the pivot check.  The results are then at ws.pin.
static int grad_finish(GradWorkspace &ws, int device, const double *res_dev, int nres)
{
    hipStream_t s = nullptr;
    HIP_TRY(hipEventRecord(ws.t1, s));
    HIP_TRY(hipMemcpyAsync(ws.pin, res_dev, sizeof(double) * nres, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(ws.pin + kGradPinInfo, ws.dinfo.p, sizeof(int), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    int h = 0;
    memcpy(&h, ws.pin + kGradPinInfo, sizeof(int));
    { float ms = 0.f; if (hipEventElapsedTime(&ms, ws.t0, ws.t1) == hipSuccess) gpu_time_add(device, ms); }
    return factor_info_word(h, "covariance matrix", nullptr);
}

// NLML and its gradient w.r.t. the log hyper-parameters for ONE theta: marginalLikelihood(...,
// computeGradient=True) of ego/gaussianprocess/trainhyper.py:47-75.  modes/dims describe
// Kernel.derivative(X, h) for h < ngrad (see GradSpec).
extern "C" int ibo_nlml_grad(int device, int ktype, int N, int D, const double *X, const double *Y,
                             const double *hyper, int nhyper, double sf2, double noise,
                             int ngrad, const int *modes, const int *dims, double *nlml_host, double *grad_host)
{
    if (!X || !Y || !hyper || !modes || !dims || !nlml_host || !grad_host || N < 1) return fail(IBO_ERR_ARG, "bad argument");
    if (ngrad < 1 || ngrad > IBO_GRAD_MAX) return fail(IBO_ERR_ARG, "ngrad=%d unsupported (1..%d)", ngrad, IBO_GRAD_MAX);
    IBO_TRY(use_device(device));
    std::lock_guard<std::mutex> lk(g_dev_mu[device & 15]);      // (its workspace too)
    KParams kp;
    IBO_TRY(make_kparams(ktype, D, hyper, nhyper, sf2, &kp));
    GradSpec gs;
    IBO_TRY(grad_spec(ngrad, modes, dims, D, &gs));
    const int Np = round_up(N, 64);
    const int nblk = ((N + 15) / 16) * ((N + 15) / 16);
    GradWorkspace &ws = g_grad_ws[device & 15];
    DevBuf<double> &dal = ws.dal, &dpart = ws.dpart, &dout = ws.dout;
    IBO_TRY(dpart.ensure((size_t)ngrad * nblk)); IBO_TRY(dout.ensure(ngrad + 2));
    hipStream_t s = nullptr;
    const double *Kinv = nullptr;
    IBO_TRY(plain_prepare(ws, kp, N, D, X, Y, noise, dout.p + ngrad, &Kinv));
    KERNEL_TRY(launch_nlml_grad(kp, gs, N, ws.X.d.p, D, Kinv, Np, dal.p, dpart.p, dout.p, s));
    IBO_TRY(grad_finish(ws, device, dout.p, ngrad + 2));
    const double *res = ws.pin;
    for (int i = 0; i < ngrad; i++) grad_host[i] = res[i];
    *nlml_host = 0.5 * res[ngrad] + res[ngrad + 1] + 0.5 * N * log(2.0 * M_PI);
    return IBO_OK;
}

// The leave-one-out objective (Rasmussen & Williams 5.4.2, to be minimised like the NLML), its gradient w.r.t. the log hyper-parameters and the
// leave-one-out predictions for ONE theta: ibo_nlml_grad's sequence up to K^-1 on its workspace, then loo.hip.
extern "C" int ibo_loo_grad(int device, int ktype, int N, int D, const double *X, const double *Y,
                            const double *hyper, int nhyper, double sf2, double noise,
                            int ngrad, const int *modes, const int *dims, double *nloo_host, double *grad_host, double *mu_host, double *s2_host)
{
    if (!X || !Y || !hyper || !nloo_host || N < 1) return fail(IBO_ERR_ARG, "bad argument");
    if (grad_host && (!modes || !dims)) return fail(IBO_ERR_ARG, "bad argument");
    if (grad_host && (ngrad < 1 || ngrad > IBO_GRAD_MAX)) return fail(IBO_ERR_ARG, "ngrad=%d unsupported (1..%d)", ngrad, IBO_GRAD_MAX);
    IBO_TRY(use_device(device));
    std::lock_guard<std::mutex> lk(g_dev_mu[device & 15]);      // (ibo_nlml_grad's workspace)
    KParams kp;
    IBO_TRY(make_kparams(ktype, D, hyper, nhyper, sf2, &kp));
    GradSpec gs;
    IBO_TRY(grad_spec(grad_host ? ngrad : 0, modes, dims, D, &gs));
    const int Np = round_up(N, 64);
    GradWorkspace &ws = g_grad_ws[device & 15];
    IBO_TRY(ws.lout.ensure(IBO_GRAD_MAX + 1)); IBO_TRY(ws.lmu.ensure(2 * (size_t)Np));
    if (gs.nh) IBO_TRY(ws.lpart.ensure(loo_contract_scratch(Np)));
    hipStream_t s = nullptr;
    const double *Kinv = nullptr;
    IBO_TRY(plain_prepare(ws, kp, N, D, X, Y, noise, nullptr, &Kinv));
    double *dmu = ws.lmu.p, *ds2 = ws.lmu.p + Np;
    KERNEL_TRY(launch_loo_value(Kinv, (size_t)Np, N, ws.Y.d.p, ws.dal.p, mu_host ? dmu : nullptr, s2_host ? ds2 : nullptr, ws.lout.p + IBO_GRAD_MAX, s));
    if (gs.nh) KERNEL_TRY(launch_loo_contract(kp, gs, N, Np, ws.X.d.p, D, Kinv, ws.dal.p, ws.lpart.p, ws.lout.p, s));
    IBO_TRY(grad_finish(ws, device, ws.lout.p, IBO_GRAD_MAX + 1));
    if (mu_host) HIP_TRY(hipMemcpy(mu_host, dmu, sizeof(double) * N, hipMemcpyDeviceToHost));
    if (s2_host) HIP_TRY(hipMemcpy(s2_host, ds2, sizeof(double) * N, hipMemcpyDeviceToHost));
    for (int i = 0; i < gs.nh; i++) grad_host[i] = ws.pin[i];
    *nloo_host = ws.pin[IBO_GRAD_MAX] + 0.5 * N * log(2.0 * M_PI);
    return IBO_OK;
}

// ------------------------------------------------------------------------ the gradient-observation model's marginal likelihood
static thread_local double t_ggp_grad_ms[IBO_GGP_GRAD_STAGES];

// NL = t^T A_nl^-1 t / 2 + sum log L_ii + (P / 2) log 2 pi of the N (D + 1)-row model of values and slopes, and its exact gradient (ibo_abi.h):
// the fit's assembly kernel with sf2 + noise on the value rows, grad_factor on the frame of P rows, then gradobs.hip's contraction.
extern "C" int ibo_ggp_nlml_grad(int device, int ktype, int N, int D, const double *X, const double *Y, const double *G,
                                 const double *hyper, int nhyper, double sf2, double noise, const double *gnoise,
                                 int ngrad, const int *modes, const int *dims, double *nlml_host, double *grad_host, double *grad_noise_host)
{
    IBO_TRY(use_device(device));
    if (!X || !Y || !G || !hyper || !gnoise || !nlml_host) return fail(IBO_ERR_ARG, "NULL argument");
    if (N < 1) return fail(IBO_ERR_ARG, "N=%d", N);
    if (grad_host && (!modes || !dims)) return fail(IBO_ERR_ARG, "modes / dims is NULL");
    if (grad_host && (ngrad < 1 || ngrad > IBO_GRAD_MAX)) return fail(IBO_ERR_ARG, "ngrad=%d unsupported (1..%d)", ngrad, IBO_GRAD_MAX);
    KParams kp;
    IBO_TRY(make_kparams(ktype, D, hyper, nhyper, sf2, &kp));
    if ((int64_t)N * (D + 1) > IBO_GGP_MAX_ROWS)
        return fail(IBO_ERR_ARG, "N (D + 1) = %lld rows, at most %d", (long long)N * (D + 1), IBO_GGP_MAX_ROWS);
    GradSpec gs;
    IBO_TRY(grad_spec(grad_host ? ngrad : 0, modes, dims, D, &gs));
    std::lock_guard<std::mutex> lk(g_dev_mu[device & 15]);      // (ibo_nlml_grad's workspace)
    const int B = D + 1, P = N * B, Np = round_up(P, 64);
    const bool want_grad = gs.nh > 0 || grad_noise_host;
    const int nres = gs.nh + B + 2;                              // the derivatives, the 1 + D noise terms, (t . alpha, sum log L_ii)
    GradWorkspace &ws = g_grad_ws[device & 15];
    IBO_TRY(ws.gout.ensure(kGradPin));
    if (want_grad) IBO_TRY(ws.gpart.ensure(gradobs_contract_scratch(N, D)));
    hipStream_t s = nullptr;
    std::vector<double> tp(Np, 0.0);                 // [Y; G] interleaved point by point, zero in the pad (compared over all Np)
    for (int i = 0; i < N; i++) {
        tp[(size_t)i * B] = Y[i];
        for (int d = 0; d < D; d++) tp[(size_t)i * B + 1 + d] = G[(size_t)i * D + d];
    }
    StageClock clock;
    IBO_TRY(clock.make(s, t_ggp_grad_ms, g_ggp_timing != 0));
    const double *Kinv = nullptr;
    double *res = ws.gout.p;
    IBO_TRY(grad_prepare(ws, {{ws.gX, X, (size_t)N * D, (size_t)N * D}, {ws.gT, tp.data(), (size_t)Np, (size_t)Np}, {ws.gN, gnoise, (size_t)D, (size_t)D}},
        P, Np, ws.gT, false, [&](const FactorBufs &b, hipStream_t q) -> int {
            KERNEL_TRY(launch_gradobs_assemble(kp, ws.gX.d.p, N, sf2 + noise, ws.gN.d.p, b.A, Np, q));
            return IBO_OK;
        }, clock, res + gs.nh + B, want_grad ? &Kinv : nullptr));
    if (want_grad) KERNEL_TRY(launch_gradobs_contract(kp, gs, ws.gX.d.p, N, Kinv, Np, ws.dal.p, noise, ws.gN.d.p, ws.gpart.p, res, s));
    IBO_TRY(clock.mark(4));
    const int rc = grad_finish(ws, device, res, nres);           // (synchronises; the sums are taken whatever it says, quietly: rc's text stays)
    for (int k = 0; clock.on && k < 4; k++) { float ms = 0.f; if (hipEventElapsedTime(&ms, clock.ev[k], clock.ev[k + 1]) == hipSuccess) t_ggp_grad_ms[k] += ms; }
    IBO_TRY(rc);
    const double *r = ws.pin;
    for (int i = 0; i < gs.nh; i++) grad_host[i] = r[i];
    if (grad_noise_host)
        for (int e = 0; e < B; e++) grad_noise_host[e] = r[gs.nh + e];
    *nlml_host = 0.5 * r[gs.nh + B] + r[gs.nh + B + 1] + 0.5 * P * log(2.0 * M_PI);
    return IBO_OK;
}

extern "C" int ibo_ggp_grad_stage_ms(double *ms, int reset)
{
    return read_stage_sums(t_ggp_grad_ms, IBO_GGP_GRAD_STAGES, ms, reset);
}

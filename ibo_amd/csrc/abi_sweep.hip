// abi_sweep.hip -- candidate sweeps behind the C ABI (one-shot, with kept per-candidate state, with the ranks' exchange): the routes and
// run_sweep, which every other evaluation unit calls (abi_eval.h), and the small pieces those units share with it.
#include "abi_eval.h"

// 2^(j/2048), j < 2048: the table behind sweep2's exp (one per device, created on first use)
static std::atomic<double *> g_exp_tab[16];
static std::mutex g_exp_mu;                          // held only while a device's table is being created (never across a grid or a gradient)
int exp_table(int device, const double **out)
{
    double *p = g_exp_tab[device & 15].load(std::memory_order_acquire);
    if (!p) {
        std::lock_guard<std::mutex> lk(g_exp_mu);     // created once per device, by whichever handle sweeps first
        p = g_exp_tab[device & 15].load(std::memory_order_relaxed);
        if (!p) {
            std::vector<double> h(2048);
            for (int j = 0; j < 2048; j++) h[j] = exp2((double)j / 2048.0);
            HIP_TRY(hipMalloc((void **)&p, sizeof(double) * 2048));
            HIP_TRY(hipMemcpy(p, h.data(), sizeof(double) * 2048, hipMemcpyHostToDevice));
            g_exp_tab[device & 15].store(p, std::memory_order_release);
        }
    }
    *out = p;
    return IBO_OK;
}

// ------------------------------------------------------------------------ sweep
// the part of the kernel arguments that comes from the handle alone
static void fill_model_args(const ibo_gp *g, SweepArgs &a)
{
    a.kp = g->kp; a.N = g->N; a.Npad = g->Npad; a.DP = g->DP;
    a.Xs = g->Xs.p; a.ak = g->ak.p; a.XA = g->XA.p; a.log_sf2 = log(g->kp.sf2); a.dot_form = (g_dot_override >= 0 && g->D <= IBO_DDOT) ? g_dot_override.load() : g->dot_form;
    a.Xp = g->Xp.p; a.W = g->W.p; a.Wp = g->Wp.p; a.alphaY = g->alphaY.p; a.alpha1 = g->alpha1.p;
    a.prior = prior_of(g);
    a.noise = g->noise;
}

// Which kernel serves a sweep of M candidates on a model of Npad padded rows.  dot_form: whether the dot form holds for this sweep;
// force_path: ibo_set_option("sweep_path") -- 0: by size, 1: GEMV, 3: panel-split, anything else: the large-batch kernels.
// No handle, no HIP call, no allocation: the thresholds below are all there is to it.
enum SweepRoute { ROUTE_SMALL2, ROUTE_SPLIT, ROUTE_GEMV, ROUTE_SWEEP2, ROUTE_TILE };
static int choose_route(int64_t M, int Npad, int dot_form, int force_path, SweepRoute *route)
{
    const int64_t ntiles = (M + 63) / 64;
    // batches up to 4096 candidates where the dot form holds: three short kernels spread over the chip (small2.hip;
    // from ~8192 candidates on the panel-split kernel's tiles fill the chip by themselves and it is the faster one).
    // They beat the GEMV kernel down to a single candidate (N = 2048: 22 us against 87; N = 1024: 16 against 38), which
    // is left with the models they do not take (no dot form, rows beyond sweep2's LDS budget).
    const bool small2_ok = force_path == 0 && M <= 4096 && dot_form && sweep2_fits(Npad);
    // (the GEMV kernel holds k* of a candidate in LDS: beyond 20416 rows a few candidates go to the panel-split kernel)
    const bool gemv = (force_path == 1) || (force_path == 0 && M <= 16 && !small2_ok && sweep_gemv_fits(Npad));
    if (gemv && !sweep_gemv_fits(Npad))
        return fail(IBO_ERR_ARG, "the GEMV sweep kernel holds at most 20416 rows in its 160 KiB of LDS (model: %d padded rows)", Npad);
    // small batches: spread the IBO_SPLIT_PANEL-row panels over the grid too (one tile per 64 candidates alone
    // would leave most of the 256 CUs idle); above ~128 tiles the plain kernel fills the chip
    // (4097 .. 8192 candidates are at most 256 tiles of the large-batch kernel -- one round of the chip, 134 us at N = 1024 and
    // 495 us at N = 2048 whatever their number, where the panel-split kernel takes 142 .. 221 and 478 .. 842 us)
    const bool sweep2_ok = dot_form && sweep2_fits(Npad);
    const bool split = !gemv && (force_path == 3 || (force_path == 0 && ntiles * 2 <= 256 && !(sweep2_ok && M > 4096)));
    *route = (split && small2_ok) ? ROUTE_SMALL2 : split ? ROUTE_SPLIT : gemv ? ROUTE_GEMV : sweep2_ok ? ROUTE_SWEEP2 : ROUTE_TILE;
    return IBO_OK;
}

// The diagnostic build's per-tile stamps (make stamps; tools/stamp_sweep.py, tools/stamp_sweep2.py) travel in mupart, `words` 64-bit words
// in all; after the launch they go to the file IBO_STAMP_FILE names.  The product's build has neither.
#ifdef IBO_STAMPS
static int stamps_attach(ibo_gp *g, SweepArgs &a, size_t words)
{
    IBO_TRY(g->mupart.ensure(words + 16));
    a.mupart = g->mupart.p;
    return IBO_OK;
}
static int stamps_dump(ibo_gp *g, size_t words)
{
    if (!getenv("IBO_STAMP_FILE")) return IBO_OK;
    std::vector<unsigned long long> h(words);
    HIP_TRY(hipStreamSynchronize(g->stream));
    HIP_TRY(hipMemcpy(h.data(), g->mupart.p, h.size() * 8, hipMemcpyDeviceToHost));
    FILE *f = fopen(getenv("IBO_STAMP_FILE"), "wb");
    if (f) { fwrite(h.data(), 8, h.size(), f); fclose(f); }
    return IBO_OK;
}
#else
static inline int stamps_attach(ibo_gp *, SweepArgs &, size_t) { return IBO_OK; }
static inline int stamps_dump(ibo_gp *, size_t) { return IBO_OK; }
#endif

// ---- one function per route: its buffers, its launch, the name ibo_last_sweep_kernel_ms reports
static int sweep_small2(ibo_gp *g, SweepArgs &a, const SweepRequest &r)
{
    hipStream_t s = g->stream;
    IBO_TRY(exp_table(g->device, &a.exp_tab));
    IBO_TRY(g->small_ws.ensure(small_sweep_workspace(g->Npad, a.M)));
    if (r.signal && !a.result_val) {             // (no arg-max to read back) the caller will spin on a host-visible word the last kernel writes
        if (!g->done_flag) {                     // (a recycled handle brings its flag along)
            HIP_TRY(hipHostMalloc((void **)&g->done_flag, 64, hipHostMallocDefault));
            *g->done_flag = 0;
        }
        if (!g->done_count.p) {
            IBO_TRY(g->done_count.ensure(1));
            HIP_TRY(hipMemsetAsync(g->done_count.p, 0, sizeof(unsigned), s));
        }
        a.done_flag = g->done_flag; a.done_seq = ++g->done_seq; a.done_count = g->done_count.p;
        g->signal_pending = true;
    }
    KERNEL_TRY(launch_sweep_small(a, g->small_ws.p, s, r.timed ? g->ev0 : nullptr, r.timed ? g->ev1 : nullptr));
    g->sweep_kernel = "wk_small_kernel";
    return IBO_OK;
}

static int sweep_split_or_gemv(ibo_gp *g, SweepArgs &a, bool gemv)
{
    const size_t chunks = gemv ? (size_t)(g->Npad / 64) : (size_t)((g->Npad + IBO_SPLIT_PANEL - 1) / IBO_SPLIT_PANEL);
    IBO_TRY(g->qpart.ensure(chunks * a.M)); IBO_TRY(g->mupart.ensure(2 * (size_t)a.M));
    a.qpart = g->qpart.p; a.mupart = g->mupart.p;
    if (gemv) KERNEL_TRY(launch_sweep_gemv(a, g->stream, g->ev0, g->ev1));
    else KERNEL_TRY(launch_sweep_mfma(a, g->stream, g->ev0, g->ev1));
    g->sweep_kernel = gemv ? "sweep_gemv_kernel" : "sweep_mfma_kernel<split>";
    return IBO_OK;
}

static int sweep_sweep2(ibo_gp *g, SweepArgs &a)
{
    const size_t words = (size_t)((a.M + IBO_S2_TCAND - 1) / IBO_S2_TCAND) * 8;
    IBO_TRY(exp_table(g->device, &a.exp_tab));
    IBO_TRY(g->qpart.ensure(3 * (size_t)a.M));    // (q, aY.k*, a1.k*) per candidate, finished by acq_finish_kernel
    a.qpart = g->qpart.p;
    IBO_TRY(stamps_attach(g, a, words));
    KERNEL_TRY(launch_sweep2(a, g->stream, g->ev0, g->ev1));
    g->sweep_kernel = "sweep2_kernel";
    return stamps_dump(g, words);
}

static int sweep_tile(ibo_gp *g, SweepArgs &a)
{
    const size_t words = (size_t)((a.M + 63) / 64) * 16;
    IBO_TRY(stamps_attach(g, a, words));
    a.dot_form = 0;                              // the first-generation tile kernel is kept in its difference form only
    KERNEL_TRY(launch_sweep_mfma(a, g->stream, g->ev0, g->ev1));
    g->sweep_kernel = "sweep_mfma_kernel";
    return stamps_dump(g, words);
}

// The sweep2 route of ibo_acq_sweep_incremental: the state of this candidate array is kept on the handle; if the model has only grown by a
// few rows (ibo_gp_extend) since it was formed, those rows are folded in -- O(N) per candidate, not O(N^2)
// (keyed on the array's GENERATION, not its address: see ibo_dev_alloc.  An array the library did not allocate
// has none, and is swept in full every time)
static int sweep_sweep2_kept(ibo_gp *g, SweepArgs &a, const SweepRequest &r)
{
    hipStream_t s = g->stream;
    const int64_t M = a.M;
    IBO_TRY(exp_table(g->device, &a.exp_tab));
    size_t off = 0;
    const uint64_t gen = alloc_generation(g->device, r.cand_dev, sizeof(double) * (size_t)M * g->D, &off);
    const bool usable = gen != 0 && g->st_gen == gen && g->st_off == off && g->st_M == M && g->st_epoch == g->fit_epoch && g->st_sf2 == g->kp.sf2 &&
                        g->st_N >= 1 && g->st_N <= g->N && g->N - g->st_N <= 8 && (!g->st_pruned || g->N - g->st_N0 <= 16) && g->state.cap >= 5 * (size_t)M &&
                        sweep2_rank1_fits(a.Npad, a.kp.D);
    IBO_TRY(g->state.ensure(5 * (size_t)M));     // [q_a, aY.k*, a1.k*, zsum, q_b]: q = (q_a + q_b) + zsum
    a.qpart = g->state.p;
    a.state5 = 1;
    // EI and UCB grow with the variance, and the variance computed from PART of W's rows bounds it from above: where only
    // the arg-max is wanted, the second half of W's rows (three quarters of the work) runs only for tiles whose bound can
    // still reach the best complete value (sweep2.hip: launch_sweep2_pruned).  PI and the plain mean, per-candidate
    // outputs, or a model the part kernels do not take: every tile complete, as before.
    // (UCB = mu + parm sigma grows with sigma only for parm >= 0: a caller's negative coefficient -- a lower confidence bound --
    // takes the complete-every-tile route)
    const bool monotone = (r.acq == IBO_ACQ_EI || (r.acq == IBO_ACQ_UCB && r.parm >= 0.0)) && !r.mu_dev && !r.s2_dev && !r.acq_dev;
    const int64_t nt32 = (M + IBO_S2_TCAND - 1) / IBO_S2_TCAND;
    a.part_rows = usable ? g->st_N0 : g->N;
    a.part_slack = 1e-13 * (1.0 + fabs(a.ymax) + fabs(a.parm));
    a.rank_hi = g->N; a.wy = g->tmp.p;               // (g->tmp[0 .. Npad) is W y after every fit, extension and ibo_gp_set_y)
    // Drift margin of the lazy refresh: an appended row i moves a stale candidate's mean by nu_i (W y)_i, nu = W k*.  With
    // R = sf2_fit P + (1 + noise - sf2_fit) I (P: the correlation matrix, unit diagonal -- the reference's diagonal rule) and
    // k* = sf2_k p*, R >= sf2_fit P whenever sf2_fit <= 1 + noise, hence |nu_i|^2 <= q = k*^T R^-1 k* <= sf2_k^2 / sf2_fit
    // (p*^T P^-1 p* <= 1 for a valid kernel).  1 for the squared exponentials, magnitude^2-dependent for the SV / Matern
    // kernels and under ibo_gp_set_kstar_sf2.  A model fitted with sf2_fit > 1 + noise has no such bound: never lazy.
    const bool nu_bounded = g->kp_fit.sf2 > 0.0 && g->kp_fit.sf2 <= 1.0 + g->noise;
    a.nu_max = nu_bounded ? (g->kp.sf2 / sqrt(g->kp_fit.sf2)) * (1.0 + 1e-9) : INFINITY;
    if (usable && g->st_pruned) {
        // a two-part state: its tiles fold the appended rows in lazily (launch_sweep2_refresh); a caller that needs every
        // candidate's own numbers (outputs, PI, the plain mean), the A/B switch, or a mean prior (whose second vector W 1
        // moves the means of stale tiles by more than any margin allows) has every tile refreshed and completed instead
        a.tile_done = g->tile_done.p; a.tile_ub = g->tile_ub.p; a.part_best = g->part_words.p; a.part_thresh = g->part_words.p + 1;
        a.tile_rows = g->tile_rows.p; a.tile_sel = g->tile_sel.p; a.part_nlev = g->st_nlev;
        a.part_lazy = monotone && g_gallery_prune == 1 && g->nb == 0 && nu_bounded;
    }
    if (usable) {
        KERNEL_TRY(launch_sweep2_refresh(a, g->st_N, g->N - 1, s, g->ev0, g->ev1));
        g->sweep_kernel = g->N > g->st_N ? "sweep2_rank1_kernel" : "acq_finish_kernel";
    } else if (g_gallery_prune && monotone && sweep2_part_fits(a.Npad, a.kp.D)) {
        IBO_TRY(g->tile_done.ensure((size_t)nt32)); IBO_TRY(g->tile_ub.ensure((size_t)nt32)); IBO_TRY(g->part_words.ensure(2));
        IBO_TRY(g->tile_rows.ensure((size_t)nt32)); IBO_TRY(g->tile_sel.ensure(2 * (size_t)nt32 + 16));     // flags | compact list | counters
        HIP_TRY(hipMemsetAsync(g->tile_done.p, 0, sizeof(int) * (size_t)nt32, s));
        HIP_TRY(hipMemsetAsync(g->tile_rows.p, 0, sizeof(int) * (size_t)nt32, s));
        a.tile_rows = g->tile_rows.p; a.tile_sel = g->tile_sel.p;
        HIP_TRY(hipMemsetAsync(g->state.p + 3 * (size_t)M, 0, sizeof(double) * 2 * (size_t)M, s));
        a.tile_done = g->tile_done.p; a.tile_ub = g->tile_ub.p; a.part_best = g->part_words.p; a.part_thresh = g->part_words.p + 1;
        a.part_nlev = g->st_nlev = sweep2_part_nlev(a.Npad);
        KERNEL_TRY(launch_sweep2_pruned(a, g_gallery_prune == 1, s, g->ev0, g->ev1));
        g->st_pruned = true;
        g->sweep_kernel = "sweep2_kernel<part>";
    } else {
        HIP_TRY(hipMemsetAsync(g->state.p + 3 * (size_t)M, 0, sizeof(double) * 2 * (size_t)M, s));
        KERNEL_TRY(launch_sweep2(a, s, g->ev0, g->ev1));
        g->st_pruned = false;
        g->sweep_kernel = "sweep2_kernel";
    }
    if (!usable) g->st_N0 = g->N;
    g->st_gen = gen; g->st_off = off; g->st_M = M; g->st_N = g->N; g->st_sf2 = g->kp.sf2; g->st_epoch = g->fit_epoch;
    return IBO_OK;
}

int upload_exclusions(ibo_gp *g, int n_excl, const double *excl_host, int *n, const double **ptr)
{
    if (n_excl <= 0) return IBO_OK;
    if (!excl_host) return fail(IBO_ERR_ARG, "excl_host is NULL");
    IBO_TRY(g->excl.ensure((size_t)n_excl * g->D));
    HIP_TRY(hipMemcpyAsync(g->excl.p, excl_host, sizeof(double) * n_excl * g->D, hipMemcpyHostToDevice, g->stream));
    HIP_TRY(hipStreamSynchronize(g->stream));
    *n = n_excl; *ptr = g->excl.p;
    return IBO_OK;
}

int read_result(ibo_gp *g, double *best_val, int64_t *best_idx)
{
    double hv; int64_t hi;
    HIP_TRY(hipMemcpyAsync(&hv, g->res_v.p, sizeof(double), hipMemcpyDeviceToHost, g->stream));
    HIP_TRY(hipMemcpyAsync(&hi, g->res_i.p, sizeof(int64_t), hipMemcpyDeviceToHost, g->stream));
    HIP_TRY(hipStreamSynchronize(g->stream));
    if (best_val) *best_val = hv;
    if (best_idx) *best_idx = hi;
    return IBO_OK;
}

int argmax_readback(ibo_gp *g, const double *part_val, const int64_t *part_idx, int64_t nblk, double *best_val, int64_t *best_idx)
{
    IBO_TRY(g->res_v.ensure(1)); IBO_TRY(g->res_i.ensure(1));
    SweepArgs f;
    memset(&f, 0, sizeof(f));
    f.part_val = const_cast<double *>(part_val); f.part_idx = const_cast<int64_t *>(part_idx);
    f.result_val = g->res_v.p; f.result_idx = g->res_i.p;
    KERNEL_TRY(launch_argmax_final(f, nblk, g->stream));
    return read_result(g, best_val, best_idx);
}

int finish_span(ibo_gp *g)
{
    HIP_TRY(hipEventRecord(g->ev1, g->stream));
    HIP_TRY(hipEventSynchronize(g->ev1));
    float ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms, g->ev0, g->ev1));
    gpu_time_add(g->device, ms);
    return IBO_OK;
}

int run_sweep(ibo_gp *g, const SweepRequest &r)
{
    if (!g->fitted) return fail(IBO_ERR_STATE, "sweep before a successful fit");
    if (r.M < 1 || !r.cand_dev) return fail(IBO_ERR_ARG, "empty candidate set");
    if (r.acq < 0 || r.acq > 3) return fail(IBO_ERR_ARG, "unknown acquisition %d", r.acq);
    SweepArgs a;
    memset(&a, 0, sizeof(a));
    fill_model_args(g, a);
    a.M = r.M; a.cand = r.cand_dev; a.cand_host = r.cand_host;
    a.clamp_lo = r.clamp_lo; a.ymax = (r.ymax == r.ymax) ? r.ymax : g->maxY; a.parm = r.parm;
    a.acq = r.acq; a.erf_mode = r.erf_mode;
    a.excl_radius = r.excl_radius;
    IBO_TRY(upload_exclusions(g, r.n_excl, r.excl_host, &a.n_excl, &a.excl));
    a.index_base = r.index_base;
    a.out_mu = r.mu_dev; a.out_s2 = r.s2_dev; a.out_acq = r.acq_dev;
    const int64_t ntiles = (r.M + 63) / 64;
    IBO_TRY(g->partv.ensure(2 * ntiles)); IBO_TRY(g->parti.ensure(2 * ntiles));     // sweep2 has 32-candidate tiles
    IBO_TRY(g->res_v.ensure(1)); IBO_TRY(g->res_i.ensure(1));
    a.part_val = g->partv.p; a.part_idx = g->parti.p;
    const bool want_best = r.best_val || r.best_idx || r.device_result;
    a.result_val = want_best ? g->res_v.p : nullptr; a.result_idx = want_best ? g->res_i.p : nullptr;
    SweepRoute route;
    IBO_TRY(choose_route(r.M, a.Npad, a.dot_form, g_force_path, &route));
    switch (route) {
    case ROUTE_SMALL2: IBO_TRY(sweep_small2(g, a, r)); break;
    case ROUTE_SPLIT: IBO_TRY(sweep_split_or_gemv(g, a, false)); break;
    case ROUTE_GEMV: IBO_TRY(sweep_split_or_gemv(g, a, true)); break;
    case ROUTE_SWEEP2: IBO_TRY(r.incremental ? sweep_sweep2_kept(g, a, r) : sweep_sweep2(g, a)); break;
    case ROUTE_TILE: IBO_TRY(sweep_tile(g, a)); break;
    }
    if (!r.best_val && !r.best_idx) return IBO_OK;        // internal callers that only want the per-point outputs (or the result on the device)
    IBO_TRY(read_result(g, r.best_val, r.best_idx));
    HIP_TRY(hipEventElapsedTime(&g->sweep_ms, g->ev0, g->ev1));
    gpu_time_add(g->device, g->sweep_ms);
    return IBO_OK;
}

// the leading arguments of ibo_acq_sweep, which three entry points carry in ibo_abi.h's order, as a request
static SweepRequest abi_request(int64_t M, const double *cand_dev, int acq, double parm, int erf_mode, double clamp_lo, double ymax,
                                int n_excl, const double *excl_host, double excl_radius, int64_t index_base)
{
    SweepRequest r;
    r.M = M; r.cand_dev = cand_dev; r.acq = acq; r.parm = parm; r.erf_mode = erf_mode; r.clamp_lo = clamp_lo; r.ymax = ymax;
    r.n_excl = n_excl; r.excl_host = excl_host; r.excl_radius = excl_radius; r.index_base = index_base;
    return r;
}

static int acq_sweep(bool incremental, ibo_gp *g, int64_t M, const double *cand_dev, int acq, double parm, int erf_mode,
                     double clamp_lo, double ymax, int n_excl, const double *excl_host,
                     double excl_radius, int64_t index_base, double *mu_dev, double *s2_dev,
                     double *acq_dev, double *best_val, int64_t *best_idx)
{
    if (!g) return fail(IBO_ERR_ARG, "gp is NULL");
    IBO_TRY(use_device(g->device));
    SweepRequest r = abi_request(M, cand_dev, acq, parm, erf_mode, clamp_lo, ymax, n_excl, excl_host, excl_radius, index_base);
    r.mu_dev = mu_dev; r.s2_dev = s2_dev; r.acq_dev = acq_dev; r.best_val = best_val; r.best_idx = best_idx;
    r.incremental = incremental;
    return run_sweep(g, r);
}

extern "C" int ibo_acq_sweep(ibo_gp_t *g, int64_t M, const double *cand_dev, int acq, double parm, int erf_mode,
                             double clamp_lo, double ymax, int n_excl, const double *excl_host,
                             double excl_radius, int64_t index_base, double *mu_dev, double *s2_dev,
                             double *acq_dev, double *best_val, int64_t *best_idx)
{
    return acq_sweep(false, g, M, cand_dev, acq, parm, erf_mode, clamp_lo, ymax, n_excl, excl_host, excl_radius, index_base, mu_dev, s2_dev, acq_dev, best_val, best_idx);
}

extern "C" int ibo_acq_sweep_incremental(ibo_gp_t *g, int64_t M, const double *cand_dev, int acq, double parm, int erf_mode,
                                         double clamp_lo, double ymax, int n_excl, const double *excl_host,
                                         double excl_radius, int64_t index_base, double *mu_dev, double *s2_dev,
                                         double *acq_dev, double *best_val, int64_t *best_idx)
{
    return acq_sweep(true, g, M, cand_dev, acq, parm, erf_mode, clamp_lo, ymax, n_excl, excl_host, excl_radius, index_base, mu_dev, s2_dev, acq_dev, best_val, best_idx);
}

// The sharded sweep's step in one call (the loop of ego/acquisition/gallery.py:93-134 cut over ranks): this rank's block is
// swept, the arg-max kernel's (value, global index) stay in HBM, a small kernel puts them and the winner's coordinates into the rank's
// slot of the all-reduce buffer, ncclAllReduce runs on the same stream and one copy brings every rank's slot to pinned host memory
// (csrc/comm.hip: ibo_comm_exchange_dev) -- one synchronisation per step, nothing staged through pageable memory.
extern "C" int ibo_acq_sweep_exchange(ibo_gp_t *g, ibo_comm_t *c, int incremental, int64_t M, const double *cand_dev, int acq, double parm,
                                      int erf_mode, double clamp_lo, double ymax, int n_excl, const double *excl_host, double excl_radius,
                                      int64_t index_base, double *local_val, int64_t *local_idx, double *best_val, int64_t *best_idx,
                                      double *best_x, int *best_rank)
{
    if (!g || !c) return fail(IBO_ERR_ARG, "NULL argument");
    IBO_TRY(use_device(g->device));
    SweepRequest r = abi_request(M, cand_dev, acq, parm, erf_mode, clamp_lo, ymax, n_excl, excl_host, excl_radius, index_base);
    r.incremental = incremental != 0; r.device_result = true;
    IBO_TRY(run_sweep(g, r));
    IBO_TRY(ibo_comm_exchange_dev(c, g->stream, g->res_v.p, g->res_i.p, cand_dev, g->D, index_base, local_val, local_idx, best_val, best_idx,
                                  best_x, best_rank));
    HIP_TRY(hipEventElapsedTime(&g->sweep_ms, g->ev0, g->ev1));      // (the exchange has synchronised the stream)
    gpu_time_add(g->device, g->sweep_ms);
    return IBO_OK;
}

extern "C" int ibo_sweep_state_info(ibo_gp_t *g, int64_t *tiles, int64_t *complete)
{
    if (!g) return fail(IBO_ERR_ARG, "gp is NULL");
    IBO_TRY(use_device(g->device));
    const int64_t nt = g->st_gen ? (g->st_M + IBO_S2_TCAND - 1) / IBO_S2_TCAND : 0;
    int64_t done = nt;
    if (nt && g->st_pruned) {
        std::vector<int> h((size_t)nt);
        HIP_TRY(hipStreamSynchronize(g->stream));
        HIP_TRY(hipMemcpy(h.data(), g->tile_done.p, sizeof(int) * (size_t)nt, hipMemcpyDeviceToHost));
        done = 0;
        for (int v : h) done += v == g->st_nlev - 1;
    }
    if (tiles) *tiles = nt;
    if (complete) *complete = done;
    return IBO_OK;
}

extern "C" int ibo_sweep_state_levels(ibo_gp_t *g, int *nlev, int *splits, int64_t *tiles_at_level)
{
    if (!g) return fail(IBO_ERR_ARG, "gp is NULL");
    IBO_TRY(use_device(g->device));
    const int64_t nt = g->st_gen ? (g->st_M + IBO_S2_TCAND - 1) / IBO_S2_TCAND : 0;
    const int nl = (nt && g->st_pruned) ? g->st_nlev : 1;
    if (nlev) *nlev = nl;
    if (splits) {
        int all[3];
        const int n = sweep2_part_levels(g->Npad, all) - 1;
        for (int i = 0; i < 3; i++) splits[i] = 0;
        for (int i = 0; i < nl - 1; i++) splits[i] = all[n - (nl - 1) + i];
    }
    if (tiles_at_level) {
        for (int i = 0; i < 4; i++) tiles_at_level[i] = 0;
        if (nl == 1) tiles_at_level[0] = nt;
        else {
            std::vector<int> h((size_t)nt);
            HIP_TRY(hipStreamSynchronize(g->stream));
            HIP_TRY(hipMemcpy(h.data(), g->tile_done.p, sizeof(int) * (size_t)nt, hipMemcpyDeviceToHost));
            for (int v : h) if (v >= 0 && v < 4) tiles_at_level[v]++;
        }
    }
    return IBO_OK;
}

extern "C" int ibo_last_sweep_kernel_ms(ibo_gp_t *g, float *ms, const char **kernel_name)
{
    if (!g) return fail(IBO_ERR_ARG, "gp is NULL");
    if (ms) *ms = g->sweep_ms;
    if (kernel_name) *kernel_name = g->sweep_kernel;
    return IBO_OK;
}

// abi_sweep.hip -- the evaluation side of the C ABI: candidate sweeps (one-shot and with kept per-candidate state), host batches,
// DIRECT on the GPU objective, and the constrained acquisition over several handles.
#include "abi_internal.h"
#include "grad.h"
#include "cov.h"
#include "cacq.h"

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
// What one sweep is asked for: the arguments of ibo_acq_sweep, and what the library's own callers add to them.  Lives on the caller's stack.
struct SweepRequest {
    int64_t M = 0;
    const double *cand_dev = nullptr;            // M x D, where the kernels read them (device memory, or pinned host memory)
    const double *cand_host = nullptr;           // the same candidates where the HOST can read them (pinned staging), or NULL
    int acq = IBO_ACQ_NONE, erf_mode = IBO_ERF_LIBM;
    double parm = 0.0, clamp_lo = 0.0, ymax = NAN;       // ymax NaN: the model's largest observation
    int n_excl = 0; const double *excl_host = nullptr; double excl_radius = 0.0;
    int64_t index_base = 0;
    double *mu_dev = nullptr, *s2_dev = nullptr, *acq_dev = nullptr;     // per-candidate outputs, optional
    double *best_val = nullptr; int64_t *best_idx = nullptr;             // the arg-max, on the host (both NULL: no read-back, no synchronisation)
    bool incremental = false;                    // keep the candidates' state on the handle (ibo_acq_sweep_incremental)
    bool timed = true;                           // kernel-time events around the launches (small2.hip's only: the others always record them)
    bool signal = false;                         // the caller will spin on the handle's host-visible word instead of an event, where the route can write it
    bool device_result = false;                  // (value, index) stay in res_v / res_i for the exchange
};

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

static int run_sweep(ibo_gp *g, const SweepRequest &r)
{
    if (!g->fitted) return fail(IBO_ERR_STATE, "sweep before a successful fit");
    if (r.M < 1 || !r.cand_dev) return fail(IBO_ERR_ARG, "empty candidate set");
    if (r.acq < 0 || r.acq > 3) return fail(IBO_ERR_ARG, "unknown acquisition %d", r.acq);
    hipStream_t s = g->stream;
    SweepArgs a;
    memset(&a, 0, sizeof(a));
    fill_model_args(g, a);
    a.M = r.M; a.cand = r.cand_dev; a.cand_host = r.cand_host;
    a.clamp_lo = r.clamp_lo; a.ymax = (r.ymax == r.ymax) ? r.ymax : g->maxY; a.parm = r.parm;
    a.acq = r.acq; a.erf_mode = r.erf_mode;
    a.n_excl = 0; a.excl_radius = r.excl_radius;
    if (r.n_excl > 0) {
        if (!r.excl_host) return fail(IBO_ERR_ARG, "excl_host is NULL");
        IBO_TRY(g->excl.ensure((size_t)r.n_excl * g->D));
        HIP_TRY(hipMemcpyAsync(g->excl.p, r.excl_host, sizeof(double) * r.n_excl * g->D, hipMemcpyHostToDevice, s));
        HIP_TRY(hipStreamSynchronize(s));
        a.n_excl = r.n_excl; a.excl = g->excl.p;
    }
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
    double hv; int64_t hi;
    HIP_TRY(hipMemcpyAsync(&hv, g->res_v.p, sizeof(double), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(&hi, g->res_i.p, sizeof(int64_t), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    HIP_TRY(hipEventElapsedTime(&g->sweep_ms, g->ev0, g->ev1));
    gpu_time_add(g->device, g->sweep_ms);
    if (r.best_val) *r.best_val = hv;
    if (r.best_idx) *r.best_idx = hi;
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

extern "C" int ibo_acq_sweep(ibo_gp_t *g, int64_t M, const double *cand_dev, int acq, double parm, int erf_mode,
                             double clamp_lo, double ymax, int n_excl, const double *excl_host,
                             double excl_radius, int64_t index_base, double *mu_dev, double *s2_dev,
                             double *acq_dev, double *best_val, int64_t *best_idx)
{
    if (!g) return fail(IBO_ERR_ARG, "gp is NULL");
    IBO_TRY(use_device(g->device));
    SweepRequest r = abi_request(M, cand_dev, acq, parm, erf_mode, clamp_lo, ymax, n_excl, excl_host, excl_radius, index_base);
    r.mu_dev = mu_dev; r.s2_dev = s2_dev; r.acq_dev = acq_dev; r.best_val = best_val; r.best_idx = best_idx;
    return run_sweep(g, r);
}

extern "C" int ibo_acq_sweep_incremental(ibo_gp_t *g, int64_t M, const double *cand_dev, int acq, double parm, int erf_mode,
                                         double clamp_lo, double ymax, int n_excl, const double *excl_host,
                                         double excl_radius, int64_t index_base, double *mu_dev, double *s2_dev,
                                         double *acq_dev, double *best_val, int64_t *best_idx)
{
    if (!g) return fail(IBO_ERR_ARG, "gp is NULL");
    IBO_TRY(use_device(g->device));
    SweepRequest r = abi_request(M, cand_dev, acq, parm, erf_mode, clamp_lo, ymax, n_excl, excl_host, excl_radius, index_base);
    r.mu_dev = mu_dev; r.s2_dev = s2_dev; r.acq_dev = acq_dev; r.best_val = best_val; r.best_idx = best_idx;
    r.incremental = true;
    return run_sweep(g, r);
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

// Host batches hand their results over as one block: (mu, s2, acq) restricted to the wanted ones, contiguous in that order, m values each.
struct Packed3 { double *p[3]; int n; };         // p[k]: where output k of such a block lies (NULL: not wanted); n: how many are
static Packed3 pack3(double *base, size_t m, const double *mu, const double *s2, const double *acq)
{
    Packed3 w = {{nullptr, nullptr, nullptr}, 0};
    const double *want[3] = {mu, s2, acq};
    for (int k = 0; k < 3; k++)
        if (want[k]) w.p[k] = base + m * w.n++;
    return w;
}
// a block in host memory -> the caller's arrays
static void unpack3(const double *base, size_t m, double *mu, double *s2, double *acq)
{
    const Packed3 w = pack3(const_cast<double *>(base), m, mu, s2, acq);
    double *dst[3] = {mu, s2, acq};
    for (int k = 0; k < 3; k++)
        if (dst[k]) memcpy(dst[k], w.p[k], sizeof(double) * m);
}
// the request of a host batch: per-candidate outputs into such a block at `base`, no arg-max
static SweepRequest batch_request(int64_t m, const double *cand_dev, int acq, double parm, int erf_mode, double clamp_lo, double ymax, const Packed3 &out)
{
    SweepRequest r;
    r.M = m; r.cand_dev = cand_dev; r.acq = acq; r.parm = parm; r.erf_mode = erf_mode; r.clamp_lo = clamp_lo; r.ymax = ymax;
    r.mu_dev = out.p[0]; r.s2_dev = out.p[1]; r.acq_dev = out.p[2];
    return r;
}

// Large host-in / host-out batches (GP.posteriors(X) on 10^5..10^7 NumPy rows): chunks of 2^17 points go through
// two sets of pinned + device buffers; the upload of chunk c+1 and the download of chunk c-1 run on their own
// streams while chunk c is in the sweep kernel, so the call costs about the kernel time, not kernel + PCIe +
// pageable staging.
static int eval_host_points_pipelined(ibo_gp *g, int64_t M, const double *Q_host, int acq, double parm, int erf_mode,
                                      double clamp_lo, double *mu_host, double *s2_host, double *acq_host, double ymax)
{
    const int64_t CH = (int64_t)1 << 17;
    const int D = g->D;
    if (!g->h2d_stream) {                             // copy streams and their events: created on first use
        HIP_TRY(hipStreamCreateWithFlags(&g->h2d_stream, hipStreamNonBlocking));
        HIP_TRY(hipStreamCreateWithFlags(&g->d2h_stream, hipStreamNonBlocking));
        for (int b = 0; b < 2; b++) {
            HIP_TRY(hipEventCreateWithFlags(&g->pe_in[b], hipEventDisableTiming));
            HIP_TRY(hipEventCreateWithFlags(&g->pe_k[b], hipEventDisableTiming));
            HIP_TRY(hipEventCreateWithFlags(&g->pe_out[b], hipEventDisableTiming));
        }
    }
    IBO_TRY(g->cand.ensure((size_t)(2 * CH) * D));
    IBO_TRY(g->outs.ensure((size_t)(2 * CH) * 3));
    IBO_TRY(ensure_pinned(g, (size_t)(2 * CH) * (D + 3)));
    double *pin_in[2] = {g->pin, g->pin + CH * D};
    double *pin_out[2] = {g->pin + 2 * CH * D, g->pin + 2 * CH * D + 3 * CH};
    double *dev_in[2] = {g->cand.p, g->cand.p + CH * D};
    double *dev_out[2] = {g->outs.p, g->outs.p + 3 * CH};
    const int64_t nch = (M + CH - 1) / CH;
    auto drain = [&](int64_t c) -> int {              // results of chunk c: pinned -> caller's arrays
        const int b = (int)(c & 1);
        const int64_t m = (c + 1 < nch) ? CH : M - c * CH;
        HIP_TRY(hipEventSynchronize(g->pe_out[b]));
        unpack3(pin_out[b], (size_t)m, mu_host ? mu_host + c * CH : nullptr, s2_host ? s2_host + c * CH : nullptr, acq_host ? acq_host + c * CH : nullptr);
        return IBO_OK;
    };
    for (int64_t c = 0; c < nch; c++) {
        const int b = (int)(c & 1);
        const int64_t m = (c + 1 < nch) ? CH : M - c * CH;
        if (c >= 2) IBO_TRY(drain(c - 2));           // frees buffer set b (its download has finished)
        memcpy(pin_in[b], Q_host + c * CH * D, sizeof(double) * m * D);
        HIP_TRY(hipMemcpyAsync(dev_in[b], pin_in[b], sizeof(double) * m * D, hipMemcpyHostToDevice, g->h2d_stream));
        HIP_TRY(hipEventRecord(g->pe_in[b], g->h2d_stream));
        HIP_TRY(hipStreamWaitEvent(g->stream, g->pe_in[b], 0));
        const Packed3 out = pack3(dev_out[b], (size_t)m, mu_host, s2_host, acq_host);
        IBO_TRY(run_sweep(g, batch_request(m, dev_in[b], acq, parm, erf_mode, clamp_lo, ymax, out)));
        HIP_TRY(hipEventRecord(g->pe_k[b], g->stream));
        HIP_TRY(hipStreamWaitEvent(g->d2h_stream, g->pe_k[b], 0));
        HIP_TRY(hipMemcpyAsync(pin_out[b], dev_out[b], sizeof(double) * m * out.n, hipMemcpyDeviceToHost, g->d2h_stream));
        HIP_TRY(hipEventRecord(g->pe_out[b], g->d2h_stream));
    }
    if (nch >= 2) IBO_TRY(drain(nch - 2));
    IBO_TRY(drain(nch - 1));
    return IBO_OK;
}

static int eval_host_points(ibo_gp *g, int64_t M, const double *Q_host, int acq, double parm, int erf_mode,
                            double clamp_lo, double *mu_host, double *s2_host, double *acq_host, double ymax = NAN)
{
    if (M >= ((int64_t)1 << 18) && g_host_pipeline)
        return eval_host_points_pipelined(g, M, Q_host, acq, parm, erf_mode, clamp_lo, mu_host, s2_host, acq_host, ymax);
    IBO_TRY(g->cand.ensure((size_t)M * g->D));
    IBO_TRY(g->outs.ensure(3 * (size_t)M));
    // pinned staging (input points + up to 3 output arrays): pageable copies cost ~15 us each and
    // DIRECT issues ~100 small batches per maximisation
    IBO_TRY(ensure_pinned(g, (size_t)M * (g->D + 3)));
    hipStream_t s = g->stream;
    double *pin_in = g->pin, *pin_out = g->pin + (size_t)M * g->D;
    memcpy(pin_in, Q_host, sizeof(double) * M * g->D);
    // Batches of at most 8192 points skip the copy launches altogether: pinned host memory is device-visible, the
    // kernels read the few KB of candidates from it and store the results into it (two ~10 us launches per batch).
    const bool zero_copy = M <= 8192;
    if (!zero_copy) HIP_TRY(hipMemcpyAsync(g->cand.p, pin_in, sizeof(double) * M * g->D, hipMemcpyHostToDevice, s));
    const Packed3 out = pack3(zero_copy ? pin_out : g->outs.p, (size_t)M, mu_host, s2_host, acq_host);
    SweepRequest r = batch_request(M, zero_copy ? pin_in : g->cand.p, acq, parm, erf_mode, clamp_lo, ymax, out);
    if (zero_copy) { r.cand_host = pin_in; r.signal = true; r.timed = false; }      // small batches: no kernel-time events either
    g->signal_pending = false;
    IBO_TRY(run_sweep(g, r));
    if (!zero_copy) HIP_TRY(hipMemcpyAsync(pin_out, g->outs.p, sizeof(double) * M * out.n, hipMemcpyDeviceToHost, s));
    if (zero_copy) {
        // a batch of this size is back in tens of microseconds: spin for a moment before handing the thread to the runtime's
        // blocking wait (whose wake-up alone costs about as much as the batch) -- on the word small2.hip's last kernel stores
        // behind its results (no event to record, signal and query), or on a completion event for the other kernels
        const bool flag = g->signal_pending;
        if (!flag) HIP_TRY(hipEventRecord(g->fit1, s));
        struct timespec w0, w1;
        clock_gettime(CLOCK_MONOTONIC, &w0);
        for (int spin = 0;; spin++) {
            if (flag) {
                if (*(volatile unsigned long long *)g->done_flag == g->done_seq) break;
                if (spin & 63) continue;
            } else {
                hipError_t q = hipEventQuery(g->fit1);
                if (q == hipSuccess) break;
                if (q != hipErrorNotReady) HIP_TRY(q);
            }
            clock_gettime(CLOCK_MONOTONIC, &w1);
            if ((w1.tv_sec - w0.tv_sec) * 1e6 + (w1.tv_nsec - w0.tv_nsec) * 1e-3 > 300.0) { HIP_TRY(hipStreamSynchronize(s)); break; }
        }
    } else HIP_TRY(hipStreamSynchronize(s));
    unpack3(pin_out, (size_t)M, mu_host, s2_host, acq_host);
    return IBO_OK;
}

extern "C" int ibo_posterior_batch(ibo_gp_t *g, int64_t M, const double *Q_host, double clamp_lo,
                                   double *mu_host, double *s2_host)
{
    if (!g || !Q_host || !mu_host) return fail(IBO_ERR_ARG, "NULL argument");
    if (M < 1) return fail(IBO_ERR_ARG, "M=%lld", (long long)M);
    IBO_TRY(use_device(g->device));
    if (!g->fitted) return fail(IBO_ERR_STATE, "posterior before a successful fit");
    return eval_host_points(g, M, Q_host, IBO_ACQ_NONE, 0.0, IBO_ERF_LIBM, clamp_lo, mu_host, s2_host, nullptr);
}

// host points in, host arrays out (any of mu / s2 / acq may be NULL): what EI(GP).negf(x), PI, UCB and their vectorised
// forms ask for -- small batches cost no allocation and no copy launch (pinned staging read and written by the kernels)
extern "C" int ibo_acq_batch(ibo_gp_t *g, int64_t M, const double *Q_host, int acq, double parm, int erf_mode,
                             double clamp_lo, double ymax, double *mu_host, double *s2_host, double *acq_host)
{
    if (!g || !Q_host || (!mu_host && !s2_host && !acq_host)) return fail(IBO_ERR_ARG, "NULL argument");
    if (M < 1) return fail(IBO_ERR_ARG, "M=%lld", (long long)M);
    if (acq < 0 || acq > 3) return fail(IBO_ERR_ARG, "unknown acquisition %d", acq);
    IBO_TRY(use_device(g->device));
    if (!g->fitted) return fail(IBO_ERR_STATE, "evaluation before a successful fit");
    return eval_host_points(g, M, Q_host, acq, parm, erf_mode, clamp_lo, mu_host, s2_host, acq_host, ymax);
}

// ------------------------------------------------------------------------ gradients with respect to the query point (grad.hip)
// The values (mu, s2, acq) come from eval_host_points -- the very numbers ibo_acq_batch returns; the gradients from the chunks of
// grad.hip, which form their own mu and s2 for the clip rule and the chain rule.  Up to 64 points: the candidates are read from, and the
// gradients written to, the handle's pinned staging (no copy launches).
extern "C" int ibo_acq_grad_batch(ibo_gp_t *g, int64_t M, const double *Q_host, int acq, double parm, int erf_mode,
                                  double clamp_lo, double ymax, double *mu_host, double *s2_host, double *acq_host,
                                  double *dmu_host, double *ds2_host, double *dacq_host)
{
    if (!g || !Q_host) return fail(IBO_ERR_ARG, "NULL argument");
    if (!mu_host && !s2_host && !acq_host && !dmu_host && !ds2_host && !dacq_host) return fail(IBO_ERR_ARG, "every output is NULL");
    if (M < 1) return fail(IBO_ERR_ARG, "M=%lld", (long long)M);
    if (acq < 0 || acq > 3) return fail(IBO_ERR_ARG, "unknown acquisition %d", acq);
    if (erf_mode != IBO_ERF_LIBM && erf_mode != IBO_ERF_NR) return fail(IBO_ERR_ARG, "unknown erf mode %d", erf_mode);
    if (acq == IBO_ACQ_NONE && dacq_host) return fail(IBO_ERR_ARG, "dacq_host with IBO_ACQ_NONE");
    IBO_TRY(use_device(g->device));
    if (!g->fitted) return fail(IBO_ERR_STATE, "gradient before a successful fit");
    if (mu_host || s2_host || acq_host)
        IBO_TRY(eval_host_points(g, M, Q_host, acq, parm, erf_mode, clamp_lo, mu_host, s2_host, acq_host, ymax));
    if (!dmu_host && !ds2_host && !dacq_host) return IBO_OK;
    const int D = g->D;
    hipStream_t s = g->stream;
    const GradPlan pl = grad_plan(g->N, g->Npad, g->DP, M);
    IBO_TRY(g->grad_ws.ensure(pl.ws_doubles));
    GradArgs a;
    memset(&a, 0, sizeof(a));
    a.kp = g->kp; a.N = g->N; a.Npad = g->Npad; a.DP = g->DP;
    a.Xp = g->Xp.p; a.W = g->W.p; a.alphaY = g->alphaY.p; a.alpha1 = g->alpha1.p;
    a.prior = prior_of(g);
    a.noise = g->noise; a.clamp_lo = clamp_lo; a.ymax = (ymax == ymax) ? ymax : g->maxY; a.parm = parm;
    a.acq = acq; a.erf_mode = erf_mode;
    a.TM = pl.TM; a.KC = pl.KC; a.nsplit = pl.nsplit; a.nparts = pl.nparts;
    double *outs_host[3] = {dmu_host, ds2_host, dacq_host};
    const bool zero_copy = M <= 64;                 // (pl.mc >= 64: one chunk)
    if (zero_copy) {
        IBO_TRY(ensure_pinned(g, (size_t)M * D * 4));
        memcpy(g->pin, Q_host, sizeof(double) * M * D);
    } else {
        IBO_TRY(g->grad_cand.ensure((size_t)pl.mc * D));
        IBO_TRY(g->grad_out.ensure((size_t)pl.mc * D * 3));
    }
    for (int64_t c0 = 0; c0 < M; c0 += pl.mc) {
        const int m = (int)(M - c0 < pl.mc ? M - c0 : pl.mc);
        const size_t nk = (size_t)m * g->Npad, np = (size_t)pl.nsplit * nk;
        a.K = g->grad_ws.p; a.H = a.K + nk; a.Pt = a.H + nk; a.Pu = a.Pt + np; a.E = a.Pu + np;
        const double *cand;
        double *obase;
        if (zero_copy) {
            cand = g->pin; obase = g->pin + (size_t)M * D;
        } else {
            HIP_TRY(hipMemcpyAsync(g->grad_cand.p, Q_host + c0 * D, sizeof(double) * m * D, hipMemcpyHostToDevice, s));
            cand = g->grad_cand.p; obase = g->grad_out.p;
        }
        double *od[3];
        for (int k = 0; k < 3; k++) od[k] = outs_host[k] ? obase + (size_t)k * m * D : nullptr;
        KERNEL_TRY(launch_grad(a, cand, m, od[0], od[1], od[2], s));
        if (!zero_copy)
            for (int k = 0; k < 3; k++)
                if (outs_host[k]) HIP_TRY(hipMemcpyAsync(outs_host[k] + c0 * D, od[k], sizeof(double) * m * D, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        if (zero_copy)
            for (int k = 0; k < 3; k++)
                if (outs_host[k]) memcpy(outs_host[k], od[k], sizeof(double) * M * D);
    }
    return IBO_OK;
}

// ------------------------------------------------------------------------ joint posterior and draws from it (cov.hip)
// mu: the launch sequence of ibo_posterior_batch (the same numbers, bit for bit)
static int cov_mean(ibo_gp *g, int64_t M, const double *Q_host, double *mu_host)
{
    std::vector<double> s2((size_t)M);
    return eval_host_points(g, M, Q_host, IBO_ACQ_NONE, 0.0, IBO_ERF_LIBM, 1e-7, mu_host, s2.data(), nullptr);
}

// Sigma of the M points into S (device, ld lds), diagonal rule diag - |v_a|^2; pad: rows and columns [M, round_up(M, 64)) identity.
// Scratch: the points, V^T (Mp x Npad) and one chunk of K* (at most 256 MiB, at least 64 points); handed back on every exit path.
static int cov_sigma(ibo_gp *g, int64_t M, const double *Q_host, double diag, int pad, double *S, size_t lds)
{
    const int N = g->N, Np = g->Npad, D = g->D, Mp = round_up((int)M, IBO_COV_TILE);
    hipStream_t s = g->stream;
    int mc = (int)((((size_t)256 << 20) / ((size_t)Np * sizeof(double))) / IBO_COV_TILE * IBO_COV_TILE);
    mc = mc < IBO_COV_TILE ? IBO_COV_TILE : (mc > Mp ? Mp : mc);
    ScopedBuf<double> q, kt, vt;
    IBO_TRY(q.ensure((size_t)M * D)); IBO_TRY(kt.ensure((size_t)mc * Np)); IBO_TRY(vt.ensure((size_t)Mp * Np));
    HIP_TRY(hipMemcpyAsync(q.p, Q_host, sizeof(double) * (size_t)M * D, hipMemcpyHostToDevice, s));
    for (int c0 = 0; c0 < Mp; c0 += mc) {
        const int mp = Mp - c0 < mc ? Mp - c0 : mc;
        const int m = (int)(M - c0 < mp ? M - c0 : mp);           // >= 1: c0 <= Mp - 64 < M
        KERNEL_TRY(launch_cov_kstar(g->kp, g->Xp.p, N, Np, g->DP, q.p + (size_t)c0 * D, m, mp, kt.p, s));
        KERNEL_TRY(launch_cov_tri(kt.p, (size_t)Np, g->W.p, (size_t)Np, N, mp, Np, vt.p + (size_t)c0 * Np, (size_t)Np, s));
    }
    KERNEL_TRY(launch_cov_syrk(g->kp, q.p, vt.p, (size_t)Np, round_up(N, 32), (int)M, Mp, diag, pad, S, lds, s));
    HIP_TRY(hipStreamSynchronize(s));
    return IBO_OK;
}

extern "C" int ibo_posterior_cov(ibo_gp_t *g, int64_t M, const double *Q_host, int with_noise, double *mu_host, double *S_host)
{
    IBO_TRY(use_device(g ? g->device : 0));
    if (!g || !Q_host || !S_host) return fail(IBO_ERR_ARG, "NULL argument");
    if (M < 1 || M > IBO_COV_MAX_M) return fail(IBO_ERR_ARG, "M=%lld outside [1, %d]", (long long)M, IBO_COV_MAX_M);
    if (!g->fitted) return fail(IBO_ERR_STATE, "posterior covariance before a successful fit");
    if (mu_host) IBO_TRY(cov_mean(g, M, Q_host, mu_host));
    hipStream_t s = g->stream;
    ScopedBuf<double> S;
    IBO_TRY(S.ensure((size_t)M * M));
    HIP_TRY(hipEventRecord(g->ev0, s));
    IBO_TRY(cov_sigma(g, M, Q_host, with_noise ? 1.0 + g->noise : 1.0, 0, S.p, (size_t)M));
    HIP_TRY(hipMemcpyAsync(S_host, S.p, sizeof(double) * (size_t)M * M, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipEventRecord(g->ev1, s));
    HIP_TRY(hipEventSynchronize(g->ev1));
    float ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms, g->ev0, g->ev1));
    gpu_time_add(g->device, ms);
    return IBO_OK;
}

// Sigma + jitter I padded to Mp = round_up(M, 64) rows (identity pad), factored in place by ibo_spd_*'s route, then F = Z L^T on the
// MFMA pipe.  Sigma never leaves the device.
extern "C" int ibo_posterior_sample(ibo_gp_t *g, int64_t M, const double *Q_host, int with_noise, double jitter, int nsamp,
                                    const double *Z_host, double *F_host, double *mu_host, int *info)
{
    IBO_TRY(use_device(g ? g->device : 0));
    if (!g || !Q_host || !Z_host || !F_host) return fail(IBO_ERR_ARG, "NULL argument");
    if (M < 1 || M > IBO_SAMPLE_MAX_M) return fail(IBO_ERR_ARG, "M=%lld outside [1, %d]", (long long)M, IBO_SAMPLE_MAX_M);
    if (nsamp < 1 || nsamp > IBO_SAMPLE_MAX_DRAWS) return fail(IBO_ERR_ARG, "nsamp=%d outside [1, %d]", nsamp, IBO_SAMPLE_MAX_DRAWS);
    if (!(jitter >= 0.0 && jitter < HUGE_VAL)) return fail(IBO_ERR_ARG, "jitter=%g is not a finite value >= 0", jitter);
    if (!g->fitted) return fail(IBO_ERR_STATE, "posterior draws before a successful fit");
    if (info) *info = 0;
    if (mu_host) IBO_TRY(cov_mean(g, M, Q_host, mu_host));
    hipStream_t s = g->stream;
    const int Mp = round_up((int)M, IBO_COV_TILE), Sp = round_up(nsamp, IBO_COV_TILE);
    ScopedBuf<double> S, d64, Z, F;
    ScopedBuf<int> dinfo;
    IBO_TRY(S.ensure((size_t)Mp * Mp)); IBO_TRY(d64.ensure((size_t)(Mp / 64) * 4096)); IBO_TRY(dinfo.ensure(1));
    IBO_TRY(Z.ensure((size_t)Sp * Mp)); IBO_TRY(F.ensure((size_t)Sp * Mp));
    HIP_TRY(hipEventRecord(g->ev0, s));
    IBO_TRY(cov_sigma(g, M, Q_host, (with_noise ? 1.0 + g->noise : 1.0) + jitter, 1, S.p, (size_t)Mp));
    KERNEL_TRY(launch_cholesky(S.p, Mp, d64.p, dinfo.p, s));
    int h = 0;
    HIP_TRY(hipMemcpyAsync(&h, dinfo.p, sizeof(int), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (h != 0) {
        if (info) *info = h;
        return fail(IBO_ERR_NOT_PD, "posterior covariance + %g I is not positive definite (pivot %d)", jitter, h);
    }
    HIP_TRY(hipMemsetAsync(Z.p, 0, sizeof(double) * (size_t)Sp * Mp, s));
    HIP_TRY(hipMemcpy2DAsync(Z.p, sizeof(double) * Mp, Z_host, sizeof(double) * M, sizeof(double) * M, nsamp, hipMemcpyHostToDevice, s));
    KERNEL_TRY(launch_cov_tri(Z.p, (size_t)Mp, S.p, (size_t)Mp, (int)M, Sp, Mp, F.p, (size_t)Mp, s));
    HIP_TRY(hipMemcpy2DAsync(F_host, sizeof(double) * M, F.p, sizeof(double) * Mp, sizeof(double) * M, nsamp, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipEventRecord(g->ev1, s));
    HIP_TRY(hipEventSynchronize(g->ev1));
    float ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms, g->ev0, g->ev1));
    gpu_time_add(g->device, ms);
    return IBO_OK;
}

// ------------------------------------------------------------------------ DIRECT on the GPU objective
int direct_on_gp(ibo_gp *g, int D, const double *lb, const double *ub, int acq, double parm, int erf_mode,
                        double clamp_lo, int maxiter, int maxtime, int maxsample, int compat,
                        double *opt, double *optx, int64_t *nsamples)
{
    if (D != g->D) return fail(IBO_ERR_ARG, "bounds have %d dimensions, model has %d", D, g->D);
    const bool dbg = getenv("IBO_DEBUG") != nullptr;
    double t_eval = 0.0; int n_batches = 0; int64_t n_pts = 0;
    ibo::batch_eval_t ev = [&](const double *pts, int n, double *vals) -> int {
        struct timespec a0, a1;
        if (dbg) clock_gettime(CLOCK_MONOTONIC, &a0);
        const int rc = eval_host_points(g, n, pts, acq, parm, erf_mode, clamp_lo, nullptr, nullptr, vals);
        if (dbg) { clock_gettime(CLOCK_MONOTONIC, &a1); t_eval += (a1.tv_sec - a0.tv_sec) * 1e3 + (a1.tv_nsec - a0.tv_nsec) * 1e-6; n_batches++; n_pts += n; }
        if (rc) return rc;
        for (int i = 0; i < n; i++) vals[i] = -vals[i];     // DIRECT minimises the negated acquisition
        return 0;
    };
    ibo::DirectOptions o;
    o.maxiter = maxiter; o.maxtime = maxtime; o.maxsample = maxsample; o.compat = compat != 0;
    o.per_rectangle = false;
    struct timespec w0, w1;
    clock_gettime(CLOCK_MONOTONIC, &w0);
    ibo::DirectResult r = ibo::direct_minimize(ev, D, lb, ub, o);
    clock_gettime(CLOCK_MONOTONIC, &w1);
    if (dbg) fprintf(stderr, "[libibo_hip] DIRECT: %d iterations, %lld samples, %d batches (%lld points): %.2f ms total, %.2f ms in GPU evaluation\n",
                     r.iterations, (long long)r.nsamples, n_batches, (long long)n_pts,
                     (w1.tv_sec - w0.tv_sec) * 1e3 + (w1.tv_nsec - w0.tv_nsec) * 1e-6, t_eval);
    if (r.status) return r.status;
    if (opt) *opt = -r.fmin;
    if (optx) for (int i = 0; i < D; i++) optx[i] = r.xmin[i];
    if (nsamples) *nsamples = r.nsamples;
    return IBO_OK;
}

extern "C" int ibo_direct_max(ibo_gp_t *g, int D, const double *lb, const double *ub, int acq, double parm,
                              int erf_mode, double clamp_lo, int maxiter, int maxtime, int maxsample,
                              int compat, double *opt, double *optx, int64_t *nsamples)
{
    if (!g || !lb || !ub) return fail(IBO_ERR_ARG, "NULL argument");
    if (acq < 0 || acq > 2) return fail(IBO_ERR_ARG, "unknown acquisition %d", acq);
    IBO_TRY(use_device(g->device));
    if (!g->fitted) return fail(IBO_ERR_STATE, "direct before a successful fit");
    return direct_on_gp(g, D, lb, ub, acq, parm, erf_mode, clamp_lo, maxiter, maxtime, maxsample, compat,
                        opt, optx, nsamples);
}


// ------------------------------------------------------------------------ constrained acquisition: A(x) prod_j Phi(z_j) over several handles (cacq.hip)
static_assert(IBO_CACQ_MAX == IBO_CACQ_MAX_CON, "the kernel argument arrays hold every constraint the ABI admits");

// the leading arguments of the four ibo_cacq_* entries
struct CacqCall {
    ibo_gp *obj; int ncon; ibo_gp *const *con; const double *thresh; const int *sense;
    int acq; double parm; int erf_mode; double clamp_lo, ymax;
};

// What the four entries check alike, in ibo_abi.h's order: the device first (as ibo_posterior_cov), then the arguments, then the handles'
// state -- and their dimensionality last, which only a fitted handle has.  points: the entry's candidate / query array; any_out: whether
// it was given an output at all.  Fills the kernel's view of the request (ymax NaN: the objective's largest observation).
static int cacq_begin(const CacqCall &c, int64_t M, const void *points, bool any_out, CacqSpec *sp)
{
    IBO_TRY(use_device(c.obj ? c.obj->device : 0));
    if (!c.obj) return fail(IBO_ERR_ARG, "the objective handle is NULL");
    if (c.ncon < 0 || c.ncon > IBO_CACQ_MAX_CON) return fail(IBO_ERR_ARG, "ncon=%d outside [0, %d]", c.ncon, IBO_CACQ_MAX_CON);
    if (c.ncon > 0 && (!c.con || !c.thresh || !c.sense)) return fail(IBO_ERR_ARG, "NULL constraint argument");
    for (int j = 0; j < c.ncon; j++) {
        if (!c.con[j]) return fail(IBO_ERR_ARG, "constraint handle %d is NULL", j);
        if (c.sense[j] != 1 && c.sense[j] != -1) return fail(IBO_ERR_ARG, "sense[%d]=%d is neither +1 nor -1", j, c.sense[j]);
        if (!(fabs(c.thresh[j]) < HUGE_VAL)) return fail(IBO_ERR_ARG, "thresh[%d]=%g is not finite", j, c.thresh[j]);
        if (c.con[j]->device != c.obj->device)
            return fail(IBO_ERR_ARG, "constraint %d lives on device %d, the objective on device %d", j, c.con[j]->device, c.obj->device);
    }
    if (M < 1) return fail(IBO_ERR_ARG, "M=%lld", (long long)M);
    if (!points) return fail(IBO_ERR_ARG, "NULL argument");
    if (c.acq == IBO_ACQ_UCB) return fail(IBO_ERR_ARG, "IBO_ACQ_UCB has no constrained form: a signed value times a probability orders nothing");
    if (c.acq != IBO_ACQ_EI && c.acq != IBO_ACQ_PI && c.acq != IBO_ACQ_NONE) return fail(IBO_ERR_ARG, "unknown acquisition %d", c.acq);
    if (c.erf_mode != IBO_ERF_LIBM && c.erf_mode != IBO_ERF_NR) return fail(IBO_ERR_ARG, "unknown erf mode %d", c.erf_mode);
    if (!any_out) return fail(IBO_ERR_ARG, "every output is NULL");
    if (!c.obj->fitted) return fail(IBO_ERR_STATE, "constrained acquisition before the objective's fit");
    for (int j = 0; j < c.ncon; j++)
        if (!c.con[j]->fitted) return fail(IBO_ERR_STATE, "constrained acquisition before constraint %d's fit", j);
    for (int j = 0; j < c.ncon; j++)
        if (c.con[j]->D != c.obj->D)
            return fail(IBO_ERR_ARG, "constraint %d has %d dimensions, the objective %d", j, c.con[j]->D, c.obj->D);
    memset(sp, 0, sizeof(*sp));
    sp->ncon = c.ncon; sp->acq = c.acq; sp->erf_mode = c.erf_mode;
    sp->ymax = (c.ymax == c.ymax) ? c.ymax : c.obj->maxY; sp->parm = c.parm;
    for (int j = 0; j < c.ncon; j++) { sp->thresh[j] = c.thresh[j]; sp->sense[j] = c.sense[j]; }
    return IBO_OK;
}

// One plain sweep per model -- (mu, s2) into device scratch, no arg-max, no read-back -- one after the other (a handle may appear more
// than once), then cacq_finish_kernel on the objective's stream.  Scratch: 16 (ncon + 1) bytes per candidate from the pool, at most
// about 1 GiB (more candidates go in chunks), handed back before the call returns.
extern "C" int ibo_cacq_sweep(ibo_gp_t *obj, int ncon, ibo_gp_t *const *con, const double *thresh, const int *sense,
                              int64_t M, const double *cand_dev, int acq, double parm, int erf_mode, double clamp_lo, double ymax,
                              int n_excl, const double *excl_host, double excl_radius, int64_t index_base,
                              double *acq_dev, double *pof_dev, double *val_dev, double *best_val, int64_t *best_idx)
{
    const CacqCall c = {obj, ncon, con, thresh, sense, acq, parm, erf_mode, clamp_lo, ymax};
    CacqArgs a;
    memset(&a, 0, sizeof(a));
    IBO_TRY(cacq_begin(c, M, cand_dev, acq_dev || pof_dev || val_dev || best_val || best_idx, &a.spec));
    ibo_gp *g = obj;
    hipStream_t s = g->stream;
    const int D = g->D;
    a.D = D; a.index_base = index_base; a.excl_radius = excl_radius;
    if (n_excl > 0) {
        if (!excl_host) return fail(IBO_ERR_ARG, "excl_host is NULL");
        IBO_TRY(g->excl.ensure((size_t)n_excl * D));
        HIP_TRY(hipMemcpyAsync(g->excl.p, excl_host, sizeof(double) * n_excl * D, hipMemcpyHostToDevice, s));
        HIP_TRY(hipStreamSynchronize(s));
        a.n_excl = n_excl; a.excl = g->excl.p;
    }
    int64_t mc = (((int64_t)1 << 30) / (16 * (ncon + 1))) / 256 * 256;        // candidates per chunk: a multiple of the combine's workgroup
    if (M <= mc) mc = M;
    const int64_t nblk = (M + 255) / 256;
    ScopedBuf<double> ms, pv;
    ScopedBuf<int64_t> pi;
    IBO_TRY(ms.ensure(2 * (size_t)(ncon + 1) * mc)); IBO_TRY(pv.ensure((size_t)nblk)); IBO_TRY(pi.ensure((size_t)nblk));
    a.ms = ms.p; a.stride = mc;
    for (int64_t c0 = 0; c0 < M; c0 += mc) {
        const int64_t m = M - c0 < mc ? M - c0 : mc;
        SweepRequest r;
        r.M = m; r.cand_dev = cand_dev + c0 * D; r.acq = IBO_ACQ_NONE; r.erf_mode = erf_mode; r.clamp_lo = clamp_lo;
        if (acq != IBO_ACQ_NONE) {                   // (the pure probability of feasibility does not look at the objective)
            r.mu_dev = ms.p; r.s2_dev = ms.p + mc;
            IBO_TRY(run_sweep(g, r));
        }
        for (int j = 0; j < ncon; j++) {
            r.mu_dev = ms.p + 2 * (size_t)(1 + j) * mc; r.s2_dev = r.mu_dev + mc;
            IBO_TRY(run_sweep(con[j], r));
            if (con[j]->stream != s) HIP_TRY(hipStreamSynchronize(con[j]->stream));     // the combine runs on the objective's stream
        }
        a.M = m; a.first = c0; a.cand = r.cand_dev;
        a.out_acq = acq_dev ? acq_dev + c0 : nullptr; a.out_pof = pof_dev ? pof_dev + c0 : nullptr; a.out_val = val_dev ? val_dev + c0 : nullptr;
        a.part_val = pv.p + c0 / 256; a.part_idx = pi.p + c0 / 256;
        KERNEL_TRY(launch_cacq_finish(a, s));
        if (c0 + mc < M) HIP_TRY(hipStreamSynchronize(s));      // the next chunk's sweeps, on other streams, write the same scratch
    }
    if (best_val || best_idx) {
        IBO_TRY(g->res_v.ensure(1)); IBO_TRY(g->res_i.ensure(1));
        SweepArgs f;
        memset(&f, 0, sizeof(f));
        f.part_val = pv.p; f.part_idx = pi.p; f.result_val = g->res_v.p; f.result_idx = g->res_i.p;
        KERNEL_TRY(launch_argmax_final(f, nblk, s));
        double hv; int64_t hi;
        HIP_TRY(hipMemcpyAsync(&hv, g->res_v.p, sizeof(double), hipMemcpyDeviceToHost, s));
        HIP_TRY(hipMemcpyAsync(&hi, g->res_i.p, sizeof(int64_t), hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        if (best_val) *best_val = hv;
        if (best_idx) *best_idx = hi;
    } else HIP_TRY(hipStreamSynchronize(s));
    return IBO_OK;
}

// Host batches (and with them every DIRECT batch): the ncon + 1 eval_host_points calls one after the other -- the objective's acquisition
// as ibo_acq_batch returns it, (mu, s2) of each constraint -- then the combine on the HOST (cacq.h's twin of gauss_cdf_pdf_dev): the
// per-model results are in host memory already, and one erf per constraint and point (about 20 ns) is less than another launch and wait.
// A, P, val: M each, any may be NULL.  keep (the gradient's): Phi, phi, z and sigma of every constraint, constraint-major.
struct CacqHostTerms { std::vector<double> cdf, pdf, z, sig; };
static int cacq_eval_host(const CacqCall &c, const CacqSpec &sp, int64_t M, const double *Q_host, double *A, double *P, double *val,
                          CacqHostTerms *keep)
{
    const size_t m = (size_t)M;
    std::vector<double> a(m, 1.0), p(m, 1.0), mu(c.ncon ? m : 0), s2(c.ncon ? m : 0);
    if (c.acq != IBO_ACQ_NONE)
        IBO_TRY(eval_host_points(c.obj, M, Q_host, c.acq, c.parm, c.erf_mode, c.clamp_lo, nullptr, nullptr, a.data(), sp.ymax));
    std::vector<double> v(a);
    if (keep) { keep->cdf.resize(m * c.ncon); keep->pdf.resize(m * c.ncon); keep->z.resize(m * c.ncon); keep->sig.resize(m * c.ncon); }
    for (int j = 0; j < c.ncon; j++) {
        IBO_TRY(eval_host_points(c.con[j], M, Q_host, IBO_ACQ_NONE, 0.0, c.erf_mode, c.clamp_lo, mu.data(), s2.data(), nullptr));
        for (size_t i = 0; i < m; i++) {
            const double sig = sqrt(s2[i]);
            const double z = (double)sp.sense[j] * (sp.thresh[j] - mu[i]) / sig;
            double cdf, pdf;
            gauss_cdf_pdf_host(c.erf_mode, z, &cdf, &pdf);
            p[i] *= cdf; v[i] *= cdf;
            if (keep) { keep->cdf[j * m + i] = cdf; keep->pdf[j * m + i] = pdf; keep->z[j * m + i] = z; keep->sig[j * m + i] = sig; }
        }
    }
    if (A) memcpy(A, a.data(), sizeof(double) * m);
    if (P) memcpy(P, p.data(), sizeof(double) * m);
    if (val) memcpy(val, v.data(), sizeof(double) * m);
    return IBO_OK;
}

extern "C" int ibo_cacq_batch(ibo_gp_t *obj, int ncon, ibo_gp_t *const *con, const double *thresh, const int *sense,
                              int64_t M, const double *Q_host, int acq, double parm, int erf_mode, double clamp_lo, double ymax,
                              double *acq_host, double *pof_host, double *val_host)
{
    const CacqCall c = {obj, ncon, con, thresh, sense, acq, parm, erf_mode, clamp_lo, ymax};
    CacqSpec sp;
    IBO_TRY(cacq_begin(c, M, Q_host, acq_host || pof_host || val_host, &sp));
    return cacq_eval_host(c, sp, M, Q_host, acq_host, pof_host, val_host, nullptr);
}

// grad val = grad A . P + A . grad P, composed on the host from ibo_acq_grad_batch per handle (dacq of the objective, dmu / ds2 of each
// constraint) in a fixed order; no division by Phi, so it stays finite where a factor underflows.
extern "C" int ibo_cacq_grad_batch(ibo_gp_t *obj, int ncon, ibo_gp_t *const *con, const double *thresh, const int *sense,
                                   int64_t M, const double *Q_host, int acq, double parm, int erf_mode, double clamp_lo, double ymax,
                                   double *val_host, double *dval_host)
{
    const CacqCall c = {obj, ncon, con, thresh, sense, acq, parm, erf_mode, clamp_lo, ymax};
    CacqSpec sp;
    IBO_TRY(cacq_begin(c, M, Q_host, val_host || dval_host, &sp));
    const size_t m = (size_t)M, D = (size_t)obj->D;
    CacqHostTerms t;
    std::vector<double> A(m), P(m);
    IBO_TRY(cacq_eval_host(c, sp, M, Q_host, A.data(), P.data(), val_host, dval_host ? &t : nullptr));
    if (!dval_host) return IBO_OK;
    std::vector<double> g1(m * D), g2(ncon ? m * D : 0), dP(m * D, 0.0);
    if (acq != IBO_ACQ_NONE)
        IBO_TRY(ibo_acq_grad_batch(obj, M, Q_host, acq, parm, erf_mode, clamp_lo, sp.ymax, nullptr, nullptr, nullptr, nullptr, nullptr, g1.data()));
    for (size_t i = 0; i < m; i++)
        for (size_t d = 0; d < D; d++) dval_host[i * D + d] = (acq != IBO_ACQ_NONE) ? g1[i * D + d] * P[i] : 0.0;
    for (int j = 0; j < ncon; j++) {
        IBO_TRY(ibo_acq_grad_batch(con[j], M, Q_host, IBO_ACQ_NONE, 0.0, erf_mode, clamp_lo, NAN, nullptr, nullptr, nullptr, g1.data(), g2.data(),
                                   nullptr));
        for (size_t i = 0; i < m; i++) {
            double w = t.pdf[j * m + i];                         // phi(z_j) prod_{k != j} Phi(z_k), k ascending
            for (int k = 0; k < ncon; k++)
                if (k != j) w *= t.cdf[k * m + i];
            const double sig = t.sig[j * m + i], z = t.z[j * m + i];
            for (size_t d = 0; d < D; d++) {
                const double dsig = g2[i * D + d] / (2.0 * sig);          // (ds2 is 0 where the clip is active)
                const double dz = -((double)sp.sense[j] * g1[i * D + d] + z * dsig) / sig;
                dP[i * D + d] += w * dz;
            }
        }
    }
    for (size_t i = 0; i < m; i++)
        for (size_t d = 0; d < D; d++) dval_host[i * D + d] += A[i] * dP[i * D + d];
    return IBO_OK;
}

// direct_on_gp's shape over all the handles: the same options, the same batched schedule, every batch through cacq_eval_host
extern "C" int ibo_cacq_direct_max(ibo_gp_t *obj, int ncon, ibo_gp_t *const *con, const double *thresh, const int *sense,
                                   int D, const double *lb, const double *ub, int acq, double parm, int erf_mode, double clamp_lo, double ymax,
                                   int maxiter, int maxtime, int maxsample, int compat, double *opt, double *optx, int64_t *nsamples)
{
    const CacqCall c = {obj, ncon, con, thresh, sense, acq, parm, erf_mode, clamp_lo, ymax};
    CacqSpec sp;
    IBO_TRY(cacq_begin(c, 1, (lb && ub) ? lb : nullptr, opt || optx || nsamples, &sp));
    if (D != obj->D) return fail(IBO_ERR_ARG, "bounds have %d dimensions, the models have %d", D, obj->D);
    const bool dbg = getenv("IBO_DEBUG") != nullptr;
    double t_eval = 0.0; int n_batches = 0; int64_t n_pts = 0;
    ibo::batch_eval_t ev = [&](const double *pts, int n, double *vals) -> int {
        struct timespec a0, a1;
        if (dbg) clock_gettime(CLOCK_MONOTONIC, &a0);
        const int rc = cacq_eval_host(c, sp, n, pts, nullptr, nullptr, vals, nullptr);
        if (dbg) { clock_gettime(CLOCK_MONOTONIC, &a1); t_eval += (a1.tv_sec - a0.tv_sec) * 1e3 + (a1.tv_nsec - a0.tv_nsec) * 1e-6; n_batches++; n_pts += n; }
        if (rc) return rc;
        for (int i = 0; i < n; i++) vals[i] = -vals[i];     // DIRECT minimises the negated value
        return 0;
    };
    ibo::DirectOptions o;
    o.maxiter = maxiter; o.maxtime = maxtime; o.maxsample = maxsample; o.compat = compat != 0;
    o.per_rectangle = false;
    struct timespec w0, w1;
    clock_gettime(CLOCK_MONOTONIC, &w0);
    ibo::DirectResult r = ibo::direct_minimize(ev, D, lb, ub, o);
    clock_gettime(CLOCK_MONOTONIC, &w1);
    if (dbg) fprintf(stderr, "[libibo_hip] constrained DIRECT (%d constraints): %d iterations, %lld samples, %d batches (%lld points): %.2f ms total, %.2f ms in evaluation\n",
                     ncon, r.iterations, (long long)r.nsamples, n_batches, (long long)n_pts,
                     (w1.tv_sec - w0.tv_sec) * 1e3 + (w1.tv_nsec - w0.tv_nsec) * 1e-6, t_eval);
    if (r.status) return r.status;
    if (opt) *opt = -r.fmin;
    if (optx) for (int i = 0; i < D; i++) optx[i] = r.xmin[i];
    if (nsamples) *nsamples = r.nsamples;
    return IBO_OK;
}

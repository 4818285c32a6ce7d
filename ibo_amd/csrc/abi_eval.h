// abi_eval.h -- what the evaluation units (abi_sweep.hip, abi_batch.hip, abi_cacq.hip, abi_ehvi.hip, abi_mes.hip, abi_kg.hip, abi_paths.hip, abi_qei.hip, abi_gradobs.hip, abi_sparse.hip, abi_rows.hip, abi_moments.hip) share beyond
// abi_internal.h: the sweep request, the host batch, and the ONE copy of the arg-max read-back, the exclusion upload, the padding of a short sweep to its size class, the timed span, the two clocks
// (abi_nlml.hip times with them too) and the read-back of their sums, the wrapped models' argument check, the V^T rows and the DIRECT driver.
#pragma once
#include "abi_internal.h"

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

// ---- abi_sweep.hip
int run_sweep(ibo_gp *g, const SweepRequest &r);
// the exclusion balls' centres (n_excl x D, host) into the handle's buffer; *n and *ptr are left alone when there are none
int upload_exclusions(ibo_gp *g, int n_excl, const double *excl_host, int *n, const double **ptr);
// (res_v, res_i) -> the host, after which the stream is idle; either pointer may be NULL
int read_result(ibo_gp *g, double *best_val, int64_t *best_idx);
// the winner among nblk per-workgroup partials (launch_argmax_final into res_v / res_i), then read_result
int argmax_readback(ibo_gp *g, const double *part_val, const int64_t *part_idx, int64_t nblk, double *best_val, int64_t *best_idx);
// closes the span an entry opened by recording ev0: records ev1, waits for it and adds ev0 -> ev1 to the device's GPU time
int finish_span(ibo_gp *g);

// run_sweep picks its kernels by the size of the launch, and two of its routes agree to rounding only.  So that a candidate's (mu, s2) -- and
// with them its value -- do not depend on how many candidates travel with it, a short launch is padded (with candidates at the origin, whose
// results nobody reads) to the size class of the call's chunk `mc`:
//   mc <= 4096  small2.hip's kernels.  Up to 128 candidates of a small model they are fused into one (launch_sweep_small: `local`, another
//               order of the sums): such a launch runs as 160 candidates, beyond the fused form's reach for every model;
//   mc >  4096  sweep2_kernel (choose_route): a tail of up to 4096 candidates runs as 4097.
// (Where the dot form is not admissible run_sweep has other routes and other thresholds; there the entries agree to rounding.)
#define CLASS_PAD_SMALL_FROM 128
#define CLASS_PAD_SMALL_TO 160
#define CLASS_PAD_LARGE_FROM 4096
static inline int64_t class_padded(int64_t m, int64_t mc)
{
    if (mc <= CLASS_PAD_LARGE_FROM) return m <= CLASS_PAD_SMALL_FROM ? CLASS_PAD_SMALL_TO : m;
    return m <= CLASS_PAD_LARGE_FROM ? CLASS_PAD_LARGE_FROM + 1 : m;
}

// The diagnostic's clock of an entry call whose unit has a timing option: two events around a span of one stream's work, the span's time
// added to one of the unit's thread-local sums (stop waits for the span's end).  Made per call; everything is a no-op unless switched on.
struct SpanClock {
    bool on = false;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    ~SpanClock() { if (e0) (void)hipEventDestroy(e0); if (e1) (void)hipEventDestroy(e1); }
    int make(bool timing) { on = timing; if (on) { HIP_TRY(hipEventCreate(&e0)); HIP_TRY(hipEventCreate(&e1)); } return IBO_OK; }
    int start(hipStream_t s) { if (on) HIP_TRY(hipEventRecord(e0, s)); return IBO_OK; }
    int stop(hipStream_t s, double *sum)
    {
        if (!on) return IBO_OK;
        float ms = 0.f;
        HIP_TRY(hipEventRecord(e1, s)); HIP_TRY(hipEventSynchronize(e1)); HIP_TRY(hipEventElapsedTime(&ms, e0, e1));
        *sum += ms;
        return IBO_OK;
    }
};
// The other clock: marks on the stream around the stages of one call as they are queued, accounted after the call's own synchronisation (no wait of its own)
struct StageClock {
    hipStream_t s = nullptr;
    double *ms = nullptr;                            // the unit's thread-local sums
    hipEvent_t ev[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    bool on = false;
    ~StageClock() { for (hipEvent_t e : ev) if (e) (void)hipEventDestroy(e); }
    int make(hipStream_t stream, double *sums, bool timing)
    {
        s = stream; ms = sums; on = timing;
        for (hipEvent_t &e : ev) if (on) HIP_TRY(hipEventCreate(&e));
        return IBO_OK;
    }
    int mark(int k) { if (on) HIP_TRY(hipEventRecord(ev[k], s)); return IBO_OK; }
    int account(int k0, int k1, int stage)           // after a synchronisation: the time between marks k0 and k1 goes to stage `stage`
    {
        float t = 0.f;
        if (on) { HIP_TRY(hipEventElapsedTime(&t, ev[k0], ev[k1])); ms[stage] += t; }
        return IBO_OK;
    }
};
// what every ibo_*_stage_ms / ibo_*_scan_ms entry does with its unit's n thread-local sums
static inline int read_stage_sums(double *sums, size_t n, double *ms, int reset)
{
    if (ms) memcpy(ms, sums, sizeof(double) * n);
    if (reset) memset(sums, 0, sizeof(double) * n);
    return IBO_OK;
}
// What the evaluating entries of the models that wrap frames (ibo_ggp, ibo_sgp) check alike: the device first, the arguments, the state
template <typename Handle>
int wrapped_check(Handle *h, const char *noun, bool ptrs_ok, int64_t M, int acq, int erf_mode, bool none_ok)
{
    IBO_TRY(use_device(h ? h->device : 0));
    if (!h || !ptrs_ok) return fail(IBO_ERR_ARG, "NULL argument");
    if (M < 1) return fail(IBO_ERR_ARG, "M=%lld", (long long)M);
    if (acq < 0 || acq > (none_ok ? IBO_ACQ_NONE : IBO_ACQ_UCB)) return fail(IBO_ERR_ARG, "unknown acquisition %d", acq);
    if (erf_mode != IBO_ERF_LIBM && erf_mode != IBO_ERF_NR) return fail(IBO_ERR_ARG, "unknown erf flavour %d", erf_mode);
    if (!h->fitted) return fail(IBO_ERR_STATE, "%s model before a successful fit", noun);
    return IBO_OK;
}

// ---- abi_batch.hip
// host points in, host arrays out (any of mu / s2 / acq may be NULL): one sweep, or the pipelined chunks of a large batch
int eval_host_points(ibo_gp *g, int64_t M, const double *Q_host, int acq, double parm, int erf_mode,
                     double clamp_lo, double *mu_host, double *s2_host, double *acq_host, double ymax = NAN);
// V^T = (W K*)^T of m points (device, m x D; mp = m rounded up to the covariance tile): K* into kt, the rows into vt, both mp x Npad
int vt_rows(ibo_gp *g, const double *pts_dev, int m, int mp, double *kt, double *vt, hipStream_t s);
// The DIRECT driver of every GPU objective.  value: the objective's values at a batch of points, to be MAXIMISED (negated here for the
// minimiser).  label: what IBO_DEBUG's line calls the search.  Returns the search's status, or fills the maximum, its place and the
// number of samples (each optional).
int direct_maximize(const ibo::batch_eval_t &value, const char *label, int D, const double *lb, const double *ub,
                    int maxiter, int maxtime, int maxsample, int compat, double *opt, double *optx, int64_t *nsamples);

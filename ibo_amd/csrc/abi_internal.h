// abi_internal.h -- what the translation units behind the C ABI (include/ibo_abi.h) share: the error channel, the option switches, the
// per-device memory pool and its buffer type, the handle (struct ibo_gp) and the helpers one unit lends another.
//   abi_core.hip    library / options / device memory / pools / handle life cycle
//   abi_fit.hip     fit (its pieces -- buffers, frame, tail -- serve abi_gradobs.hip's fit too), block extension, removal of rows, set_y, prior, accessors, ibo_cov_matrix
//   abi_pref.hip    the preference GP's device steps (ibo_pref_*)
//   abi_factor.hip  factor-and-invert for all of these and the gradients: route choice, the fit's frame, the routine, the info word; ibo_spd_* (abi_factor.h)
//   abi_sweep.hip   candidate sweeps: the routes, run_sweep, the sweep entries
//   abi_batch.hip   host batches, query-point gradients, joint posterior and draws, DIRECT on a GPU objective
//   abi_cacq.hip    the constrained acquisition (ibo_cacq_*)
//   abi_ehvi.hip    the two-objective expected hypervolume improvement (ibo_ehvi_*)
//   abi_mes.hip     max-value entropy search and the max-value cdf (ibo_mes_*)
//   abi_marg.hip    acquisitions integrated over an ensemble of models (ibo_iacq_*, include/ibo_abi_ensemble.h)
//   abi_kg.hip      the knowledge gradient (ibo_kg_*)
//   abi_paths.hip   pathwise posterior draws (ibo_paths_*)
//   abi_qei.hip     the Monte-Carlo parallel expected improvement (ibo_qei_*)
//   abi_gradobs.hip the GP observed with gradients (ibo_ggp_*): its own handle around a P-row frame, the row pipeline with its own K*
//   abi_sparse.hip  the sparse GP on inducing points (ibo_sgp_*): its own handle around two m-row frames and the kept Gram matrix
//   abi_rows.hip    the row pipeline of abi_kg, abi_qei and abi_gradobs: chunk, scratch, stage clock, host batch, device sweep (abi_rows.h)
//   abi_moments.hip the moments pipeline of abi_cacq, abi_ehvi, abi_mes, abi_marg and abi_sparse: the plain sweeps of a chunk into scratch, the
//                   stream rule, the padded tail, host batch, device sweep (abi_moments.h)
//                   (these thirteen are the evaluation units: what they share among themselves is in abi_eval.h)
//   abi_nlml.hip    marginal-likelihood grid and the three gradients (one prepare step, one rule for resident data), ibo_trim
//   abi_legacy.hip  libego's symbols (acqmaxGP, direct, logCDFs) and ibo_direct_host
// A struct that owns DevBufs has a release() directly under its member list, which ibo_trim and the destroy entries call.
// There is no CPU fallback anywhere behind this header: without a gfx950 device every compute entry point returns IBO_ERR_NO_DEVICE.
#pragma once
#include "../../include/ibo_abi.h"
#include "ibo_common.h"
#include "direct_host.h"
#include "legacy.h"

#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <ctime>
#include <string>
#include <atomic>
#include <mutex>
#include <vector>

// the thread's last error message (ibo_last_error); returns `code`
int ibo_fail(int code, const char *fmt, ...);
#define fail ibo_fail

#define HIP_TRY(expr)                                                                         \
    do {                                                                                      \
        hipError_t e_ = (expr);                                                               \
        if (e_ != hipSuccess)                                                                 \
            return fail(IBO_ERR_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
    } while (0)
#define KERNEL_TRY(expr)                                                                      \
    do {                                                                                      \
        int e_ = (expr);                                                                      \
        if (e_ != 0)                                                                          \
            return fail(IBO_ERR_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString((hipError_t)e_), __FILE__, __LINE__); \
    } while (0)
#define IBO_TRY(expr) do { int s_ = (expr); if (s_ != IBO_OK) return s_; } while (0)

// ---- option switches (abi_core.hip: ibo_set_option)
extern std::atomic<int> g_super_min_nb;        // ibo_set_option("super_min_nb", nb): block columns from which a fit runs in super-panels
extern std::atomic<int> g_host_pipeline, g_fused2_min_nb, g_gallery_prune, g_nlml_batch, g_chol_left, g_dot_override, g_legacy_exact, g_force_path, g_nlml_groups;
extern std::atomic<int> g_cacq_chunk;                // abi_cacq.hip: candidates per chunk of ibo_cacq_sweep (0: by bytes)
extern std::atomic<int> g_ehvi_chunk, g_ehvi_timing; // abi_ehvi.hip: candidates per chunk of the ibo_ehvi_* entries (0: by bytes); HIP events around the scan kernel
extern std::atomic<int> g_mes_chunk, g_mes_timing;   // abi_mes.hip: candidates per chunk of the ibo_mes_* entries (0: by bytes); HIP events around the scan kernels
extern std::atomic<int> g_iacq_chunk, g_iacq_timing; // abi_marg.hip: candidates per chunk of the ibo_iacq_* entries (0: by bytes); HIP events around a chunk's sweeps and its finish
extern std::atomic<int> g_kg_chunk, g_kg_timing;     // abi_kg.hip: candidates per chunk (0: by bytes); per-stage HIP events
extern std::atomic<int> g_qei_chunk, g_qei_timing;   // abi_qei.hip: candidates per chunk (0: by bytes); per-stage HIP events
extern std::atomic<int> g_ggp_chunk, g_ggp_timing;   // abi_gradobs.hip: candidates per chunk of the ibo_ggp_* entries (0: by bytes); per-stage HIP events
extern std::atomic<int> g_sgp_chunk, g_sgp_timing;   // abi_sparse.hip: observations / candidates per chunk of the ibo_sgp_* entries (0: by bytes); per-stage HIP events
extern std::atomic<int> g_paths_chunk;               // abi_paths.hip: candidates per launch of the ibo_paths_* entries (0: 2^21)
extern std::mutex g_dev_mu[16];             // serialises the per-device workspaces of ibo_nlml_grid / ibo_nlml_grad / ibo_trim
extern std::atomic<size_t> g_pool_limit;

int use_device(int device);
void gpu_time_add(int device, double ms);    // accumulates what ibo_gpu_time_ms reports

// ---- recycled device memory (abi_core.hip)
void *pool_get(size_t bytes, size_t *got);
void pool_put(void *p, size_t bytes);
void pool_trim(int dev);
void pool_warm(int dev);
extern thread_local bool g_pool_quiet;       // the caller has synchronised the device already (ibo_gp_destroy: once for all its buffers)
// ibo_set_option("alloc_fill", v), a test hook: -1 off; 0 .. 255: every block DevBuf::ensure or ibo_dev_alloc obtains is filled with that byte
// and the device synchronised before it is handed out, pinned staging is filled on the host.  A new buffer's content is undefined: no result
// may depend on it (tests/test_gpu_alloc_fill.py)
extern std::atomic<int> g_alloc_fill;
int alloc_fill_device(void *p, size_t bytes);      // (only while the hook is on) hipMemset + hipDeviceSynchronize
void alloc_fill_host(void *p, size_t bytes);       // memset while the hook is on, nothing otherwise

template <typename T>
struct DevBuf {
    T *p = nullptr;
    size_t cap = 0;
    size_t bytes = 0;              // what the pool handed out (a multiple of its grain, not of sizeof(T)): what goes back to it
    int ensure(size_t n)
    {
        if (n <= cap) return IBO_OK;
        release();
        size_t got = 0;
        void *q = pool_get(n * sizeof(T), &got);
        if (!q) {
            got = n * sizeof(T);
            hipError_t e = hipMalloc(&q, got);
            if (e != hipSuccess) {
                int dev = 0;
                (void)hipGetDevice(&dev);
                pool_trim(dev);                       // give the cached blocks back and try once more
                e = hipMalloc(&q, got);
            }
            if (e != hipSuccess) return fail(IBO_ERR_HIP, "hipMalloc(%zu bytes) failed: %s", got, hipGetErrorString(e));
        }
        p = (T *)q;
        cap = got / sizeof(T);
        bytes = got;
        if (g_alloc_fill.load(std::memory_order_relaxed) >= 0) return alloc_fill_device(q, got);
        return IBO_OK;
    }
    void release() { if (p) pool_put(p, bytes); p = nullptr; cap = 0; bytes = 0; }
};
// function-local buffers: handed back on every exit path (the members of handles and of the static
// workspaces are released explicitly -- a static object must not call into HIP at process exit)
template <typename T>
struct ScopedBuf : DevBuf<T> {
    ~ScopedBuf() { this->release(); }
};

struct ibo_gp {
    int device = 0;
    hipStream_t stream = nullptr;
    hipStream_t h2d_stream = nullptr, d2h_stream = nullptr;      // host-array batches: copies overlap the sweep
    hipEvent_t pe_in[2] = {nullptr, nullptr}, pe_k[2] = {nullptr, nullptr}, pe_out[2] = {nullptr, nullptr};
    hipEvent_t ev0 = nullptr, ev1 = nullptr, fit0 = nullptr, fit1 = nullptr;
    bool fitted = false;
    int N = 0, D = 0, Npad = 0, DP = 0;
    bool reversed = false;          // legacy invR path stores the observations in reverse order
    bool plain_fit = false;         // L = chol(R) of the model's own kernel matrix: ibo_gp_extend may append rows
    bool L_upper_dirty = false;     // zero_upper is deferred to ibo_gp_get_L
    bool R_valid = false;           // R = K(X, X) + diag is formed when someone asks for it (ibo_gp_get_R, ibo_pref_finish): ensure_R
    int dot_form = 1;               // SE k* via a_k + b_c + x~.c~; off when |x~|^2 is so large that the
                                    // cancellation would cost more than 1e-10 (pathological length scales)
    KParams kp;
    KParams kp_fit;                 // kp as fitted (kp.sf2 is overridden per sweep by ibo_gp_set_kstar_sf2)
    double noise = 0.0, maxY = 0.0;
    float fit_ms = 0.f, sweep_ms = 0.f;
    const char *sweep_kernel = "";
    std::vector<double> Yhost;
    double *pin = nullptr; size_t pin_cap = 0;      // pinned host staging for small host-in/host-out batches
    DevBuf<double> Xp, Xs, ak, XA, Y, R, A, L, W, T, Wp, diag64, alphaY, alpha1, tmp, cand, outs, excl, qpart, mupart, partv, res_v;
    DevBuf<int64_t> parti, res_i;
    // kept sweep state (ibo_acq_sweep_incremental): (q, aY.k*, a1.k*) per candidate of ONE device candidate array
    DevBuf<double> state;
    DevBuf<int> tile_done; DevBuf<double> tile_ub; DevBuf<unsigned long long> part_words; DevBuf<int> tile_rows, tile_sel;   // kept state with incomplete tiles (st_pruned)
    bool st_pruned = false; int st_N0 = 0; int st_nlev = 2;   // st_N0: the model's rows when the state was formed; st_nlev: its levels of W's rows
    DevBuf<double> small_ws;        // small2.hip: k* in fragment order + partial sums of a small batch
    DevBuf<double> grad_ws, grad_cand, grad_out;   // ibo_acq_grad_batch (grad.hip): one chunk's scratch, its candidates and its three M x D outputs
    uint64_t st_gen = 0; size_t st_off = 0; int64_t st_M = 0; int st_N = 0; double st_sf2 = 0.0; unsigned st_epoch = 0;   // st_gen: generation of the candidate array's allocation (0: no state)
    unsigned fit_epoch = 0;         // bumped by every full fit: a kept state never survives one
    int reserve = 0;                // rows of head-room the next fit leaves for ibo_gp_extend (ibo_gp_reserve)
    DevBuf<int> info;
    unsigned long long *done_flag = nullptr;   // pinned host word small2.hip's last kernel writes; done_seq: last value asked for
    unsigned long long done_seq = 0;
    bool signal_pending = false;
    const double *alpha_tail_Y = nullptr, *alpha_tail_1 = nullptr; int alpha_tail_Np = 0;   // where the alpha vectors' zero tails are
    DevBuf<unsigned> done_count;
    // fits from g_super_min_nb block columns on (launch_cholesky_super): [A ; E] in one tall buffer, the packed store of [L ; E^T-in-progress]
    DevBuf<double> tall, Pk2;
    // preference GP (ibo_pref_*): R^-1, the matrix being factored and its factors, vectors, sparse terms
    struct PrefWork {
        DevBuf<double> Rinv, A, Lh, E, Et, d64, vec, tmp, val;
        DevBuf<long long> lin;
        DevBuf<int> info;
        bool ready = false;
        unsigned epoch = 0; int N = 0, Npad = 0;     // the model ibo_pref_begin ran on (pref_owned): its fit_epoch, rows and padded rows
        void release() { for (DevBuf<double> *b : {&Rinv, &A, &Lh, &E, &Et, &d64, &vec, &tmp, &val}) b->release(); lin.release(); info.release(); }
    } pw;
    // prior
    int nb = 0; double ptheta = 0.0;
    DevBuf<double> pmeans, pbeta, plowerb, pwidth;
    // every DevBuf above, back to the pool (ibo_gp_destroy; streams, events and the pinned block are its own business).  Keep THIS order and
    // append: the order in which blocks return to the pool decides where the next handle's buffers lie
    void release()
    {
        for (DevBuf<double> *b : {&Xp, &Xs, &ak, &XA, &Y, &R, &A, &L, &W, &T, &Wp, &diag64, &alphaY, &alpha1, &tmp, &cand, &outs, &excl, &qpart, &mupart, &partv, &res_v}) b->release();
        parti.release(); res_i.release(); state.release(); small_ws.release(); grad_ws.release(); grad_cand.release(); grad_out.release();
        tile_done.release(); tile_ub.release(); part_words.release(); tile_rows.release(); tile_sel.release(); done_count.release(); tall.release(); Pk2.release();
        pw.release(); info.release(); pmeans.release(); pbeta.release(); plowerb.release(); pwidth.release();
    }
};

static inline int round_up(int x, int m) { return (x + m - 1) / m * m; }
// the handle's mean prior as the kernels take it (sweeps, gradients, leave-one-out)
static inline PriorDev prior_of(const ibo_gp *g)
{
    PriorDev p;
    p.nb = g->nb; p.theta = g->ptheta; p.means = g->pmeans.p; p.beta = g->pbeta.p; p.lowerb = g->plowerb.p; p.width = g->pwidth.p;
    return p;
}
// (which order factors a matrix, and the factor-and-invert routine itself: abi_factor.h)

// ---- helpers one unit lends another
int exp_table(int device, const double **out);                                                            // abi_sweep.hip: 2^(j/2048), one per device
int ibo_comm_exchange_dev(ibo_comm_t *c, hipStream_t s, const double *res_v, const int64_t *res_i, const double *cand_dev, int D, int64_t index_base,
                          double *local_val, int64_t *local_idx, double *best_val, int64_t *best_idx, double *best_x, int *best_rank);   // comm.hip
uint64_t alloc_generation(int device, const void *p, size_t bytes, size_t *offset);                       // abi_core.hip
int ensure_pinned(ibo_gp *g, size_t need);                                                                // abi_core.hip
int make_kparams(int ktype, int D, const double *hyper, int nhyper, double sf2, KParams *kp);             // abi_fit.hip
void sgp_grad_trim(int device);                                                                           // abi_sparse.hip: gives ibo_sgp_nlml_grad's private handle back (ibo_trim)
int ensure_R(ibo_gp *g);                                                                                  // abi_fit.hip: R = K(X, X) + diag, formed on request
int fit_begin(ibo_gp *g, int ktype, int N, int D, const double *X, const double *Y, const double *hyper, int nhyper, double sf2,
              double noise, bool reverse, KParams *kp);                                                   // abi_fit.hip: what every fit starts with (the staging)
int fit_factor(ibo_gp *g, const KParams &kp, int N, double noise, bool have_A, int *info);                // abi_fit.hip: a fit after staging (have_A: of g->A)
// abi_fit.hip, what fit_factor is made of, for the model that assembles its own matrix (abi_gradobs.hip): the factor-side buffers of an Np-row
// frame; the tail (between them fit_operands and fit_invert, abi_factor.h): both alpha vectors, queued; then the info word ("<noun> is not
// positive definite"; synchronises), the span fit0 -> fit1, fitted / plain_fit / fit_epoch
int fit_buffers(ibo_gp *g, int Np);
int fit_alpha(ibo_gp *g, int N);
int fit_end(ibo_gp *g, bool plain, const char *noun, int *info);
int fit_from_inverse(ibo_gp *g, int ktype, int N, int D, const double *X, const double *Y,
                     const double *hyper, int nhyper, double sf2, double noise, const double *invR);      // abi_fit.hip
int direct_on_gp(ibo_gp *g, int D, const double *lb, const double *ub, int acq, double parm, int erf_mode,
                 double clamp_lo, int maxiter, int maxtime, int maxsample, int compat,
                 double *opt, double *optx, int64_t *nsamples);                                           // abi_batch.hip

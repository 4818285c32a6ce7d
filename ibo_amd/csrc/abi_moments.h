// abi_moments.h -- the moments pipeline of the acquisitions built on plain sweeps (abi_cacq.hip, abi_ehvi.hip, abi_mes.hip, abi_sparse.hip):
// a chunk of candidates goes through one plain run_sweep per slot -- (mu, s2) into pooled scratch, no acquisition, no arg-max, no
// read-back -- then the unit's finish kernel makes a value of the moments.  The ONE copy of the chunk loop, the chunk length, the padding
// of a short launch, the scratch and the partials, the stream rule, the host batch and the device sweep -- abi_moments.hip.
#pragma once
#include "abi_eval.h"

#include <functional>

#define MOMENT_SLOTS (IBO_CACQ_MAX_CON + 1 > IBO_MARG_MAX ? IBO_CACQ_MAX_CON + 1 : IBO_MARG_MAX)        // (the constrained call's models; an ensemble's members)
#define MOMENT_OUTS 3

// One model of the call.  The scratch holds the arrays the slots ask for in slot order, mu before s2, `stride` doubles apart; a slot
// that is off keeps its places (the constrained objective under IBO_ACQ_NONE).  The same handle may fill several slots.
struct MomentSlot {
    ibo_gp *g = nullptr;
    bool mu = true, s2 = true, on = true;
    double clamp_lo = 0.0;
    int erf_mode = IBO_ERF_LIBM;
};

// What the finish is told about one chunk
struct MomentChunk {
    int64_t m = 0, c0 = 0;               // its candidates, and the first of them in the call's array
    const double *rows = nullptr;        // the rows the sweeps read: the caller's, or the padded copy
    const double *ms = nullptr;          // the scratch
    int64_t stride = 0;
    FinishTail tail;                     // filled for the unit's kernel (ibo_common.h)
    double *at(double *out) const { return out ? out + c0 : nullptr; }       // the chunk's part of a per-candidate output of the call
};
// the unit's kernel over one chunk, launched on the home stream
typedef std::function<int(const MomentChunk &c, hipStream_t s)> moments_finish_t;

struct MomentsPipeline {
    MomentSlot slot[MOMENT_SLOTS];
    int nslots = 0;
    ibo_gp *home = nullptr;              // its stream runs the finish, its buffer holds the exclusions, it reads the arg-max back
    // Whether a short launch is padded to the size class of the call's chunk (class_padded), so that a candidate's moments are the same
    // bits in a sweep, a host batch and a DIRECT batch.  Off for the constrained acquisition alone: its host batches take the other route
    // (eval_host_points per model and the combine on the host), which a padded sweep would not match any better.
    bool padded = true;
    int chunk_opt = 0;                   // the unit's chunk option
    bool timing = false;                 // the unit's timing option: the spans below go to the unit's sums
    double *sweeps_ms = nullptr, *finish_ms = nullptr;       // a chunk's sweeps (first stream to home stream); its finish
    moments_finish_t finish;
    double *out[MOMENT_OUTS] = {nullptr, nullptr, nullptr};  // the call's per-candidate outputs on the device, for the finish to fill
    int64_t mc = 0, stride = 0;          // candidates per chunk; the scratch's stride
    SpanClock clock;
    ScopedBuf<double> ms, pad;

    void add(ibo_gp *g, bool mu, bool s2, double clamp_lo, int erf_mode, bool on = true);
    // the chunk length and the scratch for M candidates, the clock
    int begin(int64_t M);
    // The chunks of cand_dev (device, M x D; cand_rows >= M: the rows it has room for, those from M on being the caller's padding) in
    // ascending order: the slots' sweeps, then the finish with `tail` completed per chunk (pv / pi: the call's partials, or NULL).
    int chunks(int64_t M, const double *cand_dev, int64_t cand_rows, FinishTail tail, double *pv, int64_t *pi);
    // Device candidates: begin, the exclusions, the chunks, then the arg-max if either of its pointers is given; the home stream is idle on return.
    int sweep(int64_t M, const double *cand_dev, int64_t cand_rows, int n_excl, const double *excl_host, double excl_radius, int64_t index_base,
              double *best_val, int64_t *best_idx);
    // Host points: uploaded with their padding (so no copy on the device), the sweep's own route, then k arrays of len[i] doubles read
    // back into host[i] (NULL: not asked for; out[i] is its twin on the device).  The device's values are the sweep's bits.
    int eval_host(int64_t M, const double *Q_host, int k, double *const *host, const size_t *len);

private:
    bool foreign() const;                // whether a slot that is on runs on another stream than home's
};

// Candidates per chunk: the option rounded up to 256, or what keeps the scratch within `budget` bytes, rounded down to 256 (at least
// 256); all of them when they fit.  (abi_sparse.hip cuts its observations by the same rule.)
int64_t moments_chunk_length(int64_t M, int64_t bytes_per_candidate, int chunk_opt, int64_t budget = (int64_t)1 << 30);

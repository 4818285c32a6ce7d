// abi_rows.h -- the row pipeline of the acquisitions built on kg.hip's row kernel (abi_kg.hip, abi_qei.hip, abi_gradobs.hip): a chunk of candidates goes
// through K*, V^T = K* W^T and the row kernel, then the unit's own tail (its cross launch and its last kernel).  The ONE copy of the chunk,
// the chunk length, the scratch, the stages' marks (StageClock: abi_eval.h), the host batch and the device sweep -- abi_rows.hip.
#pragma once
#include "abi_eval.h"
#include "cov.h"
#include "kg.h"

// what ibo_kg_stage_ms and ibo_qei_stage_ms index alike: the unit's resident state, then the five stages of a chunk
enum { ST_STATE = 0, ST_KSTAR, ST_TRI, ST_ROWS, ST_CROSS, ST_TAIL, ROW_STAGES };
static_assert(IBO_KG_STAGES == ROW_STAGES && IBO_QEI_STAGES == ROW_STAGES, "one stage layout");

// the stages after the row kernel: the cross launch, mark(4), the last kernel into out, mark(5)
typedef std::function<int(int m, int mp, const double *cand, double *out)> rows_tail_t;
// K* of a chunk by another kernel than launch_cov_kstar (abi_gradobs.hip: the rows are values AND derivatives): m points at pts -> kt, mp x Npad
typedef std::function<int(const double *pts, int m, int mp, double *kt, hipStream_t s)> rows_kstar_t;

struct RowPipeline {
    ibo_gp *g = nullptr;
    double clamp_lo = 0.0;
    int64_t mc = 0;                                  // candidates per chunk
    size_t ldx = 0;                                  // leading dimension of the cross block; 0: there is none
    bool keep_q = false;                             // the row kernel's |v|^2 is kept (in q)
    StageClock clock;
    rows_tail_t tail;
    rows_kstar_t kstar;                              // empty: launch_cov_kstar on the handle's points
    ScopedBuf<double> cand, kt, vt, mu, q, s2, cross, val;     // one chunk
    // chunk_opt: the unit's chunk option; the chunk is bounded by Npad and by cross_width doubles per candidate
    int begin(ibo_gp *g, double clamp_lo, int chunk_opt, size_t cross_width, size_t ldx, bool keep_q, bool timing, double *ms);
    // room for chunks of up to m candidates (the device is idle: a larger buffer replaces a smaller one)
    int reserve(int64_t m, bool need_cand, bool need_val);
    // One chunk: m <= mc candidates at cand (device, m x D) -> out (device, m); the per-candidate pieces stay in mu / s2 / q / cross.
    // Nothing is waited for unless the stages are being timed.
    int chunk(int m, const double *cand, double *out);
    // Host points in chunks: upload, chunk, read back what is asked for (any of the outputs may be NULL; x_host: the first ncols columns
    // of the cross block, M x ncols).  The device is idle on return.
    int eval_host(int64_t M, const double *Q_host, double *val_host, double *mu_host, double *s2_host, double *x_host, size_t ncols);
    // Device candidates in chunks: the values into out_dev (or scratch), the arg-max if either of its pointers is given, finish_span.
    int sweep(int64_t M, const double *cand_dev, int64_t index_base, double *out_dev, double *best_val, int64_t *best_idx);
};

// the row kernel's arguments for m points Q whose K* and V^T rows are at Kt and Vt (Npad wide); the outputs are the caller's to set
KgRowsArgs rows_args(const ibo_gp *g, const double *Kt, const double *Vt, const double *Q, int m, double clamp_lo);

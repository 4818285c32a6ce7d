// abi_factor.h -- factor-and-invert, once, for everything behind the C ABI that turns an SPD matrix in an identity-padded frame into
// L and W = L^-1 (pad rows zero): the fit, the likelihood gradients, the preference GP's Newton steps and ibo_spd_*.  Host code only
// (abi_factor.hip); the kernels are linalg.hip's and assemble.hip's.
#pragma once
#include "abi_internal.h"

// ---- which order factors an Np-row matrix: it fixes the last bits of L and W, depends on the size and on who asks, and is decided HERE only
enum FactorCaller {
    FACTOR_FIT,         // ibo_gp_fit, ibo_gp_fit_with_matrix, the tail of ibo_pref_finish, ibo_nlml_grad, ibo_loo_grad
    FACTOR_PREF,        // the preference GP's Hessian and C
    FACTOR_IN_PLACE     // ibo_spd_*, the legacy inverse, posterior draws
};
enum FactorRoute {
    ROUTE_RIDE,         // single-level right-looking order, pipelined block columns, W riding along (launch_cholesky_fused)
    ROUTE_RIDE_SUPER,   // the same in super-panels: the same bits (launch_cholesky_super)
    ROUTE_TWO_LEVEL,    // panels of four, K = 256 updates, out of place (launch_cholesky_fused2), W by recursive doubling
    ROUTE_IN_PLACE      // launch_cholesky (single-level up to 32 block columns, panels of four beyond), W by recursive doubling
};
// Below g_fused2_min_nb block columns (104 by default: the single-level order wins up to there -- N = 4096: 2.49 -> 2.07 ms; 6400 rows: 6.20
// against 6.50; 7040: 8.18 against 7.70) the fit and the preference GP take the ride-along, the fit in super-panels from g_super_min_nb on; beyond,
// the fit takes the two-level order and the preference GP the in-place one.  IBO_ERR_ARG where a packed store could not be addressed.
int factor_route(int Np, FactorCaller who, FactorRoute *route);

// ---- sizes every caller's `ensure` uses
static inline size_t alpha_scratch(int Np) { return 2 * (size_t)Np + 2 * (size_t)(Np / 64) * Np + 64; }       // launch_alpha's tmp2
static inline size_t diag64_size(int Np) { return (size_t)(Np / 64) * 4096; }                                   // inverses of the diagonal blocks

// ---- the buffers a caller lends (Np x Np doubles each unless said otherwise; none is kept)
struct FactorBufs {
    double *A;          // the matrix, identity pad in place; destroyed.  ROUTE_IN_PLACE: L on return.  ROUTE_RIDE_SUPER: the tall buffer
                        // [A ; E] (2 Np^2 doubles), eye == A + Np^2
    double *L;          // the factor (the out-of-place routes; its strict upper blocks are not written)
    double *eye;        // ride-along: E's working copy, the identity on entry (written here unless eye_ready); may be W
    double *Et;         // ride-along: (L^-1)^T on return, blocks on and right of the diagonal.  Doubling: scratch
    double *W;          // L^-1 on return, every element written, rows >= N zero
    double *Wp;         // W in MFMA fragment order (pack_w_kernel), or null: none (the doubling tail then packs into Et)
    double *Pk;         // ROUTE_RIDE_SUPER: the packed store, 2 Np^2 doubles.  ROUTE_TWO_LEVEL, ROUTE_IN_PLACE: Np^2 doubles lent to the
                        // packed-operand trailing update, or null (the same bits either way)
    double *d64;        // diag64_size(Np)
    int *info;          // the failing pivot (1-based) or 0; read it with factor_info
    bool info_zero;     // the caller has cleared the info word
    bool eye_ready;     // the caller has written the identity to eye (launch_cov_fit's one pass does both)
};
// Queues the factorisation of b.A (its first N rows are the matrix's own) on `route` and the inversion on s; waits for nothing.
int factor_invert(FactorRoute route, int N, int Np, const FactorBufs &b, hipStream_t s);

// ---- the frame of an Np-row matrix that asks as FACTOR_FIT: out of place on every route -- the matrix in T, the factor into L, the identity's
// working copy in W, (L^-1)^T (or the doubling's scratch) in Et; in super-panels matrix and identity are the halves of ONE tall buffer with
// a packed store of its own (`tall`, `Pk2`: sized here).  Wp (W's packed copy) and Pk (the two-level order's packed-update store) are the
// caller's to lend or not (null): the fits lend T -- free by then, T and Wp then trade places -- and W (free until the inversion), the
// likelihood frame neither (nothing sweeps it).  Picks *route, fills *b with info_zero set; eye_ready is the caller's to set.
int fit_frame(int Np, double *T, double *L, double *W, double *Et, double *Wp, double *Pk, double *d64, int *info,
              DevBuf<double> &tall, DevBuf<double> &Pk2, FactorRoute *route, FactorBufs *b);
// abi_fit.hip: that frame on a handle's own buffers (the caller writes the matrix to b->A), and factor_invert on it with the trade of T and Wp
int fit_operands(ibo_gp *g, FactorRoute *route, FactorBufs *b);
int fit_invert(ibo_gp *g, FactorRoute route, const FactorBufs &b, int N);

// ---- the info word: IBO_ERR_NOT_PD "<noun> is not positive definite (pivot ..)" unless it is zero; *info_out (if given) receives it
int factor_info_word(int h, const char *noun, int *info_out);
int factor_info(const int *info_dev, hipStream_t s, const char *noun, int *info_out);      // fetches it behind everything queued on s (synchronises)

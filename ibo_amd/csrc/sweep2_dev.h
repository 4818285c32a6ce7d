// sweep2_dev.h -- device helpers shared by the second-generation sweep kernels (sweep2.hip: large batches and the
// gallery's rank-1 refresh; small2.hip: DIRECT's batches): buffer-resource loads, the table-based exp, the k*
// value of one exponent and the per-tile candidate staging (the acquisition epilogue, finish_candidate, is in ibo_common.h).
#pragma once
#include "ibo_common.h"

typedef unsigned v4u_t __attribute__((ext_vector_type(4)));
typedef unsigned v2u_t __attribute__((ext_vector_type(2)));

__device__ __forceinline__ __amdgpu_buffer_rsrc_t s2_rsrc(const void *p, size_t bytes)
{
    return __builtin_amdgcn_make_buffer_rsrc((void *)p, 0, (int)(bytes > 0x7fffffffu ? 0x7fffffffu : bytes), 0x00020000);
}

__device__ __forceinline__ double s2_ld_f64(__amdgpu_buffer_rsrc_t r, unsigned voff, unsigned soff)
{
    v2u_t v = __builtin_amdgcn_raw_buffer_load_b64(r, voff, soff, 0);
    return __hiloint2double((int)v.y, (int)v.x);
}

__device__ __forceinline__ double s2_lo(const v4u_t &v) { return __hiloint2double((int)v.y, (int)v.x); }
__device__ __forceinline__ double s2_hi(const v4u_t &v) { return __hiloint2double((int)v.w, (int)v.z); }

// exp(y) for the k* generation in 11 VALU instructions (exp_fast in ibo_common.h takes 17, the library ~30): every
// VALU instruction here is paid in MFMA issue slots.  A 2048-entry table of 2^(j/2048) in LDS (reads are not VALU
// instructions) shortens the polynomial to degree 3:
//   t = y 2048/ln2 + 1.5 2^52 puts n = rint(y 2048/ln2) in the low mantissa bits of t; r = y - n ln2/2048, |r| <=
//   1.7e-4 (r^4/24 < 4e-17); j = n mod 2048 indexes the table and v_ldexp_f64 applies n div 2048, flushing to zero
//   what underflows.  One FMA forms r: the rounding of ln2/2048 costs |n| 2.7e-20 relative -- 2.4e-15 at y = -30
//   where k* is already 1e-13, 5.6e-14 at the underflow threshold (the worst case of that rounding; the constant as written is off by 1.13e-20: 3.4e-17 |y|).
//   Relative error <= 6e-16 + 3.4e-17 |y|: up to 6.4e-16 for |y| < 10 (reached near 10; not the < 5e-16 this comment once claimed), 1.4e-15 at
//   |y| = 35 -- the operation-by-operation restatement of tests/kstar_reference.py against mpmath; tests/test_gpu_kstar_probe.py holds
//   the device to 1e-15 (1 + |y|) over every table entry, both signs of n and the whole range down to underflow.
//   Needs |y| < 7e5 (n must fit 32 bits): the kernel's prologue bounds the scaled candidates so that it holds.
__device__ __forceinline__ double s2_exp(double y, const double *tab)
{
    const double magic = 6755399441055744.0;               // 1.5 * 2^52
    const double t = fma(y, 2954.6394437405970584, magic);              // 2048 / ln 2
    const double n = t - magic;
    const double r = fma(n, -3.384507717577858e-04, y);                 // ln2 / 2048
    const int ti = __double2loint(t);
    const double T = *(const double *)((const char *)tab + ((ti << 3) & (2047 << 3)));
    double p = fma(r, 1.0 / 6.0, 0.5);
    p = fma(p, r, 1.0);
    p = fma(p, r, 1.0);
    return __builtin_amdgcn_ldexp(T * p, ti >> 11);
}

// k* from the exponent y = a_k + b_c + x~.c~ (b_c carries log sf2 for the squared exponential)
template <int FAM>
__device__ __forceinline__ double s2_kstar(double y, double sf2, const double *tab)
{
    if (FAM == FAM_SE) return s2_exp(y, tab);
    const double z = fmax(-2.0 * y, 0.0);                                           // z = |x~ - c~|^2 = -2y
    const double rr = sqrt_fast((FAM == FAM_M3 ? 3.0 : 5.0) * z);
    const double poly = FAM == FAM_M3 ? 1.0 + rr : fma(rr, fma(rr, 1.0 / 3.0, 1.0), 1.0);
    return sf2 * poly * s2_exp(-rr, tab);
}

// TCAND candidates of a tile -> lds_c[cand][KA (+1: odd row stride, conflict-free fragment reads)] = [c~ (D) | 1 | b_c | 0..]  (c~ = c sqrt(w)).  A candidate
// beyond IBO_DOT_PULL_IN is pulled in to that radius, where k* is still 0 exactly (ibo_common.h).  The ONE staging of the dot form: sweep2_kernel,
// sweep2_rank1_kernel and small2.hip's kernels all call it; its two barriers also cover whatever the caller stored to LDS before the call.  cand: where the candidates are read from (nullptr: a.cand).  Called by the whole workgroup; ends with a barrier.
template <int FAM, int TCAND, int KA, int NT>
__device__ __forceinline__ void s2_stage_candidates(const SweepArgs &a, int64_t tile0, double *lds_c, const double *cand = nullptr)
{
    const int tid = threadIdx.x, D = a.kp.D;
    const int64_t M = a.M;
    if (!cand) cand = a.cand;
    for (int e = tid; e < TCAND * KA; e += NT) {
        const int c = e / KA, col = e - c * KA;
        int64_t gi = tile0 + c;
        if (gi > M - 1) gi = M - 1;
        lds_c[c * (KA + 1) + col] = (col < D) ? cand[gi * D + col] * a.kp.sw[col] : (col == D ? 1.0 : 0.0);
    }
    __syncthreads();
    if (tid < TCAND) {
        double n2 = 0.0;
        for (int d = 0; d < D; d++) { const double v = lds_c[tid * (KA + 1) + d]; n2 = fma(v, v, n2); }
        if (n2 > IBO_DOT_PULL_IN) {
            const double sc = sqrt(IBO_DOT_PULL_IN / n2);
            for (int d = 0; d < D; d++) lds_c[tid * (KA + 1) + d] *= sc;
            n2 = IBO_DOT_PULL_IN;
        }
        lds_c[tid * (KA + 1) + D + 1] = fma(-0.5, n2, FAM == FAM_SE ? a.log_sf2 : 0.0);
    }
    __syncthreads();
}

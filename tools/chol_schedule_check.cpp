// chol_schedule_check.cpp -- the pipelined single-level order's launch schedule (ibo_amd/csrc/chol_schedule.h) on its own, on the CPU:
//   g++ -std=c++17 -I ibo_amd/csrc tools/chol_schedule_check.cpp -o /tmp/csc && /tmp/csc
// For every nb from 4 to 362 block columns, with and without the ride-along, as one panel (launch_cholesky_fused) and -- with the
// ride-along, from 32 block columns -- in super-panels of 16 (launch_cholesky_super):
//   (a) pipe8_schedule returns, field by field, what the two loops it replaced computed (transcribed below as they stood);
//   (b) what chol_pipe8_kernel<1> does with those numbers is a right-looking factorisation: within a panel every column receives each
//       earlier step of that panel exactly once, in ascending order, never before the launch that factors the step's column has been
//       queued, and all of them before or inside the launch that factors the column itself; no column outside the panel is touched; and
//       the grid is the row workgroups plus exactly the tiles the kernel enumerates.
// Prints the number of launches checked and "N failure(s)"; the exit status is non-zero if there was one.
#include "chol_schedule.h"

#include <cstdio>
#include <vector>

static const int kSuperPanel = 16;      // (ibo_common.h)

// ---- (a) the loops as they stood before pipe8_schedule: launch_cholesky_fused's `pairs` branch ...
static Pipe8Launch fused_pairs_before(int nb, int jb, bool Ework, int &split)
{
    const int m = nb - jb - 1, nE = Ework ? jb + 1 : 0;
    const int nrow = m + nE + 1;
    const int nE1 = Ework ? 1 : 0;
    int nsingle = 0, q = 0, c_lo = 0, c_hi = 0;
    if (jb & 1) {
        nsingle = m > 0 ? m + nE1 * jb : 0;
        if (jb >= 3) { q = jb - 2; c_lo = split < nb ? split : nb; c_hi = nb; }
    } else if (jb >= 2) {
        q = jb - 1;
        long total = 0, run = 0;
        for (int k = jb + 1; k < nb; k++) total += (nb - k) + nE1 * (q + 1);
        const long later = nb - jb - 2 > 0 ? (nb - jb - 2) + nE1 * (jb + 1) : 0;
        split = jb + 1;
        while (split < nb && (split < jb + 3 || 2 * run < total + later)) { run += (nb - split) + nE1 * (q + 1); split++; }
        c_lo = jb + 1; c_hi = split;
    }
    long npair = 0;
    for (int k = c_lo; k < c_hi; k++) npair += (nb - k) + nE1 * (q + 1);
    return Pipe8Launch{nrow, nsingle, q, c_lo, c_hi, jb > 0 ? 1 : 0, nrow + nsingle + (int)npair};
}
// ... and pipe8_launch_in_panel
static Pipe8Launch in_panel_before(int nb, int jb, int c0, int c1, int &split)
{
    const int m = nb - jb - 1, nE = jb + 1;
    const int nrow = m + nE + 1;
    int nsingle = 0, q = 0, c_lo = 0, c_hi = 0;
    if (jb & 1) {
        if (jb + 1 < c1) nsingle = m + jb;
        if (jb >= c0 + 3) { q = jb - 2; c_lo = split < c1 ? split : c1; c_hi = c1; }
    } else if (jb >= c0 + 2) {
        q = jb - 1;
        long total = 0, run = 0;
        for (int k = jb + 1; k < c1; k++) total += (nb - k) + (q + 1);
        const long later = jb + 2 < c1 ? (nb - jb - 2) + (jb + 1) : 0;
        split = jb + 1;
        while (split < c1 && (split < jb + 3 || 2 * run < total + later)) { run += (nb - split) + (q + 1); split++; }
        c_lo = jb + 1; c_hi = split;
    } else split = c1;
    long npair = 0;
    for (int k = c_lo; k < c_hi; k++) npair += (nb - k) + (q + 1);
    return Pipe8Launch{nrow, nsingle, q, c_lo, c_hi, jb > c0 ? 1 : 0, nrow + nsingle + (int)npair};
}

static long g_launches = 0, g_failures = 0;
static void failure(const char *what, int nb, bool ride, int c0, int c1, int jb, int a = 0, int b = 0)
{
    if (++g_failures <= 20) printf("FAIL %s: nb=%d ride=%d panel [%d, %d) launch %d (%d, %d)\n", what, nb, (int)ride, c0, c1, jb, a, b);
}
static bool same(const Pipe8Launch &x, const Pipe8Launch &y)
{
    return x.nrow == y.nrow && x.nsingle == y.nsingle && x.q == y.q && x.c_lo == y.c_lo && x.c_hi == y.c_hi && x.pre == y.pre && x.grid == y.grid;
}

// One panel [c0, c1).  whole: the panel is launch_cholesky_fused's (compared with fused_pairs_before), else a super-panel's.
static void check_panel(int nb, bool ride, int c0, int c1, bool whole)
{
    int split = c1, split_before = c1;                  // (launch_cholesky_fused starts from nb = c1, launch_cholesky_super from c1)
    // next[k]: the step column k is due next (steps before c0 have come some other way: a deep update, or there are none)
    std::vector<int> next(nb, c0), touched(nb, -1);
    std::vector<char> factored(nb, 0);
    for (int jb = c0; jb < c1; jb++) {
        g_launches++;
        const Pipe8Launch l = pipe8_schedule(nb, jb, c0, c1, ride, split);
        const Pipe8Launch r = whole ? fused_pairs_before(nb, jb, ride, split_before) : in_panel_before(nb, jb, c0, c1, split_before);
        if (!same(l, r) || split != split_before) failure("differs from the loops it replaced", nb, ride, c0, c1, jb, split, split_before);
        // ---- what the kernel does with l (chol_pipe8_kernel<1>)
        const int m = nb - jb - 1, nE = ride ? jb + 1 : 0;
        // row workgroups: blockIdx.x < m + nE are column jb's row blocks and E's rows 0 .. jb, the last one keeps the diagonal block
        if (l.nrow != m + nE + 1) failure("nrow", nb, ride, c0, c1, jb, l.nrow);
        // pre: step jb - 1 on column jb, then the column is factored
        if (l.pre) {
            if (jb - 1 < c0 || !factored[jb - 1]) failure("pre applies a step nobody has factored", nb, ride, c0, c1, jb);
            if (next[jb] != jb - 1) failure("pre out of order", nb, ride, c0, c1, jb, next[jb]);
            next[jb] = jb;
        }
        if (next[jb] != jb) failure("column factored before all its steps arrived", nb, ride, c0, c1, jb, next[jb]);
        touched[jb] = jb;
        long tiles = 0;
        // nsingle tiles: column jb + 1, step jb - 1 alone -- its m matrix tiles (rows jb + 1 ..), then E's rows 0 .. jb - 1
        if (l.nsingle) {
            const int k = jb + 1;
            if (l.nsingle != m + (ride ? jb : 0)) failure("nsingle is not one whole column", nb, ride, c0, c1, jb, l.nsingle);
            if (k >= c1) failure("single step outside the panel", nb, ride, c0, c1, jb, k);
            else {
                if (jb - 1 < c0 || !factored[jb - 1]) failure("single step nobody has factored", nb, ride, c0, c1, jb);
                if (next[k] != jb - 1) failure("single step out of order", nb, ride, c0, c1, jb, k, next[k]);
                next[k] = jb;
                if (touched[k] == jb) failure("column twice in one launch", nb, ride, c0, c1, jb, k);
                touched[k] = jb;
            }
            tiles += l.nsingle;
        }
        // pair tiles: columns [c_lo, c_hi), steps q - 1 and q -- nb - k matrix tiles each, then E's rows 0 .. q (row q: step q alone)
        for (int k = l.c_lo; k < l.c_hi; k++) {
            if (k <= jb || k >= c1) { failure("pair outside the panel's unfactored columns", nb, ride, c0, c1, jb, k); continue; }
            if (l.q - 1 < c0 || l.q >= jb || !factored[l.q - 1] || !factored[l.q]) failure("pair of steps nobody has factored", nb, ride, c0, c1, jb, k, l.q);
            if (next[k] != l.q - 1) failure("pair out of order", nb, ride, c0, c1, jb, k, next[k]);
            next[k] = l.q + 1;
            if (touched[k] == jb) failure("column twice in one launch", nb, ride, c0, c1, jb, k);
            touched[k] = jb;
            tiles += (nb - k) + (ride ? l.q + 1 : 0);
        }
        if (l.grid != l.nrow + tiles) failure("grid", nb, ride, c0, c1, jb, l.grid, (int)(l.nrow + tiles));
        factored[jb] = 1;                               // (the tiles of this launch read only columns factored by earlier launches: checked above)
    }
    for (int k = 0; k < nb; k++) {
        const int want = k < c0 ? c0 : (k < c1 ? k : c0);      // a panel column has all of c0 .. k - 1; every other column is as it was
        if (next[k] != want) failure("steps at the end of the panel", nb, ride, c0, c1, k, next[k], want);
    }
}

int main()
{
    for (int nb = 4; nb <= 362; nb++)
        for (int ride = 0; ride < 2; ride++) {
            check_panel(nb, ride != 0, 0, nb, true);
            if (ride && nb >= 32)
                for (int c0 = 0; c0 < nb; c0 += kSuperPanel) check_panel(nb, true, c0, c0 + kSuperPanel < nb ? c0 + kSuperPanel : nb, false);
        }
    printf("%ld launches checked, %ld failure(s)\n", g_launches, g_failures);
    return g_failures ? 1 : 0;
}

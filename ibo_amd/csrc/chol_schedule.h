// chol_schedule.h -- which launch of the pipelined single-level order applies which step to which block column (chol_pipe8_kernel<1>: two
// steps per pass over the trailing tiles).  Pure host arithmetic, no HIP types: linalg.hip launches from it, tools/chol_schedule_check.cpp
// checks it on the CPU.
#pragma once

struct Pipe8Launch {
    int nrow;           // row workgroups: column jb's row blocks below the diagonal, the ride-along's rows 0 .. jb, the diagonal block's keeper
    int nsingle;        // tiles of column jb + 1 that take step jb - 1 alone (0: none)
    int q;              // the tiles of columns [c_lo, c_hi) take steps q - 1 and q
    int c_lo, c_hi;
    int pre;            // the row workgroups apply step jb - 1 to column jb before they factor it
    int grid;           // workgroups of the launch
};

// Launch jb of the panel of block columns [c0, c1) of an nb-column matrix ((0, nb): the whole matrix is one panel; a column at or beyond c1
// receives nothing here).  The pair of steps (2 p, 2 p + 1) is due on every column right of 2 p + 2 and may ride in launch 2 p + 2 or
// 2 p + 3: the columns up to `split` (at least the two that the next launches factor) take it in the even launch, the rest in the odd
// one -- which also carries step jb - 1 for column jb + 1 alone -- so that both launches have about the same number of tiles to hide under
// their chain.  c0 is even (panels are kSuperPanel = 16 columns wide).  `split` runs from launch to launch of a panel (its value before a panel's first launch is not read).  ride: W = L^-1 rides
// along, a column's tiles then include E's rows.
static inline Pipe8Launch pipe8_schedule(int nb, int jb, int c0, int c1, bool ride, int &split)
{
    const int nE1 = ride ? 1 : 0, m = nb - jb - 1;
    Pipe8Launch l = {m + nE1 * (jb + 1) + 1, 0, 0, 0, 0, jb > c0 ? 1 : 0, 0};
    if (jb & 1) {
        if (jb + 1 < c1) l.nsingle = m + nE1 * jb;
        if (jb >= c0 + 3) { l.q = jb - 2; l.c_lo = split < c1 ? split : c1; l.c_hi = c1; }
    } else if (jb >= c0 + 2) {
        l.q = jb - 1;
        // tiles of column k: (nb - k) of the matrix + (q + 1) of E; half of them, but columns jb + 1 and jb + 2 in any case
        long total = 0, run = 0;
        for (int k = jb + 1; k < c1; k++) total += (nb - k) + nE1 * (l.q + 1);
        const long later = jb + 2 < c1 ? (nb - jb - 2) + nE1 * (jb + 1) : 0;        // the odd launch's own tiles (column jb + 2)
        split = jb + 1;
        while (split < c1 && (split < jb + 3 || 2 * run < total + later)) { run += (nb - split) + nE1 * (l.q + 1); split++; }
        l.c_lo = jb + 1; l.c_hi = split;
    } else split = c1;                                          // a panel's first launch: no pair is due yet
    long npair = 0;
    for (int k = l.c_lo; k < l.c_hi; k++) npair += (nb - k) + nE1 * (l.q + 1);
    l.grid = l.nrow + l.nsingle + (int)npair;
    return l;
}

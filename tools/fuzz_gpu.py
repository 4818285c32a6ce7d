#!/usr/bin/env python3
"""Randomised parity sweep (GPU box): fit + posterior + EI over random (N, D, kernel, M) against the oracle.
python3 tools/fuzz_gpu.py [n_cases] [seed]
FUZZ_SHIFT=1: observations and candidates on the 2^-12 grid, moved by one integer per case drawn from {0, +-3, just below the dot
form's guard, just above it, +-4096} (tests/shift_reference.py); both sides get the shifted data.  Off by default: the seeds of the
summaries in profiles/ reproduce."""
import os, sys, time
import numpy as np
ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
from oracle import oracle as orc
from ibo_amd.gaussianprocess import GaussianProcess
from ibo_amd.gaussianprocess import kernel as K
from ibo_amd.acquisition import sweep

# FUZZ_OPTS="key=value,key=value": ibo_set_option switches for the whole run (e.g. super_min_nb=32: fits from 2048 rows in
# super-panels -- the same oracle, the same bars)
if os.environ.get("FUZZ_OPTS"):
    from ibo_amd import _lib
    for kv in os.environ["FUZZ_OPTS"].split(","):
        k, v = kv.split("="); _lib.check(_lib.lib.ibo_set_option(k.encode(), int(v)))
SHIFT = os.environ.get("FUZZ_SHIFT", "0") != "0"
if SHIFT:
    import shift_reference as sr


def draw_shift(rs, X0, sw):
    """one of 0, +-3, an integer that lands max |x~|^2 just inside / just beyond the guard (either sign), +-4096"""
    which = rs.randint(7)
    sign = 1 if rs.randint(2) else -1
    if which == 0: return 0
    if which in (1, 2): return 3 * sign
    if which in (5, 6): return 4096 * sign
    try:
        return sr.shift_for(X0, sw, *(sr.INSIDE if which == 3 else sr.OUTSIDE), sign=sign)
    except AssertionError:                               # length scales so short that no integer lands in the band
        return 0


ncases = int(sys.argv[1]) if len(sys.argv) > 1 else 40
rs = np.random.RandomState(int(sys.argv[2]) if len(sys.argv) > 2 else 0)
special_N = [1, 2, 15, 16, 17, 63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256, 257, 511, 512, 513, 1023, 1025, 1471, 2047, 2049]
worst = 0.0
t0 = time.time()
for case in range(ncases):
    N = int(special_N[case % len(special_N)] if case < 2 * len(special_N) else rs.randint(1, int(os.environ.get("FUZZ_NMAX", "1500"))))
    D = int(rs.randint(1, int(os.environ.get("FUZZ_DMAX", "32")) + 1))
    kind = ["ard", "iso", "m3", "m5"][rs.randint(4)]
    M = int([1, 3, 16, 17, 64, 65, 1000, 8192, 8193, 20000][rs.randint(10)])
    noise = float([.1, .01, 1e-3][rs.randint(3)])
    X = rs.rand(N, D); Y = np.sin(3 * X.sum(1)) + .01 * rs.randn(N)
    th = np.exp(rs.uniform(np.log(.2), np.log(1.5), size=D)) * max(1.0, np.sqrt(D / 8.))      # distances grow with sqrt(D)
    if kind == "ard": hyp = th; ours = K.GaussianKernel_ard(hyp)
    elif kind == "iso": hyp = th[:1]; ours = K.GaussianKernel_iso(hyp)
    elif kind == "m3": hyp = np.r_[th[0], 1.0]; ours = K.MaternKernel3(hyp)
    else: hyp = np.r_[th[0], 1.0]; ours = K.MaternKernel5(hyp)
    cand = None
    shift = 0
    if SHIFT:
        X0 = np.floor(X * sr.GRID) / sr.GRID
        Y = np.sin(3 * X0.sum(1)) + .01 * rs.randn(N)
        shift = draw_shift(rs, X0, sr.scale_of(kind, list(hyp), D))
        X = X0 + shift
        cand = np.floor(rs.rand(M, D) * sr.GRID) / sr.GRID + shift
    ogp = orc.GP(orc.Kern(kind, hyp), X, Y, noise=noise)
    try:
        np.linalg.cholesky(ogp.factor_matrix())
    except np.linalg.LinAlgError:
        continue
    gp = GaussianProcess(ours, X, Y, noise=noise)
    if cand is None:
        cand = rs.rand(M, D)
    Mo = min(M, 300)                                    # the oracle's share (it is O(N^2) per point, scalar)
    r = sweep(gp, cand, acq='ei', xi=.01, native=True, outputs=("mu", "s2", "acq"))
    o = orc.sweep_native(ogp, cand[:Mo], orc.ACQ_EI, .01)
    em = np.max(np.abs(r["mu"][:Mo] - o["mu"]) / np.maximum(np.abs(o["mu"]), 1e-9))
    es = np.max(np.abs(r["s2"][:Mo] - o["s2"]) / np.maximum(np.abs(o["s2"]), 1e-9))
    ea = np.max(np.abs(r["acq"][:Mo] - o["acq"]) / np.maximum(np.abs(o["acq"]), 1e-9) * (np.abs(o["acq"]) > 1e-12))
    ok_idx = int(np.argmax(r["acq"])) == r["best_idx"]
    worst = max(worst, em, es, ea)
    flag = "" if (max(em, es, ea) < 1e-6 and ok_idx) else "   <-- FAIL"
    print("N=%5d D=%2d %-3s M=%6d noise=%g%s  rel err mu %.1e s2 %.1e ei %.1e argmax %s%s" %
          (N, D, kind, M, noise, "  shift %d %s" % (shift, r["kernel"]) if SHIFT else "", em, es, ea, ok_idx, flag), flush=True)
print("worst relative error %.2e over %d cases, %.1f s" % (worst, ncases, time.time() - t0))

# --- DIRECT: maximizeEI / PI / UCB on the GPU objective against the oracle's sequential run -----------------
# (informational: the two objectives differ by ~1e-13 relative, so a strict comparison inside DIRECT can in
# principle go the other way on a near-tie; a mismatch in the sample count is reported, not asserted)
if os.environ.get("FUZZ_DIRECT", "1") != "0":
    from ibo_amd.acquisition import maximizeEI, maximizePI, maximizeUCB
    nd = int(os.environ.get("FUZZ_DIRECT_CASES", "12"))
    same = 0
    for case in range(nd):
        N = int(rs.randint(5, 160)); D = int(rs.randint(1, 5))
        X = rs.rand(N, D); Y = np.sin(3 * X.sum(1)) + .05 * rs.randn(N)
        th = np.exp(rs.uniform(np.log(.2), np.log(1.0), size=D))
        gp = GaussianProcess(K.GaussianKernel_ard(th), X, Y, noise=.05)
        ogp = orc.GP(orc.Kern("ard", th), X, Y, noise=.05)
        b = [[0., 1.]] * D
        which = case % 3
        if which == 0:
            opt, optx = maximizeEI(gp, b, xi=.01, maxiter=25); o = orc.acqmax_native(ogp, b, orc.ACQ_EI, .01, maxiter=25)
        elif which == 1:
            opt, optx = maximizePI(gp, b, xi=.01, maxiter=25); o = orc.acqmax_native(ogp, b, orc.ACQ_PI, .01, maxiter=25)
        else:
            from ibo_amd.acquisition import _ucb_parm
            parm = _ucb_parm(gp, b, .1, .2)
            opt, optx = maximizeUCB(gp, b, maxiter=25); o = orc.acqmax_native(ogp, b, orc.ACQ_UCB, parm, maxiter=25)
        ok = np.array_equal(np.asarray(optx), o[1]) and abs(opt - o[0]) <= 1e-6 * max(abs(o[0]), 1e-12)
        same += ok
        print("DIRECT %-3s N=%3d D=%d  opt %.6g (oracle %.6g)  same point: %s" % (["EI", "PI", "UCB"][which], N, D, opt, o[0], ok), flush=True)
        if not ok:
            acq = [orc.ACQ_EI, orc.ACQ_PI, orc.ACQ_UCB][which]
            pr = .01 if which < 2 else parm
            vv = orc.sweep_native(ogp, np.vstack([np.asarray(optx), o[1]]), acq, pr)["acq"]
            print("    ours x=%s  oracle x=%s   oracle's acquisition at both: %.17g  %.17g  (rel. diff %.1e)" %
                  (np.asarray(optx), o[1], vv[0], vv[1], abs(vv[0] - vv[1]) / max(abs(vv[1]), 1e-300)), flush=True)
    print("DIRECT: %d of %d runs end on the oracle's point" % (same, nd))

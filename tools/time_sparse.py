"""
Timing of the sparse GP on inducing points in one warm process: medians of the host clock around each call (the calls block), SE-ARD, D = 4.

  fit      N = 2^17 / m = 1024 and N = 2^20 / m = 2048: wall time and, from a second set of calls under ibo_set_option("sgp_timing", 1)
           (HIP events around every stage; the option makes a call wait once more per stage, so the wall times are taken without it),
           the stages q-sweep, generation, Gram, assemble, factor-and-invert.  The Gram stage as TFLOP/s over 2 mp^2 N / 2 useful
           flops (the lower tiles) -- beside the knowledge gradient's cross stage on the same tile body (README).
  sweep    EI over 2^20 device candidates at m = 1024 beside two plain sweeps of a 1024-row model called one after the other
  add      addData of 1, 1024 and 65536 rows onto the N = 2^17 model
  point    one host point; maximizeEI (maxiter 50)
  plain    a plain fit and EI sweep at N = 16384 for context

Prints one JSON object.

    python tools/time_sparse.py [--reps 15] [--small] [--out FILE]
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
STAGES = ("q_sweep", "generation", "gram", "assemble", "factor_invert", "cand_sweeps", "finish")


def median_ms(f, reps, warm=2):
    for _ in range(warm):
        f()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        f()
        t.append(time.perf_counter() - t0)
    return 1e3 * float(np.median(t))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--small", action="store_true", help="N = 2^14 / m = 256 only (a quick look)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from ibo_amd import _lib, DeviceArray
    from ibo_amd.gaussianprocess import GaussianProcess, SparseGaussianProcess
    from ibo_amd.gaussianprocess.kernel import GaussianKernel_ard
    from ibo_amd.acquisition import maximizeEI, sweep
    if _lib.device_count() < 1:
        raise SystemExit("no GPU: nothing to time")
    L = _lib.lib
    D, M = 4, 1 << 20
    rs = np.random.RandomState(5)
    kern = GaussianKernel_ard([.3] * D)
    res = {"clock": "wall: host (time.perf_counter around blocking calls); stages: HIP events; medians of %d after 2 warm-up calls" % args.reps}

    def data(N):
        X = rs.rand(N, D)
        return X, np.sin(3 * X.sum(1)) + .1 * rs.randn(N)

    def stage_ms(f):
        _lib.check(L.ibo_set_option(b"sgp_timing", 1))
        ms, rows = np.zeros(8), []
        try:
            for k in range(1 + max(3, args.reps // 3)):
                _lib.check(L.ibo_sgp_stage_ms(None, 1))
                f()
                _lib.check(L.ibo_sgp_stage_ms(_lib.dp(ms), 1))
                if k >= 1:
                    rows.append(ms.copy())
        finally:
            _lib.check(L.ibo_set_option(b"sgp_timing", 0))
        med = np.median(np.array(rows), axis=0)
        return {STAGES[i]: float(med[i]) for i in range(len(STAGES))}

    fits = []
    models = {}
    for N, m in (((1 << 14, 256),) if args.small else ((1 << 17, 1024), (1 << 20, 2048))):
        X, Y = data(N)
        Z = rs.rand(m, D)
        box = {}

        def fit():
            old = box.get("g")
            box["g"] = SparseGaussianProcess(kern, X, Y, Z=Z, noise=.1)
            if old is not None:
                old.close()
        reps = args.reps if N <= (1 << 17) else max(3, args.reps // 3)
        wall = median_ms(fit, reps, warm=1)
        st = stage_ms(fit)
        mp = (m + 63) // 64 * 64
        nt = (mp + 64) // 64
        fits.append(dict(N=N, m=m, fit_ms=wall, stages_ms=st, gram_tflops_useful=(mp * mp * float(N)) / (st["gram"] * 1e-3) / 1e12,
                         gram_tflops_issued=(2.0 * 64 * 64 * nt * (nt + 1) / 2 * N) / (st["gram"] * 1e-3) / 1e12))
        models[(N, m)] = box["g"]
    res["fit"] = fits
    key = sorted(models)[0]
    g = models[key]
    m = key[1]
    # the EI sweep beside two plain sweeps of an m-row model
    dc = DeviceArray.from_host(rs.rand(M, D))
    Xp, Yp = data(m)
    plain = GaussianProcess(kern, Xp, Yp, noise=.1)
    bv, bi = ctypes.c_double(), ctypes.c_int64()
    acq = DeviceArray((M,))

    def two_plain():
        for _ in range(2):
            _lib.check(L.ibo_acq_sweep(plain._handle(), M, dc.ptr, _lib.ACQ_EI, 0.01, _lib.ERF_LIBM, _lib.CLAMP_NATIVE, float("nan"), 0, None, .5, 0,
                                       None, None, acq.ptr, ctypes.byref(bv), ctypes.byref(bi)))
    sp = median_ms(lambda: sweep(g, dc, 'ei'), args.reps)
    tp = median_ms(two_plain, args.reps)
    res["sweep"] = dict(candidates=M, m=m, sparse_ei_sweep_ms=sp, two_plain_sweeps_ms=tp, ratio=sp / tp, stages_ms=stage_ms(lambda: sweep(g, dc, 'ei')))
    # addData
    adds = []
    for n in (1, 1024, 65536):
        Xa, Ya = data(n)
        adds.append(dict(rows=n, add_ms=median_ms(lambda: g.addData(Xa, Ya), max(3, args.reps // 3), warm=1)))
    res["add"] = adds
    q = rs.rand(1, D)
    res["point"] = dict(posterior_ms=median_ms(lambda: g.posterior(q[0]), 10 * args.reps),
                        maximizeEI_ms=median_ms(lambda: maximizeEI(g, [[0., 1.]] * D, maxiter=50), args.reps))
    if not args.small:
        Xf, Yf = data(16384)
        box = {}

        def pfit():
            box["g"] = GaussianProcess(kern, Xf, Yf, noise=.1)
        res["plain"] = dict(N=16384, fit_ms=median_ms(pfit, 3, warm=1), ei_sweep_ms=median_ms(lambda: sweep(box["g"], dc, 'ei'), 3, warm=1))
    s = json.dumps(res, indent=1)
    print(s)
    if args.out:
        with open(args.out, "w") as f:
            f.write(s + "\n")


if __name__ == "__main__":
    main()

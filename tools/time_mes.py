"""
Timing of max-value entropy search in one warm process: medians of the host clock around each call (the calls block).

  sweep    C2 (N = 1024, D = 4, 2^20 device candidates): ibo_mes_sweep at K = 8, 64 and 1024 samples of the maximum beside one
           plain ibo_acq_sweep on the same handle and array with mu_dev / s2_dev asked for.  The difference is the scan over the
           samples and what goes with it (sample upload, scratch, the final reduction), on the host clock.  The scan kernel's own
           device time comes from HIP events around its launch (ibo_set_option("mes_timing", 1), ibo_mes_scan_ms) in a second set of
           calls -- the option makes a call wait once more, so the wall times are taken without it -- and from it picoseconds per
           term h(gamma) (K 2^20 terms).
  maxcdf   ibo_mes_maxcdf over 2^16 candidates at 64 levels: wall time, and the reduction kernel's device time
  batch    one ibo_mes_batch point (K = 64) beside one ibo_acq_batch point
  direct   maximizeMES (K = 64 given samples, maxiter 50; and with the samples drawn by the Gumbel fit) beside maximizeEI

Prints one JSON object.

    python tools/time_mes.py [--reps 15] [--samples 8,64,1024] [--sweep-only] [--out FILE]
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def median_ms(f, reps):
    for _ in range(2):
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
    ap.add_argument("--samples", default="8,64,1024")
    ap.add_argument("--sweep-only", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from ibo_amd import _lib, DeviceArray
    from ibo_amd.gaussianprocess import GaussianProcess
    from ibo_amd.gaussianprocess.kernel import GaussianKernel_ard
    from ibo_amd.acquisition import maximizeEI
    from ibo_amd.acquisition.entropy import maximizeMES, sweepMES
    if _lib.device_count() < 1:
        raise SystemExit("no GPU: nothing to time")
    L = _lib.lib
    N, D, M = 1024, 4, 1 << 20
    rs = np.random.RandomState(5)
    X = rs.rand(N, D)
    Y = np.sin(3 * X.sum(1)) + .01 * rs.randn(N)
    GP = GaussianProcess(GaussianKernel_ard([.3] * D), X, Y, noise=.1)
    dc = DeviceArray.from_host(rs.rand(M, D))
    mu, s2 = DeviceArray((M,)), DeviceArray((M,))
    bv, bi = ctypes.c_double(), ctypes.c_int64()
    res = {"shape": dict(N=N, D=D, M=M), "clock": "wall: host (time.perf_counter around blocking calls); scan_kernel_ms: HIP events around the launch; "
                                                  "medians of %d after 2 warm-up calls" % args.reps}

    def plain():
        _lib.check(L.ibo_acq_sweep(GP._handle(), M, dc.ptr, _lib.ACQ_NONE, 0.0, _lib.ERF_LIBM, _lib.CLAMP_PY, float("nan"), 0, None, .5, 0,
                                   mu.ptr, s2.ptr, None, ctypes.byref(bv), ctypes.byref(bi)))

    def scan_ms(f):
        """median, min and max device time of the scan kernels over the calls f()"""
        _lib.check(L.ibo_set_option(b"mes_timing", 1))
        t, scan = ctypes.c_double(), []
        try:
            for k in range(2 + args.reps):
                _lib.check(L.ibo_mes_scan_ms(None, 1))
                f()
                _lib.check(L.ibo_mes_scan_ms(ctypes.byref(t), 1))
                if k >= 2:
                    scan.append(t.value)
        finally:
            _lib.check(L.ibo_set_option(b"mes_timing", 0))
        return float(np.median(scan)), [float(np.min(scan)), float(np.max(scan))]

    base = median_ms(plain, args.reps)
    sweeps = []
    for K in [int(k) for k in args.samples.split(",")]:
        ys = float(Y.max()) + .05 + 1.5 * rs.rand(K)
        ms = median_ms(lambda: sweepMES(GP, dc, ys), args.reps)
        k_ms, k_range = scan_ms(lambda: sweepMES(GP, dc, ys))
        sweeps.append(dict(samples=K, mes_sweep_ms=ms, plain_sweep_ms=base, scan_and_rest_ms=ms - base, scan_kernel_ms=k_ms,
                           scan_kernel_min_max_ms=k_range, ps_per_term=1e9 * k_ms / (K * M)))
    res["sweep"] = dict(plain_sweep_ms=base, mes=sweeps)
    if not args.sweep_only:
        Mc = 1 << 16
        sub = dc.view_rows(0, Mc)
        lev = _lib.f64(np.linspace(float(Y.max()), float(Y.max()) + 2.0, 64))
        out, stats = np.empty(64), np.empty(2)
        cdf = lambda: _lib.check(L.ibo_mes_maxcdf(GP._handle(), Mc, sub.ptr, 64, _lib.dp(lev), .1, _lib.CLAMP_PY, _lib.dp(out), _lib.dp(stats)))
        k_ms, k_range = scan_ms(cdf)
        res["maxcdf"] = dict(candidates=Mc, levels=64, maxcdf_ms=median_ms(cdf, args.reps), reduce_kernel_ms=k_ms, reduce_kernel_min_max_ms=k_range,
                             ps_per_log_cdf=1e9 * k_ms / (64 * Mc))
        ys = _lib.f64(float(Y.max()) + .05 + 1.5 * rs.rand(64))
        Q = _lib.f64(rs.rand(1, D))
        a, b, v = np.empty(1), np.empty(1), np.empty(1)
        one = median_ms(lambda: _lib.check(L.ibo_acq_batch(GP._handle(), 1, _lib.dp(Q), _lib.ACQ_NONE, 0.0, _lib.ERF_LIBM, _lib.CLAMP_PY, float("nan"),
                                                           _lib.dp(a), _lib.dp(b), None)), 10 * args.reps)
        ms = median_ms(lambda: _lib.check(L.ibo_mes_batch(GP._handle(), 64, _lib.dp(ys), .1, 1, _lib.dp(Q), _lib.CLAMP_PY, _lib.dp(v))), 10 * args.reps)
        res["batch"] = dict(points=1, samples=64, mes_batch_ms=ms, acq_batch_ms=one)
        bounds = [[0., 1.]] * D
        res["direct"] = [dict(what="maximizeEI", ms=median_ms(lambda: maximizeEI(GP, bounds, maxiter=50), args.reps)),
                         dict(what="maximizeMES", samples=64, ms=median_ms(lambda: maximizeMES(GP, bounds, ystar=ys, maxiter=50), args.reps)),
                         dict(what="maximizeMES with the Gumbel samples drawn (4096 candidates)", samples=64,
                              ms=median_ms(lambda: maximizeMES(GP, bounds, n_samples=64, seed=1, maxiter=50), args.reps))]
    s = json.dumps(res, indent=1)
    print(s)
    if args.out:
        with open(args.out, "w") as f:
            f.write(s + "\n")


if __name__ == "__main__":
    main()

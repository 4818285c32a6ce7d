"""
Timing of the two-objective expected hypervolume improvement in one warm process: medians of the host clock around each call
(the calls block; a call spans two handles, so no single handle's events cover it).

  sweep    C2 (two models of N = 1024, D = 4, 2^20 device candidates): ibo_ehvi_sweep at fronts of 0, 16, 128 and 1024 points
           beside the SUM of two plain ibo_acq_sweep calls on the same handles and array with mu_dev / s2_dev asked for.  The
           difference is the strip scan and what goes with it (front upload, scratch, the final reduction), on the host clock.
           The scan kernel's own device time comes from HIP events around its launch (ibo_set_option("ehvi_timing", 1),
           ibo_ehvi_scan_ms) in a second set of calls -- the option makes a call wait once more, so the wall times are taken
           without it -- and from it picoseconds per strip and candidate ((n + 1) 2^20 strips) and per cdf / pdf pair.
  batch    one ibo_ehvi_batch point (front of 128) beside two ibo_acq_batch points
  direct   maximizeEHVI (front of 128, maxiter 50) beside maximizeEI on the first model

Prints one JSON object.

    python tools/time_ehvi.py [--reps 15] [--fronts 0,16,128,1024] [--sweep-only] [--out FILE]
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


def arc_front(n, ref, top):
    """n mutually non-dominated points on a concave arc between ref and top"""
    t = (np.arange(n) + .5) / max(n, 1)
    return np.c_[ref[0] + (top[0] - ref[0]) * t, ref[1] + (top[1] - ref[1]) * np.sqrt(1.0 - t * t)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--fronts", default="0,16,128,1024")
    ap.add_argument("--sweep-only", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from ibo_amd import _lib, DeviceArray
    from ibo_amd.gaussianprocess import GaussianProcess
    from ibo_amd.gaussianprocess.kernel import GaussianKernel_ard
    from ibo_amd.acquisition import maximizeEI
    from ibo_amd.acquisition.multiobjective import maximizeEHVI, sweepEHVI
    if _lib.device_count() < 1:
        raise SystemExit("no GPU: nothing to time")
    L = _lib.lib
    N, D, M = 1024, 4, 1 << 20
    rs = np.random.RandomState(5)
    X1, X2 = rs.rand(N, D), rs.rand(N, D)
    Y1 = np.sin(3 * X1.sum(1)) + .01 * rs.randn(N)
    Y2 = np.cos(2 * X2[:, 0]) - X2[:, -1] + .01 * rs.randn(N)
    GPs = [GaussianProcess(GaussianKernel_ard([.3] * D), X, Y, noise=.1) for X, Y in ((X1, Y1), (X2, Y2))]
    ref = np.array([Y1.min() - .1, Y2.min() - .1])
    top = ref + .7 * (np.array([Y1.max(), Y2.max()]) - ref)
    dc = DeviceArray.from_host(rs.rand(M, D))
    mu, s2 = DeviceArray((M,)), DeviceArray((M,))
    bv, bi = ctypes.c_double(), ctypes.c_int64()
    res = {"shape": dict(N=N, D=D, M=M), "clock": "wall: host (time.perf_counter around blocking calls); scan_kernel_ms: HIP events around the launch; "
                                                  "medians of %d after 2 warm-up calls" % args.reps}

    def plain(GP):
        _lib.check(L.ibo_acq_sweep(GP._handle(), M, dc.ptr, _lib.ACQ_NONE, 0.0, _lib.ERF_LIBM, _lib.CLAMP_NATIVE, float("nan"), 0, None, .5, 0,
                                   mu.ptr, s2.ptr, None, ctypes.byref(bv), ctypes.byref(bi)))
    per_model = [median_ms(lambda GP=GP: plain(GP), args.reps) for GP in GPs]
    base = float(np.sum(per_model))
    sweeps = []
    for n in [int(k) for k in args.fronts.split(",")]:
        F = arc_front(n, ref, top)
        ms = median_ms(lambda: sweepEHVI(GPs, dc, ref, front=F), args.reps)
        _lib.check(L.ibo_set_option(b"ehvi_timing", 1))
        scan = []
        for k in range(2 + args.reps):
            _lib.check(L.ibo_ehvi_scan_ms(None, 1))
            sweepEHVI(GPs, dc, ref, front=F)
            t = ctypes.c_double()
            _lib.check(L.ibo_ehvi_scan_ms(ctypes.byref(t), 1))
            if k >= 2:
                scan.append(t.value)
        _lib.check(L.ibo_set_option(b"ehvi_timing", 0))
        k_ms = float(np.median(scan))
        sweeps.append(dict(front=n, ehvi_sweep_ms=ms, two_plain_sweeps_ms=base, scan_and_rest_ms=ms - base,
                           scan_kernel_ms=k_ms, scan_kernel_min_max_ms=[float(np.min(scan)), float(np.max(scan))],
                           ps_per_strip_and_candidate=1e9 * k_ms / ((n + 1) * M), ps_per_cdf_pdf_pair=1e9 * k_ms / (2 * (n + 1) * M)))
    res["sweep"] = dict(plain_sweep_ms=per_model, ehvi=sweeps)
    if not args.sweep_only:
        F = arc_front(128, ref, top)
        Q = _lib.f64(rs.rand(1, D))
        a, b, v = np.empty(1), np.empty(1), np.empty(1)
        one = [median_ms(lambda GP=GP: _lib.check(L.ibo_acq_batch(GP._handle(), 1, _lib.dp(Q), _lib.ACQ_NONE, 0.0, _lib.ERF_LIBM, _lib.CLAMP_NATIVE,
                                                                  float("nan"), _lib.dp(a), _lib.dp(b), None)), 10 * args.reps) for GP in GPs]
        objs = (ctypes.c_void_p * 2)(*[GP._handle() for GP in GPs])
        Fc, rc = _lib.f64(F), _lib.f64(ref)
        ms = median_ms(lambda: _lib.check(L.ibo_ehvi_batch(objs, len(Fc), _lib.dp(Fc), _lib.dp(rc), 1, _lib.dp(Q), _lib.ERF_LIBM, _lib.CLAMP_NATIVE,
                                                           _lib.dp(v))), 10 * args.reps)
        res["batch"] = dict(points=1, front=128, ehvi_batch_ms=ms, acq_batch_ms=one)
        bounds = [[0., 1.]] * D
        res["direct"] = [dict(what="maximizeEI", ms=median_ms(lambda: maximizeEI(GPs[0], bounds, maxiter=50), args.reps)),
                         dict(what="maximizeEHVI", front=128, ms=median_ms(lambda: maximizeEHVI(GPs, bounds, ref, front=F, maxiter=50), args.reps))]
    s = json.dumps(res, indent=1)
    print(s)
    if args.out:
        with open(args.out, "w") as f:
            f.write(s + "\n")


if __name__ == "__main__":
    main()

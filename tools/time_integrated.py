"""
Timing of the integrated acquisitions in one warm process: medians of the host clock around each call (the calls block;
an integrated call spans several handles, so no single handle's events cover it).

  sweep      C2 (N = 1024, D = 4, 2^20 candidates) with S = 1, 4, 16 members: ibo_iacq_sweep beside the SUM of S plain ibo_acq_sweep calls
             on the same handles with mu_dev / s2_dev asked for; the expectation is that sum plus a finish of 16 S bytes per candidate
  finish     marg_finish_kernel's device time from HIP events (ibo_set_option("iacq_timing")) and the bytes/s it stands for
  sampler    sampleHyper at N = 1024, D = 4, n = 16, chains = 8: wall time (median, as everything here) and the number of ibo_nlml_grid
             calls of one run
  maximiser  maximizeIntegratedEI at S = 8 beside maximizeEI on one member

Prints one JSON object.

    python tools/time_integrated.py [--reps 15] [--out FILE]
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
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from ibo_amd import _lib, DeviceArray
    from ibo_amd.gaussianprocess import GaussianProcess, GaussianProcessEnsemble
    from ibo_amd.gaussianprocess.hypersample import sampleHyper
    from ibo_amd.gaussianprocess.kernel import GaussianKernel_ard
    from ibo_amd.acquisition import maximizeEI, maximizeIntegratedEI
    if _lib.device_count() < 1:
        raise SystemExit("no GPU: nothing to time")
    L = _lib.lib
    N, D, M = 1024, 4, 1 << 20
    rs = np.random.RandomState(5)
    X = rs.rand(N, D)
    Y = np.sin(3 * X.sum(1)) + .01 * rs.randn(N)
    gps = [GaussianProcess(GaussianKernel_ard(.3 * np.exp(.2 * rs.randn(D))), X, Y, noise=.1) for _ in range(16)]
    ymax = float(np.max(Y))
    dc = DeviceArray.from_host(rs.rand(M, D))
    mu, s2, val = (DeviceArray((M,)) for _ in range(3))
    bv, bi = ctypes.c_double(), ctypes.c_int64()
    res = {"shape": dict(N=N, D=D, M=M)}

    def plain(GP):
        _lib.check(L.ibo_acq_sweep(GP._handle(), M, dc.ptr, _lib.ACQ_NONE, .01, _lib.ERF_LIBM, _lib.CLAMP_NATIVE, ymax, 0, None, .5, 0,
                                   mu.ptr, s2.ptr, None, ctypes.byref(bv), ctypes.byref(bi)))
    per_model = [median_ms(lambda GP=GP: plain(GP), args.reps) for GP in gps]

    def integrated(S, want_val=True):
        h = (ctypes.c_void_p * S)(*[g._handle() for g in gps[:S]])
        w = _lib.f64(np.full(S, 1.0 / S))
        _lib.check(L.ibo_iacq_sweep(h, S, _lib.dp(w), M, dc.ptr, _lib.ACQ_EI, .01, _lib.ERF_LIBM, _lib.CLAMP_NATIVE, ymax, 0, None, .5, 0,
                                    val.ptr if want_val else None, None, None, ctypes.byref(bv), ctypes.byref(bi)))
    sweeps = []
    for S in (1, 4, 16):
        ms = median_ms(lambda: integrated(S), args.reps)
        base = float(np.sum(per_model[:S]))
        stage = np.zeros(2)
        _lib.check(L.ibo_set_option(b"iacq_timing", 1))
        try:
            integrated(S)
            _lib.check(L.ibo_iacq_stage_ms(None, 1))
            for _ in range(args.reps):
                integrated(S)
            _lib.check(L.ibo_iacq_stage_ms(_lib.dp(stage), 1))
        finally:
            _lib.check(L.ibo_set_option(b"iacq_timing", 0))
        fin = float(stage[1]) / args.reps
        nbytes = M * (16.0 * S + 8.0)                # (mu, s2) per member in, val out; without exclusion balls no coordinate is loaded
        sweeps.append(dict(S=S, integrated_ms=ms, sum_of_plain_sweeps_ms=base, ratio=ms / base, sweeps_device_ms=float(stage[0]) / args.reps,
                           finish_device_ms=fin, finish_bytes_in_per_candidate=16 * S, finish_GB_per_s=nbytes / (fin * 1e-3) / 1e9 if fin > 0 else None))
    res["sweep"] = dict(plain_sweep_ms=per_model, integrated=sweeps)

    kern = GaussianKernel_ard([.3] * D)
    from ibo_amd.gaussianprocess import hypersample
    grid, calls = hypersample.trainhyper.nlml_values, []

    def counting(*a, **kw):                          # (every round of the sampler is one such call)
        calls.append(1)
        return grid(*a, **kw)
    hypersample.trainhyper.nlml_values = counting
    try:
        phi, lp = sampleHyper(kern, X, Y, n=16, chains=8, noise=1e-3, seed=0)
        per_run = len(calls)
        sampler_ms = median_ms(lambda: sampleHyper(kern, X, Y, n=16, chains=8, noise=1e-3, seed=0), args.reps)
    finally:
        hypersample.trainhyper.nlml_values = grid
    res["sampler"] = dict(n=16, chains=8, wall_ms=sampler_ms, grid_calls=per_run, ms_per_grid_call=sampler_ms / per_run,
                          mean_log_theta=[float(v) for v in phi.mean(axis=0)])

    E = GaussianProcessEnsemble.from_members(gps[:8])
    bounds = [[0., 1.]] * D
    res["maximiser"] = [dict(what="maximizeEI", ms=median_ms(lambda: maximizeEI(gps[0], bounds, maxiter=50), args.reps)),
                        dict(what="maximizeIntegratedEI", S=8, ms=median_ms(lambda: maximizeIntegratedEI(E, bounds, maxiter=50), args.reps)),
                        dict(what="maximizeIntegratedEI(polish=True)", S=8,
                             ms=median_ms(lambda: maximizeIntegratedEI(E, bounds, maxiter=50, polish=True), args.reps))]
    s = json.dumps(res, indent=1)
    print(s)
    if args.out:
        with open(args.out, "w") as f:
            f.write(s + "\n")


if __name__ == "__main__":
    main()

"""
Timing of the constrained acquisition in one warm process: medians of the host clock around each call (the calls block; a
constrained call spans several handles, so no single handle's events cover it).

  sweep    C2 (N = 1024, D = 4, 2^20 candidates) with two constraint models of the same size: ibo_cacq_sweep beside the SUM of
           the three plain ibo_acq_sweep calls on the same handles with mu_dev / s2_dev asked for
  batches  ibo_cacq_batch on DIRECT-sized batches (64 and 512 points) beside ibo_acq_batch per model: what the host-side
           combine adds to a DIRECT batch
  direct   maximizeCEI with one and with two constraints beside maximizeEI on the objective alone (N = 1024, D = 4)

Prints one JSON object.

    python tools/time_constrained.py [--reps 15] [--out FILE]
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
    from ibo_amd.gaussianprocess import GaussianProcess
    from ibo_amd.gaussianprocess.kernel import GaussianKernel_ard
    from ibo_amd.acquisition import maximizeEI
    from ibo_amd.acquisition.constrained import Constraint, maximizeCEI, sweepConstrained, feasibleIncumbent
    if _lib.device_count() < 1:
        raise SystemExit("no GPU: nothing to time")
    L = _lib.lib
    N, D, M = 1024, 4, 1 << 20
    rs = np.random.RandomState(5)
    X = rs.rand(N, D)
    Yo = np.sin(3 * X.sum(1)) + .01 * rs.randn(N)
    Y1 = np.cos(2 * X[:, 0]) - X[:, -1] + .01 * rs.randn(N)
    Y2 = ((X - .5) ** 2).sum(1) + .01 * rs.randn(N)
    ell = [.3] * D
    GPo, GP1, GP2 = (GaussianProcess(GaussianKernel_ard(ell), X, Y, noise=.1) for Y in (Yo, Y1, Y2))
    t1, t2 = float(np.percentile(Y1, 60)), float(np.percentile(Y2, 40))
    cons = [Constraint(GP1, upper=t1), Constraint(GP2, lower=t2)]
    ymax = feasibleIncumbent(GPo, cons)
    dc = DeviceArray.from_host(rs.rand(M, D))
    mu, s2, val = (DeviceArray((M,)) for _ in range(3))
    bv, bi = ctypes.c_double(), ctypes.c_int64()
    res = {"shape": dict(N=N, D=D, M=M), "ymax": ymax}

    def plain(GP, acq):
        _lib.check(L.ibo_acq_sweep(GP._handle(), M, dc.ptr, acq, .01, _lib.ERF_LIBM, _lib.CLAMP_NATIVE, ymax, 0, None, .5, 0,
                                   mu.ptr, s2.ptr, None, ctypes.byref(bv), ctypes.byref(bi)))
    per_model = [median_ms(lambda GP=GP: plain(GP, _lib.ACQ_EI if GP is GPo else _lib.ACQ_NONE), args.reps) for GP in (GPo, GP1, GP2)]
    sweeps = []
    for n in (0, 1, 2):
        ms = median_ms(lambda: sweepConstrained(GPo, cons[:n], dc, acq='ei', ymax=ymax), args.reps)
        base = float(np.sum(per_model[:n + 1]))
        sweeps.append(dict(ncon=n, constrained_ms=ms, sum_of_plain_sweeps_ms=base, ratio=ms / base))
    res["sweep"] = dict(plain_sweep_ms=per_model, constrained=sweeps)

    batches = []
    for m in (64, 512):
        Q = _lib.f64(rs.rand(m, D))
        a, b, c = np.empty(m), np.empty(m), np.empty(m)
        one = [median_ms(lambda GP=GP: _lib.check(L.ibo_acq_batch(GP._handle(), m, _lib.dp(Q), _lib.ACQ_EI, .01, _lib.ERF_LIBM,
                                                                  _lib.CLAMP_NATIVE, ymax, _lib.dp(a), _lib.dp(b), None)), 10 * args.reps)
               for GP in (GPo, GP1, GP2)]
        for n in (1, 2):
            con = (ctypes.c_void_p * n)(*[k.GP._handle() for k in cons[:n]])
            th = _lib.f64([k.thresh for k in cons[:n]]); se = (ctypes.c_int * n)(*[k.sense for k in cons[:n]])
            ms = median_ms(lambda: _lib.check(L.ibo_cacq_batch(GPo._handle(), n, con, _lib.dp(th), se, m, _lib.dp(Q), _lib.ACQ_EI, .01,
                                                               _lib.ERF_LIBM, _lib.CLAMP_NATIVE, ymax, None, None, _lib.dp(c))), 10 * args.reps)
            base = float(np.sum(one[:n + 1]))
            batches.append(dict(points=m, ncon=n, cacq_batch_ms=ms, sum_of_acq_batches_ms=base, combine_and_rest_ms=ms - base))
    res["batches"] = batches

    bounds = [[0., 1.]] * D
    direct = [dict(what="maximizeEI", ms=median_ms(lambda: maximizeEI(GPo, bounds, maxiter=50), args.reps))]
    for n in (1, 2):
        direct.append(dict(what="maximizeCEI", ncon=n, ms=median_ms(lambda: maximizeCEI(GPo, cons[:n], bounds, maxiter=50, ymax=ymax), args.reps)))
    res["direct"] = direct
    s = json.dumps(res, indent=1)
    print(s)
    if args.out:
        with open(args.out, "w") as f:
            f.write(s + "\n")


if __name__ == "__main__":
    main()

"""
Timing of ibo_acq_grad_batch against ibo_acq_batch on the same points, and of maximizeEI with and without polish, in one
process after warm-up (host clock around calls that end in a device synchronise).  Prints one JSON object.

    python tools/time_grad.py [--reps 200] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def synth(seed, N, D):
    rs = np.random.RandomState(seed)
    X = rs.rand(N, D)
    return X, np.sin(3 * X.sum(1)) + 0.01 * rs.randn(N)


def best_of(f, reps):
    for _ in range(5):
        f()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter(); f(); ts.append(time.perf_counter() - t0)
    return 1e3 * float(np.median(ts)), 1e3 * float(np.min(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from ibo_amd import _lib
    from ibo_amd.gaussianprocess import GaussianProcess
    from ibo_amd.gaussianprocess.kernel import GaussianKernel_ard
    from ibo_amd.acquisition import maximizeEI, EI
    if _lib.device_count() < 1:
        raise SystemExit("no GPU: nothing to time")
    res = {"single_point": [], "batch": [], "polish": []}
    for N, D in ((1024, 4), (2048, 4)):
        X, Y = synth(12, N, D)
        GP = GaussianProcess(GaussianKernel_ard(np.linspace(.3, .45, D)), X, Y, noise=.1)
        h = GP._handle()
        q = _lib.f64(np.random.RandomState(1).rand(1, D))
        v, g = np.empty(1), np.empty((1, D))
        acq = lambda: _lib.check(_lib.lib.ibo_acq_batch(h, 1, _lib.dp(q), 0, .01, 0, 1e-8, float("nan"), None, None, _lib.dp(v)))
        grd = lambda: _lib.check(_lib.lib.ibo_acq_grad_batch(h, 1, _lib.dp(q), 0, .01, 0, 1e-8, float("nan"), None, None, _lib.dp(v),
                                                              None, None, _lib.dp(g)))
        gonly = lambda: _lib.check(_lib.lib.ibo_acq_grad_batch(h, 1, _lib.dp(q), 0, .01, 0, 1e-8, float("nan"), None, None, None,
                                                               None, None, _lib.dp(g)))
        a, b, c = best_of(acq, args.reps), best_of(grd, args.reps), best_of(gonly, args.reps)
        res["single_point"].append(dict(N=N, D=D, acq_batch_ms=a[0], grad_batch_ms=b[0], grad_only_ms=c[0], ratio=b[0] / a[0]))
    N, D, M = 2048, 8, 1024
    X, Y = synth(3, N, D)
    GP = GaussianProcess(GaussianKernel_ard(np.linspace(.5, .8, D)), X, Y, noise=.1)
    h = GP._handle()
    Q = _lib.f64(np.random.RandomState(2).rand(M, D))
    v, g = np.empty(M), np.empty((M, D))
    acq = lambda: _lib.check(_lib.lib.ibo_acq_batch(h, M, _lib.dp(Q), 0, .01, 0, 1e-8, float("nan"), None, None, _lib.dp(v)))
    grd = lambda: _lib.check(_lib.lib.ibo_acq_grad_batch(h, M, _lib.dp(Q), 0, .01, 0, 1e-8, float("nan"), None, None, _lib.dp(v),
                                                          None, None, _lib.dp(g)))
    a, b = best_of(acq, max(10, args.reps // 4)), best_of(grd, max(10, args.reps // 4))
    res["batch"].append(dict(N=N, D=D, M=M, acq_batch_ms=a[0], grad_batch_ms=b[0], ratio=b[0] / a[0],
                             grad_gflops=2.0 * N * N * M / (b[0] * 1e-3) / 1e9))
    # the C2 model: maximizeEI with and without the polish
    X, Y = synth(12, 1024, 4)
    GP = GaussianProcess(GaussianKernel_ard(np.array([.3, .35, .4, .45])), X, Y, noise=.1)
    bounds = [[0., 1.]] * 4
    outs = {}
    for pol in (False, True):
        outs[pol] = maximizeEI(GP, bounds, polish=pol)
        ts = []
        for _ in range(20):
            t0 = time.perf_counter(); outs[pol] = maximizeEI(GP, bounds, polish=pol); ts.append(time.perf_counter() - t0)
        outs[(pol, "ms")] = 1e3 * float(np.median(ts))
    res["polish"].append(dict(N=1024, D=4, direct_ms=outs[(False, "ms")], polished_ms=outs[(True, "ms")],
                              added_ms=outs[(True, "ms")] - outs[(False, "ms")], ei_direct=outs[False][0], ei_polished=outs[True][0],
                              gain_rel=(outs[True][0] - outs[False][0]) / abs(outs[False][0]),
                              x_direct=list(map(float, outs[False][1])), x_polished=list(map(float, outs[True][1]))))
    s = json.dumps(res, indent=1)
    print(s)
    if args.out:
        with open(args.out, "w") as f:
            f.write(s + "\n")


if __name__ == "__main__":
    main()

"""
Timing of leave-one-out prediction on a fitted handle (GaussianProcess.loo, ibo_gp_loo) and of the LOO-CV objective with and
without its gradient (trainhyper.looLikelihood, ibo_loo_grad), in one warm process: medians of the device time the library
measures with events (ibo_gpu_time_ms, the difference around each call) and of the host clock around each call, beside
marginalLikelihood (ibo_nlml_grad) at the same shape and one posterior(x).  NumPy float64 doing the same work on the host's CPUs
is timed once, for context.  Prints one JSON object.  Kernel times: run it under `rocprofv3 --kernel-trace --stats -- python3
tools/time_loo.py --reps 5 --no-numpy`.

    python tools/time_loo.py [--reps 20] [--no-numpy] [--out FILE]
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


def timed(f, reps, gpu_ms):
    """(median device ms, median host ms) of f over reps calls after two warm-up calls"""
    for _ in range(2):
        f()
    dev, host = [], []
    for _ in range(reps):
        g0 = gpu_ms(); t0 = time.perf_counter()
        f()
        host.append(time.perf_counter() - t0); dev.append(gpu_ms() - g0)
    return float(np.median(dev)), 1e3 * float(np.median(host))


def numpy_loo(X, Y, ell, noise, grad):
    """the objective (and gradient) of an SE-ARD kernel in NumPy float64: Cholesky inverse, then T = B dK_h per length scale"""
    from scipy.linalg import cho_factor, cho_solve
    N, D = X.shape
    z = np.zeros((N, N))
    for d in range(D):
        z += ((X[:, d, None] - X[None, :, d]) / ell[d]) ** 2
    K = np.exp(-0.5 * z)
    B = cho_solve(cho_factor(K + noise * np.eye(N), lower=True), np.eye(N))
    al, dg = B @ Y, np.diag(B)
    v = np.sum(-0.5 * np.log(dg) + al * al / (2 * dg)) + 0.5 * N * np.log(2 * np.pi)
    g = np.zeros(D if grad else 0)
    for h in range(len(g)):
        T = B @ (K * ((X[:, h, None] - X[None, :, h]) / ell[h]) ** 2)
        g[h] = -np.sum((al * (T @ al) - 0.5 * (1 + al * al / dg) * np.sum(T * B, axis=1)) / dg)
    return v, g


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--no-numpy", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from ibo_amd import _lib
    from ibo_amd.gaussianprocess import GaussianProcess
    from ibo_amd.gaussianprocess.kernel import GaussianKernel_ard
    from ibo_amd.gaussianprocess.trainhyper import looLikelihood, marginalLikelihood
    if _lib.device_count() < 1:
        raise SystemExit("no GPU: nothing to time")
    gpu_ms = _lib.gpu_time_ms
    res = {"handle": [], "likelihood": [], "numpy": []}
    for N in (1024, 2048, 4096):
        X, Y = synth(3, N, 8)
        GP = GaussianProcess(GaussianKernel_ard(np.linspace(.5, .8, 8)), X, Y, noise=.1)
        _, loo_ms = timed(GP.loo, args.reps, gpu_ms)
        _, post_ms = timed(lambda: GP.posterior(X[0] + .01), args.reps, gpu_ms)
        res["handle"].append(dict(N=N, D=8, loo_host_us=1e3 * loo_ms, posterior_host_us=1e3 * post_ms))
    for N, D in ((1024, 4), (2048, 8), (4096, 16)):
        X, Y = synth(3, N, D)
        ell = np.linspace(.5, .8, D) * max(1.0, np.sqrt(D) / 2)
        k = GaussianKernel_ard(ell)
        reps = args.reps if N < 4096 else max(3, args.reps // 4)
        dv, hv = timed(lambda: looLikelihood(k, X, Y, D, False, noise=1e-2), reps, gpu_ms)
        dg, hg = timed(lambda: looLikelihood(k, X, Y, D, True, noise=1e-2), reps, gpu_ms)
        dn, hn = timed(lambda: marginalLikelihood(k, X, Y, D, True, noise=1e-2), reps, gpu_ms)
        flops = 2.0 * D * float(N) ** 3
        res["likelihood"].append(dict(N=N, D=D, ngrad=D, value_only_device_ms=dv, value_only_host_ms=hv, with_gradient_device_ms=dg,
                                      with_gradient_host_ms=hg, nlml_grad_device_ms=dn, nlml_grad_host_ms=hn, gflop=flops / 1e9,
                                      product_device_ms=dg - dv, product_tflops=flops / ((dg - dv) * 1e-3) / 1e12,
                                      pct_of_78_6=100.0 * flops / ((dg - dv) * 1e-3) / 78.6e12))
        if not args.no_numpy:
            v, g = looLikelihood(k, X, Y, D, True, noise=1e-2)
            t0 = time.perf_counter(); nv, _ = numpy_loo(X, Y, ell, 1e-2, False); tv = time.perf_counter() - t0
            t0 = time.perf_counter(); nv, ng = numpy_loo(X, Y, ell, 1e-2, True); tg = time.perf_counter() - t0
            res["numpy"].append(dict(N=N, D=D, value_only_s=tv, with_gradient_s=tg, value_abs_diff=abs(nv - v),
                                     grad_max_abs_diff=float(np.max(np.abs(ng - g)))))
    s = json.dumps(res, indent=1)
    print(s)
    if args.out:
        with open(args.out, "w") as f:
            f.write(s + "\n")


if __name__ == "__main__":
    main()

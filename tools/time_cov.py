"""
Timing of the joint posterior (ibo_posterior_cov), of posterior draws (GaussianProcess.sample_posterior) and of
thompsonGallery, in one warm process: medians of the device time the library measures with events (ibo_gpu_time_ms, the
difference around each call) and of the host clock around each call.  NumPy float64 doing the same work on the host's CPUs
is timed once, for context.  Prints one JSON object.  Kernel times: run it under `rocprofv3 --kernel-trace --stats -- python3
tools/time_cov.py --reps 5`.

    python tools/time_cov.py [--reps 30] [--out FILE]
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


def numpy_sigma(X, Q, w, noise):
    """the same Sigma in NumPy float64 (SE kernel, sf2 = 1): K*, cho_solve, K(Q, Q) + noise I - K*^T R^-1 K*"""
    from scipy.linalg import cho_factor, cho_solve

    def k(A, B):
        z = np.zeros((len(A), len(B)))
        for d in range(A.shape[1]):
            z += w[d] * (A[:, d, None] - B[None, :, d]) ** 2
        return np.exp(-0.5 * z)
    R = k(X, X) + noise * np.eye(len(X))
    Ks = k(X, Q)
    return k(Q, Q) + noise * np.eye(len(Q)) - Ks.T @ cho_solve(cho_factor(R, lower=True), Ks)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from ibo_amd import _lib
    from ibo_amd.gaussianprocess import GaussianProcess
    from ibo_amd.gaussianprocess.kernel import GaussianKernel_ard, MaternKernel5
    from ibo_amd.acquisition.gallery import thompsonGallery
    if _lib.device_count() < 1:
        raise SystemExit("no GPU: nothing to time")
    gpu_ms = _lib.gpu_time_ms
    res = {"sigma": [], "draws": [], "thompson": [], "numpy": []}
    for N, D, M in ((2048, 8, 4096), (1024, 4, 1024)):
        X, Y = synth(3, N, D)
        ell = np.linspace(.5, .8, D)
        GP = GaussianProcess(GaussianKernel_ard(ell), X, Y, noise=.1)
        h = GP._handle()
        Q = _lib.f64(np.random.RandomState(2).rand(M, D))
        S = np.empty((M, M))
        call = lambda: _lib.check(_lib.lib.ibo_posterior_cov(h, M, _lib.dp(Q), 1, None, _lib.dp(S)))
        dev, host = timed(call, args.reps, gpu_ms)
        flops = float(N) * N * M + float(N) * M * M
        res["sigma"].append(dict(N=N, D=D, M=M, device_ms=dev, host_ms=host, gflop=flops / 1e9, device_tflops=flops / (dev * 1e-3) / 1e12,
                                 pct_of_78_6=100.0 * flops / (dev * 1e-3) / 78.6e12))
        t0 = time.perf_counter()
        Sn = numpy_sigma(X, np.asarray(Q), 1.0 / ell ** 2, .1)
        res["numpy"].append(dict(what="sigma", N=N, D=D, M=M, ms=1e3 * (time.perf_counter() - t0),
                                 max_abs_diff=float(np.max(np.abs(Sn - S)))))
        if M == 4096:
            t0 = time.perf_counter()
            L = np.linalg.cholesky(Sn + 1e-12 * np.eye(M))
            _ = np.random.default_rng(0).standard_normal((64, M)) @ L.T
            res["numpy"].append(dict(what="cholesky + 64 draws", M=M, ms=1e3 * (time.perf_counter() - t0)))
            draw = lambda: GP.sample_posterior(Q, n=64, seed=1)
            dev, host = timed(draw, args.reps, gpu_ms)
            res["draws"].append(dict(N=N, D=D, M=M, n=64, device_ms=dev, host_ms=host))
    # the C3-like model (N = 2048, D = 8, Matern-5/2) over 4096 candidates
    X, Y = synth(3, 2048, 8)
    GP = GaussianProcess(MaternKernel5([.5, 1.0]), X, Y, noise=.1)
    C = np.random.RandomState(103).rand(4096, 8)
    dev, host = timed(lambda: GP.sample_posterior(C, n=64, seed=1), args.reps, gpu_ms)
    res["draws"].append(dict(model="c3", N=2048, D=8, M=4096, n=64, device_ms=dev, host_ms=host))
    gal = []
    dev, host = timed(lambda: gal.append(thompsonGallery(GP, C, 8, seed=1)), args.reps, gpu_ms)
    res["thompson"].append(dict(model="c3", N=2048, D=8, M=4096, gallery=8, draws=64, device_ms=dev, host_ms=host,
                                members=len(gal[-1])))
    s = json.dumps(res, indent=1)
    print(s)
    if args.out:
        with open(args.out, "w") as f:
            f.write(s + "\n")


if __name__ == "__main__":
    main()

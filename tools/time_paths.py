"""
Timing of the pathwise posterior draws (ibo_paths_*) in one warm process, medians of --reps calls:
  * creation (spectral draws on the host, then ibo_paths_create) at N = 1024 and 2048, F = 2048, S = 64
  * the sweep at the C2 shape (N = 1024, D = 4, SE-ARD, 2^20 candidates) with F = 2048 and S = 8 and 64: wall time of
    ibo_paths_sweep (arg-max only), as TFLOP/s over 2 M (Fp + Np32) S, beside the EI sweep of the same model over the same array
  * thompsonSweepGallery(N = 8) on the C3 model (N = 2048, D = 8, Matern-5/2) over 2^19 candidates
  * GaussianProcess.sample_posterior(n = 64) at M = 4096 on the C2 model, for context
Prints one JSON object.

    python tools/time_paths.py [--reps 5] [--M 1048576] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def synth(seed, N, D):
    rs = np.random.RandomState(seed)
    X = rs.rand(N, D)
    return X, np.sin(3 * X.sum(1)) + 0.01 * rs.randn(N)


def med(f, reps):
    f()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        f()
        t.append(1e3 * (time.perf_counter() - t0))
    return float(np.median(t))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--M", type=int, default=1 << 20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from ibo_amd import _lib, DeviceArray
    from ibo_amd.acquisition import PosteriorPaths, spectralDraws, sweep
    from ibo_amd.acquisition.gallery import thompsonSweepGallery
    from ibo_amd.gaussianprocess import GaussianProcess
    from ibo_amd.gaussianprocess.kernel import GaussianKernel_ard, MaternKernel5
    if _lib.device_count() < 1:
        raise SystemExit("no GPU: nothing to time")
    M, F = args.M, 2048
    res = {"M": M, "F": F, "create": [], "sweep": []}
    models = {}
    for N in (1024, 2048):
        X, Y = synth(2, N, 4)
        GP = GaussianProcess(GaussianKernel_ard([.3] * 4), X, Y, noise=.1)
        models[N] = GP
        held = []

        def create():
            held[:] = [PosteriorPaths(GP, n_paths=64, n_features=F, seed=1)]
        ms = med(create, args.reps)
        host = med(lambda: spectralDraws(GP.kernel, 4, F, 64, N, .1, 1), args.reps)
        res["create"].append(dict(N=N, S=64, wall_ms=ms, host_draws_ms=host))
        held[0].close()
    GP = models[1024]
    cand = DeviceArray.from_host(np.random.RandomState(102).rand(M, 4), GP._dev.device)
    sweep(GP, cand)
    ei = []
    for _ in range(args.reps):
        t0 = time.perf_counter()
        r = sweep(GP, cand)
        ei.append((1e3 * (time.perf_counter() - t0), r["kernel_ms"]))
    ei_flops = float(1024 ** 2 + 3 * 1024 * 4 + 4 * 1024) * M
    ei_wall, ei_kernel = float(np.median([e[0] for e in ei])), float(np.median([e[1] for e in ei]))
    res["ei_sweep"] = dict(N=1024, wall_ms=ei_wall, kernel_ms=ei_kernel, tflops=ei_flops / (ei_kernel * 1e-3) / 1e12)
    for S in (8, 64):
        P = PosteriorPaths(GP, n_paths=S, n_features=F, seed=1)
        ms = med(lambda: P.sweep(cand), args.reps)
        flops = 2.0 * M * (F + 1024) * S
        res["sweep"].append(dict(N=1024, S=S, wall_ms=ms, tflops=flops / (ms * 1e-3) / 1e12, tflops_of_the_64_columns_computed=2.0 * M * (F + 1024) * 64 / (ms * 1e-3) / 1e12,
                                 over_ei_sweep_wall=ms / ei_wall))
        P.close()
    X, Y = synth(3, 2048, 8)
    G3 = GaussianProcess(MaternKernel5([.5, 1.0]), X, Y, noise=.1)
    c3 = DeviceArray.from_host(np.random.RandomState(103).rand(1 << 19, 8), G3._dev.device)
    held = []

    def gallery():
        held[:] = [thompsonSweepGallery(G3, c3, 8, seed=1)]
    res["thompson_sweep_gallery"] = dict(N=2048, D=8, M=1 << 19, paths=64, wall_ms=med(gallery, max(1, args.reps // 2)), members=len(held[0]))
    Q = np.random.RandomState(5).rand(4096, 4)
    res["sample_posterior"] = dict(N=1024, M=4096, n=64, wall_ms=med(lambda: GP.sample_posterior(Q, n=64, seed=1), max(1, args.reps // 2)))
    s = json.dumps(res, indent=1)
    print(s)
    if args.out:
        with open(args.out, "w") as f:
            f.write(s + "\n")


if __name__ == "__main__":
    main()

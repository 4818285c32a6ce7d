"""
Timing of the pathwise draws' gradients (ibo_paths_grad_batch) on the C2 model (N = 1024, D = 4, SE-ARD) with
F = 2048 features and S = 64 paths, in one warm process, medians of --reps calls:
  * one ibo_paths_grad_batch call (values and gradients of every path) at M = 1, 64 and 1024, beside one ibo_paths_batch call at
    the same M, and beside the 2 D + 1 = 9 ibo_paths_batch calls of central differences that one gradient call replaces
  * PosteriorPaths.maxima for the 64 paths (default candidates), with the sweep alone (polish=False) beside it
  * PosteriorPaths.maximize(polish=True) beside maximize() for one path
Prints one JSON object.

    python tools/time_paths_grad.py [--reps 15] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


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
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from ibo_amd import _lib
    from ibo_amd.acquisition import PosteriorPaths
    from ibo_amd.gaussianprocess import GaussianProcess
    from ibo_amd.gaussianprocess.kernel import GaussianKernel_ard
    if _lib.device_count() < 1:
        raise SystemExit("no GPU: nothing to time")
    N, D, F, S = 1024, 4, 2048, 64
    rs = np.random.RandomState(2)
    X = rs.rand(N, D)
    GP = GaussianProcess(GaussianKernel_ard([.3] * D), X, np.sin(3 * X.sum(1)) + 0.01 * rs.randn(N), noise=.1)
    P = PosteriorPaths(GP, n_paths=S, n_features=F, seed=1)
    res = {"N": N, "D": D, "F": F, "S": S, "reps": args.reps, "grad_batch": []}
    for M in (1, 64, 1024):
        Q = np.random.RandomState(5).rand(M, D)
        E = [np.zeros((M, D)) for _ in range(D)]
        for d in range(D):
            E[d][:, d] = 1e-5

        def differences():
            P.values(Q)
            for d in range(D):
                P.values(Q + E[d]); P.values(Q - E[d])
        g = med(lambda: P.gradient(Q), args.reps)
        v = med(lambda: P.values(Q), args.reps)
        fd = med(differences, args.reps)
        res["grad_batch"].append(dict(M=M, grad_batch_ms=g, paths_batch_ms=v, nine_paths_batch_calls_ms=fd, grad_over_nine_calls=g / fd))
    bounds = [[0., 1.]] * D
    res["maxima"] = dict(paths=S, candidates=4096, wall_ms=med(lambda: P.maxima(bounds), args.reps),
                         sweep_only_ms=med(lambda: P.maxima(bounds, polish=False), args.reps))
    plain = med(lambda: P.maximize(bounds, path=0), args.reps)
    polished = med(lambda: P.maximize(bounds, path=0, polish=True), args.reps)
    o0, o1 = P.maximize(bounds, path=0)[0], P.maximize(bounds, path=0, polish=True)[0]
    res["maximize"] = dict(path=0, wall_ms=plain, polish_wall_ms=polished, opt=o0, polish_opt=o1)
    P.close()
    s = json.dumps(res, indent=1)
    print(s)
    if args.out:
        with open(args.out, "w") as f:
            f.write(s + "\n")


if __name__ == "__main__":
    main()

"""
Timing of the removal of one observation from a fitted model (GaussianProcess.removeData, ibo_gp_remove) beside what it replaces and what
it goes with, in one warm process: medians of the device time the library measures with events (last_fit_ms of each call: a removal, an
extension and a fit all report there) and of the host clock around each call.  Per shape:
    one removal at i = 0, N / 2 and N - 1       (the model is restored by a refit between repetitions, outside the clock)
    a refit of the N - 1 remaining rows         (what a removal cost before)
    one addData                                 (the O(N^2) step in the other direction)
    a window step                               (add one point, remove row 0)
and fit / remove(i = 0), the ratio GaussianProcess.REMOVE_MAX is read off at N = 1024, D = 4.  Prints one JSON object.

    python tools/time_remove.py [--reps 20] [--out FILE]
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


def timed(setup, f, reps):
    """(median device ms, median host ms) of f(model) over reps calls, each on a model setup() has just made, after two warm-up rounds"""
    dev, host = [], []
    for r in range(reps + 2):
        GP = setup()
        t0 = time.perf_counter()
        ms = f(GP)
        dt = time.perf_counter() - t0
        if r >= 2:
            dev.append(ms); host.append(dt)
    return float(np.median(dev)), 1e3 * float(np.median(host))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from ibo_amd import _lib
    from ibo_amd.gaussianprocess import GaussianProcess
    from ibo_amd.gaussianprocess.kernel import GaussianKernel_ard
    if _lib.device_count() < 1:
        raise SystemExit("no GPU: nothing to time")
    res = {"shapes": [], "REMOVE_MAX_in_source": GaussianProcess.REMOVE_MAX}
    for N, D in ((1024, 4), (2048, 8), (4096, 16)):
        X, Y = synth(3, N + 1, D)
        kern = GaussianKernel_ard(np.linspace(.5, .8, D) * max(1.0, np.sqrt(D) / 2))
        reps = args.reps if N < 4096 else max(5, args.reps // 2)
        GP = GaussianProcess(kern, X[:N], Y[:N], noise=.1, reserve_rows=1)

        def restore():
            GP.X, GP.Y = X[:N], Y[:N]
            GP._fit_device()
            return GP

        def remove(i):
            def f(g):
                g.removeData(i, _route="device")
                return g.last_fit_ms()
            return f

        def refit(g):
            g.X, g.Y = X[1:N], Y[1:N]
            g._fit_device()
            return g.last_fit_ms()

        def add(g):
            g.addData(X[N], Y[N])
            return g.last_fit_ms()

        def window(g):
            g.addData(X[N], Y[N])
            ms = g.last_fit_ms()
            g.removeData(0, _route="device")
            return ms + g.last_fit_ms()

        row = dict(N=N, D=D)
        for name, i in (("remove_first", 0), ("remove_middle", N // 2), ("remove_last", N - 1)):
            row[name + "_device_ms"], row[name + "_host_ms"] = timed(restore, remove(i), reps)
        row["refit_device_ms"], row["refit_host_ms"] = timed(restore, refit, reps)
        row["add_device_ms"], row["add_host_ms"] = timed(restore, add, reps)
        row["window_device_ms"], row["window_host_ms"] = timed(restore, window, reps)
        row["fit_over_remove_first"] = row["refit_device_ms"] / row["remove_first_device_ms"]
        # bytes a removal at i = 0 moves at the least: L read + written, W read twice + written, the repack's read and two writes
        gb = 8.0 * (2 + 3 + 3) * float(N) ** 2 / 1e9
        row["remove_first_gbytes"] = gb
        row["remove_first_tb_per_s"] = gb / row["remove_first_device_ms"]
        res["shapes"].append(row)
        GP._dev.close()
    s = json.dumps(res, indent=1)
    print(s)
    if args.out:
        with open(args.out, "w") as f:
            f.write(s + "\n")


if __name__ == "__main__":
    main()

"""
Timing of the gradient-observation model's marginal likelihood with its gradient (ibo_ggp_nlml_grad) in one warm process, SE-ARD.

  shapes   N = 256, D = 4 (P = 1280 rows) and N = 1024, D = 3 (P = 4096 rows)
  wall     medians of the host clock around the blocking call: one evaluation (value, D derivatives, 1 + D noise terms); beside it
           ibo_nlml_grad on a plain model of P rows in D dimensions -- the same factorisation, alpha and K^-1 = W^T W, so the two differ
           in the assembly and the contraction only -- and the model's own fit (ibo_ggp_fit)
  stages   from a second set of calls under ibo_set_option("ggp_timing", 1) (HIP events around every stage): assembly,
           factor-and-invert with alpha, K^-1, contraction.  The contraction as bytes/s over the P^2 / 2 doubles of K^-1's lower half it
           has to read once.
  learn    GaussianProcess(G=).learn(maxiter=30) at the smaller shape from length scales a factor 2 off: wall time, evaluations

Prints one JSON object.

    python tools/time_gradobs_learn.py [--reps 15] [--out FILE]
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
STAGES = ("assembly", "factor_invert_alpha", "kinv", "contraction")
THETA = {4: [0.5, 0.7, 0.6, 0.8], 3: [0.5, 0.7, 0.6]}
NOISE, GNOISE = 0.05, 0.02


def median_ms(f, reps, warm=2):
    for _ in range(warm):
        f()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        f()
        t.append(time.perf_counter() - t0)
    return 1e3 * float(np.median(t))


def objective(X):
    a = 0.6 + 1.1 * np.abs(np.sin(1.0 + np.arange(X.shape[1])))
    ph = X @ a + 0.3
    return 0.5 * np.sin(ph), 0.5 * np.cos(ph)[:, None] * a[None, :]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from ibo_amd import _lib
    from ibo_amd.gaussianprocess import GaussianProcess
    from ibo_amd.gaussianprocess.kernel import GaussianKernel_ard
    if _lib.device_count() < 1:
        raise SystemExit("no GPU: nothing to time")
    L, dp, dev = _lib.lib, _lib.dp, _lib.default_device()
    rs = np.random.RandomState(5)
    res = {"clock": "wall: host (time.perf_counter around blocking calls); stages: HIP events; medians of %d warm calls" % args.reps, "rows": []}
    for N, D in ((256, 4), (1024, 3)):
        P = N * (D + 1)
        X = _lib.f64(rs.rand(N, D))
        Y, G = objective(X)
        Y, G = _lib.f64(Y), _lib.f64(G)
        hyper = _lib.f64(THETA[D]); gno = _lib.f64([GNOISE] * D)
        modes = (ctypes.c_int * D)(*([0] * D)); dims = (ctypes.c_int * D)(*range(D))
        v = ctypes.c_double(); g = np.empty(D); gz = np.empty(D + 1)

        def evaluate():
            _lib.check(L.ibo_ggp_nlml_grad(dev, _lib.K_SE_ARD, N, D, dp(X), dp(Y), dp(G), dp(hyper), D, 1.0, NOISE, dp(gno), D, modes, dims,
                                           ctypes.byref(v), dp(g), dp(gz)))

        def value_only():
            _lib.check(L.ibo_ggp_nlml_grad(dev, _lib.K_SE_ARD, N, D, dp(X), dp(Y), dp(G), dp(hyper), D, 1.0, NOISE, dp(gno), 0, None, None,
                                           ctypes.byref(v), None, None))

        # a plain model of P rows in the same D dimensions (in a cube whose side keeps the point density of the N points)
        Xp = _lib.f64(rs.rand(P, D) * (P / float(N)) ** (1.0 / D)); Yp = _lib.f64(objective(Xp)[0])
        vp = ctypes.c_double(); gp = np.empty(D)

        def plain():
            _lib.check(L.ibo_nlml_grad(dev, _lib.K_SE_ARD, P, D, dp(Xp), dp(Yp), dp(hyper), D, 1.0, NOISE, D, modes, dims, ctypes.byref(vp), dp(gp)))

        h = ctypes.c_void_p()
        _lib.check(L.ibo_ggp_create(dev, ctypes.byref(h)))
        info = ctypes.c_int()

        def fit():
            _lib.check(L.ibo_ggp_fit(h, _lib.K_SE_ARD, N, D, dp(X), dp(Y), dp(G), dp(hyper), D, 1.0, NOISE, dp(gno), ctypes.byref(info)))

        row = {"N": N, "D": D, "P": P, "evaluation_ms": median_ms(evaluate, args.reps), "value_only_ms": median_ms(value_only, args.reps),
               "plain_nlml_grad_P_rows_ms": median_ms(plain, args.reps), "fit_ms": median_ms(fit, args.reps)}
        _lib.check(L.ibo_ggp_destroy(h))
        row["evaluation_over_plain"] = row["evaluation_ms"] / row["plain_nlml_grad_P_rows_ms"]
        _lib.check(L.ibo_set_option(b"ggp_timing", 1))
        ms, rows = np.zeros(4), []
        try:
            for k in range(1 + args.reps):
                _lib.check(L.ibo_ggp_grad_stage_ms(None, 1))
                evaluate()
                _lib.check(L.ibo_ggp_grad_stage_ms(dp(ms), 1))
                if k:
                    rows.append(ms.copy())
        finally:
            _lib.check(L.ibo_set_option(b"ggp_timing", 0))
        med = np.median(np.array(rows), axis=0)
        row["stage_ms"] = {s: float(m) for s, m in zip(STAGES, med)}
        row["contraction_GB_per_s"] = 8.0 * P * P / 2 / (med[3] * 1e-3) / 1e9
        res["rows"].append(row)
        if N == 256:
            model = GaussianProcess(GaussianKernel_ard(2.0 * hyper), X, Y, G=G, noise=NOISE, gnoise=GNOISE)
            t0 = time.perf_counter()
            out = model.learn(maxiter=30)
            res["learn"] = {"N": N, "D": D, "P": P, "wall_ms": 1e3 * (time.perf_counter() - t0), "evaluations": int(out.evaluations),
                            "iterations": int(out.nit), "start_value": float(out.start_value), "end_value": float(out.end_value),
                            "applied": bool(out.applied), "theta": [float(t) for t in np.exp(out.x)]}
    txt = json.dumps(res, indent=1)
    print(txt)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()

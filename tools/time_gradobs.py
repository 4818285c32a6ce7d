"""
Timing of a GP observed with gradients (ibo_ggp_fit, ibo_ggp_acq_sweep) at N = 256, D = 4 (P = 1280 rows) and N = 1024, D = 3
(P = 4096 rows), in one warm process: the host clock around each call, and the device time of each stage from the HIP events the
library records under ibo_set_option("ggp_timing", 1) (ibo_ggp_stage_ms; a sweep then waits after every chunk, so the wall time is
taken in separate calls without it).  Beside each, a PLAIN model of P rows (P points, values only, the same kernel): its fit
(ibo_gp_fit: wall and ibo_gp_last_fit_ms) and an ibo_acq_sweep of the same candidates (wall and its dominant kernel) -- the same
P-row factorisation and the same P^2 flops per candidate, reached through the fused sweep kernels instead of the explicit K*.
Prints one JSON object.

    python tools/time_gradobs.py [--reps 5] [--M 16384] [--out FILE]
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STAGES = ["assemble", "kstar", "vt_tri", "rows", "unused", "acquisition", "factor_invert", "alpha"]


def objective(X):
    a = 0.6 + 1.1 * np.abs(np.sin(1.0 + np.arange(X.shape[1])))
    ph = X @ a + 0.3
    return 0.5 * np.sin(ph), 0.5 * np.cos(ph)[:, None] * a[None, :]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--M", type=int, default=1 << 14)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from ibo_amd import _lib, DeviceArray
    from ibo_amd.acquisition import sweep
    from ibo_amd.gaussianprocess import GaussianProcess
    from ibo_amd.gaussianprocess.kernel import GaussianKernel_ard
    if _lib.device_count() < 1:
        raise SystemExit("no GPU: nothing to time")
    M, reps = args.M, args.reps
    res = {"M": M, "reps": reps, "configs": []}
    ms = np.zeros(len(STAGES))
    for N, D in ((256, 4), (1024, 3)):
        P = N * (D + 1)
        rs = np.random.RandomState(N + D)
        X = rs.rand(N, D)
        Y, G = objective(X)
        ell = np.linspace(.5, .8, D)
        C = rs.rand(M, D)
        # ---- the gradient model
        build = lambda: GaussianProcess(GaussianKernel_ard(ell), X, Y, noise=.1, gnoise=1e-4, G=G)
        GP = build()
        wall = []
        for r in range(reps):
            t0 = time.perf_counter()
            GP = build()
            wall.append(1e3 * (time.perf_counter() - t0))
        _lib.check(_lib.lib.ibo_set_option(b"ggp_timing", 1))
        try:
            _lib.check(_lib.lib.ibo_ggp_stage_ms(None, 1))
            for r in range(reps):
                build()
            _lib.check(_lib.lib.ibo_ggp_stage_ms(_lib.dp(ms), 1))
        finally:
            _lib.check(_lib.lib.ibo_set_option(b"ggp_timing", 0))
        fit_stage = {k: v / reps for k, v in zip(STAGES, ms.tolist()) if k in ("assemble", "factor_invert", "alpha")}
        dc = DeviceArray.from_host(C, GP._gdev.device)
        bv = ctypes.c_double(); bi = ctypes.c_int64()
        call = lambda: _lib.check(_lib.lib.ibo_ggp_acq_sweep(GP._gdev.h, M, dc.ptr, _lib.ACQ_EI, 0.01, _lib.ERF_LIBM, _lib.CLAMP_NATIVE,
                                                             float("nan"), 0, None, None, None, ctypes.byref(bv), ctypes.byref(bi)))
        call()
        swall = []
        for r in range(reps):
            t0 = time.perf_counter()
            call()
            swall.append(1e3 * (time.perf_counter() - t0))
        _lib.check(_lib.lib.ibo_set_option(b"ggp_timing", 1))
        try:
            _lib.check(_lib.lib.ibo_ggp_stage_ms(None, 1))
            for r in range(reps):
                call()
            _lib.check(_lib.lib.ibo_ggp_stage_ms(_lib.dp(ms), 1))
        finally:
            _lib.check(_lib.lib.ibo_set_option(b"ggp_timing", 0))
        sw_stage = {k: v / reps for k, v in zip(STAGES, ms.tolist()) if k in ("kstar", "vt_tri", "rows", "acquisition")}
        grad = dict(fit_wall_ms=float(np.median(wall)), fit_stage_ms=fit_stage, sweep_wall_ms=float(np.median(swall)), sweep_stage_ms=sw_stage,
                    vt_tri_tflops=float(P) * P * M / (sw_stage["vt_tri"] * 1e-3) / 1e12, best_val=bv.value, best_idx=bi.value)
        # ---- a plain model of P rows
        Xp = rs.rand(P, D)
        Yp, _ = objective(Xp)
        pbuild = lambda: GaussianProcess(GaussianKernel_ard(ell), Xp, Yp, noise=.1)
        plain = pbuild()
        pwall, pdev = [], []
        for r in range(reps):
            t0 = time.perf_counter()
            plain = pbuild()
            pwall.append(1e3 * (time.perf_counter() - t0))
            pdev.append(plain.last_fit_ms())
        dcp = DeviceArray.from_host(C, plain._dev.device)
        sweep(plain, dcp, acq='ei', xi=0.01)
        pswall, pskern = [], []
        for r in range(reps):
            t0 = time.perf_counter()
            r_ = sweep(plain, dcp, acq='ei', xi=0.01)
            pswall.append(1e3 * (time.perf_counter() - t0))
            pskern.append(r_["kernel_ms"])
        pl = dict(fit_wall_ms=float(np.median(pwall)), fit_device_ms=float(np.median(pdev)), sweep_wall_ms=float(np.median(pswall)),
                  sweep_kernel_ms=float(np.median(pskern)), sweep_kernel=r_["kernel"])
        res["configs"].append(dict(N=N, D=D, P=P, gradient=grad, plain_P_rows=pl))
        del GP, plain
    s = json.dumps(res, indent=1)
    print(s)
    if args.out:
        with open(args.out, "w") as f:
            f.write(s + "\n")


if __name__ == "__main__":
    main()

"""
Timing of the knowledge gradient (ibo_kg_sweep) at N = 1024, D = 4 with n = 64 / 256 / 1024 reference points over M = 2^16
candidates on the device, in one warm process: the host clock around each call, and the device time of each stage from the HIP
events the library records under ibo_set_option("kg_timing", 1) (ibo_kg_stage_ms; the call then waits after every chunk, so the
wall time is taken in separate calls without it).  For the two MFMA stages the rate per flop is set beside ibo_posterior_cov's
on the same model (tools/time_cov.py's figure: N^2 M + N M^2 flops over the device time of a call at M = 1024).  The NumPy
restatement (tests/kg_reference.py) on the host's CPUs is timed once at a reduced M, for context.  Prints one JSON object.

    python tools/time_kg.py [--reps 3] [--M 65536] [--numpy-M 256] [--out FILE]
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
sys.path.insert(0, os.path.join(ROOT, "tests"))

STAGES = ["reference_state", "kstar", "vt_tri", "rows", "cross", "epigraph"]


def synth(seed, N, D):
    rs = np.random.RandomState(seed)
    X = rs.rand(N, D)
    return X, np.sin(3 * X.sum(1)) + 0.01 * rs.randn(N)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--M", type=int, default=1 << 16)
    ap.add_argument("--numpy-M", type=int, default=256)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from ibo_amd import _lib, DeviceArray
    from ibo_amd.gaussianprocess import GaussianProcess
    from ibo_amd.gaussianprocess.kernel import GaussianKernel_ard
    if _lib.device_count() < 1:
        raise SystemExit("no GPU: nothing to time")
    N, D, M = 1024, 4, args.M
    X, Y = synth(3, N, D)
    ell = np.linspace(.5, .8, D)
    GP = GaussianProcess(GaussianKernel_ard(ell), X, Y, noise=.1)
    h = GP._handle()
    rs = np.random.RandomState(2)
    C = rs.rand(M, D)
    dc = DeviceArray.from_host(C, GP._dev.device)
    res = {"N": N, "D": D, "M": M, "kg": [], "numpy": []}
    # ibo_posterior_cov on the same model: time_cov.py's per-flop figure
    Mc = 1024
    Q = _lib.f64(C[:Mc]); S = np.empty((Mc, Mc))
    dev = []
    for r in range(args.reps + 2):
        g0 = _lib.gpu_time_ms()
        _lib.check(_lib.lib.ibo_posterior_cov(h, Mc, _lib.dp(Q), 1, None, _lib.dp(S)))
        dev.append(_lib.gpu_time_ms() - g0)
    cov_ms = float(np.median(dev[2:]))
    cov_flops = float(N) * N * Mc + float(N) * Mc * Mc
    res["posterior_cov"] = dict(M=Mc, device_ms=cov_ms, tflops=cov_flops / (cov_ms * 1e-3) / 1e12)
    bv = ctypes.c_double(); bi = ctypes.c_int64()
    ms = np.zeros(len(STAGES))
    for n in (64, 256, 1024):
        A = _lib.f64(np.r_[X[:n // 2], rs.rand(n - n // 2, D)])
        call = lambda: _lib.check(_lib.lib.ibo_kg_sweep(h, n, _lib.dp(A), M, dc.ptr, 1, 1e-7, 0, None, ctypes.byref(bv), ctypes.byref(bi)))
        call()
        wall = []
        for r in range(args.reps):
            t0 = time.perf_counter()
            call()
            wall.append(1e3 * (time.perf_counter() - t0))
        _lib.check(_lib.lib.ibo_set_option(b"kg_timing", 1))
        try:
            _lib.check(_lib.lib.ibo_kg_stage_ms(None, 1))
            for r in range(args.reps):
                call()
            _lib.check(_lib.lib.ibo_kg_stage_ms(_lib.dp(ms), 1))
        finally:
            _lib.check(_lib.lib.ibo_set_option(b"kg_timing", 0))
        st = dict(zip(STAGES, (ms / args.reps).tolist()))
        tri_flops = float(N) * N * M; cross_flops = 2.0 * N * n * M
        mfma_tflops = (tri_flops + cross_flops) / ((st["vt_tri"] + st["cross"]) * 1e-3) / 1e12
        res["kg"].append(dict(n=n, wall_ms=float(np.median(wall)), stage_ms=st, best_val=bv.value, best_idx=bi.value,
                              pair_steps=float(n + 1) ** 2 * M, ns_per_pair_step=st["epigraph"] * 1e6 / (float(n + 1) ** 2 * M),
                              vt_tri_tflops=tri_flops / (st["vt_tri"] * 1e-3) / 1e12, cross_tflops=cross_flops / (st["cross"] * 1e-3) / 1e12,
                              mfma_stages_tflops=mfma_tflops, mfma_stages_over_posterior_cov=mfma_tflops / res["posterior_cov"]["tflops"]))
        # the NumPy restatement at a reduced M
        import grad_reference as gr
        import kg_reference as kr
        if n == 64:
            t0 = time.perf_counter()
            ref = gr.RefGP(X, Y, .1, gr.FAM_SE, 1.0 / ell ** 2, 1.0)
            res["numpy"].append(dict(what="model (R, Cholesky, alpha)", ms=1e3 * (time.perf_counter() - t0)))
        Mn = args.numpy_M
        t0 = time.perf_counter()
        s = kr.slopes(ref, A, C[:Mn])
        t1 = time.perf_counter()
        b0 = np.maximum(1 - s["q"], 0) / np.sqrt(s["s2"])
        kg, _ = kr.compose(s["mu_ref"], s["mu"], s["s2"], s["b"], .1, True, b0=b0)
        t2 = time.perf_counter()
        vals = np.empty(Mn)
        _lib.check(_lib.lib.ibo_kg_batch(h, n, _lib.dp(A), Mn, _lib.dp(_lib.f64(C[:Mn])), 1, 1e-7, _lib.dp(vals), None, None, None, None))
        res["numpy"].append(dict(what="slopes + sorted envelope", n=n, M=Mn, slopes_ms=1e3 * (t1 - t0), envelope_ms=1e3 * (t2 - t1),
                                 max_abs_diff=float(np.max(np.abs(kg - vals))), threads=os.environ.get("OMP_NUM_THREADS", "")))
    s = json.dumps(res, indent=1)
    print(s)
    if args.out:
        with open(args.out, "w") as f:
            f.write(s + "\n")


if __name__ == "__main__":
    main()

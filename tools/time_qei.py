"""
Timing of the Monte-Carlo parallel expected improvement (ibo_qei_sweep) at N = 1024, D = 4, SE-ARD over M = 2^16 candidates on the
device with p = 0 / 3 / 7 / 15 pending points and S = 256 / 1024 / 4096 base samples, in one warm process: the host clock around each
call, and the device time of each stage from the HIP events the library records under ibo_set_option("qei_timing", 1)
(ibo_qei_stage_ms; the call then waits after every chunk, so the wall time is taken in separate calls without it).  For comparison,
in the same process: ibo_kg_sweep with 64 reference points (tools/time_kg.py's first row -- K*, V^T and the row kernel are the same
launches, the cross-covariance the same kernel with its division) and a plain EI sweep of the same array.  Prints one JSON object.

    python tools/time_qei.py [--reps 3] [--M 65536] [--out FILE]
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

QEI_STAGES = ["pending_state", "kstar", "vt_tri", "rows", "cross", "finish"]
KG_STAGES = ["reference_state", "kstar", "vt_tri", "rows", "cross", "epigraph"]


def synth(seed, N, D):
    rs = np.random.RandomState(seed)
    X = rs.rand(N, D)
    return X, np.sin(3 * X.sum(1)) + 0.01 * rs.randn(N)


def timed(_lib, call, reps, option, stage_ms, names):
    """(median wall ms, per-stage device ms) of `call`"""
    call()
    wall = []
    for r in range(reps):
        t0 = time.perf_counter()
        call()
        wall.append(1e3 * (time.perf_counter() - t0))
    ms = np.zeros(len(names))
    _lib.check(_lib.lib.ibo_set_option(option, 1))
    try:
        _lib.check(stage_ms(None, 1))
        for r in range(reps):
            call()
        _lib.check(stage_ms(_lib.dp(ms), 1))
    finally:
        _lib.check(_lib.lib.ibo_set_option(option, 0))
    return float(np.median(wall)), dict(zip(names, (ms / reps).tolist()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--M", type=int, default=1 << 16)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from ibo_amd import _lib, DeviceArray
    from ibo_amd.acquisition import baseSamples, sweep
    from ibo_amd.gaussianprocess import GaussianProcess
    from ibo_amd.gaussianprocess.kernel import GaussianKernel_ard
    if _lib.device_count() < 1:
        raise SystemExit("no GPU: nothing to time")
    N, D, M = 1024, 4, args.M
    X, Y = synth(3, N, D)
    GP = GaussianProcess(GaussianKernel_ard(np.linspace(.5, .8, D)), X, Y, noise=.1)
    h = GP._handle()
    rs = np.random.RandomState(2)
    C = rs.rand(M, D)
    dc = DeviceArray.from_host(C, GP._dev.device)
    res = {"N": N, "D": D, "M": M, "qei": []}
    bv = ctypes.c_double(); bi = ctypes.c_int64(); info = ctypes.c_int()
    # the yardsticks: the knowledge gradient with 64 reference points, and one EI sweep
    A = _lib.f64(np.r_[X[:32], rs.rand(32, D)])
    kg = lambda: _lib.check(_lib.lib.ibo_kg_sweep(h, 64, _lib.dp(A), M, dc.ptr, 1, 1e-7, 0, None, ctypes.byref(bv), ctypes.byref(bi)))
    wall, st = timed(_lib, kg, args.reps, b"kg_timing", _lib.lib.ibo_kg_stage_ms, KG_STAGES)
    res["kg_n64"] = dict(wall_ms=wall, stage_ms=st, shared_ms=st["kstar"] + st["vt_tri"] + st["rows"] + st["cross"])
    ei = lambda: sweep(GP, dc, acq='ei', xi=.01)
    ei()
    w = []
    for r in range(args.reps):
        t0 = time.perf_counter()
        ei()
        w.append(1e3 * (time.perf_counter() - t0))
    res["ei_sweep"] = dict(wall_ms=float(np.median(w)))
    for p in (0, 3, 7, 15):
        P = _lib.f64(rs.rand(max(p, 1), D)[:p])
        for S in (256, 1024, 4096):
            Z = baseSamples(p + 1, S, seed=1)
            call = lambda: _lib.check(_lib.lib.ibo_qei_sweep(h, p, _lib.dp(P) if p else None, S, _lib.dp(Z), float("nan"), .01, 1e-7, 0.0, M, dc.ptr,
                                                             0, None, None, ctypes.byref(bv), ctypes.byref(bi), ctypes.byref(info)))
            wall, st = timed(_lib, call, args.reps, b"qei_timing", _lib.lib.ibo_qei_stage_ms, QEI_STAGES)
            fma = float(S) * (p + 1) * M
            res["qei"].append(dict(p=p, S=S, wall_ms=wall, stage_ms=st, shared_ms=st["kstar"] + st["vt_tri"] + st["rows"] + st["cross"],
                                   best_val=bv.value, best_idx=bi.value, finish_fma=fma,
                                   finish_gfma_per_s=fma / (st["finish"] * 1e-3) / 1e9 if st["finish"] > 0 else None))
    s = json.dumps(res, indent=1)
    print(s)
    if args.out:
        with open(args.out, "w") as f:
            f.write(s + "\n")


if __name__ == "__main__":
    main()

"""
Timing of the sparse marginal likelihood's gradient (ibo_sgp_nlml_grad) in one warm process, SE-ARD, beside the fit at the same shape.

  shapes   N = 2^17 / m = 1024 and N = 2^20 / m = 2048, each with D = 4 and D = 16; objectives fitc and vfe (the two-operand contraction and
           the signed Gram product) and dtc (the contraction of length mp alone)
  wall     medians of the host clock around the blocking call (the fit is part of every call), beside ibo_sgp_fit alone
  stages   from a second set of calls under ibo_set_option("sgp_timing", 1) (HIP events around every stage; the option makes a call wait
           once more per stage, so the wall times are taken without it): fit, inverses, sweeps, generation, contraction, signed Gram, K~uu
           part, strip sums.  The fused kernel as TFLOP/s over its MFMA flops 2 (2 mp) mp N (dtc: 2 mp mp N) -- the epilogue's VALU work
           is not counted -- and the signed Gram product over mp^2 N useful flops (the lower tiles), beside the fit's Gram stage.

Prints one JSON object.

    python tools/time_sparse_grad.py [--reps 15] [--small] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
STAGES = ("fit", "inverses", "sweeps", "generation", "contraction", "signed_gram", "kuu_part", "strip_sums")


def median_ms(f, reps, warm=2):
    for _ in range(warm):
        f()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        f()
        t.append(time.perf_counter() - t0)
    return 1e3 * float(np.median(t))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--small", action="store_true", help="N = 2^14 / m = 256 only (a quick look)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from ibo_amd import _lib
    from ibo_amd.gaussianprocess import SparseGaussianProcess
    from ibo_amd.gaussianprocess.kernel import GaussianKernel_ard
    from ibo_amd.gaussianprocess.sparse import nlml_grad_raw
    if _lib.device_count() < 1:
        raise SystemExit("no GPU: nothing to time")
    L = _lib.lib
    rs = np.random.RandomState(5)
    res = {"clock": "wall: host (time.perf_counter around blocking calls); stages: HIP events; medians of %d warm calls" % args.reps, "rows": []}

    def stage_ms(f, reps):
        _lib.check(L.ibo_set_option(b"sgp_timing", 1))
        ms, rows = np.zeros(8), []
        try:
            for k in range(1 + reps):
                _lib.check(L.ibo_sgp_grad_stage_ms(None, 1))
                f()
                _lib.check(L.ibo_sgp_grad_stage_ms(_lib.dp(ms), 1))
                if k >= 1:
                    rows.append(ms.copy())
        finally:
            _lib.check(L.ibo_set_option(b"sgp_timing", 0))
        med = np.median(np.array(rows), axis=0)
        return {STAGES[i]: float(med[i]) for i in range(len(STAGES))}

    shapes = ((1 << 14, 256),) if args.small else ((1 << 17, 1024), (1 << 20, 2048))
    for N, m in shapes:
        for D in (4, 16):
            kern = GaussianKernel_ard([.3 * np.sqrt(D / 4.0)] * D)
            X = rs.rand(N, D)
            Y = np.sin(3 * X[:, :4].sum(1)) + .1 * rs.randn(N)
            Z = rs.rand(m, D)
            reps = args.reps if N <= (1 << 17) else max(3, args.reps // 3)
            mp = (m + 63) // 64 * 64
            box = {}

            def fit(method):
                old = box.get("g")
                box["g"] = SparseGaussianProcess(kern, X, Y, Z=Z, noise=.1, method=method)
                if old is not None:
                    old.close()
            for kind in ("fitc", "vfe", "dtc"):
                method = "fitc" if kind == "fitc" else "dtc"
                call = lambda: nlml_grad_raw(kern, X, Y, Z, .1, 1e-6, kind)
                wall = median_ms(call, reps, warm=1)
                fit_ms = median_ms(lambda: fit(method), reps, warm=1)
                st = stage_ms(call, max(3, reps // 3))
                two = kind != "dtc"
                flops = 2.0 * (2 if two else 1) * mp * mp * float(N)
                row = dict(N=N, m=m, D=D, kind=kind, grad_call_ms=wall, fit_alone_ms=fit_ms, stages_ms=st,
                           contraction_tflops=flops / (st["contraction"] * 1e-3) / 1e12)
                if two:
                    row["signed_gram_tflops_useful"] = (mp * mp * float(N)) / (st["signed_gram"] * 1e-3) / 1e12
                res["rows"].append(row)
                print(json.dumps(row), file=sys.stderr, flush=True)      # (progress: the large shapes take a minute each)
            box["g"].close()
    s = json.dumps(res, indent=1)
    print(s)
    if args.out:
        with open(args.out, "w") as f:
            f.write(s + "\n")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""One SHA-256 per case over the raw bytes of what the MODEL side of the ABI returns where tools/factor_bits.py does not reach -- through the
public ABI only, so the same file runs against any build of the library (IBO_HIP_LIB=/path/to/libibo_hip.so) and two builds compare line
for line:

    python3 tools/model_bits.py            every case

ggp-fit   ibo_ggp_fit: ibo_ggp_get_L, mu and sigma^2 of ibo_ggp_acq_batch at 64 fixed points
ggp-grad  ibo_ggp_nlml_grad: value, gradient, noise gradient
sgp       ibo_sgp_fit with ibo_sgp_nlml, and ibo_sgp_nlml_grad (value, hyper-parameter, log-noise and Z gradients): FITC, DTC, VFE
grid      ibo_nlml_grid at 3 theta-points
seq       the call sequences of tests/test_gpu_model_frames.py (model_frames_calls.py), hashed step by step
The gradient-observation cases are the sizes P = N (D + 1) at which each branch of the factorisation is taken (see CASES)."""
import ctypes
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import model_frames_calls as mf
from ibo_amd import _lib

DEFAULTS = {b"fused2_min_nb": 104, b"super_min_nb": 64}
CASES = [  # name, N, D, options, fit too: the branch it reaches
    ("P2", 1, 1, {}, True),                                         # one block column
    ("P66", 22, 2, {}, True),                                       # two block columns
    ("P300", 100, 2, {}, True),                                     # pipelined columns
    ("P1800", 600, 2, {}, False),                                   # launch_syrk3
    ("P2100", 700, 2, {}, True),                                    # single-level with pairs
    ("P2100-super", 700, 2, {b"super_min_nb": 32}, True),           # super-panels
    ("P2100-two-level", 700, 2, {b"fused2_min_nb": 33}, True),      # two-level
    ("P150-two-level", 50, 2, {b"fused2_min_nb": 3}, True),         # two-level, small
]
lib, check, dp, f64 = _lib.lib, _lib.check, _lib.dp, _lib.f64


def sha(*arrays):
    return hashlib.sha256(mf.bits(arrays)).hexdigest()


def show(name, entry, digest):
    print("%-16s %-24s %s" % (name, entry, digest), flush=True)


def ggp_case(name, N, D, fit):
    rs = np.random.RandomState(2000 + N)
    X = f64(rs.rand(N, D)); s = 3 * X.sum(1)
    Y, G = f64(np.sin(s) + .01 * rs.randn(N)), f64(3 * np.cos(s)[:, None] * np.ones(D) + .01 * rs.randn(N, D))
    Q, ell, gno, P = f64(rs.rand(64, D)), f64([.4, .6][:D]), f64([mf.GNOISE] * D), N * (D + 1)
    if fit:
        h, info = ctypes.c_void_p(), ctypes.c_int(0)
        check(lib.ibo_ggp_create(0, ctypes.byref(h)))
        check(lib.ibo_ggp_fit(h, _lib.K_SE_ARD, N, D, dp(X), dp(Y), dp(G), dp(ell), D, 1.0, mf.NOISE, dp(gno), ctypes.byref(info)))
        L, mu, s2 = np.empty((P, P)), np.empty(64), np.empty(64)
        check(lib.ibo_ggp_get_L(h, dp(L)))
        check(lib.ibo_ggp_acq_batch(h, 64, dp(Q), _lib.ACQ_NONE, 0.0, 0, 1e-8, float("nan"), dp(mu), dp(s2), None))
        check(lib.ibo_ggp_destroy(h))
        show(name, "ibo_ggp_fit", sha(L, mu, s2))
    modes, dims = (ctypes.c_int * D)(*([0] * D)), (ctypes.c_int * D)(*range(D))
    v, g, gz = ctypes.c_double(0), np.empty(D), np.empty(D + 1)
    check(lib.ibo_ggp_nlml_grad(0, _lib.K_SE_ARD, N, D, dp(X), dp(Y), dp(G), dp(ell), D, 1.0, mf.NOISE, dp(gno), D, modes, dims,
                                ctypes.byref(v), dp(g), dp(gz)))
    show(name, "ibo_ggp_nlml_grad", sha(np.array([v.value]), g, gz))


def sgp_cases():
    X, Y, _ = mf.data(300)
    m = 65
    Z = f64(X[:m] + .01)
    for kind, label in ((0, "FITC"), (1, "DTC"), (2, "VFE")):
        h, info, v = ctypes.c_void_p(), ctypes.c_int(0), ctypes.c_double(0)
        check(lib.ibo_sgp_create(0, ctypes.byref(h)))
        check(lib.ibo_sgp_fit(h, _lib.K_SE_ARD, mf.D, dp(f64(mf.THETA1)), mf.D, 1.0, mf.NOISE, 1e-6, min(kind, 1), m, dp(Z), 300, dp(X), dp(Y), None,
                              ctypes.byref(info)))
        check(lib.ibo_sgp_nlml(h, 1 if kind == 2 else 0, ctypes.byref(v)))
        check(lib.ibo_sgp_destroy(h))
        show("sgp-" + label, "ibo_sgp_fit+nlml", sha(np.array([v.value])))
        show("sgp-" + label, "ibo_sgp_nlml_grad", sha(*mf.sgp_nlml_grad(X, Y, kind=kind, m=m)))


def sequences():
    for name, entry, sizes in mf.RESIDENT:
        check(mf.trim())
        for k, (label, X, Y, G, ell) in enumerate(mf.resident_steps(*sizes)):
            show("seq-resident-%d" % (k + 1), name, sha(*entry(X, Y, G, ell)))
    X, Y, _ = mf.data(70)
    gX, gY, gG = mf.data(22, seed=9)
    check(mf.trim())
    for k, (entry, args) in enumerate([(mf.nlml_grad, (X, Y, None, mf.THETA1)), (mf.ggp_nlml_grad, (gX, gY, gG, mf.THETA1)),
                                       (mf.nlml_grad, (X, Y, None, mf.THETA2)), (mf.ggp_nlml_grad, (gX, gY, gG, mf.THETA1)),
                                       (mf.loo_grad, (X, Y, None, mf.THETA1)), (mf.ggp_nlml_grad, (gX, gY, gG, mf.THETA2))]):
        show("seq-apart-%d" % (k + 1), "ibo_" + entry.__name__, sha(*entry(*args)))
    for name in ("nlml_grad", "loo_grad", "ggp_nlml_grad", "nlml_grid", "sgp_nlml_grad"):
        Xs, Ys, Gs = mf.data(22 if name == "ggp_nlml_grad" else 70)
        for k in (1, 2):
            show("seq-trim-%d" % k, "ibo_" + name, sha(*getattr(mf, name)(Xs, Ys, Gs)))
            check(mf.trim())
    h, other = mf.Ggp(), mf.Ggp()
    Xg, Yg, Gg = mf.data(22)
    rc = h.fit(Xg, Yg, Gg, noise=-2.0)
    show("seq-tail-1", "ibo_ggp_fit", sha(np.array([rc, h.info.value, h.L()[0]], dtype=np.float64)))
    check(h.fit(Xg, Yg, Gg)); check(other.fit(Xg, Yg, Gg))
    show("seq-tail-2", "ibo_ggp_fit", sha(h.L()[1], other.L()[1]))


def main():
    if _lib.device_count() < 1:
        raise SystemExit("no GPU: nothing to hash")
    for name, N, D, opts, fit in CASES:
        try:
            for k, val in opts.items():
                check(lib.ibo_set_option(k, val))
            ggp_case(name, N, D, fit)
        finally:
            for k in opts:
                check(lib.ibo_set_option(k, DEFAULTS[k]))
    sgp_cases()
    for N in (65, 200):
        X, Y, _ = mf.data(N)
        show("N%d" % N, "ibo_nlml_grid", sha(*mf.nlml_grid(X, Y)))
    sequences()


if __name__ == "__main__":
    main()

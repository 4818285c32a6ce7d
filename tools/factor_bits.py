#!/usr/bin/env python3
"""One SHA-256 per case over the raw bytes of what the factor-and-invert entries return, through the public ABI only -- so the same file
runs against any build of the library (IBO_HIP_LIB=/path/to/libibo_hip.so) and two builds compare line for line:

    python3 tools/factor_bits.py                      every case
    python3 tools/factor_bits.py N300 N150-two-level   these cases only (the two a kernel trace is taken of)

fit / fitA   ibo_gp_fit / ibo_gp_fit_with_matrix: ibo_gp_get_L, ibo_gp_get_W, mu and sigma^2 at 64 fixed candidates
grad         ibo_nlml_grad: value, gradient;  ibo_loo_grad: value, gradient, mu_-i, sigma^2_-i
spd          ibo_spd_solve: X;  ibo_spd_inverse: the inverse
pref         one ibo_pref_newton_step (delta, R^-1 delta), then L and W as ibo_pref_finish leaves them
The cases are the smallest sizes at which each branch of the factorisation is taken (see CASES)."""
import ctypes
import hashlib
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ibo_amd import _lib

DEFAULTS = {b"fused2_min_nb": 104, b"super_min_nb": 64}
CASES = [  # name, rows, options, entries: the branch it reaches
    ("N1", 1, {}, "fit fitA grad spd"),                                              # one block column
    ("N65", 65, {}, "fit fitA grad spd pref"),                                       # fused steps, two block columns
    ("N200", 200, {}, "fit fitA grad spd pref"),                                     # chol_step8_kernel, below kPipeFrom
    ("N300", 300, {}, "fit fitA grad spd pref"),                                     # chol_pipe8_kernel<0>
    ("N800", 800, {}, "fit fitA grad spd pref"),                                     # pairs, from kPairsFrom
    ("N1800", 1800, {}, "grad"),                                                     # launch_syrk3, from kSyrk3From
    ("N2100", 2100, {}, "fit fitA grad spd pref"),                                   # single-level with pairs; spd: in place, panels of four
    ("N2100-super", 2100, {b"super_min_nb": 32}, "fit fitA grad pref"),              # super-panels
    ("N2100-two-level", 2100, {b"fused2_min_nb": 33}, "fit fitA grad pref"),         # two-level
    ("N150-two-level", 150, {b"fused2_min_nb": 3}, "fit fitA grad pref"),            # two-level, small
]
D, NOISE = 3, .05
ELL = np.array([.35, .45, .55])
I64 = ctypes.POINTER(ctypes.c_int64)
lib, check, dp = _lib.lib, _lib.check, _lib.dp


def sha(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def data(N):
    rs = np.random.RandomState(1000 + N)
    X = rs.rand(N, D)
    Y = np.sin(3 * X.sum(1)) + .01 * rs.randn(N)
    return X, Y, rs.rand(64, D)


def r_matrix(X):
    d = (X[:, None, :] - X[None, :, :]) / ELL
    return np.exp(-.5 * np.sum(d * d, axis=2)) + NOISE * np.eye(len(X))


class Handle(object):
    def __init__(self):
        self.h = ctypes.c_void_p()
        check(lib.ibo_gp_create(0, ctypes.byref(self.h)))

    def __del__(self):
        lib.ibo_gp_destroy(self.h)

    def fit(self, X, Y, A=None):
        N = len(X)
        info = ctypes.c_int(0)
        if A is None:
            check(lib.ibo_gp_fit(self.h, _lib.K_SE_ARD, N, D, dp(X), dp(Y), dp(ELL), D, 1.0, NOISE, ctypes.byref(info)))
        else:
            check(lib.ibo_gp_fit_with_matrix(self.h, _lib.K_SE_ARD, N, D, dp(X), dp(Y), dp(ELL), D, 1.0, NOISE, dp(A), ctypes.byref(info)))

    def factors(self, N):
        L, W = np.empty((N, N)), np.empty((N, N))
        check(lib.ibo_gp_get_L(self.h, dp(L))); check(lib.ibo_gp_get_W(self.h, dp(W)))
        return L, W

    def posterior(self, Q):
        mu, s2 = np.empty(len(Q)), np.empty(len(Q))
        check(lib.ibo_posterior_batch(self.h, len(Q), dp(Q), _lib.CLAMP_PY, dp(mu), dp(s2)))
        return mu, s2


def fit_case(X, Y, Q, A=None):
    g = Handle()
    g.fit(X, Y, A)
    return sha(*(g.factors(len(X)) + g.posterior(Q)))


def grad_case(X, Y):
    N = len(X)
    modes, dims = (ctypes.c_int * D)(*([0] * D)), (ctypes.c_int * D)(*range(D))      # SE-ARD: d/d log ell_d
    v, g = ctypes.c_double(0), np.empty(D)
    check(lib.ibo_nlml_grad(0, _lib.K_SE_ARD, N, D, dp(X), dp(Y), dp(ELL), D, 1.0, NOISE, D, modes, dims, ctypes.byref(v), dp(g)))
    lv, lg, mu, s2 = ctypes.c_double(0), np.empty(D), np.empty(N), np.empty(N)
    check(lib.ibo_loo_grad(0, _lib.K_SE_ARD, N, D, dp(X), dp(Y), dp(ELL), D, 1.0, NOISE, D, modes, dims, ctypes.byref(lv), dp(lg), dp(mu), dp(s2)))
    return sha(np.array([v.value]), g), sha(np.array([lv.value]), lg, mu, s2)


def spd_case(X, Y):
    N = len(X)
    A = _lib.f64(r_matrix(X))
    B = _lib.f64(np.vstack([Y, np.cos(np.arange(N))]))
    Xs, Ai, info = np.empty_like(B), np.empty((N, N)), ctypes.c_int(0)
    check(lib.ibo_spd_solve(0, N, dp(A), 2, dp(B), dp(Xs), ctypes.byref(info)))
    check(lib.ibo_spd_inverse(0, N, dp(A), dp(Ai), ctypes.byref(info)))
    return sha(Xs), sha(Ai)


def pref_case(X, Y):
    N = len(X)
    g = Handle()
    g.fit(X, Y)
    check(lib.ibo_pref_begin(g.h))
    # disjoint pairs (2 i, 2 i + 1) with weights rho_i: the Hessian's and C's four distinct entries per pair
    rs = np.random.RandomState(N)
    u = np.arange(0, N - 1, 2); v = u + 1
    rho = .2 + rs.rand(len(u))
    lin = np.ascontiguousarray(np.r_[u * N + u, v * N + v, u * N + v, v * N + u], dtype=np.int64)
    val = _lib.f64(np.r_[rho, rho, -rho, -rho])
    grad = _lib.f64(rs.randn(N))
    delta, rdelta, info = np.empty(N), np.empty(N), ctypes.c_int(0)
    check(lib.ibo_pref_newton_step(g.h, len(lin), lin.ctypes.data_as(I64), dp(val), dp(grad), dp(delta), dp(rdelta), ctypes.byref(info)))
    check(lib.ibo_pref_finish(g.h, len(lin), lin.ctypes.data_as(I64), dp(val), 1.0, ctypes.byref(info)))
    return sha(delta, rdelta), sha(*g.factors(N))


def main():
    if _lib.device_count() < 1:
        raise SystemExit("no GPU: nothing to hash")
    want = sys.argv[1:]
    for name, N, opts, entries in CASES:
        if want and name not in want:
            continue
        X, Y, Q = data(N)
        try:
            for k, val in opts.items():
                check(lib.ibo_set_option(k, val))
            out = []
            if "fit" in entries.split():
                out.append(("ibo_gp_fit", fit_case(X, Y, Q)))
            if "fitA" in entries.split():
                out.append(("ibo_gp_fit_with_matrix", fit_case(X, Y, Q, _lib.f64(r_matrix(X) + 1.0 * np.eye(N)))))
            if "grad" in entries.split():
                a, b = grad_case(X, Y)
                out += [("ibo_nlml_grad", a), ("ibo_loo_grad", b)]
            if "spd" in entries.split():
                a, b = spd_case(X, Y)
                out += [("ibo_spd_solve", a), ("ibo_spd_inverse", b)]
            if "pref" in entries.split():
                a, b = pref_case(X, Y)
                out += [("ibo_pref_newton_step", a), ("ibo_pref_finish", b)]
        finally:
            for k in opts:
                check(lib.ibo_set_option(k, DEFAULTS[k]))
        for entry, digest in out:
            print("%-16s %-24s %s" % (name, entry, digest), flush=True)


if __name__ == "__main__":
    main()

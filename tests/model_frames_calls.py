"""
The model-side entries through the raw ABI, one function each, and the call sequences that exercise what they keep between calls --
shared by tests/test_gpu_model_frames.py (which asserts) and tools/model_bits.py (which hashes, to compare two builds).
Every function returns a tuple of arrays: two results are "the same bits" when bits() of them agree.
"""
import ctypes

import numpy as np

from ibo_amd import _lib

D, NOISE, GNOISE = 2, .05, 1e-3
THETA1, THETA2 = np.array([.4, .6]), np.array([.55, .35])
lib, dp, f64 = _lib.lib, _lib.dp, _lib.f64
STAGES = {"ibo_sgp_stage_ms": 8, "ibo_sgp_grad_stage_ms": 8}      # IBO_SGP_STAGES, IBO_SGP_GRAD_STAGES (include/ibo_abi.h)
MODES, DIMS = (ctypes.c_int * D)(*([0] * D)), (ctypes.c_int * D)(*range(D))      # SE-ARD: d / d log ell_d


def bits(result):
    return b"".join(np.ascontiguousarray(a, dtype=np.float64).tobytes() for a in result)


def data(N, seed=7):
    """X, Y, G of N points from a fixed RandomState: a smooth function, its slopes, a little noise on both"""
    rs = np.random.RandomState(seed)
    X = rs.rand(N, D)
    s = 3 * X.sum(1)
    return f64(X), f64(np.sin(s) + .01 * rs.randn(N)), f64(3 * np.cos(s)[:, None] * np.ones(D) + .01 * rs.randn(N, D))


def trim():
    return lib.ibo_trim(0)


def nlml_grad(X, Y, G=None, ell=THETA1):
    v, g = ctypes.c_double(0), np.empty(D)
    _lib.check(lib.ibo_nlml_grad(0, _lib.K_SE_ARD, len(X), D, dp(X), dp(Y), dp(f64(ell)), D, 1.0, NOISE, D, MODES, DIMS, ctypes.byref(v), dp(g)))
    return np.array([v.value]), g


def loo_grad(X, Y, G=None, ell=THETA1):
    N = len(X)
    v, g, mu, s2 = ctypes.c_double(0), np.empty(D), np.empty(N), np.empty(N)
    _lib.check(lib.ibo_loo_grad(0, _lib.K_SE_ARD, N, D, dp(X), dp(Y), dp(f64(ell)), D, 1.0, NOISE, D, MODES, DIMS, ctypes.byref(v), dp(g), dp(mu), dp(s2)))
    return np.array([v.value]), g, mu, s2


def ggp_nlml_grad(X, Y, G, ell=THETA1):
    v, g, gz = ctypes.c_double(0), np.empty(D), np.empty(D + 1)
    gno = f64([GNOISE] * D)
    _lib.check(lib.ibo_ggp_nlml_grad(0, _lib.K_SE_ARD, len(X), D, dp(X), dp(Y), dp(G), dp(f64(ell)), D, 1.0, NOISE, dp(gno), D, MODES, DIMS,
                                     ctypes.byref(v), dp(g), dp(gz)))
    return np.array([v.value]), g, gz


def nlml_grid(X, Y, G=None, ell=THETA1):
    thetas = f64([ell, THETA2, [.3, .3]])
    out = np.empty(len(thetas))
    _lib.check(lib.ibo_nlml_grid(0, _lib.K_SE_ARD, len(X), D, dp(X), dp(Y), len(thetas), dp(thetas), D, None, NOISE, dp(out)))
    return (out,)


def sgp_nlml_grad(X, Y, G=None, ell=THETA1, kind=0, m=65):
    """the m inducing points are the leading observations, nudged"""
    Z = f64(X[:m] + .01)
    v, gh, gn, gZ, info = ctypes.c_double(0), np.empty(D), ctypes.c_double(0), np.empty((m, D)), ctypes.c_int(0)
    _lib.check(lib.ibo_sgp_nlml_grad(0, _lib.K_SE_ARD, D, dp(f64(ell)), D, 1.0, NOISE, 1e-6, kind, m, dp(Z), len(X), dp(X), dp(Y), D, MODES, DIMS,
                                     ctypes.byref(v), dp(gh), ctypes.byref(gn), dp(gZ), ctypes.byref(info)))
    return np.array([v.value]), gh, np.array([gn.value]), gZ


class Ggp(object):
    """an ibo_ggp handle: fit returns the status, the pivot is in .info"""
    def __init__(self):
        self.h, self.info = ctypes.c_void_p(), ctypes.c_int(0)
        _lib.check(lib.ibo_ggp_create(0, ctypes.byref(self.h)))

    def __del__(self):
        lib.ibo_ggp_destroy(self.h)

    def fit(self, X, Y, G, noise=NOISE, ell=THETA1):
        self.P = len(X) * (D + 1)
        return lib.ibo_ggp_fit(self.h, _lib.K_SE_ARD, len(X), D, dp(X), dp(Y), dp(G), dp(f64(ell)), D, 1.0, noise, dp(f64([GNOISE] * D)),
                               ctypes.byref(self.info))

    def L(self):
        out = np.empty((self.P, self.P))
        return lib.ibo_ggp_get_L(self.h, dp(out)), out

    def batch(self, Q):
        mu, s2 = np.empty(len(Q)), np.empty(len(Q))
        return lib.ibo_ggp_acq_batch(self.h, len(Q), dp(Q), _lib.ACQ_NONE, 0.0, 0, 1e-8, float("nan"), dp(mu), dp(s2), None), mu, s2


def resident_steps(n, n_lead, n_big):
    """The seven calls that walk an entry's resident data through every branch of "upload if the content differs": (label, X, Y, G, ell).
    n_lead < n rows pad to the same frame as n rows, so that the mirror of step 4 is as long as step 5 needs and stale behind the data."""
    X, Y, G = data(n_big)
    X2, Y2, G2 = data(n, seed=8)
    return [("data", X[:n], Y[:n], G[:n], THETA1),
            ("another theta", X[:n], Y[:n], G[:n], THETA2),
            ("changed Y", X[:n], Y2, G2, THETA2),
            ("changed X", X2, Y2, G2, THETA2),
            ("leading %d rows" % n_lead, X2[:n_lead], Y2[:n_lead], G2[:n_lead], THETA2),
            ("%d rows" % n_big, X, Y, G, THETA1),
            ("%d rows again" % n, X[:n], Y[:n], G[:n], THETA1)]


RESIDENT = [("ibo_nlml_grad", nlml_grad, (70, 65, 130)), ("ibo_loo_grad", loo_grad, (70, 65, 130)), ("ibo_ggp_nlml_grad", ggp_nlml_grad, (22, 20, 44))]

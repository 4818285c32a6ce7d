"""
Knowledge gradient (Frazier, Powell and Dayanik 2009; Scott, Frazier and Powell 2011): the expected rise of the best posterior
mean over a reference set A after one more, noisy, observation at x -- the acquisition for models whose observations carry
noise, where max(Y) is itself a noisy number and EI / PI / UCB value nothing a measurement teaches about the rest of the domain.
The reference has nothing like it.

    KnowledgeGradient(GP, ref_points, with_self=True)     .values(X) .f(x) .negf(x) .slopes(X) -> (mu_ref, mu, s2, b)
    sweepKG(GP, candidates, ref_points, with_self=True, values=False) -> (best_val, best_idx[, values])
    maximizeKG(GP, bounds, ref_points=None, n_ref=256, ...) -> (opt, optx)       DIRECT on the GPU objective
    referenceSet(GP, bounds, n, seed)                     the observed points, topped up with a Latin hypercube

With mu_a the posterior mean at a reference point a and sigma_x the (clipped) predictive deviation at x, observing x moves mu_a
by b_a(x) Z, b_a(x) = Sigma(a, x) / sigma_x, Z standard normal, and

    KG(x) = E_Z[max_i (mu_i + b_i(x) Z)] - max_i mu_i  >= 0

over the reference lines and, with with_self, the candidate's own (mu_x, Sigma(x, x) / sigma_x).  Conventions of the Python classes
everywhere: the kernel's own k* signal variance, variance clamp [1e-7, 10], libm erf.  A point's value is the same bits from
every entry.  At most 1024 reference points.  No gradients with respect to x and no exclusion balls.

Everything is computed by libibo_hip (ibo_kg_sweep, ibo_kg_batch, ibo_kg_direct_max); it works on a PrefGaussianProcess as on a
GaussianProcess -- but not while an augmented factor is in force (addObservationPoint): ValueError.  Points of another width than the
model's D are refused (ValueError); a 1-D sequence is one point.
"""
import ctypes
import functools

import numpy as np

from .. import _lib
from ..utils.latinhypercube import lhcSample
from . import _args

MAX_REF = 1024          # IBO_KG_MAX_REF
_NOUN = "knowledge gradient"
_points = functools.partial(_args._points, noun=_NOUN)


def _ref(GP, ref_points):
    A = _points(GP, ref_points, "ref_points")
    if len(A) > MAX_REF:
        raise ValueError("between 1 and %d reference points" % MAX_REF)
    return A


def referenceSet(GP, bounds, n, seed=0):
    """(n, D) reference points for the knowledge gradient: the model's observed X -- the newest first, and only the newest n if
    there are more -- topped up to n with lhcSample(bounds, n - len(X), seed)."""
    n = int(n)
    if not 1 <= n <= MAX_REF:
        raise ValueError("between 1 and %d reference points" % MAX_REF)
    X = np.atleast_2d(np.asarray(GP.X, dtype=float))[::-1][:n] if len(GP.X) else np.empty((0, len(bounds)))
    if len(X) < n:
        X = np.r_[X.reshape(-1, len(bounds)), np.vstack(lhcSample(bounds, n - len(X), seed=seed))]
    return _lib.f64(X)


class KnowledgeGradient(object):
    """KG(x) against the reference points `ref_points` ((n, D), n <= 1024); with_self: the candidate's own line takes part"""

    def __init__(self, GP, ref_points, with_self=True, **kwargs):
        self.GP = GP
        self.ref = _ref(GP, ref_points)
        self.with_self = bool(with_self)

    def _call(self, X, slopes):
        Q = _points(self.GP, X, "X")
        M, n = len(Q), len(self.ref)
        self.GP._push_prior()
        kg = np.empty(M)
        out = (np.empty(n), np.empty(M), np.empty(M), np.empty((M, n))) if slopes else None
        _lib.check(_lib.lib.ibo_kg_batch(self.GP._handle(), n, _lib.dp(self.ref), M, _lib.dp(Q), int(self.with_self), _lib.CLAMP_PY,
                                         _lib.dp(kg), *([_lib.dp(o) for o in out] if slopes else [None] * 4)))
        return out if slopes else kg

    def values(self, X):
        """the value at many points at once"""
        return self._call(X, False)

    def slopes(self, X):
        """(mu_ref (n,), mu (M,), s2 (M,), b (M, n)): the reference means, the candidates' posterior (s2 clipped) and the change
        of each reference mean per standard deviation of an observation at each candidate"""
        return self._call(X, True)

    def f(self, x):
        return self._call(x, False)[0]

    def negf(self, x):
        return -self.f(x)


def sweepKG(GP, candidates, ref_points, with_self=True, values=False, index_base=0):
    """The knowledge gradient over a whole candidate array and its arg-max (ibo_kg_sweep): candidates an (M, D) ndarray (uploaded)
    or a _lib.DeviceArray already in HBM.  Returns (best_val, best_idx) or, with values=True, (best_val, best_idx, values (M,));
    the first maximiser wins ties, index_base is added to the index."""
    A = _ref(GP, ref_points)
    cand, _ = _args._candidates(GP, candidates, A.shape[1], _NOUN)
    M = cand.shape[0]
    GP._push_prior()
    out = _lib.DeviceArray((M,), GP._dev.device) if values else None
    bv = ctypes.c_double(); bi = ctypes.c_int64()
    _lib.check(_lib.lib.ibo_kg_sweep(GP._handle(), len(A), _lib.dp(A), M, cand.ptr, int(bool(with_self)), _lib.CLAMP_PY, int(index_base),
                                     out.ptr if values else None, ctypes.byref(bv), ctypes.byref(bi)))
    return (bv.value, bi.value, out.to_host()) if values else (bv.value, bi.value)


def maximizeKG(GP, bounds, ref_points=None, n_ref=256, seed=0, maxiter=50, maxtime=30, maxsample=10000, compat=False,
               with_self=True):
    """Maximise the knowledge gradient over the box `bounds` with DIRECT on the GPU objective (ibo_kg_direct_max) -> (opt, optx).
    ref_points=None: referenceSet(GP, bounds, n_ref, seed).  opt is KnowledgeGradient(GP, ref_points, with_self).f(optx), bit for bit."""
    A = _ref(GP, referenceSet(GP, bounds, n_ref, seed) if ref_points is None else ref_points)
    lb, ub, D = _args._bounds(bounds, A.shape[1])
    GP._push_prior()
    opt = ctypes.c_double(); optx = np.empty(D); ns = ctypes.c_int64()
    _lib.check(_lib.lib.ibo_kg_direct_max(GP._handle(), len(A), _lib.dp(A), D, _lib.dp(lb), _lib.dp(ub), int(bool(with_self)),
                                          _lib.CLAMP_PY, int(maxiter), int(maxtime), int(maxsample), 1 if compat else 0,
                                          ctypes.byref(opt), _lib.dp(optx), ctypes.byref(ns)))
    return opt.value, optx

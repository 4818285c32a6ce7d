"""
Parallel expected improvement (Ginsbourger, Le Riche and Carraro 2010; the Monte-Carlo form with fixed base samples of Wilson,
Hutter and Deisenroth 2018): the value of a BATCH -- q points evaluated or shown together -- and of a candidate beside points whose
evaluations are still pending.  The reference has nothing like it.

    baseSamples(q, n_samples=512, seed=0, antithetic=True)  -> (S, q) standard normal draws
    ParallelEI(GP, pending=None, n_samples=512, seed=0, xi=0.0, jitter=0.0, Z=None)
                                            .values(X) .f(x) .negf(x) .base .pieces(X) -> (mu_pend, S_pend, mu, s2, c)
    sweepQEI(GP, candidates, pending=None, ..., values=False, index_base=0) -> (best_val, best_idx[, values])
    maximizeQEI(GP, bounds, pending=None, ...) -> (opt, optx)                  DIRECT on the GPU objective
    jointQEI(GP, Xq, ...)                   the value of a whole batch: its last point the candidate, the others pending
    proposeBatch(GP, bounds=None, candidates=None, q=4, pending=None, ...) -> (Xq, joint_value)     q greedy rounds

With y the joint predictive distribution (observation noise included) at the pending points P and the candidate x, and
t = max(Y) + xi,

    qEI(x | P) = E[max(max(y(x), max_j y(p_j)) - t, 0)]  ~  (1/S) sum_s max(max(f_s, g_s) - t, 0)

where (g_s, f_s) are the draws mu + L z_s of the (p + 1) joint normal for the rows z_s of the base samples Z: column i of Z belongs to
pending point i, the next column to the candidate.  `base` is the pending set's own value, (1/S) sum_s max(g_s - t, 0): every value is
>= base, exactly.  Conventions of the Python classes everywhere: the kernel's own k* signal variance, variance clamp [1e-7, 10].  A
point's value is the same bits from every entry.  At most 15 pending points and 4096 samples.  No gradients with respect to x and no
exclusion balls.

Everything is computed by libibo_hip (ibo_qei_sweep, ibo_qei_batch, ibo_qei_direct_max); it works on a PrefGaussianProcess as on a
GaussianProcess -- but not while an augmented factor is in force (addObservationPoint): ValueError.  Points of another width than the
model's D are refused (ValueError); a 1-D sequence is one point.
"""
import ctypes
import functools

import numpy as np

from .. import _lib
from . import _args

MAX_PENDING = 15        # IBO_QEI_MAX_PENDING
MAX_SAMPLES = 4096      # IBO_QEI_MAX_SAMPLES
_NOUN = "parallel expected improvement"
_points = functools.partial(_args._points, noun=_NOUN)


def baseSamples(q, n_samples=512, seed=0, antithetic=True):
    """(n_samples, q) standard normal draws from numpy's RandomState(seed); antithetic: the second half is the negated first half
    (n_samples even)"""
    q = int(q); S = int(n_samples)
    if q < 1 or not 1 <= S <= MAX_SAMPLES:
        raise ValueError("q >= 1 and between 1 and %d samples" % MAX_SAMPLES)
    rs = np.random.RandomState(seed)
    if not antithetic:
        return _lib.f64(rs.randn(S, q))
    if S % 2:
        raise ValueError("antithetic draws come in pairs: n_samples must be even")
    Z = rs.randn(S // 2, q)
    return _lib.f64(np.r_[Z, -Z])


def _pending(GP, pending):
    """(p, D) pending points, p <= 15; None or an empty sequence: none"""
    D = np.asarray(GP.X).shape[1] if len(GP.X) else 0
    if pending is None or len(pending) == 0:
        _points(GP, np.zeros((1, D)), "pending")          # (an empty model or an augmented factor is refused here too)
        return np.empty((0, D))
    P = _points(GP, pending, "pending")
    if len(P) > MAX_PENDING:
        raise ValueError("at most %d pending points" % MAX_PENDING)
    return P


def _samples(P, n_samples, seed, Z):
    """the (S, p + 1) base samples of a call: the first p + 1 columns of a given Z, or fresh ones"""
    w = len(P) + 1
    if Z is None:
        return baseSamples(w, n_samples, seed)
    Z = np.asarray(Z, dtype=float)
    if Z.ndim != 2 or Z.shape[1] < w or not 1 <= len(Z) <= MAX_SAMPLES:
        raise ValueError("Z must be (S, >= %d) with 1 <= S <= %d, got shape %s" % (w, MAX_SAMPLES, Z.shape))
    return _lib.f64(Z[:, :w])


class ParallelEI(object):
    """qEI(x | pending) with fixed base samples: Z (S, >= p + 1) if given (its first p + 1 columns), else baseSamples(p + 1, n_samples, seed)"""

    def __init__(self, GP, pending=None, n_samples=512, seed=0, xi=0.0, jitter=0.0, Z=None, **kwargs):
        self.GP = GP
        self.pending = _pending(GP, pending)
        self.Z = _samples(self.pending, n_samples, seed, Z)
        self.xi = float(xi)
        self.jitter = float(jitter)

    def _head(self):
        """the arguments every entry begins with"""
        p = len(self.pending)
        return (self.GP._handle(), p, _lib.dp(self.pending) if p else None, len(self.Z), _lib.dp(self.Z), float("nan"), self.xi,
                _lib.CLAMP_PY, self.jitter)

    def _call(self, X, pieces):
        Q = _points(self.GP, X, "X")
        M, p = len(Q), len(self.pending)
        self.GP._push_prior()
        v = np.empty(M); base = ctypes.c_double(); info = ctypes.c_int()
        out = (np.empty(p), np.empty((p, p)), np.empty(M), np.empty(M), np.empty((M, p))) if pieces else None
        _lib.check(_lib.lib.ibo_qei_batch(*(self._head() + (M, _lib.dp(Q), _lib.dp(v), ctypes.byref(base)) +
                                            (tuple(_lib.dp(o) for o in out) if pieces else (None,) * 5) + (ctypes.byref(info),))))
        return out if pieces else v

    def values(self, X):
        """the value at many points at once"""
        return self._call(X, False)

    def pieces(self, X):
        """(mu_pend (p,), S_pend (p, p), mu (M,), s2 (M,), c (M, p)): what the values are made of -- the pending points' means and joint
        covariance (jitter on its diagonal), the candidates' posterior (s2 clipped) and their covariances with the pending points"""
        return self._call(X, True)

    @property
    def base(self):
        """the pending set's own value (0 without pending points)"""
        self.GP._push_prior()
        base = ctypes.c_double(); info = ctypes.c_int()
        x = _lib.f64(np.asarray(self.GP.X, dtype=float)[:1])
        _lib.check(_lib.lib.ibo_qei_batch(*(self._head() + (1, _lib.dp(x), None, ctypes.byref(base)) + (None,) * 5 + (ctypes.byref(info),))))
        return base.value

    def f(self, x):
        return self._call(x, False)[0]

    def negf(self, x):
        return -self.f(x)


def sweepQEI(GP, candidates, pending=None, n_samples=512, seed=0, xi=0.0, jitter=0.0, Z=None, values=False, index_base=0):
    """qEI(. | pending) over a whole candidate array and its arg-max (ibo_qei_sweep): candidates an (M, D) ndarray (uploaded) or a
    _lib.DeviceArray already in HBM.  Returns (best_val, best_idx) or, with values=True, (best_val, best_idx, values (M,)); the first
    maximiser wins ties, index_base is added to the index."""
    acq = ParallelEI(GP, pending, n_samples, seed, xi, jitter, Z)
    cand, _ = _args._candidates(GP, candidates, acq.pending.shape[1], _NOUN)
    M = cand.shape[0]
    GP._push_prior()
    out = _lib.DeviceArray((M,), GP._dev.device) if values else None
    bv = ctypes.c_double(); bi = ctypes.c_int64(); info = ctypes.c_int()
    _lib.check(_lib.lib.ibo_qei_sweep(*(acq._head() + (M, cand.ptr, int(index_base), out.ptr if values else None, None,
                                                       ctypes.byref(bv), ctypes.byref(bi), ctypes.byref(info)))))
    return (bv.value, bi.value, out.to_host()) if values else (bv.value, bi.value)


def maximizeQEI(GP, bounds, pending=None, n_samples=512, seed=0, xi=0.0, jitter=0.0, Z=None, maxiter=50, maxtime=30, maxsample=10000,
                compat=False):
    """Maximise qEI(. | pending) over the box `bounds` with DIRECT on the GPU objective (ibo_qei_direct_max) -> (opt, optx).
    opt is ParallelEI(GP, pending, ...).f(optx), bit for bit."""
    acq = ParallelEI(GP, pending, n_samples, seed, xi, jitter, Z)
    lb, ub, D = _args._bounds(bounds, acq.pending.shape[1])
    GP._push_prior()
    opt = ctypes.c_double(); optx = np.empty(D); ns = ctypes.c_int64(); info = ctypes.c_int()
    _lib.check(_lib.lib.ibo_qei_direct_max(*(acq._head() + (D, _lib.dp(lb), _lib.dp(ub), int(maxiter), int(maxtime), int(maxsample),
                                                            1 if compat else 0, ctypes.byref(opt), _lib.dp(optx), ctypes.byref(ns),
                                                            ctypes.byref(info)))))
    return opt.value, optx


def jointQEI(GP, Xq, n_samples=512, seed=0, xi=0.0, jitter=0.0, Z=None):
    """The parallel expected improvement of the whole batch Xq ((q, D), q <= 16): its last point taken as the candidate, the others as
    pending; point i owns column i of Z."""
    Xq = _points(GP, Xq, "Xq")
    return ParallelEI(GP, Xq[:-1], n_samples, seed, xi, jitter, Z).f(Xq[-1])


def proposeBatch(GP, bounds=None, candidates=None, q=4, pending=None, n_samples=512, seed=0, xi=0.0, jitter=0.0, Z=None,
                 maxiter=50, maxtime=30, maxsample=10000, compat=False):
    """A batch of q points built greedily -> (Xq (q, D), joint_value).  Each round maximises qEI(. | pending so far) -- DIRECT over
    `bounds`, or a sweep over `candidates` (an ndarray or a DeviceArray; exactly one of the two is given) -- and its winner joins the
    pending set.  ONE Z of width len(pending) + q serves every round: pending point i always owns column i and the candidate of a round
    the next one, so a point keeps its column when it turns from candidate into pending point, and joint_value -- the last round's
    winning value -- is jointQEI of pending + Xq under that Z, bit for bit.  len(pending) + q <= 16."""
    if (bounds is None) == (candidates is None):
        raise ValueError("give bounds (DIRECT) or candidates (a sweep), one of the two")
    P = _pending(GP, pending)
    q = int(q)
    if q < 1 or len(P) + q - 1 > MAX_PENDING:
        raise ValueError("q >= 1 and at most %d points, pending ones included" % (MAX_PENDING + 1))
    w = len(P) + q
    if Z is None:
        Z = baseSamples(w, n_samples, seed)
    Z = np.asarray(Z, dtype=float)
    if Z.ndim != 2 or Z.shape[1] < w:
        raise ValueError("Z must be (S, >= %d), got shape %s" % (w, Z.shape))
    cand, host = (None, None) if candidates is None else _args._candidates(GP, candidates, P.shape[1], _NOUN)
    Xq = []
    value = 0.0
    for _ in range(q):
        if cand is None:
            value, x = maximizeQEI(GP, bounds, P, xi=xi, jitter=jitter, Z=Z, maxiter=maxiter, maxtime=maxtime, maxsample=maxsample,
                                   compat=compat)
        else:
            value, i = sweepQEI(GP, cand, P, xi=xi, jitter=jitter, Z=Z)
            if i < 0:
                raise ValueError("no candidate has a value that is a number")
            x = host[i] if host is not None else cand.view_rows(i, i + 1).to_host()[0]
        Xq.append(np.array(x, dtype=float))
        P = np.r_[P, [Xq[-1]]]
    return np.array(Xq), value

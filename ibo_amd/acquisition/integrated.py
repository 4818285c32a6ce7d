"""
Acquisitions integrated over the kernel's hyper-parameters (Snoek, Larochelle & Adams 2012): the weighted sum of EI / PI / UCB over the
members of a gaussianprocess.ensemble.GaussianProcessEnsemble -- the same data under samples of theta -- instead of one model's
point estimate.  The reference has nothing like it.

    IntegratedEI / IntegratedPI(ensemble, xi=.01, ymax=None)     IntegratedUCB(ensemble, NA, delta=0.1, scale=0.2)
        .f(x) .negf(x) .values(X) .gradient(X) .negf_grad(x)
    sweepIntegrated(ensemble, candidates, acq='ei'|'pi'|'ucb', ...) -> dict(best_val, best_idx, [val], [mean], [var])
    maximizeIntegratedEI / maximizeIntegratedPI / maximizeIntegratedUCB(ensemble, bounds, ..., polish=False) -> (opt, optx)

With (mu_s, s2_s) the posterior of member s at x, w_s the ensemble's weights (they sum to 1) and a the acquisition:

    val(x) = sum_s w_s a(mu_s, sqrt(s2_s))          every member against the same incumbent, max(ensemble.Y) unless ymax= is given

The classes have the Python classes' semantics (NR erf, clamp [1e-7, 10], the kernels' own k* variance), the sweep with native=True and
the maximisers libego's (libm erf, clamp [1e-8, 10], libego's k* variance on every member), as EI / sweep / maximizeEI have.
Everything is computed by libibo_hip (ibo_iacq_sweep, ibo_iacq_batch, ibo_iacq_grad_batch, ibo_iacq_direct_max).
"""
import ctypes

import numpy as np

from .. import _lib
from . import _args
from ._args import _kstar_native

_IACQ = {'ei': _lib.ACQ_EI, 'pi': _lib.ACQ_PI, 'ucb': _lib.ACQ_UCB}
_NOUN = "integrated acquisition"


def _ensemble(E, what):
    """refuse anything but an ensemble with data"""
    if not hasattr(E, "members") or not hasattr(E, "_pack"):
        raise TypeError("%s takes a GaussianProcessEnsemble, not %s" % (what, type(E).__name__))
    if len(E.X) == 0:
        raise ValueError("model has no data")
    return np.asarray(E.X).shape[1]


def _ymax(E, ymax):
    return float(np.max(E.Y)) if ymax is None else float(ymax)


class _Integrated(_args._HostPointAcquisition):
    """the host-point classes over the subclass's _spec() -> (acq code, parm)"""

    def _call(self, X, grad):
        E = self.GP
        D = _ensemble(E, type(self).__name__)
        Q = _lib.f64(np.atleast_2d(np.asarray(X, dtype=float)))
        if Q.ndim != 2 or Q.shape[1] != D:
            raise ValueError("X must be (M, %d) points, got shape %s" % (D, Q.shape))
        M = len(Q)
        code, parm = self._spec()
        gp, S, w = E._pack()
        lead = (gp, S, w, M, _lib.dp(Q), code, float(parm), _lib.ERF_NR, _lib.CLAMP_PY, self.ymax)
        val = np.empty(M)
        if not grad:
            _lib.check(_lib.lib.ibo_iacq_batch(*(lead + (_lib.dp(val), None, None))))
            return val
        g = np.empty((M, D))
        _lib.check(_lib.lib.ibo_iacq_grad_batch(*(lead + (_lib.dp(val), _lib.dp(g)))))
        return val, g


class IntegratedEI(_Integrated):
    """expected improvement over ymax (None: max(ensemble.Y)) averaged over the ensemble's members"""

    def __init__(self, ensemble, xi=.01, ymax=None, **kwargs):
        _ensemble(ensemble, "IntegratedEI")
        self.GP = ensemble
        self.xi = xi
        self.ymax = _ymax(ensemble, ymax)

    def _spec(self):
        return _lib.ACQ_EI, self.xi


class IntegratedPI(_Integrated):
    """probability of improvement over ymax + xi averaged over the ensemble's members"""

    def __init__(self, ensemble, xi=.01, ymax=None, **kwargs):
        _ensemble(ensemble, "IntegratedPI")
        self.GP = ensemble
        self.xi = xi
        self.ymax = _ymax(ensemble, ymax)

    def _spec(self):
        return _lib.ACQ_PI, self.xi


class IntegratedUCB(_Integrated):
    """the UCB class's upper confidence bound (its sqrt(scale * sBeta) multiplier) averaged over the ensemble's members"""

    def __init__(self, ensemble, NA, delta=0.1, scale=0.2, **kwargs):
        _ensemble(ensemble, "IntegratedUCB")
        self.GP = ensemble
        self.scale = scale
        t = len(ensemble.Y) + 1
        self.sBeta = np.sqrt(2.0 * np.log(t ** (NA // 2 + 2) * np.pi ** 2 / (3.0 * delta)))
        self.ymax = _ymax(ensemble, None)            # (UCB takes no incumbent; the entries are handed one all the same)

    def _spec(self):
        return _lib.ACQ_UCB, np.sqrt(self.scale * self.sBeta)


def _parm(E, acq, nd, native, xi, delta, scale):
    """xi for EI and PI; for UCB in nd dimensions the sigma multiplier of the native path or, native=False, the UCB class's"""
    if acq not in _IACQ:
        raise NotImplementedError('unknown acquisition function %s' % acq)
    if acq != 'ucb':
        return float(xi)
    t = len(E.Y) + 1
    beta = 2.0 * np.log(t ** (nd // 2 + 2) * np.pi ** 2 / (3.0 * delta))
    return float(np.sqrt(scale * beta)) if native else float(np.sqrt(scale * np.sqrt(beta)))


def sweepIntegrated(ensemble, candidates, acq='ei', xi=0.01, delta=0.1, scale=0.2, native=True, ymax=None, exclude=None,
                    exclude_radius=0.5, index_base=0, outputs=()):
    """Evaluate an integrated acquisition over a whole candidate array and return its arg-max (ibo_iacq_sweep).

    candidates   (M, D) ndarray (uploaded) or a _lib.DeviceArray already in HBM
    acq          'ei', 'pi' or 'ucb'; xi, or delta and scale, as sweep() takes them
    native=True  what it means in sweep(): libm erf, variance clamp [1e-8, 10] and libego's k* signal variance -- on every member,
                 the Python values restored afterwards; native=False: NR erf, clamp [1e-7, 10]
    ymax         the incumbent of every member; None: max(ensemble.Y)
    exclude      points whose exclude_radius-ball is left out of the arg-max (the gallery's rule); index_base is added to
                 the reported index
    outputs      any of 'val', 'mean', 'var': per-candidate arrays to return (host ndarrays) -- the value, the mixture's mean and variance
    Returns dict(best_val, best_idx, [val], [mean], [var]).  NaN values and excluded candidates never win, the first maximiser wins
    ties, best_idx = -1 when everything is excluded.
    """
    D = _ensemble(ensemble, "sweepIntegrated")
    for k in outputs:
        if k not in ('val', 'mean', 'var'):
            raise ValueError("unknown output %r" % (k,))
    first = ensemble.members[0]
    first._handle()
    cand, _ = _args._candidates(first, candidates, D, _NOUN)
    M = cand.shape[0]
    parm = _parm(ensemble, acq, D, native, xi, delta, scale)
    gp, S, w = ensemble._pack()
    outs = {k: _lib.DeviceArray((M,), first._dev.device) for k in outputs}
    ex = None if exclude is None or len(exclude) == 0 else _lib.f64(np.atleast_2d(exclude))
    bv = ctypes.c_double(); bi = ctypes.c_int64()
    with _kstar_native(ensemble.members, native):
        _lib.check(_lib.lib.ibo_iacq_sweep(
            gp, S, w, M, cand.ptr, _IACQ[acq], parm, _lib.ERF_LIBM if native else _lib.ERF_NR,
            _lib.CLAMP_NATIVE if native else _lib.CLAMP_PY, _ymax(ensemble, ymax), 0 if ex is None else len(ex),
            None if ex is None else _lib.dp(ex), float(exclude_radius), int(index_base),
            outs["val"].ptr if "val" in outs else None, outs["mean"].ptr if "mean" in outs else None,
            outs["var"].ptr if "var" in outs else None, ctypes.byref(bv), ctypes.byref(bi)))
    res = dict(best_val=bv.value, best_idx=bi.value)
    for k, v in outs.items():
        res[k] = v.to_host()
    return res


def _maximize(ensemble, bounds, acq, xi, delta, scale, maxiter, maxtime, maxsample, polish, ymax, compat):
    D_model = _ensemble(ensemble, "maximizeIntegrated%s" % acq.upper())
    lb, ub, D = _args._bounds(bounds, D_model)
    parm = _parm(ensemble, acq, D, True, xi, delta, scale)
    gp, S, w = ensemble._pack()
    lead = (gp, S, w)
    tail = (_IACQ[acq], parm, _lib.ERF_LIBM, _lib.CLAMP_NATIVE, _ymax(ensemble, ymax))
    opt = ctypes.c_double(); optx = np.empty(D); ns = ctypes.c_int64()
    with _kstar_native(ensemble.members):
        _lib.check(_lib.lib.ibo_iacq_direct_max(*(lead + (D, _lib.dp(lb), _lib.dp(ub)) + tail + (
            int(maxiter), int(maxtime), int(maxsample), 1 if compat else 0, ctypes.byref(opt), _lib.dp(optx), ctypes.byref(ns)))))
        best, bestx = opt.value, optx
        if polish:
            v, g = np.empty(1), np.empty((1, D))           # the polish step on the objective DIRECT maximised

            def fg(x):
                q = _lib.f64(x.reshape(1, D))
                _lib.check(_lib.lib.ibo_iacq_grad_batch(*(lead + (1, _lib.dp(q)) + tail + (_lib.dp(v), _lib.dp(g)))))
                return -v[0], -g[0].copy()

            def value_at(x):
                _lib.check(_lib.lib.ibo_iacq_batch(*(lead + (1, _lib.dp(x)) + tail + (_lib.dp(v), None, None))))
                return v[0]

            best, bestx = _args._polish_step(fg, value_at, lb, ub, best, bestx)
    return best, bestx


def maximizeIntegratedEI(ensemble, bounds, xi=0.01, maxiter=50, maxtime=30, maxsample=10000, polish=False, ymax=None, compat=True):
    """Maximise integrated expected improvement over the box `bounds` with DIRECT on the GPU objective (ibo_iacq_direct_max; libego
    semantics as maximizeEI: libm erf, clamp [1e-8, 10], libego's k* variance on every member) -> (opt, optx).  ymax=None:
    max(ensemble.Y).  polish=True: a bounded L-BFGS-B finish from DIRECT's point on ibo_iacq_grad_batch, at most POLISH_MAXITER
    iterations, kept only when strictly better.  compat: DIRECT's dimension-0 stall switch, as cdirectGP's."""
    return _maximize(ensemble, bounds, 'ei', xi, None, None, maxiter, maxtime, maxsample, polish, ymax, compat)


def maximizeIntegratedPI(ensemble, bounds, xi=0.01, maxiter=50, maxtime=30, maxsample=10000, polish=False, ymax=None, compat=True):
    """Maximise the integrated probability of improvement; everything else as maximizeIntegratedEI."""
    return _maximize(ensemble, bounds, 'pi', xi, None, None, maxiter, maxtime, maxsample, polish, ymax, compat)


def maximizeIntegratedUCB(ensemble, bounds, delta=0.1, scale=0.2, maxiter=50, maxtime=30, maxsample=10000, polish=False, compat=True):
    """Maximise the integrated upper confidence bound (the native path's sigma multiplier, as maximizeUCB); everything else as
    maximizeIntegratedEI."""
    return _maximize(ensemble, bounds, 'ucb', None, delta, scale, maxiter, maxtime, maxsample, polish, None, compat)

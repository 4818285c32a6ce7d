"""What the acquisition modules share: the checks of their arguments (points, candidate arrays, bounds), the switch to libego's k* signal
variance, the methods of a host-point acquisition class, and the polish step of the maximisers."""
import numpy as np

from .. import _lib


def _no_gradient(GP, what):
    """refuse `what` on a model observed with gradients (GaussianProcess(G=)) and on a sparse model (SparseGaussianProcess); anything
    without a G attribute passes"""
    if getattr(GP, "G", None) is not None or getattr(GP, "_kind", "gp") != "gp":
        GP._no_gradient(what)


def _points(GP, P, what, noun):
    """an (M, D) float64 matrix of points of the model's dimension; a 1-D sequence is ONE point (D coordinates), as everywhere else.
    noun: what the refusal of an augmented factor calls the acquisition"""
    if len(GP.X) == 0:
        raise ValueError("model has no data")
    _no_gradient(GP, "the %s" % noun)
    if getattr(GP, "_augdev", None) is not None:
        raise ValueError("the %s is not defined on an augmented factor (addObservationPoint): its covariances would "
                         "come from one factor and its means from another" % noun)
    P = _lib.f64(np.atleast_2d(np.asarray(P, dtype=float)))
    D = np.asarray(GP.X).shape[1]
    if P.ndim != 2 or P.shape[1] != D or len(P) < 1:
        raise ValueError("%s must be (M, %d) points, got shape %s" % (what, D, P.shape))
    return P


def _candidates(GP, candidates, D, noun):
    """(the candidates in HBM, the host's copy or None): an ndarray is checked as _points and uploaded, a _lib.DeviceArray is taken as
    it is; either must be D wide"""
    host = None if isinstance(candidates, _lib.DeviceArray) else _points(GP, candidates, "candidates", noun)
    cand = candidates if host is None else _lib.DeviceArray.from_host(host, GP._dev.device)
    if len(cand.shape) != 2 or cand.shape[1] != D:
        raise ValueError("candidates must be (M, %d) points, got shape %s" % (D, cand.shape))
    return cand, host


def _bounds(bounds, D_model):
    """(lb, ub, D) of a box of the model's dimension"""
    lb = _lib.f64([b[0] for b in bounds]); ub = _lib.f64([b[1] for b in bounds])
    if len(lb) != D_model:
        raise ValueError("bounds have %d dimensions, the model has %d" % (len(lb), D_model))
    return lb, ub, len(lb)


class _kstar_native(object):
    """libego's k* signal variance on every (plain) model involved, the Python one restored on exit; on=False: nothing"""

    def __init__(self, models, on=True):
        self.models = list(models) if on else []

    def __enter__(self):
        self.done = []
        try:
            for m in self.models:
                _lib.check(_lib.lib.ibo_gp_set_kstar_sf2(m._handle(), m.kernel._ibo_spec()[3]))
                self.done.append(m)
        except Exception:
            self.__exit__(None, None, None)
            raise
        return self

    def __exit__(self, *exc):
        for m in self.done:
            _lib.check(_lib.lib.ibo_gp_set_kstar_sf2(m._handle(), m.kernel._ibo_spec()[2]))
        self.done = []
        return False


POLISH_MAXITER = 30


class _HostPointAcquisition(object):
    """What MaxValueEntropy, ExpectedHypervolumeImprovement and the constrained classes offer alike, over the subclass's
    _call(X, grad) -> values (M,), or with grad (values, gradients (M, D)) from its *_grad_batch entry"""

    def values(self, X):
        """the value at many points at once"""
        return self._call(X, False)

    def f(self, x):
        return self._call(x, False)[0]

    def negf(self, x):
        return -self.f(x)

    def gradient(self, X):
        """(values, gradients (M, D)) at the points X, the conventions of negf"""
        return self._call(X, True)

    def negf_grad(self, x):
        """(negf(x), -grad f(x)): the objective and gradient scipy.optimize.minimize(jac=True) asks for"""
        v, g = self.gradient(x)
        return -v[0], -g[0]


def _polish_step(fg, value_at, lb, ub, opt, optx):
    """The polish step of every maximiser: bounded L-BFGS-B from DIRECT's point optx on fg(x) -> (-value, -gradient), x clipped to the
    box [lb, ub] first, at most POLISH_MAXITER iterations; the end point is re-evaluated with value_at(x) and kept only when strictly
    better than opt.  Returns (opt, optx)."""
    from scipy.optimize import minimize
    res = minimize(lambda x: fg(np.clip(x, lb, ub)), np.clip(optx, lb, ub), jac=True, method='L-BFGS-B', bounds=list(zip(lb, ub)),
                   options=dict(maxiter=POLISH_MAXITER, ftol=1e-15, gtol=1e-12))
    x = _lib.f64(np.clip(res.x, lb, ub))
    val = value_at(x)
    if val > opt:
        return float(val), x
    return opt, optx

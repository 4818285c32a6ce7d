"""
Constrained acquisition: EI / PI of an objective model weighted by the probability that constraint models are feasible
(Schonlau 1998; Gardner et al. 2014; Gelbart et al. 2014) -- "the best point of f where c1(x) <= t1 and c2(x) >= t2", the
constraints known only through their own, possibly noisy, observations.  The reference has nothing like it.

    Constraint(GP, upper=None, lower=None)       feasible where GP's function is <= upper, or >= lower (exactly one bound;
                                                 a band is two constraints on the same model)
    sweepConstrained(model, constraints, candidates, acq='ei'|'pi'|'pof', ...) -> dict(best_val, best_idx, [acq], [pof], [val])
    ConstrainedEI / ConstrainedPI / ProbFeasible  .f(x) .negf(x) .values(X) .gradient(X) .negf_grad(x)
    maximizeCEI / maximizeCPI(model, constraints, bounds, ...) -> (opt, optx)       DIRECT, optionally polished
    feasibleIncumbent(model, constraints)        the best observation of the objective that the constraint models call feasible

With (mu_j, s2_j) the posterior of constraint j at x and s_j = +1 for an upper, -1 for a lower bound t_j:

    z_j = s_j (t_j - mu_j) / sqrt(s2_j)      P(x) = prod_j Phi(z_j)      val(x) = A(x) P(x)

A is EI or PI of the objective ('pof': A = 1, the pure probability of feasibility -- what one maximises while no feasible
point is known).  UCB has no constrained form: a signed value times a probability orders nothing.  Every model keeps its own
data, kernel, noise and prior (a PrefGaussianProcess may be the objective or a constraint); they share the input dimension
and the device.  The objective model, or one constraint model, may appear more than once.

The incumbent: with ymax=None the sweep, the classes and the maximisers use feasibleIncumbent(model, constraints); when that
is None -- no observation is feasible -- they fall back to 'pof'.

Everything is computed by libibo_hip (ibo_cacq_sweep, ibo_cacq_batch, ibo_cacq_grad_batch, ibo_cacq_direct_max).
"""
import ctypes

import numpy as np

from .. import _lib
from . import _args
from ._args import _kstar_native

_CACQ = {'ei': _lib.ACQ_EI, 'pi': _lib.ACQ_PI, 'pof': _lib.ACQ_NONE}
MAX_CONSTRAINTS = 8          # IBO_CACQ_MAX_CON


class Constraint(object):
    """One inequality on the function a model describes: Constraint(GP, upper=t) is feasible where it is <= t,
    Constraint(GP, lower=t) where it is >= t.  Exactly one bound is given; a band is two constraints on the same model."""

    def __init__(self, GP, upper=None, lower=None):
        if (upper is None) == (lower is None):
            raise ValueError("a constraint has exactly one bound: upper= or lower= (a band is two constraints)")
        self.GP = GP
        self.sense = 1 if lower is None else -1
        self.thresh = float(upper if lower is None else lower)
        if not np.isfinite(self.thresh):
            raise ValueError("the bound must be finite")


def _pack(constraints):
    """(ncon, handles, thresholds, senses) as the ibo_cacq_* entries take them; every model's prior is pushed"""
    constraints = list(constraints)
    if len(constraints) > MAX_CONSTRAINTS:
        raise ValueError("at most %d constraints" % MAX_CONSTRAINTS)
    n = len(constraints)
    for c in constraints:
        if len(c.GP.X) == 0:
            raise ValueError("a constraint model has no data")
        _args._no_gradient(c.GP, "a constrained acquisition (constraint model)")
        c.GP._push_prior()
    con = (ctypes.c_void_p * max(n, 1))(*[c.GP._handle() for c in constraints])
    thresh = _lib.f64([c.thresh for c in constraints] or [0.0])
    sense = (ctypes.c_int * max(n, 1))(*[c.sense for c in constraints])
    return n, con, thresh, sense


def feasibleIncumbent(model, constraints):
    """The largest model.Y[i] among the rows whose constraint posterior MEANS at model.X[i] satisfy every bound, or None if
    there is no such row.  The constraint models may be observed at other points than the objective."""
    if len(model.X) == 0:
        return None
    ok = np.ones(len(model.X), dtype=bool)
    for c in constraints:
        mu, _ = c.GP._posterior_arrays(model.X, getvar=False)
        ok &= (mu <= c.thresh) if c.sense > 0 else (mu >= c.thresh)
    if not np.any(ok):
        return None
    return float(np.max(np.asarray(model.Y)[ok]))


def _incumbent(model, constraints, acq, ymax):
    """(acq, ymax) after the incumbent rule: ymax=None is feasibleIncumbent, and 'pof' where that is None"""
    if acq == 'pof':
        return acq, float('nan')
    if ymax is None:
        ymax = feasibleIncumbent(model, constraints)
        if ymax is None:
            return 'pof', float('nan')
    return acq, float(ymax)


def sweepConstrained(model, constraints, candidates, acq='ei', xi=0.01, native=True, ymax=None, exclude=None,
                     exclude_radius=0.5, index_base=0, outputs=()):
    """Evaluate a constrained acquisition over a whole candidate array and return its arg-max (ibo_cacq_sweep).

    constraints  a sequence of at most 8 Constraint objects (empty: the plain sweep() of the objective, bit for bit)
    candidates   (M, D) ndarray (uploaded) or a _lib.DeviceArray already in HBM
    acq          'ei', 'pi', or 'pof' (the probability of feasibility alone)
    native=True  what it means in sweep(): libm erf, variance clamp [1e-8, 10] and libego's k* signal variance -- on every
                 model involved, the Python values restored afterwards; native=False: NR erf, clamp [1e-7, 10]
    ymax         the incumbent; None: feasibleIncumbent(model, constraints), and acq='pof' when no observation is feasible
    exclude      points whose exclude_radius-ball is left out of the arg-max (the gallery's rule); index_base is added to
                 the reported index
    outputs      any of 'acq' (A), 'pof' (P), 'val' (A P): per-candidate arrays to return (host ndarrays)
    Returns dict(best_val, best_idx, acq_used, [acq], [pof], [val]).  NaN values and excluded candidates never win, the first
    maximiser wins ties, best_idx = -1 when everything is excluded.
    """
    constraints = list(constraints)
    _args._no_gradient(model, "sweepConstrained")
    if isinstance(candidates, _lib.DeviceArray):
        cand = candidates
    else:
        cand = _lib.DeviceArray.from_host(np.atleast_2d(candidates), model._dev.device)
    M = cand.shape[0]
    for k in outputs:
        if k not in ('acq', 'pof', 'val'):
            raise ValueError("unknown output %r" % (k,))
    acq, ym = _incumbent(model, constraints, acq, ymax)
    h = model._handle()
    model._push_prior()
    n, con, thresh, sense = _pack(constraints)
    outs = {k: _lib.DeviceArray((M,), model._dev.device) for k in outputs}
    ex = None if exclude is None or len(exclude) == 0 else _lib.f64(np.atleast_2d(exclude))
    bv = ctypes.c_double(); bi = ctypes.c_int64()
    with _kstar_native([model] + [c.GP for c in constraints], native):
        _lib.check(_lib.lib.ibo_cacq_sweep(
            h, n, con, _lib.dp(thresh), sense, M, cand.ptr, _CACQ[acq], float(xi), _lib.ERF_LIBM if native else _lib.ERF_NR,
            _lib.CLAMP_NATIVE if native else _lib.CLAMP_PY, ym, 0 if ex is None else len(ex),
            None if ex is None else _lib.dp(ex), float(exclude_radius), int(index_base),
            outs["acq"].ptr if "acq" in outs else None, outs["pof"].ptr if "pof" in outs else None,
            outs["val"].ptr if "val" in outs else None, ctypes.byref(bv), ctypes.byref(bi)))
    res = dict(best_val=bv.value, best_idx=bi.value, acq_used=acq)
    for k, v in outs.items():
        res[k] = v.to_host()
    return res


class _Constrained(_args._HostPointAcquisition):
    """the host-point classes: Python-class semantics (NR erf, clamp [1e-7, 10], the kernels' own k* variance), like EI / PI"""
    _acq = 'ei'

    def __init__(self, GP, constraints, xi=.01, ymax=None, **kwargs):
        _args._no_gradient(GP, "a constrained acquisition (ConstrainedEI / ConstrainedPI / ProbFeasible)")
        self.GP = GP
        self.constraints = list(constraints)
        self.xi = xi
        self.acq, self.ymax = _incumbent(GP, self.constraints, self._acq, ymax)

    def _call(self, X, grad):
        Q = _lib.f64(np.atleast_2d(np.asarray(X, dtype=float)))
        M, D = Q.shape
        self.GP._push_prior()
        n, con, thresh, sense = _pack(self.constraints)
        val = np.empty(M)
        lead = (self.GP._handle(), n, con, _lib.dp(thresh), sense, M, _lib.dp(Q), _CACQ[self.acq], float(self.xi), _lib.ERF_NR,
                _lib.CLAMP_PY, self.ymax)
        if not grad:
            _lib.check(_lib.lib.ibo_cacq_batch(*(lead + (None, None, _lib.dp(val)))))
            return val
        g = np.empty((M, D))
        _lib.check(_lib.lib.ibo_cacq_grad_batch(*(lead + (_lib.dp(val), _lib.dp(g)))))
        return val, g


class ConstrainedEI(_Constrained):
    """expected improvement over ymax times the probability of feasibility.  ymax=None: feasibleIncumbent(GP, constraints);
    when no observation is feasible the object evaluates the probability of feasibility alone (self.acq == 'pof')"""
    _acq = 'ei'


class ConstrainedPI(_Constrained):
    """probability of improvement over ymax + xi times the probability of feasibility; the incumbent rule of ConstrainedEI"""
    _acq = 'pi'


class ProbFeasible(_Constrained):
    """the probability that every constraint holds, prod_j Phi(z_j); the objective model only lends its dimension and device"""
    _acq = 'pof'

    def __init__(self, GP, constraints, **kwargs):
        super(ProbFeasible, self).__init__(GP, constraints, xi=0.0)


def _maximize(model, constraints, bounds, acq, xi, maxiter, maxtime, maxsample, polish, ymax, compat):
    constraints = list(constraints)
    if len(model.X) == 0:
        raise ValueError("model has no data")
    _args._no_gradient(model, "maximizeCEI / maximizeCPI")
    acq, ym = _incumbent(model, constraints, acq, ymax)
    lb = _lib.f64([b[0] for b in bounds]); ub = _lib.f64([b[1] for b in bounds])
    D = len(lb)
    h = model._handle()
    model._push_prior()
    n, con, thresh, sense = _pack(constraints)
    lead = (h, n, con, _lib.dp(thresh), sense)
    tail = (_CACQ[acq], float(xi), _lib.ERF_LIBM, _lib.CLAMP_NATIVE, ym)
    opt = ctypes.c_double(); optx = np.empty(D); ns = ctypes.c_int64()
    with _kstar_native([model] + [c.GP for c in constraints]):
        _lib.check(_lib.lib.ibo_cacq_direct_max(*(lead + (D, _lib.dp(lb), _lib.dp(ub)) + tail + (
            int(maxiter), int(maxtime), int(maxsample), 1 if compat else 0, ctypes.byref(opt), _lib.dp(optx), ctypes.byref(ns)))))
        best, bestx = opt.value, optx
        if polish:
            v, g = np.empty(1), np.empty((1, D))           # the polish step on the objective DIRECT maximised

            def fg(x):
                q = _lib.f64(x.reshape(1, D))
                _lib.check(_lib.lib.ibo_cacq_grad_batch(*(lead + (1, _lib.dp(q)) + tail + (_lib.dp(v), _lib.dp(g)))))
                return -v[0], -g[0].copy()

            def value_at(x):
                _lib.check(_lib.lib.ibo_cacq_batch(*(lead + (1, _lib.dp(x)) + tail + (None, None, _lib.dp(v)))))
                return v[0]

            best, bestx = _args._polish_step(fg, value_at, lb, ub, best, bestx)
    return best, bestx


def maximizeCEI(model, constraints, bounds, xi=0.01, maxiter=50, maxtime=30, maxsample=10000, polish=False, ymax=None,
                compat=True):
    """Maximise constrained expected improvement over the box `bounds` with DIRECT on the GPU objective (ibo_cacq_direct_max;
    libego semantics as maximizeEI: libm erf, clamp [1e-8, 10], libego's k* variance on every model) -> (opt, optx).
    ymax=None: feasibleIncumbent(model, constraints); when no observation is feasible the probability of feasibility is
    maximised instead.  polish=True: a bounded L-BFGS-B finish from DIRECT's point on ibo_cacq_grad_batch, at most
    POLISH_MAXITER iterations, kept only when strictly better.  compat: DIRECT's dimension-0 stall switch, as cdirectGP's."""
    return _maximize(model, constraints, bounds, 'ei', xi, maxiter, maxtime, maxsample, polish, ymax, compat)


def maximizeCPI(model, constraints, bounds, xi=0.01, maxiter=50, maxtime=30, maxsample=10000, polish=False, ymax=None,
                compat=True):
    """Maximise constrained probability of improvement; everything else as maximizeCEI."""
    return _maximize(model, constraints, bounds, 'pi', xi, maxiter, maxtime, maxsample, polish, ymax, compat)

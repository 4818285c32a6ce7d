"""
Two objectives: the expected hypervolume improvement (EHVI; Emmerich et al. 2006, Yang et al. 2019) -- "show me the points that
trade quality against cost", each objective known through its own model, both to be MAXIMISED and assumed independent.  The
reference has nothing like it: its acquisitions rank candidates for one objective.

    paretoFront(Y)                  the rows of an (n, 2) array no other row dominates, sorted by the first column
    hypervolume(Y, ref)             the area the rows of Y dominate above ref (pure NumPy)
    observedFront(models)           paretoFront of (Y1, Y2) when both models hold the same X
    sweepEHVI(models, candidates, ref, front=None, ...) -> dict(best_val, best_idx, [val])
    ExpectedHypervolumeImprovement(models, ref, front=None)   .f(x) .negf(x) .values(X) .gradient(X) .negf_grad(x)
    maximizeEHVI(models, bounds, ref, front=None, ...) -> (opt, optx)       DIRECT, optionally polished

With (mu_k, sigma_k) the posterior of objective k at x, psi_k(t) = sigma_k phi(u) + (mu_k - t) Phi(u), u = (mu_k - t) / sigma_k
(EI over t without xi), and the front in canonical form -- above ref = (r1, r2) in both coordinates, no dominated point, sorted
ascending in the first coordinate: (a_1, b_1) .. (a_n, b_n), a_0 = r1, a_{n+1} = +inf, b_{n+1} = r2 --

    EHVI(x) = sum_{i=0..n} max(psi_1(a_i) - psi_1(a_{i+1}), 0) psi_2(b_{i+1})

exactly: the improvement split into the n + 1 vertical strips between neighbouring a's.  An empty front: EI_1(r1) EI_2(r2).
Each model keeps its own data, kernel, noise and prior (a PrefGaussianProcess may be either objective); they share the input
dimension and the device, and one model may be both objectives.  At most 1024 front points are left after canonicalisation.

Everything is computed by libibo_hip (ibo_ehvi_sweep, ibo_ehvi_batch, ibo_ehvi_grad_batch, ibo_ehvi_direct_max); a candidate's
value is the same bits through each of them.
"""
import ctypes

import numpy as np

from .. import _lib
from . import _args
from ._args import _kstar_native

MAX_FRONT = 1024             # IBO_EHVI_MAX_FRONT


def paretoFront(Y):
    """The rows of Y (n, 2; both columns to be maximised) that no other row dominates, duplicates once, sorted ascending by the
    first column (the second is then strictly descending); (0, 2) for an empty Y."""
    Y = np.asarray(Y, dtype=float).reshape(-1, 2)
    if len(Y) == 0:
        return np.empty((0, 2))
    o = np.lexsort((-Y[:, 1], -Y[:, 0]))              # first column descending, the second descending among equals
    keep, best = [], -np.inf
    for i in o:
        if Y[i, 1] > best:
            keep.append(i)
            best = Y[i, 1]
    return Y[keep[::-1]].copy()


def hypervolume(Y, ref):
    """The area of the union of the boxes [ref, y] over the rows y of Y that lie strictly above ref in both columns."""
    Y = np.asarray(Y, dtype=float).reshape(-1, 2)
    r = np.asarray(ref, dtype=float).reshape(2)
    F = paretoFront(Y[(Y[:, 0] > r[0]) & (Y[:, 1] > r[1])])
    if len(F) == 0:
        return 0.0
    left = np.r_[r[0], F[:-1, 0]]
    return float(np.sum((F[:, 0] - left) * (F[:, 1] - r[1])))


def _pair(models):
    models = list(models)
    if len(models) != 2:
        raise ValueError("two objectives: models is a pair (the same model may be both)")
    for m in models:
        if len(m.X) == 0:
            raise ValueError("an objective model has no data")
        _args._no_gradient(m, "the expected hypervolume improvement")
    return models


def observedFront(models):
    """paretoFront of the observations (Y1[i], Y2[i]) when both models hold the same X; otherwise there are no joint
    observations to take a front of, and the caller passes front=."""
    a, b = _pair(models)
    Xa, Xb = np.atleast_2d(np.asarray(a.X, dtype=float)), np.atleast_2d(np.asarray(b.X, dtype=float))
    if Xa.shape != Xb.shape or not np.array_equal(Xa, Xb):
        raise ValueError("the two models are observed at different points: pass front= (an (n, 2) array of objective values)")
    return paretoFront(np.c_[np.asarray(a.Y, dtype=float).reshape(-1), np.asarray(b.Y, dtype=float).reshape(-1)])


def _lead(models, ref, front):
    """(objs, nfront, front, ref) as the ibo_ehvi_* entries take them, and what keeps their memory alive; priors are pushed"""
    models = _pair(models)
    F = _lib.f64(np.asarray(observedFront(models) if front is None else front, dtype=float).reshape(-1, 2))
    r = _lib.f64(np.asarray(ref, dtype=float).reshape(2))
    for m in models:
        m._push_prior()
    objs = (ctypes.c_void_p * 2)(*[m._handle() for m in models])
    return (objs, len(F), _lib.dp(F) if len(F) else None, _lib.dp(r)), (F, r, objs)


def sweepEHVI(models, candidates, ref, front=None, native=True, exclude=None, exclude_radius=0.5, index_base=0, outputs=()):
    """Evaluate EHVI over a whole candidate array and return its arg-max (ibo_ehvi_sweep).

    models       the pair of objective models        ref  the reference point (r1, r2)
    candidates   (M, D) ndarray (uploaded) or a _lib.DeviceArray already in HBM
    front        (n, 2) objective values (any set: it is brought into canonical form); None: observedFront(models)
    native=True  what it means in sweep(): libm erf, variance clamp [1e-8, 10] and libego's k* signal variance -- on both models,
                 the Python values restored afterwards; native=False: NR erf, clamp [1e-7, 10]
    exclude      points whose exclude_radius-ball is left out of the arg-max (the gallery's rule); index_base is added to the
                 reported index
    outputs      ('val',) to get the per-candidate values back (a host ndarray)
    Returns dict(best_val, best_idx, [val]).  NaN values and excluded candidates never win, the first maximiser wins ties,
    best_idx = -1 when nothing is admissible.
    """
    models = _pair(models)
    if isinstance(candidates, _lib.DeviceArray):
        cand = candidates
    else:
        cand = _lib.DeviceArray.from_host(np.atleast_2d(candidates), models[0]._dev.device)
    M = cand.shape[0]
    for k in outputs:
        if k != 'val':
            raise ValueError("unknown output %r" % (k,))
    lead, keep = _lead(models, ref, front)
    val = _lib.DeviceArray((M,), models[0]._dev.device) if 'val' in outputs else None
    ex = None if exclude is None or len(exclude) == 0 else _lib.f64(np.atleast_2d(exclude))
    bv = ctypes.c_double(); bi = ctypes.c_int64()
    with _kstar_native(models, native):
        _lib.check(_lib.lib.ibo_ehvi_sweep(*(lead + (
            M, cand.ptr, _lib.ERF_LIBM if native else _lib.ERF_NR, _lib.CLAMP_NATIVE if native else _lib.CLAMP_PY,
            0 if ex is None else len(ex), None if ex is None else _lib.dp(ex), float(exclude_radius), int(index_base),
            None if val is None else val.ptr, ctypes.byref(bv), ctypes.byref(bi)))))
    res = dict(best_val=bv.value, best_idx=bi.value)
    if val is not None:
        res['val'] = val.to_host()
    return res


class ExpectedHypervolumeImprovement(_args._HostPointAcquisition):
    """the host-point class: Python-class semantics (NR erf, clamp [1e-7, 10], the kernels' own k* variance), like EI / PI and
    the constrained classes.  front=None: observedFront(models), taken once, here."""

    def __init__(self, models, ref, front=None):
        self.models = _pair(models)
        self.ref = np.asarray(ref, dtype=float).reshape(2)
        self.front = paretoFront(observedFront(self.models) if front is None else front)

    def _call(self, X, grad):
        Q = _lib.f64(np.atleast_2d(np.asarray(X, dtype=float)))
        M, D = Q.shape
        lead, keep = _lead(self.models, self.ref, self.front)
        lead = lead + (M, _lib.dp(Q), _lib.ERF_NR, _lib.CLAMP_PY)
        val = np.empty(M)
        if not grad:
            _lib.check(_lib.lib.ibo_ehvi_batch(*(lead + (_lib.dp(val),))))
            return val
        g = np.empty((M, D))
        _lib.check(_lib.lib.ibo_ehvi_grad_batch(*(lead + (_lib.dp(val), _lib.dp(g)))))
        return val, g


def maximizeEHVI(models, bounds, ref, front=None, maxiter=50, maxtime=30, maxsample=10000, polish=False, compat=True):
    """Maximise EHVI over the box `bounds` with DIRECT on the GPU objective (ibo_ehvi_direct_max; libego semantics as maximizeEI:
    libm erf, clamp [1e-8, 10], libego's k* variance on both models) -> (opt, optx).  polish=True: a bounded L-BFGS-B finish from
    DIRECT's point on ibo_ehvi_grad_batch, at most POLISH_MAXITER iterations, kept only when strictly better.  compat: DIRECT's
    dimension-0 stall switch, as cdirectGP's."""
    models = _pair(models)
    lb = _lib.f64([b[0] for b in bounds]); ub = _lib.f64([b[1] for b in bounds])
    D = len(lb)
    lead, keep = _lead(models, ref, front)
    tail = (_lib.ERF_LIBM, _lib.CLAMP_NATIVE)
    opt = ctypes.c_double(); optx = np.empty(D); ns = ctypes.c_int64()
    with _kstar_native(models):
        _lib.check(_lib.lib.ibo_ehvi_direct_max(*(lead + (D, _lib.dp(lb), _lib.dp(ub)) + tail + (
            int(maxiter), int(maxtime), int(maxsample), 1 if compat else 0, ctypes.byref(opt), _lib.dp(optx), ctypes.byref(ns)))))
        best, bestx = opt.value, optx
        if polish:
            v, g = np.empty(1), np.empty((1, D))           # the polish step on the objective DIRECT maximised

            def fg(x):
                q = _lib.f64(x.reshape(1, D))
                _lib.check(_lib.lib.ibo_ehvi_grad_batch(*(lead + (1, _lib.dp(q)) + tail + (_lib.dp(v), _lib.dp(g)))))
                return -v[0], -g[0].copy()

            def value_at(x):
                _lib.check(_lib.lib.ibo_ehvi_batch(*(lead + (1, _lib.dp(x)) + tail + (_lib.dp(v),))))
                return v[0]

            best, bestx = _args._polish_step(fg, value_at, lb, ub, best, bestx)
    return best, bestx

"""
Acquisition functions and their maximisers, with the reference's names and
defaults (ego/acquisition/__init__.py):

    EI(GP, xi=.01)  PI(GP, xi=.01)  UCB(GP, NA, delta=0.1, scale=0.2)    .negf(x) / .f(x)
    .gradient(X) -> (values, gradients)   .negf_grad(x) -> (negf(x), -grad f(x))   (ibo_acq_grad_batch)
    maximizeEI(model, bounds, useCDIRECT=True, xi=0.01, maxiter=50, maxtime=30, maxsample=10000, polish=False)
    maximizePI(model, bounds, xi=0.01, maxiter=50, maxtime=30, maxsample=10000, useCDIRECT=True, polish=False)
    maximizeUCB(model, bounds, delta=0.1, scale=0.2, useCDIRECT=True, maxiter=50, maxtime=30, maxsample=10000, polish=False)
        -> (opt, optx);  polish=True: a bounded L-BFGS-B finish from DIRECT's point on the exact gradient

plus the batched entry point the GPU makes worthwhile:

    sweep(model, candidates, acq='ei', ...) -> dict(best_val, best_idx, [mu, s2, acq])

and the knowledge gradient against a reference set (knowledge.py): KnowledgeGradient, sweepKG, maximizeKG, referenceSet.
The value of a batch -- Monte-Carlo parallel EI with pending points and a greedy batch builder (batch.py): baseSamples, ParallelEI,
sweepQEI, maximizeQEI, jointQEI, proposeBatch.
Two objectives -- the expected hypervolume improvement over a Pareto front (multiobjective.py, imported as a submodule like
constrained.py): sweepEHVI, maximizeEHVI, ExpectedHypervolumeImprovement, paretoFront, hypervolume, observedFront.
Posterior draws as functions -- Thompson sampling over whole candidate arrays (pathwise.py): PosteriorPaths, spectralDraws;
with .gradient / .negf_grad (ibo_paths_grad_batch), .maximize(polish=True) and .maxima, every path's maximum by a lock-step ascent.
Max-value entropy search against samples of the maximum's value, exact (path maxima) or from a Gumbel fit that also serves a
preference GP (entropy.py): MaxValueEntropy, maxValueSamples, sweepMES, maximizeMES, gumbelFit.
Acquisitions integrated over samples of the hyper-parameters, on a GaussianProcessEnsemble (integrated.py): IntegratedEI, IntegratedPI,
IntegratedUCB, sweepIntegrated, maximizeIntegratedEI, maximizeIntegratedPI, maximizeIntegratedUCB.

The default maximize* path is the reference's cdirectGP -> acqmaxGP -> DIRECT
(ego/acquisition/__init__.py:307-447, cpp/optimizeGP.cpp:262-349) with the tree
on the host and every batch of sample points evaluated by the HIP sweep kernel.

Every kind of model -- plain, observed with gradients (G=), sparse -- goes through the same sweep, cdirectGP and _maximize: the model's
handle owner (model._owner(), gaussianprocess._Device) knows its kind and names the entry,

    kind 'gp'   ibo_acq_batch       ibo_acq_sweep (_incremental, _exchange)   ibo_direct_max       + ibo_gp_set_kstar_sf2, ibo_last_sweep_kernel_ms
    kind 'ggp'  ibo_ggp_acq_batch   ibo_ggp_acq_sweep                         ibo_ggp_direct_max
    kind 'sgp'  ibo_sgp_acq_batch   ibo_sgp_acq_sweep                         ibo_sgp_direct_max

and what a kind refuses of sweep() is the table _SWEEP_REFUSES.
"""
import ctypes

import numpy as np

from .. import _lib
from ..gaussianprocess import GaussianProcess, PrefGaussianProcess, CDF, PDF      # noqa: F401
from ..gaussianprocess.sparse import SparseGaussianProcess
from ..utils.optimize import direct, cdirect
from ..utils.latinhypercube import lhcSample                                        # noqa: F401
from . import _args
from ._args import POLISH_MAXITER                                                 # noqa: F401  (the polish step itself: _args._polish_step)

_ACQ = {'ei': _lib.ACQ_EI, 'pi': _lib.ACQ_PI, 'ucb': _lib.ACQ_UCB}


def _acq_gradient(GP, X, acq, parm, ymax):
    """values and gradients (M, D) of an acquisition at the points X with the Python classes' conventions (NR erf, clamp
    [1e-7, 10]): one ibo_acq_grad_batch call, or -- with an augmented factor in force -- the chain rule on the host from
    posterior_gradient, as GaussianProcess._eval forms the values there"""
    GP._no_gradient("gradient / negf_grad of an acquisition")
    Q = _lib.f64(np.atleast_2d(np.asarray(X, dtype=float)))
    M, D = Q.shape
    if GP._augdev is not None:
        mu, s2, dmu, ds2 = GP.posterior_gradient(Q)
        sig = np.sqrt(s2)
        dsig = ds2 / (2.0 * sig)[:, None]
        if acq == _lib.ACQ_UCB:
            return mu + parm * sig, dmu + parm * dsig
        yd = mu - ymax - parm
        Z = yd / sig
        if acq == _lib.ACQ_PI:
            return CDF(Z), (PDF(Z) / sig)[:, None] * (dmu - Z[:, None] * dsig)
        return yd * CDF(Z) + sig * PDF(Z), CDF(Z)[:, None] * dmu + PDF(Z)[:, None] * dsig
    GP._push_prior()
    val, grad = np.empty(M), np.empty((M, D))
    _lib.check(_lib.lib.ibo_acq_grad_batch(GP._handle(), M, _lib.dp(Q), acq, float(parm), _lib.ERF_NR, _lib.CLAMP_PY,
                                           float(ymax), None, None, _lib.dp(val), None, None, _lib.dp(grad)))
    return val, grad


class _ModelAcquisition(_args._HostPointAcquisition):
    """what EI, PI and UCB share (f, negf, values, gradient, negf_grad) over the subclass's _spec(grad) -> (acq code, parm, ymax):
    Python-class semantics, NR erf and the clamp [1e-7, 10]"""

    def _call(self, X, grad):
        code, parm, ymax = self._spec(grad)
        if grad:
            return _acq_gradient(self.GP, X, code, parm, ymax)
        return self.GP._eval(X, code, parm, _lib.ERF_NR, _lib.CLAMP_PY, ("acq",), ymax=ymax)["acq"]


class UCB(_ModelAcquisition):
    """upper confidence bound; note sqrt(scale * sBeta) with sBeta already a square
    root -- the class and the native path disagree in the reference and both are
    kept (ego/acquisition/__init__.py:60-71 vs :319)"""

    def __init__(self, GP, NA, delta=0.1, scale=0.2, **kwargs):
        super(UCB, self).__init__()
        self.GP = GP
        self.scale = scale
        t = len(self.GP.Y) + 1
        self.sBeta = np.sqrt(2.0 * np.log(t ** (NA // 2 + 2) * np.pi ** 2 / (3.0 * delta)))

    def _spec(self, grad):                           # (the value takes no incumbent; the gradient entry is handed one all the same)
        return _lib.ACQ_UCB, np.sqrt(self.scale * self.sBeta), np.max(self.GP.Y) if grad else None


class PI(_ModelAcquisition):
    """probability of improvement (:100-114); NR-erf CDF as the Python reference"""

    def __init__(self, GP, xi=.01, **kwargs):
        super(PI, self).__init__()
        self.GP = GP
        self.xi = xi
        self.Z = np.max(self.GP.Y) + xi

    def _spec(self, grad):
        return _lib.ACQ_PI, self.xi, self.Z - self.xi


class EI(_ModelAcquisition):
    """expected improvement (:138-169); NR-erf CDF/PDF as the Python reference.  .values(X): EI at many points at once (one GPU launch)"""

    def __init__(self, GP, xi=.01, **kwargs):
        super(EI, self).__init__()
        self.GP = GP
        self.ymax = np.max(self.GP.Y)
        self.xi = xi
        assert np.isscalar(self.ymax)
        assert np.isscalar(self.xi)

    def _spec(self, grad):
        return _lib.ACQ_EI, self.xi, self.ymax


def _ucb_parm(model, bounds, delta, scale):
    """sigma multiplier of the native UCB (ego/acquisition/__init__.py:316-319;
    NA/2 there is Python-2 integer division)"""
    t = len(model.Y) + 1
    NA = len(bounds)
    return float(np.sqrt(scale * 2.0 * np.log(t ** (NA // 2 + 2) * np.pi ** 2 / (3.0 * delta))))


def _default_parm(model, acq, nd, native, xi, delta, scale):
    """the parameter an acquisition takes where the caller names none: xi for EI and PI; for UCB in nd dimensions the sigma multiplier of
    the native path (_ucb_parm) or, native=False, the UCB class's"""
    if acq != 'ucb':
        return xi
    if native:
        return _ucb_parm(model, [None] * nd, delta, scale)
    return float(np.sqrt(scale * UCB(model, nd, delta, scale).sBeta))


def cdirectGP(model, bounds, maxiter, maxtime, maxsample, acqfunc=None, xi=-1, beta=-1, scale=-1, delta=-1, compat=True,
              return_samples=False, **kwargs):
    """cdirectGP (ego/acquisition/__init__.py:307-468), same name, positional order and defaults (`beta` is accepted and
    unused, as in the reference): same enum mapping and `parm`, then DIRECT on the GPU objective.  The model is already
    factored on the device, so the per-call linalg.inv(R) of the reference disappears.  `compat` / `return_samples` are
    additions (the dimension-0 stall switch, the sample count).
    Every kind of model takes the direct_max entry of its handle with libm erf and the native clamp; the plain kind runs it under
    libego's k* signal variance, a model observed with gradients and a sparse one under their own throughout (libego has neither to be
    compatible with)."""
    if acqfunc not in _ACQ:
        raise NotImplementedError('unknown acquisition function %s' % acqfunc)
    parm = _default_parm(model, acqfunc, len(bounds), True, xi, delta, scale)
    if len(model.X) == 0:
        raise ValueError("model has no data")
    lb = _lib.f64([b[0] for b in bounds]); ub = _lib.f64([b[1] for b in bounds])
    D = len(lb)
    plain = model._kind == 'gp'
    if plain:
        model._handle()
        model._push_prior()
    dev = model._owner()
    opt = ctypes.c_double(); optx = np.empty(D); ns = ctypes.c_int64()
    with _args._kstar_native([model], plain):
        _lib.check(dev.entry("direct_max")(dev.h, D, _lib.dp(lb), _lib.dp(ub), _ACQ[acqfunc], float(parm), _lib.ERF_LIBM,
                                           _lib.CLAMP_NATIVE, int(maxiter), int(maxtime), int(maxsample), 1 if compat else 0,
                                           ctypes.byref(opt), _lib.dp(optx), ctypes.byref(ns)))
    return (opt.value, optx, ns.value) if return_samples else (opt.value, optx)


gpuDirectGP = cdirectGP          # the name earlier rounds of this package used


def _polish(model, bounds, acqfunc, parm, opt, optx):
    """finish DIRECT's point with L-BFGS-B on the objective DIRECT maximised (libego's k* variance, libm erf, clamp
    [1e-8, 10], the same parm; one ibo_acq_grad_batch call per evaluation), bounded to the box and at most POLISH_MAXITER
    iterations.  The end point is re-evaluated with ibo_acq_batch and returned only if it is strictly better than DIRECT's."""
    lb = _lib.f64([b[0] for b in bounds]); ub = _lib.f64([b[1] for b in bounds])
    D = len(lb)
    code = _ACQ[acqfunc]
    h = model._handle()                              # (refuses the kinds without a gradient entry, as _maximize did before DIRECT ran)
    model._push_prior()
    v, g = np.empty(1), np.empty((1, D))

    def fg(x):
        q = _lib.f64(x.reshape(1, D))
        _lib.check(_lib.lib.ibo_acq_grad_batch(h, 1, _lib.dp(q), code, float(parm), _lib.ERF_LIBM, _lib.CLAMP_NATIVE,
                                               float('nan'), None, None, _lib.dp(v), None, None, _lib.dp(g)))
        return -v[0], -g[0].copy()

    def value_at(x):
        _lib.check(_lib.lib.ibo_acq_batch(h, 1, _lib.dp(x), code, float(parm), _lib.ERF_LIBM, _lib.CLAMP_NATIVE,
                                          float('nan'), None, None, _lib.dp(v)))
        return v[0]

    with _args._kstar_native([model]):
        return _args._polish_step(fg, value_at, lb, ub, opt, optx)


def _maximize(acqfunc, model, bounds, useCDIRECT, maxiter, maxtime, maxsample, polish, kwargs, **parms):
    """maximizeEI / PI / UCB; parms: the acquisition's own (xi=, or delta= and scale=)"""
    kwargs = dict(parms, **kwargs)
    if not useCDIRECT:
        print('using DIRECT')
        # (the reference forgets to forward the budgets in maximizeUCB (:86) and raises; they are forwarded)
        a = UCB(model, len(bounds), **kwargs) if acqfunc == 'ucb' else {'ei': EI, 'pi': PI}[acqfunc](model, **kwargs)
        opt, optx = direct(a.negf, bounds, maxiter=maxiter, maxtime=maxtime, maxsample=maxsample)
        return -opt, optx
    if isinstance(model, (GaussianProcess, SparseGaussianProcess)):
        if polish:
            model._no_gradient("maximize%s(polish=True)" % acqfunc.upper())
        opt, optx = cdirectGP(model, bounds, maxiter, maxtime, maxsample, acqfunc=acqfunc, **kwargs)
        if polish:
            return _polish(model, bounds, acqfunc, _ucb_parm(model, bounds, **parms) if acqfunc == 'ucb' else parms['xi'], opt, optx)
        return opt, optx
    raise ValueError


def maximizeUCB(model, bounds, delta=0.1, scale=0.2, useCDIRECT=True, maxiter=50, maxtime=30, maxsample=10000,
                polish=False, **kwargs):
    """maximise the GP-UCB of [Srinivas 2009] (:78-96); polish=True: see _polish"""
    return _maximize('ucb', model, bounds, useCDIRECT, maxiter, maxtime, maxsample, polish, kwargs, delta=delta, scale=scale)


def maximizePI(model, bounds, xi=0.01, maxiter=50, maxtime=30, maxsample=10000, useCDIRECT=True, polish=False, **kwargs):
    """maximise the probability of improvement [Lizotte 2008] (:117-134); polish=True: see _polish"""
    return _maximize('pi', model, bounds, useCDIRECT, maxiter, maxtime, maxsample, polish, kwargs, xi=xi)


def maximizeEI(model, bounds, useCDIRECT=True, xi=0.01, maxiter=50, maxtime=30, maxsample=10000, polish=False, **kwargs):
    """maximise expected improvement (:174-197); polish=True: see _polish"""
    return _maximize('ei', model, bounds, useCDIRECT, maxiter, maxtime, maxsample, polish, kwargs, xi=xi)


_SWEEP_REFUSES = {'gp': (), 'ggp': ('exclude', 'incremental', 'exchange'), 'sgp': ('incremental', 'exchange')}
_SWEEP_KERNEL = {'ggp': "gradobs row pipeline", 'sgp': "sparse two-frame sweep"}      # (the plain kind's handle names its own)


def sweep(model, candidates, acq='ei', xi=0.01, delta=0.1, scale=0.2, parm=None, native=True, ymax=None,
          exclude=None, exclude_radius=0.5, index_base=0, outputs=(), NA=None, incremental=False, exchange=None):
    """Evaluate an acquisition over a whole candidate array and return its arg-max.

    candidates   (M, D) ndarray (uploaded) or a _lib.DeviceArray already in HBM
    native=True  libego semantics: libm erf, variance clamp [1e-8, 10], k* with libego's sf2
    native=False Python-class semantics: NR erf, clamp [1e-7, 10]
    exclude      points whose exclude_radius-ball is left out of the arg-max (gallery rule)
    outputs      any of 'mu', 's2', 'acq': per-candidate arrays to return (host ndarrays)
    incremental  keep the per-candidate state of THIS DeviceArray on the model's handle and, when the model has only
                 grown through addData since the last such call, fold the new rows in instead of sweeping again
                 (fastUCBGallery's rounds).  Honoured for a caller-owned DeviceArray only (an ndarray is uploaded to a
                 temporary and swept in full); the state is keyed on the array's generation (_lib.DeviceArray.generation),
                 so a freed-and-reallocated or re-uploaded array is swept in full again
    exchange     an ibo_amd.multigpu.RcclArgmax: the sharded step in one device-side call (ibo_acq_sweep_exchange) -- this rank's
                 arg-max goes from the sweep's output words into the all-reduce buffer without visiting the host; the result then
                 also carries global_val, global_idx, global_x, global_rank (identical on every rank).  No `outputs` with it.
    Returns dict(best_val, best_idx, kernel_ms, [mu], [s2], [acq]); first maximiser wins ties.
    A model observed with gradients (G=) takes ibo_ggp_acq_sweep: the same arguments and result (kernel_ms is the whole call's device
    time), the model's own signal variance in both modes, and NotImplementedError for exclude=, incremental= and exchange=.
    A sparse model (SparseGaussianProcess) takes ibo_sgp_acq_sweep: the same, exclude= included; NotImplementedError for incremental= and
    exchange=.
    """
    kind = model._kind
    given = dict(exclude=exclude is not None and len(exclude) > 0, incremental=incremental, exchange=exchange is not None)
    for name in _SWEEP_REFUSES[kind]:
        if given[name]:
            model._no_gradient("sweep(%s=)" % name)
    plain = kind == 'gp'
    dev = model._owner()
    if isinstance(candidates, _lib.DeviceArray):
        cand = candidates
    else:
        cand = _lib.DeviceArray.from_host(np.atleast_2d(candidates), dev.device)
        incremental = False
    M = cand.shape[0]
    if parm is None:
        parm = _default_parm(model, acq, NA if NA is not None else cand.shape[1], native, xi, delta, scale)
    if plain:                                        # its handle (made now when there is none yet) and its mean prior
        model._handle()
        model._push_prior()
        dev = model._dev
    outs = {k: _lib.DeviceArray((M,), dev.device) for k in outputs}
    ex = None if exclude is None or len(exclude) == 0 else _lib.f64(np.atleast_2d(exclude))
    bv = ctypes.c_double(); bi = ctypes.c_int64()
    lead = (M, cand.ptr, _ACQ[acq], float(parm), _lib.ERF_LIBM if native else _lib.ERF_NR, _lib.CLAMP_NATIVE if native else _lib.CLAMP_PY,
            float('nan') if ymax is None else float(ymax))
    if kind != 'ggp':                                # (ibo_ggp_acq_sweep has no exclusion arguments)
        lead += (0 if ex is None else len(ex), None if ex is None else _lib.dp(ex), float(exclude_radius))
    lead += (int(index_base),)
    best = (ctypes.byref(bv), ctypes.byref(bi))
    glob = None
    t0 = None if plain else _lib.gpu_time_ms(dev.device)
    with _args._kstar_native([model], plain and native):
        if exchange is not None:
            if outputs:
                raise ValueError("per-candidate outputs are not available together with exchange=")
            gv = ctypes.c_double(); gi = ctypes.c_int64(); gr = ctypes.c_int(); gx = np.zeros(cand.shape[1])
            _lib.check(_lib.lib.ibo_acq_sweep_exchange(*((dev.h, exchange.h, 1 if incremental else 0) + lead + best + (
                ctypes.byref(gv), ctypes.byref(gi), _lib.dp(gx), ctypes.byref(gr)))))
            glob = dict(global_val=gv.value, global_idx=gi.value, global_x=gx, global_rank=gr.value)
        else:
            entry = _lib.lib.ibo_acq_sweep_incremental if incremental else dev.entry("acq_sweep")
            _lib.check(entry(*((dev.h,) + lead + tuple(outs[k].ptr if k in outs else None for k in ("mu", "s2", "acq")) + best)))
    if plain:
        ms = ctypes.c_float(); name = ctypes.c_char_p()
        _lib.check(_lib.lib.ibo_last_sweep_kernel_ms(dev.h, ctypes.byref(ms), ctypes.byref(name)))
        res = dict(best_val=bv.value, best_idx=bi.value, kernel_ms=ms.value, kernel=name.value.decode())
    else:
        res = dict(best_val=bv.value, best_idx=bi.value, kernel_ms=_lib.gpu_time_ms(dev.device) - t0, kernel=_SWEEP_KERNEL[kind])
    if glob is not None:
        res.update(glob)
    for k, v in outs.items():
        res[k] = v.to_host()
    return res


from .knowledge import KnowledgeGradient, sweepKG, maximizeKG, referenceSet          # noqa: E402,F401
from .batch import baseSamples, ParallelEI, sweepQEI, maximizeQEI, jointQEI, proposeBatch      # noqa: E402,F401
from .pathwise import PosteriorPaths, spectralDraws                                  # noqa: E402,F401
from .entropy import MaxValueEntropy, maxValueSamples, sweepMES, maximizeMES, gumbelFit      # noqa: E402,F401
from .integrated import (IntegratedEI, IntegratedPI, IntegratedUCB, sweepIntegrated, maximizeIntegratedEI,      # noqa: E402,F401
                         maximizeIntegratedPI, maximizeIntegratedUCB)

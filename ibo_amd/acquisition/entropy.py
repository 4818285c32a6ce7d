"""
Max-value entropy search (MES; Wang and Jegelka 2017): how much one observation at x tells about the VALUE of the maximum, y* --
the information-theoretic acquisition, and the usual answer to noisy objectives, where the incumbent max(Y) that EI improves on
is itself a noisy number.  The reference has nothing like it.

    maxValueSamples(GP, bounds=None, candidates=None, n=64, method='gumbel'|'paths', seed=None) -> (n,) samples of y*
    MaxValueEntropy(GP, ystar, latent=True)     .values(X) .f(x) .negf(x) .gradient(X) .negf_grad(x) .ystar
    sweepMES(GP, candidates, ystar, exclude=None, radius=0, index_base=0, outputs=False) -> dict(best_val, best_idx[, val])
    maximizeMES(GP, bounds, ystar=None, n_samples=64, method='gumbel', polish=False, ...) -> (opt, optx)

With (mu, s2) the posterior at x, v = max(s2 - s2_offset, clamp), sigma = sqrt(v) and gamma_k = (y*_k - mu) / sigma over the K samples
y*_k (sorted ascending by the library: their order does not matter),

    MES(x) = (1/K) sum_k h(gamma_k),     h(g) = g lambda(g) / 2 - log Phi(g),  lambda = phi / Phi

-- h is the entropy of N(0, 1) minus that of N(0, 1) truncated above at g, evaluated in a form that keeps log Phi in both tails.
latent=True asks for the information in the LATENT function (s2_offset = 1 + noise - sf2, so that v = sf2 - |v_x|^2; 0 where that is
negative, and for a preference GP, whose factor is not of K + noise), latent=False for that in a noisy observation (s2_offset = 0).

Where the samples come from: method='paths' draws them exactly -- the maxima of posterior paths (PosteriorPaths.maxima), with that
class's refusals (no preference GP); method='gumbel' is Wang and Jegelka's approximation, which needs only (mu, sigma) over a candidate
set and so works for every model: the cdf of the maximum over the candidates, prod_i Phi((t - mu_i) / sigma_i), is evaluated at 64
levels (ibo_mes_maxcdf), a Gumbel distribution is fitted to its quartiles and sampled.

Conventions of the Python classes everywhere: the kernel's own k* signal variance, variance clamp [1e-7, 10].  A point's value is the
same bits from every entry (within a size class of the sweep, see ibo_abi.h).  Everything is computed by libibo_hip (ibo_mes_sweep,
ibo_mes_batch, ibo_mes_grad_batch, ibo_mes_direct_max, ibo_mes_maxcdf); it works on a PrefGaussianProcess as on a GaussianProcess --
but not on a model observed with gradients (NotImplementedError), while an augmented factor is in force (addObservationPoint) or on
an empty model (ValueError).
"""
import ctypes
import functools

import numpy as np

from .. import _lib
from ..utils.latinhypercube import lhcSample
from . import _args
from .pathwise import MAXIMA_CANDIDATES, PosteriorPaths

MAX_SAMPLES = 1024           # IBO_MES_MAX_SAMPLES
MAX_LEVELS = 64              # IBO_MES_MAX_LEVELS
_NOUN = "max-value entropy search"
_points = functools.partial(_args._points, noun=_NOUN)


def _offset(GP, latent):
    """s2_offset of the ibo_mes_* entries: 1 + noise - sf2 for the latent variance of a plain GP where that is >= 0, else 0"""
    from ..gaussianprocess import PrefGaussianProcess
    if not latent or isinstance(GP, PrefGaussianProcess):
        return 0.0
    off = 1.0 + float(GP.noise) - float(GP.kernel._ibo_spec()[2])
    return off if off >= 0.0 else 0.0


def _samples(ystar):
    ys = _lib.f64(np.asarray(ystar, dtype=float).reshape(-1))
    if not 1 <= len(ys) <= MAX_SAMPLES:
        raise ValueError("between 1 and %d samples of the maximum" % MAX_SAMPLES)
    if not np.all(np.isfinite(ys)):
        raise ValueError("a sample of the maximum is not finite")
    return ys


def _maxcdf(GP, cand, levels, offset):
    """(logcdf (nlev,), (max mu, max(mu + 5 sigma))) over the device candidates (ibo_mes_maxcdf)"""
    lev = _lib.f64(np.asarray(levels, dtype=float).reshape(-1))
    out, stats = np.empty(len(lev)), np.empty(2)
    GP._push_prior()
    _lib.check(_lib.lib.ibo_mes_maxcdf(GP._handle(), cand.shape[0], cand.ptr, len(lev), _lib.dp(lev) if len(lev) else None, offset,
                                       _lib.CLAMP_PY, _lib.dp(out) if len(lev) else None, _lib.dp(stats)))
    return out, stats


def gumbelFit(levels, logcdf):
    """(a, b) of the Gumbel distribution exp(-exp(-(y - a) / b)) through the quartiles of a cdf given by its logarithm at ascending
    levels: y25, y50, y75 by linear interpolation of the cdf, b = (y25 - y75) / (log log(4/3) - log log 4), a = y50 + b log log 2"""
    cdf = np.exp(np.asarray(logcdf, dtype=float))
    y25, y50, y75 = np.interp([.25, .5, .75], cdf, np.asarray(levels, dtype=float))
    b = (y25 - y75) / (np.log(np.log(4.0 / 3.0)) - np.log(np.log(4.0)))
    return y50 + b * np.log(np.log(2.0)), b


def maxValueSamples(GP, bounds=None, candidates=None, n=64, method='gumbel', seed=None, latent=True):
    """n samples of the maximum's value y*.

    method='gumbel'   over `candidates` (an (M, D) ndarray, uploaded, or a _lib.DeviceArray; default: a seeded latin hypercube of
                      MAXIMA_CANDIDATES points in `bounds`): one ibo_mes_maxcdf call without levels for the bracket
                      [max mu, max(mu + 5 sigma)], a second at 64 evenly spaced levels in it, gumbelFit, then
                      a - b log(-log u) with u from np.random.default_rng(seed).uniform, floored at max mu
    method='paths'    PosteriorPaths(GP, n_paths=n, seed=seed).maxima(bounds, candidates)[0]: exact draws (n <= 256; no preference GP)
    latent            as MaxValueEntropy's: whose variance sigma is (the Gumbel method only; paths are draws of the latent function)
    """
    n = int(n)
    if not 1 <= n <= MAX_SAMPLES:
        raise ValueError("between 1 and %d samples of the maximum" % MAX_SAMPLES)
    if method == 'paths':
        if bounds is None:
            raise ValueError("method='paths' needs bounds")
        _args._no_gradient(GP, "the %s" % _NOUN)
        paths = PosteriorPaths(GP, n_paths=n, seed=seed)
        try:
            return _lib.f64(paths.maxima(bounds, candidates)[0])
        finally:
            paths.close()
    if method != 'gumbel':
        raise ValueError("unknown method %r" % (method,))
    D = np.asarray(GP.X).shape[1] if len(GP.X) else 0
    if candidates is None:
        if bounds is None:
            raise ValueError("bounds or candidates")
        _points(GP, np.zeros((1, D)), "candidates")                  # (the model's own refusals before any work)
        lb, ub, D = _args._bounds(bounds, D)
        candidates = np.array(lhcSample([list(b) for b in zip(lb, ub)], MAXIMA_CANDIDATES, seed=0 if seed is None else seed))
    if isinstance(candidates, _lib.DeviceArray):
        _points(GP, np.zeros((1, D)), "candidates")
    cand, _ = _args._candidates(GP, candidates, D, _NOUN)
    off = _offset(GP, latent)
    _, (lo, hi) = _maxcdf(GP, cand, [], off)
    if not np.isfinite(lo) or not np.isfinite(hi):
        raise ValueError("no candidate has a finite posterior")
    levels = np.linspace(lo, hi, MAX_LEVELS)
    logcdf, _ = _maxcdf(GP, cand, levels, off)
    a, b = gumbelFit(levels, logcdf)
    u = np.random.default_rng(seed).uniform(size=n)
    return _lib.f64(np.maximum(a - b * np.log(-np.log(u)), lo))


class MaxValueEntropy(_args._HostPointAcquisition):
    """MES(x) against the samples `ystar` of the maximum (1 .. 1024 finite numbers, any order); latent: the information in the latent
    function (the default) or in a noisy observation"""

    def __init__(self, GP, ystar, latent=True, **kwargs):
        _points(GP, np.zeros((1, np.asarray(GP.X).shape[1] if len(GP.X) else 0)), "X")
        self.GP = GP
        self.ystar = np.sort(_samples(ystar))
        self.latent = bool(latent)

    def _call(self, X, grad):
        Q = _points(self.GP, X, "X")
        M, D = Q.shape
        self.GP._push_prior()
        lead = (self.GP._handle(), len(self.ystar), _lib.dp(self.ystar), _offset(self.GP, self.latent), M, _lib.dp(Q), _lib.CLAMP_PY)
        val = np.empty(M)
        if not grad:
            _lib.check(_lib.lib.ibo_mes_batch(*(lead + (_lib.dp(val),))))
            return val
        g = np.empty((M, D))
        _lib.check(_lib.lib.ibo_mes_grad_batch(*(lead + (_lib.dp(val), _lib.dp(g)))))
        return val, g


def sweepMES(GP, candidates, ystar, exclude=None, radius=0, index_base=0, outputs=False, latent=True):
    """MES over a whole candidate array and its arg-max (ibo_mes_sweep): candidates an (M, D) ndarray (uploaded) or a
    _lib.DeviceArray already in HBM.  exclude: points whose `radius`-ball is left out of the arg-max (the gallery's rule); index_base
    is added to the reported index.  Returns dict(best_val, best_idx) and, with outputs=True, val (M,).  NaN values and excluded
    candidates never win, the first maximiser wins ties, best_idx = -1 (with -inf) when nothing is admissible."""
    ys = _samples(ystar)
    D = np.asarray(GP.X).shape[1] if len(GP.X) else 0
    if isinstance(candidates, _lib.DeviceArray):
        _points(GP, np.zeros((1, D)), "candidates")
    cand, _ = _args._candidates(GP, candidates, D, _NOUN)
    M = cand.shape[0]
    GP._push_prior()
    val = _lib.DeviceArray((M,), GP._dev.device) if outputs else None
    ex = None if exclude is None or len(exclude) == 0 else _lib.f64(np.atleast_2d(exclude))
    bv = ctypes.c_double(); bi = ctypes.c_int64()
    _lib.check(_lib.lib.ibo_mes_sweep(GP._handle(), len(ys), _lib.dp(ys), _offset(GP, latent), M, cand.ptr, _lib.CLAMP_PY,
                                      0 if ex is None else len(ex), None if ex is None else _lib.dp(ex), float(radius), int(index_base),
                                      None if val is None else val.ptr, ctypes.byref(bv), ctypes.byref(bi)))
    res = dict(best_val=bv.value, best_idx=bi.value)
    if val is not None:
        res['val'] = val.to_host()
    return res


def maximizeMES(GP, bounds, ystar=None, n_samples=64, method='gumbel', seed=None, latent=True, maxiter=50, maxtime=30, maxsample=10000,
                polish=False, compat=False):
    """Maximise MES over the box `bounds` with DIRECT on the GPU objective (ibo_mes_direct_max) -> (opt, optx).
    ystar=None: maxValueSamples(GP, bounds, n=n_samples, method=method, seed=seed).  opt is MaxValueEntropy(GP, ystar, latent).f(optx),
    bit for bit.  polish=True: a bounded L-BFGS-B finish from DIRECT's point on ibo_mes_grad_batch, at most POLISH_MAXITER
    iterations, the end point re-evaluated and kept only when strictly better."""
    acq = MaxValueEntropy(GP, maxValueSamples(GP, bounds, n=n_samples, method=method, seed=seed, latent=latent) if ystar is None else ystar,
                          latent)
    lb, ub, D = _args._bounds(bounds, np.asarray(GP.X).shape[1])
    GP._push_prior()
    opt = ctypes.c_double(); optx = np.empty(D); ns = ctypes.c_int64()
    _lib.check(_lib.lib.ibo_mes_direct_max(GP._handle(), len(acq.ystar), _lib.dp(acq.ystar), _offset(GP, latent), D, _lib.dp(lb), _lib.dp(ub),
                                           _lib.CLAMP_PY, int(maxiter), int(maxtime), int(maxsample), 1 if compat else 0,
                                           ctypes.byref(opt), _lib.dp(optx), ctypes.byref(ns)))
    if not polish:
        return opt.value, optx
    return _args._polish_step(acq.negf_grad, acq.f, lb, ub, opt.value, optx)

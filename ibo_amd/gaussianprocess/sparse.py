"""
A sparse Gaussian process on inducing points (DTC / FITC) on the MI355X backend (ibo_sgp_*).

    SparseGaussianProcess(kernel, X=None, Y=None, Z=None, m=None, noise=.1, jitter=1e-6, method='fitc', seed=None, device=None)
        .addData(X, Y)  .posterior(x, getvar=True)  .posteriors(X)  .mu(x)  .negmu(x)  .nlml(kind=None)  .close()
        .nlml_gradient(kind=None, wrt=('hyper', 'noise', 'Z'))      <- the objective and its gradient at the model's parameters
        .learn(kind=None, learn_hyper=True, learn_noise=True, learn_Z=True, maxiter=50, bounds=None)      <- L-BFGS-B on it
        attributes X, Y, Z, noise, kernel
    inducingPoints(X, m, method='subset'|'kcenter', seed=None)

The model is m rows whatever the number of observations: the fit is O(N m^2), a swept candidate costs two m-row sweeps, and addData
accumulates into the device's kept Gram matrix -- O(n m^2 + m^3), no stored data on the device.  (X and Y are kept HERE, on the host, as
the plain model's attributes are; nothing reads them after the first fit but max(Y) for the acquisition classes -- and nlml_gradient /
learn, which stream them through ibo_sgp_nlml_grad again.)

EI / PI / UCB(model).f / .negf / .values, acquisition.sweep and maximizeEI / PI / UCB work on it, through the routes every kind of model
takes (the handle is a gaussianprocess._Device of kind 'sgp': ibo_sgp_acq_batch, ibo_sgp_acq_sweep, ibo_sgp_direct_max); everything else
that takes a model refuses it with a NotImplementedError that names the call.
"""
import ctypes

import numpy as np

from .. import _lib
from . import _Device, _acq_batch
from .trainhyper import _grad_spec, _learn

_METHOD = {'fitc': 0, 'dtc': 1}
_NLML_MODEL, _NLML_VFE = 0, 1
_GET = dict(Kuu=0, G=1, A=2, Lu=3, LA=4, b=5, alpha=6, yy=7, ll=8, tt=9, N=10)

_KIND = {'fitc': 0, 'dtc': 1, 'vfe': 2}

_SPARSE_WHY = ("the model is a sparse GP on inducing points: only posterior, posteriors, mu, negmu, nlml, nlml_gradient, learn, addData, "
               "EI / PI / UCB (.f, .negf, .values), acquisition.sweep and maximizeEI / PI / UCB are built for it")


def nlml_grad_raw(kernel, X, Y, Z, noise, jitter, kind, ngrad=None, want=('hyper', 'noise', 'Z'), device=None):
    """ibo_sgp_nlml_grad for a kernel object: (value, dict of the gradients asked for) with respect to the LOG of the kernel's first
    ngrad hyper-parameters (kernel._ibo_grad_spec; None: all), the log noise and the inducing points.  kind: 'fitc', 'dtc' or 'vfe'."""
    if kind not in _KIND:
        raise ValueError("unknown objective %r ('fitc', 'dtc' or 'vfe')" % (kind,))
    Xc, Yc, Zc = _lib.rows(X), _lib.f64(Y), _lib.f64(np.array(Z, dtype=float, ndmin=2))
    N, D = Xc.shape
    if len(Yc) != N:
        raise ValueError("X has %d rows, Y %d" % (N, len(Yc)))
    if Zc.shape[1] != D:
        raise ValueError("Z has %d columns, the data %d" % (Zc.shape[1], D))
    ktype, hyper, sf2, _ = kernel._ibo_spec()
    modes, dims = _grad_spec(kernel, D, ngrad)
    n = len(modes) if 'hyper' in want else 0
    gh = np.empty(n) if n else None
    gn = ctypes.c_double() if 'noise' in want else None
    gz = np.empty(Zc.shape) if 'Z' in want else None
    v = ctypes.c_double()
    info = ctypes.c_int(0)
    _lib.check(_lib.lib.ibo_sgp_nlml_grad(_lib.default_device() if device is None else device, ktype, D, _lib.dp(hyper), len(hyper), sf2,
                                          float(noise), float(jitter), _KIND[kind], len(Zc), _lib.dp(Zc), N, _lib.dp(Xc), _lib.dp(Yc),
                                          n, modes, dims, ctypes.byref(v), None if gh is None else _lib.dp(gh),
                                          None if gn is None else ctypes.cast(ctypes.byref(gn), ctypes.POINTER(ctypes.c_double)),
                                          None if gz is None else _lib.dp(gz), ctypes.byref(info)))
    out = {}
    if 'hyper' in want:
        out['hyper'] = gh if gh is not None else np.empty(0)
    if gn is not None:
        out['noise'] = gn.value
    if gz is not None:
        out['Z'] = gz
    return v.value, out


def inducingPoints(X, m, method='subset', seed=None):
    """m of the rows of X as inducing points, on the host: 'subset' a seeded random subset (in ascending row order), 'kcenter' greedy
    farthest-point selection from a seeded first row (each further point is the row farthest from those chosen so far, the lowest row
    winning ties)"""
    X = np.array(X, dtype=float, ndmin=2)
    N = len(X)
    m = int(m)
    if m < 1 or m > N:
        raise ValueError("m=%d inducing points out of %d rows" % (m, N))
    rng = np.random.RandomState(seed)
    if method == 'subset':
        return X[np.sort(rng.permutation(N)[:m])].copy()
    if method == 'kcenter':
        idx = [int(rng.randint(N))]
        d2 = np.sum((X - X[idx[0]]) ** 2, axis=1)
        for _ in range(m - 1):
            k = int(np.argmax(d2))
            idx.append(k)
            d2 = np.minimum(d2, np.sum((X - X[k]) ** 2, axis=1))
        return X[idx].copy()
    raise ValueError("unknown selection method %r ('subset' or 'kcenter')" % (method,))


class _DeviceSGP(_Device):
    kind = 'sgp'


class SparseGaussianProcess(object):

    _kind = 'sgp'          # the kind of the model's handle (_Device)

    def __init__(self, kernel, X=None, Y=None, Z=None, m=None, noise=.1, jitter=1e-6, method='fitc', seed=None, device=None,
                 prior=None, selection='subset'):
        if prior is not None:
            raise NotImplementedError("a mean prior (prior=): not available, %s" % _SPARSE_WHY)
        if method not in _METHOD:
            raise ValueError("unknown method %r ('fitc' or 'dtc')" % (method,))
        if (X is None) != (Y is None):
            raise ValueError
        self.kernel = kernel
        self.noise = noise
        self.jitter = jitter
        self.method = method
        self.seed = seed
        self.selection = selection
        self.prior = None
        self.G = None
        self.name = 'SGP'
        self._device = device
        self._m = m
        self._sdev = None
        self._lambda = None
        self.Z = None if Z is None else np.array(Z, dtype=float, ndmin=2)
        self.X = np.zeros((0, 0))
        self.Y = np.zeros((0))
        if X is not None:
            self.addData(X, Y)

    # ------------------------------------------------------------------ refusals
    def _no_gradient(self, what):
        """the one refusal of everything that is not built for a sparse model (the name is the plain model's: the acquisition
        modules ask every model this before they touch it)"""
        raise NotImplementedError("%s: not available, %s" % (what, _SPARSE_WHY))

    def _handle(self):
        self._no_gradient("this call (it takes the model's ibo_gp_t handle)")

    def removeData(self, *a, **k):
        self._no_gradient("removeData")

    def posterior_gradient(self, *a, **k):
        self._no_gradient("posterior_gradient")

    def posterior_cov(self, *a, **k):
        self._no_gradient("posterior_cov")

    def sample_posterior(self, *a, **k):
        self._no_gradient("sample_posterior")

    def loo(self, *a, **k):
        self._no_gradient("loo")

    def loo_score(self, *a, **k):
        self._no_gradient("loo_score")

    def addObservationPoint(self, *a, **k):
        self._no_gradient("addObservationPoint")

    # ------------------------------------------------------------------ device plumbing
    @property
    def _dev(self):
        return self._sdev

    def _owner(self):
        """the handle owner (_Device) that _eval, sweep and cdirectGP run on"""
        if self._sdev is None:
            raise ValueError("model has no data")
        return self._sdev

    def _fit(self, X, Y):
        """fit a NEW handle from the data and swap it in only when that succeeded: a matrix that does not factor leaves the previous
        model answering with its earlier bits"""
        if self.Z is None:
            if self._m is None:
                raise ValueError("neither Z= nor m= was given")
            self.Z = inducingPoints(X, min(int(self._m), len(X)), self.selection, self.seed)
        ktype, hyper, sf2, _ = self.kernel._ibo_spec()
        N, D = X.shape
        if self.Z.shape[1] != D:
            raise ValueError("Z has %d columns, the data %d" % (self.Z.shape[1], D))
        dev = _DeviceSGP(self._device)
        Zc, Xc, Yc = _lib.f64(self.Z), _lib.f64(X), _lib.f64(Y)
        lam = np.empty(N)
        info = ctypes.c_int(0)
        rc = _lib.lib.ibo_sgp_fit(dev.h, ktype, D, _lib.dp(hyper), len(hyper), sf2, float(self.noise), float(self.jitter),
                                  _METHOD[self.method], len(Zc), _lib.dp(Zc), N, _lib.dp(Xc), _lib.dp(Yc), _lib.dp(lam), ctypes.byref(info))
        if rc != _lib.OK:
            msg = _lib.lib.ibo_last_error()              # (closing the handle must not replace the message)
            dev.close()
            if rc == _lib.ERR_NOT_PD:
                raise _lib.NotPositiveDefinite(rc, msg.decode("utf-8", "replace"))
            raise _lib.IBOError(rc, msg.decode("utf-8", "replace"))
        old, self._sdev = self._sdev, dev
        if old is not None:
            old.close()
        self._lambda = lam

    def addData(self, X, Y):
        """the first data fit the model; later data are accumulated into the device's kept sums (ibo_sgp_add) and A is factored again.
        A failed accumulation leaves the device handle unfitted: the model is then refitted from all the data on a new handle."""
        X = np.array(X, dtype=float, ndmin=2)
        Y = np.array(Y, dtype=float, ndmin=1).reshape(-1)
        if len(X) != len(Y):
            raise ValueError("X has %d rows, Y %d" % (len(X), len(Y)))
        if not (np.all(np.isfinite(X)) and np.all(np.isfinite(Y))):
            raise ValueError("X / Y hold a value that is not finite")
        if self._sdev is None:
            first = len(self.X) == 0
            allX = np.copy(X) if first else np.r_[self.X, X]
            allY = np.copy(Y) if first else np.r_[self.Y, Y]
            self._fit(allX, allY)                      # (raises before anything of the model changes)
            self.X, self.Y = allX, allY
            return
        if X.shape[1] != self.X.shape[1]:
            raise ValueError("X has %d columns, the model %d" % (X.shape[1], self.X.shape[1]))
        Xc, Yc = _lib.f64(X), _lib.f64(Y)
        lam = np.empty(len(Xc))
        info = ctypes.c_int(0)
        _lib.check(_lib.lib.ibo_sgp_add(self._sdev.h, len(Xc), _lib.dp(Xc), _lib.dp(Yc), _lib.dp(lam), ctypes.byref(info)))
        self.X, self.Y = np.r_[self.X, X], np.r_[self.Y, Y]
        self._lambda = np.r_[self._lambda, lam]

    def refit(self, Z=None, m=None):
        """fit again from all the data, with other inducing points (Z=, or m= rows chosen anew)"""
        if len(self.X) == 0:
            raise ValueError("model has no data")
        keep = self.Z, self._m
        if Z is not None:
            self.Z = np.array(Z, dtype=float, ndmin=2)
        elif m is not None:
            self.Z, self._m = None, m
        try:
            self._fit(self.X, self.Y)
        except Exception:
            self.Z, self._m = keep
            raise

    def close(self):
        if self._sdev is not None:
            self._sdev.close()
            self._sdev = None

    def _get(self, name):
        """what the device model is made of (ibo_sgp_get): 'Kuu', 'G', 'A', 'Lu', 'LA' (m x m), 'b', 'alpha' (m), 'yy', 'll', 'tt', 'N'"""
        m = len(self.Z)
        code = _GET[name]
        out = np.empty((m, m) if code <= 4 else (m if code <= 6 else 1))
        _lib.check(_lib.lib.ibo_sgp_get(self._sdev.h, code, _lib.dp(out)))
        return out if code <= 6 else float(out[0])

    def _eval(self, Q, acq=_lib.ACQ_NONE, parm=0.0, erf_mode=_lib.ERF_NR, clamp_lo=_lib.CLAMP_PY, want=("mu", "s2"), ymax=None):
        """host points in, host arrays out (ibo_sgp_acq_batch): the plain model's _eval"""
        return _acq_batch(self._owner(), _lib.f64(np.atleast_2d(Q)), acq, parm, erf_mode, clamp_lo, want, ymax)

    # ------------------------------------------------------------------ the plain model's API
    def posterior(self, X, getvar=True):
        """posterior mean (and variance, the noise included) at ONE point"""
        if self._sdev is None:
            return (0.0, 1.0) if getvar else 0.0
        X = np.array(X, dtype=float, ndmin=2)
        res = self._eval(X[:1], want=("mu", "s2") if getvar else ("mu",))
        if getvar:
            return res["mu"][0], res["s2"][0]
        return res["mu"][0]

    def posteriors(self, X):
        """(mu, s2) arrays at the rows of X"""
        res = self._eval(np.array(X, dtype=float, ndmin=2))
        return res["mu"], res["s2"]

    def mu(self, x):
        return self.posterior(x, getvar=False)

    def negmu(self, x):
        return -self.mu(x)

    def nlml(self, kind=None):
        """the negative log marginal likelihood of the model as fitted (kind None, or the model's own method), or kind='vfe': Titsias'
        bound, the DTC value plus its trace term (a 'dtc' model only).  Value only: nlml_gradient gives the gradient."""
        if self._sdev is None:
            raise ValueError("model has no data")
        if kind is None or kind == self.method:
            code = _NLML_MODEL
        elif kind == 'vfe':
            if self.method != 'dtc':
                raise ValueError("kind='vfe' is the DTC value plus a trace term: fit the model with method='dtc'")
            code = _NLML_VFE
        else:
            raise ValueError("kind=%r on a model fitted with method=%r" % (kind, self.method))
        v = ctypes.c_double()
        _lib.check(_lib.lib.ibo_sgp_nlml(self._sdev.h, code, ctypes.byref(v)))
        return v.value

    def _objective(self, kind):
        if kind is None:
            return 'vfe' if self.method == 'dtc' else self.method
        if kind == self.method or (kind == 'vfe' and self.method == 'dtc'):
            return kind
        if kind == 'vfe':
            raise ValueError("kind='vfe' is the DTC value plus a trace term: fit the model with method='dtc'")
        raise ValueError("kind=%r on a model fitted with method=%r" % (kind, self.method))

    def nlml_gradient(self, kind=None, wrt=('hyper', 'noise', 'Z')):
        """(value, {'hyper': ..., 'noise': ..., 'Z': ...}): the sparse negative log marginal likelihood at the model's current kernel, noise,
        Z and data, and its gradient with respect to the LOG of every kernel hyper-parameter, the log noise and every coordinate of every
        inducing point (ibo_sgp_nlml_grad: one device call that streams the host's X and Y).  kind None: 'vfe' on a 'dtc' model, the
        model's own objective otherwise; 'vfe' is Titsias' bound."""
        if self._sdev is None:
            raise ValueError("model has no data")
        wrt = tuple(wrt)
        for w in wrt:
            if w not in ('hyper', 'noise', 'Z'):
                raise ValueError("wrt holds %r ('hyper', 'noise', 'Z')" % (w,))
        return nlml_grad_raw(self.kernel, self.X, self.Y, self.Z, self.noise, self.jitter, self._objective(kind), want=wrt,
                             device=self._sdev.device)

    def learn(self, kind=None, learn_hyper=True, learn_noise=True, learn_Z=True, maxiter=50, bounds=None):
        """minimise the sparse marginal likelihood (kind as nlml_gradient's) over [log theta, log noise, vec Z] -- whichever of the three
        are switched on -- by L-BFGS-B on ibo_sgp_nlml_grad: every evaluation is one device call, a point where a matrix does not factor
        counts as +inf for the line search.  bounds: L-BFGS-B's, one (lo, hi) per variable in that order, or None.  When the search ends
        at a finite value below the one it started from -- also when it stopped for lack of iterations -- the kernel is rebuilt as
        kernel.__class__(exp(log theta)), noise and Z are set and the model is refitted; a failing refit leaves the model as it was.
        Otherwise (the start does not factor, nothing lower was found) the model is not touched.  Returns the scipy result with
        .start_value, .end_value, .evaluations and .applied (trainhyper._learn)."""
        if self._sdev is None:
            raise ValueError("model has no data")
        kind = self._objective(kind)
        cls = self.kernel.__class__
        th0 = np.log(np.asarray(self.kernel.hyperparams, dtype=float))
        Z0 = np.array(self.Z, dtype=float)
        nh = len(th0) if learn_hyper else 0
        x0 = np.r_[th0[:nh], [np.log(float(self.noise))] if learn_noise else [], Z0.ravel() if learn_Z else []]
        want = tuple(w for w, on in (('hyper', learn_hyper), ('noise', learn_noise), ('Z', learn_Z)) if on)
        dev = self._sdev.device

        def unpack(x):
            o = nh
            kern = cls(np.exp(x[:nh])) if learn_hyper else self.kernel
            noise = float(self.noise)
            if learn_noise:
                noise = float(np.exp(x[o])); o += 1
            return dict(kernel=kern, noise=noise, Z=np.array(x[o:].reshape(Z0.shape) if learn_Z else Z0, dtype=float))

        def fg(x):
            p = unpack(x)
            v, g = nlml_grad_raw(p["kernel"], self.X, self.Y, p["Z"], p["noise"], self.jitter, kind, want=want, device=dev)
            return v, np.r_[g.get('hyper', []), [g['noise']] if learn_noise else [], g['Z'].ravel() if learn_Z else []]

        return _learn(self, x0, fg, unpack, lambda: self._fit(self.X, self.Y), maxiter, bounds)

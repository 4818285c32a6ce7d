"""
Marginal likelihood of the GP hyper-parameters (ego/gaussianprocess/trainhyper.py).

    marginalLikelihood(kernel, X, Y, nhyper, computeGradient=True, useCholesky=True, noise=1e-3)
    nlml(loghyper, Kernel, X, Y)     dnlml(loghyper, Kernel, X, Y)     nlmlMulti(...)
    nlml_grid(KernelClass, thetas, X, Y, noise=1e-3)      <- new: a whole theta grid in one call
    looLikelihood(kernel, X, Y, nhyper, computeGradient=True, noise=1e-3, predictions=False)      <- new: the leave-one-out objective
    nloo(loghyper, Kernel, X, Y, noise=1e-3)     dnloo(loghyper, Kernel, X, Y, noise=1e-3)
    sparseLikelihood(kernel, X, Y, Z, nhyper, noise, jitter=1e-6, kind='vfe', computeGradient=True, gradZ=True)      <- new: the sparse
        model's objective (FITC, DTC or Titsias' bound) with its gradient w.r.t. log theta, log noise and the inducing points
    gradientLikelihood(kernel, X, Y, G, nhyper, noise=1e-3, gnoise=1e-4, computeGradient=True, gradNoise=False)      <- new: the likelihood
        of a model observed with gradients (GaussianProcess(G=)), with its gradient w.r.t. log theta, log noise and log gnoise
    ngnlml(loghyper, Kernel, X, Y, G, noise=1e-3, gnoise=1e-4)     dgnlml(loghyper, Kernel, X, Y, G, noise=1e-3, gnoise=1e-4)

The value (K assembly, Cholesky, L^-1 Y, log det) is computed on the GPU by
ibo_nlml_grid; value + gradient for one theta by ibo_nlml_grad (K^-1 = W^T W from the device
factorisation, then one fused kernel contracts K^-1 - alpha alpha^T with every dK/dtheta_i,
recomputed from X on the fly).  The leave-one-out objective (Rasmussen & Williams 5.4.2), its gradient and the leave-one-out
predictions come from ibo_loo_grad: the same sequence up to K^-1, then T = K^-1 dK/dtheta_i on the MFMA unit.
These three factor N x N; the sparse model's likelihood on m inducing points, O(N m^2), comes from ibo_sgp_nlml_grad, and the
N (D + 1)-row likelihood of values and slopes from ibo_ggp_nlml_grad.
"""
import ctypes
import hashlib

import numpy as np
from numpy.linalg import LinAlgError

from .. import _lib


def _no_gradient_data(G, what):
    """hyper-parameter learning is built for value observations: the likelihoods of an N (D + 1)-row gradient model are not"""
    if G is not None:
        raise NotImplementedError("%s with gradient observations (G=): this likelihood factors K(X, X) of the values alone -- the "
                                  "N (D + 1)-row model's own is trainhyper.gradientLikelihood (GaussianProcess.nlml / .learn)" % what)


def _spec_rows(kernels):
    specs = [k._ibo_spec() for k in kernels]
    ktype = specs[0][0]
    thetas = _lib.f64(np.array([s[1] for s in specs]))
    sf2 = _lib.f64([s[2] for s in specs])
    return ktype, thetas, sf2


def _grad_spec(kernel, D, nhyper):
    """(modes, dims): kernel._ibo_grad_spec(D)'s first nhyper rows (None: all of them) as the two int arrays the *_grad entries take"""
    spec = kernel._ibo_grad_spec(D)
    if nhyper is not None:
        if len(spec) < nhyper:
            raise ValueError("kernel has %d hyperparameters, %d gradients requested" % (len(spec), nhyper))
        spec = spec[:nhyper]
    return (ctypes.c_int * len(spec))(*[m for m, _ in spec]), (ctypes.c_int * len(spec))(*[d for _, d in spec])


class _Memo(object):
    """one likelihood's last (value, gradient): fmin_bfgs asks for f(x) and then f'(x) at the same x (also inside its line search); both
    come out of one factorisation, so the pair is computed once and the last one is remembered"""

    def __init__(self, likelihood):
        self.likelihood, self.key, self.pair = likelihood, None, None      # (the likelihood's name: looked up in this module at every call)

    def __call__(self, loghyper, kernel, arrays, key=(), **kwargs):
        """likelihood(kernel(exp(loghyper)), *arrays, len(loghyper), **kwargs), or the remembered pair.  arrays: X, Y (, G); key: what
        the kwargs add to the key"""
        loghyper = np.asarray(loghyper, dtype=float)
        # keyed on the CONTENT of the data (a digest: 0.1 ms at N=4096, D=16 against a 9 ms factorisation), so an
        # in-place edit of X or Y can never return the pair computed for the old data
        dig = hashlib.blake2b(_lib.rows(arrays[0]).tobytes(), digest_size=16)
        for a in arrays[1:]:
            dig.update(_lib.f64(a).tobytes())
        key = (loghyper.tobytes(), kernel, dig.digest()) + tuple(key)
        if self.key != key:
            self.key = None
            self.pair = globals()[self.likelihood](kernel(np.exp(loghyper)), *(tuple(arrays) + (len(loghyper),)), **kwargs)
            self.key = key
        return self.pair


def _or_100(name, pair):
    """pair()[0], or 100 when the matrix is not PD (trainhyper.py:99-115)"""
    try:
        return pair()[0]
    except LinAlgError as e:
        print(e)
        print('returning %s = 100' % name)
        return 100


def _gnoise_row(gnoise, D):
    """the D gradient noises: one number stands for every dimension"""
    gn = np.asarray(gnoise, dtype=float).reshape(-1)
    gn = _lib.f64(np.tile(gn, D) if len(gn) == 1 else gn)
    if len(gn) != D:
        raise ValueError("gnoise has %d entries, the data %d dimensions" % (len(gn), D))
    return gn


def _learn(model, x0, fg, unpack, refit, maxiter, bounds):
    """what the learn methods share: L-BFGS-B from x0 on fg(x) -> (value, gradient), a point where the matrix does not factor
    (LinAlgError) counting as +inf for the line search.  The point found is taken when it is an improvement, whatever stopped the search
    (L-BFGS-B reports success=False when it runs out of iterations): unpack(x) -> {attribute: value} is set on the model and refit() called,
    a failing refit putting the attributes back.  A start that does not factor, or a search that found nothing lower, leaves the model
    alone.  Returns the scipy result with .start_value, .end_value, .evaluations and .applied."""
    from scipy.optimize import minimize
    if len(x0) == 0:
        raise ValueError("nothing to learn")
    values = []

    def objective(x):
        try:
            v, g = fg(x)
        except LinAlgError:
            return np.inf, np.zeros(len(x))
        values.append(v)
        return v, g

    res = minimize(objective, x0, jac=True, method='L-BFGS-B', bounds=bounds, options=dict(maxiter=int(maxiter)))
    res.start_value = values[0] if values else float('nan')
    res.end_value = float(res.fun)
    res.evaluations = len(values)
    res.applied = bool(values) and np.isfinite(res.end_value) and res.end_value < res.start_value
    if not res.applied:
        return res
    new = unpack(np.asarray(res.x, dtype=float))
    keep = {k: getattr(model, k) for k in new}
    try:
        for k in new:
            setattr(model, k, new[k])
        refit()
    except Exception:
        for k in keep:
            setattr(model, k, keep[k])
        raise
    return res


def nlml_values(kernels, X, Y, noise=1e-3, device=None, spec=None, G=None):
    """NLML for a list of kernel objects of one class (a theta grid); NaN where K is not PD.
    spec: (ktype, rows, sf2) as Kernel._ibo_spec_rows gives them, instead of the objects.  G: refused (NotImplementedError)."""
    _no_gradient_data(G, "nlml_values")
    X = _lib.rows(X); Y = _lib.f64(Y)
    N, D = X.shape
    ktype, thetas, sf2 = _spec_rows(kernels) if spec is None else spec
    out = np.empty(len(thetas))
    dev = _lib.default_device() if device is None else device
    _lib.check(_lib.lib.ibo_nlml_grid(dev, ktype, N, D, _lib.dp(X), _lib.dp(Y), len(thetas), _lib.dp(thetas),
                                      thetas.shape[1], _lib.dp(sf2), float(noise), _lib.dp(out)))
    return out


def nlml_grid(Kernel, thetas, X, Y, noise=1e-3, device=None, G=None):
    """NLML at every row of `thetas` (hyper-parameters, NOT logs); returns (values, argmin).  G: refused (NotImplementedError)."""
    _no_gradient_data(G, "nlml_grid")
    vals = nlml_values(None, X, Y, noise, device, spec=Kernel._ibo_spec_rows(thetas))
    return vals, int(np.nanargmin(vals))


def marginalLikelihood(kernel, X, Y, nhyper, computeGradient=True, useCholesky=True, noise=1e-3, G=None):
    """negative log marginal likelihood and (optionally) its partial derivatives w.r.t.
    each log hyper-parameter (trainhyper.py:47-95).  useCholesky is accepted for
    signature compatibility; the device path always factors.  G: refused (NotImplementedError)."""
    _no_gradient_data(G, "marginalLikelihood")
    NX = len(X)
    assert NX == len(Y)
    if not computeGradient:
        v = nlml_values([kernel], X, Y, noise)[0]
        if not np.isfinite(v):
            raise LinAlgError("covariance matrix is not positive definite for hyperparameters %s"
                              % (kernel.hyperparams,))
        return v
    # value and gradient in one device call: Cholesky, L^-1, K^-1 = W^T W, then
    # dnlml_i = sum((K^-1 - alpha alpha^T) * dK/dtheta_i) / 2   (:70-71)
    Xa = _lib.rows(X); Ya = _lib.f64(Y)
    N, D = Xa.shape
    ktype, hyper, sf2, _ = kernel._ibo_spec()
    modes, dims = _grad_spec(kernel, D, nhyper)
    v = ctypes.c_double()
    g = np.empty(nhyper)
    try:
        _lib.check(_lib.lib.ibo_nlml_grad(_lib.default_device(), ktype, N, D, _lib.dp(Xa), _lib.dp(Ya), _lib.dp(hyper),
                                          len(hyper), sf2, float(noise), nhyper, modes, dims, ctypes.byref(v), _lib.dp(g)))
    except _lib.NotPositiveDefinite:
        raise LinAlgError("covariance matrix is not positive definite for hyperparameters %s" % (kernel.hyperparams,))
    return v.value, g


_nlml_memo = _Memo('marginalLikelihood')


def nlml(loghyper, kernel, X, Y, *args):
    """NLML as a function of LOG hyper-parameters (trainhyper.py:99-115); 100 when not PD."""
    return _or_100('nlml', lambda: _nlml_memo(loghyper, kernel, (X, Y)))


def nlmlMulti(loghyper, kernel, X, Y, *args):
    k = kernel(np.exp(loghyper))
    ml = 0.0
    for x, y in zip(X, Y):
        ml += marginalLikelihood(k, x, y, len(loghyper))[0]
    return ml


def dnlml(loghyper, kernel, X, Y):
    return _nlml_memo(loghyper, kernel, (X, Y))[1]


# ---------------------------------------------------------------------------------------- leave-one-out cross-validation
def looLikelihood(kernel, X, Y, nhyper, computeGradient=True, noise=1e-3, predictions=False, G=None):
    """the leave-one-out objective  sum_i [log(s2_-i) / 2 + (Y_i - mu_-i)^2 / (2 s2_-i) + log(2 pi) / 2]  of K = covMatrix + noise I
    (to be minimised, like marginalLikelihood) and, with computeGradient, its partial derivatives w.r.t. each log hyper-parameter:
    `value` or `(value, grad)`.  predictions=True appends (mu_-i, s2_-i), the leave-one-out predictions at this theta, as a
    last element.  LinAlgError when K is not positive definite.  G: refused (NotImplementedError)."""
    _no_gradient_data(G, "looLikelihood")
    assert len(X) == len(Y)
    Xa = _lib.rows(X); Ya = _lib.f64(Y)
    N, D = Xa.shape
    ktype, hyper, sf2, _ = kernel._ibo_spec()
    modes = dims = None
    g = None
    if computeGradient:
        modes, dims = _grad_spec(kernel, D, nhyper)
        g = np.empty(nhyper)
    mu = np.empty(N) if predictions else None
    s2 = np.empty(N) if predictions else None
    v = ctypes.c_double()
    try:
        _lib.check(_lib.lib.ibo_loo_grad(_lib.default_device(), ktype, N, D, _lib.dp(Xa), _lib.dp(Ya), _lib.dp(hyper), len(hyper), sf2,
                                         float(noise), nhyper if computeGradient else 0, modes, dims, ctypes.byref(v),
                                         _lib.dp(g) if computeGradient else None, _lib.dp(mu) if predictions else None,
                                         _lib.dp(s2) if predictions else None))
    except _lib.NotPositiveDefinite:
        raise LinAlgError("covariance matrix is not positive definite for hyperparameters %s" % (kernel.hyperparams,))
    out = (v.value, g) if computeGradient else (v.value,)
    if predictions:
        out = out + ((mu, s2),)
    return out if len(out) > 1 else out[0]


_loo_memo = _Memo('looLikelihood')


def nloo(loghyper, kernel, X, Y, noise=1e-3):
    """the leave-one-out objective as a function of LOG hyper-parameters, for fmin_bfgs; 100 when not PD (as nlml)"""
    return _or_100('nloo', lambda: _loo_memo(loghyper, kernel, (X, Y), (float(noise),), noise=noise))


def dnloo(loghyper, kernel, X, Y, noise=1e-3):
    return _loo_memo(loghyper, kernel, (X, Y), (float(noise),), noise=noise)[1]


# ---------------------------------------------------------------------------------------- the sparse (inducing-point) model
def sparseLikelihood(kernel, X, Y, Z, nhyper, noise, jitter=1e-6, kind='vfe', computeGradient=True, gradZ=True):
    """the negative log marginal likelihood of the sparse GP on the inducing points Z (kind 'fitc' or 'dtc'), or Titsias' bound
    (kind 'vfe'), and with computeGradient its partial derivatives: `value` or `(value, grad_loghyper, grad_lognoise, grad_Z)` -- with
    respect to the log of the kernel's first nhyper hyper-parameters, the log noise and (gradZ, else None) every coordinate of every
    inducing point.  One device call (ibo_sgp_nlml_grad).  LinAlgError when K~uu or A is not positive definite."""
    from .sparse import nlml_grad_raw
    assert len(X) == len(Y)
    want = () if not computeGradient else (('hyper', 'noise', 'Z') if gradZ else ('hyper', 'noise'))
    try:
        v, g = nlml_grad_raw(kernel, X, Y, Z, noise, jitter, kind, ngrad=nhyper, want=want)
    except _lib.NotPositiveDefinite:
        raise LinAlgError("the sparse model's matrices are not positive definite for hyperparameters %s" % (kernel.hyperparams,))
    if not computeGradient:
        return v
    return v, g['hyper'], g['noise'], g.get('Z')


# ---------------------------------------------------------------------------------------- the model observed with gradients
def gradientLikelihood(kernel, X, Y, G, nhyper, noise=1e-3, gnoise=1e-4, computeGradient=True, gradNoise=False):
    """the negative log marginal likelihood of the N (D + 1)-row model of values Y and slopes G (GaussianProcess(kernel, X, Y, G=G)) with
    A = C + diag(noise, gnoise_1 .. gnoise_D) per point, C the derivative covariance with the kernel's own diagonal (marginalLikelihood's
    convention, covMatrix + noise I: for a signal variance other than 1 the fitted model's value rows hold 1 + noise instead), and with
    computeGradient its exact partial derivatives: `value`, `(value, grad_loghyper)` or, with gradNoise, `(value, grad_loghyper,
    grad_lognoise, grad_loggnoise)` -- w.r.t. the log of the kernel's first nhyper hyper-parameters, the log noise and the log of each
    of the D gradient noises.  gnoise: one number or one per dimension.  One device call (ibo_ggp_nlml_grad).  LinAlgError when A is
    not positive definite, ValueError for G.shape != X.shape."""
    Xa = _lib.rows(X); Ya = _lib.f64(Y).reshape(-1)
    Ga = _lib.f64(np.array(G, dtype=float, ndmin=2))
    if Ga.shape != Xa.shape:
        raise ValueError("G has shape %s, X has %s: one partial derivative per coordinate of every point" % (Ga.shape, Xa.shape))
    assert len(Xa) == len(Ya)
    N, D = Xa.shape
    gn = _gnoise_row(gnoise, D)
    ktype, hyper, sf2, _ = kernel._ibo_spec()
    modes = dims = None
    g = None
    if computeGradient:
        modes, dims = _grad_spec(kernel, D, nhyper)
        g = np.empty(nhyper)
    gnz = np.empty(D + 1) if computeGradient and gradNoise else None
    v = ctypes.c_double()
    try:
        _lib.check(_lib.lib.ibo_ggp_nlml_grad(_lib.default_device(), ktype, N, D, _lib.dp(Xa), _lib.dp(Ya), _lib.dp(Ga), _lib.dp(hyper),
                                              len(hyper), sf2, float(noise), _lib.dp(gn), nhyper if computeGradient else 0, modes, dims,
                                              ctypes.byref(v), None if g is None or nhyper == 0 else _lib.dp(g),      # (nhyper = 0: the noise terms alone)
                                              None if gnz is None else _lib.dp(gnz)))
    except _lib.NotPositiveDefinite:
        raise LinAlgError("the gradient-observation matrix is not positive definite for hyperparameters %s" % (kernel.hyperparams,))
    if not computeGradient:
        return v.value
    return (v.value, g, gnz[0], gnz[1:].copy()) if gradNoise else (v.value, g)


_g_memo = _Memo('gradientLikelihood')


def _g_value_and_grad(loghyper, kernel, X, Y, G, noise, gnoise):
    return _g_memo(loghyper, kernel, (X, Y, G), (float(noise), _lib.f64(np.asarray(gnoise, dtype=float).reshape(-1)).tobytes()),
                   noise=noise, gnoise=gnoise)


def ngnlml(loghyper, kernel, X, Y, G, noise=1e-3, gnoise=1e-4):
    """gradientLikelihood as a function of LOG hyper-parameters, for fmin_bfgs; 100 when not PD (as nlml)"""
    return _or_100('ngnlml', lambda: _g_value_and_grad(loghyper, kernel, X, Y, G, noise, gnoise))


def dgnlml(loghyper, kernel, X, Y, G, noise=1e-3, gnoise=1e-4):
    return _g_value_and_grad(loghyper, kernel, X, Y, G, noise, gnoise)[1]

"""
Pathwise posterior draws (Matheron's rule with a random-Fourier-feature prior; Wilson et al. 2020): Thompson sampling that scales
with the rest of the library.  GaussianProcess.sample_posterior draws at M given points by factoring their M x M covariance; a
draw made here is a FUNCTION

    path_s(x) = mu(x) + phi(x).w_s - k*(x)^T A^-1 (Phi(X) w_s + eps_s),     phi_j(x) = sqrt(2 sf2 / F) cos(omega_j.x + b_j)

that can be evaluated anywhere afterwards: swept over a candidate array of any length (with an arg-max per path), sharded with
index_base, or handed to DIRECT.  The reference has nothing like it.

    spectralDraws(kernel, D, n_features, n_paths, N, eps_var, seed) -> (omega, phase, w, eps)
    PosteriorPaths(GP, n_paths=8, n_features=2048, seed=None)   .values(X) .sweep(candidates) .maximize(bounds, path) .coef() .close()
        .gradient(X, paths=None) -> (values, gradients)   .negf_grad(x, path) -> (-value, -gradient)   (ibo_paths_grad_batch)
        .maximize(..., polish=True): a bounded L-BFGS-B finish from DIRECT's point on the exact gradient
        .maxima(bounds, candidates=None, polish=True) -> (vals (S,), X (S, D)): every path's maximum, ascended in lock-step

Conventions of the Python classes: k and k* with the kernel's own sf2; mu is GP.posterior's mean, the mean prior included.  The
paths are draws of the LATENT function (sample_posterior(noise=False)); their covariance matches posterior_cov(noise=False) off the
diagonal and sf2 - |v|^2 on it, with an error of the random features that falls as 1 / sqrt(n_features).  A PosteriorPaths object
is a snapshot on the device: it stays what it is when the model gets more data, loses some or is deleted.  A value is the same bits
from values, sweep and maximize.  Everything is computed by libibo_hip (ibo_paths_*).

Not provided: exclusion balls, PrefGaussianProcess and models with an augmented factor
(NotImplementedError: the matrix they were factored from differs from K by more than a diagonal).
"""
import ctypes

import numpy as np

from .. import _lib
from ..utils.latinhypercube import lhcSample
from . import _args

MAX_PATHS = 256           # IBO_PATHS_MAX_PATHS
MAX_FEATURES = 16384      # IBO_PATHS_MAX_FEATURES
MAXIMA_CANDIDATES = 4096  # maxima's default starts: the arg-maxes of a sweep over this many latin-hypercube points


def spectralDraws(kernel, D, n_features, n_paths, N, eps_var, seed=None):
    """The random arrays of `n_paths` paths on a model of N rows in D dimensions: (omega (F, D), phase (F,), w (S, F), eps (S, N)).

    One generator, rng = np.random.default_rng(seed), asked in this order (the same seed gives the same arrays):
      1. z     = rng.standard_normal((F, D))
      2. gamma = rng.chisquare(2 nu, F)             -- Matern kernels only (2 nu = 3 or 5)
      3. phase = rng.uniform(0, 2 pi, F)
      4. w     = rng.standard_normal((S, F))
      5. eps   = sqrt(eps_var) * rng.standard_normal((S, N))
    omega = z / theta for the squared exponentials (theta per dimension for the ARD kernels), z / theta * sqrt(2 nu / gamma) for the
    Matern kernels (the multivariate Student-t spectral density); theta as kernel._ibo_spec() returns it."""
    F, S, N, D = int(n_features), int(n_paths), int(N), int(D)
    if not 1 <= F <= MAX_FEATURES:
        raise ValueError("between 1 and %d features" % MAX_FEATURES)
    if not 1 <= S <= MAX_PATHS:
        raise ValueError("between 1 and %d paths" % MAX_PATHS)
    if not eps_var >= 0:
        raise ValueError("eps_var = %r: the paths need 1 + noise >= sf2" % (eps_var,))
    ktype, hyper = kernel._ibo_spec()[:2]
    theta = np.asarray(hyper, dtype=float).reshape(-1)
    if ktype == _lib.K_SE_ARD and len(theta) != D:
        raise ValueError("the kernel has %d length scales, the data %d dimensions" % (len(theta), D))
    rng = np.random.default_rng(seed)
    omega = rng.standard_normal((F, D)) / (theta[None, :] if ktype == _lib.K_SE_ARD else theta[0])
    if ktype in (_lib.K_MATERN3, _lib.K_MATERN5):
        nu2 = 3.0 if ktype == _lib.K_MATERN3 else 5.0
        omega = omega * np.sqrt(nu2 / rng.chisquare(nu2, F))[:, None]
    phase = rng.uniform(0.0, 2.0 * np.pi, F)
    w = rng.standard_normal((S, F))
    eps = np.sqrt(float(eps_var)) * rng.standard_normal((S, N))
    return _lib.f64(omega), _lib.f64(phase), _lib.f64(w), _lib.f64(eps)


class PosteriorPaths(object):
    """`n_paths` posterior draws of GP as functions, from `n_features` random Fourier features; seed fixes them"""

    def __init__(self, GP, n_paths=8, n_features=2048, seed=None):
        from ..gaussianprocess import PrefGaussianProcess
        self._h = None
        if isinstance(GP, PrefGaussianProcess):
            raise NotImplementedError("pathwise draws of a preference GP: its factor is of R + C^-1, which differs from K by more than a diagonal")
        if getattr(GP, "_augdev", None) is not None:
            raise NotImplementedError("pathwise draws on an augmented factor (addObservationPoint)")
        if len(GP.X) == 0:
            raise ValueError("model has no data")
        _args._no_gradient(GP, "pathwise posterior draws (PosteriorPaths)")
        N, D = np.asarray(GP.X).shape
        sf2 = GP.kernel._ibo_spec()[2]
        eps_var = 1.0 + float(GP.noise) - sf2
        if eps_var < 0:
            raise ValueError("1 + noise - sf2 = %g < 0: the model's diagonal is below its kernel's, no path has this posterior" % eps_var)
        self.omega, self.phase, self.w, self.eps = spectralDraws(GP.kernel, D, n_features, n_paths, N, eps_var, seed)
        self.S, self.F, self.N, self.D = int(n_paths), int(n_features), N, D
        self.seed = seed
        self.device = GP._dev.device if GP._dev is not None else _lib.default_device()
        GP._push_prior()
        h = ctypes.c_void_p()
        _lib.check(_lib.lib.ibo_paths_create(GP._handle(), self.F, _lib.dp(self.omega), _lib.dp(self.phase), self.S, _lib.dp(self.w),
                                             _lib.dp(self.eps), ctypes.byref(h)))
        self._h = h

    def _points(self, X, what):
        P = _lib.f64(np.atleast_2d(np.asarray(X, dtype=float)))
        if P.ndim != 2 or P.shape[1] != self.D or len(P) < 1:
            raise ValueError("%s must be (M, %d) points, got shape %s" % (what, self.D, P.shape))
        return P

    def _handle(self):
        if self._h is None:
            raise ValueError("the paths have been closed")
        return self._h

    def values(self, X):
        """(S, M): every path at the points X ((M, D), or (D,) for one point)"""
        Q = self._points(X, "X")
        out = np.empty((self.S, len(Q)))
        _lib.check(_lib.lib.ibo_paths_batch(self._handle(), len(Q), _lib.dp(Q), _lib.dp(out)))
        return out

    def sweep(self, candidates, index_base=0, outputs=False):
        """Every path over a whole candidate array (an (M, D) ndarray, uploaded, or a _lib.DeviceArray already in HBM) and its
        arg-max: dict(best_val (S,), best_idx (S,)[, values (S, M)]).  Per path the first maximiser wins ties and NaN never wins;
        index_base is added to the index, which is -1 (with -inf) where no value is a number."""
        cand = candidates if isinstance(candidates, _lib.DeviceArray) else _lib.DeviceArray.from_host(self._points(candidates, "candidates"),
                                                                                                     self.device)
        if len(cand.shape) != 2 or cand.shape[1] != self.D:
            raise ValueError("candidates must be (M, %d) points, got shape %s" % (self.D, cand.shape))
        M = cand.shape[0]
        vals = _lib.DeviceArray((self.S, M), self.device) if outputs else None
        bv = np.empty(self.S); bi = np.empty(self.S, dtype=np.int64)
        _lib.check(_lib.lib.ibo_paths_sweep(self._handle(), M, cand.ptr, int(index_base), vals.ptr if outputs else None, _lib.dp(bv),
                                            bi.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))))
        res = dict(best_val=bv, best_idx=bi)
        if outputs:
            res["values"] = vals.to_host()
        return res

    def gradient(self, X, paths=None):
        """values and gradients with respect to x at the points X ((M, D), or (D,) for one point), one ibo_paths_grad_batch call:
        (S, M) and (S, M, D) for every path, or -- with `paths` an int array of length M -- (M,) and (M, D): path paths[i] at point i.
        The values are values(X)'s, bit for bit."""
        Q = self._points(X, "X")
        M = len(Q)
        if paths is None:
            po, val, grad = None, np.empty((self.S, M)), np.empty((self.S, M, self.D))
        else:
            po = np.ascontiguousarray(np.asarray(paths).reshape(-1), dtype=np.intc)
            if len(po) != M or not np.array_equal(po, np.asarray(paths).reshape(-1)):
                raise ValueError("paths must be %d integers, one per point" % M)
            if np.any(po < 0) or np.any(po >= self.S):
                raise ValueError("a path outside [0, %d)" % self.S)
            val, grad = np.empty(M), np.empty((M, self.D))
        _lib.check(_lib.lib.ibo_paths_grad_batch(self._handle(), M, _lib.dp(Q), None if po is None else po.ctypes.data_as(ctypes.POINTER(ctypes.c_int)),
                                                 _lib.dp(val), _lib.dp(grad)))
        return val, grad

    def negf_grad(self, x, path=0):
        """(-value, -gradient) of one path at one point, for scipy.optimize.minimize(jac=True)"""
        if not 0 <= int(path) < self.S:
            raise ValueError("path %r outside [0, %d)" % (path, self.S))
        v, g = self.gradient(np.asarray(x, dtype=float).reshape(1, self.D), paths=[int(path)])
        return -v[0], -g[0]

    def _box(self, bounds):
        lb = _lib.f64([b[0] for b in bounds]); ub = _lib.f64([b[1] for b in bounds])
        if len(lb) != self.D:
            raise ValueError("bounds have %d dimensions, the paths have %d" % (len(lb), self.D))
        return lb, ub

    def maximize(self, bounds, path=0, maxiter=50, maxtime=30, maxsample=10000, compat=False, polish=False):
        """Maximise one path over the box `bounds` with DIRECT on the GPU objective (ibo_paths_direct_max) -> (opt, optx);
        opt is values(optx)[path], bit for bit.  polish=True: bounded L-BFGS-B from DIRECT's point on negf_grad, at most
        POLISH_MAXITER iterations; the end point is re-evaluated with values and kept only when strictly better."""
        lb, ub = self._box(bounds)
        if not 0 <= int(path) < self.S:
            raise ValueError("path %r outside [0, %d)" % (path, self.S))
        opt = ctypes.c_double(); optx = np.empty(self.D); ns = ctypes.c_int64()
        _lib.check(_lib.lib.ibo_paths_direct_max(self._handle(), int(path), self.D, _lib.dp(lb), _lib.dp(ub), int(maxiter), int(maxtime),
                                                 int(maxsample), 1 if compat else 0, ctypes.byref(opt), _lib.dp(optx), ctypes.byref(ns)))
        if not polish:
            return opt.value, optx
        return _args._polish_step(lambda x: self.negf_grad(x, path), lambda x: self.values(x)[int(path), 0], lb, ub, opt.value, optx)

    def _ascend(self, X0, bounds):
        """Every path s ascended from its own start X0[s] inside the box, all S in lock-step: projected gradient steps with a
        Barzilai-Borwein length and backtracking, each iteration ONE ibo_paths_grad_batch call on the S trial points (path s at
        point s), at most POLISH_MAXITER of them.  A trial point is accepted when its value is strictly greater; a path whose
        step is refused halves it.  Returns (vals (S,), X (S, D)).  The end point is re-evaluated with values and replaces the
        start only when it is strictly better and its projected gradient is not larger than the start's; a start that is not finite
        stays as it is, with the value NaN."""
        from . import POLISH_MAXITER
        lb, ub = self._box(bounds)
        X0 = _lib.f64(np.asarray(X0, dtype=float).reshape(self.S, self.D))
        own = np.arange(self.S)
        live = np.all(np.isfinite(X0), axis=1)
        x = np.where(live[:, None], np.clip(X0, lb, ub), lb[None, :])             # (a dead path rides along at a corner, unread)

        def projected(x, g):                                                      # the gradient without what points out of the box
            return np.where(((x <= lb) & (g < 0)) | ((x >= ub) & (g > 0)), 0.0, g)

        f, g = self.gradient(x, paths=own)
        live &= np.isfinite(f) & np.all(np.isfinite(g), axis=1)
        g = np.where(live[:, None], g, 0.0)                                       # (a dead path does not move)
        x0, f0, pg0 = x.copy(), f.copy(), np.linalg.norm(projected(x, g), axis=1)
        diag = float(np.linalg.norm(ub - lb))

        def capped(step, g):                                                      # no step longer than the box
            gn = np.linalg.norm(g, axis=1)
            return np.where(gn > 0, np.minimum(step, diag / np.where(gn > 0, gn, 1.0)), 0.0)

        step = capped(np.full(self.S, np.inf), g) * .05                           # a first move of 5% of the box's diagonal
        for _ in range(POLISH_MAXITER - 1):
            xt = np.clip(x + step[:, None] * g, lb, ub)
            ft, gt = self.gradient(xt, paths=own)
            ok = live & (ft > f) & np.all(np.isfinite(gt), axis=1)
            dx, dg = xt - x, gt - g
            sy = -np.sum(dx * dg, axis=1)                                         # (> 0 where the path is concave along the step)
            bb = np.where(sy > 0, np.sum(dx * dx, axis=1) / np.where(sy > 0, sy, 1.0), 2.0 * step)
            x = np.where(ok[:, None], xt, x); f = np.where(ok, ft, f); g = np.where(ok[:, None], gt, g)
            step = capped(np.where(ok, bb, .5 * step), g)
        x = _lib.f64(x)
        val = self.values(x)[own, own]
        pg = np.linalg.norm(projected(x, g), axis=1)
        keep = live & (val > f0) & (pg <= pg0)
        dead = ~np.all(np.isfinite(X0), axis=1)
        X = np.where(keep[:, None], x, np.where(dead[:, None], X0, x0))
        return np.where(keep, val, np.where(dead, np.nan, f0)), X

    def maxima(self, bounds, candidates=None, polish=True):
        """(vals (S,), X (S, D)): every path's maximum over the box.  The starts are the per-path arg-maxes of one sweep over
        `candidates` (an (M, D) ndarray or a _lib.DeviceArray; default: a seeded latin hypercube of MAXIMA_CANDIDATES points in
        `bounds`); polish=True ascends all S from there in lock-step (_ascend).  vals[s] is values(X[s])[s], bit for bit, and never
        below the sweep's; a path whose sweep had no finite value returns (-inf, a row of NaN)."""
        lb, ub = self._box(bounds)
        if candidates is None:
            candidates = np.array(lhcSample([list(b) for b in zip(lb, ub)], MAXIMA_CANDIDATES, seed=0 if self.seed is None else self.seed))
        dev = isinstance(candidates, _lib.DeviceArray)
        C = candidates if dev else self._points(candidates, "candidates")
        r = self.sweep(C)
        vals, X = np.array(r["best_val"]), np.full((self.S, self.D), np.nan)
        for s, k in enumerate(r["best_idx"]):
            if k >= 0:
                X[s] = C.view_rows(int(k), int(k) + 1).to_host()[0] if dev else C[int(k)]
            else:
                vals[s] = -np.inf
        if not polish or not np.any(r["best_idx"] >= 0):
            return vals, X
        pv, pX = self._ascend(X, bounds)
        found = r["best_idx"] >= 0
        better = found & (pv > vals)
        return np.where(better, pv, vals), np.where(better[:, None], pX, X)

    def coef(self):
        """(S, F + N): per path the feature weights w_s, then the kernel weights c_s, as the device holds them"""
        out = np.empty((self.S, self.F + self.N))
        _lib.check(_lib.lib.ibo_paths_coef(self._handle(), _lib.dp(out)))
        return out

    def close(self):
        if getattr(self, "_h", None) is not None:
            try:
                _lib.lib.ibo_paths_destroy(self._h)
            except Exception:
                pass
            self._h = None

    def __del__(self):
        self.close()

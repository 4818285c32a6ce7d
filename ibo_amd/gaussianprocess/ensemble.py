"""
An ensemble of plain GP models on the same data under several hyper-parameter samples: the model behind the integrated acquisitions
(acquisition.integrated; Snoek, Larochelle & Adams 2012).  The reference has nothing like it.

    GaussianProcessEnsemble(kernels, X, Y, noise=1e-3, weights=None, prior=None)
        .members  .weights (normalised to sum 1)  .X  .Y
        .addData(X, Y)            appends and refits every member: the bits of an ensemble built on all the data at once
        .posterior(x)  .posteriors(X)      the mixture's (mean, var) (ibo_iacq_batch)
        .resample(**sampleHyper_args)      replaces the members by a new draw
    GaussianProcessEnsemble.sample(kernel, X, Y, n=8, **sampleHyper_args)      the ensemble of hypersample.sampleHyper's draws

Every member is a GaussianProcess as it stands -- its own handle, its own stream, its own behaviour; the ensemble adds the list, the
weights and the calls that take all the handles at once.  At most 32 members (IBO_IACQ_MAX).  With (mu_s, s2_s) member s's posterior:

    mean = sum_s w_s mu_s          var = sum_s w_s (s2_s + (mu_s - mean)^2)          (sum_s w_s = 1)

Preference models, models observed with gradients (G=) and sparse models are refused as members (NotImplementedError).
"""
import ctypes
import warnings

import numpy as np

from .. import _lib
from . import GaussianProcess, PrefGaussianProcess, LinAlgError
from . import hypersample

MAX_MEMBERS = 32             # IBO_IACQ_MAX

_ENSEMBLE_WHY = ("an ensemble holds plain GaussianProcess members: the integrated entries (ibo_iacq_*) sweep ibo_gp_t handles of "
                 "value observations, and neither a preference model's latent values nor the N (D + 1)-row or inducing-point models "
                 "have a per-theta refit here")


def _refuse(what):
    raise NotImplementedError("%s: not available, %s" % (what, _ENSEMBLE_WHY))


def _check_member(m):
    """refuse by name what an ensemble cannot hold"""
    if isinstance(m, PrefGaussianProcess):
        _refuse("a PrefGaussianProcess member")
    if getattr(m, "_kind", "gp") == 'sgp':
        _refuse("a sparse (SparseGaussianProcess) member")
    if getattr(m, "G", None) is not None:
        _refuse("a member observed with gradients (G=)")
    if not isinstance(m, GaussianProcess):
        raise TypeError("an ensemble member must be a GaussianProcess, not %s" % type(m).__name__)


class GaussianProcessEnsemble(object):

    def __init__(self, kernels, X, Y, noise=1e-3, weights=None, prior=None, G=None, device=None):
        if G is not None:
            _refuse("GaussianProcessEnsemble(G=)")
        kernels = list(kernels)
        if not 1 <= len(kernels) <= MAX_MEMBERS:
            raise ValueError("an ensemble has 1 .. %d members, not %d" % (MAX_MEMBERS, len(kernels)))
        self.noise = noise
        self.prior = prior
        self._device = device
        self._sample_args = None
        self._set_members([GaussianProcess(k, X, Y, prior=prior, noise=noise, device=device) for k in kernels], weights)

    @classmethod
    def from_members(cls, members, weights=None):
        """an ensemble of models that exist already (plain, fitted, on the same data)"""
        members = list(members)
        if not 1 <= len(members) <= MAX_MEMBERS:
            raise ValueError("an ensemble has 1 .. %d members, not %d" % (MAX_MEMBERS, len(members)))
        self = object.__new__(cls)
        self.noise = members[0].noise
        self.prior = members[0].prior
        self._device = members[0]._device
        self._sample_args = None
        self._set_members(members, weights)
        return self

    def _set_members(self, members, weights):
        for m in members:
            _check_member(m)
            if len(m.X) == 0:
                raise ValueError("an ensemble member has no data")
        w = np.ones(len(members)) if weights is None else np.array(weights, dtype=float).reshape(-1)
        if len(w) != len(members):
            raise ValueError("%d weights for %d members" % (len(w), len(members)))
        if not np.all(np.isfinite(w)) or np.any(w < 0) or not np.sum(w) > 0:
            raise ValueError("the weights must be finite and >= 0, one of them > 0")
        self.members = members
        self.weights = w / np.sum(w)

    # ------------------------------------------------------------------ what the members share
    @property
    def X(self):
        return self.members[0].X

    @property
    def Y(self):
        return self.members[0].Y

    @property
    def kernels(self):
        return [m.kernel for m in self.members]

    def __len__(self):
        return len(self.members)

    def _pack(self):
        """(handles, S, weights) as the ibo_iacq_* entries take them; every member's prior is pushed"""
        for m in self.members:
            _check_member(m)                         # (a member may have been given gradient data since)
            m._handle()
            m._push_prior()
        S = len(self.members)
        self._w = _lib.f64(self.weights)
        return (ctypes.c_void_p * S)(*[m._handle() for m in self.members]), S, _lib.dp(self._w)

    # ------------------------------------------------------------------ the model's calls
    def addData(self, X, Y, G=None):
        """append observations and fit every member again on all the data, so that an ensemble is a function of its data alone: grown
        point by point it is, bit for bit, the ensemble built on the same data at once.  (GaussianProcess.addData extends a factor in
        place, which agrees with a fit to rounding only; the members of an ensemble are replaced by resample() every few observations
        anyway, and at 1024 rows a fit costs about two extension steps.)  A member whose matrix does not factor leaves the whole ensemble
        as it was: LinAlgError."""
        if G is not None:
            _refuse("GaussianProcessEnsemble.addData(G=)")
        X = np.array(X, dtype=float, ndmin=2)
        Y = np.array(Y, dtype=float, ndmin=1).flatten()
        if len(Y) != len(X) or X.shape[1] != np.asarray(self.X).shape[1]:
            raise ValueError("addData takes (n, %d) points and n values, got %s and %s" % (np.asarray(self.X).shape[1], X.shape, Y.shape))
        for m in self.members:
            _check_member(m)
        old = [(m.X, m.Y) for m in self.members]
        done = []
        try:
            for m, (X0, Y0) in zip(self.members, old):
                m.refit(np.r_[X0, X], np.r_[Y0, Y])  # (a member whose fit fails is back on its old data when this raises)
                done.append(m)
        except Exception:
            for m, (X0, Y0) in zip(done, old):
                m.refit(X0, Y0)
            raise

    def _mixture(self, Q):
        Q = _lib.f64(np.atleast_2d(np.asarray(Q, dtype=float)))
        M = len(Q)
        mean, var = np.empty(M), np.empty(M)
        gp, S, w = self._pack()
        _lib.check(_lib.lib.ibo_iacq_batch(gp, S, w, M, _lib.dp(Q), _lib.ACQ_NONE, 0.0, _lib.ERF_NR, _lib.CLAMP_PY, float('nan'),
                                           None, _lib.dp(mean), _lib.dp(var)))
        return mean, var

    def posterior(self, x, getvar=True):
        """the mixture's mean (and variance) at ONE point"""
        mean, var = self._mixture(np.array(x, dtype=float, ndmin=2)[:1])
        return (mean[0], var[0]) if getvar else mean[0]

    def posteriors(self, X):
        """arrays of the mixture's means and variances -- one call"""
        return self._mixture(np.array([np.atleast_1d(np.asarray(x, dtype=float)) for x in X]))

    def mu(self, x):
        return self.posterior(x, getvar=False)

    # ------------------------------------------------------------------ from samples of the hyper-parameters
    @classmethod
    def sample(cls, kernel, X, Y, n=8, noise=1e-3, prior=None, mean_prior=None, **sampleHyper_args):
        """the ensemble of n draws of hypersample.sampleHyper(kernel, X, Y, n=n, noise=noise, prior=prior, **sampleHyper_args), equally
        weighted; prior is the sampler's (over log theta), mean_prior the members' mean prior.  A draw whose fit is not positive definite
        is dropped with a warning; ValueError when none is left."""
        if isinstance(kernel, (list, tuple)):
            raise TypeError("sample takes one kernel object: its class and hyper-parameters are the sampler's start")
        if n > MAX_MEMBERS:
            raise ValueError("an ensemble has at most %d members" % MAX_MEMBERS)
        self = object.__new__(cls)
        self.noise = noise
        self.prior = mean_prior
        self._device = sampleHyper_args.pop("device", None)
        self._sample_args = dict(kernel=kernel, n=n, prior=prior, args=dict(sampleHyper_args))
        self._draw(X, Y)
        return self

    def _draw(self, X, Y):
        a = self._sample_args
        kernel = a["kernel"]
        # (the grid that scores the draws runs where the members live)
        loghyper, logp = hypersample.sampleHyper(kernel, X, Y, n=a["n"], noise=self.noise, prior=a["prior"], device=self._device, **a["args"])
        th0 = np.asarray(kernel.hyperparams, dtype=float)
        members, kept = [], []
        for i, row in enumerate(loghyper):
            k = kernel.__class__(np.r_[np.exp(row), th0[len(row):]])
            try:
                members.append(GaussianProcess(k, X, Y, prior=self.prior, noise=self.noise, device=self._device))
                kept.append(i)
            except LinAlgError:
                warnings.warn("GaussianProcessEnsemble: the fit at hyper-parameters %s is not positive definite; the sample is dropped"
                              % (k.hyperparams,))
        if not members:
            raise ValueError("no sampled hyper-parameters gave a positive definite fit")
        self.loghyper, self.logp = loghyper[kept], logp[kept]          # (row s belongs to member s)
        self._set_members(members, None)

    def resample(self, **args):
        """replace the members by a new draw on the data as they are now; args override those of the sample() call (n=, seed=, ..).
        An ensemble that was not built by sample() needs kernel= (the sampler's start)."""
        a = dict(kernel=None, n=len(self.members), prior=None, args={}) if self._sample_args is None else dict(self._sample_args)
        a["args"] = dict(a["args"])
        for k, v in args.items():
            if k in ("kernel", "n", "prior"):
                a[k] = v
            elif k == "device":
                self._device = v
            else:
                a["args"][k] = v
        if a["kernel"] is None:
            a["kernel"] = self.members[0].kernel
        if a["n"] > MAX_MEMBERS:
            raise ValueError("an ensemble has at most %d members" % MAX_MEMBERS)
        X, Y = self.X, self.Y
        self._sample_args = a
        self._draw(X, Y)

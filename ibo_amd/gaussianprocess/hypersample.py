"""
Samples of the kernel's hyper-parameters from their posterior (Snoek, Larochelle & Adams 2012; Murray & Adams 2010), for the models
that integrate over them (ensemble.GaussianProcessEnsemble, acquisition.integrated).  The reference has nothing like it.

    sliceSample(logp_batch, x0, n, burn=20, thin=2, width=1.0, max_steps=8, seed=0) -> (samples (C, n, d), logp (C, n))
    LogNormalPrior(mean, std)     BoxPrior(lo, hi)     p * q: the product of two priors     .logpdf(phi (k, d)) -> (k,)
    sampleHyper(kernel, X, Y, nhyper=None, n=16, chains=4, burn=20, thin=2, noise=1e-3, prior=None, width=1.0, seed=0)
        -> (loghyper (n, nhyper), logp (n,))

sliceSample is univariate slice sampling with stepping-out and shrinkage (Neal 2003, figures 3 and 5), the coordinates in the fixed order
0 .. d-1, of C chains (the rows of x0) in lock-step: each chain is a small state machine (a generator) that names the one point it needs
next; every round gathers the points of the chains still running and evaluates them with ONE call logp_batch((k, d)) -> (k,).  That is
the shape the device wants: for sampleHyper a round is one ibo_nlml_grid call with one theta per active chain.  sliceSample itself is
host-only.

The draws.  Chain c draws only from numpy.random.default_rng([seed, c]) -- so a chain's samples do not depend on how many chains run
beside it -- with rng.random() alone, in this order: per sweep, per coordinate j,
    u1   the level            log y = logp(x) + log1p(-u1)
    u2   the interval         L = x_j - width u2,  R = L + width
    u3   the step budget      J = floor(max_steps u3) steps to the left at most, K = max_steps - 1 - J to the right
    then one draw per proposal of the shrinkage       x' = L + u (R - L)
The interval steps out to the left while J > 0 and logp(L) > log y, then to the right alike; a proposal is accepted when
logp(x') > log y and shrinks the interval towards x_j otherwise.  NaN and -inf count as outside the slice (no comparison with them is
true).  A coordinate whose interval has been shrunk MAX_SHRINK times keeps its value.  A sweep is one pass over the coordinates; the
first `burn` sweeps are dropped and every thin-th one after them is a sample.

The priors are densities over phi = log theta.  sampleHyper's target is  -nlml(exp phi) + log prior(phi)  with nlml from
trainhyper.nlml_values, that is with the reference's K + noise I convention (marginalLikelihood's); a theta whose matrix is not positive
definite (NaN) counts as -inf.  The noise level is not sampled.
"""
import math

import numpy as np

from .. import _lib
from . import trainhyper

MAX_SHRINK = 200


def _chain(x0, lp0, n, burn, thin, width, max_steps, rng):
    """one chain as a generator: yields the point it needs the log-density of, is sent that value, returns (samples (n, d), logp (n,))"""
    x = np.array(x0, dtype=float)
    lp = float(lp0)
    d = len(x)
    xs = np.empty((n, d)); lps = np.empty(n)
    for it in range(burn + n * thin):
        for j in range(d):
            logy = lp + math.log1p(-rng.random())
            L = x[j] - width * rng.random()
            R = L + width
            J = int(math.floor(max_steps * rng.random()))
            K = max_steps - 1 - J
            q = x.copy()
            while J > 0:
                q[j] = L
                v = yield q
                if not v > logy:
                    break
                L -= width
                J -= 1
            while K > 0:
                q[j] = R
                v = yield q
                if not v > logy:
                    break
                R += width
                K -= 1
            for _ in range(MAX_SHRINK):
                x1 = L + rng.random() * (R - L)
                q[j] = x1
                v = yield q
                if v > logy:
                    x[j] = x1
                    lp = float(v)
                    break
                if x1 < x[j]:
                    L = x1
                else:
                    R = x1
        k = it + 1 - burn
        if k > 0 and k % thin == 0:
            xs[k // thin - 1] = x
            lps[k // thin - 1] = lp
    return xs, lps


def sliceSample(logp_batch, x0, n, burn=20, thin=2, width=1.0, max_steps=8, seed=0):
    """n samples of each of C chains started at the rows of x0 (C, d) from the density exp(logp_batch); see the module's text for the
    method and the order of the draws.  logp_batch((k, d)) -> (k,) is called once per round with the points of the chains still running,
    in chain order.  Returns (samples (C, n, d), logp (C, n)): the log-density at every sample as logp_batch returned it.  ValueError when
    a start has no finite log-density."""
    x0 = np.array(x0, dtype=float, ndmin=2)
    C, d = x0.shape
    n, burn, thin, max_steps = int(n), int(burn), int(thin), int(max_steps)
    if n < 1 or burn < 0 or thin < 1 or max_steps < 1 or not width > 0:
        raise ValueError("sliceSample needs n >= 1, burn >= 0, thin >= 1, max_steps >= 1 and width > 0")
    lp0 = np.asarray(logp_batch(x0), dtype=float).reshape(-1)
    if not np.all(np.isfinite(lp0)):
        raise ValueError("chain %d starts where the log-density is not finite" % int(np.argmin(np.isfinite(lp0))))
    chains = [_chain(x0[c], lp0[c], n, burn, thin, float(width), max_steps, np.random.default_rng([int(seed), c])) for c in range(C)]
    need = {c: next(g) for c, g in enumerate(chains)}          # (n >= 1 and d >= 1: every chain asks for at least one point)
    done = {}
    while need:
        order = sorted(need)
        vals = np.asarray(logp_batch(np.array([need[c] for c in order])), dtype=float).reshape(-1)
        for c, v in zip(order, vals):
            try:
                need[c] = chains[c].send(float(v))
            except StopIteration as e:
                done[c] = e.value
                del need[c]
    return np.array([done[c][0] for c in range(C)]), np.array([done[c][1] for c in range(C)])


class _Prior(object):
    """a density over phi = log theta; p * q is their product (not normalised again)"""

    def logpdf(self, phi):
        raise NotImplementedError

    def __mul__(self, other):
        return _Product(self, other)


class _Product(_Prior):
    def __init__(self, a, b):
        self.a, self.b = a, b

    def logpdf(self, phi):
        return self.a.logpdf(phi) + self.b.logpdf(phi)


class LogNormalPrior(_Prior):
    """theta_i log-normal: phi_i = log theta_i ~ Normal(mean_i, std_i^2), independent (one number stands for every coordinate)"""

    def __init__(self, mean, std):
        self.mean = np.asarray(mean, dtype=float)
        self.std = np.asarray(std, dtype=float)
        if not np.all(self.std > 0):
            raise ValueError("std must be positive")

    def logpdf(self, phi):
        phi = np.array(phi, dtype=float, ndmin=2)
        z = (phi - self.mean) / self.std
        return np.sum(-0.5 * z * z - np.log(self.std * math.sqrt(2.0 * math.pi)), axis=1)


class BoxPrior(_Prior):
    """phi uniform on the box [lo, hi]: log density -sum log(hi - lo) inside, -inf outside"""

    def __init__(self, lo, hi):
        self.lo = np.asarray(lo, dtype=float)
        self.hi = np.asarray(hi, dtype=float)
        if not np.all(self.hi > self.lo):
            raise ValueError("hi must exceed lo")

    def logpdf(self, phi):
        phi = np.array(phi, dtype=float, ndmin=2)
        inside = np.all((phi >= self.lo) & (phi <= self.hi), axis=1)
        return np.where(inside, -np.sum(np.broadcast_to(np.log(self.hi - self.lo), phi.shape), axis=1), -np.inf)


START_JITTER = 0.1          # the chains start at log(kernel.hyperparams) + START_JITTER * standard normal draws
BOX_HALF_WIDTH = 4.0        # the default prior: a box of this half-width in log theta around the start


def _start(phi0, prior, z):
    """phi0 + START_JITTER z, the jitter halved until the prior admits the point (a start next to the edge of a box); phi0 itself after 30
    halvings"""
    scale = START_JITTER
    for _ in range(30):
        x = phi0 + scale * z
        if np.isfinite(prior.logpdf([x])[0]):
            return x
        scale *= 0.5
    return phi0.copy()


def hyperLogDensity(kernel, X, Y, nhyper=None, noise=1e-3, prior=None, device=None):
    """(logp_batch, phi0, prior): the sampler's target for the kernel's first nhyper hyper-parameters (None: all) as a function of rows of
    phi = log theta -- one ibo_nlml_grid call per batch, on `device` (None: the default device) -- the start
    log(kernel.hyperparams[:nhyper]) and the prior in force (None: BoxPrior(phi0 - 4, phi0 + 4)).  logp_batch.calls counts the grid
    calls of this target."""
    cls = kernel.__class__
    th0 = np.asarray(kernel.hyperparams, dtype=float)
    nh = len(th0) if nhyper is None else int(nhyper)
    if not 1 <= nh <= len(th0):
        raise ValueError("kernel has %d hyperparameters, %d asked for" % (len(th0), nh))
    phi0 = np.log(th0[:nh])
    if prior is None:
        prior = BoxPrior(phi0 - BOX_HALF_WIDTH, phi0 + BOX_HALF_WIDTH)
    Xa = _lib.rows(X); Ya = _lib.f64(Y)

    def logp_batch(phi):
        phi = np.array(phi, dtype=float, ndmin=2)
        lpr = np.asarray(prior.logpdf(phi), dtype=float)
        out = np.full(len(phi), -np.inf)
        ok = np.isfinite(lpr)                        # (a theta the prior excludes is not sent to the device)
        if np.any(ok):
            thetas = np.hstack([np.exp(phi[ok]), np.tile(th0[nh:], (int(np.sum(ok)), 1))])
            logp_batch.calls += 1
            v = trainhyper.nlml_values(None, Xa, Ya, noise, device, spec=cls._ibo_spec_rows(thetas))
            out[ok] = np.where(np.isfinite(v), -v + lpr[ok], -np.inf)
        return out

    logp_batch.calls = 0
    return logp_batch, phi0, prior


def sampleHyper(kernel, X, Y, nhyper=None, n=16, chains=4, burn=20, thin=2, noise=1e-3, prior=None, width=1.0, seed=0, device=None):
    """n samples of log theta for the kernel's first nhyper hyper-parameters (None: all) from  exp(-nlml(exp phi)) prior(phi),  the data
    X, Y under the kernel's class and K + noise I (marginalLikelihood's convention).  `chains` slice-sampling chains run in lock-step,
    one ibo_nlml_grid call per round with one theta per active chain; chain c starts at log(kernel.hyperparams) + 0.1 z_c, z_c the
    standard normal draws of numpy.random.default_rng([seed, c, 1]) (the 0.1 halved until the prior admits the point; a kernel whose own
    hyper-parameters the prior excludes: ValueError), and is driven by
    default_rng([seed, c]).  After burn-in the samples are taken round-robin over the chains: sample i is draw i // chains of chain
    i % chains.  prior: a LogNormalPrior, a BoxPrior or a product over log theta; None: a box of +-4 around log(kernel.hyperparams).
    device: where the grid runs (None: the default device).
    Returns (loghyper (n, nhyper), logp (n,)): logp is the target's value at each sample."""
    n, chains = int(n), int(chains)
    if n < 1 or chains < 1:
        raise ValueError("sampleHyper needs n >= 1 and chains >= 1")
    logp_batch, phi0, prior = hyperLogDensity(kernel, X, Y, nhyper, noise, prior, device)
    chains = min(chains, n)
    x0 = np.array([_start(phi0, prior, np.random.default_rng([int(seed), c, 1]).standard_normal(len(phi0))) for c in range(chains)])
    per = -(-n // chains)
    xs, lps = sliceSample(logp_batch, x0, per, burn=burn, thin=thin, width=width, seed=seed)
    # round-robin: (draw 0 of every chain, draw 1 of every chain, ..)
    loghyper = np.transpose(xs, (1, 0, 2)).reshape(per * chains, -1)[:n]
    logp = np.transpose(lps, (1, 0)).reshape(-1)[:n]
    return np.ascontiguousarray(loghyper), np.ascontiguousarray(logp)

"""
Max-value entropy search of ibo_mes_* restated in NumPy / SciPy (float64), operation by operation as include/ibo_abi.h defines it --
h, h', log Phi in the tail-safe form, the value, the gradient's sums, the gradient, the max-value cdf and the Gumbel fit -- on the
posteriors of tests/cacq_reference.py; and the same quantities in mpmath, the truth the restatement is pinned to by
tests/test_mes_reference.py.  The yardstick of tests/test_gpu_mes.py.

    v = max(s2 - s2_offset, clamp_lo),  sigma = sqrt(v),  gamma_k = (y*_k - mu) / sigma            y* ascending
    g >= 0:  q = erfc(g / sqrt 2) / 2,   lambda = phi(g) / (1 - q),     nll = -log1p(-q)
    g <  0:  e = erfcx(-g / sqrt 2),     lambda = sqrt(2 / pi) / e,     nll = g^2 / 2 - log(e / 2)         (nll = -log Phi)
    h = g lambda / 2 + nll,   T = |g lambda / 2| + |nll|                    h' = -(lambda / 2) (1 + g^2 + g lambda),  T' = (lambda / 2) (1 + g^2 + |g lambda|)
    MES = (sum_k h(gamma_k)) / K,  G_mu = -((sum_k h'_k) / K) / sigma,  G_sigma = -((sum_k h'_k gamma_k) / K) / sigma
    grad MES = G_mu dmu + G_sigma ds2 / (2 sigma)                           (ds2 = 0 where the sweep's clip or the floor of v is active)
"""
import mpmath
import numpy as np
from scipy.special import erfc, erfcx

import cacq_reference as cr

MAX_SAMPLES, MAX_LEVELS = 1024, 64


def terms(g):
    """(lambda, nll) at g (array), each branch's operations as the kernel's"""
    g = np.asarray(g, dtype=float)
    pos = g >= 0.0
    gp, gn = np.where(pos, g, 0.0), np.where(pos, -1.0, g)          # (each branch on harmless arguments where it is not taken)
    with np.errstate(all="ignore"):
        q = 0.5 * erfc(gp / np.sqrt(2.0))
        lam_p = (np.exp(-(gp * gp / 2.0)) / np.sqrt(2.0 * np.pi)) / (1.0 - q)
        nll_p = -np.log1p(-q)
        e = erfcx(-gn / np.sqrt(2.0))
        lam_n = np.sqrt(2.0 / np.pi) / e
        nll_n = gn * gn / 2.0 - np.log(e / 2.0)
    return np.where(pos, lam_p, lam_n), np.where(pos, nll_p, nll_n)


def h(g):
    """(h, T) at g"""
    g = np.asarray(g, dtype=float)
    lam, nll = terms(g)
    a = g * lam / 2.0
    return a + nll, np.abs(a) + np.abs(nll)


def dh(g):
    """(h', T') at g"""
    g = np.asarray(g, dtype=float)
    lam, _ = terms(g)
    return -(lam / 2.0) * (1.0 + g * g + g * lam), (lam / 2.0) * (1.0 + g * g + np.abs(g * lam))


def logcdf(g):
    return -terms(g)[1]


def sigma_of(s2, s2_offset, clamp_lo):
    """(sigma, follows): follows is False where the floor of v is active"""
    v = np.asarray(s2, dtype=float) - s2_offset
    floored = v < clamp_lo
    return np.sqrt(np.where(floored, clamp_lo, v)), ~floored


def from_posterior(mu, s2, ystar, s2_offset=0.0, clamp_lo=1e-8):
    """dict(val, T, gmu, gsig, sig, follows, amu, asig, gmin, gmax) over the candidates, the sums in the kernel's order (y* ascending);
    T: the mean of the terms' magnitudes; amu, asig: G_mu, G_sigma summed over the magnitudes T' of their terms"""
    ys = np.sort(np.asarray(ystar, dtype=float).reshape(-1))
    K = len(ys)
    mu = np.asarray(mu, dtype=float)
    sig, follows = sigma_of(s2, s2_offset, clamp_lo)
    z = np.zeros_like(mu)
    s, T, sd, sdg, ad, adg = z.copy(), z.copy(), z.copy(), z.copy(), z.copy(), z.copy()
    gmin, gmax = z + np.inf, z - np.inf
    for k in range(K):
        g = (ys[k] - mu) / sig
        hk, Tk = h(g)
        dk, Dk = dh(g)
        s = s + hk
        T = T + Tk
        sd = sd + dk
        sdg = sdg + dk * g
        ad = ad + Dk
        adg = adg + Dk * np.abs(g)
        gmin, gmax = np.minimum(gmin, g), np.maximum(gmax, g)
    return dict(val=s / K, T=T / K, gmu=-(sd / K) / sig, gsig=-(sdg / K) / sig, sig=sig, follows=follows, amu=(ad / K) / sig,
                asig=(adg / K) / sig, gmin=gmin, gmax=gmax)


def value(model, Q, ystar, s2_offset=0.0, clamp_lo=1e-8):
    """from_posterior on the restated posterior of a cacq_reference Model at the rows of Q"""
    mu, s2 = cr.posterior(model, Q, clamp_lo)
    return from_posterior(mu, s2, ystar, s2_offset, clamp_lo)


def value_grad(model, Q, ystar, s2_offset=0.0, clamp_lo=1e-8):
    """dict(val, dval (M, D), sval (M, D): the scale -- the same sums over absolute values, T) at the rows of Q"""
    Q = np.atleast_2d(np.asarray(Q, dtype=float))
    g = model.ref.grad(Q, sf2k=model.sf2k, clamp_lo=clamp_lo)
    r = from_posterior(g["mu"], g["s2"], ystar, s2_offset, clamp_lo)
    f = r["follows"][:, None]
    dsig = np.where(f, g["ds2"], 0.0) / (2.0 * r["sig"])[:, None]
    ssig = np.where(f, g["ss2"], 0.0) / (2.0 * r["sig"])[:, None]
    return dict(val=r["val"], T=r["T"], dval=r["gmu"][:, None] * g["dmu"] + r["gsig"][:, None] * dsig,
                sval=r["amu"][:, None] * g["smu"] + r["asig"][:, None] * ssig)


def maxcdf(mu, s2, levels, s2_offset=0.0, clamp_lo=1e-8):
    """(sum_i log Phi((t_k - mu_i) / sigma_i) per level, i ascending; the same over absolute values; max mu; max(mu + 5 sigma)), NaN
    candidates skipped"""
    mu = np.asarray(mu, dtype=float)
    sig, _ = sigma_of(s2, s2_offset, clamp_lo)
    live = ~(np.isnan(mu) | np.isnan(sig))
    mu, sig = mu[live], sig[live]
    out, mag = [], []
    for t in np.asarray(levels, dtype=float).reshape(-1):
        lc = logcdf((t - mu) / sig)
        s = a = 0.0
        for x in lc:
            s = s + x
            a = a + abs(x)
        out.append(s); mag.append(a)
    return (np.array(out), np.array(mag), float(np.max(mu)) if len(mu) else -np.inf,
            float(np.max(mu + 5.0 * sig)) if len(mu) else -np.inf)


def gumbel_fit(levels, lcdf):
    """(a, b, (y25, y50, y75)): the quartiles by linear interpolation of the cdf over the ascending levels,
    b = (y25 - y75) / (log log(4/3) - log log 4), a = y50 + b log log 2"""
    cdf = np.exp(np.asarray(lcdf, dtype=float))
    y25, y50, y75 = np.interp([.25, .5, .75], cdf, np.asarray(levels, dtype=float))
    b = (y25 - y75) / (np.log(np.log(4.0 / 3.0)) - np.log(np.log(4.0)))
    return y50 + b * np.log(np.log(2.0)), b, (y25, y50, y75)


def gumbel_samples(a, b, floor, n, seed):
    u = np.random.default_rng(seed).uniform(size=n)
    return np.maximum(a - b * np.log(-np.log(u)), floor)


# ---- the truth: mpmath at 60 digits.  For g >= 0 through erfc and log1p: Phi = 1 - 1e-198 is not a 60-digit number, 1 - Phi is.
MP_DPS = 60


def terms_mp(g):
    """(lambda, nll) as mpf"""
    with mpmath.workdps(MP_DPS):
        return _terms_mpf(mpmath.mpf(float(g)))


def walk_mp(mu, s2, ystar, s2_offset, clamp_lo, dps=MP_DPS):
    """(MES, mean T) of ONE candidate as mpf, from float64 (mu, s2): v, sigma and every gamma in `dps` digits"""
    with mpmath.workdps(dps):
        v = mpmath.mpf(float(s2)) - mpmath.mpf(float(s2_offset))
        if v < clamp_lo:
            v = mpmath.mpf(float(clamp_lo))
        sig = mpmath.sqrt(v)
        s = T = mpmath.mpf(0)
        for y in ystar:
            g = (mpmath.mpf(float(y)) - mpmath.mpf(float(mu))) / sig
            lam, nll = _terms_mpf(g)
            a = g * lam / 2
            s += a + nll
            T += abs(a) + abs(nll)
        return s / len(ystar), T / len(ystar)


def _terms_mpf(g):
    phi = mpmath.exp(-g * g / 2) / mpmath.sqrt(2 * mpmath.pi)
    if g >= 0:
        q = mpmath.erfc(g / mpmath.sqrt(2)) / 2
        return phi / (1 - q), -mpmath.log1p(-q)
    Phi = mpmath.erfc(-g / mpmath.sqrt(2)) / 2
    return phi / Phi, -mpmath.log(Phi)

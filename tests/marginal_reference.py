"""
The integrated acquisition of ibo_iacq_* (include/ibo_abi_ensemble.h) and the slice sampler of ibo_amd/gaussianprocess/hypersample.py restated
from their documents; pinned by tests/test_marginal_reference.py, the yardstick of tests/test_gpu_marginal.py.

From per-member arrays (S, M) -- mu, s2, and for the gradient dmu, ds2 (S, M, D) -- and the weights w (S,), as given, not normalised:

    a_s   = EI / PI / UCB of (mu_s, sqrt(s2_s)) against ymax with parm, either erf flavour (ACQ_NONE: mu_s)
    val   = sum_s w_s a_s                                    sval  = sum_s w_s |a_s|           (the scale of val's bar)
    mean  = (sum_s w_s mu_s) / (sum_s w_s)                   smean = (sum_s w_s |mu_s|) / sum_s w_s
    var   = (sum_s w_s (s2_s + (mu_s - mean)^2)) / sum_s w_s -- two passes; its scale svar is the same sum: every term is >= 0
    dval  = sum_s w_s da_s                                   sdval = sum_s w_s |da_s| by the chain rule over absolute values

all sums over s ascending, members with w_s == 0 left out (whatever they hold), the sums started at -0.0.  dtype np.float64 is the
statement of what the device does -- plain fp64, products and sums rounded separately; np.longdouble is the same in extended precision
with an erf of 30 digits (mpmath), the truth the float64 form is held to.  var_cancelling is the form the device must NOT use.

slice_sample_scalar is one chain of hypersample.sliceSample written as the sequential loop its document describes, one logp call per point.
"""
import math

import numpy as np

import grad_reference as gr

LD = np.longdouble
ACQ_EI, ACQ_PI, ACQ_UCB, ACQ_NONE = gr.ACQ_EI, gr.ACQ_PI, gr.ACQ_UCB, gr.ACQ_NONE
ERF_LIBM, ERF_NR = gr.ERF_LIBM, gr.ERF_NR


def _erf_ld(z):
    """erf of a long-double array to 30 digits"""
    import mpmath
    old = mpmath.mp.dps
    mpmath.mp.dps = 40
    try:
        flat = [LD(mpmath.nstr(mpmath.erf(mpmath.mpf(np.format_float_scientific(v, unique=True) if np.isfinite(v) else str(float(v)))), 30))
                for v in np.asarray(z, dtype=LD).reshape(-1)]
    finally:
        mpmath.mp.dps = old
    return np.array(flat, dtype=LD).reshape(np.shape(z))


def cdf_pdf(erf_mode, z, dtype=np.float64):
    """Phi and phi of the call's erf flavour (NR: with the reference's truncated constants), in dtype"""
    if dtype is np.float64:
        return gr.cdf_pdf(erf_mode, z)
    z = np.asarray(z, dtype=LD)
    if erf_mode == ERF_LIBM:
        return LD(0.5) * (LD(1) + _erf_ld(z / np.sqrt(LD(2)))), np.exp(-(z * z / LD(2))) / np.sqrt(LD(2) * _PI_LD)
    x = z * LD(0.707106)
    t = LD(1) / (LD(1) + LD(0.5) * np.abs(x))
    p = LD(0.17087277)
    for c in (-0.82215223, 1.48851587, -1.13520398, 0.27886807, -0.18628806, 0.09678418, 0.37409196, 1.00002368):
        p = LD(c) + t * p
    ans = LD(1) - t * np.exp(-x * x - LD(1.26551223) + t * p)
    return LD(0.5) * (LD(1) + np.where(x >= 0, ans, -ans)), np.exp(-(z * z / LD(2))) * LD(0.398942)


_PI_LD = LD("3.14159265358979323846264338327950288")


def acq_members(acq, erf_mode, mu, s2, ymax, parm, dtype=np.float64):
    """a_s (and its partials da/dmu, da/dsigma, for the gradient) of every member and point"""
    mu, s2 = np.asarray(mu, dtype=dtype), np.asarray(s2, dtype=dtype)
    one = dtype(1)
    if acq == ACQ_NONE:
        return mu, one + 0 * mu, 0 * mu
    sig = np.sqrt(s2)
    if acq == ACQ_UCB:
        return mu + dtype(parm) * sig, one + 0 * mu, dtype(parm) + 0 * mu
    yd = mu - dtype(ymax) - dtype(parm)
    z = yd / sig
    cdf, pdf = cdf_pdf(erf_mode, z, dtype)
    if acq == ACQ_PI:
        return cdf, pdf / sig, -pdf * z / sig
    return yd * cdf + sig * pdf, cdf, pdf


def acq_scale(acq, mu, s2, ymax, parm):
    """the magnitudes of the terms a_s, da_s/dmu and da_s/dsigma are made of (float64): what an absolute error of one rounding in Phi, phi
    or a product is a fraction of.  EI = yd Phi + sigma phi with Phi = (1 + erf) / 2: |yd| + sigma;  its partials Phi and phi: 1"""
    mu, s2 = np.asarray(mu, dtype=float), np.asarray(s2, dtype=float)
    sig, one = np.sqrt(s2), np.ones_like(mu)
    if acq == ACQ_NONE:
        return np.abs(mu), one, 0 * one
    if acq == ACQ_UCB:
        return np.abs(mu) + abs(parm) * sig, one, abs(parm) * one
    yd = np.abs(mu - ymax - parm)
    if acq == ACQ_PI:
        return one, one / sig, (1 + yd / sig) / sig
    return yd + sig, one, one


def _active(w):
    return [s for s in range(len(w)) if w[s] != 0.0]


def combine(w, mu, s2, a=None, dtype=np.float64):
    """dict(val, sval, mean, smean, var, svar) over the points (M,); a: the members' acquisition values (None: val = sum w mu)"""
    w = np.asarray(w, dtype=dtype)
    mu, s2 = np.asarray(mu, dtype=dtype), np.asarray(s2, dtype=dtype)
    a = mu if a is None else np.asarray(a, dtype=dtype)
    M = mu.shape[1]
    val, sm = np.full(M, -0.0, dtype=dtype), np.full(M, -0.0, dtype=dtype)
    sval, smean, sw = np.zeros(M, dtype=dtype), np.zeros(M, dtype=dtype), dtype(0)
    for s in _active(w):
        val = val + w[s] * a[s]
        sval = sval + w[s] * np.abs(a[s])
        sm = sm + w[s] * mu[s]
        smean = smean + w[s] * np.abs(mu[s])
        sw = sw + w[s]
    mean = sm / sw
    sv = np.zeros(M, dtype=dtype)
    for s in _active(w):
        d = mu[s] - mean
        sv = sv + w[s] * (s2[s] + d * d)
    return dict(val=val, sval=sval, mean=mean, smean=smean / sw, var=sv / sw, svar=sv / sw)


def var_cancelling(w, mu, s2, dtype=np.float64):
    """E[s2 + mu^2] - mean^2: the one-pass form, which loses everything when |mu| is large against the spread"""
    w = np.asarray(w, dtype=dtype)
    mu, s2 = np.asarray(mu, dtype=dtype), np.asarray(s2, dtype=dtype)
    sw = sum(w[s] for s in _active(w))
    m1 = sum(w[s] * mu[s] for s in _active(w)) / sw
    m2 = sum(w[s] * (s2[s] + mu[s] * mu[s]) for s in _active(w)) / sw
    return m2 - m1 * m1


def combine_grad(w, da, sda=None, dtype=np.float64):
    """(dval, sdval) (M, D) from the members' gradients da (S, M, D) and their scales sda (None: |da|)"""
    w = np.asarray(w, dtype=dtype)
    da = np.asarray(da, dtype=dtype)
    sda = np.abs(da) if sda is None else np.asarray(sda, dtype=dtype)
    dval, sdval = np.full(da.shape[1:], -0.0, dtype=dtype), np.zeros(da.shape[1:], dtype=dtype)
    for s in _active(w):
        dval = dval + w[s] * da[s]
        sdval = sdval + w[s] * sda[s]
    return dval, sdval


def member_grads(acq, erf_mode, mu, s2, dmu, ds2, ymax, parm, dtype=np.float64):
    """da_s (S, M, D) by the chain rule from (mu, s2, dmu, ds2): da = a_mu dmu + a_sigma ds2 / (2 sigma)"""
    _, a_mu, a_sig = acq_members(acq, erf_mode, mu, s2, ymax, parm, dtype)
    sig = np.sqrt(np.asarray(s2, dtype=dtype))
    dmu, ds2 = np.asarray(dmu, dtype=dtype), np.asarray(ds2, dtype=dtype)
    return a_mu[..., None] * dmu + a_sig[..., None] * (ds2 / (2 * sig)[..., None])


# ------------------------------------------------------------------------------------------------ the sampler, one chain, sequentially
MAX_SHRINK = 200


def slice_sample_scalar(logp, x0, n, burn=20, thin=2, width=1.0, max_steps=8, seed=0, chain=0):
    """chain `chain` of sliceSample(.., seed=seed) started at x0 (d,): logp((1, d)) -> (1,) is called for one point at a time.  The draws,
    all rng.random() of default_rng([seed, chain]): per sweep and coordinate the level, the interval's position, the step budget, then one
    per shrinkage proposal.  Returns (samples (n, d), logp (n,))."""
    rng = np.random.default_rng([int(seed), int(chain)])
    x = np.array(x0, dtype=float)
    d = len(x)

    def f(q):
        return float(np.asarray(logp(q.reshape(1, d)), dtype=float).reshape(-1)[0])

    lp = f(x)
    assert np.isfinite(lp)
    xs, lps = [], []
    for sweep in range(1, burn + n * thin + 1):
        for j in range(d):
            logy = lp + math.log1p(-rng.random())
            left = x[j] - width * rng.random()
            right = left + width
            J = int(math.floor(max_steps * rng.random()))
            K = max_steps - 1 - J
            q = x.copy()
            while J > 0:
                q[j] = left
                if not f(q) > logy:
                    break
                left -= width
                J -= 1
            while K > 0:
                q[j] = right
                if not f(q) > logy:
                    break
                right += width
                K -= 1
            for _ in range(MAX_SHRINK):
                x1 = left + rng.random() * (right - left)
                q[j] = x1
                v = f(q)
                if v > logy:
                    x[j], lp = x1, v
                    break
                if x1 < x[j]:
                    left = x1
                else:
                    right = x1
        if sweep > burn and (sweep - burn) % thin == 0:
            xs.append(x.copy()); lps.append(lp)
    return np.array(xs), np.array(lps)

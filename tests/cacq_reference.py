"""
The constrained acquisition of ibo_cacq_* restated in NumPy/SciPy (float64) from scratch -- kernel, Cholesky, posterior, clip,
acquisition, both erf flavours -- on the pieces of tests/grad_reference.py (kernel_spec, kstar, cdf_pdf, prior_grad, RefGP's
factorisation); pinned to the oracle by tests/test_cacq_reference.py, the yardstick of tests/test_gpu_constrained.py.

    z_j = s_j (t_j - mu_j) / sigma_j      P = prod_j Phi(z_j)      val = A Phi(z_0) Phi(z_1) ..   (A: EI / PI; ACQ_NONE: 1)
    dsigma_j = dsigma^2_j / (2 sigma_j)   dz_j = -(s_j dmu_j + z_j dsigma_j) / sigma_j
    dP = sum_j phi(z_j) dz_j prod_{i != j} Phi(z_i)           dval = dA P + A dP

Each gradient comes with its SCALE: the same sums over absolute values.
"""
import functools

import numpy as np
from scipy.linalg import cho_solve

import grad_reference as gr


class Model(object):
    """a RefGP with the k* signal variance and what the constrained call needs of it; thresh / sense: as a constraint"""

    def __init__(self, ref, thresh=None, sense=1, sf2k=None):
        self.ref, self.thresh, self.sense = ref, thresh, int(sense)
        self.sf2k = ref.sf2 if sf2k is None else float(sf2k)


def make(X, Y, noise, kind, hyper, prior=None, **kw):
    """Model from the oracle's kernel naming ('ard', 'iso', 'svard', 'sviso', 'm3', 'm5'); kw: thresh, sense, sf2k"""
    fam, w, sf2 = gr.kernel_spec(kind, hyper, np.atleast_2d(X).shape[1])
    return Model(gr.RefGP(X, Y, noise, fam, w, sf2, prior=prior), **kw)


def posterior(model, Q, clamp_lo):
    """(mu, s2) at the rows of Q: mu = m + k*.aY - m k*.a1, s2 = clip(1 + noise - k*.R^-1 k*, clamp_lo, 10)"""
    r = model.ref
    Q = np.atleast_2d(np.asarray(Q, dtype=float))
    K = np.empty((len(Q), len(r.Y)))
    for i, x in enumerate(Q):
        K[i] = gr.kstar(r.fam, r.w, model.sf2k, x, r.X)[0]
    if r.prior is not None:
        m = np.array([gr.prior_grad(r.prior, x)[0] for x in Q])
        mu = m + K @ r.aY - m * (K @ r.a1)
    else:
        mu = K @ r.aY
    U = cho_solve(r.cf, K.T)
    s2 = np.clip(1.0 + r.noise - np.sum(K.T * U, axis=0), clamp_lo, 10.0)
    return mu, s2


def acq_value(acq, erf_mode, mu, sig, ymax, parm):
    yd = mu - ymax - parm
    z = yd / sig
    cdf, pdf = gr.cdf_pdf(erf_mode, z)
    return cdf if acq == gr.ACQ_PI else yd * cdf + sig * pdf


def _ymax(obj, ymax):
    return float(np.max(obj.ref.Y)) if ymax is None or ymax != ymax else float(ymax)


def value(obj, cons, Q, acq=gr.ACQ_EI, parm=0.01, erf_mode=gr.ERF_LIBM, clamp_lo=1e-8, ymax=None):
    """dict(acq, pof, val, phis (ncon, M)) at the rows of Q, factors multiplied in the order A, Phi(z_0), Phi(z_1), .."""
    Q = np.atleast_2d(np.asarray(Q, dtype=float))
    if acq == gr.ACQ_NONE:
        A = np.ones(len(Q))
    else:
        mu, s2 = posterior(obj, Q, clamp_lo)
        A = acq_value(acq, erf_mode, mu, np.sqrt(s2), _ymax(obj, ymax), parm)
    P, val, phis = np.ones(len(Q)), A.copy(), []
    for c in cons:
        mu, s2 = posterior(c, Q, clamp_lo)
        cdf, _ = gr.cdf_pdf(erf_mode, c.sense * (c.thresh - mu) / np.sqrt(s2))
        P = P * cdf
        val = val * cdf
        phis.append(cdf)
    return dict(acq=A, pof=P, val=val, phis=np.array(phis).reshape(len(cons), len(Q)))


def value_grad(obj, cons, Q, acq=gr.ACQ_EI, parm=0.01, erf_mode=gr.ERF_LIBM, clamp_lo=1e-8, ymax=None):
    """dict(val, dval (M, D), sval (M, D): the scale) at the rows of Q"""
    Q = np.atleast_2d(np.asarray(Q, dtype=float))
    M, D = Q.shape
    if acq == gr.ACQ_NONE:
        A, dA, sA = np.ones(M), np.zeros((M, D)), np.zeros((M, D))
    else:
        g = obj.ref.grad(Q, sf2k=obj.sf2k, clamp_lo=clamp_lo, acq=acq, parm=parm, erf_mode=erf_mode, ymax=_ymax(obj, ymax))
        A, dA, sA = g["acq"], g["dacq"], g["sacq"]
    cdf, pdf, dz, sz = [], [], [], []
    for c in cons:
        g = c.ref.grad(Q, sf2k=c.sf2k, clamp_lo=clamp_lo)
        sig = np.sqrt(g["s2"])
        z = c.sense * (c.thresh - g["mu"]) / sig
        cd, pd = gr.cdf_pdf(erf_mode, z)
        dsig, ssig = g["ds2"] / (2 * sig)[:, None], g["ss2"] / (2 * sig)[:, None]
        cdf.append(cd); pdf.append(pd)
        dz.append(-(c.sense * g["dmu"] + z[:, None] * dsig) / sig[:, None])
        sz.append((g["smu"] + np.abs(z)[:, None] * ssig) / sig[:, None])
    P, val = np.ones(M), A.copy()
    for cd in cdf:
        P = P * cd
        val = val * cd
    dP, sP = np.zeros((M, D)), np.zeros((M, D))
    for j in range(len(cons)):
        w = pdf[j].copy()
        for i in range(len(cons)):
            if i != j:
                w = w * cdf[i]
        dP += w[:, None] * dz[j]
        sP += w[:, None] * sz[j]
    return dict(val=val, dval=dA * P[:, None] + A[:, None] * dP, sval=sA * P[:, None] + np.abs(A)[:, None] * sP)


def argmax(val, exclude=None, Q=None, radius=0.5):
    """the device's rule: NaNs and candidates inside an exclusion ball are left out, the first maximiser wins; -1: none left"""
    score = np.where(np.isnan(val), -np.inf, np.asarray(val, dtype=float))
    if exclude is not None and len(exclude):
        d = np.sqrt(((np.asarray(Q)[:, None, :] - np.atleast_2d(exclude)[None, :, :]) ** 2).sum(-1))
        score = np.where(np.any(~(d > radius), axis=1), -np.inf, score)
    k = int(np.argmax(score))
    return (-1, -np.inf) if score[k] == -np.inf else (k, float(score[k]))


# ---- the generator of the three cases the GPU sweep is compared on
GEN_CASES = ((1, 40, 2), (2, 120, 3), (3, 300, 5))
GEN_M = 3000
GEN_NOISE, GEN_XI = 0.05, 0.01


@functools.lru_cache(maxsize=None)
def generator(seed, N, D):
    """dict of one case: the data (X, Q, Yo, Yc1, Yc2), thresholds t1 (c1 <= t1: the 60th percentile) and t2 (c2 >= t2: the
    40th), the SE-iso length scale 0.3 sqrt(D), ymax = the best Yo among the rows feasible BY OBSERVATION, and the reference's
    values over Q (libm erf, clamp 1e-8: the native sweep's conventions) -- computed once, shared, to be left unchanged"""
    rs = np.random.RandomState(seed)
    X = rs.rand(N, D)
    Q = rs.rand(GEN_M, D)
    Yo = np.sin(3 * X.sum(1)) + .01 * rs.randn(N)
    Yc1 = np.cos(2 * X[:, 0]) - X[:, -1] + .01 * rs.randn(N)
    Yc2 = ((X - .5) ** 2).sum(1) + .01 * rs.randn(N)
    t1, t2 = float(np.percentile(Yc1, 60)), float(np.percentile(Yc2, 40))
    theta = 0.3 * np.sqrt(D)
    feas = (Yc1 <= t1) & (Yc2 >= t2)
    ymax = float(np.max(Yo[feas]))
    obj = make(X, Yo, GEN_NOISE, 'iso', [theta])
    cons = [make(X, Yc1, GEN_NOISE, 'iso', [theta], thresh=t1, sense=1), make(X, Yc2, GEN_NOISE, 'iso', [theta], thresh=t2, sense=-1)]
    ref = value(obj, cons, Q, gr.ACQ_EI, GEN_XI, gr.ERF_LIBM, 1e-8, ymax)
    for v in ref.values():
        v.setflags(write=False)
    return dict(X=X, Q=Q, Yo=Yo, Yc1=Yc1, Yc2=Yc2, t1=t1, t2=t2, theta=theta, ymax=ymax, obj=obj, cons=cons, ref=ref)

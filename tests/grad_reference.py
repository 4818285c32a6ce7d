"""
The gradients of ibo_acq_grad_batch restated in NumPy/SciPy (float64), for tests/test_gpu_gradients.py; pinned to the
oracle's posterior and acquisition by tests/test_grad_reference.py.

R = K(X, X; sf2) with the diagonal 1 + noise; alpha_Y, alpha_1 and u = R^-1 k* by cho_solve.  With d_i = x - X_i and
dk*_i / dx = h_i w * d_i (h_i per family, w the inverse squared length scales):
    mu   = m + k*.aY - m k*.a1        dmu = dm (1 - k*.a1) + sum_i h_i (aY_i - m a1_i) w d_i
    s2   = clip(1 + noise - k*.u)     ds2 = -2 sum_i h_i u_i w d_i   (0 where the clip is active)
and the chain rule of EI / PI / UCB.  Each gradient comes with its SCALE: the same sums over absolute values, the yardstick
of the tests' tolerance (1e-9 scale + 1e-13).
"""
import numpy as np
from scipy.linalg import cho_factor, cho_solve
from scipy.special import erf

FAM_SE, FAM_M3, FAM_M5 = 0, 1, 2
ACQ_EI, ACQ_PI, ACQ_UCB, ACQ_NONE = 0, 1, 2, 3
ERF_LIBM, ERF_NR = 0, 1


def kernel_spec(kind, hyper, D):
    """(family, w (D,), sf2) of a kernel in the oracle's naming: 'ard', 'iso', 'svard', 'sviso', 'm3', 'm5'"""
    hyper = np.asarray(hyper, dtype=float)
    if kind in ('ard', 'svard'):
        th = np.clip(hyper if kind == 'ard' else hyper[:-1], 1e-4, 1e4)
        fam, w = FAM_SE, 1.0 / th ** 2
    else:
        fam = {'iso': FAM_SE, 'sviso': FAM_SE, 'm3': FAM_M3, 'm5': FAM_M5}[kind]
        w = np.full(D, 1.0 / hyper[0] ** 2)
    sf2 = float(hyper[-1] ** 2) if kind in ('svard', 'sviso', 'm3', 'm5') else 1.0
    return fam, w, sf2


def kstar(fam, w, sf2, x, X):
    """k*(x, X_i) and h_i (dk*_i/dx = h_i w (x - X_i))"""
    diff = x[None, :] - X
    z = np.sum(w * diff ** 2, axis=1)
    if fam == FAM_SE:
        k = sf2 * np.exp(-0.5 * z)
        return k, -k, diff
    if fam == FAM_M3:
        r = np.sqrt(3.0 * z); e = np.exp(-r)
        return sf2 * (1.0 + r) * e, -3.0 * sf2 * e, diff
    r = np.sqrt(5.0 * z); e = np.exp(-r)
    return sf2 * (1.0 + r + r * r / 3.0) * e, -(5.0 / 3.0) * sf2 * (1.0 + r) * e, diff


def prior_grad(prior, x):
    """(m, dm) of an RBF-network prior given as (means (k, D), beta, theta, lowerb, width), or (0, 0)"""
    if prior is None:
        return 0.0, np.zeros(len(x))
    means, beta, theta, lo, wd = prior
    diff = (x - lo) / wd - np.atleast_2d(means)
    be = np.asarray(beta) * np.exp(-theta * np.sum(diff ** 2, axis=1))
    return float(be.sum()), (be @ diff) * (-2.0 * theta) / wd


def cdf_pdf(erf_mode, z):
    if erf_mode == ERF_LIBM:
        return 0.5 * (1.0 + erf(z / np.sqrt(2.0))), np.exp(-(z * z / 2.0)) / np.sqrt(2.0 * np.pi)
    return 0.5 * (1.0 + erf_nr(z * 0.707106)), np.exp(-(z * z / 2.0)) * 0.398942


def erf_nr(x):
    """the Numerical Recipes erf the Python reference uses (erfc by Chebyshev fit)"""
    x = np.asarray(x, dtype=float)
    t = 1.0 / (1.0 + 0.5 * np.abs(x))
    p = 0.17087277
    for c in (-0.82215223, 1.48851587, -1.13520398, 0.27886807, -0.18628806, 0.09678418, 0.37409196, 1.00002368):
        p = c + t * p
    ans = 1.0 - t * np.exp(-x * x - 1.26551223 + t * p)
    return np.where(x >= 0.0, ans, -ans)


class RefGP(object):
    def __init__(self, X, Y, noise, fam, w, sf2, prior=None):
        self.X = np.atleast_2d(np.asarray(X, dtype=float)); self.Y = np.asarray(Y, dtype=float).reshape(-1)
        self.noise, self.fam, self.w, self.sf2, self.prior = float(noise), fam, np.asarray(w, dtype=float), float(sf2), prior
        N = len(self.Y)
        R = np.empty((N, N))
        for i in range(N):
            R[i] = kstar(fam, self.w, self.sf2, self.X[i], self.X)[0]
        np.fill_diagonal(R, 1.0 + self.noise)
        self.R = R
        self.cf = cho_factor(R, lower=True)
        self.aY = cho_solve(self.cf, self.Y)
        self.a1 = cho_solve(self.cf, np.ones(N))

    def grad(self, Q, sf2k=None, clamp_lo=1e-7, acq=ACQ_NONE, parm=0.0, erf_mode=ERF_NR, ymax=None):
        """dict of mu, s2, dmu, ds2, [acq, dacq] and the scales smu, ss2, [sacq] (arrays over the rows of Q)"""
        Q = np.atleast_2d(np.asarray(Q, dtype=float))
        sf2k = self.sf2 if sf2k is None else sf2k
        ymax = float(np.max(self.Y)) if ymax is None else ymax
        M, D = Q.shape
        out = {k: np.zeros(M) for k in ("mu", "s2", "acq")}
        for k in ("dmu", "ds2", "dacq", "smu", "ss2", "sacq"):
            out[k] = np.zeros((M, D))
        for j, x in enumerate(Q):
            k, h, diff = kstar(self.fam, self.w, sf2k, x, self.X)
            u = cho_solve(self.cf, k)
            m, dm = prior_grad(self.prior, x)
            ka1 = k @ self.a1
            mu = (m + k @ self.aY - m * ka1) if self.prior is not None else k @ self.aY
            raw = 1.0 + self.noise - k @ u
            clipped = not (clamp_lo < raw < 10.0)
            s2 = min(max(raw, clamp_lo), 10.0)
            tm = (h * (self.aY - m * self.a1))[:, None] * self.w * diff
            ts = -2.0 * (h * u)[:, None] * self.w * diff
            dmu = dm * (1.0 - ka1) + tm.sum(0)
            smu = np.abs(dm * (1.0 - ka1)) + np.abs(tm).sum(0)
            ds2 = np.zeros(D) if clipped else ts.sum(0)
            ss2 = np.zeros(D) if clipped else np.abs(ts).sum(0)
            out["mu"][j], out["s2"][j] = mu, s2
            out["dmu"][j], out["ds2"][j], out["smu"][j], out["ss2"][j] = dmu, ds2, smu, ss2
            if acq != ACQ_NONE:
                sig = np.sqrt(s2)
                dsig, ssig = ds2 / (2 * sig), ss2 / (2 * sig)
                if acq == ACQ_UCB:
                    v, g, sc = mu + parm * sig, dmu + parm * dsig, smu + abs(parm) * ssig
                else:
                    yd = mu - ymax - parm
                    z = yd / sig
                    cdf, pdf = cdf_pdf(erf_mode, z)
                    if acq == ACQ_PI:
                        v, g, sc = cdf, pdf * (dmu - z * dsig) / sig, pdf * (smu + abs(z) * ssig) / sig
                    else:
                        v, g, sc = yd * cdf + sig * pdf, cdf * dmu + pdf * dsig, cdf * smu + pdf * ssig
                out["acq"][j], out["dacq"][j], out["sacq"][j] = v, g, sc
        return out


def assert_grad_close(got, want, scale, rel=1e-9, atol=1e-13, what=""):
    got, want, scale = np.asarray(got), np.asarray(want), np.asarray(scale)
    err = np.abs(got - want)
    bad = err > rel * scale + atol
    if np.any(bad):
        i = np.argwhere(bad)[0]
        raise AssertionError("%s: %d of %d entries off; first at %s: got %r want %r scale %r" %
                             (what, int(bad.sum()), bad.size, tuple(i), got[tuple(i)], want[tuple(i)], scale[tuple(i)]))

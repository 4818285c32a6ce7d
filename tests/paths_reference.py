"""
Pathwise posterior draws (ibo_paths_*) restated in NumPy/SciPy float64, for tests/test_gpu_paths.py; pinned by
tests/test_paths_reference.py to the joint posterior of tests/cov_reference.py.

On a grad_reference.RefGP (R = K(X, X; sf2) with 1 + noise on the diagonal, aY = R^-1 Y, a1 = R^-1 1), with spectral draws
(omega (F, D), phase (F,)), weights w (S, F) and eps (S, N):
    phi_j(x)  = sqrt(2 sf2 / F) cos(omega_j.x + phase_j)
    c_s       = aY - R^-1 (Phi(X) w_s + eps_s)                              coefficients (S, F + N) = [w_s, c_s]
    path_s(x) = m + phi(x).w_s + k*(x).c_s - m k*(x).a1                     (m: the mean prior at x, 0 without one)
The argument of the cosine is formed in extended precision (np.longdouble) and reduced by 2 pi there, so that data a thousand
units from the origin cost the restatement nothing; where long double is float64 the restatement is only as good as float64's
omega.x.  T (terms_scale) = |m| + sum_j |phi_j w_j| + sum_i |k*_i c_i| is the yardstick of the GPU test's bars.
"""
import numpy as np
from scipy.linalg import cho_solve

import cov_reference as cr
import grad_reference as gr

LD = np.longdouble
TWO_PI_LD = 2 * (LD(3.141592653589793) + LD(1.2246467991473532e-16))       # pi to long double's precision, from its two float64 halves


def features(omega, phase, sf2, X):
    """Phi (M, F) at the rows of X"""
    X = np.atleast_2d(np.asarray(X, dtype=float)); omega = np.atleast_2d(np.asarray(omega, dtype=float))
    t = np.zeros((len(X), len(omega)), dtype=LD) + np.asarray(phase, dtype=LD)[None, :]
    for d in range(X.shape[1]):
        t += X[:, d, None].astype(LD) * omega[None, :, d].astype(LD)
    t -= TWO_PI_LD * np.rint(t / TWO_PI_LD)
    return np.sqrt(2.0 * sf2 / len(omega)) * np.cos(t.astype(np.float64))


def prior_mean(ref, Q):
    if ref.prior is None:
        return np.zeros(len(Q))
    return np.array([gr.prior_grad(ref.prior, x)[0] for x in Q])


def coef(ref, omega, phase, w, eps):
    """(S, F + N): w_s, then c_s = aY - R^-1 (Phi(X) w_s + eps_s)"""
    w = np.atleast_2d(w); eps = np.atleast_2d(eps)
    u = features(omega, phase, ref.sf2, ref.X) @ w.T + eps.T                # N x S
    c = ref.aY[:, None] - cho_solve(ref.cf, u)
    return np.c_[w, c.T]


def _parts(ref, omega, phase, coefs, Q):
    Q = np.atleast_2d(np.asarray(Q, dtype=float))
    F = len(np.atleast_2d(omega))
    coefs = np.atleast_2d(coefs)
    return Q, features(omega, phase, ref.sf2, Q), cr.kmat(ref.fam, ref.w, ref.sf2, Q, ref.X), coefs[:, :F], coefs[:, F:], prior_mean(ref, Q)


def values(ref, omega, phase, coefs, Q):
    """(S, M): the paths with coefficients `coefs` (S, F + N) at the rows of Q"""
    Q, Phi, Ks, w, c, m = _parts(ref, omega, phase, coefs, Q)
    v = Phi @ w.T + Ks @ c.T                                                # M x S
    if ref.prior is not None:
        v = m[:, None] + v - (m * (Ks @ ref.a1))[:, None]
    return v.T


def terms_scale(ref, omega, phase, coefs, Q):
    """T (S, M) = |m| + sum_j |phi_j w_sj| + sum_i |k*_i c_si|"""
    Q, Phi, Ks, w, c, m = _parts(ref, omega, phase, coefs, Q)
    return (np.abs(m)[:, None] + np.abs(Phi) @ np.abs(w).T + np.abs(Ks) @ np.abs(c).T).T


def g_map(ref, omega, phase, Q):
    """G (M, F + N) with g_s(Q) = G [w_s ; eps_s / sqrt(d)], d = 1 + noise - sf2 (eps_s = sqrt(d) z): the part of a path that is
    random, linear in the standard normals -- Cov g = G G^T for fixed (omega, phase)"""
    Q = np.atleast_2d(np.asarray(Q, dtype=float))
    Ks = cr.kmat(ref.fam, ref.w, ref.sf2, Q, ref.X)                          # M x N
    B = cho_solve(ref.cf, Ks.T).T                                           # k*^T R^-1, M x N
    d = 1.0 + ref.noise - ref.sf2
    return np.c_[features(omega, phase, ref.sf2, Q) - B @ features(omega, phase, ref.sf2, ref.X), -np.sqrt(d) * B]


def latent_cov(ref, Q):
    """the covariance the paths aim at: cov_reference's Sigma without noise, the diagonal taken as sf2 - |v|^2"""
    S, vn = cr.cov(ref, Q, with_noise=False)
    np.fill_diagonal(S, ref.sf2 - vn ** 2)
    return S

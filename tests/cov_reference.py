"""
The joint posterior of ibo_posterior_cov restated in NumPy/SciPy (float64), for tests/test_gpu_posterior_cov.py; pinned to the
oracle by tests/test_cov_reference.py.

For query points Q on a model with R = K(X, X; sf2), diagonal 1 + noise, and k* = K(X, Q; sf2k):
    Sigma_ab = k(q_a, q_b) - k*_a^T R^-1 k*_b                  (a != b)
    Sigma_aa = 1 + noise - k*_a^T R^-1 k*_a   (with_noise)     or 1 - k*_a^T R^-1 k*_a
Two forms: `cov` from a grad_reference.RefGP (cho_solve), `cov_L` from any lower factor L of the matrix the model was fitted
with (GP.L, GP.augL: the preference GP's chol(R + C^-1)).  Each returns Sigma and |v_a| = |L^-1 k*_a|, the scale of the tests'
tolerance |dSigma_ab| <= 1e-10 (sf2 + noise + |v_a| |v_b|).
"""
import numpy as np
from scipy.linalg import cho_solve, solve_triangular

import grad_reference as gr


def kmat(fam, w, sf2, A, B):
    """K(A, B) with the formulas of grad_reference.kstar, a dimension at a time"""
    A = np.atleast_2d(np.asarray(A, dtype=float)); B = np.atleast_2d(np.asarray(B, dtype=float))
    z = np.zeros((len(A), len(B)))
    for d in range(A.shape[1]):
        z += w[d] * (A[:, d, None] - B[None, :, d]) ** 2
    if fam == gr.FAM_SE:
        return sf2 * np.exp(-0.5 * z)
    if fam == gr.FAM_M3:
        r = np.sqrt(3.0 * z)
        return sf2 * (1.0 + r) * np.exp(-r)
    r = np.sqrt(5.0 * z)
    return sf2 * (1.0 + r + r * r / 3.0) * np.exp(-r)


def _finish(KQQ, quad, noise, with_noise):
    S = KQQ - quad
    vn = np.sqrt(np.maximum(np.diag(quad), 0.0))
    np.fill_diagonal(S, (1.0 + noise if with_noise else 1.0) - np.diag(quad))
    return S, vn


def cov(ref, Q, with_noise=True, sf2k=None):
    """(Sigma, |v|) of a grad_reference.RefGP at the rows of Q"""
    sf2k = ref.sf2 if sf2k is None else sf2k
    Q = np.atleast_2d(np.asarray(Q, dtype=float))
    Ks = kmat(ref.fam, ref.w, sf2k, ref.X, Q)                 # N x M
    quad = Ks.T @ cho_solve(ref.cf, Ks)
    quad = 0.5 * (quad + quad.T)
    return _finish(kmat(ref.fam, ref.w, sf2k, Q, Q), quad, ref.noise, with_noise)


def cov_L(L, X, fam, w, sf2k, noise, Q, with_noise=True):
    """(Sigma, |v|) from a lower factor L of the fitted matrix (v = L^-1 k*)"""
    Q = np.atleast_2d(np.asarray(Q, dtype=float))
    V = solve_triangular(np.tril(L), kmat(fam, w, sf2k, X, Q), lower=True)
    return _finish(kmat(fam, w, sf2k, Q, Q), V.T @ V, noise, with_noise)


def assert_cov_close(S, Sref, vn, sf2, noise, rel=1e-10, what=""):
    tol = rel * (sf2 + noise + np.outer(vn, vn))
    err = np.abs(np.asarray(S) - Sref)
    bad = err > tol
    if np.any(bad):
        i = tuple(np.argwhere(bad)[0])
        raise AssertionError("%s: %d of %d entries off; first at %s: got %r want %r tol %r" %
                             (what, int(bad.sum()), bad.size, i, S[i], Sref[i], tol[i]))

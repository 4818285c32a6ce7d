"""
Leave-one-out predictions and the LOO-CV objective (Rasmussen & Williams 5.4.2) restated in NumPy, for tests/test_gpu_loo.py; pinned to
the oracle by tests/test_loo_reference.py.

For a symmetric positive definite A (N x N) and targets y, with B = A^-1, d_i = B_ii, alpha = B y:
    mu_-i  = y_i - alpha_i / d_i        s2_-i = 1 / d_i        (the posterior at x_i of the model fitted without observation i)
    nloo   = sum_i [-log(d_i) / 2 + alpha_i^2 / (2 d_i)] + N log(2 pi) / 2
    d nloo / d log theta_h = -sum_i [alpha_i r_i - (1 + alpha_i^2 / d_i) s_i / 2] / d_i,    T = B dA_h, r = T alpha, s_i = sum_b T_ib B_ib
    S_h    = sum_i [|alpha_i r_i| + (1 + alpha_i^2 / d_i) |s_i| / 2] / d_i                  (the scale of the gradient's tolerance)
with dA_h = oracle.Kern.derivative(X, h).  With a mean prior the reference subtracts the QUERY's prior from every target, so point i uses
alpha = B (Y - m(x_i) 1).  Two precisions: float64 (Cholesky inverse), and np.longdouble, the float64 inverse refined by two Newton steps
B <- B (2 I - A B) carried out in long double.  Every result comes with cond_2(A).
"""
import numpy as np
from scipy.linalg import cho_factor, cho_solve

from oracle import oracle as orc

HALF_LOG_2PI = 0.5 * np.log(2.0 * np.pi)


def inverse(A, longdouble=False):
    """A^-1, symmetric; float64 through the Cholesky factor, or refined in long double by two Newton steps"""
    A = np.asarray(A, dtype=np.float64)
    N = len(A)
    B = cho_solve(cho_factor(A, lower=True), np.eye(N))
    B = 0.5 * (B + B.T)
    if longdouble:
        Al = A.astype(np.longdouble); B = B.astype(np.longdouble)
        I2 = 2.0 * np.eye(N, dtype=np.longdouble)
        for _ in range(2):
            B = B @ (I2 - Al @ B)
        B = 0.5 * (B + B.T)
    return B


def cond2(A, B=None):
    """cond_2 of the symmetric positive definite A: lambda_max / lambda_min (through Lanczos on A and on B = A^-1 for a large matrix)"""
    A = np.asarray(A, dtype=np.float64)
    if len(A) <= 1100 or B is None:
        w = np.linalg.eigvalsh(A)
        return float(w[-1] / w[0])
    from scipy.sparse.linalg import eigsh
    hi = eigsh(A, k=1, which="LA", return_eigenvectors=False, tol=1e-6)[0]
    lo = eigsh(np.asarray(B, dtype=np.float64), k=1, which="LA", return_eigenvectors=False, tol=1e-6)[0]
    return float(hi * lo)


def loo_points(A, Y, m=None, longdouble=False, B=None):
    """dict(mu, s2, terms, value, d, c, B, cond): m: the prior's value at every point (or None); terms sum to value"""
    dt = np.longdouble if longdouble else np.float64
    B = inverse(A, longdouble) if B is None else B
    Y = np.asarray(Y, dtype=dt)
    d = np.diag(B).copy()
    c = B @ Y
    if m is not None:
        c = c - np.asarray(m, dtype=dt) * (B @ np.ones(len(Y), dtype=dt))
    terms = -0.5 * np.log(d) + c * c / (2.0 * d) + dt(HALF_LOG_2PI)
    return dict(mu=Y - c / d, s2=1.0 / d, terms=terms, value=terms.sum(), d=d, c=c, B=B, cond=cond2(A, B))


def handle_loo(ogp, longdouble=False):
    """the leave-one-out predictions of an oracle.GP (its R, or the matrix that replaces it; its prior)"""
    m = None if ogp.prior is None else np.array([ogp.prior.mu(x) for x in ogp.X])
    return loo_points(ogp.factor_matrix(), ogp.Y, m, longdouble)


def objective(kern, X, Y, noise, nhyper=0, longdouble=False):
    """looLikelihood's definition for an oracle.Kern: loo_points of A = cov_matrix + noise I, plus grad and S (nhyper each)"""
    dt = np.longdouble if longdouble else np.float64
    X = np.asarray(X, dtype=np.float64)
    A = kern.cov_matrix(X) + noise * np.eye(len(X))
    res = loo_points(A, Y, None, longdouble)
    B, al, d = res["B"], res["c"], res["d"]
    g = np.zeros(nhyper, dtype=dt); S = np.zeros(nhyper, dtype=dt)
    for h in range(nhyper):
        T = B @ np.asarray(kern.derivative(X, h), dtype=dt)
        r = T @ al
        s = np.sum(T * B, axis=1)
        f = 0.5 * (1.0 + al * al / d)
        g[h] = -np.sum((al * r - f * s) / d)
        S[h] = np.sum((np.abs(al * r) + f * np.abs(s)) / d)
    res["grad"], res["S"] = g, S
    return res


def brute_force(kern, X, Y, noise, prior, i):
    """(mu, s2) at X[i] of the oracle's model fitted without observation i (its variance clipped to [1e-7, 10])"""
    keep = np.arange(len(X)) != i
    return orc.GP(kern, X[keep], np.asarray(Y)[keep], noise=noise, prior=prior).posterior(X[i])


# ---- the looLikelihood cases of tests/test_gpu_loo.py: (kind, hyper, N, D, seed of conftest.synth), all with noise 1e-2
KINDS = ("ard", "iso", "svard", "sviso", "m3", "m5")
NOISE = 1e-2
FAMILY_CASES = [("ard", [.3, .6], 130, 2, 132), ("ard", [.3, .4, .5, .6, .7], 700, 5, 705),
                ("ard", list(np.linspace(.8, 1.6, 20)), 500, 20, 520),
                ("sviso", [.7, 1.3], 400, 4, 405), ("m3", [.8, 1.1], 400, 4, 405), ("m5", [.9, 1.2], 400, 4, 405),
                ("iso", [.6], 400, 4, 405), ("svard", [.5, .6, .7, .8, 1.2], 400, 4, 405)]
EDGE_CASES = [("ard", [.4, .7], N, 2, N + 2) for N in (1, 2, 64, 65, 127, 129)] + \
             [("ard", list(np.linspace(.9, 1.8, 64)), 100, 64, 164)]
ROUTE_CASES = [("ard", [.5, .7, .9, 1.1], N, 4, N + 4) for N in (1728, 1729, 2100, 2688)]
BIG_CASE = ("iso", [.6], 6700, 8, 6708)

"""
A plain restatement, in numpy.longdouble, of what PrefGaussianProcess.addPreferences computes: the MAP functional of the
reference (ego/gaussianprocess/__init__.py:355-386), its smooth twin, the stationarity equation the product states, an independent
Newton iteration to the unique minimiser, and the model steps after the MAP (:445-498, :502-519).  tests/test_pref_reference.py pins
it to the oracle without a GPU; tests/test_gpu_pref_model.py holds the product against it.

Notation.  A triple (x_v, x_u, d) says "x_v is preferred to x_u with degree d"; pref_index numbers the distinct points.  With
z_p = (y_v - y_u) / sqrt 2, w_p = d_p + 1 and t = 0.707106 z (the reference's truncated 1 / sqrt 2):

    S_ref(y)    = -sum_p w_p log(Phi_NR(z_p) + 1e-10) + y^T R^-1 y / 2,   Phi_NR(z) = (1 + erf_NR(t)) / 2     (:355-386)
    S_smooth(y) = the same with Phi(z) = erfc(-t) / 2, the exact function the NR polynomial approximates
    pdf(z)      = 0.707106 / sqrt(pi) exp(-t^2) = dPhi/dz exactly, so
    grad S_smooth = R^-1 y - A (w pdf / (Phi + 1e-10)) / sqrt 2,          A = the n x P matrix with columns e_v - e_u
    grad_stated   = R^-1 y - A (w pdf / (Phi_NR + 1e-10)) / sqrt 2        (what _S_terms returns; the zero _map_newton looks for)
    Hess S_smooth = R^-1 + A diag(rho) A^T,  rho = w (2 * 0.707106 t q + q^2) / 2,  q = pdf / (Phi + 1e-10)

rho > 0 wherever Phi >> 1e-10 (z > -6), so S_smooth is strictly convex there (Hessian >= R^-1) and has one minimiser y*.

Precision.  Vectors, R and every O(n^2) product are long double (64-bit mantissa); erfc comes from mpmath at 100 bits.  The O(n^3)
parts (Cholesky of R, the Newton solve) are LAPACK in float64: R^-1 y is then refined with long-double residuals until the
correction stops shrinking (at about cond(R) 2^-64 of the solution; it must be below 1e-13), and the Newton iteration is driven by the long-double gradient, so the float64 solve
only affects how fast it converges, not where.
"""
import numpy as np
from scipy.linalg import cho_factor, cho_solve

LD = np.longdouble
SQRT2 = np.sqrt(LD(2))
ISQ2 = LD(0.707106)                      # the reference's 1 / sqrt 2
EPS_CDF = LD(1e-10)
NR_COEF = (-0.82215223, 1.48851587, -1.13520398, 0.27886807, -0.18628806, 0.09678418, 0.37409196, 1.00002368)


# ------------------------------------------------------------------------------------------------ scalar functions
def erf_nr(z):
    """the Numerical-Recipes erf of ego/gaussianprocess/__init__.py:55-69, in the precision of z"""
    z = np.asarray(z)
    T = z.dtype.type
    t = 1 / (1 + T(0.5) * np.abs(z))
    poly = T(0.17087277)
    for c in NR_COEF:
        poly = T(c) + t * poly
    ans = 1 - t * np.exp(-z * z - T(1.26551223) + t * poly)
    return np.where(z >= 0, ans, -ans)


def cdf_nr(x):
    x = np.asarray(x)
    return x.dtype.type(0.5) * (1 + erf_nr(x * x.dtype.type(0.707106)))


def pdf_nr(x):
    """:75-77, the density the C-matrix weights use (truncated 1 / sqrt(2 pi))"""
    x = np.asarray(x)
    return np.exp(-(x * x / 2)) * x.dtype.type(0.398942)


def _erfc_ld(t):
    """erfc of a long-double array, from mpmath at 100 bits (exact to long-double rounding, tails included)"""
    import mpmath
    t = np.asarray(t, dtype=LD)
    out = np.empty(t.shape, dtype=LD)
    with mpmath.workprec(100):
        for i, x in enumerate(t.ravel()):
            hi = float(x)
            m = mpmath.erfc(mpmath.mpf(hi) + mpmath.mpf(float(x - LD(hi))))
            mh = float(m)
            out.flat[i] = LD(mh) + LD(float(m - mh))
    return out


def _pi_ld():
    import mpmath
    with mpmath.workprec(100):
        p = +mpmath.pi
        h = float(p)
        return LD(h) + LD(float(p - h))


_PI = _pi_ld()


def cdf_exact(x):
    """Phi of the module docstring: (1 + erf(0.707106 x)) / 2 with the exact erf"""
    return _erfc_ld(-(np.asarray(x, dtype=LD) * ISQ2)) / 2


def pdf_z(z):
    t = np.asarray(z, dtype=LD) * ISQ2
    return ISQ2 / np.sqrt(_PI) * np.exp(-t * t)


def nr_constants(lo=-8.0, hi=8.0, m=4001):
    """(sup over a grid of |Phi_NR - Phi|, the jump Phi_NR(0-) - Phi_NR(0+)) in long double.  The jump comes from the NR
    coefficients summing to 1.26551226 against the constant 1.26551223: erf_NR(0+) = 1 - exp(3e-8) = -3e-8 = -erf_NR(0-)."""
    x = np.linspace(LD(lo), LD(hi), m)
    x = x[x != 0]
    sup = np.max(np.abs(cdf_nr(x) - cdf_exact(x)))
    tiny = LD(2) ** -60
    jump = cdf_nr(np.array([-tiny]))[0] - cdf_nr(np.array([tiny]))[0]
    return sup, jump


# ------------------------------------------------------------------------------------------------ kernels
def corr_matrix(kind, hyper, X, noise, X2=None):
    """R (or the cross-covariance to X2) in long double from the formulas of oracle.Kern.cov; diagonal 1 + noise for R
    (_computeCorrelations :134-149 never calls the kernel for i == j)"""
    hyper = np.asarray(hyper, dtype=LD)
    A = np.asarray(X, dtype=LD)
    B = A if X2 is None else np.asarray(X2, dtype=LD)
    diff = A[:, None, :] - B[None, :, :]
    sf2 = LD(1)
    if kind in ("svard", "sviso", "m3", "m5"):
        sf2 = np.exp(2 * np.log(hyper[-1]))
    if kind in ("ard", "svard"):
        th = np.clip(hyper if kind == "ard" else hyper[:-1], LD(1e-4), LD(1e4))
        K = np.exp(-(diff * diff / (th * th)).sum(-1) / 2)
    elif kind in ("iso", "sviso"):
        K = np.exp(-(diff * diff).sum(-1) / (hyper[0] * hyper[0]) / 2)
    elif kind == "m3":
        z = np.sqrt(LD(3)) * np.sqrt((diff * diff).sum(-1)) / hyper[0]
        K = (1 + z) * np.exp(-z)
    elif kind == "m5":
        z = 5 * (diff * diff).sum(-1) / (hyper[0] * hyper[0])
        K = np.exp(-np.sqrt(z)) * (1 + np.sqrt(z) + z / 3)
    else:
        raise ValueError(kind)
    K = sf2 * K
    if X2 is None:
        K[np.diag_indices(len(A))] = LD(1) + LD(noise)
    return K


def pair_matrix(n, v, u, w, dtype=float):
    """A diag(w) A^T, dense"""
    M = np.zeros((n, n), dtype=dtype)
    np.add.at(M, (v, v), w); np.add.at(M, (u, u), w); np.add.at(M, (v, u), -w); np.add.at(M, (u, v), -w)
    return M


# ------------------------------------------------------------------------------------------------ the MAP problem
class PrefProblem(object):
    """the MAP problem of one preference set: points and index triples from oracle.pref_index, R in long double"""

    def __init__(self, kind, hyper, prefs, noise=0.1):
        from oracle import oracle as orc
        self.kind, self.hyper, self.noise = kind, np.asarray(hyper, dtype=float), float(noise)
        self.X, self.inds, self.preferred = orc.pref_index(prefs)
        self.n = len(self.X)
        self.v = np.array([i[0] for i in self.inds], dtype=int)
        self.u = np.array([i[1] for i in self.inds], dtype=int)
        self.w = np.array([i[2] + 1.0 for i in self.inds], dtype=LD)          # degree weight d + 1 (:381)
        self.R = corr_matrix(kind, hyper, self.X, noise)
        self.R64 = self.R.astype(float)
        self._cho = cho_factor(self.R64, lower=True)
        self._Rinv64 = None

    def start(self):
        """the start vector of a first addPreferences call (:408-427): .5 for a point that is ever preferred, -.5 otherwise"""
        return np.array([.5 if i in self.preferred else -.5 for i in range(self.n)])

    def rinv_mul(self, y):
        """R^-1 y in long double: float64 Cholesky solve, refined with long-double residuals"""
        y = np.asarray(y, dtype=LD)
        x = cho_solve(self._cho, y.astype(float)).astype(LD)
        last = LD(np.inf)
        for _ in range(12):
            r = y - self.R.dot(x)
            dx = cho_solve(self._cho, r.astype(float)).astype(LD)
            size = np.max(np.abs(dx))
            if not size < last / 2:                  # the correction has reached the rounding of the long-double residual
                break
            x = x + dx
            last = size
        if last > LD(1e-13) * max(np.max(np.abs(x)), LD(1e-300)):
            raise RuntimeError("refinement of R^-1 y did not converge")
        return x

    def rinv64(self):
        if self._Rinv64 is None:
            self._Rinv64 = cho_solve(self._cho, np.eye(self.n))
        return self._Rinv64

    def z(self, y):
        y = np.asarray(y, dtype=LD)
        return (y[self.v] - y[self.u]) / SQRT2

    def _scatter(self, gz):
        g = np.zeros(self.n, dtype=LD)
        np.add.at(g, self.v, gz); np.add.at(g, self.u, -gz)
        return g

    def S_ref(self, y):
        y = np.asarray(y, dtype=LD)
        return -np.sum(self.w * np.log(cdf_nr(self.z(y)) + EPS_CDF)) + y.dot(self.rinv_mul(y)) / 2

    def S_smooth(self, y, Ry=None):
        y = np.asarray(y, dtype=LD)
        Ry = self.rinv_mul(y) if Ry is None else Ry
        return -np.sum(self.w * np.log(cdf_exact(self.z(y)) + EPS_CDF)) + y.dot(Ry) / 2

    def grad_smooth(self, y, Ry=None):
        z = self.z(y)
        Ry = self.rinv_mul(y) if Ry is None else Ry
        return Ry + self._scatter(-self.w * pdf_z(z) / (cdf_exact(z) + EPS_CDF) / SQRT2)

    def grad_stated(self, y):
        z = self.z(y)
        return self.rinv_mul(y) + self._scatter(-self.w * pdf_z(z) / (cdf_nr(z) + EPS_CDF) / SQRT2)

    def rho_smooth(self, y):
        z = self.z(y)
        q = pdf_z(z) / (cdf_exact(z) + EPS_CDF)
        return self.w * (2 * ISQ2 * (ISQ2 * z) * q + q * q) / 2

    def hessian(self, y):
        """Hess S_smooth at y, float64"""
        return self.rinv64() + pair_matrix(self.n, self.v, self.u, self.rho_smooth(y).astype(float))

    def delta_nr(self, y):
        """sum_p w_p |log(Phi_NR + 1e-10) - log(Phi + 1e-10)| at y: how far S_ref and S_smooth can differ there"""
        z = self.z(y)
        return np.sum(self.w * np.abs(np.log(cdf_nr(z) + EPS_CDF) - np.log(cdf_exact(z) + EPS_CDF)))

    def jump_allowance(self, y, reach, jump):
        """extra allowance for pairs whose z at y lies within `reach` of the NR jump at 0: (for the gradient) w pdf jump / Phi^2 /
        sqrt 2 summed over those pairs, (for S) w jump / Phi; both zero when no pair is that close"""
        z = self.z(y)
        near = np.abs(z) <= reach
        if not near.any():
            return LD(0), LD(0), 0
        phi = cdf_exact(z[near])
        return (np.sum(self.w[near] * pdf_z(z[near]) * jump / (phi * phi)) / SQRT2, np.sum(self.w[near] * jump / phi), int(near.sum()))

    def minimise(self, start=None, tol=1e-12, maxit=50):
        """Newton on S_smooth in long double to |grad|_inf <= tol max(1, |y|_inf) -> (y*, steps, H* in float64).  The direction comes
        from a float64 solve with the exact Hessian; an Armijo halving guards the first steps."""
        y = np.array(self.start() if start is None else start, dtype=LD)
        Ry = self.rinv_mul(y)
        g = self.grad_smooth(y, Ry)
        steps = 0
        while np.max(np.abs(g)) > LD(tol) * max(LD(1), np.max(np.abs(y))):
            if steps == maxit:
                raise RuntimeError("the reference Newton iteration did not converge")
            rho = self.rho_smooth(y)
            if not np.all(rho > 0):
                raise RuntimeError("a Hessian weight is not positive: S_smooth is not convex here")
            d = -np.linalg.solve(self.hessian(y), g.astype(float)).astype(LD)
            Rd = self.rinv_mul(d)
            S = self.S_smooth(y, Ry)
            t = LD(1)
            gd = g.dot(d)
            # the halving is for the first steps only: once the predicted decrease is within 1e4 long-double ulps of S the
            # comparison could not resolve it, and Newton's full step is taken (quadratic convergence does the rest)
            while -gd > LD(1e4) * np.finfo(LD).eps * abs(S) and self.S_smooth(y + t * d, Ry + t * Rd) > S + LD(1e-4) * t * gd:
                t = t / 2
                if t < LD(1e-12):
                    raise RuntimeError("the reference line search failed")
            y = y + t * d
            Ry = self.rinv_mul(y)
            g = self.grad_smooth(y, Ry)
            steps += 1
        if not np.all(self.rho_smooth(y) > 0):
            raise RuntimeError("a Hessian weight is not positive at the minimiser")
        return y, steps, self.hessian(y)


# ------------------------------------------------------------------------------------------------ after the MAP
def order_fixup(Y, inds):
    """:445-457: a preferred point that did not come out above its partner is lifted to partner + .1, but only if it is never the
    unpreferred one of any triple -> (Y, number of lifts)"""
    Y = np.array(Y, dtype=float)
    unpreferred = set(u for _, u, _ in inds)
    fired = 0
    for v, u, _ in inds:
        if Y[v] <= Y[u] and v not in unpreferred:
            Y[v] = Y[u] + .1
            fired += 1
    return Y, fired


def laplace_weights(prob, Y, dtype=float):
    """:459-486: mu at the points from L = chol(R) (no prior), then one weight per pair with pdf and cdf both floored at 1e-10"""
    T = dtype
    R = prob.R if dtype is LD else prob.R64
    kdiag = corr_matrix(prob.kind, prob.hyper, prob.X[:1], 0.0, prob.X[:1])[0, 0]
    K = R.copy()
    K[np.diag_indices(prob.n)] = T(kdiag)                      # k(x_i, x_i), not the 1 + noise of R's diagonal
    Ry = prob.rinv_mul(Y) if dtype is LD else cho_solve(prob._cho, np.asarray(Y, dtype=float))
    mu = K.dot(Ry)
    d = (mu[prob.v] - mu[prob.u]) / (np.sqrt(T(2)) * np.sqrt(T(prob.noise)))
    cdf = np.maximum(cdf_nr(d), T(1e-10))
    pdf = np.maximum(pdf_nr(d), T(1e-10))
    return 1 / (2 * T(prob.noise)) * (pdf ** 2 / cdf ** 2 + d * pdf / cdf)


def model_steps(prob, Y):
    """:459-498 in float64 as the reference runs them: C = 5 I + A diag(w) A^T, inv by LU, L = chol(R + C^-1), one identity added
    to C for every failed factorisation -> dict(w, C, identities, Cinv, M, L)"""
    w = laplace_weights(prob, Y)
    C = np.eye(prob.n) * 5 + pair_matrix(prob.n, prob.v, prob.u, w)
    for k in range(11):
        Cinv = np.linalg.inv(C)
        M = prob.R64 + Cinv
        try:
            L = np.linalg.cholesky(M)
            return dict(w=w, C=C, identities=k, Cinv=Cinv, M=M, L=L)
        except np.linalg.LinAlgError:
            C = C + np.eye(prob.n)
    raise np.linalg.LinAlgError("R + C^-1 could not be factored")


def refine_inverse(C, Cinv64):
    """C^-1 to long-double accuracy from a float64 inverse: Newton-Schulz steps X <- X (2 I - C X) in long double"""
    C = np.asarray(C, dtype=LD)
    X = np.asarray(Cinv64, dtype=LD)
    I2 = 2 * np.eye(len(C), dtype=LD)
    for _ in range(3):
        X = X.dot(I2 - C.dot(X))
    return X


def cholesky_ld(M):
    """Cholesky factor in long double (column by column; for the accuracy figures of the small-noise cases, n of a few hundred)"""
    M = np.array(M, dtype=LD)
    n = len(M)
    L = np.zeros((n, n), dtype=LD)
    for j in range(n):
        s = M[j, j] - L[j, :j].dot(L[j, :j])
        if not s > 0:
            raise np.linalg.LinAlgError("not positive definite")
        L[j, j] = np.sqrt(s)
        L[j + 1:, j] = (M[j + 1:, j] - L[j + 1:, :j].dot(L[j, :j])) / L[j, j]
    return L


def _fwd_ld(L, B):
    """L^-1 B by forward substitution in long double"""
    X = np.array(B, dtype=LD)
    for i in range(len(L)):
        X[i] = (X[i] - L[i, :i].dot(X[:i])) / L[i, i]
    return X


def reference_accuracy(prob, steps, Y, Q):
    """how accurate the reference's own float64 results are at this model: max |float64 - long double| of C^-1, L and the posterior
    mean and (unclamped) variance at the points Q -> dict(Cinv, L, mu, s2)"""
    Cinv = refine_inverse(steps["C"], steps["Cinv"])
    L = cholesky_ld(prob.R + Cinv)
    k = corr_matrix(prob.kind, prob.hyper, prob.X, 0.0, Q)
    out = []
    for Lx, T in ((L, LD), (steps["L"], float)):
        Lr = _fwd_ld(Lx, k) if T is LD else np.linalg.solve(Lx, k.astype(float))
        Ld = _fwd_ld(Lx, np.asarray(Y, dtype=LD)) if T is LD else np.linalg.solve(Lx, np.asarray(Y, dtype=float))
        out.append((Lr.T.dot(Ld), (1 + T(prob.noise)) - (Lr * Lr).sum(0)))
    return dict(Cinv=float(np.max(np.abs(Cinv - steps["Cinv"]))), L=float(np.max(np.abs(L - steps["L"]))),
                mu=float(np.max(np.abs(out[0][0] - out[1][0]))), s2=float(np.max(np.abs(out[0][1] - out[1][1]))))


def add_observation(prob, steps, augX):
    """:502-519: augR over the model's points followed by the new ones, C^-1 padded with zeros, augL = chol(augR + C^-1)"""
    augR = corr_matrix(prob.kind, prob.hyper, augX, prob.noise).astype(float)
    A = augR.copy()
    A[:prob.n, :prob.n] += steps["Cinv"]
    return augR, np.linalg.cholesky(A)


def oracle_model(prob, Y, L, M=None, X=None):
    """an oracle.GP over X (the model's points by default) whose factor is L (of M): its posteriors() is the reference's posterior,
    oracle.sweep_native on it the reference's native acquisition"""
    from oracle import oracle as orc
    X = prob.X if X is None else X
    Yp = np.zeros(len(X)); Yp[:len(Y)] = Y
    gp = orc.GP(orc.Kern(prob.kind, prob.hyper), X, Yp, noise=prob.noise)
    gp.L = np.array(L)
    gp.M = gp.L.dot(gp.L.T) if M is None else np.array(M)
    return gp

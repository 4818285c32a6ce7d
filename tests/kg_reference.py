"""
The knowledge gradient of ibo_kg_sweep / ibo_kg_batch / ibo_kg_direct_max restated in NumPy/SciPy (float64), for
tests/test_gpu_knowledge_gradient.py; pinned by tests/test_kg_reference.py to piecewise quadrature, to the oracle (a refit with the
fantasised observation moves every reference mean by b_a z) and to its own long-double evaluation.

For a grad_reference.RefGP with R = K(X, X; sf2), diagonal 1 + noise, reference points A and candidates x, k* with sf2k:
    mu_a  = m + k*_a.aY - m k*_a.a1                  (m: the mean prior at a; k*_a.aY without one)
    s2_x  = clip(1 + noise - k*_x^T R^-1 k*_x, clamp_lo, 10),   sigma_x = sqrt(s2_x)
    b_a(x) = (k(a, x) - k*_a^T R^-1 k*_x) / sigma_x
    line 0 (with_self): mu_x, b_0 = max(1 - k*_x^T R^-1 k*_x, 0) / sigma_x; the reference lines follow
    KG(x) = max(E_Z[max_i (mu_i + b_i Z)] - max_i mu_i, 0)
The expected maximum is NOT computed the way the device does it (its pair scan, ibo_abi.h): the lines are sorted by slope, equal
slopes keep their highest line, the upper envelope is built with a stack, and each surviving line k contributes
(mu_k - mu*) (Phi(z_k+1) - Phi(z_k)) + b_k (phi(z_k) - phi(z_k+1)) between its breakpoints.  `scale` is the sum of the absolute
values of those terms plus max |b|: the yardstick of the tests' tolerances.

dtype=np.longdouble evaluates the envelope in long double (erf through mpmath), and slopes(.., dtype=np.longdouble) refines the
float64 Cholesky solves against residuals formed in long double (three steps: the solves are then exact to about 1e-19 times the
condition number; R in long double is formed once per model).  The restatement's own error is the worst gap between the two over
all 14 of the GPU test's CASES, measured by test_kg_reference.py::test_own_error_is_far_below_the_gpu_bars -- the twelve cases up to
700 rows whole, the two 4100-row models on every fifth reference point and every eighth candidate (12 and 8, observations and box
points, near and far candidates alike: a long-double residual there costs 4100^2 products per column) -- as a share of the GPU bar
of each quantity:
    mu 4.5e-06 of its bar, s2 2.2e-08, b 9e-06, KG 4e-09      (the 4100-row cases: mu 8.9e-08, s2 2.2e-08, b 9e-06, KG 1.6e-09)
so every GPU bar sits far more than 10 x above the restatement's error (the test asserts a share of at most 0.1).
"""
import numpy as np
from scipy.linalg import cho_solve
from scipy.special import erf

import cov_reference as cr
import grad_reference as gr

CLAMP_PY = 1e-7

# The GPU test's cases: (kind, D, N, n, M, prior, with_self) -- every kernel kind, every side of the 64-tiles and of the 32-wide k-step
# in N, n and M, one- and 64-dimensional inputs, two models beyond 4096 rows.  Noise 0.1.
CASES = [
    ("ard", 1, 1, 1, 1, False, 1), ("iso", 3, 2, 2, 63, True, 1), ("svard", 3, 63, 63, 64, False, 0), ("sviso", 8, 64, 64, 65, True, 1),
    ("m3", 3, 65, 65, 257, False, 1), ("m5", 8, 700, 257, 63, True, 0), ("ard", 8, 700, 1024, 65, False, 1),
    ("iso", 64, 65, 64, 1000, False, 1), ("svard", 64, 700, 63, 257, True, 1), ("m3", 8, 4100, 65, 64, False, 1),
    ("m5", 3, 63, 2, 1000, False, 0), ("sviso", 1, 700, 257, 257, False, 1), ("ard", 3, 4100, 64, 65, True, 0),
    ("m5", 64, 64, 1024, 1, False, 1),
]


def ref_points(X, n, seed=5):
    """n reference points: half of them observations (repeated where there are fewer than that), half spread over the box"""
    rs = np.random.RandomState(seed)
    D = X.shape[1]
    obs = X[rs.randint(0, len(X), (n + 1) // 2)]
    return np.r_[obs, rs.rand(n // 2, D) * 1.1 - .05][:n]


def _kmat(fam, w, sf2, A, B, dtype):
    if dtype == np.float64:
        return cr.kmat(fam, w, sf2, A, B)
    A = np.atleast_2d(A).astype(dtype); B = np.atleast_2d(B).astype(dtype)
    z = np.zeros((len(A), len(B)), dtype=dtype)
    for d in range(A.shape[1]):
        z += dtype(w[d]) * (A[:, d, None] - B[None, :, d]) ** 2
    s = dtype(sf2)
    if fam == gr.FAM_SE:
        return s * np.exp(-z / 2)
    if fam == gr.FAM_M3:
        r = np.sqrt(3 * z)
        return s * (1 + r) * np.exp(-r)
    r = np.sqrt(5 * z)
    return s * (1 + r + r * r / 3) * np.exp(-r)


def _solve(ref, B, dtype):
    """R^-1 B; in long double by refinement of the float64 factor's solves (R in long double is formed once per model and kept on it)"""
    if dtype == np.float64:
        return cho_solve(ref.cf, B)
    R = getattr(ref, "_R_ld", None)
    if R is None:
        R = _kmat(ref.fam, ref.w, ref.sf2, ref.X, ref.X, dtype)
        R[np.diag_indices_from(R)] = dtype(1) + dtype(ref.noise)
        ref._R_ld = R
    x = cho_solve(ref.cf, B.astype(np.float64)).astype(dtype)
    for _ in range(3):
        x = x + cho_solve(ref.cf, (B - R @ x).astype(np.float64)).astype(dtype)
    return x


def _means(ref, Ks, P, aY, a1, dtype):
    muY = Ks.T @ aY
    if ref.prior is None:
        return muY
    m = np.array([gr.prior_grad(ref.prior, np.asarray(p, dtype=float))[0] for p in P]).astype(dtype)
    return m + muY - m * (Ks.T @ a1)


def slopes(ref, A, X, clamp_lo=CLAMP_PY, sf2k=None, dtype=np.float64):
    """dict(mu_ref (n), mu (M), s2 (M, clipped), q (M, |v_x|^2), b (M, n), vnA (n), vnX (M): |v| of either set)"""
    sf2k = ref.sf2 if sf2k is None else sf2k
    A = np.atleast_2d(np.asarray(A, dtype=float)); X = np.atleast_2d(np.asarray(X, dtype=float))
    KA = _kmat(ref.fam, ref.w, sf2k, ref.X, A, dtype); KX = _kmat(ref.fam, ref.w, sf2k, ref.X, X, dtype)
    if dtype == np.float64:
        aY, a1 = ref.aY, ref.a1
        UA = _solve(ref, KA, dtype); UX = _solve(ref, KX, dtype)
    else:                                              # one refined solve for all the right-hand sides
        N, n = KA.shape
        U = _solve(ref, np.c_[ref.Y.astype(dtype), np.ones(N, dtype=dtype), KA, KX], dtype)
        aY, a1, UA, UX = U[:, 0], U[:, 1], U[:, 2:2 + n], U[:, 2 + n:]
    qA = np.sum(KA * UA, axis=0); q = np.sum(KX * UX, axis=0)
    raw = dtype(1) + dtype(ref.noise) - q
    s2 = np.minimum(np.maximum(raw, dtype(clamp_lo)), dtype(10))
    C = _kmat(ref.fam, ref.w, sf2k, X, A, dtype) - KX.T @ UA
    return dict(mu_ref=_means(ref, KA, A, aY, a1, dtype), mu=_means(ref, KX, X, aY, a1, dtype), s2=s2, q=q,
                b=C / np.sqrt(s2)[:, None], vnA=np.sqrt(np.maximum(qA, 0)), vnX=np.sqrt(np.maximum(q, 0)))


def _cdf_pdf(z, dtype):
    z = np.asarray(z, dtype=dtype)
    if dtype == np.float64:
        with np.errstate(invalid="ignore"):
            return 0.5 * (1.0 + erf(z / np.sqrt(2.0))), np.where(np.isinf(z), 0.0, np.exp(-(z * z / 2.0)) / np.sqrt(2.0 * np.pi))
    import mpmath
    mpmath.mp.prec = 120

    def back(r):                                       # an mpf as a long double: its float64 head and tail
        hi = float(r)
        return dtype(hi) + dtype(float(r - mpmath.mpf(hi)))

    cdf = np.empty(z.shape, dtype=dtype); pdf = np.empty(z.shape, dtype=dtype)
    for i, v in np.ndenumerate(z):
        if np.isinf(v):
            cdf[i], pdf[i] = (0, 0) if v < 0 else (1, 0)
        else:
            hi = float(v)
            t = mpmath.mpf(hi) + mpmath.mpf(float(v - dtype(hi)))
            cdf[i] = back(mpmath.ncdf(t)); pdf[i] = back(mpmath.npdf(t))
    return cdf, pdf


def emax(mu, b, dtype=np.float64):
    """(E_Z max_i (mu_i + b_i Z) - max_i mu_i, scale) of the lines (mu_i, b_i) by the sorted upper envelope; the value is not clipped at 0"""
    mu = np.asarray(mu, dtype=dtype); b = np.asarray(b, dtype=dtype)
    mu = mu - np.max(mu)
    order = np.lexsort((-mu, b))                       # slope ascending, the highest line of a slope first
    mu, b = mu[order], b[order]
    keep = np.r_[True, b[1:] != b[:-1]]
    mu, b = mu[keep], b[keep]
    hull, start = [], []                               # lines on the envelope and where each takes over
    for k in range(len(mu)):
        z = -np.inf
        while hull:
            t = hull[-1]
            z = (mu[t] - mu[k]) / (b[k] - b[t])
            if z <= start[-1]:
                hull.pop(); start.pop()
                z = -np.inf
            else:
                break
        hull.append(k); start.append(dtype(z))
    lo = np.array(start, dtype=dtype); hi = np.r_[lo[1:], dtype(np.inf)]
    Pl, pl = _cdf_pdf(lo, dtype); Ph, ph = _cdf_pdf(hi, dtype)
    h = np.array(hull)
    t1 = mu[h] * (Ph - Pl); t2 = b[h] * (pl - ph)
    return np.sum(t1 + t2), np.sum(np.abs(t1) + np.abs(t2)) + np.max(np.abs(b))


def lines(mu_ref, mu_x, s2_x, b0, b_row, with_self):
    """the (mu, b) of one candidate's lines in the ABI's order"""
    if with_self:
        return np.r_[mu_x, mu_ref], np.r_[b0, b_row]
    return np.asarray(mu_ref), np.asarray(b_row)


def compose(mu_ref, mu, s2, b, noise, with_self, dtype=np.float64, b0=None):
    """(KG (M), scale (M)) from slopes; b0 defaults to max(s2 - noise, 0) / sigma, which is max(1 - |v|^2, 0) / sigma wherever
    the clip of s2 is not active and 0 at the lower clip (noise > clamp_lo)"""
    M = len(mu)
    kg = np.empty(M, dtype=dtype); sc = np.empty(M, dtype=dtype)
    if b0 is None:
        b0 = np.maximum(np.asarray(s2) - noise, 0) / np.sqrt(s2)
    for x in range(M):
        v, sc[x] = emax(*lines(mu_ref, mu[x], s2[x], b0[x], b[x], with_self), dtype=dtype)
        kg[x] = max(v, 0)
    return kg, sc


def kg(ref, A, X, with_self=True, clamp_lo=CLAMP_PY, sf2k=None, dtype=np.float64):
    """dict: slopes' entries + kg (M), scale (M)"""
    s = slopes(ref, A, X, clamp_lo, sf2k, dtype)
    b0 = np.maximum(1 - s["q"], 0) / np.sqrt(s["s2"])
    s["kg"], s["scale"] = compose(s["mu_ref"], s["mu"], s["s2"], s["b"], ref.noise, with_self, dtype, b0=b0)
    return s


# ---- the GPU test's bars, from the restatement's own quantities
def tol_mu(mu):
    return 1e-6 * np.abs(mu) + 1e-9


def tol_b(s, sf2, noise):
    """(M, n): [1e-10 (sf2 + noise + |v_a| |v_x|) + 1e-6 |b|] / sigma_x -- Sigma's bar carried through the division"""
    return (1e-10 * (sf2 + noise + np.outer(s["vnX"], s["vnA"])) + 1e-6 * np.abs(s["b"])) / np.sqrt(s["s2"])[:, None]


def tol_kg(s, sf2, noise, with_self):
    """(M,): 2 max_i tol_mu_i + 0.8 max_a tol_b_a + 1e-12 scale: the Lipschitz bound of E max in (mu, b), E|Z| ~ 0.8"""
    tm = np.max(tol_mu(s["mu_ref"]))
    tm = np.maximum(tm, tol_mu(s["mu"])) if with_self else np.full(len(s["mu"]), tm)
    return 2 * tm + 0.8 * np.max(tol_b(s, sf2, noise), axis=1) + 1e-12 * s["scale"]


def case_ref(kind, D, N, prior, seed=1, noise=.1):
    """(X, Y, hyper, prior object or None, RefGP) of a case: the model of tests/test_gpu_posterior_cov.py, the RefGP with its prior"""
    import test_gpu_posterior_cov as pc
    from conftest import synth
    X, Y = synth(seed, N, D)
    hyper = pc.hyper_of(kind, D)
    p = pc.make_prior(D) if prior else None
    fam, w, sf2 = gr.kernel_spec(kind, hyper, D)
    tup = (p.means, p.beta, p.theta, p.lowerb, p.width) if prior else None
    return X, Y, hyper, p, gr.RefGP(X, Y, noise, fam, w, sf2, prior=tup)

"""
A GP observed with gradients (csrc/gradobs.h, ibo_ggp_* in include/ibo_abi.h) restated in NumPy, for tests/test_gpu_gradobs.py (CASES)
and tests/test_gpu_gradobs_routes.py (EDGE_CASES); pinned to mpmath differentiation of the kernels' defining formulas, to the oracle
and to long double by tests/test_gradobs_reference.py.

Rows are point-major: row i (D + 1) is the value at x_i, rows i (D + 1) + d (d = 1 .. D) are df/dx_d at x_i; P = N (D + 1).  For an
oracle.Kern (w_d = 1 / theta_d^2, sf2 = sf2_py), u = x - x' (x the row's point, x' the column's), z = sum_d w_d u_d^2, t_d = w_d u_d:
    SE          k = sf2 exp(-z / 2)                           g1 = k                            g2 = k
    Matern-3/2  r = sqrt(3 z),  k = sf2 (1 + r) exp(-r)       g1 = 3 sf2 exp(-r)                g2 = 3 g1 / r  (0 at r = 0)
    Matern-5/2  r = sqrt(5 z),  k = sf2 (1 + r + r^2/3) e^-r  g1 = 5/3 sf2 (1 + r) exp(-r)      g2 = 25/3 sf2 exp(-r)
    block = [ k          g1 t_e                        ]      (value, d/dx'_e)
            [ -g1 t_d    g1 w_d delta_de - g2 t_d t_e  ]      (d/dx_d, d2/dx_d dx'_e)
Diagonal of A: 1 + noise on a value row, g1(0) w_d + gnoise_d on derivative row d.  Posterior at q: k*(q) = (k(q, x_i), g1 t_d with
u = q - x_i), mu = k*.alpha with alpha = A^-1 [Y; G] interleaved, s2 = (1 + noise) - |L^-1 k*|^2 clipped to [clamp_lo, 10].
Two precisions: float64 (numpy's Cholesky, scipy's triangular solves) and np.longdouble (nlml_reference's column Cholesky and a forward
substitution carried in long double).
"""
import functools
import math

import numpy as np

from oracle import oracle as orc

CLAMP_PY, CLAMP_NATIVE = 10e-8, 1e-8
ACQ_EI, ACQ_PI, ACQ_UCB, ACQ_NONE = 0, 1, 2, 3
ERF_LIBM, ERF_NR = 0, 1

# (name, oracle kind, hyper, N, D, noise, coincident pair or None): the shared case list.  Data in the unit cube, signals of magnitude <= 1.
CASES = [
    ("se_1x1", "iso", [0.5], 1, 1, 0.1, None),                       # smallest model, P = 2
    ("m3_21x2", "m3", [0.6, 0.9], 21, 2, 0.1, None),                 # P = 63: one below the 64-row tile
    ("ard_16x3", "ard", [0.5, 0.7, 0.6], 16, 3, 0.1, None),          # P = 64: exactly one tile
    ("ard_13x4", "ard", [0.6, 0.8, 0.7, 0.9], 13, 4, 0.1, None),     # P = 65: one above a tile
    ("iso_32x3", "iso", [0.6], 32, 3, 0.1, None),                    # P = 128: exactly two tiles
    ("m5_43x2", "m5", [0.5, 0.9], 43, 2, 0.1, None),                 # P = 129: one above two tiles
    ("m5_9x16", "m5", [2.0, 1.0], 9, 16, 0.1, None),                 # P = 153: large D
    ("ard_60x4", "ard", [0.6, 0.8, 0.7, 0.9], 60, 4, 0.01, None),    # P = 300: low noise
    ("ard_205x4", "ard", [0.6, 0.8, 0.7, 0.9], 205, 4, 0.1, None),   # P = 1025: across the kernels' 1024-element chunks
    ("m3_10x2_twin", "m3", [0.6, 0.9], 10, 2, 0.1, (2, 5)),          # two coincident training points (r = 0 off the diagonal)
]
CASE_NAMES = [c[0] for c in CASES]
QUERY_COUNTS = (1, 63, 64, 65, 130)
GNOISE = 1e-4                     # the constructor's default, tiled to D

# (name, oracle kind, hyper, N, D, noise, gnoise -- a number or one entry per dimension --, coincident pair or None): the cases of
# tests/test_gpu_gradobs_routes.py.  A case of more than BIG_ROWS rows is BIG: never cached, held to float64, and admissible only with
# cond_upper <= 1e6 (tests/test_gradobs_reference.py asserts it), where the bars' factor 1e-15 max(cond, 1e6) is its floor 1e-9.
BIG_ROWS = 2000
EDGE_CASES = [
    ("ard_257x1", "ard", [0.5], 257, 1, 0.1, 1e-4, None),                          # P = 514: the second k* block holds one point and the pad
    ("m5_300x2", "m5", [0.5, 0.9], 300, 2, 0.1, 1e-4, None),                       # P = 900: the k* block border falls inside a store pass
    ("m3_513x1", "m3", [0.6, 0.9], 513, 1, 0.1, 0.02, (2, 400)),                   # P = 1026: three k* blocks, r = 0 across blocks
    ("ard_60x3_gn", "ard", [0.5, 0.7, 0.6], 60, 3, 0.1, [1e-4, 3e-3, 0.05], None), # a gnoise of its own per dimension
    ("sviso_20x2", "sviso", [0.6, 0.9], 20, 2, 0.1, 1e-4, None),                   # SE with sf2 = 0.81
    ("se_3x64", "iso", [4.0], 3, 64, 0.1, 1e-4, None),                             # D = IBO_DMAX
    ("ard_525x3", "ard", [0.5, 0.7, 0.6], 525, 3, 0.1, 0.05, None),                # P = 2100: 33 block columns, for the forced routes
    ("ard_1008x3", "ard", [0.5, 0.7, 0.6], 1008, 3, 0.1, 0.05, None),              # P = 4032: 63 block columns, the last pipelined fit
    ("ard_1009x3", "ard", [0.5, 0.7, 0.6], 1009, 3, 0.1, 0.05, None),              # P = 4036, Npad 4096: the first fit in super-panels
    ("m5_1648x3", "m5", [0.5, 0.9], 1648, 3, 0.1, 0.05, None),                     # P = 6592: 103 block columns, the last in super-panels
    ("m3_1649x3", "m3", [0.6, 0.9], 1649, 3, 0.1, 0.05, None),                     # P = 6596, Npad 6656: the first two-level fit
    ("iso_2048x3", "iso", [0.6], 2048, 3, 0.1, 0.05, None),                        # P = 8192 = IBO_GGP_MAX_ROWS
]
EDGE_NAMES = [c[0] for c in EDGE_CASES]
SMALL_EDGE_NAMES = [c[0] for c in EDGE_CASES if c[3] * (c[4] + 1) <= BIG_ROWS]
BIG_NAMES = [c[0] for c in EDGE_CASES if c[3] * (c[4] + 1) > BIG_ROWS]


def weights(kern, D):
    th = np.asarray(kern.theta, dtype=np.float64)
    return 1.0 / th ** 2 if kern.ktype == orc.K_SE_ARD else np.full(D, 1.0 / th[0] ** 2)


def factors(kern, z, dt=np.float64):
    """(k, g1, g2) from z = sum_d w_d u_d^2 (any shape)"""
    z = np.asarray(z, dtype=dt)
    sf2 = dt(kern.sf2_py)
    if kern.ktype in (orc.K_SE_ARD, orc.K_SE_ISO):
        k = sf2 * np.exp(-z / 2)
        return k, k, k
    if kern.ktype == orc.K_MATERN3:
        r = np.sqrt(3 * z)
        e = np.exp(-r)
        g1 = 3 * sf2 * e
        with np.errstate(divide="ignore", invalid="ignore"):
            g2 = np.where(r > 0, 3 * g1 / np.where(r > 0, r, 1), 0)
        return sf2 * (1 + r) * e, g1, g2.astype(dt)
    r = np.sqrt(5 * z)
    e = np.exp(-r)
    return sf2 * (1 + r + r * r / 3) * e, (dt(5) / 3) * sf2 * (1 + r) * e, (dt(25) / 3) * sf2 * e


def blocks(kern, XA, XB, dt=np.float64):
    """(nA, nB, D + 1, D + 1): the block of every pair (row point from XA, column point from XB), no diagonal rule"""
    XA = np.asarray(XA, dtype=np.float64).astype(dt); XB = np.asarray(XB, dtype=np.float64).astype(dt)
    D = XA.shape[1]
    w = weights(kern, D).astype(dt)
    u = XA[:, None, :] - XB[None, :, :]
    t = w * u
    k, g1, g2 = factors(kern, np.sum(w * u * u, axis=2), dt)
    B = np.empty(u.shape[:2] + (D + 1, D + 1), dtype=dt)
    B[:, :, 0, 0] = k
    B[:, :, 0, 1:] = g1[:, :, None] * t
    B[:, :, 1:, 0] = -g1[:, :, None] * t
    B[:, :, 1:, 1:] = g1[:, :, None, None] * np.diag(w) - g2[:, :, None, None] * (t[:, :, :, None] * t[:, :, None, :])
    return B


def tile_gnoise(gnoise, D):
    g = np.array(gnoise, dtype=np.float64, ndmin=1)
    return np.tile(g, D) if len(g) == 1 else g


def matrix(kern, X, noise, gnoise, dt=np.float64):
    """A, P x P point-major, with the diagonal rule"""
    X = np.asarray(X, dtype=np.float64)
    N, D = X.shape
    A = blocks(kern, X, X, dt).transpose(0, 2, 1, 3).reshape(N * (D + 1), N * (D + 1)).copy()
    w = weights(kern, D).astype(dt)
    g1_0 = factors(kern, dt(0), dt)[1]
    d = np.tile(np.concatenate([[dt(1) + dt(noise)], g1_0 * w + tile_gnoise(gnoise, D).astype(dt)]), N)
    A[np.diag_indices(len(A))] = d
    return A


def cond_upper(kern, X, noise, gnoise):
    """|A|_inf / min(1 + noise - sf2, min_d gnoise_d) >= cond_2(A).  A is the derivative covariance C (positive semi-definite, value
    diagonal sf2) plus the diagonal (1 + noise - sf2, gnoise_1 .. gnoise_D) per point, so lambda_min(A) >= the smallest entry of that
    diagonal (sf2 <= 1 + noise is required), and lambda_max(A) <= |A|_inf for a symmetric matrix.  Row sums in slabs of points: never
    more than a slab of A at a time."""
    X = np.asarray(X, dtype=np.float64)
    N, D = X.shape
    gn = tile_gnoise(gnoise, D)
    assert kern.sf2_py <= 1.0 + noise, "cond_upper needs sf2 <= 1 + noise"
    extra = np.concatenate([[1.0 + noise - kern.sf2_py], gn])           # what the diagonal rule adds to C's (positive) diagonal
    assert np.all(extra > 0.0)
    worst = 0.0
    for i0 in range(0, N, 64):
        rows = np.sum(np.abs(blocks(kern, X[i0:i0 + 64], X)), axis=(1, 3)) + extra[None, :]
        worst = max(worst, float(np.max(rows)))
    return worst / float(np.min(extra))


def kstar(kern, X, Q, dt=np.float64):
    """(M, P): row c holds k(q_c, x_i) and dk(q_c, x_i) / dx_i,d, point-major"""
    B = blocks(kern, Q, X, dt)
    return B[:, :, 0, :].reshape(len(B), -1).copy()


def targets(Y, G):
    """[Y; G] interleaved point by point"""
    Y = np.asarray(Y, dtype=np.float64).reshape(-1); G = np.asarray(G, dtype=np.float64).reshape(len(Y), -1)
    return np.concatenate([Y[:, None], G], axis=1).reshape(-1)


def cholesky_ld(A):
    """the lower Cholesky factor of A, column by column in long double (as nlml_reference.cholesky_ld)"""
    L = np.array(A, dtype=np.longdouble)
    for j in range(len(L)):
        if j:
            L[j:, j] -= L[j:, :j] @ L[j, :j]
        if not L[j, j] > 0:
            raise np.linalg.LinAlgError("not positive definite in column %d" % j)
        L[j, j] = np.sqrt(L[j, j])
        L[j + 1:, j] /= L[j, j]
    return np.tril(L)


def forward_ld(L, B):
    """L^-1 B (B: P x m) by forward substitution in long double"""
    V = np.array(B, dtype=np.longdouble)
    for i in range(len(L)):
        if i:
            V[i] -= L[i, :i] @ V[:i]
        V[i] /= L[i, i]
    return V


def backward_ld(L, B):
    """L^-T B"""
    V = np.array(B, dtype=np.longdouble)
    for i in range(len(L) - 1, -1, -1):
        if i + 1 < len(L):
            V[i] -= L[i + 1:, i] @ V[i + 1:]
        V[i] /= L[i, i]
    return V


def fit(kern, X, Y, G, noise, gnoise, longdouble=False):
    """dict(A, L, alpha, cond, N, D, P, kern, X, noise, dt): the factored model.  cond: cond_2 of the float64 A; of more than BIG_ROWS
    rows: cond_upper, in place of an SVD of up to 8192 rows."""
    import scipy.linalg as sl
    dt = np.longdouble if longdouble else np.float64
    X = np.asarray(X, dtype=np.float64)
    N, D = X.shape
    A = matrix(kern, X, noise, gnoise, dt)
    y = targets(Y, G).astype(dt)
    if longdouble:
        L = cholesky_ld(A)
        alpha = backward_ld(L, forward_ld(L, y[:, None]))[:, 0]
    else:
        L = np.linalg.cholesky(A)
        alpha = sl.solve_triangular(L, sl.solve_triangular(L, y, lower=True), lower=True, trans="T")
    cond = cond_upper(kern, X, noise, gnoise) if len(A) > BIG_ROWS else float(np.linalg.cond(np.asarray(A, dtype=np.float64)))
    return dict(A=A, L=L, alpha=alpha, cond=cond, N=N, D=D, P=N * (D + 1), kern=kern, X=X, noise=float(noise), dt=dt,
                maxY=float(np.max(Y)))


def posterior(m, Q, clamp_lo=CLAMP_PY):
    """dict(mu, s2, s2_raw, mu_scale = sum_j |k*_j alpha_j|, v2 = |v|^2) at the rows of Q, in the model's precision"""
    import scipy.linalg as sl
    dt = m["dt"]
    Ks = kstar(m["kern"], m["X"], np.atleast_2d(Q), dt)
    V = forward_ld(m["L"], Ks.T) if dt is np.longdouble else sl.solve_triangular(m["L"], Ks.T, lower=True)
    v2 = np.sum(V * V, axis=0)
    raw = (dt(1) + dt(m["noise"])) - v2
    return dict(mu=Ks @ m["alpha"], s2=np.clip(raw, dt(clamp_lo), dt(10)), s2_raw=raw, mu_scale=np.abs(Ks) @ np.abs(m["alpha"]), v2=v2)


def bars(m, post):
    """(bar_mu, bar_s2): 1e-15 max(cond_2, 1e6) times sum_j |k*_j alpha_j| and (1 + noise + |v|^2) -- the NLML tests' bars"""
    f = 1e-15 * max(m["cond"], 1e6)
    return f * np.asarray(post["mu_scale"], dtype=np.float64), f * (1.0 + m["noise"] + np.asarray(post["v2"], dtype=np.float64))


def erf_nr(z):
    z = np.asarray(z, dtype=np.float64)
    t = 1.0 / (1.0 + 0.5 * np.abs(z))
    p = 0.17087277
    for c in (-0.82215223, 1.48851587, -1.13520398, 0.27886807, -0.18628806, 0.09678418, 0.37409196, 1.00002368):
        p = c + t * p
    ans = 1.0 - t * np.exp(-z * z - 1.26551223 + t * p)
    return np.where(z >= 0.0, ans, -ans)


def acquisition(acq, erf_mode, mu, s2, ymax, parm):
    """acq_value_dev (csrc/ibo_common.h) on (mu, s2): EI / PI / UCB in either erf flavour, float64"""
    mu = np.asarray(mu, dtype=np.float64); sigma = np.sqrt(np.asarray(s2, dtype=np.float64))
    if acq == ACQ_NONE:
        return mu.copy()
    if acq == ACQ_UCB:
        return mu + parm * sigma
    yd = mu - ymax - parm
    Z = yd / sigma
    if erf_mode == ERF_LIBM:
        cdf = 0.5 * (1.0 + np.array([math.erf(v) for v in np.atleast_1d(Z / math.sqrt(2.0))]).reshape(np.shape(Z)))
        pdf = np.exp(-(Z * Z / 2.0)) / math.sqrt(2.0 * math.pi)
    else:
        cdf = 0.5 * (1.0 + erf_nr(Z * 0.707106))
        pdf = np.exp(-(Z * Z / 2.0)) * 0.398942
    return cdf if acq == ACQ_PI else yd * cdf + sigma * pdf


# ---------------------------------------------------------------------------- data
def objective(X):
    """a smooth function of the unit cube with |f| <= 0.5 and |df/dx_d| <= 0.85: (values, gradients)"""
    X = np.atleast_2d(np.asarray(X, dtype=np.float64))
    a = 0.6 + 1.1 * np.abs(np.sin(1.0 + np.arange(X.shape[1])))
    ph = X @ a + 0.3
    return 0.5 * np.sin(ph), 0.5 * np.cos(ph)[:, None] * a[None, :]


def points(N, D, seed):
    return np.random.RandomState(seed).rand(N, D)


def queries(X, M, seed=7):
    """M query points in the unit cube: uniform ones, with a few on and next to training points"""
    rs = np.random.RandomState(seed)
    Q = rs.rand(M, X.shape[1])
    for k in range(min(M // 8, len(X))):
        Q[8 * k] = X[k] if k % 2 == 0 else np.clip(X[k] + 1e-3, 0.0, 1.0)
    return Q


def is_big(name):
    return name in BIG_NAMES


def _make_case(name):
    if name in CASE_NAMES:
        name, kind, hyper, N, D, noise, twin = CASES[CASE_NAMES.index(name)]
        gnoise, seed = GNOISE, 100 + CASE_NAMES.index(name)
    else:
        name, kind, hyper, N, D, noise, gnoise, twin = EDGE_CASES[EDGE_NAMES.index(name)]
        seed = 200 + EDGE_NAMES.index(name)
    X = points(N, D, seed)
    if twin is not None:
        X[twin[1]] = X[twin[0]]
    Y, G = objective(X)
    for a in (X, Y, G):
        a.setflags(write=False)
    return dict(name=name, kern=orc.Kern(kind, hyper), X=X, Y=Y, G=G, noise=noise, gnoise=tile_gnoise(gnoise, D))


_cached_case = functools.lru_cache(maxsize=None)(_make_case)


def case(name):
    """dict(name, kern, X, Y, G, noise, gnoise) of a case of either list; a big one is made anew on every call"""
    return _make_case(name) if is_big(name) else _cached_case(name)


def _make_model(name, longdouble=False):
    c = case(name)
    return fit(c["kern"], c["X"], c["Y"], c["G"], c["noise"], c["gnoise"], longdouble)


_cached_model = functools.lru_cache(maxsize=None)(_make_model)


def case_model(name, longdouble=False):
    """the factored reference model of a case of either list; computed once, except a big one: float64 and made anew on every call"""
    if is_big(name):
        assert not longdouble
        return _make_model(name, False)
    return _cached_model(name, longdouble)


def reference_model(name):
    """the model the device is held to: long double wherever cond_2 > 1e6; a big case: float64 under cond_upper <= 1e6"""
    m = case_model(name, False)
    if is_big(name):
        assert m["cond"] <= 1e6, "%s is not admissible: cond_upper %.3g" % (name, m["cond"])
        return m
    return case_model(name, True) if m["cond"] > 1e6 else m

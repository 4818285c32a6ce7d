"""
The sparse GP on inducing points (ibo_sgp_* in include/ibo_abi.h) restated in NumPy, for tests/test_sparse_reference.py on the
CPU and tests/test_gpu_sparse.py on the device.  Nothing of the package under test is imported here.

k carries sf2; every diagonal counts k(x, x) as 1; noise = sigma^2, jitter = j.
    K~uu = K(Z, Z), diagonal 1 + j = L_u L_u^T, W_u = L_u^-1;  q_i = |W_u k_u(x_i)|^2
    lambda_i = sigma^2 + max(1 - q_i, 0) (fitc) or sigma^2 (dtc)
    F[a][i] = k(z_a, x_i) / sqrt(lambda_i), y~ = y / sqrt(lambda);  G = F F^T, b = F y~, yy = y~.y~, ll = sum log lambda, tt = sum max(1 - q, 0)
    A = K~uu + G = L_A L_A^T, W_A = L_A^-1, alpha = W_A^T W_A b
    mu(x) = k_u(x).alpha;  s2(x) = sigma^2 + (1 - |W_u k_u(x)|^2) + |W_A k_u(x)|^2, then clipped to [clamp_lo, 10]
    NLML = (ll + 2 sum log L_A,ii - 2 sum log L_u,ii + yy - |W_A b|^2 + N log 2 pi) / 2;  vfe = the dtc value + tt / (2 sigma^2)

Three independent forms:
    route()     the route above with EXPLICIT inverses W_u, W_A, in float64 (numpy / scipy) or long double (column Cholesky, substitution on
                the identity) -- what the device does
    dense()     the definition: Q = K_fu K~uu^-1 K_uf, S = Q_ff + Lambda; mu = Q_*f S^-1 y, s2 = 1 + sigma^2 - Q_*f S^-1 Q_f*,
                NLML = (log det S + y^T S^-1 y + N log 2 pi) / 2 from the N x N matrix.  Long double, N <= DENSE_MAX.
    whitened()  V = L_u^-1 K_uf by substitution, B = I + V Lambda^-1 V^T = L_B L_B^T; mu = v_*^T B^-1 V Lambda^-1 y,
                s2 = 1 + sigma^2 - |v_*|^2 + |L_B^-1 v_*|^2, NLML = (ll + 2 sum log L_B,ii + yy - |L_B^-1 V Lambda^-1 y|^2 + N log 2 pi) / 2

THE BARS (the project's form):
    posterior   f = 1e-15 max(cond_2(A), cond_2(K~uu), 1e6);  mu: f sum_a |k_a alpha_a|;  s2: f (1 + sigma^2 + |v_U|^2 + |v_A|^2)
    NLML        f times the sum of the terms' magnitudes, (|ll| + |2 sum log L_A| + |2 sum log L_u| + yy + |W_A b|^2 + N log 2 pi) / 2
    G, b, yy    |G_ab - ref| <= ((N + 8) u + 2 eps_k) sum_i |F_ai F_bi|, u = 2^-53.  Derivation: a term F_ai F_bi is the product of two
                entries that each carry the family's k* bar eps_k (tests/kstar_reference.py: bar_fast, taken at the largest exponent of the
                case) and three roundings of the scaling (the square root, the reciprocal, the product): relative error
                <= 2 eps_k + 6 u; the product of the two is exact inside a fused multiply-add or costs one more u; a sum of N terms in ANY
                order adds at most (N - 1) u sum |terms| (Higham, Accuracy and Stability, 4.2).  Together <= (N + 6) u + 2 eps_k, rounded
                up to N + 8.  The reference takes lambda as GIVEN (gram() below): lambda's own error is held to its own bar.
    lambda      fitc: |lambda - ref| <= 1e-12 ref + the q-bar, f_U (1 + j + q) with f_U = 1e-15 max(cond_2(K~uu), 1e6)
    Z = X       see zx_bound()
"""
import functools
import math

import numpy as np

from oracle import oracle as orc
from gradobs_reference import cholesky_ld, forward_ld, erf_nr, acquisition      # noqa: F401  (long-double column routines; the epilogue)
import kstar_reference as kr

LD = np.longdouble
U = 2.0 ** -53
CLAMP_PY, CLAMP_NATIVE = 10e-8, 1e-8
ACQ_EI, ACQ_PI, ACQ_UCB, ACQ_NONE = 0, 1, 2, 3
ERF_LIBM, ERF_NR = 0, 1
FITC, DTC = 0, 1
DENSE_MAX = 300
QUERY_COUNTS = (1, 63, 64, 65, 130)

# (name, kind, hyper, D, m, N, noise, jitter, method, Z a subset of X, shift of X and Z)
CASES = [
    ("m1_n1", "iso", [0.5], 1, 1, 1, 0.1, 1e-6, FITC, False, 0.0),
    ("m16_n200", "ard", [0.5, 0.7, 0.6], 3, 16, 200, 0.05, 1e-6, FITC, False, 0.0),
    ("m63_n1000", "m3", [0.6, 0.9], 2, 63, 1000, 0.05, 1e-6, FITC, False, 0.0),
    ("m64_n1000", "ard", [0.6, 0.8, 0.7, 0.9], 4, 64, 1000, 0.05, 1e-6, FITC, False, 0.0),       # y~ in a tile of its own
    ("m65_n1000", "m5", [0.5, 0.9], 2, 65, 1000, 0.05, 1e-6, DTC, False, 0.0),
    ("m129_n2100", "m3", [0.6, 0.9], 2, 129, 2100, 0.05, 1e-6, DTC, False, 0.0),
    ("m130_n2100", "m5", [0.7, 0.9], 3, 130, 2100, 0.05, 1e-6, FITC, False, 0.0),
    ("m100_n300_zsub", "ard", [0.5, 0.6], 2, 100, 300, 0.05, 1e-6, FITC, True, 0.0),            # lambda's clamp at q ~ 1 runs
    ("m64_n300_j8", "iso", [1.2], 5, 64, 300, 0.05, 1e-8, FITC, False, 0.0),
    ("m64_n1000_lownoise", "ard", [0.6, 0.8, 0.7, 0.9], 4, 64, 1000, 1e-4, 1e-6, FITC, False, 0.0),
    ("m64_n33", "iso", [0.6], 3, 64, 33, 0.05, 1e-6, FITC, False, 0.0),                          # N < m
    ("m64_n31", "m5", [0.6, 0.9], 3, 64, 31, 0.05, 1e-6, DTC, False, 0.0),
    ("m32_n400_shift", "ard", [0.5, 0.7, 0.6], 3, 32, 400, 0.05, 1e-6, FITC, False, 100.0),
    ("m40_n500_sf2", "sviso", [0.6, 0.9], 2, 40, 500, 0.05, 1e-6, FITC, False, 0.0),             # sf2 = 0.81
    ("m20_n150_d33", "iso", [3.0], 33, 20, 150, 0.05, 1e-6, DTC, False, 0.0),
]
CASE_NAMES = [c[0] for c in CASES]
# the route cases: above 400 inducing rows the comparator is the whitened float64 form
ROUTE_CASES = [
    ("route_m3", "m3", [0.5, 1.0], 4, 1100, 3000, 0.05, 1e-6, FITC, False, 0.0),
    ("route_se", "iso", [0.4], 6, 1100, 3000, 0.02, 1e-6, FITC, False, 0.0),
]
ROUTE_NAMES = [c[0] for c in ROUTE_CASES]
LD_MAX_M = 400


def family(kern):
    return {orc.K_SE_ARD: kr.SE, orc.K_SE_ISO: kr.SE, orc.K_MATERN3: kr.M3, orc.K_MATERN5: kr.M5}[kern.ktype]


def weights(kern, D):
    th = np.asarray(kern.theta, dtype=np.float64)
    return 1.0 / th ** 2 if kern.ktype == orc.K_SE_ARD else np.full(D, 1.0 / th[0] ** 2)


def zdist(kern, A, B, dt=np.float64):
    """z = sum_d w_d (a_d - b_d)^2 for every pair, the difference first"""
    A = np.asarray(A, dtype=np.float64).astype(dt); B = np.asarray(B, dtype=np.float64).astype(dt)
    w = weights(kern, A.shape[1]).astype(dt)
    z = np.zeros((len(A), len(B)), dtype=dt)
    for d in range(A.shape[1]):                               # (dimension by dimension: no (nA, nB, D) array)
        u = A[:, d][:, None] - B[:, d][None, :]
        z += w[d] * u * u
    return z


def kmap(kern, z, dt=np.float64):
    z = np.asarray(z, dtype=dt)
    sf2 = dt(kern.sf2_py)
    fam = family(kern)
    if fam == kr.SE:
        return sf2 * np.exp(-z / 2)
    r = np.sqrt((3 if fam == kr.M3 else 5) * z)
    return sf2 * (1 + r) * np.exp(-r) if fam == kr.M3 else sf2 * (1 + r + r * r / 3) * np.exp(-r)


def kmat(kern, A, B, dt=np.float64):
    return kmap(kern, zdist(kern, A, B, dt), dt)


def kuu(kern, Z, jitter, dt=np.float64):
    K = kmat(kern, Z, Z, dt)
    K[np.diag_indices(len(K))] = dt(1) + dt(jitter)
    return K


def _chol_inv(A, dt):
    """(L, W = L^-1 explicitly): float64 by LAPACK, long double by the column routines"""
    if dt is LD:
        L = cholesky_ld(A)
        return L, forward_ld(L, np.eye(len(L), dtype=LD))
    import scipy.linalg as sl
    L = np.linalg.cholesky(A)
    return L, sl.solve_triangular(L, np.eye(len(L)), lower=True)


def lambdas(q, noise, method, dt=np.float64):
    ex = np.maximum(dt(1) - q, dt(0))
    return (dt(noise) + ex if method == FITC else np.full(len(q), dt(noise), dtype=dt)), ex


def gram(kern, Z, X, Y, lam, dt=LD):
    """(G, b, yy, absG, absb) from GIVEN lambda: G = F F^T with F = K_uf / sqrt(lambda); abs*: sum_i |F_ai F_bi| and sum_i |F_ai y~_i|"""
    rs = 1 / np.sqrt(np.asarray(lam, dtype=np.float64).astype(dt))
    F = kmat(kern, Z, X, dt) * rs[None, :]
    yt = np.asarray(Y, dtype=np.float64).astype(dt) * rs
    return F @ F.T, F @ yt, yt @ yt, np.abs(F) @ np.abs(F).T, np.abs(F) @ np.abs(yt)


def eps_k(kern, Z, X):
    """the family's k* bar (kstar_reference.bar_fast) at the largest exponent of the case"""
    z = zdist(kern, Z, X)
    return float(np.max(kr.bar_fast(family(kern), z, kern.sf2_py)))


def gram_bar(kern, Z, X, N, absG):
    return ((N + 8) * U + 2 * eps_k(kern, Z, X)) * np.asarray(absG, dtype=np.float64)


def route(kern, Z, X, Y, noise, jitter, method, longdouble=False, prev=None):
    """The fitted model as a dict.  prev: a model to ACCUMULATE into (addData): its K~uu and factor are kept, G, b, yy, ll, tt and N grow."""
    dt = LD if longdouble else np.float64
    Z = np.asarray(Z, dtype=np.float64); X = np.asarray(X, dtype=np.float64); Y = np.asarray(Y, dtype=np.float64).reshape(-1)
    if prev is None:
        Kuu = kuu(kern, Z, jitter, dt)
        Lu, Wu = _chol_inv(Kuu, dt)
        base = dict(G=np.zeros_like(Kuu), b=np.zeros(len(Z), dtype=dt), yy=dt(0), ll=dt(0), tt=dt(0), N=0, maxY=-np.inf, lam=np.zeros(0, dtype=dt))
    else:
        Kuu, Lu, Wu, base = prev["Kuu"], prev["Lu"], prev["Wu"], prev
    Kuf = kmat(kern, Z, X, dt)
    VU = Wu @ Kuf
    q = np.sum(VU * VU, axis=0)
    lam, ex = lambdas(q, noise, method, dt)
    rs = 1 / np.sqrt(lam)
    F = Kuf * rs[None, :]
    yt = Y.astype(dt) * rs
    G = base["G"] + F @ F.T
    b = base["b"] + F @ yt
    yy = base["yy"] + yt @ yt
    ll = base["ll"] + np.sum(np.log(lam))
    tt = base["tt"] + np.sum(ex)
    N = base["N"] + len(X)
    A = Kuu + G
    LA, WA = _chol_inv(A, dt)
    wb = WA @ b
    alpha = WA.T @ wb
    ldA = 2 * np.sum(np.log(np.diag(LA))); ldU = 2 * np.sum(np.log(np.diag(Lu)))
    wb2 = wb @ wb
    c = dt(N) * np.log(2 * kr.PI_LD if longdouble else 2 * np.pi)
    nl = (ll + ldA - ldU + yy - wb2 + c) / 2
    nl_scale = (abs(ll) + abs(ldA) + abs(ldU) + yy + wb2 + c) / 2
    A64, U64 = np.asarray(A, dtype=np.float64), np.asarray(Kuu, dtype=np.float64)
    m = dict(kern=kern, Z=Z, noise=float(noise), jitter=float(jitter), method=method, dt=dt, Kuu=Kuu, Lu=Lu, Wu=Wu, q=q, lam=np.concatenate([base["lam"], lam]),
             G=G, b=b, yy=yy, ll=ll, tt=tt, N=N, A=A, LA=LA, WA=WA, alpha=alpha, wb2=wb2, nlml=nl, nlml_scale=float(nl_scale),
             vfe=(nl + tt / (2 * dt(noise))) if method == DTC else None, maxY=max(base["maxY"], float(np.max(Y))),
             condA=float(np.linalg.cond(A64)), condU=float(np.linalg.cond(U64)))
    m["f"] = 1e-15 * max(m["condA"], m["condU"], 1e6)
    return m


def posterior(m, Q, clamp_lo=CLAMP_PY):
    """dict(mu, s2, s2_raw, mu_scale, s2_scale) at the rows of Q in the model's precision; s2 composed in the device's order"""
    dt = m["dt"]
    ku = kmat(m["kern"], np.atleast_2d(Q), m["Z"], dt)                  # (M, m)
    vU = m["Wu"] @ ku.T; vA = m["WA"] @ ku.T
    qU = np.sum(vU * vU, axis=0); qA = np.sum(vA * vA, axis=0)
    raw = (dt(m["noise"]) + (dt(1) - qU)) + qA
    return dict(mu=ku @ m["alpha"], s2=np.clip(raw, dt(clamp_lo), dt(10)), s2_raw=raw, mu_scale=np.asarray(np.abs(ku) @ np.abs(m["alpha"]), dtype=np.float64),
                s2_scale=np.asarray(1.0 + m["noise"] + qU + qA, dtype=np.float64))


def bars(m, post):
    """(bar_mu, bar_s2, bar_nlml)"""
    return m["f"] * post["mu_scale"], m["f"] * post["s2_scale"], m["f"] * m["nlml_scale"]


def dense(kern, Z, X, Y, noise, jitter, method, Q):
    """the definition, in long double from the N x N matrix: dict(mu, s2_raw, nlml, vfe)"""
    X = np.asarray(X, dtype=np.float64)
    assert len(X) <= DENSE_MAX
    Lu = cholesky_ld(kuu(kern, Z, jitter, LD))
    Vf = forward_ld(Lu, kmat(kern, Z, X, LD)); Vs = forward_ld(Lu, kmat(kern, Z, np.atleast_2d(Q), LD))
    Qff = Vf.T @ Vf; Qsf = Vs.T @ Vf
    lam, ex = lambdas(np.diag(Qff).copy(), noise, method, LD)
    S = Qff + np.diag(lam)
    Ls = cholesky_ld(S)
    y = np.asarray(Y, dtype=np.float64).astype(LD)
    wy = forward_ld(Ls, y[:, None])[:, 0]
    Ws = forward_ld(Ls, Qsf.T)
    nl = (2 * np.sum(np.log(np.diag(Ls))) + wy @ wy + LD(len(X)) * np.log(2 * kr.PI_LD)) / 2
    return dict(mu=Ws.T @ wy, s2_raw=(LD(1) + LD(noise)) - np.sum(Ws * Ws, axis=0), nlml=nl,
                vfe=(nl + np.sum(ex) / (2 * LD(noise))) if method == DTC else None)


def whitened(kern, Z, X, Y, noise, jitter, method, Q, longdouble=False):
    """the whitened form: V by SUBSTITUTION, B = I + V Lambda^-1 V^T"""
    import scipy.linalg as sl
    dt = LD if longdouble else np.float64
    Kuu = kuu(kern, Z, jitter, dt)
    Lu = cholesky_ld(Kuu) if longdouble else np.linalg.cholesky(Kuu)
    solve = (lambda L, B: forward_ld(L, B)) if longdouble else (lambda L, B: sl.solve_triangular(L, B, lower=True))
    V = solve(Lu, kmat(kern, Z, X, dt))
    q = np.sum(V * V, axis=0)
    lam, ex = lambdas(q, noise, method, dt)
    Vl = V / np.sqrt(lam)[None, :]
    B = np.eye(len(Lu), dtype=dt) + Vl @ Vl.T
    LB = cholesky_ld(B) if longdouble else np.linalg.cholesky(B)
    y = np.asarray(Y, dtype=np.float64).astype(dt)
    yt = y / np.sqrt(lam)
    c = solve(LB, (Vl @ yt)[:, None])[:, 0]
    vs = solve(Lu, kmat(kern, Z, np.atleast_2d(Q), dt))
    ws = solve(LB, vs)
    nl = (np.sum(np.log(lam)) + 2 * np.sum(np.log(np.diag(LB))) + yt @ yt - c @ c + dt(len(y)) * np.log(2 * kr.PI_LD if longdouble else 2 * np.pi)) / 2
    return dict(mu=ws.T @ c, s2_raw=(dt(noise) + (dt(1) - np.sum(vs * vs, axis=0))) + np.sum(ws * ws, axis=0), nlml=nl,
                vfe=(nl + np.sum(ex) / (2 * dt(noise))) if method == DTC else None)


def exact_nlml(kern, X, Y, noise):
    """the full model's NLML (diagonal 1 + sigma^2) in long double"""
    K = kmat(kern, X, X, LD)
    K[np.diag_indices(len(K))] = LD(1) + LD(noise)
    L = cholesky_ld(K)
    wy = forward_ld(L, np.asarray(Y, dtype=np.float64).astype(LD)[:, None])[:, 0]
    return (2 * np.sum(np.log(np.diag(L))) + wy @ wy + LD(len(K)) * np.log(2 * kr.PI_LD)) / 2


def zx_bound(kern, X, Y, noise, jitter):
    """Z = X, fitc: the bound on |mu_sparse - mu_exact| and |s2_sparse - s2_exact| at the data rows.
    With K the kernel matrix of diagonal 1 and Kj = K + j I:  Q_ff = K Kj^-1 K = K - j I + j^2 Kj^-1 (from K = Kj - j I), so
    diag(Q_ff) = 1 - j + j^2 (Kj^-1)_ii <= 1 (j (Kj^-1)_ii <= 1: lambda_min(Kj) >= j), the clamp is idle, and
        Q_ff + Lambda = K + sigma^2 I + E,   E = j^2 offdiag(Kj^-1):
    the sparse model is the exact one with its matrix perturbed by E and its cross-covariance rows Q_*f = k_* - j e_i + j^2 (Kj^-1)_i.
    to first order  |d mu_i| <= |dQ_i|_2 |alpha|_2 + |k_i|_2 |S^-1|_2 |E|_2 |alpha|_2, and the variance alike with S^-1 k_i in place of alpha;
    |dQ_i|_2 <= j + j^2 |Kj^-1|_2, |E|_2 <= j^2 |Kj^-1|_2 <= j, |S^-1|_2 <= 1 / sigma^2.  A factor 2 covers the second order
    (|S^-1 E| <= j / sigma^2 << 1 is asserted)."""
    K = kmat(kern, X, X)
    K[np.diag_indices(len(K))] = 1.0
    N = len(K)
    inv_j = np.linalg.norm(np.linalg.inv(K + jitter * np.eye(N)), 2)
    S = K + noise * np.eye(N)
    alpha = np.linalg.solve(S, np.asarray(Y, dtype=np.float64))
    dq = jitter + jitter ** 2 * inv_j
    e = jitter ** 2 * inv_j
    sinv = 1.0 / noise
    assert e * sinv < 1e-2
    kn = np.linalg.norm(K, axis=1)
    na = np.linalg.norm(alpha)
    dmu = 2 * (dq * na + kn * sinv * e * na)
    sk = np.linalg.norm(np.linalg.solve(S, K), axis=0)
    ds2 = 2 * (2 * dq * sk + kn * sinv * e * sk)
    return dmu, ds2


# ---------------------------------------------------------------------------- data
def objective(X):
    return np.sin(3.0 * np.sum(np.asarray(X, dtype=np.float64), axis=1))


def _spec(name):
    for c in CASES + ROUTE_CASES:
        if c[0] == name:
            return c
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def case(name):
    """dict(kern, Z, X, Y, Q, noise, jitter, method, ...): seeded, Y = sin(3 sum x) + noise; the objective is evaluated before the shift"""
    _, kind, hyper, D, m, N, noise, jitter, method, zsub, shift = _spec(name)
    rng = np.random.RandomState(1000 + sum(ord(ch) for ch in name))
    X = rng.rand(N, D)
    Y = objective(X) + math.sqrt(noise) * rng.randn(N)
    Z = X[np.sort(rng.permutation(N)[:m])].copy() if zsub else rng.rand(m, D)
    Q = rng.rand(max(QUERY_COUNTS), D)
    if zsub:
        Q[:10] = X[:10]                                        # queries on data rows too
    return dict(name=name, kern=orc.Kern(kind, hyper), kind=kind, hyper=hyper, D=D, m=m, N=N, noise=noise, jitter=jitter, method=method,
                Z=Z + shift, X=X + shift, Y=Y, Q=Q + shift)


@functools.lru_cache(maxsize=None)
def case_model(name, longdouble=False):
    c = case(name)
    return route(c["kern"], c["Z"], c["X"], c["Y"], c["noise"], c["jitter"], c["method"], longdouble)


def device_spec(kern):
    """(ktype, hyper, sf2) as ibo_sgp_fit takes them"""
    return kern.ktype, np.ascontiguousarray(kern.theta, dtype=np.float64), float(kern.sf2_py)

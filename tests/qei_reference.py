"""
The Monte-Carlo parallel expected improvement of ibo_qei_sweep / ibo_qei_batch / ibo_qei_direct_max restated in NumPy (float64), for
tests/test_gpu_qei.py; pinned by tests/test_qei_reference.py to the oracle's EI (no pending points), to the oracle's own extension
(a refit with the pending observations drawn) and to its own long-double evaluation.

For a grad_reference.RefGP, pending points P (p of them), candidates x, base samples Z (S x (p + 1)) and t = ymax + xi:
    qEI(x | P) = (1/S) sum_s max(max_i y_si - t, 0),   y_s = mu + L z_s
over the p + 1 points (P, x): mu their posterior means (kg_reference._means), L the Cholesky factor of their joint covariance
(cov_reference.cov with with_noise = 1: Sigma_ab = k - k*_a^T R^-1 k*_b off the diagonal, 1 + noise - k*^T R^-1 k* on it), with
jitter added to the pending points' diagonal entries and the candidate's replaced by its clipped s2.
`qei` goes ANOTHER WAY than the device: it forms the full bordered (p + 1) x (p + 1) matrix per candidate, factors it whole with
np.linalg.cholesky, and takes row maxima of mu + Z L^T; the device factors S_PP once on the host and borders it per candidate by a
forward substitution (ibo_abi.h).  `compose` is the device's definition evaluated on given pieces (any dtype): L_P, l = L_P^-1 c,
d = sqrt(max(s2 - |l|^2, 0)), f_s = mu + sum_j l_j z_sj + d z_sp, g_s = max_j (mu_P + L_P z_s)_j; its scale is
|mu| + sum_j |l_j z_sj| + |d z_sp| + |t| averaged over s, the yardstick of the 1e-12 bar on the finish kernel.

The end-to-end bar `tol_qei` carries the pieces' bars through: the value is 1-Lipschitz in every f_s and every g_s, so with
E_j = mean_s |z_sj| (0.8 for normal draws; the sample's own here),
    2 tol_mu                            the candidate's mean and the pending points' (f and g each move by at most their own)
    |dl| sum_j E_j                      dl = |L_P^-1| (sqrt(p) tol_c + dL |l|): the forward substitution's reply to an error in c and in L_P,
                                        dL = |L_P| |L_P^-1|^2 p tol_S the first-order reply of a Cholesky factor to an error in S_PP
    dd E_p                              r = s2 - |l|^2 moves by dr = tol_s2 + 2 |l| |dl|, d = sqrt(r) by dr / max(d, sqrt(dr))
    dL sum_i E_i                        g's reply to the error in L_P
    1e-12 scale                         the finish itself
with tol_mu = 1e-6 |mu| + 1e-9, tol_s2 = 1e-6 s2, tol_c and tol_S Sigma's bar 1e-10 (sf2 + noise + |v_a| |v_b|), and the norms taken
from the restatement's own factor of S_PP.  Pending points are chosen apart from each other (`pending_points`) so that |L_P^-1|
stays of order 1 / sqrt(noise) and this remains a usable bar.
"""
import numpy as np

import cov_reference as cr
import kg_reference as kr

CLAMP_PY = 1e-7
XI = .01

# The GPU test's cases: (kind, D, N, p, S, M, prior).  Every kernel kind; D 1 / 3 / 8 / 64; N 1 / 10 / 65 / 1030 (the last crosses the
# 1024-element chunk of the row kernels); p 0 / 1 / 2 / 7 / 15; S 1 / 63 / 64 / 65 / 1000 / 4096 (either side of the wavefront's 64 lanes
# and of the finish's 256-sample stage); M 1 / 255 / 256 / 257 / 1000 (either side of the 16-candidate workgroup, the 64-row tile and
# the 256-candidate arg-max block); two models with a mean prior.  Noise 0.1.
CASES = [
    ("ard", 1, 1, 0, 1, 1, False), ("iso", 3, 10, 1, 63, 255, True), ("m3", 3, 65, 2, 64, 256, False), ("m5", 8, 65, 7, 65, 257, False),
    ("ard", 8, 1030, 15, 1000, 1000, False), ("iso", 64, 65, 7, 4096, 255, False), ("m3", 1, 10, 2, 1000, 1000, False),
    ("m5", 3, 1030, 1, 4096, 257, True), ("svard", 3, 65, 15, 4096, 256, False), ("ard", 64, 10, 0, 65, 1, False),
    ("iso", 8, 1, 1, 1, 256, False), ("m5", 1, 65, 0, 4096, 1000, False),
]


def pending_points(X, p, seed=7):
    """p points of the box chosen apart from each other: farthest-point selection among 256 uniform draws"""
    rs = np.random.RandomState(seed)
    D = X.shape[1]
    pool = rs.rand(256, D) * .9 + .05
    if p == 0:
        return np.empty((0, D))
    pick = [0]
    dist = np.sum((pool - pool[0]) ** 2, axis=1)
    for _ in range(p - 1):
        k = int(np.argmax(dist))
        pick.append(k)
        dist = np.minimum(dist, np.sum((pool - pool[k]) ** 2, axis=1))
    return pool[pick]


def samples(S, q, seed=13):
    return np.random.RandomState(seed).randn(S, q)


def pieces(ref, P, X, clamp_lo=CLAMP_PY, jitter=0.0, sf2k=None):
    """dict(mu_pend (p), S_pend (p, p; jitter on the diagonal), mu (M), s2 (M, clipped), c (M, p), vnP (p), vnX (M): |v| of either set,
    Sigma: the whole joint covariance of (P, X) before jitter and clip)"""
    P = np.asarray(P, dtype=float).reshape(-1, ref.X.shape[1]); X = np.atleast_2d(np.asarray(X, dtype=float))
    p = len(P)
    Sig, vn = cr.cov(ref, np.r_[P, X], True, sf2k)
    s = kr.slopes(ref, X[:1], np.r_[P, X], clamp_lo, sf2k)             # (the means and the clipped variances of all p + M points)
    S_pend = Sig[:p, :p].copy()
    S_pend[np.diag_indices(p)] += jitter
    return dict(mu_pend=s["mu"][:p], S_pend=S_pend, mu=s["mu"][p:], s2=s["s2"][p:], c=Sig[p:, :p].copy(), vnP=vn[:p], vnX=vn[p:], Sigma=Sig)


def qei(ref, P, X, Z, t, clamp_lo=CLAMP_PY, jitter=0.0, sf2k=None):
    """dict: pieces' entries + qei (M), base, L_pend (the factor of S_pend), terms (M, S): every sample's term (for standard errors)"""
    pc = pieces(ref, P, X, clamp_lo, jitter, sf2k)
    p, M = len(pc["mu_pend"]), len(pc["mu"])
    Z = np.asarray(Z, dtype=float)
    assert Z.shape[1] == p + 1
    val = np.empty(M); terms = np.empty((M, len(Z)))
    for x in range(M):
        J = np.empty((p + 1, p + 1))
        J[:p, :p] = pc["S_pend"]
        J[p, :p] = J[:p, p] = pc["c"][x]
        J[p, p] = pc["s2"][x]
        L = np.linalg.cholesky(J)
        Y = np.r_[pc["mu_pend"], pc["mu"][x]] + Z @ L.T
        terms[x] = np.maximum(np.max(Y, axis=1) - t, 0.0)
        val[x] = np.mean(terms[x])
    pc["qei"] = val; pc["terms"] = terms
    if p:
        pc["L_pend"] = np.linalg.cholesky(pc["S_pend"])
        G = pc["mu_pend"] + Z[:, :p] @ pc["L_pend"].T
        pc["base"] = float(np.mean(np.maximum(np.max(G, axis=1) - t, 0.0)))
    else:
        pc["L_pend"] = np.empty((0, 0)); pc["base"] = 0.0
    return pc


def _chol(S, dtype):
    """the lower Cholesky factor by rows, in `dtype`"""
    p = len(S)
    L = np.zeros((p, p), dtype=dtype)
    for j in range(p):
        for i in range(j):
            L[j, i] = (S[j, i] - np.sum(L[j, :i] * L[i, :i])) / L[i, i]
        L[j, j] = np.sqrt(S[j, j] - np.sum(L[j, :j] * L[j, :j]))
    return L


def compose(mu_pend, S_pend, mu, s2, c, Z, t, jitter=0.0, dtype=np.float64):
    """(qEI (M), scale (M)) by the ABI's definition from given pieces.  jitter is added to S_pend's diagonal: 0 for pieces that carry it
    already (ibo_qei_batch's S_pend_host, pieces())."""
    mu_pend = np.asarray(mu_pend, dtype=dtype); mu = np.asarray(mu, dtype=dtype); s2 = np.asarray(s2, dtype=dtype)
    Z = np.asarray(Z, dtype=dtype); t = dtype(t)
    p, M, S = len(mu_pend), len(mu), len(Z)
    c = np.asarray(c, dtype=dtype).reshape(M, p)
    Sp = np.array(S_pend, dtype=dtype).reshape(p, p)
    Sp[np.diag_indices(p)] += dtype(jitter)
    L = _chol(Sp, dtype)
    if p:
        g = np.max(mu_pend + Z[:, :p] @ L.T, axis=1)
    else:
        g = np.full(S, -np.inf, dtype=dtype)
    val = np.empty(M, dtype=dtype); scale = np.empty(M, dtype=dtype)
    for x in range(M):
        l = np.zeros(p, dtype=dtype)
        for j in range(p):
            l[j] = (c[x, j] - np.sum(L[j, :j] * l[:j])) / L[j, j]
        r = s2[x] - np.sum(l * l)
        d = np.sqrt(r) if r > 0 else dtype(0)
        f = mu[x] + Z[:, :p] @ l + d * Z[:, p]
        val[x] = np.mean(np.maximum(np.maximum(f, g) - t, dtype(0)))
        scale[x] = np.mean(np.abs(mu[x]) + np.abs(Z[:, :p]) @ np.abs(l) + np.abs(d * Z[:, p]) + np.abs(t))
    return val, scale


# ---- the GPU test's bars, from the restatement's own quantities
def tol_mu(mu):
    return 1e-6 * np.abs(mu) + 1e-9


def tol_c(w, sf2, noise):
    """(M, p): Sigma's bar for the candidates' covariances with the pending points"""
    return 1e-10 * (sf2 + noise + np.outer(w["vnX"], w["vnP"]))


def tol_S(w, sf2, noise):
    """(p, p): Sigma's bar for S_pend"""
    return 1e-10 * (sf2 + noise + np.outer(w["vnP"], w["vnP"]))


def tol_qei(w, Z, t, sf2, noise):
    """(M,): the pieces' bars carried through to the value -- the module docstring's derivation"""
    p, M = len(w["mu_pend"]), len(w["mu"])
    E = np.mean(np.abs(np.asarray(Z, dtype=float)), axis=0)
    _, scale = compose(w["mu_pend"], w["S_pend"], w["mu"], w["s2"], w["c"], Z, t)
    tm = tol_mu(w["mu"]) + (np.max(tol_mu(w["mu_pend"])) if p else 0.0)
    out = tm + 1e-12 * scale
    if p:
        L = w["L_pend"]
        nL = np.linalg.norm(L, 2); nLi = np.linalg.norm(np.linalg.inv(L), 2)
        dL = nL * nLi ** 2 * p * np.max(tol_S(w, sf2, noise))
        l = np.linalg.solve(L, w["c"].T).T                                       # (M, p)
        nl = np.linalg.norm(l, axis=1)
        dl = nLi * (np.sqrt(p) * np.max(tol_c(w, sf2, noise), axis=1) + dL * nl)
        d = np.sqrt(np.maximum(w["s2"] - nl ** 2, 0.0))
        dr = 1e-6 * w["s2"] + 2 * nl * dl
        out = out + dl * np.sum(E[:p]) + dL * np.sum(E[:p])
    else:
        d = np.sqrt(w["s2"]); dr = 1e-6 * w["s2"]
    return out + dr / np.maximum(d, np.sqrt(dr)) * E[p]


def case_inputs(case):
    """(X, Y, hyper, prior object, RefGP, P, Q, Z, t) of one of CASES"""
    import test_gpu_posterior_cov as pc
    kind, D, N, p, S, M, prior = case
    X, Y, hyper, pr, ref = kr.case_ref(kind, D, N, prior)
    return X, Y, hyper, pr, ref, pending_points(X, p), pc.queries(X, M), samples(S, p + 1), float(np.max(Y)) + XI


def ei_candidates(X, Y, n=8, seed=9):
    """points near the n best observations: EI is not negligible there, so every sampling error below is a positive number"""
    rs = np.random.RandomState(seed)
    return X[np.argsort(Y)[-n:]] + .08 * rs.randn(n, X.shape[1])


def antithetic_ratio(mu, s2, Z, t, values, ei):
    """|values - ei| over the standard error of an antithetic single-point estimate: the terms max(mu + sigma z - t, 0) of the draws z and
    -z (rows s and s + S / 2 of Z) are averaged in pairs, the pairs are the independent units"""
    half = len(Z) // 2
    terms = np.maximum(mu[:, None] + np.sqrt(s2)[:, None] * Z[:, 0] - t, 0.0)
    pair = .5 * (terms[:, :half] + terms[:, half:])
    se = np.std(pair, axis=1, ddof=1) / np.sqrt(half)
    assert np.all(se > 0)
    return np.abs(np.asarray(values) - ei) / se

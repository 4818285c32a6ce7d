"""
Where conditioning is worst: the truth for tests/test_gpu_conditioning.py, pinned on the CPU by tests/test_conditioning_reference.py.

Models.  The construction of test_gpu_parity.py::test_tolerance_where_conditioning_is_worst at seed 0 -- three clusters of N // 4 points
at c_i + 0.02 randn, the rest uniform, clipped to the cube, Y = sin(3 sum X) + .01 randn -- with X rounded to the 2^-12 grid, so that a
kernel matrix formed from differences is exact in its inputs.  Noise 1e-6 .. 1e-4: cond_2(R) lies in [1e6, 1e9] for every case of CASES
(asserted).  The 24 queries (on the 2^-16 grid): half uniform, half within 1e-3 of an observation, where sigma^2 ~ noise and the
cancellation in 1 + noise - |v|^2 is complete; the first two of that half sit beside the first and the last observation.

TrueGP.  In np.longdouble by hand, as nlml_reference.py, loo_reference.py and test_gpu_parity._longdouble_posterior do it: L column by
column, W = L^-1 row by row, alpha_Y = W^T W Y, alpha_1 = W^T W 1; from them mu and the raw sigma^2 (with the mean prior's path), the
gradients with grad_reference.RefGP.grad's scales smu and ss2, the joint covariance by cov_reference's definition, the slope rows of
kg_reference.slopes, q-EI's pieces (qei_reference.pieces) and the paths' coefficients (paths_reference.coef).  `extended` borders the
factor by one observation in O(N^2).

ref_error(case, what).  The reference's OWN float64 error: the same quantity in float64 (a) by cho_solve, as the existing restatements
do, and (b) in the device's formulation -- the explicit W, v = W k*, q = |v|^2, k* in the dot form a_k + b_c + x~.c~ of
shift_reference.exponent_dot -- each compared with TrueGP and normalised by the quantity's terms' magnitude, the worst over the entries,
over (a) and (b) and over N_PERM seeded permutations of the observation order.  One number per case and quantity, no device involved.
The case with its near-duplicate row appended (the kept-state test's addData) is restated a third way too, (c): as (b), with W's last row
by the in-place extension's own order -- z = W r, u = W^T z, d = sqrt(1 + noise - z.z), [-u, 1] / d -- which is how the device reaches
that model (ibo_gp_extend) and, at 1.2e-12 against 4e-13 on se65's sigma^2, the least accurate of the three.
The GPU file's two bars are  err <= RULE(cond) = 1e-15 max(cond_2, 1e6)  (the project's rule) and  err <= 8 ref_error  (the reference's
reach; the 8 of shift_reference.measured_bar).

Terms' magnitudes (`scales` of a truth dict):
    mu          |m| + sum_i |k*_i (aY_i - m a1_i)|                    s2      1 + noise + q
    dmu, ds2    grad_reference's smu, ss2                             Sigma   sf2 + noise + |v_a| |v_b|
    KG's b      (sf2 + noise + |v_x| |v_a|) / sigma_x + |b| (1 + noise + q) / (2 s2)     (kg_reference.tol_b: Sigma's scale through the
                division, and the variance's own bar through 1 / sigma)
    q-EI's c, S_pend: Sigma's; mu_ref, mu_pend: mu's
    paths       the coefficients are judged by the path values they give at the queries, k*(q).c_s, over paths_reference.terms_scale
                T = |m| + sum_j |phi_j w_j| + sum_i |k*_i c_i| ("coef"), and entry by entry ("coef_entry"), c_si = aY_i - (R^-1 u_s)_i
                over |aY_i| + sum_j |(R^-1)_ij| |u_sj|: an error no query's k* sees is seen there
"""
import functools

import numpy as np
from scipy.linalg import cho_factor, cho_solve, solve_triangular

import cov_reference as cr
import grad_reference as gr
import kg_reference as kr
import paths_reference as pr
import qei_reference as qr
import shift_reference as sr

LD = np.longdouble
GRID_X = 4096.0                      # observations: multiples of 2^-12
GRID_Q = 65536.0                     # queries: multiples of 2^-16 (a query 1e-3 from an observation stays beside it)
CLAMP_NATIVE, CLAMP_PY = 1e-8, 1e-7
M_TRUTH = 24
N_PERM = 5
N_REF = 5                            # reference points of KG, pending points of q-EI
PATHS_F, PATHS_S = 64, 3
COND_RANGE = (1e6, 1e9)

# name: (kind, hyper, N, D, noise, mean prior)
CASES = {
    "se65": ("ard", [.3, .3], 65, 2, 1e-6, False),
    "m5_65": ("m5", [.5, 1.0], 65, 3, 1e-6, False),
    "se300": ("ard", [.3, .3], 300, 2, 1e-5, False),
    "m5_300": ("m5", [.5, 1.0], 300, 4, 1e-4, False),
    "se1030": ("ard", [.3, .3], 1030, 2, 1e-4, False),
    "m3_64": ("m3", [.5, 1.0], 64, 3, 1e-6, False),
    "iso300_prior": ("iso", [.3], 300, 2, 1e-5, True),
    "sviso65": ("sviso", [.3, .999995], 65, 2, 1e-6, False),
}
WHATS = ("mu", "s2", "dmu", "ds2", "cov_noise", "cov_latent", "kg_mu_ref", "kg_b", "qei_mu_pend", "qei_S", "qei_c", "coef", "coef_entry")


def rule(cond):
    """the project's rule: the relative error a quantity may carry, in units of its terms' magnitude"""
    return 1e-15 * max(cond, 1e6)


def prior_tuple(D, seed=11):
    """(means, beta, theta, lowerb, width): the numbers of test_gpu_gradients.make_prior(D)"""
    rs = np.random.RandomState(seed)
    means = rs.rand(5, D); beta = rs.randn(5)
    return means, beta, 1.5, np.zeros(D) - .1, np.full(D, 1.2)


def near_duplicate(X, j=7):
    """a new observation one grid step (2^-12) from row j, inside the cube"""
    x = X[j].copy()
    x[0] += (1.0 if x[0] < .5 else -1.0) / GRID_X
    return x


@functools.lru_cache(maxsize=None)
def case_data(name, seed=0):
    """dict of one case: X, Y, Q (the 24 truth queries), A (KG's reference points), P (q-EI's pending points), the paths' draws,
    the kernel as (fam, w, sf2), sw, the prior tuple, cond (cond_2 of the float64 R), and the extension (x_new, y_new)"""
    kind, hyper, N, D, noise, with_prior = CASES[name]
    rs = np.random.RandomState(seed)
    c = rs.rand(3, D)
    X = np.clip(np.vstack([c[i] + 0.02 * rs.randn(N // 4, D) for i in range(3)] + [rs.rand(N - 3 * (N // 4), D)]), 0, 1)
    X = np.rint(X * GRID_X) / GRID_X
    Y = np.sin(3 * X.sum(1)) + .01 * rs.randn(N)
    h = M_TRUTH // 2
    rows = np.r_[0, N - 1, rs.randint(0, N, h - 2)]
    Q = np.vstack([rs.rand(h, D), np.clip(X[rows] + 1e-3 * rs.randn(h, D), 0, 1)])
    Q = np.rint(Q * GRID_Q) / GRID_Q
    fam, w, sf2 = gr.kernel_spec(kind, hyper, D)
    d = dict(name=name, kind=kind, hyper=hyper, N=N, D=D, noise=noise, X=X, Y=Y, Q=Q, fam=fam, w=w, sf2=sf2, sw=np.sqrt(w),
             prior=prior_tuple(D) if with_prior else None)
    d["A"] = kr.ref_points(X, N_REF); d["P"] = qr.pending_points(X, N_REF)
    F, S = PATHS_F, PATHS_S
    d["omega"] = rs.randn(F, D) * d["sw"]; d["phase"] = rs.rand(F) * 2 * np.pi
    d["pw"] = rs.randn(S, F); d["eps"] = np.sqrt(max(1.0 + noise - sf2, 0.0)) * rs.randn(S, N + 1)      # (one more column: the extension)
    d["x_new"] = near_duplicate(X); d["y_new"] = float(np.sin(3 * d["x_new"].sum()) + .01 * rs.randn())
    R = cr.kmat(fam, w, sf2, X, X); np.fill_diagonal(R, 1.0 + noise)
    d["cond"] = float(np.linalg.cond(R, 2))
    return d


@functools.lru_cache(maxsize=None)
def extended_data(name):
    """the case with the near-duplicate observation appended (what the kept-state test's addData leaves)"""
    d = dict(case_data(name))
    d["X"] = np.vstack([d["X"], d["x_new"]]); d["Y"] = np.r_[d["Y"], d["y_new"]]; d["N"] += 1
    R = cr.kmat(d["fam"], d["w"], d["sf2"], d["X"], d["X"]); np.fill_diagonal(R, 1.0 + d["noise"])
    d["cond"] = float(np.linalg.cond(R, 2))
    return d


# ------------------------------------------------------------------------------------------------------------ long double by hand
def kstar_ld(fam, w, sf2, X, Q):
    """(k (N, M), h (N, M), diff (N, M, D)) in long double: k*(q_j, X_i) and dk*/dq = h w (q - X_i)"""
    diff = np.asarray(Q, dtype=LD)[None, :, :] - np.asarray(X, dtype=LD)[:, None, :]
    z = np.sum(np.asarray(w, dtype=LD) * diff * diff, axis=2)
    s = LD(sf2)
    if fam == gr.FAM_SE:
        k = s * np.exp(-z / 2)
        return k, -k, diff
    if fam == gr.FAM_M3:
        r = np.sqrt(3 * z); e = np.exp(-r)
        return s * (1 + r) * e, -3 * s * e, diff
    r = np.sqrt(5 * z); e = np.exp(-r)
    return s * (1 + r + r * r / 3) * e, -(LD(5) / 3) * s * (1 + r) * e, diff


def prior_ld(prior, Q):
    """(m (M,), dm (M, D)) of the RBF-network prior in long double; zeros without one"""
    Q = np.asarray(Q, dtype=LD)
    if prior is None:
        return np.zeros(len(Q), dtype=LD), np.zeros(Q.shape, dtype=LD)
    means, beta, theta, lo, wd = prior
    diff = ((Q - np.asarray(lo, dtype=LD)) / np.asarray(wd, dtype=LD))[:, None, :] - np.asarray(means, dtype=LD)[None, :, :]
    be = np.asarray(beta, dtype=LD)[None, :] * np.exp(-LD(theta) * np.sum(diff * diff, axis=2))
    return be.sum(axis=1), np.einsum('mk,mkd->md', be, diff) * (-2 * LD(theta)) / np.asarray(wd, dtype=LD)


def chol_ld(A):
    N = len(A)
    L = np.zeros((N, N), dtype=LD)
    for j in range(N):
        L[j, j] = np.sqrt(A[j, j] - np.dot(L[j, :j], L[j, :j]))
        if j + 1 < N:
            L[j + 1:, j] = (A[j + 1:, j] - L[j + 1:, :j].dot(L[j, :j])) / L[j, j]
    return L


def inv_lower_ld(L):
    N = len(L)
    W = np.zeros((N, N), dtype=LD)
    for i in range(N):
        W[i, :i] = -np.dot(L[i, :i], W[:i, :i]) / L[i, i]
        W[i, i] = 1 / L[i, i]
    return W


class TrueGP(object):
    """the model in long double: L, W = L^-1, aY, a1 and everything the evaluation entries derive from them"""

    def __init__(self, X, Y, noise, fam, w, sf2, prior=None):
        self.X = np.atleast_2d(np.asarray(X, dtype=float)); self.Y = np.asarray(Y, dtype=float).reshape(-1)
        self.noise, self.fam, self.w, self.sf2, self.prior = float(noise), fam, np.asarray(w, dtype=float), float(sf2), prior
        R = kr._kmat(fam, self.w, self.sf2, self.X, self.X, LD)
        R[np.diag_indices_from(R)] = LD(1) + LD(self.noise)
        self.L = chol_ld(R)
        self.W = inv_lower_ld(self.L)
        self._alphas()

    def _alphas(self):
        self.aY = self.W.T.dot(self.W.dot(self.Y.astype(LD)))
        self.a1 = self.W.T.dot(self.W.dot(np.ones(len(self.Y), dtype=LD)))

    def extended(self, x, y):
        """the model with one more observation: the factor bordered, z = W r, d = sqrt(1 + noise - z.z), the new row of W = [-z^T W, 1] / d"""
        g = TrueGP.__new__(TrueGP)
        g.noise, g.fam, g.w, g.sf2, g.prior = self.noise, self.fam, self.w, self.sf2, self.prior
        N = len(self.Y)
        r = kstar_ld(self.fam, self.w, self.sf2, self.X, np.atleast_2d(x))[0][:, 0]
        z = self.W.dot(r)
        d = np.sqrt(LD(1) + LD(self.noise) - z.dot(z))
        g.X = np.vstack([self.X, x]); g.Y = np.r_[self.Y, y]
        g.L = np.zeros((N + 1, N + 1), dtype=LD); g.L[:N, :N] = self.L; g.L[N, :N] = z; g.L[N, N] = d
        g.W = np.zeros((N + 1, N + 1), dtype=LD); g.W[:N, :N] = self.W; g.W[N, :N] = -z.dot(self.W) / d; g.W[N, N] = 1 / d
        g._alphas()
        return g

    # ---- posterior
    def at(self, Q, sf2k=None, grad=False):
        """long-double dict at the rows of Q: Ks (N, M), V = W Ks, q, mu, s2 (raw), m, mu_scale, s2_scale; with grad dmu, ds2, smu, ss2"""
        Q = np.atleast_2d(np.asarray(Q, dtype=float))
        k, h, diff = kstar_ld(self.fam, self.w, self.sf2 if sf2k is None else sf2k, self.X, Q)
        V = self.W.dot(k)
        q = np.sum(V * V, axis=0)
        m, dm = prior_ld(self.prior, Q)
        eff = self.aY[:, None] - self.a1[:, None] * m[None, :]                       # aY - m a1, a column per query
        ka1 = k.T.dot(self.a1)
        out = dict(Ks=k, V=V, q=q, m=m, mu=m + k.T.dot(self.aY) - m * ka1, s2=LD(1) + LD(self.noise) - q,
                   mu_scale=np.abs(m) + np.sum(np.abs(k * eff), axis=0), s2_scale=LD(1) + LD(self.noise) + q)
        if grad:
            U = self.W.T.dot(V)
            wd = np.asarray(self.w, dtype=LD) * diff                                 # (N, M, D)
            tm = (h * eff)[:, :, None] * wd
            ts = -2 * (h * U)[:, :, None] * wd
            lead = dm * (1 - ka1)[:, None]
            out.update(dmu=lead + tm.sum(axis=0), smu=np.abs(lead) + np.abs(tm).sum(axis=0), ds2=ts.sum(axis=0), ss2=np.abs(ts).sum(axis=0))
        return out

    def cov(self, Q, with_noise=True, sf2k=None):
        """(Sigma (M, M), |v| (M,)) by cov_reference's definition"""
        Q = np.atleast_2d(np.asarray(Q, dtype=float))
        sf2k = self.sf2 if sf2k is None else sf2k
        p = self.at(Q, sf2k)
        S = kr._kmat(self.fam, self.w, sf2k, Q, Q, LD) - p["V"].T.dot(p["V"])
        S[np.diag_indices_from(S)] = (LD(1) + LD(self.noise) if with_noise else LD(1)) - p["q"]
        return S, np.sqrt(p["q"])

    def slopes(self, A, Xq, clamp_lo=CLAMP_PY):
        """kg_reference.slopes' dict in long double, with b's scale"""
        A = np.atleast_2d(np.asarray(A, dtype=float)); Xq = np.atleast_2d(np.asarray(Xq, dtype=float))
        a, x = self.at(A), self.at(Xq)
        s2 = np.minimum(np.maximum(x["s2"], LD(clamp_lo)), LD(10))
        sig = np.sqrt(s2)
        C = kr._kmat(self.fam, self.w, self.sf2, Xq, A, LD) - x["V"].T.dot(a["V"])
        b = C / sig[:, None]
        vnA, vnX = np.sqrt(a["q"]), np.sqrt(x["q"])
        b_scale = (LD(self.sf2) + LD(self.noise) + np.outer(vnX, vnA)) / sig[:, None] + np.abs(b) * (x["s2_scale"] / (2 * s2))[:, None]
        return dict(mu_ref=a["mu"], mu_ref_scale=a["mu_scale"], mu=x["mu"], s2=s2, q=x["q"], b=b, b_scale=b_scale, vnA=vnA, vnX=vnX)

    def pieces(self, P, Xq):
        """q-EI's pieces: mu_pend, S_pend (no jitter), c (M, p), and Sigma's scales for S_pend and c"""
        P = np.atleast_2d(np.asarray(P, dtype=float)); Xq = np.atleast_2d(np.asarray(Xq, dtype=float))
        p = len(P)
        S, vn = self.cov(np.r_[P, Xq], True)
        sc = LD(self.sf2) + LD(self.noise) + np.outer(vn, vn)
        pp = self.at(P)
        return dict(mu_pend=pp["mu"], mu_pend_scale=pp["mu_scale"], S_pend=S[:p, :p], S_scale=sc[:p, :p], c=S[p:, :p], c_scale=sc[p:, :p])

    def features(self, omega, phase, Xq):
        Xq = np.atleast_2d(np.asarray(Xq, dtype=float)).astype(LD); omega = np.atleast_2d(omega).astype(LD)
        t = Xq.dot(omega.T) + np.asarray(phase, dtype=LD)[None, :]
        t -= pr.TWO_PI_LD * np.rint(t / pr.TWO_PI_LD)
        return np.sqrt(2 * LD(self.sf2) / len(omega)) * np.cos(t)

    def coef(self, omega, phase, w, eps):
        """(S, F + N): paths_reference.coef in long double"""
        w = np.atleast_2d(w).astype(LD); eps = np.atleast_2d(eps).astype(LD)
        u = self.features(omega, phase, self.X).dot(w.T) + eps.T
        c = self.aY[:, None] - self.W.T.dot(self.W.dot(u))
        return np.c_[w, c.T]

    def coef_entry_scale(self, omega, phase, w, eps):
        """(S, N): the terms' magnitudes of every c_si = aY_i - sum_j (R^-1)_ij u_sj: |aY_i| + sum_j |(R^-1)_ij| |u_sj|"""
        w = np.atleast_2d(w).astype(LD); eps = np.atleast_2d(eps).astype(LD)
        u = self.features(omega, phase, self.X).dot(w.T) + eps.T
        return (np.abs(self.aY)[:, None] + np.abs(self.W.T.dot(self.W)).dot(np.abs(u))).T

    def path_scale(self, omega, phase, coefs, Xq):
        """(S, M): paths_reference.terms_scale in long double, and the k* (N, M) it was formed with"""
        F = len(np.atleast_2d(omega))
        p = self.at(Xq)
        T = np.abs(p["m"])[None, :] + np.abs(coefs[:, :F]).dot(np.abs(self.features(omega, phase, Xq)).T) + np.abs(coefs[:, F:]).dot(np.abs(p["Ks"]))
        return T, p["Ks"]


def f64(a):
    return np.asarray(a, dtype=np.float64)


def truth_of_data(d, gp=None):
    """(dict of float64 arrays: every quantity of WHATS at the case's queries with its scale under '<what>_scale', TrueGP)"""
    gp = TrueGP(d["X"], d["Y"], d["noise"], d["fam"], d["w"], d["sf2"], d["prior"]) if gp is None else gp
    N = len(gp.Y)
    p = gp.at(d["Q"], grad=True)
    t = dict(mu=p["mu"], mu_scale=p["mu_scale"], s2=p["s2"], s2_scale=p["s2_scale"], dmu=p["dmu"], dmu_scale=p["smu"], ds2=p["ds2"],
             ds2_scale=p["ss2"], q=p["q"])
    for key, wn in (("cov_noise", True), ("cov_latent", False)):
        S, vn = gp.cov(d["Q"], wn)
        t[key] = S; t[key + "_scale"] = LD(gp.sf2) + LD(gp.noise) + np.outer(vn, vn)
    s = gp.slopes(d["A"], d["Q"])
    t.update(kg_mu_ref=s["mu_ref"], kg_mu_ref_scale=s["mu_ref_scale"], kg_b=s["b"], kg_b_scale=s["b_scale"])
    pc = gp.pieces(d["P"], d["Q"])
    t.update(qei_mu_pend=pc["mu_pend"], qei_mu_pend_scale=pc["mu_pend_scale"], qei_S=pc["S_pend"], qei_S_scale=pc["S_scale"],
             qei_c=pc["c"], qei_c_scale=pc["c_scale"])
    co = gp.coef(d["omega"], d["phase"], d["pw"], d["eps"][:, :N])
    T, Ks = gp.path_scale(d["omega"], d["phase"], co, d["Q"])
    out = {k: f64(v) for k, v in t.items()}
    out["coef"] = co; out["coef_scale"] = T; out["coef_Ks"] = Ks              # (kept in long double: `shares` contracts in it)
    out["coef_entry"] = co[:, -N:]; out["coef_entry_scale"] = gp.coef_entry_scale(d["omega"], d["phase"], d["pw"], d["eps"][:, :N])
    return out, gp


@functools.lru_cache(maxsize=None)
def truth_of(name, extended=False):
    """the truth of a case (or of the case with its near-duplicate observation appended, bordered from the case's own factor)"""
    if not extended:
        return truth_of_data(case_data(name))
    d = case_data(name)
    return truth_of_data(extended_data(name), truth_of(name)[1].extended(d["x_new"], d["y_new"]))


def shares(truth, got, whats=None):
    """{what: worst |got - truth| / scale} over the quantities present in got"""
    out = {}
    for k in (WHATS if whats is None else whats):
        if k == "coef_entry" and "coef" in got:
            N = truth[k].shape[1]
            out[k] = float(np.max(np.abs(np.asarray(got["coef"], dtype=LD)[:, -N:] - truth[k]) / truth[k + "_scale"]))
            continue
        if k not in got:
            continue
        if k == "coef":
            N = truth["coef_Ks"].shape[0]
            dc = np.asarray(got[k], dtype=LD)[:, -N:] - truth[k][:, -N:]
            out[k] = float(np.max(np.abs(dc.dot(truth["coef_Ks"])) / truth["coef_scale"]))
            continue
        sc = truth[k + "_scale"]
        err = np.abs(np.asarray(got[k]) - truth[k])
        live = sc > 0
        assert np.all(err[~live] == 0), "%s: an entry without terms is not zero" % k
        out[k] = float(np.max(err[live] / sc[live])) if np.any(live) else 0.0
    return out


# ------------------------------------------------------------------------------------------------------------ float64, two ways
def _k_and_h(fam, sf2, y):
    """k and h (dk/dq = h w (q - x)) from the exponent y = -z / 2"""
    if fam == gr.FAM_SE:
        k = sf2 * np.exp(y)
        return k, -k
    z = np.maximum(-2.0 * y, 0.0)
    if fam == gr.FAM_M3:
        r = np.sqrt(3.0 * z); e = np.exp(-r)
        return sf2 * (1.0 + r) * e, -3.0 * sf2 * e
    r = np.sqrt(5.0 * z); e = np.exp(-r)
    return sf2 * (1.0 + r + r * r / 3.0) * e, -(5.0 / 3.0) * sf2 * (1.0 + r) * e


def _prior64(prior, Q):
    if prior is None:
        return np.zeros(len(Q)), np.zeros(Q.shape)
    md = [gr.prior_grad(prior, x) for x in Q]
    return np.array([a for a, _ in md]), np.array([b for _, b in md])


MUTANTS = ("W32", "droprow", "stale", "exponent", "q32", "noise")


def restate(d, form, perm=None, mutant=None, whats=WHATS):
    """the quantities of `whats` in float64 at the case's queries.  form 'a': cho_solve, k* by differences (the existing restatements);
    form 'b': explicit W, v = W k*, q = |v|^2, k* in the dot form; form 'c': as 'b' with W's last row by the in-place extension.  perm: the order the observations are factored in (results are
    returned in the case's own order).  mutant (form 'b' only): one of MUTANTS, what a subtly wrong kernel would do."""
    assert form in ("a", "b", "c") and (mutant is None or form == "b")
    N = d["N"]
    perm = np.arange(N) if perm is None else np.asarray(perm)
    X, Y = d["X"][perm], d["Y"][perm]
    fam, w, sf2, sw, noise, prior = d["fam"], d["w"], d["sf2"], d["sw"], d["noise"], d["prior"]
    R = cr.kmat(fam, w, sf2, X, X); np.fill_diagonal(R, 1.0 + noise)
    one = np.ones(N)
    pts = dict(Q=d["Q"])
    if "kg_b" in whats or "kg_mu_ref" in whats: pts["A"] = d["A"]
    if any(k.startswith("qei") for k in whats): pts["P"] = d["P"]
    if form == "a":
        cf = cho_factor(R, lower=True)
        aY, a1 = cho_solve(cf, Y), cho_solve(cf, one)
        solve = lambda B: cho_solve(cf, B)
    else:
        if form == "b":
            W = solve_triangular(np.linalg.cholesky(R), np.eye(N), lower=True)
        else:
            # the in-place extension (ibo_gp_extend) by the last observation: W of the first N - 1 rows as in (b), then z = W r,
            # u = W^T z, d = sqrt(1 + noise - z.z) and the new row of W = [-u, 1] / d; the alpha vectors again from the whole W
            n = N - 1
            W = np.zeros((N, N))
            W[:n, :n] = solve_triangular(np.linalg.cholesky(R[:n, :n]), np.eye(n), lower=True)
            z = W[:n, :n].dot(R[:n, n])
            dd = np.sqrt((1.0 + noise) - z.dot(z))
            W[n, :n] = -W[:n, :n].T.dot(z) / dd; W[n, n] = 1.0 / dd
        aY, a1 = W.T.dot(W.dot(Y)), W.T.dot(W.dot(one))
        solve = lambda B: W.T.dot(W.dot(B))
        if mutant == "noise":
            Rm = R.copy(); np.fill_diagonal(Rm, 1.0 + noise * (1.0 + 1e-6))
            Wm = solve_triangular(np.linalg.cholesky(Rm), np.eye(N), lower=True)
            aY = Wm.T.dot(Wm.dot(Y))
        elif mutant == "W32":
            W = W.astype(np.float32).astype(np.float64)
        elif mutant == "stale":
            # the rows of W's last 64-row block from the model WITHOUT its first observation (columns 1 .. N - 1; column 0 empty)
            Ws = solve_triangular(np.linalg.cholesky(R[1:, 1:]), np.eye(N - 1), lower=True)
            lo = max(N - 64, 1)
            W = W.copy(); W[lo:, 0] = 0.0; W[lo:, 1:] = Ws[lo - 1:, :]
    ev = {}
    for key, Pts in pts.items():
        if form == "a":
            k, h = _k_and_h(fam, sf2, -0.5 * _z_diff(w, X, Pts))
            U = solve(k); V = None
            q = np.sum(k * U, axis=0)
        else:
            y = sr.exponent_dot(X, Pts, sw)
            if mutant == "exponent":
                y = y * (1.0 + 1e-11)
            k, h = _k_and_h(fam, sf2, y)
            V = W.dot(k)
            if mutant == "droprow":
                V[-1] = 0.0
            q = np.sum((V * V).astype(np.float32), axis=0, dtype=np.float32).astype(np.float64) if mutant == "q32" else np.sum(V * V, axis=0)
            U = W.T.dot(V)
        m, dm = _prior64(prior, Pts)
        ka1 = k.T.dot(a1)
        mu = (m + k.T.dot(aY) - m * ka1) if prior is not None else k.T.dot(aY)
        ev[key] = dict(k=k, h=h, U=U, V=V, q=q, m=m, dm=dm, ka1=ka1, mu=mu)
    e = ev["Q"]
    Q = d["Q"]
    out = dict(mu=e["mu"], s2=1.0 + noise - e["q"])
    if "dmu" in whats or "ds2" in whats:
        diff = Q[None, :, :] - X[:, None, :]
        eff = aY[:, None] - a1[:, None] * e["m"][None, :]
        out["dmu"] = e["dm"] * (1.0 - e["ka1"])[:, None] + np.sum((e["h"] * eff)[:, :, None] * w * diff, axis=0)
        out["ds2"] = np.sum(-2.0 * (e["h"] * e["U"])[:, :, None] * w * diff, axis=0)

    def cross(a, b):                                          # k*_a^T R^-1 k*_b
        return a["k"].T.dot(b["U"]) if form == "a" else a["V"].T.dot(b["V"])
    if "cov_noise" in whats or "cov_latent" in whats:
        quad = cross(e, e)
        quad = 0.5 * (quad + quad.T)
        KQQ = cr.kmat(fam, w, sf2, Q, Q)
        out["cov_noise"], _ = cr._finish(KQQ.copy(), quad, noise, True)
        out["cov_latent"], _ = cr._finish(KQQ.copy(), quad, noise, False)
    if "A" in ev:
        a = ev["A"]
        s2 = np.clip(out["s2"], CLAMP_PY, 10.0)
        out["kg_mu_ref"] = a["mu"]
        out["kg_b"] = (cr.kmat(fam, w, sf2, Q, d["A"]) - cross(e, a)) / np.sqrt(s2)[:, None]
    if "P" in ev:
        p = ev["P"]
        out["qei_mu_pend"] = p["mu"]
        S = cr.kmat(fam, w, sf2, d["P"], d["P"]) - 0.5 * (cross(p, p) + cross(p, p).T)
        np.fill_diagonal(S, 1.0 + noise - p["q"])
        out["qei_S"] = S
        out["qei_c"] = cr.kmat(fam, w, sf2, Q, d["P"]) - cross(e, p)
    if "coef" in whats or "coef_entry" in whats:
        u = pr.features(d["omega"], d["phase"], sf2, X).dot(d["pw"].T) + d["eps"][:, :N][:, perm].T
        c = aY[:, None] - solve(u)
        inv = np.argsort(perm)
        out["coef"] = np.c_[d["pw"], c.T[:, inv]]
    return {k: v for k, v in out.items() if k in whats or (k == "coef" and "coef_entry" in whats)}


def _z_diff(w, X, Pts):
    z = np.zeros((len(X), len(Pts)))
    for dd in range(X.shape[1]):
        z += w[dd] * (X[:, dd, None] - Pts[None, :, dd]) ** 2
    return z


def permutations(N):
    """the identity and N_PERM - 1 seeded shuffles of the observation order"""
    return [np.arange(N)] + [np.random.RandomState(100 + s).permutation(N) for s in range(1, N_PERM)]


@functools.lru_cache(maxsize=None)
def ref_errors(name, extended=False):
    """{what: the reference's own float64 error} of a case: the worst share over forms (a), (b) and the permutations; the case with its
    near-duplicate row appended is also restated as the device reaches it, (c): by the in-place extension, the new row last"""
    d = extended_data(name) if extended else case_data(name)
    truth = truth_of(name, extended)[0]
    worst = {k: 0.0 for k in WHATS}
    perms = [np.r_[p, d["N"] - 1] for p in permutations(d["N"] - 1)] if extended else permutations(d["N"])
    for perm in perms:
        for form in (("a", "b", "c") if extended else ("a", "b")):
            for k, v in shares(truth, restate(d, form, perm)).items():
                worst[k] = max(worst[k], v)
    return worst


def ref_error(name, what, extended=False):
    return ref_errors(name, extended)[what]


def bars(name, what, extended=False):
    """(the project's rule, 8 x the reference's reach) for a quantity of a case"""
    d = extended_data(name) if extended else case_data(name)
    return rule(d["cond"]), 8.0 * ref_error(name, what, extended)

"""
The two-objective expected hypervolume improvement of ibo_ehvi_* restated in NumPy (float64) -- canonical front, value, the
gradient's partial sums, the gradient, both erf flavours -- on the posteriors of tests/cacq_reference.py and the pieces of
tests/grad_reference.py; pinned by tests/test_ehvi_reference.py, the yardstick of tests/test_gpu_ehvi.py.

    psi_k(t) = sigma_k phi(u) + (mu_k - t) Phi(u),  u = (mu_k - t) / sigma_k           psi_1(+inf) = 0
    d_i      = psi_1(a_i) - psi_1(a_{i+1}), 0 where negative                           i = 0 .. n,  a_0 = r1, b_{n+1} = r2
    EHVI     = sum_i d_i psi_2(b_{i+1})                                                i ascending
    S        = sum_i (m_1(a_i) + m_1(a_{i+1})) m_2(b_{i+1}),  m(t) = sigma phi(u) + |mu - t| Phi(u)      the magnitude of the terms
    G_mu1 = sum (Phi(u_1,i) - Phi(u_1,i+1)) psi_2(b_{i+1})    G_sigma1 = sum (phi(u_1,i) - phi(u_1,i+1)) psi_2(b_{i+1})     (0 where clamped)
    G_mu2 = sum d_i Phi(u_2,i+1)                              G_sigma2 = sum d_i phi(u_2,i+1)
    grad EHVI = sum_k G_mu_k dmu_k + G_sigma_k ds2_k / (2 sigma_k)
"""
import functools

import numpy as np

import grad_reference as gr
import cacq_reference as cr

MAX_FRONT = 1024


def canonical(front, ref):
    """(a, b) of the canonical front: strictly above ref in both coordinates, no dominated point, no duplicate, a ascending"""
    F = np.asarray(front, dtype=float).reshape(-1, 2)
    F = F[(F[:, 0] > ref[0]) & (F[:, 1] > ref[1])]
    keep = [p for p in F if not np.any(((F[:, 0] >= p[0]) & (F[:, 1] > p[1])) | ((F[:, 0] > p[0]) & (F[:, 1] >= p[1])))]
    K = np.unique(np.array(keep).reshape(-1, 2), axis=0)          # (sorted by the first column, duplicates once)
    return K[:, 0].copy(), K[:, 1].copy()


def psi(erf_mode, mu, sig, t):
    """(psi, Phi, phi, m) at threshold t"""
    dm = mu - t
    cdf, pdf = gr.cdf_pdf(erf_mode, dm / sig)
    return sig * pdf + dm * cdf, cdf, pdf, sig * pdf + np.abs(dm) * cdf


def from_posterior(mu1, s21, mu2, s22, front, ref, erf_mode=gr.ERF_LIBM):
    """dict(val, S, bar, gm1, gs1, gm2, gs2, sig1, sig2) over the candidates (arrays), the sums in the kernel's order;
    bar = psi_1(r1) + psi_2(r2): the bound on dEHVI/dmu_1 + dEHVI/dmu_2"""
    a, b = canonical(front, ref)
    n = len(a)
    mu1, mu2 = np.asarray(mu1, dtype=float), np.asarray(mu2, dtype=float)
    sig1, sig2 = np.sqrt(np.asarray(s21, dtype=float)), np.sqrt(np.asarray(s22, dtype=float))
    z = np.zeros_like(mu1)
    prev, c0, p0, m0 = psi(erf_mode, mu1, sig1, ref[0])
    bar = prev + psi(erf_mode, mu2, sig2, ref[1])[0]
    val, S, gm1, gs1, gm2, gs2 = z.copy(), z.copy(), z.copy(), z.copy(), z.copy(), z.copy()
    for i in range(n + 1):
        if i < n:
            nxt, c1, p1, m1 = psi(erf_mode, mu1, sig1, a[i])
        else:
            nxt, c1, p1, m1 = z, z, z, z
        w, c2, p2, m2 = psi(erf_mode, mu2, sig2, b[i] if i < n else ref[1])
        d = prev - nxt
        neg = d < 0.0
        d = np.where(neg, 0.0, d)
        val = val + d * w
        S = S + (m0 + m1) * m2
        gm1 = gm1 + np.where(neg, 0.0, (c0 - c1) * w)
        gs1 = gs1 + np.where(neg, 0.0, (p0 - p1) * w)
        gm2 = gm2 + d * c2
        gs2 = gs2 + d * p2
        prev, c0, p0, m0 = nxt, c1, p1, m1
    return dict(val=val, S=S, bar=bar, gm1=gm1, gs1=gs1, gm2=gm2, gs2=gs2, sig1=sig1, sig2=sig2)


def value(models, Q, front, ref, erf_mode=gr.ERF_LIBM, clamp_lo=1e-8):
    """from_posterior on the restated posteriors of the two cacq_reference Models at the rows of Q"""
    mu1, s21 = cr.posterior(models[0], Q, clamp_lo)
    mu2, s22 = cr.posterior(models[1], Q, clamp_lo)
    return from_posterior(mu1, s21, mu2, s22, front, ref, erf_mode)


def value_grad(models, Q, front, ref, erf_mode=gr.ERF_LIBM, clamp_lo=1e-8):
    """dict(val, dval (M, D), sval (M, D): the scale -- the same sums over absolute values) at the rows of Q"""
    Q = np.atleast_2d(np.asarray(Q, dtype=float))
    g = [m.ref.grad(Q, sf2k=m.sf2k, clamp_lo=clamp_lo) for m in models]
    r = from_posterior(g[0]["mu"], g[0]["s2"], g[1]["mu"], g[1]["s2"], front, ref, erf_mode)
    # the scale's sums: the magnitudes of the G's are bounded by the same walk over absolute values; Phi <= 1, phi <= 0.4 give
    # |G_mu1|, |G_sigma1| <= 2 psi_2(r2)-like sums -- taken from the terms themselves:
    a = from_posterior_abs(g[0]["mu"], g[0]["s2"], g[1]["mu"], g[1]["s2"], front, ref, erf_mode)
    dval, sval = np.zeros(Q.shape), np.zeros(Q.shape)
    for k, (gm, gs, am, as_) in enumerate(((r["gm1"], r["gs1"], a["gm1"], a["gs1"]), (r["gm2"], r["gs2"], a["gm2"], a["gs2"]))):
        sig = r["sig%d" % (k + 1)]
        dsig, ssig = g[k]["ds2"] / (2 * sig)[:, None], g[k]["ss2"] / (2 * sig)[:, None]
        dval += gm[:, None] * g[k]["dmu"] + gs[:, None] * dsig
        sval += am[:, None] * g[k]["smu"] + as_[:, None] * ssig
    return dict(val=r["val"], dval=dval, sval=sval, S=r["S"])


def from_posterior_abs(mu1, s21, mu2, s22, front, ref, erf_mode):
    """the four partial sums over the absolute values of their terms (no cancellation between strips): the gradient's scale"""
    a, b = canonical(front, ref)
    n = len(a)
    sig1, sig2 = np.sqrt(s21), np.sqrt(s22)
    z = np.zeros_like(np.asarray(mu1, dtype=float))
    _, c0, p0, m0 = psi(erf_mode, mu1, sig1, ref[0])
    gm1, gs1, gm2, gs2 = z.copy(), z.copy(), z.copy(), z.copy()
    for i in range(n + 1):
        _, c1, p1, m1 = psi(erf_mode, mu1, sig1, a[i]) if i < n else (z, z, z, z)
        _, c2, p2, m2 = psi(erf_mode, mu2, sig2, b[i] if i < n else ref[1])
        gm1 = gm1 + (c0 + c1) * m2
        gs1 = gs1 + (p0 + p1) * m2
        gm2 = gm2 + (m0 + m1) * c2
        gs2 = gs2 + (m0 + m1) * p2
        c0, p0, m0 = c1, p1, m1
    return dict(gm1=gm1, gs1=gs1, gm2=gm2, gs2=gs2)


def hvi(front, ref, Y):
    """The hypervolume a new point adds, for the rows y of Y at once, from the staircase: the part of the box [ref, y] above
    h(x) = max(r2, max{b_j : a_j >= x}), integrated over x in [r1, y1] piece by piece.  (Checked against hypervolume(F + {y}) -
    hypervolume(F) in tests/test_ehvi_reference.py; the quadrature of that test integrates this function.)"""
    a, b = canonical(front, ref)
    Y = np.asarray(Y, dtype=float).reshape(-1, 2)
    edges = np.r_[ref[0], a, np.inf]
    height = np.r_[b, ref[1]]
    out = np.zeros(len(Y))
    for k in range(len(height)):
        width = np.clip(np.minimum(Y[:, 0], edges[k + 1]) - edges[k], 0.0, None)
        out += width * np.clip(Y[:, 1] - height[k], 0.0, None)
    return out


# ---- the generator of the cases the GPU tests are compared on
FRONT_SIZES = (0, 1, 2, 63, 64, 65, 1023, 1024)
GEN_M = 1000
GEN_NOISE = 0.1
#        name  D   model 1 (kind, hyper, N, seed, prior)           model 2
GEN = {"d1": (1, ("iso", [.3], 25, 101, False), ("m5", [.45, .9], 40, 102, False)),
       "d3": (3, ("ard", [.5, .6, .45], 200, 103, True), ("m3", [.7, .95], 120, 104, False))}


def objectives(X):
    """the two test objectives at the rows of X: they pull apart (the second falls where the first's argument grows)"""
    return np.sin(3 * X.sum(1)), np.cos(2 * X[:, 0]) - X[:, -1]


def curve_front(n, ref, top, seed=0):
    """A raw front whose canonical form has n points: n points on the concave arc from (r1, top2') to (top1', r2) -- mutually
    non-dominated -- plus clutter that must go: each arc point pulled 10 % towards ref (dominated), every seventh duplicated,
    and points at or below ref in one coordinate; shuffled."""
    rs = np.random.RandomState(1000 + n + seed)
    t = (np.arange(n) + .5) / max(n, 1)
    L = np.asarray(top, dtype=float) - np.asarray(ref, dtype=float)
    arc = np.c_[ref[0] + L[0] * t, ref[1] + L[1] * np.sqrt(1.0 - t * t)]
    clutter = [ref + .9 * (arc - ref), arc[::7], np.c_[np.full(3, ref[0]), ref[1] + L[1] * rs.rand(3)],
               np.c_[ref[0] + L[0] * rs.rand(3), np.full(3, ref[1] - .5)]]
    F = np.vstack([arc] + clutter)
    return F[rs.permutation(len(F))]


@functools.lru_cache(maxsize=None)
def generator(name):
    """dict of one case: the data of both models (observed at different points), the candidates Q, the restated models, the
    reference point (0.1 below the smallest observation of each objective), the objective box's far corner top = max Y, and the
    restated posteriors over Q at clamp 1e-8 -- computed once, shared, to be left unchanged"""
    D, m1, m2 = GEN[name]
    out = dict(D=D, spec=(m1, m2), X=[], Y=[], prior=[], models=[])
    for k, (kind, hyper, N, seed, with_prior) in enumerate((m1, m2)):
        rs = np.random.RandomState(seed)
        X = rs.rand(N, D)
        Y = objectives(X)[k] + .01 * rs.randn(N)
        prior = None
        if with_prior:
            prior = (rs.rand(5, D), .3 * rs.randn(5), 1.5, np.zeros(D) - .1, np.full(D, 1.2))
        out["X"].append(X); out["Y"].append(Y); out["prior"].append(prior)
        out["models"].append(cr.make(X, Y, GEN_NOISE, kind, hyper, prior=prior))
    out["Q"] = np.random.RandomState(105 + D).rand(GEN_M, D) * 1.1 - .05
    out["ref"] = np.array([np.min(out["Y"][0]) - .1, np.min(out["Y"][1]) - .1])
    out["top"] = np.array([np.max(out["Y"][0]), np.max(out["Y"][1])])
    out["post"] = [cr.posterior(m, out["Q"], 1e-8) for m in out["models"]]
    for p in out["post"]:
        for v in p:
            v.setflags(write=False)
    return out


def gen_front(name, n):
    """the raw front of n canonical points for a case: the arc spans 70 % of the objective box [ref, max Y]"""
    g = generator(name)
    return curve_front(n, g["ref"], g["ref"] + .7 * (g["top"] - g["ref"]))


@functools.lru_cache(maxsize=None)
def gen_value(name, n, erf_mode=gr.ERF_LIBM):
    """the restatement over the case's candidates for the front of n points (clamp 1e-8)"""
    g = generator(name)
    (mu1, s21), (mu2, s22) = g["post"]
    r = from_posterior(mu1, s21, mu2, s22, gen_front(name, n), g["ref"], erf_mode)
    for v in r.values():
        v.setflags(write=False)
    return r

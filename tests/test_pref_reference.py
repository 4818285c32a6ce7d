"""
Pins of tests/pref_reference.py (no GPU): the long-double restatement of the preference GP against the oracle and mpmath, and the
host helpers of PrefGaussianProcess (_S_terms, _pair_sum_entries) against the restatement.  tests/test_gpu_pref_model.py then holds
the device path against the same module.
"""
import numpy as np
import pytest

import pref_reference as pr
from conftest import load_golden

LD = np.longdouble


def g7_cases():
    g = load_golden("g7_prefs")
    for name in g["names"]:
        p = str(name) + "/"
        prefs = [(v, u, d) for v, u, d in zip(g[p + "pref_v"], g[p + "pref_u"], g[p + "pref_d"])]
        yield g, p, prefs


def small_problem(kind="ard", noise=.1, seed=3, n=7, mixed=True):
    rs = np.random.RandomState(seed)
    X = rs.rand(n, 2)
    v = rs.randint(0, n, 2 * n); u = (v + 1 + rs.randint(0, n - 1, 2 * n)) % n
    prefs = [(X[a], X[b], int(d)) for a, b, d in zip(v, u, rs.randint(0, 2, 2 * n) if mixed else np.zeros(2 * n, int))]
    hyper = dict(ard=[.4, .6], iso=[.5], m3=[.5, .9], m5=[.5, .9], svard=[.4, .6, .9], sviso=[.5, .9])[kind]
    return pr.PrefProblem(kind, hyper, prefs, noise), rs


def test_nr_constants():
    """sup |Phi_NR - Phi| over [-8, 8] (4001 points) and the jump of Phi_NR at 0, as constants of the reference's function: both enter
    the bounds of the GPU test"""
    sup, jump = pr.nr_constants()
    assert abs(float(sup) - 4.1506375e-08) < 1e-14
    assert abs(float(jump) - 3.00000006e-08) < 1e-15
    # erf_NR itself against the exact erf from mpmath: twice the CDF's figure
    x = np.linspace(LD(-4), LD(4), 801)
    exact = 1 - pr._erfc_ld(x)
    assert 8.2e-8 < np.max(np.abs(pr.erf_nr(x) - exact)) < 8.4e-8
    assert np.max(np.abs(pr.erf_nr(x.astype(float)) - pr.erf_nr(x).astype(float))) < 1e-15


@pytest.mark.parametrize("kind", ["ard", "iso", "m3", "m5", "svard", "sviso"])
def test_corr_matrix_equals_the_oracle(oracle, kind):
    prob, rs = small_problem(kind, noise=.03)
    ok = oracle.Kern(kind, prob.hyper)
    gp = oracle.GP(ok, prob.X, np.zeros(prob.n), noise=.03)
    assert np.max(np.abs(prob.R64 - gp.R)) < 1e-15
    Q = rs.rand(5, 2)
    K = pr.corr_matrix(kind, prob.hyper, prob.X, 0.0, Q).astype(float)
    assert np.max(np.abs(K - np.array([[ok.cov(a, q) for q in Q] for a in prob.X]))) < 1e-15


def test_S_ref_equals_the_oracle_on_g7(oracle):
    for g, p, prefs in g7_cases():
        prob = pr.PrefProblem("ard", g[p + "hyper"], prefs, .1)
        assert np.array_equal(prob.X, g[p + "X"])
        L = np.linalg.cholesky(prob.R64)
        for y in (g[p + "Y"], prob.start(), np.random.RandomState(1).randn(prob.n)):
            want = oracle.pref_S(y, prob.inds, L)
            assert abs(float(prob.S_ref(y)) - want) <= 1e-12 * max(1.0, abs(want))


def test_gradient_and_hessian_of_S_smooth_against_mpmath():
    import mpmath
    prob, rs = small_problem()
    y = rs.randn(prob.n)
    with mpmath.workprec(200):
        Rinv = mpmath.matrix([[mpmath.mpf(float(a)) + mpmath.mpf(float(a - LD(float(a)))) for a in row] for row in prob.R]) ** -1
        c = mpmath.mpf(float(pr.ISQ2))

        def S(*yy):
            s = sum(yy[i] * Rinv[i, j] * yy[j] for i in range(prob.n) for j in range(prob.n)) / 2
            for v, u, w in zip(prob.v, prob.u, prob.w):
                z = (yy[v] - yy[u]) / mpmath.sqrt(2)
                s -= float(w) * mpmath.log(mpmath.erfc(-c * z) / 2 + mpmath.mpf(float(pr.EPS_CDF)))
            return s

        g = prob.grad_smooth(y)
        H = prob.hessian(y)
        for i in range(prob.n):
            order = [0] * prob.n; order[i] = 1
            want = mpmath.diff(S, tuple(mpmath.mpf(t) for t in y), tuple(order))
            assert abs(float(g[i]) - float(want)) <= 1e-15 * max(1.0, abs(float(want)))
        for i, j in ((0, 0), (1, 4), (5, 2)):
            order = [0] * prob.n; order[i] += 1; order[j] += 1
            want = float(mpmath.diff(S, tuple(mpmath.mpf(t) for t in y), tuple(order)))
            assert abs(H[i, j] - want) <= 1e-11 * max(1.0, abs(want))
    assert float(prob.S_smooth(y)) == pytest.approx(float(S(*[mpmath.mpf(t) for t in y])), rel=1e-15)


def test_S_terms_returns_the_stated_gradient_and_the_hessian_weights():
    """PrefGaussianProcess._S_terms: S = S_ref, g = grad_stated, rho = the Hessian weights of S_smooth up to the NR / exact difference
    in the denominator (relative 2 sup|Phi_NR - Phi| / Phi < 1e-6 for z > -1.5)"""
    from ibo_amd.gaussianprocess import PrefGaussianProcess
    for kind, noise in (("ard", .1), ("m5", 1e-2), ("sviso", 1e-3)):
        prob, rs = small_problem(kind, noise, n=9)
        for y in (rs.randn(prob.n) * .5, prob.start()):
            Ry = prob.rinv_mul(y).astype(float)
            S, g, rho = PrefGaussianProcess._S_terms(np.asarray(y, float), Ry, prob.v, prob.u, prob.w.astype(float))
            assert abs(S - float(prob.S_ref(y))) <= 1e-13 * max(1.0, abs(S))
            scale = max(1.0, np.max(np.abs(Ry)))
            assert np.max(np.abs(g - prob.grad_stated(y).astype(float))) <= 1e-14 * scale
            want = prob.rho_smooth(y).astype(float)
            z = prob.z(y).astype(float)
            assert np.all(z > -1.5) and np.max(np.abs(rho - want) / np.abs(want)) < 1e-6
            assert np.max(np.abs(rho - want) / np.abs(want)) > 1e-10            # (and the two really are different functions)


def test_pair_sum_entries_rebuild_the_pair_matrix():
    from ibo_amd.gaussianprocess import PrefGaussianProcess
    n = 9
    shapes = dict(star=(np.zeros(n - 1, int), np.arange(1, n)), chain=(np.arange(n - 1), np.arange(1, n)),
                  cycle=(np.array([0, 1, 2, 4]), np.array([1, 2, 0, 5])), both=(np.array([3, 7, 3, 1]), np.array([7, 3, 7, 3])))
    rs = np.random.RandomState(2)
    for name, (v, u) in shapes.items():
        w = rs.randn(len(v))                                  # signs mixed, as the Laplace weights can be
        lin, val = PrefGaussianProcess._pair_sum_entries(n, v, u, w)
        assert len(np.unique(lin)) == len(lin) and lin.dtype == np.int64
        M = np.zeros(n * n); M[lin] = val
        want = pr.pair_matrix(n, v, u, w)
        A = np.zeros((n, len(v))); A[v, np.arange(len(v))] = 1; A[u, np.arange(len(v))] -= 1
        assert np.max(np.abs(want - (A * w).dot(A.T))) < 1e-14, name
        assert np.array_equal(M.reshape(n, n), want), name        # same entries, summed in the reference's order
        assert set(lin.tolist()) == set(np.flatnonzero((np.abs(A).dot(np.abs(A.T))).ravel()).tolist()), name


def test_model_steps_equal_the_oracle_on_g7(oracle):
    for g, p, prefs in g7_cases():
        prob = pr.PrefProblem("ard", g[p + "hyper"], prefs, .1)
        Y = g[p + "Y"]
        steps = pr.model_steps(prob, Y)
        ogp = oracle.pref_fit(oracle.Kern("ard", g[p + "hyper"]), prefs, noise=.1, Y_map=Y)
        assert steps["identities"] == 0
        np.testing.assert_allclose(steps["C"], ogp.C, rtol=1e-9, atol=1e-11)
        np.testing.assert_allclose(steps["C"], g[p + "C"], rtol=1e-6, atol=1e-9)
        np.testing.assert_allclose(steps["L"], ogp.L, rtol=1e-9, atol=1e-11)
        np.testing.assert_allclose(steps["L"], g[p + "L"], rtol=1e-6, atol=1e-9)
        mu, s2 = pr.oracle_model(prob, Y, steps["L"], steps["M"]).posteriors(g[p + "probe"])
        np.testing.assert_allclose(mu, g[p + "post"][:, 0], rtol=1e-6, atol=1e-9)
        np.testing.assert_allclose(s2, g[p + "post"][:, 1], rtol=1e-6)
        acc = pr.reference_accuracy(prob, steps, Y, g[p + "probe"][:5])
        assert max(acc.values()) < 1e-12                         # at noise 0.1 the reference's float64 is accurate to rounding


def test_model_steps_with_negative_weights_equal_the_oracle(oracle):
    """the issue's first probe case with a violated preference at noise 1e-2: weights below zero, C indefinite, and the reference's
    LU inverse goes through with no identity added -- the oracle's loop and the restated one agree"""
    import test_gpu_pref_model as T
    c = [c for c in T.CASES if c["id"] == "neg-n40-noise1e-2"][0]
    prefs = T.make_prefs(c["seed"], c["n"], c["D"], **c["kw"])
    prob = pr.PrefProblem(c["kind"], c["hyper"], prefs, c["noise"])
    ystar, nsteps, H = prob.minimise()
    Y, fired = pr.order_fixup(ystar.astype(float), prob.inds)
    steps = pr.model_steps(prob, Y)
    assert (steps["w"] < 0).sum() >= 1 and np.linalg.eigvalsh(steps["C"])[0] < 0 and steps["identities"] == 0
    ogp = oracle.pref_fit(oracle.Kern(c["kind"], c["hyper"]), prefs, noise=c["noise"], Y_map=Y)
    np.testing.assert_allclose(steps["C"], ogp.C, rtol=1e-7, atol=1e-9 * np.abs(steps["w"]).max())
    np.testing.assert_allclose(steps["L"], ogp.L, rtol=1e-6, atol=1e-8)


def test_minimise_finds_the_minimiser():
    for kind, noise in (("ard", .1), ("m3", 1e-3)):
        prob, rs = small_problem(kind, noise, n=12)
        y, steps, H = prob.minimise()
        assert 2 <= steps <= 8
        assert float(np.max(np.abs(prob.grad_smooth(y)))) <= 1e-12 * max(1.0, float(np.max(np.abs(y))))
        assert np.linalg.eigvalsh(H - prob.rinv64())[0] > -1e-9 * np.abs(H).max()      # Hessian >= R^-1
        S0 = prob.S_smooth(y)
        for _ in range(5):
            assert prob.S_smooth(y + LD(1e-4) * rs.randn(prob.n)) > S0
        y2, _, _ = prob.minimise(start=rs.randn(prob.n))          # one minimiser whatever the start
        assert float(np.max(np.abs(y2 - y))) < 1e-11


def test_order_fixup_and_add_observation(oracle):
    # 0 > 1, 2 > 1, 1 > 3: point 2 came out below 1 and is never unpreferred -> lifted; point 1 is below 3 but is unpreferred -> kept
    inds = [(0, 1, 0), (2, 1, 0), (1, 3, 0)]
    Y, fired = pr.order_fixup([1.0, 0.2, 0.1, 0.5], inds)
    assert fired == 1 and np.array_equal(Y, [1.0, 0.2, 0.2 + .1, 0.5])
    prob, rs = small_problem("svard", .05)
    y, _, _ = prob.minimise()
    steps = pr.model_steps(prob, y.astype(float))
    augX = np.vstack([prob.X, rs.rand(3, 2)])
    augR, augL = pr.add_observation(prob, steps, augX)
    ok = oracle.Kern("svard", prob.hyper)
    want = np.array([[ok.cov(a, b) for b in augX] for a in augX]); np.fill_diagonal(want, 1.05)
    assert np.max(np.abs(augR - want)) < 1e-15
    pad = np.zeros_like(want); pad[:prob.n, :prob.n] = np.linalg.inv(steps["C"])
    assert np.max(np.abs(augL.dot(augL.T) - (want + pad))) < 1e-13

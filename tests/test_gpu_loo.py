"""
Leave-one-out predictions on a fitted handle (ibo_gp_loo, GaussianProcess.loo / .loo_score) and the LOO-CV objective with its gradient
(ibo_loo_grad, trainhyper.looLikelihood / nloo / dnloo; csrc/loo.hip).

The yardstick is tests/loo_reference.py in float64, pinned to the oracle by tests/test_loo_reference.py.  Bars (the project's own):
    value     1e-9 (N + |v|)                  the NLML tests' 1e-9, scaled by N because the value crosses zero
    gradient  1e-9 S_h                        S_h = sum_i [|alpha_i r_i| + (1 + alpha_i^2 / d_i) |s_i| / 2] / d_i, the terms' magnitudes
    mu_-i     1e-9 (|Y_i| + |alpha_i| / d_i)
    s2_-i     1e-9 relative
Every case asserts cond_2 <= 1e6 from the reference first: a bar is never met by an ill-posed input.
"""
import ctypes

import numpy as np
import pytest

import loo_reference as lr
from conftest import synth
from oracle import oracle as orc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    from ibo_amd import _lib
    if _lib.device_count() < 1:
        pytest.fail("no GPU visible: the product has no CPU fallback")
    return _lib


BASE = {"iso": [.45], "sviso": [.45, .8], "m3": [.5, .95], "m5": [.5, .9]}


def hyper_of(kind, D):
    s = max(1.0, np.sqrt(D) / 2)
    ell = np.linspace(.35, .6, D) * s
    if kind == "ard":
        return list(ell)
    if kind == "svard":
        return list(ell) + [.9]
    return [h * (s if i == 0 else 1.0) for i, h in enumerate(BASE[kind])]


def make_kernel(kind, hyper):
    from ibo_amd.gaussianprocess import kernel as K
    return {"ard": K.GaussianKernel_ard, "iso": K.GaussianKernel_iso, "svard": K.SVGaussianKernel_ard,
            "sviso": K.SVGaussianKernel_iso, "m3": K.MaternKernel3, "m5": K.MaternKernel5}[kind](np.array(hyper, dtype=float))


def make_priors(D, seed=11):
    """the same RBF-network prior for the model and for the oracle"""
    from ibo_amd.gaussianprocess.prior import RBFNMeanPrior
    rs = np.random.RandomState(seed)
    p = RBFNMeanPrior()
    p.means = rs.rand(5, D); p.beta = rs.randn(5); p.theta = 1.5; p.lowerb = np.zeros(D) - .1; p.width = np.full(D, 1.2)
    return p, orc.Prior(p.means, p.beta, p.theta, p.lowerb, p.width)


def check_points(got, ref, Y, what=""):
    """got: (mu, s2, value or None) against a loo_reference result"""
    assert ref["cond"] <= 1e6, (what, ref["cond"])
    mu, s2, v = got
    N = len(Y)
    emu = np.abs(mu - ref["mu"]); tmu = 1e-9 * (np.abs(Y) + np.abs(ref["c"]) / ref["d"])
    es2 = np.abs(s2 - ref["s2"]) / ref["s2"]
    print("%s: cond %.3g  mu err/bar %.3g  s2 rel err %.3g" % (what, ref["cond"], np.max(emu / tmu), es2.max()))
    assert np.all(emu <= tmu), what
    assert np.all(es2 <= 1e-9), what
    if v is not None:
        print("%s: value %.15g want %.15g" % (what, v, ref["value"]))
        assert abs(v - ref["value"]) <= 1e-9 * (N + abs(ref["value"])), what


def check_grad(g, ref, what=""):
    err = np.abs(np.asarray(g) - ref["grad"])
    print("%s: gradient err / S_h max %.3g" % (what, np.max(err / np.maximum(ref["S"], 1e-300)) if len(err) else 0.0))
    assert np.all(err <= 1e-9 * ref["S"]), (what, g, ref["grad"], ref["S"])


# ---------------------------------------------------------------------------------------------------------------- 1. handles
HANDLE_CASES = [  # kind, N, D, noise, prior: every family, every N, every D, both noises, with and without a prior
    ("ard", 1, 1, .1, False), ("iso", 1, 3, 1e-2, True), ("svard", 2, 3, .1, True), ("sviso", 63, 33, 1e-2, False),
    ("m3", 64, 3, .1, True), ("m5", 65, 1, 1e-2, False), ("ard", 200, 33, .1, True), ("iso", 200, 3, 1e-2, False),
    ("svard", 1025, 3, 1e-2, False), ("sviso", 1025, 1, .1, True), ("m3", 1025, 33, 1e-2, True), ("m5", 200, 3, .1, False),
    ("ard", 65, 3, 1e-2, True), ("m5", 64, 33, .1, True), ("iso", 63, 1, .1, False), ("m3", 2, 1, 1e-2, False)]


def handle_model(kind, N, D, noise, prior, seed=None):
    from ibo_amd.gaussianprocess import GaussianProcess
    X, Y = synth(N + D if seed is None else seed, N, D)
    hyper = hyper_of(kind, D)
    p, op = make_priors(D) if prior else (None, None)
    GP = GaussianProcess(make_kernel(kind, hyper), X, Y, prior=p, noise=noise)
    return GP, orc.GP(orc.Kern(kind, hyper), X, Y, noise=noise, prior=op), X, Y


@pytest.mark.parametrize("kind,N,D,noise,prior", HANDLE_CASES)
def test_loo_on_a_handle(lib, kind, N, D, noise, prior):
    GP, ogp, X, Y = handle_model(kind, N, D, noise, prior)
    ref = lr.handle_loo(ogp)
    mu, s2 = GP.loo()
    v = GP.loo_score()
    check_points((mu, s2, v), ref, Y, "%s N=%d D=%d" % (kind, N, D))
    # the score is the sum of the per-point terms of the predictions it came with
    terms = 0.5 * np.log(s2) + (Y - mu) ** 2 / (2 * s2) + lr.HALF_LOG_2PI
    assert abs(v - terms.sum()) <= 1e-9 * (N + abs(v))
    if N == 1:                                     # the prior predictive
        m = ogp.prior.mu(X[0]) if prior else 0.0
        assert abs(mu[0] - m) <= 1e-12 * (1 + abs(Y[0])) and abs(s2[0] - (1 + noise)) <= 1e-12
    # a repeat gives the same bits
    mu2, s22 = GP.loo()
    assert np.array_equal(mu, mu2) and np.array_equal(s2, s22) and GP.loo_score() == v


def test_loo_against_oracle_refits(lib):
    GP, ogp, X, Y = handle_model("ard", 65, 3, .1, True)
    mu, s2 = GP.loo()
    for i in (0, 17, 33, 63, 64):
        omu, os2 = lr.brute_force(ogp.kern, X, Y, .1, ogp.prior, i)
        assert abs(mu[i] - omu) <= 1e-9 * (abs(Y[i]) + abs(Y[i] - omu)) and abs(s2[i] - os2) <= 1e-9 * os2, i


def test_loo_after_block_extension(lib):
    """63 -> 64 -> 73 rows by addData (ibo_gp_extend, across a 64-row boundary) against a fresh model and the reference"""
    from ibo_amd.gaussianprocess import GaussianProcess
    kind, D, noise = "svard", 3, .1
    X, Y = synth(77, 73, D)
    hyper = hyper_of(kind, D)
    GP = GaussianProcess(make_kernel(kind, hyper), X[:63], Y[:63], noise=noise, reserve_rows=16)
    for n in (64, 73):
        GP.addData(X[len(GP.X):n], Y[len(GP.Y):n])
        assert len(GP.X) == n
        ref = lr.handle_loo(orc.GP(orc.Kern(kind, hyper), X[:n], Y[:n], noise=noise))
        mu, s2 = GP.loo()
        check_points((mu, s2, GP.loo_score()), ref, Y[:n], "extended to %d" % n)
        fresh = GaussianProcess(make_kernel(kind, hyper), X[:n], Y[:n], noise=noise)
        fmu, fs2 = fresh.loo()
        assert np.all(np.abs(mu - fmu) <= 1e-9 * (np.abs(Y[:n]) + np.abs(ref["c"]) / ref["d"]))
        assert np.all(np.abs(s2 - fs2) <= 1e-9 * fs2)


def test_loo_errors_and_the_preference_gp(lib):
    from ibo_amd.gaussianprocess import GaussianProcess, PrefGaussianProcess
    from ibo_amd.gaussianprocess.kernel import GaussianKernel_ard
    dp = lib.dp
    mu = np.empty(4)
    h = ctypes.c_void_p()
    lib.check(lib.lib.ibo_gp_create(lib.default_device(), ctypes.byref(h)))
    try:
        assert lib.lib.ibo_gp_loo(h, dp(mu), None, None) == lib.ERR_STATE
    finally:
        lib.check(lib.lib.ibo_gp_destroy(h))
    X, Y = synth(3, 4, 2)
    GP = GaussianProcess(GaussianKernel_ard([.5, .5]), X, Y)
    assert lib.lib.ibo_gp_loo(GP._handle(), None, None, None) == lib.ERR_ARG
    assert lib.lib.ibo_gp_loo(None, dp(mu), None, None) == lib.ERR_ARG
    v = ctypes.c_double()
    lib.check(lib.lib.ibo_gp_loo(GP._handle(), None, None, ctypes.byref(v)))
    assert v.value == GP.loo_score()
    P = PrefGaussianProcess(GaussianKernel_ard([.5, .5]))
    with pytest.raises(NotImplementedError):
        P.loo()
    with pytest.raises(NotImplementedError):
        P.loo_score()


# ---------------------------------------------------------------------------------------------------------------- 2-4. looLikelihood
_REFS = {}


def reference(case):
    """the float64 restatement of one case, computed once"""
    key = (case[0], tuple(case[1])) + tuple(case[2:])
    if key not in _REFS:
        kind, hyper, N, D, seed = case
        X, Y = synth(seed, N, D)
        _REFS[key] = (X, Y, lr.objective(orc.Kern(kind, hyper), X, Y, lr.NOISE, len(hyper)))
    return _REFS[key]


def run_case(case, repeat=False):
    from ibo_amd.gaussianprocess.trainhyper import looLikelihood
    kind, hyper, N, D, seed = case
    X, Y, ref = reference(case)
    what = "%s N=%d D=%d" % (kind, N, D)
    k = make_kernel(kind, hyper)
    v, g, (mu, s2) = looLikelihood(k, X, Y, len(hyper), True, noise=lr.NOISE, predictions=True)
    check_points((mu, s2, v), ref, Y, what)
    check_grad(g, ref, what)
    # value only (no gradient product): the same bits
    v0 = looLikelihood(k, X, Y, len(hyper), False, noise=lr.NOISE)
    assert v0 == v
    if repeat:
        v2, g2, (mu2, s22) = looLikelihood(k, X, Y, len(hyper), True, noise=lr.NOISE, predictions=True)
        assert v2 == v and np.array_equal(g, g2) and np.array_equal(mu, mu2) and np.array_equal(s2, s22)


@pytest.mark.parametrize("case", lr.FAMILY_CASES, ids=lambda c: "%s-N%d-D%d" % (c[0], c[2], c[3]))
def test_loo_likelihood_every_family(lib, case):
    run_case(case)


@pytest.mark.parametrize("case", lr.EDGE_CASES, ids=lambda c: "%s-N%d-D%d" % (c[0], c[2], c[3]))
def test_loo_likelihood_tile_and_pass_edges(lib, case):
    """rows around the 64 x 64 tile and the k-step of 32; 64 gradients: sixteen passes of four"""
    run_case(case, repeat=True)


def test_loo_likelihood_partial_pass(lib):
    """five and six derivatives: a last pass of one and of two after a full one (ARD with signal variance; the first of its length scales only)"""
    from ibo_amd.gaussianprocess.trainhyper import looLikelihood
    X, Y, ref = reference(lr.FAMILY_CASES[7])
    k = make_kernel("svard", lr.FAMILY_CASES[7][1])
    v, g = looLikelihood(k, X, Y, 5, True, noise=lr.NOISE)
    check_grad(g, ref, "svard, 5 derivatives")
    v3, g3 = looLikelihood(k, X, Y, 3, True, noise=lr.NOISE)
    assert v3 == v and np.array_equal(g3, g[:3])
    X, Y = synth(9, 70, 5)
    hyper = [.5, .6, .7, .8, .9, 1.1]
    ref = lr.objective(orc.Kern("svard", hyper), X, Y, lr.NOISE, 6)
    assert ref["cond"] <= 1e6
    v, g = looLikelihood(make_kernel("svard", hyper), X, Y, 6, True, noise=lr.NOISE)
    check_grad(g, ref, "svard, 6 derivatives")


@pytest.mark.parametrize("case", lr.ROUTE_CASES + [lr.BIG_CASE], ids=lambda c: "%s-N%d-D%d" % (c[0], c[2], c[3]))
def test_loo_likelihood_on_each_route_to_the_inverse(lib, case):
    """wtw_kernel's last size, the first packed-operand size, a 64-row last tile row, the 512-piece range; 6700 rows: the two-level order,
    whose K^-1 lies in the other buffer"""
    run_case(case, repeat=True)


def test_nlml_and_loo_gradients_on_a_small_two_level_matrix(lib):
    """fused2_min_nb = 3 sends 150 rows (three block columns) of ibo_nlml_grad and ibo_loo_grad through the two-level order and the
    doubling tail (launch_trinv without a fill, launch_pack_w) that the 6700-row cases reach by size: value to 1e-9 relative, gradient to
    1e-8 of its largest component (test_nlml_gradient_on_the_two_level_branch's bounds) against the float64 restatements, the
    leave-one-out predictions to check_points' bounds, and a repeat gives the same bits."""
    from ibo_amd.gaussianprocess.trainhyper import looLikelihood, marginalLikelihood
    theta, D, N = [.4, .5, .6], 3, 150
    X, Y = synth(150, N, D)
    k, ok = make_kernel("ard", theta), orc.Kern("ard", theta)
    ov, og = orc.marginal_likelihood(ok, X, Y, D, True, lr.NOISE)
    ref = lr.objective(ok, X, Y, lr.NOISE, D)
    lib.check(lib.lib.ibo_set_option(b"fused2_min_nb", 3))
    try:
        v, g = marginalLikelihood(k, X, Y, D, True, noise=lr.NOISE)
        lv, lg, (mu, s2) = looLikelihood(k, X, Y, D, True, noise=lr.NOISE, predictions=True)
        v2, g2 = marginalLikelihood(k, X, Y, D, True, noise=lr.NOISE)
        lv2, lg2, (mu2, s22) = looLikelihood(k, X, Y, D, True, noise=lr.NOISE, predictions=True)
    finally:
        lib.check(lib.lib.ibo_set_option(b"fused2_min_nb", 104))
    g, lg, og = np.asarray(g), np.asarray(lg), np.asarray(og)
    print("nlml: value rel err %.3g  gradient err / max %.3g" % (abs(v - ov) / abs(ov), np.abs(g - og).max() / np.abs(og).max()))
    print("loo:  value rel err %.3g  gradient err / max %.3g" % (abs(lv - ref["value"]) / abs(ref["value"]),
                                                                 np.abs(lg - ref["grad"]).max() / np.abs(ref["grad"]).max()))
    assert abs(v - ov) <= 1e-9 * abs(ov) and np.abs(g - og).max() <= 1e-8 * np.abs(og).max(), (v, ov, g, og)
    assert abs(lv - ref["value"]) <= 1e-9 * abs(ref["value"]) and np.abs(lg - ref["grad"]).max() <= 1e-8 * np.abs(ref["grad"]).max(), \
        (lv, ref["value"], lg, ref["grad"])
    check_points((mu, s2, None), ref, Y, "two-level, 150 rows")
    assert v2 == v and np.array_equal(np.asarray(g2), g)
    assert lv2 == lv and np.array_equal(np.asarray(lg2), lg) and np.array_equal(mu2, mu) and np.array_equal(s22, s2)


# ---------------------------------------------------------------------------------------------------------------- 5. shared workspace
def test_loo_and_nlml_share_one_workspace(lib):
    from ibo_amd.gaussianprocess.trainhyper import looLikelihood, marginalLikelihood
    theta, D, N = [.4, .5, .6], 3, 300
    X, Y = synth(41, N, D)
    Y2 = np.cos(2 * X.sum(1))
    k = make_kernel("ard", theta)
    ok = orc.Kern("ard", theta)
    r1 = lr.objective(ok, X, Y, lr.NOISE, D); r2 = lr.objective(ok, X, Y2, lr.NOISE, D)
    # the NLML calls alone
    lib.trim()
    plain = [marginalLikelihood(k, X, Y, D, True, noise=lr.NOISE) for _ in range(2)]
    lib.trim()
    plain.append(marginalLikelihood(k, X, Y, D, True, noise=lr.NOISE))
    # ... and with LOO calls in between
    lib.trim()
    mixed, loos = [], []
    mixed.append(marginalLikelihood(k, X, Y, D, True, noise=lr.NOISE))
    loos.append((looLikelihood(k, X, Y, D, True, noise=lr.NOISE, predictions=True), r1, Y))
    mixed.append(marginalLikelihood(k, X, Y, D, True, noise=lr.NOISE))
    loos.append((looLikelihood(k, X, Y2, D, True, noise=lr.NOISE, predictions=True), r2, Y2))
    lib.trim()
    mixed.append(marginalLikelihood(k, X, Y, D, True, noise=lr.NOISE))
    loos.append((looLikelihood(k, X, Y, D, True, noise=lr.NOISE, predictions=True), r1, Y))
    for (v, g), (pv, pg) in zip(mixed, plain):
        assert v == pv and np.array_equal(g, pg)
    for (v, g, (mu, s2)), ref, y in loos:
        check_points((mu, s2, v), ref, y, "interleaved")
        check_grad(g, ref, "interleaved")


# ---------------------------------------------------------------------------------------------------------------- 6. not positive definite
def test_loo_likelihood_not_positive_definite(lib):
    from numpy.linalg import LinAlgError
    from ibo_amd.gaussianprocess import kernel as K
    from ibo_amd.gaussianprocess.trainhyper import looLikelihood, nloo
    X, Y = synth(5, 40, 3)
    Xd = np.r_[X, X[:3]]; Yd = np.r_[Y, Y[:3]]
    k = make_kernel("ard", [.4, .5, .6])
    with pytest.raises(LinAlgError):
        looLikelihood(k, Xd, Yd, 3, True, noise=0.0)
    with pytest.raises(LinAlgError):
        looLikelihood(k, Xd, Yd, 3, False, noise=0.0)
    assert nloo(np.log([.4, .5, .6]), K.GaussianKernel_ard, Xd, Yd, 0.0) == 100
    ref = lr.objective(orc.Kern("ard", [.4, .5, .6]), X, Y, lr.NOISE, 3)
    v, g, (mu, s2) = looLikelihood(k, X, Y, 3, True, noise=lr.NOISE, predictions=True)
    check_points((mu, s2, v), ref, Y, "after a failed call")
    check_grad(g, ref, "after a failed call")


# ---------------------------------------------------------------------------------------------------------------- 7. learning
def test_bfgs_on_the_loo_objective(lib):
    from scipy.optimize import fmin_bfgs
    from ibo_amd.gaussianprocess import kernel as K
    from ibo_amd.gaussianprocess.trainhyper import nloo, dnloo
    X, Y = synth(21, 200, 2)
    x0 = np.log([.3, .3])
    f0 = nloo(x0, K.GaussianKernel_ard, X, Y)
    xs = fmin_bfgs(nloo, x0, dnloo, args=(K.GaussianKernel_ard, X, Y), maxiter=30, disp=False)
    f1 = nloo(xs, K.GaussianKernel_ard, X, Y)
    assert f1 < f0
    # (nloo / dnloo run at looLikelihood's default noise, 1e-3)
    g0 = lr.objective(orc.Kern("ard", np.exp(x0)), X, Y, 1e-3, 2)
    g1 = lr.objective(orc.Kern("ard", np.exp(xs)), X, Y, 1e-3, 2)
    assert g0["cond"] <= 1e6 and g1["cond"] <= 1e6
    print("start %.6g -> %.6g, |g| %.3g -> %.3g" % (f0, f1, np.abs(g0["grad"]).max(), np.abs(g1["grad"]).max()))
    assert np.abs(g1["grad"]).max() <= 1e-4 * np.abs(g0["grad"]).max()

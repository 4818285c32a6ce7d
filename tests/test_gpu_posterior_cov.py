"""
ibo_posterior_cov / ibo_posterior_sample and what is built on them: GaussianProcess.posterior_cov, .sample_posterior and
acquisition.gallery.thompsonGallery.

The yardstick is tests/cov_reference.py, the joint posterior restated in NumPy/SciPy float64 and pinned to the oracle by
tests/test_cov_reference.py.  Tolerance: |dSigma_ab| <= 1e-10 (sf2 + noise + |v_a| |v_b|).  The conditioning test ties Sigma to
the device's own fit and extension path (addData on a copy), which is independent code.
"""
import ctypes
from copy import deepcopy

import numpy as np
import pytest
from scipy.linalg.lapack import dpotrf

import cov_reference as cr
import grad_reference as gr
from conftest import synth

pytestmark = pytest.mark.gpu

KINDS = ["ard", "iso", "svard", "sviso", "m3", "m5"]
BASE = {"iso": [.45], "sviso": [.45, .8], "m3": [.5, .95], "m5": [.5, .9]}


@pytest.fixture(scope="module")
def lib():
    from ibo_amd import _lib
    if _lib.device_count() < 1:
        pytest.fail("no GPU visible: the product has no CPU fallback")
    return _lib


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


def make_prior(D, seed=11):
    from ibo_amd.gaussianprocess.prior import RBFNMeanPrior
    rs = np.random.RandomState(seed)
    p = RBFNMeanPrior()
    p.means = rs.rand(5, D); p.beta = rs.randn(5); p.theta = 1.5; p.lowerb = np.zeros(D) - .1; p.width = np.full(D, 1.2)
    return p


def model(kind, N, D, seed=1, noise=.1, prior=False, hyper=None):
    from ibo_amd.gaussianprocess import GaussianProcess
    X, Y = synth(seed, N, D)
    hyper = hyper_of(kind, D) if hyper is None else hyper
    GP = GaussianProcess(make_kernel(kind, hyper), X, Y, prior=make_prior(D) if prior else None, noise=noise)
    fam, w, sf2 = gr.kernel_spec(kind, hyper, D)
    return GP, gr.RefGP(X, Y, noise, fam, w, sf2)


def queries(X, M, seed=2):
    """M points: half near observations (small variance), half spread over the box and a little beyond"""
    rs = np.random.RandomState(seed)
    D = X.shape[1]
    near = X[rs.randint(0, len(X), (M + 1) // 2)] + .02 * rs.randn((M + 1) // 2, D)
    return np.r_[near, rs.rand(M // 2, D) * 1.2 - .1][:M]


def cov_call(lib, h, Q, with_noise=1, guard=False):
    Q = lib.f64(np.atleast_2d(Q))
    M = len(Q)
    pad = 8 if guard else 0
    mu = np.full(M + pad, 7.25); S = np.full(M * M + pad, 7.25)
    lib.check(lib.lib.ibo_posterior_cov(h, M, lib.dp(Q), with_noise, lib.dp(mu), lib.dp(S)))
    if guard:
        assert np.all(mu[M:] == 7.25) and np.all(S[M * M:] == 7.25), "guard overwritten"
    return mu[:M], S[:M * M].reshape(M, M)


def sample_call(lib, h, Q, Z, with_noise=1, jitter=0.0, guard=False):
    Q = lib.f64(np.atleast_2d(Q)); Z = lib.f64(np.atleast_2d(Z))
    M, n = len(Q), len(Z)
    pad = 8 if guard else 0
    F = np.full(n * M + pad, 7.25); mu = np.full(M + pad, 7.25)
    info = ctypes.c_int(-1)
    rc = lib.lib.ibo_posterior_sample(h, M, lib.dp(Q), with_noise, jitter, n, lib.dp(Z), lib.dp(F), lib.dp(mu), ctypes.byref(info))
    if guard:
        assert np.all(F[n * M:] == 7.25) and np.all(mu[M:] == 7.25), "guard overwritten"
    return rc, info.value, mu[:M], F[:n * M].reshape(n, M)


CASES = [  # kind, D, N, M, prior
    ("ard", 1, 1, 1, False), ("iso", 3, 2, 2, True), ("svard", 3, 63, 15, False), ("sviso", 8, 64, 16, True),
    ("m3", 3, 65, 17, False), ("m5", 8, 700, 63, True), ("ard", 8, 700, 64, False), ("iso", 64, 65, 65, False),
    ("svard", 64, 700, 127, True), ("m3", 8, 4100, 128, False), ("m5", 3, 63, 129, False), ("sviso", 1, 700, 1000, False),
    ("ard", 3, 4100, 1000, True), ("m5", 64, 64, 2, False),
]


@pytest.mark.parametrize("kind,D,N,M,prior", CASES)
def test_sigma_against_the_restatement(lib, kind, D, N, M, prior):
    GP, ref = model(kind, N, D, prior=prior)
    h = GP._handle()
    Q = queries(GP.X, M)
    mu0, s20 = GP.posteriors(Q)
    for wn in (1, 0):
        mu, S = cov_call(lib, h, Q, wn)
        Sref, vn = cr.cov(ref, Q, with_noise=bool(wn))
        cr.assert_cov_close(S, Sref, vn, ref.sf2, ref.noise, what="%s D=%d N=%d M=%d noise=%d" % (kind, D, N, M, wn))
        assert np.array_equal(mu, mu0)
        assert np.array_equal(S, S.T)
        if wn:
            live = (s20 > 1e-7) & (s20 < 10)
            np.testing.assert_allclose(np.diag(S)[live], s20[live], rtol=1e-10)
        mu2, S2 = cov_call(lib, h, Q, wn)
        assert np.array_equal(S, S2) and np.array_equal(mu, mu2)
    m1, S1 = GP.posterior_cov(Q)
    assert np.array_equal(m1, mu0) and np.array_equal(S1, cov_call(lib, h, Q)[1])
    m2, S2 = GP.posterior_cov(Q[0])
    assert S2.shape == (1, 1) and np.array_equal(m2, GP.posteriors(Q[:1])[0])      # (a batch of one: the small-batch route)


def test_conditioning_against_the_fit_path(lib):
    GP, ref = model("m5", 200, 4)
    Q = queries(GP.X, 24, seed=8)
    _, S = GP.posterior_cov(Q)
    for j in (0, 11, 23):
        G2 = deepcopy(GP)
        G2.addData(Q[j:j + 1], np.array([0.25]))
        _, s2 = G2.posteriors(Q)
        want = np.diag(S) - S[:, j] ** 2 / S[j, j]
        live = (np.arange(len(Q)) != j) & (s2 > 1e-7) & (s2 < 10)
        np.testing.assert_allclose(s2[live], want[live], rtol=1e-9, atol=1e-12)


def test_preference_gp_and_augmented_factor(lib):
    from ibo_amd.gaussianprocess import PrefGaussianProcess
    from ibo_amd.gaussianprocess.kernel import GaussianKernel_ard
    rs = np.random.RandomState(3)
    D = 6
    hyper = [.6] * D
    GP = PrefGaussianProcess(GaussianKernel_ard(np.array(hyper)))
    P = rs.rand(60, D)
    GP.addPreferences([(P[2 * i], P[2 * i + 1], 0) for i in range(30)])
    fam, w, sf2 = gr.kernel_spec("ard", hyper, D)
    Q = rs.rand(40, D)
    mu, S = GP.posterior_cov(Q)
    np.testing.assert_array_equal(mu, GP.posteriors(Q)[0])
    Sref, vn = cr.cov_L(GP.L, GP.X, fam, w, sf2, GP.noise, Q)
    cr.assert_cov_close(S, Sref, vn, sf2, GP.noise, what="preferences")
    assert np.array_equal(S, S.T)
    GP.addObservationPoint(rs.rand(D))
    mu, S = GP.posterior_cov(Q)
    m0, s0 = GP.posteriors(Q)
    np.testing.assert_array_equal(mu, m0)
    Sref, vn = cr.cov_L(GP.augL, GP.augX, fam, w, sf2, GP.noise, Q)
    cr.assert_cov_close(S, Sref, vn, sf2, GP.noise, what="augmented")
    live = (s0 > 1e-7) & (s0 < 10)
    np.testing.assert_allclose(np.diag(S)[live], s0[live], rtol=1e-10)
    F = GP.sample_posterior(Q, n=3, seed=1)
    assert F.shape == (3, 40) and np.all(np.isfinite(F))


def test_empty_model(lib):
    from ibo_amd.gaussianprocess import GaussianProcess
    from ibo_amd.gaussianprocess.kernel import GaussianKernel_ard
    Q = np.random.RandomState(1).rand(7, 3)
    fam, w, sf2 = gr.kernel_spec("ard", [.3] * 3, 3)
    K = cr.kmat(fam, w, sf2, Q, Q)
    np.fill_diagonal(K, 1.0)
    mu, S = GaussianProcess(GaussianKernel_ard([.3] * 3)).posterior_cov(Q)
    assert np.all(mu == 0)
    np.testing.assert_allclose(S, K, rtol=1e-13, atol=1e-15)
    assert np.all(np.diag(S) == 1)
    pr = make_prior(3)
    mu, S = GaussianProcess(GaussianKernel_ard([.3] * 3), prior=pr).posterior_cov(Q)
    np.testing.assert_allclose(mu, [pr.mu(q) for q in Q], rtol=1e-13)
    np.testing.assert_allclose(S, K, rtol=1e-13, atol=1e-15)
    with pytest.raises(ValueError):
        GaussianProcess(GaussianKernel_ard([.3] * 3)).sample_posterior(Q)


def check_draws(F, S, Z, jitter=0.0, what=""):
    L = np.linalg.cholesky(S + jitter * np.eye(len(S)))
    want = Z @ L.T
    scale = np.abs(Z) @ np.abs(L).T
    err = np.abs(F - want)
    assert np.all(err <= 1e-9 * np.max(scale, axis=1, keepdims=True)), "%s: worst %g" % (what, np.max(err / np.max(scale, axis=1, keepdims=True)))


@pytest.mark.parametrize("M", [1, 17, 129, 1000, 2049, 4160])
def test_draws_against_numpy(lib, M):
    GP, ref = model("ard", 300, 3, seed=4)
    Q = queries(GP.X, M, seed=M)
    Z = np.random.default_rng(M).standard_normal((5, M))
    rc, info, mu, F = sample_call(lib, GP._handle(), Q, Z, guard=True)
    assert rc == lib.OK and info == 0
    assert np.array_equal(mu, GP.posteriors(Q)[0])
    Sref, _ = cr.cov(ref, Q)
    check_draws(F, Sref, Z, what="M=%d" % M)
    rc, info, mu, F2 = sample_call(lib, GP._handle(), Q, Z, jitter=1e-6)
    check_draws(F2, Sref, Z, jitter=1e-6, what="M=%d jitter" % M)


def test_sample_posterior_seeds_and_jitter(lib):
    GP, ref = model("sviso", 150, 3, seed=6)
    Q = queries(GP.X, 300, seed=3)
    a = GP.sample_posterior(Q, n=4, seed=5)
    b = GP.sample_posterior(Q, n=4, seed=5)
    c = GP.sample_posterior(Q, n=4, seed=6)
    assert np.array_equal(a, b) and not np.array_equal(a, c)
    mu, S = GP.posterior_cov(Q)
    Z = np.random.default_rng(5).standard_normal((4, 300))
    check_draws(a - mu, cr.cov(ref, Q)[0], Z, what="sample_posterior")
    # exact duplicates of a candidate make the latent covariance singular: the jitter escalation still draws
    Qd = np.r_[Q[:50], Q[:50]]
    F = GP.sample_posterior(Qd, n=3, seed=1, noise=False)
    assert F.shape == (3, 100) and np.all(np.isfinite(F))


def test_indefinite_sigma_reports_the_pivot(lib):
    # svard of magnitude 2: k = 4 exp(..) off the diagonal, 1 + noise on it (the reference's rule); short length scales keep the
    # model itself positive definite, two near-duplicate candidates far from the data make Sigma indefinite
    hyper = [.01, .01, .01, 2.0]
    GP, ref = model("svard", 40, 3, seed=2, hyper=hyper)
    rs = np.random.RandomState(4)
    Q = np.r_[rs.rand(3, 3) * .2 + 2.0, [[2.5, 2.5, 2.5], [2.5, 2.5, 2.5001]], rs.rand(3, 3) * .2 + 3.0]
    Sref, _ = cr.cov(ref, Q, with_noise=False)
    _, want = dpotrf(Sref, lower=1)
    assert want > 0
    rc, info, _, _ = sample_call(lib, GP._handle(), Q, np.zeros((2, len(Q))), with_noise=0)
    assert rc == lib.ERR_NOT_PD and info == want
    with pytest.raises(np.linalg.LinAlgError):
        GP.sample_posterior(Q, n=2, seed=0, noise=False)


def test_thompson_gallery(lib):
    from ibo_amd.acquisition.gallery import thompsonGallery, MIN_SEPARATION
    GP, _ = model("ard", 15, 3, seed=7)
    C = np.random.RandomState(2).rand(2000, 3) * 1.5 - .25
    g1 = thompsonGallery(GP, C, 6, seed=3)
    g2 = thompsonGallery(GP, C, 6, seed=3)
    assert 1 <= len(g1) <= 6 and len(g1) == len(g2) and all(np.array_equal(a, b) for a, b in zip(g1, g2))
    # the walk restated: each draw's first maximiser joins when it is farther than MIN_SEPARATION from every member
    F = GP.sample_posterior(C, n=48, seed=3)
    arg = [int(np.argmax(f)) for f in F]
    want = []
    for k in arg:
        if len(want) < 6 and all(np.linalg.norm(C[k] - m) > MIN_SEPARATION for m in want):
            want.append(C[k])
    assert len(g1) == len(want) and all(np.array_equal(a, b) for a, b in zip(g1, want))
    for i in range(len(g1)):
        assert any(np.array_equal(g1[i], c) for c in C[arg])
        for j in range(i):
            assert np.linalg.norm(g1[i] - g1[j]) > MIN_SEPARATION
    one = thompsonGallery(GP, C, 1, seed=3)
    assert len(one) == 1 and np.array_equal(one[0], C[arg[0]])
    short = thompsonGallery(GP, C, 50, seed=3, draws=4)
    assert 1 <= len(short) <= 4
    from ibo_amd.gaussianprocess import PrefGaussianProcess
    from ibo_amd.gaussianprocess.kernel import GaussianKernel_ard
    rs = np.random.RandomState(5)
    P = PrefGaussianProcess(GaussianKernel_ard(np.array([.5, .5])))
    X = rs.rand(16, 2)
    P.addPreferences([(X[2 * i], X[2 * i + 1], 0) for i in range(8)])
    g = thompsonGallery(P, rs.rand(500, 2), 3, seed=1)
    assert 1 <= len(g) <= 3


@pytest.mark.parametrize("N", [8193, 16400])
def test_large_models(lib, N):
    GP, ref = model("ard", N, 8, seed=3)
    Q = queries(GP.X, 1024, seed=1)
    _, S = cov_call(lib, GP._handle(), Q)
    idx = np.r_[0:8, 500:508, 1016:1024]
    Sref, vn = cr.cov(ref, Q[idx])
    cr.assert_cov_close(S[np.ix_(idx, idx)], Sref, vn, ref.sf2, ref.noise, what="N=%d" % N)


@pytest.mark.parametrize("M", [8192, 16384])
def test_many_query_points(lib, M):
    GP, ref = model("m3", 300, 3, seed=5)
    Q = queries(GP.X, M, seed=2)
    _, S = cov_call(lib, GP._handle(), Q)
    idx = np.r_[0:8, M // 2:M // 2 + 8, M - 16:M]
    Sref, vn = cr.cov(ref, Q[idx])
    cr.assert_cov_close(S[np.ix_(idx, idx)], Sref, vn, ref.sf2, ref.noise, what="M=%d" % M)
    assert np.array_equal(S[-1], S[:, -1])
    del S
    Z = np.random.default_rng(M).standard_normal((4, M))
    rc, info, _, F = sample_call(lib, GP._handle(), Q, Z)
    assert rc == lib.OK and info == 0
    check_draws(F, cr.cov(ref, Q)[0], Z, what="draws M=%d" % M)


def test_errors_and_limits(lib):
    GP, _ = model("ard", 50, 3)
    h = GP._handle()
    q = lib.f64(np.random.RandomState(0).rand(4, 3)); S = np.empty(16); Z = np.zeros((2, 4)); F = np.empty(8); info = ctypes.c_int(0)
    dp = lib.dp
    assert lib.lib.ibo_posterior_cov(h, 0, dp(q), 1, None, dp(S)) == lib.ERR_ARG
    assert lib.lib.ibo_posterior_cov(h, 4, None, 1, None, dp(S)) == lib.ERR_ARG
    assert lib.lib.ibo_posterior_cov(h, 4, dp(q), 1, None, None) == lib.ERR_ARG
    assert lib.lib.ibo_posterior_cov(None, 4, dp(q), 1, None, dp(S)) == lib.ERR_ARG
    assert lib.lib.ibo_posterior_cov(h, 16385, dp(q), 1, None, dp(S)) == lib.ERR_ARG
    assert b"16384" in lib.lib.ibo_last_error()
    smp = lambda M, Qp, n, Zp, Fp, jit=0.0: lib.lib.ibo_posterior_sample(h, M, Qp, 1, jit, n, Zp, Fp, None, ctypes.byref(info))
    assert smp(0, dp(q), 2, dp(Z), dp(F)) == lib.ERR_ARG
    assert smp(16385, dp(q), 2, dp(Z), dp(F)) == lib.ERR_ARG
    assert b"16384" in lib.lib.ibo_last_error()
    assert smp(4, dp(q), 0, dp(Z), dp(F)) == lib.ERR_ARG
    assert smp(4, dp(q), 4097, dp(Z), dp(F)) == lib.ERR_ARG
    assert b"4096" in lib.lib.ibo_last_error()
    assert smp(4, None, 2, dp(Z), dp(F)) == lib.ERR_ARG
    assert smp(4, dp(q), 2, None, dp(F)) == lib.ERR_ARG
    assert smp(4, dp(q), 2, dp(Z), None) == lib.ERR_ARG
    assert smp(4, dp(q), 2, dp(Z), dp(F), -1.0) == lib.ERR_ARG
    assert smp(4, dp(q), 2, dp(Z), dp(F)) == lib.OK
    hp = ctypes.c_void_p()
    lib.check(lib.lib.ibo_gp_create(0, ctypes.byref(hp)))
    try:
        assert lib.lib.ibo_posterior_cov(hp, 4, dp(q), 1, None, dp(S)) == lib.ERR_STATE
        assert lib.lib.ibo_posterior_sample(hp, 4, dp(q), 1, 0.0, 2, dp(Z), dp(F), None, ctypes.byref(info)) == lib.ERR_STATE
    finally:
        lib.lib.ibo_gp_destroy(hp)
    # guards after the outputs, at sizes that are not multiples of the tiles
    cov_call(lib, h, np.random.RandomState(1).rand(70, 3), guard=True)
    rc, _, _, _ = sample_call(lib, h, np.random.RandomState(1).rand(70, 3), np.ones((3, 70)), guard=True)
    assert rc == lib.OK

"""
ibo_acq_grad_batch and what is built on it: GaussianProcess.posterior_gradient, EI / PI / UCB .gradient / .negf_grad and
maximizeEI / PI / UCB(polish=True).

The yardstick is tests/grad_reference.py, the formulas restated in NumPy/SciPy float64 (R with the diagonal 1 + noise,
cho_solve for the alphas and u = R^-1 k*) and pinned to the oracle by tests/test_grad_reference.py.  Tolerance: |err_d| <=
1e-9 sum_i |dk*_i c_i| + 1e-13 per entry, on models with cond(R) far below 1e8 (noise 0.1; tests/test_gpu_conditioning.py
holds the same gradients to long-double truth at cond(R) 1e6 .. 1e8).  Central differences of
ibo_acq_batch catch what a restatement sharing a mistake would miss (sign, scale, the k* variance).
"""
import ctypes

import numpy as np
import pytest

import grad_reference as gr
from conftest import synth

pytestmark = pytest.mark.gpu

KERNELS = {"ard": None, "iso": [.45], "svard": None, "sviso": [.45, .8], "m3": [.5, .95], "m5": [.5, .9]}


@pytest.fixture(scope="module")
def lib():
    from ibo_amd import _lib
    if _lib.device_count() < 1:
        pytest.fail("no GPU visible: the product has no CPU fallback")
    return _lib


def hyper_of(kind, D):
    ell = np.linspace(.35, .6, D) * max(1.0, np.sqrt(D) / 2)
    if kind == "ard":
        return list(ell)
    if kind == "svard":
        return list(ell) + [.9]
    return [h * (max(1.0, np.sqrt(D) / 2) if i == 0 else 1.0) for i, h in enumerate(KERNELS[kind])]


def make_kernel(kind, hyper):
    from ibo_amd.gaussianprocess import kernel as K
    return {"ard": K.GaussianKernel_ard, "iso": K.GaussianKernel_iso, "svard": K.SVGaussianKernel_ard,
            "sviso": K.SVGaussianKernel_iso, "m3": K.MaternKernel3, "m5": K.MaternKernel5}[kind](np.array(hyper, dtype=float))


def make_prior(D, seed=11):
    from ibo_amd.gaussianprocess.prior import RBFNMeanPrior
    rs = np.random.RandomState(seed)
    p = RBFNMeanPrior()
    p.means = rs.rand(5, D); p.beta = rs.randn(5); p.theta = 1.5; p.lowerb = np.zeros(D) - .1; p.width = np.full(D, 1.2)
    return p, (p.means, p.beta, p.theta, p.lowerb, p.width)


def model(kind, N, D, seed=1, noise=.1, prior=False):
    from ibo_amd.gaussianprocess import GaussianProcess
    X, Y = synth(seed, N, D)
    hyper = hyper_of(kind, D)
    pr, prt = make_prior(D) if prior else (None, None)
    GP = GaussianProcess(make_kernel(kind, hyper), X, Y, prior=pr, noise=noise)
    fam, w, sf2 = gr.kernel_spec(kind, hyper, D)
    return GP, gr.RefGP(X, Y, noise, fam, w, sf2, prior=prt)


def grad_call(lib, h, Q, acq=3, parm=0.0, erf=1, clamp=1e-7, ymax=float("nan"), want="all", guard=False):
    Q = lib.f64(np.atleast_2d(Q))
    M, D = Q.shape
    pad = 8 if guard else 0
    bufs = {k: np.full((M + pad) * (1 if k in ("mu", "s2", "acq") else D), 7.25) for k in ("mu", "s2", "acq", "dmu", "ds2", "dacq")}
    names = ("mu", "s2", "acq", "dmu", "ds2", "dacq") if want == "all" else want
    if acq == 3 and "dacq" in names:
        names = tuple(n for n in names if n != "dacq")
    p = lambda k: lib.dp(bufs[k]) if k in names else None
    lib.check(lib.lib.ibo_acq_grad_batch(h, M, lib.dp(Q), acq, float(parm), erf, clamp, ymax,
                                         p("mu"), p("s2"), p("acq"), p("dmu"), p("ds2"), p("dacq")))
    out = {}
    for k in names:
        n = M if k in ("mu", "s2", "acq") else M * D
        if guard:
            assert np.all(bufs[k][n:] == 7.25), "%s: guard overwritten" % k
        out[k] = bufs[k][:n] if k in ("mu", "s2", "acq") else bufs[k][:n].reshape(M, D)
    return out


def check_against_ref(got, ref, what=""):
    gr.assert_grad_close(got["dmu"], ref["dmu"], ref["smu"], what=what + " dmu")
    gr.assert_grad_close(got["ds2"], ref["ds2"], ref["ss2"], what=what + " ds2")
    np.testing.assert_allclose(got["mu"], ref["mu"], rtol=1e-9, atol=1e-12)
    np.testing.assert_allclose(got["s2"], ref["s2"], rtol=1e-9, atol=1e-12)


def queries(X, M, seed=2):
    rs = np.random.RandomState(seed)
    Q = rs.rand(M, X.shape[1]) * 1.2 - .1
    k = min(M // 4, len(X))
    if k >= 2:                           # on top of training inputs, the first and the last row among them
        Q[:k] = X[np.r_[0, len(X) - 1, rs.randint(0, len(X), k - 2)]]
    elif k == 1:
        Q[0] = X[-1]
    return Q


def rows_to_check(M, n=48):
    if M <= n:
        return np.arange(M)
    rs = np.random.RandomState(M)
    return np.unique(np.r_[0, M - 1, rs.randint(0, M, n - 2)])


# kernel, N, D, M: every route (<= 16 points in 16-wide tiles, more in 64-wide ones, chunks beyond 16384 points, split-K ranges
# from one row block to many) and the tile edges (N = 63 / 64 / 65, M = 16 / 17, 64 / 65)
CASES = [("ard", 1, 1, 1), ("ard", 2, 2, 2), ("iso", 63, 4, 16), ("svard", 64, 8, 17), ("sviso", 65, 33, 33),
         ("m3", 300, 2, 1000), ("m5", 1024, 4, 65), ("ard", 2048, 64, 16), ("m3", 4097, 8, 8193), ("ard", 300, 4, 70000),
         ("m5", 2048, 8, 1), ("iso", 1024, 1, 1000), ("svard", 4097, 4, 2)]


@pytest.mark.parametrize("kind,N,D,M", CASES)
def test_posterior_gradient_matches_numpy(lib, kind, N, D, M):
    GP, ref = model(kind, N, D)
    Q = queries(GP.X, M)
    got = grad_call(lib, GP._handle(), Q)
    rows = rows_to_check(M)
    r = ref.grad(Q[rows])
    check_against_ref({k: v[rows] for k, v in got.items()}, r, "%s N=%d D=%d M=%d" % (kind, N, D, M))
    mu, s2 = np.empty(M), np.empty(M)
    lib.check(lib.lib.ibo_acq_batch(GP._handle(), M, lib.dp(lib.f64(Q)), 3, 0.0, 1, 1e-7, float("nan"), lib.dp(mu), lib.dp(s2), None))
    assert np.array_equal(mu, got["mu"]) and np.array_equal(s2, got["s2"])


@pytest.mark.parametrize("kind", ["ard", "m3", "m5"])
def test_prior_enters_the_mean_gradient(lib, kind):
    GP, ref = model(kind, 200, 3, prior=True)
    Q = queries(GP.X, 40)
    GP._push_prior()
    got = grad_call(lib, GP._handle(), Q)
    r = ref.grad(Q)
    check_against_ref(got, r, kind + " prior")
    _, ref0 = model(kind, 200, 3, prior=False)
    assert np.max(np.abs(ref0.grad(Q)["dmu"] - r["dmu"])) > 1e-3      # the prior's terms are not negligible here


@pytest.mark.parametrize("clamp", [1e-7, 1e-8])
@pytest.mark.parametrize("erf", [0, 1])
@pytest.mark.parametrize("acq", [0, 1, 2])
def test_acquisition_gradients(lib, acq, erf, clamp):
    GP, ref = model("ard", 300, 3, prior=True)
    Q = queries(GP.X, 64)
    parm = .8 if acq == 2 else .01
    GP._push_prior()
    got = grad_call(lib, GP._handle(), Q, acq=acq, parm=parm, erf=erf, clamp=clamp)
    vals = np.empty(64)
    lib.check(lib.lib.ibo_acq_batch(GP._handle(), 64, lib.dp(lib.f64(Q)), acq, parm, erf, clamp, float("nan"), None, None, lib.dp(vals)))
    np.testing.assert_allclose(got["acq"], vals, rtol=1e-12, atol=0)
    r = ref.grad(Q, clamp_lo=clamp, acq=acq, parm=parm, erf_mode=erf)
    gr.assert_grad_close(got["dacq"], r["dacq"], r["sacq"], what="dacq")


@pytest.mark.parametrize("erf", [0, 1])
@pytest.mark.parametrize("acq", [0, 1, 2])
@pytest.mark.parametrize("kind", ["ard", "m5"])
def test_gradients_match_differences_of_acq_batch(lib, kind, acq, erf):
    GP, _ = model(kind, 300, 4, prior=True)
    GP._push_prior()
    h = GP._handle()
    lib.check(lib.lib.ibo_gp_set_kstar_sf2(h, 0.85))          # a k* variance other than the fit's
    try:
        Q = np.random.RandomState(9).rand(24, 4) * .8 + .1
        parm = .8 if acq == 2 else .01
        got = grad_call(lib, h, Q, acq=acq, parm=parm, erf=erf, clamp=1e-8)

        def f(P):
            v = np.empty(len(P))
            lib.check(lib.lib.ibo_acq_batch(h, len(P), lib.dp(lib.f64(P)), acq, parm, erf, 1e-8, float("nan"), None, None, lib.dp(v)))
            return v
        step = 1e-5
        G = np.zeros(Q.shape)
        for d in range(4):
            E = np.zeros(Q.shape); E[:, d] = step
            G[:, d] = (f(Q + E) - f(Q - E)) / (2 * step)
        rt = 1e-5 if erf == 0 else 1e-4
        floor = 1e-6 * np.max(np.linalg.norm(got["dacq"], axis=1))
        assert np.all(np.abs(got["dacq"] - G) <= rt * np.abs(G) + floor), np.max(np.abs(got["dacq"] - G))
    finally:
        lib.check(lib.lib.ibo_gp_set_kstar_sf2(h, 1.0))


def test_clip_gives_exactly_zero(lib):
    GP, _ = model("ard", 50, 2, noise=1e-9)          # raw sigma^2 at the inputs: between noise and 2 noise, below 1e-8
    got = grad_call(lib, GP._handle(), GP.X[:10], acq=2, parm=.5, clamp=1e-8)
    assert np.all(got["s2"] == 1e-8) and np.all(got["ds2"] == 0.0)
    assert np.array_equal(got["dacq"], got["dmu"])
    GP, _ = model("ard", 50, 2, noise=10.0)          # far from the data: 1 + 10 clipped to 10
    got = grad_call(lib, GP._handle(), np.full((3, 2), 30.0), acq=2, parm=.5)
    assert np.all(got["s2"] == 10.0) and np.all(got["ds2"] == 0.0)
    assert np.array_equal(got["dacq"], got["dmu"])


def test_lifecycle_state_errors_guards_and_bits(lib):
    from ibo_amd.gaussianprocess import GaussianProcess
    GP, ref = model("ard", 120, 3)
    h = GP._handle()
    Q = queries(GP.X, 20)
    a = grad_call(lib, h, Q, acq=0, parm=.01, guard=True)
    b = grad_call(lib, h, Q, acq=0, parm=.01, guard=True)
    for k in a:
        assert np.array_equal(a[k], b[k]), k
    big = queries(GP.X, 3000, seed=5)
    a = grad_call(lib, h, big, acq=1, parm=.01, guard=True)
    b = grad_call(lib, h, big, acq=1, parm=.01, guard=True)
    for k in a:
        assert np.array_equal(a[k], b[k]), k
    # extension by one row (ibo_gp_extend), then a refit
    rs = np.random.RandomState(4)
    x1 = rs.rand(1, 3); y1 = np.sin(3 * x1.sum(1))
    GP.addData(x1, y1)
    fam, w, sf2 = gr.kernel_spec("ard", hyper_of("ard", 3), 3)
    ref = gr.RefGP(GP.X, GP.Y, .1, fam, w, sf2)
    check_against_ref(grad_call(lib, GP._handle(), Q), ref.grad(Q), "extended")
    X2 = rs.rand(40, 3)
    GP.addData(X2, np.sin(3 * X2.sum(1)))
    ref = gr.RefGP(GP.X, GP.Y, .1, fam, w, sf2)
    check_against_ref(grad_call(lib, GP._handle(), Q), ref.grad(Q), "refit")
    lib.check(lib.lib.ibo_gp_set_kstar_sf2(GP._handle(), 0.6))
    try:
        check_against_ref(grad_call(lib, GP._handle(), Q), ref.grad(Q, sf2k=0.6), "k* variance")
    finally:
        lib.check(lib.lib.ibo_gp_set_kstar_sf2(GP._handle(), 1.0))
    # errors
    hp = ctypes.c_void_p()
    lib.check(lib.lib.ibo_gp_create(0, ctypes.byref(hp)))
    try:
        o = np.empty(3)
        q = lib.f64(np.zeros((1, 3)))
        assert lib.lib.ibo_acq_grad_batch(hp, 1, lib.dp(q), 3, 0.0, 1, 1e-7, 0.0, lib.dp(o), None, None, None, None, None) == lib.ERR_STATE
    finally:
        lib.lib.ibo_gp_destroy(hp)
    h = GP._handle()
    q = lib.f64(np.zeros((2, 3))); o = np.empty(6); v = np.empty(2)
    call = lambda M, Qp, acq, erf, *outs: lib.lib.ibo_acq_grad_batch(h, M, Qp, acq, 0.01, erf, 1e-7, 0.0, *outs)
    assert call(0, lib.dp(q), 0, 1, lib.dp(v), None, None, None, None, None) == lib.ERR_ARG
    assert call(2, None, 0, 1, lib.dp(v), None, None, None, None, None) == lib.ERR_ARG
    assert call(2, lib.dp(q), 4, 1, lib.dp(v), None, None, None, None, None) == lib.ERR_ARG
    assert call(2, lib.dp(q), 0, 2, lib.dp(v), None, None, None, None, None) == lib.ERR_ARG
    assert call(2, lib.dp(q), 0, 1, None, None, None, None, None, None) == lib.ERR_ARG
    assert call(2, lib.dp(q), 3, 1, None, None, None, None, None, lib.dp(o)) == lib.ERR_ARG
    assert call(2, lib.dp(q), 0, 1, None, None, None, None, None, lib.dp(o)) == lib.OK


def fd_posteriors(GP, Q, step=1e-5):
    G1, G2 = np.zeros(Q.shape), np.zeros(Q.shape)
    for d in range(Q.shape[1]):
        E = np.zeros(Q.shape); E[:, d] = step
        mp, sp = GP.posteriors(Q + E); mm, sm = GP.posteriors(Q - E)
        G1[:, d] = (mp - mm) / (2 * step); G2[:, d] = (sp - sm) / (2 * step)
    return G1, G2


def test_preference_gp_and_augmented_variance(lib):
    from ibo_amd.gaussianprocess import PrefGaussianProcess
    from ibo_amd.gaussianprocess.kernel import GaussianKernel_ard
    rs = np.random.RandomState(3)
    GP = PrefGaussianProcess(GaussianKernel_ard(np.array([.4, .4])))
    P = rs.rand(12, 2)
    GP.addPreferences([(P[2 * i], P[2 * i + 1], 0) for i in range(6)])
    Q = rs.rand(10, 2) * .8 + .1
    for stage in ("prefs", "augmented"):
        mu, s2, dmu, ds2 = GP.posterior_gradient(Q)
        m0, v0 = GP.posteriors(Q)
        np.testing.assert_array_equal(mu, m0)
        np.testing.assert_array_equal(s2, v0)
        G1, G2 = fd_posteriors(GP, Q)
        np.testing.assert_allclose(dmu, G1, rtol=1e-5, atol=1e-6 * np.max(np.abs(G1)))
        np.testing.assert_allclose(ds2, G2, rtol=1e-5, atol=1e-6 * np.max(np.abs(G2)))
        GP.addObservationPoint(rs.rand(2))
    from ibo_amd.acquisition import EI
    ei = EI(GP)
    v, g = ei.gradient(Q)
    np.testing.assert_array_equal(v, [-ei.negf(q) for q in Q])
    nv, ng = ei.negf_grad(Q[0])
    assert nv == -v[0] and np.array_equal(ng, -g[0])


def test_empty_model(lib):
    from ibo_amd.gaussianprocess import GaussianProcess
    from ibo_amd.gaussianprocess.kernel import GaussianKernel_ard
    Q = np.random.RandomState(1).rand(5, 3)
    mu, s2, dmu, ds2 = GaussianProcess(GaussianKernel_ard([.3] * 3)).posterior_gradient(Q)
    assert np.all(mu == 0) and np.all(s2 == 1) and np.all(dmu == 0) and np.all(ds2 == 0)
    pr, prt = make_prior(3)
    mu, s2, dmu, ds2 = GaussianProcess(GaussianKernel_ard([.3] * 3), prior=pr).posterior_gradient(Q)
    for j, q in enumerate(Q):
        m, dm = gr.prior_grad(prt, q)
        np.testing.assert_allclose(mu[j], pr.mu(q), rtol=1e-13)
        np.testing.assert_allclose(dmu[j], dm, rtol=1e-12, atol=1e-15)
    assert np.all(s2 == 1) and np.all(ds2 == 0)
    m1, s1, d1, e1 = GaussianProcess(GaussianKernel_ard([.3] * 3), prior=pr).posterior_gradient(Q[0])
    assert np.shape(d1) == (3,) and m1 == mu[0]


def test_large_models(lib):
    GP, ref = model("ard", 8193, 8)
    Q = queries(GP.X, 6)
    check_against_ref(grad_call(lib, GP._handle(), Q), ref.grad(Q), "N=8193")
    del GP, ref
    # past the MFMA sweep's 16320 rows: the call works (checked against differences of ibo_acq_batch)
    GP, _ = model("ard", 16400, 4)
    h = GP._handle()
    Q = np.random.RandomState(2).rand(3, 4)
    got = grad_call(lib, h, Q)

    def mu(P):
        v = np.empty(len(P))
        lib.check(lib.lib.ibo_acq_batch(h, len(P), lib.dp(lib.f64(P)), 3, 0.0, 1, 1e-7, float("nan"), lib.dp(v), None, None))
        return v
    for d in range(4):
        E = np.zeros(Q.shape); E[:, d] = 1e-5
        G = (mu(Q + E) - mu(Q - E)) / 2e-5
        np.testing.assert_allclose(got["dmu"][:, d], G, rtol=1e-5, atol=1e-6 * np.max(np.abs(got["dmu"])))


def c2_model():
    from ibo_amd.gaussianprocess import GaussianProcess
    from ibo_amd.gaussianprocess.kernel import GaussianKernel_ard
    X, Y = synth(12, 1024, 4)
    return GaussianProcess(GaussianKernel_ard(np.array([.3, .35, .4, .45])), X, Y, noise=.1)


def one_d_model():
    from ibo_amd.gaussianprocess import GaussianProcess
    from ibo_amd.gaussianprocess.kernel import GaussianKernel_ard
    X = np.array([[.1], [.3], [.45], [.8]]); Y = np.array([.2, .9, .5, -.3])
    return GaussianProcess(GaussianKernel_ard(np.array([.15])), X, Y, noise=.1)


@pytest.mark.parametrize("which", ["c2", "1d"])
@pytest.mark.parametrize("acqfunc", ["ei", "pi", "ucb"])
def test_polish(lib, which, acqfunc):
    from ibo_amd import acquisition as A
    GP = c2_model() if which == "c2" else one_d_model()
    D = GP.X.shape[1]
    bounds = [[0., 1.]] * D
    fn = {"ei": A.maximizeEI, "pi": A.maximizePI, "ucb": A.maximizeUCB}[acqfunc]
    o0, x0 = fn(GP, bounds)
    o1, x1 = fn(GP, bounds, polish=False)
    assert o0 == o1 and np.array_equal(x0, x1)
    op, xp = fn(GP, bounds, polish=True)
    assert np.all(xp >= 0.0) and np.all(xp <= 1.0)
    assert op >= o0
    code = A._ACQ[acqfunc]
    parm = A._ucb_parm(GP, bounds, .1, .2) if acqfunc == "ucb" else .01
    h = GP._handle()
    _, _, sf2_py, sf2_native = GP.kernel._ibo_spec()
    lib.check(lib.lib.ibo_gp_set_kstar_sf2(h, sf2_native))
    try:
        v, g = np.empty(1), np.empty((1, D))
        lib.check(lib.lib.ibo_acq_batch(h, 1, lib.dp(lib.f64(xp.reshape(1, D))), code, parm, 0, 1e-8, float("nan"), None, None, lib.dp(v)))
        np.testing.assert_allclose(op, v[0], rtol=1e-12)
        if op > o0 and np.all((xp > 1e-6) & (xp < 1 - 1e-6)):          # a smooth interior maximum: the gradient vanishes there
            lib.check(lib.lib.ibo_acq_grad_batch(h, 1, lib.dp(lib.f64(xp.reshape(1, D))), code, parm, 0, 1e-8, float("nan"),
                                                 None, None, None, None, None, lib.dp(g)))
            R = np.random.RandomState(0).rand(64, D)
            gs = np.empty((64, D))
            lib.check(lib.lib.ibo_acq_grad_batch(h, 64, lib.dp(lib.f64(R)), code, parm, 0, 1e-8, float("nan"),
                                                 None, None, None, None, None, lib.dp(gs)))
            assert np.linalg.norm(g) <= 1e-6 * np.median(np.linalg.norm(gs, axis=1)), (np.linalg.norm(g), np.median(np.linalg.norm(gs, axis=1)))
    finally:
        lib.check(lib.lib.ibo_gp_set_kstar_sf2(h, sf2_py))

"""
ibo_ggp_nlml_grad -- the marginal likelihood of a GP observed with gradients and its gradient with respect to the log hyper-parameters,
the log noise and the log gradient noises -- and what is built on it: trainhyper.gradientLikelihood / ngnlml / dgnlml,
GaussianProcess(G=).nlml() and .learn().

The yardstick is tests/gradobs_nlml_reference.py (pinned by tests/test_gradobs_nlml_reference.py): long double up to 400 rows and
wherever cond_2 > 1e6, float64 otherwise (the 2100-row case: float64 under cond_upper <= 1e6).  Bars, the project's rule:
    value      |v - value| <= 1e-15 max(cond_2, 1e6) V,    V   = |t.alpha / 2| + sum |log L_ii| + P log(2 pi) / 2
    component  |g - grad_h| <= 1e-15 max(cond_2, 1e6) G_h, G_h = sum |B_ab dA_ab| / 2 + sum |alpha_a dA_ab alpha_b| / 2
    noise      the same with the component's own terms
Bits: the value without a gradient, a second call, a component alone / in the full list / in a permuted list; ibo_nlml_grad and
ibo_loo_grad before and after; a model fitted at the learned theta.
"""
import ctypes
import functools

import numpy as np
import pytest

import gradobs_reference as gr
import gradobs_nlml_reference as gn

pytestmark = pytest.mark.gpu
GUARD = 7.25


@pytest.fixture(scope="module")
def lib():
    from ibo_amd import _lib
    if _lib.device_count() < 1:
        pytest.fail("no GPU visible: the product has no CPU fallback")
    return _lib


def call(c, spec, grad=True, gnoise_grad=True, noise=None, gnoise=None, N=None, hyper=None):
    """ibo_ggp_nlml_grad on a case through the raw ABI: (rc, value, grad, noise terms); guards behind every output"""
    from ibo_amd import _lib as L
    kern = c["kern"]
    X, Y, G = L.f64(c["X"]), L.f64(c["Y"]), L.f64(c["G"])
    N = len(X) if N is None else N
    D = X.shape[1]
    hyper = L.f64(kern.theta if hyper is None else hyper)
    gno = L.f64(gr.tile_gnoise(c["gnoise"] if gnoise is None else gnoise, D))
    n = len(spec)
    modes = (ctypes.c_int * max(n, 1))(*[m for m, _ in spec])
    dims = (ctypes.c_int * max(n, 1))(*[d for _, d in spec])
    v = np.full(1 + 8, GUARD); g = np.full(n + 8, GUARD); gz = np.full(D + 1 + 8, GUARD)
    rc = L.lib.ibo_ggp_nlml_grad(L.default_device(), kern.ktype, N, D, L.dp(X), L.dp(Y), L.dp(G), L.dp(hyper), len(hyper), kern.sf2_py,
                                 float(c["noise"] if noise is None else noise), L.dp(gno), n, modes, dims, L.dp(v),
                                 L.dp(g) if grad else None, L.dp(gz) if gnoise_grad else None)
    assert np.all(v[1:] == GUARD) and np.all(g[n:] == GUARD) and np.all(gz[D + 1:] == GUARD), "a guard behind an output was overwritten"
    if rc != L.OK:
        assert v[0] == GUARD and np.all(g == GUARD) and np.all(gz == GUARD), "an error return wrote to an output"
    if not grad:
        assert np.all(g == GUARD)
    if not gnoise_grad:
        assert np.all(gz == GUARD)
    return rc, v[0], g[:n].copy(), gz[:D + 1].copy()


@functools.lru_cache(maxsize=None)
def device_result(name):
    """(value, grad, noise terms) of a case with its kernel's own spec: computed once, read by the tests that compare bits"""
    from ibo_amd import _lib as L
    c = gn.case(name)
    rc, v, g, gz = call(c, gn.spec_of(c["kern"]))
    assert rc == L.OK, L.lib.ibo_last_error()
    return v, g, gz


@pytest.mark.parametrize("name", gn.DEVICE_CASES)
def test_value_and_every_component_within_the_bars(lib, name):
    c = gn.case(name)
    spec = gn.spec_of(c["kern"])
    ref = gn.reference(name)
    v, g, gz = device_result(name)
    rv, rg, rn = gn.shares(v, g, gz, ref)
    print("%s: P = %d, cond %.3g, shares of the bar: value %.3g, hyper %.3g, noise %.3g" % (name, ref["P"], ref["cond"], rv, np.max(rg), np.max(rn)))
    assert rv <= 1.0, (v, ref["value"])
    assert np.all(rg <= 1.0), (g, ref["grad"], rg)
    assert np.all(rn <= 1.0), (gz, ref["gnoise"], rn)
    # the value alone, the value with the noise terms alone, a second call: the same bits
    rc, v0, _, _ = call(c, spec, grad=False, gnoise_grad=False)
    assert rc == lib.OK and v0 == v
    rc, v1, _, gz1 = call(c, [], grad=False)
    assert rc == lib.OK and v1 == v and np.array_equal(gz1, gz)
    rc, v2, g2, gz2 = call(c, spec)
    assert rc == lib.OK and v2 == v and np.array_equal(g2, g) and np.array_equal(gz2, gz)


@pytest.mark.parametrize("name", ["sviso_20x2", "m3_21x2", "m5_43x2", "ard_33x3", "svard_3x64"])
def test_a_component_has_the_same_bits_in_every_list(lib, name):
    c = gn.case(name)
    spec = gn.spec_of(c["kern"])
    v, g, gz = device_result(name)
    perm = list(np.random.RandomState(3).permutation(len(spec)))
    rc, vp, gp, gzp = call(c, [spec[i] for i in perm])
    assert rc == lib.OK and vp == v and np.array_equal(gp, g[perm]) and np.array_equal(gzp, gz)
    for h in sorted(set([0, len(spec) // 2, len(spec) - 1])):
        rc, v1, g1, _ = call(c, [spec[h]], gnoise_grad=False)
        assert rc == lib.OK and v1 == v and g1[0] == g[h], (h, g1[0], g[h])
    rc, _, gd, _ = call(c, [spec[0], spec[-1], spec[0]], gnoise_grad=False)
    assert rc == lib.OK and gd[0] == g[0] and gd[1] == g[-1] and gd[2] == g[0]


@pytest.mark.parametrize("name", ["se_1x1", "ard_16x3", "ard_17x3", "ard_13x4", "ard_205x4"])
def test_unit_signal_variance_value_is_the_fitted_models(lib, name):
    """sf2 = 1: A_nl is ibo_ggp_fit's matrix, so the value is t.alpha / 2 + sum log L_ii + const with the fitted handle's own factor"""
    import scipy.linalg as sl
    from test_gpu_gradobs import Handle
    c = gn.case(name)
    assert c["kern"].sf2_py == 1.0
    h = Handle(c["kern"], c["X"], c["Y"], c["G"], c["noise"], c["gnoise"])
    L = np.tril(h.matrix("L"))
    h.close()
    t = gr.targets(c["Y"], c["G"])
    w = sl.solve_triangular(L, t, lower=True)
    logs = np.log(np.diag(L))
    const = len(t) * gn.HALF_LOG_2PI
    value, V = 0.5 * (w @ w) + logs.sum() + const, 0.5 * (w @ w) + np.abs(logs).sum() + const
    v, _, _ = device_result(name)
    assert abs(v - value) <= 1e-12 * V, (v, value)


def test_plain_entries_return_their_earlier_bits(lib):
    """ibo_nlml_grad and ibo_loo_grad on the same X before and after ibo_ggp_nlml_grad: the resident copies they compare by content are theirs"""
    c = gn.case("ard_33x3")
    kern = c["kern"]
    X, Y = lib.f64(c["X"]), lib.f64(c["Y"])
    N, D = X.shape
    hyper = lib.f64(kern.theta)
    modes = (ctypes.c_int * D)(*([0] * D)); dims = (ctypes.c_int * D)(*range(D))

    def plain():
        v = ctypes.c_double(); g = np.empty(D); vl = ctypes.c_double(); gl = np.empty(D); mu = np.empty(N); s2 = np.empty(N)
        lib.check(lib.lib.ibo_nlml_grad(lib.default_device(), kern.ktype, N, D, lib.dp(X), lib.dp(Y), lib.dp(hyper), D, 1.0, 0.05, D, modes, dims,
                                        ctypes.byref(v), lib.dp(g)))
        lib.check(lib.lib.ibo_loo_grad(lib.default_device(), kern.ktype, N, D, lib.dp(X), lib.dp(Y), lib.dp(hyper), D, 1.0, 0.05, D, modes, dims,
                                       ctypes.byref(vl), lib.dp(gl), lib.dp(mu), lib.dp(s2)))
        return v.value, g, vl.value, gl, mu, s2

    before = plain()
    rc, v, g, gz = call(c, gn.spec_of(kern))
    assert rc == lib.OK
    after = plain()
    for a, b in zip(before, after):
        assert np.array_equal(a, b)
    # ... and the other way round, with other targets on the same X in between
    c2 = dict(c, Y=np.asarray(c["Y"]) * 0.5)
    assert call(c2, gn.spec_of(kern))[0] == lib.OK
    rc, v3, g3, gz3 = call(c, gn.spec_of(kern))
    assert rc == lib.OK and v3 == v and np.array_equal(g3, g) and np.array_equal(gz3, gz)
    assert (v, ) == (device_result("ard_33x3")[0], )


def test_workspace_shrinks_fails_and_is_trimmed(lib):
    """1025 rows, then 63, then a matrix that does not factor, then 65 rows, then ibo_trim and 65 rows again: every result is the case's own"""
    def same(name):
        c = gn.case(name)
        rc, v, g, gz = call(c, gn.spec_of(c["kern"]))
        v0, g0, gz0 = device_result(name)
        assert rc == lib.OK and v == v0 and np.array_equal(g, g0) and np.array_equal(gz, gz0), name

    for name in ("ard_205x4", "m3_21x2", "ard_13x4"):
        device_result(name)
    same("ard_205x4")
    same("m3_21x2")
    twin = gn.case("m3_10x2_twin")
    rc, _, _, _ = call(twin, gn.spec_of(twin["kern"]), noise=0.0, gnoise=0.0)
    assert rc == lib.ERR_NOT_PD
    same("ard_13x4")
    lib.trim()
    same("ard_13x4")
    same("m3_21x2")


def test_coincident_points_without_noise_are_not_positive_definite(lib):
    twin = gn.case("m3_10x2_twin")
    spec = gn.spec_of(twin["kern"])
    for kw in (dict(), dict(grad=False), dict(grad=False, gnoise_grad=False)):
        rc, _, _, _ = call(twin, spec, noise=0.0, gnoise=0.0, **kw)        # (call asserts that no output was written)
        assert rc == lib.ERR_NOT_PD and b"positive definite" in lib.lib.ibo_last_error()
    from ibo_amd.gaussianprocess import trainhyper
    from ibo_amd.gaussianprocess.kernel import MaternKernel3
    with pytest.raises(np.linalg.LinAlgError):
        trainhyper.gradientLikelihood(MaternKernel3(twin["kern"].hyper), twin["X"], twin["Y"], twin["G"], 2, noise=0.0, gnoise=0.0)
    rc, v, _, _ = call(twin, spec)
    assert rc == lib.OK and v == device_result("m3_10x2_twin")[0]


def test_limits(lib):
    from oracle import oracle as orc
    X = gr.points(1639, 4, 1)                                    # 8195 rows > IBO_GGP_MAX_ROWS
    Y, G = gr.objective(X)
    big = dict(kern=orc.Kern("ard", [0.6, 0.8, 0.7, 0.9]), X=X, Y=Y, G=G, noise=0.1, gnoise=1e-4)
    assert call(big, [(0, 0)])[0] == lib.ERR_ARG
    X = gr.points(2, 65, 1)
    Y, G = gr.objective(X)
    wide = dict(kern=orc.Kern("iso", [4.0]), X=X, Y=Y, G=G, noise=0.1, gnoise=1e-4)
    assert call(wide, [(1, 0)])[0] == lib.ERR_ARG                # D = 65
    c = gn.case("svard_3x64")
    spec = gn.spec_of(c["kern"])
    assert len(spec) == 65
    assert call(c, spec + [(2, 0)])[0] == lib.ERR_ARG            # ngrad = 66
    assert call(c, spec + [(2, 0)], grad=False)[0] == lib.OK     # (value only: ngrad is not looked at)
    small = gn.case("iso_2x1")
    assert call(small, [(5, 0)])[0] == lib.ERR_ARG and call(small, [(0, 1)])[0] == lib.ERR_ARG and call(small, [(1, 0)], N=0)[0] == lib.ERR_ARG
    v = ctypes.c_double()
    Xs, Ys, Gs = lib.f64(small["X"]), lib.f64(small["Y"]), lib.f64(small["G"])
    hy = lib.f64([0.5]); gno = lib.f64([1e-4])
    assert lib.lib.ibo_ggp_nlml_grad(lib.default_device(), 1, 2, 1, lib.dp(Xs), lib.dp(Ys), None, lib.dp(hy), 1, 1.0, 0.1, lib.dp(gno), 0, None, None,
                                     ctypes.byref(v), None, None) == lib.ERR_ARG
    assert lib.lib.ibo_ggp_nlml_grad(lib.default_device(), 1, 2, 1, lib.dp(Xs), lib.dp(Ys), lib.dp(Gs), lib.dp(hy), 1, 1.0, 0.1, lib.dp(gno), 1, None, None,
                                     ctypes.byref(v), lib.dp(np.empty(1)), None) == lib.ERR_ARG


def _kernel_object(kern):
    from ibo_amd.gaussianprocess.kernel import (GaussianKernel_ard, GaussianKernel_iso, MaternKernel3, MaternKernel5, SVGaussianKernel_ard,
                                                SVGaussianKernel_iso)
    return {"ard": GaussianKernel_ard, "iso": GaussianKernel_iso, "m3": MaternKernel3, "m5": MaternKernel5, "svard": SVGaussianKernel_ard,
            "sviso": SVGaussianKernel_iso}[kern.kind]


@pytest.mark.parametrize("name", ["ard_13x4", "sviso_20x2", "m5_43x2", "ard_60x3_gn"])
def test_python_entries_return_the_abis_numbers(lib, name):
    from ibo_amd.gaussianprocess import GaussianProcess, trainhyper
    c = gn.case(name)
    cls = _kernel_object(c["kern"])
    k = cls(c["kern"].hyper)
    v, g, gz = device_result(name)
    n = len(g)
    out = trainhyper.gradientLikelihood(k, c["X"], c["Y"], c["G"], n, noise=c["noise"], gnoise=c["gnoise"], gradNoise=True)
    assert out[0] == v and np.array_equal(out[1], g) and out[2] == gz[0] and np.array_equal(out[3], gz[1:])
    v1, g1 = trainhyper.gradientLikelihood(k, c["X"], c["Y"], c["G"], 1, noise=c["noise"], gnoise=c["gnoise"])
    assert v1 == v and g1[0] == g[0]
    assert trainhyper.gradientLikelihood(k, c["X"], c["Y"], c["G"], n, noise=c["noise"], gnoise=c["gnoise"], computeGradient=False) == v
    lh = np.log(c["kern"].hyper)
    assert trainhyper.ngnlml(lh, cls, c["X"], c["Y"], c["G"], c["noise"], c["gnoise"]) == v
    assert np.array_equal(trainhyper.dgnlml(lh, cls, c["X"], c["Y"], c["G"], c["noise"], c["gnoise"]), g)
    X2 = np.array(c["X"]); X2[0, 0] += 0.01                      # (memoised by content: other data, another value)
    assert trainhyper.ngnlml(lh, cls, X2, c["Y"], c["G"], c["noise"], c["gnoise"]) != v
    if c["kern"].sf2_py == 1.0:
        model = GaussianProcess(k, c["X"], c["Y"], G=c["G"], noise=c["noise"], gnoise=c["gnoise"])
        assert model.nlml() == v


def test_ngnlml_returns_100_where_the_matrix_does_not_factor(lib, capsys):
    from ibo_amd.gaussianprocess import trainhyper
    from ibo_amd.gaussianprocess.kernel import MaternKernel3
    twin = gn.case("m3_10x2_twin")
    assert trainhyper.ngnlml(np.log(twin["kern"].hyper), MaternKernel3, twin["X"], twin["Y"], twin["G"], 0.0, 0.0) == 100
    assert "returning ngnlml = 100" in capsys.readouterr().out


def test_learn_lowers_the_likelihood_and_refits(lib):
    """16 x 3 ARD data drawn from the model at a known theta; the search starts a factor 2 off"""
    from ibo_amd.gaussianprocess import GaussianProcess
    from ibo_amd.gaussianprocess.kernel import GaussianKernel_ard
    from oracle import oracle as orc
    theta, noise, gnoise = np.array([0.5, 0.7, 0.6]), 0.01, 1e-3
    X = gr.points(16, 3, 11)
    A = gn.matrix_nl(orc.Kern("ard", theta), X, noise, gnoise)
    t = np.linalg.cholesky(A) @ np.random.RandomState(12).randn(len(A))
    Y, G = t.reshape(16, 4)[:, 0].copy(), t.reshape(16, 4)[:, 1:].copy()
    Q = gr.queries(X, 40)
    model = GaussianProcess(GaussianKernel_ard(2.0 * theta), X, Y, G=G, noise=noise, gnoise=gnoise)
    start = model.nlml()
    before = model.posteriors(Q)
    res = model.learn(maxiter=30)
    print("learn: %d evaluations, NLML %.6f -> %.6f, theta %s" % (res.evaluations, res.start_value, res.end_value, np.exp(res.x)))
    assert res.applied and res.start_value == start and res.end_value < start and model.nlml() == res.end_value
    learned = np.asarray(model.kernel.hyperparams, dtype=float)
    assert np.array_equal(learned, np.exp(res.x)) and not np.array_equal(learned, 2.0 * theta)
    fresh = GaussianProcess(GaussianKernel_ard(learned), X, Y, G=G, noise=noise, gnoise=gnoise)
    a, b = model.posteriors(Q), fresh.posteriors(Q)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and not np.array_equal(a[0], before[0])
    # the noises too, from where the first search ended: never worse
    res2 = model.learn(nhyper=0, noise=True, gnoise=True, maxiter=10)
    assert len(res2.x) == 4 and res2.start_value == res.end_value and res2.end_value <= res.end_value
    if res2.applied:
        assert model.noise == float(np.exp(res2.x[0])) and np.array_equal(model.gnoise, np.exp(res2.x[1:]))
        fresh = GaussianProcess(model.kernel, X, Y, G=G, noise=model.noise, gnoise=model.gnoise)
        assert np.array_equal(model.posteriors(Q)[0], fresh.posteriors(Q)[0])


def test_a_model_without_gradients_behaves_as_before(lib):
    from ibo_amd.gaussianprocess import GaussianProcess, trainhyper
    from ibo_amd.gaussianprocess.kernel import GaussianKernel_ard
    c = gn.case("ard_33x3")
    k = GaussianKernel_ard(c["kern"].hyper)
    model = GaussianProcess(k, c["X"], c["Y"], noise=c["noise"])
    mu = model.posteriors(c["X"][:5])
    with pytest.raises(NotImplementedError, match="trainhyper.nlml"):
        model.learn()
    with pytest.raises(NotImplementedError):
        model.nlml()
    after = model.posteriors(c["X"][:5])
    assert np.array_equal(mu[0], after[0]) and np.array_equal(mu[1], after[1])
    v, g = trainhyper.marginalLikelihood(k, c["X"], c["Y"], 3, noise=c["noise"])
    assert np.isfinite(v) and trainhyper.nlml_values([k], c["X"], c["Y"], noise=c["noise"])[0] == pytest.approx(v, rel=1e-10)
    with pytest.raises(NotImplementedError, match="marginalLikelihood"):
        trainhyper.marginalLikelihood(k, c["X"], c["Y"], 3, G=c["G"])


def test_stage_times_are_reported_under_the_timing_option(lib):
    c = gn.case("ard_60x4")
    ms = np.zeros(4)
    lib.check(lib.lib.ibo_ggp_grad_stage_ms(None, 1))
    lib.check(lib.lib.ibo_set_option(b"ggp_timing", 1))
    try:
        rc, v, g, gz = call(c, gn.spec_of(c["kern"]))
    finally:
        lib.check(lib.lib.ibo_set_option(b"ggp_timing", 0))
    lib.check(lib.lib.ibo_ggp_grad_stage_ms(lib.dp(ms), 1))
    v0, g0, gz0 = device_result("ard_60x4")
    assert rc == lib.OK and v == v0 and np.array_equal(g, g0) and np.array_equal(gz, gz0)
    assert np.all(ms > 0.0) and np.all(ms < 1e3), ms
    lib.check(lib.lib.ibo_ggp_grad_stage_ms(lib.dp(ms), 0))
    assert np.all(ms == 0.0)

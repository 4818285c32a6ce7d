"""
The NumPy restatement of max-value entropy search (tests/mes_reference.py, the yardstick of tests/test_gpu_mes.py) pinned: h, log Phi
and h' to mpmath at 60 digits over both tails; h to a quadrature of the truncated normal's differential entropy (the definition);
the gradient's sums and the gradient to central differences of the value; the Gumbel fit to the exact product of the cdfs at its
quartiles; the order of y*; and the ibo_mes_* symbols, their refusals without a device and the Python layer's refusals.  CPU only.

Bars (T, T': the magnitudes of the terms of h and h', mes_reference.py)
  * |h - truth| <= 2.5e-13 T + 1e-300 (a quarter of the device's bar), log Phi and h' alike on their own terms.  SciPy's erfc / erfcx
    leave the restatement at 5.8e-14 T over [-40, 37] (the exponent gamma^2 / 2 ~ 700 is rounded to 1.1e-13 of itself at most, and
    exp carries that into lambda and 1 - Phi) and 1.1e-16 T down to -1e5; the absolute term covers the subnormal results above 37;
  * central differences in the posterior: steps of d = 1e-5 sigma in mu and in sigma, the differences times sigma against
    sigma G with the bar 1e-6 (A + T), A the sums over the magnitudes of the h' terms (dimensionless).  In these units a step is
    d in gamma's own scale: the truncation is d^2 / 6 times a third derivative of the size of gamma^2 A at the worst (gamma up to 25
    here: 1e-8 A), the rounding 2 x 2.5e-13 T / (2 d) = 2.5e-8 T at the worst -- more than a decade of room on either;
  * the gradient in x against central differences of the value over a model: step 1e-5, bar 1e-6 (scale + T), the same reasoning with
    the posterior's own scale sums (tests/grad_reference.py) in place of A.
"""
import ctypes
import os
import re

import mpmath
import numpy as np
import pytest

from conftest import ROOT, synth
import cacq_reference as cr
import mes_reference as mr

SYMBOLS = ("ibo_mes_sweep", "ibo_mes_batch", "ibo_mes_grad_batch", "ibo_mes_direct_max", "ibo_mes_maxcdf")


def gamma_grid():
    return np.r_[np.linspace(-40.0, 40.0, 8001), np.random.RandomState(11).uniform(-40.0, 40.0, 8000), -1e3, -1e5, 1e3]


# ------------------------------------------------------------------------------------------------ (a) pinned to mpmath
def test_h_logcdf_and_dh_against_mpmath():
    g = gamma_grid()
    hv, T = mr.h(g)
    lc = mr.logcdf(g)
    dv, Td = mr.dh(g)
    assert np.all(np.isfinite(hv)) and np.all(np.isfinite(lc)) and np.all(np.isfinite(dv))
    worst = dict(h=0.0, h_far=0.0, logcdf=0.0, dh=0.0)
    with mpmath.workdps(mr.MP_DPS):
        for i, x in enumerate(g):
            lam, nll = mr.terms_mp(x)
            gx = mpmath.mpf(float(x))
            th, tT = gx * lam / 2 + nll, abs(gx * lam / 2) + abs(nll)
            td, tTd = -(lam / 2) * (1 + gx * gx + gx * lam), (lam / 2) * (1 + gx * gx + abs(gx * lam))
            bar = 2.5e-13 * tT + mpmath.mpf("1e-300")
            e = abs(mpmath.mpf(float(hv[i])) - th)
            assert e <= bar, ("h", x, float(e / bar))
            el = abs(mpmath.mpf(float(lc[i])) + nll)
            assert el <= 2.5e-13 * abs(nll) + mpmath.mpf("1e-300"), ("log Phi", x)
            ed = abs(mpmath.mpf(float(dv[i])) - td)
            assert ed <= 2.5e-13 * tTd + mpmath.mpf("1e-300"), ("h'", x, float(ed / tTd) if tTd > 0 else 0.0)
            if tT > mpmath.mpf("1e-280"):
                key = "h" if -40.0 <= x <= 37.0 else "h_far"
                worst[key] = max(worst[key], float(e / tT))
                worst["logcdf"] = max(worst["logcdf"], float(el / abs(nll)))
                worst["dh"] = max(worst["dh"], float(ed / tTd))
            # the restated T is the truth's to rounding: the bars of the GPU tests are made of it
            assert abs(mpmath.mpf(float(T[i])) - tT) <= 1e-12 * tT + mpmath.mpf("1e-300")
    print("worst errors in units of the terms' magnitude:", worst)


def test_h_is_the_entropy_lost_to_the_truncation():
    """h(g) = H[N(0, 1)] - H[N(0, 1) truncated above at g], the second by quadrature of -p log p, p = phi / Phi(g) on (-inf, g]"""
    with mpmath.workdps(40):
        H0 = mpmath.log(2 * mpmath.pi * mpmath.e) / 2
        for g in (-6.0, -2.0, -.5, 0.0, .5, 2.0, 6.0):
            Phi = mpmath.ncdf(g)
            p = lambda x: mpmath.npdf(x) / Phi
            Ht = -mpmath.quad(lambda x: p(x) * mpmath.log(p(x)), [-mpmath.inf, g - 12, g - 4, g])
            hv, T = mr.h(np.array([g]))
            assert abs(mpmath.mpf(float(hv[0])) - (H0 - Ht)) <= 2.5e-13 * float(T[0]) + mpmath.mpf("1e-20"), g
    assert mr.h(np.array([0.0]))[0][0] > 0 and np.all(np.diff(mr.h(np.linspace(-8, 8, 200))[0]) < 0)     # positive, falling in g


# ------------------------------------------------------------------------------------------------ (b) gradients
def posteriors():
    rs = np.random.RandomState(5)
    return rs.randn(60) * .8, rs.rand(60) * .5 + .02


def test_partial_sums_against_central_differences():
    mu, s2 = posteriors()
    d = 1e-5
    for K, spread in ((1, 0.0), (7, 1.0), (64, 3.0)):
        ys = 1.2 + spread * np.random.RandomState(K).rand(K)
        r = mr.from_posterior(mu, s2, ys)
        sig = r["sig"]
        f = lambda m, s: mr.from_posterior(m, s * s, ys)["val"]
        dmu = (f(mu + d * sig, sig) - f(mu - d * sig, sig)) / (2 * d)           # sigma dMES/dmu
        dsg = (f(mu, sig + d * sig) - f(mu, sig - d * sig)) / (2 * d)           # sigma dMES/dsigma
        bar = 1e-6 * (sig * (r["amu"] + r["asig"]) + r["T"])
        emu, esg = np.abs(dmu - sig * r["gmu"]), np.abs(dsg - sig * r["gsig"])
        print("K=%d: worst dMES/dmu %.3g, dMES/dsigma %.3g of the bar (gamma in [%.3g, %.3g])"
              % (K, np.max(emu / bar), np.max(esg / bar), np.min(r["gmin"]), np.max(r["gmax"])))
        assert np.all(emu <= bar) and np.all(esg <= bar)
        assert np.all(r["gmu"] > 0)                              # h falls in gamma: a mean nearer the maximum tells more


@pytest.mark.parametrize("kind,hyper,with_prior", [("iso", [.4], False), ("ard", [.5, .6, .45], True), ("m3", [.7, .95], False), ("m5", [.45, .9], False)])
def test_gradient_against_central_differences_of_the_value(kind, hyper, with_prior):
    X, Y = synth(21, 40, 3)
    prior = None
    if with_prior:
        rs = np.random.RandomState(7)
        prior = (rs.rand(4, 3), rs.randn(4), 2.0, np.zeros(3) - .1, np.full(3, 1.2))
    m = cr.make(X, Y, .05, kind, hyper, prior=prior)
    Q = np.random.RandomState(8).rand(12, 3)
    ys = float(np.max(Y)) + np.array([.05, .3, .1, .6])
    off = 1.0 + .05 - m.ref.sf2 if 1.0 + .05 - m.ref.sf2 >= 0 else 0.0
    rg = mr.value_grad(m, Q, ys, off, 1e-8)
    d = 1e-5
    for j in range(3):
        e = np.zeros(3); e[j] = d
        fd = (mr.value(m, Q + e, ys, off, 1e-8)["val"] - mr.value(m, Q - e, ys, off, 1e-8)["val"]) / (2 * d)
        bar = 1e-6 * (rg["sval"][:, j] + rg["T"])
        assert np.all(np.abs(fd - rg["dval"][:, j]) <= bar), (kind, j, float(np.max(np.abs(fd - rg["dval"][:, j]) / bar)))
    assert np.max(np.abs(rg["dval"])) > 1e-3


def test_floor_of_the_latent_variance():
    """s2 - s2_offset below clamp_lo: sigma^2 = clamp_lo and the variance's part of the gradient is gone"""
    r = mr.from_posterior(np.array([.1, .1]), np.array([.2, .05]), [.5, .7], s2_offset=.1, clamp_lo=1e-7)
    assert r["sig"][0] == np.sqrt(.2 - .1) and r["sig"][1] == np.sqrt(1e-7) and list(r["follows"]) == [True, False]


# ------------------------------------------------------------------------------------------------ (c) the Gumbel fit
def test_gumbel_fit_against_the_exact_product():
    """synthetic (mu_i, sigma_i): the fit's quartiles lie in the right cell of the level grid, between the exact cdf's values at its
    ends (monotone interpolation), the Gumbel cdf through (a, b) takes 1/2 at y50 exactly and 1/4, 3/4 at points y75 - y25 apart"""
    rs = np.random.RandomState(3)
    for M in (1, 50, 400):
        mu, s2 = rs.randn(M) * .7, rs.rand(M) * .4 + .01
        _, _, lo, hi = mr.maxcdf(mu, s2, [])
        assert lo == np.max(mu) and hi == np.max(mu + 5 * np.sqrt(s2))
        lev = np.linspace(lo, hi, 64)
        lc, mag, _, _ = mr.maxcdf(mu, s2, lev)
        a, b, q = mr.gumbel_fit(lev, lc)
        assert b > 0 and q[0] <= q[1] < q[2]
        with mpmath.workdps(40):
            exact = lambda t: float(mpmath.fprod(mpmath.ncdf((mpmath.mpf(float(t)) - float(m)) / float(np.sqrt(v))) for m, v in zip(mu, s2)))
            cdf = np.array([exact(t) for t in lev])
            # the ordered sum against the product: 1e-12 of the sum's magnitude, and the roundings of exp and of the product's float
            assert np.all(np.abs(np.exp(lc) - cdf) <= (1e-12 * mag + 4 * np.finfo(float).eps) * cdf + 1e-300)
            for p, y in zip((.25, .5, .75), q):
                if p < cdf[0]:
                    assert y == lev[0]                           # (few candidates: the bracket's lower end is above the quartile)
                    continue
                j = int(np.searchsorted(cdf, p, side="right")) - 1
                assert lev[j] <= y <= lev[j + 1] and cdf[j] <= exact(y) <= cdf[j + 1], (M, p)
        G = lambda y: np.exp(-np.exp(-(y - a) / b))
        assert abs(G(q[1]) - .5) < 1e-12
        y25g, y75g = a - b * np.log(np.log(4.0)), a - b * np.log(np.log(4.0 / 3.0))
        assert abs((y75g - y25g) - (q[2] - q[0])) < 1e-12 * (1 + abs(q[2]))
        s = mr.gumbel_samples(a, b, lo, 500, 9)
        assert np.all(s >= lo) and np.array_equal(s, mr.gumbel_samples(a, b, lo, 500, 9)) and np.ptp(s) > 0


def test_library_gumbel_fit_is_the_restatements():
    from ibo_amd.acquisition.entropy import gumbelFit
    mu, s2 = posteriors()
    _, _, lo, hi = mr.maxcdf(mu, s2, [])
    lev = np.linspace(lo, hi, 64)
    lc = mr.maxcdf(mu, s2, lev)[0]
    assert gumbelFit(lev, lc) == mr.gumbel_fit(lev, lc)[:2]


# ------------------------------------------------------------------------------------------------ (d) the order of y*
def test_value_does_not_depend_on_the_order_of_ystar():
    mu, s2 = posteriors()
    ys = 1.0 + np.random.RandomState(2).rand(65)
    r0 = mr.from_posterior(mu, s2, ys)
    for seed in (1, 2):
        r1 = mr.from_posterior(mu, s2, ys[np.random.RandomState(seed).permutation(65)])
        assert all(np.array_equal(r0[k], r1[k]) for k in ("val", "gmu", "gsig"))


# ------------------------------------------------------------------------------------------------ (e) symbols and refusals
def test_symbols_are_declared_exported_and_bound():
    from ibo_amd import _lib
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ibo_abi.h")).read(), flags=re.S)
    for s in SYMBOLS + ("ibo_mes_scan_ms",):
        assert re.search(r"\b%s\s*\(" % s, txt), "%s is not declared in ibo_abi.h" % s
        assert hasattr(_lib.lib, s), "libibo_hip.so does not export %s" % s
        assert s in _lib.EXPORTED
    assert re.search(r"#define\s+IBO_MES_MAX_SAMPLES\s+1024\b", txt) and re.search(r"#define\s+IBO_MES_MAX_LEVELS\s+64\b", txt)
    assert _lib.lib.ibo_abi_version() == 8
    L = _lib.lib
    for key in (b"mes_chunk", b"mes_timing"):
        assert L.ibo_set_option(key, 0) == _lib.OK
    assert L.ibo_set_option(b"mes_chunk", -1) == _lib.ERR_ARG


def test_refusals_that_need_no_device():
    """what the samples alone decide is refused with or without a device; with valid samples and no device: IBO_ERR_NO_DEVICE"""
    from ibo_amd import _lib
    L = _lib.lib
    Q = _lib.f64(np.zeros((2, 3))); out = np.empty(6); lb = _lib.f64(np.zeros(3)); ub = _lib.f64(np.ones(3))
    bv = ctypes.c_double(); bi = ctypes.c_int64()
    ok = _lib.f64([.5, 1.5, 1.0])
    big = _lib.f64(np.linspace(0, 1, 1025))

    def all_four(K, ys, off):
        lead = (None, K, None if ys is None else _lib.dp(ys), off)
        return [L.ibo_mes_sweep(*(lead + (2, None, 1e-8, 0, None, .5, 0, None, ctypes.byref(bv), ctypes.byref(bi)))),
                L.ibo_mes_batch(*(lead + (2, _lib.dp(Q), 1e-8, _lib.dp(out)))),
                L.ibo_mes_grad_batch(*(lead + (2, _lib.dp(Q), 1e-8, _lib.dp(out), None))),
                L.ibo_mes_direct_max(*(lead + (3, _lib.dp(lb), _lib.dp(ub), 1e-8, 5, 5, 100, 1, ctypes.byref(bv), _lib.dp(out), None)))]

    ARG = _lib.ERR_ARG
    assert all_four(3, None, 0.0) == [ARG] * 4
    assert all_four(0, ok, 0.0) == [ARG] * 4 and all_four(-1, ok, 0.0) == [ARG] * 4
    assert all_four(1025, big, 0.0) == [ARG] * 4
    for bad in (np.nan, np.inf, -np.inf):
        ys = ok.copy(); ys[1] = bad
        assert all_four(3, ys, 0.0) == [ARG] * 4
    for off in (-1e-3, np.nan, np.inf):
        assert all_four(3, ok, off) == [ARG] * 4
    lev = _lib.f64([0., np.nan])
    stats = np.empty(2)
    assert L.ibo_mes_maxcdf(None, 2, None, 65, _lib.dp(lev), 0.0, 1e-8, _lib.dp(out), _lib.dp(stats)) == ARG
    assert L.ibo_mes_maxcdf(None, 2, None, -1, _lib.dp(lev), 0.0, 1e-8, _lib.dp(out), _lib.dp(stats)) == ARG
    assert L.ibo_mes_maxcdf(None, 2, None, 2, _lib.dp(lev), 0.0, 1e-8, _lib.dp(out), _lib.dp(stats)) == ARG          # a NaN level
    assert L.ibo_mes_maxcdf(None, 2, None, 2, None, 0.0, 1e-8, _lib.dp(out), _lib.dp(stats)) == ARG
    assert L.ibo_mes_maxcdf(None, 2, None, 0, None, -1.0, 1e-8, None, _lib.dp(stats)) == ARG
    assert L.ibo_mes_scan_ms(None, 1) == _lib.OK
    if _lib.device_count() > 0:
        return                                       # (tests/test_gpu_mes.py takes over where a GPU is visible)
    NODEV = _lib.ERR_NO_DEVICE
    assert all_four(3, ok, 0.0) == [NODEV] * 4 and all_four(1024, big, .25) == [NODEV] * 4
    assert L.ibo_mes_maxcdf(None, 2, None, 0, None, 0.0, 1e-8, None, _lib.dp(stats)) == NODEV


def stub_model(n=4, D=2, G=None, aug=None, pref=False):
    """a model object as the refusals see it -- none of them reaches the device"""
    from ibo_amd.gaussianprocess import GaussianProcess, PrefGaussianProcess
    GP = object.__new__(PrefGaussianProcess if pref else GaussianProcess)
    GP.X = [np.zeros(D)] * n
    GP.Y = [0.0] * n
    GP.G, GP._augdev = G, aug
    return GP


def test_python_refusals():
    from ibo_amd.acquisition import entropy as en
    from ibo_amd.acquisition import MaxValueEntropy, maxValueSamples, sweepMES, maximizeMES           # exported
    assert MaxValueEntropy is en.MaxValueEntropy and maximizeMES is en.maximizeMES
    bounds, Q, ys = [[0., 1.]] * 2, np.zeros((3, 2)), [1.0, 2.0]
    calls = lambda GP: (lambda: MaxValueEntropy(GP, ys), lambda: sweepMES(GP, Q, ys), lambda: maximizeMES(GP, bounds, ys),
                        lambda: maxValueSamples(GP, bounds), lambda: maxValueSamples(GP, candidates=Q), lambda: maximizeMES(GP, bounds))
    for call in calls(stub_model(G=np.zeros((4, 2)))):
        with pytest.raises(NotImplementedError, match="max-value entropy search"):
            call()
    with pytest.raises(NotImplementedError):
        maxValueSamples(stub_model(G=np.zeros((4, 2))), bounds, method='paths')
    for call in calls(stub_model(aug=object())):
        with pytest.raises(ValueError, match="augmented factor"):
            call()
    for call in calls(stub_model(n=0)):
        with pytest.raises(ValueError, match="no data"):
            call()
    with pytest.raises(NotImplementedError, match="preference GP"):
        maxValueSamples(stub_model(pref=True), bounds, method='paths')
    GP = stub_model()
    for bad in ([], np.zeros(1025), [1.0, np.nan], [np.inf]):
        with pytest.raises(ValueError):
            MaxValueEntropy(GP, bad)
        with pytest.raises(ValueError):
            sweepMES(GP, Q, bad)
    with pytest.raises(ValueError):
        MaxValueEntropy(GP, ys).values(np.zeros((2, 3)))         # points of another width
    with pytest.raises(ValueError):
        maxValueSamples(GP, bounds, method='sobol')
    with pytest.raises(ValueError):
        maxValueSamples(GP, bounds, n=0)
    with pytest.raises(ValueError):
        maxValueSamples(GP)
    assert list(MaxValueEntropy(GP, [3., 1., 2.]).ystar) == [1., 2., 3.]

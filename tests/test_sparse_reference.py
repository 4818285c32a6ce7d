"""
tests/sparse_reference.py -- the NumPy restatement tests/test_gpu_sparse.py holds the device to -- pinned without a GPU: the route against
the dense definition and the whitened form in long double, float64 against long double on every listed case, the orderings of the three
marginal likelihoods, the Z = X limit against the exact model, addData in two parts; and the new symbols are declared, exported and bound.
"""
import ctypes
import os
import re

import numpy as np
import pytest

import sparse_reference as sr
from conftest import ROOT
from oracle import oracle as orc

DENSE_NAMES = [n for n in sr.CASE_NAMES if sr.case(n)["N"] <= sr.DENSE_MAX]


def _f64(a):
    return np.asarray(a, dtype=np.float64)


def _args(c):
    return c["kern"], c["Z"], c["X"], c["Y"], c["noise"], c["jitter"], c["method"]


def _worst(got, want, bar):
    return float(np.max(np.abs(_f64(np.asarray(got, dtype=sr.LD) - np.asarray(want, dtype=sr.LD))) / _f64(bar)))


def test_the_case_list_covers_what_it_claims():
    cs = [sr.case(n) for n in sr.CASE_NAMES]
    assert {c["kern"].ktype for c in cs} == {orc.K_SE_ARD, orc.K_SE_ISO, orc.K_MATERN3, orc.K_MATERN5}
    assert min(c["D"] for c in cs) == 1 and max(c["D"] for c in cs) == 33
    assert {63, 64, 65, 129, 130, 1} <= {c["m"] for c in cs} and any(c["N"] < c["m"] for c in cs)
    assert {sr.FITC, sr.DTC} == {c["method"] for c in cs}
    assert any(c["kern"].sf2_py == pytest.approx(0.81) for c in cs) and any(np.min(c["X"]) >= 100.0 for c in cs)
    c = sr.case("m100_n300_zsub")
    m = sr.case_model("m100_n300_zsub", True)
    assert np.sum(_f64(m["q"]) > 1.0 - 1e-5) >= 100, "lambda's clamp region is not reached"


@pytest.mark.parametrize("name", DENSE_NAMES)
def test_route_dense_definition_and_whitened_form_agree_in_long_double(name):
    c = sr.case(name)
    m = sr.case_model(name, True)
    p = sr.posterior(m, c["Q"], clamp_lo=-1.0)
    bmu, bs2, bnl = sr.bars(m, p)
    for other in (sr.dense(*_args(c), c["Q"]), sr.whitened(*_args(c), c["Q"], longdouble=True)):
        assert _worst(p["mu"], other["mu"], bmu) <= 1e-3
        assert _worst(p["s2_raw"], other["s2_raw"], bs2) <= 1e-3
        assert abs(float(m["nlml"] - other["nlml"])) <= 1e-3 * bnl
        if c["method"] == sr.DTC:
            assert abs(float(m["vfe"] - other["vfe"])) <= 1e-3 * bnl


@pytest.mark.parametrize("name", sr.CASE_NAMES)
def test_float64_route_is_within_a_tenth_of_the_bars_of_long_double(name):
    c = sr.case(name)
    m, ml = sr.case_model(name), sr.case_model(name, True)
    p, pl = sr.posterior(m, c["Q"], clamp_lo=-1.0), sr.posterior(ml, c["Q"], clamp_lo=-1.0)
    bmu, bs2, bnl = sr.bars(ml, pl)
    worst = max(_worst(p["mu"], pl["mu"], bmu), _worst(p["s2_raw"], pl["s2_raw"], bs2), abs(float(m["nlml"] - ml["nlml"])) / bnl)
    print("%s: float64 route against long double, worst ratio to the bars %.3g (cond A %.3g, cond Kuu %.3g)" % (name, worst, ml["condA"], ml["condU"]))
    assert worst <= 0.1
    # G, b and yy of the float64 restatement against long double FROM THE SAME lambda, at the Gram bar
    G, b, yy, aG, ab = sr.gram(c["kern"], c["Z"], c["X"], c["Y"], _f64(m["lam"]), sr.LD)
    ayy = float(yy)
    bar = sr.gram_bar(c["kern"], c["Z"], c["X"], c["N"], aG)
    assert np.all(np.abs(_f64(m["G"] - G)) <= bar)
    assert np.all(np.abs(_f64(m["b"] - b)) <= sr.gram_bar(c["kern"], c["Z"], c["X"], c["N"], ab))
    assert abs(float(m["yy"] - yy)) <= (c["N"] + 8) * sr.U * ayy


@pytest.mark.parametrize("name", sr.CASE_NAMES)
def test_whitened_float64_form_is_within_1e4_of_the_bars(name):
    c = sr.case(name)
    ml = sr.case_model(name, True)
    pl = sr.posterior(ml, c["Q"], clamp_lo=-1.0)
    bmu, bs2, bnl = sr.bars(ml, pl)
    w = sr.whitened(*_args(c), c["Q"])
    worst = max(_worst(w["mu"], pl["mu"], bmu), _worst(w["s2_raw"], pl["s2_raw"], bs2), abs(float(w["nlml"] - ml["nlml"])) / bnl)
    print("%s: whitened float64 against long double, worst ratio %.3g" % (name, worst))
    assert worst <= 1e-4


@pytest.mark.parametrize("name", sr.ROUTE_NAMES)
def test_route_cases_stay_within_the_bars_of_the_whitened_float64_form(name):
    c = sr.case(name)
    m = sr.case_model(name)
    p = sr.posterior(m, c["Q"], clamp_lo=-1.0)
    bmu, bs2, bnl = sr.bars(m, p)
    w = sr.whitened(*_args(c), c["Q"])
    worst = max(_worst(p["mu"], w["mu"], bmu), _worst(p["s2_raw"], w["s2_raw"], bs2), abs(float(m["nlml"] - w["nlml"])) / bnl)
    print("%s: cond A %.3g, route against whitened float64, worst ratio %.3g" % (name, m["condA"], worst))
    assert worst <= 0.1


@pytest.mark.parametrize("name", ["m16_n200", "m100_n300_zsub", "m64_n300_j8"])
def test_vfe_bounds_the_exact_nlml_and_dtc_is_below_vfe(name):
    c = sr.case(name)
    m = sr.route(c["kern"], c["Z"], c["X"], c["Y"], c["noise"], c["jitter"], sr.DTC, longdouble=True)
    exact = sr.exact_nlml(c["kern"], c["X"], c["Y"], c["noise"])
    slack = m["f"] * m["nlml_scale"]
    assert float(m["vfe"]) >= float(exact) - slack and float(m["nlml"]) <= float(m["vfe"])


@pytest.mark.parametrize("kind,hyper,D", [("ard", [0.5, 0.6], 2), ("m5", [0.6, 1.0], 3)])
def test_z_equal_x_fitc_is_the_exact_model_at_the_data_rows(kind, hyper, D):
    """(sf2 = 1: with another magnitude the cross-covariance of a point with itself is sf2 while every diagonal counts 1, and Z = X is
    no longer the exact model)"""
    rng = np.random.RandomState(5)
    N, noise, j = 120, 0.05, 1e-6
    X = rng.rand(N, D)
    Y = sr.objective(X) + np.sqrt(noise) * rng.randn(N)
    kern = orc.Kern(kind, hyper)
    m = sr.route(kern, X, X, Y, noise, j, sr.FITC, longdouble=True)
    p = sr.posterior(m, X, clamp_lo=sr.CLAMP_PY)
    mu, s2 = orc.GP(kern, X, Y, noise=noise).posteriors(X)
    dmu, ds2 = sr.zx_bound(kern, X, Y, noise, j)
    bmu, bs2, _ = sr.bars(m, p)
    emu, es2 = np.abs(_f64(p["mu"]) - mu), np.abs(_f64(p["s2"]) - s2)
    print("Z = X (%s): |d mu| <= %.3g (bound %.3g), |d s2| <= %.3g (bound %.3g)" % (kind, emu.max(), dmu.max(), es2.max(), ds2.max()))
    assert np.all(emu <= dmu + bmu) and np.all(es2 <= ds2 + bs2)
    assert emu.max() > 0.0


@pytest.mark.parametrize("name", ["m16_n200", "m65_n1000", "m130_n2100"])
def test_adddata_in_two_parts_is_one_fit_within_the_bars(name):
    c = sr.case(name)
    one = sr.case_model(name)
    k = c["N"] // 3
    a = sr.route(c["kern"], c["Z"], c["X"][:k], c["Y"][:k], c["noise"], c["jitter"], c["method"])
    two = sr.route(c["kern"], c["Z"], c["X"][k:], c["Y"][k:], c["noise"], c["jitter"], c["method"], prev=a)
    p1, p2 = sr.posterior(one, c["Q"]), sr.posterior(two, c["Q"])
    bmu, bs2, bnl = sr.bars(one, p1)
    assert two["N"] == one["N"] and np.array_equal(two["lam"], one["lam"]) and two["maxY"] == one["maxY"]
    assert np.all(np.abs(p1["mu"] - p2["mu"]) <= bmu) and np.all(np.abs(p1["s2"] - p2["s2"]) <= bs2) and abs(one["nlml"] - two["nlml"]) <= bnl


# ---------------------------------------------------------------------------- symbols
SGP_SYMBOLS = ["ibo_sgp_create", "ibo_sgp_destroy", "ibo_sgp_fit", "ibo_sgp_add", "ibo_sgp_acq_batch", "ibo_sgp_acq_sweep", "ibo_sgp_direct_max",
               "ibo_sgp_nlml", "ibo_sgp_get", "ibo_sgp_stage_ms"]


def test_the_symbols_are_declared_exported_and_bound_and_the_abi_version_stays():
    from ibo_amd import _lib
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ibo_abi.h")).read(), flags=re.S)
    for s in SGP_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % s, txt), "%s is not declared in ibo_abi.h" % s
        assert getattr(_lib.lib, s).argtypes is not None, "%s is not bound" % s
        assert s in _lib.EXPORTED
    assert "typedef struct ibo_sgp ibo_sgp_t;" in txt and re.search(r"#define\s+IBO_SGP_MAX_M\s+8192\b", txt)
    assert re.search(r"#define\s+IBO_ABI_VERSION\s+8\b", txt) and _lib.lib.ibo_abi_version() == 8


def test_the_options_exist_and_no_entry_computes_without_a_device():
    from ibo_amd import _lib
    assert _lib.lib.ibo_set_option(b"sgp_chunk", 512) == _lib.OK and _lib.lib.ibo_set_option(b"sgp_chunk", 0) == _lib.OK
    assert _lib.lib.ibo_set_option(b"sgp_chunk", -1) == _lib.ERR_ARG
    assert _lib.lib.ibo_set_option(b"sgp_timing", 0) == _lib.OK
    ms = np.zeros(8)
    assert _lib.lib.ibo_sgp_stage_ms(_lib.dp(ms), 1) == _lib.OK and np.all(ms == 0.0)
    if _lib.device_count() > 0:
        return                                                      # (a GPU is visible: the refusal without one cannot be observed here)
    h = ctypes.c_void_p()
    assert _lib.lib.ibo_sgp_create(0, ctypes.byref(h)) == _lib.ERR_NO_DEVICE
    q = np.zeros((1, 2)); out = np.zeros(1)
    assert _lib.lib.ibo_sgp_acq_batch(None, 1, _lib.dp(q), 0, 0.0, 0, 1e-8, float("nan"), _lib.dp(out), None, None) == _lib.ERR_NO_DEVICE


def test_the_host_side_of_the_python_class_needs_no_device():
    from ibo_amd.gaussianprocess import SparseGaussianProcess, inducingPoints, GaussianKernel_iso
    X = np.random.RandomState(3).rand(50, 2)
    for method in ("subset", "kcenter"):
        Z1, Z2 = inducingPoints(X, 7, method, seed=4), inducingPoints(X, 7, method, seed=4)
        assert Z1.shape == (7, 2) and np.array_equal(Z1, Z2) and all(any(np.array_equal(z, x) for x in X) for z in Z1)
        assert len({tuple(z) for z in Z1}) == 7
    with pytest.raises(ValueError):
        inducingPoints(X, 51)
    with pytest.raises(NotImplementedError, match="prior"):
        SparseGaussianProcess(GaussianKernel_iso([0.5]), prior=object())
    g = SparseGaussianProcess(GaussianKernel_iso([0.5]), m=5)
    assert g.posterior(X[0]) == (0.0, 1.0)
    for call in ("removeData", "posterior_gradient", "posterior_cov", "sample_posterior", "loo", "loo_score"):
        with pytest.raises(NotImplementedError, match=call):
            getattr(g, call)()

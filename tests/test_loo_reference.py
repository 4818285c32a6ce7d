"""
The NumPy restatement of leave-one-out prediction and the LOO-CV objective (tests/loo_reference.py, the yardstick of
tests/test_gpu_loo.py) against the oracle: every leave-one-out prediction is the oracle's posterior of the model refitted without that
point, the value is the sum of the per-point terms, the gradient matches central differences of the value, and the float64 variant
agrees with the long-double one.  CPU only.

Bounds: 1e-10 against the oracle's refits (its own posterior's accuracy at cond ~ 1e2); 1e-6 S_h against central differences with step
1e-5 in log theta (truncation ~ step^2 = 1e-10 of the terms' scale, rounding ~ 1e-16 |value| / step ~ 1e-11 |value|); 1e-10 S_h between
float64 and long double at cond_2 <= 1e6 (cond * 2^-53 = 1e-10).  cond_2 <= 1e6 is asserted here on every GPU case up to 1100 rows (the
long-double variant, whose products run without BLAS, up to 200 rows); the larger GPU cases assert it themselves before they compare.
"""
import ctypes

import numpy as np
import pytest

from conftest import synth
from oracle import oracle as orc
import loo_reference as lr

KERNELS = [("ard", [.3, .5, .4]), ("iso", [.4]), ("svard", [.3, .5, .4, .9]), ("sviso", [.4, .8]),
           ("m3", [.5, .95]), ("m5", [.5, 0.9])]
assert tuple(k for k, _ in KERNELS) == lr.KINDS


def _prior():
    rs = np.random.RandomState(7)
    return orc.Prior(rs.rand(4, 3), rs.randn(4), 2.0, np.zeros(3) - .1, np.full(3, 1.2))


@pytest.mark.parametrize("with_prior", [False, True])
@pytest.mark.parametrize("kind,hyper", KERNELS)
def test_every_prediction_is_the_oracle_refit_without_that_point(kind, hyper, with_prior):
    N = 40
    X, Y = synth(5, N, 3)
    prior = _prior() if with_prior else None
    kern = orc.Kern(kind, hyper)
    res = lr.handle_loo(orc.GP(kern, X, Y, noise=.1, prior=prior))
    assert res["s2"].min() > 1e-7 and res["s2"].max() < 10          # inside the oracle's clip
    for i in range(N):
        mu, s2 = lr.brute_force(kern, X, Y, .1, prior, i)
        assert abs(res["mu"][i] - mu) <= 1e-10, (i, res["mu"][i], mu)
        assert abs(res["s2"][i] - s2) <= 1e-10, (i, res["s2"][i], s2)
    # the objective is the negative log predictive density of every left-out target
    want = 0.5 * np.log(res["s2"]) + (Y - res["mu"]) ** 2 / (2 * res["s2"]) + lr.HALF_LOG_2PI
    np.testing.assert_allclose(res["terms"], want, rtol=0, atol=1e-12)
    assert res["value"] == res["terms"].sum()


# Kernel.derivative(X, 0) of the Matern-3/2 kernel is the reference's own: sf2 r^2 exp(-r) on the UNSCALED distance r, which is
# dK / d log theta only at theta = sqrt(3).  The objective's gradient is defined on that matrix, so for it the central difference in
# log theta is taken at theta = sqrt(3), and at the suite's theta = .5 along the matrix path A + t dA_h (below, every family and mode).
@pytest.mark.parametrize("kind,hyper", KERNELS + [("m3", [np.sqrt(3.0), .95])])
def test_value_is_the_sum_of_terms_and_gradient_matches_central_differences(kind, hyper):
    X, Y = synth(5, 40, 3)
    hyper = np.array(hyper, dtype=float)
    nh = len(hyper)
    kern = orc.Kern(kind, hyper)
    res = lr.objective(kern, X, Y, lr.NOISE, nh)
    assert res["value"] == res["terms"].sum()
    A = kern.cov_matrix(X) + lr.NOISE * np.eye(len(X))
    step = 1e-5
    for h in range(nh):
        e = np.zeros(nh); e[h] = step
        dA = kern.derivative(X, h)
        cdm = (lr.loo_points(A + step * dA, Y)["value"] - lr.loo_points(A - step * dA, Y)["value"]) / (2 * step)
        print(kind, h, "grad %.12g along A + t dA %.12g S_h %.6g" % (res["grad"][h], cdm, res["S"][h]))
        assert abs(res["grad"][h] - cdm) <= 1e-6 * res["S"][h]
        if kind == "m3" and h == 0 and hyper[0] != np.sqrt(3.0):
            continue
        vp = lr.objective(orc.Kern(kind, hyper * np.exp(e)), X, Y, lr.NOISE)["value"]
        vm = lr.objective(orc.Kern(kind, hyper * np.exp(-e)), X, Y, lr.NOISE)["value"]
        cd = (vp - vm) / (2 * step)
        print(kind, h, "grad %.12g central difference in log theta %.12g" % (res["grad"][h], cd))
        assert abs(res["grad"][h] - cd) <= 1e-6 * res["S"][h]


def _small(case):
    kind, hyper, N, D, seed = case
    X, Y = synth(seed, N, D)
    return kind, hyper, X[:200], Y[:200]


@pytest.mark.parametrize("case", lr.FAMILY_CASES + lr.EDGE_CASES, ids=lambda c: "%s-N%d-D%d" % (c[0], c[2], c[3]))
def test_float64_agrees_with_long_double(case):
    kind, hyper, N, D, seed = case
    X, Y = synth(seed, N, D)
    if N <= 1100:
        A = orc.Kern(kind, hyper).cov_matrix(X) + lr.NOISE * np.eye(N)
        c = lr.cond2(A)
        print("cond_2 = %.3g" % c)
        assert c <= 1e6
    kind, hyper, X, Y = _small(case)              # the case itself, or its first 200 points
    nh = len(hyper)
    r64 = lr.objective(orc.Kern(kind, hyper), X, Y, lr.NOISE, nh)
    rld = lr.objective(orc.Kern(kind, hyper), X, Y, lr.NOISE, nh, longdouble=True)
    assert r64["cond"] <= 1e6
    err = np.abs(r64["grad"] - rld["grad"]).astype(float)
    print("cond %.3g  max err / S_h = %.3g  S_h / |g| = %s" % (r64["cond"], np.max(err / np.maximum(r64["S"], 1e-300)) if nh else 0.0,
                                                              r64["S"] / np.maximum(np.abs(r64["grad"]), 1e-300)))
    assert np.all(err <= 1e-10 * r64["S"])
    assert abs(float(r64["value"] - rld["value"])) <= 1e-10 * (len(X) + abs(r64["value"]))
    assert np.all(np.abs((r64["s2"] - rld["s2"]).astype(float)) <= 1e-10 * r64["s2"])
    assert np.all(np.abs((r64["mu"] - rld["mu"]).astype(float)) <= 1e-10 * (np.abs(Y) + np.abs(r64["c"]) / r64["d"]))


def test_entries_without_a_gpu_report_no_device():
    from ibo_amd import _lib
    if _lib.device_count() > 0:
        pytest.skip("a GPU is visible here")
    X = _lib.f64(np.zeros((2, 3))); Y = _lib.f64(np.zeros(2)); th = _lib.f64([.5, .5, .5])
    v = ctypes.c_double(); mu = np.empty(2)
    assert _lib.lib.ibo_loo_grad(0, _lib.K_SE_ARD, 2, 3, _lib.dp(X), _lib.dp(Y), _lib.dp(th), 3, 1.0, 1e-2, 0, None, None,
                                 ctypes.byref(v), None, _lib.dp(mu), None) == _lib.ERR_NO_DEVICE
    assert _lib.lib.ibo_gp_loo(None, _lib.dp(mu), None, None) == _lib.ERR_ARG
    from ibo_amd.gaussianprocess import PrefGaussianProcess
    from ibo_amd.gaussianprocess.kernel import GaussianKernel_ard
    with pytest.raises(NotImplementedError):
        PrefGaussianProcess(GaussianKernel_ard([.5] * 3)).loo()
    with pytest.raises(NotImplementedError):
        PrefGaussianProcess(GaussianKernel_ard([.5] * 3)).loo_score()

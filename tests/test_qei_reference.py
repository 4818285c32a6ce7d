"""
The NumPy restatement of the Monte-Carlo parallel expected improvement (tests/qei_reference.py, the yardstick of
tests/test_gpu_qei.py) pinned three ways: without pending points against the oracle's EI, with pending points against the oracle's own
extension (draw the pending observations, refit, take EI against the raised incumbent), and `compose` against its own long-double
evaluation.  Plus the exact property the ABI promises (every value >= base) in the device's summation order.  CPU only.
"""
import ctypes
import os
import re

import numpy as np
import pytest

from oracle import oracle as orc
import grad_reference as gr
import qei_reference as qr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["ibo_qei_sweep", "ibo_qei_batch", "ibo_qei_direct_max", "ibo_qei_stage_ms"]
MODELS = [("ard", [.3, .5, .4]), ("sviso", [.4, .8]), ("m3", [.5, .95]), ("m5", [.5, .9])]


def small_model(kind, hyper, seed=5, N=30):
    from conftest import synth
    X, Y = synth(seed, N, 3)
    fam, w, sf2 = gr.kernel_spec(kind, hyper, 3)
    return X, Y, gr.RefGP(X, Y, .1, fam, w, sf2), orc.GP(orc.Kern(kind, hyper), X, Y, noise=.1)


def candidates(X, Y, seed=9):
    """near the eight best observations: places where EI is not negligible, so that every standard error is a positive number"""
    rs = np.random.RandomState(seed)
    return X[np.argsort(Y)[-8:]] + .08 * rs.randn(8, 3)


@pytest.mark.parametrize("kind,hyper", MODELS)
def test_no_pending_points_against_the_oracles_ei(kind, hyper):
    """S = 2^16 seeded iid draws: |qEI - EI| within 5 standard errors (std of the sample's terms / sqrt(S)) at every candidate.
    Worst ratio as run when this test was written (the seed is fixed): ard 0.67, sviso 0.67, m3 0.70, m5 0.68."""
    X, Y, ref, ogp = small_model(kind, hyper)
    Q = candidates(X, Y)
    t = float(np.max(Y)) + qr.XI
    Z = qr.samples(1 << 16, 1, seed=21)
    w = qr.qei(ref, np.empty((0, 3)), Q, Z, t)
    mu, s2 = ogp.posteriors(Q)
    ei = orc.acq_value(orc.ACQ_EI, orc.ERF_LIBM, mu, np.sqrt(s2), float(np.max(Y)), qr.XI)
    se = np.std(w["terms"], axis=1, ddof=1) / np.sqrt(Z.shape[0])
    assert np.all(se > 0) and np.all(ei > 1e-6)
    ratio = np.abs(w["qei"] - ei) / se
    print("%s: qEI(p = 0) against the oracle's EI, worst |difference| / standard error = %.3g" % (kind, float(np.max(ratio))))
    assert np.all(ratio <= 5.0), ratio
    assert w["base"] == 0.0


@pytest.mark.parametrize("kind,hyper", MODELS[::3])
@pytest.mark.parametrize("p", [1, 3])
def test_pending_points_against_a_refit_of_the_oracle(kind, hyper, p):
    """max(max(f, g) - t, 0) = max(g - t, 0) + max(f - max(t, g), 0), and the expectation of the last term over the candidate's own
    draw is the EI of the model refitted with the pending observations y_P against the incumbent max(t, g) -- computed by the oracle
    from (X + P, Y + y_P), which knows nothing of l and d.  The mean over the draws of the per-draw difference must vanish within
    5 of its standard errors.  Worst ratio as run when this test was written (the seed is fixed): 1.9 (p = 1), 1.2 (p = 3)."""
    X, Y, ref, ogp = small_model(kind, hyper)
    Q = candidates(X, Y)
    P = X[np.argsort(Y)[-p:]] + .05                        # near the best observations: g exceeds t in part of the draws
    t = float(np.max(Y)) + qr.XI
    S = 1500
    Z = qr.samples(S, p + 1, seed=22)
    w = qr.qei(ref, P, Q, Z, t)
    yP = w["mu_pend"] + Z[:, :p] @ w["L_pend"].T
    g = np.max(yP, axis=1)
    diff = np.empty((len(Q), S))
    for s in range(S):
        o2 = orc.GP(orc.Kern(kind, hyper), np.r_[X, P], np.r_[Y, yP[s]], noise=.1)
        mu, s2 = o2.posteriors(Q)
        ei = orc.acq_value(orc.ACQ_EI, orc.ERF_LIBM, mu, np.sqrt(s2), max(t, g[s]), 0.0)
        diff[:, s] = max(g[s] - t, 0.0) + ei - w["terms"][:, s]
    se = np.std(diff, axis=1, ddof=1) / np.sqrt(S)
    ratio = np.abs(np.mean(diff, axis=1)) / se
    print("%s, p = %d: refit identity, worst |mean difference| / standard error = %.3g (largest qEI %.3g, base %.3g)" %
          (kind, p, float(np.max(ratio)), float(np.max(w["qei"])), w["base"]))
    assert np.all(ratio <= 5.0), ratio
    assert np.max(w["qei"]) > w["base"] > 0


def test_compose_against_the_whole_matrix_route_and_long_double():
    """On the pieces of every case of the GPU test (at most 48 candidates of each): `compose` (the ABI's bordering) against `qei`
    (the whole matrix factored) and against its own long-double evaluation, as shares of the GPU bar 1e-12 scale.  Worst shares as run
    when this test was written: against the whole-matrix route 8.9e-5, against long double 1.2e-4."""
    worst_q = worst_l = 0.0
    for case in qr.CASES:
        X, Y, hyper, pr, ref, P, Q, Z, t = qr.case_inputs(case)
        Q = Q[::max(1, len(Q) // 48)][:48]
        w = qr.qei(ref, P, Q, Z, t)
        v, scale = qr.compose(w["mu_pend"], w["S_pend"], w["mu"], w["s2"], w["c"], Z, t)
        vl, _ = qr.compose(w["mu_pend"], w["S_pend"], w["mu"], w["s2"], w["c"], Z, t, dtype=np.longdouble)
        a = float(np.max(np.abs(v - w["qei"]) / (1e-12 * scale))); b = float(np.max(np.abs(v - vl) / (1e-12 * scale)))
        print(case, "compose against the whole-matrix route %.2g of the bar, against long double %.2g" % (a, b))
        worst_q = max(worst_q, a); worst_l = max(worst_l, b)
    print("worst share of 1e-12 scale: whole-matrix route %.3g, long double %.3g" % (worst_q, worst_l))
    assert worst_q <= 0.1 and worst_l <= 0.1


def lane_order_mean(terms):
    """the device's order: lane l sums the samples l, l + 64, .. in ascending order (terms > 0 only), then the butterfly, then / S"""
    v = np.zeros(64)
    for s, x in enumerate(terms):
        if x > 0:
            v[s & 63] += x
    for o in (32, 16, 8, 4, 2, 1):
        v = v + v[np.arange(64) ^ o]
    return v[0] / len(terms)


def test_values_are_at_least_base_exactly_in_one_summation_order():
    """Termwise max(f, g) - t >= g - t in floating point (subtraction is monotone), a sum in a FIXED order is monotone in every term,
    and so is the division: summed in the same order, a value can never fall below base -- not by one bit.  That is the reason base is
    summed in the candidates' order (lanes, butterfly) and not by a simpler loop: with two different orders the property fails, as the
    last assertion shows on the same terms."""
    rs = np.random.RandomState(4)
    fails_mixed = 0
    for trial in range(200):
        S = int(rs.choice([1, 63, 64, 65, 1000]))
        g = rs.randn(S) * rs.choice([1e-3, 1.0]); t = rs.randn() * .3
        f = g + rs.randn(S) * rs.choice([1e-17, 1e-9, 1.0])             # mostly a hair above or below g
        base = lane_order_mean(g - t)
        val = lane_order_mean(np.maximum(f, g) - t)
        assert val >= base
        plain = 0.0
        for x in np.maximum(g - t, 0.0):
            plain += x
        fails_mixed += val < plain / S
    assert lane_order_mean(np.array([-1.0, -2.0])) == 0.0
    assert fails_mixed > 0


def test_the_python_tests_antithetic_seed():
    """tests/test_gpu_qei.py::test_python_layer holds ParallelEI(pending=None) with baseSamples(1, 4096, seed=0) to EI within 5 standard
    errors; here the same model, candidates and draws through the restatement against the closed form.  Worst ratio as run when this
    test was written: 1.4."""
    from scipy.special import erf
    from ibo_amd.acquisition import baseSamples
    X, Y, hyper, pr, ref = qr.kr.case_ref("sviso", 3, 30, True)
    Q = qr.ei_candidates(X, Y)
    t = float(np.max(Y)) + qr.XI
    Z = baseSamples(1, 4096, seed=0)
    w = qr.qei(ref, np.empty((0, 3)), Q, Z, t)
    sd = np.sqrt(w["s2"]); z = (w["mu"] - t) / sd
    ei = (w["mu"] - t) * .5 * (1 + erf(z / np.sqrt(2))) + sd * np.exp(-z * z / 2) / np.sqrt(2 * np.pi)
    ratio = qr.antithetic_ratio(w["mu"], w["s2"], Z, t, w["qei"], ei)
    print("4096 antithetic draws, seed 0: worst |qEI - EI| / standard error = %.3g" % float(np.max(ratio)))
    assert np.all(ratio <= 5.0)


def test_symbols_are_declared_exported_and_bound():
    from ibo_amd import _lib
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ibo_abi.h")).read(), flags=re.S)
    for s in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % s, txt), "%s is not declared in ibo_abi.h" % s
        assert hasattr(_lib.lib, s), "libibo_hip.so does not export %s" % s
        assert s in _lib.EXPORTED
    assert re.search(r"#define\s+IBO_QEI_MAX_PENDING\s+15\b", txt) and re.search(r"#define\s+IBO_QEI_MAX_SAMPLES\s+4096\b", txt)
    assert re.search(r"#define\s+IBO_ABI_VERSION\s+8\b", txt)
    from ibo_amd.acquisition import baseSamples, ParallelEI, sweepQEI, maximizeQEI, jointQEI, proposeBatch      # noqa: F401
    Z = baseSamples(3, 8, seed=1)
    assert Z.shape == (8, 3) and np.array_equal(Z[4:], -Z[:4]) and np.array_equal(Z, baseSamples(3, 8, seed=1))
    assert not np.array_equal(baseSamples(3, 8, seed=1, antithetic=False)[4:], -Z[:4])
    for bad in (lambda: baseSamples(0), lambda: baseSamples(2, 4097), lambda: baseSamples(2, 7)):
        with pytest.raises(ValueError):
            bad()
    assert _lib.lib.ibo_set_option(b"qei_chunk", 0) == _lib.OK and _lib.lib.ibo_set_option(b"qei_chunk", -1) == _lib.ERR_ARG
    if _lib.device_count() > 0:
        return                                       # (tests/test_gpu_qei.py takes over where a GPU is visible)
    A = _lib.f64(np.zeros((2, 3))); Zs = _lib.f64(np.zeros((4, 3))); out = np.empty(6); lb = _lib.f64(np.zeros(3)); ub = _lib.f64(np.ones(3))
    bv = ctypes.c_double(); bi = ctypes.c_int64(); info = ctypes.c_int()
    L = _lib.lib
    head = (None, 2, _lib.dp(A), 4, _lib.dp(Zs), float("nan"), 0.0, 1e-7, 0.0)
    assert L.ibo_qei_sweep(*(head + (2, None, 0, None, None, ctypes.byref(bv), ctypes.byref(bi), ctypes.byref(info)))) == _lib.ERR_NO_DEVICE
    assert L.ibo_qei_batch(*(head + (2, _lib.dp(A), _lib.dp(out), None, None, None, None, None, None, None))) == _lib.ERR_NO_DEVICE
    assert L.ibo_qei_direct_max(*(head + (3, _lib.dp(lb), _lib.dp(ub), 5, 5, 100, 0, ctypes.byref(bv), _lib.dp(out), None, None))) == _lib.ERR_NO_DEVICE

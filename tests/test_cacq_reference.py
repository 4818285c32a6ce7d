"""
The NumPy restatement of the constrained acquisition (tests/cacq_reference.py, the yardstick of tests/test_gpu_constrained.py)
pinned to the oracle per model, its gradient checked against central differences of its own values, the generator of the GPU
comparison checked for being worth comparing on, and the four ibo_cacq_* symbols.  CPU only.
"""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT, synth
from oracle import oracle as orc
import grad_reference as gr
import cacq_reference as cr

KERNELS = [("ard", [.3, .5, .4]), ("iso", [.4]), ("sviso", [.4, .8]), ("m3", [.5, .95]), ("m5", [.5, 0.9])]
SYMBOLS = ("ibo_cacq_sweep", "ibo_cacq_batch", "ibo_cacq_grad_batch", "ibo_cacq_direct_max")


def three_models(kind, hyper, with_prior=False):
    """an objective and two constraint models observed at OTHER points, as (oracle GP, restatement) pairs"""
    out = []
    for seed, N in ((5, 40), (6, 33), (7, 25)):
        X, Y = synth(seed, N, 3)
        prior = oprior = None
        if with_prior and seed == 5:
            rs = np.random.RandomState(7)
            prior = (rs.rand(4, 3), rs.randn(4), 2.0, np.zeros(3) - .1, np.full(3, 1.2))
            oprior = orc.Prior(*prior)
        out.append((orc.GP(orc.Kern(kind, hyper), X, Y, noise=.1, prior=oprior), cr.make(X, Y, .1, kind, hyper, prior=prior)))
    out[1][1].thresh, out[1][1].sense = 0.3, 1
    out[2][1].thresh, out[2][1].sense = -0.2, -1
    return out


@pytest.mark.parametrize("with_prior", [False, True])
@pytest.mark.parametrize("kind,hyper", KERNELS)
def test_per_model_numbers_equal_the_oracles(kind, hyper, with_prior):
    """mu to 1e-9 absolute, s2 / EI / PI to 1e-6 relative: the oracle's own bars"""
    Q = np.random.RandomState(3).rand(40, 3) * 1.2 - .1
    for ogp, m in three_models(kind, hyper, with_prior):
        mu, s2 = ogp.posteriors(Q)
        rmu, rs2 = cr.posterior(m, Q, 1e-7)
        np.testing.assert_allclose(rmu, mu, rtol=0, atol=1e-9)
        np.testing.assert_allclose(rs2, s2, rtol=1e-6, atol=0)
        ymax = float(np.max(ogp.Y))
        for acq in (gr.ACQ_EI, gr.ACQ_PI):
            for erf_mode in (gr.ERF_LIBM, gr.ERF_NR):
                want = orc.acq_value(acq, erf_mode, mu, np.sqrt(s2), ymax, 0.01)
                got = cr.acq_value(acq, erf_mode, rmu, np.sqrt(rs2), ymax, 0.01)
                np.testing.assert_allclose(got, want, rtol=1e-6, atol=1e-300)


@pytest.mark.parametrize("erf_mode", [gr.ERF_LIBM, gr.ERF_NR])
def test_one_constraint_is_ei_times_phi_exactly_as_composed(erf_mode):
    (ogp, obj), (_, c1), _ = three_models("m5", [.5, .9])
    Q = np.random.RandomState(4).rand(50, 3)
    r = cr.value(obj, [c1], Q, gr.ACQ_EI, 0.01, erf_mode, 1e-7)
    mu, s2 = cr.posterior(obj, Q, 1e-7)
    ei = cr.acq_value(gr.ACQ_EI, erf_mode, mu, np.sqrt(s2), float(np.max(ogp.Y)), 0.01)
    cmu, cs2 = cr.posterior(c1, Q, 1e-7)
    phi = gr.cdf_pdf(erf_mode, (c1.thresh - cmu) / np.sqrt(cs2))[0]
    assert np.array_equal(r["val"], ei * phi) and np.array_equal(r["acq"], ei) and np.array_equal(r["pof"], phi)
    assert np.all(phi > 0) and np.all(phi < 1) and np.ptp(phi) > 0.1
    # two constraints: the order A, Phi_0, Phi_1; ACQ_NONE: A = 1; no constraint: the plain acquisition
    (_, obj), (_, c1), (_, c2) = three_models("m5", [.5, .9])
    r2 = cr.value(obj, [c1, c2], Q, gr.ACQ_EI, 0.01, erf_mode, 1e-7)
    assert np.array_equal(r2["val"], (ei * r2["phis"][0]) * r2["phis"][1])
    r3 = cr.value(obj, [c1, c2], Q, gr.ACQ_NONE, 0.0, erf_mode, 1e-7)
    assert np.array_equal(r3["val"], r2["pof"]) and np.all(r3["acq"] == 1.0)
    assert np.array_equal(cr.value(obj, [], Q, gr.ACQ_EI, 0.01, erf_mode, 1e-7)["val"], ei)


@pytest.mark.parametrize("acq", [gr.ACQ_EI, gr.ACQ_PI, gr.ACQ_NONE])
@pytest.mark.parametrize("kind,hyper", KERNELS)
def test_gradient_matches_central_differences_of_the_restatement(kind, hyper, acq):
    """h = 1e-5, agreement 1e-6 of the scale; the libm flavour only (NR's truncated constants make the analytic gradient differ
    from the derivative of the values by about 1e-6, see ibo_abi.h)"""
    (_, obj), (_, c1), (_, c2) = three_models(kind, hyper, with_prior=True)
    cons = [c1, c2, cr.Model(c1.ref, thresh=-0.4, sense=-1)]        # the third: a band on the first model
    Q = np.random.RandomState(8).rand(10, 3)
    g = cr.value_grad(obj, cons, Q, acq, 0.01, gr.ERF_LIBM, 1e-7)
    # (per-point sums here, matrix products there: the last bits differ)
    np.testing.assert_allclose(g["val"], cr.value(obj, cons, Q, acq, 0.01, gr.ERF_LIBM, 1e-7)["val"], rtol=1e-11, atol=0)
    h = 1e-5
    num = np.zeros(Q.shape)
    for d in range(Q.shape[1]):
        E = np.zeros(Q.shape); E[:, d] = h
        num[:, d] = (cr.value(obj, cons, Q + E, acq, 0.01, gr.ERF_LIBM, 1e-7)["val"] -
                     cr.value(obj, cons, Q - E, acq, 0.01, gr.ERF_LIBM, 1e-7)["val"]) / (2 * h)
    assert np.max(np.abs(g["dval"])) > 1e-3
    gr.assert_grad_close(g["dval"], num, g["sval"], rel=1e-6, atol=1e-13, what="%s acq=%d" % (kind, acq))


def test_generator_is_worth_comparing_on():
    """In each of the three cases at least 25 % of the 3000 candidates have a reference val > 1e-6 (else the GPU comparison would
    mostly compare zeros), and in at least two cases the constrained arg-max differs from the unconstrained EI arg-max (else it
    would not notice missing constraints)."""
    moved = 0
    for case in cr.GEN_CASES:
        g = cr.generator(*case)
        share = float(np.mean(g["ref"]["val"] > 1e-6))
        print("generator %s: share of val > 1e-6 = %.3f, arg-max %d (EI alone: %d)" %
              (case, share, int(np.argmax(g["ref"]["val"])), int(np.argmax(g["ref"]["acq"]))))
        assert share >= 0.25, (case, share)
        assert np.all(np.isfinite(g["ref"]["val"]))
        moved += int(np.argmax(g["ref"]["val"]) != np.argmax(g["ref"]["acq"]))
    assert moved >= 2


def test_symbols_are_declared_exported_and_bound():
    from ibo_amd import _lib
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ibo_abi.h")).read(), flags=re.S)
    for s in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % s, txt), "%s is not declared in ibo_abi.h" % s
        assert hasattr(_lib.lib, s), "libibo_hip.so does not export %s" % s
        assert s in _lib.EXPORTED
    assert re.search(r"#define\s+IBO_CACQ_MAX_CON\s+8\b", txt)
    assert _lib.lib.ibo_abi_version() == 8
    if _lib.device_count() > 0:
        return                                       # (tests/test_gpu_constrained.py takes over where a GPU is visible)
    Q = _lib.f64(np.zeros((2, 3))); out = np.empty(6); lb = _lib.f64(np.zeros(3)); ub = _lib.f64(np.ones(3))
    bv = ctypes.c_double(); bi = ctypes.c_int64()
    L = _lib.lib
    nan = float("nan")
    assert L.ibo_cacq_sweep(None, 0, None, None, None, 2, None, 0, .01, 0, 1e-8, nan, 0, None, .5, 0, None, None, None,
                            ctypes.byref(bv), ctypes.byref(bi)) == _lib.ERR_NO_DEVICE
    assert L.ibo_cacq_batch(None, 0, None, None, None, 2, _lib.dp(Q), 0, .01, 0, 1e-8, nan, None, None, _lib.dp(out)) == _lib.ERR_NO_DEVICE
    assert L.ibo_cacq_grad_batch(None, 0, None, None, None, 2, _lib.dp(Q), 0, .01, 0, 1e-8, nan, _lib.dp(out), None) == _lib.ERR_NO_DEVICE
    assert L.ibo_cacq_direct_max(None, 0, None, None, None, 3, _lib.dp(lb), _lib.dp(ub), 0, .01, 0, 1e-8, nan, 5, 5, 100, 1,
                                 ctypes.byref(bv), _lib.dp(out), None) == _lib.ERR_NO_DEVICE

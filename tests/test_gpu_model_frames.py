"""
What the model side of the C ABI keeps between calls -- the likelihood gradients' resident data and workspace, the gradient-observation
fit's frame, the sparse model's stage sums -- must never show in a result: every call returns the bits of the same call on a fresh
workspace (the one ibo_trim leaves behind).  Data: a fixed RandomState, noise 0.05, SE-ARD, D = 2 (model_frames_calls.py).
"""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def mf():
    import model_frames_calls as calls
    if calls._lib.device_count() < 1:
        pytest.fail("no GPU visible: the product has no CPU fallback")
    return calls


def fresh(mf, entry, *args):
    assert mf.trim() == mf._lib.OK
    return mf.bits(entry(*args))


@pytest.mark.parametrize("which", range(3), ids=["ibo_nlml_grad", "ibo_loo_grad", "ibo_ggp_nlml_grad"])
def test_resident_data_never_show_in_a_result(mf, which):
    """same data / another theta / changed Y / changed X / fewer rows in the same frame (the mirror's tail is stale) / more rows / back"""
    name, entry, sizes = mf.RESIDENT[which]
    mf.trim()
    for label, X, Y, G, ell in mf.resident_steps(*sizes):
        got = mf.bits(entry(X, Y, G, ell))
        assert got == fresh(mf, entry, X, Y, G, ell), "%s, step '%s': not the bits of a fresh workspace" % (name, label)


def test_plain_and_gradient_model_keep_their_data_apart(mf):
    X, Y, _ = mf.data(70)
    gX, gY, gG = mf.data(22, seed=9)
    mf.trim()
    mf.nlml_grad(X, Y, None, mf.THETA1); mf.ggp_nlml_grad(gX, gY, gG, mf.THETA1)
    got = mf.bits(mf.nlml_grad(X, Y, None, mf.THETA2))
    assert got == fresh(mf, mf.nlml_grad, X, Y, None, mf.THETA2)
    mf.ggp_nlml_grad(gX, gY, gG, mf.THETA1); mf.loo_grad(X, Y, None, mf.THETA1)
    got = mf.bits(mf.ggp_nlml_grad(gX, gY, gG, mf.THETA2))
    assert got == fresh(mf, mf.ggp_nlml_grad, gX, gY, gG, mf.THETA2)


@pytest.mark.parametrize("name", ["nlml_grad", "loo_grad", "ggp_nlml_grad", "nlml_grid", "sgp_nlml_grad"])
def test_trim_after_every_entry_and_the_same_bits_again(mf, name):
    entry = getattr(mf, name)
    X, Y, G = mf.data(22 if name == "ggp_nlml_grad" else 70)
    before = mf.bits(entry(X, Y, G))
    assert mf.trim() == mf._lib.OK
    assert mf.bits(entry(X, Y, G)) == before
    assert mf.trim() == mf._lib.OK


def test_gradient_fit_fails_and_recovers_like_a_plain_fit(mf):
    """noise = -2: the diagonal is -1 and the FIRST pivot fails by construction"""
    L = mf._lib
    X, Y, G = mf.data(22)
    Q = mf.f64(X[:3] + .05)
    h = mf.Ggp()
    rc = h.fit(X, Y, G, noise=-2.0)
    assert rc == L.ERR_NOT_PD and h.info.value == 1
    assert b"gradient-observation matrix is not positive definite" in L.lib.ibo_last_error()
    assert h.L()[0] == L.ERR_STATE and h.batch(Q)[0] == L.ERR_STATE
    bv = ctypes.c_double()
    lb, ub = mf.f64(np.zeros(mf.D)), mf.f64(np.ones(mf.D))
    assert L.lib.ibo_ggp_direct_max(h.h, mf.D, mf.dp(lb), mf.dp(ub), 0, .01, 0, 1e-8, 5, 30, 1000, 1, ctypes.byref(bv), None, None) == L.ERR_STATE
    cand = L.DeviceArray.from_host(Q)
    assert L.lib.ibo_ggp_acq_sweep(h.h, len(Q), cand.ptr, 0, .01, 0, 1e-8, float("nan"), 0, None, None, None, ctypes.byref(bv), None) == L.ERR_STATE
    L.check(h.fit(X, Y, G))
    other = mf.Ggp()
    L.check(other.fit(X, Y, G))
    (rc1, L1), (rc2, L2) = h.L(), other.L()
    assert rc1 == L.OK and rc2 == L.OK and L1.tobytes() == L2.tobytes()
    assert mf.bits(h.batch(Q)[1:]) == mf.bits(other.batch(Q)[1:])


@pytest.mark.parametrize("which", ["ibo_sgp_stage_ms", "ibo_sgp_grad_stage_ms"])
def test_sparse_stage_sums(mf, which):
    """zero while the option is off; with it on: never negative, positive in the stages a FITC gradient call runs (the fit's five and, of
    the gradient's, all eight -- the signed Gram product is not DTC's), returned and cleared by reset = 1; the results' bits do not depend
    on the option"""
    L = mf._lib
    read = getattr(L.lib, which)
    ran = range(5) if which == "ibo_sgp_stage_ms" else range(8)
    X, Y, _ = mf.data(300)
    ms = np.full(mf.STAGES[which], -1.0)
    L.check(read(mf.dp(ms), 1))
    off = mf.bits(mf.sgp_nlml_grad(X, Y))
    L.check(read(mf.dp(ms), 0))
    assert np.all(ms == 0.0)
    L.check(L.lib.ibo_set_option(b"sgp_timing", 1))
    try:
        on = mf.bits(mf.sgp_nlml_grad(X, Y))
    finally:
        L.check(L.lib.ibo_set_option(b"sgp_timing", 0))
    L.check(read(mf.dp(ms), 1))
    assert np.all(ms >= 0.0) and all(ms[k] > 0.0 for k in ran), ms
    again = np.full(mf.STAGES[which], -1.0)
    L.check(read(mf.dp(again), 0))
    assert np.all(again == 0.0)
    assert on == off

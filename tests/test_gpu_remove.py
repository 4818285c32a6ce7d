"""
Removal of observations from a fitted model on the device (ibo_gp_remove, GaussianProcess.removeData; csrc/downdate.hip).

Yardsticks: numpy.linalg.cholesky / inv of the reduced R for the factor (1e-9 of max|.|: the project's usual bar, ten times the CPU pin of
tests/test_downdate_reference.py), and a FRESH model fitted on the remaining data for everything that reads the handle, at the bars those
readers' own test files use:
    values (mu, s2, EI / PI / UCB)   1e-6 relative, 1e-9 absolute (the parity bar)
    posterior_gradient               1e-9 sum_i |dk*_i c_i| + 1e-13 per entry   (grad_reference.assert_grad_close)
    posterior_cov                    1e-10 (sf2 + noise + |v_a| |v_b|)           (cov_reference.assert_cov_close)
    loo                              mu 1e-9 (|Y_i| + |c_i| / d_i), s2 1e-9 relative
    the sweep's arg-max              the same index, or two indices whose values on the fresh model agree to 1e-12 relative
Every factor case asserts cond_2(R) <= 1e6 first: a bar is never met by an ill-posed input.  No test tries to make the device fail.
"""
import ctypes

import numpy as np
import pytest

import cov_reference as cr
import downdate_reference as dr
import grad_reference as gr
import loo_reference as lr
from conftest import synth
from oracle import oracle as orc
from test_gpu_linalg_entries import option
from wall_time import wall

pytestmark = pytest.mark.gpu

BASE = {"iso": [.45], "sviso": [.45, .8], "m3": [.5, .95], "m5": [.5, .9]}
NOISE = .1


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


def new_gp(kind, D, X, Y, prior=False, **kw):
    from ibo_amd.gaussianprocess import GaussianProcess
    return GaussianProcess(make_kernel(kind, hyper_of(kind, D)), X, Y, prior=make_prior(D) if prior else None, noise=NOISE, **kw)


def get_W(lib, GP):
    N = len(GP.X)
    W = np.empty((N, N))
    lib.check(lib.lib.ibo_gp_get_W(GP._handle(), lib.dp(W)))
    return W


def ref_R(kind, D, X):
    return orc.GP(orc.Kern(kind, hyper_of(kind, D)), X, np.zeros(len(X)), noise=NOISE).R


def cond_of(R, how):
    """cond_2 of the symmetric positive definite R: by SVD; from its eigenvalues (the same number, cheaper); or "bound": the bound
    N (1 + noise) / noise, which needs no decomposition -- R = sf2 K + (1 + noise - sf2) I with K positive semi-definite and sf2 <= 1, so
    lambda_min >= noise, and lambda_max <= trace(R) = N (1 + noise).  The bound reads the noise off R's diagonal and asserts sf2 <= 1."""
    if how == "svd":
        return dr.cond2(R)
    if how == "eigvalsh":
        w = np.linalg.eigvalsh(R)
        return w[-1] / w[0]
    assert how == "bound"
    noise = R[0, 0] - 1.0
    assert noise > 0 and np.all(np.diag(R) == R[0, 0]) and np.max(np.abs(R - np.diag(np.diag(R)))) <= 1.0
    return len(R) * (1.0 + noise) / noise


def check_factor(lib, GP, kind, D, what="", cond="svd", R=None, max_cond=1e6):
    """GP's L, W and R against NumPy's of the matrix of the points it holds now (R: that matrix, where the model is not one of new_gp's;
    cond: how cond_2 is found, see cond_of; max_cond None: no precondition -- the caller says why)"""
    if R is None:
        R = ref_R(kind, D, GP.X)
    c = cond_of(R, cond)
    assert max_cond is None or c <= max_cond, (what, c)
    Lref = np.linalg.cholesky(R)
    Wref = np.linalg.inv(Lref)
    L, W = GP.L, get_W(lib, GP)
    assert L.shape == Lref.shape
    eL, eW = dr.relerr(L, Lref), dr.relerr(W, Wref)
    print("%s: N=%d cond %.3g  L err %.3g  W err %.3g" % (what, len(GP.X), c, eL, eW))
    assert eL <= 1e-9 and eW <= 1e-9, (what, eL, eW)
    assert np.array_equal(L, np.tril(L)) and np.array_equal(W, np.tril(W)), what
    np.testing.assert_allclose(GP.R, R, rtol=1e-12, atol=0, err_msg=what)
    return eL, eW


def values_close(a, b, what=""):
    np.testing.assert_allclose(a, b, rtol=1e-6, atol=1e-9, err_msg=what)


def check_like_fresh(GP, kind, D, prior=False, what="", M=64):
    """posterior of GP against a fresh model on the data it holds now (a batch of <= 16 points, and M)"""
    fr = new_gp(kind, D, GP.X, GP.Y, prior=prior)
    Q = np.random.RandomState(5).rand(M, D) * 1.2 - .1
    for q in (Q[:9], Q):
        (m1, v1), (m0, v0) = GP.posteriors(q), fr.posteriors(q)
        values_close(m1, m0, what + " mu"); values_close(v1, v0, what + " s2")
    return fr


def prior_tuple(GP):
    p = GP.prior
    return None if p is None else (p.means, p.beta, p.theta, p.lowerb, p.width)


def check_loo_like_fresh(GP, fr, kind, D, what=""):
    """leave-one-out predictions and score against the fresh model's, at the bars of tests/test_gpu_loo.py"""
    pt = prior_tuple(GP)
    lref = lr.handle_loo(orc.GP(orc.Kern(kind, hyper_of(kind, D)), GP.X, GP.Y, noise=NOISE, prior=None if pt is None else orc.Prior(*pt)))
    assert lref["cond"] <= 1e6
    (lm1, ls1), (lm0, ls0) = GP.loo(), fr.loo()
    assert np.all(np.abs(lm1 - lm0) <= 1e-9 * (np.abs(GP.Y) + np.abs(lref["c"]) / lref["d"])), what
    assert np.all(np.abs(ls1 - ls0) <= 1e-9 * ls0), what
    assert abs(GP.loo_score() - fr.loo_score()) <= 1e-9 * (len(GP.Y) + abs(lref["value"])), what


def check_readers_like_fresh(GP, fr, kind, D, what=""):
    """gradients, joint covariance and leave-one-out of GP against the fresh model `fr` on the same data and prior: the checks and bars of
    test_readers_of_the_handle_agree_with_a_fresh_model below, for callers that drive a handle through more than one step"""
    hyper = hyper_of(kind, D)
    fam, w, sf2 = gr.kernel_spec(kind, hyper, D)
    ref = gr.RefGP(GP.X, GP.Y, NOISE, fam, w, sf2, prior=prior_tuple(GP))
    Q = np.random.RandomState(6).rand(64, D) * 1.2 - .1
    Q[:4] = GP.X[[0, len(GP.X) - 1, len(GP.X) // 2, len(GP.X) // 3]]             # on top of training inputs
    rg = ref.grad(Q)
    m1, v1, dm1, dv1 = GP.posterior_gradient(Q)
    m0, v0, dm0, dv0 = fr.posterior_gradient(Q)
    values_close(m1, m0, what); values_close(v1, v0, what)
    gr.assert_grad_close(dm1, dm0, rg["smu"], what=what + " dmu")
    gr.assert_grad_close(dv1, dv0, rg["ss2"], what=what + " ds2")
    (mc1, S1), (mc0, S0) = GP.posterior_cov(Q), fr.posterior_cov(Q)
    values_close(mc1, mc0, what)
    cr.assert_cov_close(S1, S0, cr.cov(ref, Q)[1], sf2, NOISE, what=what + " Sigma")
    assert np.array_equal(S1, S1.T)
    check_loo_like_fresh(GP, fr, kind, D, what)


# ---------------------------------------------------------------------------------------------------------------- 1. the factor
FACTOR_CASES = [("ard", 2, 1), ("ard", 3, 4), ("ard", 63, 33), ("ard", 64, 1), ("ard", 65, 4), ("ard", 128, 33), ("ard", 129, 4), ("ard", 200, 1),
                ("iso", 129, 1), ("svard", 129, 33), ("sviso", 129, 4), ("m3", 129, 1), ("m5", 129, 33)]


@pytest.mark.parametrize("kind,N,D", FACTOR_CASES)
def test_factor_after_one_removal(lib, kind, N, D):
    X, Y = synth(N + D, N, D)
    for i in sorted({r for r in (0, N - 1, 63, 64, N // 2) if r < N}):
        GP = new_gp(kind, D, X, Y)
        Rb = GP.R.copy()                                     # formed before the removal: it must be formed again after it
        GP.removeData(i, _route="device")
        keep = np.r_[0:i, i + 1:N]
        assert len(GP.X) == N - 1 and np.array_equal(GP.X, X[keep]) and np.array_equal(GP.Y, Y[keep])
        n = ctypes.c_int(); my = ctypes.c_double()
        lib.check(lib.lib.ibo_gp_info(GP._handle(), ctypes.byref(n), None, None, ctypes.byref(my)))
        assert n.value == N - 1 and my.value == Y[keep].max()
        check_factor(lib, GP, kind, D, "%s N=%d D=%d i=%d" % (kind, N, D, i))
        np.testing.assert_allclose(GP.R, Rb[np.ix_(keep, keep)], rtol=1e-12, atol=0)


# ---------------------------------------------------------------------------------------------------------------- 2. everything that reads the handle
READ_CASES = [("ard", 65, 4, 0, False), ("m5", 129, 33, 64, False), ("svard", 200, 1, 100, True), ("m3", 64, 4, 63, True),
              ("ard", 1025, 4, 3, False)]


@pytest.mark.parametrize("kind,N,D,i,prior", READ_CASES)
def test_readers_of_the_handle_agree_with_a_fresh_model(lib, kind, N, D, i, prior):
    from ibo_amd import DeviceArray
    from ibo_amd.acquisition import sweep
    X, Y = synth(N + D + 1, N, D)
    GP = new_gp(kind, D, X, Y, prior=prior)
    GP.removeData(i, _route="device")
    what = "%s N=%d D=%d i=%d" % (kind, N, D, i)
    fr = check_like_fresh(GP, kind, D, prior=prior, what=what, M=300)
    hyper = hyper_of(kind, D)
    # sweeps over a device candidate array: EI / PI / UCB, per-candidate outputs and the arg-max
    dc = DeviceArray.from_host(np.random.RandomState(9).rand(4096, D))
    for acq in ("ei", "pi", "ucb"):
        r = sweep(GP, dc, acq=acq, native=False, outputs=("mu", "s2", "acq"))
        f = sweep(fr, dc, acq=acq, native=False, outputs=("mu", "s2", "acq"))
        print("%s %s: %s (fresh model: %s)" % (what, acq, r["kernel"], f["kernel"]))
        for k in ("mu", "s2", "acq"):
            values_close(r[k], f[k], "%s %s %s" % (what, acq, k))
        a, b = f["acq"][r["best_idx"]], f["acq"][f["best_idx"]]
        assert r["best_idx"] == f["best_idx"] or abs(a - b) <= 1e-12 * abs(b), (what, acq, r["best_idx"], f["best_idx"], a, b)
    if N > 1024:                                             # above the small-batch route: the full sweep (its second panel of W's rows, the repacked Wp)
        big = DeviceArray.from_host(np.random.RandomState(10).rand(9001, D))
        r = sweep(GP, big, acq="ei", native=False, outputs=("mu", "s2", "acq"))
        f = sweep(fr, big, acq="ei", native=False, outputs=("mu", "s2", "acq"))
        print("%s 9001 candidates: %s (fresh model: %s)" % (what, r["kernel"], f["kernel"]))
        assert r["kernel"].startswith("sweep2"), r["kernel"]
        for k in ("mu", "s2", "acq"):
            values_close(r[k], f[k], "%s 9001 %s" % (what, k))
        a, b = f["acq"][r["best_idx"]], f["acq"][f["best_idx"]]
        assert r["best_idx"] == f["best_idx"] or abs(a - b) <= 1e-12 * abs(b), (what, r["best_idx"], f["best_idx"], a, b)
    # gradients, joint covariance: the bars of their own test files, scaled by the NumPy reference of the remaining data
    pt = None if not prior else (GP.prior.means, GP.prior.beta, GP.prior.theta, GP.prior.lowerb, GP.prior.width)
    fam, w, sf2 = gr.kernel_spec(kind, hyper, D)
    ref = gr.RefGP(GP.X, GP.Y, NOISE, fam, w, sf2, prior=pt)
    Q = np.random.RandomState(6).rand(64, D) * 1.2 - .1
    Q[:4] = GP.X[[0, len(GP.X) - 1, max(i - 1, 0), min(i, len(GP.X) - 1)]]      # on top of training inputs, the removed row's neighbours among them
    rg = ref.grad(Q)
    m1, v1, dm1, dv1 = GP.posterior_gradient(Q)
    m0, v0, dm0, dv0 = fr.posterior_gradient(Q)
    values_close(m1, m0, what); values_close(v1, v0, what)
    gr.assert_grad_close(dm1, dm0, rg["smu"], what=what + " dmu")
    gr.assert_grad_close(dv1, dv0, rg["ss2"], what=what + " ds2")
    (mc1, S1), (mc0, S0) = GP.posterior_cov(Q), fr.posterior_cov(Q)
    values_close(mc1, mc0, what)
    cr.assert_cov_close(S1, S0, cr.cov(ref, Q)[1], sf2, NOISE, what=what + " Sigma")
    assert np.array_equal(S1, S1.T)
    # leave-one-out
    op = None if not prior else orc.Prior(*pt)
    lref = lr.handle_loo(orc.GP(orc.Kern(kind, hyper), GP.X, GP.Y, noise=NOISE, prior=op))
    assert lref["cond"] <= 1e6
    (lm1, ls1), (lm0, ls0) = GP.loo(), fr.loo()
    assert np.all(np.abs(lm1 - lm0) <= 1e-9 * (np.abs(GP.Y) + np.abs(lref["c"]) / lref["d"])), what
    assert np.all(np.abs(ls1 - ls0) <= 1e-9 * ls0), what
    assert abs(GP.loo_score() - fr.loo_score()) <= 1e-9 * (len(GP.Y) + abs(lref["value"])), what


# ---------------------------------------------------------------------------------------------------------------- 3. sequences
def test_remove_then_add_across_the_padding_edge(lib):
    """65 -> 64 -> 65 rows: the removal gives the 65th row back, addData takes it again (ibo_gp_extend needs no refit)"""
    kind, D = "svard", 4
    X, Y = synth(31, 66, D)
    GP = new_gp(kind, D, X[:65], Y[:65])
    GP.removeData(10)
    assert len(GP.X) == 64
    check_factor(lib, GP, kind, D, "65 -> 64")
    GP._fit_device = lambda *a, **k: pytest.fail("addData refitted: the removed row's head-room was not given back")
    try:
        GP.addData(X[65], Y[65])
    finally:
        del GP._fit_device                                   # (the instance's override; the method is the class's again)
    assert len(GP.X) == 65 and np.array_equal(GP.X, np.r_[X[:10], X[11:65], X[65:66]])
    check_factor(lib, GP, kind, D, "64 -> 65")
    check_like_fresh(GP, kind, D, what="65 -> 64 -> 65")


def test_adds_and_removals_interleaved_with_reserved_rows(lib):
    kind, D = "m5", 4
    X, Y = synth(32, 70, D)
    GP = new_gp(kind, D, X[:60], Y[:60], reserve_rows=8)
    n = 60
    for step, row in enumerate((0, 30, -1)):
        GP.addData(X[n], Y[n]); n += 1
        GP.removeData(row)
        check_factor(lib, GP, kind, D, "step %d" % step)
        check_like_fresh(GP, kind, D, what="step %d" % step)
    assert len(GP.X) == 60


def test_sliding_window(lib):
    """ten steps at N = 100: add the new point, drop the oldest"""
    kind, D = "ard", 4
    X, Y = synth(33, 110, D)
    GP = new_gp(kind, D, X[:100], Y[:100], reserve_rows=4)
    for k in range(10):
        GP.addData(X[100 + k], Y[100 + k])
        GP.removeData(0)
        assert len(GP.X) == 100 and np.array_equal(GP.X, X[k + 1:k + 101]) and np.array_equal(GP.Y, Y[k + 1:k + 101])
    check_factor(lib, GP, kind, D, "window")
    check_like_fresh(GP, kind, D, what="window")


def test_several_rows_by_both_routes_and_in_any_order(lib):
    kind, D, N = "ard", 4, 130
    X, Y = synth(34, N, D)
    Q = np.random.RandomState(8).rand(64, D)
    got = []
    for rows, route in (([0, 5, N - 1], "device"), ([N - 1, 0, 5], "device"), ([5, -1, 0], "device"), ([0, 5, N - 1], "refit")):
        GP = new_gp(kind, D, X, Y)
        GP.removeData(rows, _route=route)
        assert np.array_equal(GP.X, np.delete(X, [0, 5, N - 1], axis=0))
        check_factor(lib, GP, kind, D, "%s %s" % (rows, route))
        check_like_fresh(GP, kind, D, what="%s %s" % (rows, route))
        got.append((GP.L.copy(), get_W(lib, GP), GP.posteriors(Q), GP.loo()))
    for other in got[1:3]:                                   # the same rows named in another order: the same bits
        assert np.array_equal(other[0], got[0][0]) and np.array_equal(other[1], got[0][1])
        assert np.array_equal(other[2], got[0][2]) and np.array_equal(other[3], got[0][3])
    # more rows than REMOVE_MAX take the refit route on their own; four rows through the device entry all the same
    GP = new_gp(kind, D, X, Y)
    GP.removeData([7, 3, 99, 64], _route="device")
    check_factor(lib, GP, kind, D, "four rows")
    fits = []
    fit = GP._fit_device
    GP._fit_device = lambda *a, **k: (fits.append(1), fit(*a, **k))[1]
    GP.removeData(list(range(1, GP.REMOVE_MAX + 1)))         # REMOVE_MAX rows: the device entry
    assert not fits and len(GP.X) == N - 4 - GP.REMOVE_MAX
    GP.removeData(list(range(1, GP.REMOVE_MAX + 2)))         # one more: a refit
    assert fits == [1]
    check_factor(lib, GP, kind, D, "REMOVE_MAX + 1 rows, refitted")


def test_same_call_on_equal_models_gives_the_same_bits(lib):
    kind, D, N = "m3", 33, 200
    X, Y = synth(35, N, D)
    Q = np.random.RandomState(8).rand(64, D)
    res = []
    for _ in range(2):
        GP = new_gp(kind, D, X, Y)
        GP.removeData([17, 130], _route="device")
        res.append((GP.L.copy(), get_W(lib, GP), GP.posteriors(Q)))
    assert np.array_equal(res[0][0], res[1][0]) and np.array_equal(res[0][1], res[1][1]) and np.array_equal(res[0][2], res[1][2])


# ---------------------------------------------------------------------------------------------------------------- 4. addressing
def test_a_factor_beyond_two_gib(lib):
    """16400 rows: L and W exceed 2^31 bytes each.  Against the device's own refit of the remaining rows (a NumPy factor of that size does
    not fit a test's time)."""
    kind, D, N = "ard", 2, 16400
    assert N * N * 8 > 2 ** 31
    X, Y = synth(36, N, D)
    Q = np.random.RandomState(8).rand(16, D)
    GP = new_gp(kind, D, X, Y)
    GP.removeData(0, _route="device")
    print("removal of row 0 of %d: %.3f ms on the device" % (N, GP.last_fit_ms()))
    m1, v1 = GP.posteriors(Q)
    del GP
    fr = new_gp(kind, D, X[1:], Y[1:])
    m0, v0 = fr.posteriors(Q)
    values_close(m1, m0); values_close(v1, v0)


# ---------------------------------------------------------------------------------------------------------------- 5. state
def test_kept_sweep_state_and_caches_do_not_survive(lib):
    from ibo_amd import DeviceArray
    from ibo_amd.acquisition import sweep
    kind, D, N = "ard", 4, 300
    X, Y = synth(37, N + 1, D)
    GP = new_gp(kind, D, X[:N], Y[:N], reserve_rows=4)
    dc = DeviceArray.from_host(np.random.RandomState(71).rand(9001, D))

    def state():
        t, c = ctypes.c_int64(), ctypes.c_int64()
        lib.check(lib.lib.ibo_sweep_state_info(GP._handle(), ctypes.byref(t), ctypes.byref(c)))
        return t.value, c.value
    sweep(GP, dc, acq='ei', xi=.4, native=False, incremental=True)
    GP.addData(X[N], Y[N])
    assert "rank1" in sweep(GP, dc, acq='ei', xi=.4, native=False, incremental=True)["kernel"]      # the state is alive
    assert state()[0] > 0
    L0, R0 = GP.L, GP.R
    assert L0.shape == (N + 1, N + 1)
    GP.removeData(7, _route="device")
    assert state() == (0, 0)
    assert GP.L.shape == (N, N) and GP.R.shape == (N, N)
    r = sweep(GP, dc, acq='ei', xi=.4, native=False, incremental=True, outputs=("mu", "s2", "acq"))
    fr = new_gp(kind, D, GP.X, GP.Y)
    f = sweep(fr, dc, acq='ei', xi=.4, native=False, outputs=("mu", "s2", "acq"))
    assert "rank1" not in r["kernel"] and "finish" not in r["kernel"], r["kernel"]
    for k in ("mu", "s2", "acq"):
        values_close(r[k], f[k], k)
    a, b = f["acq"][r["best_idx"]], f["acq"][f["best_idx"]]
    assert r["best_idx"] == f["best_idx"] or abs(a - b) <= 1e-12 * abs(b)
    assert state()[0] > 0                                    # and a new state is kept from here on


# ---------------------------------------------------------------------------------------------------------------- 6. refusals
def test_refusals_leave_the_model_as_it_was(lib):
    kind, D, N = "ard", 4, 40
    X, Y = synth(38, N, D)
    Q = np.random.RandomState(8).rand(20, D)
    GP = new_gp(kind, D, X, Y)
    before = GP.posteriors(Q)
    L0 = GP.L.copy()
    for bad, exc in (([3, 3], ValueError), ([3, -37], ValueError), (N, IndexError), (-N - 1, IndexError), ([0, N], IndexError),
                     (list(range(N)), ValueError), ([], ValueError)):
        with pytest.raises(exc):
            GP.removeData(bad)
        assert len(GP.X) == N and np.array_equal(GP.X, X) and np.array_equal(GP.Y, Y)
    # the entry itself: the same refusals, IBO_ERR_ARG, and nothing touched
    h = GP._handle()
    info = ctypes.c_int(0)
    y = lib.f64(Y[:N - 1])
    call = lambda hh, rows: lib.lib.ibo_gp_remove(hh, len(rows), (ctypes.c_int * max(len(rows), 1))(*rows), lib.dp(y), ctypes.byref(info))
    for rows in ([3, 3], [N], [-1], list(range(N)), []):
        assert call(h, rows) == lib.ERR_ARG, rows
    assert lib.lib.ibo_gp_remove(h, 1, None, lib.dp(y), None) == lib.ERR_ARG
    assert lib.lib.ibo_gp_remove(h, 1, (ctypes.c_int * 1)(0), None, None) == lib.ERR_ARG
    after = GP.posteriors(Q)
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
    GP._cache = {}
    assert np.array_equal(GP.L, L0)
    # a handle never fitted, and one fitted from a caller's matrix: IBO_ERR_STATE
    hn = ctypes.c_void_p()
    lib.check(lib.lib.ibo_gp_create(lib.default_device(), ctypes.byref(hn)))
    try:
        assert call(hn, [0]) == lib.ERR_STATE
    finally:
        lib.check(lib.lib.ibo_gp_destroy(hn))
    GP._fit_device(A=GP.R + .5 * np.eye(N))
    bm = GP.posteriors(Q)
    assert call(GP._handle(), [0]) == lib.ERR_STATE
    am = GP.posteriors(Q)
    assert np.array_equal(bm[0], am[0]) and np.array_equal(bm[1], am[1])
    # removeData on such a model takes the refit route (its factor is not one that can be reduced)
    GP.removeData(0)
    check_like_fresh(GP, kind, D, what="after a matrix fit")


# ---------------------------------------------------------------------------------------------------------------- 7. beyond one chunk, other routes, poor conditioning
def remove_on_device(GP, rows):
    """removeData by the device route, known to have stayed on it: _remove_device answers False where ibo_gp_remove returns IBO_ERR_STATE
    or IBO_ERR_NOT_PD, and removeData then refits without a word -- every check after it would read a fresh factor, not downdate.hip's"""
    def refused(*a, **k):
        pytest.fail("ibo_gp_remove refused rows %s: removeData fell back to a refit" % (rows,))
    GP._fit_device = refused
    try:
        GP.removeData(rows, _route="device")
    finally:
        del GP._fit_device


# downdate_scalars_kernel walks p in chunks of 1024 (m = N - 1 - i entries, ts[0] = ts[n] carried from one chunk into the next) and
# downdate_W_prefix_kernel keeps eight 64-row segments in flight (a second pass from 513 rows below i on): both sides of each edge
CHUNK_CASES = [("ard", 600, 0), ("ard", 1026, 0), ("ard", 1026, 1), ("ard", 1090, 1), ("ard", 2100, 0), ("ard", 2100, 1075),
               ("ard", 2100, 1074), ("ard", 2100, 2099), ("m5", 1090, 0)]


@pytest.mark.parametrize("kind,N,i", CHUNK_CASES)
def test_factor_after_one_removal_beyond_one_chunk(lib, kind, N, i):
    """L, W and R against NumPy at 1e-9 where m = N - 1 - i is 599, 1025 (one element into the second chunk), 1024 (exactly one chunk),
    1088, 2099 (three chunks, 33 segments), 1024 and 1025 inside a larger model, and 0.  cond_2(R) <= 1e6 is asserted from R's eigenvalues
    (numpy.linalg.eigvalsh: for a symmetric positive definite matrix the ratio of the extreme ones IS cond_2) up to 1090 rows, and at 2100
    rows by the bound N (1 + noise) / noise = 23100 (cond_of), which costs nothing: an SVD of 2100 rows alone is several seconds."""
    D = 4
    with wall("%s N=%d i=%d" % (kind, N, i)):
        X, Y = synth(N + i + 3, N, D)
        GP = new_gp(kind, D, X, Y)
        remove_on_device(GP, i)
        keep = np.r_[0:i, i + 1:N]
        assert len(GP.X) == N - 1 and np.array_equal(GP.X, X[keep]) and np.array_equal(GP.Y, Y[keep])
        check_factor(lib, GP, kind, D, "%s N=%d i=%d m=%d" % (kind, N, i, N - 1 - i), cond="bound" if N > 1500 else "eigvalsh")


def sweep_like_fresh(GP, fr, D, what):
    """one 9001-candidate sweep on the full-sweep route (it reads the repacked Wp) against the fresh model's"""
    from ibo_amd import DeviceArray
    from ibo_amd.acquisition import sweep
    big = DeviceArray.from_host(np.random.RandomState(10).rand(9001, D))
    r = sweep(GP, big, acq="ei", native=False, outputs=("mu", "s2", "acq"))
    f = sweep(fr, big, acq="ei", native=False, outputs=("mu", "s2", "acq"))
    assert r["kernel"].startswith("sweep2"), r["kernel"]
    for k in ("mu", "s2", "acq"):
        values_close(r[k], f[k], "%s 9001 %s" % (what, k))
    a, b = f["acq"][r["best_idx"]], f["acq"][f["best_idx"]]
    assert r["best_idx"] == f["best_idx"] or abs(a - b) <= 1e-12 * abs(b), (what, r["best_idx"], f["best_idx"], a, b)


ROUTES = {"super": (b"super_min_nb", 32), "two_level": (b"fused2_min_nb", 33)}
ROUTE_OPS = ["one", "two", "three", "add"]


@pytest.mark.parametrize("upto", ROUTE_OPS)
@pytest.mark.parametrize("route", sorted(ROUTES))
def test_removal_from_a_model_fitted_on_another_route(lib, route, upto):
    """2100 rows (33 block columns) fitted in super-panels (super_min_nb = 32) and in the two-level order (fused2_min_nb = 33): fit_factor
    leaves T, Wp and W in other roles there than on the plain single-level route (T and Wp traded after the transposing pack; T as
    launch_trinv's scratch), and ibo_gp_remove writes L' into T and trades L and T after an odd number of steps.  One handle goes through
    remove one row -> remove two rows in one call (even: the factor ends where it began) -> remove three rows through the entry itself
    (odd) -> addData of one point; the case `upto` replays that sequence up to its step and checks there, so every state of the handle
    is checked and no case pays for the others' NumPy factors: L (with its deferred zero_upper), W and R against NumPy at 1e-9, the
    posterior against a fresh model, one sweep on the full-sweep route.  cond_2(R) <= 23100 by the bound (cond_of)."""
    kind, D, N = "ard", 4, 2100
    key, val = ROUTES[route]
    with wall("%s up to %s" % (route, upto)):
        X, Y = synth(77, N + 1, D)
        with option(key, val):
            GP = new_gp(kind, D, X[:N], Y[:N])
            W_route = get_W(lib, GP) if upto == "one" else None
            mirror = np.arange(N)
            for op in ROUTE_OPS[:ROUTE_OPS.index(upto) + 1]:
                if op == "one":
                    remove_on_device(GP, 700)
                    mirror = np.delete(mirror, [700])
                elif op == "two":
                    remove_on_device(GP, [3, 1500])
                    mirror = np.delete(mirror, [3, 1500])
                elif op == "three":
                    rows = [0, 1024, len(mirror) - 1]
                    mirror = np.delete(mirror, rows)
                    info = ctypes.c_int(0)
                    y = lib.f64(Y[mirror])
                    lib.check(lib.lib.ibo_gp_remove(GP._handle(), 3, (ctypes.c_int * 3)(*rows), lib.dp(y), ctypes.byref(info)))
                    assert info.value == 0
                    GP.X, GP.Y = X[mirror], Y[mirror]
                    GP._cache = {}
                else:
                    GP._fit_device = lambda *a, **k: pytest.fail("addData refitted although the padding has room")
                    try:
                        GP.addData(X[N], Y[N])
                    finally:
                        del GP._fit_device
                    mirror = np.r_[mirror, N]
        assert np.array_equal(GP.X, X[mirror]) and np.array_equal(GP.Y, Y[mirror])
        if W_route is not None:
            # the option did move the fit: the two-level order forms W by recursive doubling, another order of the same sums than the
            # ride-along's, while super-panels are documented to give the bits of the step-by-step order (their buffers differ, not their sums)
            same = np.array_equal(W_route, get_W(lib, new_gp(kind, D, X[:N], Y[:N])))
            assert same == (route == "super"), (route, same)
        what = "%s after %s" % (route, upto)
        check_factor(lib, GP, kind, D, what, cond="bound")
        fr = check_like_fresh(GP, kind, D, what=what)
        sweep_like_fresh(GP, fr, D, what)


COND_CASES = [(1e-4, 2), (1e-3, 1), (1e-4, 1)]


@pytest.mark.parametrize("noise,D", COND_CASES)
def test_removal_and_extension_where_conditioning_is_worst(lib, noise, D):
    """The data of test_gpu_parity.py::test_tolerance_where_conditioning_is_worst (three clusters of near-duplicates) at N = 300, SE-ARD
    l = .3, noise 1e-4 and 1e-3: rows [0], [150] and [5, 200] removed from the fitted model by the device route, then one near-duplicate
    point appended to the last of these.  After each, mu and sigma^2 at 24 candidates (half of them 1e-3 from training points) against the
    80-bit posterior of the data the model holds, at that test's bars for a fit: 1e-7 for mu (floor 1e-9), 1e-8 for sigma^2 clipped to
    [1e-8, 10].
    The factor is held to 1e-9 against NumPy's WITHOUT the cond_2 <= 1e6 precondition of every other case here: cond_2 is 2e5 .. 2.3e6 on
    these inputs, above the precondition for some of them, and the bar is met all the same -- the float64 restatement of the removal
    (downdate_reference.remove_rows) is within 2.1e-11 (W) and 3.4e-12 (L) of NumPy's refit on exactly these inputs, and within 3.3e-10
    (mu) and 1.9e-9 (sigma^2) of the 80-bit values, where a float64 refit is within 1.0e-9 and 6e-10: the reference alone keeps more
    than five times room under each bar."""
    from ibo_amd.acquisition import sweep
    from ibo_amd.gaussianprocess import GaussianProcess
    from ibo_amd.gaussianprocess.kernel import GaussianKernel_ard
    from test_gpu_parity import _longdouble_posterior
    N, ell = 300, .3
    okern = orc.Kern("ard", np.full(D, ell))
    kfun = lambda Xm, q: np.array([okern.cov(x, q) for x in Xm])

    def rel(a, b, floor):
        return float(np.max(np.abs(a - b) / np.maximum(np.abs(b), floor)))

    def check(GP, cand, what):
        R = orc.GP(okern, GP.X, GP.Y, noise=noise).R
        eL, eW = check_factor(lib, GP, "ard", D, what, R=R, max_cond=None)
        r = sweep(GP, cand, acq='ei', xi=.01, native=True, outputs=("mu", "s2"))
        t_mu, t_s2 = _longdouble_posterior(R, GP.X, GP.Y, kfun, cand, noise)
        e_mu, e_s2 = rel(r["mu"], t_mu, 1e-9), rel(r["s2"], np.clip(t_s2, 1e-8, 10), 1e-300)
        print("%s: mu %.3g  s2 %.3g against 80 bits" % (what, e_mu, e_s2))
        assert e_mu < 1e-7 and e_s2 < 1e-8, (what, e_mu, e_s2)

    with wall("noise %g D=%d" % (noise, D)):
        rs = np.random.RandomState(N + D)
        c = rs.rand(3, D)
        X = np.clip(np.vstack([c[i] + 0.02 * rs.randn(N // 4, D) for i in range(3)] + [rs.rand(N - 3 * (N // 4), D)]), 0, 1)
        Y = np.sin(3 * X.sum(1)) + .01 * rs.randn(N)
        for rows in ([0], [N // 2], [5, 200]):
            GP = GaussianProcess(GaussianKernel_ard(np.full(D, ell)), X, Y, noise=noise)
            remove_on_device(GP, rows)
            keep = np.delete(np.arange(N), rows)
            assert np.array_equal(GP.X, X[keep]) and np.array_equal(GP.Y, Y[keep])
            cand = np.vstack([rs.rand(12, D), np.clip(X[keep][rs.randint(0, len(keep), 12)] + 1e-3 * rs.randn(12, D), 0, 1)])
            check(GP, cand, "noise %g D=%d rows %s" % (noise, D, rows))
        # the rows' head-room is back: a point 1e-3 from a training point of the first cluster goes in without a refit
        xn = np.clip(GP.X[20] + 1e-3 * rs.randn(D), 0, 1)
        GP._fit_device = lambda *a, **k: pytest.fail("addData refitted although the padding has room")
        try:
            GP.addData(xn, np.sin(3 * xn.sum()))
        finally:
            del GP._fit_device
        assert len(GP.X) == N - 1
        cand = np.vstack([rs.rand(12, D), np.clip(GP.X[rs.randint(0, N - 1, 12)] + 1e-3 * rs.randn(12, D), 0, 1)])
        cand[12] = np.clip(xn + 1e-3 * rs.randn(D), 0, 1)       # one of them next to the new point
        check(GP, cand, "noise %g D=%d rows [5, 200], then one near-duplicate" % (noise, D))

"""
The NumPy restatement of the O(N^2) removal of observations (tests/downdate_reference.py, the yardstick of tests/test_gpu_remove.py) against
numpy.linalg.cholesky / inv of the reduced matrix and against the oracle's posterior of the model refitted without the rows; and the C ABI's
and the Python mirror's new entry as far as they can be checked without a GPU.  CPU only.

Bounds: L' and W' to 1e-10 of max|.| -- a tenth of the GPU test's 1e-9; the step's own error is a few cond * 2^-53 (at cond_2 = 4e5 it was
measured at 3e-13 for L and 8e-12 for W), and every case asserts cond_2(R) <= 1e6 first: a bar is never met by an ill-posed input.  The
posterior at the project's 1e-6.
"""
import ctypes

import numpy as np
import pytest

from conftest import synth
from oracle import oracle as orc
import downdate_reference as dr
from wall_time import wall

KERNELS = [("ard", [.3, .5, .4]), ("iso", [.4]), ("svard", [.3, .5, .4, .9]), ("sviso", [.4, .8]),
           ("m3", [.5, .95]), ("m5", [.5, 0.9])]
SIZES = [2, 3, 65, 200]
NOISE = .1


def rows_of(N):
    """single rows: first, last, an interior one; and triples removed together (where three rows can go)"""
    cases = sorted({(0,), (N - 1,), (N // 2,)})
    if N > 3:
        cases += [(0, 5, N - 1), (N // 2, N // 2 + 1, 3), (N - 1, N - 2, N - 3)]
    return cases


def model(kind, hyper, N):
    X, Y = synth(N + 3, N, 3)
    gp = orc.GP(orc.Kern(kind, hyper), X, Y, noise=NOISE)
    c = dr.cond2(gp.R)
    assert c <= 1e6, (kind, N, c)
    return gp, X, Y


@pytest.mark.parametrize("N", SIZES)
@pytest.mark.parametrize("kind,hyper", KERNELS)
def test_factor_and_inverse_are_those_of_the_reduced_matrix(kind, hyper, N):
    gp, X, Y = model(kind, hyper, N)
    L = gp.L
    W = np.linalg.inv(L)
    for rows in rows_of(N):
        keep = np.setdiff1d(np.arange(N), rows)
        Rr = gp.R[np.ix_(keep, keep)]
        Lref = np.linalg.cholesky(Rr)
        Wref = np.linalg.inv(Lref)
        L2, W2 = dr.remove_rows(L, W, rows)
        assert L2.shape == Lref.shape and W2.shape == Wref.shape
        eL, eW = dr.relerr(L2, Lref), dr.relerr(W2, Wref)
        print("%s N=%d rows=%s: cond %.3g  L err %.3g  W err %.3g" % (kind, N, rows, dr.cond2(gp.R), eL, eW))
        assert eL <= 1e-10 and eW <= 1e-10, (kind, N, rows, eL, eW)
        assert np.array_equal(L2, np.tril(L2)) and np.array_equal(W2, np.tril(W2))
        # the order in which the rows are named does not matter: the same bits
        La, Wa = dr.remove_rows(L, W, rows[::-1])
        assert np.array_equal(La, L2) and np.array_equal(Wa, W2)


def test_scalars_factor_the_rank_one_update():
    """diag(d) + strict-lower(p q^T) is the Cholesky factor of I + p p^T, and diag(1 / d) - strict-lower(q p^T) its inverse"""
    gp, X, Y = model("ard", [.3, .5, .4], 65)
    W = np.linalg.inv(gp.L)
    for i in (0, 31, 63):
        p, d, q = dr.scalars(W, i)
        m = len(p)
        Lt = np.diag(d) + np.tril(np.outer(p, q), -1)
        assert dr.relerr(Lt @ Lt.T, np.eye(m) + np.outer(p, p)) <= 1e-13
        assert dr.relerr((np.diag(1 / d) - np.tril(np.outer(q, p), -1)) @ Lt, np.eye(m)) <= 1e-13
        # p is L33^-1 l32 without a product
        assert dr.relerr(p, np.linalg.solve(gp.L[i + 1:, i + 1:], gp.L[i + 1:, i])) <= 1e-12
    with pytest.raises(ValueError):
        dr.remove_rows(gp.L, W, [3, 3])
    with pytest.raises(IndexError):
        dr.remove_rows(gp.L, W, [65])


@pytest.mark.parametrize("with_prior", [False, True])
@pytest.mark.parametrize("kind,hyper", KERNELS)
def test_posterior_is_the_oracles_of_the_model_refitted_without_the_rows(kind, hyper, with_prior):
    N = 65
    rs = np.random.RandomState(7)
    prior = orc.Prior(rs.rand(4, 3), rs.randn(4), 2.0, np.zeros(3) - .1, np.full(3, 1.2)) if with_prior else None
    gp, X, Y = model(kind, hyper, N)
    Q = np.random.RandomState(3).rand(64, 3)
    for rows in [(0,), (64,), (17,), (0, 5, 64)]:
        keep = np.setdiff1d(np.arange(N), rows)
        fresh = orc.GP(orc.Kern(kind, hyper), X[keep], Y[keep], noise=NOISE, prior=prior)
        mu, s2 = fresh.posteriors(Q)
        L2, W2 = dr.remove_rows(gp.L, np.linalg.inv(gp.L), rows)
        # through the oracle with the reduced factor in place of its own ...
        down = orc.GP(orc.Kern(kind, hyper), X[keep], Y[keep], noise=NOISE, prior=prior)
        down.L = L2
        dmu, ds2 = down.posteriors(Q)
        assert np.all(np.abs(dmu - mu) <= 1e-6 * np.maximum(1.0, np.abs(mu))), (kind, rows)
        assert np.all(np.abs(ds2 - s2) <= 1e-6 * s2), (kind, rows)
        # ... and from W' alone: v = W' k*, mu = m(x) + v.(W' (Y - m(X))), s2 = 1 + noise - |v|^2 clipped to [1e-7, 10]
        kern = orc.Kern(kind, hyper)
        Ks = np.array([[kern.cov(x, c) for c in Q] for x in X[keep]])
        V = W2 @ Ks
        mq = np.array([prior.mu(c) for c in Q]) if with_prior else np.zeros(len(Q))
        wy, w1 = W2 @ Y[keep], W2 @ np.ones(len(keep))
        wmu = mq + V.T @ wy - mq * (V.T @ w1)         # the reference subtracts the QUERY's prior mean from every target
        ws2 = np.clip(1 + NOISE - np.sum(V * V, axis=0), 1e-7, 10)
        assert np.all(np.abs(wmu - mu) <= 1e-6 * np.maximum(1.0, np.abs(mu))), (kind, rows)
        assert np.all(np.abs(ws2 - s2) <= 1e-6 * s2), (kind, rows)


@pytest.mark.parametrize("N", SIZES)
@pytest.mark.parametrize("kind,hyper", KERNELS)
def test_append_row_gives_factor_and_inverse_of_the_extended_matrix(kind, hyper, N):
    """append_row (one step of ibo_gp_extend restated) from numpy's factor of the first N - 1 points, and from the restatement's own
    factor after a removal: against numpy.linalg.cholesky / inv of the matrix of the points held, at the removal's bar"""
    with wall("append_row %s N=%d" % (kind, N)):
        gp, X, Y = model(kind, hyper, N)
        R = gp.R
        L0 = np.linalg.cholesky(R[:N - 1, :N - 1])
        L2, W2 = dr.append_row(L0, np.linalg.inv(L0), R[:N - 1, N - 1], R[N - 1, N - 1])
        Lref = np.linalg.cholesky(R)
        Wref = np.linalg.inv(Lref)
        assert L2.shape == Lref.shape and W2.shape == Wref.shape
        eL, eW = dr.relerr(L2, Lref), dr.relerr(W2, Wref)
        print("%s N=%d append: L err %.3g  W err %.3g" % (kind, N, eL, eW))
        assert eL <= 1e-10 and eW <= 1e-10, (kind, N, eL, eW)
        assert np.array_equal(L2, np.tril(L2)) and np.array_equal(W2, np.tril(W2))
        assert np.array_equal(L2[:N - 1, :N - 1], L0)                    # the old rows are not touched
        if N > 2:
            # remove row 0, then append it again at the end: the factor of the rotated points
            La, Wa = dr.remove_row(Lref, Wref, 0)
            Lb, Wb = dr.append_row(La, Wa, R[1:, 0], R[0, 0])
            order = np.r_[1:N, 0]
            Lrot = np.linalg.cholesky(R[np.ix_(order, order)])
            eL, eW = dr.relerr(Lb, Lrot), dr.relerr(Wb, np.linalg.inv(Lrot))
            assert eL <= 1e-10 and eW <= 1e-10, (kind, N, eL, eW)


DRIFT_STEPS = (1, 10, 100, 300, 1000)


@pytest.mark.parametrize("noise", [.1, 1e-4])
@pytest.mark.parametrize("mode", ["window", "random"])
def test_restatement_does_not_drift_over_a_thousand_steps(mode, noise):
    """1000 steps of "append one, remove row 0" and of "append one, remove a random row" at N = 100, D = 4, SE-ARD with l = .45: the
    restatement against a fresh NumPy factor at steps 1, 10, 100, 300 and 1000, at the bar of the single step (1e-10 of max|.|, cond_2 <= 1e6
    asserted).  The premise of the device's length test (tests/test_gpu_handle_sequences.py): the algorithm itself stays flat.  Measured:
    noise .1 (cond ~ 300) L <= 5.2e-15, W <= 1.2e-14; noise 1e-4 (cond 8e4 .. 2.6e5) L <= 6.4e-13, W <= 1.3e-11 at every checkpoint (the noise 1e-4 figures move
    with the host's BLAS by a factor of two or so)."""
    with wall("1000 %s steps of the restatement at noise %g" % (mode, noise)):
        X0, plan = dr.window_plan(41, 100, 4, 1000, mode)
        got, X = dr.run_window(X0, plan, .45, noise, DRIFT_STEPS)
        assert sorted(got) == list(DRIFT_STEPS) and X.shape == (100, 4)
        for step in DRIFT_STEPS:
            c, eL, eW = got[step]
            print("%s noise %g step %4d: cond %.3g  L err %.3g  W err %.3g" % (mode, noise, step, c, eL, eW))
            assert c <= 1e6, (mode, noise, step, c)
            assert eL <= 1e-10 and eW <= 1e-10, (mode, noise, step, eL, eW)


def test_remove_entry_is_exported_bound_and_mirrored():
    """fails without the feature: the symbol, its binding, its argument check, GaussianProcess.removeData, and the preference GP's refusal"""
    from ibo_amd import _lib
    from ibo_amd.gaussianprocess import GaussianProcess, PrefGaussianProcess
    from ibo_amd.gaussianprocess.kernel import GaussianKernel_ard
    assert "ibo_gp_remove" in _lib.EXPORTED
    fn = _lib.lib.ibo_gp_remove
    assert fn.restype is ctypes.c_int and len(fn.argtypes) == 5
    rows = (ctypes.c_int * 1)(0)
    y = _lib.f64(np.zeros(1))
    info = ctypes.c_int(0)
    assert fn(None, 1, rows, _lib.dp(y), ctypes.byref(info)) == _lib.ERR_ARG
    assert _lib.lib.ibo_abi_version() == 8
    assert callable(getattr(GaussianProcess, "removeData"))
    assert isinstance(GaussianProcess.REMOVE_MAX, int) and GaussianProcess.REMOVE_MAX >= 1
    P = PrefGaussianProcess(GaussianKernel_ard([.5] * 3))
    with pytest.raises(NotImplementedError):
        P.removeData(0)
    assert P._dev is None                            # no device was touched
    # an empty model has nothing to remove
    with pytest.raises(IndexError):
        GaussianProcess(GaussianKernel_ard([.5] * 3)).removeData(0)

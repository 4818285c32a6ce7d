"""
The NumPy restatement of the joint posterior (tests/cov_reference.py, the yardstick of tests/test_gpu_posterior_cov.py) against
the oracle: its diagonal is the oracle's posterior variance, and conditioning on a query point through the oracle's own fit gives
Sigma_ii - Sigma_ij^2 / Sigma_jj.  CPU only.
"""
import ctypes

import numpy as np
import pytest

from conftest import synth
from oracle import oracle as orc
import cov_reference as cr
import grad_reference as gr

KERNELS = [("ard", [.3, .5, .4]), ("iso", [.4]), ("svard", [.3, .5, .4, .9]), ("sviso", [.4, .8]),
           ("m3", [.5, .95]), ("m5", [.5, 0.9])]


def models(kind, hyper, with_prior, N=40):
    X, Y = synth(5, N, 3)
    fam, w, sf2 = gr.kernel_spec(kind, hyper, 3)
    prior = oprior = None
    if with_prior:
        rs = np.random.RandomState(7)
        prior = (rs.rand(4, 3), rs.randn(4), 2.0, np.zeros(3) - .1, np.full(3, 1.2))
        oprior = orc.Prior(*prior)
    return orc.GP(orc.Kern(kind, hyper), X, Y, noise=.1, prior=oprior), gr.RefGP(X, Y, .1, fam, w, sf2, prior=prior)


@pytest.mark.parametrize("with_prior", [False, True])
@pytest.mark.parametrize("kind,hyper", KERNELS)
def test_diagonal_is_the_oracle_variance(kind, hyper, with_prior):
    ogp, ref = models(kind, hyper, with_prior)
    Q = np.r_[np.random.RandomState(3).rand(12, 3), ogp.X[:2] + 1e-3]
    S, vn = cr.cov(ref, Q)
    _, s2 = ogp.posteriors(Q)
    live = (s2 > 1e-7) & (s2 < 10)
    assert live.sum() >= 12
    np.testing.assert_allclose(np.diag(S)[live], s2[live], rtol=1e-10)
    assert np.array_equal(S, S.T)
    S0, _ = cr.cov(ref, Q, with_noise=False)
    np.testing.assert_allclose(np.diag(S0), np.diag(S) - .1, rtol=0, atol=1e-13)
    off = ~np.eye(len(Q), dtype=bool)
    assert np.array_equal(S0[off], S[off])
    # the L form agrees with the cho_solve form
    S1, vn1 = cr.cov_L(np.linalg.cholesky(ref.R), ref.X, ref.fam, ref.w, ref.sf2, ref.noise, Q)
    cr.assert_cov_close(S1, S, vn, ref.sf2, ref.noise, what="L form")


@pytest.mark.parametrize("kind,hyper", [KERNELS[0], KERNELS[3], KERNELS[4], KERNELS[5]])
def test_conditioning_identity_on_the_oracle(kind, hyper):
    ogp, ref = models(kind, hyper, False, N=30)
    rs = np.random.RandomState(9)
    Q = rs.rand(8, 3)
    S, _ = cr.cov(ref, Q)
    for j in (0, 3, 7):
        X2 = np.r_[ogp.X, Q[j:j + 1]]
        Y2 = np.r_[ogp.Y, [0.3]]
        o2 = orc.GP(orc.Kern(kind, hyper), X2, Y2, noise=.1)
        _, s2 = o2.posteriors(Q)
        want = np.diag(S) - S[:, j] ** 2 / S[j, j]
        others = np.arange(len(Q)) != j
        np.testing.assert_allclose(s2[others], want[others], rtol=0, atol=1e-10)


def test_entries_without_a_gpu_report_no_device():
    from ibo_amd import _lib
    if _lib.device_count() > 0:
        pytest.skip("a GPU is visible here")
    Q = _lib.f64(np.zeros((2, 3)))
    S = np.empty(4); Z = np.zeros(4); F = np.empty(4); mu = np.empty(2); info = ctypes.c_int(0)
    assert _lib.lib.ibo_posterior_cov(None, 2, _lib.dp(Q), 1, _lib.dp(mu), _lib.dp(S)) == _lib.ERR_NO_DEVICE
    assert _lib.lib.ibo_posterior_sample(None, 2, _lib.dp(Q), 1, 0.0, 2, _lib.dp(Z), _lib.dp(F), None,
                                         ctypes.byref(info)) == _lib.ERR_NO_DEVICE
    from ibo_amd.gaussianprocess import GaussianProcess
    from ibo_amd.gaussianprocess.kernel import GaussianKernel_ard
    with pytest.raises(ValueError):
        GaussianProcess(GaussianKernel_ard([.5] * 3)).sample_posterior(Q)

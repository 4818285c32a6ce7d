"""
The NumPy gradient restatement of tests/grad_reference.py (the yardstick of tests/test_gpu_gradients.py) against central
differences of the oracle: its posterior (orc_posterior_chol through oracle.GP.posteriors) and its acquisition values
(orc_acq_value), for every kernel type, with and without an RBF-network prior.  CPU only.
"""
import numpy as np
import pytest

from conftest import synth
from oracle import oracle as orc
import grad_reference as gr

KERNELS = [("ard", [.3, .5, .4]), ("iso", [.4]), ("svard", [.3, .5, .4, .9]), ("sviso", [.4, .8]),
           ("m3", [.5, .95]), ("m5", [.5, 0.9])]
H = 1e-6


def fd(f, Q, h=H):
    """central differences of f: (M, D) -> (M,), per coordinate"""
    G = np.zeros(Q.shape)
    for d in range(Q.shape[1]):
        E = np.zeros(Q.shape); E[:, d] = h
        G[:, d] = (f(Q + E) - f(Q - E)) / (2 * h)
    return G


def models(kind, hyper, with_prior):
    X, Y = synth(5, 40, 3)
    fam, w, sf2 = gr.kernel_spec(kind, hyper, 3)
    prior = None
    oprior = None
    if with_prior:
        rs = np.random.RandomState(7)
        prior = (rs.rand(4, 3), rs.randn(4), 2.0, np.zeros(3) - .1, np.full(3, 1.2))
        oprior = orc.Prior(*prior)
    ogp = orc.GP(orc.Kern(kind, hyper), X, Y, noise=.1, prior=oprior)
    ref = gr.RefGP(X, Y, .1, fam, w, sf2, prior=prior)
    return ogp, ref


@pytest.mark.parametrize("with_prior", [False, True])
@pytest.mark.parametrize("kind,hyper", KERNELS)
def test_posterior_gradient_matches_oracle_differences(kind, hyper, with_prior):
    ogp, ref = models(kind, hyper, with_prior)
    Q = np.random.RandomState(3).rand(12, 3)
    r = ref.grad(Q)
    mu, s2 = ogp.posteriors(Q)
    np.testing.assert_allclose(r["mu"], mu, rtol=1e-11, atol=1e-13)
    np.testing.assert_allclose(r["s2"], s2, rtol=1e-11, atol=1e-13)
    gmu = fd(lambda P: ogp.posteriors(P)[0], Q)
    gs2 = fd(lambda P: ogp.posteriors(P)[1], Q)
    for got, want, what in ((r["dmu"], gmu, "dmu"), (r["ds2"], gs2, "ds2")):
        np.testing.assert_allclose(got, want, rtol=1e-6, atol=1e-7 * np.max(np.abs(want)), err_msg=what)


@pytest.mark.parametrize("erf_mode", [gr.ERF_LIBM, gr.ERF_NR])
@pytest.mark.parametrize("acq", [gr.ACQ_EI, gr.ACQ_PI, gr.ACQ_UCB])
@pytest.mark.parametrize("kind,hyper", [KERNELS[0], KERNELS[4], KERNELS[5]])
def test_acquisition_gradient_matches_oracle_differences(kind, hyper, acq, erf_mode):
    ogp, ref = models(kind, hyper, True)
    Q = np.random.RandomState(4).rand(12, 3)
    parm = 0.7 if acq == gr.ACQ_UCB else 0.01
    ymax = float(np.max(ogp.Y))
    r = ref.grad(Q, acq=acq, parm=parm, erf_mode=erf_mode)

    def val(P):
        mu, s2 = ogp.posteriors(P)
        return orc.acq_value(acq, erf_mode, mu, np.sqrt(s2), ymax, parm)
    np.testing.assert_allclose(r["acq"], val(Q), rtol=1e-10, atol=1e-13)
    g = fd(val, Q)
    rtol = 1e-6 if erf_mode == gr.ERF_LIBM else 1e-4      # NR: analytic gradient of the untruncated constants
    np.testing.assert_allclose(r["dacq"], g, rtol=rtol, atol=rtol * 0.1 * np.max(np.abs(g)))


def test_clip_makes_the_variance_gradient_zero():
    X, Y = synth(2, 10, 2)
    fam, w, sf2 = gr.kernel_spec('ard', [.3, .3], 2)
    far = gr.RefGP(X, Y, 10.0, fam, w, sf2).grad(np.array([[40.0, 40.0]]))
    assert far["s2"][0] == 10.0 and np.all(far["ds2"] == 0.0)
    near = gr.RefGP(X, Y, 1e-9, fam, w, sf2).grad(X[:3], clamp_lo=1e-8)
    assert np.all(near["s2"] == 1e-8) and np.all(near["ds2"] == 0.0)

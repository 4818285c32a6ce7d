"""
The NumPy restatement of the pathwise draws' gradients (tests/paths_grad_reference.py, the yardstick of tests/test_gpu_paths_grad.py)
pinned to central differences of tests/paths_reference.py's values and to its own evaluation in long double; the new ABI entry and
the Python layer's new names.  CPU only.

The second pin sets the GPU test's composition bar: the float64 restatement stays within 1e-12 T_grad of the same formulas in
long double, a tenth of the 1e-11 T_grad the device is held to.
"""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

import cov_reference as cr
import grad_reference as gr
import paths_grad_reference as pg
import paths_reference as pr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HYPER = {"iso": [.3], "m3": [.3, 1.0], "m5": [.3, 1.0], "sviso": [.35, .9]}
CASES = [(kind, prior, D) for kind in ("iso", "m3", "m5", "sviso") for prior in (False, True) for D in (1, 3)]


def kernel_of(kind, hyper):
    from ibo_amd.gaussianprocess import kernel as K
    return {"iso": K.GaussianKernel_iso, "sviso": K.SVGaussianKernel_iso, "m3": K.MaternKernel3,
            "m5": K.MaternKernel5}[kind](np.array(hyper, dtype=float))


def setup(kind, prior, D, N=25, F=48, S=3, M=12, seed=0):
    """a model on unit-cube data, its spectral draws and coefficients, and query points of which the first four are rows of X"""
    from ibo_amd.acquisition.pathwise import spectralDraws
    rs = np.random.RandomState(40 + seed)
    X = rs.rand(N, D); Y = np.sin(3 * X.sum(1)) + .01 * rs.randn(N)
    fam, w, sf2 = gr.kernel_spec(kind, HYPER[kind], D)
    p = (rs.rand(4, D), rs.randn(4), 1.5, np.zeros(D) - .1, np.full(D, 1.2)) if prior else None
    ref = gr.RefGP(X, Y, .1, fam, w, sf2, prior=p)
    omega, phase, wts, eps = spectralDraws(kernel_of(kind, HYPER[kind]), D, F, S, N, 1 + .1 - sf2, 5 + seed)
    c = pr.coef(ref, omega, phase, wts, eps)
    Q = np.r_[X[:4], rs.rand(M - 4, D)]
    return ref, omega, phase, c, Q


@pytest.mark.parametrize("kind,prior,D", CASES)
def test_restatement_against_central_differences_of_the_values(kind, prior, D):
    ref, omega, phase, c, Q = setup(kind, prior, D)
    got = pg.grads(ref, omega, phase, c, Q)
    assert got.shape == (3, len(Q), D) and np.all(np.isfinite(got))
    step = 1e-5
    G = np.zeros(got.shape)
    for d in range(D):
        E = np.zeros(Q.shape); E[:, d] = step
        G[:, :, d] = (pr.values(ref, omega, phase, c, Q + E) - pr.values(ref, omega, phase, c, Q - E)) / (2 * step)
    bar = 1e-5 * np.abs(G) + 1e-6 * np.max(np.linalg.norm(got, axis=2))
    print("%s prior=%s D=%d: worst error / bar = %.3g" % (kind, prior, D, float(np.max(np.abs(got - G) / bar))))
    assert np.all(np.abs(got - G) <= bar)


@pytest.mark.parametrize("kind,prior,D", CASES)
def test_restatement_in_float64_against_itself_in_long_double(kind, prior, D):
    if np.finfo(np.longdouble).eps >= np.finfo(np.float64).eps:
        pytest.fail("long double is float64 here: the restatement has nothing more precise to be measured against")
    ref, omega, phase, c, Q = setup(kind, prior, D, seed=1)
    g64 = pg.grads(ref, omega, phase, c, Q)
    gld = pg.grads(ref, omega, phase, c, Q, dtype=np.longdouble)
    T = pg.grad_scale(ref, omega, phase, c, Q)
    assert gld.dtype == np.longdouble and g64.dtype == np.float64 and T.shape == g64.shape and np.all(T > 0)
    err = np.abs(gld - g64).astype(float)
    print("%s prior=%s D=%d: worst float64 error = %.3g T_grad" % (kind, prior, D, float(np.max(err / T))))
    assert np.all(err <= 1e-12 * T)


def test_the_restatements_parts_are_the_projects_own():
    ref, omega, phase, c, Q = setup("m5", True, 3)
    Ks, dK = pg.dkstar(ref, Q)
    assert np.allclose(Ks, cr.kmat(ref.fam, ref.w, ref.sf2, Q, ref.X), rtol=1e-14, atol=0)
    for j, x in enumerate(Q):
        k, h, diff = gr.kstar(ref.fam, ref.w, ref.sf2, x, ref.X)
        assert np.allclose(dK[j], h[:, None] * ref.w * diff, rtol=1e-13, atol=1e-300)
        m, dm = gr.prior_grad(ref.prior, x)
        m2, dm2 = pg.prior(ref, Q)
        assert np.allclose(m2[j], m, rtol=1e-14) and np.allclose(dm2[j], dm, rtol=1e-13, atol=1e-300)
    assert np.all(np.isfinite(dK[:4])) and np.all(dK[np.arange(4), np.arange(4)] == 0)        # a query on a model row: h is finite, x - X_i = 0


def test_the_entry_is_declared_exported_and_bound():
    from ibo_amd import _lib
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ibo_abi.h")).read(), flags=re.S)
    m = re.search(r"\bint\s+ibo_paths_grad_batch\s*\(([^)]*)\)", txt)
    assert m, "ibo_paths_grad_batch is not declared in ibo_abi.h"
    args = [re.sub(r"\s+", " ", a).strip() for a in m.group(1).split(",")]
    assert args == ["ibo_paths_t *p", "int64_t M", "const double *Q_host", "const int *path_of", "double *values_host", "double *grads_host"]
    assert hasattr(_lib.lib, "ibo_paths_grad_batch"), "libibo_hip.so does not export ibo_paths_grad_batch"
    assert "ibo_paths_grad_batch" in _lib.EXPORTED
    assert re.search(r"#define\s+IBO_ABI_VERSION\s+8\b", txt)
    if _lib.device_count() > 0:
        return                                       # (tests/test_gpu_paths_grad.py takes over where a GPU is visible)
    a = _lib.f64(np.zeros((4, 3))); out = np.empty(16)
    assert _lib.lib.ibo_paths_grad_batch(None, 2, _lib.dp(a), None, _lib.dp(out), _lib.dp(out)) == _lib.ERR_NO_DEVICE


def test_the_python_layer_has_the_new_names():
    from ibo_amd.acquisition import PosteriorPaths
    from ibo_amd.acquisition.gallery import thompsonSweepGallery
    for name in ("gradient", "negf_grad", "maxima"):
        assert callable(getattr(PosteriorPaths, name, None)), "PosteriorPaths.%s is missing" % name
    assert list(inspect.signature(PosteriorPaths.gradient).parameters)[1:] == ["X", "paths"]
    assert inspect.signature(PosteriorPaths.negf_grad).parameters["path"].default == 0
    assert inspect.signature(PosteriorPaths.maximize).parameters["polish"].default is False
    mx = inspect.signature(PosteriorPaths.maxima).parameters
    assert list(mx)[1:] == ["bounds", "candidates", "polish"] and mx["candidates"].default is None and mx["polish"].default is True
    tg = inspect.signature(thompsonSweepGallery).parameters
    assert tg["polish"].default is False and tg["bounds"].default is None
    import ibo_amd.acquisition.pathwise as pw
    assert "Not provided: gradients" not in pw.__doc__

"""
The NumPy restatement of the pathwise posterior draws (tests/paths_reference.py, the yardstick of tests/test_gpu_paths.py) pinned to
the joint posterior of tests/cov_reference.py, and acquisition.pathwise.spectralDraws pinned to the spectral densities.  CPU only.

The random part g of a path is linear in its standard normals for fixed (omega, phase), so its covariance G G^T is closed-form
and is compared with Sigma without sampling error: what is left is the error of the random features, which falls as 1 / sqrt(F).
Measured with these inputs, worst of eight seeds, max |G G^T - Sigma|: SE / Matern-3/2 / Matern-5/2 0.055 / 0.088 / 0.077 at
F = 1024 and 0.025 / 0.038 / 0.036 at F = 4096 -- at most 2.8 sf2 / sqrt(F); the bar, 5 sf2 / sqrt(F), is about twice that.
"""
import ctypes
import os
import re

import numpy as np
import pytest

import cov_reference as cr          # noqa: F401
import grad_reference as gr
import paths_reference as pr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["ibo_paths_create", "ibo_paths_destroy", "ibo_paths_info", "ibo_paths_coef", "ibo_paths_sweep", "ibo_paths_batch",
           "ibo_paths_direct_max"]
KINDS = {"iso": [.3], "m3": [.3, 1.0], "m5": [.3, 1.0]}


def kernel_of(kind, hyper):
    from ibo_amd.gaussianprocess import kernel as K
    return {"iso": K.GaussianKernel_iso, "sviso": K.SVGaussianKernel_iso, "m3": K.MaternKernel3,
            "m5": K.MaternKernel5}[kind](np.array(hyper, dtype=float))


def feature_error(kind, hyper, noise, F, seed, N=60, M=80, D=3):
    """max |G G^T - Sigma| of one model, one set of query points and one spectral draw"""
    from ibo_amd.acquisition.pathwise import spectralDraws
    rs = np.random.RandomState(100 + seed)
    X, Q = rs.rand(N, D), rs.rand(M, D)
    fam, w, sf2 = gr.kernel_spec(kind, hyper, D)
    ref = gr.RefGP(X, np.sin(3 * X.sum(1)), noise, fam, w, sf2)
    omega, phase, _, _ = spectralDraws(kernel_of(kind, hyper), D, F, 1, N, 1 + noise - sf2, seed)
    G = pr.g_map(ref, omega, phase, Q)
    return float(np.max(np.abs(G @ G.T - pr.latent_cov(ref, Q)))), sf2


@pytest.mark.parametrize("kind", sorted(KINDS))
def test_feature_covariance_reaches_the_joint_posterior(kind):
    worst = {}
    for F in (256, 1024, 4096):
        errs = [feature_error(kind, KINDS[kind], .01, F, seed) for seed in range(8)]
        worst[F] = max(e for e, _ in errs)
        sf2 = errs[0][1]
        print("%s F=%d: worst of 8 seeds max|G G^T - Sigma| = %.4f (bar %.4f)" % (kind, F, worst[F], 5 * sf2 / np.sqrt(F)))
    assert worst[1024] <= 5 * sf2 / np.sqrt(1024)
    assert worst[4096] <= 5 * sf2 / np.sqrt(4096)
    assert worst[4096] < worst[256]


def test_feature_covariance_when_eps_is_not_the_noise():
    """sf2 = 1.5, noise = 0.6: eps has variance 1 + noise - sf2 = 0.1"""
    for F in (1024, 4096):
        err, sf2 = feature_error("sviso", [.3, np.sqrt(1.5)], .6, F, 0)
        print("sviso sf2=%.2f F=%d: max|G G^T - Sigma| = %.4f (bar %.4f)" % (sf2, F, err, 5 * sf2 / np.sqrt(F)))
        assert abs(sf2 - 1.5) < 1e-12
        assert err <= 5 * sf2 / np.sqrt(F)


def test_paths_interpolate_noise_free_data():
    from ibo_amd.acquisition.pathwise import spectralDraws
    rs = np.random.RandomState(5)
    X = rs.rand(12, 2); Y = np.sin(3 * X.sum(1))
    fam, w, sf2 = gr.kernel_spec("iso", [.3], 2)
    ref = gr.RefGP(X, Y, 1e-8, fam, w, sf2)
    omega, phase, wts, eps = spectralDraws(kernel_of("iso", [.3]), 2, 512, 6, 12, 1e-8, 3)
    c = pr.coef(ref, omega, phase, wts, np.zeros_like(eps))
    v = pr.values(ref, omega, phase, c, X)
    print("noise-free interpolation: worst |path(X_i) - Y_i| = %.3g" % float(np.max(np.abs(v - Y[None, :]))))
    assert v.shape == (6, 12)
    assert np.max(np.abs(v - Y[None, :])) <= 1e-5
    away = pr.values(ref, omega, phase, c, rs.rand(5, 2) + 3.0)          # far from the data the paths are prior draws: they differ
    assert np.min(np.std(away, axis=0)) > 1e-3


def test_spectral_draws_are_deterministic_and_student_t():
    from scipy import stats
    from ibo_amd.acquisition.pathwise import spectralDraws
    k = kernel_of("m5", [.4, 1.0])
    a = spectralDraws(k, 3, 64, 5, 7, .1, 42); b = spectralDraws(k, 3, 64, 5, 7, .1, 42); c = spectralDraws(k, 3, 64, 5, 7, .1, 43)
    assert [x.shape for x in a] == [(64, 3), (64,), (5, 64), (5, 7)]
    assert all(np.array_equal(x, y) for x, y in zip(a, b)) and not np.array_equal(a[0], c[0])
    assert np.all(a[1] >= 0) and np.all(a[1] < 2 * np.pi)
    with pytest.raises(ValueError):
        spectralDraws(k, 3, 64, 5, 7, -.1, 42)
    D, theta = 2, .4
    for kind, nu2 in (("m3", 3.0), ("m5", 5.0)):
        om = np.r_[spectralDraws(kernel_of(kind, [theta, 1.0]), D, 10000, 1, 1, 0.0, 0)[0],
                   spectralDraws(kernel_of(kind, [theta, 1.0]), D, 10000, 1, 1, 0.0, 1)[0]]
        got = float(np.median(np.linalg.norm(om, axis=1) * theta))
        want = float(np.sqrt(D * stats.f(D, nu2).median()))               # |omega|^2 theta^2 / D ~ F(D, 2 nu)
        print("%s: median |omega| theta = %.4f, Student-t %.4f" % (kind, got, want))
        assert abs(got - want) <= .03 * want
    om = spectralDraws(kernel_of("iso", [theta]), D, 10000, 1, 1, 0.0, 0)[0]
    assert abs(np.median(np.linalg.norm(om, axis=1) * theta) - np.sqrt(stats.chi2(D).median())) <= .03 * np.sqrt(stats.chi2(D).median())


def test_symbols_are_declared_exported_and_bound():
    from ibo_amd import _lib
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ibo_abi.h")).read(), flags=re.S)
    for s in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % s, txt), "%s is not declared in ibo_abi.h" % s
        assert hasattr(_lib.lib, s), "libibo_hip.so does not export %s" % s
        assert s in _lib.EXPORTED
    assert re.search(r"#define\s+IBO_PATHS_MAX_PATHS\s+256\b", txt)
    assert re.search(r"#define\s+IBO_PATHS_MAX_FEATURES\s+16384\b", txt)
    assert re.search(r"#define\s+IBO_ABI_VERSION\s+8\b", txt)
    from ibo_amd.acquisition import PosteriorPaths, spectralDraws            # noqa: F401
    from ibo_amd.acquisition.gallery import thompsonSweepGallery            # noqa: F401
    if _lib.device_count() > 0:
        return                                       # (tests/test_gpu_paths.py takes over where a GPU is visible)
    a = _lib.f64(np.zeros((4, 3))); out = np.empty(8); lb = _lib.f64(np.zeros(3)); ub = _lib.f64(np.ones(3))
    h = ctypes.c_void_p(); bv = ctypes.c_double(); bi = ctypes.c_int64(); n = ctypes.c_int()
    L = _lib.lib
    assert L.ibo_paths_create(None, 4, _lib.dp(a), _lib.dp(out), 1, _lib.dp(out), _lib.dp(out), ctypes.byref(h)) == _lib.ERR_NO_DEVICE
    assert L.ibo_paths_destroy(None) == _lib.ERR_NO_DEVICE
    assert L.ibo_paths_info(None, ctypes.byref(n), None, None, None, None) == _lib.ERR_NO_DEVICE
    assert L.ibo_paths_coef(None, _lib.dp(out)) == _lib.ERR_NO_DEVICE
    assert L.ibo_paths_sweep(None, 2, None, 0, None, ctypes.byref(bv), ctypes.byref(bi)) == _lib.ERR_NO_DEVICE
    assert L.ibo_paths_batch(None, 2, _lib.dp(a), _lib.dp(out)) == _lib.ERR_NO_DEVICE
    assert L.ibo_paths_direct_max(None, 0, 3, _lib.dp(lb), _lib.dp(ub), 5, 5, 100, 0, ctypes.byref(bv), _lib.dp(out), None) == _lib.ERR_NO_DEVICE

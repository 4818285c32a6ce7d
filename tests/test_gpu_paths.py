"""
ibo_paths_* (pathwise posterior draws) and what is built on them: acquisition.pathwise (PosteriorPaths, spectralDraws) and
gallery.thompsonSweepGallery.

The yardstick is tests/paths_reference.py (NumPy float64, the cosine's argument in long double), pinned by
tests/test_paths_reference.py.  With T = |m| + sum_j |phi_j w_j| + sum_i |k*_i c_i| per (path, point):
    composition   device values against the restatement evaluated on the device's OWN coefficients (ibo_paths_coef): 1e-11 T --
                  indexing, padding, the cosine, k*
    end to end    device values against the restatement's own coefficients: 1e-6 T, the project's posterior bar (noise >= 1e-2);
                  the coefficients themselves at 1e-6 max |c|
Everything else is exact: one route (bit-equal values from any entry, chunking and position), the arg-max rule, DIRECT, snapshots.
"""
import ctypes
import functools

import numpy as np
import pytest

import grad_reference as gr
import paths_reference as pr
import test_gpu_posterior_cov as pc
from conftest import synth

pytestmark = pytest.mark.gpu

NOISE = .1
GUARD = 7.25

CASES = [  # kind, D, N, F, S, M, prior, shift
    ("ard", 1, 1, 1, 1, 1, False, 0.0),
    ("iso", 3, 63, 31, 3, 63, False, 0.0),
    ("svard", 3, 64, 32, 64, 64, False, 0.0),            # an SV kernel: sf2 = 0.81
    ("sviso", 8, 65, 33, 65, 65, False, 0.0),
    ("m3", 3, 130, 100, 100, 255, False, 0.0),
    ("m5", 8, 2100, 2048, 3, 256, False, 0.0),
    ("ard", 33, 130, 100, 64, 257, False, 0.0),
    ("iso", 64, 65, 100, 65, 1000, False, 0.0),
    ("m5", 3, 130, 100, 65, 257, True, 0.0),             # a trained mean prior: 63 paths per column tile
    ("ard", 3, 130, 2048, 64, 1000, False, 1000.0),      # data a thousand units from the origin
    ("m3", 64, 64, 31, 1, 64, False, 0.0),
    ("svard", 8, 63, 33, 64, 1, True, 0.0),
]


@pytest.fixture(scope="module")
def lib():
    from ibo_amd import _lib
    if _lib.device_count() < 1:
        pytest.fail("no GPU visible: the product has no CPU fallback")
    return _lib


class Paths(object):
    """a raw ibo_paths_t handle"""

    def __init__(self, lib, GP, omega, phase, w, eps):
        self.lib, self.S, self.F, self.N, self.D = lib, len(w), len(phase), eps.shape[1], omega.shape[1]
        GP._push_prior()
        h = ctypes.c_void_p()
        lib.check(lib.lib.ibo_paths_create(GP._handle(), self.F, lib.dp(omega), lib.dp(phase), self.S, lib.dp(w), lib.dp(eps), ctypes.byref(h)))
        self.h = h

    def coef(self):
        out = np.full(self.S * (self.F + self.N) + 8, GUARD)
        self.lib.check(self.lib.lib.ibo_paths_coef(self.h, self.lib.dp(out)))
        assert np.all(out[-8:] == GUARD)
        return out[:-8].reshape(self.S, self.F + self.N)

    def batch(self, Q):
        Q = self.lib.f64(np.atleast_2d(Q))
        out = np.full(self.S * len(Q) + 8, GUARD)
        self.lib.check(self.lib.lib.ibo_paths_batch(self.h, len(Q), self.lib.dp(Q), self.lib.dp(out)))
        assert np.all(out[-8:] == GUARD), "guard behind the values overwritten"
        return out[:-8].reshape(self.S, len(Q))

    def sweep(self, cand, M=None, index_base=0, values=True):
        """cand: a DeviceArray (or a view of one) -> (best_val (S,), best_idx (S,), values (S, M) or None)"""
        from ibo_amd import DeviceArray
        M = cand.shape[0] if M is None else M
        vals = DeviceArray((self.S * M + 8,)) if values else None
        if values:
            vals.upload(np.full(self.S * M + 8, GUARD))
        bv = np.full(self.S + 1, GUARD); bi = np.full(self.S + 1, 77, dtype=np.int64)
        self.lib.check(self.lib.lib.ibo_paths_sweep(self.h, M, cand.ptr, index_base, vals.ptr if values else None, self.lib.dp(bv),
                                                    bi.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))))
        assert bv[-1] == GUARD and bi[-1] == 77
        v = None
        if values:
            v = vals.to_host()
            assert np.all(v[-8:] == GUARD), "guard behind values_dev overwritten"
            v = v[:-8].reshape(self.S, M)
        return bv[:-1], bi[:-1], v

    def close(self):
        if self.h is not None:
            self.lib.check(self.lib.lib.ibo_paths_destroy(self.h))
            self.h = None


def model(kind, D, N, prior=False, shift=0.0, noise=NOISE, seed=1):
    from ibo_amd.gaussianprocess import GaussianProcess
    X, Y = synth(seed, N, D)
    X = X + shift
    hyper = pc.hyper_of(kind, D)
    p = pc.make_prior(D) if prior else None
    fam, w, sf2 = gr.kernel_spec(kind, hyper, D)
    tup = (p.means, p.beta, p.theta, p.lowerb, p.width) if prior else None
    return GaussianProcess(pc.make_kernel(kind, hyper), X, Y, prior=p, noise=noise), gr.RefGP(X, Y, noise, fam, w, sf2, prior=tup)


def draws(GP, ref, F, S, seed=7):
    from ibo_amd.acquisition import spectralDraws
    N, D = ref.X.shape
    return spectralDraws(GP.kernel, D, F, S, N, 1 + ref.noise - ref.sf2, seed)


@functools.lru_cache(maxsize=None)
def case_data(case):
    """one case: the device's coefficients and values and the restatement's, computed once for the tests that read them"""
    from ibo_amd import _lib
    kind, D, N, F, S, M, prior, shift = case
    GP, ref = model(kind, D, N, prior, shift)
    arrs = draws(GP, ref, F, S)
    P = Paths(_lib, GP, *arrs)
    Q = pc.queries(ref.X - shift, M) + shift
    got = dict(coef=P.coef(), values=P.batch(Q))
    P.close()
    omega, phase, w, eps = arrs
    c_ref = pr.coef(ref, omega, phase, w, eps)
    want = dict(coef=c_ref, values=pr.values(ref, omega, phase, c_ref, Q), T=pr.terms_scale(ref, omega, phase, c_ref, Q),
                own=pr.values(ref, omega, phase, got["coef"], Q), T_own=pr.terms_scale(ref, omega, phase, got["coef"], Q))
    return got, want


def close(got, want, tol, what):
    err = np.abs(np.asarray(got) - want)
    print("%s: worst error / bar = %.3g" % (what, float(np.max(err / tol))))
    assert np.all(err <= tol), "%s: worst %g of its bar" % (what, float(np.max(err / tol)))


@pytest.mark.parametrize("case", CASES)
def test_values_against_the_composition_of_their_own_coefficients(lib, case):
    got, want = case_data(case)
    assert got["values"].shape == (case[4], case[5]) and np.all(np.isfinite(got["values"]))
    close(got["values"], want["own"], 1e-11 * want["T_own"], "composition %s" % (case,))


@pytest.mark.parametrize("case", CASES)
def test_values_and_coefficients_end_to_end(lib, case):
    got, want = case_data(case)
    F = case[3]
    assert np.array_equal(got["coef"][:, :F], want["coef"][:, :F])               # the feature weights come back as they went in
    close(got["coef"][:, F:], want["coef"][:, F:], 1e-6 * np.max(np.abs(want["coef"][:, F:])), "coefficients %s" % (case,))
    close(got["values"], want["values"], 1e-6 * want["T"], "end to end %s" % (case,))


def test_info_and_errors(lib):
    GP, ref = model("ard", 3, 20)
    arrs = draws(GP, ref, 40, 5)
    P = Paths(lib, GP, *arrs)
    n = [ctypes.c_int() for _ in range(5)]
    lib.check(lib.lib.ibo_paths_info(P.h, *[ctypes.byref(x) for x in n]))
    assert [x.value for x in n] == [5, 40, 20, 3, GP._dev.device]
    L, dp = lib.lib, lib.dp
    omega, phase, w, eps = arrs
    h = ctypes.c_void_p(); out = np.empty(64); lb, ub = lib.f64(np.zeros(3)), lib.f64(np.ones(3)); bv = ctypes.c_double()
    g = GP._handle()
    assert L.ibo_paths_create(None, 40, dp(omega), dp(phase), 5, dp(w), dp(eps), ctypes.byref(h)) == lib.ERR_ARG
    assert L.ibo_paths_create(g, 40, None, dp(phase), 5, dp(w), dp(eps), ctypes.byref(h)) == lib.ERR_ARG
    assert L.ibo_paths_create(g, 40, dp(omega), dp(phase), 5, dp(w), dp(eps), None) == lib.ERR_ARG
    assert L.ibo_paths_create(g, 0, dp(omega), dp(phase), 5, dp(w), dp(eps), ctypes.byref(h)) == lib.ERR_ARG
    assert L.ibo_paths_create(g, 16385, dp(omega), dp(phase), 5, dp(w), dp(eps), ctypes.byref(h)) == lib.ERR_ARG
    assert L.ibo_paths_create(g, 40, dp(omega), dp(phase), 0, dp(w), dp(eps), ctypes.byref(h)) == lib.ERR_ARG
    assert L.ibo_paths_create(g, 40, dp(omega), dp(phase), 257, dp(w), dp(eps), ctypes.byref(h)) == lib.ERR_ARG
    fresh = ctypes.c_void_p()
    lib.check(L.ibo_gp_create(GP._dev.device, ctypes.byref(fresh)))
    assert L.ibo_paths_create(fresh, 40, dp(omega), dp(phase), 5, dp(w), dp(eps), ctypes.byref(h)) == lib.ERR_STATE
    lib.check(L.ibo_gp_destroy(fresh))
    assert L.ibo_paths_batch(P.h, 0, dp(out), dp(out)) == lib.ERR_ARG
    assert L.ibo_paths_batch(P.h, 1, None, dp(out)) == lib.ERR_ARG
    assert L.ibo_paths_sweep(P.h, 1, None, 0, None, dp(out), None) == lib.ERR_ARG
    assert L.ibo_paths_direct_max(P.h, 5, 3, dp(lb), dp(ub), 5, 5, 100, 0, ctypes.byref(bv), dp(out), None) == lib.ERR_ARG
    assert L.ibo_paths_direct_max(P.h, -1, 3, dp(lb), dp(ub), 5, 5, 100, 0, ctypes.byref(bv), dp(out), None) == lib.ERR_ARG
    assert L.ibo_paths_direct_max(P.h, 0, 2, dp(lb), dp(ub), 5, 5, 100, 0, ctypes.byref(bv), dp(out), None) == lib.ERR_ARG
    assert L.ibo_paths_direct_max(P.h, 0, 3, dp(lb), dp(ub), 5, 5, 100, 0, None, None, None) == lib.ERR_ARG
    assert L.ibo_set_option(b"paths_chunk", -1) == lib.ERR_ARG
    assert P.batch(ref.X[:2]).shape == (5, 2)                                   # the object is still usable
    P.close()


@pytest.mark.parametrize("prior", [False, True])
def test_one_route_gives_one_set_of_bits(lib, prior):
    from ibo_amd import DeviceArray
    GP, ref = model("m5", 3, 70, prior)
    S = 66
    P = Paths(lib, GP, *draws(GP, ref, 50, S))
    Q = pc.queries(ref.X, 300, seed=9)
    whole = P.batch(Q)
    for step in (1, 7, 64, 65):
        parts = np.concatenate([P.batch(Q[i:i + step]) for i in range(0, 300, step)], axis=1)
        assert np.array_equal(parts, whole), "calls of %d points" % step
    rs = np.random.RandomState(4)
    C = rs.rand(1000, 3)
    C[3:303] = Q; C[650:950] = Q
    dev = DeviceArray.from_host(C)
    try:
        lib.check(lib.lib.ibo_set_option(b"paths_chunk", 256))
        _, _, v = P.sweep(dev)
        _, _, v2 = P.sweep(dev.view_rows(650, 950))
    finally:
        lib.check(lib.lib.ibo_set_option(b"paths_chunk", 0))
    _, _, v3 = P.sweep(dev)
    assert np.array_equal(v[:, 3:303], whole) and np.array_equal(v[:, 650:950], whole) and np.array_equal(v2, whole)
    assert np.array_equal(v3, v)
    P.close()


def test_argmax_first_index_ties_nan_and_index_base(lib):
    from ibo_amd import DeviceArray
    GP, ref = model("ard", 3, 40)
    S, M = 65, 1000
    P = Paths(lib, GP, *draws(GP, ref, 64, S))
    rs = np.random.RandomState(12)
    base = rs.rand(M, 3) * 1.2 - .1
    base[0] = np.nan; base[500, 1] = np.nan
    dev = DeviceArray.from_host(base)

    def check(C, label):
        dev.upload(C)
        bv, bi, v = P.sweep(dev, index_base=5000)
        assert np.all(np.isnan(v[:, 0])) and np.all(np.isnan(v[:, 500])), label
        assert np.all(np.isfinite(np.delete(v, [0, 500], axis=1))), label
        want = np.nanargmax(v, axis=1)                                          # (the first of equals)
        assert np.array_equal(bi, want + 5000), label
        assert np.array_equal(bv, v[np.arange(S), want]), label
        bv2, bi2, _ = P.sweep(dev, index_base=5000, values=False)
        assert np.array_equal(bv2, bv) and np.array_equal(bi2, bi), label
        return bv, bi, v

    try:
        lib.check(lib.lib.ibo_set_option(b"paths_chunk", 256))
        _, bi, _ = check(base, "plain")
        # exact ties: a path's winning row copied to both sides of a 64-row seam, of a 256-row chunk seam, and far apart
        for s, (pa, pb) in ((0, (63, 64)), (64, (255, 256)), (31, (511, 768)), (63, (257, 999))):
            k = int(bi[s]) - 5000
            C = base.copy()
            C[k] = base[(k + 7) % M] if (k + 7) % M not in (0, 500) else base[1]
            C[pa] = base[k]; C[pb] = base[k]
            _, bi_t, v_t = check(C, "tie of path %d at %s" % (s, (pa, pb)))
            assert v_t[s, pa] == v_t[s, pb] == np.nanmax(v_t[s])                   # the bits do not depend on the position
            assert bi_t[s] == 5000 + pa
    finally:
        lib.check(lib.lib.ibo_set_option(b"paths_chunk", 0))
    dev.upload(np.full((M, 3), np.nan))
    bv, bi, v = P.sweep(dev, index_base=5000)
    assert np.all(np.isnan(v)) and np.all(bi == -1) and np.all(bv == -np.inf)
    P.close()


def test_direct_equals_the_host_tree_on_single_points(lib):
    GP, ref = model("iso", 2, 40)
    P = Paths(lib, GP, *draws(GP, ref, 128, 3))
    path, D = 2, 2
    lb, ub = lib.f64(np.zeros(D)), lib.f64(np.ones(D))
    opt = ctypes.c_double(); optx = np.empty(D); ns = ctypes.c_int64()
    lib.check(lib.lib.ibo_paths_direct_max(P.h, path, D, lib.dp(lb), lib.dp(ub), 12, 30, 10000, 1, ctypes.byref(opt), lib.dp(optx),
                                           ctypes.byref(ns)))
    val = np.empty(3)

    def negval(nd, x):
        q = lib.f64([x[i] for i in range(nd)])
        assert lib.lib.ibo_paths_batch(P.h, 1, lib.dp(q), lib.dp(val)) == 0
        return -val[path]
    cb = lib.OBJECTIVE(negval)
    fm = ctypes.c_double(); xm = np.empty(D); n2 = ctypes.c_int64()
    lib.check(lib.lib.ibo_direct_host(cb, D, lib.dp(lb), lib.dp(ub), 12, 30, 10000, 1, ctypes.byref(fm), lib.dp(xm), ctypes.byref(n2)))
    assert ns.value == n2.value and ns.value > 50
    assert np.array_equal(optx, xm) and opt.value == -fm.value
    assert P.batch(optx)[path, 0] == opt.value
    P.close()


def test_a_path_object_is_a_snapshot(lib):
    from ibo_amd.acquisition import PosteriorPaths
    GP, ref = model("m3", 3, 30, prior=True)
    Q = pc.queries(ref.X, 70, seed=3)
    P = PosteriorPaths(GP, n_paths=5, n_features=96, seed=11)
    before, coef = P.values(Q), P.coef()
    GP.addData(np.full(3, .5), 1.25)
    assert np.array_equal(P.values(Q), before)
    GP.removeData([0, 4])
    assert np.array_equal(P.values(Q), before)
    later = PosteriorPaths(GP, n_paths=5, n_features=96, seed=11)               # the same draws on the changed model: other paths
    assert later.N == 29 and not np.array_equal(later.values(Q)[:, :5], before[:, :5])
    later.close()
    GP._dev.close()
    del GP
    assert np.array_equal(P.values(Q), before) and np.array_equal(P.coef(), coef)
    P.close()
    with pytest.raises(ValueError):
        P.values(Q)


def test_sample_statistics_of_the_device_paths(lib):
    """S = 256 paths from F = 4096 features on a 40-row model at 30 points: the sample mean against mu and the sample covariance
    against Sigma, each within 6 standard errors of the restatement's own path covariance G G^T (exact for these features) plus,
    for the covariance, the features' 5 sf2 / sqrt(F) of tests/test_paths_reference.py."""
    GP, ref = model("iso", 3, 40)
    S, F = 256, 4096
    arrs = draws(GP, ref, F, S, seed=21)
    omega, phase, w, eps = arrs
    Q = pc.queries(ref.X, 30, seed=6)
    C = pr.g_map(ref, omega, phase, Q); C = C @ C.T
    mu = pr.values(ref, omega, phase, np.c_[np.zeros((1, F)), ref.aY[None, :]], Q)[0]
    Sigma = pr.latent_cov(ref, Q)
    se_mean = np.sqrt(np.diag(C) / S)
    se_cov = np.sqrt((np.outer(np.diag(C), np.diag(C)) + C ** 2) / (S - 1))

    def check(V, what):
        dm = np.abs(V.mean(axis=0) - mu) / se_mean
        dc = np.abs(np.cov(V.T) - Sigma) / (6 * se_cov + 5 * ref.sf2 / np.sqrt(F))
        print("%s: worst mean error %.2f standard errors, worst covariance error %.2f of its bar" % (what, dm.max(), dc.max()))
        assert dm.max() <= 6 and dc.max() <= 1, what

    check(pr.values(ref, omega, phase, pr.coef(ref, omega, phase, w, eps), Q), "restatement")      # (fails: the inputs are wrong, not the kernel)
    P = Paths(lib, GP, *arrs)
    check(P.batch(Q), "device")
    P.close()


def test_python_layer_agrees_with_the_raw_entries(lib):
    from ibo_amd import DeviceArray
    from ibo_amd.acquisition import PosteriorPaths
    GP, ref = model("svard", 2, 50)
    P = PosteriorPaths(GP, n_paths=4, n_features=200, seed=5)
    again = PosteriorPaths(GP, n_paths=4, n_features=200, seed=5)
    raw = Paths(lib, GP, P.omega, P.phase, P.w, P.eps)
    rs = np.random.RandomState(8)
    C = rs.rand(700, 2)
    assert P.values(C).shape == (4, 700) and P.values(C[0]).shape == (4, 1) and P.coef().shape == (4, 250)
    assert np.array_equal(P.values(C), raw.batch(C)) and np.array_equal(again.values(C), P.values(C))
    assert np.array_equal(P.coef(), raw.coef())
    dev = DeviceArray.from_host(C)
    bv, bi, v = raw.sweep(dev, index_base=10)
    for cand in (C, dev):
        r = P.sweep(cand, index_base=10, outputs=True)
        assert np.array_equal(r["best_val"], bv) and np.array_equal(r["best_idx"], bi) and np.array_equal(r["values"], v)
    assert sorted(P.sweep(C)) == ["best_idx", "best_val"]
    assert np.array_equal(v, P.values(C))
    opt, optx = P.maximize([[0., 1.]] * 2, path=3, maxiter=10)
    o = ctypes.c_double(); ox = np.empty(2)
    lb, ub = lib.f64(np.zeros(2)), lib.f64(np.ones(2))
    lib.check(lib.lib.ibo_paths_direct_max(raw.h, 3, 2, lib.dp(lb), lib.dp(ub), 10, 30, 10000, 0, ctypes.byref(o), lib.dp(ox), None))
    assert opt == o.value and np.array_equal(optx, ox) and P.values(optx)[3, 0] == opt
    with pytest.raises(ValueError):
        P.values(np.zeros((3, 5)))
    with pytest.raises(ValueError):
        P.maximize([[0., 1.]] * 3)
    with pytest.raises(ValueError):
        P.maximize([[0., 1.]] * 2, path=4)
    for x in (P, again, raw):
        x.close()


def test_thompson_sweep_gallery(lib):
    from ibo_amd import DeviceArray
    from ibo_amd.acquisition.gallery import thompsonSweepGallery, MIN_SEPARATION
    GP, ref = model("ard", 3, 25)
    C = np.random.RandomState(2).rand(3000, 3)
    g1 = thompsonSweepGallery(GP, C, 4, seed=3, n_features=256)
    g2 = thompsonSweepGallery(GP, DeviceArray.from_host(C), 4, seed=3, n_features=256)
    g3 = thompsonSweepGallery(GP, C, 4, seed=4, n_features=256)
    assert len(g1) == 4 and all(np.array_equal(a, b) for a, b in zip(g1, g2))
    assert not all(np.array_equal(a, b) for a, b in zip(g1, g3))
    for i, x in enumerate(g1):
        assert np.any(np.all(C == x, axis=1))                                   # a row of the candidate array
        for y in g1[:i]:
            assert np.linalg.norm(x - y) > MIN_SEPARATION
    assert 1 <= len(thompsonSweepGallery(GP, C, 50, seed=3, paths=3, n_features=64)) <= 3


def test_refusals(lib):
    from ibo_amd.acquisition import PosteriorPaths
    from ibo_amd.gaussianprocess import GaussianProcess, PrefGaussianProcess
    from ibo_amd.gaussianprocess.kernel import GaussianKernel_ard, SVGaussianKernel_iso
    with pytest.raises(NotImplementedError):
        PosteriorPaths(PrefGaussianProcess(GaussianKernel_ard(np.array([.5, .5]))))
    with pytest.raises(ValueError):
        PosteriorPaths(GaussianProcess(GaussianKernel_ard(np.array([.5, .5]))))
    GP, _ = model("ard", 2, 10)
    GP._augdev = object()                                                       # what addObservationPoint leaves in force
    try:
        with pytest.raises(NotImplementedError):
            PosteriorPaths(GP)
    finally:
        GP._augdev = None
    X = np.array([[0., 0.], [1., 0.], [0., 1.], [1., 1.]])
    big = GaussianProcess(SVGaussianKernel_iso(np.array([.1, 1.1])), X, np.arange(4.0), noise=.1)      # sf2 = 1.21 > 1 + noise
    with pytest.raises(ValueError):
        PosteriorPaths(big)
    with pytest.raises(ValueError):
        PosteriorPaths(GP, n_paths=257)
    with pytest.raises(ValueError):
        PosteriorPaths(GP, n_features=16385)

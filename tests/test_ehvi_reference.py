"""
The NumPy restatement of the two-objective expected hypervolume improvement (tests/ehvi_reference.py, the yardstick of
tests/test_gpu_ehvi.py) pinned: the empty front to the oracle's EI, the formula to a quadrature of the hypervolume difference, the
sum to a long-double evaluation, the gradient to central differences of its own values; paretoFront / hypervolume against brute
force; the generator of the GPU comparison checked for being worth comparing on; the front's canonical form in the library's
header against the restatement's; and the four ibo_ehvi_* symbols.  CPU only.
"""
import ctypes
import os
import re

import mpmath
import numpy as np
import pytest

from conftest import ROOT, synth
from oracle import oracle as orc
import grad_reference as gr
import cacq_reference as cr
import ehvi_reference as er

SYMBOLS = ("ibo_ehvi_sweep", "ibo_ehvi_batch", "ibo_ehvi_grad_batch", "ibo_ehvi_direct_max", "ibo_ehvi_scan_ms")
ERFS = [gr.ERF_LIBM, gr.ERF_NR]

# raw fronts for the formula's checks: canonical sizes 1, 2 and 7, with dominated points, duplicates and points below ref
REF = np.array([-.4, -.3])
FRONTS = {1: np.array([[.5, .6], [.2, .3], [.5, .6], [-.4, 2.], [3., -.5], [-1., -1.]]),
          2: np.array([[.1, .9], [.8, .2], [.05, .5], [.8, .2], [.7, .1], [-.5, .4]]),
          7: np.r_[er.curve_front(7, REF, np.array([1.2, 1.1]))]}
# posteriors (mu1, sigma1, mu2, sigma2) on, inside, across and far above the fronts
POSTERIORS = [(.3, .4, .2, .5), (.9, .15, .8, .1), (-.2, .6, .5, .05), (1.6, .3, 1.4, .7)]


def two_models(kind1="m5", hyper1=(.5, .9), kind2="ard", hyper2=(.3, .5, .4), with_prior=False):
    """two models observed at OTHER points, as (oracle GP, restatement) pairs"""
    out = []
    for (seed, N), kind, hyper in (((5, 40), kind1, list(hyper1)), ((6, 33), kind2, list(hyper2))):
        X, Y = synth(seed, N, 3)
        if seed == 6:
            Y = np.cos(2 * X[:, 0]) - X[:, -1]
        prior = oprior = None
        if with_prior and seed == 5:
            rs = np.random.RandomState(7)
            prior = (rs.rand(4, 3), rs.randn(4), 2.0, np.zeros(3) - .1, np.full(3, 1.2))
            oprior = orc.Prior(*prior)
        out.append((orc.GP(orc.Kern(kind, hyper), X, Y, noise=.1, prior=oprior), cr.make(X, Y, .1, kind, hyper, prior=prior)))
    return out


# ------------------------------------------------------------------------------------------------ (a) the empty front
@pytest.mark.parametrize("erf_mode", ERFS)
@pytest.mark.parametrize("with_prior", [False, True])
def test_empty_front_is_the_product_of_the_oracles_two_ei(erf_mode, with_prior):
    (o1, m1), (o2, m2) = two_models(with_prior=with_prior)
    Q = np.random.RandomState(3).rand(40, 3) * 1.2 - .1
    ref = np.array([.2, -.5])
    want = np.ones(len(Q))
    for ogp, t in ((o1, ref[0]), (o2, ref[1])):
        mu, s2 = ogp.posteriors(Q)
        want = want * orc.acq_value(gr.ACQ_EI, erf_mode, mu, np.sqrt(s2), t, 0.0)
    for front in (np.empty((0, 2)), np.array([[.1, 5.], [7., -.5], [.2, -.5]])):        # nothing, and nothing strictly above ref
        got = er.value([m1, m2], Q, front, ref, erf_mode, 1e-7)
        np.testing.assert_allclose(got["val"], want, rtol=1e-6, atol=1e-300)
    assert np.all(want > 0) and np.max(want) > 1e-3


# ------------------------------------------------------------------------------------------------ (b) the hypervolume difference
def test_staircase_hvi_is_the_hypervolume_difference():
    from ibo_amd.acquisition.multiobjective import hypervolume
    rs = np.random.RandomState(11)
    for n, F in FRONTS.items():
        Y = REF + rs.rand(300, 2) * 2.2 - .3
        want = np.array([hypervolume(np.vstack([F, y[None]]), REF) - hypervolume(F, REF) for y in Y])
        np.testing.assert_allclose(er.hvi(F, REF, Y), want, rtol=0, atol=1e-14)
        assert np.mean(want > 0) > .3 and np.mean(want == 0) > .02
        assert len(er.canonical(F, REF)[0]) == n


def gauss_legendre_grid(mu, sig, kinks, order):
    """nodes and weights (density included) over mu +- 12 sigma, cut at the kinks and at every sigma: the integrand is smooth
    (bilinear times Gaussian) inside every cell"""
    lo, hi = mu - 12 * sig, mu + 12 * sig
    cuts = np.unique(np.r_[lo, hi, [k for k in kinks if lo < k < hi], mu + sig * np.arange(-11, 12)])
    x, w = np.polynomial.legendre.leggauss(order)
    nodes = np.concatenate([.5 * (b - a) * x + .5 * (a + b) for a, b in zip(cuts[:-1], cuts[1:])])
    wts = np.concatenate([.5 * (b - a) * w for a, b in zip(cuts[:-1], cuts[1:])])
    return nodes, wts * np.exp(-.5 * ((nodes - mu) / sig) ** 2) / (sig * np.sqrt(2 * np.pi))


def quadrature(F, ref, post, order):
    mu1, s1, mu2, s2 = post
    a, b = er.canonical(F, ref)
    x, wx = gauss_legendre_grid(mu1, s1, np.r_[ref[0], a], order)
    y, wy = gauss_legendre_grid(mu2, s2, np.r_[ref[1], b], order)
    G = er.hvi(F, ref, np.c_[np.repeat(x, len(y)), np.tile(y, len(x))]).reshape(len(x), len(y))
    return float(wx @ G @ wy)


@pytest.mark.parametrize("n", [1, 2, 7])
def test_formula_is_the_expected_hypervolume_difference(n):
    """E[hypervolume(F + {y}) - hypervolume(F)] by Gauss-Legendre on the cells between the integrand's kinks, orders 12 and 8.
    The bar is the quadrature's own error -- the two orders' difference -- plus 1e-12 S for the rounding of either side's sums
    (a few hundred thousand products of about S / cells each)."""
    F = FRONTS[n]
    for post in POSTERIORS:
        mu1, s1, mu2, s2 = post
        r = er.from_posterior(np.array([mu1]), np.array([s1 ** 2]), np.array([mu2]), np.array([s2 ** 2]), F, REF, gr.ERF_LIBM)
        q12, q8 = quadrature(F, REF, post, 12), quadrature(F, REF, post, 8)
        err = abs(q12 - q8) + 1e-12 * r["S"][0]
        print("n=%d post=%s formula=%.15g quadrature=%.15g own error=%.2e" % (n, post, r["val"][0], q12, abs(q12 - q8)))
        assert abs(q12 - q8) < 1e-9 * r["S"][0]                   # (the quadrature has converged: its error bar means something)
        assert abs(r["val"][0] - q12) <= err
        assert r["val"][0] > 1e-6


# ------------------------------------------------------------------------------------------------ (c) long double
def cdf_pdf_long(erf_mode, z):
    """gr.cdf_pdf in long double: libm's erf from mpmath (30 digits, rounded), NR's fit with its truncated constants as they are"""
    L = np.longdouble
    z = np.asarray(z, dtype=L)
    if erf_mode == gr.ERF_LIBM:
        with mpmath.workdps(30):
            e = np.array([L(mpmath.nstr(mpmath.erf(mpmath.mpf(float(v)) / mpmath.sqrt(2)), 25)) for v in z.ravel()], dtype=L).reshape(z.shape)
        return L(.5) * (1 + e), np.exp(-(z * z / 2)) / np.sqrt(2 * L(np.pi))
    x = z * L(0.707106)
    t = 1 / (1 + L(.5) * np.abs(x))
    p = L(0.17087277)
    for c in (-0.82215223, 1.48851587, -1.13520398, 0.27886807, -0.18628806, 0.09678418, 0.37409196, 1.00002368):
        p = L(c) + t * p
    ans = 1 - t * np.exp(-x * x - L(1.26551223) + t * p)
    return L(.5) * (1 + np.where(x >= 0, ans, -ans)), np.exp(-(z * z / 2)) * L(0.398942)


def sum_long(mu1, s21, mu2, s22, front, ref, erf_mode):
    """er.from_posterior's value with the strips summed in 80-bit arithmetic from the same float64 (mu, s2, front)"""
    L = np.longdouble
    a, b = er.canonical(front, ref)
    n, M = len(a), len(mu1)
    sig1, sig2 = np.sqrt(s21).astype(L), np.sqrt(s22).astype(L)          # (the float64 sigmas: the kernel's inputs to the walk)

    def psi(mu, sig, t):
        dm = mu.astype(L) - L(t)
        cdf, pdf = cdf_pdf_long(erf_mode, dm / sig)
        return sig * pdf + dm * cdf

    prev = psi(mu1, sig1, ref[0])
    val = np.zeros(M, dtype=L)
    for i in range(n + 1):
        nxt = psi(mu1, sig1, a[i]) if i < n else np.zeros(M, dtype=L)
        d = prev - nxt
        val = val + np.where(d < 0, 0, d) * psi(mu2, sig2, b[i] if i < n else ref[1])
        prev = nxt
    return val


@pytest.mark.parametrize("erf_mode", ERFS)
@pytest.mark.parametrize("n", [0, 2, 7, 65])
def test_the_sum_in_long_double(erf_mode, n):
    """the same strips summed in 80-bit arithmetic from the same float64 (mu, sigma, front): 1e-12 S"""
    assert np.finfo(np.longdouble).eps < 1e-18
    L = np.longdouble
    rs = np.random.RandomState(20 + n)
    F = FRONTS[n] if n in FRONTS else er.curve_front(n, REF, np.array([1.2, 1.1]))
    a, b = er.canonical(F, REF)
    assert len(a) == n
    M = 40
    mu1, mu2 = REF[0] + rs.rand(M) * 2 - .3, REF[1] + rs.rand(M) * 2 - .3
    s21, s22 = rs.rand(M) * .3 + 1e-3, rs.rand(M) * .3 + 1e-3
    r = er.from_posterior(mu1, s21, mu2, s22, F, REF, erf_mode)
    val = sum_long(mu1, s21, mu2, s22, F, REF, erf_mode)
    err = np.abs(r["val"].astype(L) - val).astype(float)
    print("n=%d erf=%d: worst |err| / S = %.2e" % (n, erf_mode, np.max(err / r["S"])))
    assert np.all(err <= 1e-12 * r["S"])
    assert np.mean(r["val"] > 1e-9) > .5


# ------------------------------------------------------------------------------------------------ (d) the gradient
@pytest.mark.parametrize("n", [0, 2, 7])
@pytest.mark.parametrize("kinds", [("m5", (.5, .9), "ard", (.3, .5, .4)), ("iso", (.4,), "m3", (.5, .95)), ("sviso", (.4, .8), "m5", (.6, .9))])
def test_gradient_matches_central_differences_of_the_restatement(kinds, n):
    """h = 1e-5, agreement 1e-6 of the scale; the libm flavour only (NR's truncated constants make the analytic gradient differ
    from the derivative of the values by about 1e-6, see ibo_abi.h)"""
    (_, m1), (_, m2) = two_models(*kinds, with_prior=True)
    Q = np.random.RandomState(8).rand(10, 3)
    ref = np.array([-.6, -1.2])
    F = er.curve_front(n, ref, np.array([.9, .8]))
    g = er.value_grad([m1, m2], Q, F, ref, gr.ERF_LIBM, 1e-7)
    np.testing.assert_allclose(g["val"], er.value([m1, m2], Q, F, ref, gr.ERF_LIBM, 1e-7)["val"], rtol=0, atol=1e-11 * np.max(g["S"]))
    h = 1e-5
    num = np.zeros(Q.shape)
    for d in range(Q.shape[1]):
        E = np.zeros(Q.shape); E[:, d] = h
        num[:, d] = (er.value([m1, m2], Q + E, F, ref, gr.ERF_LIBM, 1e-7)["val"] -
                     er.value([m1, m2], Q - E, F, ref, gr.ERF_LIBM, 1e-7)["val"]) / (2 * h)
    assert np.max(np.abs(g["dval"])) > 1e-3
    gr.assert_grad_close(g["dval"], num, g["sval"], rel=1e-6, atol=1e-13, what="%s n=%d" % (kinds[0], n))


def test_partial_sums_are_the_derivatives_of_the_value():
    """dEHVI/dmu_k = G_mu_k and dEHVI/dsigma_k = G_sigma_k by central differences in the posterior itself: h = 1e-6, bar 1e-7 --
    rounding eps S / h is about 1e-10, truncation h^2 |f'''| / 6 with sigma >= 0.05 at most about 1e-8"""
    rs = np.random.RandomState(9)
    F = FRONTS[7]
    M = 30
    mu1, mu2 = REF[0] + rs.rand(M) * 2 - .3, REF[1] + rs.rand(M) * 2 - .3
    s1, s2 = rs.rand(M) * .5 + .05, rs.rand(M) * .5 + .05
    r = er.from_posterior(mu1, s1 ** 2, mu2, s2 ** 2, F, REF)
    h = 1e-6
    f = lambda a, b, c, d: er.from_posterior(a, b ** 2, c, d ** 2, F, REF)["val"]
    for key, num in (("gm1", (f(mu1 + h, s1, mu2, s2) - f(mu1 - h, s1, mu2, s2)) / (2 * h)),
                     ("gs1", (f(mu1, s1 + h, mu2, s2) - f(mu1, s1 - h, mu2, s2)) / (2 * h)),
                     ("gm2", (f(mu1, s1, mu2 + h, s2) - f(mu1, s1, mu2 - h, s2)) / (2 * h)),
                     ("gs2", (f(mu1, s1, mu2, s2 + h) - f(mu1, s1, mu2, s2 - h)) / (2 * h))):
        np.testing.assert_allclose(r[key], num, rtol=0, atol=1e-7)
    assert np.max(np.abs(r["gs1"])) > 1e-2 and np.max(np.abs(r["gm2"])) > 1e-2
    # never more than the bound the end-to-end tolerance uses: 0 <= G_mu1 <= psi_2(r2), 0 <= G_mu2 <= psi_1(r1)
    p1, p2 = er.psi(gr.ERF_LIBM, mu1, s1, REF[0])[0], er.psi(gr.ERF_LIBM, mu2, s2, REF[1])[0]
    assert np.all(r["gm1"] >= -1e-15) and np.all(r["gm1"] <= p2 * (1 + 1e-12))
    assert np.all(r["gm2"] >= -1e-15) and np.all(r["gm2"] <= p1 * (1 + 1e-12))


# ------------------------------------------------------------------------------------------------ (e) fronts and areas
def test_pareto_front_and_hypervolume_against_brute_force():
    from ibo_amd.acquisition.multiobjective import paretoFront, hypervolume
    rs = np.random.RandomState(12)
    for trial in range(200):
        n = rs.randint(0, 13)
        Y = np.round(rs.rand(n, 2) * 6) / 6 if trial % 2 else rs.rand(n, 2)          # (every other set on a grid: ties and duplicates)
        ref = rs.rand(2) * .5
        keep = [y for y in Y if not np.any(np.all(Y >= y, axis=1) & np.any(Y > y, axis=1))]
        want = np.unique(np.array(keep).reshape(-1, 2), axis=0)
        got = paretoFront(Y)
        assert got.shape == want.shape and np.array_equal(got, want)
        assert np.all(np.diff(got[:, 0]) > 0) and np.all(np.diff(got[:, 1]) < 0)
        # the area of the union of the boxes, cell by cell on the grid of all coordinates
        xs, ys = np.unique(np.r_[ref[0], Y[:, 0]]), np.unique(np.r_[ref[1], Y[:, 1]])
        area = 0.0
        for x0, x1 in zip(xs[:-1], xs[1:]):
            for y0, y1 in zip(ys[:-1], ys[1:]):
                if x0 >= ref[0] and y0 >= ref[1] and np.any((Y[:, 0] >= x1) & (Y[:, 1] >= y1)):
                    area += (x1 - x0) * (y1 - y0)
        assert abs(hypervolume(Y, ref) - area) <= 1e-13
        a, b = er.canonical(Y, ref)
        inside = got[(got[:, 0] > ref[0]) & (got[:, 1] > ref[1])]
        assert np.array_equal(np.c_[a, b].reshape(-1, 2), inside)
    assert paretoFront(np.empty((0, 2))).shape == (0, 2) and hypervolume(np.empty((0, 2)), [0, 0]) == 0.0


def test_observed_front_needs_joint_observations():
    from ibo_amd.acquisition.multiobjective import observedFront, paretoFront

    class Stub(object):
        def __init__(self, X, Y):
            self.X, self.Y = X, Y
    X = np.random.RandomState(13).rand(9, 2)
    Y1, Y2 = er.objectives(X)
    assert np.array_equal(observedFront([Stub(X, Y1), Stub(X.copy(), Y2)]), paretoFront(np.c_[Y1, Y2]))
    with pytest.raises(ValueError, match="front="):
        observedFront([Stub(X, Y1), Stub(X[::-1].copy(), Y2)])
    with pytest.raises(ValueError, match="front="):
        observedFront([Stub(X, Y1), Stub(X[:5], Y2[:5])])


# ------------------------------------------------------------------------------------------------ (g) the generator
@pytest.mark.parametrize("name", sorted(er.GEN))
def test_generator_is_worth_comparing_on(name):
    """for every front size at least 80 % of the case's 1000 candidates have a restated EHVI of at least 1e-8 of the objective
    box's area (else the GPU comparison would mostly compare zeros); the models are observed at different points; the raw fronts
    have the canonical sizes the GPU test names"""
    g = er.generator(name)
    area = float(np.prod(g["top"] - g["ref"]))
    assert area > .5 and g["X"][0].shape != g["X"][1].shape
    for n in er.FRONT_SIZES:
        F = er.gen_front(name, n)
        assert len(er.canonical(F, g["ref"])[0]) == n and len(F) > n
        for erf_mode in ERFS:
            v = er.gen_value(name, n, erf_mode)["val"]
            share = float(np.mean(v >= 1e-8 * area))
            print("generator %s n=%d erf=%d: share of EHVI >= 1e-8 area = %.3f, max %.3g" % (name, n, erf_mode, share, np.max(v)))
            assert share >= 0.8, (name, n, share)
            assert np.all(np.isfinite(v)) and np.all(v >= 0)


# ------------------------------------------------------------------------------------------------ the header's canonical form
FRONT_MAIN = r"""
#include "ehvi_front.h"
#include <cstdio>
int main(int argc, char **argv)
{
    int n, cap;
    double ref[2];
    if (scanf("%d %d %lf %lf", &n, &cap, &ref[0], &ref[1]) != 4) return 2;
    std::vector<double> f(2 * (size_t)n), out;
    for (int i = 0; i < 2 * n; i++) if (scanf("%lf", &f[i]) != 1) return 2;
    long long where = -1;
    const int rc = ehvi_canonical_front(n, f.data(), ref, cap, &out, &where);
    printf("%d %lld %zu\n", rc, where, out.size() / 2);
    for (size_t i = 0; i < out.size(); i++) printf("%.17g\n", out[i]);
    return 0;
}
"""


def test_the_headers_canonical_front_is_the_restatements(tmp_path):
    """ibo_amd/csrc/ehvi_front.h is host code with nothing behind it: a stand-alone program around it (the form in which it can
    be built with -fsanitize=address,undefined as well) agrees with er.canonical on random sets and reports each of its three
    errors"""
    import shutil
    import subprocess
    cxx = shutil.which("g++") or shutil.which("clang++") or shutil.which("c++") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    src = tmp_path / "front_main.cpp"
    src.write_text(FRONT_MAIN)
    exe = tmp_path / "front_main"
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-I", os.path.join(ROOT, "ibo_amd", "csrc"), str(src), "-o", str(exe)])

    def run(F, ref, cap=1024):
        F = np.asarray(F, dtype=float).reshape(-1, 2)
        text = "%d %d %r %r\n" % (len(F), cap, float(ref[0]), float(ref[1])) + "\n".join(repr(float(v)) for v in F.ravel()) + "\n"
        p = subprocess.run([str(exe)], input=text, capture_output=True, text=True, env={"PATH": os.environ.get("PATH", "")})
        assert p.returncode == 0, p.stderr
        lines = p.stdout.split()
        rc, where, n = int(lines[0]), int(lines[1]), int(lines[2])
        return rc, where, np.array([float(v) for v in lines[3:]]).reshape(n, 2)

    rs = np.random.RandomState(14)
    for trial in range(12):
        n = [0, 1, 5, 40][trial % 4]
        F = np.round(rs.rand(n, 2) * 5) / 5 if trial % 2 else rs.rand(n, 2)
        ref = rs.rand(2) * .4
        rc, _, got = run(F, ref)
        a, b = er.canonical(F, ref)
        assert rc == 0 and np.array_equal(got, np.c_[a, b].reshape(-1, 2))
    F = er.curve_front(65, REF, np.array([1., 1.]))
    rc, _, got = run(F, REF)
    assert rc == 0 and len(got) == 65
    assert run(F, REF, cap=64)[:2] == (3, 65)                      # too many left
    assert run(F, [np.nan, 0.])[0] == 1 and run(F, [0., np.inf])[0] == 1
    bad = F.copy(); bad[7, 1] = np.nan
    assert run(bad, REF)[:2] == (2, 7)
    bad[7, 1] = -np.inf
    assert run(bad, REF)[:2] == (2, 7)


# ------------------------------------------------------------------------------------------------ (f) the symbols
def test_symbols_are_declared_exported_and_bound():
    from ibo_amd import _lib
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ibo_abi.h")).read(), flags=re.S)
    for s in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % s, txt), "%s is not declared in ibo_abi.h" % s
        assert hasattr(_lib.lib, s), "libibo_hip.so does not export %s" % s
        assert s in _lib.EXPORTED
    assert re.search(r"#define\s+IBO_EHVI_MAX_FRONT\s+1024\b", txt)
    assert _lib.lib.ibo_abi_version() == 8
    if _lib.device_count() > 0:
        return                                       # (tests/test_gpu_ehvi.py takes over where a GPU is visible)
    Q = _lib.f64(np.zeros((2, 3))); out = np.empty(6); lb = _lib.f64(np.zeros(3)); ub = _lib.f64(np.ones(3))
    ref = _lib.f64([0., 0.])
    bv = ctypes.c_double(); bi = ctypes.c_int64()
    L = _lib.lib
    assert L.ibo_ehvi_sweep(None, 0, None, _lib.dp(ref), 2, None, 0, 1e-8, 0, None, .5, 0, None, ctypes.byref(bv), ctypes.byref(bi)) == _lib.ERR_NO_DEVICE
    assert L.ibo_ehvi_batch(None, 0, None, _lib.dp(ref), 2, _lib.dp(Q), 0, 1e-8, _lib.dp(out)) == _lib.ERR_NO_DEVICE
    assert L.ibo_ehvi_grad_batch(None, 0, None, _lib.dp(ref), 2, _lib.dp(Q), 0, 1e-8, _lib.dp(out), None) == _lib.ERR_NO_DEVICE
    assert L.ibo_ehvi_direct_max(None, 0, None, _lib.dp(ref), 3, _lib.dp(lb), _lib.dp(ub), 0, 1e-8, 5, 5, 100, 1,
                                 ctypes.byref(bv), _lib.dp(out), None) == _lib.ERR_NO_DEVICE

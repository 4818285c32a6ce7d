"""
tests/gradobs_reference.py -- the NumPy restatement tests/test_gpu_gradobs.py holds the device to -- pinned without a GPU:
the block formulas to mpmath differentiation of the kernels' defining formulas, the model to what it claims (it reproduces the values AND
the slopes it was given), the value-only limit to the oracle, float64 to long double on every listed case; and the new symbols are
declared, exported and bound.
"""
import ctypes
import os
import re

import numpy as np
import pytest

import gradobs_reference as gr
from conftest import ROOT
from oracle import oracle as orc

import mpmath


# ---------------------------------------------------------------------------- block formulas against mpmath
def mp_cov(kind, hyper, D):
    """the kernel's defining formula (ibo_amd/gaussianprocess/kernel.py: cov) on mpmath numbers, as a function of (x_1..x_D, x'_1..x'_D)"""
    mp = mpmath.mp
    th = [mp.mpf(repr(float(h))) for h in hyper]

    def f(*a):
        d = [a[i] - a[D + i] for i in range(D)]
        if kind == "ard":
            return mp.exp(-sum(di * di / (th[i] * th[i]) for i, di in enumerate(d)) / 2)
        if kind == "iso":
            return mp.exp(-sum(di * di for di in d) / (th[0] * th[0]) / 2)
        if kind == "m3":
            z = mp.sqrt(3) * mp.sqrt(sum(di * di for di in d)) / th[0]
            return th[1] ** 2 * (1 + z) * mp.exp(-z)
        z = sum((mp.sqrt(5) * di / th[0]) ** 2 for di in d)
        return th[1] ** 2 * mp.exp(-mp.sqrt(z)) * (1 + mp.sqrt(z) + z / 3)
    return f


FAMILY_HYPER = {"ard": [0.5, 0.8, 0.65, 1.1], "iso": [0.6], "m3": [0.7, 0.9], "m5": [0.55, 0.8]}


@pytest.mark.parametrize("D", [1, 2, 3, 4])
@pytest.mark.parametrize("kind", ["ard", "iso", "m3", "m5"])
def test_every_block_entry_is_the_mpmath_derivative_of_the_kernel_formula(kind, D):
    hyper = FAMILY_HYPER[kind][:D] if kind == "ard" else FAMILY_HYPER[kind]
    kern = orc.Kern(kind, hyper)
    rs = np.random.RandomState(10 * D + len(kind))
    x, xp = rs.rand(D), rs.rand(D)
    scale = kern.sf2_py * max(1.0, float(np.max(gr.weights(kern, D))))
    old = mpmath.mp.dps
    mpmath.mp.dps = 30
    try:
        f = mp_cov(kind, hyper, D)
        for a, b in ((x, xp), (x, x.copy())):                       # a generic pair, and coincident points (r = 0)
            B = gr.blocks(kern, a[None, :], b[None, :])[0, 0]
            at = [mpmath.mpf(repr(float(v))) for v in np.r_[a, b]]
            for i in range(D + 1):
                for j in range(D + 1):
                    order = [0] * (2 * D)
                    if i:
                        order[i - 1] += 1                           # d / dx_i
                    if j:
                        order[D + j - 1] += 1                       # d / dx'_j
                    want = f(*at) if not (i or j) else mpmath.diff(f, tuple(at), tuple(order))
                    err = abs(mpmath.mpf(float(B[i, j])) - want)
                    assert err <= 1e-13 * scale, (kind, D, i, j, float(err), float(want))
    finally:
        mpmath.mp.dps = old


def test_blocks_mirror_exactly_and_the_matrix_is_symmetric():
    for name in ("m3_10x2_twin", "ard_13x4", "m5_43x2"):
        c = gr.case(name)
        A = gr.matrix(c["kern"], c["X"], c["noise"], c["gnoise"])
        assert np.array_equal(A, A.T)
        N, D = c["X"].shape
        assert A.shape == (N * (D + 1), N * (D + 1))
        assert np.all(np.diag(A)[::D + 1] == 1.0 + c["noise"])


# ---------------------------------------------------------------------------- the model means what it says
def test_the_mean_reproduces_the_values_and_its_central_differences_the_slopes():
    """noise = gnoise = 1e-8 on a smooth function, SE-iso, long double.  In exact arithmetic K alpha = [Y; G] - Sigma alpha with
    Sigma = diag(noise, gnoise..): the mean at a training point misses Y_i by exactly noise |alpha_i|, its gradient misses G_id by
    gnoise |alpha_id|.  The central difference with step h adds h^2 / 6 times the mean's third derivative along the axis,
    |m'''| <= sum_j |alpha_j| B_j: an entry of k* is sf2 times a product of Hermite functions He_n(s) exp(-s^2 / 2) / theta^n in the scaled
    distance, n = 3 for a value entry and 4 for a derivative entry, and max |He_3 e^{-s^2/2}| < 1.4, max |He_4 e^{-s^2/2}| = 3: B_j <= 3
    max(theta^-3, theta^-4).  Rounding: the long-double solve carries 2^-63 cond_2 relative to sum_j |k*_j alpha_j|, and the difference
    quotient divides two such errors by 2 h; h balances the two terms, h = (3 rounding / third derivative)^(1/3)."""
    theta, noise = 0.5, 1e-8
    kern = orc.Kern("iso", [theta])
    X = gr.points(12, 2, 5)
    Y, G = gr.objective(X)
    m = gr.fit(kern, X, Y, G, noise, noise, longdouble=True)
    al = np.abs(np.asarray(m["alpha"], dtype=np.float64))
    p = gr.posterior(m, X)
    rnd = 2.0 ** -63 * m["cond"] * float(np.max(p["mu_scale"]))
    bar_y = noise * al[::3] + rnd
    miss_y = np.abs(np.asarray(p["mu"], dtype=np.float64) - Y)
    print("values: worst miss %.3g, bar %.3g (cond %.3g)" % (miss_y.max(), bar_y.max(), m["cond"]))
    assert np.all(miss_y <= bar_y)
    third = 3.0 * max(theta ** -3, theta ** -4) * float(np.sum(al))
    h = (3.0 * rnd / third) ** (1.0 / 3.0)
    for d in range(2):
        e = np.zeros(2); e[d] = h
        up, dn = gr.posterior(m, X + e), gr.posterior(m, X - e)
        cd = np.asarray((up["mu"] - dn["mu"]) / (2 * np.longdouble(h)), dtype=np.float64)
        bar_g = noise * al[1 + d::3] + h * h / 6.0 * third + 2.0 * rnd / (2 * h)
        miss_g = np.abs(cd - G[:, d])
        print("slopes d=%d: worst miss %.3g, bar %.3g" % (d, miss_g.max(), bar_g.max()))
        assert np.all(miss_g <= bar_g)
        assert bar_g.max() < 2e-2 * np.max(np.abs(G[:, d]))         # the bar itself is far below the slopes it certifies


# ---------------------------------------------------------------------------- the value-only limit against the oracle
def value_only_bound(kern, X, Y, G, Q, noise, gnoise):
    """(bound_mu, bound_s2) on the distance between the gradient model with derivative noise `gnoise` and the value-only model.
    Ordering A = [[Kvv, Kvd], [Kdv, Kdd + gnoise I]], S = its Schur complement on the derivative rows: S >= gnoise I because
    [[Kvv, Kvd], [Kdv, Kdd]] is a covariance plus a non-negative diagonal (sf2 <= 1 + noise), so |S^-1| <= 1 / gnoise, and
    Kvv >= (1 + noise - sf2) I.  With c = |k_v*| |Kvv^-1| |Kvd| + |k_d*|:
        a_d = S^-1 (G - Kdv Kvv^-1 Y),   mu - mu_0 = (k_d* - Kdv Kvv^-1 k_v*)^T a_d,   s2_0 - s2 = |S^-1/2 (k_d* - Kdv Kvv^-1 k_v*)|^2
        |mu - mu_0| <= c |a_d| <= c (|G| + |Kvd| |Kvv^-1| |Y|) / gnoise,      |s2 - s2_0| <= c^2 / gnoise
    with the norms bounded by entries: |Kvd| <= N sqrt(D) gmax, |k_d*| <= sqrt(N D) gmax (gmax = max |dk|, taken from the restated
    matrices), |k_v*| <= sqrt(N) sf2, |G| <= sqrt(N D) max |G|, |Y| <= sqrt(N) max |Y|, |Kvv^-1| <= 1 / (1 + noise - sf2)."""
    N, D = X.shape
    sf2 = kern.sf2_py
    assert sf2 <= 1.0 + noise
    Bxx, Bqx = gr.blocks(kern, X, X), gr.blocks(kern, Q, X)
    gmax = max(float(np.max(np.abs(Bxx[:, :, 0, 1:]))), float(np.max(np.abs(Bqx[:, :, 0, 1:]))))
    inv_vv = 1.0 / (1.0 + noise - sf2)
    kvd = N * np.sqrt(D) * gmax
    c = np.sqrt(N) * sf2 * inv_vv * kvd + np.sqrt(N * D) * gmax
    a_d = (np.sqrt(N * D) * float(np.max(np.abs(G))) + kvd * inv_vv * np.sqrt(N) * float(np.max(np.abs(Y)))) / gnoise
    return c * a_d, c * c / gnoise


@pytest.mark.parametrize("kind,hyper", [("ard", [0.5, 0.8]), ("iso", [0.6]), ("m3", [0.7, 0.9]), ("m5", [0.55, 0.8])])
def test_with_huge_gradient_noise_the_posterior_is_the_oracles_value_only_posterior(kind, hyper):
    kern = orc.Kern(kind, hyper)
    X = gr.points(8, 2, 11)
    Y, G = gr.objective(X)
    Q = gr.queries(X, 40)
    noise, gnoise = 0.1, 1e12
    m = gr.fit(kern, X, Y, G, noise, gnoise)
    p = gr.posterior(m, Q)
    mu0, s20 = orc.GP(kern, X, Y, noise=noise).posteriors(Q)
    bmu, bs2 = value_only_bound(kern, X, Y, G, Q, noise, gnoise)
    slack = 1e-12                                                   # the two float64 evaluations' own rounding (cond_2 of Kvv < 1e3)
    print("%s: mu %.3g (bound %.3g), s2 %.3g (bound %.3g)" % (kind, np.max(np.abs(p["mu"] - mu0)), bmu, np.max(np.abs(p["s2"] - s20)), bs2))
    assert bmu < 1e-3 and bs2 < 1e-3
    assert np.max(np.abs(p["mu"] - mu0)) <= bmu + slack
    assert np.max(np.abs(p["s2"] - s20)) <= bs2 + slack


# ---------------------------------------------------------------------------- float64 against long double
@pytest.mark.parametrize("name", gr.CASE_NAMES)
def test_the_float64_restatement_stays_within_half_the_bars_of_long_double(name):
    c = gr.case(name)
    m, ml = gr.case_model(name, False), gr.case_model(name, True)
    assert m["P"] == CASE_P[name]
    Q = gr.queries(c["X"], 130)
    p, pl = gr.posterior(m, Q), gr.posterior(ml, Q)
    bmu, bs2 = gr.bars(m, p)
    rmu = float(np.max(np.abs(p["mu"] - np.asarray(pl["mu"], dtype=np.float64)) / bmu))
    rs2 = float(np.max(np.abs(p["s2"] - np.asarray(pl["s2"], dtype=np.float64)) / bs2))
    print("%s: P %d cond %.3g, mu at %.3g of the bar, s2 at %.3g" % (name, m["P"], m["cond"], rmu, rs2))
    assert rmu <= 0.5 and rs2 <= 0.5
    assert np.max(np.abs(c["X"])) <= 1.0 and np.max(np.abs(c["Y"])) <= 1.0 and np.max(np.abs(c["G"])) <= 1.0


CASE_P = {"se_1x1": 2, "m3_21x2": 63, "ard_16x3": 64, "ard_13x4": 65, "iso_32x3": 128, "m5_43x2": 129, "m5_9x16": 153, "ard_60x4": 300,
          "ard_205x4": 1025, "m3_10x2_twin": 30}


def test_the_case_list_holds_what_was_asked_for():
    assert sorted(CASE_P) == sorted(gr.CASE_NAMES)
    c = gr.case("m3_10x2_twin")
    assert np.array_equal(c["X"][2], c["X"][5])
    assert gr.case("ard_60x4")["noise"] == 0.01
    assert gr.QUERY_COUNTS == (1, 63, 64, 65, 130)


# ---------------------------------------------------------------------------- the second case list: a gnoise per dimension, big cases
EDGE_P = {"ard_257x1": 514, "m5_300x2": 900, "m3_513x1": 1026, "ard_60x3_gn": 240, "sviso_20x2": 60, "se_3x64": 195, "ard_525x3": 2100,
          "ard_1008x3": 4032, "ard_1009x3": 4036, "m5_1648x3": 6592, "m3_1649x3": 6596, "iso_2048x3": 8192}


def test_the_edge_case_list_holds_what_was_asked_for():
    assert sorted(EDGE_P) == sorted(gr.EDGE_NAMES) and not set(gr.EDGE_NAMES) & set(gr.CASE_NAMES)
    assert sorted(gr.SMALL_EDGE_NAMES + gr.BIG_NAMES) == sorted(gr.EDGE_NAMES)
    assert gr.BIG_NAMES == [n for n in gr.EDGE_NAMES if EDGE_P[n] > 2000]
    for name in gr.SMALL_EDGE_NAMES:
        c = gr.case(name)
        N, D = c["X"].shape
        assert N * (D + 1) == EDGE_P[name] and c["gnoise"].shape == (D,)
        assert np.max(np.abs(c["X"])) <= 1.0 and np.max(np.abs(c["Y"])) <= 1.0 and np.max(np.abs(c["G"])) <= 1.0
        assert gr.case(name) is c                                   # small: made once
    assert np.array_equal(gr.case("ard_60x3_gn")["gnoise"], [1e-4, 3e-3, 0.05])
    assert np.all(gr.case("m3_513x1")["gnoise"] == 0.02)
    c = gr.case("m3_513x1")
    assert np.array_equal(c["X"][2], c["X"][400])
    assert abs(gr.case("sviso_20x2")["kern"].sf2_py - 0.81) < 1e-15 and gr.case("sviso_20x2")["kern"].ktype == orc.K_SE_ISO
    assert gr.case("se_3x64")["X"].shape == (3, 64)
    big = gr.case("ard_525x3")
    assert gr.is_big("ard_525x3") and gr.case("ard_525x3") is not big and np.array_equal(gr.case("ard_525x3")["X"], big["X"])
    assert all(np.all(gr.case(n)["gnoise"] == 0.05) for n in ("ard_525x3", "ard_1009x3"))
    # the listed cases are what they were: the same seeds, the default gnoise
    assert np.array_equal(gr.case("ard_13x4")["X"], gr.points(13, 4, 103)) and np.all(gr.case("ard_13x4")["gnoise"] == 1e-4)


def test_a_vector_gnoise_lands_on_its_own_derivative_rows_and_nowhere_else():
    """matrix() with three distinct gnoise entries, every entry against mpmath differentiation of the kernel's defining formula plus the
    diagonal rule: 1 + noise on a value row, the second derivative at u = 0 plus gnoise[d - 1] on derivative row d, nothing else anywhere"""
    kind, hyper, N, D, noise = "ard", FAMILY_HYPER["ard"][:3], 3, 3, 0.1
    gnoise = np.array([1e-4, 3e-3, 0.05])
    kern = orc.Kern(kind, hyper)
    X = gr.points(N, D, 31)
    A = gr.matrix(kern, X, noise, gnoise)
    scale = kern.sf2_py * max(1.0, float(np.max(gr.weights(kern, D))))
    B = D + 1
    old = mpmath.mp.dps
    mpmath.mp.dps = 30
    try:
        f = mp_cov(kind, hyper, D)
        for i in range(N):
            for j in range(N):
                at = [mpmath.mpf(repr(float(v))) for v in np.r_[X[i], X[j]]]
                for a in range(B):
                    for b in range(B):
                        order = [0] * (2 * D)
                        if a:
                            order[a - 1] += 1
                        if b:
                            order[D + b - 1] += 1
                        want = f(*at) if not (a or b) else mpmath.diff(f, tuple(at), tuple(order))
                        if i == j and a == b:
                            want = mpmath.mpf(1) + mpmath.mpf(noise) if a == 0 else want + mpmath.mpf(float(gnoise[a - 1]))
                        err = abs(mpmath.mpf(float(A[i * B + a, j * B + b])) - want)
                        assert err <= 1e-13 * scale, (i, j, a, b, float(err), float(want))
    finally:
        mpmath.mp.dps = old
    diff = A - gr.matrix(kern, X, noise, 0.0)
    assert np.array_equal(diff - np.diag(np.diag(diff)), np.zeros_like(A))
    assert np.max(np.abs(np.diag(diff) - np.tile(np.r_[0.0, gnoise], N))) <= 1e-13 * scale < 0.1 * np.min(np.diff(gnoise))
    assert np.array_equal(gr.matrix(kern, X, noise, 3e-3), gr.matrix(kern, X, noise, [3e-3] * 3))      # a number is tiled


@pytest.mark.parametrize("name", gr.CASE_NAMES + gr.SMALL_EDGE_NAMES)
def test_cond_upper_bounds_cond_2_on_the_small_cases(name):
    c = gr.case(name)
    up, cond = gr.cond_upper(c["kern"], c["X"], c["noise"], c["gnoise"]), gr.case_model(name)["cond"]
    print("%s: cond_2 %.4g, cond_upper %.4g" % (name, cond, up))
    assert up >= cond >= 1.0
    A = gr.matrix(c["kern"], c["X"], c["noise"], c["gnoise"])
    lo = min(1.0 + c["noise"] - c["kern"].sf2_py, float(np.min(c["gnoise"])))
    assert abs(up * lo / float(np.max(np.sum(np.abs(A), axis=1))) - 1.0) < 1e-12      # the slabs' row sums are |A|_inf (summed in another order)


def test_cond_upper_refuses_a_signal_variance_above_the_value_diagonal():
    X = gr.points(4, 2, 1)
    with pytest.raises(AssertionError):
        gr.cond_upper(orc.Kern("m5", [0.5, 1.2]), X, 0.1, 1e-4)     # sf2 = 1.44 > 1.1


@pytest.mark.parametrize("name", gr.BIG_NAMES)
def test_every_big_case_is_admissible_in_float64(name):
    """cond_upper <= 1e6: the bars' factor 1e-15 max(cond, 1e6) is then its floor 1e-9 and float64 the reference the rule selects"""
    c = gr.case(name)
    N, D = c["X"].shape
    up = gr.cond_upper(c["kern"], c["X"], c["noise"], c["gnoise"])
    print("%s: P %d, cond_upper %.4g" % (name, N * (D + 1), up))
    assert N * (D + 1) == EDGE_P[name] > gr.BIG_ROWS and up <= 1e6
    assert 1e-15 * max(up, 1e6) == 1e-9


def test_the_acquisition_restatement_is_the_oracles():
    rs = np.random.RandomState(3)
    mu, s2 = rs.randn(50) * 0.5, rs.rand(50) + 1e-3
    for acq in (gr.ACQ_EI, gr.ACQ_PI, gr.ACQ_UCB):
        for erf_mode in (gr.ERF_LIBM, gr.ERF_NR):
            parm = 1.3 if acq == gr.ACQ_UCB else 0.01
            got = gr.acquisition(acq, erf_mode, mu, s2, 0.4, parm)
            want = orc.acq_value(acq, erf_mode, mu, np.sqrt(s2), 0.4, parm)
            assert np.max(np.abs(got - want)) <= 1e-14 * max(1.0, np.max(np.abs(want)))


# ---------------------------------------------------------------------------- symbols
GGP_SYMBOLS = ["ibo_ggp_create", "ibo_ggp_destroy", "ibo_ggp_info", "ibo_ggp_fit", "ibo_ggp_get_R", "ibo_ggp_get_L", "ibo_ggp_acq_batch",
               "ibo_ggp_acq_sweep", "ibo_ggp_direct_max", "ibo_ggp_stage_ms"]


def test_the_symbols_are_declared_exported_and_bound_and_the_abi_version_stays():
    from ibo_amd import _lib
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ibo_abi.h")).read(), flags=re.S)
    for s in GGP_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % s, txt), "%s is not declared in ibo_abi.h" % s
        assert getattr(_lib.lib, s).argtypes is not None, "%s is not bound" % s
        assert s in _lib.EXPORTED
    assert "typedef struct ibo_ggp ibo_ggp_t;" in txt and re.search(r"#define\s+IBO_GGP_MAX_ROWS\s+\d+", txt)
    assert re.search(r"#define\s+IBO_ABI_VERSION\s+8\b", txt) and _lib.lib.ibo_abi_version() == 8


def test_the_options_exist_and_no_entry_computes_without_a_device():
    from ibo_amd import _lib
    assert _lib.lib.ibo_set_option(b"ggp_chunk", 512) == _lib.OK and _lib.lib.ibo_set_option(b"ggp_chunk", 0) == _lib.OK
    assert _lib.lib.ibo_set_option(b"ggp_chunk", -1) == _lib.ERR_ARG
    assert _lib.lib.ibo_set_option(b"ggp_timing", 0) == _lib.OK
    ms = np.zeros(8)
    assert _lib.lib.ibo_ggp_stage_ms(_lib.dp(ms), 1) == _lib.OK and np.all(ms == 0.0)
    if _lib.device_count() > 0:
        return                                                      # (a GPU is visible: the refusal without one cannot be observed here)
    h = ctypes.c_void_p()
    assert _lib.lib.ibo_ggp_create(0, ctypes.byref(h)) == _lib.ERR_NO_DEVICE
    q = np.zeros((1, 2)); out = np.zeros(1)
    assert _lib.lib.ibo_ggp_acq_batch(None, 1, _lib.dp(q), 0, 0.0, 0, 1e-8, float("nan"), _lib.dp(out), None, None) == _lib.ERR_NO_DEVICE


def test_the_constructor_refuses_what_needs_no_device():
    from ibo_amd.gaussianprocess import GaussianProcess, PrefGaussianProcess, GaussianKernel_iso
    from ibo_amd.gaussianprocess import trainhyper
    X = gr.points(4, 2, 1)
    Y, G = gr.objective(X)
    k = GaussianKernel_iso([0.5])
    with pytest.raises(ValueError):
        GaussianProcess(k, X, Y, G=G[:, :1])
    with pytest.raises(ValueError):
        GaussianProcess(k, G=G)
    with pytest.raises(NotImplementedError, match="PrefGaussianProcess"):
        PrefGaussianProcess(k, X=X, Y=Y, G=G)
    for fn, args in ((trainhyper.marginalLikelihood, (k, X, Y, 1)), (trainhyper.looLikelihood, (k, X, Y, 1)),
                     (trainhyper.nlml_values, ([k], X, Y))):
        with pytest.raises(NotImplementedError, match=fn.__name__):
            fn(*args, G=G)
    with pytest.raises(NotImplementedError, match="nlml_grid"):
        trainhyper.nlml_grid(GaussianKernel_iso, [[0.5]], X, Y, G=G)

"""
Max-value entropy search on the device: ibo_mes_sweep / ibo_mes_batch / ibo_mes_grad_batch / ibo_mes_direct_max / ibo_mes_maxcdf and
ibo_amd.acquisition.entropy on top of them.

Tolerances (T: the mean magnitude of a candidate's K terms, |gamma lambda / 2| + |log Phi|, tests/mes_reference.py)
  * the walk on the library's OWN (mu, s2) (ibo_acq_batch, IBO_ACQ_NONE, the same clamp, the same number of points -- the same
    launch of the same kernels): |dev - truth| <= 1e-12 T + 1e-300 against mpmath on a few candidates per case, and against the
    restatement on all of them at 1.25e-12 T (the restatement itself is pinned at 2.5e-13 T, tests/test_mes_reference.py);
    measured on the MI355X: see DESIGN 4.28;
  * end to end, against the restatement on the NumPy posterior (pinned to the oracle by tests/test_cacq_reference.py):
    1e-6 T + |G_mu| dmu + |G_sigma| dsigma with dmu = 1e-6 |mu| + 1e-9 and ds2 = 1e-6 s2, the posterior's parity bars
    (dsigma = ds2 / (2 sigma));
  * bit equality between the entries and across chunk sizes: np.array_equal; the two size classes of the plain sweep: 1e-12 of
    T + sigma (A_mu + A_sigma), the magnitudes of the value's terms and of its posterior derivatives' (see the test);
  * gradients: 1e-9 of the scale + 1e-13 (tests/grad_reference.py), and central differences of ibo_mes_batch with step 1e-5 at
    1e-6 (scale + T) (the reasoning of tests/test_mes_reference.py; the device's values are smooth in x to far below that);
  * ibo_mes_maxcdf: 1e-12 sum |log Phi| against the ordered sum on the library's own posterior; the bracket exactly.
Models of 25 to 200 rows, D in {1, 3}: SE-iso, SE-ARD with a mean prior, Matern-3/2, Matern-5/2, one PrefGaussianProcess.
"""
import ctypes

import mpmath
import numpy as np
import pytest

import grad_reference as gr
import cacq_reference as cr
import mes_reference as mr

pytestmark = pytest.mark.gpu

NAN = float("nan")
#        name     D  kind   hyper            N    seed prior  noise
SPECS = {"iso1": (1, "iso", [.3], 25, 201, False, .01),
         "ard3": (3, "ard", [.5, .6, .45], 200, 203, True, .05),
         "m3": (3, "m3", [.7, .95], 120, 204, False, .02),
         "m5": (1, "m5", [.45, .9], 40, 202, False, .01),
         "sharp": (3, "iso", [.35], 60, 205, False, 1e-3)}
FAMILIES = ["iso1", "ard3", "m3", "m5"]
GEN_M = 1000


@pytest.fixture(scope="module")
def lib():
    from ibo_amd import _lib
    if _lib.device_count() < 1:
        pytest.fail("no GPU visible: the product has no CPU fallback")
    return _lib


def make_kernel(kind, hyper):
    from ibo_amd.gaussianprocess import kernel as K
    return {"ard": K.GaussianKernel_ard, "iso": K.GaussianKernel_iso, "m3": K.MaternKernel3, "m5": K.MaternKernel5}[kind](np.array(hyper, dtype=float))


@pytest.fixture(scope="module")
def cases(lib):
    """per model: the data, the GaussianProcess, the restated model, 1000 candidates on the host and on the device, the offset of the
    latent variance and the restated posterior over the candidates (clamp 1e-8) -- computed once, shared, to be left unchanged"""
    from ibo_amd import DeviceArray
    from ibo_amd.gaussianprocess import GaussianProcess
    from ibo_amd.gaussianprocess.prior import RBFNMeanPrior
    out = {}
    for name, (D, kind, hyper, N, seed, with_prior, noise) in SPECS.items():
        rs = np.random.RandomState(seed)
        X = rs.rand(N, D)
        Y = np.sin(3 * X.sum(1)) + .01 * rs.randn(N)
        pr = prior = None
        if with_prior:
            pr = (rs.rand(5, D), .3 * rs.randn(5), 1.5, np.zeros(D) - .1, np.full(D, 1.2))
            prior = RBFNMeanPrior()
            prior.means, prior.beta, prior.theta, prior.lowerb, prior.width = pr
        m = cr.make(X, Y, noise, kind, hyper, prior=pr)
        GP = GaussianProcess(make_kernel(kind, hyper), X, Y, prior=prior, noise=noise)
        GP._push_prior()
        assert abs(GP.kernel._ibo_spec()[2] - m.sf2k) < 1e-15
        Q = rs.rand(GEN_M, D) * 1.1 - .05
        off = max(1.0 + noise - m.ref.sf2, 0.0)
        post = cr.posterior(m, Q, 1e-8)
        for v in post:
            v.setflags(write=False)
        out[name] = dict(D=D, X=X, Y=Y, noise=noise, m=m, GP=GP, Q=Q, dc=DeviceArray.from_host(Q), off=off, post=post)
    return out


def samples(c, K, seed=0):
    """K samples of a maximum: above the best observation by 0.02 to 0.42 (a few latent deviations of the sharper models)"""
    return float(np.max(c["Y"])) + .02 + .4 * np.random.RandomState(900 + K + seed).rand(K)


def raw_sweep(lib, GP, ys, off, dc, clamp=1e-8, exclude=None, radius=.5, base=0, want_val=True):
    """(rc, val or None, best_val, best_idx) of ibo_mes_sweep"""
    from ibo_amd import DeviceArray
    M = dc.shape[0]
    ys = lib.f64(ys)
    val = DeviceArray((M,)) if want_val else None
    if val is not None:
        val.upload(np.full(M, 7.25))
    ex = None if exclude is None else lib.f64(np.atleast_2d(exclude))
    bv = ctypes.c_double(-5.0); bi = ctypes.c_int64(-5)
    rc = lib.lib.ibo_mes_sweep(GP._handle(), len(ys), lib.dp(ys), off, M, dc.ptr, clamp, 0 if ex is None else len(ex),
                               None if ex is None else lib.dp(ex), radius, base, None if val is None else val.ptr, ctypes.byref(bv), ctypes.byref(bi))
    return rc, (val.to_host() if val is not None and rc == 0 else None), bv.value, bi.value


def raw_batch(lib, GP, ys, off, Q, clamp=1e-8, grad=False):
    """(rc, val) of ibo_mes_batch, or (rc, val, grad) of ibo_mes_grad_batch"""
    Q = lib.f64(np.atleast_2d(Q))
    M, D = Q.shape
    ys = lib.f64(ys)
    val = np.full(M, 7.25)
    if not grad:
        return lib.lib.ibo_mes_batch(GP._handle(), len(ys), lib.dp(ys), off, M, lib.dp(Q), clamp, lib.dp(val)), val
    g = np.full((M, D), 7.25)
    return lib.lib.ibo_mes_grad_batch(GP._handle(), len(ys), lib.dp(ys), off, M, lib.dp(Q), clamp, lib.dp(val), lib.dp(g)), val, g


def raw_direct(lib, GP, ys, off, D, clamp=1e-8, maxiter=8):
    ys = lib.f64(ys)
    lb, ub = lib.f64(np.zeros(D)), lib.f64(np.ones(D))
    opt = ctypes.c_double(); optx = np.empty(D); ns = ctypes.c_int64()
    rc = lib.lib.ibo_mes_direct_max(GP._handle(), len(ys), lib.dp(ys), off, D, lib.dp(lb), lib.dp(ub), clamp, maxiter, 30, 10000, 1,
                                    ctypes.byref(opt), lib.dp(optx), ctypes.byref(ns))
    return rc, opt.value, optx, ns.value


def raw_maxcdf(lib, GP, dc, levels, off, clamp=1e-8):
    lev = lib.f64(np.asarray(levels, dtype=float).reshape(-1))
    out, stats = np.full(len(lev), 7.25), np.full(2, 7.25)
    rc = lib.lib.ibo_mes_maxcdf(GP._handle(), dc.shape[0], dc.ptr, len(lev), lib.dp(lev) if len(lev) else None, off, clamp,
                                lib.dp(out) if len(lev) else None, lib.dp(stats))
    return rc, out, stats


def own_posterior(lib, GP, Q, clamp):
    """(mu, s2) of ibo_acq_batch with IBO_ACQ_NONE"""
    Q = lib.f64(np.atleast_2d(Q))
    mu, s2 = np.empty(len(Q)), np.empty(len(Q))
    lib.check(lib.lib.ibo_acq_batch(GP._handle(), len(Q), lib.dp(Q), lib.ACQ_NONE, 0.0, lib.ERF_LIBM, clamp, NAN, lib.dp(mu), lib.dp(s2), None))
    return mu, s2


def set_chunk(lib, m):
    lib.check(lib.lib.ibo_set_option(b"mes_chunk", int(m)))


def last_kernel(lib, GP):
    ms = ctypes.c_float(); name = ctypes.c_char_p()
    lib.check(lib.lib.ibo_last_sweep_kernel_ms(GP._handle(), ctypes.byref(ms), ctypes.byref(name)))
    return name.value.decode()


def pref_model(D):
    from ibo_amd.gaussianprocess import PrefGaussianProcess
    rs = np.random.RandomState(61)
    pts = rs.rand(20, D)
    f = lambda x: -np.sum((x - .4) ** 2)
    prefs = []
    for i in range(10):
        a, b = pts[2 * i], pts[2 * i + 1]
        prefs.append((a, b, 0) if f(a) > f(b) else (b, a, 0))
    GP = PrefGaussianProcess(make_kernel("ard", [.4] * D))
    GP.addPreferences(prefs)
    return GP


# ------------------------------------------------------------------------------------------------ the walk, both tails
@pytest.mark.parametrize("K", [1, 2, 63, 64, 65, 1023, 1024])
def test_walk_on_the_librarys_own_posterior(lib, cases, K):
    """200 points of the noise-1e-3 model, 50 of them next to observations (sigma down to 0.03); y* spread over mu_c +- 45 sigma_c of
    the sharpest candidate c, so that gamma covers both tails: asserted below on the library's own (mu, s2)"""
    c = cases["sharp"]
    GP, clamp = c["GP"], 1e-8
    Q = np.r_[c["Q"][:150], c["X"][:50] + 1e-3]
    mu, s2 = own_posterior(lib, GP, Q, clamp)
    sig = np.sqrt(np.maximum(s2, clamp))
    c0 = int(np.argmin(sig))
    lo, hi = mu[c0] - 45.0 * sig[c0], mu[c0] + 45.0 * sig[c0]
    runs = [np.array([lo]), np.array([hi])] if K == 1 else [np.linspace(lo, hi, K)[np.random.RandomState(K).permutation(K)]]
    gmin, gmax, worst_mp, worst_re = np.inf, -np.inf, 0.0, 0.0
    n_mp = max(2, min(12, 2400 // K))                                   # (a term costs about 0.4 ms in mpmath)
    picks = sorted(set([c0, int(np.argmax(sig))] + [int(i) for i in np.linspace(0, 199, n_mp)][:n_mp - 2]))
    for ys in runs:
        rc, val = raw_batch(lib, GP, ys, 0.0, Q, clamp)
        assert rc == 0
        r = mr.from_posterior(mu, s2, ys, 0.0, clamp)
        gmin, gmax = min(gmin, float(np.min(r["gmin"]))), max(gmax, float(np.max(r["gmax"])))
        err = np.abs(val - r["val"])
        assert np.all(err <= 1.25e-12 * r["T"] + 1e-300), ("restatement", int(np.argmax(err / (r["T"] + 1e-300))))
        worst_re = max(worst_re, float(np.max(err / (1e-12 * r["T"] + 1e-300))))
        with mpmath.workdps(40):
            for i in picks:
                t, T = mr.walk_mp(mu[i], s2[i], np.sort(ys), 0.0, clamp, dps=40)
                e = abs(mpmath.mpf(float(val[i])) - t)
                bar = 1e-12 * T + mpmath.mpf("1e-300")
                worst_mp = max(worst_mp, float(e / bar))
                assert e <= bar, ("mpmath", i, float(e / bar))
    print("K=%d: gamma in [%.1f, %.1f]; worst |dev - truth| / bar = %.3g (mpmath, %d candidates), %.3g (restatement, all)"
          % (K, gmin, gmax, worst_mp, len(picks), worst_re))
    assert gmin <= -40.0 and gmax >= 40.0


@pytest.mark.parametrize("name", FAMILIES + ["pref"])
def test_composition_of_the_librarys_own_posterior(lib, cases, name):
    """every family and the preference GP: the restatement's walk on (mu, s2) of ibo_acq_batch, the latent offset included"""
    if name == "pref":
        GP, Q, off = pref_model(3), cases["ard3"]["Q"][:300], 0.0
        mu0 = own_posterior(lib, GP, Q, 1e-7)[0]
        ys = float(np.max(mu0)) + .02 + .5 * np.random.RandomState(4).rand(64)
    else:
        c = cases[name]
        GP, Q, off, ys = c["GP"], c["Q"][:300], c["off"], samples(c, 64)
    for clamp, o in ((1e-8, off), (1e-7, 0.0)):
        rc, val = raw_batch(lib, GP, ys, o, Q, clamp)
        assert rc == 0
        mu, s2 = own_posterior(lib, GP, Q, clamp)
        r = mr.from_posterior(mu, s2, ys, o, clamp)
        err = np.abs(val - r["val"])
        print("%s clamp=%g: worst |dev - own| / T = %.3g, MES up to %.3g" % (name, clamp, float(np.max(err / r["T"])), float(np.max(val))))
        assert np.all(err <= 1.25e-12 * r["T"]) and np.all(val > 0) and np.max(val) > 1e-3


# ------------------------------------------------------------------------------------------------ end to end
def assert_end_to_end(dev, r, mu, s2, off, what=""):
    dmu = 1e-6 * np.abs(mu) + 1e-9
    dsig = 1e-6 * s2 / (2.0 * r["sig"])
    tol = 1e-6 * r["T"] + np.abs(r["gmu"]) * dmu + np.abs(r["gsig"]) * dsig
    err = np.abs(dev - r["val"])
    print("%s: worst |dev - ref| / tol = %.3g (max val %.3g)" % (what, float(np.max(err / (tol + 1e-300))), float(np.max(r["val"]))))
    assert np.all(err <= tol), (what, int(np.argmax(err / tol)), float(np.max(err / tol)))


@pytest.mark.parametrize("K", [1, 64, 1024])
@pytest.mark.parametrize("name", FAMILIES)
def test_end_to_end_against_the_restatement(lib, cases, name, K):
    """M = 1000 (four workgroups, the last one partial) against the restatement on the NumPy posterior, MES of the latent function;
    the arg-max of the call is the first arg-max of its values"""
    c = cases[name]
    ys = samples(c, K)
    rc, val, bv, bi = raw_sweep(lib, c["GP"], ys, c["off"], c["dc"])
    assert rc == 0
    mu, s2 = c["post"]
    assert_end_to_end(val, mr.from_posterior(mu, s2, ys, c["off"], 1e-8), mu, s2, c["off"], "%s K=%d" % (name, K))
    assert np.all(val >= 0) and (bi, bv) == cr.argmax(val) and bv > (1e-3 if K > 1 else 0.0)       # (far above mu a term underflows to 0)


# ------------------------------------------------------------------------------------------------ bit equality
@pytest.mark.parametrize("M", [1, 255, 256, 257, 1000])
def test_sweep_batch_gradient_and_chunks_agree_bit_for_bit(lib, cases, M):
    """one candidate array through the sweep (one chunk, and chunks of 256 and 512), the host batch and the gradient entry"""
    c = cases["ard3"]
    GP, off, ys = c["GP"], c["off"], samples(c, 65)
    Q, dc = c["Q"][:M], c["dc"].view_rows(0, M)
    try:
        set_chunk(lib, 0)
        rc, one, bv, bi = raw_sweep(lib, GP, ys, off, dc)
        assert rc == 0
        rcb, b = raw_batch(lib, GP, ys, off, Q)
        rcg, gv, gg = raw_batch(lib, GP, ys, off, Q, grad=True)
        assert rcb == 0 and rcg == 0
        assert np.array_equal(one, b) and np.array_equal(gv, b)
        for m in (256, 512):
            set_chunk(lib, m)
            rc, v, bv2, bi2 = raw_sweep(lib, GP, ys, off, dc)
            assert rc == 0 and np.array_equal(v, one) and (bv2, bi2) == (bv, bi)
            rcb, b2 = raw_batch(lib, GP, ys, off, Q)
            rcg, gv2, gg2 = raw_batch(lib, GP, ys, off, Q, grad=True)
            assert rcb == 0 and rcg == 0 and np.array_equal(b2, one) and np.array_equal(gv2, one) and np.array_equal(gg2, gg)
    finally:
        set_chunk(lib, 0)
    assert (bi, bv) == cr.argmax(one) and one[0] > 0
    assert M == 1 or np.ptp(one) > 0
    assert lib.lib.ibo_set_option(b"mes_chunk", -1) == lib.ERR_ARG


@pytest.mark.parametrize("name", ["iso1", "ard3"])
def test_direct_reports_the_batchs_value_at_its_point(lib, cases, name):
    c = cases[name]
    ys = samples(c, 64)
    rc, opt, optx, ns = raw_direct(lib, c["GP"], ys, c["off"], c["D"], maxiter=8)
    assert rc == 0 and ns > 20 and np.all(optx >= 0) and np.all(optx <= 1)
    rcb, b = raw_batch(lib, c["GP"], ys, c["off"], optx)
    rcg, gv, _ = raw_batch(lib, c["GP"], ys, c["off"], optx, grad=True)
    assert rcb == 0 and rcg == 0 and b[0] == opt and gv[0] == opt                 # bit for bit
    mu, s2 = cr.posterior(c["m"], optx, 1e-8)
    assert_end_to_end(np.array([opt]), mr.from_posterior(mu, s2, ys, c["off"], 1e-8), mu, s2, c["off"], "DIRECT %s" % name)
    rcs, val, _, _ = raw_sweep(lib, c["GP"], ys, c["off"], c["dc"])
    assert rcs == 0 and opt >= np.median(val)


def test_large_class_chunks_batch_and_gradient_agree_bit_for_bit(lib, cases):
    """Chunks above 4096 candidates: the sweep runs on sweep2_kernel.  M = 9000 in one chunk against mes_chunk = 4352 -- two full
    chunks and a tail of 296, padded to 4097 and copied into scratch on the device -- against the host batch and the gradient entry's
    value; the arg-max, index_base and an exclusion ball across the chunk boundaries; and the other class to rounding: 1e-12 of the
    magnitudes of the value's terms and of its derivatives' in the posterior"""
    from ibo_amd import DeviceArray
    c = cases["ard3"]
    GP, off, ys = c["GP"], c["off"], samples(c, 65)
    M, chunk = 9000, 4352
    Q = np.random.RandomState(77).rand(M, 3) * 1.1 - .05
    dc = DeviceArray.from_host(Q)
    try:
        set_chunk(lib, 0)
        rc, one, bv, bi = raw_sweep(lib, GP, ys, off, dc)
        name = last_kernel(lib, GP)
        rcb, b = raw_batch(lib, GP, ys, off, Q)
        rcg, gv, gg = raw_batch(lib, GP, ys, off, Q[:4100], grad=True)
        assert rc == 0 and rcb == 0 and rcg == 0 and name == "sweep2_kernel"
        assert np.array_equal(b, one) and np.array_equal(gv, one[:4100]) and (bi, bv) == cr.argmax(one)
        set_chunk(lib, chunk)
        rc, v, bv2, bi2 = raw_sweep(lib, GP, ys, off, dc)
        assert rc == 0 and np.array_equal(v, one) and (bv2, bi2) == (bv, bi)
        rcb, b2 = raw_batch(lib, GP, ys, off, Q)
        rcg, gv2, gg2 = raw_batch(lib, GP, ys, off, Q[:4500], grad=True)          # (a chunk and a tail of 148)
        assert rcb == 0 and rcg == 0 and np.array_equal(b2, one) and np.array_equal(gv2, one[:4500])
        # the winner moved into the tail and across the boundaries, with index_base
        lo = int(np.argmin(one))
        for i, j in ((2 * chunk - 1, 2 * chunk), (2 * chunk + 5, M - 1), (chunk - 1, chunk)):
            Q2 = Q.copy()
            Q2[bi] = Q[lo]; Q2[i] = Q[bi]; Q2[j] = Q[bi]
            rc, v2, bv3, bi3 = raw_sweep(lib, GP, ys, off, DeviceArray.from_host(Q2), base=(1 << 33) + 5)
            assert rc == 0 and v2[i] == bv and v2[j] == bv and (bi3, bv3) == ((1 << 33) + 5 + i, bv), (i, j)
        # an exclusion ball on the winner while it stands in the tail, whose coordinates the kernel reads from the padded copy
        t = 2 * chunk + 5
        Q2 = Q.copy()
        Q2[bi] = Q[lo]; Q2[t] = Q[bi]
        rc, v3, bve, bie = raw_sweep(lib, GP, ys, off, DeviceArray.from_host(Q2), exclude=Q[bi:bi + 1], radius=1e-3)
        assert rc == 0 and v3[t] == bv
        assert (bie, bve) == cr.argmax(v3, exclude=Q[bi:bi + 1], Q=Q2, radius=1e-3) and bie != t
        # the max-value cdf: the same bits in one chunk and in three
        lev = np.linspace(float(np.max(c["Y"])), float(np.max(c["Y"])) + 2.0, 5)
        rc1, l1, s1 = raw_maxcdf(lib, GP, dc, lev, off)
        set_chunk(lib, 0)
        rc0, l0, s0 = raw_maxcdf(lib, GP, dc, lev, off)
        assert rc0 == 0 and rc1 == 0 and np.array_equal(l0, l1) and np.array_equal(s0, s1)
    finally:
        set_chunk(lib, 0)
    # the two classes agree to rounding
    rows = np.r_[0, 255, 4351, 4352, 8999, bi]
    small = np.array([raw_batch(lib, GP, ys, off, Q[i])[1][0] for i in rows])
    mu, s2 = own_posterior(lib, GP, Q[rows], 1e-8)
    # The classes' posteriors agree to rounding: mu to a few 1e-16 |mu| and s2 = 1 + noise - q to a few 1e-16, which is up to 2e-13 of
    # the latent variance here (>= 1e-3) -- both below 1e-12 of sigma.  A value moves with them by its derivatives, so the magnitudes are
    # those of its own terms (T) and of the terms of sigma dMES/dmu and sigma dMES/dsigma (in the tail, gamma^2 times T).
    r = mr.from_posterior(mu, s2, ys, off, 1e-8)
    mag = r["T"] + r["sig"] * (r["amu"] + r["asig"])
    print("classes: worst |large - small| / magnitudes = %.3g (/ T alone: %.3g)"
          % (float(np.max(np.abs(one[rows] - small) / mag)), float(np.max(np.abs(one[rows] - small) / r["T"]))))
    assert np.all(np.abs(one[rows] - small) <= 1e-12 * mag)
    rc, sm, _, _ = raw_sweep(lib, GP, ys, off, dc.view_rows(0, 1000))
    assert rc == 0 and last_kernel(lib, GP) == "wk_small_kernel"
    assert np.array_equal(sm[[0, 255]], small[:2])                    # (the small class: a sweep of 1000 and one-point batches)


# ------------------------------------------------------------------------------------------------ y* handling
def test_ystar_order_and_the_floor_of_the_latent_variance(lib, cases):
    c = cases["sharp"]
    GP, ys = c["GP"], samples(c, 65)
    rc, v0, bv0, bi0 = raw_sweep(lib, GP, ys, c["off"], c["dc"])
    assert rc == 0
    for seed in (1, 2):
        p = np.random.RandomState(seed).permutation(65)
        rc, v1, bv1, bi1 = raw_sweep(lib, GP, ys[p], c["off"], c["dc"])
        rcg, gv, gg = raw_batch(lib, GP, ys[p], c["off"], c["Q"][:40], grad=True)
        rcg0, gv0, gg0 = raw_batch(lib, GP, ys, c["off"], c["Q"][:40], grad=True)
        assert rc == 0 and np.array_equal(v1, v0) and (bv1, bi1) == (bv0, bi0)
        assert rcg == 0 and rcg0 == 0 and np.array_equal(gv, gv0) and np.array_equal(gg, gg0)
    # an offset above some of the variances: those candidates are evaluated at sigma^2 = clamp_lo, with no variance part in the gradient
    # (at a floor of 1e-3 -- sigma = 0.032 -- so that the samples are within a few deviations of the floored candidates' means)
    Q = np.r_[c["Q"][:150], c["X"][:50] + 1e-3]
    clamp = 1e-3
    mu, s2 = own_posterior(lib, GP, Q, clamp)
    off = float(np.median(s2))
    rc, val, grad = raw_batch(lib, GP, ys, off, Q, clamp, grad=True)
    assert rc == 0
    r = mr.from_posterior(mu, s2, ys, off, clamp)
    fl = ~r["follows"]
    assert 50 <= np.sum(fl) <= 150 and np.all(r["sig"][fl] == np.sqrt(clamp))
    assert np.all(np.abs(val - r["val"]) <= 1.25e-12 * r["T"] + 1e-300)
    g = c["m"].ref.grad(Q, sf2k=c["m"].sf2k, clamp_lo=clamp)
    want = r["gmu"][:, None] * g["dmu"]                                # (where the floor is active: the mean's part alone)
    scale = r["amu"][:, None] * g["smu"]
    gr.assert_grad_close(grad[fl], want[fl], scale[fl], what="floored")
    assert np.max(np.abs(want[fl])) > 0


# ------------------------------------------------------------------------------------------------ gradients
@pytest.mark.parametrize("name,K,M", [("iso1", 1, 7), ("iso1", 65, 129), ("ard3", 2, 7), ("ard3", 65, 129), ("m3", 64, 40), ("m5", 1024, 7)])
def test_gradients_against_the_restatement(lib, cases, name, K, M):
    c = cases[name]
    GP, off, ys, Q = c["GP"], c["off"], samples(c, K), c["Q"][:M]
    rc, val, grad = raw_batch(lib, GP, ys, off, Q, 1e-8, grad=True)
    assert rc == 0
    rg = mr.value_grad(c["m"], Q, ys, off, 1e-8)
    gr.assert_grad_close(grad, rg["dval"], rg["sval"], what="%s K=%d M=%d" % (name, K, M))
    assert np.all(np.isfinite(grad)) and np.max(np.abs(rg["dval"])) > 0
    # the value alone, and the gradient alone
    Qc, yc = lib.f64(Q), lib.f64(ys)
    v2, g2 = np.empty(M), np.empty(Q.shape)
    lead = (GP._handle(), K, lib.dp(yc), off, M, lib.dp(Qc), 1e-8)
    assert lib.lib.ibo_mes_grad_batch(*(lead + (lib.dp(v2), None))) == 0
    assert lib.lib.ibo_mes_grad_batch(*(lead + (None, lib.dp(g2)))) == 0
    assert np.array_equal(v2, val) and np.array_equal(g2, grad)


def test_gradient_against_central_differences_with_a_clipped_variance(lib, cases):
    """a noise-1e-9 model, query 0 on one of its observations: s2 = clamp there (and around it) and the variance's part is 0;
    the restatement, and central differences of ibo_mes_batch at every point"""
    from ibo_amd.gaussianprocess import GaussianProcess
    rs = np.random.RandomState(73)
    X = (np.arange(6)[:, None] / 6.0 + .1 * rs.rand(6, 3)) % 1.0
    Y = np.sin(5 * X[:, 0])
    hyper = [.3 * np.sqrt(3) / 2]
    GP = GaussianProcess(make_kernel("iso", hyper), X, Y, noise=1e-9)
    m = cr.make(X, Y, 1e-9, "iso", hyper)
    Q = cases["ard3"]["Q"][:6].copy()
    Q[0] = X[2]
    clamp = 1e-3                                                       # (sigma = 0.032 there: the samples below are within its reach)
    ys = float(Y[2]) + np.array([.3, .05, .6, -.01, .02])
    assert own_posterior(lib, GP, Q, clamp)[1][0] == clamp
    rc, val, grad = raw_batch(lib, GP, ys, 0.0, Q, clamp, grad=True)
    assert rc == 0
    rg = mr.value_grad(m, Q, ys, 0.0, clamp)
    gr.assert_grad_close(grad, rg["dval"], rg["sval"], what="clipped")
    assert np.max(np.abs(rg["dval"][0])) > 0 and np.all(np.isfinite(grad))
    d = 1e-5
    for j in range(3):
        e = np.zeros(3); e[j] = d
        rcp, vp = raw_batch(lib, GP, ys, 0.0, Q + e, clamp)
        rcm, vm = raw_batch(lib, GP, ys, 0.0, Q - e, clamp)
        assert rcp == 0 and rcm == 0
        fd = (vp - vm) / (2 * d)
        bar = 1e-6 * (rg["sval"][:, j] + rg["T"])
        print("central differences, coordinate %d: worst / bar = %.3g" % (j, float(np.max(np.abs(fd - grad[:, j]) / bar))))
        assert np.all(np.abs(fd - grad[:, j]) <= bar)


# ------------------------------------------------------------------------------------------------ the max-value cdf
@pytest.mark.parametrize("name", ["iso1", "ard3", "m3"])
def test_maxcdf_against_the_ordered_sum(lib, cases, name):
    c = cases[name]
    GP, off, dc, Q = c["GP"], c["off"], c["dc"], c["Q"]
    mu, s2 = own_posterior(lib, GP, Q, 1e-8)
    sig = np.sqrt(np.maximum(s2 - off, 1e-8))
    try:
        set_chunk(lib, 0)
        rc, _, stats = raw_maxcdf(lib, GP, dc, [], off)
        assert rc == 0 and stats[0] == np.max(mu) and stats[1] == np.max(mu + 5.0 * sig)         # the bracket, exactly
        got = {}
        for nlev in (1, 64):
            lev = np.linspace(stats[0], stats[1], nlev) if nlev > 1 else np.array([.5 * (stats[0] + stats[1])])
            rc, lc, st = raw_maxcdf(lib, GP, dc, lev, off)
            assert rc == 0 and np.array_equal(st, stats)
            want, mag, _, _ = mr.maxcdf(mu, s2, lev, off, 1e-8)
            print("%s nlev=%d: worst |dev - ordered sum| / sum|log Phi| = %.3g" % (name, nlev, float(np.max(np.abs(lc - want) / mag))))
            assert np.all(np.abs(lc - want) <= 1e-12 * mag) and np.all(lc <= 0) and np.all(np.diff(lc) >= 0)
            got[nlev] = (lev, lc)
        for m in (256, 512):
            set_chunk(lib, m)
            rc, lc, st = raw_maxcdf(lib, GP, dc, got[64][0], off)
            assert rc == 0 and np.array_equal(lc, got[64][1]) and np.array_equal(st, stats)
        set_chunk(lib, 0)
        # infinite levels pass; a candidate with a NaN coordinate is skipped
        rc, lc, _ = raw_maxcdf(lib, GP, dc, [-np.inf, np.inf], off)
        assert rc == 0 and lc[0] == -np.inf and lc[1] == 0.0
        from ibo_amd import DeviceArray
        Q2 = np.r_[Q[:300], np.full((1, c["D"]), NAN), Q[300:]]
        rc, lc2, st2 = raw_maxcdf(lib, GP, DeviceArray.from_host(Q2), got[64][0], off)
        assert rc == 0 and np.all(np.isfinite(lc2)) and np.array_equal(st2, stats)
        assert np.all(np.abs(lc2 - got[64][1]) <= 1e-12 * mr.maxcdf(mu, s2, got[64][0], off, 1e-8)[1])
        rc, _, st3 = raw_maxcdf(lib, GP, DeviceArray.from_host(np.full((3, c["D"]), NAN)), [], off)
        assert rc == 0 and st3[0] == -np.inf and st3[1] == -np.inf
    finally:
        set_chunk(lib, 0)


# ------------------------------------------------------------------------------------------------ the arg-max contract
def test_argmax_contract(lib, cases):
    from ibo_amd import DeviceArray
    c = cases["ard3"]
    GP, off, ys, Q = c["GP"], c["off"], samples(c, 7), c["Q"]
    rc, base, bv, w = raw_sweep(lib, GP, ys, off, c["dc"])
    assert rc == 0 and (w, bv) == cr.argmax(base) and np.sum(base == bv) == 1
    try:
        # the best candidate twice: the lower index is reported -- at a workgroup's edge, inside the next, and across a chunk boundary
        for chunk, (i, j) in ((0, (255, 256)), (0, (256, 700)), (512, (511, 512)), (512, (300, 999)), (256, (255, 256))):
            set_chunk(lib, chunk)
            Q2 = Q.copy()
            Q2[w] = Q[int(np.argmin(base))]          # the winner leaves its own place ..
            Q2[i] = Q[w]; Q2[j] = Q[w]               # .. and stands at i and at j
            rc, v, bv2, bi2 = raw_sweep(lib, GP, ys, off, DeviceArray.from_host(Q2))
            assert rc == 0 and v[i] == bv and v[j] == bv and (bi2, bv2) == (i, bv), (chunk, i, j)
    finally:
        set_chunk(lib, 0)
    # a NaN coordinate: a NaN value that never wins, wherever it stands
    for pos in (0, w, 999):
        Q3 = Q.copy()
        Q3[pos, 1] = NAN
        rc, v, bv3, bi3 = raw_sweep(lib, GP, ys, off, DeviceArray.from_host(Q3))
        assert rc == 0 and np.isnan(v[pos]) and np.sum(np.isnan(v)) == 1
        assert (bi3, bv3) == cr.argmax(v) and bi3 != pos
        rcb, b = raw_batch(lib, GP, ys, off, Q3[pos])
        assert rcb == 0 and np.isnan(b[0])
    rc, v, bvn, bin_ = raw_sweep(lib, GP, ys, off, DeviceArray.from_host(np.full((3, 3), NAN)))
    assert rc == 0 and np.all(np.isnan(v)) and (bin_, bvn) == (-1, -np.inf)
    # an exclusion ball on the winner: the runner-up wins; everything excluded: (-inf, -1); index_base is added
    rc, v, bve, bie = raw_sweep(lib, GP, ys, off, c["dc"], exclude=Q[w:w + 1], radius=1e-3)
    assert rc == 0 and np.array_equal(v, base) and (bie, bve) == cr.argmax(base, exclude=Q[w:w + 1], Q=Q, radius=1e-3) and bie != w
    rc, _, bva, bia = raw_sweep(lib, GP, ys, off, c["dc"], exclude=[[.5, .5, .5]], radius=10.0)
    assert rc == 0 and (bia, bva) == (-1, -np.inf)
    rc, _, bvb, bib = raw_sweep(lib, GP, ys, off, c["dc"], base=(1 << 33) + 5, want_val=False)
    assert rc == 0 and (bib, bvb) == ((1 << 33) + 5 + w, bv)


def test_scan_time_diagnostic(lib, cases):
    """ibo_set_option("mes_timing", 1): the scan kernels' device time is summed per thread and the values do not change"""
    c = cases["iso1"]
    ys = samples(c, 64)
    ms = ctypes.c_double(-1.0)
    rc, v0, _, _ = raw_sweep(lib, c["GP"], ys, c["off"], c["dc"])
    try:
        lib.check(lib.lib.ibo_set_option(b"mes_timing", 1))
        lib.check(lib.lib.ibo_mes_scan_ms(None, 1))
        rc1, v1, _, _ = raw_sweep(lib, c["GP"], ys, c["off"], c["dc"])
        lib.check(lib.lib.ibo_mes_scan_ms(ctypes.byref(ms), 1))
    finally:
        lib.check(lib.lib.ibo_set_option(b"mes_timing", 0))
    assert rc == 0 and rc1 == 0 and np.array_equal(v0, v1) and 0.0 < ms.value < 50.0
    lib.check(lib.lib.ibo_mes_scan_ms(ctypes.byref(ms), 0))
    assert ms.value == 0.0


# ------------------------------------------------------------------------------------------------ errors
def test_errors(lib, cases):
    from ibo_amd.gaussianprocess import _DeviceGP
    c = cases["ard3"]
    GP, dc = c["GP"], c["dc"].view_rows(0, 4)
    L = lib.lib
    Qc = lib.f64(c["Q"][:4]); out = np.empty(4); grad = np.empty((4, 3)); ys = lib.f64(samples(c, 3))
    lb, ub = lib.f64(np.zeros(3)), lib.f64(np.ones(3))
    opt = ctypes.c_double(); bv = ctypes.c_double(); bi = ctypes.c_int64()
    fresh = _DeviceGP()

    def all_four(h, K=3, yp=lib.dp(ys), off=0.0):
        ld = (h, K, yp, off)
        return [L.ibo_mes_sweep(*(ld + (4, dc.ptr, 1e-8, 0, None, .5, 0, None, ctypes.byref(bv), ctypes.byref(bi)))),
                L.ibo_mes_batch(*(ld + (4, lib.dp(Qc), 1e-8, lib.dp(out)))),
                L.ibo_mes_grad_batch(*(ld + (4, lib.dp(Qc), 1e-8, lib.dp(out), lib.dp(grad)))),
                L.ibo_mes_direct_max(*(ld + (3, lib.dp(lb), lib.dp(ub), 1e-8, 3, 5, 100, 1, ctypes.byref(opt), None, None)))]

    ARG, STATE = lib.ERR_ARG, lib.ERR_STATE
    h = GP._handle()
    assert all_four(h) == [0] * 4
    assert all_four(None) == [ARG] * 4 and all_four(fresh.h) == [STATE] * 4
    assert all_four(h, K=0) == [ARG] * 4 and all_four(h, yp=None) == [ARG] * 4 and all_four(h, off=-1.0) == [ARG] * 4
    ld = (h, 3, lib.dp(ys), 0.0)
    assert L.ibo_mes_sweep(*(ld + (4, dc.ptr, 1e-8, 0, None, .5, 0, None, None, None))) == ARG
    assert L.ibo_mes_batch(*(ld + (4, lib.dp(Qc), 1e-8, None))) == ARG
    assert L.ibo_mes_grad_batch(*(ld + (4, lib.dp(Qc), 1e-8, None, None))) == ARG
    assert L.ibo_mes_direct_max(*(ld + (3, lib.dp(lb), lib.dp(ub), 1e-8, 3, 5, 100, 1, None, None, None))) == ARG
    assert L.ibo_mes_sweep(*(ld + (0, dc.ptr, 1e-8, 0, None, .5, 0, None, ctypes.byref(bv), ctypes.byref(bi)))) == ARG
    assert L.ibo_mes_batch(*(ld + (4, None, 1e-8, lib.dp(out)))) == ARG
    assert L.ibo_mes_direct_max(*(ld + (2, lib.dp(lb), lib.dp(ub), 1e-8, 3, 5, 100, 1, ctypes.byref(opt), None, None))) == ARG
    assert L.ibo_mes_direct_max(*(ld + (3, None, lib.dp(ub), 1e-8, 3, 5, 100, 1, ctypes.byref(opt), None, None))) == ARG
    assert L.ibo_mes_sweep(*(ld + (4, dc.ptr, 1e-8, 2, None, .5, 0, None, ctypes.byref(bv), ctypes.byref(bi)))) == ARG      # exclusions without centres
    stats = np.empty(2)
    assert L.ibo_mes_maxcdf(None, 4, dc.ptr, 0, None, 0.0, 1e-8, None, lib.dp(stats)) == ARG
    assert L.ibo_mes_maxcdf(fresh.h, 4, dc.ptr, 0, None, 0.0, 1e-8, None, lib.dp(stats)) == STATE
    assert L.ibo_mes_maxcdf(h, 0, dc.ptr, 0, None, 0.0, 1e-8, None, lib.dp(stats)) == ARG
    assert L.ibo_mes_maxcdf(h, 4, None, 0, None, 0.0, 1e-8, None, lib.dp(stats)) == ARG
    assert L.ibo_mes_maxcdf(h, 4, dc.ptr, 0, None, 0.0, 1e-8, None, None) == ARG
    fresh.close()


# ------------------------------------------------------------------------------------------------ the Python layer
def test_python_layer_against_the_abi(lib, cases):
    from ibo_amd.acquisition import entropy as en
    c = cases["ard3"]
    GP, Q, D = c["GP"], c["Q"], c["D"]
    bounds = [[0., 1.]] * D
    ys = samples(c, 64)
    off = en._offset(GP, True)
    assert off == c["off"] and en._offset(GP, False) == 0.0
    # the class, the sweep
    o = en.MaxValueEntropy(GP, ys)
    rc, bval, bgrad = raw_batch(lib, GP, ys, off, Q[:40], 1e-7, grad=True)
    assert rc == 0
    v, gg = o.gradient(Q[:40])
    assert np.array_equal(o.values(Q[:40]), bval) and np.array_equal(v, bval) and np.array_equal(gg, bgrad)
    assert o.f(Q[3]) == o.values(Q[3])[0] == bval[3] and o.negf(Q[3]) == -bval[3]
    nv, ng = o.negf_grad(Q[3])
    assert nv == -bval[3] and np.array_equal(ng, -bgrad[3]) and np.array_equal(o.ystar, np.sort(ys))
    rc, b0 = raw_batch(lib, GP, ys, 0.0, Q[:40], 1e-7)
    assert rc == 0 and np.array_equal(en.MaxValueEntropy(GP, ys, latent=False).values(Q[:40]), b0)
    r = en.sweepMES(GP, c["dc"], ys, outputs=True)
    rc, val, bv, bi = raw_sweep(lib, GP, ys, off, c["dc"], 1e-7)
    assert rc == 0 and np.array_equal(r["val"], val) and (r["best_val"], r["best_idx"]) == (bv, bi)
    r = en.sweepMES(GP, Q, ys, exclude=Q[bi:bi + 1], radius=1e-3, index_base=100)
    assert r["best_idx"] == 100 + cr.argmax(val, exclude=Q[bi:bi + 1], Q=Q, radius=1e-3)[0] and "val" not in r
    # samples of the maximum: reproducible under a seed in both methods, the Gumbel ones made of the ABI's numbers
    for method, n in (("gumbel", 64), ("paths", 8)):
        s1 = en.maxValueSamples(GP, bounds, n=n, method=method, seed=5)
        s2 = en.maxValueSamples(GP, bounds, n=n, method=method, seed=5)
        s3 = en.maxValueSamples(GP, bounds, n=n, method=method, seed=6)
        assert s1.shape == (n,) and np.array_equal(s1, s2) and not np.array_equal(s1, s3) and np.all(np.isfinite(s1))
    sg = en.maxValueSamples(GP, candidates=c["dc"], n=64, seed=5)
    rc, _, stats = raw_maxcdf(lib, GP, c["dc"], [], off, 1e-7)
    lev = np.linspace(stats[0], stats[1], 64)
    rc2, lc, _ = raw_maxcdf(lib, GP, c["dc"], lev, off, 1e-7)
    a, b, q = mr.gumbel_fit(lev, lc)
    assert rc == 0 and rc2 == 0 and np.array_equal(sg, mr.gumbel_samples(a, b, stats[0], 64, 5))
    assert np.all(sg >= stats[0]) and stats[0] < np.median(sg) < stats[1]
    # exact and approximate samples tell the same story: the medians within the bracket's width of each other
    sp = en.maxValueSamples(GP, bounds, n=32, method="paths", seed=1)
    assert abs(np.median(sp) - np.median(sg)) < stats[1] - stats[0]
    # the maximiser: DIRECT's value is the class's at its point; polish never loses
    v0, x0 = en.maximizeMES(GP, bounds, ystar=ys, maxiter=8)
    v1, x1 = en.maximizeMES(GP, bounds, ystar=ys, maxiter=8, polish=True)
    assert v1 >= v0 > 0 and np.all(x1 >= 0) and np.all(x1 <= 1) and o.f(x0) == v0 and o.f(x1) == v1
    v2, x2 = en.maximizeMES(GP, bounds, n_samples=16, seed=3, maxiter=5)
    assert v2 > 0 and en.MaxValueEntropy(GP, en.maxValueSamples(GP, bounds, n=16, seed=3)).f(x2) == v2


def test_python_layer_on_a_preference_gp(lib):
    from ibo_amd.acquisition import entropy as en
    GP = pref_model(3)
    bounds = [[0., 1.]] * 3
    ys = en.maxValueSamples(GP, bounds, n=32, seed=2)
    assert ys.shape == (32,) and np.all(np.isfinite(ys)) and np.array_equal(ys, en.maxValueSamples(GP, bounds, n=32, seed=2))
    with pytest.raises(NotImplementedError):
        en.maxValueSamples(GP, bounds, n=8, method="paths")
    assert en._offset(GP, True) == 0.0
    o = en.MaxValueEntropy(GP, ys)
    Q = np.random.RandomState(3).rand(20, 3)
    rc, b, g = raw_batch(lib, GP, ys, 0.0, Q, 1e-7, grad=True)
    v, gg = o.gradient(Q)
    assert rc == 0 and np.array_equal(v, b) and np.array_equal(gg, g) and np.all(b > 0) and np.all(np.isfinite(g))
    v0, x0 = en.maximizeMES(GP, bounds, ystar=ys, maxiter=6)
    v1, x1 = en.maximizeMES(GP, bounds, ystar=ys, maxiter=6, polish=True)
    assert v1 >= v0 > 0 and o.f(x0) == v0
    r = en.sweepMES(GP, Q, ys, outputs=True)
    assert np.array_equal(r["val"], b) and r["best_idx"] == int(np.argmax(b))

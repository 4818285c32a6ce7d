"""
The two-objective expected hypervolume improvement on the device: ibo_ehvi_sweep / ibo_ehvi_batch / ibo_ehvi_grad_batch /
ibo_ehvi_direct_max and ibo_amd.acquisition.multiobjective on top of them.

Tolerances (S, bar: the magnitude of the terms and psi_1(r1) + psi_2(r2), tests/ehvi_reference.py)
  * end to end, against the restatement (pinned by tests/test_ehvi_reference.py): |dev - ref| <= 1e-6 S + 1e-9 bar -- the suite's
    relative bar for an acquisition on the terms' magnitude, plus the posterior mean's absolute bar (1e-9) times the bound on
    dEHVI/dmu_1 + dEHVI/dmu_2;
  * composition: the restatement evaluated on the library's OWN (mu, s2) from ibo_posterior_batch at the same clamp: 1e-12 S;
  * bit equality between the entries and across chunk sizes: np.array_equal;
  * gradients: 1e-9 of the scale + 1e-13, as tests/test_gpu_constrained.py.
The models have 25 to 200 rows.  Up to 4096 candidates per chunk the per-model sweeps run on the small-batch kernels, and short
launches are padded to 160 candidates; test_large_class_* covers the other size class (chunks above 4096, sweep2_kernel, tails padded to
4097).  The return for models on different devices is NOT exercised: the suite sees one device.
"""
import ctypes

import numpy as np
import pytest

import grad_reference as gr
import cacq_reference as cr
import ehvi_reference as er

pytestmark = pytest.mark.gpu

NAN = float("nan")
CASES = sorted(er.GEN)


@pytest.fixture(scope="module")
def lib():
    from ibo_amd import _lib
    if _lib.device_count() < 1:
        pytest.fail("no GPU visible: the product has no CPU fallback")
    return _lib


def make_kernel(kind, hyper):
    from ibo_amd.gaussianprocess import kernel as K
    return {"ard": K.GaussianKernel_ard, "iso": K.GaussianKernel_iso, "svard": K.SVGaussianKernel_ard,
            "sviso": K.SVGaussianKernel_iso, "m3": K.MaternKernel3, "m5": K.MaternKernel5}[kind](np.array(hyper, dtype=float))


@pytest.fixture(scope="module")
def cases(lib):
    """per generator case: the two GaussianProcess objects (observed at different points; d3's first has a mean prior), the
    restated models and the candidates on the device"""
    from ibo_amd import DeviceArray
    from ibo_amd.gaussianprocess import GaussianProcess
    from ibo_amd.gaussianprocess.prior import RBFNMeanPrior
    out = {}
    for name in CASES:
        g = er.generator(name)
        GPs = []
        for k, (kind, hyper, N, seed, with_prior) in enumerate(g["spec"]):
            prior = None
            if with_prior:
                prior = RBFNMeanPrior()
                prior.means, prior.beta, prior.theta, prior.lowerb, prior.width = g["prior"][k]
            GP = GaussianProcess(make_kernel(kind, hyper), g["X"][k], g["Y"][k], prior=prior, noise=er.GEN_NOISE)
            GP._push_prior()
            # the restatement's k* variance is the one the raw calls below run with (the Python one)
            assert abs(GP.kernel._ibo_spec()[2] - g["models"][k].sf2k) < 1e-15
            GPs.append(GP)
        out[name] = dict(g=g, GPs=GPs, dc=DeviceArray.from_host(g["Q"]))
    return out


def lead(lib, GPs, F, ref):
    F = lib.f64(np.asarray(F, dtype=float).reshape(-1, 2))
    r = lib.f64(ref)
    objs = (ctypes.c_void_p * 2)(*[GP._handle() for GP in GPs])
    return (objs, len(F), lib.dp(F) if len(F) else None, lib.dp(r)), (F, r, objs)


def raw_sweep(lib, GPs, F, ref, dc, erf_mode=0, clamp=1e-8, exclude=None, radius=.5, base=0, want_val=True):
    """(rc, val or None, best_val, best_idx) of ibo_ehvi_sweep"""
    from ibo_amd import DeviceArray
    M = dc.shape[0]
    ld, keep = lead(lib, GPs, F, ref)
    val = DeviceArray((M,)) if want_val else None
    if val is not None:
        val.upload(np.full(M, 7.25))
    ex = None if exclude is None else lib.f64(np.atleast_2d(exclude))
    bv = ctypes.c_double(-5.0); bi = ctypes.c_int64(-5)
    rc = lib.lib.ibo_ehvi_sweep(*(ld + (M, dc.ptr, erf_mode, clamp, 0 if ex is None else len(ex), None if ex is None else lib.dp(ex),
                                        radius, base, None if val is None else val.ptr, ctypes.byref(bv), ctypes.byref(bi))))
    return rc, (val.to_host() if val is not None and rc == 0 else None), bv.value, bi.value


def raw_batch(lib, GPs, F, ref, Q, erf_mode=0, clamp=1e-8, grad=False):
    """(rc, val) of ibo_ehvi_batch, or (rc, val, grad) of ibo_ehvi_grad_batch"""
    Q = lib.f64(np.atleast_2d(Q))
    M, D = Q.shape
    ld, keep = lead(lib, GPs, F, ref)
    val = np.full(M, 7.25)
    if not grad:
        return lib.lib.ibo_ehvi_batch(*(ld + (M, lib.dp(Q), erf_mode, clamp, lib.dp(val)))), val
    g = np.full((M, D), 7.25)
    return lib.lib.ibo_ehvi_grad_batch(*(ld + (M, lib.dp(Q), erf_mode, clamp, lib.dp(val), lib.dp(g)))), val, g


def raw_direct(lib, GPs, F, ref, D, erf_mode=0, clamp=1e-8, maxiter=8):
    ld, keep = lead(lib, GPs, F, ref)
    lb, ub = lib.f64(np.zeros(D)), lib.f64(np.ones(D))
    opt = ctypes.c_double(); optx = np.empty(D); ns = ctypes.c_int64()
    rc = lib.lib.ibo_ehvi_direct_max(*(ld + (D, lib.dp(lb), lib.dp(ub), erf_mode, clamp, maxiter, 30, 10000, 1,
                                             ctypes.byref(opt), lib.dp(optx), ctypes.byref(ns))))
    return rc, opt.value, optx, ns.value


def assert_end_to_end(dev, ref, what=""):
    err = np.abs(dev - ref["val"])
    tol = 1e-6 * ref["S"] + 1e-9 * ref["bar"]
    print("%s: worst |dev - ref| / tol = %.3g (max val %.3g)" % (what, float(np.max(err / tol)), float(np.max(ref["val"]))))
    assert np.all(err <= tol), (what, int(np.argmax(err / tol)), float(np.max(err / tol)))


def set_chunk(lib, m):
    lib.check(lib.lib.ibo_set_option(b"ehvi_chunk", int(m)))


# ------------------------------------------------------------------------------------------------ front sizes, end to end
@pytest.mark.parametrize("n", er.FRONT_SIZES)
@pytest.mark.parametrize("name", CASES)
def test_front_sizes_against_the_restatement(lib, cases, name, n):
    """M = 1000 (four workgroups, the last one partial), every front size: empty, short, either side of a wavefront's 64 and the
    LDS array's limit; libm erf at clamp 1e-8, and the NR flavour at 65; the arg-max of the call is the first arg-max of its values"""
    c = cases[name]
    g = c["g"]
    F = er.gen_front(name, n)
    for erf_mode in ((0, 1) if n == 65 else (0,)):
        rc, val, bv, bi = raw_sweep(lib, c["GPs"], F, g["ref"], c["dc"], erf_mode, 1e-8)
        assert rc == 0
        assert_end_to_end(val, er.gen_value(name, n, erf_mode), "%s n=%d erf=%d" % (name, n, erf_mode))
        assert np.all(val >= 0.0)
        assert (bi, bv) == cr.argmax(val)
        assert bv > 1e-3


# ------------------------------------------------------------------------------------------------ composition
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


def own_posterior(lib, GP, Q, clamp):
    Q = lib.f64(Q)
    mu, s2 = np.empty(len(Q)), np.empty(len(Q))
    lib.check(lib.lib.ibo_posterior_batch(GP._handle(), len(Q), lib.dp(Q), clamp, lib.dp(mu), lib.dp(s2)))
    return mu, s2


@pytest.mark.parametrize("pairing", ["d1", "d3", "pref_first", "pref_second"])
def test_composition_of_the_librarys_own_posteriors(lib, cases, pairing):
    """the restatement's walk on (mu, s2) of ibo_posterior_batch at the same clamp: 1e-12 S, both flavours, fronts of 2 and 1024;
    a PrefGaussianProcess as either objective"""
    if pairing in cases:
        c = cases[pairing]
        GPs, Q, ref, top = c["GPs"], c["g"]["Q"][:300], c["g"]["ref"], c["g"]["top"]
    else:
        c = cases["d3"]
        GPp = pref_model(3)
        GPs = [GPp, c["GPs"][1]] if pairing == "pref_first" else [c["GPs"][0], GPp]
        Q = c["g"]["Q"][:300]
        k = 0 if pairing == "pref_first" else 1
        ref, top = c["g"]["ref"].copy(), c["g"]["top"].copy()
        mu = own_posterior(lib, GPp, Q, 1e-7)[0]
        ref[k], top[k] = float(np.min(mu)) - .3, float(np.max(mu)) + .1
    for n in (2, 1024):
        F = er.curve_front(n, ref, ref + .7 * (top - ref))
        for erf_mode, clamp in ((0, 1e-8), (1, 1e-7)):
            rc, val = raw_batch(lib, GPs, F, ref, Q, erf_mode, clamp)
            assert rc == 0
            (mu1, s21), (mu2, s22) = own_posterior(lib, GPs[0], Q, clamp), own_posterior(lib, GPs[1], Q, clamp)
            r = er.from_posterior(mu1, s21, mu2, s22, F, ref, erf_mode)
            err = np.abs(val - r["val"])
            print("%s n=%d erf=%d: worst |dev - own| / S = %.3g" % (pairing, n, erf_mode, float(np.max(err / r["S"]))))
            assert np.all(err <= 1e-12 * r["S"])
            assert np.mean(r["val"] > 1e-8) > .8


# ------------------------------------------------------------------------------------------------ bit equality
@pytest.mark.parametrize("M", [1, 255, 256, 257, 1000])
def test_sweep_batch_gradient_and_chunks_agree_bit_for_bit(lib, cases, M):
    """one candidate array through the sweep (one chunk, and chunks of 256 and 512), the host batch and the gradient entry"""
    c = cases["d3"]
    g = c["g"]
    F = er.gen_front("d3", 65)
    Q, dc = g["Q"][:M], c["dc"].view_rows(0, M)
    try:
        set_chunk(lib, 0)
        rc, one, bv, bi = raw_sweep(lib, c["GPs"], F, g["ref"], dc)
        assert rc == 0
        rcb, b = raw_batch(lib, c["GPs"], F, g["ref"], Q)
        rcg, gv, gg = raw_batch(lib, c["GPs"], F, g["ref"], Q, grad=True)
        assert rcb == 0 and rcg == 0
        assert np.array_equal(one, b) and np.array_equal(gv, b)
        for m in (256, 512):
            set_chunk(lib, m)
            rc, v, bv2, bi2 = raw_sweep(lib, c["GPs"], F, g["ref"], dc)
            assert rc == 0 and np.array_equal(v, one) and (bv2, bi2) == (bv, bi)
            rcb, b2 = raw_batch(lib, c["GPs"], F, g["ref"], Q)
            assert rcb == 0 and np.array_equal(b2, one)
    finally:
        set_chunk(lib, 0)
    assert (bi, bv) == cr.argmax(one) and one[0] > 0
    assert M == 1 or np.ptp(one) > 0
    assert lib.lib.ibo_set_option(b"ehvi_chunk", -1) == lib.ERR_ARG


def test_large_class_chunks_batch_and_gradient_agree_bit_for_bit(lib, cases):
    """Chunks above 4096 candidates: the per-model sweeps run on sweep2_kernel.  M = 9000 in one chunk against ehvi_chunk = 4352 --
    two full chunks and a tail of 296, which is padded to 4097 and copied into scratch on the device -- against the host batch and
    the gradient entry's value on the same points; the arg-max and index_base across the chunk boundaries; and the other class
    (one-point batches, small-batch kernels padded to 160) to rounding: 1e-12 S, the composition's bar."""
    from ibo_amd import DeviceArray
    c = cases["d3"]
    g = c["g"]
    GPs, ref = c["GPs"], g["ref"]
    F = er.gen_front("d3", 65)
    M, chunk = 9000, 4352
    Q = np.random.RandomState(77).rand(M, 3) * 1.1 - .05
    dc = DeviceArray.from_host(Q)
    names = []
    try:
        set_chunk(lib, 0)
        rc, one, bv, bi = raw_sweep(lib, GPs, F, ref, dc)
        names = [last_kernel(lib, GP) for GP in GPs]
        rcb, b = raw_batch(lib, GPs, F, ref, Q)
        rcg, gv, gg = raw_batch(lib, GPs, F, ref, Q[:4100], grad=True)
        assert rc == 0 and rcb == 0 and rcg == 0
        assert names == ["sweep2_kernel", "sweep2_kernel"]
        assert np.array_equal(b, one) and np.array_equal(gv, one[:4100])
        assert (bi, bv) == cr.argmax(one)
        set_chunk(lib, chunk)
        rc, v, bv2, bi2 = raw_sweep(lib, GPs, F, ref, dc)
        assert rc == 0 and np.array_equal(v, one) and (bv2, bi2) == (bv, bi)
        assert [last_kernel(lib, GP) for GP in GPs] == names           # the padded tail too
        rcb, b2 = raw_batch(lib, GPs, F, ref, Q)
        rcg, gv2, gg2 = raw_batch(lib, GPs, F, ref, Q[:4500], grad=True)       # (a chunk and a tail of 148)
        assert rcb == 0 and rcg == 0 and np.array_equal(b2, one) and np.array_equal(gv2, one[:4500])
        # the winner moved into the tail, twice across the last boundary, and index_base
        lo = int(np.argmin(one))
        for i, j in ((2 * chunk - 1, 2 * chunk), (2 * chunk + 5, M - 1), (chunk - 1, chunk)):
            Q2 = Q.copy()
            Q2[bi] = Q[lo]; Q2[i] = Q[bi]; Q2[j] = Q[bi]
            rc, v2, bv3, bi3 = raw_sweep(lib, GPs, F, ref, DeviceArray.from_host(Q2), base=(1 << 33) + 5)
            assert rc == 0 and v2[i] == bv and v2[j] == bv and (bi3, bv3) == ((1 << 33) + 5 + i, bv), (i, j)
        # an exclusion ball on the winner while it stands in the tail, whose coordinates the kernel reads from the padded copy
        t = 2 * chunk + 5
        Q2 = Q.copy()
        Q2[bi] = Q[lo]; Q2[t] = Q[bi]
        rc, v3, bve, bie = raw_sweep(lib, GPs, F, ref, DeviceArray.from_host(Q2), exclude=Q[bi:bi + 1], radius=1e-3)
        assert rc == 0 and v3[t] == bv
        assert (bie, bve) == cr.argmax(v3, exclude=Q[bi:bi + 1], Q=Q2, radius=1e-3) and bie != t
    finally:
        set_chunk(lib, 0)
    # the two classes agree to rounding
    rows = np.r_[0, 255, 4351, 4352, 8999, bi]
    small = np.array([raw_batch(lib, GPs, F, ref, Q[i])[1][0] for i in rows])
    (mu1, s21), (mu2, s22) = own_posterior(lib, GPs[0], Q[rows], 1e-8), own_posterior(lib, GPs[1], Q[rows], 1e-8)
    S = er.from_posterior(mu1, s21, mu2, s22, F, ref)["S"]
    print("classes: worst |large - small| / S = %.3g" % float(np.max(np.abs(one[rows] - small) / S)))
    assert np.all(np.abs(one[rows] - small) <= 1e-12 * S)
    rc, sm, _, _ = raw_sweep(lib, GPs, F, ref, dc.view_rows(0, 1000))
    assert rc == 0 and [last_kernel(lib, GP) for GP in GPs] == ["wk_small_kernel", "wk_small_kernel"]
    assert np.array_equal(sm[[0, 255]], small[:2])                    # (the small class: a sweep of 1000 and one-point batches)


def last_kernel(lib, GP):
    ms = ctypes.c_float(); name = ctypes.c_char_p()
    lib.check(lib.lib.ibo_last_sweep_kernel_ms(GP._handle(), ctypes.byref(ms), ctypes.byref(name)))
    return name.value.decode()


def test_scan_time_diagnostic(lib, cases):
    """ibo_set_option("ehvi_timing", 1): the scan kernel's device time is summed per thread and the values do not change"""
    c = cases["d1"]
    g = c["g"]
    F = er.gen_front("d1", 64)
    ms = ctypes.c_double(-1.0)
    rc, v0, _, _ = raw_sweep(lib, c["GPs"], F, g["ref"], c["dc"])
    try:
        lib.check(lib.lib.ibo_set_option(b"ehvi_timing", 1))
        lib.check(lib.lib.ibo_ehvi_scan_ms(None, 1))
        rc1, v1, _, _ = raw_sweep(lib, c["GPs"], F, g["ref"], c["dc"])
        lib.check(lib.lib.ibo_ehvi_scan_ms(ctypes.byref(ms), 1))
    finally:
        lib.check(lib.lib.ibo_set_option(b"ehvi_timing", 0))
    assert rc == 0 and rc1 == 0 and np.array_equal(v0, v1) and 0.0 < ms.value < 50.0
    lib.check(lib.lib.ibo_ehvi_scan_ms(ctypes.byref(ms), 0))
    assert ms.value == 0.0


@pytest.mark.parametrize("name", CASES)
def test_direct_reports_the_batchs_value_at_its_point(lib, cases, name):
    c = cases[name]
    g = c["g"]
    F = er.gen_front(name, 64)
    rc, opt, optx, ns = raw_direct(lib, c["GPs"], F, g["ref"], g["D"], maxiter=8)
    assert rc == 0 and ns > 20 and np.all(optx >= 0) and np.all(optx <= 1)
    rcb, b = raw_batch(lib, c["GPs"], F, g["ref"], optx)
    assert rcb == 0 and b[0] == opt                                  # bit for bit
    r = er.value(g["models"], optx, F, g["ref"], gr.ERF_LIBM, 1e-8)
    assert_end_to_end(np.array([opt]), r, "DIRECT %s" % name)
    # DIRECT does at least as well as the median candidate
    assert opt >= np.median(er.gen_value(name, 64)["val"])


# ------------------------------------------------------------------------------------------------ gradients
@pytest.mark.parametrize("erf_mode", [0, 1])
@pytest.mark.parametrize("name,n,M", [("d1", 0, 7), ("d1", 65, 129), ("d3", 2, 7), ("d3", 65, 129), ("d3", 1024, 7)])
def test_gradients_against_the_restatement(lib, cases, name, n, M, erf_mode):
    c = cases[name]
    g = c["g"]
    F = er.gen_front(name, n)
    Q = g["Q"][:M]
    clamp = 1e-8 if erf_mode == 0 else 1e-7
    rc, val, grad = raw_batch(lib, c["GPs"], F, g["ref"], Q, erf_mode, clamp, grad=True)
    assert rc == 0
    rg = er.value_grad(g["models"], Q, F, g["ref"], erf_mode, clamp)
    gr.assert_grad_close(grad, rg["dval"], rg["sval"], what="%s n=%d M=%d erf=%d" % (name, n, M, erf_mode))
    assert np.all(np.isfinite(grad)) and np.max(np.abs(rg["dval"])) > 1e-3
    # the value alone, and the gradient alone
    ld, keep = lead(lib, c["GPs"], F, g["ref"])
    Qc = lib.f64(Q)
    v2, g2 = np.empty(M), np.empty(Q.shape)
    assert lib.lib.ibo_ehvi_grad_batch(*(ld + (M, lib.dp(Qc), erf_mode, clamp, lib.dp(v2), None))) == 0
    assert lib.lib.ibo_ehvi_grad_batch(*(ld + (M, lib.dp(Qc), erf_mode, clamp, None, lib.dp(g2)))) == 0
    assert np.array_equal(v2, val) and np.array_equal(g2, grad)


def test_gradient_where_a_variance_is_clipped(lib, cases):
    """a noise-1e-9 model as the second objective, query 0 on one of its observations: s2 = clamp there and dsigma_2 = 0"""
    from ibo_amd.gaussianprocess import GaussianProcess
    c = cases["d3"]
    g = c["g"]
    rs = np.random.RandomState(73)
    X = (np.arange(6)[:, None] / 6.0 + .1 * rs.rand(6, 3)) % 1.0
    Y = np.sin(5 * X[:, 0])
    hyper = [.3 * np.sqrt(3) / 2]
    GPk = GaussianProcess(make_kernel("iso", hyper), X, Y, noise=1e-9)
    mk = cr.make(X, Y, 1e-9, "iso", hyper)
    Q = g["Q"][:5].copy()
    Q[0] = X[2]
    ref = np.array([g["ref"][0], -1.5])
    F = np.array([[g["ref"][0] + .5, float(Y[2]) - 2e-4], [g["ref"][0] + 1., -1.]])     # b_1 a fraction of sigma = 3.2e-4 below mu_2 there
    clamp = 1e-7
    assert own_posterior(lib, GPk, Q, clamp)[1][0] == clamp
    GPs, models = [c["GPs"][0], GPk], [g["models"][0], mk]
    rc, val, grad = raw_batch(lib, GPs, F, ref, Q, 1, clamp, grad=True)
    assert rc == 0
    rg = er.value_grad(models, Q, F, ref, 1, clamp)
    assert_end_to_end(val, er.value(models, Q, F, ref, 1, clamp), "clipped")
    gr.assert_grad_close(grad, rg["dval"], rg["sval"], what="clipped")
    assert np.max(np.abs(rg["dval"][0])) > 0 and np.all(np.isfinite(grad))


# ------------------------------------------------------------------------------------------------ the arg-max contract
def test_argmax_contract(lib, cases):
    from ibo_amd import DeviceArray
    c = cases["d3"]
    g = c["g"]
    GPs, ref = c["GPs"], g["ref"]
    F = er.gen_front("d3", 7)
    Q = g["Q"]
    rc, base, bv, w = raw_sweep(lib, GPs, F, ref, c["dc"])
    assert rc == 0 and (w, bv) == cr.argmax(base) and np.sum(base == bv) == 1
    try:
        # the best candidate twice: the lower index is reported -- at a workgroup's edge, inside the next, and across a chunk boundary
        for chunk, (i, j) in ((0, (255, 256)), (0, (256, 700)), (512, (511, 512)), (512, (300, 999)), (256, (255, 256))):
            set_chunk(lib, chunk)
            Q2 = Q.copy()
            Q2[w] = Q[int(np.argmin(base))]          # the winner leaves its own place ..
            Q2[i] = Q[w]; Q2[j] = Q[w]               # .. and stands at i and at j
            rc, v, bv2, bi2 = raw_sweep(lib, GPs, F, ref, DeviceArray.from_host(Q2))
            assert rc == 0 and v[i] == bv and v[j] == bv and (bi2, bv2) == (i, bv), (chunk, i, j)
        set_chunk(lib, 0)
    finally:
        set_chunk(lib, 0)
    # a NaN coordinate: a NaN value that never wins, wherever it stands
    for pos in (0, w, 999):
        Q3 = Q.copy()
        Q3[pos, 1] = NAN
        rc, v, bv3, bi3 = raw_sweep(lib, GPs, F, ref, DeviceArray.from_host(Q3))
        assert rc == 0 and np.isnan(v[pos]) and np.sum(np.isnan(v)) == 1
        assert (bi3, bv3) == cr.argmax(v) and bi3 != pos
        rcb, b = raw_batch(lib, GPs, F, ref, Q3[pos])
        assert rcb == 0 and np.isnan(b[0])
    allnan = np.full((3, 3), NAN)
    rc, v, bvn, bin_ = raw_sweep(lib, GPs, F, ref, DeviceArray.from_host(allnan))
    assert rc == 0 and np.all(np.isnan(v)) and (bin_, bvn) == (-1, -np.inf)
    # an exclusion ball on the winner: the runner-up wins; everything excluded: (-inf, -1); index_base is added
    rc, v, bve, bie = raw_sweep(lib, GPs, F, ref, c["dc"], exclude=Q[w:w + 1], radius=1e-3)
    assert rc == 0 and np.array_equal(v, base) and (bie, bve) == cr.argmax(base, exclude=Q[w:w + 1], Q=Q, radius=1e-3) and bie != w
    rc, _, bva, bia = raw_sweep(lib, GPs, F, ref, c["dc"], exclude=[[.5, .5, .5]], radius=10.0)
    assert rc == 0 and (bia, bva) == (-1, -np.inf)
    rc, _, bvb, bib = raw_sweep(lib, GPs, F, ref, c["dc"], base=(1 << 33) + 5, want_val=False)
    assert rc == 0 and (bib, bvb) == ((1 << 33) + 5 + w, bv)
    # outputs one by one
    ld, keep = lead(lib, GPs, F, ref)
    bi = ctypes.c_int64(-5); bvv = ctypes.c_double()
    assert lib.lib.ibo_ehvi_sweep(*(ld + (1000, c["dc"].ptr, 0, 1e-8, 0, None, .5, 0, None, None, ctypes.byref(bi)))) == 0 and bi.value == w
    assert lib.lib.ibo_ehvi_sweep(*(ld + (1000, c["dc"].ptr, 0, 1e-8, 0, None, .5, 0, None, ctypes.byref(bvv), None))) == 0 and bvv.value == bv


# ------------------------------------------------------------------------------------------------ sanity
def test_sanity_one_model_twice_and_a_dominating_point(lib, cases):
    c = cases["d1"]
    g = c["g"]
    GP, m = c["GPs"][0], g["models"][0]
    Q = g["Q"][:300]
    big = np.array([-50., -50.])
    F1 = np.array([[.2, .1]])
    rc, val = raw_batch(lib, [GP, GP], F1, big, Q)
    assert rc == 0
    assert_end_to_end(val, er.value([m, m], Q, F1, big, gr.ERF_LIBM, 1e-8), "one model twice")
    assert np.all(val > 0)
    # a point that dominates the whole front: no candidate's value rises -- in the restatement and on the device
    for name in CASES:
        c = cases[name]
        g = c["g"]
        F = er.gen_front(name, 63)
        a, b = er.canonical(F, g["ref"])
        Fd = np.vstack([F, [[a[-1] + .05, b[0] + .05]]])
        assert len(er.canonical(Fd, g["ref"])[0]) == 1
        (mu1, s21), (mu2, s22) = g["post"]
        r0 = er.gen_value(name, 63)["val"]
        r1 = er.from_posterior(mu1, s21, mu2, s22, Fd, g["ref"])["val"]
        assert np.all(r1 <= r0) and np.mean(r1 < r0) > .9
        rc0, v0, _, _ = raw_sweep(lib, c["GPs"], F, g["ref"], c["dc"])
        rc1, v1, _, _ = raw_sweep(lib, c["GPs"], Fd, g["ref"], c["dc"])
        assert rc0 == 0 and rc1 == 0
        assert np.all(v1 <= v0) and np.all(v1 >= 0) and np.mean(v1 < v0) > .9


# ------------------------------------------------------------------------------------------------ errors
def test_errors(lib, cases):
    from ibo_amd import DeviceArray
    from ibo_amd.gaussianprocess import GaussianProcess, _DeviceGP
    c3, c1 = cases["d3"], cases["d1"]
    g = c3["g"]
    GPs, ref = c3["GPs"], g["ref"]
    F = er.gen_front("d3", 2)
    Q = g["Q"][:4]
    dc = c3["dc"].view_rows(0, 4)
    fresh = _DeviceGP()
    L = lib.lib
    out = np.empty(4); grad = np.empty((4, 3)); Qc = lib.f64(Q)
    lb, ub = lib.f64(np.zeros(3)), lib.f64(np.ones(3))
    opt = ctypes.c_double(); bv = ctypes.c_double(); bi = ctypes.c_int64()

    def all_four(objs, nfront, front, refp, erf_mode=0):
        """the four entries' return codes for one set of leading arguments"""
        ld = (objs, nfront, front, refp)
        return [L.ibo_ehvi_sweep(*(ld + (4, dc.ptr, erf_mode, 1e-8, 0, None, .5, 0, None, ctypes.byref(bv), ctypes.byref(bi)))),
                L.ibo_ehvi_batch(*(ld + (4, lib.dp(Qc), erf_mode, 1e-8, lib.dp(out)))),
                L.ibo_ehvi_grad_batch(*(ld + (4, lib.dp(Qc), erf_mode, 1e-8, lib.dp(out), lib.dp(grad)))),
                L.ibo_ehvi_direct_max(*(ld + (3, lib.dp(lb), lib.dp(ub), erf_mode, 1e-8, 3, 5, 100, 1, ctypes.byref(opt), None, None)))]

    Fc = lib.f64(F); rc_ = lib.f64(ref)
    h = [GP._handle() for GP in GPs]
    pair = lambda a, b: (ctypes.c_void_p * 2)(a, b)
    ok = pair(h[0], h[1])
    assert all_four(ok, len(Fc), lib.dp(Fc), lib.dp(rc_)) == [0] * 4
    assert all_four(pair(h[0], h[0]), len(Fc), lib.dp(Fc), lib.dp(rc_)) == [0] * 4            # the same handle twice is allowed
    ARG, STATE = lib.ERR_ARG, lib.ERR_STATE
    assert all_four(None, len(Fc), lib.dp(Fc), lib.dp(rc_)) == [ARG] * 4
    assert all_four(pair(h[0], None), len(Fc), lib.dp(Fc), lib.dp(rc_)) == [ARG] * 4
    assert all_four(pair(None, h[1]), len(Fc), lib.dp(Fc), lib.dp(rc_)) == [ARG] * 4
    assert all_four(ok, -1, lib.dp(Fc), lib.dp(rc_)) == [ARG] * 4
    assert all_four(ok, len(Fc), None, lib.dp(rc_)) == [ARG] * 4
    assert all_four(ok, len(Fc), lib.dp(Fc), None) == [ARG] * 4
    assert all_four(ok, len(Fc), lib.dp(Fc), lib.dp(rc_), erf_mode=5) == [ARG] * 4
    for bad in ([NAN, 0.], [0., float("inf")], [-float("inf"), 0.]):
        assert all_four(ok, len(Fc), lib.dp(Fc), lib.dp(lib.f64(bad))) == [ARG] * 4
    for v in (NAN, float("inf"), -float("inf")):
        Fb = Fc.copy(); Fb[len(Fb) // 2, 1] = v
        assert all_four(ok, len(Fb), lib.dp(Fb), lib.dp(rc_)) == [ARG] * 4
    # 1025 points left after canonicalisation; 1024 and a lot of clutter pass
    F1025 = lib.f64(er.curve_front(1025, ref, g["top"]))
    assert len(er.canonical(F1025, ref)[0]) == 1025
    assert all_four(ok, len(F1025), lib.dp(F1025), lib.dp(rc_)) == [ARG] * 4
    F1024 = lib.f64(er.curve_front(1024, ref, g["top"]))
    assert len(F1024) > 2048 and all_four(ok, len(F1024), lib.dp(F1024), lib.dp(rc_)) == [0] * 4
    # an unfitted handle: state; a model of another dimension: argument
    assert all_four(pair(h[0], fresh.h), len(Fc), lib.dp(Fc), lib.dp(rc_)) == [STATE] * 4
    assert all_four(pair(fresh.h, h[1]), len(Fc), lib.dp(Fc), lib.dp(rc_)) == [STATE] * 4
    assert all_four(pair(h[0], c1["GPs"][0]._handle()), len(Fc), lib.dp(Fc), lib.dp(rc_)) == [ARG] * 4
    # every output NULL, M < 1, NULL points, bounds of another dimension
    ld = (ok, len(Fc), lib.dp(Fc), lib.dp(rc_))
    assert L.ibo_ehvi_sweep(*(ld + (4, dc.ptr, 0, 1e-8, 0, None, .5, 0, None, None, None))) == ARG
    assert L.ibo_ehvi_batch(*(ld + (4, lib.dp(Qc), 0, 1e-8, None))) == ARG
    assert L.ibo_ehvi_grad_batch(*(ld + (4, lib.dp(Qc), 0, 1e-8, None, None))) == ARG
    assert L.ibo_ehvi_direct_max(*(ld + (3, lib.dp(lb), lib.dp(ub), 0, 1e-8, 3, 5, 100, 1, None, None, None))) == ARG
    assert L.ibo_ehvi_sweep(*(ld + (0, dc.ptr, 0, 1e-8, 0, None, .5, 0, None, ctypes.byref(bv), ctypes.byref(bi)))) == ARG
    assert L.ibo_ehvi_batch(*(ld + (4, None, 0, 1e-8, lib.dp(out)))) == ARG
    assert L.ibo_ehvi_sweep(*(ld + (4, None, 0, 1e-8, 0, None, .5, 0, None, ctypes.byref(bv), ctypes.byref(bi)))) == ARG
    assert L.ibo_ehvi_direct_max(*(ld + (2, lib.dp(lb), lib.dp(ub), 0, 1e-8, 3, 5, 100, 1, ctypes.byref(opt), None, None))) == ARG
    assert L.ibo_ehvi_direct_max(*(ld + (3, None, lib.dp(ub), 0, 1e-8, 3, 5, 100, 1, ctypes.byref(opt), None, None))) == ARG
    assert L.ibo_ehvi_sweep(*(ld + (4, dc.ptr, 0, 1e-8, 2, None, .5, 0, None, ctypes.byref(bv), ctypes.byref(bi)))) == ARG    # exclusions without centres
    fresh.close()


# ------------------------------------------------------------------------------------------------ the Python layer
def test_python_wrappers_agree_with_the_abi(lib, cases):
    from ibo_amd.acquisition import multiobjective as mo
    from ibo_amd.acquisition.constrained import _kstar_native
    c = cases["d3"]
    g = c["g"]
    GPs, ref = c["GPs"], g["ref"]
    F = er.gen_front("d3", 7)
    Q = g["Q"]
    for native in (True, False):
        r = mo.sweepEHVI(GPs, c["dc"], ref, front=F, native=native, outputs=("val",))
        with _kstar_native(GPs, native):
            rc, val, bv, bi = raw_sweep(lib, GPs, F, ref, c["dc"], 0 if native else 1, 1e-8 if native else 1e-7)
        assert rc == 0 and np.array_equal(r["val"], val) and (r["best_val"], r["best_idx"]) == (bv, bi)
    # a host array, exclusions and index_base go through
    w = bi
    r = mo.sweepEHVI(GPs, Q, ref, front=F, native=False, exclude=Q[w:w + 1], exclude_radius=1e-3, index_base=100)
    assert r["best_idx"] == 100 + cr.argmax(val, exclude=Q[w:w + 1], Q=Q, radius=1e-3)[0] and "val" not in r
    with pytest.raises(ValueError):
        mo.sweepEHVI(GPs, Q, ref, front=F, outputs=("mu",))
    with pytest.raises(ValueError, match="front="):
        mo.sweepEHVI(GPs, Q, ref)                    # observed at different points: no joint observations
    with pytest.raises(ValueError):
        mo.sweepEHVI(GPs[:1], Q, ref, front=F)
    # the class: Python conventions (NR erf, clamp 1e-7, the kernels' own k* variance)
    o = mo.ExpectedHypervolumeImprovement(GPs, ref, front=F)
    assert np.array_equal(np.c_[er.canonical(o.front, ref)], np.c_[er.canonical(F, ref)]) and len(o.front) >= 7
    rc, bval, bgrad = raw_batch(lib, GPs, F, ref, Q[:40], 1, 1e-7, grad=True)
    assert rc == 0
    v, gg = o.gradient(Q[:40])
    assert np.array_equal(o.values(Q[:40]), bval) and np.array_equal(v, bval) and np.array_equal(gg, bgrad)
    assert o.f(Q[3]) == bval[3] and o.negf(Q[3]) == -bval[3]
    nv, ng = o.negf_grad(Q[3])
    assert nv == -bval[3] and np.array_equal(ng, -bgrad[3])
    # one model as both objectives: the front defaults to the observed one
    both = [GPs[1], GPs[1]]
    of = mo.observedFront(both)
    assert len(of) == 1 and of[0, 0] == of[0, 1] == np.max(GPs[1].Y)
    lo = float(np.min(GPs[1].Y)) - .1
    r = mo.sweepEHVI(both, c["dc"], [lo, lo], native=False, outputs=("val",))
    rc, val = raw_batch(lib, both, of, [lo, lo], Q, 1, 1e-7)
    assert rc == 0 and np.array_equal(r["val"], val)
    assert mo.hypervolume(of, [lo, lo]) == (of[0, 0] - lo) ** 2


@pytest.mark.parametrize("name", CASES)
def test_maximizer_and_polish(lib, cases, name):
    from ibo_amd.acquisition import multiobjective as mo
    from ibo_amd.acquisition.constrained import _kstar_native
    c = cases[name]
    g = c["g"]
    GPs, ref = c["GPs"], g["ref"]
    F = er.gen_front(name, 7)
    bounds = [[0., 1.]] * g["D"]
    v0, x0 = mo.maximizeEHVI(GPs, bounds, ref, front=F, maxiter=8)
    v1, x1 = mo.maximizeEHVI(GPs, bounds, ref, front=F, maxiter=8, polish=True)
    assert v1 >= v0 > 0 and np.all(x1 >= 0) and np.all(x1 <= 1)
    with _kstar_native(GPs):
        rc, opt, optx, ns = raw_direct(lib, GPs, F, ref, g["D"], maxiter=8)
        assert rc == 0 and (opt, list(optx)) == (v0, list(x0))
        for v, x in ((v0, x0), (v1, x1)):
            rcb, b = raw_batch(lib, GPs, F, ref, x)
            assert rcb == 0 and b[0] == v
    # the value at the returned points, from the restatement with libego's k* variance
    models = [cr.Model(m.ref, sf2k=GP.kernel._ibo_spec()[3]) for m, GP in zip(g["models"], GPs)]
    for v, x in ((v0, x0), (v1, x1)):
        assert_end_to_end(np.array([v]), er.value(models, x, F, ref, gr.ERF_LIBM, 1e-8), "maximizeEHVI %s" % name)

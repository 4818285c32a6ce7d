"""
ibo_kg_sweep / ibo_kg_batch / ibo_kg_direct_max and what is built on them: acquisition.knowledge (KnowledgeGradient, sweepKG,
maximizeKG, referenceSet).

The yardstick is tests/kg_reference.py, the knowledge gradient restated in NumPy/SciPy float64 with another algorithm for the
expected maximum (sorted upper envelope; the device scans pairs) and pinned by tests/test_kg_reference.py.  Bars:
    mu, s2     the posterior's: 1e-6 relative (+ 1e-9 absolute for mu)
    b          [1e-10 (sf2 + noise + |v_a| |v_x|) + 1e-6 |b|] / sigma_x -- Sigma's bar carried through the division
    KG         2 max_i tol_mu_i + 0.8 max_a tol_b_a + 1e-12 scale -- the Lipschitz bound of E max in (mu, b), E|Z| ~ 0.8
    KG against the envelope evaluated on the call's own mu_ref, mu, s2, b: 1e-12 scale (scale = sum |terms| + max |b|)
The fantasy test ties b to the device's own extension path (addData on a copy), which is independent code.
"""
import ctypes
import functools
import types
from copy import deepcopy

import numpy as np
import pytest

import kg_reference as kr
import test_gpu_posterior_cov as pc

pytestmark = pytest.mark.gpu

NOISE = .1
GUARD = 7.25


@pytest.fixture(scope="module")
def lib():
    from ibo_amd import _lib
    if _lib.device_count() < 1:
        pytest.fail("no GPU visible: the product has no CPU fallback")
    return _lib


def kg_call(lib, h, A, Q, with_self=1, clamp=kr.CLAMP_PY, slopes=True):
    """ibo_kg_batch with guard words behind every output -> dict(kg, [mu_ref, mu, s2, b])"""
    A = lib.f64(np.atleast_2d(A)); Q = lib.f64(np.atleast_2d(Q))
    n, M, pad = len(A), len(Q), 8
    out = {"kg": np.full(M + pad, GUARD)}
    if slopes:
        out.update(mu_ref=np.full(n + pad, GUARD), mu=np.full(M + pad, GUARD), s2=np.full(M + pad, GUARD), b=np.full(M * n + pad, GUARD))
    ptr = lambda k: lib.dp(out[k]) if k in out else None
    lib.check(lib.lib.ibo_kg_batch(h, n, lib.dp(A), M, lib.dp(Q), int(with_self), clamp, ptr("kg"), ptr("mu_ref"), ptr("mu"), ptr("s2"),
                                   ptr("b")))
    size = dict(kg=M, mu_ref=n, mu=M, s2=M, b=M * n)
    for k, v in out.items():
        assert np.all(v[size[k]:] == GUARD), "guard behind %s overwritten" % k
        out[k] = v[:size[k]]
    if slopes:
        out["b"] = out["b"].reshape(M, n)
    return out


def gp_of(kind, D, N, prior, seed=1):
    from ibo_amd.gaussianprocess import GaussianProcess
    X, Y, hyper, p, ref = kr.case_ref(kind, D, N, prior, seed=seed, noise=NOISE)
    return GaussianProcess(pc.make_kernel(kind, hyper), X, Y, prior=p, noise=NOISE), ref


@functools.lru_cache(maxsize=None)
def case_data(case):
    """one case: the library's outputs and the restatement's, computed once for the three tests that read them"""
    from ibo_amd import _lib
    kind, D, N, n, M, prior, ws = case
    GP, ref = gp_of(kind, D, N, prior)
    A = kr.ref_points(GP.X, n); Q = pc.queries(GP.X, M)
    GP._push_prior()
    got = kg_call(_lib, GP._handle(), A, Q, ws)
    want = kr.kg(ref, A, Q, bool(ws))
    return got, want, types.SimpleNamespace(sf2=ref.sf2, noise=ref.noise)     # (not the RefGP: its N x N matrices would stay cached)


def close(got, want, tol, what):
    err = np.abs(np.asarray(got) - want)
    print("%s: worst error / bar = %.3g" % (what, float(np.max(err / tol))))
    assert np.all(err <= tol), "%s: worst %g of its bar" % (what, float(np.max(err / tol)))


@pytest.mark.parametrize("case", kr.CASES)
def test_slopes_against_the_restatement(lib, case):
    got, want, ref = case_data(case)
    close(got["mu_ref"], want["mu_ref"], kr.tol_mu(want["mu_ref"]), "mu_ref %s" % (case,))
    close(got["mu"], want["mu"], kr.tol_mu(want["mu"]), "mu %s" % (case,))
    close(got["s2"], want["s2"], 1e-6 * want["s2"], "s2 %s" % (case,))
    close(got["b"], want["b"], kr.tol_b(want, ref.sf2, ref.noise), "b %s" % (case,))


@pytest.mark.parametrize("case", kr.CASES)
def test_kg_against_the_restatement(lib, case):
    got, want, ref = case_data(case)
    assert np.all(got["kg"] >= 0)
    close(got["kg"], want["kg"], kr.tol_kg(want, ref.sf2, ref.noise, case[-1]), "KG %s" % (case,))


def composition_close(got, with_self, what):
    kg, scale = kr.compose(got["mu_ref"], got["mu"], got["s2"], got["b"], NOISE, bool(with_self))
    assert np.all(got["kg"] >= 0) and np.all(np.isfinite(got["kg"]))
    err = np.abs(got["kg"] - kg)
    print("%s: worst |KG - composition| / scale = %.3g (largest KG %.3g)" % (what, float(np.max(err / np.maximum(scale, 1e-300))), float(np.max(kg))))
    assert np.all(err <= 1e-12 * scale), what


@pytest.mark.parametrize("case", kr.CASES)
def test_kg_against_the_composition_of_its_own_slopes(lib, case):
    got, _, _ = case_data(case)
    composition_close(got, case[-1], "composition %s" % (case,))


def test_degenerate_sets_against_the_composition(lib):
    from ibo_amd.gaussianprocess import GaussianProcess
    GP, _ = gp_of("ard", 3, 65, False)
    h = GP._handle()
    A = kr.ref_points(GP.X, 40); Q = pc.queries(GP.X, 70, seed=4)
    for ws in (1, 0):
        once = kg_call(lib, h, A, Q, ws)
        twice = kg_call(lib, h, np.r_[A, A], Q, ws)                  # equal lines: the index tie rule
        composition_close(twice, ws, "reference set listed twice, with_self=%d" % ws)
        np.testing.assert_allclose(twice["kg"], once["kg"], rtol=0, atol=1e-12 * (1 + np.max(np.abs(once["b"]))))
        composition_close(kg_call(lib, h, np.repeat(A[3:4], 65, axis=0), Q, ws), ws, "one point 65 times, with_self=%d" % ws)
        far = 40.0 + pc.queries(GP.X, 66, seed=6)                    # every reference slope ~ 0
        g = kg_call(lib, h, A, far, ws)
        composition_close(g, ws, "far candidates, with_self=%d" % ws)
        if not ws:
            assert np.max(np.abs(g["b"])) < 1e-100 and np.all(g["kg"] == 0)
    composition_close(kg_call(lib, h, A, np.r_[A[:9], Q[:5]], 1), 1, "candidates equal to reference points")
    Xc, _ = pc.synth(3, 50, 3)
    GPc = GaussianProcess(pc.make_kernel("m5", pc.hyper_of("m5", 3)), Xc, np.full(50, .3), noise=NOISE)
    for ws in (1, 0):
        composition_close(kg_call(lib, GPc._handle(), Xc[:33], pc.queries(Xc, 40), ws), ws, "constant Y, with_self=%d" % ws)


def test_bit_invariance_and_argmax(lib):
    from ibo_amd import DeviceArray
    GP, _ = gp_of("m5", 3, 65, True)
    h = GP._handle()
    GP._push_prior()
    A = kr.ref_points(GP.X, 64); Q = pc.queries(GP.X, 300, seed=9)
    one = kg_call(lib, h, A, Q, 1)
    for lo, hi in ((0, 1), (5, 12), (10, 74), (100, 165), (299, 300)):
        part = kg_call(lib, h, A, Q[lo:hi], 1)
        for k in ("kg", "mu", "s2", "b"):
            assert np.array_equal(part[k], one[k][lo:hi]), (k, lo, hi)
    filler = pc.queries(GP.X, 1000, seed=10)
    big = filler.copy()
    big[100:400] = Q; big[611:911] = Q                              # chunks of 256: both copies cross chunk boundaries
    dc = DeviceArray.from_host(big, GP._dev.device)
    out = DeviceArray((1000,), GP._dev.device)
    bv = ctypes.c_double(); bi = ctypes.c_int64()
    Af = lib.f64(A)
    lib.check(lib.lib.ibo_set_option(b"kg_chunk", 256))
    try:
        lib.check(lib.lib.ibo_kg_sweep(h, 64, lib.dp(Af), 1000, dc.ptr, 1, kr.CLAMP_PY, 5000, out.ptr, ctypes.byref(bv), ctypes.byref(bi)))
        chunked = kg_call(lib, h, A, Q, 1)
    finally:
        lib.check(lib.lib.ibo_set_option(b"kg_chunk", 0))
    v = out.to_host()
    assert np.array_equal(v[100:400], one["kg"]) and np.array_equal(v[611:911], one["kg"])
    for k in ("kg", "mu", "s2", "b"):
        assert np.array_equal(chunked[k], one[k]), k
    assert bv.value == np.max(v) and bi.value == 5000 + int(np.argmax(v))
    # whole-array sweep without the option (one chunk) and without the per-candidate output
    b2 = ctypes.c_double(); i2 = ctypes.c_int64()
    lib.check(lib.lib.ibo_kg_sweep(h, 64, lib.dp(Af), 1000, dc.ptr, 1, kr.CLAMP_PY, 0, None, ctypes.byref(b2), ctypes.byref(i2)))
    assert b2.value == bv.value and i2.value == int(np.argmax(v))
    # a duplicated best candidate reports the first
    k = int(np.argmax(one["kg"]))
    dup = DeviceArray.from_host(np.r_[Q[:20], Q[k:k + 1], Q, Q[k:k + 1]], GP._dev.device)
    lib.check(lib.lib.ibo_kg_sweep(h, 64, lib.dp(Af), 322, dup.ptr, 1, kr.CLAMP_PY, 7, None, ctypes.byref(b2), ctypes.byref(i2)))
    assert b2.value == one["kg"][k] and i2.value == 7 + (k if k < 20 else 20)


def stage_ms(lib, entry, reset):
    """the six per-stage sums of ibo_kg_stage_ms / ibo_qei_stage_ms"""
    ms = np.full(6 + 2, GUARD)
    lib.check(getattr(lib.lib, entry)(lib.dp(ms), reset))
    assert np.all(ms[6:] == GUARD)
    return ms[:6]


def test_timing_leaves_the_values_alone_and_fills_its_own_sums(lib):
    """kg_timing over three chunks (256 + 256 + 88): the same bits from the sweep and the host batch, six sums, their reset, none of qEI's"""
    from ibo_amd import DeviceArray
    GP, _ = gp_of("m5", 3, 65, True)
    h = GP._handle()
    GP._push_prior()
    A = kr.ref_points(GP.X, 64); C = pc.queries(GP.X, 600, seed=11)
    Af = lib.f64(A)
    dc = DeviceArray.from_host(C, GP._dev.device)

    def sweep():
        out = DeviceArray((600,), GP._dev.device)
        bv = ctypes.c_double(); bi = ctypes.c_int64()
        lib.check(lib.lib.ibo_kg_sweep(h, 64, lib.dp(Af), 600, dc.ptr, 1, kr.CLAMP_PY, 3, out.ptr, ctypes.byref(bv), ctypes.byref(bi)))
        return out.to_host(), bv.value, bi.value

    def sums_of_a_timed_call():
        ms = stage_ms(lib, "ibo_kg_stage_ms", 1)
        print("kg stage sums (ms):", ms)
        assert np.all(np.isfinite(ms)) and np.all(ms >= 0)
        assert np.all(ms > 0)                                       # every stage launches a kernel: there is a reference set
        assert np.all(stage_ms(lib, "ibo_kg_stage_ms", 0) == 0)     # the read above reset them
        assert np.all(stage_ms(lib, "ibo_qei_stage_ms", 0) == 0)    # and nothing went to the other unit's

    lib.check(lib.lib.ibo_set_option(b"kg_chunk", 256))
    try:
        lib.check(lib.lib.ibo_kg_stage_ms(None, 1)); lib.check(lib.lib.ibo_qei_stage_ms(None, 1))
        lib.check(lib.lib.ibo_kg_stage_ms(None, 0))
        v0, b0, i0 = sweep()
        host0 = kg_call(lib, h, A, C, 1)
        assert np.all(stage_ms(lib, "ibo_kg_stage_ms", 0) == 0)     # timing off: nothing is added
        lib.check(lib.lib.ibo_set_option(b"kg_timing", 1))
        v1, b1, i1 = sweep()
        sums_of_a_timed_call()
        host1 = kg_call(lib, h, A, C, 1)
        sums_of_a_timed_call()
    finally:
        lib.check(lib.lib.ibo_set_option(b"kg_timing", 0))
        lib.check(lib.lib.ibo_set_option(b"kg_chunk", 0))
        lib.check(lib.lib.ibo_kg_stage_ms(None, 1))
    assert np.array_equal(v1, v0) and b1 == b0 and i1 == i0 and i0 == 3 + int(np.argmax(v0))
    for k in ("kg", "mu_ref", "mu", "s2", "b"):
        assert np.array_equal(host1[k], host0[k]), k
    assert np.array_equal(host0["kg"], v0)


def test_many_candidates_on_a_small_model(lib):
    """N = 10 rows: the chunk is bounded by the launch grid (65280 candidates), not by bytes; 70000 candidates cross that bound"""
    from ibo_amd import DeviceArray
    GP, _ = gp_of("iso", 2, 10, False)
    h = GP._handle()
    A = lib.f64(kr.ref_points(GP.X, 3))
    C = pc.queries(GP.X, 70000, seed=12)
    dc = DeviceArray.from_host(C, GP._dev.device); out = DeviceArray((70000,), GP._dev.device)
    bv = ctypes.c_double(); bi = ctypes.c_int64()
    lib.check(lib.lib.ibo_kg_sweep(h, 3, lib.dp(A), 70000, dc.ptr, 1, kr.CLAMP_PY, 0, out.ptr, ctypes.byref(bv), ctypes.byref(bi)))
    v = out.to_host()
    assert np.all(np.isfinite(v)) and np.all(v >= 0) and bv.value == np.max(v) and bi.value == int(np.argmax(v))
    idx = np.r_[0:5, 65270:65290, 69995:70000]
    assert np.array_equal(v[idx], kg_call(lib, h, A, C[idx], 1, slopes=False)["kg"])
    assert np.array_equal(v, kg_call(lib, h, A, C, 1, slopes=False)["kg"])


@pytest.mark.parametrize("kind", ["ard", "m5"])
def test_fantasy_through_the_extension_path(lib, kind):
    GP, _ = gp_of(kind, 4, 200, False)
    A = kr.ref_points(GP.X, 50); Q = pc.queries(GP.X, 6, seed=8)
    g = kg_call(lib, GP._handle(), A, Q, 1)
    np.testing.assert_allclose(g["mu_ref"], GP.posteriors(A)[0], rtol=1e-6, atol=1e-9)
    for j in (0, 5):
        for z in (-1.5, .7):
            G2 = deepcopy(GP)
            G2.addData(Q[j:j + 1], np.array([g["mu"][j] + np.sqrt(g["s2"][j]) * z]))
            mu2, _ = G2.posteriors(A)
            want = g["mu_ref"] + g["b"][j] * z
            assert np.all(np.abs(mu2 - want) <= 1e-6 * np.abs(want) + 1e-9), float(np.max(np.abs(mu2 - want)))
            assert np.max(np.abs(g["b"][j])) > 1e-3


@pytest.mark.parametrize("D", [2, 4])
def test_direct_equals_the_host_tree_on_single_points(lib, D):
    from ibo_amd.acquisition import KnowledgeGradient, maximizeKG
    GP, _ = gp_of("ard", D, 40, False)
    h = GP._handle()
    A = lib.f64(kr.ref_points(GP.X, 32))
    lb, ub = lib.f64(np.zeros(D)), lib.f64(np.ones(D))
    opt = ctypes.c_double(); optx = np.empty(D); ns = ctypes.c_int64()
    lib.check(lib.lib.ibo_kg_direct_max(h, 32, lib.dp(A), D, lib.dp(lb), lib.dp(ub), 1, kr.CLAMP_PY, 12, 30, 10000, 1,
                                        ctypes.byref(opt), lib.dp(optx), ctypes.byref(ns)))
    val = np.empty(1)

    def negval(nd, x):
        q = lib.f64([x[i] for i in range(nd)])
        assert lib.lib.ibo_kg_batch(h, 32, lib.dp(A), 1, lib.dp(q), 1, kr.CLAMP_PY, lib.dp(val), None, None, None, None) == 0
        return -val[0]
    cb = lib.OBJECTIVE(negval)
    fm = ctypes.c_double(); xm = np.empty(D); n2 = ctypes.c_int64()
    lib.check(lib.lib.ibo_direct_host(cb, D, lib.dp(lb), lib.dp(ub), 12, 30, 10000, 1, ctypes.byref(fm), lib.dp(xm), ctypes.byref(n2)))
    assert ns.value == n2.value and ns.value > 50
    assert np.array_equal(optx, xm) and opt.value == -fm.value and opt.value > 0
    o, ox = maximizeKG(GP, [[0., 1.]] * D, ref_points=A, maxiter=12, compat=True)
    assert o == opt.value and np.array_equal(ox, optx)
    assert KnowledgeGradient(GP, A).f(ox) == o


def test_errors_leave_the_handle_usable(lib):
    GP, _ = gp_of("ard", 3, 50, False)
    h = GP._handle()
    dp = lib.dp
    A = lib.f64(kr.ref_points(GP.X, 5)); Q = lib.f64(pc.queries(GP.X, 4)); kg = np.empty(4)
    lb, ub = lib.f64(np.zeros(3)), lib.f64(np.ones(3))
    from ibo_amd import DeviceArray
    dc = DeviceArray.from_host(Q, GP._dev.device)
    bv = ctypes.c_double(); bi = ctypes.c_int64(); ns = ctypes.c_int64(); ox = np.empty(3)
    big = lib.f64(np.zeros((1025, 3)))
    bad = A.copy(); bad[2, 1] = np.inf
    nan = A.copy(); nan[4, 2] = np.nan
    batch = lambda g, n, a, M, q, out: lib.lib.ibo_kg_batch(g, n, a, M, q, 1, 1e-7, out, None, None, None, None)
    sweep = lambda g, n, a, M, c, v, i: lib.lib.ibo_kg_sweep(g, n, a, M, c, 1, 1e-7, 0, None, v, i)
    direct = lambda g, n, a, D, l, u, o: lib.lib.ibo_kg_direct_max(g, n, a, D, l, u, 1, 1e-7, 5, 5, 200, 1, o, dp(ox), ctypes.byref(ns))
    want = kg_call(lib, h, A, Q, 1, slopes=False)["kg"]
    for rc in (batch(None, 5, dp(A), 4, dp(Q), dp(kg)), batch(h, 5, None, 4, dp(Q), dp(kg)), batch(h, 5, dp(A), 4, None, dp(kg)),
               batch(h, 5, dp(A), 4, dp(Q), None), batch(h, 0, dp(A), 4, dp(Q), dp(kg)), batch(h, 1025, dp(big), 4, dp(Q), dp(kg)),
               batch(h, 5, dp(A), 0, dp(Q), dp(kg)), batch(h, 5, dp(bad), 4, dp(Q), dp(kg)), batch(h, 5, dp(nan), 4, dp(Q), dp(kg)),
               sweep(None, 5, dp(A), 4, dc.ptr, ctypes.byref(bv), ctypes.byref(bi)), sweep(h, 5, None, 4, dc.ptr, ctypes.byref(bv), ctypes.byref(bi)),
               sweep(h, 5, dp(A), 4, None, ctypes.byref(bv), ctypes.byref(bi)), sweep(h, 5, dp(A), 4, dc.ptr, None, None),
               sweep(h, 1025, dp(big), 4, dc.ptr, ctypes.byref(bv), ctypes.byref(bi)), sweep(h, 5, dp(A), 0, dc.ptr, ctypes.byref(bv), ctypes.byref(bi)),
               sweep(h, 5, dp(bad), 4, dc.ptr, ctypes.byref(bv), ctypes.byref(bi)),
               sweep(h, 0, dp(A), 4, dc.ptr, ctypes.byref(bv), ctypes.byref(bi)), sweep(h, 5, dp(nan), 4, dc.ptr, ctypes.byref(bv), ctypes.byref(bi)),
               direct(h, 1025, dp(big), 3, dp(lb), dp(ub), ctypes.byref(bv)), direct(h, 5, dp(nan), 3, dp(lb), dp(ub), ctypes.byref(bv)),
               lib.lib.ibo_kg_direct_max(h, 5, dp(A), 3, dp(lb), dp(ub), 1, 1e-7, 5, 5, 200, 1, None, None, None),
               lib.lib.ibo_kg_batch(h, 5, dp(A), -3, dp(Q), 1, 1e-7, dp(kg), None, None, None, None),
               direct(None, 5, dp(A), 3, dp(lb), dp(ub), ctypes.byref(bv)), direct(h, 5, None, 3, dp(lb), dp(ub), ctypes.byref(bv)),
               direct(h, 5, dp(A), 3, None, dp(ub), ctypes.byref(bv)), direct(h, 5, dp(A), 3, dp(lb), None, ctypes.byref(bv)),
               direct(h, 0, dp(A), 3, dp(lb), dp(ub), ctypes.byref(bv)), direct(h, 5, dp(bad), 3, dp(lb), dp(ub), ctypes.byref(bv)),
               direct(h, 5, dp(A), 2, dp(lb), dp(ub), ctypes.byref(bv)), direct(h, 5, dp(A), 4, dp(lb), dp(ub), ctypes.byref(bv))):
        assert rc == lib.ERR_ARG
        assert np.array_equal(kg_call(lib, h, A, Q, 1, slopes=False)["kg"], want)        # the handle is still usable and correct
    assert batch(h, 1025, dp(big), 4, dp(Q), dp(kg)) == lib.ERR_ARG and b"1024" in lib.lib.ibo_last_error()
    hp = ctypes.c_void_p()
    lib.check(lib.lib.ibo_gp_create(0, ctypes.byref(hp)))
    try:
        assert batch(hp, 5, dp(A), 4, dp(Q), dp(kg)) == lib.ERR_STATE
        assert sweep(hp, 5, dp(A), 4, dc.ptr, ctypes.byref(bv), ctypes.byref(bi)) == lib.ERR_STATE
        assert direct(hp, 5, dp(A), 3, dp(lb), dp(ub), ctypes.byref(bv)) == lib.ERR_STATE
    finally:
        lib.lib.ibo_gp_destroy(hp)
    assert sweep(h, 5, dp(A), 4, dc.ptr, ctypes.byref(bv), ctypes.byref(bi)) == lib.OK
    assert bv.value == np.max(want) and bi.value == int(np.argmax(want))


def test_python_layer(lib):
    from ibo_amd import DeviceArray
    from ibo_amd.acquisition import KnowledgeGradient, maximizeKG, referenceSet, sweepKG
    GP, ref = gp_of("sviso", 3, 30, True)
    bounds = [[0., 1.]] * 3
    A = referenceSet(GP, bounds, 48, seed=3)
    assert A.shape == (48, 3) and np.array_equal(A[:30], np.asarray(GP.X)[::-1])
    assert np.array_equal(A, referenceSet(GP, bounds, 48, seed=3)) and not np.array_equal(A, referenceSet(GP, bounds, 48, seed=4))
    assert np.all((A[30:] >= 0) & (A[30:] <= 1))
    assert np.array_equal(referenceSet(GP, bounds, 7), np.asarray(GP.X)[::-1][:7])
    Q = pc.queries(GP.X, 90, seed=5)
    acq = KnowledgeGradient(GP, A)
    v = acq.values(Q)
    raw = kg_call(lib, GP._handle(), A, Q, 1)
    assert np.array_equal(v, raw["kg"])
    mu_ref, mu, s2, b = acq.slopes(Q)
    assert np.array_equal(mu_ref, raw["mu_ref"]) and np.array_equal(mu, raw["mu"]) and np.array_equal(s2, raw["s2"]) and np.array_equal(b, raw["b"])
    assert acq.f(Q[7]) == v[7] and acq.negf(Q[7]) == -v[7]
    want = kr.kg(ref, A, Q, True)
    close(v, want["kg"], kr.tol_kg(want, ref.sf2, ref.noise, 1), "KnowledgeGradient.values")
    assert np.array_equal(KnowledgeGradient(GP, A, with_self=False).values(Q), kg_call(lib, GP._handle(), A, Q, 0, slopes=False)["kg"])
    bv, bi = sweepKG(GP, Q, A)
    assert bv == np.max(v) and bi == int(np.argmax(v))
    bv, bi, vals = sweepKG(GP, DeviceArray.from_host(Q, GP._dev.device), A, values=True, index_base=10)
    assert np.array_equal(vals, v) and bv == np.max(v) and bi == 10 + int(np.argmax(v))
    opt, optx = maximizeKG(GP, bounds, n_ref=40, seed=2, maxiter=8)
    assert opt > 0 and optx.shape == (3,) and np.all((optx >= 0) & (optx <= 1))
    assert opt == KnowledgeGradient(GP, referenceSet(GP, bounds, 40, seed=2)).f(optx)
    assert opt >= np.max(KnowledgeGradient(GP, referenceSet(GP, bounds, 40, seed=2)).values(np.full((1, 3), .5)))
    with pytest.raises(ValueError):
        KnowledgeGradient(GP, np.zeros((1025, 3)))
    # points of another width than the model's are refused before anything reads past them
    for call in (lambda: KnowledgeGradient(GP, A[:, :2]), lambda: acq.values(Q[:, :2]), lambda: acq.f(Q[0, :2]), lambda: sweepKG(GP, Q[:, :2], A),
                 lambda: sweepKG(GP, DeviceArray.from_host(np.c_[Q, Q[:, :1]], GP._dev.device), A), lambda: maximizeKG(GP, bounds[:2], ref_points=A),
                 lambda: referenceSet(GP, bounds, 0)):
        with pytest.raises(ValueError):
            call()
    assert np.array_equal(acq.values(Q), v)


def test_nan_candidate_stays_nan_and_never_wins(lib):
    from ibo_amd import DeviceArray
    GP, _ = gp_of("m3", 3, 65, False)
    h = GP._handle()
    A = lib.f64(kr.ref_points(GP.X, 20)); Q = pc.queries(GP.X, 70, seed=3)
    clean = kg_call(lib, h, A, Q, 1, slopes=False)["kg"]
    Qn = Q.copy(); Qn[0, 1] = np.nan; Qn[66, 0] = np.nan
    for ws in (1, 0):
        want = kg_call(lib, h, A, Q, ws, slopes=False)["kg"]
        got = kg_call(lib, h, A, Qn, ws, slopes=False)["kg"]
        assert np.isnan(got[0]) and np.isnan(got[66])
        keep = np.r_[1:66, 67:70]
        assert np.array_equal(got[keep], want[keep])
        bv = ctypes.c_double(); bi = ctypes.c_int64()
        dc = DeviceArray.from_host(Qn, GP._dev.device)
        lib.check(lib.lib.ibo_kg_sweep(h, 20, lib.dp(A), 70, dc.ptr, ws, kr.CLAMP_PY, 0, None, ctypes.byref(bv), ctypes.byref(bi)))
        assert bv.value == np.max(want[keep]) and bi.value == int(keep[np.argmax(want[keep])])
    assert np.all(np.isfinite(clean))
    # nothing but NaN: no index
    dn = DeviceArray.from_host(np.full((3, 3), np.nan), GP._dev.device)
    lib.check(lib.lib.ibo_kg_sweep(h, 20, lib.dp(A), 3, dn.ptr, 1, kr.CLAMP_PY, 0, None, ctypes.byref(bv), ctypes.byref(bi)))
    assert bi.value == -1


def test_augmented_preference_model_is_refused_and_the_plain_one_works(lib):
    from ibo_amd.acquisition import KnowledgeGradient
    from ibo_amd.gaussianprocess import PrefGaussianProcess
    from ibo_amd.gaussianprocess.kernel import GaussianKernel_ard
    rs = np.random.RandomState(3)
    GP = PrefGaussianProcess(GaussianKernel_ard(np.array([.6] * 4)))
    P = rs.rand(40, 4)
    GP.addPreferences([(P[2 * i], P[2 * i + 1], 0) for i in range(20)])
    A = rs.rand(16, 4); Q = rs.rand(30, 4)
    acq = KnowledgeGradient(GP, A)
    g = dict(zip(("mu_ref", "mu", "s2", "b"), acq.slopes(Q)))
    g["kg"] = acq.values(Q)
    kg, scale = kr.compose(g["mu_ref"], g["mu"], g["s2"], g["b"], GP.noise, True)
    assert np.all(np.abs(g["kg"] - kg) <= 1e-12 * scale) and np.max(g["kg"]) > 0
    np.testing.assert_allclose(g["mu_ref"], GP.posteriors(A)[0], rtol=1e-6, atol=1e-9)
    np.testing.assert_allclose(g["s2"], GP.posteriors(Q)[1], rtol=1e-6)
    GP.addObservationPoint(rs.rand(4))
    with pytest.raises(ValueError):
        acq.values(Q)
    with pytest.raises(ValueError):
        KnowledgeGradient(GP, A)

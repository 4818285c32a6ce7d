"""
ibo_qei_sweep / ibo_qei_batch / ibo_qei_direct_max and what is built on them: acquisition.batch (baseSamples, ParallelEI, sweepQEI,
maximizeQEI, jointQEI, proposeBatch).

The yardstick is tests/qei_reference.py, the Monte-Carlo parallel expected improvement restated in NumPy float64 by another route (the
whole bordered matrix factored per candidate; the device borders a host factor of S_PP by forward substitution) and pinned by
tests/test_qei_reference.py.  Bars:
    mu_P, mu, s2   the posterior's: 1e-6 relative (+ 1e-9 absolute for the means)
    S_PP, c        Sigma's: 1e-10 (sf2 + noise + |v_a| |v_b|)
    qEI against `compose` on the call's own pieces: 1e-12 scale -- the test of the finish kernel
    qEI end to end: qei_reference.tol_qei, the pieces' bars carried through (derived in that module's docstring)
and exact statements: values >= base, the single-sample closed form, a threshold nothing reaches, one route (bit equality between
entries, chunkings and places), DIRECT against the host tree, the arg-max contract.
"""
import ctypes
import functools
import types
from fractions import Fraction

import numpy as np
import pytest

import kg_reference as kr
import qei_reference as qr
import test_gpu_posterior_cov as pc

pytestmark = pytest.mark.gpu

NOISE = .1
GUARD = 7.25
NAN = float("nan")


@pytest.fixture(scope="module")
def lib():
    from ibo_amd import _lib
    if _lib.device_count() < 1:
        pytest.fail("no GPU visible: the product has no CPU fallback")
    return _lib


def qei_call(lib, h, P, Z, Q, ymax=NAN, xi=qr.XI, clamp=qr.CLAMP_PY, jitter=0.0, pieces=True, expect=0):
    """ibo_qei_batch with guard words behind every output -> dict(qei, base, [mu_pend, S_pend, mu, s2, c])"""
    Q = lib.f64(np.atleast_2d(Q)); Z = lib.f64(np.atleast_2d(Z))
    D = Q.shape[1]
    P = lib.f64(np.asarray(P, dtype=float).reshape(-1, D))
    p, M, S, pad = len(P), len(Q), len(Z), 8
    assert Z.shape[1] == p + 1
    out = {"qei": np.full(M + pad, GUARD)}
    if pieces:
        out.update(mu_pend=np.full(p + pad, GUARD), S_pend=np.full(p * p + pad, GUARD), mu=np.full(M + pad, GUARD), s2=np.full(M + pad, GUARD),
                   c=np.full(M * p + pad, GUARD))
    ptr = lambda k: lib.dp(out[k]) if k in out else None
    base = ctypes.c_double(GUARD); info = ctypes.c_int(-7)
    rc = lib.lib.ibo_qei_batch(h, p, lib.dp(P) if p else None, S, lib.dp(Z), ymax, xi, clamp, jitter, M, lib.dp(Q), ptr("qei"), ctypes.byref(base),
                               ptr("mu_pend"), ptr("S_pend"), ptr("mu"), ptr("s2"), ptr("c"), ctypes.byref(info))
    assert rc == expect, (rc, lib.lib.ibo_last_error())
    size = dict(qei=M, mu_pend=p, S_pend=p * p, mu=M, s2=M, c=M * p)
    for k, v in out.items():
        assert np.all(v[size[k]:] == GUARD), "guard behind %s overwritten" % k
        out[k] = v[:size[k]]
    if pieces:
        out["S_pend"] = out["S_pend"].reshape(p, p); out["c"] = out["c"].reshape(M, p)
    out["base"] = base.value; out["info"] = info.value
    return out


def sweep_call(lib, h, P, Z, dc, M, index_base=0, values=True, ymax=NAN, xi=qr.XI, jitter=0.0):
    """ibo_qei_sweep over the device array dc -> (best_val, best_idx, values or None, base)"""
    from ibo_amd import DeviceArray
    Z = lib.f64(Z)
    P = lib.f64(np.asarray(P, dtype=float).reshape(-1, dc.shape[1]))
    out = DeviceArray((M,), dc.device) if values else None
    bv = ctypes.c_double(); bi = ctypes.c_int64(); base = ctypes.c_double(); info = ctypes.c_int()
    lib.check(lib.lib.ibo_qei_sweep(h, len(P), lib.dp(P) if len(P) else None, len(Z), lib.dp(Z), ymax, xi, qr.CLAMP_PY, jitter, M, dc.ptr,
                                    index_base, out.ptr if values else None, ctypes.byref(base), ctypes.byref(bv), ctypes.byref(bi),
                                    ctypes.byref(info)))
    return bv.value, bi.value, (out.to_host() if values else None), base.value


def gp_of(kind, D, N, prior, seed=1):
    from ibo_amd.gaussianprocess import GaussianProcess
    X, Y, hyper, p, ref = kr.case_ref(kind, D, N, prior, seed=seed, noise=NOISE)
    return GaussianProcess(pc.make_kernel(kind, hyper), X, Y, prior=p, noise=NOISE), ref


@functools.lru_cache(maxsize=None)
def case_data(case):
    """one case: the library's outputs and the restatement's, computed once for the tests that read them"""
    from ibo_amd import _lib
    from ibo_amd.gaussianprocess import GaussianProcess
    X, Y, hyper, pr, ref, P, Q, Z, t = qr.case_inputs(case)
    GP = GaussianProcess(pc.make_kernel(case[0], hyper), X, Y, prior=pr, noise=NOISE)
    GP._push_prior()
    got = qei_call(_lib, GP._handle(), P, Z, Q)
    want = qr.qei(ref, P, Q, Z, t)
    del want["Sigma"], want["terms"]
    return got, want, types.SimpleNamespace(sf2=ref.sf2, noise=ref.noise, Z=Z, t=t)


def close(got, want, tol, what):
    err = np.abs(np.asarray(got) - want)
    if err.size == 0:
        return
    print("%s: worst error / bar = %.3g" % (what, float(np.max(err / tol))))
    assert np.all(err <= tol), "%s: worst %g of its bar" % (what, float(np.max(err / tol)))


def compose_close(got, Z, t, what):
    v, scale = qr.compose(got["mu_pend"], got["S_pend"], got["mu"], got["s2"], got["c"], Z, t)
    assert np.all(np.isfinite(got["qei"])) and np.all(got["qei"] >= got["base"]) and got["base"] >= 0
    err = np.abs(got["qei"] - v)
    print("%s: worst |qEI - composition| / scale = %.3g (largest qEI %.3g, base %.3g)" %
          (what, float(np.max(err / scale)), float(np.max(v)), got["base"]))
    assert np.all(err <= 1e-12 * scale), what


@pytest.mark.parametrize("case", qr.CASES)
def test_pieces_against_the_restatement(lib, case):
    got, want, ref = case_data(case)
    assert got["info"] == 0
    close(got["mu_pend"], want["mu_pend"], qr.tol_mu(want["mu_pend"]), "mu_pend %s" % (case,))
    close(got["mu"], want["mu"], qr.tol_mu(want["mu"]), "mu %s" % (case,))
    close(got["s2"], want["s2"], 1e-6 * want["s2"], "s2 %s" % (case,))
    close(got["S_pend"], want["S_pend"], qr.tol_S(want, ref.sf2, ref.noise), "S_pend %s" % (case,))
    close(got["c"], want["c"], qr.tol_c(want, ref.sf2, ref.noise), "c %s" % (case,))
    assert np.array_equal(got["S_pend"], got["S_pend"].T)


@pytest.mark.parametrize("case", qr.CASES)
def test_value_against_the_composition_of_its_own_pieces(lib, case):
    got, _, ref = case_data(case)
    compose_close(got, ref.Z, ref.t, "composition %s" % (case,))


@pytest.mark.parametrize("case", qr.CASES)
def test_value_against_the_restatement(lib, case):
    got, want, ref = case_data(case)
    close(got["qei"], want["qei"], qr.tol_qei(want, ref.Z, ref.t, ref.sf2, ref.noise), "qEI %s" % (case,))
    close(got["base"], want["base"], np.max(qr.tol_qei(want, ref.Z, ref.t, ref.sf2, ref.noise)), "base %s" % (case,))
    assert np.all(got["qei"] >= got["base"])                      # exactly: one summation order (ibo_abi.h)
    if case[3] == 0:
        assert got["base"] == 0.0


def test_exact_small_cases(lib):
    GP, _ = gp_of("ard", 3, 65, False)
    h = GP._handle()
    Q = pc.queries(GP.X, 40, seed=4)
    t = float(np.max(GP.Y)) + qr.XI
    for z in (-1.3, 0.0, .4, 2.5):
        g = qei_call(lib, h, [], [[z]], Q)
        d = np.sqrt(g["s2"])
        # one sample, no pending point: f = fma(sigma, z, mu) (ibo_abi.h), formed exactly here and rounded once
        f = np.array([float(Fraction(m) + Fraction(s) * Fraction(z)) for m, s in zip(g["mu"], d)])
        want = np.maximum(f - t, 0.0)
        assert np.all(np.abs(g["qei"] - want) <= 1e-15 * np.abs(want)), float(np.max(np.abs(g["qei"] - want)))
        assert g["base"] == 0.0
    assert np.any(want > 0)
    # a threshold nothing reaches: every term is 0, and so is the value -- exactly
    P = qr.pending_points(GP.X, 3); Z = qr.samples(1000, 4)
    g = qei_call(lib, h, P, Z, Q, ymax=1e6)
    assert np.all(g["qei"] == 0.0) and g["base"] == 0.0
    # ymax given: the same as the default when it is max(Y)
    a = qei_call(lib, h, P, Z, Q, pieces=False); b = qei_call(lib, h, P, Z, Q, ymax=float(np.max(GP.Y)), pieces=False)
    assert np.array_equal(a["qei"], b["qei"]) and a["base"] == b["base"] and np.max(a["qei"]) > a["base"] >= 0


def test_one_route_bit_for_bit(lib):
    from ibo_amd import DeviceArray
    GP, _ = gp_of("m5", 3, 65, True)
    h = GP._handle()
    GP._push_prior()
    P = qr.pending_points(GP.X, 7); Z = qr.samples(1000, 8); Q = pc.queries(GP.X, 300, seed=9)
    one = qei_call(lib, h, P, Z, Q)
    for lo, hi in ((0, 1), (5, 12), (10, 74), (100, 165), (299, 300)):             # calls of 1, 7, 64 and 65 points
        part = qei_call(lib, h, P, Z, Q[lo:hi])
        for k in ("qei", "mu", "s2", "c"):
            assert np.array_equal(part[k], one[k][lo:hi]), (k, lo, hi)
        assert part["base"] == one["base"] and np.array_equal(part["S_pend"], one["S_pend"])
    singles = np.array([qei_call(lib, h, P, Z, Q[i], pieces=False)["qei"][0] for i in range(0, 300, 13)])
    assert np.array_equal(singles, one["qei"][::13])
    filler = pc.queries(GP.X, 1000, seed=10)
    big = filler.copy()
    big[100:400] = Q; big[611:911] = Q                              # chunks of 256: both copies cross chunk boundaries
    dc = DeviceArray.from_host(big, GP._dev.device)
    lib.check(lib.lib.ibo_set_option(b"qei_chunk", 256))
    try:
        bv, bi, v, base = sweep_call(lib, h, P, Z, dc, 1000, index_base=5000)
        chunked = qei_call(lib, h, P, Z, Q)
    finally:
        lib.check(lib.lib.ibo_set_option(b"qei_chunk", 0))
    assert np.array_equal(v[100:400], one["qei"]) and np.array_equal(v[611:911], one["qei"]) and base == one["base"]
    for k in ("qei", "mu", "s2", "c"):
        assert np.array_equal(chunked[k], one[k]), k
    assert bv == np.max(v) and bi == 5000 + int(np.argmax(v))
    # whole-array sweep without the option (one chunk) and without the per-candidate output
    b2, i2, _, base2 = sweep_call(lib, h, P, Z, dc, 1000, values=False)
    assert b2 == bv and i2 == int(np.argmax(v)) and base2 == base
    # without pending points as well
    Z1 = qr.samples(65, 1)
    one0 = qei_call(lib, h, [], Z1, Q, pieces=False)["qei"]
    _, _, v0, base0 = sweep_call(lib, h, [], Z1, dc, 1000)
    assert np.array_equal(v0[100:400], one0) and np.array_equal(v0[611:911], one0) and base0 == 0.0


def stage_ms(lib, entry, reset):
    """the six per-stage sums of ibo_qei_stage_ms / ibo_kg_stage_ms"""
    ms = np.full(6 + 2, GUARD)
    lib.check(getattr(lib.lib, entry)(lib.dp(ms), reset))
    assert np.all(ms[6:] == GUARD)
    return ms[:6]


def test_timing_leaves_the_values_alone_and_fills_its_own_sums(lib):
    """qei_timing over three chunks (256 + 256 + 88), with 7 pending points and with none: the same bits from the sweep and the host batch,
    six sums, their reset, none of the knowledge gradient's"""
    from ibo_amd import DeviceArray
    GP, _ = gp_of("m5", 3, 65, True)
    h = GP._handle()
    GP._push_prior()
    C = pc.queries(GP.X, 600, seed=11)
    dc = DeviceArray.from_host(C, GP._dev.device)

    def sums_of_a_timed_call(p):
        ms = stage_ms(lib, "ibo_qei_stage_ms", 1)
        print("qei stage sums (ms), p = %d:" % p, ms)
        assert np.all(np.isfinite(ms)) and np.all(ms >= 0)
        launching = [1, 2, 3, 5] + ([0, 4] if p else [])            # the pending state and the cross stage launch nothing without pending points
        assert np.all(ms[launching] > 0)
        if not p:
            assert ms[0] == 0.0
        assert np.all(stage_ms(lib, "ibo_qei_stage_ms", 0) == 0)    # the read above reset them
        assert np.all(stage_ms(lib, "ibo_kg_stage_ms", 0) == 0)     # and nothing went to the other unit's

    lib.check(lib.lib.ibo_set_option(b"qei_chunk", 256))
    try:
        lib.check(lib.lib.ibo_qei_stage_ms(None, 1)); lib.check(lib.lib.ibo_kg_stage_ms(None, 1))
        lib.check(lib.lib.ibo_qei_stage_ms(None, 0))
        for p in (7, 0):
            P = qr.pending_points(GP.X, p); Z = qr.samples(256, p + 1)
            lib.check(lib.lib.ibo_set_option(b"qei_timing", 0))
            sweep0 = sweep_call(lib, h, P, Z, dc, 600, index_base=3)
            host0 = qei_call(lib, h, P, Z, C)
            assert np.all(stage_ms(lib, "ibo_qei_stage_ms", 0) == 0)    # timing off: nothing is added
            lib.check(lib.lib.ibo_set_option(b"qei_timing", 1))
            sweep1 = sweep_call(lib, h, P, Z, dc, 600, index_base=3)
            sums_of_a_timed_call(p)
            host1 = qei_call(lib, h, P, Z, C)
            sums_of_a_timed_call(p)
            (b0, i0, v0, base0), (b1, i1, v1, base1) = sweep0, sweep1
            assert np.array_equal(v1, v0) and b1 == b0 and i1 == i0 and base1 == base0 and i0 == 3 + int(np.argmax(v0))
            for k in ("qei", "mu_pend", "S_pend", "mu", "s2", "c"):
                assert np.array_equal(host1[k], host0[k]), (k, p)
            assert host1["base"] == host0["base"] == base0 and np.array_equal(host0["qei"], v0)
    finally:
        lib.check(lib.lib.ibo_set_option(b"qei_timing", 0))
        lib.check(lib.lib.ibo_set_option(b"qei_chunk", 0))
        lib.check(lib.lib.ibo_qei_stage_ms(None, 1))


@pytest.mark.parametrize("D,p", [(2, 2), (4, 0)])
def test_direct_equals_the_host_tree_on_single_points(lib, D, p):
    from ibo_amd.acquisition import ParallelEI, maximizeQEI
    GP, _ = gp_of("ard", D, 40, False)
    h = GP._handle()
    P = lib.f64(qr.pending_points(GP.X, p)); Z = lib.f64(qr.samples(64, p + 1))
    lb, ub = lib.f64(np.zeros(D)), lib.f64(np.ones(D))
    opt = ctypes.c_double(); optx = np.empty(D); ns = ctypes.c_int64(); info = ctypes.c_int()
    head = (h, p, lib.dp(P) if p else None, 64, lib.dp(Z), NAN, qr.XI, qr.CLAMP_PY, 0.0)
    lib.check(lib.lib.ibo_qei_direct_max(*(head + (D, lib.dp(lb), lib.dp(ub), 12, 30, 10000, 1, ctypes.byref(opt), lib.dp(optx), ctypes.byref(ns),
                                                   ctypes.byref(info)))))
    val = np.empty(1)

    def negval(nd, x):
        q = lib.f64([x[i] for i in range(nd)])
        assert lib.lib.ibo_qei_batch(*(head + (1, lib.dp(q), lib.dp(val), None, None, None, None, None, None, None))) == 0
        return -val[0]
    cb = lib.OBJECTIVE(negval)
    fm = ctypes.c_double(); xm = np.empty(D); n2 = ctypes.c_int64()
    lib.check(lib.lib.ibo_direct_host(cb, D, lib.dp(lb), lib.dp(ub), 12, 30, 10000, 1, ctypes.byref(fm), lib.dp(xm), ctypes.byref(n2)))
    assert ns.value == n2.value and ns.value > 50
    assert np.array_equal(optx, xm) and opt.value == -fm.value and opt.value > 0
    o, ox = maximizeQEI(GP, [[0., 1.]] * D, P, xi=qr.XI, Z=Z, maxiter=12, compat=True)
    assert o == opt.value and np.array_equal(ox, optx)
    assert ParallelEI(GP, P, xi=qr.XI, Z=Z).f(ox) == o


def test_argmax_contract(lib):
    from ibo_amd import DeviceArray
    GP, _ = gp_of("m3", 3, 65, False)
    h = GP._handle()
    P = qr.pending_points(GP.X, 2); Z = qr.samples(63, 3); Q = pc.queries(GP.X, 600, seed=3)
    clean = qei_call(lib, h, P, Z, Q, pieces=False)["qei"]
    k = int(np.argmax(clean))
    # the best candidate again on both sides of a 256 boundary, after its first place or before it: the first index wins
    for places in ((255, 256), (511, 512, 599)):
        C = Q.copy()
        C[list(places)] = Q[k]
        dc = DeviceArray.from_host(C, GP._dev.device)
        bv, bi, v, _ = sweep_call(lib, h, P, Z, dc, 600, index_base=7)
        assert bv == clean[k] and bi == 7 + min(k, places[0]) and np.array_equal(v[list(places)], np.full(len(places), clean[k]))
    # NaN candidates: NaN values, never the winner -- the best one among them
    Qn = Q.copy(); Qn[k, 1] = np.nan; Qn[0, 0] = np.nan; Qn[256, 2] = np.nan
    got = qei_call(lib, h, P, Z, Qn, pieces=False)["qei"]
    bad = np.zeros(600, dtype=bool); bad[[k, 0, 256]] = True
    assert np.all(np.isnan(got[bad])) and np.array_equal(got[~bad], clean[~bad])
    bv, bi, v, _ = sweep_call(lib, h, P, Z, DeviceArray.from_host(Qn, GP._dev.device), 600, index_base=3)
    keep = np.flatnonzero(~bad)
    assert np.all(np.isnan(v[bad])) and bv == np.max(clean[keep]) and bi == 3 + int(keep[np.argmax(clean[keep])])
    # without pending points the same
    g0 = qei_call(lib, h, [], Z[:, :1], Qn, pieces=False)["qei"]
    assert np.all(np.isnan(g0[bad])) and np.all(np.isfinite(g0[~bad]))
    # nothing but NaN: no index, and index_base is not added
    dn = DeviceArray.from_host(np.full((300, 3), np.nan), GP._dev.device)
    bv, bi, _, _ = sweep_call(lib, h, P, Z, dn, 300, index_base=11, values=False)
    assert bv == -np.inf and bi == -1


def test_degenerate_geometry_against_the_composition(lib):
    GP, _ = gp_of("ard", 3, 65, False)
    h = GP._handle()
    P = qr.pending_points(GP.X, 3); Z = qr.samples(1000, 4); Q = pc.queries(GP.X, 70, seed=4)
    t = float(np.max(GP.Y)) + qr.XI
    # candidates equal to pending points
    g = qei_call(lib, h, P, Z, np.r_[P, Q[:5], P[1:2]])
    compose_close(g, Z, t, "candidates equal to pending points")
    # the same pending point listed twice, a little jitter
    P2 = np.r_[P[:2], P[1:2], P[2:]]; Z2 = qr.samples(1000, 5)
    g = qei_call(lib, h, P2, Z2, np.r_[Q, P2[1:2]], jitter=1e-8)
    compose_close(g, Z2, t, "a pending point listed twice")
    assert g["S_pend"][1, 1] == g["S_pend"][2, 2] and g["S_pend"][1, 2] < g["S_pend"][1, 1]
    plain = qei_call(lib, h, P2, Z2, Q[:1], jitter=0.0)
    assert np.all(np.diag(g["S_pend"]) > np.diag(plain["S_pend"])) and np.allclose(np.diag(g["S_pend"]) - np.diag(plain["S_pend"]), 1e-8, rtol=1e-6)
    # a joint covariance that is not positive definite: k* signal variance 2 puts k(p, p) = 2 above the diagonal 1 + noise
    GP2, _ = gp_of("ard", 3, 10, False)
    h2 = GP2._handle()
    far = np.full((2, 3), 30.0)
    lib.check(lib.lib.ibo_gp_set_kstar_sf2(h2, 2.0))
    bad = qei_call(lib, h2, far, Z[:, :3], Q[:4], expect=lib.ERR_NOT_PD)
    assert bad["info"] == 2
    lib.check(lib.lib.ibo_gp_set_kstar_sf2(h2, 1.0))
    ok = qei_call(lib, h2, far, Z[:, :3], Q[:4])
    assert ok["info"] == 0 and np.all(np.isfinite(ok["qei"]))


def test_errors_leave_the_handle_usable(lib):
    from ibo_amd import DeviceArray
    GP, _ = gp_of("ard", 3, 50, False)
    h = GP._handle()
    dp = lib.dp
    P = lib.f64(qr.pending_points(GP.X, 5)); Z = lib.f64(qr.samples(64, 6)); Q = lib.f64(pc.queries(GP.X, 4)); v = np.empty(4)
    lb, ub = lib.f64(np.zeros(3)), lib.f64(np.ones(3))
    dc = DeviceArray.from_host(Q, GP._dev.device)
    bv = ctypes.c_double(); bi = ctypes.c_int64(); ns = ctypes.c_int64(); ox = np.empty(3); info = ctypes.c_int()
    bigP = lib.f64(np.zeros((16, 3))); bigZ = lib.f64(np.zeros((4097, 17)))
    badP = P.copy(); badP[2, 1] = np.inf
    nanP = P.copy(); nanP[4, 2] = np.nan
    badZ = Z.copy(); badZ[63, 5] = np.inf
    nanZ = Z.copy(); nanZ[0, 0] = np.nan
    L = lib.lib

    def batch(g=h, p=5, pend=dp(P), S=64, z=dp(Z), xi=.01, jitter=0.0, M=4, q=dp(Q), out=dp(v)):
        return L.ibo_qei_batch(g, p, pend, S, z, NAN, xi, 1e-7, jitter, M, q, out, None, None, None, None, None, None, ctypes.byref(info))

    def sweep(g=h, p=5, pend=dp(P), S=64, z=dp(Z), xi=.01, jitter=0.0, M=4, c=dc.ptr, val=ctypes.byref(bv), idx=ctypes.byref(bi)):
        return L.ibo_qei_sweep(g, p, pend, S, z, NAN, xi, 1e-7, jitter, M, c, 0, None, None, val, idx, ctypes.byref(info))

    def direct(g=h, p=5, pend=dp(P), S=64, z=dp(Z), xi=.01, jitter=0.0, D=3, lo=dp(lb), hi=dp(ub), o=ctypes.byref(bv), x=dp(ox)):
        return L.ibo_qei_direct_max(g, p, pend, S, z, NAN, xi, 1e-7, jitter, D, lo, hi, 5, 5, 200, 1, o, x, ctypes.byref(ns), ctypes.byref(info))

    want = qei_call(lib, h, P, Z, Q, pieces=False)["qei"]
    common = (dict(g=None), dict(pend=None), dict(z=None), dict(p=-1), dict(p=16, pend=dp(bigP), z=dp(bigZ)), dict(S=0), dict(S=4097, z=dp(bigZ)),
              dict(pend=dp(badP)), dict(pend=dp(nanP)), dict(z=dp(badZ)), dict(z=dp(nanZ)), dict(xi=NAN), dict(xi=np.inf), dict(jitter=NAN),
              dict(jitter=np.inf), dict(jitter=-1e-9))
    calls = [lambda kw=kw: batch(**kw) for kw in common] + [lambda kw=kw: sweep(**kw) for kw in common] + [lambda kw=kw: direct(**kw) for kw in common]
    calls += [lambda: batch(q=None), lambda: batch(out=None), lambda: batch(M=0), lambda: batch(M=-3),
              lambda: sweep(c=None), lambda: sweep(val=None, idx=None), lambda: sweep(M=0),
              lambda: direct(lo=None), lambda: direct(hi=None), lambda: direct(D=2), lambda: direct(D=4),
              lambda: L.ibo_qei_direct_max(h, 5, dp(P), 64, dp(Z), NAN, .01, 1e-7, 0.0, 3, dp(lb), dp(ub), 5, 5, 200, 1, None, None, None, None)]
    for i, call in enumerate(calls):
        assert call() == lib.ERR_ARG, i
        assert np.array_equal(qei_call(lib, h, P, Z, Q, pieces=False)["qei"], want)        # the handle is still usable and correct
    assert batch(p=16, pend=dp(bigP), z=dp(bigZ)) == lib.ERR_ARG and b"15" in L.ibo_last_error()
    assert batch(S=4097, z=dp(bigZ)) == lib.ERR_ARG and b"4096" in L.ibo_last_error()
    hp = ctypes.c_void_p()
    lib.check(L.ibo_gp_create(0, ctypes.byref(hp)))
    try:
        assert batch(g=hp) == lib.ERR_STATE and sweep(g=hp) == lib.ERR_STATE and direct(g=hp) == lib.ERR_STATE
    finally:
        L.ibo_gp_destroy(hp)
    # no pending points: pend_host may be NULL; info is optional
    assert batch(p=0, pend=None) == lib.OK and np.all(np.isfinite(v))
    assert L.ibo_qei_batch(h, 5, dp(P), 64, dp(Z), NAN, .01, 1e-7, 0.0, 4, dp(Q), dp(v), None, None, None, None, None, None, None) == lib.OK
    assert np.array_equal(v, want)
    assert sweep() == lib.OK and bv.value == np.max(want) and bi.value == int(np.argmax(want))


def test_python_layer(lib):
    from ibo_amd import DeviceArray
    from ibo_amd.acquisition import EI, ParallelEI, baseSamples, jointQEI, maximizeQEI, proposeBatch, sweepQEI
    GP, ref = gp_of("sviso", 3, 30, True)
    bounds = [[0., 1.]] * 3
    P = qr.pending_points(GP.X, 3)
    Q = pc.queries(GP.X, 90, seed=5)
    acq = ParallelEI(GP, P, n_samples=256, seed=3, xi=qr.XI)
    assert acq.Z.shape == (256, 4) and np.array_equal(acq.Z, baseSamples(4, 256, seed=3))
    v = acq.values(Q)
    raw = qei_call(lib, GP._handle(), P, acq.Z, Q)
    assert np.array_equal(v, raw["qei"]) and acq.base == raw["base"]
    for a, k in zip(acq.pieces(Q), ("mu_pend", "S_pend", "mu", "s2", "c")):
        assert np.array_equal(a, raw[k]), k
    assert acq.f(Q[7]) == v[7] and acq.negf(Q[7]) == -v[7]
    t = float(np.max(GP.Y)) + qr.XI
    want = qr.qei(ref, P, Q, acq.Z, t)
    close(v, want["qei"], qr.tol_qei(want, acq.Z, t, ref.sf2, ref.noise), "ParallelEI.values")
    bv, bi = sweepQEI(GP, Q, P, xi=qr.XI, Z=acq.Z)
    assert bv == np.max(v) and bi == int(np.argmax(v))
    bv, bi, vals = sweepQEI(GP, DeviceArray.from_host(Q, GP._dev.device), P, n_samples=256, seed=3, xi=qr.XI, values=True, index_base=10)
    assert np.array_equal(vals, v) and bv == np.max(v) and bi == 10 + int(np.argmax(v))
    # the greedy batch over an array: the hand-written loop of sweeps, point for point; its value is the batch's joint value
    C = pc.queries(GP.X, 1000, seed=6)
    Zb = baseSamples(3 + 4, 512, seed=2)
    Xq, joint = proposeBatch(GP, candidates=C, q=4, pending=P, xi=qr.XI, Z=Zb)
    pend = P
    for j in range(4):
        val, i = sweepQEI(GP, C, pend, xi=qr.XI, Z=Zb)
        assert np.array_equal(Xq[j], C[i]), j
        pend = np.r_[pend, C[i:i + 1]]
    assert joint == val and joint == jointQEI(GP, np.r_[P, Xq], xi=qr.XI, Z=Zb) and joint > 0
    Xd, jd = proposeBatch(GP, candidates=DeviceArray.from_host(C, GP._dev.device), q=4, pending=P, n_samples=512, seed=2, xi=qr.XI)
    assert np.array_equal(Xd, Xq) and jd == joint
    # with bounds: the loop of maximizeQEI
    Xb, jb = proposeBatch(GP, bounds=bounds, q=3, xi=qr.XI, Z=Zb, maxiter=6)
    pend = np.empty((0, 3))
    for j in range(3):
        val, x = maximizeQEI(GP, bounds, pend, xi=qr.XI, Z=Zb, maxiter=6)
        assert np.array_equal(Xb[j], x), j
        pend = np.r_[pend, [x]]
    assert jb == val and jb == jointQEI(GP, Xb, xi=qr.XI, Z=Zb) and np.all((Xb >= 0) & (Xb <= 1))
    # refusals: a wrong width, too many pending points, both or neither of bounds and candidates
    for call in (lambda: ParallelEI(GP, P[:, :2]), lambda: acq.values(Q[:, :2]), lambda: acq.f(Q[0, :2]), lambda: sweepQEI(GP, Q[:, :2], P),
                 lambda: sweepQEI(GP, DeviceArray.from_host(np.c_[Q, Q[:, :1]], GP._dev.device), P), lambda: maximizeQEI(GP, bounds[:2], P),
                 lambda: ParallelEI(GP, np.zeros((16, 3))), lambda: jointQEI(GP, np.zeros((17, 3))), lambda: proposeBatch(GP, bounds=bounds, q=14, pending=P),
                 lambda: proposeBatch(GP), lambda: proposeBatch(GP, bounds=bounds, candidates=C), lambda: ParallelEI(GP, P, Z=np.zeros((8, 3)))):
        with pytest.raises(ValueError):
            call()
    assert np.array_equal(acq.values(Q), v)
    # without pending points and with 4096 antithetic draws: EI within 5 standard errors of the sample (pairs are the independent units)
    acq0 = ParallelEI(GP, None, n_samples=4096, seed=0, xi=qr.XI)
    Qe = qr.ei_candidates(np.asarray(GP.X), np.asarray(GP.Y))
    _, _, mu, s2, _ = acq0.pieces(Qe)
    ratio = qr.antithetic_ratio(mu, s2, acq0.Z, t, acq0.values(Qe), np.array([EI(GP, xi=qr.XI).f(x) for x in Qe]))
    print("ParallelEI without pending points against EI: worst |difference| / standard error = %.3g" % float(np.max(ratio)))
    assert np.all(ratio <= 5.0) and acq0.base == 0.0


def test_preference_model_and_the_augmented_refusal(lib):
    from ibo_amd.acquisition import ParallelEI
    from ibo_amd.gaussianprocess import PrefGaussianProcess
    from ibo_amd.gaussianprocess.kernel import GaussianKernel_ard
    rs = np.random.RandomState(3)
    GP = PrefGaussianProcess(GaussianKernel_ard(np.array([.6] * 4)))
    X = rs.rand(40, 4)
    GP.addPreferences([(X[2 * i], X[2 * i + 1], 0) for i in range(20)])
    P = rs.rand(3, 4); Q = rs.rand(30, 4)
    acq = ParallelEI(GP, P, n_samples=256, seed=1)
    g = dict(zip(("mu_pend", "S_pend", "mu", "s2", "c"), acq.pieces(Q)))
    g["qei"] = acq.values(Q); g["base"] = acq.base
    maxy = ctypes.c_double()
    lib.check(lib.lib.ibo_gp_info(GP._handle(), None, None, None, ctypes.byref(maxy)))
    compose_close(g, acq.Z, maxy.value, "preference model")
    assert np.max(g["qei"]) > 0
    np.testing.assert_allclose(g["mu_pend"], GP.posteriors(P)[0], rtol=1e-6, atol=1e-9)
    np.testing.assert_allclose(g["s2"], GP.posteriors(Q)[1], rtol=1e-6)
    GP.addObservationPoint(rs.rand(4))
    with pytest.raises(ValueError):
        acq.values(Q)
    with pytest.raises(ValueError):
        ParallelEI(GP, P)

"""
ibo_ggp_* -- a GP observed with gradients -- and what is built on it: GaussianProcess(G=), addData(X, Y, G), EI / PI / UCB,
acquisition.sweep and maximizeEI / PI / UCB on such a model.

The yardstick is tests/gradobs_reference.py (pinned by tests/test_gradobs_reference.py), in long double wherever cond_2(A) > 1e6.  Bars:
    R          1e-12 x the largest magnitude of that kind of block entry in A (value-value, value-derivative, derivative-derivative)
    L          |L L^T - A|_max <= 4 P 2^-53 max_i A_ii, the Cholesky backward-error bound
    mu, s2     1e-15 max(cond_2, 1e6) x sum_j |k*_j alpha_j|, resp. x (1 + noise + |v|^2): the NLML tests' bars
    EI/PI/UCB  1e-12 x max(1, |value|) against acq_value_dev restated on the device's own (mu, s2); end to end against the reference's
               (mu, s2) 1e-6 relative, on top of that 1e-12 (the epilogue's own bar: a PI of 1e-13 from the NR erf is quantised at 1e-16)
    sweep, DIRECT against the host batch: bit for bit
"""
import ctypes
import functools

import numpy as np
import pytest

import gradobs_reference as gr
from test_gradobs_reference import value_only_bound

pytestmark = pytest.mark.gpu
GUARD = 7.25


@pytest.fixture(scope="module")
def lib():
    from ibo_amd import _lib
    if _lib.device_count() < 1:
        pytest.fail("no GPU visible: the product has no CPU fallback")
    return _lib


class Handle(object):
    """an ibo_ggp_t fitted through the raw ABI"""

    def __init__(self, kern, X, Y, G, noise, gnoise, fit=True):
        from ibo_amd import _lib
        self.lib = _lib
        self.h = ctypes.c_void_p()
        _lib.check(_lib.lib.ibo_ggp_create(_lib.default_device(), ctypes.byref(self.h)))
        self.N, self.D = X.shape
        self.P = self.N * (self.D + 1)
        self.info = ctypes.c_int(-1)
        if fit:
            _lib.check(self.fit(kern, X, Y, G, noise, gnoise))

    def fit(self, kern, X, Y, G, noise, gnoise):
        L = self.lib
        hyper = L.f64(kern.theta)
        return L.lib.ibo_ggp_fit(self.h, kern.ktype, len(X), X.shape[1], L.dp(L.f64(X)), L.dp(L.f64(Y)), L.dp(L.f64(G)), L.dp(hyper), len(hyper),
                                 kern.sf2_py, float(noise), L.dp(L.f64(gr.tile_gnoise(gnoise, X.shape[1]))), ctypes.byref(self.info))

    def matrix(self, name):
        out = np.full(self.P * self.P + 8, GUARD)
        self.lib.check(getattr(self.lib.lib, "ibo_ggp_get_" + name)(self.h, self.lib.dp(out)))
        assert np.all(out[self.P * self.P:] == GUARD)
        return out[:self.P * self.P].reshape(self.P, self.P)

    def batch(self, Q, acq=gr.ACQ_NONE, parm=0.0, erf_mode=gr.ERF_LIBM, clamp=gr.CLAMP_PY, ymax=float("nan"), want=("mu", "s2", "acq")):
        L = self.lib
        Q = L.f64(np.atleast_2d(Q))
        M = len(Q)
        out = {k: np.full(M + 8, GUARD) for k in want}
        ptr = lambda k: L.dp(out[k]) if k in out else None
        L.check(L.lib.ibo_ggp_acq_batch(self.h, M, L.dp(Q), acq, float(parm), erf_mode, clamp, float(ymax), ptr("mu"), ptr("s2"), ptr("acq")))
        for k in out:
            assert np.all(out[k][M:] == GUARD), "guard behind %s overwritten" % k
            out[k] = out[k][:M]
        return out

    def sweep(self, cand, M, acq, parm, erf_mode, clamp, ymax=float("nan"), index_base=0, outputs=True):
        L = self.lib
        dev = L.default_device()
        outs = {k: L.DeviceArray((M + 8,), dev) for k in (("mu", "s2", "acq") if outputs else ())}
        for v in outs.values():
            v.upload(np.full(M + 8, GUARD))
        bv = ctypes.c_double(); bi = ctypes.c_int64()
        p = lambda k: outs[k].ptr if k in outs else None
        L.check(L.lib.ibo_ggp_acq_sweep(self.h, M, cand.ptr, acq, float(parm), erf_mode, clamp, float(ymax), int(index_base),
                                        p("mu"), p("s2"), p("acq"), ctypes.byref(bv), ctypes.byref(bi)))
        res = dict(best_val=bv.value, best_idx=bi.value)
        for k, v in outs.items():
            a = v.to_host()
            assert np.all(a[M:] == GUARD), "guard behind the sweep's %s overwritten" % k
            res[k] = a[:M]
        return res

    def close(self):
        if getattr(self, "h", None):
            try:
                self.lib.lib.ibo_ggp_destroy(self.h)
            except Exception:
                pass
            self.h = None

    def __del__(self):
        self.close()


@functools.lru_cache(maxsize=None)
def device_case(name):
    """one listed case on the device and in the reference, computed once for the tests that read it: the handle, the queries (the
    smaller query counts are prefixes of the 130) and the reference's posterior there"""
    c = gr.case(name)
    ref = gr.reference_model(name)
    Q = gr.queries(c["X"], max(gr.QUERY_COUNTS))
    Q.setflags(write=False)
    return Handle(c["kern"], c["X"], c["Y"], c["G"], c["noise"], c["gnoise"]), c, ref, Q, gr.posterior(ref, Q, gr.CLAMP_PY)


def same_bits(a, b):
    return np.array_equal(np.asarray(a).view(np.uint64), np.asarray(b).view(np.uint64))


# ---------------------------------------------------------------------------- the matrix and its factor
@pytest.mark.parametrize("name", gr.CASE_NAMES)
def test_R_is_the_restated_matrix_and_L_its_factor(lib, name):
    h, c, ref, _, _ = device_case(name)
    N, D, P = h.N, h.D, h.P
    info = [ctypes.c_int(), ctypes.c_int(), ctypes.c_int(), ctypes.c_int(), ctypes.c_double()]
    lib.check(lib.lib.ibo_ggp_info(h.h, *[ctypes.byref(v) for v in info]))
    assert [v.value for v in info[:3]] == [N, D, P] and info[4].value == np.max(c["Y"])
    A = gr.matrix(c["kern"], c["X"], c["noise"], c["gnoise"])
    R = h.matrix("R")
    assert np.array_equal(R, R.T)
    val = np.zeros(P, dtype=bool); val[::D + 1] = True
    for rows, cols, kind in ((val, val, "value-value"), (val, ~val, "value-derivative"), (~val, ~val, "derivative-derivative")):
        a, r = A[np.ix_(rows, cols)], R[np.ix_(rows, cols)]
        err, bar = float(np.max(np.abs(a - r))), 1e-12 * float(np.max(np.abs(a)))
        print("%s %s: |R - A| %.3g, bar %.3g" % (name, kind, err, bar))
        assert err <= bar, (kind, err, bar)
    L = h.matrix("L")
    assert np.all(np.triu(L, 1) == 0.0)
    back, bar = float(np.max(np.abs(L @ L.T - R))), 4.0 * P * 2.0 ** -53 * float(np.max(np.diag(R)))
    print("%s: |L L^T - A| %.3g, bar %.3g" % (name, back, bar))
    assert back <= bar


# ---------------------------------------------------------------------------- the posterior
@pytest.mark.parametrize("name", gr.CASE_NAMES)
def test_posterior_within_the_conditioning_bars(lib, name):
    h, c, ref, Q, want = device_case(name)
    bmu, bs2 = gr.bars(ref, want)
    wmu, ws2 = np.asarray(want["mu"], dtype=np.float64), np.asarray(want["s2"], dtype=np.float64)
    for M in gr.QUERY_COUNTS:
        got = h.batch(Q[:M], want=("mu", "s2"))
        rmu, rs2 = np.abs(got["mu"] - wmu[:M]) / bmu[:M], np.abs(got["s2"] - ws2[:M]) / bs2[:M]
        print("%s M=%d (cond %.3g, %s): mu at %.3g of the bar, s2 at %.3g" % (name, M, ref["cond"], ref["dt"].__name__, rmu.max(), rs2.max()))
        assert np.all(rmu <= 1.0) and np.all(rs2 <= 1.0)
    full = h.batch(Q, want=("mu", "s2"))
    for M in gr.QUERY_COUNTS:                                          # a point's bits do not depend on the batch it came in
        part = h.batch(Q[:M], want=("mu", "s2"))
        assert same_bits(part["mu"], full["mu"][:M]) and same_bits(part["s2"], full["s2"][:M])


@pytest.mark.parametrize("name", gr.CASE_NAMES)
def test_acquisitions_in_both_erf_flavours(lib, name):
    h, c, ref, Q, want = device_case(name)
    wmu, ws2 = np.asarray(want["mu"], dtype=np.float64), np.asarray(want["s2"], dtype=np.float64)
    ymax = float(np.max(c["Y"]))
    for acq, parm in ((gr.ACQ_EI, 0.01), (gr.ACQ_PI, 0.01), (gr.ACQ_UCB, 1.7)):
        for erf_mode in (gr.ERF_LIBM, gr.ERF_NR):
            got = h.batch(Q, acq, parm, erf_mode, gr.CLAMP_PY)
            own = gr.acquisition(acq, erf_mode, got["mu"], got["s2"], ymax, parm)
            e1 = np.abs(got["acq"] - own) / np.maximum(1.0, np.abs(own))
            end = gr.acquisition(acq, erf_mode, wmu, ws2, ymax, parm)
            e2 = np.abs(got["acq"] - end) / (1e-6 * np.abs(end) + 1e-12)
            print("%s acq %d erf %d: epilogue %.3g (bar 1e-12), end to end at %.3g of the bar" % (name, acq, erf_mode, e1.max(), e2.max()))
            assert np.all(e1 <= 1e-12) and np.all(e2 <= 1.0)
            explicit = h.batch(Q, acq, parm, erf_mode, gr.CLAMP_PY, ymax=ymax)         # ymax NaN is max(Y), over the values only
            assert same_bits(explicit["acq"], got["acq"])


# ---------------------------------------------------------------------------- the sweep
SWEEP_M = (1, 63, 64, 65, 300, 4097)


@pytest.mark.parametrize("chunk", [256, 0])
@pytest.mark.parametrize("name", ["ard_13x4", "m5_43x2"])
def test_sweep_is_the_batch_bit_for_bit(lib, name, chunk):
    h, c, _, _, _ = device_case(name)
    Q = lib.f64(np.random.RandomState(17).rand(max(SWEEP_M), h.D))
    base = {}
    spec = ((gr.ACQ_EI, 0.01, gr.ERF_LIBM, gr.CLAMP_NATIVE), (gr.ACQ_UCB, 1.3, gr.ERF_NR, gr.CLAMP_PY))
    assert lib.lib.ibo_set_option(b"ggp_chunk", 0) == 0
    for s in spec:
        base[s] = h.batch(Q, *s)
    cand = lib.DeviceArray.from_host(Q)
    assert lib.lib.ibo_set_option(b"ggp_chunk", chunk) == 0            # 256: 300 candidates span two chunks, 4097 seventeen
    try:
        for s in spec:
            again = h.batch(Q, *s)                                     # the host batch itself, in other chunks
            for k in ("mu", "s2", "acq"):
                assert same_bits(again[k], base[s][k])
            for M in SWEEP_M:
                r = h.sweep(cand, M, *s, index_base=1000)
                for k in ("mu", "s2", "acq"):
                    assert same_bits(r[k], base[s][k][:M]), (name, chunk, M, k)
                k0 = int(np.argmax(base[s]["acq"][:M]))
                assert r["best_idx"] == 1000 + k0 and r["best_val"] == base[s]["acq"][k0]
                bare = h.sweep(cand, M, *s, outputs=False)
                assert bare["best_idx"] == k0 and bare["best_val"] == r["best_val"]
    finally:
        assert lib.lib.ibo_set_option(b"ggp_chunk", 0) == 0


def test_sweep_arg_max_rule(lib):
    """the first of duplicated best candidates wins; a NaN row never wins; nothing admissible: (-inf, -1)"""
    h, c, _, _, _ = device_case("ard_13x4")
    M = 700
    Q = lib.f64(np.random.RandomState(23).rand(M, h.D))
    s = (gr.ACQ_EI, 0.01, gr.ERF_LIBM, gr.CLAMP_NATIVE)
    k0 = int(np.argmax(h.batch(Q, *s)["acq"]))
    for dup in (5, 300, 699):                                          # the winner again: before it, in a later chunk, last
        if dup == k0:
            continue
        Q2 = Q.copy(); Q2[dup] = Q[k0]
        r = h.sweep(lib.DeviceArray.from_host(Q2), M, *s, index_base=10, outputs=False)
        assert r["best_idx"] == 10 + min(dup, k0)
    assert lib.lib.ibo_set_option(b"ggp_chunk", 256) == 0
    try:
        Q3 = Q.copy(); Q3[k0, 1] = np.nan; Q3[0] = np.nan
        r = h.sweep(lib.DeviceArray.from_host(Q3), M, *s)
        assert np.isnan(r["acq"][k0]) and np.isnan(r["mu"][k0]) and np.isnan(r["acq"][0])
        score = np.where(np.isnan(r["acq"]), -np.inf, r["acq"])
        assert r["best_idx"] == int(np.argmax(score)) != k0 and r["best_val"] == score.max()
        r = h.sweep(lib.DeviceArray.from_host(np.full((300, h.D), np.nan)), 300, *s, index_base=7, outputs=False)
        assert r["best_idx"] == -1 and r["best_val"] == -np.inf
    finally:
        assert lib.lib.ibo_set_option(b"ggp_chunk", 0) == 0


# ---------------------------------------------------------------------------- DIRECT
def test_direct_equals_the_host_tree_on_single_points(lib):
    h, c, _, _, _ = device_case("m5_43x2")
    D = 2
    lb, ub = lib.f64(np.zeros(D)), lib.f64(np.ones(D))
    opt = ctypes.c_double(); optx = np.empty(D); ns = ctypes.c_int64()
    lib.check(lib.lib.ibo_ggp_direct_max(h.h, D, lib.dp(lb), lib.dp(ub), gr.ACQ_EI, 0.01, gr.ERF_LIBM, gr.CLAMP_NATIVE, 10, 30, 10000, 1,
                                         ctypes.byref(opt), lib.dp(optx), ctypes.byref(ns)))
    val = np.empty(1)

    def negval(nd, x):
        q = lib.f64([x[i] for i in range(nd)])
        assert lib.lib.ibo_ggp_acq_batch(h.h, 1, lib.dp(q), gr.ACQ_EI, 0.01, gr.ERF_LIBM, gr.CLAMP_NATIVE, float("nan"), None, None,
                                         lib.dp(val)) == 0
        return -val[0]
    cb = lib.OBJECTIVE(negval)
    fm = ctypes.c_double(); xm = np.empty(D); n2 = ctypes.c_int64()
    lib.check(lib.lib.ibo_direct_host(cb, D, lib.dp(lb), lib.dp(ub), 10, 30, 10000, 1, ctypes.byref(fm), lib.dp(xm), ctypes.byref(n2)))
    assert ns.value == n2.value and ns.value > 30
    assert np.array_equal(optx, xm) and opt.value == -fm.value and opt.value > 0


# ---------------------------------------------------------------------------- the value-only limit
@pytest.mark.parametrize("kind,hyper", [("ard", [0.5, 0.8]), ("m3", [0.7, 0.9]), ("m5", [0.55, 0.8])])
def test_with_huge_gradient_noise_the_device_agrees_with_its_plain_twin(lib, kind, hyper):
    from oracle import oracle as orc
    kern = orc.Kern(kind, hyper)
    X = gr.points(8, 2, 11)
    Y, G = gr.objective(X)
    Q = lib.f64(gr.queries(X, 40))
    noise, gnoise = 0.1, 1e12
    h = Handle(kern, X, Y, G, noise, gnoise)
    got = h.batch(Q, gr.ACQ_EI, 0.01, gr.ERF_LIBM, gr.CLAMP_PY)
    p = ctypes.c_void_p()
    lib.check(lib.lib.ibo_gp_create(lib.default_device(), ctypes.byref(p)))
    try:
        th = lib.f64(kern.theta)
        lib.check(lib.lib.ibo_gp_fit(p, kern.ktype, len(X), 2, lib.dp(lib.f64(X)), lib.dp(lib.f64(Y)), lib.dp(th), len(th), kern.sf2_py, noise, None))
        mu, s2 = np.empty(len(Q)), np.empty(len(Q))
        lib.check(lib.lib.ibo_acq_batch(p, len(Q), lib.dp(Q), gr.ACQ_NONE, 0.0, gr.ERF_LIBM, gr.CLAMP_PY, float("nan"), lib.dp(mu), lib.dp(s2), None))
    finally:
        lib.lib.ibo_gp_destroy(p)
    bmu, bs2 = value_only_bound(kern, X, Y, G, Q, noise, gnoise)
    print("%s: mu %.3g (bound %.3g + 1e-9), s2 %.3g (bound %.3g + 1e-9)" % (kind, np.max(np.abs(got["mu"] - mu)), bmu, np.max(np.abs(got["s2"] - s2)), bs2))
    assert np.max(np.abs(got["mu"] - mu)) <= bmu + 1e-9 and np.max(np.abs(got["s2"] - s2)) <= bs2 + 1e-9
    h.close()


# ---------------------------------------------------------------------------- errors
def test_state_and_argument_errors_and_a_matrix_without_a_factor(lib):
    c = gr.case("ard_13x4")
    h = Handle(c["kern"], c["X"], c["Y"], c["G"], c["noise"], c["gnoise"], fit=False)
    q = lib.f64(c["X"][:2]); out = np.zeros(2)
    bv = ctypes.c_double(); lb = lib.f64(np.zeros(4)); ub = lib.f64(np.ones(4))
    assert lib.lib.ibo_ggp_acq_batch(h.h, 2, lib.dp(q), 0, 0.01, 0, 1e-8, float("nan"), None, None, lib.dp(out)) == lib.ERR_STATE
    assert lib.lib.ibo_ggp_get_R(h.h, lib.dp(np.zeros(65 * 65))) == lib.ERR_STATE and lib.lib.ibo_ggp_get_L(h.h, lib.dp(np.zeros(65 * 65))) == lib.ERR_STATE
    assert lib.lib.ibo_ggp_direct_max(h.h, 4, lib.dp(lb), lib.dp(ub), 0, 0.01, 0, 1e-8, 5, 30, 1000, 1, ctypes.byref(bv), None, None) == lib.ERR_STATE
    cand = lib.DeviceArray.from_host(q)
    assert lib.lib.ibo_ggp_acq_sweep(h.h, 2, cand.ptr, 0, 0.01, 0, 1e-8, float("nan"), 0, None, None, None, ctypes.byref(bv), None) == lib.ERR_STATE
    lib.check(h.fit(c["kern"], c["X"], c["Y"], c["G"], c["noise"], c["gnoise"]))
    assert h.info.value == 0
    good = h.batch(q, want=("mu",))["mu"]
    assert lib.lib.ibo_ggp_acq_batch(h.h, 0, lib.dp(q), 0, 0.01, 0, 1e-8, float("nan"), None, None, lib.dp(out)) == lib.ERR_ARG
    assert lib.lib.ibo_ggp_acq_batch(h.h, 2, lib.dp(q), 0, 0.01, 0, 1e-8, float("nan"), None, None, None) == lib.ERR_ARG
    assert lib.lib.ibo_ggp_acq_batch(h.h, 2, lib.dp(q), 7, 0.01, 0, 1e-8, float("nan"), None, None, lib.dp(out)) == lib.ERR_ARG
    assert lib.lib.ibo_ggp_acq_batch(h.h, 2, None, 0, 0.01, 0, 1e-8, float("nan"), None, None, lib.dp(out)) == lib.ERR_ARG
    assert lib.lib.ibo_ggp_direct_max(h.h, 3, lib.dp(lb), lib.dp(ub), 0, 0.01, 0, 1e-8, 5, 30, 1000, 1, ctypes.byref(bv), None, None) == lib.ERR_ARG
    assert lib.lib.ibo_ggp_direct_max(h.h, 4, lib.dp(lb), lib.dp(ub), 3, 0.01, 0, 1e-8, 5, 30, 1000, 1, ctypes.byref(bv), None, None) == lib.ERR_ARG
    assert same_bits(h.batch(q, want=("mu",))["mu"], good)
    # more rows than IBO_GGP_MAX_ROWS: refused before anything is touched (8192 rows: N = 1639, D = 4 is 8195)
    big = np.zeros((1639, 4))
    assert h.fit(c["kern"], big, np.zeros(1639), big, 0.1, 1e-4) == lib.ERR_ARG
    assert same_bits(h.batch(q, want=("mu",))["mu"], good)
    # the first two points coincide, noise = gnoise = 0, sf2 = 1: the value row of the second point repeats that of the first, whose
    # cross terms with its own derivatives are exactly 0 -- the pivot of row D + 2 is 1 - 1 = 0: a returned error, not a fault
    from oracle import oracle as orc
    X = np.array(c["X"][:6]); X[1] = X[0]
    Y, G = gr.objective(X)
    rc = h.fit(orc.Kern("ard", [0.6, 0.8, 0.7, 0.9]), X, Y, G, 0.0, 0.0)
    print("coincident points without noise: status %d, pivot %d" % (rc, h.info.value))
    assert rc == lib.ERR_NOT_PD and h.info.value == 6
    assert lib.lib.ibo_ggp_acq_batch(h.h, 2, lib.dp(q), 0, 0.01, 0, 1e-8, float("nan"), None, None, lib.dp(out)) == lib.ERR_STATE
    lib.check(h.fit(c["kern"], c["X"], c["Y"], c["G"], c["noise"], c["gnoise"]))
    assert same_bits(h.batch(q, want=("mu",))["mu"], good)
    h.close()


# ---------------------------------------------------------------------------- the Python layer
def make_kernel(kind, hyper):
    from ibo_amd.gaussianprocess import kernel as K
    return {"ard": K.GaussianKernel_ard, "iso": K.GaussianKernel_iso, "m3": K.MaternKernel3, "m5": K.MaternKernel5}[kind](hyper)


def python_model(name, upto=None):
    from ibo_amd.gaussianprocess import GaussianProcess
    c = gr.case(name)
    kind, hyper = gr.CASES[gr.CASE_NAMES.index(name)][1:3]
    n = len(c["X"]) if upto is None else upto
    return GaussianProcess(make_kernel(kind, hyper), c["X"][:n], c["Y"][:n], noise=c["noise"], G=c["G"][:n]), c


def test_a_model_built_with_G_works_through_every_listed_call(lib):
    from ibo_amd.acquisition import EI, PI, UCB, sweep, maximizeEI, maximizePI, maximizeUCB
    GP, c = python_model("m5_43x2")
    h, _, ref, Q, want = device_case("m5_43x2")
    assert GP.G.shape == GP.X.shape and np.array_equal(GP.gnoise, [1e-4, 1e-4])
    raw = h.batch(Q, gr.ACQ_EI, 0.01, gr.ERF_NR, gr.CLAMP_PY, ymax=np.max(GP.Y))
    mu, s2 = GP.posteriors(Q)
    assert same_bits(mu, raw["mu"]) and same_bits(s2, raw["s2"])
    m0, v0 = GP.posterior(Q[3])
    assert m0 == mu[3] and v0 == s2[3] and GP.mu(Q[3]) == mu[3] and GP.negmu(Q[3]) == -mu[3] and GP.posterior(Q[3], getvar=False) == mu[3]
    P = 43 * 3
    assert GP.R.shape == (P, P) and GP.L.shape == (P, P)
    assert np.array_equal(GP.R, h.matrix("R")) and np.array_equal(GP.L, h.matrix("L"))
    ei, pi, ucb = EI(GP, xi=0.01), PI(GP, xi=0.01), UCB(GP, 2)
    assert same_bits(ei.values(Q), raw["acq"]) and ei.f(Q[5]) == raw["acq"][5] and ei.negf(Q[5]) == -raw["acq"][5]
    assert pi.f(Q[5]) == h.batch(Q[5], gr.ACQ_PI, 0.01, gr.ERF_NR, gr.CLAMP_PY)["acq"][0] == -pi.negf(Q[5])
    assert ucb.f(Q[5]) == h.batch(Q[5], gr.ACQ_UCB, np.sqrt(ucb.scale * ucb.sBeta), gr.ERF_NR, gr.CLAMP_PY)["acq"][0] == -ucb.negf(Q[5])
    r = sweep(GP, Q, acq='ei', xi=0.01, native=False, outputs=("mu", "s2", "acq"), index_base=50)
    assert same_bits(r["acq"], raw["acq"]) and same_bits(r["mu"], mu) and same_bits(r["s2"], s2)
    assert r["best_idx"] == 50 + int(np.argmax(raw["acq"])) and r["best_val"] == raw["acq"].max()
    nat = sweep(GP, lib.DeviceArray.from_host(Q), acq='pi', xi=0.02, native=True, ymax=0.3, outputs=("acq",))
    assert same_bits(nat["acq"], h.batch(Q, gr.ACQ_PI, 0.02, gr.ERF_LIBM, gr.CLAMP_NATIVE, ymax=0.3)["acq"])
    b = [[0., 1.]] * 2
    for fn, code, kw, parm in ((maximizeEI, gr.ACQ_EI, dict(xi=0.01), 0.01), (maximizePI, gr.ACQ_PI, dict(xi=0.01), 0.01),
                               (maximizeUCB, gr.ACQ_UCB, {}, None)):
        opt, optx = fn(GP, b, maxiter=6, **kw)
        if parm is None:
            from ibo_amd.acquisition import _ucb_parm
            parm = _ucb_parm(GP, b, 0.1, 0.2)
        assert opt == h.batch(optx, code, parm, gr.ERF_LIBM, gr.CLAMP_NATIVE)["acq"][0]
        assert np.all(optx >= 0.0) and np.all(optx <= 1.0)


def test_addData_with_G_equals_a_fresh_model_bit_for_bit(lib):
    GP, c = python_model("ard_13x4", upto=9)
    GP.addData(c["X"][9:12], c["Y"][9:12], c["G"][9:12])
    GP.addData(c["X"][12], c["Y"][12], c["G"][12])                     # one point, as vectors
    fresh, _ = python_model("ard_13x4")
    assert np.array_equal(GP.X, fresh.X) and np.array_equal(GP.Y, fresh.Y) and np.array_equal(GP.G, fresh.G)
    Q = gr.queries(c["X"], 65)
    for a, b in zip(GP.posteriors(Q), fresh.posteriors(Q)):
        assert same_bits(a, b)
    assert np.array_equal(GP.R, fresh.R) and np.array_equal(GP.L, fresh.L)
    from copy import deepcopy
    twin = deepcopy(GP)
    assert same_bits(twin.posteriors(Q)[0], fresh.posteriors(Q)[0])


def test_refused_calls_and_mixed_data(lib):
    from ibo_amd import NotPositiveDefinite
    from ibo_amd.gaussianprocess import GaussianProcess, PrefGaussianProcess
    from ibo_amd import acquisition as A
    from ibo_amd.acquisition import constrained as C, multiobjective as MO
    GP, c = python_model("iso_32x3")
    X, Y, G = c["X"], c["Y"], c["G"]
    Q = gr.queries(X, 8)
    before = GP.posteriors(Q)
    with pytest.raises(ValueError):
        GaussianProcess(GP.kernel, X, Y, G=G[:, :2])
    with pytest.raises(ValueError):
        GP.addData(X[:1] + 0.01, Y[:1])                                # a gradient model, data without G
    plain = GaussianProcess(GP.kernel, X, Y, noise=0.1)
    with pytest.raises(ValueError):
        plain.addData(X[:1] + 0.01, Y[:1], G[:1])                      # a plain model, data with G
    assert same_bits(plain.posteriors(Q)[0], GaussianProcess(GP.kernel, X, Y, noise=0.1).posteriors(Q)[0])

    class Prior(object):
        means = np.zeros((1, 3)); beta = np.ones(1); theta = 1.0; lowerb = np.zeros(3); width = np.ones(3)
    with pytest.raises(NotImplementedError, match="prior"):
        GaussianProcess(GP.kernel, X, Y, prior=Prior(), G=G)
    with pytest.raises(NotImplementedError, match="PrefGaussianProcess"):
        PrefGaussianProcess(GP.kernel, X=X, Y=Y, G=G)
    b = [[0., 1.]] * 3
    refused = [
        ("removeData", lambda: GP.removeData(0)), ("posterior_gradient", lambda: GP.posterior_gradient(Q)),
        ("posterior_cov", lambda: GP.posterior_cov(Q)), ("sample_posterior", lambda: GP.sample_posterior(Q)),
        ("loo", lambda: GP.loo()), ("loo", lambda: GP.loo_score()),
        ("polish", lambda: A.maximizeEI(GP, b, polish=True)), ("polish", lambda: A.maximizePI(GP, b, polish=True)),
        ("polish", lambda: A.maximizeUCB(GP, b, polish=True)),
        ("incremental", lambda: A.sweep(GP, Q, incremental=True)), ("exclude", lambda: A.sweep(GP, Q, exclude=X[:2])),
        ("exchange", lambda: A.sweep(GP, Q, exchange=object())),
        ("gradient", lambda: A.EI(GP).gradient(Q)),
        ("knowledge gradient", lambda: A.KnowledgeGradient(GP, X[:4])), ("knowledge gradient", lambda: A.sweepKG(GP, Q, X[:4])),
        ("knowledge gradient", lambda: A.maximizeKG(GP, b, n_ref=8)),
        ("parallel expected improvement", lambda: A.ParallelEI(GP)), ("parallel expected improvement", lambda: A.sweepQEI(GP, Q)),
        ("parallel expected improvement", lambda: A.proposeBatch(GP, bounds=b, q=2)),
        ("constrained", lambda: C.ConstrainedEI(GP, [])), ("constrained", lambda: C.ConstrainedEI(plain, [C.Constraint(GP, upper=0.0)]).values(Q)),
        ("sweepConstrained", lambda: C.sweepConstrained(GP, [], Q)), ("maximizeCEI", lambda: C.maximizeCEI(GP, [], b)),
        ("hypervolume", lambda: MO.sweepEHVI([GP, plain], Q, [-1.0, -1.0])), ("hypervolume", lambda: MO.ExpectedHypervolumeImprovement([plain, GP], [-1.0, -1.0])),
        ("pathwise", lambda: A.PosteriorPaths(GP, n_paths=2, n_features=64)),
        ("fastUCBGallery", lambda: __import__("ibo_amd.acquisition.gallery", fromlist=["x"]).fastUCBGallery(GP, b, 2)),
        ("handle", lambda: GP._handle()),
    ]
    for word, call in refused:
        with pytest.raises(NotImplementedError, match=word):
            call()
    for a, bb in zip(GP.posteriors(Q), before):
        assert same_bits(a, bb)
    # a matrix without a factor (see the ABI test): NotPositiveDefinite with the pivot in its message, and the model as it was
    Xd = np.array(X[:5]); Xd[1] = Xd[0]
    Yd, Gd = gr.objective(Xd)
    with pytest.raises(NotPositiveDefinite, match="pivot"):
        GaussianProcess(make_kernel("iso", [0.6]), Xd, Yd, noise=0.0, gnoise=0.0, G=Gd)
    ok = GaussianProcess(make_kernel("iso", [0.6]), Xd[[0, 2, 3]], Yd[[0, 2, 3]], noise=0.0, gnoise=0.0, G=Gd[[0, 2, 3]])
    keep = ok.posteriors(Q)
    with pytest.raises(np.linalg.LinAlgError):
        ok.addData(Xd[1], Yd[1], Gd[1])                                # the first point again
    assert len(ok.X) == 3 and ok.G.shape == (3, 3)
    for a, bb in zip(ok.posteriors(Q), keep):
        assert same_bits(a, bb)

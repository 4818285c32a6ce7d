"""
ibo_sgp_* -- the sparse GP on inducing points (DTC / FITC) -- and what is built on it: SparseGaussianProcess, EI / PI / UCB,
acquisition.sweep and maximizeEI / PI / UCB on such a model.

The yardstick is tests/sparse_reference.py (pinned by tests/test_sparse_reference.py), in long double up to 400 inducing rows and the
whitened float64 form above.  Bars (derived beside the reference):
    K~uu       1e-12 relative (the library's exp: kstar_reference.bar_lib is below it for every case here)
    lambda     1e-12 relative + the q-bar f_U (1 + j + q)
    G, b, yy   ((N + 8) 2^-53 + 2 eps_k) sum_i |F_ai F_bi| against the reference's sums FROM THE DEVICE'S lambda
    ll, tt     (N + 8) 2^-53 sum |terms| + what lambda's bar moves them by
    A          exactly symmetric; |L_A L_A^T - A| <= 4 m 2^-53 max A_ii
    mu, s2, NLML   1e-15 max(cond_2(A), cond_2(K~uu), 1e6) x the terms' magnitudes
    EI/PI/UCB  1e-12 x max(1, |value|) against the epilogue restated on the device's own (mu, s2); 1e-6 relative end to end
    chunks, entries, sweep against batch, DIRECT against the host driver: bit for bit where the header says so
"""
import ctypes

import numpy as np
import pytest

import sparse_reference as sr

pytestmark = pytest.mark.gpu
GUARD = 7.25
GET = dict(Kuu=0, G=1, A=2, Lu=3, LA=4, b=5, alpha=6, yy=7, ll=8, tt=9, N=10)


@pytest.fixture(scope="module")
def lib():
    from ibo_amd import _lib
    if _lib.device_count() < 1:
        pytest.fail("no GPU visible: the product has no CPU fallback")
    return _lib


class Handle(object):
    """an ibo_sgp_t driven through the raw ABI"""

    def __init__(self):
        from ibo_amd import _lib
        self.lib = _lib
        self.h = ctypes.c_void_p()
        _lib.check(_lib.lib.ibo_sgp_create(_lib.default_device(), ctypes.byref(self.h)))
        self.info = ctypes.c_int(-1)
        self.lam = None

    def fit_rc(self, kern, Z, X, Y, noise, jitter, method):
        L = self.lib
        ktype, hyper, sf2 = sr.device_spec(kern)
        self.m, self.D = np.atleast_2d(Z).shape
        lam = np.full(len(X) + 8, GUARD)
        rc = L.lib.ibo_sgp_fit(self.h, ktype, self.D, L.dp(hyper), len(hyper), sf2, float(noise), float(jitter), int(method), self.m, L.dp(L.f64(Z)),
                               len(X), L.dp(L.f64(X)), L.dp(L.f64(Y)), L.dp(lam), ctypes.byref(self.info))
        if rc == L.OK:
            assert np.all(lam[len(X):] == GUARD)
            self.lam = lam[:len(X)].copy()
        return rc

    def fit(self, *a):
        self.lib.check(self.fit_rc(*a))
        return self

    def fit_case(self, c, method=None):
        return self.fit(c["kern"], c["Z"], c["X"], c["Y"], c["noise"], c["jitter"], c["method"] if method is None else method)

    def add_rc(self, X, Y):
        L = self.lib
        lam = np.empty(len(X))
        rc = L.lib.ibo_sgp_add(self.h, len(X), L.dp(L.f64(X)), L.dp(L.f64(Y)), L.dp(lam), ctypes.byref(self.info))
        if rc == L.OK:
            self.lam = np.r_[self.lam, lam]
        return rc

    def get(self, name):
        m = self.m
        n = m * m if GET[name] <= 4 else (m if GET[name] <= 6 else 1)
        out = np.full(n + 8, GUARD)
        self.lib.check(self.lib.lib.ibo_sgp_get(self.h, GET[name], self.lib.dp(out)))
        assert np.all(out[n:] == GUARD)
        return out[:n].reshape(m, m) if GET[name] <= 4 else (out[:n].copy() if GET[name] <= 6 else float(out[0]))

    def state(self):
        """everything the fit leaves behind, for bit comparisons"""
        return {k: self.get(k) for k in GET}

    def nlml(self, kind=0):
        v = ctypes.c_double()
        self.lib.check(self.lib.lib.ibo_sgp_nlml(self.h, kind, ctypes.byref(v)))
        return v.value

    def batch(self, Q, acq=sr.ACQ_NONE, parm=0.0, erf_mode=sr.ERF_LIBM, clamp=sr.CLAMP_PY, ymax=float("nan"), want=("mu", "s2", "acq")):
        L = self.lib
        Q = L.f64(np.atleast_2d(Q))
        M = len(Q)
        out = {k: np.full(M + 8, GUARD) for k in want}
        ptr = lambda k: L.dp(out[k]) if k in out else None
        L.check(L.lib.ibo_sgp_acq_batch(self.h, M, L.dp(Q), acq, float(parm), erf_mode, clamp, float(ymax), ptr("mu"), ptr("s2"), ptr("acq")))
        for k in out:
            assert np.all(out[k][M:] == GUARD), "guard behind %s overwritten" % k
            out[k] = out[k][:M]
        return out

    def sweep(self, cand, M, acq, parm=0.0, erf_mode=sr.ERF_LIBM, clamp=sr.CLAMP_PY, ymax=float("nan"), index_base=0, excl=None, radius=0.0):
        L = self.lib
        dev = L.default_device()
        outs = {k: L.DeviceArray((M + 8,), dev) for k in ("mu", "s2", "acq")}
        for v in outs.values():
            v.upload(np.full(M + 8, GUARD))
        bv = ctypes.c_double(); bi = ctypes.c_int64()
        ex = None if excl is None else L.f64(np.atleast_2d(excl))
        L.check(L.lib.ibo_sgp_acq_sweep(self.h, M, cand.ptr, acq, float(parm), erf_mode, clamp, float(ymax), 0 if ex is None else len(ex),
                                        None if ex is None else L.dp(ex), float(radius), int(index_base),
                                        outs["mu"].ptr, outs["s2"].ptr, outs["acq"].ptr, ctypes.byref(bv), ctypes.byref(bi)))
        res = dict(best_val=bv.value, best_idx=bi.value)
        for k, v in outs.items():
            a = v.to_host()
            assert np.all(a[M:] == GUARD), "guard behind the sweep's %s overwritten" % k
            res[k] = a[:M]
        return res

    def close(self):
        if getattr(self, "h", None):
            try:
                self.lib.lib.ibo_sgp_destroy(self.h)
            except Exception:                                    # (interpreter shutdown: the module is gone)
                pass
            self.h = None

    def __del__(self):
        self.close()


_HANDLES = {}


def fitted(name):
    """one fitted handle per case and session"""
    if name not in _HANDLES:
        _HANDLES[name] = Handle().fit_case(sr.case(name))
    return _HANDLES[name]


def reference(name):
    """the yardstick model of a case: long double up to LD_MAX_M inducing rows"""
    return sr.case_model(name, sr.case(name)["m"] <= sr.LD_MAX_M)


def f64(a):
    return np.asarray(a, dtype=np.float64)


def option(lib, key, value):
    lib.check(lib.lib.ibo_set_option(key, value))


# ---------------------------------------------------------------------------- the pieces of the fit
@pytest.mark.parametrize("name", sr.CASE_NAMES)
def test_the_pieces_of_the_fit_meet_their_bars(lib, name):
    c, ref, h = sr.case(name), reference(name), fitted(name)
    N, m = c["N"], c["m"]
    Kuu = h.get("Kuu")
    assert np.max(np.abs(Kuu - f64(ref["Kuu"]))) <= 1e-12 * max(1.0, c["kern"].sf2_py)
    # lambda: 1e-12 relative + the q-bar
    q = f64(ref["q"])
    fU = 1e-15 * max(ref["condU"], 1e6)
    lam_ref = f64(ref["lam"])
    lam_bar = 1e-12 * lam_ref + (fU * (1.0 + c["jitter"] + q) if c["method"] == sr.FITC else 0.0)
    print("%s: lambda worst ratio %.3g" % (name, np.max(np.abs(h.lam - lam_ref) / lam_bar)))
    assert np.all(np.abs(h.lam - lam_ref) <= lam_bar)
    # G, b, yy against long-double sums from the device's own lambda
    G, b, yy, aG, ab = sr.gram(c["kern"], c["Z"], c["X"], c["Y"], h.lam, sr.LD)
    dG, db, dyy = h.get("G"), h.get("b"), h.get("yy")
    barG = sr.gram_bar(c["kern"], c["Z"], c["X"], N, aG)
    print("%s: G worst ratio %.3g, b %.3g" % (name, np.max(np.abs(dG - f64(G)) / barG),
                                             np.max(np.abs(db - f64(b)) / sr.gram_bar(c["kern"], c["Z"], c["X"], N, ab))))
    assert np.array_equal(dG, dG.T)
    assert np.all(np.abs(f64(dG - G)) <= barG)
    assert np.all(np.abs(f64(db - b)) <= sr.gram_bar(c["kern"], c["Z"], c["X"], N, ab))
    assert abs(float(dyy - yy)) <= (N + 8) * sr.U * float(yy)
    # ll and tt: their own summation error plus what lambda's bar moves them by
    ll_bar = (N + 8) * sr.U * float(np.sum(np.abs(np.log(lam_ref)))) + float(np.sum(lam_bar / lam_ref)) + 4 * sr.U * N
    assert abs(h.get("ll") - float(ref["ll"])) <= ll_bar
    assert abs(h.get("tt") - float(ref["tt"])) <= (N + 8) * sr.U * float(ref["tt"]) + float(np.sum(fU * (1.0 + c["jitter"] + q)))
    assert h.get("N") == N
    # A: symmetric bit for bit, the sum of the two device matrices, and factored to the backward-error bound
    A, LA = h.get("A"), h.get("LA")
    assert np.array_equal(A, A.T) and np.array_equal(A, Kuu + dG)
    assert np.max(np.abs(LA @ LA.T - A)) <= 4 * m * sr.U * np.max(np.diag(A))
    Lu = h.get("Lu")
    assert np.max(np.abs(Lu @ Lu.T - Kuu)) <= 4 * m * sr.U * np.max(np.diag(Kuu))


@pytest.mark.parametrize("name", sr.CASE_NAMES + sr.ROUTE_NAMES)
def test_posterior_and_marginal_likelihoods_meet_the_bars(lib, name):
    c, ref, h = sr.case(name), reference(name), fitted(name)
    p = sr.posterior(ref, c["Q"], clamp_lo=-1.0)
    if c["m"] > sr.LD_MAX_M:                                   # the whitened float64 form is the comparator of the route cases
        w = sr.whitened(c["kern"], c["Z"], c["X"], c["Y"], c["noise"], c["jitter"], c["method"], c["Q"])
        want_mu, want_s2, want_nl = w["mu"], w["s2_raw"], w["nlml"]
    else:
        want_mu, want_s2, want_nl = p["mu"], p["s2_raw"], ref["nlml"]
    bmu, bs2, bnl = sr.bars(ref, p)
    for M in sr.QUERY_COUNTS:
        got = h.batch(c["Q"][:M], clamp=-1.0, want=("mu", "s2"))
        assert np.all(np.abs(got["mu"] - f64(want_mu)[:M]) <= bmu[:M]), name
        assert np.all(np.abs(got["s2"] - f64(want_s2)[:M]) <= bs2[:M]), name
    full = h.batch(c["Q"], clamp=-1.0, want=("mu", "s2"))
    print("%s: mu worst ratio %.3g, s2 %.3g, nlml %.3g" % (name, np.max(np.abs(full["mu"] - f64(want_mu)) / bmu),
                                                           np.max(np.abs(full["s2"] - f64(want_s2)) / bs2), abs(h.nlml(0) - float(want_nl)) / bnl))
    clipped = h.batch(c["Q"], clamp=sr.CLAMP_PY, want=("s2",))["s2"]
    assert np.array_equal(clipped, np.clip(full["s2"], sr.CLAMP_PY, 10.0))          # the clip comes AFTER the composition
    assert abs(h.nlml(0) - float(want_nl)) <= bnl
    if c["method"] == sr.DTC:
        assert abs(h.nlml(1) - float(ref["vfe"])) <= bnl and h.nlml(1) >= h.nlml(0)
    else:
        v = ctypes.c_double()
        assert lib.lib.ibo_sgp_nlml(h.h, 1, ctypes.byref(v)) == lib.ERR_ARG


@pytest.mark.parametrize("name", ["m16_n200", "m65_n1000", "m130_n2100"])
def test_the_third_marginal_likelihood_of_a_case_fitted_the_other_way(lib, name):
    c = sr.case(name)
    other = sr.DTC if c["method"] == sr.FITC else sr.FITC
    ref = sr.route(c["kern"], c["Z"], c["X"], c["Y"], c["noise"], c["jitter"], other, longdouble=True)
    h = Handle().fit_case(c, method=other)
    bnl = ref["f"] * ref["nlml_scale"]
    assert abs(h.nlml(0) - float(ref["nlml"])) <= bnl
    if other == sr.DTC:
        assert abs(h.nlml(1) - float(ref["vfe"])) <= bnl
    h.close()


@pytest.mark.parametrize("name", ["m16_n200", "m65_n1000", "m40_n500_sf2"])
def test_acquisitions_in_both_erf_flavours(lib, name):
    c, ref, h = sr.case(name), reference(name), fitted(name)
    pr = sr.posterior(ref, c["Q"], clamp_lo=sr.CLAMP_PY)
    ymax = float(np.max(c["Y"]))
    for acq, parm in ((sr.ACQ_EI, 0.01), (sr.ACQ_PI, 0.01), (sr.ACQ_UCB, 1.7)):
        for erf_mode in (sr.ERF_LIBM, sr.ERF_NR):
            got = h.batch(c["Q"], acq, parm, erf_mode)
            own = sr.acquisition(acq, erf_mode, got["mu"], got["s2"], ymax, parm)
            assert np.all(np.abs(got["acq"] - own) <= 1e-12 * np.maximum(1.0, np.abs(own)))
            want = sr.acquisition(acq, erf_mode, f64(pr["mu"]), f64(pr["s2"]), ymax, parm)
            assert np.all(np.abs(got["acq"] - want) <= 1e-6 * np.abs(want) + 1e-12)
    assert np.array_equal(h.batch(c["Q"], sr.ACQ_EI, 0.01, ymax=ymax)["acq"], h.batch(c["Q"], sr.ACQ_EI, 0.01)["acq"])     # ymax NaN: max(Y)


# ---------------------------------------------------------------------------- chunks and entries: bit for bit
def _big(method):
    rng = np.random.RandomState(77)
    N, m, D = 9000, 65, 3
    X = rng.rand(N, D)
    return sr.orc.Kern("ard", [0.5, 0.7, 0.6]), rng.rand(m, D), X, sr.objective(X) + 0.2 * rng.randn(N), 0.05, 1e-6, method


@pytest.mark.parametrize("method,chunks", [(sr.DTC, (256, 512, 8192)), (sr.FITC, (256, 512, 4096))])
def test_the_kept_sums_do_not_depend_on_the_chunking(lib, method, chunks):
    args = _big(method)
    states = []
    try:
        for ch in chunks:
            option(lib, b"sgp_chunk", ch)
            h = Handle().fit(*args)
            states.append((h.state(), h.lam))
            h.close()
    finally:
        option(lib, b"sgp_chunk", 0)
    # dtc: G+ -- and with it A, its factor and alpha -- does not read q at all, so the largest chunk (another size class of the q sweep)
    # gives the same bits too; only tt, the sum of the sweep's own 1 - q_i, is held to the q-bar there
    first = states[0][0]
    fU = 1e-15 * max(np.linalg.cond(first["Kuu"]), 1e6)
    for (st, lam), ch in zip(states[1:], chunks[1:]):
        assert np.array_equal(lam, states[0][1])
        for k in GET:
            if k == "tt" and ch > 4096:
                assert abs(st[k] - first[k]) <= 2 * len(lam) * fU * (2.0 + args[5])
                continue
            assert np.array_equal(st[k], first[k]), "%s differs between chunkings" % k


def test_fit_in_chunks_and_add_in_parts_equal_the_one_chunk_fit(lib):
    c = sr.case("m65_n1000")
    X, Y = c["X"][:600], c["Y"][:600]
    args = (c["kern"], c["Z"], X, Y, c["noise"], c["jitter"], sr.FITC)
    one = Handle().fit(*args)
    want = one.state()
    try:
        option(lib, b"sgp_chunk", 256)
        three = Handle().fit(*args)                              # three chunks, the last short
        got = three.state()
    finally:
        option(lib, b"sgp_chunk", 0)
    for k in GET:
        assert np.array_equal(got[k], want[k]), k
    added = Handle().fit(c["kern"], c["Z"], X[:256], Y[:256], c["noise"], c["jitter"], sr.FITC)
    lib.check(added.add_rc(X[256:], Y[256:]))
    got = added.state()
    for k in GET:
        assert np.array_equal(got[k], want[k]), k
    assert np.array_equal(added.lam, one.lam)
    # 100 + 500 rows: the Gram sums are cut at another place -- within the bars
    parts = Handle().fit(c["kern"], c["Z"], X[:100], Y[:100], c["noise"], c["jitter"], sr.FITC)
    lib.check(parts.add_rc(X[100:], Y[100:]))
    ref = sr.route(c["kern"], c["Z"], X, Y, c["noise"], c["jitter"], sr.FITC, longdouble=True)
    p = sr.posterior(ref, c["Q"])
    bmu, bs2, bnl = sr.bars(ref, p)
    a, b = one.batch(c["Q"], want=("mu", "s2")), parts.batch(c["Q"], want=("mu", "s2"))
    assert np.all(np.abs(a["mu"] - b["mu"]) <= bmu) and np.all(np.abs(a["s2"] - b["s2"]) <= bs2) and abs(one.nlml() - parts.nlml()) <= bnl
    assert np.all(np.abs(b["mu"] - f64(p["mu"])) <= bmu)
    for h in (one, three, added, parts):
        h.close()


@pytest.mark.parametrize("M", [1, 63, 64, 65, 300, 4097])
def test_the_sweep_is_the_batch_bit_for_bit(lib, M):
    c, h = sr.case("m65_n1000"), fitted("m65_n1000")
    Q = np.random.RandomState(M).rand(M, c["D"])
    cand = lib.DeviceArray.from_host(Q, lib.default_device())
    for acq, parm, erf_mode in ((sr.ACQ_EI, 0.01, sr.ERF_LIBM), (sr.ACQ_UCB, 1.3, sr.ERF_NR)):
        b = h.batch(Q, acq, parm, erf_mode)
        s = h.sweep(cand, M, acq, parm, erf_mode, index_base=1000)
        for k in ("mu", "s2", "acq"):
            assert np.array_equal(b[k], s[k]), k
        k = int(np.argmax(b["acq"]))
        assert s["best_idx"] == 1000 + k and s["best_val"] == b["acq"][k]


def test_the_arg_max_contract(lib):
    c, h = sr.case("m65_n1000"), fitted("m65_n1000")
    M = 700
    Q = np.random.RandomState(9).rand(M, c["D"])
    base = h.batch(Q, sr.ACQ_EI, 0.01)["acq"]
    k = int(np.argmax(base))
    j = 650 if k != 650 else 600
    Q[j] = Q[k]                                                 # duplicated winners: the first index wins
    first = min(k, j)
    Q[5 if first != 5 else 6] = np.nan                          # a NaN row never wins
    cand = lib.DeviceArray.from_host(Q, lib.default_device())
    s = h.sweep(cand, M, sr.ACQ_EI, 0.01, index_base=10 ** 10)
    assert np.isnan(s["acq"][5 if first != 5 else 6]) and s["best_idx"] == 10 ** 10 + first and s["best_val"] == s["acq"][first]
    # exclusion balls around the winner take out every copy of it
    e = h.sweep(cand, M, sr.ACQ_EI, 0.01, excl=Q[first][None, :], radius=1e-9)
    score = np.where(np.isnan(s["acq"]), -np.inf, s["acq"])
    score[[i for i in range(M) if np.array_equal(Q[i], Q[first])]] = -np.inf
    assert e["best_idx"] == int(np.argmax(score)) and e["best_val"] == score[e["best_idx"]]
    # nothing admissible: (-inf, -1)
    n = h.sweep(cand, M, sr.ACQ_EI, 0.01, excl=np.full((1, c["D"]), 0.5), radius=100.0)
    assert n["best_val"] == -np.inf and n["best_idx"] == -1


def test_direct_on_the_device_is_the_host_driver_on_the_batch(lib):
    c, h = sr.case("m64_n300_j8"), None
    rng = np.random.RandomState(4)
    X = rng.rand(200, 2)
    Y = sr.objective(X) + 0.1 * rng.randn(200)
    h = Handle().fit(sr.orc.Kern("ard", [0.4, 0.5]), rng.rand(30, 2), X, Y, 0.05, 1e-6, sr.FITC)
    lb, ub = lib.f64([0.0, 0.0]), lib.f64([1.0, 1.0])
    opt = ctypes.c_double(); optx = np.empty(2); ns = ctypes.c_int64()
    lib.check(lib.lib.ibo_sgp_direct_max(h.h, 2, lib.dp(lb), lib.dp(ub), sr.ACQ_EI, 0.01, sr.ERF_LIBM, sr.CLAMP_NATIVE, 10, 30, 10000, 1,
                                         ctypes.byref(opt), lib.dp(optx), ctypes.byref(ns)))
    cb = lib.OBJECTIVE(lambda n, x: -float(h.batch(np.array([x[i] for i in range(n)]), sr.ACQ_EI, 0.01, sr.ERF_LIBM, sr.CLAMP_NATIVE, want=("acq",))["acq"][0]))
    fm = ctypes.c_double(); xm = np.empty(2); n2 = ctypes.c_int64()
    lib.check(lib.lib.ibo_direct_host(cb, 2, lib.dp(lb), lib.dp(ub), 10, 30, 10000, 1, ctypes.byref(fm), lib.dp(xm), ctypes.byref(n2)))
    assert opt.value == -fm.value and np.array_equal(optx, xm) and ns.value == n2.value
    h.close()


# ---------------------------------------------------------------------------- Z = X against the device's own plain model
def test_z_equal_x_against_the_plain_model_on_the_device(lib):
    from ibo_amd.gaussianprocess import GaussianProcess, GaussianKernel_ard
    rng = np.random.RandomState(5)
    N, noise, j = 120, 0.05, 1e-6
    X = rng.rand(N, 2)
    Y = sr.objective(X) + np.sqrt(noise) * rng.randn(N)
    kern = sr.orc.Kern("ard", [0.5, 0.6])
    h = Handle().fit(kern, X, X, Y, noise, j, sr.FITC)
    got = h.batch(X, want=("mu", "s2"))
    mu, s2 = GaussianProcess(GaussianKernel_ard(np.array([0.5, 0.6])), X, Y, noise=noise).posteriors(X)
    ref = sr.route(kern, X, X, Y, noise, j, sr.FITC)
    p = sr.posterior(ref, X)
    bmu, bs2, _ = sr.bars(ref, p)
    dmu, ds2 = sr.zx_bound(kern, X, Y, noise, j)
    plain_f = 1e-15 * max(np.linalg.cond(sr.kuu(kern, X, noise)), 1e6)       # the plain model's own bars
    assert np.all(np.abs(got["mu"] - mu) <= dmu + bmu + plain_f * p["mu_scale"])
    assert np.all(np.abs(got["s2"] - s2) <= ds2 + bs2 + plain_f * p["s2_scale"])
    h.close()


# ---------------------------------------------------------------------------- errors and the life of a handle
def test_errors_and_a_refitted_handle(lib):
    c = sr.case("m16_n200")
    kern, Z, X, Y = c["kern"], c["Z"], c["X"], c["Y"]
    h = Handle()
    q = np.zeros((1, c["D"])); out = np.zeros(1)
    assert lib.lib.ibo_sgp_acq_batch(h.h, 1, lib.dp(q), 3, 0.0, 0, 1e-8, float("nan"), lib.dp(out), None, None) == lib.ERR_STATE
    bad = X.copy(); bad[7, 1] = np.inf
    assert h.fit_rc(kern, Z, bad, Y, 0.05, 1e-6, sr.FITC) == lib.ERR_ARG
    badz = Z.copy(); badz[0, 0] = np.nan
    assert h.fit_rc(kern, badz, X, Y, 0.05, 1e-6, sr.FITC) == lib.ERR_ARG
    bady = Y.copy(); bady[3] = np.nan
    assert h.fit_rc(kern, Z, X, bady, 0.05, 1e-6, sr.FITC) == lib.ERR_ARG
    assert h.fit_rc(kern, Z, X, Y, 0.0, 1e-6, sr.FITC) == lib.ERR_ARG and h.fit_rc(kern, Z, X, Y, 0.05, -1e-9, sr.FITC) == lib.ERR_ARG
    assert h.fit_rc(kern, Z, X, Y, 0.05, 1e-6, 2) == lib.ERR_ARG
    # one handle through m = 65, 1, 130, a failed fit and 64: each equals a fresh handle bit for bit
    rng = np.random.RandomState(12)
    for m in (65, 1, 130, -1, 64):
        if m < 0:
            dup = Z[:6].copy(); dup[1] = dup[0]                  # coincident inducing points, no jitter: the second pivot is 1 - 1 = 0 exactly
            assert h.fit_rc(kern, dup, X, Y, 0.05, 0.0, sr.FITC) == lib.ERR_NOT_PD
            assert b"K~uu" in lib.lib.ibo_last_error() and h.info.value == 2
            assert lib.lib.ibo_sgp_acq_batch(h.h, 1, lib.dp(q), 3, 0.0, 0, 1e-8, float("nan"), lib.dp(out), None, None) == lib.ERR_STATE
            continue
        Zm = rng.rand(m, c["D"])
        lib.check(h.fit_rc(kern, Zm, X, Y, 0.05, 1e-6, sr.FITC))
        fresh = Handle().fit(kern, Zm, X, Y, 0.05, 1e-6, sr.FITC)
        a, b = h.state(), fresh.state()
        for k in GET:
            assert np.array_equal(a[k], b[k]), (m, k)
        assert np.array_equal(h.batch(c["Q"])["mu"], fresh.batch(c["Q"])["mu"]) and h.nlml() == fresh.nlml()
        fresh.close()
    assert h.add_rc(bad[:10], Y[:10]) == lib.ERR_ARG
    lib.check(h.add_rc(X[:10], Y[:10]))                          # (a refused argument left the model fitted)
    h.close()


# ---------------------------------------------------------------------------- the Python layer
def test_the_python_layer(lib):
    from ibo_amd.gaussianprocess import SparseGaussianProcess, inducingPoints, GaussianKernel_ard
    from ibo_amd import acquisition as aq
    from ibo_amd.acquisition import constrained, gallery, multiobjective
    c = sr.case("m16_n200")
    k = GaussianKernel_ard(np.array(c["hyper"]))
    g = SparseGaussianProcess(k, c["X"], c["Y"], Z=c["Z"], noise=c["noise"], jitter=c["jitter"])
    ref = reference("m16_n200")
    p = sr.posterior(ref, c["Q"])
    bmu, bs2, bnl = sr.bars(ref, p)
    mu, s2 = g.posteriors(c["Q"])
    assert np.all(np.abs(mu - f64(p["mu"])) <= bmu) and np.all(np.abs(s2 - f64(p["s2"])) <= bs2)
    m0, v0 = g.posterior(c["Q"][0])
    assert m0 == mu[0] or abs(m0 - mu[0]) <= bmu[0]
    assert g.mu(c["Q"][0]) == -g.negmu(c["Q"][0]) and abs(g.nlml() - float(ref["nlml"])) <= bnl and g.nlml("fitc") == g.nlml()
    with pytest.raises(ValueError):
        g.nlml("vfe")
    assert np.array_equal(g._get("G"), fitted("m16_n200").get("G"))
    # the acquisition classes, the sweep and the maximisers
    ei = aq.EI(g)
    vals = ei.values(c["Q"])
    assert ei.f(c["Q"][3]) == -ei.negf(c["Q"][3]) and abs(ei.f(c["Q"][3]) - vals[3]) <= 1e-12
    assert np.isfinite(aq.PI(g).f(c["Q"][3])) and np.isfinite(aq.UCB(g, c["D"]).f(c["Q"][3]))
    r = aq.sweep(g, c["Q"], 'ei', native=False, outputs=("acq", "mu", "s2"), index_base=7)
    assert np.array_equal(r["acq"], vals) and r["best_idx"] == 7 + int(np.argmax(vals)) and np.array_equal(r["mu"], mu)
    r2 = aq.sweep(g, c["Q"], 'ei', native=False, exclude=[c["Q"][int(np.argmax(vals))]], exclude_radius=1e-9)
    assert r2["best_idx"] != r["best_idx"] - 7
    bounds = [[0.0, 1.0]] * c["D"]
    for fn in (aq.maximizeEI, aq.maximizePI, aq.maximizeUCB):
        opt, optx = fn(g, bounds, maxiter=5)
        assert np.isfinite(opt) and np.all((optx >= 0) & (optx <= 1))
    # refusals name the call
    for what, call in (("removeData", lambda: g.removeData([0])), ("posterior_gradient", lambda: g.posterior_gradient(c["Q"])),
                       ("gradient", lambda: ei.gradient(c["Q"])), ("gradient", lambda: ei.negf_grad(c["Q"][0])),
                       ("polish", lambda: aq.maximizeEI(g, bounds, polish=True)), ("posterior_cov", lambda: g.posterior_cov(c["Q"])),
                       ("sample_posterior", lambda: g.sample_posterior(c["Q"])), ("loo", lambda: g.loo()), ("loo_score", lambda: g.loo_score()),
                       ("incremental", lambda: aq.sweep(g, c["Q"], incremental=True)), ("exchange", lambda: aq.sweep(g, c["Q"], exchange=object())),
                       ("knowledge gradient", lambda: aq.sweepKG(g, c["Q"], c["Q"][:4])), ("parallel expected improvement", lambda: aq.sweepQEI(g, c["Q"])),
                       ("sweepConstrained", lambda: constrained.sweepConstrained(g, [], c["Q"])),
                       ("hypervolume", lambda: multiobjective.sweepEHVI([g, g], c["Q"], [0.0, 0.0])),
                       ("entropy", lambda: aq.sweepMES(g, c["Q"], np.array([1.0]))), ("PosteriorPaths", lambda: aq.PosteriorPaths(g, 2, seed=1)),
                       ("fastUCBGallery", lambda: gallery.fastUCBGallery(g, bounds, 2))):
        with pytest.raises(NotImplementedError, match=what):
            call()
    # addData accumulates; m= with both selection methods is reproducible
    g2 = SparseGaussianProcess(k, c["X"][:120], c["Y"][:120], Z=c["Z"], noise=c["noise"], jitter=c["jitter"])
    g2.addData(c["X"][120:], c["Y"][120:])
    mu2, s22 = g2.posteriors(c["Q"])
    assert len(g2.Y) == c["N"] and np.all(np.abs(mu2 - mu) <= bmu) and np.all(np.abs(s22 - s2) <= bs2)
    for sel in ("subset", "kcenter"):
        a = SparseGaussianProcess(k, c["X"], c["Y"], m=12, noise=c["noise"], seed=3, selection=sel)
        b = SparseGaussianProcess(k, c["X"], c["Y"], m=12, noise=c["noise"], seed=3, selection=sel)
        assert np.array_equal(a.Z, b.Z) and np.array_equal(a.Z, inducingPoints(c["X"], 12, sel, 3)) and np.array_equal(a.posteriors(c["Q"])[0], b.posteriors(c["Q"])[0])
        a.close(); b.close()
    # a matrix that does not factor leaves the previous model answering with its earlier bits
    before = g.posteriors(c["Q"])[0]
    with pytest.raises(lib.NotPositiveDefinite, match="K~uu"):
        g.jitter = 0.0
        g.refit(Z=np.r_[c["Z"][:1], c["Z"][:5]])
    g.jitter = c["jitter"]
    assert np.array_equal(g.posteriors(c["Q"])[0], before) and np.array_equal(g.Z, c["Z"])
    with pytest.raises(ValueError):
        g.addData(np.full((1, c["D"]), np.nan), [0.0])
    g.close(); g2.close()


def test_streaming_forty_chunks_is_one_fit_within_the_bars(lib):
    rng = np.random.RandomState(21)
    N, m, D, noise = 20000, 64, 4, 0.05
    X = rng.rand(N, D)
    Y = sr.objective(X) + np.sqrt(noise) * rng.randn(N)
    Z = rng.rand(m, D)
    kern = sr.orc.Kern("ard", [0.6, 0.8, 0.7, 0.9])
    Q = rng.rand(130, D)
    one = Handle().fit(kern, Z, X, Y, noise, 1e-6, sr.FITC)
    h = Handle().fit(kern, Z, X[:500], Y[:500], noise, 1e-6, sr.FITC)
    for i in range(1, 40):
        lib.check(h.add_rc(X[500 * i:500 * (i + 1)], Y[500 * i:500 * (i + 1)]))
    ref = sr.route(kern, Z, X, Y, noise, 1e-6, sr.FITC)
    p = sr.posterior(ref, Q)
    w = sr.whitened(kern, Z, X, Y, noise, 1e-6, sr.FITC, Q)
    bmu, bs2, bnl = sr.bars(ref, p)
    for hh in (one, h):
        got = hh.batch(Q, want=("mu", "s2"))
        assert np.all(np.abs(got["mu"] - w["mu"]) <= bmu) and np.all(np.abs(got["s2"] - np.clip(w["s2_raw"], sr.CLAMP_PY, 10)) <= bs2)
        assert abs(hh.nlml() - w["nlml"]) <= bnl and hh.get("N") == N
    one.close(); h.close()

"""
The k* probe on the device ("the k* probe"; reference, grids and bars: tests/kstar_reference.py, checked on the CPU by
tests/test_kstar_reference.py).

The one-row model X = 0, Y = 4, noise = 3 has L = 2, W = 1/2 and alphaY = 1 exactly, so the mean a sweep returns is the bits of the k*
its kernel generated and s2 = 4 - mu^2 / 4.  Every sweep route, ibo_acq_batch and the library-exp entries are held to the mpmath truth
at bars of order 1e-15 (1 + |y|) over grids that visit every entry of s2_exp's table at the centre and both ends of its reduction
interval, positive exponents, the run down to underflow, exp_fast's clamp and the candidate pull-in; N = 64 / 65 / 129 models with
alphaY = e_i hold every fragment position; the acquisition epilogue is held to 8 eps (|ydiff| + sigma) over z = -40 .. 40.
Each test prints the worst ratio to its bar ("RATIO ..." lines).  Run on the MI355X box with `pytest -m gpu`.

Where c = x gives exactly sf2: everywhere except the squared exponential with sf2 != 1 on the hand-written routines, where log sf2
rides in the exponent (exp(log sf2) is sf2 only to the bar).  Beyond the pull-in radius k* is exactly 0 on the routes that stage their
candidates through s2_stage_candidates (small2.hip's kernels, sweep2_kernel, the kept state); the first-generation kernels' dot form
has no pull-in and answers exp_fast's clamp, which the underflow condition covers.
"""
from ctypes import byref, c_char_p, c_double, c_float, c_int, c_int64, c_void_p

import numpy as np
import pytest

import kstar_reference as kr

pytestmark = pytest.mark.gpu
LD = np.longdouble
NAN = float("nan")
CLAMP = 1e-8
FAM = {"ard": kr.SE, "iso": kr.SE, "sv": kr.SE, "m3": kr.M3, "m5": kr.M5}
KTYPE = {"ard": 0, "iso": 1, "sv": 1, "m3": 2, "m5": 3}
VARIANTS = [("ard", 1.0), ("iso", 1.0), ("sv", 1e-6), ("sv", 1e6), ("m3", 1.0), ("m3", 1e-6), ("m3", 1e6), ("m5", 1.0), ("m5", 1e-6), ("m5", 1e6)]
DOT_D = (1, 4, 5, 16, 17, 32)
DIFF_D = (1, 5, 17, 33, 64)
# route: option values, how the candidates are cut into calls, the kernel ibo_last_sweep_kernel_ms must name, the routine behind k*
ROUTES = {
    "small2":        dict(path=0, dot=-1, chunk=4096, kernel="wk_small_kernel", routine="s2", dims=DOT_D),
    "small2-local":  dict(path=0, dot=-1, chunk=128, kernel="wk_small_kernel", routine="s2", dims=(1, 4, 5), thin=True),       # wkl_small_kernel: <= 128 candidates, D <= 10
    "sweep2":        dict(path=0, dot=-1, sizes=True, kernel="sweep2_kernel", routine="s2", dims=DOT_D),                      # 12288 and 8193 candidates
    "sweep2-forced": dict(path=2, dot=1, chunk=4000, kernel="sweep2_kernel", routine="s2", dims=(4, 17)),
    "kept":          dict(path=0, dot=-1, sizes=True, kernel="sweep2_kernel", routine="s2", dims=DOT_D, reserve=511, incremental=True),
    "gemv":          dict(path=1, dot=-1, chunk=4096, kernel="sweep_gemv_kernel", routine="lib", dims=DIFF_D),
    "tile-diff":     dict(path=2, dot=0, chunk=12288, kernel="sweep_mfma_kernel", routine="fast", dims=DIFF_D),
    "split-dot":     dict(path=3, dot=1, chunk=4096, kernel="sweep_mfma_kernel<split>", routine="fast", dims=DOT_D),
    "split-diff":    dict(path=3, dot=0, chunk=4096, kernel="sweep_mfma_kernel<split>", routine="fast", dims=DIFF_D),
    "batch":         dict(path=0, dot=-1, chunk=4096, kernel="wk_small_kernel", routine="s2", dims=(1, 5, 32), host=True),
}


@pytest.fixture(scope="module")
def L():
    from ibo_amd import _lib
    if _lib.device_count() < 1:
        pytest.fail("no GPU visible: the product has no CPU fallback")
    err = c_double()
    _lib.check(_lib.lib.ibo_selftest_mfma(0, byref(err)))
    return _lib


class Options(object):
    """sweep_path / dot_form for the length of a with-block; restored whatever happens"""

    def __init__(self, L, path, dot):
        self.L, self.path, self.dot = L, path, dot

    def __enter__(self):
        self.L.check(self.L.lib.ibo_set_option(b"sweep_path", self.path)); self.L.check(self.L.lib.ibo_set_option(b"dot_form", self.dot))

    def __exit__(self, *exc):
        self.L.check(self.L.lib.ibo_set_option(b"sweep_path", 0)); self.L.check(self.L.lib.ibo_set_option(b"dot_form", -1))


class Model(object):
    """a handle fitted through the C ABI"""

    def __init__(self, L, kind, D, ell, sf2, X, Y, noise, reserve=0):
        self.L, self.D, self.N = L, D, len(Y)
        self.dev = L.default_device()
        self.h = c_void_p()
        L.check(L.lib.ibo_gp_create(self.dev, byref(self.h)))
        if reserve:
            L.check(L.lib.ibo_gp_reserve(self.h, reserve))
        X = L.f64(np.reshape(X, (self.N, D))); Y = L.f64(Y)
        hyper = L.f64(np.broadcast_to(ell, (D,)) if kind == "ard" else np.atleast_1d(ell)[:1])
        info = c_int(0)
        L.check(L.lib.ibo_gp_fit(self.h, KTYPE[kind], self.N, D, L.dp(X), L.dp(Y), L.dp(hyper), len(hyper), float(sf2), float(noise), byref(info)))

    def close(self):
        if self.h:
            self.L.lib.ibo_gp_destroy(self.h)
            self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def matrix(self, which):
        out = np.empty((self.N, self.N))
        self.L.check(getattr(self.L.lib, "ibo_gp_get_" + which)(self.h, self.L.dp(out)))
        return out

    def set_y(self, Y):
        Y = self.L.f64(Y)
        self.L.check(self.L.lib.ibo_gp_set_y(self.h, self.L.dp(Y)))

    def kernel(self):
        ms, nm = c_float(), c_char_p()
        self.L.check(self.L.lib.ibo_last_sweep_kernel_ms(self.h, byref(ms), byref(nm)))
        return nm.value.decode()

    def sweep(self, C, acq=3, parm=0.0, erf=0, ymax=NAN, incremental=False, dc=None):
        """ibo_acq_sweep(_incremental) with outputs -> (mu, s2, acq, kernel name)"""
        from ibo_amd import DeviceArray
        M = len(C)
        dc = DeviceArray.from_host(C) if dc is None else dc
        out = [DeviceArray((M,)) for _ in range(3)]
        bv, bi = c_double(), c_int64()
        f = self.L.lib.ibo_acq_sweep_incremental if incremental else self.L.lib.ibo_acq_sweep
        self.L.check(f(self.h, M, dc.ptr, acq, parm, erf, CLAMP, ymax, 0, None, 0.0, 0, out[0].ptr, out[1].ptr, out[2].ptr, byref(bv), byref(bi)))
        r = [o.to_host() for o in out]
        for o in out:
            o.free()
        return r[0], r[1], r[2], self.kernel()

    def batch(self, Q, acq=3, parm=0.0, erf=0, ymax=NAN):
        """ibo_acq_batch on host points -> (mu, s2, acq, kernel name)"""
        Q = self.L.f64(Q); M = len(Q)
        mu, s2, av = np.empty(M), np.empty(M), np.empty(M)
        self.L.check(self.L.lib.ibo_acq_batch(self.h, M, self.L.dp(Q), acq, parm, erf, CLAMP, ymax, self.L.dp(mu), self.L.dp(s2), self.L.dp(av)))
        return mu, s2, av, self.kernel()


def probe_model(L, kind, D, sf2, reserve=0):
    ell = kr.probe_length_scales("ard" if kind == "ard" else "iso", D)
    return Model(L, kind, D, ell, sf2, np.zeros((1, D)), [kr.PROBE_Y], kr.PROBE_NOISE, reserve=reserve)


def run_route(m, route, C):
    """mu and s2 of every row of C through one route, in as many calls as its sizes ask for; the kernel name asserted after each"""
    r = ROUTES[route]
    M = len(C)
    mu, s2 = np.full(M, NAN), np.full(M, NAN)
    pos = 0
    while pos < M:
        if r.get("sizes"):
            size = 12288 if M - pos >= 12288 else 8193                   # sweep2_kernel's two sizes of the issue: short ends wrap around
        else:
            size = min(r["chunk"], M - pos)
        idx = (pos + np.arange(size)) % M
        take = min(size, M - pos)
        if r.get("host"):
            a, b, _, name = m.batch(C[idx])
        else:
            a, b, _, name = m.sweep(C[idx], incremental=r.get("incremental", False))
        assert name == r["kernel"], (route, size, name)
        mu[idx[:take]], s2[idx[:take]] = a[:take], b[:take]
        pos += take
    return mu, s2


def hold(tag, mu, s2, G, fam, sf2, routine):
    """the returned mean against the truth at the routine's bar, the variance against 4 - mu^2 / 4; prints the worst ratio"""
    lib = routine == "lib"
    want = G["m"] * LD(sf2)
    rel = kr.bar_lib(fam, G["z"], sf2) if lib else kr.bar_fast(fam, G["z"], sf2)
    bad, worst = kr.violations(mu, want, rel, fam, G["z"], sf2, lib=lib)
    print("RATIO %s: worst |mu - k*| / bar %.3f over %d candidates" % (tag, worst, len(mu)))
    assert len(bad) == 0, (tag, len(bad), G["y"][bad][:4], mu[bad][:4], want[bad][:4].astype(np.float64))
    assert not np.any(np.isnan(s2))
    d = np.abs(s2 - kr.probe_s2(mu, CLAMP))
    assert np.all(d <= kr.S2_ULPS), (tag, d.max())
    # c = x (the last grid point)
    at = mu[G["z"] == 0.0]
    if fam != kr.SE or sf2 == 1.0 or lib:
        assert len(at) and np.all(at == sf2), (tag, at)
    if routine == "s2":
        far = G["z"] > kr.PULL_IN
        assert far.sum() >= 3 and np.all(mu[far] == 0.0) and np.all(s2[far] == 1.0 + kr.PROBE_NOISE), (tag, mu[far])
    return worst


# ------------------------------------------------------------------------------------------------------------ 2. the pure probe
def test_probe_model_is_exact(L):
    for kind, sf2 in VARIANTS:
        with probe_model(L, kind, 3, sf2) as m:
            assert m.matrix("L")[0, 0] == kr.PROBE_L and m.matrix("W")[0, 0] == kr.PROBE_W and m.matrix("R")[0, 0] == 1.0 + kr.PROBE_NOISE
            mu, s2, _, _ = m.batch(np.zeros((1, 3)))
            assert mu[0] == sf2 or (FAM[kind] == kr.SE and sf2 != 1.0 and abs(mu[0] - sf2) <= 2e-14 * sf2)      # alphaY = 1


@pytest.mark.parametrize("route", list(ROUTES))
@pytest.mark.parametrize("kind,sf2", VARIANTS)
def test_kstar_of_every_route(L, kind, sf2, route):
    r = ROUTES[route]
    fam = FAM[kind]
    with Options(L, r["path"], r["dot"]):
        first = True
        for D in r["dims"]:
            G = kr.probe_grid(fam, D, "ard" if kind == "ard" else "iso", full=(D == r["dims"][0] and not r.get("thin")))
            with probe_model(L, kind, D, sf2, reserve=r.get("reserve", 0)) as m:
                mu, s2 = run_route(m, route, G["C"])
                hold("%s %s sf2=%g D=%d" % (route, kind, sf2, D), mu, s2, G, fam, sf2, r["routine"])
                if first:
                    # the same call again: the same bits (for the kept state this is its second visit: acq_finish_kernel on the state)
                    sub = G["C"][:8193] if r.get("sizes") else G["C"][:r["chunk"]]
                    a = m.batch(sub) if r.get("host") else m.sweep(sub, incremental=r.get("incremental", False))
                    b = m.batch(sub) if r.get("host") else m.sweep(sub, incremental=r.get("incremental", False))
                    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[0], mu[:len(sub)]), route
                    first = False


def test_kept_state_second_visit(L):
    """ibo_acq_sweep_incremental twice on ONE device array: the second call evaluates the kept state (acq_finish_kernel) and returns the first's bits"""
    from ibo_amd import DeviceArray
    G = kr.probe_grid(kr.SE, 4, "ard", full=True)
    with probe_model(L, "ard", 4, 1.0, reserve=511) as m:
        dc = DeviceArray.from_host(G["C"][:12288])
        a = m.sweep(G["C"][:12288], incremental=True, dc=dc)
        b = m.sweep(G["C"][:12288], incremental=True, dc=dc)
        assert a[3] == "sweep2_kernel" and b[3] == "acq_finish_kernel", (a[3], b[3])
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
        dc.free()


@pytest.mark.parametrize("kind,sf2", VARIANTS)
def test_rank1_refresh_regenerates_kstar(L, kind, sf2):
    """the kept state's rank-1 refresh has its own k* generation (sweep2_rank1_kernel re-forms the means from the current alpha vectors).
    The probe model is extended by one observation 200 length scales down the last axis with target 0: R = diag(4, 4) and alphaY = (1, 0) (to 1e-75),
    so the refreshed mean is again the bits of k*(0, c), now from that kernel; k* of the new row is 0 at every candidate (they lie at
    non-negative last coordinates) and meets a zero alpha anyway."""
    from ibo_amd import DeviceArray
    fam = FAM[kind]
    D = 4
    G = kr.probe_grid(fam, D, "ard" if kind == "ard" else "iso", full=True)
    C = G["C"][np.r_[np.arange(0, 12288 - 1484), np.arange(12288, len(G["C"]))]]       # 12288 candidates: most of the table grid and every other grid
    sub = dict((k, G[k][np.r_[np.arange(0, 12288 - 1484), np.arange(12288, len(G["C"]))]]) for k in ("y", "z", "m"))
    assert len(C) == 12288 and np.all(C[:, D - 1] >= 0)
    with probe_model(L, kind, D, sf2, reserve=511) as m:
        dc = DeviceArray.from_host(C)
        a = m.sweep(C, incremental=True, dc=dc)
        assert a[3] == "sweep2_kernel"
        ell = np.broadcast_to(G["ell"], (D,))
        xn = np.zeros((1, D)); xn[0, D - 1] = -100.0 * ell[D - 1]
        info = c_int(0)
        L.check(L.lib.ibo_gp_extend(m.h, 1, L.dp(L.f64(xn)), L.dp(L.f64([kr.PROBE_Y, 0.0])), byref(info)))
        m.N = 2
        R = m.matrix("R"); Lf = m.matrix("L")
        # (exactly diag(4, 4) for the squared exponential; the Matern kernels leave e^-173 = 1e-75 between the two rows, which moves nothing)
        assert np.array_equal(np.diag(R), [4.0, 4.0]) and np.array_equal(np.diag(Lf), [2.0, 2.0]) and abs(R[0, 1]) < 1e-60 and abs(Lf[1, 0]) < 1e-60
        b = m.sweep(C, incremental=True, dc=dc)
        assert b[3] == "sweep2_rank1_kernel", b[3]
        hold("rank1 %s sf2=%g D=%d" % (kind, sf2, D), b[0], b[1], sub, fam, sf2, "s2")
        assert np.array_equal(a[0], b[0])                                # the two kernels share s2_exp and the staging: the same bits
        dc.free()


# ------------------------------------------------------------------------------------------------------------ 2b. the library-exp entries
LIB_VARIANTS = [("ard", 1.0), ("sv", 1e6), ("m3", 1e-6), ("m5", 1.0)]


def _sample(G, n):
    """n grid points spread over every grid, the last ones (pull-in, c = x) always among them"""
    M = len(G["y"])
    return np.unique(np.r_[np.linspace(0, M - 1, n).astype(int), np.arange(M - 16, M)])


@pytest.mark.parametrize("kind,sf2", LIB_VARIANTS)
@pytest.mark.parametrize("D", [1, 5, 33])
def test_library_exp_entries(L, kind, sf2, D):
    """ibo_cov_matrix (cross and square), ibo_gp_get_R of the two-point model {0, c}, ibo_posterior_cov's mean and S_aa"""
    fam = FAM[kind]
    G = kr.probe_grid(fam, D, "ard" if kind == "ard" else "iso", full=(D == 1))
    ell = G["ell"]
    hyper = L.f64(np.broadcast_to(ell, (D,)) if kind == "ard" else ell[:1])
    dev = L.default_device()
    want = G["m"] * LD(sf2)
    tag = "%s sf2=%g D=%d" % (kind, sf2, D)

    def held(what, got, idx):
        sub = dict(y=G["y"][idx], z=G["z"][idx])
        bad, worst = kr.violations(got, want[idx], kr.bar_lib(fam, sub["z"], sf2), fam, sub["z"], sf2, lib=True)
        print("RATIO %s %s: worst / bar %.3f over %d" % (what, tag, worst, len(got)))
        assert len(bad) == 0, (what, tag, sub["y"][bad][:4], np.asarray(got)[bad][:4], want[idx][bad][:4].astype(np.float64))
        assert np.all(np.asarray(got)[sub["z"] == 0.0] == sf2)
    # cross-covariance K(C, {0}) of the whole grid
    M = len(G["C"])
    A1 = L.f64(G["C"]); A2 = L.f64(np.zeros((1, D))); K = np.empty((M, 1))
    L.check(L.lib.ibo_cov_matrix(dev, KTYPE[kind], D, L.dp(hyper), len(hyper), sf2, M, L.dp(A1), 1, L.dp(A2), 0, 0.0, L.dp(K)))
    held("ibo_cov_matrix cross", K[:, 0], np.arange(M))
    # the square form on {0} and 200 grid points: row and column 0
    idx = _sample(G, 200)
    A = L.f64(np.vstack([np.zeros((1, D)), G["C"][idx]])); n = len(A); Ks = np.empty((n, n))
    L.check(L.lib.ibo_cov_matrix(dev, KTYPE[kind], D, L.dp(hyper), len(hyper), sf2, n, L.dp(A), 0, None, L.DIAG_UNIT_PLUS_NOISE, 0.25, L.dp(Ks)))
    assert np.all(np.diag(Ks) == 1.25) and np.array_equal(Ks, Ks.T)
    held("ibo_cov_matrix square", Ks[0, 1:], idx)
    # ibo_gp_get_R of the two-point model {0, c}
    ok = np.flatnonzero((G["z"] > 0) & (want < 1.0) & (want > 1e-300))   # (a diagonal of 1.25 whatever sf2 is: k < 1.25 keeps the pair positive definite)
    few = ok[np.linspace(0, len(ok) - 1, 12).astype(int)]
    got = []
    for i in few:
        with Model(L, kind, D, ell, sf2, np.vstack([np.zeros(D), G["C"][i]]), [1.0, -1.0], 0.25) as m2:
            R = m2.matrix("R")
            assert R[0, 0] == 1.25 and R[1, 1] == 1.25 and R[0, 1] == R[1, 0]
            got.append(R[0, 1])
    held("ibo_gp_get_R", np.array(got), few)
    # ibo_posterior_cov on the probe model: the mean is k*, S_aa = 4 - k*^2 / 4
    idx = _sample(G, 400)
    Q = L.f64(G["C"][idx]); mu = np.empty(len(idx)); S = np.empty((len(idx), len(idx)))
    with probe_model(L, kind, D, sf2) as m:
        L.check(L.lib.ibo_posterior_cov(m.h, len(idx), L.dp(Q), 1, L.dp(mu), L.dp(S)))
    # (the mean is ibo_posterior_batch's: the sweep kernels' k* -- small2.hip's up to 32 dimensions, the panel-split kernel's beyond -- at their
    # bar; S_aa from the library-exp k* of cov.hip)
    bad, worst = kr.violations(mu, want[idx], kr.bar_fast(fam, G["z"][idx], sf2), fam, G["z"][idx], sf2)
    print("RATIO ibo_posterior_cov mean %s: worst / bar %.3f" % (tag, worst))
    assert len(bad) == 0
    kk = want[idx]
    saa = (LD(4) - kk * kk / 4).astype(np.float64)
    tol = kr.S2_ULPS + 2 * kr.bar_lib(fam, G["z"][idx], sf2) * (kk * kk / 4).astype(np.float64)
    assert np.all(np.abs(np.diag(S) - saa) <= tol), (tag, np.max(np.abs(np.diag(S) - saa) / tol))


@pytest.mark.parametrize("kind,sf2", LIB_VARIANTS)
def test_gradient_of_kstar(L, kind, sf2):
    """ibo_acq_grad_batch on the probe model: dmu = dk*/dc = sf2 map'(z) 2 c_d / ell_d^2 in closed form.  Bar: the library bar on the
    exponential (4 eps (1 + |y|)) plus 6 eps for the factor's products and the Matern polynomial."""
    fam = FAM[kind]
    for D in (1, 5):
        G = kr.probe_grid(fam, D, "ard" if kind == "ard" else "iso", full=(D == 1))
        idx = _sample(G, 600)
        idx = idx[(G["z"][idx] < 1400.0)]                                 # (the derivative of a flushed value is not held)
        Q = L.f64(G["C"][idx]); M = len(idx)
        mu, dmu = np.empty(M), np.empty((M, D))
        with probe_model(L, kind, D, sf2) as m:
            L.check(L.lib.ibo_acq_grad_batch(m.h, M, L.dp(Q), 3, 0.0, 0, CLAMP, NAN, L.dp(mu), None, None, L.dp(dmu), None, None))
        dm = kr.kernel_dmap(fam, G["z"][idx], G["zlo"][idx]) * LD(sf2)
        ell = np.broadcast_to(G["ell"], (D,))
        want = dm[:, None] * (2 * G["C"][idx] / (ell * ell)[None, :])
        rel = (kr.bar_lib(fam, G["z"][idx], sf2) + 6 * kr.EPS)[:, None]
        scale = np.abs(want)
        err = np.abs(LD(1) * dmu - want)
        ok = (err <= rel * scale) | (scale < LD(kr.TINY_EXP) * max(1.0, sf2) * 1e6)
        with np.errstate(divide="ignore", invalid="ignore"):
            ratio = np.where(scale >= LD(kr.TINY_EXP) * max(1.0, sf2) * 1e6, err / (rel * scale), 0).astype(np.float64)
        print("RATIO ibo_acq_grad_batch dmu %s sf2=%g D=%d: worst / bar %.3f" % (kind, sf2, D, np.nanmax(ratio)))
        assert np.all(ok) and not np.any(np.isnan(dmu)), (kind, sf2, D, np.nanmax(ratio))


@pytest.mark.parametrize("kind,sf2", LIB_VARIANTS)
def test_knowledge_gradient_slopes(L, kind, sf2):
    """ibo_kg_batch's slopes on the probe model with ONE reference point a 1000 length scales out (k*(a) = 0 exactly, so v_a = 0): the
    candidates q = a + c have mu = 0, s2 = 4, and the slope of a's line is k(q, a) / sigma_q = k(q, a) / 2 -- kg.hip's library-exp k"""
    fam = FAM[kind]
    G = kr.probe_grid(fam, 1, "iso", full=True)
    idx = _sample(G, 3000)
    idx = idx[G["z"][idx] <= 2 * 745.0]                                   # (farther out a + c meets nothing new)
    a = np.array([[500.0]])                                               # 1000 length scales of 0.5
    Q = L.f64(a + G["C"][idx]); M = len(Q)
    zhi, zlo = kr.z_exact(Q, a[0], np.array([0.5]))
    want = kr.kernel_map(fam, zhi, zlo) * LD(sf2) / 2
    kg, mu_ref, mu, s2, b = np.empty(M), np.empty(1), np.empty(M), np.empty(M), np.empty((M, 1))
    with probe_model(L, kind, 1, sf2) as m:
        L.check(L.lib.ibo_kg_batch(m.h, 1, L.dp(L.f64(a)), M, L.dp(Q), 0, CLAMP, L.dp(kg), L.dp(mu_ref), L.dp(mu), L.dp(s2), L.dp(b)))
    assert mu_ref[0] == 0.0 and np.all(mu == 0.0) and np.all(s2 == 4.0)
    bad, worst = kr.violations(b[:, 0], want, kr.bar_lib(fam, zhi, sf2) + 2 * kr.EPS, fam, zhi, sf2, lib=True)
    print("RATIO ibo_kg_batch slopes %s sf2=%g: worst / bar %.3f over %d" % (kind, sf2, worst, M))
    assert len(bad) == 0, (zhi[bad][:4], b[bad, 0][:4], want[bad][:4].astype(np.float64))


@pytest.mark.parametrize("kind", ["iso", "m3", "m5"])
@pytest.mark.parametrize("dot", [-1, 0])
def test_likelihood_grid_exponent(L, kind, dot):
    """one ibo_nlml_grid call on N = 2, X = {0, 1}, Y = (1, -1) with 3500 length scales: nlml = 1 / (a - k) + log((a - k)(a + k)) / 2 +
    log 2 pi, a = 1 + noise, in long double from the true k.  dot -1: cov_grid_mfma_kernel (exp_fast on the exponent GEMM); 0:
    cov_grid_kernel.  Bar: the hand-written routines' bar on k times |d nlml / d k|, plus 8 eps |nlml| for the 2 x 2 factorisation."""
    fam = FAM[kind]
    noise = 0.25
    g = kr.exponent_grids()
    y = np.concatenate([g["table"][3::4], g["logrun"][320::1], g["edge"][::8]])
    y = y[y < 0]
    theta = 1.0 / np.sqrt(-2.0 * y)                                       # z = 1 / theta^2 ~ -2y: the truth takes the double theta as it is
    k = kr.kernel_of_theta(fam, theta)
    z = (1.0 / theta) ** 2
    want, slope = kr.nlml_2x2(k, noise)
    X = L.f64([[0.0], [1.0]]); Y = L.f64([1.0, -1.0]); T = L.f64(theta.reshape(-1, 1)); out = np.empty(len(theta))
    try:
        L.check(L.lib.ibo_set_option(b"dot_form", dot))
        L.check(L.lib.ibo_nlml_grid(L.default_device(), KTYPE[kind], 2, 1, L.dp(X), L.dp(Y), len(theta), L.dp(T), 1, None, noise, L.dp(out)))
    finally:
        L.check(L.lib.ibo_set_option(b"dot_form", -1))
    tol = (kr.bar_fast(fam, z, 1.0) * k * slope + LD(kr.FLUSH_ATOL) + 8 * kr.EPS * np.abs(want)).astype(np.float64)
    err = np.abs(LD(1) * out - want).astype(np.float64)
    print("RATIO ibo_nlml_grid %s dot_form=%d: worst |nlml - truth| / bar %.3f over %d length scales; share of the bar that is k's at the worst point %.2f"
          % (kind, dot, np.max(err / tol), len(theta), float((kr.bar_fast(fam, z, 1.0) * k * slope)[np.argmax(err / tol)] / tol[np.argmax(err / tol)])))
    assert not np.any(np.isnan(out)) and np.all(err <= tol), (theta[np.argmax(err / tol)], np.max(err / tol))


# ------------------------------------------------------------------------------------------------------------ 3. every fragment position
POS_D = 7
POS_ROUTES = ["small2", "sweep2-forced", "kept", "gemv", "tile-diff", "split-dot", "split-diff", "batch"]


def position_points(N, ell):
    """N points mutually >= 40 length scales apart with |x~|^2 <= 11200: the corners of {0, 40 ell}^7 in binary order, and for row 128,
    which the cube has no corner for, (80 ell_0, 0, ..)"""
    bits = (np.arange(min(N, 128))[:, None] >> np.arange(POS_D)[None, :]) & 1
    X = 40.0 * bits * ell[None, :]
    if N > 128:
        extra = np.zeros((N - 128, POS_D)); extra[:, 0] = 80.0 * ell[0] * (1 + np.arange(N - 128))
        X = np.vstack([X, extra])
    return X


def position_offsets():
    """130 scaled offsets, multiples of 1/16 with |offset|^2 <= 40: differences, squares and sums are exact in the difference form"""
    rs = np.random.RandomState(7)
    K = rs.randint(-38, 39, size=(130, POS_D)).astype(np.float64)
    K[0] = 0.0                                                            # c = x_i
    K[1:40] = np.rint(K[1:40] / 6)                                        # near ones
    return K / 16.0


@pytest.mark.parametrize("kind", ["ard", "m5"])
@pytest.mark.parametrize("N", [64, 65, 129])
def test_every_fragment_position(L, kind, N):
    fam = FAM[kind]
    ell = kr.probe_length_scales("ard", POS_D) if kind == "ard" else np.full(POS_D, 0.5)
    X = position_points(N, ell)
    off = position_offsets()
    zhi, zlo = kr.z_exact(off * ell[None, :], np.zeros(POS_D), ell)
    assert zhi.max() <= 40 and not np.any(zlo)
    want = kr.kernel_map(fam, zhi, zlo)
    c2 = None
    rows = list(range(64)) if N == 64 else ([64, 0, 63] if N == 65 else [128, 64, 127, 5])
    worst = {}
    with Model(L, kind, POS_D, ell if kind == "ard" else ell[:1], 1.0, X, np.zeros(N), kr.PROBE_NOISE, reserve=512 - N) as m:
        R = m.matrix("R")
        assert np.all(np.diag(R) == 4.0) and np.max(np.abs(R - np.diag(np.diag(R)))) < 1e-20
        for i in rows:
            m.set_y(R[:, i])
            mu_obs, _, _, _ = m.batch(X)                                  # alphaY = e_i: the posterior at the observations is e_i
            e = np.zeros(N); e[i] = 1.0
            assert np.max(np.abs(mu_obs - e)) <= 1e-12, (i, np.max(np.abs(mu_obs - e)))
            C = X[i][None, :] + off * ell[None, :]
            assert np.array_equal((C - X[i][None, :]) / ell[None, :], off)
            c2 = np.sum((C / ell[None, :]) ** 2, axis=1)
            x2 = float(np.sum((X[i] / ell) ** 2))
            for route in POS_ROUTES:
                r = ROUTES[route]
                with Options(L, 2 if route == "kept" else r["path"], r["dot"]):       # (130 candidates reach the kept state's kernel only when forced)
                    if r.get("host"):
                        mu, s2, _, name = m.batch(C)
                    else:
                        mu, s2, _, name = m.sweep(C, incremental=r.get("incremental", False))
                assert name == r["kernel"], (route, name)
                lib = r["routine"] == "lib"
                rel = kr.bar_lib(fam, zhi) if lib else kr.bar_fast(fam, zhi, 1.0)
                dot = r["routine"] == "s2" or route == "split-dot"
                if dot:
                    # the documented cancellation of y = a_k + b_c + x~.c~: dy = 2 (|x~|^2 + |c~|^2) eps absolute in the exponent, i.e. relative in k* for
                    # the squared exponential; the Matern kernels take z = -2y: |d log k / d z| 2 dy, at most 3 dy (3/2: nu / (1 + r)) or 5/3 dy (5/2: nu (1 + r) / (3 poly))
                    rel = rel + 2 * (x2 + c2) * kr.EPS * {kr.SE: 1.0, kr.M3: 3.0, kr.M5: 5.0 / 3.0}[fam]
                bad, w = kr.violations(mu, want, rel, fam, zhi, 1.0, lib=lib)
                worst[route] = max(worst.get(route, 0.0), w)
                assert len(bad) == 0, (route, i, w, bad[:5], mu[bad][:5], want[bad][:5].astype(np.float64))
                assert np.all(np.abs(s2 - kr.probe_s2(mu, CLAMP)) <= kr.S2_ULPS), (route, i)
    for route in POS_ROUTES:
        print("RATIO positions %s N=%d %s: worst |mu - k*_i| / bar %.3f over rows %s" % (kind, N, route, worst[route], rows if len(rows) < 8 else "0..63"))


# ------------------------------------------------------------------------------------------------------------ 4. the acquisition epilogue
ZGRID = np.r_[np.arange(-40.0, 40.25, 0.25), -1e-8, 1e-8, 0.0]
XI = 0.01


@pytest.mark.parametrize("erf_mode", [0, 1])
@pytest.mark.parametrize("entry", ["small2", "sweep2", "batch"])
def test_acquisition_epilogue_over_its_range(L, entry, erf_mode):
    """EI, PI and UCB at one candidate of the probe model while ymax moves z = (mu - ymax - xi) / sigma over -40 .. 40: against the
    reference's formula in mpmath from the device's own mu and s2, at 8 eps (|ydiff| + sigma) absolute (NR: plus its erf's rounding)"""
    from ibo_amd import DeviceArray
    M = {"small2": 2, "sweep2": 8193, "batch": 3}[entry]
    with probe_model(L, "iso", 2, 1.0) as m:
        C = np.tile(np.array([[0.375, -0.25]]), (M, 1))
        dc = None if entry == "batch" else DeviceArray.from_host(C)
        call = (lambda **kw: m.batch(C, **kw)) if entry == "batch" else (lambda **kw: m.sweep(C, dc=dc, **kw))
        mu, s2, _, name = call()
        assert name == {"small2": "wk_small_kernel", "sweep2": "sweep2_kernel", "batch": "wk_small_kernel"}[entry]
        assert np.all(mu == mu[0]) and np.all(s2 == s2[0]) and 0.3 < mu[0] < 0.9
        mu0, s20 = float(mu[0]), float(s2[0])
        sigma = float(np.sqrt(s20))
        ymax = mu0 - XI - ZGRID * sigma
        for acq, nm in ((0, "EI"), (1, "PI")):
            got = np.empty(len(ZGRID))
            for i, ym in enumerate(ymax):
                a, b, v, _ = call(acq=acq, parm=XI, erf=erf_mode, ymax=float(ym))
                assert a[0] == mu0 and b[0] == s20 and np.all(v == v[0])
                got[i] = v[0]
            want, yd, sg = kr.acq_truth(acq, erf_mode, mu0, s20, ymax, XI)
            bar = kr.acq_bar(acq, erf_mode, yd, sg)
            err = np.abs(LD(1) * got - want).astype(np.float64)
            print("RATIO epilogue %s %s erf=%d: worst |value - truth| / bar %.3f" % (entry, nm, erf_mode, np.max(err / bar)))
            assert not np.any(np.isnan(got)) and np.all(err <= bar), (nm, ZGRID[np.argmax(err / bar)], np.max(err / bar))
            if acq == 1:
                assert np.all(got >= 0.0) and np.all(got <= 1.0)
        for parm in (0.0, 0.5, 2.0, 1e3, -1.5):
            a, b, v, _ = call(acq=2, parm=parm, erf=erf_mode)
            want, yd, sg = kr.acq_truth(2, erf_mode, mu0, s20, 0.0, parm)
            assert abs(LD(v[0]) - want) <= kr.acq_bar(2, erf_mode, abs(mu0), abs(parm) * sigma), (parm, v[0])
        if dc is not None:
            dc.free()

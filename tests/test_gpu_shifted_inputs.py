"""
Inputs away from the unit cube on every kernel route ("inputs away from the origin").

Every other model of the suite has its observations in [0, 1)^D.  Here the data sit tens to a million units from the origin, on
both sides of the three dot-form guards (max |x~|^2 <= 2e4: csrc/abi_fit.hip dot_form_ok and ibo_gp_extend; 1e5: csrc/abi_nlml.hip) and
beyond the candidate pull-in (|c~|^2 > 6e5: IBO_DOT_PULL_IN in csrc/ibo_common.h, applied by s2_stage_candidates in csrc/sweep2_dev.h).

The reference is the oracle at the UNSHIFTED data: on the 2^-12 grid moved by an integer it returns the same bits at the shifted
data (tests/shift_reference.py, tests/test_shift_reference.py), so the bars are test_gpu_parity.py's, unchanged: mu at rtol 1e-6,
atol 1e-9; s2 at rtol 1e-6; the acquisition at rtol 1e-6, atol 1e-12; the arg-max the argmax of the returned values.  Where the dot
form is compared with the difference form on one handle the bar is 8 x the float64 emulation's deviation for that very case
(shift_reference.measured_bar), never above 1e-6.  The entries that subtract before they scale must not notice the shift at all:
np.array_equal.  Run on the MI355X box with `pytest -m gpu`.
"""
import ctypes

import numpy as np
import pytest

import shift_reference as sr

pytestmark = pytest.mark.gpu

RT = 1e-6
ACQ_ATOL = 1e-12
DOT_ROUTES = ("wk_small_kernel", "sweep2_kernel", "sweep2_kernel<part>", "sweep2_rank1_kernel")


@pytest.fixture(scope="module")
def ibo():
    import ibo_amd
    from ibo_amd import _lib
    if _lib.device_count() < 1:
        pytest.fail("no GPU visible: the product has no CPU fallback")
    err = ctypes.c_double()
    _lib.check(_lib.lib.ibo_selftest_mfma(0, ctypes.byref(err)))
    return ibo_amd


def close(a, b, rtol=RT, atol=1e-12):
    np.testing.assert_allclose(a, b, rtol=rtol, atol=atol)


def option(name, value):
    from ibo_amd import _lib
    _lib.check(_lib.lib.ibo_set_option(name, value))


def make_kernel(kind, hyper):
    from ibo_amd.gaussianprocess import kernel as K
    return {"ard": K.GaussianKernel_ard, "iso": K.GaussianKernel_iso, "m3": K.MaternKernel3, "m5": K.MaternKernel5}[kind](np.array(hyper, dtype=float))


def make_prior(prior):
    from ibo_amd.gaussianprocess.prior import RBFNMeanPrior
    if prior is None:
        return None
    p = RBFNMeanPrior()
    p.means, p.beta, p.theta, p.lowerb, p.width = prior
    return p


def relerr(a, b, atol=0.0):
    """the worst |a - b| / (|b| + atol / rtol-free floor): what the summaries in profiles/ quote"""
    return float(np.max(np.abs(np.asarray(a) - np.asarray(b)) / np.maximum(np.abs(np.asarray(b)), 1e-300 + atol)))


def run_sweep(GP, cand, path=0, dot=-1, **kw):
    """one native EI sweep with per-candidate outputs under a forced route / exponent form; the options are restored"""
    from ibo_amd.acquisition import sweep
    try:
        option(b"sweep_path", path); option(b"dot_form", dot)
        r = sweep(GP, cand, acq='ei', xi=.01, native=True, outputs=("mu", "s2", "acq"), **kw)
    finally:
        option(b"sweep_path", 0); option(b"dot_form", -1)
    assert r["best_idx"] == int(np.argmax(r["acq"])), (r["kernel"], r["best_idx"], int(np.argmax(r["acq"])))
    return r


class Reference(object):
    """the oracle's native EI sweep of a model at chosen rows of its candidate array, evaluated once per row"""

    def __init__(self, oracle, kind, hyper, X, Y, noise, C, prior=None):
        self.orc, self.C = oracle, C
        self.ogp = oracle.GP(oracle.Kern(kind, hyper), X, Y, noise=noise, prior=None if prior is None else oracle.Prior(*prior))
        self.invR = self.ogp.inv_factor()
        self.have = {}

    def at(self, idx):
        idx = np.asarray(idx, dtype=int)
        new = np.array([i for i in np.unique(idx) if i not in self.have], dtype=int)
        if len(new):
            o = self.orc.sweep_native(self.ogp, self.C[new], self.orc.ACQ_EI, .01, invR=self.invR)
            for j, i in enumerate(new):
                self.have[int(i)] = (o["mu"][j], o["s2"][j], o["acq"][j])
        v = np.array([self.have[int(i)] for i in idx])
        return dict(mu=v[:, 0], s2=v[:, 1], acq=v[:, 2])

    def check(self, r, M, what, extra=(), log=None):
        """the suite's bars on about 60 candidates of a sweep of the first M rows: spread, on observations, last tile, arg-max"""
        idx = sr.sample_index(M, np.r_[1, 7, r["best_idx"], np.asarray(extra, dtype=int)])
        o = self.at(idx)
        e = (relerr(r["mu"][idx], o["mu"], 1e-3), relerr(r["s2"][idx], o["s2"]), relerr(r["acq"][idx], o["acq"], 1e-6))
        print("%s %s M=%d: worst relative error on %d sampled candidates  mu %.2g  s2 %.2g  acq %.2g" % (what, r["kernel"], M, len(idx), e[0], e[1], e[2]))
        if log is not None:
            log.append((r["kernel"], M) + e)
        close(r["mu"][idx], o["mu"], atol=1e-9); close(r["s2"][idx], o["s2"]); close(r["acq"][idx], o["acq"], atol=ACQ_ATOL)
        # the winner beats every sampled candidate by the oracle's own numbers too
        w = self.at([r["best_idx"]])["acq"][0]
        assert w >= o["acq"].max() - (RT * abs(w) + ACQ_ATOL)
        return o


# ------------------------------------------------------------------------------------------------------------ a. both sides of the guard
@pytest.mark.parametrize("name", [c[0] for c in sr.SWEEP_CASES])
def test_both_sides_of_the_guard_on_every_sweep_route(ibo, oracle, name):
    """a model just inside the guard takes the dot routes (wk_small_kernel at 17, 600 and 4096 candidates, the panel-split kernel
    when forced, sweep2_kernel at 8300) and the GEMV kernel when forced; moved the other way to just beyond the guard it takes the
    GEMV kernel (3 candidates), the panel-split kernel in its difference form (40) and sweep_mfma_kernel (8300).  All against the
    oracle at the unshifted data; inside, the dot form against the difference form of the same handle at the measured bar."""
    from ibo_amd.gaussianprocess import GaussianProcess
    c = sr.sweep_case(name)
    ref = Reference(oracle, c["kind"], c["hyper"], c["X0"], c["Y"], c["noise"], c["C0"])
    if name == [s[0] for s in sr.SWEEP_CASES if s[1] == c["kind"]][0]:
        # one case per family: the oracle at the shifted data gives the same bits
        idx = sr.sample_index(sr.SWEEP_M, [1, 7])
        shifted = Reference(oracle, c["kind"], c["hyper"], c["X0"] + c["t_in"], c["Y"], c["noise"], c["C0"] + c["t_in"])
        a, b = ref.at(idx), shifted.at(idx)
        assert all(np.array_equal(a[k], b[k]) for k in ("mu", "s2", "acq"))
    dev = sr.sweep_case_deviation(name)
    bar = sr.measured_bar(dev["dot"] + dev["scaled"])
    print("%s: emulated s2 deviation dot %.2g, scaled-first %.2g: dot-against-difference bar %.2g" % (name, dev["dot"], dev["scaled"], bar))
    t = c["t_in"]
    GP = GaussianProcess(make_kernel(c["kind"], c["hyper"]), c["X0"] + t, c["Y"], noise=c["noise"])
    C = c["C0"] + t
    for M, path, kernel in ((17, 0, "wk_small_kernel"), (600, 0, "wk_small_kernel"), (4096, 0, "wk_small_kernel"),
                            (40, 3, "sweep_mfma_kernel<split>"), (sr.SWEEP_M, 0, "sweep2_kernel"), (40, 1, "sweep_gemv_kernel")):
        r = run_sweep(GP, C[:M], path)
        assert r["kernel"] == kernel, (M, path, r["kernel"])
        assert r["s2"][7] < 1.0 / (1.0 + c["noise"])                    # on an observation
        if path == 1:
            ref.check(r, M, "%s inside (t=%d)" % (name, t))
            continue
        d = run_sweep(GP, C[:M], path, dot=0)
        if M == sr.SWEEP_M:
            assert d["kernel"] == "sweep_mfma_kernel"
        assert d["kernel"] not in DOT_ROUTES, d["kernel"]
        # the oracle also judges the candidates where the two forms disagree most
        worst = [int(np.argmax(np.abs(r["mu"] - d["mu"]) / (sr.MU_ATOL + sr.MU_RTOL * np.abs(d["mu"])))), int(np.argmax(np.abs(r["mu"] - d["mu"]))),
                 int(np.argmax(np.abs(r["s2"] - d["s2"]) / d["s2"]))]
        ref.check(r, M, "%s inside (t=%d)" % (name, t), extra=worst)
        ref.check(d, M, "%s inside, difference form" % name, extra=worst)
        m = min(M, sr.EMU_M)                                             # (the rows the emulation covers; the rest at the suite's bar)
        print("%s M=%d: dot against difference, worst s2 deviation %.2g (bar %.2g), worst |mu deviation| %.2g" %
              (name, M, relerr(r["s2"][:m], d["s2"][:m]), bar, np.max(np.abs(r["mu"] - d["mu"]))))
        close(r["s2"][:m], d["s2"][:m], rtol=bar, atol=0)
        # (each form is held to the suite's bar against the oracle, so the two may differ by twice that)
        close(r["s2"], d["s2"], rtol=2 * RT, atol=0); close(r["mu"], d["mu"], rtol=2 * RT, atol=2e-9)
    t = c["t_out"]
    GP = GaussianProcess(make_kernel(c["kind"], c["hyper"]), c["X0"] + t, c["Y"], noise=c["noise"])
    C = c["C0"] + t
    for M, kernel in ((3, "sweep_gemv_kernel"), (40, "sweep_mfma_kernel<split>"), (sr.SWEEP_M, "sweep_mfma_kernel")):
        r = run_sweep(GP, C[:M])
        assert r["kernel"] == kernel, (M, r["kernel"])
        ref.check(r, M, "%s outside (t=%d)" % (name, t))


# ------------------------------------------------------------------------------------------------------------ b. far offsets
@pytest.mark.parametrize("name", [c[0] for c in sr.FAR_CASES])
def test_far_offsets_on_the_difference_routes(ibo, oracle, name):
    """thousands to a million units from the origin only the difference routes run (they scale first and subtract afterwards:
    |x~| 2^-53 a coordinate): the suite's bars against the oracle still hold"""
    from ibo_amd.gaussianprocess import GaussianProcess
    c = sr.far_case(name)
    ref = Reference(oracle, c["kind"], c["hyper"], c["X0"], c["Y"], c["noise"], c["C0"])
    GP = GaussianProcess(make_kernel(c["kind"], c["hyper"]), c["X0"] + c["t"], c["Y"], noise=c["noise"])
    C = c["C0"] + c["t"]
    for M, kernel in ((40, "sweep_mfma_kernel<split>"), (sr.SWEEP_M, "sweep_mfma_kernel")):
        r = run_sweep(GP, C[:M])
        assert r["kernel"] == kernel, (M, r["kernel"])
        ref.check(r, M, "%s (t=%d)" % (name, c["t"]))
    mu, s2 = GP.posterior(C[7])                                          # one point: the GEMV kernel
    o = ref.at([7])
    close(mu, o["mu"][0], atol=1e-9); close(max(s2, 1e-7), max(o["s2"][0], 1e-7))


# ------------------------------------------------------------------------------------------------------------ c. beyond the pull-in radius
@pytest.mark.parametrize("name", [c[0] for c in sr.PULLIN_CASES])
def test_candidates_beyond_the_pull_in_radius(ibo, oracle, name):
    """64 candidates at |c~|^2 = 5.9e5, 6.1e5, 1e7 and 1e12 (towards the data, away from them, along an axis, at random) among
    ordinary ones, on a model near the guard's edge: k* is exactly 0 there, so mu is the prior's mean at the REAL point (0 without a
    prior) and s2 = 1 + noise, on sweep2_kernel, wk_small_kernel, the panel-split kernel's dot form and the rank-1 refresh; the
    arg-max is the difference form's"""
    from ibo_amd import DeviceArray
    from ibo_amd.gaussianprocess import GaussianProcess
    c = sr.pullin_case(name)
    X = c["X0"] + c["t"]
    ref = Reference(oracle, c["kind"], c["hyper"], X, c["Y"], c["noise"], c["C"], prior=c["prior"])
    GP = GaussianProcess(make_kernel(c["kind"], c["hyper"]), X, c["Y"], noise=c["noise"], prior=make_prior(c["prior"]))
    far = c["far"]
    want_mu = np.zeros(len(far)) if c["prior"] is None else np.array([ref.ogp.prior.mu(x) for x in c["C"][far]])

    def far_values(r, what):
        close(r["s2"][far], 1.0 + c["noise"], rtol=1e-15, atol=0)
        close(r["mu"][far], want_mu, atol=1e-9)
        assert np.all(np.isfinite(r["acq"][far])), what
    for M, path, kernel in ((sr.SWEEP_M, 0, "sweep2_kernel"), (600, 0, "wk_small_kernel"), (200, 3, "sweep_mfma_kernel<split>")):
        r = run_sweep(GP, c["C"][:M], path)
        assert r["kernel"] == kernel, (M, path, r["kernel"])
        ref.check(r, M, "%s pull-in" % name, extra=far)
        far_values(r, kernel)
        d = run_sweep(GP, c["C"][:M], path, dot=0)
        assert d["kernel"] not in DOT_ROUTES
        far_values(d, "difference form")
        assert r["best_idx"] == d["best_idx"], (kernel, r["best_idx"], d["best_idx"])
    # the kept state and its rank-1 refresh stage the candidates with their own copy of the pull-in
    dc = DeviceArray.from_host(c["C"])
    r = run_sweep(GP, dc, incremental=True)
    assert r["kernel"] == "sweep2_kernel"
    far_values(r, "kept state")
    xn = sr.dyadic(7, 1, c["D"])[0] * 0.5 + c["t"]
    GP.addData(xn, float(np.sin(3 * (xn - c["t"]).sum())))
    r = run_sweep(GP, dc, incremental=True)
    assert r["kernel"] == "sweep2_rank1_kernel"
    far_values(r, "rank-1 refresh")
    ref2 = Reference(oracle, c["kind"], c["hyper"], GP.X, GP.Y, c["noise"], c["C"], prior=c["prior"])
    ref2.check(r, sr.SWEEP_M, "%s pull-in, rank-1 refresh" % name, extra=far)


# ------------------------------------------------------------------------------------------------------------ d. extension across the guard
def test_extension_across_the_guard(ibo, oracle):
    """GP.addData of single points through ibo_gp_extend: a point inside the guard leaves the sweeps on the dot routes, a point at
    |x~|^2 ~ 1.1 x the guard sends the next ones to the difference routes -- also ibo_acq_sweep_incremental with a kept state on the handle --
    and a refit back inside the guard starts over rather than reuse that state"""
    from ibo_amd import DeviceArray
    from ibo_amd.gaussianprocess import GaussianProcess
    from ibo_amd.acquisition import sweep
    c = sr.extend_case()
    N, X, Y, C = c["N"], c["X"], c["Y"], c["C"]
    kern = make_kernel(c["kind"], c["hyper"])
    GP = GaussianProcess(kern, X, Y[:N], noise=c["noise"])
    extended = []
    inner = GP._extend_device
    GP._extend_device = lambda n_old, Xnew: extended.append(inner(n_old, Xnew)) or extended[-1]
    dc = DeviceArray.from_host(C)

    def fresh(rows, targets):
        return GaussianProcess(kern, rows, targets, noise=c["noise"])

    def against_fresh(r, rows, targets, what):
        """bit for bit in best_idx and to 1e-9 in value against a full ibo_acq_sweep on a fresh handle; the oracle refitted on all rows"""
        ref = fresh(rows, targets)
        f = run_sweep(ref, dc)
        assert r["best_idx"] == f["best_idx"], (what, r["best_idx"], f["best_idx"])
        close(r["best_val"], f["best_val"], rtol=1e-9, atol=0)
        close(r["mu"], f["mu"], rtol=1e-9, atol=1e-10); close(r["s2"], f["s2"], rtol=1e-9, atol=0); close(r["acq"], f["acq"], rtol=1e-9, atol=ACQ_ATOL)
        Reference(oracle, c["kind"], c["hyper"], rows, targets, c["noise"], C).check(r, len(C), what)
        return ref, f

    r = run_sweep(GP, dc, incremental=True)
    assert r["kernel"] == "sweep2_kernel"
    against_fresh(r, X, Y[:N], "extend: start")
    # 1. a point inside the guard: an extension, and the dot routes stay
    L0, ms0 = np.array(GP.L), GP.last_fit_ms()
    GP.addData(c["p_in"], Y[N])
    assert extended == [True]
    assert np.array_equal(np.array(GP.L)[:N, :N], L0) and GP.last_fit_ms() != ms0      # the old rows of L untouched, a new timing on the handle
    rows = np.vstack([X, c["p_in"]])
    r = run_sweep(GP, dc, incremental=True)
    assert r["kernel"] == "sweep2_rank1_kernel"
    ref, _ = against_fresh(r, rows, Y[:N + 1], "extend: a point inside")
    close(GP.L, ref.L, rtol=1e-12, atol=1e-13)
    assert run_sweep(GP, C[:40])["kernel"] == "wk_small_kernel" and run_sweep(GP, C[:8300])["kernel"] == "sweep2_kernel"
    # 2. a point beyond the guard: an extension again, and every later sweep on a difference route
    GP.addData(c["p_out"], Y[N + 1])
    assert extended == [True, True]
    rows = np.vstack([rows, c["p_out"]])
    r = run_sweep(GP, dc, incremental=True)
    assert r["kernel"] == "sweep_mfma_kernel", r["kernel"]
    ref, f = against_fresh(r, rows, Y, "extend: across the guard")
    assert f["kernel"] == "sweep_mfma_kernel"                            # the fresh handle's own guard agrees
    np.testing.assert_array_equal(GP.R, ref.R)
    close(GP.L, ref.L, rtol=1e-12, atol=1e-13)
    for M, kernel in ((3, "sweep_gemv_kernel"), (40, "sweep_mfma_kernel<split>"), (8300, "sweep_mfma_kernel")):
        a, b = run_sweep(GP, C[:M]), run_sweep(ref, C[:M])
        assert a["kernel"] == kernel and b["kernel"] == kernel, (M, a["kernel"], b["kernel"])
        close(a["mu"], b["mu"], rtol=1e-9, atol=1e-10); close(a["s2"], b["s2"], rtol=1e-9, atol=0); assert a["best_idx"] == b["best_idx"]
    r = run_sweep(GP, dc, incremental=True)                              # once more: still no kept dot-form state in use
    assert r["kernel"] == "sweep_mfma_kernel"
    # 3. refitted back inside the guard (the crossing row dropped): the state kept before the crossing is stale
    GP.X, GP.Y = rows[:N + 1], Y[:N + 1]
    GP._fit_device()
    r = run_sweep(GP, dc, incremental=True)
    assert r["kernel"] == "sweep2_kernel", r["kernel"]
    against_fresh(r, rows[:N + 1], Y[:N + 1], "extend: refitted inside")
    r = sweep(GP, dc, acq='ei', xi=.01, incremental=True)               # arg-max only on the state just formed
    f = sweep(fresh(rows[:N + 1], Y[:N + 1]), dc, acq='ei', xi=.01)
    assert r["best_idx"] == f["best_idx"]; close(r["best_val"], f["best_val"], rtol=1e-9, atol=0)


# ------------------------------------------------------------------------------------------------------------ e. translation invariance
INVARIANT_CASES = [("ard", 193, 3, .1), ("iso", 600, 16, 1e-3), ("m3", 193, 16, 1e-3), ("m5", 600, 3, .1)]


def _entries(kind, N, D, noise, t):
    """every subtract-first entry at the data moved by t: {name: array}"""
    from ibo_amd import _lib
    from ibo_amd.gaussianprocess import GaussianProcess
    from ibo_amd.acquisition import EI, PI, UCB
    from ibo_amd.gaussianprocess.trainhyper import marginalLikelihood, nlml_values
    hyper = sr.hyper_of(kind, D)
    kern = make_kernel(kind, hyper)
    X0 = sr.dyadic(600 + N + D, N + 3, D); Y = sr.targets(601, X0)
    Q0 = sr.candidates(602, X0[:N], 24)
    rs = np.random.RandomState(603)
    prior = (rs.rand(4, D), rs.randn(4), 2.0, np.full(D, -.125 + t), np.full(D, 2.0))
    out = {}
    GP = GaussianProcess(kern, X0[:N] + t, Y[:N], noise=noise, prior=make_prior(prior))
    out["fit L"], out["fit R"] = np.array(GP.L), np.array(GP.R)
    GP.addData(X0[N] + t, Y[N]); GP.addData(X0[N + 1:] + t, Y[N + 1:])
    out["extended L"], out["extended R"] = np.array(GP.L), np.array(GP.R)
    Q = Q0 + t
    ktype, hy, sf2, _ = kern._ibo_spec()
    dev = _lib.default_device()
    K = np.empty((N, N)); Kx = np.empty((24, N))
    A = _lib.f64(X0[:N] + t); B = _lib.f64(Q)
    _lib.check(_lib.lib.ibo_cov_matrix(dev, ktype, D, _lib.dp(hy), len(hy), sf2, N, _lib.dp(A), 0, None, _lib.DIAG_UNIT_PLUS_NOISE, noise, _lib.dp(K)))
    _lib.check(_lib.lib.ibo_cov_matrix(dev, ktype, D, _lib.dp(hy), len(hy), sf2, 24, _lib.dp(B), N, _lib.dp(A), 0, 0.0, _lib.dp(Kx)))
    out["cov_matrix square"], out["cov_matrix cross"] = K, Kx
    mu, s2, dmu, ds2 = GP.posterior_gradient(Q)
    out["posterior_gradient dmu"], out["posterior_gradient ds2"] = dmu, ds2
    out["~posterior mu"], out["~posterior s2"] = mu, s2                  # (from the sweep kernels: scaled first -- held to 1e-6 below)
    for nm, a in (("EI", EI(GP, xi=.01)), ("PI", PI(GP, xi=.01)), ("UCB", UCB(GP, D))):
        v, g = a.gradient(Q)
        out[nm + ".gradient"], out["~" + nm + " value"] = g, v
    mu, S = GP.posterior_cov(Q)
    out["posterior_cov Sigma"], out["~posterior_cov mu"] = S, mu
    Z = _lib.f64(np.random.default_rng(5).standard_normal((3, 24))); F = np.empty((3, 24)); info = ctypes.c_int(0)
    _lib.check(_lib.lib.ibo_posterior_sample(GP._handle(), 24, _lib.dp(_lib.f64(Q)), 1, 0.0, 3, _lib.dp(Z), _lib.dp(F), None, ctypes.byref(info)))
    out["sample_posterior draws - mu"] = F
    out["~sample_posterior"] = GP.sample_posterior(Q, n=3, seed=5)
    lm, ls = GP.loo()
    out["loo mu"], out["loo s2"] = lm, ls
    v, g = marginalLikelihood(kern, X0[:N] + t, Y[:N], len(hyper), noise=noise)
    out["nlml_grad value"], out["nlml_grad gradient"] = np.array([v]), g
    try:
        option(b"dot_form", 0)
        longer = [h * 1.25 for h in hyper[:1]] + hyper[1:]               # a second theta-point: another first length scale
        out["=nlml_grid (difference form)"] = nlml_values([kern, make_kernel(kind, longer)], X0[:N] + t, Y[:N], noise)
    finally:
        option(b"dot_form", -1)
    out["=reference"] = (X0[:N], Y[:N], [hyper, longer])
    return out


@pytest.mark.parametrize("kind,N,D,noise", INVARIANT_CASES)
def test_subtract_first_entries_do_not_notice_an_integer_shift(ibo, oracle, kind, N, D, noise):
    """the fit and the extension (L, R), ibo_cov_matrix, the query-point gradients, the joint posterior covariance and the draws'
    deviations from the mean, the leave-one-out predictions and ibo_nlml_grad subtract unscaled coordinates before anything else: at
    data on the 2^-12 grid moved by 94 or by -2^20 (query points and the prior's lower bound moved along) they return the bits of
    the unshifted call.  Two groups scale first and keep their own bars instead: the values that come out of the sweep kernels next
    to the gradients (mu, s2, acquisition values, the draws' mean) the suite's 1e-6, and ibo_nlml_grid's difference form
    (cov_grid_kernel scales the coordinates on their way into LDS) its 1e-9 against the oracle at the unshifted data."""
    base = _entries(kind, N, D, noise, 0)
    X0, Y, hypers = base["=reference"]
    nlml = np.array([oracle.marginal_likelihood(oracle.Kern(kind, h), X0, Y, 1, compute_gradient=False, noise=noise) for h in hypers])
    differs = []
    for t in (94, -1048576):
        got = _entries(kind, N, D, noise, t)
        for k in base:
            if k == "=reference":
                continue
            if k.startswith("="):
                print("%s N=%d D=%d t=%d: %s deviates from the oracle by %.2g, from the unshifted call by %.2g" % (kind, N, D, t, k[1:], relerr(got[k], nlml), relerr(got[k], base[k])))
                close(got[k], nlml, rtol=1e-9, atol=0)
            elif k.startswith("~"):
                close(got[k], base[k], rtol=RT, atol=1e-9)
            elif not np.array_equal(got[k], base[k]):
                differs.append("%s at t=%d: worst deviation %.3g" % (k, t, float(np.max(np.abs(got[k] - base[k]) / (np.abs(base[k]) + 1e-300)))))
    assert not differs, differs


@pytest.mark.parametrize("t", [94, 4096])
def test_loo_gradient_scales_first_and_keeps_its_bar(ibo, oracle, t):
    """looLikelihood's dK generation (csrc/loo.hip) scales the coordinates first: its 1e-9-of-the-terms bar against
    loo_reference at the unshifted data holds at the shifted ones"""
    import loo_reference as lr
    from ibo_amd.gaussianprocess.trainhyper import looLikelihood
    for kind, N, D in (("ard", 193, 3), ("m5", 300, 4)):
        hyper = sr.hyper_of(kind, D)
        X0 = sr.dyadic(700 + N, N, D); Y = sr.targets(701, X0)
        nh = len(hyper)
        ref = lr.objective(oracle.Kern(kind, hyper), X0, Y, lr.NOISE, nh)
        assert ref["cond"] <= 1e6
        v, g, (mu, s2) = looLikelihood(make_kernel(kind, hyper), X0 + t, Y, nh, True, noise=lr.NOISE, predictions=True)
        err = np.abs(np.asarray(g) - ref["grad"])
        print("loo gradient %s t=%d: err / S_h max %.3g" % (kind, t, np.max(err / ref["S"])))
        assert np.all(err <= 1e-9 * ref["S"]), (kind, t, g, ref["grad"], ref["S"])
        assert abs(v - ref["value"]) <= 1e-9 * (N + abs(ref["value"]))
        assert np.all(np.abs(mu - ref["mu"]) <= 1e-9 * (np.abs(Y) + np.abs(ref["c"]) / ref["d"])) and np.all(np.abs(s2 - ref["s2"]) <= 1e-9 * ref["s2"])


# ------------------------------------------------------------------------------------------------------------ f. the NLML grid at the guard
@pytest.mark.parametrize("name", [c[0] for c in sr.NLML_CASES])
def test_nlml_grid_on_both_sides_of_its_guard(ibo, oracle, name):
    """ibo_nlml_grid where every theta-point keeps sum_d w_d max_k x_kd^2 just under 1e5 (the dot form on the MFMA unit): the
    difference route against the oracle at 1e-9 as in the unit cube, the dot route at max(1e-9, 8 x the emulation's deviation);
    with one more theta-point just over the bound the whole call is the forced difference call, bit for bit"""
    from ibo_amd.gaussianprocess.trainhyper import nlml_values
    c = sr.nlml_case(name)
    X = c["X0"] + c["t"]
    kernels = lambda rows: [make_kernel(c["kind"], list(th)) for th in rows]

    def both(rows):
        v = nlml_values(kernels(rows), X, c["Y"], c["noise"])
        try:
            option(b"dot_form", 0)
            d = nlml_values(kernels(rows), X, c["Y"], c["noise"])
        finally:
            option(b"dot_form", -1)
        return np.asarray(v), np.asarray(d)
    ref = np.array([oracle.marginal_likelihood(oracle.Kern(c["kind"], th), c["X0"], c["Y"], 1, compute_gradient=False, noise=c["noise"]) for th in c["thetas_over"]])
    dev = sr.nlml_case_deviation(name)
    bar = sr.measured_bar(dev, 1e-9)
    v, d = both(c["thetas"])
    n = len(c["thetas"])
    print("%s t=%d: NLML worst relative deviation from the oracle: difference route %.2g, dot route %.2g (emulated %.2g, bar %.2g); dot against difference %.2g"
          % (name, c["t"], relerr(d, ref[:n]), relerr(v, ref[:n]), dev, bar, relerr(v, d)))
    assert np.all(np.isfinite(v)) and not np.array_equal(v, d)          # the dot route did run
    close(d, ref[:n], rtol=1e-9, atol=0)
    close(v, ref[:n], rtol=bar, atol=0)
    v, d = both(c["thetas_over"])
    assert np.array_equal(v, d)
    close(d, ref, rtol=1e-9, atol=0)


# ------------------------------------------------------------------------------------------------------------ g. DIRECT and the Python layer
def test_direct_and_the_python_layer_on_shifted_anisotropic_boxes(ibo, oracle):
    """maximizeEI / PI / UCB (maxiter 20), the polish and a gallery on boxes away from the origin, with the checks of
    test_direct_max_across_models_against_the_oracle: the value returned is the oracle's acquisition at the point returned, the
    point lies in the box, a second call returns the same bits, DIRECT took the oracle's number of samples (or ended on a flat
    maximum the oracle values the same to 1e-9: at most once), and the polished value is no less than the unpolished one"""
    from ibo_amd.gaussianprocess import GaussianProcess
    from ibo_amd.acquisition import maximizeEI, maximizePI, maximizeUCB, _ucb_parm, cdirectGP
    from ibo_amd.acquisition.gallery import fastUCBGallery
    flat = []
    # (two boxes inside the sweeps' guard -- DIRECT's batches run on the dot routes -- and two beyond it)
    boxes = [(300, 4, [[20., 21.]] * 4, True), (300, 4, [[-94., -93.]] * 4, False), (120, 3, [[-24., -23.]] * 3, True),
             (120, 3, [[-8., -4.], [100., 101.], [-1000., -999.5]], False)]
    for N, D, bounds, inside in boxes:
        box = np.array(bounds)
        width = box[:, 1] - box[:, 0]
        X0 = sr.dyadic(800 + N, N, D); Y = sr.targets(801, X0)
        X = box[:, 0] + X0 * width                                       # exact: the widths are powers of two
        assert np.array_equal((X - box[:, 0]) / width, X0)
        hyper = list(np.array(sr.hyper_of("ard", D)) * width)
        GP = GaussianProcess(make_kernel("ard", hyper), X, Y, noise=.1)
        ogp = oracle.GP(oracle.Kern("ard", hyper), X, Y, noise=.1)
        invR = ogp.inv_factor()
        assert (sr.row_bound(X, sr.scale_of("ard", hyper, D)) <= sr.GUARD) == inside
        assert (run_sweep(GP, X[:17] + width / 8)["kernel"] == "wk_small_kernel") == inside
        for f, acq, code, kw in ((maximizeEI, 'ei', oracle.ACQ_EI, dict(xi=.01)), (maximizePI, 'pi', oracle.ACQ_PI, dict(xi=.01)),
                                 (maximizeUCB, 'ucb', oracle.ACQ_UCB, dict())):
            parm = _ucb_parm(GP, bounds, .1, .2) if acq == 'ucb' else .01
            r, again = f(GP, bounds, maxiter=20, **kw), f(GP, bounds, maxiter=20, **kw)
            assert r[0] == again[0] and np.array_equal(np.asarray(r[1]), np.asarray(again[1])), (r, again)
            optx = np.asarray(r[1], dtype=float)
            assert optx.shape == (D,) and np.all(optx >= box[:, 0]) and np.all(optx <= box[:, 1]), optx
            o, ox, ons = oracle.acqmax_native(ogp, bounds, code, parm, maxiter=20, invR=invR)
            at = oracle.sweep_native(ogp, np.vstack([optx, ox]), code, parm, invR=invR)["acq"]
            close(r[0], at[0], atol=ACQ_ATOL)
            ns = cdirectGP(GP, bounds, 20, 30, 10000, acqfunc=acq, return_samples=True, **(dict(delta=.1, scale=.2) if acq == 'ucb' else kw))[2]
            print("DIRECT %s N=%d box %s: value %.12g at %s, %d samples (oracle %.12g, %d samples)" % (acq, N, bounds[-1], r[0], optx, ns, o, ons))
            if ns != ons or not np.allclose(optx, ox, rtol=1e-9, atol=0):
                close(at[0], at[1], rtol=1e-9, atol=ACQ_ATOL)            # a flat maximum: the oracle values both end points the same
                flat.append((acq, N, bounds[-1]))
            p = f(GP, bounds, maxiter=20, polish=True, **kw) if acq == 'ei' else None
            if p is not None:
                px = np.asarray(p[1], dtype=float)
                assert p[0] >= r[0] and np.all(px >= box[:, 0]) and np.all(px <= box[:, 1])
                close(p[0], oracle.sweep_native(ogp, px[None, :], code, parm, invR=invR)["acq"][0], atol=ACQ_ATOL)
        if D == 3 and width[0] == 4.0:
            # a gallery of 4 over 4096 candidates in the anisotropic box: members in the box, farther apart than the rule asks, the same twice
            cand = box[:, 0] + sr.dyadic(802, 4096, D) * width
            g1 = np.array(fastUCBGallery(GP, bounds, 4, candidates=cand, maxiter=20))
            g2 = np.array(fastUCBGallery(GP, bounds, 4, candidates=cand, maxiter=20))
            assert g1.shape == (4, D) and np.array_equal(g1, g2)
            assert np.all(g1 >= box[:, 0]) and np.all(g1 <= box[:, 1])
            assert min(np.linalg.norm(g1[i] - g1[j]) for i in range(4) for j in range(i)) > .5
    assert len(flat) <= 1, flat

"""
Where conditioning is worst: the evaluation entries held to long-double truth on models of cond_2(R) 1e6 .. 1e8.

Every other accuracy bar of the suite is asserted at noise 0.1 / 0.05, or (test_gpu_parity.py::test_tolerance_where_conditioning_is_worst)
on wk_small_kernel's mu / s2 / EI alone.  Here the models of tests/conditioning_reference.py -- clustered near-duplicates on the 2^-12
grid, noise 1e-6 .. 1e-4 -- go through every sweep route, the kept state and its rank-1 fold, the gradients, the joint covariance, the
pieces of KG and q-EI and the paths' solve, each compared with TrueGP at 24 queries, half of them beside an observation.

Two bars per quantity, both asserted, the error in units of the quantity's terms' magnitude (conditioning_reference's table):
    the project's rule    err <= 1e-15 max(cond_2, 1e6)                     the outer cap
    the reference's reach err <= 8 ref_error(case, quantity)                8 x the error of float64 itself (cho_solve and the device's
                                                                            formulation, five observation orders), computed without a device
EI and its gradient carry the moments' bars through: value cdf dmu + pdf dsigma, gradient as grad_reference's sacq plus the reply of
cdf, pdf and 1 / sigma to the moments' errors; the files' atol 1e-12 stays.  Run on the MI355X box with `pytest -m gpu -s`: every check
prints its worst err / bar.

Measured on the MI355X (worst err / min(rule, 8 ref_error) over the cases; profiles/r11_conditioning_summary.txt has the table per case):
    sweeps, every route (wk_small 17 / 600, sweep2 4137, split dot / diff, tile diff, GEMV 3)   mu 0.13   s2 0.24   EI 0.10
    ibo_acq_batch                                                                                mu 0.13   s2 0.19   EI 0.10
    kept state: first / second visit and the two-part form                                      mu 0.13   s2 0.22   EI 0.10
    kept state after the rank-1 fold (truth and ref_error of the extended data)                  mu 0.27   s2 0.31   EI 0.19
    gradients: 16 points (16-wide tiles), 17 and 70 (64-wide tiles), each                        dmu 0.15  ds2 0.22  dEI 0.05
    joint covariance, with and without noise                                                     Sigma 0.17   smallest eigenvalue < 0.001
    KG: mu_ref 0.15, b 0.41;  q-EI: mu_pend 0.15, S_pend 0.35, c 0.16;  path coefficients 0.12 through the path values, 0.09 entry by entry
The first run found one figure beyond the reach: sigma^2 after the fold on se65, 2.9e-12 against 8 x 2.0e-13.  The in-place extension's
own order -- z = W r, u = W^T z, d = sqrt(1 + noise - z.z), the new row of W = [-u, 1] / d -- restated in float64 is 1.2e-12 from the
truth there (2.7 x the from-scratch factor's error): it joined ref_error of the extended data as formulation (c), and the device sits at
0.31 of the bar that follows.
"""
import ctypes

import numpy as np
import pytest

import conditioning_reference as cc
import grad_reference as gr
import qei_reference as qr

pytestmark = pytest.mark.gpu

NAMES = list(cc.CASES)
XI = .01
ACQ_ATOL = 1e-12
M_BIG = 4097 + 40
# (M, sweep_path, dot_form (-1: the handle's own choice, 1 / 0: the dot / difference form forced), the kernel ibo_last_sweep_kernel_ms must name)
ROUTES = [(17, 0, -1, "wk_small_kernel"), (600, 0, -1, "wk_small_kernel"), (M_BIG, 0, -1, "sweep2_kernel"),
          (600, 3, 1, "sweep_mfma_kernel<split>"), (600, 3, 0, "sweep_mfma_kernel<split>"), (600, 2, 0, "sweep_mfma_kernel"),
          (3, 1, -1, "sweep_gemv_kernel")]
WORST = {}


@pytest.fixture(scope="module")
def lib():
    from ibo_amd import _lib
    if _lib.device_count() < 1:
        pytest.fail("no GPU visible: the product has no CPU fallback")
    err = ctypes.c_double()
    _lib.check(_lib.lib.ibo_selftest_mfma(0, ctypes.byref(err)))
    yield _lib
    print("\nworst err / min(rule, 8 ref_error) per case and quantity:")
    whats = sorted({w for _, w in WORST})
    for w in whats:
        print("  %-26s %s" % (w, "  ".join("%s %.3f" % (n, WORST[(n, w)]) for n in NAMES if (n, w) in WORST)))


def option(name, value):
    from ibo_amd import _lib
    _lib.check(_lib.lib.ibo_set_option(name, value))


def new_gp(name, reserve_rows=0):
    import test_gpu_gradients as tg
    import test_gpu_posterior_cov as pc
    from ibo_amd.gaussianprocess import GaussianProcess
    d = cc.case_data(name)
    prior = None
    if d["prior"] is not None:
        prior, tup = tg.make_prior(d["D"])
        assert all(np.array_equal(np.asarray(a), np.asarray(b)) for a, b in zip(tup, d["prior"]))
    GP = GaussianProcess(pc.make_kernel(d["kind"], d["hyper"]), d["X"], d["Y"], prior=prior, noise=d["noise"], reserve_rows=reserve_rows)
    GP._push_prior()
    return GP


_GPS, _TRUTH = {}, {}


def model(name):
    """one fitted handle per case for the whole file (never mutated: the kept-state test fits its own)"""
    if name not in _GPS:
        _GPS[name] = new_gp(name)
    return _GPS[name]


def truth(name, ext=False):
    """the module's cache of TrueGP's numbers per case"""
    if (name, ext) not in _TRUTH:
        _TRUTH[(name, ext)] = cc.truth_of(name, ext)[0]
    return _TRUTH[(name, ext)]


def note(name, label, share):
    WORST[(name, label)] = max(WORST.get((name, label), 0.0), float(share))


def hold(name, what, got, want, scale, ext=False, label=None):
    """both bars on one quantity: the worst |got - want| / scale against the rule and against 8 x ref_error"""
    rule, reach = cc.bars(name, what, ext)
    err = float(np.max(np.abs(np.asarray(got) - want) / scale))
    label = label or what
    print("%s %s: err %.3g  rule %.3g  8 ref_error %.3g  err / bar %.3f" % (name, label, err, rule, reach, err / min(rule, reach)))
    note(name, label, err / min(rule, reach))
    assert reach <= rule
    assert err <= rule, "%s %s: %g beyond the project's rule %g" % (name, label, err, rule)
    assert err <= reach, "%s %s: %g beyond 8 x the reference's own error %g" % (name, label, err, reach)


def hold_moments(name, t, sel, mu, s2, label, ext=False):
    hold(name, "mu", mu, t["mu"][sel], t["mu_scale"][sel], ext, label + " mu")
    hold(name, "s2", s2, t["s2"][sel], t["s2_scale"][sel], ext, label + " s2")


def ei_of(mu, s2, ymax, erf_mode):
    sig = np.sqrt(s2)
    yd = mu - ymax - XI
    z = yd / sig
    cdf, pdf = gr.cdf_pdf(erf_mode, z)
    return yd * cdf + sig * pdf, cdf, pdf, z, sig


def hold_ei(name, t, sel, got, ymax, erf_mode, label, ext=False):
    """EI against the truth's, the two moment bars carried through: cdf dmu + pdf dsigma (+ the files' atol 1e-12)"""
    want, cdf, pdf, _, sig = ei_of(t["mu"][sel], t["s2"][sel], ymax, erf_mode)
    err = np.abs(np.asarray(got) - want)
    share = 0.0
    for k in (0, 1):                                       # the rule, then the reach
        tol = cdf * cc.bars(name, "mu", ext)[k] * t["mu_scale"][sel] + pdf * cc.bars(name, "s2", ext)[k] * t["s2_scale"][sel] / (2 * sig) + ACQ_ATOL
        share = max(share, float(np.max(err / tol)))
        assert np.all(err <= tol), "%s %s: EI %g of its %s" % (name, label, float(np.max(err / tol)), ("rule", "reach")[k])
    print("%s %s ei: err / bar %.3f" % (name, label, share))
    note(name, label + " ei", share)


def placed(name, M, seed=3):
    """(candidates (M, D), positions, the queries' own numbers): the case's truth queries at the ends, at the tile seams and scattered
    through an array of uniform filler; fewer than 24 rows take queries of both halves in turn, the two beside the first and the
    last observation first"""
    d = cc.case_data(name)
    h = cc.M_TRUTH // 2
    order = np.array([i for pair in zip(range(h, 2 * h), range(h)) for i in pair])
    rs = np.random.RandomState(seed + M)
    fixed = [p for p in (0, M - 1, 15, 16, 31, 32, 63, 64, 255, 256, 511, 512, 1023, 1024, 4095, 4096) if 0 <= p < M]
    pos = list(dict.fromkeys(fixed))[:cc.M_TRUTH]
    free = [p for p in rs.permutation(M) if p not in pos]
    pos = np.array(pos + free[:min(M, cc.M_TRUTH) - len(pos)], dtype=int)
    sel = order[:len(pos)]
    cand = rs.rand(M, d["D"])
    cand[pos] = d["Q"][sel]
    return cand, pos, sel


# ------------------------------------------------------------------------------------------------------------ sweeps
@pytest.mark.parametrize("name", NAMES)
def test_host_batch(lib, name):
    """ibo_acq_batch at M = 24: native EI (libm erf, clamp 1e-8)"""
    GP, d, t = model(name), cc.case_data(name), truth(name)
    M = cc.M_TRUTH
    mu, s2, acq = np.empty(M), np.empty(M), np.empty(M)
    lib.check(lib.lib.ibo_acq_batch(GP._handle(), M, lib.dp(lib.f64(d["Q"])), gr.ACQ_EI, XI, gr.ERF_LIBM, cc.CLAMP_NATIVE, float("nan"),
                                    lib.dp(mu), lib.dp(s2), lib.dp(acq)))
    sel = np.arange(M)
    hold_moments(name, t, sel, mu, s2, "acq_batch")
    hold_ei(name, t, sel, acq, float(np.max(d["Y"])), gr.ERF_LIBM, "acq_batch")


@pytest.mark.parametrize("name", NAMES)
def test_every_sweep_route(lib, name):
    """ibo_acq_sweep with per-candidate outputs on every route sweep_path / dot_form reach; the reported kernel asserted each time"""
    from ibo_amd.acquisition import sweep
    GP, d, t = model(name), cc.case_data(name), truth(name)
    for M, path, dot, kernel in ROUTES:
        cand, pos, sel = placed(name, M)
        try:
            option(b"sweep_path", path); option(b"dot_form", dot)
            r = sweep(GP, cand, acq='ei', xi=XI, native=False, outputs=("mu", "s2", "acq"))
        finally:
            option(b"sweep_path", 0); option(b"dot_form", -1)
        assert r["kernel"] == kernel, (M, path, dot, r["kernel"])
        label = "%s%s M=%d" % (kernel, {-1: "", 0: " diff", 1: " dot"}[dot], M)
        hold_moments(name, t, sel, r["mu"][pos], r["s2"][pos], label)
        hold_ei(name, t, sel, r["acq"][pos], float(np.max(d["Y"])), gr.ERF_NR, label)
        assert r["best_idx"] == int(np.argmax(r["acq"]))


# ------------------------------------------------------------------------------------------------------------ kept state
def state_info(lib, GP):
    tiles, done = ctypes.c_int64(), ctypes.c_int64()
    lib.check(lib.lib.ibo_sweep_state_info(GP._handle(), ctypes.byref(tiles), ctypes.byref(done)))
    return tiles.value, done.value


@pytest.mark.parametrize("name", NAMES)
def test_kept_state_and_the_rank1_fold(lib, name):
    """ibo_acq_sweep_incremental on a fixed device array under gallery_prune 2 (every tile complete): the first visit, the second visit
    (the kept q and dot products alone), the two-part form of the first visit where the model has the rows for it, and the visit after a
    one-row addData of a near-duplicate of an existing row, which extends the factor in place (no refit) and folds the row into the
    state (sweep2_rank1_kernel) -- that one against a TrueGP of the extended data"""
    from ibo_amd import DeviceArray
    from ibo_amd.acquisition import sweep
    d = cc.case_data(name)
    cand, pos, sel = placed(name, M_BIG)
    kw = dict(acq='ei', xi=XI, native=False, incremental=True)
    out = dict(outputs=("mu", "s2", "acq"))
    try:
        option(b"gallery_prune", 2)
        GP = new_gp(name, reserve_rows=4)
        refits = []
        fit = GP._fit_device
        GP._fit_device = lambda *a, **k: (refits.append(1), fit(*a, **k))[1]
        dc = DeviceArray.from_host(cand)
        for visit, kernel in (("first visit", "sweep2_kernel"), ("second visit", "acq_finish_kernel")):
            r = sweep(GP, dc, **kw, **out)
            assert r["kernel"] == kernel, (visit, r["kernel"])
            assert state_info(lib, GP)[0] == state_info(lib, GP)[1]
            hold_moments(name, truth(name), sel, r["mu"][pos], r["s2"][pos], visit)
            hold_ei(name, truth(name), sel, r["acq"][pos], float(np.max(d["Y"])), gr.ERF_NR, visit)
        GP.addData(d["x_new"], d["y_new"])
        assert not refits and len(GP.X) == d["N"] + 1, "the near-duplicate row did not extend the factor in place"
        r = sweep(GP, dc, **kw, **out)
        assert r["kernel"] == "sweep2_rank1_kernel", r["kernel"]
        assert state_info(lib, GP)[0] == state_info(lib, GP)[1]
        te = truth(name, True)
        hold_moments(name, te, sel, r["mu"][pos], r["s2"][pos], "after the fold", ext=True)
        hold_ei(name, te, sel, r["acq"][pos], float(max(np.max(d["Y"]), d["y_new"])), gr.ERF_NR, "after the fold", ext=True)
        # the two-part form: an arg-max-only first visit forms the state in two parts, the visit with outputs reads it
        GP2 = new_gp(name)
        dc2 = DeviceArray.from_host(cand)
        first = sweep(GP2, dc2, **kw)
        assert first["kernel"] == ("sweep2_kernel<part>" if d["N"] >= 500 else "sweep2_kernel"), first["kernel"]
        assert state_info(lib, GP2)[0] == state_info(lib, GP2)[1]
        r = sweep(GP2, dc2, **kw, **out)
        assert r["kernel"] == "acq_finish_kernel", r["kernel"]
        assert r["best_idx"] == first["best_idx"] and r["best_idx"] == int(np.argmax(r["acq"]))
        hold_moments(name, truth(name), sel, r["mu"][pos], r["s2"][pos], "two-part state")
    finally:
        option(b"gallery_prune", 1)


# ------------------------------------------------------------------------------------------------------------ gradients
@pytest.mark.parametrize("M", [16, 17, 70])
@pytest.mark.parametrize("name", NAMES)
def test_gradients(lib, name, M):
    """ibo_acq_grad_batch on either side of grad_plan's threshold -- 16 points in 16-wide tiles, 17 and 70 in 64-wide ones (70: two tiles) --
    dmu, ds2, and dEI with both erf modes; 16 and 17 points take queries of both halves in turn"""
    import test_gpu_gradients as tg
    GP, d, t = model(name), cc.case_data(name), truth(name)
    cand, pos, sel = placed(name, M, seed=5)
    ymax = float(np.max(d["Y"]))
    for erf_mode in (gr.ERF_LIBM, gr.ERF_NR):
        got = tg.grad_call(lib, GP._handle(), cand, acq=gr.ACQ_EI, parm=XI, erf=erf_mode, clamp=cc.CLAMP_PY, guard=True)
        label = "grad M=%d" % M
        if erf_mode == gr.ERF_LIBM:
            hold_moments(name, t, sel, got["mu"][pos], got["s2"][pos], label)
            hold(name, "dmu", got["dmu"][pos], t["dmu"][sel], t["dmu_scale"][sel], label=label + " dmu")
            hold(name, "ds2", got["ds2"][pos], t["ds2"][sel], t["ds2_scale"][sel], label=label + " ds2")
        hold_ei(name, t, sel, got["acq"][pos], ymax, erf_mode, label + " erf%d" % erf_mode)
        # dEI = cdf dmu + pdf dsigma, dsigma = ds2 / (2 sigma): grad_reference's sacq with the bars on dmu and ds2, and the first-order
        # reply of cdf, pdf and 1 / sigma to the moments' own errors
        _, cdf, pdf, z, sig = ei_of(t["mu"][sel], t["s2"][sel], ymax, erf_mode)
        dmu, ds2 = t["dmu"][sel], t["ds2"][sel]
        dsig = ds2 / (2 * sig)[:, None]
        want = cdf[:, None] * dmu + pdf[:, None] * dsig
        err = np.abs(got["dacq"][pos] - want)
        share = 0.0
        for k in (0, 1):
            b = {w: cc.bars(name, w)[k] for w in ("mu", "s2", "dmu", "ds2")}
            e_mu = b["mu"] * t["mu_scale"][sel]; e_sig = b["s2"] * t["s2_scale"][sel] / (2 * sig)
            e_z = (e_mu + np.abs(z) * e_sig) / sig
            e_dsig = b["ds2"] * t["ds2_scale"][sel] / (2 * sig)[:, None] + np.abs(dsig) * (e_sig / sig)[:, None]
            tol = (cdf[:, None] * b["dmu"] * t["dmu_scale"][sel] + pdf[:, None] * e_dsig
                   + (pdf * e_z)[:, None] * np.abs(dmu) + (np.abs(z) * pdf * e_z)[:, None] * np.abs(dsig) + ACQ_ATOL)
            share = max(share, float(np.max(err / tol)))
            assert np.all(err <= tol), "%s M=%d erf %d: dEI %g of its %s" % (name, M, erf_mode, float(np.max(err / tol)), ("rule", "reach")[k])
        print("%s %s dEI erf %d: err / bar %.3f" % (name, label, erf_mode, share))
        note(name, label + " dEI erf%d" % erf_mode, share)


# ------------------------------------------------------------------------------------------------------------ joint covariance
@pytest.mark.parametrize("name", NAMES)
def test_joint_covariance(lib, name):
    """ibo_posterior_cov at the 24 queries, with and without noise: every Sigma_ab, and the smallest eigenvalue within the bar's reach of the
    truth's (Weyl: it moves by at most the 2-norm of the error, which the bar bounds by the norm of bar x scale)"""
    import test_gpu_posterior_cov as pc
    GP, d, t = model(name), cc.case_data(name), truth(name)
    for wn, what in ((1, "cov_noise"), (0, "cov_latent")):
        mu, S = pc.cov_call(lib, GP._handle(), d["Q"], wn, guard=True)
        assert np.array_equal(S, S.T)
        hold(name, what, S, t[what], t[what + "_scale"])
        hold(name, "mu", mu, t["mu"], t["mu_scale"], label=what + " mu")
        lam, lam_t = np.linalg.eigvalsh(S)[0], np.linalg.eigvalsh(t[what])[0]
        reach = min(cc.bars(name, what)) * np.linalg.norm(t[what + "_scale"], 2)
        print("%s %s: smallest eigenvalue %.6g, truth %.6g, |difference| / reach %.3f" % (name, what, lam, lam_t, abs(lam - lam_t) / reach))
        note(name, what + " eigmin", abs(lam - lam_t) / reach)
        assert abs(lam - lam_t) <= reach, (name, what, lam, lam_t, reach)


# ------------------------------------------------------------------------------------------------------------ KG and q-EI pieces
@pytest.mark.parametrize("name", NAMES)
def test_kg_and_qei_pieces(lib, name):
    """what ibo_kg_batch and ibo_qei_batch return besides their values: the means of the reference and pending points, the slopes, c and
    S_pend, at 5 reference / pending points chosen by kg_reference.ref_points / qei_reference.pending_points"""
    import test_gpu_knowledge_gradient as tk
    import test_gpu_qei as tq
    GP, d, t = model(name), cc.case_data(name), truth(name)
    sel = np.arange(cc.M_TRUTH)
    got = tk.kg_call(lib, GP._handle(), d["A"], d["Q"], 1, cc.CLAMP_PY)
    hold(name, "kg_mu_ref", got["mu_ref"], t["kg_mu_ref"], t["kg_mu_ref_scale"])
    hold(name, "kg_b", got["b"], t["kg_b"], t["kg_b_scale"])
    hold_moments(name, t, sel, got["mu"], got["s2"], "kg")
    Z = qr.samples(64, cc.N_REF + 1)
    got = tq.qei_call(lib, GP._handle(), d["P"], Z, d["Q"], clamp=cc.CLAMP_PY)
    assert got["info"] == 0
    hold(name, "qei_mu_pend", got["mu_pend"], t["qei_mu_pend"], t["qei_mu_pend_scale"])
    hold(name, "qei_S", got["S_pend"], t["qei_S"], t["qei_S_scale"])
    hold(name, "qei_c", got["c"], t["qei_c"], t["qei_c_scale"])
    hold_moments(name, t, sel, got["mu"], got["s2"], "qei")


# ------------------------------------------------------------------------------------------------------------ paths
@pytest.mark.parametrize("name", NAMES)
def test_path_coefficients(lib, name):
    """ibo_paths_coef after ibo_paths_create with 64 features and 3 paths: the weights come back as given; the solve's coefficients are
    judged by the path values they give at the queries over paths_reference.terms_scale, and entry by entry over the magnitudes of the
    terms of c_i = aY_i - (R^-1 u)_i (an error that no query's k* sees)"""
    import test_gpu_paths as tp
    GP, d, t = model(name), cc.case_data(name), truth(name)
    N = d["N"]
    P = tp.Paths(lib, GP, lib.f64(d["omega"]), lib.f64(d["phase"]), lib.f64(d["pw"]), lib.f64(d["eps"][:, :N]))
    try:
        co = P.coef()
    finally:
        P.close()
    assert co.shape == (cc.PATHS_S, cc.PATHS_F + N) and np.array_equal(co[:, :cc.PATHS_F], d["pw"])
    for what, share in cc.shares(t, dict(coef=co), whats=("coef", "coef_entry")).items():
        rule, reach = cc.bars(name, what)
        print("%s %s: err %.3g  rule %.3g  8 ref_error %.3g  err / bar %.3f" % (name, what, share, rule, reach, share / min(rule, reach)))
        note(name, what, share / min(rule, reach))
        assert reach <= rule
        assert share <= rule, (name, what, share, rule)
        assert share <= reach, (name, what, share, reach)

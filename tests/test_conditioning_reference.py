"""
tests/conditioning_reference.py pinned on the CPU: the cases' condition numbers, TrueGP against the oracle and against the existing
float64 restatements (on a well-conditioned model, where those are good to 1e-12), the order of the GPU file's two bars
(ref_error <= rule / 8 for every quantity of every case) and the sensitivity of the tighter one: six mutants of the device's formulation
-- what a subtly wrong kernel would do -- each exceed 8 x ref_error on at least one case, so tests/test_gpu_conditioning.py would fail
a kernel that did the same.
"""
import numpy as np
import pytest

import conditioning_reference as cc
import cov_reference as cr
import grad_reference as gr
import kg_reference as kr
import paths_reference as pr
import qei_reference as qr

NAMES = list(cc.CASES)


def test_cases_are_the_ones_the_gpu_file_needs():
    """the five models of the issue's table, a Matern-3/2 one at N = 64, an SE-iso one with a mean prior at N = 300 and an sviso one with
    sf2 != 1; N = 64 / 65 cross the 64-row tile, 1030 the 1024-row panel"""
    table = {n: (c[0], c[2], c[3], c[4]) for n, c in cc.CASES.items()}
    assert table["se65"] == ("ard", 65, 2, 1e-6) and table["m5_65"] == ("m5", 65, 3, 1e-6) and table["se300"] == ("ard", 300, 2, 1e-5)
    assert table["m5_300"] == ("m5", 300, 4, 1e-4) and table["se1030"] == ("ard", 1030, 2, 1e-4)
    assert table["m3_64"][:2] == ("m3", 64) and table["iso300_prior"][:2] == ("iso", 300) and cc.CASES["iso300_prior"][5]
    assert table["sviso65"][0] == "sviso" and cc.case_data("sviso65")["sf2"] != 1.0
    for n in NAMES:
        assert cc.CASES[n][4] in (1e-6, 1e-5, 1e-4) and cc.CASES[n][2] in (64, 65, 300, 1030)


@pytest.mark.parametrize("name", NAMES)
def test_condition_number_and_queries(name):
    """cond_2(R) in [1e6, 1e9], before and after the kept-state test's near-duplicate row; the inputs on their grids; half of the queries
    within 1e-3 (and a grid step) of an observation, the first and the last row among them; no truth variance within a factor 2 of either
    clamp (1e-8 native, 1e-7 Python), none near the upper one: nothing compared is clipped"""
    d = cc.case_data(name)
    print("%s: cond_2 %.3g, with the near-duplicate row %.3g" % (name, d["cond"], cc.extended_data(name)["cond"]))
    for dd in (d, cc.extended_data(name)):
        assert cc.COND_RANGE[0] <= dd["cond"] <= cc.COND_RANGE[1], (name, dd["cond"])
    assert np.array_equal(d["X"] * cc.GRID_X, np.rint(d["X"] * cc.GRID_X)) and np.array_equal(d["Q"] * cc.GRID_Q, np.rint(d["Q"] * cc.GRID_Q))
    assert d["X"].min() >= 0 and d["X"].max() <= 1 and len(d["Q"]) == cc.M_TRUTH
    h = cc.M_TRUTH // 2
    dist = np.sqrt(((d["Q"][:, None, :] - d["X"][None, :, :]) ** 2).sum(axis=2))
    assert np.all(dist[h:].min(axis=1) < 1e-3 * 4 * np.sqrt(d["D"]) + 1 / cc.GRID_Q)
    assert dist[h, 0] < 5e-3 and dist[h + 1, -1] < 5e-3
    assert 0 < np.abs(d["x_new"] - d["X"][7]).sum() <= 1 / cc.GRID_X and not np.any(np.all(d["X"] == d["x_new"], axis=1))
    for ext in (False, True):
        s2 = cc.truth_of(name, ext)[0]["s2"]
        assert s2.min() > 2 * cc.CLAMP_PY > 2 * cc.CLAMP_NATIVE and s2.max() < 5.0, (name, s2.min(), s2.max())
        assert s2[h:].max() < 50 * (1 + d["noise"] - min(d["sf2"], 1.0) + d["noise"])       # beside an observation: sigma^2 ~ noise


@pytest.mark.parametrize("name", NAMES)
def test_truth_agrees_with_the_oracle(oracle, name):
    """the oracle's Python path (two triangular solves) at the suite's bar: mu at rtol 1e-6 / atol 1e-9, sigma^2 at rtol 1e-6"""
    d = cc.case_data(name)
    t = cc.truth_of(name)[0]
    prior = None if d["prior"] is None else oracle.Prior(*d["prior"])
    ogp = oracle.GP(oracle.Kern(d["kind"], d["hyper"]), d["X"], d["Y"], noise=d["noise"], prior=prior)
    mu, s2 = ogp.posteriors(d["Q"])
    np.testing.assert_allclose(mu, t["mu"], rtol=1e-6, atol=1e-9)
    np.testing.assert_allclose(s2, t["s2"], rtol=1e-6)


def test_truth_follows_the_existing_restatements():
    """on a well-conditioned model (noise 0.1, Matern-5/2 with a mean prior) every TrueGP quantity equals what grad_reference,
    cov_reference, kg_reference (float64 and its long-double path), qei_reference and paths_reference define, at 1e-11 of its scale"""
    d = dict(cc.case_data("m5_65"))
    d["noise"] = .1; d["prior"] = cc.prior_tuple(d["D"])
    t, gp = cc.truth_of_data(d)
    ref = gr.RefGP(d["X"], d["Y"], d["noise"], d["fam"], d["w"], d["sf2"], prior=d["prior"])
    g = ref.grad(d["Q"])
    want = dict(mu=g["mu"], s2=g["s2"], dmu=g["dmu"], ds2=g["ds2"])
    np.testing.assert_allclose(t["dmu_scale"], g["smu"], rtol=1e-9); np.testing.assert_allclose(t["ds2_scale"], g["ss2"], rtol=1e-9)
    for key, wn in (("cov_noise", True), ("cov_latent", False)):
        want[key], vn = cr.cov(ref, d["Q"], wn)
        np.testing.assert_allclose(t[key + "_scale"], ref.sf2 + ref.noise + np.outer(vn, vn), rtol=1e-9)
    s = kr.slopes(ref, d["A"], d["Q"])
    want.update(kg_mu_ref=s["mu_ref"], kg_b=s["b"])
    pc = qr.pieces(ref, d["P"], d["Q"])
    want.update(qei_mu_pend=pc["mu_pend"], qei_S=pc["S_pend"], qei_c=pc["c"])
    want["coef"] = pr.coef(ref, d["omega"], d["phase"], d["pw"], d["eps"][:, :d["N"]])
    got = cc.shares(t, want)
    print({k: "%.2g" % v for k, v in got.items()})
    assert set(got) == set(cc.WHATS) and max(got.values()) < 1e-11, got
    np.testing.assert_allclose(t["coef"].astype(float), want["coef"], rtol=1e-9, atol=1e-12)
    T = pr.terms_scale(ref, d["omega"], d["phase"], want["coef"], d["Q"])
    np.testing.assert_allclose(t["coef_scale"].astype(float), T, rtol=1e-9)
    sl = kr.slopes(ref, d["A"], d["Q"], dtype=np.longdouble)
    np.testing.assert_allclose(sl["b"].astype(float), t["kg_b"], rtol=1e-13, atol=1e-15)
    np.testing.assert_allclose(sl["mu_ref"].astype(float), t["kg_mu_ref"], rtol=1e-13, atol=1e-15)
    # both restatements of this file too, and the bordered factor against a factor from scratch
    for form in ("a", "b"):
        assert max(cc.shares(t, cc.restate(d, form)).values()) < 1e-11
    x, y = d["x_new"], d["y_new"]
    e = gp.extended(x, y); f = cc.TrueGP(e.X, e.Y, d["noise"], d["fam"], d["w"], d["sf2"], d["prior"])
    assert float(np.max(np.abs(e.W - f.W))) < 1e-17 * float(np.max(np.abs(f.W))) * 100 and float(np.max(np.abs(e.aY - f.aY))) < 1e-16 * float(np.max(np.abs(f.aY)))


def test_long_double_is_wider_than_float64():
    """the truth is only a truth where np.longdouble carries more than 53 bits"""
    assert np.finfo(np.longdouble).nmant >= 63


@pytest.mark.parametrize("name", NAMES)
def test_the_two_bars_are_ordered(name):
    """the reference's own float64 error -- cho_solve and the device's formulation, five observation orders -- is at most 1/8 of the
    project's rule 1e-15 max(cond_2, 1e6) for every quantity: 8 x ref_error is the tighter bar, the rule the outer cap"""
    for ext in (False, True):
        d = cc.extended_data(name) if ext else cc.case_data(name)
        errs = cc.ref_errors(name, ext)
        r = cc.rule(d["cond"])
        print("%s%s: ref_error / rule  %s" % (name, " +1 row" if ext else "", {k: "%.1e" % (v / r) for k, v in errs.items()}))
        assert set(errs) == set(cc.WHATS)
        for k, v in errs.items():
            assert 0 < v <= r / 8, (name, ext, k, v, r)


@pytest.mark.parametrize("mutant", cc.MUTANTS)
def test_mutants_of_the_device_formulation_exceed_the_reach(mutant):
    """W rounded to float32; the last row of W dropped; W's last 64-row block from a model one observation shorter (a stale tile); k*
    with a relative exponent error of 1e-11; q accumulated in float32; alpha_Y from a factor with noise (1 + 1e-6): each is farther than
    8 x ref_error from the truth in mu or sigma^2 on at least one case"""
    caught = []
    for name in NAMES:
        d = cc.case_data(name)
        got = cc.shares(cc.truth_of(name)[0], cc.restate(d, "b", mutant=mutant, whats=("mu", "s2")))
        ratio = {k: v / (8.0 * cc.ref_error(name, k)) for k, v in got.items()}
        print("%s on %s: error / (8 ref_error)  %s" % (mutant, name, {k: "%.2g" % v for k, v in ratio.items()}))
        if max(ratio.values()) > 1.0:
            caught.append(name)
    assert caught, mutant

"""
tests/shift_reference.py (the yardstick of tests/test_gpu_shifted_inputs.py) on the CPU: the oracle returns the same bits at data
moved by an integer; the float64 restatement of the device's three exponent forms loses what DESIGN.md says it loses; and every
case of the GPU file is, by the reference alone, a model worth comparing against (it factors, its sampled candidates are not all
tails, the emulated error leaves room under the bars the GPU file holds).  CPU only.
"""
import numpy as np
import pytest

from oracle import oracle as orc
import shift_reference as sr

KINDS = [("ard", [.3, .33, .36, .3]), ("iso", [.3]), ("m3", [.45, 1.0]), ("m5", [.45, 1.0])]
SHIFTS = (-3, 94, 4096, -1048576)


def test_dyadic_points_and_integer_shifts():
    X0 = sr.dyadic(1, 50, 3)
    assert X0.shape == (50, 3) and np.all(X0 >= 0) and np.all(X0 < 1) and np.array_equal(X0 * 4096, np.round(X0 * 4096))
    sw = np.array([3.0, 2.5, 4.0])
    for sign in (1, -1):
        for lo, hi in (sr.INSIDE, sr.OUTSIDE):
            t = sr.shift_for(X0, sw, lo, hi, sign=sign)
            assert t == int(t) and np.sign(t) == sign and lo <= sr.row_bound(X0 + t, sw) <= hi
            assert np.array_equal((X0 + t) - t, X0)
    # the per-dimension bound of the NLML grid is never below the per-row one, and several theta rows take the largest
    sws = np.array([[3.0, 2.5, 4.0], [1.0, 1.0, 1.0]])
    t = sr.shift_for(X0, sws, 0.9e5, 0.99e5, sign=-1, bound=sr.dim_bound)
    assert 0.9e5 <= sr.dim_bound(X0 + t, sws) <= 0.99e5 and sr.row_bound(X0 + t, sws) <= sr.dim_bound(X0 + t, sws)
    with pytest.raises(AssertionError):
        sr.shift_for(X0, sw * 100, 0.999e5, 1.0e5)             # a band no integer reaches


@pytest.mark.parametrize("with_prior", [False, True])
@pytest.mark.parametrize("kind,hyper", KINDS)
def test_oracle_is_bit_equal_under_an_integer_shift(kind, hyper, with_prior):
    """the reference of every shifted case: native sweep, Python-path posterior and the NLML at (X0 + t, C0 + t) -- the prior's
    lower bound moved along -- are the bits of the unshifted run"""
    N, D = 200, 4
    X0 = sr.dyadic(11, N, D); Y = sr.targets(12, X0); C0 = sr.candidates(13, X0, 64)
    rs = np.random.RandomState(14)
    pr = (rs.rand(4, D), rs.randn(4), 2.0, np.full(D, -.125), np.full(D, 2.0)) if with_prior else None
    for noise in (.1, 1e-3):
        def run(t):
            prior = None if pr is None else orc.Prior(pr[0], pr[1], pr[2], pr[3] + t, pr[4])
            ogp = orc.GP(orc.Kern(kind, hyper), X0 + t, Y, noise=noise, prior=prior)
            o = orc.sweep_native(ogp, C0 + t, orc.ACQ_EI, .01)
            mu, s2 = ogp.posteriors(C0 + t)
            nl = orc.marginal_likelihood(orc.Kern(kind, hyper), X0 + t, Y, 1, compute_gradient=False, noise=noise)
            return o["mu"], o["s2"], o["acq"], np.array([o["best_idx"]]), mu, s2, ogp.L, np.array([nl])
        base = run(0)
        assert (base[1] < .5).sum() >= 10
        for t in SHIFTS:
            for a, b in zip(run(t), base):
                assert np.array_equal(a, b), (kind, noise, t)


def test_what_each_form_loses_against_the_distance_from_the_origin():
    """the table of DESIGN.md ("inputs away from the origin"): N = 300, D = 4, length scale 0.3, at the unit cube, at the edge of the
    sweeps' guard (2e4), at the edge of the grid's (1e5, the sweeps' former one), at t = 4096 and at t = -2^20"""
    N, D = 300, 4
    X0 = sr.dyadic(21, N, D); C0 = sr.candidates(22, X0, 200); Y = sr.targets(23, X0)
    sw = sr.scale_of("iso", [.3], D)
    edge = sr.shift_for(X0, sw, 0.95 * sr.GUARD, sr.GUARD)
    edge5 = sr.shift_for(X0, sw, 0.95e5, 1.0e5)
    rows = []
    for t in (0, edge, edge5, 4096, -2 ** 20):
        for kind, hyper in (("iso", [.3]), ("m3", [.3, 1.0])):
            for noise in (.1, 1e-3):
                s, m = sr.s2_deviation(X0, C0, t, kind, hyper, noise), sr.mu_deviation(X0, Y, C0, t, kind, hyper, noise)
                rows.append((t, kind, noise, s, m))
                print("t %8d  max|x~|^2 %.1e  %-3s noise %-5g  s2: scaled-first %.1e dot %.1e   mu / its bar: scaled-first %.1e dot %.1e" %
                      (t, sr.row_bound(X0 + t, sw), kind, noise, s["scaled"], s["dot"], m["scaled"], m["dot"]))
    for t, kind, noise, s, m in rows:
        assert s["scaled"] < 1.25e-7 and m["scaled"] < 0.125          # the difference form holds the suite's bars out to 2^20, 8 x under
        if t == 0:
            assert s["scaled"] < 1e-11 and s["dot"] < 1e-10 and m["dot"] < 1e-5
        elif t == edge:
            assert s["dot"] < 1.25e-8 and m["dot"] < 0.0125           # the sweeps' edge: a factor of 80 at this size
        elif t == edge5:
            assert s["dot"] < 1.25e-7 and m["dot"] < 0.125            # the former edge: still fine at 300 rows -- not at 1100 (below)
        elif noise == 1e-3:
            assert s["dot"] > 1e-6 and m["dot"] > 1.0                 # why there is a guard at all
    # the mean's error is absolute, (error of the exponent) x sum_i |k*_i alpha_i|, and grows with the model: at 1100 rows the former
    # edge leaves no factor of two, the present one a factor of four
    c = sr.sweep_case("m3_d32_n1100")
    m = sr.mu_deviation(c["X0"], c["Y"], c["C0"][:sr.EMU_M], sr.shift_for(c["X0"], c["sw"], 0.80e5, 0.98e5, sign=-1), c["kind"], c["hyper"], c["noise"])
    assert m["dot"] > 0.4 and sr.sweep_case_mu_deviation("m3_d32_n1100")["dot"] < 0.125
    # the NLML of a dot-form K just inside the grid's edge: beyond the unit cube's 1e-10, harmless to an optimiser
    n0, n1 = sr.nlml_deviation(X0, Y, 0, "iso", [.3], 1e-3), sr.nlml_deviation(X0, Y, edge5, "iso", [.3], 1e-3)
    assert n0["dot"] < 1e-10 and n1["scaled"] < 1e-10 and n1["dot"] < 1.25e-7


def _sampled(c, idx, t=0):
    ogp = orc.GP(orc.Kern(c["kind"], c["hyper"]), c["X0"] + t, c["Y"], noise=c["noise"])          # (np.linalg.cholesky raises if it does not factor)
    return orc.sweep_native(ogp, c["C0"][idx] + t, orc.ACQ_EI, .01)


@pytest.mark.parametrize("name", [c[0] for c in sr.SWEEP_CASES])
def test_sweep_cases_by_the_reference_alone(name):
    c = sr.sweep_case(name)
    assert sr.INSIDE[0] <= sr.row_bound(c["X0"] + c["t_in"], c["sw"]) <= sr.INSIDE[1]
    assert sr.OUTSIDE[0] <= sr.row_bound(c["X0"] + c["t_out"], c["sw"]) <= sr.OUTSIDE[1]
    assert np.sign(c["t_in"]) == -np.sign(c["t_out"])
    idx = sr.sample_index(sr.SWEEP_M, [1, 7])
    o = _sampled(c, idx)
    assert 55 <= len(idx) <= 70 and (o["s2"] < .5).sum() >= 10 and (o["acq"] > 1e-12).sum() >= 10
    for M in (3, 17, 40, 600, 4096):                             # every prefix the GPU file sweeps has its own sample
        sub = sr.sample_index(M, [1, 7])
        assert sub.max() == M - 1 and len(sub) <= 70
    dev = sr.sweep_case_deviation(name)
    print("%s: t_in %d t_out %d  emulated s2 deviation inside the guard: scaled-first %.2g, dot %.2g" % (name, c["t_in"], c["t_out"], dev["scaled"], dev["dot"]))
    assert dev["scaled"] < 1e-10 and dev["dot"] <= 1.25e-7       # 8 x the dot form's stays under 1e-6
    assert sr.measured_bar(dev["dot"] + dev["scaled"]) <= 1e-6
    mdev = sr.sweep_case_mu_deviation(name)
    print("%s: emulated deviation of the mean in units of its bar (1e-9 + 1e-6 |mu|): scaled-first %.2g, dot %.2g" % (name, mdev["scaled"], mdev["dot"]))
    assert mdev["scaled"] < 1e-2 and mdev["dot"] <= 0.25          # the mean's error is absolute and grows with the model: 4 x under its bar at these sizes


@pytest.mark.parametrize("kind", ["ard", "iso", "m3", "m5"])
def test_one_sweep_case_per_family_has_the_same_reference_bits_at_the_shifted_data(kind):
    name = [c[0] for c in sr.SWEEP_CASES if c[1] == kind][0]
    c = sr.sweep_case(name)
    idx = sr.sample_index(sr.SWEEP_M, [1, 7])
    o = _sampled(c, idx)
    for t in (c["t_in"], c["t_out"]):
        s = _sampled(c, idx, t)
        assert all(np.array_equal(o[k], s[k]) for k in ("mu", "s2", "acq")) and o["best_idx"] == s["best_idx"]


@pytest.mark.parametrize("name", [c[0] for c in sr.FAR_CASES])
def test_far_cases_by_the_reference_alone(name):
    c = sr.far_case(name)
    idx = sr.sample_index(sr.SWEEP_M, [1, 7])
    o = _sampled(c, idx)
    assert (o["s2"] < .5).sum() >= 10 and (o["acq"] > 1e-12).sum() >= 10
    assert sr.row_bound(c["X0"] + c["t"], c["sw"]) > 1e7          # far beyond the guard: difference routes only
    dev = sr.s2_deviation(c["X0"], c["C0"][:sr.EMU_M], c["t"], c["kind"], c["hyper"], c["noise"])
    print("%s: emulated s2 deviation, scaled-first %.2g (dot, never run there: %.2g)" % (name, dev["scaled"], dev["dot"]))
    assert dev["scaled"] <= 2.5e-7                                # the difference form keeps 4 x under 1e-6 out to 2^20


@pytest.mark.parametrize("name", [c[0] for c in sr.PULLIN_CASES])
def test_pullin_cases_by_the_reference_alone(name):
    """far candidates: k* underflows for every family (Matern-3/2 last), so mu is the prior's mean at the REAL point (0 without
    one) and s2 = 1 + noise, exactly; the near ones keep the comparison alive"""
    c = sr.pullin_case(name)
    X = c["X0"] + c["t"]
    assert sr.INSIDE[0] <= sr.row_bound(X, c["sw"]) <= sr.INSIDE[1]
    r2 = np.sum((c["C"][c["far"]] * c["sw"]) ** 2, axis=1)
    np.testing.assert_allclose(r2, np.repeat(sr.PULLIN_R2, 16), rtol=1e-12)
    assert (r2 < sr.PULL_IN).sum() == 16 and (r2 > sr.PULL_IN).sum() == 48
    # towards the data: the closest approach of all, still hundreds of length scales
    gap = np.sqrt(np.min(np.sum(((X[:, None, :] - c["C"][c["far"]][None, :, :]) * c["sw"]) ** 2, axis=2)))
    assert gap > np.sqrt(min(sr.PULLIN_R2)) - np.sqrt(sr.GUARD) - 1e-6          # hundreds of length scales
    prior = None if c["prior"] is None else orc.Prior(*c["prior"])
    ogp = orc.GP(orc.Kern(c["kind"], c["hyper"]), X, c["Y"], noise=c["noise"], prior=prior)
    idx = sr.sample_index(sr.SWEEP_M, np.r_[1, 7, c["far"]])
    o = orc.sweep_native(ogp, c["C"][idx], orc.ACQ_EI, .01)
    far = np.isin(idx, c["far"])
    assert np.all(o["s2"][far] == 1.0 + c["noise"])
    if prior is None:
        assert np.all(o["mu"][far] == 0.0)
    else:
        m = np.array([prior.mu(x) for x in c["C"][idx][far]])
        assert np.array_equal(o["mu"][far], m) and (np.abs(m) > 1e-3).sum() >= 16           # alive where the pull-in moves the point
        pulled = c["C"][idx][far] * np.minimum(1.0, np.sqrt(sr.PULL_IN / r2))[:, None]
        mp = np.array([prior.mu(x) for x in pulled])
        assert (np.abs(mp - m) > 1e-6 * np.abs(m)).sum() >= 16                              # ... and would be wrong at the pulled-in one
    assert (o["s2"][~far] < .5).sum() >= 10 and (o["acq"] > 1e-12).sum() >= 10


def test_extension_case_by_the_reference_alone():
    c = sr.extend_case()
    assert sr.INSIDE[0] <= sr.row_bound(c["X"], c["sw"]) <= sr.INSIDE[1]
    assert sr.row_bound(c["p_in"][None, :], c["sw"]) <= sr.GUARD < 1.1 * sr.GUARD <= sr.row_bound(c["p_out"][None, :], c["sw"]) <= 1.2 * sr.GUARD
    rows = np.vstack([c["X"], c["p_in"], c["p_out"]])
    assert np.array_equal(rows * 8192, np.round(rows * 8192))               # every row on a dyadic grid: exact in fp64
    ogp = orc.GP(orc.Kern(c["kind"], c["hyper"]), rows, c["Y"], noise=c["noise"])
    idx = sr.sample_index(len(c["C"]), [1, 7])
    o = orc.sweep_native(ogp, c["C"][idx], orc.ACQ_EI, .01)
    assert (o["s2"] < .5).sum() >= 10 and (o["acq"] > 1e-12).sum() >= 10


@pytest.mark.parametrize("name", [c[0] for c in sr.NLML_CASES])
def test_nlml_cases_by_the_reference_alone(name):
    c = sr.nlml_case(name)
    X = c["X0"] + c["t"]
    sws = np.array([sr.scale_of(c["kind"], list(th), c["D"]) for th in c["thetas"]])
    assert sr.dim_bound(X, sws) <= sr.NLML_GUARD < sr.dim_bound(X, np.array([sr.scale_of(c["kind"], list(th), c["D"]) for th in c["thetas_over"]]))
    for th in c["thetas_over"]:
        a = orc.marginal_likelihood(orc.Kern(c["kind"], th), c["X0"], c["Y"], 1, compute_gradient=False, noise=c["noise"])
        b = orc.marginal_likelihood(orc.Kern(c["kind"], th), X, c["Y"], 1, compute_gradient=False, noise=c["noise"])
        assert np.isfinite(a) and a == b
    dev = sr.nlml_case_deviation(name)
    print("%s: t %d  emulated NLML deviation of the dot form %.2g" % (name, c["t"], dev))
    assert sr.measured_bar(dev, 1e-9) <= 1e-6

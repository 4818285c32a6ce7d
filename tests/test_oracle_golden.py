"""
Pin the CPU oracle (oracle/) against the golden vectors produced by the real
reference (tests/golden/make_golden.py) and, when present, against the
reference's own compiled C++ (oracle/_ref/libego.so).  CPU only.
"""
import numpy as np

from conftest import load_golden, kern_from_golden, synth

RT = 1e-9   # oracle-vs-reference tolerance (same algorithm, same fp64; only summation order differs)
REF_ACQMAX = ((0, .01), (1, .05), (2, 1.3))   # (acquisition, parameter) of the acqmaxGP runs held against the compiled reference: EI, PI, UCB


def close(a, b, rtol=RT, atol=1e-12):
    np.testing.assert_allclose(a, b, rtol=rtol, atol=atol)


def test_g9_lhc_bit_exact(oracle):
    g = load_golden("g9_lhc")
    for seed, n in ((22, 5), (23, 5), (0, 10), (7, 12)):
        got = np.array(oracle.lhc_sample(g["s%d_bounds" % seed].tolist(), n, seed=seed))
        assert np.array_equal(got, g["s%d" % seed])


def test_g1_demo(oracle):
    g = load_golden("g1_demo")
    k = oracle.Kern("ard", g["hyper"])
    gp = oracle.GP(k, g["X"], g["Y"], noise=float(g["noise"]))
    close(gp.R, g["R"]); close(gp.L, g["L"])
    mu, s2 = gp.posteriors(g["probe"])
    close(mu, g["post"][:, 0]); close(s2, g["post"][:, 1])
    # known answers quoted in SURVEY 8(c)
    close(mu[0], 0.8556561848875622); close(s2[0], 0.29460407402037647)
    close(mu[1], 0.0, atol=1e-12); close(s2[1], 1.1)
    opt, optx, ns = oracle.acqmax_native(gp, g["bounds"].tolist(), oracle.ACQ_EI, parm=float(g["xi"]))
    close(opt, g["c_opt"]); close(optx, g["c_optx"])
    assert ns == 17          # dim-0-fixed stall of the native DIRECT
    close(opt, 0.14274080649281737)


def test_g2_marginal_likelihood(oracle):
    g = load_golden("g2_hyper")
    X, Y = g["X"], g["Y"]
    for name, kind, nh in (("ard", "ard", 3), ("sviso", "sviso", 2), ("m3", "m3", 2), ("m5", "m5", 2)):
        k = oracle.Kern(kind, g[name + "_hyper"])
        for h in range(nh):
            close(k.derivative(X, h), g["%s_d%d" % (name, h)])
        for tag, noise in (("n0", 0.0), ("n1", 1e-3)):
            v, d = oracle.marginal_likelihood(k, X, Y, nh, True, noise=noise)
            close(v, g["%s_%s_nlml" % (name, tag)]); close(d, g["%s_%s_grad" % (name, tag)], rtol=1e-7)
            close(oracle.nlml_c(k, X, Y, noise=noise), v)
    # Rasmussen gpml targets quoted by the reference's tests (ego/unittest_GP.py:196-198,234-236,263-272)
    close(g["ard_n0_nlml"], 5.8404, rtol=1e-4); close(g["sviso_n0_nlml"], 7.514, rtol=1e-4)
    close(g["m3_n0_nlml"], 5.1827, rtol=1e-4); close(g["m5_n0_nlml"], 5.6652, rtol=1e-4)
    close(g["m5_n0_grad"], [4.4782, -4.8737], rtol=1e-4)


def _gp_from_case(oracle, g, name):
    p = name + "/"
    k = kern_from_golden(oracle, g[p + "ktype"], g[p + "hyper"])
    prior = None
    if p + "pmeans" in g.files:
        prior = oracle.Prior(g[p + "pmeans"], g[p + "pbeta"], float(g[p + "ptheta"]), g[p + "plowerb"], g[p + "pwidth"])
    return oracle.GP(k, g[p + "X"], g[p + "Y"], noise=float(g[p + "noise"]), prior=prior), p


def test_g3_seeded_cases(oracle):
    g = load_golden("g3_cases")
    for name in g["names"]:
        gp, p = _gp_from_case(oracle, g, str(name))
        D = gp.X.shape[1]
        bounds = g[p + "bounds"].tolist()
        close(gp.R, g[p + "R"]); close(gp.L, g[p + "L"], rtol=1e-8)
        probe = g[p + "probe"]
        mu, s2 = gp.posteriors(probe)
        close(mu, g[p + "post"][:, 0], rtol=1e-8, atol=1e-10); close(s2, g[p + "post"][:, 1], rtol=1e-8)
        if gp.prior is not None:
            close([gp.prior.mu(q) for q in probe], g[p + "prior_mu"])
        ymax = gp.Y.max()
        sig = np.sqrt(s2)
        close(oracle.acq_value(oracle.ACQ_EI, oracle.ERF_NR, mu, sig, ymax, .01), g[p + "ei_py"], rtol=1e-7, atol=1e-13)
        close(oracle.acq_value(oracle.ACQ_PI, oracle.ERF_NR, mu, sig, ymax, .01), g[p + "pi_py"], rtol=1e-7, atol=1e-13)
        close(oracle.acq_value(oracle.ACQ_UCB, oracle.ERF_NR, mu, sig, ymax,
                               oracle.ucb_coef_py(len(gp.Y), D, .1, .2)), g[p + "ucb_py"], rtol=1e-8)
        close(oracle.ucb_parm_native(len(gp.Y), D, .1, .2), g[p + "ucb_parm"])
        # native flavour (libm erf, invR double matvec, clamp 1e-8)
        for acq, key, parm in ((oracle.ACQ_EI, "ei_c", .01), (oracle.ACQ_PI, "pi_c", .01),
                               (oracle.ACQ_UCB, "ucb_c", float(g[p + "ucb_parm"]))):
            sw = oracle.sweep_native(gp, probe, acq, parm)
            close(sw["acq"], g[p + key], rtol=1e-8, atol=1e-13)
        # optimisers: native DIRECT on the native objective must reproduce maximize*
        for acq, key, parm in ((oracle.ACQ_EI, "max_ei", .01), (oracle.ACQ_PI, "max_pi", .01),
                               (oracle.ACQ_UCB, "max_ucb", float(g[p + "ucb_parm"]))):
            opt, optx, _ = oracle.acqmax_native(gp, bounds, acq, parm, maxiter=10)
            close(opt, g[p + key][0], rtol=1e-8, atol=1e-12); close(optx, g[p + key][1:], rtol=1e-9)
        opt, optx, _ = oracle.acqmax_native(gp, bounds, oracle.ACQ_EI, .01)
        close(opt, g[p + "max_ei50"][0], rtol=1e-8, atol=1e-12); close(optx, g[p + "max_ei50"][1:], rtol=1e-9)
        # Python objective (NR erf, Cholesky posterior) through both DIRECT implementations
        def negei(x):
            m, v = gp.posterior(np.asarray(x, dtype=float))
            return -oracle.acq_value(oracle.ACQ_EI, oracle.ERF_NR, m, np.sqrt(v), ymax, .01)[0]
        f, x, _ = oracle.cdirect(negei, bounds, maxiter=10)
        close(f, g[p + "cdirect_ei"][0], rtol=1e-7, atol=1e-12); close(x, g[p + "cdirect_ei"][1:], rtol=1e-9)
        f, x, _ = oracle.direct_py(negei, bounds, maxiter=10)
        close(f, g[p + "direct_ei"][0], rtol=1e-7, atol=1e-12); close(x, g[p + "direct_ei"][1:], rtol=1e-9)


def shekel5(g):
    A, C = g["shekel_A"], g["shekel_C"]
    return lambda x: -sum(1. / (np.dot(x - a, x - a) + c) for a, c in zip(A, C))


def test_g4_direct_known_answers(oracle):
    g = load_golden("g4_direct")
    f = shekel5(g)
    b = g["shekel_bounds"].tolist()
    fm, xm, _ = oracle.cdirect(f, b, maxiter=20)
    close(np.r_[fm, xm], g["shekel_cdirect"])
    assert abs(fm - (-10.1532)) < 1e-3 and np.all(np.abs(xm - 4.0) < 1e-3)   # ego/unittest_IBO.py:76-82
    fm, xm, _ = oracle.direct_py(f, b, maxiter=20)
    close(np.r_[fm, xm], g["shekel_direct"])

    def foo(x, a1, a2):
        return -np.sum(np.sin(np.array(x) * a1) + np.array(x) * a2)
    b3 = [[0., 5.]] * 3
    fm, xm, _ = oracle.cdirect(foo, b3, args=[3.0, 0.0], maxiter=10); close(np.r_[fm, xm], g["foo_c1"])
    fm, xm, _ = oracle.cdirect(foo, b3, args=[-2.0, 2.0], maxiter=10); close(np.r_[fm, xm], g["foo_c2"])
    fm, xm, _ = oracle.direct_py(foo, b3, args=[3.0, 0.0], maxiter=20); close(np.r_[fm, xm], g["foo_d1"])
    # fixed-dimension sample counts, incl. the dim-0 stall
    foo3 = lambda x: float(np.sum((np.array(x) - .3) ** 2))
    for row, bb in zip(g["fixed_counts"], ([[0., 1.]] * 3, [[0., 1.], [.5, .5], [0., 1.]], [[.5, .5], [0., 1.], [0., 1.]])):
        fm, xm, ns = oracle.cdirect(foo3, bb, maxiter=50, maxsample=10000)
        assert ns == int(row[0])
        close(np.r_[fm, xm], row[1:])


def test_g6_synthetic_sweeps(oracle):
    g = load_golden("g6_sweeps")
    for name in g["names"]:
        p = str(name) + "/"
        N, D, M, seed = int(g[p + "N"]), int(g[p + "D"]), int(g[p + "M"]), int(g[p + "seed"])
        X, Y = synth(seed, N, D)
        cand = np.random.RandomState(100 + seed).rand(M, D)
        k = kern_from_golden(oracle, g[p + "ktype"], g[p + "hyper"])
        gp = oracle.GP(k, X, Y, noise=.1)
        mu, s2 = gp.posteriors(cand)
        close(mu, g[p + "mu"], rtol=1e-8, atol=1e-10); close(s2, g[p + "s2"], rtol=1e-8)
        sig = np.sqrt(s2); ymax = Y.max()
        close(oracle.acq_value(oracle.ACQ_EI, oracle.ERF_NR, mu, sig, ymax, .01), g[p + "ei_py"], rtol=1e-7, atol=1e-13)
        close(oracle.acq_value(oracle.ACQ_PI, oracle.ERF_NR, mu, sig, ymax, .01), g[p + "pi_py"], rtol=1e-7, atol=1e-13)
        if p + "ei_c" in g.files:
            sub = slice(0, min(M, 128))
            sw = oracle.sweep_native(gp, cand[sub], oracle.ACQ_EI, .01)
            close(sw["acq"], g[p + "ei_c"][sub], rtol=1e-7, atol=1e-13)
            assert sw["best_idx"] == int(np.argmax(g[p + "ei_c"][sub]))
            close(oracle.sweep_native(gp, cand[sub], oracle.ACQ_PI, .01)["acq"], g[p + "pi_c"][sub], rtol=1e-7, atol=1e-13)
            close(oracle.sweep_native(gp, cand[sub], oracle.ACQ_UCB, 1.5)["acq"], g[p + "ucb_c"][sub], rtol=1e-8)


def test_g7_preference_gp(oracle):
    g = load_golden("g7_prefs")
    for name in g["names"]:
        p = str(name) + "/"
        prefs = [(v, u, d) for v, u, d in zip(g[p + "pref_v"], g[p + "pref_u"], g[p + "pref_d"])]
        k = oracle.Kern("ard", g[p + "hyper"])
        # parity boundary sits after the MAP: feed the reference's Y_map
        gp = oracle.pref_fit(k, prefs, noise=.1, Y_map=g[p + "Y"])
        close(gp.X, g[p + "X"], rtol=0, atol=0)
        close(gp.R, g[p + "R"]); close(gp.C, g[p + "C"], rtol=1e-7, atol=1e-10); close(gp.L, g[p + "L"], rtol=1e-7, atol=1e-10)
        mu, s2 = gp.posteriors(g[p + "probe"])
        close(mu, g[p + "post"][:, 0], rtol=1e-7, atol=1e-10); close(s2, g[p + "post"][:, 1], rtol=1e-7)
        sw = oracle.sweep_native(gp, g[p + "probe"], oracle.ACQ_EI, .01)
        close(sw["acq"], g[p + "ei_c"], rtol=1e-6, atol=1e-12)
        # the MAP itself: S is convex, our BFGS must reach the reference's objective value
        gp2 = oracle.pref_fit(k, prefs, noise=.1)
        S_ref = oracle.pref_S(g[p + "Y"], gp.inds, np.linalg.cholesky(gp.R))
        S_our = oracle.pref_S(gp2.Y, gp2.inds, np.linalg.cholesky(gp2.R))
        assert abs(S_ref - S_our) < 1e-4 * max(1.0, abs(S_ref))
        # gallery with the injected latin-hypercube samples
        gal, _ = oracle.fast_gallery(gp, g[p + "bounds"].tolist(), 4, list(g[p + "lhc"]))
        close(np.array(gal), g[p + "gallery"], rtol=1e-7, atol=1e-9)
        # the all-core form of the sample step (what the GPU tests run at 20 000 candidates) makes the same picks
        gal_f, _ = oracle.fast_gallery(gp, g[p + "bounds"].tolist(), 4, list(g[p + "lhc"]), fast=True)
        np.testing.assert_array_equal(np.array(gal_f), np.array(gal))


def test_g8_nlml(oracle):
    g = load_golden("g8_nlml")
    for N in (64, 256):
        X, Y = synth(5, N, 16)
        for th, v in zip(g["n%d_theta" % N], g["n%d_nlml" % N]):
            k = oracle.Kern("ard", th)
            close(oracle.nlml_c(k, X, Y, 1e-3), v, rtol=1e-9)
            close(oracle.marginal_likelihood(k, X, Y, 16, False, 1e-3), v, rtol=1e-9)
    X, Y = synth(5, 64, 16)
    v, d = oracle.marginal_likelihood(oracle.Kern("ard", g["n64_grad_theta"]), X, Y, 16, True, 1e-3)
    close(v, g["n64_grad_nlml"]); close(d, g["n64_grad"], rtol=1e-7, atol=1e-10)


def test_oracle_matches_compiled_reference(oracle):
    """oracle/_ref/libego.so = the reference's own C++; compare DIRECT runs sample-for-sample.  Without oracle/_ref (no
    reference sources to build it from) the compiled reference's answers come from tests/golden/g11_ref_direct.npz."""
    ref = oracle.RefLib() if oracle.RefLib.available() else None
    stored = load_golden("g11_ref_direct")
    g = load_golden("g3_cases")
    for name in g["names"]:
        gp, p = _gp_from_case(oracle, g, str(name))
        bounds = g[p + "bounds"].tolist()
        for acq, parm in REF_ACQMAX:
            o, ox, _ = oracle.acqmax_native(gp, bounds, acq, parm, maxiter=15)
            if ref is not None:
                r, rx = ref.acqmax(gp, bounds, acq, parm, maxiter=15)
            else:
                r, rx = stored["acqmax/%s/%d" % (name, acq)][0], stored["acqmax/%s/%d" % (name, acq)][1:]
            close(o, r, rtol=1e-12, atol=1e-14); close(ox, rx, rtol=1e-13)
    g4 = load_golden("g4_direct")
    f = shekel5(g4)
    a = oracle.cdirect(f, g4["shekel_bounds"].tolist(), maxiter=25)
    if ref is not None:
        b = ref.direct(f, g4["shekel_bounds"].tolist(), maxiter=25)
    else:
        s = stored["shekel_direct"]
        b = (s[0], s[1:-1], s[-1])
    assert a[2] == b[2]
    close(np.r_[a[0], a[1]], np.r_[b[0], b[1]], rtol=0, atol=0)


def test_best_effort_cpu_sweep_matches_reference_shaped_sweep(oracle):
    """orc_sweep_fast (bench.py's all-core CPU leg: alpha cached, triangular L^-1, OpenMP) computes the same
    posterior + EI/UCB as the reference-shaped orc_sweep_native"""
    from conftest import synth
    X, Y = synth(5, 96, 3)
    gp = oracle.GP(oracle.Kern("ard", [.3, .4, .5]), X, Y, noise=.1)
    cand = np.random.RandomState(6).rand(300, 3)
    for acq, parm in ((oracle.ACQ_EI, .01), (oracle.ACQ_UCB, .3)):
        a = oracle.sweep_native(gp, cand, acq, parm)
        b = oracle.sweep_fast(gp, cand, acq, parm)
        assert np.allclose(a["acq"], b["acq"], rtol=1e-8, atol=1e-13)
        assert a["best_idx"] == b["best_idx"]

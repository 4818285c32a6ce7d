"""
PrefGaussianProcess.addPreferences end to end against tests/pref_reference.py: the MAP that _map_newton returns against the unique
minimiser of the functional, computed independently in long double, and every model step after it (point numbering, order fix-up,
C with the regulariser's identities, L = chol(R + C^-1), posterior, EI, addObservationPoint) against the reference's steps restated
in NumPy and the oracle.

The MAP is captured with monkeypatch around PrefGaussianProcess._map_newton (its return value, before the order fix-up, and its
start vector); Newton steps are counted by wrapping _lib.lib.ibo_pref_newton_step.  The product has no hook for either.

Cases: one spine that varies each axis against a default (GaussianKernel_ard, D = 2, 64 points in 32 disjoint pairs, noise 0.1,
degree 0, preferences that agree with sum sin(3 x), one addPreferences call), plus the named combinations:
    kernel      iso, ard (the default), m3, m5, svard, sviso
    dimensions  1, 6, 17, 33
    points      2, 63, 65, 129 (a random tree: pair k joins point k + 1 to an earlier one, so every point is in about two pairs),
                1024 (512 disjoint pairs in 6-D, C4's size), 150 points through the two-level order (fused2_min_nb = 3)
    noise       1e-2, 1e-3
    degree      mixed 0 / 1
    structure   star (one point in n - 1 pairs), chain, random tree; a ring 0 > 1 > ... > 63 > 0 with a cycle a > b > c > a across it,
                and the ring with one pair in both directions (the second copy names its point with a -0.0 coordinate): in a ring
                every point is the unpreferred one of some triple, so the order fix-up must stay silent (degrees mixed 0 / 1: a ring of
                equal weights has y* = 0 and every pair on the NR jump)
    flipped     10 %, 20 %, 30 % of the preferences of a random tree reversed (the order fix-up fires in the last two)
    calls       the default's preferences in three calls (warm start checked), a second call that repeats an earlier triple
    negative weights (noise <= 1e-2, flipped preferences, random pairs as in the issue's probes): neg-n40-noise1e-2,
                neg-n40-noise1e-3, neg-n100-noise1e-3-degrees, and traced-stall (30 points in 1-D, length scale 0.1, noise 1e-3, 30 %
                flipped: the case in which the parent's line search spun to maxit on the NumPy restatement)
    No case was found in which the reference's own cholesky(R + inv(C)) fails and k = 1 .. 10 identities mend it: of 400 random sets
    (noise 1e-2 .. 1e-4, 10 - 40 % flipped, 20 - 100 points, 302 of them with negative weights) and 900 more along two scans of the
    noise, every one factored with no identity or (11 sets, all at noise 1e-4) with none of the eleven: the negative eigenvalues of C
    are 1e3 .. 1e5 in size, an identity does not move them.  test_pref_device_steps_on_every_route (diag = -1) stays the only cover
    of a regulariser that succeeds; test_reference_cannot_factor_and_neither_can_the_product below walks the whole loop.

What is asserted (every bound is computed from the reference; none from the product's output):
  (a) r = grad_stated(Y) in long double: |r|_inf <= 1e-9 max(1, |Y|_inf) + e_fp, e_fp = 2 sqrt(n) u (|W^T||W||Y|)_inf   [stop rule]
  (b) |Y - y*|_2 <= 1.01 |H*^-1|_2 (|r|_2 + m), m = |grad_stated(y*)|_2; and the first-order form
      |Y - y1|_inf <= 1.01 |H*^-1|_inf (|r|_inf + |grad_stated(y1)|_inf) with y1 = y* - H*^-1 grad_stated(y*)
  (c) S_ref(Y) - S_ref(y*) <= Delta(Y) + Delta(y*) + r^T H*^-1 r / 2
  (d) calls of ibo_pref_newton_step <= steps of the reference's Newton iteration from the same start + 3
  (e) numbering, fix-up, C (identities included), L, posterior at 40 points, native EI, addObservationPoint twice (1 point, then 3)
  (f) three calls: (a) - (c) against the y* of the full set, GP.X in the numbering of the full set, every warm start as :408-427
  (g) negative weights: the reference has a weight < 0 and adds no identity; the product gives the reference's model

Every case prints what it measured beside what it allowed (run with -s).  Worst measured with the two device calls of _map_newton
replaced by NumPy (R^-1 y as W^T (W y) in float64, the Newton solve by LAPACK), all single-call cases: (a) |r|_inf 1.2e-9 of 1.2e-9
allowed (|Y|_inf 1.2); (b) |Y - y*|_2 9.6e-7 of 2.3e-4 (1024 points), |Y - y1|_inf 9.6e-10 of 1.1e-7; (c) S gap 4.9e-14 of 1e-6 .. 2e-5;
(d) 3 - 5 steps where the reference took 3 - 6.  Reference float64 accuracy at noise 1e-3 (20 negative weights): C^-1 1.9e-14.  Figures
from an MI355X have not been recorded yet; the cases print them.
"""
import ctypes

import numpy as np
import pytest
from scipy.linalg import solve_triangular

import pref_reference as pr

pytestmark = pytest.mark.gpu

RT = 1e-6
ACQ_ATOL = 1e-12
U = 2.0 ** -53
LD = np.longdouble


@pytest.fixture(scope="module")
def ibo():
    import ibo_amd
    from ibo_amd import _lib
    if _lib.device_count() < 1:
        pytest.fail("no GPU visible: the product has no CPU fallback")
    err = ctypes.c_double()
    _lib.check(_lib.lib.ibo_selftest_mfma(0, ctypes.byref(err)))
    return ibo_amd


# ------------------------------------------------------------------------------------------------ cases
def hyper_of(kind, D):
    """length scales ~ sqrt(D) / 2 (as test_gpu_linalg_entries.kern_args), magnitude 0.9 where the kernel has one"""
    ls = 0.5 * np.sqrt(D) * np.linspace(.8, 1.2, D)
    if kind == "ard":
        return list(ls)
    if kind == "svard":
        return list(ls) + [.9]
    if kind == "iso":
        return [float(ls.mean())]
    return [float(ls.mean()), .9]


def our_kernel(kind, hyper):
    from ibo_amd.gaussianprocess import kernel as K
    cls = dict(ard=K.GaussianKernel_ard, iso=K.GaussianKernel_iso, m3=K.MaternKernel3, m5=K.MaternKernel5,
               svard=K.SVGaussianKernel_ard, sviso=K.SVGaussianKernel_iso)[kind]
    return cls(np.array(hyper, dtype=float))


def make_prefs(seed, n, D, structure="disjoint", flip=0.0, mixed=False, P=None):
    """(preference triples, [sizes of the addPreferences calls]) from a fixed seed"""
    rs = np.random.RandomState(seed)
    X = rs.rand(n, D)
    f = np.sin(3 * X).sum(1)
    extra = []
    if structure == "probe":                              # random pairs, drawn as the issue's probes draw them
        v = rs.randint(0, n, P); u = (v + 1 + rs.randint(0, n - 1, P)) % n
    elif structure == "disjoint":
        v = np.arange(0, n, 2); u = v + 1
    elif structure == "star":
        v = np.zeros(n - 1, dtype=int); u = np.arange(1, n)
    elif structure == "chain":
        v = np.arange(n - 1); u = v + 1
    elif structure == "tree":
        u = np.arange(1, n); v = np.array([rs.randint(0, k) for k in u])
    else:                                                 # cycle, both: a ring, so every point is the unpreferred one of some triple
        v = np.arange(n); u = (v + 1) % n
    ring = structure in ("cycle", "both")
    sw = (f[v] < f[u]) & (not ring)
    v, u = np.where(sw, u, v), np.where(sw, v, u)
    fl = rs.rand(len(v)) < flip
    v, u = np.where(fl, u, v), np.where(fl, v, u)
    deg = rs.randint(0, 2, len(v)) if mixed else np.zeros(len(v), dtype=int)
    prefs = [(X[a].copy(), X[b].copy(), int(d)) for a, b, d in zip(v, u, deg)]
    if structure == "cycle":
        extra = [(X[5].copy(), X[9].copy(), 0), (X[9].copy(), X[20].copy(), 0), (X[20].copy(), X[5].copy(), 0)]
    if structure == "both":
        X[0, 0] = 0.0
        prefs = [(X[a].copy(), X[b].copy(), int(d)) for a, b, d in zip(v, u, deg)]
        minus = X[0].copy(); minus[0] = -0.0
        extra = [(X[1].copy(), minus, 0)]                    # the ring has 0 > 1
    return prefs + extra


def case(id, kind="ard", D=2, n=64, noise=.1, seed=11, hyper=None, calls=None, min_nb=None, neg=False, fixup=None, **kw):
    return dict(id=id, kind=kind, D=D, n=n, noise=noise, seed=seed, hyper=hyper, calls=calls, min_nb=min_nb, neg=neg, fixup=fixup, kw=kw)


CASES = (
    [case("kernel-" + k, kind=k) for k in ("iso", "ard", "m3", "m5", "svard", "sviso")] +
    [case("dim-%d" % d, D=d) for d in (1, 6, 17, 33)] +
    [case("n-2", n=2), case("n-63", n=63, structure="tree"), case("n-65", n=65, structure="tree"),
     case("n-129", n=129, structure="tree"), case("n-1024-c4", n=1024, D=6),
     case("n-150-two-level", n=150, D=3, min_nb=3)] +
    [case("noise-1e-2", noise=1e-2), case("noise-1e-3", noise=1e-3), case("degree-mixed", mixed=True)] +
    [case("star", n=40, structure="star"), case("chain", structure="chain"), case("tree", structure="tree"),
     case("cycle", structure="cycle", mixed=True, fixup=0), case("both-directions", structure="both", mixed=True, fixup=0)] +
    [case("flipped-10", structure="tree", flip=.1, seed=21), case("flipped-20", structure="tree", flip=.2, seed=22, fixup="fires"),
     case("flipped-30", structure="tree", flip=.3, seed=23, fixup="fires")] +
    [case("three-calls", calls=(10, 12, 10)), case("repeated-triple", calls=(32, "repeat"))] +
    [case("neg-n40-noise1e-2", n=40, noise=1e-2, seed=3, hyper=[.3, .3], structure="probe", P=60, flip=.2, neg=True),
     case("neg-n40-noise1e-3", n=40, noise=1e-3, seed=4, hyper=[.3, .3], structure="probe", P=60, flip=.2, neg=True),
     case("neg-n100-noise1e-3-degrees", n=100, noise=1e-3, seed=5, hyper=[.3, .3], structure="probe", P=200, flip=.1, mixed=True,
          neg=True),
     case("traced-stall", n=30, D=1, noise=1e-3, seed=7, hyper=[.1], structure="probe", P=20, flip=.3, neg=True)])


def calls_of(c, prefs):
    """the lists of triples handed to the successive addPreferences calls"""
    if c["calls"] is None:
        return [prefs]
    out, at = [], 0
    for k in c["calls"]:
        if k == "repeat":
            out.append([prefs[3], prefs[0]] if len(out) else prefs)        # a call that repeats two earlier triples
        else:
            out.append(prefs[at:at + k]); at += k
    return out


# ------------------------------------------------------------------------------------------------ the bounds
def map_bounds(prob, start):
    """everything about the MAP that comes from the reference alone: y*, its Newton steps from `start`, H*^-1 and its norms,
    m = |grad_stated(y*)|_2, y1 = the first-order zero of the stated equation and its residual"""
    ystar, steps, H = prob.minimise(start)
    Hinv = np.linalg.inv(H)
    gs = prob.grad_stated(ystar)
    y1 = ystar - Hinv.astype(LD).dot(gs)
    return dict(ystar=ystar, steps=steps, Hinv=Hinv, n2=float(np.linalg.norm(Hinv, 2)), ninf=float(np.abs(Hinv).sum(1).max()),
                m=float(np.linalg.norm(gs)), y1=y1, g1=float(np.max(np.abs(prob.grad_stated(y1)))))


def fp_allowance(prob, Y):
    """e_fp of (a): the device forms R^-1 y as W^T (W y), W = L^-1, two triangular products of length <= n in float64.  Each
    computed product is (T + dT) x with |dT| <= gamma_n |T| (Higham, Accuracy and Stability, 3.5), so to first order
    |fl(W^T fl(W y)) - W^T W y| <= 2 gamma_n |W^T||W||y|: c = 2.  gamma_n = n u is the worst case, every rounding error pushing the
    same way; for errors that scatter, gamma_n becomes sqrt(n) u (Higham and Mary 2019, "A new approach to probabilistic rounding
    error analysis"), and that is what is allowed here: e_fp = 2 sqrt(n) u (|W^T||W||Y|)_inf.  On the 4100-row model of
    test_pref_device_steps_on_every_route, norm-wise, | |W^T||W||Y| | / |R^-1 Y| = 762 and this allowance is 2 * 64.03 * u * 762 =
    1.08e-11, 39 times the 2.8e-13 measured there (the worst-case n u form would be 2478 times it)."""
    W = solve_triangular(np.linalg.cholesky(prob.R64), np.eye(prob.n), lower=True)
    return 2 * np.sqrt(prob.n) * U * float(np.max(np.abs(W).T.dot(np.abs(W).dot(np.abs(np.asarray(Y, dtype=float))))))


def check_map(prob, Y, newton_calls, ref, jump, figures):
    """(a) - (d) for a captured MAP Y; figures collects what was measured beside what was allowed"""
    Y = np.asarray(Y, dtype=float)
    Yl = Y.astype(LD)
    r = prob.grad_stated(Yl)
    rinf, r2 = float(np.max(np.abs(r))), float(np.linalg.norm(r))
    # (b) first: its bound is the reach within which a pair's z may sit on the other side of the NR jump at Y than at y*
    # 1.01: the bounds use H* for the mean Hessian between Y and y*; over a distance of 1e-5 at most the weights rho change by a
    # relative 1e-5 |d log rho / dz| < 1e-4, and H >= R^-1 throughout, so one per cent covers the second-order term many times
    b2 = 1.01 * ref["n2"] * (r2 + ref["m"])
    d2 = float(np.linalg.norm(Yl - ref["ystar"]))
    binf = 1.01 * ref["ninf"] * (rinf + ref["g1"])
    dinf = float(np.max(np.abs(Yl - ref["y1"])))
    ja_g, ja_S, near = prob.jump_allowance(ref["ystar"], LD(b2), jump)
    a_bound = 1e-9 * max(1.0, float(np.max(np.abs(Y)))) + fp_allowance(prob, Y) + float(ja_g)
    gap = float(prob.S_ref(Yl) - prob.S_ref(ref["ystar"]))
    c_bound = float(prob.delta_nr(Yl) + prob.delta_nr(ref["ystar"])) + float(r.astype(float).dot(ref["Hinv"].dot(r.astype(float)))) / 2 \
        + float(ja_S)
    figures.update(a=(rinf, a_bound), b2=(d2, b2), binf=(dinf, binf), c=(gap, c_bound), d=(newton_calls, ref["steps"] + 3),
                   pairs_at_jump=near)
    print("    (a) |r|inf %.3e <= %.3e | (b) |Y-y*|2 %.3e <= %.3e, |Y-y1|inf %.3e <= %.3e | (c) S gap %.3e <= %.3e | (d) steps %d <= %d"
          " | pairs at the jump %d" % (rinf, a_bound, d2, b2, dinf, binf, gap, c_bound, newton_calls, ref["steps"] + 3, near))
    assert rinf <= a_bound, ("(a)", rinf, a_bound)
    assert d2 <= b2, ("(b) 2-norm", d2, b2)
    assert dinf <= binf + float(ja_g) * ref["ninf"], ("(b) first order", dinf, binf)
    assert gap <= c_bound, ("(c)", gap, c_bound)
    assert newton_calls <= ref["steps"] + 3, ("(d)", newton_calls, ref["steps"])


def expected_start(prevX, prevY, prob):
    """:408-427: a point keeps its latent value; a new one starts at the top of the current range if ever preferred, else the bottom"""
    if prevX is None:
        return prob.start()
    had = dict((tuple(x), y) for x, y in zip(prevX, prevY))
    top, bottom = max(prevY), min(prevY)
    return np.array([had.get(tuple(x), top if i in prob.preferred else bottom) for i, x in enumerate(prob.X)])


# ------------------------------------------------------------------------------------------------ the test
@pytest.mark.parametrize("c", CASES, ids=[c["id"] for c in CASES])
def test_pref_model_against_reference(ibo, oracle, monkeypatch, c):
    from ibo_amd import _lib
    from ibo_amd.acquisition import sweep
    from ibo_amd.gaussianprocess import PrefGaussianProcess
    kind, D, noise = c["kind"], c["D"], c["noise"]
    hyper = c["hyper"] or hyper_of(kind, D)
    prefs = make_prefs(c["seed"], c["n"], D, **c["kw"])
    _, jump = pr.nr_constants(m=3)

    captured = {}
    real_newton = PrefGaussianProcess._map_newton
    real_step = _lib.lib.ibo_pref_newton_step

    def newton(self, start, prefinds, *a, **k):
        captured["start"] = np.array(start, dtype=float)
        captured["steps"] = 0
        captured["Y"] = np.array(real_newton(self, start, prefinds, *a, **k), dtype=float)
        return captured["Y"].copy()

    def step(*a):
        captured["steps"] += 1
        return real_step(*a)

    monkeypatch.setattr(PrefGaussianProcess, "_map_newton", newton)
    monkeypatch.setattr(_lib.lib, "ibo_pref_newton_step", step)
    if c["min_nb"]:
        _lib.check(_lib.lib.ibo_set_option(b"fused2_min_nb", c["min_nb"]))
    try:
        GP = PrefGaussianProcess(our_kernel(kind, hyper), noise=noise)
        given, prevX, prevY = [], None, None
        for chunk in calls_of(c, prefs):
            given = given + list(chunk)
            GP.addPreferences(list(chunk))
            prob = pr.PrefProblem(kind, hyper, given, noise)
            # (e) numbering (a -0.0 coordinate included), (f) warm start
            assert np.array_equal(GP.X, prob.X) and np.array_equal(np.signbit(GP.X), np.signbit(prob.X))
            assert np.array_equal(captured["start"], expected_start(prevX, prevY, prob))
            prevX, prevY = np.array(GP.X), np.array(GP.Y)
        figures = {}
        ref = map_bounds(prob, captured["start"])
        print("\n  %s: n = %d, %d pairs, |Y|inf %.2f, reference Newton steps %d, |H*^-1|2 %.3g, m %.3e"
              % (c["id"], prob.n, len(prob.inds), float(np.max(np.abs(ref["ystar"]))), ref["steps"], ref["n2"], ref["m"]))
        check_map(prob, captured["Y"], captured["steps"], ref, jump, figures)

        # (e) the order fix-up: decided at y* with a margin of 1e-3, so rounding cannot flip its branch
        ys = ref["ystar"].astype(float)
        unpref = set(prob.u.tolist())
        movable = np.array([v not in unpref for v in prob.v])
        if movable.any():
            assert np.min(np.abs(ys[prob.v[movable]] - ys[prob.u[movable]])) >= 1e-3, "case too close to call: choose another seed"
        Yfix, fired = pr.order_fixup(captured["Y"], prob.inds)
        assert fired == pr.order_fixup(ys, prob.inds)[1]
        if c["fixup"] == 0:
            assert fired == 0
        if c["fixup"] == "fires":
            assert fired >= 1
        assert np.array_equal(GP.Y, Yfix)

        # (e), (g) the model steps on the product's own Y
        steps = pr.model_steps(prob, GP.Y)
        nneg = int((steps["w"] < 0).sum())
        if c["neg"]:
            assert nneg >= 1 and steps["identities"] == 0
        probe = np.random.RandomState(5).rand(40, D)
        acc = dict(Cinv=0.0, L=0.0, mu=0.0, s2=0.0)
        if noise <= 1e-2:                               # the reference's own float64 accuracy where weights reach 1e4 .. 1e6
            acc = pr.reference_accuracy(prob, steps, GP.Y, probe)
        bar_L, bar_mu, bar_s2 = max(1e-9, 10 * acc["L"]), max(1e-9, 10 * acc["mu"]), max(1e-12, 10 * acc["s2"])
        wmax = max(1.0, float(np.max(np.abs(steps["w"]))))
        eC = float(np.max(np.abs(GP.C - steps["C"])))
        eL = float(np.max(np.abs(np.tril(GP.L) - steps["L"])))
        ogp = pr.oracle_model(prob, GP.Y, steps["L"], steps["M"])
        mu, s2 = GP.posteriors(probe)
        omu, os2 = ogp.posteriors(probe)
        print("    (e) fix-up fired %d, negative weights %d, identities %d, max|w| %.3g | C %.2e (bar %.2e) L %.2e (bar %.2e) mu %.2e "
              "(bar %.2e) s2 %.2e | reference float64 accuracy: C^-1 %.2e L %.2e mu %.2e s2 %.2e"
              % (fired, nneg, steps["identities"], wmax, eC, 1e-9 * wmax, eL, bar_L, float(np.max(np.abs(mu - omu))), bar_mu,
                 float(np.max(np.abs(s2 - os2))), acc["Cinv"], acc["L"], acc["mu"], acc["s2"]))
        np.testing.assert_allclose(GP.C, steps["C"], rtol=RT, atol=1e-9 * wmax)      # one identity too many or too few: 1 on the diagonal
        np.testing.assert_allclose(GP.R, prob.R64, rtol=1e-12, atol=1e-14)
        np.testing.assert_allclose(np.tril(GP.L), steps["L"], rtol=RT, atol=bar_L)
        np.testing.assert_allclose(mu, omu, rtol=RT, atol=bar_mu)
        np.testing.assert_allclose(s2, os2, rtol=RT, atol=bar_s2)
        r = sweep(GP, probe, acq='ei', xi=.01, native=True, outputs=("acq",))
        o = oracle.sweep_native(ogp, probe, oracle.ACQ_EI, .01)
        np.testing.assert_allclose(r["acq"], o["acq"], rtol=RT, atol=max(ACQ_ATOL, 10 * acc["mu"]))

        # (e) addObservationPoint twice: one point, then three
        new = np.random.RandomState(6).rand(4, D)
        augX = prob.X
        for rows in (new[:1], new[1:]):
            GP.addObservationPoint(rows[0] if len(rows) == 1 else rows)
            augX = np.vstack([augX, rows])
            augR, augL = pr.add_observation(prob, steps, augX)
            assert np.array_equal(GP.augX, augX)
            np.testing.assert_allclose(GP.augR, augR, rtol=1e-12, atol=1e-14)
            np.testing.assert_allclose(np.tril(GP.augL), augL, rtol=RT, atol=bar_L)
            amu, as2 = GP.posteriors(probe)
            np.testing.assert_allclose(amu, omu, rtol=RT, atol=bar_mu)             # the mean keeps using L (:214-223)
            np.testing.assert_allclose(as2, pr.oracle_model(prob, GP.Y, augL, X=augX).posteriors(probe)[1], rtol=RT, atol=bar_s2)
    finally:
        if c["min_nb"]:
            _lib.check(_lib.lib.ibo_set_option(b"fused2_min_nb", 104))


def test_reference_cannot_factor_and_neither_can_the_product(ibo, capsys):
    """38 points in 1-D, noise 1e-4, 30 % of 80 preferences flipped: 22 negative weights, and R + inv(C + k I) has an eigenvalue of
    -3.7e-5 for every k = 0 .. 10 (computed here from the reference), so the reference's regulariser loop runs out and cholesky raises
    LinAlgError (:489-497).  The product must run the same eleven attempts and raise the same."""
    from ibo_amd.gaussianprocess import PrefGaussianProcess
    prefs = make_prefs(1049, 40, 1, structure="probe", P=80, flip=.3)
    prob = pr.PrefProblem("ard", [.1], prefs, 1e-4)
    ystar, _, _ = prob.minimise()
    Y, _ = pr.order_fixup(ystar.astype(float), prob.inds)
    w = pr.laplace_weights(prob, Y)
    C = np.eye(prob.n) * 5 + pr.pair_matrix(prob.n, prob.v, prob.u, w)
    worst = max(np.linalg.eigvalsh(prob.R64 + np.linalg.inv(C + k * np.eye(prob.n)))[0] for k in range(11))
    assert (w < 0).sum() >= 1 and worst < -1e-6                  # far from a tie: rounding cannot turn any attempt around
    with pytest.raises(np.linalg.LinAlgError):
        pr.model_steps(prob, Y)
    GP = PrefGaussianProcess(our_kernel("ard", [.1]), noise=1e-4)
    with pytest.raises(np.linalg.LinAlgError):
        GP.addPreferences(prefs)
    assert capsys.readouterr().out.count("adding regularizer") == 11


def test_newer_acquisitions_across_an_observation_point_and_more_preferences(ibo):
    """One preference model through addPreferences -> addObservationPoint -> addPreferences, with the knowledge gradient, q-EI and the
    constrained sweep read at every stage.  A preference GP is no plain fit (its factor is that of R + C^-1), so it stays out of
    tests/test_gpu_acquisition_sequences.py; what holds for it is what the families' own files pin on an unchanged model:
      after addPreferences   KG and q-EI are the compositions of their own pieces (1e-12 of scale), their means and variances the
                             posterior's (1e-6 / 1e-9); the constrained sweep is the composition of the library's own per-model sweeps
                             (rtol 1e-12, atol 1e-15), its arg-max the first maximiser of its values
      after addObservationPoint   the classes refuse (ValueError: covariances from one factor, means from another) -- objects made before
                             the call and new ones; the handle itself is untouched: the raw entries return the bits they returned before
                             and are again the compositions of their pieces, the variance that of ibo_posterior_batch on the handle;
                             the constrained sweep, which reads the handle as sweep() does, returns its earlier bits as well
      after more preferences (new points: the model is refactored, the augmented factor dropped) the objects made at the start work
                             again, follow the model, and every check of the first stage holds on the new model."""
    import kg_reference as kr
    import qei_reference as qr
    from ibo_amd import DeviceArray, _lib
    from ibo_amd.acquisition import KnowledgeGradient, ParallelEI, sweep
    from ibo_amd.acquisition.constrained import Constraint, sweepConstrained
    from ibo_amd.gaussianprocess import PrefGaussianProcess
    from conftest import synth
    from test_gpu_constrained import compose, own_close, pair
    from test_gpu_knowledge_gradient import kg_call
    from test_gpu_qei import compose_close, qei_call
    rs = np.random.RandomState(3)
    D = 4
    pts = rs.rand(60, D)
    f = lambda x: -np.sum((x - .4) ** 2)
    prefs = [(pts[2 * i], pts[2 * i + 1], 0) if f(pts[2 * i]) > f(pts[2 * i + 1]) else (pts[2 * i + 1], pts[2 * i], 0) for i in range(30)]
    GP = PrefGaussianProcess(our_kernel("ard", [.6] * D))
    GP.addPreferences(prefs[:20])
    Xc, _ = synth(62, 30, D)
    GPc, _ = pair("m5", [.6, .9], Xc, Xc[:, 0] + Xc[:, 1])
    A, Q, P = rs.rand(16, D), rs.rand(30, D), qr.pending_points(pts, 3)
    C = rs.rand(1000, D)
    dc = DeviceArray.from_host(C)
    Z = qr.samples(64, 4)
    con = [Constraint(GPc, upper=.9)]
    kg, qei = KnowledgeGradient(GP, A), ParallelEI(GP, P, Z=Z)

    def own_posterior(X):
        X = _lib.f64(X)
        mu, s2 = np.empty(len(X)), np.empty(len(X))
        _lib.check(_lib.lib.ibo_posterior_batch(GP._handle(), len(X), _lib.dp(X), 1e-7, _lib.dp(mu), _lib.dp(s2)))
        return mu, s2

    def raw(what):
        """the three entries on the handle as it is, each against the composition of the library's own pieces"""
        h = GP._handle()
        g = kg_call(_lib, h, A, Q, 1)
        k, scale = kr.compose(g["mu_ref"], g["mu"], g["s2"], g["b"], GP.noise, True)
        assert np.all(np.abs(g["kg"] - k) <= 1e-12 * scale) and np.max(g["kg"]) > 0, what
        np.testing.assert_allclose(g["mu_ref"], own_posterior(A)[0], rtol=1e-6, atol=1e-9, err_msg=what)
        np.testing.assert_allclose(g["s2"], own_posterior(Q)[1], rtol=1e-6, err_msg=what)
        q = qei_call(_lib, h, P, Z, Q, xi=0.0)
        maxy = ctypes.c_double()
        _lib.check(_lib.lib.ibo_gp_info(h, None, None, None, ctypes.byref(maxy)))
        compose_close(q, Z, maxy.value, what + " q-EI")
        assert np.max(q["qei"]) > 0
        np.testing.assert_allclose(q["mu_pend"], own_posterior(P)[0], rtol=1e-6, atol=1e-9, err_msg=what)
        np.testing.assert_allclose(q["s2"], own_posterior(Q)[1], rtol=1e-6, err_msg=what)
        r = sweepConstrained(GP, con, dc, acq='ei', xi=.01, ymax=maxy.value, outputs=("acq", "pof", "val"))
        pm = [sweep(GP, dc, acq='ei', xi=.01, ymax=maxy.value, outputs=("mu", "s2", "acq")), sweep(GPc, dc, outputs=("mu", "s2"))]
        val, pof = compose(pm, [(1, .9, 1)])
        assert np.array_equal(r["acq"], pm[0]["acq"]), what
        own_close(r["val"], val); own_close(r["pof"], pof)
        assert r["best_idx"] == int(np.argmax(r["val"])) and r["best_val"] == np.max(r["val"]) and np.ptp(pof) > .3 and r["best_val"] > 0, what
        return dict(kg=g["kg"], b=g["b"], qei=q["qei"], c=q["c"], val=r["val"], pof=r["pof"])

    def classes(what):
        """the Python objects made at the start return the raw entries' bits, and the posterior is the model's own"""
        h = GP._handle()
        assert np.array_equal(kg.values(Q), kg_call(_lib, h, A, Q, 1, slopes=False)["kg"]), what
        assert np.array_equal(qei.values(Q), qei_call(_lib, h, P, Z, Q, xi=0.0, pieces=False)["qei"]), what
        np.testing.assert_allclose(kg.slopes(Q)[0], GP.posteriors(A)[0], rtol=1e-6, atol=1e-9, err_msg=what)
        np.testing.assert_allclose(qei.pieces(Q)[3], GP.posteriors(Q)[1], rtol=1e-6, err_msg=what)

    first = raw("after addPreferences")
    classes("after addPreferences")
    GP.addObservationPoint(rs.rand(D))
    for call in (lambda: kg.values(Q), lambda: qei.values(Q), lambda: KnowledgeGradient(GP, A), lambda: ParallelEI(GP, P, Z=Z)):
        with pytest.raises(ValueError):
            call()
    second = raw("after addObservationPoint")
    for k in first:
        assert np.array_equal(first[k], second[k]), k
    assert not np.allclose(GP.posteriors(Q)[1], own_posterior(Q)[1], rtol=1e-6)      # the augmented variance IS in force for the posterior
    n0 = len(GP.X)
    GP.addPreferences(prefs[20:])
    assert len(GP.X) == n0 + 20 and GP._augdev is None
    third = raw("after more preferences")
    classes("after more preferences")
    for k in first:                                  # (the constraint model was left alone: its factor of the product has not moved)
        assert np.array_equal(first[k], third[k]) == (k == "pof"), k

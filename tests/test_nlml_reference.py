"""
The NumPy restatement of the marginal likelihood and its gradient (tests/nlml_reference.py, the yardstick of tests/test_gpu_nlml.py)
against the oracle, against itself in long double, against mpmath at 50 digits, and against central differences of its own value.
CPU only.

Bounds: 1e-12 of V / G_h against the oracle (two float64 routes at cond_2 <= 1e6; measured <= 7e-15 and <= 4e-14); one tenth of a case's
bar between float64 and long double (the yardstick's room; measured <= 0.02); 1e-3 of the bar between long double and mpmath (long double's
2^-64 C against the bar's 1e-15 C); 1e-8 G_h against central differences with step 1e-5 in log theta (truncation ~ step^2 = 1e-10).
Every test prints a RATIO line: the worst error over its bound.
"""
import numpy as np
import pytest

import nlml_reference as nr
from conftest import synth
from oracle import oracle as orc

WELL_TABLE = [("a-" + nr.case_id(c), nr.family_case, c) for c in nr.FAMILY_CASES] + \
             [("a-coincident-" + k, nr.coincident_case, k) for k in nr.COINCIDENT_KINDS] + \
             [("d-" + nr.case_id(nr.SPEC_CASE[:1] + nr.SPEC_CASE[2:]), nr.table_case, nr.SPEC_CASE)]
ILL_TABLE = [("b-" + nr.case_id(c[:1] + c[2:]) + "-l%g" % c[1][0], nr.table_case, c) for c in nr.ILL_CASES]
ROUTE_TABLE = [("c-" + nr.case_id(c[:1] + c[2:]), nr.table_case, c) for c in nr.ROUTE_CASES]
ids = lambda t: t[0]


def test_the_tables_hold_what_the_gpu_file_needs():
    ns = {}
    for kind, N, D in nr.FAMILY_CASES:
        ns.setdefault(N, set()).add(kind)
    assert set(ns) >= {1, 2, 15, 16, 17, 63, 64, 65, 127, 128, 129, 200} and all(len(k) >= 2 for N, k in ns.items() if N != 70)
    assert all(ns[N] == set(nr.KINDS) for N in (63, 64, 65))
    assert {D for _, _, D in nr.FAMILY_CASES} >= {1, 3, 17, 33, 34, 64}
    assert len(set(t[0] for t in WELL_TABLE + ILL_TABLE + ROUTE_TABLE)) == len(WELL_TABLE + ILL_TABLE + ROUTE_TABLE)


@pytest.mark.parametrize("entry", WELL_TABLE + ROUTE_TABLE, ids=ids)
def test_float64_restatement_against_the_oracle(entry):
    key, load, c = entry
    case = load(c)
    kind, hyper, X, Y, noise = case
    r = nr.reference(key, case, longdouble=False)
    nr.assert_tier(r["cond"], nr.WELL, key)
    kern = orc.Kern(kind, hyper)
    ov, og = orc.marginal_likelihood(kern, X, Y, len(hyper), True, noise)
    oc = orc.nlml_c(kern, X, Y, noise)
    rv = max(abs(r["value"] - ov), abs(r["value"] - oc)) / (1e-12 * r["V"])
    rg = np.max(nr.over(np.abs(r["grad"] - og), 1e-12 * r["G"]))
    print("RATIO oracle %s: cond %.3g  value %.3g  gradient %.3g (of 1e-12 V, 1e-12 G_h)" % (key, r["cond"], rv, rg))
    assert rv <= 1 and rg <= 1


@pytest.mark.parametrize("entry", WELL_TABLE + ILL_TABLE, ids=ids)
def test_float64_is_within_a_tenth_of_the_bar_of_long_double(entry):
    key, load, c = entry
    case = load(c)
    r64 = nr.reference(key, case, longdouble=False)
    rld = nr.reference(key, case, longdouble=True)
    nr.assert_tier(rld["cond"], nr.ILL if entry in ILL_TABLE else nr.WELL, key)
    rv, rg = nr.ratios(r64["value"], r64["grad"], rld)
    print("RATIO float64 / long double %s: cond %.3g  Newton move %.3g  value %.3g  gradient %.3g (of the bar)"
          % (key, rld["cond"], rld["move"], rv, rg.max()))
    assert rv <= 0.1 and np.all(rg <= 0.1)


def test_tier_membership():
    for key, load, c in WELL_TABLE + ROUTE_TABLE:
        kind, hyper, X, Y, noise = load(c)
        if len(X) > 400 and key != ROUTE_TABLE[0][0]:
            continue                                  # (1729 rows: the 1728-row matrix with one more point; asserted on the GPU, where it is computed anyway)
        nr.assert_tier(nr.lr.cond2(orc.Kern(kind, hyper).cov_matrix(X) + noise * np.eye(len(X))), nr.WELL, key)
    conds = []
    for key, load, c in ILL_TABLE:
        kind, hyper, X, Y, noise = load(c)
        conds.append(nr.lr.cond2(orc.Kern(kind, hyper).cov_matrix(X) + noise * np.eye(len(X))))
        nr.assert_tier(conds[-1], nr.ILL, key)
    print("ill-conditioned tier:", " ".join("%.3g" % c for c in conds))
    assert {c[0] for c in nr.ILL_CASES} == {"ard", "m3", "m5"}
    # the same model at noise 1e-4 belongs to neither tier, and the m5 model at 1e-9 is beyond the second
    kind, hyper, X, Y, _ = nr.table_case(nr.ILL_CASES[0])
    c = nr.lr.cond2(orc.Kern(kind, hyper).cov_matrix(X) + 1e-4 * np.eye(len(X)))
    assert 1e6 < c < 1e7
    c = nr.lr.cond2(orc.Kern("m5", [3., 1.2]).cov_matrix(X) + 1e-9 * np.eye(len(X)))
    assert c > 2e10


# ---------------------------------------------------------------------------------------------------------------- mpmath
def _mp_truth(kern, X, Y, noise, nh):
    import mpmath as mp
    mp.mp.dps = 50
    N = len(X)
    A = mp.matrix((kern.cov_matrix(X) + noise * np.eye(N)).tolist())
    B = A ** -1
    y = mp.matrix([mp.mpf(float(v)) for v in Y])
    al = B * y
    L = mp.cholesky(A)
    value = (y.T * al)[0] / 2 + sum(mp.log(L[i, i]) for i in range(N)) + mp.mpf(N) / 2 * mp.log(2 * mp.pi)
    grad = []
    for h in range(nh):
        dK = mp.matrix(kern.derivative(X, h).tolist())
        t1 = sum(B[a, b] * dK[a, b] for a in range(N) for b in range(N)) / 2
        t2 = (al.T * dK * al)[0] / 2
        grad.append(t1 - t2)
    return value, grad


@pytest.mark.parametrize("kind,hyper,noise,tier", [("svard", [.5, .7, .9], 1e-2, (0, 1e6)), ("ard", [.5, .7], 1e-8, (1e8, 1e10)),
                                                   ("m5", [3., 1.2], 1e-7, (1e8, 1e10))])
def test_long_double_against_mpmath(kind, hyper, noise, tier):
    mp = pytest.importorskip("mpmath")
    X, Y = synth(50, 48, 2)
    kern = orc.Kern(kind, hyper)
    r = nr.nlml(kern, X, Y, noise, len(hyper), longdouble=True)
    assert tier[0] <= r["cond"] <= tier[1], r["cond"]
    value, grad = _mp_truth(kern, X, Y, noise, len(hyper))
    f = mp.mpf(nr.bar_factor(r["cond"]))
    ld = lambda x: mp.mpf(float(x)) + mp.mpf(float(x - np.longdouble(float(x))))          # a long double, exactly
    rv = float(abs(ld(r["value"]) - value) / (f * ld(r["V"])))
    rg = [float(abs(ld(r["grad"][h]) - grad[h]) / (f * ld(r["G"][h]))) for h in range(len(hyper))]
    print("RATIO long double / mpmath %s noise %g: cond %.3g  value %.3g  gradient %.3g (of the bar)" % (kind, noise, r["cond"], rv, max(rg)))
    assert rv <= 1e-3 and max(rg) <= 1e-3


# ---------------------------------------------------------------------------------------------------------------- the value's own derivative
DIFF_KERNELS = [("ard", [.3, .5, .4]), ("iso", [.4]), ("svard", [.3, .5, .4, .9]), ("sviso", [.4, .8]), ("m5", [.5, .9]),
                ("m3", [.5, .95]), ("m3", [np.sqrt(3.0), .95])]


@pytest.mark.parametrize("kind,hyper", DIFF_KERNELS, ids=lambda v: v if isinstance(v, str) else "l%.3g" % v[0])
def test_gradient_is_the_derivative_of_the_value(kind, hyper):
    """central differences, in long double, of the restated value in log theta.  The Matern-3/2 length scale is the reference's quirk
    (the unscaled distance): its component is the derivative only at theta = sqrt(3), where the two distances coincide, and is NOT
    at theta = .5 -- which is asserted, so that a restatement that quietly repaired the quirk would be noticed."""
    X, Y = synth(5, 40, 3)
    hyper = np.array(hyper, dtype=float)
    nh = len(hyper)
    r = nr.nlml(orc.Kern(kind, hyper), X, Y, nr.NOISE, nh, longdouble=True)
    step = np.longdouble(1e-5)
    worst = 0.0
    for h in range(nh):
        e = np.zeros(nh); e[h] = float(step)
        vp = nr.nlml(orc.Kern(kind, hyper * np.exp(e)), X, Y, nr.NOISE, 0, longdouble=True)["value"]
        vm = nr.nlml(orc.Kern(kind, hyper * np.exp(-e)), X, Y, nr.NOISE, 0, longdouble=True)["value"]
        cd = (vp - vm) / (2 * step)
        ratio = float(abs(r["grad"][h] - cd) / (1e-8 * r["G"][h]))
        print(kind, h, "grad %.15g central difference %.15g G_h %.6g ratio %.3g" % (r["grad"][h], cd, r["G"][h], ratio))
        if kind == "m3" and h == 0 and hyper[0] != np.sqrt(3.0):
            assert ratio > 1e3                       # the quirk, kept
            continue
        worst = max(worst, ratio)
    print("RATIO central difference %s: %.3g (of 1e-8 G_h)" % (kind, worst))
    assert worst <= 1


# ---------------------------------------------------------------------------------------------------------------- derivative specs
@pytest.mark.parametrize("kind", nr.KINDS)
def test_spec_helper_is_the_oracle_derivative_on_the_canonical_list(kind):
    X, Y = synth(9, 30, 4)
    hyper = nr.hyper_of(kind, 4)
    kern = orc.Kern(kind, hyper)
    for h, (mode, dim) in enumerate(nr.canonical_spec(kind, 4)):
        want = kern.derivative(X, h)
        got = nr.spec_derivative(kern, X, mode, dim)
        assert np.max(np.abs(got - want)) <= 1e-15 * np.max(np.abs(want)), (kind, h)       # (z summed in another order: a few ulps)
    with pytest.raises(ValueError):
        nr.spec_derivative(kern, X, 5, 0)
    with pytest.raises(ValueError):
        nr.spec_derivative(kern, X, 0, 4)


def test_mode_identities_on_se_ard():
    kind, hyper, X, Y, noise = nr.table_case(nr.SPEC_CASE)
    kern = orc.Kern(kind, hyper)
    D, N = X.shape[1], len(X)
    r = nr.nlml(kern, X, Y, noise, longdouble=True, spec=[(0, d) for d in range(D)] + [(1, 0), (2, 0)])
    g, G = r["grad"], r["G"]
    # the length scales' components add up to the iso component (z = sum_d w_d u_d^2)
    assert abs(g[:D].sum() - g[D]) <= 1e-15 * (G[:D].sum() + G[D])
    # dK = 2 K = 2 (A - noise I):  sum (B - alpha alpha^T) o (A - noise I) = N - noise tr B - y.alpha + noise alpha.alpha
    B, al = r["B"], r["alpha"]
    y = np.asarray(Y).astype(np.longdouble)
    want = N - noise * np.trace(B) - y @ al + noise * (al @ al)
    print("mode 2: %.15g  identity %.15g" % (g[D + 1], want))
    assert abs(g[D + 1] - want) <= 1e-15 * (N + noise * np.trace(B) + abs(y @ al) + noise * (al @ al))
    assert nr.SPEC_LISTS[0] == nr.canonical_spec(kind, D) and len(nr.SPEC_LISTS) == 2 + (D + 1) + 2


def test_n_equals_one_closed_forms():
    for c in [c for c in nr.FAMILY_CASES if c[1] == 1]:
        kind, hyper, X, Y, noise = nr.family_case(c)
        r = nr.reference("a-" + nr.case_id(c), (kind, hyper, X, Y, noise), longdouble=True)
        value, grad, G = nr.closed_form_n1(kind, hyper, Y, noise)
        assert abs(r["value"] - value) <= 1e-15 * r["V"]            # (the oracle's K is a float64)
        assert np.all(np.abs(r["grad"] - grad) <= 1e-15 * G) and np.all(np.abs(r["G"] - G) <= 1e-15 * G)

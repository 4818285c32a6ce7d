"""
Hyper-parameter learning against exact truth: ibo_nlml_grad, ibo_nlml_grid and trainhyper.marginalLikelihood / nlml / dnlml / nlml_values
(csrc/abi_nlml.hip, nlml_grad_fast_kernel / nlml_grad_kernel / grad_reduce_kernel and launch_cov_matrix_batched in csrc/assemble.hip).

The yardstick is tests/nlml_reference.py, pinned by tests/test_nlml_reference.py: in long double for every case up to 400 rows and every
ill-conditioned one, in float64 beyond 400 rows at cond_2 <= 1e6.  Bars, with C the reference's cond_2:
    value      |v - value|    <= 1e-15 max(C, 1e6) V        V   = |y.alpha / 2| + sum |log L_ii| + N log(2 pi) / 2
    gradient   |g_h - grad_h| <= 1e-15 max(C, 1e6) G_h      G_h = |T1_h| + |T2_h|, every component against its own
Every case asserts its tier from the reference first (C <= 1e6, or 1e7 <= C <= 2e10): a bar is never met by an input outside its tier.
Every test prints "RATIO <group> ..." lines: the worst error over its bar.  Groups: a families and sizes, b the ill-conditioned tier,
c the routes to K^-1, d raw derivative specs, e the theta grid, f the kept workspaces, g the learning loop.
"""
import ctypes

import numpy as np
import pytest

import loo_reference as lr
import nlml_reference as nr
from conftest import synth
from oracle import oracle as orc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    from ibo_amd import _lib
    if _lib.device_count() < 1:
        pytest.fail("no GPU visible: the product has no CPU fallback")
    return _lib


def make_kernel(kind, hyper):
    from ibo_amd.gaussianprocess import kernel as K
    return {"ard": K.GaussianKernel_ard, "iso": K.GaussianKernel_iso, "svard": K.SVGaussianKernel_ard,
            "sviso": K.SVGaussianKernel_iso, "m3": K.MaternKernel3, "m5": K.MaternKernel5}[kind](np.array(hyper, dtype=float))


def check(group, what, v, g, ref, tier=nr.WELL):
    """a device value (and gradient, or None) against a reference of the stated tier; prints the RATIO line"""
    nr.assert_tier(ref["cond"], tier, what)
    rv, rg = nr.ratios(v, g, ref)
    worst = float(rg.max()) if len(rg) else 0.0
    print("RATIO %s %s: cond %.3g  value %.3g  gradient %.3g%s" % (group, what, ref["cond"], rv, worst,
                                                                   "" if not len(rg) else "  (component %d of %d)" % (int(rg.argmax()), len(rg))))
    assert rv <= 1.0, (what, v, ref["value"], ref["V"])
    assert np.all(rg <= 1.0), (what, g, ref["grad"], ref["G"])
    return max(rv, worst)


def run_ml(case, nh=None):
    from ibo_amd.gaussianprocess.trainhyper import marginalLikelihood
    kind, hyper, X, Y, noise = case
    return marginalLikelihood(make_kernel(kind, hyper), X, Y, len(hyper) if nh is None else nh, True, noise=noise)


# ---------------------------------------------------------------------------------------------------------------- a. families and sizes
@pytest.mark.parametrize("c", nr.FAMILY_CASES, ids=nr.case_id)
def test_a_every_family_at_every_tile_layout(lib, c):
    """a partly filled diagonal tile, one point in the second tile row, one point in all; D = 33: the LD = 65 instantiation; 34 and 65
    derivatives: the general kernel in two and four passes.  marginalLikelihood's value-only call (the grid) meets the value bar too."""
    from ibo_amd.gaussianprocess.trainhyper import marginalLikelihood
    case = nr.family_case(c)
    kind, hyper, X, Y, noise = case
    ref = nr.reference("a-" + nr.case_id(c), case, longdouble=True)
    v, g = run_ml(case)
    check("a", nr.case_id(c), v, g, ref)
    v0 = marginalLikelihood(make_kernel(kind, hyper), X, Y, len(hyper), False, noise=noise)
    check("a", nr.case_id(c) + " value only", v0, None, ref)
    if len(X) == 1:
        # one observation: every length scale's derivative is exactly 0; the value and the signal variance's derivative against their closed
        # forms at 1e-15 of |value| and of G_h (the derivative is a difference of two terms: 2^-53 of each is all float64 can promise)
        cv, cg, cG = nr.closed_form_n1(kind, hyper, Y, noise)
        nl = len(hyper) - (kind in ("svard", "sviso", "m3", "m5"))
        assert np.all(np.asarray(g)[:nl] == 0.0), g
        eg = nr.over(np.abs(np.asarray(g) - cg), 1e-15 * cG).max()
        print("RATIO a %s closed form: value %.3g, value only %.3g (of 1e-15 |value|)  gradient %.3g (of 1e-15 G_h)"
              % (nr.case_id(c), abs(v - cv) / (1e-15 * abs(cv)), abs(v0 - cv) / (1e-15 * abs(cv)), eg))
        assert abs(v - cv) <= 1e-15 * abs(cv) and abs(v0 - cv) <= 1e-15 * abs(cv), (v, v0, cv)
        assert eg <= 1.0, (g, cg)
    v2, g2 = run_ml(case)
    assert v2 == v and np.array_equal(g, g2)


@pytest.mark.parametrize("kind", nr.COINCIDENT_KINDS)
def test_a_three_coincident_rows(lib, kind):
    """row 0 again as rows 7 and 70 of 129: z = 0 off the diagonal, in the diagonal tile and in the one below it"""
    case = nr.coincident_case(kind)
    ref = nr.reference("a-coincident-" + kind, case, longdouble=True)
    v, g = run_ml(case)
    check("a", "coincident rows " + kind, v, g, ref)
    v2, g2 = run_ml(case)
    assert v2 == v and np.array_equal(g, g2)


# ---------------------------------------------------------------------------------------------------------------- b. the ill-conditioned tier
@pytest.mark.parametrize("c", nr.ILL_CASES, ids=lambda c: nr.case_id(c[:1] + c[2:]) + "-l%g" % c[1][0])
def test_b_ill_conditioned_tier(lib, c):
    case = nr.table_case(c)
    what = nr.case_id(c[:1] + c[2:]) + "-l%g" % c[1][0]
    ref = nr.reference("b-" + what, case, longdouble=True)
    v, g = run_ml(case)
    check("b", what, v, g, ref, nr.ILL)
    v2, g2 = run_ml(case)
    assert v2 == v and np.array_equal(g, g2)


# ---------------------------------------------------------------------------------------------------------------- c. routes of K^-1
@pytest.mark.parametrize("c", nr.ROUTE_CASES, ids=lambda c: nr.case_id(c[:1] + c[2:]))
def test_c_both_products_that_form_the_inverse(lib, c):
    """1728 rows: wtw_kernel's last size; 1729: the first on the packed-operand product -- every component at its own bar"""
    case = nr.table_case(c)
    ref = nr.reference("c-" + nr.case_id(c[:1] + c[2:]), case, longdouble=False)
    v, g = run_ml(case)
    check("c", nr.case_id(c[:1] + c[2:]), v, g, ref)


# ---------------------------------------------------------------------------------------------------------------- d. raw derivative specs
def raw_grad(lib, kind, hyper, X, Y, noise, spec, ngrad=None, null_modes=False):
    """ibo_nlml_grad with a (mode, dim) list of its own: (return code, value, gradient)"""
    ktype, th, sf2, _ = make_kernel(kind, hyper)._ibo_spec()
    Xa = lib.rows(X); Ya = lib.f64(Y)
    N, D = Xa.shape
    n = len(spec)
    modes = (ctypes.c_int * max(n, 1))(*[m for m, _ in spec])
    dims = (ctypes.c_int * max(n, 1))(*[d for _, d in spec])
    v = ctypes.c_double(np.nan)
    g = np.full(max(n, 1), np.nan)
    rc = lib.lib.ibo_nlml_grad(lib.default_device(), ktype, N, D, lib.dp(Xa), lib.dp(Ya), lib.dp(th), len(th), sf2, float(noise),
                               n if ngrad is None else ngrad, None if null_modes else modes, dims, ctypes.byref(v), lib.dp(g))
    return rc, v.value, g[:n]


def test_d_derivative_lists_of_every_shape(lib):
    """the full list, reversed, every single component, a repeat, and mode 1 on the ARD kernel: every component at its own bar against
    nlml_reference.spec_derivative, and with the same bits in whatever list it appears (nlml_grad_fast_kernel keeps a derivative's sum
    apart from the others'; grad_reduce_kernel adds the same tiles in the same order); the value has the same bits in all"""
    case = nr.table_case(nr.SPEC_CASE)
    kind, hyper, X, Y, noise = case
    bits, value, worst = {}, None, 0.0
    for spec in nr.SPEC_LISTS:
        ref = nr.reference("d", case, longdouble=True, spec=spec)
        rc, v, g = raw_grad(lib, kind, hyper, X, Y, noise, spec)
        assert rc == lib.OK, (spec, lib.lib.ibo_last_error())
        worst = max(worst, check("d", "svard %s" % (spec,), v, g, ref))
        value = v if value is None else value
        assert v == value, spec
        for s, gh in zip(spec, g):
            assert bits.setdefault(s, gh) == gh, (s, spec)
    assert set(bits) == set(nr.SPEC_FULL) | {(1, 0)}
    # mode 1 on this ARD kernel is the sum of its five mode-0 components, within the two bars
    full = nr.reference("d", case, longdouble=True, spec=nr.SPEC_FULL)
    iso = nr.reference("d", case, longdouble=True, spec=[(1, 0)])
    f = nr.bar_factor(full["cond"])
    assert abs(sum(bits[(0, d)] for d in range(5)) - bits[(1, 0)]) <= f * float(full["G"][:5].sum() + iso["G"][0])
    print("RATIO d lists on svard: worst %.3g" % worst)


@pytest.mark.parametrize("kind,hyper,spec", nr.SPEC_OTHER, ids=[k for k, _, _ in nr.SPEC_OTHER])
def test_d_modes_on_other_kernels(lib, kind, hyper, spec):
    """modes 3 and 4 on the Matern kernels (out of order, 3 twice), mode 2 on a kernel without a signal variance"""
    _, _, X, Y, noise = nr.table_case(nr.SPEC_CASE)
    case = (kind, hyper, X, Y, noise)
    ref = nr.reference("d-" + kind, case, longdouble=True, spec=spec)
    rc, v, g = raw_grad(lib, kind, hyper, X, Y, noise, spec)
    assert rc == lib.OK
    check("d", "%s %s" % (kind, spec), v, g, ref)
    for i, s in enumerate(spec):
        assert g[i] == g[spec.index(s)]
    if kind != "ard":                                 # the canonical list of the kind through Python: the same value bits
        v2, g2 = run_ml(case)
        assert v2 == v
        for h, s in enumerate(nr.canonical_spec(kind, 5)):
            assert g2[h] == g[spec.index(s)]


def test_d_refusals_leave_the_workspace_usable(lib):
    case = nr.table_case(nr.SPEC_CASE)
    kind, hyper, X, Y, noise = case
    D = X.shape[1]
    good = nr.SPEC_FULL
    rc, v, g = raw_grad(lib, kind, hyper, X, Y, noise, good)
    assert rc == lib.OK
    long_list = [(0, 0)] * 66
    refused = [dict(spec=good, ngrad=0), dict(spec=long_list, ngrad=66), dict(spec=[(-1, 0)] + good[1:]), dict(spec=good[:2] + [(5, 0)]),
               dict(spec=[(0, D)]), dict(spec=good[:3] + [(0, -1)]), dict(spec=good, null_modes=True)]
    for kw in refused:
        rc2, v2, g2 = raw_grad(lib, kind, hyper, X, Y, noise, **kw)
        assert rc2 == lib.ERR_ARG, kw
        assert np.isnan(v2) and np.all(np.isnan(g2)), kw            # nothing was written
        rc3, v3, g3 = raw_grad(lib, kind, hyper, X, Y, noise, good)
        assert rc3 == lib.OK and v3 == v and np.array_equal(g3, g), kw
    check("d", "after the refusals", v3, g3, nr.reference("d", case, longdouble=True, spec=good))


# ---------------------------------------------------------------------------------------------------------------- e. the theta grid
GRID_CASES = [("sviso", 1, 3, 1), ("m5", 1, 2, 9), ("svard", 2, 3, 17), ("m3", 2, 1, 9), ("m3", 63, 3, 9), ("svard", 63, 2, 1),
              ("sviso", 64, 17, 17), ("m5", 64, 3, 9), ("m5", 65, 1, 17), ("svard", 65, 3, 9), ("sviso", 127, 3, 9), ("m3", 127, 17, 1),
              ("svard", 128, 3, 17), ("m5", 128, 33, 1), ("m3", 300, 3, 1), ("sviso", 300, 2, 1)]


def grid_rows(kind, D, n):
    """n hyper-parameter rows around nlml_reference.hyper_of: length scales times 0.8 .. 1.5, a signal magnitude of its own per row"""
    rs = np.random.RandomState(100 * n + D)
    base = np.array(nr.hyper_of(kind, D))
    rows = np.tile(base, (n, 1))
    nl = len(base) - (kind in ("svard", "sviso", "m3", "m5"))
    rows[:, :nl] *= np.exp(rs.uniform(np.log(.8), np.log(1.5), size=(n, nl)))
    if nl < len(base):
        rows[:, -1] = np.linspace(.7, 1.3, n) if n > 1 else [.85]
    return rows


def option(lib, name, value):
    lib.check(lib.lib.ibo_set_option(name, value))


def grid_both_forms(lib, call):
    """call() at the default (the dot form where its guard admits it) and with dot_form = 0"""
    v = np.asarray(call())
    try:
        option(lib, b"dot_form", 0)
        d = np.asarray(call())
    finally:
        option(lib, b"dot_form", -1)
    return v, d


def check_grid(lib, group, what, kind, rows, X, Y, noise, values, with_grad=True):
    """every theta-point of a grid against its own truth, and against ibo_nlml_grad's value at that theta within the sum of the two bars"""
    worst = 0.0
    for t, row in enumerate(rows):
        case = (kind, list(row), X, Y, noise)
        ref = nr.reference("%s-%s-%d" % (group, what, t), case, longdouble=len(X) <= 400, nhyper=0)
        nr.assert_tier(ref["cond"], nr.WELL, what)
        gv = run_ml(case, 1)[0] if with_grad else None
        for vals in values:
            rv, _ = nr.ratios(vals[t], None, ref)
            worst = max(worst, rv)
            assert rv <= 1.0, (what, t, vals[t], ref["value"])
            if with_grad:
                assert abs(gv - ref["value"]) <= nr.bar_factor(ref["cond"]) * ref["V"]
                assert abs(gv - vals[t]) <= 2 * nr.bar_factor(ref["cond"]) * ref["V"]
    print("RATIO %s %s: worst value / bar %.3g over %d theta-points" % (group, what, worst, len(rows)))
    return worst


@pytest.mark.parametrize("kind,N,D,n", GRID_CASES, ids=lambda v: str(v))
def test_e_grid_of_every_family_with_its_own_signal_variances(lib, kind, N, D, n):
    """launch_cov_matrix_batched's Matern and signal-variance forms and the sf2s argument at real sizes; N + 1 = 64 and 128 (the appended y
    row fills the last block), N = 64 and 128 (it sits alone in a block column that is dropped), N = 1"""
    from ibo_amd.gaussianprocess.trainhyper import nlml_values
    X, Y = synth(N + D, N, D)
    rows = grid_rows(kind, D, n)
    v, d = grid_both_forms(lib, lambda: nlml_values([make_kernel(kind, r) for r in rows], X, Y, nr.NOISE))
    assert np.all(np.isfinite(v)) and np.all(np.isfinite(d))
    if kind in ("sviso", "svard") and N >= 63 and n > 1:
        assert not np.array_equal(v, d)                # the dot form did run
    check_grid(lib, "e", "%s N=%d D=%d n=%d" % (kind, N, D, n), kind, rows, X, Y, nr.NOISE, [v, d])
    v2 = nlml_values([make_kernel(kind, r) for r in rows], X, Y, nr.NOISE)
    assert np.array_equal(v, v2)


def raw_grid(lib, X, Y, rows, noise):
    """ibo_nlml_grid for SE-ARD without the sf2s argument"""
    Xa = lib.rows(X); Ya = lib.f64(Y); th = lib.f64(rows)
    out = np.full(len(th), np.inf)
    lib.check(lib.lib.ibo_nlml_grid(lib.default_device(), lib.K_SE_ARD, Xa.shape[0], Xa.shape[1], lib.dp(Xa), lib.dp(Ya), len(th), lib.dp(th),
                                    th.shape[1], None, float(noise), lib.dp(out)))
    return out


ARD_GRID = dict(N=300, D=3, n=9)


def ard_grid():
    X, Y = synth(303, ARD_GRID["N"], ARD_GRID["D"])
    return X, Y, grid_rows("ard", ARD_GRID["D"], ARD_GRID["n"])


def test_e_raw_grid_without_signal_variances(lib):
    X, Y, rows = ard_grid()
    v, d = grid_both_forms(lib, lambda: raw_grid(lib, X, Y, rows, nr.NOISE))
    assert not np.array_equal(v, d)                    # the dot form did run
    check_grid(lib, "e", "ard raw N=300 n=9", "ard", rows, X, Y, nr.NOISE, [v, d])
    one = raw_grid(lib, X[:1], Y[:1], rows, nr.NOISE)  # one observation, nine theta-points: the same closed form nine times
    cv = nr.closed_form_n1("ard", list(rows[0]), Y[:1], nr.NOISE)[0]
    assert np.all(np.abs(one - float(cv)) <= 1e-15 * abs(float(cv)))


def test_e_one_theta_point_beyond_the_dot_forms_guard(lib):
    """sum_d w_d max_k x_kd^2 > 1e5 for theta-point 4 alone (a length scale of 0.003 on the unit cube): the whole call takes the
    difference form, bit for bit, and the nine values still meet their bars; without that point the dot form runs"""
    N, D = 128, 2
    X, Y = synth(N + D, N, D)
    rows = grid_rows("ard", D, 9)
    rows[4, 0] = .003
    assert (X[:, 0] ** 2).max() / rows[4, 0] ** 2 > 1e5 and all((X ** 2).max(0) @ (1 / r ** 2) < 1e5 for r in np.delete(rows, 4, 0))
    v, d = grid_both_forms(lib, lambda: raw_grid(lib, X, Y, rows, nr.NOISE))
    assert np.array_equal(v, d)
    check_grid(lib, "e", "ard beyond the guard", "ard", rows, X, Y, nr.NOISE, [v])
    keep = np.delete(rows, 4, 0)
    v8, d8 = grid_both_forms(lib, lambda: raw_grid(lib, X, Y, keep, nr.NOISE))
    assert not np.array_equal(v8, d8) and np.array_equal(d8, np.delete(d, 4))


def test_e_left_looking_panel_with_rows_below_and_the_tail(lib):
    """m5, 1600 rows, nine theta-points: float64 truth at cond_2 <= 1e6"""
    from ibo_amd.gaussianprocess.trainhyper import nlml_values
    N, D, n = 1600, 4, 9
    X, Y = synth(N + D, N, D)
    rows = grid_rows("m5", D, n)
    v = np.asarray(nlml_values([make_kernel("m5", r) for r in rows], X, Y, nr.NOISE))
    check_grid(lib, "e", "m5 N=1600 n=9", "m5", rows, X, Y, nr.NOISE, [v], with_grad=False)
    gv = run_ml(("m5", list(rows[3]), X, Y, nr.NOISE))[0]
    ref = nr.reference("e-m5 N=1600 n=9-3", ("m5", list(rows[3]), X, Y, nr.NOISE), longdouble=False, nhyper=0)
    assert abs(gv - v[3]) <= 2 * nr.bar_factor(ref["cond"]) * ref["V"]


# ---------------------------------------------------------------------------------------------------------------- f. the kept workspaces
def test_f_gradient_workspace_with_fewer_rows_of_the_same_arrays(lib):
    """300 rows, then the first 290 of the same arrays (the same Npad, the same leading targets: the device keeps Y with ten stale
    values behind row 290, which gemv_lower2_kernel's kend clamp leaves unread), 300 again, the last ten targets set to 0, 290 again:
    every step against its own truth"""
    theta, D = [.4, .5, .6], 3
    X, Y = synth(303, 300, D)
    Y0 = Y.copy(); Y0[290:] = 0.0
    steps = [("300", X, Y), ("290", X[:290], Y[:290]), ("300", X, Y), ("300 zeros", X, Y0), ("290", X[:290], Y0[:290])]
    lib.trim()
    got = {}
    for i, (key, x, y) in enumerate(steps):
        case = ("ard", theta, x, y, nr.NOISE)
        ref = nr.reference("f-" + key, case, longdouble=True)
        v, g = run_ml(case)
        check("f", "step %d: %s rows" % (i, key), v, g, ref)
        if key in got:
            assert got[key][0] == v and np.array_equal(got[key][1], g), (i, key)
        got[key] = (v, g)


def test_f_a_good_call_after_a_failed_one(lib):
    from numpy.linalg import LinAlgError
    from ibo_amd.gaussianprocess.trainhyper import looLikelihood
    case = nr.table_case(nr.SPEC_CASE)
    kind, hyper, X, Y, noise = case
    ref = nr.reference("d-" + nr.case_id(nr.SPEC_CASE[:1] + nr.SPEC_CASE[2:]), case, longdouble=True)
    v, g = run_ml(case)
    check("f", "before the failure", v, g, ref)
    Xd = np.r_[X, X[:8]]; Yd = np.r_[Y, Y[:8]]             # coincident pairs and no noise: pivots that are rounding noise
    with pytest.raises(LinAlgError):
        run_ml((kind, hyper, Xd, Yd, 0.0))
    v2, g2 = run_ml(case)
    assert v2 == v and np.array_equal(g2, g)
    with pytest.raises(LinAlgError):
        run_ml((kind, hyper, Xd, Yd, 0.0))
    k = make_kernel(kind, hyper)
    lv, lg, (mu, s2) = looLikelihood(k, X, Y, len(hyper), True, noise=noise, predictions=True)
    lref = lr.objective(orc.Kern(kind, hyper), X, Y, noise, len(hyper))
    assert lref["cond"] <= 1e6
    assert abs(lv - lref["value"]) <= 1e-9 * (len(X) + abs(lref["value"]))
    assert np.all(np.abs(np.asarray(lg) - lref["grad"]) <= 1e-9 * lref["S"])
    assert np.all(np.abs(mu - lref["mu"]) <= 1e-9 * (np.abs(Y) + np.abs(lref["c"]) / lref["d"])) and np.all(np.abs(s2 - lref["s2"]) <= 1e-9 * lref["s2"])
    v3, g3 = run_ml(case)
    assert v3 == v and np.array_equal(g3, g)


def test_f_grid_workspace_after_a_failed_matrix(lib):
    """nine good theta-points at 300 rows; the same geometry with point 4 numerically singular (the identity pad is reused, not
    rewritten): NaN there, the other eight at their earlier bits; the nine good ones again; ibo_trim and once more"""
    N, D, noise = 300, 3, 1e-14
    X, Y = synth(N + D, N, D)
    rows = np.exp(np.random.RandomState(77).uniform(np.log(.02), np.log(.04), size=(9, D)))     # nearly diagonal matrices: fine with next to no noise
    bad = rows.copy(); bad[4] = 3e3
    lib.trim()
    good = raw_grid(lib, X, Y, rows, noise)
    check_grid(lib, "f", "grid before the failed matrix", "ard", rows, X, Y, noise, [good], with_grad=False)
    out = raw_grid(lib, X, Y, bad, noise)
    keep = np.arange(9) != 4
    assert np.isnan(out[4]) and np.array_equal(out[keep], good[keep])
    assert np.array_equal(raw_grid(lib, X, Y, rows, noise), good)
    lib.trim()
    assert np.array_equal(raw_grid(lib, X, Y, rows, noise), good)


def test_f_grid_gradient_and_loo_interleaved_on_two_data_sets(lib):
    from ibo_amd.gaussianprocess.trainhyper import looLikelihood, nlml_values
    small = nr.table_case(nr.SPEC_CASE)
    X, Y, rows = ard_grid()
    big = ("ard", list(rows[2]), X, Y, nr.NOISE)
    srows = grid_rows("svard", 5, 9)

    def sequence():
        out = []
        for case, grid in ((small, srows), (big, rows), (small, srows)):
            kind, hyper, x, y, noise = case
            out.append(np.asarray(nlml_values([make_kernel(kind, r) for r in grid], x, y, noise)))
            out.append(run_ml(case))
            out.append(looLikelihood(make_kernel(kind, hyper), x, y, len(hyper), True, noise=noise))
            out.append(np.asarray(nlml_values([make_kernel(kind, r) for r in grid], x, y, noise)))
        return out
    first, second = sequence(), sequence()
    for i, (case, grid, tag) in enumerate(((small, srows, "130 rows"), (big, rows, "300 rows"), (small, srows, "130 rows again"))):
        kind, hyper, x, y, noise = case
        g0, (v, g), (lv, lg), g1 = first[4 * i:4 * i + 4]
        assert np.array_equal(g0, g1)
        check_grid(lib, "f", "interleaved grid, " + tag, kind, grid, x, y, noise, [g0], with_grad=False)
        check("f", "interleaved gradient, " + tag, v, g, nr.reference("f-il-%s" % tag[:8], case, longdouble=True))
        lref = lr.objective(orc.Kern(kind, hyper), x, y, noise, len(hyper))
        assert lref["cond"] <= 1e6
        assert abs(lv - lref["value"]) <= 1e-9 * (len(x) + abs(lref["value"])) and np.all(np.abs(np.asarray(lg) - lref["grad"]) <= 1e-9 * lref["S"])
    for a, b in zip(first, second):
        if isinstance(a, tuple):
            assert a[0] == b[0] and np.array_equal(a[1], b[1])
        else:
            assert np.array_equal(a, b)


# ---------------------------------------------------------------------------------------------------------------- g. the learning loop
def test_g_bfgs_ends_where_the_restated_gradient_vanishes(lib):
    """fmin_bfgs on nlml / dnlml (Matern-5/2, 65 rows, D = 2; their noise is marginalLikelihood's default, 1e-3): at the returned point the
    RESTATED gradient has |g_h| <= 1e-5 G_h, and the value is the restatement's within its bar"""
    from scipy.optimize import fmin_bfgs
    from ibo_amd.gaussianprocess import kernel as K
    from ibo_amd.gaussianprocess.trainhyper import nlml, dnlml
    X, Y = synth(67, 65, 2)
    x0 = np.log([.3, .7])
    xs = fmin_bfgs(nlml, x0, dnlml, args=(K.MaternKernel5, X, Y), gtol=1e-7, maxiter=200, disp=False)
    case = ("m5", list(np.exp(xs)), X, Y, 1e-3)
    ref = nr.reference("g", case, longdouble=True)
    v = nlml(xs, K.MaternKernel5, X, Y)
    g = dnlml(xs, K.MaternKernel5, X, Y)
    check("g", "at the optimum theta = %s" % np.exp(xs), v, g, ref)
    rel = (np.abs(ref["grad"]) / ref["G"]).astype(float)
    print("RATIO g |grad_h| / (1e-5 G_h) at the optimum: %s   from %.6g to %.6g" % (rel / 1e-5, nlml(x0, K.MaternKernel5, X, Y), v))
    assert v < nlml(x0, K.MaternKernel5, X, Y)
    assert np.all(rel <= 1e-5)

"""
The gradient-observation model's marginal likelihood on the CPU: tests/gradobs_nlml_reference.py (the formulas of DESIGN 4.31 in NumPy)
against central differences of its own long-double value, float64 against long double at half the project's bar, its exact special cases,
and the Python surface of ibo_ggp_nlml_grad.  No GPU.
"""
import math
import os
import re

import numpy as np
import pytest

import gradobs_reference as gr
import gradobs_nlml_reference as gn
from oracle import oracle as orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LD = np.longdouble


def fd_case(kind, hyper, N, D, twin):
    X = gr.points(N, D, 400 + N + 10 * D)
    if twin is not None:
        X[twin[1]] = X[twin[0]]
    Y, G = gr.objective(X)
    return X, Y, G, np.array(gn.FD_GNOISE[:D], dtype=float)


@pytest.mark.parametrize("case", gn.FD_CASES, ids=[c[0] for c in gn.FD_CASES])
def test_long_double_gradient_against_central_differences(case):
    """Every component -- each hyper-parameter, the noise, each gradient noise -- against the central difference of the long-double value at
    steps h and h / 2 in the log of the parameter.  The bar is the quotient's own error: its truncation, h^2 |f'''| / 8 as the two steps
    show it (|D(h) - D(h / 2)|), plus the rounding of a difference of two long-double values whose factorisation carries cond_2 times the
    long-double unit, 8 eps max(cond_2, 1e6) V / h."""
    kind, hyper, N, D, twin = case
    X, Y, G, gno = fd_case(kind, hyper, N, D, twin)
    hyper = np.array(hyper, dtype=float)
    res = gn.nlml(orc.Kern(kind, hyper), X, Y, G, gn.FD_NOISE, gno, longdouble=True)
    lh, ln, lg = np.log(hyper), math.log(gn.FD_NOISE), np.log(gno)
    value = lambda l, n, g: gn.value_ld(orc.Kern(kind, np.exp(l)), X, Y, G, float(np.exp(n)), np.exp(g))
    assert abs(value(lh, ln, lg) - res["value"]) <= 1e-15 * float(res["V"])
    rnd = 8 * float(np.finfo(LD).eps) * max(res["cond"], 1e6) * float(res["V"]) / gn.FD_H
    worst = [0.0, 0.0]

    def check(what, fun, g, scale):
        est, trunc = gn.richardson(fun, gn.FD_H)
        tol = float(trunc) + rnd
        err = abs(float(est - g))
        worst[0] = max(worst[0], err / tol); worst[1] = max(worst[1], err / float(scale))
        assert err <= tol, (kind, what, float(g), float(est), tol)

    assert len(res["grad"]) == len(hyper)
    for i in range(len(lh)):
        def f(h, i=i):
            l = lh.copy(); l[i] += h
            return value(l, ln, lg)
        check("hyper %d" % i, f, res["grad"][i], res["G"][i])
    check("noise", lambda h: value(lh, ln + h, lg), res["gnoise"][0], res["Gnoise"][0])
    for e in range(D):
        def f(h, e=e):
            g = lg.copy(); g[e] += h
            return value(lh, ln, g)
        check("gnoise %d" % e, f, res["gnoise"][1 + e], res["Gnoise"][1 + e])
    print("%s: worst share of the difference quotient's own error %.3f, worst error / sum of term magnitudes %.2e" % (kind, worst[0], worst[1]))


F64_CASES = [n for n in gn.DEVICE_CASES if not gr.is_big(n)]


@pytest.mark.parametrize("name", F64_CASES)
def test_float64_against_long_double_within_half_the_bar(name):
    c = gn.case(name)
    got = gn.nlml(c["kern"], c["X"], c["Y"], c["G"], c["noise"], c["gnoise"])
    ref = gn.nlml(c["kern"], c["X"], c["Y"], c["G"], c["noise"], c["gnoise"], longdouble=True, cond=got["cond"])
    rv, rg, rn = gn.shares(got["value"], got["grad"], got["gnoise"], ref)
    print("%s: P = %d, cond_2 = %.3g, worst shares of the bar: value %.3g, hyper %.3g, noise %.3g" % (name, ref["P"], ref["cond"], rv, np.max(rg), np.max(rn)))
    assert rv <= 0.5 and np.all(rg <= 0.5) and np.all(rn <= 0.5), (rv, rg, rn)


@pytest.mark.parametrize("N,D", [(9, 3), (16, 2)])
def test_iso_gradient_is_the_sum_of_the_ard_components_at_equal_length_scales(N, D):
    X = gr.points(N, D, 5)
    Y, G = gr.objective(X)
    iso = gn.nlml(orc.Kern("iso", [0.6]), X, Y, G, 0.05, 1e-3, longdouble=True)
    ard = gn.nlml(orc.Kern("ard", [0.6] * D), X, Y, G, 0.05, 1e-3, longdouble=True)
    assert abs(iso["value"] - ard["value"]) <= 1e-17 * float(iso["V"])
    # (two orders of summation of the same long-double terms, through an inverse that carries cond_2 times the long-double unit)
    assert abs(iso["grad"][0] - ard["grad"].sum()) <= 8 * float(np.finfo(LD).eps) * max(iso["cond"], 1e6) * float(iso["G"][0])
    assert np.all(np.abs(iso["gnoise"] - ard["gnoise"]) <= 1e-17 * np.asarray(iso["Gnoise"]))


@pytest.mark.parametrize("name", ["ard_16x3", "iso_32x3", "ard_60x3_gn", "se_1x1"])
@pytest.mark.parametrize("dt", [np.float64, LD])
def test_unit_signal_variance_gives_the_fit_matrix_bit_for_bit(name, dt):
    c = gn.case(name)
    assert c["kern"].sf2_py == 1.0
    assert np.array_equal(gn.matrix_nl(c["kern"], c["X"], c["noise"], c["gnoise"], dt), gr.matrix(c["kern"], c["X"], c["noise"], c["gnoise"], dt))


def test_another_signal_variance_changes_the_value_rows_only():
    c = gn.case("sviso_20x2")
    A, F = gn.matrix_nl(c["kern"], c["X"], c["noise"], c["gnoise"]), gr.matrix(c["kern"], c["X"], c["noise"], c["gnoise"])
    d = np.diag(A - F).reshape(-1, 3)
    assert np.all(d[:, 1:] == 0.0) and np.allclose(d[:, 0], c["kern"].sf2_py - 1.0, rtol=0, atol=4 * 2.0 ** -52)      # (three roundings near 1)
    assert np.array_equal(A - np.diag(np.diag(A)), F - np.diag(np.diag(F)))


@pytest.mark.parametrize("name", [n for n in gn.DEVICE_CASES if gr.is_big(n)])
def test_big_cases_are_admissible(name):
    c = gn.case(name)
    cu = gn.cond_upper_nl(c["kern"], c["X"], c["noise"], c["gnoise"])
    print("%s: cond_upper %.3g" % (name, cu))
    assert cu <= 1e6


def test_cond_upper_bounds_cond_2():
    for name in ("m3_21x2", "sviso_20x2", "ard_60x3_gn"):
        c = gn.case(name)
        cu = gn.cond_upper_nl(c["kern"], c["X"], c["noise"], c["gnoise"])
        assert np.linalg.cond(gn.matrix_nl(c["kern"], c["X"], c["noise"], c["gnoise"])) <= cu


def test_device_cases_cover_the_shapes():
    shapes = {n: (gn.case(n)["X"].shape) for n in gn.DEVICE_CASES if not gr.is_big(n)}
    P = sorted((N * (D + 1)) for N, D in shapes.values())
    for want in (2, 60, 63, 64, 65, 68, 124, 128, 129, 132, 153, 1025):
        assert want in P, want
    assert shapes["svard_3x64"] == (3, 64) and len(gn.spec_of(gn.case("svard_3x64")["kern"])) == 65
    assert gn.case("ard_60x4")["noise"] == 0.01 and len(set(gn.case("ard_60x3_gn")["gnoise"])) == 3
    X = gn.case("m3_10x2_twin")["X"]
    assert np.array_equal(X[2], X[5])


# ---------------------------------------------------------------------------- the Python surface
def test_symbols_declared_exported_and_bound():
    from ibo_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "ibo_abi.h")).read()
    for s in ("ibo_ggp_nlml_grad", "ibo_ggp_grad_stage_ms"):
        assert re.search(r"\bint\s+%s\s*\(" % s, hdr), "%s is not declared in ibo_abi.h" % s
        assert hasattr(_lib.lib, s), "libibo_hip.so does not export %s" % s
        assert s in _lib.EXPORTED, s
        assert getattr(_lib.lib, s).argtypes, "%s is not bound" % s
    assert re.search(r"#define\s+IBO_ABI_VERSION\s+8\b", hdr) and _lib.lib.ibo_abi_version() == 8
    assert re.search(r"#define\s+IBO_GGP_GRAD_STAGES\s+4\b", hdr)


def test_refusals_name_the_new_function_and_shapes_are_checked():
    from ibo_amd.gaussianprocess import GaussianProcess, trainhyper
    from ibo_amd.gaussianprocess.kernel import GaussianKernel_iso
    X = gr.points(4, 2, 1)
    Y, G = gr.objective(X)
    k = GaussianKernel_iso([0.5])
    for fn, args in ((trainhyper.marginalLikelihood, (k, X, Y, 1)), (trainhyper.looLikelihood, (k, X, Y, 1)), (trainhyper.nlml_values, ([k], X, Y))):
        with pytest.raises(NotImplementedError, match="gradientLikelihood") as e:
            fn(*args, G=G)
        assert fn.__name__ in str(e.value)
    with pytest.raises(NotImplementedError, match="gradientLikelihood"):
        trainhyper.nlml_grid(GaussianKernel_iso, [[0.5]], X, Y, G=G)
    with pytest.raises(ValueError, match="shape"):
        trainhyper.gradientLikelihood(k, X, Y, G[:, :1], 1)
    with pytest.raises(ValueError, match="gnoise"):
        trainhyper.gradientLikelihood(k, X, Y, G, 1, gnoise=[1e-3, 1e-3, 1e-3])
    plain = GaussianProcess(k)
    with pytest.raises(NotImplementedError, match="trainhyper.nlml"):
        plain.learn()
    with pytest.raises(NotImplementedError, match="trainhyper.marginalLikelihood"):
        plain.nlml()

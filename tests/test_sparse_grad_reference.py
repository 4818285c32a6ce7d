"""
The sparse marginal likelihood's gradient on the CPU: tests/sparse_grad_reference.py (the formulas of DESIGN 4.30 in NumPy) against central
differences of sparse_reference's long-double value, in float64 against long double at a tenth of the project's bar, its exact special
cases, and the Python surface of ibo_sgp_nlml_grad.  No GPU.
"""
import functools
import math
import os

import numpy as np
import pytest

from oracle import oracle as orc
import sparse_reference as sr
import sparse_grad_reference as sg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (name, kernel kind, hyper, D, shift): N = 120, m = 12, noise 0.05, jitter 1e-6 -- every family, sf2 != 1, inputs at 100
FD_CASES = [("ard", "ard", [0.5, 0.7, 0.6], 3, 0.0), ("iso", "iso", [0.6], 2, 0.0), ("m3", "m3", [0.6, 0.9], 2, 0.0), ("m5", "m5", [0.5, 0.9], 2, 0.0),
            ("sviso", "sviso", [0.6, 0.9], 2, 0.0), ("ard_shift", "ard", [0.5, 0.7, 0.6], 3, 100.0)]
FD_N, FD_M, FD_NOISE, FD_JITTER, FD_H = 120, 12, 0.05, 1e-6, 1e-3


@functools.lru_cache(maxsize=None)
def fd_case(name):
    _, kname, hyper, D, shift = [c for c in FD_CASES if c[0] == name][0]
    rng = np.random.RandomState(77 + sum(ord(ch) for ch in name))
    X = rng.rand(FD_N, D)
    Y = sr.objective(X) + 0.2 * rng.randn(FD_N)
    Z = rng.rand(FD_M, D)
    return kname, np.array(hyper, dtype=float), D, Z + shift, X + shift, Y


def _fd_tol(res, h):
    """the rounding of a difference quotient of the long-double value: its explicit inverses carry cond_2 times the long-double unit
    (res['f'] is 1e-15 max(cond_2(A), cond_2(K~uu), 1e6))"""
    return 8 * float(np.finfo(np.longdouble).eps) * (res["f"] / 1e-15) * res["model"]["nlml_scale"] / h


@pytest.mark.parametrize("via", ["route", "dense"])
@pytest.mark.parametrize("kind", sg.KINDS)
@pytest.mark.parametrize("name", [c[0] for c in FD_CASES])
def test_long_double_gradient_against_central_differences(name, kind, via):
    kname, hyper, D, Z, X, Y = fd_case(name)
    res = sg.gradient(orc.Kern(kname, hyper), Z, X, Y, FD_NOISE, FD_JITTER, kind, longdouble=True)
    gh, _ = sg.hyper_of(res, sg.grad_spec(kname, D))
    lh, ln = np.log(hyper), math.log(FD_NOISE)
    value = lambda l, n, z: sg.value_at(kname, l, n, z, X, Y, FD_JITTER, kind, via)
    assert abs(value(lh, ln, Z) - res["value"]) <= 1e-12 * res["model"]["nlml_scale"]
    rnd = _fd_tol(res, FD_H)
    worst = 0.0

    def check(what, fun, g):
        nonlocal worst
        est, trunc = sg.richardson(fun, FD_H, 0.0)
        tol = float(trunc) + rnd
        worst = max(worst, abs(float(est - g)) / tol)
        assert abs(float(est - g)) <= tol, (name, kind, via, what, float(g), float(est), tol)

    for i in range(len(lh)):
        def f(h, i=i):
            l = lh.copy(); l[i] += h
            return value(l, ln, Z)
        check("hyper %d" % i, f, gh[i])
    check("noise", lambda h: value(lh, ln + h, Z), res["noise"])
    coords = [(0, 0), (FD_M // 2, D - 1), (FD_M - 1, 0)] if via == "route" else [(FD_M // 2, D - 1)]
    for a, d in coords:
        def f(h, a=a, d=d):
            Z2 = Z.copy(); Z2[a, d] += h
            return value(lh, ln, Z2)
        check("Z %d %d" % (a, d), f, res["Z"][a, d])
    print("%s %s %s: worst share of the difference quotient's own error %.3f" % (name, kind, via, worst))


F64_CASES = [("m1_n1", None), ("m16_n200", None), ("m64_n300_j8", None), ("m100_n300_zsub", None), ("m64_n33", None), ("m40_n500_sf2", None),
             ("m20_n150_d33", "dtc"), ("m20_n150_d33", "vfe"), ("m32_n400_shift", None)]


def case_kind(name, kind=None):
    c = sr.case(name)
    return kind if kind is not None else ("fitc" if c["method"] == sr.FITC else "dtc")


@functools.lru_cache(maxsize=None)
def case_gradient(name, kind, longdouble):
    c = sr.case(name)
    return sg.gradient(c["kern"], c["Z"], c["X"], c["Y"], c["noise"], c["jitter"], kind, longdouble=longdouble)


def shares(got, ref, spec):
    """the worst |got - ref| / bar per block, the bar from the reference's term magnitudes"""
    f = ref["f"]
    gh, _ = sg.hyper_of(got, spec); rh, ra = sg.hyper_of(ref, spec)
    out = dict(hyper=float(np.max(np.abs(gh - rh) / (f * ra))), noise=float(abs(got["noise"] - ref["noise"]) / (f * ref["noise_abs"])))
    out["Z"] = float(np.max(np.abs(got["Z"] - ref["Z"]) / (f * ref["Z_abs"])))
    return out


@pytest.mark.parametrize("name,kind", F64_CASES)
def test_float64_against_long_double_within_a_tenth_of_the_bar(name, kind):
    kind = case_kind(name, kind)
    c = sr.case(name)
    ref = case_gradient(name, kind, True)
    got = sg.gradient(c["kern"], c["Z"], c["X"], c["Y"], c["noise"], c["jitter"], kind, longdouble=False, indicator=ref["ind"])
    s = shares(got, ref, sg.grad_spec(c["kind"], c["D"]))
    print("%s %s: f = %.2e, worst shares of the bar %s" % (name, kind, ref["f"], s))
    assert max(s.values()) <= sg.WORST_SHARE_F64, s


def rel_errors(got, ref, spec):
    """|g - ref| / |ref| in the 2-norm per block (the noise: one number)"""
    gh, _ = sg.hyper_of(got, spec); rh, _ = sg.hyper_of(ref, spec)
    return dict(hyper=float(np.linalg.norm((gh - rh).astype(float)) / np.linalg.norm(rh.astype(float))),
                noise=float(abs(got["noise"] - ref["noise"]) / abs(ref["noise"])),
                Z=float(np.linalg.norm((np.asarray(got["Z"]) - ref["Z"]).astype(float)) / np.linalg.norm(ref["Z"].astype(float))))


@pytest.mark.parametrize("name,kind", sorted(sg.REL_F64))
def test_well_conditioned_relative_error_is_the_recorded_one(name, kind):
    """the well-conditioned cases: the float64 restatement's relative error per block, the worst over five orders of the observations,
    stays within what sparse_grad_reference records -- the device test holds ten times that"""
    c = sr.case(name)
    ref = case_gradient(name, kind, True)
    assert ref["f"] <= 2e-9 or name == "m16_n200"
    rel = {}
    for seed in sg.REL_ORDERS:                                  # the same problem with its observations in another order: another draw of the rounding
        p = np.arange(c["N"]) if seed is None else np.random.RandomState(seed).permutation(c["N"])
        got = sg.gradient(c["kern"], c["Z"], c["X"][p], c["Y"][p], c["noise"], c["jitter"], kind, longdouble=False)
        for k, v in rel_errors(got, ref, sg.grad_spec(c["kind"], c["D"])).items():
            rel[k] = max(rel.get(k, 0.0), v)
    print("%s %s float64 against long double, relative per block, worst of %d orders: %s" % (name, kind, len(sg.REL_ORDERS), rel))
    for k in rel:
        assert rel[k] <= sg.REL_F64[name, kind][k], rel


def test_every_well_conditioned_case_is_recorded():
    """REL_F64 holds every case with f <= 2e-9 under its own objective (the DTC cases also as vfe where the device test runs them so),
    m1_n1 apart (see the file)"""
    for name in sr.CASE_NAMES:
        kind = case_kind(name)
        if sr.case_model(name)["f"] <= 2e-9 and name != "m1_n1":
            assert (name, kind) in sg.REL_F64, name


@pytest.mark.parametrize("name", ["m65_n1000", "m20_n150_d33"])
def test_vfe_noise_gradient_is_dtc_minus_trace_term(name):
    c = sr.case(name)
    d = case_gradient(name, "dtc", False); v = case_gradient(name, "vfe", False)
    tt = float(d["model"]["tt"])
    want = d["noise"] - tt / (2 * c["noise"])
    assert abs(v["noise"] - want) <= 4 * np.finfo(float).eps * (abs(d["noise"]) + tt / (2 * c["noise"]))
    assert float(v["value"]) == float(d["value"] + d["model"]["tt"] / (2 * c["noise"]))


def test_dtc_gradient_does_not_depend_on_q():
    c = sr.case("m64_n31")
    a = sg.gradient(c["kern"], c["Z"], c["X"], c["Y"], c["noise"], c["jitter"], "dtc", indicator=np.zeros(c["N"]))
    b = sg.gradient(c["kern"], c["Z"], c["X"], c["Y"], c["noise"], c["jitter"], "dtc", indicator=np.ones(c["N"]))
    for k in ("Z", "L", "sf", "noise"):
        assert np.array_equal(np.asarray(a[k]), np.asarray(b[k])), k


# ---------------------------------------------------------------------------- the Python surface
def test_symbols_declared_exported_and_bound():
    from ibo_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "ibo_abi.h")).read()
    for s in ("ibo_sgp_nlml_grad", "ibo_sgp_grad_stage_ms"):
        assert "int %s(" % s in hdr, s
        assert s in _lib.EXPORTED, s
        assert getattr(_lib.lib, s).argtypes is not None, s
    assert "#define IBO_SGP_VFE  2" in hdr
    assert _lib.lib.ibo_abi_version() == 8


def test_learn_and_gradient_need_data():
    from ibo_amd.gaussianprocess import SparseGaussianProcess
    from ibo_amd.gaussianprocess.kernel import GaussianKernel_ard
    from ibo_amd.gaussianprocess import trainhyper
    model = SparseGaussianProcess(GaussianKernel_ard([0.3, 0.3]), m=4)
    with pytest.raises(ValueError):
        model.nlml_gradient()
    with pytest.raises(ValueError):
        model.learn()
    assert callable(trainhyper.sparseLikelihood)

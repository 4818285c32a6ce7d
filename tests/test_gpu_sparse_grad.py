"""
ibo_sgp_nlml_grad -- the sparse marginal likelihood's gradient with respect to the log hyper-parameters, the log noise and the inducing
points, for fitc / dtc / vfe -- and what is built on it: SparseGaussianProcess.nlml_gradient / .learn and trainhyper.sparseLikelihood.

The yardstick is tests/sparse_grad_reference.py (pinned by tests/test_sparse_grad_reference.py) in long double; every case is one of
sparse_reference.CASES, plus one D = 64 case.  THE BAR, for every hyper component, the noise and every entry of grad_Z:
    |g - ref| <= 1e-15 max(cond_2(A), cond_2(K~uu), 1e6) x the sum of the magnitudes of the component's terms
with the FITC indicator [1 - q_i > 0] taken from the device's own lambda (as sparse_reference.gram takes lambda as given).  On the
well-conditioned cases the reference records (f <= 2e-9, and m16_n200), additionally ten times the float64 restatement's relative error per block.
Values, repeated calls, partial outputs and arbitrary modes / dims lists: bit for bit.
"""
import ctypes
import functools

import numpy as np
import pytest

from oracle import oracle as orc
import sparse_reference as sr
import sparse_grad_reference as sg

pytestmark = pytest.mark.gpu
GUARD = 7.25

# (case, objective): the case's own method, and the DTC cases again as vfe
GRAD_CASES = [("m1_n1", "fitc"), ("m16_n200", "fitc"), ("m63_n1000", "fitc"), ("m64_n1000", "fitc"), ("m65_n1000", "dtc"), ("m65_n1000", "vfe"),
              ("m129_n2100", "dtc"), ("m129_n2100", "vfe"), ("m130_n2100", "fitc"), ("m100_n300_zsub", "fitc"), ("m64_n300_j8", "fitc"),
              ("m64_n1000_lownoise", "fitc"), ("m64_n33", "fitc"), ("m64_n31", "dtc"), ("m32_n400_shift", "fitc"), ("m40_n500_sf2", "fitc"),
              ("m20_n150_d33", "dtc"), ("m20_n150_d33", "vfe"), ("m65_n300_d64", "fitc")]


@pytest.fixture(scope="module")
def lib():
    from ibo_amd import _lib
    if _lib.device_count() < 1:
        pytest.fail("no GPU visible: the product has no CPU fallback")
    return _lib


@functools.lru_cache(maxsize=None)
def case(name):
    if name != "m65_n300_d64":
        return sr.case(name)
    rng = np.random.RandomState(6465)                           # the dimension loop at its limit: D = 64, m = 65, N = 300
    D, m, N, noise = 64, 65, 300, 0.05
    X = rng.rand(N, D)
    Y = np.sin(3.0 * np.sum(X[:, :3], axis=1)) + np.sqrt(noise) * rng.randn(N)
    return dict(name=name, kern=orc.Kern("iso", [4.0]), kind="iso", hyper=[4.0], D=D, m=m, N=N, noise=noise, jitter=1e-6, method=sr.FITC,
                Z=rng.rand(m, D), X=X, Y=Y)


def call(L, c, kind, spec=None, want=("hyper", "noise", "Z"), noise=None, jitter=None, Z=None, X=None, kind_code=None):
    """the raw entry with guard cells behind every output: dict(rc, value, hyper, noise, Z, info)"""
    ktype, hyper, sf2 = sr.device_spec(c["kern"])
    spec = sg.grad_spec(c["kind"], c["D"]) if spec is None else spec
    n = len(spec) if "hyper" in want else 0
    Z = L.f64(c["Z"] if Z is None else Z); X = L.f64(c["X"] if X is None else X); Y = L.f64(c["Y"])
    m, D = Z.shape
    modes = (ctypes.c_int * max(n, 1))(*[s[0] for s in spec[:n]]); dims = (ctypes.c_int * max(n, 1))(*[s[1] for s in spec[:n]])
    v = np.full(2, GUARD); gh = np.full(n + 8, GUARD); gn = np.full(2, GUARD); gz = np.full(m * D + 8, GUARD)
    info = ctypes.c_int(-1)
    rc = L.lib.ibo_sgp_nlml_grad(L.default_device(), ktype, D, L.dp(hyper), len(hyper), sf2, float(c["noise"] if noise is None else noise),
                                 float(c["jitter"] if jitter is None else jitter), sg.KIND_CODE[kind] if kind_code is None else kind_code,
                                 m, L.dp(Z), len(X), L.dp(X), L.dp(Y), n, modes, dims, L.dp(v), L.dp(gh) if n else None,
                                 L.dp(gn) if "noise" in want else None, L.dp(gz) if "Z" in want else None, ctypes.byref(info))
    assert v[1] == GUARD and gn[1] == GUARD and np.all(gh[n:] == GUARD) and np.all(gz[m * D:] == GUARD), "a guard cell was overwritten"
    return dict(rc=rc, value=v[0], hyper=gh[:n].copy(), noise=gn[0], Z=gz[:m * D].reshape(m, D).copy(), info=info.value,
                untouched=bool(v[0] == GUARD and gn[0] == GUARD and np.all(gh == GUARD) and np.all(gz == GUARD)))


def fitted(L, c, method):
    """(handle, lambda) of a plain ibo_sgp_fit with the same arguments"""
    ktype, hyper, sf2 = sr.device_spec(c["kern"])
    h = ctypes.c_void_p()
    L.check(L.lib.ibo_sgp_create(L.default_device(), ctypes.byref(h)))
    lam = np.empty(c["N"])
    info = ctypes.c_int(0)
    Z = L.f64(c["Z"]); X = L.f64(c["X"]); Y = L.f64(c["Y"])
    L.check(L.lib.ibo_sgp_fit(h, ktype, c["D"], L.dp(hyper), len(hyper), sf2, float(c["noise"]), float(c["jitter"]), method, len(Z), L.dp(Z),
                              len(X), L.dp(X), L.dp(Y), L.dp(lam), ctypes.byref(info)))
    return h, lam


@functools.lru_cache(maxsize=None)
def device_indicator(name):
    """[1 - q_i > 0] as the device's own FITC lambda says it: lambda_i > noise"""
    from ibo_amd import _lib as L
    c = case(name)
    h, lam = fitted(L, c, sr.FITC)
    L.check(L.lib.ibo_sgp_destroy(h))
    return tuple(bool(b) for b in lam > c["noise"])


@functools.lru_cache(maxsize=None)
def reference(name, kind):
    """long double (every case here has m <= LD_MAX_M); computed once and shared"""
    c = case(name)
    assert c["m"] <= sr.LD_MAX_M
    ind = np.array(device_indicator(name)) if kind == "fitc" else None
    return sg.gradient(c["kern"], c["Z"], c["X"], c["Y"], c["noise"], c["jitter"], kind, longdouble=True, indicator=ind)


def bar_shares(got, ref, spec):
    f = ref["f"]
    rh, ra = sg.hyper_of(ref, spec)
    return dict(hyper=float(np.max(np.abs(got["hyper"] - rh) / (f * ra))) if len(spec) else 0.0,
                noise=float(abs(got["noise"] - ref["noise"]) / (f * ref["noise_abs"])),
                Z=float(np.max(np.abs(got["Z"] - ref["Z"]) / (f * ref["Z_abs"]))),
                value=float(abs(got["value"] - ref["value"]) / (f * ref["model"]["nlml_scale"])))


@pytest.mark.parametrize("name,kind", GRAD_CASES)
def test_gradient_within_the_bar(lib, name, kind):
    c = case(name)
    spec = sg.grad_spec(c["kind"], c["D"])
    got = call(lib, c, kind)
    assert got["rc"] == lib.OK, lib.lib.ibo_last_error()
    ref = reference(name, kind)
    s = bar_shares(got, ref, spec)
    print("%s %s: f = %.2e, worst shares of the bar %s" % (name, kind, ref["f"], s))
    assert max(s.values()) <= 1.0, s
    if (name, kind) in sg.REL_F64:
        rh, _ = sg.hyper_of(ref, spec)
        rel = dict(hyper=float(np.linalg.norm((got["hyper"] - rh).astype(float)) / np.linalg.norm(rh.astype(float))),
                   noise=float(abs(got["noise"] - ref["noise"]) / abs(ref["noise"])),
                   Z=float(np.linalg.norm((got["Z"] - ref["Z"]).astype(float)) / np.linalg.norm(ref["Z"].astype(float))))
        print("%s %s: relative error per block %s" % (name, kind, rel))
        for k in rel:
            assert rel[k] <= sg.REL_DEVICE_FACTOR * sg.REL_F64[name, kind][k], rel


@pytest.mark.parametrize("name,kind", [("m16_n200", "fitc"), ("m65_n1000", "dtc"), ("m65_n1000", "vfe"), ("m130_n2100", "fitc")])
def test_value_is_ibo_sgp_nlml_bit_for_bit(lib, name, kind):
    c = case(name)
    h, _ = fitted(lib, c, sr.FITC if kind == "fitc" else sr.DTC)
    v = ctypes.c_double()
    lib.check(lib.lib.ibo_sgp_nlml(h, 1 if kind == "vfe" else 0, ctypes.byref(v)))
    lib.check(lib.lib.ibo_sgp_destroy(h))
    got = call(lib, c, kind)
    assert got["rc"] == lib.OK and got["value"] == v.value
    assert call(lib, c, kind, want=())["value"] == v.value      # (no gradient asked for: the fit alone)


def same_bits(a, b, keys=("value", "hyper", "noise", "Z")):
    return all(np.array_equal(np.asarray(a[k]), np.asarray(b[k])) for k in keys)


@pytest.mark.parametrize("name,kind", [("m130_n2100", "fitc"), ("m129_n2100", "vfe")])
def test_two_calls_give_the_same_bits(lib, name, kind):
    c = case(name)
    a = call(lib, c, kind)
    lib.check(lib.lib.ibo_trim(lib.default_device()))           # (the private handle is made anew)
    b = call(lib, c, kind)
    assert a["rc"] == lib.OK and same_bits(a, b)


@pytest.mark.parametrize("name,kind", [("m130_n2100", "fitc"), ("m129_n2100", "vfe")])
def test_chunkings_agree_within_the_bar(lib, name, kind):
    c = case(name)
    spec = sg.grad_spec(c["kind"], c["D"])
    ref = reference(name, kind)
    try:
        for chunk in (256, 512, 8192):
            lib.check(lib.lib.ibo_set_option(b"sgp_chunk", chunk))
            got = call(lib, c, kind)
            assert got["rc"] == lib.OK
            s = bar_shares(got, ref, spec)
            print("%s %s sgp_chunk=%d: %s" % (name, kind, chunk, s))
            assert max(s.values()) <= 1.0, (chunk, s)
    finally:
        lib.check(lib.lib.ibo_set_option(b"sgp_chunk", 0))


def test_partial_outputs_keep_their_bits(lib):
    c = case("m64_n1000")
    full = call(lib, c, "fitc")
    noZ = call(lib, c, "fitc", want=("hyper", "noise"))
    noH = call(lib, c, "fitc", want=("noise", "Z"))
    onlyZ = call(lib, c, "fitc", want=("Z",))
    assert same_bits(full, noZ, ("value", "hyper", "noise")) and np.all(noZ["Z"] == GUARD)
    assert same_bits(full, noH, ("value", "noise", "Z")) and len(noH["hyper"]) == 0
    assert same_bits(full, onlyZ, ("value", "Z")) and onlyZ["noise"] == GUARD


def test_a_component_keeps_its_bits_in_any_list(lib):
    c = case("m64_n1000")                                       # ard, D = 4
    full = call(lib, c, "fitc", spec=[(0, 0), (0, 1), (0, 2), (0, 3), (2, 0)])
    mixed = call(lib, c, "fitc", spec=[(2, 0), (0, 3), (0, 0), (0, 3)])
    assert mixed["rc"] == lib.OK
    assert np.array_equal(mixed["hyper"], full["hyper"][[4, 3, 0, 3]])
    assert same_bits(full, mixed, ("value", "noise", "Z"))
    c = case("m40_n500_sf2")                                    # sviso: the length scale and the magnitude swapped
    a = call(lib, c, "fitc"); b = call(lib, c, "fitc", spec=[(2, 0), (1, 0)])
    assert np.array_equal(b["hyper"], a["hyper"][::-1])


def test_errors_leave_the_outputs_untouched(lib):
    c = case("m16_n200")
    X = c["X"].copy(); X[3, 1] = np.nan
    for r in (call(lib, c, "fitc", X=X), call(lib, c, "fitc", noise=0.0), call(lib, c, "fitc", noise=float("inf")),
              call(lib, c, "fitc", kind_code=3), call(lib, c, "fitc", spec=[(0, 7)]), call(lib, c, "fitc", spec=[(5, 0)])):
        assert r["rc"] == lib.ERR_ARG and r["untouched"]
    ok = call(lib, c, "fitc", kind_code=2)                      # kind 2 with nothing else wrong: the bound of a DTC fit
    assert ok["rc"] == lib.OK and np.isfinite(ok["value"])
    Z = c["Z"].copy(); Z[1] = Z[0]                              # coincident inducing points, no jitter: the second pivot is 1 - 1 = 0 exactly
    r = call(lib, c, "fitc", Z=Z, jitter=0.0)
    assert r["rc"] == lib.ERR_NOT_PD and r["untouched"] and r["info"] >= 1
    good = call(lib, c, "fitc")                                 # an error path, not a fault: the next call is served
    assert good["rc"] == lib.OK and same_bits(good, call(lib, c, "fitc"))


# ---------------------------------------------------------------------------- Python
def py_kernel(c):
    from ibo_amd.gaussianprocess import kernel as K
    cls = {"ard": K.GaussianKernel_ard, "iso": K.GaussianKernel_iso, "sviso": K.SVGaussianKernel_iso, "m3": K.MaternKernel3, "m5": K.MaternKernel5}
    return cls[c["kind"]](c["hyper"])


@pytest.mark.parametrize("name,method,kind", [("m16_n200", "fitc", None), ("m65_n1000", "dtc", None), ("m65_n1000", "dtc", "dtc"), ("m40_n500_sf2", "fitc", "fitc")])
def test_nlml_gradient_and_sparse_likelihood_are_the_raw_entry(lib, name, method, kind):
    from ibo_amd.gaussianprocess import SparseGaussianProcess, trainhyper
    c = case(name)
    model = SparseGaussianProcess(py_kernel(c), c["X"], c["Y"], Z=c["Z"], noise=c["noise"], jitter=c["jitter"], method=method)
    objective = kind if kind is not None else ("vfe" if method == "dtc" else method)
    raw = call(lib, c, objective)
    v, g = model.nlml_gradient(kind)
    assert v == raw["value"] and np.array_equal(g["hyper"], raw["hyper"]) and g["noise"] == raw["noise"] and np.array_equal(g["Z"], raw["Z"])
    assert v == model.nlml(None if objective != "vfe" else "vfe")
    v2, g2 = model.nlml_gradient(kind, wrt=("noise",))
    assert v2 == v and set(g2) == {"noise"} and g2["noise"] == raw["noise"]
    sv, sh, sn, sz = trainhyper.sparseLikelihood(model.kernel, c["X"], c["Y"], c["Z"], len(raw["hyper"]), c["noise"], jitter=c["jitter"], kind=objective)
    assert sv == v and np.array_equal(sh, raw["hyper"]) and sn == raw["noise"] and np.array_equal(sz, raw["Z"])
    assert trainhyper.sparseLikelihood(model.kernel, c["X"], c["Y"], c["Z"], 1, c["noise"], jitter=c["jitter"], kind=objective, computeGradient=False) == v
    if c["kern"].sf2_py == 1.0:                                 # coincident inducing points, no jitter, k = 1 between them: the second pivot of
        Z = c["Z"].copy(); Z[1] = Z[0]                          # K~uu is 0 exactly -- LinAlgError, as marginalLikelihood raises it
        with pytest.raises(np.linalg.LinAlgError):
            trainhyper.sparseLikelihood(model.kernel, c["X"], c["Y"], Z, 1, c["noise"], jitter=0.0, kind=objective)
    model.close()


@pytest.mark.parametrize("method", ["dtc", "fitc"])
def test_learn_lowers_the_objective_and_refits(lib, method, monkeypatch):
    from ibo_amd.gaussianprocess import GaussianProcess, SparseGaussianProcess
    from ibo_amd.gaussianprocess.kernel import GaussianKernel_ard
    c = case("m16_n200")
    plain = GaussianProcess(GaussianKernel_ard(c["hyper"]), c["X"][:50], c["Y"][:50], noise=c["noise"])
    before = plain.posteriors(c["Q"][:64])
    start = GaussianKernel_ard(3.0 * np.asarray(c["hyper"]))     # length scales 3 x off, noise 10 x off
    model = SparseGaussianProcess(start, c["X"], c["Y"], Z=c["Z"], noise=10 * c["noise"], jitter=c["jitter"], method=method)
    v0 = model.nlml("vfe" if method == "dtc" else None)
    res = model.learn(maxiter=15)
    assert res.start_value == v0 and res.end_value < res.start_value
    assert model.nlml("vfe" if method == "dtc" else None) <= v0
    fresh = SparseGaussianProcess(model.kernel.__class__(model.kernel.hyperparams), c["X"], c["Y"], Z=model.Z, noise=model.noise, jitter=c["jitter"], method=method)
    a, b = model.posteriors(c["Q"][:64]), fresh.posteriors(c["Q"][:64])
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    fresh.close()
    assert res.applied
    # a refit that fails ON THE DEVICE leaves the old handle answering: coincident inducing points without jitter (sf2 = 1: the second
    # pivot of K~uu is 0 exactly) through _fit, the route learn() and refit() share
    keep = model.kernel, model.noise, model.Z.copy(), model.jitter
    dup = model.Z.copy(); dup[1] = dup[0]
    model.jitter = 0.0
    with pytest.raises(np.linalg.LinAlgError):
        model.refit(Z=dup)
    assert np.array_equal(model.Z, keep[2])
    # ... and a start that does not factor is not a result: nothing is applied, nothing refitted
    model.Z = dup
    res2 = model.learn(maxiter=2, learn_Z=False)
    assert not res2.applied and not np.isfinite(res2.end_value) and np.array_equal(model.Z, dup) and model.kernel is keep[0] and model.noise == keep[1]
    model.Z, model.jitter = keep[2], keep[3]
    a2 = model.posteriors(c["Q"][:64])
    assert np.array_equal(a[0], a2[0]) and np.array_equal(a[1], a2[1])
    # learn()'s own restore when the refit after a successful search fails
    other = SparseGaussianProcess(start, c["X"], c["Y"], Z=c["Z"], noise=10 * c["noise"], jitter=c["jitter"], method=method)
    o0 = other.posteriors(c["Q"][:64])
    okeep = other.kernel, other.noise, other.Z.copy()

    def broken(X, Y):
        raise lib.NotPositiveDefinite(lib.ERR_NOT_PD, "refit refused")
    monkeypatch.setattr(other, "_fit", broken)
    with pytest.raises(np.linalg.LinAlgError):
        other.learn(maxiter=3)
    assert other.kernel is okeep[0] and other.noise == okeep[1] and np.array_equal(other.Z, okeep[2])
    o1 = other.posteriors(c["Q"][:64])
    assert np.array_equal(o0[0], o1[0]) and np.array_equal(o0[1], o1[1])
    other.close()
    model.close()
    after = plain.posteriors(c["Q"][:64])                        # the plain model: untouched bits
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])

"""
The constrained acquisition on the device: ibo_cacq_sweep / ibo_cacq_batch / ibo_cacq_grad_batch / ibo_cacq_direct_max and
ibo_amd.acquisition.constrained on top of them.

Tolerances
  * against the restatement (tests/cacq_reference.py, pinned to the oracle by tests/test_cacq_reference.py): the suite's own
    acquisition rule, rtol 1e-6, atol 1e-12 (RT, ACQ_ATOL of tests/test_gpu_parity.py);
  * against the composition of the library's OWN per-model outputs on the same DeviceArray (sweep(.., outputs=('mu', 's2',
    'acq'))): rtol 1e-12, atol 1e-15 -- those come through the same route and carry the same bits; at most nine factors of a
    few ulps each, and each Phi carries about one unit of 1.1e-16 absolute from erf;
  * gradients: 1e-9 of the scale + 1e-13, as tests/test_gpu_gradients.py.
"""
import ctypes

import numpy as np
import pytest
from scipy.special import erf

import grad_reference as gr
import cacq_reference as cr
import shift_reference as sr
from conftest import synth

pytestmark = pytest.mark.gpu

RT, ACQ_ATOL = 1e-6, 1e-12
OWN_RT, OWN_ATOL = 1e-12, 1e-15
NAN = float("nan")


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


def pair(kind, hyper, X, Y, noise=.1, prior=None):
    """(GaussianProcess, restatement) of one model; prior: (RBFNMeanPrior, its arrays) or None"""
    from ibo_amd.gaussianprocess import GaussianProcess
    GP = GaussianProcess(make_kernel(kind, hyper), X, Y, prior=None if prior is None else prior[0], noise=noise)
    return GP, cr.make(X, Y, noise, kind, hyper, prior=None if prior is None else prior[1])


def ref_con(GP, m, thresh, sense, native):
    """the restatement's constraint: the model with its bound and the k* variance the call uses"""
    return cr.Model(m.ref, thresh=thresh, sense=sense, sf2k=GP.kernel._ibo_spec()[3 if native else 2])


def compose(per_model, cons):
    """val, pof from the library's own per-model outputs (libm flavour): per_model[0] the objective's dict, [1 + j] constraint j's"""
    val = per_model[0]["acq"].copy()
    pof = np.ones(len(val))
    for (k, t, s) in cons:
        z = s * (t - per_model[k]["mu"]) / np.sqrt(per_model[k]["s2"])
        phi = 0.5 * (1.0 + erf(z / np.sqrt(2.0)))
        pof *= phi
        val *= phi
    return val, pof


def own_close(a, b):
    np.testing.assert_allclose(a, b, rtol=OWN_RT, atol=OWN_ATOL)


def ref_close(a, b):
    np.testing.assert_allclose(a, b, rtol=RT, atol=ACQ_ATOL)


def rows_to_check(M, n=200):
    if M <= n:
        return np.arange(M)
    return np.unique(np.r_[0, M - 1, np.random.RandomState(M).randint(0, M, n - 2)])


def pack(lib, cons):
    """(ncon, con, thresh, sense) from [(handle, thresh, sense)]"""
    n = len(cons)
    con = (ctypes.c_void_p * max(n, 1))(*[c[0] for c in cons])
    thresh = lib.f64([c[1] for c in cons] or [0.0])
    sense = (ctypes.c_int * max(n, 1))(*[c[2] for c in cons])
    return n, con, lib.dp(thresh), sense, thresh


def raw_batch(lib, obj, cons, Q, acq=0, parm=.01, erf_mode=1, clamp=1e-7, ymax=NAN, grad=False):
    """(rc, dict) of ibo_cacq_batch (acq, pof, val) or ibo_cacq_grad_batch (val, dval)"""
    Q = lib.f64(np.atleast_2d(Q))
    M, D = Q.shape
    n, con, th, se, keep = pack(lib, cons)
    if grad:
        val, dval = np.full(M, 7.25), np.full((M, D), 7.25)
        rc = lib.lib.ibo_cacq_grad_batch(obj, n, con, th, se, M, lib.dp(Q), acq, parm, erf_mode, clamp, ymax, lib.dp(val), lib.dp(dval))
        return rc, dict(val=val, dval=dval)
    out = {k: np.full(M, 7.25) for k in ("acq", "pof", "val")}
    rc = lib.lib.ibo_cacq_batch(obj, n, con, th, se, M, lib.dp(Q), acq, parm, erf_mode, clamp, ymax, lib.dp(out["acq"]),
                                lib.dp(out["pof"]), lib.dp(out["val"]))
    return rc, out


def raw_sweep(lib, obj, cons, dc, acq=0, parm=.01, erf_mode=0, clamp=1e-8, ymax=NAN):
    n, con, th, se, keep = pack(lib, cons)
    bv = ctypes.c_double(-5.0); bi = ctypes.c_int64(-5)
    rc = lib.lib.ibo_cacq_sweep(obj, n, con, th, se, dc.shape[0], dc.ptr, acq, parm, erf_mode, clamp, ymax, 0, None, .5, 0,
                                None, None, None, ctypes.byref(bv), ctypes.byref(bi))
    return rc, bv.value, bi.value


# ------------------------------------------------------------------------------------------------ combine boundaries
@pytest.fixture(scope="module")
def small_models(lib):
    """objective N = 40, D = 2, SE-iso; two Matern-5/2 constraint models with N = 33 observed at other points; one candidate
    array of 70001 rows whose prefixes the cases sweep"""
    from ibo_amd import DeviceArray
    Xo, Yo = synth(31, 40, 2)
    X1, _ = synth(32, 33, 2)
    X2, _ = synth(33, 33, 2)
    Y1 = np.cos(2 * X1[:, 0]) - X1[:, 1]
    Y2 = ((X2 - .5) ** 2).sum(1)
    obj = pair("iso", [.4], Xo, Yo)
    c1 = pair("m5", [.6, .9], X1, Y1)
    c2 = pair("m5", [.5, .95], X2, Y2)
    Q = np.random.RandomState(34).rand(70001, 2) * 1.1 - .05
    return dict(obj=obj, c=[c1, c2], Q=Q, dc=DeviceArray.from_host(Q))


# eight constraints on the two models: (model, bound kind, threshold)
EIGHT = [(0, "upper", .35), (1, "lower", .12), (0, "lower", -.6), (1, "upper", .45), (0, "upper", .5), (1, "lower", .05),
         (0, "lower", -.9), (1, "upper", .6)]


@pytest.mark.parametrize("M", [1, 255, 256, 257, 5000, 70001])
def test_combine_boundaries(lib, small_models, M):
    """the workgroup edge, several workgroups, the final reduction over more than 256 partials; 0, 1, 2 and 8 constraints"""
    from ibo_amd.acquisition import sweep
    from ibo_amd.acquisition.constrained import Constraint, sweepConstrained
    sm = small_models
    (GPo, mo), cs = sm["obj"], sm["c"]
    dc = sm["dc"].view_rows(0, M)
    Q = sm["Q"][:M]
    ymax = .6
    per_model = [sweep(GPo, dc, acq='ei', xi=.01, ymax=ymax, outputs=("mu", "s2", "acq"))] + \
                [sweep(GP, dc, acq='ei', outputs=("mu", "s2")) for GP, _ in cs]
    rows = rows_to_check(M)
    for ncon in (0, 1, 2, 8):
        cons = [Constraint(cs[k][0], **{kind: t}) for k, kind, t in EIGHT[:ncon]]
        r = sweepConstrained(GPo, cons, dc, acq='ei', xi=.01, ymax=ymax, outputs=("acq", "pof", "val"))
        assert r["acq_used"] == 'ei'
        val, pof = compose(per_model, [(1 + k, t, 1 if kind == "upper" else -1) for k, kind, t in EIGHT[:ncon]])
        assert np.array_equal(r["acq"], per_model[0]["acq"])
        own_close(r["val"], val); own_close(r["pof"], pof)
        # the arg-max rule on the entry's own values
        k, v = cr.argmax(r["val"])
        assert (r["best_idx"], r["best_val"]) == (k, v)
        if ncon == 0:                                # the same request through the same route: bit for bit
            assert np.array_equal(r["val"], per_model[0]["acq"]) and np.all(r["pof"] == 1.0)
            assert (r["best_val"], r["best_idx"]) == (per_model[0]["best_val"], per_model[0]["best_idx"])
        rcons = [ref_con(cs[k][0], cs[k][1], t, 1 if kind == "upper" else -1, True) for k, kind, t in EIGHT[:ncon]]
        ref = cr.value(mo, rcons, Q[rows], gr.ACQ_EI, .01, gr.ERF_LIBM, 1e-8, ymax)
        ref_close(r["val"][rows], ref["val"]); ref_close(r["pof"][rows], ref["pof"]); ref_close(r["acq"][rows], ref["acq"])
    if M == 257:
        nine = [(cs[0][0]._handle(), .1, 1)] * 9
        rc, _, _ = raw_sweep(lib, GPo._handle(), nine, dc)
        assert rc == lib.ERR_ARG
        assert raw_batch(lib, GPo._handle(), nine, Q)[0] == lib.ERR_ARG


def test_pof_alone_and_pi(lib, small_models):
    """IBO_ACQ_NONE: A = 1, val = P (the objective is not consulted); PI as the objective's factor"""
    from ibo_amd.acquisition import sweep
    from ibo_amd.acquisition.constrained import Constraint, sweepConstrained
    sm = small_models
    (GPo, mo), cs = sm["obj"], sm["c"]
    M = 777
    dc, Q = sm["dc"].view_rows(0, M), sm["Q"][:M]
    cons = [Constraint(cs[0][0], upper=.35), Constraint(cs[1][0], lower=.12)]
    rcons = [ref_con(cs[0][0], cs[0][1], .35, 1, True), ref_con(cs[1][0], cs[1][1], .12, -1, True)]
    r = sweepConstrained(GPo, cons, dc, acq='pof', outputs=("acq", "pof", "val"))
    assert np.all(r["acq"] == 1.0) and np.array_equal(r["val"], r["pof"])
    ref = cr.value(mo, rcons, Q, gr.ACQ_NONE, 0.0, gr.ERF_LIBM, 1e-8)
    ref_close(r["val"], ref["val"])
    assert r["best_idx"] == int(np.argmax(r["val"]))
    p = sweepConstrained(GPo, cons, dc, acq='pi', xi=.02, ymax=.5, outputs=("acq", "val"))
    assert np.array_equal(p["acq"], sweep(GPo, dc, acq='pi', xi=.02, ymax=.5, outputs=("acq",))["acq"])
    ref_close(p["val"], cr.value(mo, rcons, Q, gr.ACQ_PI, .02, gr.ERF_LIBM, 1e-8, .5)["val"])


# ------------------------------------------------------------------------------------------------ routes
def make_prior(D, seed=11):
    from ibo_amd.gaussianprocess.prior import RBFNMeanPrior
    rs = np.random.RandomState(seed)
    p = RBFNMeanPrior()
    p.means = rs.rand(5, D); p.beta = rs.randn(5); p.theta = 1.5; p.lowerb = np.zeros(D) - .1; p.width = np.full(D, 1.2)
    return p, (p.means, p.beta, p.theta, p.lowerb, p.width)


def last_kernel(lib, GP):
    ms = ctypes.c_float(); name = ctypes.c_char_p()
    lib.check(lib.lib.ibo_last_sweep_kernel_ms(GP._handle(), ctypes.byref(ms), ctypes.byref(name)))
    return name.value.decode()


@pytest.fixture(scope="module")
def route_models(lib):
    X, Y = synth(41, 600, 5)
    Xc, _ = synth(42, 600, 5)
    Yc = np.cos(2 * Xc[:, 0]) - Xc[:, -1]
    return pair("ard", [.5, .6, .7, .55, .65], X, Y, prior=make_prior(5)), pair("m3", [.9, .95], Xc, Yc)


@pytest.mark.parametrize("M,kernel", [(4096, "wk_small_kernel"), (4097, "sweep2_kernel")])
@pytest.mark.parametrize("native", [True, False])
def test_routes_small_and_large_batch(lib, route_models, M, kernel, native):
    """N = 600, D = 5, SE-ARD objective with an RBFN prior + Matern-3/2 constraint on either side of the small-batch threshold,
    native (libm erf, clamp 1e-8, libego's k* variance: 1 for the Matern-3/2 model of magnitude .95) and Python semantics"""
    from ibo_amd import DeviceArray
    from ibo_amd.acquisition import sweep
    from ibo_amd.acquisition.constrained import Constraint, sweepConstrained
    (GPo, mo), (GPc, mc) = route_models
    Q = np.random.RandomState(43).rand(M, 5)
    dc = DeviceArray.from_host(Q)
    r = sweepConstrained(GPo, [Constraint(GPc, upper=.1)], dc, acq='ei', xi=.01, native=native, outputs=("acq", "pof", "val"))
    assert last_kernel(lib, GPo) == kernel and last_kernel(lib, GPc) == kernel
    ymax = cr_incumbent(GPo, [(GPc, .1, 1)])
    rows = rows_to_check(M, 120)
    erf_mode, clamp = (gr.ERF_LIBM, 1e-8) if native else (gr.ERF_NR, 1e-7)
    ref = cr.value(mo, [ref_con(GPc, mc, .1, 1, native)], Q[rows], gr.ACQ_EI, .01, erf_mode, clamp, ymax)
    ref_close(r["val"][rows], ref["val"]); ref_close(r["pof"][rows], ref["pof"])
    assert float(np.mean(ref["val"] > 1e-6)) > .1 and np.ptp(ref["pof"]) > .5
    k, v = cr.argmax(r["val"])
    assert (r["best_idx"], r["best_val"]) == (k, v)
    if native:
        pm = [sweep(GPo, dc, acq='ei', xi=.01, ymax=ymax, outputs=("mu", "s2", "acq")), sweep(GPc, dc, outputs=("mu", "s2"))]
        val, pof = compose(pm, [(1, .1, 1)])
        own_close(r["val"], val); own_close(r["pof"], pof)
    # the k* variance is the Python one again on both handles
    mu = GPc._posterior_arrays(Q[:5])[0]
    np.testing.assert_allclose(mu, cr.posterior(ref_con(GPc, mc, .1, 1, False), Q[:5], 1e-7)[0], rtol=0, atol=1e-9)


def cr_incumbent(GPo, cons):
    """feasibleIncumbent from the library's own means, spelled out"""
    ok = np.ones(len(GPo.X), dtype=bool)
    for GP, t, s in cons:
        mu = GP._posterior_arrays(GPo.X)[0]
        ok &= (mu <= t) if s > 0 else (mu >= t)
    return float(np.max(GPo.Y[ok]))


def test_one_handle_outside_the_dot_form_guard(lib):
    """a constraint model whose scaled observations lie beyond the dot form's guard (|x~|^2 > 2e4, built as
    tests/shift_reference.py builds them) next to an objective inside it, M = 300: the two handles of one call take different
    kernels"""
    from ibo_amd import DeviceArray
    from ibo_amd.acquisition import sweep
    from ibo_amd.acquisition.constrained import Constraint, sweepConstrained
    c = sr.sweep_case("ard_d4_n200")
    t = c["t_out"]
    Xc = c["X0"] + t
    Yc = np.cos(2 * c["X0"][:, 0]) - c["X0"][:, -1]
    Xo = sr.dyadic(77, 150, 4) + t
    GPc, mc = pair("ard", c["hyper"], Xc, Yc, noise=c["noise"])
    GPo, mo = pair("iso", [1.0], Xo, sr.targets(78, Xo - t), noise=.1)
    assert sr.row_bound(Xc, c["sw"]) > sr.GUARD and sr.row_bound(Xo, np.ones(4)) < sr.GUARD
    Q = c["C0"][:300] + t
    dc = DeviceArray.from_host(Q)
    r = sweepConstrained(GPo, [Constraint(GPc, upper=.2)], dc, acq='ei', ymax=.5, outputs=("pof", "val"))
    assert last_kernel(lib, GPo) == "wk_small_kernel" and last_kernel(lib, GPc) == "sweep_mfma_kernel<split>"
    ref = cr.value(mo, [ref_con(GPc, mc, .2, 1, True)], Q, gr.ACQ_EI, .01, gr.ERF_LIBM, 1e-8, .5)
    ref_close(r["val"], ref["val"]); ref_close(r["pof"], ref["pof"])
    assert np.ptp(ref["pof"]) > .5
    pm = [sweep(GPo, dc, acq='ei', xi=.01, ymax=.5, outputs=("mu", "s2", "acq")), sweep(GPc, dc, outputs=("mu", "s2"))]
    own_close(r["val"], compose(pm, [(1, .2, 1)])[0])


# ------------------------------------------------------------------------------------------------ the generator's cases
@pytest.mark.parametrize("case", cr.GEN_CASES)
def test_generator_cases_against_the_restatement(lib, case):
    from ibo_amd.acquisition.constrained import Constraint, sweepConstrained
    g = cr.generator(*case)
    D = case[2]
    GPo, _ = pair("iso", [g["theta"]], g["X"], g["Yo"], noise=cr.GEN_NOISE)
    GP1, _ = pair("iso", [g["theta"]], g["X"], g["Yc1"], noise=cr.GEN_NOISE)
    GP2, _ = pair("iso", [g["theta"]], g["X"], g["Yc2"], noise=cr.GEN_NOISE)
    r = sweepConstrained(GPo, [Constraint(GP1, upper=g["t1"]), Constraint(GP2, lower=g["t2"])], g["Q"], acq='ei', xi=cr.GEN_XI,
                         ymax=g["ymax"], outputs=("acq", "pof", "val"))
    for k in ("acq", "pof", "val"):
        ref_close(r[k], g["ref"][k])
    assert r["best_idx"] == int(np.argmax(g["ref"]["val"]))
    ref_close(r["best_val"], float(np.max(g["ref"]["val"])))
    assert g["Q"].shape == (3000, D)


# ------------------------------------------------------------------------------------------------ arg-max rules
def test_argmax_rules(lib, small_models):
    from ibo_amd import DeviceArray
    from ibo_amd.acquisition.constrained import Constraint, sweepConstrained
    sm = small_models
    (GPo, mo), cs = sm["obj"], sm["c"]
    Q = sm["Q"][:1500]
    cons = [Constraint(cs[0][0], upper=.35), Constraint(cs[1][0], lower=.12)]
    kw = dict(acq='ei', xi=.01, ymax=.6)
    base = sweepConstrained(GPo, cons, Q, outputs=("val",), **kw)
    w = base["best_idx"]
    assert base["best_val"] > 1e-4
    # the candidate array concatenated with itself: the winner is in the first half
    twice = sweepConstrained(GPo, cons, np.r_[Q, Q], **kw)
    assert (twice["best_idx"], twice["best_val"]) == (w, base["best_val"])
    # an exclusion ball on the winner: the runner-up wins
    rad = 1e-3
    ex = sweepConstrained(GPo, cons, Q, exclude=Q[w:w + 1], exclude_radius=rad, **kw)
    k, v = cr.argmax(base["val"], exclude=Q[w:w + 1], Q=Q, radius=rad)
    assert k != w and (ex["best_idx"], ex["best_val"]) == (k, v)
    # everything excluded: -1;  index_base is added
    assert sweepConstrained(GPo, cons, Q, exclude=[[.5, .5]], exclude_radius=10.0, **kw)["best_idx"] == -1
    assert sweepConstrained(GPo, cons, Q, index_base=(1 << 33) + 5, **kw)["best_idx"] == (1 << 33) + 5 + w
    # thresholds so far out that every Phi underflows: 0.0 at the first candidate that is not excluded, a finite (zero) gradient
    far = [Constraint(cs[0][0], upper=-1e6), Constraint(cs[1][0], lower=1e6)]
    z = sweepConstrained(GPo, far, Q, exclude=Q[:3], exclude_radius=1e-9, outputs=("val",), **kw)
    assert np.all(z["val"] == 0.0) and z["best_val"] == 0.0 and z["best_idx"] == 3
    for native in (0, 1):
        rc, g = raw_batch(lib, GPo._handle(), [(cs[0][0]._handle(), -1e6, 1), (cs[1][0]._handle(), 1e6, -1)], Q[:9], 0, .01,
                          native, 1e-7, .6, grad=True)
        assert rc == 0 and np.all(g["val"] == 0.0) and np.all(g["dval"] == 0.0)


# ------------------------------------------------------------------------------------------------ the same handle twice
def test_same_handle_twice_and_handles_left_alone(lib):
    from ibo_amd import DeviceArray
    from ibo_amd.acquisition import sweep
    from ibo_amd.acquisition.constrained import Constraint, sweepConstrained
    X, Y = synth(51, 300, 3)
    Xc, _ = synth(52, 200, 3)
    GPo, mo = pair("ard", [.4, .5, .45], X, Y)
    GPc, mc = pair("m5", [.7, .9], Xc, np.cos(2 * Xc[:, 0]) - Xc[:, -1])
    Q = np.random.RandomState(53).rand(9001, 3)
    dc = DeviceArray.from_host(Q)
    probe = np.random.RandomState(54).rand(50, 3)
    before = [GP.posteriors(probe) for GP in (GPo, GPc)]
    # a kept incremental state on the objective, as a plain sweep leaves it
    kept = sweep(GPo, dc, acq='ei', incremental=True, outputs=("acq",))
    tiles, done = ctypes.c_int64(), ctypes.c_int64()
    lib.check(lib.lib.ibo_sweep_state_info(GPo._handle(), ctypes.byref(tiles), ctypes.byref(done)))
    state = (tiles.value, done.value)
    assert state[0] == (9001 + 31) // 32
    plain = sweep(GPo, dc, acq='ei', outputs=("acq",))            # what a plain sweep does to it: nothing
    lib.check(lib.lib.ibo_sweep_state_info(GPo._handle(), ctypes.byref(tiles), ctypes.byref(done)))
    assert (tiles.value, done.value) == state
    # the objective as its own constraint, and one constraint model twice as a band
    cons = [Constraint(GPo, lower=-.2), Constraint(GPc, upper=.3), Constraint(GPc, lower=-.5)]
    r = sweepConstrained(GPo, cons, dc, acq='ei', xi=.01, ymax=.7, outputs=("acq", "pof", "val"))
    rows = rows_to_check(9001, 150)
    rc = [ref_con(GPo, mo, -.2, -1, True), ref_con(GPc, mc, .3, 1, True), ref_con(GPc, mc, -.5, -1, True)]
    ref = cr.value(mo, rc, Q[rows], gr.ACQ_EI, .01, gr.ERF_LIBM, 1e-8, .7)
    ref_close(r["val"][rows], ref["val"]); ref_close(r["pof"][rows], ref["pof"])
    assert np.ptp(ref["pof"]) > .3
    pm = [sweep(GPo, dc, acq='ei', xi=.01, ymax=.7, outputs=("mu", "s2", "acq")), sweep(GPc, dc, outputs=("mu", "s2"))]
    own_close(r["val"], compose(pm, [(0, -.2, -1), (1, .3, 1), (1, -.5, -1)])[0])
    # host batches and gradients with the repeated handles
    rcb, b = raw_batch(lib, GPo._handle(), [(GPo._handle(), -.2, -1), (GPc._handle(), .3, 1), (GPc._handle(), -.5, -1)], Q[:200],
                       0, .01, 0, 1e-8, .7)
    assert rcb == 0
    # (the sweep above ran with libego's k* variance, 0.81 for this Matern-5/2 model as well: sf2_native = sf2_py there)
    ref_close(b["val"], cr.value(mo, rc, Q[:200], gr.ACQ_EI, .01, gr.ERF_LIBM, 1e-8, .7)["val"])
    # afterwards: the same posteriors, bit for bit, and the kept state as it was
    after = [GP.posteriors(probe) for GP in (GPo, GPc)]
    for (m0, s0), (m1, s1) in zip(before, after):
        assert np.array_equal(m0, m1) and np.array_equal(s0, s1)
    lib.check(lib.lib.ibo_sweep_state_info(GPo._handle(), ctypes.byref(tiles), ctypes.byref(done)))
    assert (tiles.value, done.value) == state
    again = sweep(GPo, dc, acq='ei', incremental=True, outputs=("acq",))
    assert again["kernel"] == "acq_finish_kernel" and np.array_equal(again["acq"], kept["acq"])


# ------------------------------------------------------------------------------------------------ a preference GP as the objective
def test_preference_objective_with_a_measured_constraint(lib):
    from ibo_amd import DeviceArray
    from ibo_amd.gaussianprocess import PrefGaussianProcess
    from ibo_amd.acquisition import sweep
    from ibo_amd.acquisition.constrained import Constraint, sweepConstrained, feasibleIncumbent
    rs = np.random.RandomState(61)
    pts = rs.rand(16, 2)
    f = lambda x: -np.sum((x - .4) ** 2)
    prefs = []
    for i in range(8):                                # 8 preferences, D = 2
        a, b = pts[2 * i], pts[2 * i + 1]
        prefs.append((a, b, 0) if f(a) > f(b) else (b, a, 0))
    GPp = PrefGaussianProcess(make_kernel("ard", [.4, .4]))
    GPp.addPreferences(prefs)
    Xc, _ = synth(62, 30, 2)
    GPc, _ = pair("m5", [.6, .9], Xc, Xc[:, 0] + Xc[:, 1])
    Q = rs.rand(2500, 2)
    dc = DeviceArray.from_host(Q)
    con = [Constraint(GPc, upper=.9)]
    ymax = feasibleIncumbent(GPp, con)
    assert ymax is not None
    r = sweepConstrained(GPp, con, dc, acq='ei', xi=.01, outputs=("acq", "pof", "val"))
    pm = [sweep(GPp, dc, acq='ei', xi=.01, ymax=ymax, outputs=("mu", "s2", "acq")), sweep(GPc, dc, outputs=("mu", "s2"))]
    val, pof = compose(pm, [(1, .9, 1)])
    assert np.array_equal(r["acq"], pm[0]["acq"])
    own_close(r["val"], val); own_close(r["pof"], pof)
    assert r["best_idx"] == int(np.argmax(r["val"])) and np.ptp(pof) > .5 and r["best_val"] > 0


# ------------------------------------------------------------------------------------------------ host batches and gradients
HYPER = {"ard": None, "iso": [.45], "svard": None, "sviso": [.45, .8], "m3": [.5, .95], "m5": [.5, .9]}


def hyper_of(kind, D):
    f = max(1.0, np.sqrt(D) / 2)
    ell = np.linspace(.35, .6, D) * f
    if kind == "ard":
        return list(ell)
    if kind == "svard":
        return list(ell) + [.9]
    return [h * (f if i == 0 else 1.0) for i, h in enumerate(HYPER[kind])]


def clip_model(D):
    """six well separated observations with noise 1e-9: a query on one of them has its variance clipped"""
    rs = np.random.RandomState(70 + D)
    X = (np.arange(6)[:, None] / 6.0 + .1 * rs.rand(6, D)) % 1.0
    return pair("iso", [.3 * max(1.0, np.sqrt(D) / 2)], X, np.sin(5 * X[:, 0]), noise=1e-9)


@pytest.mark.parametrize("kind,D,ncon,M,acq,erf_mode", [("ard", 1, 1, 1, 0, 1), ("iso", 3, 3, 7, 0, 0), ("sviso", 8, 1, 129, 1, 1),
                                                          ("m3", 3, 3, 5000, 0, 1), ("m5", 8, 3, 129, 1, 0), ("svard", 1, 3, 7, 3, 1),
                                                          ("m5", 3, 1, 5000, 3, 0)])
def test_batch_and_gradient(lib, kind, D, ncon, M, acq, erf_mode):
    """ibo_cacq_batch and ibo_cacq_grad_batch against the restatement, every kernel family, D in {1, 3, 8}, one and three
    constraints; with three, the third is a noise-1e-9 model and query 0 sits on one of its observations (clip active,
    dsigma = 0 there)"""
    Xo, Yo = synth(81, 60, D)
    Xc, _ = synth(82, 45, D)
    GPo, mo = pair(kind, hyper_of(kind, D), Xo, Yo, prior=make_prior(D) if D == 3 else None)
    GPa, ma = pair("m5" if kind != "m5" else "ard", hyper_of("m5" if kind != "m5" else "ard", D), Xc, np.cos(2 * Xc[:, 0]) - Xc[:, -1])
    GPo._push_prior()
    clamp = 1e-7
    cons, rcons = [(GPa._handle(), .2, 1)], [ref_con(GPa, ma, .2, 1, False)]
    Q = np.random.RandomState(83).rand(M, D) * 1.1 - .05
    if ncon == 3:
        GPk, mk = clip_model(D)
        tk = float(GPk.Y[2]) + 2e-4                   # sigma = sqrt(clamp) = 3.2e-4 on the observation: z = 0.6 there, Phi and phi alive
        cons += [(GPa._handle(), -.7, -1), (GPk._handle(), tk, 1)]
        rcons += [ref_con(GPa, ma, -.7, -1, False), ref_con(GPk, mk, tk, 1, False)]
        Q[0] = GPk.X[2]
        mu, s2 = np.empty(1), np.empty(1)
        lib.check(lib.lib.ibo_acq_batch(GPk._handle(), 1, lib.dp(lib.f64(Q[:1])), 3, 0.0, erf_mode, clamp, NAN, lib.dp(mu), lib.dp(s2), None))
        assert s2[0] == clamp
    ymax = float(np.max(Yo)) - .3
    rcb, b = raw_batch(lib, GPo._handle(), cons, Q, acq, .01, erf_mode, clamp, ymax)
    rcg, g = raw_batch(lib, GPo._handle(), cons, Q, acq, .01, erf_mode, clamp, ymax, grad=True)
    assert rcb == 0 and rcg == 0
    assert np.array_equal(g["val"], b["val"])                    # bit for bit
    rows = rows_to_check(M, 48)
    ref = cr.value(mo, rcons, Q[rows], acq, .01, erf_mode, clamp, ymax)
    for k in ("acq", "pof", "val"):
        ref_close(b[k][rows], ref[k])
    rg = cr.value_grad(mo, rcons, Q[rows], acq, .01, erf_mode, clamp, ymax)
    gr.assert_grad_close(g["dval"][rows], rg["dval"], rg["sval"], what="%s D=%d ncon=%d M=%d" % (kind, D, ncon, M))
    assert np.all(np.isfinite(g["dval"])) and np.max(np.abs(rg["dval"])) > 1e-6
    if ncon == 3:
        assert b["pof"][0] > 1e-3 and np.max(np.abs(rg["dval"][0])) > 0       # the clipped point takes part
    if acq != 3:                                     # the objective's factor is ibo_acq_batch's number
        a = np.empty(M)
        lib.check(lib.lib.ibo_acq_batch(GPo._handle(), M, lib.dp(lib.f64(Q)), acq, .01, erf_mode, clamp, ymax, None, None, lib.dp(a)))
        assert np.array_equal(a, b["acq"])
    else:
        assert np.all(b["acq"] == 1.0)


def test_classes_follow_the_python_conventions(lib, small_models):
    from ibo_amd.acquisition.constrained import Constraint, ConstrainedEI, ConstrainedPI, ProbFeasible, feasibleIncumbent
    sm = small_models
    (GPo, mo), cs = sm["obj"], sm["c"]
    cons = [Constraint(cs[0][0], upper=.35), Constraint(cs[1][0], lower=.12)]
    rcons = [ref_con(cs[0][0], cs[0][1], .35, 1, False), ref_con(cs[1][0], cs[1][1], .12, -1, False)]
    ymax = feasibleIncumbent(GPo, cons)
    assert ymax == cr_incumbent(GPo, [(cs[0][0], .35, 1), (cs[1][0], .12, -1)]) and ymax <= np.max(GPo.Y)
    Q = sm["Q"][:40]
    for cls, acq in ((ConstrainedEI, gr.ACQ_EI), (ConstrainedPI, gr.ACQ_PI), (ProbFeasible, gr.ACQ_NONE)):
        o = cls(GPo, cons, xi=.01)
        ref = cr.value_grad(mo, rcons, Q, acq, .01, gr.ERF_NR, 1e-7, ymax)
        ref_close(o.values(Q), ref["val"])
        v, g = o.gradient(Q)
        assert np.array_equal(v, o.values(Q))
        gr.assert_grad_close(g, ref["dval"], ref["sval"], what=cls.__name__)
        assert o.f(Q[3]) == v[3] and o.negf(Q[3]) == -v[3]
        nv, ng = o.negf_grad(Q[3])
        assert nv == -v[3] and np.array_equal(ng, -g[3])
    # no feasible row: the incumbent is None and the classes evaluate the probability of feasibility
    none = [Constraint(cs[0][0], upper=-50.0)]
    assert feasibleIncumbent(GPo, none) is None
    assert ConstrainedEI(GPo, none).acq == 'pof'
    with pytest.raises(ValueError):
        Constraint(GPo)
    with pytest.raises(ValueError):
        Constraint(GPo, upper=1.0, lower=0.0)


# ------------------------------------------------------------------------------------------------ DIRECT
def test_direct_equals_the_host_tree_on_single_points(lib, small_models):
    """ibo_cacq_direct_max against ibo_direct_host driven by a Python callback on single-point -ibo_cacq_batch: D = 2, N = 40,
    maxiter = 15, compat on"""
    sm = small_models
    (GPo, mo), cs = sm["obj"], sm["c"]
    cons = [(cs[0][0]._handle(), .35, 1), (cs[1][0]._handle(), .12, -1)]
    n, con, th, se, keep = pack(lib, cons)
    lb, ub = lib.f64([0., 0.]), lib.f64([1., 1.])
    opt = ctypes.c_double(); optx = np.empty(2); ns = ctypes.c_int64()
    lib.check(lib.lib.ibo_cacq_direct_max(GPo._handle(), n, con, th, se, 2, lib.dp(lb), lib.dp(ub), 0, .01, 0, 1e-8, .6, 15, 30, 10000, 1,
                                          ctypes.byref(opt), lib.dp(optx), ctypes.byref(ns)))

    def negval(nd, x):
        q = np.array([x[i] for i in range(nd)])
        rc, b = raw_batch(lib, GPo._handle(), cons, q, 0, .01, 0, 1e-8, .6)
        assert rc == 0
        return -b["val"][0]
    cb = lib.OBJECTIVE(negval)
    fm = ctypes.c_double(); xm = np.empty(2); n2 = ctypes.c_int64()
    lib.check(lib.lib.ibo_direct_host(cb, 2, lib.dp(lb), lib.dp(ub), 15, 30, 10000, 1, ctypes.byref(fm), lib.dp(xm), ctypes.byref(n2)))
    assert ns.value == n2.value and ns.value > 50
    np.testing.assert_allclose(optx, xm, rtol=0, atol=1e-12)
    np.testing.assert_allclose(opt.value, -fm.value, rtol=0, atol=1e-12)
    assert opt.value > 1e-4


def test_maximizers(lib, small_models):
    from ibo_amd.acquisition.constrained import Constraint, maximizeCEI, maximizeCPI, sweepConstrained
    sm = small_models
    (GPo, mo), cs = sm["obj"], sm["c"]
    cons = [Constraint(cs[0][0], upper=.35), Constraint(cs[1][0], lower=.12)]
    bounds = [[0., 1.]] * 2
    v0, x0 = maximizeCEI(GPo, cons, bounds, maxiter=15)
    v1, x1 = maximizeCEI(GPo, cons, bounds, maxiter=15, polish=True)
    assert v1 >= v0 > 0 and np.all(x1 >= 0) and np.all(x1 <= 1)
    # the value at the returned point, from the restatement (libego's conventions)
    ymax = cr_incumbent(GPo, [(cs[0][0], .35, 1), (cs[1][0], .12, -1)])
    rcons = [ref_con(cs[0][0], cs[0][1], .35, 1, True), ref_con(cs[1][0], cs[1][1], .12, -1, True)]
    for v, x in ((v0, x0), (v1, x1)):
        ref_close(v, cr.value(mo, rcons, x, gr.ACQ_EI, .01, gr.ERF_LIBM, 1e-8, ymax)["val"][0])
    # DIRECT does at least as well as a coarse sweep of the same objective
    s = sweepConstrained(GPo, cons, sm["Q"][:200], acq='ei')
    assert v1 >= s["best_val"] * .5
    vp, xp = maximizeCPI(GPo, cons, bounds, maxiter=10)
    ref_close(vp, cr.value(mo, rcons, xp, gr.ACQ_PI, .01, gr.ERF_LIBM, 1e-8, ymax)["val"][0])
    # no feasible row: the probability of feasibility is maximised
    t = float(np.min(cs[0][0]._posterior_arrays(GPo.X)[0])) - .05     # just below every row's mean: none feasible, P alive
    none = [Constraint(cs[0][0], upper=t)]
    vf, xf = maximizeCEI(GPo, none, bounds, maxiter=10)
    ref_close(vf, cr.value(mo, [ref_con(cs[0][0], cs[0][1], t, 1, True)], xf, gr.ACQ_NONE, 0.0, gr.ERF_LIBM, 1e-8)["val"][0])
    assert vf > .1
    assert sweepConstrained(GPo, none, sm["Q"][:50])["acq_used"] == 'pof'


# ------------------------------------------------------------------------------------------------ errors
def test_errors(lib, small_models):
    from ibo_amd.gaussianprocess import _DeviceGP
    sm = small_models
    (GPo, mo), cs = sm["obj"], sm["c"]
    ho, hc = GPo._handle(), cs[0][0]._handle()
    Q = sm["Q"][:4]
    dc = sm["dc"].view_rows(0, 4)
    X3, Y3 = synth(91, 20, 3)
    GP3, _ = pair("iso", [.4], X3, Y3)
    fresh = _DeviceGP()
    cases = [([(GP3._handle(), .1, 1)], 0, 0, lib.ERR_ARG),          # a D mismatch
             ([(fresh.h, .1, 1)], 0, 0, lib.ERR_STATE),              # an unfitted constraint
             ([(hc, .1, 1)], 2, 0, lib.ERR_ARG),                     # UCB
             ([(hc, .1, 0)], 0, 0, lib.ERR_ARG),                     # a sense of 0
             ([(hc, NAN, 1)], 0, 0, lib.ERR_ARG),                    # a NaN threshold
             ([(hc, float("inf"), 1)], 0, 0, lib.ERR_ARG),
             ([(hc, .1, 1)], 7, 0, lib.ERR_ARG), ([(hc, .1, 1)], 0, 5, lib.ERR_ARG)]
    for cons, acq, erf_mode, want in cases:
        assert raw_batch(lib, ho, cons, Q, acq, .01, erf_mode)[0] == want
        assert raw_batch(lib, ho, cons, Q, acq, .01, erf_mode, grad=True)[0] == want
        assert raw_sweep(lib, ho, cons, dc, acq, .01, erf_mode)[0] == want
        n, con, th, se, keep = pack(lib, cons)
        lb, ub = lib.f64([0., 0.]), lib.f64([1., 1.])
        opt = ctypes.c_double()
        assert lib.lib.ibo_cacq_direct_max(ho, n, con, th, se, 2, lib.dp(lb), lib.dp(ub), acq, .01, erf_mode, 1e-8, NAN, 3, 5, 100, 1,
                                           ctypes.byref(opt), None, None) == want
    n, con, th, se, keep = pack(lib, [(hc, .1, 1)])
    out = np.empty(4)
    L = lib.lib
    assert L.ibo_cacq_batch(None, n, con, th, se, 4, lib.dp(lib.f64(Q)), 0, .01, 0, 1e-8, NAN, None, None, lib.dp(out)) == lib.ERR_ARG
    assert L.ibo_cacq_batch(ho, n, con, th, se, 4, lib.dp(lib.f64(Q)), 0, .01, 0, 1e-8, NAN, None, None, None) == lib.ERR_ARG
    assert L.ibo_cacq_batch(ho, n, con, th, se, 0, lib.dp(lib.f64(Q)), 0, .01, 0, 1e-8, NAN, None, None, lib.dp(out)) == lib.ERR_ARG
    assert L.ibo_cacq_batch(ho, 1, None, th, se, 4, lib.dp(lib.f64(Q)), 0, .01, 0, 1e-8, NAN, None, None, lib.dp(out)) == lib.ERR_ARG
    assert L.ibo_cacq_batch(ho, -1, con, th, se, 4, lib.dp(lib.f64(Q)), 0, .01, 0, 1e-8, NAN, None, None, lib.dp(out)) == lib.ERR_ARG
    assert L.ibo_cacq_batch(ho, n, con, th, se, 4, lib.dp(lib.f64(Q)), 0, .01, 0, 1e-8, NAN, None, None, lib.dp(out)) == lib.OK
    fresh.close()

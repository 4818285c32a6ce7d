"""
Acquisitions integrated over an ensemble of models on the device (include/ibo_abi_ensemble.h: ibo_iacq_sweep, _batch, _grad_batch, _direct_max)
and the Python layer on top of them (gaussianprocess.ensemble, gaussianprocess.hypersample, acquisition.integrated).

The yardstick is tests/marginal_reference.py (pinned on the CPU by tests/test_marginal_reference.py).  Bars, the project's for the constrained
acquisition, EHVI and MES:
    composition   val / mean / var against the restatement on the library's OWN per-member ibo_acq_batch outputs: 1e-12 of sum_s w_s |a_s|,
                  of the mean's and the variance's terms
    end to end    against the NumPy restatement from the data on: 1e-6 of the terms' magnitudes, a posterior off by 1e-6 of its own terms
                  carried through the value's partial derivatives (assert_end_to_end of the MES test)
    gradients     1e-9 of sum_s w_s |dacq_s| against the restatement on the library's own per-member gradients; central differences of
                  ibo_iacq_batch (libm erf) at 1e-6 of (the gradient's scale + the value's), the bar of the MES test
and bit equality wherever the header promises it.  Shapes: N in {70, 130}, D in {3, 5}, S in {1, 2, 5, 32}, M in {1, 65, 130, 600, 1000, 4097},
members of the four kernel families in turn.  Every test prints what it measured before it asserts.
"""
import ctypes
import warnings

import numpy as np
import pytest

import cacq_reference as cr
import marginal_reference as mr

pytestmark = pytest.mark.gpu

NAN = float("nan")
GUARD = 7.25
TINY = float(np.finfo(float).tiny)
SHAPES = ((70, 3), (130, 5))
SS = (1, 2, 5, 32)
MS = (1, 65, 130, 600, 1000, 4097)
NOISE = .05
ACQS = ((mr.ACQ_EI, .01, mr.ERF_LIBM, 1e-8), (mr.ACQ_PI, .01, mr.ERF_NR, 1e-7), (mr.ACQ_UCB, 1.3, mr.ERF_LIBM, 1e-8), (mr.ACQ_NONE, 0.0, mr.ERF_LIBM, 1e-7))


@pytest.fixture(scope="module")
def lib():
    from ibo_amd import _lib
    if _lib.device_count() < 1:
        pytest.fail("no GPU visible: the product has no CPU fallback")
    return _lib


def make_kernel(kind, hyper):
    from ibo_amd.gaussianprocess import kernel as K
    return {"ard": K.GaussianKernel_ard, "iso": K.GaussianKernel_iso, "m3": K.MaternKernel3, "m5": K.MaternKernel5}[kind](np.array(hyper, dtype=float))


def member_spec(s, D, rs):
    """member s: the four families in turn, the length scales spread by a factor of about two around 0.3 sqrt(D)"""
    kind = ("ard", "iso", "m3", "m5")[s % 4]
    ell = .3 * np.sqrt(D) * np.exp(.35 * rs.randn(D if kind == "ard" else 1))
    return kind, list(ell) + ([.7 + .25 * rs.rand()] if kind in ("m3", "m5") else [])      # (the fit's diagonal is 1 + noise: a magnitude above 1 is not PD)


@pytest.fixture(scope="module")
def ens(lib):
    """per shape: the data, 32 member models (GaussianProcess objects and their restatements' recipes), 4097 candidates on the host and on
    the device, and weights -- made once, shared, to be left unchanged"""
    from ibo_amd import DeviceArray
    from ibo_amd.gaussianprocess import GaussianProcess
    out = {}
    for N, D in SHAPES:
        rs = np.random.RandomState(500 + N)
        X = rs.rand(N, D)
        Y = np.sin(3 * X.sum(1)) + .05 * rs.randn(N)
        specs = [member_spec(s, D, rs) for s in range(32)]
        gps = [GaussianProcess(make_kernel(k, h), X, Y, noise=NOISE) for k, h in specs]
        Q = rs.rand(4097, D) * 1.1 - .05
        Q.setflags(write=False)
        w = rs.rand(32) + .1
        out[(N, D)] = dict(N=N, D=D, X=X, Y=Y, specs=specs, gps=gps, Q=Q, dc=DeviceArray.from_host(Q), w=w)
    return out


def handles(gps):
    return (ctypes.c_void_p * len(gps))(*[g._handle() if g is not None else None for g in gps])


def set_chunk(lib, m):
    lib.check(lib.lib.ibo_set_option(b"iacq_chunk", int(m)))


def raw_sweep(lib, gps, w, dc, M, spec, ymax=NAN, exclude=None, radius=.5, base=0, want=("val", "mean", "var"), S=None):
    """(rc, dict of the outputs asked for, best_val, best_idx) of ibo_iacq_sweep over the first M rows of dc; outputs start from GUARD"""
    from ibo_amd import DeviceArray
    acq, parm, erf_mode, clamp = spec
    w = lib.f64(w)
    outs = {}
    for k in want:
        outs[k] = DeviceArray((M,))
        outs[k].upload(np.full(M, GUARD))
    ex = None if exclude is None else lib.f64(np.atleast_2d(exclude))
    bv = ctypes.c_double(-5.0); bi = ctypes.c_int64(-5)
    rc = lib.lib.ibo_iacq_sweep(handles(gps), len(gps) if S is None else S, lib.dp(w), M, dc.ptr, acq, parm, erf_mode, clamp, ymax,
                                0 if ex is None else len(ex), None if ex is None else lib.dp(ex), radius, base,
                                *[outs[k].ptr if k in outs else None for k in ("val", "mean", "var")], ctypes.byref(bv), ctypes.byref(bi))
    return rc, {k: v.to_host() for k, v in outs.items()}, bv.value, bi.value


def raw_batch(lib, gps, w, Q, spec, ymax=NAN, want=("val", "mean", "var"), S=None):
    """(rc, dict) of ibo_iacq_batch; outputs start from GUARD"""
    acq, parm, erf_mode, clamp = spec
    Q = lib.f64(np.atleast_2d(Q)); w = lib.f64(w)
    M = len(Q)
    outs = {k: np.full(M, GUARD) for k in want}
    rc = lib.lib.ibo_iacq_batch(handles(gps), len(gps) if S is None else S, lib.dp(w), M, lib.dp(Q), acq, parm, erf_mode, clamp, ymax,
                                *[lib.dp(outs[k]) if k in outs else None for k in ("val", "mean", "var")])
    return rc, outs


def raw_grad(lib, gps, w, Q, spec, ymax=NAN, S=None):
    acq, parm, erf_mode, clamp = spec
    Q = lib.f64(np.atleast_2d(Q)); w = lib.f64(w)
    val, g = np.full(len(Q), GUARD), np.full(Q.shape, GUARD)
    rc = lib.lib.ibo_iacq_grad_batch(handles(gps), len(gps) if S is None else S, lib.dp(w), len(Q), lib.dp(Q), acq, parm, erf_mode, clamp, ymax,
                                     lib.dp(val), lib.dp(g))
    return rc, val, g


def raw_direct(lib, gps, w, D, spec, ymax=NAN, maxiter=10, S=None):
    acq, parm, erf_mode, clamp = spec
    w = lib.f64(w)
    lb, ub = lib.f64(np.zeros(D)), lib.f64(np.ones(D))
    opt = ctypes.c_double(GUARD); optx = np.full(D, GUARD); ns = ctypes.c_int64(-5)
    rc = lib.lib.ibo_iacq_direct_max(handles(gps), len(gps) if S is None else S, lib.dp(w), D, lib.dp(lb), lib.dp(ub), acq, parm, erf_mode, clamp,
                                     ymax, maxiter, 30, 10000, 1, ctypes.byref(opt), lib.dp(optx), ctypes.byref(ns))
    return rc, opt.value, optx, ns.value


def own_members(lib, gps, Q, spec, ymax, grad=False):
    """(mu, s2, a) (S, M) of ibo_acq_batch per member -- with grad the (S, M, D) dacq (ACQ_NONE: dmu) of ibo_acq_grad_batch too.
    Up to 128 points travel with points at the origin up to 160, as the integrated entries send them (ibo_abi_ensemble.h: a short launch
    runs in the size class of its chunk; ibo_acq_batch alone would take the fused small kernel, whose sums run in another order, and
    EI far below the incumbent turns a last-bit difference of mu into far more than 1e-12 of the value)"""
    acq, parm, erf_mode, clamp = spec
    Q = lib.f64(np.atleast_2d(Q))
    m_asked = len(Q)
    if not grad and m_asked <= 128:
        Q = lib.f64(np.r_[Q, np.zeros((160 - m_asked, Q.shape[1]))])
    M, D = Q.shape
    mu, s2, a, da = np.empty((len(gps), M)), np.empty((len(gps), M)), np.empty((len(gps), M)), np.empty((len(gps), M, D))
    for s, g in enumerate(gps):
        none = acq == mr.ACQ_NONE
        lib.check(lib.lib.ibo_acq_batch(g._handle(), M, lib.dp(Q), acq, parm, erf_mode, clamp, ymax, lib.dp(mu[s]), lib.dp(s2[s]), None if none else lib.dp(a[s])))
        if none:
            a[s] = mu[s]
        if grad:
            lib.check(lib.lib.ibo_acq_grad_batch(g._handle(), M, lib.dp(Q), acq, parm, erf_mode, clamp, ymax, None, None, None,
                                                 lib.dp(da[s]) if none else None, None, None if none else lib.dp(da[s])))
    return (mu, s2, a, da) if grad else (mu[:, :m_asked], s2[:, :m_asked], a[:, :m_asked])


def pick(c, S):
    """S members of a shape (the first S: every family from S = 5 on) and their weights"""
    return c["gps"][:S], c["w"][:S].copy()


# ------------------------------------------------------------------------------------------------ composition
@pytest.mark.parametrize("S", SS)
@pytest.mark.parametrize("shape", SHAPES)
def test_composition_of_the_librarys_own_member_outputs(lib, ens, shape, S):
    c = ens[shape]
    gps, w = pick(c, S)
    ymax = float(np.max(c["Y"]))
    worst = {}
    for i, M in enumerate(MS):
        for spec in (ACQS if M in (65, 1000) else (ACQS[i % 4],)):
            Q = c["Q"][:M]
            rc, out = raw_batch(lib, gps, w, Q, spec)
            assert rc == 0, lib.lib.ibo_last_error()
            mu, s2, a = own_members(lib, gps, Q, spec, ymax)
            r = mr.combine(w, mu, s2, a)
            for k, sk in (("val", "sval"), ("mean", "smean"), ("var", "svar")):
                ratio = float(np.max(np.abs(out[k] - r[k]) / (1e-12 * r[sk] + TINY)))
                worst[k] = max(worst.get(k, 0.0), ratio)
                assert np.all(np.abs(out[k] - r[k]) <= 1e-12 * r[sk] + TINY), (k, M, spec, ratio)
            assert np.all(out["var"] > 0)
    print("composition N=%d D=%d S=%d: worst error / bar %s" % (shape + (S, worst)))


@pytest.mark.parametrize("shape,S,M", [((70, 3), 5, 600), ((130, 5), 2, 130), ((70, 3), 32, 65)])
def test_end_to_end_against_the_numpy_restatement(lib, ens, shape, S, M):
    c = ens[shape]
    gps, w = pick(c, S)
    ymax = float(np.max(c["Y"]))
    Q = c["Q"][:M]
    models = [cr.make(c["X"], c["Y"], NOISE, k, h) for k, h in c["specs"][:S]]
    for spec in ACQS:
        acq, parm, erf_mode, clamp = spec
        post = [cr.posterior(m, Q, clamp) for m in models]
        mu, s2 = np.array([p[0] for p in post]), np.array([p[1] for p in post])
        a, a_mu, a_sig = mr.acq_members(acq, erf_mode, mu, s2, ymax, parm)
        r = mr.combine(w, mu, s2, a)
        rc, out = raw_batch(lib, gps, w, Q, spec)
        assert rc == 0
        # The bar of the MES and constrained tests: 1e-6 of the terms, plus what a posterior off by 1e-6 of ITS terms -- mu by
        # 1e-6 |mu| + 1e-9, sigma by 1e-6 s2 / (2 sigma) -- moves the value by, through the value's own partial derivatives
        dmu = 1e-6 * np.abs(mu) + 1e-9
        dsig = 1e-6 * s2 / (2.0 * np.sqrt(s2))
        sw = float(np.sum(w))
        dmean = sum(w[s] * dmu[s] for s in range(S)) / sw
        bars = dict(val=1e-6 * r["sval"] + sum(w[s] * (np.abs(a_mu[s]) * dmu[s] + np.abs(a_sig[s]) * dsig[s]) for s in range(S)),
                    mean=dmean,
                    var=1e-6 * r["svar"] + sum(w[s] * (1e-6 * s2[s] + 2 * np.abs(mu[s] - r["mean"]) * (dmu[s] + dmean)) for s in range(S)) / sw)
        for k in ("val", "mean", "var"):
            ratio = float(np.max(np.abs(out[k] - r[k]) / bars[k]))
            print("end to end N=%d D=%d S=%d M=%d acq=%d %s: worst error / bar %.3g" % (shape + (S, M, acq, k, ratio)))
            assert np.all(np.abs(out[k] - r[k]) <= bars[k]), (k, spec)


# ------------------------------------------------------------------------------------------------ gradients
@pytest.mark.parametrize("shape,S,M", [((70, 3), 1, 7), ((70, 3), 5, 65), ((130, 5), 2, 129), ((130, 5), 32, 7)])
def test_gradients_against_the_restatement_and_central_differences(lib, ens, shape, S, M):
    c = ens[shape]
    gps, w = pick(c, S)
    if S > 2:
        w[1] = 0.0
    ymax = float(np.max(c["Y"]))
    Q = np.array(c["Q"][:M])
    D = Q.shape[1]
    for spec in ACQS:
        rc, val, g = raw_grad(lib, gps, w, Q, spec)
        assert rc == 0
        rcb, b = raw_batch(lib, gps, w, Q, spec, want=("val",))
        assert rcb == 0 and val.tobytes() == b["val"].tobytes()          # the gradient entry's value is the batch's, bit for bit
        mu, s2, a, da = own_members(lib, gps, Q, spec, ymax, grad=True)
        dval, sdval = mr.combine_grad(w, da)
        ratio = float(np.max(np.abs(g - dval) / (1e-9 * sdval + TINY)))
        print("gradient N=%d D=%d S=%d M=%d acq=%d: worst error / bar %.3g" % (shape + (S, M, spec[0], ratio)))
        assert np.all(np.abs(g - dval) <= 1e-9 * sdval + TINY) and np.all(np.isfinite(g)) and np.max(np.abs(g)) > 0
        if M > 7:
            continue
        # Central differences of ibo_iacq_batch, with libm's erf: the NR flavour's analytic gradient is documented to differ from the
        # derivative of its values by about 1e-6 relative (ibo_abi.h, ibo_acq_grad_batch: the truncated constants), which is this bar.
        # h = 1e-6: the h^2 / 6 term and the rounding of the two values, 2^-52 |val| / h = 2e-10 |val|, both stay far below it
        fspec = (spec[0], spec[1], mr.ERF_LIBM, spec[3])
        rc, fval, fg = raw_grad(lib, gps, w, Q, fspec)
        fmu, fs2, fa, fda = own_members(lib, gps, Q, fspec, ymax, grad=True)
        fsd = mr.combine_grad(w, fda)[1]
        sval = mr.combine(w, fmu, fs2, fa)["sval"]
        d = 1e-6
        for j in range(D):
            e = np.zeros(D); e[j] = d
            rcp, vp = raw_batch(lib, gps, w, Q + e, fspec, want=("val",))
            rcm, vm = raw_batch(lib, gps, w, Q - e, fspec, want=("val",))
            assert rc == 0 and rcp == 0 and rcm == 0
            fd = (vp["val"] - vm["val"]) / (2 * d)
            bar = 1e-6 * (fsd[:, j] + sval + 1.0)
            print("central differences acq=%d coordinate %d: worst / bar = %.3g" % (spec[0], j, float(np.max(np.abs(fd - fg[:, j]) / bar))))
            assert np.all(np.abs(fd - fg[:, j]) <= bar)
    # either output alone
    acq, parm, erf_mode, clamp = ACQS[0]
    Qc, wc = lib.f64(Q), lib.f64(w)
    lead = (handles(gps), S, lib.dp(wc), M, lib.dp(Qc), acq, parm, erf_mode, clamp, NAN)
    rc, val, g = raw_grad(lib, gps, w, Q, ACQS[0])
    v2, g2 = np.full(M, GUARD), np.full(Q.shape, GUARD)
    assert lib.lib.ibo_iacq_grad_batch(*(lead + (lib.dp(v2), None))) == 0 and lib.lib.ibo_iacq_grad_batch(*(lead + (None, lib.dp(g2)))) == 0
    assert v2.tobytes() == val.tobytes() and g2.tobytes() == g.tobytes()


# ------------------------------------------------------------------------------------------------ bit equalities
@pytest.mark.parametrize("shape", SHAPES)
def test_one_member_of_weight_one_is_the_plain_sweep_bit_for_bit(lib, ens, shape):
    """M = 130, 1000 and 4097: no launch is padded there.  And the same handle twice with weights 1/2, 1/2."""
    from ibo_amd import DeviceArray
    c = ens[shape]
    for k, spec in enumerate(ACQS[:3]):
        g = c["gps"][k]                              # (an ARD, an isotropic and a Matern member)
        acq, parm, erf_mode, clamp = spec
        for M in (130, 1000, 4097):
            a = DeviceArray((M,)); a.upload(np.full(M, GUARD))
            bv = ctypes.c_double(); bi = ctypes.c_int64()
            lib.check(lib.lib.ibo_acq_sweep(g._handle(), M, c["dc"].ptr, acq, parm, erf_mode, clamp, NAN, 0, None, .5, 0, None, None, a.ptr,
                                            ctypes.byref(bv), ctypes.byref(bi)))
            plain = a.to_host()
            rc, out, v1, i1 = raw_sweep(lib, [g], [1.0], c["dc"], M, spec, want=("val", "mean"))
            assert rc == 0 and out["val"].tobytes() == plain.tobytes() and (v1, i1) == (bv.value, bi.value), (spec, M)
            rc, two, v2, i2 = raw_sweep(lib, [g, g], [.5, .5], c["dc"], M, spec, want=("val", "mean", "var"))
            assert rc == 0 and two["val"].tobytes() == plain.tobytes() and (v2, i2) == (v1, i1), (spec, M)
            assert two["mean"].tobytes() == out["mean"].tobytes()


@pytest.mark.parametrize("shape,S", [((70, 3), 5), ((130, 5), 2), ((130, 5), 32)])
def test_sweep_batch_and_direct_agree_bit_for_bit(lib, ens, shape, S):
    c = ens[shape]
    gps, w = pick(c, S)
    spec = ACQS[0]
    kept = {}
    try:
        for chunk in (256, 0):
            set_chunk(lib, chunk)
            for M in (1, 65, 130, 600, 4097):
                rc, sw, bv, bi = raw_sweep(lib, gps, w, c["dc"], M, spec)
                rcb, b = raw_batch(lib, gps, w, c["Q"][:M], spec)
                rcg, gv, _ = raw_grad(lib, gps, w, c["Q"][:M], spec) if M <= 130 else (0, b["val"], None)
                assert rc == 0 and rcb == 0 and rcg == 0
                for k in ("val", "mean", "var"):
                    assert sw[k].tobytes() == b[k].tobytes(), (chunk, M, k)
                assert gv.tobytes() == b["val"].tobytes()
                assert (bi, bv) == cr.argmax(sw["val"])
                kept[(chunk, M)] = sw["val"]
            # DIRECT's value at its point is the batch's there
            rc, opt, optx, ns = raw_direct(lib, gps, w, shape[1], spec, maxiter=4)
            rcb, b = raw_batch(lib, gps, w, optx, spec, want=("val",))
            assert rc == 0 and rcb == 0 and opt == b["val"][0] and ns > 10, (chunk, opt, b["val"][0])
    finally:
        set_chunk(lib, 0)
    # within the small size class the chunk does not matter either; 4097 candidates in one launch are the other class: to rounding
    for M in (1, 65, 130, 600):
        assert kept[(256, M)].tobytes() == kept[(0, M)].tobytes(), M
    assert np.allclose(kept[(256, 4097)], kept[(0, 4097)], rtol=1e-9, atol=1e-12)
    assert kept[(0, 600)][:65].tobytes() == kept[(0, 65)].tobytes()


def test_a_member_without_weight_changes_no_bit(lib, ens):
    """a member fitted to NaN targets, weight 0, in the middle and at the end of the list: neither swept nor read"""
    from ibo_amd.gaussianprocess import GaussianProcess
    c = ens[(70, 3)]
    gps, w = pick(c, 5)
    ymax = float(np.max(c["Y"]))
    bad = GaussianProcess(make_kernel("ard", [.4, .5, .6]), c["X"], np.full(len(c["Y"]), NAN), noise=NOISE)
    mu = np.empty(3)
    lib.check(lib.lib.ibo_acq_batch(bad._handle(), 3, lib.dp(lib.f64(c["Q"][:3])), mr.ACQ_NONE, 0.0, 0, 1e-8, NAN, lib.dp(mu), None, None))
    assert np.all(np.isnan(mu)), "the member is meant to poison whatever reads it"
    for spec in ACQS:
        for M in (65, 600):
            rc, ref, bv, bi = raw_sweep(lib, gps, w, c["dc"], M, spec, ymax=ymax)
            for at in (1, 5):
                g2 = gps[:at] + [bad] + gps[at:]
                w2 = np.r_[w[:at], 0.0, w[at:]]
                rc2, out, bv2, bi2 = raw_sweep(lib, g2, w2, c["dc"], M, spec, ymax=ymax)
                assert rc == 0 and rc2 == 0 and (bv2, bi2) == (bv, bi)
                for k in ("val", "mean", "var"):
                    assert out[k].tobytes() == ref[k].tobytes(), (spec, M, at, k)
                rcg, v, g = raw_grad(lib, g2, w2, c["Q"][:7], spec, ymax=ymax)
                rcr, vr, gr_ = raw_grad(lib, gps, w, c["Q"][:7], spec, ymax=ymax)
                assert rcg == 0 and rcr == 0 and v.tobytes() == vr.tobytes() and g.tobytes() == gr_.tobytes()


# ------------------------------------------------------------------------------------------------ the arg-max contract
def test_argmax_contract(lib, ens):
    from ibo_amd import DeviceArray
    c = ens[(70, 3)]
    gps, w = pick(c, 5)
    spec, M = ACQS[0], 600
    Q = np.array(c["Q"][:M])
    try:
        set_chunk(lib, 256)
        rc, base, bv, win = raw_sweep(lib, gps, w, c["dc"], M, spec, want=("val",))
        base = base["val"]
        assert rc == 0 and (win, bv) == cr.argmax(base) and np.sum(base == bv) == 1
        low = Q[int(np.argmin(base))]
        for i in (255, 256, 511, 512):               # the winner at the last row of a chunk and the first of the next
            Q2 = Q.copy(); Q2[win] = low; Q2[i] = Q[win]
            rc, v, bv2, bi2 = raw_sweep(lib, gps, w, DeviceArray.from_host(Q2), M, spec, want=("val",))
            assert rc == 0 and v["val"][i] == bv and (bi2, bv2) == (i, bv), i
        for i, j in ((255, 256), (256, 511), (511, 512), (300, 599)):      # the winner twice: the first index
            Q2 = Q.copy(); Q2[win] = low; Q2[i] = Q[win]; Q2[j] = Q[win]
            rc, v, bv2, bi2 = raw_sweep(lib, gps, w, DeviceArray.from_host(Q2), M, spec, want=("val",))
            assert rc == 0 and v["val"][i] == bv and v["val"][j] == bv and (bi2, bv2) == (i, bv), (i, j)
        for pos in (0, win, 256, 599):               # a NaN coordinate: a NaN value that never wins
            Q3 = Q.copy(); Q3[pos, 1] = NAN
            rc, v, bv3, bi3 = raw_sweep(lib, gps, w, DeviceArray.from_host(Q3), M, spec)
            assert rc == 0 and np.isnan(v["val"][pos]) and np.sum(np.isnan(v["val"])) == 1 and np.isnan(v["mean"][pos])
            assert (bi3, bv3) == cr.argmax(v["val"]) and bi3 != pos
        rc, v, bvn, bin_ = raw_sweep(lib, gps, w, DeviceArray.from_host(np.full((3, 3), NAN)), 3, spec, want=("val",))
        assert rc == 0 and np.all(np.isnan(v["val"])) and (bin_, bvn) == (-1, -np.inf)
        rc, v, bve, bie = raw_sweep(lib, gps, w, c["dc"], M, spec, exclude=Q[win:win + 1], radius=1e-3, want=("val",))
        assert rc == 0 and np.array_equal(v["val"], base) and (bie, bve) == cr.argmax(base, exclude=Q[win:win + 1], Q=Q, radius=1e-3) and bie != win
        rc, _, bva, bia = raw_sweep(lib, gps, w, c["dc"], M, spec, exclude=[[.5, .5, .5]], radius=10.0, want=("val",))
        assert rc == 0 and (bia, bva) == (-1, -np.inf)
        rc, _, bvb, bib = raw_sweep(lib, gps, w, c["dc"], M, spec, base=(1 << 33) + 5, want=())
        assert rc == 0 and (bib, bvb) == ((1 << 33) + 5 + win, bv)
    finally:
        set_chunk(lib, 0)


# ------------------------------------------------------------------------------------------------ DIRECT
def test_direct_on_the_device_is_the_host_driver_on_the_batch(lib):
    from ibo_amd.gaussianprocess import GaussianProcess
    rs = np.random.RandomState(77)
    X = rs.rand(40, 2)
    Y = np.sin(3 * X.sum(1)) + .05 * rs.randn(40)
    gps = [GaussianProcess(make_kernel(k, h), X, Y, noise=NOISE) for k, h in (("ard", [.3, .5]), ("iso", [.4]), ("m5", [.5, .9]))]
    w = [.5, .2, .3]
    spec = ACQS[0]
    rc, opt, optx, ns = raw_direct(lib, gps, w, 2, spec, maxiter=10)
    assert rc == 0

    def negval(nd, x):
        rcb, b = raw_batch(lib, gps, w, [x[i] for i in range(nd)], spec, want=("val",))
        assert rcb == 0
        return -b["val"][0]
    cb = lib.OBJECTIVE(negval)
    lb, ub = lib.f64(np.zeros(2)), lib.f64(np.ones(2))
    fm = ctypes.c_double(); xm = np.empty(2); n2 = ctypes.c_int64()
    lib.check(lib.lib.ibo_direct_host(cb, 2, lib.dp(lb), lib.dp(ub), 10, 30, 10000, 1, ctypes.byref(fm), lib.dp(xm), ctypes.byref(n2)))
    assert ns == n2.value and ns > 30
    assert np.array_equal(optx, xm) and opt == -fm.value and opt > 0


# ------------------------------------------------------------------------------------------------ errors
def test_argument_errors_leave_the_outputs_alone(lib, ens):
    from ibo_amd.gaussianprocess import GaussianProcess, _DeviceGP
    c, c5 = ens[(70, 3)], ens[(130, 5)]
    gps, w = pick(c, 3)
    spec = ACQS[0]
    ARG, STATE = lib.ERR_ARG, lib.ERR_STATE
    fresh = _DeviceGP()

    class Raw(object):                               # (a bare handle where the helpers expect a model)
        def __init__(self, h):
            self.h = h

        def _handle(self):
            return self.h

    def all_four(gps, w, S=None, D=3):
        """the four return codes; every output must still hold its guard"""
        rcs, M = [], 4
        rc, out, bv, bi = raw_sweep(lib, gps, w, c["dc"], M, spec, S=S)
        assert all(np.all(v == GUARD) for v in out.values()) and (bv, bi) == (-5.0, -5)
        rcs.append(rc)
        rc, out = raw_batch(lib, gps, w, c["Q"][:M], spec, S=S)
        assert all(np.all(v == GUARD) for v in out.values())
        rcs.append(rc)
        rc, v, g = raw_grad(lib, gps, w, c["Q"][:M], spec, S=S)
        assert np.all(v == GUARD) and np.all(g == GUARD)
        rcs.append(rc)
        rc, opt, optx, ns = raw_direct(lib, gps, w, D, spec, maxiter=3, S=S)
        assert opt == GUARD and np.all(optx == GUARD) and ns == -5
        rcs.append(rc)
        return rcs

    rc, out, _, _ = raw_sweep(lib, gps, w, c["dc"], 4, spec)
    assert rc == 0 and not np.any(out["val"] == GUARD)
    assert all_four(gps, w, S=0) == [ARG] * 4
    assert all_four(c["gps"] + [c["gps"][0]], np.ones(33), S=33) == [ARG] * 4
    assert all_four(gps, [.5, -.1, .5]) == [ARG] * 4
    assert all_four(gps, [.5, NAN, .5]) == [ARG] * 4
    assert all_four(gps, [.5, np.inf, .5]) == [ARG] * 4
    assert all_four(gps, [0., 0., 0.]) == [ARG] * 4
    assert all_four([gps[0], None, gps[2]], w) == [ARG] * 4
    assert all_four([gps[0], Raw(fresh.h), gps[2]], w) == [STATE] * 4
    assert all_four([gps[0], c5["gps"][0], gps[2]], w) == [ARG] * 4      # mixed D
    L = lib.lib
    wc, Qc = lib.f64(w), lib.f64(c["Q"][:4])
    lead = (handles(gps), 3, lib.dp(wc))
    tail = (spec[0], spec[1], spec[2], spec[3], NAN)
    lb, ub = lib.f64(np.zeros(3)), lib.f64(np.ones(3))
    opt = ctypes.c_double(GUARD)
    assert L.ibo_iacq_sweep(*(lead + (4, c["dc"].ptr) + tail + (0, None, .5, 0, None, None, None, None, None))) == ARG      # every output NULL
    assert L.ibo_iacq_batch(*(lead + (4, lib.dp(Qc)) + tail + (None, None, None))) == ARG
    assert L.ibo_iacq_grad_batch(*(lead + (4, lib.dp(Qc)) + tail + (None, None))) == ARG
    assert L.ibo_iacq_direct_max(*(lead + (3, lib.dp(lb), lib.dp(ub)) + tail + (3, 5, 100, 1, None, None, None))) == ARG
    out = np.full(4, GUARD)
    assert L.ibo_iacq_batch(*(lead + (0, lib.dp(Qc)) + tail + (lib.dp(out), None, None))) == ARG
    assert L.ibo_iacq_batch(*(lead + (4, None) + tail + (lib.dp(out), None, None))) == ARG
    assert L.ibo_iacq_batch(*((None, 3, lib.dp(wc)) + (4, lib.dp(Qc)) + tail + (lib.dp(out), None, None))) == ARG
    assert L.ibo_iacq_batch(*((handles(gps), 3, None) + (4, lib.dp(Qc)) + tail + (lib.dp(out), None, None))) == ARG
    assert L.ibo_iacq_batch(*(lead + (4, lib.dp(Qc)) + (7, .01, 0, 1e-8, NAN) + (lib.dp(out), None, None))) == ARG
    assert L.ibo_iacq_batch(*(lead + (4, lib.dp(Qc)) + (0, .01, 2, 1e-8, NAN) + (lib.dp(out), None, None))) == ARG
    assert L.ibo_iacq_direct_max(*(lead + (2, lib.dp(lb), lib.dp(ub)) + tail + (3, 5, 100, 1, ctypes.byref(opt), None, None))) == ARG
    assert L.ibo_iacq_direct_max(*(lead + (3, None, lib.dp(ub)) + tail + (3, 5, 100, 1, ctypes.byref(opt), None, None))) == ARG
    assert np.all(out == GUARD) and opt.value == GUARD
    assert L.ibo_set_option(b"iacq_chunk", -1) == ARG
    fresh.close()


def test_stage_time_diagnostic(lib, ens):
    c = ens[(70, 3)]
    gps, w = pick(c, 5)
    ms = np.full(2, -1.0)
    rc, v0, _, _ = raw_sweep(lib, gps, w, c["dc"], 1000, ACQS[0])
    try:
        lib.check(lib.lib.ibo_set_option(b"iacq_timing", 1))
        lib.check(lib.lib.ibo_iacq_stage_ms(None, 1))
        rc1, v1, _, _ = raw_sweep(lib, gps, w, c["dc"], 1000, ACQS[0])
        lib.check(lib.lib.ibo_iacq_stage_ms(lib.dp(ms), 1))
    finally:
        lib.check(lib.lib.ibo_set_option(b"iacq_timing", 0))
    assert rc == 0 and rc1 == 0 and all(v0[k].tobytes() == v1[k].tobytes() for k in v0)
    assert np.all(ms > 0) and np.all(ms < 200.0), ms
    lib.check(lib.lib.ibo_iacq_stage_ms(lib.dp(ms), 0))
    assert np.all(ms == 0.0)


# ------------------------------------------------------------------------------------------------ the Python layer
def test_python_layer(lib, ens):
    from ibo_amd import DeviceArray
    from ibo_amd.gaussianprocess import GaussianProcess, PrefGaussianProcess, GaussianProcessEnsemble
    from ibo_amd.gaussianprocess.sparse import SparseGaussianProcess
    from ibo_amd.acquisition import (IntegratedEI, IntegratedPI, IntegratedUCB, sweepIntegrated, maximizeIntegratedEI, maximizeIntegratedPI,
                                     maximizeIntegratedUCB, EI, sweep)
    c = ens[(70, 3)]
    X, Y, D = c["X"], c["Y"], 3
    kernels = [make_kernel(k, h) for k, h in c["specs"][:4]]
    E = GaussianProcessEnsemble(kernels, X, Y, noise=NOISE, weights=[1, 2, 3, 2])
    assert len(E.members) == 4 and abs(E.weights.sum() - 1) < 1e-15 and E.X is E.members[0].X and np.array_equal(E.Y, Y)
    Q = np.array(c["Q"][:65])
    # the mixture posterior: ibo_iacq_batch with ACQ_NONE under the Python conventions
    rc, raw = raw_batch(lib, E.members, E.weights, Q, (mr.ACQ_NONE, 0.0, mr.ERF_NR, 1e-7))
    mean, var = E.posteriors(Q)
    assert rc == 0 and mean.tobytes() == raw["mean"].tobytes() and var.tobytes() == raw["var"].tobytes()
    m1, v1 = E.posterior(Q[0])
    mu_s = np.array([m.posteriors(Q[:1])[0][0] for m in E.members])
    assert abs(m1 - float(E.weights @ mu_s)) < 1e-12 * np.sum(np.abs(E.weights * mu_s)) + 1e-15 and v1 > 0 and E.mu(Q[0]) == m1
    # the classes
    ymax = float(np.max(Y))
    for cls, spec in ((IntegratedEI, (mr.ACQ_EI, .01, mr.ERF_NR, 1e-7)), (IntegratedPI, (mr.ACQ_PI, .01, mr.ERF_NR, 1e-7))):
        a = cls(E, xi=.01)
        rc, raw = raw_batch(lib, E.members, E.weights, Q, spec, ymax=ymax, want=("val",))
        assert a.values(Q).tobytes() == raw["val"].tobytes() and a.f(Q[3]) == a.values(Q)[3] and a.negf(Q[3]) == -a.f(Q[3])
        v, g = a.gradient(Q[:5])
        rcg, vr, gr_ = raw_grad(lib, E.members, E.weights, Q[:5], spec, ymax=ymax)
        assert v.tobytes() == vr.tobytes() and g.tobytes() == gr_.tobytes()
        nv, ng = a.negf_grad(Q[2])
        assert nv == -v[2] and np.array_equal(ng, -g[2])
    u = IntegratedUCB(E, D)
    assert np.all(np.isfinite(u.values(Q))) and u.gradient(Q[:2])[1].shape == (2, 3)
    one = GaussianProcessEnsemble(kernels[:1], X, Y, noise=NOISE)
    assert np.allclose(IntegratedEI(one).values(Q), EI(one.members[0]).values(Q), rtol=1e-9, atol=1e-15)      # (65 points: another size class, to rounding)
    # the sweep
    r = sweepIntegrated(E, c["dc"].view_rows(0, 1000), outputs=('val', 'mean', 'var'))
    r2 = sweepIntegrated(E, np.array(c["Q"][:1000]), outputs=('val',))
    assert r["best_idx"] == r2["best_idx"] and r["val"].tobytes() == r2["val"].tobytes() and (r["best_idx"], r["best_val"]) == cr.argmax(r["val"])
    s1 = sweep(one.members[0], c["dc"].view_rows(0, 1000), outputs=('acq',))
    r1 = sweepIntegrated(one, c["dc"].view_rows(0, 1000), outputs=('val',))
    assert r1["val"].tobytes() == s1["acq"].tobytes() and (r1["best_val"], r1["best_idx"]) == (s1["best_val"], s1["best_idx"])
    for acq in ('pi', 'ucb'):
        rr = sweepIntegrated(E, c["dc"].view_rows(0, 130), acq=acq, native=False, exclude=[Q[0]], exclude_radius=.2, index_base=7)
        assert rr["best_idx"] >= 7
    with pytest.raises(ValueError):
        sweepIntegrated(E, c["dc"].view_rows(0, 130), outputs=('acq',))
    # the maximisers: polish never returns less than DIRECT
    bounds = [[0., 1.]] * D
    for f in (maximizeIntegratedEI, maximizeIntegratedPI, maximizeIntegratedUCB):
        o, ox = f(E, bounds, maxiter=6)
        op, oxp = f(E, bounds, maxiter=6, polish=True)
        print("%s: DIRECT %.6g, polished %.6g" % (f.__name__, o, op))
        assert op >= o and np.all(oxp >= 0) and np.all(oxp <= 1) and np.isfinite(o)
    # addData: the ensemble grown in two steps is the ensemble built on all the data at once, bit for bit
    rs = np.random.RandomState(9)
    Xn, Yn = rs.rand(3, D), rs.randn(3)
    grown = GaussianProcessEnsemble(kernels, X, Y, noise=NOISE, weights=[1, 2, 3, 2])
    grown.addData(Xn[:1], Yn[:1])
    grown.addData(Xn[1:], Yn[1:])
    built = GaussianProcessEnsemble(kernels, np.r_[X, Xn], np.r_[Y, Yn], noise=NOISE, weights=[1, 2, 3, 2])
    a, b = IntegratedEI(grown).values(Q), IntegratedEI(built).values(Q)
    print("addData against a fresh ensemble: %d of %d values differ" % (np.sum(a != b), len(a)))
    assert len(grown.X) == len(X) + 3 and np.array_equal(grown.Y, np.r_[Y, Yn]) and a.tobytes() == b.tobytes()
    ga, gb = grown.posteriors(Q), built.posteriors(Q)
    assert ga[0].tobytes() == gb[0].tobytes() and ga[1].tobytes() == gb[1].tobytes()
    assert all(np.array_equal(m.L, f.L) for m, f in zip(grown.members, built.members))
    # a member whose fit fails leaves the whole ensemble as it was (the second member's fit is made to fail once)
    two = GaussianProcessEnsemble(kernels[:2], X, Y, noise=NOISE)
    before = IntegratedEI(two).values(Q)
    fit, failed = two.members[1]._fit_device, []

    def fails_once(*args, **kw):
        if not failed:
            failed.append(1)
            raise np.linalg.LinAlgError("made to fail")
        return fit(*args, **kw)
    two.members[1]._fit_device = fails_once
    with pytest.raises(np.linalg.LinAlgError):
        two.addData(Xn, Yn)
    assert len(two.X) == len(X) and all(len(m.X) == len(X) and len(m.Y) == len(X) for m in two.members)
    assert IntegratedEI(two).values(Q).tobytes() == before.tobytes()
    two.addData(Xn, Yn)
    assert IntegratedEI(two).values(Q).tobytes() == IntegratedEI(GaussianProcessEnsemble(kernels[:2], np.r_[X, Xn], np.r_[Y, Yn], noise=NOISE)).values(Q).tobytes()
    with pytest.raises(ValueError):
        grown.addData(np.zeros((2, D + 1)), [0., 0.])
    # the refusals
    for bad in (lambda: GaussianProcessEnsemble(kernels, X, Y, G=np.zeros_like(X)),
                lambda: GaussianProcessEnsemble.from_members([PrefGaussianProcess(kernels[0])]),
                lambda: GaussianProcessEnsemble.from_members([GaussianProcess(kernels[0], X, Y, G=np.zeros_like(X), noise=NOISE)]),
                lambda: GaussianProcessEnsemble.from_members([SparseGaussianProcess(kernels[0], X, Y, X[:10], noise=NOISE)]),
                lambda: E.addData(Xn, Yn, G=np.zeros_like(Xn))):
        with pytest.raises(NotImplementedError):
            bad()
    with pytest.raises(ValueError):
        GaussianProcessEnsemble([kernels[0]] * 33, X, Y)
    with pytest.raises(ValueError):
        GaussianProcessEnsemble(kernels, X, Y, weights=[1, -1, 1, 1])
    with pytest.raises(TypeError):
        IntegratedEI(E.members[0])


def test_refit_gives_the_bits_of_a_new_model(lib, ens):
    """GaussianProcess.refit, which the ensemble's addData is built on: after an in-place extension, and with other data given"""
    from ibo_amd.gaussianprocess import GaussianProcess, PrefGaussianProcess
    c = ens[(70, 3)]
    X, Y, Q = c["X"], c["Y"], np.array(c["Q"][:65])
    k = make_kernel(*c["specs"][0])
    rs = np.random.RandomState(9)
    Xn, Yn = rs.rand(3, 3), rs.randn(3)
    g = GaussianProcess(k, X, Y, noise=NOISE)
    g.addData(Xn, Yn)
    g.refit()
    fresh = GaussianProcess(k, np.r_[X, Xn], np.r_[Y, Yn], noise=NOISE)
    assert np.array_equal(g.L, fresh.L) and g.posteriors(Q)[0].tobytes() == fresh.posteriors(Q)[0].tobytes()
    g.refit(X, Y)
    small = GaussianProcess(k, X, Y, noise=NOISE)
    assert len(g.X) == 70 and np.array_equal(g.L, small.L) and g.posteriors(Q)[1].tobytes() == small.posteriors(Q)[1].tobytes()
    with pytest.raises(ValueError):
        g.refit(X)
    with pytest.raises(ValueError):
        g.refit(X, Y[:5])
    assert len(g.X) == 70 and g.posteriors(Q)[0].tobytes() == small.posteriors(Q)[0].tobytes()
    with pytest.raises(NotImplementedError):
        PrefGaussianProcess(k).refit()
    with pytest.raises(NotImplementedError):
        GaussianProcess(k, X[:10], Y[:10], G=np.zeros((10, 3)), noise=NOISE).refit()


# ------------------------------------------------------------------------------------------------ the sampler on the device
@pytest.fixture(scope="module")
def known(lib):
    """data drawn from a GP of known SE-ARD length scales, N = 40, D = 2; the sampler is started at a corner of the prior box"""
    rs = np.random.RandomState(21)
    X = rs.rand(40, 2)
    true = np.array([.25, .6])
    d = (X[:, None, :] - X[None, :, :]) / true
    K = np.exp(-.5 * np.sum(d * d, axis=2)) + 1e-3 * np.eye(40)
    Y = np.linalg.cholesky(K) @ rs.randn(40)
    return dict(X=X, Y=Y, true=np.log(true), lo=np.log(true) - 2.0, hi=np.log(true) + 2.0)


def test_sample_hyper_is_reproducible_and_its_logp_is_the_target(lib, known, oracle):
    import nlml_reference as nr
    from ibo_amd.gaussianprocess.hypersample import sampleHyper, BoxPrior, LogNormalPrior
    from ibo_amd.gaussianprocess.trainhyper import nlml_values
    X, Y = known["X"], known["Y"]
    prior = BoxPrior(known["lo"], known["hi"]) * LogNormalPrior(known["true"] + .3, 1.5)
    start = make_kernel("ard", np.exp(known["true"] + .5))
    a = sampleHyper(start, X, Y, n=12, chains=4, burn=5, thin=1, noise=1e-3, prior=prior, seed=3)
    b = sampleHyper(start, X, Y, n=12, chains=4, burn=5, thin=1, noise=1e-3, prior=prior, seed=3)
    assert a[0].shape == (12, 2) and a[1].shape == (12,)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
    other = sampleHyper(start, X, Y, n=12, chains=4, burn=5, thin=1, noise=1e-3, prior=prior, seed=4)
    assert other[0].tobytes() != a[0].tobytes()
    same, worst = 0, 0.0
    for phi, lp in zip(*a):
        k = make_kernel("ard", np.exp(phi))
        one = -nlml_values([k], X, Y, 1e-3)[0] + prior.logpdf([phi])[0]
        ref = nr.nlml(oracle.Kern("ard", np.exp(phi)), X, Y, 1e-3, 0, longdouble=False)
        bar = 2 * nr.bar_factor(ref["cond"]) * ref["V"]              # (twice the grid's bar: what test_gpu_nlml.py holds grid against single to)
        same += one == lp
        worst = max(worst, abs(one - lp) / bar)
        assert abs(one - lp) <= bar, (phi, lp, one, bar)
    print("sampleHyper logp against one theta at a time: %d of 12 bit-equal, worst difference / bar %.3g" % (same, worst))


def test_the_sample_mean_moves_from_the_corner_towards_the_true_length_scales(lib, known):
    from ibo_amd.gaussianprocess.hypersample import sampleHyper, BoxPrior
    X, Y = known["X"], known["Y"]
    corner = known["hi"] - .05                       # (just inside the box's upper corner: both length scales 7 times too long)
    phi, lp = sampleHyper(make_kernel("ard", np.exp(corner)), X, Y, n=32, chains=4, burn=20, thin=2, noise=1e-3,
                          prior=BoxPrior(known["lo"], known["hi"]), seed=0)
    mean = phi.mean(axis=0)
    print("true log theta %s, start %s, sample mean %s" % (known["true"], corner, mean))
    assert np.all(phi >= known["lo"]) and np.all(phi <= known["hi"]) and np.all(np.isfinite(lp))
    assert np.linalg.norm(mean - known["true"]) < np.linalg.norm(corner - known["true"])          # (nearer than the point it started from)


def test_an_ensemble_from_samples(lib, known):
    from ibo_amd.gaussianprocess import GaussianProcessEnsemble
    from ibo_amd.acquisition import IntegratedEI, maximizeIntegratedEI
    X, Y = known["X"], known["Y"]
    start = make_kernel("ard", np.exp(known["true"] + .3))
    with warnings.catch_warnings():
        warnings.simplefilter("error")               # (nothing is dropped here)
        E = GaussianProcessEnsemble.sample(start, X, Y, n=6, chains=3, burn=5, thin=1, seed=1)
    assert len(E.members) == 6 and E.loghyper.shape == (6, 2) and np.allclose(E.weights, 1 / 6.0)
    assert all(np.allclose(np.log(m.kernel.hyperparams), r) for m, r in zip(E.members, E.loghyper))
    first = [m.kernel.hyperparams.copy() for m in E.members]
    v = IntegratedEI(E).values(np.random.RandomState(2).rand(9, 2))
    assert np.all(np.isfinite(v)) and np.all(v >= 0)
    o, ox = maximizeIntegratedEI(E, [[0., 1.]] * 2, maxiter=5)
    assert np.isfinite(o) and ox.shape == (2,)
    E.addData(np.array([[.5, .5]]), [0.1])
    E.resample(seed=2, n=4)
    assert len(E.members) == 4 and len(E.X) == 41 and not np.array_equal(E.members[0].kernel.hyperparams, first[0])


def test_a_draw_whose_fit_is_not_positive_definite_is_dropped_with_a_warning(lib, known, monkeypatch):
    """Matern-3/2 draws of (length scale, magnitude): a magnitude of 1.5 puts 2.25 k beside a diagonal of 1 + noise, which no fit factors
    (the sampler's own likelihood, K + noise I, does).  The sampler is replaced by fixed draws so that which rows fail is known."""
    from ibo_amd.gaussianprocess import GaussianProcessEnsemble, ensemble
    X, Y = known["X"], known["Y"]
    draws = np.log(np.array([[.5, .8], [.5, 1.5], [.4, .9], [.6, 1.5]]))
    seen = {}

    def fixed(kernel, X, Y, **kw):
        seen.update(kw)
        return draws.copy(), np.arange(4.0)
    monkeypatch.setattr(ensemble.hypersample, "sampleHyper", fixed)
    with pytest.warns(UserWarning, match="not positive definite") as rec:
        E = GaussianProcessEnsemble.sample(make_kernel("m3", [.5, .8]), X, Y, n=4, noise=1e-3, device=0)
    assert len(rec) == 2 and seen["device"] == 0 and seen["n"] == 4
    assert len(E.members) == 2 and np.array_equal(E.loghyper, draws[[0, 2]]) and np.array_equal(E.logp, [0.0, 2.0])
    assert all(np.allclose(np.log(m.kernel.hyperparams), r) for m, r in zip(E.members, E.loghyper)) and np.allclose(E.weights, .5)
    assert np.all(np.isfinite(E.posteriors(X[:3])[0]))
    monkeypatch.setattr(ensemble.hypersample, "sampleHyper", lambda kernel, X, Y, **kw: (draws[[1, 3]].copy(), np.zeros(2)))
    with pytest.warns(UserWarning), pytest.raises(ValueError):
        GaussianProcessEnsemble.sample(make_kernel("m3", [.5, .8]), X, Y, n=2, noise=1e-3)

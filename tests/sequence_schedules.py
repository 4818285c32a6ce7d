"""
The fixed mutation schedules of tests/test_gpu_acquisition_sequences.py, their host-side replay, and the restatements of the six newer
acquisition families on a replayed state.  tests/test_sequence_reference.py pins what is in here on the CPU; the GPU file holds a handle
that went through the same steps to it.

A schedule is an explicit list of steps (op, argument, refit): the third entry says whether the Python class refits (padding full, more than
EXTEND_MAX points, more than REMOVE_MAX rows) or the step runs in place on the handle.
    ("add", k, refit)        addData of k points drawn from the schedule's generator
    ("rm", rows, refit)      removeData of these row indices
    ("set_y", amplitude, False)   ibo_gp_set_y with Y + amplitude * randn
    ("prior", index, False)  the mean prior becomes priors[index]: None, make_prior(D, 11), make_prior(D, 12)
    ("kstar", c, False)      ibo_gp_set_kstar_sf2 with c times the model's own signal variance (1.0 restores it)
The replay draws from numpy.random.RandomState(seed) exactly as test_gpu_handle_sequences.Driver does (rows, targets, then per step the new
rows and their targets, or the randn of set_y), so the GPU file can assert after every step that the driver's mirror IS the replayed state.

The two-model entries (constrained EI, EHVI) need a second model of the SAME dimension: ibo_cacq_* and ibo_ehvi_* refuse models of different
D.  The partner of a schedule is therefore the OTHER schedule's kernel, prior, row count, reserve and steps replayed at the driven model's
D (other data: seed + 50), at its own stage: after the driven model's step k it has gone through its first min(k, its length) steps, so
the two handles of a call differ in N, in Npad and in how their factors came about.  The D = 33 schedule pairs with a plain model.

`restate(state, pts, partner)` evaluates kg_reference, qei_reference, cacq_reference, ehvi_reference, paths_reference and
paths_grad_reference on a state and returns {key: (value, bar)} -- key "family/..." -- with every bar the family's own:
    kg     mu_ref, mu: kr.tol_mu; s2: 1e-6 s2; b: kr.tol_b; kg: kr.tol_kg                       (16 reference points, both with_self)
    qei    mu_pend, mu: qr.tol_mu; s2: 1e-6 s2; S_pend, c: qr.tol_S, qr.tol_c; qei, base: qr.tol_qei     (5 pending points, 64 antithetic draws)
    cacq   acq, pof, val: rtol 1e-6, atol 1e-12 (ref_close); dval: 1e-9 sval + 1e-13            (NR erf / clamp 1e-7 on the batch, libm / 1e-8 on the sweep rows)
    ehvi   val: 1e-6 S + 1e-9 bar; dval: 1e-9 sval + 1e-13                                      (fronts of 0 and 65 points)
    paths  coef: 1e-6 max |c|; values: 1e-6 T                                                   (F = 96, S = 5, eps redrawn for the state's N)
    pgrad  grads: 1e-6 T_grad
The points (`points`) belong to ONE state -- the one after a step -- and the same points serve the state before it, so that the two
restatements can be compared entry by entry (test_sequence_reference.py, "every changing step is visible").
"""
import copy
import functools
import types

import numpy as np

import cacq_reference as cr
import ehvi_reference as er
import grad_reference as gr
import kg_reference as kr
import paths_grad_reference as pg
import paths_reference as pr
import qei_reference as qr
from test_gpu_handle_sequences import KSTAR_SCALE, target
from test_gpu_remove import NOISE, hyper_of, make_kernel, make_prior

EXTEND_MAX, REMOVE_MAX = 16, 2          # GaussianProcess.EXTEND_MAX / .REMOVE_MAX (the CPU test asserts they still are)
SET_Y = .05                             # set_y's amplitude, Driver.step's

SCHEDULES = {
    # 62 -> 63 -> 64 (N == Npad) -> 65 (padding refit, Npad 128) -> 64 -> 62 (a whole stale 64-tile behind N) -> ... -> 65 -> 62 (refit)
    "ard": dict(kind="ard", D=4, N0=62, reserve=0, prior=0, seed=201, other="m5", steps=[
        ("add", 1, False), ("add", 1, False), ("add", 1, True), ("rm", [0], False), ("rm", [9, 40], False), ("set_y", SET_Y, False),
        ("prior", 1, False), ("prior", 2, False), ("kstar", KSTAR_SCALE, False), ("kstar", 1.0, False), ("add", 3, False),
        ("rm", [1, 20, 50], True)]),
    # 31 (+ 8 reserved: Npad 64) -> 32 -> 33 -> 32 (the last row) -> 30 -> ... -> 47 (refit) -> 46
    "m5": dict(kind="m5", D=8, N0=31, reserve=8, prior=1, seed=202, other="ard", steps=[
        ("add", 1, False), ("add", 1, False), ("rm", [32], False), ("rm", [3, 17], False), ("set_y", SET_Y, False), ("prior", 0, False),
        ("add", EXTEND_MAX + 1, True), ("rm", [23], False)]),
    # the difference-form-only route: no dot form, no kept state.  70 (Npad 128) -> 71 -> 69 -> 69 -> 70
    "svard": dict(kind="svard", D=33, N0=70, reserve=0, prior=0, seed=203, other=None, steps=[
        ("add", 1, False), ("rm", [5, 60], False), ("set_y", SET_Y, False), ("add", 1, False)]),
}
PLAIN = dict(kind="m5", N=45, seed=204)            # the D = 33 schedule's partner: one plain fit, never changed

N_REF, N_PEND, N_SAMP, N_BATCH, N_SWEEP = 16, 5, 64, 64, 1000
PATHS_F, PATHS_S, PATHS_SEED = 96, 5, 17
FRONTS = (0, 65)
EHVI_REF, EHVI_TOP = np.array([-1.5, -1.5]), np.array([1.0, 1.0])
CON_OTHER, CON_SELF = (.2, 1), (-.2, -1)           # (threshold, sense): the partner's function <= .2; the objective's own >= -.2
SWEEP_ROWS = np.unique(np.r_[0, 255, 256, 999, np.random.RandomState(3).randint(0, N_SWEEP, 28)])
FAMILIES = ("kg", "qei", "cacq", "ehvi", "paths", "pgrad")
VALUE_OF = {"kg": "kg/ws1/kg", "qei": "qei/qei", "cacq": "cacq/other/val", "ehvi": "ehvi/other/65/val", "paths": "paths/values",
            "pgrad": "pgrad/grads"}               # the quantity that must move with every changing step


def padded(n, reserve):
    return -(-(n + reserve) // 64) * 64


def priors_of(D):
    out = [None]
    for seed in (11, 12):
        p = make_prior(D, seed)
        out.append((p.means, p.beta, p.theta, p.lowerb, p.width))
    return out


def _state(sch, D, X, Y, pk, kc, Npad, seed):
    return types.SimpleNamespace(kind=sch["kind"], D=D, X=X.copy(), Y=Y.copy(), pk=pk, kc=kc, N=len(X), Npad=Npad, seed=seed,
                                 prior=priors_of(D)[pk])


@functools.lru_cache(maxsize=None)
def replay(name, D=None, seed=None):
    """the states of schedule `name` (at dimension D, from `seed`): [before any step, after step 1, ..]"""
    sch = SCHEDULES[name]
    D = sch["D"] if D is None else D
    seed = sch["seed"] if seed is None else seed
    rs = np.random.RandomState(seed)
    X = rs.rand(sch["N0"], D)
    Y = target(X, rs)
    pk, kc, Npad = sch["prior"], 1.0, padded(sch["N0"], sch["reserve"])
    out = [_state(sch, D, X, Y, pk, kc, Npad, seed)]
    for op, arg, refit in sch["steps"]:
        if op == "add":
            x = rs.rand(arg, D)
            y = target(x, rs)
            assert refit == (Npad - len(X) < arg or arg > EXTEND_MAX), (name, op, arg)
            X, Y = np.r_[X, x], np.r_[Y, y]
        elif op == "rm":
            assert refit == (len(arg) > REMOVE_MAX), (name, op, arg)
            keep = np.setdiff1d(np.arange(len(X)), arg)
            assert len(keep) == len(X) - len(arg)
            X, Y = X[keep], Y[keep]
        elif op == "set_y":
            Y = Y + arg * rs.randn(len(Y))
        elif op == "prior":
            pk = arg
        elif op == "kstar":
            kc = arg
        else:
            raise ValueError(op)
        if refit:
            Npad = padded(len(X), sch["reserve"])
        assert len(X) <= Npad
        out.append(_state(sch, D, X, Y, pk, kc, Npad, seed))
    return out


@functools.lru_cache(maxsize=None)
def partner_states(name):
    """the partner of schedule `name` after each of ITS steps (see the module docstring); a plain model for the D = 33 schedule"""
    sch = SCHEDULES[name]
    if sch["other"] is None:
        rs = np.random.RandomState(PLAIN["seed"])
        X = rs.rand(PLAIN["N"], sch["D"])
        return [_state(PLAIN, sch["D"], X, target(X, rs), 0, 1.0, padded(PLAIN["N"], 0), PLAIN["seed"])]
    return replay(sch["other"], sch["D"], SCHEDULES[sch["other"]]["seed"] + 50)


def partner_at(name, k):
    """the partner's state after the driven model's step k"""
    ps = partner_states(name)
    return ps[min(k, len(ps) - 1)]


def ref_of(st):
    """(RefGP of a state, its k* signal variance)"""
    fam, w, sf2 = gr.kernel_spec(st.kind, hyper_of(st.kind, st.D), st.D)
    ref = gr.RefGP(st.X, st.Y, NOISE, fam, w, sf2, prior=st.prior)
    return ref, st.kc * sf2


def cond_bound(st):
    """cond_2(R) <= N (1 + noise) / noise by test_gpu_remove.cond_of's bound, asserted on the state's own matrix"""
    from test_gpu_remove import cond_of
    return cond_of(ref_of(st)[0].R, "bound")


def draws(st, N=None):
    """the spectral draws of a state: eps is S x N, so it is drawn anew whenever N changes (omega, phase, w come first and stay)"""
    from ibo_amd.acquisition import spectralDraws
    sf2 = gr.kernel_spec(st.kind, hyper_of(st.kind, st.D), st.D)[2]
    return spectralDraws(make_kernel(st.kind, hyper_of(st.kind, st.D)), st.D, PATHS_F, PATHS_S, st.N if N is None else N, 1 + NOISE - sf2,
                         PATHS_SEED)


def points(st):
    """what a state is evaluated at: Q (64 host points, the first four training inputs as check_readers_like_fresh takes them), A (16
    reference points), P (5 pending points), Z (64 antithetic draws), C (the first 1000 rows of the driver's candidate array)"""
    from ibo_amd.acquisition import baseSamples
    Q = np.random.RandomState(6).rand(N_BATCH, st.D) * 1.2 - .1
    Q[:4] = st.X[[0, st.N - 1, st.N // 2, st.N // 3]]
    C = np.random.RandomState(st.seed + 1000).rand(9001, st.D)[:N_SWEEP]
    return types.SimpleNamespace(Q=Q, A=kr.ref_points(st.X, N_REF), P=qr.pending_points(st.X, N_PEND), Z=baseSamples(N_PEND + 1, N_SAMP, seed=1),
                                 C=C, fronts={n: er.curve_front(n, EHVI_REF, EHVI_REF + .7 * (EHVI_TOP - EHVI_REF)) for n in FRONTS})


def paths_ref(ref, sf2k):
    """the RefGP the path restatements read: the factor of the fitted matrix, features and k* with the handle's k* signal variance"""
    if sf2k == ref.sf2:
        return ref
    r = copy.copy(ref)
    r.sf2 = sf2k
    return r


def restate(st, pts, partner, families=FAMILIES):
    """{key: (value, bar)} of the families on state `st` at the points `pts`, the second model `partner` (a state)"""
    ref, sf2k = ref_of(st)
    out = {}
    if "kg" in families:
        for ws in (1, 0):
            w = kr.kg(ref, pts.A, pts.Q, bool(ws), sf2k=sf2k)
            pre = "kg/ws%d/" % ws
            out[pre + "mu_ref"] = (w["mu_ref"], kr.tol_mu(w["mu_ref"]))
            out[pre + "mu"] = (w["mu"], kr.tol_mu(w["mu"]))
            out[pre + "s2"] = (w["s2"], 1e-6 * w["s2"])
            out[pre + "b"] = (w["b"], kr.tol_b(w, ref.sf2, ref.noise))
            out[pre + "kg"] = (w["kg"], kr.tol_kg(w, ref.sf2, ref.noise, ws))
    if "qei" in families:
        t = float(np.max(st.Y)) + qr.XI
        w = qr.qei(ref, pts.P, pts.Q, pts.Z, t, sf2k=sf2k)
        tq = qr.tol_qei(w, pts.Z, t, ref.sf2, ref.noise)
        out["qei/mu_pend"] = (w["mu_pend"], qr.tol_mu(w["mu_pend"]))
        out["qei/mu"] = (w["mu"], qr.tol_mu(w["mu"]))
        out["qei/s2"] = (w["s2"], 1e-6 * w["s2"])
        out["qei/S_pend"] = (w["S_pend"], qr.tol_S(w, ref.sf2, ref.noise))
        out["qei/c"] = (w["c"], qr.tol_c(w, ref.sf2, ref.noise))
        out["qei/qei"] = (w["qei"], tq)
        out["qei/base"] = (np.array([w["base"]]), np.array([np.max(tq)]))
    if "cacq" in families or "ehvi" in families:
        mo = cr.Model(ref, sf2k=sf2k)
        pref, psf2k = ref_of(partner)
        mp = cr.Model(pref, sf2k=psf2k)
    if "cacq" in families:
        close = lambda v: (v, 1e-6 * np.abs(v) + 1e-12)                       # test_gpu_constrained.ref_close
        for name, m, (th, se) in (("other", mp, CON_OTHER), ("self", mo, CON_SELF)):
            con = [cr.Model(m.ref, thresh=th, sense=se, sf2k=m.sf2k)]
            b = cr.value(mo, con, pts.Q, gr.ACQ_EI, .01, gr.ERF_NR, 1e-7)
            s = cr.value(mo, con, pts.C[SWEEP_ROWS], gr.ACQ_EI, .01, gr.ERF_LIBM, 1e-8)
            g = cr.value_grad(mo, con, pts.Q, gr.ACQ_EI, .01, gr.ERF_NR, 1e-7)
            for k in ("acq", "pof", "val"):
                out["cacq/%s/%s" % (name, k)] = close(b[k])
            for k in ("pof", "val"):
                out["cacq/%s/sweep_%s" % (name, k)] = close(s[k])
            out["cacq/%s/dval" % name] = (g["dval"], 1e-9 * g["sval"] + 1e-13)
    if "ehvi" in families:
        for name, models in (("other", [mo, mp]), ("self", [mo, mo])):
            for n in FRONTS:
                g = er.value_grad(models, pts.Q, pts.fronts[n], EHVI_REF, gr.ERF_LIBM, 1e-8)
                v = er.value(models, pts.Q, pts.fronts[n], EHVI_REF, gr.ERF_LIBM, 1e-8)
                out["ehvi/%s/%d/val" % (name, n)] = (v["val"], 1e-6 * v["S"] + 1e-9 * v["bar"])
                out["ehvi/%s/%d/dval" % (name, n)] = (g["dval"], 1e-9 * g["sval"] + 1e-13)
    if "paths" in families or "pgrad" in families:
        omega, phase, w, eps = draws(st)
        rk = paths_ref(ref, sf2k)
        c = pr.coef(rk, omega, phase, w, eps)
    if "paths" in families:
        out["paths/coef"] = (c[:, PATHS_F:], np.full(c[:, PATHS_F:].shape, 1e-6 * np.max(np.abs(c[:, PATHS_F:]))))
        out["paths/values"] = (pr.values(rk, omega, phase, c, pts.Q), 1e-6 * pr.terms_scale(rk, omega, phase, c, pts.Q))
    if "pgrad" in families:
        out["pgrad/grads"] = (pg.grads(rk, omega, phase, c, pts.Q), 1e-6 * pg.grad_scale(rk, omega, phase, c, pts.Q))
    return out


def family_of(key):
    return key.split("/")[0]

"""
The six newer acquisition families -- constrained EI (ibo_cacq_*), the knowledge gradient (ibo_kg_*), pathwise draws (ibo_paths_*), Monte-Carlo
q-EI (ibo_qei_*), two-objective EHVI (ibo_ehvi_*) and path gradients (ibo_paths_grad_batch) -- on a handle that has been CHANGED: extended,
reduced, given other targets, another prior, another k* variance, refitted by the padding, by EXTEND_MAX and by REMOVE_MAX.  The life-cycle
files (test_gpu_handle_sequences.py, test_gpu_remove.py) hold the older readers to a fresh model after every step; the families' own files
build their models with one plain fit.  Here the fixed schedules of tests/sequence_schedules.py put N on the edges of the newer kernels (the
64-row tile, the 32-wide k-step of cov_tri and of q-EI's cross block, N == Npad, a whole stale 64-tile behind N), and after EVERY step every
family is held
    to its restatement on the driver's host mirror (sequence_schedules.restate: kg_reference, qei_reference, cacq_reference, ehvi_reference,
        paths_reference, paths_grad_reference), at the family's own bar, and to the compositions of its own pieces (composition_close,
        compose_close at 1e-12 of scale; the paths' values and gradients on the device's own coefficients at 1e-11 T / 1e-11 T_grad);
    to a FRESH handle on the same data through the same calls: each is within one bar of the same restatement, so the two agree within two
        bars -- the only number here that is not a family's own, and it is derived.  No bit identity with the fresh model: an extended or
        reduced factor differs from a refitted one in its last bits;
    to ONE set of bits whatever the route, on the changed handle: sweep = host batch = single-point batches, chunk option 256 against 0
        (KG, q-EI, paths with grad_batch's values, EHVI with the gradient entry's values);
    to the arg-max contract: best_idx is index_base (7) + the first arg-max of the sweep's own returned values.
The two-model entries get a second handle of the same dimension that is itself in the middle of ANOTHER schedule (sequence_schedules:
the partner), so the two handles of one call differ in N, Npad and history; and the driven handle as its own constraint / second objective.
The driver's refit counter asserts which steps refit and which run in place (Driver.add / .remove): an in-place step that refitted silently
would test nothing.  tests/test_sequence_reference.py shows on the CPU that every step moves every family's value by at least ten bars, so a
handle that still held the old rows, Y, prior or k* variance fails here.  Noise .1: cond_2(R) <= N 1.1 / .1, asserted per schedule.

Worst error / bar over the steps of each schedule, measured on an MI355X (changed handle against the restatement; in brackets the changed
handle against the fresh one, as a share of its two bars; paths and pgrad include the 1e-11 bars on the device's own coefficients):
    ard    kg 1.7e-6 [7.9e-7]  qei 6.5e-6 [4.5e-6]  cacq 1.2e-4 [2.0e-5]  ehvi 1.4e-6 [5.2e-7]  paths 2.5e-5 [1.0e-5]  pgrad 2.9e-5 [1.6e-5]
    m5     kg 1.1e-6 [2.1e-7]  qei 2.0e-6 [5.3e-7]  cacq 3.0e-6 [6.5e-7]  ehvi 9.7e-7 [2.2e-7]  paths 2.5e-5 [7.4e-6]  pgrad 3.5e-5 [1.2e-5]
    svard  kg 1.3e-6 [2.8e-7]  qei 2.2e-6 [6.0e-7]  cacq 9.9e-7 [7.8e-7]  ehvi 5.2e-7 [2.0e-7]  paths 2.1e-5 [7.5e-6]  pgrad 4.9e-5 [1.4e-5]
At noise .1 and these sizes the device is five to six orders of magnitude inside every bar, on changed handles as on fresh ones, and every
bit comparison held: no step of these schedules exposed a stale row, a stale Y, prior or k* variance in any family.  A case takes 0.1 .. 0.35 s.
"""
import ctypes

import numpy as np
import pytest

import cacq_reference as cr
import paths_grad_reference as pg
import paths_reference as pr
import qei_reference as qr
import sequence_schedules as ss
from test_gpu_constrained import pack
from test_gpu_constrained import raw_batch as cacq_batch
from test_gpu_ehvi import raw_batch as ehvi_batch
from test_gpu_ehvi import raw_sweep as ehvi_sweep
from test_gpu_handle_sequences import Driver
from test_gpu_knowledge_gradient import composition_close, kg_call
from test_gpu_paths import Paths
from test_gpu_paths_grad import grad_call
from test_gpu_qei import compose_close, qei_call
from test_gpu_qei import sweep_call as qei_sweep
from test_gpu_remove import NOISE, cond_of, new_gp
from wall_time import wall

pytestmark = pytest.mark.gpu

NAN = float("nan")
BASE = 7                       # index_base of every sweep
SINGLES = (0, 255, 256, 999)   # candidates evaluated once more in a batch of one
STEPS = [(name, k) for name in sorted(ss.SCHEDULES) for k in range(1, len(ss.SCHEDULES[name]["steps"]) + 1)]


@pytest.fixture(scope="module")
def lib():
    from ibo_amd import _lib
    if _lib.device_count() < 1:
        pytest.fail("no GPU visible: the product has no CPU fallback")
    return _lib


# ---------------------------------------------------------------------------------------------------------------- driving a handle
def apply(lib, d, step):
    """one step of a schedule on the driver d; Driver.add / .remove assert the refit count, the other steps must not refit at all"""
    op, arg, refit = step
    before = d.refits
    if op == "add":
        d.add(arg, refit)
    elif op == "rm":
        d.remove(list(arg), None if refit else "device", refit)
    elif op == "set_y":
        d.Y = d.Y + arg * d.rs.randn(len(d.Y))
        lib.check(lib.lib.ibo_gp_set_y(d.GP._handle(), lib.dp(lib.f64(d.Y))))
        d.GP.Y = d.Y.copy()
    elif op == "prior":
        d.pk = arg
        d.GP.prior = d.priors[arg]
        d.GP._push_prior()
    elif op == "kstar":
        d.kc = arg
        lib.check(lib.lib.ibo_gp_set_kstar_sf2(d.GP._handle(), arg * d.GP.kernel._ibo_spec()[2]))
    else:
        raise ValueError(op)
    assert d.refits - before == int(refit), (step, d.refits - before)


def driver_of(lib, name, D=None, seed=None):
    sch = ss.SCHEDULES[name]
    d = Driver(lib, sch["kind"], sch["D"] if D is None else D, sch["N0"], sch["reserve"], bool(sch["prior"]),
               sch["seed"] if seed is None else seed)
    d.kc = 1.0
    return d


class Plain(object):
    """the D = 33 schedule's partner: one plain fit that no step changes"""

    def __init__(self, st):
        self.GP, self.X, self.Y, self.pk, self.Npad = new_gp(st.kind, st.D, st.X, st.Y), st.X, st.Y, 0, st.Npad


class Pair(object):
    """the driven handle of a schedule and its partner, both moved step by step; is_state asserts the mirrors ARE the replayed states"""

    def __init__(self, lib, name):
        self.lib, self.name, self.sch = lib, name, ss.SCHEDULES[name]
        self.d = driver_of(lib, name)
        other = self.sch["other"]
        if other is None:
            self.p, self.psteps = Plain(ss.partner_states(name)[0]), []
        else:
            self.p = driver_of(lib, other, self.sch["D"], ss.SCHEDULES[other]["seed"] + 50)
            self.psteps = ss.SCHEDULES[other]["steps"]
        self.k = 0
        self.is_state()

    def step(self):
        self.k += 1
        apply(self.lib, self.d, self.sch["steps"][self.k - 1])
        if self.k <= len(self.psteps):
            apply(self.lib, self.p, self.psteps[self.k - 1])
        self.is_state()

    def is_state(self):
        for drv, st in ((self.d, ss.replay(self.name)[self.k]), (self.p, ss.partner_at(self.name, self.k))):
            assert np.array_equal(drv.X, st.X) and np.array_equal(drv.Y, st.Y) and drv.pk == st.pk and drv.Npad == st.Npad, (self.name, self.k)
            assert np.array_equal(drv.GP.X, st.X) and np.array_equal(drv.GP.Y, st.Y)
        assert self.d.kc == ss.replay(self.name)[self.k].kc

    def fresh(self):
        """a fresh model on the driven handle's data, prior and k* variance"""
        fr = self.d.fresh()
        fr._push_prior()
        self.lib.check(self.lib.lib.ibo_gp_set_kstar_sf2(fr._handle(), self.d.kc * fr.kernel._ibo_spec()[2]))
        return fr

    def cand(self):
        return self.d.cand.view_rows(0, ss.N_SWEEP)


# ---------------------------------------------------------------------------------------------------------------- the calls
def cacq_sweep(lib, obj, cons, dc, erf_mode=0, clamp=1e-8, base=0):
    """ibo_cacq_sweep with its three per-candidate outputs -> dict(acq, pof, val, best_val, best_idx)"""
    from ibo_amd import DeviceArray
    n, con, th, se, keep = pack(lib, cons)
    M = dc.shape[0]
    outs = {k: DeviceArray((M,)) for k in ("acq", "pof", "val")}
    bv = ctypes.c_double(-5.0); bi = ctypes.c_int64(-5)
    lib.check(lib.lib.ibo_cacq_sweep(obj, n, con, th, se, M, dc.ptr, 0, .01, erf_mode, clamp, NAN, 0, None, .5, base, outs["acq"].ptr,
                                     outs["pof"].ptr, outs["val"].ptr, ctypes.byref(bv), ctypes.byref(bi)))
    res = {k: v.to_host() for k, v in outs.items()}
    res.update(best_val=bv.value, best_idx=bi.value)
    return res


def kg_sweep(lib, h, A, dc, ws=1, base=0):
    from ibo_amd import DeviceArray
    M = dc.shape[0]
    A = lib.f64(A)
    out = DeviceArray((M,))
    bv = ctypes.c_double(); bi = ctypes.c_int64()
    lib.check(lib.lib.ibo_kg_sweep(h, len(A), lib.dp(A), M, dc.ptr, ws, 1e-7, base, out.ptr, ctypes.byref(bv), ctypes.byref(bi)))
    return out.to_host(), bv.value, bi.value


def first_argmax(v, bv, bi, what):
    assert bi == BASE + int(np.argmax(v)) and bv == np.max(v), (what, bi, int(np.argmax(v)))


def batch_outputs(lib, GP, other, st, pts, cand, rk, what):
    """every family's host-batch outputs (and the constrained sweep's rows) on the handle of GP -> ({key: value} under restate's keys,
    {key: (value, restatement on the device's own coefficients, bar)}); the compositions of a call's own pieces are asserted here"""
    h = GP._handle()
    GP._push_prior(); other._push_prior()
    out, own = {}, {}
    for ws in (1, 0):
        g = kg_call(lib, h, pts.A, pts.Q, ws)
        composition_close(g, ws, "%s KG with_self=%d" % (what, ws))
        for k in ("mu_ref", "mu", "s2", "b", "kg"):
            out["kg/ws%d/%s" % (ws, k)] = g[k]
    g = qei_call(lib, h, pts.P, pts.Z, pts.Q)
    assert g["info"] == 0 and np.array_equal(g["S_pend"], g["S_pend"].T)
    compose_close(g, pts.Z, float(np.max(st.Y)) + qr.XI, what + " q-EI")
    for k in ("mu_pend", "mu", "s2", "S_pend", "c", "qei"):
        out["qei/" + k] = g[k]
    out["qei/base"] = np.array([g["base"]])
    for name, hc, (th, se) in (("other", other._handle(), ss.CON_OTHER), ("self", h, ss.CON_SELF)):
        cons = [(hc, th, se)]
        rc, b = cacq_batch(lib, h, cons, pts.Q, 0, .01, 1, 1e-7)
        rcg, gb = cacq_batch(lib, h, cons, pts.Q, 0, .01, 1, 1e-7, grad=True)
        assert rc == 0 and rcg == 0 and np.array_equal(gb["val"], b["val"])
        s = cacq_sweep(lib, h, cons, cand, 0, 1e-8, BASE)
        assert (s["best_idx"] - BASE, s["best_val"]) == cr.argmax(s["val"]), what
        for k in ("acq", "pof", "val"):
            out["cacq/%s/%s" % (name, k)] = b[k]
        for k in ("pof", "val"):
            out["cacq/%s/sweep_%s" % (name, k)] = s[k][ss.SWEEP_ROWS]
        out["cacq/%s/dval" % name] = gb["dval"]
    for name, GPs in (("other", [GP, other]), ("self", [GP, GP])):
        for n in ss.FRONTS:
            rc, val, grad = ehvi_batch(lib, GPs, pts.fronts[n], ss.EHVI_REF, pts.Q, 0, 1e-8, grad=True)
            assert rc == 0 and np.all(val >= 0)
            out["ehvi/%s/%d/val" % (name, n)] = val
            out["ehvi/%s/%d/dval" % (name, n)] = grad
    omega, phase, w, eps = ss.draws(st)
    assert eps.shape == (ss.PATHS_S, len(GP.X))
    P = Paths(lib, GP, omega, phase, w, eps)
    try:
        coef = P.coef()
        vals = P.batch(pts.Q)
        v2, grads = grad_call(lib, P, pts.Q)
    finally:
        P.close()
    assert np.array_equal(coef[:, :ss.PATHS_F], w) and np.array_equal(v2, vals)
    out["paths/coef"], out["paths/values"], out["pgrad/grads"] = coef[:, ss.PATHS_F:], vals, grads
    if rk is None:
        return out, own
    own["paths/own_values"] = (vals, pr.values(rk, omega, phase, coef, pts.Q), 1e-11 * pr.terms_scale(rk, omega, phase, coef, pts.Q))
    own["pgrad/own_grads"] = (grads, pg.grads(rk, omega, phase, coef, pts.Q), 1e-11 * pg.grad_scale(rk, omega, phase, coef, pts.Q))
    return out, own


def route_outputs(lib, GP, other, st, pts, cand, what, chunks=(0, 256)):
    """On the handle of GP: the sweeps over the 1000 device candidates against the host batch over the same rows, batches of one, and the
    chunk options at 256 against 0 -- np.array_equal throughout; every sweep's best_idx against its own values.  -> {key: sweep values}"""
    h = GP._handle()
    GP._push_prior(); other._push_prior()
    C, bits = pts.C, {}
    F = pts.fronts[65]
    omega, phase, w, eps = ss.draws(st)
    P = Paths(lib, GP, omega, phase, w, eps)
    try:
        for chunk in chunks:
            for key in (b"kg_chunk", b"qei_chunk", b"paths_chunk", b"ehvi_chunk"):
                lib.check(lib.lib.ibo_set_option(key, chunk))
            for ws in (1, 0):
                v, bv, bi = kg_sweep(lib, h, pts.A, cand, ws, BASE)
                first_argmax(v, bv, bi, what + " KG")
                assert np.array_equal(kg_call(lib, h, pts.A, C, ws, slopes=False)["kg"], v), (what, "KG sweep against batch", chunk)
                one = np.array([kg_call(lib, h, pts.A, C[i], ws, slopes=False)["kg"][0] for i in SINGLES])
                assert np.array_equal(one, v[list(SINGLES)]), (what, "KG batches of one", chunk)
                assert np.array_equal(bits.setdefault("kg/ws%d" % ws, v), v), (what, "kg_chunk")
            bv, bi, v, base = qei_sweep(lib, h, pts.P, pts.Z, cand, ss.N_SWEEP, index_base=BASE)
            first_argmax(v, bv, bi, what + " q-EI")
            g = qei_call(lib, h, pts.P, pts.Z, C, pieces=False)
            assert np.array_equal(g["qei"], v) and g["base"] == base, (what, "q-EI sweep against batch", chunk)
            one = np.array([qei_call(lib, h, pts.P, pts.Z, C[i], pieces=False)["qei"][0] for i in SINGLES])
            assert np.array_equal(one, v[list(SINGLES)]), (what, "q-EI batches of one", chunk)
            assert np.array_equal(bits.setdefault("qei", v), v), (what, "qei_chunk")
            bv, bi, v = P.sweep(cand, index_base=BASE)
            assert np.array_equal(bi, BASE + np.argmax(v, axis=1)) and np.array_equal(bv, np.max(v, axis=1)), what + " paths"
            assert np.array_equal(P.batch(C), v) and np.array_equal(grad_call(lib, P, C)[0], v), (what, "paths sweep, batch, grad_batch", chunk)
            assert np.array_equal(bits.setdefault("paths", v), v), (what, "paths_chunk")
            for name, GPs in (("other", [GP, other]), ("self", [GP, GP])):
                rc, v, bv, bi = ehvi_sweep(lib, GPs, F, ss.EHVI_REF, cand, base=BASE)
                assert rc == 0
                first_argmax(v, bv, bi, what + " EHVI")
                rcb, b = ehvi_batch(lib, GPs, F, ss.EHVI_REF, C)
                rcg, gv, _ = ehvi_batch(lib, GPs, F, ss.EHVI_REF, C, grad=True)
                assert rcb == 0 and rcg == 0 and np.array_equal(b, v) and np.array_equal(gv, v), (what, "EHVI sweep, batch, gradient entry", chunk)
                assert np.array_equal(bits.setdefault("ehvi/" + name, v), v), (what, "ehvi_chunk")
    finally:
        P.close()
        for key in (b"kg_chunk", b"qei_chunk", b"paths_chunk", b"ehvi_chunk"):
            lib.check(lib.lib.ibo_set_option(key, 0))
    return bits


def worst_by_family(ratios):
    w = {}
    for key, r in ratios.items():
        w[ss.family_of(key)] = max(w.get(ss.family_of(key), 0.0), r)
    return " ".join("%s %.3g" % (f, w[f]) for f in ss.FAMILIES)


def check_step(lib, pair, what):
    """all of the module docstring's checks on the pair's driven handle as it is now"""
    st, partner = ss.replay(pair.name)[pair.k], ss.partner_at(pair.name, pair.k)
    pts = ss.points(st)
    ref, sf2k = ss.ref_of(st)
    rk = ss.paths_ref(ref, sf2k)
    want = ss.restate(st, pts, partner)
    res = {}
    for label, GP in (("changed", pair.d.GP), ("fresh", pair.fresh())):
        out, own = batch_outputs(lib, GP, pair.p.GP, st, pts, pair.cand(), rk, "%s %s" % (what, label))
        assert sorted(out) == sorted(want)
        r = {key: (out[key], want[key][0], want[key][1]) for key in want}
        r.update(own)
        ratios = {key: float(np.max(np.abs(g - w) / bar)) for key, (g, w, bar) in r.items()}
        print("%s, %s handle: worst error / bar  %s" % (what, label, worst_by_family(ratios)))
        for key in sorted(ratios):
            assert ratios[key] <= 1.0, (what, label, key, ratios[key])
        res[label] = r
    # each handle is within one bar of its restatement: their errors differ by at most two
    gap = {key: float(np.max(np.abs((res["changed"][key][0] - res["changed"][key][1]) - (res["fresh"][key][0] - res["fresh"][key][1]))
                             / (2 * res["changed"][key][2]))) for key in res["changed"]}
    print("%s, changed against fresh: worst difference / two bars  %s" % (what, worst_by_family(gap)))
    for key in sorted(gap):
        assert gap[key] <= 1.0, (what, "changed against fresh", key, gap[key])
    route_outputs(lib, pair.d.GP, pair.p.GP, st, pts, pair.cand(), what)


# ---------------------------------------------------------------------------------------------------------------- 1, 2. every step
@pytest.mark.parametrize("name,k", STEPS)
def test_every_family_after_every_step(lib, name, k):
    """The schedule `name` replayed up to its step k on a handle of its own (the refit counter asserts every step on the way, and the
    mirror is the replayed state after each), then check_step.  One case per step, so that a case stays at a second or two."""
    with wall("%s step %d" % (name, k)):
        pair = Pair(lib, name)
        for _ in range(k):
            pair.step()
        op, arg, refit = ss.SCHEDULES[name]["steps"][k - 1]
        st = ss.replay(name)[k]
        assert cond_of(ss.ref_of(st)[0].R, "bound") <= st.N * (1 + NOISE) / NOISE * (1 + 1e-12)
        assert pair.d.GP.kernel._ibo_spec()[2] <= 1.0
        check_step(lib, pair, "%s step %d (%s%s, N=%d of %d)" % (name, k, op, ", refit" if refit else "", st.N, st.Npad))


# ---------------------------------------------------------------------------------------------------------------- 3. further tests
def test_kept_state_survives_the_newer_entries_across_a_change(lib):
    """The first schedule's model, 9001 device candidates: an incremental EI sweep keeps a state; ibo_kg_sweep, ibo_qei_sweep and
    ibo_ehvi_sweep (the handle as both objectives) over the SAME DeviceArray leave ibo_sweep_state_info as it was; addData of one point in
    place; the next incremental sweep continues the state (rank1 / finish kernel) and finds the fresh model's arg-max (Driver.sweep's rule).
    The mutation-crossing counterpart of test_gpu_constrained.py::test_same_handle_twice_and_handles_left_alone."""
    with wall("kept state"):
        d = driver_of(lib, "ard")
        GP, h = d.GP, d.GP._handle()
        st = ss.replay("ard")[0]
        pts = ss.points(st)

        def state():
            t, c = ctypes.c_int64(), ctypes.c_int64()
            lib.check(lib.lib.ibo_sweep_state_info(h, ctypes.byref(t), ctypes.byref(c)))
            return t.value, c.value
        d.sweep()
        kept = state()
        assert kept[0] == (9001 + 31) // 32
        v, bv, bi = kg_sweep(lib, h, pts.A, d.cand, 1, BASE)
        first_argmax(v, bv, bi, "KG over the kept state's array")
        bv, bi, v, _ = qei_sweep(lib, h, pts.P, pts.Z, d.cand, 9001, index_base=BASE)
        first_argmax(v, bv, bi, "q-EI over the kept state's array")
        rc, v, bv, bi = ehvi_sweep(lib, [GP, GP], pts.fronts[65], ss.EHVI_REF, d.cand, base=BASE)
        assert rc == 0
        first_argmax(v, bv, bi, "EHVI over the kept state's array")
        assert state() == kept
        d.add(1, False)
        kernel = d.sweep()
        assert "rank1" in kernel or "finish" in kernel, kernel
        assert state()[0] == kept[0]


def test_first_schedule_gives_the_same_bits_on_two_handles(lib):
    """KG, q-EI, EHVI and path outputs (host batches with their pieces, and whole sweeps) after every step of the first schedule on two
    handles: np.array_equal -- the fixed-order sums promise it.  test_mixed_sequence_gives_the_same_bits_on_two_handles covers L, W and
    the posteriors only."""
    with wall("the first schedule twice"):
        runs = []
        for _ in range(2):
            pair, got = Pair(lib, "ard"), []
            for k in range(1, len(pair.sch["steps"]) + 1):
                pair.step()
                st = ss.replay("ard")[k]
                pts = ss.points(st)
                out, _ = batch_outputs(lib, pair.d.GP, pair.p.GP, st, pts, pair.cand(), None, "step %d" % k)
                out.update(("sweep/" + key, v) for key, v in route_outputs(lib, pair.d.GP, pair.p.GP, st, pts, pair.cand(), "step %d" % k,
                                                                           chunks=(0,)).items())
                got.append(out)
            runs.append(got)
        for k, (a, b) in enumerate(zip(*runs), 1):
            assert sorted(a) == sorted(b)
            for key in a:
                assert np.array_equal(a[key], b[key]), ("step %d" % k, key)


def test_python_objects_follow_the_model(lib):
    """KnowledgeGradient, ParallelEI, ConstrainedEI, ExpectedHypervolumeImprovement (front= given) and a PosteriorPaths object built BEFORE
    the first schedule starts.  After step 2 (in place) and step 3 (the padding refit) the acquisition objects return what the raw entry
    returns on the handle as it is now, bit for bit (the same call; ConstrainedEI with the incumbent it took when it was built), and no
    longer what they returned before the step; the PosteriorPaths object returns its old values (a snapshot); one made now has the
    restatement's coefficients on the data as they are now (1e-6 max |c|, the feature weights as they went in)."""
    from ibo_amd.acquisition import KnowledgeGradient, ParallelEI, PosteriorPaths
    from ibo_amd.acquisition.constrained import ConstrainedEI, Constraint
    from ibo_amd.acquisition.multiobjective import ExpectedHypervolumeImprovement
    with wall("python objects"):
        pair = Pair(lib, "ard")
        GP, other = pair.d.GP, pair.p.GP
        pts = ss.points(ss.replay("ard")[0])
        Q, F = pts.Q, pts.fronts[65]
        th, se = ss.CON_OTHER
        objs = dict(kg=KnowledgeGradient(GP, pts.A), qei=ParallelEI(GP, pts.P, xi=qr.XI, Z=pts.Z), cacq=ConstrainedEI(GP, [Constraint(other, upper=th)], xi=.01),
                    ehvi=ExpectedHypervolumeImprovement([GP, other], ss.EHVI_REF, front=F))
        assert objs["cacq"].acq == 'ei'
        paths = PosteriorPaths(GP, n_paths=ss.PATHS_S, n_features=ss.PATHS_F, seed=ss.PATHS_SEED)
        snapshot = paths.values(Q), paths.gradient(Q)[1], paths.coef()

        def raw():
            h = GP._handle()
            rc, c = cacq_batch(lib, h, [(other._handle(), th, se)], Q, 0, .01, 1, 1e-7, objs["cacq"].ymax)
            rce, e = ehvi_batch(lib, [GP, other], F, ss.EHVI_REF, Q, 1, 1e-7)
            assert rc == 0 and rce == 0
            return dict(kg=kg_call(lib, h, pts.A, Q, 1, slopes=False)["kg"], qei=qei_call(lib, h, pts.P, pts.Z, Q, pieces=False)["qei"], cacq=c["val"], ehvi=e)
        last = {k: o.values(Q) for k, o in objs.items()}
        for k in (1, 2, 3):
            pair.step()
            if k == 1:
                continue
            now, want = {key: o.values(Q) for key, o in objs.items()}, raw()
            for key in objs:
                assert np.array_equal(now[key], want[key]), (k, key)
                assert not np.array_equal(now[key], last[key]), (k, key, "the object did not follow the model")
            last = now
            assert np.array_equal(paths.values(Q), snapshot[0]) and np.array_equal(paths.gradient(Q)[1], snapshot[1])
            assert np.array_equal(paths.coef(), snapshot[2])
            st = ss.replay("ard")[k]
            new = PosteriorPaths(GP, n_paths=ss.PATHS_S, n_features=ss.PATHS_F, seed=ss.PATHS_SEED)
            try:
                assert new.N == st.N and np.array_equal(new.omega, paths.omega) and np.array_equal(new.w, paths.w)
                got = new.coef()
                c = pr.coef(ss.ref_of(st)[0], new.omega, new.phase, new.w, new.eps)
                assert np.array_equal(got[:, :ss.PATHS_F], new.w)
                err = np.abs(got[:, ss.PATHS_F:] - c[:, ss.PATHS_F:])
                assert np.all(err <= 1e-6 * np.max(np.abs(c[:, ss.PATHS_F:]))), (k, float(np.max(err)))
            finally:
                new.close()
        assert pair.d.refits == 1
        paths.close()

"""
The inputs of tests/test_gpu_acquisition_sequences.py pinned on the CPU: the schedules of tests/sequence_schedules.py replayed on the host
and the six families' restatements evaluated on every state, alone -- no device.  For every schedule and step:
    (a) cond_2(R) <= N (1 + noise) / noise (test_gpu_remove.cond_of's bound, which asserts sf2 <= 1 and reads the noise off R), < 1e6
    (b) the step is VISIBLE: the restatement on the data before the step and after it, at the same points, differ somewhere by at least
        10 times the quantity's bar, in every family (sequence_schedules.VALUE_OF names the quantity: the family's value; the covariance
        pieces s2, b, c, S_pend do not depend on Y or the prior and cannot move with set_y or a prior step).  Every step of the schedules
        changes the model (add, remove, set_y, prior, k*), so "the device still used the old rows, Y, prior or k* variance" is a
        failure of the GPU test, not a pass within tolerance.  A condition on the inputs: were it missed, the inputs would change, not the 10.
    (c) float64 against long double, as far below the bars as the families' own reference tests require: the knowledge gradient's mu, s2, b
        and KG at most 0.1 of their bars (test_kg_reference.py), q-EI's composition at most 0.1 of 1e-12 scale (test_qei_reference.py),
        EHVI's sum at most 1e-12 S (test_ehvi_reference.py), the path gradients at most 1e-12 T_grad (test_paths_grad_reference.py).
        The constrained restatement and the path values have no long-double form in their own files and none here.
Smallest visibility found, as run when this file was written (ratio of the change to the bar; the assertion asks for 10):
    kg 763 (ard step 1)   qei 1.1e3 (ard step 1)   cacq 5.5e4 (svard step 2)   ehvi 198 (ard step 1)   paths 2.2e3 (svard step 3)   pgrad 4.7e3 (svard step 3)
Largest share of a bar in (c): kg b 1.2e-6, q-EI's composition 4.2e-5; EHVI's sum 6.2e-16 S; the path gradients 3.6e-16 T_grad.
"""
import numpy as np
import pytest

import ehvi_reference as er
import kg_reference as kr
import paths_grad_reference as pg
import paths_reference as pr
import qei_reference as qr
import sequence_schedules as ss
from test_ehvi_reference import sum_long

STEPS = [(name, k) for name in sorted(ss.SCHEDULES) for k in range(1, len(ss.SCHEDULES[name]["steps"]) + 1)]
LD = np.longdouble


def test_schedules_sit_on_the_edges_they_are_meant_for():
    from ibo_amd.gaussianprocess import GaussianProcess
    assert (GaussianProcess.EXTEND_MAX, GaussianProcess.REMOVE_MAX) == (ss.EXTEND_MAX, ss.REMOVE_MAX)
    sizes = {name: [(s.N, s.Npad) for s in ss.replay(name)] for name in ss.SCHEDULES}
    assert sizes["ard"] == [(62, 64), (63, 64), (64, 64), (65, 128), (64, 128), (62, 128), (62, 128), (62, 128), (62, 128), (62, 128),
                            (62, 128), (65, 128), (62, 64)]
    assert sizes["m5"] == [(31, 64), (32, 64), (33, 64), (32, 64), (30, 64), (30, 64), (30, 64), (47, 64), (46, 64)]
    assert sizes["svard"] == [(70, 128), (71, 128), (69, 128), (69, 128), (70, 128)]
    assert [s.pk for s in ss.replay("ard")][6:9] == [0, 1, 2] and [s.pk for s in ss.replay("m5")][5:7] == [1, 0]
    assert [s.kc for s in ss.replay("ard")][8:11] == [1.0, ss.KSTAR_SCALE, 1.0]
    for name, sch in ss.SCHEDULES.items():
        refits = [k for k, (_, _, refit) in enumerate(sch["steps"], 1) if refit]
        assert refits == {"ard": [3, 12], "m5": [7], "svard": []}[name]
        # the partner has the driven model's dimension and, at every step, another row count or another padding
        for k in range(len(sch["steps"]) + 1):
            p, s = ss.partner_at(name, k), ss.replay(name)[k]
            assert p.D == s.D and (p.N, p.Npad) != (s.N, s.Npad)


@pytest.mark.parametrize("name,k", STEPS)
def test_cond_bound(name, k):
    for st in (ss.replay(name)[k], ss.partner_at(name, k)) + ((ss.replay(name)[0],) if k == 1 else ()):
        c = ss.cond_bound(st)
        assert c <= st.N * (1 + ss.NOISE) / ss.NOISE * (1 + 1e-12) and c < 1e6, (name, k, c)


@pytest.mark.parametrize("name,k", STEPS)
def test_every_changing_step_is_visible(name, k):
    before, after, partner = ss.replay(name)[k - 1], ss.replay(name)[k], ss.partner_at(name, k)
    op = ss.SCHEDULES[name]["steps"][k - 1][0]
    assert op in ("add", "rm", "set_y", "prior", "kstar")
    pts = ss.points(after)
    r0, r1 = ss.restate(before, pts, partner), ss.restate(after, pts, partner)
    seen = {}
    for key, (v1, bar) in r1.items():
        v0 = r0[key][0]
        if v0.shape == v1.shape:                           # (the kernel weights of the paths are one per model row)
            seen[key] = float(np.max(np.abs(v1 - v0) / bar))
    print("%s step %d (%s): " % (name, k, op) + "  ".join("%s %.3g" % (f, seen[ss.VALUE_OF[f]]) for f in ss.FAMILIES))
    for f in ss.FAMILIES:
        assert seen[ss.VALUE_OF[f]] >= 10.0, (name, k, op, f, seen[ss.VALUE_OF[f]])
    if op in ("add", "rm", "kstar"):                       # what reads W and k* alone moves too
        for key in ("kg/ws1/s2", "kg/ws1/b", "qei/c", "qei/S_pend"):
            assert seen[key] >= 10.0, (name, k, op, key, seen[key])


@pytest.mark.parametrize("name,k", STEPS)
def test_float64_against_long_double(name, k):
    assert np.finfo(LD).eps < 1e-18, "long double is float64 here: the restatements have nothing more precise to be measured against"
    st, partner = ss.replay(name)[k], ss.partner_at(name, k)
    pts = ss.points(st)
    ref, sf2k = ss.ref_of(st)
    share = {}
    for ws in (1, 0):
        s = kr.kg(ref, pts.A, pts.Q, bool(ws), sf2k=sf2k)
        t = kr.kg(ref, pts.A, pts.Q, bool(ws), sf2k=sf2k, dtype=LD)
        share["kg mu"] = max(float(np.max(np.abs(s["mu_ref"] - t["mu_ref"]) / kr.tol_mu(s["mu_ref"]))),
                             float(np.max(np.abs(s["mu"] - t["mu"]) / kr.tol_mu(s["mu"]))), share.get("kg mu", 0.0))
        share["kg s2"] = max(float(np.max(np.abs(s["s2"] - t["s2"]) / (1e-6 * s["s2"]))), share.get("kg s2", 0.0))
        share["kg b"] = max(float(np.max(np.abs(s["b"] - t["b"]) / kr.tol_b(s, ref.sf2, ref.noise))), share.get("kg b", 0.0))
        share["kg kg"] = max(float(np.max(np.abs(s["kg"] - t["kg"]) / kr.tol_kg(s, ref.sf2, ref.noise, ws))), share.get("kg kg", 0.0))
    tq = float(np.max(st.Y)) + qr.XI
    w = qr.qei(ref, pts.P, pts.Q, pts.Z, tq, sf2k=sf2k)
    v, scale = qr.compose(w["mu_pend"], w["S_pend"], w["mu"], w["s2"], w["c"], pts.Z, tq)
    vl, _ = qr.compose(w["mu_pend"], w["S_pend"], w["mu"], w["s2"], w["c"], pts.Z, tq, dtype=LD)
    share["qei compose"] = float(np.max(np.abs(v - vl) / (1e-12 * scale)))
    share["qei routes"] = float(np.max(np.abs(v - w["qei"]) / (1e-12 * scale)))
    print("%s step %d: shares of the GPU bars: " % (name, k) + ", ".join("%s %.2g" % kv for kv in sorted(share.items())))
    assert max(share.values()) <= 0.1, share
    # EHVI: the walk in 80 bits on the restated posteriors of both pairings
    mo = ss.cr.Model(ref, sf2k=sf2k)
    pref, psf2k = ss.ref_of(partner)
    mp = ss.cr.Model(pref, sf2k=psf2k)
    (mu1, s21), (mu2, s22) = ss.cr.posterior(mo, pts.Q, 1e-8), ss.cr.posterior(mp, pts.Q, 1e-8)
    worst = 0.0
    for n in ss.FRONTS:
        for m2, v2 in ((mu2, s22), (mu1, s21)):
            r = er.from_posterior(mu1, s21, m2, v2, pts.fronts[n], ss.EHVI_REF, ss.gr.ERF_LIBM)
            err = np.abs(r["val"].astype(LD) - sum_long(mu1, s21, m2, v2, pts.fronts[n], ss.EHVI_REF, ss.gr.ERF_LIBM)).astype(float)
            worst = max(worst, float(np.max(err / r["S"])))
            assert np.all(err <= 1e-12 * r["S"]), (name, k, n)
    # the path gradients
    omega, phase, wts, eps = ss.draws(st)
    rk = ss.paths_ref(ref, sf2k)
    c = pr.coef(rk, omega, phase, wts, eps)
    g64, gld = pg.grads(rk, omega, phase, c, pts.Q), pg.grads(rk, omega, phase, c, pts.Q, dtype=LD)
    T = pg.grad_scale(rk, omega, phase, c, pts.Q)
    err = np.abs(gld - g64).astype(float)
    print("%s step %d: EHVI sum %.2g S, path gradients %.2g T_grad" % (name, k, worst, float(np.max(err / T))))
    assert gld.dtype == LD and np.all(T > 0) and np.all(err <= 1e-12 * T)

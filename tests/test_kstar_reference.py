"""
The k* probe's reference checked without a GPU (tests/kstar_reference.py): the probe model's factor is exact, the grids cover what they
claim, the candidates realise them, the restated s2_exp / exp_fast stay within HALF of every bar over every grid, the table the library
builds is 2^(j/2048) correctly rounded, and the epilogue's and the 2 x 2 likelihood's closed forms agree with independent evaluations.
"""
import mpmath as mp
import numpy as np
import pytest

import kstar_reference as kr

LD = np.longdouble
FAMS = {"se": kr.SE, "m3": kr.M3, "m5": kr.M5}


def grid_points(D, kind="iso", full=True):
    g = kr.probe_grid(kr.SE, D, kind, full)
    return g["y"], g["C"], g["ell"], g["z"], g["zlo"]


def truth(fam, D, kind, full):
    g = kr.probe_grid(fam, D, kind, full)
    return g["y"], g["C"], g["ell"], g["z"], g["m"]


def test_probe_model_factor_is_exact():
    assert kr.probe_factor() == (kr.PROBE_L, kr.PROBE_W, kr.PROBE_ALPHA) == (2.0, 0.5, 1.0)
    # s2 next to mu = k*: 4 - mu^2 / 4, clipped
    assert np.array_equal(kr.probe_s2([0.0, 1.0, 2.0, 4.0, 1e6], 1e-8), [4.0, 3.75, 3.0, 1e-8, 1e-8])


def test_table_is_correctly_rounded():
    """the C library's exp2(j / 2048.0), which csrc/abi_sweep.hip stores, is 2^(j/2048) correctly rounded for every j"""
    assert np.array_equal(kr.s2_table(), kr.s2_table_exact())


def test_grids_cover_what_they_claim():
    g = kr.exponent_grids()
    assert all(np.all(v <= 0) for v in g.values())
    # every table index twice (n = -j and -j - 2048) at the centre and near both ends of the reduction interval |r| <= ln2 / 4096 = 1.69e-4
    n = np.rint(g["table"] * kr.S2_C["inv"])
    r = g["table"] - n * kr.S2_C["ln2_2048"]
    for lo, hi in ((-1.65e-4, -1.55e-4), (-1e-9, 1e-9), (1.55e-4, 1.65e-4)):
        count = np.bincount(n[(r >= lo) & (r <= hi)].astype(np.int64) & 2047, minlength=2048)
        if lo > 0:
            count[0] += 1                        # y = +1.6e-4 needs sf2 > 1: index 0 meets its upper end once here
        assert np.all(count >= 2), lo
    # ... and under sf2 = 1e6 / 1e-6 (the argument moved by +-13.8, the offsets by a fraction of a step) every index at least five times again
    for sf2 in (1e6, 1e-6):
        n = np.rint((g["table"] + np.log(sf2)) * kr.S2_C["inv"])
        assert np.all(np.bincount(n.astype(np.int64) & 2047, minlength=2048) >= 5), sf2
    # positive exponents through sf2 = 1e6, the negative-n index wrap at sf2 = 1 and 1e-6
    assert np.all(np.rint((g["table"] + np.log(1e6)) * kr.S2_C["inv"]) > 0) and np.sum(np.rint(g["table"] * kr.S2_C["inv"]) < 0) >= 12280
    assert g["logrun"].max() >= -1e-299 and g["logrun"].min() <= -744.9
    assert g["edge"].min() < -745 and g["far"].min() == -kr.PULL_IN / 2 and g["beyond"].max() < -kr.PULL_IN / 2
    assert np.any((g["edge"] < -708) & (g["edge"] > -708.39))            # between exp_fast's clamp and the smallest normal number


@pytest.mark.parametrize("D,kind", [(1, "iso"), (4, "ard"), (5, "iso"), (17, "ard"), (32, "iso"), (33, "ard"), (64, "iso")])
def test_candidates_realise_the_grid(D, kind):
    y, C, ell, zhi, zlo = grid_points(D, kind, full=(D == 1))
    z = -2 * y
    with np.errstate(divide="ignore", invalid="ignore"):
        rel = np.where(z > 0, np.abs(zhi - z) / z, zhi)
    assert rel.max() <= 3 * kr.EPS, rel.max()                            # the last axis' square root and the remainder's rounding
    ellD = np.broadcast_to(ell, (D,))
    assert np.array_equal((C / ellD) * ellD, C)
    if D > 1:
        # all axes but the last: squares and every partial sum exact
        Ct = C / ellD
        s = np.zeros(len(C))
        for d in range(D - 1):
            p, e = kr.two_prod(Ct[:, d], Ct[:, d])
            s, t = kr.two_sum(s, p)
            assert not np.any(e) and not np.any(t)


CASES = [(routine, fam, sf2, D, kind)
         for routine in ("s2", "fast-dot", "fast-diff")
         for fam, sf2, D, kind in (("se", 1.0, 1, "iso"), ("se", 1e6, 1, "iso"), ("se", 1e-6, 4, "ard"), ("se", 1.0, 32, "ard"),
                                   ("m3", 1.0, 1, "iso"), ("m3", 1e6, 5, "iso"), ("m5", 1.0, 1, "iso"), ("m5", 1e-6, 17, "iso"))]


@pytest.mark.parametrize("routine,fam,sf2,D,kind", CASES)
def test_restatements_stay_within_half_of_every_bar(routine, fam, sf2, D, kind):
    """over every grid; for the Matern kernels also with sqrt_fast's stated 2e-16 put on the square root, either sign"""
    f = FAMS[fam]
    y, C, ell, z, m = truth(f, D, kind, D == 1)
    want = m * LD(sf2)
    for serr in ((0.0,) if f == kr.SE else (0.0, 2e-16, -2e-16)):
        got = kr.kstar_restated(routine, f, C, ell, sf2, sqrt_err=serr)
        if routine == "s2":
            # beyond the pull-in radius the dot form answers exactly 0 (and the truth is far below any double)
            far = z > kr.PULL_IN
            assert np.any(far) and np.all(got[far] == 0.0) and np.all(want[far] < LD("1e-500"))
        bad, worst = kr.violations(got, want, kr.bar_fast(f, z, sf2) / 2, f, z, sf2)
        print("%s %s sf2=%g D=%d sqrt_err=%g: worst ratio to HALF the bar %.3f" % (routine, fam, sf2, D, serr, worst))
        assert len(bad) == 0, (worst, y[bad][:5], got[bad][:5], want[bad][:5])


def test_routine_bound_of_the_bar_text():
    """the two routines alone, exact argument: relative error <= 6e-16 + 3.4e-17 |y| on every grid point where the result is a normal number"""
    g = kr.exponent_grids()
    for shift in (0.0, float(np.log(1e6)), float(np.log(1e-6))):
        y = np.concatenate([g["table"], g["logrun"], g["edge"]]) + shift
        with mp.workprec(160):
            want = np.array([kr._mp_to_ld(mp.exp(mp.mpf(float(v)))) for v in y])
        for name, f, lo in (("s2_exp", kr.s2_exp, -708.39), ("exp_fast", kr.exp_fast, -708.0)):
            sel = y >= lo
            rel = (np.abs(LD(1) * f(y[sel]) - want[sel]) / want[sel]).astype(np.float64)
            ratio = rel / (6e-16 + 3.4e-17 * np.abs(y[sel]))
            small = np.abs(y[sel]) < 10
            print("%s shift %.3g: worst relative error %.3g for |y| < 10, worst ratio to 6e-16 + 3.4e-17 |y| %.3f" % (name, shift, rel[small].max() if small.any() else 0.0, ratio.max()))
            assert ratio.max() <= 1.0


def test_library_chain_within_half_its_bar():
    """z by wsqdist_dev's operations and a one-ulp exp / correctly rounded sqrt (NumPy's) stay within half of 4 eps (1 + |y|)"""
    for fam, D, kind in (("se", 4, "ard"), ("m3", 1, "iso"), ("m5", 17, "iso")):
        f = FAMS[fam]
        y, C, ell, z, m = truth(f, D, kind, D == 1)
        w = 1.0 / (np.broadcast_to(ell, (D,)) ** 2)
        zz = np.zeros(len(C))
        for d in range(D):
            zz = kr.fma(w[d] * C[:, d], C[:, d], zz)
        with np.errstate(under="ignore"):
            if f == kr.SE:
                got = 1.0 * np.exp(-0.5 * zz)
            else:
                r = np.sqrt(kr.NU[f] * zz)
                got = 1.0 * ((1.0 + r) if f == kr.M3 else (1.0 + r + r * r * (1.0 / 3.0))) * np.exp(-r)
        bad, worst = kr.violations(got, m, kr.bar_lib(f, z) / 2, f, z, 1.0, lib=True)
        print("library chain %s D=%d: worst ratio to half the bar %.3f" % (fam, D, worst))
        assert len(bad) == 0


def test_derivative_of_the_map():
    """kernel_dmap against a central difference of kernel_map in long double"""
    z = np.array([0.03, 0.5, 2.0, 9.0, 40.0])
    h = 1e-7 * z
    for f in (kr.SE, kr.M3, kr.M5):
        d = kr.kernel_dmap(f, z, np.zeros(5))
        num = (kr.kernel_map(f, z + h, np.zeros(5)) - kr.kernel_map(f, z - h, np.zeros(5))) / (LD(2) * ((z + h) - (z - h)) / 2)
        assert np.all(np.abs(d - num) <= 1e-9 * np.abs(d)), (f, d, num)


def test_acquisition_truth_and_bar():
    import math
    mu, s2 = 0.75, 3.859375
    sg = math.sqrt(s2)
    for erf_mode in (0, 1):
        ei, yd, s = kr.acq_truth(0, erf_mode, mu, s2, mu, 0.0)                # Z = 0: EI = sigma phi(0)
        assert yd == 0.0 and abs(float(ei) - sg * (0.3989422804014327 if erf_mode == 0 else 0.398942)) <= 1e-15
        z = np.r_[np.arange(-40, 40.25, 0.25), -1e-8, 1e-8, 0.0]
        ymax = mu - 0.01 - z * sg
        pi, _, _ = kr.acq_truth(1, erf_mode, mu, s2, ymax, 0.01)
        ei, yd, s = kr.acq_truth(0, erf_mode, mu, s2, ymax, 0.01)
        assert np.all(pi >= 0) and np.all(pi <= 1) and np.all(np.isfinite(ei.astype(np.float64)))
        if erf_mode == 0:
            ref_pi = np.array([0.5 * math.erfc(-v / math.sqrt(2)) for v in z])
            assert np.max(np.abs(pi.astype(np.float64) - ref_pi)) <= 1e-13    # (an independent erfc; z itself is rebuilt from a rounded ymax)
        else:
            ref_pi = np.array([0.5 * math.erfc(-v / math.sqrt(2)) for v in z])
            assert np.max(np.abs(pi.astype(np.float64) - ref_pi)) < 2e-6      # the fit's 1.2e-7 and the truncated 1 / sqrt 2
        bar = kr.acq_bar(0, erf_mode, yd, s)
        assert np.all(bar >= 8 * kr.EPS * sg) and np.all(bar <= 16 * kr.EPS * (yd + s + 1))
    u, yd, s = kr.acq_truth(2, 0, mu, s2, 0.0, 2.5)
    assert abs(float(u) - (mu + 2.5 * sg)) <= 1e-15


def test_two_point_likelihood_closed_form():
    """nlml_2x2 against the definition through a 2 x 2 solve and determinant in long double; its derivative against a difference"""
    for k, noise in ((0.0, 0.1), (0.3, 0.1), (0.999, 1e-3), (1e-200, 0.5)):
        a = LD(1) + LD(noise)
        det = a * a - LD(k) * LD(k)
        yKy = (a * 2 + 2 * LD(k)) / det                                 # (1, -1) K^-1 (1, -1)^T
        want = yKy / 2 + np.log(det) / 2 + np.log(2 * kr.PI_LD)
        v, dv = kr.nlml_2x2(k, noise)
        assert abs(v - want) <= 1e-17 * abs(want), (k, v, want)
        h = 1e-9
        num = (kr.nlml_2x2(k + h, noise)[0] - kr.nlml_2x2(k - h, noise)[0]) / (2 * LD(h))
        assert abs(abs(num) - dv) <= 1e-6 * (1 + dv)

"""
The NumPy restatement of the knowledge gradient (tests/kg_reference.py, the yardstick of tests/test_gpu_knowledge_gradient.py)
pinned three ways: its expected maximum against piecewise quadrature and against the pair scan the ABI defines, its slopes b against
the oracle (a refit with the fantasised observation moves every reference mean by b_a z), and the whole against its own long-double
evaluation.  CPU only.
"""
import ctypes
import os
import re

import numpy as np
import pytest
from scipy.integrate import quad

from oracle import oracle as orc
import grad_reference as gr
import kg_reference as kr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["ibo_kg_sweep", "ibo_kg_batch", "ibo_kg_direct_max", "ibo_kg_stage_ms"]


def line_sets():
    """seeded sets of lines (mu, b): random ones, equal slopes, equal lines, a single line, all slopes zero, near-identical lines"""
    rs = np.random.RandomState(17)
    sets = []
    for n in (2, 3, 5, 8, 13):
        for _ in range(4):
            sets.append((rs.randn(n), rs.randn(n) * rs.choice([.01, .3, 2.0])))
    mu, b = rs.randn(6), rs.randn(6)
    b[3] = b[1]; b[5] = b[1]                                  # equal slopes, different heights
    sets.append((mu, b))
    mu, b = rs.randn(7), rs.randn(7)
    mu[4], b[4] = mu[2], b[2]; mu[6], b[6] = mu[2], b[2]      # equal lines
    sets.append((mu, b))
    sets.append((np.r_[mu, mu], np.r_[b, b]))                 # a set listed twice over
    sets.append((np.array([.7]), np.array([1.3])))            # n = 1
    sets.append((rs.randn(5), np.zeros(5)))                   # all b = 0
    sets.append((np.full(4, .25), rs.randn(4)))               # all mu equal
    mu, b = rs.randn(5), rs.randn(5)
    sets.append((np.r_[mu, mu[1] * (1 + 2e-16)], np.r_[b, b[1] * (1 - 2e-16)]))      # two nearly identical lines
    return sets


def emax_quad(mu, b):
    """E max_i (mu_i + b_i Z) - max mu by scipy.integrate.quad between consecutive pairwise crossings"""
    mu = mu - np.max(mu)
    n = len(mu)
    cuts = [-40.0, -10.0, 10.0, 40.0]                        # (the two inner ones only keep quad's first panels on the bell)
    for i in range(n):
        for j in range(i):
            if b[i] != b[j]:
                z = (mu[j] - mu[i]) / (b[i] - b[j])
                if -40 < z < 40:
                    cuts.append(z)
    cuts = np.unique(cuts)
    f = lambda z: np.max(mu + b * z) * np.exp(-z * z / 2) / np.sqrt(2 * np.pi)
    return sum(quad(f, lo, hi, epsabs=0, epsrel=2e-14, limit=200)[0] for lo, hi in zip(cuts[:-1], cuts[1:]))


def emax_pairs(mu, b):
    """the pair scan of ibo_abi.h, the device's algorithm, a line at a time"""
    mu = np.asarray(mu, dtype=float) - np.max(mu)
    n = len(mu)
    total = 0.0
    for i in range(n):
        lo, hi, out = -np.inf, np.inf, False
        for j in range(n):
            if b[j] < b[i]:
                lo = max(lo, (mu[j] - mu[i]) / (b[i] - b[j]))
            elif b[j] > b[i]:
                hi = min(hi, (mu[j] - mu[i]) / (b[i] - b[j]))
            else:
                out = out or mu[j] > mu[i] or (mu[j] == mu[i] and j < i)
        if not out and lo < hi:
            (Pl, Ph), (pl, ph) = kr._cdf_pdf(np.array([lo, hi]), np.float64)
            total += mu[i] * (Ph - Pl) + b[i] * (pl - ph)
    return total


@pytest.mark.filterwarnings("ignore::scipy.integrate.IntegrationWarning")      # (quad asked for more than it can certify: the bar below is the check)
def test_envelope_against_quadrature_and_the_pair_scan():
    worst_q = worst_p = 0.0
    for mu, b in line_sets():
        v, scale = kr.emax(mu, b)
        worst_q = max(worst_q, abs(v - emax_quad(mu, b)) / max(scale, 1e-300))
        worst_p = max(worst_p, abs(v - emax_pairs(mu, b)) / max(scale, 1e-300))
        assert v >= -1e-15 * scale
    print("envelope against quadrature: worst %.3g of scale; against the pair scan: %.3g" % (worst_q, worst_p))
    assert worst_q <= 1e-13 and worst_p <= 1e-13
    assert kr.emax([.7], [1.3])[0] == 0.0 and kr.emax(np.arange(5.0), np.zeros(5))[0] == 0.0


def test_random_sets_with_ties_against_the_pair_scan():
    rs = np.random.RandomState(3)
    worst = 0.0
    for t in range(300):
        n = rs.randint(1, 40)
        mu = np.round(rs.randn(n), rs.choice([1, 3, 15])); b = np.round(rs.randn(n) * rs.choice([.05, 1.0]), rs.choice([1, 3, 15]))
        v, scale = kr.emax(mu, b)
        worst = max(worst, abs(v - emax_pairs(mu, b)) / max(scale, 1e-300))
    print("300 random sets with ties and duplicated slopes: worst %.3g of scale" % worst)
    assert worst <= 1e-13


@pytest.mark.parametrize("kind,hyper", [("ard", [.3, .5, .4]), ("sviso", [.4, .8]), ("m3", [.5, .95]), ("m5", [.5, .9])])
def test_slopes_against_a_refit_of_the_oracle(kind, hyper):
    from conftest import synth
    X, Y = synth(5, 30, 3)
    fam, w, sf2 = gr.kernel_spec(kind, hyper, 3)
    ref = gr.RefGP(X, Y, .1, fam, w, sf2)
    ogp = orc.GP(orc.Kern(kind, hyper), X, Y, noise=.1)
    rs = np.random.RandomState(9)
    A = np.r_[rs.rand(9, 3), X[:3]]
    Q = np.r_[rs.rand(4, 3), X[4:5] + 1e-3]
    s = kr.slopes(ref, A, Q)
    mu0, _ = ogp.posteriors(A)
    np.testing.assert_allclose(s["mu_ref"], mu0, rtol=0, atol=1e-10)
    mq, s2q = ogp.posteriors(Q)
    np.testing.assert_allclose(s["mu"], mq, rtol=0, atol=1e-10)
    np.testing.assert_allclose(s["s2"], s2q, rtol=1e-10)
    for j in range(len(Q)):
        for z in (-2.0, -.5, 0.0, 1.0, 2.0):
            o2 = orc.GP(orc.Kern(kind, hyper), np.r_[X, Q[j:j + 1]], np.r_[Y, [mq[j] + np.sqrt(s2q[j]) * z]], noise=.1)
            mu1, _ = o2.posteriors(A)
            np.testing.assert_allclose(mu1, mu0 + s["b"][j] * z, rtol=0, atol=1e-10)


def test_own_error_is_far_below_the_gpu_bars():
    """float64 against long double on all of the GPU test's cases: every gap as a share of the GPU test's bar for that quantity.  The
    cases up to 700 rows run whole; of the two 4100-row models, whose long-double residuals cost 4100^2 products per column, every
    fifth or so reference point (observations and box points alike) and every eighth candidate (near and far alike): 12 and 8."""
    import test_gpu_posterior_cov as pc
    share = dict(mu=0.0, s2=0.0, b=0.0, kg=0.0)
    for kind, D, N, n, M, prior, ws in kr.CASES:
        X, Y, hyper, p, ref = kr.case_ref(kind, D, N, prior)
        A = kr.ref_points(X, n); Q = pc.queries(X, M)
        if N > 700:
            A = A[::n // 12][:12]; Q = Q[::M // 8][:8]
            assert len(A) == 12 and len(Q) == 8
        s = kr.kg(ref, A, Q, bool(ws))
        t = kr.kg(ref, A, Q, bool(ws), dtype=np.longdouble)
        one = dict(mu=max(float(np.max(np.abs(s["mu_ref"] - t["mu_ref"]) / kr.tol_mu(s["mu_ref"]))),
                          float(np.max(np.abs(s["mu"] - t["mu"]) / kr.tol_mu(s["mu"])))),
                   s2=float(np.max(np.abs(s["s2"] - t["s2"]) / (1e-6 * s["s2"]))),
                   b=float(np.max(np.abs(s["b"] - t["b"]) / kr.tol_b(s, ref.sf2, ref.noise))),
                   kg=float(np.max(np.abs(s["kg"] - t["kg"]) / kr.tol_kg(s, ref.sf2, ref.noise, ws))))
        print((kind, D, N, n, M, prior, ws), ", ".join("%s %.2g" % kv for kv in sorted(one.items())))
        for k in share:
            share[k] = max(share[k], one[k])
    print("restatement against its long-double evaluation, worst share of the GPU bar: " +
          ", ".join("%s %.2g" % kv for kv in sorted(share.items())))
    assert max(share.values()) <= 0.1, share


def test_symbols_are_declared_exported_and_bound():
    from ibo_amd import _lib
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ibo_abi.h")).read(), flags=re.S)
    for s in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % s, txt), "%s is not declared in ibo_abi.h" % s
        assert hasattr(_lib.lib, s), "libibo_hip.so does not export %s" % s
        assert s in _lib.EXPORTED
    assert re.search(r"#define\s+IBO_KG_MAX_REF\s+1024\b", txt)
    from ibo_amd.acquisition import KnowledgeGradient, sweepKG, maximizeKG, referenceSet      # noqa: F401
    if _lib.device_count() > 0:
        return                                       # (tests/test_gpu_knowledge_gradient.py takes over where a GPU is visible)
    A = _lib.f64(np.zeros((2, 3))); out = np.empty(6); lb = _lib.f64(np.zeros(3)); ub = _lib.f64(np.ones(3))
    bv = ctypes.c_double(); bi = ctypes.c_int64()
    L = _lib.lib
    assert L.ibo_kg_sweep(None, 2, _lib.dp(A), 2, None, 1, 1e-7, 0, None, ctypes.byref(bv), ctypes.byref(bi)) == _lib.ERR_NO_DEVICE
    assert L.ibo_kg_batch(None, 2, _lib.dp(A), 2, _lib.dp(A), 1, 1e-7, _lib.dp(out), None, None, None, None) == _lib.ERR_NO_DEVICE
    assert L.ibo_kg_direct_max(None, 2, _lib.dp(A), 3, _lib.dp(lb), _lib.dp(ub), 1, 1e-7, 5, 5, 100, 0,
                               ctypes.byref(bv), _lib.dp(out), None) == _lib.ERR_NO_DEVICE

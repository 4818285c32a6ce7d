"""
The negative log marginal likelihood and its gradient (ego/gaussianprocess/trainhyper.py:47-95) restated in NumPy, for
tests/test_gpu_nlml.py; pinned to the oracle, to long double and to mpmath by tests/test_nlml_reference.py.

For an oracle.Kern, data X, Y and a noise, with A = K + noise I, B = A^-1, alpha = B y and A = L L^T:
    value  = y.alpha / 2 + sum_i log L_ii + N log(2 pi) / 2
    V      = |y.alpha / 2| + sum_i |log L_ii| + N log(2 pi) / 2              (the scale of the value's tolerance)
    grad_h = T1_h - T2_h,   T1_h = sum_ab B_ab dK_h,ab / 2,   T2_h = alpha^T dK_h alpha / 2
    G_h    = |T1_h| + |T2_h|                                                   (the scale of component h's tolerance)
with dK_h = oracle.Kern.derivative(X, h), quirks included (Matern-3/2 on the unscaled distance), or, for a raw derivative spec
(modes, dims), the matrix csrc/ibo_common.h documents for GradSpec's modes (spec_derivative).  K and dK_h are the oracle's float64
matrices, taken as exact.  Two precisions: float64 (B and log det from the Cholesky factor) and np.longdouble (loo_reference.inverse:
the float64 inverse refined by Newton steps carried in long double, accepted only if one further step moves B by less than
newton_bar(C) = max(1e-16, 2^-64 C) of its largest entry -- asserted; log det from a column Cholesky carried in long double).  1e-16 is the
check as it was asked for; a step evaluated in long double cannot repeat itself more closely than its own rounding, 2^-64 |A| |B| ~ 2^-64 C of
B (measured: 0.01 to 0.3 of that on the ill-conditioned cases), which is 5e-5 of the bars' 1e-15 C.  Every result comes with cond_2(A).

Bars (C: the reference's cond_2):   |v - value| <= 1e-15 max(C, 1e6) V      |g_h - grad_h| <= 1e-15 max(C, 1e6) G_h, every h separately
and two tiers, asserted from the reference before a device result is looked at: C <= 1e6, and 1e7 <= C <= 2e10.
"""
import numpy as np

import loo_reference as lr
from oracle import oracle as orc

HALF_LOG_2PI = lr.HALF_LOG_2PI


def newton_bar(cond):
    """how far one further Newton step may move the long-double inverse, relative to its largest entry"""
    return max(1e-16, 2.0 ** -64 * float(cond))


WELL, ILL = "well", "ill"
TIERS = {WELL: (0.0, 1e6), ILL: (1e7, 2e10)}


def bar_factor(cond):
    """the bars' factor in front of V and G_h"""
    return 1e-15 * max(float(cond), 1e6)


def assert_tier(cond, tier, what=""):
    lo, hi = TIERS[tier]
    assert lo <= cond <= hi, "%s: cond_2 = %.3g is outside the %s-conditioned tier [%g, %g]" % (what, cond, tier, lo, hi)


def cholesky_ld(A):
    """the lower Cholesky factor of A, column by column in long double"""
    L = np.array(A, dtype=np.longdouble)
    N = len(L)
    for j in range(N):
        if j:
            L[j:, j] -= L[j:, :j] @ L[j, :j]
        if not L[j, j] > 0:
            raise np.linalg.LinAlgError("not positive definite in column %d" % j)
        L[j, j] = np.sqrt(L[j, j])
        L[j + 1:, j] /= L[j, j]
    return np.tril(L)


def inverse_checked(A, longdouble):
    """(B, move, cond): loo_reference.inverse; in long double with the relative move of one further Newton step, asserted below newton_bar"""
    B = lr.inverse(A, longdouble)
    cond = lr.cond2(A, B)
    if not longdouble:
        return B, 0.0, cond
    Al = np.asarray(A, dtype=np.float64).astype(np.longdouble)
    B2 = B @ (2.0 * np.eye(len(Al), dtype=np.longdouble) - Al @ B)
    B2 = 0.5 * (B2 + B2.T)
    move = float(np.max(np.abs(B2 - B)) / np.max(np.abs(B)))
    assert move < newton_bar(cond), "the long-double inverse has not converged: one more Newton step moves it by %.3g (cond %.3g)" % (move, cond)
    return B, move, cond


def spec_derivative(kern, X, mode, dim):
    """the matrix GradSpec's mode stands for (csrc/ibo_common.h), float64: 0 K w_dim u_dim^2 (SE-ARD length scale of dimension dim);
    1 K z, z = sum_d w_d u_d^2 (SE-iso length scale); 2 2 K (signal magnitude); 3 sf2 r^2 exp(-r) on the UNSCALED distance r, diagonal 0
    (Matern-3/2); 4 sf2 (5 z + (5 z)^(3/2)) exp(-sqrt(5 z)) / 3, diagonal 0 (Matern-5/2).  w_d = 1 / theta_d^2 (one theta for all d but for ARD);
    u = x_a - x_b; K and sf2 are the kernel's own."""
    X = np.asarray(X, dtype=np.float64)
    N, D = X.shape
    if not (0 <= mode <= 4 and 0 <= dim < D):
        raise ValueError("bad derivative spec (%d, %d)" % (mode, dim))
    w = 1.0 / kern.theta ** 2 if kern.ktype == orc.K_SE_ARD else np.full(D, 1.0 / kern.theta[0] ** 2)
    u2 = (X[:, None, :] - X[None, :, :]) ** 2
    if mode == 2:
        return 2.0 * kern.cov_matrix(X)
    if mode == 0:
        return kern.cov_matrix(X) * (w[dim] * u2[:, :, dim])
    z = np.sum(w * u2, axis=2)
    if mode == 1:
        return kern.cov_matrix(X) * z
    if mode == 3:
        r = np.sqrt(np.sum(u2, axis=2))
        C = kern.sf2_py * r ** 2 * np.exp(-r)
    else:
        C = kern.sf2_py * (5.0 * z + np.sqrt(5.0 * z) ** 3.0) * np.exp(-np.sqrt(5.0 * z)) / 3.0
    np.fill_diagonal(C, 0.0)
    return C


def canonical_spec(kind, D):
    """the (mode, dim) list of Kernel._ibo_grad_spec: hyper-parameter h of the kind, in order"""
    return {"ard": [(0, d) for d in range(D)], "svard": [(0, d) for d in range(D)] + [(2, 0)], "iso": [(1, 0)], "sviso": [(1, 0), (2, 0)],
            "m3": [(3, 0), (2, 0)], "m5": [(4, 0), (2, 0)]}[kind]


def nlml(kern, X, Y, noise, nhyper=0, longdouble=False, spec=None):
    """dict(value, V, quad, logdet, grad, G, T1, T2, alpha, B, cond, move).  The gradient's components are the first `nhyper`
    hyper-parameters of the kernel (oracle.Kern.derivative), or, with spec = [(mode, dim), ...], the matrices of spec_derivative."""
    dt = np.longdouble if longdouble else np.float64
    X = np.asarray(X, dtype=np.float64)
    N = len(X)
    A = kern.cov_matrix(X) + noise * np.eye(N)
    B, move, cond = inverse_checked(A, longdouble)
    y = np.asarray(Y, dtype=np.float64).astype(dt)
    al = B @ y
    logL = np.log(np.diag(cholesky_ld(A))) if longdouble else np.log(np.diag(np.linalg.cholesky(A)))
    quad = 0.5 * (y @ al)
    const = dt(N) * dt(HALF_LOG_2PI)
    res = dict(value=quad + logL.sum() + const, V=np.abs(quad) + np.abs(logL).sum() + const, quad=quad, logdet=logL.sum(),
               alpha=al, B=B, cond=cond, move=move)
    dKs = [kern.derivative(X, h) for h in range(nhyper)] if spec is None else [spec_derivative(kern, X, m, d) for m, d in spec]
    T1 = np.zeros(len(dKs), dtype=dt); T2 = np.zeros(len(dKs), dtype=dt)
    for h, dK in enumerate(dKs):
        dK = np.asarray(dK, dtype=np.float64).astype(dt)
        T1[h] = 0.5 * np.sum(B * dK)
        T2[h] = 0.5 * (al @ (dK @ al))
    res["T1"], res["T2"], res["grad"], res["G"] = T1, T2, T1 - T2, np.abs(T1) + np.abs(T2)
    return res


def over(err, bar):
    """err / bar, elementwise, with 0 / 0 = 0 (N = 1: a length scale's terms, and so its bar, are exactly 0 -- and so must the error be)"""
    err = np.atleast_1d(np.asarray(err, dtype=np.float64)); bar = np.atleast_1d(np.asarray(bar, dtype=np.float64))
    out = np.where(err == 0.0, 0.0, np.inf)
    np.divide(err, bar, out=out, where=bar > 0)
    return out


def ratios(v, g, ref):
    """(value error / its bar, every gradient component's error / its bar) of a device result against a reference"""
    f = bar_factor(ref["cond"])
    rv = float(abs(v - ref["value"]) / (f * ref["V"]))
    if g is None or not len(ref["grad"]):
        return rv, np.zeros(0)
    return rv, over(np.abs(np.asarray(g, dtype=np.float64) - ref["grad"]), f * ref["G"])


# ---- the cases of tests/test_gpu_nlml.py and tests/test_nlml_reference.py.  Data: conftest.synth(N + D, N, D) unless a case says otherwise.
KINDS = lr.KINDS
NOISE = 1e-2
BASE = {"iso": [.45], "sviso": [.45, .8], "m3": [.5, .95], "m5": [.5, .9]}


def hyper_of(kind, D):
    """length scales that grow with sqrt(D), a signal magnitude different from 1"""
    s = max(1.0, np.sqrt(D) / 2)
    ell = np.linspace(.35, .6, D) * s
    if kind == "ard":
        return list(ell)
    if kind == "svard":
        return list(ell) + [.9]
    return [h * (s if i == 0 else 1.0) for i, h in enumerate(BASE[kind])]


def case_id(c):
    return "%s-N%d-D%d" % (c[0], c[1], c[2]) + ("-noise%g" % c[3] if len(c) > 3 and c[3] != NOISE else "")


# a. (kind, N, D) at NOISE, long double: every N with two kinds or more, every kind at 63, 64 and 65, D in {1, 3, 17, 33}; 65 derivatives
# (svard, D = 64: the general kernel, LD = 65, four passes) and 34 (ard, D = 34: the first size on the general kernel)
FAMILY_CASES = [("ard", 1, 3), ("svard", 1, 1), ("m3", 1, 1), ("m5", 1, 3), ("iso", 2, 3), ("sviso", 2, 17), ("ard", 15, 17), ("m3", 15, 3),
                ("svard", 16, 3), ("m5", 16, 1), ("iso", 17, 1), ("m5", 17, 33),
                ("ard", 63, 33), ("iso", 63, 3), ("svard", 63, 17), ("sviso", 63, 1), ("m3", 63, 33), ("m5", 63, 3),
                ("ard", 64, 1), ("iso", 64, 17), ("svard", 64, 33), ("sviso", 64, 3), ("m3", 64, 17), ("m5", 64, 33),
                ("ard", 65, 3), ("iso", 65, 33), ("svard", 65, 1), ("sviso", 65, 33), ("m3", 65, 1), ("m5", 65, 17),
                ("ard", 127, 17), ("sviso", 127, 3), ("iso", 128, 33), ("m3", 128, 3), ("svard", 129, 33), ("m5", 129, 1),
                ("ard", 200, 3), ("m3", 200, 17), ("sviso", 200, 33),
                ("svard", 70, 64), ("ard", 70, 34)]
COINCIDENT_KINDS = ("m3", "m5", "ard")          # 129 rows, D = 3, row 0 copied over rows 7 and 70
# b. (kind, hyper, N, D, noise), long double, 1e7 <= cond <= 2e10
ILL_CASES = [("ard", [.5, .7], 200, 2, 1e-5), ("ard", [.5, .7], 200, 2, 1e-6), ("ard", [.5, .7], 200, 2, 1e-8),
             ("ard", [.25, .35], 200, 2, 1e-8), ("ard", [.12, .15], 200, 2, 1e-7),
             ("m5", [3., 1.2], 200, 2, 1e-7), ("m3", [3., 1.2], 200, 2, 1e-8)]
# c. float64, cond <= 1e6: wtw_kernel's last size and the first of the packed-operand product
ROUTE_CASES = [("ard", [.5, .7, .9, 1.1], N, 4, NOISE) for N in (1728, 1729)]
# d. the raw entry's data set
SPEC_CASE = ("svard", [.4, .5, .6, .7, .8, .9], 130, 5, NOISE)
SPEC_FULL = canonical_spec("svard", 5)
SPEC_LISTS = [SPEC_FULL, SPEC_FULL[::-1]] + [[s] for s in SPEC_FULL] + [[(0, 3), (0, 3), (2, 0), (0, 0)], [(1, 0)]]
SPEC_OTHER = [("m3", [.5, .95], [(3, 0), (2, 0), (3, 0)]), ("m5", [.5, .9], [(2, 0), (4, 0)]), ("ard", [.4, .5, .6, .7, .8], [(2, 0), (0, 4)])]


def family_case(c):
    """(kind, hyper, X, Y, noise) of a FAMILY_CASES row"""
    from conftest import synth
    kind, N, D = c
    X, Y = synth(N + D, N, D)
    return kind, hyper_of(kind, D), X, Y, NOISE


def coincident_case(kind):
    from conftest import synth
    X, Y = synth(132, 129, 3)
    X = X.copy(); X[7] = X[0]; X[70] = X[0]
    return kind, hyper_of(kind, 3), X, Y, NOISE


def table_case(c):
    """(kind, hyper, X, Y, noise) of an ILL_CASES / ROUTE_CASES / SPEC_CASE row"""
    from conftest import synth
    kind, hyper, N, D, noise = c
    X, Y = synth(N + D, N, D)
    return kind, list(hyper), X, Y, noise


def closed_form_n1(kind, hyper, Y, noise):
    """(value, grad, G) for one observation: A = sf2 + noise; every length scale's derivative is 0, the signal magnitude's is dA = 2 sf2,
    its two terms sf2 / A and sf2 y^2 / A^2 (their sum: G)"""
    sf2 = orc.Kern(kind, hyper).sf2_py
    a = np.longdouble(sf2) + np.longdouble(noise)
    y = np.longdouble(Y[0])
    value = 0.5 * y * y / a + 0.5 * np.log(a) + np.longdouble(HALF_LOG_2PI)
    grad = np.zeros(len(hyper), dtype=np.longdouble); G = np.zeros(len(hyper), dtype=np.longdouble)
    if kind in ("svard", "sviso", "m3", "m5"):
        grad[-1] = 0.5 * (1 / a - (y / a) ** 2) * 2 * np.longdouble(sf2)
        G[-1] = 0.5 * (1 / a + (y / a) ** 2) * 2 * np.longdouble(sf2)
    return value, grad, G


_CACHE = {}


def reference(key, case, longdouble=True, nhyper=None, spec=None):
    """nlml() of a (kind, hyper, X, Y, noise) case, computed once per content (key only labels it) and left unchanged; every
    hyper-parameter unless told otherwise"""
    import hashlib
    kind, hyper, X, Y, noise = case
    dig = hashlib.blake2b(np.ascontiguousarray(X, dtype=np.float64).tobytes(), digest_size=16)
    dig.update(np.ascontiguousarray(Y, dtype=np.float64).tobytes())
    nh = len(hyper) if nhyper is None and spec is None else (nhyper or 0)
    ck = (kind, tuple(float(h) for h in hyper), float(noise), dig.digest(), bool(longdouble), nh, None if spec is None else tuple(spec))
    if ck not in _CACHE:
        _CACHE[ck] = nlml(orc.Kern(kind, hyper), X, Y, noise, nh, longdouble, spec)
    return _CACHE[ck]

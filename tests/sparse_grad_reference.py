"""
The gradient of the sparse GP's negative log marginal likelihood (ibo_sgp_nlml_grad in include/ibo_abi.h) restated in NumPy on
the pieces of sparse_reference.py, in float64 or long double, for tests/test_sparse_grad_reference.py on the CPU and
tests/test_gpu_sparse_grad.py on the device.  Nothing of the package under test is imported here.

Notation is sparse_reference's (k carries sf2, every diagonal is the constant 1, the jitter is a constant).  With K = K_uf (m x N):
    mu_i = alpha.k_i,  a_i = k_i^T A^-1 k_i,  c_i = [1 / lambda_i - ((y_i - mu_i)^2 + a_i) / lambda_i^2] / 2 = dNL/dlambda_i
    e_i  = c_i [1 - q_i > 0] (fitc),  0 (dtc),  [1 - q_i > 0] / (2 sigma^2) (vfe);  v_i = K~uu^-1 k_i
    dNL/dK, column i:  g_i = (A^-1 k_i + alpha (mu_i - y_i)) / lambda_i - 2 e_i v_i
    dNL/dK~uu off the diagonal:  S = (A^-1 + alpha alpha^T - K~uu^-1) / 2 + sum_i e_i v_i v_i^T
    dNL/dlog sigma^2 = sigma^2 (sum_i c_i - [vfe] tt / (2 sigma^4))
    with z = sum_d w_d Delta_d^2 and rho = dk/dz (SE -k/2; Matern-3/2 -(3/2) sf2 e^-r; Matern-5/2 -(5/6) sf2 (1 + r) e^-r, r = sqrt(nu z)):
    dNL/dZ_ad      = 2 w_d [sum_i g_ai rho_ai (Z_ad - X_id) + 2 sum_{b != a} S_ab rho_ab (Z_ad - Z_bd)]
    dNL/dlog l_d   = -2 w_d [sum_ai g_ai rho_ai (Z_ad - X_id)^2 + sum_{a != b} S_ab rho_ab (Z_ad - Z_bd)^2]      (one length scale: summed over d)
    dNL/dlog sf    = 2 [sum_ai g_ai k_ai + sum_{a != b} S_ab K~uu,ab]

Every component comes with the SUM OF THE MAGNITUDES OF ITS TERMS -- |A^-1 k / lambda| + |alpha r| + |2 e v| carried through |rho| and |Delta|,
the four parts of S likewise, and for the noise sigma^2 (sum (1 / lambda + ((y - mu)^2 + a) / lambda^2) / 2 + tt / (2 sigma^4)) -- and THE BAR is
    |g - ref| <= 1e-15 max(cond_2(A), cond_2(K~uu), 1e6) x that sum
(the project's form, sparse_reference.bars).  On the ill-conditioned cases the terms cancel to 1e-7 .. 1e-11 of their magnitudes: a float64
gradient is honest there at the bar, not relatively.

FLOAT64 AGAINST LONG DOUBLE, recorded by tests/test_sparse_grad_reference.py (the restatement in float64 against itself in long double):
    worst share of the bar over m1_n1, m16_n200, m64_n300_j8, m100_n300_zsub, m64_n33, m40_n500_sf2, m20_n150_d33 (dtc and vfe), m32_n400_shift:
        see WORST_SHARE_F64 (held to a tenth)
    relative error |g - g_ld| / |g_ld| (2-norm per block) on the well-conditioned cases (f <= 2e-9, and m16_n200): see REL_F64 -- the device
    gets ten times that.
"""
import numpy as np

from oracle import oracle as orc
import kstar_reference as kr
import sparse_reference as sr

LD = np.longdouble
KINDS = ("fitc", "dtc", "vfe")
KIND_CODE = {"fitc": 0, "dtc": 1, "vfe": 2}
# the float64 restatement against long double, as measured by tests/test_sparse_grad_reference.py on this formulation
WORST_SHARE_F64 = 0.1           # the project's rule: a tenth of the bar
# The well-conditioned cases: every case of sparse_reference.CASES with f <= 2e-9 (cond_2 within twice the floor 1e6 of the bar's factor),
# each under the objectives the device test runs it with, and m16_n200 (f = 1.2e-8), the case this figure was first taken on.
# The figure is |g - g_ld| / |g_ld| (2-norm per block: hyper / noise / Z) of the float64 restatement, and it is taken as the WORST OVER FIVE
# ORDERS OF THE OBSERVATIONS -- the case's own and the permutations RandomState(0 .. 3) --, rounded UP to one digit.  Why not the one order:
# at these condition numbers the error is the accumulated rounding of sums over N m terms, and one order is one draw of it.  On m63_n1000
# the hyper block gives 4.97e-15 in the case's own order and 5.58e-14, 4.35e-14, 1.37e-14, 5.26e-14 under the four permutations -- the same
# mathematical problem, the same algorithm; ten times the luckiest draw is no bound on any other summation order, the device's among them.
# (m16_n200 does not move: there the conditioning of the factors decides, not the order of the sums.)  Measured, worst of five:
#   m16_n200 fitc 1.55e-9 / 4.70e-10 / 8.78e-10      m63_n1000 fitc 5.58e-14 / 2.11e-14 / 1.89e-12      m64_n31 dtc 1.83e-13 / 1.04e-13 / 8.29e-13
#   m40_n500_sf2 fitc 1.59e-13 / 8.20e-14 / 3.82e-12      m20_n150_d33 dtc 2.25e-10 / 2.33e-14 / 3.25e-12, vfe 3.05e-13 / 1.60e-14 / 3.12e-12
#   m130_n2100 fitc 2.07e-13 / 9.73e-14 / 2.21e-11      m65_n1000 dtc 4.35e-11 / 7.76e-12 / 2.60e-11, vfe 5.58e-14 / 4.40e-14 / 3.14e-12
# m1_n1 (f = 1e-9) is left out: with one observation on one inducing point the hyper and Z gradients are a pure cancellation -- the float64
# restatement's relative error against long double is 1.0 -- so a relative norm says nothing there; the term-magnitude bar holds it.
REL_ORDERS = (None, 0, 1, 2, 3)     # the case's own order, then the seeds of the permutations
REL_F64 = {("m16_n200", "fitc"): {"hyper": 2e-9, "noise": 5e-10, "Z": 9e-10},
           ("m63_n1000", "fitc"): {"hyper": 6e-14, "noise": 3e-14, "Z": 2e-12},
           ("m64_n31", "dtc"): {"hyper": 2e-13, "noise": 2e-13, "Z": 9e-13},
           ("m40_n500_sf2", "fitc"): {"hyper": 2e-13, "noise": 9e-14, "Z": 4e-12},
           ("m20_n150_d33", "dtc"): {"hyper": 3e-10, "noise": 3e-14, "Z": 4e-12},
           ("m20_n150_d33", "vfe"): {"hyper": 4e-13, "noise": 2e-14, "Z": 4e-12},
           ("m130_n2100", "fitc"): {"hyper": 3e-13, "noise": 1e-13, "Z": 3e-11},
           ("m65_n1000", "dtc"): {"hyper": 5e-11, "noise": 8e-12, "Z": 3e-11},
           ("m65_n1000", "vfe"): {"hyper": 6e-14, "noise": 5e-14, "Z": 4e-12}}
REL_DEVICE_FACTOR = 10          # what the device is allowed on the same cases: ten times the recorded figure


def grad_spec(kind, D):
    """(mode, dim) per hyper-parameter, ibo_nlml_grad's: what ibo_amd's Kernel._ibo_grad_spec says for the same class"""
    return {"ard": [(0, d) for d in range(D)], "svard": [(0, d) for d in range(D)] + [(2, 0)], "iso": [(1, 0)], "sviso": [(1, 0), (2, 0)],
            "m3": [(3, 0), (2, 0)], "m5": [(4, 0), (2, 0)]}[kind]


def rho(kern, z, k, dt=np.float64):
    """dk/dz from z and k: finite at z = 0"""
    fam = sr.family(kern)
    if fam == kr.SE:
        return -k / 2
    sf2 = dt(kern.sf2_py)
    r = np.sqrt((3 if fam == kr.M3 else 5) * z)
    if fam == kr.M3:
        return -dt(3) / 2 * sf2 * np.exp(-r)
    return -dt(5) / 6 * sf2 * (1 + r) * np.exp(-r)


def gradient(kern, Z, X, Y, noise, jitter, kind, longdouble=False, indicator=None):
    """dict(value, Z, Z_abs (m x D), L, L_abs (D: dNL/dlog l_d per dimension), sf, sf_abs, noise, noise_abs, f, model).
    indicator (optional, N): [1 - q_i > 0] as GIVEN (the device's own), instead of the model's."""
    assert kind in KINDS
    dt = LD if longdouble else np.float64
    method = sr.FITC if kind == "fitc" else sr.DTC
    mdl = sr.route(kern, Z, X, Y, noise, jitter, method, longdouble)
    Z = np.asarray(Z, dtype=np.float64); X = np.asarray(X, dtype=np.float64)
    y = np.asarray(Y, dtype=np.float64).reshape(-1).astype(dt)
    m, D = Z.shape
    s2 = dt(noise)
    zf = sr.zdist(kern, Z, X, dt); K = sr.kmap(kern, zf, dt)
    zu = sr.zdist(kern, Z, Z, dt); Ku = sr.kmap(kern, zu, dt)
    Ainv = mdl["WA"].T @ mdl["WA"]; Uinv = mdl["Wu"].T @ mdl["Wu"]
    alpha = mdl["alpha"]
    lam = mdl["lam"]
    mu = alpha @ K
    P = Ainv @ K
    a = np.sum(K * P, axis=0)
    V = Uinv @ K
    ind = (dt(1) - mdl["q"] > 0) if indicator is None else np.asarray(indicator, dtype=bool)
    ind = ind.astype(dt)
    c1 = 1 / lam / 2; c2 = ((y - mu) ** 2 + a) / lam ** 2 / 2
    c = c1 - c2
    e = c * ind if kind == "fitc" else (np.zeros(len(y), dtype=dt) if kind == "dtc" else ind / (2 * s2))
    r = (mu - y) / lam
    T1 = P / lam[None, :]; T2 = alpha[:, None] * r[None, :]; T3 = 2 * e[None, :] * V
    g = T1 + T2 - T3
    gabs = np.abs(T1) + np.abs(T2) + np.abs(T3)
    S1 = Ainv / 2; S2 = np.outer(alpha, alpha) / 2; S3 = Uinv / 2; S4 = (V * e[None, :]) @ V.T
    S = S1 + S2 - S3 + S4
    Sabs = np.abs(S1) + np.abs(S2) + np.abs(S3) + (np.abs(V) * np.abs(e)[None, :]) @ np.abs(V).T
    off = 1 - np.eye(m, dtype=dt)
    S = S * off; Sabs = Sabs * off
    rf = rho(kern, zf, K, dt); ru = rho(kern, zu, Ku, dt)
    hf = g * rf; hfa = gabs * np.abs(rf); hu = S * ru; hua = Sabs * np.abs(ru)
    w = sr.weights(kern, D).astype(dt)
    gZ = np.zeros((m, D), dtype=dt); gZa = np.zeros((m, D), dtype=dt); L = np.zeros(D, dtype=dt); La = np.zeros(D, dtype=dt)
    Zl = Z.astype(dt); Xl = X.astype(dt)
    for d in range(D):
        df = Zl[:, d][:, None] - Xl[:, d][None, :]
        du = Zl[:, d][:, None] - Zl[:, d][None, :]
        gZ[:, d] = 2 * w[d] * (np.sum(hf * df, axis=1) + 2 * np.sum(hu * du, axis=1))
        gZa[:, d] = 2 * w[d] * (np.sum(hfa * np.abs(df), axis=1) + 2 * np.sum(hua * np.abs(du), axis=1))
        L[d] = -2 * w[d] * (np.sum(hf * df * df) + np.sum(hu * du * du))
        La[d] = 2 * w[d] * (np.sum(hfa * df * df) + np.sum(hua * du * du))
    sf = 2 * (np.sum(g * K) + np.sum(S * Ku))
    sfa = 2 * (np.sum(gabs * np.abs(K)) + np.sum(Sabs * np.abs(Ku)))
    vfe = kind == "vfe"
    gn = s2 * (np.sum(c) - (mdl["tt"] / (2 * s2 * s2) if vfe else 0))
    gna = s2 * (np.sum(c1) + np.sum(c2) + (mdl["tt"] / (2 * s2 * s2) if vfe else 0))
    return dict(value=mdl["vfe"] if vfe else mdl["nlml"], Z=gZ, Z_abs=gZa, L=L, L_abs=La, sf=sf, sf_abs=sfa, noise=gn, noise_abs=gna,
                f=mdl["f"], model=mdl, c=c, e=e, ind=ind)


def hyper_of(res, spec):
    """(gradient, sum of term magnitudes) per entry of a (mode, dim) list: ibo_sgp_nlml_grad's grad_hyper"""
    gh, ga = [], []
    for mode, dim in spec:
        if mode == 0:
            gh.append(res["L"][dim]); ga.append(res["L_abs"][dim])
        elif mode == 2:
            gh.append(res["sf"]); ga.append(res["sf_abs"])
        else:
            gh.append(np.sum(res["L"])); ga.append(np.sum(res["L_abs"]))
    return np.array(gh), np.array(ga)


def value_at(kind_name, loghyper, lognoise, Z, X, Y, jitter, kind, via="route"):
    """the objective in long double at (log hyper, log noise, Z): sparse_reference.route, or its dense() definition (N <= DENSE_MAX)"""
    kern = orc.Kern(kind_name, np.exp(np.asarray(loghyper, dtype=np.float64)))
    noise = float(np.exp(lognoise))
    method = sr.FITC if kind == "fitc" else sr.DTC
    if via == "route":
        mdl = sr.route(kern, Z, X, Y, noise, jitter, method, longdouble=True)
    else:
        mdl = sr.dense(kern, Z, X, Y, noise, jitter, method, np.asarray(Z)[:1])
    return mdl["vfe"] if kind == "vfe" else mdl["nlml"]


def central(fun, h):
    return (fun(+h) - fun(-h)) / (2 * LD(h))


def richardson(fun, h, scale):
    """(estimate, tolerance): central differences at h and h / 2; the tolerance is the coarser quotient's own truncation error as the two
    steps show it, |D(h) - D(h / 2)| (the finer one's is a quarter of it), plus the rounding of a difference of two long-double values of
    size `scale` over 2 (h / 2): 8 eps scale / h"""
    d1, d2 = central(fun, h), central(fun, h / 2)
    return d2, abs(d1 - d2) + 8 * float(np.finfo(LD).eps) * float(scale) / h

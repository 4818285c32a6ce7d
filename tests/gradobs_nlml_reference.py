"""
The marginal likelihood of a GP observed with gradients and its gradient (ibo_ggp_nlml_grad in include/ibo_abi.h) restated in
NumPy, for tests/test_gpu_gradobs_nlml.py; pinned to central differences of its own long-double value and to long double by
tests/test_gradobs_nlml_reference.py.

Targets t = [Y; G] interleaved point-major, P = N (D + 1).  A_nl = C + diag(noise, gnoise_1 .. gnoise_D) per point, C the derivative
covariance of gradobs_reference.blocks with ITS OWN diagonal -- sf2 on a value row, g1(0) w_d on derivative row d (gradobs_reference.matrix
puts 1 + noise on a value row whatever sf2 is; for sf2 = 1 the two are the same bits).  With A_nl = L L^T, B = A_nl^-1, alpha = B t:
    value  = t.alpha / 2 + sum_i log L_ii + P log(2 pi) / 2          V   = |t.alpha / 2| + sum_i |log L_ii| + P log(2 pi) / 2
    grad_h = sum_ab (B - alpha alpha^T)_ab dA_h,ab / 2                G_h = sum_ab |B_ab dA_h,ab| / 2 + sum_ab |alpha_a dA_h,ab alpha_b| / 2
    noise  = noise sum_{value rows} (B_ii - alpha_i^2) / 2            its scale: noise sum_{value rows} (|B_ii| + alpha_i^2) / 2
    gnoise_e likewise over the rows of d/dx_e
dA_h = dA_nl / dlog theta_h, the exact derivative (dblocks): with z = sum_d w_d u_d^2, t_d = w_d u_d and (k, g1, g2) of gradobs_reference,
    mode 0 (SE-ARD, dimension h)   dz = -2 w_h u_h^2, dt_d = -2 t_d [d = h], dw_d = -2 w_d [d = h], dk = -(g1/2) dz, dg1 = -(g2/2) dz, dg2 = -(k/2) dz
    modes 1, 3, 4 (one scale)      dz = -2 z, dt_d = -2 t_d, dw_d = -2 w_d, dk = g1 z, dg1 = g2 z, dg2 = k z (SE), 9 sf2 e^-r (1 + r) / r
                                   (Matern-3/2; 0 at r = 0, where t_d t_e = 0), 25/3 sf2 e^-r r (Matern-5/2)
    d(value, d/dx'_e) = dg1 t_e + g1 dt_e, the (d/dx_d, value) entry its negative; d(d, e) = (dg1 w_d + g1 dw_d) [d = e] - dg2 t_d t_e - g2 (dt_d t_e + t_d dt_e)
    mode 2 (signal magnitude)      dA = 2 C, diagonal included
Two precisions: float64 (numpy's Cholesky, scipy's triangular solves) and np.longdouble (gradobs_reference's column Cholesky and
substitutions).  Bars, the project's rule:  |v - value| <= 1e-15 max(cond_2, 1e6) V,  |g - grad_h| <= 1e-15 max(cond_2, 1e6) G_h.
"""
import functools

import numpy as np

import gradobs_reference as gr
from nlml_reference import bar_factor, canonical_spec, over
from oracle import oracle as orc

LD = np.longdouble
HALF_LOG_2PI = 0.5 * np.log(2 * np.pi)
LD_ROWS = 400                       # truth is long double up to here and wherever cond_2 > 1e6, float64 otherwise

# (name, oracle kind, hyper, N, D, noise, gnoise, coincident pair or None) of the cases gradobs_reference has no entry for
NEW_CASES = [
    ("ard_1x3", "ard", [0.5, 0.7, 0.6], 1, 3, 0.1, 1e-4, None),              # one point: every pair is its own
    ("iso_2x1", "iso", [0.5], 2, 1, 0.1, 1e-4, None),                        # one pair off the diagonal
    ("ard_15x3", "ard", [0.5, 0.7, 0.6], 15, 3, 0.1, 1e-4, None),            # one below the 16-point tile
    ("ard_17x3", "ard", [0.5, 0.7, 0.6], 17, 3, 0.1, 1e-4, None),            # one above: P = 68, point 16's block straddles rows 63 | 64
    ("ard_31x3", "ard", [0.5, 0.7, 0.6], 31, 3, 0.1, 1e-4, None),
    ("ard_33x3", "ard", [0.5, 0.7, 0.6], 33, 3, 0.1, 1e-4, None),            # three tiles a side
    ("svard_3x64", "svard", list(2.0 + 0.03 * np.arange(64)) + [0.9], 3, 64, 0.1, 1e-4, None),      # 65 derivatives: the ngrad limit
]
NEW_NAMES = [c[0] for c in NEW_CASES]
# the device's shapes: P = 2; 1 x 3; 2 x 1; around the 16-point tile at D = 3; P = 63, 65, 129, 153; 65 derivatives; sf2 = 0.81; low noise;
# a gnoise per dimension; a coincident pair; P = 1025; P = 2100 (the packed-operand W^T W, float64 under cond_upper <= 1e6)
DEVICE_CASES = ["se_1x1", "ard_1x3", "iso_2x1", "ard_15x3", "ard_16x3", "ard_17x3", "ard_31x3", "iso_32x3", "ard_33x3", "m3_21x2", "ard_13x4",
                "m5_43x2", "m5_9x16", "svard_3x64", "sviso_20x2", "ard_60x4", "ard_60x3_gn", "m3_10x2_twin", "ard_205x4", "ard_525x3"]
# every family, with a coincident pair for Matern-3/2, at N = 7 .. 10 and D = 2 .. 3: the central-difference cases
FD_CASES = [("ard", [0.5, 0.7, 0.6], 8, 3, None), ("svard", [0.5, 0.7, 0.9], 9, 2, None), ("iso", [0.6], 10, 2, None),
            ("sviso", [0.6, 0.9], 7, 3, None), ("m3", [0.6, 0.9], 10, 2, (2, 5)), ("m5", [0.5, 0.9], 9, 3, None)]
FD_NOISE, FD_GNOISE, FD_H = 0.05, [1e-3, 4e-3, 2e-2], 1e-3


def spec_of(kern):
    """the (mode, dim) list of the kernel's hyper-parameters, in order (Kernel._ibo_grad_spec)"""
    return canonical_spec(kern.kind, len(kern.theta) if kern.ktype == orc.K_SE_ARD else 1)


def matrix_nl(kern, X, noise, gnoise, dt=np.float64):
    """A_nl, P x P point-major: gradobs_reference.matrix with sf2 + noise on the value rows"""
    X = np.asarray(X, dtype=np.float64)
    N, D = X.shape
    A = gr.blocks(kern, X, X, dt).transpose(0, 2, 1, 3).reshape(N * (D + 1), N * (D + 1)).copy()
    w = gr.weights(kern, D).astype(dt)
    g1_0 = gr.factors(kern, dt(0), dt)[1]
    A[np.diag_indices(len(A))] = np.tile(np.concatenate([[dt(kern.sf2_py) + dt(noise)], g1_0 * w + gr.tile_gnoise(gnoise, D).astype(dt)]), N)
    return A


def dfactor2(kern, z, k, dt):
    """dg2 / dlog(the one length scale) in its finite form"""
    sf2 = dt(kern.sf2_py)
    if kern.ktype in (orc.K_SE_ARD, orc.K_SE_ISO):
        return k * z
    if kern.ktype == orc.K_MATERN3:
        r = np.sqrt(3 * z)
        with np.errstate(divide="ignore", invalid="ignore"):
            return np.where(r > 0, 9 * sf2 * np.exp(-r) * (1 + r) / np.where(r > 0, r, 1), 0).astype(dt)
    r = np.sqrt(5 * z)
    return (dt(25) / 3) * sf2 * np.exp(-r) * r


def dmatrix(kern, X, mode, dim, dt=np.float64):
    """dA_nl / dlog theta of one (mode, dim), P x P, diagonal included"""
    X = np.asarray(X, dtype=np.float64).astype(dt)
    N, D = X.shape
    if mode == 2:
        C = gr.blocks(kern, X, X, dt).transpose(0, 2, 1, 3).reshape(N * (D + 1), N * (D + 1)).copy()
        w = gr.weights(kern, D).astype(dt)
        C[np.diag_indices(len(C))] = np.tile(np.concatenate([[dt(kern.sf2_py)], gr.factors(kern, dt(0), dt)[1] * w]), N)
        return 2 * C
    w = gr.weights(kern, D).astype(dt)
    u = X[:, None, :] - X[None, :, :]
    t = w * u
    z = np.sum(w * u * u, axis=2)
    k, g1, g2 = gr.factors(kern, z, dt)
    if mode == 0:
        assert kern.ktype == orc.K_SE_ARD
        sel = np.zeros(D, dtype=dt); sel[dim] = 1
        dz = -2 * w[dim] * u[:, :, dim] ** 2
        dk, dg1, dg2 = -(g1 / 2) * dz, -(g2 / 2) * dz, -(k / 2) * dz
    else:
        sel = np.ones(D, dtype=dt)
        dk, dg1, dg2 = g1 * z, g2 * z, dfactor2(kern, z, k, dt)
    dt_ = -2 * t * sel
    dw = -2 * w * sel
    B = np.empty((N, N, D + 1, D + 1), dtype=dt)
    B[:, :, 0, 0] = dk
    B[:, :, 0, 1:] = dg1[:, :, None] * t + g1[:, :, None] * dt_
    B[:, :, 1:, 0] = -B[:, :, 0, 1:]
    tt = t[:, :, :, None] * t[:, :, None, :]
    B[:, :, 1:, 1:] = (dg1[:, :, None, None] * np.diag(w) + g1[:, :, None, None] * np.diag(dw) - dg2[:, :, None, None] * tt
                       - g2[:, :, None, None] * (dt_[:, :, :, None] * t[:, :, None, :] + t[:, :, :, None] * dt_[:, :, None, :]))
    return B.transpose(0, 2, 1, 3).reshape(N * (D + 1), N * (D + 1)).copy()


def factor(A, y, longdouble):
    """(L, alpha, B = A^-1) of A = L L^T in the precision asked for"""
    import scipy.linalg as sl
    if longdouble:
        L = gr.cholesky_ld(A)
        W = gr.forward_ld(L, np.eye(len(L), dtype=LD))
        B = W.T @ W
        return L, B @ y, B
    L = np.linalg.cholesky(A)
    W = sl.solve_triangular(L, np.eye(len(L)), lower=True)
    return L, sl.solve_triangular(L, sl.solve_triangular(L, y, lower=True), lower=True, trans="T"), W.T @ W


def value_ld(kern, X, Y, G, noise, gnoise):
    """the value alone, in long double"""
    A = matrix_nl(kern, X, noise, gnoise, LD)
    y = gr.targets(Y, G).astype(LD)
    L = gr.cholesky_ld(A)
    v = gr.forward_ld(L, y[:, None])[:, 0]
    return 0.5 * (v @ v) + np.sum(np.log(np.diag(L))) + LD(len(y)) * LD(HALF_LOG_2PI)


def nlml(kern, X, Y, G, noise, gnoise, spec=None, longdouble=False, cond=None):
    """dict(value, V, grad, G, gnoise (1 + D: the noise, then the D gradient noises), Gnoise, alpha, L, cond): the gradient's components are
    those of spec = [(mode, dim), ...] (default: the kernel's own hyper-parameters).  cond: cond_2 of the float64 A_nl unless given."""
    dt = LD if longdouble else np.float64
    X = np.asarray(X, dtype=np.float64)
    N, D = X.shape
    P = N * (D + 1)
    gn = gr.tile_gnoise(gnoise, D)
    A = matrix_nl(kern, X, noise, gn, dt)
    y = gr.targets(Y, G).astype(dt)
    L, al, B = factor(A, y, longdouble)
    logL = np.log(np.diag(L))
    quad = 0.5 * (y @ al)
    const = dt(P) * dt(HALF_LOG_2PI)
    if cond is None:
        cond = float(np.linalg.cond(matrix_nl(kern, X, noise, gn))) if longdouble else float(np.linalg.cond(A))
    res = dict(value=quad + logL.sum() + const, V=np.abs(quad) + np.abs(logL).sum() + const, alpha=al, L=L, cond=cond, N=N, D=D, P=P)
    spec = spec_of(kern) if spec is None else spec
    g = np.zeros(len(spec), dtype=dt); Gs = np.zeros(len(spec), dtype=dt)
    aa = np.abs(al)
    for h, (mode, dim) in enumerate(spec):
        dA = dmatrix(kern, X, mode, dim, dt)
        g[h] = 0.5 * np.sum(B * dA) - 0.5 * (al @ (dA @ al))
        Gs[h] = 0.5 * np.sum(np.abs(B * dA)) + 0.5 * (aa @ (np.abs(dA) @ aa))
    d = np.diag(B) - al * al
    da = np.abs(np.diag(B)) + al * al
    sc = np.concatenate([[dt(noise)], gn.astype(dt)])
    res["grad"], res["G"] = g, Gs
    res["gnoise"] = 0.5 * sc * d.reshape(N, D + 1).sum(axis=0)
    res["Gnoise"] = 0.5 * sc * da.reshape(N, D + 1).sum(axis=0)
    return res


def shares(v, g, gn, ref):
    """(value error / its bar, every component's error / its bar, every noise component's error / its bar) against a reference"""
    f = bar_factor(ref["cond"])
    rv = float(abs(v - ref["value"]) / (f * ref["V"]))
    rg = over(np.abs(np.asarray(g, dtype=LD) - ref["grad"]), f * ref["G"]) if g is not None and len(ref["grad"]) else np.zeros(0)
    rn = over(np.abs(np.asarray(gn, dtype=LD) - ref["gnoise"]), f * ref["Gnoise"]) if gn is not None else np.zeros(0)
    return rv, rg, rn


# ---------------------------------------------------------------------------- cases
def _make_case(name):
    if name not in NEW_NAMES:
        return gr.case(name)
    name, kind, hyper, N, D, noise, gnoise, twin = NEW_CASES[NEW_NAMES.index(name)]
    X = gr.points(N, D, 300 + NEW_NAMES.index(name))
    if twin is not None:
        X[twin[1]] = X[twin[0]]
    Y, G = gr.objective(X)
    for a in (X, Y, G):
        a.setflags(write=False)
    return dict(name=name, kern=orc.Kern(kind, hyper), X=X, Y=Y, G=G, noise=noise, gnoise=gr.tile_gnoise(gnoise, D))


_cached_case = functools.lru_cache(maxsize=None)(_make_case)


def case(name):
    """dict(name, kern, X, Y, G, noise, gnoise): a case of gradobs_reference's lists or of NEW_CASES"""
    return _make_case(name) if gr.is_big(name) else _cached_case(name)


def cond_upper_nl(kern, X, noise, gnoise):
    """gradobs_reference.cond_upper for A_nl: |A_nl|_inf / min(noise, min_d gnoise_d) >= cond_2(A_nl) -- A_nl is C (positive semi-definite)
    plus the diagonal (noise, gnoise_1 .. gnoise_D) per point"""
    X = np.asarray(X, dtype=np.float64)
    N, D = X.shape
    extra = np.concatenate([[float(noise)], gr.tile_gnoise(gnoise, D)])
    assert np.all(extra > 0.0)
    worst = 0.0
    for i0 in range(0, N, 64):
        rows = np.sum(np.abs(gr.blocks(kern, X[i0:i0 + 64], X)), axis=(1, 3)) + extra[None, :]
        worst = max(worst, float(np.max(rows)))
    return worst / float(np.min(extra))


@functools.lru_cache(maxsize=None)
def reference(name, spec=None):
    """the result the device is held to: long double up to LD_ROWS rows and wherever cond_2 > 1e6, float64 otherwise; a big case
    (gradobs_reference.BIG_ROWS): float64 under cond_upper_nl <= 1e6.  spec: a tuple of (mode, dim), default the kernel's own."""
    c = case(name)
    spec = None if spec is None else list(spec)
    args = (c["kern"], c["X"], c["Y"], c["G"], c["noise"], c["gnoise"])
    if gr.is_big(name):
        cu = cond_upper_nl(c["kern"], c["X"], c["noise"], c["gnoise"])
        assert cu <= 1e6, "%s is not admissible: cond_upper %.3g" % (name, cu)
        return nlml(*args, spec=spec, cond=cu)
    ref = nlml(*args, spec=spec)
    if ref["P"] <= LD_ROWS or ref["cond"] > 1e6:
        ref = nlml(*args, spec=spec, longdouble=True, cond=ref["cond"])
    return ref


# ---------------------------------------------------------------------------- difference quotients
def central(fun, h):
    return (fun(+h) - fun(-h)) / (2 * LD(h))


def richardson(fun, h):
    """(estimate, truncation): central differences at h and h / 2; the coarser quotient's own truncation error as the two steps show it,
    |D(h) - D(h / 2)| = h^2 |f'''| / 8 to leading order (the finer one's, h^2 |f'''| / 24, is a third of it)"""
    d1, d2 = central(fun, h), central(fun, h / 2)
    return d2, abs(d1 - d2)

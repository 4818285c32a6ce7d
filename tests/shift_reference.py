"""
Inputs away from the origin, for tests/test_gpu_shifted_inputs.py; pinned by tests/test_shift_reference.py.

The oracle (oracle/ibo_oracle.c, orc_cov) subtracts coordinates before it scales them.  Observations and candidates on the grid of
multiples of 2^-12 in [0, 1) moved by one integer t, |t| <= 2^20, are still exact in fp64 and so are all their differences: the
oracle then returns the SAME BITS at (X0 + t, C0 + t) as at (X0, C0).  The reference of a shifted case is therefore the reference
the suite already trusts at the unshifted data, and its bars carry over unchanged.

The device does not always subtract first.  This file restates in float64 the three ways the library forms the exponent
-z / 2 = -|x~ - c~|^2 / 2  (x~ = x / length scale):
    exact   differences of the unshifted coordinates, then the scaling          (what the oracle and the subtract-first kernels do)
    scaled  x~ and c~ of the SHIFTED coordinates, then their differences         (sweep.hip's difference form; loses |x~| 2^-53 a coordinate)
    dot     a_k + b_c + x~.c~,  a = -|x~|^2 / 2,  b = -|c~|^2 / 2                (the MFMA routes; loses |x~|^2 2^-52: hence the guards)
and from each the posterior variance at one shared factor L and the NLML, so that the error of each form is a number a test can
read: the measured-bar tests of the GPU file take 8 x these deviations.  The products are written a dimension at a time, each
multiplication and addition rounded on its own (no fused multiply-add, no BLAS).

The cases of the GPU file are listed here too (SWEEP_CASES, FAR_CASES, PULLIN_CASES, EXTEND_CASE, NLML_CASES), so that the
reference tests can check on the CPU what the GPU file will ask of them.
"""
import functools

import numpy as np
from scipy.linalg import solve_triangular

import grad_reference as gr

GRID = 4096.0                       # coordinates are multiples of 2^-12
GUARD = 2e4                         # IBO_DOT_GUARD (csrc/ibo_common.h; dot_form_ok and ibo_gp_extend in csrc/abi_fit.hip): max |x~|^2 that admits the dot-form sweeps
NLML_GUARD = 1e5                    # IBO_DOT_GUARD_NLML (ibo_nlml_grid, csrc/abi_nlml.hip): the per-dimension bound that admits the dot-form covariance pass
PULL_IN = 6e5                       # IBO_DOT_PULL_IN (csrc/ibo_common.h; s2_stage_candidates in csrc/sweep2_dev.h): |c~|^2 beyond which a candidate is pulled in
INSIDE = (0.80 * GUARD, 0.98 * GUARD)        # where the cases "inside the guard" put max |x~|^2
OUTSIDE = (1.02 * GUARD, 1.3 * GUARD)        # ... and the cases beyond it
MU_RTOL, MU_ATOL = 1e-6, 1e-9       # the suite's bar on the posterior mean (tests/test_gpu_parity.py)


def dyadic(seed, N, D):
    """(N, D) points whose coordinates are multiples of 2^-12 in [0, 1)"""
    return np.random.RandomState(seed).randint(0, int(GRID), size=(N, D)) / GRID


def targets(seed, X0):
    """the suite's synthetic targets (conftest.synth) at the UNSHIFTED points"""
    return np.sin(3 * X0.sum(1)) + 0.01 * np.random.RandomState(seed).randn(len(X0))


def scale_of(kind, hyper, D):
    """sw (D,): the reciprocal length scales of a kernel in the oracle's naming"""
    return np.sqrt(gr.kernel_spec(kind, hyper, D)[1])


def row_bound(X, sw):
    """max_i sum_d (X_id sw_d)^2 -- what dot_form_ok and ibo_gp_extend compare with the guard; sw (D,) or (T, D): the largest over the rows of sw"""
    sw = np.atleast_2d(sw)
    return max(float(np.max(np.sum((X * s) ** 2, axis=1))) for s in sw)


def dim_bound(X, sw):
    """max_theta sum_d w_d max_k X_kd^2 -- the per-dimension bound of ibo_nlml_grid (csrc/abi_nlml.hip); never below row_bound"""
    sw = np.atleast_2d(sw)
    xm = np.max(X * X, axis=0)
    return max(float(np.sum(s * s * xm)) for s in sw)


def shift_for(X0, sw, lo, hi, sign=1, bound=row_bound):
    """an integer t of the given sign, the same in every dimension, with lo <= bound(X0 + t, sw) <= hi; X0 + t is exact"""
    sw = np.atleast_2d(np.asarray(sw, dtype=float))
    mid = 0.5 * (lo + hi)
    k0 = int(np.sqrt(mid / max(float(np.sum(s * s)) for s in sw)))
    best = None
    for k in range(max(k0 - 4, 0), k0 + 6):
        t = int(sign) * k
        b = bound(X0 + t, sw)
        if lo <= b <= hi and (best is None or abs(b - mid) < abs(best[1] - mid)):
            best = (t, b)
    assert best is not None, "no integer shift puts the bound into [%g, %g]" % (lo, hi)
    t = best[0]
    assert abs(t) <= 2 ** 20 and np.array_equal((X0 + t) - t, X0)
    return t


# ----------------------------------------------------------------------------------------------- the three exponent forms
def exponent_exact(A0, B0, sw):
    """-z / 2 from the differences of the unshifted coordinates (exact on the grid), scaled afterwards"""
    z = np.zeros((len(A0), len(B0)))
    for d in range(A0.shape[1]):
        df = (A0[:, d, None] - B0[None, :, d]) * sw[d]
        z = z + df * df
    return -0.5 * z


def exponent_scaled(A, B, sw):
    """-z / 2 from coordinates scaled first, subtracted afterwards (A, B: the SHIFTED points)"""
    As, Bs = A * sw, B * sw
    z = np.zeros((len(A), len(B)))
    for d in range(A.shape[1]):
        df = As[:, d, None] - Bs[None, :, d]
        z = z + df * df
    return -0.5 * z


def exponent_dot(A, B, sw):
    """a_k + b_c + x~.c~ (A, B: the SHIFTED points); every product and sum rounded on its own"""
    As, Bs = A * sw, B * sw
    a, b = np.zeros(len(A)), np.zeros(len(B))
    dot = np.zeros((len(A), len(B)))
    for d in range(A.shape[1]):
        a = a + As[:, d] * As[:, d]
        b = b + Bs[:, d] * Bs[:, d]
        dot = dot + As[:, d, None] * Bs[None, :, d]
    return ((-0.5 * a)[:, None] + (-0.5 * b)[None, :]) + dot


def kernel_of(fam, sf2, y):
    """the covariance of one exponent y = -z / 2, as the device's s2_kstar forms it"""
    if fam == gr.FAM_SE:
        return sf2 * np.exp(y)
    z = np.maximum(-2.0 * y, 0.0)
    if fam == gr.FAM_M3:
        r = np.sqrt(3.0 * z)
        return sf2 * (1.0 + r) * np.exp(-r)
    r = np.sqrt(5.0 * z)
    return sf2 * (1.0 + r + r * r / 3.0) * np.exp(-r)


def forms(X0, C0, t, sw):
    """{'exact' | 'scaled' | 'dot': exponent matrix (N, M)} of the observations X0 + t against the points C0 + t"""
    return dict(exact=exponent_exact(X0, C0, sw), scaled=exponent_scaled(X0 + t, C0 + t, sw), dot=exponent_dot(X0 + t, C0 + t, sw))


def factor(X0, fam, sw, sf2, noise):
    """L = chol(R), R from the exact form with the model's diagonal 1 + noise"""
    R = kernel_of(fam, sf2, exponent_exact(X0, X0, sw))
    np.fill_diagonal(R, 1.0 + noise)
    return np.linalg.cholesky(R)


def s2_of(L, kstar, noise, clamp_lo=1e-8):
    v = solve_triangular(L, kstar, lower=True)
    return np.clip(1.0 + noise - np.sum(v * v, axis=0), clamp_lo, 10.0)


def s2_deviation(X0, C0, t, kind, hyper, noise):
    """{'scaled' | 'dot': the worst relative deviation of the posterior variance from the exact form's}, all at the same L"""
    D = X0.shape[1]
    fam, w, sf2 = gr.kernel_spec(kind, hyper, D)
    sw = np.sqrt(w)
    L = factor(X0, fam, sw, sf2, noise)
    y = forms(X0, C0, t, sw)
    ref = s2_of(L, kernel_of(fam, sf2, y["exact"]), noise)
    return {k: float(np.max(np.abs(s2_of(L, kernel_of(fam, sf2, y[k]), noise) - ref) / ref)) for k in ("scaled", "dot")}


def mu_deviation(X0, Y, C0, t, kind, hyper, noise):
    """{'scaled' | 'dot': the worst |mu - mu of the exact form| in units of the suite's bar MU_ATOL + MU_RTOL |mu|}, all with the same
    alpha = R^-1 Y: the mean's error is ABSOLUTE, about (error of the exponent) x sum_i |k*_i alpha_i|, and grows with the model"""
    D = X0.shape[1]
    fam, w, sf2 = gr.kernel_spec(kind, hyper, D)
    sw = np.sqrt(w)
    L = factor(X0, fam, sw, sf2, noise)
    alpha = solve_triangular(L.T, solve_triangular(L, Y, lower=True), lower=False)
    y = forms(X0, C0, t, sw)
    ref = kernel_of(fam, sf2, y["exact"]).T.dot(alpha)
    bar = MU_ATOL + MU_RTOL * np.abs(ref)
    return {k: float(np.max(np.abs(kernel_of(fam, sf2, y[k]).T.dot(alpha) - ref) / bar)) for k in ("scaled", "dot")}


def nlml_of(K, Y):
    L = np.linalg.cholesky(K)
    a = solve_triangular(L, Y, lower=True)
    return 0.5 * a.dot(a) + np.sum(np.log(np.diag(L))) + 0.5 * len(Y) * np.log(2.0 * np.pi)


def nlml_deviation(X0, Y, t, kind, hyper, noise):
    """{'scaled' | 'dot': |NLML - NLML of the exact form| / |NLML of the exact form|} with K = K(X, X) + noise I, diagonal sf2 + noise"""
    D = X0.shape[1]
    fam, w, sf2 = gr.kernel_spec(kind, hyper, D)
    sw = np.sqrt(w)
    y = forms(X0, X0, t, sw)
    out = {}
    for k in ("exact", "scaled", "dot"):
        K = kernel_of(fam, sf2, y[k])
        K = np.tril(K) + np.tril(K, -1).T                    # the factorisation reads the lower triangle
        np.fill_diagonal(K, sf2 + noise)
        out[k] = nlml_of(K, Y)
    return {k: abs(out[k] - out["exact"]) / abs(out["exact"]) for k in ("scaled", "dot")}


def measured_bar(dev, floor=0.0):
    """the bar of a dot-against-difference comparison: 8 x the emulated deviation (the MFMA's other summation order and its D + 2
    terms), never above the suite's 1e-6"""
    bar = max(floor, 8.0 * dev)
    assert bar <= 1e-6, "the emulation itself (%g) leaves no room under 1e-6" % dev
    return bar


# ----------------------------------------------------------------------------------------------- the GPU file's cases
def hyper_of(kind, D):
    """length scales that keep the posterior alive in D dimensions (and sum_d sw_d^2 small enough for an integer shift to hit a band)"""
    base = {1: .23, 3: .3, 4: .3, 5: .35, 6: .5, 16: .9, 32: 1.5}[D]
    if kind == "ard":
        return [base * (1.0 + 0.1 * (d % 3)) for d in range(D)]
    return [base] if kind == "iso" else [base * 1.5, 1.0]


def candidates(seed, X0, M):
    """(M, D) on the grid: every other one within 1/16 of an observation (variance well below the prior's), the rest anywhere;
    candidate 1 and 7 sit ON observations and the last one repeats the first (a ragged last tile with a duplicate)"""
    rs = np.random.RandomState(seed)
    N, D = X0.shape
    C = rs.randint(0, int(GRID), size=(M, D)) / GRID
    near = X0[rs.randint(0, N, size=M)] + rs.randint(-256, 257, size=(M, D)) / GRID
    C[::2] = np.clip(near, 0.0, (GRID - 1) / GRID)[::2]
    if M > 1: C[1] = X0[3 % N]
    if M > 7: C[7] = X0[5 % N]
    if M > 8: C[M - 1] = C[0]
    return C


# (name, kind, D, N, noise, sign of the shift inside the guard -- the one beyond it has the other sign)
SWEEP_CASES = [("ard_d4_n200", "ard", 4, 200, .1, 1), ("iso_d1_n200", "iso", 1, 200, 1e-3, -1),
               ("m3_d5_n1000", "m3", 5, 1000, 1e-3, 1), ("m5_d16_n1100", "m5", 16, 1100, .1, -1),
               ("ard_d32_n200", "ard", 32, 200, 1e-3, 1), ("m5_d4_n1000", "m5", 4, 1000, 1e-3, -1),
               ("iso_d16_n200", "iso", 16, 200, .1, 1), ("m3_d32_n1100", "m3", 32, 1100, .1, -1),
               ("ard_d5_n1100", "ard", 5, 1100, 1e-3, -1), ("m3_d1_n200", "m3", 1, 200, .1, 1),
               ("iso_d4_n1000", "iso", 4, 1000, .1, 1), ("m5_d5_n200", "m5", 5, 200, 1e-3, 1)]
SWEEP_M = 8300                       # the large batch; the smaller ones are prefixes of the same array
EMU_M = 600                          # the prefix the emulation (and the measured-bar comparison) covers

# (name, kind, noise, t): N = 300, D = 4 on the difference routes
FAR_CASES = [("ard_p4096", "ard", 1e-3, 4096), ("ard_m65536", "ard", .1, -65536), ("ard_p1048576", "ard", 1e-3, 1048576),
             ("m5_p4096", "m5", .1, 4096), ("m5_m65536", "m5", 1e-3, -65536), ("m5_p1048576", "m5", .1, 1048576)]

# (name, kind, D, N, noise, sign, with a mean prior)
PULLIN_CASES = [("ard", "ard", 4, 200, .1, 1, False), ("iso", "iso", 4, 200, 1e-3, -1, False), ("m3", "m3", 4, 200, .1, 1, False),
                ("m5", "m5", 4, 200, 1e-3, -1, False), ("ard_prior", "ard", 4, 200, .1, 1, True)]
PULLIN_R2 = (5.9e5, 6.1e5, 1e7, 1e12)

# (name, kind, D, N, noise): 5 theta-points for 'ard', one for the others
NLML_CASES = [("ard_n500_d3", "ard", 3, 500, 1e-2), ("ard_n1000_d6", "ard", 6, 1000, 1e-3), ("iso_n500_d3", "iso", 3, 500, 1e-3),
              ("m3_n1000_d6", "m3", 6, 1000, 1e-2), ("m5_n500_d3", "m5", 3, 500, 1e-2), ("m5_n1000_d6", "m5", 6, 1000, 1e-3)]


@functools.lru_cache(maxsize=None)
def sweep_case(name):
    """dict of one SWEEP_CASES model: X0, Y, C0 (SWEEP_M candidates), hyper, t_in / t_out (shifts on either side of the guard)"""
    _, kind, D, N, noise, sign = [c for c in SWEEP_CASES if c[0] == name][0]
    seed = 1000 + 7 * N + D
    X0 = dyadic(seed, N, D)
    hyper = hyper_of(kind, D)
    sw = scale_of(kind, hyper, D)
    return dict(kind=kind, D=D, N=N, noise=noise, hyper=hyper, sw=sw, X0=X0, Y=targets(seed + 1, X0), C0=candidates(seed + 2, X0, SWEEP_M),
                t_in=shift_for(X0, sw, *INSIDE, sign=sign), t_out=shift_for(X0, sw, *OUTSIDE, sign=-sign))


@functools.lru_cache(maxsize=None)
def sweep_case_deviation(name):
    """the emulated s2 deviations of a SWEEP_CASES model inside the guard, over the first EMU_M candidates"""
    c = sweep_case(name)
    return s2_deviation(c["X0"], c["C0"][:EMU_M], c["t_in"], c["kind"], c["hyper"], c["noise"])


@functools.lru_cache(maxsize=None)
def sweep_case_mu_deviation(name):
    """the emulated deviations of the mean of a SWEEP_CASES model inside the guard, in units of the suite's bar, over the first EMU_M candidates"""
    c = sweep_case(name)
    return mu_deviation(c["X0"], c["Y"], c["C0"][:EMU_M], c["t_in"], c["kind"], c["hyper"], c["noise"])


@functools.lru_cache(maxsize=None)
def far_case(name):
    _, kind, noise, t = [c for c in FAR_CASES if c[0] == name][0]
    N, D = 300, 4
    X0 = dyadic(2000 + abs(t) % 97, N, D)
    hyper = hyper_of(kind, D)
    assert np.array_equal((X0 + t) - t, X0)
    return dict(kind=kind, D=D, N=N, noise=noise, hyper=hyper, sw=scale_of(kind, hyper, D), X0=X0, Y=targets(2001, X0),
                C0=candidates(2002, X0, SWEEP_M), t=t)


def sample_index(M, extra=()):
    """about 60 candidates of a sweep of M: the first 17, a spread over the rest, those on observations, the last tile's last"""
    idx = np.r_[np.arange(min(M, 17)), np.arange(17, M, max(1, M // 40)), [M - 1], np.asarray(extra, dtype=int)]
    return np.unique(idx[(idx >= 0) & (idx < M)])


@functools.lru_cache(maxsize=None)
def pullin_case(name):
    """a model inside the guard near its edge; candidates 100 .. 163 of C lie at |c~|^2 in PULLIN_R2 (16 directions each: towards
    the data, away from them, along an axis and its opposite, twelve random ones).  C is in SHIFTED coordinates."""
    _, kind, D, N, noise, sign, with_prior = [c for c in PULLIN_CASES if c[0] == name][0]
    X0 = dyadic(3000 + len(name), N, D)
    hyper = hyper_of(kind, D)
    sw = scale_of(kind, hyper, D)
    t = shift_for(X0, sw, *INSIDE, sign=sign)
    C = candidates(3001, X0, SWEEP_M) + t
    rs = np.random.RandomState(3002)
    u = rs.randn(16, D)
    u[0] = (X0.mean(0) + t) * sw; u[1] = -u[0]; u[2] = np.eye(D)[0]; u[3] = -u[2]
    u /= np.linalg.norm(u, axis=1)[:, None]
    far = np.vstack([u * np.sqrt(r2) / sw for r2 in PULLIN_R2])
    C[100:100 + len(far)] = far
    prior = None
    if with_prior:                   # wide basis functions: the prior is alive hundreds of units away, where the pulled-in point is NOT the real one
        prior = (rs.rand(5, D), rs.randn(5), 2.0, np.full(D, float(t)), np.full(D, 1024.0))
    return dict(kind=kind, D=D, N=N, noise=noise, hyper=hyper, sw=sw, X0=X0, Y=targets(3003, X0), C=C, t=t, far=np.arange(100, 100 + len(far)),
                prior=prior)


@functools.lru_cache(maxsize=None)
def extend_case():
    """a model inside the guard that grows across it: X (N rows, shifted), p_in (inside the guard), p_out (|x~|^2 ~ 1.1 x the guard), the
    targets of all N + 2 rows and 9001 candidates (shifted)"""
    kind, D, N, noise = "ard", 4, 500, .1
    X0 = dyadic(5000, N, D)
    hyper = hyper_of(kind, D)
    sw = scale_of(kind, hyper, D)
    t = shift_for(X0, sw, *INSIDE)
    X = X0 + t
    p_in = dyadic(5001, 1, D)[0] * 0.5 + t
    far = X[int(np.argmax(np.sum((X * sw) ** 2, axis=1)))]
    p_out = [far + 0.25 * k for k in range(1, 200) if row_bound((far + 0.25 * k)[None, :], sw) >= 1.1 * GUARD][0]
    assert row_bound(p_in[None, :], sw) < row_bound(X, sw) <= INSIDE[1] and 1.1 * GUARD <= row_bound(p_out[None, :], sw) <= 1.2 * GUARD
    Y = targets(5002, np.vstack([X0, p_in - t, p_out - t]))
    return dict(kind=kind, D=D, N=N, noise=noise, hyper=hyper, sw=sw, t=t, X=X, p_in=p_in, p_out=p_out, Y=Y, C=candidates(5003, X0, 9001) + t)


@functools.lru_cache(maxsize=None)
def nlml_case(name):
    """X0, Y, the theta rows (thetas; the last row of thetas_over pushes the per-dimension bound just over the guard) and the shift"""
    _, kind, D, N, noise = [c for c in NLML_CASES if c[0] == name][0]
    X0 = dyadic(4000 + N + D, N, D)
    base = np.array(hyper_of(kind, D))
    if kind == "ard":
        rs = np.random.RandomState(4001)
        thetas = base[None, :] * np.exp(rs.uniform(np.log(1.0), np.log(1.6), size=(5, D)))
        thetas[0] = base                                         # the shortest length scales: the row that decides the bound
    else:
        thetas = base[None, :]
    sws = np.array([scale_of(kind, th, D) for th in thetas])
    t = shift_for(X0, sws, 0.90 * NLML_GUARD, 0.99 * NLML_GUARD, sign=1 if N == 500 else -1, bound=dim_bound)
    over = thetas[0].copy()
    over[0] *= 0.6                                              # one shorter length scale: the bound passes the guard
    thetas_over = np.vstack([thetas, over])
    b = dim_bound(X0 + t, np.array([scale_of(kind, th, D) for th in thetas_over]))
    assert NLML_GUARD < b < 4 * NLML_GUARD, b
    return dict(kind=kind, D=D, N=N, noise=noise, X0=X0, Y=targets(4002, X0), thetas=thetas, thetas_over=thetas_over, t=t)


@functools.lru_cache(maxsize=None)
def nlml_case_deviation(name):
    """the worst emulated dot-form NLML deviation over the theta rows of a case"""
    c = nlml_case(name)
    return max(nlml_deviation(c["X0"], c["Y"], c["t"], c["kind"], list(th), c["noise"])["dot"] for th in c["thetas"])

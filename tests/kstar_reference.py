"""
The truth, the bars, the grids and the restatements behind the k* probe (tests/test_kstar_reference.py on the CPU,
tests/test_gpu_kstar_probe.py on the device; DESIGN.md, "the k* probe").

THE PROBE MODEL.  One observation at the origin, Y = 4, noise = 3.  The fitted matrix is R = [1 + noise] = [4] whatever the
kernel (the reference's diagonal rule), so L = 2, W = 1/2 and alphaY = W (W Y) = 1, all exact; the padded rows of W and of the
alpha vectors are exact zeros.  The posterior mean a sweep returns at a candidate c is then 1 * k*(c) + 0 + ..: the bits its kernel
generated for k*(0, c), and s2 = 1 + noise - (k* / 2)^2 = 4 - mu^2 / 4.  With x = 0 the dot form's y = a_k + b_c + x~.c~ is b_c
itself (a_k = -0, every product 0), so its cancellation term |x~|^2 2^-52 is absent and the bar can be the FUNCTION's bar.

THE TRUTH is sf2 * map(z) in mpmath at 160 bits, from z = sum_d (c_d - x_d)^2 / theta_d^2 of the DOUBLES the device is given.
Every length scale of the probe is a power of two, so w = 1 / theta^2, sqrt(w) and c~ = c sqrt(w) are exact on the device and
z is available exactly as a double-double (error-free transformations, z_exact); the rounding that is left is the routine's own.

THE GRIDS are grids of the exponent y = -z / 2 (exponent_grids); candidates() realises each z as a point in D dimensions: every
axis but the last carries +-q, q a four-bit dyadic number <= sqrt(z / D) (squares and their partial sums are exact in any order
that takes the last axis last), the last axis the remainder.  The bars below therefore do not grow with D.

THE BARS, in eps = 2^-52 (coefficients from counting roundings and from the bounds stated beside the routines in
csrc/sweep2_dev.h and csrc/ibo_common.h; nothing here was tuned to device output):

  squared exponential on s2_exp (dot form) and on exp_fast (either form):   |got - want| <= want * 1e-15 (1 + |y| + |log sf2|)
      y = -z / 2; 1e-15 = 4.5 eps.  The routine: <= 6e-16 + 3.4e-17 |y| (2.7 eps + 0.15 eps |y|: the restatements below over the
      grids below; the source's own statements are 5e-16 / 4.4e-16 at small |y| and |n| 2.7e-20 from ln2/2048's rounding).  The
      roundings in front of it: |c~|^2 (eps / 2 on z), y = log sf2 - z / 2 (eps / 2 on |y| + |log sf2|), log sf2 itself (one
      ulp of a library log: eps |log sf2|), c~ where a scale is no power of two (eps on z) -- <= 2 eps (|y| + |log sf2|).
      Sum <= 2.7 eps + 2.15 eps (|y| + |log sf2|); with a margin of two, 4.5 eps (1 + |y| + |log sf2|).
  Matern 3/2 and 5/2 on either routine:   |got - want| <= want * eps (10 + 5.2 r),  r = sqrt(nu z)
      r carries z's roundings halved (<= 0.75 eps), the product nu z (eps / 4), sqrt_fast's stated 2e-16 (0.9 eps) and c~'s
      (eps / 2): 2.4 eps relative.  k = sf2 poly(r) exp(-r) moves by |d log k / d log r| = r^2 / (1 + r) (3/2) or
      r^2 (1 + r) / (3 poly) (5/2), both <= r, per unit of that; exp(-r) adds the routine's 2.7 eps + 0.15 eps r, the polynomial
      and the two products 2 eps.  Sum <= 4.7 eps + 2.55 eps r; with a margin of two (rounded up), eps (10 + 5.2 r).
  the library's exp and sqrt (cov, fit, grad, kg, paths, extend, the GEMV sweep):   want * 4 eps (1 + |y|)   (Matern: |y| -> r)
      exp and sqrt within one ulp (eps each), z's two roundings (eps |y|), the products (1.5 eps): <= 2.5 eps + eps |y|, margin 1.6.
  underflow:  where want / (sf2 poly) < exp(-708) = 3.3e-308 the device may return a flushed 0 (v_ldexp_f64 and the library
      flush or keep a denormal) and exp_fast its clamp exp(-708) (the source: "valid for -708 <= y"; between that and the smallest
      normal number 2.2e-308 the clamp already answers).  There the condition is |got - want| <= 4e-308 * max(1, sf2 poly)
      -- 4e-308 on the exponential itself, which the Matern kernels multiply by sf2 poly(r) afterwards -- and never a NaN.
"""
import ctypes
import ctypes.util

import mpmath as mp
import numpy as np

EPS = 2.0 ** -52
LD = np.longdouble
LN2 = float(np.log(2.0))
PI_LD = LD(3.141592653589793) + LD(1.2246467991473532e-16)
TINY_EXP = 3.3075530985118e-308          # exp(-708) rounded up: exp_fast's clamp; below it the absolute condition holds
FLUSH_ATOL = 4e-308
SE, M3, M5 = 0, 1, 2
NU = {M3: 3.0, M5: 5.0}
PULL_IN = 6e5                            # IBO_DOT_PULL_IN (csrc/ibo_common.h)

# ---------------------------------------------------------------------------------------------------- the probe model
PROBE_Y, PROBE_NOISE = 4.0, 3.0
PROBE_L, PROBE_W, PROBE_ALPHA = 2.0, 0.5, 1.0
S2_ULPS = 4 * 2.0 ** -50                 # 4 ulp of 4


def probe_factor():
    """(L, W, alphaY) of the one-row model from its definition, in exact rational arithmetic"""
    from fractions import Fraction as F
    R = F(1) + F(PROBE_NOISE)
    L = F(int(np.sqrt(float(R))))
    assert L * L == R
    W = 1 / L
    return float(L), float(W), float(W * (W * F(PROBE_Y)))


def probe_s2(mu, clamp_lo):
    """the variance the probe model must return next to mu: 1 + noise - (W mu)^2, clipped as the sweep clips"""
    mu = np.asarray(mu, dtype=LD)
    return np.clip(LD(1.0 + PROBE_NOISE) - mu * mu / 4, LD(clamp_lo), LD(10.0)).astype(np.float64)


# ---------------------------------------------------------------------------------------------------- error-free arithmetic
def two_sum(a, b):
    s = a + b
    bb = s - a
    return s, (a - (s - bb)) + (b - bb)


def two_prod(a, b):
    """a b = p + e exactly (Veltkamp / Dekker; operands scaled so that the split cannot overflow or lose bits to underflow)"""
    a = np.asarray(a, dtype=np.float64); b = np.asarray(b, dtype=np.float64)
    ea = np.where(a == 0, 0, np.frexp(a)[1]); eb = np.where(b == 0, 0, np.frexp(b)[1])
    a1 = np.ldexp(a, -ea); b1 = np.ldexp(b, -eb)
    p = a1 * b1
    c = 134217729.0 * a1; ah = c - (c - a1); al = a1 - ah
    c = 134217729.0 * b1; bh = c - (c - b1); bl = b1 - bh
    e = ((ah * bh - p) + ah * bl + al * bh) + al * bl
    return np.ldexp(p, ea + eb), np.ldexp(e, ea + eb)


def fma(a, b, c):
    """round(a b + c) from the exact product and a long-double sum: the device's v_fma_f64 up to a double rounding at 2^-64"""
    p, e = two_prod(a, b)
    return ((LD(1) * p + np.asarray(c, dtype=LD)) + e).astype(np.float64)


def z_exact(C, x, ell):
    """z = sum_d ((c_d - x_d) / ell_d)^2 as an unevaluated sum hi + lo of two doubles, relative error about 2^-100.
    ell: powers of two (asserted), so the division is exact.  C: (M, D); x, ell: (D,)"""
    C = np.atleast_2d(np.asarray(C, dtype=np.float64)); x = np.asarray(x, dtype=np.float64); ell = np.asarray(ell, dtype=np.float64)
    assert np.all(np.frexp(ell)[0] == 0.5), "the exact path needs power-of-two length scales"
    hi = np.zeros(len(C)); lo = np.zeros(len(C))
    with np.errstate(under="ignore"):
        for d in range(C.shape[1]):
            u, du = two_sum(C[:, d] / ell[d], -x[d] / ell[d])
            p, e = two_prod(u, u)
            hi, t = two_sum(hi, p)
            lo = lo + (t + e + 2.0 * u * du)
        return two_sum(hi, lo)


# ---------------------------------------------------------------------------------------------------- the truth
def _ld(m):
    h = float(m)
    return LD(h) + LD(float(m - mp.mpf(h)))


def _map_mp(fam, z):
    if fam == SE:
        return mp.exp(-z / 2)
    r = mp.sqrt(NU[fam] * z)
    return ((1 + r) if fam == M3 else (1 + r + r * r / 3)) * mp.exp(-r)


def _to_ld_or_zero(v):
    # (long double reaches 1e-4932: anything smaller is 0 for every condition below)
    return LD(0) if abs(v) < mp.mpf(10) ** -4900 else (_mp_to_ld(v) if v > 0 else -_mp_to_ld(-v))


def kernel_map(fam, zhi, zlo):
    """map(z) without sf2 in mpmath, as long double (64-bit mantissa; its exponent range keeps what a double flushes)"""
    out = np.empty(len(zhi), dtype=LD)
    with mp.workprec(160):
        for i in range(len(zhi)):
            out[i] = _to_ld_or_zero(_map_mp(fam, mp.mpf(float(zhi[i])) + mp.mpf(float(zlo[i]))))
    return out


def kernel_of_theta(fam, theta):
    """map(z) of the pair {0, 1} in one dimension under the length scales theta (any doubles): z = 1 / theta^2, in mpmath"""
    out = np.empty(len(theta), dtype=LD)
    with mp.workprec(160):
        for i, t in enumerate(theta):
            out[i] = _to_ld_or_zero(_map_mp(fam, 1 / mp.mpf(float(t)) ** 2))
    return out


def _mp_to_ld(v):
    man, ex = mp.frexp(v)                                                # v = man 2^ex, 0.5 <= man < 1
    return np.ldexp(_ld(man), int(ex))


def kernel_dmap(fam, zhi, zlo):
    """d map / d z in mpmath (the closed-form derivative behind dk*/dc = dmap/dz * 2 (c - x) / theta^2), as long double"""
    out = np.empty(len(zhi), dtype=LD)
    with mp.workprec(160):
        for i in range(len(zhi)):
            z = mp.mpf(float(zhi[i])) + mp.mpf(float(zlo[i]))
            if fam == SE:
                v = -mp.exp(-z / 2) / 2
            else:
                r = mp.sqrt(NU[fam] * z)
                # d/dz [(1 + r) e^-r] = -nu e^-r / 2;  d/dz [(1 + r + r^2/3) e^-r] = -nu (1 + r) e^-r / 6
                v = -NU[fam] * mp.exp(-r) / 2 if fam == M3 else -NU[fam] * (1 + r) * mp.exp(-r) / 6
            out[i] = LD(0) if abs(v) < mp.mpf(10) ** -4900 else _mp_to_ld(v)
    return out


def radius(fam, z):
    """|y| for the squared exponential, r = sqrt(nu z) for the Matern kernels: what the bars grow with"""
    z = np.asarray(z, dtype=np.float64)
    return z / 2 if fam == SE else np.sqrt(NU[fam] * z)


def prefactor(fam, z, sf2):
    """what multiplies the exponential after it is formed: 1 where sf2 rides in the exponent (squared exponential on the fast
    routines), sf2 poly(r) for the Matern kernels"""
    if fam == SE:
        return np.ones_like(np.asarray(z, dtype=np.float64))
    r = radius(fam, z)
    return sf2 * ((1 + r) if fam == M3 else (1 + r + r * r / 3))


# ---------------------------------------------------------------------------------------------------- the bars
def bar_fast(fam, z, sf2):
    """relative bar of the hand-written routines (s2_exp, exp_fast, sqrt_fast), dot or difference form"""
    if fam == SE:
        return 1e-15 * (1 + radius(SE, z) + abs(np.log(sf2)))
    return EPS * (10 + 5.2 * radius(fam, z))


def bar_lib(fam, z, sf2=1.0):
    """relative bar of the library's exp / sqrt behind cov_from_z_rt"""
    return 4 * EPS * (1 + radius(fam, z))


def violations(got, want, rel, fam, z, sf2, lib=False):
    """indices where got misses want (long double): beyond the relative bar and, in the underflow range, beyond the absolute one;
    or a NaN.  Also returns the worst ratio to the relative bar among the points held to it."""
    got = np.asarray(got, dtype=np.float64)
    # (the library route multiplies the squared exponential by sf2 as well; a product below 1 can itself underflow: never under 1)
    pre = np.maximum(np.full(len(got), float(sf2)) if (lib and fam == SE) else prefactor(fam, z, sf2), 1.0)
    err = np.abs(LD(1) * got - want)
    tiny = want < LD(TINY_EXP) * pre
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        ratio = np.where(tiny, LD(0), err / (want * rel)).astype(np.float64)
    ok = np.where(tiny, err <= LD(FLUSH_ATOL) * pre, ratio <= 1.0) & np.isfinite(got)
    return np.flatnonzero(~ok), float(np.nanmax(ratio)) if len(ratio) else 0.0


# ---------------------------------------------------------------------------------------------------- the grids
def exponent_grids():
    """{name: y <= 0}: the exponents -z/2 the probe visits (sf2 != 1 moves the function's argument by log sf2: positive arguments
    through sf2 = 1e6, arguments below -13.8 through 1e-6)"""
    j = np.arange(4096, dtype=np.float64)
    table = (-j * (LN2 / 2048))[:, None] + np.array([-1.6e-4, 0.0, 1.6e-4])[None, :]    # every table index twice: centre and both ends of |r| <= 1.7e-4
    table = np.minimum(table.ravel(), 0.0)
    logrun = -np.logspace(-300, np.log10(745.0), 640)
    # around the underflow threshold and exp_fast's clamp, in steps of 1/16
    edge = -np.arange(700.0, 752.0, 0.0625)
    far = -np.r_[760.0, 1e3, 1e4, 1e5, 2.9e5, 0.5 * PULL_IN * (1 - 2.0 ** -40), 0.5 * PULL_IN]
    beyond = -np.r_[0.5 * PULL_IN * (1 + 2.0 ** -40), 3.1e5, 1e7, 1e12]
    return dict(table=table, logrun=logrun, edge=edge, far=far, beyond=beyond, origin=np.zeros(1))


def probe_length_scales(kind, D):
    """power-of-two length scales: distinct per axis for the ARD kernel, one for the others"""
    if kind == "ard":
        return np.array([0.5, 2.0, 0.25, 1.0] * 16)[:D]
    return np.array([0.5])


def candidates(y, ell, D):
    """(len(y), D) points c with sum_d (c_d / ell_d)^2 = -2y up to the rounding of the last axis' square root; see the module text"""
    z = -2.0 * np.asarray(y, dtype=np.float64)
    ell = np.broadcast_to(np.asarray(ell, dtype=np.float64), (D,)) if np.size(ell) == 1 else np.asarray(ell, dtype=np.float64)
    Ct = np.zeros((len(z), D))
    with np.errstate(under="ignore", divide="ignore"):
        if D > 1:
            s = np.sqrt(z / D)
            m, e = np.frexp(s)
            q = np.ldexp(np.floor(m * 16) / 16, e)                        # four bits, rounded down: (D - 1) q^2 <= z (D - 1) / D
            sign = np.where(np.arange(D - 1) % 2 == 0, 1.0, -1.0)
            Ct[:, :D - 1] = q[:, None] * sign[None, :]
            rem = z - (D - 1) * q * q
        else:
            rem = z
        Ct[:, D - 1] = np.sqrt(np.maximum(rem, 0.0))
    return Ct * ell[None, :]


def thin(y, every=7):
    return y[::every]


_grids = {}


def probe_grid(fam, D, kind="iso", full=True):
    """every grid realised in D dimensions around the origin, with its truth (computed once per process): dict(y, C, ell, z,
    m = map(z) as long double).  full: every table point (13.7k candidates); otherwise every seventh (3.2k)"""
    key = (fam, D, kind, full)
    if key not in _grids:
        g = exponent_grids()
        y = np.concatenate([g["table"] if full else thin(g["table"]), g["logrun"], g["edge"], g["far"], g["beyond"], g["origin"]])
        ell = probe_length_scales(kind, D)
        C = candidates(y, ell, D)
        zhi, zlo = z_exact(C, np.zeros(D), np.broadcast_to(ell, (D,)))
        _grids[key] = dict(y=y, C=C, ell=ell, z=zhi, zlo=zlo, m=kernel_map(fam, zhi, zlo))
    return _grids[key]


# ---------------------------------------------------------------------------------------------------- the restatements
_libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
_libm.exp2.restype = ctypes.c_double
_libm.exp2.argtypes = [ctypes.c_double]


def s2_table():
    """2^(j/2048) as the library builds it (csrc/abi_sweep.hip exp_table): the C library's exp2 of j / 2048.0"""
    return np.array([_libm.exp2(j / 2048.0) for j in range(2048)])


def s2_table_exact():
    with mp.workprec(160):
        return np.array([float(mp.power(2, mp.mpf(j) / 2048)) for j in range(2048)])


S2_C = dict(inv=2954.6394437405970584, ln2_2048=3.384507717577858e-04)
MAGIC = 6755399441055744.0


def _low_word(t):
    return (np.asarray(t, dtype=np.float64).view(np.int64) & 0xffffffff).astype(np.uint32).view(np.int32)


def s2_exp(y, tab=None, c=S2_C):
    """csrc/sweep2_dev.h s2_exp, operation by operation.  v_ldexp_f64's flush of a denormal result is not restated (np.ldexp
    keeps the denormal): the underflow condition covers either."""
    tab = s2_table() if tab is None else tab
    y = np.asarray(y, dtype=np.float64)
    t = fma(y, c["inv"], MAGIC)
    n = t - MAGIC
    r = fma(n, -c["ln2_2048"], y)
    ti = _low_word(t)
    T = tab[ti & 2047]
    p = fma(r, 1.0 / 6.0, 0.5)
    p = fma(p, r, 1.0)
    p = fma(p, r, 1.0)
    with np.errstate(under="ignore"):
        return np.ldexp(T * p, (ti >> 11).astype(np.int64))


EXP_FAST_C = [2.76263763215172631873e-07, 2.76401811512398433028e-06, 2.48015043005816596198e-05, 1.98411702694117908236e-04,
              1.38888889325245227201e-03, 8.33333338566888577603e-03, 4.16666666665730586749e-02, 1.66666666665543999892e-01,
              5.00000000000000555112e-01, 1.00000000000000666134e+00, 1.0]


def exp_fast(y, coef=EXP_FAST_C):
    """csrc/ibo_common.h exp_fast, operation by operation (2^n by ldexp: the same bits as the integer add while the result is normal)"""
    y = np.maximum(np.asarray(y, dtype=np.float64), -708.0)
    t = fma(y, 1.4426950408889634074, MAGIC)
    n = t - MAGIC
    r = fma(n, -6.93147180369123816490e-01, y)
    r = fma(n, -1.90821492927058770002e-10, r)
    p = np.full_like(y, coef[0])
    for c in coef[1:]:
        p = fma(p, r, c)
    return np.ldexp(p, _low_word(t).astype(np.int64))


def kstar_restated(routine, fam, C, ell, sf2, sqrt_err=0.0, **kw):
    """k*(0, c) as the sweep kernels form it from the candidate: c~ = c / ell, |c~|^2 by FMAs in ascending order, then
    routine 's2' (sweep2 / small2: b_c = log sf2 - |c~|^2 / 2 into s2_exp; candidates beyond the pull-in radius pulled in),
    'fast-dot' (the first-generation kernels' dot form) or 'fast-diff' (their difference form, cov_from_z_fast).
    sqrt_err: a relative error put on sqrt_fast's result (its own arithmetic, v_rsq_f64 and a correction, is not restated: the
    bar budgets its stated 2e-16)"""
    C = np.atleast_2d(np.asarray(C, dtype=np.float64)); ell = np.broadcast_to(np.asarray(ell, dtype=np.float64), (C.shape[1],))
    Ct = C * (1.0 / ell)[None, :]
    n2 = np.zeros(len(C))
    for d in range(C.shape[1]):
        n2 = fma(Ct[:, d], Ct[:, d], n2)
    ex = (lambda v: s2_exp(v, **kw)) if routine == "s2" else (lambda v: exp_fast(v, **kw))
    if routine == "s2":
        n2 = np.minimum(n2, PULL_IN)
    log_sf2 = float(np.log(sf2))
    if fam == SE:
        return ex(fma(-0.5, n2, log_sf2))
    z = n2
    rr = np.sqrt(np.maximum(NU[fam] * z, 1e-300)) * (1.0 + sqrt_err)
    poly = 1.0 + rr if fam == M3 else fma(rr, fma(rr, 1.0 / 3.0, 1.0), 1.0)
    with np.errstate(under="ignore"):
        return sf2 * poly * ex(-rr)


# ---------------------------------------------------------------------------------------------------- the acquisition epilogue
NR_COEF = [0.17087277, -0.82215223, 1.48851587, -1.13520398, 0.27886807, -0.18628806, 0.09678418, 0.37409196, 1.00002368]
# erf_nr_dev (csrc/ibo_common.h): nine Horner steps on |values| <= 1.5 (14 eps on t p), z^2 (eps z^2 / 2) and the constant: the
# exponential's argument is off by <= eps (15 + z^2) absolute, its value t exp(..) <= min(1, e^(-z^2)) relative by that much plus two
# ulp: |erf error| <= 16 eps (z^2 e^(-z^2) <= 0.37).
NR_ERF_ROUNDING = 16 * EPS


def acq_truth(acq, erf_mode, mu, s2, ymax, parm):
    """EI (0) / PI (1) / UCB (2) by the reference's formula in mpmath from the device's own mu and s2 (scalars or equal-length
    arrays); erf_mode 1: the Numerical-Recipes erf with its truncated constants 0.707106 and 0.398942.  Returns (value, |ydiff|, sigma)."""
    mu, s2, ymax = np.broadcast_arrays(np.asarray(mu, dtype=np.float64), np.asarray(s2, dtype=np.float64), np.asarray(ymax, dtype=np.float64))
    val = np.empty(mu.shape, dtype=LD); yd = np.empty(mu.shape); sg = np.empty(mu.shape)
    with mp.workprec(160):
        for i in np.ndindex(mu.shape):
            m, sigma = mp.mpf(float(mu[i])), mp.sqrt(mp.mpf(float(s2[i])))
            sg[i] = float(sigma)
            if acq == 2:
                val[i] = _ld(m + mp.mpf(parm) * sigma); yd[i] = abs(float(mu[i]))
                continue
            ydiff = m - mp.mpf(float(ymax[i])) - mp.mpf(parm)
            Z = ydiff / sigma
            yd[i] = abs(float(ydiff))
            if erf_mode == 0:
                cdf = (1 + mp.erf(Z / mp.sqrt(2))) / 2
                pdf = mp.exp(-Z * Z / 2) / mp.sqrt(2 * mp.pi)
            else:
                u = Z * mp.mpf(0.707106)
                t = 1 / (1 + abs(u) / 2)
                p = mp.mpf(NR_COEF[0])
                for c in NR_COEF[1:]:
                    p = mp.mpf(c) + t * p
                e = 1 - t * mp.exp(-u * u - mp.mpf(1.26551223) + t * p)
                cdf = (1 + (e if u >= 0 else -e)) / 2
                pdf = mp.exp(-Z * Z / 2) * mp.mpf(0.398942)
            v = cdf if acq == 1 else ydiff * cdf + sigma * pdf
            val[i] = LD(0) if abs(v) < mp.mpf(10) ** -4900 else (_mp_to_ld(v) if v > 0 else -_mp_to_ld(-v))
    return val, yd, sg


def acq_bar(acq, erf_mode, ydiff_abs, sigma):
    """absolute: 8 eps (|ydiff| + sigma) (UCB = mu + parm sigma: |mu| and |parm| sigma in their places -- a value of 2000 has an ulp
    of 2e-13), plus for the NR flavour its erf's rounding through the value"""
    bar = 8 * EPS * (ydiff_abs + sigma)
    if erf_mode == 1 and acq != 2:
        bar = bar + 0.5 * NR_ERF_ROUNDING * (1.0 if acq == 1 else ydiff_abs)
    return bar


# ---------------------------------------------------------------------------------------------------- the 2 x 2 likelihood
def nlml_2x2(k, noise):
    """-log p(Y | X) of N = 2, Y = (1, -1) from the off-diagonal covariance k (long double), diagonal a = 1 + noise:
    1 / (a - k) + log((a - k)(a + k)) / 2 + log 2 pi;  also |d nlml / d k|"""
    k = np.asarray(k, dtype=LD)
    a = LD(1) + LD(noise)
    v = 1 / (a - k) + np.log((a - k) * (a + k)) / 2 + np.log(2 * PI_LD)
    return v, np.abs(1 / (a - k) ** 2 - k / ((a - k) * (a + k)))

"""
The arg-max contract of every entry that picks a winner (include/ibo_abi.h; csrc/ibo_common.h above wave_argmax), stated in plain
NumPy, and the inputs tests/test_gpu_argmax_contract.py puts in front of the kernels.

The rule
    the largest value wins; the FIRST index wins ties (numpy.argmax order); NaN values, rows inside an exclusion ball
    (min_j |c - e_j| <= radius; a NaN distance counts as inside, as the kernels' !(sqrt(d2) > r) does) and rows past M never win;
    nothing admissible: (-inf, -1), the -1 not shifted; otherwise index_base is added to the index.

The plateau construction
    A tie has to be a tie on every route, whatever tile, lane or chunk a row lands in.  Rows whose every coordinate lies in
    [1000, 2000] are more than a thousand length scales from unit-cube data: k* = 0 exactly in every kernel family (the exponent
    underflows; the first-generation tile kernel's clamped exp leaves 1e-308, which the sums absorb), so mu = 0, s2 = 1 + noise and
    the acquisition value carry the same bits in every such row.  With Y shifted down by 4 (max Y about -3) that value -- the
    plateau -- lies far above anything a unit-cube row reaches; tests/test_argmax_reference.py proves the margin on the CPU for every
    model and acquisition used here.  Coordinates are multiples of 0.25, so distances between far rows and to a centre 0.25 away
    are exact.
"""
import math

import numpy as np

from conftest import synth

NOISE = .1
Y_SHIFT = 4.0
LOSER_BASE = 1500              # distinct unit-cube rows; longer loser arrays repeat them (equal losers lose all the same)
MARGIN = 0.9                   # max(loser) < MARGIN * plateau

# name -> (seed, N, D, kind, hyper) -- kind as oracle.Kern names it
MODELS = {
    "se193": (193, 193, 3, "ard", [.3, .35, .4]),
    "se1024": (1024, 1024, 4, "ard", [.3] * 4),
    "m5_512": (512, 512, 3, "m5", [.6, 1.0]),
    "m3_64": (64, 64, 3, "m3", [.6, 1.0]),
}
# the acquisitions of the GPU file, all under native=True (libm erf, clamp 1e-8): name -> (sweep's acq, parm)
ACQS = {"ei": ("ei", .01), "pi": ("pi", .3), "ucb": ("ucb", 2.0)}


def argmax_rule(values, cand=None, exclude=None, radius=0.0, index_base=0):
    """(value, index) of the contract.  values (M,); cand (M, D) and exclude (n, D) only where there are exclusion balls."""
    values = np.asarray(values, dtype=float)
    ok = ~np.isnan(values)
    if exclude is not None and len(exclude):
        cand = np.asarray(cand, dtype=float); exclude = np.atleast_2d(np.asarray(exclude, dtype=float))
        for e in exclude:
            d = np.sqrt(np.sum((cand - e) ** 2, axis=1))
            with np.errstate(invalid="ignore"):
                ok &= d > radius                        # (NaN > r is False: excluded)
    idx = np.flatnonzero(ok)
    if len(idx) == 0:
        return -np.inf, -1
    j = int(np.argmax(values[idx]))                    # numpy.argmax: the first maximiser
    return float(values[idx][j]), int(index_base) + int(idx[j])


def model_data(name):
    """(X, Y) of a model: conftest.synth with Y shifted down so that max(Y) is about -3"""
    seed, N, D, _, _ = MODELS[name]
    X, Y = synth(seed, N, D)
    return X, Y - Y_SHIFT


def losers(M, D, seed=7):
    """M unit-cube rows: LOSER_BASE distinct ones, repeated"""
    base = np.random.RandomState(seed).rand(LOSER_BASE, D)
    return base[np.arange(M) % LOSER_BASE].copy()


def far_rows(n, D, seed=11):
    """n distinct rows with every coordinate a multiple of 0.25 in [1000, 2000], no two within 1 of each other in the first
    coordinate (so that a centre 0.25 away from one is at least 0.75 from every other)"""
    rs = np.random.RandomState(seed)
    first = 1000.0 + rs.choice(1000, size=n, replace=False)
    rest = rs.randint(4000, 8001, size=(n, D - 1)) * 0.25
    return np.c_[first, rest]


def plant(M, D, P, seed=7):
    """the array of a position test: losers everywhere, distinct far rows at the indices P (in the order given)"""
    cand = losers(M, D, seed)
    P = list(P)
    cand[P] = far_rows(len(P), D)
    return cand


KG_MODEL, KG_NREF = "se193", 8


def kg_inputs():
    """(reference points, strong row, weak rows) for ibo_kg_sweep, where a far row is worth nothing (its own line is the incumbent):
    of LOSER_BASE unit-cube rows the one with the largest knowledge gradient under tests/kg_reference.py, and the rows that stay below
    half of it.  Copies of the strong row are the ties; tests/test_argmax_reference.py pins the margin."""
    import grad_reference as gr
    import kg_reference as kr
    _, _, D, kind, hyper = MODELS[KG_MODEL]
    X, Y = model_data(KG_MODEL)
    A = np.ascontiguousarray(X[:KG_NREF])
    pool = losers(LOSER_BASE, D)
    fam, w, sf2 = gr.kernel_spec(kind, hyper, D)
    v = kr.kg(gr.RefGP(X, Y, NOISE, fam, w, sf2), A, pool)["kg"]
    j = int(np.argmax(v))
    return A, pool[j].copy(), pool[v < 0.5 * v[j]].copy(), float(v[j]), float(np.max(v[v < 0.5 * v[j]]))


def plant_kg(M, P, strong, weak):
    """weak rows, repeated, with copies of the strong row at the indices P"""
    cand = weak[np.arange(M) % len(weak)].copy()
    cand[list(P)] = strong
    return cand


def _cdf(z): return 0.5 * (1.0 + math.erf(z / math.sqrt(2.0)))
def _pdf(z): return math.exp(-(z * z / 2.0)) / math.sqrt(2.0 * math.pi)


def acq_closed_form(acq, parm, mu, sigma, ymax):
    """EI / PI / UCB in float64 with libm's erf (native=True), as csrc/ibo_common.h: acq_value_dev states them"""
    if acq == "ucb":
        return mu + parm * sigma
    ydiff = mu - ymax - parm
    z = ydiff / sigma
    return _cdf(z) if acq == "pi" else ydiff * _cdf(z) + sigma * _pdf(z)


def plateau_value(acq, parm, ymax, noise=NOISE):
    """the value of a far row: the closed form at (mu, sigma) = (0, sqrt(1 + noise))"""
    return acq_closed_form(acq, parm, 0.0, math.sqrt(1.0 + noise), ymax)

"""
The call sequences of tests/test_gpu_alloc_fill.py: every entry of the C ABI that touches device memory, through the raw ABI, at the smallest
shapes that still have every kind of pad -- N in {70, 130, 200} (no multiple of 64 or 128, on both sides of 128), D in {3, 5} (DP = 4 or 8
with pad columns), M in {1, 65, 130, 1000} candidates (off every 64 / 256 seam, within the size classes).

A case is a function of one argument, a Rec.  It creates ALL its handles and device arrays inside itself, records every output, return
code, info word and DIRECT sample count, and destroys what it created (the `made` list of run()).  run(name) returns the record as a list
of (label, itemsize, bytes): two runs agree when the lists are equal; first_difference() names the first output and index that differ.
Outputs start from GUARD, never from np.empty, so that an element an entry leaves alone is the same bytes in every run; device outputs are
ibo_dev_alloc arrays (filled by the hook like every new buffer, then overwritten with GUARD) read back whole.

Every entry claims "the same bits from call to call" (README), so NOT_BIT_REPRODUCIBLE is empty: the control of the test is bit equality
for every label.  A timing (ibo_gp_last_fit_ms, the *_stage_ms / *_scan_ms sums) is not a result and is not recorded.

The sparse model: "sgp_chunk" is rounded up to 256 observations, so the 300 observations of `sgp` travel in two chunks (256 + 44, the last
one partial); `sgp_three_chunks` runs the same sequence on 600 (256 + 256 + 88).
"""
import ctypes
import re
from collections import OrderedDict

import numpy as np

from ibo_amd import _lib

lib, dp, f64 = _lib.lib, _lib.dp, _lib.f64
GUARD = -7.25e301
NOISE = .05
I64P, IP = ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int)
EI, PI, UCB, NONE = _lib.ACQ_EI, _lib.ACQ_PI, _lib.ACQ_UCB, _lib.ACQ_NONE
NAN = float("nan")
MS = (1, 65, 130, 1000)
SHAPES = ((70, 3), (130, 5), (200, 3))
ACQS = ((EI, .01), (PI, .01), (UCB, 1.3))
DIRECT = (10, 30, 10000, 1)           # maxiter, maxtime, maxsample, compat
NOT_BIT_REPRODUCIBLE = {}             # label prefix -> (bar, where it is documented): none (see above)

# entries that hand out, fill or read no buffer whose content a result could depend on: one line each
NO_DEVICE_MEMORY = OrderedDict([
    ("ibo_abi_version", "a constant"),
    ("ibo_last_error", "the thread's message buffer on the host"),
    ("ibo_device_count", "asks the runtime, allocates nothing"),
    ("ibo_device_name", "asks the runtime, allocates nothing"),
    ("ibo_gpu_time_ms", "a host-side sum of event times: a timing, not a result"),
    ("ibo_gp_last_fit_ms", "an event time: a timing, not a result"),
    ("ibo_last_sweep_kernel_ms", "an event time and a kernel's name: a timing, not a result"),
    ("ibo_ehvi_scan_ms", "a per-thread sum of event times on the host"),
    ("ibo_mes_scan_ms", "a per-thread sum of event times on the host"),
    ("ibo_kg_stage_ms", "a per-thread sum of event times on the host"),
    ("ibo_qei_stage_ms", "a per-thread sum of event times on the host"),
    ("ibo_ggp_stage_ms", "a per-thread sum of event times on the host"),
    ("ibo_ggp_grad_stage_ms", "a per-thread sum of event times on the host"),
    ("ibo_sgp_stage_ms", "a per-thread sum of event times on the host"),
    ("ibo_sgp_grad_stage_ms", "a per-thread sum of event times on the host"),
    ("ibo_direct_host", "DIRECT on a host callback: no GPU is touched"),
    ("direct", "libego's DIRECT on a host callback: no GPU is touched"),
    ("logCDFs", "a host-side sum"),
])


class Rec(object):
    def __init__(self):
        self.out, self.made = [], []

    def put(self, label, a):
        self.out.append((label, np.array(a, copy=True)))

    def rc(self, label, code):
        """a return code: recorded, and returned so that a case can stop where going on would read what a failed call left"""
        self.out.append((label + ".rc", np.array([code], dtype=np.int64)))
        return code

    def own(self, destroy, h):
        self.made.append((destroy, h))
        return h


def run(name):
    """one run of a case: [(label, itemsize, bytes)]"""
    rec = Rec()
    try:
        CASES[name](rec)
    finally:
        for destroy, h in reversed(rec.made):
            destroy(h)
    return [(label, a.dtype.itemsize, a.tobytes()) for label, a in rec.out]


def first_difference(a, b):
    """None, or a sentence naming the first output and the first index at which two records differ"""
    if [x[0] for x in a] != [x[0] for x in b]:
        return "the runs recorded different outputs: %s / %s" % ([x[0] for x in a][:40], [x[0] for x in b][:40])
    for (label, size, x), (_, _, y) in zip(a, b):
        if x != y:
            if len(x) != len(y):
                return "output '%s': %d bytes against %d" % (label, len(x), len(y))
            i = next(k for k in range(len(x)) if x[k] != y[k]) // size
            return "output '%s' differs first at index %d: %s against %s" % (label, i, x[i * size:(i + 1) * size].hex(), y[i * size:(i + 1) * size].hex())
    return None


def return_codes(record):
    return [(label, int(np.frombuffer(b, dtype=np.int64)[0])) for label, _, b in record if label.endswith(".rc")]


def option(key, value):
    _lib.check(lib.ibo_set_option(key, value))


def trim():
    return lib.ibo_trim(0)


# ---------------------------------------------------------------------------------------------- data and handles
def data(N, D, seed=11):
    rs = np.random.RandomState(seed)
    X = rs.rand(N, D)
    s = 3 * X.sum(1)
    return f64(X), f64(np.sin(s) + .01 * rs.randn(N))


def ell(D):
    return f64([.4, .55, .35, .6, .45][:D])


def points(M, D, seed=5):
    return f64(np.random.RandomState(seed + M).rand(M, D))


def guard(*shape):
    return np.full(shape, GUARD)


class Dev(object):
    """a caller's device array through the raw entries"""
    def __init__(self, rec, host):
        host = f64(host)
        self.shape, self.nbytes, self.ptr = host.shape, host.nbytes, ctypes.c_void_p()
        _lib.check(lib.ibo_dev_alloc(0, self.nbytes, ctypes.byref(self.ptr)))
        rec.own(lambda d: lib.ibo_dev_free(0, d.ptr), self)
        _lib.check(lib.ibo_memcpy_h2d(0, self.ptr, host.ctypes.data_as(ctypes.c_void_p), self.nbytes))

    def to_host(self):
        out = guard(*self.shape)
        _lib.check(lib.ibo_memcpy_d2h(0, out.ctypes.data_as(ctypes.c_void_p), self.ptr, self.nbytes))
        return out


def dev_in(rec, a):
    return Dev(rec, a)


def dev_out(rec, *shape):
    """an output array: GUARD in every element, as the host outputs have, so that what an entry leaves alone is the same bytes in every run"""
    return Dev(rec, guard(*shape))


def read(rec, label, d):
    rec.rc(label + ".sync", lib.ibo_device_synchronize(0))
    rec.put(label, d.to_host())


def gp_new(rec):
    h = ctypes.c_void_p()
    _lib.check(lib.ibo_gp_create(0, ctypes.byref(h)))
    return rec.own(lib.ibo_gp_destroy, h)


def gp_fit(rec, label, h, X, Y, A=None, noise=NOISE):
    info = ctypes.c_int(-7)
    N, D = X.shape
    if A is None:
        rc = lib.ibo_gp_fit(h, _lib.K_SE_ARD, N, D, dp(X), dp(Y), dp(ell(D)), D, 1.0, noise, ctypes.byref(info))
    else:
        rc = lib.ibo_gp_fit_with_matrix(h, _lib.K_SE_ARD, N, D, dp(X), dp(Y), dp(ell(D)), D, 1.0, noise, dp(A), ctypes.byref(info))
    rec.put(label + ".info", [info.value])
    return rec.rc(label, rc)


def fitted(rec, label, N, D, seed=11, reserve=0):
    X, Y = data(N, D, seed)
    h = gp_new(rec)
    if reserve:
        rec.rc(label + ".reserve", lib.ibo_gp_reserve(h, reserve))
    gp_fit(rec, label, h, X, Y)
    return h, X, Y


def gp_state(rec, label, h, N, D):
    """what a handle holds, through the accessors and a host batch of 65 points"""
    for name, get in (("L", lib.ibo_gp_get_L), ("W", lib.ibo_gp_get_W), ("R", lib.ibo_gp_get_R)):
        out = guard(N, N)
        rec.rc(label + "." + name, get(h, dp(out)))
        rec.put(label + "." + name, out)
    n, d, dev, my = ctypes.c_int(-7), ctypes.c_int(-7), ctypes.c_int(-7), ctypes.c_double(GUARD)
    rec.rc(label + ".gp_info", lib.ibo_gp_info(h, ctypes.byref(n), ctypes.byref(d), ctypes.byref(dev), ctypes.byref(my)))
    rec.put(label + ".gp_info", [n.value, d.value, dev.value, my.value])
    batch(rec, label + ".batch", h, 65, D)


def batch(rec, label, h, M, D, acq=EI, parm=.01):
    Q = points(M, D)
    mu, s2, a = guard(M), guard(M), guard(M)
    rec.rc(label, lib.ibo_acq_batch(h, M, dp(Q), acq, parm, 0, 1e-8, NAN, dp(mu), dp(s2), dp(a)))
    for name, v in (("mu", mu), ("s2", s2), ("acq", a)):
        rec.put(label + "." + name, v)


def sweep(rec, label, h, M, D, acq, parm, entry=None, lead=()):
    """ibo_acq_sweep's arguments on any entry that carries them (lead: what the entry puts in front)"""
    cand = dev_in(rec, points(M, D))
    mu, s2, a = dev_out(rec, M), dev_out(rec, M), dev_out(rec, M)
    bv, bi = ctypes.c_double(GUARD), ctypes.c_int64(-7)
    excl = f64(np.full((1, D), .5))
    rc = (entry or lib.ibo_acq_sweep)(*(lead + (h, M, cand.ptr, acq, parm, 0, 1e-8, NAN, 1, dp(excl), .05, 1000, mu.ptr, s2.ptr, a.ptr,
                                              ctypes.byref(bv), ctypes.byref(bi))))
    rec.rc(label, rc)
    rec.put(label + ".best", [bv.value]); rec.put(label + ".idx", [bi.value])
    for name, v in (("mu", mu), ("s2", s2), ("acq", a)):
        read(rec, label + "." + name, v)


def direct_out(rec, label, rc, opt, optx, ns):
    rec.rc(label, rc)
    rec.put(label + ".opt", [opt.value]); rec.put(label + ".optx", optx); rec.put(label + ".nsamples", [ns.value])


def box(D):
    return f64(np.zeros(D)), f64(np.ones(D)), ctypes.c_double(GUARD), guard(D), ctypes.c_int64(-7)


# ---------------------------------------------------------------------------------------------- plain ibo_gp
def case_library(rec):
    err = ctypes.c_double(GUARD)
    rec.rc("selftest", lib.ibo_selftest_mfma(0, ctypes.byref(err)))
    rec.put("selftest.err", [err.value])
    d = dev_out(rec, 1000)
    g = ctypes.c_uint64(0)
    rec.rc("generation", lib.ibo_dev_generation(0, d.ptr, ctypes.byref(g)))
    rec.put("generation.nonzero", [int(g.value != 0)])
    rec.rc("trim", lib.ibo_trim(0))


def case_fit(N, D, min_nb=None):
    def case(rec):
        if min_nb:
            option(b"fused2_min_nb", min_nb)    # the two-level order from min_nb block columns on: every size here
        try:
            h, X, Y = fitted(rec, "fit", N, D)
            gp_state(rec, "fit", h, N, D)
            h2, _, _ = fitted(rec, "again", N, D, seed=12)       # a second model beside the first: its buffers are what the pool has left
            gp_state(rec, "again", h2, N, D)
        finally:
            option(b"fused2_min_nb", 104)
    return case


def prior_arrays(D, nb=4):
    rs = np.random.RandomState(3)
    return nb, f64(rs.rand(nb, D)), f64(rs.randn(nb)), 2.0, f64(np.zeros(D)), f64(np.ones(D))


def case_fit_prior(N, D):
    def case(rec):
        X, Y = data(N, D)
        h = gp_new(rec)
        gp_fit(rec, "fit", h, X, Y)
        nb, means, beta, theta, lo, wd = prior_arrays(D)            # (the prior takes its dimension from the fitted model)
        rec.rc("prior", lib.ibo_gp_set_prior(h, nb, dp(means), dp(beta), theta, dp(lo), dp(wd)))
        gp_state(rec, "fit", h, N, D)
        sweep(rec, "sweep", h, 130, D, EI, .01)
        loo(rec, "loo", h, N)
        grad_batch(rec, "grad", h, 65, D, EI)
    return case


def case_fit_with_matrix(rec):
    N, D = 130, 3
    X, Y = data(N, D)
    rs = np.random.RandomState(4)
    d2 = ((X[:, None, :] - X[None, :, :]) ** 2 / ell(D) ** 2).sum(2)
    A = f64(np.exp(-.5 * d2) + np.diag(1.0 + NOISE + rs.rand(N)) - np.eye(N))
    h = gp_new(rec)
    gp_fit(rec, "fit", h, X, Y, A=A)
    gp_state(rec, "fit", h, N, D)
    sweep(rec, "sweep", h, 130, D, UCB, 1.3)


def extend(rec, label, h, Xnew, Yall):
    info = ctypes.c_int(-7)
    rc = rec.rc(label, lib.ibo_gp_extend(h, len(Xnew), dp(Xnew), dp(Yall), ctypes.byref(info)))
    rec.put(label + ".info", [info.value])
    return rc


def case_extend_one(rec):
    N, D = 130, 3
    X, Y = data(N + 1, D)
    h = gp_new(rec)
    gp_fit(rec, "fit", h, f64(X[:N]), f64(Y[:N]))
    R = guard(N, N)
    rec.rc("R", lib.ibo_gp_get_R(h, dp(R)))     # R formed: the extension keeps it up to date
    extend(rec, "extend", h, f64(X[N:]), Y)
    gp_state(rec, "extended", h, N + 1, D)
    sweep(rec, "sweep", h, 130, D, EI, .01)


def case_extend_across_128(rec):
    """70 rows with head-room, then 60 more in one call: the model grows across 128 rows inside its 192-row frame"""
    N0, n, D = 70, 60, 5
    X, Y = data(N0 + n, D)
    h = gp_new(rec)
    rec.rc("reserve", lib.ibo_gp_reserve(h, 64))
    gp_fit(rec, "fit", h, f64(X[:N0]), f64(Y[:N0]))
    extend(rec, "extend", h, f64(X[N0:]), Y)
    gp_state(rec, "extended", h, N0 + n, D)
    sweep(rec, "sweep", h, 1000, D, EI, .01)


def case_remove(N, D, rows):
    def case(rec):
        h, X, Y = fitted(rec, "fit", N, D)
        keep = np.setdiff1d(np.arange(N), rows)
        r = (ctypes.c_int * len(rows))(*rows)
        info = ctypes.c_int(-7)
        rec.rc("remove", lib.ibo_gp_remove(h, len(rows), r, dp(f64(Y[keep])), ctypes.byref(info)))
        rec.put("remove.info", [info.value])
        gp_state(rec, "removed", h, N - len(rows), D)
        sweep(rec, "sweep", h, 130, D, PI, .01)
    return case


def case_set_y(rec):
    N, D = 130, 5
    h, X, Y = fitted(rec, "fit", N, D)
    _, Y2 = data(N, D, seed=21)
    rec.rc("set_y", lib.ibo_gp_set_y(h, dp(Y2)))
    batch(rec, "batch", h, 130, D)
    loo(rec, "loo", h, N)
    rec.rc("kstar_sf2", lib.ibo_gp_set_kstar_sf2(h, .8))
    batch(rec, "batch_sf2", h, 65, D)
    mu, s2 = guard(65), guard(65)
    rec.rc("posterior", lib.ibo_posterior_batch(h, 65, dp(points(65, D)), 1e-7, dp(mu), dp(s2)))
    rec.put("posterior.mu", mu); rec.put("posterior.s2", s2)


SWEEP_IMPLS = OrderedDict([("small2", (0, -1)), ("gemv", (1, -1)), ("sweep2", (2, -1)), ("split", (3, -1)), ("tile", (2, 0))])


def case_sweep(impl, N, D):
    """EI / PI / UCB over every candidate count on one sweep implementation: (sweep_path, dot_form)"""
    def case(rec):
        path, dot = SWEEP_IMPLS[impl]
        h, X, Y = fitted(rec, "fit", N, D)
        option(b"sweep_path", path); option(b"dot_form", dot)
        try:
            for acq, parm in ACQS:
                for M in MS:
                    sweep(rec, "sweep.acq%d.M%d" % (acq, M), h, M, D, acq, parm)
        finally:
            option(b"sweep_path", 0); option(b"dot_form", -1)
    return case


def state_words(rec, label, h):
    t, c = ctypes.c_int64(-7), ctypes.c_int64(-7)
    rec.rc(label + ".state", lib.ibo_sweep_state_info(h, ctypes.byref(t), ctypes.byref(c)))
    nlev, splits, at = ctypes.c_int(-7), (ctypes.c_int * 3)(-7, -7, -7), (ctypes.c_int64 * 4)(-7, -7, -7, -7)
    rec.rc(label + ".levels", lib.ibo_sweep_state_levels(h, ctypes.byref(nlev), splits, at))
    rec.put(label + ".state", [t.value, c.value, nlev.value] + list(splits) + list(at))


def kept_rounds(rec, h, X, Y, N, D, one_round):
    """three rounds on ONE candidate array: sweep, append a row, sweep, append a row, sweep"""
    M = 1000
    cand = dev_in(rec, points(M, D))
    for k in range(3):
        one_round("round%d" % k, cand, M)
        state_words(rec, "round%d" % k, h)
        if k < 2 and extend(rec, "extend%d" % k, h, f64(X[N + k:N + k + 1]), f64(Y[:N + k + 1])) != _lib.OK:
            return


def case_incremental(rec):
    N, D = 130, 3
    X, Y = data(N + 2, D)
    h = gp_new(rec)
    gp_fit(rec, "fit", h, f64(X[:N]), f64(Y[:N]))
    option(b"sweep_path", 2)                    # the kernel that keeps state (by size it serves more than 4096 candidates)
    try:
        def one_round(label, cand, M):
            for acq, parm, outs in ((EI, .01, False), (UCB, 1.3, True)):
                mu, s2, a = (dev_out(rec, M), dev_out(rec, M), dev_out(rec, M)) if outs else (None, None, None)
                bv, bi = ctypes.c_double(GUARD), ctypes.c_int64(-7)
                rec.rc(label + ".acq%d" % acq, lib.ibo_acq_sweep_incremental(
                    h, M, cand.ptr, acq, parm, 0, 1e-8, NAN, 0, None, 0.0, 0, mu and mu.ptr, s2 and s2.ptr, a and a.ptr, ctypes.byref(bv), ctypes.byref(bi)))
                rec.put(label + ".acq%d.best" % acq, [bv.value, bi.value])
                if outs:
                    for name, v in (("mu", mu), ("s2", s2), ("acq", a)):
                        read(rec, label + ".acq%d.%s" % (acq, name), v)
        kept_rounds(rec, h, X, Y, N, D, one_round)
    finally:
        option(b"sweep_path", 0)


def case_exchange(rec):
    """a communicator of ONE rank: the exchange's buffers and kernels without a second process"""
    N, D = 130, 3
    X, Y = data(N + 2, D)
    uid = ctypes.create_string_buffer(_lib.COMM_ID_BYTES)
    if rec.rc("unique_id", lib.ibo_comm_get_unique_id(uid)) != _lib.OK:
        return
    c = ctypes.c_void_p()
    if rec.rc("comm_init", lib.ibo_comm_init(0, 1, 0, uid, ctypes.byref(c))) != _lib.OK:
        return
    rec.own(lib.ibo_comm_destroy, c)
    n = ctypes.c_int(-7)
    rec.rc("count", lib.ibo_comm_count(c, ctypes.byref(n)))
    rec.put("count", [n.value])
    h = gp_new(rec)
    gp_fit(rec, "fit", h, f64(X[:N]), f64(Y[:N]))
    option(b"sweep_path", 2)
    try:
        def one_round(label, cand, M):
            for inc in (1, 0):
                lv, li, bv, bi, bx, br = ctypes.c_double(GUARD), ctypes.c_int64(-7), ctypes.c_double(GUARD), ctypes.c_int64(-7), guard(D), ctypes.c_int(-7)
                rec.rc(label + ".inc%d" % inc, lib.ibo_acq_sweep_exchange(
                    h, c, inc, M, cand.ptr, EI, .01, 0, 1e-8, NAN, 0, None, 0.0, 1000, ctypes.byref(lv), ctypes.byref(li), ctypes.byref(bv), ctypes.byref(bi),
                    dp(bx), ctypes.byref(br)))
                rec.put(label + ".inc%d.words" % inc, [lv.value, li.value, bv.value, bi.value, br.value])
                rec.put(label + ".inc%d.x" % inc, bx)
        kept_rounds(rec, h, X, Y, N, D, one_round)
    finally:
        option(b"sweep_path", 0)
    bv, bi, bp, br = ctypes.c_double(GUARD), ctypes.c_int64(-7), guard(D), ctypes.c_int(-7)
    rec.rc("argmax", lib.ibo_comm_argmax(c, 1.5, 42, dp(f64([.1, .2, .3])), D, ctypes.byref(bv), ctypes.byref(bi), dp(bp), ctypes.byref(br)))
    rec.put("argmax.words", [bv.value, bi.value, br.value]); rec.put("argmax.payload", bp)
    buf = f64(np.arange(1500.0))                # more than the buffers hold so far: they grow
    rec.rc("allreduce", lib.ibo_comm_allreduce_sum(c, dp(buf), len(buf)))
    rec.put("allreduce", buf)
    rec.rc("barrier", lib.ibo_comm_barrier(c))


def grad_batch(rec, label, h, M, D, acq):
    Q = points(M, D)
    mu, s2, a, dmu, ds2, da = guard(M), guard(M), guard(M), guard(M, D), guard(M, D), guard(M, D)
    rec.rc(label, lib.ibo_acq_grad_batch(h, M, dp(Q), acq, .01, 0, 1e-8, NAN, dp(mu), dp(s2), dp(a), dp(dmu), dp(ds2), dp(da)))
    for name, v in (("mu", mu), ("s2", s2), ("acq", a), ("dmu", dmu), ("ds2", ds2), ("dacq", da)):
        rec.put(label + "." + name, v)


def case_grad_batch(N, D):
    def case(rec):
        h, X, Y = fitted(rec, "fit", N, D)
        for M in (1, 65, 130):
            for acq in (EI, PI, UCB):
                grad_batch(rec, "grad.acq%d.M%d" % (acq, M), h, M, D, acq)
    return case


def case_posterior_cov(N, D):
    def case(rec):
        h, X, Y = fitted(rec, "fit", N, D)
        M, nsamp = 70, 5
        Q = points(M, D)
        for wn in (1, 0):
            mu, S = guard(M), guard(M, M)
            rec.rc("cov%d" % wn, lib.ibo_posterior_cov(h, M, dp(Q), wn, dp(mu), dp(S)))
            rec.put("cov%d.mu" % wn, mu); rec.put("cov%d.S" % wn, S)
        Z = f64(np.random.RandomState(8).randn(nsamp, M))
        F, mu, info = guard(nsamp, M), guard(M), ctypes.c_int(-7)
        rec.rc("sample", lib.ibo_posterior_sample(h, M, dp(Q), 1, 1e-6, nsamp, dp(Z), dp(F), dp(mu), ctypes.byref(info)))
        rec.put("sample.F", F); rec.put("sample.mu", mu); rec.put("sample.info", [info.value])
    return case


def loo(rec, label, h, N):
    mu, s2, v = guard(N), guard(N), ctypes.c_double(GUARD)
    rec.rc(label, lib.ibo_gp_loo(h, dp(mu), dp(s2), ctypes.byref(v)))
    rec.put(label + ".mu", mu); rec.put(label + ".s2", s2); rec.put(label + ".nloo", [v.value])


def ard_spec(D):
    return D, (ctypes.c_int * D)(*([0] * D)), (ctypes.c_int * D)(*range(D))


def case_likelihood(N, D):
    """ibo_gp_loo, then the stateless entries on the device's workspace: ibo_loo_grad, ibo_nlml_grad, ibo_nlml_grid over three theta"""
    def case(rec):
        h, X, Y = fitted(rec, "fit", N, D)
        loo(rec, "loo", h, N)
        ng, modes, dims = ard_spec(D)
        v, g, mu, s2 = ctypes.c_double(GUARD), guard(D), guard(N), guard(N)
        rec.rc("loo_grad", lib.ibo_loo_grad(0, _lib.K_SE_ARD, N, D, dp(X), dp(Y), dp(ell(D)), D, 1.0, NOISE, ng, modes, dims, ctypes.byref(v), dp(g), dp(mu), dp(s2)))
        rec.put("loo_grad.value", [v.value]); rec.put("loo_grad.grad", g); rec.put("loo_grad.mu", mu); rec.put("loo_grad.s2", s2)
        v, g = ctypes.c_double(GUARD), guard(D)
        rec.rc("nlml_grad", lib.ibo_nlml_grad(0, _lib.K_SE_ARD, N, D, dp(X), dp(Y), dp(ell(D)), D, 1.0, NOISE, ng, modes, dims, ctypes.byref(v), dp(g)))
        rec.put("nlml_grad.value", [v.value]); rec.put("nlml_grad.grad", g)
        thetas = f64([ell(D), ell(D)[::-1], [.3] * D])
        out = guard(3)
        rec.rc("nlml_grid", lib.ibo_nlml_grid(0, _lib.K_SE_ARD, N, D, dp(X), dp(Y), 3, dp(thetas), D, None, NOISE, dp(out)))
        rec.put("nlml_grid", out)
        rec.rc("trim", lib.ibo_trim(0))         # the workspaces go back: the next run's are new again
    return case


def case_cov_matrix(rec):
    D = 5
    A1, A2 = points(130, D), points(70, D, seed=6)
    for rule in (_lib.DIAG_UNIT_PLUS_NOISE, _lib.DIAG_KERNEL_PLUS_NOISE):
        K = guard(130, 130)
        rec.rc("square%d" % rule, lib.ibo_cov_matrix(0, _lib.K_SE_ARD, D, dp(ell(D)), D, 1.3, 130, dp(A1), 0, None, rule, NOISE, dp(K)))
        rec.put("square%d" % rule, K)
    K = guard(130, 70)
    rec.rc("cross", lib.ibo_cov_matrix(0, _lib.K_MATERN5, D, dp(f64([.5])), 1, 1.0, 130, dp(A1), 70, dp(A2), 0, 0.0, dp(K)))
    rec.put("cross", K)


def case_spd(rec):
    n, nrhs = 70, 3
    rs = np.random.RandomState(9)
    B = rs.randn(n, n)
    A = f64(B.dot(B.T) / n + np.eye(n))
    rhs, Xs, info = f64(rs.randn(nrhs, n)), guard(nrhs, n), ctypes.c_int(-7)
    rec.rc("solve", lib.ibo_spd_solve(0, n, dp(A), nrhs, dp(rhs), dp(Xs), ctypes.byref(info)))
    rec.put("solve.X", Xs); rec.put("solve.info", [info.value])
    Ai, info = guard(n, n), ctypes.c_int(-7)
    rec.rc("inverse", lib.ibo_spd_inverse(0, n, dp(A), dp(Ai), ctypes.byref(info)))
    rec.put("inverse.A", Ai); rec.put("inverse.info", [info.value])


def case_direct(N, D):
    def case(rec):
        h, X, Y = fitted(rec, "fit", N, D)
        for acq, parm in ACQS:
            lb, ub, opt, optx, ns = box(D)
            rc = lib.ibo_direct_max(h, D, dp(lb), dp(ub), acq, parm, 0, 1e-8, *(DIRECT + (ctypes.byref(opt), dp(optx), ctypes.byref(ns))))
            direct_out(rec, "direct.acq%d" % acq, rc, opt, optx, ns)
    return case


def case_legacy_fast(rec):
    """libego's symbol on the fast route: the inverse is factored on the device and the sweep kernels evaluate DIRECT's batches"""
    N, D = 70, 3
    X, Y = data(N, D)
    d2 = ((X[:, None, :] - X[None, :, :]) ** 2 / ell(D) ** 2).sum(2)
    invR = f64(np.linalg.inv(np.exp(-.5 * d2) + NOISE * np.eye(N)))
    lb, ub, one = f64(np.zeros(D)), f64(np.ones(D)), np.zeros(1)
    libc = ctypes.CDLL(None)
    libc.free.argtypes = [ctypes.c_void_p]
    option(b"legacy_exact", 0)
    try:
        for acq, parm in ACQS:
            r = lib.acqmaxGP(D, dp(lb), dp(ub), dp(invR), dp(X), dp(Y), N, acq, 0, dp(ell(D)), 0, dp(one), dp(one), 0., dp(one), dp(one), parm, NOISE, 10, 30, 10000)
            rec.put("acqmaxGP.acq%d.null" % acq, [int(not bool(r))])
            if bool(r):
                rec.put("acqmaxGP.acq%d" % acq, [r[i] for i in range(D + 1)])
                libc.free(r)
    finally:
        option(b"legacy_exact", 1)


# ---------------------------------------------------------------------------------------------- preference GP
def case_pref(rec):
    from ibo_amd.gaussianprocess import PrefGaussianProcess
    N, D, P = 130, 3, 40
    h, X, Y = fitted(rec, "fit", N, D)
    rs = np.random.RandomState(13)
    v = rs.randint(0, N, P); u = (v + 1 + rs.randint(0, N - 1, P)) % N
    lin, val = PrefGaussianProcess._pair_sum_entries(N, v, u, rs.rand(P) + .1)
    lin, val = np.ascontiguousarray(lin, dtype=np.int64), f64(val)
    if rec.rc("begin", lib.ibo_pref_begin(h)) != _lib.OK:
        return
    out = guard(N)
    rec.rc("rinv_mul", lib.ibo_pref_rinv_mul(h, dp(Y), dp(out)))
    rec.put("rinv_mul", out)
    for k in range(2):
        delta, rdelta, info = guard(N), guard(N), ctypes.c_int(-7)
        rec.rc("newton%d" % k, lib.ibo_pref_newton_step(h, len(lin), lin.ctypes.data_as(I64P), dp(val), dp(f64(rs.randn(N))), dp(delta), dp(rdelta), ctypes.byref(info)))
        rec.put("newton%d.delta" % k, delta); rec.put("newton%d.rdelta" % k, rdelta); rec.put("newton%d.info" % k, [info.value])
    info = ctypes.c_int(-7)
    rec.rc("finish", lib.ibo_pref_finish(h, len(lin), lin.ctypes.data_as(I64P), dp(val), 1.0, ctypes.byref(info)))
    rec.put("finish.info", [info.value])
    gp_state(rec, "finished", h, N, D)
    sweep(rec, "sweep", h, 130, D, EI, .01)


# ---------------------------------------------------------------------------------------------- acquisitions on several models
def three_models(rec, D=3):
    return [fitted(rec, "fit%d" % N, N, D, seed=30 + N)[0] for N in (130, 70, 200)]


def case_cacq(rec):
    D = 3
    obj, c1, c2 = three_models(rec, D)
    con = (ctypes.c_void_p * 2)(c1, c2)
    lead = (obj, 2, con, dp(f64([.2, -.1])), (ctypes.c_int * 2)(1, -1))
    for acq, parm in ((EI, .01), (PI, .01), (NONE, 0.0)):
        for M in (65, 1000):
            cand = dev_in(rec, points(M, D))
            a, p, v = dev_out(rec, M), dev_out(rec, M), dev_out(rec, M)
            bv, bi = ctypes.c_double(GUARD), ctypes.c_int64(-7)
            label = "sweep.acq%d.M%d" % (acq, M)
            rec.rc(label, lib.ibo_cacq_sweep(*(lead + (M, cand.ptr, acq, parm, 0, 1e-8, NAN, 1, dp(f64(np.full((1, D), .5))), .05, 1000, a.ptr, p.ptr, v.ptr,
                                                    ctypes.byref(bv), ctypes.byref(bi)))))
            rec.put(label + ".best", [bv.value, bi.value])
            for name, d in (("acq", a), ("pof", p), ("val", v)):
                read(rec, label + "." + name, d)
    M = 130
    Q = points(M, D)
    a, p, v = guard(M), guard(M), guard(M)
    rec.rc("batch", lib.ibo_cacq_batch(*(lead + (M, dp(Q), EI, .01, 0, 1e-8, NAN, dp(a), dp(p), dp(v)))))
    rec.put("batch.acq", a); rec.put("batch.pof", p); rec.put("batch.val", v)
    v, dv = guard(65), guard(65, D)
    rec.rc("grad", lib.ibo_cacq_grad_batch(*(lead + (65, dp(points(65, D)), EI, .01, 0, 1e-8, NAN, dp(v), dp(dv)))))
    rec.put("grad.val", v); rec.put("grad.dval", dv)
    lb, ub, opt, optx, ns = box(D)
    rc = lib.ibo_cacq_direct_max(*(lead + (D, dp(lb), dp(ub), EI, .01, 0, 1e-8, NAN) + DIRECT + (ctypes.byref(opt), dp(optx), ctypes.byref(ns))))
    direct_out(rec, "direct", rc, opt, optx, ns)


def case_kg(N, D):
    def case(rec):
        h, X, Y = fitted(rec, "fit", N, D)
        nref = 70
        ref = points(nref, D, seed=40)
        for ws in (1, 0):
            for M in (1, 130, 1000):
                cand, kg = dev_in(rec, points(M, D)), dev_out(rec, M)
                bv, bi = ctypes.c_double(GUARD), ctypes.c_int64(-7)
                label = "sweep.self%d.M%d" % (ws, M)
                rec.rc(label, lib.ibo_kg_sweep(h, nref, dp(ref), M, cand.ptr, ws, 1e-8, 1000, kg.ptr, ctypes.byref(bv), ctypes.byref(bi)))
                rec.put(label + ".best", [bv.value, bi.value])
                read(rec, label + ".kg", kg)
        M = 65
        kg, mr, mu, s2, b = guard(M), guard(nref), guard(M), guard(M), guard(M, nref)
        rec.rc("batch", lib.ibo_kg_batch(h, nref, dp(ref), M, dp(points(M, D)), 1, 1e-8, dp(kg), dp(mr), dp(mu), dp(s2), dp(b)))
        for name, v in (("kg", kg), ("mu_ref", mr), ("mu", mu), ("s2", s2), ("b", b)):
            rec.put("batch." + name, v)
        lb, ub, opt, optx, ns = box(D)
        rc = lib.ibo_kg_direct_max(h, nref, dp(ref), D, dp(lb), dp(ub), 1, 1e-8, *(DIRECT + (ctypes.byref(opt), dp(optx), ctypes.byref(ns))))
        direct_out(rec, "direct", rc, opt, optx, ns)
    return case


def case_qei(N, D):
    def case(rec):
        h, X, Y = fitted(rec, "fit", N, D)
        npend, nsamp = 3, 100
        pend = points(npend, D, seed=50)
        Z = f64(np.random.RandomState(51).randn(nsamp, npend + 1))
        lead = (h, npend, dp(pend), nsamp, dp(Z), NAN, .01, 1e-8, 1e-9)
        for M in (1, 130, 1000):
            cand, q = dev_in(rec, points(M, D)), dev_out(rec, M)
            base, bv, bi, info = ctypes.c_double(GUARD), ctypes.c_double(GUARD), ctypes.c_int64(-7), ctypes.c_int(-7)
            label = "sweep.M%d" % M
            rec.rc(label, lib.ibo_qei_sweep(*(lead + (M, cand.ptr, 1000, q.ptr, ctypes.byref(base), ctypes.byref(bv), ctypes.byref(bi), ctypes.byref(info)))))
            rec.put(label + ".words", [base.value, bv.value, bi.value, info.value])
            read(rec, label + ".qei", q)
        M = 65
        q, base, mp, Sp, mu, s2, c, info = guard(M), ctypes.c_double(GUARD), guard(npend), guard(npend, npend), guard(M), guard(M), guard(M, npend), ctypes.c_int(-7)
        rec.rc("batch", lib.ibo_qei_batch(*(lead + (M, dp(points(M, D)), dp(q), ctypes.byref(base), dp(mp), dp(Sp), dp(mu), dp(s2), dp(c), ctypes.byref(info)))))
        for name, v in (("qei", q), ("base", [base.value]), ("mu_pend", mp), ("S_pend", Sp), ("mu", mu), ("s2", s2), ("c", c), ("info", [info.value])):
            rec.put("batch." + name, v)
        lb, ub, opt, optx, ns = box(D)
        info = ctypes.c_int(-7)
        rc = lib.ibo_qei_direct_max(*(lead + (D, dp(lb), dp(ub)) + DIRECT + (ctypes.byref(opt), dp(optx), ctypes.byref(ns), ctypes.byref(info))))
        direct_out(rec, "direct", rc, opt, optx, ns)
        rec.put("direct.info", [info.value])
    return case


def case_ehvi(rec):
    D = 3
    o1, o2, _ = three_models(rec, D)
    obj = (ctypes.c_void_p * 2)(o1, o2)
    front = f64([[-.8, .9], [-.3, .6], [.1, .3], [.5, .0], [.8, -.6]])
    lead = (obj, len(front), dp(front), dp(f64([-1.5, -1.5])))
    for M in (1, 130, 1000):
        cand, v = dev_in(rec, points(M, D)), dev_out(rec, M)
        bv, bi = ctypes.c_double(GUARD), ctypes.c_int64(-7)
        label = "sweep.M%d" % M
        rec.rc(label, lib.ibo_ehvi_sweep(*(lead + (M, cand.ptr, 0, 1e-8, 1, dp(f64(np.full((1, D), .5))), .05, 1000, v.ptr, ctypes.byref(bv), ctypes.byref(bi)))))
        rec.put(label + ".best", [bv.value, bi.value])
        read(rec, label + ".val", v)
    v = guard(65)
    rec.rc("batch", lib.ibo_ehvi_batch(*(lead + (65, dp(points(65, D)), 0, 1e-8, dp(v)))))
    rec.put("batch.val", v)
    v, g = guard(65), guard(65, D)
    rec.rc("grad", lib.ibo_ehvi_grad_batch(*(lead + (65, dp(points(65, D)), 0, 1e-8, dp(v), dp(g)))))
    rec.put("grad.val", v); rec.put("grad.grad", g)
    lb, ub, opt, optx, ns = box(D)
    rc = lib.ibo_ehvi_direct_max(*(lead + (D, dp(lb), dp(ub), 0, 1e-8) + DIRECT + (ctypes.byref(opt), dp(optx), ctypes.byref(ns))))
    direct_out(rec, "direct", rc, opt, optx, ns)


def case_mes(N, D):
    def case(rec):
        h, X, Y = fitted(rec, "fit", N, D)
        K = 7
        ystar = f64(Y.max() + .05 + .3 * np.random.RandomState(60).rand(K))
        lead = (h, K, dp(ystar), 0.0)
        for M in (1, 130, 1000):
            cand, v = dev_in(rec, points(M, D)), dev_out(rec, M)
            bv, bi = ctypes.c_double(GUARD), ctypes.c_int64(-7)
            label = "sweep.M%d" % M
            rec.rc(label, lib.ibo_mes_sweep(*(lead + (M, cand.ptr, 1e-8, 1, dp(f64(np.full((1, D), .5))), .05, 1000, v.ptr, ctypes.byref(bv), ctypes.byref(bi)))))
            rec.put(label + ".best", [bv.value, bi.value])
            read(rec, label + ".val", v)
            lev, lc, st = f64([Y.max(), Y.max() + .2, Y.max() + 1.0]), guard(3), guard(2)
            rec.rc("maxcdf.M%d" % M, lib.ibo_mes_maxcdf(h, M, cand.ptr, 3, dp(lev), 0.0, 1e-8, dp(lc), dp(st)))
            rec.put("maxcdf.M%d.logcdf" % M, lc); rec.put("maxcdf.M%d.stats" % M, st)
        v = guard(65)
        rec.rc("batch", lib.ibo_mes_batch(*(lead + (65, dp(points(65, D)), 1e-8, dp(v)))))
        rec.put("batch.val", v)
        v, g = guard(65), guard(65, D)
        rec.rc("grad", lib.ibo_mes_grad_batch(*(lead + (65, dp(points(65, D)), 1e-8, dp(v), dp(g)))))
        rec.put("grad.val", v); rec.put("grad.grad", g)
        lb, ub, opt, optx, ns = box(D)
        rc = lib.ibo_mes_direct_max(*(lead + (D, dp(lb), dp(ub), 1e-8) + DIRECT + (ctypes.byref(opt), dp(optx), ctypes.byref(ns))))
        direct_out(rec, "direct", rc, opt, optx, ns)
    return case


# ---------------------------------------------------------------------------------------------- paths
def case_paths(N, D, F, prior=False):
    """F features (1: the smallest count the entry allows, and no multiple of 64) and 5 paths"""
    def case(rec):
        X, Y = data(N, D)
        h = gp_new(rec)
        gp_fit(rec, "fit", h, X, Y)
        if prior:
            nb, means, beta, theta, lo, wd = prior_arrays(D)
            rec.rc("prior", lib.ibo_gp_set_prior(h, nb, dp(means), dp(beta), theta, dp(lo), dp(wd)))
        S = 5
        rs = np.random.RandomState(70)
        omega, phase, w, eps = f64(rs.randn(F, D) / ell(D)), f64(2 * np.pi * rs.rand(F)), f64(rs.randn(S, F)), f64(np.sqrt(NOISE) * rs.randn(S, N))
        p = ctypes.c_void_p()
        if rec.rc("create", lib.ibo_paths_create(h, F, dp(omega), dp(phase), S, dp(w), dp(eps), ctypes.byref(p))) != _lib.OK:
            return
        rec.own(lib.ibo_paths_destroy, p)
        words = [ctypes.c_int(-7) for _ in range(5)]
        rec.rc("info", lib.ibo_paths_info(p, *[ctypes.byref(x) for x in words]))
        rec.put("info", [x.value for x in words])
        coef = guard(S, F + N)
        rec.rc("coef", lib.ibo_paths_coef(p, dp(coef)))
        rec.put("coef", coef)
        for M in (1, 130, 1000):
            cand, vals = dev_in(rec, points(M, D)), dev_out(rec, S, M)
            bv, bi = guard(S), np.full(S, -7, dtype=np.int64)
            label = "sweep.M%d" % M
            rec.rc(label, lib.ibo_paths_sweep(p, M, cand.ptr, 1000, vals.ptr, dp(bv), bi.ctypes.data_as(I64P)))
            rec.put(label + ".best", bv); rec.put(label + ".idx", bi)
            read(rec, label + ".values", vals)
        M = 65
        Q = points(M, D)
        vals = guard(S, M)
        rec.rc("batch", lib.ibo_paths_batch(p, M, dp(Q), dp(vals)))
        rec.put("batch", vals)
        vals, grads = guard(S, M), guard(S, M, D)
        rec.rc("grad", lib.ibo_paths_grad_batch(p, M, dp(Q), None, dp(vals), dp(grads)))
        rec.put("grad.values", vals); rec.put("grad.grads", grads)
        pof = np.ascontiguousarray(np.arange(M) % S, dtype=np.int32)
        vals, grads = guard(M), guard(M, D)
        rec.rc("grad_of", lib.ibo_paths_grad_batch(p, M, dp(Q), pof.ctypes.data_as(IP), dp(vals), dp(grads)))
        rec.put("grad_of.values", vals); rec.put("grad_of.grads", grads)
        for path in (0, S - 1):
            lb, ub, opt, optx, ns = box(D)
            rc = lib.ibo_paths_direct_max(p, path, D, dp(lb), dp(ub), *(DIRECT + (ctypes.byref(opt), dp(optx), ctypes.byref(ns))))
            direct_out(rec, "direct.path%d" % path, rc, opt, optx, ns)
    return case


# ---------------------------------------------------------------------------------------------- sparse GP
def case_sgp(N, method):
    """m = 65 inducing points; chunks of 256 observations (the option's grain): N = 300 in two, N = 600 in three, the last one partial"""
    def case(rec):
        m, D = 65, 3
        X, Y = data(N + 41, D, seed=80)
        Z = f64(X[:m] + .01)
        h = ctypes.c_void_p()
        _lib.check(lib.ibo_sgp_create(0, ctypes.byref(h)))
        rec.own(lib.ibo_sgp_destroy, h)
        option(b"sgp_chunk", 256)
        try:
            lam, info = guard(N), ctypes.c_int(-7)
            rc = rec.rc("fit", lib.ibo_sgp_fit(h, _lib.K_SE_ARD, D, dp(ell(D)), D, 1.0, NOISE, 1e-6, method, m, dp(Z), N, dp(f64(X[:N])), dp(f64(Y[:N])), dp(lam),
                                               ctypes.byref(info)))
            rec.put("fit.lambda", lam); rec.put("fit.info", [info.value])
            if rc != _lib.OK:
                return
            sgp_state(rec, "fit", h, m, method)
            for n0, n in ((N, 1), (N + 1, 40)):
                lam, info = guard(n), ctypes.c_int(-7)
                label = "add%d" % n
                rc = rec.rc(label, lib.ibo_sgp_add(h, n, dp(f64(X[n0:n0 + n])), dp(f64(Y[n0:n0 + n])), dp(lam), ctypes.byref(info)))
                rec.put(label + ".lambda", lam); rec.put(label + ".info", [info.value])
                if rc != _lib.OK:
                    return
                sgp_state(rec, label, h, m, method)
            for M in (1, 130, 1000):
                Q = points(M, D)
                mu, s2, a = guard(M), guard(M), guard(M)
                rec.rc("batch.M%d" % M, lib.ibo_sgp_acq_batch(h, M, dp(Q), EI, .01, 0, 1e-8, NAN, dp(mu), dp(s2), dp(a)))
                rec.put("batch.M%d.mu" % M, mu); rec.put("batch.M%d.s2" % M, s2); rec.put("batch.M%d.acq" % M, a)
                for acq, parm in ACQS:
                    sweep(rec, "sweep.acq%d.M%d" % (acq, M), h, M, D, acq, parm, entry=lib.ibo_sgp_acq_sweep)
            lb, ub, opt, optx, ns = box(D)
            rc = lib.ibo_sgp_direct_max(h, D, dp(lb), dp(ub), EI, .01, 0, 1e-8, *(DIRECT + (ctypes.byref(opt), dp(optx), ctypes.byref(ns))))
            direct_out(rec, "direct", rc, opt, optx, ns)
        finally:
            option(b"sgp_chunk", 0)
    return case


def sgp_state(rec, label, h, m, method):
    for what, shape in ((0, (m, m)), (1, (m, m)), (2, (m, m)), (3, (m, m)), (4, (m, m)), (5, (m,)), (6, (m,)), (7, (1,)), (8, (1,)), (9, (1,)), (10, (1,))):
        out = guard(*shape)
        rec.rc("%s.get%d" % (label, what), lib.ibo_sgp_get(h, what, dp(out)))
        rec.put("%s.get%d" % (label, what), out)
    for kind in ((0, 1) if method == 1 else (0,)):      # the model's own value; Titsias' bound, which only a DTC model has
        v = ctypes.c_double(GUARD)
        rec.rc("%s.nlml%d" % (label, kind), lib.ibo_sgp_nlml(h, kind, ctypes.byref(v)))
        rec.put("%s.nlml%d" % (label, kind), [v.value])


def case_sgp_nlml_grad(rec):
    m, D, N = 65, 3, 300
    X, Y = data(N, D, seed=80)
    Z = f64(X[:m] + .01)
    ng, modes, dims = ard_spec(D)
    option(b"sgp_chunk", 256)
    try:
        for kind in (0, 2):                     # IBO_SGP_FITC, IBO_SGP_VFE
            v, gh, gn, gZ, info = ctypes.c_double(GUARD), guard(D), ctypes.c_double(GUARD), guard(m, D), ctypes.c_int(-7)
            rec.rc("kind%d" % kind, lib.ibo_sgp_nlml_grad(0, _lib.K_SE_ARD, D, dp(ell(D)), D, 1.0, NOISE, 1e-6, kind, m, dp(Z), N, dp(X), dp(Y), ng, modes, dims,
                                                          ctypes.byref(v), dp(gh), ctypes.byref(gn), dp(gZ), ctypes.byref(info)))
            rec.put("kind%d.words" % kind, [v.value, gn.value, info.value]); rec.put("kind%d.hyper" % kind, gh); rec.put("kind%d.Z" % kind, gZ)
    finally:
        option(b"sgp_chunk", 0)
    rec.rc("trim", lib.ibo_trim(0))


# ---------------------------------------------------------------------------------------------- gradient-observation GP
def case_ggp(rec):
    N, D = 22, 3                                # P = 88 rows in a 128-row frame
    rs = np.random.RandomState(90)
    X = f64(rs.rand(N + 3, D))
    s = 3 * X.sum(1)
    Y, G = f64(np.sin(s) + .01 * rs.randn(N + 3)), f64(3 * np.cos(s)[:, None] * np.ones(D) + .01 * rs.randn(N + 3, D))
    gno = f64([1e-3] * D)
    h = ctypes.c_void_p()
    _lib.check(lib.ibo_ggp_create(0, ctypes.byref(h)))
    rec.own(lib.ibo_ggp_destroy, h)
    for label, n in (("fit", N), ("add", N + 3)):       # the model has no extension: more data are a fit of all of them, in the handle's frame
        info = ctypes.c_int(-7)
        rc = rec.rc(label, lib.ibo_ggp_fit(h, _lib.K_SE_ARD, n, D, dp(f64(X[:n])), dp(f64(Y[:n])), dp(f64(G[:n])), dp(ell(D)), D, 1.0, NOISE, dp(gno), ctypes.byref(info)))
        rec.put(label + ".info", [info.value])
        if rc != _lib.OK:
            return
        P = n * (D + 1)
        words = [ctypes.c_int(-7) for _ in range(4)]
        my = ctypes.c_double(GUARD)
        rec.rc(label + ".ggp_info", lib.ibo_ggp_info(h, *([ctypes.byref(x) for x in words] + [ctypes.byref(my)])))
        rec.put(label + ".ggp_info", [x.value for x in words] + [my.value])
        for name, get in (("R", lib.ibo_ggp_get_R), ("L", lib.ibo_ggp_get_L)):
            out = guard(P, P)
            rec.rc(label + "." + name, get(h, dp(out)))
            rec.put(label + "." + name, out)
        for M in (1, 130, 1000):
            Q = points(M, D)
            mu, s2, a = guard(M), guard(M), guard(M)
            rec.rc("%s.batch.M%d" % (label, M), lib.ibo_ggp_acq_batch(h, M, dp(Q), EI, .01, 0, 1e-8, NAN, dp(mu), dp(s2), dp(a)))
            rec.put("%s.batch.M%d.mu" % (label, M), mu); rec.put("%s.batch.M%d.s2" % (label, M), s2); rec.put("%s.batch.M%d.acq" % (label, M), a)
            for acq, parm in ACQS:
                cand = dev_in(rec, Q)
                dmu, ds2, da = dev_out(rec, M), dev_out(rec, M), dev_out(rec, M)
                bv, bi = ctypes.c_double(GUARD), ctypes.c_int64(-7)
                lab = "%s.sweep.acq%d.M%d" % (label, acq, M)
                rec.rc(lab, lib.ibo_ggp_acq_sweep(h, M, cand.ptr, acq, parm, 0, 1e-8, NAN, 1000, dmu.ptr, ds2.ptr, da.ptr, ctypes.byref(bv), ctypes.byref(bi)))
                rec.put(lab + ".best", [bv.value, bi.value])
                for name, v in (("mu", dmu), ("s2", ds2), ("acq", da)):
                    read(rec, lab + "." + name, v)
    lb, ub, opt, optx, ns = box(D)
    rc = lib.ibo_ggp_direct_max(h, D, dp(lb), dp(ub), EI, .01, 0, 1e-8, *(DIRECT + (ctypes.byref(opt), dp(optx), ctypes.byref(ns))))
    direct_out(rec, "direct", rc, opt, optx, ns)
    ng, modes, dims = ard_spec(D)
    v, g, gz = ctypes.c_double(GUARD), guard(D), guard(D + 1)
    rec.rc("nlml_grad", lib.ibo_ggp_nlml_grad(0, _lib.K_SE_ARD, N, D, dp(f64(X[:N])), dp(f64(Y[:N])), dp(f64(G[:N])), dp(ell(D)), D, 1.0, NOISE, dp(gno), ng, modes, dims,
                                              ctypes.byref(v), dp(g), dp(gz)))
    rec.put("nlml_grad.value", [v.value]); rec.put("nlml_grad.grad", g); rec.put("nlml_grad.noise", gz)
    rec.rc("trim", lib.ibo_trim(0))


# ---------------------------------------------------------------------------------------------- the table
CASES = OrderedDict()
CASES["library"] = case_library
for _N, _D in ((70, 3), (70, 5), (130, 3), (130, 5), (200, 3), (200, 5)):
    CASES["fit_%dx%d" % (_N, _D)] = case_fit(_N, _D)
for _N, _D in SHAPES:
    CASES["fit_two_level_%dx%d" % (_N, _D)] = case_fit(_N, _D, min_nb=2)
CASES["fit_prior_70x5"] = case_fit_prior(70, 5)
CASES["fit_prior_130x3"] = case_fit_prior(130, 3)
CASES["fit_with_matrix"] = case_fit_with_matrix
CASES["extend_one"] = case_extend_one
CASES["extend_across_128"] = case_extend_across_128
CASES["remove_130x3"] = case_remove(130, 3, [3, 64, 129])
CASES["remove_200x5"] = case_remove(200, 5, [0, 127, 128, 199])
CASES["set_y"] = case_set_y
for _impl in SWEEP_IMPLS:
    for _N, _D in SHAPES:
        CASES["sweep_%s_%dx%d" % (_impl, _N, _D)] = case_sweep(_impl, _N, _D)
CASES["incremental"] = case_incremental
CASES["exchange"] = case_exchange
CASES["grad_batch_70x3"] = case_grad_batch(70, 3)
CASES["grad_batch_130x5"] = case_grad_batch(130, 5)
CASES["posterior_cov_130x5"] = case_posterior_cov(130, 5)
CASES["posterior_cov_200x3"] = case_posterior_cov(200, 3)
for _N, _D in SHAPES:
    CASES["likelihood_%dx%d" % (_N, _D)] = case_likelihood(_N, _D)
CASES["cov_matrix"] = case_cov_matrix
CASES["spd"] = case_spd
CASES["direct_130x3"] = case_direct(130, 3)
CASES["direct_200x5"] = case_direct(200, 5)
CASES["legacy_fast"] = case_legacy_fast
CASES["pref"] = case_pref
CASES["cacq"] = case_cacq
CASES["kg_130x3"] = case_kg(130, 3)
CASES["kg_70x5"] = case_kg(70, 5)
CASES["qei_130x3"] = case_qei(130, 3)
CASES["qei_200x5"] = case_qei(200, 5)
CASES["ehvi"] = case_ehvi
CASES["mes_130x3"] = case_mes(130, 3)
CASES["mes_70x5"] = case_mes(70, 5)
CASES["paths_f1"] = case_paths(130, 3, 1)
CASES["paths_f65_prior"] = case_paths(70, 5, 65, prior=True)
CASES["sgp_fitc"] = case_sgp(300, 0)
CASES["sgp_dtc"] = case_sgp(300, 1)
CASES["sgp_three_chunks"] = case_sgp(600, 0)
CASES["sgp_nlml_grad"] = case_sgp_nlml_grad
CASES["ggp"] = case_ggp


def entries_called():
    """every ABI symbol this module calls (lib.NAME, or NAME handed on as an entry): read from its own source"""
    with open(__file__.rstrip("c")) as f:
        src = f.read()
    return set(re.findall(r"\blib\.(\w+)\b", src))

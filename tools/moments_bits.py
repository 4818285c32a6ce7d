#!/usr/bin/env python3
"""One SHA-256 per case over the raw bytes of what the entries on the moments pipeline return (ibo_cacq_sweep, ibo_ehvi_*, ibo_mes_*,
ibo_sgp_acq_*), through the public ABI only -- so the same file runs against any build of the library
(IBO_HIP_LIB=/path/to/libibo_hip.so) and two builds compare line for line:

    python3 tools/moments_bits.py                 every case
    python3 tools/moments_bits.py M600-c256       these cases only

Two models (40 and 300 rows, D = 3) and a sparse one (m = 70) from fixed seeds.  A case is a number of candidates and a chunk option:
every M around the small size class and the workgroup (1, 128, 129, 256, 257), 600 (at 256: two full chunks and an 88-row tail, which
needs the padded copy) and 9000 (at 4352: the large class with a padded tail).  A line folds an entry's runs without and with two
exclusion balls and a non-zero index_base into one digest; the sweeps hash every per-candidate output and the arg-max."""
import ctypes
import hashlib
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ibo_amd import _lib

CASES = [(M, c) for M in (1, 128, 129, 256, 257, 600) for c in (0, 256)] + [(9000, 0), (9000, 4352)]
CHUNK_OPTIONS = (b"cacq_chunk", b"ehvi_chunk", b"mes_chunk", b"sgp_chunk")
D, NOISE, SGP_M, INDEX_BASE, RADIUS = 3, .05, 70, 1000003, .15
ELL = np.array([.35, .45, .55])
CLAMP = _lib.CLAMP_NATIVE
I64 = ctypes.POINTER(ctypes.c_int64)
lib, check, dp = _lib.lib, _lib.check, _lib.dp


def sha(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def data(N, shift=0.0):
    rs = np.random.RandomState(2000 + N)
    X = rs.rand(N, D)
    return X, np.sin(3 * X.sum(1) + shift) + .01 * rs.randn(N)


def fitted(N, shift):
    h = ctypes.c_void_p()
    check(lib.ibo_gp_create(0, ctypes.byref(h)))
    X, Y = data(N, shift)
    info = ctypes.c_int(0)
    check(lib.ibo_gp_fit(h, _lib.K_SE_ARD, N, D, dp(X), dp(Y), dp(ELL), D, 1.0, NOISE, ctypes.byref(info)))
    return h, Y


def fitted_sparse(method):
    h = ctypes.c_void_p()
    check(lib.ibo_sgp_create(0, ctypes.byref(h)))
    X, Y = data(300)
    Z = _lib.f64(np.random.RandomState(7).rand(SGP_M, D))
    info = ctypes.c_int(0)
    check(lib.ibo_sgp_fit(h, _lib.K_SE_ARD, D, dp(ELL), D, 1.0, NOISE, 1e-6, method, SGP_M, dp(Z), 300, dp(X), dp(Y), None, ctypes.byref(info)))
    return h


def handles(*hs):
    return (ctypes.c_void_p * len(hs))(*[h.value for h in hs])


def exclusion_variants(cand):
    """(n_excl, centres, radius, index_base): none, then two balls around candidates of the set"""
    centres = _lib.f64(np.vstack([cand[0], cand[len(cand) // 2]]))
    return [(0, None, 0.0, 0), (2, dp(centres), RADIUS, INDEX_BASE)], centres


def swept(M, nout, call):
    """call(excl arguments, device outputs, best_val, best_idx) per exclusion variant -> everything it wrote"""
    out = []
    for ex in call.variants:
        dev = [_lib.DeviceArray((M,)) for _ in range(nout)]
        bv, bi = ctypes.c_double(0), ctypes.c_int64(0)
        check(call(ex, [d.ptr for d in dev], ctypes.byref(bv), ctypes.byref(bi)))
        out += [d.to_host() for d in dev] + [np.array([bv.value]), np.array([bi.value], dtype=np.int64)]
    return sha(*out)


def cacq_lines(g, cand, cdev, variants):
    M = len(cand)
    thresh, sense = _lib.f64([.2, -.1]), (ctypes.c_int * 2)(1, -1)
    for ncon in (0, 2):
        con = handles(g[40], g[40]) if ncon else None                 # one constraint handle, twice
        for acq in (_lib.ACQ_EI, _lib.ACQ_NONE):
            def call(ex, dev, bv, bi):
                return lib.ibo_cacq_sweep(g[300], ncon, con, dp(thresh) if ncon else None, sense if ncon else None, M, cdev.ptr, acq, .01,
                                          _lib.ERF_LIBM, CLAMP, float("nan"), ex[0], ex[1], ex[2], ex[3], dev[0], dev[1], dev[2], bv, bi)
            call.variants = variants
            yield "ibo_cacq_sweep ncon=%d acq=%d" % (ncon, acq), swept(M, 3, call)


def ehvi_lines(g, cand, cdev, variants):
    M = len(cand)
    front, ref = _lib.f64([[-.2, .6], [.1, .3], [.5, -.1]]), _lib.f64([-1.5, -1.5])
    for name, obj in (("two", handles(g[300], g[40])), ("same", handles(g[300], g[300]))):
        lead = (obj, len(front), dp(front), dp(ref))

        def call(ex, dev, bv, bi):
            return lib.ibo_ehvi_sweep(*(lead + (M, cdev.ptr, _lib.ERF_LIBM, CLAMP, ex[0], ex[1], ex[2], ex[3], dev[0], bv, bi)))
        call.variants = variants
        yield "ibo_ehvi_sweep %s" % name, swept(M, 1, call)
        val, val2, grad = np.empty(M), np.empty(M), np.empty((M, D))
        check(lib.ibo_ehvi_batch(*(lead + (M, dp(cand), _lib.ERF_LIBM, CLAMP, dp(val)))))
        yield "ibo_ehvi_batch %s" % name, sha(val)
        check(lib.ibo_ehvi_grad_batch(*(lead + (M, dp(cand), _lib.ERF_LIBM, CLAMP, dp(val2), dp(grad)))))
        yield "ibo_ehvi_grad_batch %s" % name, sha(val2, grad)


def mes_lines(g, ymax, cand, cdev, variants):
    M = len(cand)
    for K, off in ((1, 0.0), (64, NOISE)):
        ys = _lib.f64(ymax + .05 + .4 * np.random.RandomState(K).rand(K))
        lead = (g[300], K, dp(ys), off)

        def call(ex, dev, bv, bi):
            return lib.ibo_mes_sweep(*(lead + (M, cdev.ptr, CLAMP, ex[0], ex[1], ex[2], ex[3], dev[0], bv, bi)))
        call.variants = variants
        yield "ibo_mes_sweep K=%d" % K, swept(M, 1, call)
        val, val2, grad = np.empty(M), np.empty(M), np.empty((M, D))
        check(lib.ibo_mes_batch(*(lead + (M, dp(cand), CLAMP, dp(val)))))
        yield "ibo_mes_batch K=%d" % K, sha(val)
        check(lib.ibo_mes_grad_batch(*(lead + (M, dp(cand), CLAMP, dp(val2), dp(grad)))))
        yield "ibo_mes_grad_batch K=%d" % K, sha(val2, grad)
    for nlev in (0, 8):
        lev, logcdf, stats = _lib.f64(ymax + np.linspace(-.5, 1., 8)), np.zeros(8), np.empty(2)
        check(lib.ibo_mes_maxcdf(g[300], M, cdev.ptr, nlev, dp(lev) if nlev else None, NOISE, CLAMP, dp(logcdf) if nlev else None, dp(stats)))
        yield "ibo_mes_maxcdf nlev=%d" % nlev, sha(logcdf, stats)


def sgp_lines(sg, cand, cdev, variants):
    M = len(cand)
    for name, h in sg:
        def call(ex, dev, bv, bi):
            return lib.ibo_sgp_acq_sweep(h, M, cdev.ptr, _lib.ACQ_EI, .01, _lib.ERF_LIBM, CLAMP, float("nan"), ex[0], ex[1], ex[2], ex[3],
                                         dev[0], dev[1], dev[2], bv, bi)
        call.variants = variants
        yield "ibo_sgp_acq_sweep %s" % name, swept(M, 3, call)
        mu, s2, acq = np.empty(M), np.empty(M), np.empty(M)
        check(lib.ibo_sgp_acq_batch(h, M, dp(cand), _lib.ACQ_EI, .01, _lib.ERF_LIBM, CLAMP, float("nan"), dp(mu), dp(s2), dp(acq)))
        yield "ibo_sgp_acq_batch %s" % name, sha(mu, s2, acq)


def direct_lines(g, ymax, sg):
    lb, ub = _lib.f64([0.] * D), _lib.f64([1.] * D)
    tail = lambda: (50, 30, 200, 1, ctypes.byref(opt), dp(optx), ctypes.byref(ns))
    opt, optx, ns = ctypes.c_double(0), np.empty(D), ctypes.c_int64(0)
    thresh, sense = _lib.f64([.2, -.1]), (ctypes.c_int * 2)(1, -1)
    check(lib.ibo_cacq_direct_max(*((g[300], 2, handles(g[40], g[40]), dp(thresh), sense, D, dp(lb), dp(ub), _lib.ACQ_EI, .01, _lib.ERF_LIBM, CLAMP,
                                    float("nan")) + tail())))
    yield "ibo_cacq_direct_max", sha(np.array([opt.value]), optx, np.array([ns.value]))
    front, ref = _lib.f64([[-.2, .6], [.1, .3], [.5, -.1]]), _lib.f64([-1.5, -1.5])
    check(lib.ibo_ehvi_direct_max(*((handles(g[300], g[40]), len(front), dp(front), dp(ref), D, dp(lb), dp(ub), _lib.ERF_LIBM, CLAMP) + tail())))
    yield "ibo_ehvi_direct_max", sha(np.array([opt.value]), optx, np.array([ns.value]))
    ys = _lib.f64(ymax + .05 + .4 * np.random.RandomState(64).rand(64))
    check(lib.ibo_mes_direct_max(*((g[300], 64, dp(ys), NOISE, D, dp(lb), dp(ub), CLAMP) + tail())))
    yield "ibo_mes_direct_max", sha(np.array([opt.value]), optx, np.array([ns.value]))
    check(lib.ibo_sgp_direct_max(*((sg[0][1], D, dp(lb), dp(ub), _lib.ACQ_EI, .01, _lib.ERF_LIBM, CLAMP) + tail())))
    yield "ibo_sgp_direct_max", sha(np.array([opt.value]), optx, np.array([ns.value]))


def main():
    if _lib.device_count() < 1:
        raise SystemExit("no GPU: nothing to hash")
    want = sys.argv[1:]
    g, ymax = {}, 0.0
    for N, shift in ((40, 1.0), (300, 0.0)):
        g[N], Y = fitted(N, shift)
        ymax = float(Y.max())
    sg = [("fitc", fitted_sparse(0)), ("dtc", fitted_sparse(1))]
    for M, chunk in CASES:
        name = "M%d-c%d" % (M, chunk)
        if want and name not in want:
            continue
        cand = _lib.f64(np.random.RandomState(M).rand(M, D))
        cdev = _lib.DeviceArray.from_host(cand)
        variants, _keep = exclusion_variants(cand)
        try:
            for k in CHUNK_OPTIONS:
                check(lib.ibo_set_option(k, chunk))
            for part in (cacq_lines(g, cand, cdev, variants), ehvi_lines(g, cand, cdev, variants), mes_lines(g, ymax, cand, cdev, variants),
                         sgp_lines(sg, cand, cdev, variants)):
                for entry, digest in part:
                    print("%-12s %-30s %s" % (name, entry, digest), flush=True)
        finally:
            for k in CHUNK_OPTIONS:
                check(lib.ibo_set_option(k, 0))
    if not want or "direct" in want:
        for entry, digest in direct_lines(g, ymax, sg):
            print("%-12s %-30s %s" % ("direct", entry, digest), flush=True)


if __name__ == "__main__":
    main()

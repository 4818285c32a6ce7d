"""
The buffer-fill contract of tests/test_gpu_alloc_fill.py for the entries of include/ibo_abi_ensemble.h, which tests/alloc_fill_calls.py's table
-- held to _lib.EXPORTED -- does not list: no result of ibo_iacq_sweep, ibo_iacq_batch, ibo_iacq_grad_batch or ibo_iacq_direct_max may depend
on what a newly obtained device buffer held (the pooled scratch of the moments, the padded copy of a short launch, the partials, the staging).

Each case runs twice on a 0x00 fill (the control: it is reproducible bit for bit), then on 0xFF (every unwritten double a NaN) and on 0x7F
(every unwritten double 1.4e306, which the arg-max rule does not discard), and every run must return the bytes of the first.  S = 3 members --
the second with weight 0, so that its places in the scratch are never written -- at (N, D) = (70, 3) and (130, 5), M in {1, 65, 130, 1000}
(both sides of the padding to 160, off every 256 seam), "iacq_chunk" at its default and at 256.  Rec, first_difference, return_codes, option
and trim are alloc_fill_calls's.  ibo_iacq_stage_ms is a timing, not a result: a per-thread sum of event times on the host, left out.
"""
import ctypes

import numpy as np
import pytest

import alloc_fill_calls as calls
from alloc_fill_calls import Rec, first_difference, return_codes, option, trim

pytestmark = pytest.mark.gpu

_lib, lib, dp, f64 = calls._lib, calls.lib, calls.dp, calls.f64
GUARD, NAN = calls.GUARD, calls.NAN
MS = (1, 65, 130, 1000)
SHAPES = ((70, 3), (130, 5))
W = (.5, 0.0, 1.25)


def case(N, D, chunk):
    def run_case(rec):
        hs = [calls.fitted(rec, "fit%d" % s, N, D, seed=40 + s)[0] for s in range(3)]
        gp = (ctypes.c_void_p * 3)(*hs)
        w = f64(W)
        lead = (gp, 3, dp(w))
        option(b"iacq_chunk", chunk)
        try:
            for acq, parm in ((calls.EI, .01), (calls.UCB, 1.3)):
                tail = (acq, parm, 0, 1e-8, NAN)
                for M in MS:
                    label = "acq%d.M%d" % (acq, M)
                    cand = calls.dev_in(rec, calls.points(M, D))
                    v, m, s = calls.dev_out(rec, M), calls.dev_out(rec, M), calls.dev_out(rec, M)
                    bv, bi = ctypes.c_double(GUARD), ctypes.c_int64(-7)
                    rec.rc(label + ".sweep", lib.ibo_iacq_sweep(*(lead + (M, cand.ptr) + tail + (1, dp(f64(np.full((1, D), .5))), .05, 1000,
                                                                                              v.ptr, m.ptr, s.ptr, ctypes.byref(bv), ctypes.byref(bi)))))
                    rec.put(label + ".sweep.best", [bv.value, bi.value])
                    for name, d in (("val", v), ("mean", m), ("var", s)):
                        calls.read(rec, label + ".sweep." + name, d)
                    Q = calls.points(M, D)
                    hv, hm, hs_ = calls.guard(M), calls.guard(M), calls.guard(M)
                    rec.rc(label + ".batch", lib.ibo_iacq_batch(*(lead + (M, dp(Q)) + tail + (dp(hv), dp(hm), dp(hs_)))))
                    rec.put(label + ".batch.val", hv); rec.put(label + ".batch.mean", hm); rec.put(label + ".batch.var", hs_)
                    gv, dv = calls.guard(M), calls.guard(M, D)
                    rec.rc(label + ".grad", lib.ibo_iacq_grad_batch(*(lead + (M, dp(Q)) + tail + (dp(gv), dp(dv)))))
                    rec.put(label + ".grad.val", gv); rec.put(label + ".grad.dval", dv)
                lb, ub, opt, optx, ns = calls.box(D)
                rc = lib.ibo_iacq_direct_max(*(lead + (D, dp(lb), dp(ub)) + tail + calls.DIRECT + (ctypes.byref(opt), dp(optx), ctypes.byref(ns))))
                calls.direct_out(rec, "acq%d.direct" % acq, rc, opt, optx, ns)
        finally:
            option(b"iacq_chunk", 0)
    return run_case


CASES = {"iacq_%dx%d_chunk%d" % (N, D, chunk): case(N, D, chunk) for N, D in SHAPES for chunk in (0, 256)}


def run(name):
    """one run of a case, as alloc_fill_calls.run: [(label, itemsize, bytes)]"""
    rec = Rec()
    try:
        CASES[name](rec)
    finally:
        for destroy, h in reversed(rec.made):
            destroy(h)
    return [(label, a.dtype.itemsize, a.tobytes()) for label, a in rec.out]


def run_filled(name, byte):
    assert trim() == _lib.OK
    option(b"alloc_fill", byte)
    try:
        return run(name)
    finally:
        option(b"alloc_fill", -1)


@pytest.fixture(scope="module", autouse=True)
def device():
    if _lib.device_count() < 1:
        pytest.fail("no GPU visible: the product has no CPU fallback")
    try:
        yield
    finally:
        option(b"alloc_fill", -1)


@pytest.mark.parametrize("name", list(CASES))
def test_no_integrated_result_depends_on_what_a_new_buffer_held(name):
    first = run_filled(name, 0x00)
    bad = [(label, rc) for label, rc in return_codes(first) if rc != _lib.OK]
    assert not bad, "case '%s' is meant to succeed throughout; on a zero fill: %s (%s)" % (name, bad, lib.ibo_last_error())
    diff = first_difference(first, run_filled(name, 0x00))
    assert diff is None, "case '%s' is not reproducible on a zero fill: %s" % (name, diff)
    for byte in (0xFF, 0x7F):
        diff = first_difference(first, run_filled(name, byte))
        assert diff is None, "case '%s', new buffers filled with 0x%02X against 0x00: %s" % (name, byte, diff)


def test_the_five_entries_are_covered_or_named():
    """what tests/test_alloc_fill_table.py asks of _lib.EXPORTED, for _lib.EXPORTED_ENSEMBLE: every entry is called above, or is the timing"""
    import inspect
    src = inspect.getsource(case)
    for name in _lib.EXPORTED_ENSEMBLE:
        assert ("lib.%s(" % name in src) != (name == "ibo_iacq_stage_ms"), name

"""
No result may depend on what a newly obtained buffer held.  Every device buffer of the library comes from DevBuf::ensure (csrc/abi_internal.h)
-- the arena, the free list or the device -- as it is: zeros from the driver in a new process, the leftovers of another model in a warm one.
ibo_set_option("alloc_fill", byte) fills every such block, the arrays of ibo_dev_alloc and the pinned staging with that byte; each case of
tests/alloc_fill_calls.py (every entry that touches device memory, at the smallest shapes that have every kind of pad) runs

    twice on 0x00   the control: the case is reproducible bit for bit, so a later difference means something
    on 0xFF         every unwritten double a NaN, every int -1: a NaN runs through every sum it enters
    on 0x7F         every unwritten double 1.4e306, every int 0x7F7F7F7F: the arg-max rule discards NaN by contract, a huge finite partial wins

and every run must return the bytes of the first: values, indices, status codes, info words, DIRECT's sample counts.  ibo_trim before each
run gives the workspaces of the stateless entries back, so that each run allocates them anew.  A mismatch names the first output and index.
"""
import pytest

import alloc_fill_calls as calls

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def af():
    if calls._lib.device_count() < 1:
        pytest.fail("no GPU visible: the product has no CPU fallback")
    try:
        yield calls
    finally:
        calls.option(b"alloc_fill", -1)


def run_filled(af, name, byte):
    assert af.trim() == af._lib.OK
    af.option(b"alloc_fill", byte)
    try:
        return af.run(name)
    finally:
        af.option(b"alloc_fill", -1)


def test_the_option_takes_a_byte_or_minus_one(af):
    L = af._lib
    try:
        for v in (0, 0x7F, 255, -1):
            assert L.lib.ibo_set_option(b"alloc_fill", v) == L.OK
        for v in (-2, 256, 0x7F7F):
            assert L.lib.ibo_set_option(b"alloc_fill", v) == L.ERR_ARG
        # the hook is at work: a caller's new array reads back as the byte, whatever the driver handed out
        import ctypes
        import numpy as np
        for v in (0x7F, 0xFF, 0x00):
            af.option(b"alloc_fill", v)
            p, out = ctypes.c_void_p(), np.full(1000, af.GUARD)
            L.check(L.lib.ibo_dev_alloc(0, out.nbytes, ctypes.byref(p)))
            try:
                L.check(L.lib.ibo_memcpy_d2h(0, out.ctypes.data_as(ctypes.c_void_p), p, out.nbytes))
            finally:
                L.check(L.lib.ibo_dev_free(0, p))
            assert out.tobytes() == bytes([v]) * out.nbytes
    finally:
        af.option(b"alloc_fill", -1)


@pytest.mark.parametrize("name", list(calls.CASES))
def test_no_result_depends_on_what_a_new_buffer_held(af, name):
    first = run_filled(af, name, 0x00)
    bad = [(label, rc) for label, rc in af.return_codes(first) if rc != af._lib.OK]
    assert not bad, "case '%s' is meant to succeed throughout; on a zero fill: %s (%s)" % (name, bad, af._lib.lib.ibo_last_error())
    again = run_filled(af, name, 0x00)
    assert af.NOT_BIT_REPRODUCIBLE == {}        # (no entry is documented otherwise: the control is bit equality for every output)
    diff = af.first_difference(first, again)
    assert diff is None, "case '%s' is not reproducible on a zero fill: %s" % (name, diff)
    for byte in (0xFF, 0x7F):
        diff = af.first_difference(first, run_filled(af, name, byte))
        assert diff is None, "case '%s', new buffers filled with 0x%02X against 0x00: %s" % (name, byte, diff)

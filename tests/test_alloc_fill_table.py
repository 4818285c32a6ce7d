"""
The table of tests/alloc_fill_calls.py cannot fall behind the ABI unnoticed: every name of _lib.EXPORTED is either called by a case or listed
in NO_DEVICE_MEMORY with the reason it needs none.  No GPU: the module's own source is read.
"""
import alloc_fill_calls as calls


def test_every_entry_is_in_a_case_or_needs_no_device_memory():
    exported = set(calls._lib.EXPORTED)
    called = calls.entries_called() & exported
    listed = set(calls.NO_DEVICE_MEMORY)
    assert listed <= exported, "NO_DEVICE_MEMORY names what the ABI does not have: %s" % sorted(listed - exported)
    assert not (called & listed), "both called by a case and listed as needing no device memory: %s" % sorted(called & listed)
    assert not (exported - called - listed), "in neither a case nor NO_DEVICE_MEMORY: %s" % sorted(exported - called - listed)
    assert all(isinstance(r, str) and r.strip() and "\n" not in r for r in calls.NO_DEVICE_MEMORY.values())


def test_the_table_holds_the_shapes_with_every_kind_of_pad():
    assert calls.MS == (1, 65, 130, 1000) and {n for n, _ in calls.SHAPES} == {70, 130, 200} and {d for _, d in calls.SHAPES} == {3, 5}
    assert len(calls.CASES) == len(set(calls.CASES)) and all(callable(c) for c in calls.CASES.values())


def test_first_difference_names_the_output_and_the_index():
    import numpy as np
    a = [("x", 8, np.arange(4.0).tobytes()), ("y.rc", 8, np.array([0], dtype=np.int64).tobytes())]
    b = [("x", 8, np.array([0., 1., 2.5, 3.]).tobytes()), ("y.rc", 8, np.array([3], dtype=np.int64).tobytes())]
    assert calls.first_difference(a, a) is None
    assert "output 'x' differs first at index 2" in calls.first_difference(a, b)
    assert calls.return_codes(b) == [("y.rc", 3)]

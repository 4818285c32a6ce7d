"""
The preference workspace of ibo_pref_begin belongs to the model it was begun on (csrc/abi_pref.hip, pref_owned): this fit, this number of
rows, this padding.  After ibo_gp_extend, ibo_gp_remove or another fit of the handle, ibo_pref_rinv_mul, ibo_pref_newton_step and
ibo_pref_finish return IBO_ERR_STATE with the handle and their outputs untouched, until ibo_pref_begin is called again; the reference's
regulariser loop (ibo_pref_finish again with a larger diag after IBO_ERR_NOT_PD) keeps working.

The entries are called directly, on N = 150, D = 3 as tests/test_gpu_parity.py::test_pref_device_steps_match_dense_algebra does, and the
recovered steps are held to NumPy's dense algebra at that test's bars.  The padded size is 192 rows from the begin to every call that is
expected to be refused -- only a fit changes it (asserted: no extension or removal here refits) and the one refit is at the same N -- so
no call here -- accepted or refused, before the rule or with it -- can address outside a buffer:
a stale workspace with ANOTHER padded size is closed by reading pref_owned and is deliberately not exercised.

Before the rule: ibo_gp_extend does not advance the fit epoch (a kept sweep state survives an extension), which was all pref_check
compared, so the Newton step after an extension ran on R^-1 of the old rows with a zero row and column; ibo_pref_finish looked at
pw.ready alone, so it ran after a removal and after a refit.  Cases (i) to (iii) fail there, (iv) passes.
"""
import ctypes

import numpy as np
import pytest
from scipy.spatial.distance import cdist

from wall_time import wall

pytestmark = pytest.mark.gpu

N, D, P = 150, 3, 220
ELL, NOISE = .4, .05
GUARD = -7.25e301
I64 = ctypes.POINTER(ctypes.c_int64)


@pytest.fixture(scope="module")
def lib():
    from ibo_amd import _lib
    if _lib.device_count() < 1:
        pytest.fail("no GPU visible: the product has no CPU fallback")
    return _lib


def close(a, b, rtol, atol):
    np.testing.assert_allclose(a, b, rtol=rtol, atol=atol)


def data(seed=77):
    rs = np.random.RandomState(seed)
    return rs.rand(N + 1, D), rs.randn(N + 1), rs


def model(X, Y):
    from ibo_amd.gaussianprocess import GaussianProcess
    from ibo_amd.gaussianprocess.kernel import GaussianKernel_ard
    return GaussianProcess(GaussianKernel_ard([ELL] * D), X, Y, noise=NOISE)


def r_matrix(X):
    R = np.exp(-.5 * cdist(X / ELL, X / ELL, "sqeuclidean"))
    R[np.diag_indices(len(X))] = 1.0 + NOISE
    return R


def pairs(n, rs):
    """P pairs on n points, points that occur in several pairs among them: (v, u, rho) and the distinct entries of their sum"""
    from ibo_amd.gaussianprocess import PrefGaussianProcess
    v = rs.randint(0, n, P); u = (v + 1 + rs.randint(0, n - 1, P)) % n
    rho = rs.rand(P) + .1
    lin, val = PrefGaussianProcess._pair_sum_entries(n, v, u, rho)
    assert len(lin) < 4 * P
    return v, u, rho, lin, val


def pair_matrix(n, v, u, rho, diag):
    C = diag * np.eye(n)
    np.add.at(C, (v, v), rho); np.add.at(C, (u, u), rho)
    np.add.at(C, (v, u), -rho); np.add.at(C, (u, v), -rho)
    return C


def padded(n):
    """the padded size a fit of n rows gives the handle (stage_data: rows rounded up to 64, no rows reserved here); only a fit changes it"""
    return -(-n // 64) * 64


def newton(lib, h, n, lin, val, g):
    delta, rdelta = np.full(n, GUARD), np.full(n, GUARD)
    info = ctypes.c_int(0)
    rc = lib.lib.ibo_pref_newton_step(h, len(lin), lin.ctypes.data_as(I64), lib.dp(val), lib.dp(g), lib.dp(delta), lib.dp(rdelta), ctypes.byref(info))
    return rc, delta, rdelta


def rinv_mul(lib, h, y):
    out = np.full(len(y), GUARD)
    return lib.lib.ibo_pref_rinv_mul(h, lib.dp(y), lib.dp(out)), out


def finish(lib, h, lin, val, diag):
    info = ctypes.c_int(0)
    return lib.lib.ibo_pref_finish(h, len(lin), lin.ctypes.data_as(I64), lib.dp(val), diag, ctypes.byref(info)), info.value


def untouched(a):
    return bool(np.all(a.view(np.uint64) == np.array([GUARD]).view(np.uint64)[0]))


def refused_everywhere(lib, GP, rs, Q):
    """the three entries return IBO_ERR_STATE on GP's handle, write nothing, and leave the model's posterior bit for bit"""
    n = len(GP.X)
    h = GP._handle()
    v, u, rho, lin, val = pairs(n, rs)
    g = rs.randn(n)
    before = GP.posteriors(Q)
    rc, delta, rdelta = newton(lib, h, n, lin, val, g)
    assert rc == lib.ERR_STATE, "ibo_pref_newton_step accepted a workspace begun on another model (%d)" % rc
    assert untouched(delta) and untouched(rdelta)
    rc, out = rinv_mul(lib, h, g)
    assert rc == lib.ERR_STATE, "ibo_pref_rinv_mul accepted a workspace begun on another model (%d)" % rc
    assert untouched(out)
    rc, info = finish(lib, h, lin, val, 5.0)
    assert rc == lib.ERR_STATE, "ibo_pref_finish accepted a workspace begun on another model (%d)" % rc
    after = GP.posteriors(Q)
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])


def steps_match_dense_algebra(lib, GP, rs):
    """after a new ibo_pref_begin: the Newton step and R^-1 y against NumPy on the points the model holds now"""
    n = len(GP.X)
    h = GP._handle()
    lib.check(lib.lib.ibo_pref_begin(h))
    Rinv = np.linalg.inv(r_matrix(GP.X))
    v, u, rho, lin, val = pairs(n, rs)
    g = rs.randn(n)
    rc, delta, rdelta = newton(lib, h, n, lin, val, g)
    lib.check(rc)
    ref = -np.linalg.solve(Rinv + pair_matrix(n, v, u, rho, 0.0), g)
    close(delta, ref, rtol=1e-8, atol=1e-10); close(rdelta, Rinv.dot(ref), rtol=1e-7, atol=1e-9)
    rc, out = rinv_mul(lib, h, g)
    lib.check(rc)
    close(out, Rinv.dot(g), rtol=1e-8, atol=1e-10)


def test_extension_ends_the_workspace(lib):
    """(i) begin -> addData of one row inside the padding (no refit, asserted; 150 and 151 rows both pad to 192) -> refused; begin again ->
    the steps of the 151-row model"""
    with wall("extension"):
        X, Y, rs = data()
        Q = rs.rand(20, D)
        GP = model(X[:N], Y[:N])
        lib.check(lib.lib.ibo_pref_begin(GP._handle()))
        GP._fit_device = lambda *a, **k: pytest.fail("addData refitted: the padded size may have changed")
        try:
            GP.addData(X[N], Y[N])
        finally:
            del GP._fit_device
        assert len(GP.X) == N + 1 and padded(N + 1) == padded(N) == 192
        refused_everywhere(lib, GP, rs, Q)
        steps_match_dense_algebra(lib, GP, rs)


def test_removal_ends_the_workspace(lib):
    """(ii) begin -> removeData(7) on the device (a removal never changes the padded size) -> refused; begin again -> the steps of the
    149-row model"""
    with wall("removal"):
        X, Y, rs = data(78)
        Q = rs.rand(20, D)
        GP = model(X[:N], Y[:N])
        lib.check(lib.lib.ibo_pref_begin(GP._handle()))
        GP._fit_device = lambda *a, **k: pytest.fail("removeData refitted")
        try:
            GP.removeData(7, _route="device")
        finally:
            del GP._fit_device
        assert len(GP.X) == N - 1 and padded(N) == 192
        refused_everywhere(lib, GP, rs, Q)
        steps_match_dense_algebra(lib, GP, rs)


def test_refit_ends_the_workspace(lib):
    """(iii) begin -> a refit at the same N (the same padded size) with other data -> ibo_pref_finish refused, and the other two"""
    with wall("refit"):
        X, Y, rs = data(79)
        Q = rs.rand(20, D)
        GP = model(X[:N], Y[:N])
        lib.check(lib.lib.ibo_pref_begin(GP._handle()))
        GP.X, GP.Y = X[1:N + 1].copy(), Y[1:N + 1].copy()
        GP._fit_device()
        assert len(GP.X) == N
        v, u, rho, lin, val = pairs(N, rs)
        before = GP.posteriors(Q)
        rc, info = finish(lib, GP._handle(), lin, val, 5.0)
        assert rc == lib.ERR_STATE, "ibo_pref_finish accepted the workspace of an earlier fit (%d)" % rc
        after = GP.posteriors(Q)
        assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
        refused_everywhere(lib, GP, rs, Q)
        steps_match_dense_algebra(lib, GP, rs)


def test_regulariser_loop_keeps_its_workspace(lib):
    """(iv) begin -> ibo_pref_finish with C = -I + pairs (not positive definite, as tests/test_gpu_linalg_entries.py provokes it) ->
    IBO_ERR_NOT_PD; the call again with diag = 5 -> IBO_OK and L = chol(R + C^-1) against NumPy.  The handle is unfitted between the two
    and the epoch has not moved.  A successful finish keeps the workspace too (the same points, the same R): once more with diag = 6."""
    with wall("regulariser loop"):
        X, Y, rs = data(80)
        GP = model(X[:N], Y[:N])
        h = GP._handle()
        lib.check(lib.lib.ibo_pref_begin(h))
        v, u, rho, lin, val = pairs(N, rs)
        R = r_matrix(X[:N])
        rc, info = finish(lib, h, lin, val, -1.0)
        assert rc == lib.ERR_NOT_PD and info > 0, (rc, info)
        for diag in (5.0, 6.0):
            rc, info = finish(lib, h, lin, val, diag)
            assert (rc, info) == (lib.OK, 0), (diag, rc, info)
            L = np.empty((N, N))
            lib.check(lib.lib.ibo_gp_get_L(h, lib.dp(L)))
            close(np.tril(L), np.linalg.cholesky(R + np.linalg.inv(pair_matrix(N, v, u, rho, diag))), rtol=1e-9, atol=1e-11)
        # the model is no plain fit any more: the other two entries refuse it, as before the rule
        g = rs.randn(N)
        assert newton(lib, h, N, lin, val, g)[0] == lib.ERR_STATE and rinv_mul(lib, h, g)[0] == lib.ERR_STATE

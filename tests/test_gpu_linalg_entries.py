"""
The other callers of the factorisation kernels: ibo_spd_solve / ibo_spd_inverse (in-place launch_cholesky, then launch_trinv,
launch_pack_w, launch_alpha / launch_wtw), the info word on every route, ibo_gp_fit_with_matrix on every route (launch_pad_copy
instead of the fit's covariance pass), the preference GP's device steps on every route of pref_factor, and ibo_cov_matrix in both
forms.

The references are NumPy / SciPy in float64 (LAPACK's dpotrf for the info word); covariance entries are formed in long double.
Matrices with a controlled condition number are Q diag(s) Q^T, Q from the QR decomposition of a Gaussian matrix and s log-spaced
from 1 to 1/kappa.  The sizes are chosen for the launch shapes: one block, the block edges, 5 and 7 block columns (the ragged nodes
of launch_trinv's recursive doubling), 32 block columns (the last size of launch_cholesky's panel 1) and 33 / 35 / 65 block columns
(panel 4 with a last panel of 1 and of 3 block columns).

Host memory: below 3 GB (the 6700-row cases hold a handful of 6700 x 6700 matrices).
"""
import contextlib
import ctypes
import gc

import numpy as np
import pytest
from scipy.linalg import cho_factor, cho_solve, solve_triangular
from scipy.linalg.lapack import dpotrf
from scipy.spatial.distance import cdist

from conftest import synth

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
NOISE = 0.1
XI = 0.01
GUARD = -7.25e301              # written after every host output array; must come back untouched
NGUARD = 67


@pytest.fixture(scope="module")
def ibo():
    import ibo_amd
    from ibo_amd import _lib
    if _lib.device_count() < 1:
        pytest.fail("no GPU visible: the product has no CPU fallback")
    err = ctypes.c_double()
    _lib.check(_lib.lib.ibo_selftest_mfma(0, ctypes.byref(err)))
    return ibo_amd


def opt(key, value):
    from ibo_amd import _lib
    _lib.check(_lib.lib.ibo_set_option(key, value))


class option:
    """with option(b"key", v): ... -- the option restored to its default in `finally`"""
    DEFAULTS = {b"fused2_min_nb": 104, b"super_min_nb": 64, b"sweep_path": 0}

    def __init__(self, key, value):
        self.key, self.value = key, value

    def __enter__(self):
        opt(self.key, self.value)

    def __exit__(self, *a):
        opt(self.key, self.DEFAULTS[self.key])


def guarded(n):
    """a host output of n doubles followed by NGUARD guard values: (the whole buffer, the output view)"""
    buf = np.full(n + NGUARD, GUARD)
    return buf, buf[:n]


def guards_intact(buf, n):
    return bool(np.all(buf[n:].view(np.uint64) == np.array([GUARD]).view(np.uint64)[0]))


def same_bits(a, b):
    return np.array_equal(np.asarray(a).view(np.uint64), np.asarray(b).view(np.uint64))


def dev():
    from ibo_amd import _lib
    return _lib.default_device()


# ---------------------------------------------------------------------------------------------------- matrices
def orthogonal(N, seed):
    Q, R = np.linalg.qr(np.random.RandomState(seed).randn(N, N))
    return Q * np.sign(np.diag(R))


def conditioned(Q, kappa):
    """Q diag(s) Q^T, s log-spaced from 1 down to 1/kappa: 2-norm condition number kappa"""
    s = np.logspace(0, -np.log10(kappa), len(Q)) if len(Q) > 1 else np.ones(1)
    A = (Q * s).dot(Q.T)
    return (A + A.T) / 2


def kernel_matrix(N, seed):
    """K(X, X) + 0.1 I for SE-ARD on D = 3, and an upper bound on its condition number (Gershgorin over 0.1)"""
    X = np.random.RandomState(seed).rand(N, 3)
    A = np.exp(-.5 * cdist(X / .3, X / .3, "sqeuclidean")) + 0.1 * np.eye(N)
    return A, float(np.abs(A).sum(1).max() / 0.1)


def r_matrix(X, ell, noise=NOISE):
    """R = K(X, X) by the SE-ARD formula, diagonal 1 + noise"""
    R = np.exp(-.5 * cdist(X / ell, X / ell, "sqeuclidean"))
    R[np.diag_indices(len(X))] = 1.0 + noise
    return R


def pairs(n, P, seed):
    rs = np.random.RandomState(seed)
    v = rs.randint(0, n, P); u = (v + 1 + rs.randint(0, max(n - 1, 1), P)) % n
    return v, u, rs.rand(P) + .1


def pair_matrix(n, v, u, rho, diag):
    C = diag * np.eye(n)
    np.add.at(C, (v, v), rho); np.add.at(C, (u, u), rho)
    np.add.at(C, (v, u), -rho); np.add.at(C, (u, v), -rho)
    return C


def lapack_info(A):
    return int(dpotrf(A, lower=1, clean=0, overwrite_a=0)[1])


def make_indefinite(A, k):
    """A with its leading minor of order k + 1 strongly indefinite (and the minors before it untouched)"""
    B = A.copy()
    B[k, k] = -10.0 * np.abs(A).max()
    return B


# ---------------------------------------------------------------------------------------------------- the entry points
def spd_solve(A, B):
    from ibo_amd import _lib
    N = len(A); nrhs = len(B)
    buf, X = guarded(nrhs * N)
    info = ctypes.c_int(-1)
    rc = _lib.lib.ibo_spd_solve(dev(), N, _lib.dp(_lib.f64(A)), nrhs, _lib.dp(_lib.f64(B)), _lib.dp(X), ctypes.byref(info))
    assert guards_intact(buf, nrhs * N), "ibo_spd_solve wrote past its output (N=%d nrhs=%d)" % (N, nrhs)
    return rc, info.value, X.reshape(nrhs, N).copy()


def spd_inverse(A):
    from ibo_amd import _lib
    N = len(A)
    buf, Ai = guarded(N * N)
    info = ctypes.c_int(-1)
    rc = _lib.lib.ibo_spd_inverse(dev(), N, _lib.dp(_lib.f64(A)), _lib.dp(Ai), ctypes.byref(info))
    assert guards_intact(buf, N * N), "ibo_spd_inverse wrote past its output (N=%d)" % N
    return rc, info.value, Ai.reshape(N, N).copy()


def fnorm(A):
    return float(np.sqrt(np.sum(np.square(A, dtype=np.longdouble))))


# ---------------------------------------------------------------------------------------------------- 1. spd solve / inverse
SPD_SIZES = [1, 2, 63, 64, 65, 129, 320, 448, 2048, 2049, 2200, 4160]
# forward errors are bounded by C kappa sqrt(N) eps, the residual of the inverse by C N eps.  Worst measured on an MI355X (all sizes,
# kappa = 1e1 / 1e6 / 1e10 / the kernel matrix): solve 0.19 / 0.025 / 0.020 / 0.16 of kappa sqrt(N) eps (6.1e-16 at N = 2; 4.1e-15,
# 3.2e-11, 1.9e-7 and 1.6e-13 absolute at 2200 - 4160 rows), inverse 0.13 / 0.009 / 0.022 / 0.050 (4.3e-15, 3.3e-11, 1.8e-7, 1.6e-13 at
# 4160 rows), residual 0.5 N eps (N = 1; 0.12 from N = 2 on), A^-1 exactly symmetric everywhere.
SOLVE_C = 1.0
INV_C = 1.0
RESID_C = 1.0


@pytest.mark.parametrize("N", SPD_SIZES)
def test_spd_solve_and_inverse_across_launch_shapes(ibo, N):
    """ibo_spd_solve / ibo_spd_inverse against scipy's cho_solve and numpy's inv for kappa = 1e1, 1e6, 1e10 and a kernel matrix
    K + 0.1 I, with 1, 2 and 11 right-hand sides: forward error below C kappa sqrt(N) eps, ||A A^-1 - I|| / (||A|| ||A^-1||) below
    C N eps, A^-1 symmetric to the last bit (launch_wtw forms both triangles with the same products in the same order), nothing written past the outputs, a repeat gives the same bits."""
    from ibo_amd import _lib
    Q = orthogonal(N, N)
    Kk, kk = kernel_matrix(N, N + 1)
    cases = [("kappa=1e1", conditioned(Q, 1e1), 1e1, 11), ("kappa=1e6", conditioned(Q, 1e6), 1e6, 1),
             ("kappa=1e10", conditioned(Q, 1e10), 1e10, 2), ("K+0.1I", Kk, kk, 11)]
    del Q
    rs = np.random.RandomState(N + 2)
    for name, A, kappa, nrhs in cases:
        B = rs.randn(nrhs, N)
        rc, info, X = spd_solve(A, B)
        assert rc == _lib.OK and info == 0, (N, name, rc, info)
        Xr = cho_solve(cho_factor(A, lower=True), B.T).T
        ferr = max(np.linalg.norm(X[r] - Xr[r]) / np.linalg.norm(Xr[r]) for r in range(nrhs))
        scale = kappa * np.sqrt(N) * EPS
        assert ferr <= SOLVE_C * scale, (N, name, ferr, ferr / scale)
        rc2, _, X2 = spd_solve(A, B)
        assert rc2 == _lib.OK and same_bits(X, X2), (N, name)

        rc, info, Ai = spd_inverse(A)
        assert rc == _lib.OK and info == 0, (N, name, rc, info)
        Ar = np.linalg.inv(A)
        ferr = fnorm(Ai - Ar) / fnorm(Ar)
        resid = fnorm(A.dot(Ai) - np.eye(N)) / (fnorm(A) * fnorm(Ai))
        asym = fnorm(Ai - Ai.T) / fnorm(Ai)
        assert ferr <= INV_C * scale, (N, name, ferr, ferr / scale)
        assert resid <= RESID_C * N * EPS, (N, name, resid, resid / (N * EPS))
        assert asym == 0.0, (N, name, asym)
        rc2, _, Ai2 = spd_inverse(A)
        assert rc2 == _lib.OK and same_bits(Ai, Ai2), (N, name)
        del Ai, Ai2, Ar
    gc.collect()


# ---------------------------------------------------------------------------------------------------- 2. info and not-PD
def test_info_word_matches_lapack_on_the_spd_entries(ibo):
    """A PD matrix with its leading minor k + 1 made strongly indefinite: ibo_spd_solve and ibo_spd_inverse return IBO_ERR_NOT_PD and
    info equal to LAPACK dpotrf's, for k at the first pivot, around the first block edge and in a later panel of the panel-4 route
    (2200 rows); the next call with the PD matrix is right"""
    from ibo_amd import _lib
    for N, ks in ((200, (0, 62, 63, 64, 65, 190)), (2200, (0, 63, 64, 1500, 2199))):
        A, _ = kernel_matrix(N, 3 * N)
        B = np.random.RandomState(N).randn(2, N)
        for k in ks:
            Abad = make_indefinite(A, k)
            want = lapack_info(Abad)
            assert want == k + 1
            rc, info, _ = spd_solve(Abad, B)
            assert (rc, info) == (_lib.ERR_NOT_PD, want), (N, k, rc, info)
            rc, info, _ = spd_inverse(Abad)
            assert (rc, info) == (_lib.ERR_NOT_PD, want), (N, k, rc, info)
        rc, info, X = spd_solve(A, B)
        assert rc == _lib.OK and info == 0
        Xr = cho_solve(cho_factor(A, lower=True), B.T).T
        assert np.abs(X - Xr).max() <= 1e-11 * np.abs(Xr).max()
        rc, info, Ai = spd_inverse(A)
        assert rc == _lib.OK and info == 0
        Ar = np.linalg.inv(A)
        assert np.abs(Ai - Ar).max() <= 1e-11 * np.abs(Ar).max()


def gp_of(X, Y, ell):
    from ibo_amd.gaussianprocess import GaussianProcess
    from ibo_amd.gaussianprocess.kernel import GaussianKernel_ard
    return GaussianProcess(GaussianKernel_ard(np.asarray(ell, float)), X, Y, noise=NOISE)


def fit_with_matrix(GP, A):
    """ibo_gp_fit_with_matrix on GP's handle with GP's data: (rc, info)"""
    from ibo_amd import _lib
    ktype, hyper, sf2, _ = GP.kernel._ibo_spec()
    X = _lib.f64(GP.X); Y = _lib.f64(GP.Y)
    info = ctypes.c_int(-1)
    rc = _lib.lib.ibo_gp_fit_with_matrix(GP._handle(), ktype, len(X), X.shape[1], _lib.dp(X), _lib.dp(Y), _lib.dp(hyper), len(hyper),
                                         sf2, NOISE, _lib.dp(_lib.f64(A)), ctypes.byref(info))
    return rc, info.value


def sweep_rc(GP, cand):
    from ibo_amd.acquisition import sweep
    from ibo_amd import _lib
    try:
        sweep(GP, cand, acq='ei', xi=XI)
    except _lib.IBOError as e:
        return e.code
    return _lib.OK


@pytest.mark.parametrize("route", ["single", "super", "two_level"])
def test_info_word_and_state_after_fit_with_matrix_not_pd(ibo, route):
    """ibo_gp_fit_with_matrix of a matrix whose leading minor k + 1 is strongly indefinite, in the single-level order (700 rows), in
    super-panels (super_min_nb = 32, 2100 rows) and in the two-level order (fused2_min_nb = 33, 2100 rows): IBO_ERR_NOT_PD, info equal to
    LAPACK dpotrf's, the handle unfitted (a sweep returns IBO_ERR_STATE); the next fit with a good matrix gives chol(A)"""
    from ibo_amd import _lib
    N, key, val = {"single": (700, None, None), "super": (2100, b"super_min_nb", 32), "two_level": (2100, b"fused2_min_nb", 33)}[route]
    X, Y = synth(5, N, 4)
    ell = [.4] * 4
    A = r_matrix(X, ell) + 0.5 * np.eye(N)
    cand = np.random.RandomState(1).rand(20, 4)
    with option(key, val) if key else contextlib.nullcontext():
        GP = gp_of(X, Y, ell)
        for k in (0, 62, 63, 64, 65, N - 100, N - 1):
            Abad = make_indefinite(A, k)
            want = lapack_info(Abad)
            assert want == k + 1
            rc, info = fit_with_matrix(GP, Abad)
            assert (rc, info) == (_lib.ERR_NOT_PD, want), (route, k, rc, info)
            assert sweep_rc(GP, cand) == _lib.ERR_STATE, (route, k)
        rc, info = fit_with_matrix(GP, A)
        assert rc == _lib.OK and info == 0
        L = np.array(GP.L)
    assert np.abs(L - np.linalg.cholesky(A)).max() < 1e-11


# ---------------------------------------------------------------------------------------------------- 3. fit with a matrix
def get_W(GP):
    from ibo_amd import _lib
    N = len(GP.X)
    buf, W = guarded(N * N)
    _lib.check(_lib.lib.ibo_gp_get_W(GP._handle(), _lib.dp(W)))
    assert guards_intact(buf, N * N)
    return W.reshape(N, N).copy()


def get_R(GP):
    from ibo_amd import _lib
    N = len(GP.X)
    buf, R = guarded(N * N)
    _lib.check(_lib.lib.ibo_gp_get_R(GP._handle(), _lib.dp(R)))
    assert guards_intact(buf, N * N)
    return R.reshape(N, N).copy()


def sweep_outputs(GP, cand):
    from ibo_amd.acquisition import sweep
    return sweep(GP, cand, acq='ei', xi=XI, native=True, outputs=("mu", "s2", "acq"))


FIT_CASES = [(1, None, None), (65, None, None), (700, None, None), (2113, b"fused2_min_nb", 33), (4100, None, None), (6700, None, None)]


@pytest.mark.parametrize("N,key,val", FIT_CASES, ids=["n1", "n65", "n700", "n2113-two-level", "n4100-super", "n6700-two-level"])
def test_fit_with_matrix_on_every_route(ibo, N, key, val):
    """ibo_gp_fit_with_matrix(A = R + C^-1, C = 5 I + random pairs): L against numpy's cholesky(A), W L = I on probe rows; mu = k*^T A^-1 y
    and sigma^2 = clip(1 + noise - k*^T A^-1 k*) on the small-batch, large-batch and GEMV kernels; ibo_gp_get_R still returns K(X, X) with
    diagonal 1 + noise; ibo_gp_extend and ibo_pref_begin refuse with IBO_ERR_STATE and change nothing; at 4100 rows L and W are bit-equal
    to the step-by-step order (super_min_nb = 1000).  Worst measured on an MI355X (6700 rows): L 6.0e-15, W L - I 4.0e-15, mu 9.2e-15,
    sigma^2 3.3e-14 relative; the kernels are wk_small_kernel, sweep2_kernel and sweep_gemv_kernel at every size."""
    from ibo_amd import _lib
    D = 4
    ell = np.array([.35, .4, .45, .5])
    X, Y = synth(N + 11, N, D)
    R = r_matrix(X, ell)
    v, u, rho = pairs(N, max(1, N // 3), N)
    A = R + np.linalg.inv(pair_matrix(N, v, u, rho, 5.0))
    A = (A + A.T) / 2
    Lr = np.linalg.cholesky(A)
    with option(key, val) if key else contextlib.nullcontext():
        GP = gp_of(X, Y, ell)
        rc, info = fit_with_matrix(GP, A)
        assert rc == _lib.OK and info == 0
        L = np.array(GP.L)
        W = get_W(GP)
        Rg = get_R(GP)
    errL = np.abs(L - Lr).max()
    probe = np.unique(np.r_[np.random.RandomState(N).randint(0, N, 200), np.arange(max(0, N - 16), N)])
    errW = np.abs(W[probe].dot(L) - np.eye(N)[probe]).max()
    assert errL < 1e-11 and np.abs(np.triu(L, 1)).max() == 0.0, (N, errL)
    assert errW < 1e-10 and np.all(np.triu(W, 1) == 0.0), (N, errW)
    assert np.array_equal(Rg, Rg.T) and np.all(np.diag(Rg) == 1.0 + NOISE)
    assert np.abs(Rg - R).max() <= 1e-13, (N, np.abs(Rg - R).max())
    if N == 4100:
        with option(b"super_min_nb", 1000):
            GP1 = gp_of(X, Y, ell)
            rc, info = fit_with_matrix(GP1, A)
            assert rc == _lib.OK
            assert np.array_equal(np.array(GP1.L), L) and np.array_equal(get_W(GP1), W)
        del GP1
    del W, Rg
    gc.collect()
    # the posterior: k* in long double, alpha and L^-1 k* from the reference factor
    rs = np.random.RandomState(N + 5)
    cand = np.vstack([X[-8:], X[-8:] + 1e-3, rs.rand(5000 - 16, D)])
    alpha = cho_solve((Lr, True), Y)

    def ref(Q):
        ks = np.exp(-.5 * (((X[:, None, :].astype(np.longdouble) - Q[None, :, :]) / ell) ** 2).sum(-1))
        vv = solve_triangular(Lr, ks.astype(np.float64), lower=True, check_finite=False)
        mu = (ks * alpha.astype(np.longdouble)[:, None]).sum(0)
        s2 = np.longdouble(1.0 + NOISE) - (vv.astype(np.longdouble) ** 2).sum(0)
        return mu.astype(np.float64), np.clip(s2.astype(np.float64), 1e-8, 10.0)
    idx = np.r_[np.arange(64), np.arange(64, 5000, 97)]
    mu_r, s2_r = ref(cand[idx])
    kernels = {}
    for tag, c, path in (("small", cand[:300], 0), ("large", cand, 0), ("gemv", cand[:16], 1)):
        with option(b"sweep_path", path):
            r = sweep_outputs(GP, c)
        kernels[tag] = r["kernel"]
        sel = idx[idx < len(c)]
        emu = np.abs(r["mu"][sel] - mu_r[:len(sel)]).max(); es2 = np.abs(r["s2"][sel] / s2_r[:len(sel)] - 1).max()
        assert emu <= 1e-12 and es2 <= 1e-11, (N, tag, r["kernel"], emu, es2)
        if tag == "large":
            before = r
    assert kernels["small"] == "wk_small_kernel" and kernels["large"] == "sweep2_kernel" and kernels["gemv"] == "sweep_gemv_kernel", kernels
    # what the header says the handle refuses after a fit from a matrix, and that nothing changed
    info = ctypes.c_int(0)
    xn = np.random.RandomState(3).rand(1, D); yall = np.r_[Y, 0.5]
    assert _lib.lib.ibo_gp_extend(GP._handle(), 1, _lib.dp(xn), _lib.dp(yall), ctypes.byref(info)) == _lib.ERR_STATE
    assert _lib.lib.ibo_pref_begin(GP._handle()) == _lib.ERR_STATE
    after = sweep_outputs(GP, cand)
    assert all(same_bits(before[k], after[k]) for k in ("mu", "s2", "acq")) and after["best_idx"] == before["best_idx"]
    gc.collect()


# ---------------------------------------------------------------------------------------------------- 4. preference steps
PREF_CASES = [(150, 3), (1000, 16), (4100, None), (6700, None)]


@pytest.mark.parametrize("n,min_nb", PREF_CASES, ids=["n150-two-level-3", "n1000-two-level-16", "n4100-super-fit", "n6700-two-level"])
def test_pref_device_steps_on_every_route(ibo, n, min_nb):
    """test_pref_device_steps_match_dense_algebra on the other routes of pref_factor: the two-level order at 3 and 16 block columns
    (fused2_min_nb lowered), the step-by-step order on a model fitted in super-panels (4100 rows), the default two-level order with the
    in-place packed update (6700 rows).  delta, R^-1 delta, R^-1 y and the L of ibo_pref_finish against dense algebra; ibo_pref_finish
    with diag = -1 (C not positive definite) returns IBO_ERR_NOT_PD with LAPACK's info for C, and a retry with diag = 5 succeeds.
    Worst measured on an MI355X (norm-wise relative): delta 1.9e-13, R^-1 delta 2.0e-13, R^-1 y 2.8e-13; L 6.7e-15 (4100 rows)."""
    from ibo_amd import _lib
    from ibo_amd.gaussianprocess import PrefGaussianProcess
    D = 3
    ell = [.4] * D
    X, Y = synth(n + 21, n, D)
    P = max(220, n // 2)
    v, u, rho = pairs(n, P, n + 1)
    lin, val = PrefGaussianProcess._pair_sum_entries(n, v, u, rho)
    i64 = ctypes.POINTER(ctypes.c_int64)
    g = np.random.RandomState(n).randn(n)
    with option(b"fused2_min_nb", min_nb or 104):
        GP = gp_of(X, Y, ell)
        h = GP._handle()
        _lib.check(_lib.lib.ibo_pref_begin(h))
        R = r_matrix(X, ell)
        Lr = np.linalg.cholesky(R)
        Rinv = cho_solve((Lr, True), np.eye(n))
        H = Rinv + pair_matrix(n, v, u, rho, 0.0)
        delta = np.empty(n); rdelta = np.empty(n); out = np.empty(n); info = ctypes.c_int(-1)
        _lib.check(_lib.lib.ibo_pref_newton_step(h, len(lin), lin.ctypes.data_as(i64), _lib.dp(val), _lib.dp(g), _lib.dp(delta),
                                                 _lib.dp(rdelta), ctypes.byref(info)))
        assert info.value == 0
        dref = -np.linalg.solve(H, g)
        rdref = cho_solve((Lr, True), dref)
        _lib.check(_lib.lib.ibo_pref_rinv_mul(h, _lib.dp(Y), _lib.dp(out)))
        ryref = cho_solve((Lr, True), Y)
        e_d = np.linalg.norm(delta - dref) / np.linalg.norm(dref)
        e_rd = np.linalg.norm(rdelta - rdref) / np.linalg.norm(rdref)
        e_ry = np.linalg.norm(out - ryref) / np.linalg.norm(ryref)
        assert e_d <= 1e-11 and e_rd <= 1e-11 and e_ry <= 1e-11, (n, e_d, e_rd, e_ry)
        del H, Rinv
        # C = -I + pairs is not positive definite: the reference's regulariser loop adds to the diagonal and tries again
        Cbad = pair_matrix(n, v, u, rho, -1.0)
        rc = _lib.lib.ibo_pref_finish(h, len(lin), lin.ctypes.data_as(i64), _lib.dp(val), -1.0, ctypes.byref(info))
        assert (rc, info.value) == (_lib.ERR_NOT_PD, lapack_info(Cbad)), (n, rc, info.value, lapack_info(Cbad))
        _lib.check(_lib.lib.ibo_pref_finish(h, len(lin), lin.ctypes.data_as(i64), _lib.dp(val), 5.0, ctypes.byref(info)))
        assert info.value == 0
        L = np.array(GP.L)
    C = pair_matrix(n, v, u, rho, 5.0)
    Lf = np.linalg.cholesky(R + np.linalg.inv(C))
    e_L = np.abs(np.tril(L) - Lf).max()
    assert e_L <= 1e-11 and np.abs(np.triu(L, 1)).max() == 0.0, (n, e_L)
    gc.collect()


# ---------------------------------------------------------------------------------------------------- 5. cov matrix
KERNELS = [("ard", None), ("svard", 1.7), ("iso", None), ("sviso", 0.6), ("m3", 1.3), ("m5", 0.8)]


def kern_args(kind, mag, D):
    """(oracle.Kern, ktype, hyper handed to ibo_cov_matrix, sf2): length scales ~ sqrt(D) / 2"""
    from oracle import oracle as orc
    ls = 0.5 * np.sqrt(D) * np.linspace(.8, 1.2, D)
    if kind in ("ard", "svard"):
        hyper = list(ls) + ([mag] if mag else [])
    else:
        hyper = [ls[0]] + ([mag] if mag else [])
    k = orc.Kern(kind, hyper)
    return k, k.ktype, np.asarray(k.theta if kind in ("ard", "svard") else k.hyper[:1], float), k.sf2_py


def cov_ref(k, A, B):
    """the oracle's formulas (Kern.cov) on every pair at once, in long double"""
    A = np.asarray(A, np.longdouble); B = np.asarray(B, np.longdouble)
    diff = A[:, None, :] - B[None, :, :]
    th = np.asarray(k.theta, np.longdouble)
    if k.kind in ("ard", "svard"):
        v = np.exp(-.5 * ((diff / th) ** 2).sum(-1))
    elif k.kind in ("iso", "sviso"):
        v = np.exp(-.5 * (diff ** 2).sum(-1) / th[0] ** 2)
    elif k.kind == "m3":
        z = np.sqrt(np.longdouble(3)) * np.sqrt((diff ** 2).sum(-1)) / th[0]
        v = (1 + z) * np.exp(-z)
    else:
        z = np.sqrt(((np.sqrt(np.longdouble(5)) * diff / th[0]) ** 2).sum(-1))
        v = np.exp(-z) * (1 + z + z * z / 3)
    return (np.longdouble(k.sf2_py) * v).astype(np.float64)


def cov_matrix(ktype, D, hyper, sf2, A1, A2, diag_rule=0, noise=0.0):
    from ibo_amd import _lib
    n1 = len(A1); n2 = len(A2) if A2 is not None else n1
    buf, K = guarded(n1 * n2)
    rc = _lib.lib.ibo_cov_matrix(dev(), ktype, D, _lib.dp(hyper), len(hyper), sf2, n1, _lib.dp(_lib.f64(A1)), n2 if A2 is not None else 0,
                                 None if A2 is None else _lib.dp(_lib.f64(A2)), diag_rule, noise, _lib.dp(K))
    _lib.check(rc)
    assert guards_intact(buf, n1 * n2), (n1, n2)
    return K.reshape(n1, n2).copy()


@pytest.mark.parametrize("D", [1, 4, 32, 33, 64])
def test_cov_matrix_cross_and_square_forms(ibo, D):
    """ibo_cov_matrix against the oracle's kernel formulas in long double at 1e-12 relative: every kernel type (SV kernels and Matern
    with sf2 != 1), the cross form K(A1, A2) at (n1, n2) among 1, 63, 64, 65, 130, the square form with both diagonal rules, the cross
    form of a set with itself (sf2 on the diagonal, no rule); the formula itself checked against oracle.Kern.cov entry by entry"""
    rs = np.random.RandomState(D)
    P = rs.rand(260, D)
    shapes = [(1, 130), (63, 64), (64, 65), (65, 1), (130, 63), (1, 1)]
    for kind, mag in KERNELS:
        k, ktype, hyper, sf2 = kern_args(kind, mag, D)
        ref = cov_ref(k, P[:5], P[5:9])
        for i in range(5):
            for j in range(4):
                assert abs(ref[i, j] - k.cov(P[i], P[5 + j])) <= 1e-13 * abs(ref[i, j]) + 1e-300, (kind, D)
        for n1, n2 in shapes:
            A1, A2 = P[:n1], P[130:130 + n2]
            K = cov_matrix(ktype, D, hyper, sf2, A1, A2)
            np.testing.assert_allclose(K, cov_ref(k, A1, A2), rtol=1e-12, atol=1e-300, err_msg="%s D=%d %dx%d" % (kind, D, n1, n2))
        A1 = P[:130]
        Kx = cov_matrix(ktype, D, hyper, sf2, A1, A1)                   # the cross form of a set with itself: no diagonal rule
        Kr = cov_ref(k, A1, A1)
        np.testing.assert_allclose(Kx, Kr, rtol=1e-12, atol=1e-300, err_msg="%s D=%d self" % (kind, D))
        assert np.all(np.diag(Kx) == sf2), (kind, D)
        for rule, noise, dval in ((0, 0.1, 1.1), (1, 0.1, sf2 + 0.1), (1, 0.0, sf2)):
            Ks = cov_matrix(ktype, D, hyper, sf2, A1, None, rule, noise)
            off = ~np.eye(130, dtype=bool)
            np.testing.assert_allclose(Ks[off], Kr[off], rtol=1e-12, atol=1e-300, err_msg="%s D=%d rule %d" % (kind, D, rule))
            assert np.allclose(np.diag(Ks), dval, rtol=1e-15, atol=0), (kind, D, rule, np.diag(Ks)[:3], dval)


def test_cov_matrix_refuses_bad_sizes(ibo):
    """n1 < 1, and n2 < 1 with A2 given, return IBO_ERR_ARG (a negative n2 used to reach the allocation and come back as a HIP error);
    the next call is right"""
    from ibo_amd import _lib
    A = np.random.RandomState(0).rand(4, 2)
    K = np.empty(16)
    hyper = np.array([.5])
    for n1, n2 in ((0, 4), (-1, 4), (4, 0), (4, -3)):
        assert _lib.lib.ibo_cov_matrix(dev(), 1, 2, _lib.dp(hyper), 1, 1.0, n1, _lib.dp(A), n2, _lib.dp(A), 0, 0.0, _lib.dp(K)) == _lib.ERR_ARG, (n1, n2)
    k, ktype, hyper, sf2 = kern_args("iso", None, 2)
    np.testing.assert_allclose(cov_matrix(ktype, 2, hyper, sf2, A, A), cov_ref(k, A, A), rtol=1e-12)

"""
Large models: the kernels at the sizes where their limits lie -- 64 KiB of LDS in the GEMV kernel (8192 rows), the last
size whose packed matrices fit a 2 GiB buffer descriptor (16320 rows), 16384 rows where the packed W is exactly 2^31
bytes, the first size beyond the large-batch kernel (16385), the last size the GEMV kernel's LDS holds (20416) and
one past it, the super-panel order and the NLML's packed product moved past 2 GiB by an option.

The reference is the oracle's posterior restated in NumPy/LAPACK (ref_post, ref_nlml below; the oracle's C loops cannot
run at these sizes): R from the kernel formula with diagonal 1 + noise, numpy.linalg.cholesky (what the reference
itself uses, ego/gaussianprocess/__init__.py:299), cho_solve / solve_triangular for alpha and L^-1 k*, sigma^2 clamped
as oracle.sweep_native clamps it, EI through oracle.acq_value, the NLML and its gradient as in
ego/gaussianprocess/trainhyper.py:47-95.  k* and the final sums are in long double.  float64 BLAS / LAPACK does the
O(N^2) and O(N^3) work: R is formed by differences (cdist), and with noise 0.1 the models here have condition numbers
below ~5e4, so the reference's own error in mu and sigma^2 is below ~1e-10 relative -- four orders under RT.  The
helper is pinned against the oracle at 1e-12 (test_reference_helper_agrees_with_the_oracle).

All models are prefixes of ONE data set of 20481 rows (D = 8, SE-ARD), so one NumPy Cholesky of its R serves every
SE-ARD size (the leading block of a Cholesky factor is the factor of the leading block).

Host memory: about 12 GB at the peak (the 20481-row factor, 3.4 GB, is kept for the module; a 16384-row L and W
fetched from the device take 2.1 GB each).
"""
import ctypes
import gc

import numpy as np
import pytest
from scipy.linalg import cho_solve, solve_triangular
from scipy.linalg.lapack import dpotri
from scipy.spatial.distance import cdist

from conftest import synth

pytestmark = pytest.mark.gpu

RT = 1e-6
ACQ_ATOL = 1e-12
NOISE = 0.1
XI = 0.01
D = 8
ELL = np.linspace(.4, .6, D)          # SE-ARD length scales
NBIG = 20481


@pytest.fixture(scope="module")
def ibo():
    import ibo_amd
    from ibo_amd import _lib
    if _lib.device_count() < 1:
        pytest.fail("no GPU visible: the product has no CPU fallback")
    err = ctypes.c_double()
    _lib.check(_lib.lib.ibo_selftest_mfma(0, ctypes.byref(err)))
    return ibo_amd


def close(a, b, rtol=RT, atol=1e-12):
    np.testing.assert_allclose(a, b, rtol=rtol, atol=atol)


def opt(key, value):
    from ibo_amd import _lib
    _lib.check(_lib.lib.ibo_set_option(key, value))


# ---------------------------------------------------------------------------------------------------- the reference
def cov_block(kind, hyper, A, B, dtype=np.float64):
    """K(A, B) by the oracle's formulas (oracle/ibo_oracle.c orc_cov): 'ard' (length scales), 'm3' / 'm5' ([l, magnitude])"""
    A = np.asarray(A, dtype); B = np.asarray(B, dtype)
    if dtype == np.float64:
        if kind == "ard":
            z = cdist(A / np.asarray(hyper), B / np.asarray(hyper), "sqeuclidean")
            return np.exp(-.5 * z)
        r = cdist(A, B, "euclidean")
    else:
        if kind == "ard":
            h = np.asarray(hyper, dtype)
            z = (((A[:, None, :] - B[None, :, :]) / h) ** 2).sum(-1)
            return np.exp(-.5 * z)
        r = np.sqrt(((A[:, None, :] - B[None, :, :]) ** 2).sum(-1))
    ell, sf2 = np.asarray(hyper[0], dtype), np.asarray(hyper[1] ** 2, dtype)
    if kind == "m3":
        z = np.sqrt(np.asarray(3.0, dtype)) * r / ell
        return sf2 * (1 + z) * np.exp(-z)
    z = np.sqrt(np.asarray(5.0, dtype)) * r / ell
    return sf2 * (1 + z + z * z / 3) * np.exp(-z)


def r_matrix(kind, hyper, X, noise=NOISE, rows=2048):
    """R = K(X, X) with the reference's diagonal 1 + noise (ego/gaussianprocess/__init__.py:134-149)"""
    N = len(X)
    R = np.empty((N, N))
    for i in range(0, N, rows):
        R[i:i + rows] = cov_block(kind, hyper, X[i:i + rows], X)
    R[np.diag_indices(N)] = 1.0 + noise
    return R


class Ref:
    """The posterior of oracle.GP / oracle.sweep_native from a Cholesky factor L (lower, float64)."""

    def __init__(self, kind, hyper, X, Y, L, noise=NOISE):
        self.kind, self.hyper, self.X, self.Y, self.noise = kind, hyper, X, np.asarray(Y, float), noise
        self.L = np.asfortranarray(L)
        self.alpha = cho_solve((self.L, True), self.Y, check_finite=False)
        self.maxY = float(np.max(self.Y))

    def post(self, Q, clamp_lo=1e-8):
        Q = np.atleast_2d(Q)
        mu = np.empty(len(Q)); s2 = np.empty(len(Q))
        for c in range(0, len(Q), 16):
            ks = cov_block(self.kind, self.hyper, self.X, Q[c:c + 16], np.longdouble)            # (N, m), long double
            v = solve_triangular(self.L, ks.astype(np.float64), lower=True, check_finite=False)
            mu[c:c + 16] = (ks * self.alpha.astype(np.longdouble)[:, None]).sum(0)
            s2[c:c + 16] = np.longdouble(1.0 + self.noise) - (v.astype(np.longdouble) ** 2).sum(0)
        return mu, np.clip(s2, clamp_lo, 10.0)

    def sweep(self, Q):
        from oracle import oracle as orc
        mu, s2 = self.post(Q)
        return mu, s2, orc.acq_value(orc.ACQ_EI, orc.ERF_LIBM, mu, np.sqrt(s2), self.maxY, XI)


def ref_nlml(kind, hyper, X, Y, L, noise=NOISE, rows=2048):
    """the NLML and its gradient w.r.t. the log hyperparameters as oracle.marginal_likelihood (trainhyper.py:47-95) for K = R, from L"""
    N = len(X)
    Y = np.asarray(Y, float)
    L = np.asfortranarray(L)
    alpha = cho_solve((L, True), Y, check_finite=False)
    v = 0.5 * float(np.dot(Y.astype(np.longdouble), alpha.astype(np.longdouble))) + float(np.log(np.diag(L).astype(np.longdouble)).sum()) \
        + 0.5 * N * np.log(2.0 * np.pi)
    Ki, info = dpotri(L, lower=1, overwrite_c=0)
    assert info == 0
    nh = len(hyper) if kind == "ard" else 2
    g = np.zeros(nh, np.longdouble)
    for i in range(0, N, rows):                          # A = K^-1 - alpha alpha^T, one block of rows at a time (K^-1 from its lower half)
        j = slice(i, min(N, i + rows))
        A = np.tril(Ki[j], i) + np.triu(Ki[:, j].T, i + 1) - np.outer(alpha[j], alpha)
        K = cov_block(kind, hyper, X[j], X)
        if kind == "ard":
            for d in range(nh):
                C = ((X[j, d, None] - X[None, :, d]) / hyper[d]) ** 2
                g[d] += np.sum((A * K * C).astype(np.longdouble))
        else:
            r = cdist(X[j], X, "euclidean")
            C = hyper[1] ** 2 * r ** 2 * np.exp(-r)          # the oracle's dK/dlog(theta_0) for Matern-3/2 (oracle.Kern.derivative)
            C[np.arange(j.stop - j.start), np.arange(j.start, j.stop)] = 0.0
            g[0] += np.sum((A * C).astype(np.longdouble))
            g[1] += np.sum((A * 2.0 * K).astype(np.longdouble))
    return v, (g / 2).astype(np.float64)


def candidates(X, ell, n_rand, seed):
    """the last 16 observations exactly, each of them moved by 1e-3 of a length scale, the first observation, random points"""
    rs = np.random.RandomState(seed)
    u = rs.randn(16, X.shape[1]); u /= np.linalg.norm(u, axis=1, keepdims=True)
    return np.vstack([X[-16:], X[-16:] + 1e-3 * np.asarray(ell) * u, X[:1], rs.rand(n_rand, X.shape[1])])


@pytest.fixture(scope="module")
def big():
    """the data set every SE-ARD model here is a prefix of, and the NumPy Cholesky factor of its R"""
    rs = np.random.RandomState(2024)
    X = rs.rand(NBIG, D)
    Y = np.sin(3 * X.sum(1)) + 0.01 * rs.randn(NBIG)
    R = r_matrix("ard", ELL, X)
    L = np.linalg.cholesky(R)
    del R
    gc.collect()
    return X, Y, L


def prefix_ref(big, N):
    X, Y, L = big
    return Ref("ard", ELL, X[:N], Y[:N], L[:N, :N])


def gp(kind, hyper, X, Y):
    from ibo_amd.gaussianprocess import GaussianProcess
    from ibo_amd.gaussianprocess import kernel as K
    k = {"ard": lambda: K.GaussianKernel_ard(np.array(hyper, float)), "m3": lambda: K.MaternKernel3(np.array(hyper, float)),
         "m5": lambda: K.MaternKernel5(np.array(hyper, float))}[kind]()
    return GaussianProcess(k, X, Y, noise=NOISE)


def last_kernel(GP):
    from ibo_amd import _lib
    ms = ctypes.c_float(); name = ctypes.c_char_p()
    _lib.check(_lib.lib.ibo_last_sweep_kernel_ms(GP._handle(), ctypes.byref(ms), ctypes.byref(name)))
    return name.value.decode()


def get_W(GP):
    from ibo_amd import _lib
    N = len(GP.X)
    W = np.empty((N, N)); _lib.check(_lib.lib.ibo_gp_get_W(GP._handle(), _lib.dp(W)))
    return W


def check_sweep(GP, ref, cand, kernel, idx=None):
    """sweep() on cand reports `kernel`; mu, sigma^2, EI against the reference on idx (all when None)"""
    from ibo_amd.acquisition import sweep
    r = sweep(GP, cand, acq='ei', xi=XI, native=True, outputs=("mu", "s2", "acq"))
    assert r["kernel"] == kernel, (r["kernel"], kernel, len(GP.X), len(cand))
    idx = np.arange(len(cand)) if idx is None else np.asarray(idx)
    mu, s2, acq = ref.sweep(cand[idx])
    close(r["mu"][idx], mu, atol=1e-9); close(r["s2"][idx], s2); close(r["acq"][idx], acq, atol=ACQ_ATOL)
    assert r["best_idx"] == int(np.argmax(r["acq"]))
    return r


def check_posterior_x(GP, ref, pts, kernel):
    """posterior(x), one point per call, against the reference (the Python path's clamp)"""
    mu, s2 = ref.post(pts, clamp_lo=1e-7)
    for q, m, v in zip(pts, mu, s2):
        m1, v1 = GP.posterior(q)
        assert last_kernel(GP) == kernel, (last_kernel(GP), kernel, len(GP.X))
        close(m1, m, atol=1e-9); close(v1, v)


def check_fit(GP, ref, nprobe=200):
    """L against NumPy's Cholesky, W L = I on probe rows"""
    N = len(GP.X)
    L = np.array(GP.L)
    assert np.abs(L - ref.L).max() < 1e-11 and np.abs(np.triu(L, 1)).max() == 0.0, N
    W = get_W(GP)
    probe = np.r_[np.random.RandomState(N).randint(0, N, nprobe - 16), np.arange(N - 16, N)]
    assert np.abs(W[probe].dot(L) - np.eye(N)[probe]).max() < 1e-10 and np.all(np.triu(W, 1) == 0.0), N
    del L, W
    gc.collect()


# ---------------------------------------------------------------------------------------------------- the tests
def test_reference_helper_agrees_with_the_oracle(oracle):
    """the NumPy restatement against the oracle itself at 1000 rows: posteriors, EI, NLML and its gradient to 1e-12"""
    X, Y = synth(1000, 1000, D)
    for kind, hyper in (("ard", ELL), ("m5", [.8, 1.0]), ("m3", [.8, 1.0])):
        L = np.linalg.cholesky(r_matrix(kind, hyper, X))
        ref = Ref(kind, hyper, X, Y, L)
        ogp = oracle.GP(oracle.Kern(kind, hyper), X, Y, noise=NOISE)
        cand = candidates(X, hyper if kind == "ard" else [hyper[0]] * D, 40, 3)
        mu, s2 = ref.post(cand, clamp_lo=1e-7)
        omu, os2 = ogp.posteriors(cand)
        close(mu, omu, rtol=1e-12, atol=1e-13); close(s2, os2, rtol=1e-12)
        m2, v2, a2 = ref.sweep(cand)
        o = oracle.sweep_native(ogp, cand, oracle.ACQ_EI, XI)
        close(m2, o["mu"], rtol=1e-10, atol=1e-11); close(v2, o["s2"], rtol=1e-10); close(a2, o["acq"], rtol=1e-10, atol=1e-14)
        if kind in ("ard", "m3"):
            v, g = ref_nlml(kind, hyper, X, Y, L, rows=384)          # (several blocks of rows, as at the large sizes)
            ov, og = oracle.marginal_likelihood(oracle.Kern(kind, hyper), X, Y, D if kind == "ard" else 2, True, NOISE)
            close(v, ov, rtol=1e-12); close(g, og, rtol=1e-12, atol=1e-12 * np.abs(og).max())


def test_gemv_kernel_at_the_64k_lds_boundary(ibo, big):
    """the GEMV kernel holds 8 Npad bytes of LDS: 64 KiB at 8192 rows, dynamic LDS from 8193 (Npad 8256) -- forced by sweep_path=1, and by
    the difference form (dot_form=0) for at most 16 candidates; 40 candidates in the difference form take the panel-split kernel.  SE-ARD at
    both sizes, Matern-5/2 at 8193."""
    X, Y, _ = big
    cases = [("ard", ELL, 8192), ("ard", ELL, 8193), ("m5", [.8, 1.0], 8193)]
    try:
        for kind, hyper, N in cases:
            if kind == "ard":
                ref = prefix_ref(big, N)
            else:
                ref = Ref(kind, hyper, X[:N], Y[:N], np.linalg.cholesky(r_matrix(kind, hyper, X[:N])))
            GP = gp(kind, hyper, X[:N], Y[:N])
            cand = candidates(X[:N], hyper if kind == "ard" else [hyper[0]] * D, 7, N)
            for path, form in ((1, -1), (0, 0)):
                opt(b"sweep_path", path); opt(b"dot_form", form)
                check_sweep(GP, ref, cand[:16], "sweep_gemv_kernel")
                check_sweep(GP, ref, cand[16:32], "sweep_gemv_kernel")
                check_sweep(GP, ref, cand, "sweep_gemv_kernel" if path == 1 else "sweep_mfma_kernel<split>")
                opt(b"sweep_path", 0); opt(b"dot_form", -1)
            del GP, ref
    finally:
        opt(b"sweep_path", 0); opt(b"dot_form", -1)


def test_nlml_gradient_on_the_two_level_branch(ibo, big):
    """from 104 block columns (6656 rows) ibo_nlml_grad factors in the two-level order and forms K^-1 from launch_trinv / launch_pack_w /
    launch_wtw: value to 1e-9 relative, gradient to 1e-8 of its largest component, a repeat gives the same bits"""
    from ibo_amd.gaussianprocess import kernel as K
    from ibo_amd.gaussianprocess.trainhyper import marginalLikelihood
    X, Y, Lbig = big
    for kind, hyper, N in (("ard", ELL, 6700), ("m3", [.8, 1.0], 8193)):
        if kind == "ard":
            k, nh, L = K.GaussianKernel_ard(ELL), D, Lbig[:N, :N]
        else:
            k, nh, L = K.MaternKernel3(np.array(hyper)), 2, np.linalg.cholesky(r_matrix(kind, hyper, X[:N]))
        v, g = marginalLikelihood(k, X[:N], Y[:N], nh, True, noise=NOISE)
        ov, og = ref_nlml(kind, hyper, X[:N], Y[:N], L)
        assert abs(v - ov) <= 1e-9 * abs(ov) and np.abs(np.asarray(g) - og).max() <= 1e-8 * np.abs(og).max(), (N, v, ov, g, og)
        v2, g2 = marginalLikelihood(k, X[:N], Y[:N], nh, True, noise=NOISE)
        assert v2 == v and np.array_equal(np.asarray(g2), np.asarray(g))


@pytest.mark.parametrize("N", [16320, 16383, 16384])
def test_fit_and_sweeps_at_the_2gib_descriptor_boundary(ibo, big, N):
    """16320 rows: the last size whose packed matrices lie inside 2^31 - 1 bytes (the large-batch kernel sweep2_kernel, the small-batch
    wk_small_kernel); 16383: the last row padding; 16384: the packed W is exactly 2^31 bytes (the large-batch kernel got the variances wrong
    there: from 16321 rows on, batches go to the first-generation tile kernel, the panel-split kernel and the GEMV kernel).  The fit (L, W),
    a large batch (2^16 + 37 candidates), a small batch (300), posterior(x); arg-max exact against the reference's."""
    from ibo_amd.acquisition import sweep
    X, Y, _ = big
    ref = prefix_ref(big, N)
    GP = gp("ard", ELL, X[:N], Y[:N])
    check_fit(GP, ref)
    s2k = N <= 16320
    cand = candidates(X[:N], ELL, 300 - 33, N)
    r = check_sweep(GP, ref, cand, "wk_small_kernel" if s2k else "sweep_mfma_kernel<split>")                     # every candidate against the reference
    mu, s2, acq = ref.sweep(cand)
    assert r["best_idx"] == int(np.argmax(acq))
    assert np.all(s2[:16] < 0.2)                                          # (the observations themselves: sigma^2 near the noise)
    rs = np.random.RandomState(N + 1)
    big_cand = np.vstack([cand, rs.rand(2 ** 16 + 37 - len(cand), D)])
    rb = sweep(GP, big_cand, acq='ei', xi=XI, native=True, outputs=("mu", "s2", "acq"))
    assert rb["kernel"] == ("sweep2_kernel" if s2k else "sweep_mfma_kernel")
    # the reference on the boundary candidates, a sample, and the 32 best by the kernel's values (the reference's arg-max is among them
    # unless the kernel's error exceeds the gap to the 33rd)
    top = np.argsort(rb["acq"])[-32:]
    idx = np.unique(np.r_[np.arange(33), rs.randint(0, len(big_cand), 64), top])
    mu, s2, acq = ref.sweep(big_cand[idx])
    close(rb["mu"][idx], mu, atol=1e-9); close(rb["s2"][idx], s2); close(rb["acq"][idx], acq, atol=ACQ_ATOL)
    assert rb["best_idx"] == int(idx[np.argmax(acq)]) == int(np.argmax(rb["acq"]))
    check_posterior_x(GP, ref, cand[:33], "wk_small_kernel" if s2k else "sweep_gemv_kernel")


def test_add_data_across_the_padding_boundary_to_16384_rows(ibo, big):
    """16320 rows, one more (a refit: the padding is full), then block extensions to 16384 that write the tail of the packed W: the sweeps
    against a refit (test_add_data_block_extension_equals_refit's tolerances) and against the reference after every step"""
    X, Y, _ = big
    GP = gp("ard", ELL, X[:16320], Y[:16320])
    n = 16320
    for a in (1, 16, 16, 15, 16):
        GP.addData(X[n:n + a] if a > 1 else X[n], Y[n:n + a] if a > 1 else Y[n])
        n += a
        ref_gp = gp("ard", ELL, X[:n], Y[:n])
        ref = prefix_ref(big, n)
        cand = np.vstack([candidates(X[:n], ELL, 8300 - 33, n)])
        from ibo_amd.acquisition import sweep
        ra = sweep(GP, cand, outputs=("mu", "s2", "acq")); rb = sweep(ref_gp, cand, outputs=("mu", "s2", "acq"))
        assert ra["kernel"] == rb["kernel"] == "sweep_mfma_kernel"
        close(ra["mu"], rb["mu"], rtol=1e-10, atol=1e-11); close(ra["s2"], rb["s2"], rtol=1e-10); assert ra["best_idx"] == rb["best_idx"]
        idx = np.r_[np.arange(33), np.arange(33, 8300, 400)]
        mu, s2, acq = ref.sweep(cand[idx])
        close(ra["mu"][idx], mu, atol=1e-9); close(ra["s2"][idx], s2); close(ra["acq"][idx], acq, atol=ACQ_ATOL)
        probe = cand[:40]
        close(GP.posteriors(probe), ref_gp.posteriors(probe), rtol=1e-11, atol=1e-12)
        del ref_gp, ref
        gc.collect()
    assert n == 16384


def test_direct_at_16384_rows_on_the_small_batch_kernels(ibo, big):
    """DIRECT's batches by the default routing (the GEMV kernel and the panel-split kernel: the model is beyond small2.hip's kernels) and all on
    the panel-split kernel take the same samples and find the same point"""
    from ibo_amd.acquisition import gpuDirectGP
    X, Y, _ = big
    GP = gp("ard", ELL, X[:16384], Y[:16384])
    runs = []
    try:
        for path in (0, 3):
            opt(b"sweep_path", path)
            runs.append(gpuDirectGP(GP, [[0., 1.]] * D, 10, 300, 10000, acqfunc='ei', xi=XI, return_samples=True))
    finally:
        opt(b"sweep_path", 0)
    (v0, x0, n0), (v3, x3, n3) = runs
    assert n3 == n0 and np.array_equal(x3, x0)
    close(v3, v0, rtol=1e-9)


def test_beyond_the_large_batch_kernel_16385_rows(ibo, big):
    """16385 rows (Npad 16448): large batches on the first-generation tile kernel in difference form, at most 16 candidates on the GEMV kernel
    with dynamic LDS, the panel-split kernel in between"""
    X, Y, _ = big
    N = 16385
    ref = prefix_ref(big, N)
    GP = gp("ard", ELL, X[:N], Y[:N])
    cand = candidates(X[:N], ELL, 300 - 33, N)
    check_sweep(GP, ref, cand[:16], "sweep_gemv_kernel")
    check_sweep(GP, ref, cand[16:32], "sweep_gemv_kernel")
    check_sweep(GP, ref, cand, "sweep_mfma_kernel<split>")
    big_cand = np.vstack([cand, np.random.RandomState(5).rand(2 ** 16 + 37 - len(cand), D)])
    from ibo_amd.acquisition import sweep
    rb = sweep(GP, big_cand, acq='ei', xi=XI, native=True, outputs=("mu", "s2", "acq"))
    assert rb["kernel"] == "sweep_mfma_kernel"
    top = np.argsort(rb["acq"])[-32:]
    idx = np.unique(np.r_[np.arange(33), np.arange(33, len(big_cand), 1024), top])
    mu, s2, acq = ref.sweep(big_cand[idx])
    close(rb["mu"][idx], mu, atol=1e-9); close(rb["s2"][idx], s2); close(rb["acq"][idx], acq, atol=ACQ_ATOL)
    assert rb["best_idx"] == int(idx[np.argmax(acq)])
    check_posterior_x(GP, ref, cand[:33:4], "sweep_gemv_kernel")


def test_gemv_kernel_lds_capacity_20416_and_20480_rows(ibo, big):
    """20416 rows: the GEMV kernel's 160 KiB of LDS hold k* of the model (8 Npad bytes) and its own 96 bytes -- posterior(x) against the
    reference.  20480 rows do not fit (a launch that asked for the whole 160 KiB failed): a few points go to the panel-split kernel instead
    and are right; forcing the GEMV kernel is refused with a library error that names the
    limit, before any launch, and the same process then fits and sweeps a small model correctly"""
    from ibo_amd import _lib
    from ibo_amd.acquisition import sweep
    X, Y, _ = big
    for N, kernel in ((20416, "sweep_gemv_kernel"), (20480, "sweep_mfma_kernel<split>")):
        ref = prefix_ref(big, N)
        GP = gp("ard", ELL, X[:N], Y[:N])
        cand = candidates(X[:N], ELL, 3, N)
        check_posterior_x(GP, ref, cand[::3], kernel)
        check_sweep(GP, ref, cand[:16], kernel)
        if N == 20480:
            opt(b"sweep_path", 1)
            try:
                with pytest.raises(_lib.IBOError, match="LDS"):
                    sweep(GP, cand[:16], acq='ei', xi=XI)
            finally:
                opt(b"sweep_path", 0)
        del GP, ref
        gc.collect()
    Xs, Ys = synth(7, 300, 3)
    from oracle import oracle as orc
    GPs = gp("ard", [.3, .4, .5], Xs, Ys)
    c = np.random.RandomState(8).rand(500, 3)
    r = sweep(GPs, c, acq='ei', xi=XI, outputs=("mu", "s2", "acq"))
    o = orc.sweep_native(orc.GP(orc.Kern("ard", [.3, .4, .5]), Xs, Ys, noise=NOISE), c, orc.ACQ_EI, XI)
    close(r["mu"], o["mu"], atol=1e-9); close(r["s2"], o["s2"]); close(r["acq"], o["acq"], atol=ACQ_ATOL)
    assert r["best_idx"] == o["best_idx"]


def test_super_panel_order_moved_past_2gib(ibo, big):
    """fused2_min_nb=200 keeps 11600 rows (Npad 11648) in the single-level order, whose super-panels would store a 2 Npad^2 x 8-byte tall
    matrix (more than 2^31 - 1 bytes): L and W against NumPy"""
    X, Y, _ = big
    N = 11600
    opt(b"fused2_min_nb", 200)
    try:
        GP = gp("ard", ELL, X[:N], Y[:N])
        check_fit(GP, prefix_ref(big, N))
    finally:
        opt(b"fused2_min_nb", 104)


def test_nlml_packed_product_moved_past_2gib(ibo, big):
    """fused2_min_nb=300 keeps 16384 rows in the single-level order in ibo_nlml_grad, whose packed operand for K^-1 = W^T W is Npad^2 x 8 =
    2^31 bytes: value and gradient against the reference"""
    from ibo_amd.gaussianprocess import kernel as K
    from ibo_amd.gaussianprocess.trainhyper import marginalLikelihood
    X, Y, Lbig = big
    N = 16384
    opt(b"fused2_min_nb", 300)
    try:
        v, g = marginalLikelihood(K.GaussianKernel_ard(ELL), X[:N], Y[:N], D, True, noise=NOISE)
    finally:
        opt(b"fused2_min_nb", 104)
    ov, og = ref_nlml("ard", ELL, X[:N], Y[:N], Lbig[:N, :N])
    assert abs(v - ov) <= 1e-9 * abs(ov) and np.abs(np.asarray(g) - og).max() <= 1e-8 * np.abs(og).max(), (v, ov, g, og)

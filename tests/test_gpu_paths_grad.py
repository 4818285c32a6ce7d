"""
ibo_paths_grad_batch (gradients of the pathwise posterior draws with respect to x) and what is built on it: PosteriorPaths.gradient,
.negf_grad, .maximize(polish=True), .maxima and gallery.thompsonSweepGallery(polish=True).

The yardstick is tests/paths_grad_reference.py (NumPy float64, the sine's argument in long double), pinned by
tests/test_paths_grad_reference.py.  With T_grad = |d_d m| (1 + |s1|) + sum_j |d_d phi_j w_j| + sum_i |d_d k_i| (|c_i| + |m a1_i|)
per (path, point, dimension):
    composition   device gradients against the restatement evaluated on the device's OWN coefficients (ibo_paths_coef): 1e-11 T_grad,
                  the bar of the values' composition -- the same arithmetic; the restatement itself stays within 1e-12 T_grad of
                  long double (test_paths_grad_reference.py)
    end to end    device gradients against the restatement's own coefficients: 1e-6 T_grad, the project's end-to-end bar
    differences   central differences of ibo_paths_batch, step 1e-5: 1e-5 |G| + 1e-6 max |grad|, the bar of test_gpu_gradients.py
Everything else is exact: one route (bit-equal gradients alone, at any place of a batch, in any chunk, with and without path_of),
values bit-equal to ibo_paths_batch, NaN staying with its point, snapshots.
"""
import ctypes
import functools

import numpy as np
import pytest

import paths_grad_reference as pg
import paths_reference as pr
import test_gpu_paths as tp
import test_gpu_posterior_cov as pc

pytestmark = pytest.mark.gpu

GUARD = tp.GUARD
DC = 4            # the kernel's dimension chunk (PG_DC of ibo_amd/csrc/paths.h)

CASES = [  # kind, D, N, F, S, M, prior, shift
    ("ard", 1, 1, 1, 1, 1, False, 0.0),
    ("iso", 3, 63, 31, 3, 63, False, 0.0),
    ("svard", 3, 64, 32, 64, 64, False, 0.0),
    ("sviso", 8, 65, 33, 65, 65, False, 0.0),
    ("m3", 3, 130, 100, 100, 255, False, 0.0),
    ("m5", 3, 130, 100, 65, 257, True, 0.0),             # a trained mean prior: 63 paths per column tile
    ("svard", 8, 63, 33, 64, 1, True, 0.0),
    ("ard", 3, 130, 256, 64, 100, False, 1000.0),        # data a thousand units from the origin
    ("m5", 8, 1030, 1024, 3, 64, False, 0.0),            # one long K loop
    ("sviso", DC - 1, 40, 40, 5, 70, True, 0.0),         # one dimension below, at and above the kernel's chunk
    ("ard", DC, 40, 40, 5, 70, False, 0.0),
    ("m3", DC + 1, 40, 40, 5, 70, True, 0.0),
    ("ard", 33, 65, 33, 2, 65, False, 0.0),
    ("m3", 64, 65, 33, 2, 65, True, 0.0),
]


@pytest.fixture(scope="module")
def lib():
    from ibo_amd import _lib
    if _lib.device_count() < 1:
        pytest.fail("no GPU visible: the product has no CPU fallback")
    return _lib


def grad_rc(lib, P, Q, path_of=None, values=True):
    """the raw entry with guard words behind both outputs -> (status, values, grads)"""
    Q = lib.f64(np.atleast_2d(Q))
    M = len(Q)
    nv = M if path_of is not None else P.S * M
    v = np.full(nv + 8, GUARD); g = np.full(nv * P.D + 8, GUARD)
    po = None if path_of is None else np.ascontiguousarray(path_of, dtype=np.intc)
    rc = lib.lib.ibo_paths_grad_batch(P.h, M, lib.dp(Q), None if po is None else po.ctypes.data_as(ctypes.POINTER(ctypes.c_int)),
                                      lib.dp(v) if values else None, lib.dp(g))
    assert np.all(g[-8:] == GUARD), "guard behind the gradients overwritten"
    assert np.all(v[-8:] == GUARD), "guard behind the values overwritten"
    if not values:
        assert np.all(v == GUARD)
    shape = (M,) if path_of is not None else (P.S, M)
    return rc, v[:-8].reshape(shape), g[:-8].reshape(shape + (P.D,))


def grad_call(lib, P, Q, path_of=None, values=True):
    rc, v, g = grad_rc(lib, P, Q, path_of, values)
    lib.check(rc)
    return v, g


@functools.lru_cache(maxsize=None)
def case_data(case):
    """one case: the device's coefficients, values and gradients and the restatement's, computed once for the tests that read them"""
    from ibo_amd import _lib
    kind, D, N, F, S, M, prior, shift = case
    GP, ref = tp.model(kind, D, N, prior, shift)
    arrs = tp.draws(GP, ref, F, S)
    P = tp.Paths(_lib, GP, *arrs)
    Q = pc.queries(ref.X - shift, M) + shift
    v, g = grad_call(_lib, P, Q)
    got = dict(coef=P.coef(), values=v, grads=g, batch=P.batch(Q))
    P.close()
    omega, phase, w, eps = arrs
    c_ref = pr.coef(ref, omega, phase, w, eps)
    want = dict(grads=pg.grads(ref, omega, phase, c_ref, Q), T=pg.grad_scale(ref, omega, phase, c_ref, Q),
                own=pg.grads(ref, omega, phase, got["coef"], Q), T_own=pg.grad_scale(ref, omega, phase, got["coef"], Q))
    return got, want


def close(got, want, tol, what):
    err = np.abs(np.asarray(got) - want)
    print("%s: worst error / bar = %.3g" % (what, float(np.max(err / tol))))
    assert np.all(err <= tol), "%s: worst %g of its bar" % (what, float(np.max(err / tol)))


@pytest.mark.parametrize("case", CASES)
def test_gradients_against_the_composition_of_their_own_coefficients(lib, case):
    got, want = case_data(case)
    assert got["grads"].shape == (case[4], case[5], case[1]) and np.all(np.isfinite(got["grads"]))
    assert np.array_equal(got["values"], got["batch"])                          # the values are ibo_paths_batch's bits
    close(got["grads"], want["own"], 1e-11 * want["T_own"], "composition %s" % (case,))


@pytest.mark.parametrize("case", CASES)
def test_gradients_end_to_end(lib, case):
    got, want = case_data(case)
    close(got["grads"], want["grads"], 1e-6 * want["T"], "end to end %s" % (case,))


@pytest.mark.parametrize("kind", ["ard", "m5"])
def test_gradients_against_differences_of_the_librarys_own_values(lib, kind):
    GP, ref = tp.model(kind, 3, 50, prior=True)
    P = tp.Paths(lib, GP, *tp.draws(GP, ref, 100, 5))
    Q = np.random.RandomState(3).rand(40, 3)
    _, got = grad_call(lib, P, Q)
    step = 1e-5
    G = np.zeros(got.shape)
    for d in range(3):
        E = np.zeros(Q.shape); E[:, d] = step
        G[:, :, d] = (P.batch(Q + E) - P.batch(Q - E)) / (2 * step)
    P.close()
    bar = 1e-5 * np.abs(G) + 1e-6 * np.max(np.linalg.norm(got, axis=2))
    close(got, G, bar, "central differences %s" % kind)


@pytest.mark.parametrize("prior", [False, True])
def test_one_route_gives_one_set_of_bits(lib, prior):
    GP, ref = tp.model("m5", 3, 70, prior)
    S = 66
    P = tp.Paths(lib, GP, *tp.draws(GP, ref, 50, S))
    Q = pc.queries(ref.X, 300, seed=9)
    v, g = grad_call(lib, P, Q)
    assert np.array_equal(v, P.batch(Q))
    _, g_only = grad_call(lib, P, Q, values=False)
    assert np.array_equal(g_only, g)
    q = Q[17]
    _, alone = grad_call(lib, P, q)
    assert np.array_equal(alone[:, 0], g[:, 17])
    B = Q[:130].copy()
    B[0] = q; B[63] = q; B[64] = q
    vb, gb = grad_call(lib, P, B)
    for place in (0, 63, 64):
        assert np.array_equal(gb[:, place], alone[:, 0]), "place %d of a batch of 130" % place
    assert np.array_equal(gb[:, 1:63], g[:, 1:63]) and np.array_equal(gb[:, 65:130], g[:, 65:130]) and np.array_equal(vb, P.batch(B))
    po = (np.arange(300) * 7) % S
    try:
        lib.check(lib.lib.ibo_set_option(b"paths_chunk", 256))
        v2, g2 = grad_call(lib, P, Q)
        vp2, gp2 = grad_call(lib, P, Q, path_of=po)
    finally:
        lib.check(lib.lib.ibo_set_option(b"paths_chunk", 0))
    assert np.array_equal(g2, g) and np.array_equal(v2, v), "paths_chunk = 256 against the default"
    vp, gp = grad_call(lib, P, Q, path_of=po)
    assert np.array_equal(gp, g[po, np.arange(300)]) and np.array_equal(vp, v[po, np.arange(300)]), "path_of against the full output"
    assert np.array_equal(gp2, gp) and np.array_equal(vp2, vp)
    P.close()


@pytest.mark.parametrize("kind", ["m3", "m5"])
def test_a_query_on_a_model_row_and_a_nan_coordinate(lib, kind):
    GP, ref = tp.model(kind, 3, 40, prior=(kind == "m5"))
    arrs = tp.draws(GP, ref, 64, 5)
    P = tp.Paths(lib, GP, *arrs)
    Q = np.r_[ref.X[:6], pc.queries(ref.X, 64, seed=4)]
    v, g = grad_call(lib, P, Q)
    assert np.all(np.isfinite(g)) and np.all(np.isfinite(v))
    own = P.coef()
    close(g, pg.grads(ref, arrs[0], arrs[1], own, Q), 1e-11 * pg.grad_scale(ref, arrs[0], arrs[1], own, Q), "on model rows %s" % kind)
    B = Q.copy(); B[3, 1] = np.nan; B[64] = np.nan
    vn, gn = grad_call(lib, P, B)
    assert np.all(np.isnan(gn[:, [3, 64]])) and np.all(np.isnan(vn[:, [3, 64]]))
    rest = np.delete(np.arange(len(Q)), [3, 64])
    assert np.array_equal(gn[:, rest], g[:, rest]) and np.array_equal(vn[:, rest], v[:, rest])
    P.close()


def test_errors_closed_objects_and_snapshots(lib):
    from ibo_amd.acquisition import PosteriorPaths
    GP, ref = tp.model("m3", 3, 30, prior=True)
    P = tp.Paths(lib, GP, *tp.draws(GP, ref, 40, 5))
    Q = pc.queries(ref.X, 6, seed=3)
    for bad in ([0, 1, 5, 0, 0, 0], [0, -1, 0, 0, 0, 0]):
        rc, v, g = grad_rc(lib, P, Q, path_of=bad)
        assert rc == lib.ERR_ARG and np.all(g == GUARD) and np.all(v == GUARD)
    L, dp = lib.lib, lib.dp
    out = np.empty(200); q = lib.f64(Q)
    assert L.ibo_paths_grad_batch(P.h, 0, dp(q), None, dp(out), dp(out)) == lib.ERR_ARG
    assert L.ibo_paths_grad_batch(P.h, 6, None, None, dp(out), dp(out)) == lib.ERR_ARG
    assert L.ibo_paths_grad_batch(P.h, 6, dp(q), None, dp(out), None) == lib.ERR_ARG
    assert L.ibo_paths_grad_batch(None, 6, dp(q), None, dp(out), dp(out)) == lib.ERR_ARG
    assert grad_call(lib, P, Q)[1].shape == (5, 6, 3)                           # the object is still usable
    P.close()
    PP = PosteriorPaths(GP, n_paths=5, n_features=96, seed=11)
    v0, g0 = PP.gradient(Q)
    GP.addData(np.full(3, .5), 1.25)
    v1, g1 = PP.gradient(Q)
    assert np.array_equal(v1, v0) and np.array_equal(g1, g0)                    # a snapshot: the model's new row is not in it
    PP.close()
    with pytest.raises(ValueError):
        PP.gradient(Q)
    with pytest.raises(ValueError):
        PP.negf_grad(Q[0])


def test_python_layer_agrees_with_the_raw_entry(lib):
    from ibo_amd.acquisition import PosteriorPaths
    GP, ref = tp.model("svard", 2, 50)
    P = PosteriorPaths(GP, n_paths=4, n_features=200, seed=5)
    raw = tp.Paths(lib, GP, P.omega, P.phase, P.w, P.eps)
    C = np.random.RandomState(8).rand(70, 2)
    v, g = P.gradient(C)
    rv, rg = grad_call(lib, raw, C)
    assert v.shape == (4, 70) and g.shape == (4, 70, 2) and np.array_equal(v, rv) and np.array_equal(g, rg)
    assert np.array_equal(v, P.values(C))
    po = np.arange(70) % 4
    vp, gp = P.gradient(C, paths=po)
    assert vp.shape == (70,) and gp.shape == (70, 2) and np.array_equal(vp, v[po, np.arange(70)]) and np.array_equal(gp, g[po, np.arange(70)])
    v1, g1 = P.gradient(C[0])
    assert v1.shape == (4, 1) and g1.shape == (4, 1, 2) and np.array_equal(g1[:, 0], g[:, 0])
    nf, ng = P.negf_grad(C[5], path=3)
    assert nf == -v[3, 5] and np.array_equal(ng, -g[3, 5])
    assert P.negf_grad(C[5])[0] == -v[0, 5]
    with pytest.raises(ValueError):
        P.gradient(C, paths=[0, 1])
    with pytest.raises(ValueError):
        P.gradient(C[:2], paths=[0, 4])
    with pytest.raises(ValueError):
        P.negf_grad(C[0], path=4)
    bounds = [[0., 1.]] * 2
    for path in (0, 3):
        opt, optx = P.maximize(bounds, path=path, maxiter=10)
        popt, poptx = P.maximize(bounds, path=path, maxiter=10, polish=True)
        print("path %d: DIRECT %.12g, polished %.12g" % (path, opt, popt))
        assert popt >= opt and P.values(poptx)[path, 0] == popt
        assert np.all(poptx >= 0) and np.all(poptx <= 1)
        assert (popt > opt) or np.array_equal(poptx, optx)
    raw.close(); P.close()


def projected_norm(x, g, lo, hi):
    g = np.where(((x <= lo) & (g < 0)) | ((x >= hi) & (g > 0)), 0.0, g)
    return np.linalg.norm(g, axis=1)


def test_maxima_ascends_every_path_in_lock_step(lib):
    from ibo_amd.acquisition import PosteriorPaths
    from ibo_amd.utils.latinhypercube import lhcSample
    GP, ref = tp.model("ard", 2, 30)
    S = 16
    P = PosteriorPaths(GP, n_paths=S, n_features=256, seed=5)
    bounds = [[0., 1.]] * 2
    C = np.array(lhcSample(bounds, 4096, seed=5))
    sw = P.sweep(C)
    start_x = C[sw["best_idx"]]
    vals, X = P.maxima(bounds)                                                  # the default candidates: this seed's latin hypercube
    assert vals.shape == (S,) and X.shape == (S, 2)
    v0, X0 = P.maxima(bounds, polish=False)
    assert np.array_equal(v0, sw["best_val"]) and np.array_equal(X0, start_x)
    own = np.arange(S)
    assert np.all(vals >= sw["best_val"]) and np.any(vals > sw["best_val"])
    assert np.array_equal(vals, P.values(X)[own, own])
    assert np.all(X >= 0) and np.all(X <= 1)
    moved = np.any(X != start_x, axis=1)
    assert np.array_equal(moved, vals > sw["best_val"])
    n0 = projected_norm(start_x, P.gradient(start_x, paths=own)[1], 0.0, 1.0)
    n1 = projected_norm(X, P.gradient(X, paths=own)[1], 0.0, 1.0)
    print("maxima: %d of %d paths moved; projected gradient %.3g -> %.3g (medians); worst gain %.3g" %
          (moved.sum(), S, np.median(n0), np.median(n1), float(np.max(vals - sw["best_val"]))))
    assert np.all(n1[moved] <= n0[moved])
    v2, X2 = P.maxima(bounds, candidates=C)
    assert np.array_equal(v2, vals) and np.array_equal(X2, X)
    nan_c = np.full((5, 2), np.nan)
    vn, Xn = P.maxima(bounds, candidates=nan_c)
    assert np.all(vn == -np.inf) and np.all(np.isnan(Xn))
    P.close()


def test_thompson_sweep_gallery_polish(lib):
    from ibo_amd.acquisition.gallery import thompsonSweepGallery, MIN_SEPARATION
    GP, ref = tp.model("ard", 3, 25)
    C = np.random.RandomState(2).rand(3000, 3)
    g1 = thompsonSweepGallery(GP, C, 4, seed=3, n_features=256)
    g2 = thompsonSweepGallery(GP, C, 4, seed=3, n_features=256, polish=False)
    assert len(g1) == len(g2) == 4 and all(np.array_equal(a, b) for a, b in zip(g1, g2))
    g3 = thompsonSweepGallery(GP, C, 4, seed=3, n_features=256, polish=True, bounds=[[0., 1.]] * 3)
    assert 1 <= len(g3) <= 4
    for i, x in enumerate(g3):
        assert x.shape == (3,) and np.all(x >= 0) and np.all(x <= 1)
        for y in g3[:i]:
            assert np.linalg.norm(x - y) > MIN_SEPARATION
    assert not all(np.any(np.all(C == x, axis=1)) for x in g3)                  # at least one member left its candidate row
    with pytest.raises(ValueError):
        thompsonSweepGallery(GP, C, 4, seed=3, n_features=256, polish=True)

"""
ibo_ggp_* where tests/test_gpu_gradobs.py does not go: k* beyond one block of 256 data points, a gnoise of its own per dimension, D = 64,
sf2 != 1 on the SE family, the three fit routes at their default switches (up to IBO_GGP_MAX_ROWS = 8192 rows) and forced at 2100 rows,
one handle refitted to other shapes, sweeps of more candidates than one by-bytes chunk holds, the timing path, translated inputs.

The yardstick and every bar are tests/test_gpu_gradobs.py's (gradobs_reference.py, EDGE_CASES): R at 1e-12 of its kind of block, L by the
Cholesky backward bound 4 P 2^-53 max A_ii, mu / s2 within gr.bars, and bit equality.  A case of more than 2000 rows is held to float64
under cond_upper <= 1e6 (asserted in tests/test_gradobs_reference.py), where the bars' factor is its floor 1e-9; such a case is fitted
once, by one test, and nothing of it is kept.
"""
import ctypes
import gc

import numpy as np
import pytest

import gradobs_reference as gr
import test_gpu_gradobs as tg
from test_gpu_gradobs import Handle, same_bits, device_case, lib          # noqa: F401  (lib: the fixture)

pytestmark = pytest.mark.gpu
EI = (gr.ACQ_EI, 0.01, gr.ERF_LIBM, gr.CLAMP_NATIVE)
DEFAULTS = {b"super_min_nb": 64, b"fused2_min_nb": 104}


def info_of(lib, h):
    v = [ctypes.c_int(), ctypes.c_int(), ctypes.c_int(), ctypes.c_int(), ctypes.c_double()]
    lib.check(lib.lib.ibo_ggp_info(h.h, *[ctypes.byref(x) for x in v]))
    return tuple(x.value for x in v)


def check_R(name, A, R, N, D):
    """|R - A| by kind of block at 1e-12 of that kind's largest entry of A; views, no copies (A and R may hold 8192 rows)"""
    B = D + 1
    A4, R4 = A.reshape(N, B, N, B), R.reshape(N, B, N, B)
    shares = []
    for kind, a, r in (("value-value", A4[:, 0, :, 0], R4[:, 0, :, 0]), ("value-derivative", A4[:, 0, :, 1:], R4[:, 0, :, 1:]),
                       ("derivative-value", A4[:, 1:, :, 0], R4[:, 1:, :, 0]), ("derivative-derivative", A4[:, 1:, :, 1:], R4[:, 1:, :, 1:])):
        err = max(float(np.max(np.abs(a[i0:i0 + 256] - r[i0:i0 + 256]))) for i0 in range(0, N, 256))
        bar = 1e-12 * float(np.max(np.abs(a)))
        print("%s %s: |R - A| %.3g, bar %.3g" % (name, kind, err, bar))
        assert err <= bar, (kind, err, bar)
        shares.append(err / bar)
    return max(shares)


def l_rows(P):
    """the rows on which L of more than 4096 rows is checked: the first and the last 64-row block, the rows around every multiple of
    1024, and 256 rows from a fixed seed"""
    rows = set(range(64)) | set(range(P - 64, P))
    for k in range(1, P // 1024 + 1):
        rows |= {r for r in (1024 * k - 1, 1024 * k, 1024 * k + 1) if r < P}
    rows |= set(np.random.RandomState(4242).choice(P, 256, replace=False).tolist())
    return np.array(sorted(rows))


def check_L(name, L, R, P):
    """|L L^T - R|_max <= 4 P 2^-53 max A_ii: on the whole product up to 4096 rows, on l_rows beyond"""
    assert all(not np.any(np.triu(L[i0:i0 + 512], i0 + 1)) for i0 in range(0, P, 512))
    bar = 4.0 * P * 2.0 ** -53 * float(np.max(np.diag(R)))
    if P <= 4096:
        back, what = float(np.max(np.abs(L @ L.T - R))), "every row"
    else:
        rows = l_rows(P)
        back, what = float(np.max(np.abs(L[rows] @ L.T - R[rows]))), "%d rows" % len(rows)
    print("%s: |L L^T - A| %.3g on %s, bar %.3g" % (name, back, what, bar))
    assert back <= bar
    return back / bar


def check_posterior(name, h, ref, Q):
    want = gr.posterior(ref, Q, gr.CLAMP_PY)
    bmu, bs2 = gr.bars(ref, want)
    got = h.batch(Q, want=("mu", "s2"))
    rmu = np.abs(got["mu"] - np.asarray(want["mu"], dtype=np.float64)) / bmu
    rs2 = np.abs(got["s2"] - np.asarray(want["s2"], dtype=np.float64)) / bs2
    print("%s M=%d (cond %.3g, %s): mu at %.3g of the bar, s2 at %.3g" % (name, len(Q), ref["cond"], ref["dt"].__name__, rmu.max(), rs2.max()))
    assert np.all(rmu <= 1.0) and np.all(rs2 <= 1.0)
    return got, bmu, bs2


def check_sweep(lib, h, Q, spec=EI, index_base=1000):
    """the sweep's outputs are the batch's bits and its winner is NumPy's first arg-max of them"""
    Q = lib.f64(Q)
    base = h.batch(Q, *spec)
    r = h.sweep(lib.DeviceArray.from_host(Q), len(Q), *spec, index_base=index_base)
    for k in ("mu", "s2", "acq"):
        assert same_bits(r[k], base[k]), k
    k0 = int(np.argmax(base["acq"]))
    assert r["best_idx"] == index_base + k0 and r["best_val"] == base["acq"][k0]
    return r


# ---------------------------------------------------------------------------- small edge cases on the existing checks
@pytest.mark.parametrize("name", gr.SMALL_EDGE_NAMES)
def test_edge_R_is_the_restated_matrix_and_L_its_factor(lib, name):
    tg.test_R_is_the_restated_matrix_and_L_its_factor(lib, name)


@pytest.mark.parametrize("name", gr.SMALL_EDGE_NAMES)
def test_edge_posterior_within_the_conditioning_bars(lib, name):
    tg.test_posterior_within_the_conditioning_bars(lib, name)


@pytest.mark.parametrize("name", gr.SMALL_EDGE_NAMES)
def test_edge_acquisitions_in_both_erf_flavours(lib, name):
    tg.test_acquisitions_in_both_erf_flavours(lib, name)


def test_the_edge_cases_are_where_they_claim_to_be(lib):
    """k* blocks of 256 points: 2 at N = 257 (one point and the pad in the second), 2 at N = 300 with 768 entries per block, 3 at N = 513;
    the frames' pads; the coincident pair in two different blocks; the long-double reference where cond_2 > 1e6"""
    for name, Ppad, blocks in (("ard_257x1", 576, 2), ("m5_300x2", 960, 2), ("m3_513x1", 1088, 3)):
        h, c, ref, _, _ = device_case(name)
        assert -(-h.P // 64) * 64 == Ppad and -(-h.N // 256) == blocks
        assert (ref["dt"] is np.longdouble) == (ref["cond"] > 1e6)
    assert device_case("ard_257x1")[2]["dt"] is np.longdouble and device_case("m5_300x2")[2]["dt"] is np.longdouble
    X = gr.case("m3_513x1")["X"]
    assert np.array_equal(X[2], X[400]) and 2 // 256 != 400 // 256
    R = device_case("m3_513x1")[0].matrix("R")
    kern = gr.case("m3_513x1")["kern"]
    assert R[2 * 2, 400 * 2] == kern.sf2_py and R[2 * 2 + 1, 400 * 2] == 0.0 and R[2 * 2, 400 * 2 + 1] == 0.0      # r = 0 off the diagonal
    # a query ON a point of the third block: r = 0 in k* off block 0 -- the value entry is sf2, the derivative entry 0, the mean finite
    h = device_case("m3_513x1")[0]
    got = h.batch(X[512:513], want=("mu", "s2"))
    assert np.isfinite(got["mu"][0]) and np.isfinite(got["s2"][0])


def test_every_dimension_carries_its_own_gnoise(lib):
    """ard_60x3_gn, gnoise (1e-4, 3e-3, 0.05): diag(R) on derivative row d minus the same entry of the matrix restated with gnoise = 0 is
    gnoise[d - 1], within the R bar of a derivative-derivative entry"""
    h, c, ref, _, _ = device_case("ard_60x3_gn")
    N, D = c["X"].shape
    B = D + 1
    assert len(set(c["gnoise"].tolist())) == D
    A0 = gr.matrix(c["kern"], c["X"], c["noise"], 0.0)
    R = h.matrix("R")
    bar = 1e-12 * float(np.max(np.abs(A0.reshape(N, B, N, B)[:, 1:, :, 1:])))
    add = (np.diag(R) - np.diag(A0)).reshape(N, B)
    for d in range(1, B):
        err = float(np.max(np.abs(add[:, d] - c["gnoise"][d - 1])))
        print("derivative %d: gnoise %.3g, worst miss %.3g, bar %.3g" % (d, c["gnoise"][d - 1], err, bar))
        assert err <= bar
    assert np.all(np.diag(R)[::B] == 1.0 + c["noise"])
    off = R - A0
    off[np.diag_indices(len(off))] = 0.0
    assert float(np.max(np.abs(off))) <= bar                          # and nowhere else


def test_65_dimensions_are_refused_and_the_model_stays(lib):
    c = gr.case("ard_13x4")
    h = Handle(c["kern"], c["X"], c["Y"], c["G"], c["noise"], c["gnoise"])
    Q = gr.queries(c["X"], 65)
    before = (info_of(lib, h), h.matrix("R"), h.matrix("L"), h.batch(Q, *EI))
    from oracle import oracle as orc
    X = gr.points(2, 65, 9)
    Y, G = gr.objective(X)
    for kern in (orc.Kern("iso", [4.0]), orc.Kern("ard", [4.0] * 65)):
        assert h.fit(kern, X, Y, G, 0.1, 1e-4) == lib.ERR_ARG
        after = (info_of(lib, h), h.matrix("R"), h.matrix("L"), h.batch(Q, *EI))
        assert after[0] == before[0] and np.array_equal(after[1], before[1]) and np.array_equal(after[2], before[2])
        for k in ("mu", "s2", "acq"):
            assert same_bits(after[3][k], before[3][k])
    ok = gr.case("se_3x64")                                            # 64 is served
    lib.check(h.fit(ok["kern"], ok["X"], ok["Y"], ok["G"], ok["noise"], ok["gnoise"]))
    assert info_of(lib, h)[:3] == (3, 64, 195)
    h.close()


# ---------------------------------------------------------------------------- the three fit routes
@pytest.mark.parametrize("name,route", [("ard_1008x3", "pipelined, 63 block columns"), ("ard_1009x3", "super-panels, Npad 4096"),
                                        ("m5_1648x3", "super-panels, 103 block columns"), ("m3_1649x3", "two-level, Npad 6656"),
                                        ("iso_2048x3", "two-level, 8192 rows: the limit")])
def test_a_fit_on_its_default_route(lib, name, route):
    """no option set: the route is the one the row count selects.  info, R by kind of block, L by the backward bound (every row up to
    4096, l_rows beyond), mu / s2 at 65 queries within bars(), EI from the sweep bit-equal to the batch with its arg-max at M = 300.
    Worst share of each bar measured on an MI355X (R, L, mu, s2):
        P = 4032  3.7e-4, 1.5e-3, 1.4e-7, 4.8e-7        P = 4036  3.7e-4, 1.6e-3, 1.3e-7, 4.2e-7        P = 6592  8.8e-4, 1.1e-3, 3.2e-7, 4.7e-7
        P = 6596  5.2e-4, 9.4e-4, 2.4e-7, 5.8e-7        P = 8192  4.4e-4, 1.0e-3, 6.9e-8, 5.3e-7
    The 8192-row case takes about 11 s, nearly all of it in the float64 reference on the host."""
    c = gr.case(name)
    N, D = c["X"].shape
    P = N * (D + 1)
    ref = gr.reference_model(name)
    assert ref["dt"] is np.float64 and 1e-15 * max(ref["cond"], 1e6) == 1e-9
    h = Handle(c["kern"], c["X"], c["Y"], c["G"], c["noise"], c["gnoise"])
    try:
        assert h.info.value == 0 and info_of(lib, h) == (N, D, P, lib.default_device(), float(np.max(c["Y"])))
        R = h.matrix("R")
        assert all(np.array_equal(R[i0:i0 + 512], R[:, i0:i0 + 512].T) for i0 in range(0, P, 512))
        sR = check_R(name, ref["A"], R, N, D)
        L = h.matrix("L")
        sL = check_L(name, L, R, P)
        del R, L
        Q = gr.queries(c["X"], 65)
        got, bmu, bs2 = check_posterior(name, h, ref, Q)
        want = gr.posterior(ref, Q, gr.CLAMP_PY)
        smu = float(np.max(np.abs(got["mu"] - want["mu"]) / bmu)); ss2 = float(np.max(np.abs(got["s2"] - want["s2"]) / bs2))
        print("%s (%s) P %d: worst share of the bars: R %.3g, L %.3g, mu %.3g, s2 %.3g" % (name, route, P, sR, sL, smu, ss2))
        check_sweep(lib, h, np.random.RandomState(17).rand(300, D))
    finally:
        h.close()
        del ref, c
        gc.collect()


def test_three_routes_at_2100_rows_agree(lib):
    """ard_525x3 (33 block columns) by default (pipelined), in super-panels (super_min_nb = 32) and in the two-level order
    (fused2_min_nb = 33): every fit within the bars of one reference, the three posteriors within twice the bar of each other"""
    name = "ard_525x3"
    c = gr.case(name)
    N, D = c["X"].shape
    ref = gr.reference_model(name)
    Q = gr.queries(c["X"], 65)
    posts = {}
    try:
        for route, opts in (("default", {}), ("super", {b"super_min_nb": 32}), ("two_level", {b"fused2_min_nb": 33})):
            for k, v in opts.items():
                lib.check(lib.lib.ibo_set_option(k, v))
            h = Handle(c["kern"], c["X"], c["Y"], c["G"], c["noise"], c["gnoise"])
            for k in opts:
                lib.check(lib.lib.ibo_set_option(k, DEFAULTS[k]))
            assert h.info.value == 0
            R = h.matrix("R")
            check_R(name + " " + route, ref["A"], R, N, D)
            check_L(name + " " + route, h.matrix("L"), R, h.P)
            posts[route], bmu, bs2 = check_posterior(name + " " + route, h, ref, Q)
            check_sweep(lib, h, np.random.RandomState(17).rand(300, D))
            h.close()
    finally:
        for k, v in DEFAULTS.items():
            lib.check(lib.lib.ibo_set_option(k, v))
    for a, b in (("default", "super"), ("default", "two_level"), ("super", "two_level")):
        dmu = float(np.max(np.abs(posts[a]["mu"] - posts[b]["mu"]) / bmu)); ds2 = float(np.max(np.abs(posts[a]["s2"] - posts[b]["s2"]) / bs2))
        print("%s against %s: mu at %.3g of the bar, s2 at %.3g (allowed: 2)" % (a, b, dmu, ds2))
        assert dmu <= 2.0 and ds2 <= 2.0
    # the options did move the fit: super-panels are documented to give the bits of the step-by-step order (other buffers, the same sums),
    # the two-level order forms W by recursive doubling -- another order of the same sums
    assert same_bits(posts["super"]["mu"], posts["default"]["mu"]) and same_bits(posts["super"]["s2"], posts["default"]["s2"])
    assert not (same_bits(posts["two_level"]["mu"], posts["default"]["mu"]) and same_bits(posts["two_level"]["s2"], posts["default"]["s2"]))


# ---------------------------------------------------------------------------- one handle, many shapes
def snapshot(lib, h, c):
    Q = gr.queries(c["X"], 130)
    sw = check_sweep(lib, h, np.random.RandomState(29).rand(300, c["X"].shape[1]), index_base=5)
    return dict(info=info_of(lib, h), R=h.matrix("R"), L=h.matrix("L"), batch=h.batch(Q, *EI), sweep=sw)


def test_one_handle_refitted_to_other_shapes_equals_fresh_handles(lib):
    """shrinking and growing N, other D, other families, a frame with a second k* block after smaller ones, a failed fit in between: after
    every successful fit everything read from the handle is a fresh handle's, bit for bit"""
    from oracle import oracle as orc
    first = gr.case("ard_205x4")
    h = Handle(first["kern"], first["X"], first["Y"], first["G"], first["noise"], first["gnoise"], fit=False)
    bad = gr.case("ard_13x4")
    Xd = np.array(bad["X"][:6]); Xd[1] = Xd[0]
    Yd, Gd = gr.objective(Xd)
    try:
        for name in ("ard_205x4", "se_1x1", "m5_9x16", "ard_257x1", "ard_13x4", None, "m3_21x2"):
            if name is None:
                rc = h.fit(orc.Kern("ard", [0.6, 0.8, 0.7, 0.9]), Xd, Yd, Gd, 0.0, 0.0)
                assert rc == lib.ERR_NOT_PD and h.info.value == 6
                q = lib.f64(Xd[:2]); out = np.zeros(2); bv = ctypes.c_double(); lb = lib.f64(np.zeros(4)); ub = lib.f64(np.ones(4))
                big = np.zeros(1025 * 1025)
                assert lib.lib.ibo_ggp_acq_batch(h.h, 2, lib.dp(q), 0, 0.01, 0, 1e-8, float("nan"), None, None, lib.dp(out)) == lib.ERR_STATE
                assert lib.lib.ibo_ggp_get_R(h.h, lib.dp(big)) == lib.ERR_STATE and lib.lib.ibo_ggp_get_L(h.h, lib.dp(big)) == lib.ERR_STATE
                assert lib.lib.ibo_ggp_direct_max(h.h, 4, lib.dp(lb), lib.dp(ub), 0, 0.01, 0, 1e-8, 5, 30, 1000, 1, ctypes.byref(bv), None,
                                                  None) == lib.ERR_STATE
                cand = lib.DeviceArray.from_host(q)
                assert lib.lib.ibo_ggp_acq_sweep(h.h, 2, cand.ptr, 0, 0.01, 0, 1e-8, float("nan"), 0, None, None, None, ctypes.byref(bv),
                                                 None) == lib.ERR_STATE
                assert not np.any(big) and not np.any(out)
                continue
            c = gr.case(name)
            lib.check(h.fit(c["kern"], c["X"], c["Y"], c["G"], c["noise"], c["gnoise"]))
            h.N, h.D = c["X"].shape
            h.P = h.N * (h.D + 1)
            assert h.info.value == 0
            got, want = snapshot(lib, h, c), snapshot(lib, device_case(name)[0], c)
            assert got["info"] == want["info"], name
            assert np.array_equal(got["R"], want["R"]) and np.array_equal(got["L"], want["L"]), name
            for k in ("mu", "s2", "acq"):
                assert same_bits(got["batch"][k], want["batch"][k]), (name, k)
                assert same_bits(got["sweep"][k], want["sweep"][k]), (name, k)
            assert got["sweep"]["best_idx"] == want["sweep"]["best_idx"] and got["sweep"]["best_val"] == want["sweep"]["best_val"]
    finally:
        h.close()


def test_addData_one_point_at_a_time_across_the_tile_equals_fresh_models(lib):
    """D = 4: 12 points are 60 rows, 13 are 65, 14 are 70 -- the frame grows from one 64-row tile to two"""
    GP, c = tg.python_model("ard_60x4", upto=12)
    Q = gr.queries(c["X"], 65)
    for n in (13, 14):
        GP.addData(c["X"][n - 1], c["Y"][n - 1], c["G"][n - 1])
        fresh, _ = tg.python_model("ard_60x4", upto=n)
        assert GP.R.shape == (5 * n, 5 * n)
        assert np.array_equal(GP.X, fresh.X) and np.array_equal(GP.Y, fresh.Y) and np.array_equal(GP.G, fresh.G)
        for a, b in zip(GP.posteriors(Q), fresh.posteriors(Q)):
            assert same_bits(a, b)
        assert np.array_equal(GP.R, fresh.R) and np.array_equal(GP.L, fresh.L)


def test_the_python_gnoise_vector_reaches_the_device_as_given(lib):
    from ibo_amd.gaussianprocess import GaussianProcess
    h, c, _, Q, _ = device_case("ard_60x3_gn")
    GP = GaussianProcess(tg.make_kernel("ard", [0.5, 0.7, 0.6]), c["X"], c["Y"], noise=c["noise"], gnoise=[1e-4, 3e-3, 0.05], G=c["G"])
    assert np.array_equal(GP.gnoise, c["gnoise"])
    assert np.array_equal(GP.R, h.matrix("R")) and np.array_equal(GP.L, h.matrix("L"))
    raw = h.batch(Q, want=("mu", "s2"))
    mu, s2 = GP.posteriors(Q)
    assert same_bits(mu, raw["mu"]) and same_bits(s2, raw["s2"])
    other = GaussianProcess(tg.make_kernel("ard", [0.5, 0.7, 0.6]), c["X"], c["Y"], noise=c["noise"], gnoise=[0.05, 3e-3, 1e-4], G=c["G"])
    assert not np.array_equal(other.R, GP.R)                           # the order matters
    for wrong in ([1e-4, 3e-3], [1e-4, 3e-3, 0.05, 0.05]):
        with pytest.raises(ValueError):
            GaussianProcess(tg.make_kernel("ard", [0.5, 0.7, 0.6]), c["X"], c["Y"], noise=c["noise"], gnoise=wrong, G=c["G"])


# ---------------------------------------------------------------------------- chunks by bytes
BYTES_CHUNK = 65280                  # what chunk_length (abi_rows.hip) allows a frame of 64 rows: the grid's limit, not the 256 MiB


def test_a_sweep_across_the_by_bytes_chunk_border(lib):
    """se_1x1 (Npad 64), ggp_chunk = 0: 65280 + 5 candidates are two chunks.  Outputs against the host batch in chunks of 256, the arg-max
    against NumPy's with the winner planted just before, on and behind the border, and the lowest index of a duplicated winner across it"""
    h, c, _, _, _ = device_case("se_1x1")
    M = BYTES_CHUNK + 5
    Q = lib.f64(np.random.RandomState(41).rand(M, 1))

    def batch256(pts):
        assert lib.lib.ibo_set_option(b"ggp_chunk", 256) == 0
        try:
            return h.batch(pts, *EI)
        finally:
            assert lib.lib.ibo_set_option(b"ggp_chunk", 0) == 0

    def sweep0(pts, outputs=True):
        assert lib.lib.ibo_set_option(b"ggp_chunk", 0) == 0
        return h.sweep(lib.DeviceArray.from_host(pts), M, *EI, index_base=0, outputs=outputs)

    base = batch256(Q)
    r = sweep0(Q)
    for k in ("mu", "s2", "acq"):
        assert same_bits(r[k], base[k]), k
    k0 = int(np.argmax(base["acq"]))
    assert r["best_idx"] == k0 and r["best_val"] == base["acq"][k0]
    best, dull = Q[k0].copy(), Q[int(np.argmin(base["acq"]))].copy()
    for at in (BYTES_CHUNK - 1, BYTES_CHUNK, BYTES_CHUNK + 4):
        Q2 = Q.copy(); Q2[k0] = dull; Q2[at] = best                    # the winner lives at `at` alone
        want = batch256(Q2)
        assert int(np.argmax(want["acq"])) == at
        r = sweep0(Q2)
        assert same_bits(r["acq"], want["acq"])
        assert r["best_idx"] == at and r["best_val"] == want["acq"][at], (at, r["best_idx"])
    Q3 = Q.copy(); Q3[k0] = dull; Q3[100] = best; Q3[BYTES_CHUNK + 1] = best
    r = sweep0(Q3, outputs=False)
    assert r["best_idx"] == 100 and r["best_val"] == base["acq"][k0]


# ---------------------------------------------------------------------------- the timing path
def test_timing_changes_no_bit_and_fills_its_slots(lib):
    """ggp_timing = 1 (events and a stream synchronisation per chunk): the fit, the batch and the sweep return the bits they return without
    it; the eight sums are finite and >= 0, the fit's (0, 6, 7) and the chunks' (1, 2, 3, 5) are filled, [4] -- this unit has no cross
    stage -- is 0 as include/ibo_abi.h says (it used to collect the gap between two event records, 0.03 ms over six chunks); a reset
    clears them.  No bound on any time."""
    c = gr.case("m5_43x2")
    Q = lib.f64(np.random.RandomState(17).rand(600, 2))
    cand = lib.DeviceArray.from_host(Q)
    ms = np.full(8, -1.0)

    def run():
        h = Handle(c["kern"], c["X"], c["Y"], c["G"], c["noise"], c["gnoise"])
        out = (h.matrix("L"), h.batch(Q, *EI), h.sweep(cand, 600, *EI, index_base=3))
        h.close()
        return out
    assert lib.lib.ibo_set_option(b"ggp_chunk", 256) == 0               # three chunks per call
    try:
        off = run()
        assert lib.lib.ibo_ggp_stage_ms(lib.dp(ms), 1) == 0 and np.all(ms == 0.0)      # nothing is timed unless asked
        assert lib.lib.ibo_set_option(b"ggp_timing", 1) == 0
        on = run()
        assert lib.lib.ibo_set_option(b"ggp_timing", 0) == 0
        assert lib.lib.ibo_ggp_stage_ms(lib.dp(ms), 0) == 0
        print("stage ms:", ms)
        assert np.all(np.isfinite(ms)) and np.all(ms >= 0.0) and ms[4] == 0.0
        assert ms[0] + ms[6] + ms[7] > 0.0 and ms[1] + ms[2] + ms[3] + ms[5] > 0.0
        again = np.full(8, -1.0)
        assert lib.lib.ibo_ggp_stage_ms(lib.dp(again), 1) == 0 and np.array_equal(again, ms)
        assert lib.lib.ibo_ggp_stage_ms(lib.dp(again), 0) == 0 and np.all(again == 0.0)
    finally:
        assert lib.lib.ibo_set_option(b"ggp_timing", 0) == 0 and lib.lib.ibo_set_option(b"ggp_chunk", 0) == 0
    assert np.array_equal(on[0], off[0])
    for k in ("mu", "s2", "acq"):
        assert same_bits(on[1][k], off[1][k]) and same_bits(on[2][k], off[2][k])
    assert on[2]["best_idx"] == off[2]["best_idx"] and on[2]["best_val"] == off[2]["best_val"]


# ---------------------------------------------------------------------------- translated inputs
@pytest.mark.parametrize("kind,hyper", [("ard", [0.5, 0.7, 0.6]), ("iso", [0.6]), ("m3", [0.6, 0.9]), ("m5", [0.5, 0.9])])
def test_a_common_shift_of_data_and_queries_changes_no_bit(lib, kind, hyper):
    """X and Q on the 2^-10 grid, both moved by the integer vector (37, -5, 1024): every difference x - x' is exact before and after, and
    the kernels form the difference before anything else (wsqdist_dev, ta, tb) -- a dot form or a scaled copy would not survive this"""
    from oracle import oracle as orc
    kern = orc.Kern(kind, hyper)
    rs = np.random.RandomState(61)
    N, D, M = 70, 3, 130
    X = np.floor(rs.rand(N, D) * 1024.0) / 1024.0
    X[40] = X[7]                                                       # r = 0 off the diagonal, shifted too
    Q = np.floor(rs.rand(M, D) * 1024.0) / 1024.0
    Q[::16] = X[:len(Q[::16])]
    Y, G = gr.objective(X)
    shift = np.array([37.0, -5.0, 1024.0])
    assert np.array_equal((X + shift) - shift, X) and np.array_equal((Q + shift) - shift, Q)
    assert np.array_equal((Q + shift)[:, None, :] - (X + shift)[None, :, :], Q[:, None, :] - X[None, :, :])
    res = []
    for s in (np.zeros(3), shift):
        h = Handle(kern, X + s, Y, G, 0.1, [1e-4, 3e-3, 0.05])
        res.append((h.matrix("R"), h.matrix("L"), h.batch(Q + s, *EI), check_sweep(lib, h, Q + s)))
        h.close()
    a, b = res
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    for k in ("mu", "s2", "acq"):
        assert same_bits(a[2][k], b[2][k]) and same_bits(a[3][k], b[3][k]), k
    assert a[3]["best_idx"] == b[3]["best_idx"] and a[3]["best_val"] == b[3]["best_val"]

"""
The arg-max contract (include/ibo_abi.h; csrc/ibo_common.h above wave_argmax) at every reduction boundary on every route: the largest
value wins, the FIRST index wins ties, NaN values / excluded rows / lanes past M never win, -1 when nothing is admissible, index_base
added -- ibo_acq_sweep on each of its kernels, ibo_acq_sweep_incremental, ibo_acq_sweep_exchange, ibo_cacq_sweep, ibo_kg_sweep.

Ties are made by the plateau construction of tests/argmax_reference.py (far rows: k* = 0 exactly, the same bits wherever they
stand; the margin over every other row is proved on the CPU by tests/test_argmax_reference.py).  Only index equality, bit equality
and the project's 1e-6 relative bar (the plateau against its float64 closed form) are asserted.
"""
import ctypes

import numpy as np
import pytest

import argmax_reference as ar

pytestmark = pytest.mark.gpu

BIG_BASE = (1 << 33) + 5
BASES = (0, 1000, BIG_BASE)
M_TILE = 16384 + 64 + 5          # 258 partials of the 64-candidate kernels: two rounds of argmax_final_kernel's 256-stride loop
M_FIN = 65536 + 256 + 7          # 258 partials of the 256-candidate finish kernels; beyond ibo_kg_sweep's chunk limit of 65280
PAYLOAD = np.uint64(0x7FF8DEADBEEF0001)      # a NaN no kernel produces
GUARD = 512


@pytest.fixture(scope="module")
def ibo():
    import ibo_amd
    from ibo_amd import _lib
    if _lib.device_count() < 1:
        pytest.fail("no GPU visible: the product has no CPU fallback")
    return ibo_amd


def kernel_of(name):
    from ibo_amd.gaussianprocess import kernel as K
    _, _, _, kind, hyper = ar.MODELS[name]
    return {"ard": K.GaussianKernel_ard, "m5": K.MaternKernel5, "m3": K.MaternKernel3}[kind](list(hyper))


def new_model(name, reserve_rows=0):
    from ibo_amd.gaussianprocess import GaussianProcess
    X, Y = ar.model_data(name)
    return GaussianProcess(kernel_of(name), X, Y, noise=ar.NOISE, reserve_rows=reserve_rows)


_MODELS = {}


def model(name):
    """one fitted model per name for the whole file (never mutated: the tests that add data fit their own)"""
    if name not in _MODELS:
        _MODELS[name] = new_model(name)
    return _MODELS[name]


class options(object):
    """ibo_set_option switches for the length of a with-block, the defaults restored afterwards"""
    DEFAULT = {"sweep_path": 0, "dot_form": -1, "gallery_prune": 1, "kg_chunk": 0, "cacq_chunk": 0}

    def __init__(self, **kw):
        self.kw = kw

    def __enter__(self):
        from ibo_amd import _lib
        try:
            for k, v in self.kw.items():
                _lib.check(_lib.lib.ibo_set_option(k.encode(), v))
        except Exception:
            self.__exit__()
            raise

    def __exit__(self, *exc):
        from ibo_amd import _lib
        for k in self.kw:
            _lib.check(_lib.lib.ibo_set_option(k.encode(), self.DEFAULT[k]))
        return False


# one-shot routes of ibo_acq_sweep: name -> (model, options, M, reported kernel, candidates per partial, seams inside [1, M))
ROUTES = {
    "gemv": ("se193", dict(dot_form=0), 16, "sweep_gemv_kernel", 64, ()),
    "wkl_small": ("se193", {}, 128, "wk_small_kernel", 64, (16, 32, 64)),                # wave-local launch: N <= 512, M <= 128
    "wk_small_1": ("se1024", {}, 256, "wk_small_kernel", 64, (16, 32, 64)),              # one 16-candidate block per workgroup
    "wk_small_2": ("se1024", {}, 4096, "wk_small_kernel", 64, (16, 32, 64, 256)),
    "split": ("se193", dict(sweep_path=3), M_TILE, "sweep_mfma_kernel<split>", 64, (16, 32, 64, 256, 16384)),
    "tile_diff": ("se193", dict(dot_form=0), M_TILE, "sweep_mfma_kernel", 64, (16, 32, 64, 256, 16384)),
    "sweep2_se": ("se193", {}, M_FIN, "sweep2_kernel", 256, (16, 32, 64, 256, 16384, 65536)),
    "sweep2_m5": ("m5_512", {}, M_FIN, "sweep2_kernel", 256, (32, 256, 65536)),
    "sweep2_m3": ("m3_64", {}, M_FIN, "sweep2_kernel", 256, (32, 256, 65536)),
    "tile_diff_m5": ("m5_512", dict(dot_form=0), M_TILE, "sweep_mfma_kernel", 64, (64, 16384)),
    "wkl_small_m3": ("m3_64", {}, 128, "wk_small_kernel", 64, (16, 64)),
}


def position_sets(M, g, seams):
    """the sets P of tied rows for an array of M candidates reduced g at a time: the ends, both sides of every seam and the seam alone (it
    can win, and loses on index only), two partials on one thread of argmax_final_kernel, a spread set; each a list in planting order"""
    sets = [[0], [M - 1], [0, M - 1]]
    for b in seams:
        if 0 < b < M:
            sets += [[b - 1, b], [b]]
    nparts = (M + g - 1) // g
    if nparts > 256:
        # two partials that land on the same thread of argmax_final_kernel (e and e + 256): the later one listed first
        hi = 300 if 300 < nparts else nparts - 1
        sets += [[hi * g, (hi - 256) * g], [hi * g]]
    step = M // 5                                                              # (more than a workgroup's candidates wherever M allows)
    spread = [min(M - 1, 4 * step + 3), 3 * step + 2, 2 * step + 1, step]      # four workgroups (where there are four), descending
    if step >= 2:
        sets.append(spread)
    return sets


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def plateau_of(GP, acq):
    name, parm = ar.ACQS[acq]
    return ar.plateau_value(name, parm, float(np.max(GP.Y)))


def sweep_kw(acq):
    name, parm = ar.ACQS[acq]
    return dict(acq=name, parm=parm, native=True)


def check_winner(r, values, cand, P, base, plateau, exclude=None, radius=0.0, what=""):
    """the assertions on one result (tied rows bit-equal, plateau value, the rule on the written values, the lowest tied row wins): r = dict(best_val, best_idx), values = the written acquisition"""
    P = sorted(P)
    assert len(set(bits(values[P]).tolist())) == 1, "far rows differ in bits %s %s" % (what, [values[p].hex() for p in P])
    others = np.delete(values, P)
    if len(others):
        assert np.nanmax(others) < ar.MARGIN * plateau, "input condition: a loser reaches %g of the plateau %s" % (np.nanmax(others) / plateau, what)
    assert abs(values[P[0]] - plateau) <= 1e-6 * abs(plateau), (values[P[0]], plateau, what)
    want = ar.argmax_rule(values, cand, exclude, radius, base)
    assert (r["best_val"], r["best_idx"]) == want, (r["best_val"], r["best_idx"], want, what)
    if exclude is None:
        assert r["best_idx"] == base + P[0], (r["best_idx"], base, P, what)
        assert bits(r["best_val"])[()] == bits(values[P[0]])[()], what


@pytest.mark.parametrize("route", sorted(ROUTES))
def test_positions_and_index_base_on_every_one_shot_route(ibo, route):
    """(a), (b): far rows at the reduction seams of the route; every acquisition and every index base at least once per route"""
    from ibo_amd.acquisition import sweep
    mname, opts, M, kernel, g, seams = ROUTES[route]
    GP = model(mname)
    D = GP.X.shape[1]
    with options(**opts):
        for n, P in enumerate(position_sets(M, g, seams)):
            cand = ar.plant(M, D, P)
            runs = [("ei", BASES[n % 3])]
            if n == 2:
                runs = [(a, b) for a in ("ei", "pi", "ucb") for b in BASES]
            for acq, base in runs:
                r = sweep(GP, cand, index_base=base, outputs=("acq",), **sweep_kw(acq))
                assert r["kernel"] == kernel, (route, r["kernel"])
                check_winner(r, r["acq"], cand, P, base, plateau_of(GP, acq), what=(route, P, acq, base))


def excl_cases(cand, P, D):
    """(c): (exclude, radius, expected winner's row or -1) for a two-member P"""
    lo, hi = sorted(P)
    step = np.zeros(D); step[0] = 0.25
    return [([cand[lo]], 1e-9, hi),                                         # the lowest member inside a ball: the next one wins
            ([cand[lo] + step], 0.25, hi),                                  # at exactly 0.25: the boundary is closed
            ([cand[lo] + step], float(np.nextafter(0.25, 0)), lo),          # ... and admitted one ulp inside
            ([cand[hi] + step, cand[lo] - step], 0.25, None),                   # both far rows gone: whatever the rule names among the rest
            ([np.full(D, .5)], 1e6, -1)]                                    # everything excluded


@pytest.mark.parametrize("route", sorted(ROUTES))
def test_exclusion_balls_on_every_one_shot_route(ibo, route):
    from ibo_amd.acquisition import sweep
    mname, opts, M, kernel, g, seams = ROUTES[route]
    GP = model(mname)
    D = GP.X.shape[1]
    b = seams[-1] if seams else M // 2
    P = [b - 1, b]
    cand = ar.plant(M, D, P)
    plateau = plateau_of(GP, "ei")
    with options(**opts):
        r0 = sweep(GP, cand, outputs=("mu", "s2", "acq"), **sweep_kw("ei"))
        assert r0["kernel"] == kernel
        for excl, radius, winner in excl_cases(cand, P, D):
            r = sweep(GP, cand, exclude=excl, exclude_radius=radius, index_base=BIG_BASE, outputs=("mu", "s2", "acq"), **sweep_kw("ei"))
            assert r["kernel"] == kernel
            for k in ("mu", "s2", "acq"):
                assert np.array_equal(bits(r[k]), bits(r0[k])), (route, k, radius)      # outputs do not see the balls
            check_winner(r, r["acq"], cand, P, BIG_BASE, plateau, exclude=excl, radius=radius, what=(route, radius))
            if winner is not None:
                assert r["best_idx"] == (-1 if winner < 0 else BIG_BASE + winner), (route, radius, r["best_idx"])
            if winner == -1:
                assert r["best_val"] == -np.inf                              # what argmax_final_kernel writes for an empty arg-max


def nan_rows(M, p0):
    return sorted(set([0, p0 - 1, p0 + 1, M - 1]) - set([p0]))


@pytest.mark.parametrize("route", sorted(ROUTES))
def test_nan_candidates_on_every_one_shot_route(ibo, route):
    """(d): NaN rows at index 0, on both sides of the winner inside its 16-column block and its tile, and at M - 1 never win, come out
    as NaN, and leave every other row's mu, s2, acq bit for bit as without them; an all-NaN array has no winner"""
    from ibo_amd.acquisition import sweep
    mname, opts, M, kernel, g, seams = ROUTES[route]
    GP = model(mname)
    D = GP.X.shape[1]
    p0 = 37 if M > 64 else M // 2
    clean = ar.plant(M, D, [p0])
    bad = nan_rows(M, p0)
    cand = clean.copy()
    for n, i in enumerate(bad):
        if n % 2: cand[i] = np.nan                       # the whole row
        else: cand[i, n % D] = np.nan                    # one coordinate
    with options(**opts):
        r0 = sweep(GP, clean, outputs=("mu", "s2", "acq"), **sweep_kw("ei"))
        r = sweep(GP, cand, index_base=1000, outputs=("mu", "s2", "acq"), **sweep_kw("ei"))
        rn = sweep(GP, np.full((M, D), np.nan), index_base=1000, **sweep_kw("ei"))
    assert r["kernel"] == kernel and rn["kernel"] == kernel
    keep = np.setdiff1d(np.arange(M), bad)
    for k in ("mu", "s2", "acq"):
        assert np.all(np.isnan(r[k][bad])), (route, k, r[k][bad])
        assert np.array_equal(bits(r[k][keep]), bits(r0[k][keep])), (route, k)
    assert r["best_idx"] == 1000 + p0 and bits(r["best_val"])[()] == bits(r0["acq"][p0])[()]
    assert (r["best_val"], r["best_idx"]) == ar.argmax_rule(r["acq"], index_base=1000)
    assert rn["best_idx"] == -1 and rn["best_val"] == -np.inf


# ---------------------------------------------------------------------------------------------- the kept state
@pytest.mark.parametrize("mname,acq", [("se1024", "ei"), ("m5_512", "ucb"), ("m5_512", "pi")])
@pytest.mark.parametrize("prune", [0, 1, 2])
def test_kept_state_positions_before_and_after_a_new_row(ibo, mname, acq, prune):
    """ibo_acq_sweep_incremental under gallery_prune 0 / 1 / 2: the arg-max-only call that forms the state, the call with outputs that
    completes it, and the lazy refresh after a one-row addData"""
    from ibo_amd import DeviceArray
    from ibo_amd.acquisition import sweep
    M, g = M_FIN, 256
    D = ar.MODELS[mname][2]
    two_part = prune != 0 and acq != "pi"                # PI is not monotone in the variance: one kernel, every tile complete
    Xn = np.random.RandomState(5).rand(3, D)
    sets = [[0, M - 1], [31, 32], [255, 256], [65535, 65536], [257 * g, g], [M - 1]]
    with options(gallery_prune=prune):
        for n, P in enumerate(sets):
            GP = new_model(mname, reserve_rows=4)        # (head-room: the new row extends the factor in place, the state survives)
            plateau = plateau_of(GP, acq)
            cand = ar.plant(M, D, P)
            dc = DeviceArray.from_host(cand)
            base = BASES[n % 3]
            first = sweep(GP, dc, index_base=base, incremental=True, **sweep_kw(acq))
            assert first["kernel"] == ("sweep2_kernel<part>" if two_part else "sweep2_kernel"), first["kernel"]
            full = sweep(GP, dc, index_base=base, incremental=True, outputs=("acq",), **sweep_kw(acq))
            check_winner(first, full["acq"], cand, P, base, plateau, what=(mname, prune, P, "first"))
            check_winner(full, full["acq"], cand, P, base, plateau, what=(mname, prune, P, "full"))
            GP.addData(Xn[n % 3], -4.5)                  # below every observation: the incumbent stays
            again = sweep(GP, dc, index_base=base, incremental=True, **sweep_kw(acq))
            assert again["kernel"] == "sweep2_rank1_kernel", again["kernel"]
            excl, radius, winner = excl_cases(cand, [P[0], P[-1]], D)[0] if len(P) > 1 else ([np.full(D, .5)], 1e6, -1)
            ex = sweep(GP, dc, index_base=base, incremental=True, exclude=excl, exclude_radius=radius, **sweep_kw(acq))
            after = sweep(GP, dc, index_base=base, incremental=True, outputs=("acq",), **sweep_kw(acq))
            check_winner(again, after["acq"], cand, P, base, plateau, what=(mname, prune, P, "refreshed"))
            assert (ex["best_val"], ex["best_idx"]) == ar.argmax_rule(after["acq"], cand, excl, radius, base), (mname, prune, P)
            assert ex["best_idx"] == (-1 if winner < 0 else base + winner)


# ---------------------------------------------------------------------------------------------- constrained and KG
def constraints_of(which):
    from ibo_amd.acquisition.constrained import Constraint
    # far rows: mean 0, feasible with Phi(1 / sqrt(1.1)) = 0.83; unit-cube rows: mean about -4
    table = {"one": [("m3_64", -1.0)], "two": [("m3_64", -1.0), ("m5_512", -1.0)], "twice": [("m3_64", -1.0), ("m3_64", -1.5)],
             "objective": [("se193", -1.0)]}
    return [Constraint(model(m), lower=t) for m, t in table[which]]


def cacq_plateau(GP, cons, acq):
    name, parm = ar.ACQS[acq]
    v = ar.plateau_value(name, parm, float(np.max(GP.Y)))
    for c in cons:
        v *= ar._cdf(c.sense * (c.thresh - 0.0) / np.sqrt(1.0 + ar.NOISE))
    return v


def csweep(GP, cons, cand, acq="ei", **kw):
    from ibo_amd.acquisition.constrained import sweepConstrained
    name, parm = ar.ACQS[acq]
    r = sweepConstrained(GP, cons, cand, acq=name, xi=parm, native=True, ymax=float(np.max(GP.Y)), outputs=("acq", "pof", "val"), **kw)
    assert r["acq_used"] == name
    return r


@pytest.mark.parametrize("which", ["one", "two"])
def test_constrained_sweep_positions_exclusion_and_nan(ibo, which):
    GP = model("se193")
    cons = constraints_of(which)
    M, g, D = M_FIN, 256, 3
    for n, P in enumerate(position_sets(M, g, (64, 256, 65536))):
        cand = ar.plant(M, D, P)
        acq = ("ei", "pi")[n % 2]
        r = csweep(GP, cons, cand, acq, index_base=BASES[n % 3])
        check_winner(r, r["val"], cand, P, BASES[n % 3], cacq_plateau(GP, cons, acq), what=(which, P, acq))
    P = [65535, 65536]
    cand = ar.plant(M, D, P)
    r0 = csweep(GP, cons, cand)
    for excl, radius, winner in excl_cases(cand, P, D):
        r = csweep(GP, cons, cand, exclude=excl, exclude_radius=radius, index_base=BIG_BASE)
        for k in ("acq", "pof", "val"):
            assert np.array_equal(bits(r[k]), bits(r0[k])), (which, k, radius)
        check_winner(r, r["val"], cand, P, BIG_BASE, cacq_plateau(GP, cons, "ei"), exclude=excl, radius=radius, what=(which, radius))
        if winner is not None:
            assert r["best_idx"] == (-1 if winner < 0 else BIG_BASE + winner)
        if winner == -1:
            assert r["best_val"] == -np.inf
    # (d) NaN rows; M small enough that the per-model sweeps run on small2.hip's kernels too
    for M in (M_FIN, 300):
        p0 = 37
        clean = ar.plant(M, D, [p0])
        bad = nan_rows(M, p0)
        cand = clean.copy()
        cand[bad[0], 1] = np.nan; cand[bad[1:]] = np.nan
        r0 = csweep(GP, cons, clean); r = csweep(GP, cons, cand, index_base=1000)
        keep = np.setdiff1d(np.arange(M), bad)
        for k in ("acq", "pof", "val"):
            assert np.all(np.isnan(r[k][bad])), (which, M, k, r[k][bad])
            assert np.array_equal(bits(r[k][keep]), bits(r0[k][keep])), (which, M, k)
        assert r["best_idx"] == 1000 + p0 and (r["best_val"], r["best_idx"]) == ar.argmax_rule(r["val"], index_base=1000)
        rn = csweep(GP, cons, np.full((M, D), np.nan), index_base=1000)
        assert rn["best_idx"] == -1 and rn["best_val"] == -np.inf


_KG = []


def kg_case():
    """(model, reference points, strong row, weak rows, the strong row's value under tests/kg_reference.py)"""
    if not _KG:
        A, strong, weak, best, _ = ar.kg_inputs()
        _KG.append((model(ar.KG_MODEL), A, strong, weak, best))
    return _KG[0]


def check_kg(got, cand_P, base, best):
    bv, bi, v = got
    Ps = sorted(cand_P)
    assert len(set(bits(v[Ps]).tolist())) == 1, "copies of one row differ in bits %s" % [v[p].hex() for p in Ps]
    assert np.max(np.delete(v, Ps)) < ar.MARGIN * v[Ps[0]], (v[Ps[0]], best)
    assert (bv, bi) == ar.argmax_rule(v, index_base=base) and bi == base + Ps[0] and bits(bv)[()] == bits(v[Ps[0]])[()], (cand_P, bv, bi)


def test_knowledge_gradient_positions(ibo):
    """ibo_kg_sweep against 8 reference points: 258 partials of kg_argmax_kernel, two chunks (65280 + 519 candidates); the ties are
    copies of the row with the largest knowledge gradient (a far row's own line is the incumbent: it is worth nothing)"""
    from ibo_amd.acquisition import sweepKG
    GP, A, strong, weak, best = kg_case()
    M, g = M_FIN, 256
    for n, P in enumerate(position_sets(M, g, (64, 256, 65280, 65536))):
        cand = ar.plant_kg(M, P, strong, weak)
        base = BASES[n % 3]
        check_kg(sweepKG(GP, cand, A, values=True, index_base=base), P, base, best)


# ---------------------------------------------------------------------------------------------- (e) outputs touch exactly [0, M)
WINDOW_M = (1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 255, 256, 257, 4096, 4097, 8192, 8193)


class Windows(object):
    """n output arrays of up to `cap` elements as interior windows of ONE device buffer: GUARD payload words before and after each"""

    def __init__(self, n, cap, device):
        from ibo_amd import DeviceArray
        self.n, self.cap, self.span = n, cap, cap + 2 * GUARD
        self.buf = DeviceArray((n * self.span,), device)
        self.fill = np.full(n * self.span, PAYLOAD, dtype=np.uint64).view(np.float64)

    def reset(self):
        self.buf.upload(self.fill)

    def ptr(self, k):
        return ctypes.c_void_p(self.buf.ptr.value + 8 * (k * self.span + GUARD))

    def read(self, M, what):
        """the n windows' first M values, after checking every word around them and that no payload is left inside"""
        h = self.buf.to_host().view(np.uint64).reshape(self.n, self.span)
        out = []
        for k in range(self.n):
            assert np.all(h[k, :GUARD] == PAYLOAD), "output %d: a word BEFORE the window was written %s" % (k, what)
            after = h[k, GUARD + M:]
            assert np.all(after == PAYLOAD), "output %d: word %d past the window was written %s" % (k, int(np.flatnonzero(after != PAYLOAD)[0]), what)
            assert not np.any(h[k, GUARD:GUARD + M] == PAYLOAD), "output %d: an element of [0, M) was not written %s" % (k, what)
            out.append(h[k, GUARD:GUARD + M].copy())
        return out


def raw_acq_sweep(GP, cand_ptr, M, w):
    """ibo_acq_sweep as acquisition.sweep(native=True, acq='ei') calls it, the three outputs into the windows w"""
    from ibo_amd import _lib
    h = GP._handle()
    GP._push_prior()
    _, _, sf2_py, sf2_native = GP.kernel._ibo_spec()
    bv = ctypes.c_double(); bi = ctypes.c_int64()
    _lib.check(_lib.lib.ibo_gp_set_kstar_sf2(h, sf2_native))
    try:
        _lib.check(_lib.lib.ibo_acq_sweep(h, M, cand_ptr, _lib.ACQ_EI, .01, _lib.ERF_LIBM, _lib.CLAMP_NATIVE, float("nan"), 0, None, 0.0, 0,
                                          w.ptr(0), w.ptr(1), w.ptr(2), ctypes.byref(bv), ctypes.byref(bi)))
    finally:
        _lib.check(_lib.lib.ibo_gp_set_kstar_sf2(h, sf2_py))
    return bv.value, bi.value


def raw_cacq_sweep(GP, cons, cand_ptr, M, w):
    from ibo_amd import _lib
    from ibo_amd.acquisition.constrained import _pack
    n, con, thresh, sense = _pack(cons)
    GP._push_prior()
    bv = ctypes.c_double(); bi = ctypes.c_int64()
    _lib.check(_lib.lib.ibo_cacq_sweep(GP._handle(), n, con, _lib.dp(thresh), sense, M, cand_ptr, _lib.ACQ_EI, .01, _lib.ERF_NR, _lib.CLAMP_PY,
                                       float(np.max(GP.Y)), 0, None, 0.0, 0, w.ptr(0), w.ptr(1), w.ptr(2), ctypes.byref(bv), ctypes.byref(bi)))
    return bv.value, bi.value


def raw_kg_sweep(GP, A, cand_ptr, M, w):
    from ibo_amd import _lib
    A = _lib.f64(A)
    GP._push_prior()
    bv = ctypes.c_double(); bi = ctypes.c_int64()
    _lib.check(_lib.lib.ibo_kg_sweep(GP._handle(), len(A), _lib.dp(A), M, cand_ptr, 1, _lib.CLAMP_PY, 0, w.ptr(0), ctypes.byref(bv), ctypes.byref(bi)))
    return bv.value, bi.value


def window_cases(call, nout, D, groups, device, what):
    """call(cand_ptr, M, windows) -> (best_val, best_idx).  groups: (longest M of a route, the Ms that run on it); every M's outputs
    against guard words and against the same rows of the route's longest array"""
    from ibo_amd import DeviceArray
    cap = max(g[0] for g in groups)
    cand = np.random.RandomState(3).rand(cap, D)
    dc = DeviceArray.from_host(cand, device)
    w = Windows(nout, cap, device)
    for longest, Ms in groups:
        w.reset()
        call(dc.ptr, longest, w)
        ref = w.read(longest, (what, longest))
        for M in Ms:
            w.reset()
            bv, bi = call(dc.ptr, M, w)
            got = w.read(M, (what, M))
            for k in range(nout):
                assert np.array_equal(got[k], ref[k][:M]), "output %d differs from the longer array's rows %s" % (k, (what, M, longest))
            assert (bv, bi) == ar.argmax_rule(got[nout - 1].view(np.float64)), (what, M)


# which of WINDOW_M share a route (the groups' first element is the route's longest array here)
DOT_GROUPS = ((128, (1, 15, 16, 17, 31, 32, 33, 63, 64, 65)), (256, (255, 256)), (4096, (257, 4096)), (8193 + 39, (4097, 8192, 8193)))
DIFF_GROUPS = ((16, (1, 15, 16)), (8192, (17, 31, 32, 33, 63, 64, 65, 255, 256, 257, 4096, 4097, 8192)), (8193 + 39, (8193,)))
assert sorted(m for _, ms in DOT_GROUPS for m in ms) == sorted(WINDOW_M) == sorted(m for _, ms in DIFF_GROUPS for m in ms)


@pytest.mark.parametrize("form", ["dot", "diff"])
def test_plain_sweep_outputs_touch_exactly_their_window(ibo, form):
    GP = model("se193")
    with options(dot_form=-1 if form == "dot" else 0):
        window_cases(lambda p, M, w: raw_acq_sweep(GP, p, M, w), 3, 3, DOT_GROUPS if form == "dot" else DIFF_GROUPS, GP._dev.device, form)


def test_constrained_sweep_outputs_touch_exactly_their_window(ibo):
    GP = model("se193")
    cons = constraints_of("one")
    window_cases(lambda p, M, w: raw_cacq_sweep(GP, cons, p, M, w), 3, 3, DOT_GROUPS, GP._dev.device, "cacq")


def test_knowledge_gradient_outputs_touch_exactly_their_window(ibo):
    GP, A = kg_case()[:2]
    window_cases(lambda p, M, w: raw_kg_sweep(GP, A, p, M, w), 1, 3, ((8193, WINDOW_M),), GP._dev.device, "kg")


# ---------------------------------------------------------------------------------------------- (f) chunk seams
CHUNK_SETS = ([255, 256], [511, 768], [999, 0])


def test_knowledge_gradient_chunk_seams(ibo):
    from ibo_amd.acquisition import sweepKG
    GP, A, strong, weak, best = kg_case()
    for P in CHUNK_SETS:
        cand = ar.plant_kg(1000, P, strong, weak)
        whole = sweepKG(GP, cand, A, values=True, index_base=1000)
        with options(kg_chunk=256):
            parts = sweepKG(GP, cand, A, values=True, index_base=1000)
        assert np.array_equal(bits(parts[2]), bits(whole[2])) and parts[:2] == whole[:2], P
        check_kg(parts, P, 1000, best)


@pytest.mark.parametrize("which", ["one", "two", "twice", "objective"])
def test_constrained_sweep_chunk_seams(ibo, which):
    """ibo_set_option("cacq_chunk"): the chunk loop of ibo_cacq_sweep -- scratch stride, output and partial offsets, the chunk's first
    index, the wait between chunks -- against the one-chunk call, bit for bit"""
    GP = model("se193")
    cons = constraints_of(which)
    for P in CHUNK_SETS:
        cand = ar.plant(1000, 3, P)
        cases = [dict(index_base=0), dict(index_base=BIG_BASE, exclude=[cand[min(P)]], exclude_radius=1e-9),
                 dict(index_base=1000, exclude=[np.full(3, .5)], exclude_radius=1e6)]
        whole = [csweep(GP, cons, cand, **kw) for kw in cases]
        assert whole[0]["best_idx"] == min(P) and whole[1]["best_idx"] == BIG_BASE + max(P) and whole[2]["best_idx"] == -1
        for chunk in (256, 512, 300):                    # (300 is rounded up to 512)
            with options(cacq_chunk=chunk):
                parts = [csweep(GP, cons, cand, **kw) for kw in cases]
            for a, b, kw in zip(parts, whole, cases):
                for k in ("acq", "pof", "val"):
                    assert np.array_equal(bits(a[k]), bits(b[k])), (which, P, chunk, k)
                assert bits(a["best_val"])[()] == bits(b["best_val"])[()] and a["best_idx"] == b["best_idx"], (which, P, chunk, a["best_idx"], b["best_idx"])
                assert (a["best_val"], a["best_idx"]) == ar.argmax_rule(a["val"], cand, kw.get("exclude"), kw.get("exclude_radius", 0.0),
                                                                        kw["index_base"]), (which, P, chunk)


def test_cacq_chunk_option_is_checked(ibo):
    from ibo_amd import _lib
    assert _lib.lib.ibo_set_option(b"cacq_chunk", -1) == _lib.ERR_ARG
    _lib.check(_lib.lib.ibo_set_option(b"cacq_chunk", 0))


# ---------------------------------------------------------------------------------------------- (g) the ranks' exchange
def test_exchange_on_a_world_of_one(ibo):
    from ibo_amd import DeviceArray
    from ibo_amd.acquisition import sweep
    from ibo_amd.multigpu import RcclArgmax
    GP = model("se193")
    comm = RcclArgmax(1, 0, RcclArgmax.unique_id(), device=0)
    try:
        for M, P in ((M_FIN, [65536, 255, 65535]), (128, [64, 63]), (M_FIN, [257 * 256, 256])):
            cand = ar.plant(M, 3, P)
            dc = DeviceArray.from_host(cand)
            for inc in (False, True):
                r = sweep(GP, dc, index_base=BIG_BASE, exchange=comm, incremental=inc, **sweep_kw("ei"))
                assert r["global_idx"] == r["best_idx"] == BIG_BASE + min(P), (M, P, inc, r)
                assert r["global_val"] == r["best_val"] and r["global_rank"] == 0
                assert abs(r["best_val"] - plateau_of(GP, "ei")) <= 1e-6 * plateau_of(GP, "ei")
                assert np.array_equal(r["global_x"], cand[min(P)])
                r = sweep(GP, dc, index_base=BIG_BASE, exchange=comm, incremental=inc, exclude=[np.full(3, .5)], exclude_radius=1e6,
                          **sweep_kw("ei"))
                assert r["global_idx"] == -1 and r["best_idx"] == -1, (M, inc, r)
    finally:
        comm.close()

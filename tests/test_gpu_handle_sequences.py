"""
Life cycles of a fitted handle: long mixed sequences of the five entries that change it in place (ibo_gp_extend, ibo_gp_remove, ibo_gp_set_y,
ibo_gp_set_prior, ibo_gp_set_kstar_sf2), of refits, and of the readers whose derived state must follow (the kept sweep state of
ibo_acq_sweep_incremental, the lazily formed R, the lazily zeroed upper blocks of L), against a FRESH model on a host-side mirror of what
the handle should hold -- after every step.

Yardsticks, all taken from tests/test_gpu_remove.py (helpers imported, not restated):
    every step        posteriors at 64 points against the fresh model, 1e-6 relative / 1e-9 absolute (the parity bar)
    a kept-state sweep   the fresh model's full sweep: the same arg-max, or two indices whose values on the fresh model agree to 1e-12
    every tenth step and the last   L, W, R against NumPy at 1e-9 (check_factor); gradients, joint covariance, leave-one-out against the
                      fresh model at the bars of their own files (check_readers_like_fresh)
Noise .1 throughout the mixed sequences: cond_2(R) <= N (1 + noise) / noise < 1e6 at these sizes without a decomposition (cond_of's bound:
lambda_min >= noise because sf2 <= 1, lambda_max <= trace), asserted once per sequence on the largest N it reaches.

The length test holds the device's factor after 300 "append one, remove one" steps to a fresh NumPy factor at 1e-9 AND to flatness: its error
at step 300 may be at most 8 times the larger of the float64 restatement's worst checkpoint error on the same sequence
(downdate_reference.run_window, which tests/test_downdate_reference.py shows to stay flat over 1000 steps) and 1e-13.  The factor 8 is room
for another summation order (FMA contraction, 64-row segments), a margin over the reference and not over the device.
"""
import numpy as np
import pytest

import downdate_reference as dr
from oracle import oracle as orc
from test_gpu_remove import (NOISE, check_factor, check_loo_like_fresh, check_readers_like_fresh, get_W, make_prior, new_gp, ref_R,
                             values_close)
from wall_time import wall

pytestmark = pytest.mark.gpu

STEPS = 40
M_SWEEP = 9001
KSTAR_SCALE = .75           # the kstar operation's k* signal variance, in units of the model's own
OPS = ["add1", "addk", "add_refit", "rm1", "rm2", "rm_refit", "set_y", "prior", "kstar", "read_R", "read_L", "loo", "sweep"]


@pytest.fixture(scope="module")
def lib():
    from ibo_amd import _lib
    if _lib.device_count() < 1:
        pytest.fail("no GPU visible: the product has no CPU fallback")
    return _lib


def target(X, rs):
    X = np.atleast_2d(X)
    return np.sin(3 * X.sum(1)) + 0.01 * rs.randn(len(X))


def schedule(rs):
    """STEPS operations in a seeded order: every one of OPS twice, eleven more drawn at random, and once the three steps sweep, add one
    point, sweep next to each other -- the second of these sweeps finds a kept state with one appended row to fold in"""
    ops = OPS * 2
    ops += [OPS[k] for k in rs.randint(0, len(OPS), STEPS - 3 - len(ops))]
    rs.shuffle(ops)
    at = int(rs.randint(0, len(ops) + 1))
    return ops[:at] + ["sweep", "add1", "sweep"] + ops[at:]


class Driver:
    """one handle and the mirror of what it should hold: X, Y, the prior, the padded size; one operation per step"""

    def __init__(self, lib, kind, D, N0, reserve, prior, seed):
        from ibo_amd import DeviceArray
        self.lib, self.kind, self.D, self.N0, self.reserve = lib, kind, D, N0, reserve
        self.rs = np.random.RandomState(seed)
        self.X = self.rs.rand(N0, D)
        self.Y = target(self.X, self.rs)
        self.priors = [None, make_prior(D, 11), make_prior(D, 12)]
        self.pk = 1 if prior else 0
        self.GP = new_gp(kind, D, self.X, self.Y, reserve_rows=reserve)
        self.GP.prior = self.priors[self.pk]
        self.refits = 0
        self.pad_refits = 0                               # refits of an addData that EXTEND_MAX allowed and the padding did not
        fit = self.GP._fit_device

        def counted(*a, **k):
            self.refits += 1
            return fit(*a, **k)
        self.GP._fit_device = counted
        self.Npad = self.padded(N0)
        self.cand = DeviceArray.from_host(np.random.RandomState(seed + 1000).rand(M_SWEEP, D))
        self.Q = np.random.RandomState(5).rand(64, D) * 1.2 - .1
        self.sizes = [N0]
        self.kernels = []

    def padded(self, n):
        return -(-(n + self.reserve) // 64) * 64          # stage_data: rows + reserved rows, rounded up to 64, at every fit

    def fresh(self):
        fr = new_gp(self.kind, self.D, self.X, self.Y)
        fr.prior = self.priors[self.pk]
        return fr

    # ------------------------------------------------------------------------------------------------ operations
    def add(self, k, refit):
        x = self.rs.rand(k, self.D)
        y = target(x, self.rs)
        before, room = self.refits, self.Npad - len(self.X)
        self.GP.addData(x if k > 1 else x[0], y if k > 1 else y[0])
        self.X, self.Y = np.r_[self.X, x], np.r_[self.Y, y]
        assert self.refits - before == int(refit), ("addData of %d rows at N=%d, padded %d" % (k, len(self.X) - k, self.Npad), self.refits - before)
        if refit:
            self.pad_refits += int(room < k <= self.GP.EXTEND_MAX)
            self.Npad = self.padded(len(self.X))

    def remove(self, rows, route, refit):
        before = self.refits
        self.GP.removeData(rows if len(rows) > 1 else rows[0], _route=route)
        keep = np.setdiff1d(np.arange(len(self.X)), rows)
        self.X, self.Y = self.X[keep], self.Y[keep]
        assert self.refits - before == int(refit), ("removeData of %s" % (rows,), self.refits - before)
        if refit:
            self.Npad = self.padded(len(self.X))

    def step(self, op):
        GP, rs, lib = self.GP, self.rs, self.lib
        N = len(self.X)
        room = self.Npad - N
        if op in ("addk", "add_refit") and N > self.N0 + 20:      # the model has grown enough: back below where it began
            op = "rm_refit"
        if op.startswith("rm") and N < 8:
            op = "add1"
        if op == "add1":
            self.add(1, room < 1)
        elif op == "addk":
            k = int(rs.randint(2, 6))
            self.add(k, room < k)
        elif op == "add_refit":                           # past the padding where that is a few rows away, else more rows than EXTEND_MAX
            k = room + 1 if room + 1 <= 5 else GP.EXTEND_MAX + 1
            self.add(k, True)
        elif op == "rm1":
            self.remove([[0, N - 1, int(rs.randint(0, N))][int(rs.randint(0, 3))]], "device", False)
        elif op == "rm2":
            self.remove(sorted(int(r) for r in rs.choice(N, 2, replace=False)), "device", False)
        elif op == "rm_refit":                            # more rows than REMOVE_MAX: the class refits
            k = max(GP.REMOVE_MAX + 1, N - self.N0 + 2)
            self.remove(sorted(int(r) for r in rs.choice(N, k, replace=False)), None, True)
        elif op == "set_y":
            self.Y = self.Y + .05 * rs.randn(N)
            lib.check(lib.lib.ibo_gp_set_y(GP._handle(), lib.dp(lib.f64(self.Y))))
            GP.Y = self.Y.copy()
        elif op == "prior":                               # none -> one -> another -> none
            self.pk = (self.pk + 1) % 3
            GP.prior = self.priors[self.pk]
        elif op == "kstar":
            self.kstar()
        elif op == "read_R":
            np.testing.assert_allclose(GP.R, ref_R(self.kind, self.D, self.X), rtol=1e-12, atol=0)
        elif op == "read_L":
            L = GP.L
            assert np.array_equal(L, np.tril(L)) and dr.relerr(L, np.linalg.cholesky(ref_R(self.kind, self.D, self.X))) <= 1e-9
        elif op == "loo":
            check_loo_like_fresh(GP, self.fresh(), self.kind, self.D, "loo")
        elif op == "sweep":
            self.sweep()
        else:
            raise ValueError(op)
        self.sizes.append(len(self.X))
        return op

    def sweep(self, fr=None):
        """one kept-state sweep against the full sweep of a fresh model (fr: that model, where the caller has prepared one); its kernel"""
        from ibo_amd.acquisition import sweep
        r = sweep(self.GP, self.cand, acq='ei', xi=.1, native=False, incremental=True)
        f = sweep(self.fresh() if fr is None else fr, self.cand, acq='ei', xi=.1, native=False, outputs=("acq",))
        self.kernels.append(r["kernel"])
        a, b = f["acq"][r["best_idx"]], f["acq"][f["best_idx"]]
        assert r["best_idx"] == f["best_idx"] or abs(a - b) <= 1e-12 * abs(b), (r["kernel"], r["best_idx"], f["best_idx"], a, b)
        return r["kernel"]

    def kstar(self):
        """Another k* signal variance, c times the model's own, for a read and a kept-state sweep; then the model's own again.
        ibo_gp_set_kstar_sf2 scales k* by c and leaves R alone, so with m the prior's mean, (mu0, s2_0) the fresh model's posterior under
        its own variance and R's diagonal 1 + noise whatever sf2 (the Python-class rule):
            mu = m + c (mu0 - m)        s2 = (1 + noise) - c^2 ((1 + noise) - s2_0)
        held at the parity bar (c = .75 keeps s2 in (.48, 1.1): no clamp, no cancellation).  The sweep under the other variance comes
        straight after one under the model's own, so it finds a kept state formed for ANOTHER k* (st_sf2): that state must not be
        continued -- the kernel is a full one -- and the arg-max is the fresh model's under the same variance."""
        GP, lib, c = self.GP, self.lib, KSTAR_SCALE
        sf2 = GP.kernel._ibo_spec()[2]
        self.sweep()
        fr = self.fresh()
        m0, v0 = fr.posteriors(self.Q)
        assert np.all((v0 > 1e-7) & (v0 < 10.0))          # the clamp of `posteriors` is not active: s2_0 is the raw variance
        p = self.priors[self.pk]
        m = np.zeros(len(self.Q)) if p is None else np.array([p.mu(q) for q in self.Q])
        lib.check(lib.lib.ibo_gp_set_kstar_sf2(GP._handle(), c * sf2))
        try:
            lib.check(lib.lib.ibo_gp_set_kstar_sf2(fr._handle(), c * sf2))
            m1, v1 = GP.posteriors(self.Q)
            values_close(m1, m + c * (m0 - m), "mu under %g sf2" % c)
            values_close(v1, (1 + NOISE) - c * c * ((1 + NOISE) - v0), "s2 under %g sf2" % c)
            kernel = self.sweep(fr)
            assert "rank1" not in kernel and "finish" not in kernel, kernel
        finally:
            lib.check(lib.lib.ibo_gp_set_kstar_sf2(GP._handle(), sf2))

    # ------------------------------------------------------------------------------------------------ checks
    def check_step(self, what):
        GP = self.GP
        assert np.array_equal(GP.X, self.X) and np.array_equal(GP.Y, self.Y), what
        fr = self.fresh()
        (m1, v1), (m0, v0) = GP.posteriors(self.Q), fr.posteriors(self.Q)
        values_close(m1, m0, what + " mu"); values_close(v1, v0, what + " s2")
        return fr, (m1, v1)

    def check_all(self, fr, what):
        check_factor(self.lib, self.GP, self.kind, self.D, what, cond="bound")
        check_readers_like_fresh(self.GP, fr, self.kind, self.D, what)


def run_sequence(lib, kind, D, N0, reserve, prior, seed, checks=True):
    d = Driver(lib, kind, D, N0, reserve, prior, seed)
    ops = schedule(d.rs)
    done = []
    post = None
    for k, op in enumerate(ops, 1):
        done.append(d.step(op))
        what = "%s D=%d step %d (%s, N=%d)" % (kind, D, k, done[-1], len(d.X))
        if checks:
            fr, post = d.check_step(what)
            if k % 10 == 0 or k == len(ops):
                d.check_all(fr, what)
    if not checks:
        post = d.GP.posteriors(d.Q)
    return d, done, (d.GP.L.copy(), get_W(lib, d.GP), post)


SEQUENCES = {"ard-d4-n60": ("ard", 4, 60, 8, False, 101, 64), "m5-d8-n126-prior": ("m5", 8, 126, 0, True, 102, 128),
             "svard-d33-n70": ("svard", 33, 70, 0, False, 103, None)}


@pytest.mark.parametrize("name", sorted(SEQUENCES))
def test_mixed_sequence_agrees_with_a_fresh_model_after_every_step(lib, name):
    """40 steps, every operation of OPS at least twice in a seeded order (schedule): SE-ARD D = 4 from 60 rows with 8 reserved (the row count
    crosses 64 in both directions), Matern-5/2 D = 8 with a mean prior from 126 rows (crosses 128: the padding fills up and is given back),
    SV-ARD D = 33 from 70 rows (no dot form and no kept state: its sweep operation is a full sweep)."""
    kind, D, N0, reserve, prior, seed, edge = SEQUENCES[name]
    with wall("sequence " + name):
        d, done, _ = run_sequence(lib, kind, D, N0, reserve, prior, seed)
        sizes = np.array(d.sizes)
        print("%s: %s" % (name, " ".join("%s:%d" % (o, n) for o, n in zip(done, sizes[1:]))))
        print("%s: rows %d .. %d, %d refits, sweeps on %s" % (name, sizes.min(), sizes.max(), d.refits, sorted(set(d.kernels))))
        assert sizes.max() * (1 + NOISE) / NOISE < 1e6 and d.GP.kernel._ibo_spec()[2] <= 1.0        # cond_2(R) < 1e6 at every step
        # (step() turns an addk / add_refit into rm_refit once the model has grown by 20 rows: with these seeds each still runs)
        assert set(done) >= set(OPS), sorted(set(OPS) - set(done))
        if name == "m5-d8-n126-prior":                    # the padding, not EXTEND_MAX, forced a refit: 128 rows were full
            assert d.pad_refits >= 1 and np.any(np.diff(-(-sizes // 64)) > 0), (d.pad_refits, list(sizes))
        if edge is not None:
            up = np.sum((sizes[:-1] <= edge) & (sizes[1:] > edge)); down = np.sum((sizes[:-1] > edge) & (sizes[1:] <= edge))
            assert up >= 1 and down >= 1, (name, edge, list(sizes))
        if kind != "svard":
            assert any("rank1" in k or "finish" in k for k in d.kernels), d.kernels        # the kept state was really used, not only formed


def test_mixed_sequence_gives_the_same_bits_on_two_handles(lib):
    kind, D, N0, reserve, prior, seed, _ = SEQUENCES["ard-d4-n60"]
    with wall("the first sequence twice"):
        a = run_sequence(lib, kind, D, N0, reserve, prior, seed, checks=False)
        b = run_sequence(lib, kind, D, N0, reserve, prior, seed, checks=False)
        assert a[1] == b[1]
        assert np.array_equal(a[2][0], b[2][0]) and np.array_equal(a[2][1], b[2][1])
        assert np.array_equal(a[2][2][0], b[2][2][0]) and np.array_equal(a[2][2][1], b[2][2][1])


LENGTH_STEPS = (1, 10, 100, 300)


@pytest.mark.parametrize("noise", [.1, 1e-4])
@pytest.mark.parametrize("mode", ["window", "random"])
def test_three_hundred_window_steps_stay_flat(lib, mode, noise):
    """300 steps "append one point, remove row 0" (window) and "append one, remove a random row" (random) at N = 100, D = 4, SE-ARD l = .45,
    4 reserved rows, at noise .1 (cond_2 ~ 300) and 1e-4 (cond_2 ~ 2e5; <= 1e6 asserted by SVD at every checkpoint).  At steps 1, 10, 100 and
    300: L, W, R against NumPy at 1e-9; at step 300 each of the two errors at most 8 max(the restatement's worst checkpoint error of that
    matrix on the same sequence, 1e-13).
    Measured on an MI355X (device error at steps 1, 10, 100, 300; the restatement's worst checkpoint error in brackets):
        window  noise .1     L 1.7e-15 1.6e-15 4.7e-15 8.5e-15 [6.6e-15]   W 5.0e-15 4.3e-15 1.2e-14 2.0e-14 [1.5e-14]
        window  noise 1e-4   L 4.0e-14 4.6e-14 2.8e-13 1.7e-13 [3.0e-13]   W 5.1e-13 1.2e-12 2.7e-12 2.9e-12 [5.9e-12]
        random  noise .1     L 1.7e-15 1.5e-15 2.5e-15 2.7e-15 [3.3e-15]   W 3.8e-15 3.9e-15 4.8e-15 5.8e-15 [8.0e-15]
        random  noise 1e-4   L 3.8e-14 8.7e-14 1.1e-13 6.7e-14 [1.0e-13]   W 3.2e-13 7.7e-13 1.5e-12 5.3e-13 [1.1e-12]
    The brackets are computed by the host that runs the test and move with its BLAS at noise 1e-4 (another NumPy build gave L 2.3e-13,
    W 2.9e-12 for window and L 1.5e-13, W 1.9e-12 for random; the noise .1 figures came out the same), and the 8x bar moves with them:
    it is a margin over the restatement as computed next to the device run, not over a recorded number.
    The device follows the restatement's level, which moves with cond_2 of the window, not with the step count."""
    from ibo_amd.gaussianprocess import GaussianProcess
    from ibo_amd.gaussianprocess.kernel import GaussianKernel_ard
    N, D, ell = 100, 4, .45
    with wall("300 %s steps at noise %g" % (mode, noise)):
        X0, plan = dr.window_plan(43, N, D, LENGTH_STEPS[-1], mode)
        ref, Xend = dr.run_window(X0, plan, ell, noise, LENGTH_STEPS)
        worst_L, worst_W = max(v[1] for v in ref.values()), max(v[2] for v in ref.values())
        f = lambda X: np.sin(3 * np.atleast_2d(X).sum(1))
        okern = orc.Kern("ard", [ell] * D)
        GP = GaussianProcess(GaussianKernel_ard([ell] * D), X0, f(X0), noise=noise, reserve_rows=4)
        GP._fit_device = lambda *a, **k: pytest.fail("a window step refitted")
        got = {}
        try:
            for step, (x, row) in enumerate(plan, 1):
                GP.addData(x, f(x)[0])
                GP.removeData(row)
                if step in LENGTH_STEPS:
                    what = "%s noise %g step %d" % (mode, noise, step)
                    got[step] = check_factor(lib, GP, "ard", D, what, R=orc.GP(okern, GP.X, GP.Y, noise=noise).R)
        finally:
            del GP._fit_device
        assert np.array_equal(GP.X, Xend)
        print("%s noise %g: device L %s  W %s  (restatement's worst: L %.2g, W %.2g)" % (
            mode, noise, " ".join("%.2g" % got[s][0] for s in LENGTH_STEPS), " ".join("%.2g" % got[s][1] for s in LENGTH_STEPS), worst_L, worst_W))
        eL, eW = got[LENGTH_STEPS[-1]]
        assert eL <= 8 * max(worst_L, 1e-13), (mode, noise, eL, worst_L)
        assert eW <= 8 * max(worst_W, 1e-13), (mode, noise, eW, worst_W)

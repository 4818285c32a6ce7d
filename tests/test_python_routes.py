"""Which library entry the Python layer reaches for each kind of model -- plain (ibo_gp_t), observed with gradients (ibo_ggp_t), sparse
(ibo_sgp_t) -- and with which scalar arguments, without a device: a recording stand-in takes the place of _lib.lib.  It answers IBO_OK
to everything that creates, fits or sets something; an evaluating entry records its call and raises a marker, so every route is
followed up to the entry and (for the plain kind's k* signal variance) through what it does when the entry raises.

The expected names and arguments are those of the routes before they were merged into one (one copy per kind then)."""
import gc

import numpy as np
import pytest

from ibo_amd import _lib
from ibo_amd.acquisition import EI, maximizeEI, sweep
from ibo_amd.gaussianprocess import GaussianProcess, SparseGaussianProcess
from ibo_amd.gaussianprocess.kernel import SVGaussianKernel_ard

KINDS = ("gp", "ggp", "sgp")
PREFIX = {"gp": "ibo_", "ggp": "ibo_ggp_", "sgp": "ibo_sgp_"}
DIRECT = {"gp": "ibo_direct_max", "ggp": "ibo_ggp_direct_max", "sgp": "ibo_sgp_direct_max"}
EVALUATING = set(p + n for p in PREFIX.values() for n in ("acq_batch", "acq_sweep")) | set(DIRECT.values()) | {
    "ibo_posterior_batch", "ibo_acq_sweep_incremental", "ibo_acq_sweep_exchange", "ibo_acq_grad_batch"}
P = "*"                      # a pointer argument that is not null

GRADIENT_WHY = ("the model is observed with gradients (G=): it has N (D + 1) rows of values and derivatives, and only posterior, "
                "posteriors, mu, negmu, R, L, nlml, learn, EI / PI / UCB, acquisition.sweep and maximizeEI / PI / UCB are built for it")
SPARSE_WHY = ("the model is a sparse GP on inducing points: only posterior, posteriors, mu, negmu, nlml, nlml_gradient, learn, addData, "
              "EI / PI / UCB (.f, .negf, .values), acquisition.sweep and maximizeEI / PI / UCB are built for it")


class Reached(Exception):
    pass


def shown(a):
    if a is None:
        return None
    if isinstance(a, float) and a != a:
        return "nan"
    return a if isinstance(a, (int, float, bytes)) else P


class StandIn(object):
    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def entry(*args):
            self.calls.append((name, tuple(shown(a) for a in args)))
            if name in EVALUATING:
                raise Reached(name)
            if name.endswith("_create") or name == "ibo_dev_alloc":
                args[-1]._obj.value = 0x1000 * len(self.calls)        # (a handle that is not null)
            return b"" if name == "ibo_last_error" else _lib.OK
        return entry

    def only(self):
        """the one evaluating call since the last clear()"""
        hit = [c for c in self.calls if c[0] in EVALUATING]
        assert len(hit) == 1, self.calls
        return hit[0]

    def kstar(self):
        """(position, value) of the ibo_gp_set_kstar_sf2 calls, and the position of the evaluating call"""
        at = [i for i, c in enumerate(self.calls) if c[0] in EVALUATING]
        return [(i, c[1][1]) for i, c in enumerate(self.calls) if c[0] == "ibo_gp_set_kstar_sf2"], at


@pytest.fixture
def routes(monkeypatch):
    """(the stand-in, build(kind) -> a fitted model of that kind); the real library is back afterwards and never sees a handle made here"""
    lib = StandIn()
    monkeypatch.setattr(_lib, "lib", lib)
    made = []

    def build(kind):
        rs = np.random.RandomState(3)
        X = rs.rand(6, 2)
        Y = np.sin(3 * X.sum(1))
        kernel = SVGaussianKernel_ard([.3, .4, 2.])
        if kind == "sgp":
            GP = SparseGaussianProcess(kernel, X, Y, m=4, noise=.05, seed=1)
        else:
            GP = GaussianProcess(kernel, X, Y, noise=.05, G=rs.randn(6, 2) if kind == "ggp" else None)
        made.append(GP)
        del lib.calls[:]
        return GP

    yield lib, build
    for GP in made:
        for dev in (getattr(GP, "_dev", None), getattr(GP, "_gdev", None), getattr(GP, "_augdev", None)):
            if dev is not None:
                dev.h = None
    del made[:]
    gc.collect()                                     # (DeviceArray temporaries of a raised route free themselves into the stand-in)


@pytest.mark.parametrize("kind", KINDS)
def test_host_batch_reaches_the_entry_of_the_kind(routes, kind):
    lib, build = routes
    GP = build(kind)
    x = np.array([.2, .7])
    batch = PREFIX[kind] + "acq_batch"

    with pytest.raises(Reached):
        GP.posterior(x)
    if kind == "gp":                                 # the plain model's posterior has an entry of its own
        assert lib.only() == ("ibo_posterior_batch", (P, 1, P, _lib.CLAMP_PY, P, P))
    else:
        assert lib.only() == (batch, (P, 1, P, _lib.ACQ_NONE, 0.0, _lib.ERF_NR, _lib.CLAMP_PY, "nan", P, P, None))

    del lib.calls[:]
    with pytest.raises(Reached):
        GP._eval(np.ones((3, 2)) * .5)
    assert lib.only() == (batch, (P, 3, P, _lib.ACQ_NONE, 0.0, _lib.ERF_NR, _lib.CLAMP_PY, "nan", P, P, None))

    del lib.calls[:]
    with pytest.raises(Reached):
        GP._eval(x, _lib.ACQ_UCB, 1.5, _lib.ERF_LIBM, _lib.CLAMP_NATIVE, ("acq",), ymax=.25)
    assert lib.only() == (batch, (P, 1, P, _lib.ACQ_UCB, 1.5, _lib.ERF_LIBM, _lib.CLAMP_NATIVE, .25, None, None, P))

    del lib.calls[:]
    with pytest.raises(Reached):
        EI(GP, xi=.02).negf(x)
    assert lib.only() == (batch, (P, 1, P, _lib.ACQ_EI, .02, _lib.ERF_NR, _lib.CLAMP_PY, float(np.max(GP.Y)), None, None, P))
    assert lib.kstar()[0] == []                      # the Python classes keep the kernel's own k* variance


@pytest.mark.parametrize("native", (True, False))
@pytest.mark.parametrize("kind", KINDS)
def test_sweep_reaches_the_entry_of_the_kind(routes, kind, native):
    lib, build = routes
    GP = build(kind)
    C = np.random.RandomState(4).rand(5, 2)
    modes = (_lib.ERF_LIBM, _lib.CLAMP_NATIVE) if native else (_lib.ERF_NR, _lib.CLAMP_PY)
    no_balls = () if kind == "ggp" else (0, None, 0.5)               # (ibo_ggp_acq_sweep has no exclusion arguments)

    with pytest.raises(Reached):
        sweep(GP, C, acq='ei', native=native)
    assert lib.only() == (PREFIX[kind] + "acq_sweep", (P, 5, P, _lib.ACQ_EI, 0.01) + modes + ("nan",) + no_balls + (0, None, None, None, P, P))

    del lib.calls[:]
    balls = () if kind == "ggp" else (2, P, .25)
    with pytest.raises(Reached):
        sweep(GP, C, acq='pi', xi=.03, native=native, ymax=.5, index_base=7, outputs=('mu', 'acq'), exclude_radius=.25,
              exclude=None if kind == "ggp" else C[:2])
    assert lib.only() == (PREFIX[kind] + "acq_sweep", (P, 5, P, _lib.ACQ_PI, 0.03) + modes + (.5,) + balls + (7, P, None, P, P, P))


@pytest.mark.parametrize("kind", KINDS)
def test_direct_reaches_the_entry_of_the_kind(routes, kind):
    lib, build = routes
    GP = build(kind)
    with pytest.raises(Reached):
        maximizeEI(GP, [[0., 1.]] * 2, useCDIRECT=True)
    assert lib.only() == (DIRECT[kind], (P, 2, P, P, _lib.ACQ_EI, 0.01, _lib.ERF_LIBM, _lib.CLAMP_NATIVE, 50, 30, 10000, 1, P, P, P))
    del lib.calls[:]
    with pytest.raises(Reached):
        maximizeEI(GP, [[0., 1.]] * 2, xi=.05, maxiter=8, maxtime=3, maxsample=200)
    assert lib.only() == (DIRECT[kind], (P, 2, P, P, _lib.ACQ_EI, 0.05, _lib.ERF_LIBM, _lib.CLAMP_NATIVE, 8, 3, 200, 1, P, P, P))


def test_plain_kind_switches_the_kstar_variance_around_the_entry(routes):
    """libego's value before the entry, the kernel's own after it -- also though the entry raised (it always does here)"""
    lib, build = routes
    GP = build("gp")
    _, _, sf2_py, sf2_native = GP.kernel._ibo_spec()
    assert sf2_py != sf2_native
    C = np.random.RandomState(4).rand(5, 2)
    for call in (lambda: sweep(GP, C, native=True), lambda: maximizeEI(GP, [[0., 1.]] * 2), lambda: sweep(GP, _lib.DeviceArray.from_host(C))):
        del lib.calls[:]
        with pytest.raises(Reached):
            call()
        (first, v0), (last, v1) = lib.kstar()[0]
        assert (v0, v1) == (sf2_native, sf2_py)
        assert [first < at < last for at in lib.kstar()[1]] == [True]
    del lib.calls[:]
    with pytest.raises(Reached):
        sweep(GP, C, native=False)
    assert lib.kstar()[0] == []


@pytest.mark.parametrize("kind", ("ggp", "sgp"))
def test_other_kinds_never_touch_the_kstar_variance(routes, kind):
    lib, build = routes
    GP = build(kind)
    for call in (lambda: sweep(GP, np.ones((3, 2)) * .5, native=True), lambda: maximizeEI(GP, [[0., 1.]] * 2)):
        with pytest.raises(Reached):
            call()
    assert lib.kstar()[0] == []


def test_refusals_of_the_sweep_keep_their_order_and_text(routes):
    lib, build = routes
    C = np.ones((3, 2)) * .5
    exchange = object()
    GP = build("ggp")
    for kw, what in ((dict(exclude=C[:1], incremental=True, exchange=exchange), "sweep(exclude=)"),
                     (dict(incremental=True, exchange=exchange), "sweep(incremental=)"),
                     (dict(exchange=exchange), "sweep(exchange=)")):
        with pytest.raises(NotImplementedError) as e:
            sweep(GP, C, **kw)
        assert str(e.value) == "%s: not available, %s" % (what, GRADIENT_WHY)
    GP = build("sgp")
    for kw, what in ((dict(exclude=C[:1], incremental=True, exchange=exchange), "sweep(incremental=)"),
                     (dict(exclude=C[:1], exchange=exchange), "sweep(exchange=)")):
        with pytest.raises(NotImplementedError) as e:
            sweep(GP, C, **kw)
        assert str(e.value) == "%s: not available, %s" % (what, SPARSE_WHY)
    assert [c for c in lib.calls if c[0] in EVALUATING] == []
    for kind, why in (("ggp", GRADIENT_WHY), ("sgp", SPARSE_WHY)):
        GP = build(kind)
        with pytest.raises(NotImplementedError) as e:
            maximizeEI(GP, [[0., 1.]] * 2, polish=True)
        assert str(e.value) == "maximizeEI(polish=True): not available, %s" % why
        with pytest.raises(NotImplementedError) as e:
            GP._handle()
        assert str(e.value) == "this call (it takes the model's ibo_gp_t handle): not available, %s" % why
        with pytest.raises(NotImplementedError) as e:
            EI(GP).gradient(C)
        assert str(e.value) == "gradient / negf_grad of an acquisition: not available, %s" % why
    assert [c for c in lib.calls if c[0] in EVALUATING] == []

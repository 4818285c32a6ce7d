#!/usr/bin/env python3
"""What the Python layer does with the library, one line per scenario: which entries it calls, in which order and with which scalar
arguments, and a SHA-256 over the raw bytes of everything it returns.  Through the public API only, so the same file runs on any
revision of the package and two revisions compare line for line (with the same build of the library, IBO_HIP_LIB=/path/to/libibo_hip.so):

    python3 tools/python_routes_bits.py                 every scenario
    python3 tools/python_routes_bits.py gp ggp48        the scenarios whose name starts with one of these

A line reads  <scenario> | <entries, runs of one entry folded as name*k> | calls <digest of the full call log> | out <digest>.
The call log holds every entry's name with its int / float / bytes arguments; a pointer argument is logged as '*', or 'None' when null.

Models: a plain GP (N = 40, D = 3) without and with an RBF mean prior, a model observed with gradients of 48 rows (N = 12, D = 3) and one
of 66 rows (N = 22, D = 2: across the 64-row pad), a sparse model (N = 200, m = 16, D = 3) fitted as 'fitc' and as 'dtc'.  Each is
evaluated at M = 300 candidates (across the 256-candidate chunk edge), as an ndarray and as a DeviceArray."""
import hashlib
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ibo_amd import _lib                                                                   # noqa: E402
from ibo_amd.gaussianprocess import GaussianProcess, SparseGaussianProcess                 # noqa: E402
from ibo_amd.gaussianprocess.kernel import GaussianKernel_ard                              # noqa: E402
from ibo_amd.gaussianprocess.prior import RBFNMeanPrior                                    # noqa: E402
from ibo_amd.gaussianprocess import trainhyper                                             # noqa: E402
from ibo_amd.acquisition import EI, PI, UCB, sweep, maximizeEI, maximizePI, maximizeUCB    # noqa: E402

M, NOISE = 300, .05
ELL = {2: [.4, .5], 3: [.35, .45, .55]}


class Recorder(object):
    """stands where _lib.lib stood: every entry asked of it is the library's own, logged when called"""

    def __init__(self, real):
        self.__dict__["real"], self.__dict__["log"] = real, []

    def __getattr__(self, name):
        fn = getattr(self.real, name)

        def logged(*args):
            self.log.append("%s(%s)" % (name, ", ".join(repr(a) if isinstance(a, (int, float, bytes)) else ("None" if a is None else "*")
                                                         for a in args)))
            return fn(*args)
        return logged


def digest(obj, h):
    if isinstance(obj, dict):
        for k in sorted(obj):
            if k != "kernel_ms":                     # (a time)
                h.update(str(k).encode())
                digest(obj[k], h)
    elif isinstance(obj, (tuple, list)):
        for o in obj:
            digest(o, h)
    elif isinstance(obj, (str, bytes)):
        h.update(obj.encode() if isinstance(obj, str) else obj)
    elif obj is None:
        h.update(b"None")
    else:
        h.update(np.ascontiguousarray(np.asarray(obj, dtype=np.float64)).tobytes())


def folded(log):
    names, out = [c.split("(", 1)[0] for c in log], []
    for n in names:
        if out and out[-1][0] == n:
            out[-1][1] += 1
        else:
            out.append([n, 1])
    return " ".join(n if k == 1 else "%s*%d" % (n, k) for n, k in out)


def data(N, D, seed):
    rs = np.random.RandomState(seed)
    X = rs.rand(N, D)
    s = 3 * X.sum(1)
    return X, np.sin(s) + .01 * rs.randn(N), 3 * np.cos(s)[:, None] * np.ones((1, D)) + .01 * rs.randn(N, D)


def prior():
    rs = np.random.RandomState(5)
    return RBFNMeanPrior(means=[c for c in rs.rand(4, 3)], beta=rs.randn(4) * .3, theta=10., lowerb=np.zeros(3), width=np.ones(3))


def model(name):
    if name in ("gp", "gp+prior"):
        X, Y, _ = data(40, 3, 40)
        return GaussianProcess(GaussianKernel_ard(ELL[3]), X, Y, noise=NOISE, prior=prior() if name == "gp+prior" else None)
    if name in ("ggp48", "ggp66"):
        N, D = (12, 3) if name == "ggp48" else (22, 2)
        X, Y, G = data(N, D, N)
        return GaussianProcess(GaussianKernel_ard(ELL[D]), X, Y, noise=NOISE, gnoise=1e-3, G=G)
    X, Y, _ = data(200, 3, 200)
    return SparseGaussianProcess(GaussianKernel_ard(ELL[3]), X, Y, m=16, noise=NOISE, method=name[4:], seed=3)


def result_fields(res):
    """(.evaluations is hashed where every revision has it: the gradient model's learner)"""
    return [res.x, res.fun, res.start_value, res.end_value, res.applied]


def model_scenarios(name):
    """(scenario, thunk) for one model; the thunks run in this order on ONE model (the learners, which change it, come last)"""
    D = 2 if name == "ggp66" else 3
    box = [[0., 1.]] * D
    C = _lib.f64(np.random.RandomState(M + D).rand(M, D))
    state = {}

    def GP():
        if "m" not in state:
            state["m"] = model(name)
        return state["m"]

    yield "fit", lambda: (GP().X.shape, GP().Y)
    yield "posteriors", lambda: GP().posteriors(C)
    yield "posterior", lambda: (GP().posterior(C[0]), GP().posterior(C[1], getvar=False), GP().mu(C[2]))
    for label, cand in (("ndarray", lambda: C), ("DeviceArray", lambda: _lib.DeviceArray.from_host(C))):
        for native in (True, False):
            for acq in ("ei", "pi", "ucb"):
                yield ("sweep %s native=%d %s" % (label, native, acq),
                       lambda cand=cand, native=native, acq=acq: sweep(GP(), cand(), acq=acq, native=native, outputs=('mu', 's2', 'acq')))
            if not name.startswith("ggp"):
                yield ("sweep %s native=%d ei exclude" % (label, native),
                       lambda cand=cand, native=native: sweep(GP(), cand(), acq='ei', native=native, outputs=('mu', 's2', 'acq'),
                                                              exclude=C[[0, 150]], exclude_radius=.15, index_base=1000003))
    yield "negf", lambda: (EI(GP()).negf(C[3]), PI(GP()).negf(C[3]), UCB(GP(), D).negf(C[3]), EI(GP(), xi=.05).f(C[4]))
    yield "EI.values", lambda: EI(GP()).values(C)
    yield "maximizeEI", lambda: maximizeEI(GP(), box, maxiter=8)
    yield "maximizePI", lambda: maximizePI(GP(), box, maxiter=8)
    yield "maximizeUCB", lambda: maximizeUCB(GP(), box, maxiter=8)
    if name == "gp":
        yield "maximizeEI polish", lambda: maximizeEI(GP(), box, maxiter=8, polish=True)
    if name.startswith("ggp"):
        yield "nlml", lambda: GP().nlml()

        def learn():
            res = GP().learn(noise=True, gnoise=True, maxiter=3)
            return result_fields(res), res.evaluations, GP().kernel.hyperparams, GP().noise, GP().gnoise, GP().posteriors(C[:5])
        yield "learn", learn
    if name.startswith("sgp"):
        yield "nlml", lambda: (GP().nlml(), GP().nlml_gradient())
        yield "learn", lambda: (result_fields(GP().learn(maxiter=3)), GP().kernel.hyperparams, GP().noise, GP().Z, GP().posteriors(C[:5]))


def likelihood_scenarios():
    X, Y, _ = data(40, 3, 40)
    Xg, Yg, Gg = data(12, 3, 12)
    Xs, Ys, _ = data(200, 3, 200)
    Z = Xs[::13][:16].copy()
    K, k = GaussianKernel_ard, GaussianKernel_ard(ELL[3])
    lh = np.log(ELL[3])
    yield "marginalLikelihood", lambda: (trainhyper.marginalLikelihood(k, X, Y, 3, noise=NOISE),
                                         trainhyper.marginalLikelihood(k, X, Y, 3, computeGradient=False, noise=NOISE))
    yield "looLikelihood", lambda: (trainhyper.looLikelihood(k, X, Y, 3, noise=NOISE, predictions=True),
                                    trainhyper.looLikelihood(k, X, Y, 3, computeGradient=False, noise=NOISE))
    yield "gradientLikelihood", lambda: (trainhyper.gradientLikelihood(k, Xg, Yg, Gg, 3, noise=NOISE, gnoise=1e-3, gradNoise=True),
                                         trainhyper.gradientLikelihood(k, Xg, Yg, Gg, 2, noise=NOISE, gnoise=[1e-3, 2e-3, 3e-3]),
                                         trainhyper.gradientLikelihood(k, Xg, Yg, Gg, 0, noise=NOISE, computeGradient=False))
    yield "sparseLikelihood", lambda: [trainhyper.sparseLikelihood(k, Xs, Ys, Z, 3, NOISE, kind=kind, gradZ=gz)
                                       for kind, gz in (("vfe", True), ("fitc", True), ("dtc", False))] + [
                                           trainhyper.sparseLikelihood(k, Xs, Ys, Z, 3, NOISE, computeGradient=False)]
    yield "nlml dnlml twice", lambda: (trainhyper.nlml(lh, K, X, Y), trainhyper.dnlml(lh, K, X, Y), trainhyper.nlml(lh, K, X, Y),
                                       trainhyper.dnlml(lh + .1, K, X, Y), trainhyper.nlml(lh + .1, K, X, Y))
    yield "nloo dnloo twice", lambda: (trainhyper.nloo(lh, K, X, Y, NOISE), trainhyper.dnloo(lh, K, X, Y, NOISE),
                                       trainhyper.nloo(lh, K, X, Y, 2 * NOISE))
    yield "ngnlml dgnlml twice", lambda: (trainhyper.ngnlml(lh, K, Xg, Yg, Gg, NOISE, 1e-3), trainhyper.dgnlml(lh, K, Xg, Yg, Gg, NOISE, 1e-3),
                                          trainhyper.dgnlml(lh, K, Xg, Yg, Gg, NOISE, 2e-3))


def main():
    if _lib.device_count() < 1:
        raise SystemExit("no GPU: nothing to hash")
    want = sys.argv[1:]
    rec = Recorder(_lib.lib)
    _lib.lib = rec
    groups = [(name, model_scenarios(name)) for name in ("gp", "gp+prior", "ggp48", "ggp66", "sgp-fitc", "sgp-dtc")]
    groups.append(("likelihood", likelihood_scenarios()))
    for group, scenarios in groups:
        if want and not any(group.startswith(w) for w in want):
            continue
        for scenario, thunk in scenarios:
            del rec.log[:]
            h = hashlib.sha256()
            digest(thunk(), h)
            calls = hashlib.sha256("\n".join(rec.log).encode()).hexdigest()[:16]
            print("%s: %s | %s | calls %s | out %s" % (group, scenario, folded(rec.log), calls, h.hexdigest()), flush=True)
            if os.environ.get("ROUTES_BITS_CALLS"):                   # the full call log, for reading a difference
                print("    " + "\n    ".join(rec.log), flush=True)


if __name__ == "__main__":
    main()

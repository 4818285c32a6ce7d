"""What knowledge.py and batch.py check alike about their arguments: points, candidate arrays, bounds."""
import numpy as np

from .. import _lib


def _no_gradient(GP, what):
    """refuse `what` on a model observed with gradients (GaussianProcess(G=)) and on a sparse model (SparseGaussianProcess); anything
    without a G attribute passes"""
    if getattr(GP, "G", None) is not None or getattr(GP, "_sparse", False):
        GP._no_gradient(what)


def _points(GP, P, what, noun):
    """an (M, D) float64 matrix of points of the model's dimension; a 1-D sequence is ONE point (D coordinates), as everywhere else.
    noun: what the refusal of an augmented factor calls the acquisition"""
    if len(GP.X) == 0:
        raise ValueError("model has no data")
    _no_gradient(GP, "the %s" % noun)
    if getattr(GP, "_augdev", None) is not None:
        raise ValueError("the %s is not defined on an augmented factor (addObservationPoint): its covariances would "
                         "come from one factor and its means from another" % noun)
    P = _lib.f64(np.atleast_2d(np.asarray(P, dtype=float)))
    D = np.asarray(GP.X).shape[1]
    if P.ndim != 2 or P.shape[1] != D or len(P) < 1:
        raise ValueError("%s must be (M, %d) points, got shape %s" % (what, D, P.shape))
    return P


def _candidates(GP, candidates, D, noun):
    """(the candidates in HBM, the host's copy or None): an ndarray is checked as _points and uploaded, a _lib.DeviceArray is taken as
    it is; either must be D wide"""
    host = None if isinstance(candidates, _lib.DeviceArray) else _points(GP, candidates, "candidates", noun)
    cand = candidates if host is None else _lib.DeviceArray.from_host(host, GP._dev.device)
    if len(cand.shape) != 2 or cand.shape[1] != D:
        raise ValueError("candidates must be (M, %d) points, got shape %s" % (D, cand.shape))
    return cand, host


def _bounds(bounds, D_model):
    """(lb, ub, D) of a box of the model's dimension"""
    lb = _lib.f64([b[0] for b in bounds]); ub = _lib.f64([b[1] for b in bounds])
    if len(lb) != D_model:
        raise ValueError("bounds have %d dimensions, the model has %d" % (len(lb), D_model))
    return lb, ub, len(lb)

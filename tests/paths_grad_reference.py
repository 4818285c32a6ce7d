"""
The gradients of the pathwise posterior draws (ibo_paths_grad_batch) restated in NumPy, for tests/test_gpu_paths_grad.py; pinned by
tests/test_paths_grad_reference.py to central differences of tests/paths_reference.py's values and to itself in long double.

Notation of paths_reference.py and grad_reference.py: amp = sqrt(2 sf2 / F), t_j = omega_j.x + b_j, z_i = sum_d w_d (x_d - X_id)^2,
coefficients [w_s ; c_s], m the mean prior and s1 = k*.a1.
    d phi_j / dx_d   = -amp sin(t_j) omega_jd
    d k(x, X_i)/dx_d = h_i w_d (x_d - X_id)           h_i: -k, -3 sf2 e^-r, -(5/3) sf2 (1 + r) e^-r  (grad_reference.kstar)
    g_sd             = sum_j d_d phi_j w_sj + sum_i d_d k_i c_si                 gs1_d = sum_i d_d k_i a1_i
    d_d path_s       = g_sd   without a prior,   d_d m (1 - s1) + g_sd - m gs1_d   with one
The sine's argument is formed in long double and reduced by 2 pi there, as paths_reference.features does.  Every function takes
dtype: np.float64 (the yardstick) or np.longdouble (everything after the inputs in extended precision: what the yardstick's own
rounding is measured against).  T_grad (grad_scale) = |d_d m| (1 + |s1|) + sum_j |d_d phi_j w_sj| + sum_i |d_d k_i| (|c_si| + |m a1_i|)
is the yardstick of the tests' bars.
"""
import numpy as np

import grad_reference as gr
import paths_reference as pr

LD = pr.LD


def dfeatures(omega, phase, sf2, Q, dtype=np.float64):
    """d Phi (M, F, D) at the rows of Q"""
    Q = np.atleast_2d(np.asarray(Q, dtype=float)); omega = np.atleast_2d(np.asarray(omega, dtype=float))
    t = np.zeros((len(Q), len(omega)), dtype=LD) + np.asarray(phase, dtype=LD)[None, :]
    for d in range(Q.shape[1]):
        t += Q[:, d, None].astype(LD) * omega[None, :, d].astype(LD)
    t -= pr.TWO_PI_LD * np.rint(t / pr.TWO_PI_LD)
    amp = np.sqrt(dtype(2.0) * dtype(sf2) / dtype(len(omega)))
    return (-amp * np.sin(t.astype(dtype)))[:, :, None] * omega.astype(dtype)[None, :, :]


def dkstar(ref, Q, dtype=np.float64):
    """(k* (M, N), d k* (M, N, D)) at the rows of Q"""
    Q = np.atleast_2d(np.asarray(Q, dtype=float)).astype(dtype)
    w, sf2 = ref.w.astype(dtype), dtype(ref.sf2)
    diff = Q[:, None, :] - ref.X.astype(dtype)[None, :, :]
    z = np.sum(w * diff ** 2, axis=2)
    if ref.fam == gr.FAM_SE:
        k = sf2 * np.exp(-z / 2)
        h = -k
    elif ref.fam == gr.FAM_M3:
        r = np.sqrt(3 * z); e = np.exp(-r)
        k, h = sf2 * (1 + r) * e, -3 * sf2 * e
    else:
        r = np.sqrt(5 * z); e = np.exp(-r)
        k, h = sf2 * (1 + r + r * r / 3) * e, -(dtype(5) / 3) * sf2 * (1 + r) * e
    return k, h[:, :, None] * w * diff


def prior(ref, Q, dtype=np.float64):
    """(m (M,), dm (M, D)) of the RBF-network prior (grad_reference.prior_grad's), zeros without one"""
    Q = np.atleast_2d(np.asarray(Q, dtype=float)).astype(dtype)
    if ref.prior is None:
        return np.zeros(len(Q), dtype=dtype), np.zeros(Q.shape, dtype=dtype)
    means, beta, theta, lo, wd = [np.asarray(a, dtype=float).astype(dtype) for a in ref.prior]
    diff = (Q - lo)[:, None, :] / wd - np.atleast_2d(means)[None, :, :]                    # M x nb x D
    be = beta * np.exp(-theta * np.sum(diff ** 2, axis=2))
    return be.sum(axis=1), np.einsum("mb,mbd->md", be, diff) * (-2 * theta) / wd


def _parts(ref, omega, phase, coefs, Q, dtype):
    F = len(np.atleast_2d(omega))
    coefs = np.atleast_2d(coefs).astype(dtype)
    dPhi = dfeatures(omega, phase, ref.sf2, Q, dtype)
    Ks, dK = dkstar(ref, Q, dtype)
    m, dm = prior(ref, Q, dtype)
    return dPhi, Ks, dK, coefs[:, :F], coefs[:, F:], m, dm, ref.a1.astype(dtype)


def grads(ref, omega, phase, coefs, Q, dtype=np.float64):
    """(S, M, D): the gradients of the paths with coefficients `coefs` (S, F + N) at the rows of Q"""
    dPhi, Ks, dK, w, c, m, dm, a1 = _parts(ref, omega, phase, coefs, Q, dtype)
    g = np.tensordot(w, dPhi, axes=([1], [1])) + np.tensordot(c, dK, axes=([1], [1]))      # S x M x D
    if ref.prior is not None:
        s1 = Ks @ a1
        gs1 = np.tensordot(dK, a1, axes=([1], [0]))                                         # M x D
        g = (dm * (1 - s1)[:, None])[None, :, :] + g - (m[:, None] * gs1)[None, :, :]
    return g


def grad_scale(ref, omega, phase, coefs, Q, dtype=np.float64):
    """T_grad (S, M, D)"""
    dPhi, Ks, dK, w, c, m, dm, a1 = _parts(ref, omega, phase, coefs, Q, dtype)
    T = np.tensordot(np.abs(w), np.abs(dPhi), axes=([1], [1])) + np.tensordot(np.abs(c), np.abs(dK), axes=([1], [1]))
    if ref.prior is not None:
        T = T + (np.abs(dm) * (1 + np.abs(Ks @ a1))[:, None])[None, :, :]
        T = T + np.einsum("mid,mi->md", np.abs(dK), np.abs(m[:, None] * a1[None, :]))[None, :, :]
    return T

"""
Removal of observations from a fitted model in O(N^2): the float64 NumPy restatement of what csrc/downdate.hip computes (ibo_gp_remove,
GaussianProcess.removeData).  The yardstick of tests/test_gpu_remove.py, itself pinned to numpy.linalg.cholesky / inv of the reduced matrix
and to the oracle's posterior by tests/test_downdate_reference.py.

With A = L L^T, W = L^-1 and row / column i taken out (m = N - 1 - i rows below it, trailing block L33 = L[i+1:, i+1:]):

    p = -W[i+1:, i] / W[i, i]                     (= L33^-1 l32, l32 = L[i+1:, i])
    t_0 = 1, t_{k+1} = t_k + p_k^2                one sequential sum in index order
    d_k = sqrt(t_{k+1} / t_k),  q_k = p_k / sqrt(t_k t_{k+1})
    Lt = diag(d) + strict-lower(p q^T)            the Cholesky factor of I + p p^T;  Lt^-1 = diag(1 / d) - strict-lower(q p^T)
    L33' = L33 Lt                                 column k = d_k L33[:, k] + q_k s_k,  s_k = sum_{j > k} p_j L33[:, j]   (suffix scan along rows)
    W~ = W[i+1:, :] + p (x) W[i, :]
    W'[j, :] = W~[j, :] / d_j - q_j sum_{k < j} p_k W~[k, :],  column i dropped                                          (prefix scan down columns)

Rows above i keep their entries (W loses its column i, which is zero there).  The step adds the positive semi-definite p p^T: nothing cancels.
"""
import numpy as np


def scalars(W, i):
    """(p, d, q) of one removal, the sum t in index order"""
    N = W.shape[0]
    m = N - 1 - i
    p = -W[i + 1:, i] / W[i, i]
    t = np.empty(m + 1)
    t[0] = 1.0
    for k in range(m):
        t[k + 1] = t[k] + p[k] * p[k]
    d = np.sqrt(t[1:] / t[:-1])
    q = p / np.sqrt(t[:-1] * t[1:])
    return p, d, q


def remove_row(L, W, i):
    """(L', W') of the model without observation i (0-based), (N - 1) x (N - 1) each, from the N x N lower triangular L and W = L^-1"""
    L = np.asarray(L, dtype=float); W = np.asarray(W, dtype=float)
    N = L.shape[0]
    if not (0 <= i < N and N >= 2):
        raise IndexError(i)
    m = N - 1 - i
    p, d, q = scalars(W, i)
    keep = np.r_[0:i, i + 1:N]
    L2 = L[np.ix_(keep, keep)].copy()
    W2 = W[np.ix_(keep, keep)].copy()
    if m == 0:
        return L2, W2
    # L: suffix scan along every row of the trailing block, from the diagonal leftwards
    L33 = L[i + 1:, i + 1:]
    out = np.zeros((m, m))
    s = np.zeros(m)
    for k in range(m - 1, -1, -1):
        col = L33[:, k]
        out[:, k] = d[k] * col + q[k] * s
        s = s + p[k] * col
    L2[i:, i:] = np.tril(out)
    # W: prefix scan down every column of the rows below i
    Wt = W[i + 1:, :] + np.outer(p, W[i, :])
    res = np.empty_like(Wt)
    S = np.zeros(N)
    for j in range(m):
        res[j] = Wt[j] / d[j] - q[j] * S
        S = S + p[j] * Wt[j]
    W2[i:, :] = res[:, keep]
    return L2, np.tril(W2)


def remove_rows(L, W, rows):
    """several observations: one step per row in DESCENDING index order, so the earlier indices stay valid"""
    rows = sorted(int(r) for r in rows)
    if len(set(rows)) != len(rows):
        raise ValueError("an index given twice")
    for r in reversed(rows):
        L, W = remove_row(L, W, r)
    return L, W


def cond2(A):
    s = np.linalg.svd(A, compute_uv=False)
    return s[0] / s[-1]


def relerr(got, ref):
    """max |got - ref| / max |ref|"""
    return np.max(np.abs(got - ref)) / np.max(np.abs(ref))

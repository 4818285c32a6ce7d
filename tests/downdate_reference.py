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

append_row is the other half of a sliding window: one step of ibo_gp_extend (GaussianProcess.addData) restated the same way.
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


def append_row(L, W, k, r):
    """(L', W') of the model with one more observation, (N + 1) x (N + 1) each: k = the new point's covariances with the N old ones, r its own
    diagonal entry.  z = W k, d = sqrt(r - z^T z); the new row of L is [z, d], the new row of W is [-z^T W / d, 1 / d]."""
    L = np.asarray(L, dtype=float); W = np.asarray(W, dtype=float); k = np.asarray(k, dtype=float)
    N = L.shape[0]
    z = W @ k
    d = np.sqrt(r - z @ z)
    L2 = np.zeros((N + 1, N + 1)); W2 = np.zeros((N + 1, N + 1))
    L2[:N, :N] = L; L2[N, :N] = z; L2[N, N] = d
    W2[:N, :N] = W; W2[N, :N] = -(z @ W) / d; W2[N, N] = 1.0 / d
    return L2, W2


def se_ard_matrix(X, ell, noise):
    """R = K(X, X) of the SE-ARD kernel with length scales ell, diagonal 1 + noise (GaussianProcess._computeCorrelations)"""
    X = np.asarray(X, dtype=float) / ell
    R = np.exp(-.5 * ((X[:, None, :] - X[None, :, :]) ** 2).sum(-1))
    R[np.diag_indices(len(X))] = 1.0 + noise
    return R


def window_plan(seed, N, D, steps, mode):
    """a seeded sequence of `steps` steps "append one point, remove one row" on N points in the unit cube: (X0, [(x_new, row), ...]).
    mode "window": the row is 0 (the oldest point goes); mode "random": any of the N + 1 rows present after the append."""
    rs = np.random.RandomState(seed)
    X0 = rs.rand(N, D)
    plan = []
    for _ in range(steps):
        x = rs.rand(D)
        plan.append((x, 0 if mode == "window" else int(rs.randint(0, N + 1))))
    return X0, plan


def run_window(X0, plan, ell, noise, checkpoints):
    """append_row + remove_row along a window_plan, from numpy's factor of X0.  At every step in `checkpoints` (1-based):
    {step: (cond_2(R), err L, err W)} against numpy.linalg.cholesky / inv of the matrix of the points held then.  -> (that dict, X at the end)"""
    X = np.array(X0, dtype=float)
    L = np.linalg.cholesky(se_ard_matrix(X, ell, noise))
    W = np.linalg.inv(L)
    out = {}
    for step, (x, row) in enumerate(plan, 1):
        k = np.exp(-.5 * (((X - x) / ell) ** 2).sum(-1))
        L, W = append_row(L, W, k, 1.0 + noise)
        X = np.vstack([X, x])
        L, W = remove_row(L, W, row)
        X = np.delete(X, row, axis=0)
        if step in checkpoints:
            R = se_ard_matrix(X, ell, noise)
            Lr = np.linalg.cholesky(R)
            out[step] = (cond2(R), relerr(L, Lr), relerr(W, np.linalg.inv(Lr)))
    return out, X


def cond2(A):
    s = np.linalg.svd(A, compute_uv=False)
    return s[0] / s[-1]


def relerr(got, ref):
    """max |got - ref| / max |ref|"""
    return np.max(np.abs(got - ref)) / np.max(np.abs(ref))

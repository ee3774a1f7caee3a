"""The f64 model of sbo_remove (csrc/remove.hip): deleting training points
from a lower Cholesky factor L and its inverse X = L^-1 by Givens rotations.

Removing stored position i of n: the carry column w = L[i+1:, i] and the
carry row x = X[i, :]; for k = i+1 .. n-1, in this order,

    r = hypot(L_kk, w_k),  c = L_kk / r,  s = w_k / r
    (L_jk, w_j)   <- (c L_jk + s w_j, -s L_jk + c w_j)      for rows j >= k
    (X_k,:, x)    <- (c X_k,: + s x,  -s X_k,: + c x)       for every column

then row and column i of both leave.  Several points go one after another in
ascending stored position with no compaction in between (a later chain only
touches columns to the right of its own position), and one compaction at the
end drops all of them.
"""
import numpy as np


def remove_chain(L, X, i):
    """Rotate position i out of L and X in place (row / column i stay, dead)."""
    n = L.shape[0]
    w = L[:, i].copy()
    x = X[i, :].copy()
    for k in range(i + 1, n):
        a, b = L[k, k], w[k]
        r = np.hypot(a, b)
        c, s = a / r, b / r
        col = L[k:, k].copy()
        L[k:, k] = c * col + s * w[k:]
        w[k:] = -s * col + c * w[k:]
        row = X[k, :].copy()
        X[k, :] = c * row + s * x
        x = -s * row + c * x


def remove(L, X, positions):
    """(L', X') after removing the stored `positions` (any order, no duplicates)
    from the factor L and its inverse X (dense n x n f64, lower)."""
    L = np.array(L, dtype=np.float64)
    X = np.array(X, dtype=np.float64)
    pos = sorted(int(p) for p in positions)
    for i in pos:
        remove_chain(L, X, i)
    keep = np.setdiff1d(np.arange(L.shape[0]), pos)
    return np.tril(L[np.ix_(keep, keep)]), np.tril(X[np.ix_(keep, keep)])


def remove_map(order, idx):
    """sbo_debug_remove_map's semantics: the stored positions of the caller
    indices `idx` in ascending order, and the renumbered order of the rows left
    (new index = old index minus the removed indices below it: numpy.delete)."""
    order = np.asarray(order, dtype=np.int64)
    idx = np.asarray(idx, dtype=np.int64)
    inv = np.empty_like(order)
    inv[order] = np.arange(order.size)
    pos = np.sort(inv[idx])
    renum = np.full(order.size, -1, dtype=np.int64)
    kept_idx = np.delete(np.arange(order.size), idx)
    renum[kept_idx] = np.arange(kept_idx.size)
    new_order = renum[np.delete(order, pos)]
    return pos, new_order

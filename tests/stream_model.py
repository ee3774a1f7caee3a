"""numpy f64 restatement of the streaming tick's update (sbo_tick_stream,
csrc/predict_update.hip).

A block append leaves the old rows of L^-1 and the old entries of
z = L^-1 (obs - m0) as they were, so with rows n_map .. n - 1 appended since
the posterior was last computed, every query q moves by

    v      = L^-1[n_map:n, 0:n] k*(q)
    var_new = var_old - sum_r v_r^2
    mu_new  = mu_old  + sum_r v_r z_r

Everything here works from a dense lower factor L (the device's f32 factor
widened, ``TerrainMapper.factor()``, or an f64 one), the training points in
the factor's order (``order()``) and f32 coordinates widened to f64, as the
kernel reads them.
"""
import numpy as np


def linv_rows(L, r0, r1):
    """Rows r0 .. r1 - 1 of L^-1 (f64): R L = I[r0:r1], solved as L^T R^T = I[:, r0:r1]."""
    L = np.asarray(L, np.float64)
    n = L.shape[0]
    rhs = np.zeros((n, r1 - r0))
    rhs[np.arange(r0, r1), np.arange(r1 - r0)] = 1.0
    # (back substitution on the trailing block that holds the answer's nonzeros:
    # rows of L^-1 are zero right of the diagonal)
    R = np.zeros((r1 - r0, n))
    R[:, :r1] = np.linalg.solve(L[:r1, :r1].T, rhs[:r1]).T
    return R


def kstar(x, y, qx, qy, ell, sf2):
    """(n, m) K*[k, q] = sf2 exp(-|x_k - q|^2 / 2 l^2) from f32 coordinates widened to f64."""
    x, y, qx, qy = (np.asarray(a, np.float32).astype(np.float64) for a in (x, y, qx, qy))
    d2 = (x[:, None] - qx[None, :]) ** 2 + (y[:, None] - qy[None, :]) ** 2
    return sf2 * np.exp(-d2 / (2.0 * ell * ell))


def update(L, x, y, obs, m0, n_map, qx, qy, ell, sf2):
    """(d var, d mu, |L^-1_r|_1, z_r) of the rows n_map .. n - 1 of the factor L
    over the queries: what one sbo_tick_stream update adds to the kept state,
    and the norms its cutoff bounds are made of."""
    L = np.asarray(L, np.float64)
    n = L.shape[0]
    R = linv_rows(L, n_map, n)
    z = R @ (np.asarray(obs, np.float32).astype(np.float64) - m0)
    v = R @ kstar(x, y, qx, qy, ell, sf2)
    return -(v * v).sum(axis=0), (v * z[:, None]).sum(axis=0), np.abs(R).sum(axis=1), z


def tile_boxes(x, y, tile=64):
    """(x0, x1, y0, y1) per 64-point k-tile of the training points in factor order."""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    return [(x[i:i + tile].min(), x[i:i + tile].max(), y[i:i + tile].min(), y[i:i + tile].max())
            for i in range(0, x.size, tile)]


def box_distance2(a, b):
    dx = max(0.0, a[0] - b[1], b[0] - a[1])
    dy = max(0.0, a[2] - b[3], b[2] - a[3])
    return dx * dx + dy * dy

"""numpy f64 restatement of the what-if posterior (sbo_whatif, csrc/whatif.hip).

Fitted state: K = K_f + s I (s = noise_level + jitter), a dense lower factor L
of it, the training points in the factor's order, z = L^-1 (obs - m0); the kept
posterior (mu, var) of the queries and its ``safe`` flags.  For candidates c_j:

    k_j   = k(train, c_j)        u_j = L^-1 k_j        w_j = L^-T u_j  (= K^-1 k_j)
    mu_c  = m0 + u_j . z         var_c = sf2 - |u_j|^2          d_j = var_c + s
    cov(q, c_j) = k(q, c_j) - k*(q) . w_j

and, conditioning on the optimistic y_j = mu_c + beta sd_c, sd_c = sqrt(max(var_c, 0)):

    mu'(q)  = mu(q)  + cov(q, c_j) beta sd_c / d_j
    var'(q) = var(q) - cov(q, c_j)^2 / d_j
    lo'(q)  = mu'(q) - beta sqrt(max(var'(q), 0))
    gain_j  = #{ q : not safe(q) and lo'(q) > f_min }

f32 coordinates are widened to f64 wherever a kernel value is formed, as the
kernels read them.
"""
import numpy as np

from tests.stream_model import kstar


def zvec(L, obs, m0):
    """z = L^-1 (obs - m0) in f64."""
    return np.linalg.solve(np.asarray(L, np.float64), np.asarray(obs, np.float32).astype(np.float64) - m0)


def whatif(L, x, y, z, m0, s, ell, sf2, cx, cy, qx, qy, mu, var, safe, beta, f_min):
    """dict of cov (p, m), cand_mu, cand_var, w_l1 (p), mu_new, var_new, lo_new
    (p, m), newly (p, m bool) and gain (p)."""
    L = np.asarray(L, np.float64)
    U = np.linalg.solve(L, kstar(x, y, cx, cy, ell, sf2))          # (n, p)
    W = np.linalg.solve(L.T, U)
    cand_mu = m0 + U.T @ np.asarray(z, np.float64)
    cand_var = sf2 - (U * U).sum(axis=0)
    d = cand_var + s
    cov = kstar(cx, cy, qx, qy, ell, sf2) - W.T @ kstar(x, y, qx, qy, ell, sf2)
    sd_c = np.sqrt(np.maximum(cand_var, 0.0))
    mu_new = np.asarray(mu, np.float64)[None, :] + cov * (beta * sd_c / d)[:, None]
    var_new = np.asarray(var, np.float64)[None, :] - cov * cov / d[:, None]
    lo_new = mu_new - beta * np.sqrt(np.maximum(var_new, 0.0))
    newly = (lo_new > f_min) & ~np.asarray(safe, bool)[None, :]
    return dict(cov=cov, cand_mu=cand_mu, cand_var=cand_var, w_l1=np.abs(W).sum(axis=0), mu_new=mu_new,
                var_new=var_new, lo_new=lo_new, newly=newly, gain=newly.sum(axis=1))


def cutoff(w_l1, cand_var, s, beta, sf2, budget_var, budget_mean):
    """sbo_whatif's auto cutoff restated: (L, err_cov).  The smallest L in
    [16, 149] that keeps every candidate's mean and variance bound within the
    budgets, 150 if none does, 0 (dense) when a budget is <= 0."""
    w_l1, cand_var = np.asarray(w_l1, np.float64), np.asarray(cand_var, np.float64)
    if not (budget_var > 0.0 and budget_mean > 0.0):
        return 0, 0.0
    v, d = np.maximum(cand_var, 0.0), cand_var + s
    L = 150
    for cand in range(16, 150):
        e = sf2 * 2.0 ** -cand * w_l1
        if np.all(abs(beta) * np.sqrt(v) * e / d <= budget_mean) and \
                np.all((2.0 * np.sqrt(sf2 * v) * e + e * e) / d <= budget_var):
            L = cand
            break
    return L, float(sf2 * 2.0 ** -L * w_l1.max())


def posterior(L, x, y, z, m0, ell, sf2, qx, qy):
    """(mu, var) of the queries from the factor: mu = m0 + v . z, var = sf2 - |v|^2, v = L^-1 k*."""
    V = np.linalg.solve(np.asarray(L, np.float64), kstar(x, y, qx, qy, ell, sf2))
    return m0 + V.T @ np.asarray(z, np.float64), sf2 - (V * V).sum(axis=0)


def candidates(qx, qy, safe, width, x, y, box, ell, p, seed=5):
    """p candidate points (f32) for a grid of `width` columns with flags
    `safe`: first one point 10 l outside the data box, one on a training point
    and one off the grid, then frontier grid points (unsafe points with a safe
    4-neighbour, with the grid's own coordinates) and further off-grid points.
    Returns (cx, cy, grid index or -1 per candidate)."""
    from safe_bayesian_optimization_amd.terrain import uniform
    qx, qy = np.asarray(qx, np.float32), np.asarray(qy, np.float32)
    S = np.asarray(safe, bool).reshape(-1, width)
    nb = np.zeros_like(S)
    nb[1:] |= S[:-1]
    nb[:-1] |= S[1:]
    nb[:, 1:] |= S[:, :-1]
    nb[:, :-1] |= S[:, 1:]
    frontier = np.flatnonzero((~S & nb).reshape(-1))
    (x0, x1), (y0, y1) = box
    u = uniform(seed, 2 * p + 2)
    cx, cy, gi = [], [], []
    special = [(x1 + 10.0 * ell, y1 + 10.0 * ell, -1), (float(x[7]), float(y[7]), -1),
               (x0 + u[0] * (x1 - x0), y0 + u[1] * (y1 - y0), -1)]
    step = max(1, frontier.size // max(1, p))
    for j in range(p):
        if j == 0 and frontier.size:      # (p = 1: a frontier point)
            c = (qx[frontier[0]], qy[frontier[0]], int(frontier[0]))
        elif j <= len(special):
            c = special[j - 1]
        elif j % 4 == 3 or (j * step) >= frontier.size:
            c = (x0 + u[2 * j] * (x1 - x0), y0 + u[2 * j + 1] * (y1 - y0), -1)
        else:
            i = int(frontier[j * step])
            c = (qx[i], qy[i], i)
        cx.append(c[0])
        cy.append(c[1])
        gi.append(c[2])
    return np.asarray(cx, np.float32), np.asarray(cy, np.float32), np.asarray(gi, np.int64)

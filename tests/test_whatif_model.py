"""The what-if posterior's identity in numpy f64 (tests/whatif_model.py) against
a refit, sbo_whatif's cutoff chooser against its rule restated, and the
expander selection (no device)."""
import ctypes

import numpy as np
import pytest

from tests import whatif_model as WM
from tests.stream_model import kstar
from safe_bayesian_optimization_amd import _native as N
from safe_bayesian_optimization_amd import node
from safe_bayesian_optimization_amd.terrain import normal, smooth_field, uniform

ELL, SF2, SN2, M0, BETA = 0.4, 1.0, 0.1, 0.0, 2.0
GRID = (37, 29)


def case(n, box, seed):
    (x0, x1), (y0, y1) = box
    u = uniform(seed, 2 * n)
    x = (x0 + u[0::2] * (x1 - x0)).astype(np.float32)
    y = (y0 + u[1::2] * (y1 - y0)).astype(np.float32)
    obs = (smooth_field(x - x0, y - y0, max(x1 - x0, y1 - y0), ELL, seed) +
           np.sqrt(SN2) * normal(seed + 1, n)).astype(np.float32)
    gx = np.linspace(x0 - 0.3, x1 + 0.3, GRID[0])
    gy = np.linspace(y0 - 0.3, y1 + 0.3, GRID[1])
    QY, QX = np.meshgrid(gy, gx, indexing="ij")
    return x, y, obs, QX.reshape(-1).astype(np.float32), QY.reshape(-1).astype(np.float32)


def gram(x, y):
    return kstar(x, y, x, y, ELL, SF2) + SN2 * np.eye(len(x))


def nrel(a, b):
    return float(np.abs(a - b).max() / np.abs(b).max())


SIDE = ELL * np.sqrt(333 / 8.0)


@pytest.mark.parametrize("n,box", [(333, ((0.0, SIDE), (0.0, SIDE))), (700, ((0.0, 1.0), (0.0, 2.5))),
                                   (1061, ((0.0, 24 * ELL), (0.0, 24 * ELL)))])
def test_whatif_is_the_refit_with_the_fantasy_point(n, box):
    """mu', var' of the model equal the posterior of a numpy refit with
    (c_j, mu_c + beta sd_c) added: 1e-8 normwise (f64 eps x cond(K) <= 1e5 x 1e3
    of margin; measured 6e-15)."""
    x, y, obs, qx, qy = case(n, box, seed=1)
    L = np.linalg.cholesky(gram(x, y))
    z = WM.zvec(L, obs, M0)
    mu, var = WM.posterior(L, x, y, z, M0, ELL, SF2, qx, qy)
    f_min = float(np.percentile(obs, 40.0))
    safe = mu - BETA * np.sqrt(np.maximum(var, 0.0)) > f_min
    cx, cy, _ = WM.candidates(qx, qy, safe, GRID[0], x, y, box, ELL, 9)
    w = WM.whatif(L, x, y, z, M0, SN2, ELL, SF2, cx, cy, qx, qy, mu, var, safe, BETA, f_min)
    assert w["gain"].max() > 0 and np.unique(w["gain"]).size > 1, w["gain"]
    worst = 0.0
    for j in range(cx.size):
        x1, y1 = np.append(x, cx[j]), np.append(y, cy[j])
        yj = w["cand_mu"][j] + BETA * np.sqrt(max(w["cand_var"][j], 0.0))
        r1 = np.append(obs.astype(np.float64), yj) - M0
        L1 = np.linalg.cholesky(gram(x1, y1))
        mu1, var1 = WM.posterior(L1, x1, y1, np.linalg.solve(L1, r1), M0, ELL, SF2, qx, qy)
        worst = max(worst, nrel(w["mu_new"][j], mu1), nrel(w["var_new"][j], var1))
    print(f"n {n}: refit identity {worst:.2e}, gains {w['gain']}")
    assert worst < 1e-8, worst


def chooser(w_l1, cand_var, s, beta, sf2, bvar, bmean):
    w_l1, cand_var = np.ascontiguousarray(w_l1, np.float64), np.ascontiguousarray(cand_var, np.float64)
    L, err = ctypes.c_int32(-7), ctypes.c_double(-1.0)
    st = N.lib().sbo_debug_whatif_cutoff(w_l1.size, w_l1.ctypes.data, cand_var.ctypes.data, s, beta, sf2, bvar, bmean,
                                         ctypes.byref(L), ctypes.byref(err))
    assert st == 0
    return L.value, err.value


def test_cutoff_chooser_follows_its_rule():
    u = uniform(9, 64)
    w_l1 = 1.0 + 400.0 * u[:32]
    cand_var = 0.9 * u[32:]
    cand_var[3] = -1e-9      # (a rounded-negative variance: sd_c = 0)
    budget = 2.0 ** -20
    # the smallest L that fits: L itself is within the budgets and L - 1 is not
    L, err = chooser(w_l1, cand_var, SN2, BETA, SF2, budget, budget)
    assert (L, err) == WM.cutoff(w_l1, cand_var, SN2, BETA, SF2, budget, budget)
    assert 16 < L < 150

    def within(Lc):
        e = SF2 * 2.0 ** -Lc * w_l1
        v, d = np.maximum(cand_var, 0.0), cand_var + SN2
        return bool(np.all(BETA * np.sqrt(v) * e / d <= budget) and
                    np.all((2.0 * np.sqrt(SF2 * v) * e + e * e) / d <= budget))
    assert within(L) and not within(L - 1)
    assert err == SF2 * 2.0 ** -L * w_l1.max()
    # a generous budget stops at the range's lower end
    assert chooser(w_l1, cand_var, SN2, BETA, SF2, 1e6, 1e6)[0] == 16
    # only the mean budget binds / only the variance budget binds
    for bv, bm in ((1e6, 2.0 ** -30), (2.0 ** -30, 1e6)):
        assert chooser(w_l1, cand_var, SN2, BETA, SF2, bv, bm) == WM.cutoff(w_l1, cand_var, SN2, BETA, SF2, bv, bm)
    # no L in range qualifies: 150, which drops only exact zeros
    L, err = chooser(w_l1 * 1e30, cand_var, SN2, BETA, SF2, 1e-300, 1e-300)
    assert L == 150 and err == SF2 * 2.0 ** -150 * 1e30 * w_l1.max()
    # a budget <= 0: dense
    for bv, bm in ((0.0, 1.0), (1.0, 0.0), (-1.0, -1.0)):
        assert chooser(w_l1, cand_var, SN2, BETA, SF2, bv, bm) == (0, 0.0)
    # argument checks, and the struct the library writes
    assert N.lib().sbo_debug_whatif_cutoff(0, None, None, 0.1, 2.0, 1.0, 1.0, 1.0, None, None) == 1
    assert N.lib().sbo_whatif(None, None, None, 1, 2.0, 0.0, None, None, None, None, None, None, 0) == 1
    assert ctypes.sizeof(N.sbo_whatif_info) == 80


def test_select_expander_ties_follow_the_nodes_rule():
    cands = np.arange(6)
    # the maximal gain wins whatever its width
    assert node.select_expander(cands, [0, 3, 1, 3, 0, 2], [9.0, 1.0, 9.0, 0.5, 9.0, 9.0]) == 1
    # among equal gains: the first strict maximum of width in sorted order
    assert node.select_expander(cands, [3, 3, 1, 3, 0, 3], [1.0, 2.0, 9.0, 2.0, 9.0, 1.5]) == 1
    assert node.select_expander(cands, [0, 0, 0, 0, 0, 0], [1.0, 2.0, 3.0, 3.0, 0.0, 1.0]) == 2
    assert node.select_expander(np.zeros(0, np.int64), [], []) == -1


@pytest.mark.parametrize("seed", [2, 3, 4])
def test_zero_gains_reproduce_next_subgoal(seed):
    """On a random field with every gain zero, the expander selection over the
    node's candidate set is sbo_next_subgoal's choice."""
    W, H = 23, 17
    gy, gx = np.meshgrid(np.linspace(0.0, 3.2, H), np.linspace(0.0, 4.4, W), indexing="ij")
    Dx, Dy = gx.reshape(-1), gy.reshape(-1)
    u = uniform(seed, 2 * W * H)
    lo = smooth_field(Dx, Dy, 4.4, ELL, seed) - 0.2 * u[:W * H]
    hi = lo + 0.1 + u[W * H:]
    hi[::7] = hi[3]          # equal widths among candidates: the strict > matters
    lo[::7] = lo[3]
    safe = (lo > np.percentile(lo, 55.0)).astype(np.uint8)
    goal = (4.0 * u[0], 3.0 * u[1])
    want = node.next_subgoal(Dx, Dy, lo, hi, safe, W, H, *goal)
    frontier = node.find_safety_contour_indices(Dx, Dy, safe, W, H)
    assert frontier.size >= 8 and want >= 0
    cands, pos = node.subgoal_candidates(Dx, Dy, frontier, goal)
    assert np.unique(cands).size == cands.size and np.all(np.diff(pos) > 0)
    assert pos[-1] < max(1, frontier.size // 4)
    b = node.select_expander(cands, np.zeros(cands.size, np.int64), (hi - lo)[cands])
    assert cands[b] == want

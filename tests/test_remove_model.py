"""tests/remove_model.py (the f64 recurrences of sbo_remove) against a fresh
factorization: numpy.linalg.cholesky and numpy.linalg.inv of the RBF matrix
without the removed rows and columns.

n = 260 (three 128-column chain steps, the last one partial), default
hyper-parameters, about 8 points per l^2.  Tolerance 1e-12, absolute and
elementwise: the recurrences reach <= 6e-14 here (n rotations of unit
roundoff 1.1e-16 on entries of at most 1 / sqrt(noise) ~ 3.2).
"""
import numpy as np
import pytest

from safe_bayesian_optimization_amd.terrain import Hyper, uniform
from tests import remove_model as RM

N_PTS = 260
TOL = 1e-12


@pytest.fixture(scope="module")
def gram():
    h = Hyper()
    side = h.length_scale * np.sqrt(N_PTS / 8.0)
    u = uniform(5, 2 * N_PTS)
    x, y = u[0::2] * side, u[1::2] * side
    d2 = (x[:, None] - x[None, :]) ** 2 + (y[:, None] - y[None, :]) ** 2
    K = h.sf2 * np.exp(-0.5 * d2 / h.length_scale ** 2) + h.sn2 * np.eye(N_PTS)
    L = np.linalg.cholesky(K)
    return K, L, np.linalg.inv(L)


def random_positions(count):
    return sorted(int(p) for p in np.random.default_rng(11).choice(N_PTS, count, replace=False))


CASES = {"first": [0], "last": [N_PTS - 1], "step_edge_127": [127], "step_edge_128": [128],
         "batch5": [5, 128, 129, 255, 259], "batch33": random_positions(33)}


@pytest.mark.parametrize("case", list(CASES))
def test_rotations_match_a_fresh_factorization(gram, case):
    K, L, X = gram
    pos = CASES[case]
    keep = np.setdiff1d(np.arange(N_PTS), pos)
    L1, X1 = RM.remove(L, X, pos)
    Lref = np.linalg.cholesky(K[np.ix_(keep, keep)])
    Xref = np.linalg.inv(Lref)
    assert L1.shape == Lref.shape and X1.shape == Xref.shape
    assert np.all(np.diag(L1) > 0.0)
    dl, dx = np.abs(L1 - Lref).max(), np.abs(X1 - np.tril(Xref)).max()
    print(f"{case}: |dL| {dl:.2e} |dX| {dx:.2e}")
    assert dl <= TOL and dx <= TOL


def test_batch_order_does_not_matter(gram):
    _, L, X = gram
    a = RM.remove(L, X, [5, 128, 129, 255, 259])
    b = RM.remove(L, X, [259, 5, 255, 129, 128])
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_inputs_are_left_alone(gram):
    _, L, X = gram
    L0, X0 = L.copy(), X.copy()
    RM.remove(L, X, [3, 200])
    assert np.array_equal(L, L0) and np.array_equal(X, X0)

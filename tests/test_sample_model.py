"""The posterior sample paths in numpy f64 (tests/sample_model.py) against an
independent dense posterior, their independence of how a range of samples is
cut into calls, and sbo_sample's cutoff chooser against its rule restated (no
device).

The statistical checks are conditions on one seed, not statistics to re-tune:
S = 256 samples of seed 7 at F = 256 and 1024 features on the three shapes of
tests/test_gpu_whatif.py.  Measured with this model: rms of (path - mu) / sd
0.968 .. 1.014, max_q |mean_j path - mu| at most 3.00 sd_max / sqrt(S),
kernel_err 0.1227 at F = 256 and 0.0519 at F = 1024.  A model without eps gives
an rms of 0.63 - 0.65, eps scaled by s instead of sqrt(s) 0.67 - 0.70, features
scaled by sqrt(2 / F) 1.18 - 1.21, the update's sign wrong more than 12.
"""
import ctypes

import numpy as np
import pytest

from tests import sample_model as SM
from tests.stream_model import kstar
from tests.test_whatif_model import ELL, M0, SF2, SIDE, SN2, case
from safe_bayesian_optimization_amd import _native as N
from safe_bayesian_optimization_amd.terrain import uniform

S, SEED = 256, 7
SHAPES = {
    "n333": (333, ((0.0, SIDE), (0.0, SIDE))),
    "lpsc700": (700, ((0.0, 1.0), (0.0, 2.5))),
    "box24l": (1061, ((0.0, 24 * ELL), (0.0, 24 * ELL))),
}
_fits = {}


def fit(shape):
    """(L, x, y, qx, qy, mu, sd): a numpy fit of the shape and its dense posterior on the grid, by
    solves with K itself (computed once, never changed)."""
    if shape not in _fits:
        n, box = SHAPES[shape]
        x, y, obs, qx, qy = case(n, box, seed=1)
        K = kstar(x, y, x, y, ELL, SF2) + SN2 * np.eye(n)
        Ks = kstar(x, y, qx, qy, ELL, SF2)
        mu = M0 + Ks.T @ np.linalg.solve(K, obs.astype(np.float64) - M0)
        var = SF2 - (Ks * np.linalg.solve(K, Ks)).sum(axis=0)
        _fits[shape] = (np.linalg.cholesky(K), x, y, qx, qy, mu, np.sqrt(var))
    return _fits[shape]


@pytest.mark.parametrize("F", [256, 1024])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_paths_have_the_posteriors_moments(shape, F):
    L, x, y, qx, qy, mu, sd = fit(shape)
    r = SM.sample(L, x, y, np.arange(x.size), SN2, ELL, np.sqrt(SF2), qx, qy, mu, SEED, 0, S, F)
    dev = r["paths"] - mu[None, :]
    rms = float(np.sqrt(np.mean((dev / sd[None, :]) ** 2)))
    mean_err = float(np.abs(dev.mean(axis=0)).max() / (sd.max() / np.sqrt(S)))
    print(f"{shape} F {F}: rms {rms:.3f} mean {mean_err:.2f} sd_max/sqrt(S) kernel_err {r['kernel_err']:.4f}")
    assert 0.93 <= rms <= 1.07
    assert mean_err <= 4.0
    assert r["kernel_err"] <= 4.0 / np.sqrt(2.0 * F)


def test_a_path_does_not_depend_on_how_the_samples_are_cut():
    L, x, y, qx, qy, mu, _ = fit("n333")
    args = (L, x, y, np.arange(x.size), SN2, ELL, np.sqrt(SF2), qx, qy, mu, SEED)
    whole = SM.sample(*args, 0, 150, 37)["paths"]
    a, b = SM.sample(*args, 0, 17, 37)["paths"], SM.sample(*args, 17, 133, 37)["paths"]
    # (the draws are the same numbers; the matrix products over another number of columns may block differently)
    assert np.abs(np.vstack([a, b]) - whole).max() <= 1e-12 * np.abs(whole).max()
    d0, d1 = SM.draws(SEED, 0, 150, 37, 333), SM.draws(SEED, 17, 133, 37, 333)
    assert np.array_equal(d0[0], d1[0]) and np.array_equal(d0[1][17:], d1[1]) and np.array_equal(d0[2][17:], d1[2])
    # the training order moves eps with its point: a permuted fit draws the same paths
    o = np.argsort(uniform(3, x.size))
    Lp = np.linalg.cholesky(kstar(x[o], y[o], x[o], y[o], ELL, SF2) + SN2 * np.eye(x.size))
    perm = SM.sample(Lp, x[o], y[o], o, SN2, ELL, np.sqrt(SF2), qx, qy, mu, SEED, 0, 17, 37)["paths"]
    assert np.abs(perm - a).max() <= 1e-9 * np.abs(a).max()


def chooser(w_l1, sf2, bmean):
    w_l1 = np.ascontiguousarray(w_l1, np.float64)
    L, err = ctypes.c_int32(-7), ctypes.c_double(-1.0)
    st = N.lib().sbo_debug_sample_cutoff(w_l1.size, w_l1.ctypes.data, sf2, bmean, ctypes.byref(L), ctypes.byref(err))
    assert st == 0
    return L.value, err.value


def test_cutoff_chooser_follows_its_rule():
    u = uniform(9, 32)
    budget = 2.0 ** -20
    for scale in (1.0, 1e2, 1e4, 1e6):          # |w|_1 spanning 1 .. 1e6
        w_l1 = 1.0 + (scale - 1.0) * u
        L, err = chooser(w_l1, SF2, budget)
        assert (L, err) == SM.cutoff(w_l1, SF2, budget)
        assert 16 < L < 150
        # the smallest L that fits: L is within the budget and L - 1 is not
        assert SF2 * 2.0 ** -L * w_l1.max() <= budget < SF2 * 2.0 ** -(L - 1) * w_l1.max()
        assert err == SF2 * 2.0 ** -L * w_l1.max()
    w_l1 = 1.0 + 400.0 * u
    # another sf2; a generous budget stops at the range's lower end
    assert chooser(w_l1, 2.5, budget) == SM.cutoff(w_l1, 2.5, budget)
    assert chooser(w_l1, SF2, 1e6) == (16, SF2 * 2.0 ** -16 * w_l1.max())
    # no L in range qualifies: 150, which drops only exact zeros
    L, err = chooser(w_l1 * 1e30, SF2, 1e-300)
    assert L == 150 and err == SF2 * 2.0 ** -150 * 1e30 * w_l1.max()
    # a budget <= 0: dense
    for bm in (0.0, -1.0):
        assert chooser(w_l1, SF2, bm) == (0, 0.0)
    # argument checks, and the struct the library writes
    assert N.lib().sbo_debug_sample_cutoff(0, None, 1.0, 1.0, None, None) == 1
    assert N.lib().sbo_sample(None, 7, 0, 1, 1, 2.0, 0.0, 0, None, None, None, None, 0) == 1
    assert N.lib().sbo_debug_sample_draws(None, 7, 0, 1, 1, None, None, None) == 1
    assert ctypes.sizeof(N.sbo_sample_info) == 96

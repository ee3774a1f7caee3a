"""The f64 model of sbo_evidence (tests/evidence_model.py) against independent
references, and the host parts of the C ABI (no device):

  - both forms of the model against scikit-learn's log_marginal_likelihood and
    its gradient, ConstantKernel * RBF + WhiteKernel, to 1e-8 relative;
  - its leave-one-out predictive against n brute-force refits at n = 40;
  - sbo_debug_evidence_pairs (the k-tile pair cutoff) against the model's numpy
    restatement on 1061 points over 24 l x 24 l in k-d order;
  - sbo_evidence's argument checks that need no device.
"""
import ctypes

import numpy as np
import pytest

from safe_bayesian_optimization_amd import _native as N
from tests import evidence_model as EM

ELL, SF, NOISE = 0.4, 1.0, 0.1


def rel(a, b):
    return float(np.max(np.abs(np.asarray(a) - np.asarray(b))) / max(np.max(np.abs(b)), 1e-300))


@pytest.mark.parametrize("n, side, ell, sf, noise, m0", [(150, 3.0, 0.4, 1.0, 0.1, 0.0),
                                                        (96, 2.0, 0.7, 1.3, 0.05, 0.25)])
def test_model_matches_sklearn(n, side, ell, sf, noise, m0):
    import sklearn.gaussian_process as gp
    from sklearn.gaussian_process.kernels import RBF, ConstantKernel, WhiteKernel
    x, y, obs = EM.case_data(n, (0.0, side), (0.0, side), ell, noise)
    x, y, obs = (np.asarray(a, np.float64) for a in (x, y, obs))
    k = ConstantKernel(sf * sf) * RBF(ell) + WhiteKernel(noise)
    g = gp.GaussianProcessRegressor(kernel=k, alpha=0.0, optimizer=None).fit(np.stack([x, y], 1), obs - m0)
    theta = np.log([sf * sf, ell, noise])
    lml, grad = g.log_marginal_likelihood(theta, eval_gradient=True)
    # sklearn: d / d (log sf2, log l, log noise);  d / d log sigma_f = 2 d / d log sf2
    ref = np.array([grad[1], 2.0 * grad[0], grad[2]])
    a = EM.evidence(x, y, obs, ell, sf, noise, m0)
    L = np.linalg.cholesky(EM.kernel(x, y, ell, sf * sf)[0] + noise * np.eye(n))
    b = EM.evidence_from_factor(L, x, y, obs, ell, sf, noise, m0)
    for e in (a, b):
        assert abs(e["lml"] - lml) <= 1e-8 * abs(lml)
        assert rel(e["grad"][:3], ref) <= 1e-8
    # the prior mean's derivative: central difference of the model's own lml
    h = 1e-5
    fd = (EM.evidence(x, y, obs, ell, sf, noise, m0 + h)["lml"] -
          EM.evidence(x, y, obs, ell, sf, noise, m0 - h)["lml"]) / (2 * h)
    assert abs(a["grad"][3] - fd) <= 1e-6 * max(1.0, abs(fd))
    assert abs(b["grad"][3] - a["grad"][3]) <= 1e-8 * max(1.0, abs(a["grad"][3]))


def test_model_loo_matches_brute_force():
    n = 40
    x, y, obs = EM.case_data(n, (0.0, 2.0), (0.0, 2.0), ELL, NOISE)
    mean, var = EM.loo_brute_force(x, y, obs, ELL, SF, NOISE, 0.1)
    a = EM.evidence(x, y, obs, ELL, SF, NOISE, 0.1)
    L = np.linalg.cholesky(EM.kernel(x, y, ELL, SF * SF)[0] + NOISE * np.eye(n))
    b = EM.evidence_from_factor(L, x, y, obs, ELL, SF, NOISE, 0.1)
    lp = float(np.sum(-0.5 * np.log(2 * np.pi * var) - 0.5 * (np.asarray(obs, np.float64) - mean) ** 2 / var))
    for e in (a, b):
        assert rel(e["loo_mean"], mean) <= 1e-12
        assert rel(e["loo_var"], var) <= 1e-12
        assert abs(e["loo_log_pred"] - lp) <= 1e-12 * abs(lp)


def kd_sorted(x, y, obs):
    perm = np.empty(x.size, np.int64)
    assert N.lib().sbo_kd_order(x.ctypes.data, y.ctypes.data, x.size, 0, perm.ctypes.data) == 0
    return x[perm], y[perm], obs[perm]


def native_pairs(boxes, a, s, ell, sf, budget):
    T = boxes.shape[0]
    boxes = np.ascontiguousarray(boxes, np.float32)
    a, s = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(s, np.float64)
    drop = np.full((T, T), 7, np.uint8)
    bound = ctypes.c_double(-1.0)
    st = N.lib().sbo_debug_evidence_pairs(boxes.ctypes.data, a.ctypes.data, s.ctypes.data, T,
                                          N.sbo_hyper(ell, sf, NOISE, 0.0), budget, drop.ctypes.data,
                                          ctypes.byref(bound))
    assert st == 0
    return drop, bound.value


def test_pair_cutoff_matches_model_and_bounds_its_effect():
    n = 1061
    x, y, obs = kd_sorted(*EM.case_data(n, (0.0, 24 * ELL), (0.0, 24 * ELL), ELL, NOISE))
    e = EM.evidence(x, y, obs, ELL, SF, NOISE)
    boxes = EM.tile_boxes(x, y)
    a, s = EM.tile_l1(e["alpha"], e["c"])
    T = boxes.shape[0]
    assert T == 17
    budget = n * 2.0 ** -20
    drop, bound = native_pairs(boxes, a, s, ELL, SF, budget)
    mdrop, mbound = EM.pair_cutoff(boxes, a, s, ELL, SF * SF, budget)
    assert set(np.unique(drop)) <= {0, 1}
    assert np.array_equal(drop.astype(bool), mdrop)
    assert np.array_equal(drop, drop.T) and not drop.diagonal().any()
    assert abs(bound - mbound) <= 1e-12 * mbound
    Kinv = np.linalg.inv(EM.kernel(x, y, ELL, SF * SF)[0] + NOISE * np.eye(n))
    effect = EM.dropped_effect(mdrop, x, y, e["alpha"], Kinv, ELL, SF * SF)
    print(f"dropped {int(drop.sum())} of {T * T} ordered pairs, bound {bound:.3e}, budget {budget:.3e}, "
          f"effect {effect:.3e}")
    assert abs(effect) <= bound <= budget
    assert drop.sum() >= 0.10 * T * T          # not vacuous
    # no budget, no drops; a budget below every bound, none either
    for b in (0.0, -1.0, 1e-300):
        d0, b0 = native_pairs(boxes, a, s, ELL, SF, b)
        assert not d0.any() and b0 == 0.0
    # a larger budget drops a superset and never a pair closer than sqrt(2) l
    d1, b1 = native_pairs(boxes, a, s, ELL, SF, 1e6)
    assert (d1 >= drop).all() and b1 <= 1e6
    m1, _ = EM.pair_cutoff(boxes, a, s, ELL, SF * SF, 1e6)
    assert np.array_equal(d1.astype(bool), m1) and not d1.all()


def test_evidence_rejects_null_arguments_without_device():
    lib = N.lib()
    info = N.sbo_evidence_info()
    info.struct_size = ctypes.sizeof(info)
    assert lib.sbo_evidence(None, ctypes.byref(info), None, None, 0) == 1
    assert lib.sbo_evidence(None, None, None, None, 0) == 1
    bound = ctypes.c_double()
    assert lib.sbo_debug_evidence_pairs(None, None, None, 3, N.sbo_hyper(ELL, SF, NOISE, 0.0), 1.0, None,
                                        ctypes.byref(bound)) == 1
    assert ctypes.sizeof(N.sbo_evidence_info) == 120

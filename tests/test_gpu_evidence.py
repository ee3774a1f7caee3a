"""sbo_evidence (include/sbo.h, csrc/evidence.hip) through the C ABI on cuda:0:
the log marginal likelihood, its gradient and the leave-one-out predictive
read off the fitted state, against the f64 model of tests/evidence_model.py.

Deviations are max |d| / max |ref| per quantity (a scalar is its own vector;
the four gradients are one vector, so are each LOO array).  Two references:
the model given the device's own f32 factor (what the device arithmetic adds
to it: f64 rounding only) and the model from scratch (which adds the f32
factorization's error, bounded by the project's end-to-end 2e-4).

Measured on an MI355X (the largest deviation over the three cases, all
quantities, grad[0] with every pair run: what the cutoff adds is the cutoff
test's own assertion, |d grad0| <= grad_err_bound <= grad_budget):
    given the factor   MEASURED_GIVEN, tolerance GIVEN_TOL = 16 x that
    end to end         MEASURED_E2E,   tolerance E2E_TOL   =  4 x that (< 2e-4)
    fit_hyper          MEASURED_DELTA nats below the model's optimum,
                       DELTA = 4 x that
"""
import ctypes

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from safe_bayesian_optimization_amd import TerrainMapper  # noqa: E402
from safe_bayesian_optimization_amd import _native as N  # noqa: E402
from safe_bayesian_optimization_amd.terrain import Hyper, normal, uniform  # noqa: E402
from tests import evidence_model as EM  # noqa: E402

# lpsc_box, the gradient vector (its LOO variance: 2.5e-15).  After appends, every pair run (budget 0, so
# grad[0] carries no cutoff): 1.8e-15 at worst (a LOO variance), the gradient vector 1.5e-15 on a grad[0] of 2.3e2
MEASURED_GIVEN = 6.4e-15
GIVEN_TOL = 16 * MEASURED_GIVEN
# lpsc_box, the gradient vector, every pair run (9.605e-6; its LOO mean 5.3e-6); the appended state against a
# fresh fit, both under the default budget: 6.2e-6 (a LOO variance)
MEASURED_E2E = 9.6e-6
E2E_TOL = 4 * MEASURED_E2E
MEASURED_DELTA = 5.6e-9      # nats; 14 evaluations on either side, optimum 1.27 nats above the truth
DELTA = 4 * MEASURED_DELTA

HYPER = Hyper()
ELL = HYPER.length_scale
CASES = {
    "one_tile_row": (300, (0.0, 4 * ELL), (0.0, 4 * ELL)),      # one partial 256-row block, every pair kept
    "wide": (1061, (0.0, 24 * ELL), (0.0, 24 * ELL)),           # 17 tiles, the cutoff drops pairs
    "lpsc_box": (700, (0.0, 1.0), (0.0, 2.5)),                  # dense data: the precise regime
}
SCALARS = ("lml", "data_fit", "log_det", "loo_log_pred")


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def call(gm, loo=True, flags=0, struct_size=None, mean=None, var=None):
    """(status, info, loo_mean, loo_var) of one sbo_evidence call."""
    info = N.sbo_evidence_info()
    info.struct_size = ctypes.sizeof(info) if struct_size is None else struct_size
    n = gm.n
    if loo and mean is None and var is None:
        mean, var = np.full(n, np.nan), np.full(n, np.nan)
    ptr = lambda a: None if a is None else ctypes.c_void_p(a.data_ptr() if hasattr(a, "data_ptr") else a.ctypes.data)  # noqa: E731
    st = N.lib().sbo_evidence(gm.ctx.handle, ctypes.byref(info), ptr(mean), ptr(var), flags)
    return st, info, mean, var


def as_dict(info, mean, var):
    d = {f: getattr(info, f) for f, _ in N.sbo_evidence_info._fields_ if f != "grad"}
    d["grad"] = np.array(info.grad[:])
    d["loo_mean"], d["loo_var"] = mean, var
    return d


def evidence(gm):
    st, info, mean, var = call(gm)
    assert st == 0, N.lib().sbo_last_error(gm.ctx.handle)
    return as_dict(info, mean, var)


def nrel(a, b):
    a, b = np.atleast_1d(np.asarray(a, np.float64)), np.atleast_1d(np.asarray(b, np.float64))
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


def deviations(got, ref):
    """Per quantity max |d| / max |ref| (the four gradients are one vector)."""
    return {k: nrel(got[k], ref[k]) for k in SCALARS + ("loo_mean", "loo_var", "grad")}


def model_given_factor(gm, x, y, obs, hyper=HYPER):
    """The model from the device's factor; LOO arrays back in the caller's order."""
    L, _ = gm.factor()
    o = gm.order()
    m = EM.evidence_from_factor(L.astype(np.float64), x[o], y[o], obs[o], hyper.length_scale, hyper.sigma_f,
                                hyper.noise_level, hyper.prior_mean)
    for k in ("loo_mean", "loo_var"):
        a = np.empty_like(m[k])
        a[o] = m[k]
        m[k] = a
    return m


class Case:
    def __init__(self, name):
        n, xr, yr = CASES[name]
        self.name, self.n = name, n
        self.x, self.y, self.obs = EM.case_data(n, xr, yr, ELL, HYPER.noise_level)
        self.gm = TerrainMapper(0, HYPER)
        self.gm.fit(self.x, self.y, self.obs)
        self.cut = evidence(self.gm)                        # the default budget
        self.gm.set_option(N.SBO_OPT_EVIDENCE_BUDGET, 0)
        self.dense = evidence(self.gm)
        self.gm.set_option(N.SBO_OPT_EVIDENCE_BUDGET, 20)
        self.given = model_given_factor(self.gm, self.x, self.y, self.obs)
        self.scratch = EM.evidence(self.x, self.y, self.obs, ELL, HYPER.sigma_f, HYPER.noise_level, HYPER.prior_mean)


@pytest.fixture(scope="module")
def cases(dev):
    return {k: Case(k) for k in CASES}


@pytest.mark.parametrize("name", list(CASES))
def test_matches_model_given_device_factor(cases, name):
    c = cases[name]
    d = deviations(c.dense, c.given)
    print(f"\n[given factor] {name} n={c.n}: " + " ".join(f"{k}={v:.3e}" for k, v in d.items()))
    assert c.dense["n"] == c.n and c.dense["pairs_kept"] == c.dense["pairs_total"] and not c.dense["dropped"]
    assert c.dense["grad_err_bound"] == 0.0
    assert max(d.values()) <= GIVEN_TOL, d


@pytest.mark.parametrize("name", list(CASES))
def test_matches_f64_model_end_to_end(cases, name):
    c = cases[name]
    d = deviations(c.dense, c.scratch)           # (what the cutoff adds: test_cutoff_is_bounded_...)
    print(f"\n[end to end] {name} n={c.n}: " + " ".join(f"{k}={v:.3e}" for k, v in d.items()))
    assert max(d.values()) <= E2E_TOL <= 2e-4, d


def test_cutoff_is_bounded_and_touches_grad0_only(cases):
    c = cases["wide"]
    cut, dense = c.cut, c.dense
    T = (c.n + 63) // 64
    assert cut["pairs_total"] == dense["pairs_total"] == T * (T + 1) // 2
    dropped = cut["pairs_total"] - cut["pairs_kept"]
    err = abs(cut["grad"][0] - dense["grad"][0])
    print(f"\n[cutoff] kept {cut['pairs_kept']} of {cut['pairs_total']}, |d grad0| {err:.3e}, "
          f"bound {cut['grad_err_bound']:.3e}, budget {cut['grad_budget']:.3e}, grad0 {dense['grad'][0]:.6e}")
    assert cut["dropped"] == 1 and dropped >= 0.10 * cut["pairs_total"]
    assert cut["grad_budget"] == c.n * 2.0 ** -20
    assert err <= cut["grad_err_bound"] <= cut["grad_budget"]
    assert cut["grad_err_bound"] > 0.0
    for k in SCALARS + ("n",):
        assert cut[k] == dense[k], k
    assert np.array_equal(cut["grad"][1:], dense["grad"][1:])
    assert np.array_equal(cut["loo_mean"], dense["loo_mean"]) and np.array_equal(cut["loo_var"], dense["loo_var"])
    # the small case is too tight for any pair to be sqrt(2) l apart in a droppable way
    s = cases["one_tile_row"]
    assert s.cut["pairs_kept"] == s.cut["pairs_total"] and s.cut["grad"][0] == s.dense["grad"][0]


def test_appends_across_a_tile_boundary(dev):
    n0, b, reps = 1000, 9, 3
    n = n0 + b * reps
    x, y, obs = EM.case_data(n, (0.0, 12 * ELL), (0.0, 12 * ELL), ELL, HYPER.noise_level, seed=5)
    gm = TerrainMapper(0, HYPER)
    gm.set_option(N.SBO_OPT_EVIDENCE_BUDGET, 0)                  # every pair: grad[0] at the given-factor tolerance
    gm.fit(x[:n0], y[:n0], obs[:n0])
    epoch_order = gm.order()[:n0].copy()
    for r in range(reps):
        m = n0 + b * (r + 1)
        gm.append(x[m - b:m], y[m - b:m], obs[m - b:m])
        assert np.array_equal(gm.order()[:n0], epoch_order)      # block appends: no re-sort
        got = evidence(gm)
        ref = model_given_factor(gm, x[:m], y[:m], obs[:m])
        d = deviations(got, ref)
        print(f"\n[append] n={m}: " + " ".join(f"{k}={v:.3e}" for k, v in d.items()) + f" grad0={ref['grad'][0]:.4e}")
        assert got["pairs_kept"] == got["pairs_total"] and got["grad_err_bound"] == 0.0
        assert got["n"] == m and got["pairs_total"] == ((m + 63) // 64) * ((m + 63) // 64 + 1) // 2
        assert max(d.values()) <= GIVEN_TOL, d
    # the appended state against a fresh fit of all the points, both under the default budget
    gm.set_option(N.SBO_OPT_EVIDENCE_BUDGET, 20)
    cut = evidence(gm)
    fresh = TerrainMapper(0, HYPER)
    fresh.fit(x, y, obs)
    ref = evidence(fresh)
    d = deviations(cut, ref)
    print(f"\n[append vs fresh fit] n={n}: " + " ".join(f"{k}={v:.3e}" for k, v in d.items()) +
          f"; kept {cut['pairs_kept']} / {ref['pairs_kept']} of {cut['pairs_total']}, bounds "
          f"{cut['grad_err_bound']:.3e} / {ref['grad_err_bound']:.3e}, |d grad0| vs dense "
          f"{abs(cut['grad'][0] - got['grad'][0]):.3e}")
    assert abs(cut["grad"][0] - got["grad"][0]) <= cut["grad_err_bound"] <= cut["grad_budget"]
    assert max(d.values()) <= E2E_TOL, d


def test_states_that_hold_no_evidence(dev, cases):
    c = cases["one_tile_row"]
    gm = TerrainMapper(0, HYPER)
    assert call(gm)[0] == N.SBO_E_STATE                          # before a fit
    gm.set_option(N.SBO_OPT_INVERSE_BITS, 32)
    gm.fit(c.x, c.y, c.obs)
    assert call(gm)[0] == N.SBO_E_STATE                          # no f64 inverse
    gm.set_option(N.SBO_OPT_INVERSE_BITS, 64)
    gm.fit(c.x, c.y, c.obs)
    assert call(gm)[0] == 0
    x = c.x.copy()
    y = c.y.copy()
    x[200], y[200] = x[10], y[10]                                # a duplicated point, no noise: K singular
    bad = TerrainMapper(0, Hyper(noise_level=0.0), ctx=gm.ctx)
    with pytest.raises(N.NotSPDError):
        bad.fit(x, y, c.obs)
    assert call(gm)[0] == N.SBO_E_STATE                          # after a failed fit
    other = TerrainMapper(0, HYPER)
    other.import_state(c.gm.export_state())
    assert other.n == c.n and call(other)[0] == N.SBO_E_STATE    # an imported state holds no factor
    for v in (1, 9, 61, -1):
        with pytest.raises(N.SboError):
            gm.set_option(N.SBO_OPT_EVIDENCE_BUDGET, v)


def test_arguments_and_outputs(dev, cases):
    c = cases["lpsc_box"]
    gm, n = c.gm, c.n
    lib = N.lib()
    assert lib.sbo_evidence(gm.ctx.handle, None, None, None, 0) == 1
    st, info, _, _ = call(gm, loo=False)
    assert st == 0 and info.lml == c.cut["lml"] and info.struct_size == ctypes.sizeof(info)
    # a shorter struct: the bytes past struct_size stay as they were
    size = N.sbo_evidence_info.data_fit.offset
    raw = (ctypes.c_ubyte * ctypes.sizeof(N.sbo_evidence_info))(*([0xA5] * ctypes.sizeof(N.sbo_evidence_info)))
    part = N.sbo_evidence_info.from_buffer(raw)
    part.struct_size = size
    assert lib.sbo_evidence(gm.ctx.handle, ctypes.byref(part), None, None, 0) == 0
    assert part.struct_size == size and part.n == n and part.lml == c.cut["lml"]
    assert bytes(raw[size:]) == b"\xa5" * (ctypes.sizeof(N.sbo_evidence_info) - size)
    # device pointers for the LOO outputs, and one output alone
    dm = torch.full((n,), float("nan"), dtype=torch.float64, device=dev)
    dv = torch.full((n,), float("nan"), dtype=torch.float64, device=dev)
    st, info, _, _ = call(gm, flags=N.SBO_DEVICE_PTRS, mean=dm, var=dv)
    torch.cuda.synchronize()
    assert st == 0
    assert np.array_equal(dm.cpu().numpy(), c.cut["loo_mean"]) and np.array_equal(dv.cpu().numpy(), c.cut["loo_var"])
    only = np.full(n, np.nan)
    assert call(gm, mean=None, var=only)[0] == 0 and np.array_equal(only, c.cut["loo_var"])


def test_reads_only_and_repeats_bitwise(dev, cases):
    c = cases["wide"]
    gm = c.gm
    gx, gy = np.meshgrid(np.linspace(-0.3, 24 * ELL + 0.3, 37), np.linspace(-0.3, 24 * ELL + 0.3, 29))
    qx, qy = gx.reshape(-1).astype(np.float32), gy.reshape(-1).astype(np.float32)
    f_min = float(np.percentile(c.obs, 40.0))

    def tick():
        m = qx.size
        outs = dict(mu=np.empty(m, np.float32), sd=np.empty(m, np.float32), lo=np.empty(m, np.float64),
                    hi=np.empty(m, np.float64), safe=np.empty(m, np.uint8))
        key = gm.tick(qx, qy, 2.0, f_min, outputs=outs)
        return outs, (key.score, key.idx)

    def same(a, b):
        for k in SCALARS + ("n", "pairs_kept", "pairs_total", "grad_err_bound", "grad_budget", "dropped"):
            assert a[k] == b[k], k
        for k in ("grad", "loo_mean", "loo_var"):
            assert np.array_equal(a[k], b[k]), k

    before, key0 = tick()
    first = evidence(gm)
    same(first, c.cut)                         # (the fixture's call: two calls agree bitwise)
    same(evidence(gm), first)
    gm.trim()
    same(evidence(gm), first)                  # the workspace comes back
    after, key1 = tick()
    assert key0 == key1
    for k in before:
        assert np.array_equal(before[k], after[k]), k
    L0, a0 = c.gm.factor()
    evidence(gm)
    L1, a1 = c.gm.factor()
    assert np.array_equal(L0, L1) and np.array_equal(a0, a1)


# ---------------------------------------------------------------- fit_hyper
def prior_draw(n=400, seed=11, ell=0.5, sf=1.3, noise=0.05, side=6.0):
    u = uniform(seed, 2 * n)
    x = np.ascontiguousarray(u[0::2] * side, np.float32)
    y = np.ascontiguousarray(u[1::2] * side, np.float32)
    Kf, _ = EM.kernel(x, y, ell, sf * sf)
    f = np.linalg.cholesky(Kf + 1e-10 * np.eye(n)) @ normal(seed + 1, n)
    return x, y, np.ascontiguousarray(f + np.sqrt(noise) * normal(seed + 2, n), np.float32)


def test_fit_hyper_reaches_the_models_optimum(dev):
    from scipy.optimize import minimize
    truth, start = (0.5, 1.3, 0.05), (1.0, 1.0, 0.2)
    x, y, obs = prior_draw()
    bounds = [(v / 20.0, v * 20.0) for v in start]
    lml = lambda h: EM.evidence(x, y, obs, *h)["lml"]  # noqa: E731

    def neg(theta):
        e = EM.evidence(x, y, obs, *np.exp(theta))
        return -e["lml"], -e["grad"][:3]

    res = minimize(neg, np.log(start), jac=True, method="L-BFGS-B", bounds=[tuple(np.log(b)) for b in bounds],
                   options={"maxiter": 50})
    best = -res.fun
    gm = TerrainMapper(0, Hyper(*start))
    h = gm.fit_hyper(x, y, obs, max_iter=50)
    got = lml((h.length_scale, h.sigma_f, h.noise_level))
    print(f"\n[fit_hyper] device ({h.length_scale:.5f}, {h.sigma_f:.5f}, {h.noise_level:.5f}) lml {got:.6f}; "
          f"model {tuple(np.round(np.exp(res.x), 5))} lml {best:.6f} in {res.nfev} evaluations; "
          f"truth lml {lml(truth):.6f}; start lml {lml(start):.6f}; below the optimum by {best - got:.3e}")
    assert h == gm.hyper and gm.n == x.size
    e = gm.evidence()
    assert abs(e["lml"] - got) <= E2E_TOL * abs(got)           # left fitted at the returned values
    assert got >= best - DELTA
    assert got > lml(truth)

"""The fast / precise sweep decision where it is made: at its threshold, under
appends that do not reach a re-probe, and on a training sample that has to
span the stored points (the figures in
profiles/probe_decision.log).

Every reference is the fp64 oracle given the device's own factor
(oracle_given_factor for the default tick; oracle_given_factor64 has the same
variance -- sigma^2 depends on the factor alone -- and is the reference the
precise sweep's recorded sigma^2 error is taken against).  The precise sweep
is printed beside the oracle, never used as one.  Every fit has N <= 2048 and
a 96 x 96 grid.

  1. Three ladders carry the probe's reading across kPreciseTol = 5e-6: the
     lpsc box with N rising, C2-like data with the fitted length scale rising,
     and the same at sn2 = 0.01.  Every rung: the default tick meets the 1e-5
     contract over the whole grid and on a near-data sample, whichever sweep
     the probe chose; the verdict is (err > 5e-6); where it is "precise" the
     forced fast sweep is measurably worse.  Each ladder must hold two fast
     rungs in [2.5e-6, 5e-6] and two precise ones in (5e-6, 1e-5].
  2. The highest fast rung of the box and the length-scale ladder, then 24 %
     more points in batches of 16 (below SBO_OPT_REPROBE and SBO_OPT_RESORT:
     the verdict stands): uniform appends and appends into one l x l square.
     The contract after 8, 16 and 24 %, through sbo_tick and through the
     streaming tick's update path.
  3. Box data with 150 exact duplicates of one location at either end of the
     stored order, n in {700, 1000, 1500}: the probe's smallest variance must
     see the cluster wherever it is stored.

Set SBO_PROBE_DECISION_LOG to a file name to have every printed figure appended
to it (how profiles/probe_decision.log was written).
"""
import dataclasses
import math
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from safe_bayesian_optimization_amd import TerrainMapper, synthetic  # noqa: E402
from safe_bayesian_optimization_amd import _native as N  # noqa: E402
from safe_bayesian_optimization_amd.terrain import Hyper, more_points, normal, smooth_field  # noqa: E402
from safe_bayesian_optimization_amd.terrain import synthetic_box, uniform  # noqa: E402

from test_gpu_headline import REL_TOL, f32, full_outputs, host, nrel, oracle_given_factor  # noqa: E402
from test_gpu_parity import oracle_given_factor64  # noqa: E402
from test_gpu_precision import near_data_sample  # noqa: E402

PRECISE_TOL = 5e-6   # kPreciseTol (csrc/sbo_api.cpp), as include/sbo.h documents it
GRID = 96

# The rungs (chosen on an MI355X so that each ladder brackets the threshold:
# profiles/probe_decision.log has every reading).
LADDERS = {
    # synthetic_box(n, 96, 96), default hyper-parameters
    "box": (192, 256, 288, 320, 352, 384, 448, 512, 640, 768),
    # synthetic(2048, 96, 96) (generated at l = 0.4), fitted with l'
    "len": (0.4, 0.4416, 0.4876, 0.512, 0.5383, 0.5895, 0.5944, 0.6563, 0.7246, 0.8),
    # the same data, sn2 = 0.01, fitted with l'
    "low": (0.2, 0.2208, 0.2438, 0.2692, 0.2786, 0.2972, 0.305, 0.3281, 0.3623, 0.4),
}
RUNGS = [(fam, knob) for fam, knobs in LADDERS.items() for knob in knobs]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def record(line):
    print(line)
    path = os.environ.get("SBO_PROBE_DECISION_LOG")
    if path:
        with open(path, "a") as f:
            f.write(line + "\n")


def ladder_workload(family, knob):
    """(the workload as generated, the workload as fitted)."""
    if family == "box":
        wl = synthetic_box(int(knob), GRID, GRID)
        return wl, wl
    gen = synthetic(2048, GRID, GRID)
    hyper = Hyper(length_scale=float(knob), noise_level=0.01 if family == "low" else 0.1)
    return gen, dataclasses.replace(gen, hyper=hyper)


def fitted(wl, dev):
    t = lambda a: torch.tensor(f32(a), device=dev)  # noqa: E731
    gm = TerrainMapper(0, wl.hyper)
    gm.fit(t(wl.x), t(wl.y), t(wl.obs))
    return gm


def tick_host(gm, wl, qx, qy, dev):
    """One sbo_tick over (qx, qy): its outputs on the host."""
    t = lambda a: torch.tensor(f32(a), device=dev)  # noqa: E731
    outs = full_outputs(qx.size, dev)
    gm.tick(t(qx), t(qy), wl.beta, wl.f_min, outputs=outs)
    torch.cuda.synchronize()
    return host(outs)


def contract_errors(h, sel, hs, omu, ovar):
    """The section-1 contract's four figures: mu and sigma^2 over the whole
    grid (outputs h), and over the near-data sample sel (outputs hs, of the
    sample's own points in sel's order) with sigma^2 normalised by the whole
    grid's largest variance."""
    var = lambda o: o["sd"].astype(np.float64) ** 2  # noqa: E731
    return dict(mu=nrel(h["mu"], omu), var=nrel(var(h), ovar), near_mu=nrel(hs["mu"], omu[sel]),
                near_var=float(np.abs(var(hs) - ovar[sel]).max() / np.abs(ovar).max()))


def near_sample(wl, seed):
    """Up to 2048 grid points within half a length scale of a training point:
    docs/DESIGN_HISTORY.md 5a puts the fast sweep's worst points 0.05-0.5 l
    from the nearest one."""
    return near_data_sample(wl, 2048, 0.5 * wl.hyper.length_scale, seed)


def default_contract(gm, wl, dev, seed):
    """The default tick over the whole grid and over the near-data sample (a
    tick of its own) against the oracle given the factor; also returns the
    oracle's (mu, var)."""
    omu, ovar = oracle_given_factor(gm, wl, wl.qx, wl.qy)
    sel = near_sample(wl, seed)
    h = tick_host(gm, wl, wl.qx, wl.qy, dev)
    hs = tick_host(gm, wl, wl.qx[sel], wl.qy[sel], dev)
    return contract_errors(h, sel, hs, omu, ovar), (omu, ovar)


def assert_contract(e, what):
    assert e["mu"] < REL_TOL and e["var"] < REL_TOL, (what, e)
    assert e["near_mu"] < REL_TOL and e["near_var"] < REL_TOL, (what, e)


def fmt(e):
    return " ".join(f"{k} {v:.2e}" for k, v in e.items())


# ------------------------------------------------- 1. ladders across the threshold
_rungs = {}


def rung(dev, family, knob):
    """One rung's readings, measured once per session: the probe, the default
    tick's contract errors, and the forced fast and forced precise sweeps'
    whole-grid sigma^2 errors, all against the oracle given the factor."""
    if (family, knob) in _rungs:
        return _rungs[family, knob]
    _, wl = ladder_workload(family, knob)
    gm = fitted(wl, dev)
    try:
        pi = gm.probe_info()
        in_effect = gm.precision()[0]
        e, (_, ovar) = default_contract(gm, wl, dev, seed=17)
        forced = {}
        for name, opt in (("fast", 0), ("precise", 1)):
            gm.set_option(N.SBO_OPT_PRECISION, opt)
            assert gm.precision()[0] == bool(opt)
            forced[name] = nrel(tick_host(gm, wl, wl.qx, wl.qy, dev)["sd"].astype(np.float64) ** 2, ovar)
        gm.set_option(N.SBO_OPT_PRECISION, -1)
        assert gm.precision()[0] == in_effect and gm.probe_info() == pi   # the readings outlive the forcing
        if family == "box" and knob == LADDERS["box"][0]:
            # sigma^2 has one reference: the f64-alpha oracle's variance is the same array
            assert np.array_equal(oracle_given_factor64(gm, wl, wl.qx, wl.qy)[1], ovar)
    finally:
        gm.close()
    r = dict(family=family, knob=knob, n=wl.x.size, probe=pi, in_effect=in_effect, default=e, fast=forced["fast"],
             precise=forced["precise"])
    record(f"ladder {family} {knob:g} (N={wl.x.size}): probe err {pi['err']:.3e} grid {pi['err_grid']:.3e} train "
           f"{pi['err_train']:.3e} -> {'precise' if pi['precise'] else 'fast'}; whole grid var vs oracle: forced fast "
           f"{r['fast']:.3e} forced precise {r['precise']:.3e}; fast / probe {r['fast'] / pi['err']:.2f}; "
           f"default tick: {fmt(e)}")
    _rungs[family, knob] = r
    return r


@pytest.mark.parametrize("family,knob", RUNGS, ids=[f"{f}-{k:g}" for f, k in RUNGS])
def test_ladder_rung(dev, family, knob):
    """One rung, default options: the contract whichever sweep the probe chose;
    the verdict is the documented rule; a "precise" verdict changed something."""
    r = rung(dev, family, knob)
    assert_contract(r["default"], (family, knob))
    assert bool(r["probe"]["precise"]) == (r["probe"]["err"] > PRECISE_TOL)
    assert r["in_effect"] == bool(r["probe"]["precise"])
    if r["probe"]["precise"]:
        assert r["fast"] > r["default"]["var"], r


@pytest.mark.parametrize("family", list(LADDERS))
def test_ladder_brackets_threshold(dev, family):
    """The ladder is not vacuous: two rungs just under the threshold that keep
    the fast sweep, two just over it that switch."""
    assert len(LADDERS[family]) <= 10
    rs = [rung(dev, family, k)["probe"] for k in LADDERS[family]]
    under = [p["err"] for p in rs if not p["precise"] and 2.5e-6 <= p["err"] <= 5e-6]
    over = [p["err"] for p in rs if p["precise"] and 5e-6 < p["err"] <= 1e-5]
    record(f"ladder {family}: fast rungs in [2.5e-6, 5e-6]: {len(under)}, precise rungs in (5e-6, 1e-5]: {len(over)}")
    assert len(under) >= 2 and len(over) >= 2, [p["err"] for p in rs]


# ------------------------------------------------------ 2. a verdict that goes stale
def appended_points(gen, fit, k, shape, seed):
    """k further measurements of the generating workload's own field: uniform
    over the training box (more_points where it applies), or all inside one
    l x l square at the box's centre -- the robot working one spot."""
    if shape == "uniform" and gen.side is not None:
        return more_points(gen, k, seed=seed)
    u = uniform(seed ^ 0xADD, 2 * k)
    x0, x1, y0, y1 = gen.x.min(), gen.x.max(), gen.y.min(), gen.y.max()
    if shape == "uniform":
        x, y = x0 + u[0::2] * (x1 - x0), y0 + u[1::2] * (y1 - y0)
    else:
        ell = fit.hyper.length_scale
        x, y = 0.5 * (x0 + x1) + (u[0::2] - 0.5) * ell, 0.5 * (y0 + y1) + (u[1::2] - 0.5) * ell
    side = gen.side if gen.side is not None else 2.5   # synthetic_box's field square (its box starts at 0, 0)
    h = gen.hyper
    obs = smooth_field(x, y, side, h.length_scale, gen.seed) + math.sqrt(h.sn2) * normal(seed + 7, k)
    return x, y, obs


@pytest.mark.parametrize("shape", ["uniform", "one_spot"])
@pytest.mark.parametrize("family", ["box", "len"])
def test_stale_verdict_under_appends(dev, family, shape):
    """The highest rung that kept the fast sweep, grown by 24 % in batches of
    16: no append re-probes or re-sorts, so the fit's verdict stands.  After
    8, 16 and 24 % the contract against the oracle of the appended factor,
    through sbo_tick and through the streaming tick, which must have taken its
    update path after every batch.  Then one more batch with SBO_OPT_REPROBE 0:
    the fresh reading beside the stale one (recorded)."""
    knob = next(k for k in reversed(LADDERS[family]) if not rung(dev, family, k)["probe"]["precise"])
    gen, wl = ladder_workload(family, knob)
    n0, batch = wl.x.size, 16
    total = int(0.24 * n0)
    marks = [int(round(0.08 * n0)), int(round(0.16 * n0)), total]
    ax, ay, aobs = appended_points(gen, wl, total + batch, shape, seed=31)
    X, Y, OBS = np.concatenate([wl.x, ax]), np.concatenate([wl.y, ay]), np.concatenate([wl.obs, aobs])
    t = lambda a: torch.tensor(f32(a), device=dev)  # noqa: E731
    Xd, Yd, Od, qx, qy = t(X), t(Y), t(OBS), t(wl.qx), t(wl.qy)
    gm = TerrainMapper(0, wl.hyper)
    try:
        gm.fit(Xd[:n0], Yd[:n0], Od[:n0])
        stale = gm.probe_info()
        assert not stale["precise"] and stale["n_at_probe"] == n0
        souts = full_outputs(qx.numel(), dev)
        gm.tick_stream(qx, qy, wl.beta, wl.f_min, outputs=souts)
        assert gm.stream_info()["reason"] == "FIRST"
        n = n0
        while n < n0 + total:
            b = min(batch, n0 + total - n)
            gm.append(Xd[n:n + b], Yd[n:n + b], Od[n:n + b])
            n += b
            assert gm.probe_info()["n_at_probe"] == n0 and not gm.precision()[0]
            gm.tick_stream(qx, qy, wl.beta, wl.f_min, outputs=souts)
            info = gm.stream_info()
            assert (info["path"], info["reason"], info["rows"]) == (1, "UPDATED", b), info
            if n - n0 < marks[0]:
                continue
            marks.pop(0)
            torch.cuda.synchronize()
            cur = dataclasses.replace(wl, x=X[:n], y=Y[:n], obs=OBS[:n])
            e, (omu, ovar) = default_contract(gm, cur, dev, seed=n)
            hs = host(souts)
            sel = near_sample(cur, n)
            es = contract_errors(hs, sel, {k: v[sel] for k, v in hs.items()}, omu, ovar)
            record(f"stale {family} {knob:g} {shape}: N {n0} -> {n} (+{100.0 * (n - n0) / n0:.1f} %), probe of N={n0} "
                   f"err {stale['err']:.3e}; tick: {fmt(e)}; stream update: {fmt(es)}")
            assert_contract(e, (family, shape, n, "tick"))
            assert_contract(es, (family, shape, n, "tick_stream"))
        assert not marks and gm.n == n0 + total
        gm.set_option(N.SBO_OPT_REPROBE, 0)
        gm.append(Xd[n:n + batch], Yd[n:n + batch], Od[n:n + batch])
        fresh = gm.probe_info()
        assert fresh["n_at_probe"] == n0 + total + batch == gm.n
        record(f"stale {family} {knob:g} {shape}: stale probe (N={n0}) err {stale['err']:.3e} -> fast; fresh probe "
               f"(N={gm.n}) err {fresh['err']:.3e} grid {fresh['err_grid']:.3e} train {fresh['err_train']:.3e} -> "
               f"{'precise' if fresh['precise'] else 'fast'}")
    finally:
        gm.close()


# ------------------------------------- 3. the training sample spans the stored points
DUPLICATES = 150


@pytest.mark.parametrize("end", ["low", "high"])
@pytest.mark.parametrize("n", [700, 1000, 1500])
def test_probe_sample_spans_stored_points(dev, n, end):
    """The publisher's dwells: 150 of n box points are exact duplicates of one
    location, at the low or the high end of the box's longer side -- in the
    k-d order the head or the tail of the stored points.  The variance there
    (0.1 / 150 at sn2 = 0.1) is the smallest anywhere, and a sample that
    strides over all n positions with a stride <= 3 lands in the run of 150:
    the probe's var_min must see it.  A sample of positions 0 ... 511 (n / 512)
    never reaches the tail.  l = 0.2 (fp64, host): the smallest variance at
    any other training point is 5 to 10 x the cluster's at these n, so a
    var_min within 2 x of the cluster's can only come from the cluster (at
    l = 0.4 the rest of the n = 1500 data is dense enough to come within
    1.96 x, and the assertion would pass without the tail)."""
    wl = synthetic_box(n, GRID, GRID, seed=n, hyper=Hyper(length_scale=0.2))
    by_y = np.argsort(wl.y)
    dup = by_y[-DUPLICATES:] if end == "high" else by_y[:DUPLICATES]
    at = by_y[-1] if end == "high" else by_y[0]     # the extreme point: the training box stays
    x, y = wl.x.copy(), wl.y.copy()
    x[dup], y[dup] = x[at], y[at]
    wl = dataclasses.replace(wl, x=x, y=y)
    gm = fitted(wl, dev)
    try:
        # where the duplicates sit in the stored order, against the positions
        # the floor stride n / 512 reaches
        pos = np.flatnonzero(np.isin(gm.order(), dup))
        reach = 511 * (n // 512)
        assert pos.size == DUPLICATES
        assert (pos.max() <= reach) if end == "low" else (pos.min() > reach), (pos.min(), pos.max(), reach)
        pi = gm.probe_info()
        _, ovar_at = oracle_given_factor(gm, wl, x[[at]], y[[at]])
        e, _ = default_contract(gm, wl, dev, seed=n)
        record(f"span n={n} {end}: duplicates at stored positions {pos.min()}..{pos.max()}, floor stride reaches "
               f"{reach}; m_train {pi['m_train']}; var_min {pi['var_min']:.3e}, oracle at the duplicates {ovar_at[0]:.3e} "
               f"(ratio {pi['var_min'] / ovar_at[0]:.2f}); probe err {pi['err']:.3e} -> "
               f"{'precise' if pi['precise'] else 'fast'}; default tick: {fmt(e)}")
        assert pi["var_min"] <= 2.0 * ovar_at[0]
        assert_contract(e, (n, end))
        stride = -(-n // 512)
        assert pi["m_train"] == -(-(n - stride // 2) // stride)     # [0, n) at the ceiling stride
    finally:
        gm.close()

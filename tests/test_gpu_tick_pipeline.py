"""Two corners of the tick pipeline (csrc/sbo_api.cpp: run_tick over a TickPlan)
that no other test reaches: what a plan-only or cost request does on a context
whose ticks run the precise sweep in chunks and in item blocks.

N = 600 on the lpsc box (3 row blocks) and a ragged 40 x 33 raster (1320
queries, 11 query blocks); SBO_OPT_TABLE_MB 1 holds the K* table of two query
blocks at this N (12 k-tiles x 34304 B each), so the tick runs in six chunks.
"""
import ctypes

import numpy as np
import pytest
from scipy.linalg import solve_triangular

from oracle import oracle as O
from safe_bayesian_optimization_amd import TerrainMapper
from safe_bayesian_optimization_amd import _native as N
from safe_bayesian_optimization_amd.terrain import synthetic_box

pytestmark = pytest.mark.gpu

PLAN_BLOCK = 2 << 8 | 4


def f32(a):
    return np.ascontiguousarray(a, np.float32)


def nrel(a, b):
    return float(np.abs(np.asarray(a, np.float64) - b).max() / np.abs(b).max())


def debug_plan(gm, qx, qy):
    lib = N.lib()
    n = ctypes.c_int64(0)
    gm.ctx.check(lib.sbo_debug_plan(gm.ctx.handle, qx.ctypes.data, qy.ctypes.data, qx.size, None, 0, ctypes.byref(n)))
    buf = np.empty(n.value, np.int32)
    gm.ctx.check(lib.sbo_debug_plan(gm.ctx.handle, qx.ctypes.data, qy.ctypes.data, qx.size, buf.ctypes.data, buf.size,
                                    ctypes.byref(n)))
    return buf


@pytest.fixture(scope="module")
def box():
    """The fitted context (the probe has run; the precise sweep in effect), the
    queries, and the fp64 oracle's posterior from the device's own factor with
    alpha solved in f64 (what the precise sweep targets)."""
    wl = synthetic_box(600, 40, 33, seed=600)
    gm = TerrainMapper(0, wl.hyper)
    gm.set_option(N.SBO_OPT_PRECISION, 1)
    gm.set_option(N.SBO_OPT_TABLE_MB, 1)
    gm.fit(wl.x, wl.y, wl.obs)
    precise, perr, _, _ = gm.precision()
    print(f"lpsc box N=600: precise={precise}, the probe's fast-sweep error {perr:.2e}")
    assert precise and perr >= 0.0
    L, _ = gm.factor()
    o = gm.order()
    L64 = L.astype(np.float64)
    h = wl.hyper
    r = f32(wl.obs)[o].astype(np.float64) - h.prior_mean
    alpha = solve_triangular(L64.T, solve_triangular(L64, r, lower=True), lower=False)
    qx, qy = f32(wl.qx), f32(wl.qy)
    omu, ovar = O.predict(O.colmajor_from_lower(L64), alpha, f32(wl.x)[o], f32(wl.y)[o], qx, qy, h.length_scale,
                          h.sf2, h.prior_mean)
    omu.setflags(write=False)
    ovar.setflags(write=False)
    yield gm, wl, qx, qy, omu, ovar
    gm.close()


def test_query_cost_ignores_plan_block(box):
    """sbo_query_cost's plan is row-block-major by rule: SBO_OPT_PLAN_BLOCK,
    which reorders the precise tick's items, leaves the cost bitwise as it is."""
    gm, wl, qx, qy, _, _ = box
    c0 = np.asarray(gm.query_cost(qx, qy)).copy()
    gm.set_option(N.SBO_OPT_PLAN_BLOCK, PLAN_BLOCK)
    try:
        c1 = np.asarray(gm.query_cost(qx, qy)).copy()
        p1 = debug_plan(gm, qx, qy)
    finally:
        gm.set_option(N.SBO_OPT_PLAN_BLOCK, 0)
    assert c0.dtype == np.float32 and c0.shape == (1320,) and c0.max() > 0
    assert np.array_equal(c0.view(np.uint32), c1.view(np.uint32))
    assert np.array_equal(p1, debug_plan(gm, qx, qy))


@pytest.mark.parametrize("plan_block", [0, PLAN_BLOCK])
def test_debug_plan_around_a_chunked_tick(box, plan_block):
    """sbo_debug_plan right after a chunked precise tick (whose last chunk's
    plan sits in the workspace) is sbo_debug_plan before it; the tick itself
    is within 1e-5 of the fp64 oracle in sigma^2 and mu."""
    gm, wl, qx, qy, omu, ovar = box
    gm.set_option(N.SBO_OPT_PLAN_BLOCK, plan_block)
    try:
        before = debug_plan(gm, qx, qy)
        mu, sd = gm.predict(qx, qy)
        after = debug_plan(gm, qx, qy)
    finally:
        gm.set_option(N.SBO_OPT_PLAN_BLOCK, 0)
    assert before[0] == 3 and before[1] >= 11 and before[2] > 0       # row blocks, query blocks, kept tiles
    assert np.array_equal(before, after)
    emu, evar = nrel(mu, omu), nrel(sd.astype(np.float64) ** 2, ovar)
    print(f"chunked precise tick, plan block {plan_block}: mu {emu:.2e} var {evar:.2e}")
    assert emu < 1e-5 and evar < 1e-5

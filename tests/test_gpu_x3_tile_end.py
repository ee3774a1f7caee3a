"""The split sweep's tile end (csrc/predict_x3_rowhalf.hpp: x3_tile_end, the
K* hand-over and the item end) on a plan that walks many items back to back:
the R = 0 chains handed across the step barrier, the zeroing of the outer
sums between items, items of no, one and many tiles -- bit for bit against the
diagnostic build's k-half predecessor (variant 62) at every precision level
and at 1, 3, 8 and the default number of sweep groups."""
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import oracle as O
from safe_bayesian_optimization_amd import TerrainMapper, synthetic
from safe_bayesian_optimization_amd import _native as N

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_TRAIN, N_NEAR, N_FAR = 1100, 1500, 44     # five row blocks (the last ragged); 12 query blocks + the far one
GROUPS = (1, 3, 8, 0)                       # SBO_OPT_SWEEP_GROUPS (0: the default, one per CU)
FORCES = (None, 0, 1, 2)                    # SBO_LVL_FORCE (diagnostic build only)
WEIGHTS = (33 / 64, 42 / 64, 1.0)           # sbo_query_cost's tile weights at one, three, six product(s)

CHILD = r'''
import os, sys, numpy as np
sys.path.insert(0, {root!r})
from safe_bayesian_optimization_amd import TerrainMapper
from safe_bayesian_optimization_amd import _native as N
d = np.load({inp!r})
from safe_bayesian_optimization_amd.terrain import Hyper
gm = TerrainMapper(0, Hyper())
gm.set_option(N.SBO_OPT_PRECISION, 0)    # the split sweep, whatever the probe would choose
gm.fit(d["x"], d["y"], d["obs"])
out = {{}}
L, alpha = gm.factor()
out["L"], out["alpha"], out["order"] = L, alpha, gm.order()
out["cost"] = np.asarray(gm.query_cost(d["qx"], d["qy"]))    # the default plan of variant 3
for force in {forces!r}:
    if force is None:
        os.environ.pop("SBO_LVL_FORCE", None)
    else:
        os.environ["SBO_LVL_FORCE"] = str(force)
    for groups in {groups!r}:
        gm.set_option(N.SBO_OPT_SWEEP_GROUPS, groups)
        for v in {variants!r}:
            gm.set_option(N.SBO_OPT_KERNEL_VARIANT, v)
            mu, sd = gm.predict(d["qx"], d["qy"])
            out["mu_%s_%d_%d" % (force, groups, v)] = np.asarray(mu)
            out["sd_%s_%d_%d" % (force, groups, v)] = np.asarray(sd)
gm.close()
np.savez({path!r}, **out)
'''


def _child(lib, inp, path, forces, variants):
    env = dict(os.environ, SBO_LIB=lib)
    env.pop("SBO_LVL_FORCE", None)
    r = subprocess.run([sys.executable, "-c", CHILD.format(root=ROOT, inp=inp, path=path, forces=list(forces),
                                                          groups=list(GROUPS), variants=list(variants))],
                       env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    return dict(np.load(path))


def _block_tiles(cost):
    """Kept tiles of every query block that can be told apart in
    sbo_query_cost's output: cost = the block's kept tiles over all its items,
    weighted 1, 42/64, 33/64 by level, / the block's size, the same for every
    query of the block.  Queries are grouped by their cost; a group is a block
    if it has a block's size (128, or the last block's M % 128).  Returns the
    tile count per such block where every tile has one weight (0 for an empty
    block), -1 where a mix has no single answer."""
    cost = np.asarray(cost, np.float64)
    sizes = {128, cost.size % 128}
    tiles = []
    for c in np.unique(cost):
        n = int(np.sum(cost == c))
        if n not in sizes:
            continue
        total, t = c * n, -1
        for w in WEIGHTS:
            k = total / w
            if abs(k - round(k)) < 1e-4:
                t = int(round(k))
                break
        tiles.append(t)
    return tiles


def test_tile_end_every_level_and_group_count(tmp_path):
    """N = 1100 (five row blocks, the last ragged), M = 1500 + 44: a 50 x 30
    grid over the data and 44 queries beyond its corner, which the sweep's
    order puts last.  The twelve blocks over the data keep many tiles per
    item; the far queries' own block is moved out (scanning sbo_query_cost,
    the plan alone) to the distance at which it keeps exactly one tile: one
    item of a single tile, and, with five row blocks, empty items beside it.
    At one sweep group a single workgroup walks every item back to back.

    Bit for bit: the product against the diagnostic build's variant 3 (one
    kernel from one header) under the default plan; variant 3 against the
    k-half predecessor (variant 62) under the default plan and with every
    tile forced to six, three and one product(s), at every group count; and
    every group count against every other.  The default plan keeps the 1e-5
    contract against the fp64 oracle."""
    prod = os.path.join(ROOT, "safe_bayesian_optimization_amd", "lib", "libsbo.so")
    diag = os.path.join(ROOT, "safe_bayesian_optimization_amd", "lib", "libsbo_diag.so")
    assert os.path.exists(diag), "lib/libsbo_diag.so not built (make -C safe_bayesian_optimization_amd diag)"
    wl = synthetic(N_TRAIN, 50, 30, seed=31)
    assert wl.qx.size == N_NEAR
    side, ls = float(wl.qx.max()), wl.hyper.length_scale
    rng = np.random.default_rng(7)
    ux, uy = rng.random(N_FAR), rng.random(N_FAR)

    def queries(dist):
        return (np.concatenate([wl.qx, side + ls * (dist + ux)]).astype(np.float32),
                np.concatenate([wl.qy, side + ls * (dist + uy)]).astype(np.float32))

    # the distance (in length scales beyond the data's corner) at which a
    # block keeps one tile: the first of the scan, the plan being monotone in it
    gm = TerrainMapper(0, wl.hyper)
    try:
        gm.set_option(N.SBO_OPT_PRECISION, 0)
        gm.fit(wl.x, wl.y, wl.obs)
        dist = next((t for t in np.arange(1.0, 8.0, 1.0 / 32) if 1 in _block_tiles(gm.query_cost(*queries(t)))), None)
    finally:
        gm.close()
    assert dist is not None, "no distance at which a far query block keeps exactly one tile"
    print(f"far queries at {dist:.5f} length scales: a block of one kept tile")
    qx, qy = queries(dist)
    assert qx.size == N_NEAR + N_FAR
    inp = str(tmp_path / "in.npz")
    np.savez(inp, x=wl.x, y=wl.y, obs=wl.obs, qx=qx, qy=qy)
    p = _child(prod, inp, str(tmp_path / "prod.npz"), [None], [3])
    d = _child(diag, inp, str(tmp_path / "diag.npz"), FORCES, [3, 62])
    # the plan each library swept holds a one-tile item and (its block's four
    # other row blocks) empty items, beside blocks of many tiles
    for res in (p, d):
        tiles = _block_tiles(res["cost"])
        print("kept tiles per block:", tiles)
        assert 1 in tiles and (N_TRAIN + 255) // 256 == 5
        assert max(tiles) > 5 or -1 in tiles
    assert np.array_equal(p["cost"], d["cost"])
    for g in GROUPS:
        for k in ("mu", "sd"):
            assert np.array_equal(p[f"{k}_None_{g}_3"], d[f"{k}_None_{g}_3"]), (k, g)
            assert np.array_equal(p[f"{k}_None_{g}_3"], p[f"{k}_None_{GROUPS[0]}_3"]), (k, g)
    for force in FORCES:
        for g in GROUPS:
            for k in ("mu", "sd"):
                a, b = d[f"{k}_{force}_{g}_3"], d[f"{k}_{force}_{g}_62"]
                assert np.array_equal(a, b), (k, force, g, int(np.sum(a != b)))
                assert np.array_equal(a, d[f"{k}_{force}_{GROUPS[0]}_3"]), (k, force, g)
    # the forced levels are different computations, not one result three times
    assert not np.array_equal(d["sd_0_1_3"], d["sd_2_1_3"])
    # the fp64 oracle given the device factor
    o = p["order"]
    Lcm = O.colmajor_from_lower(p["L"].astype(np.float64))
    omu, ovar = O.predict(Lcm, p["alpha"].astype(np.float64), wl.x.astype(np.float32)[o], wl.y.astype(np.float32)[o],
                          qx, qy, wl.hyper.length_scale, wl.hyper.sf2, wl.hyper.prior_mean)
    for name, res in (("product", p), ("diagnostic", d)):
        for g in GROUPS:
            gmu = res[f"mu_None_{g}_3"].astype(np.float64)
            gvar = res[f"sd_None_{g}_3"].astype(np.float64) ** 2
            emu = np.abs(gmu - omu).max() / np.abs(omu).max()
            evar = np.abs(gvar - ovar).max() / np.abs(ovar).max()
            print(f"{name}, groups {g}: mu_err={emu:.2e} var_err={evar:.2e}")
            assert emu < 1e-5 and evar < 1e-5, (name, g, emu, evar)

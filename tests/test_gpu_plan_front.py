"""The tick's plan builder (csrc/kernels.hip: plan_count_kernel with the column
prefilter, the flat water-filling totals and the cheap-row-block shortcut; the
list chain; the acquisition that skips empty items) against the diagnostic
build's reference builder (SBO_PLAN_REF=1: every (row block, k-tile) pair's
bounds evaluated in every pass, empty items' partials written and read).

The plan is compared through sbo_debug_plan (include/sbo.h): the kept tiles
with their levels, and every item's threshold and kept count, must be the same
arrays; the tick's outputs the same bytes.  Each library runs all cases in one
child process of its own (SBO_LIB).

The prefilter's t >= kPlanD2 branch needs N > 131072 and is not covered."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import oracle as O
from safe_bayesian_optimization_amd import TerrainMapper, synthetic
from safe_bayesian_optimization_amd import _native as N
from safe_bayesian_optimization_amd.terrain import Hyper

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HYPER = dict(length_scale=0.4, sigma_f=1.5, noise_level=0.1, prior_mean=0.25)   # sqrt(sf2) = 1.5 exactly
FAR = 40.0    # length scales


def queries(wl, kind):
    """Query sets over a workload's square [0, side]^2 (length scale ls)."""
    side, ls = float(wl.side), wl.hyper.length_scale
    if kind == "raster":      # 40 x 30 inside the training box: 1200 queries, the last block partial
        gy, gx = np.meshgrid(np.linspace(0.1 * side, 0.9 * side, 30), np.linspace(0.1 * side, 0.9 * side, 40),
                             indexing="ij")
        return gx.reshape(-1), gy.reshape(-1)
    if kind == "scatter":     # 1000 scattered points: no grid, the Morton path
        rng = np.random.default_rng(17)
        return rng.random(1000) * side, rng.random(1000) * side
    if kind == "straddle":    # a raster from inside the data to FAR length scales beyond its edge
        gy, gx = np.meshgrid(np.linspace(0.0, side, 30), np.linspace(0.5 * side, side + FAR * ls, 40), indexing="ij")
        return gx.reshape(-1), gy.reshape(-1)
    if kind == "far":         # the raster's shape, FAR length scales from every training point
        gy, gx = np.meshgrid(np.linspace(0.0, side, 30), np.linspace(side + FAR * ls, 2 * side + FAR * ls, 40),
                             indexing="ij")
        return gx.reshape(-1), gy.reshape(-1)
    if kind == "mixed":       # scattered far points with one block's worth of near ones among them
        rng = np.random.default_rng(23)
        qx = side + FAR * ls + rng.random(1200) * side
        qy = rng.random(1200) * side
        qx[512:640] = 0.4 * side + rng.random(128) * 0.2 * side
        qy[512:640] = 0.4 * side + rng.random(128) * 0.2 * side
        return qx, qy
    if kind == "first256":
        qx, qy = queries(wl, "raster")
        return qx[:256], qy[:256]
    raise ValueError(kind)


# One context per library walks these steps in order, so every tick meets the
# workspace the ticks before it left: ("opt", options) sets options (the skip
# budget takes effect at the next fit), ("fit", N) fits, ("run", tag, query
# sets) plans and ticks each set.
STEPS = [
    ("opt", {N.SBO_OPT_PRECISION: 0}),         # the split sweep, whatever the probe would choose
    ("fit", 300),
    ("run", "n300", ["raster", "scatter"]),
    ("opt", {N.SBO_OPT_PRECISION: 1}),         # the precise path's plans and f64 partials
    ("run", "n300_precise", ["raster"]),
    ("opt", {N.SBO_OPT_PRECISION: 0}),
    ("fit", 1100),
    ("run", "n1100", ["raster", "scatter", "straddle", "far", "mixed"]),
    ("opt", {N.SBO_OPT_KERNEL_VARIANT: 22}),
    ("run", "n1100_v22", ["raster", "straddle"]),
    ("opt", {N.SBO_OPT_KERNEL_VARIANT: 3, N.SBO_OPT_TILE_SKIP: 0}),
    ("run", "n1100_dense", ["raster", "straddle"]),
    ("opt", {N.SBO_OPT_TILE_SKIP: -1, N.SBO_OPT_SKIP_BUDGET: 12}),
    ("fit", 1100),
    ("run", "n1100_b12", ["raster", "straddle"]),
    ("opt", {N.SBO_OPT_SKIP_BUDGET: 30}),
    ("fit", 1100),
    ("run", "n1100_b30", ["raster", "straddle"]),
    ("fit", 16640),                            # 65 row blocks: the last has 260 tiles > kPlanBinCache, water-filling on
    ("run", "n16640", ["first256"]),
]


def workload(n):
    return synthetic(n, 8, 8, seed=31, hyper=Hyper(**HYPER))


def debug_plan(gm, qx, qy):
    """sbo_debug_plan as (nI, nQ, items [nI, nQ, 2] = (thr, count), records [kept, 4] = (I, qb, t, level))."""
    lib = N.lib()
    qx = np.ascontiguousarray(qx, np.float32)
    qy = np.ascontiguousarray(qy, np.float32)
    n = ctypes.c_int64(0)
    gm.ctx.check(lib.sbo_debug_plan(gm.ctx.handle, qx.ctypes.data, qy.ctypes.data, qx.size, None, 0, ctypes.byref(n)))
    buf = np.empty(n.value, np.int32)
    gm.ctx.check(lib.sbo_debug_plan(gm.ctx.handle, qx.ctypes.data, qy.ctypes.data, qx.size, buf.ctypes.data, buf.size,
                                    ctypes.byref(n)))
    nI, nQ, kept = int(buf[0]), int(buf[1]), int(buf[2])
    items = buf[4:4 + 2 * nI * nQ].reshape(nI, nQ, 2)
    rec = buf[4 + 2 * nI * nQ:].reshape(kept, 4)
    assert int(items[:, :, 1].sum()) == kept and int((items[:, :, 1] > 0).sum()) == int(buf[3])
    return nI, nQ, items, rec


def tick(gm, wl, qx, qy):
    m = qx.size
    out = dict(mu=np.empty(m, np.float32), sd=np.empty(m, np.float32), lo=np.empty(m, np.float64),
               hi=np.empty(m, np.float64), safe=np.empty(m, np.uint8))
    key = gm.tick(np.ascontiguousarray(qx, np.float32), np.ascontiguousarray(qy, np.float32), wl.beta, wl.f_min,
                  outputs=out)
    out["key"] = np.array([key.score, float(key.idx)], np.float64)
    return out


def run_cases(path):
    """Every step on the library this process loaded; one npz."""
    lib = N.lib()
    res = {}
    gm = TerrainMapper(0, Hyper(**HYPER))
    wl = None
    try:
        for step in STEPS:
            if step[0] == "opt":
                for o, v in step[1].items():
                    gm.set_option(o, v)
                continue
            if step[0] == "fit":
                wl = workload(step[1])
                gm.fit(wl.x, wl.y, wl.obs)
                continue
            tag, kinds = step[1], step[2]
            for kind in kinds:
                qx, qy = queries(wl, kind)
                nI, nQ, items, rec = debug_plan(gm, qx, qy)
                k = f"{tag}/{kind}/"
                res[k + "shape"] = np.array([nI, nQ])
                res[k + "items"] = items
                # canonical order: the test compares plans, not the list chain's item order
                res[k + "rec"] = rec[np.lexsort((rec[:, 3], rec[:, 2], rec[:, 1], rec[:, 0]))]
                lib.sbo_profile(gm.ctx.handle, 1)
                for name, a in tick(gm, wl, qx, qy).items():
                    res[k + name] = a
                mf, lv = ctypes.c_double(), (ctypes.c_int64 * 3)()
                gm.ctx.check(lib.sbo_profile_mfma(gm.ctx.handle, ctypes.byref(mf), lv))
                lib.sbo_profile(gm.ctx.handle, 0)
                res[k + "mfma"] = np.array([mf.value, lv[0], lv[1], lv[2]], np.float64)
    finally:
        gm.close()
    np.savez(path, **res)


def _spawn(lib, path, ref):
    env = dict(os.environ, SBO_LIB=lib)
    env.pop("SBO_PLAN_REF", None)
    if ref:
        env["SBO_PLAN_REF"] = "1"
    code = (f"import sys; sys.path.insert(0, {ROOT!r}); sys.path.insert(0, {os.path.join(ROOT, 'tests')!r}); "
            f"import test_gpu_plan_front as T; T.run_cases({path!r})")
    return subprocess.Popen([sys.executable, "-c", code], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                            text=True)


@pytest.fixture(scope="module")
def both(tmp_path_factory):
    d = tmp_path_factory.mktemp("plan_front")
    prod = os.path.join(ROOT, "safe_bayesian_optimization_amd", "lib", "libsbo.so")
    diag = os.path.join(ROOT, "safe_bayesian_optimization_amd", "lib", "libsbo_diag.so")
    assert os.path.exists(diag), "lib/libsbo_diag.so not built (make -C safe_bayesian_optimization_amd diag)"
    paths = [str(d / "prod.npz"), str(d / "ref.npz")]
    procs = [_spawn(prod, paths[0], False), _spawn(diag, paths[1], True)]    # side by side
    for pr in procs:
        _, err = pr.communicate(timeout=300)
        assert pr.returncode == 0, err[-3000:]
    return dict(np.load(paths[0])), dict(np.load(paths[1]))


def test_plan_and_outputs_match_the_reference_builder(both):
    """Every run of STEPS: the same kept tiles and levels, thresholds and
    counts as the reference builder's, and byte-equal tick outputs -- the
    mixed set (one near block among far ones, ticked after the far raster on
    the same context) included."""
    p, r = both
    assert sorted(p) == sorted(r)
    for k in sorted(p):
        if k.endswith("/mfma"):
            continue
        a, b = p[k], r[k]
        assert a.dtype == b.dtype and a.shape == b.shape, k
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), (k, int(np.sum(a != b)))
    # the cases are what they claim to be
    assert tuple(p["n300/raster/shape"])[0] == 2 and tuple(p["n1100/raster/shape"])[0] == 5
    assert tuple(p["n16640/first256/shape"])[0] == 65 and p["n16640/first256/sd"].size == 256
    assert p["n1100/raster/sd"].size == 1200 and p["n1100/scatter/sd"].size == 1000
    for tag in ("n300", "n1100", "n16640"):
        kind = "first256" if tag == "n16640" else "raster"
        assert p[f"{tag}/{kind}/rec"].shape[0] > 0
    # levels are in play by default, and off for variant 22
    assert np.any(p["n1100/raster/rec"][:, 3] > 0) and not np.any(p["n1100_v22/raster/rec"][:, 3] > 0)
    # the dense plan keeps every tile of every item
    it = p["n1100_dense/raster/items"]
    assert np.array_equal(it[:, :, 1], np.repeat(4 * (np.arange(5) + 1)[:, None], it.shape[1], axis=1))
    # budgets move the plan
    assert p["n1100_b12/raster/rec"].shape[0] < p["n1100_b30/raster/rec"].shape[0]


def test_prefilter_takes_both_branches(both):
    """The straddling raster at N = 1100: some query blocks keep no tile in any
    row block (every k-tile far by the column bound), some keep tiles in every
    row block."""
    p, _ = both
    cnt = p["n1100/straddle/items"][:, :, 1]          # [nI, nQ]
    per_block = (cnt > 0).sum(axis=0)
    print("non-empty row blocks per query block:", per_block.tolist())
    assert np.any(per_block == 0) and np.any(per_block == cnt.shape[0])


def test_no_stale_partial_is_read(both):
    """After a near raster, a raster FAR length scales away on the same context
    and workspace: every item empty, so mu is the prior mean and sd is
    sqrt(sf2) exactly, and lo / hi / safe are the oracle's compute_sets of them."""
    p, _ = both
    wl = workload(1100)
    assert p["n1100/raster/items"][:, :, 1].sum() > 0
    assert p["n1100/far/items"].shape[1] * 128 >= 1200 and not np.any(p["n1100/far/items"][:, :, 1])
    mu, sd = p["n1100/far/mu"], p["n1100/far/sd"]
    assert np.all(mu == np.float32(HYPER["prior_mean"])) and np.all(sd == np.float32(HYPER["sigma_f"]))
    lo, hi, safe = O.compute_sets(mu, sd, wl.beta, wl.f_min)
    assert np.array_equal(p["n1100/far/lo"], lo) and np.array_equal(p["n1100/far/hi"], hi)
    assert np.array_equal(p["n1100/far/safe"], safe)
    # the mixed set has exactly one kind of each
    cnt = p["n1100/mixed/items"][:, :, 1]
    assert np.any(cnt.sum(axis=0) == 0) and np.any(cnt.sum(axis=0) > 0)
    assert np.any(p["n1100/mixed/sd"] != np.float32(HYPER["sigma_f"]))


def test_profile_counters_match(both):
    """sbo_profile_mfma's tiles_by_level and mfma_flops of the N = 1100 raster tick."""
    p, r = both
    a, b = p["n1100/raster/mfma"], r["n1100/raster/mfma"]
    print("mfma_flops, tiles at six / three / one product(s):", a.tolist())
    assert a[0] > 0 and a[1:].sum() == p["n1100/raster/rec"].shape[0]
    assert np.array_equal(a, b)
    for lvl in range(3):
        assert a[1 + lvl] == np.sum(p["n1100/raster/rec"][:, 3] == lvl)

"""The split sweep on row-half stages (csrc/predict_x3_rowhalf.hpp): the layout
of its operand, and the sweep against the diagnostic build's k-half
predecessor (variant 62) under every precision level.

A stage is row half R of a packed 64-k tile: three bf16 planes of 16 KiB, each
eight row blocks x two k halves of one 1 KiB lane-fragment piece (include/sbo.h,
sbo_debug_x3_operand)."""
import ctypes
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
BM, BK, TILE = 256, 64, 256 * 64
STAGE, PLANE = 49152, 16384


def _bf16_rne(a):
    """f32 -> bf16 bits (round to nearest even), and the bf16 value back as f32."""
    u = np.ascontiguousarray(a, np.float32).view(np.uint32)
    b = ((u + np.uint32(0x7FFF) + ((u >> np.uint32(16)) & np.uint32(1))) >> np.uint32(16)).astype(np.uint16)
    return b, (b.astype(np.uint32) << np.uint32(16)).view(np.float32)


def _split3(a):
    """v = v0 + v1 + v2 in bf16, each piece the rounding of what the ones before left."""
    a = np.ascontiguousarray(a, np.float32)
    b0, f0 = _bf16_rne(a)
    r1 = a - f0
    b1, f1 = _bf16_rne(r1)
    b2, _ = _bf16_rne(r1 - f1)
    return b0, b1, b2


def _tile_offset(k, row):
    """csrc/sbo_internal.hpp tile_offset: A[row][k] inside a packed [BK][BM] tile."""
    return (((row >> 6) * BK + k) * 16 + (row & 15)) * 4 + ((row >> 4) & 3)


def _operands(gm):
    """(f32 packed operand as [tiles, 16384], x3 operand as bytes) of a fitted mapper."""
    blob = gm.export_state().cpu().numpy()
    npad = int(blob[16:24].view(np.int64)[0])
    off_aug = int(blob[112:120].view(np.int64)[0])
    nI = npad // BM
    tiles = 4 * nI * (nI + 1) // 2
    aug = blob[off_aug:off_aug + 4 * tiles * TILE].view(np.float32).reshape(tiles, TILE)
    lib = N.lib()
    nb = ctypes.c_int64(0)
    gm.ctx.check(lib.sbo_debug_x3_operand(gm.ctx.handle, None, 0, ctypes.byref(nb)))
    assert nb.value == tiles * 2 * STAGE
    x3 = np.empty(nb.value, np.uint8)
    gm.ctx.check(lib.sbo_debug_x3_operand(gm.ctx.handle, x3.ctypes.data, x3.size, ctypes.byref(nb)))
    return aug, x3


def _check_layout(aug, x3):
    tiles = aug.shape[0]
    # [R, rb, h, g, r, j] -> the element's offset in the f32 tile
    R, rb, h, g, r, j = np.meshgrid(np.arange(2), np.arange(8), np.arange(2), np.arange(4), np.arange(16),
                                    np.arange(8), indexing="ij")
    src = _tile_offset(32 * h + 8 * g + j, 16 * (8 * R + rb) + r)
    # ... and the bf16's byte address in the tile's two stages (plane 0)
    dst = R * STAGE + (2 * rb + h) * 1024 + (16 * g + r) * 16 + 2 * j
    assert np.unique(dst).size == dst.size == 2 * 8 * 2 * 64 * 8
    vals = aug[:, src.ravel()]                                  # [tiles, 16384]
    pieces = _split3(vals)
    got = x3.view(np.uint16).reshape(tiles, 2 * STAGE // 2)
    for p in range(3):
        want = pieces[p].reshape(tiles, -1)
        have = got[:, (dst.ravel() + p * PLANE) // 2]
        bad = np.argwhere(want != have)
        assert bad.size == 0, (p, bad[:4], want[tuple(bad[0])], have[tuple(bad[0])])
    assert np.any(pieces[1]) and np.any(pieces[2])


def test_pack_layout_fit_and_append():
    """Every bf16 piece of the x3 operand against a numpy split3 of the f32
    packed operand at the documented byte address: a fit of N = 300 (two row
    blocks, the second ragged), and N = 64*5 + 7 after one append of 40
    (the incremental repack); then the state exported and imported into a
    fresh context: the same operand, and bitwise the same predictions."""
    wl = synthetic(300, 20, 15, seed=11)
    gm = TerrainMapper(0, wl.hyper)
    try:
        gm.fit(wl.x, wl.y, wl.obs)
        _check_layout(*_operands(gm))
    finally:
        gm.close()
    n0 = 64 * 5 + 7
    wl = synthetic(n0 + 40, 20, 15, seed=12)
    gm = TerrainMapper(0, wl.hyper)
    g2 = TerrainMapper(0, wl.hyper)
    try:
        gm.fit(wl.x[:n0], wl.y[:n0], wl.obs[:n0])
        gm.predict(wl.qx, wl.qy)              # the operand derived once before the append
        gm.append(wl.x[n0:], wl.y[n0:], wl.obs[n0:])
        assert gm.n == n0 + 40
        aug, x3 = _operands(gm)
        _check_layout(aug, x3)
        mu, sd = gm.predict(wl.qx, wl.qy)
        g2.import_state(gm.export_state())
        mu2, sd2 = g2.predict(wl.qx, wl.qy)
        assert np.array_equal(np.asarray(mu), np.asarray(mu2)) and np.array_equal(np.asarray(sd), np.asarray(sd2))
        aug2, x32 = _operands(g2)
        assert np.array_equal(aug.view(np.uint32), aug2.view(np.uint32)) and np.array_equal(x3, x32)
    finally:
        gm.close()
        g2.close()


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
    for v in {variants!r}:
        gm.set_option(N.SBO_OPT_KERNEL_VARIANT, v)
        mu, sd = gm.predict(d["qx"], d["qy"])
        out["mu_%s_%d" % (force, v)] = np.asarray(mu)
        out["sd_%s_%d" % (force, v)] = np.asarray(sd)
gm.close()
np.savez({path!r}, **out)
'''


def _child(lib, inp, path, forces, variants):
    env = dict(os.environ, SBO_LIB=lib)
    env.pop("SBO_LVL_FORCE", None)
    r = subprocess.run([sys.executable, "-c", CHILD.format(root=ROOT, inp=inp, path=path, forces=forces,
                                                          variants=variants)],
                       env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    return dict(np.load(path))


def _far_block_tiles(cost):
    """Kept tiles of the last (44-query) block over all its items, from
    sbo_query_cost: cost = the block's kept tiles weighted 1, 42/64, 33/64 by
    level, / the block's size.  The count if every tile has one weight (a mix
    has no single answer: -1), 0 for none."""
    far = np.asarray(cost, np.float64)[256:]
    assert far.size == 44 and np.all(far == far[0]), "the far queries are not one block of the plan"
    total = far[0] * 44
    for w in (33 / 64, 42 / 64, 1.0):
        n = total / w
        if abs(n - round(n)) < 1e-4:
            return int(round(n))
    return -1


def test_sweep_matches_k_half_predecessor_at_every_level(tmp_path):
    """N = 520 (three row blocks, the last ragged), M = 300 (three query blocks,
    the last ragged).  The last block lies outside the data, at the distance
    at which the plan keeps exactly one tile of it -- one item of a single
    tile, whose first step is its last and whose K* was built during another
    item's last tile -- found by scanning `sbo_query_cost` (the plan, no
    sweep) and asserted in both libraries on the input they sweep.

    The product and the diagnostic build's variant 3 are one kernel from one
    header and must agree bit for bit, default plan and full precision
    (variant 22).  Levels can be forced only in the diagnostic build
    (SBO_LVL_FORCE exists under SBO_DIAG alone, and the product takes no new
    knob), so with every kept tile forced to six, three and one product(s) --
    and under the default plan -- variant 3 is held bit for bit to the k-half
    predecessor (variant 62) there: another kernel on another operand layout,
    the stronger check.  The default plan and variant 22 keep the 1e-5
    contract against the fp64 oracle.  Each library runs in a child process
    of its own."""
    prod = os.path.join(ROOT, "safe_bayesian_optimization_amd", "lib", "libsbo.so")
    diag = os.path.join(ROOT, "safe_bayesian_optimization_amd", "lib", "libsbo_diag.so")
    assert os.path.exists(diag), "lib/libsbo_diag.so not built (make -C safe_bayesian_optimization_amd diag)"
    wl = synthetic(520, 16, 16, seed=21)
    side, ls = float(wl.qx.max()), wl.hyper.length_scale
    rng = np.random.default_rng(5)
    ux, uy = rng.random(44), rng.random(44)

    def queries(dist):
        return (np.concatenate([wl.qx[:256], side + ls * (dist + ux)]).astype(np.float32),
                np.concatenate([wl.qy[:256], side + ls * (dist + uy)]).astype(np.float32))

    # the distance (in length scales beyond the data's corner) at which the far
    # block keeps one tile: the first of the scan, the plan being monotone in it
    gm = TerrainMapper(0, wl.hyper)
    try:
        gm.set_option(N.SBO_OPT_PRECISION, 0)
        gm.fit(wl.x, wl.y, wl.obs)
        dist = next((t for t in np.arange(2.0, 8.0, 1.0 / 32) if _far_block_tiles(gm.query_cost(*queries(t))) == 1),
                    None)
    finally:
        gm.close()
    assert dist is not None, "no distance at which the far query block keeps exactly one tile"
    print(f"far block at {dist:.5f} length scales: one kept tile")
    qx, qy = queries(dist)
    assert qx.size == 300
    inp = str(tmp_path / "in.npz")
    np.savez(inp, x=wl.x, y=wl.y, obs=wl.obs, qx=qx, qy=qy)
    p = _child(prod, inp, str(tmp_path / "prod.npz"), [None], [3, 22])
    d = _child(diag, inp, str(tmp_path / "diag.npz"), [None, 0, 1, 2], [3, 22, 62])
    # the single-tile item is in the plan each library swept
    assert _far_block_tiles(p["cost"]) == 1 and _far_block_tiles(d["cost"]) == 1
    for v in (3, 22):
        for k in ("mu", "sd"):
            assert np.array_equal(p[f"{k}_None_{v}"], d[f"{k}_None_{v}"]), (k, v)
    for force in (None, 0, 1, 2):
        for k in ("mu", "sd"):
            a, b = d[f"{k}_{force}_3"], d[f"{k}_{force}_62"]
            assert np.array_equal(a, b), (k, force, int(np.sum(a != b)))
    # the forced levels are different computations, not one result three times
    assert not np.array_equal(d["sd_0_3"], d["sd_2_3"])
    # the fp64 oracle given the device factor
    o = p["order"]
    Lcm = O.colmajor_from_lower(p["L"].astype(np.float64))
    omu, ovar = O.predict(Lcm, p["alpha"].astype(np.float64), wl.x.astype(np.float32)[o], wl.y.astype(np.float32)[o],
                          qx, qy, wl.hyper.length_scale, wl.hyper.sf2, wl.hyper.prior_mean)
    for res in (p, d):
        for v in (3, 22):
            gmu = res[f"mu_None_{v}"].astype(np.float64)
            gvar = res[f"sd_None_{v}"].astype(np.float64) ** 2
            emu = np.abs(gmu - omu).max() / np.abs(omu).max()
            evar = np.abs(gvar - ovar).max() / np.abs(ovar).max()
            print(f"variant {v}: mu_err={emu:.2e} var_err={evar:.2e}")
            assert emu < 1e-5 and evar < 1e-5, (v, emu, evar)

"""Device time of sbo_whatif beside the stream update of as many rows.

    python tools/whatif_timing.py [--n 16384] [--reps 3] > profiles/whatif.log

Every line of profiles/whatif.log is this tool's output, the header included.

Two settings of n points: bench.py's C4 synthetic domain on a 1000 x 1000 grid,
and config/lpsc.yaml's own box [0, 1] x [0, 2.5] on the mapper's 300 x 120
grid.  Per setting and repetition: fit n - 64 points, sbo_tick_stream (the
full sweep, kept), append 64 points, sbo_tick_stream again -- the yardstick:
predict_update_kernel over R = 64 rows (the largest R that path takes by
default), timed by sbo_profile's events round that launch alone.  Then, on the
same fit (n points) and kept posterior, sbo_whatif for p = 16, 64 and 256
candidates uniform over the data box: the weights' time (fill, the two
triangular products, the candidate sums; with SBO_OPT_WHATIF_GEMM 0 dtrmm and
1 dgemm) and the sweep's time (whatif_kernel alone), both from sbo_profile's
events, the tiles kept and the cutoff L.  Medians over the repetitions after
one warm-up repetition.  Both kernels run the one k-tile walk of
csrc/kstar_walk.hpp, so the yardstick times the same loop over another left
operand; for a kernel of another build, run this tool under SBO_LIB.  The update and the sweep
at p = 64 contract the same m x n_kept x 64 products; the update's cutoff
spends 2^-SBO_OPT_STREAM_SHARE of the skip budget, the what-if's all of it, so
their kept tiles differ: both are printed, the ratio per kept tile too, and
the p = 64 sweep is also run at the update's own cutoff (SBO_OPT_TILE_SKIP set
to its L for that call), where both multiply the same tiles.
"""
import argparse
import ctypes
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def profile_ms(gm, fn):
    """(predict ms, fill ms) of sbo_profile's events round the launches fn makes."""
    from safe_bayesian_optimization_amd import _native as N
    lib = N.lib()
    gm.ctx.check(lib.sbo_profile(gm.ctx.handle, 1))
    out = fn()
    pm, fm = ctypes.c_double(), ctypes.c_double()
    pc, fc = ctypes.c_int64(), ctypes.c_int64()
    gm.ctx.check(lib.sbo_profile_read(gm.ctx.handle, ctypes.byref(pm), ctypes.byref(pc), ctypes.byref(fm),
                                      ctypes.byref(fc)))
    gm.ctx.check(lib.sbo_profile(gm.ctx.handle, 0))
    return pm.value, fm.value, out


def run(name, wl, reps):
    import torch

    from safe_bayesian_optimization_amd import TerrainMapper
    from safe_bayesian_optimization_amd import _native as N
    from safe_bayesian_optimization_amd.terrain import uniform
    dev = torch.device("cuda:0")
    f32 = lambda v: torch.as_tensor(np.ascontiguousarray(v, np.float32), device=dev)  # noqa: E731
    n, R = wl.x.size, 64
    X, Y, OBS, QX, QY = f32(wl.x), f32(wl.y), f32(wl.obs), f32(wl.qx), f32(wl.qy)
    m = QX.numel()
    outs = dict(mu=torch.empty(m, device=dev), sd=torch.empty(m, device=dev),
                lo=torch.empty(m, dtype=torch.float64, device=dev), hi=torch.empty(m, dtype=torch.float64, device=dev),
                safe=torch.empty(m, dtype=torch.uint8, device=dev))
    gm = TerrainMapper(0, wl.hyper)
    upd, upd_tiles, rows, same_l = [], None, {}, []
    for rep in range(reps + 1):
        gm.fit(X[:n - R], Y[:n - R], OBS[:n - R])
        gm.tick_stream(QX, QY, wl.beta, wl.f_min, outputs=outs)
        gm.append(X[n - R:], Y[n - R:], OBS[n - R:])
        ms, _, _ = profile_ms(gm, lambda: gm.tick_stream(QX, QY, wl.beta, wl.f_min, outputs=outs))
        info = gm.stream_info()
        assert info["path"] == 1 and info["rows"] == R, info
        if rep:
            upd.append(ms)
        upd_tiles = (info["tiles_kept"], info["tiles_total"], info["cutoff_log2"])
        for p in (16, 64, 256):
            u = uniform(7 + p, 2 * p)
            cx = f32(wl.x.min() + u[0::2] * (wl.x.max() - wl.x.min()))
            cy = f32(wl.y.min() + u[1::2] * (wl.y.max() - wl.y.min()))
            for gemm in (0, 1):
                gm.set_option(N.SBO_OPT_WHATIF_GEMM, gemm)
                sweep, weights, w = profile_ms(gm, lambda: gm.whatif(cx, cy, wl.beta, wl.f_min))
                if rep:
                    rows.setdefault((p, gemm), []).append((weights, sweep, w))
            gm.set_option(N.SBO_OPT_WHATIF_GEMM, 0)
            if p == 64:   # the sweep at the update's own cutoff: the same kept tiles
                gm.set_option(N.SBO_OPT_TILE_SKIP, upd_tiles[2])
                sweep, _, w = profile_ms(gm, lambda: gm.whatif(cx, cy, wl.beta, wl.f_min))
                gm.set_option(N.SBO_OPT_TILE_SKIP, -1)
                if rep:
                    same_l.append((sweep, w["tiles_kept"]))
    u_ms = float(np.median(upd))
    print(f"{name}: n={n} m={m} stream update R=64: update_kernel_ms={u_ms:.3f} tiles_kept={upd_tiles[0]} "
          f"tiles_total={upd_tiles[1]} L={upd_tiles[2]}", flush=True)
    for (p, gemm), v in sorted(rows.items()):
        wms, sms = float(np.median([a[0] for a in v])), float(np.median([a[1] for a in v]))
        w = v[-1][2]
        line = (f"{name}: p={p} weights={'dgemm' if gemm else 'dtrmm'} weights_ms={wms:.3f} sweep_ms={sms:.3f} "
                f"tiles_kept={w['tiles_kept']} tiles_total={w['tiles_total']} L={w['cutoff_log2']} "
                f"err_cov={w['err_cov']:.3e} best_gain={w['best_gain']} nonzero_gains={int((w['gain'] > 0).sum())}")
        if p == 64:
            per_tile = (sms / max(w["tiles_kept"], 1)) / (u_ms / max(upd_tiles[0], 1))
            line += f" sweep_over_update={sms / u_ms:.3f} per_kept_tile={per_tile:.3f}"
        print(line, flush=True)
    s_ms = float(np.median([a[0] for a in same_l]))
    print(f"{name}: p=64 at the update's cutoff L={upd_tiles[2]}: sweep_ms={s_ms:.3f} tiles_kept={same_l[-1][1]} "
          f"sweep_over_update={s_ms / u_ms:.3f}", flush=True)
    gm.close()


def main():
    a = argparse.ArgumentParser()
    a.add_argument("--n", type=int, default=16384)
    a.add_argument("--reps", type=int, default=3)
    a = a.parse_args()
    print(f"# tools/whatif_timing.py --n {a.n} --reps {a.reps}: medians of {a.reps} warm repetitions, 1 GPU",
          flush=True)
    from safe_bayesian_optimization_amd.terrain import synthetic, synthetic_box
    run("C4 synthetic 1000x1000", synthetic(a.n, 1000, 1000, seed=0, name="C4"), a.reps)
    run("lpsc box 300x120", synthetic_box(a.n, 300, 120, seed=0), a.reps)


if __name__ == "__main__":
    main()

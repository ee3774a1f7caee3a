#!/usr/bin/env python3
"""The node's steady state with a kept posterior: "append b points, tick" with
sbo_tick_stream, beside sbo_tick's full sweep on the same context and state.

Per workload one JSON line: append_ms, tick_ms (sbo_tick_stream, every call
ends in a device synchronise) and full_tick_ms (sbo_tick right after it, the
same fit and queries) as mean / median / min over the iterations, the path
and reason counts, and tiles_kept / tiles_total of the updates.

  c4_append1   C4 (N = 16384, 1000 x 1000 grid), one-point appends
  c5_loop      C5 (N 1000 -> 8000 in 50 appends, 512 x 512 grid), at the default
               SBO_OPT_STREAM_MAX_ROWS and with the cap lifted
  rows_curve   C5's shapes at N = 4000: update against full tick for R = 1 .. 512
  lpsc_mapper  the lpsc box at N = 16384 on the mapper's 300 x 120 grid
  lpsc_grid    the lpsc box at N = 16384 on a 1000 x 1000 grid

usage: python tools/stream_tick_ab.py [--workloads a,b,...] [--iters K]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from safe_bayesian_optimization_amd import TerrainMapper, synthetic  # noqa: E402
from safe_bayesian_optimization_amd import _native as N  # noqa: E402
from safe_bayesian_optimization_amd.terrain import more_points, normal, smooth_field, synthetic_box, uniform  # noqa: E402

DEV = torch.device("cuda:0")


def t32(a):
    return torch.as_tensor(np.ascontiguousarray(a, np.float32), device=DEV)


def stats(v):
    return {"mean": statistics.fmean(v), "median": statistics.median(v), "min": min(v), "n": len(v)} if v else None


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


class Loop:
    """One mapper, one query grid; step(points) = append, tick_stream, sbo_tick."""

    def __init__(self, wl, options=()):
        self.wl = wl
        self.gm = TerrainMapper(0, wl.hyper)
        for o, v in options:
            self.gm.set_option(o, v)
        self.qx, self.qy = t32(wl.qx), t32(wl.qy)
        m = self.qx.numel()
        self.outs = dict(mu=torch.empty(m, device=DEV), sd=torch.empty(m, device=DEV),
                         lo=torch.empty(m, dtype=torch.float64, device=DEV),
                         hi=torch.empty(m, dtype=torch.float64, device=DEV),
                         safe=torch.empty(m, dtype=torch.uint8, device=DEV))
        self.key = torch.empty(2, dtype=torch.int64, device=DEV)
        self.t_app, self.t_tick, self.t_full, self.t_upd = [], [], [], []
        self.reasons, self.kept, self.total = {}, 0, 0

    def fit(self, x, y, obs):
        self.gm.fit(t32(x), t32(y), t32(obs))
        self.stream()
        self.full()
        torch.cuda.synchronize()

    def stream(self):
        self.gm.tick_stream(self.qx, self.qy, self.wl.beta, self.wl.f_min, outputs=self.outs, key_out=self.key)

    def full(self):
        self.gm.tick(self.qx, self.qy, self.wl.beta, self.wl.f_min, outputs=self.outs, key_out=self.key)

    def step(self, x, y, obs, full=True, record=True):
        X, Y, Ob = t32(x), t32(y), t32(obs)
        ta = timed(lambda: self.gm.append(X, Y, Ob))
        tt = timed(self.stream)
        info = self.gm.stream_info()
        tf = timed(self.full) if full else None
        if not record:
            return
        self.t_app.append(ta)
        self.t_tick.append(tt)
        if info["path"] == 1:
            self.t_upd.append(tt)
        if tf is not None:
            self.t_full.append(tf)
        self.reasons[info["reason"]] = self.reasons.get(info["reason"], 0) + 1
        self.kept += info["tiles_kept"]
        self.total += info["tiles_total"]

    def line(self, name, **extra):
        m = self.qx.numel()
        out = {"workload": name, "M": m, "n_after": self.gm.n, "precise_sweep": self.gm.precision()[0],
               "append_ms": stats(self.t_app), "tick_ms": stats(self.t_tick), "update_tick_ms": stats(self.t_upd),
               "full_tick_ms": stats(self.t_full), "reasons": self.reasons,
               "tiles_kept_over_total": [self.kept, self.total]}
        out.update(extra)
        print(json.dumps(out), flush=True)
        self.gm.close()


def box_points(k, seed, hyper):
    """k further measurements on the lpsc box, from synthetic_box's own field."""
    u = uniform(seed ^ 0xADD, 2 * k)
    x, y = u[0::2], 2.5 * u[1::2]
    return x, y, smooth_field(x, y, 2.5, hyper.length_scale, 0) + np.sqrt(hyper.sn2) * normal(seed + 7, k)


def c4_append1(iters):
    wl = synthetic(16384, 1000, 1000, seed=0, name="C4")
    lp = Loop(wl)
    lp.fit(wl.x, wl.y, wl.obs)
    ax, ay, ao = more_points(wl, iters + 1, seed=2024)
    for i in range(iters + 1):
        lp.step(ax[i:i + 1], ay[i:i + 1], ao[i:i + 1], record=i > 0)
    lp.line("c4_append1", b=1)


def c5_loop(iters, max_rows=None):
    wl = synthetic(8000, 512, 512, seed=0, name="C5")
    chunks = np.linspace(1000, 8000, 51).round().astype(int)
    lp = Loop(wl, [] if max_rows is None else [(N.SBO_OPT_STREAM_MAX_ROWS, max_rows)])
    lp.fit(wl.x[:1000], wl.y[:1000], wl.obs[:1000])
    for a, b in zip(chunks[:-1], chunks[1:]):
        lp.step(wl.x[a:b], wl.y[a:b], wl.obs[a:b])
    lp.line("c5_loop", b=140, stream_max_rows="default" if max_rows is None else max_rows)


def rows_curve(iters):
    wl = synthetic(8000, 512, 512, seed=0, name="C5")
    for R in (1, 8, 16, 32, 64, 128, 256, 512):
        lp = Loop(wl, [(N.SBO_OPT_STREAM_MAX_ROWS, 65536), (N.SBO_OPT_RESORT, 0)])
        lp.fit(wl.x[:4000], wl.y[:4000], wl.obs[:4000])
        for i in range(4):
            a = 4000 + i * R
            lp.step(wl.x[a:a + R], wl.y[a:a + R], wl.obs[a:a + R], record=i > 0)
        lp.line("rows_curve", b=R)


def lpsc(name, gw, gh, iters, full_every):
    wl = synthetic_box(16384, gw, gh, seed=0)
    lp = Loop(wl)
    lp.fit(wl.x, wl.y, wl.obs)
    ax, ay, ao = box_points(iters + 1, 2024, wl.hyper)
    for i in range(iters + 1):
        lp.step(ax[i:i + 1], ay[i:i + 1], ao[i:i + 1], full=i % full_every == 0, record=i > 0)
    lp.line(name, b=1)


def main():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--workloads", default="c4_append1,c5_loop,rows_curve,lpsc_mapper,lpsc_grid")
    p.add_argument("--iters", type=int, default=30, help="one-point appends per workload")
    a = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("stream_tick_ab.py needs a GPU")
    for w in a.workloads.split(","):
        if w == "c4_append1":
            c4_append1(a.iters)
        elif w == "c5_loop":
            c5_loop(a.iters)
            c5_loop(a.iters, max_rows=1024)
        elif w == "rows_curve":
            rows_curve(a.iters)
        elif w == "lpsc_mapper":
            lpsc("lpsc_mapper_grid", 300, 120, a.iters, 5)
        elif w == "lpsc_grid":
            lpsc("lpsc_stress_box", 1000, 1000, max(4, a.iters // 6), 3)
        else:
            raise SystemExit(f"unknown workload {w}")


if __name__ == "__main__":
    main()

"""Device time of sbo_remove beside the same run's warm refit of the remaining points.

    python tools/remove_timing.py [--n 16384] [--reps 10] > profiles/remove.log
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o remove -- python tools/remove_timing.py --kernels
    python tools/remove_timing.py --stats DIR/.../remove_kernel_stats.csv >> profiles/remove.log

Every line of profiles/remove.log is this tool's output, the header included.

bench.py's C4 training set (n points, about 8 per l^2), SBO_OPT_RESORT 0 and
SBO_OPT_REMOVE_MAX 256 so that every removal takes the rotation path; warmed
up; times are device events on the context's stream around calls that end in
a synchronise; the versions alternate inside each repetition; median and
[min, max] over the repetitions.
  1. one point at stored position 0, n/4, n/2, 3n/4, n-1, each followed by
     the append that restores n, and the warm sbo_fit of the n-1 points left;
  2. b = 2, 4, ... 256 points at uniformly random stored positions, and the
     warm sbo_fit of the n-b points left;
  3. the window step -- remove 1, append 1, full tick on the C4 grid -- next
     to fit + tick.
The two decisions read off it (include/sbo.h): whether the
one-point removal at position 0 beats the refit by more than the run's
spread, and SBO_OPT_REMOVE_MAX's default: the largest power of two b <= 256
whose removal takes at most 0.8 of the refit's time.

--kernels: a few one-point removals at position 0 and nothing else, for a
kernel trace.  --stats: that trace's per-kernel statistics, the remove_*
kernels' times per call, and for the row pass over X the bytes it must move
(16 B per touched element: column c of n is touched in rows max(1, c) .. n-1
for position 0) over its time as a share of the HBM peak (8 TB/s).
"""
import argparse
import csv
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_PEAK = 8.0e12


def stat(v):
    v = np.asarray(v, np.float64)
    return f"{np.median(v):.3f} [{v.min():.3f}, {v.max():.3f}]"


class Timed:
    """A mapper on a torch stream, and device-event timing of calls on it."""

    def __init__(self, wl):
        import torch

        from safe_bayesian_optimization_amd import TerrainMapper
        from safe_bayesian_optimization_amd import _native as N
        self.torch = torch
        self.dev = torch.device("cuda:0")
        self.stream = torch.cuda.Stream(self.dev)
        self.gm = TerrainMapper(0, wl.hyper)
        self.gm.ctx.set_stream(self.stream)
        self.gm.set_option(N.SBO_OPT_RESORT, 0)
        self.gm.set_option(N.SBO_OPT_REMOVE_MAX, 256)
        self.x, self.y, self.obs = (np.ascontiguousarray(a, np.float32) for a in (wl.x, wl.y, wl.obs))

    def t(self, a):
        return self.torch.as_tensor(np.ascontiguousarray(a, np.float32), device=self.dev)

    def ms(self, fn):
        torch = self.torch
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(self.stream):
            e0.record()
            out = fn()
            e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1), out

    def fit(self, keep=None):
        x, y, o = (self.x, self.y, self.obs) if keep is None else (self.x[keep], self.y[keep], self.obs[keep])
        X, Y, O = self.t(x), self.t(y), self.t(o)
        self.cur = (x, y, o)
        return self.ms(lambda: self.gm.fit(X, Y, O))[0]


def one_point(T, n, reps):
    places = {"0": 0, "n/4": n // 4, "n/2": n // 2, "3n/4": 3 * n // 4, "n-1": n - 1}
    rm = {k: [] for k in places}
    ap = {k: [] for k in places}
    dev = {k: [] for k in places}
    fit = []
    T.fit()
    for _ in range(reps):
        for name, pos in places.items():
            x, y, o = T.cur
            idx = int(T.gm.order()[pos])
            t, info = T.ms(lambda: T.gm.remove([idx]))
            assert info["path"] == 1 and info["first_row"] == pos
            rm[name].append(t)
            dev[name].append(info["ms"])
            px, py, po = T.t(x[idx:idx + 1]), T.t(y[idx:idx + 1]), T.t(o[idx:idx + 1])
            ap[name].append(T.ms(lambda: T.gm.append(px, py, po))[0])
            keep = np.r_[np.delete(np.arange(n), idx), idx]
            T.cur = (x[keep], y[keep], o[keep])
        fit.append(T.fit(np.arange(n - 1)))
        T.fit()
    for name in places:
        print(f"one point at stored position {name}: remove_ms {stat(rm[name])} (info.ms {stat(dev[name])}) "
              f"append_ms {stat(ap[name])}", flush=True)
    print(f"warm sbo_fit of the {n - 1} points left: fit_ms {stat(fit)}", flush=True)
    f, r0 = np.asarray(fit), np.asarray(rm["0"])
    spread = max(f.max() - f.min(), r0.max() - r0.min())
    wins = np.median(f) - np.median(r0) > spread
    print(f"worst case against the refit: position 0 {np.median(r0):.3f} ms, refit {np.median(f):.3f} ms, the run's "
          f"spread {spread:.3f} ms: the removal {'wins' if wins else 'DOES NOT WIN'} by more than the spread",
          flush=True)
    return float(np.median(f))


def batches(T, n, reps):
    rng = np.random.default_rng(0)
    best = 1
    for b in (2, 4, 8, 16, 32, 64, 128, 256):
        rm, fit = [], []
        for _ in range(reps):
            T.fit()
            pos = rng.choice(n, b, replace=False)
            idx = T.gm.order()[pos]
            t, info = T.ms(lambda: T.gm.remove(idx))
            assert info["path"] == 1
            rm.append(t)
            fit.append(T.fit(np.delete(np.arange(n), idx)))
        ratio = np.median(rm) / np.median(fit)
        if ratio <= 0.8 and best * 2 == b:
            best = b
        print(f"b = {b} random stored positions: remove_ms {stat(rm)} warm fit of the {n - b} left fit_ms {stat(fit)} "
              f"ratio {ratio:.3f}", flush=True)
    print(f"SBO_OPT_REMOVE_MAX default by the 0.8 rule: {best}", flush=True)


def window(T, wl, n, reps):
    torch = T.torch
    qx, qy = T.t(wl.qx), T.t(wl.qy)
    m = qx.numel()
    outs = dict(mu=torch.empty(m, dtype=torch.float32, device=T.dev), sd=torch.empty(m, dtype=torch.float32, device=T.dev))
    tick = lambda: T.gm.tick(qx, qy, wl.beta, wl.f_min, outputs=outs)  # noqa: E731
    T.fit()
    tick()
    step, refit = [], []
    for r in range(reps):
        x, y, o = T.cur
        px, py, po = T.t(x[:1]), T.t(y[:1]), T.t(o[:1])

        def win():
            T.gm.forget_oldest(1)
            T.gm.append(px, py, po)
            tick()
        step.append(T.ms(win)[0])
        T.cur = (np.r_[x[1:], x[:1]], np.r_[y[1:], y[:1]], np.r_[o[1:], o[:1]])
        X, Y, O = T.t(T.cur[0]), T.t(T.cur[1]), T.t(T.cur[2])

        def full():
            T.gm.fit(X, Y, O)
            tick()
        refit.append(T.ms(full)[0])
    print(f"window step (remove 1 + append 1 + full tick, m = {m}): ms {stat(step)}; fit + tick: ms {stat(refit)}",
          flush=True)


def kernels_only(T, n):
    T.fit()
    for _ in range(3):
        idx = int(T.gm.order()[0])
        T.gm.remove([idx])
        T.fit()


def read_stats(path, n):
    rows = []
    with open(path) as f:
        for r in csv.DictReader(f):
            if "remove_" in r.get("Name", ""):
                rows.append(r)
    touched = sum(n - max(1, c) for c in range(n))
    for r in rows:
        name = r["Name"].split("(")[0]
        calls, avg_us = int(r["Calls"]), float(r["AverageNs"]) / 1e3
        line = f"kernel {name}: calls {calls} average_us {avg_us:.2f} total_ms {float(r['TotalDurationNs']) / 1e6:.3f}"
        if "remove_rows_kernel" in name:
            gbs = 16.0 * touched / (avg_us * 1e-6)
            line += (f" bytes_to_move {16.0 * touched:.4e} (position 0, n = {n}) rate {gbs / 1e12:.3f} TB/s "
                     f"hbm_peak_share {gbs / HBM_PEAK:.3f}")
        print(line, flush=True)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--n", type=int, default=16384)
    p.add_argument("--reps", type=int, default=10)
    p.add_argument("--kernels", action="store_true")
    p.add_argument("--stats")
    a = p.parse_args()
    if a.stats:
        print(f"# tools/remove_timing.py --stats: the remove_* kernels of a rocprofv3 --kernel-trace --stats run of "
              f"--kernels (one point at stored position 0, n = {a.n})", flush=True)
        read_stats(a.stats, a.n)
        return
    from safe_bayesian_optimization_amd.terrain import synthetic
    wl = synthetic(a.n, 1000, 1000, seed=0, name="C4")
    T = Timed(wl)
    if a.kernels:
        kernels_only(T, a.n)
        return
    print(f"# tools/remove_timing.py --n {a.n} --reps {a.reps}: median [min, max] of {a.reps} repetitions, device "
          f"events, 1 GPU", flush=True)
    T.fit()
    T.fit()
    one_point(T, a.n, a.reps)
    batches(T, a.n, a.reps)
    window(T, wl, a.n, a.reps)


if __name__ == "__main__":
    main()

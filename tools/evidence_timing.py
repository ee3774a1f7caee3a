"""Device time of sbo_evidence beside the same run's warm fit.

    python tools/evidence_timing.py [--n 16384] [--reps 3] [--bench BEFORE.json AFTER.json] > profiles/evidence.log

Every line of profiles/evidence.log is this tool's output, the header included.
--bench takes two files that each hold the JSON result line of a
`bench.py --gpus 1` run, on the parent commit and on this one, and prints
their rate, tick time and fit times as two more lines: that the existing paths
did not move.

Two data sets of n points: bench.py's C4 synthetic domain (about 8 points per
l^2, where the k-tile pair cutoff drops most pairs) and config/lpsc.yaml's own
box [0, 1] x [0, 2.5] (dense data: no pair is sqrt(2) l apart enough to drop,
and SBO_OPT_EVIDENCE_BUDGET 0 runs every pair).  Per data set: the warm fit
(wall clock, synchronised), sbo_evidence's device time (its own `ms`: the two
kernel phases) and wall time, the pairs kept, the cutoff's bound, and the Gram
contraction's rate: 2 * 64 * 64 * (n - 64 J) flop per kept pair (I, J) over
the call's device time, against the 78.6 TFLOP/s f64 matrix peak.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

F64_PEAK = 78.6e12


def run(name, wl, budget, reps):
    import torch

    from safe_bayesian_optimization_amd import TerrainMapper
    from safe_bayesian_optimization_amd import _native as N
    dev = torch.device("cuda:0")
    f32 = lambda v: torch.as_tensor(np.ascontiguousarray(v, np.float32), device=dev)  # noqa: E731
    X, Y, OBS = f32(wl.x), f32(wl.y), f32(wl.obs)
    gm = TerrainMapper(0, wl.hyper)
    gm.set_option(N.SBO_OPT_EVIDENCE_BUDGET, budget)
    n = X.numel()
    fit_ms = []
    for _ in range(reps + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        gm.fit(X, Y, OBS)
        torch.cuda.synchronize()
        fit_ms.append((time.perf_counter() - t0) * 1e3)
    dev_ms, wall_ms = [], []
    for _ in range(reps + 1):
        t0 = time.perf_counter()
        e = gm.evidence()
        wall_ms.append((time.perf_counter() - t0) * 1e3)
        dev_ms.append(e["ms"])
    T = (n + 63) // 64
    # every pair's flop; a run that dropped pairs does less and reports no rate
    dense_flop = sum(2.0 * 64 * 64 * (n - 64 * J) * (J + 1) for J in range(T))
    ms = float(np.median(dev_ms[1:]))
    line = (f"{name}: n={n} budget={budget} warm_fit_ms={np.median(fit_ms[1:]):.2f} "
            f"evidence_device_ms={ms:.3f} evidence_wall_ms={np.median(wall_ms[1:]):.3f} "
            f"pairs_kept={e['pairs_kept']} pairs_total={e['pairs_total']} "
            f"grad_err_bound={e['grad_err_bound']:.3e} grad_budget={e['grad_budget']:.3e} "
            f"lml={e['lml']:.6f} grad=({', '.join(f'{g:.6e}' for g in e['grad'])}) loo_log_pred={e['loo_log_pred']:.6f}")
    if e["pairs_kept"] == e["pairs_total"]:
        line += f" gram_flop={dense_flop:.4e} f64_mfma_peak_fraction={dense_flop / (ms * 1e-3) / F64_PEAK:.3f}"
    print(line, flush=True)
    gm.close()
    return e


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--n", type=int, default=16384)
    p.add_argument("--reps", type=int, default=3)
    p.add_argument("--bench", nargs=2, metavar=("BEFORE", "AFTER"))
    a = p.parse_args()
    print(f"# tools/evidence_timing.py --n {a.n} --reps {a.reps}: medians of {a.reps} warm repetitions, 1 GPU", flush=True)
    from safe_bayesian_optimization_amd.terrain import synthetic, synthetic_box
    c4 = synthetic(a.n, 8, 8, seed=0, name="C4")
    cut = run("C4 synthetic, cutoff", c4, 20, a.reps)
    dense = run("C4 synthetic, dense", c4, 0, a.reps)
    print(f"C4 synthetic: |grad0(cutoff) - grad0(dense)| = {abs(cut['grad'][0] - dense['grad'][0]):.3e} "
          f"(bound {cut['grad_err_bound']:.3e})", flush=True)
    run("lpsc box, dense", synthetic_box(a.n, 8, 8, seed=0), 0, a.reps)
    run("lpsc box, cutoff", synthetic_box(a.n, 8, 8, seed=0), 20, a.reps)
    for name, path in zip(("before", "after"), a.bench or ()):
        with open(path) as f:
            d = json.loads(f.read().strip().splitlines()[-1])
        fit = " ".join(f"{k}={v:.2f}" for k, v in d.items() if "fit" in k and isinstance(v, (int, float)))
        print(f"bench.py {name}: steps={d['steps']} warmup={d['warmup']} value={d['value']:.4e} {d['unit']} "
              f"ms_per_step={d['ms_per_step']:.3f} {fit}", flush=True)


if __name__ == "__main__":
    main()
